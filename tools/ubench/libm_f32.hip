// libm_f32.hip -- the device's bare expf, logf, sinf, cosf and tanhf of a file of floats, compiled like the library (build.py's FLAGS):
// the yardstick of tests/activation_sweep_f32.py allows each of them K_f float steps around the correctly rounded value, and K_f is
// measured here against float64, never against a kernel of the project (tools/libm_f32_ulp.py writes the arguments and reads the results).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-pass-failed -Wno-unused-result -munsafe-fp-atomics -o libm_f32 libm_f32.hip
//   ./libm_f32 arguments.f32 results.f32 [pow_arguments.f32 pow_results.f32]
// results.f32: [5][n] floats -- expf, logf, sinf, cosf, tanhf of the n arguments, in that order.
// pow_arguments.f32: [m][2] floats (base, exponent); pow_results.f32: [m] floats, powf(base, exponent) -- what adam_debias (k_misc.hip) calls.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(call)                                                                                   \
	do {                                                                                              \
		const hipError_t e_ = (call);                                                                 \
		if (e_ != hipSuccess) {                                                                       \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));                \
			return 1;                                                                                 \
		}                                                                                             \
	} while (0)

__global__ void __launch_bounds__(256) k_libm_f32(const uint32_t n, const float* __restrict__ x, float* __restrict__ y) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const float v = x[i];
	y[i] = expf(v);
	y[(size_t)n + i] = logf(v);
	y[(size_t)2 * n + i] = sinf(v);
	y[(size_t)3 * n + i] = cosf(v);
	y[(size_t)4 * n + i] = tanhf(v);
}

__global__ void __launch_bounds__(256) k_powf(const uint32_t m, const float* __restrict__ args, float* __restrict__ y) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < m) y[i] = powf(args[2 * i], args[2 * i + 1]);
}

static int run_powf(const char* in_path, const char* out_path) {
	FILE* f = fopen(in_path, "rb");
	if (!f) {
		perror(in_path);
		return 1;
	}
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	if (bytes <= 0 || bytes % 8 != 0 || bytes / 8 >= (1l << 24)) {
		fprintf(stderr, "%s: expected between 1 and 2^24 pairs of floats\n", in_path);
		return 1;
	}
	const uint32_t m = (uint32_t)(bytes / 8);
	std::vector<float> args((size_t)2 * m), y(m);
	if (fread(args.data(), 4, args.size(), f) != args.size()) {
		fprintf(stderr, "%s: short read\n", in_path);
		return 1;
	}
	fclose(f);
	float *da = nullptr, *dy = nullptr;
	CHECK(hipMalloc(&da, args.size() * 4));
	CHECK(hipMalloc(&dy, (size_t)m * 4));
	CHECK(hipMemcpy(da, args.data(), args.size() * 4, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_powf, dim3((m + 255) / 256), dim3(256), 0, 0, m, da, dy);
	CHECK(hipGetLastError());
	CHECK(hipDeviceSynchronize());
	CHECK(hipMemcpy(y.data(), dy, (size_t)m * 4, hipMemcpyDeviceToHost));
	FILE* o = fopen(out_path, "wb");
	if (!o) {
		perror(out_path);
		return 1;
	}
	if (fwrite(y.data(), 4, y.size(), o) != y.size() || fclose(o) != 0) {
		fprintf(stderr, "%s: short write\n", out_path);
		return 1;
	}
	printf("%u pairs, powf -> %s\n", m, out_path);
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 3 && argc != 5) {
		fprintf(stderr, "usage: %s arguments.f32 results.f32 [pow_arguments.f32 pow_results.f32]\n", argv[0]);
		return 2;
	}
	FILE* f = fopen(argv[1], "rb");
	if (!f) {
		perror(argv[1]);
		return 1;
	}
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	if (bytes <= 0 || bytes % 4 != 0 || bytes / 4 >= (1l << 28)) {
		fprintf(stderr, "%s: expected between 1 and 2^28 floats\n", argv[1]);
		return 1;
	}
	const uint32_t n = (uint32_t)(bytes / 4);
	std::vector<float> x(n), y((size_t)5 * n);
	if (fread(x.data(), 4, n, f) != n) {
		fprintf(stderr, "%s: short read\n", argv[1]);
		return 1;
	}
	fclose(f);
	float *dx = nullptr, *dy = nullptr;
	CHECK(hipMalloc(&dx, (size_t)n * 4));
	CHECK(hipMalloc(&dy, (size_t)5 * n * 4));
	CHECK(hipMemcpy(dx, x.data(), (size_t)n * 4, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_libm_f32, dim3((n + 255) / 256), dim3(256), 0, 0, n, dx, dy);
	CHECK(hipGetLastError());
	CHECK(hipDeviceSynchronize());
	CHECK(hipMemcpy(y.data(), dy, (size_t)5 * n * 4, hipMemcpyDeviceToHost));
	FILE* o = fopen(argv[2], "wb");
	if (!o) {
		perror(argv[2]);
		return 1;
	}
	if (fwrite(y.data(), 4, y.size(), o) != y.size() || fclose(o) != 0) {
		fprintf(stderr, "%s: short write\n", argv[2]);
		return 1;
	}
	printf("%u arguments, 5 functions -> %s\n", n, argv[2]);
	return argc == 5 ? run_powf(argv[3], argv[4]) : 0;
}
