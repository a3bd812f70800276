// grid_nd_api.cpp -- grids of 1, 5, 6 and 7 input dimensions through the C++ header API and the C ABI, compiled with plain g++ and linked
// with -ltcnn_amd (tests/test_grid_nd_host.py, tests/test_grid_nd_surfaces.py).
//   grid_nd_api --no-gpu '<encoding json>'
//       per dims in 0 .. 8 and precision: "dims <d> fp16|fp32 n_params <n> width <padded output width>", or "dims <d> ... error <message>"
//       -- also through the network-with-input-encoding factories for the dimensions a grid takes (a trainer allocates on the GPU: not here)
//   grid_nd_api <dims> '<encoding json>' <in.bin> <out.bin>
//       in.bin: uint32 n, then x float [n][dims], then the parameters as half bits [n_params].  Creates the encoding through the C ABI and
//       through the header API, runs inference with each, destroys both and writes the two outputs, half bits [n][width] each, to out.bin.
#include <tiny-cuda-nn/common.h>
#include <tiny-cuda-nn/cpp_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace tcnn;

#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED: %s (line %d): %s\n", #x, __LINE__, tcnn_last_error()); return 1; } } while (0)

static int host(const char* text) {
	const json encoding = json::parse(text);
	const json network = {{"otype", "FullyFusedMLP"}, {"activation", "ReLU"}, {"output_activation", "None"}, {"n_neurons", 64}, {"n_hidden_layers", 2}};
	for (uint32_t dims = 0; dims <= 8; ++dims) {
		for (int fp32 = 0; fp32 < 2; ++fp32) {
			std::printf("dims %u %s ", dims, fp32 ? "fp32" : "fp16");
			try {
				std::unique_ptr<cpp::Module> m{cpp::create_encoding(dims, encoding, fp32 ? cpp::Precision::Fp32 : cpp::Precision::Fp16)};
				std::printf("n_params %zu width %u\n", m->n_params(), m->n_output_dims());
			} catch (const std::runtime_error& e) {
				std::printf("error %s\n", e.what());
			}
		}
		if (dims < 1 || dims > 7) continue;
		// the other factories take such a grid too
		std::unique_ptr<cpp::Module> plain{cpp::create_encoding(dims, encoding, cpp::Precision::Fp16)};
		std::unique_ptr<cpp::Module> with_network{cpp::create_network_with_input_encoding(dims, 3, encoding, network)};
		REQUIRE(with_network->n_input_dims() == dims && with_network->n_params() > plain->n_params());
		tcnn_module_t h = nullptr;
		REQUIRE(tcnn_create_network_with_input_encoding_precision(dims, 3, encoding.dump().c_str(), json{{"otype", "CutlassMLP"}, {"n_neurons", 32}, {"n_hidden_layers", 1}}.dump().c_str(), TCNN_PRECISION_FP32, &h) == TCNN_OK);
		tcnn_module_destroy(h);
	}
	std::printf("host checks ok\n");
	return 0;
}

int main(int argc, char** argv) {
	if (argc == 3 && !std::strcmp(argv[1], "--no-gpu")) return host(argv[2]);
	if (argc != 5) return 2;
	const uint32_t dims = (uint32_t)std::atoi(argv[1]);
	const json encoding = json::parse(argv[2]);
	FILE* in = std::fopen(argv[3], "rb");
	REQUIRE(in != nullptr);
	uint32_t n = 0;
	REQUIRE(std::fread(&n, 4, 1, in) == 1 && n % BATCH_SIZE_GRANULARITY == 0);
	std::vector<float> x((size_t)n * dims);
	REQUIRE(std::fread(x.data(), 4, x.size(), in) == x.size());

	tcnn_module_t c_module = nullptr;
	REQUIRE(tcnn_create_encoding(dims, encoding.dump().c_str(), TCNN_PRECISION_FP16, &c_module) == TCNN_OK);
	std::unique_ptr<cpp::Module> module{cpp::create_encoding(dims, encoding, cpp::Precision::Fp16)};
	const size_t n_params = tcnn_module_n_params(c_module);
	const uint32_t width = tcnn_module_n_output_dims(c_module);
	REQUIRE(module->n_params() == n_params && module->n_output_dims() == width && module->n_input_dims() == dims);
	std::vector<uint16_t> params(n_params);
	REQUIRE(std::fread(params.data(), 2, n_params, in) == n_params);
	std::fclose(in);

	void *d_x = nullptr, *d_params = nullptr, *d_out = nullptr;
	REQUIRE(tcnn_gpu_malloc(x.size() * 4, &d_x) == TCNN_OK && tcnn_gpu_malloc(n_params * 2, &d_params) == TCNN_OK && tcnn_gpu_malloc((size_t)n * width * 2, &d_out) == TCNN_OK);
	REQUIRE(tcnn_gpu_memcpy(d_x, x.data(), x.size() * 4, TCNN_MEMCPY_HOST_TO_DEVICE) == TCNN_OK);
	REQUIRE(tcnn_gpu_memcpy(d_params, params.data(), n_params * 2, TCNN_MEMCPY_HOST_TO_DEVICE) == TCNN_OK);
	std::vector<uint16_t> out((size_t)n * width * 2);
	REQUIRE(tcnn_module_inference(c_module, nullptr, n, (const float*)d_x, d_out, d_params) == TCNN_OK);
	REQUIRE(tcnn_stream_synchronize(nullptr) == TCNN_OK);
	REQUIRE(tcnn_gpu_memcpy(out.data(), d_out, (size_t)n * width * 2, TCNN_MEMCPY_DEVICE_TO_HOST) == TCNN_OK);
	tcnn_module_destroy(c_module);
	REQUIRE(tcnn_gpu_memset(d_out, 0xff, (size_t)n * width * 2) == TCNN_OK);
	module->inference(nullptr, n, (const float*)d_x, d_out, d_params);
	REQUIRE(tcnn_stream_synchronize(nullptr) == TCNN_OK);
	REQUIRE(tcnn_gpu_memcpy(out.data() + (size_t)n * width, d_out, (size_t)n * width * 2, TCNN_MEMCPY_DEVICE_TO_HOST) == TCNN_OK);
	module.reset();
	REQUIRE(tcnn_gpu_free(d_x) == TCNN_OK && tcnn_gpu_free(d_params) == TCNN_OK && tcnn_gpu_free(d_out) == TCNN_OK);

	FILE* f = std::fopen(argv[4], "wb");
	REQUIRE(f != nullptr && std::fwrite(&width, 4, 1, f) == 1 && std::fwrite(out.data(), 2, out.size(), f) == out.size());
	std::fclose(f);
	std::printf("gpu checks ok\n");
	return 0;
}
