// The header API's tcnn::Optimizer<T> (include/tiny-cuda-nn/tcnn_api.h; optimizer.h of the reference) as a caller with its own gradients
// uses it: allocate / step / serialize on a small parameter vector, compared with the standalone optimizer of the C ABI (tcnn_optimizer_*)
// driven next to it in the same program.  `--no-gpu`: the host-side checks only.
#include <tiny-cuda-nn/optimizer.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

using tcnn::json;

// float -> binary16 bits, round to nearest even (normal and zero values only: all this test uses)
static uint16_t to_half_bits(float f) {
	uint32_t u;
	std::memcpy(&u, &f, 4);
	const uint32_t sign = (u >> 16) & 0x8000u;
	if ((u & 0x7fffffffu) == 0) return (uint16_t)sign;
	const int32_t e = (int32_t)((u >> 23) & 0xffu) - 127 + 15;
	if (e <= 0 || e >= 31) std::abort();
	uint32_t m = u & 0x7fffffu;
	uint32_t h = ((uint32_t)e << 10) | (m >> 13);
	const uint32_t rest = m & 0x1fffu;
	if (rest > 0x1000u || (rest == 0x1000u && (h & 1u))) ++h;
	return (uint16_t)(sign | h);
}

template <typename F>
static bool throws_with(F&& f, const char* needle) {
	try { f(); } catch (const std::exception& e) { return std::strstr(e.what(), needle) != nullptr; }
	return false;
}

struct Vectors {
	tcnn::GPUMemory<float> w_fp;
	tcnn::GPUMemory<tcnn::half> w;
	void init(const std::vector<float>& fp, const std::vector<tcnn::half>& h) { w_fp.resize_and_copy_from_host(fp); w.resize_and_copy_from_host(h); }
	bool equals(const Vectors& o) const {
		std::vector<float> a, b;
		std::vector<tcnn::half> c, d;
		w_fp.copy_to_host(a); o.w_fp.copy_to_host(b); w.copy_to_host(c); o.w.copy_to_host(d);
		return a.size() == b.size() && std::memcmp(a.data(), b.data(), 4 * a.size()) == 0 && c.size() == d.size() && std::memcmp(c.data(), d.data(), 2 * c.size()) == 0;
	}
};

int main(int argc, char** argv) {
	const bool gpu = !(argc > 1 && std::string{argv[1]} == "--no-gpu");
	const json config = {{"otype", "Ema"}, {"decay", 0.9f}, {"nested", {{"otype", "Adam"}, {"learning_rate", 1e-2}, {"beta1", 0.9f}, {"beta2", 0.99f}, {"epsilon", 1e-15}, {"l2_reg", 1e-4}}}};

	// ---- host: configuration before allocate() behaves as it always did; the native entry points need allocate()
	{
		std::unique_ptr<tcnn::Optimizer<tcnn::half>> opt{tcnn::create_optimizer<tcnn::half>(config)};
		REQUIRE(opt->hyperparams().value("otype", "") == "Ema" && opt->n_weights() == 0 && opt->custom_weights() == nullptr);
		opt->update_hyperparams(json{{"otype", "SGD"}});
		REQUIRE(opt->hyperparams().value("otype", "") == "SGD");
		REQUIRE(throws_with([&] { opt->learning_rate(); }, "call allocate() first"));
		REQUIRE(throws_with([&] { opt->step(nullptr, 1.0f, nullptr, nullptr, (const tcnn::half*)nullptr); }, "call allocate() first"));
		tcnn::Optimizer<tcnn::half> bad{json{{"otype", "Shampoo"}}};
		REQUIRE(throws_with([&] { bad.allocate(16); }, "Invalid optimizer type: Shampoo")); // checked before anything touches a device
		tcnn::Optimizer<tcnn::half> composite{json{{"otype", "Composite"}, {"nested", {{"otype", "Adam"}}}}};
		REQUIRE(throws_with([&] { composite.allocate(16); }, "Must provide an array of nested"));
	}
	std::printf("host checks ok\n");
	if (!gpu) return 0;

	// ---- device: 2 weight matrices (384 weights) and 619 further parameters -- 1003 in all, so that the last quad is ragged
	const std::vector<std::pair<uint32_t, uint32_t>> layers = {{16, 16}, {16, 8}};
	const size_t n = 1003, n_matrix = 384;
	std::vector<float> w_fp(n);
	std::vector<tcnn::half> w(n);
	for (size_t i = 0; i < n; ++i) {
		w_fp[i] = ((float)((i * 37) % 129) - 64.0f) / 256.0f + 1.0f / 1024.0f;
		w[i].bits = to_half_bits(w_fp[i]);
	}
	auto gradients = [&](int step, std::vector<tcnn::half>& g_half, std::vector<float>& g_float) {
		g_half.resize(n);
		g_float.resize(n);
		for (size_t i = 0; i < n; ++i) {
			float g = ((float)((i * 53 + (size_t)step * 17) % 97) - 48.0f) / 4.0f; // scaled by 128, a multiple of 1/4: exact in half
			if (i >= n_matrix && (i + (size_t)step) % 3 == 0) g = 0.0f;                    // skipped parameters, and whole skipped quads below
			if (i >= 512 && i < 640) g = 0.0f;
			g_half[i].bits = to_half_bits(g);
			g_float[i] = g / 128.0f;
		}
	};

	tcnn::Optimizer<tcnn::half> from_header{config}, from_header_fp32{config};
	from_header.allocate(n, layers);
	from_header_fp32.allocate(n, layers);
	REQUIRE(from_header.n_weights() == n && from_header.step() == 0 && std::fabs(from_header.learning_rate() - 1e-2f) < 1e-9f);
	REQUIRE(from_header.hyperparams()["nested"].value("otype", "") == "Adam" && from_header.custom_weights() != nullptr);
	const uint32_t flat[4] = {16, 16, 16, 8};
	tcnn_optimizer_t abi = nullptr;
	REQUIRE(tcnn_optimizer_create(config.dump().c_str(), n, flat, 2, &abi) == TCNN_OK);

	Vectors a, b, c;
	a.init(w_fp, w); b.init(w_fp, w); c.init(w_fp, w);
	tcnn::GPUMemory<tcnn::half> g_dev(n);
	tcnn::GPUMemory<float> g32_dev(n);
	std::vector<tcnn::half> g_half;
	std::vector<float> g_float;
	auto one_step = [&](int step) {
		gradients(step, g_half, g_float);
		g_dev.copy_from_host(g_half);
		g32_dev.copy_from_host(g_float);
		from_header.step(nullptr, 128.0f, a.w_fp.data(), a.w.data(), g_dev.data());
		from_header_fp32.step(nullptr, 1.0f, c.w_fp.data(), c.w.data(), g32_dev.data());
		return tcnn_optimizer_step(abi, nullptr, 128.0f, b.w_fp.data(), b.w.data(), g_dev.data(), TCNN_PRECISION_FP16) == TCNN_OK && tcnn_stream_synchronize(nullptr) == TCNN_OK;
	};
	for (int step = 0; step < 3; ++step) REQUIRE(one_step(step));
	REQUIRE(from_header.step() == 3 && tcnn_optimizer_step_count(abi) == 3);
	REQUIRE(a.equals(b));       // the header's optimizer is the C ABI's
	REQUIRE(a.equals(c));       // fp32 gradients (a half times 2^-7, loss scale 1) give the same bits as the half ones at loss scale 128
	{
		std::vector<float> now;
		a.w_fp.copy_to_host(now);
		REQUIRE(now[0] != w_fp[0] && now[n - 1] != w_fp[n - 1]); // the first matrix weight and the ragged tail moved
		for (size_t i = 512; i < 640; ++i) REQUIRE(now[i] == w_fp[i]); // quads without a gradient did not
	}
	// custom weights: the EMA, the same from both
	{
		std::vector<tcnn::half> ema_a(n), ema_b(n);
		REQUIRE(tcnn_gpu_memcpy(ema_a.data(), from_header.custom_weights(), 2 * n, TCNN_MEMCPY_DEVICE_TO_HOST) == TCNN_OK);
		REQUIRE(tcnn_gpu_memcpy(ema_b.data(), tcnn_optimizer_custom_weights(abi), 2 * n, TCNN_MEMCPY_DEVICE_TO_HOST) == TCNN_OK);
		REQUIRE(std::memcmp(ema_a.data(), ema_b.data(), 2 * n) == 0);
	}
	// serialize -> a fresh optimizer -> the same next step; the object is what a Trainer's snapshot holds as "optimizer"
	const json state = from_header.serialize();
	REQUIRE(state.contains("weights_ema_binary") && state["nested"].value("current_step", 0u) == 3u && state["nested"]["first_moments_binary"].get_binary().size() == 4 * n);
	tcnn::Optimizer<tcnn::half> resumed{config};
	resumed.allocate(n, layers);
	resumed.deserialize(state);
	REQUIRE(resumed.step() == 3);
	Vectors d;
	{
		std::vector<float> fp;
		std::vector<tcnn::half> h;
		a.w_fp.copy_to_host(fp); a.w.copy_to_host(h);
		d.init(fp, h);
	}
	from_header.set_learning_rate(5e-3f);
	resumed.set_learning_rate(5e-3f);
	REQUIRE(tcnn_optimizer_set_learning_rate(abi, 5e-3f) == TCNN_OK && std::fabs(tcnn_optimizer_learning_rate(abi) - 5e-3f) < 1e-9f);
	REQUIRE(one_step(3));
	resumed.step(nullptr, 128.0f, d.w_fp.data(), d.w.data(), g_dev.data());
	REQUIRE(tcnn_stream_synchronize(nullptr) == TCNN_OK);
	REQUIRE(a.equals(b) && a.equals(d));
	from_header.update_hyperparams(json{{"nested", {{"beta1", 0.5f}}}});
	REQUIRE(from_header.hyperparams()["nested"].value("beta1", 0.0f) == 0.5f);
	tcnn_optimizer_destroy(abi);
	std::printf("gpu checks ok\n");
	return 0;
}
