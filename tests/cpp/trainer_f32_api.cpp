// Full-precision training through the header API (include/tiny-cuda-nn/tcnn_api.h): create_from_config_as<float> is the reference's
// build without TCNN_HALF_PRECISION -- Trainer<float, float, float>, Loss<float>, Optimizer<float> -- with ONE float parameter vector,
// float ForwardContext matrices and an Optimizer<float> that a caller can also step on its own.  `--no-gpu`: the host-side checks only
// (types, and the configuration errors that need no device).
#include <tiny-cuda-nn/config.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

using namespace tcnn;

typedef Trainer<float, float, float> trainer_f32_t;
static_assert(std::is_same<decltype(std::declval<trainer_f32_t::ForwardContext>().output()), const float*>::value, "ForwardContext::output() of an fp32 trainer is const float*");
static_assert(std::is_same<decltype(std::declval<trainer_f32_t::ForwardContext>().dL_doutput()), const float*>::value, "ForwardContext::dL_doutput() of an fp32 trainer is const float*");
static_assert(std::is_same<decltype(std::declval<trainer_f32_t>().params()), float*>::value, "params() of an fp32 trainer is float*");
static_assert(std::is_same<decltype(std::declval<Optimizer<float>>().custom_weights()), float*>::value, "Optimizer<float>::custom_weights() is float*");
static_assert(std::is_same<decltype(TrainableModelT<float>::trainer), std::shared_ptr<trainer_f32_t>>::value, "TrainableModelT<float> holds the fp32 trainer");
static_assert(std::is_same<TrainableModel, TrainableModelT<network_precision_t>>::value, "TrainableModel is the network_precision_t alias");

template <typename F>
static bool throws_with(F&& f, const char* needle) {
	try { f(); } catch (const std::exception& e) { return std::strstr(e.what(), needle) != nullptr; }
	return false;
}

// configuration A: Frequency(3, 4 frequencies) -> CutlassMLP 48 x 2 Tanh -> 3 outputs, L2, Adam
static json config_a(const char* network_otype = "CutlassMLP") {
	return json{
		{"loss", {{"otype", "L2"}}},
		{"optimizer", {{"otype", "Adam"}, {"learning_rate", 1e-2}, {"beta1", 0.9f}, {"beta2", 0.99f}, {"epsilon", 1e-8}, {"l2_reg", 1e-6}}},
		{"encoding", {{"otype", "Frequency"}, {"n_frequencies", 4}}},
		{"network", {{"otype", network_otype}, {"activation", "Tanh"}, {"output_activation", "None"}, {"n_neurons", 48}, {"n_hidden_layers", 2}}},
	};
}

static int host_checks() {
	// reported before anything is allocated on a device
	REQUIRE(throws_with([] { create_from_config_as<float>(3, 3, config_a("FullyFusedMLP")); }, "FullyFusedMLP can only be used if the network precision is set to __half."));
	tcnn_trainer_t t = nullptr;
	REQUIRE(tcnn_create_from_config_precision(3, 3, config_a().dump().c_str(), 1337, 7, &t) == TCNN_ERROR && std::strstr(tcnn_last_error(), "Unknown precision") != nullptr);
	Optimizer<float> bad{json{{"otype", "Shampoo"}}};
	REQUIRE(throws_with([&] { bad.allocate(16); }, "Invalid optimizer type: Shampoo"));
	tcnn_optimizer_t o = nullptr;
	REQUIRE(tcnn_optimizer_create_precision("{\"otype\": \"Adam\"}", 16, nullptr, 0, 7, &o) == TCNN_ERROR && std::strstr(tcnn_last_error(), "Unknown precision") != nullptr);
	REQUIRE(tcnn_default_loss_scale(TCNN_PRECISION_FP32) == 1.0f && tcnn_preferred_precision() == TCNN_PRECISION_FP16);
	std::printf("host checks ok\n");
	return 0;
}

static int gpu_checks() {
	const uint32_t n_in = 3, n_out = 3, batch = 512;
	auto model = create_from_config_as<float>(n_in, n_out, config_a());
	auto trainer = model.trainer;
	REQUIRE(tcnn_trainer_precision(trainer->handle()) == TCNN_PRECISION_FP32);
	const size_t n_params = trainer->n_params();
	REQUIRE(n_params == 48u * 32u + 48u * 48u + 16u * 48u); // Frequency(3, 4): 24 features padded to 32
	REQUIRE(trainer->params() == trainer->params_full_precision() && trainer->params_inference() == trainer->params());
	REQUIRE((void*)trainer->param_gradients() != (void*)trainer->params());

	std::vector<float> xs((size_t)batch * n_in), ts((size_t)batch * n_out);
	uint32_t state = 12345;
	auto rnd = [&] { state = state * 1664525u + 1013904223u; return (state >> 8) * (1.0f / 16777216.0f); };
	for (uint32_t i = 0; i < batch; ++i) {
		const float x = rnd(), y = rnd(), z = rnd();
		xs[3 * i] = x; xs[3 * i + 1] = y; xs[3 * i + 2] = z;
		ts[3 * i] = std::sin(3 * x) * z; ts[3 * i + 1] = x * y; ts[3 * i + 2] = std::cos(2 * y);
	}
	GPUMatrix<float> input(n_in, batch), target(n_out, batch), prediction(n_out, batch);
	tcnn_gpu_memcpy(input.data(), xs.data(), xs.size() * sizeof(float), TCNN_MEMCPY_HOST_TO_DEVICE);
	tcnn_gpu_memcpy(target.data(), ts.data(), ts.size() * sizeof(float), TCNN_MEMCPY_HOST_TO_DEVICE);

	float first = 0, last = 0;
	for (uint32_t i = 0; i < 10; ++i) {
		auto ctx = trainer->training_step(nullptr, input, target);
		if (i == 0 || i == 9) (i == 0 ? first : last) = trainer->loss(nullptr, *ctx);
		if (i == 0) {
			// float context matrices: [n][16]; the padding columns of dL_doutput are zeros and the live ones are 2 (out - target) / n_total
			const float* out = ctx->output();
			const float* dy = ctx->dL_doutput();
			REQUIRE(ctx->padded_output_width == 16 && out != nullptr && dy != nullptr);
			std::vector<float> o(16), d(16);
			tcnn_stream_synchronize(nullptr);
			tcnn_gpu_memcpy(o.data(), out, 16 * sizeof(float), TCNN_MEMCPY_DEVICE_TO_HOST);
			tcnn_gpu_memcpy(d.data(), dy, 16 * sizeof(float), TCNN_MEMCPY_DEVICE_TO_HOST);
			for (int j = 0; j < 3; ++j) REQUIRE(d[j] == (2 * (o[j] - ts[j])) / (float)(batch * n_out)); // loss scale 1: the gradient is not scaled
			for (int j = 3; j < 16; ++j) REQUIRE(d[j] == 0.0f);
		}
	}
	std::printf("fp32 loss %g -> %g after 10 steps (%s)\n", first, last, tcnn_trainer_last_step_kernel(trainer->handle()));
	REQUIRE(std::isfinite(first) && std::isfinite(last) && last < first);
	REQUIRE(trainer->optimizer_step_count() == 10 && std::string{tcnn_trainer_last_step_kernel(trainer->handle())} == "unfused");

	// snapshot round trip through MessagePack: float parameters, and a second trainer restored from it infers the same
	model.network->inference(nullptr, input, prediction);
	tcnn_stream_synchronize(nullptr);
	const std::vector<float> p = prediction.to_cpu_vector();
	{
		const json snap = trainer->serialize(true);
		REQUIRE(snap.value("params_type", "") == "float" && snap["params_binary"].get_binary().size() == 4 * n_params);
		REQUIRE(snap["optimizer"].value("current_step", 0u) == 10u);
		auto other = create_from_config_as<float>(n_in, n_out, config_a());
		other.trainer->deserialize(json::from_msgpack(json::to_msgpack(snap)));
		GPUMatrix<float> again(n_out, batch);
		other.network->inference(nullptr, input, again);
		tcnn_stream_synchronize(nullptr);
		REQUIRE(again.to_cpu_vector() == p && other.trainer->optimizer_step_count() == 10);
		std::vector<float> a(n_params), b(n_params);
		tcnn_gpu_memcpy(a.data(), trainer->params(), 4 * n_params, TCNN_MEMCPY_DEVICE_TO_HOST);
		tcnn_gpu_memcpy(b.data(), other.trainer->params(), 4 * n_params, TCNN_MEMCPY_DEVICE_TO_HOST);
		REQUIRE(std::memcmp(a.data(), b.data(), 4 * n_params) == 0);
	}

	// Optimizer<float> on its own: ONE weight vector (1003 weights: a ragged last quad), fp32 gradients; the master weights are the bits the
	// half-weight optimizer leaves when it is given the same fp32 gradients
	{
		const json adam = {{"otype", "Ema"}, {"decay", 0.9f}, {"nested", {{"otype", "Adam"}, {"learning_rate", 1e-2}, {"beta1", 0.9f}, {"beta2", 0.99f}, {"epsilon", 1e-15}, {"l2_reg", 1e-4}}}};
		const std::vector<std::pair<uint32_t, uint32_t>> layers = {{16, 16}, {16, 8}};
		const size_t n = 1003;
		Optimizer<float> opt32{adam};
		Optimizer<half> opt16{adam};
		opt32.allocate(n, layers);
		opt16.allocate(n, layers);
		REQUIRE(tcnn_optimizer_weight_precision(opt32.handle()) == TCNN_PRECISION_FP32 && tcnn_optimizer_weight_precision(opt16.handle()) == TCNN_PRECISION_FP16);
		std::vector<float> w(n), g(n);
		for (size_t i = 0; i < n; ++i) w[i] = ((float)((i * 37) % 129) - 64.0f) / 256.0f + 1.0f / 1024.0f;
		GPUMemory<float> w32, w16_fp, g_dev(n);
		GPUMemory<half> w16(n);
		w32.resize_and_copy_from_host(w);
		w16_fp.resize_and_copy_from_host(w);
		w16.memset(0);
		for (int step = 0; step < 3; ++step) {
			for (size_t i = 0; i < n; ++i) {
				g[i] = ((float)((i * 53 + (size_t)step * 17) % 97) - 48.0f) / 509.0f;
				if (i >= 384 && (i + (size_t)step) % 3 == 0) g[i] = 0.0f;
			}
			g_dev.copy_from_host(g);
			opt32.step(nullptr, 1.0f, w32.data(), step == 0 ? nullptr : w32.data(), g_dev.data()); // weights: null, or the master vector itself
			opt16.step(nullptr, 1.0f, w16_fp.data(), w16.data(), g_dev.data());
		}
		tcnn_stream_synchronize(nullptr);
		std::vector<float> a, b;
		w32.copy_to_host(a);
		w16_fp.copy_to_host(b);
		REQUIRE(opt32.step() == 3 && std::memcmp(a.data(), b.data(), 4 * n) == 0 && a[0] != w[0] && a[n - 1] != w[n - 1]);
		REQUIRE(opt32.custom_weights() != nullptr && opt32.serialize()["weights_ema_binary"].get_binary().size() == 4 * n);
		GPUMemory<float> elsewhere(n);
		REQUIRE(throws_with([&] { opt32.step(nullptr, 1.0f, w32.data(), elsewhere.data(), g_dev.data()); }, "one weight vector"));
		REQUIRE(throws_with([&] { opt32.deserialize(opt16.serialize()); }, "wrong size")); // half EMA weights are never reinterpreted as floats
	}
	free_all_gpu_memory_arenas();
	std::printf("gpu checks ok\n");
	return 0;
}

int main(int argc, char** argv) {
	try {
		if (host_checks()) return 1;
		if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return 0;
		return gpu_checks();
	} catch (const std::exception& e) {
		std::printf("exception: %s\n", e.what());
		return 2;
	}
}
