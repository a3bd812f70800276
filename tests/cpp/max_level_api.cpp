// max_level_api.cpp -- the grid encodings' max_level through the C++ header API (GridEncoding::set_max_level / max_level /
// set_max_level_gpu / max_level_gpu, grid_interface.h:101-123), which has no encoding object of its own: the four methods sit on
// NetworkWithInputEncoding and reach the Trainer that binds it.
//   max_level_api --no-gpu : a value set before any Trainer binds is held by the network
//   max_level_api          : ... and applied at binding; later settings reach the trainer; a coarse-to-fine schedule trains
#include <tiny-cuda-nn/config.h>
#include <tiny-cuda-nn/cpp_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tcnn;

#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static json config() {
	return {
		{"loss", {{"otype", "L2"}}},
		{"optimizer", {{"otype", "Adam"}, {"learning_rate", 1e-2}, {"beta1", 0.9f}, {"beta2", 0.99f}, {"epsilon", 1e-15}, {"l2_reg", 1e-6}}},
		{"encoding", {{"otype", "HashGrid"}, {"n_levels", 16}, {"n_features_per_level", 2}, {"log2_hashmap_size", 15}, {"base_resolution", 16}, {"per_level_scale", 1.5}}},
		{"network", {{"otype", "FullyFusedMLP"}, {"activation", "ReLU"}, {"output_activation", "None"}, {"n_neurons", 64}, {"n_hidden_layers", 2}}},
	};
}

static int host_checks() {
	const json c = config();
	NetworkWithInputEncoding<network_precision_t> network{2, 3, c["encoding"], c["network"]};
	REQUIRE(network.max_level() == 1000.f && network.max_level_gpu() == nullptr);
	network.set_max_level(0.5f);
	REQUIRE(network.max_level() == 0.5f);
	float dummy[4] = {};
	network.set_max_level_gpu(dummy); // held, never read while no trainer is bound
	REQUIRE(network.max_level_gpu() == dummy);
	network.set_max_level_gpu(nullptr);
	REQUIRE(network.max_level_gpu() == nullptr);
	REQUIRE(network.hyperparams()["encoding"].value("otype", "") == "HashGrid"); // the setting is no hyperparameter
	std::printf("host checks ok\n");
	return 0;
}

static int gpu_checks() {
	const json c = config();
	const uint32_t n = 1 << 14;
	auto network = std::make_shared<NetworkWithInputEncoding<network_precision_t>>(2, 3, c["encoding"], c["network"]);
	network->set_max_level(0.25f); // before binding: held
	auto trainer = std::make_shared<Trainer<float, network_precision_t, network_precision_t>>(network, std::make_shared<Optimizer<network_precision_t>>(c["optimizer"]),
	                                                                                         std::make_shared<Loss<network_precision_t>>(c["loss"]));
	REQUIRE(tcnn_trainer_max_level(trainer->handle()) == 0.25f); // applied at binding
	REQUIRE(network->max_level() == 0.25f);
	network->set_max_level(0.5f);
	REQUIRE(tcnn_trainer_max_level(trainer->handle()) == 0.5f);

	std::vector<float> xs((size_t)n * 2), ts((size_t)n * 3);
	uint32_t state = 777;
	auto rnd = [&] { state = state * 1664525u + 1013904223u; return (state >> 8) * (1.0f / 16777216.0f); };
	for (uint32_t i = 0; i < n; ++i) {
		const float x = rnd(), y = rnd();
		xs[2 * i] = x; xs[2 * i + 1] = y;
		ts[3 * i] = 0.5f + 0.5f * std::sin(6 * x); ts[3 * i + 1] = x * y; ts[3 * i + 2] = 0.5f + 0.5f * std::cos(4 * y);
	}
	GPUMatrix<float> batch(2, n), target(3, n), prediction(3, n);
	tcnn_gpu_memcpy(batch.data(), xs.data(), xs.size() * sizeof(float), TCNN_MEMCPY_HOST_TO_DEVICE);
	tcnn_gpu_memcpy(target.data(), ts.data(), ts.size() * sizeof(float), TCNN_MEMCPY_HOST_TO_DEVICE);

	// per sample: every row keeps half of the levels
	GPUMemory<float> per_sample(n);
	std::vector<float> half(n, 0.5f);
	per_sample.copy_from_host(half);
	network->set_max_level_gpu(per_sample.data());
	REQUIRE(network->max_level_gpu() == per_sample.data());
	auto ctx = trainer->training_step(nullptr, batch, target);
	const float with_array = trainer->loss(nullptr, *ctx);
	network->set_max_level_gpu(nullptr);
	REQUIRE(std::isfinite(with_array));

	// coarse to fine: the cut-off ramps from 0.1 to 1 over 50 steps
	float first = 0, last = 0;
	for (uint32_t i = 0; i < 50; ++i) {
		network->set_max_level(0.1f + 0.9f * (float)i / 49.0f);
		auto step = trainer->training_step(nullptr, batch, target);
		if (i == 0 || i == 49) (i == 0 ? first : last) = trainer->loss(nullptr, *step);
	}
	std::printf("loss %g -> %g over the ramp\n", first, last);
	REQUIRE(std::isfinite(last) && last < first);
	network->inference(nullptr, batch, prediction);
	tcnn_stream_synchronize(nullptr);
	std::printf("gpu checks ok\n");
	return 0;
}

int main(int argc, char** argv) {
	try {
		if (host_checks()) return 1;
		if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return 0;
		return gpu_checks();
	} catch (const std::exception& e) {
		std::printf("FAILED with exception: %s\n", e.what());
		return 1;
	}
}
