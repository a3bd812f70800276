// input_jvp_api.cpp -- input_jvp (every output's derivative along given input directions, forward mode) through the C++ headers, with a
// plain C++14 compiler: tcnn::cpp::Module::input_jvp / last_input_jvp_route (cpp_api.h) and tcnn::NetworkWithInputEncoding<T>::input_jvp
// (tcnn_api.h).  Host checks only -- modules are made without a device, and every error here is reported before anything is allocated or
// launched; what the routes compute is tests/test_input_jvp_gpu.py's.
#include <tiny-cuda-nn/config.h>
#include <tiny-cuda-nn/cpp_api.h>

#include <cstdio>
#include <memory>
#include <string>

using namespace tcnn;

#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

template <typename F>
static std::string message_of(F&& f) {
	try {
		f();
	} catch (const std::exception& e) {
		return e.what();
	}
	return "";
}

static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static int host_checks() {
	const json encoding = {{"otype", "HashGrid"}, {"n_levels", 4}, {"n_features_per_level", 2}, {"log2_hashmap_size", 10}, {"base_resolution", 4}, {"per_level_scale", 2.0}};
	const json network = {{"otype", "FullyFusedMLP"}, {"activation", "ReLU"}, {"output_activation", "None"}, {"n_neurons", 64}, {"n_hidden_layers", 2}};
	float input[4] = {}, tangents[4] = {};
	unsigned short jvp[4] = {};

	std::unique_ptr<cpp::Module> module{cpp::create_network_with_input_encoding(3, 17, encoding, network)};
	REQUIRE(module->n_output_dims() == 32);
	REQUIRE(module->last_input_jvp_route() == "none");
	REQUIRE(has(message_of([&] { module->input_jvp(nullptr, 256, 3, input, nullptr, jvp, nullptr, input); }), "tangents"));
	REQUIRE(has(message_of([&] { module->input_jvp(nullptr, 256, 3, input, tangents, nullptr, nullptr, input); }), "jvp"));
	REQUIRE(has(message_of([&] { module->input_jvp(nullptr, 256, 0, input, tangents, jvp, nullptr, input); }), "n_tangents"));
	REQUIRE(has(message_of([&] { module->input_jvp(nullptr, 300, 3, input, tangents, jvp, nullptr, input); }), "BATCH_SIZE_GRANULARITY"));
	REQUIRE(module->last_input_jvp_route() == "none"); // a refused call is no call
	REQUIRE(module->last_input_gradient_route() == "none");
	REQUIRE(module->last_input_jacobian_route() == "none");

	// a module without a tangent: PPNG1 alone, and a Composite that holds one beside a OneBlob (which has a tangent)
	const json ppng = {{"otype", "PPNG1"}, {"n_frequencies", 2}, {"n_quants", 8}, {"n_features", 2}, {"rank", 2}};
	std::unique_ptr<cpp::Module> no_tangent{cpp::create_encoding(3, ppng, cpp::Precision::Fp16)};
	REQUIRE(message_of([&] { no_tangent->input_jvp(nullptr, 256, 1, input, tangents, jvp, nullptr, input); }) == "input_jvp: not implemented for PPNG1");
	const json composite = json::parse(R"({"otype": "Composite", "nested": [{"otype": "OneBlob", "n_bins": 16, "n_dims_to_encode": 2},
		{"otype": "PPNG1", "n_frequencies": 2, "n_quants": 8, "n_features": 2, "rank": 2, "n_dims_to_encode": 3}]})");
	std::unique_ptr<cpp::Module> mixed{cpp::create_encoding(5, composite, cpp::Precision::Fp16)};
	REQUIRE(message_of([&] { mixed->input_jvp(nullptr, 256, 2, input, tangents, jvp, nullptr, input); }) == "input_jvp: not implemented for Composite");
	REQUIRE(mixed->last_input_jvp_route() == "none");

	// the C ABI's NULL handles
	REQUIRE(tcnn_module_input_jvp(nullptr, nullptr, 256, 1, input, tangents, jvp, nullptr, input) == TCNN_ERROR && std::string{tcnn_last_error()} != "");
	REQUIRE(tcnn_trainer_input_jvp(nullptr, nullptr, 256, 1, input, tangents, jvp) == TCNN_ERROR && std::string{tcnn_last_error()} != "");
	REQUIRE(tcnn_module_last_input_jvp_route(nullptr) == nullptr && std::string{tcnn_last_error()} != "");

	// NetworkWithInputEncoding<T>: needs a bound Trainer, as inference does; the result is in the network's precision T
	NetworkWithInputEncoding<network_precision_t> unbound{3, 17, encoding, network};
	GPUMatrix<float> x(input, 3, 256), v(tangents, 9, 256);
	GPUMatrix<network_precision_t> out((network_precision_t*)jvp, 3 * 32, 256);
	REQUIRE(has(message_of([&] { unbound.input_jvp(nullptr, 3, x, v, out); }), "construct a Trainer first"));
	void (NetworkWithInputEncoding<float>::*fp32_method)(stream_t, uint32_t, const GPUMatrix<float>&, const GPUMatrix<float>&, GPUMatrix<float>&) = &NetworkWithInputEncoding<float>::input_jvp;
	REQUIRE(fp32_method != nullptr);
	std::printf("host checks ok\n");
	return 0;
}

int main() {
	try {
		return host_checks();
	} catch (const std::exception& e) {
		std::printf("FAILED with exception: %s\n", e.what());
		return 1;
	}
}
