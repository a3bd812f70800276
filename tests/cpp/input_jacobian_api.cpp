// input_jacobian_api.cpp -- input_jacobian (input_gradient for several output columns from one forward pass) through the C++ headers, with a
// plain C++14 compiler: tcnn::cpp::Module::input_jacobian / last_input_jacobian_route (cpp_api.h) and
// tcnn::NetworkWithInputEncoding<T>::input_jacobian (tcnn_api.h).  Host checks only -- modules are made without a device, and every error
// here is reported before anything is allocated or launched; what the routes compute is tests/test_input_jacobian_gpu.py's.
#include <tiny-cuda-nn/config.h>
#include <tiny-cuda-nn/cpp_api.h>

#include <cstdio>
#include <memory>
#include <string>
#include <vector>

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

static int host_checks() {
	const json encoding = {{"otype", "HashGrid"}, {"n_levels", 4}, {"n_features_per_level", 2}, {"log2_hashmap_size", 10}, {"base_resolution", 4}, {"per_level_scale", 2.0}};
	const json network = {{"otype", "FullyFusedMLP"}, {"activation", "ReLU"}, {"output_activation", "None"}, {"n_neurons", 64}, {"n_hidden_layers", 2}};
	const std::string invalid_dim = "Invalid dimension to compute the input gradient for.";
	float input[4] = {}, jacobian[4] = {};

	// cpp::Module: 17 outputs are 32 padded columns -- 31 is legal (and would need a device), 32 is not
	std::unique_ptr<cpp::Module> module{cpp::create_network_with_input_encoding(3, 17, encoding, network)};
	REQUIRE(module->n_output_dims() == 32);
	REQUIRE(module->last_input_jacobian_route() == "none");
	const uint32_t good[3] = {31, 0, 31}, bad[3] = {0, 32, 1};
	std::vector<uint32_t> many(33, 0u);
	REQUIRE(message_of([&] { module->input_jacobian(nullptr, 256, bad, 3, input, jacobian, nullptr, input, 128.0f); }) == invalid_dim);
	REQUIRE(message_of([&] { module->input_jacobian(nullptr, 256, good, 0, input, jacobian, nullptr, input, 128.0f); }).find("n_dims") != std::string::npos);
	REQUIRE(message_of([&] { module->input_jacobian(nullptr, 256, many.data(), 33, input, jacobian, nullptr, input, 128.0f); }).find("n_dims") != std::string::npos);
	REQUIRE(message_of([&] { module->input_jacobian(nullptr, 256, nullptr, 3, input, jacobian, nullptr, input, 128.0f); }).find("n_dims") != std::string::npos);
	REQUIRE(message_of([&] { module->input_jacobian(nullptr, 300, good, 3, input, jacobian, nullptr, input, 128.0f); }).find("BATCH_SIZE_GRANULARITY") != std::string::npos);
	REQUIRE(module->last_input_jacobian_route() == "none"); // a refused call is no call
	REQUIRE(module->last_input_gradient_route() == "none");
	std::unique_ptr<cpp::Module> bare{cpp::create_encoding(3, encoding, cpp::Precision::Fp16)};
	const uint32_t past = bare->n_output_dims();
	REQUIRE(message_of([&] { bare->input_jacobian(nullptr, 256, &past, 1, input, jacobian, nullptr, input, 1.0f); }) == invalid_dim);

	// the C ABI's NULL handles
	REQUIRE(tcnn_module_input_jacobian(nullptr, nullptr, 256, good, 3, input, jacobian, nullptr, input, 128.0f) == TCNN_ERROR && std::string{tcnn_last_error()} != "");
	REQUIRE(tcnn_trainer_input_jacobian(nullptr, nullptr, 256, good, 3, input, jacobian, 128.0f) == TCNN_ERROR && std::string{tcnn_last_error()} != "");
	REQUIRE(tcnn_module_last_input_jacobian_route(nullptr) == nullptr && std::string{tcnn_last_error()} != "");

	// NetworkWithInputEncoding<T>: needs a bound Trainer, as inference does; the default backprop_scale is T's loss scale
	NetworkWithInputEncoding<network_precision_t> unbound{3, 17, encoding, network};
	GPUMatrix<float> x(input, 3, 256), jac(jacobian, 9, 256);
	const std::string no_trainer = message_of([&] { unbound.input_jacobian(nullptr, {0, 1, 2}, x, jac); });
	REQUIRE(no_trainer.find("construct a Trainer first") != std::string::npos);
	void (NetworkWithInputEncoding<float>::*fp32_method)(stream_t, const std::vector<uint32_t>&, const GPUMatrix<float>&, GPUMatrix<float>&, float) = &NetworkWithInputEncoding<float>::input_jacobian;
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
