// input_jvp_backward_api.cpp -- training through input_jvp through the C++ headers, with a plain C++14 compiler:
// tcnn::cpp::Module::input_jvp_fwd / input_jvp_bwd / last_input_jvp_backward_route (cpp_api.h) and
// tcnn::NetworkWithInputEncoding<T>::input_jvp_forward / input_jvp_backward (tcnn_api.h).  Host checks only -- modules are made without a
// device, contexts come from calls on an empty batch, and every error here is reported before anything is allocated or launched; what the
// routes compute is tests/test_input_jvp_backward_gpu.py's.
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
	float input[4] = {}, tangents[4] = {}, d_input[4] = {}, d_tangents[4] = {};
	unsigned short jvp[4] = {}, d_jvp[4] = {}, d_params[4] = {};

	std::unique_ptr<cpp::Module> module{cpp::create_network_with_input_encoding(3, 17, encoding, network)};
	REQUIRE(module->last_input_jvp_backward_route() == "none");
	// the forward call refuses what input_jvp refuses, and leaves no context
	REQUIRE(has(message_of([&] { module->input_jvp_fwd(nullptr, 256, 3, input, nullptr, jvp, nullptr, input); }), "tangents"));
	REQUIRE(has(message_of([&] { module->input_jvp_fwd(nullptr, 256, 3, input, tangents, nullptr, nullptr, input); }), "jvp"));
	REQUIRE(has(message_of([&] { module->input_jvp_fwd(nullptr, 256, 0, input, tangents, jvp, nullptr, input); }), "n_tangents"));
	REQUIRE(has(message_of([&] { module->input_jvp_fwd(nullptr, 300, 3, input, tangents, jvp, nullptr, input); }), "BATCH_SIZE_GRANULARITY"));

	const cpp::Context ctx = module->input_jvp_fwd(nullptr, 0, 3, nullptr, tangents, jvp, nullptr, nullptr); // an empty batch: nothing runs
	REQUIRE(ctx.ctx != nullptr);
	REQUIRE(has(message_of([&] { module->input_jvp_bwd(nullptr, ctx, 256, 3, input, nullptr, d_jvp, nullptr, input, d_params, d_input, d_tangents); }), "tangents"));
	REQUIRE(has(message_of([&] { module->input_jvp_bwd(nullptr, ctx, 256, 3, input, tangents, nullptr, nullptr, input, d_params, d_input, d_tangents); }), "dL_djvp"));
	REQUIRE(has(message_of([&] { module->input_jvp_bwd(nullptr, ctx, 256, 0, input, tangents, d_jvp, nullptr, input, d_params, d_input, d_tangents); }), "n_tangents"));
	REQUIRE(has(message_of([&] { module->input_jvp_bwd(nullptr, ctx, 300, 3, input, tangents, d_jvp, nullptr, input, d_params, d_input, d_tangents); }), "BATCH_SIZE_GRANULARITY"));
	REQUIRE(has(message_of([&] { module->input_jvp_bwd(nullptr, ctx, 256, 3, input, tangents, d_jvp, nullptr, input, d_params, d_input, d_tangents); }), "context"));
	REQUIRE(has(message_of([&] { module->input_jvp_bwd(nullptr, cpp::Context{}, 0, 3, input, tangents, d_jvp, nullptr, input, d_params, d_input, d_tangents); }), "invalid context"));
	// a context of forward() is of another call kind; and backward() takes none of input_jvp_fwd
	const cpp::Context forward_ctx = module->forward(nullptr, 0, nullptr, nullptr, nullptr, true);
	REQUIRE(message_of([&] { module->input_jvp_bwd(nullptr, forward_ctx, 0, 3, input, tangents, d_jvp, nullptr, input, d_params, d_input, d_tangents); }) ==
	        "Module::bwd: called with invalid context. fwd likely (mistakenly) ran in inference mode.");
	REQUIRE(message_of([&] { module->backward(nullptr, ctx, 0, d_input, d_jvp, d_params, input, jvp, input); }) ==
	        "Module::bwd: called with invalid context. fwd likely (mistakenly) ran in inference mode.");
	module->input_jvp_bwd(nullptr, ctx, 0, 3, nullptr, tangents, d_jvp, nullptr, nullptr, d_params, d_input, d_tangents, TCNN_GRADIENT_ACCUMULATE); // an empty batch is no work
	REQUIRE(module->last_input_jvp_backward_route() == "none"); // a refused call is no call
	REQUIRE(module->last_input_jvp_route() == "none");

	// OneBlob: a tangent, but no derivative of it by x -- dL_dinput is refused, the other two are served; its second-order pass stays refused
	const json oneblob = {{"otype", "OneBlob"}, {"n_bins", 16}};
	std::unique_ptr<cpp::Module> blob{cpp::create_network_with_input_encoding(3, 3, oneblob, network)};
	const cpp::Context blob_ctx = blob->input_jvp_fwd(nullptr, 0, 1, nullptr, tangents, jvp, nullptr, nullptr);
	REQUIRE(message_of([&] { blob->input_jvp_bwd(nullptr, blob_ctx, 0, 1, input, tangents, d_jvp, nullptr, input, d_params, d_input, d_tangents); }) ==
	        "input_jvp_backward: dL_dinput not implemented for NetworkWithInputEncoding");
	blob->input_jvp_bwd(nullptr, blob_ctx, 0, 1, nullptr, tangents, d_jvp, nullptr, nullptr, d_params, nullptr, d_tangents);
	const cpp::Context blob_forward = blob->forward(nullptr, 0, nullptr, nullptr, nullptr, true);
	REQUIRE(has(message_of([&] { blob->backward_backward_input(nullptr, blob_forward, 256, input, input, d_jvp, d_params, nullptr, d_input, input); }), "not implemented error"));

	// a module without a tangent
	const json ppng = {{"otype", "PPNG1"}, {"n_frequencies", 2}, {"n_quants", 8}, {"n_features", 2}, {"rank", 2}};
	std::unique_ptr<cpp::Module> no_tangent{cpp::create_encoding(3, ppng, cpp::Precision::Fp16)};
	REQUIRE(message_of([&] { no_tangent->input_jvp_fwd(nullptr, 256, 1, input, tangents, jvp, nullptr, input); }) == "input_jvp: not implemented for PPNG1");
	REQUIRE(message_of([&] { no_tangent->input_jvp_bwd(nullptr, ctx, 256, 3, input, tangents, d_jvp, nullptr, input, d_params, d_input, d_tangents); }) == "input_jvp: not implemented for PPNG1");

	// the C ABI's NULL handles
	tcnn_context_t c = nullptr;
	REQUIRE(tcnn_module_input_jvp_forward(nullptr, nullptr, 256, 1, input, tangents, jvp, nullptr, input, &c) == TCNN_ERROR && std::string{tcnn_last_error()} != "");
	REQUIRE(tcnn_trainer_input_jvp_forward(nullptr, nullptr, 256, 1, input, tangents, jvp, nullptr, &c) == TCNN_ERROR && std::string{tcnn_last_error()} != "");
	REQUIRE(tcnn_trainer_input_jvp_backward(nullptr, nullptr, nullptr, 256, 1, input, tangents, d_jvp, nullptr, d_input, d_tangents, TCNN_GRADIENT_OVERWRITE) == TCNN_ERROR);
	REQUIRE(tcnn_module_last_input_jvp_backward_route(nullptr) == nullptr && std::string{tcnn_last_error()} != "");

	// NetworkWithInputEncoding<T>: needs a bound Trainer, as inference does
	NetworkWithInputEncoding<network_precision_t> unbound{3, 17, encoding, network};
	GPUMatrix<float> x(input, 3, 256), v(tangents, 9, 256), dx(d_input, 3, 256), dv(d_tangents, 9, 256);
	GPUMatrix<network_precision_t> out((network_precision_t*)jvp, 3 * 32, 256), d_out((network_precision_t*)d_jvp, 3 * 32, 256);
	REQUIRE(has(message_of([&] { unbound.input_jvp_forward(nullptr, 3, x, v, out); }), "construct a Trainer first"));
	NetworkWithInputEncoding<network_precision_t>::InputJvpContext none;
	REQUIRE(has(message_of([&] { unbound.input_jvp_backward(nullptr, none, 3, x, v, d_out, nullptr, &dx, &dv, GradientMode::Accumulate); }), "construct a Trainer first"));
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
