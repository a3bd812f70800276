// cpp_api.h -- the reference's plugin interface tcnn::cpp (include/tiny-cuda-nn/cpp_api.h:50-115, src/cpp_api.cu:39-167),
// header-only over libtcnn_amd.so's C ABI.  This is what the reference's torch extension (bindings/torch/tinycudann/
// bindings.cpp) and any other tcnn::cpp::Module client compile against; see INTEGRATION.md section 1.
#pragma once

#include "../tcnn_amd.h"
#include "json_select.h"

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>

namespace tcnn { namespace cpp {

using json = tcnn::json;
typedef void* stream_t; // hipStream_t

enum class LogSeverity { Info = TCNN_LOG_INFO, Debug = TCNN_LOG_DEBUG, Warning = TCNN_LOG_WARNING, Error = TCNN_LOG_ERROR, Success = TCNN_LOG_SUCCESS }; // cpp_api.h:52-58
enum class Precision { Fp32 = TCNN_PRECISION_FP32, Fp16 = TCNN_PRECISION_FP16 };                                                                        // cpp_api.h:69-72

namespace detail {
inline void ok(int rc) { if (rc != TCNN_OK) throw std::runtime_error{tcnn_last_error()}; }
}

inline uint32_t batch_size_granularity() { return tcnn_batch_size_granularity(); }
inline int cuda_device() { int d = 0; detail::ok(tcnn_device(&d)); return d; }
inline void set_cuda_device(int device) { detail::ok(tcnn_set_device(device)); }
inline void free_temporary_memory() { tcnn_free_temporary_memory(); }
inline bool has_networks() { return tcnn_has_networks() != 0; }
inline float default_loss_scale(Precision p) { return tcnn_default_loss_scale((int)p); }
inline Precision preferred_precision() { return (Precision)tcnn_preferred_precision(); }

// cpp_api.h:80, cpp_api.cu:61-63 (bound by the torch extension, bindings.cpp:304).  The C ABI takes a function pointer and a user
// pointer; the std::function is kept here.  An empty callback restores the library's default sink (stderr).
namespace detail {
inline std::function<void(LogSeverity, const std::string&)>& log_callback() {
	static std::function<void(LogSeverity, const std::string&)> f;
	return f;
}
inline void log_trampoline(int severity, const char* message, void*) {
	if (log_callback()) log_callback()((LogSeverity)severity, std::string{message ? message : ""});
}
}
inline void set_log_callback(const std::function<void(LogSeverity, const std::string&)>& callback) {
	detail::log_callback() = callback;
	tcnn_set_log_callback(callback ? detail::log_trampoline : nullptr, nullptr);
}

struct Context { // cpp_api.h:82-84
	std::shared_ptr<void> ctx;
};

class Module { // cpp_api.h:86-111: all pointers are device pointers owned by the caller
public:
	explicit Module(tcnn_module_t handle) : m_handle{handle} {}
	Module(const Module&) = delete;
	Module& operator=(const Module&) = delete;
	~Module() { tcnn_module_destroy(m_handle); }

	void inference(stream_t stream, uint32_t n_elements, const float* input, void* output, void* params) { detail::ok(tcnn_module_inference(m_handle, stream, n_elements, input, output, params)); }
	Context forward(stream_t stream, uint32_t n_elements, const float* input, void* output, void* params, bool prepare_input_gradients) {
		tcnn_context_t c = nullptr;
		detail::ok(tcnn_module_forward(m_handle, stream, n_elements, input, output, params, prepare_input_gradients ? 1 : 0, &c));
		return Context{std::shared_ptr<void>{(void*)c, [](void* p) { tcnn_context_destroy((tcnn_context_t)p); }}};
	}
	void backward(stream_t stream, const Context& ctx, uint32_t n_elements, float* dL_dinput, const void* dL_doutput, void* dL_dparams, const float* input, const void* output, const void* params) {
		if (!ctx.ctx) throw std::runtime_error{"Module::backward: called with invalid context. forward likely (mistakenly) ran in inference mode."};
		detail::ok(tcnn_module_backward(m_handle, stream, (tcnn_context_t)ctx.ctx.get(), n_elements, dL_dinput, dL_doutput, dL_dparams, input, output, params));
	}
	void backward_backward_input(stream_t stream, const Context& ctx, uint32_t n_elements, const float* dL_ddLdinput, const float* input, const void* dL_doutput, void* dL_dparams, void* dL_ddLdoutput,
	                             float* dL_dinput, const void* params) {
		detail::ok(tcnn_module_backward_backward_input(m_handle, stream, (tcnn_context_t)ctx.ctx.get(), n_elements, dL_ddLdinput, input, dL_doutput, dL_dparams, dL_ddLdoutput, dL_dinput, params));
	}

	// DifferentiableObject::input_gradient (object.h:342-366; the reference's cpp::Module does not expose it): d_dinput [n_elements][n_input_dims]
	// = d output[dim] / d input with `params`; output (may be nullptr): the forward pass's output.  See tcnn_module_input_gradient.
	void input_gradient(stream_t stream, uint32_t n_elements, uint32_t dim, const float* input, float* d_dinput, void* output, const void* params, float backprop_scale) {
		detail::ok(tcnn_module_input_gradient(m_handle, stream, n_elements, dim, input, d_dinput, output, params, backprop_scale));
	}
	std::string last_input_gradient_route() const { return tcnn_module_last_input_gradient_route(m_handle); } // "none" | "two-pass" | the fused kernel's name
	// input_gradient for n_dims output columns from one forward pass: jacobian [n_elements][n_dims][n_input_dims], rows [:, k, :] bit for bit
	// input_gradient(dim = dims[k]).  dims is a host array.  See tcnn_module_input_jacobian.
	void input_jacobian(stream_t stream, uint32_t n_elements, const uint32_t* dims, uint32_t n_dims, const float* input, float* jacobian, void* output, const void* params, float backprop_scale) {
		detail::ok(tcnn_module_input_jacobian(m_handle, stream, n_elements, dims, n_dims, input, jacobian, output, params, backprop_scale));
	}
	std::string last_input_jacobian_route() const { return tcnn_module_last_input_jacobian_route(m_handle); } // "none" | "two-pass" | the fused kernel's name
	// forward mode: jvp [n_elements][n_tangents][n_output_dims()] in output_precision(), jvp[:, t, :] = J(x) tangents[:, t, :] for tangents
	// [n_elements][n_tangents][n_input_dims()] floats; output may be null.  No backprop_scale (linear in the tangent).  See tcnn_module_input_jvp.
	void input_jvp(stream_t stream, uint32_t n_elements, uint32_t n_tangents, const float* input, const float* tangents, void* jvp, void* output, const void* params) {
		detail::ok(tcnn_module_input_jvp(m_handle, stream, n_elements, n_tangents, input, tangents, jvp, output, params));
	}
	std::string last_input_jvp_route() const { return tcnn_module_last_input_jvp_route(m_handle); } // "none" | "two-pass" | the fused kernel's name
	// Training through input_jvp: input_jvp_fwd is input_jvp (the same bits in jvp and output) and returns the context input_jvp_bwd takes.
	// input_jvp_bwd: the gradients of sum_t <dL_djvp[:, t, :], J v_t> + <dL_doutput, f(x)> -- dL_dparams under gradient_mode (TCNN_GRADIENT_*), dL_dinput
	// [n_elements][n_input_dims()], dL_dtangents [n_elements][n_tangents][n_input_dims()]; dL_doutput and every result may be null.  No loss
	// scale inside.  See tcnn_module_input_jvp_forward / _backward.
	Context input_jvp_fwd(stream_t stream, uint32_t n_elements, uint32_t n_tangents, const float* input, const float* tangents, void* jvp, void* output, const void* params) {
		tcnn_context_t c = nullptr;
		detail::ok(tcnn_module_input_jvp_forward(m_handle, stream, n_elements, n_tangents, input, tangents, jvp, output, params, &c));
		return Context{std::shared_ptr<void>{(void*)c, [](void* p) { tcnn_context_destroy((tcnn_context_t)p); }}};
	}
	void input_jvp_bwd(stream_t stream, const Context& ctx, uint32_t n_elements, uint32_t n_tangents, const float* input, const float* tangents, const void* dL_djvp, const void* dL_doutput,
	                   const void* params, void* dL_dparams, float* dL_dinput, float* dL_dtangents, int gradient_mode = TCNN_GRADIENT_OVERWRITE) {
		if (!ctx.ctx) throw std::runtime_error{"Module::bwd: called with invalid context. fwd likely (mistakenly) ran in inference mode."};
		detail::ok(tcnn_module_input_jvp_backward(m_handle, stream, (tcnn_context_t)ctx.ctx.get(), n_elements, n_tangents, input, tangents, dL_djvp, dL_doutput, params, dL_dparams, dL_dinput,
		                                          dL_dtangents, dL_dparams ? gradient_mode : TCNN_GRADIENT_IGNORE));
	}
	std::string last_input_jvp_backward_route() const { return tcnn_module_last_input_jvp_backward_route(m_handle); } // "none" | "two-pass"

	uint32_t n_input_dims() const { return tcnn_module_n_input_dims(m_handle); }
	uint32_t n_output_dims() const { return tcnn_module_n_output_dims(m_handle); } // padded width, cpp_api.cu:130
	size_t n_params() const { return tcnn_module_n_params(m_handle); }
	Precision param_precision() const { return (Precision)tcnn_module_param_precision(m_handle); }
	Precision output_precision() const { return (Precision)tcnn_module_output_precision(m_handle); }
	void initialize_params(size_t seed, float* params_full_precision, float scale = 1.0f) { detail::ok(tcnn_module_initialize_params(m_handle, seed, params_full_precision, scale)); }
	json hyperparams() const { return json::parse(tcnn_module_hyperparams(m_handle)); }
	std::string name() const { return tcnn_module_name(m_handle); }
	tcnn_module_t handle() const { return m_handle; }

private:
	tcnn_module_t m_handle;
};

// caller owns the result (the reference's bindings wrap it in a unique_ptr, bindings.cpp:265)
inline Module* create_network_with_input_encoding(uint32_t n_input_dims, uint32_t n_output_dims, const json& encoding, const json& network) {
	tcnn_module_t h = nullptr;
	detail::ok(tcnn_create_network_with_input_encoding(n_input_dims, n_output_dims, encoding.dump().c_str(), network.dump().c_str(), &h));
	return new Module{h};
}
inline Module* create_network(uint32_t n_input_dims, uint32_t n_output_dims, const json& network) {
	tcnn_module_t h = nullptr;
	detail::ok(tcnn_create_network(n_input_dims, n_output_dims, network.dump().c_str(), &h));
	return new Module{h};
}
inline Module* create_encoding(uint32_t n_input_dims, const json& encoding, Precision requested_precision) {
	tcnn_module_t h = nullptr;
	detail::ok(tcnn_create_encoding(n_input_dims, encoding.dump().c_str(), (int)requested_precision, &h));
	return new Module{h};
}

}} // namespace tcnn::cpp
