// tcnn_api.h -- the C++ header surface that callers of the reference compile against (samples/mlp_learning_an_image.cu,
// instant-ngp style code), provided over libtcnn_amd.so's C ABI (include/tcnn_amd.h).  Header-only, no HIP or torch types:
// any C++14 compiler, link with -ltcnn_amd.
//
// What is mirrored (reference file:line):
//   tcnn::json                                     nlohmann::json as used by config.h:53 / the samples' config literals (the real one when <json/json.hpp> is on the include path)
//   tcnn::GPUMemory<T>                             gpu_memory.h:60-392   (allocation, host <-> device copies, memset)
//   tcnn::GPUMatrixDynamic<T>, GPUMatrix<T, L>     gpu_matrix.h:115-470  (m x n, column-major by default = [n][m] in memory)
//   tcnn::Loss<T>, create_loss<T>                  loss.h:41-77, src/loss.cu:54-68          (all nine losses; evaluate() on the caller's matrices)
//   tcnn::Optimizer<T>, create_optimizer<T>        optimizer.h:44-95, src/optimizer.cu:50-82 (every optimizer of the library; allocate / step for callers with their own gradients)
//   tcnn::NetworkWithInputEncoding<T>              network_with_input_encoding.h:40-180
//   tcnn::Trainer<T, PARAMS_T, COMPUTE_T>          trainer.h:48-363  (training_step, loss, inference via the network, params)
//   tcnn::TrainableModel, create_from_config       config.h:46-63
//   tcnn::TrainableModelT<T>, create_from_config_as<T>   the same for a chosen precision: <float> is the reference's build without
//                                                  TCNN_HALF_PRECISION (Trainer<float, float, float>, Loss<float>, Optimizer<float>)
//   tcnn::free_all_gpu_memory_arenas               gpu_memory.h:751
// Errors are std::runtime_error carrying the library's message, as in the reference (common_host.h:71-110).
// The objects are thin: a Trainer owns the native trainer handle; the NetworkWithInputEncoding, Loss and Optimizer objects
// carry configuration until a Trainer binds them (the reference's Trainer likewise takes ownership of the parameters,
// trainer.h:322-336).  Like the reference: one GPU per process, not thread-safe.
#pragma once

#include "../tcnn_amd.h"
#include "json_select.h" // tcnn::json: nlohmann::json where <json/json.hpp> is on the include path, else json_lite.h's
#include "random.h" // trainer.h includes random.h in the reference: callers get default_rng_t / generate_random_uniform from config.h

#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace tcnn {

typedef void* stream_t; // hipStream_t (cudaStream_t in the reference)

static constexpr uint32_t BATCH_SIZE_GRANULARITY = 256; // common.h:235

struct half { uint16_t bits; }; // IEEE binary16 storage; arithmetic happens on the device
typedef half network_precision_t; // common.h:86-90 (TCNN_HALF_PRECISION)

enum class MatrixLayout { RowMajor = 0, SoA = 0, ColumnMajor = 1, AoS = 1 }; // common.h:157-162
static constexpr MatrixLayout RM = MatrixLayout::RowMajor;
static constexpr MatrixLayout CM = MatrixLayout::ColumnMajor;

enum class GradientMode { Ignore = 0, Overwrite = 1, Accumulate = 2 };

namespace detail {
inline void check(int rc) {
	if (rc != TCNN_OK) throw std::runtime_error{tcnn_last_error()};
}
// the TCNN_PRECISION_* of an element type: half or float, nothing else
template <typename T> struct precision_of { static_assert(sizeof(T) == 0, "tcnn: the precision is half or float"); };
template <> struct precision_of<half> { static constexpr int value = TCNN_PRECISION_FP16; };
template <> struct precision_of<float> { static constexpr int value = TCNN_PRECISION_FP32; };
inline std::string to_text(const json& j) { return j.dump(); }
inline std::string to_text(const std::string& s) { return s; }
inline std::string to_text(const char* s) { return s; }
template <typename J> auto to_text(const J& j) -> decltype(j.dump()) { return j.dump(); } // e.g. nlohmann::json
inline json to_json(const json& j) { return j; }
template <typename J> json to_json(const J& j) { return json::parse(to_text(j)); } // text, or another json type
} // namespace detail

inline void free_all_gpu_memory_arenas() { tcnn_free_temporary_memory(); }

// ------------------------------------------------------------------------------------------------------------ GPUMemory
template <typename T>
class GPUMemory {
public:
	GPUMemory() = default;
	explicit GPUMemory(size_t size) { resize(size); }
	GPUMemory(const GPUMemory&) = delete;
	GPUMemory& operator=(const GPUMemory&) = delete;
	GPUMemory(GPUMemory&& o) noexcept { *this = std::move(o); }
	GPUMemory& operator=(GPUMemory&& o) noexcept {
		std::swap(m_data, o.m_data);
		std::swap(m_size, o.m_size);
		return *this;
	}
	~GPUMemory() { if (m_data) tcnn_gpu_free(m_data); }

	void resize(size_t size) {
		if (size == m_size) return;
		if (m_data) { detail::check(tcnn_gpu_free(m_data)); m_data = nullptr; }
		m_size = size;
		if (size) { void* p = nullptr; detail::check(tcnn_gpu_malloc(size * sizeof(T), &p)); m_data = (T*)p; }
	}
	void enlarge(size_t size) { if (size > m_size) resize(size); }
	void memset(int value) { detail::check(tcnn_gpu_memset(m_data, value, m_size * sizeof(T))); }
	void copy_from_host(const T* host, size_t n) { detail::check(tcnn_gpu_memcpy(m_data, host, n * sizeof(T), TCNN_MEMCPY_HOST_TO_DEVICE)); }
	void copy_from_host(const T* host) { copy_from_host(host, m_size); }
	void copy_from_host(const std::vector<T>& v) {
		if (v.size() < m_size) throw std::runtime_error{"Trying to copy " + std::to_string(m_size) + " elements, but vector size is only " + std::to_string(v.size()) + "."};
		copy_from_host(v.data(), m_size);
	}
	void resize_and_copy_from_host(const std::vector<T>& v) { resize(v.size()); copy_from_host(v.data(), v.size()); }
	void copy_to_host(T* host, size_t n) const { detail::check(tcnn_gpu_memcpy(host, m_data, n * sizeof(T), TCNN_MEMCPY_DEVICE_TO_HOST)); }
	void copy_to_host(T* host) const { copy_to_host(host, m_size); }
	void copy_to_host(std::vector<T>& v) const { v.resize(m_size); copy_to_host(v.data(), m_size); }
	void copy_from_device(const GPUMemory<T>& other) {
		if (other.m_size > m_size) resize(other.m_size);
		detail::check(tcnn_gpu_memcpy(m_data, other.m_data, other.m_size * sizeof(T), TCNN_MEMCPY_DEVICE_TO_DEVICE));
	}
	T* data() const { return m_data; }
	size_t size() const { return m_size; }
	size_t get_num_elements() const { return m_size; }
	size_t get_bytes() const { return m_size * sizeof(T); }
	size_t bytes() const { return get_bytes(); }

private:
	T* m_data = nullptr;
	size_t m_size = 0;
};

// ------------------------------------------------------------------------------------------------------------ GPUMatrix
// m rows (dims) x n columns (batch).  ColumnMajor (default): element (i, j) at data[i + j * m] = [n][m] in memory.
template <typename T>
class GPUMatrixDynamic {
public:
	GPUMatrixDynamic() = default;
	GPUMatrixDynamic(uint32_t m, uint32_t n, MatrixLayout layout = CM) : m_rows{m}, m_cols{n}, m_layout{layout}, m_owned{std::make_shared<GPUMemory<T>>((size_t)m * n)} { m_data = m_owned->data(); }
	GPUMatrixDynamic(T* data, uint32_t m, uint32_t n, MatrixLayout layout = CM) : m_rows{m}, m_cols{n}, m_data{data}, m_layout{layout} {}
	T* data() const { return m_data; }
	uint32_t m() const { return m_rows; }
	uint32_t n() const { return m_cols; }
	uint32_t rows() const { return m_rows; }
	uint32_t cols() const { return m_cols; }
	size_t n_elements() const { return (size_t)m_rows * m_cols; }
	size_t n_bytes() const { return n_elements() * sizeof(T); }
	MatrixLayout layout() const { return m_layout; }
	void memset(int value) { detail::check(tcnn_gpu_memset(m_data, value, n_bytes())); }
	std::vector<T> to_cpu_vector() const {
		std::vector<T> v(n_elements());
		detail::check(tcnn_gpu_memcpy(v.data(), m_data, n_bytes(), TCNN_MEMCPY_DEVICE_TO_HOST));
		return v;
	}

protected:
	uint32_t m_rows = 0, m_cols = 0;
	T* m_data = nullptr;
	MatrixLayout m_layout = CM;
	std::shared_ptr<GPUMemory<T>> m_owned;
};

template <typename T, MatrixLayout LAYOUT = MatrixLayout::ColumnMajor>
class GPUMatrix : public GPUMatrixDynamic<T> {
public:
	GPUMatrix() = default;
	GPUMatrix(uint32_t m, uint32_t n) : GPUMatrixDynamic<T>{m, n, LAYOUT} {}
	GPUMatrix(T* data, uint32_t m, uint32_t n) : GPUMatrixDynamic<T>{data, m, n, LAYOUT} {}
};

// ------------------------------------------------------------------------------------------ loss / optimizer / network
// loss.h:38-61.  A Trainer takes the object for its configuration; evaluate() runs the loss on matrices that are the caller's
// (tcnn_loss_evaluate): the device code a trainer's loss runs, so the same bits.  T is the type of predictions and gradients: half or float.
template <typename T>
class Loss {
public:
	explicit Loss(const json& params) : m_params(params) { // parentheses: braces would select json's initializer-list constructor
		const std::string otype = params.value("otype", "RelativeL2");
		std::string lower;
		for (char ch : otype) lower.push_back((char)((ch >= 'A' && ch <= 'Z') ? ch - 'A' + 'a' : ch));
		static const char* known[] = {"l2", "relativel2", "relativel2luminance", "l1", "relativel1", "mape", "smape", "crossentropy", "variance"}; // src/loss.cu:57-65
		bool ok = false;
		for (const char* k : known) ok = ok || lower == k;
		if (!ok) throw std::runtime_error{"Invalid loss type: " + otype}; // src/loss.cu:85-93
		detail::check(tcnn_loss_type(m_params.dump().c_str(), &m_type)); // resolved once: evaluate() is a call whose cost is the host's
	}
	json hyperparams() const { return m_params; }
	void update_hyperparams(const json&) {} // no loss of the reference has any (losses/*.h)

	// loss.h:41-49 with the checks of losses/*.h (l2.h:89-95): dims = target.m(), stride = prediction.m(); values and gradients have the
	// prediction's stride, and their rows beyond dims are written as zeros.
	void evaluate(stream_t stream, const float loss_scale, const GPUMatrix<T>& prediction, const GPUMatrix<float>& target, GPUMatrix<float>& values, GPUMatrix<T>& gradients,
	              const GPUMatrix<float>* data_pdf = nullptr) const {
		check_shapes(prediction, target, data_pdf);
		if (values.m() != prediction.m()) throw std::runtime_error{"Loss::evaluate check failed: values.m() == stride"};
		if (gradients.m() != prediction.m()) throw std::runtime_error{"Loss::evaluate check failed: gradients.m() == stride"};
		detail::check(tcnn_loss_evaluate(type(), stream, loss_scale, nullptr, prediction.n(), target.m(), prediction.data(), prediction.m(), detail::precision_of<T>::value, target.data(),
		                                 data_pdf ? data_pdf->data() : nullptr, values.data(), values.m(), gradients.data(), gradients.m(), nullptr));
	}
	void evaluate(const float loss_scale, const GPUMatrix<T>& prediction, const GPUMatrix<float>& target, GPUMatrix<float>& values, GPUMatrix<T>& gradients,
	              const GPUMatrix<float>* data_pdf = nullptr) const { // loss.h:51-60
		evaluate(nullptr, loss_scale, prediction, target, values, gradients, data_pdf);
	}
	// Not in the reference: the sum of the values -- what trainer->loss() reports -- into one device float instead of a values matrix,
	// reduced in a fixed order inside the same pass (the same arguments give the same bits).
	void evaluate(stream_t stream, const float loss_scale, const GPUMatrix<T>& prediction, const GPUMatrix<float>& target, float* loss_sum, GPUMatrix<T>& gradients,
	              const GPUMatrix<float>* data_pdf = nullptr) const {
		check_shapes(prediction, target, data_pdf);
		if (gradients.m() != prediction.m()) throw std::runtime_error{"Loss::evaluate check failed: gradients.m() == stride"};
		if (!loss_sum) throw std::runtime_error{"Loss::evaluate check failed: loss_sum != nullptr"};
		detail::check(tcnn_loss_evaluate(type(), stream, loss_scale, nullptr, prediction.n(), target.m(), prediction.data(), prediction.m(), detail::precision_of<T>::value, target.data(),
		                                 data_pdf ? data_pdf->data() : nullptr, nullptr, 0, gradients.data(), gradients.m(), loss_sum));
	}

private:
	static void check_shapes(const GPUMatrix<T>& prediction, const GPUMatrix<float>& target, const GPUMatrix<float>* data_pdf) {
		if (prediction.n() != target.n()) throw std::runtime_error{"Loss::evaluate check failed: prediction.n() == target.n()"};
		if (data_pdf && data_pdf->m() != target.m()) throw std::runtime_error{"Loss::evaluate check failed: !data_pdf || data_pdf->m() == dims"};
	}
	int type() const { return m_type; }
	json m_params;
	int m_type = 0; // the library's number for the loss (tcnn_loss_type)
};
template <typename T> Loss<T>* create_loss(const json& params) { return new Loss<T>{params}; }

// optimizer.h:40-66.  Configuration only until allocate(), which makes the native optimizer (tcnn_optimizer_t); a Trainer does not
// need that -- it builds its own optimizer from hyperparams().  T is the type of the working weights and of the gradients: half, or
// float -- then there is ONE weight vector: step() takes weights == weights_full_precision (or nullptr) and fp32 gradients, and
// custom_weights() points at floats.
template <typename T>
class Optimizer {
public:
	explicit Optimizer(const json& params) : m_params(params) {}
	Optimizer(const Optimizer&) = delete;
	Optimizer& operator=(const Optimizer&) = delete;
	~Optimizer() { if (m_handle) tcnn_optimizer_destroy(m_handle); }

	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes = {}) {
		static_assert(std::is_same<T, half>::value || std::is_same<T, float>::value, "tcnn::Optimizer<T>: the working weights are half or float");
		std::vector<uint32_t> flat;
		for (const auto& ls : layer_sizes) { flat.push_back(ls.first); flat.push_back(ls.second); }
		tcnn_optimizer_t fresh = nullptr;
		detail::check(tcnn_optimizer_create_precision(m_params.dump().c_str(), n_weights, flat.data(), layer_sizes.size(), detail::precision_of<T>::value, &fresh));
		if (m_handle) tcnn_optimizer_destroy(m_handle);
		m_handle = fresh;
	}
	// gradients: scaled by loss_scale, like the ones a Trainer's backward pass writes
	void step(stream_t stream, float loss_scale, float* weights_full_precision, T* weights, const T* gradients) {
		detail::check(tcnn_optimizer_step(allocated("step"), stream, loss_scale, weights_full_precision, weights, gradients, detail::precision_of<T>::value));
	}
	// the same on fp32 gradients (no counterpart in the reference): read as they are, never rounded to half.  (Optimizer<float>: the
	// overload above already is this one.)
	template <typename U = T>
	void step(stream_t stream, float loss_scale, float* weights_full_precision, typename std::enable_if<!std::is_same<U, float>::value, U>::type* weights, const float* gradients) {
		detail::check(tcnn_optimizer_step(allocated("step"), stream, loss_scale, weights_full_precision, weights, gradients, TCNN_PRECISION_FP32));
	}
	float learning_rate() const { return tcnn_optimizer_learning_rate(allocated("learning_rate")); }
	void set_learning_rate(float val) { detail::check(tcnn_optimizer_set_learning_rate(allocated("set_learning_rate"), val)); }
	uint32_t step() const { return tcnn_optimizer_step_count(allocated("step")); }
	size_t n_weights() const { return m_handle ? tcnn_optimizer_n_params(m_handle) : 0; }
	T* custom_weights() const { return m_handle ? (T*)tcnn_optimizer_custom_weights(m_handle) : nullptr; }
	// after the caller has overwritten `weights` by other means (a loaded snapshot)
	void weights_restored(stream_t stream, const T* weights) { detail::check(tcnn_optimizer_weights_restored(allocated("weights_restored"), stream, weights)); }

	json hyperparams() const {
		if (!m_handle) return m_params;
		const char* text = tcnn_optimizer_hyperparams(m_handle);
		if (!text) throw std::runtime_error{tcnn_last_error()};
		return json::parse(text);
	}
	void update_hyperparams(const json& params) {
		if (m_handle) detail::check(tcnn_optimizer_update_hyperparams(m_handle, params.dump().c_str()));
		else m_params = params;
	}
	// the object a Trainer's snapshot carries as its "optimizer" entry (binary values inside)
	json serialize() const {
		const void* bytes = nullptr;
		size_t size = 0;
		detail::check(tcnn_optimizer_serialize(allocated("serialize"), &bytes, &size));
		return json::from_msgpack(std::vector<uint8_t>((const uint8_t*)bytes, (const uint8_t*)bytes + size));
	}
	void deserialize(const json& data) {
		const std::vector<uint8_t> bytes = json::to_msgpack(data);
		detail::check(tcnn_optimizer_deserialize(allocated("deserialize"), bytes.data(), bytes.size()));
	}
	tcnn_optimizer_t handle() const { return m_handle; }

private:
	tcnn_optimizer_t allocated(const char* what) const {
		if (!m_handle) throw std::runtime_error{std::string{"Optimizer::"} + what + ": call allocate() first"};
		return m_handle;
	}
	json m_params;
	tcnn_optimizer_t m_handle = nullptr;
};
template <typename T> Optimizer<T>* create_optimizer(const json& params) { return new Optimizer<T>{params}; }

template <typename T, typename PARAMS_T, typename COMPUTE_T> class Trainer;

template <typename T>
class NetworkWithInputEncoding {
public:
	NetworkWithInputEncoding(uint32_t n_dims_to_encode, uint32_t n_output_dims, const json& encoding, const json& network)
	: m_n_input_dims{n_dims_to_encode}, m_n_output_dims{n_output_dims}, m_encoding(encoding), m_network(network) {}

	// object.h:147-176: float in, float out (unpadded width); needs a Trainer to have bound the parameters
	void inference(stream_t stream, const GPUMatrixDynamic<float>& input, GPUMatrixDynamic<float>& output, bool use_inference_params = true) {
		if (!m_trainer) throw std::runtime_error{"NetworkWithInputEncoding::inference: the network has no parameters yet (construct a Trainer first)"};
		if (input.m() != m_n_input_dims || output.m() != m_n_output_dims || input.n() != output.n()) throw std::runtime_error{"inference: matrix shapes do not match the network"};
		detail::check(tcnn_trainer_inference(m_trainer, stream, input.n(), input.data(), (int)input.layout(), output.data(), (int)output.layout(), use_inference_params ? 1 : 0));
	}
	void inference(const GPUMatrixDynamic<float>& input, GPUMatrixDynamic<float>& output) { inference(nullptr, input, output); }

	// object.h:342-366: d_dinput = d output[dim] / d input with the bound Trainer's inference parameters (dim counts padded columns); no
	// parameter gradient is touched.  Both matrices are column-major n_dims x batch, as the reference's GPUMatrix<float> is.
	void input_gradient(stream_t stream, uint32_t dim, const GPUMatrix<float>& input, GPUMatrix<float>& d_dinput, float backprop_scale = tcnn_default_loss_scale(detail::precision_of<T>::value)) {
		if (!m_trainer) throw std::runtime_error{"NetworkWithInputEncoding::input_gradient: the network has no parameters yet (construct a Trainer first)"};
		if (dim >= padded_output_width()) throw std::runtime_error{"Invalid dimension to compute the input gradient for."}; // object.h:350
		if (input.m() != m_n_input_dims || d_dinput.m() != m_n_input_dims || input.n() != d_dinput.n()) throw std::runtime_error{"input_gradient: matrix shapes do not match the network"};
		detail::check(tcnn_trainer_input_gradient(m_trainer, stream, input.n(), dim, input.data(), d_dinput.data(), backprop_scale));
	}
	// The same for several output columns from one forward pass: jacobian is column-major (dims.size() * n_dims) x batch, so that sample i's
	// block is [dims.size()][n_dims] and its row k is input_gradient(dims[k])'s column i, bit for bit.
	void input_jacobian(stream_t stream, const std::vector<uint32_t>& dims, const GPUMatrix<float>& input, GPUMatrix<float>& jacobian, float backprop_scale = tcnn_default_loss_scale(detail::precision_of<T>::value)) {
		if (!m_trainer) throw std::runtime_error{"NetworkWithInputEncoding::input_jacobian: the network has no parameters yet (construct a Trainer first)"};
		if (input.m() != m_n_input_dims || jacobian.m() != dims.size() * m_n_input_dims || input.n() != jacobian.n()) throw std::runtime_error{"input_jacobian: matrix shapes do not match the network"};
		detail::check(tcnn_trainer_input_jacobian(m_trainer, stream, input.n(), dims.data(), (uint32_t)dims.size(), input.data(), jacobian.data(), backprop_scale));
	}
	// Forward mode: every output's derivative along n_tangents input directions.  tangents is column-major (n_tangents * n_dims) x batch --
	// sample i's block is [n_tangents][n_dims] -- and jvp column-major (n_tangents * padded_output_width()) x batch in the network's
	// precision T: sample i's block is [n_tangents][padded_output_width()], row t = J(x_i) tangents_i[t].  No backprop_scale: the map is
	// linear in the tangent (tcnn_amd.h: tcnn_module_input_jvp).
	void input_jvp(stream_t stream, uint32_t n_tangents, const GPUMatrix<float>& input, const GPUMatrix<float>& tangents, GPUMatrix<T>& jvp) {
		if (!m_trainer) throw std::runtime_error{"NetworkWithInputEncoding::input_jvp: the network has no parameters yet (construct a Trainer first)"};
		if (input.m() != m_n_input_dims || tangents.m() != n_tangents * m_n_input_dims || jvp.m() != n_tangents * padded_output_width() || input.n() != tangents.n() || input.n() != jvp.n()) {
			throw std::runtime_error{"input_jvp: matrix shapes do not match the network"};
		}
		detail::check(tcnn_trainer_input_jvp(m_trainer, stream, input.n(), n_tangents, input.data(), tangents.data(), jvp.data()));
	}
	// Training through input_jvp, on the bound Trainer's TRAINING parameters (tcnn_amd.h: tcnn_module_input_jvp_forward / _backward).
	// input_jvp_forward: input_jvp's jvp, the network's output (optional: padded_output_width() x batch) and the context of the backward call.
	// input_jvp_backward: the gradients of sum_t <dL_djvp_t, J v_t> + <dL_doutput, f(x)> -- the parameter gradients into the Trainer's
	// gradient buffer under param_gradients_mode (Trainer::optimizer_step reads it), and optionally dL_dinput (n_dims x batch) and
	// dL_dtangents (shaped as tangents).  No loss scale inside: cotangents scaled by one give gradients scaled by it.  First order only.
	struct InputJvpContext {
		tcnn_context_t handle = nullptr;
		InputJvpContext() = default;
		InputJvpContext(const InputJvpContext&) = delete;
		InputJvpContext& operator=(const InputJvpContext&) = delete;
		~InputJvpContext() { if (handle) tcnn_context_destroy(handle); }
	};
	std::unique_ptr<InputJvpContext> input_jvp_forward(stream_t stream, uint32_t n_tangents, const GPUMatrix<float>& input, const GPUMatrix<float>& tangents, GPUMatrix<T>& jvp,
	                                                   GPUMatrix<T>* output = nullptr) {
		if (!m_trainer) throw std::runtime_error{"NetworkWithInputEncoding::input_jvp_forward: the network has no parameters yet (construct a Trainer first)"};
		if (input.m() != m_n_input_dims || tangents.m() != n_tangents * m_n_input_dims || jvp.m() != n_tangents * padded_output_width() || input.n() != tangents.n() || input.n() != jvp.n() ||
		    (output && (output->m() != padded_output_width() || output->n() != input.n()))) {
			throw std::runtime_error{"input_jvp_forward: matrix shapes do not match the network"};
		}
		std::unique_ptr<InputJvpContext> ctx{new InputJvpContext};
		detail::check(tcnn_trainer_input_jvp_forward(m_trainer, stream, input.n(), n_tangents, input.data(), tangents.data(), jvp.data(), output ? output->data() : nullptr, &ctx->handle));
		return ctx;
	}
	void input_jvp_backward(stream_t stream, const InputJvpContext& ctx, uint32_t n_tangents, const GPUMatrix<float>& input, const GPUMatrix<float>& tangents, const GPUMatrix<T>& dL_djvp,
	                        const GPUMatrix<T>* dL_doutput = nullptr, GPUMatrix<float>* dL_dinput = nullptr, GPUMatrix<float>* dL_dtangents = nullptr,
	                        GradientMode param_gradients_mode = GradientMode::Overwrite) {
		if (!m_trainer) throw std::runtime_error{"NetworkWithInputEncoding::input_jvp_backward: the network has no parameters yet (construct a Trainer first)"};
		if (input.m() != m_n_input_dims || tangents.m() != n_tangents * m_n_input_dims || dL_djvp.m() != n_tangents * padded_output_width() || input.n() != tangents.n() ||
		    input.n() != dL_djvp.n() || (dL_doutput && (dL_doutput->m() != padded_output_width() || dL_doutput->n() != input.n())) ||
		    (dL_dinput && (dL_dinput->m() != m_n_input_dims || dL_dinput->n() != input.n())) || (dL_dtangents && (dL_dtangents->m() != tangents.m() || dL_dtangents->n() != input.n()))) {
			throw std::runtime_error{"input_jvp_backward: matrix shapes do not match the network"};
		}
		detail::check(tcnn_trainer_input_jvp_backward(m_trainer, stream, ctx.handle, input.n(), n_tangents, input.data(), tangents.data(), dL_djvp.data(), dL_doutput ? dL_doutput->data() : nullptr,
		                                              dL_dinput ? dL_dinput->data() : nullptr, dL_dtangents ? dL_dtangents->data() : nullptr, (int)param_gradients_mode));
	}

	uint32_t input_width() const { return m_n_input_dims; }
	uint32_t output_width() const { return m_n_output_dims; }
	uint32_t padded_output_width() const { return m_trainer ? tcnn_trainer_padded_output_width(m_trainer) : (m_n_output_dims + 15) / 16 * 16; }
	size_t n_params() const { return m_trainer ? tcnn_trainer_n_params(m_trainer) : 0; }
	json hyperparams() const { return m_trainer ? json::parse(tcnn_trainer_network_hyperparams(m_trainer)) : json{{"otype", "NetworkWithInputEncoding"}, {"encoding", m_encoding}, {"network", m_network}}; }
	const json& encoding_config() const { return m_encoding; }
	const json& network_config() const { return m_network; }

	// max_level of the grid encoding (GridEncoding, grid_interface.h:101-123; tcnn_amd.h states the rule): a fraction of the levels,
	// 1000 keeps every one.  A value set before a Trainer binds the network is held here and applied at binding.
	// set_max_level_gpu: one float per row in device memory (the caller's; nullptr: the scalar again), at least as many as the rows of
	// every call made while it is set.
	float max_level() const { return m_trainer ? tcnn_trainer_max_level(m_trainer) : m_max_level; }
	void set_max_level(float value) {
		if (m_trainer) detail::check(tcnn_trainer_set_max_level(m_trainer, value));
		m_max_level = value;
	}
	float* max_level_gpu() const { return m_max_level_gpu; }
	void set_max_level_gpu(float* per_sample) {
		if (m_trainer) detail::check(tcnn_trainer_set_max_level_gpu(m_trainer, per_sample));
		m_max_level_gpu = per_sample;
	}

private:
	template <typename A, typename B, typename C> friend class Trainer;
	// at binding: a setting made before reaches the trainer (nothing is called while nothing was set)
	void bind(tcnn_trainer_t trainer) {
		m_trainer = trainer;
		if (!(m_max_level == 1000.f) || m_max_level_gpu) {
			detail::check(tcnn_trainer_set_max_level(trainer, m_max_level));
			detail::check(tcnn_trainer_set_max_level_gpu(trainer, m_max_level_gpu));
		}
	}
	uint32_t m_n_input_dims, m_n_output_dims;
	json m_encoding, m_network;
	tcnn_trainer_t m_trainer = nullptr; // borrowed from the Trainer that bound this network
	float m_max_level = 1000.f;         // grid_interface.h:118
	float* m_max_level_gpu = nullptr;
};

// ---------------------------------------------------------------------------------------------------------------- Trainer
// <float, half, half>: the mixed-precision trainer.  <float, float, float>: the full-precision one -- params() == params_full_precision(),
// float output / dL_doutput / gradients, loss scale 1, every training_step unfused.
template <typename T, typename PARAMS_T, typename COMPUTE_T = T>
class Trainer {
	static_assert(std::is_same<T, float>::value, "tcnn::Trainer<T, PARAMS_T, COMPUTE_T>: the input type T is float");
	static_assert(std::is_same<PARAMS_T, COMPUTE_T>::value && (std::is_same<COMPUTE_T, half>::value || std::is_same<COMPUTE_T, float>::value),
	              "tcnn::Trainer<T, PARAMS_T, COMPUTE_T>: parameters and compute are both half or both float");
public:
	struct ForwardContext { // trainer.h:89-95
		tcnn_train_ctx_t handle = nullptr;
		uint32_t n = 0, padded_output_width = 0;
		~ForwardContext() { if (handle) tcnn_train_ctx_destroy(handle); }
		const COMPUTE_T* output() const { return (const COMPUTE_T*)tcnn_train_ctx_output(handle); }         // [n][padded_output_width]
		const COMPUTE_T* dL_doutput() const { return (const COMPUTE_T*)tcnn_train_ctx_dL_doutput(handle); }
		const float* L() const { return tcnn_train_ctx_L(handle); }
	};

	Trainer(std::shared_ptr<NetworkWithInputEncoding<COMPUTE_T>> model, std::shared_ptr<Optimizer<PARAMS_T>> optimizer, std::shared_ptr<Loss<COMPUTE_T>> loss, uint32_t seed = 1337)
	: m_model{std::move(model)}, m_optimizer{std::move(optimizer)}, m_loss{std::move(loss)} {
		json config = json::object();
		config["encoding"] = m_model->encoding_config();
		config["network"] = m_model->network_config();
		config["optimizer"] = m_optimizer->hyperparams();
		config["loss"] = m_loss->hyperparams();
		detail::check(tcnn_create_from_config_precision(m_model->input_width(), m_model->output_width(), config.dump().c_str(), seed, detail::precision_of<COMPUTE_T>::value, &m_handle));
		try {
			m_model->bind(m_handle);
		} catch (...) {
			m_model->m_trainer = nullptr;
			tcnn_trainer_destroy(m_handle);
			throw;
		}
	}
	Trainer(const Trainer&) = delete;
	Trainer& operator=(const Trainer&) = delete;
	~Trainer() {
		if (m_model && m_model->m_trainer == m_handle) m_model->m_trainer = nullptr;
		if (m_handle) tcnn_trainer_destroy(m_handle);
	}

	// trainer.h:163-190
	std::unique_ptr<ForwardContext> training_step(stream_t stream, const GPUMatrixDynamic<T>& input, const GPUMatrix<float>& target, const GPUMatrix<float>* data_pdf = nullptr,
	                                              bool run_optimizer = true, GPUMatrixDynamic<T>* dL_dinput = nullptr, bool use_inference_params = false,
	                                              GradientMode gradient_mode = GradientMode::Overwrite, const GPUMatrix<COMPUTE_T>* external_dL_dy = nullptr) {
		if (input.n() != target.n()) throw std::runtime_error{"training_step: input and target batch sizes differ"};
		auto ctx = std::make_unique<ForwardContext>();
		detail::check(tcnn_trainer_training_step(m_handle, stream, input.n(), input.data(), (int)input.layout(), target.data(), data_pdf ? data_pdf->data() : nullptr, run_optimizer ? 1 : 0,
		                                         dL_dinput ? dL_dinput->data() : nullptr, use_inference_params ? 1 : 0, (int)gradient_mode, external_dL_dy ? (const void*)external_dL_dy->data() : nullptr,
		                                         &ctx->handle));
		ctx->n = input.n();
		ctx->padded_output_width = tcnn_trainer_padded_output_width(m_handle);
		return ctx;
	}
	std::unique_ptr<ForwardContext> training_step(const GPUMatrixDynamic<T>& input, const GPUMatrix<float>& target) { return training_step(nullptr, input, target); } // trainer.h:192

	float loss(stream_t stream, const ForwardContext& ctx) { // trainer.h:205-207
		float value = 0;
		detail::check(tcnn_trainer_loss(m_handle, stream, ctx.handle, &value));
		return value;
	}
	void optimizer_step(stream_t stream, float loss_scale) { detail::check(tcnn_trainer_optimizer_step(m_handle, stream, loss_scale)); } // trainer.h:155-157

	size_t n_params() const { return tcnn_trainer_n_params(m_handle); }                                              // trainer.h:338
	float* params_full_precision() const { return tcnn_trainer_params_full_precision(m_handle); }                    // trainer.h:226
	PARAMS_T* params() const { return (PARAMS_T*)tcnn_trainer_params(m_handle); }                                    // trainer.h:230
	PARAMS_T* params_inference() const { return (PARAMS_T*)tcnn_trainer_params_inference(m_handle); }                // trainer.h:234
	PARAMS_T* param_gradients() const { return (PARAMS_T*)tcnn_trainer_param_gradients(m_handle); }                  // trainer.h:238
	void set_params_full_precision(const float* params, size_t n, bool device_ptr = false) { detail::check(tcnn_trainer_set_params_full_precision(m_handle, params, n, device_ptr ? 1 : 0)); }
	void set_params(const PARAMS_T* params, size_t n, bool device_ptr = false) { detail::check(tcnn_trainer_set_params(m_handle, params, n, device_ptr ? 1 : 0)); }
	void initialize_params() { detail::check(tcnn_trainer_initialize_params(m_handle)); }                             // trainer.h:68-87
	void update_hyperparams(const json& params) { detail::check(tcnn_trainer_update_hyperparams(m_handle, params.dump().c_str())); } // trainer.h:213
	json hyperparams() const { return json::parse(tcnn_trainer_hyperparams(m_handle)); }
	uint32_t optimizer_step_count() const { return tcnn_trainer_optimizer_step_count(m_handle); }

	// trainer.h:275-315: the snapshot object (binary values inside); store it with json::to_msgpack like callers of the reference do
	json serialize(bool serialize_optimizer = false) {
		const void* bytes = nullptr;
		size_t size = 0;
		detail::check(tcnn_trainer_serialize(m_handle, serialize_optimizer ? 1 : 0, &bytes, &size));
		return json::from_msgpack(std::vector<uint8_t>((const uint8_t*)bytes, (const uint8_t*)bytes + size));
	}
	void deserialize(const json& data) {
		const std::vector<uint8_t> bytes = json::to_msgpack(data);
		detail::check(tcnn_trainer_deserialize(m_handle, bytes.data(), bytes.size()));
	}

	std::shared_ptr<NetworkWithInputEncoding<COMPUTE_T>> model() const { return m_model; }
	tcnn_trainer_t handle() const { return m_handle; }

private:
	std::shared_ptr<NetworkWithInputEncoding<COMPUTE_T>> m_model;
	std::shared_ptr<Optimizer<PARAMS_T>> m_optimizer;
	std::shared_ptr<Loss<COMPUTE_T>> m_loss;
	tcnn_trainer_t m_handle = nullptr;
};

// ----------------------------------------------------------------------------------------------------- config.h:46-63
template <typename T>
struct TrainableModelT {
	std::shared_ptr<Loss<T>> loss;
	std::shared_ptr<Optimizer<T>> optimizer;
	std::shared_ptr<NetworkWithInputEncoding<T>> network;
	std::shared_ptr<Trainer<float, T, T>> trainer;
};
typedef TrainableModelT<network_precision_t> TrainableModel;

// create_from_config for a chosen precision: create_from_config_as<float>(...) trains in full precision
template <typename T, typename J>
inline TrainableModelT<T> create_from_config_as(uint32_t n_input_dims, uint32_t n_output_dims, const J& config_in) {
	const json config = detail::to_json(config_in);
	const json encoding_opts = config.value("encoding", json::object());
	const json loss_opts = config.value("loss", json::object());
	const json optimizer_opts = config.value("optimizer", json::object());
	const json network_opts = config.value("network", json::object());
	std::shared_ptr<Loss<T>> loss{create_loss<T>(loss_opts)};
	std::shared_ptr<Optimizer<T>> optimizer{create_optimizer<T>(optimizer_opts)};
	auto network = std::make_shared<NetworkWithInputEncoding<T>>(n_input_dims, n_output_dims, encoding_opts, network_opts);
	auto trainer = std::make_shared<Trainer<float, T, T>>(network, optimizer, loss);
	return {loss, optimizer, network, trainer};
}
inline TrainableModel create_from_config(uint32_t n_input_dims, uint32_t n_output_dims, json config) {
	return create_from_config_as<network_precision_t>(n_input_dims, n_output_dims, config);
}
template <typename J>
inline TrainableModel create_from_config(uint32_t n_input_dims, uint32_t n_output_dims, const J& config) { return create_from_config(n_input_dims, n_output_dims, json::parse(detail::to_text(config))); }

} // namespace tcnn
