// model.h -- host-side object model of libtcnn_amd: the MI355X counterpart of the reference's
// Encoding / Network / NetworkWithInputEncoding / Loss / Optimizer / Trainer classes, reduced to the hot path
// (SURVEY.md section 8).  Everything here is orchestration: which kernel runs on which buffer in which order.
//
// Reference files restated (relative to /root/reference):
//   include/tiny-cuda-nn/encodings/grid.h:653-1208, oneblob.h:167-307, identity.h:88-190, src/encoding.cu:144-158
//   src/fully_fused_mlp.cu:636-891, src/network.cu:48-137
//   include/tiny-cuda-nn/network_with_input_encoding.h:40-192
//   include/tiny-cuda-nn/losses/{l2,relative_l2}.h, src/loss.cu:85-93
//   include/tiny-cuda-nn/optimizers/adam.h:122-327, src/optimizer.cu:50-82
//   include/tiny-cuda-nn/trainer.h:48-363, config.h:46-63, object.h:120-270
#pragma once

#include "json_lite.h"
#include "tcnn_common.h"
#include "mlp_side_jobs.h"

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <random>
#include <unordered_map>
#include <vector>

namespace tcnn_amd {

// ------------------------------------------------------------------------------------------------------------------
// logging (common_host.h:46-69)
// ------------------------------------------------------------------------------------------------------------------
struct LogSink {
	void (*callback)(int, const char*, void*) = nullptr;
	void* user = nullptr;
};
inline LogSink& log_sink() { static LogSink s; return s; }
inline void log_message(int severity, const std::string& msg) {
	LogSink& s = log_sink();
	if (s.callback) s.callback(severity, msg.c_str(), s.user);
}

inline std::string to_lower(std::string s) {
	for (auto& ch : s) ch = (char)std::tolower((unsigned char)ch);
	return s;
}
inline bool equals_case_insensitive(const std::string& a, const std::string& b) { return to_lower(a) == to_lower(b); } // common_host.h:238-246

// ------------------------------------------------------------------------------------------------------------------
// Stream-ordered caching arena (the role of GPUMemoryArena, gpu_memory.h:426-720): blocks are handed out per stream and
// returned to that stream's free list when their owner dies, so reuse is ordered by the stream itself.
// ------------------------------------------------------------------------------------------------------------------
class Arena {
public:
	static Arena& instance() { static Arena a; return a; }

	void* alloc(hipStream_t stream, size_t bytes, size_t* capacity_out) {
		bytes = std::max<size_t>((bytes + 255) / 256 * 256, 256);
		std::lock_guard<std::mutex> lock{m_mutex};
		int dev = 0;
		HIP_CHECK_THROW(hipGetDevice(&dev));
		auto& fl = m_free[key(dev, stream)];
		auto it = fl.lower_bound(bytes);
		if (it != fl.end() && it->first <= bytes * 2 + (1u << 20)) {
			void* p = it->second;
			*capacity_out = it->first;
			fl.erase(it);
			return p;
		}
		void* p = nullptr;
		hipError_t err = hipMalloc(&p, bytes);
		if (err != hipSuccess) {
			release_locked();
			HIP_CHECK_THROW(hipMalloc(&p, bytes));
		}
		m_total += bytes;
		*capacity_out = bytes;
		return p;
	}

	void free(hipStream_t stream, int dev, void* p, size_t capacity) {
		std::lock_guard<std::mutex> lock{m_mutex};
		m_free[key(dev, stream)].emplace(capacity, p);
	}

	void release_all() { // free_all_gpu_memory_arenas, gpu_memory.h:751
		std::lock_guard<std::mutex> lock{m_mutex};
		release_locked();
	}

	size_t total_bytes() const { return m_total; }

private:
	static std::pair<int, hipStream_t> key(int dev, hipStream_t s) { return {dev, s}; }
	void release_locked() {
		(void)hipDeviceSynchronize();
		for (auto& kv : m_free) {
			for (auto& blk : kv.second) {
				(void)hipFree(blk.second);
				m_total -= blk.first;
			}
			kv.second.clear();
		}
	}
	std::mutex m_mutex;
	std::map<std::pair<int, hipStream_t>, std::multimap<size_t, void*>> m_free;
	size_t m_total = 0;
};

class ArenaBuf {
public:
	ArenaBuf() = default;
	ArenaBuf(hipStream_t stream, size_t bytes) : m_stream{stream}, m_bytes{bytes} {
		if (bytes == 0) return;
		HIP_CHECK_THROW(hipGetDevice(&m_dev));
		m_ptr = Arena::instance().alloc(stream, bytes, &m_capacity);
	}
	~ArenaBuf() { reset(); }
	ArenaBuf(const ArenaBuf&) = delete;
	ArenaBuf& operator=(const ArenaBuf&) = delete;
	ArenaBuf(ArenaBuf&& o) noexcept { *this = std::move(o); }
	ArenaBuf& operator=(ArenaBuf&& o) noexcept {
		if (this != &o) {
			reset();
			m_ptr = o.m_ptr; m_stream = o.m_stream; m_bytes = o.m_bytes; m_capacity = o.m_capacity; m_dev = o.m_dev;
			o.m_ptr = nullptr; o.m_bytes = 0;
		}
		return *this;
	}
	void reset() {
		if (m_ptr) Arena::instance().free(m_stream, m_dev, m_ptr, m_capacity);
		m_ptr = nullptr;
		m_bytes = 0;
	}
	void* data() const { return m_ptr; }
	template <typename T> T* as() const { return (T*)m_ptr; }
	size_t bytes() const { return m_bytes; }
	explicit operator bool() const { return m_ptr != nullptr; }
private:
	void* m_ptr = nullptr;
	hipStream_t m_stream = nullptr;
	size_t m_bytes = 0, m_capacity = 0;
	int m_dev = 0;
};

// Persistent device allocation (GPUMemory<T>, gpu_memory.h:60-392)
class DeviceBuf {
public:
	DeviceBuf() = default;
	explicit DeviceBuf(size_t bytes) { resize(bytes); }
	~DeviceBuf() { if (m_ptr) (void)hipFree(m_ptr); }
	DeviceBuf(const DeviceBuf&) = delete;
	DeviceBuf& operator=(const DeviceBuf&) = delete;
	DeviceBuf(DeviceBuf&& o) noexcept : m_ptr{o.m_ptr}, m_bytes{o.m_bytes} { o.m_ptr = nullptr; o.m_bytes = 0; }
	DeviceBuf& operator=(DeviceBuf&& o) noexcept {
		if (this != &o) {
			if (m_ptr) (void)hipFree(m_ptr);
			m_ptr = o.m_ptr; m_bytes = o.m_bytes;
			o.m_ptr = nullptr; o.m_bytes = 0;
		}
		return *this;
	}
	void resize(size_t bytes) {
		if (bytes == m_bytes) return;
		if (m_ptr) { (void)hipFree(m_ptr); m_ptr = nullptr; }
		m_bytes = bytes;
		if (bytes) HIP_CHECK_THROW(hipMalloc(&m_ptr, bytes));
	}
	void memset(int v) { if (m_bytes) HIP_CHECK_THROW(hipMemset(m_ptr, v, m_bytes)); }
	void* data() const { return m_ptr; }
	template <typename T> T* as() const { return (T*)m_ptr; }
	size_t bytes() const { return m_bytes; }
private:
	void* m_ptr = nullptr;
	size_t m_bytes = 0;
};

// ------------------------------------------------------------------------------------------------------------------
// pcg32 (dependencies/pcg32/pcg32.h:40-166, the published PCG-XSH-RR 64/32 generator)
// ------------------------------------------------------------------------------------------------------------------
struct Pcg32 {
	uint64_t st[2] = {0x853c49e6748fea9bULL, 0xda3e39cb94b95bdbULL};
	static constexpr uint64_t MULT = 0x5851f42d4c957f2dULL;
	Pcg32() = default;
	explicit Pcg32(uint64_t initstate, uint64_t initseq = 1) {
		st[0] = 0;
		st[1] = (initseq << 1u) | 1u;
		next_uint();
		st[0] += initstate;
		next_uint();
	}
	uint32_t next_uint() {
		const uint64_t old = st[0];
		st[0] = old * MULT + st[1];
		const uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
		const uint32_t rot = (uint32_t)(old >> 59u);
		return (xorshifted >> rot) | (xorshifted << ((~rot + 1u) & 31));
	}
	float next_float() {
		const uint32_t u = (next_uint() >> 9) | 0x3f800000u;
		float f;
		memcpy(&f, &u, 4);
		return f - 1.0f;
	}
};

// ------------------------------------------------------------------------------------------------------------------
// Encodings
// ------------------------------------------------------------------------------------------------------------------
struct EncodingContext {
	ArenaBuf to_reduce; // Composite encoding with a Sum / Product reduction: the nested outputs [nested][n][width]
	ArenaBuf dy_dx;       // grid only: float [n][L*F][D]
	ArenaBuf chunk_mask;  // grid only: uint64 [L][32][n/64] bit planes, which samples touch which scatter chunk (filter for the LDS scatter)
	ArenaBuf hit_elems;   // grid only, instead of chunk_mask: the hit lists of this batch (GridHitLists::elems); counters and validity below
	GridHitLists hit_lists;
	uint64_t hit_generation = 0; // the encoding's list counters are reused by later forward passes: lists are valid while this is the latest one on its stream
	const void* hit_stream = nullptr;
	uint32_t n = 0;
	GridForwardRoute route; // grid only: how this batch was produced, and the gradient kernels that follow from it (grid_forward_route)
	std::vector<EncodingContext> nested; // Composite: one context per nested encoding
};

// What the caller of Encoding::backward() offers to that one call, and what the call reports back.  An encoding is free to ignore all of it.
struct BackwardHandoff {
	const MlpReduceJob* reduce_job = nullptr; // a small job the pass may carry on one of its launches, or pass on with the prologue
	// the optimizer's launch offers to run the scatter's finalize pass (and the reduce job) as its prologue (AdamPrologue, tcnn_common.h):
	// a backward pass that takes the offer fills it in, sets ->pending and launches no finalize pass of its own
	AdamPrologue* prologue = nullptr;
	void* list_gradients = nullptr;           // GridBackwardRoute::tail was taken: the workspace the MLP kernel's tail filled, read instead of launching k_grid_list_gradients
	bool reduce_carried = false;              // reported: reduce_job went with a launch of this pass or with the prologue -- it is no longer the caller's to run
};

// What a caller that asked Encoding::forward_route() itself hands to forward(): the route (kernel Planes: `out` is level planes [padded / F][n][F]),
// a side job the plane kernel carries (the fragment images of the network behind the encoding) and the samples the fused MLP kernel's workgroups
// will work on (mlp_train_item_map): a grid that writes hit lists forms its items from them where its item size allows (GridBackwardRoute::tail)
struct ForwardPlan {
	GridForwardRoute route;
	const MlpPrepJob* prep_job = nullptr;
	const GridItemMap* item_map = nullptr;
};

class Encoding {
public:
	virtual ~Encoding() {}
	virtual uint32_t input_width() const = 0;
	virtual uint32_t output_width() const = 0; // unpadded
	uint32_t padded_output_width() const { return output_width() + m_n_to_pad; }
	virtual uint32_t required_output_alignment() const { return 1; }
	virtual void set_padded_output_width(uint32_t padded) { // encoding.h: each encoding pads its own output with ones
		CHECK_THROW(padded >= output_width());
		m_n_to_pad = padded - output_width();
	}
	void set_alignment(uint32_t alignment) { // encoding.h:70-72
		const uint32_t a = std::lcm(alignment, required_output_alignment());
		set_padded_output_width(next_multiple(output_width(), a));
	}
	virtual size_t n_params() const { return 0; }
	virtual void initialize_params(Pcg32& rng, float* params_full_precision, float scale) {}
	// out: [n][padded_output_width] T (T = float if fp32 else half)
	// prepare_param_gradients: a backward pass with parameter gradients will follow (lets the grid record its scatter filter); plan (optional): ForwardPlan
	virtual EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan = nullptr) = 0;
	// dL_dy [n][padded] T; grads: T[n_params] or nullptr (Ignore)
	// route: this encoding's backward_route() for this pass -- the form dL_dy has and, for a grid, its gradient kernel; handoff (optional): BackwardHandoff
	virtual void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute& route, BackwardHandoff* handoff = nullptr) = 0;
	// How backward() will run for this context, asked once per pass in front of whatever produces dL_dy; offer: the richest form the caller can deliver it in
	virtual GridBackwardRoute backward_route(const Switches& sw, hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, GridDyForm offer, bool want_dL_dx, GradientMode mode) { return {}; }
	void backward_rows(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) {
		backward(stream, ctx, n, x, dL_dy, dL_dx, params, grads, mode, backward_route(switches(), stream, ctx, n, x, GridDyForm::Rows, dL_dx != nullptr, mode));
	}
	// second-order input gradients (object.h:278-288), with v = dL_ddLdx [n][d_in] fp32 and d = dL_dy [n][padded] T:
	//   dL_ddLdy [n][padded] T = J v (the tangent; exactly zero in the padding columns), dL_dx = d/dx <v, J^T d> in fp32 through the view,
	//   grads = d/dparams of the same by `mode`.  Null results (and Ignore) are not computed; dL_dy may be null when only dL_ddLdy is asked for.
	// Provided by the grid encoding (grid.h:902-1026), PPNG3 (ppng_3.h:609-676), Identity, Frequency, TriangleWave, SphericalHarmonics,
	// Empty, and a Composite of those (any reduction).  OneBlob, PPNG1 and PPNG2 have none.
	virtual void backward_backward_input(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                                     MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) {
		throw std::runtime_error{"DifferentiableObject::backward_backward_input_impl: not implemented error"};
	}
	// false: backward_backward_input() throws the error above.  A model that puts more passes around the encoding's asks first, so that
	// the error comes before anything of its own is allocated or launched (NetworkWithInputEncoding).
	virtual bool has_second_order() const { return false; }
	virtual bool second_order_reads_dL_dy() const { return true; } // false: backward_backward_input() needs no dL_dy (dL/dx is linear in x)
	// input_jvp: the tangent alone, t [n][padded] T = J v for v [n][d_in] fp32 (exactly zero in the padding columns), on the context of a
	// forward(prepare_input_gradients).  Every encoding with a second-order pass has it there -- backward_backward_input() asked for
	// dL_ddLdy only, so that t is that pass's dL_ddLdy bit for bit; OneBlob has a kernel for it; PPNG1 / PPNG2 have none.
	virtual bool has_tangent() const { return has_second_order(); }
	virtual void tangent(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView v, void* t, const void* params) {
		backward_backward_input(stream, ctx, n, x, v, nullptr, t, nullptr, params, nullptr, GradientMode::Ignore);
	}
	// true: the encoding is half(x * scale + offset) padded with ones -- cheap enough to apply inside the consumer's load
	virtual bool as_identity(float& scale, float& offset) const { return false; }
	// n_bins if this is a half-precision OneBlob encoding the MLP kernels can evaluate inside their input load (MlpIo::x_oneblob_bins), else 0
	virtual uint32_t as_oneblob() const { return 0; }
	virtual uint64_t scatter_wide_fallbacks() { return 0; }      // grid only: tasks of the list-fed scatter that had to take the 64-bit passes
	virtual uint64_t list_scatters() const { return 0; }         // grid only: backward passes that ran the list-fed scatter (k_grid_scatter_lists)
	// How a batch will be produced, asked before the forward pass (grid_forward_route; as_planes: the caller takes level planes where the kernel is Planes, through a ForwardPlan)
	virtual GridForwardRoute forward_route(const Switches& sw, uint32_t n, bool as_planes, bool prepare_input_gradients, bool prepare_param_gradients) const { return {}; }
	virtual Json hyperparams() const = 0;
	bool fp32() const { return m_fp32; }
	// max_level of the grid encodings (grid_interface.h:101-123), read at call time.  false: no grid encoding here to take it.
	// per_sample: n floats in device memory for every call made while it is set (the caller's; nullptr: the scalar applies)
	virtual bool set_max_level(float max_level) { return false; }
	virtual bool set_max_level_gpu(const float* per_sample) { return false; }
	virtual bool get_max_level(float& max_level, const float*& per_sample) const { return false; }
protected:
	explicit Encoding(bool fp32) : m_fp32{fp32} {}
	bool m_fp32;
	uint32_t m_n_to_pad = 0;
};

inline GridType string_to_grid_type(const std::string& s) {
	if (equals_case_insensitive(s, "Hash")) return GridType::Hash;
	if (equals_case_insensitive(s, "Dense")) return GridType::Dense;
	if (equals_case_insensitive(s, "Tiled") || equals_case_insensitive(s, "Tile")) return GridType::Tiled;
	throw std::runtime_error{"Invalid grid type: " + s};
}
inline HashType string_to_hash_type(const std::string& s) {
	if (equals_case_insensitive(s, "Prime")) return HashType::Prime;
	if (equals_case_insensitive(s, "CoherentPrime")) return HashType::CoherentPrime;
	if (equals_case_insensitive(s, "ReversedPrime")) return HashType::ReversedPrime;
	if (equals_case_insensitive(s, "Rng")) return HashType::Rng;
	throw std::runtime_error{"Invalid hash type: " + s};
}
inline InterpolationType string_to_interpolation_type(const std::string& s) {
	if (equals_case_insensitive(s, "Nearest")) return InterpolationType::Nearest;
	if (equals_case_insensitive(s, "Linear")) return InterpolationType::Linear;
	if (equals_case_insensitive(s, "Smoothstep")) return InterpolationType::Smoothstep;
	throw std::runtime_error{"Invalid interpolation type: " + s};
}

class GridEncoding : public Encoding {
public:
	GridEncoding(uint32_t n_dims_to_encode, const Json& enc, bool fp32) : Encoding{fp32} { // grid.h:1143-1208 + :668-730
		const uint32_t F = enc.value("n_features_per_level", 2u);
		if (F != 1 && F != 2 && F != 4 && F != 8) throw std::runtime_error{"GridEncoding: n_features_per_level must be 1, 2, 4, or 8."};
		const uint32_t log2_hashmap_size = enc.value("log2_hashmap_size", 19u);
		const std::string encoding_type = enc.value("otype", "Grid");
		const std::string default_type = equals_case_insensitive(encoding_type, "TiledGrid") ? "Tiled" : (equals_case_insensitive(encoding_type, "DenseGrid") ? "Dense" : "Hash");
		uint32_t n_features;
		if (enc.contains("n_features") || enc.contains("n_grid_features")) {
			n_features = enc.contains("n_features") ? enc.value("n_features", 0u) : enc.value("n_grid_features", 0u);
			if (enc.contains("n_levels")) throw std::runtime_error{"GridEncoding: may not specify n_features and n_levels simultaneously (one determines the other)"};
		} else {
			n_features = F * enc.value("n_levels", 16u);
		}
		const uint32_t n_levels = n_features / F;
		const GridType grid_type = string_to_grid_type(enc.value("type", default_type));
		const uint32_t base_resolution = enc.value("base_resolution", 16u);
		const float per_level_scale = enc.value("per_level_scale", grid_type == GridType::Dense ? std::exp(std::log(256.0f / (float)base_resolution) / (n_levels - 1)) : 2.0f);
		const HashType hash_type = string_to_hash_type(enc.value("hash", "CoherentPrime"));
		m_stochastic_interpolation = enc.value("stochastic_interpolation", false); // grid.h:284-298: read by the parameter-gradient pass alone (GridBackwardRoute::stochastic)
		if (n_dims_to_encode < 1 || n_dims_to_encode > GRID_MAX_DIMS) throw std::runtime_error{"GridEncoding: number of input dims must be 2 or 3."}; // (grid.h:1181: the reference's text)
		if (n_levels > MAX_N_LEVELS) throw std::runtime_error{"GridEncoding: m_n_levels must be at most MAX_N_LEVELS=128"};
		if (n_features % F != 0) throw std::runtime_error{"GridEncoding: n_features must be a multiple of N_FEATURES_PER_LEVEL"};

		m_n_features = n_features;
		m_log2_hashmap_size = log2_hashmap_size;
		m_base_resolution = base_resolution;
		m_per_level_scale = per_level_scale;

		memset(&m_meta, 0, sizeof(m_meta));
		m_meta.n_pos_dims = n_dims_to_encode;
		m_meta.n_features_per_level = F;
		m_meta.n_levels = n_levels;
		m_meta.grid_type = (uint32_t)grid_type;
		m_meta.hash_type = (uint32_t)hash_type;
		m_meta.interpolation = (uint32_t)string_to_interpolation_type(enc.value("interpolation", "Linear"));
		static const uint32_t prime[7] = {1958374283u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};
		static const uint32_t coherent[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};
		static const uint32_t reversed[7] = {2165219737u, 1434869437u, 2097192037u, 3674653429u, 805459861u, 2654435761u, 1958374283u};
		const uint32_t* primes = hash_type == HashType::Prime ? prime : (hash_type == HashType::ReversedPrime ? reversed : coherent);
		for (uint32_t d = 0; d < GRID_MAX_DIMS; ++d) m_meta.primes[d] = primes[d]; // common_device.h:645-661

		const float log2_scale = std::log2(per_level_scale); // float overload (grid.h:694)
		uint32_t offset = 0;
		for (uint32_t i = 0; i < n_levels; ++i) {
			const float scale = exp2f(i * log2_scale) * base_resolution - 1.0f; // common_device.h:709-714
			const uint32_t resolution = (uint32_t)ceilf(scale) + 1;             // :716-718
			const uint32_t max_params = std::numeric_limits<uint32_t>::max() / 2;
			uint32_t params_in_level = std::pow((float)resolution, n_dims_to_encode) > (float)max_params ? max_params : powi(resolution, n_dims_to_encode);
			params_in_level = next_multiple(params_in_level, 8u);
			if (grid_type == GridType::Tiled) params_in_level = std::min(params_in_level, powi(base_resolution, n_dims_to_encode));
			else if (grid_type == GridType::Hash) params_in_level = std::min(params_in_level, 1u << log2_hashmap_size);

			GridLevel& lv = m_meta.levels[i];
			lv.offset = offset;
			lv.size = params_in_level;
			lv.scale = scale;
			// grid_index's stride loop (common_device.h:692-704), evaluated once here, uint32 wrap-around included
			uint32_t stride = 1;
			for (uint32_t d = 0; d < GRID_MAX_DIMS; ++d) lv.stride[d] = 0;
			for (uint32_t d = 0; d < n_dims_to_encode && stride <= params_in_level; ++d) {
				lv.stride[d] = stride;
				stride *= resolution;
			}
			lv.hashed = (grid_type == GridType::Hash && params_in_level < stride) ? 1u : 0u;
			lv.size_mask = (params_in_level & (params_in_level - 1)) == 0 ? params_in_level - 1 : 0;
			m_resolutions.push_back(resolution);
			offset += params_in_level;
		}
		m_n_entries = offset;
		m_n_params = (size_t)offset * F;
		if (F >= 2) {
			grid_scatter_setup_levels(m_meta);
			for (uint32_t i = 0; i < n_levels; ++i) {
				// the sample filter describes 64 chunks per level; levels cut finer go through the binned kernels (up to 4096 chunks)
				m_scatter_levels_ok &= m_meta.levels[i].scatter_binned || m_meta.levels[i].scatter_n_chunks <= grid_scatter_max_chunks();
				m_any_binned |= m_meta.levels[i].scatter_binned != 0;
			}
		}
	}

	// device copy of the level table, uploaded on first use (construction itself never touches the GPU)
	const GridMeta* dev_meta() {
		if (!m_dev_meta.data()) {
			m_dev_meta.resize(sizeof(GridMeta));
			HIP_CHECK_THROW(hipMemcpy(m_dev_meta.data(), &m_meta, sizeof(GridMeta), hipMemcpyHostToDevice));
		}
		return (const GridMeta*)m_dev_meta.data();
	}

	static uint32_t powi(uint32_t base, uint32_t exponent) {
		uint32_t result = 1;
		for (uint32_t i = 0; i < exponent; ++i) result *= base;
		return result;
	}

	uint32_t input_width() const override { return m_meta.n_pos_dims; }
	uint32_t output_width() const override { return m_n_features; }
	uint32_t required_output_alignment() const override { return m_meta.n_features_per_level; }
	size_t n_params() const override { return m_n_params; }
	const GridMeta& meta() const { return m_meta; }
	const std::vector<uint32_t>& resolutions() const { return m_resolutions; }

	void initialize_params(Pcg32& rng, float* params_full_precision, float scale) override { // grid.h:1059-1062
		generate_random_uniform(nullptr, rng.st, n_params(), params_full_precision, -1e-4f * scale, 1e-4f * scale);
	}

	EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan) override {
		EncodingContext ctx;
		if ((!out && !prepare_input_gradients) || padded_output_width() == 0 || n == 0) return ctx;
		// The encoded batch as a matrix (callers with their own network: the PyTorch Encoding module, a grid nested in a Composite): the level-plane
		// kernel -- XCD-aware, and the one that writes the hit lists the fast gradient kernel reads -- and a transposition behind it, instead of
		// the AoS kernel and the bit-plane gradient kernel (3-D, F = 2, 2^18 samples through the PyTorch module: 1.74 -> 0.42 ms forward + backward; a Composite of such a grid and spherical harmonics in front of a 64x2 network: 1.89 -> 0.49 ms per training step).
		const GridForwardRoute route = plan ? plan->route : forward_route(switches(), n, false, prepare_input_gradients, prepare_param_gradients);
		if (route.kernel == GridForwardKernel::Planes) return forward_planes(stream, route, n, x, params, out, plan->prep_job, plan->item_map);
		if (route.kernel == GridForwardKernel::PlanesToRows) {
			ArenaBuf planes{stream, (size_t)n * padded_output_width() * sizeof(uint16_t)};
			ctx = forward_planes(stream, route, n, x, params, planes.data());
			grid_planes_to_rows(stream, m_meta, n, padded_output_width(), planes.data(), out, padded_output_width()); // (the planes of zeros behind the levels' included)
			return ctx;
		}
		ctx.route = route;
		if (prepare_input_gradients) ctx.dy_dx = ArenaBuf{stream, (size_t)n * m_n_features * m_meta.n_pos_dims * sizeof(float)};
		const bool want_filter = route.recorded == GridRecorded::BitPlanes;
		ArenaBuf mask;
		if (want_filter) mask = ArenaBuf{stream, (size_t)m_meta.n_levels * n * (GRID_FILTER_MAX_CHUNKS / 64) * sizeof(uint64_t)};
		grid_forward(stream, m_meta, dev_meta(), m_fp32, n, x, params, out, padded_output_width(), ctx.dy_dx.as<float>(), mask.as<uint64_t>());
		if (max_level_forward_active()) { // grid.h:67-90: an off level writes zeros into its features and into dy_dx
			const uint32_t F = m_meta.n_features_per_level, D = m_meta.n_pos_dims;
			if (out) zero_levels(stream, m_fp32 ? 4 : 2, n, F, padded_output_width(), F, out, false);
			if (ctx.dy_dx) zero_levels(stream, 4, n, F * D, (uint64_t)m_n_features * D, (uint64_t)F * D, ctx.dy_dx.data(), false);
		}
		if (want_filter) {
			ctx.chunk_mask = ArenaBuf{stream, (size_t)m_meta.n_levels * grid_scatter_max_chunks() * (n / 64) * sizeof(uint64_t)};
			ctx.n = n;
			grid_mask_to_bits(stream, m_meta, dev_meta(), n, mask.as<uint64_t>(), ctx.chunk_mask.as<uint64_t>());
		}
		return ctx;
	}

	GridFacts facts() const { return GridFacts{&m_meta, m_fp32, m_scatter_levels_ok, m_any_binned, m_n_to_pad, m_stochastic_interpolation}; }
	GridForwardRoute forward_route(const Switches& sw, uint32_t n, bool as_planes, bool prepare_input_gradients, bool prepare_param_gradients) const override {
		return grid_forward_route(facts(), sw, n, as_planes, prepare_input_gradients, prepare_param_gradients);
	}

	struct PlanesPlan {
		DeviceBuf dev_work;
		uint32_t max_items = 0, blocks_per_xcd = 0;
	};
	PlanesPlan& planes_plan(uint32_t n_, bool hit_lists) {
		const uint32_t n = n_ | (hit_lists ? 0x80000000u : 0u); // (key; n itself is below 2^24 + 1)
		auto it = m_planes_plans.find(n);
		if (it != m_planes_plans.end()) return *it->second;
		auto plan = std::make_unique<PlanesPlan>();
		std::vector<uint32_t> work;
		grid_planes_plan(m_meta, n_, hit_lists, work, plan->max_items, plan->blocks_per_xcd);
		plan->dev_work.resize(work.size() * sizeof(uint32_t));
		HIP_CHECK_THROW(hipMemcpy(plan->dev_work.data(), work.data(), work.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
		return *(m_planes_plans[n] = std::move(plan));
	}

	EncodingContext forward_planes(hipStream_t stream, const GridForwardRoute& route, uint32_t n, MatView x, const void* params, void* out_planes,
	                               const MlpPrepJob* prep_job = nullptr, const GridItemMap* item_map = nullptr) {
		EncodingContext ctx;
		CHECK_THROW(route.planned && route.kernel != GridForwardKernel::Rows);
		ctx.route = route;
		const bool want_lists = route.recorded == GridRecorded::HitLists;
		if (want_lists) {
			// Hit lists (k_grid_scatter_lists.hip): the storage is this pass's own; the stragglers' counts live in one of the stream's two
			// counter sets -- this launch counts in one and zeroes the other for the next forward pass, so no memset sits between the steps.
			HitCounters& hc = hit_counters(stream);
			GridHitLists& hl = ctx.hit_lists;
			hl.item_samples = grid_hit_item_samples(m_meta);
			hl.n_items = div_round_up(n, hl.item_samples);
			hl.item_capacity = hl.item_samples << (m_meta.n_pos_dims - 1);
			hl.straggler_capacity = n << (m_meta.n_pos_dims - 1);
			// an item is what one workgroup of the MLP kernel produces where the two sizes agree, else item_samples consecutive samples
			hl.map = grid_item_map(hl.item_samples, 0, 1);
			if (item_map && item_map->n_windows > 1 && item_map->window * item_map->n_windows == hl.item_samples && n % hl.item_samples == 0 &&
			    item_map->stride == hl.n_items * item_map->window && item_map->window % (64 * grid_planes_spt(m_meta)) == 0) hl.map = *item_map;
			const size_t L = m_meta.n_levels;
			const size_t elems_bytes = L * hl.n_items * hl.item_capacity * GRID_HIT_WORDS * sizeof(uint32_t), sidx_bytes = next_multiple_sz(L * hl.n_items * hl.item_capacity * sizeof(uint16_t), 256);
			const size_t heads_bytes = next_multiple_sz(L * hl.n_items * GRID_HIT_HEADS * sizeof(uint32_t), 256);
			ctx.hit_elems = ArenaBuf{stream, elems_bytes + sidx_bytes + heads_bytes + L * hl.straggler_capacity * 2 * sizeof(uint32_t)};
			hl.elems = ctx.hit_elems.as<uint32_t>();
			hl.sidx = (uint16_t*)((char*)ctx.hit_elems.data() + elems_bytes);
			hl.heads = (uint32_t*)((char*)ctx.hit_elems.data() + elems_bytes + sidx_bytes);
			hl.stragglers = (uint32_t*)((char*)ctx.hit_elems.data() + elems_bytes + sidx_bytes + heads_bytes);
			hl.counts = hc.sets[hc.next].as<uint32_t>();
			hl.zero_counts = hc.sets[hc.next ^ 1].as<uint32_t>();
			hc.next ^= 1;
			if (const char* e = lab_env("TCNN_AMD_FWD_LISTS_DEV")) hl.dev_flags = (uint32_t)atoi(e); // 1: no copy-out, 2: plain instead of streamed stores, 4: no offsets (1 and 4: wrong results)
			ctx.hit_generation = ++hc.generation;
			ctx.hit_stream = (const void*)stream;
			ctx.n = n;
		} else if (route.recorded == GridRecorded::BitPlanes) {
			ctx.chunk_mask = ArenaBuf{stream, (size_t)m_meta.n_levels * grid_scatter_max_chunks() * (n / 64) * sizeof(uint64_t)};
			ctx.n = n;
		}
		PlanesPlan& plan = planes_plan(n, want_lists);
		grid_forward_planes(stream, m_meta, dev_meta(), plan.dev_work.as<uint32_t>(), plan.max_items, plan.blocks_per_xcd, n, x, params, out_planes, ctx.chunk_mask.as<uint64_t>(), prep_job,
		                    want_lists ? &ctx.hit_lists : nullptr);
		if (m_n_to_pad) HIP_CHECK_THROW(hipMemsetAsync((uint16_t*)out_planes + (size_t)n * m_n_features, 0, (size_t)n * m_n_to_pad * sizeof(uint16_t), stream)); // grid.h:749-759: the grid pads with zeros
		if (max_level_forward_active()) { // grid.h:67-90 (hit lists and chunk masks stay those of every level: the gradient side decides for itself)
			const uint32_t F = m_meta.n_features_per_level;
			zero_levels(stream, 2, n, F, F, (uint64_t)n * F, out_planes, false);
		}
		return ctx;
	}

	// hit lists of this very batch, their counters not yet handed to a later forward pass of this stream
	bool lists_current(hipStream_t stream, const EncodingContext& ctx, uint32_t n) { return ctx.hit_elems && ctx.n == n && ctx.hit_stream == (const void*)stream && hit_counters(stream).generation == ctx.hit_generation; }
	// (a per-sample array overrides the scalar)
	GridMaxLevel max_level_state() const { return m_max_level_gpu ? GridMaxLevel::PerSample : (levels_on(true) < m_meta.n_levels ? GridMaxLevel::Scalar : GridMaxLevel::None); }
	GridBackwardRoute backward_route(const Switches& sw, hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, GridDyForm offer, bool want_dL_dx, GradientMode mode) override {
		GridBackwardRoute r = grid_backward_route(facts(), sw, ctx.route, lists_current(stream, ctx, n), n, offer, want_dL_dx, mode, max_level_state(), x.stride_dim == 1 && x.stride_sample == m_meta.n_pos_dims);
		const GridHitLists& hl = ctx.hit_lists;
		r.tail = r.tail && hl.map.n_windows >= 2 && hl.n_items * hl.item_samples == n; // (items formed from an MLP kernel's workgroups: forward_planes)
		if (r.tail) {
			r.list_tail.sidx = hl.sidx, r.list_tail.heads = hl.heads, r.list_tail.map = hl.map;
			r.list_tail.n_items = hl.n_items, r.list_tail.item_capacity = hl.item_capacity;
			r.tail_bytes = grid_list_gradients_bytes(m_meta, hl);
		}
		return r;
	}

	void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute& route, BackwardHandoff* handoff) override {
		if ((!dL_dx && mode == GradientMode::Ignore) || n == 0) return;
		const BackwardHandoff offer = handoff ? *handoff : BackwardHandoff{};
		const auto all_levels = [&](const void* dy) { // (reports through the caller's hand-off, if there is one)
			const bool carried = backward_all_levels(stream, ctx, n, x, dy, dL_dx, params, grads, mode, route, offer);
			if (handoff) handoff->reduce_carried = carried;
		};
		const GridMaxLevel max_level = max_level_state();
		if (max_level == GridMaxLevel::None) return all_levels(dL_dy);
		if (max_level == GridMaxLevel::PerSample) { // dL/dy of the skipped (sample, level) pairs zeroed -- the exact sums add nothing for a zero product
			const uint32_t F = m_meta.n_features_per_level;
			const bool dy_planes = route.dy == GridDyForm::Planes; // (never records, never the MLP kernel's tail: the route sees the array)
			const size_t elem = dy_planes ? 2 : (m_fp32 ? 4 : 2);
			ArenaBuf masked{stream, (size_t)n * padded_output_width() * elem};
			zero_levels(stream, elem, n, F, dy_planes ? F : padded_output_width(), dy_planes ? (uint64_t)n * F : F, masked.data(), true, dL_dy);
			return all_levels(masked.data());
		}
		// scalar (grid.h:237-245): the route declines the optimizer's prologue and the MLP kernel's tail -- the off levels' gradients are
		// settled below, after the kernels, and the optimizer's own launch sees every parameter
		GradientTail tail{*this, stream, grads, mode, levels_on(true)};
		all_levels(dL_dy);
		tail.settle();
	}

	// a dispatch on the route's kernel; returns whether offer.reduce_job was carried: by a launch of this pass, or handed on with the prologue
	bool backward_all_levels(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode,
	                         const GridBackwardRoute& route, const BackwardHandoff& offer) {
		const uint32_t F = m_meta.n_features_per_level;
		const bool dy_planes = route.dy != GridDyForm::Rows, accumulate = mode == GradientMode::Accumulate;
		uint32_t dy_stride_sample = dy_planes ? F : padded_output_width(), dy_stride_level = dy_planes ? n * F : F;
		bool carried = false;
		if (mode != GradientMode::Ignore) CHECK_THROW(grads != nullptr && route.kernel != GridGradientKernel::None); // (a route of backward_route())
		switch (mode == GradientMode::Ignore ? GridGradientKernel::None : route.kernel) {
		case GridGradientKernel::None: break;
		case GridGradientKernel::AtomicScratch32: { // grid.h:660: F == 1 accumulates in fp32
			ArenaBuf tmp{stream, n_params() * sizeof(float)};
			if (mode == GradientMode::Overwrite) HIP_CHECK_THROW(hipMemsetAsync(tmp.data(), 0, n_params() * sizeof(float), stream));
			else cast_half_to_float(stream, n_params(), grads, tmp.as<float>());
			grid_backward(stream, m_meta, dev_meta(), true, n, x, dL_dy, false, padded_output_width(), tmp.data(), route.stochastic);
			cast_float_to_half(stream, n_params(), tmp.as<float>(), grads);
		} break;
		case GridGradientKernel::Atomic:
			if (mode == GradientMode::Overwrite) HIP_CHECK_THROW(hipMemsetAsync(grads, 0, n_params() * (m_fp32 ? 4 : 2), stream)); // grid.h:858
			grid_backward(stream, m_meta, dev_meta(), m_fp32, n, x, dL_dy, m_fp32, padded_output_width(), grads, route.stochastic);
			break;
		case GridGradientKernel::Lists: { // k_grid_scatter_lists.hip: a static plan, nothing to tune
			CHECK_THROW(!route.stochastic); // (list elements carry all 2^D corners with their weights: grid_backward_route)
			ScatterPlan& plan = scatter_plan(n, stream, true);
			// dL/dy as rows (a caller's own network): into level planes first -- the streamed tasks read a level's gradients sample after
			// sample, 4 bytes out of every row's 64 otherwise (2^18 samples: the owners 82 us from rows, 42 from planes; the transposition 12)
			ArenaBuf dy_as_planes;
			const void* dy_src = dL_dy;
			if (!dy_planes && grid_planes_to_rows_supported(m_meta, n, m_n_features)) {
				dy_as_planes = ArenaBuf{stream, (size_t)n * m_n_features * sizeof(uint16_t)};
				grid_rows_to_planes(stream, m_meta, n, m_n_features, dL_dy, padded_output_width(), dy_as_planes.data());
				dy_src = dy_as_planes.data(), dy_stride_sample = F, dy_stride_level = n * F;
			}
			++m_list_scatters;
			const bool defer = take_prologue(route, offer, plan, grads, mode);
			// dL/dy in list order: written and read by the two kernels of this call -- or written by the MLP kernel's tail already
			const bool filled = offer.list_gradients != nullptr;
			ArenaBuf gvals;
			if (!filled) gvals = ArenaBuf{stream, grid_list_gradients_bytes(m_meta, ctx.hit_lists)};
			carried = grid_backward_lists(stream, m_meta, dev_meta(), plan.dev_tasks.as<GridScatterTask>(), plan.n_tasks, plan.dev_ranges.as<GridScatterRange>(), defer ? 0u : plan.n_ranges,
			                              plan.scratch.as<uint64_t>(), n, x, dy_src, dy_stride_sample, dy_stride_level, grads, ctx.hit_lists, filled ? offer.list_gradients : gvals.data(), accumulate,
			                              defer ? nullptr : offer.reduce_job, hit_counters(stream).fallbacks.as<uint32_t>(), filled) ||
			          (defer && offer.reduce_job); // (it went with the prologue)
		} break;
		case GridGradientKernel::BitPlanes: { // k_grid_scatter.hip
			ScatterPlan& plan = scatter_plan(n, stream, false);
			const uint64_t* mask = (ctx.chunk_mask && ctx.n == n) ? ctx.chunk_mask.as<uint64_t>() : nullptr;
			// The second filtered launch at this batch size is timed per task and the plan re-cut from the measured
			// per-level work (grid_scatter_plan): one stream synchronisation, once per (encoding, batch size).
			const bool tune = route.tune && !plan.tuned && mask && plan.n_tasks > 0 && ++plan.launches == 2;
			DeviceBuf times;
			if (tune) {
				times.resize((size_t)plan.n_tasks * 8 * sizeof(uint64_t));
				times.memset(0);
			}
			// (not in the step whose launch is timed for the tuner: the plan, ranges and scratch included, is rebuilt right after it)
			const bool defer = !tune && take_prologue(route, offer, plan, grads, mode);
			carried = grid_backward_lds(stream, m_meta, dev_meta(), plan.dev_tasks.as<GridScatterTask>(), plan.n_tasks, plan.dev_ranges.as<GridScatterRange>(), defer ? 0u : plan.n_ranges,
			                            plan.scratch.as<uint64_t>(), n, x, dL_dy, dy_stride_sample, dy_stride_level, grads, mask, accumulate, route.dy == GridDyForm::Records,
			                            tune ? times.as<uint64_t>() : nullptr, defer ? nullptr : offer.reduce_job, route.stochastic) ||
			          (defer && offer.reduce_job); // (it went with the prologue)
			if (route.binned) { // levels cut into more than 64 chunks (k_grid_bin.hip)
				ArenaBuf workspace{stream, grid_bin_workspace_bytes(m_meta, n)};
				grid_backward_binned(stream, m_meta, dev_meta(), n, x, dL_dy, dy_stride_sample, dy_stride_level, grads, accumulate, workspace.data(), hit_counters(stream).fallbacks.as<uint32_t>(), route.stochastic);
			}
			if (tune) {
				HIP_CHECK_THROW(hipStreamSynchronize(stream));
				std::vector<uint64_t> h((size_t)plan.n_tasks * 8);
				HIP_CHECK_THROW(hipMemcpy(h.data(), times.data(), h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
				const std::vector<float> level_us = grid_scatter_level_costs(m_meta, plan.host_tasks, h);
				build_scatter_plan(plan, n, &level_us);
				plan.tuned = true;
			}
		} break;
		}
		if (dL_dx) {
			CHECK_THROW(ctx.dy_dx);
			grid_backward_input(stream, m_meta, m_fp32, n, dL_dy, padded_output_width(), ctx.dy_dx.as<float>(), *dL_dx);
		}
		return carried;
	}

	// grid.h:902-1026
	bool has_second_order() const override { return true; }
	void backward_backward_input(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                             MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) override {
		if ((!dL_ddLdy && mode == GradientMode::Ignore && !dL_dx) || padded_output_width() == 0 || n == 0) return;
		const uint32_t l_bwd = m_max_level_gpu ? m_meta.n_levels : levels_on(true);
		if (!m_max_level_gpu && l_bwd == m_meta.n_levels) return backward_backward_input_all_levels(stream, ctx, n, x, dL_ddLdx, dL_dy, dL_ddLdy, dL_dx, params, grads, mode);
		// grid.h:377-384, :482-490: both kernels skip the (sample, level) pairs the gradient rule puts off -- a zero dL/dy there gives them
		// nothing (dL_ddLdy reads dy_dx, which the forward pass zeroed by the forward rule, :626-650)
		ArenaBuf masked;
		if (dL_dy) {
			const uint32_t F = m_meta.n_features_per_level;
			const size_t elem = m_fp32 ? 4 : 2;
			masked = ArenaBuf{stream, (size_t)n * padded_output_width() * elem};
			zero_levels(stream, elem, n, F, padded_output_width(), F, masked.data(), true, dL_dy);
			dL_dy = masked.data();
		}
		GradientTail tail{*this, stream, grads, mode, l_bwd};
		backward_backward_input_all_levels(stream, ctx, n, x, dL_ddLdx, dL_dy, dL_ddLdy, dL_dx, params, grads, mode);
		tail.settle();
	}

	void backward_backward_input_all_levels(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                                        MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) {
		const size_t elem = m_fp32 ? 4 : 2;
		if (dL_ddLdy) CHECK_THROW(ctx.dy_dx); // needs the forward pass to have run with prepare_input_gradients
		const float* dy_dx = ctx.dy_dx.as<float>();
		if (mode != GradientMode::Ignore) {
			CHECK_THROW(grads != nullptr);
			const bool scratch32 = !m_fp32 && m_meta.n_features_per_level == 1; // grid.h:660: F == 1 accumulates in fp32 and casts (:934-941, :971-975)
			if (scratch32) {
				ArenaBuf tmp{stream, n_params() * sizeof(float)};
				if (mode == GradientMode::Overwrite) HIP_CHECK_THROW(hipMemsetAsync(tmp.data(), 0, n_params() * sizeof(float), stream));
				else cast_half_to_float(stream, n_params(), grads, tmp.as<float>());
				grid_backward_backward_input(stream, m_meta, dev_meta(), false, true, n, x, dL_ddLdx, dL_dy, padded_output_width(), params, dy_dx, tmp.data(), nullptr, nullptr);
				cast_float_to_half(stream, n_params(), tmp.as<float>(), grads);
			} else {
				if (mode == GradientMode::Overwrite) HIP_CHECK_THROW(hipMemsetAsync(grads, 0, n_params() * elem, stream)); // grid.h:943-945
				grid_backward_backward_input(stream, m_meta, dev_meta(), m_fp32, m_fp32, n, x, dL_ddLdx, dL_dy, padded_output_width(), params, dy_dx, grads, nullptr, nullptr);
			}
		}
		if (dL_ddLdy || dL_dx) {
			grid_backward_backward_input(stream, m_meta, dev_meta(), m_fp32, m_fp32, n, x, dL_ddLdx, dL_dy, padded_output_width(), params, dy_dx, nullptr, dL_ddLdy, dL_dx);
		}
	}

	// the tasks of a gradient kernel and what goes with them; like the kernels it owns device state a launch leaves behind for the next one on
	// the same stream (the zeroed scratch table)
	struct ScatterPlan {
		DeviceBuf dev_tasks, dev_ranges, scratch;
		std::vector<GridScatterTask> host_tasks;
		std::vector<GridScatterRange> host_ranges;
		uint32_t n_tasks = 0, n_ranges = 0;
		uint32_t launches = 0;
		bool lists = false; // the list-fed kernel's plan: static, nothing to tune
		bool tuned = false;
	};
	// The optimizer's launch has offered to run this backward pass's finalize pass (offer.prologue): hand it the plan's shared ranges, their
	// scratch and the reduce job.  Only where the route allows it and there is something to finish: shared ranges or the job.
	bool take_prologue(const GridBackwardRoute& route, const BackwardHandoff& offer, const ScatterPlan& plan, void* grads, GradientMode mode) const {
		AdamPrologue* p = offer.prologue;
		if (!route.prologue || !p || p->pending || (plan.host_ranges.empty() && !offer.reduce_job)) return false;
		p->dev_ranges = plan.dev_ranges.as<GridScatterRange>();
		p->ranges = plan.host_ranges;
		p->scratch = plan.scratch.as<uint64_t>();
		p->grad_base = grads;
		p->accumulate = mode == GradientMode::Accumulate;
		p->has_reduce = offer.reduce_job != nullptr;
		if (offer.reduce_job) {
			p->reduce_elems = offer.reduce_job->n_elems;
			p->reduce_slabs = offer.reduce_job->n_slabs;
			p->slabs = offer.reduce_job->slabs;
			p->reduce_accumulate = offer.reduce_job->accumulate;
		}
		p->pending = true;
		return true;
	}

	// (re)builds the device-side plan -- the bit-plane kernel's tasks (grid_scatter_plan, re-cut once by the tuner) or the list-fed kernel's
	// (grid_scatter_lists_plan); the caller guarantees that no launch using the old one is still running
	void build_scatter_plan(ScatterPlan& plan, uint32_t n, const std::vector<float>* measured_level_us) {
		size_t scratch_elems = 0;
		if (plan.lists) grid_scatter_lists_plan(m_meta, n, plan.host_tasks, plan.host_ranges, scratch_elems);
		else grid_scatter_plan(m_meta, n, plan.host_tasks, plan.host_ranges, scratch_elems, measured_level_us);
		plan.n_tasks = (uint32_t)plan.host_tasks.size();
		plan.n_ranges = (uint32_t)plan.host_ranges.size();
		auto upload = [](DeviceBuf& b, const void* src, size_t bytes) {
			b.resize(bytes);
			if (bytes) HIP_CHECK_THROW(hipMemcpy(b.data(), src, bytes, hipMemcpyHostToDevice));
		};
		upload(plan.dev_tasks, plan.host_tasks.data(), plan.host_tasks.size() * sizeof(GridScatterTask));
		upload(plan.dev_ranges, plan.host_ranges.data(), plan.host_ranges.size() * sizeof(GridScatterRange));
		plan.scratch.resize(0);
		plan.scratch.resize(scratch_elems * sizeof(uint64_t));
		plan.scratch.memset(0); // the finalize pass leaves it zeroed again after every step
	}
	// One plan per (batch size, stream, kernel): a plan owns mutable device state -- the scratch table of the shared chunks, which a step
	// leaves zeroed for the next one, and the task list the tuner replaces after a stream synchronisation -- so two streams that
	// run backward passes of this encoding at the same time must not share one.  Steps on ONE stream are ordered and may.
	ScatterPlan& scatter_plan(uint32_t n, hipStream_t stream, bool lists) {
		const auto key = std::make_pair(n | (lists ? 0x80000000u : 0u), (const void*)stream); // (n itself is below 2^24 + 1)
		auto it = m_scatter_plans.find(key);
		if (it != m_scatter_plans.end()) return *it->second;
		auto plan = std::make_unique<ScatterPlan>();
		plan->lists = lists;
		build_scatter_plan(*plan, n, nullptr);
		return *(m_scatter_plans[key] = std::move(plan));
	}

	static size_t next_multiple_sz(size_t v, size_t m) { return (v + m - 1) / m * m; }
	struct HitCounters {
		DeviceBuf sets[2], fallbacks; // two sets of list tails [n_levels][GRID_HIT_COUNT_STRIDE]; how many tasks took the 64-bit passes
		int next = 0;
		uint64_t generation = 0;
	};
	HitCounters& hit_counters(hipStream_t stream) {
		auto it = m_hit_counters.find((const void*)stream);
		if (it != m_hit_counters.end()) return *it->second;
		auto hc = std::make_unique<HitCounters>();
		for (auto& set : hc->sets) {
			set.resize((size_t)m_meta.n_levels * GRID_HIT_COUNT_STRIDE * sizeof(uint32_t));
			set.memset(0);
		}
		hc->fallbacks.resize(sizeof(uint32_t));
		hc->fallbacks.memset(0);
		return *(m_hit_counters[(const void*)stream] = std::move(hc));
	}
public:
	// tasks of the list-fed scatter that found their packed 32-bit sums unprovable and ran the 64-bit passes, since this encoding was built (all streams)
	uint64_t scatter_wide_fallbacks() override {
		uint64_t total = 0;
		for (auto& kv : m_hit_counters) {
			uint32_t v = 0;
			HIP_CHECK_THROW(hipMemcpy(&v, kv.second->fallbacks.data(), sizeof(v), hipMemcpyDeviceToHost));
			total += v;
		}
		return total;
	}

	uint64_t list_scatters() const override { return m_list_scatters; }

	// grid_interface.h:101-123 (not part of the hyperparameters or snapshots, as there)
	bool set_max_level(float max_level) override { m_max_level = max_level; return true; }
	bool set_max_level_gpu(const float* per_sample) override { m_max_level_gpu = per_sample; return true; }
	bool get_max_level(float& max_level, const float*& per_sample) const override {
		max_level = m_max_level;
		per_sample = m_max_level_gpu;
		return true;
	}

	// The scalar cut-off's levels that produce output (gradient_rule false) or receive gradients (true); the off levels are a suffix.
	// The reference's fp32 expressions (grid.h:67-75, :237-245): m = (max_level * num_grid_features) / F, then l >= m + 1e-3f / l > m + 1e-3f.
	uint32_t levels_on(bool gradient_rule) const {
		const volatile float m = (m_max_level * (float)m_n_features) / (float)m_meta.n_features_per_level;
		const volatile float threshold = m + 1e-3f;
		for (uint32_t l = 0; l < m_meta.n_levels; ++l) {
			if (gradient_rule ? (float)l > threshold : (float)l >= threshold) return l;
		}
		return m_meta.n_levels;
	}
	bool max_level_forward_active() const { return m_max_level_gpu || levels_on(false) < m_meta.n_levels; }

private:
	// zeroes the off (sample, level) pairs of a forward output / dy_dx (gradient_rule false) or of a dL/dy copy (true), laid out as
	// data + i * sample_stride + l * level_stride, `width` elements per pair
	// src: a masked copy of src into data instead (the levels' elements only: padding features are left unwritten)
	void zero_levels(hipStream_t stream, size_t elem_bytes, uint32_t n, uint32_t width, uint64_t sample_stride, uint64_t level_stride, void* data, bool gradient_rule,
	                 const void* src = nullptr) const {
		const uint32_t level0 = m_max_level_gpu ? 0u : levels_on(gradient_rule);
		grid_zero_levels(stream, elem_bytes, n, m_meta.n_levels, level0, width, sample_stride, level_stride, data, src, m_max_level_gpu, m_n_features, m_meta.n_features_per_level, gradient_rule);
	}
	// The scalar cut-off skips the levels from l_bwd on: their parameter gradients, one contiguous tail, end up zero (Overwrite, grid.h:857)
	// or untouched (Accumulate, signed zeros included) whatever the gradient kernels wrote there.
	struct GradientTail {
		hipStream_t stream;
		char* tail = nullptr;
		size_t bytes = 0;
		bool accumulate = false;
		ArenaBuf saved;
		GradientTail(const GridEncoding& e, hipStream_t s, void* grads, GradientMode mode, uint32_t l_bwd) : stream{s} {
			if (!grads || mode == GradientMode::Ignore || l_bwd >= e.m_meta.n_levels) return;
			const size_t elem = e.m_fp32 ? 4 : 2, first = (size_t)e.m_meta.levels[l_bwd].offset * e.m_meta.n_features_per_level;
			tail = (char*)grads + first * elem;
			bytes = (e.n_params() - first) * elem;
			accumulate = mode == GradientMode::Accumulate;
			if (accumulate) {
				saved = ArenaBuf{stream, bytes};
				HIP_CHECK_THROW(hipMemcpyAsync(saved.data(), tail, bytes, hipMemcpyDeviceToDevice, stream));
			}
		}
		void settle() {
			if (!tail) return;
			if (accumulate) HIP_CHECK_THROW(hipMemcpyAsync(tail, saved.data(), bytes, hipMemcpyDeviceToDevice, stream));
			else HIP_CHECK_THROW(hipMemsetAsync(tail, 0, bytes, stream));
		}
	};

public:
	Json hyperparams() const override { // grid.h:1098-1115
		static const char* types[] = {"Hash", "Dense", "Tiled"};
		static const char* interps[] = {"Nearest", "Linear", "Smoothstep"};
		static const char* hashes[] = {"Prime", "CoherentPrime", "ReversedPrime", "Rng"};
		Json j = Json::object();
		j["otype"] = "Grid";
		j["type"] = types[m_meta.grid_type];
		j["n_levels"] = m_meta.n_levels;
		j["n_features_per_level"] = m_meta.n_features_per_level;
		j["base_resolution"] = m_base_resolution;
		j["per_level_scale"] = m_per_level_scale;
		j["interpolation"] = interps[m_meta.interpolation];
		j["hash"] = hashes[m_meta.hash_type];
		if (m_meta.grid_type == (uint32_t)GridType::Hash) j["log2_hashmap_size"] = m_log2_hashmap_size;
		return j;
	}

private:
	GridMeta m_meta;
	DeviceBuf m_dev_meta;
	std::map<std::pair<uint32_t, const void*>, std::unique_ptr<ScatterPlan>> m_scatter_plans;
	std::map<const void*, std::unique_ptr<HitCounters>> m_hit_counters;
	std::map<uint32_t, std::unique_ptr<PlanesPlan>> m_planes_plans;
	bool m_scatter_levels_ok = true;
	bool m_any_binned = false;
	uint64_t m_list_scatters = 0;
	float m_max_level = 1000.f;               // grid_interface.h:118: every level on
	const float* m_max_level_gpu = nullptr;   // grid_interface.h:119
	std::vector<uint32_t> m_resolutions;
	uint32_t m_n_features, m_log2_hashmap_size, m_base_resolution, m_n_entries;
	float m_per_level_scale;
	bool m_stochastic_interpolation;
	size_t m_n_params;
};

class OneBlobEncoding : public Encoding {
public:
	OneBlobEncoding(uint32_t n_bins, uint32_t n_dims_to_encode, bool fp32) : Encoding{fp32}, m_n_bins{n_bins}, m_n_dims{n_dims_to_encode} {
		if ((n_bins & (n_bins - 1)) != 0 || n_bins == 0) throw std::runtime_error{"Number of bins must be a power of 2"}; // oneblob.h:173-177
	}
	uint32_t input_width() const override { return m_n_dims; }
	uint32_t output_width() const override { return m_n_dims * m_n_bins; }
	uint32_t as_oneblob() const override { // Switches::fuse_oneblob off: always the encoding's own kernel (A/B runs, tests)
		return (!m_fp32 && m_n_bins >= 32 && switches().fuse_oneblob) ? m_n_bins : 0;
	}
	EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan) override {
		if (out && padded_output_width() > 0) oneblob_forward(stream, m_fp32, n, m_n_dims, m_n_bins, x, out, padded_output_width());
		return {};
	}
	void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute&, BackwardHandoff*) override {
		if (!dL_dx) return;
		oneblob_backward_input(stream, m_fp32, n, m_n_dims, m_n_bins, x, dL_dy, padded_output_width(), *dL_dx);
	}
	// no second-order pass (as in the reference), but a tangent: (T)(v k') with backward()'s k' (k_oneblob_tangent)
	bool has_tangent() const override { return true; }
	void tangent(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView v, void* t, const void* params) override {
		if (t && padded_output_width() > 0 && n > 0) oneblob_tangent(stream, m_fp32, n, m_n_dims, m_n_bins, x, v, t, padded_output_width());
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "OneBlob";
		j["n_bins"] = m_n_bins;
		return j;
	}
private:
	uint32_t m_n_bins, m_n_dims;
};

// dL_dx = 0 for n samples of n_dims input dims, whatever the view's layout
inline void zero_input_gradient(hipStream_t stream, uint32_t n, uint32_t n_dims, const MatViewMut& dL_dx) {
	if (n == 0 || n_dims == 0) return;
	const bool aos = dL_dx.stride_dim == 1 && dL_dx.stride_sample == n_dims, soa = dL_dx.stride_sample == 1 && dL_dx.stride_dim == n;
	if (aos || soa) {
		HIP_CHECK_THROW(hipMemsetAsync(dL_dx.data, 0, (size_t)n * n_dims * sizeof(float), stream));
	} else { // any other view: one strided column per input dim
		for (uint32_t d = 0; d < n_dims; ++d) {
			HIP_CHECK_THROW(hipMemset2DAsync(dL_dx.data + (size_t)d * dL_dx.stride_dim, (size_t)dL_dx.stride_sample * sizeof(float), 0, sizeof(float), n, stream));
		}
	}
}

// encodings/empty.h:58-150: encodes nothing -- its output is its padding, ones (e.g. as a placeholder inside a Composite); zero
// gradient towards its inputs.  (There output_width() reports the padded width; here it is 0 and the padding is the padding.)
class EmptyEncoding : public Encoding {
public:
	EmptyEncoding(uint32_t n_dims_to_encode, bool fp32) : Encoding{fp32}, m_n_dims{n_dims_to_encode} {}
	uint32_t input_width() const override { return m_n_dims; }
	uint32_t output_width() const override { return 0; }
	EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan) override {
		if (out && padded_output_width() > 0) identity_forward(stream, m_fp32, n, 0, 1.0f, 0.0f, x, out, padded_output_width()); // no live columns: all padding
		return {};
	}
	void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute&, BackwardHandoff*) override {
		if (dL_dx) zero_input_gradient(stream, n, m_n_dims, *dL_dx);
	}
	// the output is constant: a zero tangent over the padding and no Hessian term
	bool has_second_order() const override { return true; }
	bool second_order_reads_dL_dy() const override { return false; }
	void backward_backward_input(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                             MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) override {
		if (dL_ddLdy && padded_output_width() > 0 && n > 0) HIP_CHECK_THROW(hipMemsetAsync(dL_ddLdy, 0, (size_t)n * padded_output_width() * (m_fp32 ? 4 : 2), stream));
		if (dL_dx) zero_input_gradient(stream, n, m_n_dims, *dL_dx);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "Empty";
		return j;
	}
private:
	uint32_t m_n_dims;
};

// encodings/ppng.h:30-119 + ppng_1.h:215-379 (this fork's PPNG1: per frequency and phase a rank-R product of three 1-D tables
// looked up at sin(freq (x - 0.5) + phase); k_ppng.hip).  3 input dims, half precision; parameter gradients only, as there.
// PPNG2 (ppng_2.h:345-506) differs in the tables: three Q x Q planes per (frequency, phase, feature, rank) instead of three rows.
class PpngEncoding : public Encoding {
public:
	PpngEncoding(uint32_t variant, uint32_t n_dims_to_encode, const Json& enc, bool fp32) : Encoding{fp32}, m_variant{variant} {
		const std::string PPNG1 = variant == 3 ? std::string{"PPNG"} : "PPNG" + std::to_string(variant); // the messages name the variant (ppng_3.h:710, :721 say "PPNG")
		if (n_dims_to_encode != 3) throw std::runtime_error{PPNG1 + (variant == 3 ? ": number of input dims must be 2,3 or 4." : ": number of input dims must be 2 or 3")}; // ppng_1.h:370-376, ppng_3.h:717-722 (3 only)
		if (fp32) throw std::runtime_error{PPNG1 + ": this build provides the half-precision form"};
		m_log2_min_freq = (int32_t)enc.value("log2_min_freq", 0);
		m_log2_max_freq = (int32_t)enc.value("log2_max_freq", 6);
		m_n_quants = enc.value("n_quants", 64u);
		m_n_frequencies = enc.value("n_frequencies", 6u);
		m_rank = variant == 3 ? 1u : enc.value("rank", 4u);
		m_n_features = enc.value("n_features", 4u);
		if (variant != 3 && m_rank != 2 && m_rank != 4 && m_rank != 8 && m_rank != 16) throw std::runtime_error{PPNG1 + ": rank must be 1, 2, 4, 8 or 16"};
		if (variant == 3 && m_n_features == 1) throw std::runtime_error{"PPNG: this build provides 2, 4 or 8 features (the single-feature form sums fp32 products in arbitrary order there)"};
		if (m_n_features != 2 && m_n_features != 4 && m_n_features != 8) throw std::runtime_error{PPNG1 + ": number of features must be 1, 2, 4 or 8"};
		if (m_n_frequencies < 2 || m_n_quants < 2) throw std::runtime_error{PPNG1 + ": needs at least 2 frequencies and 2 quantisation bins"};
		if (variant == 3) { // ppng_3.h:489-494
			m_n_params = (size_t)m_n_frequencies * 2 * m_n_quants * m_n_quants * m_n_quants * m_n_features;
			if (m_n_params >= (1ull << 32)) throw std::runtime_error{"PPNG: the volume does not fit 32-bit offsets"};
		} else {
			m_n_params = (size_t)m_n_frequencies * 2 * 3 * m_n_features * m_n_quants * (variant == 2 ? m_n_quants : 1u) * m_rank;
		}
	}
	uint32_t input_width() const override { return 3; }
	uint32_t output_width() const override { return m_n_frequencies * 2 * m_n_features; }
	size_t n_params() const override { return m_n_params; }
	void initialize_params(Pcg32& rng, float* params_full_precision, float scale) override { // ppng_1.h:325-328; PPNG3 keeps the base class' range (ppng.h:66-69)
		const float range = m_variant == 3 ? 1e-4f : 0.7f;
		generate_random_uniform(nullptr, rng.st, n_params(), params_full_precision, -range * scale, range * scale);
	}
	EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan) override {
		if (out && padded_output_width() > 0 && n > 0) {
			if (m_variant == 3) ppng3_forward(stream, false, n, m_n_frequencies, m_n_quants, m_n_features, m_log2_min_freq, m_log2_max_freq, x, params, out, padded_output_width());
			else (m_variant == 2 ? ppng2_forward : ppng1_forward)(stream, false, n, m_n_frequencies, m_n_quants, m_n_features, m_rank, m_log2_min_freq, m_log2_max_freq, x, params, out, padded_output_width());
		}
		return {};
	}
	void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute&, BackwardHandoff*) override {
		if (dL_dx) {
			// PPNG1 / PPNG2: the reference leaves dL_dinput untouched (ppng_1.h:268-321 never writes it); PPNG3: ppng_3.h:586-607
			if (m_variant == 3 && padded_output_width() > 0) ppng3_backward_input(stream, false, n, m_n_frequencies, m_n_quants, m_n_features, m_log2_min_freq, m_log2_max_freq, x, params, dL_dy, padded_output_width(), *dL_dx);
			else zero_input_gradient(stream, n, 3, *dL_dx);
		}
		if (mode == GradientMode::Ignore || padded_output_width() == 0) return;
		CHECK_THROW(grads != nullptr);
		uint64_t* const scratch = scratch_for(stream);
		if (m_variant == 3) {
			const size_t ws_bytes = ppng3_backward_workspace_bytes(n, m_n_frequencies, m_n_quants, m_n_features);
			ArenaBuf ws = ws_bytes ? ArenaBuf{stream, ws_bytes} : ArenaBuf{};
			ppng3_backward(stream, false, n, m_n_frequencies, m_n_quants, m_n_features, m_log2_min_freq, m_log2_max_freq, x, dL_dy, padded_output_width(), ws.data(),
			               scratch, grads, mode == GradientMode::Accumulate);
			return;
		}
		(m_variant == 2 ? ppng2_backward : ppng1_backward)(stream, false, n, m_n_frequencies, m_n_quants, m_n_features, m_rank, m_log2_min_freq, m_log2_max_freq, x, params, dL_dy,
		                                                   padded_output_width(), scratch, grads, mode == GradientMode::Accumulate);
	}
	// ppng_3.h:609-676 (PPNG1 / PPNG2 have none)
	bool has_second_order() const override { return m_variant == 3; }
	void backward_backward_input(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                             MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) override {
		if (m_variant != 3) return Encoding::backward_backward_input(stream, ctx, n, x, dL_ddLdx, dL_dy, dL_ddLdy, dL_dx, params, grads, mode);
		if ((!dL_ddLdy && mode == GradientMode::Ignore && !dL_dx) || padded_output_width() == 0 || n == 0) return;
		uint64_t* scratch = nullptr;
		if (mode != GradientMode::Ignore) {
			CHECK_THROW(grads != nullptr);
			scratch = scratch_for(stream);
		}
		ppng3_backward_backward_input(stream, false, n, m_n_frequencies, m_n_quants, m_n_features, m_log2_min_freq, m_log2_max_freq, x, dL_ddLdx, params, dL_dy, padded_output_width(), scratch,
		                              mode != GradientMode::Ignore ? grads : nullptr, mode == GradientMode::Accumulate, dL_ddLdy, dL_dx);
	}
	Json hyperparams() const override { // ppng.h:92-103
		Json j = Json::object();
		j["otype"] = "PPNG" + std::to_string(m_variant);
		j["n_frequencies"] = m_n_frequencies;
		j["log2_min_freq"] = m_log2_min_freq;
		j["log2_max_freq"] = m_log2_max_freq;
		j["n_quants"] = m_n_quants;
		j["n_features_per_level"] = m_n_features;
		j["rank"] = m_rank;
		return j;
	}
private:
	uint64_t* scratch_for(hipStream_t stream) { // per stream: zero between passes (k_ppng_finalize)
		std::unique_ptr<DeviceBuf>& scratch = m_scratch[(const void*)stream];
		if (!scratch) {
			scratch = std::make_unique<DeviceBuf>(m_n_params * sizeof(uint64_t));
			scratch->memset(0);
		}
		return scratch->as<uint64_t>();
	}
	uint32_t m_variant;
	int32_t m_log2_min_freq, m_log2_max_freq;
	uint32_t m_n_quants, m_n_frequencies, m_rank, m_n_features;
	size_t m_n_params;
	std::map<const void*, std::unique_ptr<DeviceBuf>> m_scratch;
};

class IdentityEncoding : public Encoding {
public:
	IdentityEncoding(uint32_t n_dims_to_encode, float scale, float offset, bool fp32) : Encoding{fp32}, m_n_dims{n_dims_to_encode}, m_scale{scale}, m_offset{offset} {}
	uint32_t input_width() const override { return m_n_dims; }
	uint32_t output_width() const override { return m_n_dims; }
	bool as_identity(float& scale, float& offset) const override {
		scale = m_scale;
		offset = m_offset;
		return !m_fp32;
	}
	EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan) override {
		if (out && padded_output_width() > 0) identity_forward(stream, m_fp32, n, m_n_dims, m_scale, m_offset, x, out, padded_output_width());
		return {};
	}
	void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute&, BackwardHandoff*) override {
		if (!dL_dx) return;
		identity_backward_input(stream, m_fp32, n, m_n_dims, m_scale, dL_dy, padded_output_width(), *dL_dx);
	}
	// dL/dx = scale dL/dy is linear in dL/dy and does not depend on x: the tangent t = scale v (zero in the padding) is all there is
	bool has_second_order() const override { return true; }
	bool second_order_reads_dL_dy() const override { return false; }
	void backward_backward_input(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                             MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) override {
		if (dL_ddLdy && padded_output_width() > 0) identity_backward_backward_input(stream, m_fp32, n, m_n_dims, m_scale, dL_ddLdx, dL_ddLdy, padded_output_width());
		if (dL_dx) zero_input_gradient(stream, n, m_n_dims, *dL_dx);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "Identity";
		j["scale"] = m_scale;
		j["offset"] = m_offset;
		return j;
	}
private:
	uint32_t m_n_dims;
	float m_scale, m_offset;
};

// src/encoding.cu:144-158 (case-insensitive registry :48-54; default otype OneBlob)
// encodings/frequency.h:104-220 (two outputs per frequency: sin, cos) and encodings/triangle_wave.h:110-220 (one)
class PeriodicEncoding : public Encoding {
public:
	PeriodicEncoding(bool triangle, uint32_t n_frequencies, uint32_t n_dims_to_encode, bool fp32) : Encoding{fp32}, m_triangle{triangle}, m_n_frequencies{n_frequencies}, m_n_dims{n_dims_to_encode} {}
	uint32_t input_width() const override { return m_n_dims; }
	uint32_t outputs_per_input() const { return m_n_frequencies * (m_triangle ? 1u : 2u); }
	uint32_t output_width() const override { return m_n_dims * outputs_per_input(); }
	EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan) override {
		EncodingContext ctx;
		if (!out || padded_output_width() == 0 || n == 0) return ctx;
		if (prepare_input_gradients) ctx.dy_dx = ArenaBuf{stream, (size_t)n * output_width() * sizeof(float)};
		periodic_forward(stream, m_triangle, m_fp32, n, m_n_dims, m_n_frequencies, x, out, padded_output_width(), ctx.dy_dx.as<float>());
		return ctx;
	}
	void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute&, BackwardHandoff*) override {
		if (!dL_dx || n == 0) return;
		CHECK_THROW(ctx.dy_dx); // frequency.h:150-152: needs a forward pass with prepare_input_gradients
		periodic_backward_input(stream, m_fp32, n, m_n_dims, outputs_per_input(), dL_dy, padded_output_width(), ctx.dy_dx.as<float>(), *dL_dx);
	}
	// Frequency: tangent and Hessian term in one launch, from x (ctx.dy_dx is not read).  TriangleWave is piecewise linear: the tangent is all there is.
	bool has_second_order() const override { return true; }
	bool second_order_reads_dL_dy() const override { return !m_triangle; }
	void backward_backward_input(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                             MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) override {
		if (n == 0) return;
		if (dL_dx && (m_triangle || padded_output_width() == 0)) zero_input_gradient(stream, n, m_n_dims, *dL_dx);
		if (padded_output_width() == 0) return;
		periodic_backward_backward_input(stream, m_triangle, m_fp32, n, m_n_dims, m_n_frequencies, x, dL_ddLdx, dL_dy, dL_ddLdy, padded_output_width(), m_triangle ? nullptr : dL_dx);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = m_triangle ? "TriangleWave" : "Frequency";
		j["n_frequencies"] = m_n_frequencies;
		return j;
	}
private:
	bool m_triangle;
	uint32_t m_n_frequencies, m_n_dims;
};

// encodings/spherical_harmonics.h:110-230
class SphericalHarmonicsEncoding : public Encoding {
public:
	SphericalHarmonicsEncoding(uint32_t degree, uint32_t n_dims_to_encode, bool fp32) : Encoding{fp32}, m_degree{degree} {
		if (n_dims_to_encode != 3) throw std::runtime_error{"Can only encode 3D directions in spherical harmonics."};
		if (degree == 0) throw std::runtime_error{"Spherical harmonics must have positive degree."};
		if (degree > 8) throw std::runtime_error{"Spherical harmonics are only implemented up to degree 8."};
	}
	uint32_t input_width() const override { return 3; }
	uint32_t output_width() const override { return m_degree * m_degree; }
	EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan) override {
		if (out && padded_output_width() > 0) sh_forward(stream, m_fp32, n, m_degree, x, out, padded_output_width());
		return {};
	}
	void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute&, BackwardHandoff*) override {
		if (!dL_dx) return;
		sh_backward_input(stream, m_fp32, n, m_degree, x, dL_dy, padded_output_width(), *dL_dx);
	}
	// one launch: sh_eval with a dotted twin of every quantity (k_sh_bwd_bwd_input)
	bool has_second_order() const override { return true; }
	void backward_backward_input(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                             MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) override {
		if (n == 0) return;
		if (padded_output_width() == 0) {
			if (dL_dx) zero_input_gradient(stream, n, 3, *dL_dx);
			return;
		}
		sh_backward_backward_input(stream, m_fp32, n, m_degree, x, dL_ddLdx, dL_dy, dL_ddLdy, padded_output_width(), dL_dx);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "SphericalHarmonics";
		j["degree"] = m_degree;
		return j;
	}
private:
	uint32_t m_degree;
};

inline std::unique_ptr<Encoding> create_encoding(uint32_t n_dims_to_encode, const Json& enc, uint32_t alignment, bool fp32);

// encodings/composite.h:126-420, reduction "Concatenation": nested encodings over slices of the input dims, their (padded)
// outputs side by side, their parameters one after the other.  Every nested encoding writes its own AoS block, which is then
// copied into its column range of the composite row (and dL_dy copied out the same way): a few extra bytes per sample instead
// of a width / stride distinction in every encoding kernel.
class CompositeEncoding : public Encoding {
public:
	CompositeEncoding(uint32_t n_dims_to_encode, const Json& params, bool fp32) : Encoding{fp32}, m_n_dims{n_dims_to_encode} {
		if (!params.contains("nested") || !params["nested"].is_array()) throw std::runtime_error{"Must provide an array of nested encodings to CompositeEncoding."};
		const std::string reduction = params.value("reduction", "Concatenation"); // common.h string_to_reduction_type
		if (equals_case_insensitive(reduction, "Concatenation")) m_reduction = Reduction::Concatenation;
		else if (equals_case_insensitive(reduction, "Sum")) m_reduction = Reduction::Sum;
		else if (equals_case_insensitive(reduction, "Product")) m_reduction = Reduction::Product;
		else throw std::runtime_error{"Invalid reduction type: " + reduction};
		const Json& nested = params["nested"];
		m_config = params;
		uint32_t total = 0;
		for (size_t i = 0; i < nested.size(); ++i) { // composite.h:147-158
			total += nested.at(i).value("n_dims_to_encode", 0u);
			if (nested.at(i).contains("dims_to_encode_begin")) { total = 0xFFFFFFFFu; break; }
		}
		if (total != 0xFFFFFFFFu && total > n_dims_to_encode) throw std::runtime_error{"CompositeEncoding: nested encodings must not encode more dims " + std::to_string(total) + " than composite " + std::to_string(n_dims_to_encode)};
		uint32_t unspecified = total == 0xFFFFFFFFu ? 0xFFFFFFFFu : (n_dims_to_encode - total);
		uint32_t offset = 0;
		for (size_t i = 0; i < nested.size(); ++i) { // composite.h:163-187
			const Json& cfg = nested.at(i);
			uint32_t dims;
			if (cfg.contains("n_dims_to_encode")) {
				if (cfg.contains("dims_to_encode_begin")) offset = cfg.value("dims_to_encode_begin", 0u);
				dims = cfg.value("n_dims_to_encode", 0u);
			} else {
				if (unspecified == 0xFFFFFFFFu) throw std::runtime_error{"CompositeEncoding: may only leave 'n_dims_to_encode' unspecified for a single nested encoding"};
				dims = unspecified;
				unspecified = 0xFFFFFFFFu;
			}
			if (dims > 0) {
				if (offset + dims > n_dims_to_encode) throw std::runtime_error{"CompositeEncoding: nested encoding reaches past the input dims"};
				m_nested.emplace_back(create_encoding(dims, cfg, 1, fp32));
				m_begin.push_back(offset);
			}
			offset += dims;
		}
		if (m_nested.empty()) throw std::runtime_error{"CompositeEncoding: no nested encoding encodes anything"};
		if (m_reduction == Reduction::Concatenation) {
			// composite.h:189-200: pad each nested output so that the next one starts at a multiple of ITS required alignment
			uint32_t so_far = 0;
			for (size_t i = 0; i + 1 < m_nested.size(); ++i) {
				const uint32_t desired = m_nested[i + 1]->required_output_alignment();
				m_nested[i]->set_padded_output_width(next_multiple(so_far + m_nested[i]->output_width(), desired) - so_far);
				so_far += m_nested[i]->padded_output_width();
			}
		} else {
			// composite.h:199-211: every nested encoding at the common alignment, and all of the same width
			const uint32_t alignment = required_output_alignment();
			for (auto& e : m_nested) e->set_alignment(alignment);
			for (auto& e : m_nested) {
				if (e->output_width() != m_nested.front()->output_width()) throw std::runtime_error{"CompositeEncoding: nested encodings of a Sum / Product reduction must have the same output width"};
			}
		}
	}
	uint32_t input_width() const override { return m_n_dims; }
	uint32_t output_width() const override { // composite.h:352-366: the sum of the nested PADDED widths; reductions: the (common) padded width
		if (m_reduction != Reduction::Concatenation) return m_nested.front()->padded_output_width();
		uint32_t total = 0;
		for (const auto& e : m_nested) total += e->padded_output_width();
		return total;
	}
	uint32_t required_output_alignment() const override {
		uint32_t a = 1;
		for (const auto& e : m_nested) a = std::lcm(a, e->required_output_alignment());
		return a;
	}
	void set_padded_output_width(uint32_t padded) override { // composite.h:375-385: the last nested encoding absorbs the padding
		if (m_reduction != Reduction::Concatenation) { // :381-384: every nested encoding is padded to the same width
			for (auto& e : m_nested) e->set_padded_output_width(padded);
			return;
		}
		const uint32_t prev = output_width() - m_nested.back()->padded_output_width();
		CHECK_THROW(padded >= prev + m_nested.back()->output_width());
		m_nested.back()->set_padded_output_width(padded - prev);
	}
	size_t n_params() const override {
		size_t n = 0;
		for (const auto& e : m_nested) n += e->n_params();
		return n;
	}
	void initialize_params(Pcg32& rng, float* params_full_precision, float scale) override { // composite.h:422-428
		size_t offset = 0;
		for (auto& e : m_nested) {
			e->initialize_params(rng, params_full_precision + offset, scale);
			offset += e->n_params();
		}
	}
	EncodingContext forward(hipStream_t stream, uint32_t n, MatView x, const void* params, void* out, bool prepare_input_gradients, bool prepare_param_gradients, const ForwardPlan* plan) override {
		EncodingContext ctx;
		if (!out || n == 0) return ctx;
		const size_t elem = m_fp32 ? 4 : 2;
		ctx.nested.resize(m_nested.size());
		uint32_t col = 0;
		size_t p_off = 0;
		if (m_reduction != Reduction::Concatenation) { // composite.h:259-300
			const uint32_t w = reduction_width();
			const size_t block_bytes = (size_t)n * w * elem;
			ctx.to_reduce = ArenaBuf{stream, block_bytes * m_nested.size()}; // [nested][n][w]: kept for the product's backward pass
			for (size_t i = 0; i < m_nested.size(); ++i) {
				Encoding& e = *m_nested[i];
				const MatView xs{x.data + (size_t)m_begin[i] * x.stride_dim, x.stride_sample, x.stride_dim};
				ctx.nested[i] = e.forward(stream, n, xs, (const char*)params + p_off * elem, (char*)ctx.to_reduce.data() + i * block_bytes, prepare_input_gradients, prepare_param_gradients);
				p_off += e.n_params();
			}
			composite_reduce_forward(stream, m_fp32, m_reduction == Reduction::Product, (size_t)n * w, (uint32_t)m_nested.size(), ctx.to_reduce.data(), out);
			return ctx;
		}
		for (size_t i = 0; i < m_nested.size(); ++i) {
			Encoding& e = *m_nested[i];
			const uint32_t w = e.padded_output_width();
			ArenaBuf block{stream, (size_t)n * w * elem};
			const MatView xs{x.data + (size_t)m_begin[i] * x.stride_dim, x.stride_sample, x.stride_dim};
			ctx.nested[i] = e.forward(stream, n, xs, (const char*)params + p_off * elem, block.data(), prepare_input_gradients, prepare_param_gradients);
			copy_columns(stream, elem, n, block.data(), w, 0, out, padded_output_width(), col, w);
			col += w;
			p_off += e.n_params();
		}
		return ctx;
	}
	void backward(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, const void* dL_dy, MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode, const GridBackwardRoute&, BackwardHandoff*) override {
		if (n == 0) return;
		CHECK_THROW(ctx.nested.size() == m_nested.size());
		const size_t elem = m_fp32 ? 4 : 2;
		// input dims no nested encoding looks at have zero gradient
		if (dL_dx) zero_input_gradient(stream, n, m_n_dims, *dL_dx);
		uint32_t col = 0;
		size_t p_off = 0;
		if (m_reduction != Reduction::Concatenation) { // composite.h:302-330: dL/d(nested outputs) from dL/d(reduced output), then the nested passes
			const uint32_t w = reduction_width();
			const size_t block_bytes = (size_t)n * w * elem;
			CHECK_THROW(ctx.to_reduce);
			ArenaBuf dnested{stream, block_bytes * m_nested.size()};
			composite_reduce_backward(stream, m_fp32, m_reduction == Reduction::Product, (size_t)n * w, (uint32_t)m_nested.size(), ctx.to_reduce.data(), dL_dy, dnested.data());
			for (size_t i = 0; i < m_nested.size(); ++i) {
				Encoding& e = *m_nested[i];
				const MatView xs{x.data + (size_t)m_begin[i] * x.stride_dim, x.stride_sample, x.stride_dim};
				MatViewMut dxs{};
				if (dL_dx) dxs = MatViewMut{dL_dx->data + (size_t)m_begin[i] * dL_dx->stride_dim, dL_dx->stride_sample, dL_dx->stride_dim};
				e.backward_rows(stream, ctx.nested[i], n, xs, (const char*)dnested.data() + i * block_bytes, dL_dx ? &dxs : nullptr, (const char*)params + p_off * elem,
				                grads ? (char*)grads + p_off * elem : nullptr, mode);
				p_off += e.n_params();
			}
			return;
		}
		for (size_t i = 0; i < m_nested.size(); ++i) {
			Encoding& e = *m_nested[i];
			const uint32_t w = e.padded_output_width();
			ArenaBuf block{stream, (size_t)n * w * elem};
			copy_columns(stream, elem, n, dL_dy, padded_output_width(), col, block.data(), w, 0, w);
			const MatView xs{x.data + (size_t)m_begin[i] * x.stride_dim, x.stride_sample, x.stride_dim};
			MatViewMut dxs{};
			if (dL_dx) dxs = MatViewMut{dL_dx->data + (size_t)m_begin[i] * dL_dx->stride_dim, dL_dx->stride_sample, dL_dx->stride_dim};
			e.backward_rows(stream, ctx.nested[i], n, xs, block.data(), dL_dx ? &dxs : nullptr, (const char*)params + p_off * elem, grads ? (char*)grads + p_off * elem : nullptr, mode);
			col += w;
			p_off += e.n_params();
		}
	}
	// Second-order pass: every nested encoding's own, on its slices of x, v, dL_dx, the parameters and the gradients.
	//   Concatenation: dL_dy's column range copied out, the tangent copied into the same range of dL_ddLdy.
	//   Sum: every nested pass receives dL_dy as it is; dL_ddLdy = sum_i t_i (the forward reduction on the tangents).
	//   Product (y = prod_i y_i, P_i = prod_{k != i} y_k, S = sum_i <t_i, dL_dy P_i>):
	//     1. g_i = dL_dy P_i (the first-order reduction kernel)   2. nested_i(v_i, dL_dy = g_i) -> t_i, its Hessian term, its gradients
	//     3. k_composite_reduce_bwd_bwd -> dL_ddLdy = sum_i t_i P_i and q_k = dS/dy_k
	//     4. nested_k.backward(dL_dy = q_k), accumulated onto the results of 2. (two or more factors only: q is zero for one)
	// Input dims no nested encoding reads get zero dL_dx; where slices overlap the later encoding's slice replaces the earlier one's, as in
	// backward() (and the reference's composite.h:302-330) -- in step 4 as well, which runs into a buffer of its own before it is added.
	bool has_second_order() const override {
		for (const auto& e : m_nested) {
			if (!e->has_second_order()) return false;
		}
		return true;
	}
	bool second_order_reads_dL_dy() const override {
		if (m_reduction == Reduction::Product && m_nested.size() > 1) return true; // q_k
		for (const auto& e : m_nested) {
			if (e->second_order_reads_dL_dy()) return true;
		}
		return false;
	}
	void backward_backward_input(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy,
	                             MatViewMut* dL_dx, const void* params, void* grads, GradientMode mode) override {
		if (!has_second_order()) return Encoding::backward_backward_input(stream, ctx, n, x, dL_ddLdx, dL_dy, dL_ddLdy, dL_dx, params, grads, mode);
		const bool want_grads = mode != GradientMode::Ignore && n_params() > 0;
		if (n == 0 || (!dL_ddLdy && !dL_dx && !want_grads)) return;
		CHECK_THROW(ctx.nested.size() == m_nested.size());
		CHECK_THROW(!want_grads || grads != nullptr);
		CHECK_THROW(dL_dy != nullptr || !(second_order_reads_dL_dy() && (dL_dx || want_grads)));
		const size_t elem = m_fp32 ? 4 : 2;
		if (dL_dx) zero_input_gradient(stream, n, m_n_dims, *dL_dx);
		const auto slice = [&](const MatView& m, size_t i) { return MatView{m.data + (size_t)m_begin[i] * m.stride_dim, m.stride_sample, m.stride_dim}; };
		const auto slice_mut = [&](const MatViewMut& m, size_t i) { return MatViewMut{m.data + (size_t)m_begin[i] * m.stride_dim, m.stride_sample, m.stride_dim}; };
		size_t p_off = 0;
		if (m_reduction == Reduction::Concatenation) {
			uint32_t col = 0;
			for (size_t i = 0; i < m_nested.size(); ++i) {
				Encoding& e = *m_nested[i];
				const uint32_t w = e.padded_output_width();
				ArenaBuf d_block, t_block;
				if (w > 0 && dL_dy && e.second_order_reads_dL_dy()) {
					d_block = ArenaBuf{stream, (size_t)n * w * elem};
					copy_columns(stream, elem, n, dL_dy, padded_output_width(), col, d_block.data(), w, 0, w);
				}
				if (w > 0 && dL_ddLdy) t_block = ArenaBuf{stream, (size_t)n * w * elem};
				MatViewMut dxs{};
				if (dL_dx) dxs = slice_mut(*dL_dx, i);
				e.backward_backward_input(stream, ctx.nested[i], n, slice(x, i), slice(dL_ddLdx, i), d_block.data(), t_block.data(), dL_dx ? &dxs : nullptr, (const char*)params + p_off * elem,
				                          grads ? (char*)grads + p_off * elem : nullptr, mode);
				if (t_block) copy_columns(stream, elem, n, t_block.data(), w, 0, dL_ddLdy, padded_output_width(), col, w);
				col += w;
				p_off += e.n_params();
			}
			return;
		}
		const bool product = m_reduction == Reduction::Product;
		const uint32_t n_nested = (uint32_t)m_nested.size();
		const uint32_t w = reduction_width();
		const size_t n_elems = (size_t)n * w, block_bytes = n_elems * elem;
		if (w == 0) return;
		const bool want_q = product && n_nested > 1 && (dL_dx || want_grads);
		ArenaBuf g_nested, tangents;
		if (product && dL_dy) { // 1.
			CHECK_THROW(ctx.to_reduce);
			g_nested = ArenaBuf{stream, block_bytes * n_nested};
			composite_reduce_backward(stream, m_fp32, true, n_elems, n_nested, ctx.to_reduce.data(), dL_dy, g_nested.data());
		}
		if (dL_ddLdy || want_q) tangents = ArenaBuf{stream, block_bytes * n_nested};
		for (size_t i = 0; i < n_nested; ++i) { // 2.
			Encoding& e = *m_nested[i];
			MatViewMut dxs{};
			if (dL_dx) dxs = slice_mut(*dL_dx, i);
			const void* d_i = product ? (g_nested ? (const char*)g_nested.data() + i * block_bytes : nullptr) : dL_dy;
			e.backward_backward_input(stream, ctx.nested[i], n, slice(x, i), slice(dL_ddLdx, i), d_i, tangents ? (char*)tangents.data() + i * block_bytes : nullptr, dL_dx ? &dxs : nullptr,
			                          (const char*)params + p_off * elem, grads ? (char*)grads + p_off * elem : nullptr, mode);
			p_off += e.n_params();
		}
		if (!product) {
			if (dL_ddLdy) composite_reduce_forward(stream, m_fp32, false, n_elems, n_nested, tangents.data(), dL_ddLdy);
			return;
		}
		ArenaBuf q;
		if (want_q) q = ArenaBuf{stream, block_bytes * n_nested};
		CHECK_THROW(ctx.to_reduce);
		composite_reduce_backward_backward(stream, m_fp32, n_elems, n_nested, ctx.to_reduce.data(), tangents.data(), dL_dy, dL_ddLdy, q.data()); // 3.
		if (!want_q) return;
		ArenaBuf dx_more;
		MatViewMut dx_view{nullptr, m_n_dims, 1u};
		if (dL_dx) {
			dx_more = ArenaBuf{stream, (size_t)n * m_n_dims * sizeof(float)};
			dx_view.data = dx_more.as<float>();
			zero_input_gradient(stream, n, m_n_dims, dx_view);
		}
		p_off = 0;
		for (size_t k = 0; k < n_nested; ++k) { // 4.
			Encoding& e = *m_nested[k];
			MatViewMut dxs{};
			if (dL_dx) dxs = slice_mut(dx_view, k);
			const bool grads_k = want_grads && e.n_params() > 0;
			e.backward_rows(stream, ctx.nested[k], n, slice(x, k), (const char*)q.data() + k * block_bytes, dL_dx ? &dxs : nullptr, (const char*)params + p_off * elem,
			                grads_k ? (char*)grads + p_off * elem : nullptr, grads_k ? GradientMode::Accumulate : GradientMode::Ignore);
			p_off += e.n_params();
		}
		if (dL_dx) add_input_gradient(stream, n, m_n_dims, MatView{dx_view.data, dx_view.stride_sample, dx_view.stride_dim}, *dL_dx);
	}
	// The tangent alone: what backward_backward_input() runs for dL_ddLdy -- the nested tangents on their slices of x and v, copied into
	// their column ranges (Concatenation), summed (Sum), or sum_i t_i P_i (Product) by the same kernels on the same values -- but through
	// the nested tangent(), so that a nested OneBlob, which has no second-order pass, takes part.
	bool has_tangent() const override {
		for (const auto& e : m_nested) {
			if (!e->has_tangent()) return false;
		}
		return true;
	}
	void tangent(hipStream_t stream, const EncodingContext& ctx, uint32_t n, MatView x, MatView v, void* t, const void* params) override {
		if (n == 0 || !t) return;
		CHECK_THROW(has_tangent() && ctx.nested.size() == m_nested.size());
		const size_t elem = m_fp32 ? 4 : 2;
		const auto slice = [&](const MatView& m, size_t i) { return MatView{m.data + (size_t)m_begin[i] * m.stride_dim, m.stride_sample, m.stride_dim}; };
		size_t p_off = 0;
		if (m_reduction == Reduction::Concatenation) {
			uint32_t col = 0;
			for (size_t i = 0; i < m_nested.size(); ++i) {
				Encoding& e = *m_nested[i];
				const uint32_t w = e.padded_output_width();
				if (w > 0) {
					ArenaBuf t_block{stream, (size_t)n * w * elem};
					e.tangent(stream, ctx.nested[i], n, slice(x, i), slice(v, i), t_block.data(), (const char*)params + p_off * elem);
					copy_columns(stream, elem, n, t_block.data(), w, 0, t, padded_output_width(), col, w);
				}
				col += w;
				p_off += e.n_params();
			}
			return;
		}
		const uint32_t n_nested = (uint32_t)m_nested.size();
		const uint32_t w = reduction_width();
		const size_t n_elems = (size_t)n * w, block_bytes = n_elems * elem;
		if (w == 0) return;
		ArenaBuf tangents{stream, block_bytes * n_nested};
		for (size_t i = 0; i < n_nested; ++i) {
			Encoding& e = *m_nested[i];
			e.tangent(stream, ctx.nested[i], n, slice(x, i), slice(v, i), (char*)tangents.data() + i * block_bytes, (const char*)params + p_off * elem);
			p_off += e.n_params();
		}
		if (m_reduction == Reduction::Sum) return composite_reduce_forward(stream, m_fp32, false, n_elems, n_nested, tangents.data(), t);
		CHECK_THROW(ctx.to_reduce);
		composite_reduce_backward_backward(stream, m_fp32, n_elems, n_nested, ctx.to_reduce.data(), tangents.data(), nullptr, t, nullptr);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "Composite";
		j["reduction"] = m_reduction == Reduction::Sum ? "Sum" : (m_reduction == Reduction::Product ? "Product" : "Concatenation");
		Json nested = Json::array();
		for (const auto& e : m_nested) nested.push_back(e->hyperparams());
		j["nested"] = nested;
		return j;
	}
private:
	enum class Reduction { Concatenation, Sum, Product };
	// Width of a reduction's operands.  The reference lays the nested outputs out at multiples of their UNPADDED width but
	// reduces at multiples of the PADDED one (composite.h:274 against :261): the two agree -- and the result is defined --
	// only when no nested output needs padding, which is what this build accepts.
	uint32_t reduction_width() const {
		for (const auto& e : m_nested) {
			if (e->padded_output_width() != e->output_width()) {
				throw std::runtime_error{"CompositeEncoding: a Sum / Product reduction needs nested encodings whose output width (" + std::to_string(e->output_width()) +
				                         ") is a multiple of the required alignment (padded to " + std::to_string(e->padded_output_width()) + ")"};
			}
		}
		return m_nested.front()->padded_output_width();
	}
public:
	uint64_t list_scatters() const override {
		uint64_t total = 0;
		for (const auto& e : m_nested) total += e->list_scatters();
		return total;
	}
	// every grid nested here takes the setting; a nested grid sees all n rows (its own input columns), so the per-sample array is indexed by row
	bool set_max_level(float max_level) override {
		bool any = false;
		for (auto& e : m_nested) any |= e->set_max_level(max_level);
		return any;
	}
	bool set_max_level_gpu(const float* per_sample) override {
		bool any = false;
		for (auto& e : m_nested) any |= e->set_max_level_gpu(per_sample);
		return any;
	}
	bool get_max_level(float& max_level, const float*& per_sample) const override {
		for (const auto& e : m_nested) {
			if (e->get_max_level(max_level, per_sample)) return true;
		}
		return false;
	}

private:
	uint32_t m_n_dims;
	Json m_config;
	Reduction m_reduction = Reduction::Concatenation;
	std::vector<std::unique_ptr<Encoding>> m_nested;
	std::vector<uint32_t> m_begin;
};

inline std::unique_ptr<Encoding> create_encoding(uint32_t n_dims_to_encode, const Json& enc, uint32_t alignment, bool fp32) {
	const std::string name = to_lower(enc.value("otype", "OneBlob"));
	std::unique_ptr<Encoding> result;
	if (name == "grid" || name == "hashgrid" || name == "tiledgrid" || name == "densegrid") {
		result.reset(new GridEncoding{n_dims_to_encode, enc, fp32});
	} else if (name == "oneblob") {
		result.reset(new OneBlobEncoding{enc.value("n_bins", 16u), n_dims_to_encode, fp32});
	} else if (name == "identity") {
		result.reset(new IdentityEncoding{n_dims_to_encode, enc.value("scale", 1.0f), enc.value("offset", 0.0f), fp32});
	} else if (name == "empty") {
		result.reset(new EmptyEncoding{n_dims_to_encode, fp32});
	} else if (name == "ppng1" || name == "ppng2" || name == "ppng3") {
		result.reset(new PpngEncoding{(uint32_t)(name.back() - '0'), n_dims_to_encode, enc, fp32});
	} else if (name == "frequency") {
		result.reset(new PeriodicEncoding{false, enc.value("n_frequencies", 12u), n_dims_to_encode, fp32});
	} else if (name == "trianglewave") {
		result.reset(new PeriodicEncoding{true, enc.value("n_frequencies", 12u), n_dims_to_encode, fp32});
	} else if (name == "sphericalharmonics") {
		result.reset(new SphericalHarmonicsEncoding{enc.value("degree", 4u), n_dims_to_encode, fp32});
	} else if (name == "composite") {
		result.reset(new CompositeEncoding{n_dims_to_encode, enc, fp32});
	} else if (name == "oneblobfrequency" || name == "nrc") {
		// src/encoding.cu:96-119: the neural radiance caching input layer = TriangleWave on 3 position dims, OneBlob on the next 5,
		// Identity on whatever is left
		Json tri = Json::object(), blob = Json::object(), rest = Json::object();
		tri["n_dims_to_encode"] = 3u;
		tri["otype"] = "TriangleWave";
		tri["n_frequencies"] = enc.value("n_frequencies", 12u);
		blob["n_dims_to_encode"] = 5u;
		blob["otype"] = "OneBlob";
		blob["n_bins"] = enc.value("n_bins", 4u);
		rest["otype"] = "Identity";
		Json nested = Json::array();
		nested.push_back(tri);
		nested.push_back(blob);
		nested.push_back(rest);
		Json composite = Json::object();
		composite["otype"] = "Composite";
		composite["nested"] = nested;
		result.reset(new CompositeEncoding{n_dims_to_encode, composite, fp32});
	} else {
		throw std::runtime_error{"Encoding '" + enc.value("otype", "OneBlob") + "' not found (this build provides Grid/HashGrid/TiledGrid/DenseGrid, OneBlob, Identity, Empty, Frequency, TriangleWave, SphericalHarmonics, Composite, PPNG1, PPNG2)"};
	}
	if (alignment > 0) result->set_alignment(alignment);
	return result;
}

// ------------------------------------------------------------------------------------------------------------------
// Network: FullyFusedMLP and CutlassMLP (identical math): the fused kernels where they cover the shape, else layer by layer
// ------------------------------------------------------------------------------------------------------------------
inline Activation string_to_activation(const std::string& s) {
	static const std::pair<const char*, Activation> table[] = {
		{"None", Activation::None}, {"ReLU", Activation::ReLU}, {"LeakyReLU", Activation::LeakyReLU}, {"Exponential", Activation::Exponential},
		{"Sine", Activation::Sine}, {"Sigmoid", Activation::Sigmoid}, {"Squareplus", Activation::Squareplus}, {"Softplus", Activation::Softplus},
		{"Tanh", Activation::Tanh}};
	for (const auto& kv : table) if (equals_case_insensitive(s, kv.first)) return kv.second;
	throw std::runtime_error{"Invalid activation name: " + s};
}
inline const char* to_string(Activation a) {
	static const char* names[] = {"None", "ReLU", "LeakyReLU", "Exponential", "Sine", "Sigmoid", "Squareplus", "Softplus", "Tanh"};
	return names[(uint32_t)a];
}

struct NetworkContext {
	ArenaBuf hidden; // [n_hidden][n][width] in the network's precision
	ArenaBuf pre;    // layer-by-layer Sine networks: the hidden layers' pre-activations, laid out as `hidden` (cutlass_mlp.cu:53)
};

class Network {
public:
	static constexpr uint32_t REQUIRED_ALIGNMENT = 16; // fully_fused_mlp.h:108-110, cutlass_mlp.h:115-121

	// precision Fp32: the reference's build without TCNN_HALF_PRECISION (common.h:99-123) as a choice per network -- CutlassMLP<float>.
	// Parameters, activations, gradients and every second-order intermediate are floats, and the network always runs layer by layer
	// (k_mlp_layers.hip; weight gradients: k_mlp_layers_f32.hip): no fragment images, no fused training plan.
	explicit Network(const Json& net, Precision precision = Precision::Fp16) : m_fp32{precision == Precision::Fp32} { // network.cu:48-137
		const std::string otype = net.value("otype", "MLP");
		m_fully_fused = equals_case_insensitive(otype, "MegakernelMLP") || equals_case_insensitive(otype, "FullyFusedMLP");
		const bool cutlass = equals_case_insensitive(otype, "MLP") || equals_case_insensitive(otype, "CutlassMLP");
		if (!m_fully_fused && !cutlass) throw std::runtime_error{"Invalid network type: " + otype};
		if (m_fully_fused && m_fp32) throw std::runtime_error{"FullyFusedMLP can only be used if the network precision is set to __half."}; // network.cu:102-103
		if (!net.contains("n_input_dims") || !net.contains("n_output_dims")) throw std::runtime_error{"network config needs n_input_dims and n_output_dims"};
		m_input_width = net.value("n_input_dims", 0u);
		m_output_width = net.value("n_output_dims", 0u);
		m_width = net.value("n_neurons", 128u);
		m_n_hidden = net.value("n_hidden_layers", 5u);
		m_activation = string_to_activation(net.value("activation", "ReLU"));
		m_output_activation = string_to_activation(net.value("output_activation", "None"));
		// fully_fused_mlp.cu:869-881 restricts FullyFusedMLP to these widths; the fused kernels also cover CutlassMLP at 256
		const bool fused_width = m_width == 16 || m_width == 32 || m_width == 64 || m_width == 128 || (cutlass && m_width == 256);
		if (cutlass) {
			// CutlassMLP (cutlass_mlp.cu:39-92) takes any width; here multiples of REQUIRED_ALIGNMENT up to 1024 (cutlass_mlp.h:115-121),
			// zero hidden layers and Sine -- the shapes the fused kernels do not cover run layer by layer (k_mlp_layers.hip)
			if (m_width % REQUIRED_ALIGNMENT != 0 || m_width < 16 || m_width > 1024) {
				throw std::runtime_error{"CutlassMLP: n_neurons must be a multiple of 16 between 16 and 1024, but got " + std::to_string(m_width) + "."};
			}
			m_layerwise = !fused_width || m_n_hidden == 0 || m_activation == Activation::Sine;
		} else {
			if (!fused_width) {
				throw std::runtime_error{"FullyFusedMLP only supports 16, 32, 64, and 128 neurons, but got " + std::to_string(m_width) + ". (CutlassMLP: any multiple of 16 up to 1024.)"};
			}
			if (m_n_hidden <= 0) throw std::runtime_error{"FullyFusedMLP requires at least 1 hidden layer (3 layers in total)."};
			if (m_activation == Activation::Sine) throw std::runtime_error{"FullyFusedMLP: Sine activation is not supported in the fused kernels"};
		}
		if (m_n_hidden + 1 > MAX_MLP_LAYERS) throw std::runtime_error{"MLP: too many layers for this build"};
		if (m_input_width % 16 != 0) throw std::runtime_error{"MLP: input width must be a multiple of 16"};
		m_layerwise = m_layerwise || m_fp32 || switches().mlp_layerwise; // TCNN_AMD_MLP_LAYERWISE=1: the A/B form for any shape
		m_padded_output_width = next_multiple(m_output_width, REQUIRED_ALIGNMENT);

		// matrices: fully_fused_mlp.cu:659-671
		memset(&m_desc, 0, sizeof(m_desc));
		m_desc.in_width = m_input_width;
		m_desc.width = m_width;
		m_desc.out_width = m_padded_output_width;
		m_desc.n_hidden = m_n_hidden;
		m_desc.n_layers = m_n_hidden + 1;
		m_desc.activation = (uint32_t)m_activation;
		m_desc.output_activation = (uint32_t)m_output_activation;
		uint32_t w_off = 0, f_off = 0, b_off = 0;
		for (uint32_t l = 0; l < m_desc.n_layers; ++l) {
			MlpLayer& L = m_desc.layers[l];
			L.rows = l == m_desc.n_layers - 1 ? m_padded_output_width : m_width;
			L.cols = l == 0 ? m_input_width : m_width;
			L.w_off = w_off;
			L.ks_fwd = div_round_up(L.cols, 32);
			L.ks_bwd = div_round_up(L.rows, 32);
			L.natural_k = l == 0 ? 1u : 0u;
			L.fwd_off = f_off;
			L.bwd_off = b_off;
			f_off += (L.rows / 16) * L.ks_fwd;
			b_off += (L.cols / 16) * L.ks_bwd;
			w_off += L.rows * L.cols;
		}
		// (the layer-by-layer path reads the parameters as they are: no fragment images)
		m_desc.n_frags_fwd = m_layerwise ? 0u : f_off;
		m_desc.n_frags_bwd = m_layerwise ? 0u : b_off;
		m_desc.n_frags_r32 = !m_layerwise && r32_shape_ok(m_desc) ? R32Frags(m_desc).n_frags() : 0u;
		m_n_params = w_off;
	}

	// the network runs layer by layer (k_mlp_layers.hip) instead of the fused kernels: CutlassMLP shapes they do not cover, or
	// TCNN_AMD_MLP_LAYERWISE=1 when the model was created.  Fragment images, fused input / output forms and the fused training step
	// are then never used.
	bool layerwise() const { return m_layerwise; }
	bool has_output_activation() const { return m_output_activation != Activation::None; }
	bool fully_fused() const { return m_fully_fused; } // otype FullyFusedMLP: no second-order pass (as in the reference); CutlassMLP has one
	Precision precision() const { return m_fp32 ? Precision::Fp32 : Precision::Fp16; }
	size_t element_size() const { return m_fp32 ? sizeof(float) : sizeof(_Float16); } // bytes of a parameter, an activation, a gradient

	uint32_t input_width() const { return m_input_width; }
	uint32_t output_width() const { return m_output_width; }
	uint32_t padded_output_width() const { return m_padded_output_width; }
	uint32_t width() const { return m_width; }
	uint32_t n_hidden() const { return m_n_hidden; }
	size_t n_params() const { return m_n_params; }
	const MlpDesc& desc() const { return m_desc; }

	std::vector<std::pair<uint32_t, uint32_t>> layer_sizes() const {
		std::vector<std::pair<uint32_t, uint32_t>> r;
		for (uint32_t l = 0; l < m_desc.n_layers; ++l) r.emplace_back(m_desc.layers[l].rows, m_desc.layers[l].cols);
		return r;
	}

	void initialize_params(Pcg32& rng, float* params_full_precision, float scale) { // fully_fused_mlp.cu:866-891, gpu_matrix.h:284-299
		std::vector<float> host(m_n_params);
		for (uint32_t l = 0; l < m_desc.n_layers; ++l) {
			const MlpLayer& L = m_desc.layers[l];
			// Sine: SIREN (cutlass_mlp.cu:360-366, gpu_matrix.h:335-369) -- U(+-30 scale / fan_in) for the first matrix, U(+-scale sqrt(6 / fan_in))
			// for the others; else Xavier over fan_in + fan_out
			const float s = m_activation != Activation::Sine ? scale * std::sqrt(6.0f / (float)(L.cols + L.rows))
			                : l == 0 ? scale * (30.0f / (float)L.cols) : scale * std::sqrt(6.0f / (float)L.cols);
			float* w = host.data() + L.w_off;
			for (size_t i = 0; i < (size_t)L.rows * L.cols; ++i) w[i] = rng.next_float() * 2.0f * s - s;
		}
		HIP_CHECK_THROW(hipMemcpy(params_full_precision, host.data(), m_n_params * sizeof(float), hipMemcpyHostToDevice));
	}

	// ---- A fragment image that lives across training steps, for models whose optimizer step rides on the weight gradients' slab
	// reduction (BASELINE config 2).  k_wgrad_reduce_adam writes every weight it updates into the image elements that hold it
	// (AdamInReduce::image / image_inv), so the next step starts with a current image instead of a k_mlp_prep launch -- 4.5 of config 2's
	// 27 us.  The image is current for the parameter vector `live_params()`; whoever changes those parameters any other way calls
	// invalidate_live_image() (the Trainer does, and stops using the image for good once it has handed out a pointer to its parameters).
	struct LiveImage {
		DeviceBuf image, inverse;       // inverse: uint32 [n_params][IMAGE_INV_WIDTH], the image elements that hold a weight (0xffffffff: none)
		const void* params = nullptr;   // what the image is current for
	};
	// nullptr: a weight of this network sits in more than IMAGE_INV_WIDTH image elements (no supported shape does)
	LiveImage* live_image() const {
		if (m_layerwise) return nullptr;
		if (m_live_state == 0) {
			const uint32_t total = (m_desc.n_frags_fwd + m_desc.n_frags_bwd + m_desc.n_frags_r32) * 512;
			std::vector<uint32_t> inv(m_n_params * IMAGE_INV_WIDTH, 0xffffffffu), count(m_n_params, 0);
			m_live_state = 1;
			for (uint32_t gid = 0; gid < total && m_live_state == 1; ++gid) {
				const int32_t src = mlp_prep_source(m_desc, gid);
				if (src < 0) continue;
				if ((size_t)src >= m_n_params || count[src] == IMAGE_INV_WIDTH) m_live_state = -1;
				else inv[(size_t)src * IMAGE_INV_WIDTH + count[src]++] = gid;
			}
			if (m_live_state == 1) {
				m_live.image.resize(mlp_image_bytes(m_desc));
				m_live.inverse.resize(inv.size() * sizeof(uint32_t));
				HIP_CHECK_THROW(hipMemcpy(m_live.inverse.data(), inv.data(), inv.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
			}
		}
		return m_live_state == 1 ? &m_live : nullptr;
	}
	void invalidate_live_image() const { m_live.params = nullptr; }

	// images: [fwd][bwd] fragment images of `params`
	ArenaBuf prepare(hipStream_t stream, const void* params, bool want_bwd) const {
		if (m_layerwise) throw std::runtime_error{"Network::prepare: a layer-by-layer network has no fragment images"};
		ArenaBuf image{stream, mlp_image_bytes(m_desc)};
		mlp_prepare_weights(stream, m_desc, params, image.data(), want_bwd);
		return image;
	}

	void inference(hipStream_t stream, uint32_t n, const void* input, void* output, const void* params) const {
		if (m_layerwise) return forward_layers(stream, n, input, output, params, nullptr, nullptr);
		ArenaBuf image = prepare(stream, params, false);
		mlp_forward(stream, m_desc, image.data(), n, input, output, nullptr);
	}
	// inference with the input / output conversions fused into the kernel (see MlpIo); the layer-by-layer path takes the plain form only
	void inference_io(hipStream_t stream, uint32_t n, const MlpIo& io, const void* params) const {
		if (m_layerwise) {
			if (!io.x_half || io.x_plane_features || io.x_f32.data || io.x_oneblob_bins || !io.out_half || io.out_f32.data) {
				throw std::runtime_error{"Network::inference_io: a layer-by-layer network takes a half input matrix and writes a half output matrix"};
			}
			return forward_layers(stream, n, io.x_half, io.out_half, params, nullptr, nullptr);
		}
		ArenaBuf image = prepare(stream, params, false);
		mlp_forward_io(stream, m_desc, image.data(), n, io, nullptr);
	}

	NetworkContext forward(hipStream_t stream, uint32_t n, const void* input, void* output, const void* params) const {
		NetworkContext ctx;
		ctx.hidden = ArenaBuf{stream, (size_t)m_n_hidden * n * m_width * element_size()};
		if (m_layerwise) {
			if (m_activation == Activation::Sine) ctx.pre = ArenaBuf{stream, (size_t)m_n_hidden * n * m_width * element_size()};
			forward_layers(stream, n, input, output, params, ctx.hidden.data(), ctx.pre.data());
			return ctx;
		}
		ArenaBuf image = prepare(stream, params, false);
		mlp_forward(stream, m_desc, image.data(), n, input, output, ctx.hidden.data());
		return ctx;
	}

	// dL_dinput: optional [n][in_width]; gradients: [n_params] or nullptr (both in the network's precision)
	void backward(hipStream_t stream, const NetworkContext& ctx, uint32_t n, const void* input, const void* output, const void* dL_doutput,
	              void* dL_dinput, const void* params, void* gradients, GradientMode mode, uint32_t dx_plane_features = 0) const {
		// output-activation transfer, computed once up front like the reference (fully_fused_mlp.cu:757-762)
		const void* dY = dL_doutput;
		ArenaBuf dY_tmp;
		MlpDesc desc = m_desc;
		if (m_output_activation != Activation::None) {
			dY_tmp = ArenaBuf{stream, (size_t)n * m_padded_output_width * element_size()};
			mlp_activation_backward_output(stream, precision(), (size_t)n * m_padded_output_width, (uint32_t)m_output_activation, dL_doutput, output, dY_tmp.data());
			dY = dY_tmp.data();
			desc.output_activation = (uint32_t)Activation::None;
		}
		if (m_layerwise) {
			if (dx_plane_features) throw std::runtime_error{"Network::backward: a layer-by-layer network writes dL/dinput as a matrix, not as level planes"};
			return backward_layers(stream, ctx, n, input, dY, dL_dinput, params, gradients, mode);
		}
		ArenaBuf image = prepare(stream, params, true);
		ArenaBuf dhidden{stream, (size_t)m_n_hidden * n * m_width * 2};
		mlp_backward(stream, desc, image.data(), n, dY, output, ctx.hidden.data(), dhidden.data(), dL_dinput, dx_plane_features);
		if (mode == GradientMode::Ignore) return;
		CHECK_THROW(gradients != nullptr);

		const bool accumulate = mode == GradientMode::Accumulate;
		const size_t hstride = (size_t)n * m_width; // elements per hidden layer
		std::vector<WgradPanel> panels;
		for (uint32_t l = 0; l < m_desc.n_layers; ++l) { // (the hidden layers' activations and gradients are tiled, k_mlp.hip hidden_tile_off)
			const MlpLayer& L = m_desc.layers[l];
			const bool dO_tiled = l != m_desc.n_layers - 1, In_tiled = l != 0;
			const void* dO = dO_tiled ? at((const void*)dhidden.data(), hstride * l) : dY;
			const void* In = In_tiled ? at((const void*)ctx.hidden.data(), hstride * (l - 1)) : input;
			add_wgrad_panels(panels, L, dO, layer_ld(l), In, l == 0 ? m_input_width : m_width, at(gradients, L.w_off), dO_tiled, In_tiled);
		}
		ArenaBuf ws{stream, wgrad_panels_workspace_floats(precision(), panels.data(), (uint32_t)panels.size(), n) * sizeof(float)};
		mlp_wgrad_panels(stream, precision(), n, panels.data(), (uint32_t)panels.size(), accumulate, ws.as<float>()); // (layers of one shape share a launch)
	}

	// ---- input_gradient (object.h:342-366) for the network alone: dL_dinput [n][in_width] (or level planes) in the network's precision =
	// backprop_scale * d output[dim] / d input.  The plan (mlp_input_gradient_plan, asked once per call by the caller, who needs it to choose
	// the input's form) decides between the fused kernel and forward + backward on a one-hot dL/dy: the same bits either way.
	// io: fused -- whatever mlp_input_gradient takes; two-pass -- x_half rows.  io.out_half: optional with the fused kernel, needed by the two passes.
	MlpInputGradPlan input_gradient_plan(uint32_t n) const { return mlp_input_gradient_plan(m_desc, m_layerwise, n); }
	void input_gradient(hipStream_t stream, const MlpInputGradPlan& plan, uint32_t n, const MlpIo& io, uint32_t dim, float backprop_scale, const void* params, void* dL_dinput,
	                    uint32_t dx_plane_features) const {
		CHECK_THROW(dim < m_padded_output_width && dL_dinput != nullptr);
		if (plan.fused) {
			ArenaBuf image = prepare(stream, params, true);
			return mlp_input_gradient(stream, m_desc, plan, image.data(), n, io, dim, backprop_scale, dL_dinput, dx_plane_features);
		}
		CHECK_THROW(io.x_half != nullptr && io.out_half != nullptr && !io.x_plane_features && !io.x_f32.data && !io.x_oneblob_bins);
		ArenaBuf d_doutput{stream, (size_t)n * m_padded_output_width * element_size()};
		input_gradient_one_hot(stream, precision(), n, m_padded_output_width, dim, backprop_scale, d_doutput.data());
		const NetworkContext ctx = forward(stream, n, io.x_half, io.out_half, params);
		backward(stream, ctx, n, io.x_half, io.out_half, d_doutput.data(), dL_dinput, params, nullptr, GradientMode::Ignore, dx_plane_features);
	}

	// ---- input_jacobian: input_gradient for n_dims output columns from one forward pass.  dL_dinput: n_dims buffers one behind the other,
	// buffer k bit for bit what input_gradient(dim = dims[k]) writes.  The fused kernel (mlp_input_jacobian_plan), or one forward pass and
	// n_dims backward passes on its context.
	MlpInputGradPlan input_jacobian_plan(uint32_t n, uint32_t n_dims) const { return mlp_input_jacobian_plan(m_desc, m_layerwise, n, n_dims); }
	void input_jacobian(hipStream_t stream, const MlpInputGradPlan& plan, uint32_t n, const MlpIo& io, const uint32_t* dims, uint32_t n_dims, float backprop_scale, const void* params,
	                    void* dL_dinput, uint32_t dx_plane_features) const {
		CHECK_THROW(dims != nullptr && n_dims > 0 && dL_dinput != nullptr);
		for (uint32_t k = 0; k < n_dims; ++k) CHECK_THROW(dims[k] < m_padded_output_width);
		if (plan.fused) {
			ArenaBuf image = prepare(stream, params, true);
			return mlp_input_jacobian(stream, m_desc, plan, image.data(), n, io, dims, n_dims, backprop_scale, dL_dinput, dx_plane_features);
		}
		CHECK_THROW(io.x_half != nullptr && io.out_half != nullptr && !io.x_plane_features && !io.x_f32.data && !io.x_oneblob_bins);
		ArenaBuf d_doutput{stream, (size_t)n * m_padded_output_width * element_size()};
		const NetworkContext ctx = forward(stream, n, io.x_half, io.out_half, params);
		for (uint32_t k = 0; k < n_dims; ++k) {
			input_gradient_one_hot(stream, precision(), n, m_padded_output_width, dims[k], backprop_scale, d_doutput.data());
			backward(stream, ctx, n, io.x_half, io.out_half, d_doutput.data(), (char*)dL_dinput + (size_t)k * n * m_input_width * element_size(), params, nullptr, GradientMode::Ignore,
			         dx_plane_features);
		}
	}

	// ---- input_jvp: the network's part of J v for n_tangents directions.  tangents: n_tangents buffers one behind the other, each
	// [n][in_width] in the network's precision (a fused plan: or tangents_f32, see mlp_input_jvp); jvp [n][jvp_tangents][padded output
	// width], of which this call writes tangents t0 .. t0 + n_tangents - 1.  The fused kernel (mlp_input_jvp_plan), or layer by layer from
	// the row-major input exactly as second_order_begin / _finish run their forward and tangent passes -- mlp_layer_forward once,
	// mlp_layer_tangent per tangent with g = r_out = nullptr -- for any otype: a FullyFusedMLP has tangents though no second-order pass.
	// io.out_half (optional): the output, bit for bit inference()'s -- the fused kernel's forward chain, the layer-by-layer chain of a
	// layerwise network, or for a fused-shape network on the two passes its own inference().
	MlpInputJvpPlan input_jvp_plan(uint32_t n, uint32_t n_tangents) const { return mlp_input_jvp_plan(m_desc, m_layerwise, n, n_tangents); }
	void input_jvp(hipStream_t stream, const MlpInputJvpPlan& plan, uint32_t n, const MlpIo& io, const void* tangents, MatView tangents_f32, uint32_t n_tangents, const void* params,
	               void* jvp, uint32_t jvp_tangents, uint32_t t0) const {
		CHECK_THROW(n_tangents > 0 && t0 + n_tangents <= jvp_tangents && jvp != nullptr);
		const uint32_t pw = m_padded_output_width;
		if (plan.fused) {
			ArenaBuf image = prepare(stream, params, false);
			return mlp_input_jvp(stream, m_desc, plan, image.data(), n, io, tangents, tangents_f32, n_tangents, at(jvp, (size_t)t0 * pw), jvp_tangents * pw);
		}
		CHECK_THROW(io.x_half != nullptr && tangents != nullptr && !io.x_plane_features && !io.x_f32.data && !io.x_oneblob_bins && !tangents_f32.data);
		SecondOrderPass pass = second_order_forward(stream, n, io.x_half, params);
		if (io.out_half) {
			if (m_layerwise) HIP_CHECK_THROW(hipMemcpyAsync(io.out_half, at((const void*)pass.h.data(), pass.slot * (m_desc.n_layers - 1)), (size_t)n * pw * element_size(), hipMemcpyDeviceToDevice, stream));
			else inference(stream, n, io.x_half, io.out_half, params);
		}
		ArenaBuf one;
		if (jvp_tangents > 1) one = ArenaBuf{stream, (size_t)n * pw * element_size()};
		for (uint32_t t = 0; t < n_tangents; ++t) {
			void* u_K = jvp_tangents > 1 ? one.data() : jvp;
			second_order_finish(stream, pass, n, at(tangents, (size_t)t * n * m_input_width), u_K, nullptr, params, nullptr, GradientMode::Ignore);
			if (jvp_tangents > 1) copy_columns(stream, element_size(), n, u_K, pw, 0, jvp, jvp_tangents * pw, (t0 + t) * pw, pw);
		}
	}

	// ---- Second-order input gradients of a CutlassMLP: the gradients of S = <v, dL/dinput> for a given v = dL2/d(dL/dinput).
	// With h_0 = input, z_k = W_k h_{k-1}, h_k = a_k(z_k), g_K = dL/dy, d_k = g_k a_k'(z_k), g_{k-1} = W_k^T d_k (dL/dinput = g_0):
	//   tangent    u_0 = v, z'_k = W_k u_{k-1}, u_k = a_k'(z_k) z'_k                  dS/d(dL/dy) = u_K
	//   bilinear   dS/dW_k = d_k^T u_{k-1}
	//   curvature  r_k = a_k''(z_k) g_k z'_k, p_K = r_K, p_k = r_k + a_k'(z_k) W_{k+1}^T p_{k+1}, dS/dW_k += p_k^T h_{k-1}, dS/dinput = W_1^T p_1
	// The curvature pass exists only where some a_k'' != 0: for None / ReLU / LeakyReLU throughout it is not launched and dS/dinput is zero.
	// Always layer by layer on row-major matrices (k_mlp_layers.hip), whatever kernels the first-order passes of this shape run: the
	// forward pass and the first-order data pass are run again from the network's input (second_order_begin), keeping z_k (or h_k where
	// the sign is all a' needs), g_k for the layers with curvature, and d_k; g_0 is not needed and not computed.  Two steps, so that a
	// model with an encoding in front can allocate v in between (NetworkWithInputEncoding::backward_backward_input).
	static bool has_curvature(uint32_t act) {
		return act != (uint32_t)Activation::None && act != (uint32_t)Activation::ReLU && act != (uint32_t)Activation::LeakyReLU;
	}
	bool any_curvature() const { return has_curvature((uint32_t)m_output_activation) || (m_n_hidden > 0 && has_curvature((uint32_t)m_activation)); }

	struct SecondOrderPass {
		ArenaBuf h, z, g, d, wt; // [n_layers] slots of n x max(width, padded output width) elements each (wt: laid out as the parameters)
		size_t slot = 0;
		const void* input = nullptr;
		const void* dL_doutput = nullptr;
		bool have_d = false, have_wt0 = false;
	};

	// the route of input_jvp_backward() for this network ("two-pass": the passes below, composed by the model)
	MlpInputJvpBackwardPlan input_jvp_backward_plan(uint32_t n, uint32_t n_tangents) const { return mlp_input_jvp_backward_plan(m_desc, m_layerwise, n, n_tangents); }

	// need_d: second_order_finish() will be asked for parameter gradients or for dS_dinput (else only the forward pass is run again)
	// (For any otype, as second_order_forward(): input_jvp_backward() runs these passes for a FullyFusedMLP too.  The public
	// backward_backward_input of a FullyFusedMLP is refused by the model in front, before it gets here.)
	SecondOrderPass second_order_begin(hipStream_t stream, uint32_t n, const void* input, const void* dL_doutput, const void* params, bool need_d) const {
		SecondOrderPass s = second_order_forward(stream, n, input, params);
		s.dL_doutput = dL_doutput;
		const uint32_t K = m_desc.n_layers;
		const bool curved = any_curvature();
		const void* p = params;
		if (!need_d) return s;
		s.have_d = true;
		s.d = ArenaBuf{stream, K * s.slot * element_size()};
		if (curved) s.g = ArenaBuf{stream, K * s.slot * element_size()};
		s.wt = ArenaBuf{stream, m_n_params * element_size()};
		for (uint32_t l = 1; l < K; ++l) mlp_layer_transpose(stream, precision(), m_desc.layers[l].rows, m_desc.layers[l].cols, at(p, m_desc.layers[l].w_off), at(s.wt.data(), m_desc.layers[l].w_off));
		if (layer_act(K - 1) != (uint32_t)Activation::None) { // d_K = a_K'(z_K) g_K
			mlp_layer_delta(stream, precision(), (size_t)n * m_padded_output_width, layer_act(K - 1), dL_doutput, aux_of(s, K - 1), at(s.d.data(), s.slot * (K - 1)));
		}
		for (uint32_t l = K - 1; l > 0; --l) {
			const MlpLayer& L = m_desc.layers[l];
			const uint32_t act = layer_act(l - 1);
			mlp_layer_backward_keep(stream, precision(), n, d_of(s, l), layer_ld(l), at(s.wt.data(), L.w_off), L.rows, L.cols, act, aux_of(s, l - 1),
			                    has_curvature(act) ? at(s.g.data(), s.slot * (l - 1)) : nullptr, at(s.d.data(), s.slot * (l - 1)), m_width);
		}
		return s;
	}
	// the forward half of second_order_begin(): h_k (and z_k where a' needs it), layer by layer from the row-major input.  For any otype:
	// input_jvp() runs it for a FullyFusedMLP too, which has tangents though no second-order pass.
	SecondOrderPass second_order_forward(hipStream_t stream, uint32_t n, const void* input, const void* params) const {
		SecondOrderPass s;
		const uint32_t K = m_desc.n_layers;
		s.slot = (size_t)n * std::max(m_width, m_padded_output_width);
		s.input = input;
		const bool curved = any_curvature();
		const void* p = params;
		s.h = ArenaBuf{stream, K * s.slot * element_size()};
		if (curved) s.z = ArenaBuf{stream, K * s.slot * element_size()};
		const void* in = input;
		uint32_t ldi = m_input_width;
		for (uint32_t l = 0; l < K; ++l) {
			const MlpLayer& L = m_desc.layers[l];
			void* out = at(s.h.data(), s.slot * l);
			mlp_layer_forward(stream, precision(), n, in, ldi, at(p, L.w_off), L.rows, L.cols, layer_act(l), out, layer_ld(l), has_curvature(layer_act(l)) ? at(s.z.data(), s.slot * l) : nullptr);
			in = out;
			ldi = m_width;
		}
		return s;
	}

	// (all in the network's precision)  v: [n][in_width].  Optional results: dL_ddLdoutput [n][padded output width]; dS_dinput [n][in_width], written only if
	// any_curvature() (else it is zero and nothing is launched for it); gradients per mode.
	void second_order_finish(hipStream_t stream, SecondOrderPass& s, uint32_t n, const void* v, void* dL_ddLdoutput, void* dS_dinput, const void* params, void* gradients,
	                         GradientMode mode) const {
		const uint32_t K = m_desc.n_layers;
		const bool curved = any_curvature();
		const bool want_grads = mode != GradientMode::Ignore;
		const bool want_p = curved && (want_grads || dS_dinput);
		if (!dL_ddLdoutput && !want_grads && !(curved && dS_dinput)) return;
		if (want_grads) CHECK_THROW(gradients != nullptr);
		if (want_grads || want_p) CHECK_THROW(s.have_d);
		const void* p = params;
		ArenaBuf u{stream, K * s.slot * element_size()}, r;
		if (want_p) r = ArenaBuf{stream, K * s.slot * element_size()};
		auto u_of = [&](uint32_t l) { return l == K - 1 && dL_ddLdoutput ? dL_ddLdoutput : at(u.data(), s.slot * l); };
		const void* in = v;
		uint32_t ldi = m_input_width;
		for (uint32_t l = 0; l < K; ++l) {
			const MlpLayer& L = m_desc.layers[l];
			const bool curv = want_p && has_curvature(layer_act(l));
			const void* g = l == K - 1 ? s.dL_doutput : at((const void*)s.g.data(), s.slot * l);
			mlp_layer_tangent(stream, precision(), n, in, ldi, at(p, L.w_off), L.rows, L.cols, layer_act(l), aux_of(s, l), curv ? g : nullptr, u_of(l), curv ? at(r.data(), s.slot * l) : nullptr, layer_ld(l));
			in = u_of(l);
			ldi = m_width;
		}
		uint32_t top = 0; // the last layer with curvature: p_k = 0 above it
		for (uint32_t l = 0; l < K; ++l) if (has_curvature(layer_act(l))) top = l;
		if (want_p) {
			if (dS_dinput && !s.have_wt0) {
				mlp_layer_transpose(stream, precision(), m_desc.layers[0].rows, m_desc.layers[0].cols, p, s.wt.data());
				s.have_wt0 = true;
			}
			for (uint32_t l = top; l > 0; --l) {
				const MlpLayer& L = m_desc.layers[l];
				void* below = at(r.data(), s.slot * (l - 1));
				mlp_layer_curvature_backward(stream, precision(), n, at(r.data(), s.slot * l), layer_ld(l), at(s.wt.data(), L.w_off), L.rows, L.cols, layer_act(l - 1), aux_of(s, l - 1),
				                         has_curvature(layer_act(l - 1)) ? below : nullptr, below, m_width);
			}
			if (dS_dinput) {
				const MlpLayer& L = m_desc.layers[0];
				mlp_layer_backward(stream, precision(), n, r.data(), layer_ld(0), s.wt.data(), L.rows, L.cols, (uint32_t)Activation::None, nullptr, dS_dinput, m_input_width);
			}
		}
		if (!want_grads) return;
		// dS/dW_k = d_k^T u_{k-1}, then += p_k^T h_{k-1} for the layers up to `top` (the sum is rounded to the network's precision once per term)
		std::vector<WgradPanel> panels;
		for (uint32_t pass = 0; pass < (want_p ? 2u : 1u); ++pass) {
			panels.clear();
			for (uint32_t l = 0; l < (pass ? top + 1 : K); ++l) {
				const MlpLayer& L = m_desc.layers[l];
				const void* dO = pass ? at((const void*)r.data(), s.slot * l) : d_of(s, l);
				const void* In = l == 0 ? (pass ? s.input : v) : pass ? at((const void*)s.h.data(), s.slot * (l - 1)) : at((const void*)u.data(), s.slot * (l - 1));
				add_wgrad_panels(panels, L, dO, layer_ld(l), In, l == 0 ? m_input_width : m_width, at(gradients, L.w_off));
			}
			launch_wgrad_panels(stream, n, panels, pass ? true : mode == GradientMode::Accumulate);
		}
	}

	Json hyperparams() const { // fully_fused_mlp.h:137-145
		Json j = Json::object();
		j["otype"] = m_fully_fused ? "FullyFusedMLP" : "CutlassMLP";
		j["activation"] = to_string(m_activation);
		j["output_activation"] = to_string(m_output_activation);
		j["n_neurons"] = m_width;
		j["n_hidden_layers"] = m_n_hidden;
		return j;
	}

private:
	// ---- the layer-by-layer path (cutlass_mlp.cu:140-300): activations [n][width] in memory, one GEMM launch per layer
	// `elems` elements of the network's precision behind base (null stays null)
	const void* at(const void* base, size_t elems) const { return base ? (const char*)base + elems * element_size() : nullptr; }
	void* at(void* base, size_t elems) const { return base ? (char*)base + elems * element_size() : nullptr; }
	uint32_t layer_act(uint32_t l) const { return (uint32_t)(l == m_desc.n_layers - 1 ? m_output_activation : m_activation); }
	uint32_t layer_ld(uint32_t l) const { return l == m_desc.n_layers - 1 ? m_padded_output_width : m_width; } // of the layer's output

	// hidden: [n_hidden][n][width] post-activations (nullptr: inference, two rotating buffers); pre: the same for the pre-activations (Sine)
	void forward_layers(hipStream_t stream, uint32_t n, const void* input, void* output, const void* params, void* hidden, void* pre) const {
		const size_t hstride = (size_t)n * m_width;
		ArenaBuf rotate;
		if (!hidden && m_n_hidden > 0) rotate = ArenaBuf{stream, std::min<size_t>(m_n_hidden, 2) * hstride * element_size()};
		const void* in = input;
		uint32_t ldi = m_input_width;
		for (uint32_t l = 0; l < m_desc.n_layers; ++l) {
			const MlpLayer& L = m_desc.layers[l];
			const bool last = l == m_desc.n_layers - 1;
			void* out = last ? output : hidden ? at(hidden, hstride * l) : at(rotate.data(), hstride * (l & 1));
			void* p = !last && pre ? at(pre, hstride * l) : nullptr;
			mlp_layer_forward(stream, precision(), n, in, ldi, at(params, L.w_off), L.rows, L.cols, layer_act(l), out, layer_ld(l), p);
			in = out;
			ldi = m_width;
		}
	}

	void backward_layers(hipStream_t stream, const NetworkContext& ctx, uint32_t n, const void* input, const void* dY, void* dL_dinput, const void* params, void* gradients,
	                     GradientMode mode) const {
		const size_t hstride = (size_t)n * m_width;
		const bool sine = m_activation == Activation::Sine;
		const void* hidden = ctx.hidden.data();
		const void* aux = sine ? ctx.pre.data() : hidden; // what act' reads: cos of the pre-activation for Sine, else the output
		ArenaBuf dhidden{stream, (size_t)m_n_hidden * hstride * element_size()};
		// W^T of every layer that passes a gradient on: layer 0 only when dL/dinput is wanted
		ArenaBuf wt{stream, m_n_params * element_size()};
		const void* p = params;
		for (uint32_t l = dL_dinput ? 0 : 1; l < m_desc.n_layers; ++l) {
			const MlpLayer& L = m_desc.layers[l];
			mlp_layer_transpose(stream, precision(), L.rows, L.cols, at(p, L.w_off), at(wt.data(), L.w_off));
		}
		for (uint32_t l = m_desc.n_layers; l-- > 0;) {
			const MlpLayer& L = m_desc.layers[l];
			const void* dO = l == m_desc.n_layers - 1 ? dY : at((const void*)dhidden.data(), hstride * l);
			const uint32_t ldo = layer_ld(l);
			if (l > 0) { // dL/d(hidden l - 1), through the derivative of its activation
				mlp_layer_backward(stream, precision(), n, dO, ldo, at(wt.data(), L.w_off), L.rows, L.cols, (uint32_t)m_activation, at(aux, hstride * (l - 1)), at(dhidden.data(), hstride * (l - 1)), m_width);
			} else if (dL_dinput) {
				mlp_layer_backward(stream, precision(), n, dO, ldo, at(wt.data(), L.w_off), L.rows, L.cols, (uint32_t)Activation::None, nullptr, dL_dinput, m_input_width);
			}
		}
		if (mode == GradientMode::Ignore) return;
		CHECK_THROW(gradients != nullptr);
		// weight gradients: mlp_wgrad_panels on the row-major buffers, panels of at most 128 x 128, launched in groups whose fp32 slabs
		// fit a bounded workspace (a 1024-wide layer is 64 panels of up to 256 slabs each; the groups run in stream order and share it)
		std::vector<WgradPanel> panels;
		for (uint32_t l = 0; l < m_desc.n_layers; ++l) {
			const MlpLayer& L = m_desc.layers[l];
			const void* dO = l == m_desc.n_layers - 1 ? dY : at((const void*)dhidden.data(), hstride * l);
			const void* In = l == 0 ? input : at(hidden, hstride * (l - 1));
			add_wgrad_panels(panels, L, dO, layer_ld(l), In, l == 0 ? m_input_width : m_width, at(gradients, L.w_off));
		}
		launch_wgrad_panels(stream, n, panels, mode == GradientMode::Accumulate);
	}

	// what a' (and a'') of layer l are evaluated from in the second-order pass: z_l where the layer has curvature, else h_l (the sign)
	const void* aux_of(const SecondOrderPass& s, uint32_t l) const {
		if (layer_act(l) == (uint32_t)Activation::None) return nullptr;
		return at((const void*)(has_curvature(layer_act(l)) ? s.z.data() : s.h.data()), s.slot * l);
	}
	const void* d_of(const SecondOrderPass& s, uint32_t l) const { // d_K = g_K for an output layer without activation
		return l == m_desc.n_layers - 1 && layer_act(l) == (uint32_t)Activation::None ? s.dL_doutput : at((const void*)s.d.data(), s.slot * l);
	}

	// panels of at most 128 x 128 of one layer's weight gradient.  Row-major operands: a panel's first column is that many elements in; tiled
	// ones (the fused kernels' hidden matrices, k_mlp.hip hidden_tile_off): whole tiles of 16 columns x 16 samples = 256 elements in
	void add_wgrad_panels(std::vector<WgradPanel>& panels, const MlpLayer& L, const void* dO, uint32_t ldo, const void* In, uint32_t ldi, void* g, bool dO_tiled = false,
	                      bool In_tiled = false) const {
		for (uint32_t r0 = 0; r0 < L.rows; r0 += 128)
			for (uint32_t c0 = 0; c0 < L.cols; c0 += 128)
				panels.push_back(WgradPanel{at(dO, dO_tiled ? (size_t)(r0 / 16) * 256 : r0), ldo, std::min(128u, L.rows - r0), at(In, In_tiled ? (size_t)(c0 / 16) * 256 : c0), ldi,
				                            std::min(128u, L.cols - c0), at(g, (size_t)r0 * L.cols + c0), L.cols, dO_tiled, In_tiled});
	}

	void launch_wgrad_panels(hipStream_t stream, uint32_t n, const std::vector<WgradPanel>& panels, bool accumulate) const {
		constexpr size_t WORKSPACE_FLOATS = (size_t)64 << 20; // 256 MB
		auto workspace_floats = [&](const WgradPanel* p, size_t count) { return wgrad_panels_workspace_floats(precision(), p, (uint32_t)count, n); };
		size_t max_floats = 0;
		for (const WgradPanel& q : panels) max_floats = std::max(max_floats, workspace_floats(&q, 1));
		ArenaBuf ws{stream, std::max(max_floats, std::min(WORKSPACE_FLOATS, workspace_floats(panels.data(), panels.size()))) * sizeof(float)};
		const size_t ws_floats = ws.bytes() / sizeof(float);
		for (size_t i = 0; i < panels.size();) {
			size_t j = i, floats = 0;
			while (j < panels.size() && floats + workspace_floats(&panels[j], 1) <= ws_floats) floats += workspace_floats(&panels[j++], 1);
			mlp_wgrad_panels(stream, precision(), n, panels.data() + i, (uint32_t)(j - i), accumulate, ws.as<float>());
			i = j;
		}
	}

	bool m_fully_fused;
	bool m_layerwise = false;
	bool m_fp32 = false;
	uint32_t m_input_width, m_output_width, m_padded_output_width, m_width, m_n_hidden;
	Activation m_activation, m_output_activation;
	MlpDesc m_desc;
	size_t m_n_params;
	mutable LiveImage m_live;
	mutable int m_live_state = 0; // 0: not built yet, 1: usable, -1: not usable for this network
};

// ------------------------------------------------------------------------------------------------------------------
// Model = DifferentiableObject<float, T, T> (object.h:120-270)
// ------------------------------------------------------------------------------------------------------------------
struct ModelContext {
	virtual ~ModelContext() {}
};

class Model {
public:
	virtual ~Model() {}
	virtual uint32_t input_width() const = 0;
	virtual uint32_t output_width() const = 0;
	virtual uint32_t padded_output_width() const = 0;
	virtual size_t n_params() const = 0;
	virtual Precision precision() const = 0;
	virtual std::vector<std::pair<uint32_t, uint32_t>> layer_sizes() const = 0;
	virtual void initialize_params(Pcg32& rng, float* params_full_precision, float scale) = 0;
	virtual uint64_t list_scatters() const { return 0; } // backward passes of the model's grid encoding(s) that ran the list-fed gradient kernel
	virtual uint64_t list_gradient_tails() const { return 0; } // fused steps whose MLP kernel stored dL/dy in list order itself (no k_grid_list_gradients launch)
	// max_level of the model's grid encoding(s) (Encoding::set_max_level); false: the model has none
	virtual Encoding* input_encoding() { return nullptr; }
	bool set_max_level(float max_level) { Encoding* e = input_encoding(); return e && e->set_max_level(max_level); }
	bool set_max_level_gpu(const float* per_sample) { Encoding* e = input_encoding(); return e && e->set_max_level_gpu(per_sample); }
	bool get_max_level(float& max_level, const float*& per_sample) { Encoding* e = input_encoding(); return e && e->get_max_level(max_level, per_sample); }
	virtual void inference(hipStream_t stream, uint32_t n, MatView input, void* output, const void* params) = 0;
	// float output of the unpadded width (object.h:147-176: inference + trim_and_cast_from); models may fuse the conversion
	virtual void inference_f32(hipStream_t stream, uint32_t n, MatView input, MatViewMut output, const void* params) {
		check_batch(n);
		if (n == 0) return;
		const uint32_t pw = padded_output_width();
		ArenaBuf tmp{stream, (size_t)n * pw * (precision() == Precision::Fp32 ? 4 : 2)};
		inference(stream, n, input, tmp.data(), params);
		trim_and_cast(stream, precision() == Precision::Fp32, n, pw, output_width(), tmp.data(), output);
	}
	virtual std::unique_ptr<ModelContext> forward(hipStream_t stream, uint32_t n, MatView input, void* output, const void* params, bool prepare_input_gradients) = 0;
	virtual void backward(hipStream_t stream, const ModelContext& ctx, uint32_t n, MatView input, const void* output, const void* dL_doutput,
	                      MatViewMut* dL_dinput, const void* params, void* gradients, GradientMode mode) = 0;
	// object.h:278-331: second-order input gradients.  dL_ddLdinput [n][input_width] float arrives at dL_dinput; optional
	// results: dL_ddLdoutput [n][padded_output_width], dL_dinput (overwritten), parameter gradients per `mode`.
	virtual void backward_backward_input(hipStream_t stream, const ModelContext& ctx, uint32_t n, MatView input, MatView dL_ddLdinput, const void* dL_doutput,
	                                     void* dL_ddLdoutput, MatViewMut* dL_dinput, const void* params, void* gradients, GradientMode mode) {
		throw std::runtime_error{"DifferentiableObject::backward_backward_input_impl: not implemented error"}; // object.h:288
	}
	// object.h:342-366: d_dinput [n][input_width] = d output[dim] / d input with the caller's (inference) parameters; no parameter gradient is
	// touched and no context is left.  output (optional): the forward pass's output [n][padded_output_width] in the module's precision.
	// Every route gives what the generic one gives, bit for bit: d_doutput = (T)backprop_scale in column dim and +0 elsewhere,
	// forward(prepare_input_gradients), backward(GradientMode::Ignore), times 1.0f / backprop_scale (formed once, the reference's `mult`).
	void input_gradient(hipStream_t stream, uint32_t n, uint32_t dim, MatView input, MatViewMut d_dinput, void* output, const void* params, float backprop_scale) {
		if (dim >= padded_output_width()) throw std::runtime_error{"Invalid dimension to compute the input gradient for."}; // object.h:350
		check_batch(n);
		CHECK_THROW(n == 0 || (input.data != nullptr && d_dinput.data != nullptr));
		if (n == 0) return;
		m_last_input_gradient_route = input_gradient_impl(stream, n, dim, input, d_dinput, output, params, backprop_scale);
		input_gradient_rescale(stream, n, input_width(), 1.0f / backprop_scale, d_dinput);
	}
	const char* last_input_gradient_route() const { return m_last_input_gradient_route.c_str(); } // "none" before the first call
	// input_gradient for n_dims output columns from ONE forward pass: jacobian [n][n_dims][input_width] floats, row-major; rows [:, k, :] are
	// bit for bit what input_gradient(dim = dims[k]) gives, and output is the output it gives.  dims (host): any order, repeats and padded
	// columns allowed, 1 <= n_dims <= padded_output_width().  Everything is checked before anything is allocated or launched.
	void input_jacobian(hipStream_t stream, uint32_t n, const uint32_t* dims, uint32_t n_dims, MatView input, float* jacobian, void* output, const void* params, float backprop_scale) {
		if (!dims || n_dims == 0 || n_dims > padded_output_width()) {
			throw std::runtime_error{"input_jacobian: n_dims = " + std::to_string(n_dims) + " must be between 1 and the padded output width " + std::to_string(padded_output_width()) +
			                         ", with that many dims"};
		}
		for (uint32_t k = 0; k < n_dims; ++k) {
			if (dims[k] >= padded_output_width()) throw std::runtime_error{"Invalid dimension to compute the input gradient for."}; // object.h:350
		}
		check_batch(n);
		CHECK_THROW(n == 0 || (input.data != nullptr && jacobian != nullptr));
		if (n == 0) return;
		m_last_input_jacobian_route = input_jacobian_impl(stream, n, dims, n_dims, input, jacobian, output, params, backprop_scale);
		input_gradient_rescale(stream, n, n_dims * input_width(), 1.0f / backprop_scale, MatViewMut{jacobian, n_dims * input_width(), 1u});
	}
	const char* last_input_jacobian_route() const { return m_last_input_jacobian_route.c_str(); } // "none" before the first call
	// Forward mode: jvp [n][n_tangents][padded_output_width] in the module's precision, jvp[:, t, :] = J(x) tangents[:, t, :] for tangents
	// [n][n_tangents][input_width] floats, row-major -- every output column's derivative along n_tangents input directions, at inference:
	// no parameter gradient is touched and no context is left.  output (optional) is bit for bit inference()'s.  On the "two-pass" route
	// jvp[:, t, :] is bit for bit the dL_ddLdoutput of forward(prepare_input_gradients) + backward_backward_input(dL_ddLdinput =
	// tangents[:, t, :]) wherever that pass exists.  No backprop_scale: the map is linear in v, a caller who fears half overflow scales v.
	// Everything is checked before anything is allocated or launched; a refused call leaves the route strings alone.
	void input_jvp(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, void* jvp, void* output, const void* params) {
		if (!tangents) throw std::runtime_error{"input_jvp: tangents must not be NULL"};
		if (!jvp) throw std::runtime_error{"input_jvp: jvp must not be NULL"};
		if (n_tangents == 0) throw std::runtime_error{"input_jvp: n_tangents = 0 must be at least 1"};
		check_batch(n);
		if (!has_tangent()) throw std::runtime_error{"input_jvp: not implemented for " + name()};
		CHECK_THROW(n == 0 || input.data != nullptr);
		if (n == 0) return;
		m_last_input_jvp_route = input_jvp_impl(stream, n, n_tangents, input, tangents, jvp, output, params);
	}
	const char* last_input_jvp_route() const { return m_last_input_jvp_route.c_str(); } // "none" before the first call

	// ---- Training through input_jvp (DESIGN.md "Training through input_jvp").  input_jvp_forward() is input_jvp() -- the same route, the
	// same bits in jvp and output -- and returns a context that holds no device memory: input_jvp_backward() runs the module's
	// forward(prepare_input_gradients) again from x, which is cheaper to repeat than to keep for every pending call.
	struct InputJvpContext : public ModelContext {
		uint32_t n = 0, n_tangents = 0;
	};
	std::unique_ptr<ModelContext> input_jvp_forward(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, void* jvp, void* output, const void* params) {
		input_jvp(stream, n, n_tangents, input, tangents, jvp, output, params);
		auto ctx = std::make_unique<InputJvpContext>();
		ctx->n = n;
		ctx->n_tangents = n_tangents;
		return ctx;
	}
	// The gradients of L = sum_t <dL_djvp[:, t, :], J(x) tangents[:, t, :]> + <dL_doutput, f(x)>, first order only.  dL_djvp
	// [n][n_tangents][padded_output_width] and dL_doutput [n][padded_output_width] (optional) in the module's precision, taken as they are
	// (no loss scale inside).  Optional results: gradients per `mode`, dL_dinput [n][input_width] and dL_dtangents
	// [n][n_tangents][input_width] floats.  Only what is asked for is computed.  Everything is checked before anything is allocated or
	// launched; a refused call leaves the route strings alone.
	void input_jvp_backward(hipStream_t stream, const ModelContext& mctx, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, const void* dL_djvp,
	                        const void* dL_doutput, const void* params, void* gradients, MatViewMut* dL_dinput, float* dL_dtangents, GradientMode mode) {
		if (!tangents) throw std::runtime_error{"input_jvp_backward: tangents must not be NULL"};
		if (!dL_djvp) throw std::runtime_error{"input_jvp_backward: dL_djvp must not be NULL"};
		if (n_tangents == 0) throw std::runtime_error{"input_jvp_backward: n_tangents = 0 must be at least 1"};
		check_batch(n);
		if (!has_tangent()) throw std::runtime_error{"input_jvp: not implemented for " + name()};
		const InputJvpContext* ctx = dynamic_cast<const InputJvpContext*>(&mctx);
		if (!ctx) throw std::runtime_error{"Module::bwd: called with invalid context. fwd likely (mistakenly) ran in inference mode."};
		if (ctx->n != n || ctx->n_tangents != n_tangents) {
			throw std::runtime_error{"input_jvp_backward: the context is of a call with n = " + std::to_string(ctx->n) + ", n_tangents = " + std::to_string(ctx->n_tangents)};
		}
		const bool want_grads = mode != GradientMode::Ignore;
		CHECK_THROW(!want_grads || gradients != nullptr);
		// d/dx of an encoding's tangent is its second-order pass: OneBlob has a tangent but no k''
		Encoding* e = input_encoding();
		const bool encoding_second_order = !e || e->has_second_order();
		if (dL_dinput && !encoding_second_order) throw std::runtime_error{"input_jvp_backward: dL_dinput not implemented for " + name()};
		if (want_grads && !encoding_second_order && e->n_params() > 0) throw std::runtime_error{"input_jvp_backward: dL_dparams not implemented for " + name()};
		CHECK_THROW(n == 0 || (input.data != nullptr && (params != nullptr || n_params() == 0)));
		if (n == 0 || (!want_grads && !dL_dinput && !dL_dtangents)) return;
		m_last_input_jvp_backward_route = input_jvp_backward_impl(stream, n, n_tangents, input, tangents, dL_djvp, dL_doutput, params, want_grads ? gradients : nullptr, dL_dinput, dL_dtangents, mode);
	}
	const char* last_input_jvp_backward_route() const { return m_last_input_jvp_backward_route.c_str(); } // "none" before the first call
	virtual bool has_tangent() const { return false; } // false: PPNG1 / PPNG2 (or a Composite holding one) is part of the module
	virtual Json hyperparams() const = 0;
	std::string name() const { return hyperparams().value("otype", "<Unknown>"); } // object.h:51-53
protected:
	// writes d_dinput scaled by backprop_scale and returns the route's name.  The generic route, for every module:
	virtual std::string input_gradient_impl(hipStream_t stream, uint32_t n, uint32_t dim, MatView input, MatViewMut d_dinput, void* output, const void* params, float backprop_scale) {
		input_gradient_two_pass(stream, n, dim, input, d_dinput, output, params, backprop_scale);
		return "two-pass";
	}
	void input_gradient_two_pass(hipStream_t stream, uint32_t n, uint32_t dim, MatView input, MatViewMut d_dinput, void* output, const void* params, float backprop_scale) {
		const uint32_t pw = padded_output_width();
		const size_t bytes = (size_t)n * pw * (precision() == Precision::Fp32 ? 4 : 2);
		ArenaBuf out_tmp, d_doutput{stream, bytes};
		if (!output) out_tmp = ArenaBuf{stream, bytes};
		void* out = output ? output : out_tmp.data();
		input_gradient_one_hot(stream, precision(), n, pw, dim, backprop_scale, d_doutput.data());
		const std::unique_ptr<ModelContext> ctx = forward(stream, n, input, out, params, true);
		backward(stream, *ctx, n, input, out, d_doutput.data(), &d_dinput, params, nullptr, GradientMode::Ignore);
	}
	// writes the jacobian scaled by backprop_scale and returns the route's name.  The generic route, for every module: ONE
	// forward(prepare_input_gradients), then a one-hot dL/dy and backward(GradientMode::Ignore) per dim on the same context, each into its
	// strided slice of the result (the encodings' input-gradient kernels write through any view).
	virtual std::string input_jacobian_impl(hipStream_t stream, uint32_t n, const uint32_t* dims, uint32_t n_dims, MatView input, float* jacobian, void* output, const void* params,
	                                        float backprop_scale) {
		input_jacobian_two_pass(stream, n, dims, n_dims, input, jacobian, output, params, backprop_scale);
		return "two-pass";
	}
	void input_jacobian_two_pass(hipStream_t stream, uint32_t n, const uint32_t* dims, uint32_t n_dims, MatView input, float* jacobian, void* output, const void* params, float backprop_scale) {
		const uint32_t pw = padded_output_width();
		const size_t bytes = (size_t)n * pw * (precision() == Precision::Fp32 ? 4 : 2);
		ArenaBuf out_tmp, d_doutput{stream, bytes};
		if (!output) out_tmp = ArenaBuf{stream, bytes};
		void* out = output ? output : out_tmp.data();
		const std::unique_ptr<ModelContext> ctx = forward(stream, n, input, out, params, true);
		for (uint32_t k = 0; k < n_dims; ++k) {
			input_gradient_one_hot(stream, precision(), n, pw, dims[k], backprop_scale, d_doutput.data());
			MatViewMut slice = jacobian_slice(jacobian, k, n_dims);
			backward(stream, *ctx, n, input, out, d_doutput.data(), &slice, params, nullptr, GradientMode::Ignore);
		}
	}
	// rows [:, k, :] of the [n][n_dims][input_width] result as a view of [n][input_width]
	MatViewMut jacobian_slice(float* jacobian, uint32_t k, uint32_t n_dims) const { return MatViewMut{jacobian + (size_t)k * input_width(), n_dims * input_width(), 1u}; }
	// writes jvp and returns the route's name.  The generic route, for every module with a tangent: ONE forward(prepare_input_gradients),
	// then the module's tangent per direction on that context -- its second-order pass asked for dL_ddLdoutput alone -- into a row-major
	// [n][padded_output_width] buffer that is copied into its columns of the result (one direction: written in place).
	virtual std::string input_jvp_impl(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, void* jvp, void* output, const void* params) {
		input_jvp_two_pass(stream, n, n_tangents, input, tangents, jvp, output, params);
		return "two-pass";
	}
	// t [n][padded_output_width] = J v on the context of a forward(prepare_input_gradients); v: a view of [n][input_width] floats
	virtual void tangent(hipStream_t stream, const ModelContext& ctx, uint32_t n, MatView input, MatView v, void* t, const void* params) {
		throw std::runtime_error{"input_jvp: not implemented for " + name()};
	}
	void input_jvp_two_pass(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, void* jvp, void* output, const void* params) {
		const uint32_t pw = padded_output_width();
		const size_t elem = precision() == Precision::Fp32 ? 4 : 2, bytes = (size_t)n * pw * elem;
		ArenaBuf out_tmp, one;
		if (!output) out_tmp = ArenaBuf{stream, bytes};
		if (n_tangents > 1) one = ArenaBuf{stream, bytes};
		const std::unique_ptr<ModelContext> ctx = forward(stream, n, input, output ? output : out_tmp.data(), params, true);
		for (uint32_t t = 0; t < n_tangents; ++t) {
			void* dst = n_tangents > 1 ? one.data() : jvp;
			tangent(stream, *ctx, n, input, tangent_slice(tangents, t, n_tangents), dst, params);
			if (n_tangents > 1) copy_columns(stream, elem, n, dst, pw, 0, jvp, n_tangents * pw, t * pw, pw);
		}
	}
	// The composed route of input_jvp_backward(), for every module with a tangent, from existing passes alone.  <u, J(x, theta) v>
	// differentiated by theta and x is what the second-order pass gives for dL_ddLdinput = v and dL_doutput = u, and by v it is the
	// first-order J^T u.  So, on ONE forward(prepare_input_gradients):
	//   first           backward(dL_doutput), if there is one: the parameter gradients under the caller's mode, dL_dinput written in place
	//   per tangent t   tangent_reverse(v_t, u_t) -- the second-order pass -- for the parameter gradients (the caller's mode if nothing was
	//                   written before, else Accumulate) and dL_dinput (likewise in place, else added in order);
	//                   backward(dL_doutput = u_t, Ignore) into the tangent's strided slice of dL_dtangents
	// with u_t = dL_djvp[:, t, :] copied out of the caller's matrix (one tangent: read in place).  Every result is bit for bit what a caller
	// gets who chains forward / backward / backward_backward_input by hand in this order, accumulating the parameter gradients through the
	// second-order pass's Accumulate mode and adding the input gradients in fp32, where the module has those passes.
	virtual std::string input_jvp_backward_impl(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, const void* dL_djvp, const void* dL_doutput,
	                                            const void* params, void* gradients, MatViewMut* dL_dinput, float* dL_dtangents, GradientMode mode) {
		const uint32_t pw = padded_output_width(), w = input_width();
		const size_t elem = precision() == Precision::Fp32 ? 4 : 2, bytes = (size_t)n * pw * elem;
		const bool want_grads = gradients != nullptr && mode != GradientMode::Ignore;
		ArenaBuf out{stream, bytes}, one, dx_more;
		if (n_tangents > 1) one = ArenaBuf{stream, bytes};
		MatViewMut dx_view{nullptr, w, 1u};
		if (dL_dinput && (n_tangents > 1 || dL_doutput)) {
			dx_more = ArenaBuf{stream, (size_t)n * w * sizeof(float)};
			dx_view.data = dx_more.as<float>();
		}
		const std::unique_ptr<ModelContext> ctx = forward(stream, n, input, out.data(), params, true);
		bool first = true; // nothing written yet: the next pass writes the gradients under the caller's mode and dL_dinput in place
		if (dL_doutput && (want_grads || dL_dinput)) {
			backward(stream, *ctx, n, input, out.data(), dL_doutput, dL_dinput, params, gradients, want_grads ? mode : GradientMode::Ignore);
			first = false;
		}
		for (uint32_t t = 0; t < n_tangents; ++t) {
			const void* u = dL_djvp;
			if (n_tangents > 1) {
				copy_columns(stream, elem, n, dL_djvp, n_tangents * pw, t * pw, one.data(), pw, 0, pw);
				u = one.data();
			}
			if (want_grads || dL_dinput) {
				MatViewMut* dx = !dL_dinput ? nullptr : first ? dL_dinput : &dx_view;
				tangent_reverse(stream, *ctx, n, input, tangent_slice(tangents, t, n_tangents), u, dx, params, gradients, !want_grads ? GradientMode::Ignore : first ? mode : GradientMode::Accumulate);
				if (dL_dinput && !first) add_input_gradient(stream, n, w, MatView{dx_view.data, dx_view.stride_sample, dx_view.stride_dim}, *dL_dinput);
				first = false;
			}
			if (dL_dtangents) {
				MatViewMut slice{dL_dtangents + (size_t)t * w, n_tangents * w, 1u};
				backward(stream, *ctx, n, input, out.data(), u, &slice, params, nullptr, GradientMode::Ignore);
			}
		}
		return "two-pass";
	}
	// the second-order pass as input_jvp_backward() needs it: backward_backward_input() asked for dL_dinput and the parameter gradients.
	// A model whose public pass refuses modules that this one serves (FullyFusedMLP, OneBlob) overrides it.
	virtual void tangent_reverse(hipStream_t stream, const ModelContext& ctx, uint32_t n, MatView input, MatView v, const void* u, MatViewMut* dL_dinput, const void* params,
	                             void* gradients, GradientMode mode) {
		backward_backward_input(stream, ctx, n, input, v, u, nullptr, dL_dinput, params, gradients, mode);
	}
	// rows [:, t, :] of the [n][n_tangents][input_width] tangents as a view of [n][input_width]
	MatView tangent_slice(const float* tangents, uint32_t t, uint32_t n_tangents) const { return MatView{tangents + (size_t)t * input_width(), n_tangents * input_width(), 1u}; }
private:
	std::string m_last_input_gradient_route = "none";
	std::string m_last_input_jacobian_route = "none";
	std::string m_last_input_jvp_route = "none";
	std::string m_last_input_jvp_backward_route = "none";
public:

	static void check_batch(uint32_t n) { // object.h:130,150,197,246
		if (n % BATCH_SIZE_GRANULARITY != 0) throw std::runtime_error{"batch size " + std::to_string(n) + " is not a multiple of BATCH_SIZE_GRANULARITY = 256"};
	}
};

// Event brackets around the pieces of ONE fused training step, on the step's stream (the measurement hook of bench.py, SURVEY 8d:
// "time the MLP fwd+bwd+wgrad region separately").  Events are created without the system-scope release a default event
// performs (hipEventDisableSystemFence): that write-back made a bracketed kernel 40 % slower than it is inside a step.
struct StepProfile {
	enum Piece { Encode = 0, MlpKernel = 1, EncodingBackward = 2, Optimizer = 3, N_PIECES = 4 };
	struct Sample { hipEvent_t begin[N_PIECES], end[N_PIECES]; bool used[N_PIECES]; };
	std::vector<Sample> samples;
	bool armed = false;
	Sample* current = nullptr;

	void arm() { armed = true; }
	void begin_step() {
		current = nullptr;
		if (!armed) return;
		armed = false;
		samples.emplace_back();
		current = &samples.back();
		for (int i = 0; i < N_PIECES; ++i) {
			current->used[i] = false;
			HIP_CHECK_THROW(hipEventCreateWithFlags(&current->begin[i], 0x20000000u)); // hipEventDisableSystemFence, timing enabled
			HIP_CHECK_THROW(hipEventCreateWithFlags(&current->end[i], 0x20000000u));
		}
	}
	void mark(hipStream_t stream, Piece p, bool end) {
		if (!current) return;
		HIP_CHECK_THROW(hipEventRecord(end ? current->end[p] : current->begin[p], stream));
		if (end) current->used[p] = true;
	}
	void end_step() { current = nullptr; }
	// sums over the profiled steps since the last call (milliseconds per piece) and their number; synchronises the stream
	uint32_t collect(hipStream_t stream, float* ms) {
		HIP_CHECK_THROW(hipStreamSynchronize(stream));
		for (int i = 0; i < N_PIECES; ++i) ms[i] = 0.0f;
		for (Sample& s : samples) {
			for (int i = 0; i < N_PIECES; ++i) {
				float t = 0.0f;
				if (s.used[i]) HIP_CHECK_THROW(hipEventElapsedTime(&t, s.begin[i], s.end[i]));
				ms[i] += t;
				(void)hipEventDestroy(s.begin[i]);
				(void)hipEventDestroy(s.end[i]);
			}
		}
		const uint32_t n = (uint32_t)samples.size();
		samples.clear();
		return n;
	}
	~StepProfile() {
		for (Sample& s : samples)
			for (int i = 0; i < N_PIECES; ++i) {
				(void)hipEventDestroy(s.begin[i]);
				(void)hipEventDestroy(s.end[i]);
			}
	}
};

// The data of one fused training step (NetworkWithInputEncoding::fused_step / fused_mlp_and_scatter).  target == nullptr requires
// external_dL_dy; out / dL_dout / L: [n][padded_out], or the compact [n][dims] matrices with compact_context (any may be null).
struct FusedStepData {
	const float* target = nullptr;
	const float* data_pdf = nullptr;
	const void* external_dL_dy = nullptr;
	LossType loss = LossType::L2;
	float loss_scale = 1.0f;
	void* out = nullptr;
	void* dL_dout = nullptr;
	float* L = nullptr;
	bool compact_context = false;
	MatViewMut* dL_dinput = nullptr;
	const void* params = nullptr;
	void* gradients = nullptr;
	GradientMode mode = GradientMode::Overwrite;
	StepProfile* profile = nullptr;
};
// Where the optimizer's update of a fused training step runs: decided once per step, by Trainer::training_step.
enum class OptimizerPlace { None, InReduce, Prologue, OwnLaunch };
// What that decision hands to the step -- at most one of the two:
struct OptimizerOffer {
	// InReduce: the slab reduction applies this update (k_wgrad_reduce_adam).  Binding: the step must be one whose reduction carries
	// it (NetworkWithInputEncoding::reduction_carries_update), and the caller launches no optimizer afterwards.
	const AdamInReduce* in_reduce = nullptr;
	// Prologue: the optimizer's launch offers to finish the gradients itself.  ->pending reports whether the backward pass took the offer.
	AdamPrologue* prologue = nullptr;
};

class NetworkWithInputEncoding : public Model {
public:
	// precision: of the whole module -- Fp32 creates the encoding in its fp32 form and the network as Network{json, Precision::Fp32}, so that
	// parameters, the encoded batch, output and every gradient are floats (mixed modules do not exist)
	NetworkWithInputEncoding(uint32_t n_dims_to_encode, uint32_t n_output_dims, const Json& encoding, const Json& network, Precision precision = Precision::Fp16) {
		// network_with_input_encoding.h:45-56: encoding aligned to the network's minimum alignment (16), network sized from it
		m_encoding = create_encoding(n_dims_to_encode, encoding, Network::REQUIRED_ALIGNMENT, precision == Precision::Fp32);
		Json local = network.is_object() ? network : Json::object();
		local["n_input_dims"] = m_encoding->padded_output_width();
		local["n_output_dims"] = n_output_dims;
		m_network.reset(new Network{local, precision});
	}

	uint32_t input_width() const override { return m_encoding->input_width(); }
	uint32_t output_width() const override { return m_network->output_width(); }
	uint32_t padded_output_width() const override { return m_network->padded_output_width(); }
	size_t n_params() const override { return m_network->n_params() + m_encoding->n_params(); }
	Precision precision() const override { return m_network->precision(); }
	std::vector<std::pair<uint32_t, uint32_t>> layer_sizes() const override { return m_network->layer_sizes(); }
	Encoding& encoding() { return *m_encoding; }
	Encoding* input_encoding() override { return m_encoding.get(); }
	Network& network() { return *m_network; }

	void initialize_params(Pcg32& rng, float* params_full_precision, float scale) override { // :124-130, network first
		m_network->initialize_params(rng, params_full_precision, scale);
		m_encoding->initialize_params(rng, params_full_precision + m_network->n_params(), scale);
	}

	void inference(hipStream_t stream, uint32_t n, MatView input, void* output, const void* params) override {
		inference_fused(stream, n, input, output, nullptr, params);
	}
	void inference_f32(hipStream_t stream, uint32_t n, MatView input, MatViewMut output, const void* params) override {
		inference_fused(stream, n, input, nullptr, &output, params);
	}

	// object.h:147-176 for this model, with as few passes over memory as the kernels allow: an Identity encoding is applied
	// inside the MLP kernel's input load, a grid is evaluated into level planes by the XCD-aware kernel, and the float
	// output (trim_and_cast_from) is written by the MLP kernel itself.
	void inference_fused(hipStream_t stream, uint32_t n, MatView input, void* output_half, const MatViewMut* output_f32, const void* params) {
		check_batch(n);
		if (n == 0) return;
		const _Float16* p = (const _Float16*)params;
		if (m_network->layerwise()) { // no fused input or output forms: the encoding's own kernel writes the batch, a trim casts the output
			// (output_half: the output in the module's precision)
			ArenaBuf network_input{stream, (size_t)n * m_encoding->padded_output_width() * elem()}, out_tmp;
			m_encoding->forward(stream, n, input, encoding_params(params), network_input.data(), false, false);
			if (!output_half) out_tmp = ArenaBuf{stream, (size_t)n * m_network->padded_output_width() * elem()};
			m_network->inference(stream, n, network_input.data(), output_half ? output_half : out_tmp.data(), params);
			if (output_f32) trim_and_cast(stream, elem() == 4, n, m_network->padded_output_width(), m_network->output_width(), output_half ? output_half : out_tmp.data(), *output_f32);
			return;
		}
		MlpIo io{};
		io.out_half = output_half;
		if (output_f32) {
			io.out_f32 = *output_f32;
			io.out_f32_dims = m_network->output_width();
		}
		ArenaBuf network_input;
		float scale = 1, offset = 0;
		if (m_encoding->as_identity(scale, offset)) {
			io.x_f32 = input;
			io.x_f32_dims = m_encoding->input_width();
			io.x_scale = scale;
			io.x_offset = offset;
		} else if (m_encoding->as_oneblob() && m_encoding->padded_output_width() == m_network->input_width() && (m_network->desc().width == 64 || m_network->desc().width == 128)) {
			io.x_f32 = input;
			io.x_f32_dims = m_encoding->input_width();
			io.x_oneblob_bins = m_encoding->as_oneblob();
		} else {
			network_input = ArenaBuf{stream, (size_t)n * m_encoding->padded_output_width() * 2};
			io.x_half = network_input.data();
			const ForwardPlan plan{m_encoding->forward_route(switches(), n, true, false, false)};
			io.x_plane_features = plan.route.plane_features;
			m_encoding->forward(stream, n, input, p + m_network->n_params(), network_input.data(), false, false, &plan);
		}
		m_network->inference_io(stream, n, io, p);
	}

	struct Ctx : public ModelContext {
		ArenaBuf network_input;     // AoS [n][padded], or level planes (encoding_ctx.route.plane_features > 0)
		EncodingContext encoding_ctx;
		NetworkContext network_ctx; // hidden activations; empty for fused contexts
		bool fused = false;         // produced by fused_encode(): backward() goes through the fused MLP kernel
		bool input_gradients = false; // forward() ran with prepare_input_gradients
		uint32_t oneblob_bins = 0;  // > 0: no encoded batch was written -- the MLP kernels evaluate the OneBlob encoding of the input themselves
		ArenaBuf image;             // the network's fragment images, if the encoding's forward kernel built them on the way (MlpPrepJob)
		// the MLP's weight-gradient slabs once their reduction was handed to a LATER launch (AdamPrologue: the optimizer's, enqueued after
		// fused_step returns): they stay allocated as long as this context does -- the arena's rule is "consumer enqueued before the free"
		mutable ArenaBuf slabs_kept;
	};

	// cpp_api.cu:84-95.  Without input gradients the forward pass keeps nothing but the encoded batch: backward() recomputes the
	// MLP's forward pass inside the fused kernel (k_train.hip) from it, which is cheaper than storing and re-reading the hidden
	// activations (k_mlp_fwd with hidden stores + k_mlp_bwd + 3 x k_wgrad: 158 us; the fused kernel: 78 us on C3a).
	std::unique_ptr<ModelContext> forward(hipStream_t stream, uint32_t n, MatView input, void* output, const void* params, bool prepare_input_gradients) override {
		check_batch(n);
		auto ctx = std::make_unique<Ctx>();
		ctx->input_gradients = prepare_input_gradients;
		if (n == 0) return ctx;
		const _Float16* p = (const _Float16*)params;
		if (!prepare_input_gradients && fused_step_supported(n)) {
			fused_encode(stream, *ctx, n, input, params, m_encoding->forward_route(switches(), n, true, false, true), false, true);
			MlpIo io{};
			if (ctx->oneblob_bins) {
				io.x_f32 = input;
				io.x_f32_dims = m_encoding->input_width();
				io.x_oneblob_bins = ctx->oneblob_bins;
			} else {
				io.x_half = ctx->network_input.data();
				io.x_plane_features = ctx->encoding_ctx.route.plane_features;
			}
			io.out_half = output;
			m_network->inference_io(stream, n, io, p);
			return ctx;
		}
		ctx->network_input = ArenaBuf{stream, (size_t)n * m_encoding->padded_output_width() * elem()};
		ctx->encoding_ctx = m_encoding->forward(stream, n, input, encoding_params(params), ctx->network_input.data(), prepare_input_gradients, true);
		ctx->network_ctx = m_network->forward(stream, n, ctx->network_input.data(), output, params);
		return ctx;
	}

	void backward(hipStream_t stream, const ModelContext& mctx, uint32_t n, MatView input, const void* output, const void* dL_doutput,
	              MatViewMut* dL_dinput, const void* params, void* gradients, GradientMode mode) override {
		check_batch(n);
		if (n == 0) return;
		const Ctx& ctx = dynamic_cast<const Ctx&>(mctx);
		if (ctx.fused) {
			if (dL_dinput) throw std::runtime_error{"NetworkWithInputEncoding::backward: input gradients were not prepared by forward()"};
			FusedStepData step;
			step.external_dL_dy = dL_doutput;
			step.params = params;
			step.gradients = gradients;
			step.mode = mode;
			fused_mlp_and_scatter(stream, switches(), ctx, n, input, step, OptimizerOffer{});
			return;
		}
		ArenaBuf dL_dnetwork_input;
		if (m_encoding->n_params() > 0 || dL_dinput) { // :93-96
			dL_dnetwork_input = ArenaBuf{stream, (size_t)n * m_encoding->padded_output_width() * elem()};
		}
		// the grid scatter reads dL/d(encoding) with unit stride when the MLP writes it as level planes
		const GridDyForm offer = dL_dnetwork_input && !m_network->layerwise() ? GridDyForm::Planes : GridDyForm::Rows;
		const GridBackwardRoute route = m_encoding->backward_route(switches(), stream, ctx.encoding_ctx, n, input, offer, dL_dinput != nullptr, mode);
		m_network->backward(stream, ctx.network_ctx, n, ctx.network_input.data(), output, dL_doutput, dL_dnetwork_input.data(), params, gradients, mode, route.plane_features);
		if (dL_dnetwork_input) {
			m_encoding->backward(stream, ctx.encoding_ctx, n, input, dL_dnetwork_input.data(), dL_dinput, encoding_params(params), encoding_params(gradients), mode, route);
		}
	}

	// object.h:342-366 for this model: the encoding's forward pass with dy_dx, the network's input_gradient by its plan (the fused kernel, or
	// forward + backward), the encoding's backward pass to dL/dinput -- the kernels forward(prepare_input_gradients) and backward(Ignore) run,
	// except that a fused network stores no activations.  An Identity encoding is applied inside the fused kernel's load, as at inference.
	// (A OneBlob encoding in front keeps the two passes: its fused input form is not part of the kernel.)
	std::string input_gradient_impl(hipStream_t stream, uint32_t n, uint32_t dim, MatView input, MatViewMut d_dinput, void* output, const void* params, float backprop_scale) override {
		MlpInputGradPlan plan = m_network->input_gradient_plan(n);
		if (m_encoding->as_oneblob()) plan = MlpInputGradPlan{};
		const uint32_t enc_w = m_encoding->padded_output_width();
		MlpIo io{};
		io.out_half = output;
		ArenaBuf network_input, out_tmp;
		EncodingContext encoding_ctx;
		float scale = 1, offset = 0;
		if (plan.fused && m_encoding->as_identity(scale, offset)) {
			io.x_f32 = input;
			io.x_f32_dims = m_encoding->input_width();
			io.x_scale = scale;
			io.x_offset = offset;
		} else {
			network_input = ArenaBuf{stream, (size_t)n * enc_w * elem()};
			encoding_ctx = m_encoding->forward(stream, n, input, encoding_params(params), network_input.data(), true, false);
			io.x_half = network_input.data();
		}
		if (!plan.fused && !output) { // the two passes read the output back
			out_tmp = ArenaBuf{stream, (size_t)n * m_network->padded_output_width() * elem()};
			io.out_half = out_tmp.data();
		}
		ArenaBuf dL_dnetwork_input{stream, (size_t)n * enc_w * elem()};
		const GridDyForm offer = !m_network->layerwise() ? GridDyForm::Planes : GridDyForm::Rows; // (as backward() offers it)
		const GridBackwardRoute route = m_encoding->backward_route(switches(), stream, encoding_ctx, n, input, offer, true, GradientMode::Ignore);
		m_network->input_gradient(stream, plan, n, io, dim, backprop_scale, params, dL_dnetwork_input.data(), route.plane_features);
		m_encoding->backward(stream, encoding_ctx, n, input, dL_dnetwork_input.data(), &d_dinput, encoding_params(params), nullptr, GradientMode::Ignore, route);
		return plan.name;
	}

	// input_gradient_impl for n_dims output columns: the encoding's forward pass with dy_dx runs ONCE (behind a grid it is most of an
	// input_gradient call), the network writes one dL/d(network input) buffer per dim -- the fused Jacobian kernel from one forward chain, or
	// one forward pass and a backward pass per dim -- and the encoding's backward pass runs per buffer into its strided slice of the result,
	// on one route asked once.  The buffers are temporaries: groups of as many dims as fit INPUT_JACOBIAN_TMP_BYTES at a time (a fused
	// network repeats its forward chain per group, a two-pass network its forward pass; the encoding pass is never repeated).
	static constexpr size_t INPUT_JACOBIAN_TMP_BYTES = (size_t)256 << 20; // (the bound of mlp_wgrad_panels' workspace)
	std::string input_jacobian_impl(hipStream_t stream, uint32_t n, const uint32_t* dims, uint32_t n_dims, MatView input, float* jacobian, void* output, const void* params,
	                                float backprop_scale) override {
		MlpInputGradPlan plan = m_network->input_jacobian_plan(n, n_dims);
		if (m_encoding->as_oneblob()) plan = MlpInputGradPlan{};
		const uint32_t enc_w = m_encoding->padded_output_width();
		MlpIo io{};
		io.out_half = output;
		ArenaBuf network_input, out_tmp;
		EncodingContext encoding_ctx;
		float scale = 1, offset = 0;
		if (plan.fused && m_encoding->as_identity(scale, offset)) {
			io.x_f32 = input;
			io.x_f32_dims = m_encoding->input_width();
			io.x_scale = scale;
			io.x_offset = offset;
		} else {
			network_input = ArenaBuf{stream, (size_t)n * enc_w * elem()};
			encoding_ctx = m_encoding->forward(stream, n, input, encoding_params(params), network_input.data(), true, false);
			io.x_half = network_input.data();
		}
		if (!plan.fused && !output) { // the two passes read the output back
			out_tmp = ArenaBuf{stream, (size_t)n * m_network->padded_output_width() * elem()};
			io.out_half = out_tmp.data();
		}
		const size_t buf_bytes = (size_t)n * enc_w * elem();
		const uint32_t group = (uint32_t)std::min<size_t>(n_dims, std::max<size_t>(INPUT_JACOBIAN_TMP_BYTES / std::max<size_t>(buf_bytes, 1), 1));
		ArenaBuf dL_dnetwork_input{stream, buf_bytes * group};
		const GridDyForm offer = !m_network->layerwise() ? GridDyForm::Planes : GridDyForm::Rows; // (as backward() offers it)
		const GridBackwardRoute route = m_encoding->backward_route(switches(), stream, encoding_ctx, n, input, offer, true, GradientMode::Ignore);
		for (uint32_t k0 = 0; k0 < n_dims; k0 += group) {
			const uint32_t n_group = std::min(group, n_dims - k0);
			m_network->input_jacobian(stream, plan, n, io, dims + k0, n_group, backprop_scale, params, dL_dnetwork_input.data(), route.plane_features);
			if (plan.fused) io.out_half = nullptr; // stored with the first group
			for (uint32_t k = 0; k < n_group; ++k) {
				MatViewMut slice = jacobian_slice(jacobian, k0 + k, n_dims);
				m_encoding->backward(stream, encoding_ctx, n, input, (const char*)dL_dnetwork_input.data() + k * buf_bytes, &slice, encoding_params(params), nullptr, GradientMode::Ignore, route);
			}
		}
		return plan.name;
	}

	// input_jvp for this model, mirroring input_jacobian_impl: the encoding's forward pass with dy_dx runs ONCE, the encoding's tangent
	// (Encoding::tangent: its second-order pass asked for dL_ddLdy alone, or OneBlob's kernel) runs per direction into buffers one behind
	// the other, and the network carries them to the output -- the fused kernel, or the layer-by-layer forward and tangent passes
	// (Network::input_jvp).  A fused plan behind an Identity encoding reads input and tangents through the fused Identity load and needs no
	// buffer.  The tangent buffers are temporaries: groups of as many directions as fit INPUT_JACOBIAN_TMP_BYTES at a time; a further group
	// repeats the network's forward chain, never the encoding pass.  (A grid tangent kernel that reads dy_dx once for all directions
	// is left for later: DESIGN.md "input_jvp".)
	bool has_tangent() const override { return m_encoding->has_tangent(); }
	std::string input_jvp_impl(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, void* jvp, void* output, const void* params) override {
		MlpInputJvpPlan plan = m_network->input_jvp_plan(n, n_tangents);
		if (m_encoding->as_oneblob()) plan = MlpInputJvpPlan{};
		const uint32_t enc_w = m_encoding->padded_output_width();
		MlpIo io{};
		io.out_half = output;
		ArenaBuf network_input, encoded_tangents;
		EncodingContext encoding_ctx;
		float scale = 1, offset = 0;
		const bool identity = plan.fused && m_encoding->as_identity(scale, offset);
		if (identity) {
			io.x_f32 = input;
			io.x_f32_dims = m_encoding->input_width();
			io.x_scale = scale;
			io.x_offset = offset;
		} else {
			network_input = ArenaBuf{stream, (size_t)n * enc_w * elem()};
			encoding_ctx = m_encoding->forward(stream, n, input, encoding_params(params), network_input.data(), true, false);
			io.x_half = network_input.data();
		}
		const size_t buf_bytes = (size_t)n * enc_w * elem();
		const uint32_t group = identity ? n_tangents : (uint32_t)std::min<size_t>(n_tangents, std::max<size_t>(INPUT_JACOBIAN_TMP_BYTES / std::max<size_t>(buf_bytes, 1), 1));
		if (!identity) encoded_tangents = ArenaBuf{stream, buf_bytes * group};
		for (uint32_t t0 = 0; t0 < n_tangents; t0 += group) {
			const uint32_t n_group = std::min(group, n_tangents - t0);
			MatView tangents_f32{};
			if (identity) tangents_f32 = MatView{tangents + (size_t)t0 * input_width(), n_tangents * input_width(), 1u};
			for (uint32_t t = 0; t < n_group && !identity; ++t) {
				m_encoding->tangent(stream, encoding_ctx, n, input, tangent_slice(tangents, t0 + t, n_tangents), (char*)encoded_tangents.data() + t * buf_bytes, encoding_params(params));
			}
			m_network->input_jvp(stream, plan, n, io, encoded_tangents.data(), tangents_f32, n_group, params, jvp, n_tangents, t0);
			io.out_half = nullptr; // stored with the first group
		}
		return plan.name;
	}

	// Second-order input gradients through encoding and network (the network: Network::second_order_*, CutlassMLP only).  With
	// e = encoding(x) and v = dL_ddLdinput:
	//   1. g_e = dL/de from the network's first-order backward pass on the context's activations -- the very kernels backward() runs, so
	//      that the model gives what its parts give when a caller chains them by hand -- and the network's layer-by-layer passes from e
	//   2. encoding.backward_backward_input(x, v, dL_dy = g_e) -> t = J_enc v, the encoding's second-order gradients, its part of dL_dinput
	//   3. the network's second-order pass with v := t -> dL_ddLdoutput, the network's gradients, q = dS/de
	//   4. where the network has curvature (q != 0): encoding.backward(dL_dy = q), accumulated onto the results of 2.
	// FullyFusedMLP has no second-order pass, as in the reference (ask for "otype": "CutlassMLP"), and neither have most encodings: both
	// are reported before anything is allocated or launched.
	void backward_backward_input(hipStream_t stream, const ModelContext& mctx, uint32_t n, MatView input, MatView dL_ddLdinput, const void* dL_doutput,
	                             void* dL_ddLdoutput, MatViewMut* dL_dinput, const void* params, void* gradients, GradientMode mode) override {
		if (m_network->fully_fused() || !m_encoding->has_second_order()) {
			return Model::backward_backward_input(stream, mctx, n, input, dL_ddLdinput, dL_doutput, dL_ddLdoutput, dL_dinput, params, gradients, mode);
		}
		second_order(stream, mctx, n, input, dL_ddLdinput, dL_doutput, dL_ddLdoutput, dL_dinput, params, gradients, mode);
	}
protected:
	// the route is the network's plan's (mlp_input_jvp_backward_plan).  Every class is "two-pass" today, the generic composition; a fused entry
	// has no kernel to run yet and is refused here instead of being served by another route under its name.
	std::string input_jvp_backward_impl(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, const void* dL_djvp, const void* dL_doutput,
	                                    const void* params, void* gradients, MatViewMut* dL_dinput, float* dL_dtangents, GradientMode mode) override {
		const MlpInputJvpBackwardPlan plan = m_network->input_jvp_backward_plan(n, n_tangents);
		if (plan.fused) throw std::runtime_error{std::string{"input_jvp_backward: no kernel for the plan's route "} + plan.name};
		Model::input_jvp_backward_impl(stream, n, n_tangents, input, tangents, dL_djvp, dL_doutput, params, gradients, dL_dinput, dL_dtangents, mode);
		return plan.name;
	}
	// input_jvp_backward()'s second-order pass: the passes above for any network otype -- Network::second_order_* run for a FullyFusedMLP as
	// they do for input_jvp -- and behind an encoding that has a tangent but no second-order pass (OneBlob), where step 2 is the tangent
	// alone: such an encoding has no parameters here and dL_dinput is not asked for (Model::input_jvp_backward refuses both).
	void tangent_reverse(hipStream_t stream, const ModelContext& ctx, uint32_t n, MatView input, MatView v, const void* u, MatViewMut* dL_dinput, const void* params, void* gradients,
	                     GradientMode mode) override {
		second_order(stream, ctx, n, input, v, u, nullptr, dL_dinput, params, gradients, mode);
	}
private:
	void second_order(hipStream_t stream, const ModelContext& mctx, uint32_t n, MatView input, MatView dL_ddLdinput, const void* dL_doutput,
	                  void* dL_ddLdoutput, MatViewMut* dL_dinput, const void* params, void* gradients, GradientMode mode) {
		const bool tangent_only = !m_encoding->has_second_order();
		CHECK_THROW(!tangent_only || (!dL_dinput && m_encoding->n_params() == 0));
		check_batch(n);
		const Ctx& ctx = dynamic_cast<const Ctx&>(mctx);
		if (ctx.fused || !ctx.input_gradients) throw std::runtime_error{"NetworkWithInputEncoding::backward: input gradients were not prepared by forward()"};
		const bool want_grads = mode != GradientMode::Ignore;
		if (n == 0 || (!dL_ddLdoutput && !dL_dinput && !want_grads)) return;
		CHECK_THROW(!want_grads || gradients != nullptr);
		const void* p = params;
		void* g = want_grads ? gradients : nullptr;
		const size_t enc_bytes = (size_t)n * m_encoding->padded_output_width() * elem();
		const bool enc_grads = want_grads && m_encoding->n_params() > 0;
		// q feeds the encoding's parameter gradients and dL_dinput only
		const bool want_q = m_network->any_curvature() && (enc_grads || dL_dinput);

		ArenaBuf g_e, t{stream, enc_bytes}, q;
		if (!tangent_only && m_encoding->second_order_reads_dL_dy() && (enc_grads || dL_dinput)) {
			g_e = ArenaBuf{stream, enc_bytes};
			ArenaBuf output; // backward() reads it for the output activation's derivative only
			if (m_network->has_output_activation()) {
				output = ArenaBuf{stream, (size_t)n * m_network->padded_output_width() * elem()};
				m_network->inference(stream, n, ctx.network_input.data(), output.data(), p);
			}
			m_network->backward(stream, ctx.network_ctx, n, ctx.network_input.data(), output.data(), dL_doutput, g_e.data(), p, nullptr, GradientMode::Ignore);
		}
		Network::SecondOrderPass pass = m_network->second_order_begin(stream, n, ctx.network_input.data(), dL_doutput, p, want_grads || want_q);
		if (tangent_only) m_encoding->tangent(stream, ctx.encoding_ctx, n, input, dL_ddLdinput, t.data(), encoding_params(p));
		else m_encoding->backward_backward_input(stream, ctx.encoding_ctx, n, input, dL_ddLdinput, g_e.data(), t.data(), dL_dinput, encoding_params(p), encoding_params(g), mode);
		if (want_q) q = ArenaBuf{stream, enc_bytes};
		m_network->second_order_finish(stream, pass, n, t.data(), dL_ddLdoutput, q.data(), p, g, mode);
		if (!want_q) return;
		ArenaBuf dx_more;
		MatViewMut dx_view{nullptr, m_encoding->input_width(), 1u};
		if (dL_dinput) {
			dx_more = ArenaBuf{stream, (size_t)n * m_encoding->input_width() * sizeof(float)};
			dx_view.data = dx_more.as<float>();
		}
		m_encoding->backward_rows(stream, ctx.encoding_ctx, n, input, q.data(), dL_dinput ? &dx_view : nullptr, encoding_params(p), enc_grads ? encoding_params(g) : nullptr,
		                          enc_grads ? GradientMode::Accumulate : GradientMode::Ignore);
		if (dL_dinput) add_input_gradient(stream, n, m_encoding->input_width(), MatView{dx_view.data, dx_view.stride_sample, dx_view.stride_dim}, *dL_dinput);
	}
public:

	// TCNN_AMD_FUSED_STEP=0 selects the reference-shaped kernel sequence (forward / loss / backward / wgrad) for A/B runs
	static bool use_fused_step() { return switches().fused_step; }
	bool fused_step_supported(uint32_t n) const { return use_fused_step() && !m_network->layerwise() && mlp_train_any_kernel(m_network->desc(), n); }
	// exactly when the slab reduction of a fused step is a launch of its own that finishes EVERY gradient of the model, so that it can apply
	// the optimizer's update behind it (OptimizerOffer::in_reduce): no encoding parameters, no dL/dinput asked for, gradients overwritten
	bool reduction_carries_update(bool want_dL_dinput, GradientMode mode) const { return m_encoding->n_params() == 0 && !want_dL_dinput && mode == GradientMode::Overwrite; }
	bool live_image_kept() const { return m_live_image_kept; }           // the last fused step's optimizer launch left the live image current
	void invalidate_live_image() { m_network->invalidate_live_image(); } // the parameters change(d) some other way
	size_t image_preps() const { return m_image_preps; }                 // k_mlp_prep launches of fused steps so far (a test's view of the above)
	const char* last_train_kernel() const { return m_last_train_kernel; } // short name of the MLP kernel the last fused step launched (MlpTrainPlan::name)
	uint64_t scatter_wide_fallbacks() { return m_encoding->scatter_wide_fallbacks(); }
	uint64_t list_scatters() const override { return m_encoding->list_scatters(); }
	uint64_t list_gradient_tails() const override { return m_list_gradient_tails; }
	bool context_keeps_slabs(const ModelContext& c) const { const Ctx* x = dynamic_cast<const Ctx*>(&c); return x && (bool)x->slabs_kept; }
	// the register-resident fused kernel (k_train_regs.hip) writes dL_doutput / L as compact [n][dims] matrices (TrainContext::compact)
	bool fused_compact_context_supported(uint32_t n) const {
		if (m_network->layerwise()) return false;
		const bool ok = use_fused_step() && mlp_train_compact_context(m_network->desc(), n) && m_network->padded_output_width() == 16;
		// the register-resident kernels address [n][...] matrices with 32-bit byte offsets: beyond 2^22 rows the step silently took the
		// much slower LDS-image kernel -- say so once (a caller can split the batch)
		if (!ok && use_fused_step() && n > (1u << 22) && mlp_train_compact_context(m_network->desc(), 1u << 22)) {
			static bool told = false;
			if (!told) {
				told = true;
				const std::string msg = "training_step: batches of more than 4194304 rows run the general fused MLP kernel (several times slower for this network); split the batch to stay on the fast path";
				log_message(TCNN_LOG_WARNING, msg);
				fprintf(stderr, "tcnn_amd warning: %s\n", msg.c_str());
			}
		}
		return ok;
	}

	// forward + loss + backward of a training step with the MLP part as ONE kernel (k_train.hip): same results as
	// forward() -> loss_evaluate() -> backward(), activations never leave the CU.
	std::unique_ptr<ModelContext> fused_step(hipStream_t stream, uint32_t n, MatView input, const FusedStepData& step, const OptimizerOffer& optimizer) {
		check_batch(n);
		auto ctx = std::make_unique<Ctx>();
		// Everything in order on the caller's stream.  Running the two small kernels around the MLP kernel (k_mlp_prep, k_wgrad_reduce,
		// ~5 us each, independent of the encoding kernels) on a side stream was measured and lost 13-15 us per step on every
		// workload: a cross-stream event dependency costs more here than the kernels it hides (the same happened with Adam).
		if (step.profile) step.profile->mark(stream, StepProfile::Encode, false);
		// The MLP kernel is known before the encoding runs (mlp_train_plan on the step's request): where its workgroups each produce one whole
		// work item of a grid's hit lists, the grid forms its items from those samples and the kernel's tail stores dL/dy in list order itself
		// (list_gradient_tails; TCNN_AMD_LISTGRAD_IN_MLP=0: k_grid_list_gradients as a launch of its own, items of consecutive samples).
		const Switches sw = switches(); // one copy for the whole step
		const GridForwardRoute route = m_encoding->forward_route(sw, n, true, step.dL_dinput != nullptr, step.mode != GradientMode::Ignore);
		GridItemMap item_map;
		const bool mapped = sw.listgrad_in_mlp && route.recorded == GridRecorded::HitLists && route.plane_features && // (hit lists: dL/dy will be plain level planes of that F)
		                    mlp_train_item_map(mlp_train_plan(m_network->desc(), step_request(n, step, route.plane_features, 0, true, route.plane_features, false)), item_map);
		fused_encode(stream, *ctx, n, input, step.params, route, step.dL_dinput != nullptr, step.mode != GradientMode::Ignore, sw.side_jobs, mapped ? &item_map : nullptr);
		if (step.profile) step.profile->mark(stream, StepProfile::Encode, true);
		fused_mlp_and_scatter(stream, sw, *ctx, n, input, step, optimizer);
		return ctx;
	}

	// first half of the fused step: the encoding, as level planes where the encoding can produce them
	// route: the encoding's forward_route(), asked as_planes by the caller (with its prepare_input_gradients / prepare_param_gradients)
	void fused_encode(hipStream_t stream, Ctx& ctx, uint32_t n, MatView input, const void* params, const GridForwardRoute& route, bool prepare_input_gradients, bool prepare_param_gradients,
	                  bool prep_image = false, const GridItemMap* item_map = nullptr) {
		const _Float16* p = (const _Float16*)params;
		const uint32_t n_net = (uint32_t)m_network->n_params();
		if (m_network->layerwise()) throw std::runtime_error{"NetworkWithInputEncoding::fused_encode: a layer-by-layer network has no fused training step"};
		// a OneBlob encoding is evaluated by the MLP kernels inside their input load where they can (k_mlp.hip, k_train.hip)
		if (!prepare_input_gradients && m_encoding->as_oneblob() && m_encoding->padded_output_width() == m_network->input_width() &&
		    mlp_train_oneblob_in_kernel(m_network->desc(), n, m_encoding->as_oneblob())) {
			ctx.oneblob_bins = m_encoding->as_oneblob();
			ctx.fused = true;
			return;
		}
		ctx.network_input = ArenaBuf{stream, (size_t)n * m_encoding->padded_output_width() * 2};
		// grids hand the encoded batch over as level planes (XCD-aware forward kernel, scatter filter produced on the way)
		ForwardPlan plan{route, nullptr, item_map};
		MlpPrepJob job;
		if (route.plane_features && prep_image) { // the forward kernel also builds the network's fragment images (k_mlp_prep as a side job)
			ctx.image = ArenaBuf{stream, mlp_image_bytes(m_network->desc())};
			job.desc = m_network->desc();
			job.params = params;
			job.image = ctx.image.data();
			plan.prep_job = &job;
		}
		ctx.encoding_ctx = m_encoding->forward(stream, n, input, p + n_net, ctx.network_input.data(), prepare_input_gradients, prepare_param_gradients, &plan);
		ctx.fused = true;
	}

	// what a fused step asks of the MLP kernel (mlp_train_plan)
	MlpTrainRequest step_request(uint32_t n, const FusedStepData& step, uint32_t x_plane_f, uint32_t oneblob_bins, bool need_dx, uint32_t plane_f, bool records) const {
		MlpTrainRequest request;
		request.n = n;
		request.x_plane_features = x_plane_f;
		request.oneblob_bins = oneblob_bins;
		request.oneblob_dims = oneblob_bins ? m_encoding->input_width() : 0u;
		request.dims = m_network->output_width();
		request.loss = step.loss;
		request.external_dL_dy = step.external_dL_dy != nullptr;
		request.data_pdf = step.data_pdf != nullptr;
		request.out = step.out != nullptr;
		request.dL_dx = need_dx;
		request.dx_plane_features = plane_f;
		request.dx_record_dims = records ? m_encoding->input_width() : 0u;
		request.gradients = step.mode != GradientMode::Ignore;
		request.compact_context = step.compact_context;
		return request;
	}

	// second half: ONE MLP kernel (forward recomputed in registers, loss or external dL/doutput, backward, weight gradients),
	// the slab reduction and the encoding's backward pass.
	void fused_mlp_and_scatter(hipStream_t stream, const Switches& sw, const Ctx& ctx, uint32_t n, MatView input, const FusedStepData& step, const OptimizerOffer& optimizer) {
		const void* params = step.params;
		MatViewMut* dL_dinput = step.dL_dinput;
		const GradientMode mode = step.mode;
		StepProfile* profile = step.profile;
		const _Float16* p = (const _Float16*)params;
		_Float16* g = (_Float16*)step.gradients;
		const uint32_t n_net = (uint32_t)m_network->n_params();
		const bool need_dx = m_encoding->n_params() > 0 || dL_dinput;
		ArenaBuf dL_dnetwork_input;
		// how the encoding's backward pass will run, and with it the form the MLP kernel writes dL/d(encoding) in: asked once, here
		const GridBackwardRoute route = need_dx ? m_encoding->backward_route(sw, stream, ctx.encoding_ctx, n, input, GridDyForm::Records, dL_dinput != nullptr, mode) : GridBackwardRoute{};
		const bool records = route.dy == GridDyForm::Records;
		if (need_dx) dL_dnetwork_input = ArenaBuf{stream, records ? (size_t)n * route.record_planes * 16 : (size_t)n * m_encoding->padded_output_width() * 2};

		const MlpDesc& d = m_network->desc();
		// a model whose only parameters are the network's: the optimizer's update rides on the slab reduction (k_wgrad_reduce_adam), which
		// then also keeps the network's live image current (Network::live_image)
		const bool with_adam = optimizer.in_reduce != nullptr;
		CHECK_THROW(!with_adam || reduction_carries_update(dL_dinput != nullptr, mode)); // the caller's decision binds
		Network::LiveImage* live = with_adam && !ctx.image && sw.live_image ? m_network->live_image() : nullptr;
		m_live_image_kept = false;
		ArenaBuf prepared;
		const void* image_data;
		if (ctx.image) image_data = ctx.image.data();
		else if (live) {
			if (live->params != params) { // first step, or the parameters were changed behind the image's back
				mlp_prepare_weights(stream, d, params, live->image.data(), true);
				++m_image_preps;
			}
			image_data = live->image.data();
		} else {
			prepared = m_network->prepare(stream, params, true);
			++m_image_preps;
			image_data = prepared.data();
		}
		// which kernel, and over how many workgroups: decided once, here (mlp_train_plan); each workgroup writes one weight-gradient slab
		const MlpTrainRequest request = step_request(n, step, ctx.encoding_ctx.route.plane_features, ctx.oneblob_bins, need_dx, route.plane_features, records);
		const MlpTrainPlan plan = mlp_train_plan(d, request);
		if (!plan.ok) throw std::runtime_error{"NetworkWithInputEncoding: no fused training kernel for this network, batch and set of options"};
		CHECK_THROW(g != nullptr || !request.gradients);
		const uint32_t n_slabs = request.gradients ? plan.grid : 0u;
		ArenaBuf slabs;
		if (n_slabs) slabs = ArenaBuf{stream, (size_t)n_slabs * n_net * sizeof(float)};
		MlpTrainArgs args;
		args.image = image_data;
		args.x = ctx.network_input.data();
		if (ctx.oneblob_bins) args.oneblob_x = input;
		args.target = step.target, args.data_pdf = step.data_pdf, args.external_dL_dy = step.external_dL_dy;
		args.loss_scale = step.loss_scale;
		args.out = step.out, args.dL_dout = step.dL_dout, args.L = step.L;
		args.dL_dx = dL_dnetwork_input.data();
		args.dx_record_x = records ? input.data : nullptr;
		args.slabs = slabs.as<float>();
		args.n_params = n_net;
		// the kernel's tail stores dL/dy in the order of the grid's hit lists where the forward pass formed its items from this plan's workgroups
		GridListTail list_tail = route.list_tail;
		ArenaBuf list_gradients;
		GridItemMap item_map;
		if (route.tail && mlp_train_item_map(plan, item_map) && item_map == list_tail.map) {
			list_gradients = ArenaBuf{stream, route.tail_bytes};
			list_tail.gvals = list_gradients.data();
			args.list_tail = &list_tail;
			++m_list_gradient_tails;
		}
		if (profile) profile->mark(stream, StepProfile::MlpKernel, false);
		mlp_train_launch(stream, d, plan, args);
		m_last_train_kernel = plan.name;
		if (profile) profile->mark(stream, StepProfile::MlpKernel, true);
		// (Carrying the slab reduction on the grid scatter's launch the way k_mlp_prep rides on the forward kernel was built and
		// measured: its workgroups each take a whole CU's LDS slot for a few microseconds, in front of the task list they delay the
		// long coarse-level tasks, behind it they wait for a slot -- the scatter grew by 5.4 / 6.5 us for the 4.4 us launch saved.)
		// The slab reduction rides on the scatter's finalize launch when the encoding's backward pass has one (two ~4.5 us launches
		// become one); otherwise, or with TCNN_AMD_SIDE_JOBS=0, it is a launch of its own.
		MlpReduceJob reduce_job;
		BackwardHandoff offer; // to the encoding's backward pass
		offer.prologue = optimizer.prologue;
		offer.list_gradients = list_gradients.data();
		if (mode != GradientMode::Ignore) {
			reduce_job.n_elems = n_net;
			reduce_job.n_slabs = n_slabs;
			reduce_job.slabs = slabs.as<float>();
			reduce_job.grad = g;
			reduce_job.accumulate = mode == GradientMode::Accumulate ? 1 : 0;
			if (!(need_dx && sw.side_jobs)) {
				AdamInReduce adam_here;
				if (with_adam) {
					adam_here = *optimizer.in_reduce;
					if (live) {
						adam_here.image = live->image.data();
						adam_here.image_inv = live->inverse.as<uint32_t>();
					}
				}
				mlp_reduce_slabs(stream, n_net, n_slabs, slabs.as<float>(), g, mode == GradientMode::Accumulate, with_adam ? &adam_here : nullptr);
				if (live) {
					live->params = params; // current again once this launch has run
					m_live_image_kept = true;
				}
			} else offer.reduce_job = &reduce_job;
		}
		if (need_dx) {
			if (profile) profile->mark(stream, StepProfile::EncodingBackward, false);
			m_encoding->backward(stream, ctx.encoding_ctx, n, input, dL_dnetwork_input.data(), dL_dinput, p + n_net, g ? g + n_net : nullptr, mode, route, &offer);
			if (offer.reduce_job) {
				if (!offer.reduce_carried) mlp_reduce_slabs(stream, n_net, n_slabs, slabs.as<float>(), g, mode == GradientMode::Accumulate);
				else if (offer.prologue && offer.prologue->pending && offer.prologue->has_reduce) ctx.slabs_kept = std::move(slabs); // read by the optimizer's launch
			}
			if (profile) profile->mark(stream, StepProfile::EncodingBackward, true);
		}
	}

	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "NetworkWithInputEncoding";
		j["encoding"] = m_encoding->hyperparams();
		j["network"] = m_network->hyperparams();
		return j;
	}

private:
	size_t elem() const { return m_network->element_size(); } // bytes of a parameter, an encoded feature, an output, a gradient
	// the encoding's part of a parameter or gradient vector of the module (the network's comes first); null stays null
	const void* encoding_params(const void* params) const { return params ? (const char*)params + m_network->n_params() * elem() : nullptr; }
	void* encoding_params(void* params) const { return params ? (char*)params + m_network->n_params() * elem() : nullptr; }

	bool m_live_image_kept = false;
	size_t m_image_preps = 0;
	uint64_t m_list_gradient_tails = 0;
	const char* m_last_train_kernel = "";
	std::unique_ptr<Encoding> m_encoding;
	std::unique_ptr<Network> m_network;
};

// standalone encoding as a Module (cpp_api.cu:156-165: alignment 0 -> no padding)
class EncodingModel : public Model {
public:
	EncodingModel(uint32_t n_dims_to_encode, const Json& encoding, Precision precision) : m_precision{precision} {
		m_encoding = create_encoding(n_dims_to_encode, encoding, 0, precision == Precision::Fp32);
	}
	uint32_t input_width() const override { return m_encoding->input_width(); }
	uint32_t output_width() const override { return m_encoding->padded_output_width(); }
	uint32_t padded_output_width() const override { return m_encoding->padded_output_width(); }
	size_t n_params() const override { return m_encoding->n_params(); }
	Precision precision() const override { return m_precision; }
	std::vector<std::pair<uint32_t, uint32_t>> layer_sizes() const override { return {}; }
	void initialize_params(Pcg32& rng, float* params_full_precision, float scale) override { m_encoding->initialize_params(rng, params_full_precision, scale); }
	uint64_t list_scatters() const override { return m_encoding->list_scatters(); }
	Encoding* input_encoding() override { return m_encoding.get(); }

	struct Ctx : public ModelContext {
		EncodingContext encoding_ctx;
	};
	void inference(hipStream_t stream, uint32_t n, MatView input, void* output, const void* params) override {
		check_batch(n);
		m_encoding->forward(stream, n, input, params, output, false, false);
	}
	std::unique_ptr<ModelContext> forward(hipStream_t stream, uint32_t n, MatView input, void* output, const void* params, bool prepare_input_gradients) override {
		check_batch(n);
		auto ctx = std::make_unique<Ctx>();
		ctx->encoding_ctx = m_encoding->forward(stream, n, input, params, output, prepare_input_gradients, true);
		return ctx;
	}
	void backward(hipStream_t stream, const ModelContext& mctx, uint32_t n, MatView input, const void* output, const void* dL_doutput,
	              MatViewMut* dL_dinput, const void* params, void* gradients, GradientMode mode) override {
		check_batch(n);
		const Ctx& ctx = dynamic_cast<const Ctx&>(mctx);
		m_encoding->backward_rows(stream, ctx.encoding_ctx, n, input, dL_doutput, dL_dinput, params, gradients, mode);
	}
	void backward_backward_input(hipStream_t stream, const ModelContext& mctx, uint32_t n, MatView input, MatView dL_ddLdinput, const void* dL_doutput,
	                             void* dL_ddLdoutput, MatViewMut* dL_dinput, const void* params, void* gradients, GradientMode mode) override {
		check_batch(n);
		const Ctx& ctx = dynamic_cast<const Ctx&>(mctx);
		m_encoding->backward_backward_input(stream, ctx.encoding_ctx, n, input, dL_ddLdinput, dL_doutput, dL_ddLdoutput, dL_dinput, params, gradients, mode);
	}
	bool has_tangent() const override { return m_encoding->has_tangent(); }
	Json hyperparams() const override { return m_encoding->hyperparams(); }
protected:
	void tangent(hipStream_t stream, const ModelContext& mctx, uint32_t n, MatView input, MatView v, void* t, const void* params) override {
		const Ctx& ctx = dynamic_cast<const Ctx&>(mctx);
		m_encoding->tangent(stream, ctx.encoding_ctx, n, input, v, t, params);
	}
	// (an encoding with a tangent but no second-order pass -- OneBlob -- has no parameters and is not asked for dL_dinput: nothing to do)
	void tangent_reverse(hipStream_t stream, const ModelContext& ctx, uint32_t n, MatView input, MatView v, const void* u, MatViewMut* dL_dinput, const void* params, void* gradients,
	                     GradientMode mode) override {
		if (m_encoding->has_second_order()) Model::tangent_reverse(stream, ctx, n, input, v, u, dL_dinput, params, gradients, mode);
	}
private:
	Precision m_precision;
	std::unique_ptr<Encoding> m_encoding;
};

// ------------------------------------------------------------------------------------------------------------------
// Loss (src/loss.cu:85-93) and Adam (optimizers/adam.h:122-327, src/optimizer.cu:50-82)
// ------------------------------------------------------------------------------------------------------------------
inline LossType create_loss(const Json& loss) {
	const std::string otype = loss.value("otype", "RelativeL2");
	static const std::pair<const char*, LossType> table[] = { // src/loss.cu:57-65
		{"L2", LossType::L2}, {"RelativeL2", LossType::RelativeL2}, {"RelativeL2Luminance", LossType::RelativeL2Luminance}, {"L1", LossType::L1},
		{"RelativeL1", LossType::RelativeL1}, {"Mape", LossType::Mape}, {"Smape", LossType::Smape}, {"CrossEntropy", LossType::CrossEntropy}, {"Variance", LossType::Variance}};
	for (const auto& kv : table) if (equals_case_insensitive(otype, kv.first)) return kv.second;
	throw std::runtime_error{"Invalid loss type: " + otype};
}
inline const char* to_string(LossType t) {
	static const char* names[] = {"L2", "RelativeL2", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance", "RelativeL2Luminance"};
	return names[(uint32_t)t];
}
// Loss<T>::evaluate (loss.h:41-60) on predictions that are the caller's (tcnn_loss_evaluate): everything is checked here, before anything
// touches the device; the partials of the sum come from the arena, so a call allocates nothing once warm and never synchronises.
inline void loss_evaluate_on_predictions(hipStream_t stream, int type, int precision, float loss_scale, const float* scale_dev, uint32_t n, uint32_t dims,
                                         const void* prediction, uint32_t prediction_stride, const float* target, const float* data_pdf,
                                         float* values, uint32_t values_stride, void* gradients, uint32_t gradients_stride, float* loss_sum) {
	const std::string who = "tcnn_loss_evaluate: ";
	if (type < 0 || type > (int)LossType::RelativeL2Luminance) throw std::runtime_error{who + "Invalid loss type: " + std::to_string(type)};
	if (precision != (int)Precision::Fp32 && precision != (int)Precision::Fp16) throw std::runtime_error{who + "Unknown precision " + std::to_string(precision)};
	if (!values && !gradients && !loss_sum) throw std::runtime_error{who + "no output requested (values, gradients and loss_sum are all NULL)"};
	if (dims < 1) throw std::runtime_error{who + "dims must be at least 1"};
	if ((LossType)type == LossType::RelativeL2Luminance && dims < 3) throw std::runtime_error{who + "RelativeL2Luminance reads three channels per row and needs dims >= 3, got " + std::to_string(dims)};
	uint32_t max_stride = prediction_stride;
	const auto check_stride = [&](const char* name, uint32_t stride) {
		if (stride < dims) throw std::runtime_error{who + "the " + name + " stride " + std::to_string(stride) + " is smaller than dims " + std::to_string(dims)};
		max_stride = std::max(max_stride, stride);
	};
	check_stride("prediction", prediction_stride);
	if (values) check_stride("values", values_stride);
	if (gradients) check_stride("gradients", gradients_stride);
	if ((uint64_t)n * max_stride >= (1ull << 32)) throw std::runtime_error{who + "n * stride must be below 2^32"};
	if (n == 0) { // nothing to launch; the sum of no values
		if (loss_sum) HIP_CHECK_THROW(hipMemsetAsync(loss_sum, 0, sizeof(float), stream));
		return;
	}
	if (!prediction || !target) throw std::runtime_error{who + "prediction and target must not be NULL"};
	LossEvalRequest r;
	r.type = (LossType)type;
	r.precision = (Precision)precision;
	r.n = n;
	r.dims = dims;
	r.loss_scale = loss_scale;
	r.scale_dev = scale_dev;
	r.prediction = prediction;
	r.prediction_stride = prediction_stride;
	r.target = target;
	r.data_pdf = data_pdf;
	r.values = values;
	r.values_stride = values_stride;
	r.gradients = gradients;
	r.gradients_stride = gradients_stride;
	r.loss_sum = loss_sum;
	ArenaBuf partials; // returned to the stream's free list when this call ends: the stream orders its reuse
	if (loss_sum) {
		partials = ArenaBuf{stream, LOSS_EVAL_MAX_BLOCKS * sizeof(float)};
		r.partials = partials.as<float>();
	}
	loss_eval_launch(stream, r);
	HIP_CHECK_THROW(hipGetLastError());
}

// the fused training kernel evaluates these two inside its loss stage; the others go forward -> k_loss -> backward
inline bool loss_in_fused_kernel(LossType t) { return t == LossType::L2 || t == LossType::RelativeL2; }

// snapshot helpers (gpu_memory_json.h:36-71): device memory <-> json binary value
inline Json device_to_binary(const void* device, size_t n_bytes) {
	std::vector<uint8_t> host(n_bytes);
	if (n_bytes) HIP_CHECK_THROW(hipMemcpy(host.data(), device, n_bytes, hipMemcpyDeviceToHost));
	return Json::binary(std::move(host));
}
// binary value, or nlohmann's text form of one: {"bytes": [...], "subtype": null} (gpu_memory_json.h:55-67)
inline std::vector<uint8_t> binary_of(const Json& j) {
	if (j.is_binary()) return j.get_binary();
	if (j.is_object()) {
		const Json& arr = j["bytes"];
		std::vector<uint8_t> bytes(arr.size());
		for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = (uint8_t)arr.at(i).as_double();
		return bytes;
	}
	throw std::runtime_error{"Invalid json type: must be either binary or object"};
}

// optimizer.h:44-95
class Optimizer {
public:
	virtual ~Optimizer() {}
	virtual void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) = 0;
	// Weight precision Fp32 (Optimizer<float> of the reference's build without TCNN_HALF_PRECISION): ONE float weight vector -- the master
	// vector is the working vector -- fp32 gradients, and float custom weights.  Chosen before the state is allocated; nested optimizers follow.
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes, Precision weight_precision) {
		set_weight_precision(weight_precision);
		allocate(n_weights, layer_sizes);
	}
	virtual void set_weight_precision(Precision p) { m_weight_precision = p; }
	Precision weight_precision() const { return m_weight_precision; }
	bool fp32_weights() const { return m_weight_precision == Precision::Fp32; }
	size_t weight_bytes() const { return fp32_weights() ? sizeof(float) : 2; } // of one working / custom weight
	// gradients: n_weights values in `precision` -- the trainer's half gradients (scaled by loss_scale), or fp32 ones a caller computed itself
	// (a PyTorch parameter's .grad; loss_scale 1 when they are unscaled already).  The weights stay what they are: fp32 master, half working copy.
	// With fp32 weights: `weights` is null or weights_full_precision itself, and the gradients are fp32.
	virtual void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) = 0;
	// step() with the backward pass's finalize pass as the prologue of the same launch (AdamPrologue).  takes_prologue(): this optimizer
	// can; step_with_prologue returns false when this prologue's shapes do not fit -- nothing has happened then, the caller runs the
	// finalize pass and step() itself.
	virtual bool takes_prologue() const { return false; }
	// The step applied by the reduction of the weight gradients (AdamInReduce).  can_step_in_reduce(): this optimizer can;
	// begin_step_in_reduce starts a step and describes it for the launch that will apply it to EVERY parameter: that launch then equals
	// step() bit for bit, and nothing more is to be launched for this step.
	virtual bool can_step_in_reduce() const { return false; }
	virtual AdamInReduce begin_step_in_reduce(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights) {
		throw std::runtime_error{"Optimizer: this optimizer's step cannot be applied by the slab reduction"};
	}
	virtual bool step_with_prologue(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, void* gradients, const AdamPrologue& prologue) { return false; }
	virtual float learning_rate() const = 0;
	virtual void set_learning_rate(float val) = 0;
	virtual uint32_t step_count() const = 0;
	virtual size_t n_weights() const = 0;
	virtual void* custom_weights() const { return nullptr; } // half weights the trainer uses for inference instead of its own (EMA)
	virtual void update_hyperparams(const Json& params) = 0;
	virtual Json hyperparams() const = 0;
	virtual Json serialize() const = 0;
	virtual void deserialize(const Json& data, size_t n_weights) = 0;
	// after a snapshot was loaded into `weights`: optimizers that assemble custom weights from several sources rebuild them
	virtual void weights_restored(hipStream_t stream, const void* weights) {}
protected:
	// every step() starts here: an fp32-weight optimizer has no second weight vector and reads no half gradients.  Returns the working
	// weights (the master vector itself with fp32 weights).
	void* checked_weights(float* weights_full_precision, void* weights, GradientPrecision precision) const {
		if (!fp32_weights()) return weights;
		if (weights != nullptr && weights != (void*)weights_full_precision) throw std::runtime_error{"Optimizer: with fp32 weights there is one weight vector (weights must be null or weights_full_precision)."};
		if (precision != GradientPrecision::Fp32) throw std::runtime_error{"Optimizer: with fp32 weights the gradients must be fp32."};
		return weights_full_precision;
	}
	Precision m_weight_precision = Precision::Fp16;
};
inline std::unique_ptr<Optimizer> create_optimizer(const Json& params);

class AdamOptimizer : public Optimizer {
public:
	explicit AdamOptimizer(const Json& params) { update_hyperparams(params); }
	float learning_rate() const override { return m_h.learning_rate; }
	void set_learning_rate(float val) override { m_h.learning_rate = val; }
	size_t n_weights() const override { return m_n_weights; }

	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) override { // adam.h:128-148
		m_n_weights = n_weights;
		if (n_weights * sizeof(float) > m_first_moments.bytes()) {
			m_first_moments.resize(n_weights * sizeof(float));
			m_second_moments.resize(n_weights * sizeof(float));
		}
		m_steps16 = narrow_steps_enabled();
		m_param_steps.resize(0);
		m_param_steps.resize(n_weights * step_bytes());
		m_first_moments.memset(0);
		m_second_moments.memset(0);
		m_param_steps.memset(0);
		m_n_matrix = 0;
		for (const auto& ls : layer_sizes) m_n_matrix += (size_t)ls.first * ls.second;
	}

	// adam.h:278-299
	Json serialize() const override {
		auto blob = [](const DeviceBuf& buf, size_t n_bytes) { return device_to_binary(buf.data(), n_bytes); };
		Json data = Json::object();
		data["current_step"] = Json((uint32_t)m_current_step);
		data["base_learning_rate"] = Json((float)m_h.learning_rate);
		data["first_moments_binary"] = blob(m_first_moments, m_n_weights * sizeof(float));
		data["second_moments_binary"] = blob(m_second_moments, m_n_weights * sizeof(float));
		if (m_steps16) { // the snapshot carries uint32 counts whatever is kept here
			std::vector<uint16_t> narrow(m_n_weights);
			if (m_n_weights) HIP_CHECK_THROW(hipMemcpy(narrow.data(), m_param_steps.data(), m_n_weights * sizeof(uint16_t), hipMemcpyDeviceToHost));
			std::vector<uint8_t> wide(m_n_weights * sizeof(uint32_t));
			for (size_t i = 0; i < m_n_weights; ++i) {
				const uint32_t v = narrow[i];
				std::memcpy(wide.data() + 4 * i, &v, 4);
			}
			data["param_steps_binary"] = Json::binary(std::move(wide));
		} else {
			data["param_steps_binary"] = blob(m_param_steps, m_n_weights * sizeof(uint32_t));
		}
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		auto load = [&](DeviceBuf& buf, const std::vector<uint8_t>& bytes, size_t elem) {
			if (bytes.size() != n_weights * elem) throw std::runtime_error{"Adam: snapshot state has the wrong size."};
			buf.resize(bytes.size());
			if (!bytes.empty()) HIP_CHECK_THROW(hipMemcpy(buf.data(), bytes.data(), bytes.size(), hipMemcpyHostToDevice));
		};
		m_n_weights = n_weights;
		load(m_first_moments, binary_of(data["first_moments_binary"]), sizeof(float));
		load(m_second_moments, binary_of(data["second_moments_binary"]), sizeof(float));
		m_current_step = (uint32_t)data["current_step"].as_double();
		m_steps16 = narrow_steps_enabled() && m_current_step < NARROW_STEP_LIMIT;
		if (data.contains("param_steps_binary")) {
			const std::vector<uint8_t>& bytes = binary_of(data["param_steps_binary"]);
			if (bytes.size() != n_weights * sizeof(uint32_t)) throw std::runtime_error{"Adam: snapshot state has the wrong size."};
			std::vector<uint16_t> narrow(m_steps16 ? n_weights : 0);
			for (size_t i = 0; m_steps16 && i < n_weights; ++i) {
				uint32_t v;
				std::memcpy(&v, bytes.data() + 4 * i, 4);
				if (v >= NARROW_STEP_LIMIT) m_steps16 = false; // a count the narrow form cannot hold (a foreign snapshot): keep all 32 bits
				else narrow[i] = (uint16_t)v;
			}
			m_param_steps.resize(0);
			m_param_steps.resize(n_weights * step_bytes());
			if (n_weights) HIP_CHECK_THROW(hipMemcpy(m_param_steps.data(), m_steps16 ? (const void*)narrow.data() : (const void*)bytes.data(), n_weights * step_bytes(), hipMemcpyHostToDevice));
		} else {
			m_param_steps.resize(0);
			m_param_steps.resize(n_weights * step_bytes());
			m_param_steps.memset(0);
		}
		m_h.learning_rate = (float)data["base_learning_rate"].as_double();
	}

	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override { // adam.h:150-188
		weights = checked_weights(weights_full_precision, weights, precision);
		++m_current_step;
		ensure_debias_table(stream);
		ensure_step_width(stream);
		adam_step(stream, m_h, m_n_weights, m_n_matrix, loss_scale, m_current_step, weights_full_precision, weights, gradients,
		          m_first_moments.as<float>(), m_second_moments.as<float>(), m_param_steps.data(), m_steps16, m_debias.as<float>(), precision, m_weight_precision);
	}

	// (the prologue and the in-reduce form finish half gradients and store a half working copy: not with fp32 weights)
	bool takes_prologue() const override { return !fp32_weights(); }
	bool step_with_prologue(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, void* gradients, const AdamPrologue& prologue) override {
		if (fp32_weights() || switches().adam_prologue_refused) return false; // (tests: the caller's path for a prologue this launch does not take)
		++m_current_step;
		ensure_debias_table(stream);
		ensure_step_width(stream);
		if (adam_step_with_prologue(stream, m_h, m_n_weights, m_n_matrix, loss_scale, m_current_step, weights_full_precision, weights, gradients, m_first_moments.as<float>(),
		                            m_second_moments.as<float>(), m_param_steps.data(), m_steps16, m_debias.as<float>(), prologue)) return true;
		--m_current_step; // (the table and the width of the counts are as step() wants them; it counts the step itself)
		return false;
	}

	// The per-parameter update counts (this fork's adam.h:66-99: a parameter whose gradient is zero in a step is skipped, so it has
	// a count of its own) are 4 of the 18 bytes per parameter a step reads and 4 of the 18 it writes.  No count exceeds the
	// optimizer's own step count, so while that is below 2^16 - 1 the counts are kept as uint16 -- 34 -> 32 bytes moved per parameter
	// by the HBM-bound kernel -- and widened in place of one step's time before one could overflow; snapshots carry uint32 either
	// way.  TCNN_AMD_ADAM_STEPS32=1: uint32 from the start (A/B runs, tests).
	static constexpr uint32_t NARROW_STEP_LIMIT = 65535;
	static bool narrow_steps_enabled() { return !switches().adam_steps32; }
	size_t step_bytes() const { return m_steps16 ? sizeof(uint16_t) : sizeof(uint32_t); }
	void ensure_step_width(hipStream_t stream) { // call with m_current_step = the step about to be applied
		if (!m_steps16 || m_current_step < NARROW_STEP_LIMIT) return;
		DeviceBuf wide;
		wide.resize(m_n_weights * sizeof(uint32_t));
		adam_widen_steps(stream, m_n_weights, m_param_steps.data(), wide.data());
		HIP_CHECK_THROW(hipStreamSynchronize(stream)); // once in 65 535 steps: the narrow array is freed right after
		m_param_steps = std::move(wide);
		m_steps16 = false;
	}

	bool can_step_in_reduce() const override { return !fp32_weights(); } // (k_wgrad_reduce_adam)
	AdamInReduce begin_step_in_reduce(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights) override {
		if (fp32_weights()) return Optimizer::begin_step_in_reduce(stream, loss_scale, weights_full_precision, weights);
		++m_current_step;
		ensure_debias_table(stream);
		ensure_step_width(stream);
		AdamInReduce out;
		out.args = make_adam_args(m_h, loss_scale, m_current_step);
		out.w_fp = weights_full_precision;
		out.w_half = weights;
		out.m1 = m_first_moments.as<float>();
		out.m2 = m_second_moments.as<float>();
		out.steps = m_param_steps.data();
		out.steps16 = m_steps16 ? 1u : 0u;
		out.debias_table = m_debias.as<float>();
		return out;
	}

	// debias factors for steps [0, m_debias_filled), computed ahead in blocks of 4096 steps; refilled when the betas change
	void ensure_debias_table(hipStream_t stream) {
		const bool stale = m_debias_beta1 != m_h.beta1 || m_debias_beta2 != m_h.beta2;
		if (!stale && m_current_step < m_debias_filled) return;
		const uint32_t want = next_multiple(m_current_step + 1, 4096u) + 4096u;
		if ((size_t)want * sizeof(float) > m_debias.bytes()) {
			HIP_CHECK_THROW(hipStreamSynchronize(stream)); // the old table may still be in use
			m_debias.resize((size_t)want * 2 * sizeof(float));
			m_debias_filled = 0;
		}
		const uint32_t from = stale ? 0u : m_debias_filled;
		adam_fill_debias_table(stream, m_h.beta1, m_h.beta2, from, want, m_debias.as<float>());
		m_debias_filled = want;
		m_debias_beta1 = m_h.beta1;
		m_debias_beta2 = m_h.beta2;
	}

	void update_hyperparams(const Json& p) override { // adam.h:210-258
		if (!p.is_object()) return;
		if (p.contains("beta1")) m_h.beta1 = (float)p["beta1"].as_double();
		if (p.contains("beta2")) m_h.beta2 = (float)p["beta2"].as_double();
		if (p.contains("epsilon")) m_h.epsilon = (float)p["epsilon"].as_double();
		if (p.contains("learning_rate")) m_h.learning_rate = (float)p["learning_rate"].as_double();
		if (p.contains("l2_reg")) m_h.l2_reg = (float)p["l2_reg"].as_double();
		if (p.contains("adabound")) m_h.adabound = p["adabound"].as_bool();
		if (p.contains("relative_decay")) m_h.relative_decay = (float)p["relative_decay"].as_double();
		if (p.contains("absolute_decay")) m_h.absolute_decay = (float)p["absolute_decay"].as_double();
		if (p.contains("clipping_magnitude")) m_h.clipping_magnitude = (float)p["clipping_magnitude"].as_double();
		if (p.contains("non_matrix_learning_rate_factor")) m_h.non_matrix_learning_rate_factor = (float)p["non_matrix_learning_rate_factor"].as_double();
		if (p.contains("optimize_matrix_params")) m_h.optimize_matrix_params = p["optimize_matrix_params"].as_bool();
		if (p.contains("optimize_non_matrix_params")) m_h.optimize_non_matrix_params = p["optimize_non_matrix_params"].as_bool();
	}

	Json hyperparams() const override { // adam.h:260-276
		Json j = Json::object();
		j["otype"] = "Adam";
		j["beta1"] = m_h.beta1;
		j["beta2"] = m_h.beta2;
		j["epsilon"] = m_h.epsilon;
		j["learning_rate"] = m_h.learning_rate;
		j["l2_reg"] = m_h.l2_reg;
		j["adabound"] = m_h.adabound;
		j["relative_decay"] = m_h.relative_decay;
		j["absolute_decay"] = m_h.absolute_decay;
		j["clipping_magnitude"] = m_h.clipping_magnitude;
		j["non_matrix_learning_rate_factor"] = m_h.non_matrix_learning_rate_factor;
		j["optimize_matrix_params"] = m_h.optimize_matrix_params;
		j["optimize_non_matrix_params"] = m_h.optimize_non_matrix_params;
		return j;
	}

	uint32_t step_count() const override { return m_current_step; }
	const AdamHyper& hyper() const { return m_h; }
	float* first_moments() const { return m_first_moments.as<float>(); }
	float* second_moments() const { return m_second_moments.as<float>(); }
	size_t n_matrix() const { return m_n_matrix; }

private:
	AdamHyper m_h;
	size_t m_n_weights = 0, m_n_matrix = 0;
	DeviceBuf m_first_moments, m_second_moments, m_param_steps, m_debias;
	uint32_t m_debias_filled = 0;
	float m_debias_beta1 = -1.0f, m_debias_beta2 = -1.0f;
	uint32_t m_current_step = 0;
	bool m_steps16 = true; // width of m_param_steps, see ensure_step_width
};

// optimizers/sgd.h:44-150
class SgdOptimizer : public Optimizer {
public:
	explicit SgdOptimizer(const Json& params) { update_hyperparams(params); }
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>&) override { m_n_weights = n_weights; }
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override {
		weights = checked_weights(weights_full_precision, weights, precision);
		++m_current_step;
		sgd_step(stream, m_n_weights, loss_scale, m_learning_rate, m_l2_reg, weights_full_precision, weights, gradients, precision, m_weight_precision);
	}
	float learning_rate() const override { return m_learning_rate; }
	void set_learning_rate(float val) override { m_learning_rate = val; }
	uint32_t step_count() const override { return m_current_step; }
	size_t n_weights() const override { return m_n_weights; }
	void update_hyperparams(const Json& p) override {
		if (!p.is_object()) return;
		if (p.contains("learning_rate")) m_learning_rate = (float)p["learning_rate"].as_double();
		if (p.contains("l2_reg")) m_l2_reg = (float)p["l2_reg"].as_double();
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "SGD";
		j["learning_rate"] = m_learning_rate;
		j["l2_reg"] = m_l2_reg;
		return j;
	}
	Json serialize() const override {
		Json data = Json::object();
		data["current_step"] = Json((uint32_t)m_current_step);
		data["learning_rate"] = Json(m_learning_rate);
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		m_n_weights = n_weights;
		m_current_step = (uint32_t)data["current_step"].as_double();
		m_learning_rate = (float)data["learning_rate"].as_double();
	}
private:
	size_t m_n_weights = 0;
	uint32_t m_current_step = 0;
	float m_learning_rate = 1e-3f, m_l2_reg = 1e-8f; // sgd.h:151-152
};

// optimizers/exponential_decay.h:45-160: scales the nested optimizer's learning rate by decay_base every decay_interval steps
class ExponentialDecayOptimizer : public Optimizer {
public:
	explicit ExponentialDecayOptimizer(const Json& params) {
		m_nested = create_optimizer(params.value("nested", Json::object()));
		update_hyperparams(params);
		m_learning_rate_factor = 1.0f;
		m_base_learning_rate = m_nested->learning_rate();
	}
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) override { m_nested->allocate(n_weights, layer_sizes); }
	void set_weight_precision(Precision p) override { m_weight_precision = p; m_nested->set_weight_precision(p); }
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override { // :60-71
		weights = checked_weights(weights_full_precision, weights, precision);
		if (step_count() == 0) m_learning_rate_factor = 1.0f;
		if (step_count() >= m_decay_start && (step_count() - m_decay_start) % m_decay_interval == 0 && step_count() <= m_decay_end) m_learning_rate_factor *= m_decay_base;
		m_nested->set_learning_rate(m_base_learning_rate * m_learning_rate_factor);
		m_nested->step(stream, loss_scale, weights_full_precision, weights, gradients, precision);
	}
	float learning_rate() const override { return m_base_learning_rate * m_learning_rate_factor; }
	void set_learning_rate(float val) override {
		m_base_learning_rate = val / m_learning_rate_factor;
		m_nested->set_learning_rate(m_base_learning_rate * m_learning_rate_factor);
	}
	uint32_t step_count() const override { return m_nested->step_count(); }
	size_t n_weights() const override { return m_nested->n_weights(); }
	void* custom_weights() const override { return m_nested->custom_weights(); }
	void update_hyperparams(const Json& p) override {
		if (!p.is_object()) return;
		if (p.contains("decay_base")) m_decay_base = (float)p["decay_base"].as_double();
		if (p.contains("decay_interval")) m_decay_interval = std::max(1u, (uint32_t)p["decay_interval"].as_double());
		if (p.contains("decay_start")) m_decay_start = (uint32_t)p["decay_start"].as_double();
		if (p.contains("decay_end")) m_decay_end = (uint32_t)p["decay_end"].as_double();
		if (p.contains("nested")) m_nested->update_hyperparams(p["nested"]);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "ExponentialDecay";
		j["nested"] = m_nested->hyperparams();
		j["decay_base"] = m_decay_base;
		j["decay_interval"] = m_decay_interval;
		j["decay_start"] = m_decay_start;
		j["decay_end"] = m_decay_end;
		return j;
	}
	Json serialize() const override {
		Json data = Json::object();
		data["nested"] = m_nested->serialize();
		data["learning_rate"] = Json(m_base_learning_rate);
		data["learning_rate_factor"] = Json(m_learning_rate_factor);
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		m_base_learning_rate = (float)data["learning_rate"].as_double();
		m_learning_rate_factor = data.value("learning_rate_factor", 1.0f);
		m_nested->deserialize(data["nested"], n_weights);
	}
private:
	std::unique_ptr<Optimizer> m_nested;
	float m_learning_rate_factor = 1.0f, m_base_learning_rate = 0.0f;
	float m_decay_base = 0.1f;
	uint32_t m_decay_interval = 10000, m_decay_start = 10000, m_decay_end = 10000000;
};

// optimizers/ema.h:44-230: debiased exponential moving average of the nested optimizer's weights, used for inference
class EmaOptimizer : public Optimizer {
public:
	explicit EmaOptimizer(const Json& params) {
		m_nested = create_optimizer(params.value("nested", Json::object()));
		update_hyperparams(params);
	}
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) override {
		m_nested->allocate(n_weights, layer_sizes);
		if (n_weights * weight_bytes() <= m_weights_ema.bytes()) return;
		m_weights_ema.resize(n_weights * weight_bytes());
		m_weights_ema.memset(0);
		if (m_full_precision && !fp32_weights()) { // (float EMA weights are their own fp32 copy)
			m_tmp.resize(n_weights * sizeof(float));
			m_tmp.memset(0);
		}
	}
	void set_weight_precision(Precision p) override { m_weight_precision = p; m_nested->set_weight_precision(p); }
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override { // :98-132
		weights = checked_weights(weights_full_precision, weights, precision);
		m_nested->step(stream, loss_scale, weights_full_precision, weights, gradients, precision);
		const uint32_t current_step = m_nested->step_count();
		const float ema_debias_old = 1 - (float)std::pow(m_ema_decay, current_step - 1);
		const float ema_debias_new = 1.0f / (1 - (float)std::pow(m_ema_decay, current_step));
		if (void* nested_custom = m_nested->custom_weights()) weights = nested_custom;
		ema_step(stream, n_weights(), m_ema_decay, ema_debias_old, ema_debias_new, weights, m_weights_ema.data(), m_full_precision && !fp32_weights() ? m_tmp.as<float>() : nullptr, m_weight_precision);
	}
	float learning_rate() const override { return m_nested->learning_rate(); }
	void set_learning_rate(float val) override { m_nested->set_learning_rate(val); }
	uint32_t step_count() const override { return m_nested->step_count(); }
	size_t n_weights() const override { return m_nested->n_weights(); }
	void* custom_weights() const override { return m_weights_ema.data(); }
	void update_hyperparams(const Json& p) override {
		if (!p.is_object()) return;
		if (p.contains("decay")) m_ema_decay = (float)p["decay"].as_double();
		if (p.contains("full_precision")) m_full_precision = p["full_precision"].as_bool();
		if (p.contains("nested")) m_nested->update_hyperparams(p["nested"]);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "EMA";
		j["nested"] = m_nested->hyperparams();
		j["decay"] = m_ema_decay;
		j["full_precision"] = m_full_precision;
		return j;
	}
	Json serialize() const override {
		Json data = Json::object();
		data["nested"] = m_nested->serialize();
		data["weights_ema_binary"] = device_to_binary(m_weights_ema.data(), n_weights() * weight_bytes());
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		const std::vector<uint8_t> bytes = binary_of(data["weights_ema_binary"]);
		if (bytes.size() != n_weights * weight_bytes()) throw std::runtime_error{"EMA: snapshot state has the wrong size."}; // (never reinterpreted in the other precision)
		m_weights_ema.resize(bytes.size());
		HIP_CHECK_THROW(hipMemcpy(m_weights_ema.data(), bytes.data(), bytes.size(), hipMemcpyHostToDevice));
		if (m_full_precision && !fp32_weights()) {
			m_tmp.resize(n_weights * sizeof(float));
			cast_half_to_float(nullptr, n_weights, m_weights_ema.data(), m_tmp.as<float>());
			HIP_CHECK_THROW(hipDeviceSynchronize());
		}
		m_nested->deserialize(data["nested"], n_weights);
	}
private:
	float m_ema_decay = 0.99f;
	bool m_full_precision = false;
	std::unique_ptr<Optimizer> m_nested;
	DeviceBuf m_weights_ema, m_tmp;
};

// optimizers/novograd.h:96-261: layer-wise second moments.  Only the weight MATRICES are optimized (the layer list is all it walks,
// :132-166): parameters behind them -- grid entries -- are left alone, as in the reference.
class NovogradOptimizer : public Optimizer {
public:
	explicit NovogradOptimizer(const Json& params) { update_hyperparams(params); }
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) override { // :103-124
		m_n_weights = n_weights;
		m_layers.clear();
		for (const auto& ls : layer_sizes) m_layers.push_back((size_t)ls.first * ls.second);
		m_first_moments.resize(0);
		m_first_moments.resize(n_weights * sizeof(float));
		m_first_moments.memset(0);
		m_per_layer_second_moments.resize(0);
		m_per_layer_second_moments.resize(m_layers.size() * sizeof(float));
		m_per_layer_second_moments.memset(0);
	}
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override { // :126-167
		weights = checked_weights(weights_full_precision, weights, precision);
		++m_current_step;
		size_t offset = 0;
		const size_t gradient_bytes = precision == GradientPrecision::Fp32 ? sizeof(float) : 2;
		for (size_t i = 0; i < m_layers.size(); ++i) {
			novograd_layer_step(stream, m_layers[i], m_relative_decay, m_absolute_decay, loss_scale, m_learning_rate, m_current_step == 1 ? 0.0f : m_beta1, // exact values on the first step
			                    m_current_step == 1 ? 0.0f : m_beta2, m_epsilon, weights_full_precision + offset, (char*)weights + weight_bytes() * offset, (const char*)gradients + gradient_bytes * offset,
			                    m_first_moments.as<float>() + offset, m_per_layer_second_moments.as<float>() + i, precision, m_weight_precision);
			offset += m_layers[i];
		}
	}
	float learning_rate() const override { return m_learning_rate; }
	void set_learning_rate(float val) override { m_learning_rate = val; }
	uint32_t step_count() const override { return m_current_step; }
	size_t n_weights() const override { return m_n_weights; }
	void update_hyperparams(const Json& p) override {
		if (!p.is_object()) return;
		if (p.contains("beta1")) m_beta1 = (float)p["beta1"].as_double();
		if (p.contains("beta2")) m_beta2 = (float)p["beta2"].as_double();
		if (p.contains("epsilon")) m_epsilon = (float)p["epsilon"].as_double();
		if (p.contains("learning_rate")) m_learning_rate = (float)p["learning_rate"].as_double();
		if (p.contains("relative_decay")) m_relative_decay = (float)p["relative_decay"].as_double();
		if (p.contains("absolute_decay")) m_absolute_decay = (float)p["absolute_decay"].as_double();
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "Novograd";
		j["beta1"] = m_beta1;
		j["beta2"] = m_beta2;
		j["epsilon"] = m_epsilon;
		j["learning_rate"] = m_learning_rate;
		j["relative_decay"] = m_relative_decay;
		j["absolute_decay"] = m_absolute_decay;
		return j;
	}
	Json serialize() const override {
		Json data = Json::object();
		data["current_step"] = Json((uint32_t)m_current_step);
		data["base_learning_rate"] = Json((float)m_learning_rate);
		data["first_moments_binary"] = device_to_binary(m_first_moments.data(), m_n_weights * sizeof(float));
		data["per_layer_second_moments_binary"] = device_to_binary(m_per_layer_second_moments.data(), m_layers.size() * sizeof(float));
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		const std::vector<uint8_t> first = binary_of(data["first_moments_binary"]), second = binary_of(data["per_layer_second_moments_binary"]);
		if (first.size() != n_weights * sizeof(float) || second.size() != m_layers.size() * sizeof(float)) throw std::runtime_error{"Novograd: snapshot state has the wrong size."};
		m_n_weights = n_weights;
		m_first_moments.resize(first.size());
		m_per_layer_second_moments.resize(second.size());
		if (!first.empty()) HIP_CHECK_THROW(hipMemcpy(m_first_moments.data(), first.data(), first.size(), hipMemcpyHostToDevice));
		if (!second.empty()) HIP_CHECK_THROW(hipMemcpy(m_per_layer_second_moments.data(), second.data(), second.size(), hipMemcpyHostToDevice));
		m_current_step = (uint32_t)data["current_step"].as_double();
		m_learning_rate = (float)data["base_learning_rate"].as_double();
	}
private:
	size_t m_n_weights = 0;
	std::vector<size_t> m_layers;
	DeviceBuf m_first_moments, m_per_layer_second_moments;
	uint32_t m_current_step = 0;
	float m_learning_rate = 1e-3f, m_beta1 = 0.9f, m_beta2 = 0.999f, m_epsilon = 1e-8f, m_relative_decay = 0.0f, m_absolute_decay = 0.0f;
};

// optimizers/average.h:62-174: the mean of the weights after each of the last n_samples steps, as inference weights
class AverageOptimizer : public Optimizer {
public:
	explicit AverageOptimizer(const Json& params) {
		m_nested = create_optimizer(params.value("nested", Json::object()));
		update_hyperparams(params);
	}
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) override { // :69-80
		m_n_weights = n_weights;
		m_layer_sizes = layer_sizes;
		m_allocated = true;
		m_nested->allocate(n_weights, layer_sizes);
		m_weights_samples.resize(0);
		m_weights_samples.resize(n_weights * m_n_samples * weight_bytes());
		m_weights_samples.memset(0);
		m_weights_average.resize(0);
		m_weights_average.resize(n_weights * weight_bytes());
		m_weights_average.memset(0);
	}
	void set_weight_precision(Precision p) override { m_weight_precision = p; m_nested->set_weight_precision(p); }
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override { // :82-92
		weights = checked_weights(weights_full_precision, weights, precision);
		m_nested->step(stream, loss_scale, weights_full_precision, weights, gradients, precision);
		char* current = (char*)m_weights_samples.data() + (size_t)(step_count() % m_n_samples) * m_n_weights * weight_bytes(); // the slot of the step just taken
		average_step(stream, m_n_weights, m_n_samples, weights, current, m_weights_average.data(), m_weight_precision);
	}
	float learning_rate() const override { return m_nested->learning_rate(); }
	void set_learning_rate(float val) override { m_nested->set_learning_rate(val); }
	uint32_t step_count() const override { return m_nested->step_count(); }
	size_t n_weights() const override { return m_nested->n_weights(); }
	void* custom_weights() const override { return m_weights_average.data(); }
	void update_hyperparams(const Json& p) override { // :131-142: a new window length starts the window over
		if (!p.is_object()) return;
		if (p.contains("n_samples")) {
			m_n_samples = (uint32_t)p["n_samples"].as_double();
			if (m_n_samples == 0) throw std::runtime_error{"AverageOptimizer: n_samples must be positive"};
			if (m_allocated) allocate(m_n_weights, m_layer_sizes);
		}
		if (p.contains("nested")) m_nested->update_hyperparams(p["nested"]);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "Average";
		j["nested"] = m_nested->hyperparams();
		j["n_samples"] = m_n_samples;
		return j;
	}
	Json serialize() const override {
		Json data = Json::object();
		data["nested"] = m_nested->serialize();
		data["weights_samples_binary"] = device_to_binary(m_weights_samples.data(), m_n_weights * m_n_samples * weight_bytes());
		data["weights_average_binary"] = device_to_binary(m_weights_average.data(), m_n_weights * weight_bytes());
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		const std::vector<uint8_t> samples = binary_of(data["weights_samples_binary"]), average = binary_of(data["weights_average_binary"]);
		if (average.size() != n_weights * weight_bytes() || samples.size() != n_weights * weight_bytes() * m_n_samples) throw std::runtime_error{"Average: snapshot state has the wrong size."};
		m_n_weights = n_weights;
		m_weights_samples.resize(samples.size());
		m_weights_average.resize(average.size());
		if (!samples.empty()) HIP_CHECK_THROW(hipMemcpy(m_weights_samples.data(), samples.data(), samples.size(), hipMemcpyHostToDevice));
		if (!average.empty()) HIP_CHECK_THROW(hipMemcpy(m_weights_average.data(), average.data(), average.size(), hipMemcpyHostToDevice));
		m_nested->deserialize(data["nested"], n_weights);
	}
private:
	uint32_t m_n_samples = 128;
	size_t m_n_weights = 0;
	bool m_allocated = false;
	std::vector<std::pair<uint32_t, uint32_t>> m_layer_sizes;
	std::unique_ptr<Optimizer> m_nested;
	DeviceBuf m_weights_samples, m_weights_average;
};

// optimizers/batched.h:63-162: the nested optimizer steps once per batch_size_multiplier calls, on the mean of their gradients
class BatchedOptimizer : public Optimizer {
public:
	explicit BatchedOptimizer(const Json& params) {
		m_nested = create_optimizer(params.value("nested", Json::object()));
		update_hyperparams(params);
	}
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) override {
		m_nested->allocate(n_weights, layer_sizes);
		m_averaged_gradients.resize(n_weights * sizeof(float));
		m_averaged_gradients.memset(0);
		if (fp32_weights()) return; // (fp32 gradients reach the nested optimizer as the fp32 mean: no half pool, in memory or in snapshots)
		m_averaged_gradients_half.resize(n_weights * 2);
		m_averaged_gradients_half.memset(0);
	}
	void set_weight_precision(Precision p) override { m_weight_precision = p; m_nested->set_weight_precision(p); }
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override { // :77-89
		weights = checked_weights(weights_full_precision, weights, precision);
		batched_accumulate(stream, n_weights(), m_current_step % m_batch_size_multiplier == 0, m_batch_size_multiplier, gradients, m_averaged_gradients.as<float>(), precision);
		++m_current_step;
		if (m_current_step % m_batch_size_multiplier == 0) {
			if (precision == GradientPrecision::Fp32) { // the nested optimizer reads the fp32 mean as it is: no rounding to half on the way
				m_nested->step(stream, loss_scale, weights_full_precision, weights, m_averaged_gradients.data(), precision);
				return;
			}
			cast_float_to_half(stream, n_weights(), m_averaged_gradients.as<float>(), m_averaged_gradients_half.data());
			m_nested->step(stream, loss_scale, weights_full_precision, weights, m_averaged_gradients_half.data());
		}
	}
	float learning_rate() const override { return m_nested->learning_rate(); }
	void set_learning_rate(float val) override { m_nested->set_learning_rate(val); }
	uint32_t step_count() const override { return m_current_step; }
	size_t n_weights() const override { return m_nested->n_weights(); }
	void* custom_weights() const override { return m_nested->custom_weights(); }
	void weights_restored(hipStream_t stream, const void* weights) override { m_nested->weights_restored(stream, weights); }
	void update_hyperparams(const Json& p) override {
		if (!p.is_object()) return;
		if (p.contains("batch_size_multiplier")) {
			m_batch_size_multiplier = (uint32_t)p["batch_size_multiplier"].as_double();
			if (m_batch_size_multiplier == 0) throw std::runtime_error{"BatchedOptimizer: batch_size_multiplier must be positive"};
		}
		if (p.contains("nested")) m_nested->update_hyperparams(p["nested"]);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "Batched";
		j["nested"] = m_nested->hyperparams();
		j["batch_size_multiplier"] = m_batch_size_multiplier;
		return j;
	}
	Json serialize() const override {
		Json data = Json::object();
		data["nested"] = m_nested->serialize();
		data["averaged_gradients_binary"] = device_to_binary(m_averaged_gradients.data(), n_weights() * sizeof(float));
		if (!fp32_weights()) data["averaged_gradients_half_binary"] = device_to_binary(m_averaged_gradients_half.data(), n_weights() * 2);
		data["current_step"] = Json((uint32_t)m_current_step);
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		const std::vector<uint8_t> pool = binary_of(data["averaged_gradients_binary"]);
		const std::vector<uint8_t> half = fp32_weights() ? std::vector<uint8_t>{} : binary_of(data["averaged_gradients_half_binary"]);
		if (pool.size() != n_weights * sizeof(float) || half.size() != (fp32_weights() ? 0 : n_weights * 2)) throw std::runtime_error{"Batched: snapshot state has the wrong size."};
		m_current_step = (uint32_t)data["current_step"].as_double();
		m_averaged_gradients.resize(pool.size());
		m_averaged_gradients_half.resize(half.size());
		if (!pool.empty()) HIP_CHECK_THROW(hipMemcpy(m_averaged_gradients.data(), pool.data(), pool.size(), hipMemcpyHostToDevice));
		if (!half.empty()) HIP_CHECK_THROW(hipMemcpy(m_averaged_gradients_half.data(), half.data(), half.size(), hipMemcpyHostToDevice));
		m_nested->deserialize(data["nested"], n_weights);
	}
private:
	uint32_t m_batch_size_multiplier = 16, m_current_step = 0;
	std::unique_ptr<Optimizer> m_nested;
	DeviceBuf m_averaged_gradients, m_averaged_gradients_half;
};

// optimizers/lookahead.h:61-168: every n_steps steps the slow weights move a fraction alpha towards the fast ones, which restart
// from them; the slow weights are the inference weights
class LookaheadOptimizer : public Optimizer {
public:
	explicit LookaheadOptimizer(const Json& params) {
		m_nested = create_optimizer(params.value("nested", Json::object()));
		update_hyperparams(params);
	}
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) override {
		m_nested->allocate(n_weights, layer_sizes);
		if (n_weights * weight_bytes() <= m_weights_lookahead.bytes()) return;
		m_weights_lookahead.resize(n_weights * weight_bytes());
		m_weights_lookahead.memset(0);
	}
	void set_weight_precision(Precision p) override { m_weight_precision = p; m_nested->set_weight_precision(p); }
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override { // :78-98
		weights = checked_weights(weights_full_precision, weights, precision);
		const uint32_t current_step = m_nested->step_count();
		if (current_step == 0) HIP_CHECK_THROW(hipMemcpyAsync(m_weights_lookahead.data(), weights, n_weights() * weight_bytes(), hipMemcpyDeviceToDevice, stream));
		if (current_step % m_n_steps == 0) lookahead_step(stream, n_weights(), m_alpha, weights_full_precision, weights, m_weights_lookahead.data(), m_weight_precision);
		m_nested->step(stream, loss_scale, weights_full_precision, weights, gradients, precision);
	}
	float learning_rate() const override { return m_nested->learning_rate(); }
	void set_learning_rate(float val) override { m_nested->set_learning_rate(val); }
	uint32_t step_count() const override { return m_nested->step_count(); }
	size_t n_weights() const override { return m_nested->n_weights(); }
	void* custom_weights() const override { return m_weights_lookahead.data(); }
	void update_hyperparams(const Json& p) override {
		if (!p.is_object()) return;
		if (p.contains("alpha")) m_alpha = (float)p["alpha"].as_double();
		if (p.contains("n_steps")) {
			m_n_steps = (uint32_t)p["n_steps"].as_double();
			if (m_n_steps == 0) throw std::runtime_error{"LookaheadOptimizer: n_steps must be positive"};
		}
		if (p.contains("nested")) m_nested->update_hyperparams(p["nested"]);
	}
	Json hyperparams() const override {
		Json j = Json::object();
		j["otype"] = "Lookahead";
		j["nested"] = m_nested->hyperparams();
		j["alpha"] = m_alpha;
		j["n_steps"] = m_n_steps;
		return j;
	}
	Json serialize() const override {
		Json data = Json::object();
		data["nested"] = m_nested->serialize();
		data["weights_lookahead_binary"] = device_to_binary(m_weights_lookahead.data(), n_weights() * weight_bytes());
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		const std::vector<uint8_t> bytes = binary_of(data["weights_lookahead_binary"]);
		if (bytes.size() != n_weights * weight_bytes()) throw std::runtime_error{"Lookahead: snapshot state has the wrong size."};
		m_weights_lookahead.resize(bytes.size());
		if (!bytes.empty()) HIP_CHECK_THROW(hipMemcpy(m_weights_lookahead.data(), bytes.data(), bytes.size(), hipMemcpyHostToDevice));
		m_nested->deserialize(data["nested"], n_weights);
	}
private:
	float m_alpha = 0.5f;
	uint32_t m_n_steps = 16;
	std::unique_ptr<Optimizer> m_nested;
	DeviceBuf m_weights_lookahead;
};

// optimizers/composite.h:44-74 (slice_weights) as it is meant: the layers that start at or after `offset`; a cut inside a layer
// is an error.  (The reference's loop advances the layer index before adding that layer's size: it skips layer 0 and runs one
// past the end of the list for any offset > 0 -- undefined behaviour there, the intended slice here.)
inline std::vector<std::pair<uint32_t, uint32_t>> slice_layer_sizes(const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes, size_t offset) {
	std::vector<std::pair<uint32_t, uint32_t>> out;
	size_t pos = 0;
	for (const auto& ls : layer_sizes) {
		const size_t size = (size_t)ls.first * ls.second;
		if (pos < offset && offset < pos + size) throw std::runtime_error{"Invalid slice. Can't slice within a layer."};
		if (pos >= offset) out.push_back(ls);
		pos += size;
	}
	return out;
}

// optimizers/composite.h:76-173: nested[i] optimizes the next "n_params_to_optimize" weights of the parameter vector
class CompositeOptimizer : public Optimizer {
public:
	explicit CompositeOptimizer(const Json& params) {
		if (!params.contains("nested") || !params["nested"].is_array() || params["nested"].size() == 0) {
			throw std::runtime_error{"Must provide an array of nested encodings to CompositeOptimizer."};
		}
		m_offsets.push_back(0);
		for (size_t i = 0; i < params["nested"].size(); ++i) {
			const Json& nested = params["nested"].at(i);
			m_offsets.push_back(m_offsets.back() + (size_t)nested.value("n_params_to_optimize", 0));
			m_nested.emplace_back(create_optimizer(nested));
			m_base_learning_rates.push_back(m_nested.back()->learning_rate());
		}
		update_hyperparams(params);
	}
	void allocate(size_t n_weights, const std::vector<std::pair<uint32_t, uint32_t>>& layer_sizes) override {
		CHECK_THROW(n_weights >= m_offsets.back()); // weights past the last nested optimizer stay as they are
		m_need_custom_weights = false;
		for (size_t i = 0; i < m_nested.size(); ++i) {
			m_nested[i]->allocate(m_offsets[i + 1] - m_offsets[i], slice_layer_sizes(layer_sizes, m_offsets[i]));
			m_need_custom_weights |= m_nested[i]->custom_weights() != nullptr;
		}
		m_n_total = n_weights;
		if (m_need_custom_weights) { // sized for the whole vector: the trainer runs inference from it (the reference sizes it to the optimized part only)
			m_custom_weights.resize(n_weights * weight_bytes());
			m_custom_weights.memset(0);
		}
	}
	void set_weight_precision(Precision p) override {
		m_weight_precision = p;
		for (auto& n : m_nested) n->set_weight_precision(p);
	}
	void step(hipStream_t stream, float loss_scale, float* weights_full_precision, void* weights, const void* gradients, GradientPrecision precision = GradientPrecision::Fp16) override {
		weights = checked_weights(weights_full_precision, weights, precision);
		const size_t gradient_bytes = precision == GradientPrecision::Fp32 ? sizeof(float) : 2;
		for (size_t i = 0; i < m_nested.size(); ++i) {
			const size_t offset = m_offsets[i];
			m_nested[i]->step(stream, loss_scale, weights_full_precision + offset, (char*)weights + weight_bytes() * offset, (const char*)gradients + gradient_bytes * offset, precision);
		}
		weights_restored(stream, weights);
	}
	// composite.h:86-93: the custom weights are the nested optimizers' custom weights where they have any, else the weights
	void weights_restored(hipStream_t stream, const void* weights) override {
		if (!m_need_custom_weights) return;
		const size_t wb = weight_bytes();
		for (size_t i = 0; i < m_nested.size(); ++i) {
			const size_t offset = m_offsets[i];
			m_nested[i]->weights_restored(stream, (const char*)weights + wb * offset);
			const void* src = m_nested[i]->custom_weights() ? m_nested[i]->custom_weights() : (const void*)((const char*)weights + wb * offset);
			HIP_CHECK_THROW(hipMemcpyAsync((char*)m_custom_weights.data() + wb * offset, src, m_nested[i]->n_weights() * wb, hipMemcpyDeviceToDevice, stream));
		}
		if (m_n_total > m_offsets.back()) {
			const size_t done = m_offsets.back();
			HIP_CHECK_THROW(hipMemcpyAsync((char*)m_custom_weights.data() + wb * done, (const char*)weights + wb * done, (m_n_total - done) * wb, hipMemcpyDeviceToDevice, stream));
		}
	}
	float learning_rate() const override { return m_learning_rate_factor; }
	void set_learning_rate(float val) override {
		m_learning_rate_factor = val;
		for (size_t i = 0; i < m_nested.size(); ++i) m_nested[i]->set_learning_rate(m_base_learning_rates[i] * m_learning_rate_factor);
	}
	uint32_t step_count() const override { return m_nested[0]->step_count(); }
	size_t n_weights() const override { return m_offsets.back(); }
	void* custom_weights() const override { return m_need_custom_weights ? m_custom_weights.data() : nullptr; }
	void update_hyperparams(const Json& p) override {
		if (!p.is_object() || !p.contains("nested") || !p["nested"].is_array()) return;
		for (size_t i = 0; i < m_nested.size() && i < p["nested"].size(); ++i) m_nested[i]->update_hyperparams(p["nested"].at(i));
	}
	Json hyperparams() const override {
		Json nested = Json::array();
		for (const auto& n : m_nested) nested.push_back(n->hyperparams());
		Json j = Json::object();
		j["otype"] = "Composite";
		j["nested"] = nested;
		return j;
	}
	Json serialize() const override {
		Json nested = Json::array(), rates = Json::array();
		for (const auto& n : m_nested) nested.push_back(n->serialize());
		for (float r : m_base_learning_rates) rates.push_back(Json(r));
		Json data = Json::object();
		data["nested"] = nested;
		data["base_learning_rates"] = rates;
		data["learning_rate_factor"] = m_learning_rate_factor;
		return data;
	}
	void deserialize(const Json& data, size_t n_weights) override {
		CHECK_THROW(n_weights >= m_offsets.back());
		const Json& nested = data["nested"];
		for (size_t i = 0; i < m_nested.size(); ++i) m_nested[i]->deserialize(nested.at(i), m_offsets[i + 1] - m_offsets[i]);
		const Json& rates = data["base_learning_rates"];
		m_base_learning_rates.clear();
		for (size_t i = 0; i < rates.size(); ++i) m_base_learning_rates.push_back((float)rates.at(i).as_double());
		set_learning_rate((float)data["learning_rate_factor"].as_double());
	}
private:
	std::vector<std::unique_ptr<Optimizer>> m_nested;
	std::vector<float> m_base_learning_rates;
	std::vector<size_t> m_offsets;
	size_t m_n_total = 0;
	float m_learning_rate_factor = 1.0f;
	bool m_need_custom_weights = false;
	DeviceBuf m_custom_weights;
};

// src/optimizer.cu:50-82
inline std::unique_ptr<Optimizer> create_optimizer(const Json& params) {
	const std::string otype = params.value("otype", "Adam");
	if (equals_case_insensitive(otype, "Adam")) return std::unique_ptr<Optimizer>{new AdamOptimizer{params}};
	if (equals_case_insensitive(otype, "SGD")) return std::unique_ptr<Optimizer>{new SgdOptimizer{params}};
	if (equals_case_insensitive(otype, "ExponentialDecay")) return std::unique_ptr<Optimizer>{new ExponentialDecayOptimizer{params}};
	if (equals_case_insensitive(otype, "Ema")) return std::unique_ptr<Optimizer>{new EmaOptimizer{params}};
	if (equals_case_insensitive(otype, "Composite")) return std::unique_ptr<Optimizer>{new CompositeOptimizer{params}};
	if (equals_case_insensitive(otype, "Average")) return std::unique_ptr<Optimizer>{new AverageOptimizer{params}};
	if (equals_case_insensitive(otype, "Batched")) return std::unique_ptr<Optimizer>{new BatchedOptimizer{params}};
	if (equals_case_insensitive(otype, "Lookahead")) return std::unique_ptr<Optimizer>{new LookaheadOptimizer{params}};
	if (equals_case_insensitive(otype, "Novograd")) return std::unique_ptr<Optimizer>{new NovogradOptimizer{params}};
	throw std::runtime_error{"Invalid optimizer type: " + otype + " (this build provides Adam, SGD, ExponentialDecay, Ema, Composite, Average, Batched, Lookahead, Novograd)"};
}

// ------------------------------------------------------------------------------------------------------------------
// Trainer (trainer.h:48-363) + create_from_config (config.h:53-63)
// ------------------------------------------------------------------------------------------------------------------
struct TrainContext { // Trainer::ForwardContext, trainer.h:89-95
	// (an fp32 trainer's output and dL_doutput are floats, and its contexts never take the compact form)
	ArenaBuf output;      // half  [n][padded_out]
	ArenaBuf dL_doutput;  // half  [n][padded_out]
	const void* dL_doutput_ptr = nullptr; // = dL_doutput or the caller's external_dL_dy
	ArenaBuf L;           // float [n][padded_out]
	std::unique_ptr<ModelContext> model_ctx;
	uint32_t n = 0;

	// Compact form (the register-resident fused MLP kernel, k_train_regs.hip): of the reference's [n][16] matrices dL_doutput and
	// L only the n_output_dims live columns are non-zero, and at 96 bytes per sample they would be more than a third of what that
	// kernel stores.  The step writes them dense as [n][dims]; the padded matrices are produced from those on first access
	// (tcnn_train_ctx_dL_doutput / _L), and loss() sums the compact L.
	bool compact = false;
	uint32_t dims = 0, padded_width = 0;
	hipStream_t stream = nullptr;
	ArenaBuf compact_dL_doutput; // half  [n][dims]
	ArenaBuf compact_L;          // float [n][dims]
	void materialize();
};

inline void TrainContext::materialize() {
	if (!compact || L) return;
	L = ArenaBuf{stream, (size_t)n * padded_width * sizeof(float)};
	dL_doutput = ArenaBuf{stream, (size_t)n * padded_width * 2};
	dL_doutput_ptr = dL_doutput.data();
	CHECK_THROW(padded_width == 16);
	mlp_expand_context(stream, n, dims, compact_dL_doutput.data(), compact_L.as<float>(), dL_doutput.data(), L.as<float>());
}

inline MatView make_view(const float* data, uint32_t width, uint32_t n, int layout) {
	return layout == 1 ? MatView{data, width, 1u} : MatView{data, 1u, n};
}
inline MatViewMut make_view_mut(float* data, uint32_t width, uint32_t n, int layout) {
	return layout == 1 ? MatViewMut{data, width, 1u} : MatViewMut{data, 1u, n};
}

class Trainer {
public:
	// precision Fp32: Trainer<float, float, float> of the reference's build without TCNN_HALF_PRECISION -- the fp32 module, Loss<float>,
	// Optimizer<float>, loss scale 1.  ONE float parameter vector (params() == params_full_precision()), float gradients, float output and
	// dL_doutput; every training step is the unfused sequence forward -> loss -> backward -> optimizer.
	Trainer(uint32_t n_input_dims, uint32_t n_output_dims, const Json& config, uint32_t seed, Precision precision = Precision::Fp16) : m_fp32{precision == Precision::Fp32} {
		// config.h:53-63
		const Json encoding = config.value("encoding", Json::object());
		const Json loss = config.value("loss", Json::object());
		const Json optimizer = config.value("optimizer", Json::object());
		const Json network = config.value("network", Json::object());
		m_loss = create_loss(loss);
		m_optimizer = create_optimizer(optimizer);
		if (m_fp32) { // what the configuration alone decides is reported before anything is allocated on the device (network.cu:102-103)
			const std::string otype = network.is_object() ? network.value("otype", "MLP") : std::string{"MLP"};
			if (equals_case_insensitive(otype, "MegakernelMLP") || equals_case_insensitive(otype, "FullyFusedMLP")) {
				throw std::runtime_error{"FullyFusedMLP can only be used if the network precision is set to __half."};
			}
		}
		m_model.reset(new NetworkWithInputEncoding{n_input_dims, n_output_dims, encoding, network, precision});
		// trainer.h:52-55
		std::seed_seq seq{seed};
		std::vector<uint32_t> seeds(2);
		seq.generate(std::begin(seeds), std::end(seeds));
		m_rng = Pcg32{seeds.front()};
		m_scalar.resize(sizeof(float) * 2048);
		initialize_params();
	}

	void initialize_params() { // trainer.h:68-87
		const size_t n = m_model->n_params();
		m_optimizer->allocate(n, m_model->layer_sizes(), precision());
		m_params_fp.resize(n * sizeof(float));
		m_grads.resize(n * elem());
		m_params_fp.memset(0);
		m_grads.memset(0);
		m_model->initialize_params(m_rng, m_params_fp.as<float>(), 1.0f);
		if (!m_fp32) { // (fp32: the master vector is the working vector)
			m_params.resize(n * 2);
			m_params.memset(0);
			cast_float_to_half(nullptr, n, m_params_fp.as<float>(), m_params.data());
		}
		HIP_CHECK_THROW(hipDeviceSynchronize());
	}

	std::unique_ptr<TrainContext> forward(hipStream_t stream, float loss_scale, uint32_t n, MatView input, const float* target, const float* data_pdf,
	                                      bool use_inference_params, bool prepare_input_gradients, const void* external_dL_dy) { // trainer.h:97-141
		auto ctx = std::make_unique<TrainContext>();
		ctx->n = n;
		const uint32_t pw = m_model->padded_output_width();
		ctx->output = ArenaBuf{stream, (size_t)n * pw * elem()};
		ctx->model_ctx = m_model->forward(stream, n, input, ctx->output.data(), use_inference_params ? params_inference() : working_params(), prepare_input_gradients);
		ctx->L = ArenaBuf{stream, (size_t)n * pw * sizeof(float)};
		if (external_dL_dy) {
			ctx->dL_doutput_ptr = external_dL_dy;
			// the reference leaves L uninitialised in this case; zero it so that loss() is defined
			HIP_CHECK_THROW(hipMemsetAsync(ctx->L.data(), 0, ctx->L.bytes(), stream));
		} else {
			CHECK_THROW(target != nullptr);
			ctx->dL_doutput = ArenaBuf{stream, (size_t)n * pw * elem()};
			ctx->dL_doutput_ptr = ctx->dL_doutput.data();
			loss_evaluate(stream, m_loss, n, pw, m_model->output_width(), loss_scale, ctx->output.data(), target, ctx->L.as<float>(), ctx->dL_doutput.data(), data_pdf, precision());
		}
		return ctx;
	}

	void backward(hipStream_t stream, const TrainContext& ctx, uint32_t n, MatView input, MatViewMut* dL_dinput, bool use_inference_params, GradientMode mode) { // trainer.h:147-149
		const_cast<TrainContext&>(ctx).materialize(); // a context of the fused step keeps dL_doutput compact until somebody asks for it
		m_model->backward(stream, *ctx.model_ctx, n, input, ctx.output.data(), ctx.dL_doutput_ptr, dL_dinput, use_inference_params ? params_inference() : working_params(), m_grads.data(), mode);
	}

	size_t params_updated_in_flush() const { return m_params_updated_in_flush; }
	size_t m_prologue_steps = 0;

	// Where the optimizer's update of a fused step runs (OptimizerPlace), decided once, before the step, and binding except that an offered
	// prologue may come back not taken (the tuner's timed step, binned levels, a scalar max_level, a Composite encoding, shapes the
	// optimizer's launch refuses): then the finalize pass and the optimizer are the two launches they were.
	//   InReduce (TCNN_AMD_ADAM_IN_REDUCE=0 turns it off): models without encoding parameters (BASELINE config 2) -- the update runs behind
	//     the weight gradients' slab reduction (k_wgrad_reduce_adam; bit-identical, one ~4 us launch less per step);
	//   Prologue (TCNN_AMD_ADAM_PROLOGUE=0 turns it off): the scatter's finalize pass and the MLP's slab reduction as the prologue of the
	//     optimizer's launch (k_adam_prologue; one launch and one kernel boundary less per step).
	OptimizerPlace optimizer_place(bool run_optimizer, GradientMode mode, bool want_dL_dinput) const {
		if (!run_optimizer) return OptimizerPlace::None;
		const Switches sw = switches();
		if (sw.adam_in_reduce && m_optimizer->can_step_in_reduce() && m_model->reduction_carries_update(want_dL_dinput, mode)) return OptimizerPlace::InReduce;
		if (sw.adam_prologue && mode != GradientMode::Ignore && m_optimizer->takes_prologue()) return OptimizerPlace::Prologue;
		return OptimizerPlace::OwnLaunch;
	}

	// the finalize pass and the slab reduction an AdamPrologue holds, as the launches they were
	void run_prologue_alone(hipStream_t stream, const AdamPrologue& p) {
		MlpReduceJob job;
		if (p.has_reduce) {
			job.n_elems = p.reduce_elems;
			job.n_slabs = p.reduce_slabs;
			job.slabs = p.slabs;
			job.grad = m_grads.data();
			job.accumulate = p.reduce_accumulate;
		}
		if (!p.ranges.empty()) grid_scatter_finalize(stream, p.dev_ranges, (uint32_t)p.ranges.size(), p.scratch, p.grad_base, p.accumulate, p.has_reduce ? &job : nullptr);
		else if (p.has_reduce) mlp_reduce_slabs(stream, p.reduce_elems, p.reduce_slabs, p.slabs, m_grads.data(), p.reduce_accumulate != 0);
	}

	void optimizer_step(hipStream_t stream, float loss_scale) { // trainer.h:155-157
		m_model->invalidate_live_image();
		m_optimizer->step(stream, loss_scale, m_params_fp.as<float>(), working_params(), m_grads.data(), m_fp32 ? GradientPrecision::Fp32 : GradientPrecision::Fp16);
	}

	std::unique_ptr<TrainContext> training_step(hipStream_t stream, uint32_t n, MatView input, const float* target, const float* data_pdf, bool run_optimizer,
	                                            MatViewMut* dL_dinput, bool use_inference_params, GradientMode mode, const void* external_dL_dy) { // trainer.h:163-190
		const float loss_scale = m_fp32 ? 1.0f : LOSS_SCALE_FP16; // (tcnn_default_loss_scale)
		std::unique_ptr<TrainContext> ctx;
		const bool other_weights = use_inference_params && params_inference() != working_params(); // EMA weights requested for this step
		if (!m_fp32 && m_model->fused_step_supported(n) && (external_dL_dy || loss_in_fused_kernel(m_loss)) && !other_weights) {
			// MI355X path: encoding -> ONE fused MLP kernel (forward + loss + backward + weight gradients) -> grid scatter
			ctx = std::make_unique<TrainContext>();
			ctx->n = n;
			const uint32_t pw = m_model->padded_output_width();
			ctx->output = ArenaBuf{stream, (size_t)n * pw * 2};
			ctx->compact = !external_dL_dy && mode != GradientMode::Ignore && m_model->fused_compact_context_supported(n);
			if (ctx->compact) {
				CHECK_THROW(target != nullptr);
				ctx->dims = m_model->output_width();
				ctx->padded_width = pw;
				ctx->stream = stream;
				ctx->compact_dL_doutput = ArenaBuf{stream, (size_t)n * ctx->dims * 2};
				ctx->compact_L = ArenaBuf{stream, (size_t)n * ctx->dims * sizeof(float)};
			} else {
				ctx->L = ArenaBuf{stream, (size_t)n * pw * sizeof(float)};
				if (external_dL_dy) {
					ctx->dL_doutput_ptr = external_dL_dy;
					HIP_CHECK_THROW(hipMemsetAsync(ctx->L.data(), 0, ctx->L.bytes(), stream));
				} else {
					CHECK_THROW(target != nullptr);
					ctx->dL_doutput = ArenaBuf{stream, (size_t)n * pw * 2};
					ctx->dL_doutput_ptr = ctx->dL_doutput.data();
				}
			}
			m_params_updated_in_flush = 0;
			m_profile.begin_step();
			const OptimizerPlace place = optimizer_place(run_optimizer, mode, dL_dinput != nullptr);
			AdamInReduce in_reduce;
			AdamPrologue prologue;
			OptimizerOffer offer;
			if (place == OptimizerPlace::InReduce) {
				in_reduce = m_optimizer->begin_step_in_reduce(stream, loss_scale, m_params_fp.as<float>(), m_params.data());
				offer.in_reduce = &in_reduce;
			} else if (place == OptimizerPlace::Prologue) offer.prologue = &prologue;
			FusedStepData step;
			step.target = target, step.data_pdf = data_pdf, step.external_dL_dy = external_dL_dy;
			step.loss = m_loss;
			step.loss_scale = loss_scale;
			step.out = ctx->output.data();
			step.dL_dout = ctx->compact ? ctx->compact_dL_doutput.data() : ctx->dL_doutput.data();
			step.L = ctx->compact ? ctx->compact_L.as<float>() : ctx->L.as<float>();
			step.compact_context = ctx->compact;
			step.dL_dinput = dL_dinput;
			step.params = m_params.data(), step.gradients = m_grads.data();
			step.mode = mode;
			step.profile = &m_profile;
			ctx->model_ctx = m_model->fused_step(stream, n, input, step, offer);
			// The network's live fragment image outlives the step only if its weights are what they were, or the launch that updated them
			// kept the image current (InReduce, Network::live_image) -- and never once somebody holds a pointer to the parameters.
			if (m_params_exposed || (place != OptimizerPlace::None && !m_model->live_image_kept())) m_model->invalidate_live_image();
			if (place != OptimizerPlace::None) {
				m_profile.mark(stream, StepProfile::Optimizer, false);
				if (place == OptimizerPlace::InReduce) m_params_updated_in_flush = m_model->n_params(); // the reduction has applied the update: nothing more to launch
				else if (prologue.pending && m_optimizer->step_with_prologue(stream, loss_scale, m_params_fp.as<float>(), m_params.data(), m_grads.data(), prologue)) ++m_prologue_steps;
				else {
					if (prologue.pending) run_prologue_alone(stream, prologue); // shapes the fused launch does not take: the two launches of before
					m_optimizer->step(stream, loss_scale, m_params_fp.as<float>(), m_params.data(), m_grads.data());
				}
				m_profile.mark(stream, StepProfile::Optimizer, true);
			}
			m_profile.end_step();
			m_last_step_kernel = m_model->last_train_kernel();
			return ctx;
		} else {
			m_last_step_kernel = "unfused";
			ctx = forward(stream, loss_scale, n, input, target, data_pdf, use_inference_params, dL_dinput != nullptr, external_dL_dy);
			backward(stream, *ctx, n, input, dL_dinput, use_inference_params, mode);
		}
		m_params_updated_in_flush = 0;
		if (run_optimizer) optimizer_step(stream, loss_scale);
		return ctx;
	}

	float loss(hipStream_t stream, const TrainContext& ctx) { // trainer.h:205-207 + reduce_sum.h:140-151
		float* partials = m_scalar.as<float>();
		float* result = partials + 1024;
		if (ctx.compact && !ctx.L) reduce_sum(stream, (size_t)ctx.n * ctx.dims, ctx.compact_L.as<float>(), partials, result); // the padding columns are zeros
		else reduce_sum(stream, (size_t)ctx.n * m_model->padded_output_width(), ctx.L.as<float>(), partials, result);
		float host = 0;
		HIP_CHECK_THROW(hipMemcpyAsync(&host, result, sizeof(float), hipMemcpyDeviceToHost, stream));
		HIP_CHECK_THROW(hipStreamSynchronize(stream));
		return host;
	}

	void inference(hipStream_t stream, uint32_t n, MatView input, MatViewMut output, bool use_inference_params) { // object.h:147-176
		Model::check_batch(n);
		if (n == 0) return;
		m_model->inference_f32(stream, n, input, output, use_inference_params ? params_inference() : working_params());
	}

	// object.h:342-366 on the inference parameters (trainer.h binds them to the model): no gradient buffer, no optimizer state is touched
	void input_gradient(hipStream_t stream, uint32_t n, uint32_t dim, MatView input, MatViewMut d_dinput, float backprop_scale) {
		m_model->input_gradient(stream, n, dim, input, d_dinput, nullptr, params_inference(), backprop_scale);
	}
	void input_jacobian(hipStream_t stream, uint32_t n, const uint32_t* dims, uint32_t n_dims, MatView input, float* jacobian, float backprop_scale) {
		m_model->input_jacobian(stream, n, dims, n_dims, input, jacobian, nullptr, params_inference(), backprop_scale);
	}
	void input_jvp(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, void* jvp) {
		m_model->input_jvp(stream, n, n_tangents, input, tangents, jvp, nullptr, params_inference());
	}

	// object.h:133-145, inference_mixed_precision: the network's own output, half [n][padded_output_width] (what inference() casts); floats from an fp32 trainer
	void inference_mixed_precision(hipStream_t stream, uint32_t n, MatView input, void* output_half, bool use_inference_params) {
		Model::check_batch(n);
		if (n == 0) return;
		m_model->inference(stream, n, input, output_half, use_inference_params ? params_inference() : working_params());
	}

	void set_params_full_precision(const float* params, size_t n_params, bool device_ptr) { // trainer.h:242-254
		if (n_params != m_model->n_params()) throw std::runtime_error{"Can't set fp params because buffer has the wrong size."};
		m_model->invalidate_live_image();
		HIP_CHECK_THROW(hipMemcpy(m_params_fp.data(), params, sizeof(float) * n_params, device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
		if (!m_fp32) cast_float_to_half(nullptr, n_params, m_params_fp.as<float>(), m_params.data());
		if (params_inference() != working_params()) HIP_CHECK_THROW(hipMemcpy(params_inference(), working_params(), elem() * n_params, hipMemcpyDeviceToDevice));
		HIP_CHECK_THROW(hipDeviceSynchronize());
	}

	// params: in the trainer's precision (an fp32 trainer's parameters ARE the full-precision ones)
	void set_params(const void* params, size_t n_params, bool device_ptr) { // trainer.h:256-269
		if (n_params != m_model->n_params()) throw std::runtime_error{"Can't set params because buffer has the wrong size."};
		if (m_fp32) return set_params_full_precision((const float*)params, n_params, device_ptr);
		m_model->invalidate_live_image();
		HIP_CHECK_THROW(hipMemcpy(m_params.data(), params, 2 * n_params, device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
		cast_half_to_float(nullptr, n_params, m_params.data(), m_params_fp.as<float>());
		if (params_inference() != m_params.data()) HIP_CHECK_THROW(hipMemcpy(params_inference(), m_params.data(), 2 * n_params, hipMemcpyDeviceToDevice));
		HIP_CHECK_THROW(hipDeviceSynchronize());
	}

	void update_hyperparams(const Json& params) { // trainer.h:213-216
		m_optimizer->update_hyperparams(params.value("optimizer", Json::object()));
	}

	// ---- snapshot wire format, trainer.h:275-315 (+ adam.h:278-299, gpu_memory_json.h:36-71): an object holding the half
	// parameters as a binary blob and, optionally, the optimizer's state.  Callers store it as MessagePack (Json::to_msgpack).
	Json serialize(bool serialize_optimizer) {
		HIP_CHECK_THROW(hipDeviceSynchronize());
		const size_t n = m_model->n_params();
		Json data = Json::object();
		data["n_params"] = Json((uint64_t)n);
		data["params_type"] = m_fp32 ? "float" : "__half"; // type_to_string<T>() of the reference: the name snapshots carry
		data["params_binary"] = device_to_binary(params_inference(), elem() * n); // trainer.h:281: the inference parameters (EMA weights if there are any)
		if (serialize_optimizer) data["optimizer"] = m_optimizer->serialize();
		return data;
	}

	void deserialize(const Json& data) {
		const std::string type = data.value("params_type", "__half");
		const std::vector<uint8_t> bytes = binary_of(data["params_binary"]);
		if (type == "float") {
			if (bytes.size() % sizeof(float) != 0) throw std::runtime_error{"Can't set fp params because buffer has the wrong size."};
			set_params_full_precision((const float*)bytes.data(), bytes.size() / sizeof(float), false);
		} else if (type == "__half" && m_fp32) { // trainer.h:303-305: cast to the trainer's type
			if (bytes.size() != 2 * m_model->n_params()) throw std::runtime_error{"Can't set params because buffer has the wrong size."};
			DeviceBuf half;
			half.resize(bytes.size());
			DeviceBuf wide;
			wide.resize(bytes.size() * 2);
			if (!bytes.empty()) HIP_CHECK_THROW(hipMemcpy(half.data(), bytes.data(), bytes.size(), hipMemcpyHostToDevice));
			cast_half_to_float(nullptr, bytes.size() / 2, half.data(), wide.as<float>());
			HIP_CHECK_THROW(hipDeviceSynchronize());
			set_params_full_precision(wide.as<float>(), bytes.size() / 2, true);
		} else if (type == "__half") {
			if (bytes.size() % 2 != 0) throw std::runtime_error{"Can't set params because buffer has the wrong size."};
			set_params(bytes.data(), bytes.size() / 2, false);
		} else {
			throw std::runtime_error{"Trainer: snapshot parameters must be of type float of __half"};
		}
		if (data.contains("optimizer")) {
			m_optimizer->deserialize(data["optimizer"], m_model->n_params());
			m_optimizer->weights_restored(nullptr, working_params());
		}
		HIP_CHECK_THROW(hipDeviceSynchronize());
	}

	Json hyperparams() const { // trainer.h:218-224
		Json j = Json::object();
		j["otype"] = "Trainer";
		j["optimizer"] = m_optimizer->hyperparams();
		Json l = Json::object();
		l["otype"] = to_string(m_loss);
		j["loss"] = l;
		return j;
	}

	// Training through input_jvp on the trainer's training parameters: Model::input_jvp_forward / _backward, the parameter gradients into
	// the trainer's gradient buffer (optimizer_step() reads it).  No loss scale inside: the caller's cotangents carry it.
	std::unique_ptr<ModelContext> input_jvp_forward(hipStream_t stream, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, void* jvp, void* output) {
		return m_model->input_jvp_forward(stream, n, n_tangents, input, tangents, jvp, output, working_params());
	}
	void input_jvp_backward(hipStream_t stream, const ModelContext& ctx, uint32_t n, uint32_t n_tangents, MatView input, const float* tangents, const void* dL_djvp, const void* dL_doutput,
	                        MatViewMut* dL_dinput, float* dL_dtangents, GradientMode mode) {
		m_model->input_jvp_backward(stream, ctx, n, n_tangents, input, tangents, dL_djvp, dL_doutput, working_params(), m_grads.data(), dL_dinput, dL_dtangents, mode);
	}

	NetworkWithInputEncoding& model() { return *m_model; }
	Optimizer& optimizer() { return *m_optimizer; }
	StepProfile& profile() { return m_profile; }
	// trainer.h:329-333: the optimizer's own weights (EMA) if it keeps any, else the training parameters
	void* params_inference() const { void* custom = m_optimizer->custom_weights(); return custom ? custom : working_params(); }
	Precision precision() const { return m_fp32 ? Precision::Fp32 : Precision::Fp16; }
	size_t elem() const { return m_fp32 ? sizeof(float) : 2; } // bytes of a parameter, an output element, a gradient
	// the parameters training runs with: the half copy, or the one float vector of an fp32 trainer
	void* working_params() const { return m_fp32 ? m_params_fp.data() : m_params.data(); }
	size_t n_params() const { return m_model->n_params(); }
	// The reference hands out mutable pointers here (trainer.h:226-232).  A caller may write through them at any later time, so from the
	// first call on no fragment image of the half parameters is trusted beyond the step that built it (Network::live_image)
	float* params_full_precision() { expose_params(); return m_params_fp.as<float>(); }
	void* params() { expose_params(); return working_params(); }
	const void* params_unexposed() const { return working_params(); } // for comparisons only
	size_t image_preps() const { return m_model->image_preps(); }
	uint64_t scatter_wide_fallbacks() { return m_model->scatter_wide_fallbacks(); }
	uint64_t list_scatters() const { return m_model->list_scatters(); }
	uint64_t list_gradient_tails() const { return m_model->list_gradient_tails(); }
	size_t prologue_steps() const { return m_prologue_steps; }
	// short name of the MLP training kernel the last training_step launched ("unfused": k_mlp_fwd -> k_loss -> k_mlp_bwd -> k_wgrad*; "" before the first)
	const char* last_step_kernel() const { return m_last_step_kernel; }
	void* param_gradients() const { return m_grads.data(); }

private:
	std::unique_ptr<NetworkWithInputEncoding> m_model;
	std::unique_ptr<Optimizer> m_optimizer;
	LossType m_loss;
	Pcg32 m_rng;
	DeviceBuf m_params_fp, m_params, m_grads, m_scalar;
	StepProfile m_profile;
	size_t m_params_updated_in_flush = 0;
	const char* m_last_step_kernel = "";
	bool m_params_exposed = false;
	const bool m_fp32 = false;
	void expose_params() {
		m_params_exposed = true;
		m_model->invalidate_live_image();
	}
};

} // namespace tcnn_amd
