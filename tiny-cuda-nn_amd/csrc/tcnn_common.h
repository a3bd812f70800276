// tcnn_common.h -- shared enums, error macros and kernel-launcher declarations of libtcnn_amd (gfx950 only).
//
// Names follow the reference's vocabulary (include/tiny-cuda-nn/common.h:112-170) so that the host object model in
// module.cpp reads like the reference's; the numbering is ours.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace tcnn_amd {

enum class Activation : uint32_t { None = 0, ReLU = 1, LeakyReLU = 2, Exponential = 3, Sine = 4, Sigmoid = 5, Squareplus = 6, Softplus = 7, Tanh = 8 };
enum class GridType : uint32_t { Hash = 0, Dense = 1, Tiled = 2 };
enum class HashType : uint32_t { Prime = 0, CoherentPrime = 1, ReversedPrime = 2, Rng = 3 };
enum class InterpolationType : uint32_t { Nearest = 0, Linear = 1, Smoothstep = 2 };
enum class LossType : uint32_t { L2 = 0, RelativeL2 = 1, L1 = 2, RelativeL1 = 3, Mape = 4, Smape = 5, CrossEntropy = 6, Variance = 7, RelativeL2Luminance = 8 }; // src/loss.cu:57-65
enum class Precision : uint32_t { Fp32 = 0, Fp16 = 1 };      // cpp_api.h:69-72
// what an optimizer's `gradients` pointer holds: the trainer's half gradients, or a caller's own fp32 ones (same values as Precision)
enum class GradientPrecision : uint32_t { Fp32 = 0, Fp16 = 1 };
enum class GradientMode : uint32_t { Ignore = 0, Overwrite = 1, Accumulate = 2 }; // common.h GradientMode

constexpr uint32_t BATCH_SIZE_GRANULARITY = 256; // common.h:235
constexpr float LOSS_SCALE_FP16 = 128.0f;        // common.h:232
constexpr uint32_t MAX_N_LEVELS = 128;           // grid_interface.h:84
constexpr uint32_t MAX_MLP_LAYERS = 16;

#define TCNN_STR2(x) #x
#define TCNN_STR(x) TCNN_STR2(x)
#define CHECK_THROW(x) \
	do { if (!(x)) throw std::runtime_error{std::string{__FILE__ ":" TCNN_STR(__LINE__) " check failed: " #x}}; } while (0)
#define HIP_CHECK_THROW(x) \
	do { hipError_t _e = (x); if (_e != hipSuccess) throw std::runtime_error{std::string{__FILE__ ":" TCNN_STR(__LINE__) " " #x " failed: "} + hipGetErrorString(_e)}; } while (0)

inline uint32_t div_round_up(uint32_t v, uint32_t d) { return (v + d - 1) / d; }

// The A/B switches of the training step and of inference (DESIGN.md "Switches"): every one defaults to the fast path, none changes a result
// beyond what is stated there.  They are read from the environment when create_from_config / a module constructor runs (switches_reload,
// capi.cpp) -- not per step -- and the set is PROCESS-WIDE: creating a model under another environment changes the kernels of every live
// model from its next pass on (reads and the reload are serialised by a lock; a grid's backward pass follows its forward pass: GridForwardRoute).
// A process that wants another setting sets the variable and creates its models afterwards; tests that compare two settings build one model at a time.
// switches_reload() is the ONLY reader of the environment in the product library: a consumer is handed a copy, or takes one (switches()) once per call.
struct Switches {
	bool grid_planes = true;      // TCNN_AMD_GRID_PLANES=0: the AoS forward kernel inside the fused training step
	bool grid_rows_planes = true; // TCNN_AMD_GRID_ROWS_PLANES=0: callers that want the encoded batch as a matrix get k_grid_fwd (AoS) instead of the plane kernel + a transposition
	bool grid_scatter_lds = true; // TCNN_AMD_GRID_SCATTER=atomic: the reference-shaped global-atomic gradient kernel
	bool scatter_records = true;  // TCNN_AMD_SCATTER_RECORDS=0: gradient planes instead of {coordinates, gradient} records
	bool scatter_tune = true;     // TCNN_AMD_SCATTER_TUNE=0: the untuned task list of k_grid_scatter
	int scatter_lists = -1;       // TCNN_AMD_SCATTER_LISTS=0 / 1: never / wherever possible (unset: where it pays, grid_scatter_prefers_lists)
	bool scatter_wide = false;    // TCNN_AMD_SCATTER_WIDE=1: every task of k_grid_scatter_lists through its 64-bit passes (tests)
	bool fused_step = true;       // TCNN_AMD_FUSED_STEP=0: forward / loss / backward / wgrad kernels instead of the fused step
	bool side_jobs = true;        // TCNN_AMD_SIDE_JOBS=0: k_mlp_prep and the slab reduction as launches of their own
	bool live_image = true;       // TCNN_AMD_LIVE_IMAGE=0: k_mlp_prep every step
	bool adam_steps32 = false;    // TCNN_AMD_ADAM_STEPS32=1: uint32 update counts from the start
	bool adam_in_reduce = true;   // TCNN_AMD_ADAM_IN_REDUCE=0: k_adam as a launch of its own for models without encoding parameters
	bool adam_prologue = true;    // TCNN_AMD_ADAM_PROLOGUE=0: the scatter's finalize pass (+ slab reduction) as a launch of its own in front of k_adam
	bool adam_prologue_refused = false; // TCNN_AMD_ADAM_PROLOGUE=refuse (tests): the optimizer is offered the prologue and turns it down, as it does for shapes its launch does not take
	bool mlp_r32 = true;          // TCNN_AMD_MLP_R32=0: k_mlp_train_regs / k_mlp_train instead of the 32x32x16 kernels
	int mlp_r32a = -1;            // TCNN_AMD_MLP_R32A=0 / 1: k_mlp_train_r32 / k_mlp_train_r32a whatever the batch size
	bool mlp_regs = true;         // TCNN_AMD_MLP_REGS=0: the LDS-image kernels of k_train.hip
	bool mlp_fast = true;         // TCNN_AMD_MLP_FAST=0: k_mlp_train_regs with run-time formats
	uint32_t mlp_prio = 1;        // TCNN_AMD_MLP_PRIO: wave priorities of the MLP kernels (0 none, 1 alternating per trip, 2, 3)
	bool listgrad_in_mlp = true;  // TCNN_AMD_LISTGRAD_IN_MLP=0: k_grid_list_gradients as a launch of its own instead of the tail of k_mlp_train_r32
	bool mlp_layerwise = false;   // TCNN_AMD_MLP_LAYERWISE=1: every network of a model created now runs the layer-by-layer kernels (k_mlp_layers.hip)
	bool mlp_regw = true;         // TCNN_AMD_MLP_REGW=0: k_mlp_train reads its weight fragments from the images instead of holding them in registers
	bool mlp_variant_forced = false; // TCNN_AMD_MLP_VARIANT=nb,nw,maxt (all three must parse): k_train.hip's table offers that instance of k_mlp_train alone
	int mlp_variant[3] = {0, 0, 0};  //   nb, nw, maxt
	bool wgrad_rows = true;       // TCNN_AMD_WGRAD_ROWS=0: mlp_wgrad_panels runs k_wgrad for every shape, never k_wgrad_rows / k_wgrad_cols
	bool mlp_fwd_lds = true;      // TCNN_AMD_MLP_FWD_LDS=0: wide inference (128 neurons, large batches) keeps its fragment image in L2 instead of LDS
	bool fuse_oneblob = true;     // TCNN_AMD_FUSE_ONEBLOB=0: a OneBlob encoding in front of a network is encoded into rows, never inside the MLP kernels
};
Switches switches(); // a copy of the process-wide set, taken under its lock
void switches_reload();

// Laboratory knobs (DESIGN.md "Switches"): environment variables that only the laboratory build (build.py --dev) reads.  In the product
// library the answer is "unset" at compile time, and what hangs on a knob is dead code.
#ifdef TCNN_AMD_DEV
inline const char* lab_env(const char* name) { return getenv(name); }
#else
constexpr const char* lab_env(const char*) { return nullptr; }
#endif

// Laboratory build with the variable `env` set: the in-kernel clocks of a launch site's `launches`-th launch.  A launch function keeps one
// static DevClocks; in the product library alloc() is nullptr, fetch() is false and the printing behind it is dead code.
struct DevClocks {
	const char* env;
	int left;
	explicit DevClocks(const char* env_, int launches = 5) : env{env_}, left{launches} {}
	// a zeroed buffer for the kernel's `dbg` argument while the site's launches are still counted, else nullptr
	unsigned long long* alloc(size_t bytes) const {
		unsigned long long* dbg = nullptr;
		if (lab_env(env) && left > 0) {
			HIP_CHECK_THROW(hipMalloc(&dbg, bytes));
			HIP_CHECK_THROW(hipMemset(dbg, 0, bytes));
		}
		return dbg;
	}
	// after the launch: the first `count` clocks to the host, the buffer freed; true on the launch whose clocks are to be printed
	bool fetch(unsigned long long* dbg, unsigned long long* host, size_t count) {
		if (!dbg) return false;
		HIP_CHECK_THROW(hipMemcpy(host, dbg, count * 8, hipMemcpyDeviceToHost));
		(void)hipFree(dbg);
		return --left == 0;
	}
};
inline uint32_t next_multiple(uint32_t v, uint32_t d) { return div_round_up(v, d) * d; }

// ------------------------------------------------------------------------------------------------------------------
// Grid encoding: per-level table precomputed on the HOST (so host and device agree bit-for-bit on scale/resolution,
// SURVEY 7 "hard parts"); the encoding keeps one device copy (6 KiB, too large for the kernarg segment).
// ------------------------------------------------------------------------------------------------------------------
constexpr uint32_t GRID_MAX_DIMS = 7; // dimensions a grid encodes: the hash has seven primes (common_device.h:633)
struct GridLevel {
	uint32_t offset;      // first entry of the level (in entries, grid.h:714)
	uint32_t size;        // hashmap_size = entries in the level
	float    scale;       // grid_scale(level) (common_device.h:709-714)
	uint32_t hashed;      // 1: index = hash(cell) ; 0: index = sum cell_d * stride[d]   (common_device.h:690-707)
	uint32_t stride[GRID_MAX_DIMS]; // per-dim stride of the dense index INCLUDING the uint32 wrap-around / early-exit behaviour
	uint32_t size_mask;   // size-1 if size is a power of two, else 0 (then a real modulo is used)
	// LDS owner-computes scatter (k_grid_bwd_lds): the level's table is cut into scatter_n_chunks chunks of scatter_per_chunk entries
	uint32_t scatter_per_chunk;
	uint32_t scatter_shift;    // log2(scatter_per_chunk) if it is a power of two, else 0xffffffff
	uint32_t scatter_n_chunks;
	uint32_t scatter_binned;   // 1: too many chunks for the sample filter -- the level's gradients go through k_grid_bin.hip
};

struct GridMeta {
	uint32_t n_pos_dims;
	uint32_t n_features_per_level;
	uint32_t n_levels;
	uint32_t grid_type;
	uint32_t hash_type;
	uint32_t interpolation;
	uint32_t primes[GRID_MAX_DIMS];
	GridLevel levels[MAX_N_LEVELS];
};

// input matrix addressing: element (dim d, sample i) at data[i * stride_sample + d * stride_dim]
struct MatView {
	const float* data;
	uint32_t stride_sample;
	uint32_t stride_dim;
};
struct MatViewMut {
	float* data;
	uint32_t stride_sample;
	uint32_t stride_dim;
};

// half data travels as void* on the host side
// chunk_mask (optional, uint64 [n_levels][n][GRID_FILTER_MAX_CHUNKS / 64]): bit c set <=> the sample touches scatter chunk c of that level (filter for k_grid_scatter)
void grid_forward(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32, uint32_t n, MatView x, const void* grid, void* out, uint32_t out_stride, float* dy_dx,
                  uint64_t* chunk_mask);
// ---- 5, 6 and 7 dimensions (k_grid_nd.hip): the same three passes in the rolled kernel form; grid_forward, grid_backward and
// grid_backward_backward_input hand such grids on to these
void grid_nd_forward(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32, uint32_t n, MatView x, const void* grid, void* out, uint32_t out_stride, float* dy_dx,
                     uint64_t* chunk_mask);
void grid_nd_backward(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32_grad, uint32_t n, MatView x, const void* dL_dy, bool dy_fp32, uint32_t dy_stride, void* grad,
                      bool stochastic);
// (the grid and the input term; dL_ddLdy has no corner loop and keeps k_grid_bwdbwd_dLdoutput)
void grid_nd_backward_backward_input(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32, bool fp32_grad, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy,
                                     uint32_t dy_stride, const void* grid, void* grad, MatViewMut* dL_dx);
// ---- training-step forward (k_grid_planes.hip): half, F >= 2, D in {2, 3}; level-major and XCD-aware.
// out_planes: half [n_levels][n][F]; chunk_bits (optional): uint64 [n_levels][GRID_FILTER_MAX_CHUNKS][n / 64], written for levels with 2 .. GRID_FILTER_MAX_CHUNKS scatter chunks.
bool grid_planes_supported(const GridMeta& meta, uint32_t n);
bool grid_planes_to_rows_supported(const GridMeta& meta, uint32_t n, uint32_t width);
// planes [width / F][n][F] -> the first `width` columns of rows [n][row_stride] and back (halves; the callers that want the encoded batch as a
// matrix, k_grid_planes.hip; width: the levels' features, or the padded width with its planes of zeros)
void grid_planes_to_rows(hipStream_t stream, const GridMeta& meta, uint32_t n, uint32_t width, const void* planes, void* rows, uint32_t row_stride);
void grid_rows_to_planes(hipStream_t stream, const GridMeta& meta, uint32_t n, uint32_t width, const void* rows, uint32_t row_stride, void* planes);
uint32_t grid_planes_spt(const GridMeta& meta);        // samples per thread of the kernel shape used for this grid
void grid_planes_plan(const GridMeta& meta, uint32_t n, bool hit_lists, std::vector<uint32_t>& work, uint32_t& max_items, uint32_t& blocks_per_xcd); // hit_lists: the shape of the kernel that writes them (larger work items)
// prep_job (optional, mlp_side_jobs.h; passed to the kernel by value): the kernel also builds the MLP's fragment images
struct MlpPrepJob;
// ---- hit lists (round 4; round 5: elements that carry their entries and weights, gradients transposed into list order).
// The scatter's sample filter as a STREAM instead of bit planes to be scanned.  For every level cut into 2 .. GRID_FILTER_MAX_CHUNKS chunks
// the forward kernel writes, per work item (grid_hit_item_samples() consecutive samples of one level), the item's elements SORTED BY
// CHUNK into the item's own region of the level's pool, plus 65 offsets: where each chunk's run starts inside the region ([64]: how
// many elements the item has).  An element is one CELL ROW of one sample -- the two corners that differ in dimension 0 only -- and
// carries everything the chunk's owner needs but the gradient:
//     elems [..][0]: entry of corner A (cell_0) | entry of corner B (cell_0 + 1) << 16, both relative to the chunk's first entry;
//     elems [..][1]: (half) weight of A | (half) weight of B << 16 -- the fp32 products of grid.h:147-160 rounded to half, as grid.h:254 uses them
//                    (no corner B here -- Nearest interpolation, or B lies in another chunk --: A's entry again with weight +0, so that
//                    the owner adds both corners of every element without a test: a product with +0 adds nothing);
//     sidx  [..]   : the sample, relative to the item's first one (16 bits).
// After the MLP kernel a streaming pass (k_grid_list_gradients, k_grid_scatter_lists.hip) brings dL/dy into the same order: per item it
// loads the item's slice of the level's gradient plane into LDS (2 KB) and writes gvals [..] = dL/dy of element's sample, position
// for position (where a workgroup of the fused MLP kernel produces exactly one item -- GridItemMap below -- that kernel's tail does this
// itself and the pass is not launched: GridListTail).  The chunk's owner then walks the items' runs of its chunk reading elems and gvals side by side -- dense loads, no
// gather, no coordinates, no pos_fract, no hash.  (Round 4: 4-byte elements {sample, corner bits}; the owner gathered a 16-byte record
// per element from a 4 MB plane per level pair.  Each such gather costs the CU a whole 128-byte line from its L2, ~3 clocks per lane
// whatever the bytes used -- 40 us of the kernel's 59 - 66 at 2^18 samples, profiles/r05_scatter_timeline.txt -- and needs the plane
// resident in the XCD's L2, which tied the form to batches of 2^17 .. 2^19.)  No counters, no atomics: a region's place is the item's
// number.  The one exception: a row whose two corners fall into different chunks (one in ~8000 on hashed levels) sends corner B to the
// level's straggler list {sample | corner bit << grid_hit_mask_shift, chunk}, which every owner of the level scans and evaluates from the coordinates.
inline constexpr uint32_t grid_hit_mask_shift(uint32_t n_pos_dims) { return 32u - (1u << n_pos_dims); } // 28 (2-D), 24 (3-D): stragglers only
constexpr uint32_t GRID_HIT_COUNT_STRIDE = 64;   // uint32 per level between the straggler counts (one memory channel each)
constexpr uint32_t GRID_HIT_HEADS = 65;          // offsets per item: GRID_FILTER_MAX_CHUNKS + 1
constexpr uint32_t GRID_HIT_WORDS = 2;           // uint32 per element
// Which samples form work item j: n_windows runs of `window` consecutive samples, `stride` samples apart --
//     position p of item j (p = s * window + t, t < window) is sample j * window + t + s * stride.
// {item_samples, 0, 1}: item_samples consecutive samples.  {256, grid * 256, trips}: exactly the samples workgroup j of k_mlp_train_r32
// works on (it deals 32-sample blocks out block-cyclically), so that the kernel's tail can bring its own dL/dy into list order
// (GridListTail).  `window` is a power of two and a multiple of what one wave of the forward kernel covers: every run a wave loads or
// stores stays dense.  Every kernel that turns (item, position) into a sample goes through grid_item_sample().
struct GridItemMap {
	uint32_t window = 0, window_shift = 0, stride = 0, n_windows = 0;
	bool operator==(const GridItemMap& o) const { return window == o.window && window_shift == o.window_shift && stride == o.stride && n_windows == o.n_windows; }
};
inline GridItemMap grid_item_map(uint32_t window, uint32_t stride, uint32_t n_windows) {
	GridItemMap m;
	m.window = window, m.stride = stride, m.n_windows = n_windows;
	while ((1u << m.window_shift) < window) ++m.window_shift;
	return m;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t grid_item_sample(const GridItemMap& m, uint32_t item, uint32_t pos) { return (item << m.window_shift) + (pos & (m.window - 1u)) + (pos >> m.window_shift) * m.stride; }
struct GridHitLists {
	uint32_t* elems = nullptr;       // [n_levels][n_items][item_capacity][GRID_HIT_WORDS]
	uint16_t* sidx = nullptr;        // [n_levels][n_items][item_capacity]
	uint32_t* heads = nullptr;       // [n_levels][GRID_HIT_HEADS][n_items]: chunk-major, so that an owner reads its chunk's offsets of consecutive items with dense loads
	uint32_t* stragglers = nullptr;  // [n_levels][straggler_capacity][2]: {sample | corner bit, chunk}
	uint32_t* counts = nullptr;      // [n_levels][GRID_HIT_COUNT_STRIDE]: stragglers per level; all zero when the forward kernel starts
	uint32_t* zero_counts = nullptr; // the counter set of the NEXT forward launch on this stream: zeroed by this one
	uint32_t n_items = 0, item_samples = 0, item_capacity = 0, straggler_capacity = 0;
	GridItemMap map;                 // the samples of an item (item_samples = map.window * map.n_windows)
	uint32_t dev_flags = 0;          // laboratory build only (TCNN_AMD_FWD_LISTS_DEV): timing-only variants of the list output
};
// What the tail of k_mlp_train_r32 needs to store the dL/dy it has just written in list order itself (the work of k_grid_list_gradients):
// workgroup j's samples are item j's (lists.map), F = 2, plain level planes.  level_mask: bit l set <=> level l is listed.
struct GridListTail {
	const uint16_t* sidx = nullptr;
	const uint32_t* heads = nullptr;
	void* gvals = nullptr;           // [n_levels][n_items][item_capacity] half2; nullptr: no tail
	uint32_t n_items = 0, item_capacity = 0, n_levels = 0, level_mask = 0;
	GridItemMap map;
};
uint32_t grid_hit_item_samples(const GridMeta& meta); // samples per work item of the forward kernel shape used for this grid (k_grid_planes.hip)
// the kernels address the pool (12 bytes x 2^(D-1) rows per sample and level) and the straggler masks with 32 bits
inline uint32_t grid_hit_max_samples(const GridMeta& meta) { return meta.n_pos_dims <= 2 ? (1u << 24) : (1u << 22); }
// hit_lists (optional, instead of chunk_bits): see above
void grid_forward_planes(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, const uint32_t* dev_work, uint32_t max_items, uint32_t blocks_per_xcd, uint32_t n,
                         MatView x, const void* grid, void* out_planes, uint64_t* chunk_bits, const MlpPrepJob* prep_job = nullptr, const GridHitLists* hit_lists = nullptr);
// reference-shaped gradient scatter with global float atomics (fp32 grids, F == 1, tables too large for the LDS scheme).
// grad: T[n_params] accumulated in place (caller zeroes it).  For F == 1 && !fp32 the caller passes an fp32 scratch as `grad`.
// stochastic (here and in the other gradient launchers): GridBackwardRoute::stochastic -- dL/dy itself onto the one corner drawn per (sample, level)
void grid_backward(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32_grad, uint32_t n, MatView x, const void* dL_dy, bool dy_fp32, uint32_t dy_stride, void* grad,
                   bool stochastic = false);

// ---- LDS owner-computes scatter (k_grid_scatter.hip): exact 64-bit fixed-point accumulation, one task per workgroup
struct GridScatterTask {
	uint32_t level;
	uint32_t entry_begin, n_entries;      // owned chunk of the level's table (n_entries == 0: padding task)
	uint32_t sample_begin, sample_end;    // samples examined by this task
	uint32_t flush_atomic;                // 1: several tasks share the chunk -> merge into the scratch table, finalize rounds
	uint32_t scratch_begin;               // first element of the chunk inside the scratch table (shared chunks only)
	uint32_t pad;
};
struct GridScatterRange { size_t grad_begin; uint32_t n_elems; uint32_t scratch_begin; uint32_t pad; }; // shared chunks, for the finalize pass
struct MlpReduceJob;                                // mlp_side_jobs.h
constexpr uint32_t GRID_FILTER_MAX_CHUNKS = 64;     // chunks per level the sample filter can describe (bit planes per level)
uint32_t grid_scatter_max_chunks();                 // = GRID_FILTER_MAX_CHUNKS
void grid_scatter_setup_levels(GridMeta& meta);     // fills GridLevel::scatter_* (how each level's table is cut into chunks)
bool grid_scatter_prefers_lists(const GridMeta& meta); // the grid has levels of many chunks: hit lists (k_grid_scatter_lists.hip) instead of bit planes
// Plans the task list for a batch of n samples (half gradients, F >= 2).
// measured_level_us (optional): per-level workgroup time of a first launch (grid_scatter_level_costs) -> tuned task sizes
void grid_scatter_plan(const GridMeta& meta, uint32_t n, std::vector<GridScatterTask>& tasks, std::vector<GridScatterRange>& shared_ranges, size_t& scratch_elems,
                       const std::vector<float>* measured_level_us = nullptr);
// times: uint64[tasks.size()][8] copied back from grid_backward_lds(task_times)
std::vector<float> grid_scatter_level_costs(const GridMeta& meta, const std::vector<GridScatterTask>& tasks, const std::vector<uint64_t>& times);
// chunk_mask [n_levels][n][GRID_FILTER_MAX_CHUNKS / 64] uint64 -> chunk_bits [n_levels][GRID_FILTER_MAX_CHUNKS][n / 64] uint64 (one ballot word per 64 samples per (level, chunk))
void grid_mask_to_bits(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, uint32_t n, const uint64_t* chunk_mask, uint64_t* chunk_bits);
// dL_dy element (sample i, level l, feature f) at dL_dy[i * dy_stride_sample + l * dy_stride_level + f].
// chunk_bits: optional filter derived from grid_forward's masks for the SAME batch (n samples); nullptr -> every sample is examined in full.
// scratch: uint64[scratch_elems], zero on entry, zero again on return.  Writes EVERY gradient element (no memset needed);
// accumulate = GradientMode::Accumulate.  Returns whether reduce_job was carried (by the finalize launch, when there is one).
bool grid_backward_lds(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, const GridScatterTask* dev_tasks, uint32_t n_tasks,
                       const GridScatterRange* dev_ranges, uint32_t n_ranges, uint64_t* scratch, uint32_t n, MatView x,
                       const void* dL_dy, uint32_t dy_stride_sample, uint32_t dy_stride_level, void* grad, const uint64_t* chunk_bits, bool accumulate, bool dy_records = false,
                       uint64_t* task_times = nullptr, // task_times (optional): device uint64[n_tasks][8], per-task timestamps for the plan tuner
                       const MlpReduceJob* reduce_job = nullptr, bool stochastic = false); // stochastic: not with dy_records
// ---- the same scatter fed by hit lists (k_grid_scatter_lists.hip): two workgroups per CU with 64 KiB of accumulators each -- both features
// of an entry in ONE 64-bit LDS add as 2 x int32 while a per-task bound proves that no half can overflow, 64-bit accumulators in two
// passes otherwise -- tasks of its own plan (GridScatterTask::pad = split s | n_splits << 16: which share of a chunk's list), same scratch, same results.
uint32_t grid_scatter_lists_lds_bytes();
// the kernel's tasks in launch order (one workgroup each; block b runs on XCD b % 8: k_grid_scatter_lists.hip)
void grid_scatter_lists_plan(const GridMeta& meta, uint32_t n, std::vector<GridScatterTask>& tasks, std::vector<GridScatterRange>& shared_ranges, size_t& scratch_elems);
bool grid_backward_lists(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, const GridScatterTask* dev_tasks, uint32_t n_tasks,
                         const GridScatterRange* dev_ranges, uint32_t n_ranges, uint64_t* scratch, uint32_t n, MatView x,
                         const void* dL_dy, uint32_t dy_stride_sample, uint32_t dy_stride_level, void* grad, const GridHitLists& lists, void* gvals, bool accumulate,
                         const MlpReduceJob* reduce_job, uint32_t* fallback_count = nullptr, bool gvals_filled = false);
// gvals: workspace of grid_list_gradients_bytes(): dL/dy in list order, half [n_levels][n_items][item_capacity][F], written by the launch's first
// kernel -- or, gvals_filled, by the MLP kernel's tail already (GridListTail): that first kernel is then not launched
size_t grid_list_gradients_bytes(const GridMeta& meta, const GridHitLists& lists);
// the finalize pass of the shared chunks (+ the MLP's slab reduction), shared by both scatter kernels; false: no ranges, nothing was launched
bool grid_scatter_finalize(hipStream_t stream, const GridScatterRange* dev_ranges, uint32_t n_ranges, uint64_t* scratch, void* grad, bool accumulate, const MlpReduceJob* reduce_job);
// dy_records: dL_dy is float4 [grid_scatter_record_planes()][n] scatter records {coordinates, gradient halves} (mlp_device.h
// store_dx_record; D = 2 with F = 2 packs two levels into one record); x is then not read
bool grid_scatter_records_supported(const GridMeta& meta);
uint32_t grid_scatter_record_planes(const GridMeta& meta);

// ---- The grid encoding's two routes: how a batch is produced and how its parameter gradients are accumulated, each decided ONCE per pass by
// a pure host function (no GPU call, no environment, no switches(): the Switches set is an argument).  The forward route is kept in the
// EncodingContext and the backward route FOLLOWS IT, whatever the process-wide switches say by the time the backward pass runs.
struct GridFacts { // what a GridEncoding knows from its construction (and its padding) on
	const GridMeta* meta;
	bool fp32, scatter_levels_ok, any_binned; // levels_ok: every level is cut into at most GRID_FILTER_MAX_CHUNKS chunks or binned (k_grid_bin.hip)
	uint32_t n_to_pad;                        // padding features behind the levels'
	bool stochastic = false;                  // the config's stochastic_interpolation (grid.h:284-298; what it changes: grid_stochastic_gradients)
};
// The parameter-gradient pass puts every (sample, level)'s dL/dy on ONE corner drawn per pair, with weight 1.  Nearest returns before the
// flag is read (grid.h:279-282): such a grid is a plain Nearest grid on every route.
inline bool grid_stochastic_gradients(const GridFacts& g) { return g.stochastic && g.meta->interpolation != (uint32_t)InterpolationType::Nearest; }
enum class GridForwardKernel : uint32_t { Rows, Planes, PlanesToRows }; // k_grid_fwd (AoS); k_grid_fwd_planes; the latter + a transposition into rows
enum class GridRecorded : uint32_t { Nothing, BitPlanes, HitLists };    // what the forward pass leaves for the gradient kernel
struct GridForwardRoute {
	bool planned = false; // false: a default-constructed context -- its backward route is planned from the switches of that moment
	GridForwardKernel kernel = GridForwardKernel::Rows;
	GridRecorded recorded = GridRecorded::Nothing;
	bool lds = false;            // a later backward pass with parameter gradients runs the LDS owner-computes kernels, else the global-atomic one
	uint32_t plane_features = 0; // Planes: the encoded batch is level planes [padded / F][n][F] of this F
};
// half precision, F >= 2, every level's table cut into at most 64 chunks (the sample filter) or binned; TCNN_AMD_GRID_SCATTER=atomic: never
inline bool grid_lds_gradients(const GridFacts& g, const Switches& sw, uint32_t n) {
	return !g.fp32 && g.meta->n_features_per_level >= 2 && sw.grid_scatter_lds && g.scatter_levels_ok && n % 64 == 0;
}
// Hit lists instead of bit planes: TCNN_AMD_SCATTER_LISTS=0 never, =1 wherever the kernel can take the grid (tests), unset where it pays
inline bool grid_hit_lists_wanted(const GridFacts& g, const Switches& sw, uint32_t n) {
	const GridMeta& meta = *g.meta;
	if (sw.scatter_lists == 0) return false;
	if (g.any_binned || n > grid_hit_max_samples(meta) || meta.n_pos_dims > 3 || meta.hash_type == (uint32_t)HashType::Rng) return false; // (Rng: its hash is a loop)
	if (sw.scatter_lists == 1) return true;
	// Where it pays (DESIGN.md "Batch sizes", "Away from the BASELINE configurations"; profiles/r05_sweep.txt, r05_shape_sweep.txt): grids with
	// levels of many chunks, at every batch size; below 2^16 samples a 2-D grid's bit planes are level with the lists or ahead, in 3-D they lose everywhere
	if (meta.n_pos_dims == 2 && n < (1u << 16)) return false;
	return grid_scatter_prefers_lists(meta);
}
// as_planes: the caller takes the encoded batch as level planes where the grid can write them (the fused step, fused inference), else it
// wants the matrix [n][padded].  The plane kernel writes no dy_dx: input gradients keep the AoS kernel.
inline GridForwardRoute grid_forward_route(const GridFacts& g, const Switches& sw, uint32_t n, bool as_planes, bool input_gradients, bool param_gradients) {
	const GridMeta& meta = *g.meta;
	const uint32_t F = meta.n_features_per_level;
	GridForwardRoute r;
	r.planned = true;
	r.lds = grid_lds_gradients(g, sw, n);
	// (a padded encoding -- 12 levels x 2 features in front of a 16-aligned network -- has whole planes of zeros behind its levels' planes)
	const bool planes = !input_gradients && !g.fp32 && sw.grid_planes && g.n_to_pad % F == 0 && grid_planes_supported(meta, n);
	if (planes && as_planes) r.kernel = GridForwardKernel::Planes;
	else if (planes && sw.grid_rows_planes && grid_planes_to_rows_supported(meta, n, meta.n_levels * F + g.n_to_pad)) r.kernel = GridForwardKernel::PlanesToRows;
	if (r.kernel == GridForwardKernel::Planes) r.plane_features = F;
	// (a stochastic grid never records hit lists: their elements carry all 2^D corners with their weights.  Bit planes stay a valid filter --
	// the drawn corner is one of the corners whose chunks were recorded)
	const bool lists = r.kernel != GridForwardKernel::Rows && !grid_stochastic_gradients(g) && grid_hit_lists_wanted(g, sw, n);
	if (param_gradients && r.lds) r.recorded = lists ? GridRecorded::HitLists : GridRecorded::BitPlanes;
	return r;
}

enum class GridDyForm : uint32_t { Rows, Planes, Records }; // dL/dy as [n][padded]; level planes [padded / F][n][F]; 16-byte records {coordinates, gradients}
enum class GridGradientKernel : uint32_t { None, Atomic, AtomicScratch32, BitPlanes, Lists }; // BitPlanes: k_grid_scatter (unfiltered where nothing was recorded)
enum class GridMaxLevel : uint32_t { None, Scalar, PerSample };                               // the max_level state when the backward pass runs
struct GridBackwardRoute { // the default: dL/dy as rows, nothing else -- every encoding but the grid
	GridDyForm dy = GridDyForm::Rows;
	uint32_t plane_features = 0, record_planes = 0; // Planes, Records: the F of [padded / F][n][F]; Records: 16-byte records per sample (grid_scatter_record_planes)
	GridGradientKernel kernel = GridGradientKernel::None;
	// binned: k_grid_bin.hip follows for the levels cut into more than 64 chunks; tune: the bit-plane kernel's plan may be re-cut from a timed launch
	// (TCNN_AMD_SCATTER_TUNE); prologue: the finalize pass may be left to the optimizer's launch where that offers it (AdamPrologue)
	bool binned = false, tune = false, prologue = false;
	bool stochastic = false; // every gradient kernel of this pass puts dL/dy on the one corner drawn per (sample, level) (grid_stochastic_gradients); never with Lists, Records or tail
	// the fused MLP kernel's tail may store dL/dy in list order itself where its workgroups' samples are the lists' items (mlp_train_item_map() ==
	// list_tail.map): what it needs for that, all but gvals -- the caller's workspace of tail_bytes, handed back as BackwardHandoff::list_gradients
	bool tail = false;
	GridListTail list_tail;
	size_t tail_bytes = 0;
};
// fwd, lists_current: the context's forward route, and whether its hit lists are still their stream's latest (GridEncoding::lists_current)
// offer: the richest form the caller can deliver dL/dy in -- Rows (a caller's own network), Planes (the unfused network kernels), Records (the fused step)
inline GridBackwardRoute grid_backward_route(const GridFacts& g, const Switches& sw, const GridForwardRoute& fwd, bool lists_current, uint32_t n, GridDyForm offer, bool want_dL_dx,
                                             GradientMode mode, GridMaxLevel max_level, bool x_contiguous) {
	const GridMeta& meta = *g.meta;
	const uint32_t F = meta.n_features_per_level;
	GridBackwardRoute r;
	if (mode == GradientMode::Ignore) return r;
	r.stochastic = grid_stochastic_gradients(g);
	if (!(fwd.planned ? fwd.lds : grid_lds_gradients(g, sw, n))) { // the reference-shaped kernel; half with F == 1 accumulates in fp32 (grid.h:660)
		r.kernel = (!g.fp32 && F == 1) ? GridGradientKernel::AtomicScratch32 : GridGradientKernel::Atomic;
		return r;
	}
	// LDS owner-computes scatter with exact integer accumulation.  Stale lists (a later forward pass took their counters): the unfiltered bit-plane kernel.
	const bool lists = fwd.recorded == GridRecorded::HitLists && lists_current && !r.stochastic;
	r.kernel = lists ? GridGradientKernel::Lists : GridGradientKernel::BitPlanes;
	r.binned = !lists && g.any_binned;
	r.tune = !lists && sw.scatter_tune;
	// (not under a scalar cut-off: the off levels' gradients are settled after the kernels, and the optimizer's own launch sees every parameter)
	r.prologue = max_level != GridMaxLevel::Scalar && !g.any_binned;
	if (offer == GridDyForm::Rows || want_dL_dx) return r;
	r.dy = GridDyForm::Planes, r.plane_features = F;
	// Scatter records: the MLP kernel interleaves the coordinates with dL/d(encoding) and the scatter does one gather per hit instead of two (C3a: the scatter gains
	// 12 us, the MLP kernel loses 6 to 4x the dX bytes).  Not with hit lists, current or stale (their elements carry entries and weights), nor with a per-sample max_level.
	// Nor for a stochastic grid: its owners read dL/dy as planes beside the coordinates -- one kernel form less for a pass nobody has tuned yet.
	if (offer == GridDyForm::Records && !r.stochastic && fwd.recorded != GridRecorded::HitLists && g.n_to_pad == 0 && max_level != GridMaxLevel::PerSample && sw.scatter_records && !g.any_binned &&
	    grid_scatter_records_supported(meta) && x_contiguous) {
		r.dy = GridDyForm::Records, r.record_planes = grid_scatter_record_planes(meta);
		return r;
	}
	// (a max_level cut-off masks or settles gradients around the kernels: k_grid_list_gradients as a pass of its own then)
	r.tail = offer == GridDyForm::Records && lists && F == 2 && max_level == GridMaxLevel::None && sw.listgrad_in_mlp && meta.n_levels <= 16 &&
	         (grid_hit_item_samples(meta) << (meta.n_pos_dims - 1)) <= 2048;
	if (r.tail) {
		r.list_tail.n_levels = meta.n_levels;
		for (uint32_t l = 0; l < meta.n_levels; ++l) {
			const GridLevel& lv = meta.levels[l];
			if (lv.scatter_n_chunks > 1 && lv.scatter_n_chunks <= GRID_FILTER_MAX_CHUNKS && !lv.scatter_binned) r.list_tail.level_mask |= 1u << l;
		}
	}
	return r;
}

// ---- PPNG1 (k_ppng.hip; encodings/ppng_1.h): features half [F][2][3][C][Q][R]; out / dL_dy AoS with row stride out_stride;
// scratch: uint64[n_params], zero on entry, zero again on return (exact integer sums of the fp16 products, rounded once)
void ppng1_forward(hipStream_t stream, bool fp32_out, uint32_t n, uint32_t F, uint32_t Q, uint32_t C, uint32_t R, int32_t log2_min_freq, int32_t log2_max_freq, MatView x,
                   const void* features, void* out, uint32_t out_stride);
void ppng1_backward(hipStream_t stream, bool fp32_dy, uint32_t n, uint32_t F, uint32_t Q, uint32_t C, uint32_t R, int32_t log2_min_freq, int32_t log2_max_freq, MatView x,
                    const void* features, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad, bool accumulate);

// PPNG2 (encodings/ppng_2.h): features half [F][2][3][C][Q][Q][R], otherwise as PPNG1
void ppng2_forward(hipStream_t stream, bool fp32_out, uint32_t n, uint32_t F, uint32_t Q, uint32_t C, uint32_t R, int32_t log2_min_freq, int32_t log2_max_freq, MatView x,
                   const void* features, void* out, uint32_t out_stride);
void ppng2_backward(hipStream_t stream, bool fp32_dy, uint32_t n, uint32_t F, uint32_t Q, uint32_t C, uint32_t R, int32_t log2_min_freq, int32_t log2_max_freq, MatView x,
                    const void* features, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad, bool accumulate);
// PPNG3 (encodings/ppng_3.h): features half [F][2][Q^3][C] (cell = p_0 + Q p_1 + Q^2 p_2), C in {2, 4, 8}; dL_dx is written (not accumulated)
void ppng3_forward(hipStream_t stream, bool fp32_out, uint32_t n, uint32_t F, uint32_t Q, uint32_t C, int32_t log2_min_freq, int32_t log2_max_freq, MatView x, const void* features, void* out,
                   uint32_t out_stride);
size_t ppng3_backward_workspace_bytes(uint32_t n, uint32_t F, uint32_t Q, uint32_t C); // the third coordinate's bins of every (f, s, sample); 0 when the layers do not fit the LDS
void ppng3_backward(hipStream_t stream, bool fp32_dy, uint32_t n, uint32_t F, uint32_t Q, uint32_t C, int32_t log2_min_freq, int32_t log2_max_freq, MatView x, const void* dL_dy,
                    uint32_t dy_stride, void* workspace, uint64_t* scratch, void* grad, bool accumulate);
void ppng3_backward_input(hipStream_t stream, bool fp32_dy, uint32_t n, uint32_t F, uint32_t Q, uint32_t C, int32_t log2_min_freq, int32_t log2_max_freq, MatView x, const void* features,
                          const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx);
// second order (ppng_3.h:609-676): grad (nullable; scratch as above), dL_ddLdy (nullable, [n][dy_stride]) and dL_dx (nullable, written)
void ppng3_backward_backward_input(hipStream_t stream, bool fp32_dy, uint32_t n, uint32_t F, uint32_t Q, uint32_t C, int32_t log2_min_freq, int32_t log2_max_freq, MatView x, MatView dL_ddLdx,
                                   const void* features, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad, bool accumulate, void* dL_ddLdy, MatViewMut* dL_dx);

// ---- binned form for levels cut into more than 64 chunks (k_grid_bin.hip; GridLevel::scatter_binned): no filter, no gathers.
// Same exact result as grid_backward_lds; writes every gradient element of the binned levels.  workspace: grid_bin_workspace_bytes().
bool grid_bin_supported(const GridMeta& meta); // F in {2, 4}
uint32_t grid_bin_max_chunks();                // chunks per level (4096)
uint32_t grid_bin_acc_bytes();                 // LDS accumulators per workgroup = chunk size of binned levels
size_t grid_bin_workspace_bytes(const GridMeta& meta, uint32_t n);
void grid_backward_binned(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, uint32_t n, MatView x, const void* dL_dy, uint32_t dy_stride_sample,
                          uint32_t dy_stride_level, void* grad, bool accumulate, void* workspace,
                          uint32_t* fallback_count = nullptr, // (optional, device) chunks whose packed 32-bit sums could not be proven and were added again in 64 bits
                          bool stochastic = false);
void grid_backward_input(hipStream_t stream, const GridMeta& meta, bool fp32, uint32_t n, const void* dL_dy, uint32_t dy_stride, const float* dy_dx, MatViewMut dL_dx);
// second-order input gradients (k_grid_bwdbwd.hip; grid.h:352-650): each of grad (accumulated in place, GT = float if fp32_grad),
// dL_ddLdy (T [n][dy_stride], needs dy_dx) and dL_dx (overwritten, needs grid) is optional
void grid_backward_backward_input(hipStream_t stream, const GridMeta& meta, const GridMeta* dev_meta, bool fp32, bool fp32_grad, uint32_t n, MatView x, MatView dL_ddLdx, const void* dL_dy,
                                  uint32_t dy_stride, const void* grid, const float* dy_dx, void* grad, void* dL_ddLdy, MatViewMut* dL_dx);

// OneBlob / Identity (AoS output, T = half or float)
void oneblob_forward(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_bins, MatView x, void* out, uint32_t out_stride);
void oneblob_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_bins, MatView x, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx);
// the tangent J v (k_encodings.hip k_oneblob_tangent): t[i][d * n_bins + b] = (T)(v[i][d] * k'), k' the fp32 derivative of bin b that
// oneblob_backward_input multiplies dL_dy by -- one rounding; exactly zero in the padding columns
void oneblob_tangent(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_bins, MatView x, MatView v, void* t, uint32_t t_stride);
void identity_forward(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, float scale, float offset, MatView x, void* out, uint32_t out_stride);
void identity_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, float scale, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx);
// second order: dL_ddLdy[i][j] = (T)(dL_ddLdx[i][j] * scale) for j < n_dims, 0 for the padding
void identity_backward_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, float scale, MatView dL_ddLdx, void* dL_ddLdy, uint32_t dy_stride);
// Frequency / TriangleWave (k_encodings.hip): dy_dx (optional) float [n][n_dims * outputs_per_input], consumed by the backward pass
void periodic_forward(hipStream_t stream, bool triangle, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_frequencies, MatView x, void* out, uint32_t out_stride, float* dy_dx);
void periodic_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t n_dims, uint32_t outputs_per_input, const void* dL_dy, uint32_t dy_stride, const float* dy_dx, MatViewMut dL_dx);
// second-order pass: dL_ddLdy [n][dy_stride] T = J dL_ddLdx (zero in the padding) and / or dL_dx (Frequency: the Hessian term, read from x and dL_dy,
// not from dy_dx; TriangleWave has none and writes no dL_dx); a null result is not computed
void periodic_backward_backward_input(hipStream_t stream, bool triangle, bool fp32, uint32_t n, uint32_t n_dims, uint32_t n_frequencies, MatView x, MatView dL_ddLdx, const void* dL_dy,
                                       void* dL_ddLdy, uint32_t dy_stride, MatViewMut* dL_dx);
// Composite encoding reductions (composite.h:47-133): `in` holds the nested outputs [n_nested][n_elems], T = float if fp32 else half
void composite_reduce_forward(hipStream_t stream, bool fp32, bool product, size_t n_elems, uint32_t n_nested, const void* in, void* out);
void composite_reduce_backward(hipStream_t stream, bool fp32, bool product, size_t n_elems, uint32_t n_nested, const void* in, const void* dL_dout, void* dL_din);
// Product, second order: from the nested values, their tangents [n_nested][n_elems] and dL_dout to dL_ddLdout [n_elems] and q [n_nested][n_elems] (either may be null)
void composite_reduce_backward_backward(hipStream_t stream, bool fp32, size_t n_elems, uint32_t n_nested, const void* in, const void* tangents, const void* dL_dout, void* dL_ddLdout, void* q);
// SphericalHarmonics: degree^2 outputs, the padding columns FIRST (spherical_harmonics.h:58-64)
void sh_forward(hipStream_t stream, bool fp32, uint32_t n, uint32_t degree, MatView x, void* out, uint32_t out_stride);
void sh_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t degree, MatView x, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx);
void sh_backward_backward_input(hipStream_t stream, bool fp32, uint32_t n, uint32_t degree, MatView x, MatView dL_ddLdx, const void* dL_dy, void* dL_ddLdy, uint32_t dy_stride, MatViewMut* dL_dx);

// ------------------------------------------------------------------------------------------------------------------
// Fully fused MLP.  Weight matrices are row-major [fan_out][fan_in] half, contiguous (fully_fused_mlp.cu:656-671).
// The kernels consume "fragment images": the weights pre-permuted into MFMA A-operand order (see k_mlp.hip).
// ------------------------------------------------------------------------------------------------------------------
struct MlpLayer {
	uint32_t rows, cols;    // fan_out, fan_in
	uint32_t w_off;         // element offset of the matrix inside the parameter vector
	uint32_t fwd_off;       // first fragment of the forward image (A = W)
	uint32_t bwd_off;       // first fragment of the backward image (A = W^T)
	uint32_t ks_fwd;        // k-steps (of 32) of the forward product = ceil(cols / 32)
	uint32_t ks_bwd;        // k-steps of the backward product = ceil(rows / 32)
	uint32_t natural_k;     // 1: forward fragments use natural k order (layer 0, B operand loaded from memory)
};

struct MlpDesc {
	uint32_t in_width, width, out_width, n_hidden, n_layers;
	uint32_t activation, output_activation;
	uint32_t n_frags_fwd, n_frags_bwd;
	uint32_t n_frags_r32;   // third section of the image: fragments for v_mfma_f32_32x32x16_f16 (k_train_r32.hip; mlp_side_jobs.h R32Frags), 0: none
	MlpLayer layers[MAX_MLP_LAYERS];
};

size_t mlp_image_bytes(const MlpDesc& d);   // bytes of the fwd + bwd (+ r32) images
// params (half, row-major matrices) -> images.  image = [fwd frags][bwd frags], 1 KiB per fragment.
void mlp_prepare_weights(hipStream_t stream, const MlpDesc& d, const void* params, void* image, bool want_bwd);
// x: [n][in_width] half AoS; out: [n][out_width] half; hidden (optional): [n_hidden][n][width] half post-activation
void mlp_forward(hipStream_t stream, const MlpDesc& d, const void* image, uint32_t n, const void* x, void* out, void* hidden);
// The same kernel with its input / output conversions fused in (inference path):
//   input : x_half AoS [n][in_width], or level planes [in_width / F][n][F] (x_plane_features = F), or -- x_f32.data != nullptr --
//           the float matrix itself with the Identity encoding applied on the fly ((half)(x * scale + offset), padding = 1), or
//           with the OneBlob encoding applied on the fly (x_oneblob_bins);
//   output: out_half [n][out_width] and / or out_f32: the first out_f32_dims outputs as floats (trim_and_cast, object.cu:61-67).
struct MlpIo {
	const void* x_half;
	uint32_t x_plane_features;
	MatView x_f32;
	uint32_t x_f32_dims;
	float x_scale, x_offset;
	uint32_t x_oneblob_bins; // > 0 (a power of two >= 32): x_f32 holds coordinates and the network's input is their OneBlob encoding, evaluated in the kernel
	void* out_half;
	MatViewMut out_f32;
	uint32_t out_f32_dims;
};
void mlp_forward_io(hipStream_t stream, const MlpDesc& d, const void* image, uint32_t n, const MlpIo& io, void* hidden);
// Reference-shaped backward: dL_dout [n][out_width]; hidden from mlp_forward; writes dhidden [n_hidden][n][width] and (optional) dL_dx [n][in_width]
// dx_plane_features = 0: dL_dx is AoS [n][in_width]; = F > 0: "level planes" [in_width / F][n][F] (what the grid scatter reads)
void mlp_backward(hipStream_t stream, const MlpDesc& d, const void* image, uint32_t n, const void* dL_dout, const void* out, const void* hidden, void* dhidden, void* dL_dx,
                  uint32_t dx_plane_features);
// ---- input_gradient (object.h:342-366): d output[dim] / d (network input) at inference.  One kernel (k_mlp_input_grad.hip) runs the forward
// chain, keeps every hidden layer's halves in registers, seeds backprop_scale on row `dim` and runs the backward chain: bit for bit what
// mlp_forward (hidden stored) + mlp_activation_backward_output + mlp_backward give for a one-hot dL/dy, without the stored activations and
// the dhidden nobody reads.  Which instantiation, with its NB and grid, or the two passes: decided once per call by mlp_input_gradient_plan.
constexpr uint32_t MLP_INPUT_GRAD_MAX_HIDDEN = 4; // depths 1 .. 4 are instantiated
struct MlpInputGradPlan {
	bool fused = false;          // false: forward + backward (name "two-pass")
	char name[48] = "two-pass";  // the route's name (tcnn_module_last_input_gradient_route): "two-pass" | "k_mlp_input_grad<W,NB,NH>/relu|act" (mlp_input_jacobian_plan: k_mlp_input_jacobian<...>)
	uint32_t nb = 0, grid = 0;   // fused: column blocks of 16 samples per wave and trip, workgroups of 4 waves
	bool relu = false;           // fused: the compiled ReLU form, else the activation chosen at run time
};
// Pure host code: no GPU call, no allocation, no environment.  layerwise: Network::layerwise() -- fp32, Sine, zero hidden layers, widths the
// fused kernels do not cover, TCNN_AMD_MLP_LAYERWISE=1 when the network was created.  Two-pass also for depths and widths without an
// instantiation (256), for n that is no multiple of 16 NB, and for 128 x (3 | 4) ReLU on a full machine, where the fused kernel measured no
// faster (DESIGN.md "input_gradient").
MlpInputGradPlan mlp_input_gradient_plan(const MlpDesc& d, bool layerwise, uint32_t n);
// io: the network's input as mlp_forward_io takes it (rows, level planes or the fused Identity input; no OneBlob) and, optionally, out_half;
// dL_dx half [n][in_width] or level planes (dx_plane_features), as mlp_backward writes it; dim < d.out_width; plan.fused must hold for (d, n)
void mlp_input_gradient(hipStream_t stream, const MlpDesc& d, const MlpInputGradPlan& plan, const void* image, uint32_t n, const MlpIo& io, uint32_t dim, float backprop_scale,
                        void* dL_dx, uint32_t dx_plane_features);
// ---- input_jacobian: input_gradient for K output columns d_0 .. d_{K-1} from ONE forward chain (k_mlp_input_jacobian.hip): buffer k is bit
// for bit what mlp_input_gradient(dim = d_k) writes.  The dims travel in the kernel's arguments, MLP_INPUT_JACOBIAN_MAX_DIMS per launch; more
// dims run as further launches, each with a forward chain of its own.
constexpr uint32_t MLP_INPUT_JACOBIAN_MAX_DIMS = 16;
// Pure host code, as mlp_input_gradient_plan: "two-pass" (one forward pass, n_dims backward passes) or "k_mlp_input_jacobian<W,NB,NH>/relu|act".
// The rule: fused where the half-precision fused kernels exist -- not layerwise, fragment images present, 16 / 32 / 64 / 128 wide, 1 .. 4
// hidden layers, n a multiple of 16 NB (NB = 2 at 128 wide, else 4) -- except in the classes where it measured no faster than the Jacobian's
// own two passes by more than 3 % (DESIGN.md "input_jacobian"):
//   - a run-time activation (anything but ReLU) with more than 256 workgroups (n / (64 NB)) and n_dims above the class's limit --
//     16 wide: none for 1 .. 3 hidden layers, 0 for 4 (never fused); 32 wide: none for 1 | 2, 1 for 3, 0 for 4; 64 wide: 3 for 1, else 2;
//     128 wide: 2 for 1, else 1;
//   - ReLU, 128 wide, 2 hidden layers, n >= 2^20, n_dims > 8.
// mlp_input_gradient_plan's exception (128 wide, ReLU, 3 | 4 hidden layers, full machine) is not carried over: it rests on a kernel whose
// forward chain was not shared, and this one measured 1.14 to 1.21 there at 3 dims.
MlpInputGradPlan mlp_input_jacobian_plan(const MlpDesc& d, bool layerwise, uint32_t n, uint32_t n_dims);
// io as for mlp_input_gradient; dims: n_dims host values < d.out_width; dL_dx: n_dims buffers one behind the other, each half [n][in_width] or
// level planes (dx_plane_features); the output (io.out_half, optional) is stored once
void mlp_input_jacobian(hipStream_t stream, const MlpDesc& d, const MlpInputGradPlan& plan, const void* image, uint32_t n, const MlpIo& io, const uint32_t* dims, uint32_t n_dims,
                        float backprop_scale, void* dL_dx, uint32_t dx_plane_features);
// ---- input_jvp: J(x) v for every output column along T input directions, forward mode (k_mlp_input_jvp.hip).  The network's part: from its
// input rows and T tangent buffers u_0 (one behind the other, each half [n][in_width]) to T buffers u_K (each half [n][out_width]), with
// u_k = a_k' (.) half(W_k u_{k-1}): the accumulator starts at +0, the k-steps ascend, one rounding to half per layer, a' in fp32 from the half
// pre-activation (the sign of the half output for ReLU / LeakyReLU).  One wave owns 16 NB samples; per layer every weight fragment is read
// once and feeds the forward product and the products of TT tangent chains; nothing but the live operands is kept across layers.  More
// tangents than TT are further launches, each with a forward chain of its own; the output is stored by the first.
constexpr uint32_t MLP_INPUT_JVP_MAX_TT = 3; // tangent chains per launch: TT = 1 and TT = 3 are instantiated
struct MlpInputJvpPlan {
	bool fused = false;          // false: the layer-by-layer passes (name "two-pass")
	char name[48] = "two-pass";  // tcnn_module_last_input_jvp_route: "two-pass" | "k_mlp_input_jvp<W,NB,NH,TT>/relu|act"
	uint32_t nb = 0, grid = 0;   // fused: column blocks of 16 samples per wave and trip, workgroups of 4 waves
	uint32_t tt = 0;             // fused: tangent chains per launch
	bool relu = false;           // fused: the compiled ReLU form, else the activation chosen at run time
};
// Pure host code, as the two plans above.  Layer-by-layer networks (fp32, Sine, zero hidden layers, widths and depths without an
// instantiation, TCNN_AMD_MLP_LAYERWISE=1) are always "two-pass", and so is n that is no multiple of 16 NB.  A fused class gets the kernel
// only where tools/bench_input_jvp.py measured it faster than this call's own two-pass route by more than 3 %, the spread between boxes:
// measured in every class -- ReLU | run-time form x 16 / 32 / 64 / 128 wide x 1 .. 4 hidden layers x TT = 1 | 3, at 2^18 and 2^14 rows --
// the two passes take 1.31 to 9.85 times the kernel's time, so every instantiated class is fused (DESIGN.md "input_jvp / The plan rule";
// profiles/input_jvp_bench.txt, section 2).  TT = 1 for one tangent, else 3; NB = nb_of's, halved for TT = 3 at 64 and 128 wide.
MlpInputJvpPlan mlp_input_jvp_plan(const MlpDesc& d, bool layerwise, uint32_t n, uint32_t n_tangents);
// io: the network's input as mlp_input_gradient takes it (rows, level planes or the fused Identity input) and, optionally, out_half.
// tangents: n_tangents buffers of half [n][in_width] rows one behind the other, or -- tangents_f32.data != nullptr -- the caller's float
// [n][n_tangents][x_f32_dims] with the Identity encoding's tangent applied in the load: (half)(v * io.x_scale), ZERO in the padding.
// jvp: half, tangent t of sample s at jvp[s * jvp_stride + t * out_width] (jvp_stride = out_width times the tangents of the whole call, of
// which this may be a group).  plan.fused must hold for (d, n).
void mlp_input_jvp(hipStream_t stream, const MlpDesc& d, const MlpInputJvpPlan& plan, const void* image, uint32_t n, const MlpIo& io, const void* tangents, MatView tangents_f32,
                   uint32_t n_tangents, void* jvp, uint32_t jvp_stride);
// ---- input_jvp_backward: the reverse of input_jvp (parameter, input and tangent gradients of L = sum_t <dL_djvp_t, J v_t> + <dL_doutput, f>).
// The plan has MlpInputJvpPlan's shape, so that a fused kernel "k_mlp_input_jvp_bwd<W,NB,NH,TT>/relu|act" can enter a class here once
// tools/bench_input_jvp_backward.py has measured it faster than the composed route by more than 3 %.  No such kernel is built yet: every
// class is "two-pass" -- the composed route of the existing second-order and first-order passes (DESIGN.md "Training through input_jvp").
struct MlpInputJvpBackwardPlan {
	bool fused = false;          // false: the composed route (name "two-pass")
	char name[48] = "two-pass";  // tcnn_module_last_input_jvp_backward_route
	uint32_t nb = 0, grid = 0;   // fused: column blocks of 16 samples per wave and trip, workgroups of 4 waves
	uint32_t tt = 0;             // fused: tangent chains per launch
	bool relu = false;           // fused: the compiled ReLU form, else the activation chosen at run time
};
// Pure host code, a pure function of its arguments.  NetworkWithInputEncoding::input_jvp_backward_impl asks it per call and reports its name.
inline MlpInputJvpBackwardPlan mlp_input_jvp_backward_plan(const MlpDesc& d, bool layerwise, uint32_t n, uint32_t n_tangents) {
	(void)d; (void)layerwise; (void)n; (void)n_tangents;
	return MlpInputJvpBackwardPlan{};
}
// the two ends of every input_gradient route (object.h:352-365): d_doutput [n][width] T = (T)backprop_scale in column dim, +0 elsewhere;
// d_dinput[i][j] *= mult for j < dims (mult = 1.0f / backprop_scale, formed once by the caller)
void input_gradient_one_hot(hipStream_t stream, Precision precision, uint32_t n, uint32_t width, uint32_t dim, float backprop_scale, void* d_doutput);
void input_gradient_rescale(hipStream_t stream, uint32_t n, uint32_t dims, float mult, MatViewMut d_dinput);
// ---- the Trainer's fused step: forward + loss + backward + weight gradients in ONE kernel, one of about twenty (k_train.hip: LDS images,
// any 64- / 128-wide network with <= 32 outputs; k_train_regs.hip: (16 | 32) -> 64 -> [64 ->] 16 with everything in registers;
// k_train_r32{,a}.hip, k_train_r32ob.hip, k_train_r32w.hip: BASELINE configs 3, 2 and 5 on the 32x32x16 matrix instruction).  Which one runs
// and over how many workgroups is decided ONCE per step, by mlp_train_plan, from a request that holds everything the choice depends on;
// the caller sizes the weight-gradient slabs with the plan's grid and hands the same plan to mlp_train_launch, which decides nothing.
struct MlpTrainRequest {
	uint32_t n = 0;
	// the network's input: half AoS [n][in_width] (both 0), level planes [in_width / F][n][F] (x_plane_features = F in {2, 4, 8}), or the
	// OneBlob encoding of oneblob_dims coordinates per sample evaluated inside the kernel (oneblob_bins > 0, a power of two >= 32)
	uint32_t x_plane_features = 0, oneblob_bins = 0, oneblob_dims = 0;
	uint32_t dims = 0;               // live outputs: columns of target / data_pdf
	LossType loss = LossType::L2;    // unused with external_dL_dy
	bool external_dL_dy = false;     // dL/dy [n][out_width] half (loss-scaled) comes from the caller: no target, no loss, dL_dout and L not written
	bool data_pdf = false;
	bool out = false;                // the network's output [n][out_width] is written
	// dL/d(input): none; AoS [n][in_width] (dx_plane_features = 0); level planes of F features; or -- dx_record_dims = k > 0, with planes --
	// 16-byte scatter records {k coordinates (floats, read from dx_record_x [n][k]), gradient halves}, float4 [in_width / F][n] or, for
	// 2 dims and F = 2, [in_width / 4][n] with two levels per record (mlp_device.h store_dx_record; needs 4 k + 2 F <= 16)
	bool dL_dx = false;
	uint32_t dx_plane_features = 0, dx_record_dims = 0;
	bool gradients = false;          // weight gradients: one fp32 slab of partial sums per workgroup, slabs [plan.grid][n_params]
	bool compact_context = false;    // dL_dout and L are the COMPACT matrices [n][dims] (mlp_expand_context pads them), else [n][out_width]
};
enum class MlpTrainKernel : uint32_t { None, R32ob, R32w, R32, R32a, Regs, Train }; // Regs: "regs_fast" | "regs"; Train: the k_train.hip table
struct MlpTrainPlan {
	bool ok = false;                 // false: no fused kernel takes this request (name says nothing then)
	MlpTrainKernel kernel = MlpTrainKernel::None;
	// the kernel's short name, a static string (Trainer::last_step_kernel): "r32", "r32a", "r32w", "r32ob", "regs_fast", "regs",
	// "train<W,NB,NW,MAXT>/relu|act", "train_regw|train_ob/relu|act" (act: the activation chosen at run time)
	const char* name = "";
	uint32_t grid = 0;               // workgroups of the launch = weight-gradient slabs
	MlpTrainRequest request;
	// what the chosen kernel's launch needs besides:
	struct Config { int nb, nw, maxt; uint32_t lds_bytes, s; bool ok, image_in_lds, regw; } config{}; // Train: the instance of k_mlp_train (regw: weight fragments in registers)
	int regs_in_tiles = 0, regs_hidden = 0; // Regs: the instance's input tiles of 16 and hidden layers
	bool regs_fast = false;          // Regs: compile-time formats
	bool r32ob_shared = false;       // R32ob: shared weight-gradient tiles, else per-wave accumulators
};
// Pure host code: no GPU call, no allocation, no look at the environment (laboratory knobs aside): the plan depends on its arguments and
// on the process switches (one copy, switches(), taken when called -- once per step) alone.
MlpTrainPlan mlp_train_plan(const MlpDesc& d, const MlpTrainRequest& request);
struct MlpTrainArgs {
	const void* image = nullptr;                           // the network's fragment images
	const void* x = nullptr;                               // the network's input (not with OneBlob)
	MatView oneblob_x{};                                   // with OneBlob: the coordinates [n][oneblob_dims], any layout
	const float *target = nullptr, *data_pdf = nullptr;    // [n][dims]
	const void* external_dL_dy = nullptr;
	float loss_scale = 1.0f;
	void *out = nullptr, *dL_dout = nullptr, *dL_dx = nullptr;
	float *L = nullptr, *slabs = nullptr;
	const float* dx_record_x = nullptr;
	uint32_t n_params = 0;                                 // floats per slab
	const GridListTail* list_tail = nullptr;               // the kernel also stores dL_dx in the grid's list order (mlp_train_item_map() must hold for the plan)
};
// The item map under which workgroup j of plan's kernel produces exactly item j's dL/dx (k_mlp_train_r32 with plain level planes, every
// wave the same number of trips); false: this plan has none.
bool mlp_train_item_map(const MlpTrainPlan& plan, GridItemMap& map);
// launches plan.grid workgroups of plan's kernel; args must be what plan.request describes (checked)
void mlp_train_launch(hipStream_t stream, const MlpDesc& d, const MlpTrainPlan& plan, const MlpTrainArgs& args);
// what a caller asks before it knows the whole request -- the kernels' own predicates, as mlp_train_plan applies them:
bool mlp_train_any_kernel(const MlpDesc& d, uint32_t n);                          // some fused kernel takes batches of n samples
bool mlp_train_oneblob_in_kernel(const MlpDesc& d, uint32_t n, uint32_t n_bins);  // one of them evaluates a OneBlob encoding of n_bins bins itself
bool mlp_train_compact_context(const MlpDesc& d, uint32_t n);                     // the kernel for (d, n) with weight gradients writes compact context matrices
void mlp_expand_context(hipStream_t stream, uint32_t n, uint32_t dims, const void* compact_dL_dout, const float* compact_L, void* dL_dout, float* L);
// grad[i] (=|+=) sum_k slabs[k][i], fixed order, rounded to half once
// adam (optional, not with accumulate): the optimizer's update of these (matrix) weights is applied behind the reduction, bit-identical to adam_step run afterwards
struct AdamInReduce;
void mlp_reduce_slabs(hipStream_t stream, uint32_t n_params, uint32_t n_slabs, const float* slabs, void* grad_half, bool accumulate, const AdamInReduce* adam = nullptr);
// dW[rows x cols] = sum_i dO[i][rows]^T In[i][cols]; result written as half into grad (overwrite or accumulate). workspace: float[wgrad_workspace_floats()]
size_t wgrad_workspace_floats(uint32_t rows, uint32_t cols, uint32_t n);
// several such products over the same n samples (a network's layers): same results as one mlp_wgrad() each, fewer launches
// (dO_tiled / In_tiled: the operand is a hidden layer's stored activations or gradients in k_mlp_fwd / k_mlp_bwd's tiled form, ld = the full
// width of that matrix and a panel's first column c0 absorbed by the pointer as + (c0 / 16) * 256 halves; k_mlp.hip hidden_tile_off)
// Fp32 (k_mlp_layers_f32.hip): row-major float operands into float grad, panels of at most 128 x 128, never tiled: fp32 slabs summed in a fixed order
struct WgradPanel { const void* dO; uint32_t ldo, rows; const void* In; uint32_t ldi, cols; void* grad; uint32_t ldg; bool dO_tiled, In_tiled; };
size_t wgrad_panels_workspace_floats(Precision precision, const WgradPanel* panels, uint32_t count, uint32_t n);
void mlp_wgrad_panels(hipStream_t stream, Precision precision, uint32_t n, const WgradPanel* panels, uint32_t count, bool accumulate, float* workspace);
void mlp_wgrad(hipStream_t stream, uint32_t n, const void* dO, uint32_t ldo, uint32_t rows, const void* In, uint32_t ldi, uint32_t cols,
               void* grad_half, uint32_t ldg, bool accumulate, float* workspace);
// ---- the layer-by-layer path (k_mlp_layers.hip; Network::layerwise): one GEMM per layer on row-major matrices of `precision` (T below:
// half, or float with the weights read from the fp32 parameter vector as they are), n % 256 == 0, rows / cols multiples of 16, the leading
// dimension of x a whole 16-byte piece (8 halfs, 4 floats), that of y a multiple of 4.  Fp16: the fp32 accumulator is rounded to half, then
// the activation is applied.  Fp32: every product is one ascending-k fmaf chain per element from +0 (the contract at LayerElem<float> in
// that file) and (T) is no rounding at all.
// forward: y[s][r] = act((T) sum_c x[s][c] w[r][c]) for r < rows; w [rows][cols]; pre (optional): the pre-activation, laid out as y
void mlp_layer_forward(hipStream_t stream, Precision precision, uint32_t n, const void* x, uint32_t ldx, const void* w, uint32_t rows, uint32_t cols, uint32_t activation, void* y,
                       uint32_t ldy, void* pre);
// backward data: dL_din[s][c] = act'((T) sum_r dL_dout[s][r] w[r][c]) for c < cols, from wt = w^T [cols][rows] (mlp_layer_transpose);
// aux (laid out as dL_din): the forward output of the layer that produced the input -- its pre-activation for Sine; activation None: unused
void mlp_layer_backward(hipStream_t stream, Precision precision, uint32_t n, const void* dL_dout, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols, uint32_t activation,
                        const void* aux, void* dL_din, uint32_t ldi);
void mlp_layer_transpose(hipStream_t stream, Precision precision, uint32_t rows, uint32_t cols, const void* w, void* wt); // wt [cols][rows] = w [rows][cols]^T
// ---- the three products of the second-order pass (Network::second_order_begin / _finish).  a', a'' are evaluated in fp32 from aux: the
// layer's pre-activation, or its output for ReLU / LeakyReLU; unused for None.  One rounding to T per stored matrix.
// tangent: acc = sum_c u_in[s][c] w[r][c];  u_out = a'(aux) acc;  r_out (optional, needs g) = a''(aux) g acc.  aux, g, u_out, r_out: [n][ldy]
void mlp_layer_tangent(hipStream_t stream, Precision precision, uint32_t n, const void* u_in, uint32_t ldu, const void* w, uint32_t rows, uint32_t cols, uint32_t activation,
                       const void* aux, const void* g, void* u_out, void* r_out, uint32_t ldy);
// backward data, keeping the gradient from before the derivative: acc = sum_r d_out[s][r] w[r][c] (from wt);  g_in (optional) = (T) acc;
// d_in = a'(aux) g_in.  aux, g_in, d_in: [n][ldi]
void mlp_layer_backward_keep(hipStream_t stream, Precision precision, uint32_t n, const void* d_out, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols, uint32_t activation,
                             const void* aux, void* g_in, void* d_in, uint32_t ldi);
// curvature: acc = sum_r p_out[s][r] w[r][c] (from wt);  p_in = r_in + a'(aux) acc (r_in optional: zero; p_in may be r_in).  [n][ldi]
void mlp_layer_curvature_backward(hipStream_t stream, Precision precision, uint32_t n, const void* p_out, uint32_t ldo, const void* wt, uint32_t rows, uint32_t cols,
                                  uint32_t activation, const void* aux, const void* r_in, void* p_in, uint32_t ldi);
void mlp_layer_delta(hipStream_t stream, Precision precision, size_t n_elems, uint32_t activation, const void* g, const void* aux, void* delta); // delta = a'(aux) g, element by element
// fully_fused_mlp.cu:757-762: result = dL_dout * act'(out), element by element, from the forward OUTPUT values (fused networks too)
void mlp_activation_backward_output(hipStream_t stream, Precision precision, size_t n_elems, uint32_t activation, const void* dL_dout, const void* out, void* result);
void add_input_gradient(hipStream_t stream, uint32_t n, uint32_t dims, MatView src, MatViewMut dst);                                           // dst += src, [n][dims] floats

// ------------------------------------------------------------------------------------------------------------------
// loss / reduction / optimizer / init plumbing
// ------------------------------------------------------------------------------------------------------------------
void loss_evaluate(hipStream_t stream, LossType type, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale,
                   const void* pred_half, const float* target, float* values, void* grads_half, const float* data_pdf, Precision precision = Precision::Fp16);
// sum of n floats -> *result_dev (device float, overwritten). workspace-free: uses a two-stage reduction through `partials` (>= 1024 floats)
void reduce_sum(hipStream_t stream, size_t n, const float* values, float* partials, float* result_dev);
// reduce_sum's second stage alone: the sum of n_partials floats, in k_reduce_stage2's order, for kernels that write their own partials
void reduce_partials(hipStream_t stream, uint32_t n_partials, const float* partials, float* result_dev);

// Loss evaluation on caller-owned predictions (k_loss_eval.hip): every element is loss_element (loss_device.h), as in loss_evaluate.
// Each output is optional (NULL) and has its own row stride; columns >= dims of an output row are written as zeros.
constexpr uint32_t LOSS_EVAL_MAX_BLOCKS = 1024; // the fixed grid's bound = the number of floats `partials` must hold
struct LossEvalRequest {
	LossType type = LossType::L2;
	Precision precision = Precision::Fp16; // of prediction and gradients
	uint32_t n = 0, dims = 0;
	float loss_scale = 1.0f;
	const float* scale_dev = nullptr; // device, optional: one more fp32 factor of the gradient, multiplied in before its one rounding
	const void* prediction = nullptr; // [n][prediction_stride], unit column stride
	uint32_t prediction_stride = 0;
	const float* target = nullptr;    // compact [n][dims]
	const float* data_pdf = nullptr;  // compact [n][dims], optional
	float* values = nullptr;          // [n][values_stride]
	uint32_t values_stride = 0;
	void* gradients = nullptr;        // [n][gradients_stride], in the prediction's type
	uint32_t gradients_stride = 0;
	float* loss_sum = nullptr;        // device: the sum of all values, reduced in a fixed order without storing them
	float* partials = nullptr;        // with loss_sum: LOSS_EVAL_MAX_BLOCKS floats of workspace
};
// the arguments are the caller's to check (model.h: loss_evaluate_on_predictions); launches one kernel, and k_reduce_stage2 for loss_sum
void loss_eval_launch(hipStream_t stream, const LossEvalRequest& r);

struct AdamHyper {
	float learning_rate = 1e-3f, beta1 = 0.9f, beta2 = 0.999f, epsilon = 1e-8f, l2_reg = 1e-8f;
	float relative_decay = 0.0f, absolute_decay = 0.0f, clipping_magnitude = 0.0f, non_matrix_learning_rate_factor = 1.0f;
	bool adabound = false, optimize_matrix_params = true, optimize_non_matrix_params = true;
};
// kernel-side form of the hyperparameters of one step (k_misc.hip make_adam_args)
struct AdamArgs {
	float relative_weight_decay, absolute_weight_decay, weight_clipping_magnitude, loss_scale, learning_rate, non_matrix_learning_rate_factor;
	float beta1, beta2, epsilon, lower_lr_bound, upper_lr_bound, l2_reg;
	uint32_t optimize_matrix_params, optimize_non_matrix_params;
	float inv_loss_scale;
	uint32_t inv_loss_scale_exact;
	uint32_t common_step; // the optimizer's own step count: the per-parameter count of every parameter that was updated in every step
};
AdamArgs make_adam_args(const AdamHyper& h, float loss_scale, uint32_t current_step);
// The optimizer's update carried by the slab reduction (k_wgrad_reduce_adam, k_mlp.hip): a matrix weight's gradient is final the moment
// its slabs are summed, so adam.h:48-119 runs on it at once.  Arrays are indexed like the gradient array the kernel writes.
constexpr uint32_t IMAGE_INV_WIDTH = 4; // a weight sits in at most 4 image elements: forward and transposed fragments of the 16x16x32 and of the 32x32x16 sections
struct AdamInReduce {
	AdamArgs args;
	float* w_fp = nullptr;
	void* w_half = nullptr;
	float* m1 = nullptr;
	float* m2 = nullptr;
	void* steps = nullptr; // uint32, or uint16 if steps16
	uint32_t steps16 = 0;
	const float* debias_table = nullptr;
	// Network::live_image: the network's fragment images and, per parameter, the IMAGE_INV_WIDTH image elements that hold it
	// (0xffffffff: none) -- the kernel writes an updated weight there too, so that the next step needs no k_mlp_prep launch
	void* image = nullptr;
	const uint32_t* image_inv = nullptr;
};
// What the backward pass of a fused step leaves for the optimizer's launch to finish (k_adam_prologue, k_misc.hip): the scatter's finalize
// pass -- the shared chunks' exact sums in `scratch` are rounded into the gradient, the scratch left zero -- and the fixed-order sum of the
// MLP's weight-gradient slabs.  Both are the last writes of the gradients the optimizer reads next: in ONE launch the workgroup that
// finishes a gradient updates its parameters at once, every other workgroup does what k_adam does, and the step has one ~5 us launch
// (k_grid_scatter_finalize) and one kernel boundary less.  Same rounding, same adam_one: gradients, weights, moments, counts bit-identical.
struct AdamPrologue {
	bool pending = false;                      // the backward pass left its finalize pass here instead of launching it
	const GridScatterRange* dev_ranges = nullptr;
	std::vector<GridScatterRange> ranges;      // host copy; grad_begin relative to grad_base
	uint64_t* scratch = nullptr;
	void* grad_base = nullptr;                 // half: the gradient array the ranges index (the encoding's part of the gradient vector)
	bool accumulate = false;
	bool has_reduce = false;
	uint32_t reduce_elems = 0, reduce_slabs = 0; // the MLP's weights (the first reduce_elems parameters) and its slabs
	const float* slabs = nullptr;
	int reduce_accumulate = 0;
};
// adam_step with the prologue in the same launch.  false: the shapes do not allow it (alignment) -- nothing was launched, the caller
// runs grid_scatter_finalize / mlp_reduce_slabs and adam_step itself.
bool adam_step_with_prologue(hipStream_t stream, const AdamHyper& h, size_t n, size_t n_matrix, float loss_scale, uint32_t current_step,
                             float* w_fp, void* w_half, void* g_half, float* m1, float* m2, void* steps, bool steps16, const float* debias_table, const AdamPrologue& p);
// steps: the per-parameter update counts, uint32 or -- steps16 -- uint16 (what the optimizer keeps while every count fits:
// 4 of the 36 bytes per parameter the kernel moves are the counts' upper halves otherwise)
void adam_step(hipStream_t stream, const AdamHyper& h, size_t n, size_t n_matrix, float loss_scale, uint32_t current_step,
               float* w_fp, void* w_half, const void* gradients, float* m1, float* m2, void* steps, bool steps16, const float* debias_table,
               GradientPrecision precision = GradientPrecision::Fp16, Precision weight_precision = Precision::Fp16);
void adam_widen_steps(hipStream_t stream, size_t n, const void* steps16, void* steps32); // uint16 -> uint32
// debias_table[t] = sqrtf(1 - powf(beta2, t)) / (1 - powf(beta1, t)) (adam.h:97-98), evaluated on the device, for t in [from, to)
void adam_fill_debias_table(hipStream_t stream, float beta1, float beta2, uint32_t from, uint32_t to, float* table);
// Test hook (tcnn_adam_math_sweep, tcnn_amd.h): adam_device.h's guarded square root and division against sqrtf and `/`, compared bit for
// bit on the device; nothing is stored per element.  Synchronises.  mismatches: their number; first_bad: the smallest offending input
// (the square root's operand; denominator << 32 | numerator), ~0 if none.
void adam_math_sweep(hipStream_t stream, int what, uint64_t first, uint64_t count, uint32_t n_numerators, float numerator_lo, float numerator_hi, uint64_t seed, uint64_t* mismatches,
                     uint64_t* first_bad);
// dst[i][dst_col + j] = src[i][src_col + j] for j < width; elements of 2 or 4 bytes (Composite encoding)
void copy_columns(hipStream_t stream, size_t elem_bytes, uint32_t n, const void* src, uint32_t src_stride, uint32_t src_col, void* dst, uint32_t dst_stride, uint32_t dst_col, uint32_t width);
// optimizers/sgd.h:44-72 and optimizers/ema.h:44-78 (half parameters; gradients in `precision`, here and below)
void sgd_step(hipStream_t stream, size_t n, float loss_scale, float learning_rate, float l2_reg, float* weights_full_precision, void* weights, const void* gradients,
              GradientPrecision precision = GradientPrecision::Fp16, Precision weight_precision = Precision::Fp16);
// weight_precision Fp32 (here and below): the optimizer's weights are ONE float vector -- weights_full_precision is read and stored, `weights` is
// not touched -- its gradients are fp32, and the buffers an optimizer keeps beside them (EMA, samples, average, lookahead) are floats
void ema_step(hipStream_t stream, size_t n, float decay, float debias_old, float debias_new, const void* weights, void* weights_ema, float* tmp, Precision weight_precision = Precision::Fp16);
// optimizers/average.h:44-60, batched.h:44-61, lookahead.h:44-59 (half parameters)
void average_step(hipStream_t stream, size_t n, uint32_t n_samples, const void* weights, void* current_sample, void* average, Precision weight_precision = Precision::Fp16);
void batched_accumulate(hipStream_t stream, size_t n, bool first, uint32_t multiplier, const void* gradients, float* pool, GradientPrecision precision = GradientPrecision::Fp16);
void lookahead_step(hipStream_t stream, size_t n, float alpha, float* weights_full_precision, void* weights, void* weights_lookahead, Precision weight_precision = Precision::Fp16);
// optimizers/novograd.h:44-94 for ONE layer of n weights: the layer's second moment from the sum of its squared gradients, then the step
void novograd_layer_step(hipStream_t stream, size_t n, float relative_decay, float absolute_decay, float loss_scale, float learning_rate, float beta1, float beta2, float epsilon,
                         float* weights_full_precision, void* weights, const void* gradients, float* first_moments, float* layer_second_moment,
                         GradientPrecision precision = GradientPrecision::Fp16, Precision weight_precision = Precision::Fp16);

// random.h:40-70: strided uniform fill from a pcg32 state; advances (state, inc) on the host copy by n
void generate_random_uniform(hipStream_t stream, uint64_t* state_inc_host, size_t n, float* out, float lower, float upper);
void cast_float_to_half(hipStream_t stream, size_t n, const float* in, void* out);
void cast_half_to_float(hipStream_t stream, size_t n, const void* in, float* out);
// object.cu:61-67: [n][in_stride] T -> float out(dim, sample) = out.data[i*stride_sample + d*stride_dim], d < dims
void trim_and_cast(hipStream_t stream, bool fp32, uint32_t n, uint32_t in_stride, uint32_t dims, const void* in, MatViewMut out);
void fill_half(hipStream_t stream, size_t n, void* out, float value);
// max_level (k_grid_max_level.hip): zeroes the `width` elements at data + i * sample_stride + l * level_stride (2- or 4-byte elements) of every
// (sample i < n, level level0 <= l < n_levels) pair that is off -- all of them without per_sample (the scalar cut-off's suffix), else those
// whose per_sample[i] puts them off by the forward rule (l >= m + 1e-3f) or the gradient rule (l > m + 1e-3f), m = per_sample[i] * n_grid_features / F.
// src (same layout): a masked copy instead -- every pair of every level is written, from src where the pair is on (scalar: l < level0)
void grid_zero_levels(hipStream_t stream, size_t elem_bytes, uint32_t n, uint32_t n_levels, uint32_t level0, uint32_t width, uint64_t sample_stride, uint64_t level_stride,
                      void* data, const void* src, const float* per_sample, uint32_t n_grid_features, uint32_t F, bool gradient_rule);

} // namespace tcnn_amd
