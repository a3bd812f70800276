// k_mlp_layers_f32.hip -- the weight gradients of the layer-by-layer MLP path in full precision (Network{json, Precision::Fp32}; the
// layer products themselves are the fp32 instantiation of k_layer_gemm, k_mlp_layers.hip).  Another algorithm than the half one
// (k_wgrad*, k_mlp.hip), behind the same entry points: mlp_wgrad_panels(stream, Precision::Fp32, ..) ends here.
//
// dW[r][c] = sum_s D[s][r] X[s][c] on row-major float operands (k_wgrad_f32): panels of at most 128 x 128; a workgroup multiplies
// chunks of 32 samples (chunk b, b + grid, ... in ascending order) into an fp32 slab of its own and k_wgrad_reduce_f32 adds the slabs
// in ascending order: no atomics, the same inputs give the same bits; Overwrite stores the sum, Accumulate adds it to what is there.
#include "mlp_device.h"

namespace tcnn_amd {
namespace {

constexpr uint32_t WF_CHUNK = 32;      // samples per staged chunk
constexpr uint32_t WF_MAX = 128;       // a panel is at most WF_MAX x WF_MAX
constexpr uint32_t WF_MAX_SLABS = 256; // workgroups (= slabs) per panel
constexpr uint32_t WF_MAX_JOBS = 16;   // panels per launch
// floats per LDS row of a chunk: = 16 modulo 64, so that the four sample rows of a 16x16x4 operand read fall into four different groups of 16 banks
__host__ __device__ inline uint32_t wf_pitch(const uint32_t width) { return width + ((80u - (width & 63u)) & 63u); }
constexpr uint32_t WF_MAX_PITCH = 144; // wf_pitch(128), the largest for widths up to WF_MAX

struct WgradJobF32 {
	const float* dO; // [n][ldo], the panel's `rows` columns
	const float* In; // [n][ldi], the panel's `cols` columns
	float* slabs;    // [grid][rows][cols]
	float* grad;     // [rows][ldg]
	uint32_t ldo, ldi, ldg, rows, cols;
};
struct WgradJobsF32 { WgradJobF32 job[WF_MAX_JOBS]; };

// blockIdx.y: the panel; blockIdx.x: the slab.  A wave owns tiles wave, wave + 4, ... of the panel's (rows / 16) x (cols / 16) tiles.
__global__ void __launch_bounds__(256) k_wgrad_f32(const uint32_t n, const WgradJobsF32 jobs) {
	__shared__ __attribute__((aligned(16))) float P[WF_CHUNK * WF_MAX_PITCH];
	__shared__ __attribute__((aligned(16))) float Q[WF_CHUNK * WF_MAX_PITCH];
	const float* __restrict__ dO = jobs.job[blockIdx.y].dO;
	const float* __restrict__ In = jobs.job[blockIdx.y].In;
	const uint32_t ldo = jobs.job[blockIdx.y].ldo, ldi = jobs.job[blockIdx.y].ldi;
	const uint32_t rows = jobs.job[blockIdx.y].rows, cols = jobs.job[blockIdx.y].cols;
	const uint32_t rp = wf_pitch(rows), cp = wf_pitch(cols);
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t q = lane >> 4, li = lane & 15;
	const uint32_t tc = cols / 16, n_tiles = (rows / 16) * tc;
	constexpr int TILES = (WF_MAX / 16) * (WF_MAX / 16) / 4; // per wave

	// where this thread's 16-byte pieces of a chunk come from and go to (at most 4 per operand; rows, cols <= WF_MAX)
	const uint32_t pr = rows / 4, pc = cols / 4; // pieces per sample row
	uint32_t p_src[4], p_dst[4], q_src[4], q_dst[4];
#pragma unroll
	for (uint32_t i = 0; i < 4; ++i) {
		const uint32_t p = tid + i * 256;
		const uint32_t sp = p / pr, cpp = (p - sp * pr) * 4, sq = p / pc, cq = (p - sq * pc) * 4;
		p_src[i] = sp * ldo + cpp, p_dst[i] = sp * rp + cpp;
		q_src[i] = sq * ldi + cq, q_dst[i] = sq * cp + cq;
	}
	const uint32_t n_p = WF_CHUNK * pr, n_q = WF_CHUNK * pc;
	f4 pv[4], qv[4];
	auto fetch = [&](const uint32_t ch) {
		const float* d = dO + (size_t)ch * WF_CHUNK * ldo;
		const float* x = In + (size_t)ch * WF_CHUNK * ldi;
#pragma unroll
		for (uint32_t i = 0; i < 4; ++i) {
			if (tid + i * 256 < n_p) pv[i] = *(const f4*)(d + p_src[i]);
			if (tid + i * 256 < n_q) qv[i] = *(const f4*)(x + q_src[i]);
		}
	};

	uint32_t tile_at[TILES]; // 16 ti | 16 tj << 16
	f4 acc[TILES];
#pragma unroll
	for (int u = 0; u < TILES; ++u) {
		const uint32_t t = wave + 4 * u, ti = t / tc, tj = t - ti * tc;
		tile_at[u] = (16 * ti) | ((16 * tj) << 16);
		acc[u] = f4{0, 0, 0, 0};
	}

	const uint32_t n_chunks = n / WF_CHUNK;
	if (blockIdx.x < n_chunks) fetch(blockIdx.x);
	for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
#pragma unroll
		for (uint32_t i = 0; i < 4; ++i) {
			if (tid + i * 256 < n_p) *(f4*)(P + p_dst[i]) = pv[i];
			if (tid + i * 256 < n_q) *(f4*)(Q + q_dst[i]) = qv[i];
		}
		__syncthreads();
		if (ch + gridDim.x < n_chunks) fetch(ch + gridDim.x); // in flight while this chunk is multiplied
		// A[row = l & 15][k = l >> 4] = dO[sample 4 kk + (l >> 4)][16 ti + (l & 15)], B[k][col] = In[the same sample][16 tj + (l & 15)]
#pragma unroll 2
		for (uint32_t kk = 0; kk < WF_CHUNK / 4; ++kk) {
			const uint32_t s = 4 * kk + q;
#pragma unroll
			for (int u = 0; u < TILES; ++u) {
				if (wave + 4 * u >= n_tiles) continue; // wave-uniform
				acc[u] = mfma_f32(P[s * rp + (tile_at[u] & 0xffffu) + li], Q[s * cp + (tile_at[u] >> 16) + li], acc[u]);
			}
		}
		__syncthreads();
	}
	// D[row = 4 (l >> 4) + r][col = l & 15] of tile (ti, tj)
	float* slab = jobs.job[blockIdx.y].slabs + (size_t)blockIdx.x * rows * cols;
#pragma unroll
	for (int u = 0; u < TILES; ++u) {
		if (wave + 4 * u >= n_tiles) continue;
#pragma unroll
		for (int r = 0; r < 4; ++r) slab[(size_t)((tile_at[u] & 0xffffu) + 4 * q + r) * cols + (tile_at[u] >> 16) + li] = acc[u][r];
	}
}

// grad (=|+=) slab 0 + slab 1 + ..., added in that order
__global__ void __launch_bounds__(256) k_wgrad_reduce_f32(const uint32_t n_slabs, const WgradJobsF32 jobs, const int accumulate) {
	const uint32_t rows = jobs.job[blockIdx.y].rows, cols = jobs.job[blockIdx.y].cols, ldg = jobs.job[blockIdx.y].ldg;
	const uint32_t n_elems = rows * cols;
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_elems) return;
	const float* __restrict__ slabs = jobs.job[blockIdx.y].slabs + i;
	float sum = slabs[0];
	for (uint32_t k = 1; k < n_slabs; ++k) sum += slabs[(size_t)k * n_elems];
	const uint32_t r = i / cols, c = i - r * cols;
	float* g = jobs.job[blockIdx.y].grad + (size_t)r * ldg + c;
	*g = accumulate ? *g + sum : sum;
}

inline uint32_t wgrad_grid_f32(const uint32_t n) { return std::max(1u, std::min(n / WF_CHUNK, WF_MAX_SLABS)); }

} // namespace

size_t wgrad_panels_workspace_floats_f32(const WgradPanel* panels, uint32_t count, uint32_t n) {
	size_t total = 0;
	for (uint32_t i = 0; i < count; ++i) total += (size_t)wgrad_grid_f32(n) * panels[i].rows * panels[i].cols;
	return total;
}

void mlp_wgrad_panels_f32(hipStream_t stream, uint32_t n, const WgradPanel* panels, uint32_t count, bool accumulate, float* workspace) {
	CHECK_THROW(n % WF_CHUNK == 0);
	if (n == 0) return;
	const uint32_t grid = wgrad_grid_f32(n);
	size_t at = 0;
	for (uint32_t i = 0; i < count; i += WF_MAX_JOBS) {
		WgradJobsF32 jobs{};
		const uint32_t n_jobs = std::min(WF_MAX_JOBS, count - i);
		uint32_t max_elems = 0;
		for (uint32_t j = 0; j < n_jobs; ++j) {
			const WgradPanel& p = panels[i + j];
			CHECK_THROW(p.rows % 16 == 0 && p.cols % 16 == 0 && p.rows > 0 && p.cols > 0 && p.rows <= WF_MAX && p.cols <= WF_MAX);
			CHECK_THROW(p.ldo % 4 == 0 && p.ldi % 4 == 0 && !p.dO_tiled && !p.In_tiled);
			jobs.job[j] = WgradJobF32{(const float*)p.dO, (const float*)p.In, workspace + at, (float*)p.grad, p.ldo, p.ldi, p.ldg, p.rows, p.cols};
			at += (size_t)grid * p.rows * p.cols;
			max_elems = std::max(max_elems, p.rows * p.cols);
		}
		hipLaunchKernelGGL(k_wgrad_f32, dim3(grid, n_jobs), dim3(256), 0, stream, n, jobs);
		hipLaunchKernelGGL(k_wgrad_reduce_f32, dim3(div_round_up(max_elems, 256u), n_jobs), dim3(256), 0, stream, grid, jobs, accumulate ? 1 : 0);
		HIP_CHECK_THROW(hipGetLastError());
	}
}

} // namespace tcnn_amd
