// k_tensorf.hip -- the TensoRF factorisations: ONE resolution per level and many components F (2 .. 32) per factor.
//   VM, 3-D: mode k = 0, 1, 2 is the plane over the axis pair (0,1), (0,2), (1,2) -- KPlanes' pair order -- times the line over the remaining
//            axis 2, 1, 0:  y[l 3F + k F + f] = (T)(P_k[f] * V_k[f]).  Modes are concatenated, not summed.
//   CP, 2- to 4-D: one line per axis:  y[l F + f] = (T)(V_0[f] * V_1[f] * ... * V_{D-1}[f]), left to right.
// Parameters per level: the 3 planes [k][entries][F], entries = next_multiple(R^2, 8), then the lines [k][next_multiple(R, 8)][F] (CP: lines only).
//
// Cell and fraction: pos_fract, Linear.  A plane value P[f] is KPlanes' fp32 fmaf chain over the four corners (bit 0: +1 along a, stride 1;
// bit 1: +1 along b, stride R; weight (x part) * (y part); index in uint32 modulo the entry count).  A line value is
// V[f] = fmaf(w, v1, (1 - w) * v0), entries cell and cell + 1 (uint32) modulo the line's entry count.  Nothing is rounded before the product.
//
// The work splits over COMPONENTS, not levels: the unit of work is a chunk of E = min(F, 16 bytes / sizeof(T)) components of one (level, mode),
// so that a corner is one 16-byte load (F >= 8 in half, >= 4 in float; below that the whole F-wide row, all the layout allows).
//
//   k_tensorf_fwd        one lane per (sample, 16-byte output chunk): consecutive lanes write consecutive chunks of one AoS row, a wave stores
//                        dense rows.  For F below the chunk width a lane holds 16 / (F sizeof(T)) units -- several modes or levels -- and still
//                        stores 16 bytes.  All gathers of a lane are issued first, then the chains; chunks behind the width store ones.
//                        Cell and fraction are recomputed per lane: the lanes of a sample are at different modes and, for small F, levels
//                        (another scale), so only x itself could be shared, and pos_fract is 4 VALU instructions per axis against a
//                        ds_bpermute per value passed by shuffle.
//   k_tensorf_bwd_input  the lookup again from x; W lanes per sample take the chunks j, j + W, ...; each forms its partial dL/dx over its
//                        components, a fixed-order xor butterfly combines them: one store per sample, no atomics, the same bits every run.
//   k_tensorf_bwd        dL/dparams, half: a workgroup owns one (level, component chunk) and a slice of the batch, a lane takes a sample and
//                        walks the modes.  Every contribution is rounded to half and added as 2^-24 fixed point (grid_fixed.h): exact, so
//                        order-independent.  Line accumulators ALWAYS live in LDS -- a line has R entries and every sample of the batch hits
//                        two of them -- and are flushed with one global add per non-zero entry per workgroup.  Plane accumulators share the
//                        LDS with the lines when both fit 64 KB; else the planes take a pass of their own, in LDS when they fit alone and in
//                        the global scratch when not, and the lines take another.  A line too long for the LDS is cut into segments (grid.z).
//   k_tensorf_bwd_f32    fp32 modules: one lane per (sample, level, chunk), float atomicAdd into the gradient (order not fixed).
//
// Second order ("second_order": true), with v = dL_ddLdx, d = dL_dy, vs = scale * v and Q = <v, J^T d>; the interpolation is Linear, so
// d pos / d x = scale and a plane's only second derivative is its mixed one, M = p0 - p1 - p2 + p3.  Each kernel stands beside its
// first-order counterpart and takes its split; none shares a body with it.
//   k_tensorf_tangent       t = J v for a RUN-TIME number of directions: locate, the gathers, the conversions and everything that does not
//                           depend on v (VM: P, V, the slopes daP, dbP, V'; CP: V_i' and the others' products O_i) once per lane, then a
//                           rolled loop over the directions -- load v, a few fused multiply-adds per component, one store.  Padding: zeros.
//                           VM: DP = fmaf(vs_b, dbP, vs_a * daP), t = fmaf(DP, V, P * (V' * vs_c)).  CP: t = sum_i (V_i' * vs_i) O_i, fused, i up.
//   k_tensorf_bwdbwd_input  dQ/dx, W lanes per sample and the butterfly of k_tensorf_bwd_input.  VM, in cells: axis a fmaf(M * vs_b, V,
//                           daP * (V' * vs_c)), axis b fmaf(M * vs_a, V, dbP * (V' * vs_c)), axis c V' * DP, each summed over f by
//                           fmaf(d_f, ., sum), then fmaf(scale, sum, total).  CP: axis i V_i' * D_v O_i, the derivative carried through the
//                           prefix and suffix products (others_tangent): no pair products, no division.
//   k_tensorf_bwdbwd        dQ/dparams, half: k_tensorf_bwd's split, tensorf_plan's passes and accumulators, exact sums.  A plane corner
//                           gets d_f * fmaf(V, D_v w_q, w_q * (V' * vs_c)), a VM line entry d_f * fmaf(DP, w_e, P * (+-vs_c)), a CP line
//                           entry d_f * fmaf(D_v O_i, w_e, O_i * (+-vs_i)).  A lines-only pass gathers the plane corners alone, a
//                           planes-only pass the two line entries.
//   k_tensorf_bwdbwd_f32    the same contributions by float atomicAdd, k_tensorf_bwd_f32's split.
//
// D, F and the decomposition are compile-time; arrays are indexed by unrolled loop variables only and the mode's axes are chosen by
// selects (no scratch, no static LDS).  Compiled with -ffp-contract=off and without packed fp32 instructions (build.py).
#include "grid_fixed.h"

#include <type_traits>

namespace tcnn_amd {
namespace {

typedef TensoRFShape::Levels TensoRFLevels;

constexpr uint32_t TENSORF_LDS_BYTES = 64 * 1024; // accumulators of one workgroup: two workgroups per CU
constexpr uint32_t TENSORF_BWD_SAMPLES = 2048;    // samples per workgroup of k_tensorf_bwd

// the component chunk of type T at F components
template <typename T, int F> struct TensoRFChunk {
	static constexpr int CH = 16 / (int)sizeof(T); // elements of one 16-byte store
	static constexpr int E = F < CH ? F : CH;      // components of one unit of work
	static constexpr int S = CH / E;               // units per forward lane
};

template <typename V> __device__ inline float tensorf_elem(const V& v, int f) { return (float)v[f]; }
__host__ __device__ inline uint32_t tensorf_line_entries(uint32_t R) { return (R + 7u) & ~7u; }
__device__ inline uint32_t tensorf_wrap(uint32_t i, uint32_t size) { return i >= size ? i % size : i; }

// one of three values for a run-time a, by selects (values, not an array: a select between loads would become a load at a selected address)
template <typename V> __device__ inline V tensorf_pick(const V v0, const V v1, const V v2, const uint32_t a) { return a == 0u ? v0 : (a == 1u ? v1 : v2); }

// a sample's cells and fractions at one level, and the level's sizes
template <int D>
struct TensoRFCell {
	float pos[D], scale;
	uint32_t cell[D], R, size, lsize;

	__device__ inline void setup(const float (&x)[D], const TensoRFLevels& lv, const uint32_t level) {
		scale = lv.scale[level];
		R = lv.resolution[level];
		size = lv.entries[level];
		lsize = tensorf_line_entries(R);
#pragma unroll
		for (int d = 0; d < D; ++d) {
			float derivative;
			cell[d] = pos_fract(x[d], scale, (uint32_t)InterpolationType::Linear, &pos[d], &derivative);
		}
	}
};

// One VM unit: E components of mode k.  locate() settles fractions and entries, load() issues the gathers it is asked for.
template <typename T, int F, int E>
struct TensoRFVM {
	typedef typename VecOf<T, E>::type vecE;
	vecE p[4], l[2];
	float pa, pb, pl;
	uint32_t pidx[4], lidx[2];

	__device__ inline void locate(const TensoRFCell<3>& cs, const uint32_t k) {
		const uint32_t a = k == 2u ? 1u : 0u, b = k == 0u ? 1u : 2u, c = 2u - k;
		const float p0 = cs.pos[0], p1 = cs.pos[1], p2 = cs.pos[2];
		const uint32_t c0 = cs.cell[0], c1 = cs.cell[1], c2 = cs.cell[2];
		pa = tensorf_pick(p0, p1, p2, a); pb = tensorf_pick(p0, p1, p2, b); pl = tensorf_pick(p0, p1, p2, c);
		const uint32_t base = tensorf_pick(c0, c1, c2, a) + tensorf_pick(c0, c1, c2, b) * cs.R, lc = tensorf_pick(c0, c1, c2, c);
		if (base < cs.size - cs.R - 1u) { // no corner needs the modulo (KPlanesCell::corners)
			pidx[0] = base; pidx[1] = base + 1u; pidx[2] = base + cs.R; pidx[3] = base + cs.R + 1u;
		} else {
#pragma unroll
			for (int q = 0; q < 4; ++q) pidx[q] = tensorf_wrap(base + (uint32_t)(q & 1) + (uint32_t)(q >> 1) * cs.R, cs.size);
		}
		lidx[0] = tensorf_wrap(lc, cs.lsize);
		lidx[1] = tensorf_wrap(lc + 1u, cs.lsize);
	}
	// table: the level's first parameter; f0: the chunk's first component
	__device__ inline void load(const T* __restrict__ table, const TensoRFCell<3>& cs, const uint32_t k, const uint32_t f0, const bool planes, const bool lines) {
		if (planes) {
#pragma unroll
			for (int q = 0; q < 4; ++q) p[q] = *(const vecE*)&table[((size_t)k * cs.size + pidx[q]) * F + f0];
		}
		if (lines) {
#pragma unroll
			for (int q = 0; q < 2; ++q) l[q] = *(const vecE*)&table[((size_t)3 * cs.size + (size_t)k * cs.lsize + lidx[q]) * F + f0];
		}
	}
	__device__ inline float weight(const int q) const { return ((q & 1) ? pa : 1 - pa) * ((q & 2) ? pb : 1 - pb); }
	__device__ inline void plane_values(float (&P)[E]) const {
#pragma unroll
		for (int f = 0; f < E; ++f) P[f] = 0.0f;
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const float w = weight(q);
#pragma unroll
			for (int f = 0; f < E; ++f) P[f] = fmaf(w, tensorf_elem(p[q], f), P[f]);
		}
	}
	__device__ inline void line_values(float (&V)[E]) const {
		const float w0 = 1 - pl;
#pragma unroll
		for (int f = 0; f < E; ++f) V[f] = fmaf(pl, tensorf_elem(l[1], f), w0 * tensorf_elem(l[0], f));
	}
	// second order: the plane's slopes along a and b (per cell, as k_tensorf_bwd_input forms them) and its mixed derivative; the line's slope
	__device__ inline void plane_slopes(float (&dA)[E], float (&dB)[E], float (&M)[E]) const {
#pragma unroll
		for (int f = 0; f < E; ++f) {
			const float v0 = tensorf_elem(p[0], f), v1 = tensorf_elem(p[1], f), v2 = tensorf_elem(p[2], f), v3 = tensorf_elem(p[3], f);
			M[f] = (v3 - v2) - (v1 - v0);
			dA[f] = fmaf(pb, M[f], v1 - v0);
			dB[f] = fmaf(pa, (v3 - v1) - (v2 - v0), v2 - v0);
		}
	}
	__device__ inline void line_slope(float (&dV)[E]) const {
#pragma unroll
		for (int f = 0; f < E; ++f) dV[f] = tensorf_elem(l[1], f) - tensorf_elem(l[0], f);
	}
	// D_v w_q = vs_a d w_q / d a + vs_b d w_q / d b
	__device__ inline float weight_tangent(const int q, const float vsa, const float vsb) const {
		return fmaf((q & 2) ? vsb : -vsb, (q & 1) ? pa : 1 - pa, ((q & 1) ? vsa : -vsa) * ((q & 2) ? pb : 1 - pb));
	}
};

// vs_a, vs_b, vs_c of mode k from a 3-D direction: scale * v, the axes chosen by selects
__device__ inline void tensorf_mode_direction(const float (&vin)[3], const float scale, const uint32_t k, float& vsa, float& vsb, float& vsc) {
	const uint32_t a = k == 2u ? 1u : 0u, b = k == 0u ? 1u : 2u, c = 2u - k;
	const float s0 = scale * vin[0], s1 = scale * vin[1], s2 = scale * vin[2];
	vsa = tensorf_pick(s0, s1, s2, a); vsb = tensorf_pick(s0, s1, s2, b); vsc = tensorf_pick(s0, s1, s2, c);
}

// One CP unit: E components of all D lines
template <typename T, int D, int F, int E>
struct TensoRFCP {
	typedef typename VecOf<T, E>::type vecE;
	vecE l[D][2];
	uint32_t lidx[D][2];

	__device__ inline void locate(const TensoRFCell<D>& cs) {
#pragma unroll
		for (int d = 0; d < D; ++d) {
			lidx[d][0] = tensorf_wrap(cs.cell[d], cs.lsize);
			lidx[d][1] = tensorf_wrap(cs.cell[d] + 1u, cs.lsize);
		}
	}
	__device__ inline void load(const T* __restrict__ table, const TensoRFCell<D>& cs, const uint32_t f0) {
#pragma unroll
		for (int d = 0; d < D; ++d) {
#pragma unroll
			for (int q = 0; q < 2; ++q) l[d][q] = *(const vecE*)&table[((size_t)d * cs.lsize + lidx[d][q]) * F + f0];
		}
	}
	__device__ inline void line_values(const TensoRFCell<D>& cs, float (&V)[D][E]) const {
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const float w0 = 1 - cs.pos[d];
#pragma unroll
			for (int f = 0; f < E; ++f) V[d][f] = fmaf(cs.pos[d], tensorf_elem(l[d][1], f), w0 * tensorf_elem(l[d][0], f));
		}
	}
	// O[d][f]: the product of the other lines' values (prefix times suffix)
	__device__ static inline void others(const float (&V)[D][E], float (&O)[D][E]) {
#pragma unroll
		for (int f = 0; f < E; ++f) {
			float suffix[D];
			suffix[D - 1] = 1.0f;
#pragma unroll
			for (int d = D - 2; d >= 0; --d) suffix[d] = suffix[d + 1] * V[d + 1][f];
			float prefix = 1.0f;
#pragma unroll
			for (int d = 0; d < D; ++d) {
				O[d][f] = prefix * suffix[d];
				prefix *= V[d][f];
			}
		}
	}
	// second order: the lines' slopes; and O with S[d][f] = D_v O[d][f], from the values and their derivatives Tv along v -- the derivative
	// rides on the same prefix and suffix products (k_kplanes_bwdbwd's scheme)
	__device__ inline void line_slopes(float (&dV)[D][E]) const {
#pragma unroll
		for (int d = 0; d < D; ++d) {
#pragma unroll
			for (int f = 0; f < E; ++f) dV[d][f] = tensorf_elem(l[d][1], f) - tensorf_elem(l[d][0], f);
		}
	}
	__device__ static inline void others_tangent(const float (&V)[D][E], const float (&Tv)[D][E], float (&O)[D][E], float (&S)[D][E]) {
#pragma unroll
		for (int f = 0; f < E; ++f) {
			float suffix[D], dsuffix[D];
			suffix[D - 1] = 1.0f; dsuffix[D - 1] = 0.0f;
#pragma unroll
			for (int d = D - 2; d >= 0; --d) {
				dsuffix[d] = fmaf(dsuffix[d + 1], V[d + 1][f], suffix[d + 1] * Tv[d + 1][f]);
				suffix[d] = suffix[d + 1] * V[d + 1][f];
			}
			float prefix = 1.0f, dprefix = 0.0f;
#pragma unroll
			for (int d = 0; d < D; ++d) {
				O[d][f] = prefix * suffix[d];
				S[d][f] = fmaf(dprefix, suffix[d], prefix * dsuffix[d]);
				dprefix = fmaf(dprefix, V[d][f], prefix * Tv[d][f]);
				prefix *= V[d][f];
			}
		}
	}
};

// E values of dL/dy behind column `col` of a row: one load where the stride keeps it aligned
template <typename T, int E>
__device__ inline void tensorf_load_dy(const T* __restrict__ row, const uint32_t col, const uint32_t dy_stride, float (&g)[E]) {
	typedef typename VecOf<T, E>::type vecE;
	if (dy_stride % E == 0) {
		const vecE gv = *(const vecE*)(row + col);
#pragma unroll
		for (int f = 0; f < E; ++f) g[f] = tensorf_elem(gv, f);
	} else {
#pragma unroll
		for (int f = 0; f < E; ++f) g[f] = (float)row[col + f];
	}
}

// ---------------------------------------------------------------------------------------------------------------- forward
// n_units: n_levels * 3 (VM) or n_levels (CP); n_slots: 16-byte chunks of a row, ceil(out_stride / CH)
template <typename T, bool CP, int D, int F>
__global__ void __launch_bounds__(256) k_tensorf_fwd(const uint32_t n, const uint32_t n_units, const TensoRFLevels lv, const MatView x, const T* __restrict__ params,
                                                     T* __restrict__ out, const uint32_t out_stride, const uint32_t n_slots) {
	typedef TensoRFChunk<T, F> C;
	constexpr int CH = C::CH, E = C::E, S = C::S;
	typedef typename VecOf<T, CH>::type vecCH;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_slots;
	if (i >= n) return;
	const uint32_t j = gid - i * n_slots;
	float xin[D];
	load_coords<D>(x, i, xin);
	float res[CH];
#pragma unroll
	for (int e = 0; e < CH; ++e) res[e] = 1.0f; // units behind the width: the padding
	if constexpr (CP) {
		TensoRFCP<T, D, F, E> u[S];
		TensoRFCell<D> cs[S];
		bool live[S];
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const uint32_t col = j * CH + s * E, level = col / F;
			live[s] = level < n_units;
			if (live[s]) {
				cs[s].setup(xin, lv, level);
				u[s].locate(cs[s]);
				u[s].load(params + (size_t)lv.offset[level] * F, cs[s], col % F);
			}
		}
#pragma unroll
		for (int s = 0; s < S; ++s) {
			if (live[s]) {
				float V[D][E];
				u[s].line_values(cs[s], V);
#pragma unroll
				for (int f = 0; f < E; ++f) {
					float r = V[0][f];
#pragma unroll
					for (int d = 1; d < D; ++d) r *= V[d][f];
					res[s * E + f] = r;
				}
			}
		}
	} else {
		TensoRFVM<T, F, E> u[S];
		bool live[S];
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const uint32_t col = j * CH + s * E, unit = col / F, level = unit / 3u, k = unit - level * 3u;
			live[s] = unit < n_units;
			if (live[s]) {
				TensoRFCell<3> cs;
				cs.setup(xin, lv, level);
				u[s].locate(cs, k);
				u[s].load(params + (size_t)lv.offset[level] * F, cs, k, col % F, true, true);
			}
		}
#pragma unroll
		for (int s = 0; s < S; ++s) {
			if (live[s]) {
				float P[E], V[E];
				u[s].plane_values(P);
				u[s].line_values(V);
#pragma unroll
				for (int f = 0; f < E; ++f) res[s * E + f] = P[f] * V[f];
			}
		}
	}
	T* o = out + (size_t)i * out_stride + (size_t)j * CH;
	if (out_stride % CH == 0) { // rows are 16-byte storable (required_output_alignment); then j * CH + CH <= out_stride
		vecCH w;
#pragma unroll
		for (int e = 0; e < CH; ++e) w[e] = (T)res[e];
		*(vecCH*)o = w;
	} else { // a caller that set its own width (a stand-alone module, a Composite's inner blocks)
#pragma unroll
		for (int e = 0; e < CH; ++e) if (j * CH + e < out_stride) o[e] = (T)res[e];
	}
}

// ---------------------------------------------------------------------------------------------------------------- tangent, n_t directions
// the terms of one unit that do not depend on the direction.  VM: P, V and the slopes daP, dbP, V'; CP: V_d' and the others' products O_d
template <int E> struct TensoRFTangentVM { float P[E], V[E], dA[E], dB[E], dV[E]; };
template <int D, int E> struct TensoRFTangentCP { float dV[D][E], O[D][E]; };

// k_tensorf_fwd's split.  Per lane, once: cells, the gathers, the conversions and every term without v; then the rolled loop over the
// directions.  Direction t is v.data + t * v_next through v's strides; its result goes to the buffer t * t_next bytes behind `out`.
// Units behind the width store zeros.
template <typename T, bool CP, int D, int F>
__global__ void __launch_bounds__(256) k_tensorf_tangent(const uint32_t n, const uint32_t n_units, const TensoRFLevels lv, const MatView x, const MatView v, const uint32_t v_next,
                                                         const uint32_t n_t, const T* __restrict__ params, T* __restrict__ out, const uint32_t out_stride, const size_t t_next,
                                                         const uint32_t n_slots, const int vector_stores) {
	typedef TensoRFChunk<T, F> C;
	constexpr int CH = C::CH, E = C::E, S = C::S;
	typedef typename VecOf<T, CH>::type vecCH;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / n_slots;
	if (i >= n) return;
	const uint32_t j = gid - i * n_slots;
	float xin[D];
	load_coords<D>(x, i, xin);
	bool live[S];
	float scale[S];
	uint32_t mode[S];
	typename std::conditional<CP, TensoRFTangentCP<D, E>, TensoRFTangentVM<E>>::type w[S]; // what a unit keeps for the loop
	if constexpr (CP) {
		TensoRFCP<T, D, F, E> u[S];
		TensoRFCell<D> cs[S];
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const uint32_t col = j * CH + s * E, level = col / F;
			live[s] = level < n_units;
			mode[s] = 0u;
			scale[s] = 0.0f;
			if (live[s]) {
				cs[s].setup(xin, lv, level);
				scale[s] = cs[s].scale;
				u[s].locate(cs[s]);
				u[s].load(params + (size_t)lv.offset[level] * F, cs[s], col % F);
			}
		}
#pragma unroll
		for (int s = 0; s < S; ++s) {
			if (live[s]) {
				float V[D][E];
				u[s].line_values(cs[s], V);
				u[s].line_slopes(w[s].dV);
				u[s].others(V, w[s].O);
			}
		}
	} else {
		TensoRFVM<T, F, E> u[S];
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const uint32_t col = j * CH + s * E, unit = col / F, level = unit / 3u;
			live[s] = unit < n_units;
			mode[s] = unit - level * 3u;
			scale[s] = 0.0f;
			if (live[s]) {
				TensoRFCell<3> cs;
				cs.setup(xin, lv, level);
				scale[s] = cs.scale;
				u[s].locate(cs, mode[s]);
				u[s].load(params + (size_t)lv.offset[level] * F, cs, mode[s], col % F, true, true);
			}
		}
#pragma unroll
		for (int s = 0; s < S; ++s) {
			if (live[s]) {
				float M[E];
				u[s].plane_values(w[s].P);
				u[s].line_values(w[s].V);
				u[s].plane_slopes(w[s].dA, w[s].dB, M);
				u[s].line_slope(w[s].dV);
			}
		}
	}
	const size_t o_first = (size_t)i * out_stride + (size_t)j * CH;
#pragma unroll 1
	for (uint32_t t = 0; t < n_t; ++t) {
		float vin[D], res[CH];
		load_coords<D>(MatView{v.data + (size_t)t * v_next, v.stride_sample, v.stride_dim}, i, vin);
#pragma unroll
		for (int e = 0; e < CH; ++e) res[e] = 0.0f;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			if (live[s]) {
				if constexpr (CP) {
#pragma unroll
					for (int f = 0; f < E; ++f) {
						float r = (w[s].dV[0][f] * (scale[s] * vin[0])) * w[s].O[0][f];
#pragma unroll
						for (int d = 1; d < D; ++d) r = fmaf(w[s].dV[d][f] * (scale[s] * vin[d]), w[s].O[d][f], r);
						res[s * E + f] = r;
					}
				} else {
					float vsa, vsb, vsc;
					tensorf_mode_direction(vin, scale[s], mode[s], vsa, vsb, vsc);
#pragma unroll
					for (int f = 0; f < E; ++f) res[s * E + f] = fmaf(fmaf(vsb, w[s].dB[f], vsa * w[s].dA[f]), w[s].V[f], w[s].P[f] * (w[s].dV[f] * vsc));
				}
			}
		}
		T* o = (T*)((char*)out + (size_t)t * t_next) + o_first;
		if (vector_stores) { // (out_stride % CH == 0, so j * CH + CH <= out_stride, and every buffer starts on a multiple of 16 bytes)
			vecCH row;
#pragma unroll
			for (int e = 0; e < CH; ++e) row[e] = (T)res[e];
			*(vecCH*)o = row;
		} else {
#pragma unroll
			for (int e = 0; e < CH; ++e) if (j * CH + e < out_stride) o[e] = (T)res[e];
		}
	}
}

// ---------------------------------------------------------------------------------------------------------------- dL/dx
// W lanes per sample (a power of two, <= 64); lane j takes the units j, j + W, ... of n_units * (F / E)
template <typename T, bool CP, int D, int F>
__global__ void __launch_bounds__(256) k_tensorf_bwd_input(const uint32_t n, const uint32_t n_items, const TensoRFLevels lv, const MatView x, const T* __restrict__ params,
                                                           const T* __restrict__ dL_dy, const uint32_t dy_stride, const uint32_t W, const MatViewMut dL_dx) {
	constexpr int E = TensoRFChunk<T, F>::E;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / W, j = gid & (W - 1u);
	const bool live = i < n; // (no early return: every lane of the wave takes part in the butterfly)
	float sum[D];
#pragma unroll
	for (int d = 0; d < D; ++d) sum[d] = 0.0f;
	if (live) {
		float xin[D];
		load_coords<D>(x, i, xin);
		const T* __restrict__ row = dL_dy + (size_t)i * dy_stride;
		for (uint32_t item = j; item < n_items; item += W) {
			const uint32_t col = item * E, f0 = col % F;
			float g[E];
			tensorf_load_dy<T, E>(row, col, dy_stride, g);
			if constexpr (CP) {
				const uint32_t level = col / F;
				TensoRFCell<D> cs;
				cs.setup(xin, lv, level);
				TensoRFCP<T, D, F, E> u;
				u.locate(cs);
				u.load(params + (size_t)lv.offset[level] * F, cs, f0);
				float V[D][E], O[D][E];
				u.line_values(cs, V);
				u.others(V, O);
#pragma unroll
				for (int d = 0; d < D; ++d) {
					float dx = 0.0f; // in cells; times scale below
#pragma unroll
					for (int f = 0; f < E; ++f) dx = fmaf(g[f] * O[d][f], tensorf_elem(u.l[d][1], f) - tensorf_elem(u.l[d][0], f), dx);
					sum[d] = fmaf(cs.scale, dx, sum[d]);
				}
			} else {
				const uint32_t unit = col / F, level = unit / 3u, k = unit - level * 3u;
				TensoRFCell<3> cs;
				cs.setup(xin, lv, level);
				TensoRFVM<T, F, E> u;
				u.locate(cs, k);
				u.load(params + (size_t)lv.offset[level] * F, cs, k, f0, true, true);
				float P[E], V[E];
				u.plane_values(P);
				u.line_values(V);
				float da = 0.0f, db = 0.0f, dc = 0.0f;
#pragma unroll
				for (int f = 0; f < E; ++f) {
					const float v0 = tensorf_elem(u.p[0], f), v1 = tensorf_elem(u.p[1], f), v2 = tensorf_elem(u.p[2], f), v3 = tensorf_elem(u.p[3], f);
					const float gv = g[f] * V[f];
					da = fmaf(gv, fmaf(u.pb, (v3 - v2) - (v1 - v0), v1 - v0), da); // dP/dx_a = (1 - y)(v1 - v0) + y (v3 - v2)
					db = fmaf(gv, fmaf(u.pa, (v3 - v1) - (v2 - v0), v2 - v0), db); // dP/dx_b = (1 - x)(v2 - v0) + x (v3 - v1)
					dc = fmaf(g[f] * P[f], tensorf_elem(u.l[1], f) - tensorf_elem(u.l[0], f), dc);
				}
				const uint32_t a = k == 2u ? 1u : 0u, b = k == 0u ? 1u : 2u; // the line's axis is the third
#pragma unroll
				for (int d = 0; d < 3; ++d) sum[d] = fmaf(cs.scale, a == (uint32_t)d ? da : (b == (uint32_t)d ? db : dc), sum[d]);
			}
		}
	}
	for (uint32_t m = W >> 1; m >= 1; m >>= 1) {
#pragma unroll
		for (int d = 0; d < D; ++d) sum[d] += __shfl_xor(sum[d], (int)m, 64);
	}
	if (live && j == 0) {
#pragma unroll
		for (int d = 0; d < D; ++d) dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)d * dL_dx.stride_dim] = sum[d];
	}
}

// ---------------------------------------------------------------------------------------------------------------- dQ/dx
// k_tensorf_bwd_input's split and butterfly, for Q = <v, J^T dL_dy>: v is one direction, any layout
template <typename T, bool CP, int D, int F>
__global__ void __launch_bounds__(256) k_tensorf_bwdbwd_input(const uint32_t n, const uint32_t n_items, const TensoRFLevels lv, const MatView x, const MatView v,
                                                              const T* __restrict__ params, const T* __restrict__ dL_dy, const uint32_t dy_stride, const uint32_t W,
                                                              const MatViewMut dL_dx) {
	constexpr int E = TensoRFChunk<T, F>::E;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / W, j = gid & (W - 1u);
	const bool live = i < n; // (no early return: every lane of the wave takes part in the butterfly)
	float sum[D];
#pragma unroll
	for (int d = 0; d < D; ++d) sum[d] = 0.0f;
	if (live) {
		float xin[D], vin[D];
		load_coords<D>(x, i, xin);
		load_coords<D>(v, i, vin);
		const T* __restrict__ row = dL_dy + (size_t)i * dy_stride;
		for (uint32_t item = j; item < n_items; item += W) {
			const uint32_t col = item * E, f0 = col % F;
			float g[E];
			tensorf_load_dy<T, E>(row, col, dy_stride, g);
			if constexpr (CP) {
				const uint32_t level = col / F;
				TensoRFCell<D> cs;
				cs.setup(xin, lv, level);
				TensoRFCP<T, D, F, E> u;
				u.locate(cs);
				u.load(params + (size_t)lv.offset[level] * F, cs, f0);
				float V[D][E], dV[D][E], Tv[D][E], O[D][E], S[D][E];
				u.line_values(cs, V);
				u.line_slopes(dV);
#pragma unroll
				for (int d = 0; d < D; ++d) {
					const float vs = cs.scale * vin[d];
#pragma unroll
					for (int f = 0; f < E; ++f) Tv[d][f] = dV[d][f] * vs;
				}
				u.others_tangent(V, Tv, O, S);
#pragma unroll
				for (int d = 0; d < D; ++d) {
					float dx = 0.0f; // in cells; times scale below
#pragma unroll
					for (int f = 0; f < E; ++f) dx = fmaf(g[f], dV[d][f] * S[d][f], dx);
					sum[d] = fmaf(cs.scale, dx, sum[d]);
				}
			} else {
				const uint32_t unit = col / F, level = unit / 3u, k = unit - level * 3u;
				TensoRFCell<3> cs;
				cs.setup(xin, lv, level);
				TensoRFVM<T, F, E> u;
				u.locate(cs, k);
				u.load(params + (size_t)lv.offset[level] * F, cs, k, f0, true, true);
				float V[E], dV[E], dA[E], dB[E], M[E];
				u.line_values(V);
				u.line_slope(dV);
				u.plane_slopes(dA, dB, M);
				float vsa, vsb, vsc;
				tensorf_mode_direction(vin, cs.scale, k, vsa, vsb, vsc);
				float da = 0.0f, db = 0.0f, dc = 0.0f;
#pragma unroll
				for (int f = 0; f < E; ++f) {
					const float lvs = dV[f] * vsc;
					da = fmaf(g[f], fmaf(M[f] * vsb, V[f], dA[f] * lvs), da);
					db = fmaf(g[f], fmaf(M[f] * vsa, V[f], dB[f] * lvs), db);
					dc = fmaf(g[f], dV[f] * fmaf(vsb, dB[f], vsa * dA[f]), dc);
				}
				const uint32_t a = k == 2u ? 1u : 0u, b = k == 0u ? 1u : 2u; // the line's axis is the third
#pragma unroll
				for (int d = 0; d < 3; ++d) sum[d] = fmaf(cs.scale, a == (uint32_t)d ? da : (b == (uint32_t)d ? db : dc), sum[d]);
			}
		}
	}
	for (uint32_t m = W >> 1; m >= 1; m >>= 1) {
#pragma unroll
		for (int d = 0; d < D; ++d) sum[d] += __shfl_xor(sum[d], (int)m, 64);
	}
	if (live && j == 0) {
#pragma unroll
		for (int d = 0; d < D; ++d) dL_dx.data[(size_t)i * dL_dx.stride_sample + (size_t)d * dL_dx.stride_dim] = sum[d];
	}
}

// ---------------------------------------------------------------------------------------------------------------- dL/dparams, half
// Where a level's accumulators go (host and device agree): passes 0 .. 3 of k_tensorf_bwd
//   0  planes and lines together in LDS (CP: the lines, whole)     1  planes alone, in LDS     2  planes alone, in the global scratch
//   3  lines alone in LDS, in n_segs segments of seg_len entries
struct TensoRFPlan {
	bool together, planes_lds;
	uint32_t seg_len, n_segs;
	__host__ __device__ bool in_pass(bool cp, int pass) const { return together ? pass == 0 : (pass == 3 || (!cp && pass == (planes_lds ? 1 : 2))); }
};
__host__ __device__ inline TensoRFPlan tensorf_plan(const bool cp, const uint32_t K, const uint32_t size, const uint32_t lsize, const uint32_t E) {
	const uint64_t per_entry = (uint64_t)E * 8u, plane_bytes = cp ? 0u : 3u * (uint64_t)size * per_entry, line_bytes = (uint64_t)K * lsize * per_entry;
	TensoRFPlan r;
	r.together = plane_bytes + line_bytes <= TENSORF_LDS_BYTES;
	r.planes_lds = plane_bytes <= TENSORF_LDS_BYTES;
	const uint32_t most = (uint32_t)(TENSORF_LDS_BYTES / (K * per_entry)) & ~7u; // at least 64
	r.seg_len = lsize < most ? lsize : most;
	r.n_segs = (lsize + r.seg_len - 1u) / r.seg_len;
	return r;
}

typedef __attribute__((address_space(3))) unsigned long long tensorf_lds_u64;

__device__ inline unsigned long long tensorf_fixed(const float contribution) { return (unsigned long long)half_to_fixed_fast((half_t)contribution); }

// grid: (batch slices, n_levels * F / E, line segments)
template <bool CP, int D, int F>
__global__ void __launch_bounds__(256) k_tensorf_bwd(const uint32_t n, const TensoRFLevels lv, const MatView x, const half_t* __restrict__ params, const half_t* __restrict__ dL_dy,
                                                     const uint32_t dy_stride, unsigned long long* __restrict__ scratch, const int pass) {
	extern __shared__ __attribute__((aligned(16))) char tensorf_smem[];
	constexpr int E = TensoRFChunk<half_t, F>::E, NC = F / E, K = CP ? D : 3;
	const uint32_t level = blockIdx.y / NC, f0 = (blockIdx.y - level * NC) * E;
	const uint32_t R = lv.resolution[level], size = lv.entries[level], lsize = tensorf_line_entries(R);
	const TensoRFPlan plan = tensorf_plan(CP, K, size, lsize, E);
	if (!plan.in_pass(CP, pass)) return; // the other launches' level
	const bool do_planes = !CP && pass != 3, do_lines = pass == 0 || pass == 3, planes_lds = do_planes && pass != 2;
	const uint32_t seg_begin = blockIdx.z * plan.seg_len;
	if (blockIdx.z > 0 && (!do_lines || seg_begin >= lsize)) return;
	const uint32_t seg_len = min(plan.seg_len, lsize - seg_begin);
	const uint32_t plane_words = planes_lds ? 3u * size * E : 0u, line_words = do_lines ? K * seg_len * E : 0u; // together at most 8192
	unsigned long long* smem = (unsigned long long*)tensorf_smem;
	tensorf_lds_u64* acc_planes = (tensorf_lds_u64*)tensorf_smem;
	tensorf_lds_u64* acc_lines = acc_planes + plane_words;
	for (uint32_t e = threadIdx.x; e < plane_words + line_words; e += blockDim.x) smem[e] = 0ull;
	__syncthreads();

	const half_t* __restrict__ table = params + (size_t)lv.offset[level] * F;
	unsigned long long* global_acc = scratch + (size_t)lv.offset[level] * F;
	const uint32_t begin = blockIdx.x * TENSORF_BWD_SAMPLES, end = min(n, begin + TENSORF_BWD_SAMPLES);
	for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
		float xin[D];
		load_coords<D>(x, i, xin);
		TensoRFCell<D> cs;
		cs.setup(xin, lv, level);
		const half_t* __restrict__ row = dL_dy + (size_t)i * dy_stride;
		if constexpr (CP) {
			TensoRFCP<half_t, D, F, E> u;
			u.locate(cs);
			u.load(table, cs, f0);
			float g[E], V[D][E], O[D][E];
			tensorf_load_dy<half_t, E>(row, level * F + f0, dy_stride, g);
			u.line_values(cs, V);
			u.others(V, O);
#pragma unroll
			for (int d = 0; d < D; ++d) {
#pragma unroll
				for (int q = 0; q < 2; ++q) {
					const uint32_t at = u.lidx[d][q] - seg_begin;
					if (at < seg_len) {
						const float w = q ? cs.pos[d] : 1 - cs.pos[d];
#pragma unroll
						for (int f = 0; f < E; ++f) __hip_atomic_fetch_add(acc_lines + ((uint32_t)d * seg_len + at) * E + f, tensorf_fixed((g[f] * O[d][f]) * w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					}
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				TensoRFVM<half_t, F, E> u;
				u.locate(cs, (uint32_t)k);
				u.load(table, cs, (uint32_t)k, f0, do_lines, do_planes); // a plane's gradient reads the line, a line's the plane
				float g[E];
				tensorf_load_dy<half_t, E>(row, (level * 3u + k) * F + f0, dy_stride, g);
				if (do_planes) {
					float V[E];
					u.line_values(V);
#pragma unroll
					for (int q = 0; q < 4; ++q) {
						const float w = u.weight(q);
						const uint32_t entry = (uint32_t)k * size + u.pidx[q];
#pragma unroll
						for (int f = 0; f < E; ++f) {
							const unsigned long long t = tensorf_fixed((g[f] * V[f]) * w);
							if (planes_lds) __hip_atomic_fetch_add(acc_planes + entry * E + f, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
							else if (t != 0) atomicAdd(global_acc + (size_t)entry * F + f0 + f, t);
						}
					}
				}
				if (do_lines) {
					float P[E];
					u.plane_values(P);
#pragma unroll
					for (int q = 0; q < 2; ++q) {
						const uint32_t at = u.lidx[q] - seg_begin;
						if (at < seg_len) {
							const float w = q ? u.pl : 1 - u.pl;
#pragma unroll
							for (int f = 0; f < E; ++f) __hip_atomic_fetch_add(acc_lines + ((uint32_t)k * seg_len + at) * E + f, tensorf_fixed((g[f] * P[f]) * w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
						}
					}
				}
			}
		}
	}
	__syncthreads();
	for (uint32_t e = threadIdx.x; e < plane_words; e += blockDim.x) { // word e: entry e / E (of the 3 planes), component f0 + e % E
		const unsigned long long v = smem[e];
		if (v != 0) atomicAdd(global_acc + (size_t)(e / E) * F + f0 + e % E, v);
	}
	const size_t first_line = CP ? 0 : (size_t)3 * size; // in entries behind the level's first
	for (uint32_t e = threadIdx.x; e < line_words; e += blockDim.x) {
		const unsigned long long v = smem[plane_words + e];
		const uint32_t k = e / (seg_len * E), r = e - k * (seg_len * E);
		if (v != 0) atomicAdd(global_acc + (first_line + (size_t)k * lsize + seg_begin + r / E) * F + f0 + r % E, v);
	}
}

// dQ/dparams, half: k_tensorf_bwd's grid, passes (tensorf_plan), accumulators and flush, with the second-order contributions.  What a pass
// gathers: a plane corner's contribution reads the line alone (V, V'), a line entry's the plane alone (P, DP).
template <bool CP, int D, int F>
__global__ void __launch_bounds__(256) k_tensorf_bwdbwd(const uint32_t n, const TensoRFLevels lv, const MatView x, const MatView v, const half_t* __restrict__ params,
                                                        const half_t* __restrict__ dL_dy, const uint32_t dy_stride, unsigned long long* __restrict__ scratch, const int pass) {
	extern __shared__ __attribute__((aligned(16))) char tensorf_smem[];
	constexpr int E = TensoRFChunk<half_t, F>::E, NC = F / E, K = CP ? D : 3;
	const uint32_t level = blockIdx.y / NC, f0 = (blockIdx.y - level * NC) * E;
	const uint32_t R = lv.resolution[level], size = lv.entries[level], lsize = tensorf_line_entries(R);
	const TensoRFPlan plan = tensorf_plan(CP, K, size, lsize, E);
	if (!plan.in_pass(CP, pass)) return; // the other launches' level
	const bool do_planes = !CP && pass != 3, do_lines = pass == 0 || pass == 3, planes_lds = do_planes && pass != 2;
	const uint32_t seg_begin = blockIdx.z * plan.seg_len;
	if (blockIdx.z > 0 && (!do_lines || seg_begin >= lsize)) return;
	const uint32_t seg_len = min(plan.seg_len, lsize - seg_begin);
	const uint32_t plane_words = planes_lds ? 3u * size * E : 0u, line_words = do_lines ? K * seg_len * E : 0u; // together at most 8192
	unsigned long long* smem = (unsigned long long*)tensorf_smem;
	tensorf_lds_u64* acc_planes = (tensorf_lds_u64*)tensorf_smem;
	tensorf_lds_u64* acc_lines = acc_planes + plane_words;
	for (uint32_t e = threadIdx.x; e < plane_words + line_words; e += blockDim.x) smem[e] = 0ull;
	__syncthreads();

	const half_t* __restrict__ table = params + (size_t)lv.offset[level] * F;
	unsigned long long* global_acc = scratch + (size_t)lv.offset[level] * F;
	const uint32_t begin = blockIdx.x * TENSORF_BWD_SAMPLES, end = min(n, begin + TENSORF_BWD_SAMPLES);
	for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
		float xin[D], vin[D];
		load_coords<D>(x, i, xin);
		load_coords<D>(v, i, vin);
		TensoRFCell<D> cs;
		cs.setup(xin, lv, level);
		const half_t* __restrict__ row = dL_dy + (size_t)i * dy_stride;
		if constexpr (CP) {
			TensoRFCP<half_t, D, F, E> u;
			u.locate(cs);
			u.load(table, cs, f0);
			float g[E], V[D][E], Tv[D][E], O[D][E], S[D][E];
			tensorf_load_dy<half_t, E>(row, level * F + f0, dy_stride, g);
			u.line_values(cs, V);
			u.line_slopes(Tv);
#pragma unroll
			for (int d = 0; d < D; ++d) {
				const float vs = cs.scale * vin[d];
#pragma unroll
				for (int f = 0; f < E; ++f) Tv[d][f] *= vs;
			}
			u.others_tangent(V, Tv, O, S);
#pragma unroll
			for (int d = 0; d < D; ++d) {
				const float vs = cs.scale * vin[d];
#pragma unroll
				for (int q = 0; q < 2; ++q) {
					const uint32_t at = u.lidx[d][q] - seg_begin;
					if (at < seg_len) {
						const float w = q ? cs.pos[d] : 1 - cs.pos[d], sv = q ? vs : -vs;
#pragma unroll
						for (int f = 0; f < E; ++f) __hip_atomic_fetch_add(acc_lines + ((uint32_t)d * seg_len + at) * E + f, tensorf_fixed(g[f] * fmaf(S[d][f], w, O[d][f] * sv)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					}
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				TensoRFVM<half_t, F, E> u;
				u.locate(cs, (uint32_t)k);
				u.load(table, cs, (uint32_t)k, f0, do_lines, do_planes);
				float g[E], vsa, vsb, vsc;
				tensorf_load_dy<half_t, E>(row, (level * 3u + k) * F + f0, dy_stride, g);
				tensorf_mode_direction(vin, cs.scale, (uint32_t)k, vsa, vsb, vsc);
				if (do_planes) {
					float V[E], lvs[E];
					u.line_values(V);
					u.line_slope(lvs);
#pragma unroll
					for (int f = 0; f < E; ++f) lvs[f] *= vsc;
#pragma unroll
					for (int q = 0; q < 4; ++q) {
						const float w = u.weight(q), dw = u.weight_tangent(q, vsa, vsb);
						const uint32_t entry = (uint32_t)k * size + u.pidx[q];
#pragma unroll
						for (int f = 0; f < E; ++f) {
							const unsigned long long t = tensorf_fixed(g[f] * fmaf(V[f], dw, w * lvs[f]));
							if (planes_lds) __hip_atomic_fetch_add(acc_planes + entry * E + f, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
							else if (t != 0) atomicAdd(global_acc + (size_t)entry * F + f0 + f, t);
						}
					}
				}
				if (do_lines) {
					float P[E], dA[E], dB[E], M[E];
					u.plane_values(P);
					u.plane_slopes(dA, dB, M);
#pragma unroll
					for (int q = 0; q < 2; ++q) {
						const uint32_t at = u.lidx[q] - seg_begin;
						if (at < seg_len) {
							const float w = q ? u.pl : 1 - u.pl, sv = q ? vsc : -vsc;
#pragma unroll
							for (int f = 0; f < E; ++f) __hip_atomic_fetch_add(acc_lines + ((uint32_t)k * seg_len + at) * E + f, tensorf_fixed(g[f] * fmaf(fmaf(vsb, dB[f], vsa * dA[f]), w, P[f] * sv)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
						}
					}
				}
			}
		}
	}
	__syncthreads();
	for (uint32_t e = threadIdx.x; e < plane_words; e += blockDim.x) { // word e: entry e / E (of the 3 planes), component f0 + e % E
		const unsigned long long w = smem[e];
		if (w != 0) atomicAdd(global_acc + (size_t)(e / E) * F + f0 + e % E, w);
	}
	const size_t first_line = CP ? 0 : (size_t)3 * size; // in entries behind the level's first
	for (uint32_t e = threadIdx.x; e < line_words; e += blockDim.x) {
		const unsigned long long w = smem[plane_words + e];
		const uint32_t k = e / (seg_len * E), r = e - k * (seg_len * E);
		if (w != 0) atomicAdd(global_acc + (first_line + (size_t)k * lsize + seg_begin + r / E) * F + f0 + r % E, w);
	}
}

// scratch (exact sums) -> gradients, rounded once; the scratch is left zeroed for the next pass
__global__ void __launch_bounds__(256) k_tensorf_finalize(const size_t n_params, unsigned long long* __restrict__ scratch, half_t* __restrict__ grad, const int accumulate) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_params) return;
	long long s = (long long)scratch[i];
	if (s != 0) scratch[i] = 0;
	if (accumulate) s += half_to_fixed_fast(grad[i]);
	grad[i] = fixed_to_half_fast(s);
}

// ---------------------------------------------------------------------------------------------------------------- dL/dparams, float
__global__ void __launch_bounds__(256) k_tensorf_zero(const size_t n, float* __restrict__ p) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) p[i] = 0.0f;
}

// one lane per (sample, level, chunk of E components)
template <bool CP, int D, int F>
__global__ void __launch_bounds__(256) k_tensorf_bwd_f32(const uint32_t n, const uint32_t n_levels, const TensoRFLevels lv, const MatView x, const float* __restrict__ params,
                                                         const float* __restrict__ dL_dy, const uint32_t dy_stride, float* __restrict__ grad) {
	constexpr int E = TensoRFChunk<float, F>::E, NC = F / E;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, per_sample = n_levels * NC;
	const uint32_t i = gid / per_sample;
	if (i >= n) return;
	const uint32_t item = gid - i * per_sample, level = item / NC, f0 = (item - level * NC) * E;
	float xin[D];
	load_coords<D>(x, i, xin);
	TensoRFCell<D> cs;
	cs.setup(xin, lv, level);
	const float* __restrict__ table = params + (size_t)lv.offset[level] * F;
	float* __restrict__ gtable = grad + (size_t)lv.offset[level] * F;
	const float* __restrict__ row = dL_dy + (size_t)i * dy_stride;
	if constexpr (CP) {
		TensoRFCP<float, D, F, E> u;
		u.locate(cs);
		u.load(table, cs, f0);
		float g[E], V[D][E], O[D][E];
		tensorf_load_dy<float, E>(row, level * F + f0, dy_stride, g);
		u.line_values(cs, V);
		u.others(V, O);
#pragma unroll
		for (int d = 0; d < D; ++d) {
#pragma unroll
			for (int q = 0; q < 2; ++q) {
				const float w = q ? cs.pos[d] : 1 - cs.pos[d];
#pragma unroll
				for (int f = 0; f < E; ++f) atomicAdd(gtable + ((size_t)d * cs.lsize + u.lidx[d][q]) * F + f0 + f, (g[f] * O[d][f]) * w);
			}
		}
	} else {
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			TensoRFVM<float, F, E> u;
			u.locate(cs, (uint32_t)k);
			u.load(table, cs, (uint32_t)k, f0, true, true);
			float g[E], P[E], V[E];
			tensorf_load_dy<float, E>(row, (level * 3u + k) * F + f0, dy_stride, g);
			u.plane_values(P);
			u.line_values(V);
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const float w = u.weight(q);
#pragma unroll
				for (int f = 0; f < E; ++f) atomicAdd(gtable + ((size_t)k * cs.size + u.pidx[q]) * F + f0 + f, (g[f] * V[f]) * w);
			}
#pragma unroll
			for (int q = 0; q < 2; ++q) {
				const float w = q ? u.pl : 1 - u.pl;
#pragma unroll
				for (int f = 0; f < E; ++f) atomicAdd(gtable + ((size_t)3 * cs.size + (size_t)k * cs.lsize + u.lidx[q]) * F + f0 + f, (g[f] * P[f]) * w);
			}
		}
	}
}

// dQ/dparams, float: k_tensorf_bwd_f32's split, k_tensorf_bwdbwd's contributions
template <bool CP, int D, int F>
__global__ void __launch_bounds__(256) k_tensorf_bwdbwd_f32(const uint32_t n, const uint32_t n_levels, const TensoRFLevels lv, const MatView x, const MatView v,
                                                            const float* __restrict__ params, const float* __restrict__ dL_dy, const uint32_t dy_stride, float* __restrict__ grad) {
	constexpr int E = TensoRFChunk<float, F>::E, NC = F / E;
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, per_sample = n_levels * NC;
	const uint32_t i = gid / per_sample;
	if (i >= n) return;
	const uint32_t item = gid - i * per_sample, level = item / NC, f0 = (item - level * NC) * E;
	float xin[D], vin[D];
	load_coords<D>(x, i, xin);
	load_coords<D>(v, i, vin);
	TensoRFCell<D> cs;
	cs.setup(xin, lv, level);
	const float* __restrict__ table = params + (size_t)lv.offset[level] * F;
	float* __restrict__ gtable = grad + (size_t)lv.offset[level] * F;
	const float* __restrict__ row = dL_dy + (size_t)i * dy_stride;
	if constexpr (CP) {
		TensoRFCP<float, D, F, E> u;
		u.locate(cs);
		u.load(table, cs, f0);
		float g[E], V[D][E], Tv[D][E], O[D][E], S[D][E];
		tensorf_load_dy<float, E>(row, level * F + f0, dy_stride, g);
		u.line_values(cs, V);
		u.line_slopes(Tv);
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const float vs = cs.scale * vin[d];
#pragma unroll
			for (int f = 0; f < E; ++f) Tv[d][f] *= vs;
		}
		u.others_tangent(V, Tv, O, S);
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const float vs = cs.scale * vin[d];
#pragma unroll
			for (int q = 0; q < 2; ++q) {
				const float w = q ? cs.pos[d] : 1 - cs.pos[d], sv = q ? vs : -vs;
#pragma unroll
				for (int f = 0; f < E; ++f) atomicAdd(gtable + ((size_t)d * cs.lsize + u.lidx[d][q]) * F + f0 + f, g[f] * fmaf(S[d][f], w, O[d][f] * sv));
			}
		}
	} else {
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			TensoRFVM<float, F, E> u;
			u.locate(cs, (uint32_t)k);
			u.load(table, cs, (uint32_t)k, f0, true, true);
			float g[E], P[E], V[E], lvs[E], dA[E], dB[E], M[E], vsa, vsb, vsc;
			tensorf_load_dy<float, E>(row, (level * 3u + k) * F + f0, dy_stride, g);
			tensorf_mode_direction(vin, cs.scale, (uint32_t)k, vsa, vsb, vsc);
			u.plane_values(P);
			u.line_values(V);
			u.plane_slopes(dA, dB, M);
			u.line_slope(lvs);
#pragma unroll
			for (int f = 0; f < E; ++f) lvs[f] *= vsc;
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const float w = u.weight(q), dw = u.weight_tangent(q, vsa, vsb);
#pragma unroll
				for (int f = 0; f < E; ++f) atomicAdd(gtable + ((size_t)k * cs.size + u.pidx[q]) * F + f0 + f, g[f] * fmaf(V[f], dw, w * lvs[f]));
			}
#pragma unroll
			for (int q = 0; q < 2; ++q) {
				const float w = q ? u.pl : 1 - u.pl, sv = q ? vsc : -vsc;
#pragma unroll
				for (int f = 0; f < E; ++f) atomicAdd(gtable + ((size_t)3 * cs.size + (size_t)k * cs.lsize + u.lidx[q]) * F + f0 + f, g[f] * fmaf(fmaf(vsb, dB[f], vsa * dA[f]), w, P[f] * sv));
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------------------------- launches
uint32_t tensorf_blocks_for(uint64_t threads) {
	CHECK_THROW(threads < (1ull << 32));
	return (uint32_t)((threads + 255) / 256);
}

size_t tensorf_n_params(const TensoRFShape& p) {
	const uint32_t last = p.n_levels - 1;
	const size_t lines = (size_t)(p.cp ? p.n_dims : 3u) * tensorf_line_entries(p.levels.resolution[last]), planes = p.cp ? 0 : (size_t)3 * p.levels.entries[last];
	return ((size_t)p.levels.offset[last] + planes + lines) * p.n_components;
}

template <typename T, bool CP, int D, int F>
void launch_fwd(hipStream_t s, const TensoRFShape& p, uint32_t n, MatView x, const void* params, void* out, uint32_t out_stride) {
	const uint32_t n_slots = div_round_up(out_stride, (uint32_t)TensoRFChunk<T, F>::CH);
	hipLaunchKernelGGL((k_tensorf_fwd<T, CP, D, F>), dim3(tensorf_blocks_for((uint64_t)n * n_slots)), dim3(256), 0, s, n, p.n_levels * p.n_modes(), p.levels, x, (const T*)params, (T*)out,
	                   out_stride, n_slots);
}

template <typename T, bool CP, int D, int F>
void launch_bwd_input(hipStream_t s, const TensoRFShape& p, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	const uint32_t n_items = p.output_width() / (uint32_t)TensoRFChunk<T, F>::E;
	uint32_t W = 1;
	while (W < n_items && W < 64) W *= 2;
	hipLaunchKernelGGL((k_tensorf_bwd_input<T, CP, D, F>), dim3(tensorf_blocks_for((uint64_t)n * W)), dim3(256), 0, s, n, n_items, p.levels, x, (const T*)params, (const T*)dL_dy, dy_stride, W,
	                   dL_dx);
}

// v: null for dL/dparams, the direction for dQ/dparams (the k_tensorf_bwdbwd kernels; the same launches, passes and LDS)
template <bool CP, int D, int F>
void launch_bwd(hipStream_t s, const TensoRFShape& p, bool fp32, uint32_t n, MatView x, const MatView* v, const void* params, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch,
                void* grad, bool accumulate) {
	const size_t n_params = tensorf_n_params(p);
	if (fp32) {
		const dim3 blocks(tensorf_blocks_for((uint64_t)n * p.n_levels * (F / TensoRFChunk<float, F>::E)));
		if (!accumulate) hipLaunchKernelGGL(k_tensorf_zero, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (float*)grad);
		if (n > 0 && !v) hipLaunchKernelGGL((k_tensorf_bwd_f32<CP, D, F>), blocks, dim3(256), 0, s, n, p.n_levels, p.levels, x, (const float*)params, (const float*)dL_dy, dy_stride, (float*)grad);
		if (n > 0 && v) hipLaunchKernelGGL((k_tensorf_bwdbwd_f32<CP, D, F>), blocks, dim3(256), 0, s, n, p.n_levels, p.levels, x, *v, (const float*)params, (const float*)dL_dy, dy_stride, (float*)grad);
		return;
	}
	if (n > 0) {
		// One launch per pass that some level takes (each asks for the most LDS a level of it needs); in each the other levels' workgroups
		// return at once.
		constexpr uint32_t E = TensoRFChunk<half_t, F>::E, K = CP ? D : 3;
		size_t lds_bytes[4] = {0, 0, 0, 0};
		uint32_t segments[4] = {0, 0, 0, 0};
		for (uint32_t l = 0; l < p.n_levels; ++l) {
			const uint32_t size = p.levels.entries[l], lsize = tensorf_line_entries(p.levels.resolution[l]);
			const TensoRFPlan plan = tensorf_plan(CP, K, size, lsize, E);
			const size_t plane_bytes = CP ? 0 : (size_t)3 * size * E * 8, line_bytes = (size_t)K * plan.seg_len * E * 8;
			for (int pass = 0; pass < 4; ++pass) {
				if (!plan.in_pass(CP, pass)) continue;
				lds_bytes[pass] = std::max(lds_bytes[pass], pass == 0 ? plane_bytes + line_bytes : pass == 1 ? plane_bytes : pass == 2 ? (size_t)0 : line_bytes);
				segments[pass] = std::max(segments[pass], pass == 3 ? plan.n_segs : 1u);
			}
		}
		for (int pass = 0; pass < 4; ++pass) {
			if (segments[pass] == 0) continue;
			CHECK_THROW(lds_bytes[pass] <= TENSORF_LDS_BYTES && segments[pass] <= 65535u);
			const dim3 blocks(div_round_up(n, TENSORF_BWD_SAMPLES), p.n_levels * (F / E), segments[pass]);
			if (!v) hipLaunchKernelGGL((k_tensorf_bwd<CP, D, F>), blocks, dim3(256), (uint32_t)lds_bytes[pass], s, n, p.levels, x, (const half_t*)params, (const half_t*)dL_dy, dy_stride,
			                           (unsigned long long*)scratch, pass);
			else hipLaunchKernelGGL((k_tensorf_bwdbwd<CP, D, F>), blocks, dim3(256), (uint32_t)lds_bytes[pass], s, n, p.levels, x, *v, (const half_t*)params, (const half_t*)dL_dy, dy_stride,
			                        (unsigned long long*)scratch, pass);
		}
	}
	hipLaunchKernelGGL(k_tensorf_finalize, dim3((uint32_t)((n_params + 255) / 256)), dim3(256), 0, s, n_params, (unsigned long long*)scratch, (half_t*)grad, accumulate ? 1 : 0);
}

template <typename T, bool CP, int D, int F>
void launch_tangent(hipStream_t s, const TensoRFShape& p, uint32_t n, MatView x, MatView v, uint32_t v_next, uint32_t n_t, const void* params, void* t, uint32_t t_stride, size_t t_next) {
	constexpr uint32_t CH = TensoRFChunk<T, F>::CH;
	const uint32_t n_slots = div_round_up(t_stride, CH);
	const bool vector_stores = t_stride % CH == 0 && t_next % 16 == 0;
	hipLaunchKernelGGL((k_tensorf_tangent<T, CP, D, F>), dim3(tensorf_blocks_for((uint64_t)n * n_slots)), dim3(256), 0, s, n, p.n_levels * p.n_modes(), p.levels, x, v, v_next, n_t,
	                   (const T*)params, (T*)t, t_stride, t_next, n_slots, vector_stores ? 1 : 0);
}

template <typename T, bool CP, int D, int F>
void launch_bwdbwd_input(hipStream_t s, const TensoRFShape& p, uint32_t n, MatView x, MatView v, const void* params, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	const uint32_t n_items = p.output_width() / (uint32_t)TensoRFChunk<T, F>::E;
	uint32_t W = 1;
	while (W < n_items && W < 64) W *= 2;
	hipLaunchKernelGGL((k_tensorf_bwdbwd_input<T, CP, D, F>), dim3(tensorf_blocks_for((uint64_t)n * W)), dim3(256), 0, s, n, n_items, p.levels, x, v, (const T*)params, (const T*)dL_dy, dy_stride,
	                   W, dL_dx);
}

// run CALL with the compile-time <CP, D, F> of the shape
#define TCNN_TENSORF_F(CP_, D_, CALL) \
	switch (p.n_components) { \
		case 2: { constexpr bool CP = CP_; constexpr int D = D_, F = 2; CALL; } break; \
		case 4: { constexpr bool CP = CP_; constexpr int D = D_, F = 4; CALL; } break; \
		case 8: { constexpr bool CP = CP_; constexpr int D = D_, F = 8; CALL; } break; \
		case 16: { constexpr bool CP = CP_; constexpr int D = D_, F = 16; CALL; } break; \
		case 32: { constexpr bool CP = CP_; constexpr int D = D_, F = 32; CALL; } break; \
		default: throw std::runtime_error{"TensoRF: n_components must be 2, 4, 8, 16 or 32"}; \
	}
#define TCNN_TENSORF_DISPATCH(CALL) \
	if (!p.cp) { \
		if (p.n_dims != 3) throw std::runtime_error{"TensoRF: decomposition VM takes n_dims_to_encode 3"}; \
		TCNN_TENSORF_F(false, 3, CALL) \
	} else { \
		switch (p.n_dims) { \
			case 2: TCNN_TENSORF_F(true, 2, CALL) break; \
			case 3: TCNN_TENSORF_F(true, 3, CALL) break; \
			case 4: TCNN_TENSORF_F(true, 4, CALL) break; \
			default: throw std::runtime_error{"TensoRF: decomposition CP takes n_dims_to_encode 2 to 4"}; \
		} \
	}

} // namespace

void tensorf_forward(hipStream_t stream, const TensoRFShape& p, bool fp32, uint32_t n, MatView x, const void* params, void* out, uint32_t out_stride) {
	if (n == 0 || out_stride == 0) return;
	CHECK_THROW(out_stride >= p.output_width());
	if (fp32) { TCNN_TENSORF_DISPATCH((launch_fwd<float, CP, D, F>(stream, p, n, x, params, out, out_stride))) }
	else { TCNN_TENSORF_DISPATCH((launch_fwd<half_t, CP, D, F>(stream, p, n, x, params, out, out_stride))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void tensorf_backward_input(hipStream_t stream, const TensoRFShape& p, bool fp32, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, MatViewMut dL_dx) {
	if (n == 0) return;
	CHECK_THROW(dy_stride >= p.output_width());
	if (fp32) { TCNN_TENSORF_DISPATCH((launch_bwd_input<float, CP, D, F>(stream, p, n, x, params, dL_dy, dy_stride, dL_dx))) }
	else { TCNN_TENSORF_DISPATCH((launch_bwd_input<half_t, CP, D, F>(stream, p, n, x, params, dL_dy, dy_stride, dL_dx))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void tensorf_backward(hipStream_t stream, const TensoRFShape& p, bool fp32, uint32_t n, MatView x, const void* params, const void* dL_dy, uint32_t dy_stride, uint64_t* scratch, void* grad,
                      bool accumulate) {
	CHECK_THROW(dy_stride >= p.output_width());
	TCNN_TENSORF_DISPATCH((launch_bwd<CP, D, F>(stream, p, fp32, n, x, nullptr, params, dL_dy, dy_stride, scratch, grad, accumulate)))
	HIP_CHECK_THROW(hipGetLastError());
}

void tensorf_tangent(hipStream_t stream, const TensoRFShape& p, bool fp32, uint32_t n, MatView x, MatView v, uint32_t v_next, uint32_t n_tangents, const void* params, void* t,
                     uint32_t t_stride, size_t t_next) {
	if (n == 0 || t_stride == 0 || n_tangents == 0) return;
	CHECK_THROW(t_stride >= p.output_width() && t_next % (fp32 ? 4 : 2) == 0);
	if (fp32) { TCNN_TENSORF_DISPATCH((launch_tangent<float, CP, D, F>(stream, p, n, x, v, v_next, n_tangents, params, t, t_stride, t_next))) }
	else { TCNN_TENSORF_DISPATCH((launch_tangent<half_t, CP, D, F>(stream, p, n, x, v, v_next, n_tangents, params, t, t_stride, t_next))) }
	HIP_CHECK_THROW(hipGetLastError());
}

void tensorf_backward_backward_input(hipStream_t stream, const TensoRFShape& p, bool fp32, uint32_t n, MatView x, MatView v, const void* params, const void* dL_dy, uint32_t dy_stride,
                                     MatViewMut* dL_dx, uint64_t* scratch, void* grad, bool accumulate) {
	CHECK_THROW(dy_stride >= p.output_width());
	if (dL_dx && n > 0) {
		if (fp32) { TCNN_TENSORF_DISPATCH((launch_bwdbwd_input<float, CP, D, F>(stream, p, n, x, v, params, dL_dy, dy_stride, *dL_dx))) }
		else { TCNN_TENSORF_DISPATCH((launch_bwdbwd_input<half_t, CP, D, F>(stream, p, n, x, v, params, dL_dy, dy_stride, *dL_dx))) }
	}
	if (grad) { TCNN_TENSORF_DISPATCH((launch_bwd<CP, D, F>(stream, p, fp32, n, x, &v, params, dL_dy, dy_stride, scratch, grad, accumulate))) }
	HIP_CHECK_THROW(hipGetLastError());
}

} // namespace tcnn_amd
