// r32_device.h -- the device code that the fused MLP training kernels built on v_mfma_f32_32x32x16_f16 share (k_train_r32.hip,
// k_train_r32a.hip, k_train_r32w.hip, k_train_r32ob.hip): the matrix instruction and its accumulating forms, result tile -> next operand,
// ReLU and its derivative on packed halves, the scheduling macros, buffer descriptors and the per-trip input load, the wave-private LDS
// image (layout, accessors), weight-fragment staging, the two loss tails, the output-row store and the stores of dL/d(encoded input).
// Operand maps: mlp_side_jobs.h (R32Frags).
//
// What is NOT here: a kernel's trip body (a pinned software pipeline of regions), its accumulators, barriers and final reduction.  These
// kernels are sensitive to how the source is phrased ("The 32x32x16 kernels": the stream rule) -- every piece below is in the
// form that leaves each kernel's instruction stream as it was when the piece stood in the kernel; tools/kernel_isa_diff.py checks it.
#pragma once

#include "mlp_device.h"

namespace tcnn_amd {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f8v __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ inline f16v mfma32(const h8 a, const h8 b, const f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
// Accumulate into AGPRs (weight-gradient tiles that live there for the whole kernel; every other matrix instruction is a builtin that the
// compiler places in ordinary registers: -mllvm -amdgpu-mfma-vgpr-form, build.py).  No hazard to pad: the operands come from LDS reads,
// which the compiler waits for, and back-to-back accumulation into the same registers needs no wait
__device__ inline void mfma32_acc(f16v& acc, const h8 a, const h8 b) { asm("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b)); }
__device__ inline void mfma16_acc(f4& acc, const h8 a, const h8 b) { asm("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b)); }
__device__ inline f16v zero16() {
	f16v z;
#pragma unroll
	for (int i = 0; i < 16; ++i) z[i] = 0.0f;
	return z;
}
// result registers 8 s .. 8 s + 7 -> the B fragment of the next layer's k-step (round to nearest even, like the reference's fp16 accumulators are read)
__device__ inline h8 pack8(const f16v v, const int s) {
	const f8v t = {v[8 * s + 0], v[8 * s + 1], v[8 * s + 2], v[8 * s + 3], v[8 * s + 4], v[8 * s + 5], v[8 * s + 6], v[8 * s + 7]};
	return __builtin_convertvector(t, h8);
}
// ReLU(half) = x > 0 ? x : 0 (common_device.h:92-98) as a signed integer maximum of the bit patterns (never -0: the backward pass tells
// "positive" from "zero" by the bits)
__device__ inline h8 relu8(const h8 v) { return __builtin_bit_cast(h8, __builtin_elementwise_max(__builtin_bit_cast(s16x8, v), s16x8{0, 0, 0, 0, 0, 0, 0, 0})); }
// ... and its derivative from the forward output (common_device.h:241-297): the gradient where the output has any bit set, +0 elsewhere
// (min(bits, 1) = 0 / 1, times the gradient's bits as an integer product)
template <bool AND_FORM = false> __device__ inline h8 relu_bwd8(const h8 g, const h8 fwd) {
	const u32x4 f = __builtin_bit_cast(u32x4, fwd), gb = __builtin_bit_cast(u32x4, g);
	u32x4 r;
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		uint32_t m, o;
		asm("v_pk_min_u16 %0, %1, 1 op_sel_hi:[1,0]" : "=v"(m) : "v"(f[i]));
		if constexpr (AND_FORM) { // 0 - (0 / 1) = all zeros / all ones, and
			asm("v_pk_sub_u16 %0, 0, %1 op_sel_hi:[0,1]" : "=v"(o) : "v"(m));
			o &= gb[i];
		} else {
			asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(o) : "v"(gb[i]), "v"(m));
		}
		r[i] = o;
	}
	return __builtin_bit_cast(h8, r);
}

// ---- scheduling.  A trip is written as a software pipeline of regions closed by R32_SB(): a region holds the matrix instructions of one
// step of the chain together with the vector / LDS work of the step before and the LDS reads of the operands of the region after
// (k_train_r32.hip).  Within a region R32_MVD(V, D): one matrix instruction, then V vector and D LDS instructions (sched_group_barrier
// masks: 0x8 MFMA, 0x2 VALU, 0x80 DS)
#define R32_SB() __builtin_amdgcn_sched_barrier(0)
#define R32_MVD(V, D) do { __builtin_amdgcn_sched_group_barrier(0x8, 1, 0); __builtin_amdgcn_sched_group_barrier(0x2, V, 0); __builtin_amdgcn_sched_group_barrier(0x80, D, 0); } while (0)

// ---- global addressing: raw buffer accesses -- a descriptor (scalar, per matrix) + a lane offset that never changes + a scalar offset of
// the trip's 32-sample block: the trip loop spends one scalar addition per stream on addresses and no vector instruction (as plain
// pointers the compiler carried 64-bit vector addresses: ~40 vector and ~50 scalar instructions per trip).  Offsets are 32-bit (the plans
// cap n); an access beyond a matrix is dropped by the range check instead of faulting.
// The descriptor's last word, 0x00020000, is DATA_FORMAT = 4 (32 bits; bits 15..18 of word 3) and nothing else: no swizzle, no
// structured stride, offsets checked against `bytes` -- what the compiler itself uses for untyped buffer access on gfx9.
__device__ inline auto r32_buffer(const void* p, const uint32_t bytes) { return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, (int)bytes, 0x00020000); }

// The per-trip input of the kernels fed by level planes of 2 features (32 inputs): this lane's two natural-order k-steps of sample c
// (features 16 s + 8 h + 2 i, + 1: levels 8 s + 4 h + i at + (8 s + i) n 4; x_off = (4 h n + c) 4), its two targets (t_off[r]: output
// min(2 r + h, dims - 1) -- outputs >= dims re-read the last one, masked where used) and, for scatter records, the sample's position.
struct R32In { h8 x[2]; float t[2]; float2 xs; };
// Declares the lane offsets x_off, t_off and the lambda load_in(block) -> R32In over the kernel's a, c, h, n4 = 4 n and the descriptors
// rs_x, rs_t, rs_xs (a macro: as a function the compiler commutes one scalar addition of the plane offsets, which the dL/dx plane stores
// share -- 2 lines per plane-form instance of k_mlp_train_r32a).
// blk: scalar for the compiler too -- it is the scalar offset of every access (left to the compiler the trip's block number lived in a vector
// register and every one of these loads sat in a waterfall loop of its own -- v_readfirstlane, compare, branch: 22 per trip)
#define R32_DEFINE_LOAD_IN(REC) \
	const uint32_t x_off = (4 * h * a.n + c) * 4; \
	uint32_t t_off[2]; \
	_Pragma("unroll") for (int r = 0; r < 2; ++r) t_off[r] = (c * a.dims + min(2 * r + h, a.dims - 1)) * 4; \
	auto load_in = [&](const uint32_t blk_) -> R32In { \
		const uint32_t blk = __builtin_amdgcn_readfirstlane(blk_); \
		R32In r; \
		_Pragma("unroll") for (int s = 0; s < 2; ++s) { \
			u32x4 v; \
			_Pragma("unroll") for (int i = 0; i < 4; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b32(rs_x, x_off, blk * 128 + n4 * (8 * s + i), 0); \
			r.x[s] = __builtin_bit_cast(h8, v); \
		} \
		const uint32_t tb = blk * (128 * a.dims); \
		r.t[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_t, t_off[0], tb, 0)); \
		r.t[1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_t, t_off[1], tb, 0)); \
		if constexpr (REC) r.xs = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs_xs, c * 8, blk * 256, 0)); \
		else r.xs = float2{0, 0}; \
		return r; \
	}

// Cache policy of the scatter-record stores (the aux operand of the raw buffer stores: 0 default, 2 nontemporal).  Round 2 measured that
// streamed records cost the scatter 10 us: its tasks then ran on whatever XCD and found the records in the writer's L2.  Since round 4 a
// record plane is gathered by ONE XCD, which pulls it into its own L2 whatever the writers' L2s hold -- and every dirty line left in
// those at the kernel's end is written back on the kernel's time.
#ifndef TCNN_R32_REC_AUX
#define TCNN_R32_REC_AUX 0
#endif
constexpr int R32_REC_AUX = TCNN_R32_REC_AUX;
#ifndef TCNN_R32_OUT_AUX
#define TCNN_R32_OUT_AUX 2
#endif
constexpr int R32_OUT_AUX = TCNN_R32_OUT_AUX; // the [n][16] output rows (2: nontemporal)

// ---- the wave-private LDS image of a 32-feature x 32-sample tile (2 KiB): plane g (4 features) at 256 g, sample n inside it at
// 8 ((n + 4 g) & 31).  The rotation by 4 g makes both accesses conflict-free: a plane-wise write (32 lanes = the 32 samples of one plane,
// 8 bytes each) covers the plane's 256 bytes -- the 64 banks once -- whatever the rotation, and a transposing read (per 32 lanes 4
// consecutive samples x 8 planes, 32 bytes per plane) finds plane g's 32 bytes 32 g bytes further on than plane 0's: 8 x 32 bytes, the 64
// banks once.
//   w_chain, w_nat [2 s + e] -- writes: this lane holds, per k-step s and half e of a CHAIN fragment, the 4 features of plane 4 s + 2 e + h
//     of sample c (c = lane & 31, h = lane >> 5); of the NATURAL-order input fragment: plane 4 s + 2 h + e.
//   r_tr [2 s' + e], r_16 [2 half + e] -- transposing reads (ds_read_b64_tr_b16: per 16 lanes a block of 4 rows x 16 columns; lane 4 q + p
//     supplies the address of row q, columns 4 p .. 4 p + 3, and receives column (lane & 15) of the 4 rows):
//     32x32x16 operand of sample k-step s': element j = sample 16 s' + 8 hh + j of feature (lane & 31), hh = lane >> 5: reads e = 0, 1 of 4 samples;
//     16x16x32 operand (all 32 samples): element j = sample 8 (lane >> 4) + j of feature 16 half + (lane & 15).
// WBASE / RBASE: what the write / read maps carry besides the offset inside a tile (the wave's image area where a wave reads its own
// images only; 0 or the area's start where it reads every wave's).
// A macro, not a function: as a function (maps returned in a struct, through references, forced inline) the compiler arranges the address
// arithmetic differently and pairs the image writes into ds_write2st64_b64 -- ~1 500 of k_train_r32a.hip's 5 565 instructions change.
#define R32_IMAGE_MAPS(WBASE, RBASE) \
	uint32_t w_chain[4], w_nat[4], r_tr[4], r_16[4]; \
	_Pragma("unroll") for (int k = 0; k < 4; ++k) { \
		const uint32_t gc = 4 * (k >> 1) + 2 * (k & 1) + h, gn = 4 * (k >> 1) + 2 * h + (k & 1); \
		w_chain[k] = (WBASE) + gc * 256 + ((c + 4 * gc) & 31) * 8; \
		w_nat[k] = (WBASE) + gn * 256 + ((c + 4 * gn) & 31) * 8; \
	} \
	{ \
		const uint32_t grp = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3, hh = grp >> 1; \
		const uint32_t g = 4 * (grp & 1) + p; \
		_Pragma("unroll") for (int k = 0; k < 4; ++k) { \
			const uint32_t row = 16 * (k >> 1) + 8 * hh + 4 * (k & 1) + q; \
			r_tr[k] = (RBASE) + g * 256 + ((row + 4 * g) & 31) * 8; \
			const uint32_t g16 = 4 * (k >> 1) + p, row16 = 8 * grp + 4 * (k & 1) + q; \
			r_16[k] = (RBASE) + g16 * 256 + ((row16 + 4 * g16) & 31) * 8; \
		} \
	}

// accessors; a0, a1: byte addresses in LDS of a fragment's two halves (a lane map's entries 2 s, 2 s + 1 plus the tile's offset)
__device__ inline void r32_img_write(char* smem, const uint32_t a0, const uint32_t a1, const h8 v) { // a fragment as it stands in the registers
	*(h4*)(smem + a0) = h4{v[0], v[1], v[2], v[3]};
	*(h4*)(smem + a1) = h4{v[4], v[5], v[6], v[7]};
}
__device__ inline h8 r32_img_read(const char* smem, const uint32_t a0, const uint32_t a1) { // ... and back
	const h4 lo = *(const h4*)(smem + a0), hi = *(const h4*)(smem + a1);
	return h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ inline h8 r32_img_read_tr(const char* smem, const uint32_t a0, const uint32_t a1) { // transposed: an operand of a weight-gradient product
	const h4 lo = lds_read_tr((const half_t*)(smem + a0)), hi = lds_read_tr((const half_t*)(smem + a1));
	return h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ---- weight fragments (NF of 1 KiB) from the image in global memory (a.image) to the start of LDS, by the workgroup's NW waves: every
// load first (the last round clamped, not branched), the guarded stores behind them -- at once or, in k_train_r32a.hip, after other loads.
// Macros over the kernel's `a`, `tid`, `smem`: as functions filling an array through a reference, forced inline or not, they change 694 ..
// 758 of the ~1 440 lines of each k_mlp_train_r32a instance.
#define R32_STAGE_LOAD(TMP, NF, NW) \
	h8 TMP[((NF) * 64 + (NW) * 64 - 1) / ((NW) * 64)]; \
	_Pragma("unroll") for (int k = 0; k < ((NF) * 64 + (NW) * 64 - 1) / ((NW) * 64); ++k) TMP[k] = a.image[min(tid + k * (NW) * 64, (uint32_t)(NF) * 64u - 1u)]
#define R32_STAGE_STORE(TMP, NF, NW) \
	_Pragma("unroll") for (int k = 0; k < ((NF) * 64 + (NW) * 64 - 1) / ((NW) * 64); ++k) { \
		if (tid + k * (NW) * 64 < (uint32_t)(NF) * 64u) ((h8*)smem)[tid + k * (NW) * 64] = TMP[k]; \
	}

// ---- out [n][16] halves: result register g of lane half h holds output 2 g + h; words (2 g, 2 g + 1) of this lane and of its partner
// lane (the other half) interleave into the row, of which this lane gets half h (16 bytes)
// u[k] = outputs (4 k + h, 4 k + 2 + h): lanes < 32 keep u[k] and receive the partner's u[k]; lanes >= 32 receive the partner's u[k + 2] and
// keep their own -- sw[0], sw[1] = outputs (4 k' + 0, 4 k' + 2) and (4 k' + 1, 4 k' + 3), k' = k + 2 h --, then (even.lo, odd.lo), (even.hi, odd.hi).
// Declares ROW (u32x4).  A macro: as a function it left k_train_r32.hip and k_train_r32a.hip as they were and changed every line of
// k_mlp_train_r32w (2 780 of 2 682; that kernel spills, and the spills moved).
#define R32_OUT_ROW(ROW, OV) \
	u32x4 ROW; \
	{ \
		const u32x4 u = __builtin_bit_cast(u32x4, OV); \
		uint32_t w[4]; \
		_Pragma("unroll") for (int k = 0; k < 2; ++k) { \
			const auto sw = __builtin_amdgcn_permlane32_swap(u[k], u[k + 2], false, false); \
			w[2 * k + 0] = __builtin_amdgcn_perm(sw[1], sw[0], 0x05040100u); \
			w[2 * k + 1] = __builtin_amdgcn_perm(sw[1], sw[0], 0x07060302u); \
		} \
		ROW = u32x4{w[0], w[1], w[2], w[3]}; \
	}

// ---- dL/d(encoded input) of a 32-feature tile (result tile dx of W0^T dH0: registers 4 g .. 4 g + 3 are features 8 g + 4 h .. + 3 of sample
// c), for the grid encoding's scatter.  Offsets: lane offset `off` (never changes), the trip's block blk (scalar).
// STORES of 16 bytes take the block's offset in the VECTOR offset (one addition) and no scalar offset: with a scalar-register offset the
// compiler assumes the hardware needs no wait state between such a store and a vector instruction that overwrites its data registers
// (GCNHazardRecognizer: "only if the instruction is not using a register in the soffset field"); on gfx950 it does -- measured: the third
// dword of two of a trip's four records came out as whatever the next conversion wrote there.  (The output row's store obeys the same rule.)
// Records: 16 bytes {x, y, gradients of levels 2 p, 2 p + 1}, level pair p = 2 g + h at + g 2 n 16 (the bit-plane scatter, k_grid_scatter.hip);
// off = (h n + c) 16
template <typename RS> __device__ inline void r32_store_dx_records(const RS rs_rec, const uint32_t off, const uint32_t blk, const uint32_t n, const f16v dx, const float2 xs) {
	const u32x4 lo = __builtin_bit_cast(u32x4, pack8(dx, 0)), hi = __builtin_bit_cast(u32x4, pack8(dx, 1));
	const uint32_t x0 = __builtin_bit_cast(uint32_t, xs.x), x1 = __builtin_bit_cast(uint32_t, xs.y);
	const uint32_t rb = blk * 512, pair2 = n * 32; // pair2: two level pairs further
	__builtin_amdgcn_raw_buffer_store_b128(u32x4{x0, x1, lo[0], lo[1]}, rs_rec, off + rb, 0, R32_REC_AUX);
	__builtin_amdgcn_raw_buffer_store_b128(u32x4{x0, x1, lo[2], lo[3]}, rs_rec, off + (rb + pair2), 0, R32_REC_AUX);
	__builtin_amdgcn_raw_buffer_store_b128(u32x4{x0, x1, hi[0], hi[1]}, rs_rec, off + (rb + 2 * pair2), 0, R32_REC_AUX);
	__builtin_amdgcn_raw_buffer_store_b128(u32x4{x0, x1, hi[2], hi[3]}, rs_rec, off + (rb + 3 * pair2), 0, R32_REC_AUX);
}
// Plain level planes half2 [16][n] -- half the bytes -- for the list-fed scatter, whose elements know entries and weights
// (k_grid_scatter_lists.hip): word 2 g + j of the tile's 8 is level 4 g + 2 h + j of sample c, at + (4 g + j) n 4 -- eight dense 128-byte
// runs per half wave; OFF = (2 h n + c) 4
// (a macro: as a function the compiler commutes one scalar addition of the offsets in k_mlp_train_r32a -- 2 lines per instance; RS: the
// descriptor, OFF: the lane offset, BLK: the block, N4: 4 n, DX: the result tile)
#define R32_STORE_DX_PLANES(RS, OFF, BLK, N4, DX) do { \
		const u32x4 lo_ = __builtin_bit_cast(u32x4, pack8(DX, 0)), hi_ = __builtin_bit_cast(u32x4, pack8(DX, 1)); \
		const uint32_t w_[8] = {lo_[0], lo_[1], lo_[2], lo_[3], hi_[0], hi_[1], hi_[2], hi_[3]}; \
		_Pragma("unroll") for (int k = 0; k < 8; ++k) __builtin_amdgcn_raw_buffer_store_b32(w_[k], RS, OFF, (BLK) * 128 + (N4) * (4 * (k >> 1) + (k & 1)), R32_REC_AUX); \
	} while (0)

// ---- the loss on the result tile, compact form: l2.h:40-74 / relative_l2.h:40-75 on one refined reciprocal (loss_l2_fused, mlp_device.h),
// the two output slots of a lane (element r of OV: output 2 r + h; targets T[r]) side by side; values and gradients of the live outputs go
// to the compact context matrices [n][dims].  Declares DYF: dL/doutput as the B fragment of the first backward product (k = position).
// NO_LOSS: a timing-only stand-in (results are wrong).  A macro over the kernel's a, h, blk, n_total, lsc, rs_g (halves), rs_l (floats) and
// cg_off0 = (c dims + h) 2: as a function, by value and forced inline too, it changes 236 .. 1 121 lines of each k_mlp_train_r32a instance.
#define R32_LOSS_COMPACT(DYF, RELATIVE, NO_LOSS, OV, T) \
	h8 DYF = h8{0, 0, 0, 0, 0, 0, 0, 0}; \
	{ \
		float value[2]; \
		half_t grad[2]; \
		_Pragma("unroll") for (int r = 0; r < 2; ++r) { \
			const float prediction = (float)OV[r]; \
			if constexpr (NO_LOSS) { \
				value[r] = prediction - T[r]; \
				grad[r] = (half_t)(a.loss_scale * prediction / n_total); \
			} else loss_l2_fused<RELATIVE>(prediction, T[r], lsc, value[r], grad[r]); \
		} \
		asm volatile("" : "+v"(value[0]), "+v"(value[1])); /* both chains are evaluated here, in one block, not inside the masked stores below */ \
		_Pragma("unroll") for (int r = 0; r < 2; ++r) { \
			const bool live = 2 * r + h < a.dims; \
			DYF[r] = live ? grad[r] : (half_t)0.0f; \
			if (live) { \
				__builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(uint16_t, grad[r]), rs_g, cg_off0 + 4 * r, blk * (64 * a.dims), 2); \
				__builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, value[r]), rs_l, 2 * cg_off0 + 8 * r, blk * (128 * a.dims), 2); \
			} \
		} \
	}

// ---- the loss on the result tile, padded form: the same evaluation, context matrices in the reference's padded form [n][16] -- outputs
// 0..3 come from the two lanes of the sample (this lane: 2 r + h), the rest is zero.  Lanes h = 0 collect them; every lane stores its half
// of the row (16 bytes of dL/doutput, 32 bytes of the loss values; row_off = c 32 + h 16).  Declares DYF as above.  A macro over the
// kernel's a, h, blk, lsc, row_off: as a function it changes every line of k_mlp_train_r32w (2 849 of 2 682).
#define R32_LOSS_PADDED(DYF, RELATIVE, OV, T) \
	h8 DYF = h8{0, 0, 0, 0, 0, 0, 0, 0}; \
	{ \
		float value[2]; \
		half_t grad[2]; \
		_Pragma("unroll") for (int r = 0; r < 2; ++r) { \
			loss_l2_fused<RELATIVE>((float)OV[r], T[r], lsc, value[r], grad[r]); \
			const bool live = 2 * r + h < a.dims; \
			if (!live) { value[r] = 0.0f; grad[r] = (half_t)0.0f; } \
			DYF[r] = grad[r]; \
		} \
		typedef _Float16 h2 __attribute__((ext_vector_type(2))); \
		const uint32_t gpk = __builtin_bit_cast(uint32_t, (h2{grad[0], grad[1]})); /* (out h, out 2 + h) */ \
		const auto sg = __builtin_amdgcn_permlane32_swap(gpk, gpk, false, false);    /* lanes < 32: [0] own, [1] the partner's */ \
		const auto s0 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, value[0]), __builtin_bit_cast(uint32_t, value[0]), false, false); \
		const auto s1 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, value[1]), __builtin_bit_cast(uint32_t, value[1]), false, false); \
		u32x4 grow = u32x4{0, 0, 0, 0}, l0 = u32x4{0, 0, 0, 0}; \
		if (h == 0) { \
			grow[0] = __builtin_amdgcn_perm(sg[1], sg[0], 0x05040100u); /* (g0, g1) */ \
			grow[1] = __builtin_amdgcn_perm(sg[1], sg[0], 0x07060302u); /* (g2, g3) */ \
			l0 = u32x4{s0[0], s0[1], s1[0], s1[1]};                     /* L0, L1, L2, L3 */ \
		} \
		*(u32x4*)((char*)a.dL_dout + (size_t)blk * 1024 + row_off) = grow; \
		float* lrow = (float*)((char*)a.L + (size_t)blk * 2048 + 2 * row_off); \
		*(u32x4*)lrow = l0; \
		*(u32x4*)(lrow + 4) = u32x4{0, 0, 0, 0}; \
	}

} // namespace
} // namespace tcnn_amd
