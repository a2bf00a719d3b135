// What the hand-written MLP kernels (k_policy_mlp, k_sarl_actor, k_sarl_critic, k_marl_critic) share: the split
// float16 product on v_mfma_f32_32x32x16_f16 and the register order it leaves behind.  This is the one place that
// describes them; the kernels' headers say only what each does differently.
//
// Orientation.  D = A.B with A = weights (rows = 32 output features) and B = activations (columns = 32 rows of the
// batch), so after the K loop a LANE holds, for its row (lane & 31), half of that row's 32 output features in
// registers; the other half sits in lane ^ 32.
//
// Precision.  Both operands are split, x = hi + lo with hi = fp16(x), lo = fp16(x - hi) (split16), and the three
// significant partial products hi.hi + lo.hi + hi.lo taken as three MFMAs per k-step of 16 with float32 accumulation
// (mfma3): 2^-22 relative per product.  A weight matrix is pre-multiplied by a power of two 2^s -- its largest entry
// lands in [64, 128) -- so that its low part stays in the float16 normal range; the accumulator is multiplied back by
// 2^-s (exactly) where the float32 bias is added.  The low part of a small activation (< 0.125) can be a float16
// subnormal: absolute error <= 2^-25 per such product, below the float32 rounding of the sum.
//
// C/D register map of v_mfma_f32_32x32x16: register q of lane l is D[row = (q & 3) + 8 (q >> 2) + 4 (l >> 5)][col =
// l & 31], i.e. feature (q & 3) + 8 (q >> 2) + 4 h of the tile for batch row r (h = l >> 5, r = l & 31).  tile_of
// fetches 16 per-feature parameters in that order.
//
// Permuted k order.  A B operand of k-step s wants, in lane (r, h), the 8 values k = 16 s + 8 h + j of row r.  The
// registers 8u .. 8u+7 of a C/D tile are 8 features of row r already, so they ARE the B operand of a k-step as they
// stand -- "registers 8u .. 8u+7 = k-step u" -- provided the next layer's weight is laid out in the matching k order:
// k-step 2 tile + u, element j of lane (r, h) = feature 32 tile + 16 u + 8 (j >> 2) + 4 h + (j & 3).  The pack
// functions (host: ris_vec_marl_amd/_wstream.py "cd" order; device: acc_order_weights in risvec_pack.hpp) write the
// weight streams that way, so a layer's output needs only the ReLU and the split before it feeds the next MFMA.
#pragma once

#include <hip/hip_runtime.h>

#include "risvec_dev.hpp"

namespace risvec {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

constexpr float kLnEps = 1e-5f;
constexpr int kAhead = 4;            // gemm_tiles: weight fragments are requested this many k-steps ahead of their MFMAs

__device__ __forceinline__ void split16(const f32x8_t& y, half8_t& hi, half8_t& lo) {
    hi = __builtin_convertvector(y, half8_t);
    lo = __builtin_convertvector(y - __builtin_convertvector(hi, f32x8_t), half8_t);
}

__device__ __forceinline__ half8_t ld_frag(const uint4* p) {
    const uint4 v = *p;
    return __builtin_bit_cast(half8_t, v);
}

__device__ __forceinline__ f32x16_t mfma3(const half8_t& ah, const half8_t& al, const half8_t& bh, const half8_t& bl, f32x16_t d) {
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, d, 0, 0, 0);
    return d;
}

// acc[m] += W_m . B over nks k-steps.  wa: this wavefront's block of the stream, [nks][MT][hi | lo][64]; sb: the B
// fragments in LDS, [nks][hi | lo][64].  nks >= 1.
template <int MT>
__device__ __forceinline__ void gemm_tiles(f32x16_t (&acc)[MT], const uint4* __restrict__ wa, const uint4* sb, int nks, int lane) {
    half8_t ah[kAhead][MT], al[kAhead][MT];
    auto fetch = [&](int i, int s) {
        const uint4* p = wa + (size_t)(s < nks ? s : nks - 1) * (2 * MT * kWave) + lane;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            ah[i][m] = ld_frag(p + (2 * m) * kWave);
            al[i][m] = ld_frag(p + (2 * m + 1) * kWave);
        }
    };
#pragma unroll
    for (int i = 0; i < kAhead; ++i) fetch(i, i);
    for (int s0 = 0; s0 < nks; s0 += kAhead) {
#pragma unroll
        for (int i = 0; i < kAhead; ++i) {
            const int s = s0 + i;
            if (s < nks) {
                const half8_t bh = ld_frag(sb + (2 * s) * kWave + lane), bl = ld_frag(sb + (2 * s + 1) * kWave + lane);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = mfma3(ah[i][m], al[i][m], bh, bl, acc[m]);
                fetch(i, s + kAhead);
            }
        }
    }
}

// 16 per-feature parameters tab[base ..] in C/D register order: features (q & 3) + 8 (q >> 2) + 4 h
__device__ __forceinline__ f32x16_t tile_of(const float* tab, int base, int h) {
    f32x16_t tl;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 q4 = *reinterpret_cast<const float4*>(tab + base + 8 * g + 4 * h);
        tl[4 * g] = q4.x; tl[4 * g + 1] = q4.y; tl[4 * g + 2] = q4.z; tl[4 * g + 3] = q4.w;
    }
    return tl;
}

__device__ __forceinline__ float sum16(const f32x16_t& v) {
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += v[q];
    return s;
}

// relu(acc u + bias) of one C/D tile
__device__ __forceinline__ f32x16_t bias_relu(const f32x16_t& acc, float u, const f32x16_t& b) {
    f32x16_t y = acc * u + b;
#pragma unroll
    for (int q = 0; q < 16; ++q) y[q] = fmaxf(y[q], 0.0f);
    return y;
}

// registers 8u .. 8u+7 of a C/D tile -> the split B fragments of k-step 2 tile + u, left in LDS
__device__ __forceinline__ void put_tile(uint4* sh, int tile, const f32x16_t& y, int lane) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        f32x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = y[8 * u + j];
        half8_t hi, lo;
        split16(v, hi, lo);
        uint4* p = sh + ((2 * tile + u) * 2) * kWave + lane;
        p[0] = __builtin_bit_cast(uint4, hi);
        p[kWave] = __builtin_bit_cast(uint4, lo);
    }
}

}  // namespace risvec
