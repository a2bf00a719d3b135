// What the on-device weight packs (k_sarl_actor_pack, k_sarl_critic_pack, k_marl_critic_pack) share: the order-independent
// maxima of the statistics launch, the shift of a float32 operand, and the split and the fragment order of the
// critics' pack launch.  The split is the one of risvec_mfma.hpp (read its header) taken scalar by scalar:
// hi = half(w), lo = half(w - float(hi)).  No product feeds a sum in any of this, so there is nothing for the compiler
// to contract; the pragma says so all the same.
#pragma once

#include "risvec_mfma.hpp"

#pragma clang fp contract(off)

namespace risvec {

constexpr int kStatBlock = 1024;                 // 16 wavefronts per workgroup of the statistics launch
constexpr int kStatWaves = kStatBlock / kWave;
constexpr int kPackBlock = 256;

// the largest of v over the workgroup (order-independent); red: kStatWaves slots of LDS
template <typename T>
__device__ __forceinline__ T block_max(T v, T* red) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const T w = __shfl_xor(v, o, kWave);
        v = w > v ? w : v;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    T r = red[0];
    for (int i = 1; i < kStatWaves; ++i) r = red[i] > r ? red[i] : r;
    __syncthreads();
    return r;
}

__device__ __forceinline__ float max4(float m, const float4& v) {
    return fmaxf(fmaxf(fmaxf(m, fabsf(v.x)), fmaxf(fabsf(v.y), fabsf(v.z))), fabsf(v.w));
}

// largest |x| of this thread's share of slice b (of nb) of p[0 .. n): floats up to the first 16-byte boundary and
// behind the last whole float4 belong to slice 0, the float4 between are dealt out in nb runs
__device__ __forceinline__ float amax_slice(const float* p, long long n, int b, int nb) {
    const int tid = threadIdx.x;
    long long head = (4 - (long long)((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3;
    head = head < n ? head : n;
    const long long n4 = (n - head) / 4, tail = head + 4 * n4;
    float m = 0.0f;
    if (b == 0) {
        if (tid < head) m = fabsf(p[tid]);
        if (tid >= kWave && tail + (tid - kWave) < n) m = fabsf(p[tail + (tid - kWave)]);     // at most 3 floats
    }
    const float4* v = reinterpret_cast<const float4*>(p + head);
    const long long per = (n4 + nb - 1) / nb, lo = per * b, hi = lo + per < n4 ? lo + per : n4;
#pragma unroll 4
    for (long long i = lo + tid; i < hi; i += kStatBlock) m = max4(m, v[i]);
    return m;
}

// The shift s of a float32 operand whose slices' maxima sit one per lane in a (0 in the lanes beyond the slices):
// s = clamp(floor(log2f(64 / max(amax, 1e-30))), -40, 40), wave-uniform, every lane of the wavefront taking part.
// (The slot by reference: by value k_marl_critic_pack comes out with another register assignment.)
__device__ __forceinline__ int shift_of_slots(const float& slot) {
    float a = slot;
    for (int o = kWave / 2; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, kWave));
    return (int)fminf(fmaxf(floorf(log2f(64.0f / fmaxf(a, 1e-30f))), -40.0f), 40.0f);
}

// 8 scaled weights -> the hi and the lo halves: rows 2 pr and 2 pr + 1 of the stream
__device__ __forceinline__ void store_pair(uint4* ws, long long pr, int lane, const float (&w)[8]) {
    half8_t hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        hi[j] = (_Float16)w[j];
        lo[j] = (_Float16)(w[j] - (float)hi[j]);
    }
    ws[(2 * pr) * kWave + lane] = __builtin_bit_cast(uint4, hi);
    ws[(2 * pr + 1) * kWave + lane] = __builtin_bit_cast(uint4, lo);
}

// A fragment whose k index runs over an accumulator tile's rows: element j = X[f0 + 8 (j >> 2) + (j & 3)][n], where
// X[f][n] = W[n * ld + f] (a Linear weight [out, in] read as [in, out]); f0 and ld multiples of 4
__device__ __forceinline__ void acc_order_weights(const float* W, int ld, int n, int f0, bool vec, double mult, float (&w)[8]) {
    const float* p = W + (size_t)n * ld + f0;
    float v[8];
    if (vec) {
        const float4 lo4 = *reinterpret_cast<const float4*>(p);
        const float4 hi4 = *reinterpret_cast<const float4*>(p + 8);
        v[0] = lo4.x; v[1] = lo4.y; v[2] = lo4.z; v[3] = lo4.w; v[4] = hi4.x; v[5] = hi4.y; v[6] = hi4.z; v[7] = hi4.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[8 * (j >> 2) + (j & 3)];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (float)((double)v[j] * mult);
}

}  // namespace risvec
