// The Polyak blend that ends every learn() of the single-agent (DDPG) learner, update_network_parameters
// (Simulation-SARL/ddpg_torch.py:104-130), for up to 32 tensors in ONE launch:
//     target[i] = fl32( fl32(tau * online[i]) + fl32(one_minus_tau * target[i]) )
// two rounded products and one rounded sum -- `tau * a + (1 - tau) * b` on float32 tensors, statement by statement.
// A fused multiply-add rounds once where the reference rounds twice and gives other bits in about a quarter of the
// elements, hence the pragma below (hipcc contracts by default).
//
// The pointers and element counts travel by value in the kernel's argument block, with the first workgroup of every
// tensor: a workgroup finds its tensor by walking that list (wave-uniform, <= 32 steps).  A workgroup blends 1024
// float4 where the two pointers of a pair sit at the same offset from a 16-byte boundary (the floats in front of the
// first boundary and behind the last whole float4 are left to the tensor's first workgroup), and 4096 single floats
// where they do not.  Every element has one reader-writer: the update is in place and nothing else is touched.
#include "risvec_launch.hpp"

#pragma clang fp contract(off)

namespace risvec {
namespace {

constexpr int kSuBlock = 256;
constexpr int kSuVec = 4;                        // float4 (or runs of 4 floats) per thread
constexpr long long kSuChunk = (long long)kSuBlock * kSuVec;       // float4 per workgroup

struct SoftArgs {
    const float* online[kSoftUpdateMax];
    float* target[kSoftUpdateMax];
    long long numel[kSoftUpdateMax];
    int first[kSoftUpdateMax + 1];               // first workgroup of tensor i; first[n_tensors] = the grid
    int n_tensors;
    float tau, omt;
};

__host__ __device__ inline bool same_phase(const float* a, const float* b) {
    return ((reinterpret_cast<uintptr_t>(a) ^ reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
}
// floats in front of the first 16-byte boundary
__host__ __device__ inline long long head_of(const float* p, long long n) {
    const long long h = (4 - (long long)((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3;
    return h < n ? h : n;
}

__device__ __forceinline__ float blend(float on, float tg, float tau, float omt) {
    const float a = tau * on;
    const float b = omt * tg;
    return a + b;
}

__global__ void __launch_bounds__(kSuBlock)
k_soft_update(SoftArgs A) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int i = 0;
    while (i + 1 < A.n_tensors && b >= A.first[i + 1]) ++i;      // block-uniform
    const long long c = b - A.first[i];
    const float* on = A.online[i];
    float* tg = A.target[i];
    const long long n = A.numel[i];
    const float tau = A.tau, omt = A.omt;
    if (same_phase(on, tg)) {
        const long long head = head_of(tg, n), n4 = (n - head) / 4, tail = head + 4 * n4;
        if (c == 0) {
            if (tid < head) tg[tid] = blend(on[tid], tg[tid], tau, omt);
            const long long e = tail + (tid - kWave);            // at most 3 floats
            if (tid >= kWave && e < n) tg[e] = blend(on[e], tg[e], tau, omt);
        }
        const float4* o4 = reinterpret_cast<const float4*>(on + head);
        float4* t4 = reinterpret_cast<float4*>(tg + head);
        float4 vo[kSuVec], vt[kSuVec];
#pragma unroll
        for (int k = 0; k < kSuVec; ++k) {
            const long long e = c * kSuChunk + k * kSuBlock + tid;
            if (e < n4) { vo[k] = o4[e]; vt[k] = t4[e]; }
        }
#pragma unroll
        for (int k = 0; k < kSuVec; ++k) {
            const long long e = c * kSuChunk + k * kSuBlock + tid;
            if (e < n4)
                t4[e] = make_float4(blend(vo[k].x, vt[k].x, tau, omt), blend(vo[k].y, vt[k].y, tau, omt),
                                    blend(vo[k].z, vt[k].z, tau, omt), blend(vo[k].w, vt[k].w, tau, omt));
        }
    } else {
#pragma unroll 4
        for (int k = 0; k < 4 * kSuVec; ++k) {
            const long long e = c * (4 * kSuChunk) + k * kSuBlock + tid;
            if (e < n) tg[e] = blend(on[e], tg[e], tau, omt);
        }
    }
}

}  // namespace

hipError_t launch_soft_update(int n_tensors, const float* const* online, float* const* target, const int64_t* numel,
                              float tau, float one_minus_tau, hipStream_t st) {
    if (n_tensors < 1 || n_tensors > kSoftUpdateMax) return hipErrorInvalidValue;
    SoftArgs a{};
    long long blocks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const long long n = numel[i];
        a.online[i] = online[i];
        a.target[i] = target[i];
        a.numel[i] = n;
        a.first[i] = (int)blocks;
        long long nb;
        if (same_phase(online[i], target[i])) {
            const long long n4 = (n - head_of(target[i], n)) / 4;
            nb = n4 > 0 ? (n4 + kSuChunk - 1) / kSuChunk : 1;
        } else {
            nb = (n + 4 * kSuChunk - 1) / (4 * kSuChunk);
        }
        blocks += nb;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    }
    a.first[n_tensors] = (int)blocks;
    a.n_tensors = n_tensors;
    a.tau = tau;
    a.omt = one_minus_tau;
    note_kernel("k_soft_update");
    hipLaunchKernelGGL(k_soft_update, dim3((unsigned)blocks), dim3(kSuBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace risvec
