// clip_grad_norm_ -> torch.optim.Adam.step() -> the Polyak blend of the target, for any number of networks ("groups": one
// clip scope and one Adam instance each) in TWO launches, or one without clipping:
//     k_adam_sqsum   partials[block] = sum of fl32(g g) over the block's chunk of one gradient tensor, added up in float64
//     k_adam_step    every workgroup adds up its group's partials in one fixed order (so all of a group's workgroups hold
//                    the same bits), norm = fl32(sqrt(sum)), coef = min(max_norm / (norm + 1e-6), 1) in float32 as
//                    clip_grad_norm_ states it, then per element, every operation rounded to float32 on its own:
//                        g = grad coef (+ weight_decay param)         m = m + (g - m)(1 - beta1)
//                        v = v beta2 + ((1 - beta2) g) g              p = p - (step_size m) / (sqrt(v) / bc2_sqrt + eps)
//                        target = tau p + (1 - tau) target            (k_soft_update's blend, same bits)
// No fused multiply-add anywhere (hipcc contracts by default, hence the pragma), no atomics, and `/` and sqrtf are the
// correctly rounded ones hipcc emits by default (the Makefile passes no fast-math switch).
//
// The descriptors live in device memory (RisVecAdamTensor, RisVecAdamGroup) with block_tensor[b] = the tensor of workgroup
// b, so neither the tensor count nor the group count is bounded by the argument block.  A workgroup owns one chunk of
// kAdamChunk elements of one tensor: elements [c kAdamChunk, (c+1) kAdamChunk).  kAdamChunk is a multiple of 4, so every
// chunk starts at its tensor's offset from a 16-byte boundary: where all pointers of a descriptor share that offset the
// chunk goes 16 bytes at a time between its first and last boundary, with the floats in front and behind (at most 3 each)
// done singly; elsewhere it goes float by float.  Every element has one reader-writer.
#include "risvec_launch.hpp"

#pragma clang fp contract(off)

namespace risvec {
namespace {

constexpr int kAdBlock = 256;
constexpr int kAdVec = kAdamChunk / (4 * kAdBlock);           // float4 per thread
static_assert(kAdVec * 4 * kAdBlock == kAdamChunk && kAdBlock == 4 * kWave, "chunk = 256 threads x whole float4s");

struct AdamArgs {
    const RisVecAdamTensor* tensors;
    const RisVecAdamGroup* groups;
    const int32_t* block_tensor;
    double* partials;
    float* norms;
    double bc1;                                               // 1 - beta1^t
    float omb1, b2, omb2, bc2_sqrt, eps, tau, omt;
    int n_tensors, n_groups;
    uint32_t flags;
};

__device__ __forceinline__ int phase_of(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

// the sum of the 256 threads' values in one fixed order, returned to every thread
__device__ __forceinline__ double block_sum(double x, double* lds) {
    const int tid = threadIdx.x;
    lds[tid] = x;
    __syncthreads();
#pragma unroll
    for (int s = kAdBlock / 2; s > 0; s >>= 1) {
        if (tid < s) lds[tid] += lds[tid + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double sq(float g) {
    const float s = g * g;                                    // one float32 rounding per square
    return (double)s;
}

__global__ void __launch_bounds__(kAdBlock)
k_adam_sqsum(AdamArgs A) {
    __shared__ double lds[kAdBlock];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ti = A.block_tensor[b];
    double acc = 0.0;
    if (ti >= 0 && ti < A.n_tensors) {
        const RisVecAdamTensor d = A.tensors[ti];
        const long long lo = (long long)(b - d.first_block) * kAdamChunk;
        const long long len = d.numel - lo < kAdamChunk ? d.numel - lo : kAdamChunk;
        if (lo >= 0 && len > 0) {
            const float* g = d.grad + lo;
            const int hd = (4 - phase_of(g)) & 3;
            const int head = hd < len ? hd : (int)len, n4 = (int)(len - head) / 4, tail = head + 4 * n4;
            if (tid < head) acc += sq(g[tid]);
            const float4* g4 = reinterpret_cast<const float4*>(g + head);
#pragma unroll
            for (int k = 0; k < kAdVec; ++k) {
                const int e = k * kAdBlock + tid;
                if (e < n4) {
                    const float4 x = g4[e];
                    acc += sq(x.x); acc += sq(x.y); acc += sq(x.z); acc += sq(x.w);
                }
            }
            const int e = tail + (tid - kWave);               // at most 3 floats
            if (tid >= kWave && e < len) acc += sq(g[e]);
        }
    }
    const double s = block_sum(acc, lds);
    if (tid == 0) A.partials[b] = s;
}

struct Hyper {
    float coef, wd, omb1, b2, omb2, bc2_sqrt, eps, step, tau, omt;
};

// one element; gr leaves as the clipped gradient
__device__ __forceinline__ void adam1(float& p, float& gr, float& m, float& v, const Hyper& h) {
    float g = gr * h.coef;
    gr = g;
    if (h.wd != 0.f) {
        const float d = h.wd * p;
        g = g + d;
    }
    const float dm = g - m;
    const float wm = dm * h.omb1;
    m = m + wm;
    const float vb = v * h.b2;
    const float wg = h.omb2 * g;
    const float gg = wg * g;
    v = vb + gg;
    const float r = sqrtf(v) / h.bc2_sqrt;
    const float denom = r + h.eps;
    const float sm = h.step * m;
    const float u = sm / denom;
    p = p - u;
}

__device__ __forceinline__ float blend(float on, float tg, float tau, float omt) {
    const float a = tau * on;
    const float b = omt * tg;
    return a + b;
}

__global__ void __launch_bounds__(kAdBlock)
k_adam_step(AdamArgs A) {
    __shared__ double lds[kAdBlock];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ti = A.block_tensor[b];
    if (ti < 0 || ti >= A.n_tensors) return;                  // block-uniform
    const RisVecAdamTensor d = A.tensors[ti];
    if (d.group < 0 || d.group >= A.n_groups) return;
    const RisVecAdamGroup G = A.groups[d.group];
    Hyper h;
    h.coef = 1.f;
    if (A.flags & RISVEC_ADAM_CLIP) {
        double acc = 0.0;
        for (int i = tid; i < G.n_blocks; i += kAdBlock) acc += A.partials[G.first_block + i];
        const double sum = block_sum(acc, lds);
        const float norm = (float)sqrt(sum);
        if (b == G.first_block && tid == 0) A.norms[d.group] = norm;
        if (G.max_norm >= 0.f) {                              // clip_grad_norm_: max_norm / (total_norm + 1e-6), clamp(max=1)
            const float c = G.max_norm / (norm + 1e-6f);
            h.coef = c > 1.f ? 1.f : c;                       // a NaN stays a NaN, as torch.clamp leaves it
        }
    }
    h.wd = G.weight_decay;
    h.omb1 = A.omb1; h.b2 = A.b2; h.omb2 = A.omb2; h.bc2_sqrt = A.bc2_sqrt; h.eps = A.eps;
    h.step = (float)(G.lr / A.bc1);                           // the double quotient, rounded once
    h.tau = A.tau; h.omt = A.omt;

    const long long lo = (long long)(b - d.first_block) * kAdamChunk;
    const long long len64 = d.numel - lo < kAdamChunk ? d.numel - lo : kAdamChunk;
    if (lo < 0 || len64 <= 0) return;
    const int len = (int)len64;
    float* p = d.param + lo;
    float* gr = d.grad + lo;
    float* m = d.exp_avg + lo;
    float* v = d.exp_avg_sq + lo;
    float* tg = ((A.flags & RISVEC_ADAM_BLEND) && d.target) ? d.target + lo : nullptr;
    const bool wr_grad = (A.flags & RISVEC_ADAM_WRITE_GRAD) != 0;

    auto one = [&](int e) {
        float pe = p[e], ge = gr[e], me = m[e], ve = v[e];
        adam1(pe, ge, me, ve, h);
        p[e] = pe; m[e] = me; v[e] = ve;
        if (wr_grad) gr[e] = ge;
        if (tg) tg[e] = blend(pe, tg[e], h.tau, h.omt);
    };

    const int ph = phase_of(p);
    const bool vec = phase_of(gr) == ph && phase_of(m) == ph && phase_of(v) == ph && (!tg || phase_of(tg) == ph);
    if (vec) {
        const int hd = (4 - ph) & 3;
        const int head = hd < len ? hd : len, n4 = (len - head) / 4, tail = head + 4 * n4;
        if (tid < head) one(tid);
        {
            const int e = tail + (tid - kWave);               // at most 3 floats
            if (tid >= kWave && e < len) one(e);
        }
        float4* p4 = reinterpret_cast<float4*>(p + head);
        float4* g4 = reinterpret_cast<float4*>(gr + head);
        float4* m4 = reinterpret_cast<float4*>(m + head);
        float4* v4 = reinterpret_cast<float4*>(v + head);
        float4* t4 = tg ? reinterpret_cast<float4*>(tg + head) : nullptr;
        float4 vp[kAdVec], vg[kAdVec], vm[kAdVec], vv[kAdVec], vt[kAdVec];
#pragma unroll
        for (int k = 0; k < kAdVec; ++k) {
            const int e = k * kAdBlock + tid;
            if (e < n4) {
                vp[k] = p4[e]; vg[k] = g4[e]; vm[k] = m4[e]; vv[k] = v4[e];
                if (t4) vt[k] = t4[e];
            }
        }
#pragma unroll
        for (int k = 0; k < kAdVec; ++k) {
            const int e = k * kAdBlock + tid;
            if (e < n4) {
                adam1(vp[k].x, vg[k].x, vm[k].x, vv[k].x, h);
                adam1(vp[k].y, vg[k].y, vm[k].y, vv[k].y, h);
                adam1(vp[k].z, vg[k].z, vm[k].z, vv[k].z, h);
                adam1(vp[k].w, vg[k].w, vm[k].w, vv[k].w, h);
                p4[e] = vp[k]; m4[e] = vm[k]; v4[e] = vv[k];
                if (wr_grad) g4[e] = vg[k];
                if (t4)
                    t4[e] = make_float4(blend(vp[k].x, vt[k].x, h.tau, h.omt), blend(vp[k].y, vt[k].y, h.tau, h.omt),
                                        blend(vp[k].z, vt[k].z, h.tau, h.omt), blend(vp[k].w, vt[k].w, h.tau, h.omt));
            }
        }
    } else {
#pragma unroll 4
        for (int k = 0; k < 4 * kAdVec; ++k) {
            const int e = k * kAdBlock + tid;
            if (e < len) one(e);
        }
    }
}

}  // namespace

hipError_t launch_adam_step(const AdamLaunch& a, hipStream_t st) {
    AdamArgs A{};
    A.tensors = a.tensors; A.groups = a.groups; A.block_tensor = a.block_tensor;
    A.partials = a.partials; A.norms = a.norms;
    A.bc1 = a.bc1;
    A.omb1 = a.omb1; A.b2 = a.b2; A.omb2 = a.omb2; A.bc2_sqrt = a.bc2_sqrt; A.eps = a.eps; A.tau = a.tau; A.omt = a.omt;
    A.n_tensors = a.n_tensors; A.n_groups = a.n_groups; A.flags = a.flags;
    if (a.n_blocks < 1) return hipErrorInvalidValue;
    if (a.flags & RISVEC_ADAM_CLIP) {
        note_kernel("k_adam_sqsum + k_adam_step");
        hipLaunchKernelGGL(k_adam_sqsum, dim3((unsigned)a.n_blocks), dim3(kAdBlock), 0, st, A);
        if (hipError_t err = hipGetLastError()) return err;
    } else {
        note_kernel("k_adam_step");
    }
    hipLaunchKernelGGL(k_adam_step, dim3((unsigned)a.n_blocks), dim3(kAdBlock), 0, st, A);
    return hipGetLastError();
}

}  // namespace risvec
