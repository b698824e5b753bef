// ppo_opt.hip — one optimiser step of the PPO update on the device (include/heligym_amd.h, hg_ppo_adam):
// the early-stop and non-finite guards, global gradient-norm clipping and Adam over the flat 5641-float
// parameter vector, with its counters, in one launch.
//
// Shape.  ONE block of 1024 threads (16 waves): the state's counters are read by every thread before a
// barrier and rewritten by thread 0 after it, so there is nothing to order between blocks, no ticket, no
// fence and no atomic.  Thread t owns the elements t, t + 1024, .. (at most 6).  Every load of the step
// (gradient, theta, m, v: 24 per thread) is issued before the first barrier; what is left behind it is the
// 22 KB reduction and the element-wise update.
// The norm.  Thread t: s = fma(g, g, s) over its elements in ascending order from 0; the wave's sum by the
// xor butterfly 32, 16, .. 1; the 16 wave sums added in wave order.  All of it a function of compile-time
// constants, so two calls on equal inputs give equal bits.
// The bias corrections lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) are formed in fp64 by one thread
// (beta^t by squaring, at most 31 trips) while the others wait at the reduction's barrier, and rounded to
// fp32 once; everything per element is fp32.
#include "ppo_opt.h"

namespace hgk {
namespace {

constexpr int kAdamThreads = 1024, kAdamWaves = kAdamThreads / 64;
constexpr int kAdamPer = (kPpoParams + kAdamThreads - 1) / kAdamThreads;

__device__ __forceinline__ double pow_int(double b, uint32_t n) {
    double r = 1.0;
    for (; n; n >>= 1) {
        if (n & 1) r = r * b;
        b = b * b;
    }
    return r;
}

__global__ __launch_bounds__(kAdamThreads) void ppo_adam_kernel(const PpoAdamArgs a) {
    __shared__ float s_part[kAdamWaves];
    __shared__ float s_corr[2];   // lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* const tail = a.state + kOptTail;
    float* const mp = reinterpret_cast<float*>(a.state) + kOptM;
    float* const vp = reinterpret_cast<float*>(a.state) + kOptV;
    const uint32_t applied = tail[kOptApplied], seen = tail[kOptSeen], stop = tail[kOptStop];
    const uint32_t n_nonfinite = tail[kOptSkippedNonfinite], n_stopped = tail[kOptSkippedStopped];
    const float kl = (a.target_kl > 0.0f && a.stats != nullptr) ? a.stats[2] : 0.0f;
    float g[kAdamPer], th[kAdamPer], m[kAdamPer], v[kAdamPer];
#pragma unroll
    for (int u = 0; u < kAdamPer; ++u) {
        const int e = tid + u * kAdamThreads;
        const bool in = e < kPpoParams;
        g[u] = in ? a.grad[e] : 0.0f;
        th[u] = in ? a.theta[e] : 0.0f;
        m[u] = in ? mp[e] : 0.0f;
        v[u] = in ? vp[e] : 0.0f;
    }
    const bool stop_now = a.target_kl > 0.0f && a.stats != nullptr && kl > 1.5f * a.target_kl;
    float s = 0.0f;
#pragma unroll
    for (int u = 0; u < kAdamPer; ++u) s = fmaf(g[u], g[u], s);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s = s + __shfl_xor(s, k, 64);
    if (lane == 0) s_part[wave] = s;
    if (tid == kAdamThreads - 64) {
        const uint32_t t = applied + 1u;
        const double lr = a.lr_dev ? (double)a.lr_dev[0] : a.lr;
        s_corr[0] = (float)(lr / (1.0 - pow_int(a.beta1, t)));
        s_corr[1] = (float)(1.0 / sqrt(1.0 - pow_int(a.beta2, t)));
    }
    __syncthreads();   // (and: every thread has read the tail before thread 0 rewrites it)
    if (stop != 0u || stop_now) {
        if (tid == 0) {
            tail[kOptSeen] = seen + 1u;
            if (stop == 0u) tail[kOptStop] = 1u;
            tail[kOptSkippedStopped] = n_stopped + 1u;
        }
        return;
    }
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < kAdamWaves; ++w) tot = tot + s_part[w];
    const float nrm = sqrtf(tot);
    if (!(fabsf(nrm) <= 3.402823466e+38f)) {   // NaN or infinite: theta, m and v stay as they are
        if (tid == 0) {
            tail[kOptSeen] = seen + 1u;
            tail[kOptSkippedNonfinite] = n_nonfinite + 1u;
            reinterpret_cast<float*>(tail)[kOptNorm] = nrm;
        }
        return;
    }
    float c = 1.0f;
    if (a.max_norm > 0.0f) {
        const float q = a.max_norm / (nrm + 1e-6f);
        c = fminf(1.0f, q);
    }
    const float step = s_corr[0], rs2 = s_corr[1];
#pragma unroll
    for (int u = 0; u < kAdamPer; ++u) {
        const int e = tid + u * kAdamThreads;
        if (e < kPpoParams) {
            const float gp = c * g[u];
            const float gm = a.omb1 * gp;
            const float mn = fmaf(a.b1, m[u], gm);
            const float gv = a.omb2 * gp;
            const float gv2 = gv * gp;
            const float vn = fmaf(a.b2, v[u], gv2);
            const float den = fmaf(sqrtf(vn), rs2, a.eps);
            const float r = mn / den;
            mp[e] = mn;
            vp[e] = vn;
            a.theta[e] = fmaf(-step, r, th[u]);
        }
    }
    if (tid == 0) {
        tail[kOptApplied] = applied + 1u;
        tail[kOptSeen] = seen + 1u;
        reinterpret_cast<float*>(tail)[kOptNorm] = nrm;
        reinterpret_cast<float*>(tail)[kOptClipCoef] = c;
    }
}

// hg_ppo_opt_init: a kernel rather than a memset, so that a captured call is a kernel node like the rest
__global__ __launch_bounds__(kAdamThreads) void ppo_opt_zero_kernel(uint32_t* __restrict__ state) {
    for (int e = threadIdx.x; e < kOptWords; e += kAdamThreads) state[e] = 0u;
}

}  // namespace

hipError_t launch_ppo_opt_zero(uint32_t* state, hipStream_t stream) {
    hipLaunchKernelGGL(ppo_opt_zero_kernel, dim3(1), dim3(kAdamThreads), 0, stream, state);
    return hipGetLastError();
}

hipError_t launch_ppo_adam(const PpoAdamArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(ppo_adam_kernel, dim3(1), dim3(kAdamThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hgk
