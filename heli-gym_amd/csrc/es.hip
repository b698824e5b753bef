// es.hip — populations of policies and an evolution-strategies learner on the device
// (include/heligym_amd.h: hg_pop_pack, hg_es_perturb, hg_es_noise, hg_pop_fitness, hg_es_grad).  The
// population rollout itself is heligym_amd.hip's (rollout_pop_kernel, beside step_body).
//
// Images.  One thread per element of a packed image (policy_mlp.h's layout): image_value() maps the
// element's index back to the parameter it carries -- the inverse of the gather policy_pack_kernel and
// value_pack_kernel do -- and reads it through a functor, so hg_pop_pack (the functor loads theta_p) and
// hg_es_perturb (the functor forms fma(+-sigma, eps, theta) from the counters) write the same bits for the
// same parameters and no [P,5641] intermediate exists unless the caller asks for it.
// Noise.  eps_j[i] is normal i & 3 of ONE Philox4x32-10 call on (i >> 2, j, g_lo, g_hi), Box-Muller as the
// policy noise's (policy_mlp.h, policy_action); es_normals() is the only place it is formed, for the
// perturbation, the export and the gradient alike.
// Orders of summation (all functions of the arguments and compile-time constants):
//   fitness   per env an fp64 chain over k ascending; thread t of the member's block adds its envs t, t + 256,
//             .. ascending; the 256 thread sums by the halving tree s[t] += s[t + w], w = 128, 64, .. 1.
//   gradient  per (parameter, chunk of kEsPairChunk consecutive pairs) an fp32 fma chain over the pairs
//             ascending from 0; the chunks' partials added ascending from 0 by the parameter's own thread; one
//             multiplication by -1/(P sigma).
//   norm      hg_ppo_adam's: per thread an fma chain over its elements t, t + 1024, ..; the xor butterfly
//             32, 16, .. 1 in the wave; the 16 wave sums in wave order.
//   stats     per thread p = t, t + 1024, .. ascending (fp64 sum, min, max, count, first best); the halving
//             tree over the 1024 threads, a tie of the best value going to the lower index.
#include "es.h"

// Philox4x32-10 and u01 as heligym_amd.hip states them (tests/philox_ref.py restates both bitwise)
struct U4 {
    uint32_t x, y, z, w;
};
__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
__device__ __forceinline__ float u01(uint32_t x) {
    return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f);
}
#include "policy_mlp.h"   // the image's layout (after philox / u01, as in heligym_amd.hip)

namespace hgk {
namespace {

static_assert(kEsImageFloats == hgp::kPolicyFloats, "image size");

__device__ __forceinline__ uint64_t es_generation(const EsNoiseKey& key) {
    return (uint64_t)(key.gen + (key.gen_dev ? (int64_t)key.gen_dev[0] : 0));
}

// the four normals of parameter quad `quad` of pair `pair` in generation g
__device__ __forceinline__ void es_normals(uint32_t quad, uint32_t pair, uint64_t g, uint32_t k0, uint32_t k1,
                                           float z[4]) {
    const U4 r = philox(U4{quad, pair, (uint32_t)g, (uint32_t)(g >> 32)}, k0, k1);
    const float r0 = sqrtf(__log2f(u01(r.x)) * -1.38629436111989061f);   // sqrt(-2 ln u)
    const float r1 = sqrtf(__log2f(u01(r.z)) * -1.38629436111989061f);
    const float a1 = __uint_as_float((r.y >> 9) | 0x3f800000u), a3 = __uint_as_float((r.w >> 9) | 0x3f800000u);
    z[0] = r0 * __builtin_amdgcn_cosf(a1);
    z[1] = r0 * __builtin_amdgcn_sinf(a1);
    z[2] = r1 * __builtin_amdgcn_cosf(a3);
    z[3] = r1 * __builtin_amdgcn_sinf(a3);
}

// Element idx of the packed image of the parameters th(0 .. 5641): what policy_pack_kernel (with log_std
// when stochastic) and value_pack_kernel leave there.
template <class F>
__device__ __forceinline__ float image_value(int idx, F th, bool stochastic, const float* mean, const float* scale) {
    using namespace hgp;
    if (idx < kHeadFloats) {
        if (idx < kStdOff + 4) return stochastic ? expf(th(kPpoLogStd + idx - kStdOff)) : 0.f;
        if (idx == kStochOff) return stochastic ? 1.f : 0.f;
        if (idx == kLogStdSumOff)
            return stochastic ? ((th(kPpoLogStd) + th(kPpoLogStd + 1)) + th(kPpoLogStd + 2)) + th(kPpoLogStd + 3) : 0.f;
        if (idx >= kMeanOff && idx < kMeanOff + 17) return mean ? mean[idx - kMeanOff] : 0.f;
        if (idx >= kScaleOff && idx < kScaleOff + 17) return scale ? scale[idx - kScaleOff] : 1.f;
        return 0.f;
    }
    const int s = (idx - kHeadFloats) >> 6, l = (idx - kHeadFloats) & 63;
    const int h = l >> 5, i = l & 31;
    if (s < kL1Slots) {
        const int mt = s / kL1Steps, k = 2 * (s % kL1Steps) + h, row = 32 * mt + i;
        return k < 17 ? th(kPpoW1 + row * 17 + k) : th(kPpoB1 + row);
    }
    if (s < kL1Slots + kL2Slots) {
        const int s2 = s - kL1Slots, mt = s2 / kL2Steps, kp = s2 % kL2Steps, row = 32 * mt + i;
        if (kp < 32) return th(kPpoW2 + row * 64 + acc_row(kp >> 4, kp & 15, h));
        return h == 0 ? th(kPpoB2 + row) : 0.f;
    }
    const int kp = s - kL1Slots - kL2Slots;
    if (i < 8) {
        const int o = i & 3;
        if (kp < 32) return th(kPpoW3 + o * 64 + acc_row(kp >> 4, kp & 15, h));
        return h == 0 ? th(kPpoB3 + o) : 0.f;
    }
    if (i == kValueRowLo || i == kValueRowHi) {
        if (kp < 32) return th(kPpoWv + acc_row(kp >> 4, kp & 15, h));
        return h == 0 ? th(kPpoBv) : 0.f;
    }
    return 0.f;
}

// hg_pop_pack: block (p, y) writes elements 256 y .. of image p
__global__ __launch_bounds__(kEsBlock) void pop_pack_kernel(const float* __restrict__ theta, int stochastic,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ scale, float* __restrict__ images) {
    const int idx = (int)(blockIdx.y * kEsBlock + threadIdx.x);
    if (idx >= kEsImageFloats) return;
    const float* th_p = theta + (size_t)blockIdx.x * kPpoParams;
    images[(size_t)blockIdx.x * kEsImageFloats + idx] =
        image_value(idx, [&](int i) { return th_p[i]; }, stochastic != 0, mean, scale);
}

// hg_es_perturb: block (j, y) writes elements 256 y .. of the images of members 2 j and 2 j + 1 and, past the
// image's 7552, of their parameter vectors.
__global__ __launch_bounds__(kEsBlock) void es_perturb_kernel(const float* __restrict__ theta, float sigma,
                                                              const EsNoiseKey key, int stochastic,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ scale, float* __restrict__ images,
                                                              float* __restrict__ member_theta) {
    const int idx = (int)(blockIdx.y * kEsBlock + threadIdx.x);
    const uint32_t pair = blockIdx.x;
    const uint64_t g = es_generation(key);
    auto member = [&](float sg) {
        return [=](int i) {
            const float t = theta[i];
            if (i >= kEsPerturbed) return t;
            float z[4];
            es_normals((uint32_t)i >> 2, pair, g, key.k0, key.k1, z);
            const float e = (i & 2) ? ((i & 1) ? z[3] : z[2]) : ((i & 1) ? z[1] : z[0]);
            return fmaf(sg, e, t);
        };
    };
    if (idx < kEsImageFloats) {
        float* im = images + (size_t)(2 * pair) * kEsImageFloats + idx;
        im[0] = image_value(idx, member(sigma), stochastic != 0, mean, scale);
        im[kEsImageFloats] = image_value(idx, member(-sigma), stochastic != 0, mean, scale);
    } else if (member_theta != nullptr && idx < kEsImageFloats + kPpoParams) {
        const int i = idx - kEsImageFloats;
        float* mt = member_theta + (size_t)(2 * pair) * kPpoParams + i;
        mt[0] = member(sigma)(i);
        mt[kPpoParams] = member(-sigma)(i);
    }
}

// hg_es_noise: one thread per quad
__global__ __launch_bounds__(kEsBlock) void es_noise_kernel(const EsNoiseKey key, uint32_t pair, float* __restrict__ out) {
    const int q = (int)(blockIdx.x * kEsBlock + threadIdx.x);
    if (q >= kEsQuads) return;
    float z[4];
    es_normals((uint32_t)q, pair, es_generation(key), key.k0, key.k1, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) out[4 * q + c] = z[c];
}

// hg_pop_fitness: block p sums member p's envs (the order: the head of this file)
__global__ __launch_bounds__(kEsBlock) void pop_fitness_kernel(const PopFitnessArgs a) {
    __shared__ double s_sum[kEsBlock];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * a.epm;
    const int64_t cnt = a.N - base < a.epm ? a.N - base : a.epm;
    double acc = 0.0;
    for (int64_t e = t; e < cnt; e += kEsBlock) {
        const int64_t n = base + e;
        double es = 0.0;
        if (!a.first_episode) {
            for (int32_t k = 0; k < a.K; ++k) es = es + (double)a.reward[(int64_t)k * a.N + n];
        } else {
            bool alive = a.restart ? true : a.alive[n] != 0;
            for (int32_t k = 0; k < a.K; ++k) {
                const int64_t at = (int64_t)k * a.N + n;
                const double r = (double)a.reward[at];
                const bool done = (a.terminated[at] | a.truncated[at]) != 0;
                es = alive ? es + r : es;   // by selection: nothing of a finished env's rows enters
                alive = alive && !done;
            }
            a.alive[n] = alive ? 1 : 0;
        }
        acc = acc + es;
    }
    s_sum[t] = acc;
    __syncthreads();
#pragma unroll
    for (int w = kEsBlock / 2; w >= 1; w >>= 1) {
        if (t < w) s_sum[t] = s_sum[t] + s_sum[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double before = a.restart ? 0.0 : a.sum[blockIdx.x];
        const double tot = before + s_sum[0];
        a.sum[blockIdx.x] = tot;
        a.fitness[blockIdx.x] = (float)(tot / (double)cnt);
    }
}

// a fitness as the ranks order it: every non-finite value (NaN included) is -inf
__device__ __forceinline__ float rank_key(float f) {
    return fabsf(f) <= 3.402823466e+38f ? f : -__builtin_huge_valf();
}

// hg_es_grad, first launch: u_p = r_p / (P - 1) - 1/2, r_p = #{q: f_q < f_p} + #{q < p: f_q == f_p}.  The
// division is formed in fp64 and rounded to fp32 once, which is the correctly rounded fp32 quotient (both
// operands are integers below 2^24 and fp64 carries more than 2 * 24 + 2 bits).
// The P keys pass through LDS in tiles of kEsRankTile (each thread stages four, then every thread reads the
// tile as broadcast quads); the count is an integer, so its order does not matter.
__global__ __launch_bounds__(kEsBlock) void es_rank_kernel(const float* __restrict__ fitness, int32_t P,
                                                           float* __restrict__ u) {
    __shared__ float4 s_key[kEsRankTile / 4];
    const int p = (int)(blockIdx.x * kEsBlock + threadIdx.x);
    const float fp = p < P ? rank_key(fitness[p]) : 0.f;
    int32_t r = 0;
    for (int q0 = 0; q0 < P; q0 += kEsRankTile) {
        float k[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // past the end: +inf, which counts for no one (a key is never above it)
            const int q = q0 + 4 * (int)threadIdx.x + c;
            k[c] = q < P ? rank_key(fitness[q]) : __builtin_huge_valf();
        }
        __syncthreads();   // (the previous tile has been read)
        s_key[threadIdx.x] = make_float4(k[0], k[1], k[2], k[3]);
        __syncthreads();
        const int quads = (P - q0 < kEsRankTile ? P - q0 + 3 : kEsRankTile) / 4;
        for (int j = 0; j < quads; ++j) {
            const float4 f = s_key[j];
            const int q = q0 + 4 * j;
            r += (f.x < fp || (f.x == fp && q + 0 < p)) ? 1 : 0;
            r += (f.y < fp || (f.y == fp && q + 1 < p)) ? 1 : 0;
            r += (f.z < fp || (f.z == fp && q + 2 < p)) ? 1 : 0;
            r += (f.w < fp || (f.w == fp && q + 3 < p)) ? 1 : 0;
        }
    }
    if (p >= P) return;
    const float quot = (float)((double)r / (double)(P - 1));
    u[p] = quot - 0.5f;
}

// second launch: block (x, c), thread = parameter quad, the fma chain over the pairs of chunk c
__global__ __launch_bounds__(kEsBlock) void es_partial_kernel(const EsGradArgs a) {
    const int q = (int)(blockIdx.x * kEsBlock + threadIdx.x);
    if (q >= kEsQuads) return;
    const uint64_t g = es_generation(a.key);
    const int pairs = a.P / 2, j0 = (int)blockIdx.y * kEsPairChunk;
    const int j1 = j0 + kEsPairChunk < pairs ? j0 + kEsPairChunk : pairs;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = j0; j < j1; ++j) {
        const float w = a.ws[2 * j] - a.ws[2 * j + 1];
        float z[4];
        es_normals((uint32_t)q, (uint32_t)j, g, a.key.k0, a.key.k1, z);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = fmaf(w, z[c], acc[c]);
    }
    float* part = a.ws + es_u_floats(a.P) + (int64_t)blockIdx.y * kEsPerturbed + 4 * q;
    *reinterpret_cast<float4*>(part) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

constexpr int kEsReduceWaves = kEsReduceThreads / 64;
constexpr int kEsReducePer = (kPpoParams + kEsReduceThreads - 1) / kEsReduceThreads;

struct EsBest {
    float v;
    int32_t at;   // -1: none
};
__device__ __forceinline__ EsBest better(EsBest x, EsBest y) {   // the larger value; a tie to the lower index
    if (x.at < 0) return y;
    if (y.at < 0) return x;
    if (y.v > x.v || (y.v == x.v && y.at < x.at)) return y;
    return x;
}

// third launch: one thread per parameter adds the chunks' partials ascending and scales the sum
__global__ __launch_bounds__(kEsBlock) void es_sum_kernel(const EsGradArgs a) {
    const int e = (int)(blockIdx.x * kEsBlock + threadIdx.x);
    if (e >= kPpoParams) return;
    float gv = 0.0f;
    if (e < kEsPerturbed) {
        const int nc = (int)es_chunks(a.P);
        const float* part = a.ws + es_u_floats(a.P) + e;
        float s = 0.0f;
        for (int c = 0; c < nc; ++c) s = s + part[(int64_t)c * kEsPerturbed];
        gv = a.scale * s;
    }
    a.grad[e] = gv;
}

// fourth launch (only with stats): one block.  The gradient's norm and the fitness statistics.
__global__ __launch_bounds__(kEsReduceThreads) void es_stats_kernel(const EsGradArgs a) {
    __shared__ float s_part[kEsReduceWaves];
    __shared__ double s_sum[kEsReduceThreads];
    __shared__ float s_min[kEsReduceThreads], s_max[kEsReduceThreads];
    __shared__ int32_t s_bad[kEsReduceThreads];
    __shared__ EsBest s_best[kEsReduceThreads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float sq = 0.0f;
#pragma unroll
    for (int u = 0; u < kEsReducePer; ++u) {
        const int e = tid + u * kEsReduceThreads;
        if (e < kPpoParams) {
            const float gv = a.grad[e];
            sq = fmaf(gv, gv, sq);
        }
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) sq = sq + __shfl_xor(sq, k, 64);
    if (lane == 0) s_part[wave] = sq;
    double sum = 0.0;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    int32_t bad = 0;
    EsBest best{0.f, -1};
    for (int p = tid; p < a.P; p += kEsReduceThreads) {
        const float f = a.fitness[p];
        if (fabsf(f) <= 3.402823466e+38f) {
            sum = sum + (double)f;
            mn = fminf(mn, f);
            mx = fmaxf(mx, f);
            best = better(best, EsBest{f, p});
        } else {
            ++bad;
        }
    }
    s_sum[tid] = sum;
    s_min[tid] = mn;
    s_max[tid] = mx;
    s_bad[tid] = bad;
    s_best[tid] = best;
    __syncthreads();
    for (int w = kEsReduceThreads / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            s_sum[tid] = s_sum[tid] + s_sum[tid + w];
            s_min[tid] = fminf(s_min[tid], s_min[tid + w]);
            s_max[tid] = fmaxf(s_max[tid], s_max[tid + w]);
            s_bad[tid] = s_bad[tid] + s_bad[tid + w];
            s_best[tid] = better(s_best[tid], s_best[tid + w]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        float tot = 0.0f;
#pragma unroll
        for (int w = 0; w < kEsReduceWaves; ++w) tot = tot + s_part[w];
        const int32_t good = a.P - s_bad[0];
        const float nan = __uint_as_float(0x7fc00000u);
        a.stats[0] = good > 0 ? (float)(s_sum[0] / (double)good) : nan;
        a.stats[1] = good > 0 ? s_min[0] : nan;
        a.stats[2] = good > 0 ? s_max[0] : nan;
        a.stats[3] = (float)s_bad[0];
        a.stats[4] = (float)s_best[0].at;
        a.stats[5] = sqrtf(tot);
        a.stats[6] = 0.0f;
        a.stats[7] = 0.0f;
    }
}

}  // namespace

hipError_t launch_pop_pack(const float* theta, int64_t P, int stochastic, const float* mean, const float* scale,
                           float* images, hipStream_t stream) {
    const dim3 grid((unsigned)P, (kEsImageFloats + kEsBlock - 1) / kEsBlock);
    hipLaunchKernelGGL(pop_pack_kernel, grid, dim3(kEsBlock), 0, stream, theta, stochastic, mean, scale, images);
    return hipGetLastError();
}

hipError_t launch_es_perturb(const float* theta, int64_t P, float sigma, const EsNoiseKey& key, int stochastic,
                             const float* mean, const float* scale, float* images, float* member_theta,
                             hipStream_t stream) {
    const int elems = kEsImageFloats + (member_theta ? kPpoParams : 0);
    const dim3 grid((unsigned)(P / 2), (elems + kEsBlock - 1) / kEsBlock);
    hipLaunchKernelGGL(es_perturb_kernel, grid, dim3(kEsBlock), 0, stream, theta, sigma, key, stochastic, mean, scale,
                       images, member_theta);
    return hipGetLastError();
}

hipError_t launch_es_noise(const EsNoiseKey& key, uint32_t pair, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(es_noise_kernel, dim3((kEsQuads + kEsBlock - 1) / kEsBlock), dim3(kEsBlock), 0, stream, key, pair,
                       out);
    return hipGetLastError();
}

hipError_t launch_pop_fitness(const PopFitnessArgs& a, int64_t P, hipStream_t stream) {
    hipLaunchKernelGGL(pop_fitness_kernel, dim3((unsigned)P), dim3(kEsBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_es_grad(const EsGradArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(es_rank_kernel, dim3((a.P + kEsBlock - 1) / kEsBlock), dim3(kEsBlock), 0, stream, a.fitness, a.P,
                       a.ws);
    const dim3 grid((kEsQuads + kEsBlock - 1) / kEsBlock, (unsigned)es_chunks(a.P));
    hipLaunchKernelGGL(es_partial_kernel, grid, dim3(kEsBlock), 0, stream, a);
    hipLaunchKernelGGL(es_sum_kernel, dim3((kPpoParams + kEsBlock - 1) / kEsBlock), dim3(kEsBlock), 0, stream, a);
    if (a.stats != nullptr) hipLaunchKernelGGL(es_stats_kernel, dim3(1), dim3(kEsReduceThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hgk
