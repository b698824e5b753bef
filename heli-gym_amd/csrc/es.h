// es.h — launchers of the population / evolution-strategies kernels (es.hip), called by hg_pop_pack,
// hg_es_perturb, hg_es_noise, hg_pop_fitness and hg_es_grad (heligym_amd.hip).  The functions, the noise's
// counters and the orders of summation are stated in include/heligym_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppo_grad.h"

namespace hgk {

constexpr int kEsImageFloats = 7552;          // hgp::kPolicyFloats (policy_mlp.h; asserted in es.hip)
constexpr int kEsPerturbed = kPpoLogStd;      // the actor-mean parameters: theta[0 .. 5572)
constexpr int kEsQuads = kEsPerturbed / 4;    // one Philox call per quad of parameters
static_assert(kEsPerturbed % 4 == 0, "the perturbed block is whole quads");
constexpr int kEsMaxPop = 16384;              // hg_es_grad's population cap (the ranks are P^2 comparisons)
constexpr int kEsPairChunk = 16;              // pairs per fma chain of the gradient's partial sums
constexpr int kEsBlock = 256;                 // pack / perturb / rank / partial / fitness blocks
constexpr int kEsRankTile = 4 * kEsBlock;      // fitness keys staged in LDS per pass of the rank kernel
constexpr int kEsReduceThreads = 1024;        // the norm and the statistics: one block
// key words of the parameter noise: the turbulence key (seed lo, seed hi) with these constants XORed in
constexpr uint32_t kEsKey0 = 0x65735F6Eu, kEsKey1 = 0x6F697365u;

// hg_es_grad's workspace: the utilities u [P rounded up to 4] fp32, then one partial gradient [5572] fp32
// per chunk of kEsPairChunk pairs
constexpr int64_t es_u_floats(int64_t P) { return (P + 3) & ~(int64_t)3; }
constexpr int64_t es_chunks(int64_t P) { return (P / 2 + kEsPairChunk - 1) / kEsPairChunk; }
constexpr int64_t es_workspace_bytes(int64_t P) { return 4 * (es_u_floats(P) + es_chunks(P) * kEsPerturbed); }

struct EsNoiseKey {
    uint32_t k0, k1;          // the seed's words with kEsKey0 / kEsKey1 XORed in
    int64_t gen;
    const int32_t* gen_dev;   // or nullptr
};

// P images [P, 7552] from P flat parameter vectors [P, 5641], one launch.
hipError_t launch_pop_pack(const float* theta, int64_t P, int stochastic, const float* mean, const float* scale,
                           float* images, hipStream_t stream);
// P images (and, if member_theta is not null, the P parameter vectors) of theta +- sigma eps_j, one launch.
hipError_t launch_es_perturb(const float* theta, int64_t P, float sigma, const EsNoiseKey& key, int stochastic,
                             const float* mean, const float* scale, float* images, float* member_theta,
                             hipStream_t stream);
// eps_pair [5572]
hipError_t launch_es_noise(const EsNoiseKey& key, uint32_t pair, float* out, hipStream_t stream);

struct PopFitnessArgs {
    const float* reward;
    const uint8_t* terminated;
    const uint8_t* truncated;
    int64_t N, epm;
    int32_t K, first_episode, restart;
    uint8_t* alive;   // or nullptr (window mode)
    double* sum;
    float* fitness;
};
hipError_t launch_pop_fitness(const PopFitnessArgs& a, int64_t P, hipStream_t stream);

struct EsGradArgs {
    const float* fitness;
    int32_t P;
    float scale;   // -1 / (P sigma)
    EsNoiseKey key;
    float* grad;
    float* stats;   // or nullptr
    float* ws;
};
// ranks -> partial sums per pair chunk -> their fixed-order sum -> (with stats) the norm and the statistics:
// three launches, four with stats
hipError_t launch_es_grad(const EsGradArgs& a, hipStream_t stream);

}  // namespace hgk
