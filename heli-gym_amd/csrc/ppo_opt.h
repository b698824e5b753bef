// ppo_opt.h — launcher of the device optimiser step of the PPO update (ppo_opt.hip), called by hg_ppo_adam
// and hg_ppo_update (heligym_amd.hip).  The function and the state layout are stated in
// include/heligym_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppo_grad.h"

namespace hgk {

// optimiser state, in 4-byte words: m [5641] | pad | v [5641] | pad | a tail of 16 words
constexpr int kOptM = 0, kOptV = 5648, kOptTail = 11296, kOptWords = kOptTail + 16;
constexpr int64_t kPpoOptStateBytes = (int64_t)kOptWords * 4;
// the tail's words
constexpr int kOptApplied = 0, kOptSeen = 1, kOptStop = 2, kOptSkippedNonfinite = 3, kOptSkippedStopped = 4,
              kOptNorm = 5, kOptClipCoef = 6;
static_assert(kOptV >= kPpoParams && kOptTail >= kOptV + kPpoParams && kPpoOptStateBytes % 16 == 0, "state layout");

struct PpoAdamArgs {
    float* theta;
    const float* grad;
    const float* stats;    // the minibatch's statistics row (hg_ppo_grad's), or nullptr
    uint32_t* state;
    const float* lr_dev;   // or nullptr: lr
    double lr, beta1, beta2;
    float b1, b2, omb1, omb2, eps;   // the betas, 1 - beta (each rounded once from double), epsilon
    float max_norm;        // <= 0: no clipping
    float target_kl;       // <= 0: no early stop
};

// One optimiser step on `stream` (one block).
hipError_t launch_ppo_adam(const PpoAdamArgs& a, hipStream_t stream);
// The state's kOptWords words zeroed by a kernel on `stream`.
hipError_t launch_ppo_opt_zero(uint32_t* state, hipStream_t stream);

}  // namespace hgk
