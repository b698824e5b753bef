// ppo_grad.h — launcher of the fused PPO loss-gradient kernel (ppo_grad.hip), called by hg_ppo_grad
// (heligym_amd.hip).  The function and the parameter layout are stated in include/heligym_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hgk {

// flat parameter layout (HG_PPO_N_PARAMS floats, each tensor row-major as torch.nn.Linear stores it)
constexpr int kPpoW1 = 0, kPpoB1 = 1088, kPpoW2 = 1152, kPpoB2 = 5248, kPpoW3 = 5312, kPpoB3 = 5568, kPpoLogStd = 5572,
              kPpoWv = 5576, kPpoBv = 5640, kPpoParams = 5641;
// one partial per block: the 5641 gradient sums, padded to a multiple of 4, then 8 statistic sums
constexpr int kPpoStatsOff = 5648, kPpoPartialFloats = 5656;
constexpr int kPpoMaxBlocks = 256;   // one block of four waves per CU of an MI355X
constexpr int64_t kPpoWorkspaceBytes = (int64_t)kPpoMaxBlocks * kPpoPartialFloats * 4;

struct PpoGradArgs {
    const float* theta;
    const float* mean;    // or nullptr
    const float* scale;   // or nullptr
    const float* obs;
    const float* act;
    const float* logp_old;
    const float* adv;
    const float* ret;
    const int32_t* index;   // or nullptr
    int64_t B, M;
    float clip, vf_coef, ent_coef, inv_m;
    float* grad;
    float* stats;   // or nullptr
    float* ws;
};

// The gradient kernel, then the fixed-order reduction of its per-block partials, both on `stream`.
hipError_t launch_ppo_grad(const PpoGradArgs& a, hipStream_t stream);

// The same kernel body with the weighted imitation loss's head (hg_bc_grad), then the same reduction.
// `a` as above with adv = the weights or nullptr (1), ret = the value targets or nullptr (no value term;
// vf_coef is 0 then), logp_old and clip unused; mode HG_BC_NLL or HG_BC_MSE.
hipError_t launch_bc_grad(const PpoGradArgs& a, int mode, hipStream_t stream);

}  // namespace hgk
