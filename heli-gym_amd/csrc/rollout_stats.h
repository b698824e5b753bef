// rollout_stats.h — launchers of the running normalisation and episode statistics of a rollout
// (rollout_stats.hip), called by hg_rollout_stats and hg_rollout_stats_init (heligym_amd.hip).  The function
// and the state layout are stated in include/heligym_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hgk {

// the fp64 head, in doubles
constexpr int kStatsObsCount = 0, kStatsObsMean = 1, kStatsObsM2 = 18, kStatsRetCount = 35, kStatsRetMean = 36,
              kStatsRetM2 = 37, kStatsEpisodes = 38, kStatsEnvSteps = 39, kStatsSkippedRows = 40,
              kStatsSkippedReturns = 41, kStatsHeadDoubles = 48;
constexpr int kStatsCols = 17;
constexpr int64_t kStatsHeadBytes = (int64_t)kStatsHeadDoubles * 8;
static_assert(kStatsObsM2 == kStatsObsMean + kStatsCols && kStatsRetCount == kStatsObsM2 + kStatsCols &&
              kStatsSkippedReturns < kStatsHeadDoubles && kStatsHeadBytes % 16 == 0, "head layout");

// the workspace behind the per-env arrays: per-block partial sums, [quantity][block] doubles, and the word the
// finalising kernel leaves the reward scale in for the scaling kernel
constexpr int kStatsObsBlocksMax = 512, kStatsObsQ = 36;     // count | S1[17] | S2[17] | skipped rows
constexpr int kStatsScanBlocksMax = 256, kStatsScanQ = 16;   // (rollout_stats.hip names the sixteen)
constexpr int64_t kStatsWorkspaceBytes =
    ((int64_t)kStatsObsQ * kStatsObsBlocksMax + (int64_t)kStatsScanQ * kStatsScanBlocksMax) * 8 + 16;

// head | G [n] f32 | ep_ret [n] f32 | ep_len [n] i32 | padding to 16 bytes | workspace
constexpr int64_t stats_env_bytes(int64_t n) { return (12 * n + 15) / 16 * 16; }
constexpr int64_t stats_state_bytes(int64_t n) { return kStatsHeadBytes + stats_env_bytes(n) + kStatsWorkspaceBytes; }

struct RolloutStatsArgs {
    void* state;
    const float* obs;
    const float* reward;
    const uint8_t* terminated;
    const uint8_t* truncated;
    const uint8_t* info;   // or nullptr
    const float* obs0;     // or nullptr
    int64_t n;
    int32_t nsteps;
    float gamma;           // the configuration's gamma rounded once
    double obs_eps, ret_eps;
    float max_obs_scale, clip_reward;
    uint32_t update;
    float* obs_mean_out;   // each output or nullptr
    float* obs_scale_out;
    float* reward_scale_out;
    float* reward_out;
    float* obs_in_out;
    float* episode_out;
};

// The whole call on `stream`: the scans, the observation pass, the merge and, with reward_out, the scaling.
hipError_t launch_rollout_stats(const RolloutStatsArgs& a, hipStream_t stream);
// The state's stats_state_bytes(n) bytes zeroed by a kernel on `stream`.
hipError_t launch_rollout_stats_zero(void* state, int64_t n, hipStream_t stream);

}  // namespace hgk
