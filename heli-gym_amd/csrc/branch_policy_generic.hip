// branch_policy_generic.hip -- hg_rollout_branch_policy's kernels with the generic constants (any airframe but the
// compiled-in one) and their mixed-fleet variants, in a translation unit of their own because they are built
// differently from the rest of the step family.
//
// In the main translation unit (__launch_bounds__(64, 1), -amdgpu-mfma-vgpr-form) this body needs 374 values per
// lane against 256 architectural VGPRs, and the register allocator splits live ranges into AGPRs.  It placed the
// copies that park the row's step count and ending bits inside the wind model's divergent altitude branch, which
// lanes below 1 000 ft never run, so alive_steps and end_info came back as whatever the registers last held
// (measured on MI355X: 1 201 849 895 where the constant-specialised kernel returns 24; the returns were right).
// Keeping the two in LDS across the step, and building without -amdgpu-mfma-vgpr-form (accumulators in AGPRs,
// 393 registers), each moved the loss to another value (the returns, the ending bits).  Bound to two waves per
// SIMD the kernel has no AGPRs to split into: it keeps 256 VGPRs and spills 123 to 134 values to scratch (452 to
// 484 bytes per lane), and a scratch spill is stored where the value is defined, under the lanes that define
// it.  That costs time per step and gives the right rows: bitwise the constant-specialised kernels on every
// output, with lanes above and below 1 000 ft in one wave (tests/test_gpu_branch_policy_generic.py).
#include <type_traits>

#include "step_kernels.h"

namespace {

template <int TASK, bool NOISE_OFF>
__global__ __launch_bounds__(64, 2) void rollout_branch_policy_generic_kernel(
    float* __restrict__ state_p, int64_t rows_p, uint64_t seed_p, int64_t envoff_p, ParamArg Pa,
    const Template<float>* __restrict__ Tp, const StepArgs a, const PolicyArgs pol, const BranchArgs br,
    const BranchPolicyArgs bp) {
    StepExtras x;
    x.pol = &pol;
    x.br = &br;
    x.bp = &bp;
    step_body<TASK, kNT | kFeat | kMulti | kPolicy | kBranch | (NOISE_OFF ? kEta : 0)>(state_p, rows_p, seed_p, envoff_p, Pa, Tp,
                                                                                     a, blockIdx.x, x);
}

// a mixed fleet (hg_set_fleet): the constants of the env tile the wave's 64 rows branch from -- the host admits
// only `branches` that divide 64 or are multiples of it
template <int TASK, bool NOISE_OFF>
__global__ __launch_bounds__(64, 2) void rollout_branch_policy_fleet_kernel(
    float* __restrict__ state_p, int64_t rows_p, uint64_t seed_p, int64_t envoff_p, ParamArg Pa,
    const Template<float>* __restrict__ Tp, const StepArgs a, const PolicyArgs pol, const BranchArgs br,
    const BranchPolicyArgs bp, const FleetArgs fl) {
    const ParamArg Pc = fleet_params(fl, (blockIdx.x * 64u / br.branches) / (uint32_t)kTileEnvs);   // (rows < 2^31)
    StepExtras x;
    x.pol = &pol;
    x.br = &br;
    x.bp = &bp;
    step_body<TASK, kNT | kFeat | kMulti | kPolicy | kBranch | (NOISE_OFF ? kEta : 0)>(state_p, rows_p, seed_p, envoff_p, Pc, Tp,
                                                                                     a, blockIdx.x, x);
}

template <int TASK, bool NOISE_OFF>
void launch(bool fleet, unsigned grid, hipStream_t s, float* state, int64_t rows, uint64_t seed, int64_t envoff, ParamArg pa,
            const Template<float>* tp, const StepArgs& a, const PolicyArgs& pol, const BranchArgs& br,
            const BranchPolicyArgs& bp, const FleetArgs& fl) {
    if (fleet)
        hipLaunchKernelGGL((rollout_branch_policy_fleet_kernel<TASK, NOISE_OFF>), dim3(grid), dim3(64), 0, s, state, rows, seed,
                           envoff, pa, tp, a, pol, br, bp, fl);
    else
        hipLaunchKernelGGL((rollout_branch_policy_generic_kernel<TASK, NOISE_OFF>), dim3(grid), dim3(64), 0, s, state, rows, seed,
                           envoff, pa, tp, a, pol, br, bp);
}

}  // namespace

namespace hgk {

// The argument structs are the including translation unit's own (step_kernels.h, anonymous namespace): they
// cross as pointers to the same layouts.  fl == NULL: the handle's one image `pa`.
hipError_t launch_branch_policy_generic(int32_t task, bool noise_off, unsigned grid, hipStream_t s, float* state,
                                        int64_t rows, uint64_t seed, int64_t envoff, const void* pa, const void* tp,
                                        const void* step_args, const void* pol, const void* br, const void* bp,
                                        const void* fl) {
    const FleetArgs none{};
    const FleetArgs& f = fl ? *static_cast<const FleetArgs*>(fl) : none;
    auto go = [&](auto t, auto n) {
        launch<decltype(t)::value, decltype(n)::value>(fl != nullptr, grid, s, state, rows, seed, envoff,
                                                       static_cast<const Params<float>*>(pa),
                                                       static_cast<const Template<float>*>(tp),
                                                       *static_cast<const StepArgs*>(step_args),
                                                       *static_cast<const PolicyArgs*>(pol), *static_cast<const BranchArgs*>(br),
                                                       *static_cast<const BranchPolicyArgs*>(bp), f);
    };
    auto by_noise = [&](auto t) {
        if (noise_off) go(t, std::true_type{});
        else go(t, std::false_type{});
    };
    switch (task) {
        case HG_TASK_HOVER: by_noise(std::integral_constant<int, HG_TASK_HOVER>{}); break;
        case HG_TASK_FORWARD_FLIGHT: by_noise(std::integral_constant<int, HG_TASK_FORWARD_FLIGHT>{}); break;
        default: by_noise(std::integral_constant<int, HG_TASK_HELI>{}); break;
    }
    return hipPeekAtLastError();   // (the caller reports it, as for the library's other launches)
}

}  // namespace hgk
