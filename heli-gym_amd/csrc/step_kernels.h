// step_kernels.h — the step's device code: the noise (Philox4x32-10), the kernel arguments, `step_body` and
// the two kernels every build of it has, `step_kernel` and the small-batch `step_help_kernel`.
//
// Included by heligym_amd.hip, whose rollout, branch and re-trim kernels wrap `step_body` too, and by
// step_rtc.hip, which compiles the same code with another airframe's constants and nothing else of the
// library.  Everything is in the including translation unit's anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/heligym_amd.h"
#include "physics.h"
#include "retrim.h"
#include "baked.h"
#include "weather.h"
#include "goals.h"

using hg::Params;
using hg::Template;
using hgk::kTileEnvs;
using hgk::kTileWords;
using hgk::kFusedLine;
using hgk::kFusedSlot;
using hgk::kFusedWaveCtrs;

namespace {

#ifndef HG_STEP_BLOCK
#define HG_STEP_BLOCK 64
#endif
constexpr int kStepBlock = HG_STEP_BLOCK;   // step kernel block: one or more waves, one state tile each
static_assert(kTileEnvs == 64, "a state tile is one wave");

// ------------------------------------------------------------------------------ Philox4x32-10
struct U4 {
    uint32_t x, y, z, w;
};

#ifndef HG_PHILOX_ROUNDS   // (A/B builds only: the library's noise stream is Philox4x32-10)
#define HG_PHILOX_ROUNDS 10
#endif
__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < HG_PHILOX_ROUNDS; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
#ifndef HG_NO_BITOP3
        // hi ^ y ^ k as one three-input bitwise instruction (truth table 0x96 = XOR3)
        c = U4{(uint32_t)__builtin_amdgcn_bitop3_b32(hi1, c.y, k0, 0x96), lo1,
               (uint32_t)__builtin_amdgcn_bitop3_b32(hi0, c.w, k1, 0x96), lo0};
#else
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
#endif
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// ((x >> 8) + 0.5) 2^-24 in fp32: from 2^23 on the + 0.5 rounds to even, so u is in (0, 1] (1 at the top:
// a zero Box-Muller radius, never a log of 0); tests/philox_ref.py restates it bitwise
__device__ __forceinline__ float u01(uint32_t x) {
    return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f);
}

// ------------------------------------------------------------------------------ kernels

// Kernel arguments.  What the state loads wait for -- the state base, n (a lane is active), the noise
// key -- are the step kernel's first scalar parameters, preloaded into SGPRs at wave launch
// (-amdgpu-kernarg-preload-count), so no scalar-load round trip sits in front of the state loads;
// StepArgs follows, its feature-only fields last.  192 bytes in all, three scalar-cache lines (200
// bytes, a fourth line on the critical path, cost 0.23 us per step).
constexpr int kStepPreloadArgs = 6;   // state, n, seed, env_offset, Pa, Tp
struct StepArgs {
    const float2* hmap;
    const float* actions;
    float* obs;
    float* reward;
    uint8_t* terminated;
    uint8_t* truncated;
    uint8_t* info;
    const float* eta;
    float* final_obs_rows;       // [N,17] terminal observations of this step's auto-resets at their rows (hg_step_rows), or NULL
    int32_t nsteps;          // MULTI: steps per launch (inputs / outputs stacked [nsteps][N])
    int32_t retrim_slot;     // -1, or the slot of retrim_count's ring of three this step counts into (it
                             // zeroes the next one)
    // FEAT only
    int32_t* reset_count;
    int32_t* reset_count_next;   // zeroed by this launch for a later step (hg_step_chained), or NULL
    int32_t* reset_index;
    float* final_obs;
    float* retrim_wind;      // reset_mode RETRIM: [3][N] wind of the step (the trim wind of a reset)
    int4* retrim_recs;       // ... compacted jobs {env, trim wind} of the envs to re-trim
    int32_t* retrim_count;   // ... their number: retrim_count[max(retrim_slot, 0)]
    const float* tmpl_env;   // per-env reset templates [N][39] (Params::env_templates), else unused
    // next-step auto-resets re-trimmed concurrently with the following step (reset_mode RETRIM):
    int4* ov_recs;           // jobs {env, trim wind} of the envs whose episode ends this step, or NULL
    int32_t* ov_count;       // ... their number (zeroed by the previous step of the sequence)
    int32_t* ov_count_next;  // ... the next step's count, zeroed by this launch
    int32_t ov_active;       // the resets due this step are being trimmed by a concurrent retrim_kernel
                             // (ov mode): their state, but for the step counter, and their observation
                             // rows are that kernel's to write
    // fused same-step re-trim (step_fused_kernel): records published by device-coherent stores (env
    // last), the resets deferred as in ov mode (the trim writes all but the step counter)
    unsigned long long* fused_ctr;   // this launch's fused slot (kFusedSlot ints), or NULL (not fused)
    int32_t* fused_next;     // the next launch's slot, zeroed by this launch
};

// Model constants travel as a pointer to a device copy (scalar loads); by value they would take
// ~0.6 KB of kernel arguments and spill more SGPRs.
using ParamArg = const Params<float>* __restrict__;

#ifndef HG_NTS_WAVES   // bulk per-step launches store non-temporally up to this many waves per SIMD
#define HG_NTS_WAVES 4
#endif
#ifndef HG_NT_WAVES   // the lone-wave (NT) variant up to this many waves per SIMD
#define HG_NT_WAVES 2
#endif
#ifndef HG_MIN_WAVES
#define HG_MIN_WAVES 1
#endif
#ifndef HG_EARLY_POST   // post-step terrain texels requested right after the RK update (0: after the reward)
#define HG_EARLY_POST 1
#endif
#ifndef HG_MIN_WAVES_BULK   // launches with more waves than SIMDs (not NT): waves per SIMD the
#define HG_MIN_WAVES_BULK 3   // registers must fit (3: <= 168 VGPRs; uncapped the bulk variant took
#endif                        // 173 and ran two: 262 144 envs 21.1 -> 19.3 us, 1 M and 4 M unchanged)

constexpr int kTplFloats = (int)(sizeof(Template<float>) / sizeof(float));
static_assert(kTplFloats <= 64, "reset template must fit one float per lane");
// the template's device copy holds one float per lane of a wave (HG_TPL_FULL: every lane loads one)
constexpr size_t kTplAlloc = 64 * sizeof(float);
#ifndef HG_RT_QUEUE_LATE   // the re-trim queue's records written after the state stores (lone-wave kernels)
#define HG_RT_QUEUE_LATE 1
#endif
#ifndef HG_TPL_FULL_HELP
#define HG_TPL_FULL_HELP 1
#endif
#ifndef HG_RESET_LDS   // 1: the lone-wave kernels' same-step reset reads the template from the wave's LDS copy
#define HG_RESET_LDS 1   // under the resetting lanes' mask (0: readlane + select for every lane of the wave)
#endif
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// Output stores.  NT = non-temporal for the dword-and-wider columns (the byte flags stay plain):
// used when the whole batch is resident at once (<= one wave per SIMD), where the step is latency
// bound and streaming the outputs shortens the end-of-kernel write-back; with more waves than
// SIMDs the plain write-back path is faster.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <bool NT, typename T>
__device__ __forceinline__ void st_out(T* p, T v) {
    if constexpr (NT && sizeof(T) >= 4) __builtin_nontemporal_store(v, p);
    else *p = v;
}
template <bool NT>
__device__ __forceinline__ void st_out4(float* p, const float* s) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(s);
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
    else *reinterpret_cast<f32x4*>(p) = v;
}

typedef __attribute__((address_space(4))) const Params<float> ConstParams;
__device__ __forceinline__ const Params<float>* reload_params(const Params<float>* p) {
    ConstParams* c = (ConstParams*)p;
    asm volatile("" : "+s"(c));   // opaque: the loads cannot be hoisted out of the step loop
    return (const Params<float>*)c;
}

// Per-lane access at a small byte offset from a uniform base (SGPR-base global load / store).  The
// explicit global address space keeps the saddr form (`global_store_dword voff, v, s[base]`) even
// for bases that went through an opaque copy, which would otherwise be flat stores with a 64-bit
// VALU address add each.
#define HG_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ T ld_lane(const T* __restrict__ base, uint32_t idx) {
    const HG_GLOBAL char* g = (const HG_GLOBAL char*)base + idx * (uint32_t)sizeof(T);
    if constexpr (sizeof(T) == 16) {   // float4: load as a plain vector (no address-space copy ctor)
        typedef float v4 __attribute__((ext_vector_type(4)));
        return __builtin_bit_cast(T, *(const HG_GLOBAL v4*)g);
    } else {
        return *(const HG_GLOBAL T*)g;
    }
}
template <bool NT, typename T>
__device__ __forceinline__ void st_lane(T* base, uint32_t idx, T v) {
    HG_GLOBAL T* p = (HG_GLOBAL T*)((HG_GLOBAL char*)base + idx * (uint32_t)sizeof(T));
    if constexpr (NT && sizeof(T) >= 4) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// Observations of a step: each wave stages its 64 rows in its own LDS slice (stride 17 is
// bank-conflict free) and writes them back as contiguous float4, with no block-wide barrier.
// MULTI (hg_rollout): step s's rows start at obs + s*N*17 floats, 16-byte aligned only when
// N % 4 == 0 (or s % 4 == 0); unaligned rows go out as dwords.
// `skip` (uniform): rows another kernel writes (the concurrently re-trimmed resets), stored around.
template <bool NT, bool MULTI>
__device__ __forceinline__ void store_obs_wave(float* w_obs, const float obs[17], float* dst, int64_t so, int64_t w0,
                                               int64_t n, int lane, uint64_t skip = 0) {
#pragma unroll
    for (int c = 0; c < 17; ++c) w_obs[lane * 17 + c] = obs[c];
    __builtin_amdgcn_wave_barrier();
    const int nw = (n - w0) < 64 ? (int)(n - w0) : 64;
    const int cnt = nw > 0 ? nw * 17 : 0;
    float* out = dst + (so + w0) * 17;
    if (skip) {
        for (int j = lane; j < cnt; j += 64)
            if (!((skip >> (j / 17)) & 1)) st_out<NT>(out + j, w_obs[j]);
        return;
    }
    const bool aligned = !MULTI || (((uintptr_t)out & 15) == 0);
    if (nw == 64 && aligned) {   // full wave: 272 float4, all LDS reads issued before the first store
        f32x4 v[5];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = *reinterpret_cast<const f32x4*>(w_obs + 4 * (lane + 64 * t));
        if (lane < 16) v[4] = *reinterpret_cast<const f32x4*>(w_obs + 4 * (lane + 256));
#pragma unroll
        for (int t = 0; t < 4; ++t) st_out4<NT>(out + 4 * (lane + 64 * t), reinterpret_cast<const float*>(&v[t]));
        if (lane < 16) st_out4<NT>(out + 4 * (lane + 256), reinterpret_cast<const float*>(&v[4]));
        return;
    }
    const int n4 = aligned ? cnt >> 2 : 0;
    for (int j = lane; j < n4; j += 64) st_out4<NT>(out + 4 * j, w_obs + 4 * j);
    for (int j = (n4 << 2) + lane; j < cnt; j += 64) st_out<NT>(out + j, w_obs[j]);
}


// x in [-pi, pi) (fp32 pi rounds up, so the strict bounds are the fp32 values in [-pi, pi)); NaN: false
__device__ __forceinline__ bool in_pi_range(float x) {
    return x > -3.14159274101257324f && x < 3.14159274101257324f;
}

// RK4 combinations (dynamics.py:158-171) on pairs of state components, so that they issue as packed
// fp32 (v_pk_fma_f32: two lanes' worth of fma per instruction at the issue cost of one): each
// component is rounded exactly as the scalar `acc += 2k; st = hs + k h` / `hs += (acc + k) dt/6`.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <bool FIRST>
__device__ __forceinline__ void rk_stage(const float* hs, const float* k, float* acc, float* st, float h) {
#pragma unroll
    for (int c = 0; c < 18; c += 2) {
        const f32x2 kk = {k[c], k[c + 1]}, hh = {hs[c], hs[c + 1]};
        f32x2 aa;
        if (FIRST) {
            aa = kk;
        } else {
            const f32x2 a0 = {acc[c], acc[c + 1]};
            aa = a0 + 2.f * kk;
        }
        const f32x2 ss = hh + kk * h;
        acc[c] = aa.x; acc[c + 1] = aa.y;
        st[c] = ss.x; st[c + 1] = ss.y;
    }
}

__device__ __forceinline__ void rk_update(float* hs, const float* k, const float* acc, float dt6) {
#pragma unroll
    for (int c = 0; c < 18; c += 2) {
        const f32x2 kk = {k[c], k[c + 1]}, hh = {hs[c], hs[c + 1]}, aa = {acc[c], acc[c + 1]};
        const f32x2 r = hh + (aa + kk) * dt6;
        hs[c] = r.x; hs[c + 1] = r.y;
    }
}

// Turbulence noise of a step (wind_dynamics.py:49-52: eta = randn(3) / sqrt(dt)): injected by the
// caller (ETA), or Box-Muller normals from Philox4x32-10 keyed by (global env id, step, episode).
template <bool ETA>
__device__ __forceinline__ void draw_eta(const StepArgs& a, uint64_t seed, int64_t env_offset, const Params<float>& P,
                                         int64_t so, int64_t blk0,
                                         uint32_t lo, int32_t step, int32_t epi, float eta[3]) {
    if (ETA) {
        const float* eb = a.eta + 3 * (so + blk0);
        eta[0] = ld_lane(eb + 0, 3 * lo);
        eta[1] = ld_lane(eb + 1, 3 * lo);
        eta[2] = ld_lane(eb + 2, 3 * lo);
    } else {
        const uint64_t gid = (uint64_t)(env_offset + blk0 + lo);
        const U4 r = philox(U4{(uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)step, (uint32_t)epi},
                            (uint32_t)seed, (uint32_t)(seed >> 32));
        // Box-Muller.  Radii sqrt(-2 ln u) / sqrt(dt) = sqrt(log2(u) * (-2 ln 2 / dt)) with u in (0, 1]
        // from the top 24 bits; angles in revolutions for the hardware sin / cos (v_sin_f32 takes
        // revolutions: sin(2 pi u) = v_sin(u)), u in [1, 2) from the top 23 bits (a whole turn apart)
        const float rk = P.eta_norm * P.eta_norm * -1.38629436111989061f;   // -2 ln 2 / dt
        const float r0 = sqrtf(__log2f(u01(r.x)) * rk);
        const float r1 = sqrtf(__log2f(u01(r.z)) * rk);
        const float a1 = __uint_as_float((r.y >> 9) | 0x3f800000u), a3 = __uint_as_float((r.w >> 9) | 0x3f800000u);
        eta[0] = r0 * __builtin_amdgcn_cosf(a1);
        eta[1] = r0 * __builtin_amdgcn_sinf(a1);
        eta[2] = r1 * __builtin_amdgcn_cosf(a3);
    }
}

// Diagnostic build only: per-wave phase timestamps (s_memtime) of one launch, for latency
// attribution; lane 0 of each of the first HG_TIMING_WAVES waves records them.
#ifndef HG_TIMING
#define HG_TIMING 0
#endif

#if HG_TIMING
#define HG_TIMING_WAVES 2048
#define HG_TIMING_SLOTS 17   // 0..13 phase stamps, 14/15 realtime end/start, 16 the wave's branch flags
__device__ unsigned long long g_timing[HG_TIMING_WAVES][HG_TIMING_SLOTS];
__device__ unsigned long long g_timing_help[HG_TIMING_WAVES][5];   // the helper waves' stamps (HSTAMP, below)
#endif
#if HG_TIMING == 2
// HG_TIMING=2, the launch-tail mode: the production schedule (no phase stamps, no wait for the stores), per
// wave only the realtime stamp at entry, the one after its last store is issued, the branch flags and the
// hardware ids, for HG_TAIL_RING consecutive launches.  A launch's ring slot is g_tail_launch as the wave
// reads it at entry; wave 0 advances it as its last act (dependent launches: a launch's waves all enter
// long before its wave 0 ends; every record carries the index it read, so the reader can check that).
// The branch flags are plain stores to words of their own (g_timing slots 1..4, zeroed at entry, read back
// after the end stamp): no load's round trip inside the schedule.
#define HG_TAIL_RING 128
#define HG_TAIL_WAVES 1024
__device__ unsigned long long g_tail[HG_TAIL_RING][HG_TAIL_WAVES][4];   // start, end, flags | launch << 32, HW_ID | XCC_ID << 32
__device__ unsigned int g_tail_launch;
#define TSTAMP(j, ...) do { } while (0)
#define HSTAMP(j, ...) do { } while (0)
#define HG_STAMP_WAVE() (blockDim.x == 128 ? (int)blockIdx.x : (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6))
static_assert(HG_STEP_BLOCK != 128, "HG_TIMING builds tell the helper kernel's blocks by their 128 threads");
#define HG_STAGE_FLAG(bit)                                                                      \
    do {                                                                                        \
        const int w_ = HG_STAMP_WAVE();                                                         \
        if ((threadIdx.x & 63) == 0 && w_ < HG_TAIL_WAVES) g_timing[w_][(bit) == 1 ? 1 : ((bit) == 2 ? 2 : ((bit) == 4 ? 3 : 4))] = (bit); \
    } while (0)
#elif HG_TIMING
#define TSTAMP(j, ...)                                                                          \
    do {                                                                                        \
        asm volatile("" ::__VA_ARGS__);                                                         \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                             \
        const int w_ = (int)(i >> 6);                                                           \
        if ((tid & 63) == 0 && w_ < HG_TIMING_WAVES) g_timing[w_][j] = t_;                      \
    } while (0)
// the stamping wave's tile from the hardware ids (the small-batch kernel's blocks are a stepping wave and
// its helper: the stepping wave is wave 0, its tile the block).  A 128-thread block is taken for the
// small-batch kernel's, so the timing build keeps the one-wave step blocks of the default build.
static_assert(HG_STEP_BLOCK != 128, "HG_TIMING builds tell the helper kernel's blocks by their 128 threads");
#define HG_STAMP_WAVE() (blockDim.x == 128 ? (int)blockIdx.x : (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6))
// the same stamp from inside the RK driver (stage_f32.h), where only the hardware ids are in scope
#define HG_STAGE_STAMP(j, ...)                                                                  \
    do {                                                                                        \
        asm volatile("" ::__VA_ARGS__);                                                         \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                             \
        const int w_ = HG_STAMP_WAVE();                                                         \
        if ((threadIdx.x & 63) == 0 && w_ < HG_TIMING_WAVES) g_timing[w_][j] = t_;              \
    } while (0)
// which wave-uniform branches the wave took (HG_TIMING builds): 1 reset, 2 gear contact code,
// 4 the full sincos of a large attitude increment
#define HG_STAGE_FLAG(bit)                                                                      \
    do {                                                                                        \
        const int w_ = HG_STAMP_WAVE();                                                         \
        if ((threadIdx.x & 63) == 0 && w_ < HG_TIMING_WAVES) g_timing[w_][16] |= (bit);         \
    } while (0)
// the small-batch kernel's helper waves (one per tile): 0 start (s_memrealtime), 1 start (s_memtime),
// 2 the tile's counters arrived (noise key), 3 noise and wind step done, 4 past the hand-off barrier
#define HSTAMP(j, ...)                                                                     \
    do {                                                                                        \
        asm volatile("" ::__VA_ARGS__);                                                         \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                             \
        if (lane == 0 && tile < HG_TIMING_WAVES) g_timing_help[tile][j] = t_;                   \
    } while (0)
#else
#define TSTAMP(j, ...) do { } while (0)
#define HSTAMP(j, ...) do { } while (0)
#endif

}  // namespace
#include "stage_f32.h"   // (after the timing macros: HG_STAGE_STAMP)
#include "policy_mlp.h"  // (after philox / u01)
namespace {

// hg_rollout_policy's arguments beside StepArgs (which keeps its size: the per-step kernels' argument
// segment is three scalar-cache lines)
struct PolicyArgs {
    const float* pk = nullptr;     // the handle's packed policy (policy_mlp.h)
    const float* obs0 = nullptr;   // [N,17] the observations step 0's actions are computed from
    float* actions_out = nullptr;  // [nsteps,N,4] the sampled actions
};

// hg_rollout_ac's further outputs, [nsteps,N] each, any of them null (value and next_value together).
// A struct of its own: PolicyArgs is a kernel argument of hg_rollout_policy's kernels.
struct AcArgs {
    float* logp = nullptr;         // log pi(a_k | o_k)
    float* value = nullptr;        // V(o_k), o_k the observation a_k was computed from
    float* next_value = nullptr;   // terminated[k] ? 0 : V(o'_k), o'_k step k's observation before any reset
};

// hg_rollout_branch's arguments beside StepArgs (of which it reads hmap, actions and nsteps); the kernel's
// row count N * branches travels as its `n`.  A struct of its own, like the two above.
struct BranchArgs {
    float* ret = nullptr;              // [N*branches] discounted return of each row
    int32_t* alive_steps = nullptr;    // [N*branches] steps up to and including the row's ending step, or NULL
    uint8_t* end_info = nullptr;       // [N*branches] the ending step's HG_INFO_* bits (0: survived), or NULL
    uint32_t branches = 1;             // rows per env: row r is branch r % branches of env r / branches
    float gamma = 1.f;
};

// hg_rollout_branch_policy's arguments beside StepArgs, PolicyArgs (pk, obs0) and BranchArgs; all wave-uniform.
// A struct of its own once more: no existing kernel's argument segment moves.
struct BranchPolicyArgs {
    const float* residual = nullptr;   // [nsteps, N*branches, 4] added to the policy's mean, or NULL
    hgp::ActBox box = {};              // the applied action's bounds
    int32_t bootstrap = 0;             // HG_BOOTSTRAP_VALUE: survivors and truncated rows add disc * value_scale * V(o')
    float value_scale = 1.f;
};

// hg_set_weather's per-env records (weather.h): a kernel argument of the weather kernels alone, after every
// other one -- no existing kernel's argument segment moves.
struct WeatherArgs {
    const f32x4* rec = nullptr;    // [tiles][2][64] 16-byte words: {wm_n, wm_e, cos, sin}, {sigma_low, turb_level, 0, 0}
    const float* tep = nullptr;    // [tiles * 64][16] the env's TEP row (13 values), read above 1000 ft only
};

// hg_set_fleet's airframe classes: a kernel argument of the fleet kernels alone, after every other one -- no
// existing kernel's argument segment moves.  A state tile (one wave) has one class, so the model constants
// stay scalar loads from one uniform pointer: step_body is given `table + tile_class[tile]` where the other
// kernels give it the handle's one image, and is the same code.
struct FleetArgs {
    const Params<float>* table = nullptr;   // [n_classes] the classes' constant images
    const int32_t* tile_class = nullptr;    // [tiles] the class of each 64-env state tile
};
// The constants of env tile `tile` (wave-uniform).  One scalar load (constant address space: uniform address,
// read-only table) in front of every constant load of the wave: the fleet kernels issue it first thing, so it
// is in flight with the state groups' loads.
__device__ __forceinline__ ParamArg fleet_params(const FleetArgs& fl, uint32_t tile) {
    typedef __attribute__((address_space(4))) const int32_t ConstI32;
    const int32_t c = __builtin_amdgcn_readfirstlane(((ConstI32*)fl.tile_class)[tile]);
    return fl.table + c;
}
// the env tile of this wave of a step-family block (blocks of kStepBlock / 64 tiles)
__device__ __forceinline__ uint32_t fleet_wave_tile() {
    if constexpr (kStepBlock == 64) return blockIdx.x;
    else return blockIdx.x * (kStepBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

// hg_set_goals' per-env goals (goals.h): a kernel argument of the goal kernels alone, after every other one -- no
// existing kernel's argument segment moves.  `sample` and `relative` are wave-uniform run-time flags.
struct GoalArgs {
    f32x4* rec = nullptr;    // [tiles][2][64] 16-byte words: the normalised goal, the goal in ft and ft/s
    hgg::Box box = {};       // sample: the box a reset draws the new episode's goal from
    double n_x = 1.0, n_v = 1.0;   // the normalisers of word 0 (derive()'s, fp64)
    int32_t sample = 0;      // box mode: a reset draws the goal of episode epi + 1 and stores its record
    int32_t relative = 0;    // the observation rows minus the goal (word 1)
};
// relative observations: the goal's fp32 value off the task's columns (N_POS, E_POS, ALTITUDE; or ALTITUDE and
// LON_AIR_SPD).  The wind model's carry reads columns 4, 5, 6 and 16, which stay.
template <int TASK>
__device__ __forceinline__ void goal_shift(float obs[17], const f32x4& gf) {
    if (TASK == HG_TASK_HOVER) {
        obs[13] -= gf.x;
        obs[14] -= gf.y;
        obs[15] -= gf.z;
    } else {
        obs[15] -= gf.z;
        obs[1] -= gf.w;
    }
}

// What a variant of step_body reads beside StepArgs: a kernel points at the arguments its flags name and
// leaves the rest at the empty ones, which no code of its variant reads.
constexpr PolicyArgs kNoPolicy{};
constexpr AcArgs kNoAc{};
constexpr BranchArgs kNoBranch{};
constexpr BranchPolicyArgs kNoBranchPolicy{};
constexpr WeatherArgs kNoWeather{};
constexpr GoalArgs kNoGoal{};
struct StepExtras {
    const PolicyArgs* pol = &kNoPolicy;            // kPolicy
    const AcArgs* ac = &kNoAc;                     // kAc
    const BranchArgs* br = &kNoBranch;             // kBranch
    const BranchPolicyArgs* bp = &kNoBranchPolicy; // kBranch | kPolicy
    const WeatherArgs* wx = &kNoWeather;           // kWeather
    const GoalArgs* gl = &kNoGoal;                 // kGoal
};

// step_body's variant: the task, a mask V of the flags below and HELP, the helper kernel's tiles per block
// (0 in every other kernel).  A kernel names the flags it turns on -- kNT | kFeat | (ETA ? kEta : 0) -- and
// every flag is off unless named.  All compile-time, so the hot kernel has no data-independent branches
// to merge around; every variant computes the same bits (-ffp-contract=on), so a wrong flag shows in
// speed or in a feature's absence, not in the parity tests.  The body is a device function so that the
// run-time specialised code objects (step_rtc.hip) wrap the same code in kernels of their own names.
enum StepFlag : uint32_t {
    // noise injected by the caller, a.eta (else in-kernel Philox).  With kBranch: no noise (eta = 0).
    kEta = 1u << 0,
    // the lone-wave step: streaming output stores (see st_out), the uniform-branch wind step, resets as
    // selects; for launches of up to HG_NT_WAVES waves per SIMD
    kNT = 1u << 1,
    // the optional features (reset-info compaction, per-reset re-trim, next-step auto-reset, TimeLimit,
    // per-env reset templates) -- without it the kernel carries none of their registers
    kFeat = 1u << 2,
    // a.nsteps consecutive steps per launch (hg_rollout) with the env state kept in registers between them
    kMulti = 1u << 3,
    // the default airframe's model constants compiled in as instruction literals (baked.h), the run-time
    // fields still read from the device copy
    kBaked = 1u << 4,
    // the bulk step (no kNT) with non-temporal output stores all the same
    kNTS = 1u << 5,
    // (with kMulti: hg_rollout_policy) each step's action is the handle's MLP policy (policy_mlp.h) of the
    // observation row the previous step wrote -- the lane's `obs` registers, from pol.obs0 at the first
    // step -- and is stored to pol.actions_out; a.actions is not read
    kPolicy = 1u << 6,
    // (with kPolicy: hg_rollout_ac) the policy is evaluated by hgp::policy_eval, which also gives the
    // action's log-probability and the value head's V of the same observation, stored to ac.logp and
    // ac.value.  ac.next_value[k] is the value of the observation step k produced before any reset: where
    // step k did not reset, that is the next iteration's V, stored one step late (the last step's by one
    // more forward pass after the steps); where it reset, the terminal observation is about to be
    // overwritten and is evaluated at once, in a wave-uniform branch only waves with such a lane take
    kAc = 1u << 7,
    // (with kMulti and kFeat: hg_rollout_branch) a lane is a row of the N * branches candidates (n_p their
    // number), `branches` consecutive rows start from one env's state, which each lane loads from that
    // env's tile slot and nobody writes back.  A row is stepped as above up to its first ending step and
    // never reset; nothing is stored per step, the discounted return, the step count and the ending
    // step's info bits once at the end.
    // With kPolicy (hg_rollout_branch_policy): the row's action is the policy's mean of the row's own
    // observation -- its env's row of pol.obs0 at the first step -- plus bp.residual's row, clamped
    // (hgp::residual_action).  One hgp::policy_eval(sample = false) per iteration gives that mean and V of
    // the same observation, which is the bootstrap term of a row the previous step truncated and, in one
    // more iteration that leaves before the step, of the rows that survived the horizon.
    kBranch = 1u << 8,
    // (hg_set_weather) the wind model's weather constants -- mean wind, its direction's cos / sin,
    // sigma_low, the TEP row -- are the lane's own, from wx's per-env record, instead of the handle's
    // (Params, or kBaked's literals).  The record's two words are requested with the state groups, once
    // per launch; the TEP row inside the wind model's branch for lanes above 1000 ft.
    kWeather = 1u << 9,
    // (hg_set_goals) the task's target is the lane's own, from gl's per-env record, instead of the handle's
    // (Params::tgt_n, vel_tgt_n, dwn_tgt_n): word 0 is requested with the state groups, word 1 -- read for
    // relative observations only -- with them in the lone-wave kernels and the rollouts, after the RK in the
    // bulk step (its registers are bound to three waves per SIMD).  gl.relative: every observation row is
    // shifted by the goal of the episode it belongs to.  gl.sample: a reset draws the new episode's goal
    // (goals.h), stores its record and shifts the reset observation by it; kMulti keeps the goal in
    // registers across the steps.
    kGoal = 1u << 10,
};
template <int TASK, uint32_t V, int HELP = 0>
__device__ __forceinline__ void step_body(float* __restrict__ state_p, int64_t n_p, uint64_t seed_p, int64_t envoff_p,
                                          ParamArg Pa, const Template<float>* __restrict__ Tp, const StepArgs& a,
                                          int64_t bid, const StepExtras& x = StepExtras{}) {
    constexpr bool ETA = V & kEta, NT = V & kNT, FEAT = V & kFeat, MULTI = V & kMulti, BAKED = V & kBaked, NTS = V & kNTS,
                   POLICY = V & kPolicy, AC = V & kAc, BRANCH = V & kBranch, WEATHER = V & kWeather, GOAL = V & kGoal;
    const PolicyArgs& pol = *x.pol;
    const AcArgs& ac = *x.ac;
    const BranchArgs& br = *x.br;
    const BranchPolicyArgs& bp = *x.bp;
    const WeatherArgs& wx = *x.wx;
    const GoalArgs& gl = *x.gl;
    static_assert(HELP == 0 || (!ETA && !MULTI), "wind helper waves: in-kernel noise, one step per launch");
    static_assert(!WEATHER || (HELP == 0 && !BRANCH && FEAT), "per-env weather: the one-wave step, per-env templates");
    static_assert(!GOAL || (FEAT && HELP == 0 && !BRANCH && !WEATHER), "per-env goals: the one-wave step, the optional features");
    static_assert(!GOAL || TASK == HG_TASK_HOVER || TASK == HG_TASK_FORWARD_FLIGHT, "per-env goals: a task with a target");
    static_assert(!POLICY || (MULTI && HELP == 0), "the in-kernel policy belongs to the rollout");
    static_assert(!AC || POLICY, "log-probabilities and values are the in-kernel policy's");
    static_assert(!BRANCH || (MULTI && FEAT && HELP == 0 && !AC), "branched rollouts: the rollout's steps");
    static_assert(!(BRANCH && POLICY) || NT, "policy-guided branches: one wave per SIMD, the lone-wave step");
    // the policy's matrix products take the wave's 64 envs as their columns: a block is one wave
    static_assert(!POLICY || kStepBlock == 64, "hg_rollout_policy needs one-wave step blocks (HG_STEP_BLOCK 64)");
    __shared__ float s_obs[(HELP ? HELP * 64 : kStepBlock) * HG_N_OBS];   // one 64-row slice per wave
    __shared__ float s_wind[HELP ? HELP * 8 * 64 : 1];   // HELP: each tile's wind output and wind state
    // the lone-wave kernels (kNT, the helper kernel): the wave's copy of the reset template, one 256-byte slice
    // per wave, written at entry from the float each lane loads and read back by the resetting lanes alone
    constexpr bool kResetLds = HG_RESET_LDS && NT && !MULTI;
    __shared__ __attribute__((aligned(16))) float s_tpl[kResetLds ? (HELP ? HELP : kStepBlock / 64) * 64 : 4];
    constexpr bool kNTS = NT || NTS;   // non-temporal output stores
    const Params<float>& P0 = *Pa;   // model constants: scalar loads from a device copy
    // BAKED: the default airframe's constants as instruction literals (baked.h); only the runtime
    // fields (dt, target, limits, flags) are loaded
    Params<float> PB;
    if constexpr (BAKED) PB = hg::bake(*Pa);
    const int lane = threadIdx.x & 63;
    // HELP: blocks of HELP tiles, waves 0 .. HELP-1 step them, waves HELP .. 2 HELP-1 run their noise and
    // wind step (helper wave j + HELP for tile j) and hand it over in LDS
    const int wave_id = (kStepBlock == 64 && HELP == 0) ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wv = HELP ? wave_id % (HELP ? HELP : 1) : wave_id;   // uniform
    const int64_t tile = bid * (HELP ? HELP : kStepBlock / 64) + wv;
    const int64_t blk0 = tile * 64;   // this wave's first env
    const int tid = lane;
    const int64_t i = blk0 + tid;
    const int64_t n = n_p;
    const bool active = i < n;
    // Addressing: this wave's state tile (7 groups x 64 lanes x 16 bytes, contiguous, retrim.h) from
    // one uniform (SGPR) base at group 4, so every group is an immediate offset (-4 .. +2 KB, inside
    // the 13-bit field) of the same SGPR-base access with the lane's byte offset: no address
    // arithmetic per group.  Lanes past the end of a ragged last tile step its padding and store
    // nothing; for the caller's [N]-row buffers they read row blk0.
    const uint32_t lo = (uint32_t)(active ? tid : 0);
    const uint32_t lt = (uint32_t)tid;
    f32x4* st_b = reinterpret_cast<f32x4*>(state_p + tile * kTileWords) + 4 * kTileEnvs;
#define GRP(ptr, g) ((ptr) + ((g) - 4) * kTileEnvs)

#if HG_TIMING == 2
    // (the helper kernel's waves are not recorded: the tail mode is the one-wave step's)
    const unsigned long long tail_t0 = __builtin_amdgcn_s_memrealtime();
    const unsigned tail_launch = __builtin_amdgcn_readfirstlane(*(volatile unsigned int*)&g_tail_launch);
    if (HELP == 0 && tid == 0 && tile < HG_TAIL_WAVES) g_timing[tile][1] = g_timing[tile][2] = g_timing[tile][3] = g_timing[tile][4] = 0;
#elif HG_TIMING
    if ((tid & 63) == 0 && (i >> 6) < HG_TIMING_WAVES) {
        g_timing[i >> 6][15] = __builtin_amdgcn_s_memrealtime();
        g_timing[i >> 6][16] = 0;
    }
#endif
    if constexpr (HELP > 0) {
        const bool helper = wave_id >= HELP;
        if (tile * 64 >= n_p) {   // (a last block's missing tiles: both waves meet at the barrier)
            asm volatile("s_barrier" ::: "memory");
            return;
        }
        if (helper) {   // the tile's noise and wind step (Heli.step :195-199), the same code as below
#if HG_TIMING
            if (lane == 0 && tile < HG_TIMING_WAVES) g_timing_help[tile][0] = __builtin_amdgcn_s_memrealtime();
#endif
            HSTAMP(1, "v"(lane));
            const Params<float>& PH = BAKED ? PB : P0;
            const f32x4 g0 = ld_lane(GRP(st_b, 0), lt), g1 = ld_lane(GRP(st_b, 1), lt), g2 = ld_lane(GRP(st_b, 2), lt),
                        g3 = ld_lane(GRP(st_b, 3), lt);
            float ws[5], carry[4], eta[3], W[3];
            carry[3] = g1.z; carry[0] = g1.w; carry[1] = g2.x; carry[2] = g2.y;
            ws[0] = g2.z; ws[1] = g2.w; ws[2] = g3.x; ws[3] = g3.y; ws[4] = g3.z;
            HSTAMP(2, "v"(g0.w), "v"(g1.x));
            draw_eta<false>(a, seed_p, envoff_p, PH, 0, blk0, lo, __float_as_int(g0.w), __float_as_int(g1.x), eta);
            hg::wind_step_f32<true>(PH, ws, carry, eta, W);
            HSTAMP(3, "v"(W[0]), "v"(ws[4]));
            float* sw = s_wind + wv * 8 * 64 + lane;
            sw[0] = W[0]; sw[64] = W[1]; sw[128] = W[2];
#pragma unroll
            for (int c = 0; c < 5; ++c) sw[(3 + c) * 64] = ws[c];
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            HSTAMP(4, "v"(lane));
            return;
        }
    }
    TSTAMP(0, "v"(tid));
    // reset template (heli[18] | carry[4] | obs[17]) one float per lane, requested with the state so
    // that a reset costs no round trip at the end (and no late load is outstanding when the step
    // ends: a load issued near the stage-4 code makes the compiler wait for it there)
    // the helper kernel: every lane loads (the device copy is padded to one float per lane, kTplAlloc),
    // no divergent load (4 096 envs 5.20 -> 5.15 us; the other kernels measured slower so)
    // (BRANCH: never a reset, no template)
    const float tpl = BRANCH ? 0.f
                             : ((HELP > 0 && HG_TPL_FULL_HELP) || lane < kTplFloats ? reinterpret_cast<const float*>(Tp)[lane] : 0.f);
    if constexpr (kResetLds) s_tpl[wv * 64 + lane] = tpl;   // (private to the wave: no barrier but the wave's own order)
    // BRANCH: the env this lane's row branches from (rows past the end take row blk0's), and its state
    // groups where its tile keeps them: per-lane 16-byte loads, up to 64 lanes of one address
    uint32_t b_env = 0;
    const f32x4* b_st = nullptr;
    if constexpr (BRANCH) {
        b_env = (uint32_t)(blk0 + lo) / br.branches;   // (rows < 2^31: checked by the host)
        b_st = reinterpret_cast<const f32x4*>(state_p + (int64_t)(b_env / kTileEnvs) * kTileWords) + b_env % kTileEnvs;
    }
    // The state groups in the order they are needed (retrim.h slot table): position and step
    // counter (-> terrain texel address, noise key), the rest of the key and the carry, the wind
    // state (-> wind step), then the heli state.  hs[2], hs[3] (the rotor azimuths) are not stepped.
    float hs[18], ws[5], carry[4];
    int32_t step, succ, epi;
    {
        // (HELP: group 2 -- carry[1..2], wind state -- is the helper wave's; the carry is rewritten
        // at the end of every step and the wind state comes back from the helper)
        f32x4 g0, g1, g2, g3, g4, g5, g6;
        if constexpr (BRANCH) {
            g0 = b_st[0 * kTileEnvs]; g1 = b_st[1 * kTileEnvs]; g2 = b_st[2 * kTileEnvs]; g3 = b_st[3 * kTileEnvs];
            g4 = b_st[4 * kTileEnvs]; g5 = b_st[5 * kTileEnvs]; g6 = b_st[6 * kTileEnvs];
        } else {
            g0 = ld_lane(GRP(st_b, 0), lt); g1 = ld_lane(GRP(st_b, 1), lt);
            g2 = HELP ? f32x4{0.f, 0.f, 0.f, 0.f} : ld_lane(GRP(st_b, 2), lt);
            g3 = ld_lane(GRP(st_b, 3), lt); g4 = ld_lane(GRP(st_b, 4), lt); g5 = ld_lane(GRP(st_b, 5), lt);
            g6 = ld_lane(GRP(st_b, 6), lt);
        }
        hs[15] = g0.x; hs[16] = g0.y; hs[17] = g0.z; step = __float_as_int(g0.w);
        epi = __float_as_int(g1.x); succ = __float_as_int(g1.y); carry[3] = g1.z; carry[0] = g1.w;
        carry[1] = g2.x; carry[2] = g2.y; ws[0] = g2.z; ws[1] = g2.w;
        ws[2] = g3.x; ws[3] = g3.y; ws[4] = g3.z; hs[14] = g3.w;
        hs[0] = g4.x; hs[1] = g4.y; hs[4] = g4.z; hs[5] = g4.w;
        hs[6] = g5.x; hs[7] = g5.y; hs[8] = g5.z; hs[9] = g5.w;
        hs[10] = g6.x; hs[11] = g6.y; hs[12] = g6.z; hs[13] = g6.w;
        hs[2] = 0.f; hs[3] = 0.f;
    }
    // WEATHER: the lane's record, requested behind the state groups (the rows are padded to whole tiles)
    hg::LaneWind lw = {};
    if constexpr (WEATHER) {
        const f32x4* rec = wx.rec + tile * (2 * kTileEnvs);
        const f32x4 r0 = ld_lane(rec, lt), r1 = ld_lane(rec + kTileEnvs, lt);
        lw.wm[0] = r0.x; lw.wm[1] = r0.y; lw.wind_dir_cos = r0.z; lw.wind_dir_sin = r0.w;
        lw.sigma_low = r1.x;
        lw.tep_row = wx.tep + (blk0 + tid) * hgw::kTepFloats;
    }
    // GOAL: the lane's record, requested behind the state groups (the rows are padded to whole tiles)
    constexpr bool kGoalEarly = NT || MULTI;   // word 1 with word 0 (else after the RK, when relative)
    f32x4 gn = {0.f, 0.f, 0.f, 0.f}, gf = {0.f, 0.f, 0.f, 0.f};
    f32x4* g_rec = nullptr;
    if constexpr (GOAL) {
        g_rec = gl.rec + tile * (2 * kTileEnvs);
        gn = ld_lane(g_rec, lt);
        if constexpr (kGoalEarly) gf = ld_lane(g_rec + kTileEnvs, lt);
    }
#ifndef HG_EARLY_PAIRS   // 1: the stages' constant pairs formed while the state loads are in flight (round 5
#define HG_EARLY_PAIRS 0  // A/B: 7.062 -> 7.088 us, profiles/r05_valu_ab.txt; not adopted)
#endif
#if HG_EARLY_PAIRS
    // (data-independent: issued ahead of the first wait for the state, off the step's critical path)
    const hg::StepK Kpairs = hg::step_k<NT && HG_PIN_CONSTANTS>(BAKED ? PB : P0);
#endif
    if (FEAT && !BRANCH && bid == 0 && tid == 0) {   // counters of a later step (rings of three)
        if (a.reset_count_next) *a.reset_count_next = 0;
        if (a.retrim_slot >= 0 && a.retrim_count) a.retrim_count[a.retrim_slot == 2 ? 0 : a.retrim_slot + 1] = 0;
        if (a.ov_count_next) *a.ov_count_next = 0;
    }
    if (FEAT && !BRANCH && bid == 0 && a.fused_next && tid < kFusedWaveCtrs + 1) a.fused_next[kFusedLine * tid] = 0;
    if (FEAT && !BRANCH && bid == 0 && a.fused_next && tid < 2) a.fused_next[1 + tid] = 0;
    const int nsteps = MULTI ? a.nsteps : 1;
    // BRANCH: the row's return and discount, its steps so far, its ending step's info bits; a row is
    // alive until its first ending step.  The rows of an env waiting for its next-step reset (whose next
    // step ignores the action) are over before they start.
    float br_G = 0.f, br_disc = 1.f;
    int32_t br_T = 0;
    uint32_t br_end = 0;
    bool br_alive = BRANCH && active && !(P0.autoreset_next && step < 0);
    bool defer_st = false;   // (one step per launch) a deferred reset: the step counter alone is stored
    // the re-trim queue (below): the wave's job mask, the slot counter's old value (leader lane), this
    // lane's job and its trim wind
    unsigned long long rt_mask = 0;
    int rt_base = 0;
    bool rt_job = false, rt_next = false;
    // (the bulk variant writes them at once: the values kept live past the stores cost it registers,
    // 262 144 envs 46.6 -> 47.3 us with the late write)
    constexpr bool kRtLate = HG_RT_QUEUE_LATE && NT && !MULTI;
    unsigned long long rc_mask = 0;   // the same for the compacted reset info
    int rc_base = 0;
    bool rc_job = false;
    float fo[kRtLate ? 17 : 1];
    float rw0 = 0.f, rw1 = 0.f, rw2 = 0.f;
    auto rt_queue = [&]() {
        if (FEAT && rt_mask) {
            const int leader = __ffsll((long long)rt_mask) - 1;
            const int slot = __builtin_amdgcn_readlane(rt_base, leader) + __popcll(rt_mask & ((1ull << lane) - 1ull));
            if (rt_job && slot < n) {
                if (rt_next) {   // a next-step reset: the wind recorded at the episode's last step
                    rw0 = a.retrim_wind[i];
                    rw1 = a.retrim_wind[n + i];
                    rw2 = a.retrim_wind[2 * n + i];
                }
                if (a.fused_ctr) {
                    // fused: the wind, then env, as device-coherent (agent-scope) stores with a wait for
                    // the wind's between them -- the trim polls env and then reads the wind the same
                    // way.  No release: the trim reads nothing else this wave stored (deferred reset),
                    // so no L2 write-back is needed, and its waits for the record flush no cache.
                    int* rp = reinterpret_cast<int*>(a.retrim_recs + slot);
                    __hip_atomic_store(rp + 1, __float_as_int(rw0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(rp + 2, __float_as_int(rw1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(rp + 3, __float_as_int(rw2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(rp, (int)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    a.retrim_recs[slot] = make_int4((int32_t)i, __float_as_int(rw0), __float_as_int(rw1), __float_as_int(rw2));
                }
            }
        }
    };
    // POLICY: the weights as this lane's matrix operands, kept across the steps, and the observation
    // row the next action is computed from (lanes past the end of a ragged tile read row blk0)
    hgp::Weights pw;
    float pobs[POLICY ? 17 : 1];
    if constexpr (POLICY) {
        hgp::load_weights(pol.pk, lane, pw);
        // (BRANCH: the row's env's observation, as its state groups above)
        const float* row = pol.obs0 + (BRANCH ? (int64_t)b_env : blk0 + lo) * 17;
#pragma unroll
        for (int c = 0; c < 17; ++c) pobs[c] = row[c];
    }
    // AC: whether the previous step reset the lane (its next_value is stored already) or terminated it
    bool ac_prev_reset = false, ac_prev_term = false;
    // (AC with values: one more pass after the last step, which only evaluates the last observation)
    // (BRANCH with POLICY and a bootstrap: the same, for the survivors' V(o_H))
    const int niter = AC ? nsteps + (ac.next_value ? 1 : 0) : ((BRANCH && POLICY) ? nsteps + (bp.bootstrap ? 1 : 0) : nsteps);
    // BRANCH with POLICY: the row's last step truncated it without terminating it: its V(o') is due
    bool bp_pend = false;
    for (int sstep = 0; sstep < niter; ++sstep) {
    // MULTI: the constants are re-read (scalar cache) each step rather than kept live across the
    // loop, where ~130 of them would spill out of the SGPR file
    const Params<float>& P = BAKED ? PB : (MULTI ? *reload_params(Pa) : P0);
    const int64_t so = MULTI ? (int64_t)sstep * n : 0;   // first row of this step's inputs / outputs
    float4 act;
    if constexpr (AC) {
        const hgp::Eval ev = hgp::policy_eval(pw, pol.pk, pobs, lane, seed_p, (uint64_t)(envoff_p + blk0 + lo), step, epi,
                                              sstep < nsteps);
        // the previous step's next_value where that step did not reset: this observation's value
        if (ac.next_value && sstep > 0 && active && !ac_prev_reset)
            st_lane<kNTS>(ac.next_value + (so - n) + blk0, (uint32_t)tid, ac_prev_term ? 0.f : ev.v);
        if (sstep == nsteps) break;
        act = ev.a;
        if (active) {
            st_lane<kNTS>(reinterpret_cast<f32x4*>(pol.actions_out) + so + blk0, (uint32_t)tid,
                          f32x4{act.x, act.y, act.z, act.w});
            if (ac.logp) st_lane<kNTS>(ac.logp + so + blk0, (uint32_t)tid, ev.logp);
            if (ac.value) st_lane<kNTS>(ac.value + so + blk0, (uint32_t)tid, ev.v);
        }
    } else if constexpr (BRANCH && POLICY) {
        const hgp::Eval ev = hgp::policy_eval(pw, pol.pk, pobs, lane, seed_p, 0, 0, 0, false);
        if (bp.bootstrap) {   // (uniform) br_disc here is the discount after the previous step's multiply
            const bool boot = bp_pend || (sstep == nsteps && br_alive);
            br_G = boot ? fmaf(br_disc, bp.value_scale * ev.v, br_G) : br_G;
            bp_pend = false;
        }
        if (sstep == nsteps || !__any(br_alive)) break;   // (wave-uniform)
        float4 res = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bp.residual) res = ld_lane(reinterpret_cast<const float4*>(bp.residual) + so + blk0, lo);
        act = hgp::residual_action(ev.a, res, bp.residual != nullptr, bp.box);
    } else if constexpr (POLICY) {
        act = hgp::policy_action(pw, pol.pk, pobs, lane, seed_p, (uint64_t)(envoff_p + blk0 + lo), step, epi);
        if (active)
            st_lane<kNTS>(reinterpret_cast<f32x4*>(pol.actions_out) + so + blk0, (uint32_t)tid,
                          f32x4{act.x, act.y, act.z, act.w});
    } else {
        act = ld_lane(reinterpret_cast<const float4*>(a.actions) + so + blk0, lo);
    }
    // terrain texels under the committed position (F6): issued now, combined after the wind step
    const hg::GroundCell<float> cell_c = hg::ground_cell(P, hs[15], hs[16]);
    const hg::GroundTexels tex_c = hg::ground_fetch(a.hmap, cell_c);

    TSTAMP(1, "v"(hs[17]), "v"(act.w), "v"(epi), "v"(carry[3]), "v"(ws[4]));
    float W[3];
    hg::StepCtx ctx;
    hg::RK4Step<NT, (HELP > 0)> rk;   // NT: the launch is one wave per SIMD; HELP: stage 1 split
    if constexpr (HELP > 0) {
        // the wind-independent part of the step's shared context and of stage 1 (kinematics, gear)
        // while the helper wave runs the wind
        const hg::Ground<float> h_c = hg::ground_combine<float>(tex_c, cell_c);
        ctx = hg::step_ctx(P, act.x, act.y, act.z, act.w, 0.f, 0.f, 0.f, h_c, hs[17]);
#if HG_EARLY_PAIRS
        rk.begin(P, ctx, hs, hg::att0(hs), Kpairs);
#else
        rk.begin(P, ctx, hs, hg::att0(hs));
#endif
        TSTAMP(2, "v"(ctx.z0), "v"(hs[0]));   // (HELP: the wind-independent context and stage-1 share done)
        asm volatile("s_barrier" ::: "memory");
        TSTAMP(3, "v"(tid));                  // (HELP: past the hand-off barrier)
        const float* sw = s_wind + wv * 8 * 64 + lane;
        W[0] = sw[0]; W[1] = sw[64]; W[2] = sw[128];
#pragma unroll
        for (int c = 0; c < 5; ++c) ws[c] = sw[(3 + c) * 64];
        ctx.W0 = W[0]; ctx.W1 = W[1]; ctx.W2 = W[2];
        TSTAMP(4, "v"(W[0]), "v"(ws[4]));     // (HELP: the wind read from LDS)
    } else {
    // turbulence noise (wind_dynamics.py:49-52): injected, or Philox normals
    float eta[3];
    if constexpr (BRANCH) {
        // the env's own noise, whichever row this is (keyed by its global id and the row's counters, which
        // advance as the env's will), or none
        if constexpr (ETA) eta[0] = eta[1] = eta[2] = 0.f;
        else draw_eta<false>(a, seed_p, envoff_p, P, 0, (int64_t)b_env, 0u, step, epi, eta);
    } else {
        draw_eta<ETA>(a, seed_p, envoff_p, P, so, blk0, lo, step, epi, eta);
    }

    // ground height under the committed position (F6), wind step (Heli.step :195-199)
    TSTAMP(2, "v"(eta[2]), "v"(eta[0]));
    if constexpr (WEATHER) hg::wind_step_f32<NT>(P, lw, ws, carry, eta, W);
    else hg::wind_step_f32<NT>(P, ws, carry, eta, W);   // (the lone-wave kernels: the uniform-branch form)
    TSTAMP(3, "v"(W[2]), "v"(W[0]));
    const hg::Ground<float> h_c = hg::ground_combine<float>(tex_c, cell_c);

    TSTAMP(4, "v"(h_c.delta), "v"(h_c.hi));
    ctx = hg::step_ctx(P, act.x, act.y, act.z, act.w, W[0], W[1], W[2], h_c, hs[17]);
#if HG_EARLY_PAIRS
    rk.begin(P, ctx, hs, hg::att0(hs), Kpairs);
#else
    rk.begin(P, ctx, hs, hg::att0(hs));
#endif
    }
    // RK4 (dynamics.py:158-171); observation from the stage-4 input (F5)
    float k[18], obs[17];
    rk.finish(P, ctx, hs, k, obs);
#if HG_EARLY_POST
    // the terrain texels under the post-step position (the flags' ground height), requested now so
    // that their latency hides behind the wraps and the reward
    const hg::GroundCell<float> cell_p = hg::ground_cell(P, hs[15], hs[16]);
    const hg::GroundTexels tex_p = hg::ground_fetch(a.hmap, cell_p);
#endif
    TSTAMP(8, "v"(hs[8]), "v"(hs[11]), "v"(obs[16]));
    if constexpr (GOAL) {   // relative observations: this row in the frame of the running episode's goal
        if (gl.relative) {
            if constexpr (!kGoalEarly) gf = ld_lane(g_rec + kTileEnvs, lt);
            goal_shift<TASK>(obs, gf);
        }
    }
    if (FEAT && !BRANCH && P.reset_retrim && active && !(P.autoreset_next && step < 0)) {   // F8: a reset trims against this wind
        float* wb = a.retrim_wind + blk0;   // [3][N]: three coalesced rows
        st_lane<false>(wb, (uint32_t)tid, W[0]);
        st_lane<false>(wb + n, (uint32_t)tid, W[1]);
        st_lane<false>(wb + 2 * n, (uint32_t)tid, W[2]);
    }
    // step_after (helicopter_dynamics.py:73-77)
    // utils.py pi_bound, (x + pi) % 2pi - pi.  An angle already in [-pi, pi) is kept as is -- what
    // the reference's fp64 arithmetic returns to 1e-16, where the fp32 round trip through x + pi
    // costs up to half an ulp of pi.  The rotor azimuths wrap in nearly every wave every step; the
    // flapping and euler angles only in a wave-uniform branch taken when one of them left the range.
    // (The rotor azimuths' wrap is az_advance's.)
    {
        const int ang[5] = {4, 5, 12, 13, 14};
        // every angle in (-pi, pi) <=> the largest |angle| below fp32 pi (two v_max3 with |.| operand
        // modifiers and one compare instead of five range tests; a NaN angle drops out of the max
        // and stays NaN either way)
        const float amax = fmaxf(fmaxf(fmaxf(fabsf(hs[4]), fabsf(hs[5])), fabsf(hs[12])),
                                 fmaxf(fabsf(hs[13]), fabsf(hs[14])));
        const bool all_in = amax < 3.14159274101257324f;
        if (__any(!all_in)) {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float x = hs[ang[j]];
                hs[ang[j]] = in_pi_range(x) ? x : hg::pi_bound(x);
            }
        }
    }

    TSTAMP(9, "v"(hs[0]));
    // reward (helicopter_with_tasks.py) and flags (helicopter.py:201-205, 219-240)
    bool success_step = false;
    float rew = 0.f;
    if constexpr (GOAL) {   // the lane's own target
        const float tgt[3] = {gn.x, gn.y, gn.z};
        if (TASK == HG_TASK_HOVER) rew = hg::reward_hover(P, tgt, hs, k, &success_step);
        if (TASK == HG_TASK_FORWARD_FLIGHT) rew = hg::reward_forward(P, gn.w, gn.z, hs, k, &success_step);
    } else {
        if (TASK == HG_TASK_HOVER) rew = hg::reward_hover(P, hs, k, &success_step);
        if (TASK == HG_TASK_FORWARD_FLIGHT) rew = hg::reward_forward(P, hs, k, &success_step);
    }
#if HG_EARLY_POST
    const hg::Ground<float> h_post = hg::ground_combine<float>(tex_p, cell_p);
#else
    const hg::Ground<float> h_post = hg::ground_height(P, a.hmap, hs[15], hs[16]);
#endif
    const bool waiting = step < 0;   // ended last step, reset due now (next-step auto-reset)
    step += 1;
    const bool failed = hg::is_failed(P, hs, k, h_post);
    TSTAMP(10, "v"(rew), "v"((int)failed));
    const bool successed = succ >= P.success_steps;   // successed_time before this step's add
    const bool time_up = step >= P.time_up_steps;
    // next-step auto-reset: an env that ended last step (counter -(n + 1)) only resets this step
    const bool pending = FEAT && !BRANCH && P.autoreset_next && waiting;   // (BRANCH: such a row is not alive)
    const bool term = (failed || successed) && !pending;
    const bool trunc = (time_up || (FEAT && step >= P.max_episode_steps)) && !pending;   // + TimeLimit
    const bool done = term || trunc;
    succ += success_step ? 1 : 0;

    if constexpr (BRANCH) {
        // the row's accumulation, masked by select: a row past its end keeps stepping beside its live
        // neighbours (physics.h clamps the terrain indices of a non-finite position) and adds nothing
        br_G = br_alive ? fmaf(br_disc, rew, br_G) : br_G;
        br_disc = br_disc * br.gamma;
        br_T += br_alive ? 1 : 0;
        br_end = (br_alive && done) ? (uint32_t)((failed ? HG_INFO_FAILED : 0) | (successed ? HG_INFO_SUCCESSED : 0) |
                                                 (time_up ? HG_INFO_TIME_UP : 0) | (success_step ? HG_INFO_SUCCESS_STEP : 0))
                                    : br_end;
        if constexpr (POLICY) bp_pend = bp.bootstrap && br_alive && trunc && !term;
        br_alive = br_alive && !done;
        // (wave-uniform; POLICY: a lane's pending bootstrap takes the next iteration's forward pass)
        if (!__any(POLICY ? (br_alive || bp_pend) : br_alive)) break;
        if constexpr (POLICY) {
#pragma unroll
            for (int c = 0; c < 17; ++c) pobs[c] = obs[c];
        }
        carry[0] = obs[4];
        carry[1] = obs[5];
        carry[2] = obs[6];
        carry[3] = obs[16];
        continue;   // no outputs per step, no reset
    }

    // auto-reset (same step, or the step after the end)
    const bool do_reset = P.autoreset && active && ((FEAT && P.autoreset_next) ? pending : done);
    // a reset whose trim runs concurrently with this step -- a next-step reset in ov mode, any reset in
    // a fused launch: only the step counter is stored here, the trim writes the rest
#ifndef HG_FUSED_NOTRIM   // diagnostic: 1, a fused launch's trim blocks leave at once and its resets
#define HG_FUSED_NOTRIM 0   // take the template (the step's own cost in that launch)
#endif
    const bool defer = FEAT && (a.ov_active || (a.fused_ctr && !HG_FUSED_NOTRIM)) && do_reset;
    defer_st = defer;
    if (active) {
        st_lane<kNTS>(a.reward + so + blk0, (uint32_t)tid, pending ? 0.f : rew);
        st_lane<kNTS>(a.terminated + so + blk0, (uint32_t)tid, (uint8_t)term);
        st_lane<kNTS>(a.truncated + so + blk0, (uint32_t)tid, (uint8_t)trunc);
        if (a.info)
            st_lane<kNTS>(a.info + so + blk0, (uint32_t)tid, pending ? (uint8_t)0 : (uint8_t)((failed ? HG_INFO_FAILED : 0) | (successed ? HG_INFO_SUCCESSED : 0) |
                                  (time_up ? HG_INFO_TIME_UP : 0) | (success_step ? HG_INFO_SUCCESS_STEP : 0) |
                                  (do_reset ? HG_INFO_RESET : 0)));
    }
    // uncompacted reset info (hg_step_rows): the terminal observation at the env's own row, in a
    // wave-uniform branch taken only by waves with a reset
    if (!MULTI && a.final_obs_rows && __ballot(do_reset)) {
        if (do_reset) {   // the 68-byte row as four 16-byte stores and one dword (dword-aligned rows)
            typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
            f4u* row = reinterpret_cast<f4u*>(a.final_obs_rows + i * 17);
#pragma unroll
            for (int q = 0; q < 4; ++q) row[q] = f4u{obs[4 * q], obs[4 * q + 1], obs[4 * q + 2], obs[4 * q + 3]};
            a.final_obs_rows[i * 17 + 16] = obs[16];
        }
    }

    if constexpr (AC) {
        // next_value of a lane this step resets: V of its terminal observation (`obs`, before the reset
        // below overwrites it), 0 where it terminated.  The forward pass runs only in waves with a lane
        // that was truncated and reset, and then in all 64 lanes: the matrix instructions take every
        // column, and a column's result depends on that column alone.
        if (ac.next_value) {
            if (__any(do_reset)) {
                float vt = 0.f;
                if (__any(do_reset && !term))
                    vt = hgp::policy_eval(pw, pol.pk, obs, lane, seed_p, 0, 0, 0, false).v;
                if (do_reset) st_lane<kNTS>(ac.next_value + so + blk0, (uint32_t)tid, term ? 0.f : vt);
            }
            ac_prev_reset = do_reset;
            ac_prev_term = term;
        }
    }

    // compacted reset info with a wave-ballot compaction (HG_RT_QUEUE_LATE: as the re-trim queue
    // below, the slots used after the state stores, the terminal observations kept until then)
    if (FEAT && P.autoreset && a.reset_count) {
        if constexpr (kRtLate) asm volatile("" ::"v"(tpl));
        const unsigned long long mask = __ballot(do_reset);
        if constexpr (kRtLate) {
            rc_mask = mask;
            if (mask) {
                const int leader = __ffsll((long long)mask) - 1;
                if (lane == leader) rc_base = atomicAdd(a.reset_count, __popcll(mask));
            }
#pragma unroll
            for (int c = 0; c < 17; ++c) fo[c] = obs[c];
            rc_job = do_reset;
        } else if (mask) {
            const int leader = __ffsll((long long)mask) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(a.reset_count, __popcll(mask));
            base = __shfl(base, leader);
            if (do_reset) {
                const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
                if (a.reset_index && slot < n) a.reset_index[slot] = (int32_t)i;
                if (a.final_obs && slot < n) {
#pragma unroll
                    for (int c = 0; c < 17; ++c) a.final_obs[(int64_t)slot * 17 + c] = obs[c];
                }
            }
        }
    }
    if (FEAT && a.ov_recs) {   // ov mode: the episodes ending now, trimmed while the next step runs
        const bool ends = active && done && P.autoreset;
        const unsigned long long mask = __ballot(ends);
        if (mask) {
            const int leader = __ffsll((long long)mask) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(a.ov_count, __popcll(mask));
            base = __shfl(base, leader);
            const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
            if (ends && slot < n)
                a.ov_recs[slot] = make_int4((int32_t)i, __float_as_int(W[0]), __float_as_int(W[1]), __float_as_int(W[2]));
        }
    }
    // queue the resets for retrim_kernel (which overwrites the template).  HG_RT_QUEUE_LATE: the slot
    // counter's atomic is issued here and its value used after the state stores (lone-wave
    // kernels, one step per launch: 65 536 envs same-step re-trim 30.43 -> 30.11 us), so that the round trip of the device-scope atomic overlaps them instead of lengthening
    // the wave (the library is built without the atomic optimizer, which would read the value here)
    if (FEAT && P.reset_retrim) {
        // the reset template's load (issued at the start) waited for here, not after the atomic
        if constexpr (kRtLate) asm volatile("" ::"v"(tpl));
        rt_job = do_reset && !a.ov_active;
        rt_mask = __ballot(rt_job);
        if (a.fused_ctr) {
            // fused: every wave counts itself, so that the trim waves know the queue is complete once
            // the count reaches the wave count.  A wave with jobs reserves them and counts itself in
            // one atomic (its jobs in the low word, itself in the high word); a wave without, in one of
            // kFusedWaveCtrs counters on lines of their own, without waiting for the old value: every
            // wave on one address serialised the atomics (65 536 envs: the step waves ended 10 to 45 us
            // into the launch, scripts/fused_probe.py)
            if (rt_mask) {
                const int leader = __ffsll((long long)rt_mask) - 1;
                if (lane == leader)
                    rt_base = (int)(uint32_t)atomicAdd(a.fused_ctr, (1ull << 32) | (unsigned long long)__popcll(rt_mask));
            } else if (lane == 0) {
                int32_t* wc = reinterpret_cast<int32_t*>(a.fused_ctr) + kFusedLine * (1 + (int)(bid % kFusedWaveCtrs));
                __hip_atomic_fetch_add(wc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else if (rt_mask) {
            const int leader = __ffsll((long long)rt_mask) - 1;
            if (lane == leader) rt_base = atomicAdd(a.retrim_count + (a.retrim_slot > 0 ? a.retrim_slot : 0), __popcll(rt_mask));
        }
        rt_next = P.autoreset_next;
        rw0 = W[0];   // the job's trim wind (same-step reset; a next-step reset reads its own, below)
        rw1 = W[1];
        rw2 = W[2];
    }
    if (!kRtLate) rt_queue();
    if (FEAT && P.env_templates) {   // this env's own reset target (its own trim condition)
        if (do_reset) {
            const float* tr = a.tmpl_env + (int64_t)i * kTplFloats;
#pragma unroll
            for (int c = 0; c < 18; ++c) hs[c] = tr[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) carry[c] = tr[18 + c];
#pragma unroll
            for (int c = 0; c < 17; ++c) obs[c] = tr[22 + c];
            // the loads complete inside this branch (vmcnt(0)): the memory-counter waits after the join
            // then need not count the re-trim queue's atomic on the other path
            if constexpr (kRtLate) __builtin_amdgcn_s_waitcnt(0xF70);
        }
    } else if (__ballot(do_reset)) {
#if HG_TIMING
        HG_STAGE_FLAG(1);
#endif
        // Template<float> = heli[18] | carry[4] | obs[17], float c held by lane c.
        if constexpr (kResetLds) {
            // the resetting lanes read the wave's LDS copy, ten 16-byte reads of wave-uniform addresses under
            // their own mask: no lane reads another lane's register, nothing runs for the other lanes
            __builtin_amdgcn_wave_barrier();
            if (do_reset) {
                const f32x4* tq = reinterpret_cast<const f32x4*>(s_tpl + wv * 64);
                float t[40];
#pragma unroll
                for (int q = 0; q < 10; ++q) {
                    const f32x4 v = tq[q];
                    t[4 * q] = v.x; t[4 * q + 1] = v.y; t[4 * q + 2] = v.z; t[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int c = 0; c < 18; ++c) hs[c] = t[c];
#pragma unroll
                for (int c = 0; c < 4; ++c) carry[c] = t[18 + c];
#pragma unroll
                for (int c = 0; c < 17; ++c) obs[c] = t[22 + c];
            }
        } else {
        // The readlanes run in this wave-uniform branch (every lane has loaded its template float), the
        // selects per lane.
#pragma unroll
        for (int c = 0; c < 18; ++c) {
            const float v = lane_value(tpl, c);
            hs[c] = do_reset ? v : hs[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = lane_value(tpl, 18 + c);
            carry[c] = do_reset ? v : carry[c];
        }
#pragma unroll
        for (int c = 0; c < 17; ++c) {
            const float v = lane_value(tpl, 22 + c);
            obs[c] = do_reset ? v : obs[c];
        }
        }
    }
    if constexpr (GOAL) {
        // the new episode's goal, in a wave-uniform branch only waves with a reset take: box mode draws it for
        // episode epi + 1 (the fp64 divides of its record are here and nowhere else) and stores both words;
        // the reset observation (the template's, absolute) goes into the new goal's frame
        if ((gl.sample || gl.relative) && __ballot(do_reset)) {
            if (do_reset) {
                if (gl.sample) {
                    float r[hgg::kRecFloats];
                    hgg::goal_draw_record(seed_p, (uint64_t)(envoff_p + blk0 + lo), epi + 1, gl.box, gl.n_x, gl.n_v, r);
                    gn = f32x4{r[0], r[1], r[2], r[3]};
                    gf = f32x4{r[4], r[5], r[6], r[7]};
                    st_lane<false>(g_rec, lt, gn);
                    st_lane<false>(g_rec + kTileEnvs, lt, gf);
                }
                if (gl.relative) goal_shift<TASK>(obs, gf);
            }
        }
    }
    if constexpr (NT) {
        // the lone-wave kernels: the same assignments as selects, no divergent branch (65 536 envs
        // -0.08 us; the bulk variant keeps the branch)
#pragma unroll
        for (int c = 0; c < 5; ++c) ws[c] = do_reset ? 0.f : ws[c];
        carry[0] = do_reset ? carry[0] : obs[4];
        carry[1] = do_reset ? carry[1] : obs[5];
        carry[2] = do_reset ? carry[2] : obs[6];
        carry[3] = do_reset ? carry[3] : obs[16];
        step = do_reset ? 0 : ((FEAT && P.autoreset_next && done) ? -step - 1 : step);
        succ = do_reset ? 0 : succ;
        epi = do_reset ? epi + 1 : epi;
    } else if (do_reset) {
#pragma unroll
        for (int c = 0; c < 5; ++c) ws[c] = 0.f;
        step = 0;
        succ = 0;
        epi += 1;
    } else {
        carry[0] = obs[4];
        carry[1] = obs[5];
        carry[2] = obs[6];
        carry[3] = obs[16];
        if (FEAT && P.autoreset_next && done) step = -step - 1;   // reset on the next step (n = step kept)
    }
    uint64_t skip_rows = 0;
    if (FEAT && !MULTI) skip_rows = __ballot(defer);
    store_obs_wave<kNTS, MULTI>(s_obs + wv * 64 * HG_N_OBS, obs, a.obs, so, blk0, n, lane, skip_rows);
    if constexpr (POLICY) {
#pragma unroll
        for (int c = 0; c < 17; ++c) pobs[c] = obs[c];
    }
    }   // steps
    if constexpr (BRANCH) {   // the row's three results; the env's state stays as it was read
        if (active) {
            st_lane<kNTS>(br.ret + blk0, (uint32_t)tid, br_G);
            if (br.alive_steps) st_lane<kNTS>(br.alive_steps + blk0, (uint32_t)tid, br_T);
            if (br.end_info) st_lane<kNTS>(br.end_info + blk0, (uint32_t)tid, (uint8_t)br_end);
        }
        return;
    }
    TSTAMP(13, "v"(hs[0]), "v"(carry[3]));
    st_b = reinterpret_cast<f32x4*>(state_p + tile * kTileWords) + 4 * kTileEnvs;
    asm volatile("" : "+s"(st_b));
    if (FEAT && !MULTI && __ballot(defer_st)) {   // a deferred reset: its step counter only (the trim writes the rest)
        if (defer_st) reinterpret_cast<int32_t*>(GRP(st_b, 0) + tid)[3] = 0;
    }
    if (active && !(FEAT && !MULTI && defer_st)) {
        // the lane index re-materialised in this block, so that each store selects the SGPR-base
        // form (a 32-bit lane offset) instead of a 64-bit VALU address add per store
        uint32_t t = (uint32_t)tid;
        asm volatile("" : "+v"(t));
        st_lane<kNTS>(GRP(st_b, 0), t, f32x4{hs[15], hs[16], hs[17], __int_as_float(step)});
        st_lane<kNTS>(GRP(st_b, 1), t, f32x4{__int_as_float(epi), __int_as_float(succ), carry[3], carry[0]});
        st_lane<kNTS>(GRP(st_b, 2), t, f32x4{carry[1], carry[2], ws[0], ws[1]});
        st_lane<kNTS>(GRP(st_b, 3), t, f32x4{ws[2], ws[3], ws[4], hs[14]});
        st_lane<kNTS>(GRP(st_b, 4), t, f32x4{hs[0], hs[1], hs[4], hs[5]});
        st_lane<kNTS>(GRP(st_b, 5), t, f32x4{hs[6], hs[7], hs[8], hs[9]});
        st_lane<kNTS>(GRP(st_b, 6), t, f32x4{hs[10], hs[11], hs[12], hs[13]});
    }
#undef GRP
    if (kRtLate) rt_queue();
    if constexpr (kRtLate) {
        if (FEAT && rc_mask) {
            const int leader = __ffsll((long long)rc_mask) - 1;
            const int slot = __builtin_amdgcn_readlane(rc_base, leader) + __popcll(rc_mask & ((1ull << lane) - 1ull));
            if (rc_job && slot < n) {
                if (a.reset_index) a.reset_index[slot] = (int32_t)i;
                if (a.final_obs) {
#pragma unroll
                    for (int c = 0; c < 17; ++c) a.final_obs[(int64_t)slot * 17 + c] = fo[c];
                }
            }
        }
    }

    TSTAMP(11, "v"(tid));
#if HG_TIMING == 2
    if constexpr (HELP == 0 && !MULTI) {
        // the end stamp once the last store is issued (not drained); then the record, off the measured life
        asm volatile("" ::: "memory");
        const unsigned long long tail_t1 = __builtin_amdgcn_s_memrealtime();
        // HW_ID (register 4: CU_ID bits 11:8, SH_ID 12, SE_ID 15:13) and XCC_ID (register 20, bits 3:0), all 32 bits
        const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));
        if (tid == 0 && tile < HG_TAIL_WAVES) {
            volatile unsigned long long* fl = &g_timing[tile][0];
            const unsigned long long flags = fl[1] | fl[2] | fl[3] | fl[4];
            unsigned long long* rec = g_tail[tail_launch % HG_TAIL_RING][tile];
            rec[0] = tail_t0;
            rec[1] = tail_t1;
            rec[2] = flags | ((unsigned long long)tail_launch << 32);
            rec[3] = hw | ((unsigned long long)xcc << 32);
            if (tile == 0) g_tail_launch = tail_launch + 1;
        }
    }
#elif HG_TIMING
    __builtin_amdgcn_s_waitcnt(0);
    TSTAMP(12, "v"(tid));
    if ((tid & 63) == 0 && (i >> 6) < HG_TIMING_WAVES) g_timing[i >> 6][14] = __builtin_amdgcn_s_memrealtime();
#endif
}

template <int TASK, bool ETA, bool NT, bool FEAT, bool MULTI, bool BAKED, bool NTS>
__global__ __launch_bounds__(kStepBlock, NT ? HG_MIN_WAVES : HG_MIN_WAVES_BULK) void step_kernel(float* __restrict__ state_p, int64_t n_p, uint64_t seed_p,
                                                      int64_t envoff_p, ParamArg Pa,
                                                      const Template<float>* __restrict__ Tp, const StepArgs a) {
    step_body<TASK, (ETA ? kEta : 0) | (NT ? kNT : 0) | (FEAT ? kFeat : 0) | (MULTI ? kMulti : 0) | (BAKED ? kBaked : 0) |
                        (NTS ? kNTS : 0)>(state_p, n_p, seed_p, envoff_p, Pa, Tp, a, blockIdx.x);
}

// Small batches (up to half a wave per SIMD): each block is a tile's wave and a helper wave that runs
// the tile's noise and wind step (no input from the helicopter state) while the tile's wave loads
// its state and forms the rest of the step's context (density, controls, terrain, attitude
// sin/cos), the wind handed over in LDS at one barrier.  Bitwise the one-wave kernel (tested).
// Per step, against the one-wave kernel: 4 096 envs 5.80 -> 5.63 us, 16 384 6.29 -> 6.08,
// 32 768 6.73 -> 6.63 (profiles/r04_helper_ab.txt).  Not used at a wave per SIMD, where the helpers
// share SIMDs with the stepping waves: 65 536 envs 7.39 -> 7.44 us (blocks of 2 or 4 tiles with their
// helpers: 8.81, 7.59).
#ifndef HG_HELPER   // tiles per block in the small-batch helper kernel; 0: none
#define HG_HELPER 1
#endif
#ifndef HG_HELPER_DIV   // the helper kernel up to resident_envs / HG_HELPER_DIV envs (2: two tiles per CU)
#define HG_HELPER_DIV 2
#endif
#if HG_HELPER > 0
template <int TASK, bool FEAT, bool BAKED>
__global__ __launch_bounds__(128 * HG_HELPER, 1) void step_help_kernel(float* __restrict__ state_p, int64_t n_p, uint64_t seed_p,
                                                                    int64_t envoff_p, ParamArg Pa,
                                                                    const Template<float>* __restrict__ Tp, const StepArgs a) {
    step_body<TASK, kNT | (FEAT ? kFeat : 0) | (BAKED ? kBaked : 0), HG_HELPER>(state_p, n_p, seed_p, envoff_p, Pa, Tp, a,
                                                                                 blockIdx.x);
}
#endif

}  // namespace
