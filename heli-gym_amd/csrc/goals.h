// Per-env goals (hg_set_goals): the record of one env's target as the goal kernels read it, and the draw of
// a box goal, each one function for the host and the device, so that a table handle given the drawn goals,
// hg_goal_draw and the reset branch of the step kernels form the same bits.
#ifndef HELIGYM_AMD_GOALS_H
#define HELIGYM_AMD_GOALS_H
#include <math.h>
#include <stdint.h>

#include "../../include/heligym_amd.h"

#ifndef HG_GOAL_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HG_GOAL_HD __host__ __device__ __forceinline__
#else
#define HG_GOAL_HD inline
#endif
#endif

namespace hgg {

// Per-env records.  Two 16-byte words per env, kept tile by tile like the state and the weather records (a
// wave's 64 first words, then its 64 second words), padded to whole tiles:
//   word 0 {north / n_x, east / n_x, -sea_alt / n_x, vel / n_v}   the normalised goal, derive()'s expressions
//                                                                (an fp64 divide, one rounding to fp32); the
//                                                                forward-flight dwn_tgt_n is its third entry
//   word 1 {north, east, sea_alt, vel}                            the goal in ft and ft/s, fp32: what relative
//                                                                observations subtract
constexpr int kRecFloats = 8;   // per env
constexpr int64_t kTile = 64;
inline int64_t padded_envs(int64_t n) { return (n + kTile - 1) / kTile * kTile; }
// float k of word w of env i in the tile-ordered image
inline size_t rec_index(int64_t i, int w, int k) {
    return (size_t)((i / kTile) * kTile * kRecFloats + (w * kTile + i % kTile) * 4 + k);
}

// The library's Philox4x32-10 streams, (counter) under (key); `seed` is the handle's but where noted:
//   turbulence noise   (gid_lo, gid_hi, episode step, episode)   seed                          step_kernels.h draw_eta
//   action noise       (gid_lo, gid_hi, episode step, episode)   seed ^ (0x706F6C69, 0x63795F7A)   policy_mlp.h
//   random actions     (gid_lo, gid_hi, step_lo, step_hi)        caller's seed ^ (0xA511E9B3, 0x63D83595)
//   minibatch shuffle  keyed permutation rounds                  caller's seed ^ (0x73687566, 0x666C655F)
//   ES perturbations   es.h                                      caller's seed ^ (0x65735F6E, 0x6F697365)
//   MPPI candidates    (gid_lo, gid_hi, t, branch)               caller's sample seed
//   box goals          (gid_lo, gid_hi, episode, kGoalTag)       seed ^ (kGoalKey0, kGoalKey1)     here
constexpr uint32_t kGoalKey0 = 0x676F616Cu, kGoalKey1 = 0x5F626F78u;   // "goal", "_box"
constexpr uint32_t kGoalTag = 0u;

struct Words {
    uint32_t x, y, z, w;
};

// Philox4x32-10 in plain integer arithmetic (the 32 x 32 -> 64-bit products): the same words on the host and
// on the device as step_kernels.h's philox, which names device instructions
HG_GOAL_HD Words philox(Words c, uint32_t k0, uint32_t k1) {
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = Words{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// step_kernels.h u01: ((x >> 8) + 0.5) 2^-24 in fp32, in (0, 1]
HG_GOAL_HD float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// the normalisers of the task's lengths and speeds (derive(): n_x = 2 R, n_v = sqrt(2 R g))
inline void goal_norms(const hg_airframe& a, double* n_x, double* n_v) {
    *n_x = 2 * a.mr_R;
    *n_v = sqrt(2 * a.mr_R * a.env_GRAV);
}

// One env's record from its target {north, east, sea_alt, vel}.  derive()'s expressions for tgt_n, vel_tgt_n
// and dwn_tgt_n: the division in fp64, one rounding to fp32.
HG_GOAL_HD void goal_record(const double g[4], double n_x, double n_v, float rec[kRecFloats]) {
    rec[0] = (float)(g[0] / n_x);
    rec[1] = (float)(g[1] / n_x);
    rec[2] = (float)(-g[2] / n_x);
    rec[3] = (float)(g[3] / n_v);
    rec[4] = (float)g[0];
    rec[5] = (float)g[1];
    rec[6] = (float)g[2];
    rec[7] = (float)g[3];
}

// The box, fp32: lo and hi of {north, east, sea_alt, vel}
struct Box {
    float lo[4], hi[4];
};

// The goal of global env `gid` in episode `epi`: u_k from word k of one Philox call, field k =
// fma(u_k, hi_k - lo_k, lo_k) in fp32 clamped into [lo_k, hi_k] (lo_k == hi_k gives lo_k).
HG_GOAL_HD void goal_draw(uint64_t seed, uint64_t gid, int32_t epi, const Box& b, float g[4]) {
    const Words r = philox(Words{(uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)epi, kGoalTag}, (uint32_t)seed ^ kGoalKey0,
                           (uint32_t)(seed >> 32) ^ kGoalKey1);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
    for (int k = 0; k < 4; ++k) {
        const float v = fmaf(u01(w[k]), b.hi[k] - b.lo[k], b.lo[k]);
        g[k] = fminf(fmaxf(v, b.lo[k]), b.hi[k]);
    }
}

// ... and its record: word 0 from the fp32 values by goal_record's divide
HG_GOAL_HD void goal_draw_record(uint64_t seed, uint64_t gid, int32_t epi, const Box& b, double n_x, double n_v,
                                 float rec[kRecFloats]) {
    float g[4];
    goal_draw(seed, gid, epi, b, g);
    const double gd[4] = {(double)g[0], (double)g[1], (double)g[2], (double)g[3]};
    goal_record(gd, n_x, n_v, rec);
}

inline void target_fields(const hg_target& t, double g[4]) {
    g[0] = t.north_loc;
    g[1] = t.east_loc;
    g[2] = t.sea_alt;
    g[3] = t.vel;
}

// nullptr, or what is wrong with a target of `task` (the fields the task does not use are not looked at)
inline const char* check_target(int32_t task, const hg_target& t) {
    if (task == HG_TASK_HOVER) {
        if (!isfinite(t.north_loc) || !isfinite(t.east_loc) || !isfinite(t.sea_alt)) return "a non-finite value";
    } else {
        if (!isfinite(t.sea_alt) || !isfinite(t.vel)) return "a non-finite value";
        if (!(t.vel > 0)) return "vel <= 0 (the forward-flight reward divides by the speed)";
    }
    return nullptr;
}

// nullptr, or what is wrong with the box
inline const char* check_box(int32_t task, const hg_goal_box& b) {
    const char* bad = check_target(task, b.lo);
    if (!bad) bad = check_target(task, b.hi);
    if (bad) return bad;
    if (task == HG_TASK_HOVER) {
        if (b.lo.north_loc > b.hi.north_loc || b.lo.east_loc > b.hi.east_loc || b.lo.sea_alt > b.hi.sea_alt) return "lo > hi";
    } else {
        if (b.lo.sea_alt > b.hi.sea_alt || b.lo.vel > b.hi.vel) return "lo > hi";
    }
    return nullptr;
}

// The box in fp32.  A field the task does not use takes the handle's target for both bounds, so that the
// record's unused entries are the handle's (and finite).
inline Box make_box(int32_t task, const hg_goal_box& b, const hg_target& own) {
    hg_target lo = b.lo, hi = b.hi;
    if (task == HG_TASK_HOVER) {
        lo.vel = hi.vel = own.vel;
    } else {
        lo.north_loc = hi.north_loc = own.north_loc;
        lo.east_loc = hi.east_loc = own.east_loc;
    }
    double l[4], h[4];
    target_fields(lo, l);
    target_fields(hi, h);
    Box r;
    for (int k = 0; k < 4; ++k) {
        r.lo[k] = (float)l[k];
        r.hi[k] = (float)h[k];
    }
    return r;
}

}  // namespace hgg
#endif
