/*
 * heligym_amd.h — C-ABI of the MI355X-native vectorised heli-gym step().
 *
 * The reference (ugurcanozalp/heli-gym v2) has no FFI on this path: its boundary is the
 * gymnasium `Heli` env (heligym/envs/helicopter.py:28-243) calling two Python
 * `DynamicSystem.step` objects (heligym/envs/dynamics/dynamics.py:158-171).  Each entry point
 * below replaces one piece of that surface; the reference file:line it replaces is cited on it.
 * The only native precedent in the reference is its renderer C-ABI
 * (heligym/envs/renderer/src/py_api.h:17-90, opaque handles, ctypes-bound in pyapi.py:9-32);
 * this header follows the same opaque-handle style but every call returns an error code.
 *
 * Conventions
 *  - Units are the reference's US customary units (ft, slug, lb, s, rad).
 *  - All `*_dev` pointers are device (HBM) pointers owned by the caller, e.g. PyTorch-ROCm
 *    tensors; `stream` is a hipStream_t passed as void* (NULL = default stream).  Device calls
 *    are asynchronous on `stream`, never synchronise, never allocate, and are hipGraph-capturable.
 *  - Host pointers are plain host memory.  Sizes are element counts.
 *  - Return value: HG_OK (0) or a negative HG_E_* code; hg_last_error() gives the message of the
 *    last failure on the calling thread.  A handle is not re-entrant: one stream/thread at a time.
 *  - Layouts: actions [N,4] fp32 row-major; obs [N,17] fp32 row-major in the reference order
 *    (helicopter_dynamics.py:23-25); per-env state record [N,HG_STATE_COLS] fp32 (see below).
 */
#ifndef HELIGYM_AMD_H
#define HELIGYM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_ABI_VERSION 3

#define HG_N_OBS 17        /* helicopter_dynamics.py:23-27 */
#define HG_N_ACT 4         /* helicopter_dynamics.py:28 */
#define HG_N_HELI 18       /* vi_mr vi_tr psi_mr psi_tr betas[2] uvw[3] pqr[3] euler[3] xyz[3] (:55-64) */
#define HG_N_WIND 5        /* us vs[2] ws[2] (wind_dynamics.py:39-42) */
#define HG_N_CARRY 4       /* previous obs N_VEL, E_VEL, DES_RATE, GROUND_ALTITUDE (helicopter.py:195-196) */
/* state record columns: heli[18] | wind[5] | carry[4] */
#define HG_STATE_COLS (HG_N_HELI + HG_N_WIND + HG_N_CARRY)
/* counter record columns (int32): episode step, success steps, episode index */
#define HG_COUNTER_COLS 3

enum {
    HG_OK = 0,
    HG_E_INVALID = -1,   /* bad argument / shape */
    HG_E_HIP = -2,       /* HIP runtime error (no device, launch failure, ...) */
    HG_E_TRIM = -3,      /* trim did not converge (helicopter_dynamics.py:543-544) */
    HG_E_NOMEM = -4
};

/* Tasks: helicopter.py:242-243 (Heli, reward 0), helicopter_with_tasks.py:5-52 (HeliHover),
 * helicopter_with_tasks.py:54-115 (HeliForwardFlight). */
enum { HG_TASK_HELI = 0, HG_TASK_HOVER = 1, HG_TASK_FORWARD_FLIGHT = 2 };

/* Reset state of auto-reset envs (hg_config.reset_mode).
 *   HG_RESET_TEMPLATE: the trim against the mean wind, computed once (the reference's first reset,
 *                      helicopter.py:55 + helicopter_dynamics.py:66-71), broadcast in-kernel.
 *   HG_RESET_RETRIM:   every reset re-trimmed on the device against the wind of the env's last step,
 *                      as the reference does from its second episode on (the heli model keeps the
 *                      last set_wind, helicopter.py:198 -> helicopter_dynamics.py:66-71,491-555). */
enum { HG_RESET_TEMPLATE = 0, HG_RESET_RETRIM = 1 };

/* When auto-reset envs restart (hg_config.autoreset_mode, with autoreset = 1).
 *   HG_AUTORESET_SAME_STEP: the step that ends an episode returns the reset observation; the
 *                           terminal one goes to final_obs_dev (gymnasium SAME_STEP / SB3 style).
 *   HG_AUTORESET_NEXT_STEP: the ending step returns the terminal observation; the env's next step
 *                           ignores its action and returns the reset observation with reward 0 and
 *                           both flags false (gymnasium >= 1.0 vector default).  Between the two,
 *                           the env's episode-step counter reads -1. */
enum { HG_AUTORESET_SAME_STEP = 0, HG_AUTORESET_NEXT_STEP = 1 };

/* info bit-field written per env by hg_step (helicopter.py:219-224). */
/* hg_debug_failed / hg_debug_failed_host: the clauses of Heli._is_failed (helicopter.py:226-234) that hold for a
 * row, whether or not they fail it: failed = (CONTACT and (SINK or ROLL or PITCH)) or NS or EW or CEILING.
 * HG_FAIL_FAILED: that combination as the function that reports the clauses forms it (a copy of the step
 * kernels' test, which returns `failed`; the two are equal on every row). */
enum { HG_FAIL_CONTACT = 1, HG_FAIL_SINK = 2, HG_FAIL_ROLL = 4, HG_FAIL_PITCH = 8, HG_FAIL_NS = 16, HG_FAIL_EW = 32,
       HG_FAIL_CEILING = 64, HG_FAIL_FAILED = 128 };
enum { HG_INFO_FAILED = 1, HG_INFO_SUCCESSED = 2, HG_INFO_TIME_UP = 4, HG_INFO_SUCCESS_STEP = 8,
       HG_INFO_RESET = 16 /* auto-reset at the end of this step (same-step auto-reset) */ };

/* Raw airframe + environment parameters: the fields of heligym/envs/helis/aw109.yaml:2-101. */
typedef struct hg_airframe {
    /* ENV (aw109.yaml:2-16) */
    double env_R, env_T0, env_LAPSE, env_RO_SEA, env_GRAV, env_MAX_GR_ALT, env_NS_MAX, env_EW_MAX;
    double env_WIND_DIR_deg, env_WIND_SPD;
    int32_t env_TURB_LVL, _pad0;
    /* HELI (aw109.yaml:18-37) */
    double HP_LOSS, VTRANS, FS_CG, WL_CG, WT, IX, IY, IZ, IXZ;
    double COL_OS, COL_L, COL_H, LON_L, LON_H, LAT_L, LAT_H, PED_OS, PED_L, PED_H;
    /* MR (:39-52) */
    double mr_FS, mr_WL, mr_IS, mr_E, mr_IB, mr_R, mr_A, mr_RPM, mr_CD0, mr_B, mr_C, mr_TWST, mr_K1;
    /* TR (:54-63) */
    double tr_FS, tr_WL, tr_R, tr_A, tr_C, tr_RPM, tr_CD0, tr_TWST, tr_B;
    /* FUS (:65-71) */
    double fus_FS, fus_WL, fus_XUU, fus_YVV, fus_ZWW, fus_COR;
    /* HT (:73-78) */
    double ht_FS, ht_WL, ht_ZUU, ht_ZUW, ht_ZMAX;
    /* VT (:80-85) */
    double vt_FS, vt_WL, vt_YUU, vt_YUV, vt_YMAX;
    /* WN (:87-93) */
    double wn_FS, wn_WL, wn_ZUU, wn_ZUW, wn_ZMAX, wn_B;
    /* LG (:95-101) */
    double lg_K, lg_C, lg_BL_MN, lg_FS_MN, lg_FS_N, lg_WL;
} hg_airframe;

/* Trim condition (helicopter.py:36-44, helicopter_dynamics.py:45-53, consumed by trim :491-555). */
typedef struct hg_trim_cond {
    double yaw, yaw_rate, ned_vel[3], gr_alt, xy[2], psi_mr, psi_tr;
} hg_trim_cond;

/* Task target (helicopter_with_tasks.py:9-13, 59-63): north_loc, east_loc, sea_alt, heading, vel. */
typedef struct hg_target {
    double north_loc, east_loc, sea_alt, heading, vel;
} hg_target;

typedef struct hg_config {
    hg_airframe af;
    hg_trim_cond trim;
    hg_target target;
    double dt;            /* helicopter.py:18-19 (1/FPS = 0.02); north star uses 0.01 */
    double max_time;      /* helicopter.py:33-34,89-92 (40 s) */
    int32_t task;         /* HG_TASK_* */
    int32_t autoreset;    /* 1: reset finished envs inside hg_step (same-step autoreset) */
    uint64_t seed;        /* Philox key for the turbulence noise (wind_dynamics.py:49-52) */
    int64_t env_offset;   /* global id of local env 0 (sharding: results independent of rank count) */
    int32_t reset_mode;   /* HG_RESET_* */
    int32_t autoreset_mode; /* HG_AUTORESET_* */
    int64_t max_episode_steps; /* > 0: also truncate at this many steps (gymnasium TimeLimit, the
                                  registry's max_episode_steps=5000, heligym/__init__.py:4-18); 0: off */
} hg_config;

/* Reset template produced by the trim (host values). */
typedef struct hg_trim_result {
    double state[HG_N_HELI];       /* trimmed heli state (fp32-rounded, as the reference stores it) */
    double action[HG_N_ACT];       /* trim controls */
    double obs[HG_N_OBS];          /* observation at the trim state */
    double state_dots[HG_N_HELI];  /* dynamics at the trim state */
    double residual;               /* final ||y - y*||^2 of the Newton iteration */
    int32_t iterations;
    int32_t failed;                /* reset-time _is_failed() (helicopter.py:226-234) */
} hg_trim_result;

typedef struct hg_env hg_env;

/* Library / error ----------------------------------------------------------------------------- */
int32_t hg_abi_version(void);
const char* hg_last_error(void);

/* Model constants of a config as the step kernel sees them (Params<float> of csrc/physics.h,
 * `bytes` = its size), or only the fields that csrc/baked.h compiles in (`baked_only`, the rest
 * zero).  Host only; for scripts/gen_baked_constants.py and tests. */
int32_t hg_debug_params(const hg_config* cfg, int32_t rows, int32_t cols, int32_t baked_only, void* out,
                        int64_t bytes);
/* 1 when every compiled-in model constant (csrc/baked.h) equals this config's, i.e. hg_create will
 * select the constant-specialised step kernel for it; 0 otherwise.  Host only. */
int32_t hg_config_is_baked(const hg_config* cfg, int32_t rows, int32_t cols);

/* Host memory the kernels can read and write directly (pinned, mapped, coherent): `*host` is the
 * CPU address, `*dev` the address to pass to hg_step / hg_reset as a device pointer.  For
 * single-env or small-batch loops that want results on the host without separate copies (the
 * single-env drop-in: one launch and one stream synchronisation per step).  Free with
 * hg_host_free(host). */
int32_t hg_host_alloc(int64_t bytes, void** host, void** dev);
void hg_host_free(void* host);

/* Fill `cfg` with the AW109 / HeliHover defaults (aw109.yaml, helicopter.py:18-44,
 * helicopter_with_tasks.py:5-25).  Host only. */
void hg_default_config(hg_config* cfg);

/* Trim (host, fp64).  Replaces HelicopterDynamics.trim / __trim_fcn
 * (helicopter_dynamics.py:491-576) as called from reset (:66-71).  `terrain_ft` is the
 * [rows, cols] ground-height map in ft (helicopter_dynamics.py:39-43), `wind_ned` the wind the
 * trim is solved against (helicopter.py:55: the mean wind).  Heights are fp64 like the reference's
 * png/65535*MAX_GR_ALT; the library keeps each as an fp32 {hi, lo} pair. */
int32_t hg_trim(const hg_config* cfg, const double* terrain_ft, int32_t rows, int32_t cols,
                const double wind_ned[3], hg_trim_result* out);

/* Handle lifetime: replaces Heli.__init__ (helicopter.py:47-86: yaml params, HelicopterDynamics
 * and WindDynamics construction, terrain load) for `num_envs` independent helicopters, and
 * Heli.close (helicopter.py:185-187).  Uploads the terrain, derives the model constants, trims
 * the reset template against the mean wind. */
int32_t hg_create(const hg_config* cfg, const double* terrain_ft, int32_t rows, int32_t cols,
                  int64_t num_envs, hg_env** out);
void hg_destroy(hg_env* env);
int64_t hg_num_envs(const hg_env* env);

/* Setters: Heli.set_max_time (helicopter.py:89-92), set_target (:94-96), set_trim_cond
 * (:101-103; re-trims the reset template).  Host only; affect subsequent device calls. */
int32_t hg_set_max_time(hg_env* env, double max_time);
int32_t hg_set_target(hg_env* env, const hg_target* target);
/* Allow (1, the default) or forbid (0) the constant-specialised step kernel (csrc/baked.h), which
 * hg_create selects when the config's model constants are the compiled-in default airframe's.
 * Both kernels give bitwise-identical results; this switch exists for A/B timing and the tests.
 * Returns 1 if the specialised kernel is now in use, 0 if not, or an HG_E_* code. */
int32_t hg_set_specialized(hg_env* env, int32_t enable);
int32_t hg_set_trim_cond(hg_env* env, const hg_trim_cond* trim);
int32_t hg_get_template(const hg_env* env, hg_trim_result* out);

/* Reset: replaces Heli.reset (helicopter.py:208-217) -> WindDynamics.reset (wind_dynamics.py:44-47)
 * + HelicopterDynamics.reset (helicopter_dynamics.py:66-71).  Envs with mask_dev[i] != 0 (all
 * envs if mask_dev == NULL) get the trimmed state, zero turbulence state, zero counters; their
 * observation row is written to obs_dev [N,17] (other rows untouched).  In HG_RESET_RETRIM mode
 * each masked env is trimmed against the wind of its last step (the mean wind before its first
 * step), as the reference's reset trims against the model's last set_wind. */
int32_t hg_reset(hg_env* env, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* Step: replaces Heli.step (helicopter.py:192-206) with everything it calls — WindDynamics.step
 * (dynamics.py:158-171 + wind_dynamics.py:49-125), HelicopterDynamics.step (dynamics.py:158-171
 * + helicopter_dynamics.py:73-77,400-489), the task reward (helicopter_with_tasks.py:27-52 /
 * 78-115) and _get_info (helicopter.py:219-240) — for all N envs in one kernel launch.
 *   actions_dev     [N,4]  fp32 in (no clipping, like the reference)
 *   obs_dev         [N,17] fp32 out (for auto-reset envs: the reset observation)
 *   reward_dev      [N]    fp32 out
 *   terminated_dev  [N]    u8 out   (failed or successed; helicopter.py:203)
 *   truncated_dev   [N]    u8 out   (time_up; helicopter.py:204)
 *   info_dev        [N]    u8 out or NULL (HG_INFO_* bits)
 *   eta_dev         [N,3]  fp32 in or NULL: turbulence noise already scaled by 1/sqrt(dt)
 *                          (parity / replay); NULL = in-kernel Philox4x32-10 normals keyed by
 *                          (seed, env_offset+i, episode, step)
 *   reset_count_dev [1]    i32 out or NULL: number of envs auto-reset this step (zeroed here)
 *   reset_index_dev [N]    i32 out or NULL: compacted ids of those envs (wave-ballot order)
 *   final_obs_dev   [N,17] fp32 out or NULL: their terminal observations, same compacted order */
int32_t hg_step(hg_env* env, const float* actions_dev, float* obs_dev, float* reward_dev,
                uint8_t* terminated_dev, uint8_t* truncated_dev, uint8_t* info_dev,
                const float* eta_dev, int32_t* reset_count_dev, int32_t* reset_index_dev,
                float* final_obs_dev, void* stream);

/* hg_step without the separate zeroing launch of the reset count: `reset_count_dev` must already be
 * 0 (the previous chained step zeroed it), and this launch zeroes `reset_count_next_dev` (another
 * buffer, for a later step) from inside the step kernel.  A caller rotating three count buffers
 * (step k: count[k % 3], next count[(k + 1) % 3]) keeps each step's count readable until the step
 * after next.  reset_count_dev is still zeroed by a memset launch when the handle's previous step
 * launch was not an hg_step_chained call of the same sequence -- the first call, after hg_step /
 * hg_step_rows / hg_rollout, the first call captured into a graph (so that every replay starts
 * from a zeroed count) and the first eager call after a capture.  Same results as hg_step. */
int32_t hg_step_chained(hg_env* env, const float* actions_dev, float* obs_dev, float* reward_dev,
                        uint8_t* terminated_dev, uint8_t* truncated_dev, uint8_t* info_dev,
                        const float* eta_dev, int32_t* reset_count_dev, int32_t* reset_index_dev,
                        float* final_obs_dev, int32_t* reset_count_next_dev, void* stream);

/* hg_step with the same-step reset info left uncompacted: the terminal observation of every env
 * auto-reset in this step goes to its own row of `final_obs_rows_dev` [N,17] (other rows are left
 * untouched) and its info byte carries HG_INFO_RESET, so the reset envs are the rows whose info has
 * that bit.  No count, no atomics, no zeroing launch: the step runs the same kernel as a plain
 * hg_step (the specialised one for the default airframe).  info_dev is required. */
int32_t hg_step_rows(hg_env* env, const float* actions_dev, float* obs_dev, float* reward_dev,
                     uint8_t* terminated_dev, uint8_t* truncated_dev, uint8_t* info_dev,
                     const float* eta_dev, float* final_obs_rows_dev, void* stream);

/* Open-loop rollout: `nsteps` consecutive hg_step calls in one launch, each env's state kept in
 * registers between steps (state is read and written once).  Results are identical to nsteps
 * hg_step calls with the same inputs (same auto-reset, noise keys, flags).  Inputs / outputs are
 * stacked per step: actions_dev [nsteps,N,4], obs_dev [nsteps,N,17], reward_dev [nsteps,N],
 * terminated_dev / truncated_dev / info_dev (or NULL) [nsteps,N], eta_dev [nsteps,N,3] or NULL.
 * For action sequences fixed in advance (sampling-based planning, data generation, replay); no
 * reset-info compaction; not available with HG_RESET_RETRIM. */
int32_t hg_rollout(hg_env* env, const float* actions_dev, int32_t nsteps, float* obs_dev, float* reward_dev,
                   uint8_t* terminated_dev, uint8_t* truncated_dev, uint8_t* info_dev, const float* eta_dev,
                   void* stream);

/* ---- Closed-loop rollouts: an MLP policy held by the handle and evaluated inside the rollout kernel.
 *
 * Model (fixed):   x = (obs - obs_mean) * obs_scale                               [17]
 *                  a = W3 tanh(W2 tanh(W1 x + b1) + b2) + b3 + exp(log_std) * z     [4]
 * W1 [64,17], b1 [64], W2 [64,64], b2 [64], W3 [4,64], b3 [4], row-major [out,in] as torch.nn.Linear
 * stores them; log_std [4], obs_mean [17], obs_scale [17]; all fp32.  Two hidden layers of width 64
 * with tanh, no other size or activation.  The action is the raw sampled value: it is not clipped
 * (the reference does not clip actions either).
 * Arithmetic: fp32 throughout.  Each matrix product is an fp32 fused-multiply-add chain (the exact
 * fp32 matrix instruction, one rounding per product, the bias added last); tanh(v) = sign(v) (1 - t) /
 * (1 + t) with t = exp2(-2 log2(e) |v|); x is one subtraction and one multiplication; the noise is
 * added as fma(exp(log_std), z, mean action).  Against an fp64 evaluation of the same weights the
 * error is that of an fp32 evaluation in another summation order.
 * Noise: absent when log_std is NULL (deterministic policy: nothing is drawn).  Otherwise z is four
 * standard normals from ONE Philox4x32-10 call and Box-Muller, by the device functions of the
 * turbulence noise (hg_debug_eta):
 *   counter = (gid_lo, gid_hi, episode step, episode index), gid = env_offset + i, the env's raw
 *             counters (the step counter of an env waiting for its next-step reset is negative),
 *             exactly the turbulence noise's counter;
 *   key     = (seed_lo ^ 0x706F6C69, seed_hi ^ 0x63795F7A)  -- the turbulence key is (seed_lo, seed_hi),
 *             so these two constants separate the streams;
 *   words (r0, r1, r2, r3) -> u(r) = ((r >> 8) + 0.5) 2^-24 in fp32 (in (0, 1]), turn fraction
 *             f(r) = (r >> 9) 2^-23;   R0 = sqrt(-2 ln u(r0)), R1 = sqrt(-2 ln u(r2));
 *             z = (R0 cos 2 pi f(r1), R0 sin 2 pi f(r1), R1 cos 2 pi f(r3), R1 sin 2 pi f(r3)).
 * The noise depends on the env's own counters only: it is the same however the envs are sharded
 * over handles (env_offset), and the same in hg_rollout_policy and hg_policy_act.
 *
 * hg_set_policy: copy (repack) the weights into the handle's own device buffer, allocated by
 * hg_create.  All arguments are device pointers; log_std, obs_mean, obs_scale may be NULL (no noise /
 * 0 / 1).  Asynchronous on `stream`, allocates nothing, capturable into a graph: a training loop
 * calls it once per update.  Like hg_rollout it ends a sequence of chained steps. */
int32_t hg_set_policy(hg_env* env, const float* W1_dev, const float* b1_dev, const float* W2_dev,
                      const float* b2_dev, const float* W3_dev, const float* b3_dev, const float* log_std_dev,
                      const float* obs_mean_dev, const float* obs_scale_dev, void* stream);

/* One action per env, actions_dev [N,4] (16-byte aligned), of the policy applied to obs_dev [N,17]
 * with the noise of each env's current counters (read from the env's state as hg_debug_eta reads
 * them).  The env is not modified.  The same device function as hg_rollout_policy's: acting and
 * stepping (hg_step) in turn is bitwise that rollout.  HG_E_INVALID if no policy was set. */
int32_t hg_policy_act(hg_env* env, const float* obs_dev, float* actions_dev, void* stream);

/* hg_rollout with the actions computed in the kernel: step 0's from obs0_dev [N,17], step s+1's from
 * the observation row step s writes (for an env auto-reset in step s that is its reset observation,
 * per-env templates included).  The sampled actions go to actions_out_dev [nsteps,N,4]; the other
 * outputs are stacked exactly as hg_rollout's.  Same restrictions and argument checks as hg_rollout
 * (no auto-resets in HG_RESET_RETRIM; actions_out_dev and obs_dev 16-byte aligned); HG_E_INVALID if no
 * policy was set.  One wave per SIMD (the weights stay in registers across the steps); counted by
 * hg_debug_launches as a lone-wave launch, like hg_rollout's. */
int32_t hg_rollout_policy(hg_env* env, const float* obs0_dev, int32_t nsteps, float* actions_out_dev,
                          float* obs_dev, float* reward_dev, uint8_t* terminated_dev, uint8_t* truncated_dev,
                          uint8_t* info_dev, const float* eta_dev, void* stream);

/* ---- Actor-critic rollouts: what a PPO / A2C learner needs beside the actions, from the same launch.
 *
 * Value head (fixed):   v = w_v . tanh(h2) + b_v,   h2 = W2 tanh(W1 x + b1) + b2 the policy's second
 * hidden layer: w_v [64], b_v [1], fp32, sharing the policy's trunk.  It is one more row of the last
 * matrix product, so it adds no matrix instruction, and the actions are bitwise the same with or
 * without it.  (A separate critic network is not offered: it would double the matrix work and does not
 * fit the register file beside the actor.)
 * Log-probability:   logp = -1/2 (z0^2 + z1^2 + z2^2 + z3^2) - (log_std0 + .. + log_std3) - 2 ln(2 pi),
 * from the z the action was built from (not from (a - mean) / std), fp32, the squares as one fma chain;
 * the sum of log_std is formed left to right by hg_set_policy.  0 for a deterministic policy.
 *
 * hg_set_value_head: copy w_v, b_v (device pointers) into the handle's policy buffer.  It and
 * hg_set_policy write disjoint parts of that buffer: either order gives the same result and a later
 * hg_set_policy keeps the head.  Asynchronous on `stream`, allocates nothing, capturable. */
int32_t hg_set_value_head(hg_env* env, const float* wv_dev, const float* bv_dev, void* stream);

/* hg_policy_act with two more outputs, each [N] fp32 or NULL (actions_dev may be NULL too): the
 * log-probability of each action and the value head's V(obs).  HG_E_INVALID for value_dev while no
 * value head is set.  The env is not modified.  The device function is hg_rollout_ac's: evaluating
 * and stepping (hg_step) in turn is bitwise that rollout. */
int32_t hg_policy_eval(hg_env* env, const float* obs_dev, float* actions_dev, float* logp_dev, float* value_dev,
                       void* stream);

/* hg_rollout_policy with three more [nsteps,N] fp32 outputs, each of them or NULL (value_dev and
 * next_value_dev together or not at all; they need a value head).  The first six outputs, the env's
 * state and its counters are bitwise hg_rollout_policy's.  With o_0 = obs0 and o_k = obs[k-1], the
 * observation action k was computed from:
 *   logp[k]       = log pi(a_k | o_k)
 *   value[k]      = V(o_k)
 *   next_value[k] = terminated[k] ? 0 : V(o'_k), where o'_k is the observation step k produced BEFORE
 *                   any auto-reset: obs[k], unless info[k] has HG_INFO_RESET -- then the terminal
 *                   observation hg_step_rows would put in final_obs_rows, which no other output of a
 *                   rollout carries.  So a TimeLimit truncation bootstraps from the value of the state
 *                   the episode was cut at, and a termination from 0.
 * Modes: hg_rollout_policy's without HG_AUTORESET_NEXT_STEP (the filler transition of a next-step
 * reset would need a validity mask the advantage recursion does not have): HG_E_INVALID. */
int32_t hg_rollout_ac(hg_env* env, const float* obs0_dev, int32_t nsteps, float* actions_out_dev, float* obs_dev,
                      float* reward_dev, uint8_t* terminated_dev, uint8_t* truncated_dev, uint8_t* info_dev,
                      const float* eta_dev, float* logp_dev, float* value_dev, float* next_value_dev, void* stream);

/* Generalised advantage estimation over [nsteps,N] rows (N the env's), from the last step back:
 *   delta_k = reward[k] + gamma next_value[k] - value[k]
 *   A_k     = delta_k + gamma lam ((terminated[k] | truncated[k]) ? 0 : A_{k+1}),   A_nsteps = 0
 *   ret_k   = A_k + value[k]
 * adv_out_dev [nsteps,N]; ret_out_dev [nsteps,N] or NULL.  The flags cut the chain by selection, so
 * nothing (not a NaN either) crosses an episode's end.  fp32, each line one fused multiply-add.  Takes
 * hg_rollout_ac's outputs as they are, or a caller's own critic's values.  The env is not modified. */
int32_t hg_gae(hg_env* env, const float* reward_dev, const float* value_dev, const float* next_value_dev,
               const uint8_t* terminated_dev, const uint8_t* truncated_dev, int32_t nsteps, float gamma, float lam,
               float* adv_out_dev, float* ret_out_dev, void* stream);

/* ---- The update half: the clipped PPO loss's gradient for the actor-critic above, in one kernel.
 *
 * Flat parameter vector theta [HG_PPO_N_PARAMS] fp32, each tensor row-major [out,in] as torch.nn.Linear
 * stores it (offset: tensor, count):
 *      0: W1 [64,17] 1088     1088: b1 [64] 64      1152: W2 [64,64] 4096     5248: b2 [64] 64
 *   5312: W3 [4,64] 256       5568: b3 [4] 4        5572: log_std [4] 4
 *   5576: w_v [64] 64         5640: b_v [1] 1
 * The call takes these raw weights, the LEARNER's current ones, not the handle's packed policy image:
 * the weights change with every optimiser step inside an epoch, hg_set_policy is called once per
 * collection.  `env` is used only for its device and the error convention (hg_last_error), as in hg_gae;
 * the env is not modified: not its state, counters, azimuth records, the chain bookkeeping of
 * hg_step_chained, nor the overlapped re-trim.
 *
 * The function.  Rows i of the minibatch: index_dev[0..M) into the B stored rows, or, with index_dev
 * NULL, the rows 0..B-1 themselves (then M == B):
 *   x = (obs_i - mean) * scale;  h1 = tanh(W1 x + b1);  h2 = tanh(W2 h1 + b2);  mu = W3 h2 + b3;  v = w_v . h2 + b_v
 *   z = (a_i - mu) * exp(-log_std);   logp = -1/2 sum z^2 - sum log_std - 2 ln(2 pi);   r = exp(logp - logp_old_i)
 *   L = (1/M) sum_i [ -min(r A_i, clamp(r, 1 - clip, 1 + clip) A_i) + vf_coef * 1/2 (v - ret_i)^2 ] - ent_coef * H,
 *   H = sum log_std + 2 (1 + ln(2 pi))
 * grad_dev [HG_PPO_N_PARAMS] = dL/dtheta in theta's layout, as torch autograd differentiates that
 * expression: a sample contributes nothing through r when (A_i > 0 and r > 1 + clip) or (A_i < 0 and
 * r < 1 - clip), and -A_i r dlogp otherwise.  grad_dev is overwritten, not accumulated into.
 * Numerics: fp32 throughout; tanh is the policy's formula above and tanh' = 1 - h^2; every matrix
 * product, forward and backward, is an exact fp32 fma chain on the fp32 matrix instruction (the biases
 * the last k pair of the forward chains, as in the rollout kernels); the sums over samples are fp32.
 * stats_dev [8] or NULL:  [0] mean policy term  [1] mean 1/2 (v - ret)^2, unweighted
 *   [2] mean (logp_old - logp), the usual approximate KL  [3] fraction of samples with r outside
 *   [1 - clip, 1 + clip]  [4] H  [5] L  [6] mean r  [7] skipped index entries, as a float.
 * Out-of-range index entries (outside [0, B)) are skipped and counted, never dereferenced; the means
 * still divide by M (1/M is a kernel argument).
 * Asynchronous on `stream`, allocates nothing, capturable; theta_dev is read when the kernel runs, so a
 * replayed graph sees updated weights.  Deterministic: no floating-point atomics; per-block partial sums
 * go to workspace_dev (hg_ppo_grad_workspace_bytes() bytes, 16-byte aligned, contents irrelevant before
 * and after) and are added in a fixed order, and the launch shape depends on M and compile-time constants
 * only: two calls on the same inputs give the same bits.
 * HG_E_INVALID, outputs untouched: NULL env; a NULL or misaligned (4 bytes; actions_dev and
 * workspace_dev 16) required pointer; B < 1; M < 1; M > 2^31 - 256; index_dev NULL with M != B; clip not
 * in (0, 1); a non-finite or negative vf_coef or ent_coef.  obs_mean_dev / obs_scale_dev [17] or NULL
 * (0 / 1) are constants of the function, not differentiated. */
#define HG_PPO_N_PARAMS 5641

int64_t hg_ppo_grad_workspace_bytes(void);      /* fixed; a multiple of 16; host only */

int32_t hg_ppo_grad(hg_env* env, const float* theta_dev,           /* [5641] the LEARNER's current weights */
                    const float* obs_mean_dev, const float* obs_scale_dev,   /* [17] or NULL (0 / 1); constants */
                    const float* obs_dev, const float* actions_dev,          /* [B,17], [B,4] (16-byte aligned) */
                    const float* logp_old_dev, const float* adv_dev, const float* ret_dev,   /* [B] */
                    int64_t B, const int32_t* index_dev, int64_t M,           /* minibatch rows, or NULL: M == B, rows 0..B-1 */
                    float clip, float vf_coef, float ent_coef,
                    float* grad_dev,      /* [5641] out, overwritten (not accumulated) */
                    float* stats_dev,     /* [8] out or NULL */
                    void* workspace_dev, void* stream);

/* ---- The supervised half: the weighted imitation loss's gradient, the same kernel with a second loss head.
 *
 * For a caller that holds states, better actions and better return estimates -- a planner's (hg_mppi_value),
 * a hand-written controller's, logged flights: behaviour cloning, DAgger / expert iteration,
 * advantage-weighted regression.  theta's layout, the rows (index_dev[0..M) into the B stored rows, or
 * 0..B-1 with index_dev NULL and M == B) and x, h1, h2, mu, v are hg_ppo_grad's, computed by the same code:
 *   z_c  = (a*_i,c - mu_c) * exp(-log_std_c)
 *   logp = -1/2 sum z^2 - sum log_std - 2 ln(2 pi)             (hg_ppo_grad's expression, the same fma chain)
 *   mode HG_BC_NLL:  l_i = -logp                                (log_std is trained)
 *   mode HG_BC_MSE:  l_i = 1/2 sum_c (a*_i,c - mu_c)^2          (log_std sees only the entropy term)
 *   L = (1/M) sum_i [ w_i l_i + vf_coef * 1/2 (v - y_i)^2 ] - ent_coef * H,   H = sum log_std + 2 (1 + ln(2 pi))
 * target_dev [B,4]: the actions a*, 16-byte aligned.
 * weight_dev [B] or NULL (w = 1, bitwise a tensor of ones).  The weights are used as given: a negative one
 *   pushes away from its target, a non-finite one gives a non-finite gradient, which hg_ppo_adam's guard
 *   drops.  The value term is unweighted.
 * value_target_dev [B], the y, or NULL: NULL requires vf_coef == 0; the pointer is then never read, the
 *   value term is 0 and so is stats[1].
 * grad_dev [HG_PPO_N_PARAMS] = dL/dtheta in theta's layout, overwritten.  Per sample, with g = -w_i / M:
 *   NLL: dL/dmu_c = g z_c exp(-log_std_c), dL/dlog_std_c += g (z_c^2 - 1);   MSE: dL/dmu_c = -(a*_c - mu_c) w_i / M
 *   and nothing on log_std, whose gradient is then -ent_coef bitwise.  dL/dv = vf_coef (v - y_i) / M.
 * stats_dev [8] or NULL:  [0] mean w l  [1] mean 1/2 (v - y)^2  [2] mean sum_c (a* - mu)^2, unweighted, in
 *   both modes  [3] mean w  [4] H  [5] L = [0] + vf_coef [1] - ent_coef H  [6] mean logp(a*), unweighted
 *   [7] skipped index entries, as a float.  (hg_ppo_grad's reduction, unchanged: five sums times 1/M.)  In
 *   mode HG_BC_NLL with weight_dev NULL, [0] == -[6] bitwise.
 * Everything else is hg_ppo_grad's: fp32 and exact fma chains on the fp32 matrix instruction; out-of-range
 * index entries skipped and counted, the means still dividing by M; asynchronous on `stream`, allocates
 * nothing, capturable, theta_dev read when the kernel runs; deterministic (no atomics, partial sums through
 * workspace_dev, hg_ppo_grad_workspace_bytes() bytes, added in a fixed order; the launch shape a function of
 * M and compile-time constants); the env is not modified.
 * HG_E_INVALID, outputs untouched: NULL env; a NULL or misaligned (4 bytes; target_dev and workspace_dev
 * 16) required pointer; a misaligned optional one; B < 1; M < 1; M > 2^31 - 256; index_dev NULL with
 * M != B; a mode outside the enum; a non-finite or negative vf_coef or ent_coef; value_target_dev NULL with
 * vf_coef != 0. */
enum { HG_BC_NLL = 0, HG_BC_MSE = 1 };

int32_t hg_bc_grad(hg_env* env, const float* theta_dev,            /* [5641] the LEARNER's current weights */
                   const float* obs_mean_dev, const float* obs_scale_dev,    /* [17] or NULL (0 / 1); constants */
                   const float* obs_dev, const float* target_dev,            /* [B,17], [B,4] (16-byte aligned) */
                   const float* weight_dev,                                  /* [B] or NULL: w = 1 */
                   const float* value_target_dev,                            /* [B] or NULL: needs vf_coef == 0 */
                   int64_t B, const int32_t* index_dev, int64_t M,            /* minibatch rows, or NULL: M == B, rows 0..B-1 */
                   int32_t mode, float vf_coef, float ent_coef,
                   float* grad_dev,      /* [5641] out, overwritten (not accumulated) */
                   float* stats_dev,     /* [8] out or NULL */
                   void* workspace_dev, void* stream);

/* ---- The update phase on the device: minibatch shuffle, gradient clipping, Adam, and all of it in one call.
 *
 * Every call below is asynchronous on `stream`, allocates nothing, makes no host decision that depends on
 * device data and can be captured into a graph; `env` is used for its device and the error convention
 * only and is not modified (hg_set_policy_theta excepted: it is hg_set_policy + hg_set_value_head).
 *
 * Optimiser state: hg_ppo_opt_state_bytes() = 45248 bytes of device memory, 16-byte aligned, owned by the
 * caller.  In 4-byte words (offset: content):
 *       0: m [5641] fp32, Adam's first moment, in theta's layout
 *    5648: v [5641] fp32, the second moment
 *   11296: a tail of 16 words:
 *          +0 applied            i32  Adam steps taken: the t of the bias corrections
 *          +1 seen               i32  hg_ppo_adam calls, applied or not
 *          +2 stop               i32  set by the approximate-KL early stop, cleared by hg_ppo_update's start
 *          +3 skipped_nonfinite  i32  calls dropped because the gradient norm was not finite
 *          +4 skipped_stopped    i32  calls dropped because `stop` was set (the one that set it included)
 *          +5 last_norm          fp32 the last computed gradient norm, before clipping
 *          +6 last_clip_coef     fp32 the last applied clip coefficient
 *          +7 .. +15             reserved, zero
 *   (words 5641 .. 5647 and 11289 .. 11295 are padding, zero.)
 * hg_ppo_opt_init zeroes the state (one kernel). */
int64_t hg_ppo_opt_state_bytes(void);           /* fixed; a multiple of 16; host only */
int32_t hg_ppo_opt_init(hg_env* env, void* state_dev, void* stream);

/* A stateless random permutation of 0 .. B-1 into index_out_dev [B] i32: no sort, no scratch memory.
 *   e = epoch + (epoch_dev ? *epoch_dev : 0), a 64-bit sum; epoch_dev is read when the kernel runs, so a
 *       replayed graph whose epoch_dev points at a counter draws a new permutation every replay.
 *   w = max(1, bit_length(B - 1)),  half = ceil(w / 2),  mask = 2^half - 1.
 *   Element i starts at x = i.  One pass: L = x >> half, R = x & mask; four Feistel rounds j = 0 .. 3,
 *       (L, R) <- (R, L ^ (F(R, j) & mask));  x = (L << half) | R.
 *   Passes repeat while x >= B (cycle walking); index[i] is the first x < B.  The passes permute
 *   [0, 4^half), a domain under 4 B, and the orbit of i returns to i < B: the walk always ends, after
 *   under 4 passes in the mean.
 *   F(R, j) = word 0 of Philox4x32-10 on the counter (R, j, e_lo, e_hi) with the key
 *   (seed_lo ^ 0x73687566, seed_hi ^ 0x666C655F).
 * HG_E_INVALID, output untouched: NULL env; NULL index_out_dev; a misaligned (4 bytes) pointer; B < 1;
 * B > 2^31 - 256. */
int32_t hg_ppo_shuffle(hg_env* env, int64_t B, uint64_t seed, int64_t epoch, const int32_t* epoch_dev,
                       int32_t* index_out_dev, void* stream);

/* The optimiser's settings: a host struct, read when the call is made. */
typedef struct hg_ppo_opt_cfg {
    double lr;             /* learning rate */
    const float* lr_dev;   /* device pointer or NULL; if set the kernel uses *lr_dev, read when it runs, in
                              place of lr: a schedule is one 4-byte copy between replays of a captured graph */
    double beta1, beta2;   /* Adam's betas, in [0, 1) */
    double eps;            /* Adam's epsilon */
    float max_grad_norm;   /* global gradient-norm clip; <= 0 or +inf: off */
    float target_kl;       /* approximate-KL early stop; <= 0: off */
} hg_ppo_opt_cfg;

/* One optimiser step: theta_dev [5641] updated in place from grad_dev [5641] (not modified); stats_dev
 * [8], hg_ppo_grad's statistics of the minibatch grad_dev came from, or NULL.  With the tail's words of
 * state_dev as named above, in this order:
 *   1. seen += 1.
 *   2. If stop is set: skipped_stopped += 1, done.
 *   3. If target_kl > 0 and stats_dev is given and stats[2] > 1.5 target_kl (fp32): set stop,
 *      skipped_stopped += 1, done.  (The usual rule: stats[2] was measured at the weights the previous
 *      steps left, so this minibatch and every later one are dropped until stop is cleared.)
 *   4. nrm = sqrt(sum g^2) in fp32, in a fixed order that depends on compile-time constants only
 *      (csrc/ppo_opt.hip states it); last_norm = nrm.
 *   5. If nrm is not finite: skipped_nonfinite += 1, done; theta, m, v and applied stay bitwise as they are.
 *   6. c = max_grad_norm on ? min(1, max_grad_norm / (nrm + 1e-6)) : 1  (torch's clip_grad_norm_);
 *      last_clip_coef = c.
 *   7. g' = c g.
 *   8. applied += 1;  t = applied.
 *   9. m = fma(beta1, m, (1 - beta1) g');   v = fma(beta2, v, ((1 - beta2) g') g').
 *  10. theta = fma(-(lr / (1 - beta1^t)), m / fma(sqrt(v), 1 / sqrt(1 - beta2^t), eps), theta).
 * Precision: lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) are formed in fp64 on the device from the double
 * betas, t and lr (or (double)*lr_dev) and rounded to fp32 once; beta, 1 - beta and eps are rounded to
 * fp32 once from double; everything per element is fp32.
 * Deterministic: one block, no atomics; two calls on equal inputs give equal bits.
 * HG_E_INVALID, nothing touched: NULL env; NULL theta_dev, grad_dev, state_dev or cfg; a misaligned pointer
 * (4 bytes; state_dev 16); lr or eps non-finite or negative; a beta outside [0, 1) or non-finite; NaN
 * max_grad_norm or target_kl. */
int32_t hg_ppo_adam(hg_env* env, float* theta_dev, const float* grad_dev, const float* stats_dev, void* state_dev,
                    const hg_ppo_opt_cfg* cfg, void* stream);

/* The whole update phase, enqueued by one call.  The arguments up to workspace_dev are hg_ppo_grad's
 * (theta_dev is also written); index_dev [B] i32 is scratch for the permutations; stats_out_dev
 * [n_epochs * n_minibatches, 8] receives each minibatch's statistics row, or NULL -- but target_kl > 0
 * REQUIRES stats_out_dev (the early stop reads the row): HG_E_INVALID without it.
 *   stop = 0 (one single-thread kernel);
 *   for each epoch:  hg_ppo_shuffle(B, seed, epoch = 0, epoch_dev = the state's `seen` word) -> index_dev;
 *     for minibatch j = 0 .. n_minibatches-1, rows [floor(j B / n), floor((j + 1) B / n)) of index_dev:
 *       hg_ppo_grad over that slice (its two launches) -> grad_dev and the minibatch's stats row,
 *       hg_ppo_adam(theta_dev, grad_dev, that row, state_dev, cfg).
 * `seen` advances with every optimiser call, so every epoch of every call, and every replay of a captured
 * call, draws another permutation.  The results are bitwise those of the same calls made one by one.
 * HG_E_INVALID before anything is enqueued: what hg_ppo_shuffle, hg_ppo_grad and hg_ppo_adam refuse;
 * n_epochs < 1; n_minibatches outside 1 .. B. */
int32_t hg_ppo_update(hg_env* env, float* theta_dev, const float* obs_mean_dev, const float* obs_scale_dev,
                      const float* obs_dev, const float* actions_dev, const float* logp_old_dev, const float* adv_dev,
                      const float* ret_dev, int64_t B, float clip, float vf_coef, float ent_coef, float* grad_dev,
                      void* workspace_dev, int32_t n_epochs, int32_t n_minibatches, uint64_t seed, int32_t* index_dev,
                      float* stats_out_dev, void* state_dev, const hg_ppo_opt_cfg* cfg, void* stream);

/* hg_ppo_update's loop with hg_bc_grad as the gradient: the same optimiser state, cfg, slice rule, index_dev
 * scratch and stats_out_dev [n_epochs * n_minibatches, 8] (hg_bc_grad's rows, or NULL); the arguments up to
 * workspace_dev are hg_bc_grad's.
 *   stop = 0;  for each epoch: hg_ppo_shuffle keyed on the state's `seen` word;  for each minibatch:
 *   hg_bc_grad over the slice, then hg_ppo_adam with cfg's target_kl taken as 0.
 * The results are bitwise those of the same calls made one by one.  cfg->target_kl > 0 is refused: the
 * optimiser's early stop reads stats[2], which is a squared action error here, not a KL.
 * HG_E_INVALID before anything is enqueued: what hg_ppo_shuffle, hg_bc_grad and hg_ppo_adam refuse;
 * target_kl > 0; n_epochs < 1; n_minibatches outside 1 .. B. */
int32_t hg_bc_update(hg_env* env, float* theta_dev, const float* obs_mean_dev, const float* obs_scale_dev,
                     const float* obs_dev, const float* target_dev, const float* weight_dev,
                     const float* value_target_dev, int64_t B, int32_t mode, float vf_coef, float ent_coef,
                     float* grad_dev, void* workspace_dev, int32_t n_epochs, int32_t n_minibatches, uint64_t seed,
                     int32_t* index_dev, float* stats_out_dev, void* state_dev, const hg_ppo_opt_cfg* cfg, void* stream);

/* Publish the learner's weights to the env: hg_set_policy + hg_set_value_head on the tensors of a flat
 * theta_dev [5641] (log_std included: a stochastic policy), bitwise those two calls.  obs_mean_dev /
 * obs_scale_dev [17] or NULL. */
int32_t hg_set_policy_theta(hg_env* env, const float* theta_dev, const float* obs_mean_dev, const float* obs_scale_dev,
                            void* stream);

/* ---- Running normalisation and episode statistics: one pass over what a rollout wrote.
 *
 * What SB3's VecNormalize / gymnasium's NormalizeObservation + NormalizeReward and an episode monitor keep,
 * kept on the device across calls: running moments of the observations and of the discounted return, per-env
 * return and length accumulators that survive the end of a K-step launch, and the aggregates of the episodes
 * that ended in this one.  Asynchronous on `stream`, allocates nothing, capturable.  The env is not modified:
 * it is used for N, its device and the error convention, as in hg_gae.
 *
 * Inputs, a rollout's outputs as they are (N the env's): obs_dev [nsteps,N,17] fp32, reward_dev [nsteps,N]
 * fp32, terminated_dev / truncated_dev [nsteps,N] u8; info_dev [nsteps,N] u8 or NULL (the success count is
 * then 0); obs0_dev [N,17], the observations the rollout started from, required iff obs_in_out_dev is given.
 *
 * State: hg_rollout_stats_state_bytes(n_envs) bytes of device memory, 16-byte aligned, owned by the caller
 * (byte offset: content):
 *        0: an fp64 head of 48 doubles (double index: content):
 *             0: obs_count              rows that entered the observation moments
 *             1: obs_mean [17]
 *            18: obs_M2 [17]            sum of squared deviations: the population variance is M2 / count
 *            35: ret_count              samples of G that entered the return moments
 *            36: ret_mean
 *            37: ret_M2
 *            38: episodes               lifetime total of completed episodes
 *            39: env_steps              lifetime total of env-steps
 *            40: skipped_rows           lifetime total of observation rows left out (a non-finite value)
 *            41: skipped_returns        lifetime total of return samples left out (non-finite)
 *            42 .. 47                   reserved, zero
 *      384: G [N] fp32, each env's discounted return so far
 *   384 + 4 N: ep_ret [N] fp32, the running episode's return
 *   384 + 8 N: ep_len [N] i32, its length
 *   384 + 12 N, rounded up to a multiple of 16: a workspace of 180240 bytes for the kernels' partial sums,
 *             its contents irrelevant between calls.
 * hg_rollout_stats_init zeroes all of it (one kernel, not a memset).
 *
 * Per env n, for k = 0 .. nsteps-1, in this order (fp32; gamma is the configuration's, rounded to fp32 once):
 *   1. G = fma(gamma, G, reward[k,n]); the sample G enters the return moments.
 *   2. ep_ret = ep_ret + reward[k,n];  ep_len = ep_len + 1.
 *   3. If terminated[k,n] | truncated[k,n]: the episode (ep_ret, ep_len, terminated[k,n] != 0,
 *      info[k,n] & HG_INFO_SUCCESSED) enters this call's episode aggregates, then G, ep_ret and ep_len are set
 *      to 0 (by assignment: a NaN does not survive its episode's end).
 * Observation moments: over all nsteps * N rows of obs_dev, per column, population moments.  The batch is
 * accumulated in fp64 as shifted sums, sum (x - c) and sum (x - c)^2, with c the state's mean when obs_count
 * > 0 and otherwise the row obs[0,0,:] (a non-finite value of it replaced by 0), and merged into the state
 * by Chan's update; the return moments likewise, with c the state's ret_mean or 0.  A row with any non-finite
 * value is left out of all 17 columns and counted; a non-finite sample of G is left out of the return moments
 * and counted (G, ep_ret carry what the arithmetic gives until the episode's end clears them); an episode
 * whose return is not finite is counted, with its length and flags, but left out of the return statistics.
 * Nothing non-finite ever enters the head.
 *
 * Outputs, each or NULL, all from the state AFTER this call's merge (SB3's order):
 *   obs_mean_out_dev [17]     (float)obs_mean
 *   obs_scale_out_dev [17]    min((float)(1 / sqrt(obs_M2 / obs_count + obs_eps)), max_obs_scale), fp64 rounded once
 *   reward_scale_out_dev [1]  (float)(1 / sqrt(ret_M2 / ret_count + ret_eps))
 *   reward_out_dev [nsteps,N] clamp(reward * reward_scale, +-clip_reward): one fp32 multiply, a NaN stays a NaN;
 *                             must not be reward_dev
 *   obs_in_out_dev [nsteps,N,17]  the observations the actions were computed from: obs_in[0] = obs0,
 *                             obs_in[k] = obs[k-1], bitwise
 *   episode_out_dev [16] fp32 [0] episodes completed in this call  [1] mean, [2] population standard deviation,
 *                             [3] min, [4] max of their returns  [5] their mean length  [6] of them terminated
 *                             [7] truncated only  [8] with HG_INFO_SUCCESSED  [9] mean finite reward per step of
 *                             the batch  [10] observation rows, [11] return samples left out in this call
 *                             [12] episodes with a non-finite return (left out of [1] .. [4])  [13] .. [15] zero.
 *                             Without a completed episode [1] .. [5] are NaN and the counts 0.
 * With a count of 0 the mean is 0 and the scales are 1.
 *
 * cfg.update: a cleared bit freezes that part of the head and the outputs come from the state as it stands
 * (evaluation).  HG_STATS_UPDATE_OBS: the observation moments and skipped_rows; HG_STATS_UPDATE_RET: the
 * return moments and skipped_returns; episodes and env_steps advance when either bit is set.  The per-env
 * scans and the episode aggregates always run.
 *
 * Deterministic: no atomics; the launch shapes depend on (nsteps, N) and compile-time constants only and the
 * partial sums are added in a fixed order (csrc/rollout_stats.hip states it): two calls on the same inputs
 * and state give the same bits.
 * HG_E_INVALID, outputs and state untouched: NULL env; NULL state_dev, obs_dev, reward_dev, terminated_dev,
 * truncated_dev or cfg; a misaligned pointer (state_dev, obs_dev, obs0_dev, obs_in_out_dev 16 bytes, the other
 * fp32 pointers 4); nsteps < 1; obs_in_out_dev without obs0_dev; reward_out_dev == reward_dev; gamma outside
 * [0, 1] or NaN; a negative or NaN eps; max_obs_scale or clip_reward NaN or <= 0; unknown update bits. */
enum { HG_STATS_UPDATE_OBS = 1, HG_STATS_UPDATE_RET = 2 };

typedef struct hg_rollout_stats_cfg {
    double gamma;          /* the discount of G, in [0, 1] */
    double obs_eps;        /* added to the observation variance under the square root, >= 0 */
    double ret_eps;        /* added to the return variance under the square root, >= 0 */
    float max_obs_scale;   /* upper bound of obs_scale; +inf: off */
    float clip_reward;     /* bound of |reward_out|; +inf: off */
    uint32_t update;       /* HG_STATS_UPDATE_* bits */
    uint32_t reserved;     /* zero */
} hg_rollout_stats_cfg;

int64_t hg_rollout_stats_state_bytes(int64_t n_envs);   /* a multiple of 16; negative for n_envs < 1; host only */
int32_t hg_rollout_stats_init(hg_env* env, void* state_dev, void* stream);
int32_t hg_rollout_stats(hg_env* env, void* state_dev, const float* obs_dev, const float* reward_dev,
                         const uint8_t* terminated_dev, const uint8_t* truncated_dev, const uint8_t* info_dev,
                         const float* obs0_dev, int32_t nsteps, const hg_rollout_stats_cfg* cfg, float* obs_mean_out_dev,
                         float* obs_scale_out_dev, float* reward_scale_out_dev, float* reward_out_dev,
                         float* obs_in_out_dev, float* episode_out_dev, void* stream);

/* ---- Branched planning rollouts: many candidate action sequences per env, scored without touching it.
 *
 * What a receding-horizon sampling planner (MPPI, CEM, random shooting) needs from the rollout: `branches`
 * candidates per env, all starting from the env's current state, each reduced to one discounted return.
 * Row r = e * branches + b of every [N*branches] array is branch b of env e.  All three calls are
 * asynchronous on `stream`, allocate nothing, can be captured into a graph, and do not modify the env:
 * not its state, counters, azimuth records, the chain bookkeeping of hg_step_chained, nor the overlapped
 * re-trim.  HG_E_INVALID (env untouched) for horizon < 1, branches < 1, N * branches >= 2^31 - 256, a
 * NULL or misaligned pointer, and what each call names below.
 *
 * hg_rollout_branch: actions_dev [horizon, N*branches, 4] (16-byte aligned) -> return_dev [N*branches],
 * alive_steps_dev [N*branches] i32 or NULL, end_info_dev [N*branches] u8 or NULL.
 *   Branch b of env e starts from env e's state and counters exactly as the env's next hg_step would read
 *   them and evolves exactly as hg_rollout would evolve that env under actions[t, r], up to and including
 *   the first step whose terminated or truncated flag is set (failure, success, max_time,
 *   max_episode_steps); after it the branch contributes nothing.  There is never a reset inside a
 *   branch, whatever the handle's autoreset, autoreset_mode or reset_mode: HG_RESET_RETRIM handles are
 *   accepted.  The branches of an env waiting for its next-step auto-reset (negative step counter: its
 *   next step ignores the action) return 0 with alive_steps 0 and end_info 0.
 *   return[r]      = sum over t < T_r of gamma^t reward_t, fp32, in step order: G = fma(disc, reward_t, G),
 *                    then disc = disc * gamma, from G = 0, disc = 1;  gamma in (0, 1].
 *   alive_steps[r] = T_r, the steps up to and including the ending one (horizon for a surviving branch).
 *   end_info[r]    = the ending step's HG_INFO_* bits without HG_INFO_RESET; 0 for a surviving branch.
 *   noise_mode HG_BRANCH_NOISE_ENV: the turbulence noise of env e's own key (env_offset + e, its episode
 *     step and episode index): every branch of an env meets the realisation the env itself will meet.
 *     These are common random numbers between the candidates, and they make the call bitwise hg_rollout
 *     of that env.  Stated plainly: THIS PLANNER SEES THE GUSTS AHEAD -- its returns are those of the
 *     noise the env is about to draw, which no real controller knows.
 *   noise_mode HG_BRANCH_NOISE_OFF: eta = 0 through the same wind step, a certainty-equivalent planner;
 *     bitwise hg_rollout with an all-zero eta_dev.
 *   Counted by hg_debug_launches as a lone-wave launch while N * branches rows fit two waves per SIMD,
 *   as a bulk launch past that. */
enum { HG_BRANCH_NOISE_ENV = 0, HG_BRANCH_NOISE_OFF = 1 };

int32_t hg_rollout_branch(hg_env* env, const float* actions_dev, int32_t horizon, int32_t branches, float gamma,
                          int32_t noise_mode, float* return_dev, int32_t* alive_steps_dev, uint8_t* end_info_dev,
                          void* stream);

/* Candidates around a nominal sequence nominal_dev [horizon, N, 4] -> actions_out_dev [horizon, N*branches, 4]
 * (both 16-byte aligned):   actions_out[t, r, c] = clamp(nominal[t, e, c] + sigma[c] * z_c, lo[c], hi[c]),
 * the sum one fma.  Branch 0 has no perturbation: it is the clamped nominal.  z is four standard normals
 * from ONE Philox4x32-10 call with counter (gid_lo, gid_hi, t, b), gid = env_offset + e, and key
 * (sample_seed_lo, sample_seed_hi), through the Box-Muller of the policy noise above (same device
 * functions).  Keyed by the global env id: the rows do not depend on how the envs are sharded.  The
 * caller varies sample_seed per control step.  sigma (finite, >= 0), lo <= hi: host arrays of 4, passed
 * by value into the kernel's arguments. */
int32_t hg_mppi_sample(hg_env* env, const float* nominal_dev, int32_t horizon, int32_t branches, const float sigma[4],
                       const float lo[4], const float hi[4], uint64_t sample_seed, float* actions_out_dev,
                       void* stream);

/* The MPPI update, per env:   w_b = exp2((G_b - G_max) * (log2(e) / lambda)),  G_max the largest finite return,
 *   nominal_out[t, e, c] = (sum_b w_b actions[t, r, c]) / (sum_b w_b),
 * both sums fp32 fma chains over b ascending, so the result does not depend on N, on the env's position
 * or on the launch shape.  A non-finite G_b gets weight 0; an env with no finite return gets branch 0's
 * rows.  lambda > 0.  nominal_out_dev [horizon, N, 4] may not overlap actions_dev. */
int32_t hg_mppi_update(hg_env* env, const float* actions_dev, const float* return_dev, int32_t horizon,
                       int32_t branches, float lambda, float* nominal_out_dev, void* stream);

/* What the planner thinks each env's state is worth: hg_mppi_update's weights applied to the returns
 * themselves.  return_dev [N, branches]; per env, with w_b and G_max exactly hg_mppi_update's (the same
 * exp2((G_b - G_max) * (log2(e) / lambda)), 0 for a non-finite G_b):
 *   value[e] = (sum_b w_b G_b) / (sum_b w_b),  num = fma(w_b, G_b, num) and den = den + w_b over b ascending:
 *              the chain hg_mppi_update runs on an action column (a non-finite G_b enters as 0 times 0);
 *   best[e]  = G_max                                       (best_dev [N] or NULL);
 *   ess[e]   = den^2 / sum_b w_b^2, sq = fma(w_b, w_b, sq)  (ess_dev [N] or NULL): the effective sample size.
 * An env with no finite return gets value 0, best -inf, ess 0.  With hg_rollout_branch_policy's
 * HG_BOOTSTRAP_VALUE returns, value is the planner's n-step lookahead value: hg_bc_grad's value_target_dev.
 * One wave per env; asynchronous, capturable, the env is not modified.
 * HG_E_INVALID, outputs untouched: branches outside hg_mppi_update's range; lambda not > 0 (or
 * log2(e) / lambda not finite in fp32); NULL return_dev or value_dev; a misaligned (4 bytes) pointer; NULL env. */
int32_t hg_mppi_value(hg_env* env, const float* return_dev, int32_t branches, float lambda, float* value_dev,
                      float* best_dev, float* ess_dev, void* stream);

/* ---- Policy-guided planning: the handle's policy inside the branches, its value head behind them.
 *
 * A candidate is *policy + residual*: closed-loop, so the policy meets each gust and the residual only has
 * to improve on it; and a row the horizon cuts is worth V of its last observation instead of nothing.
 * hg_mppi_sample and hg_mppi_update work unchanged on residual sequences.  Both calls below are
 * asynchronous on `stream`, allocate nothing, can be captured into a graph, and do not modify the env
 * (state, counters, azimuth records, chain bookkeeping, overlapped re-trim), like the three above.
 *
 * hg_policy_act_mean: actions[i] = clamp(mu(obs[i]) + residual[i]) and value[i] = V(obs[i]).
 *   mu is the policy's MEAN: the noise (log_std) is ignored even for a stochastic policy image, nothing is
 *   drawn, no counter is read.  mu is bitwise hg_policy_act's action for the same weights packed without
 *   log_std.  The sum is one fp32 add per component (no add at all when residual_dev is NULL); the clamp is
 *   hg_mppi_sample's fminf(fmaxf(x, lo[c]), hi[c]); lo and hi are host arrays of 4 passed by value into the
 *   kernel's arguments, both NULL for no clamp.  value_dev is bitwise hg_policy_eval's and needs a value
 *   head.  The same device function as hg_rollout_branch_policy's: acting with it and stepping (hg_step) in
 *   turn is bitwise that call's branch.
 *   HG_E_INVALID: exactly one of lo / hi NULL, a NaN bound or lo[c] > hi[c], obs_dev NULL, residual_dev or
 *   actions_dev not 16-byte aligned, no policy set, value_dev without a value head. */
int32_t hg_policy_act_mean(hg_env* env, const float* obs_dev, const float* residual_dev, const float lo[4],
                           const float hi[4], float* actions_dev, float* value_dev, void* stream);

/* hg_rollout_branch_policy: hg_rollout_branch with the actions computed inside the rows.  obs0_dev [N,17]:
 * the envs' current observations; residual_dev [horizon, N*branches, 4] (16-byte aligned) or NULL; outputs
 * as hg_rollout_branch's.  Row r = e * branches + b.
 *   Unchanged from hg_rollout_branch: the env's state and counters are read as its next hg_step would read
 *   them; never a reset inside a branch; HG_RESET_RETRIM handles are accepted; the rows of an env waiting
 *   for its next-step reset return (0, 0, 0); noise_mode, alive_steps and end_info.
 *   Observations: o_0 = obs0[e]; o_{t+1} is the observation step t produced.
 *   Action, while the row is alive at step t: a_t = clamp(mu(o_t) + residual[t, r]), exactly
 *     hg_policy_act_mean's (mean, one fp32 add, clamp; lo / hi both NULL: no clamp).
 *   Step and return: the step hg_rollout would take with a_t; G = fma(disc, reward_t, G), then
 *     disc = disc * gamma, from G = 0, disc = 1.
 *   bootstrap HG_BOOTSTRAP_VALUE: hg_rollout_ac's next_value rule applied to a branch.  A row that survives
 *     the horizon, or whose ending step is truncated and not terminated, gets one more term
 *     G = fma(disc, value_scale * V(o'), G): o' the observation its last step produced, disc the value after
 *     that step's multiply, value_scale * V one fp32 multiply.  A terminated row gets nothing.  A critic
 *     trained on hg_rollout_stats' scaled rewards scores in raw reward units with
 *     value_scale = 1 / reward_scale.
 *   One forward pass per step gives mu(o_t) and V(o_t); with the bootstrap one more pass follows the last
 *   step.  One wave per SIMD, the weights in registers across the steps; counted by hg_debug_launches as a
 *   lone-wave launch (out[4]), like hg_rollout_policy's.
 *   HG_E_INVALID, nothing touched: what hg_rollout_branch refuses; no policy set; bootstrap outside the
 *   enum; HG_BOOTSTRAP_VALUE without a value head; a non-finite value_scale; exactly one of lo / hi NULL,
 *   a NaN bound or lo[c] > hi[c]; obs0_dev or return_dev NULL; a misaligned pointer. */
enum { HG_BOOTSTRAP_NONE = 0, HG_BOOTSTRAP_VALUE = 1 };

int32_t hg_rollout_branch_policy(hg_env* env, const float* obs0_dev, const float* residual_dev, int32_t horizon,
                                 int32_t branches, float gamma, int32_t noise_mode, const float lo[4],
                                 const float hi[4], int32_t bootstrap, float value_scale, float* return_dev,
                                 int32_t* alive_steps_dev, uint8_t* end_info_dev, void* stream);

/* Batched device trim:HelicopterDynamics.trim (helicopter_dynamics.py:491-576) of the env's trim
 * condition against `count` winds at once — the reset path of reset_mode HG_RESET_RETRIM, exposed
 * for direct use.  Same Newton iteration as hg_trim (fp64, trial point rounded to fp32), with the
 * 32 Jacobian evaluations and the 10 line-search trials of each step evaluated in parallel lanes.
 *   wind_dev   [count,3] fp32 in (NED, ft/s)
 *   state_dev  [count,18] fp32 out or NULL, action_dev [count,4] fp32 out or NULL,
 *   obs_dev    [count,17] fp32 out or NULL, status_dev [count] i32 out or NULL
 *              (HG_OK, or HG_E_TRIM where the Newton iteration failed; outputs untouched there) */
int32_t hg_trim_batch(hg_env* env, const float* wind_dev, int64_t count, float* state_dev, float* action_dev,
                      float* obs_dev, int32_t* status_dev, void* stream);

/* Batched device trim for `count` trim conditions (host array `conds`, the reference's
 * set_trim_cond dicts, helicopter.py:101-106), against `wind_dev` [count,3] fp32 or, if NULL, the
 * mean wind: the first reset of `count` differently configured envs at once.  Outputs as
 * hg_trim_batch.  Synchronises with `stream` before returning. */
int32_t hg_trim_conds_batch(hg_env* env, const hg_trim_cond* conds, int64_t count, const float* wind_dev,
                            float* state_dev, float* action_dev, float* obs_dev, int32_t* status_dev,
                            void* stream);

/* Per-env reset targets (a batched set_trim_cond): templates_dev [N,39] fp32 = trimmed heli state
 * 18 | carry 4 (obs N/E/D velocity, ground altitude) | observation 17, one row per env, used by
 * hg_reset and by auto-reset instead of the shared template.  NULL reverts to the shared
 * template.  Copied; HG_RESET_TEMPLATE mode only. */
int32_t hg_set_reset_templates(hg_env* env, const float* templates_dev, void* stream);

/* ---- Per-env weather: turbulence level, mean wind direction and speed that differ across one handle's envs.
 *
 * The airframe document's ENV block (TURB_LVL, WIND_DIR, WIND_SPD) is the handle-wide weather.  A weather is
 * the same three numbers for one env; turb_level may be fractional (the TEP table is interpolated as for the
 * integer levels).  An env given a weather steps bitwise like an env of a handle whose airframe document has
 * that ENV block (same seed, global env id and reset template). */
typedef struct hg_weather {
    float turb_level;     /* 0 .. 7 */
    float wind_dir_deg;   /* the mean wind's direction, degrees */
    float wind_spd;       /* ft/s, >= 0 */
} hg_weather;

/* weather [N] (host), or NULL: back to the handle-wide weather and the shared reset template.
 * conds   [N] (host) trim conditions, or NULL: the handle's own for every env.
 * Builds each env's constants (hg_weather_constants), trims every env on the device against its own mean
 * wind (the code behind hg_trim_conds_batch) and installs the results as per-env reset templates (the code
 * behind hg_set_reset_templates); env states are not touched (hg_reset starts episodes from the templates).
 * status_dev [N] i32 or NULL receives each trim's status.  If any trim fails: HG_E_TRIM, and the handle is as
 * it was.  HG_E_INVALID: a NULL env; a non-finite value, turb_level outside [0, 7] or wind_spd < 0 (the
 * message names the first such env); reset_mode HG_RESET_RETRIM.
 * Synchronises with the device; not capturable.  The stepping calls that follow are capturable as before:
 * hg_step, hg_step_rows, hg_step_chained, hg_rollout, hg_rollout_policy, hg_rollout_ac and hg_rollout_pop
 * honour the weather at every N (through kernels of their own: the lone-wave and the bulk step; no
 * helper-wave, non-temporal bulk or run-time specialised variant, which are bitwise equal anyway).
 * hg_rollout_branch and hg_rollout_branch_policy return HG_E_INVALID ("... per-env weather") while it is set; so do
 * hg_set_trim_cond and hg_set_reset_templates (pass `conds` here instead).  hg_set_target, hg_set_max_time,
 * hg_reset, hg_get_state and hg_set_state work as before. */
int32_t hg_set_weather(hg_env* env, const hg_weather* weather, const hg_trim_cond* conds, int32_t* status_dev,
                       void* stream);

/* out_host [N] or NULL: each env's weather (the handle-wide one while none is set).  templates_dev [N,39]
 * or NULL: the reset templates in use, hg_set_reset_templates' layout (the shared one in every row while no
 * per-env templates are set).  Synchronises with `stream`. */
int32_t hg_get_weather(hg_env* env, hg_weather* out_host, float* templates_dev, void* stream);

/* Host only, no device: what hg_set_weather uploads for one env, formed by the code that forms the
 * handle-wide constants from the ENV block.  record = {wm north, wm east, cos dir, sin dir, sigma_low,
 * turb_level, 0, 0}; tep_row = the TEP table's row at turb_level (13 values) and 3 zeros.  `cfg` is
 * validated for NULL only (no constant of a weather depends on the rest of the configuration today). */
int32_t hg_weather_constants(const hg_config* cfg, const hg_weather* w, float record[8], float tep_row[16]);

/* ---- Per-env goals: task targets that differ across one handle's envs, optionally redrawn at every reset.
 *
 * hg_config::target (hg_set_target) is one target for the whole handle.  A goal table gives each env its own;
 * an env given a goal steps bitwise like an env of a handle whose target is that goal (same seed, global env
 * id and reset template).  HG_TASK_HOVER uses north_loc, east_loc and sea_alt; HG_TASK_FORWARD_FLIGHT uses
 * sea_alt and vel; the other fields of a goal are not looked at.  HG_TASK_HELI has no target: HG_E_INVALID.
 *
 * Two modes.  TABLE: `goals_host` [N], kept until changed.  BOX: a closed range per field; env i's goal in
 * episode e is hg_goal_draw(cfg, box, env_offset + i, e) -- a pure function of the handle's seed, the env's
 * global id, the episode counter (the one the turbulence noise is keyed by) and the box, so it does not depend
 * on the batch or on how the envs are sharded.  The kernel that resets an env draws the new episode's goal and
 * stores it into the table (no host work: the stepping calls stay capturable); hg_reset and hg_set_state with
 * counters redraw it, so the table always holds draw(seed, gid_i, episode_i).
 *
 * obs_mode HG_GOAL_OBS_RELATIVE: every observation row the stepping calls produce has the goal's fp32 value
 * subtracted, in fp32, from columns 13, 14, 15 (N_POS, E_POS, ALTITUDE; hover) or from column 15 and column 1
 * (LON_AIR_SPD minus the target speed; forward flight) -- obs, final_obs, final_obs_rows, the in-kernel policy's
 * input and the terminal forward pass of next_value, each in the frame of the goal of the episode the row
 * belongs to (a terminal observation the ending episode's, the reset observation the new one's), and the
 * rows hg_reset writes.  Rewards, flags and the state are those of absolute observations.
 *
 * Both NULL: back to the handle-wide target.  Synchronises with the device; not capturable.
 * HG_E_INVALID with a message that names the cause: both goals_host and box given; a non-finite value; lo > hi;
 * vel <= 0 for forward flight; an obs_mode outside the enum; HG_TASK_HELI; reset_mode HG_RESET_RETRIM (the trim
 * kernel writes the observation rows); a handle with per-env weather or a fleet (hg_set_weather and
 * hg_set_fleet refuse a goal handle too).  While goals are set: hg_set_target returns HG_E_INVALID ("pass goals
 * to hg_set_goals"), and so do hg_rollout_pop, hg_rollout_branch and hg_rollout_branch_policy.  hg_step,
 * hg_step_rows, hg_step_chained, hg_rollout, hg_rollout_policy and hg_rollout_ac honour the goals at every N
 * through kernels of their own (the lone-wave and the bulk step with the optional features; no helper-wave,
 * non-temporal bulk or run-time specialised variant), counted by hg_debug_launches in the lone-wave or bulk
 * bucket.  hg_set_max_time, hg_reset, hg_get_state, hg_set_state and per-env reset templates work as before. */
typedef struct hg_goal_box {
    hg_target lo, hi;
} hg_goal_box;
enum { HG_GOAL_OBS_ABSOLUTE = 0, HG_GOAL_OBS_RELATIVE = 1 };
enum { HG_GOALS_OFF = 0, HG_GOALS_TABLE = 1, HG_GOALS_BOX = 2 };
int32_t hg_set_goals(hg_env* env, const hg_target* goals_host /* [N] or NULL */, const hg_goal_box* box /* or NULL */,
                     int32_t obs_mode, void* stream);
/* Any output may be NULL.  goals_host [N]: each env's goal now (the handle-wide target while none is set; in box
 * mode the fp32 values the table holds; heading is the handle's).  box: the box (zeros unless mode is BOX).
 * Synchronises with `stream`. */
int32_t hg_get_goals(hg_env* env, hg_target* goals_host, hg_goal_box* box, int32_t* mode, int32_t* obs_mode,
                     void* stream);
/* Host only: the record hg_set_goals uploads for a target, rec = {north / n_x, east / n_x, -sea_alt / n_x,
 * vel / n_v, north, east, sea_alt, vel}: rec[0..2] bitwise the tgt_n, rec[3] the vel_tgt_n and rec[2] the
 * dwn_tgt_n of a handle configured with that target (hg_debug_params). */
int32_t hg_goal_record(const hg_config* cfg, const hg_target* target, float rec[8]);
/* Host only: the device's draw for global env id `global_env` in episode `episode` of a handle configured as
 * `cfg` (its seed, task, airframe and target, which fills the fields the task does not use).  out (or NULL):
 * the goal; rec (or NULL): its record. */
int32_t hg_goal_draw(const hg_config* cfg, const hg_goal_box* box, int64_t global_env, int32_t episode,
                     hg_target* out, float rec[8]);
/* Diagnostic, host only, fp64: the task layer (reward and success_step of cfg's task, the functions the step
 * kernels instantiate in fp32) on n rows of post-step heli state [n,18] and k4 derivatives [n,18].  goals NULL:
 * under cfg's own target (the constants of a handle configured as cfg).  goals [n]: row i under goals[i] through
 * the per-env goal forms, fed the fp32 record hg_goal_record gives for it, as the goal kernels are.
 * reward [n], success [n] (0 / 1).  HG_TASK_HELI is refused. */
int32_t hg_debug_task_host(const hg_config* cfg, const double* heli, const double* dots, const hg_target* goals,
                           int64_t n, double* reward, uint8_t* success);
/* Diagnostic, host only, fp64: Heli._is_failed (the function the step kernels instantiate in fp32) on n rows of
 * post-step heli state [n,18] and k4 derivatives [n,18], with the ground height of `terrain_ft` [rows, cols] under
 * each row's position and the constants of a handle configured as cfg.  failed [n] (0 / 1), clauses [n]
 * (HG_FAIL_* bits). */
int32_t hg_debug_failed_host(const hg_config* cfg, const double* terrain_ft, int32_t rows, int32_t cols,
                             const double* heli, const double* dots, int64_t n, uint8_t* failed, uint8_t* clauses);

/* ---- Mixed fleets: airframes that differ across one handle's envs, one airframe class per 64-env state tile.
 *
 * A handle steps every env with one airframe's constants.  A fleet gives each state tile (envs 64 t .. 64 t + 63,
 * one wave of the step kernels) a class of its own: the kernels read the tile's class with one scalar load and
 * take that class's constant image where they took the handle's, so the constants stay scalar loads and the
 * step's code is the generic step's.  An env of a class steps bitwise like an env of a handle created with that
 * airframe (same seed, global env id, trim condition).
 *
 * classes [n_classes] (host): raw airframe + ENV block of each class.  conds [n_classes] (host) or NULL: the
 * handle's own trim condition for every class.  tile_class [ceil(N/64)] (host): the class of each 64-env
 * state tile (envs 64 t .. 64 t + 63).  status_host [n_classes] or NULL: each class's trim status.
 * classes == NULL: back to the handle's own airframe and the shared reset template.
 *
 * Derives each class's constants as hg_create does for a config with that airframe (hg_fleet_constants; dt,
 * task, target, limits and reset flags are the handle's), trims each class on the host against its own mean
 * wind (the code behind hg_trim) and installs every env's class trim as its reset template (the code behind
 * hg_set_reset_templates); env states are not touched.  A trim that fails, does not converge to the
 * reference's threshold or is not finite: HG_E_TRIM, status_host names the classes, the handle is as it was.
 * HG_E_INVALID, outputs untouched: a NULL env; n_classes < 1 or > the number of tiles; a tile_class entry
 * outside [0, n_classes); a non-finite airframe field; a class whose env_MAX_GR_ALT, env_NS_MAX or env_EW_MAX
 * differs from the handle's (the terrain is shared); reset_mode HG_RESET_RETRIM (the device trim reads one
 * airframe); a handle with per-env weather set.  A fleet together with per-env weather is out of scope:
 * hg_set_weather on a fleet handle returns HG_E_INVALID too.
 * Synchronises with the device; not capturable.  The stepping calls that follow are capturable as before.
 * Measured at 65 536 hover envs: hg_step 9.10 us with 1 class, 9.03 with 3, 9.10 with 1 024 (one per tile),
 * against 7.57 for the generic kernel without per-env reset templates; this call 0.055 s for 1 024 classes.
 * While a fleet is set: hg_step, hg_step_rows, hg_step_chained, hg_rollout, hg_rollout_policy, hg_rollout_ac,
 * hg_rollout_pop, hg_rollout_branch and hg_rollout_branch_policy step each env with its tile's constants
 * (kernels of their own: the generic lone-wave and bulk step; never the constant-specialised, run-time
 * specialised or helper-wave variants), counted by hg_debug_launches in the lone-wave or bulk bucket by the
 * usual size rule.  The branched rollouts need `branches` to divide 64 or be a multiple of 64 (a wave's 64
 * rows then belong to one tile), else HG_E_INVALID.  hg_get_state, hg_set_state and hg_reset use each env's
 * class's rotor speeds for the azimuths.  hg_set_target and hg_set_max_time update every class.
 * hg_set_trim_cond and hg_set_reset_templates return HG_E_INVALID (pass `conds` here).  hg_trim_batch and
 * hg_trim_conds_batch keep trimming the handle's own airframe. */
int32_t hg_set_fleet(hg_env* env, const hg_airframe* classes, const hg_trim_cond* conds, int32_t n_classes,
                     const int32_t* tile_class, int32_t* status_host, void* stream);
/* Any output may be NULL (not all).  Without a fleet: one class, the handle's own airframe, every tile 0.
 * templates_dev [N,39]: the reset templates in use, as hg_get_weather returns them.  Synchronises. */
int32_t hg_get_fleet(hg_env* env, int32_t* n_classes, int32_t* tile_class_host /* [tiles] or NULL */,
                     hg_airframe* classes_host /* [n_classes] or NULL */, float* templates_dev /* [N,39] or NULL */);
/* host only: the Params<float> image of class `af` on a handle configured as `cfg` (its dt, task, target,
 * limits, reset flags) -- bitwise hg_debug_params of `cfg` with cfg.af replaced by `af`, baked_only = 0 */
int32_t hg_fleet_constants(const hg_config* cfg, const hg_airframe* af, int32_t rows, int32_t cols,
                           void* out, int64_t bytes);

/* Run-time specialisation for airframes other than the compiled-in default one (whose constants
 * are instruction literals of the library's step kernel): load a gfx950 code object built from
 * csrc/step_rtc.hip with this env's constant image (`image`, the sizeof(Params<float>) bytes
 * hg_debug_params returns with baked_only = 1) for `task`.  Per-step launches (no injected noise,
 * not hg_rollout) of an env whose constants match the image then run its kernels; results are
 * bitwise those of the generic kernel.  Returns 1 when in use, 0 when loaded but not matching,
 * < 0 on error.  Not part of the reference surface (replaces nothing: the reference has one
 * NumPy code path for every airframe). */
int32_t hg_load_specialized(hg_env* env, const char* code_object_path, int32_t task, const void* image,
                            int64_t bytes);

/* Number of RETRIM-mode auto-resets so far whose trim failed (those envs got the template state).
 * Synchronises with the device. */
int32_t hg_retrim_failures(hg_env* env, int64_t* count);

/* Diagnostic: re-trim job records that named no env (or a job count past N), skipped by the trim
 * instead of indexing the state with them; 0 in a correct run.  Synchronises with the device. */
int32_t hg_debug_retrim_invalid(hg_env* env, int64_t* count);

/* Diagnostic: the device trim's Newton solves since creation (every re-trim, hg_trim_batch and
 * hg_trim_conds_batch of this env): counts[0] solved with the pivot order of the host's trim of the
 * env's condition (gj_mfma.h gjs_solve), counts[1] of them rejected by the residual test and
 * re-solved with the pivot search.  Synchronous (reads device counters). */
int32_t hg_debug_retrim_solves(hg_env* env, int64_t* counts);

/* Diagnostic: the re-trim job-count rings (out[0..2] the step re-trim ring, out[3..5] the overlapped
 * re-trim ring or -7, out[6..8] hg_reset's job count, failures, invalid jobs).  Synchronises. */
int32_t hg_debug_queues(hg_env* env, int32_t* out);

/* Diagnostic: host-side launch counts of this handle since creation: out[0] step calls (hg_step,
 * hg_step_chained, hg_step_rows), out[1] steps whose launch held the previous step's re-trims
 * (hg_set_retrim_overlap), out[2] run-time specialised kernel launches, out[3] small-batch helper
 * kernel launches, out[4] lone-wave (one or two waves per SIMD) launches, out[5] bulk launches
 * (out[3..5] count hg_rollout's too, out[4..5] hg_rollout_branch's, out[4] hg_rollout_branch_policy's).
 * Host only. */
int32_t hg_debug_launches(const hg_env* env, int64_t* out);

/* HG_RESET_RETRIM with next-step auto-reset (gymnasium's default, make_vec's): the episodes a step ends
 * are re-trimmed (helicopter.py:208-212 -> helicopter_dynamics.py:491-555) while the next step runs,
 * in the same kernel launch as that step (its first blocks), so the caller's stream sees every step
 * complete and the results are bitwise the serial path's.  A step holds the trims of the previous
 * step's ends only when that step was the previous launch of the same sequence (eager, or captured
 * into the same graph) with no other state-changing call on the handle in between, with in-kernel
 * noise and at most two step waves per SIMD (N <= 131 072 on MI355X); otherwise its due resets are
 * trimmed after it, serially.  enable = 1 (the default) or 0 (always serial: A/B and tests); 2 also
 * fuses, with same-step auto-reset, a step's re-trims into its own launch: trim blocks first, each
 * taking a reset as soon as its env's step wave has published it (in-kernel noise, at most two step
 * waves per SIMD).  Bitwise the serial path, but slower on MI355X (65 536 envs: 33.7 against 29.4 us
 * per step; the step waves run about 7 us longer beside the trims), so opt-in.  Returns 1 if the
 * next-step mode is configured and enabled, 0 otherwise, or HG_E_*. */
int32_t hg_set_retrim_overlap(hg_env* env, int32_t enable);

/* State access for parity tests / checkpointing (the reference's StateNumpy,
 * dynamics.py:75-128, exposed as one record per env): state [N,HG_STATE_COLS] fp32,
 * counters [N,HG_COUNTER_COLS] i32 (either may be NULL).  The rotor azimuths (state columns 2, 3)
 * are not part of the stepped state: hg_get_state reconstructs them (each step adds dt * Omega and
 * wraps, bitwise what the step would have carried), at a cost linear in the steps since the env's
 * last reset / set_state / hg_get_state (each read re-anchors the env's azimuth record at the values
 * it returns, so periodic reads keep every read short).  A negative episode-step counter marks an env whose next-step auto-reset
 * is due (read back as -1). */
int32_t hg_get_state(hg_env* env, float* state_dev, int32_t* counters_dev, void* stream);
int32_t hg_set_state(hg_env* env, const float* state_dev, const int32_t* counters_dev, void* stream);

/* Synthetic policy for benchmarks: actions [N,4] ~ U(lo, hi) from Philox4x32-10 keyed by
 * (seed, env_offset+i, step).  Not part of the reference surface. */
int32_t hg_random_actions(hg_env* env, float* actions_dev, uint64_t seed, uint64_t step,
                          float lo, float hi, void* stream);

/* Diagnostic (parity tests): the turbulence noise eta [N,3] fp32 (already scaled by 1/sqrt(dt)) that
 * each env's next hg_step with eta_dev == NULL draws in-kernel — WindDynamics.step_before
 * (wind_dynamics.py:49-52) restated as Philox4x32-10 keyed by (seed, env_offset+i, episode step,
 * episode index) and Box-Muller, computed by the same device function from the env's current
 * counters.  A step given these values as eta_dev is bitwise the in-kernel step. */
int32_t hg_debug_eta(hg_env* env, float* eta_dev, void* stream);

/* Diagnostic (parity tests): the task layer alone, fp32, on n rows of post-step heli state heli_dev [n,18] and k4
 * derivatives dots_dev [n,18]: the reward functions the step kernels call, with the handle's device constants
 * (its target, after hg_set_target).  While per-env goals are set, row i is evaluated under the record of env
 * i % N through the goal forms.  reward_dev [n] fp32, success_dev [n] u8 (success_step).  n is any count >= 0;
 * it changes no state of the handle.  HG_TASK_HELI is refused. */
int32_t hg_debug_task(hg_env* env, const float* heli_dev, const float* dots_dev, float* reward_dev,
                      uint8_t* success_dev, int64_t n, void* stream);

/* Diagnostic (parity tests): the failure test alone, fp32, on n rows of post-step heli state heli_dev [n,18] and k4
 * derivatives dots_dev [n,18]: the function the step kernels call, with the handle's device constants and terrain
 * texels; under a fleet, row i with the constants of the class of env i % N.  failed_dev [n] u8 (0 / 1),
 * clauses_dev [n] u8 (HG_FAIL_* bits).  n is any count >= 0; it changes no state of the handle. */
int32_t hg_debug_failed(hg_env* env, const float* heli_dev, const float* dots_dev, uint8_t* failed_dev,
                        uint8_t* clauses_dev, int64_t n, void* stream);

/* Diagnostic (known-answer tests): the device Philox4x32-10 on `count` rows of in_dev
 * {ctr0, ctr1, ctr2, ctr3, key0, key1} (u32) -> out_dev [count,4] u32.  It has no handle: it runs on
 * the calling thread's current HIP device, and both buffers must be device memory of that device
 * holding at least 6*count and 4*count words. */
int32_t hg_debug_philox(const uint32_t* in_dev, uint32_t* out_dev, int64_t count, void* stream);

/* Benchmark clock: one single-lane kernel on `stream` that writes the GPU's constant 100 MHz clock
 * (s_memrealtime) to dst_dev[0] when it runs.  Two stamps around K steps launched (or captured) on
 * the same stream time exactly those K kernels, each with its dependent-launch gap, plus the gap
 * after the first stamp.  Not part of the reference surface. */
int32_t hg_clock_stamp(uint64_t* dst_dev, void* stream);

/* ---- Populations of policies and an evolution-strategies learner on the device.
 *
 * A handle holds one policy image; the calls below run MANY policies over the envs of one handle in one
 * launch and build the gradient-free learner (OpenAI-ES: antithetic pairs, centred ranks) around that
 * rollout.  Every device call is asynchronous on `stream`, allocates nothing, makes no host decision that
 * depends on device data and can be captured into a graph; none uses a floating-point atomic, and every launch
 * shape is a function of the arguments and compile-time constants, so two calls on equal inputs give equal
 * bits.  HG_E_INVALID means nothing was enqueued and no output was touched; the arguments that do not need
 * the handle are checked before it, so they are refused with a NULL env too.
 *
 * theta is hg_ppo_grad's flat layout [HG_PPO_N_PARAMS].  An IMAGE is a packed policy as the rollout kernels
 * load it (csrc/policy_mlp.h): hg_policy_image_floats() = 7552 floats.  A population's images are
 * caller-owned device memory [P, 7552], 16-byte aligned. */
int64_t hg_policy_image_floats(void);           /* 7552; host only */

/* Image p (p = 0 .. P-1) = bitwise what hg_set_policy_theta(theta_dev + 5641 p, obs_mean_dev, obs_scale_dev)
 * leaves in a handle's own buffer, the value head's elements included; with stochastic == 0 the head words
 * (exp(log_std), the stochastic flag, the log_std sum) are those of hg_set_policy with log_std == NULL: zero.
 * obs_mean_dev / obs_scale_dev [17] or NULL (0 / 1), shared by all members.  One launch for all P images.
 * The env is used for its device and the error convention only.
 * HG_E_INVALID: NULL env, theta_dev or images_dev; images_dev not 16-byte aligned, another pointer not
 * 4-byte aligned; P outside 1 .. 65536. */
int32_t hg_pop_pack(hg_env* env, const float* theta_dev, int64_t P, int32_t stochastic, const float* obs_mean_dev,
                    const float* obs_scale_dev, float* images_dev, void* stream);

/* hg_rollout_policy (eta_dev == NULL: in-kernel noise; injected noise is not offered) in which the wave of
 * state tile t -- envs 64 t .. 64 t + 63 -- evaluates image (64 t) / envs_per_member of images_dev [P, 7552]:
 * member p owns envs p * envs_per_member .. min(N, (p + 1) * envs_per_member) - 1.  Outputs, their stacking,
 * restrictions (no auto-resets in HG_RESET_RETRIM), the action noise's key (an env's noise depends on its own
 * counters, not on its member) and hg_debug_launches accounting (a lone-wave launch) are hg_rollout_policy's;
 * member p's rows are bitwise hg_rollout_policy's of a handle of that member's envs with env_offset
 * advanced by p * envs_per_member, the same seed and image p as its policy.  The handle's own policy is
 * neither read nor required nor modified.
 * HG_E_INVALID: what hg_rollout_policy refuses (its "no policy set" excepted); NULL or misaligned (16 bytes)
 * images_dev; P outside 1 .. 65536; envs_per_member not a positive multiple of 64; N outside
 * ((P - 1) * envs_per_member, P * envs_per_member] (every member owns at least one env; the last may be
 * short or ragged). */
int32_t hg_rollout_pop(hg_env* env, const float* images_dev, int64_t P, int64_t envs_per_member, const float* obs0_dev,
                       int32_t nsteps, float* actions_out_dev, float* obs_dev, float* reward_dev,
                       uint8_t* terminated_dev, uint8_t* truncated_dev, uint8_t* info_dev, void* stream);

/* ES members from counters.  The noise of pair j (members 2 j and 2 j + 1), parameter i < 5572 (the
 * actor-mean parameters W1 .. b3; log_std, w_v, b_v are not perturbed), generation
 *   g = gen + (gen_dev ? *gen_dev : 0), a 64-bit sum; gen_dev [1] i32 is read when the kernel runs, so a
 *       replayed graph whose gen_dev points at a counter (the optimiser state's `applied` or `seen` word)
 *       draws fresh noise every replay:
 *   eps_j[i] = normal (i & 3) of the four Box-Muller normals (z0 .. z3 of hg_set_policy's noise paragraph,
 *              the same u(r), f(r), R0, R1) of ONE Philox4x32-10 call on
 *   counter = (i >> 2, j, g_lo, g_hi),   key = (seed_lo ^ 0x65735F6E, seed_hi ^ 0x6F697365).
 * The noise is never stored: hg_es_perturb and hg_es_grad both regenerate it.
 *
 * hg_es_perturb: theta_{2j} = fma(sigma, eps_j, theta), theta_{2j+1} = fma(-sigma, eps_j, theta) element-wise in
 * fp32 for i < 5572, theta's own bits for i >= 5572; images_dev [P, 7552] image p = bitwise hg_pop_pack of
 * theta_p (stochastic, obs_mean_dev, obs_scale_dev as there); member_theta_dev [P, 5641] or NULL receives the
 * theta_p themselves (how a caller keeps the best member).  One launch; the noise goes from registers into
 * the packed layout, and no [P, 5641] intermediate exists when member_theta_dev is NULL.
 * HG_E_INVALID: NULL env, theta_dev or images_dev; images_dev not 16-byte aligned, another pointer not 4-byte;
 * P odd or outside 2 .. 65536; sigma not finite or <= 0. */
int32_t hg_es_perturb(hg_env* env, const float* theta_dev, int64_t P, float sigma, uint64_t seed, int64_t gen,
                      const int32_t* gen_dev, int32_t stochastic, const float* obs_mean_dev, const float* obs_scale_dev,
                      float* images_dev, float* member_theta_dev, void* stream);

/* Diagnostic, the counterpart of hg_debug_eta: out_dev [5572] = eps_pair as the two calls around it compute
 * it (the same device function).  HG_E_INVALID: NULL env or out_dev; a misaligned (4 bytes) pointer; pair
 * outside 0 .. 32767. */
int32_t hg_es_noise(hg_env* env, uint64_t seed, int64_t gen, const int32_t* gen_dev, int64_t pair, float* out_dev,
                    void* stream);

/* Per-member fitness from what hg_rollout_pop wrote, accumulated across calls (long episodes are collected
 * in chunks of K steps).  reward_dev [K, N] fp32, terminated_dev / truncated_dev [K, N] u8 (N the env's),
 * members as in hg_rollout_pop.
 *   HG_POP_FIT_WINDOW:        every reward counts (the flags are not read and may be NULL).
 *   HG_POP_FIT_FIRST_EPISODE: an env's rewards count up to and including its first step with
 *                             terminated | truncated since the last restart; alive_dev [N] u8 (required)
 *                             carries that across calls: 1 while the env still counts.
 *   restart != 0: sum = 0 and alive = 1 are taken before this call's rewards, inside the same launch.
 * Per env: e_n = an fp64 sum of its counted rewards over k ascending, from 0 (rewards are selected, not
 * multiplied by a flag: nothing of a finished env's later rows enters).  Per member, with c = its env count
 * (envs_per_member, less for the last): thread t (0 .. 255) adds e_n of its envs base + t, base + t + 256, ..
 * in ascending order from 0; the 256 thread sums are added by the halving tree s[t] += s[t + w], w = 128, 64,
 * .. 1 -- an order that depends on envs_per_member and c only.  Then sum_dev[p] += that (fp64) and
 * fitness_out_dev[p] = (float)(sum_dev[p] / c): the mean counted reward sum per env of member p so far.
 * (Every addition is fp64 on fp32 rewards: chunked calls and one call over the concatenation agree bitwise
 * whenever no addition rounds -- e.g. a member's counted rewards spanning under 2^16 in magnitude and fewer
 * than 2^13 of them -- and to fp64 rounding otherwise.)  A non-finite reward makes that member's sum and fitness non-finite and
 * touches no other member.
 * HG_E_INVALID: NULL env, reward_dev, sum_dev or fitness_out_dev; a mode outside the enum; FIRST_EPISODE
 * without terminated_dev, truncated_dev or alive_dev; sum_dev not 8-byte or an fp32 pointer not 4-byte
 * aligned; K < 1; P, envs_per_member, N as hg_rollout_pop refuses them. */
enum { HG_POP_FIT_WINDOW = 0, HG_POP_FIT_FIRST_EPISODE = 1 };

int32_t hg_pop_fitness(hg_env* env, const float* reward_dev, const uint8_t* terminated_dev, const uint8_t* truncated_dev,
                       int32_t K, int64_t P, int64_t envs_per_member, int32_t mode, int32_t restart, uint8_t* alive_dev,
                       double* sum_dev, float* fitness_out_dev, void* stream);

/* The ES gradient estimate from P fitnesses, fitness_dev [P] fp32 (member order: pair j = members 2 j, 2 j + 1).
 *   rank     r_p = #{q : f_q < f_p} + #{q < p : f_q == f_p}, where every non-finite f (NaN included) counts as
 *            -inf (so they rank lowest, ties by index): r is always a permutation of 0 .. P-1.
 *   utility  u_p = fl(r_p / (P - 1)) - 1/2 in fp32: one correctly rounded fp32 division, one subtraction.
 *   grad[i]  = s * sum_j (u_{2j} - u_{2j+1}) eps_j[i] for i < 5572, exactly 0 for 5572 <= i < 5641, with
 *            s = (float)(-1 / ((double)P * (double)sigma)) and eps regenerated from hg_es_perturb's counters
 *            (seed, gen, gen_dev as there).  The minus sign makes hg_ppo_adam's descent ascend the fitness.
 *   order    w_j = u_{2j} - u_{2j+1} (one fp32 subtraction); pairs in chunks of 16 consecutive ones; per chunk
 *            acc = fma(w_j, eps_j[i], acc) over its pairs ascending, from 0; the chunks' sums added ascending,
 *            from 0; one multiplication by s.  A function of P and compile-time constants only.
 *   stats_dev [8] or NULL: [0] mean (an fp64 sum, rounded once), [1] min, [2] max of the finite fitnesses
 *            (NaN when there is none)  [3] the number of non-finite ones  [4] the index of the best finite
 *            member, the lowest index among ties (-1 when there is none)  [5] ||grad||_2 (fp32, hg_ppo_adam's
 *            summation order)  [6], [7] zero.
 * P is even, 2 .. 16384 (the ranks are P^2 comparisons); hg_es_workspace_bytes(P) bytes at workspace_dev,
 * 16-byte aligned, contents irrelevant before and after (the utilities, then one partial gradient per
 * chunk).  Three launches, a fourth with stats_dev.  grad_dev feeds hg_ppo_adam(theta, grad, NULL, state, cfg) unchanged: its
 * non-finite guard, norm clip, Adam and lr_dev apply.  Z-score shaping and weight decay are not offered.
 * HG_E_INVALID: NULL env, fitness_dev, grad_dev or workspace_dev; workspace_dev not 16-byte, another pointer
 * not 4-byte aligned; P odd or outside 2 .. 16384; sigma not finite or <= 0.  hg_es_workspace_bytes returns
 * HG_E_INVALID for such a P. */
int64_t hg_es_workspace_bytes(int64_t P);       /* a multiple of 16; host only */

int32_t hg_es_grad(hg_env* env, const float* fitness_dev, int64_t P, float sigma, uint64_t seed, int64_t gen,
                   const int32_t* gen_dev, float* grad_dev, float* stats_dev, void* workspace_dev, void* stream);

/* Diagnostics (tests): copy the handle's own packed policy image to image_out_dev [7552], or replace it with
 * image_dev [7552] (any image of a population; the handle then counts as having a policy and a value
 * head).  Device-to-device copies on `stream`. */
int32_t hg_debug_get_policy_image(hg_env* env, float* image_out_dev, void* stream);
int32_t hg_debug_set_policy_image(hg_env* env, const float* image_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HELIGYM_AMD_H */
