"""Running observation / return normalisation and episode statistics of rollouts (hg_rollout_stats).

`RolloutStats` owns the device state and the output tensors `HeliVecEnv.rollout_stats` fills;
`rollout_stats_ref` is the same function in NumPy float64: the checker of the kernels and the statement of
what they compute (include/heligym_amd.h has it in words).
"""
import ctypes

import numpy as np

from . import _abi

N_OBS = _abi.HG_N_OBS
# the fp64 head of the state, name -> index in doubles (include/heligym_amd.h's table)
STATS_HEAD = {"obs_count": 0, "obs_mean": 1, "obs_M2": 18, "ret_count": 35, "ret_mean": 36, "ret_M2": 37,
              "episodes": 38, "env_steps": 39, "skipped_rows": 40, "skipped_returns": 41}
STATS_HEAD_DOUBLES = 48
STATS_HEAD_BYTES = 8 * STATS_HEAD_DOUBLES
STATS_WORKSPACE_BYTES = 180240
# episode_out's words
EPISODE_FIELDS = ("episodes", "return_mean", "return_std", "return_min", "return_max", "length_mean", "terminated",
                  "truncated", "success", "reward_mean", "skipped_rows", "skipped_returns", "nonfinite_returns")


def stats_state_bytes(n_envs):
    """hg_rollout_stats_state_bytes: head | G, ep_ret, ep_len [n] | padding to 16 bytes | workspace."""
    n = int(n_envs)
    return STATS_HEAD_BYTES + (12 * n + 15) // 16 * 16 + STATS_WORKSPACE_BYTES


class RolloutStats:
    """The persistent state of hg_rollout_stats for `env` (a HeliVecEnv) and the tensors its outputs go to:
    `state` (int32 words, hg_rollout_stats_state_bytes(N) bytes) with the views `head` (float64 [48]), `G`,
    `ep_ret` (float32 [N]) and `ep_len` (int32 [N]); `obs_mean`, `obs_scale` (float32 [17]: what
    set_policy_theta, ppo_grad and ppo_update take), `reward_scale` [1] and `episode` [16] (EPISODE_FIELDS)."""

    def __init__(self, env):
        t = env.torch
        n, dev = int(env.num_envs), env.device
        self.env = env
        self.state = t.zeros((stats_state_bytes(n) // 4,), dtype=t.int32, device=dev)
        w = STATS_HEAD_BYTES // 4
        self.head = self.state[:w].view(t.float64)
        self.G = self.state[w:w + n].view(t.float32)
        self.ep_ret = self.state[w + n:w + 2 * n].view(t.float32)
        self.ep_len = self.state[w + 2 * n:w + 3 * n]
        self.obs_mean = t.zeros((N_OBS,), dtype=t.float32, device=dev)
        self.obs_scale = t.ones((N_OBS,), dtype=t.float32, device=dev)
        self.reward_scale = t.ones((1,), dtype=t.float32, device=dev)
        self.episode = t.zeros((16,), dtype=t.float32, device=dev)

    def zero_(self):
        """Forget everything: the state zeroed by hg_rollout_stats_init (a kernel on the current stream,
        capturable), the outputs back to mean 0 / scale 1."""
        if self.state.is_cuda:
            env = self.env
            env._check(env.lib.hg_rollout_stats_init(env._h, ctypes.c_void_p(self.state.data_ptr()), env._stream()))
        else:
            self.state.fill_(0)
        self.obs_mean.fill_(0.0)
        self.obs_scale.fill_(1.0)
        self.reward_scale.fill_(1.0)
        self.episode.fill_(0.0)
        return self

    def moments(self):
        """The head as a dict (one device-to-host copy, which synchronises): obs_count, obs_mean [17], obs_var
        [17] (population), ret_count, ret_mean, ret_var, and the lifetime totals episodes, env_steps,
        skipped_rows, skipped_returns."""
        h = self.head.cpu().numpy()
        L = STATS_HEAD
        nc, rc = h[L["obs_count"]], h[L["ret_count"]]
        return dict(obs_count=int(nc), obs_mean=h[L["obs_mean"]:L["obs_mean"] + N_OBS].copy(),
                    obs_var=h[L["obs_M2"]:L["obs_M2"] + N_OBS] / max(nc, 1.0),
                    ret_count=int(rc), ret_mean=float(h[L["ret_mean"]]), ret_var=float(h[L["ret_M2"]] / max(rc, 1.0)),
                    episodes=int(h[L["episodes"]]), env_steps=int(h[L["env_steps"]]),
                    skipped_rows=int(h[L["skipped_rows"]]), skipped_returns=int(h[L["skipped_returns"]]))

    def episode_dict(self):
        """`episode` as {EPISODE_FIELDS: float} (one device-to-host copy, which synchronises)."""
        return dict(zip(EPISODE_FIELDS, (float(x) for x in self.episode.cpu().numpy())))


def _np(x, dtype):
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def _chan(n_a, mean_a, m2_a, x):
    """Chan's update of (count, mean, M2) by the float64 samples x [m, ...] (two passes over the batch)."""
    m = x.shape[0]
    if m == 0:
        return n_a, mean_a, m2_a
    c = x[0]
    mean_b = c + (x - c).mean(axis=0)
    m2_b = ((x - mean_b) ** 2).sum(axis=0)
    if n_a == 0:
        return float(m), mean_b, m2_b
    n = n_a + m
    delta = mean_b - mean_a
    return float(n), mean_a + delta * (m / n), m2_a + m2_b + delta * delta * (n_a * m / n)


def rollout_stats_fresh(n_envs):
    """The reference's state after hg_rollout_stats_init."""
    return dict(obs_count=0.0, obs_mean=np.zeros(N_OBS), obs_M2=np.zeros(N_OBS), ret_count=0.0, ret_mean=0.0, ret_M2=0.0,
                episodes=0, env_steps=0, skipped_rows=0, skipped_returns=0,
                G=np.zeros(n_envs, np.float32), ep_ret=np.zeros(n_envs, np.float32), ep_len=np.zeros(n_envs, np.int32))


def rollout_stats_ref(state, obs, reward, terminated, truncated, info=None, obs0=None, gamma=0.99, update_obs=True,
                      update_ret=True, obs_eps=1e-8, ret_eps=1e-8, max_obs_scale=None, clip_reward=None):
    """hg_rollout_stats in NumPy: the moments in float64 (two passes over the batch, then Chan's update), the
    per-env scans in the device's float32 (ep_ret by float32 additions; G = fma(gamma, G, r) through float64,
    where the product of two float32 is exact, rounded to float32 once more).  `state`: None for a fresh one
    (rollout_stats_fresh) or the dict a previous call returned; it is not modified.  obs [K,N,17], reward
    [K,N], terminated / truncated / info [K,N] (arrays or tensors).  Returns (new state, outputs) with outputs
    obs_mean, obs_scale [17], reward_scale [1], reward_out [K,N] (float32), obs_in [K,N,17] (with obs0),
    episode [16] (float32, EPISODE_FIELDS), and, for the tests, `returns`: the samples of G [K,N] and
    `episode_returns` / `episode_lengths`: the completed episodes in (step, env) order."""
    obs, reward = _np(obs, np.float32), _np(reward, np.float32)
    term, trunc = _np(terminated, np.uint8), _np(truncated, np.uint8)
    info, obs0 = _np(info, np.uint8), _np(obs0, np.float32)
    K, N = reward.shape
    s = dict(rollout_stats_fresh(N) if state is None else state)
    G, er, el = s["G"].copy(), s["ep_ret"].copy(), s["ep_len"].copy()
    g32 = np.float64(np.float32(gamma))
    samples = np.empty((K, N), np.float32)
    ep_ret, ep_len, ep_term, ep_succ = [], [], [], []
    with np.errstate(all="ignore"):
        for k in range(K):
            r = reward[k]
            G = (g32 * G.astype(np.float64) + r.astype(np.float64)).astype(np.float32)
            samples[k] = G
            er = er + r
            el = el + 1
            done = (term[k] | trunc[k]) != 0
            if done.any():
                ep_ret.append(er[done])
                ep_len.append(el[done])
                ep_term.append(term[k][done] != 0)
                ep_succ.append((info[k][done] & _abi.HG_INFO_SUCCESSED) != 0 if info is not None else np.zeros(done.sum(), bool))
                G, er, el = np.where(done, np.float32(0), G), np.where(done, np.float32(0), er), np.where(done, 0, el)
    s["G"], s["ep_ret"], s["ep_len"] = G.astype(np.float32), er.astype(np.float32), el.astype(np.int32)
    ep_ret = np.concatenate(ep_ret) if ep_ret else np.zeros(0, np.float32)
    ep_len = np.concatenate(ep_len) if ep_len else np.zeros(0, np.int32)
    ep_term = np.concatenate(ep_term) if ep_term else np.zeros(0, bool)
    ep_succ = np.concatenate(ep_succ) if ep_succ else np.zeros(0, bool)

    rows = obs.reshape(K * N, N_OBS)
    row_ok = np.isfinite(rows).all(axis=1)
    ret_ok = np.isfinite(samples.reshape(-1))
    if update_obs:
        s["obs_count"], s["obs_mean"], s["obs_M2"] = _chan(s["obs_count"], s["obs_mean"], s["obs_M2"],
                                                           rows[row_ok].astype(np.float64))
        s["skipped_rows"] = s["skipped_rows"] + int((~row_ok).sum())
    if update_ret:
        n, m, m2 = _chan(s["ret_count"], s["ret_mean"], s["ret_M2"], samples.reshape(-1)[ret_ok].astype(np.float64))
        s["ret_count"], s["ret_mean"], s["ret_M2"] = n, float(m), float(m2)
        s["skipped_returns"] = s["skipped_returns"] + int((~ret_ok).sum())
    if update_obs or update_ret:
        s["episodes"] = s["episodes"] + len(ep_ret)
        s["env_steps"] = s["env_steps"] + K * N

    out = {}
    inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        if s["obs_count"] > 0:
            out["obs_mean"] = np.asarray(s["obs_mean"], np.float64).astype(np.float32)
            scale = (1.0 / np.sqrt(np.asarray(s["obs_M2"], np.float64) / s["obs_count"] + obs_eps)).astype(np.float32)
            out["obs_scale"] = np.minimum(scale, inf if max_obs_scale is None else np.float32(max_obs_scale))
        else:
            out["obs_mean"], out["obs_scale"] = np.zeros(N_OBS, np.float32), np.ones(N_OBS, np.float32)
        rs = np.float32(1.0 / np.sqrt(s["ret_M2"] / s["ret_count"] + ret_eps)) if s["ret_count"] > 0 else np.float32(1.0)
        out["reward_scale"] = np.array([rs], np.float32)
        clip = inf if clip_reward is None else np.float32(clip_reward)
        x = reward * rs
        x = np.where(x > clip, clip, x)
        out["reward_out"] = np.where(x < -clip, -clip, x).astype(np.float32)
        if obs0 is not None:
            out["obs_in"] = np.concatenate([obs0[None], obs[:-1]], axis=0)
        e = np.zeros(16, np.float64)
        fin = np.isfinite(ep_ret)
        good = ep_ret[fin].astype(np.float64)
        e[0] = len(ep_ret)
        e[1:6] = np.nan
        if len(good):
            e[1], e[2], e[3], e[4] = good.mean(), good.std(), good.min(), good.max()
        if len(ep_ret):
            e[5] = ep_len.astype(np.float64).mean()
        e[6], e[7], e[8] = ep_term.sum(), (~ep_term).sum(), ep_succ.sum()
        rf = reward[np.isfinite(reward)].astype(np.float64)
        e[9] = rf.mean() if len(rf) else np.nan
        e[10], e[11], e[12] = (~row_ok).sum(), (~ret_ok).sum(), (~fin).sum()
        out["episode"] = e.astype(np.float32)
    out["returns"], out["episode_returns"], out["episode_lengths"] = samples, ep_ret, ep_len
    return s, out
