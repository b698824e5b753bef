"""GPU: running normalisation and episode statistics on the device (hg_rollout_stats, hg_rollout_stats_init,
HeliVecEnv.rollout_stats) against heligym_amd.stats.rollout_stats_ref.

  1. against the reference in float64, at shapes on each side of every loop bound of the kernels;
  2. persistence: one call on K rows against two calls on its halves, an episode crossing the split;
  3. non-finite values are skipped and counted, the head stays finite, the env recovers;
  4. frozen (update = 0): the head is untouched, the scans and the episode aggregates advance;
  5. determinism, and a captured call replayed against eager calls;
  6. on a real env's rollout, which leaves the env untouched and feeds set_policy_theta / ppo_grad;
  7. argument errors leave the state and every output untouched.

Synthetic batches: seeded NumPy, a done flag on about one step in five, a column at 1e4 +- 1e-2 (column 3), a
constant column (column 9).  The kernels' loop bounds (csrc/rollout_stats.hip, rollout_stats.h):
  SCAN_UNROLL = 8       steps of an env's scan loaded ahead of the dependent chain; the last K % 8 in a batch of their own
  SCAN_ENVS   = 65 536  envs of the scan's largest grid (256 blocks x 256 lanes); past it a lane takes several
  TILE_ROWS   = 1 024   flat rows of obs per tile of the observation pass; the last tile is partial
  OBS_ROWS    = 524 288 rows of the observation pass's largest grid (512 blocks x TILE_ROWS); past it a block
                        takes several tiles
  N % 4                 the shifted copy uses 16-byte stores when N is a multiple of 4 and 4-byte stores otherwise
Run with -m gpu."""
import ctypes

import numpy as np
import pytest

from test_gpu_policy_rollout import _assert_same

from heligym_amd import stats as hstats

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAMMA = 0.97
SCAN_UNROLL, SCAN_ENVS, TILE_ROWS, OBS_ROWS = 8, 65536, 1024, 524288
# (K, N): every case but the last has at most 2^17 rows
SHAPES = [
    (1, 1),                 # one row: everything below every bound (the scan's remainder alone), a tile of one row
    (SCAN_UNROLL, 4),       # exactly one unrolled batch and no remainder, 16-byte copy stores
    (19, 65),               # K = 2 x 8 + 3: two batches and a remainder; N % 4 = 1: 4-byte copy stores; 1 235 rows: 2 tiles
    (SCAN_UNROLL + 7, 3),   # a batch and the longest remainder
    (11, 260),              # N % 4 = 0 over 2 860 rows: two whole tiles and a partial one
    (1, SCAN_ENVS + 65),    # above the scan's grid: lanes 0 .. 64 take two envs; 65 tiles
    # the observation pass's block loop runs twice only past 524 288 rows, so this one case is larger than the
    # 2^17 rows the others keep to: 590 436 rows (40 MB), 577 tiles on 512 blocks, N a multiple of 4
    (9, SCAN_ENVS + 68),
]
assert all(K * N <= 2 ** 17 for K, N in SHAPES[:-1]) and SHAPES[-1][0] * SHAPES[-1][1] > OBS_ROWS
assert SHAPES[2] == (19, 65) and 19 % SCAN_UNROLL and 19 > SCAN_UNROLL and 19 * 65 % TILE_ROWS and 19 * 65 > TILE_ROWS


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


@pytest.fixture(scope="module")
def envs(torch):
    """N -> a HeliVecEnv of N envs (hg_rollout_stats uses the handle for N and its device only)."""
    from heligym_amd import HeliVecEnv
    made = {}

    def get(n):
        if n not in made:
            made[n] = HeliVecEnv(n, task="hover", dt=0.01, device=DEV, seed=1)
        return made[n]
    yield get
    for e in made.values():
        e.close()


def make_batch(K, N, seed):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((K, N, 17), dtype=np.float32) * np.logspace(-2, 3, 17, dtype=np.float32)
    obs += np.linspace(-50, 50, 17, dtype=np.float32)
    obs[..., 3] = (1e4 + 1e-2 * rng.standard_normal((K, N))).astype(np.float32)
    obs[..., 9] = np.float32(-3.25)
    reward = rng.standard_normal((K, N), dtype=np.float32) + np.float32(0.3)
    u = rng.random((K, N))
    term, trunc = (u < 0.1).astype(np.uint8), ((u > 0.05) & (u < 0.2)).astype(np.uint8)   # both set on 1 in 20
    info = (2 * (term & (rng.random((K, N)) < 0.5)) + 16 * (term | trunc)).astype(np.uint8)
    obs0 = rng.standard_normal((N, 17), dtype=np.float32)
    return dict(obs=obs, reward=reward, terminated=term, truncated=trunc, info=info, obs0=obs0)


def cut(b, lo, hi):
    """Steps lo .. hi-1 of a batch, with the obs0 that goes with them."""
    c = {k: b[k][lo:hi] for k in ("obs", "reward", "terminated", "truncated", "info")}
    c["obs0"] = b["obs0"] if lo == 0 else b["obs"][lo - 1]
    return c


def device_call(torch, env, S, b, outputs=True, **kw):
    """env.rollout_stats on a batch -> everything it wrote, on the host."""
    t = torch
    d = {k: t.as_tensor(v, device=DEV) for k, v in b.items()}
    K, N = b["reward"].shape
    obs_in = t.full((K, N, 17), -7.0, device=DEV) if outputs else None
    rew_out = t.full((K, N), -7.0, device=DEV) if outputs else None
    env.rollout_stats(S, d, gamma=GAMMA, obs0=d["obs0"] if outputs else None, obs_in=obs_in, reward_out=rew_out, **kw)
    t.cuda.synchronize()
    return read_back(S, obs_in, rew_out)


def read_back(S, obs_in=None, rew_out=None):
    r = dict(head=S.head.cpu().numpy(), G=S.G.cpu().numpy(), ep_ret=S.ep_ret.cpu().numpy(), ep_len=S.ep_len.cpu().numpy(),
             obs_mean=S.obs_mean.cpu().numpy(), obs_scale=S.obs_scale.cpu().numpy(),
             reward_scale=S.reward_scale.cpu().numpy(), episode=S.episode.cpu().numpy())
    if obs_in is not None:
        r["obs_in"], r["reward_out"] = obs_in.cpu().numpy(), rew_out.cpu().numpy()
    return r


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where(np.isnan(a), 0, d).max() if d.size else 0


def g64(batches, N):
    """The float64 chain of G over the batches: (final G [N], the largest finite |G| met)."""
    G, top = np.zeros(N), 0.0
    g = float(np.float32(GAMMA))
    with np.errstate(all="ignore"):
        for b in batches:
            for k in range(b["reward"].shape[0]):
                G = g * G + b["reward"][k].astype(np.float64)
                if np.isfinite(G).any():
                    top = max(top, np.abs(G[np.isfinite(G)]).max())
                G = np.where((b["terminated"][k] | b["truncated"][k]) != 0, 0.0, G)
    return G, top


def check_moments(dev, ref):
    """The head against the reference's state: mean within 1e-9 (|mean| + std), M2 within 1e-9 relative (fp64 sums
    of <= 2^20 terms give <= 1.2e-10; the shift's cancellation factor 1 + ((mean - c) / std)^2 is <= ~50 for c a
    sample or the running mean; the merge adds a little), counts exact."""
    h, L = dev["head"], hstats.STATS_HEAD
    assert np.isfinite(h).all()
    assert h[L["obs_count"]] == ref["obs_count"] and h[L["ret_count"]] == ref["ret_count"]
    for k in ("episodes", "env_steps", "skipped_rows", "skipped_returns"):
        assert h[L[k]] == ref[k], (k, h[L[k]], ref[k])
    assert np.all(h[42:] == 0)
    if ref["obs_count"]:
        mean, m2 = h[1:18], h[18:35]
        std = np.sqrt(np.asarray(ref["obs_M2"]) / ref["obs_count"])
        err = np.abs(mean - ref["obs_mean"]) / (np.abs(ref["obs_mean"]) + std)
        print("obs mean error / (|mean| + std):", err.max(), " M2 relative error:",
              (np.abs(m2 - ref["obs_M2"]) / np.maximum(ref["obs_M2"], 1e-300)).max())
        assert np.all(np.abs(mean - ref["obs_mean"]) <= 1e-9 * (np.abs(ref["obs_mean"]) + std))
        assert np.all(np.abs(m2 - ref["obs_M2"]) <= 1e-9 * np.asarray(ref["obs_M2"]))
    if ref["ret_count"]:
        std = np.sqrt(ref["ret_M2"] / ref["ret_count"])
        print("ret mean error:", abs(h[36] - ref["ret_mean"]), " M2 relative error:",
              abs(h[37] - ref["ret_M2"]) / max(ref["ret_M2"], 1e-300))
        assert abs(h[36] - ref["ret_mean"]) <= 1e-9 * (abs(ref["ret_mean"]) + std)
        assert abs(h[37] - ref["ret_M2"]) <= 1e-9 * ref["ret_M2"]


def check_outputs(dev, b, obs_eps=1e-8, ret_eps=1e-8, max_obs_scale=None, clip_reward=None):
    """The outputs against the formulas on the DEVICE's own head (float64, rounded to float32 once)."""
    h = dev["head"]
    with np.errstate(all="ignore"):
        if h[0] > 0:
            assert np.array_equal(dev["obs_mean"].view(np.int32), h[1:18].astype(np.float32).view(np.int32))
            want = (1.0 / np.sqrt(h[18:35] / h[0] + obs_eps)).astype(np.float32)
            if max_obs_scale is not None:
                want = np.minimum(want, np.float32(max_obs_scale))
            assert ulps(dev["obs_scale"], want) <= 2
        else:
            assert np.all(dev["obs_mean"] == 0) and np.all(dev["obs_scale"] == 1)
        want = np.float32(1.0 / np.sqrt(h[37] / h[35] + ret_eps)) if h[35] > 0 else np.float32(1.0)
        assert ulps(dev["reward_scale"], [want]) <= 2
        if "reward_out" in dev:
            x = b["reward"] * dev["reward_scale"][0]
            if clip_reward is not None:
                c = np.float32(clip_reward)
                x = np.where(x > c, c, x)
                x = np.where(x < -c, -c, x)
            assert np.array_equal(dev["reward_out"].view(np.int32), x.astype(np.float32).view(np.int32))
            assert np.array_equal(dev["obs_in"][0].view(np.int32), b["obs0"].view(np.int32))
            assert np.array_equal(dev["obs_in"][1:].view(np.int32), b["obs"][:-1].view(np.int32))


def check_scans(dev, ref, ref_out, batches, k_total):
    """The per-env arrays and episode_out against the reference."""
    N = ref["G"].shape[0]
    assert np.array_equal(dev["ep_len"], ref["ep_len"])
    assert np.array_equal(dev["ep_ret"].view(np.int32), ref["ep_ret"].view(np.int32))   # sequential float32 additions
    # G is a chain of k_total fused multiply-adds, each within 2^-24 of its exact value, against the float64 chain
    G, top = g64(batches, N)
    tol = k_total * 2.0 ** -23 * max(1.0, top)
    fin = np.isfinite(G)
    assert np.array_equal(np.isfinite(dev["G"]), fin)
    print("G error:", np.abs(dev["G"][fin] - G[fin]).max() if fin.any() else 0.0, " allowed:", tol)
    assert np.all(np.abs(dev["G"][fin] - G[fin]) <= tol)
    e, r = dev["episode"], ref_out["episode"]
    for j in (0, 6, 7, 8, 10, 11, 12, 13, 14, 15):   # counts: exact
        assert e[j] == r[j], (j, e[j], r[j])
    for j in (3, 4):   # min, max: order-free
        assert ulps(e[j:j + 1], r[j:j + 1]) == 0, j
    for j in (1, 5, 9):   # means: fp64 sums in another order, rounded to float32 once
        assert ulps(e[j:j + 1], r[j:j + 1]) <= 2, (j, e[j], r[j])
    # the standard deviation comes from sum r^2 / n - mean^2 in fp64: its variance is off by at most a few 2^-53 of
    # (mean^2 + variance), the square root of which bounds the error where the true deviation is 0
    if not np.isnan(r[2]):
        assert abs(float(e[2]) - float(r[2])) <= 2 * np.spacing(np.float32(r[2])) + 3e-8 * abs(float(r[1])), (e[2], r[2])
    else:
        assert np.isnan(e[2])


def full_check(torch, env, b, **kw):
    from heligym_amd import RolloutStats, rollout_stats_ref
    S = RolloutStats(env)
    dev = device_call(torch, env, S, b, **kw)
    ref, ref_out = rollout_stats_ref(None, b["obs"], b["reward"], b["terminated"], b["truncated"], b["info"], b["obs0"],
                                     gamma=GAMMA, **kw)
    check_moments(dev, ref)
    check_outputs(dev, b, **{k: v for k, v in kw.items() if k in ("max_obs_scale", "clip_reward")})
    check_scans(dev, ref, ref_out, [b], b["reward"].shape[0])
    return S, dev, ref, ref_out


# ------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("K,N", SHAPES)
def test_against_the_reference(torch, envs, K, N):
    b = make_batch(K, N, seed=K * 1000 + N)
    kw = dict(max_obs_scale=50.0, clip_reward=1.5) if (K, N) == (19, 65) else {}
    S, dev, ref, _ = full_check(torch, envs(N), b, **kw)
    h = dev["head"]
    assert h[1 + 9] == -3.25 and h[18 + 9] == 0.0          # the constant column is exact
    assert dev["obs_mean"][9] == np.float32(-3.25)
    assert abs(h[1 + 3] - 1e4) < 5e-2 and (K * N < 100 or 0.5e-4 < h[18 + 3] / h[0] < 2e-4)   # 1e4 +- 1e-2 survives
    if kw:
        assert dev["obs_scale"].max() == 50.0 and np.abs(dev["reward_out"]).max() == 1.5
    assert dev["episode"][0] == ((b["terminated"] | b["truncated"]) != 0).sum()
    assert S.moments()["obs_count"] == K * N and S.episode_dict()["episodes"] == dev["episode"][0]


def test_init_zeroes_by_a_kernel_and_optional_arguments(torch, envs):
    """hg_rollout_stats_init over a dirty state; a call without info, obs0 or any optional output."""
    from heligym_amd import RolloutStats, rollout_stats_ref
    K, N = 19, 65
    env, b = envs(N), make_batch(19, 65, seed=3)
    S = RolloutStats(env)
    S.state.fill_(0x7FC00001)
    S.obs_scale.fill_(9.0)
    S.zero_()
    torch.cuda.synchronize()
    assert int(S.state.abs().max()) == 0 and float(S.obs_scale.max()) == 1.0
    d = {k: torch.as_tensor(b[k], device=DEV) for k in ("obs", "reward", "terminated", "truncated")}
    env.rollout_stats(S, d, gamma=GAMMA)
    torch.cuda.synchronize()
    dev = read_back(S)
    ref, ref_out = rollout_stats_ref(None, b["obs"], b["reward"], b["terminated"], b["truncated"], gamma=GAMMA)
    check_moments(dev, ref)
    check_outputs(dev, b)
    check_scans(dev, ref, ref_out, [b], K)
    assert dev["episode"][8] == 0 and dev["episode"][0] > 0   # no info: no success count


# ------------------------------------------------------------------------------------------- 2. persistence
def test_two_calls_on_the_halves_are_one_call(torch, envs):
    from heligym_amd import RolloutStats, rollout_stats_ref
    K, N, split = 19, 65, 8
    env, b = envs(N), make_batch(K, N, seed=77)
    for k in (split - 2, split - 1, split):   # env 5's episode crosses the split, from step 5 to step 10
        b["terminated"][k, 5] = b["truncated"][k, 5] = 0
    b["terminated"][split - 3, 5] = b["terminated"][split + 1, 5] = 1
    _, one, ref_one, _ = full_check(torch, env, b)
    S = RolloutStats(env)
    b1, b2 = cut(b, 0, split), cut(b, split, K)
    d1 = device_call(torch, env, S, b1)
    r1, o1 = rollout_stats_ref(None, b1["obs"], b1["reward"], b1["terminated"], b1["truncated"], b1["info"], b1["obs0"], GAMMA)
    check_moments(d1, r1)
    check_scans(d1, r1, o1, [b1], split)
    d2 = device_call(torch, env, S, b2)
    r2, o2 = rollout_stats_ref(r1, b2["obs"], b2["reward"], b2["terminated"], b2["truncated"], b2["info"], b2["obs0"], GAMMA)
    check_moments(d2, r2)       # the merged state against the two-call reference
    check_moments(d2, ref_one)  # and against the one-call reference
    check_outputs(d2, b2)
    check_scans(d2, r2, o2, [b1, b2], K)
    for k in ("G", "ep_ret", "ep_len"):   # bitwise the single call's
        assert np.array_equal(d2[k].view(np.int32), one[k].view(np.int32)), k
    assert np.array_equal(d2["head"][[0, 35, 38, 39, 40, 41]], one["head"][[0, 35, 38, 39, 40, 41]])
    assert d1["episode"][0] + d2["episode"][0] == one["episode"][0]
    # the crossing episode: counted once, in the second call, with its whole length and return
    whole = b["reward"][split - 2:split + 2, 5]
    ret = np.float32(0)
    for x in whole:
        ret = np.float32(ret + x)
    at = [i for i, (ln, rt) in enumerate(zip(o2["episode_lengths"], o2["episode_returns"])) if ln == 4 and rt == ret]
    assert len(at) >= 1 and not any(ln == 4 and rt == ret for ln, rt in zip(o1["episode_lengths"], o1["episode_returns"]))


# ------------------------------------------------------------------------------------------- 3. non-finite
def test_non_finite_values_are_skipped_and_counted(torch, envs):
    K, N = 19, 65
    env, b = envs(N), make_batch(K, N, seed=5)
    b["obs"][4, 17, 11] = np.inf
    b["reward"][6, 30] = np.nan
    b["terminated"][6:9, 30] = b["truncated"][6:9, 30] = 0   # the NaN lives for steps 6, 7, 8, 9
    b["terminated"][9, 30] = 1
    S, dev, ref, ref_out = full_check(torch, env, b)   # (the reference skips the same, nothing is left out)
    h = dev["head"]
    assert h[0] == K * N - 1 and h[40] == 1 and dev["episode"][10] == 1
    assert h[35] == K * N - 4 and h[41] == 4 and dev["episode"][11] == 4
    assert dev["episode"][12] == 1 and np.isfinite(dev["episode"][1:6]).all()
    assert np.isfinite(h).all()
    assert np.isfinite(dev["G"]).all() and np.isfinite(dev["ep_ret"]).all()   # env 30 recovered at its episode's end
    assert np.isnan(dev["reward_out"][6, 30]) and np.isfinite(np.delete(dev["reward_out"].ravel(), 6 * N + 30)).all()
    assert np.isinf(dev["obs_in"][5, 17, 11])   # the copy is bitwise, whatever the values


# ------------------------------------------------------------------------------------------- 4. frozen
def test_frozen_head(torch, envs):
    from heligym_amd import rollout_stats_ref
    K, N = 19, 65
    env = envs(N)
    b, c = make_batch(K, N, seed=8), make_batch(K, N, seed=9)
    S, d1, r1, _ = full_check(torch, env, b)
    d2 = device_call(torch, env, S, c, update_obs=False, update_ret=False)
    r2, o2 = rollout_stats_ref(r1, c["obs"], c["reward"], c["terminated"], c["truncated"], c["info"], c["obs0"], GAMMA,
                               update_obs=False, update_ret=False)
    assert np.array_equal(d2["head"].view(np.int64), d1["head"].view(np.int64))   # bitwise
    for k in ("obs_mean", "obs_scale", "reward_scale"):   # from the state as it stands: the first call's, bitwise
        assert np.array_equal(d2[k].view(np.int32), d1[k].view(np.int32)), k
    check_outputs(d2, c)
    check_scans(d2, r2, o2, [b, c], 2 * K)   # the scans and the episode aggregates advance
    assert d2["episode"][0] > 0 and not np.array_equal(d2["episode"], d1["episode"])
    # one part frozen, the other not
    d3 = device_call(torch, env, S, b, update_obs=False)
    r3, _ = rollout_stats_ref(r2, b["obs"], b["reward"], b["terminated"], b["truncated"], b["info"], b["obs0"], GAMMA,
                              update_obs=False)
    assert np.array_equal(d3["head"][:35].view(np.int64), d1["head"][:35].view(np.int64)) and d3["head"][35] == 2 * K * N
    check_moments(d3, r3)


# ------------------------------------------------------------------------------------------- 5. determinism, capture
def test_same_call_same_bits_and_a_captured_call(torch, envs):
    from heligym_amd import RolloutStats
    K, N = 19, 65
    env = envs(N)
    t = torch
    batches = [make_batch(K, N, seed=s) for s in (21, 22, 23)]
    A = RolloutStats(env)
    first = device_call(t, env, A, batches[0])
    snap = A.state.clone()
    a = device_call(t, env, A, batches[1], clip_reward=2.0)
    A.state.copy_(snap)
    a2 = device_call(t, env, A, batches[1], clip_reward=2.0)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), a2[k].view(np.uint8)), k
    assert not np.array_equal(a["head"], first["head"])
    # a captured call replayed three times against three eager calls
    E, G_ = RolloutStats(env), RolloutStats(env)
    d = {k: t.as_tensor(v).to(DEV) for k, v in batches[0].items()}
    outs = {w: (t.empty((K, N, 17), device=DEV), t.empty((K, N), device=DEV)) for w in "eg"}
    kw = dict(gamma=GAMMA, obs0=d["obs0"], max_obs_scale=20.0, clip_reward=2.0)
    env.rollout_stats(RolloutStats(env), d, obs_in=outs["g"][0], reward_out=outs["g"][1], **kw)   # (every kernel has run once)
    t.cuda.synchronize()
    side = t.cuda.Stream()
    side.wait_stream(t.cuda.current_stream())
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph, stream=side):
        env.rollout_stats(G_, d, obs_in=outs["g"][0], reward_out=outs["g"][1], **kw)
    assert float(G_.head[0]) == 0.0   # captured, not run
    for b in batches:
        for k, v in b.items():
            d[k].copy_(t.as_tensor(v))
        graph.replay()
        env.rollout_stats(E, d, obs_in=outs["e"][0], reward_out=outs["e"][1], **kw)
        t.cuda.synchronize()
        w = S_words(G_)
        _assert_same(t, G_.state[:w], E.state[:w], "state")
        for k in ("obs_mean", "obs_scale", "reward_scale", "episode"):
            _assert_same(t, getattr(G_, k), getattr(E, k), k)
        _assert_same(t, outs["g"][0], outs["e"][0], "obs_in")
        _assert_same(t, outs["g"][1], outs["e"][1], "reward_out")
    assert float(G_.head[0]) == 3 * K * N


def S_words(S):
    """The words of the state before the workspace (head and per-env arrays)."""
    return hstats.STATS_HEAD_BYTES // 4 + 3 * S.G.shape[0]


# ------------------------------------------------------------------------------------------- 6. a real env
def test_on_a_real_rollout(torch):
    import types
    from heligym_amd import ActorCriticParams, HeliVecEnv, RolloutStats, rollout_stats_ref
    t = torch
    nn = t.nn
    K, N = 8, 128
    t.manual_seed(4)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
    cpu = ActorCriticParams(actor, nn.Linear(64, 1), nn.Parameter(t.full((4,), -1.0)))
    P = types.SimpleNamespace(theta=cpu.theta.detach().to(DEV).clone(), grad=t.zeros((5641,), device=DEV))
    env = HeliVecEnv(N, task="hover", dt=0.01, device=DEV, seed=6, autoreset=True, autoreset_mode="same_step",
                     max_episode_steps=5)
    try:
        env.set_policy_theta(P)
        obs0 = env.reset()[0].clone()
        out = env.rollout_actor_critic(K, gamma=GAMMA, obs0=obs0)
        S = RolloutStats(env)
        obs_in, rew_out = t.empty((K, N, 17), device=DEV), t.empty((K, N), device=DEV)
        t.cuda.synchronize()
        s0, c0 = (x.clone() for x in env.get_state())
        assert env.rollout_stats(S, out, gamma=GAMMA, obs0=obs0, obs_in=obs_in, reward_out=rew_out) is S
        t.cuda.synchronize()
        s1, c1 = env.get_state()
        _assert_same(t, s0, s1, "env state")
        _assert_same(t, c0, c1, "env counters")
        b = {k: out[k].cpu().numpy() for k in ("obs", "reward", "terminated", "truncated", "info")}
        b["obs0"] = obs0.cpu().numpy()
        dev = read_back(S, obs_in, rew_out)
        ref, ref_out = rollout_stats_ref(None, out["obs"], out["reward"], out["terminated"], out["truncated"], out["info"],
                                         obs0, gamma=GAMMA)
        check_moments(dev, ref)
        check_outputs(dev, b)
        check_scans(dev, ref, ref_out, [b], K)
        assert dev["episode"][7] > 0 and dev["episode"][0] >= N   # the TimeLimit of 5 steps truncates
        assert dev["episode"][5] <= 5
        # the tensors go to the policy and the learner as they are
        env.set_policy_theta(P, S.obs_mean, S.obs_scale)
        g, st = env.ppo_grad(P, obs_in, out["actions"], out["logp"], out["advantages"], out["returns"],
                             obs_mean=S.obs_mean, obs_scale=S.obs_scale)
        t.cuda.synchronize()
        assert bool(t.isfinite(g).all()) and bool(t.isfinite(st).all())
        # rollout_policy's tuple is read the same way
        S2 = RolloutStats(env)
        env.rollout_stats(S2, tuple(out[k] for k in ("actions", "obs", "reward", "terminated", "truncated", "info")),
                          gamma=GAMMA)
        t.cuda.synchronize()
        w = S_words(S)
        _assert_same(t, S2.state[:w], S.state[:w], "state from the tuple")
    finally:
        env.close()


# ------------------------------------------------------------------------------------------- 7. refusals
def test_argument_errors_touch_nothing(torch, envs):
    from heligym_amd import RolloutStats, _abi
    t = torch
    K, N = 3, 4
    env = envs(N)
    lib = env.lib
    S = RolloutStats(env)
    S.state.fill_(0x3F800001)
    f = lambda *s: t.full(s, 5.5, device=DEV)   # noqa: E731
    u = lambda: t.zeros((K, N), dtype=t.uint8, device=DEV)   # noqa: E731
    bufs = dict(obs=f(K, N, 17), reward=f(K, N), term=u(), trunc=u(), info=u(), obs0=f(N, 17), mean=f(17), scale=f(17),
                rscale=f(4), rout=f(K, N), oin=f(K, N, 17), epi=f(16))
    before = {k: v.clone() for k, v in bufs.items()}
    state_before = S.state.clone()
    p = {k: v.data_ptr() for k, v in bufs.items()}
    good = dict(gamma=0.99, obs_eps=1e-8, ret_eps=1e-8, max_obs_scale=float("inf"), clip_reward=float("inf"), update=3)

    def call(cfg=None, h=env._h, state=S.state.data_ptr(), nsteps=K, null_cfg=False, **ptr):
        q = dict(p, **ptr)
        c = dict(good, **(cfg or {}))
        cs = _abi.hg_rollout_stats_cfg(c["gamma"], c["obs_eps"], c["ret_eps"], c["max_obs_scale"], c["clip_reward"],
                                       c["update"], 0)
        return lib.hg_rollout_stats(h, state, q["obs"], q["reward"], q["term"], q["trunc"], q["info"], q["obs0"], nsteps,
                                    None if null_cfg else ctypes.byref(cs), q["mean"], q["scale"], q["rscale"], q["rout"],
                                    q["oin"], q["epi"], None)

    cases = [
        (dict(h=None), "env is NULL"),
        (dict(state=None), "state must be a device pointer"),
        (dict(state=S.state.data_ptr() + 8), "state must be 16-byte aligned"),
        (dict(obs=None), "must be device pointers"), (dict(reward=None), "must be device pointers"),
        (dict(term=None), "must be device pointers"), (dict(trunc=None), "must be device pointers"),
        (dict(null_cfg=True), "cfg a host pointer"),
        (dict(obs=p["obs"] + 4), "16-byte aligned"), (dict(obs0=p["obs0"] + 8), "16-byte aligned"),
        (dict(oin=p["oin"] + 4), "16-byte aligned"),
        (dict(reward=p["reward"] + 2), "4-byte aligned"), (dict(rscale=p["rscale"] + 1), "4-byte aligned"),
        (dict(nsteps=0), "nsteps must be >= 1"), (dict(nsteps=-2), "nsteps must be >= 1"),
        (dict(obs0=None), "obs_in_out needs obs0"),
        (dict(rout=p["reward"]), "reward_out must not be reward"),
        (dict(cfg=dict(gamma=1.0000001)), "gamma must be in [0, 1]"), (dict(cfg=dict(gamma=-0.1)), "gamma must be in [0, 1]"),
        (dict(cfg=dict(gamma=float("nan"))), "gamma must be in [0, 1]"),
        (dict(cfg=dict(obs_eps=-1e-9)), "obs_eps and ret_eps"), (dict(cfg=dict(ret_eps=float("nan"))), "obs_eps and ret_eps"),
        (dict(cfg=dict(max_obs_scale=0.0)), "max_obs_scale and clip_reward"),
        (dict(cfg=dict(clip_reward=float("nan"))), "max_obs_scale and clip_reward"),
        (dict(cfg=dict(update=4)), "unknown update bits"),
    ]
    for kw, text in cases:
        lib.hg_num_envs(None)   # (leaves another message behind)
        assert call(**kw) == -1, kw
        assert text.encode() in lib.hg_last_error(), (kw, lib.hg_last_error())
    for h, st, text in ((None, S.state.data_ptr(), "env is NULL"), (env._h, None, "state must be a device pointer"),
                        (env._h, S.state.data_ptr() + 4, "16-byte aligned")):
        assert lib.hg_rollout_stats_init(h, st, None) == -1 and text.encode() in lib.hg_last_error()
    t.cuda.synchronize()
    _assert_same(t, S.state, state_before, "state")
    for k, v in bufs.items():
        _assert_same(t, v, before[k], k)
    S.zero_()
    assert call() == 0   # the same arguments, unspoiled, are accepted
    t.cuda.synchronize()
    assert not t.equal(bufs["scale"], before["scale"]) and float(bufs["epi"][0]) == 0.0 and float(S.head[0]) == K * N
