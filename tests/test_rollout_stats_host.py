"""CPU-side checks of the running-normalisation surface (hg_rollout_stats_state_bytes, hg_rollout_stats_init,
hg_rollout_stats): the symbols are exported and declared with the header's argument counts, refuse a NULL env,
the state's layout in heligym_amd.stats is the header's, the ctypes mirror of the configuration is the header's
struct, HeliVecEnv.rollout_stats refuses bad arguments with ValueError before the library is called, and
rollout_stats_ref agrees with an independent scalar two-pass computation.  No device calls."""
import ctypes
import re

import numpy as np
import pytest
import torch

from test_branch_host import _bare_env
from test_policy_host import HEADER, header_arg_counts

from heligym_amd import RolloutStats, _abi, rollout_stats_ref, stats

NEW = {"hg_rollout_stats_state_bytes": 1, "hg_rollout_stats_init": 3, "hg_rollout_stats": 17}


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_stats_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    assert counts["hg_gae"] == 12   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == n, name
    assert lib.hg_abi_version() == 3 == _abi.HG_ABI_VERSION   # purely additive
    assert re.search(r"#define\s+HG_ABI_VERSION\s+3\b", open(HEADER).read())


def test_stats_calls_refuse_a_null_env(lib):
    cfg = _abi.hg_rollout_stats_cfg(0.99, 1e-8, 1e-8, float("inf"), float("inf"), 3, 0)
    calls = {"hg_rollout_stats_init": (None, 0x1000, None),
             "hg_rollout_stats": (None, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None, None, 4, ctypes.byref(cfg))
             + (None,) * 7}
    for name, args in calls.items():
        lib.hg_num_envs(None)
        assert getattr(lib, name)(*args) == -1, name
        assert b"env is NULL" in lib.hg_last_error(), name


def test_state_bytes_and_layout_are_the_headers(lib):
    for n in (1, 2, 3, 4, 5, 64, 65, 4096, 65536, 100003):
        b = lib.hg_rollout_stats_state_bytes(n)
        assert b == stats.stats_state_bytes(n), n
        assert b % 16 == 0
        assert b >= stats.STATS_HEAD_BYTES + 12 * n + stats.STATS_WORKSPACE_BYTES
        assert lib.hg_rollout_stats_state_bytes(n + 4) - b == 48   # 12 bytes per env (the padding has period 4)
    assert lib.hg_rollout_stats_state_bytes(0) < 0 and lib.hg_rollout_stats_state_bytes(-7) < 0
    txt = open(HEADER).read()
    L = stats.STATS_HEAD
    assert list(L) == ["obs_count", "obs_mean", "obs_M2", "ret_count", "ret_mean", "ret_M2", "episodes", "env_steps",
                       "skipped_rows", "skipped_returns"]
    for name, off in L.items():
        kind = r" \[17\]" if name in ("obs_mean", "obs_M2") else r"\s"
        assert re.search(rf"\b{off}: {name}{kind}", txt), name
    assert L["obs_M2"] == L["obs_mean"] + 17 and L["ret_count"] == L["obs_M2"] + 17
    assert max(L.values()) < stats.STATS_HEAD_DOUBLES == 48 and stats.STATS_HEAD_BYTES == 384
    assert re.search(r"an fp64 head of 48 doubles", txt) and re.search(r"\b384: G \[N\] fp32", txt)
    assert re.search(rf"a workspace of {stats.STATS_WORKSPACE_BYTES} bytes", txt)
    m = re.search(r"enum\s*\{\s*HG_STATS_UPDATE_OBS\s*=\s*(\d+)\s*,\s*HG_STATS_UPDATE_RET\s*=\s*(\d+)\s*\}", txt)
    assert m and (int(m.group(1)), int(m.group(2))) == (_abi.HG_STATS_UPDATE_OBS, _abi.HG_STATS_UPDATE_RET) == (1, 2)
    assert len(stats.EPISODE_FIELDS) == 13


def test_config_struct_is_the_headers():
    txt = open(HEADER).read()
    body = re.search(r"typedef struct hg_rollout_stats_cfg \{(.*?)\} hg_rollout_stats_cfg;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    ctype = {"double": ctypes.c_double, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
    assert [(n, ctype[t]) for t, n in decl] == list(_abi.hg_rollout_stats_cfg._fields_)
    assert [f[0] for f in _abi.hg_rollout_stats_cfg._fields_] == ["gamma", "obs_eps", "ret_eps", "max_obs_scale",
                                                                  "clip_reward", "update", "reserved"]
    assert ctypes.sizeof(_abi.hg_rollout_stats_cfg) == 40


def test_stats_object_views_and_moments():
    env = _bare_env(6)
    s = RolloutStats(env)
    assert s.state.dtype == torch.int32 and s.state.numel() * 4 == stats.stats_state_bytes(6)
    assert s.head.dtype == torch.float64 and s.head.shape == (48,) and s.head.data_ptr() == s.state.data_ptr()
    assert s.G.data_ptr() == s.state.data_ptr() + 384 and s.G.dtype == torch.float32 and s.G.shape == (6,)
    assert s.ep_ret.data_ptr() == s.state.data_ptr() + 384 + 24 and s.ep_ret.dtype == torch.float32
    assert s.ep_len.data_ptr() == s.state.data_ptr() + 384 + 48 and s.ep_len.dtype == torch.int32
    assert [tuple(x.shape) for x in (s.obs_mean, s.obs_scale, s.reward_scale, s.episode)] == [(17,), (17,), (1,), (16,)]
    assert float(s.obs_scale.min()) == 1.0 and float(s.obs_mean.abs().max()) == 0.0
    s.head[0] = 4.0
    s.head[1:18] = torch.arange(17, dtype=torch.float64)
    s.head[18:35] = 8.0
    s.head[35:42] = torch.tensor([2.0, -1.5, 5.0, 7.0, 800.0, 1.0, 3.0], dtype=torch.float64)
    m = s.moments()
    assert m["obs_count"] == 4 and np.array_equal(m["obs_mean"], np.arange(17.0)) and np.all(m["obs_var"] == 2.0)
    assert (m["ret_count"], m["ret_mean"], m["ret_var"]) == (2, -1.5, 2.5)
    assert (m["episodes"], m["env_steps"], m["skipped_rows"], m["skipped_returns"]) == (7, 800, 1, 3)
    s.G.fill_(1.0)
    assert int(s.zero_().state.abs().max()) == 0 and s.moments()["obs_count"] == 0


def test_wrapper_validates_first():
    N, K = 4, 3
    env = _bare_env(N)
    S = RolloutStats(env)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)   # noqa: E731
    u8 = torch.uint8

    def roll(**kw):
        d = dict(actions=z(K, N, 4), obs=z(K, N, 17), reward=z(K, N), terminated=z(K, N, dtype=u8),
                 truncated=z(K, N, dtype=u8), info=z(K, N, dtype=u8))
        d.update(kw)
        return d

    for key, wrong in (("obs", z(K, N, 16)), ("obs", z(K, N + 1, 17)), ("obs", z(K, N, 17, dtype=torch.float64)),
                       ("obs", z(K, N, 34)[:, :, ::2]), ("obs", z(K, N, 17).to("meta")), ("obs", np.zeros((K, N, 17))),
                       ("reward", z(K, N + 1)), ("reward", z(K, N, dtype=torch.float64)), ("reward", z(K * N)),
                       ("terminated", z(K, N, dtype=torch.bool)), ("truncated", z(K + 1, N, dtype=u8)),
                       ("info", z(K, N, dtype=torch.int8))):
        with pytest.raises(ValueError, match=key if key != "reward" else "reward"):
            env.rollout_stats(S, roll(**{key: wrong}))
    with pytest.raises(ValueError, match="RolloutStats"):
        env.rollout_stats(z(10), roll())
    with pytest.raises(ValueError, match="stats.state"):
        env.rollout_stats(RolloutStats(_bare_env(N + 1)), roll())
    with pytest.raises(ValueError, match="rollout"):
        env.rollout_stats(S, (z(K, N, 17), z(K, N)))
    with pytest.raises(ValueError, match="no 'truncated'"):
        env.rollout_stats(S, {k: v for k, v in roll().items() if k != "truncated"})
    with pytest.raises(ValueError, match="obs_in needs obs0"):
        env.rollout_stats(S, roll(), obs_in=z(K, N, 17))
    with pytest.raises(ValueError, match="obs0"):
        env.rollout_stats(S, roll(), obs0=z(N, 16), obs_in=z(K, N, 17))
    with pytest.raises(ValueError, match="obs_in"):
        env.rollout_stats(S, roll(), obs0=z(N, 17), obs_in=z(K - 1, N, 17))
    r = roll()
    with pytest.raises(ValueError, match="reward_out must not be"):
        env.rollout_stats(S, r, reward_out=r["reward"])
    with pytest.raises(ValueError, match="reward_out"):
        env.rollout_stats(S, r, reward_out=z(K, N, dtype=torch.float16))
    for kw, what in ((dict(gamma=1.5), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(gamma=float("nan")), "gamma"),
                     (dict(gamma="x"), "numbers"), (dict(obs_eps=-1e-8), "eps"), (dict(ret_eps=float("nan")), "eps"),
                     (dict(max_obs_scale=0.0), "max_obs_scale"), (dict(clip_reward=float("nan")), "clip_reward")):
        with pytest.raises(ValueError, match=what):
            env.rollout_stats(S, r, **kw)
    with pytest.raises(AssertionError, match="hg_rollout_stats"):   # valid arguments do reach the library
        env.rollout_stats(S, r, obs0=z(N, 17), obs_in=z(K, N, 17), reward_out=z(K, N), max_obs_scale=10.0, clip_reward=5.0)
    with pytest.raises(AssertionError, match="hg_rollout_stats"):   # rollout_policy's tuple
        env.rollout_stats(S, tuple(r[k] for k in ("actions", "obs", "reward", "terminated", "truncated", "info")),
                          update_obs=False, update_ret=False)


def _scalar_two_pass(obs, reward, term, trunc, info, gamma):
    """The whole history at once, env by env and value by value in Python floats (float64): moments by two
    passes, the scans per env.  Knows nothing of calls, batches or merges."""
    K, N, _ = obs.shape
    rows = [obs[k, n].astype(np.float64) for k in range(K) for n in range(N) if np.isfinite(obs[k, n]).all()]
    mean = [sum(r[c] for r in rows) / len(rows) for c in range(17)]
    m2 = [sum((r[c] - mean[c]) ** 2 for r in rows) for c in range(17)]
    g = float(np.float32(gamma))
    samples, episodes = [], []
    G_end, ret_end, len_end = [], [], []
    for n in range(N):
        G, er, el = 0.0, 0.0, 0
        for k in range(K):
            G = g * G + float(reward[k, n])
            samples.append(G)
            er += float(reward[k, n])
            el += 1
            if term[k, n] or trunc[k, n]:
                episodes.append((k, n, er, el, bool(term[k, n]), bool(info[k, n] & 2)))
                G, er, el = 0.0, 0.0, 0
        G_end.append(G), ret_end.append(er), len_end.append(el)
    rm = sum(samples) / len(samples)
    rm2 = sum((x - rm) ** 2 for x in samples)
    return dict(n=len(rows), mean=np.array(mean), m2=np.array(m2), ret_n=len(samples), ret_mean=rm, ret_m2=rm2,
                episodes=sorted(episodes), G=np.array(G_end), ep_ret=np.array(ret_end), ep_len=np.array(len_end))


def test_reference_against_a_scalar_two_pass_computation():
    rng = np.random.default_rng(11)
    K, N, split = 12, 5, 7
    obs = rng.normal(size=(K, N, 17)).astype(np.float32) * np.logspace(-2, 3, 17, dtype=np.float32)
    obs[..., 3] = (1e4 + 1e-2 * rng.normal(size=(K, N))).astype(np.float32)
    obs[..., 9] = np.float32(-3.25)
    reward = rng.normal(size=(K, N)).astype(np.float32)
    term = (rng.random((K, N)) < 0.12).astype(np.uint8)
    trunc = (rng.random((K, N)) < 0.12).astype(np.uint8)
    term[split - 1:split + 1, 2] = trunc[split - 1:split + 1, 2] = 0   # env 2's episode runs across the split
    term[split + 2, 2] = 1
    info = (term * 2 * (rng.random((K, N)) < 0.5)).astype(np.uint8)
    obs0 = rng.normal(size=(N, 17)).astype(np.float32)
    gamma = 0.9
    want = _scalar_two_pass(obs, reward, term, trunc, info, gamma)

    s1, o1 = rollout_stats_ref(None, obs[:split], reward[:split], term[:split], trunc[:split], info[:split], obs0, gamma)
    s2, o2 = rollout_stats_ref(s1, obs[split:], reward[split:], term[split:], trunc[split:], info[split:], obs[split - 1],
                               gamma, clip_reward=0.5, max_obs_scale=3.0)
    one, oa = rollout_stats_ref(None, obs, reward, term, trunc, info, obs0, gamma)
    for s in (s2, one):
        assert s["obs_count"] == want["n"] == K * N and s["ret_count"] == want["ret_n"]
        std = np.sqrt(want["m2"] / want["n"])
        assert np.all(np.abs(s["obs_mean"] - want["mean"]) <= 1e-12 * (np.abs(want["mean"]) + std))
        assert np.all(np.abs(s["obs_M2"] - want["m2"]) <= 1e-9 * want["m2"])
        assert s["obs_mean"][9] == -3.25 and s["obs_M2"][9] == 0.0   # the constant column is exact
        # G is a float32 chain in the reference: K roundings of 2^-24 relative each against the float64 chain
        tol = K * 2.0 ** -23 * max(1.0, np.abs(want["G"]).max())
        assert abs(s["ret_mean"] - want["ret_mean"]) <= tol and abs(s["ret_M2"] - want["ret_m2"]) <= 1e-5 * want["ret_m2"]
        assert np.all(np.abs(s["G"] - want["G"]) <= tol) and np.all(np.abs(s["ep_ret"] - want["ep_ret"]) <= tol)
        assert np.array_equal(s["ep_len"], want["ep_len"])
        assert s["episodes"] == len(want["episodes"]) and s["env_steps"] == K * N
        assert s["skipped_rows"] == 0 and s["skipped_returns"] == 0
    # the two calls' per-env arrays are the single call's, bitwise; an episode across the split is counted once, whole
    for k in ("G", "ep_ret", "ep_len"):
        assert np.array_equal(s2[k], one[k]), k
    assert o1["episode"][0] + o2["episode"][0] == oa["episode"][0] == len(want["episodes"])
    crossing = [e for e in want["episodes"] if e[1] == 2 and e[0] == split + 2]
    assert len(crossing) == 1 and crossing[0][3] > 3   # (longer than the second call's share of it)
    got = sorted(zip(o2["episode_lengths"].tolist(), o2["episode_returns"].tolist()))
    assert any(ln == crossing[0][3] and abs(rt - crossing[0][2]) <= 1e-5 for ln, rt in got)
    rets = np.array([e[2] for e in want["episodes"]])
    assert abs(oa["episode"][1] - rets.mean()) <= 1e-5 and abs(oa["episode"][2] - rets.std()) <= 1e-5
    assert abs(oa["episode"][3] - rets.min()) <= 1e-5 and abs(oa["episode"][4] - rets.max()) <= 1e-5
    assert abs(oa["episode"][5] - np.mean([e[3] for e in want["episodes"]])) <= 1e-6
    assert oa["episode"][6] == sum(e[4] for e in want["episodes"])
    assert oa["episode"][7] == sum(not e[4] for e in want["episodes"])
    assert oa["episode"][8] == sum(e[5] for e in want["episodes"]) and np.all(oa["episode"][10:] == 0)
    assert abs(oa["episode"][9] - reward.astype(np.float64).mean()) <= 1e-6

    # outputs: from the state after the merge
    var = s2["obs_M2"] / s2["obs_count"]
    assert np.array_equal(o2["obs_mean"], s2["obs_mean"].astype(np.float32))
    assert np.array_equal(o2["obs_scale"], np.minimum((1 / np.sqrt(var + 1e-8)).astype(np.float32), np.float32(3.0)))
    assert o2["obs_scale"][9] == 3.0 and oa["obs_scale"][9] == np.float32(1e4)   # 1 / sqrt(0 + 1e-8), clamped or not
    rs = np.float32(1 / np.sqrt(s2["ret_M2"] / s2["ret_count"] + 1e-8))
    assert o2["reward_scale"][0] == rs
    assert np.array_equal(o2["reward_out"], np.clip(reward[split:] * rs, np.float32(-0.5), np.float32(0.5)))
    assert np.abs(o2["reward_out"]).max() == 0.5
    assert np.array_equal(oa["obs_in"][0], obs0) and np.array_equal(oa["obs_in"][1:], obs[:-1])


def test_reference_skips_non_finite_and_freezes():
    rng = np.random.default_rng(5)
    K, N = 6, 3
    obs = rng.normal(size=(K, N, 17)).astype(np.float32)
    reward = rng.normal(size=(K, N)).astype(np.float32)
    term = np.zeros((K, N), np.uint8)
    term[3, 1] = 1
    trunc = np.zeros((K, N), np.uint8)
    obs[2, 0, 5] = np.inf
    reward[1, 1] = np.nan
    s, o = rollout_stats_ref(None, obs, reward, term, trunc, gamma=0.5)
    assert s["obs_count"] == K * N - 1 and s["skipped_rows"] == 1
    assert s["ret_count"] == K * N - 3 and s["skipped_returns"] == 3   # steps 1, 2, 3 of env 1
    assert np.isfinite(s["obs_mean"]).all() and np.isfinite(s["obs_M2"]).all() and np.isfinite([s["ret_mean"], s["ret_M2"]]).all()
    assert np.isfinite(s["G"]).all() and np.isfinite(s["ep_ret"]).all() and s["ep_len"][1] == 2   # recovered
    assert o["episode"][0] == 1 and o["episode"][12] == 1 and np.isnan(o["episode"][1:5]).all() and o["episode"][5] == 4
    assert o["episode"][10] == 1 and o["episode"][11] == 3 and np.isnan(o["reward_out"][1, 1])
    f, of = rollout_stats_ref(s, obs, reward, term, trunc, gamma=0.5, update_obs=False, update_ret=False)
    for k in ("obs_count", "ret_count", "ret_mean", "ret_M2", "episodes", "env_steps", "skipped_rows", "skipped_returns"):
        assert f[k] == s[k], k
    assert np.array_equal(f["obs_mean"], s["obs_mean"]) and np.array_equal(f["obs_M2"], s["obs_M2"])
    assert np.array_equal(of["obs_mean"], o["obs_mean"]) and np.array_equal(of["obs_scale"], o["obs_scale"])
    assert of["episode"][0] == 1 and f["ep_len"][0] == 2 * K and of["episode"][5] == 6   # the scans still advance
