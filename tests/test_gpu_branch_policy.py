"""GPU: policy-guided planning (hg_policy_act_mean, hg_rollout_branch_policy, PolicyMPPI).

Twin method, as test_gpu_branch_rollout.py's: handle A is the env under test and carries the policy image
WITH log_std = -1; handle B has the same N, seed, env_offset and weights WITHOUT log_std and never
auto-resets, so its step t always returns the observation step t produced.  For a checked branch b,
B.set_state(*A.get_state()) and H times policy_act_mean(obs, residual[t, b::branches], lo, hi) -> step (zeros
as eta for noise "off"); the values policy_act_mean returns on the way are V(o_0) .. V(o_H).  The expected
return, alive_steps and end_info are formed on the host from B's rewards, flags, info bits and values.

  1. policy_act_mean: the mean, the residual and the clamp, the value, the env untouched;
  2. bitwise against the stepwise twin, bootstrap off and on, value_scale in {1, 0.25, 3.7}, gamma 1 and 0.5
     (the discount a power of two: every fma an exactly rounded add of an exact product, value_scale * V one
     float32 product), over four populations;
  3. a zero policy is bitwise rollout_branch;   4. no residual is bitwise rollout_policy's return;
  5. gamma = 0.99 against a float64 recurrence;   6. a NaN observation row stays inside its env;
  7. the env untouched, pending envs, a RETRIM handle, a launch past one wave per SIMD;
  8. a whole PolicyMPPI.plan() in one graph;   9. errors that need a handle.
Run with -m gpu."""
import numpy as np
import pytest

import golden_cases as gc
from test_gpu_branch_rollout import (BRANCHES, DEV, H, N, RESET_BIT, _assert_same, _checked, _env, _return32, _trim,   # noqa: F401
                                     torch)
from test_gpu_policy_rollout import _golden_obs

pytestmark = pytest.mark.gpu

GAMMAS = (1.0, 0.5, 0.99)
BOOTS = ((False, 1.0), (True, 1.0), (True, 0.25), (True, 3.7))   # (bootstrap, value_scale)
NORTH_OUT = gc.north_out()   # ft: past the airframe's NS half-extent, so is_failed's bounds clause fires
FAILED, SUCCESSED, TIME_UP = 1, 2, 4


def _weights(torch, trim, zero=False, seed=31):
    """Random 17-64-64-4 weights with b3 = the trim action and a small W3 (zero: W3 = 0, b3 = 0), the golden
    observations' column mean and 1 / std as the input normalisation, and a value head."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g)   # noqa: E731
    W1, b1, W2, b2 = r(64, 17) / 17 ** 0.5, 0.1 * r(64), r(64, 64) / 8.0, 0.1 * r(64)
    W3, b3 = 0.02 * r(4, 64), trim.detach().cpu().clone()
    head = (r(64) / 8.0, torch.tensor([0.3]))
    if zero:
        W3, b3 = torch.zeros(4, 64), torch.zeros(4)
    o = _golden_obs().astype(np.float64)
    return dict(pairs=[(W1, b1), (W2, b2), (W3, b3)], head=head,
                obs_mean=torch.tensor(o.mean(0), dtype=torch.float32),
                obs_scale=torch.tensor(1.0 / o.std(0), dtype=torch.float32))


def _set(torch, env, w, stochastic, head=True):
    env.set_policy(w["pairs"], log_std=torch.full((4,), -1.0) if stochastic else None, obs_mean=w["obs_mean"],
                   obs_scale=w["obs_scale"])
    if head:
        env.set_value_head(w["head"])


def _pair(torch, n, task="hover", zero=False, **kw):
    """(A, B, weights): A as the caller asks, with the stochastic image; B its twin that never auto-resets."""
    A = _env(torch, n, task, **kw)
    B = _env(torch, n, task, **{**kw, "autoreset": False, "autoreset_mode": "same_step"})
    w = _weights(torch, _trim(torch, A), zero=zero)
    _set(torch, A, w, True)
    _set(torch, B, w, False)
    return A, B, w


def _age(torch, env, period=7):
    """test_gpu_branch_rollout._age_unevenly, also returning each env's observation at its age [N,17]."""
    n = env.num_envs
    env.reset()
    act = _trim(torch, env).expand(n, 4).contiguous()
    snaps, obs = [env.get_state()], [env.obs.clone()]
    for _ in range(period - 1):
        obs.append(env.step(act)[0].clone())
        snaps.append(env.get_state())
    age = torch.arange(n, device=DEV) % period
    rows = torch.arange(n, device=DEV)
    env.set_state(torch.stack([s for s, _ in snaps])[age, rows], torch.stack([c for _, c in snaps])[age, rows])
    return age.cpu().numpy(), torch.stack(obs)[age, rows].contiguous()


def _residuals(torch, n, branches, horizon, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.15 * torch.randn((horizon, n * branches, 4), generator=g)).to(DEV).contiguous()


def _bounds(torch, env):
    """Applied-action bounds tight enough around the trim action that the clamp is at work."""
    trim = _trim(torch, env).cpu().numpy()
    return (trim - np.float32(0.2)).astype(np.float32), (trim + np.float32(0.25)).astype(np.float32)


def _twin(torch, A, B, obs0, res, horizon, branches, b, noise, lo, hi):
    """B's stepwise loop of branch b from A's state.  Returns numpy: reward [H,N] float32, T [N], end_info [N],
    boot [N] bool (the row survived, or its ending step truncated without terminating it) and vboot [N]
    float32 = V(o'), o' the observation the row's last step produced."""
    B.set_state(*A.get_state())
    n, u8 = A.num_envs, torch.uint8
    eta = torch.zeros((n, 3), device=DEV) if noise == "off" else None
    obs, rows, vals = obs0, [], []
    for t in range(horizon):
        r = None if res is None else res[t, b::branches].contiguous()
        act, v = B.policy_act_mean(obs, r, lo, hi, value=True)
        obs, rew, term, trunc, _ = B.step(act, eta=eta)
        obs = obs.clone()
        rows.append((rew.clone(), term.to(u8), trunc.to(u8), B.info_u8.clone()))
        vals.append(v)
    vals.append(B.policy_act_mean(obs, value=True)[1])
    rew, term, trunc, info = (torch.stack(c).cpu().numpy() for c in zip(*rows))
    vals = torch.stack(vals).cpu().numpy()
    done = (term | trunc) != 0
    ended = done.any(0)
    first = np.where(ended, done.argmax(0), horizon - 1)
    T = np.where(ended, first + 1, horizon).astype(np.int32)
    cols = np.arange(n)
    end = np.where(ended, info[first, cols] & ~np.uint8(RESET_BIT), 0).astype(np.uint8)
    boot = ~ended | ((trunc[first, cols] != 0) & (term[first, cols] == 0))
    return rew, T, end, boot, vals[T, cols]


def _return32_boot(rew, T, gamma, boot, vboot, scale):
    """_return32 with the header's bootstrap term: after the row's last step, G = fma(disc, scale * V, G) with
    the discount after that step's multiply and scale * V one float32 product.  For gamma a power of two
    disc * x is exact, so the float32 add is the fma."""
    sv = (np.float32(scale) * vboot.astype(np.float32)).astype(np.float32)
    G, disc = np.zeros(rew.shape[1], np.float32), np.float32(1.0)
    for t in range(rew.shape[0]):
        G = np.where(t < T, (disc * rew[t] + G).astype(np.float32), G)
        disc = np.float32(disc * np.float32(gamma))
        G = np.where(boot & (T == t + 1), (disc * sv + G).astype(np.float32), G)
    return G


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


# ---------------------------------------------------------------------------------------------- 1
def test_policy_act_mean(torch):
    A, B, w = _pair(torch, N, max_episode_steps=9)
    _, obs = _age(torch, A)
    s0, c0 = A.get_state()
    lo, hi = _bounds(torch, A)
    mu = A.policy_act_mean(obs)
    _assert_same(torch, mu, B.policy_act(obs), "the stochastic image's mean against the deterministic policy_act")
    assert float((A.policy_act(obs) - mu).abs().min()) > 0   # (A's own policy_act does draw)
    res = _residuals(torch, N, 1, 1, seed=3)[0]
    got, val = A.policy_act_mean(obs, res, lo, hi, value=True)
    ref = np.clip((mu.cpu().numpy() + res.cpu().numpy()).astype(np.float32), lo, hi)
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(ref))
    clamped = (got.cpu().numpy() == lo) | (got.cpu().numpy() == hi)
    assert 0.05 < clamped.mean() < 0.95, clamped.mean()   # the clamp is at work, and not everywhere
    unclamped = A.policy_act_mean(obs, res)
    np.testing.assert_array_equal(_bits(unclamped.cpu().numpy()), _bits((mu.cpu().numpy() + res.cpu().numpy()).astype(np.float32)))
    _assert_same(torch, val, A.policy_evaluate(obs)[2], "value against policy_evaluate's")
    _assert_same(torch, A.policy_act_mean(obs, value=True)[1], val, "value with and without a residual")
    assert torch.isfinite(val).all() and float(val.std()) > 0
    out = torch.zeros((N, 4), device=DEV)
    assert A.policy_act_mean(obs, res, lo, hi, out=out) is out
    _assert_same(torch, out, got, "out=")
    A.obs.copy_(obs)   # obs=None: the env's own observations
    _assert_same(torch, A.policy_act_mean(residual=res, lo=lo, hi=hi), got, "obs=None")
    s1, c1 = A.get_state()
    _assert_same(torch, s0, s1, "state")
    _assert_same(torch, c0, c1, "counters")
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------- 2, 5
POPULATIONS = ("time_limit", "max_time", "survive", "terminated")
_cache = {}


def _case(torch, task, pop):
    """One population under both noise modes, every branch count, gamma in GAMMAS and every BOOTS entry: A's
    three outputs per call, and the twin's rows per checked branch (computed once, shared by tests 2 and 5)."""
    key = (task, pop)
    if key in _cache:
        return _cache[key]
    kw = {"time_limit": dict(max_episode_steps=9),
          # a far target: no success steps, so nothing but the clock ends these branches
          "max_time": dict(target={"sea_alt": 30000.0}), "survive": {}, "terminated": dict(max_episode_steps=9)}[pop]
    A, B, _ = _pair(torch, N, task, **kw)
    if pop == "max_time":   # time_up from step 12 on: a fresh env's branches end at their last step
        A.set_max_time(0.115)
        B.set_max_time(0.115)
    age, obs0 = _age(torch, A)
    if pop == "terminated":
        # envs 0, 3, ..: the success-step counter past its threshold (successed at the first step), those of
        # them that are multiples of 6 also one step before the TimeLimit (terminated AND truncated at once);
        # envs 1, 4, ..: north of the map (failed at the first step); envs 2, 5, ..: the TimeLimit alone
        s, c = A.get_state()
        s, c = s.clone(), c.clone()
        c[0::3, 1] = 1_000_000
        c[0::6, 0] = 8
        s[1::3, 15] = NORTH_OUT
        A.set_state(s, c)
    lo, hi = _bounds(torch, A)
    lone0 = A.debug_launches()["lone_wave"]
    calls, out = 0, {"age": age}
    for branches in BRANCHES:
        res = _residuals(torch, N, branches, H, seed=100 + branches)
        for noise in ("env", "off"):
            got = {}
            for gamma in GAMMAS:
                for boot, scale in BOOTS:
                    o = A.rollout_branch_policy(res, branches, obs0=obs0, gamma=gamma, noise=noise, lo=lo, hi=hi,
                                                bootstrap=boot, value_scale=scale)
                    calls += 1
                    got[(gamma, boot, scale)] = {k: v.cpu().numpy() for k, v in o.items()}
            twin = {b: _twin(torch, A, B, obs0, res, H, branches, b, noise, lo, hi) for b in _checked(branches)}
            out[(branches, noise)] = (got, twin)
    assert A.debug_launches()["lone_wave"] - lone0 == calls   # counted as the policy rollouts are
    A.close()
    B.close()
    _cache[key] = out
    return out


@pytest.mark.parametrize("pop", POPULATIONS)
@pytest.mark.parametrize("task", ["hover", "forward_flight"])
def test_bitwise_against_the_stepwise_twin(torch, task, pop):
    out = _case(torch, task, pop)
    age = out["age"]
    env = np.arange(N)
    for branches in BRANCHES:
        for noise in ("env", "off"):
            got, twin = out[(branches, noise)]
            for b, (rew, T, end, boot, vboot) in twin.items():
                for gamma in (1.0, 0.5):
                    plain = _return32(rew, T, gamma)
                    for bs, scale in BOOTS:
                        what = (task, pop, branches, noise, b, gamma, bs, scale)
                        g = got[(gamma, bs, scale)]
                        np.testing.assert_array_equal(g["alive_steps"][:, b], T, err_msg=str(what))
                        np.testing.assert_array_equal(g["end_info"][:, b], end, err_msg=str(what))
                        ref = _return32_boot(rew, T, gamma, boot, vboot, scale) if bs else plain
                        np.testing.assert_array_equal(_bits(g["returns"][:, b]), _bits(ref), err_msg=str(what))
                        if bs:   # the rows the rule names got V(o'), the terminated ones nothing
                            np.testing.assert_array_equal(_bits(ref[~boot]), _bits(plain[~boot]), err_msg=str(what))
                            assert (ref[boot] != plain[boot]).mean() > 0.99, what
                # the population is what it claims to be
                ended = (T < H) | (end != 0)
                if pop == "time_limit":   # TimeLimit 9, env e aged e % 7: truncated (only) at step 9 - e % 7
                    np.testing.assert_array_equal(T, 9 - age)
                    assert T.min() == 3 and T.max() == 9 and boot.all() and not end.any()
                elif pop == "max_time":   # time_up at episode step 12: the fresh ones at their last step
                    np.testing.assert_array_equal(T, H - age)
                    assert np.all(end & TIME_UP) and not np.any(end & (FAILED | SUCCESSED)) and boot.all()
                    assert (T == H).sum() >= N // 7
                elif pop == "survive":
                    assert np.all(T == H) and np.all(end == 0) and boot.all() and not ended.any()
                else:
                    su, fa, tl = env % 3 == 0, env % 3 == 1, env % 3 == 2
                    assert np.all(T[su | fa] == 1) and np.all(end[su] & SUCCESSED) and np.all(end[fa] & FAILED)
                    assert not boot[su | fa].any() and boot[tl].all() and np.all(T[tl] == 9 - age[tl]) and not end[tl].any()
                    assert su[::6].all()   # (multiples of 6: terminated and truncated by the same step)
                assert np.isfinite(rew[0]).all() and np.isfinite(vboot).all() and np.abs(vboot).min() > 0
    if pop == "survive":   # the noise modes differ, the branches of one env differ, the policy acts
        r_env, r_off = (out[(3, m)][0][(1.0, False, 1.0)]["returns"] for m in ("env", "off"))
        assert np.mean(r_env != r_off) > 0.9 and np.mean(r_env[:, 0] != r_env[:, 1]) > 0.9


@pytest.mark.parametrize("pop", POPULATIONS)
@pytest.mark.parametrize("task", ["hover", "forward_flight"])
def test_discounted_return_against_float64(torch, task, pop):
    """gamma = 0.99: |G - G64| <= 2 (H + 2) 2^-24 (sum_t gamma^t |r_t| + gamma^T |s V|) per row, G64 the
    float64 recurrence over the twin's fp32 rewards and value (disc_t carries at most t roundings, each fma
    one, the product s V one more)."""
    out = _case(torch, task, pop)
    gamma32 = float(np.float32(0.99))
    worst = 0.0
    for branches in BRANCHES:
        for noise in ("env", "off"):
            got, twin = out[(branches, noise)]
            for b, (rew, T, _, boot, vboot) in twin.items():
                live = np.arange(H)[:, None] < T[None, :]
                w = (gamma32 ** np.arange(H))[:, None] * live
                rew64 = np.where(live, rew.astype(np.float64), 0.0)   # (a dead row's rewards may be non-finite)
                for bs, scale in BOOTS:
                    tail = gamma32 ** T * float(np.float32(scale)) * vboot.astype(np.float64) * (boot & bs)
                    ref = (w * rew64).sum(0) + tail
                    bound = 2 * (H + 2) * 2.0 ** -24 * ((w * np.abs(rew64)).sum(0) + np.abs(tail))
                    g = got[(0.99, bs, scale)]
                    err = np.abs(g["returns"][:, b].astype(np.float64) - ref)
                    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                    assert np.all(err <= bound), (task, pop, branches, noise, b, bs, scale, err.max(), bound.min())
                    np.testing.assert_array_equal(g["alive_steps"][:, b], T)
    print(f"\n[gamma 0.99 {task} {pop}] max err / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("task", ["hover", "forward_flight"])
def test_zero_policy_is_bitwise_rollout_branch(torch, task):
    """W3 = 0 and b3 = 0: mu = +0, so a_t = residual[t, r] and, without clamp or bootstrap, every row of
    every launch is the open-loop kernel's."""
    A, B, _ = _pair(torch, N, task, zero=True, max_episode_steps=9)
    B.close()
    _, obs0 = _age(torch, A)
    trim = _trim(torch, A)
    for branches in BRANCHES:
        actions = (_residuals(torch, N, branches, H, seed=500 + branches) + trim).clamp_(-1.0, 1.0).contiguous()
        for noise in ("env", "off"):
            for gamma in (1.0, 0.99):
                ref = A.rollout_branch(actions, branches, gamma=gamma, noise=noise)
                got = A.rollout_branch_policy(actions, branches, obs0=obs0, gamma=gamma, noise=noise)
                for k in ref:
                    _assert_same(torch, got[k], ref[k], (task, branches, noise, gamma, k))
                assert int((ref["alive_steps"] < H).sum()) > 0 and float(ref["returns"].abs().max()) > 0
    A.close()


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("task", ["hover", "forward_flight"])
def test_no_residual_is_rollout_policy_s_return(torch, task):
    """residuals=None, one branch, no clamp: "what does this policy earn from here over the next H steps" is
    the discounted sum of the deterministic twin's rollout_policy rewards from the same state."""
    A, B, _ = _pair(torch, N, task, max_episode_steps=9)
    age, obs0 = _age(torch, A)
    B.set_state(*A.get_state())
    _, _, rew, term, trunc, info = B.rollout_policy(H, obs0=obs0)
    rew, done = rew.cpu().numpy(), ((term | trunc) != 0).cpu().numpy()
    ended = done.any(0)
    T = np.where(ended, done.argmax(0) + 1, H).astype(np.int32)
    np.testing.assert_array_equal(T, 9 - age)
    for gamma in (1.0, 0.5):
        got = A.rollout_branch_policy(None, 1, obs0=obs0, gamma=gamma, horizon=H)
        np.testing.assert_array_equal(got["alive_steps"].cpu().numpy()[:, 0], T)
        np.testing.assert_array_equal(_bits(got["returns"].cpu().numpy()[:, 0]), _bits(_return32(rew, T, gamma)))
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------- 6
def test_a_nan_observation_row_stays_inside_its_env(torch):
    """The matrix products take the wave's 64 rows as columns and rows of several envs share a wave: a NaN
    obs0 row must reach no other env's rows."""
    A, B, _ = _pair(torch, N, max_episode_steps=9)
    B.close()
    _, obs0 = _age(torch, A)
    lo, hi = _bounds(torch, A)
    bad = obs0.clone()
    bad[37] = float("nan")
    others = torch.arange(N, device=DEV) != 37
    for branches in (3, 70):
        res = _residuals(torch, N, branches, H, seed=600 + branches)
        kw = dict(gamma=0.5, lo=lo, hi=hi, bootstrap=True, value_scale=0.25)
        ref = {k: v.clone() for k, v in A.rollout_branch_policy(res, branches, obs0=obs0, **kw).items()}
        got = A.rollout_branch_policy(res, branches, obs0=bad, **kw)
        for k in ref:
            _assert_same(torch, got[k][others], ref[k][others], (branches, k))
        assert torch.isfinite(ref["returns"]).all()
        assert not torch.equal(got["returns"][37].view(torch.int32), ref["returns"][37].view(torch.int32))
    A.close()


# ---------------------------------------------------------------------------------------------- 7
def _check_against_twin(torch, A, B, obs0, res, branches, bs, got, lo, hi, rows=None, gamma=0.5, scale=0.25, horizon=H):
    rows = slice(None) if rows is None else rows
    Ts = []
    for b in bs:
        rew, T, end, boot, vboot = _twin(torch, A, B, obs0, res, horizon, branches, b, "env", lo, hi)
        np.testing.assert_array_equal(got["alive_steps"][rows, b], T[rows])
        np.testing.assert_array_equal(got["end_info"][rows, b], end[rows])
        np.testing.assert_array_equal(_bits(got["returns"][rows, b]), _bits(_return32_boot(rew, T, gamma, boot, vboot, scale)[rows]))
        Ts.append(T)
    return Ts


def test_env_is_untouched(torch):
    A, B, w = _pair(torch, N, max_episode_steps=9)
    C = _env(torch, N, max_episode_steps=9)   # a third handle that is never planned on
    _, obs0 = _age(torch, A)
    lo, hi = _bounds(torch, A)
    s0, c0 = A.get_state()
    C.set_state(s0, c0)
    launches0 = A.debug_launches()["steps"]
    for branches, noise, bs in ((3, "env", True), (70, "off", False)):
        A.rollout_branch_policy(_residuals(torch, N, branches, H, seed=7), branches, obs0=obs0, gamma=0.5, noise=noise,
                                lo=lo, hi=hi, bootstrap=bs)
    A.policy_act_mean(obs0, value=True)
    s1, c1 = A.get_state()
    _assert_same(torch, s0, s1, "state")
    _assert_same(torch, c0, c1, "counters")
    assert A.debug_launches()["steps"] == launches0
    act = (_residuals(torch, N, 1, 1, seed=8)[0] + _trim(torch, A)).contiguous()
    for k in range(4):   # ... and it steps on as its twin does (through the TimeLimit resets of the oldest)
        oa, oc = A.step(act), C.step(act)
        for name, x, y in zip(("obs", "reward", "terminated", "truncated"), oa[:4], oc[:4]):
            _assert_same(torch, x, y, (k, name))
        _assert_same(torch, A.info_u8, C.info_u8, (k, "info"))
    (sa, ca), (sc, cc) = A.get_state(), C.get_state()
    _assert_same(torch, sa, sc, "state after steps")
    _assert_same(torch, ca, cc, "counters after steps")
    for e in (A, B, C):
        e.close()


def test_next_step_pending_envs_and_a_retrim_handle(torch):
    """autoreset_mode next_step, TimeLimit 5, env e aged e % 7: age 5 has just ended (waiting for its
    reset), age 6 has been reset.  A waiting env's rows are (0, 0, 0), bootstrap or not; the others match
    the twin."""
    kw = dict(autoreset_mode="next_step", max_episode_steps=5)
    A, B, w = _pair(torch, N, **kw)
    age, obs0 = _age(torch, A)
    lo, hi = _bounds(torch, A)
    pending = A.get_state()[1].cpu().numpy()[:, 0] < 0
    np.testing.assert_array_equal(pending, age == 5)
    assert pending.any() and (~pending).any()
    results = {}
    for branches in (3, 70):
        res = _residuals(torch, N, branches, H, seed=200 + branches)
        for bs in (False, True):
            out = A.rollout_branch_policy(res, branches, obs0=obs0, gamma=0.5, lo=lo, hi=hi, bootstrap=bs, value_scale=0.25)
            got = {k: v.cpu().numpy() for k, v in out.items()}
            assert not got["returns"][pending].view(np.int32).any()   # +0.0
            assert not got["alive_steps"][pending].any() and not got["end_info"][pending].any()
        results[branches] = (res, {k: v.clone() for k, v in out.items()})
        Ts = _check_against_twin(torch, A, B, obs0, res, branches, _checked(branches), got, lo, hi, rows=~pending)
        assert all((T[~pending] < H).all() and T[~pending].min() >= 1 for T in Ts)
    # a RETRIM handle is accepted: a branch never resets, so from the same state its rows are the template handle's
    R = _env(torch, N, reset_mode="retrim", **kw)
    _set(torch, R, w, True)
    R.set_state(*A.get_state())
    s0, c0 = R.get_state()
    for branches, (res, out) in results.items():
        got = R.rollout_branch_policy(res, branches, obs0=obs0, gamma=0.5, lo=lo, hi=hi, bootstrap=True, value_scale=0.25)
        for k in out:
            _assert_same(torch, got[k], out[k], ("retrim", branches, k))
    s1, c1 = R.get_state()
    _assert_same(torch, s0, s1, "retrim state")
    _assert_same(torch, c0, c1, "retrim counters")
    for e in (A, B, R):
        e.close()


def test_a_launch_past_one_wave_per_simd(torch):
    """1 030 envs x 64 branches are 65 920 rows, just past one wave per SIMD on MI355X (65 536): the rows past
    it run as further one-wave blocks of the same launch."""
    n, branches, h = 1030, 64, 4
    A, B, _ = _pair(torch, n, max_episode_steps=9)
    age, obs0 = _age(torch, A)
    lo, hi = _bounds(torch, A)
    res = _residuals(torch, n, branches, h, seed=300)
    before = A.debug_launches()
    out = A.rollout_branch_policy(res, branches, obs0=obs0, gamma=0.5, lo=lo, hi=hi, bootstrap=True, value_scale=0.25)
    after = A.debug_launches()
    assert after["lone_wave"] - before["lone_wave"] == 1 and after["bulk"] == before["bulk"]
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for T in _check_against_twin(torch, A, B, obs0, res, branches, (0, 63), got, lo, hi, horizon=h):
        np.testing.assert_array_equal(T, np.minimum(9 - age, h))   # ages 5 and 6 end at steps 4 and 3
    A.close()
    B.close()


# ---------------------------------------------------------------------------------------------- 8
def test_graph_capture_of_a_whole_plan(torch):
    """PolicyMPPI.plan() -- sample, score with the bootstrap, update, act -- captured on one stream; two
    replays give the eager bits (the env is untouched, so every run starts from the same state)."""
    from heligym_amd import PolicyMPPI
    n, branches, h = N, 6, 8
    A, B, _ = _pair(torch, n)
    B.close()
    _, obs0 = _age(torch, A)
    lo, hi = _bounds(torch, A)
    mk = lambda: PolicyMPPI(A, h, branches, sigma=0.1, lam=0.05, res_lo=-0.3, res_hi=0.3, lo=lo, hi=hi, gamma=0.5,   # noqa: E731
                            seed=77, bootstrap=True, value_scale=0.5)
    e = mk()
    act_e = e.plan(obs0).clone()
    nom_e, sc_e, cand_e = e.nominal.clone(), {k: v.clone() for k, v in e.scores.items()}, e.actions.clone()
    assert 0 < float(nom_e.abs().max()) <= 0.3 * (1 + 2.0 ** -20)   # the update moved the residual, inside its bounds
    assert float((act_e - A.policy_act_mean(obs0, lo=lo, hi=hi)).abs().max()) > 0

    m = mk()
    m.plan(obs0)   # (allocates the score buffers)
    m.reset()
    m.samplings = 0
    start = m.nominal
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        m.plan(obs0)
    assert m.nominal is not start and not start.any()   # (the replays read the zero residual they were captured with)
    for rep in range(2):
        for x in (m.nominal, m.actions, m.action, *m.scores.values()):
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        _assert_same(torch, m.actions, cand_e, (rep, "candidates"))
        _assert_same(torch, m.nominal, nom_e, (rep, "nominal"))
        _assert_same(torch, m.action, act_e, (rep, "action"))
        for k in sc_e:
            _assert_same(torch, m.scores[k], sc_e[k], (rep, k))
    A.close()


# ---------------------------------------------------------------------------------------------- 9
def test_errors_that_need_a_handle_leave_outputs_and_env_untouched(torch):
    from heligym_amd._abi import HeliGymError
    n, branches, h = N, 3, 4
    env = _env(torch, n, max_episode_steps=9)
    _, obs0 = _age(torch, env)
    s0, c0 = env.get_state()
    res = _residuals(torch, n, branches, h, seed=9)
    mark = lambda: dict(returns=torch.full((n, branches), 7.0, device=DEV),   # noqa: E731
                        alive_steps=torch.full((n, branches), 7, dtype=torch.int32, device=DEV),
                        end_info=torch.full((n, branches), 7, dtype=torch.uint8, device=DEV))
    out, act = mark(), torch.full((n, 4), 7.0, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        for k, v in mark().items():
            _assert_same(torch, out[k], v, k)
        _assert_same(torch, act, torch.full((n, 4), 7.0, device=DEV), "actions")
        s1, c1 = env.get_state()
        _assert_same(torch, s0, s1, "state")
        _assert_same(torch, c0, c1, "counters")

    with pytest.raises(HeliGymError, match="no policy set"):
        env.rollout_branch_policy(res, branches, obs0=obs0, out=out)
    with pytest.raises(HeliGymError, match="no policy set"):
        env.policy_act_mean(obs0, out=act)
    untouched()
    w = _weights(torch, _trim(torch, env))
    _set(torch, env, w, True, head=False)
    with pytest.raises(HeliGymError, match="needs a value head"):
        env.rollout_branch_policy(res, branches, obs0=obs0, bootstrap=True, out=out)
    with pytest.raises(HeliGymError, match="needs a value head"):
        env.policy_act_mean(obs0, out=act, value=True)
    huge = -(-(2 ** 31 - 256) // n)   # N * branches >= 2^31 - 256: refused by the library, past the wrapper's shapes
    rc = env.lib.hg_rollout_branch_policy(env._h, obs0.data_ptr(), None, h, huge, 1.0, 0, None, None, 0, 1.0,
                                          out["returns"].data_ptr(), None, None, None)
    assert rc == -1 and b"N * branches" in env.lib.hg_last_error()
    with pytest.raises(ValueError):   # the wrapper refuses a wrong shape before the library sees it
        env.rollout_branch_policy(res, branches + 1, obs0=obs0, out=out)
    untouched()
    # and the good calls go through, without a value head too
    env.rollout_branch_policy(res, branches, obs0=obs0, out=out)
    env.policy_act_mean(obs0, out=act)
    torch.cuda.synchronize()
    assert torch.isfinite(out["returns"]).all() and int(out["alive_steps"].min()) >= 1 and not (act == 7.0).any()
    env.close()
