"""GPU: branched planning rollouts and the device MPPI planner (hg_rollout_branch, hg_mppi_sample,
hg_mppi_update).

Twin method: handle A is the env under test, handle B has the same config, N, seed and env_offset.  For a
checked branch b, B.set_state(*A.get_state()), B.rollout(actions[:, b::branches]) (with zeros as eta for
noise="off"), and the expected return, alive_steps and end_info are formed on the host from B's [H, N]
rewards, flags and info, cut at the first end.

  1. bitwise against hg_rollout (gamma 1 and 0.5: the discount is a power of two, each fma a
     single-rounded add of an exact product, so a NumPy float32 recurrence is bit-exact);
  2. gamma = 0.99 against a float64 recurrence over B's fp32 rewards;
  3. the env is untouched;  4. envs waiting for their next-step reset, and a RETRIM handle;
  5. the launches past one and past two waves per SIMD (the bulk variant);
  6. mppi_sample;  7. / 8. mppi_update, also at horizons past one pass of its wave (4 * horizon > 64, > 256)
     and at branch counts past the weights it keeps in LDS (> 1024);  9. graph capture;  10. errors.

A failure termination cannot be forced within 12 steps (0.12 s) by any action in [-1, 1]: from the trim at
100 ft the descent rate, the attitude limits and the ground are all out of reach in that time.  It is
covered by the flags, the reward and the info bits being computed by the very code hg_rollout runs (one
function body, csrc/heligym_amd.hip step_body), which the parity tests pin to the reference.
Run with -m gpu."""
import numpy as np
import pytest

import philox_ref as pr
from test_gpu_noise import ETA_ABS, ETA_REL

pytestmark = pytest.mark.gpu

H = 12
N = 130                       # three state tiles, the last one ragged
BRANCHES = (1, 3, 64, 70)     # waves inside one env, spanning several envs, straddling tiles
SEED = 0x5EED_7E4B_0000_0031
RESET_BIT = 16
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def _env(torch, n, task="hover", **kw):
    from heligym_amd import HeliVecEnv
    kw.setdefault("seed", SEED)
    kw.setdefault("autoreset", True)
    return HeliVecEnv(n, task=task, dt=0.01, device=DEV, **kw)


def _assert_same(torch, a, b, what):
    """Equal as integer views: NaNs and signed zeros count."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), what


def _trim(torch, env):
    return torch.as_tensor(np.asarray(env.template()["action"], dtype=np.float32), device=DEV)


def _age_unevenly(torch, env, period=7):
    """Env e stepped e % period times at its trim action from a reset (the others' later steps undone by
    set_state of the snapshot taken at their age).  Returns the ages [N] (numpy)."""
    n = env.num_envs
    env.reset()
    act = _trim(torch, env).expand(n, 4).contiguous()
    snaps = [env.get_state()]
    for _ in range(period - 1):
        env.step(act)
        snaps.append(env.get_state())
    age = torch.arange(n, device=DEV) % period
    rows = torch.arange(n, device=DEV)
    env.set_state(torch.stack([s for s, _ in snaps])[age, rows], torch.stack([c for _, c in snaps])[age, rows])
    return age.cpu().numpy()


def _candidates(torch, env, branches, horizon, seed):
    """[horizon, N*branches, 4]: the trim action plus 0.2 randn, clipped to [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    a = 0.2 * torch.randn((horizon, env.num_envs * branches, 4), generator=g)
    return (a.to(DEV) + _trim(torch, env)).clamp_(-1.0, 1.0).contiguous()


def _checked(branches):
    return list(range(branches)) if branches <= 3 else [0, 1, 63, branches - 1]


def _twin(torch, A, B, actions, branches, b, noise):
    """B's rollout of branch b from A's state: (reward [H,N] float32, T [N], end_info [N]) as numpy."""
    B.set_state(*A.get_state())
    h, n = actions.shape[0], A.num_envs
    eta = torch.zeros((h, n, 3), device=DEV) if noise == "off" else None
    _, rew, term, trunc, info = B.rollout(actions[:, b::branches].contiguous(), eta=eta)
    done = (term | trunc).cpu().numpy() != 0
    ended = done.any(0)
    first = np.where(ended, done.argmax(0), h - 1)
    T = np.where(ended, first + 1, h).astype(np.int32)
    end = np.where(ended, info.cpu().numpy()[first, np.arange(n)] & ~np.uint8(RESET_BIT), 0).astype(np.uint8)
    return rew.cpu().numpy(), T, end


def _return32(rew, T, gamma):
    """The header's recurrence in float32: G = fma(disc, r_t, G), disc *= gamma, over t < T.  For gamma a
    power of two disc * r_t is exact, so the float32 add is the fma."""
    G, disc = np.zeros(rew.shape[1], np.float32), np.float32(1.0)
    for t in range(rew.shape[0]):
        G = np.where(t < T, (disc * rew[t] + G).astype(np.float32), G)
        disc = np.float32(disc * np.float32(gamma))
    return G


POPULATIONS = ("time_limit", "max_time", "survive")
_cache = {}


def _case(torch, task, pop):
    """One population under both noise modes, every branch count and gamma in {1, 0.5, 0.99}: A's three
    outputs per call, and the twin's rewards / T / end_info per checked branch (computed once, shared by
    tests 1 and 2)."""
    key = (task, pop)
    if key in _cache:
        return _cache[key]
    kw = {"time_limit": dict(max_episode_steps=9),
          # a far target: no success steps, so nothing but the clock ends these branches
          "max_time": dict(target={"sea_alt": 30000.0}), "survive": {}}[pop]
    A, B = _env(torch, N, task, **kw), _env(torch, N, task, **kw)
    if pop == "max_time":   # time_up from step 12 on: a fresh env's branches end at their last step
        A.set_max_time(0.115)
        B.set_max_time(0.115)
    age = _age_unevenly(torch, A)
    lone0 = A.debug_launches()["lone_wave"]
    calls, res = 0, {"age": age}
    for branches in BRANCHES:
        actions = _candidates(torch, A, branches, H, seed=100 + branches)
        for noise in ("env", "off"):
            got = {}
            for gamma in (1.0, 0.5, 0.99):
                out = A.rollout_branch(actions, branches, gamma=gamma, noise=noise)
                calls += 1
                got[gamma] = {k: v.cpu().numpy() for k, v in out.items()}
            twin = {b: _twin(torch, A, B, actions, branches, b, noise) for b in _checked(branches)}
            res[(branches, noise)] = (got, twin)
    assert A.debug_launches()["lone_wave"] - lone0 == calls   # these sizes: the lone-wave variant
    A.close()
    B.close()
    _cache[key] = res
    return res


@pytest.mark.parametrize("pop", POPULATIONS)
@pytest.mark.parametrize("task", ["hover", "forward_flight"])
def test_bitwise_against_rollout(torch, task, pop):
    res = _case(torch, task, pop)
    age = res["age"]
    for branches in BRANCHES:
        for noise in ("env", "off"):
            got, twin = res[(branches, noise)]
            for b, (rew, T, end) in twin.items():
                for gamma in (1.0, 0.5):
                    what = (task, pop, branches, noise, b, gamma)
                    g = got[gamma]
                    np.testing.assert_array_equal(g["alive_steps"][:, b], T, err_msg=str(what))
                    np.testing.assert_array_equal(g["end_info"][:, b], end, err_msg=str(what))
                    np.testing.assert_array_equal(g["returns"][:, b].view(np.int32), _return32(rew, T, gamma).view(np.int32),
                                                  err_msg=str(what))
                # the population is what it claims to be
                if pop == "time_limit":   # TimeLimit 9, env e aged e % 7: ends at step 9 - e % 7, from 3 to 9
                    np.testing.assert_array_equal(T, 9 - age)
                    assert T.min() == 3 and T.max() == 9
                elif pop == "max_time":   # time_up at episode step 12: ends at 12 - age, the fresh ones at the last step
                    np.testing.assert_array_equal(T, H - age)
                    assert np.all(end & 4) and (T == H).sum() >= N // 7
                else:
                    assert np.all(T == H) and np.all(end == 0)
                assert np.isfinite(rew).all() and (task == "heli" or np.abs(rew).max() > 0)
    if pop == "survive":   # the two noise modes differ, and so do the branches of one env
        r_env, r_off = res[(3, "env")][0][1.0]["returns"], res[(3, "off")][0][1.0]["returns"]
        assert np.mean(r_env != r_off) > 0.9 and np.mean(r_env[:, 0] != r_env[:, 1]) > 0.9


@pytest.mark.parametrize("pop", POPULATIONS)
@pytest.mark.parametrize("task", ["hover", "forward_flight"])
def test_discounted_return_against_float64(torch, task, pop):
    """gamma = 0.99: |G - G64| <= 2 (H + 1) 2^-24 sum_t gamma^t |r_t| per row, G64 the float64 recurrence
    over the twin's fp32 rewards (disc_t carries at most t roundings, each fma one)."""
    res = _case(torch, task, pop)
    gamma32 = float(np.float32(0.99))
    worst = 0.0
    for branches in BRANCHES:
        for noise in ("env", "off"):
            got, twin = res[(branches, noise)]
            for b, (rew, T, _) in twin.items():
                live = np.arange(H)[:, None] < T[None, :]
                w = (gamma32 ** np.arange(H))[:, None] * live
                ref = (w * rew.astype(np.float64)).sum(0)
                bound = 2 * (H + 1) * 2.0 ** -24 * (w * np.abs(rew.astype(np.float64))).sum(0)
                err = np.abs(got[0.99]["returns"][:, b].astype(np.float64) - ref)
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                assert np.all(err <= bound), (task, pop, branches, noise, b, err.max(), bound.min())
                np.testing.assert_array_equal(got[0.99]["alive_steps"][:, b], T)
    print(f"\n[gamma 0.99 {task} {pop}] max err / bound {worst:.3f}")


def test_env_is_untouched(torch):
    A, B = _env(torch, N, max_episode_steps=9), _env(torch, N, max_episode_steps=9)
    _age_unevenly(torch, A)
    s0, c0 = A.get_state()
    B.set_state(s0, c0)
    launches0 = A.debug_launches()["steps"]
    for branches, noise in ((3, "env"), (70, "off")):
        A.rollout_branch(_candidates(torch, A, branches, H, seed=7), branches, gamma=0.5, noise=noise)
    s1, c1 = A.get_state()
    _assert_same(torch, s0, s1, "state")
    _assert_same(torch, c0, c1, "counters")
    assert A.debug_launches()["steps"] == launches0
    act = _candidates(torch, A, 1, 1, seed=8)[0]
    for k in range(4):   # ... and it steps on as its twin does (through the TimeLimit resets of the oldest)
        oa, ob = A.step(act), B.step(act)
        for name, x, y in zip(("obs", "reward", "terminated", "truncated"), oa[:4], ob[:4]):
            _assert_same(torch, x, y, (k, name))
        _assert_same(torch, A.info_u8, B.info_u8, (k, "info"))
    (sa, ca), (sb, cb) = A.get_state(), B.get_state()
    _assert_same(torch, sa, sb, "state after steps")
    _assert_same(torch, ca, cb, "counters after steps")
    A.close()
    B.close()


def test_next_step_pending_envs_and_a_retrim_handle(torch):
    """autoreset_mode next_step, TimeLimit 5, env e aged e % 7: age 5 has just ended (waiting for its
    reset), age 6 has been reset.  A waiting env's rows are (0, 0, 0); the others match the twin."""
    kw = dict(autoreset_mode="next_step", max_episode_steps=5)
    A, B = _env(torch, N, **kw), _env(torch, N, **kw)
    age = _age_unevenly(torch, A)
    ctr = A.get_state()[1].cpu().numpy()
    pending = ctr[:, 0] < 0
    np.testing.assert_array_equal(pending, age == 5)
    assert pending.any() and (~pending).any()
    results = {}
    for branches in (3, 70):
        actions = _candidates(torch, A, branches, H, seed=200 + branches)
        out = A.rollout_branch(actions, branches, gamma=0.5)
        results[branches] = (actions, out)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert not got["returns"][pending].view(np.int32).any()   # +0.0
        assert not got["alive_steps"][pending].any() and not got["end_info"][pending].any()
        for b in _checked(branches):
            rew, T, end = _twin(torch, A, B, actions, branches, b, "env")
            live = ~pending
            np.testing.assert_array_equal(got["alive_steps"][live, b], T[live])
            np.testing.assert_array_equal(got["end_info"][live, b], end[live])
            np.testing.assert_array_equal(got["returns"][live, b].view(np.int32), _return32(rew, T, 0.5)[live].view(np.int32))
            assert (T[live] < H).all() and T[live].min() >= 1
    # a RETRIM handle (whose auto-resets hg_rollout refuses) is accepted: a branch never resets, so from the
    # same state its rows are bitwise the template handle's
    R = _env(torch, N, reset_mode="retrim", **kw)
    R.set_state(*A.get_state())
    s0, c0 = R.get_state()
    for branches, (actions, out) in results.items():
        got = R.rollout_branch(actions, branches, gamma=0.5)
        for k in out:
            _assert_same(torch, got[k], out[k], ("retrim", branches, k))
    s1, c1 = R.get_state()
    _assert_same(torch, s0, s1, "retrim state")
    _assert_same(torch, c0, c1, "retrim counters")
    for e in (A, B, R):
        e.close()


@pytest.mark.parametrize("n,kind", [(1030, "lone_wave"), (2050, "bulk")])
def test_larger_launches(torch, n, kind):
    """x 64 branches: 1 030 envs are 65 920 rows, just past one wave per SIMD on MI355X (65 536), where the
    lone-wave kernel bound to two waves per SIMD takes over; 2 050 envs are 131 200 rows, just past two
    waves per SIMD (131 072): the bulk variant."""
    branches, h = 64, 4
    A, B = _env(torch, n, max_episode_steps=9), _env(torch, n, max_episode_steps=9)
    age = _age_unevenly(torch, A)
    actions = _candidates(torch, A, branches, h, seed=300)
    before = A.debug_launches()
    out = A.rollout_branch(actions, branches, gamma=0.5)
    after = A.debug_launches()
    other = "bulk" if kind == "lone_wave" else "lone_wave"
    assert after[kind] - before[kind] == 1 and after[other] == before[other]
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for b in (0, 63):
        rew, T, end = _twin(torch, A, B, actions, branches, b, "env")
        np.testing.assert_array_equal(got["alive_steps"][:, b], T)
        np.testing.assert_array_equal(got["end_info"][:, b], end)
        np.testing.assert_array_equal(got["returns"][:, b].view(np.int32), _return32(rew, T, 0.5).view(np.int32))
        np.testing.assert_array_equal(T, np.minimum(9 - age, h))   # ages 5 and 6 end at steps 4 and 3
    A.close()
    B.close()


def _z_ref(gid, t, b, seed):
    """include/heligym_amd.h: one Philox4x32-10 call on (gid_lo, gid_hi, t, b) keyed (seed_lo, seed_hi),
    float64 Box-Muller of the four words as the policy noise's."""
    r = pr.noise_words(gid, t, b, seed)
    r0, r1 = np.sqrt(-2.0 * np.log(pr.u01(r[:, 0]))), np.sqrt(-2.0 * np.log(pr.u01(r[:, 2])))
    a1, a3 = 2 * np.pi * pr.turn_frac(r[:, 1]), 2 * np.pi * pr.turn_frac(r[:, 3])
    return np.stack([r0 * np.cos(a1), r0 * np.sin(a1), r1 * np.cos(a3), r1 * np.sin(a3)], axis=1)


def test_mppi_sample(torch):
    n, branches, h, off, seed = 70, 5, 3, (1 << 33) + 5, 0x1234_5678_9ABC_DEF1
    sigma, lo, hi = np.float32([0.3, 0.2, 0.1, 0.05]), np.float32([-0.5, -0.4, -0.5, -0.25]), np.float32([0.5, 0.4, 0.3, 0.5])
    env = _env(torch, n, env_offset=off)
    g = torch.Generator().manual_seed(11)
    nominal = (1.2 * torch.rand((h, n, 4), generator=g) - 0.6).to(DEV)
    out = env.mppi_sample(nominal, branches, sigma, lo, hi, seed)
    got = out.cpu().numpy().reshape(h, n, branches, 4)
    nom = nominal.cpu().numpy()
    clamped = np.minimum(np.maximum(nom, lo), hi)
    assert (clamped != nom).mean() > 0.05   # the clamp is at work
    np.testing.assert_array_equal(got[:, :, 0].view(np.int32), clamped.view(np.int32))   # branch 0: clamp(nominal)
    assert np.all(got >= lo) and np.all(got <= hi)
    tt, ee, bb = np.meshgrid(np.arange(h), np.arange(n), np.arange(branches), indexing="ij")
    z = _z_ref(off + ee.ravel(), tt.ravel(), bb.ravel(), seed).reshape(h, n, branches, 4)
    ref = np.clip(nom[:, :, None, :].astype(np.float64) + sigma.astype(np.float64) * z, lo, hi)
    tol = sigma * (ETA_ABS + ETA_REL * np.abs(z)) + 2.0 ** -23 * np.abs(ref)
    err = np.abs(got[:, :, 1:].astype(np.float64) - ref[:, :, 1:])
    print(f"\n[mppi_sample] max |d| {err.max():.3e}, max |d| / tol {(err / tol[:, :, 1:]).max():.3f}")
    assert np.all(err <= tol[:, :, 1:])
    inner = (got[:, :, 1:] > lo) & (got[:, :, 1:] < hi)
    assert inner.mean() > 0.5 and np.abs(got[:, :, 1:] - clamped[:, :, None, :])[inner].std() > 0.02   # perturbed
    part = _env(torch, 32, env_offset=off + 32)   # envs 32..63 of the population held by another handle
    sub = part.mppi_sample(nominal[:, 32:64].contiguous(), branches, sigma, lo, hi, seed).cpu().numpy()
    np.testing.assert_array_equal(sub.reshape(h, 32, branches, 4).view(np.int32), got[:, 32:64].view(np.int32))
    env.close()
    part.close()


def test_mppi_update_one_hot_limit(torch):
    n, branches = N, 70
    env = _env(torch, n)
    env.reset()
    nominal = _trim(torch, env).expand(H, n, 4).contiguous()
    actions = env.mppi_sample(nominal, branches, 0.2, -1.0, 1.0, seed=5)
    G = env.rollout_branch(actions, branches, gamma=1.0)["returns"]
    g = G.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    gaps = g.max(1, keepdims=True) - g
    best = g.argmax(1)
    runner_up = np.sort(gaps, axis=1)[:, 1]
    assert runner_up.min() > 0   # one best branch per env
    lam = float(runner_up.min()) / 400.0
    assert (runner_up / lam).min() > 200   # every weight but the best underflows
    out = env.mppi_update(actions, G, lam)
    pick = actions.view(H, n, branches, 4)[:, torch.arange(n, device=DEV), torch.as_tensor(best, device=DEV)]
    _assert_same(torch, out, pick.contiguous(), "one-hot nominal")
    again = env.rollout_branch(out, 1, gamma=1.0)["returns"]   # another lane, another branch count: the same number
    _assert_same(torch, again[:, 0], G.max(1).values, "re-scored G_max")
    env.close()


def _update_ref(actions, G, lam, dtype):
    """The header's update in `dtype`, sums over b ascending (float32: each line one rounding, the fma
    formed in float64 and rounded once)."""
    h, rows, _ = actions.shape
    n, branches = G.shape
    a = actions.reshape(h, n, branches, 4).astype(dtype)
    fin = np.isfinite(G)
    gmax = np.where(fin, G, -np.inf).max(1, keepdims=True).astype(dtype)
    k = dtype(1.4426950408889634 / lam)
    with np.errstate(invalid="ignore"):
        x = ((G.astype(dtype) - gmax) * k).astype(dtype)
        w = np.where(fin, np.exp2(x), 0).astype(dtype)
    num, den = np.zeros((h, n, 4), dtype), np.zeros((n,), dtype)
    for b in range(branches):
        num = (w[None, :, b, None].astype(np.float64) * a[:, :, b].astype(np.float64) + num.astype(np.float64)).astype(dtype)
        den = (den + w[:, b]).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (num / den[None, :, None]).astype(dtype)
    return np.where(fin.any(1)[None, :, None], out, a[:, :, 0])


@pytest.mark.parametrize("branches", [3, 70])
def test_mppi_update_general_case(torch, branches):
    """Gaps (G_max - G_b) / lambda <= 20.  Against float64 the kernel's error may be at most 4x that of
    the float32 NumPy restatement in the stated order on the same rows (the margin
    test_policy_values_against_float64 uses for the hardware exp2)."""
    n, h, lam = N, 5, 0.5
    rng = np.random.RandomState(branches)
    G = (3.0 - 10.0 * rng.rand(n, branches)).astype(np.float32)
    acts = rng.uniform(-1, 1, size=(h, n * branches, 4)).astype(np.float32)
    a4 = acts.reshape(h, n, branches, 4)
    G[5, 1] = np.nan            # a NaN return weighs nothing
    G[9, 0] = np.inf            # nor an infinite one
    G[6, :] = np.nan            # no finite return: branch 0's rows
    G[100], a4[:, 100] = G[7], a4[:, 7]   # env 7's data again at env 100
    fin = np.isfinite(G)
    gaps = np.where(fin, np.where(fin, G, -np.inf).max(1, keepdims=True) - G, 0) / lam
    assert gaps.max() <= 20 and gaps.max() > 15
    env = _env(torch, n)
    got32 = env.mppi_update(torch.as_tensor(acts, device=DEV), torch.as_tensor(G, device=DEV), lam).cpu().numpy()
    env.close()
    ref = _update_ref(acts, G, lam, np.float64)
    r32 = _update_ref(acts, G, lam, np.float32)
    some = fin.any(1)
    err = np.abs(got32.astype(np.float64) - ref)[:, some].max()
    err32 = np.abs(r32.astype(np.float64) - ref)[:, some].max()
    print(f"\n[mppi_update B={branches}] kernel max|d| {err:.3e}, float32 NumPy max|d| {err32:.3e}, ratio {err / err32:.2f} (bound 4)")
    assert np.isfinite(got32).all() and err32 > 0
    assert err <= 4 * err32
    np.testing.assert_array_equal(got32[:, 6].view(np.int32), a4[:, 6, 0].view(np.int32))       # all-NaN env: branch 0
    np.testing.assert_array_equal(got32[:, 7].view(np.int32), got32[:, 100].view(np.int32))     # place-independent
    # the NaN branch's actions do not enter: replacing them changes nothing
    a4[:, 5, 1] = 1e30
    env = _env(torch, n)
    again = env.mppi_update(torch.as_tensor(acts, device=DEV), torch.as_tensor(G, device=DEV), lam).cpu().numpy()
    env.close()
    np.testing.assert_array_equal(again[:, 5].view(np.int32), got32[:, 5].view(np.int32))


def _update_inputs(seed, n, branches, h, lam):
    """Returns and candidates drawn as test_mppi_update_general_case draws them, every return finite."""
    rng = np.random.RandomState(seed)
    G = (3.0 - 10.0 * rng.rand(n, branches)).astype(np.float32)
    acts = rng.uniform(-1, 1, size=(h, n * branches, 4)).astype(np.float32)
    assert ((G.max(1, keepdims=True) - G) / lam).max() <= 20   # no weight underflows
    return G, acts


def _update_values(torch, env, what, acts, G, lam):
    """The kernel's result, checked against float64 with test_mppi_update_general_case's yardstick over the envs
    that have a finite return."""
    fin = np.isfinite(G)
    gaps = np.where(fin, np.where(fin, G, -np.inf).max(1, keepdims=True) - G, 0) / lam
    assert gaps.max() <= 20
    got32 = env.mppi_update(torch.as_tensor(acts, device=DEV), torch.as_tensor(G, device=DEV), lam).cpu().numpy()
    ref = _update_ref(acts, G, lam, np.float64)
    r32 = _update_ref(acts, G, lam, np.float32)
    some = fin.any(1)
    err = np.abs(got32.astype(np.float64) - ref)[:, some].max()
    err32 = np.abs(r32.astype(np.float64) - ref)[:, some].max()
    print(f"\n[mppi_update {what}] kernel max|d| {err:.3e}, float32 NumPy max|d| {err32:.3e}, ratio {err / err32:.2f} (bound 4)")
    assert np.isfinite(got32).all() and err32 > 0
    assert err <= 4 * err32
    return got32


# The update kernel's lane owns the elements j0, j0 + 64, j0 + 128, j0 + 192 (q = 0 .. 3) of the env's
# nel = 4 * horizon and starts again at j0 + 256; a chain past the end reads element j0 once more and is not stored.
#   horizon  nel
#     16      64   one pass, q = 0 alone, every lane live
#     17      68   q = 1 has 4 live lanes, 60 padded ones beside them
#     30     120   examples/mppi_hover.py's default: q = 1 with 56 live lanes
#     64     256   all four chains full, one trip
#     65     260   a second trip of 4 lanes (q = 0 only)
#    100     400   a second trip with q = 0, 1 full and q = 2 with 16 lanes
@pytest.mark.parametrize("h", [16, 17, 30, 64, 65, 100])
def test_mppi_update_past_one_pass_of_the_wave(torch, h):
    """Values; and every row t of the result is bitwise the horizon-1 call (nel = 4: lanes 0-3, q = 0, one trip)
    on that step's candidates, whatever lane, chain and trip the longer call gave it."""
    n, branches, lam = 3, 7, 0.5   # (one wave per env: the kernel does not depend on N)
    G, acts = _update_inputs(100 + h, n, branches, h, lam)
    env = _env(torch, n)
    got = _update_values(torch, env, f"H={h} B={branches}", acts, G, lam)
    a, g = torch.as_tensor(acts, device=DEV), torch.as_tensor(G, device=DEV)
    rows = torch.cat([env.mppi_update(a[t:t + 1], g, lam) for t in range(h)])
    env.close()
    np.testing.assert_array_equal(rows.cpu().numpy().view(np.int32), got.view(np.int32))


# Past HG_MPPI_LDS_BRANCHES = 1024 the weights are recomputed per element in place of read from LDS:
# 1024 is the last size that keeps them, 1025 the first that does not, 1100 = 17 * 64 + 12 a ragged one.
@pytest.mark.parametrize("branches", [1024, 1025, 1100])
def test_mppi_update_past_the_lds_weights(torch, branches):
    n, h, lam = 3, 5, 0.5
    G, acts = _update_inputs(branches, n, branches, h, lam)
    a4 = acts.reshape(h, n, branches, 4)
    if branches == 1025:
        G[1, :] = np.nan       # no finite return: branch 0's rows
        G[2, 513] = np.nan     # a NaN return weighs nothing
    env = _env(torch, n)
    got = _update_values(torch, env, f"H={h} B={branches}", acts, G, lam)
    if branches == 1025:
        np.testing.assert_array_equal(got[:, 1].view(np.int32), a4[:, 1, 0].view(np.int32))
        a4[:, 2, 513] = 1e30   # the NaN branch's actions do not enter: replacing them changes nothing
        again = env.mppi_update(torch.as_tensor(acts, device=DEV), torch.as_tensor(G, device=DEV), lam).cpu().numpy()
        np.testing.assert_array_equal(again.view(np.int32), got.view(np.int32))
    env.close()


def test_mppi_update_recomputed_weights_are_bitwise_the_lds_ones(torch):
    """1024 branches (weights from LDS) against the same with a 1025th branch whose return is NaN (weights
    recomputed): each element's chain runs over b ascending, the last branch weighs 0 and fma(0, a, num) = num
    for a finite a and a non-zero num, so the bits are the same."""
    n, h, lam, branches = 3, 5, 0.5, 1024
    G, acts = _update_inputs(branches, n, branches, h, lam)
    a4 = acts.reshape(h, n, branches, 4)
    # no partial sum of a chain is zero (float64, b ascending)
    w = np.exp2((G.astype(np.float64) - G.max(1, keepdims=True)) * (1.4426950408889634 / lam))
    assert (np.cumsum(w[None, :, :, None] * a4, axis=2) != 0).all()
    extra = np.random.RandomState(7).uniform(-1, 1, size=(h, n, 1, 4)).astype(np.float32)
    acts1 = np.ascontiguousarray(np.concatenate([a4, extra], axis=2).reshape(h, n * (branches + 1), 4))
    G1 = np.concatenate([G, np.full((n, 1), np.nan, np.float32)], axis=1)
    env = _env(torch, n)
    lds = env.mppi_update(torch.as_tensor(acts, device=DEV), torch.as_tensor(G, device=DEV), lam)
    rec = env.mppi_update(torch.as_tensor(acts1, device=DEV), torch.as_tensor(G1, device=DEV), lam)
    _assert_same(torch, rec, lds, "1025 branches, the last one NaN, against 1024")
    env.close()


def test_graph_capture(torch):
    """sample -> branch -> update captured on one stream; two replays equal the eager result bitwise (the
    env is untouched, so every run starts from the same state)."""
    n, branches, h = N, 6, 8
    env = _env(torch, n)
    env.reset()
    nominal = _trim(torch, env).expand(h, n, 4).contiguous()

    def plan(bufs=None):
        acts = env.mppi_sample(nominal, branches, 0.15, -1.0, 1.0, seed=77, out=None if bufs is None else bufs[0])
        sc = env.rollout_branch(acts, branches, gamma=0.5, out=None if bufs is None else bufs[1])
        new = env.mppi_update(acts, sc["returns"], 0.01, out=None if bufs is None else bufs[2])
        return acts, sc, new

    eager = plan()
    bufs = tuple(torch.zeros_like(x) if torch.is_tensor(x) else {k: torch.zeros_like(v) for k, v in x.items()}
                 for x in eager)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan(bufs)
    for rep in range(2):
        for x in (bufs[0], bufs[2], *bufs[1].values()):
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        _assert_same(torch, bufs[0], eager[0], (rep, "actions"))
        _assert_same(torch, bufs[2], eager[2], (rep, "nominal"))
        for k in eager[1]:
            _assert_same(torch, bufs[1][k], eager[1][k], (rep, k))
    assert float((eager[2] - nominal).abs().max()) > 0   # the update moved the nominal
    env.close()


def test_errors_leave_the_env_untouched(torch):
    from heligym_amd._abi import HeliGymError, check
    import ctypes
    n, branches, h = N, 3, 4
    env = _env(torch, n, max_episode_steps=9)
    _age_unevenly(torch, env)
    lib, hnd = env.lib, env._h
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)   # noqa: E731
    acts, ret, nom = f32(h, n * branches, 4), f32(n * branches), f32(h, n, 4)
    odd = f32(h * n * branches * 4 + 4)[1:]   # 4 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 4
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    F4 = ctypes.c_float * 4
    one, neg = F4(1, 1, 1, 1), F4(-1, -1, -1, -1)
    huge = -(-(2 ** 31 - 256) // n)   # N * branches >= 2^31 - 256
    assert n * huge >= 2 ** 31 - 256 > n * (huge - 1)

    def branch(actions=acts, horizon=h, b=branches, gamma=1.0, noise=0, out=ret):
        return lambda: lib.hg_rollout_branch(hnd, None if actions is None else P(actions), horizon, b, gamma, noise,
                                             None if out is None else P(out), None, None, None)

    def update(lam=1.0, out=nom, horizon=h, b=branches):
        return lambda: lib.hg_mppi_update(hnd, P(acts), P(ret), horizon, b, lam, P(out), None)

    def sample(sigma=one, lo=neg, hi=one, horizon=h, b=branches, out=acts):
        return lambda: lib.hg_mppi_sample(hnd, P(nom), horizon, b, sigma, lo, hi, 1, P(out), None)

    bad = [branch(horizon=0), branch(b=0), branch(b=huge), branch(gamma=0.0), branch(gamma=1.5), branch(gamma=float("nan")),
           branch(gamma=float("inf")), branch(noise=2), branch(noise=-1), branch(actions=None), branch(out=None),
           branch(actions=odd), update(lam=0.0), update(lam=-1.0), update(lam=float("nan")), update(out=acts),
           update(horizon=0), update(b=huge), sample(sigma=F4(1, 1, -1, 1)), sample(lo=one, hi=neg), sample(horizon=0),
           sample(b=0), sample(b=huge), sample(out=odd)]
    s0, c0 = env.get_state()
    for j, call in enumerate(bad):
        with pytest.raises(HeliGymError, match="error -1"):
            check(call(), lib)
    with pytest.raises(ValueError):   # the wrapper refuses a wrong shape before the library sees it
        env.rollout_branch(acts, branches + 1)
    torch.cuda.synchronize()
    s1, c1 = env.get_state()
    _assert_same(torch, s0, s1, "state")
    _assert_same(torch, c0, c1, "counters")
    assert check(branch()(), lib) == 0   # and the good call goes through
    torch.cuda.synchronize()
    env.close()
