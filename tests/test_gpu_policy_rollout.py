"""GPU: closed-loop policy rollouts (hg_set_policy, hg_policy_act, hg_rollout_policy).

  1. the fused rollout is bitwise the stepwise loop policy_act -> step (the path the parity tests pin
     to the reference), through TimeLimit resets, both auto-reset modes, injected noise and per-env
     reset templates;
  2. with zero weights and a constant action it is bitwise the open-loop rollout();
  3. the policy's values against a float64 forward pass, measured against a float32 NumPy one;
  4. the action noise against a host restatement written from the header's key layout, its separation
     from the turbulence stream and its independence of sharding;
  5. set_policy + rollout_policy captured into one graph;
  6. argument errors leave the env untouched.
Run with -m gpu."""
import numpy as np
import pytest

import philox_ref as pr
from conftest import load_golden
from test_gpu_noise import ETA_ABS, ETA_REL

pytestmark = pytest.mark.gpu

K = 12
SEED = 0x5EED_7E4B_0000_0029
KEY0, KEY1 = 0x706F6C69, 0x63795F7A   # include/heligym_amd.h: the action noise's key constants


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
    kw.setdefault("max_episode_steps", 5)
    return HeliVecEnv(n, task=task, dt=0.01, device="cuda:0", **kw)


def _golden_obs():
    d = load_golden("traj_dt0.01.npz")
    return np.concatenate([d[f"{n}/obs"] for n in ("hover_random", "forward80", "alt1500_medium")]).astype(np.float32)


@pytest.fixture(scope="module")
def policy(torch):
    """torch's default Linear init under a fixed seed; obs_mean / obs_scale the golden observations'
    column mean and 1 / std; log_std around -1."""
    nn = torch.nn
    torch.manual_seed(20)
    m = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
    o = _golden_obs().astype(np.float64)
    return dict(model=m, log_std=torch.tensor([-1.0, -0.7, -1.3, -0.9]),
                obs_mean=torch.tensor(o.mean(0), dtype=torch.float32),
                obs_scale=torch.tensor(1.0 / o.std(0), dtype=torch.float32))


def _set(env, policy, stochastic=True):
    env.set_policy(policy["model"], log_std=policy["log_std"] if stochastic else None,
                   obs_mean=policy["obs_mean"], obs_scale=policy["obs_scale"])


def _on_device(policy):
    """The same policy as (W, b) pairs and vectors already on the GPU (nothing to copy in set_policy)."""
    m = policy["model"]
    to = lambda t: t.detach().to("cuda:0")   # noqa: E731
    return dict(model=[(to(l.weight), to(l.bias)) for l in (m[0], m[2], m[4])], log_std=to(policy["log_std"]),
                obs_mean=to(policy["obs_mean"]), obs_scale=to(policy["obs_scale"]))


def _assert_same(torch, a, b, what):
    """Equal as integer views: NaNs and signed zeros count."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), what


def _stepwise(torch, env, eta=None):
    """K times policy_act(obs) then step(actions): the stacked outputs rollout_policy returns."""
    obs = env.obs
    rows = []
    for k in range(K):
        act = env.policy_act(obs)
        obs, rew, term, trunc, _ = env.step(act, eta=None if eta is None else eta[k])
        rows.append((act.clone(), obs.clone(), rew.clone(), term.view(torch.uint8).clone(),
                     trunc.view(torch.uint8).clone(), env.info_u8.clone()))
    return tuple(torch.stack(c) for c in zip(*rows))


NAMES = ("actions", "obs", "reward", "terminated", "truncated", "info")
RESET_BIT = 16


@pytest.mark.parametrize("case,n", [("hover_same_stochastic", 200), ("hover_same_stochastic", 1),
                                    ("hover_same_stochastic", 64), ("forward_next_deterministic", 200),
                                    ("hover_noreset_eta_stochastic", 200), ("hover_templates_stochastic", 200)])
def test_fused_rollout_bitwise_equals_stepwise(torch, policy, case, n):
    kw, task, stochastic, eta = {}, "hover", True, None
    if case == "forward_next_deterministic":
        kw, task, stochastic = dict(autoreset_mode="next_step"), "forward_flight", False
    elif case == "hover_noreset_eta_stochastic":
        kw = dict(autoreset=False)
        g = torch.Generator().manual_seed(5)
        eta = (10.0 * torch.randn((K, n, 3), generator=g)).to("cuda:0")
    a, b = _env(torch, n, task, **kw), _env(torch, n, task, **kw)
    for e in (a, b):
        if case == "hover_templates_stochastic":
            e.set_trim_conds([{"gr_alt": 60.0 + 0.5 * i} for i in range(n)])
        _set(e, policy, stochastic)
        e.reset()
    epi0 = a.get_state()[1][:, 2].clone()
    b.get_state()
    fused = a.rollout_policy(K, eta=eta)
    step = _stepwise(torch, b, eta)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, fused, step):
        _assert_same(torch, x, y, (case, n, name))
    (sa, ca), (sb, cb) = a.get_state(), b.get_state()
    _assert_same(torch, sa, sb, "state")
    _assert_same(torch, ca, cb, "counters")
    assert torch.isfinite(fused[0]).all()
    resets = int(((fused[5] & RESET_BIT) != 0).sum())
    print(f"\n[{case} N={n}] {K} steps bitwise, {resets} reset bits, episodes begun {int((ca[:, 2] - epi0).min())}")
    if kw.get("autoreset", True):   # TimeLimit 5: every env reset twice in 12 steps
        assert int((ca[:, 2] - epi0).min()) >= 2
        assert resets >= 2 * n or kw.get("autoreset_mode") == "next_step"   # (a next-step reset's info byte is 0)
    if case == "hover_templates_stochastic":   # the reset observations the next action saw are the envs' own
        assert float((fused[1][4, :, 16] - fused[1][4, 0, 16]).abs().max()) > 50.0
    a.close()
    b.close()


def test_constant_policy_equals_open_loop_rollout(torch):
    """All weights zero, b3 an action: rollout_policy is rollout() of that action (hg_policy_act plays
    no part)."""
    n = 200
    b3 = torch.tensor([0.31, -0.17, 0.08, 0.23])
    z = lambda *s: torch.zeros(s)   # noqa: E731
    a, b = _env(torch, n), _env(torch, n)
    a.set_policy([(z(64, 17), z(64)), (z(64, 64), z(64)), (z(4, 64), b3)])
    a.reset()
    b.reset()
    fused = a.rollout_policy(K)
    acts = b3.to("cuda:0").expand(K, n, 4).contiguous()
    ref = b.rollout(acts)
    torch.cuda.synchronize()
    _assert_same(torch, fused[0], acts, "actions_out")
    for name, x, y in zip(NAMES[1:], fused[1:], ref):
        _assert_same(torch, x, y, name)
    assert int(((fused[5] & RESET_BIT) != 0).sum()) >= 2 * n
    (sa, ca), (sb, cb) = a.get_state(), b.get_state()
    _assert_same(torch, sa, sb, "state")
    _assert_same(torch, ca, cb, "counters")
    a.close()
    b.close()


def _forward(obs, p, dtype):
    """NumPy forward pass of the policy in `dtype` (weights, normalisation and inputs are the float32
    values, converted)."""
    m = p["model"]
    c = lambda t: t.detach().numpy().astype(dtype)   # noqa: E731
    x = (obs.astype(dtype) - c(p["obs_mean"])) * c(p["obs_scale"])
    h = np.tanh(x @ c(m[0].weight).T + c(m[0].bias))
    h = np.tanh(h @ c(m[2].weight).T + c(m[2].bias))
    out = h @ c(m[4].weight).T + c(m[4].bias)
    assert out.dtype == dtype
    return out


def test_policy_values_against_float64(torch, policy):
    """Deterministic policy_act on golden observation rows against the float64 forward pass.
    Yardstick: the error of the float32 NumPy forward pass against the same float64 result; the
    kernel's max abs error must be <= 4x that (another summation order, an exp-based tanh), floored at
    4 ulp of the largest |action|."""
    n = 200
    rows = _golden_obs()
    obs = rows[np.linspace(0, len(rows) - 1, n).astype(int)]
    env = _env(torch, n)
    _set(env, policy, stochastic=False)
    env.reset()
    got = env.policy_act(torch.as_tensor(obs, device="cuda:0")).cpu().numpy().astype(np.float64)
    ref = _forward(obs, policy, np.float64)
    err32 = np.abs(_forward(obs, policy, np.float32).astype(np.float64) - ref).max()
    err = np.abs(got - ref).max()
    floor = 4 * float(np.spacing(np.float32(np.abs(ref).max())))
    print(f"\n[policy values] kernel max|d| {err:.3e}, float32 NumPy max|d| {err32:.3e}, ratio {err / err32:.2f} "
          f"(bound 4; floor {floor:.3e}; max|a| {np.abs(ref).max():.3f})")
    assert np.abs(ref).max() > 0.05 and np.abs(ref).std() > 0.01   # a non-trivial function of the rows
    assert err <= max(4 * err32, floor)
    env.close()


def _z_ref(gid, step, epi, seed):
    """The action noise from include/heligym_amd.h: one Philox4x32-10 call on (gid_lo, gid_hi, step,
    episode) with the key (seed_lo ^ KEY0, seed_hi ^ KEY1), float64 Box-Muller of the four words."""
    gid = np.asarray(gid, dtype=np.int64).astype(np.uint64)
    rows = np.empty((len(gid), 6), dtype=np.uint64)
    rows[:, 0] = gid & np.uint64(pr.MASK)
    rows[:, 1] = gid >> np.uint64(32)
    rows[:, 2] = np.asarray(step, dtype=np.int64).astype(np.uint64) & np.uint64(pr.MASK)
    rows[:, 3] = np.asarray(epi, dtype=np.int64).astype(np.uint64) & np.uint64(pr.MASK)
    rows[:, 4] = np.uint64((seed & pr.MASK) ^ KEY0)
    rows[:, 5] = np.uint64(((seed >> 32) & pr.MASK) ^ KEY1)
    r = pr.philox4x32_10(rows)
    r0, r1 = np.sqrt(-2.0 * np.log(pr.u01(r[:, 0]))), np.sqrt(-2.0 * np.log(pr.u01(r[:, 2])))
    a1, a3 = 2 * np.pi * pr.turn_frac(r[:, 1]), 2 * np.pi * pr.turn_frac(r[:, 3])
    return np.stack([r0 * np.cos(a1), r0 * np.sin(a1), r1 * np.cos(a3), r1 * np.sin(a3)], axis=1)


def test_action_noise_matches_host_and_is_its_own_stream(torch):
    """Zero weights and biases, log_std = 0: actions == z.  z against the host restatement (tolerance of
    the eta test), z is not the turbulence noise of the same env, and an env holding envs 64..127 of the
    population (env_offset) draws bitwise their rows."""
    n, off = 200, (1 << 33) + 5
    z = lambda *s: torch.zeros(s)   # noqa: E731
    pairs = [(z(64, 17), z(64)), (z(64, 64), z(64)), (z(4, 64), z(4))]
    rng = np.random.RandomState(9)
    ctr = np.zeros((n, 3), np.int32)
    ctr[:, 0] = rng.randint(-5000, 5000, size=n)
    ctr[:, 2] = rng.randint(0, 1 << 20, size=n)
    env = _env(torch, n, env_offset=off)
    env.set_policy(pairs, log_std=z(4))
    env.set_state(counters=ctr)
    got32 = env.policy_act().cpu().numpy()
    got = got32.astype(np.float64)
    ref = _z_ref(off + np.arange(n), ctr[:, 0], ctr[:, 2], SEED)
    err, tol = np.abs(got - ref), ETA_ABS + ETA_REL * np.abs(ref)
    print(f"\n[action noise] max|d| {err.max():.3e}, max |d|/tol {(err / tol).max():.3f}")
    assert np.all(err <= tol), np.argwhere(err > tol)[:10]
    eta = env.debug_eta().cpu().numpy().astype(np.float64) * 0.1   # sqrt(dt): unit normals
    assert np.abs(got[:, :3] - eta).max() > 1.0 and np.mean(np.abs(got[:, :3] - eta) < 1e-3) < 0.01
    _, c2 = env.get_state()
    np.testing.assert_array_equal(c2.cpu().numpy()[:, [0, 2]], np.where(ctr < 0, -1, ctr)[:, [0, 2]])   # env unmodified
    part = _env(torch, 64, env_offset=off + 64)
    part.set_policy(pairs, log_std=z(4))
    part.set_state(counters=ctr[64:128])
    np.testing.assert_array_equal(part.policy_act().cpu().numpy().view(np.int32), got32[64:128].view(np.int32))
    env.close()
    part.close()


def test_set_policy_and_rollout_in_one_graph(torch, policy):
    """set_policy + rollout_policy(12) captured into one graph (a linear chain), replayed twice: bitwise
    two eager calls on a twin env."""
    n = 200
    a, b = _env(torch, n), _env(torch, n)
    cur_a, cur_b = a.reset()[0].clone(), b.reset()[0].clone()
    dev = _on_device(policy)
    u8, f32 = torch.uint8, torch.float32
    out = (torch.empty((K, n, 4), dtype=f32, device="cuda:0"), torch.empty((K, n, 17), dtype=f32, device="cuda:0"),
           torch.empty((K, n), dtype=f32, device="cuda:0"), torch.empty((K, n), dtype=u8, device="cuda:0"),
           torch.empty((K, n), dtype=u8, device="cuda:0"), torch.empty((K, n), dtype=u8, device="cuda:0"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _set(a, dev)
        assert a.rollout_policy(K, obs0=cur_a, out=out) is out
    for rep in range(2):
        g.replay()
        _set(b, dev)
        ref = b.rollout_policy(K, obs0=cur_b)
        torch.cuda.synchronize()
        for name, x, y in zip(NAMES, out, ref):
            _assert_same(torch, x, y, (rep, name))
        cur_a.copy_(out[1][-1])
        cur_b.copy_(ref[1][-1])
    (sa, ca), (sb, cb) = a.get_state(), b.get_state()
    _assert_same(torch, sa, sb, "state")
    _assert_same(torch, ca, cb, "counters")
    assert int(ca[:, 2].min()) >= 1 + 4   # reset() and two TimeLimit resets per rollout
    a.close()
    b.close()


def test_errors_leave_the_env_untouched(torch, policy):
    from heligym_amd._abi import HeliGymError
    n = 200

    def unchanged(env, call):
        env.reset()
        s0, c0 = env.get_state()
        with pytest.raises(HeliGymError, match="error -1"):
            call()
        s1, c1 = env.get_state()
        _assert_same(torch, s0, s1, "state")
        _assert_same(torch, c0, c1, "counters")

    env = _env(torch, n)
    unchanged(env, lambda: env.rollout_policy(K))   # no policy set
    unchanged(env, lambda: env.policy_act())
    _set(env, policy)
    good = env.rollout_policy(K)
    big = torch.empty((K * n * 17 + 4,), dtype=torch.float32, device="cuda:0")
    bad = (good[0], big[1:1 + K * n * 17].view(K, n, 17)) + good[2:]   # obs 4 bytes off a 16-byte boundary
    assert bad[1].data_ptr() % 16 == 4
    unchanged(env, lambda: env.rollout_policy(K, out=bad))
    env.close()
    env = _env(torch, n, reset_mode="retrim", max_episode_steps=None)
    _set(env, policy)
    unchanged(env, lambda: env.rollout_policy(K))   # auto-resets that re-trim run between steps
    env.close()
