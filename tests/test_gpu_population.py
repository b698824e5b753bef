"""GPU: populations of policies and the evolution-strategies learner (hg_pop_pack, hg_rollout_pop,
hg_es_perturb, hg_es_noise, hg_pop_fitness, hg_es_grad; heligym_amd.evolution.ES).

  1. pop_pack is bitwise set_policy_theta, image by image (the 7552 floats, and through policy_evaluate);
  2. a population rollout is bitwise one rollout_policy per member on separate handles (pins tile -> member);
  3. the handle's own policy is neither needed nor touched;
  4. the parameter noise against the host Philox, its key separation and gen + *gen_dev;
  5. es_perturb: theta +- sigma eps within one fp32 rounding, the images bitwise pop_pack of member_theta;
  6. pop_fitness against float64 NumPy, chunked, first-episode, restart, NaN containment;
  7. es_grad: utilities bitwise, the gradient within its rounding bound, stats, monotone invariance,
     at sizes past each loop's threshold (named below);
  8. one generation captured and replayed equals the eager calls bitwise;
  9. the estimator descends a toy quadratic (a sign or pairing error fails here);
 10. errors leave outputs and the env untouched.
Run with -m gpu."""
import types

import numpy as np
import pytest

import philox_ref as pr
from test_gpu_noise import ETA_ABS, ETA_REL

pytestmark = pytest.mark.gpu

K = 12
DEV = "cuda:0"
SEED = 0x5EED_7E4B_0000_0031
ES_KEY0, ES_KEY1 = 0x65735F6E, 0x6F697365      # include/heligym_amd.h: the parameter noise's key constants
POL_KEY0, POL_KEY1 = 0x706F6C69, 0x63795F7A    # the action noise's
NP, NPERT, NIMG = 5641, 5572, 7552
# hg_es_grad's loops (csrc/es.h): an fma chain is kEsPairChunk = 16 pairs, so 17 pairs (P = 34) is the first
# size with two partials to add; the rank kernel's blocks are kEsBlock = 256 members and it stages the keys in
# LDS kEsRankTile = 1024 at a time, and the statistics' one block strides the members by kEsReduceThreads =
# 1024, so P = 2050 is past all three (three key tiles, the last of two keys; 65 chunks).
PAIR_CHUNK, RANK_BLOCK, RANK_TILE, REDUCE_THREADS = 16, 256, 1024, 1024
GRAD_SIZES = (2, 6, 2 * PAIR_CHUNK + 2, 2 * max(RANK_TILE, REDUCE_THREADS) + 2)
# unit normals: test_gpu_noise's bounds hold for eta = z / sqrt(dt) at dt = 0.01; scaled back by sqrt(dt)
Z_ABS, Z_REL = ETA_ABS * 0.1, ETA_REL


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def _env(n, task="hover", **kw):
    from heligym_amd import HeliVecEnv
    kw.setdefault("seed", SEED)
    kw.setdefault("autoreset", True)
    kw.setdefault("max_episode_steps", 5)
    return HeliVecEnv(n, task=task, dt=0.01, device=DEV, **kw)


def _theta_cpu(torch, seed):
    """torch's default init under `seed`, log_std around -1, as one flat [5641] vector."""
    from heligym_amd import ActorCriticParams
    nn = torch.nn
    torch.manual_seed(seed)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
    critic = nn.Linear(64, 1)
    ls = torch.tensor([-1.0, -0.7, -1.3, -0.9]) + 0.01 * seed
    return ActorCriticParams(actor, critic, ls).theta.detach().clone()


@pytest.fixture(scope="module")
def thetas(torch):
    """Four independently initialised members [4, 5641] on the device, and the shared normalisation."""
    th = torch.stack([_theta_cpu(torch, 40 + p) for p in range(4)]).to(DEV)
    g = torch.Generator().manual_seed(3)
    mean = (0.1 * torch.randn(17, generator=g)).to(DEV)
    scale = (1.0 + 0.1 * torch.rand(17, generator=g)).to(DEV)
    return types.SimpleNamespace(th=th, mean=mean, scale=scale)


def _P(torch, theta):
    """What the wrappers take as `params`: theta and grad on the device."""
    return types.SimpleNamespace(theta=theta.clone(), grad=torch.zeros(NP, device=DEV))


def _same(torch, a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.is_floating_point():
        it = torch.int64 if a.dtype == torch.float64 else torch.int32
        a, b = a.contiguous().view(it), b.contiguous().view(it)
    assert torch.equal(a, b), what


def _set_member(torch, env, theta, v, stochastic):
    """The member's policy on a handle of its own, by the calls that existed before populations did."""
    from heligym_amd import policy
    if stochastic:
        env.set_policy_theta(_P(torch, theta), obs_mean=v.mean, obs_scale=v.scale)
        return
    w = policy.ppo_views(theta)
    env.set_policy([(w["W1"], w["b1"]), (w["W2"], w["b2"]), (w["W3"], w["b3"])], log_std=None, obs_mean=v.mean,
                   obs_scale=v.scale)
    env.set_value_head((w["w_v"], w["b_v"]))


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("stochastic", [True, False])
def test_pop_pack_is_set_policy_theta(torch, thetas, stochastic):
    n = 70
    env, scratch, probe = _env(n), _env(n), _env(n)
    th3 = thetas.th[:3].contiguous()
    images = env.pop_pack(th3, stochastic=stochastic, obs_mean=thetas.mean, obs_scale=thetas.scale)
    assert images.shape == (3, NIMG)
    obs = scratch.reset()[0].clone()
    probe.reset()
    for p in range(3):
        _set_member(torch, scratch, th3[p], thetas, stochastic)
        _same(torch, images[p], scratch.debug_policy_image(), ("image", p))
        # and through behaviour: the image installed in another handle evaluates bitwise the same
        probe.debug_policy_image(set_to=images[p].clone())
        for x, y, name in zip(probe.policy_evaluate(obs), scratch.policy_evaluate(obs), ("actions", "logp", "value")):
            _same(torch, x, y, (name, p))
    head = images[:, :6].cpu().numpy()
    if stochastic:
        assert (head[:, 4] == 1.0).all() and (head[:, :4] > 0).all()
    else:
        assert not head.any()
    assert not torch.equal(images[0], images[1])
    # without normalisation: mean 0, scale 1
    bare = env.pop_pack(th3, stochastic=stochastic)
    assert not bare[:, 8:25].any() and (bare[:, 25:42] == 1.0).all()
    _same(torch, bare[:, 64:], images[:, 64:], "weights")


# ------------------------------------------------------------------ 2
NAMES = ("actions", "obs", "reward", "terminated", "truncated", "info")
SHAPES = [(4, 64, 200), (2, 128, 256), (1, 64, 1)]
CASES = ["hover_same_stochastic", "forward_next_deterministic", "hover_templates_stochastic"]


@pytest.mark.parametrize("P,epm,n", SHAPES)
@pytest.mark.parametrize("case", CASES)
def test_population_rollout_is_one_rollout_per_member(torch, thetas, case, P, epm, n):
    kw, task, stochastic = {}, "hover", True
    if case == "forward_next_deterministic":
        kw, task, stochastic = dict(autoreset_mode="next_step"), "forward_flight", False
    conds = [{"gr_alt": 60.0 + 0.5 * i} for i in range(n)]
    pop = _env(n, task, **kw)
    tmpl = None
    if case == "hover_templates_stochastic":
        r = pop.set_trim_conds(conds)
        # the rows hg_set_reset_templates takes (HeliVecEnv.set_trim_conds): the members get slices of these
        tmpl = torch.cat([r["state"], r["obs"][:, 4:7], r["obs"][:, 16:17], r["obs"]], dim=1).contiguous()
    pop.reset()
    th = thetas.th[:P].contiguous()
    images = pop.pop_pack(th, stochastic=stochastic, obs_mean=thetas.mean, obs_scale=thetas.scale)
    launches0 = pop.debug_launches()
    got = pop.rollout_population(K, images, epm)
    launches1 = pop.debug_launches()
    state, ctr = pop.get_state()
    torch.cuda.synchronize()
    assert sum(launches1.values()) - sum(launches0.values()) == 1   # one launch for all members, counted as hg_rollout_policy's
    for p in range(P):
        lo, hi = p * epm, min(n, (p + 1) * epm)
        one = _env(hi - lo, task, env_offset=lo, **kw)
        if tmpl is not None:
            rows = tmpl[lo:hi].contiguous()
            one._check(one.lib.hg_set_reset_templates(one._h, rows.data_ptr(), one._stream()))
        one.reset()
        _set_member(torch, one, th[p], thetas, stochastic)
        want = one.rollout_policy(K)
        for name, x, y in zip(NAMES, got, want):
            _same(torch, x[:, lo:hi].contiguous(), y, (case, P, epm, n, p, name))
        s1, c1 = one.get_state()
        _same(torch, state[lo:hi].contiguous(), s1, ("state", p))
        _same(torch, ctr[lo:hi].contiguous(), c1, ("counters", p))
        one.close()
    assert torch.isfinite(got[0]).all()
    if P > 1:   # the members differ (independent inits), so a kernel that ignored the member offset failed above
        c = min(epm, n - epm)
        assert not torch.equal(th[0], th[1]) and not torch.equal(got[0][:, :c], got[0][:, epm:epm + c])
    if case != "forward_next_deterministic":
        assert int(((got[5] & 16) != 0).sum()) >= 2 * n   # TimeLimit 5: every env reset twice in 12 steps
    pop.close()


# ------------------------------------------------------------------ 3
def test_the_handles_own_policy_is_not_read(torch, thetas):
    n, epm = 200, 64
    a, twin = _env(n), _env(n)
    a.reset(), twin.reset()
    images = a.pop_pack(thetas.th, obs_mean=thetas.mean, obs_scale=thetas.scale)
    a.rollout_population(K, images, epm)          # no policy set on the handle: succeeds
    with pytest.raises(Exception, match="no policy set"):
        a.rollout_policy(1)
    # the handle's own policy and a population in turn: the own rollout is what a twin without populations gives
    b = _env(n)
    b.reset()
    for e in (b, twin):
        _set_member(torch, e, thetas.th[3], thetas, True)
    own0 = b.debug_policy_image().clone()
    first = b.rollout_population(K, images, epm)
    twin_first = twin.rollout_population(K, images, epm)
    _same(torch, b.debug_policy_image(), own0, "own image after a population rollout")
    got = b.rollout_policy(K, obs0=first[1][K - 1].clone())
    want = twin.rollout_policy(K, obs0=twin_first[1][K - 1].clone())
    for name, x, y in zip(NAMES, got, want):
        _same(torch, x, y, name)


# ------------------------------------------------------------------ 4
def _host_eps(seed, pair, gen, key0=ES_KEY0, key1=ES_KEY1):
    """eps_pair [5572] in float64 from the header's counter and key, by tests/philox_ref.py."""
    k0, k1 = (seed & 0xFFFFFFFF) ^ key0, (seed >> 32) ^ key1
    g = gen & (2 ** 64 - 1)
    rows = np.empty((NPERT // 4, 6), dtype=np.uint64)
    rows[:, 0] = np.arange(NPERT // 4)          # i >> 2
    rows[:, 1:] = (pair, g & 0xFFFFFFFF, g >> 32, k0, k1)
    r = pr.philox4x32_10(rows)
    r0 = np.sqrt(-2.0 * np.log(pr.u01(r[:, 0])))
    r1 = np.sqrt(-2.0 * np.log(pr.u01(r[:, 2])))
    a1, a3 = 2.0 * np.pi * pr.turn_frac(r[:, 1]), 2.0 * np.pi * pr.turn_frac(r[:, 3])
    return np.stack([r0 * np.cos(a1), r0 * np.sin(a1), r1 * np.cos(a3), r1 * np.sin(a3)], axis=1).reshape(-1)   # i & 3


def test_noise_is_the_headers(torch):
    env = _env(64)
    seed = 0x0123_4567_89AB_CDEF
    for pair, gen in ((0, 0), (5, 7), (32767, (1 << 32) + 3)):
        got = env.es_noise(seed, pair, gen=gen).cpu().numpy().astype(np.float64)
        want = _host_eps(seed, pair, gen)
        err = np.abs(got - want)
        print(f"\n[es_noise pair {pair} gen {gen}] max err {err.max():.3e}, sd {got.std():.4f}")
        assert np.all(err <= Z_ABS + Z_REL * np.abs(want)), err.max()
    base = env.es_noise(seed, 5, gen=7)
    for other in (env.es_noise(seed, 6, gen=7), env.es_noise(seed, 5, gen=8), env.es_noise(seed + 1, 5, gen=7),
                  env.es_noise(seed ^ (1 << 40), 5, gen=7)):
        assert float((other == base).float().mean()) < 0.01
    # gen and *gen_dev add (a 64-bit sum)
    four = torch.tensor([4], dtype=torch.int32, device=DEV)
    _same(torch, env.es_noise(seed, 5, gen=3, gen_dev=four), base, "gen + *gen_dev")
    _same(torch, env.es_noise(seed, 5, gen=(1 << 32) - 1, gen_dev=four), env.es_noise(seed, 5, gen=(1 << 32) + 3), "carry")
    # the stream is neither the action noise's nor the turbulence's of the same seed
    g = base.cpu().numpy().astype(np.float64)
    for k0, k1 in ((POL_KEY0, POL_KEY1), (0, 0)):
        other = _host_eps(seed, 5, 7, k0, k1)
        assert np.mean(np.abs(g - other) <= Z_ABS + Z_REL * np.abs(other)) < 0.01
    x = np.concatenate([env.es_noise(seed, j).cpu().numpy() for j in range(8)]).astype(np.float64)
    assert abs(x.mean()) < 0.02 and abs(x.std() - 1.0) < 0.02


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("P", [2, 6])
@pytest.mark.parametrize("stochastic", [True, False])
def test_perturb(torch, thetas, P, stochastic):
    env = _env(64)
    seed, gen, sigma = 99, 11, 0.05
    params = _P(torch, thetas.th[1])
    mt = torch.full((P, NP), float("nan"), device=DEV)
    images = env.es_perturb(params, P, sigma, seed, gen=gen, stochastic=stochastic, obs_mean=thetas.mean,
                            obs_scale=thetas.scale, member_theta=mt)
    th = params.theta.cpu().numpy()
    got = mt.cpu().numpy()
    s64 = float(np.float32(sigma))
    for j in range(P // 2):
        eps = env.es_noise(seed, j, gen=gen).cpu().numpy().astype(np.float64)
        for m, sg in ((2 * j, 1.0), (2 * j + 1, -1.0)):
            want = th[:NPERT].astype(np.float64) + sg * s64 * eps
            bound = 2.0 ** -23 * (np.abs(th[:NPERT]) + np.abs(s64 * eps))
            err = np.abs(got[m, :NPERT] - want)
            assert np.all(err <= bound), (m, float((err / bound).max()))
            assert np.array_equal(got[m, NPERT:].view(np.int32), th[NPERT:].view(np.int32)), m
        assert np.abs(got[2 * j, :NPERT] - got[2 * j + 1, :NPERT]).max() > sigma   # the pair is spread
    if P > 2:
        assert not np.array_equal(got[0], got[2])
    _same(torch, images, env.pop_pack(mt, stochastic=stochastic, obs_mean=thetas.mean, obs_scale=thetas.scale), "images")
    # the head words: hg_set_policy's with / without log_std
    scratch = _env(64)
    _set_member(torch, scratch, mt[P - 1], thetas, stochastic)
    _same(torch, images[P - 1], scratch.debug_policy_image(), "image of the last member")
    # without member_theta: the same images
    again = env.es_perturb(params, P, sigma, seed, gen=gen, stochastic=stochastic, obs_mean=thetas.mean,
                           obs_scale=thetas.scale)
    _same(torch, again, images, "images without member_theta")


# ------------------------------------------------------------------ 6
@pytest.fixture(scope="module")
def rolled(torch, thetas):
    """Two chunks of a population rollout at the shapes of (2), shared by the fitness tests (not modified)."""
    out = {}
    for P, epm, n in SHAPES[:2]:
        env = _env(n)
        env.reset()
        images = env.pop_pack(thetas.th[:P].contiguous(), obs_mean=thetas.mean, obs_scale=thetas.scale)
        c1 = tuple(x.clone() for x in env.rollout_population(K, images, epm))
        c2 = tuple(x.clone() for x in env.rollout_population(K, images, epm, obs0=c1[1][K - 1].clone()))
        out[(P, epm, n)] = (env, c1, c2)
    return out


@pytest.mark.parametrize("P,epm,n", SHAPES[:2])
@pytest.mark.parametrize("mode", ["window", "first_episode"])
def test_fitness(torch, rolled, mode, P, epm, n):
    from heligym_amd import pop_fitness_ref
    env, c1, c2 = rolled[(P, epm, n)]
    r1, te1, tr1 = (c1[2].clone(), c1[3].clone(), c1[4].clone())
    r2, te2, tr2 = (c2[2].clone(), c2[3].clone(), c2[4].clone())
    if mode == "first_episode":
        # TimeLimit 5 would end every episode inside chunk 1: keep a few envs alive into chunk 2, and end env 3
        # exactly at the last step of chunk 1, so chunk 2's rewards of env 3 must not count
        te1[:, :8] = 0
        tr1[:, :8] = 0
        tr1[K - 1, 3] = 1
        te2[:, :8] = 0
        tr2[:, :8] = 0
        tr2[4, 0] = 1
    f8 = lambda: torch.full((P,), 123.0, dtype=torch.float64, device=DEV)   # noqa: E731 (restart must clear it)
    u8 = lambda: torch.full((n,), 0, dtype=torch.uint8, device=DEV)         # noqa: E731
    sums, alive = f8(), u8()
    fit1 = env.pop_fitness(r1, te1, tr1, P, epm, sums, mode=mode, restart=True, alive=alive).clone()
    s1, f1, a1 = pop_fitness_ref(r1.cpu().numpy(), te1.cpu().numpy(), tr1.cpu().numpy(), P, epm, mode=mode)
    got = sums.cpu().numpy()
    print(f"\n[pop_fitness {mode} P={P}] sums {got}, rel err {np.abs(got - s1).max() / np.abs(s1).max():.2e}")
    assert np.all(np.abs(got - s1) <= 1e-12 * np.abs(s1))
    assert np.array_equal(fit1.cpu().numpy(), (got / np.array([min(n, (p + 1) * epm) - p * epm for p in range(P)]))
                          .astype(np.float32))
    if mode == "first_episode":
        assert np.array_equal(alive.cpu().numpy(), a1) and a1[:8].tolist() == [1, 1, 1, 0, 1, 1, 1, 1] and not a1[8:].any()
    fit2 = env.pop_fitness(r2, te2, tr2, P, epm, sums, mode=mode, alive=alive).clone()
    s2, f2, a2 = pop_fitness_ref(r2.cpu().numpy(), te2.cpu().numpy(), tr2.cpu().numpy(), P, epm, mode=mode, alive=a1, sums=s1)
    assert np.all(np.abs(sums.cpu().numpy() - s2) <= 1e-12 * np.abs(s2))
    assert s2[0] != s1[0]
    if mode == "first_episode":
        assert np.array_equal(alive.cpu().numpy(), a2) and a2[0] == 0 and a2[1] == 1
        # env 3 ended at the last step of chunk 1: member 0's gain in chunk 2 is envs 0 (to step 4), 1, 2, 4 .. 7 only
        gain = r2.double()[:, [1, 2, 4, 5, 6, 7]].sum().item() + r2.double()[:5, 0].sum().item()
        assert abs((s2[0] - s1[0]) - gain) <= 1e-12 * abs(gain)
    # two chunked calls == one call over the concatenation, bitwise (fp64 sums of these fp32 rewards are exact)
    sums_c, alive_c = f8(), u8()
    fit_c = env.pop_fitness(torch.cat([r1, r2]), torch.cat([te1, te2]), torch.cat([tr1, tr2]), P, epm, sums_c, mode=mode,
                            restart=True, alive=alive_c)
    _same(torch, sums_c, sums, "chunked sums")
    _same(torch, fit_c, fit2, "chunked fitness")
    _same(torch, alive_c, alive, "chunked alive")
    # two runs are bitwise equal; restart clears
    sums_d, alive_d = f8(), u8()
    env.pop_fitness(r1, te1, tr1, P, epm, sums_d, mode=mode, restart=True, alive=alive_d)
    fit_d = env.pop_fitness(r2, te2, tr2, P, epm, sums_d, mode=mode, alive=alive_d)
    _same(torch, sums_d, sums, "rerun sums")
    _same(torch, fit_d, fit2, "rerun fitness")
    fit_r = env.pop_fitness(r1, te1, tr1, P, epm, sums_d, mode=mode, restart=True, alive=alive_d)
    _same(torch, fit_r, fit1, "restart")
    # a NaN reward in one env poisons only its member
    bad = r1.clone()
    bad[2, epm + 1] = float("nan")
    fit_n = env.pop_fitness(bad, te1, tr1, P, epm, f8(), mode=mode, restart=True, alive=u8()).cpu().numpy()
    assert np.isnan(fit_n[1]) and np.array_equal(np.delete(fit_n, 1), np.delete(fit1.cpu().numpy(), 1))
    # the inputs were not written
    _same(torch, r1, c1[2], "reward untouched")


# ------------------------------------------------------------------ 7
def _fitness_for(P, rng):
    f = rng.normal(size=P).astype(np.float32)
    if P >= 6:
        f[4] = f[1]              # a tie
        f[2] = np.nan            # and a NaN
    if P >= 34:
        f[20] = -np.inf
        f[7] = f[1]
    return f


@pytest.mark.parametrize("P", GRAD_SIZES)
def test_grad(torch, P):
    from heligym_amd import es_grad_ref, es_utilities_ref
    env = _env(64)
    seed, gen, sigma = 0xABCDEF, 5, 0.03
    rng = np.random.default_rng(P)
    f = _fitness_for(P, rng)
    fit = torch.tensor(f, device=DEV)
    params = _P(torch, torch.zeros(NP))
    params.grad.fill_(7.0)
    grad, stats = env.es_grad(params, fit, sigma, seed, gen=gen)
    g = grad.cpu().numpy()
    st = stats.cpu().numpy()
    # utilities: the workspace's first P floats, bitwise the restatement
    u = env._es_workspace(P)[:4 * P].view(torch.float32).cpu().numpy()
    assert np.array_equal(u.view(np.int32), es_utilities_ref(f).view(np.int32))
    eps = torch.stack([env.es_noise(seed, j, gen=gen) for j in range(P // 2)]).cpu().numpy()
    want = es_grad_ref(f, eps, sigma)
    w = np.abs((u[0::2] - u[1::2]).astype(np.float64))
    bound = (P / 2 + 4) * 2.0 ** -24 * (w @ np.abs(eps.astype(np.float64))) / (P * float(np.float32(sigma)))
    err = np.abs(g[:NPERT] - want[:NPERT])
    print(f"\n[es_grad P={P}] |g| {np.linalg.norm(g):.4e}, max err / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), float((err / bound).max())
    assert not g[NPERT:].any() and np.array_equal(g[NPERT:].view(np.int32), np.zeros(NP - NPERT, np.int32))
    # stats against NumPy
    fin = np.isfinite(f)
    assert abs(st[0] - f[fin].astype(np.float64).mean()) <= 2.0 ** -23 * abs(f[fin].astype(np.float64).mean())
    assert st[1] == f[fin].min() and st[2] == f[fin].max() and st[3] == (~fin).sum()
    assert st[4] == int(np.argmax(np.where(fin, f, -np.inf)))   # argmax: the lowest index among ties
    nrm = np.linalg.norm(g.astype(np.float64))
    # 6 fma + 6 butterfly + 16 wave additions on the squares (halved by the root), then the root itself
    assert abs(st[5] - nrm) <= 2.0 ** -19 * nrm and st[6] == 0 and st[7] == 0
    # two runs are bitwise equal; a monotone transform of the fitness leaves the gradient bitwise unchanged
    p2 = _P(torch, torch.zeros(NP))
    g2, s2 = env.es_grad(p2, fit, sigma, seed, gen=gen)
    _same(torch, g2, grad, "rerun")
    _same(torch, s2, stats, "rerun stats")
    efit = torch.exp(fit)
    g3, _ = env.es_grad(p2, efit, sigma, seed, gen=gen)
    assert len(np.unique(efit.cpu().numpy()[fin])) == len(np.unique(f[fin]))   # (exp kept the values apart)
    _same(torch, g3, grad, "exp(fitness)")
    # gen + *gen_dev
    five = torch.tensor([2], dtype=torch.int32, device=DEV)
    g4, _ = env.es_grad(p2, fit, sigma, seed, gen=gen - 2, gen_dev=five)
    _same(torch, g4, grad, "gen_dev")
    # stats are optional (the library's NULL)
    g5 = torch.zeros(NP, device=DEV)
    lib = env.lib
    env._check(lib.hg_es_grad(env._h, fit.data_ptr(), P, sigma, seed, gen, None, g5.data_ptr(), None,
                              env._es_workspace(P).data_ptr(), None))
    _same(torch, g5, grad, "without stats")


def test_grad_stats_without_a_finite_member(torch):
    env = _env(64)
    fit = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")], device=DEV)
    grad, stats = env.es_grad(_P(torch, torch.zeros(NP)), fit, 0.1, 1)
    st = stats.cpu().numpy()
    assert np.isnan(st[:3]).all() and st[3] == 4 and st[4] == -1
    # the ranks are still a permutation (by index): u = (-1/2, -1/6, 1/6, 1/2), a finite gradient
    assert torch.isfinite(grad).all() and float(grad.abs().max()) > 0


# ------------------------------------------------------------------ 8
def test_a_generation_captured_equals_eager(torch, thetas):
    from heligym_amd import ES, PPOOptState
    P, epm = 4, 64
    n = P * epm

    def make():
        env = _env(n)
        env.reset()
        params, state = _P(torch, thetas.th[0]), PPOOptState(DEV)
        es = ES(env, params, state, P, epm, sigma=0.05, seed=17, lr=1e-2, max_grad_norm=1.0, obs_mean=thetas.mean,
                obs_scale=thetas.scale)
        return env, params, state, es

    ea, pa, sa, esa = make()
    eb, pb, sb, esb = make()
    # (the rollout's output buffers are allocated outside the capture; the warm-up launch is undone by the resets)
    esa._out = ea.rollout_population(K, esa.images.zero_(), epm)
    esb._out = eb.rollout_population(K, esb.images.zero_(), epm)
    ea.reset(), eb.reset()
    obs0a, obs0b = ea.obs.clone(), eb.obs.clone()
    rows_a, rows_b, noise = [], [], []
    for _ in range(3):
        esa.generation(K, chunks=2, obs0=obs0a)
        rows_a.append((pa.theta.clone(), sa.state.clone(), esa.stats.clone(), esa.fitness.clone()))
        noise.append(esa.member_theta[0].clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        esb.generation(K, chunks=2, obs0=obs0b)
    assert sb.counters()["applied"] == 0   # captured, not run
    for _ in range(3):
        g.replay()
        rows_b.append((pb.theta.clone(), sb.state.clone(), esb.stats.clone(), esb.fitness.clone()))
    torch.cuda.synchronize()
    for k, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        for name, x, y in zip(("theta", "state", "stats", "fitness"), ra, rb):
            _same(torch, x, y, (k, name))
    assert sa.counters()["applied"] == 3
    assert not torch.equal(rows_a[0][0], rows_a[1][0])
    # successive generations drew different noise: member 0's offset from theta changes direction
    d0 = noise[0] - thetas.th[0]
    d1 = noise[1] - rows_a[0][0]
    assert float((d0[:NPERT] * d1[:NPERT]).sum().abs()) < 0.2 * float(d0[:NPERT].norm() * d1[:NPERT].norm())
    i, fbest, th = esa.best_member()
    assert 0 <= i < P and fbest == float(esa.fitness.max()) and th.shape == (NP,)
    _same(torch, ea.debug_policy_image(), eb.debug_policy_image(), "published policy")


# ------------------------------------------------------------------ 9
def test_the_estimator_descends_a_toy_quadratic(torch, thetas):
    from heligym_amd import PPOOptState
    env = _env(64)
    P, sigma, seed = 64, 0.05, 5
    params, state = _P(torch, thetas.th[2]), PPOOptState(DEV)
    gsrc = torch.Generator().manual_seed(8)
    target = (thetas.th[2].cpu() + 0.3 * torch.randn(NP, generator=gsrc)).to(DEV)
    mt = torch.empty((P, NP), device=DEV)
    d0 = float((params.theta - target)[:NPERT].norm())
    tail0 = params.theta[NPERT:].clone()
    for _ in range(30):
        env.es_perturb(params, P, sigma, seed, gen_dev=state.tail[0:1], member_theta=mt)
        fit = -((mt - target)[:, :NPERT] ** 2).sum(1)
        env.es_grad(params, fit.contiguous(), sigma, seed, gen_dev=state.tail[0:1])
        env.ppo_adam(params, state, lr=0.02)
    d1 = float((params.theta - target)[:NPERT].norm())
    print(f"\n[toy ES] |theta - target| {d0:.3f} -> {d1:.3f} in 30 generations of {P}")
    assert state.counters()["applied"] == 30
    assert d1 < d0
    _same(torch, params.theta[NPERT:].clone(), tail0, "unperturbed parameters")


# ------------------------------------------------------------------ 10
def test_errors_leave_outputs_and_the_env_untouched(torch, thetas):
    from heligym_amd import HeliGymError
    n, P, epm = 200, 4, 64
    env = _env(n)
    env.reset()
    lib, h = env.lib, env._h
    images = env.pop_pack(thetas.th, obs_mean=thetas.mean, obs_scale=thetas.scale)
    s0, c0 = env.get_state()
    s0, c0 = s0.clone(), c0.clone()
    mark = 7.25
    act = torch.full((K, n, 4), mark, device=DEV)
    obs = torch.full((K, n, 17), mark, device=DEV)
    rew = torch.full((K, n), mark, device=DEV)
    te = torch.full((K, n), 9, dtype=torch.uint8, device=DEV)
    tr = torch.full((K, n), 9, dtype=torch.uint8, device=DEV)
    img_out = torch.full((P, NIMG), mark, device=DEV)
    mt_out = torch.full((P, NP), mark, device=DEV)
    sums = torch.full((P,), mark, dtype=torch.float64, device=DEV)
    fit = torch.full((P,), mark, device=DEV)
    alive = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    grad = torch.full((NP,), mark, device=DEV)
    ws = env._es_workspace(P)
    th = thetas.th[0].contiguous()
    p = lambda t: t.data_ptr()   # noqa: E731

    def rollout(P=P, epm=epm, images_p=p(images), k=K, act_p=p(act)):
        return lib.hg_rollout_pop(h, images_p, P, epm, p(env.obs), k, act_p, p(obs), p(rew), p(te), p(tr), None, None)

    def fitness(P=P, epm=epm, mode=1, alive_p=p(alive), k=K):
        return lib.hg_pop_fitness(h, p(rew), p(te), p(tr), k, P, epm, mode, 1, alive_p, p(sums), p(fit), None)

    bad = [rollout(P=3), rollout(P=5), rollout(epm=96), rollout(epm=0), rollout(images_p=p(images) + 4), rollout(k=0),
           rollout(images_p=None), rollout(act_p=p(act) + 4), rollout(P=65537),
           fitness(P=3), fitness(epm=32), fitness(mode=1, alive_p=None), fitness(mode=2), fitness(k=0),
           lib.hg_pop_pack(h, p(thetas.th), 0, 1, None, None, p(img_out), None),
           lib.hg_pop_pack(h, p(thetas.th), P, 1, None, None, p(img_out) + 4, None),
           lib.hg_es_perturb(h, p(th), 3, 0.1, 1, 0, None, 1, None, None, p(img_out), p(mt_out), None),
           lib.hg_es_perturb(h, p(th), P, 0.0, 1, 0, None, 1, None, None, p(img_out), p(mt_out), None),
           lib.hg_es_perturb(h, p(th), P, float("nan"), 1, 0, None, 1, None, None, p(img_out), p(mt_out), None),
           lib.hg_es_perturb(h, p(th), P, 0.1, 1, 0, None, 1, None, None, p(img_out) + 8, p(mt_out), None),
           lib.hg_es_grad(h, p(fit), 3, 0.1, 1, 0, None, p(grad), None, p(ws), None),
           lib.hg_es_grad(h, p(fit), 16386, 0.1, 1, 0, None, p(grad), None, p(ws), None),
           lib.hg_es_grad(h, p(fit), P, -1.0, 1, 0, None, p(grad), None, p(ws), None),
           lib.hg_es_grad(h, p(fit), P, 0.1, 1, 0, None, p(grad), None, p(ws) + 4, None),
           lib.hg_es_noise(h, 1, 0, None, -1, p(grad), None)]
    assert all(rc == -1 for rc in bad), bad
    retrim = _env(64, reset_mode="retrim")
    with pytest.raises(HeliGymError, match="RETRIM"):
        retrim.rollout_population(2, images[:1].contiguous(), 64)
    torch.cuda.synchronize()
    for name, t in dict(act=act, obs=obs, rew=rew, img=img_out, mt=mt_out, sums=sums, fit=fit, grad=grad).items():
        assert bool((t == mark).all()), name
    for name, t in dict(te=te, tr=tr, alive=alive).items():
        assert bool((t == 9).all()), name
    s1, c1 = env.get_state()
    _same(torch, s1, s0, "state")
    _same(torch, c1, c0, "counters")
    assert rollout() == 0 and fitness() == 0   # the same arguments, valid, do run
    torch.cuda.synchronize()
    assert not bool((act == mark).any()) and bool(torch.isfinite(fit).all())
