"""GPU: the fused PPO loss-gradient kernel (hg_ppo_grad, HeliVecEnv.ppo_grad).

  1. values: the gradient and the statistics against heligym_amd.policy.ppo_loss in float64 on the CPU,
     measured against float32 CPU torch autograd of the same expression;
  2. an index is bitwise the materialised rows; out-of-range entries are skipped and counted;
     and the same past the kernels' loop thresholds (a wave's second and third tile, the reduction's
     sixteen-deep batches, the block cap), with an index of up to 131 139 draws from the stored rows;
  3. clip semantics: a batch clipped out entirely leaves only the entropy term's gradient;
  4. determinism, and a captured call replayed on changed weights;
  5. consistency with the rollout that produced the data;
  6. argument errors leave the outputs and the env untouched.

Inputs throughout: observations from the golden rows the policy tests use, a seeded random policy, "old"
log-probabilities from a perturbed copy of the weights (ratios on both sides of both clip edges), normal
advantages.  Run with -m gpu."""
import ctypes
import math
import types

import numpy as np
import pytest

from test_gpu_policy_rollout import _assert_same, _golden_obs

pytestmark = pytest.mark.gpu

B = 4200
CLIP, VF, ENT = 0.2, 0.5, 0.01
SIZES = (1, 63, 64, 65, 200, 4099)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def make_data():
    """The stored rows (float32 CPU tensors) and the learner's weights; pure CPU."""
    import torch
    from heligym_amd import ActorCriticParams
    from heligym_amd.policy import LOG_2PI, ppo_views
    nn = torch.nn
    torch.manual_seed(20)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
    critic = nn.Linear(64, 1)
    params = ActorCriticParams(actor, critic, nn.Parameter(torch.tensor([-1.0, -0.7, -1.3, -0.9])))
    rows = _golden_obs()
    o64 = rows.astype(np.float64)
    obs = torch.as_tensor(rows[(np.arange(B) * 7) % len(rows)])
    mean = torch.tensor(o64.mean(0), dtype=torch.float32)
    scale = torch.tensor(1.0 / o64.std(0), dtype=torch.float32)
    g = torch.Generator().manual_seed(77)
    # the behaviour policy: a perturbed copy of the weights; its actions and their log-probabilities
    old = (params.theta.detach() + 0.02 * torch.randn((5641,), generator=g)).double()
    p = ppo_views(old)
    x = (obs.double() - mean.double()) * scale.double()
    h2 = torch.tanh(torch.tanh(x @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"])
    z = torch.randn((B, 4), generator=g, dtype=torch.float64)
    actions = (h2 @ p["W3"].T + p["b3"] + torch.exp(p["log_std"]) * z).float()
    zz = (actions.double() - (h2 @ p["W3"].T + p["b3"])) * torch.exp(-p["log_std"])
    logp_old = (-0.5 * (zz * zz).sum(-1) - p["log_std"].sum() - 2 * LOG_2PI).float()
    adv = torch.randn((B,), generator=g)
    # returns one unit above the (untrained) critic's values, as an untrained critic's are: with zero-mean
    # errors db_v, a group of ONE number, is a sum that cancels to a tenth of its terms, and what float32
    # torch's error on that one number happens to be decides the bound (measured so at M = 64: kernel
    # 3.9e-9 against float32 torch's 1.7e-10, where M = 63 and 65 gave torch 2.3e-9 and 5.9e-10)
    ret = (h2 @ p["w_v"] + p["b_v"]).float() + 1.0 + 0.5 * torch.randn((B,), generator=g)
    # row 0 is the lone lane of M = 1: it must contribute through the ratio, not only through the value
    new = ppo_views(params.theta.detach().double())
    n2 = torch.tanh(torch.tanh(x[:1] @ new["W1"].T + new["b1"]) @ new["W2"].T + new["b2"])
    z0 = (actions[:1].double() - (n2 @ new["W3"].T + new["b3"])) * torch.exp(-new["log_std"])
    r0 = float(torch.exp(-0.5 * (z0 * z0).sum() - new["log_std"].sum() - 2 * LOG_2PI - logp_old[0].double()))
    if (adv[0] > 0 and r0 > 1 + CLIP) or (adv[0] < 0 and r0 < 1 - CLIP):
        adv[0] = -adv[0]
    return types.SimpleNamespace(params=params, obs=obs, actions=actions, logp_old=logp_old, adv=adv, ret=ret, mean=mean,
                                 scale=scale)


def loss_on(torch, d, theta, rows, dtype, clip=CLIP, vf=VF, ent=ENT, logp_old=None, divisor=None):
    """ppo_loss of the stored rows `rows` (a LongTensor) in `dtype` on the CPU: (gradient, stats).  divisor: the M
    the means divide by when it is not len(rows) (skipped index entries)."""
    from heligym_amd.policy import LOG_2PI, ppo_loss, ppo_views
    c = lambda t: t[rows].to(dtype)   # noqa: E731
    th = theta.detach().cpu().to(dtype).clone().requires_grad_(True)
    lp = d.logp_old if logp_old is None else logp_old
    L, stats = ppo_loss(th, c(d.obs), c(d.actions), c(lp), c(d.adv), c(d.ret), clip, vf, ent,
                        None if d.mean is None else d.mean.to(dtype), None if d.scale is None else d.scale.to(dtype))
    if divisor is not None:
        k = len(rows) / divisor
        H = ppo_views(th)["log_std"].sum() + 2.0 * (1.0 + LOG_2PI)
        L = (L + ent * H) * k - ent * H
        stats = stats.clone()
        stats[[0, 1, 2, 3, 6]] *= k
        stats[5] = stats[0] + vf * stats[1] - ent * stats[4]
    L.backward()
    return th.grad.detach(), stats.detach()


def ratios(torch, d, theta, logp_old=None):
    """float64 probability ratios of every stored row under `theta`."""
    from heligym_amd.policy import LOG_2PI, ppo_views
    p = ppo_views(theta.detach().cpu().double())
    x = d.obs.double() if d.mean is None else (d.obs.double() - d.mean.double()) * d.scale.double()
    h2 = torch.tanh(torch.tanh(x @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"])
    z = (d.actions.double() - (h2 @ p["W3"].T + p["b3"])) * torch.exp(-p["log_std"])
    logp = -0.5 * (z * z).sum(-1) - p["log_std"].sum() - 2 * LOG_2PI
    return torch.exp(logp - (d.logp_old if logp_old is None else logp_old).double()), logp


@pytest.fixture(scope="module")
def data(torch):
    d = make_data()
    # the inputs do what the tests need, in float64: a good part of the samples is clipped out, and no
    # ratio sits so close to a clip edge that float32 could put it on the other side
    r, _ = ratios(torch, d, d.params.theta)
    out = ((d.adv > 0) & (r > 1 + CLIP)) | ((d.adv < 0) & (r < 1 - CLIP))
    for m in SIZES[2:]:
        assert 0.10 <= float(out[:m].double().mean()) <= 0.60, (m, float(out[:m].double().mean()))
    assert float(torch.minimum((r - (1 + CLIP)).abs(), (r - (1 - CLIP)).abs()).min()) >= 1e-4
    assert bool((r > 1 + CLIP).any()) and bool((r < 1 - CLIP).any()) and not bool(out[0])
    assert 0.10 <= float(out.double().mean()) <= 0.60
    d.dev = types.SimpleNamespace(**{k: getattr(d, k).to("cuda:0") for k in ("obs", "actions", "logp_old", "adv", "ret",
                                                                            "mean", "scale")})
    d.theta = d.params.theta.detach().clone()   # (CPU, float32: the weights every test starts from)
    d.refs = {}
    return d


@pytest.fixture(scope="module")
def env(torch):
    from heligym_amd import HeliVecEnv
    e = HeliVecEnv(64, task="hover", dt=0.01, device="cuda:0", seed=3, autoreset=True, max_episode_steps=5)
    yield e
    e.close()


def dev_params(torch, theta):
    """What HeliVecEnv.ppo_grad reads of an ActorCriticParams: theta and grad on the device."""
    return types.SimpleNamespace(theta=theta.detach().to("cuda:0").clone(),
                                 grad=torch.full((5641,), float("nan"), device="cuda:0"))


def run(torch, env, d, theta, rows=None, index=None, **kw):
    """ppo_grad on the first `rows` stored rows (all B when None) -> (grad, stats) on the CPU."""
    P = dev_params(torch, theta)
    s = slice(None) if rows is None else slice(0, rows)
    v = d.dev
    kw = dict(dict(clip=CLIP, vf_coef=VF, ent_coef=ENT), **kw)
    lp = kw.pop("logp_old", v.logp_old)
    g, st = env.ppo_grad(P, v.obs[s], v.actions[s], lp[s], v.adv[s], v.ret[s], index=index, obs_mean=v.mean,
                         obs_scale=v.scale, **kw)
    torch.cuda.synchronize()
    return g.cpu(), st.cpu()


def reference(torch, d, m):
    """(float64 gradient, float64 stats, float32 CPU gradient, float32 CPU stats) of rows 0..m-1, computed once."""
    if m not in d.refs:
        rows = torch.arange(m)
        d.refs[m] = loss_on(torch, d, d.theta, rows, torch.float64) + loss_on(torch, d, d.theta, rows, torch.float32)
    return d.refs[m]


def check_values(torch, what, got, got_stats, ref):
    """The kernel's max abs error per parameter group (and over stats[0..6]) against float64 must be within
    max(4 x the float32 CPU torch error against the same float64 values, 4 ulp of the group's largest
    magnitude)."""
    from heligym_amd.policy import PPO_LAYOUT
    g64, s64, g32, s32 = ref
    groups = {k: slice(o, o + math.prod(s)) for k, (o, s) in PPO_LAYOUT.items()}
    worst = []
    for name, (x, x32, x64) in dict({k: (got[s], g32[s], g64[s]) for k, s in groups.items()},
                                    stats=(got_stats[:7], s32[:7], s64[:7])).items():
        err = float((x.double() - x64).abs().max())
        err32 = float((x32.double() - x64).abs().max())
        floor = 4 * float(np.spacing(np.float32(float(x64.abs().max()))))
        bound = max(4 * err32, floor)
        print(f"[{what}] {name:8s} kernel max|d| {err:.3e}  float32 torch {err32:.3e}  floor {floor:.3e}  "
              f"err/bound {err / bound if bound else float('inf'):.3f}")
        worst.append((name, err, bound))
    assert torch.isfinite(got).all() and torch.isfinite(got_stats).all(), what
    bad = [(n, e, b) for n, e, b in worst if not e <= b]
    assert not bad, (what, bad)


@pytest.mark.parametrize("m", SIZES)
def test_values_against_float64(torch, data, env, m):
    print()
    got, st = run(torch, env, data, data.theta, rows=m)
    ref = reference(torch, data, m)
    assert float(ref[0].abs().max()) > 1e-3   # a non-trivial gradient
    check_values(torch, f"M={m}", got, st, ref)
    assert float(st[7]) == 0.0


def test_values_without_normalisation(torch, data, env):
    """obs_mean = obs_scale = NULL: the kernel reads the observations as they are.  The rows are the module's,
    normalised beforehand in float32 on the CPU; the reference is ppo_loss of those float32 inputs without
    a normalisation."""
    m = 65   # two tiles, the second one lane
    x = (data.obs - data.mean) * data.scale
    d = types.SimpleNamespace(**dict(vars(data), obs=x, mean=None, scale=None))
    r, _ = ratios(torch, d, data.theta)
    assert float(torch.minimum((r[:m] - (1 + CLIP)).abs(), (r[:m] - (1 - CLIP)).abs()).min()) >= 1e-4
    v = data.dev
    P = dev_params(torch, data.theta)
    got, st = env.ppo_grad(P, x[:m].to("cuda:0"), v.actions[:m], v.logp_old[:m], v.adv[:m], v.ret[:m], clip=CLIP,
                           vf_coef=VF, ent_coef=ENT, obs_mean=None, obs_scale=None)
    torch.cuda.synchronize()
    rows = torch.arange(m)
    ref = loss_on(torch, d, data.theta, rows, torch.float64) + loss_on(torch, d, data.theta, rows, torch.float32)
    assert float(ref[0].abs().max()) > 1e-3
    print()
    check_values(torch, f"M={m}, no mean / scale", got.cpu(), st.cpu(), ref)
    assert float(st[7]) == 0.0


# Sizes past the kernels' own loop thresholds, reached with an index drawn with replacement from the B stored
# rows.  tiles = ceil(M / 64); the gradient kernel runs nb = min(ceil(tiles / 4), 256) blocks of four waves, wave
# w of block k taking the tiles 4 k + w, 4 k + w + 4 nb, ..; the reduce kernel's chain c adds the blocks c, c + 4,
# .., sixteen at a time while b + 60 < nb and one at a time after that.
#   M        tiles  nb
#   15 361     241   61   chain 0 takes one batch of sixteen (0 + 60 < 61), chains 1-3 the one-by-one loop only
#   16 384     256   64   every chain exactly one batch and nothing after it; every lane of every tile valid
#   16 385     257   65   chain 0 a batch and one more term; block 64 is one wave with one valid lane
#   33 000     516  129   two batches (b = c, c + 64: c + 124 < 129) and a term after them for chain 0
#   65 666   1 027  256   the block cap: tiles 1024-1026 are the second trip of block 0's waves 0-2, the last one
#                         with 2 valid lanes; four batches per chain and nothing after them
#  131 139   2 050  256   every wave takes two tiles, waves 0 and 1 of block 0 a third (tiles 2048, 2049; 3 lanes)
LARGE = (15361, 16384, 16385, 33000, 65666, 131139)
OUT_OF_RANGE = (-1, B, 2 ** 31 - 1, -2 ** 31)


def large_case(torch, d, m):
    """A drawn index of m entries, the same with four entries that name no row, and the references; once per m."""
    key = ("large", m)
    if key not in d.refs:
        g = torch.Generator().manual_seed(1000 + m)
        clean = torch.randint(0, B, (m,), generator=g, dtype=torch.int64)
        # where the four go: the first lane of all; the last lane of tile 1; a lane of tile 1024, a wave's second
        # trip, where M reaches it (else of tile 5); the last entry (the last, ragged, tile's last valid lane)
        where = [0, 127, 1024 * 64 + 35 if m > 1025 * 64 else 5 * 64 + 35, m - 1]
        assert where[2] < m - 1
        planted = clean.clone()
        planted[where] = torch.tensor(OUT_OF_RANGE)
        keep = torch.ones(m, dtype=torch.bool)
        keep[where] = False
        rows = clean[keep]
        r, _ = ratios(torch, d, d.theta)
        clipped_out = ((d.adv > 0) & (r > 1 + CLIP)) | ((d.adv < 0) & (r < 1 - CLIP))
        outside = (r < 1 - CLIP) | (r > 1 + CLIP)
        for ix in (clean, rows):
            assert 0.10 <= float(clipped_out[ix].double().mean()) <= 0.60, m
        ref, ref_clean = (loss_on(torch, d, d.theta, ix, torch.float64, divisor=m)
                          + loss_on(torch, d, d.theta, ix, torch.float32, divisor=m) for ix in (rows, clean))
        d.refs[key] = types.SimpleNamespace(clean=clean, planted=planted, rows=rows, ref=ref, ref_clean=ref_clean,
                                            outside=int(outside[rows].sum()), outside_clean=int(outside[clean].sum()))
    return d.refs[key]


@pytest.mark.parametrize("m", LARGE)
def test_large_index_values_and_exact_counts(torch, data, env, m):
    """Values as test_values_against_float64; and two counts no tolerance covers: the rows whose ratio is outside
    the clip range and the entries that name no row.  stats[3] is that count, an integer below 2^24 that float32
    sums exactly, times the float32 1 / M: two roundings, so stats[3] * M is within count * 2^-22 < 0.04 of it.
    Once with four entries out of range (the means still divide by M), once with every entry in range, so that
    the last tile's last lane contributes."""
    c = large_case(torch, data, m)
    got, st = run(torch, env, data, data.theta, index=c.planted.to(torch.int32).to("cuda:0"))
    print()
    check_values(torch, f"M={m} by index, 4 out of range", got, st, c.ref)
    assert float(st[7]) == len(OUT_OF_RANGE)
    assert round(float(st[3]) * m) == c.outside, (float(st[3]) * m, c.outside)
    # and with every entry in range (the last tile's lanes all count)
    got, st = run(torch, env, data, data.theta, index=c.clean.to(torch.int32).to("cuda:0"))
    check_values(torch, f"M={m} by index", got, st, c.ref_clean)
    assert float(st[7]) == 0.0
    assert round(float(st[3]) * m) == c.outside_clean, (float(st[3]) * m, c.outside_clean)


def test_large_index_second_trip_is_bitwise_the_materialised_rows_and_deterministic(torch, data, env):
    m = 65666   # 1 027 tiles on 256 blocks: the first three waves take a second tile, with and without an index
    c = large_case(torch, data, m)
    v = data.dev
    ix = c.clean.to(torch.int32).to("cuda:0")
    a, sa = run(torch, env, data, data.theta, index=ix)
    b, sb = run(torch, env, data, data.theta, index=ix)
    _assert_same(torch, a, b, "two calls")
    _assert_same(torch, sa, sb, "two calls' stats")
    P = dev_params(torch, data.theta)
    di = c.clean.to("cuda:0")
    gm, sm = env.ppo_grad(P, v.obs[di].contiguous(), v.actions[di].contiguous(), v.logp_old[di].contiguous(),
                          v.adv[di].contiguous(), v.ret[di].contiguous(), clip=CLIP, vf_coef=VF, ent_coef=ENT,
                          obs_mean=v.mean, obs_scale=v.scale)
    torch.cuda.synchronize()
    _assert_same(torch, a, gm.cpu(), "gradient")
    _assert_same(torch, sa, sm.cpu(), "stats")
    assert float(sa[7]) == 0.0 and round(float(sa[3]) * m) == c.outside_clean


def test_index_is_bitwise_the_materialised_rows(torch, data, env):
    g = torch.Generator().manual_seed(9)
    idx = torch.randperm(B, generator=g)[:777]
    v = data.dev
    a, sa = run(torch, env, data, data.theta, index=idx.to(torch.int32).to("cuda:0"))
    P = dev_params(torch, data.theta)
    di = idx.to("cuda:0")
    gm, sm = env.ppo_grad(P, v.obs[di].contiguous(), v.actions[di].contiguous(), v.logp_old[di].contiguous(),
                          v.adv[di].contiguous(), v.ret[di].contiguous(), clip=CLIP, vf_coef=VF, ent_coef=ENT,
                          obs_mean=v.mean, obs_scale=v.scale)
    torch.cuda.synchronize()
    _assert_same(torch, a, gm.cpu(), "gradient")
    _assert_same(torch, sa, sm.cpu(), "stats")
    # two entries that name no row: skipped and counted, the means still over M
    bad = torch.cat([idx[:100], torch.tensor([-1]), idx[100:500], torch.tensor([B]), idx[500:]])
    got, st = run(torch, env, data, data.theta, index=bad.to(torch.int32).to("cuda:0"))
    assert float(st[7]) == 2.0
    ref = (loss_on(torch, data, data.theta, idx, torch.float64, divisor=len(bad))
           + loss_on(torch, data, data.theta, idx, torch.float32, divisor=len(bad)))
    print()
    check_values(torch, "index with 2 of 779 out of range", got, st, ref)


def test_a_batch_clipped_out_leaves_the_entropy_term(torch, data, env):
    m = 200
    _, logp = ratios(torch, data, data.theta)
    lp_old = (logp - torch.sign(data.adv.double())).float()   # r = e where A > 0, 1 / e where A < 0
    assert bool((data.adv[:m] != 0).all())
    got, st = run(torch, env, data, data.theta, rows=m, vf_coef=0.0, ent_coef=0.01, logp_old=lp_old.to("cuda:0"))
    want = torch.zeros(5641)
    want[5572:5576] = -0.01
    _assert_same(torch, got, want, "gradient")
    assert float(st[3]) == 1.0


def test_deterministic_and_replayed_on_changed_weights(torch, data, env):
    m = 4099
    v = data.dev
    a, sa = run(torch, env, data, data.theta, rows=m)
    b, sb = run(torch, env, data, data.theta, rows=m)
    _assert_same(torch, a, b, "two eager calls")
    _assert_same(torch, sa, sb, "two eager calls' stats")
    P = dev_params(torch, data.theta)
    stats = torch.empty((8,), dtype=torch.float32, device="cuda:0")
    args = (v.obs[:m], v.actions[:m], v.logp_old[:m], v.adv[:m], v.ret[:m])
    kw = dict(clip=CLIP, vf_coef=VF, ent_coef=ENT, obs_mean=v.mean, obs_scale=v.scale, stats=stats)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        env.ppo_grad(P, *args, **kw)
    g.replay()
    torch.cuda.synchronize()
    _assert_same(torch, P.grad.cpu(), a, "replay 1")
    _assert_same(torch, stats.cpu(), sa, "replay 1 stats")
    gen = torch.Generator().manual_seed(4)
    theta2 = data.theta + 0.01 * torch.randn((5641,), generator=gen)
    P.theta.copy_(theta2)   # in place: the graph reads the same buffer
    g.replay()
    torch.cuda.synchronize()
    c, sc = run(torch, env, data, theta2, rows=m)
    assert not torch.equal(c, a)
    _assert_same(torch, P.grad.cpu(), c, "replay 2")
    _assert_same(torch, stats.cpu(), sc, "replay 2 stats")


def test_consistent_with_the_rollout_that_made_the_data(torch, data):
    """A 64-env, K = 8 actor-critic rollout fed back with the weights that produced it: the ratio is 1 and the
    approximate KL 0 up to the rounding float32 torch shows on the same device data."""
    from heligym_amd import ActorCriticParams, HeliVecEnv
    from heligym_amd.policy import ppo_loss
    nn = torch.nn
    torch.manual_seed(20)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to("cuda:0")
    critic = nn.Linear(64, 1).to("cuda:0")
    P = ActorCriticParams(actor, critic, nn.Parameter(torch.tensor([-1.0, -0.7, -1.3, -0.9], device="cuda:0")))
    assert P.theta.device.type == "cuda"
    v = data.dev
    K, n = 8, 64
    env = HeliVecEnv(n, task="hover", dt=0.01, device="cuda:0", seed=3, autoreset=True, max_episode_steps=5)
    env.set_policy(actor, log_std=P.log_std.detach(), obs_mean=v.mean, obs_scale=v.scale)
    env.set_value_head(critic)
    obs0 = env.reset()[0].clone()
    out = env.rollout_actor_critic(K, obs0=obs0)
    obs_in = torch.cat([obs0[None], out["obs"][:-1]]).contiguous()   # the observation each action was computed from
    _, st = env.ppo_grad(P, obs_in, out["actions"], out["logp"], out["advantages"], out["returns"], clip=CLIP,
                         vf_coef=VF, ent_coef=ENT, obs_mean=v.mean, obs_scale=v.scale)
    with torch.no_grad():
        _, ref = ppo_loss(P, obs_in.view(-1, 17), out["actions"].view(-1, 4), out["logp"].view(-1),
                          out["advantages"].view(-1), out["returns"].view(-1), CLIP, VF, ENT, v.mean, v.scale)
    torch.cuda.synchronize()
    st, ref = st.cpu().double(), ref.cpu().double()
    floor = 8 * float(np.spacing(np.float32(float(out["logp"].abs().max()))))
    print(f"\n[rollout consistency] kernel KL {float(st[2]):.3e}, |r - 1| {abs(float(st[6]) - 1):.3e}; float32 torch "
          f"KL {float(ref[2]):.3e}, |r - 1| {abs(float(ref[6]) - 1):.3e}; floor {floor:.3e}")
    assert abs(float(st[2])) <= max(4 * abs(float(ref[2])), floor)
    assert abs(float(st[6]) - 1) <= max(4 * abs(float(ref[6]) - 1), floor)
    assert torch.isfinite(P.grad).all() and float(P.grad.abs().max()) > 0
    assert actor[2].weight.grad.data_ptr() == P.grad.data_ptr() + 4 * 1152   # the modules see the kernel's gradient
    env.close()


def test_errors_leave_outputs_and_env_untouched(torch, data, env):
    lib, v = env.lib, data.dev
    m = 200
    env.reset()
    s0, c0 = env.get_state()
    P = dev_params(torch, data.theta)
    P.grad.fill_(-7.0)
    stats = torch.full((8,), -7.0, device="cuda:0")
    ws = torch.empty((lib.hg_ppo_grad_workspace_bytes() + 16,), dtype=torch.uint8, device="cuda:0")
    idx = torch.arange(m, dtype=torch.int32, device="cuda:0")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)   # noqa: E731
    good = dict(env=env._h, theta=p(P.theta), mean=p(v.mean), scale=p(v.scale), obs=p(v.obs), act=p(v.actions),
                lp=p(v.logp_old), adv=p(v.adv), ret=p(v.ret), B=B, index=p(idx), M=m, clip=0.2, vf=0.5, ent=0.01,
                grad=p(P.grad), stats=p(stats), ws=p(ws), stream=env._stream())
    cases = {"NULL env": dict(env=None), "B < 1": dict(B=0), "M < 1": dict(M=0), "M too large": dict(M=2 ** 31 - 255),
             "no index, M != B": dict(index=None), "clip 0": dict(clip=0.0), "clip 1": dict(clip=1.0),
             "clip nan": dict(clip=float("nan")), "vf < 0": dict(vf=-0.5), "vf inf": dict(vf=float("inf")),
             "ent < 0": dict(ent=-0.01), "ent nan": dict(ent=float("nan")),
             "actions 4 bytes off": dict(act=off(v.actions, 4)), "workspace 8 bytes off": dict(ws=off(ws, 8)),
             "theta 2 bytes off": dict(theta=off(P.theta, 2)), "stats 1 byte off": dict(stats=off(stats, 1)),
             "index 2 bytes off": dict(index=off(idx, 2))}
    for k in ("theta", "obs", "act", "lp", "adv", "ret", "grad", "ws"):
        cases[f"NULL {k}"] = {k: None}
    for name, change in cases.items():
        a = dict(good, **change)
        assert lib.hg_ppo_grad(*a.values()) == -1, name
        assert lib.hg_last_error(), name
    torch.cuda.synchronize()
    assert bool((P.grad == -7.0).all()) and bool((stats == -7.0).all())
    assert lib.hg_ppo_grad(*good.values()) == 0   # (and NULL mean / scale / stats are allowed)
    assert lib.hg_ppo_grad(*dict(good, mean=None, scale=None, stats=None).values()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(P.grad).all()
    s1, c1 = env.get_state()
    _assert_same(torch, s0, s1, "state")
    _assert_same(torch, c0, c1, "counters")
