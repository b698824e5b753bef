"""GPU: the PPO update on the device (hg_ppo_shuffle, hg_ppo_adam, hg_ppo_update, hg_set_policy_theta and their
HeliVecEnv wrappers).

  1. the shuffle is the host restatement (tests/ppo_shuffle_ref.py), exactly, also keyed by a device counter, at
     sizes up to 262 144 and at an epoch past 2^32;
  2. the optimiser step's values against a float64 restatement, measured against CPU float32 torch Adam, at step
     counts 1 .. 6, 1 000 and 1 000 003;
  3. ppo_update is bitwise the calls it is made of, made one by one;
  4. determinism, and what must stay untouched does;
  5. a non-finite gradient is dropped and counted, the next clean one applied;
  6. the approximate-KL early stop, and its clearing;
  7. a learning rate rewritten on the device under a captured graph;
  8. a whole training iteration captured once and replayed, against the same iterations run eagerly;
  9. hg_set_policy_theta is set_policy + set_value_head;
 10. argument errors leave everything untouched.

Data: test_gpu_ppo_grad.make_data (B = 4200 stored rows).  Run with -m gpu."""
import ctypes
import math
import types

import numpy as np
import pytest

from ppo_shuffle_ref import shuffle_ref
from test_gpu_policy_rollout import _assert_same
from test_gpu_ppo_grad import B, CLIP, ENT, VF, dev_params, make_data

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-8
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


@pytest.fixture(scope="module")
def data(torch):
    d = make_data()
    d.dev = types.SimpleNamespace(**{k: getattr(d, k).to(DEV) for k in ("obs", "actions", "logp_old", "adv", "ret",
                                                                        "mean", "scale")})
    d.theta = d.params.theta.detach().clone()
    return d


@pytest.fixture(scope="module")
def env(torch):
    from heligym_amd import HeliVecEnv
    e = HeliVecEnv(64, task="hover", dt=0.01, device=DEV, seed=3, autoreset=True, max_episode_steps=5)
    yield e
    e.close()


def fresh(torch, d):
    """(params, state): the weights every test starts from and a zero optimiser state, on the device."""
    from heligym_amd import PPOOptState
    return dev_params(torch, d.theta), PPOOptState(DEV)


def rows_of(d, n=None, adv=None):
    v = d.dev
    s = slice(None) if n is None else slice(0, n)
    return (v.obs[s], v.actions[s], v.logp_old[s], (v.adv if adv is None else adv)[s], v.ret[s])


def loss_kw(d):
    return dict(clip=CLIP, vf_coef=VF, ent_coef=ENT, obs_mean=d.dev.mean, obs_scale=d.dev.scale)


def by_hand(torch, env, d, P, S, rows, epochs, minibatches, seed, index, stats, **opt):
    """ppo_update's sequence made of the single calls (without the leading clear of `stop`)."""
    n = rows[0].shape[0]
    cuts = [j * n // minibatches for j in range(minibatches + 1)]
    for ep in range(epochs):
        env.ppo_shuffle(n, seed, epoch=0, epoch_dev=S.seen, out=index)
        for j in range(minibatches):
            row = stats[ep * minibatches + j]
            env.ppo_grad(P, *rows, index=index[cuts[j]:cuts[j + 1]], stats=row, **loss_kw(d))
            env.ppo_adam(P, S, stats=row, **opt)
    return [b - a for a, b in zip(cuts, cuts[1:])]


# ------------------------------------------------------------------------------------------- 1. shuffle
# 65 537: B - 1 has 17 bits, half = 9, the domain 4^9 = 262 144 just under 4 B (the longest cycle walks);
# 262 144: B - 1 has 18 bits, half = 9, the domain is B itself (no element walks)
@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 4099, 65537, 262144))
def test_shuffle_is_the_host_restatement(torch, env, n):
    seed = 0x9E3779B97F4A7C15
    got = env.ppo_shuffle(n, seed).cpu().numpy()
    want, passes = shuffle_ref(n, seed, 0)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(np.sort(got), np.arange(n))
    if n == 65537:
        assert passes.max() > 8   # (three of four values of the domain are outside [0, B): long walks exist)
    if n == 262144:
        assert passes.max() == 1


def test_shuffle_reads_its_epoch_on_the_device(torch, env):
    seed, n = 77, 4099
    five = torch.tensor([5], dtype=torch.int32, device=DEV)
    a = env.ppo_shuffle(n, seed, epoch=5)
    b = env.ppo_shuffle(n, seed, epoch=0, epoch_dev=five)
    c = env.ppo_shuffle(n, seed, epoch=-2, epoch_dev=five)
    _assert_same(torch, a, b, "epoch 5 on the host and on the device")
    assert np.array_equal(a.cpu().numpy(), shuffle_ref(n, seed, 5)[0])
    assert np.array_equal(c.cpu().numpy(), shuffle_ref(n, seed, 3)[0])
    assert not torch.equal(a, c)


def test_shuffle_epoch_past_32_bits(torch, env):
    """epoch = 2^32 + 3: the high word of the round function's epoch counter, e_hi, is 1, not 0; reached on the
    host, and as 2^32 on the host plus 3 in the device word."""
    seed, n = 77, 4099
    big = 2 ** 32 + 3
    want = shuffle_ref(n, seed, big)[0]
    a = env.ppo_shuffle(n, seed, epoch=big).cpu().numpy()
    three = torch.tensor([3], dtype=torch.int32, device=DEV)
    b = env.ppo_shuffle(n, seed, epoch=2 ** 32, epoch_dev=three).cpu().numpy()
    assert np.array_equal(a, want) and np.array_equal(b, want)
    assert np.array_equal(np.sort(a), np.arange(n))
    low = env.ppo_shuffle(n, seed, epoch=3).cpu().numpy()
    assert np.array_equal(low, shuffle_ref(n, seed, 3)[0]) and not np.array_equal(a, low)


# ------------------------------------------------------------------------------------------- 2. Adam values
def adam_ref64(torch, theta, m, v, t0, g, lr, betas, eps, max_norm):
    """One step in float64 from float32 inputs: (theta, m, v, norm, clip coefficient)."""
    th, m, v, g = (x.double() for x in (theta, m, v, g))
    nrm = torch.sqrt((g * g).sum())
    c = min(1.0, max_norm / (float(nrm) + 1e-6)) if max_norm else 1.0
    g = c * g
    t = t0 + 1
    b1, b2 = betas
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    th = th - (lr / (1 - b1 ** t)) * m / (torch.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return th, m, v, float(nrm), c


def adam_torch32(torch, theta, m, v, t0, g, lr, betas, eps, max_norm):
    """The same step by CPU float32 torch.optim.Adam after clip_grad_norm_: (theta, m, v, norm)."""
    p = torch.nn.Parameter(theta.clone())
    p.grad = g.clone()
    nrm = float(torch.linalg.vector_norm(p.grad))
    if max_norm:
        torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], nrm


def check_step(torch, what, got, ref64, ref32):
    """Per tensor group: the kernel's max error against float64 within max(4 x CPU float32 torch's error against the
    same float64 values, `floor` ulp of the group's largest magnitude); floor 1 for theta, 4 for m and v."""
    from heligym_amd.policy import PPO_LAYOUT
    bad = []
    for q, name, floor_ulp in ((0, "theta", 1), (1, "m", 4), (2, "v", 4)):
        for k, (o, shape) in PPO_LAYOUT.items():
            s = slice(o, o + math.prod(shape))
            x, x32, x64 = got[q][s], ref32[q][s], ref64[q][s]
            err = float((x.double() - x64).abs().max())
            err32 = float((x32.double() - x64).abs().max())
            floor = floor_ulp * float(np.spacing(np.float32(float(x64.abs().max()))))
            bound = max(4 * err32, floor)
            print(f"[{what}] {name:5s} {k:8s} kernel max|d| {err:.3e}  float32 torch {err32:.3e}  floor {floor:.3e}  "
                  f"err/bound {err / bound:.3f}")
            if not err <= bound:
                bad.append((name, k, err, bound))
    err = abs(got[3] - ref64[3])
    bound = max(4 * abs(ref32[3] - ref64[3]), 8 * float(np.spacing(np.float32(ref64[3]))))
    print(f"[{what}] norm {got[3]:.9e}  kernel |d| {err:.3e}  float32 torch {abs(ref32[3] - ref64[3]):.3e}  "
          f"err/bound {err / bound:.3f}")
    if not err <= bound:
        bad.append(("norm", "", err, bound))
    assert not bad, (what, bad)


@pytest.mark.parametrize("clipped", (False, True), ids=("max_grad_norm above the norm", "max_grad_norm below the norm"))
def test_adam_values_against_float64(torch, data, env, clipped):
    print()
    P, S = fresh(torch, data)
    m = 4099
    gen = torch.Generator().manual_seed(12)
    # the sixth gradient: magnitudes over twelve decades, both signs
    synthetic = (10.0 ** (12.0 * torch.rand((5641,), generator=gen) - 6.0)) * torch.sign(torch.randn((5641,), generator=gen))
    for step in range(6):
        if step < 5:
            env.ppo_grad(P, *rows_of(data, m), **loss_kw(data))
        else:
            P.grad.copy_(synthetic)
        g = P.grad.cpu()
        nrm64 = float(torch.sqrt((g.double() ** 2).sum()))
        max_norm = (0.5 if clipped else 2.0) * nrm64
        before = (P.theta.cpu(), S.m.cpu(), S.v.cpu())
        c0 = S.counters()
        assert c0["applied"] == step == c0["seen"]
        env.ppo_adam(P, S, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=max_norm)
        c1 = S.counters()
        assert (c1["applied"], c1["seen"], c1["stop"], c1["skipped_nonfinite"], c1["skipped_stopped"]) == (step + 1,) * 2 + (0,) * 3
        ref64 = adam_ref64(torch, *before, step, g, LR, BETAS, EPS, max_norm)
        ref32 = adam_torch32(torch, *before, step, g, LR, BETAS, EPS, max_norm)
        got = (P.theta.cpu(), S.m.cpu(), S.v.cpu(), c1["last_norm"])
        assert float((got[0] - before[0]).abs().max()) > 0.1 * LR   # a real step
        check_step(torch, f"step {step + 1}, clip coefficient {ref64[4]:.3f}", got, ref64, ref32)
        assert (ref64[4] < 1.0) == clipped
        assert abs(c1["last_clip_coef"] - ref64[4]) <= 1e-6
        _assert_same(torch, P.grad.cpu(), g, "grad is not modified")


@pytest.mark.parametrize("t0", (999, 1000002))
def test_adam_values_at_a_working_step_count(torch, data, env, t0):
    """One step from a state whose `applied` word says t0 steps were taken: beta^t by squaring takes 10 trips for
    t = 1 000 = 0b1111101000 and 20 for t = 1 000 003 (six steps take 3), and the fp64 bias corrections are the
    ones of a long run: 1 - 0.999^1000 = 0.632 at the first, both 1 to the last fp64 bit at the second."""
    print()
    P, S = fresh(torch, data)
    for _ in range(3):   # m and v of a few real steps
        env.ppo_grad(P, *rows_of(data, 4099), **loss_kw(data))
        env.ppo_adam(P, S, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=0.5)
    env.ppo_grad(P, *rows_of(data, 4099), **loss_kw(data))
    S.tail[0] = t0
    g = P.grad.cpu()
    max_norm = 0.5 * float(torch.sqrt((g.double() ** 2).sum()))
    before = (P.theta.cpu(), S.m.cpu(), S.v.cpu())
    assert float(before[1].abs().max()) > 0 and float(before[2].abs().max()) > 0
    c0 = S.counters()
    assert (c0["applied"], c0["seen"]) == (t0, 3)
    env.ppo_adam(P, S, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=max_norm)
    c1 = S.counters()
    assert (c1["applied"], c1["seen"], c1["stop"], c1["skipped_nonfinite"], c1["skipped_stopped"]) == (t0 + 1, 4, 0, 0, 0)
    ref64 = adam_ref64(torch, *before, t0, g, LR, BETAS, EPS, max_norm)
    ref32 = adam_torch32(torch, *before, t0, g, LR, BETAS, EPS, max_norm)
    got = (P.theta.cpu(), S.m.cpu(), S.v.cpu(), c1["last_norm"])
    assert float((got[0] - before[0]).abs().max()) > 0.1 * LR   # a real step
    check_step(torch, f"step {t0 + 1}, clip coefficient {ref64[4]:.3f}", got, ref64, ref32)
    assert ref64[4] < 1.0 and abs(c1["last_clip_coef"] - ref64[4]) <= 1e-6
    _assert_same(torch, P.grad.cpu(), g, "grad is not modified")


# ------------------------------------------------------------------------------------------- 3. composition
@pytest.mark.parametrize("n, epochs, minibatches, sizes", ((B, 2, 3, [1400, 1400, 1400]), (4099, 2, 4, [1024, 1025, 1025, 1025])))
def test_update_is_bitwise_its_parts(torch, data, env, n, epochs, minibatches, sizes):
    opt = dict(lr=LR, betas=BETAS, eps=EPS, max_grad_norm=0.5)
    rows = rows_of(data, n)
    P1, S1 = fresh(torch, data)
    ix1 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    st1 = env.ppo_update(P1, S1, *rows, epochs=epochs, minibatches=minibatches, seed=11, index=ix1, **loss_kw(data), **opt)
    assert st1.shape == (epochs * minibatches, 8)
    P2, S2 = fresh(torch, data)
    ix2 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    st2 = torch.full((epochs * minibatches, 8), float("nan"), device=DEV)
    assert by_hand(torch, env, data, P2, S2, rows, epochs, minibatches, 11, ix2, st2, **opt) == sizes
    torch.cuda.synchronize()
    _assert_same(torch, P1.theta, P2.theta, "theta")
    _assert_same(torch, S1.state, S2.state, "optimiser state")
    _assert_same(torch, st1, st2, "stats rows")
    _assert_same(torch, ix1, ix2, "index")
    c = S1.counters()
    assert c["applied"] == c["seen"] == epochs * minibatches and c["stop"] == 0
    assert np.array_equal(np.sort(ix1.cpu().numpy()), np.arange(n))
    assert np.array_equal(ix1.cpu().numpy(), shuffle_ref(n, 11, (epochs - 1) * minibatches)[0])   # keyed by `seen`
    assert torch.isfinite(st1).all() and not torch.equal(P1.theta.cpu(), data.theta)


# ------------------------------------------------------------------------------------------- 4. determinism
def test_deterministic_and_inputs_untouched(torch, data, env):
    opt = dict(lr=LR, betas=BETAS, eps=EPS, max_grad_norm=0.5)
    env.reset()
    s0, c0 = env.get_state()
    rows = rows_of(data)
    before = [r.clone() for r in rows]
    runs = []
    for _ in range(2):
        P, S = fresh(torch, data)
        st = env.ppo_update(P, S, *rows, epochs=2, minibatches=3, seed=5, **loss_kw(data), **opt).clone()
        runs.append((P.theta.clone(), S.state.clone(), st))
    for a, b, what in zip(*runs, ("theta", "optimiser state", "stats rows")):
        _assert_same(torch, a, b, what)
    for a, b in zip(rows, before):
        _assert_same(torch, a, b, "stored rows")
    s1, c1 = env.get_state()
    _assert_same(torch, s0, s1, "env state")
    _assert_same(torch, c0, c1, "env counters")
    P, S = fresh(torch, data)
    env.ppo_grad(P, *rows, **loss_kw(data))
    g = P.grad.clone()
    env.ppo_adam(P, S, **opt)
    _assert_same(torch, P.grad, g, "grad after ppo_adam")


# ------------------------------------------------------------------------------------------- 5. non-finite gradient
def test_nonfinite_gradient_is_dropped_and_counted(torch, data, env):
    opt = dict(lr=LR, betas=BETAS, eps=EPS, max_grad_norm=0.5)
    P, S = fresh(torch, data)
    index = env.ppo_shuffle(B, 21, epoch_dev=S.seen)
    adv = data.dev.adv.clone()
    adv[int(index[0])] = float("nan")   # a row of the first of three minibatches
    rows = rows_of(data, adv=adv)
    stats = torch.empty((8,), device=DEV)
    snap = lambda: (P.theta.clone(), S.m.clone(), S.v.clone())   # noqa: E731
    s0 = snap()
    env.ppo_grad(P, *rows, index=index[:1400], stats=stats, **loss_kw(data))
    assert not bool(torch.isfinite(P.grad).all())
    env.ppo_adam(P, S, stats=stats, **opt)
    for a, b, what in zip(s0, snap(), ("theta", "m", "v")):
        _assert_same(torch, a, b, what)
    c = S.counters()
    assert (c["applied"], c["seen"], c["skipped_nonfinite"], c["skipped_stopped"], c["stop"]) == (0, 1, 1, 0, 0)
    assert not math.isfinite(c["last_norm"])
    env.ppo_grad(P, *rows, index=index[1400:2800], stats=stats, **loss_kw(data))
    env.ppo_adam(P, S, stats=stats, **opt)
    c = S.counters()
    assert (c["applied"], c["seen"], c["skipped_nonfinite"]) == (1, 2, 1) and math.isfinite(c["last_norm"])
    assert float((P.theta - s0[0]).abs().max()) > 0.5 * LR and bool(torch.isfinite(P.theta).all())
    # the same through ppo_update: the same permutation (seen = 0), so the first minibatch is the dropped one
    P, S = fresh(torch, data)
    env.ppo_update(P, S, *rows, epochs=1, minibatches=3, seed=21, **loss_kw(data), **opt)
    c = S.counters()
    assert (c["applied"], c["seen"], c["skipped_nonfinite"], c["skipped_stopped"]) == (2, 3, 1, 0)
    assert bool(torch.isfinite(P.theta).all()) and bool(torch.isfinite(S.m).all()) and bool(torch.isfinite(S.v).all())


# ------------------------------------------------------------------------------------------- 6. KL stop
def test_kl_stop_drops_the_rest_and_is_cleared(torch, data, env):
    opt = dict(lr=LR, betas=BETAS, eps=EPS, max_grad_norm=0.5)
    rows = rows_of(data)
    P, S = fresh(torch, data)
    st = env.ppo_update(P, S, *rows, epochs=2, minibatches=3, seed=4, **loss_kw(data), **opt)
    kl0 = float(st[0, 2])
    assert kl0 > 0.0   # the behaviour policy is a perturbed copy: the first minibatch's approximate KL
    # (the targeted run starts from the same `seen`, so its first minibatch is the same rows at the same weights)
    P, S = fresh(torch, data)
    theta0 = P.theta.clone()
    st2 = env.ppo_update(P, S, *rows, epochs=2, minibatches=3, seed=4, target_kl=0.5 * kl0 / 1.5, **loss_kw(data), **opt)
    _assert_same(torch, P.theta, theta0, "theta")
    c = S.counters()
    assert (c["applied"], c["seen"], c["stop"], c["skipped_stopped"], c["skipped_nonfinite"]) == (0, 6, 1, 6, 0)
    assert int(S.m.view(torch.int32).abs().max()) == 0 and int(S.v.view(torch.int32).abs().max()) == 0
    assert bool(torch.isfinite(st2).all())   # (the gradients were still computed, and dropped)
    # a target above every minibatch's KL stops nothing
    P3, S3 = fresh(torch, data)
    env.ppo_update(P3, S3, *rows, epochs=2, minibatches=3, seed=4, target_kl=10.0 * float(st[:, 2].abs().max()) + 1.0,
                   **loss_kw(data), **opt)
    assert S3.counters()["applied"] == 6
    # the next update, target off, starts clean
    env.ppo_update(P, S, *rows, epochs=2, minibatches=3, seed=4, **loss_kw(data), **opt)
    c = S.counters()
    assert (c["applied"], c["seen"], c["stop"], c["skipped_stopped"]) == (6, 12, 0, 6)
    assert not torch.equal(P.theta, theta0)


def test_replayed_update_clears_stop_every_time(torch, data, env):
    """A captured ppo_update whose `stop` word is set before every replay (as an update stopped by its KL target
    leaves it) clears it on every replay: the clear is a kernel node.  (A 4-byte memset node in its place left
    the word stale on some replays: 2 of 20 updates of scripts/bench_ppo_update.py were dropped whole.)"""
    P, S = fresh(torch, data)
    rows = rows_of(data)
    kw = dict(epochs=1, minibatches=2, seed=8, lr=LR, betas=BETAS, eps=EPS, **loss_kw(data))
    env.ppo_update(*fresh(torch, data), *rows, **kw)   # (every kernel has run once before the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        env.ppo_update(P, S, *rows, **kw)
    replays = 12
    for _ in range(replays):
        S.state[11296 + 2] = 1
        g.replay()
    c = S.counters()
    assert (c["applied"], c["seen"], c["stop"], c["skipped_stopped"]) == (2 * replays, 2 * replays, 0, 0)


# ------------------------------------------------------------------------------------------- 7. lr on the device
def test_captured_step_reads_lr_on_the_device(torch, data, env):
    opt = dict(betas=BETAS, eps=EPS, max_grad_norm=0.5)
    P, S = fresh(torch, data)
    env.ppo_grad(P, *rows_of(data, 4099), **loss_kw(data))
    Pe, Se = fresh(torch, data)
    Pe.grad.copy_(P.grad)
    env.ppo_adam(*fresh(torch, data), lr=1.0, **opt)   # (the kernel has run once before the capture)
    lr_dev = torch.tensor([1e-3], device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        env.ppo_adam(P, S, lr=123.0, lr_dev=lr_dev, **opt)
    assert S.counters()["seen"] == 0   # captured, not run
    for lr in (7e-4, 2e-4):
        lr_dev.fill_(lr)
        g.replay()
        env.ppo_adam(Pe, Se, lr=float(np.float32(lr)), **opt)
        torch.cuda.synchronize()
        _assert_same(torch, P.theta, Pe.theta, f"theta at lr {lr}")
        _assert_same(torch, S.state, Se.state, f"state at lr {lr}")
    assert S.counters()["applied"] == 2


# ------------------------------------------------------------------------------------------- 8. a captured iteration
def graph_edges(raw_graph):
    """(number of nodes, [(from, to)] node handles) of a captured graph, from the HIP runtime the process has loaded."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    graph, n = ctypes.c_void_p(raw_graph), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = n.value
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(n)) == 0
    src, dst = (ctypes.c_void_p * n.value)(), (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(n)) == 0
    return nodes, list(zip(src[:n.value], dst[:n.value]))


def test_a_whole_iteration_captured_and_replayed(torch, data):
    from heligym_amd import HeliVecEnv, PPOOptState
    K, n, iters = 8, 64, 3
    v = data.dev
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)   # noqa: E731
    u8 = lambda: torch.empty((K, n), dtype=torch.uint8, device=DEV)   # noqa: E731

    def make():
        env = HeliVecEnv(n, task="hover", dt=0.01, device=DEV, seed=3, autoreset=True, max_episode_steps=5)
        h = types.SimpleNamespace(env=env, P=dev_params(torch, data.theta), S=PPOOptState(DEV))
        env.set_policy_theta(h.P, v.mean, v.scale)
        h.obs0 = env.reset()[0].clone()
        h.out = dict(actions=f32(K, n, 4), obs=f32(K, n, 17), reward=f32(K, n), terminated=u8(), truncated=u8(), info=u8(),
                     logp=f32(K, n), value=f32(K, n), next_value=f32(K, n), advantages=f32(K, n), returns=f32(K, n))
        h.obs_in, h.index, h.stats = f32(K, n, 17), torch.empty((K * n,), dtype=torch.int32, device=DEV), f32(4, 8)
        # every kernel of the iteration has run once before a capture; on a scratch state, the env as it was
        s0, c0 = env.get_state()
        env.rollout_actor_critic(K, obs0=h.obs0, out=h.out)
        env.ppo_update(dev_params(torch, data.theta), PPOOptState(DEV), h.obs_in.zero_(), h.out["actions"], h.out["logp"],
                       h.out["advantages"], h.out["returns"], epochs=1, minibatches=1, index=h.index, stats=f32(1, 8),
                       **loss_kw(data))
        env.set_state(s0, c0)
        return h

    def iteration(h):
        out = h.env.rollout_actor_critic(K, obs0=h.obs0, out=h.out)
        h.obs_in[0].copy_(h.obs0)
        h.obs_in[1:].copy_(out["obs"][:-1])
        h.env.ppo_update(h.P, h.S, h.obs_in, out["actions"], out["logp"], out["advantages"], out["returns"], epochs=2,
                         minibatches=2, seed=31, index=h.index, stats=h.stats, lr=LR, betas=BETAS, eps=EPS,
                         max_grad_norm=0.5, publish=True, **loss_kw(data))
        h.obs0.copy_(out["obs"][-1])

    eager, graphed = make(), make()
    _assert_same(torch, eager.obs0, graphed.obs0, "the two handles start alike")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=side):
        iteration(graphed)
    nodes, edges = graph_edges(g.raw_cuda_graph())
    # rollout, GAE, two copies, the clear, 2 x (shuffle, 2 x (gradient, reduction, optimiser)), two packs, a copy
    assert nodes >= 22 and len(edges) == nodes - 1, (nodes, len(edges))
    assert len({a for a, _ in edges}) == len(edges) == len({b for _, b in edges}), "a node with two successors or predecessors"
    g.instantiate()
    perms = []
    for it in range(iters):
        iteration(eager)
        g.replay()
        torch.cuda.synchronize()
        _assert_same(torch, graphed.index, eager.index, f"iteration {it}: permutation")
        perms.append(eager.index.cpu().numpy().copy())
    assert not any(np.array_equal(perms[a], perms[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    assert eager.S.counters()["seen"] == 4 * iters == eager.S.counters()["applied"]
    _assert_same(torch, graphed.P.theta, eager.P.theta, "theta")
    _assert_same(torch, graphed.S.state, eager.S.state, "optimiser state")
    _assert_same(torch, graphed.obs0, eager.obs0, "last observations")
    _assert_same(torch, graphed.stats, eager.stats, "stats rows")
    for a, b, what in zip(graphed.env.get_state(), eager.env.get_state(), ("env state", "env counters")):
        _assert_same(torch, a, b, what)
    assert not torch.equal(eager.P.theta.cpu(), data.theta)
    eager.env.close()
    graphed.env.close()


# ------------------------------------------------------------------------------------------- 9. set_policy_theta
def test_set_policy_theta_is_set_policy_and_set_value_head(torch, data, env):
    v, p = data.dev, data.params
    obs = env.reset()[0].clone()
    env.set_policy(p.actor, log_std=p.log_std.detach(), obs_mean=v.mean, obs_scale=v.scale)
    env.set_value_head(p.critic)
    want = [x.clone() for x in env.policy_evaluate(obs)]
    other = dev_params(torch, 0.5 * data.theta)
    env.set_policy_theta(other)
    scrubbed = env.policy_evaluate(obs)
    assert not torch.equal(scrubbed[0], want[0]) and not torch.equal(scrubbed[2], want[2])
    env.set_policy_theta(dev_params(torch, data.theta), v.mean, v.scale)
    for a, b, what in zip(env.policy_evaluate(obs), want, ("actions", "logp", "value")):
        _assert_same(torch, a, b, what)


# ------------------------------------------------------------------------------------------- 10. errors
def test_errors_leave_everything_untouched(torch, data, env):
    from heligym_amd import _abi
    lib, v = env.lib, data.dev
    env.reset()
    s0, c0 = env.get_state()
    theta = torch.full((5641,), -7.0, device=DEV)
    grad = torch.full((5641,), -7.0, device=DEV)
    state = torch.full((11312 + 4,), -7, dtype=torch.int32, device=DEV)
    index = torch.full((B + 4,), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((6, 8), -7.0, device=DEV)
    lr_dev = torch.full((2,), 1e-3, device=DEV)
    ws = torch.empty((lib.hg_ppo_grad_workspace_bytes() + 16,), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)   # noqa: E731
    nan, inf = float("nan"), float("inf")

    def cfg(**kw):
        d = dict(dict(lr=3e-4, lr_dev=None, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.5, target_kl=0.0), **kw)
        return ctypes.byref(_abi.hg_ppo_opt_cfg(*d.values()))

    bad_cfgs = {"lr < 0": dict(lr=-1e-3), "lr nan": dict(lr=nan), "lr inf": dict(lr=inf), "beta1 1": dict(beta1=1.0),
                "beta1 < 0": dict(beta1=-0.1), "beta2 1": dict(beta2=1.0), "beta2 nan": dict(beta2=nan),
                "eps < 0": dict(eps=-1e-8), "eps inf": dict(eps=inf), "max_grad_norm nan": dict(max_grad_norm=nan),
                "target_kl nan": dict(target_kl=nan), "lr_dev 2 bytes off": dict(lr_dev=lr_dev.data_ptr() + 2)}
    calls = []   # (name, function, arguments)

    good = dict(env=env._h, B=B, seed=1, epoch=0, epoch_dev=None, out=p(index), stream=env._stream())
    for name, ch in {"NULL env": dict(env=None), "NULL out": dict(out=None), "out 2 bytes off": dict(out=off(index, 2)),
                     "epoch_dev 2 bytes off": dict(epoch_dev=off(state, 2)), "B 0": dict(B=0), "B < 0": dict(B=-5),
                     "B too large": dict(B=2 ** 31 - 255)}.items():
        calls.append(("shuffle: " + name, lib.hg_ppo_shuffle, dict(good, **ch)))
    assert lib.hg_ppo_shuffle(*dict(good, B=8, epoch_dev=off(state, 4)).values()) == 0
    torch.cuda.synchronize()
    assert sorted(index[:8].tolist()) == list(range(8)) and bool((index[8:] == -7).all())
    index.fill_(-7)

    good = dict(env=env._h, theta=p(theta), grad=p(grad), stats=p(stats), state=p(state), cfg=cfg(), stream=env._stream())
    changes = {"NULL env": dict(env=None), "NULL theta": dict(theta=None), "NULL grad": dict(grad=None),
               "NULL state": dict(state=None), "NULL cfg": dict(cfg=None), "theta 2 bytes off": dict(theta=off(theta, 2)),
               "grad 1 byte off": dict(grad=off(grad, 1)), "stats 2 bytes off": dict(stats=off(stats, 2)),
               "state 8 bytes off": dict(state=off(state, 8))}
    changes.update({k: dict(cfg=cfg(**c)) for k, c in bad_cfgs.items()})
    for name, ch in changes.items():
        calls.append(("adam: " + name, lib.hg_ppo_adam, dict(good, **ch)))

    good = dict(env=env._h, theta=p(theta), mean=p(v.mean), scale=p(v.scale), obs=p(v.obs), act=p(v.actions),
                lp=p(v.logp_old), adv=p(v.adv), ret=p(v.ret), B=B, clip=0.2, vf=0.5, ent=0.01, grad=p(grad), ws=p(ws),
                epochs=2, minibatches=3, seed=1, index=p(index), stats=p(stats), state=p(state), cfg=cfg(),
                stream=env._stream())
    changes = {"NULL env": dict(env=None), "B 0": dict(B=0), "B too large": dict(B=2 ** 31 - 255), "clip 0": dict(clip=0.0),
               "clip nan": dict(clip=nan), "vf < 0": dict(vf=-0.5), "ent inf": dict(ent=inf), "epochs 0": dict(epochs=0),
               "minibatches 0": dict(minibatches=0), "minibatches > B": dict(minibatches=B + 1),
               "actions 4 bytes off": dict(act=off(v.actions, 4)), "workspace 8 bytes off": dict(ws=off(ws, 8)),
               "index 2 bytes off": dict(index=off(index, 2)), "stats 1 byte off": dict(stats=off(stats, 1)),
               "state 4 bytes off": dict(state=off(state, 4)), "NULL cfg": dict(cfg=None),
               "target_kl without stats": dict(stats=None, cfg=cfg(target_kl=0.02))}
    for k in ("theta", "obs", "act", "lp", "adv", "ret", "grad", "ws", "index", "state"):
        changes[f"NULL {k}"] = {k: None}
    changes.update({k: dict(cfg=cfg(**c)) for k, c in bad_cfgs.items()})
    for name, ch in changes.items():
        calls.append(("update: " + name, lib.hg_ppo_update, dict(good, **ch)))

    for name, ch in {"NULL env": (None, p(state), None), "NULL state": (env._h, None, None),
                     "state 4 bytes off": (env._h, off(state, 4), None)}.items():
        calls.append(("opt_init: " + name, lib.hg_ppo_opt_init, dict(enumerate(ch))))
    for name, ch in {"NULL env": (None, p(theta), None, None, None), "NULL theta": (env._h, None, None, None, None),
                     "theta 2 bytes off": (env._h, off(theta, 2), None, None, None),
                     "mean 2 bytes off": (env._h, p(theta), off(v.mean, 2), None, None)}.items():
        calls.append(("set_policy_theta: " + name, lib.hg_set_policy_theta, dict(enumerate(ch))))

    for name, fn, args in calls:
        assert lib.hg_set_max_time(None, 1.0) == -1   # (leaves its own message behind)
        before = lib.hg_last_error()
        assert fn(*args.values()) == -1, name
        msg = lib.hg_last_error()
        assert msg and msg != before, name   # the refusal wrote a message of its own
    torch.cuda.synchronize()
    assert bool((theta == -7.0).all()) and bool((grad == -7.0).all()) and bool((stats == -7.0).all())
    assert bool((state == -7).all()) and bool((index == -7).all())
    s1, c1 = env.get_state()
    _assert_same(torch, s0, s1, "env state")
    _assert_same(torch, c0, c1, "env counters")
    # and the good calls pass: init zeroes exactly the state's bytes, NULL stats / mean / scale are allowed
    assert lib.hg_ppo_opt_init(env._h, p(state), env._stream()) == 0
    torch.cuda.synchronize()
    assert int(state[:11312].abs().max()) == 0 and bool((state[11312:] == -7).all())
    theta.copy_(data.theta)
    assert lib.hg_ppo_update(*dict(good, mean=None, scale=None, stats=None).values()) == 0
    assert lib.hg_ppo_update(*good.values()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(theta).all()) and int(state[11296]) == 12 and bool((index[B:] == -7).all())
