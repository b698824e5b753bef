"""GPU: the fused imitation gradient (hg_bc_grad, HeliVecEnv.bc_grad) and its update phase (hg_bc_update).

  1. values: the gradient and the statistics of both modes, with and without weights, against
     heligym_amd.policy.bc_loss in float64 on the CPU, by test_gpu_ppo_grad.py's rule (check_values, imported);
  2. exact properties no tolerance covers: MSE leaves log_std the entropy term alone, zero weights leave nothing
     else, NLL's weighted term is minus the mean log-probability, weight=None is a tensor of ones;
  3. an index is bitwise the materialised rows; out-of-range entries are skipped and counted; the same past the
     reduction's batch and the block cap (test_gpu_ppo_grad.py's table of sizes);
  4. determinism, and a captured call replayed on changed weights;
  5. bc_update is bitwise its parts, refuses a KL stop, and brings the squared action error down;
  6. argument errors leave the outputs, the weights and the optimiser state untouched.

Inputs follow test_gpu_ppo_grad.py's recipe (make_data, imported): B = 4200 golden observation rows, a seeded
random student, targets = the actions of a perturbed copy of the weights plus its noise; weights uniform in
[0, 2] with about a tenth exactly 0; value targets one unit above the untrained critic, for the reason that
file's comment gives.  Run with -m gpu."""
import ctypes
import types

import numpy as np
import pytest

from test_gpu_policy_rollout import _assert_same
from test_gpu_ppo_grad import B, OUT_OF_RANGE, SIZES, check_values, dev_params, make_data

pytestmark = pytest.mark.gpu

VF, ENT = 0.5, 0.01
DEV = "cuda:0"
MODES = ("nll", "mse")
LS = slice(5572, 5576)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


@pytest.fixture(scope="module")
def data(torch):
    d = make_data()
    g = torch.Generator().manual_seed(303)
    w = 2.0 * torch.rand((B,), generator=g)
    w[torch.rand((B,), generator=g) < 0.1] = 0.0
    w[0] = 1.25   # the lone row of M = 1 counts
    assert 0.05 <= float((w == 0).double().mean()) <= 0.15
    d.target, d.weight, d.y = d.actions, w, d.ret
    d.dev = types.SimpleNamespace(**{k: getattr(d, k).to(DEV) for k in ("obs", "target", "weight", "y", "mean", "scale")})
    d.theta = d.params.theta.detach().clone()   # (CPU, float32: the weights every test starts from)
    d.refs = {}
    return d


@pytest.fixture(scope="module")
def env(torch):
    from heligym_amd import HeliVecEnv
    e = HeliVecEnv(64, task="hover", dt=0.01, device=DEV, seed=3, autoreset=True, max_episode_steps=5)
    yield e
    e.close()


def loss_on(torch, d, theta, rows, dtype, mode, weighted, vf=VF, ent=ENT, divisor=None):
    """bc_loss of the stored rows `rows` (a LongTensor) in `dtype` on the CPU: (gradient, stats).  divisor: the M
    the means divide by when it is not len(rows) (skipped index entries)."""
    from heligym_amd.policy import LOG_2PI, bc_loss, ppo_views
    c = lambda t: t[rows].to(dtype)   # noqa: E731
    th = theta.detach().cpu().to(dtype).clone().requires_grad_(True)
    L, stats = bc_loss(th, c(d.obs), c(d.target), c(d.weight) if weighted else None, c(d.y), mode, vf, ent,
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


def refs_of(torch, d, key, rows, mode, weighted, divisor=None):
    """(float64 gradient, float64 stats, float32 CPU gradient, float32 CPU stats), computed once per key."""
    key = (key, mode, weighted)
    if key not in d.refs:
        d.refs[key] = (loss_on(torch, d, d.theta, rows, torch.float64, mode, weighted, divisor=divisor)
                       + loss_on(torch, d, d.theta, rows, torch.float32, mode, weighted, divisor=divisor))
    return d.refs[key]


def run(torch, env, d, theta, mode, weighted, rows=None, index=None, **kw):
    """bc_grad on the first `rows` stored rows (all B when None) -> (grad, stats) on the CPU."""
    P = dev_params(torch, theta)
    s = slice(None) if rows is None else slice(0, rows)
    v = d.dev
    kw = dict(dict(vf_coef=VF, ent_coef=ENT, obs_mean=v.mean, obs_scale=v.scale), **kw)
    w = kw.pop("weight", v.weight if weighted else None)
    g, st = env.bc_grad(P, v.obs[s], v.target[s], weight=None if w is None else w[s], value_target=v.y[s], index=index,
                        mode=mode, **kw)
    torch.cuda.synchronize()
    return g.cpu(), st.cpu()


# ------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("weighted", (True, False), ids=("weights", "w = 1"))
@pytest.mark.parametrize("mode", MODES)
def test_values_against_float64(torch, data, env, mode, weighted, m):
    print()
    got, st = run(torch, env, data, data.theta, mode, weighted, rows=m)
    ref = refs_of(torch, data, m, torch.arange(m), mode, weighted)
    assert float(ref[0].abs().max()) > 1e-3   # a non-trivial gradient
    check_values(torch, f"{mode}, {'weights' if weighted else 'w = 1'}, M={m}", got, st, ref)
    assert float(st[7]) == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_values_without_normalisation(torch, data, env, mode):
    """obs_mean = obs_scale = NULL: the rows are the module's, normalised beforehand in float32 on the CPU."""
    m = 65   # two tiles, the second one lane
    x = (data.obs - data.mean) * data.scale
    d = types.SimpleNamespace(**dict(vars(data), obs=x, mean=None, scale=None))
    v = data.dev
    P = dev_params(torch, data.theta)
    got, st = env.bc_grad(P, x[:m].to(DEV), v.target[:m], weight=v.weight[:m], value_target=v.y[:m], mode=mode,
                          vf_coef=VF, ent_coef=ENT, obs_mean=None, obs_scale=None)
    torch.cuda.synchronize()
    rows = torch.arange(m)
    ref = (loss_on(torch, d, data.theta, rows, torch.float64, mode, True)
           + loss_on(torch, d, data.theta, rows, torch.float32, mode, True))
    assert float(ref[0].abs().max()) > 1e-3
    print()
    check_values(torch, f"{mode}, M={m}, no mean / scale", got.cpu(), st.cpu(), ref)
    assert float(st[7]) == 0.0


# ------------------------------------------------------------------------------------------- 2. exact properties
@pytest.mark.parametrize("m", (200, 4099))
def test_mse_leaves_log_std_the_entropy_term(torch, data, env, m):
    got, _ = run(torch, env, data, data.theta, "mse", True, rows=m)
    _assert_same(torch, got[LS], torch.full((4,), -ENT), "d L / d log_std")
    got, _ = run(torch, env, data, data.theta, "mse", True, rows=m, ent_coef=0.0)
    assert bool((got[LS] == 0).all())


@pytest.mark.parametrize("mode", MODES)
def test_zero_weights_leave_only_the_entropy_term(torch, data, env, mode):
    m = 4099
    got, st = run(torch, env, data, data.theta, mode, True, rows=m, weight=torch.zeros((B,), device=DEV), vf_coef=0.0)
    want = torch.zeros(5641)
    want[LS] = -ENT
    assert bool((got == want).all()), int((got != want).sum())
    assert float(st[0]) == 0.0 and float(st[3]) == 0.0 and float(st[2]) > 0.0


@pytest.mark.parametrize("m", (65, 4099))
def test_nll_without_weights_is_minus_the_mean_logp(torch, data, env, m):
    _, st = run(torch, env, data, data.theta, "nll", False, rows=m)
    assert float(st[0]) != 0.0
    _assert_same(torch, st[0:1], -st[6:7], "stats[0] against -stats[6]")
    assert float(st[3]) == float(np.float32(m) * (np.float32(1.0) / np.float32(m)))   # m ones, times the float32 1 / m


@pytest.mark.parametrize("mode", MODES)
def test_no_weights_is_a_tensor_of_ones(torch, data, env, mode):
    m = 4099
    a, sa = run(torch, env, data, data.theta, mode, False, rows=m)
    b, sb = run(torch, env, data, data.theta, mode, True, rows=m, weight=torch.ones((B,), device=DEV))
    _assert_same(torch, a, b, "gradient")
    _assert_same(torch, sa, sb, "stats")


# ------------------------------------------------------------------------------------------- 3. index
def materialised(torch, env, d, mode, di):
    v = d.dev
    P = dev_params(torch, d.theta)
    g, s = env.bc_grad(P, v.obs[di].contiguous(), v.target[di].contiguous(), weight=v.weight[di].contiguous(),
                       value_target=v.y[di].contiguous(), mode=mode, vf_coef=VF, ent_coef=ENT, obs_mean=v.mean,
                       obs_scale=v.scale)
    torch.cuda.synchronize()
    return g.cpu(), s.cpu()


@pytest.mark.parametrize("mode", MODES)
def test_index_is_bitwise_the_materialised_rows(torch, data, env, mode):
    g = torch.Generator().manual_seed(9)
    idx = torch.randperm(B, generator=g)
    a, sa = run(torch, env, data, data.theta, mode, True, index=idx.to(torch.int32).to(DEV))
    gm, sm = materialised(torch, env, data, mode, idx.to(DEV))
    _assert_same(torch, a, gm, "gradient")
    _assert_same(torch, sa, sm, "stats")
    # four entries that name no row: skipped and counted, the means still over M
    cut = (0, 100, 500, B)
    parts = [idx[cut[0]:cut[1]], idx[cut[1]:cut[2]], idx[cut[2]:cut[3]]]
    bad = torch.cat([torch.tensor(OUT_OF_RANGE[:1]), parts[0], torch.tensor(OUT_OF_RANGE[1:2]), parts[1],
                     torch.tensor(OUT_OF_RANGE[2:3]), parts[2], torch.tensor(OUT_OF_RANGE[3:])])
    got, st = run(torch, env, data, data.theta, mode, True, index=bad.to(torch.int32).to(DEV))
    assert float(st[7]) == 4.0
    ref = refs_of(torch, data, "planted permutation", idx, mode, True, divisor=len(bad))
    print()
    check_values(torch, f"{mode}, a permutation with 4 of {len(bad)} out of range", got, st, ref)


# test_gpu_ppo_grad.py's table: 16 385 = 257 tiles on 65 blocks, the reduction's batch of sixteen plus one term and a
# block of one wave with one valid lane; 65 666 = 1 027 tiles on the cap of 256 blocks, three waves' second tile
@pytest.mark.parametrize("m", (16385, 65666))
@pytest.mark.parametrize("mode", MODES)
def test_large_index_values_counts_and_materialised_rows(torch, data, env, mode, m):
    g = torch.Generator().manual_seed(1000 + m)
    clean = torch.randint(0, B, (m,), generator=g, dtype=torch.int64)
    where = [0, 127, 1024 * 64 + 35 if m > 1025 * 64 else 5 * 64 + 35, m - 1]
    planted = clean.clone()
    planted[where] = torch.tensor(OUT_OF_RANGE)
    keep = torch.ones(m, dtype=torch.bool)
    keep[where] = False
    print()
    got, st = run(torch, env, data, data.theta, mode, True, index=planted.to(torch.int32).to(DEV))
    check_values(torch, f"{mode}, M={m} by index, 4 out of range", got, st,
                 refs_of(torch, data, ("planted", m), clean[keep], mode, True, divisor=m))
    assert float(st[7]) == len(OUT_OF_RANGE)
    a, sa = run(torch, env, data, data.theta, mode, True, index=clean.to(torch.int32).to(DEV))
    check_values(torch, f"{mode}, M={m} by index", a, sa, refs_of(torch, data, ("clean", m), clean, mode, True))
    assert float(sa[7]) == 0.0
    gm, sm = materialised(torch, env, data, mode, clean.to(DEV))
    _assert_same(torch, a, gm, "gradient")
    _assert_same(torch, sa, sm, "stats")


# ------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("mode", MODES)
def test_deterministic_and_replayed_on_changed_weights(torch, data, env, mode):
    m = 4099
    v = data.dev
    a, sa = run(torch, env, data, data.theta, mode, True, rows=m)
    b, sb = run(torch, env, data, data.theta, mode, True, rows=m)
    _assert_same(torch, a, b, "two eager calls")
    _assert_same(torch, sa, sb, "two eager calls' stats")
    P = dev_params(torch, data.theta)
    stats = torch.empty((8,), dtype=torch.float32, device=DEV)
    kw = dict(weight=v.weight[:m], value_target=v.y[:m], mode=mode, vf_coef=VF, ent_coef=ENT, obs_mean=v.mean,
              obs_scale=v.scale, stats=stats)
    env.bc_grad(P, v.obs[:m], v.target[:m], **kw)   # (the workspace exists before the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        env.bc_grad(P, v.obs[:m], v.target[:m], **kw)
    g.replay()
    torch.cuda.synchronize()
    _assert_same(torch, P.grad.cpu(), a, "replay 1")
    _assert_same(torch, stats.cpu(), sa, "replay 1 stats")
    gen = torch.Generator().manual_seed(4)
    theta2 = data.theta + 0.01 * torch.randn((5641,), generator=gen)
    P.theta.copy_(theta2)   # in place: the graph reads the same buffer
    g.replay()
    torch.cuda.synchronize()
    c, sc = run(torch, env, data, theta2, mode, True, rows=m)
    assert not torch.equal(c, a)
    _assert_same(torch, P.grad.cpu(), c, "replay 2")
    _assert_same(torch, stats.cpu(), sc, "replay 2 stats")


# ------------------------------------------------------------------------------------------- 5. bc_update
OPT = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.5)


def fresh(torch, d):
    from heligym_amd import PPOOptState
    return dev_params(torch, d.theta), PPOOptState(DEV)


@pytest.mark.parametrize("mode", MODES)
def test_update_is_bitwise_its_parts(torch, data, env, mode):
    epochs, minibatches, n = 2, 3, B
    v = data.dev
    kw = dict(weight=v.weight, value_target=v.y, mode=mode, vf_coef=VF, ent_coef=ENT, obs_mean=v.mean, obs_scale=v.scale)
    P1, S1 = fresh(torch, data)
    ix1 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    st1 = env.bc_update(P1, S1, v.obs, v.target, epochs=epochs, minibatches=minibatches, seed=11, index=ix1, publish=False,
                        **kw, **OPT)
    assert st1.shape == (epochs * minibatches, 8)
    P2, S2 = fresh(torch, data)
    ix2 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    st2 = torch.full((epochs * minibatches, 8), float("nan"), device=DEV)
    cuts = [j * n // minibatches for j in range(minibatches + 1)]
    assert [b - a for a, b in zip(cuts, cuts[1:])] == [1400, 1400, 1400]
    for ep in range(epochs):
        env.ppo_shuffle(n, 11, epoch=0, epoch_dev=S2.seen, out=ix2)
        for j in range(minibatches):
            row = st2[ep * minibatches + j]
            env.bc_grad(P2, v.obs, v.target, index=ix2[cuts[j]:cuts[j + 1]], stats=row, **kw)
            env.ppo_adam(P2, S2, stats=row, **OPT)
    torch.cuda.synchronize()
    _assert_same(torch, P1.theta, P2.theta, "theta")
    _assert_same(torch, S1.state, S2.state, "optimiser state")
    _assert_same(torch, st1, st2, "stats rows")
    _assert_same(torch, ix1, ix2, "index")
    c = S1.counters()
    assert c["applied"] == c["seen"] == epochs * minibatches and c["stop"] == 0
    assert torch.isfinite(st1).all() and not torch.equal(P1.theta.cpu(), data.theta)


def test_update_refuses_a_kl_stop(torch, data, env):
    from heligym_amd import _abi
    lib, v = env.lib, data.dev
    P, S = fresh(torch, data)
    theta0, state0 = P.theta.clone(), S.state.clone()
    P.grad.fill_(-7.0)
    stats = torch.full((6, 8), -7.0, device=DEV)
    index = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty((lib.hg_ppo_grad_workspace_bytes(),), dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for kl, rc in ((0.02, -1), (0.0, 0)):
        cfg = _abi.hg_ppo_opt_cfg(3e-4, None, 0.9, 0.999, 1e-8, 0.5, kl)
        assert lib.hg_set_max_time(None, 1.0) == -1   # (leaves its own message behind)
        got = lib.hg_bc_update(env._h, p(P.theta), p(v.mean), p(v.scale), p(v.obs), p(v.target), p(v.weight), p(v.y), B,
                               _abi.HG_BC_NLL, VF, ENT, p(P.grad), p(ws), 2, 3, 1, p(index), p(stats), p(S.state),
                               ctypes.byref(cfg), env._stream())
        assert got == rc, kl
        torch.cuda.synchronize()
        if rc:
            assert b"target_kl" in lib.hg_last_error()
            _assert_same(torch, P.theta, theta0, "theta")
            _assert_same(torch, S.state, state0, "optimiser state")
            assert bool((P.grad == -7.0).all()) and bool((stats == -7.0).all()) and bool((index == -7).all())
    assert S.counters()["applied"] == 6 and bool(torch.isfinite(stats).all())


def test_update_brings_the_action_error_down(torch, data, env):
    """8 epochs x 4 minibatches in MSE mode on a fixed teacher's mean actions: the last minibatch's mean squared
    action error is below the first's (a strict inequality, no threshold)."""
    from heligym_amd.policy import ppo_views
    v = data.dev
    g = torch.Generator().manual_seed(12)
    p = ppo_views(data.theta + 0.1 * torch.randn((5641,), generator=g))
    x = (data.obs - data.mean) * data.scale
    teacher = (torch.tanh(torch.tanh(x @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"]) @ p["W3"].T + p["b3"]).contiguous()
    P, S = fresh(torch, data)
    st = env.bc_update(P, S, v.obs, teacher.to(DEV), epochs=8, minibatches=4, seed=5, mode="mse", obs_mean=v.mean,
                       obs_scale=v.scale, lr=1e-3, publish=False)
    torch.cuda.synchronize()
    st = st.cpu()
    print(f"\n[bc_update] mean squared action error: first minibatch {float(st[0, 2]):.4e}, last {float(st[-1, 2]):.4e}")
    assert st.shape == (32, 8) and bool(torch.isfinite(st).all())
    assert float(st[-1, 2]) < float(st[0, 2])
    assert S.counters()["applied"] == 32


def test_update_publishes(torch, data):
    """publish=True (the default) ends with set_policy_theta: the env acts with the updated weights."""
    from heligym_amd import HeliVecEnv
    v = data.dev
    e = HeliVecEnv(64, task="hover", dt=0.01, device=DEV, seed=3)
    try:
        P, S = fresh(torch, data)
        e.bc_update(P, S, v.obs, v.target, epochs=1, minibatches=2, seed=5, mode="mse", obs_mean=v.mean, obs_scale=v.scale)
        obs = e.reset()[0].clone()
        a = e.policy_act_mean(obs).clone()
        e.set_policy_theta(P, v.mean, v.scale)
        _assert_same(torch, a, e.policy_act_mean(obs), "actions of the published weights")
    finally:
        e.close()


# ------------------------------------------------------------------------------------------- 6. errors
def test_errors_leave_everything_untouched(torch, data, env):
    from heligym_amd import _abi
    lib, v = env.lib, data.dev
    m = 200
    env.reset()
    s0, c0 = env.get_state()
    theta = data.theta.to(DEV).clone()
    theta0 = theta.clone()
    grad = torch.full((5641,), -7.0, device=DEV)
    stats = torch.full((6, 8), -7.0, device=DEV)
    state = torch.full((11312,), -7, dtype=torch.int32, device=DEV)
    index = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty((lib.hg_ppo_grad_workspace_bytes() + 16,), dtype=torch.uint8, device=DEV)
    idx = torch.arange(m, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)   # noqa: E731
    nan, inf = float("nan"), float("inf")
    cfg = lambda kl=0.0: ctypes.byref(_abi.hg_ppo_opt_cfg(3e-4, None, 0.9, 0.999, 1e-8, 0.5, kl))   # noqa: E731
    # (case, the change, a word of the message: the argument it names)
    shared = [("NULL env", dict(env=None), "env"), ("B < 1", dict(B=0), "B"), ("mode 2", dict(mode=2), "mode"),
              ("mode -1", dict(mode=-1), "mode"), ("vf < 0", dict(vf=-0.5), "vf_coef"), ("vf inf", dict(vf=inf), "vf_coef"),
              ("ent < 0", dict(ent=-0.01), "ent_coef"), ("ent nan", dict(ent=nan), "ent_coef"),
              ("no value target, vf != 0", dict(y=None), "value_target"),
              ("target 4 bytes off", dict(target=off(v.target, 4)), "target"),
              ("workspace 8 bytes off", dict(ws=off(ws, 8)), "workspace"),
              ("theta 2 bytes off", dict(theta=off(theta, 2)), "pointer"),
              ("weight 2 bytes off", dict(weight=off(v.weight, 2)), "pointer"),
              ("value target 1 byte off", dict(y=off(v.y, 1)), "pointer"),
              ("stats 1 byte off", dict(stats=off(stats, 1)), "pointer")]
    for k in ("theta", "obs", "target", "grad"):
        shared.append((f"NULL {k}", {k: None}, k))
    shared.append(("NULL ws", dict(ws=None), "workspace"))
    good = dict(env=env._h, theta=p(theta), mean=p(v.mean), scale=p(v.scale), obs=p(v.obs), target=p(v.target),
                weight=p(v.weight), y=p(v.y), B=B, index=p(idx), M=m, mode=_abi.HG_BC_MSE, vf=0.5, ent=0.01, grad=p(grad),
                stats=p(stats), ws=p(ws), stream=env._stream())
    calls = [("grad: " + n, lib.hg_bc_grad, dict(good, **ch), word) for n, ch, word in shared]
    calls += [("grad: " + n, lib.hg_bc_grad, dict(good, **ch), word) for n, ch, word in (
        ("M < 1", dict(M=0), "M"), ("M too large", dict(M=2 ** 31 - 255), "M"), ("no index, M != B", dict(index=None), "index"),
        ("index 2 bytes off", dict(index=off(idx, 2)), "pointer"))]
    good_up = dict(env=env._h, theta=p(theta), mean=p(v.mean), scale=p(v.scale), obs=p(v.obs), target=p(v.target),
                   weight=p(v.weight), y=p(v.y), B=B, mode=_abi.HG_BC_MSE, vf=0.5, ent=0.01, grad=p(grad), ws=p(ws), epochs=2,
                   minibatches=3, seed=1, index=p(index), stats=p(stats), state=p(state), cfg=cfg(), stream=env._stream())
    calls += [("update: " + n, lib.hg_bc_update, dict(good_up, **ch), word) for n, ch, word in shared]
    calls += [("update: " + n, lib.hg_bc_update, dict(good_up, **ch), word) for n, ch, word in (
        ("epochs 0", dict(epochs=0), "n_epochs"), ("minibatches 0", dict(minibatches=0), "n_minibatches"),
        ("minibatches > B", dict(minibatches=B + 1), "n_minibatches"), ("NULL index", dict(index=None), "index"),
        ("NULL state", dict(state=None), "state"), ("state 4 bytes off", dict(state=off(state, 4)), "state"),
        ("NULL cfg", dict(cfg=None), "cfg"), ("target_kl 0.02", dict(cfg=cfg(0.02)), "target_kl"))]
    for name, fn, args, word in calls:
        assert lib.hg_set_max_time(None, 1.0) == -1   # (leaves its own message behind)
        before = lib.hg_last_error()
        assert fn(*args.values()) == -1, name
        msg = lib.hg_last_error()
        assert msg and msg != before and word.encode() in msg, (name, msg)
    torch.cuda.synchronize()
    assert bool((grad == -7.0).all()) and bool((stats == -7.0).all())
    assert bool((state == -7).all()) and bool((index == -7).all())
    _assert_same(torch, theta, theta0, "theta")
    # the good calls pass (and NULL mean / scale / stats / weight are allowed, a NULL value target with vf_coef 0)
    assert lib.hg_bc_grad(*good.values()) == 0
    assert lib.hg_bc_grad(*dict(good, mean=None, scale=None, stats=None, weight=None, y=None, vf=0.0).values()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all())
    _assert_same(torch, theta, theta0, "theta after the gradient calls")
    s1, c1 = env.get_state()
    _assert_same(torch, s0, s1, "env state")
    _assert_same(torch, c0, c1, "env counters")
