"""CPU-side checks of the imitation loss's surface (hg_bc_grad, hg_bc_update, hg_mppi_value): the symbols are
exported and declared with the header's argument counts and refuse a NULL env; heligym_amd.policy.bc_loss, the
statement of the function the kernel differentiates, is checked in float64 against central finite differences
and for the exact relations its statistics promise; HeliVecEnv's wrappers refuse bad arguments with ValueError
before the library is called.  No device calls."""
import ctypes

import numpy as np
import pytest
import torch

from test_branch_host import _bare_env
from test_policy_host import header_arg_counts

from heligym_amd import ActorCriticParams, PPOOptState, _abi, bc_loss, policy

NEW = {"hg_bc_grad": 18, "hg_bc_update": 22, "hg_mppi_value": 8}
M = 37


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    for name, n in NEW.items():
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == n, name
    assert lib.hg_abi_version() == 3   # purely additive
    assert (_abi.HG_BC_NLL, _abi.HG_BC_MSE) == (0, 1) and _abi.BC_MODES == {"nll": 0, "mse": 1}


def test_calls_refuse_a_null_env(lib):
    cfg = _abi.hg_ppo_opt_cfg(3e-4, None, 0.9, 0.999, 1e-8, 0.5, 0.0)
    buf = (ctypes.c_float * 64)()   # 16-byte aligned or not, the NULL env is refused on its own message
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {"hg_bc_grad": (None,) + (p,) * 7 + (8, None, 8, 0, 0.0, 0.0, p, None, p, None),
             "hg_bc_update": (None,) + (p,) * 7 + (8, 0, 0.0, 0.0, p, p, 1, 1, 0, p, None, p, ctypes.byref(cfg), None),
             "hg_mppi_value": (None, p, 4, 1.0, p, None, None, None)}
    for name, args in calls.items():
        lib.hg_num_envs(None)
        assert getattr(lib, name)(*args) == -1, name
        assert b"env is NULL" in lib.hg_last_error(), name


def _problem(seed=5):
    """A seeded float64 student, rows, targets off the student's mean, weights with exact zeros, value targets."""
    g = torch.Generator().manual_seed(seed)
    theta = 0.3 * torch.randn((policy.PPO_N_PARAMS,), generator=g, dtype=torch.float64)
    theta[5572:5576] = torch.tensor([-1.0, -0.7, -1.3, -0.9], dtype=torch.float64)
    obs = torch.randn((M, 17), generator=g, dtype=torch.float64)
    target = torch.randn((M, 4), generator=g, dtype=torch.float64)
    weight = 2.0 * torch.rand((M,), generator=g, dtype=torch.float64)
    weight[::9] = 0.0
    y = torch.randn((M,), generator=g, dtype=torch.float64) + 1.0
    mean = 0.1 * torch.randn((17,), generator=g, dtype=torch.float64)
    scale = 0.5 + torch.rand((17,), generator=g, dtype=torch.float64)
    return theta, obs, target, weight, y, mean, scale


@pytest.mark.parametrize("mode", ("nll", "mse"))
@pytest.mark.parametrize("weighted", (False, True), ids=("w = 1", "weights"))
def test_bc_loss_against_central_differences(mode, weighted):
    theta, obs, target, weight, y, mean, scale = _problem()
    w = weight if weighted else None
    f = lambda th: bc_loss(th, obs, target, w, y, mode, 0.5, 0.01, mean, scale)   # noqa: E731
    th = theta.clone().requires_grad_(True)
    L, stats = f(th)
    L.backward()
    assert float(stats[5]) == float(L.detach()) and float(stats[7]) == 0.0
    g = torch.Generator().manual_seed(1)
    h = 1e-6
    for name, (off, shape) in policy.PPO_LAYOUT.items():
        n = int(np.prod(shape))
        for k in set(torch.randint(0, n, (5,), generator=g).tolist()) | {0, n - 1}:
            d = torch.zeros_like(theta)
            d[off + k] = h
            fd = float(f(theta + d)[0] - f(theta - d)[0]) / (2 * h)
            an = float(th.grad[off + k])
            # central differences in float64: truncation h^2 f''' / 6 and rounding eps |L| / h, both ~ 1e-10
            assert abs(fd - an) <= 1e-7 * max(1.0, abs(an)), (name, k, fd, an)


def test_bc_loss_exact_relations():
    theta, obs, target, weight, y, mean, scale = _problem()
    # NLL without weights: the weighted term is minus the mean log-probability, bitwise
    _, st = bc_loss(theta, obs, target, None, y, "nll", 0.5, 0.01, mean, scale)
    assert float(st[0]) == -float(st[6]) and float(st[3]) == 1.0
    # MSE: log_std sees only the entropy term
    th = theta.clone().requires_grad_(True)
    L, st = bc_loss(th, obs, target, weight, y, "mse", 0.5, 0.01, mean, scale)
    L.backward()
    assert th.grad[5572:5576].tolist() == [-0.01] * 4
    assert float(st[0]) != float(st[2]) and float(st[3]) == float(weight.mean())
    # no value target: no value term, and a value coefficient is refused
    th = theta.clone().requires_grad_(True)
    L, st = bc_loss(th, obs, target, weight, None, "nll", 0.0, 0.0)
    L.backward()
    assert float(st[1]) == 0.0 and float(th.grad[5576:].abs().max()) == 0.0
    with pytest.raises(ValueError, match="vf_coef"):
        bc_loss(theta, obs, target, None, None, "nll", 0.5, 0.0)
    with pytest.raises(ValueError, match="mode"):
        bc_loss(theta, obs, target, None, y, "l1", 0.5, 0.0)
    # all weights zero and no value term: only the entropy term is left
    th = theta.clone().requires_grad_(True)
    L, _ = bc_loss(th, obs, target, torch.zeros_like(weight), y, "nll", 0.0, 0.01)
    L.backward()
    want = torch.zeros_like(theta)
    want[5572:5576] = -0.01
    assert torch.equal(th.grad, want)


def _params():
    nn = torch.nn
    torch.manual_seed(2)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
    return ActorCriticParams(actor, nn.Linear(64, 1), nn.Parameter(torch.full((4,), -1.0)))


def test_wrappers_validate_first():
    env = _bare_env(4)
    P, S = _params(), PPOOptState("cpu")
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)   # noqa: E731
    B = 12
    obs, tgt, w, y = z(B, 17), z(B, 4), z(B), z(B)
    for call in (lambda **kw: env.bc_grad(P, obs, tgt, **kw),
                 lambda **kw: env.bc_update(P, S, obs, tgt, epochs=1, minibatches=2, **kw)):
        with pytest.raises(ValueError, match="mode"):
            call(mode="l1")
        with pytest.raises(ValueError, match="vf_coef"):
            call(vf_coef=0.5)   # no value_target
        with pytest.raises(ValueError, match="vf_coef"):
            call(value_target=y, vf_coef=-1.0)
        with pytest.raises(ValueError, match="ent_coef"):
            call(ent_coef=float("nan"))
        with pytest.raises(ValueError, match="weight"):
            call(weight=z(B + 1))
        with pytest.raises(ValueError, match="weight"):
            call(weight=z(B, dtype=torch.float64))
        with pytest.raises(ValueError, match="value_target"):
            call(value_target=z(B, 1), vf_coef=0.5)
        with pytest.raises(ValueError, match="obs_mean"):
            call(obs_mean=z(16))
    with pytest.raises(ValueError, match="target"):
        env.bc_grad(P, obs, z(B, 3))
    with pytest.raises(ValueError, match="obs"):
        env.bc_grad(P, z(B, 16), tgt)
    with pytest.raises(ValueError, match="index"):
        env.bc_grad(P, obs, tgt, index=z(5))
    with pytest.raises(ValueError, match="stats"):
        env.bc_grad(P, obs, tgt, stats=z(7))

    class Half:
        theta, grad = z(5641), z(5640)
    with pytest.raises(ValueError, match="params.grad"):
        env.bc_grad(Half, obs, tgt)
    with pytest.raises(AssertionError, match="hg_ppo_grad_workspace_bytes|hg_bc_grad"):   # valid arguments reach the library
        env.bc_grad(P, obs, tgt, weight=w, value_target=y, vf_coef=0.5, mode="mse", index=z(5, dtype=torch.int32))

    with pytest.raises(TypeError):
        env.bc_update(P, S, obs, tgt, target_kl=0.02)   # no such keyword: this loss has no KL
    with pytest.raises(ValueError, match="epochs"):
        env.bc_update(P, S, obs, tgt, epochs=0, minibatches=2)
    for n in (0, B + 1):
        with pytest.raises(ValueError, match="minibatches"):
            env.bc_update(P, S, obs, tgt, epochs=1, minibatches=n)
    with pytest.raises(ValueError, match="state"):
        env.bc_update(P, None, obs, tgt, epochs=1, minibatches=2)
    with pytest.raises(ValueError, match="lr"):
        env.bc_update(P, S, obs, tgt, epochs=1, minibatches=2, lr=-1.0)
    with pytest.raises(ValueError, match="stats"):
        env.bc_update(P, S, obs, tgt, epochs=2, minibatches=3, stats=z(5, 8))
    with pytest.raises(AssertionError, match="hg_ppo_grad_workspace_bytes|hg_bc_update"):
        env.bc_update(P, S, obs, tgt, weight=w, value_target=y, vf_coef=0.5, epochs=2, minibatches=3, publish=False)

    G = z(4, 6)
    for b in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="branches"):
            env.mppi_value(G, b, 1.0)
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lam"):
            env.mppi_value(G, 6, lam)
    for wrong in (z(4, 5), z(5, 6), z(24), z(4, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="returns"):
            env.mppi_value(wrong, 6, 1.0)
    ok = dict(value=z(4), best=z(4), ess=z(4))
    for key, bad in (("value", z(5)), ("best", z(4, dtype=torch.float64)), ("ess", z(4, 1))):
        with pytest.raises(ValueError, match=key):
            env.mppi_value(G, 6, 1.0, out=dict(ok, **{key: bad}))
    with pytest.raises(AssertionError, match="hg_mppi_value"):
        env.mppi_value(G, 6, 1.0, out=ok)


def test_planner_value_needs_a_scored_set():
    from heligym_amd import MPPI
    planner = MPPI.__new__(MPPI)
    planner.scores = None
    with pytest.raises(ValueError, match="plan"):
        planner.value()
