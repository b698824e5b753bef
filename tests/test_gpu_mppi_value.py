"""GPU: what the planner thinks a state is worth (hg_mppi_value, HeliVecEnv.mppi_value, MPPI.value).

N = 3 envs; branches 1, 5, 64, 65 and 1025 (past HG_MPPI_LDS_BRANCHES = 1024: the weights are recomputed, not kept
in LDS).  Seeded returns; env 1 has a NaN, a +inf and a -inf planted (where there are branches enough), env 2 has
no finite return at all.

  1. value is bitwise hg_mppi_update's weighted mean of an action column that holds the returns (horizon 1);
  2. best is the largest finite return, exactly;
  3. ess against a float32 NumPy evaluation in the kernel's order, within (branches + 3) ulp;
  4. the env without a finite return gets (0, -inf, 0);
  5. refusals leave the outputs untouched;
  6. PolicyMPPI.value() after a plan() is mppi_value of the planner's scores.
Run with -m gpu."""
import ctypes

import numpy as np
import pytest

from test_gpu_branch_policy import _age, _bounds, _pair
from test_gpu_branch_rollout import DEV, _assert_same, _env, torch   # noqa: F401

pytestmark = pytest.mark.gpu

N = 3
BRANCHES = (1, 5, 64, 65, 1025)
LAM = 0.7


@pytest.fixture(scope="module")
def env(torch):
    e = _env(torch, N)
    yield e
    e.close()


def returns_of(branches):
    """[N, branches] float32: env 0 clean, env 1 with NaN / +inf / -inf planted, env 2 without a finite return."""
    rng = np.random.default_rng(100 + branches)
    G = (2.0 * rng.standard_normal((N, branches))).astype(np.float32)
    planted = [(0, np.nan), (2, np.inf), (3, -np.inf)]
    for b, v in planted:
        if b < branches - 1:   # (the last branch stays finite: env 1 always has a finite return)
            G[1, b] = v
    G[2] = np.resize(np.array([np.nan, -np.inf, np.inf], dtype=np.float32), branches)
    return G


def ess_ref(G, lam):
    """The kernel's chain in float32 NumPy: k as the host forms it; the weight's argument one float32 subtraction and
    one float32 product; exp2 evaluated in float64 and rounded once; den = den + w and sq = fma(w, w, sq) over b
    ascending (the fma: an exact float64 product, one float64 sum, rounded to float32); ess = (den * den) / sq."""
    f = np.float32
    k = f(1.4426950408889634 / float(f(lam)))
    out = np.zeros(G.shape[0], dtype=np.float32)
    for e, row in enumerate(G):
        fin = np.isfinite(row)
        if not fin.any():
            continue
        gmax = row[fin].max()
        den, sq = f(0), f(0)
        for g, ok in zip(row, fin):
            w = f(np.exp2(np.float64(f(f(g - gmax) * k)))) if ok else f(0)
            den = f(den + w)
            sq = f(np.float64(w) * np.float64(w) + np.float64(sq))
        out[e] = f(f(den * den) / sq)
    return out


@pytest.mark.parametrize("branches", BRANCHES)
def test_value_best_and_ess(torch, env, branches):
    G = returns_of(branches)
    ret = torch.as_tensor(G, device=DEV)
    out = env.mppi_value(ret, branches, LAM)
    # 1. the existing kernel on an action column that holds the returns.  A non-finite return has weight 0, and
    # 0 * inf is NaN in that kernel's fma, so its rows of the column hold 0: fma(0, 0, num) = num, the term the
    # value kernel adds for such a branch.
    col = torch.where(torch.isfinite(ret), ret, torch.zeros_like(ret)).reshape(1, N * branches, 1)
    actions = col.expand(1, N * branches, 4).contiguous()
    nominal = env.mppi_update(actions, ret, LAM)
    torch.cuda.synchronize()
    finite = np.isfinite(G).any(1)
    assert finite.tolist() == [True, True, False]
    for c in range(4):
        _assert_same(torch, out["value"][:2], nominal[0, :2, c].contiguous(), f"value against mppi_update's column {c}")
    value, best, ess = (out[k].cpu().numpy() for k in ("value", "best", "ess"))
    # 2. best: the largest finite return
    for e in (0, 1):
        assert best[e] == G[e][np.isfinite(G[e])].max()
        assert G[e][np.isfinite(G[e])].min() <= value[e] <= best[e]
    # 3. ess.  The bound: the reference runs the kernel's operations in the kernel's order, so the two differ only
    # where an operation is not the same function: the device's exp2 and division are not correctly rounded.  A
    # weight one ulp off shifts its term of den and of sq by at most one ulp of that term, which is at most one
    # ulp of the running sum it enters: `branches` terms, at most `branches` ulp of den^2 / sq in all (den's
    # shifts count twice and sq's once, but a term's share of den and of sq cannot both be the whole sum unless
    # it is the only term); then den * den, the division (2.5 ulp on the device) and the reference's own rounding
    # of the quotient: 3 more.
    ref = ess_ref(G, LAM)
    for e in (0, 1):
        ulp = float(np.spacing(np.float32(ref[e])))
        err = abs(float(ess[e]) - float(ref[e]))
        print(f"\n[branches {branches}, env {e}] value {value[e]:.6f} best {best[e]:.6f} ess {ess[e]:.6f} "
              f"(reference {ref[e]:.6f}, {err / ulp:.1f} ulp; bound {branches + 3})")
        assert err <= (branches + 3) * ulp, (e, ess[e], ref[e])
        assert 1.0 - 1e-6 <= ess[e] <= np.isfinite(G[e]).sum() + 1e-3
    if branches == 1:
        assert value[0] == G[0, 0] and ess[0] == 1.0
    # 4. no finite return
    assert value[2] == 0.0 and best[2] == -np.inf and ess[2] == 0.0
    # best / ess are optional, and the value does not depend on them; `out` is reused
    lone = torch.full((N,), -7.0, device=DEV)
    assert env.lib.hg_mppi_value(env._h, ctypes.c_void_p(ret.data_ptr()), branches, LAM, ctypes.c_void_p(lone.data_ptr()),
                                 None, None, env._stream()) == 0
    again = env.mppi_value(ret, branches, LAM, out=out)
    torch.cuda.synchronize()
    assert again is out
    _assert_same(torch, lone, out["value"], "value without best / ess")


def test_refusals_leave_the_outputs_untouched(torch, env):
    lib = env.lib
    branches = 5
    ret = torch.as_tensor(returns_of(branches), device=DEV)
    val, best, ess = (torch.full((N + 1,), -7.0, device=DEV) for _ in range(3))
    env.reset()
    s0, c0 = env.get_state()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)   # noqa: E731
    good = dict(env=env._h, ret=p(ret), branches=branches, lam=LAM, value=p(val), best=p(best), ess=p(ess),
                stream=env._stream())
    cases = {"NULL env": (dict(env=None), b"env"), "NULL return": (dict(ret=None), b"return"),
             "NULL value": (dict(value=None), b"value"), "branches 0": (dict(branches=0), b"branches"),
             "branches < 0": (dict(branches=-3), b"branches"), "lambda 0": (dict(lam=0.0), b"lambda"),
             "lambda < 0": (dict(lam=-1.0), b"lambda"), "lambda nan": (dict(lam=float("nan")), b"lambda"),
             "lambda inf": (dict(lam=float("inf")), b"lambda"), "lambda tiny": (dict(lam=1e-45), b"lambda"),
             "return 2 bytes off": (dict(ret=off(ret, 2)), b"aligned"), "value 1 byte off": (dict(value=off(val, 1)), b"aligned"),
             "best 2 bytes off": (dict(best=off(best, 2)), b"aligned"), "ess 3 bytes off": (dict(ess=off(ess, 3)), b"aligned")}
    for name, (change, word) in cases.items():
        assert lib.hg_set_max_time(None, 1.0) == -1   # (leaves its own message behind)
        before = lib.hg_last_error()
        assert lib.hg_mppi_value(*dict(good, **change).values()) == -1, name
        msg = lib.hg_last_error()
        assert msg and msg != before and word in msg, (name, msg)
    torch.cuda.synchronize()
    for t in (val, best, ess):
        assert bool((t == -7.0).all())
    assert lib.hg_mppi_value(*good.values()) == 0
    torch.cuda.synchronize()
    for t in (val, best, ess):
        assert bool((t[:N] != -7.0).all()) and float(t[N]) == -7.0
    s1, c1 = env.get_state()
    _assert_same(torch, s0, s1, "env state")
    _assert_same(torch, c0, c1, "env counters")


def test_planner_value_is_mppi_value_of_its_scores(torch):
    from heligym_amd import PolicyMPPI
    n, branches, h = 6, 6, 4
    A, B, _ = _pair(torch, n)
    B.close()
    try:
        _, obs0 = _age(torch, A)
        lo, hi = _bounds(torch, A)
        planner = PolicyMPPI(A, h, branches, sigma=0.1, lam=0.05, res_lo=-0.3, res_hi=0.3, lo=lo, hi=hi, gamma=0.5, seed=77,
                             bootstrap=True, value_scale=0.5)
        with pytest.raises(ValueError, match="plan"):
            planner.value()
        planner.plan(obs0)
        got = planner.value()
        want = A.mppi_value(planner.scores["returns"], branches, 0.05)
        torch.cuda.synchronize()
        for k in ("value", "best", "ess"):
            _assert_same(torch, got[k], want[k], k)
        G = planner.scores["returns"]
        assert bool(torch.isfinite(got["value"]).all())
        _assert_same(torch, got["best"], G.max(1).values, "best against the returns' maximum")
        assert bool((got["value"] <= got["best"]).all()) and bool((got["ess"] >= 1.0 - 1e-6).all())
    finally:
        A.close()
