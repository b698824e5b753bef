"""The task layer on the device away from the default targets: hg_debug_task (the reward functions the step kernels
call, with the handle's device constants or the per-env goal records) on every row of tests/golden/task_kats.npz,
and the short reference episodes of task_traj.npz replayed on one goal handle whose neighbouring lanes hold
different targets, stepped and through hg_rollout.  The assertions and tolerances are those of
tests/test_task_host.py (golden_cases.check_task_kats); the trajectories use contract (ii).  Run with -m gpu."""
import numpy as np
import pytest

import golden_cases as gc

pytestmark = pytest.mark.gpu

TASKS = ("hover", "forward_flight")
N_TRAJ = 130   # three tiles, the last one ragged


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def _env(n, task, **kw):
    from heligym_amd import HeliVecEnv
    return HeliVecEnv(n, task=task, autoreset=False, device="cuda:0", **kw)


@pytest.fixture(scope="module", params=TASKS)
def kats(request):
    return request.param, gc.load_task_kats(request.param)


def _distinct(k):
    keys = np.stack([k["target"][f] for f in k["target"]], axis=1)
    _, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    return order, np.split(order, np.nonzero(np.diff(inv[order]))[0] + 1)


def test_debug_task_on_reference_rows(torch, kats):
    """Every row three ways: through a set_target handle per distinct target (the rows sorted by target, each
    group one launch on its slice), through one goal handle whose env i holds row i's target, and the two
    bitwise equal on the clear rows."""
    task, k = kats
    n = len(k["reward"])
    order, groups = _distinct(k)
    heli = torch.as_tensor(k["heli"][order].astype(np.float32), device="cuda:0").contiguous()
    dots = torch.as_tensor(k["dots"][order].astype(np.float32), device="cuda:0").contiguous()
    rew = torch.full((n,), 7.0, dtype=torch.float32, device="cuda:0")
    succ = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    env = _env(64, task)
    at = 0
    for rows in groups:
        env.set_target({f: float(v[rows[0]]) for f, v in k["target"].items()})
        m = len(rows)
        env.debug_task(heli[at:at + m], dots[at:at + m], out=(rew[at:at + m], succ[at:at + m]))
        at += m
    torch.cuda.synchronize()
    env.close()
    r_set, s_set = np.empty(n, np.float32), np.empty(n, np.uint8)
    r_set[order], s_set[order] = rew.cpu().numpy(), succ.cpu().numpy()
    assert set(np.unique(s_set)) <= {0, 1}
    worst = gc.check_task_kats(k, task, r_set, s_set, "set_target handle")
    print(f"\n[task kats {task}] device, set_target handle ({len(groups)} targets): worst err/tol {worst:.3g}")

    # one goal handle, env i <- row i's target; the row count is no multiple of the 64-env tile
    N = n if n % 64 else n + 1
    assert N >= 130 and N % 64 != 0
    other = {"north_loc": 11.0, "east_loc": -7.0, "sea_alt": 1234.5} if task == "hover" else {"vel": 61.0, "sea_alt": 1234.5}
    genv = _env(N, task, target=other)
    genv.set_goals(goals={f: np.r_[v, np.full(N - n, v[0])] for f, v in k["target"].items()})
    heli = torch.as_tensor(k["heli"].astype(np.float32), device="cuda:0").contiguous()
    dots = torch.as_tensor(k["dots"].astype(np.float32), device="cuda:0").contiguous()
    rg, sg = genv.debug_task(heli, dots)
    # rows past the handle's envs wrap around: 2 N + 3 rows see env i % N
    idx = torch.arange(2 * N + 3, device="cuda:0") % n
    wrap = (idx % N) == (torch.arange(2 * N + 3, device="cuda:0") % N)   # rows whose env is their own row's
    rw, sw = genv.debug_task(heli[idx].contiguous(), dots[idx].contiguous())
    torch.cuda.synchronize()
    genv.close()
    r_goal, s_goal = rg.cpu().numpy(), sg.cpu().numpy()
    worst = gc.check_task_kats(k, task, r_goal, s_goal, "goal handle")
    print(f"[task kats {task}] device, one goal handle of {N} envs: worst err/tol {worst:.3g}")
    c = k["clear"]
    assert np.array_equal(r_goal[c].view(np.uint32), r_set[c].view(np.uint32)) and np.array_equal(s_goal[c], s_set[c])
    w, ii = wrap.cpu().numpy(), idx.cpu().numpy()
    assert w.sum() >= n
    assert np.array_equal(rw.cpu().numpy()[w].view(np.uint32), r_goal[ii[w]].view(np.uint32))
    assert np.array_equal(sw.cpu().numpy()[w], s_goal[ii[w]])


def _replay(torch, e, scen):
    """The scenario's episode on one goal handle of N_TRAJ envs, env i under target i % G: stepped with the
    recorded actions and noise, then again from the same state through one hg_rollout."""
    names = list(e["targets"])
    G, N, T = len(names), N_TRAJ, len(e["action"])
    of_env = [names[i % G] for i in range(N)]
    first = e["targets"][names[0]]["target"]
    env = _env(N, e["task"], dt=e["dt"], max_time=e["max_time"], target=dict(first, heading=0.0))
    env.set_goals(goals={f: np.array([e["targets"][n]["target"][f] for n in of_env]) for f in first})
    st = np.concatenate([e["init_state"], e["init_wind_state"], e["init_obs"][[4, 5, 6, 16]]]).astype(np.float32)
    st = np.tile(st, (N, 1))
    act = torch.as_tensor(np.tile(e["action"][:, None, :], (1, N, 1)).astype(np.float32), device="cuda:0").contiguous()
    eta = torch.as_tensor(np.tile(e["eta"][:, None, :], (1, N, 1)).astype(np.float32), device="cuda:0").contiguous()
    env.set_state(st, np.zeros((N, 3), np.int32))
    out = {key: [] for key in ("obs", "reward", "terminated", "truncated", "failed", "successed", "time_up", "success_step")}
    for t in range(T):
        obs, rew, term, trunc, info = env.step(act[t], eta=eta[t])
        for key, v in (("obs", obs), ("reward", rew), ("terminated", term), ("truncated", trunc)):
            out[key].append(v.clone())
        for key in ("failed", "successed", "time_up", "success_step"):
            out[key].append(info[key].clone())
    stepped = {key: torch.stack(v).cpu().numpy() for key, v in out.items()}
    env.set_state(st, np.zeros((N, 3), np.int32))
    ro = [x.cpu().numpy() for x in env.rollout(act, eta=eta)]
    env.close()
    return names, of_env, stepped, ro


@pytest.mark.parametrize("scen", ["hover", "forward80"])
def test_task_trajectories_on_one_goal_handle(torch, scen):
    e = gc.load_task_traj()[scen]
    names, of_env, got, ro = _replay(torch, e, scen)
    G = len(names)
    for j, name in enumerate(names):
        g = e["targets"][name]
        T = len(g["reward"])
        envs = np.arange(j, N_TRAJ, G)
        for key, v in got.items():   # the envs of one target are one computation
            assert np.array_equal(v[:, envs], np.repeat(v[:, envs[:1]], len(envs), axis=1), equal_nan=True), (name, key)
        i = envs[-1]   # (the last one: the ragged tile for some target)
        lo, hi, scale = gc.reward_bounds(e["heli"][:T], e["dots"][:T], e["task"], tol=gc._traj_tol, **g["target"])
        rt = gc.TRAJ_ABS + gc.TRAJ_REL * scale
        r = got["reward"][:T, i].astype(np.float64)
        excess = np.maximum(np.maximum(lo - r, r - hi), 0.0) / rt
        print(f"\n[task traj {scen}/{name}] env {i}: ends at step {T - 1}; reward worst excess/tol {excess.max():.3g}")
        assert np.all(excess <= 1.0), (name, np.argmax(excess), excess.max())
        for key in ("success_step", "successed", "time_up", "terminated", "truncated", "failed"):
            assert np.array_equal(got[key][:T, i].astype(bool), g[key].astype(bool)), (name, key)
        ended = got["terminated"][:, i].astype(bool) | got["truncated"][:, i].astype(bool)
        assert int(np.argmax(ended)) == T - 1 and ended[T - 1]
    # neighbouring lanes end at different steps
    ends = [len(e["targets"][n]["reward"]) for n in of_env[:G]]
    assert len(set(ends)) >= 2
    # the same episodes through one rollout launch (per-env goals held across the steps, injected noise)
    obs, rew, term, trunc, info = ro
    assert np.array_equal(obs.view(np.uint32), got["obs"].view(np.uint32))
    assert np.array_equal(rew.view(np.uint32), got["reward"].view(np.uint32))
    assert np.array_equal(term.astype(bool), got["terminated"].astype(bool))
    assert np.array_equal(trunc.astype(bool), got["truncated"].astype(bool))
    bits = (got["failed"].astype(np.uint8) | got["successed"].astype(np.uint8) << 1 | got["time_up"].astype(np.uint8) << 2
            | got["success_step"].astype(np.uint8) << 3)
    assert np.array_equal(info & 15, bits)
