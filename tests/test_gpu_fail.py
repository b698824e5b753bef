"""Heli._is_failed on the device: hg_debug_failed (the function the step kernels call, with the handle's device
constants and terrain texels) on every row of tests/golden/fail_kats.npz for both airframes and on a mixed fleet; full
steps from one step short of each boundary through every kernel family against or_step; the short reference episodes
of fail_traj.npz stepped and through hg_rollout; and lanes that fail by different clauses beside lanes that hold a
clause and must not fail, in one wave.  The contract is tests/test_fail_host.py's (golden_cases.check_fail_kats).
Run with -m gpu."""
import numpy as np
import pytest

import golden_cases as gc

pytestmark = pytest.mark.gpu

AIRFRAMES = ("aw109", "heavy", "aw109_narrow")   # (the last: the bundled airframe over heavy's narrower map)
BIT = gc.FAIL_BIT
DEG = np.pi / 180


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def _env(n, doc="aw109", **kw):
    from heligym_amd import HeliVecEnv
    kw.setdefault("autoreset", False)
    return HeliVecEnv(n, task="hover", dt=0.01, heli_name=doc, device="cuda:0", **kw)


def _dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda:0").contiguous()


def _report(who, name, k, failed, clauses):
    from heligym_amd import _abi
    failed, clauses = failed.cpu().numpy(), clauses.cpu().numpy()
    assert set(np.unique(failed)) <= {0, 1}
    # the copy that reports the clauses combines them as the step kernels' is_failed does, on every row
    assert np.array_equal((clauses & _abi.HG_FAIL_FAILED) != 0, failed == 1)
    nc, nt = gc.check_fail_kats(k, failed, clauses & 127, who)
    ins = k["inside"] & ~k["raises"][:, None]
    print(f"\n[fail kats {name}] {who}: every row outside the margin agrees; inside it {nc} of {int(ins[:, 0].sum())} contact "
          f"and {nt} of {int(ins[:, 1].sum())} ceiling rows differ in that bit")
    return failed, clauses


@pytest.mark.parametrize("name", AIRFRAMES)
def test_debug_failed_on_reference_rows(torch, name):
    k = gc.load_fail_kats(name)
    n = len(k["failed"])
    env = _env(130, k["doc"])
    f, c = env.debug_failed(_dev(torch, k["heli"]), _dev(torch, k["dots"]))
    torch.cuda.synchronize()
    env.close()
    assert n > 2000 and n % 64
    _report("device", name, k, f, c)


def test_debug_failed_on_a_fleet_whose_tiles_alternate(torch):
    """One handle of four tiles, the aw109 and the heavy airframe alternating (a fleet's classes share the handle's
    map: both over the narrower one): row i of the fixture of class (i // 64) % 2 sits at env i, so each row is checked
    under its own class; the rows past the handle's envs wrap around to env i % N."""
    fleet = ("aw109_narrow", "heavy")
    ks = [gc.load_fail_kats(a) for a in fleet]
    S = min(len(k["failed"]) for k in ks)
    ks = [{key: (v[:S] if isinstance(v, np.ndarray) and len(v) == len(k["failed"]) else v) for key, v in k.items()} for k in ks]
    N = 256
    env = _env(N, ks[0]["doc"])
    env.set_fleet([k["doc"] for k in ks], tile_class=[0, 1, 0, 1])
    cls = (np.arange(S) % N) // 64 % 2
    heli = np.where(cls[:, None] == 0, ks[0]["heli"], ks[1]["heli"])
    dots = np.where(cls[:, None] == 0, ks[0]["dots"], ks[1]["dots"])
    f, c = env.debug_failed(_dev(torch, heli), _dev(torch, dots))
    torch.cuda.synchronize()
    env.close()
    f, c = f.cpu().numpy(), c.cpu().numpy()
    for a, k in enumerate(ks):
        rows = cls == a
        sub = {key: (v[rows] if isinstance(v, np.ndarray) and len(v) == S else v) for key, v in k.items()}
        nc, nt = gc.check_fail_kats(sub, f[rows], c[rows] & 127, f"fleet class {fleet[a]}")
        assert rows.sum() > 900
        print(f"\n[fail kats fleet] class {fleet[a]}: {int(rows.sum())} rows agree outside the margin ({nc} contact, {nt} "
              f"ceiling bits differ inside it)")
    # the classes do differ on these rows: the heavy airframe's sink-rate threshold and WL_CG are others
    assert np.all(ks[0]["thresholds"][[0, 4]] != ks[1]["thresholds"][[0, 4]])


# ------------------------------------------------------------------------------------------------
# full steps from one step short of each boundary

def _body(roll, pitch, yaw, v_ned):
    """Body-axis velocity of a NED velocity at the attitude (the transpose of the body-to-NED rotation)."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    b2n = np.array([[cp * cy, sr * sp * cy - cr * sy, cr * sp * cy + sr * sy],
                    [cp * sy, sr * sp * sy + cr * cy, cr * sp * sy - sr * cy],
                    [-sp, sr * cp, cr * cp]])
    return b2n.T @ np.asarray(v_ned, dtype=np.float64)


# name -> (x, y, agl or None, alt offset from gta + 10000 or None, roll, pitch (None: the trim's), NED velocity, fails)
CASES = [
    ("hover", 0.0, 0.0, 100.0, None, None, None, (0.0, 0.0, 0.0), False),
    ("north", gc.half_extent()[0] - 0.3, 0.0, 100.0, None, None, None, (60.0, 0.0, 0.0), True),
    ("north_leaving", gc.half_extent()[0] - 0.3, 0.0, 100.0, None, None, None, (-60.0, 0.0, 0.0), False),
    ("south", -gc.half_extent()[0] + 0.3, 0.0, 100.0, None, None, None, (-60.0, 0.0, 0.0), True),
    ("east", 0.0, gc.half_extent()[1] - 0.3, 100.0, None, None, None, (0.0, 60.0, 0.0), True),
    ("west", 0.0, -gc.half_extent()[1] + 0.3, 100.0, None, None, None, (0.0, -60.0, 0.0), True),
    ("west_leaving", 0.0, -gc.half_extent()[1] + 0.3, 100.0, None, None, None, (0.0, 60.0, 0.0), False),
    ("ceiling", 0.0, 0.0, None, -0.3, None, None, (0.0, 0.0, -60.0), True),
    ("ceiling_descending", 0.0, 0.0, None, -0.3, None, None, (0.0, 0.0, 60.0), False),
    ("hard_landing", 10.0, -20.0, 0.3, None, None, None, (0.0, 0.0, 80.0), True),
    ("fast_sink_in_the_air", 10.0, -20.0, 100.0, None, None, None, (0.0, 0.0, 80.0), False),
    ("roll_over", 10.0, -20.0, 0.08, None, 75 * DEG, None, (0.0, 0.0, 20.0), True),
    ("rolled_in_the_air", 10.0, -20.0, 100.0, None, 75 * DEG, None, (0.0, 0.0, 20.0), False),
    ("landing_rolled_negative", 10.0, -20.0, 0.08, None, -75 * DEG, None, (0.0, 0.0, 20.0), False),
    ("pitch_over", 10.0, -20.0, 0.08, None, -170 * DEG, 70 * DEG, (0.0, 0.0, 20.0), True),
    ("landing_pitched_negative", 10.0, -20.0, 0.08, None, -170 * DEG, -70 * DEG, (0.0, 0.0, 20.0), False),
]


@pytest.fixture(scope="module")
def boundary(terrain_u16):
    """The CASES as set_state rows [K, 27] built from the reset template, and what or_step(state_f32=True) says of
    one step with the trim action and no turbulence: failed [K], the post-step clause bits."""
    from heligym_amd import config
    from oracle.oracle import Oracle
    cfg, doc = config.make_config(task="hover", dt=0.01)
    orc = Oracle(cfg, terrain_u16)
    tr = orc.trim({})
    st0, obs0, act = np.array(tr.state), np.array(tr.obs), np.array(tr.action, dtype=np.float32)
    wl_cg = doc["airframe"]["WL_CG"] / 12
    thr = gc.load_fail_kats("aw109")["thresholds"]
    rows, failed, bits = [], [], []
    for name, x, y, agl, top, roll, pitch, v_ned, fails in CASES:
        s = st0.copy()
        s[15], s[16] = np.float32(x), np.float32(y)
        gta = orc.ground_height(s[15], s[16], state_f32=True) + wl_cg
        s[17] = np.float32(-(gta + agl)) if top is None else np.float32(-(gta + 10000.0 + top))
        s[12] = np.float32(s[12] if roll is None else roll)
        s[13] = np.float32(s[13] if pitch is None else pitch)
        s[6:9] = _body(s[12], s[13], s[14], v_ned).astype(np.float32)
        prev = obs0.copy()
        e = orc.env_from(s, np.zeros(5), prev, np.zeros(18), state_f32=True)
        o = orc.step(e, act, np.zeros(3))
        heli, dots = np.array(e.heli), np.array(e.dots)
        f, c = orc.is_failed(heli, dots, state_f32=False)
        assert bool(o.failed) == bool(f[0]) == fails == bool(o.terminated), (name, o.failed, int(c[0]))
        # the outcome holds within the single-step tolerance: no clause that decides it sits next to its threshold
        g1 = orc.ground_height(heli[15], heli[16]) + wl_cg
        assert gc.fail_traj_determinate(heli[None], dots[None], np.array([g1]), thr, scale=4.0), name
        rows.append(np.concatenate([s, np.zeros(5), prev[[4, 5, 6, 16]]]).astype(np.float32))
        failed.append(fails)
        bits.append(int(c[0]))
    by = dict(zip((c[0] for c in CASES), bits))
    # each boundary is crossed by its own clause alone, and the controls hold a clause without failing
    assert [by[n] for n in ("north", "south", "east", "west", "ceiling")] == [BIT["ns"]] * 2 + [BIT["ew"]] * 2 + [BIT["ceiling"]]
    assert by["hard_landing"] == BIT["contact"] | BIT["sink"] and by["roll_over"] == BIT["contact"] | BIT["roll"]
    assert by["pitch_over"] == BIT["contact"] | BIT["pitch"] and by["fast_sink_in_the_air"] == BIT["sink"]
    assert by["rolled_in_the_air"] == BIT["roll"] and by["landing_rolled_negative"] == BIT["contact"]
    assert by["landing_pitched_negative"] == BIT["contact"] and by["hover"] == by["north_leaving"] == 0
    return {"rows": np.array(rows), "failed": np.array(failed), "action": act}


def _lanes(b, n, shift=0):
    """Env i holds case (i + shift + i // 64) % K: every wave holds every case, at other lanes in each tile."""
    i = np.arange(n)
    case = (i + shift + i // 64) % len(CASES)
    return case, b["rows"][case].copy(), b["failed"][case]


def _check_step(torch, env, b, n, who, autoreset=False):
    from heligym_amd import _abi
    case, st, want = _lanes(b, n)
    env.set_state(st, np.zeros((n, 3), np.int32))
    act = _dev(torch, np.tile(b["action"], (n, 1)))
    eta = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
    obs, rew, term, trunc, info = env.step(act, eta=eta)
    torch.cuda.synchronize()
    bits = env.info_u8.cpu().numpy()
    bad = np.nonzero(term.cpu().numpy().astype(bool) != want)[0]
    assert len(bad) == 0, (who, [(int(i), CASES[case[i]][0]) for i in bad[:8]])
    assert np.array_equal((bits & _abi.HG_INFO_FAILED) != 0, want), who
    assert np.array_equal((bits & _abi.HG_INFO_RESET) != 0, want if autoreset else np.zeros(n, bool)), who
    assert not trunc.cpu().numpy().any() and not (bits & (_abi.HG_INFO_SUCCESSED | _abi.HG_INFO_TIME_UP)).any()
    assert np.array_equal(info["failed"].cpu().numpy().astype(bool), want)
    return term.cpu().numpy().astype(bool)


@pytest.mark.parametrize("autoreset", [False, True], ids=["no_autoreset", "autoreset"])
def test_full_steps_helper_kernel(torch, boundary, autoreset):
    """130 envs (three tiles, the last ragged): the helper kernel.  With auto-reset on, the reset bit is `failed`."""
    env = _env(130, autoreset=autoreset)
    env.reset()
    _check_step(torch, env, boundary, 130, "helper kernel", autoreset)
    env.close()


@pytest.mark.parametrize("kind", ["weather", "goals", "fleet"])
def test_full_steps_lone_wave_kernel_at_small_n(torch, boundary, kind):
    """A weather, goal or fleet handle runs the one-wave lone kernel family at any N: 130 envs."""
    env = _env(130)
    if kind == "weather":
        env.set_weather(turb_level=float(env.cfg.af.env_TURB_LVL))   # every env the document's own weather
    elif kind == "goals":
        env.set_goals(goals={"north_loc": np.linspace(-50.0, 50.0, 130)})
    else:
        env.set_fleet(["aw109", "aw109"], tile_class=[0, 1, 0])
    env.reset()
    _check_step(torch, env, boundary, 130, f"lone-wave kernel ({kind} handle)")
    env.close()


def test_full_steps_rollout_and_branch_end_info(torch, boundary):
    """hg_rollout (one launch, two steps: the second from the state the first left, auto-reset off) and
    rollout_branch's end_info and alive_steps, two branches per env, no turbulence."""
    from heligym_amd import _abi
    n = 130
    case, st, want = _lanes(boundary, n, shift=5)
    env = _env(n)
    env.reset()
    env.set_state(st, np.zeros((n, 3), np.int32))
    act1 = _dev(torch, np.tile(boundary["action"], (n, 1)))
    eta1 = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
    o1, r1, t1, _, _ = env.step(act1, eta=eta1)
    o1, r1, t1, i1 = o1.clone(), r1.clone(), t1.clone(), env.info_u8.clone()
    env.set_state(st, np.zeros((n, 3), np.int32))
    obs, rew, term, trunc, info = env.rollout(act1[None].contiguous(), eta=eta1[None].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(term[0].cpu().numpy().astype(bool), want)
    assert np.array_equal((info[0].cpu().numpy() & _abi.HG_INFO_FAILED) != 0, want)
    assert torch.equal(obs[0].view(torch.int32), o1.view(torch.int32)) and torch.equal(rew[0].view(torch.int32), r1.view(torch.int32))
    assert torch.equal(info[0], i1) and torch.equal(term[0].to(torch.bool), t1.to(torch.bool))
    # branches: both branches of an env start from its state
    env.set_state(st, np.zeros((n, 3), np.int32))
    B = 2
    out = env.rollout_branch(act1.repeat_interleave(B, dim=0)[None].contiguous(), B, noise="off")
    torch.cuda.synchronize()
    end, alive = out["end_info"].cpu().numpy(), out["alive_steps"].cpu().numpy()
    env.close()
    assert np.array_equal(end, np.where(want, _abi.HG_INFO_FAILED, 0).astype(np.uint8)[:, None].repeat(B, 1))
    assert np.all(alive == 1)


def test_full_step_bulk_kernel_at_its_smallest_size(torch, boundary):
    """One step of 2 * 64 * 4 * CUs + 1 envs: the first env count past the lone-wave range."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 64 * 4 * cus + 1
    env = _env(n)
    env.reset()
    got = _check_step(torch, env, boundary, n, "bulk kernel")
    env.close()
    assert got.sum() > n // 3 and got[n - 1] == boundary["failed"][_lanes(boundary, n)[0][n - 1]]


def test_clauses_mixed_in_one_wave_equal_one_clause_per_wave(torch, boundary):
    """Lanes that fail by different clauses beside lanes that hold a clause and must not fail (every wave holds all
    16 cases): each lane bitwise the same lane of a handle whose lanes all hold that lane's case."""
    n = 130
    case, st, want = _lanes(boundary, n)
    act = _dev(torch, np.tile(boundary["action"], (n, 1)))
    eta = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")

    def run(state):
        env = _env(n, seed=3)
        env.reset()
        env.set_state(state, np.zeros((n, 3), np.int32))
        obs, rew, term, _, _ = env.step(act, eta=eta)
        s, _ = env.get_state()
        out = [x.cpu().numpy().copy() for x in (obs, rew, term, env.info_u8, s)]
        env.close()
        return out

    mixed = run(st)
    assert np.array_equal(mixed[2].astype(bool), want)
    for c in range(len(CASES)):
        pure = run(np.tile(boundary["rows"][c], (n, 1)))
        rows = case == c
        assert rows.sum() >= 8
        for got, ref, what in zip(mixed, pure, ("obs", "reward", "terminated", "info", "state")):
            assert np.array_equal(got[rows].view(np.uint8), ref[rows].view(np.uint8)), (CASES[c][0], what)
        assert np.all(pure[2].astype(bool) == boundary["failed"][c])


# ------------------------------------------------------------------------------------------------
# fail_traj.npz on the device

def test_fail_trajectories(torch):
    """Every episode of fail_traj.npz in one handle, episode j at envs j, j + E, ... (lanes of one wave end at
    different steps by different clauses), stepped with the recorded actions and noise: each ends at the reference's
    step by the reference's flag, the controls do not fail; then the same through one hg_rollout, bitwise."""
    traj = gc.load_fail_traj()
    names = list(traj)
    E, N = len(names), 130
    T = max(len(e["failed"]) for e in traj.values())
    of_env = [names[i % E] for i in range(N)]
    st = np.stack([np.concatenate([traj[s]["init_state"], traj[s]["init_wind_state"], traj[s]["init_obs"][[4, 5, 6, 16]]])
                   for s in of_env]).astype(np.float32)
    act = np.zeros((T, N, 4), np.float32)
    eta = np.zeros((T, N, 3), np.float32)
    for i, s in enumerate(of_env):   # past its end an episode repeats its last action with no noise (not compared)
        k = len(traj[s]["failed"])
        act[:k, i], eta[:k, i] = traj[s]["action"], traj[s]["eta"]
        act[k:, i] = traj[s]["action"][-1]
    act, eta = _dev(torch, act), _dev(torch, eta)
    env = _env(N)
    env.reset()
    env.set_state(st, np.zeros((N, 3), np.int32))
    got = {key: [] for key in ("obs", "reward", "terminated", "truncated", "info")}
    for t in range(T):
        obs, rew, term, trunc, _ = env.step(act[t], eta=eta[t])
        for key, v in zip(got, (obs, rew, term, trunc, env.info_u8)):
            got[key].append(v.clone())
    got = {key: torch.stack(v).cpu().numpy() for key, v in got.items()}
    env.set_state(st, np.zeros((N, 3), np.int32))
    ro = [x.cpu().numpy() for x in env.rollout(act, eta=eta)]
    env.close()
    from heligym_amd import _abi
    for j, s in enumerate(names):
        e = traj[s]
        k = len(e["failed"])
        envs = np.arange(j, N, E)
        for key, v in got.items():   # the envs of one episode are one computation
            assert np.array_equal(v[:, envs], np.repeat(v[:, envs[:1]], len(envs), axis=1), equal_nan=True), (s, key)
        i = envs[-1]
        failed = (got["info"][:k, i] & _abi.HG_INFO_FAILED) != 0
        assert np.array_equal(failed, e["failed"].astype(bool)), (s, np.nonzero(failed)[0][:3], k)
        assert np.array_equal(got["terminated"][:k, i].astype(bool), e["terminated"].astype(bool)), s
        assert not got["truncated"][:k, i].any()
        if e["fails"]:
            assert int(np.argmax(got["terminated"][:, i])) == k - 1
        print(f"\n[fail traj {s}] env {i}: " + (f"ends at the reference's step {k - 1}" if e["fails"] else f"{k} steps, does not fail"))
    obs, rew, term, trunc, info = ro
    # (no auto-reset: past its ending step an env goes on alike in both)
    assert np.array_equal(obs.view(np.uint32), got["obs"].view(np.uint32))
    assert np.array_equal(rew.view(np.uint32), got["reward"].view(np.uint32))
    assert np.array_equal(term.astype(bool), got["terminated"].astype(bool)) and np.array_equal(info, got["info"])
