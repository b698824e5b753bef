"""Turn the golden trajectories (tests/golden/traj_dt*.npz, recorded from the reference by
tools/gen_goldens.py) into batched single-step cases: one env per recorded step, its pre-step
state taken from the reference itself.  Data only — no oracle, no reference code."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TASK_KEY = {"hover": "success_hover", "forward_flight": "success_ff"}
REWARD_KEY = {"hover": "reward_hover", "forward_flight": "reward_ff"}


def success_threshold(dt, max_time=40.0):
    """Steps of success needed for `successed` (helicopter.py:205,236-237 float accumulation)."""
    s, k = 0.0, 0
    while not s >= max_time / 4:
        s += dt
        k += 1
    return k


def time_up_threshold(dt, max_time=40.0):
    t, k = 0.0, 0
    while not t > max_time:
        t += dt
        k += 1
    return k


def _npz(path):
    """An npz read whole into a dict (NpzFile decompresses a member again on every access)."""
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def load(tag):
    return _npz(os.path.join(GOLDEN, f"traj_dt{tag}.npz"))


def single_step_batch(d, task="hover"):
    dt = float(d["dt"])
    n_succ = success_threshold(dt)
    n_up = time_up_threshold(dt)
    rows = {k: [] for k in ("state", "counters", "actions", "eta", "obs", "heli", "wind", "reward",
                            "failed", "successed", "time_up", "terminated", "truncated", "success_step",
                            "dots", "scenario", "t")}
    for n in d["scenarios"]:
        g = lambda k: d[f"{n}/{k}"]  # noqa: E731
        T = len(g("reward_hover"))
        succ_flags = g(TASK_KEY[task])
        for t in range(T):
            if t == 0:
                heli, wind, prev_obs = g("init_state"), g("init_wind_state"), g("init_obs")
            else:
                heli, wind, prev_obs = g("state")[t - 1], g("wind_state")[t - 1], g("obs")[t - 1]
            carry = [prev_obs[4], prev_obs[5], prev_obs[6], prev_obs[16]]
            succ_before = int(np.sum(succ_flags[:t]))
            rows["state"].append(np.concatenate([heli, wind, carry]))
            rows["counters"].append([t, succ_before, 0])
            rows["actions"].append(g("action")[t])
            rows["eta"].append(g("eta")[t])
            rows["obs"].append(g("obs")[t])
            rows["heli"].append(g("state")[t])
            rows["wind"].append(g("wind_state")[t])
            rows["dots"].append(g("state_dots")[t])
            rows["reward"].append(g(REWARD_KEY[task])[t])
            failed = bool(g("failed")[t])
            successed = succ_before >= n_succ
            time_up = (t + 1) >= n_up
            rows["failed"].append(failed)
            rows["successed"].append(successed)
            rows["time_up"].append(time_up)
            rows["terminated"].append(failed or successed)
            rows["truncated"].append(time_up)
            rows["success_step"].append(bool(succ_flags[t]))
            rows["scenario"].append(str(n))
            rows["t"].append(t)
    out = {k: np.array(v) for k, v in rows.items()}
    out["dt"] = dt
    return out


def step_errors(got, ref, angle_cols=()):
    """|got - ref| with angle columns compared modulo 2*pi."""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    for c in angle_cols:
        d[..., c] = np.minimum(d[..., c], np.abs(d[..., c] - 2 * np.pi))
    return d


HELI_ANGLE_COLS = (2, 3, 4, 5, 12, 13, 14)   # psi_mr psi_tr betas euler (wrapped, utils.py:3-4)
OBS_ANGLE_COLS = (7, 8, 9)


def edge_distance_ft(x, y, rows=1024, span=6561.6798):
    """Distance (ft) of a position from the nearest terrain cell edge of the reference's height
    map (helicopter_dynamics.py:168-186), where its ground height is discontinuous."""
    px = span / rows
    fx = (x / px) % 1.0
    fy = (y / px) % 1.0
    return px * min(fx, 1 - fx, fy, 1 - fy)


def _tol(x):
    return 2e-4 + 2e-5 * np.abs(x)


def _terminal_bounds(arg, arg_tol, d):
    """-sum(sign(arg) * d) where sign(arg) is ambiguous when |arg| <= arg_tol: [lo, hi] bounds."""
    amb = np.abs(arg) <= arg_tol
    fixed = np.where(amb, 0.0, -np.sign(arg) * d)
    span = np.where(amb, np.abs(d), 0.0)
    return fixed.sum(axis=-1) - span.sum(axis=-1), fixed.sum(axis=-1) + span.sum(axis=-1)


REWARD_ABS, REWARD_REL = 2e-4, 2e-5   # the reward contract: |dr| <= REWARD_ABS + REWARD_REL * (sum of |term|)
TRAJ_ABS, TRAJ_REL = 1e-3, 1e-4       # contract (ii), free-running trajectories


def _traj_tol(x):
    return TRAJ_ABS + TRAJ_REL * np.abs(x)


def _pymax(final, terminal):
    """Python's max(final, terminal) (helicopter_with_tasks.py:37,44): the terminal term only where
    `terminal > final` holds, so a NaN terminal term leaves the final one and a NaN final one stays."""
    return np.where(terminal > final, terminal, final)


def _mag(a):
    """|a| where finite, else 0: a term that is inf or NaN drops out of the reward's rounding scale."""
    return np.where(np.isfinite(a), np.abs(a), 0.0)


def task_terms(heli, dots, task, n_t=np.sqrt(2 * 18 / 32.2), n_x=36.0, n_v=np.sqrt(2 * 18 * 32.2), n_a=32.2,
               north_loc=0.0, east_loc=0.0, sea_alt=4000.0, vel=100.0, tol=None):
    """The task layer's terms (helicopter_with_tasks.py:27-52, 78-115) in fp64 for rows of post-step
    state and k4 derivatives; the target fields are scalars or one value per row.  Returns a dict:
    args [n, A] every sign() argument, arg_tol [n, A] its ambiguity tolerance (the state tolerance
    `tol` carried to the argument), terms [n, A] what each sign multiplies, final [n, G] the
    *_final_reward of every group, groups: the columns of args of each group."""
    _tol = tol or globals()["_tol"]
    h = np.asarray(heli, dtype=np.float64)
    d = np.asarray(dots, dtype=np.float64)
    n = len(h)
    bc = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))  # noqa: E731
    with np.errstate(all="ignore"):
        pn, pdn = h[:, 9:12] * n_t, d[:, 9:12] * n_t ** 2
        pf = -(pn ** 2).sum(axis=1)
        ptol = _tol(h[:, 9:12]) * n_t
        if task == "hover":
            # np.array([...], float32) / 36 stays float32 (:33)
            tgt = (np.stack([bc(north_loc), bc(east_loc), -bc(sea_alt)], axis=1).astype(np.float32)
                   / np.float32(n_x)).astype(np.float64)
            e = h[:, 15:18] / n_x - tgt
            return {"args": np.concatenate([pn, e], axis=1),
                    "arg_tol": np.concatenate([ptol, _tol(h[:, 15:18]) / n_x], axis=1),
                    "terms": np.concatenate([pdn, d[:, 15:18] / n_v], axis=1),
                    "final": np.stack([pf, -(e ** 2).sum(axis=1)], axis=1), "groups": ((0, 1, 2), (3, 4, 5))}
        v = np.sqrt((h[:, 6:9] ** 2).sum(axis=1))
        # np.array(vel, float32) / np.float64 is float64; np.array(-alt, float32) / 36 stays float32 (:87-88)
        ev = v / n_v - bc(vel).astype(np.float32).astype(np.float64) / n_v
        vdn = (h[:, 6:9] * d[:, 6:9]).sum(axis=1) / v / n_a
        ed = h[:, 17] / n_x - ((-bc(sea_alt)).astype(np.float32) / np.float32(n_x)).astype(np.float64)
        return {"args": np.concatenate([pn, ev[:, None], ed[:, None]], axis=1),
                "arg_tol": np.concatenate([ptol, (_tol(v) / n_v)[:, None], (_tol(h[:, 17]) / n_x)[:, None]], axis=1),
                "terms": np.concatenate([pdn, vdn[:, None], (d[:, 17] / n_v)[:, None]], axis=1),
                "final": np.stack([pf, -ev ** 2, -ed ** 2], axis=1), "groups": ((0, 1, 2), (3,), (4,))}


def reward_bounds(heli, dots, task, n_t=np.sqrt(2 * 18 / 32.2), n_x=36.0, n_v=np.sqrt(2 * 18 * 32.2),
                  n_a=32.2, sea_alt=4000.0, vel=100.0, tol=None, north_loc=0.0, east_loc=0.0):
    """Interval of task rewards (helicopter_with_tasks.py:27-52, 78-115) consistent with the
    post-step state `heli` and k4 derivatives `dots` once every sign() argument that lies within
    the parity tolerance of zero is treated as ambiguous: the reward jumps there.  Also returns
    the magnitude scale of the reward's terms (sum of |term|), the scale rounding errors follow.
    tol: the state tolerance x -> |dx| deciding the ambiguity (default contract (i)).
    north_loc, east_loc, sea_alt, vel: the target, scalars or one value per row."""
    t = task_terms(heli, dots, task, n_t, n_x, n_v, n_a, north_loc, east_loc, sea_alt, vel, tol)
    lo = hi = scale = 0.0
    with np.errstate(all="ignore"):
        for g, cols in enumerate(t["groups"]):
            c = list(cols)
            t_lo, t_hi = _terminal_bounds(t["args"][:, c], t["arg_tol"][:, c], t["terms"][:, c])
            f = t["final"][:, g]
            lo = lo + _pymax(f, t_lo)
            hi = hi + _pymax(f, t_hi)
            scale = scale + _mag(f) + _mag(t["terms"][:, c]).sum(axis=1)
    k = len(t["groups"])
    return lo / k, hi / k, scale / k


CONTACT_GR_ALT = 10.0   # ft: below this ground altitude the landing gear can be in contact


def f8_resets():
    """Second-episode reset fixtures (tests/golden/reset_f8.npz): (dt, trim cond vector, wind, reset
    state, reset action, reset obs) for the recorded cases and the crash-ended episodes."""
    d = np.load(os.path.join(GOLDEN, "reset_f8.npz"), allow_pickle=False)
    rows = [(float(d["case/dt"][i]), d["case/cond"][i], d["case/wind_ned"][i], d["case/state"][i],
             d["case/action"][i], d["case/obs"][i]) for i in range(len(d["case/dt"]))]
    rows += [(float(d["episode/dt"][i]), None, d["episode/wind_ned"][i], d["episode/reset_state"][i],
              d["episode/reset_action"][i], d["episode/reset_obs"][i]) for i in range(len(d["episode/dt"]))]
    return rows


def f8_episodes():
    d = np.load(os.path.join(GOLDEN, "reset_f8.npz"), allow_pickle=False)
    return {k.split("/", 1)[1]: d[k] for k in d.files if k.startswith("episode/")}


VARIANTS = ("turb5", "turb7_wind", "turb0", "heavy", "wing")

TASK_FIELDS = {"hover": ("north_loc", "east_loc", "sea_alt"), "forward_flight": ("vel", "sea_alt")}


def _edge_tol(x):
    """The ambiguity of a sign() argument on the edge rows of task_kats.npz, whose inputs are exact fp32 values:
    only the arithmetic differs.  An argument is a difference of two operands of the state value's magnitude
    over a normaliser; the fp32 forms round the normaliser's reciprocal, the product and the target quotient
    (half an ulp each), the reference rounds its target and quotient to fp32 too, and sqrt of the speed adds
    two more: under 4 ulp of the operand, which 8 ulp of the state value covers (ulp(x) / n >= ulp(x / n) / 2)."""
    with np.errstate(all="ignore"):
        return 8.0 * np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def load_task_kats(task):
    """task_kats.npz for one task: heli, dots [n,18] float64 (fp32 values), target {field: [n]}, reward,
    success_step, label ("" on clear rows), clear (mask), candidates, dropped."""
    d = _npz(os.path.join(GOLDEN, "task_kats.npz"))
    row = d[f"{task}/row"].astype(np.int64)
    out = {"heli": d["heli"][row].astype(np.float64), "dots": d["dots"][row].astype(np.float64),
           "target": {f: d[f"{task}/target"][:, j].copy() for j, f in enumerate(TASK_FIELDS[task])},
           "reward": d[f"{task}/reward"], "success_step": d[f"{task}/success_step"],
           "label": np.array([str(s) for s in d[f"{task}/label"]]),
           "candidates": int(d[f"{task}/candidates"]), "dropped": int(d[f"{task}/dropped"])}
    out["clear"] = out["label"] == ""
    return out


def task_bounds(k, task, rows=None):
    """reward_bounds of task_kats rows under each row's own target: contract (i) ambiguity on clear rows (none
    is ambiguous there), _edge_tol on edge rows.  (lo, hi, reward tolerance)."""
    rows = np.arange(len(k["reward"])) if rows is None else rows
    lo, hi, rt = np.empty(len(rows)), np.empty(len(rows)), np.empty(len(rows))
    for mask, tol in ((k["clear"][rows], None), (~k["clear"][rows], _edge_tol)):
        if not mask.any():
            continue
        r = rows[mask]
        a, b, s = reward_bounds(k["heli"][r], k["dots"][r], task, tol=tol, **{f: v[r] for f, v in k["target"].items()})
        lo[mask], hi[mask], rt[mask] = a, b, REWARD_ABS + REWARD_REL * s
    return lo, hi, rt


def check_task_kats(k, task, reward, success, who):
    """The assertions every evaluator of the task layer meets on task_kats.npz: clear rows within the reward
    contract of the reference, edge rows inside the sign-ambiguity bounds, NaN where and only where the
    reference's reward is, success_step equal but on the rows built to sit within tolerance of -1.  Returns the
    worst error / tolerance over the finite rows."""
    reward = np.asarray(reward, dtype=np.float64)
    ref = k["reward"]
    bad = np.nonzero(np.isnan(reward) != np.isnan(ref))[0]
    assert len(bad) == 0, (who, task, "isnan", [(k["label"][i], reward[i], ref[i]) for i in bad[:10]])
    lo, hi, rt = task_bounds(k, task)
    fin = ~np.isnan(ref)
    with np.errstate(all="ignore"):
        clear = k["clear"] & fin
        err = np.where(clear, np.abs(reward - ref), np.maximum(np.maximum(lo - reward, reward - hi), 0.0))
        ratio = np.where(fin, err / rt, 0.0)
    bad = np.nonzero(~(ratio <= 1.0))[0]
    assert len(bad) == 0, (who, task, [(i, k["label"][i], reward[i], ref[i], lo[i], hi[i], rt[i]) for i in bad[:10]])
    near = np.array([s.startswith("near_minus_one") for s in k["label"]])
    bad = np.nonzero((np.asarray(success).astype(bool) != k["success_step"]) & ~near)[0]
    assert len(bad) == 0, (who, task, "success_step", [(i, k["label"][i]) for i in bad[:10]])
    return float(ratio.max())


def load_task_traj():
    """task_traj.npz as {scenario: {task, dt, max_time, action, eta, init_*, heli, dots (post-step rows with
    the recorded columns filled in, the rest 0), targets: {name: {target: {field: value}, reward, flags...}}}}."""
    d = _npz(os.path.join(GOLDEN, "task_traj.npz"))
    cols = d["cols"]
    out = {}
    for s in (str(x) for x in d["scenarios"]):
        task = str(d[f"{s}/task"])
        T = len(d[f"{s}/action"])
        e = {"task": task, "dt": float(d["dt"]), "max_time": float(d["max_time"]), "heli": np.zeros((T, 18)),
             "dots": np.zeros((T, 18)), "targets": {}}
        e["heli"][:, cols], e["dots"][:, cols] = d[f"{s}/state_cols"], d[f"{s}/dots_cols"]
        for key in ("action", "eta", "init_state", "init_wind_state", "init_obs", "init_state_dots", "init_trim_cond"):
            e[key] = d[f"{s}/{key}"]
        for t in (str(x) for x in d[f"{s}/targets"]):
            g = {key: d[f"{s}/{t}/{key}"] for key in ("reward", "success_step", "failed", "successed", "time_up",
                                                      "terminated", "truncated")}
            g["target"] = dict(zip(TASK_FIELDS[task], map(float, d[f"{s}/{t}/target"])))
            e["targets"][t] = g
        out[s] = e
    return out


def load_contact(dt):
    """The landings of tests/golden/traj_contact.npz recorded at time step `dt`, shaped like a
    traj_dt*.npz file (scenarios, dt, <name>/<key>) so single_step_batch and the trajectory tests
    read them the same way.  Hover reward only."""
    d = _npz(os.path.join(GOLDEN, "traj_contact.npz"))
    names = [str(n) for n in d["scenarios"] if abs(float(d[f"{n}/dt"]) - dt) < 1e-12]
    v = {k: d[k] for k in d if k.split("/", 1)[0] in names}
    v["scenarios"] = np.array(names)
    v["dt"] = np.array(dt)
    return v


def load_variant(name):
    """traj_var_<name>.npz and the airframe document it was recorded with: the bundled AW109
    parameters with the recorded edits applied (turbulence level, mean wind, mass, rotor speeds)."""
    import copy
    import json
    from heligym_amd import config
    d = _npz(os.path.join(GOLDEN, f"traj_var_{name}.npz"))
    doc = copy.deepcopy(config.load_airframe("aw109"))
    doc["airframe"].update(json.loads(str(d["airframe_edits_json"])))
    return d, doc


# ------------------------------------------------------------------------------------------------
# Heli._is_failed (helicopter.py:226-234): fail_kats.npz, fail_traj.npz

FAIL_CLAUSES = ("contact", "sink", "roll", "pitch", "ns", "ew", "ceiling")   # bit i of a clause byte (HG_FAIL_*)
FAIL_BIT = {c: 1 << i for i, c in enumerate(FAIL_CLAUSES)}
HMAP_H_TOL = 0.0   # ft: tests/test_oracle_golden.py holds the terrain height hmap_h to the reference exactly


def fail_margin(alt):
    """How close to its threshold the altitude of a terrain clause (contact: gta, ceiling: gta + 10000) may lie
    before the clause counts as ambiguous: the suite's tolerance on the interpolated terrain height plus one fp32
    ulp of the altitude."""
    with np.errstate(all="ignore"):
        return HMAP_H_TOL + np.spacing(np.abs(np.asarray(alt, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def fail_inside(alt, gta):
    """[n, 2] bool: the contact / the ceiling clause of each row lies inside fail_margin of the reference's own gta."""
    alt, gta = np.asarray(alt, dtype=np.float64), np.asarray(gta, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = fail_margin(alt)
        return np.stack([np.abs(alt - gta) <= m, np.abs(alt - gta - 10000.0) <= m], axis=1)


def half_extent(airframe=None):
    """(NS_MAX / 2, EW_MAX / 2) ft of an airframe document (default: the bundled AW109): beyond it _is_failed's
    bounds clause fires."""
    from heligym_amd import config
    af = (airframe or config.load_airframe("aw109"))["airframe"]
    return float(af["env_NS_MAX"]) / 2, float(af["env_EW_MAX"]) / 2


def north_out(airframe=None):
    """A north position (ft) past the map's half-extent by about 20 ft, so that the NS clause alone fails an env."""
    return float(np.ceil(half_extent(airframe)[0] + 19.0))


def fail_airframe(edits_json):
    """The airframe document a fail_kats.npz airframe was recorded with: the bundled AW109 with the edits."""
    import copy
    import json
    from heligym_amd import config
    doc = copy.deepcopy(config.load_airframe("aw109"))
    doc["airframe"].update(json.loads(str(edits_json)))
    return doc


def load_fail_kats(airframe):
    """fail_kats.npz for one airframe: heli, dots [n,18] float64 (fp32 values), failed, hit, raises, gta, clauses,
    label, kind, inside [n,2], doc (the airframe document), dtypes."""
    d = _npz(os.path.join(GOLDEN, "fail_kats.npz"))
    k = {key: d[f"{airframe}/{key}"] for key in ("failed", "hit", "raises", "gta", "clauses", "kind", "inside", "thresholds")}
    k["heli"], k["dots"] = d[f"{airframe}/heli"].astype(np.float64), d[f"{airframe}/dots"].astype(np.float64)
    k["label"] = np.array([str(s) for s in d[f"{airframe}/label"]])
    k["doc"] = fail_airframe(d[f"{airframe}/airframe_edits_json"])
    k["dtypes"] = {key: str(d[key]) for key in ("gta_dtype", "altitude_minus_gta_dtype", "euler_compare_dtype",
                                                "zdot_compare_dtype", "state_dtype", "state_dots_dtype")}
    return k


def check_fail_kats(k, failed, clauses, who):
    """The agreement contract on fail_kats.npz.  The single-component clauses (sink, roll, pitch, NS, EW) agree with
    the reference on every row, the fp32 threshold rows included.  Contact and ceiling agree on every row outside
    fail_margin of the reference's own gta; inside it only that clause's bit may differ.  `failed` agrees wherever
    every clause bit does.  Rows on which the reference raises (NaN x or y) are not compared.  Returns (rows whose
    contact bit differs, rows whose ceiling bit differs, least |altitude - threshold| / margin among agreeing
    terrain-clause decisions)."""
    failed, clauses = np.asarray(failed).astype(bool), np.asarray(clauses).astype(np.uint8)
    ok = ~k["raises"]
    diff = (clauses ^ k["clauses"]) & 127
    single = sum(FAIL_BIT[c] for c in ("sink", "roll", "pitch", "ns", "ew"))
    bad = np.nonzero(ok & ((diff & single) != 0))[0]
    assert len(bad) == 0, (who, "single-component clause", [(i, k["label"][i], int(clauses[i]), int(k["clauses"][i])) for i in bad[:10]])
    n_diff = []
    for col, c in ((0, "contact"), (1, "ceiling")):
        d = ok & ((diff & FAIL_BIT[c]) != 0)
        bad = np.nonzero(d & ~k["inside"][:, col])[0]
        alt = -k["heli"][:, 17]
        assert len(bad) == 0, (who, c, [(i, k["label"][i], alt[i] - k["gta"][i] - (10000.0 if col else 0.0)) for i in bad[:10]])
        n_diff.append(int(d.sum()))
    bad = np.nonzero(ok & (diff == 0) & (failed != k["failed"]))[0]
    assert len(bad) == 0, (who, "failed", [(i, k["label"][i]) for i in bad[:10]])
    return n_diff[0], n_diff[1]


def load_fail_traj():
    """fail_traj.npz as {scenario: {dt, fails, action, eta, init_*, failed, terminated, ..., clauses, gta, heli, dots
    (post-step rows with the recorded columns filled in, the rest 0)}}."""
    d = _npz(os.path.join(GOLDEN, "fail_traj.npz"))
    cols = d["cols"]
    out = {}
    for s in (str(x) for x in d["scenarios"]):
        T = len(d[f"{s}/action"])
        e = {"dt": float(d["dt"]), "fails": bool(d[f"{s}/fails"]), "heli": np.zeros((T, 18)), "dots": np.zeros((T, 18))}
        e["heli"][:, cols], e["dots"][:, 17] = d[f"{s}/state_cols"], d[f"{s}/zdot"]
        for key in ("action", "eta", "init_state", "init_wind_state", "init_obs", "init_state_dots", "init_trim_cond",
                    "failed", "successed", "time_up", "terminated", "truncated", "clauses", "gta"):
            e[key] = d[f"{s}/{key}"]
        out[s] = e
    return out


def fail_traj_determinate(heli, dots, gta, thresholds, scale=1.0):
    """Whether `failed` of every recorded step of a free-running episode is the same for every implementation within
    the trajectory tolerance, scaled by `scale`: positions (x, y, altitude), which only integrate, within
    (t + 1) fp32 ulps at step t (one rounding of the stored state per step) plus the terrain margin; roll, pitch
    and the sink rate within contract (ii).  A clause within tolerance of its threshold counts both ways.
    thresholds: (V_TIP * 0.05, 60 deg, NS_MAX / 2, EW_MAX / 2)."""
    heli, dots = np.asarray(heli, dtype=np.float64), np.asarray(dots, dtype=np.float64)
    t_sink, t_ang, t_ns, t_ew = thresholds[:4]
    steps = np.arange(len(heli)) + 1.0
    alt = -heli[:, 17]
    pos = lambda v: scale * (steps * fail_margin(v))  # noqa: E731
    vals = [(gta - alt, pos(alt)), (dots[:, 17] - t_sink, scale * _traj_tol(dots[:, 17])),
            (heli[:, 12] - t_ang, scale * _traj_tol(heli[:, 12])), (heli[:, 13] - t_ang, scale * _traj_tol(heli[:, 13])),
            (np.abs(heli[:, 15]) - t_ns, pos(heli[:, 15])), (np.abs(heli[:, 16]) - t_ew, pos(heli[:, 16])),
            (alt - gta - 10000.0, pos(alt))]
    lo = [v > tol for v, tol in vals]     # holds for certain
    hi = [v > -tol for v, tol in vals]    # may hold
    f = lambda c: (c[0] & (c[1] | c[2] | c[3])) | c[4] | c[5] | c[6]  # noqa: E731
    return bool(np.array_equal(f(lo), f(hi)))
