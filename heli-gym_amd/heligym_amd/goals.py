"""Per-env goals on the host: the device's draw restated in NumPy, and a sampler of goal tables.

`goal_ref` restates csrc/goals.h (goal_draw, goal_record) bitwise, so a learner can recompute the goal of any
stored row from (seed, global env id, episode) alone: one Philox4x32-10 call on the counter (gid_lo, gid_hi,
episode, 0) under the key seed ^ (0x676F616C, 0x5F626F78); u_k = ((word_k >> 8) + 0.5) 2^-24 in float32; field
k = fma(u_k, hi_k - lo_k, lo_k) in float32, clamped into [lo_k, hi_k].  The Philox rounds are the ones
tests/philox_ref.py restates for the turbulence noise (its known-answer vectors pin both).
"""
import numpy as np

from . import config

GOAL_FIELDS = {"hover": ("north_loc", "east_loc", "sea_alt"), "forward_flight": ("sea_alt", "vel")}
_SLOT = {"north_loc": 0, "east_loc": 1, "sea_alt": 2, "vel": 3}   # the record's order
GOAL_KEY = (0x676F616C, 0x5F626F78)
GOAL_TAG = 0
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def _philox4x32_10(ctr, k0, k1):
    """ctr: four uint64 arrays of values < 2^32; k0, k1: ints -> four uint32 arrays."""
    x, y, z, w = (np.asarray(c, dtype=np.uint64).copy() for c in ctr)
    k0, k1 = np.uint64(k0 & _MASK), np.uint64(k1 & _MASK)
    m = np.uint64(_MASK)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * x, np.uint64(_M1) * z   # exact: 32 x 32 bits
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ w ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(_W0)) & m, (k1 + np.uint64(_W1)) & m
    return [v.astype(np.uint32) for v in (x, y, z, w)]


def _u01(x):
    a = (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (a + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def _fma32(u, w, c):
    """fma(u, w, c) of float32 arrays with one rounding: the product is exact in float64 (24 + 24 bits), the
    sum's float64 rounding error is recovered (TwoSum) and decides the one case in which rounding the float64
    sum to float32 would round twice -- a sum that sits midway between two float32 numbers."""
    p = u.astype(np.float64) * w.astype(np.float64)
    a = c.astype(np.float64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    f = s.astype(np.float32)
    r = s - f.astype(np.float64)                       # exact; its sign points from f to s
    g = np.nextafter(f, np.where(r > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (r != 0) & (np.abs(s - g.astype(np.float64)) == np.abs(r))
    return np.where(tie & (err != 0) & (np.sign(err) == np.sign(r)), g, f).astype(np.float32)


def _task_name(task):
    if task in GOAL_FIELDS:
        return task
    for name, code in config.TASKS.items():
        if code == task and name in GOAL_FIELDS:
            return name
    raise ValueError(f"task {task!r} has no target; one of {sorted(GOAL_FIELDS)}")


def box_arrays(box, task, target=None):
    """(lo, hi) float32 [4] in the record's order {north_loc, east_loc, sea_alt, vel} of a {field: (lo, hi)}
    box: keys checked against the task's fields, finite, lo <= hi, vel > 0; a field the task does not use, or a
    missing one, takes `target` (default: the task's default target) for both ends."""
    task = _task_name(task)
    fields = GOAL_FIELDS[task]
    if not isinstance(box, dict) or not box:
        raise ValueError(f"box must be a non-empty dict {{field: (lo, hi)}} over {fields}")
    unknown = sorted(set(box) - set(fields))
    if unknown:
        raise ValueError(f"box: unknown field(s) {unknown} for task {task!r}; its fields are {fields}")
    own = dict.fromkeys(_SLOT, 0.0)
    own.update(config.DEFAULT_TARGETS[task])
    own.update(target or {})
    lo, hi = np.zeros(4), np.zeros(4)
    for name, k in _SLOT.items():
        r = box.get(name, own[name])
        a, b = (r, r) if np.isscalar(r) else r
        a, b = float(a), float(b)
        if name in fields:
            if not (np.isfinite(a) and np.isfinite(b)):
                raise ValueError(f"box[{name!r}] must be finite, got {r}")
            if a > b:
                raise ValueError(f"box[{name!r}]: lo > hi ({a} > {b})")
            if name == "vel" and not a > 0:
                raise ValueError(f"box['vel']: vel <= 0 ({a}); the forward-flight reward divides by the speed")
        lo[k], hi[k] = a, b
    return lo.astype(np.float32), hi.astype(np.float32)


def goal_ref(seed, env_ids, episodes, box, task, airframe="aw109", target=None):
    """The goal of global env ids `env_ids` in episodes `episodes` (broadcast against each other) of a box-mode
    handle with this seed: a dict of float32 arrays over the task's fields, plus `record` [M,8] float32, the
    device record {north / n_x, east / n_x, -sea_alt / n_x, vel / n_v, north, east, sea_alt, vel}.  Bitwise
    hg_goal_draw and the step kernels' reset branch.  `airframe`: a name or document (the normalisers);
    `target`: the handle's target, which fills the fields the task does not use."""
    task = _task_name(task)
    lo, hi = box_arrays(box, task, target)
    gid, epi = np.broadcast_arrays(np.atleast_1d(np.asarray(env_ids, dtype=np.int64)).ravel(),
                                   np.atleast_1d(np.asarray(episodes, dtype=np.int64)).ravel())
    g64 = gid.astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = (g64 & np.uint64(_MASK), g64 >> np.uint64(32), epi.astype(np.uint64) & np.uint64(_MASK),
           np.full(g64.shape, GOAL_TAG, dtype=np.uint64))
    words = _philox4x32_10(ctr, (seed & _MASK) ^ GOAL_KEY[0], (seed >> 32) ^ GOAL_KEY[1])
    g = np.empty((len(g64), 4), dtype=np.float32)
    for k in range(4):
        n = len(g64)
        v = _fma32(_u01(words[k]), np.full(n, hi[k] - lo[k], dtype=np.float32), np.full(n, lo[k], dtype=np.float32))
        g[:, k] = np.minimum(np.maximum(v, lo[k]), hi[k])
    af = config.load_airframe(airframe)["airframe"] if not hasattr(airframe, "mr_R") else None
    R, grav = (float(af["mr_R"]), float(af["env_GRAV"])) if af is not None else (airframe.mr_R, airframe.env_GRAV)
    n_x, n_v = 2 * R, float(np.sqrt(2 * R * grav))
    d = g.astype(np.float64)
    rec = np.concatenate([np.stack([d[:, 0] / n_x, d[:, 1] / n_x, -d[:, 2] / n_x, d[:, 3] / n_v], axis=1).astype(np.float32),
                          g], axis=1)
    out = {name: g[:, _SLOT[name]].copy() for name in GOAL_FIELDS[task]}
    out["record"] = rec
    return out


def sample_goals(n, task, around=None, spread=None, seed=0):
    """Uniform draws of n goals for HeliVecEnv.set_goals(goals=sample_goals(n, ...)): a dict of [n] float64 arrays
    over the task's fields, field f inside [around[f] - spread[f], around[f] + spread[f]], a function of `seed`
    alone (NumPy's PCG64).  `around` defaults to the task's default target; `spread` to 200 ft north / east,
    100 ft of altitude and 20 ft/s of speed (kept above 1 ft/s)."""
    task = _task_name(task)
    centre = dict(config.DEFAULT_TARGETS[task])
    centre.update(around or {})
    sp = {"north_loc": 200.0, "east_loc": 200.0, "sea_alt": 100.0, "vel": 20.0}
    sp.update(spread or {})
    unknown = sorted((set(around or {}) | set(spread or {})) - set(_SLOT))
    if unknown:
        raise ValueError(f"sample_goals: unknown field(s) {unknown}")
    rng = np.random.default_rng(seed)
    out = {}
    for name in GOAL_FIELDS[task]:
        c, s = float(centre[name]), float(sp[name])
        if not (np.isfinite(c) and np.isfinite(s) and s >= 0):
            raise ValueError(f"sample_goals: {name} needs a finite centre and a spread >= 0, got {c}, {s}")
        v = c + s * (2.0 * rng.random(int(n)) - 1.0)
        out[name] = np.maximum(v, 1.0) if name == "vel" else v
    return out
