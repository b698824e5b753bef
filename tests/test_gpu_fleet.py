"""GPU: mixed fleets (HeliVecEnv.set_fleet / hg_set_fleet), one airframe class per 64-env state tile.

  1. one fleet handle holds the reference's recordings of several airframes and steps each batch inside the
     project's contract (i), the contract each variant is held to alone (test_gpu_parity);
  2. a fleet's rows in class-c tiles are bitwise the same rows of an ordinary handle of airframe c with the
     same N, seed and env_offset (envs are independent, the noise is keyed by global env id): per step with
     crashes, TimeLimit truncations and resets to the class's own template, interleaved tiles and a ragged last
     tile, in the lone-wave and in the bulk kernel, the rotor azimuths (per-class rotor speeds) included;
  3. the same for every rollout: open-loop (injected and in-kernel noise), policy, actor-critic, population
     (member blocks off the class tiles), branched and policy-guided branched;
  4. setters, revert, refusals, a class whose trim fails, get_fleet;
  5. 20 captured steps replayed equal 20 eager ones.
The classes are the bundled AW109 and the recorded variants of tests/golden (heavy: other mass and both rotor
speeds; wing: a winged airframe; turb*: other ENV blocks).  Run with -m gpu."""
import copy
import functools

import numpy as np
import pytest

import golden_cases as gc
from test_gpu_parity import check_vs_reference
from test_gpu_policy_rollout import _set, policy  # noqa: F401  (a fixed-seed 17-64-64-4 policy)

pytestmark = pytest.mark.gpu

SEED = 3
MAX_STEPS = 150


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


@functools.lru_cache(maxsize=None)
def _doc(name):
    from heligym_amd import config
    return config.load_airframe("aw109") if name == "aw109" else gc.load_variant(name)[1]


def _env(n, name="aw109", **kw):
    from heligym_amd import HeliVecEnv
    kw.setdefault("autoreset", True)
    kw.setdefault("max_episode_steps", MAX_STEPS)
    kw.setdefault("dt", 0.01)
    return HeliVecEnv(n, task="hover", heli_name=copy.deepcopy(_doc(name)), seed=SEED, device="cuda:0", **kw)


def _class_rows(torch, tile_class, n):
    """Per class, the env indices of its tiles (device int64 tensors)."""
    cls = np.repeat(np.asarray(tile_class), 64)[:n]
    return [torch.as_tensor(np.nonzero(cls == c)[0], device="cuda:0") for c in range(int(cls.max()) + 1)]


def _bits(torch, x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def _same(torch, a, b, idx, what, dim=0):
    """a and b bitwise equal on the rows `idx` of dimension `dim`."""
    x, y = _bits(torch, a.index_select(dim, idx)), _bits(torch, b.index_select(dim, idx))
    if not torch.equal(x, y):
        bad = (x != y).nonzero()
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()} "
                             f"(row {int(idx[bad[0][dim]])})")


# ------------------------------------------------------------------------------------------------ 1. reference parity
def _pad_tiles(b):
    """A single-step batch's per-row arrays padded to whole tiles by repeating the first row."""
    n = len(b["state"])
    pad = (-n) % 64
    take = np.concatenate([np.arange(n), np.zeros(pad, dtype=np.int64)])
    return {k: b[k][take] for k in ("state", "counters", "actions", "eta")}, n


@pytest.mark.parametrize("tag,names", [("0.01", ("turb5", "heavy", "wing")), ("0.02", ("turb7_wind", "turb0"))])
def test_reference_parity_of_every_class_in_one_handle(torch, tag, names):
    """Contract (i) of test_single_step_vs_reference(_parameter_variants), every batch in one fleet handle."""
    batches = [("aw109", f"{tag}/hover", gc.single_step_batch(gc.load(tag), "hover"))]
    rows = {"turb5": 450, "heavy": 581, "wing": 500, "turb7_wind": 500, "turb0": 240}
    for nm in names:
        b = gc.single_step_batch(gc.load_variant(nm)[0], "hover")
        assert len(b["state"]) == rows[nm] and abs(b["dt"] - float(tag)) < 1e-12, (nm, len(b["state"]), b["dt"])
        batches.append((nm, f"var_{nm}/hover", b))
    parts, spans, tile_class, at = [], [], [], 0
    for c, (_, _, b) in enumerate(batches):
        p, n = _pad_tiles(b)
        parts.append(p)
        spans.append((at, at + n))
        tile_class += [c] * (len(p["state"]) // 64)
        at += len(p["state"])
    cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    env = _env(at, dt=float(tag), autoreset=False, max_episode_steps=None)
    status = env.set_fleet([_doc(nm) for nm, _, _ in batches], tile_class=tile_class)
    assert status.tolist() == [0] * len(batches)
    env.set_state(cat["state"].astype(np.float32), cat["counters"].astype(np.int32))
    act = torch.as_tensor(cat["actions"].astype(np.float32), device=env.device)
    eta = torch.as_tensor(cat["eta"].astype(np.float32), device=env.device)
    obs, rew, term, trunc, info = env.step(act, eta=eta)
    st, ctr = env.get_state()
    torch.cuda.synchronize()
    out = {"obs": obs.cpu().numpy().astype(np.float64), "reward": rew.cpu().numpy().astype(np.float64),
           "terminated": term.cpu().numpy(), "truncated": trunc.cpu().numpy(),
           "state": st.cpu().numpy().astype(np.float64), "counters": ctr.cpu().numpy()}
    for k in ("failed", "successed", "time_up", "success_step"):
        out[k] = info[k].cpu().numpy()
    env.close()
    for (nm, rt_name, b), (s, e) in zip(batches, spans):
        check_vs_reference(b, {k: v[s:e] for k, v in out.items()}, "hover", rt_name)


# ------------------------------------------------------------------------------------------------ 2. per step
CLASSES = ("aw109", "heavy", "wing")


def _lockstep(torch, fleet, refs, rows, K, every):
    """K steps of the fleet handle and its per-class reference handles with the same actions; observations,
    rewards, both flags, state and counters every `every` steps and at the end, class by class, bitwise.
    Returns the number of done flags among each class's compared rows and the fleet's state at the first check
    (mid-episode: at a multiple of the time limit every surviving env has just been reset)."""
    n = fleet.num_envs
    first = None
    act = torch.empty((n, 4), dtype=torch.float32, device=fleet.device)
    done = torch.zeros((n,), dtype=torch.int64, device=fleet.device)
    for k in range(K):
        fleet.random_actions(act, seed=8, step=k)
        act[::4, 0] = -1.0   # low collective on every fourth env: crashes, resets from the class's template
        obs, rew, term, trunc, _ = fleet.step(act)
        done += (term | trunc)
        outs = [r.step(act) for r in refs]
        if k % every == every - 1 or k == K - 1:
            for c, (idx, (o, r, te, tr, _)) in enumerate(zip(rows, outs)):
                tag = f"step {k}, class {c}"
                _same(torch, obs, o, idx, "obs, " + tag)
                _same(torch, rew, r, idx, "reward, " + tag)
                _same(torch, term, te, idx, "terminated, " + tag)
                _same(torch, trunc, tr, idx, "truncated, " + tag)
            st, ctr = fleet.get_state()
            for c, (idx, r) in enumerate(zip(rows, refs)):
                rs, rc = r.get_state()
                _same(torch, st, rs, idx, f"state (azimuths in columns 2, 3), step {k}, class {c}")
                _same(torch, ctr, rc, idx, f"counters, step {k}, class {c}")
            first = st.clone() if first is None else first
    return [int(done[idx].sum()) for idx in rows], first


def _fleet_and_refs(n, tile_class, **kw):
    fleet = _env(n, **kw)
    status = fleet.set_fleet([_doc(nm) for nm in CLASSES], tile_class=tile_class)
    assert status.tolist() == [0, 0, 0]
    refs = [_env(n, nm, **kw) for nm in CLASSES]
    for e in [fleet] + refs:
        e.reset()
    return fleet, refs


def test_interleaved_tiles_bitwise_equal_one_handle_per_class(torch):
    n, tile_class = 64 * 7 + 37, [0, 1, 2, 1, 0, 2, 0, 1]
    fleet, refs = _fleet_and_refs(n, tile_class)
    rows = _class_rows(torch, tile_class, n)
    assert sum(len(r) for r in rows) == n and len(rows[1]) == 64 * 2 + 37
    before = fleet.debug_launches()
    done, st = _lockstep(torch, fleet, refs, rows, 300, 50)
    after = fleet.debug_launches()
    assert all(d > 0 for d in done), done   # every class reset (crashes, and the time limit at step 150)
    assert after["lone_wave"] - before["lone_wave"] == 300 and after["bulk"] == before["bulk"], (before, after)
    assert after["helper"] == after["specialized"] == 0, after
    # the classes do differ: the heavy variant turns both rotors at other speeds
    a = st[:, 2:4]   # (step 50)
    assert bool((a != 0).all()) and not torch.equal(a[rows[0]][:64], a[rows[1]][:64])
    print(f"\n[fleet interleaved] done flags per class over 300 steps: {done}")
    for e in [fleet] + refs:
        e.close()


def test_bulk_kernel_bitwise_equal_one_handle_per_class(torch):
    """Past the lone-wave range (two waves per SIMD), sized from the device: contiguous thirds, and tile 1 given
    class 1 between two class-0 tiles, so that an off-by-one in the tile index shows at once."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * (2 * 64 * 4 * cus) + 65
    tiles = (n + 63) // 64
    tile_class = np.minimum(np.arange(tiles) * 3 // tiles, 2).astype(np.int32)
    tile_class[1] = 1
    assert tile_class[0] == tile_class[2] == 0 and tile_class[-1] == 2
    fleet, refs = _fleet_and_refs(n, tile_class, max_episode_steps=60)   # (100 steps: resets at the time limit)
    rows = _class_rows(torch, tile_class, n)
    before = fleet.debug_launches()
    done, _ = _lockstep(torch, fleet, refs, rows, 100, 50)
    after = fleet.debug_launches()
    assert after["bulk"] - before["bulk"] == 100 and after["lone_wave"] == before["lone_wave"], (before, after)
    assert all(d > 0 for d in done), done
    print(f"\n[fleet bulk] N = {n}, done flags per class over 100 steps: {done}")
    for e in [fleet] + refs:
        e.close()


# ------------------------------------------------------------------------------------------------ 3. rollouts
N3, TILES3, K3 = 64 * 4 + 19, [0, 1, 2, 1, 0], 40


@pytest.fixture(scope="module")
def trio(torch, policy):  # noqa: F811
    """The fleet handle of test 3 and its reference handles, with the policy and a value head."""
    fleet, refs = _fleet_and_refs(N3, TILES3)
    head = (torch.linspace(-0.3, 0.3, 64), torch.tensor([0.1]))
    for e in [fleet] + refs:
        _set(e, policy)
        e.set_value_head(head)
    yield fleet, refs, _class_rows(torch, TILES3, N3)
    for e in [fleet] + refs:
        e.close()


def _restart(envs, near_limit):
    """Every handle reset; every fifth env `near_limit` steps from its time limit (truncations and resets to the
    class's template inside a rollout)."""
    for e in envs:
        e.reset()
        _, ctr = e.get_state()
        ctr = ctr.clone()
        ctr[::5, 0] = MAX_STEPS - near_limit
        e.set_state(None, ctr)


def _same_state(torch, fleet, refs, rows, what):
    st, ctr = fleet.get_state()
    for c, (idx, r) in enumerate(zip(rows, refs)):
        rs, rc = r.get_state()
        _same(torch, st, rs, idx, f"state after {what}, class {c}")
        _same(torch, ctr, rc, idx, f"counters after {what}, class {c}")


def test_every_stepping_rollout_bitwise_equals_one_handle_per_class(torch, trio):
    fleet, refs, rows = trio
    _restart([fleet] + refs, 20)
    g = torch.Generator().manual_seed(5)
    act = (2.0 * torch.rand((K3, N3, 4), generator=g) - 1.0).to("cuda:0")
    eta = torch.randn((K3, N3, 3), generator=g).to("cuda:0") * 10.0   # (1 / sqrt(dt) = 10)
    for name, kw in (("rollout, in-kernel noise", {}), ("rollout, injected noise", dict(eta=eta))):
        out = fleet.rollout(act, **kw)
        for c, (idx, r) in enumerate(zip(rows, refs)):
            for j, (x, y) in enumerate(zip(out, r.rollout(act, **kw))):
                _same(torch, x, y, idx, f"{name}, output {j}, class {c}", dim=1)
        if not kw:
            assert int(out[3].sum()) > 0   # truncated, and reset from a per-class template, inside the rollout
    _same_state(torch, fleet, refs, rows, "rollout")
    obs0 = out[0][-1].contiguous()
    pol = fleet.rollout_policy(K3, obs0=obs0)
    for c, (idx, r) in enumerate(zip(rows, refs)):
        for j, (x, y) in enumerate(zip(pol, r.rollout_policy(K3, obs0=obs0))):
            _same(torch, x, y, idx, f"rollout_policy output {j}, class {c}", dim=1)
    _restart([fleet] + refs, 20)
    obs0 = fleet.get_fleet()["templates"][:, 22:].contiguous()
    ac = fleet.rollout_actor_critic(K3, obs0=obs0)
    assert int(ac["truncated"].sum()) > 0
    assert torch.isfinite(ac["value"]).all() and torch.isfinite(ac["next_value"]).all()
    for c, (idx, r) in enumerate(zip(rows, refs)):
        ra = r.rollout_actor_critic(K3, obs0=obs0)
        for key in ("actions", "obs", "reward", "terminated", "truncated", "info", "logp", "value", "next_value",
                    "advantages"):
            _same(torch, ac[key], ra[key], idx, f"rollout_actor_critic {key}, class {c}", dim=1)
    _same_state(torch, fleet, refs, rows, "rollout_actor_critic")
    # a population whose member blocks (128 envs) and class tiles do not coincide
    _restart([fleet] + refs, 6)
    P = (N3 + 127) // 128
    thetas = (0.1 * torch.randn((P, 5641), generator=g)).to("cuda:0")
    images = fleet.pop_pack(thetas)
    pop = fleet.rollout_population(12, images, 128, obs0=obs0)
    assert int(pop[4].sum()) > 0
    for c, (idx, r) in enumerate(zip(rows, refs)):
        for j, (x, y) in enumerate(zip(pop, r.rollout_population(12, images, 128, obs0=obs0))):
            _same(torch, x, y, idx, f"rollout_population output {j}, class {c}", dim=1)
    _same_state(torch, fleet, refs, rows, "rollout_population")


def test_branched_rollouts_bitwise_equal_one_handle_per_class(torch, trio):
    from heligym_amd import HeliGymError
    fleet, refs, rows = trio
    _restart([fleet] + refs, 10)
    H = 24
    g = torch.Generator().manual_seed(6)
    for B, noise in ((16, "env"), (64, "env"), (16, "off")):
        act = (2.0 * torch.rand((H, N3 * B, 4), generator=g) - 1.0).to("cuda:0")
        out = fleet.rollout_branch(act, B, gamma=0.98, noise=noise)
        # every fifth env's branches end at the time limit, the others' run the horizon
        assert int((out["alive_steps"] < H).sum()) > 0 and int((out["alive_steps"] == H).sum()) > 0
        for c, (idx, r) in enumerate(zip(rows, refs)):
            ro = r.rollout_branch(act, B, gamma=0.98, noise=noise)
            for key in ("returns", "alive_steps", "end_info"):
                _same(torch, out[key], ro[key], idx, f"rollout_branch {key}, branches {B}, noise {noise}, class {c}")
    # the classes' branches do differ
    assert not torch.equal(out["returns"][rows[0]][:64], out["returns"][rows[1]][:64])
    _same_state(torch, fleet, refs, rows, "the branched rollouts (which touch no state)")
    # a wave's 64 rows must belong to one tile
    act3 = torch.zeros((H, N3 * 3, 4), device="cuda:0")
    with pytest.raises(HeliGymError, match="branches must divide 64 or be a multiple of 64"):
        fleet.rollout_branch(act3, 3)
    refs[0].rollout_branch(act3, 3)   # (an ordinary handle takes any count)


def test_policy_guided_branches_bitwise_equal_one_handle_per_class(torch, trio):
    """rollout_branch_policy, branches 64, bootstrap on, against the per-class reference handles, bitwise.  (The
    heavy and wing references run the generic-constant kernels of csrc/branch_policy_generic.hip, which
    tests/test_gpu_branch_policy_generic.py holds against the constant-specialised ones.)"""
    fleet, refs, rows = trio
    _restart([fleet] + refs, 10)
    H, B = 24, 64
    g = torch.Generator().manual_seed(7)
    obs0 = fleet.get_fleet()["templates"][:, 22:].contiguous()
    res = (0.4 * torch.rand((H, N3 * B, 4), generator=g) - 0.2).to("cuda:0")
    out = fleet.rollout_branch_policy(res, B, obs0=obs0, gamma=0.98, bootstrap=True, lo=-1.0, hi=1.0)
    assert torch.isfinite(out["returns"]).all()
    assert int((out["alive_steps"] < H).sum()) > 0 and int((out["alive_steps"] == H).sum()) > 0
    assert int(out["alive_steps"].min()) >= 1 and int(out["alive_steps"].max()) == H
    for c, (idx, r) in enumerate(zip(rows, refs)):
        ro = r.rollout_branch_policy(res, B, obs0=obs0, gamma=0.98, bootstrap=True, lo=-1.0, hi=1.0)
        for key in ("returns", "alive_steps", "end_info"):
            _same(torch, out[key], ro[key], idx, f"rollout_branch_policy {key}, class {c}")
    act3 = torch.zeros((H, N3 * 3, 4), device="cuda:0")
    from heligym_amd import HeliGymError
    with pytest.raises(HeliGymError, match="branches must divide 64 or be a multiple of 64"):
        fleet.rollout_branch_policy(act3, 3, obs0=obs0)


# ------------------------------------------------------------------------------------------------ 4. surface
def test_setters_act_on_every_class(torch):
    n, tile_class = 64 * 2 + 5, [0, 1, 2]
    fleet, refs = _fleet_and_refs(n, tile_class)
    rows = _class_rows(torch, tile_class, n)
    for e in [fleet] + refs:
        e.set_target({"sea_alt": 3700.0, "north_loc": 40.0})
        e.set_max_time(0.6)   # time_up after 61 steps of 0.01 s
    done, _ = _lockstep(torch, fleet, refs, rows, 80, 20)
    assert all(d > 0 for d in done), done
    for e in [fleet] + refs:
        e.close()


def test_revert_is_bitwise_a_handle_that_never_had_a_fleet(torch):
    n = 64 * 2 + 5
    fleet, plain = _env(n), _env(n)
    fleet.set_fleet([_doc(nm) for nm in CLASSES], tile_class=[2, 1, 0])
    fleet.reset()
    act = torch.empty((n, 4), dtype=torch.float32, device=fleet.device)
    for k in range(10):
        fleet.random_actions(act, seed=8, step=k)
        fleet.step(act)
    assert fleet.set_fleet(None) is None
    assert fleet.get_fleet()["tile_class"].tolist() == [0, 0, 0] and len(fleet.get_fleet()["airframes"]) == 1
    ctr = fleet.get_state()[1].clone()
    ctr[:, 2] = 0   # (the episode index keys the noise: the same episode as the plain handle's first)
    fleet.set_state(None, ctr)
    fleet.reset()
    plain.reset()
    every = torch.arange(n, device="cuda:0")
    _lockstep(torch, fleet, [plain], [every], 50, 10)
    la = fleet.debug_launches()
    assert la["helper"] == 50, la   # back on the handle's own kernels
    for e in (fleet, plain):
        e.close()


def test_refusals_leave_the_handle_as_it_was(torch):
    from heligym_amd import HeliGymError
    n, tile_class = 64 * 2 + 5, [0, 1, 2]
    docs = [_doc(nm) for nm in CLASSES]
    fleet = _env(n)
    fleet.set_fleet(docs, tile_class=tile_class)
    with pytest.raises(HeliGymError, match="a fleet is set"):
        fleet.set_weather(turb_level=2.0)
    with pytest.raises(HeliGymError, match="a fleet is set"):
        fleet.set_trim_cond({"gr_alt": 200.0})
    with pytest.raises(HeliGymError, match="a fleet is set"):
        fleet.set_trim_conds([{"gr_alt": 200.0}] * n)
    with pytest.raises(HeliGymError, match="a fleet is set"):
        fleet.set_trim_conds(None)
    lib, h = fleet.lib, fleet._h
    from heligym_amd.vector import fleet_arrays
    import ctypes
    arr, tc = fleet_arrays(docs, n, tile_class=tile_class)
    p32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))   # noqa: E731
    status = np.full(3, -99, dtype=np.int32)

    def refused(rc, text):
        assert rc == -1 and text.encode() in lib.hg_last_error(), (rc, lib.hg_last_error())
        assert status.tolist() == [-99] * 3   # outputs untouched

    refused(lib.hg_set_fleet(h, arr, None, 0, p32(tc), p32(status), None), "n_classes must be in [1, 3]")
    refused(lib.hg_set_fleet(h, arr, None, 4, p32(tc), p32(status), None), "n_classes must be in [1, 3]")
    refused(lib.hg_set_fleet(h, arr, None, 3, None, p32(status), None), "tile_class is NULL")
    for bad in ([0, 1, 3], [0, -1, 2]):
        refused(lib.hg_set_fleet(h, arr, None, 3, p32(np.array(bad, dtype=np.int32)), p32(status), None),
                "is outside [0, n_classes)")
    with pytest.raises(ValueError, match="tile_class must have 3 entries"):
        fleet.set_fleet(docs, tile_class=[0, 1])
    arr2, _ = fleet_arrays(docs, n, tile_class=tile_class)
    arr2[1].IX = float("inf")
    refused(lib.hg_set_fleet(h, arr2, None, 3, p32(tc), p32(status), None), "class 1: a non-finite airframe field")
    for field in ("env_MAX_GR_ALT", "env_NS_MAX", "env_EW_MAX"):
        other = copy.deepcopy(docs)
        other[2]["airframe"][field] *= 1.5
        with pytest.raises(HeliGymError, match="class 2: env_MAX_GR_ALT, env_NS_MAX and env_EW_MAX must be the handle's"):
            fleet.set_fleet(other, tile_class=tile_class)
    # every refusal above left the fleet in place
    got = fleet.get_fleet()
    assert got["tile_class"].tolist() == tile_class and len(got["airframes"]) == 3
    fleet.close()
    wenv = _env(n)
    wenv.set_weather(turb_level=3.0)
    with pytest.raises(HeliGymError, match="per-env weather is set"):
        wenv.set_fleet(docs, tile_class=tile_class)
    wenv.close()
    renv = _env(n, reset_mode="retrim", autoreset=False)
    with pytest.raises(HeliGymError, match="HG_RESET_TEMPLATE"):
        renv.set_fleet(docs, tile_class=tile_class)
    renv.close()


def test_a_failing_class_trim_names_the_class_and_changes_nothing(torch):
    from heligym_amd import HeliGymError
    n, tile_class = 64 * 2 + 5, [0, 1, 2]
    fleet, plain = _env(n), _env(n)
    docs = [copy.deepcopy(_doc(nm)) for nm in CLASSES]
    docs[1]["airframe"]["WT"] *= 50.0
    with pytest.raises(HeliGymError, match=r"error -3: trim failed for classes \[1\] \(1 of 3\)") as ei:
        fleet.set_fleet(docs, tile_class=tile_class)
    assert ei.value.status.tolist() == [0, -3, 0]
    assert len(fleet.get_fleet()["airframes"]) == 1
    for e in (fleet, plain):
        e.reset()
    every = torch.arange(n, device="cuda:0")
    _lockstep(torch, fleet, [plain], [every], 30, 10)
    for e in (fleet, plain):
        e.close()


def test_get_fleet_returns_what_was_set(torch):
    n, tile_class = 64 * 2 + 5, [1, 2, 0]
    docs = [_doc(nm) for nm in CLASSES]
    conds = [{"gr_alt": 100.0}, {"gr_alt": 400.0}, {"gr_alt": 150.0, "yaw": 0.3}]
    fleet = _env(n)
    assert fleet.set_fleet(docs, tile_class=tile_class, conds=conds).tolist() == [0, 0, 0]
    got = fleet.get_fleet()
    assert got["tile_class"].dtype == np.int32 and got["tile_class"].tolist() == tile_class
    assert len(got["airframes"]) == 3
    for af, doc in zip(got["airframes"], docs):
        for k, v in af.items():
            assert v == (int(doc["airframe"][k]) if k == "env_TURB_LVL" else float(doc["airframe"][k])), k
    tm = got["templates"].cpu().numpy()
    assert tm.shape == (n, 39)
    for t, c in enumerate(tile_class):
        ref = _env(64, CLASSES[c], trim_cond=conds[c])
        r = ref.template()
        ref.close()
        o = r["obs"].astype(np.float32)
        want = np.concatenate([r["state"].astype(np.float32), o[4:7], o[16:17], o])
        blk = tm[64 * t:min(n, 64 * (t + 1))]
        np.testing.assert_array_equal(blk.view(np.int32), np.broadcast_to(want, blk.shape).view(np.int32),
                                      err_msg=f"tile {t}, class {c}")
    # envs_per_class: consecutive blocks
    fleet.set_fleet(docs[:2], envs_per_class=128)
    assert fleet.get_fleet()["tile_class"].tolist() == [0, 0, 1]
    fleet.close()


# ------------------------------------------------------------------------------------------------ 5. capture
def test_captured_steps_of_a_fleet_replay_like_eager(torch):
    n, K, tile_class = 64 * 7 + 37, 20, [0, 1, 2, 1, 0, 2, 0, 1]
    outs = []
    for use_graph in (False, True):
        env = _env(n)
        env.set_fleet([_doc(nm) for nm in CLASSES], tile_class=tile_class)
        env.reset()
        bank = torch.empty((K, n, 4), dtype=torch.float32, device=env.device)
        for k in range(K):
            env.random_actions(bank[k], seed=4, step=k)
        torch.cuda.synchronize()
        if use_graph:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for k in range(K):
                    env.step_async(bank[k], with_reset_info=False)
            env.reset()                      # capture does not execute: start from the reset state
            g.replay()
        else:
            env.reset()                      # same episode index (it keys the noise) as the graph run
            for k in range(K):
                env.step_async(bank[k], with_reset_info=False)
        torch.cuda.synchronize()
        st, ctr = env.get_state()
        outs.append((env.obs.cpu().numpy().copy(), st.cpu().numpy().copy(), ctr.cpu().numpy().copy()))
        env.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
