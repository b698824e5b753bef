"""GPU: per-env weather (HeliVecEnv.set_weather / hg_set_weather).  One handle whose envs differ in turbulence
level, mean wind direction and speed steps every env bitwise like a handle whose airframe document has that
env's ENV block (same seed, global env id and reset template): per step with auto-resets, in the rollouts, in
both launch variants a weather handle runs, and against the reference's own recordings at other weathers with
the project's contract (i).  The weathers are the airframe's default and the recorded ones of
tests/golden/traj_var_turb5.npz, traj_var_turb7_wind.npz and traj_var_turb0.npz.  Run with -m gpu.

Not tested: a wind no trim converges for.  The host trim (hg_trim) of the default airframe converges for every
mean wind tried up to 199 ft/s from four sides, so there is no such case below 200 ft/s to report per env."""
import ctypes
import functools

import numpy as np
import pytest

import golden_cases as gc
from test_gpu_parity import TRIM_REL, check_vs_reference
from test_gpu_policy_rollout import _set, policy  # noqa: F401  (a fixed-seed 17-64-64-4 policy)

pytestmark = pytest.mark.gpu

SEED = 17


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


@functools.lru_cache(maxsize=None)
def _weather(name):
    """(airframe document, (turb_level, wind_dir, wind_spd)) of a recorded weather or the default one."""
    from heligym_amd import config
    doc = "aw109" if name == "default" else gc.load_variant(name)[1]
    af = config.make_config(heli_name=doc)[0].af
    return doc, (float(af.env_TURB_LVL), float(af.env_WIND_DIR_deg), float(af.env_WIND_SPD))


def _env(n, doc="aw109", offset=0, dt=0.01, **kw):
    from heligym_amd import HeliVecEnv
    kw.setdefault("autoreset", True)
    return HeliVecEnv(n, task="hover", dt=dt, heli_name=doc, seed=SEED, env_offset=offset, device="cuda:0", **kw)


def _set_weather(env, names, conds=None):
    w = np.array([_weather(nm)[1] for nm in names], dtype=np.float32)   # (_weather is cached: N may be large)
    return env.set_weather(turb_level=w[:, 0], wind_dir=w[:, 1], wind_spd=w[:, 2], conds=conds)


def _give_templates(env, rows):
    """The weather handle's own template rows as a plain handle's per-env reset templates."""
    from heligym_amd.vector import _ptr
    rows = rows.contiguous()
    env._check(env.lib.hg_set_reset_templates(env._h, _ptr(rows), env._stream()))


def _same(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    if a.dtype == np.float32:
        a, b = a.view(np.int32), b.view(np.int32)
    np.testing.assert_array_equal(a, b, err_msg=what)


def _lockstep(torch, wenv, refs, K, every=25):
    """Step the weather handle and its reference handles (start, end, env) together with the actions of
    test_gpu_variants._run; every `every` steps and at the end compare observations, rewards, done flags and
    get_state() block by block, bitwise.  Returns the number of done flags per block."""
    n = wenv.num_envs
    act = torch.empty((n, 4), dtype=torch.float32, device=wenv.device)
    done = torch.zeros((n,), dtype=torch.int64, device=wenv.device)
    for k in range(K):
        wenv.random_actions(act, seed=8, step=k)
        act[::3, 0] = -1.0   # low collective on every third env: crashes and resets
        obs, rew, term, trunc, _ = wenv.step(act)
        done += (term | trunc)
        outs = [env.step(act[s:e].contiguous()) for s, e, env in refs]
        if k % every == every - 1 or k == K - 1:
            st, ctr = wenv.get_state()
            for (s, e, env), (o, r, te, tr, _) in zip(refs, outs):
                tag = f"step {k}, envs [{s}, {e})"
                _same(obs[s:e], o, "obs, " + tag)
                _same(rew[s:e], r, "reward, " + tag)
                _same(term[s:e], te, "terminated, " + tag)
                _same(trunc[s:e], tr, "truncated, " + tag)
                rs, rc = env.get_state()
                _same(st[s:e], rs, "state, " + tag)
                _same(ctr[s:e], rc, "counters, " + tag)
    return [int(done[s:e].sum()) for s, e, _ in refs]


BLOCKS = ((0, 70, "default", 100.0), (70, 139, "turb7_wind", 2500.0), (139, 200, "turb5", 1500.0))


@pytest.fixture(scope="module")
def blocks(torch):
    """One handle of 200 envs in three contiguous weathers and ground altitudes (edges off the wave size: waves
    mix weathers, and lanes above and below 1 000 ft), and a plain handle per block with that weather as
    its airframe document's, the block's env ids and the weather handle's own template rows."""
    wenv = _env(200)
    names = [nm for s, e, nm, _ in BLOCKS for _ in range(s, e)]
    conds = [{"gr_alt": alt} for s, e, _, alt in BLOCKS for _ in range(s, e)]
    _set_weather(wenv, names, conds)
    tm = wenv.get_weather()["templates"]
    refs = []
    for s, e, nm, _ in BLOCKS:
        env = _env(e - s, doc=_weather(nm)[0], offset=s)
        _give_templates(env, tm[s:e])
        refs.append((s, e, env))
    yield wenv, refs, tm
    for env in [wenv] + [r[2] for r in refs]:
        env.close()


def test_contiguous_blocks_bitwise_equal_one_handle_per_weather(torch, blocks):
    wenv, refs, tm = blocks
    alt = tm[:, 21].cpu().numpy()   # the templates' observed altitude (the condition's plus the gear's reach)
    for s, e, _, a in BLOCKS:
        assert np.all(np.abs(alt[s:e] - a) < 5.0), (s, e, alt[s:e])   # each block trimmed at its own condition
    for env in [wenv] + [r[2] for r in refs]:
        env.reset()
    done = _lockstep(torch, wenv, refs, 300)
    assert done[0] > 0, done   # auto-resets (to each env's own template) in block 0
    print(f"\n[weather blocks] done flags per block over 300 steps: {done}")


def test_weather_varying_lane_by_lane_bitwise_equals_one_env_handles(torch):
    order = ("default", "turb7_wind", "turb5")
    names = [order[i % 3] for i in range(12)]
    wenv = _env(12)
    _set_weather(wenv, names)
    tm = wenv.get_weather()["templates"]
    refs = []
    for i, nm in enumerate(names):
        env = _env(1, doc=_weather(nm)[0], offset=i)
        _give_templates(env, tm[i:i + 1])
        refs.append((i, i + 1, env))
    for env in [wenv] + [r[2] for r in refs]:
        env.reset()
    _lockstep(torch, wenv, refs, 200)
    for env in [wenv] + [r[2] for r in refs]:
        env.close()


def test_rollouts_bitwise_equal_one_handle_per_weather(torch, blocks, policy):  # noqa: F811
    wenv, refs, tm = blocks
    n, K = wenv.num_envs, 40
    head = (torch.linspace(-0.3, 0.3, 64), torch.tensor([0.1]))
    for env in [wenv] + [r[2] for r in refs]:
        env.reset()
        _set(env, policy)
        env.set_value_head(head)
    # every fifth env 20 steps from its time limit: truncations and resets to per-env templates inside the rollouts
    st, ctr = wenv.get_state()
    ctr = ctr.clone()
    ctr[::5, 0] = gc.time_up_threshold(0.01) - 20
    wenv.set_state(st, ctr)
    for s, e, env in refs:
        env.set_state(st[s:e].contiguous(), ctr[s:e].contiguous())
    g = torch.Generator().manual_seed(5)
    act = (2.0 * torch.rand((K, n, 4), generator=g) - 1.0).to("cuda:0")
    out = wenv.rollout(act)
    assert int(out[3].sum()) > 0   # truncated somewhere
    for s, e, env in refs:
        for j, (x, y) in enumerate(zip(out, env.rollout(act[:, s:e].contiguous()))):
            _same(x[:, s:e], y, f"rollout output {j}, envs [{s}, {e})")
    obs0 = out[0][-1].contiguous()
    pol = wenv.rollout_policy(K, obs0=obs0)
    for s, e, env in refs:
        for j, (x, y) in enumerate(zip(pol, env.rollout_policy(K, obs0=obs0[s:e].contiguous()))):
            _same(x[:, s:e], y, f"rollout_policy output {j}, envs [{s}, {e})")
    obs0 = pol[1][-1].contiguous()
    ac = wenv.rollout_actor_critic(K, obs0=obs0)
    assert torch.isfinite(ac["value"]).all() and torch.isfinite(ac["next_value"]).all()
    for s, e, env in refs:
        r = env.rollout_actor_critic(K, obs0=obs0[s:e].contiguous())
        for key in wenv.AC_KEYS:
            _same(ac[key][:, s:e], r[key], f"rollout_actor_critic {key}, envs [{s}, {e})")
    sw, cw = wenv.get_state()
    for s, e, env in refs:
        rs, rc = env.get_state()
        _same(sw[s:e], rs, "state after the rollouts")
        _same(cw[s:e], rc, "counters after the rollouts")


def test_population_rollout_on_a_weather_handle_is_one_policy_rollout_per_member(torch, blocks):
    """rollout_population on the weather handle (4 members of 64 envs, the last one short, the members' edges
    off the weathers' edges): member p's rows bitwise rollout_policy of the same handle from the same state
    with image p as its policy -- the rollout the tests above hold against one handle per weather."""
    wenv, _, tm = blocks
    n, K, m = wenv.num_envs, 12, 64
    P = (n + m - 1) // m
    g = torch.Generator().manual_seed(9)
    thetas = (0.1 * torch.randn((P, 5641), generator=g)).to("cuda:0")
    images = wenv.pop_pack(thetas)
    wenv.reset()
    st, ctr = wenv.get_state()
    ctr = ctr.clone()
    ctr[::5, 0] = gc.time_up_threshold(0.01) - 6   # truncations and resets to per-env templates inside the rollout
    obs0 = tm[:, 22:].contiguous()
    wenv.set_state(st, ctr)
    pop = [x.clone() for x in wenv.rollout_population(K, images, m, obs0=obs0)]
    assert int(pop[4].sum()) > 0
    for p in range(P):
        wenv.set_state(st, ctr)
        wenv.debug_policy_image(set_to=images[p].contiguous())
        one = wenv.rollout_policy(K, obs0=obs0)
        a, b = p * m, min(n, (p + 1) * m)
        for j, (x, y) in enumerate(zip(pop, one)):
            _same(x[:, a:b], y[:, a:b], f"member {p}, output {j}")
        assert p == 0 or not np.array_equal(pop[0][:, a:b].cpu().numpy(), pop[0][:, :b - a].cpu().numpy())


RUN = 32   # the launch-variant tests alternate two weathers in runs of 32 envs (by global env id)
PAIR = ("turb7_wind", "default")


def _runs(n, offset=0):
    return [PAIR[((offset + i) // RUN) % 2] for i in range(n)]


def test_weather_handle_launch_variants_bitwise_equal(torch):
    """A weather handle runs two step variants: the lone-wave one up to two waves per SIMD, the bulk one
    past it.  One batch of 2 H envs (bulk) against its two halves (lone-wave; env_offset 0 and H), sized from
    the CU count as test_gpu_variants does; 100 steps, bitwise."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nt_max = 2 * 64 * 4 * cus
    H = (3 * nt_max) // 4 + 9
    H -= H % 3
    assert H <= nt_max < 2 * H and H % 3 == 0 and H % 64
    full = _env(2 * H)
    _set_weather(full, _runs(2 * H))
    tm = full.get_weather()["templates"]
    refs = []
    for off in (0, H):
        env = _env(H, offset=off)
        _set_weather(env, _runs(H, off))
        _same(env.get_weather()["templates"], tm[off:off + H], "templates of a half")
        refs.append((off, off + H, env))
    for env in [full] + [r[2] for r in refs]:
        env.reset()
    launches0 = full.debug_launches()
    done = _lockstep(torch, full, refs, 100, every=50)
    la, lb = full.debug_launches(), refs[0][2].debug_launches()
    assert la["bulk"] - launches0["bulk"] == 100 and lb["lone_wave"] == 100 and lb["helper"] == 0, (la, lb)
    print(f"\n[weather variants] H = {H}, done flags {done}")
    for env in [full] + [r[2] for r in refs]:
        env.close()


@pytest.mark.parametrize("where", ["past_helper_range", "past_lone_wave_range"])
def test_weather_at_the_sizes_where_the_launch_changes(torch, where):
    """N just past the size up to which a plain handle runs the helper-wave kernel, and just past the lone-wave
    range: 64 sampled envs (the last two whole runs, one of each weather, in the ragged tail's neighbourhood)
    against a plain handle of their weather at the same env ids, 30 steps, bitwise."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 64 * cus + 3 if where == "past_helper_range" else 2 * 64 * 4 * cus + 65
    wenv = _env(n)
    _set_weather(wenv, _runs(n))
    tm = wenv.get_weather()["templates"]
    last = (n // RUN - 1) * RUN   # the last whole run
    refs = []
    for s in (last - RUN, last):
        nm = PAIR[(s // RUN) % 2]
        env = _env(RUN, doc=_weather(nm)[0], offset=s)
        _give_templates(env, tm[s:s + RUN])
        refs.append((s, s + RUN, env))
    assert {PAIR[(r[0] // RUN) % 2] for r in refs} == set(PAIR)
    for env in [wenv] + [r[2] for r in refs]:
        env.reset()
    _lockstep(torch, wenv, refs, 30, every=15)
    for env in [wenv] + [r[2] for r in refs]:
        env.close()


def _single_steps(torch, dt, parts):
    """parts: (batch, weather name) pairs.  Their rows interleaved row by row into one handle on the default
    airframe, each row given its weather, its recorded pre-step state and one step with its recorded eta
    (test_gpu_parity.run_single_steps).  Returns one output dict per part."""
    sizes = [len(b["state"]) for b, _ in parts]
    order = sorted((j, p) for p, m in enumerate(sizes) for j in range(m))   # row j of part p, interleaved
    src = np.array([p for _, p in order])
    row = np.array([j for j, _ in order])
    cat = lambda key, dt_: np.stack([parts[p][0][key][j] for j, p in order]).astype(dt_)   # noqa: E731
    n = len(order)
    wenv = _env(n, dt=dt, autoreset=False)
    _set_weather(wenv, [parts[p][1] for p in src])
    wenv.set_state(cat("state", np.float32), cat("counters", np.int32))
    act = torch.as_tensor(cat("actions", np.float32), device=wenv.device)
    eta = torch.as_tensor(cat("eta", np.float32), device=wenv.device)
    obs, rew, term, trunc, info = wenv.step(act, eta=eta)
    st, ctr = wenv.get_state()
    torch.cuda.synchronize()
    full = {"obs": obs.cpu().numpy().astype(np.float64), "reward": rew.cpu().numpy().astype(np.float64),
            "terminated": term.cpu().numpy(), "truncated": trunc.cpu().numpy(),
            "state": st.cpu().numpy().astype(np.float64), "counters": ctr.cpu().numpy()}
    for k in ("failed", "successed", "time_up", "success_step"):
        full[k] = info[k].cpu().numpy()
    wenv.close()
    outs = []
    for p in range(len(parts)):
        sel = np.nonzero(src == p)[0]
        assert np.array_equal(row[sel], np.arange(sizes[p]))
        outs.append({k: v[sel] for k, v in full.items()})
    return outs


def test_recorded_weathers_in_one_handle_vs_reference_dt002(torch):
    """The reference's steps recorded at turbulence 7 with a 35 ft/s wind from 120 degrees and at turbulence
    0, interleaved row by row in one handle on the default airframe: each part within contract (i) of its
    recording, with the rounding terms already stored for it (test_gpu_parity.check_vs_reference)."""
    parts = [(gc.single_step_batch(gc.load_variant(nm)[0], "hover"), nm) for nm in ("turb7_wind", "turb0")]
    assert all(b["dt"] == 0.02 for b, _ in parts)
    for (b, nm), out in zip(parts, _single_steps(torch, 0.02, parts)):
        check_vs_reference(b, out, "hover", f"var_{nm}/hover")


def test_recorded_weathers_in_one_handle_vs_reference_dt001(torch):
    """The same at dt 0.01: the recording at turbulence 5 interleaved with the default weather's recording
    (traj_dt0.01, hover task)."""
    parts = [(gc.single_step_batch(gc.load_variant("turb5")[0], "hover"), "turb5"),
             (gc.single_step_batch(gc.load("0.01"), "hover"), "default")]
    assert all(b["dt"] == 0.01 for b, _ in parts)
    outs = _single_steps(torch, 0.01, parts)
    check_vs_reference(parts[0][0], outs[0], "hover", "var_turb5/hover")
    check_vs_reference(parts[1][0], outs[1], "hover", "0.01/hover")


def test_templates_match_the_host_trim_and_reset_writes_them(torch, terrain_u16):
    """The template set_weather installs for each of the three weathers (ground altitude 100 ft) against the
    host's fp64 trim (hg_trim) of a config with that ENV block and its mean wind: contract (iii).  hg_reset
    then writes each env's own template observation."""
    from heligym_amd import _abi, config
    names = ("default", "turb7_wind", "turb5", "turb7_wind", "default")
    wenv = _env(len(names))
    r = _set_weather(wenv, names)
    assert bool((r["status"] == 0).all())
    tm = r["templates"].cpu().numpy().astype(np.float64)
    lib = _abi.load_library()
    worst = 0.0
    for i, nm in enumerate(names):
        cfg, doc = config.make_config(task="hover", dt=0.01, heli_name=_weather(nm)[0])
        hm = config.terrain_ft(terrain_u16, cfg.af.env_MAX_GR_ALT)
        tr = _abi.hg_trim_result()
        assert lib.hg_trim(ctypes.byref(cfg), hm.ctypes.data, hm.shape[0], hm.shape[1], None, ctypes.byref(tr)) == 0
        for got, ref in ((tm[i, :18], np.array(tr.state)), (tm[i, 22:], np.array(tr.obs)),
                         (tm[i, 18:22], np.array(tr.obs)[[4, 5, 6, 16]])):
            err = np.abs(got - ref) / (np.abs(ref) + 1)
            worst = max(worst, float(err.max()))
            assert np.all(err <= TRIM_REL), (i, nm, err.max())
    print(f"\n[weather templates vs host trim] worst |d|/(|x|+1) = {worst:.2e}")
    assert not np.array_equal(tm[0], tm[1]) and np.array_equal(tm[0], tm[4]) and np.array_equal(tm[1], tm[3])
    obs, _ = wenv.reset()
    _same(obs, r["templates"][:, 22:].contiguous(), "reset observations")
    st, ctr = wenv.get_state()
    for c in (0, 1) + tuple(range(4, 18)):   # (the rotor azimuths are reconstructed, not stored)
        _same(st[:, c].contiguous(), r["templates"][:, c].contiguous(), f"reset state column {c}")
    _same(st[:, 23:27].contiguous(), r["templates"][:, 18:22].contiguous(), "reset carry")
    assert int(ctr[:, :2].abs().sum()) == 0   # episode step and success count (column 2 counts the episodes)
    w = wenv.get_weather()
    for k, col in (("turb_level", 0), ("wind_dir", 1), ("wind_spd", 2)):
        np.testing.assert_array_equal(w[k], np.array([_weather(nm)[1][col] for nm in names], dtype=np.float32))
    wenv.close()


def _steps(torch, env, K):
    """K steps from a reset, with the counters of a fresh handle (the noise is keyed by the episode index too)."""
    env.reset()
    env.set_state(counters=torch.zeros((env.num_envs, 3), dtype=torch.int32, device=env.device))
    act = torch.empty((env.num_envs, 4), dtype=torch.float32, device=env.device)
    for k in range(K):
        env.random_actions(act, seed=8, step=k)
        obs, rew, term, trunc, _ = env.step(act)
    st, ctr = env.get_state()
    return obs.clone(), rew.clone(), st, ctr


def test_surface(torch, policy):  # noqa: F811
    from heligym_amd import HeliGymError, HeliVecEnv
    n = 64
    env, plain = _env(n), _env(n)
    ref = _steps(torch, plain, 50)
    own = env.get_weather()
    assert np.all(own["turb_level"] == 1) and np.all(own["wind_dir"] == 45) and np.all(own["wind_spd"] == 20)
    shared = own["templates"].clone()
    _same(shared, shared[:1].expand(n, 39).contiguous(), "the shared template in every row")
    assert env.set_weather(turb_level=6.5, wind_spd=np.linspace(0, 60, n), wind_dir=200.0) is not None
    w = env.get_weather()
    assert np.all(w["turb_level"] == 6.5) and w["wind_spd"][-1] == 60 and not bool((w["templates"] == shared).all())
    diff = _steps(torch, env, 50)
    assert not np.array_equal(diff[0].cpu().numpy(), ref[0].cpu().numpy())
    # the calls that would replace what the weather installed
    with pytest.raises(HeliGymError, match="hg_set_weather"):
        env.set_trim_cond({"gr_alt": 300.0})
    with pytest.raises(HeliGymError, match="hg_set_weather"):
        env.set_trim_conds([{"gr_alt": 300.0}] * n)
    with pytest.raises(HeliGymError, match="hg_set_weather"):
        env.set_trim_conds(None)
    # the entry points that refuse per-env weather
    _set(env, policy)
    with pytest.raises(HeliGymError, match="hg_rollout_branch does not support per-env weather"):
        env.rollout_branch(torch.zeros((3, n * 2, 4), device=env.device), 2)
    with pytest.raises(HeliGymError, match="hg_rollout_branch_policy does not support per-env weather"):
        env.rollout_branch_policy(torch.zeros((3, n * 2, 4), device=env.device), 2, obs0=env.obs)
    # out-of-range weathers name the env and change nothing
    for kw, text in ((dict(turb_level=7.5), "turb_level outside"), (dict(wind_spd=-1.0), "negative wind_spd"),
                     (dict(wind_dir=float("nan")), "non-finite")):
        with pytest.raises(HeliGymError, match=text):
            env.set_weather(**kw)
    bad = np.zeros(n, dtype=np.float32)
    bad[37] = 9.0
    with pytest.raises(HeliGymError, match="env 37"):
        env.set_weather(turb_level=bad)
    again = _steps(torch, env, 50)
    for x, y in zip(diff, again):
        _same(x, y, "the weather after refused calls")
    # no argument: the handle-wide weather and the shared template again, bitwise a fresh plain handle
    assert env.set_weather() is None
    _same(env.get_weather()["templates"], shared, "the shared template restored")
    back = _steps(torch, env, 50)
    for x, y in zip(ref, back):
        _same(x, y, "after set_weather()")
    env.set_trim_cond({"gr_alt": 100.0})   # accepted again
    env.close()
    plain.close()
    retrim = HeliVecEnv(8, task="hover", dt=0.01, reset_mode="retrim", device="cuda:0")
    with pytest.raises(HeliGymError, match="HG_RESET_TEMPLATE"):
        retrim.set_weather(turb_level=3.0)
    retrim.close()
