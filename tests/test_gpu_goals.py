"""GPU: per-env goals (HeliVecEnv.set_goals / hg_set_goals).  One handle whose envs differ in their task target
steps every env bitwise like a handle whose one target is that env's goal (same seed, global env id and reset
template); relative observations are the absolute ones minus the goal's fp32 value on the task's columns and change
nothing else; a box handle's table is goal_ref(seed, global id, episode) after every step, reset and set_state, and
each of its episodes is bitwise a table handle's that holds that episode's goals -- per step in both auto-reset
modes, in the three rollouts, in both launch variants and inside a captured graph.  Run with -m gpu.

With template resets an episode does not depend on what came before it (the noise is keyed by the env's
counters), and with the TimeLimit of 3 steps used here no goal decides when an episode ends, so the table handle
for episode e passes through the same counters and its rows inside episode e are the box handle's."""
import numpy as np
import pytest

from test_gpu_policy_rollout import _set, policy  # noqa: F401  (a fixed-seed 17-64-64-4 policy)

from heligym_amd.vector import _ptr

pytestmark = pytest.mark.gpu

SEED = 23
HOVER_COLS, FF_COLS = (13, 14, 15), (1, 15)
BOX = dict(north_loc=(-200.0, 200.0), east_loc=(-200.0, 200.0), sea_alt=(1546.0, 1746.0))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def _env(n, offset=0, task="hover", **kw):
    from heligym_amd import HeliVecEnv
    kw.setdefault("autoreset", True)
    return HeliVecEnv(n, task=task, dt=0.01, seed=SEED, env_offset=offset, device="cuda:0", **kw)


def _same(a, b, what):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype == np.float32:
        a, b = a.view(np.int32), b.view(np.int32)
    np.testing.assert_array_equal(a, b, err_msg=what)


def _actions(torch, K, n, seed=5, scale=0.2):
    """Open-loop actions around the hover trim's controls."""
    g = torch.Generator().manual_seed(seed)
    trim = torch.tensor([-0.0856, -0.3351, -0.0413, 0.1754])
    return (trim + scale * (2.0 * torch.rand((K, n, 4), generator=g) - 1.0)).clamp(-1, 1).to("cuda:0").contiguous()


def _ref(seed, gid, epi, box=BOX, task="hover"):
    from heligym_amd import goal_ref
    return goal_ref(seed, gid, epi, box, task)


def _goals_equal_ref(env, ctr, what, box=BOX, task="hover"):
    """get_goals() against goal_ref at the counters' episode, bitwise (the table holds fp32 values)."""
    g = env.get_goals()
    gid = env.cfg.env_offset + np.arange(env.num_envs)
    want = _ref(SEED, gid, ctr[:, 2].cpu().numpy(), box, task)
    for name in box:
        got = g[name]
        assert np.all(got.astype(np.float32) == got), what
        _same(got.astype(np.float32), want[name], f"{what}: {name}")


# ------------------------------------------------------------------------------------------ table mode
BLOCKS = ((0, 70), (70, 139), (139, 200))


def test_table_blocks_bitwise_equal_one_handle_per_goal(torch):
    """200 envs in three goal blocks whose edges (70, 139) fall inside waves: a goal at the template's own
    position, one 30 ft north of it, and the default far target.  max_time 0.2 s: the near goals reach `successed`
    after max_time / 4 of success steps and reset then, the far block runs to time-up."""
    from heligym_amd import _abi
    env = _env(200)
    alt0 = float(env.template()["obs"][15])
    goals = [dict(north_loc=0.0, east_loc=0.0, sea_alt=alt0), dict(north_loc=30.0, east_loc=0.0, sea_alt=alt0),
             dict(env.get_target())]
    table = {k: np.concatenate([np.full(e - s, g[k]) for (s, e), g in zip(BLOCKS, goals)]) for k in BOX}
    refs = []
    for (s, e), g in zip(BLOCKS, goals):
        r = _env(e - s, offset=s)
        r.set_target(g)
        refs.append(r)
    # per-env reset templates compose with per-env goals; the plain handles get the same rows
    env.set_trim_conds([{"gr_alt": 100.0 + (i % 7)} for i in range(200)])
    tm = env.get_weather()["templates"]
    for (s, e), r in zip(BLOCKS, refs):
        rows = tm[s:e].contiguous()
        r._check(r.lib.hg_set_reset_templates(r._h, _ptr(rows), r._stream()))
    env.set_goals(goals=table)
    got = env.get_goals()
    assert got["mode"] == "table" and got["relative"] is False and got["box"] is None
    for k in BOX:
        np.testing.assert_array_equal(got[k], table[k])
    for x in [env] + refs:
        x.set_max_time(0.2)
        x.reset()
    K = 30
    act = _actions(torch, K, 200, scale=0.05)
    first_reset = np.full(200, K)
    succ = np.zeros(200, dtype=bool)
    for k in range(K):
        obs, rew, term, trunc, info = env.step(act[k])
        bits = env.info_u8.cpu().numpy()
        succ |= (bits & _abi.HG_INFO_SUCCESSED) != 0
        first_reset = np.where(((bits & _abi.HG_INFO_RESET) != 0) & (first_reset == K), k, first_reset)
        st, ctr = env.get_state()
        for (s, e), r in zip(BLOCKS, refs):
            o, rw, te, tr, _ = r.step(act[k, s:e].contiguous())
            tag = f"step {k}, envs [{s}, {e})"
            _same(obs[s:e], o, "obs, " + tag)
            _same(rew[s:e], rw, "reward, " + tag)
            _same(term[s:e], te, "terminated, " + tag)
            _same(trunc[s:e], tr, "truncated, " + tag)
            _same(env.info_u8[s:e], r.info_u8, "info, " + tag)
            rs, rc = r.get_state()
            _same(st[s:e], rs, "state, " + tag)
            _same(ctr[s:e], rc, "counters, " + tag)
    (s0, e0), (s1, e1), (s2, e2) = BLOCKS
    assert succ[s1:e1].all() and succ[s0:e0].all() and not succ[s2:e2].any(), "the goal is the lane's own"
    assert first_reset[s1:e1].max() < first_reset[s2:e2].min() < K, (first_reset[s1:e1].max(), first_reset[s2:e2].min())
    la = env.debug_launches()
    assert la["lone_wave"] == K and la["helper"] == 0 and la["specialized"] == 0 and la["bulk"] == 0, la
    for x in [env] + refs:
        x.close()


def test_goal_varying_lane_by_lane_bitwise_equals_one_env_handles(torch):
    n, K = 67, 12
    env = _env(n)
    alt0 = float(env.template()["obs"][15])
    pair = [dict(north_loc=10.0, east_loc=-20.0, sea_alt=alt0 + 5.0), dict(north_loc=-400.0, east_loc=90.0, sea_alt=3000.0)]
    env.set_goals(goals={k: np.array([pair[i % 2][k] for i in range(n)]) for k in BOX})
    lanes = (0, 1, 31, 63, 64, 65, 66)
    refs = []
    for i in lanes:
        r = _env(1, offset=i)
        r.set_target(pair[i % 2])
        refs.append(r)
    for x in [env] + refs:
        x.reset()
    act = _actions(torch, K, n)
    for k in range(K):
        obs, rew, term, trunc, _ = env.step(act[k])
        for i, r in zip(lanes, refs):
            o, rw, te, tr, _ = r.step(act[k, i:i + 1].contiguous())
            _same(obs[i:i + 1], o, f"obs, step {k}, lane {i}")
            _same(rew[i:i + 1], rw, f"reward, step {k}, lane {i}")
            _same(term[i:i + 1], te, f"terminated, step {k}, lane {i}")
    assert not np.array_equal(rew[0:1].cpu().numpy(), rew[1:2].cpu().numpy())
    for x in [env] + refs:
        x.close()


# ------------------------------------------------------------------------------------------ relative observations
@pytest.mark.parametrize("task", ["hover", "forward_flight"])
def test_relative_observations_are_absolute_minus_the_goal(torch, task):
    n, K = 130, 10
    rng = np.random.default_rng(2)
    if task == "hover":
        goals = dict(north_loc=rng.uniform(-300, 300, n), east_loc=rng.uniform(-300, 300, n), sea_alt=rng.uniform(1500, 1800, n))
        cols, order = HOVER_COLS, ("north_loc", "east_loc", "sea_alt")
    else:
        goals = dict(sea_alt=rng.uniform(1500, 4100, n), vel=rng.uniform(40.0, 160.0, n))
        cols, order = FF_COLS, ("vel", "sea_alt")
    a, r = _env(n, task=task, max_episode_steps=4), _env(n, task=task, max_episode_steps=4)
    a.set_goals(goals=goals)
    r.set_goals(goals=goals, relative=True)
    assert r.get_goals()["relative"] is True
    g32 = {k: torch.as_tensor(v.astype(np.float32), device="cuda:0") for k, v in goals.items()}

    def shifted(x):   # [..., n, 17] absolute rows -> relative ones: a torch fp32 subtraction per column
        y = x.clone()
        for c, name in zip(cols, order):
            y[..., c] = x[..., c] - g32[name]
        return y
    oa, _ = a.reset()
    orr, _ = r.reset()
    _same(orr, shifted(oa), "reset observations")
    act = _actions(torch, K, n)
    resets = 0
    for k in range(K):
        xa = a.step(act[k])
        xr = r.step(act[k])
        _same(xr[0], shifted(xa[0]), f"obs, step {k}")
        other = [c for c in range(17) if c not in cols]
        _same(xr[0][:, other].contiguous(), xa[0][:, other].contiguous(), f"untouched columns, step {k}")
        _same(xr[1], xa[1], f"reward, step {k}")
        _same(xr[2], xa[2], f"terminated, step {k}")
        _same(xr[3], xa[3], f"truncated, step {k}")
        ia, ir = xa[4]["reset_index"], xr[4]["reset_index"]
        _same(ia, ir, f"reset_index, step {k}")
        if len(ia):
            resets += len(ia)
            fa = torch.zeros((n, 17), device="cuda:0")
            fa[ia] = xa[4]["final_obs"]
            _same(xr[4]["final_obs"], shifted(fa)[ir], f"final_obs, step {k}")
        (sa, ca), (sr, cr) = a.get_state(), r.get_state()
        _same(sr, sa, f"state, step {k}")
        _same(cr, ca, f"counters, step {k}")
    assert resets >= 2 * n   # TimeLimit 4: resets inside the run
    a.close()
    r.close()


# ------------------------------------------------------------------------------------------ box mode
def _start(torch, env):
    """reset(), then counters that differ across the envs: episode steps 0 .. 2 and episode indices 1, 6, 11."""
    env.reset()
    st, ctr = env.get_state()
    ctr = ctr.clone()
    i = torch.arange(env.num_envs, device=ctr.device)
    ctr[:, 0] = (i % 3).to(torch.int32)
    ctr[:, 2] = (1 + 5 * ((i // 3) % 3)).to(torch.int32)
    env.set_state(st, ctr)
    return ctr


def _run_steps(torch, env, act, mode, check=None):
    """K steps; per step obs, reward, flags, the dense terminal observations (NaN where no reset), and the
    episode index before and after the step."""
    n, K = env.num_envs, act.shape[0]
    out = dict(obs=[], reward=[], term=[], trunc=[], final=[], e0=[], e1=[])
    ctr = env.get_state()[1]
    for k in range(K):
        out["e0"].append(ctr[:, 2].cpu().numpy().copy())
        final = torch.full((n, 17), float("nan"), device="cuda:0")
        if mode == "same_step_compact":
            env.step_async(act[k], with_reset_info=True)
            cnt = int(env.reset_count.item())
            final[env.reset_index[:cnt].long()] = env.final_obs[:cnt]
            obs, rew, term, trunc = env.obs, env.reward, env.terminated_u8.bool(), env.truncated_u8.bool()
        else:
            obs, rew, term, trunc, info = env.step(act[k])
            if mode == "same_step":
                final[info["reset_index"]] = info["final_obs"]
        ctr = env.get_state()[1]
        out["e1"].append(ctr[:, 2].cpu().numpy().copy())
        for key, v in (("obs", obs), ("reward", rew), ("term", term), ("trunc", trunc), ("final", final)):
            out[key].append(v.cpu().numpy().copy())
        if check:
            check(k, ctr)
    return {k: np.stack(v) for k, v in out.items()}


def _hold_episode(env, e):
    """The table handle `env` given every env's goal of episode e (the drawn fp32 values)."""
    ref = _ref(SEED, env.cfg.env_offset + np.arange(env.num_envs), e)
    env.set_goals(goals={k: ref[k].astype(np.float64) for k in BOX}, relative=True)


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


@pytest.mark.parametrize("mode", ["same_step", "same_step_compact", "next_step"])
def test_box_goals_follow_the_episode_and_each_episode_is_a_table_handle(torch, mode):
    n, K = 67, 8
    kw = dict(autoreset_mode="next_step" if mode == "next_step" else "same_step")
    box = _env(n, max_episode_steps=3, **kw)
    box.set_goals(box=BOX, relative=True)
    g = box.get_goals()
    assert g["mode"] == "box" and g["relative"] is True and g["box"] == {k: tuple(v) for k, v in BOX.items()}
    _goals_equal_ref(box, box.get_state()[1], "after set_goals")
    box.reset(mask=(torch.arange(n) % 2 == 0))
    _goals_equal_ref(box, box.get_state()[1], "after reset(mask)")
    ctr0 = _start(torch, box)
    _goals_equal_ref(box, ctr0, "after set_state with counters")
    act = _actions(torch, K, n)
    b = _run_steps(torch, box, act, mode, check=lambda k, ctr: _goals_equal_ref(box, ctr, f"after step {k}"))
    assert (b["e1"][-1] > b["e0"][0]).all() and b["trunc"].sum() >= 2 * n   # resets fell inside the run
    episodes = sorted(set(np.unique(b["e0"])) | set(np.unique(b["e1"])))
    assert 3 <= len(episodes) <= 12, episodes
    tab = _env(n, max_episode_steps=3, **kw)
    for e in episodes:
        _hold_episode(tab, e)
        tab.reset(mask=(torch.arange(n) % 2 == 0))
        _start(torch, tab)
        t = _run_steps(torch, tab, act, mode)
        np.testing.assert_array_equal(t["e0"], b["e0"])   # the same counters, whatever the goals
        np.testing.assert_array_equal(t["e1"], b["e1"])
        m0, m1 = b["e0"] == e, b["e1"] == e   # [K, n]: the step ran in episode e / its observation row belongs to e
        for key in ("reward", "term", "trunc"):
            np.testing.assert_array_equal(_bits(b[key])[m0], _bits(t[key])[m0], err_msg=f"{key}, episode {e}")
        np.testing.assert_array_equal(_bits(b["obs"])[m1], _bits(t["obs"])[m1], err_msg=f"obs, episode {e}")
        if mode != "next_step":   # the terminal observation: the ending episode's frame
            np.testing.assert_array_equal(_bits(b["final"])[m0], _bits(t["final"])[m0], err_msg=f"final_obs, episode {e}")
            assert np.isfinite(b["final"][m0 & ~m1]).all() and np.isnan(b["final"][m0 & m1]).all()
    tab.close()
    # the frames differ: a reset observation is the template's minus the new goal
    tmpl = box.template()["obs"].astype(np.float32)
    k, i = np.argwhere(b["e1"] != b["e0"])[0]
    want = _ref(SEED, [i], [b["e1"][k, i]])
    for c, name in zip(HOVER_COLS, ("north_loc", "east_loc", "sea_alt")):
        assert b["obs"][k, i, c] == np.float32(tmpl[c] - want[name][0])
    box.close()


def test_rollouts_on_a_box_handle_match_table_handles_per_episode(torch, policy):  # noqa: F811
    n, K = 67, 8
    head = (torch.linspace(-0.3, 0.3, 64), torch.tensor([0.1]))
    act = _actions(torch, K, n)

    def run(env):
        _set(env, policy)
        env.set_value_head(head)
        obs0, _ = env.reset()
        obs0 = obs0.clone()
        _start(torch, env)
        e0 = env.get_state()[1][:, 2].cpu().numpy().copy()
        r = {}
        ro = env.rollout(act)
        r["rollout"] = dict(obs=ro[0], reward=ro[1], term=ro[2], trunc=ro[3])
        cur = ro[0][-1].contiguous()
        rp = env.rollout_policy(K, obs0=cur)
        r["policy"] = dict(actions=rp[0], obs=rp[1], reward=rp[2], term=rp[3], trunc=rp[4])
        cur = rp[1][-1].contiguous()
        ac = env.rollout_actor_critic(K, obs0=cur)
        r["ac"] = dict(actions=ac["actions"], obs=ac["obs"], reward=ac["reward"], term=ac["terminated"],
                       trunc=ac["truncated"], logp=ac["logp"], value=ac["value"], next_value=ac["next_value"])
        e_end = env.get_state()[1][:, 2].cpu().numpy().copy()
        return {k: {kk: vv.cpu().numpy().copy() for kk, vv in v.items()} for k, v in r.items()}, e0, e_end, obs0

    box = _env(n, max_episode_steps=3)
    box.set_goals(box=BOX, relative=True)
    b, e_start, e_end, _ = run(box)
    _goals_equal_ref(box, box.get_state()[1], "after the rollouts")
    # the episode of every row: the index advances at each truncation (TimeLimit 3, same-step reset)
    epis = {}
    e = e_start.copy()
    for name in ("rollout", "policy", "ac"):
        before, after = np.zeros((K, n), np.int64), np.zeros((K, n), np.int64)
        for k in range(K):
            before[k] = e
            e = e + (b[name]["trunc"][k] | b[name]["term"][k]).astype(np.int64)
            after[k] = e
        epis[name] = (before, after)
        assert b[name]["trunc"].sum() >= 2 * n and not b[name]["term"].any()
    np.testing.assert_array_equal(e, e_end)
    # (next_value included: at a truncation it is the value of the terminal observation in the ending episode's
    # frame, which the table handle of that episode computes from its own rows; the test below pins its value)
    tab = _env(n, max_episode_steps=3)
    for ep in sorted(set(np.unique(np.stack([x for pair in epis.values() for x in pair])))):
        _hold_episode(tab, ep)
        t, _, _, _ = run(tab)
        for name in ("rollout", "policy", "ac"):
            m0, m1 = epis[name][0] == ep, epis[name][1] == ep
            for key in b[name]:
                m = m1 if key == "obs" else m0
                np.testing.assert_array_equal(_bits(b[name][key])[m], _bits(t[name][key])[m],
                                              err_msg=f"{name} {key}, episode {ep}")
    tab.close()
    box.close()


def test_next_value_at_a_truncation_is_the_value_of_the_old_frames_terminal_observation(torch, policy):  # noqa: F811
    """rollout_actor_critic(1) from a state one step short of the TimeLimit: every env is truncated and reset in
    that step, and next_value must be policy_evaluate's value of the terminal observation in the ending episode's
    frame -- which a table handle without auto-reset, holding that episode's goals, exposes."""
    n = 67
    head = (torch.linspace(-0.3, 0.3, 64), torch.tensor([0.1]))
    box = _env(n, max_episode_steps=3)
    box.set_goals(box=BOX, relative=True)
    obs0, _ = box.reset()
    st, ctr = box.get_state()
    ctr = ctr.clone()
    ctr[:, 0] = 2
    box.set_state(st, ctr)
    old = _ref(SEED, np.arange(n), ctr[:, 2].cpu().numpy())
    tab = _env(n, max_episode_steps=3, autoreset=False)
    tab.set_goals(goals={k: old[k].astype(np.float64) for k in BOX}, relative=True)
    tab.reset()
    tab.set_state(st, ctr)
    for env in (box, tab):
        _set(env, policy)
        env.set_value_head(head)
    ac = box.rollout_actor_critic(1, obs0=obs0.clone())
    assert bool(ac["truncated"].all()) and not bool(ac["terminated"].any())
    term_obs = tab.step(ac["actions"][0].contiguous())[0].clone()   # the same step, no reset: the terminal rows
    assert bool(tab.truncated_u8.all())
    _same(ac["next_value"][0], tab.policy_evaluate(term_obs)[2], "next_value at a truncation")
    new = _ref(SEED, np.arange(n), ctr[:, 2].cpu().numpy() + 1)
    tmpl = box.template()["obs"].astype(np.float32)
    assert np.all(ac["obs"][0][:, 15].cpu().numpy() == tmpl[15] - new["sea_alt"])   # the row itself: the new frame
    assert not np.array_equal(ac["next_value"][0].cpu().numpy(), box.policy_evaluate(ac["obs"][0].contiguous())[2].cpu().numpy())
    box.close()
    tab.close()


# ------------------------------------------------------------------------------------------ launch variants
def _whole_against_parts(torch, n, cuts, K):
    """One box / relative handle of n envs against handles of its parts (env_offset at each cut), K steps under a
    TimeLimit of 3 from staggered counters: bitwise, the goal tables included."""
    edges = list(zip([0] + cuts, cuts + [n]))
    full = _env(n, max_episode_steps=3)
    parts = [_env(e - s, offset=s, max_episode_steps=3) for s, e in edges]
    for env in [full] + parts:
        env.set_goals(box=BOX, relative=True)
        env.reset()
    st, ctr = full.get_state()
    ctr = ctr.clone()
    ctr[:, 0] = (torch.arange(n, device=ctr.device) % 3).to(torch.int32)
    full.set_state(st, ctr)
    for (s, e), env in zip(edges, parts):
        env.set_state(st[s:e].contiguous(), ctr[s:e].contiguous())
    act = _actions(torch, K, n)
    for k in range(K):
        obs, rew, term, trunc, _ = full.step(act[k])
        outs = [env.step(act[k, s:e].contiguous()) for (s, e), env in zip(edges, parts)]
        if k % 4 == 3 or k == K - 1:
            stf, ctf = full.get_state()
            gf = full.get_goals()
            for (s, e), env, (o, r, te, tr, _) in zip(edges, parts, outs):
                tag = f"step {k}, envs [{s}, {e})"
                _same(obs[s:e], o, "obs, " + tag)
                _same(rew[s:e], r, "reward, " + tag)
                _same(term[s:e], te, "terminated, " + tag)
                _same(trunc[s:e], tr, "truncated, " + tag)
                rs, rc = env.get_state()
                _same(stf[s:e], rs, "state, " + tag)
                _same(ctf[s:e], rc, "counters, " + tag)
                gp = env.get_goals()
                for name in BOX:
                    np.testing.assert_array_equal(gf[name][s:e], gp[name], err_msg=f"goal {name}, " + tag)
    _goals_equal_ref(full, full.get_state()[1], "the whole handle's table")
    assert int(full.get_state()[1][:, 2].min()) >= 1 + (K - 2) // 3
    la = [env.debug_launches() for env in [full] + parts]
    for env in [full] + parts:
        env.close()
    return la


def test_goal_handle_launch_variants_bitwise_equal(torch):
    """A goal handle runs two step variants: the lone-wave one up to two waves per SIMD, the bulk one past it.
    One batch of 2 H envs (bulk) against its two halves (lone-wave; env_offset 0 and H), sized from the CU count."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nt_max = 2 * 64 * 4 * cus
    H = (3 * nt_max) // 4 + 9
    H -= H % 3
    assert H <= nt_max < 2 * H and H % 64
    K = 12
    la = _whole_against_parts(torch, 2 * H, [H], K)
    assert la[0]["bulk"] == K and la[0]["lone_wave"] == 0 and la[1]["lone_wave"] == K and la[1]["bulk"] == 0, la
    assert all(x["helper"] == 0 and x["specialized"] == 0 for x in la), la


def test_goal_handle_with_a_ragged_last_tile(torch):
    _whole_against_parts(torch, 130, [64], 9)


# ------------------------------------------------------------------------------------------ capture
def test_captured_steps_replay_bitwise_and_keep_the_table(torch):
    n, K = 132, 6   # (a ragged last tile; n % 4 == 0 keeps every step's [n,17] row block 16-byte aligned)
    a, b = _env(n, max_episode_steps=3), _env(n, max_episode_steps=3)
    for env in (a, b):
        env.set_goals(box=BOX, relative=True)
        env.reset()
    act = _actions(torch, K, n)
    rows_a = torch.zeros((K, n, 17), device="cuda:0")
    rows_b = torch.zeros((K, n, 17), device="cuda:0")
    st0, ctr0 = a.get_state()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # (warm-up on the capture's stream, then back to the start)
        a.step_async(act[0], with_reset_info=False, obs_out=rows_a[0])
        a.set_state(st0, ctr0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):   # one chain of six step launches
        for k in range(K):
            a.step_async(act[k], with_reset_info=False, obs_out=rows_a[k])
    for rep in range(2):
        rows_a.zero_()
        g.replay()
        for k in range(K):
            b.step_async(act[k], with_reset_info=False, obs_out=rows_b[k])
        torch.cuda.synchronize()
        _same(rows_a, rows_b, f"observations, replay {rep}")
        _same(a.reward, b.reward, f"reward, replay {rep}")
        _same(a.truncated_u8, b.truncated_u8, f"truncated, replay {rep}")
        (sa, ca), (sb, cb) = a.get_state(), b.get_state()
        _same(sa, sb, f"state, replay {rep}")
        _same(ca, cb, f"counters, replay {rep}")
        assert int(ca[:, 2].min()) == 1 + 2 * (rep + 1)   # two resets per replay
        _goals_equal_ref(a, ca, f"the table after replay {rep}")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------ surface
def _steps(torch, env, K):
    env.reset()
    env.set_state(counters=torch.zeros((env.num_envs, 3), dtype=torch.int32, device=env.device))
    act = _actions(torch, K, env.num_envs, seed=11)
    for k in range(K):
        obs, rew, term, trunc, _ = env.step(act[k])
    st, ctr = env.get_state()
    return obs.clone(), rew.clone(), st, ctr


def test_surface(torch, policy):  # noqa: F811
    from heligym_amd import HeliGymError, HeliVecEnv
    n = 64
    env, plain = _env(n), _env(n)
    ref = _steps(torch, plain, 20)
    own = env.get_goals()
    assert own["mode"] == "off" and own["box"] is None and not own["relative"]
    assert np.all(own["sea_alt"] == 4000.0) and np.all(own["north_loc"] == 0.0)
    env.set_goals(goals=dict(sea_alt=np.linspace(1600.0, 1700.0, n)), relative=True)
    diff = _steps(torch, env, 20)
    assert not np.array_equal(diff[1].cpu().numpy(), ref[1].cpu().numpy())
    with pytest.raises(HeliGymError, match="pass goals to hg_set_goals"):
        env.set_target(dict(sea_alt=1234.0))
    assert env.get_target()["sea_alt"] == 4000.0
    with pytest.raises(HeliGymError, match="hg_set_weather: per-env goals are set"):
        env.set_weather(turb_level=3.0)
    from heligym_amd import sample_fleet
    with pytest.raises(HeliGymError, match="hg_set_fleet: per-env goals are set"):
        env.set_fleet(sample_fleet(1), envs_per_class=64)
    _set(env, policy)
    with pytest.raises(HeliGymError, match="hg_rollout_branch does not support per-env goals"):
        env.rollout_branch(torch.zeros((3, n * 2, 4), device=env.device), 2)
    with pytest.raises(HeliGymError, match="hg_rollout_branch_policy does not support per-env goals"):
        env.rollout_branch_policy(torch.zeros((3, n * 2, 4), device=env.device), 2, obs0=env.obs)
    with pytest.raises(HeliGymError, match="hg_rollout_pop does not support per-env goals"):
        env.rollout_population(3, env.pop_pack(torch.zeros((1, 5641), device=env.device)), 64)
    bad = np.full(n, 1650.0)
    bad[37] = np.inf
    with pytest.raises((HeliGymError, ValueError), match="non-finite"):
        env.set_goals(goals=dict(sea_alt=bad))
    again = _steps(torch, env, 20)
    for x, y in zip(diff, again):
        _same(x, y, "the goals after refused calls")
    la = env.debug_launches()
    assert la["lone_wave"] == 40 and la["helper"] == 0 and la["bulk"] == 0, la
    env.set_goals()   # reverts: bitwise a fresh plain handle
    assert env.get_goals()["mode"] == "off"
    back = _steps(torch, env, 20)
    for x, y in zip(ref, back):
        _same(x, y, "after set_goals()")
    assert env.debug_launches()["helper"] == 20   # the plain handle's small-batch kernel again
    env.set_target(dict(sea_alt=4000.0))   # accepted again
    env.close()
    plain.close()
    # refusals that need another handle
    w = _env(n)
    w.set_weather(turb_level=2.0)
    with pytest.raises(HeliGymError, match="hg_set_goals: per-env weather is set"):
        w.set_goals(goals=dict(sea_alt=1700.0))
    w.set_weather()
    w.set_fleet(sample_fleet(1), envs_per_class=64)
    with pytest.raises(HeliGymError, match="hg_set_goals: a fleet is set"):
        w.set_goals(box=BOX)
    w.close()
    retrim = HeliVecEnv(8, task="hover", dt=0.01, reset_mode="retrim", device="cuda:0")
    with pytest.raises(HeliGymError, match="HG_RESET_TEMPLATE"):
        retrim.set_goals(goals=dict(sea_alt=1700.0))
    retrim.close()
    heli = HeliVecEnv(8, task="heli", dt=0.01, device="cuda:0")
    with pytest.raises((HeliGymError, ValueError), match="no target"):
        heli.set_goals(goals=dict(sea_alt=1700.0))
    heli.close()
    ff = _env(8, task="forward_flight")
    with pytest.raises((HeliGymError, ValueError), match="vel <= 0"):
        ff.set_goals(box=dict(vel=(0.0, 50.0)))
    with pytest.raises(HeliGymError, match="vel <= 0"):
        ff.set_goals(goals=dict(vel=-3.0))
    ff.set_goals(box=dict(vel=(60.0, 140.0), sea_alt=(3000.0, 4100.0)))
    _goals_equal_ref(ff, ff.get_state()[1], "forward flight", box=dict(vel=(60.0, 140.0), sea_alt=(3000.0, 4100.0)),
                     task="forward_flight")
    ff.close()
