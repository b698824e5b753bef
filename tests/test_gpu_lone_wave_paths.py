"""GPU: the lone-wave step's reworked paths, every comparison bitwise.

 * Same-step resets (the lone-wave kernels read the reset template from the wave's LDS copy under the resetting
   lanes' mask): resetting lanes against the template, their neighbours against a twin env nothing resets in.
 * The attitude classes of att_step (short series, long series, full sincos, a NaN rate) mixed inside one wave
   against the same lanes stepped in waves that hold one class only.
 * In-kernel noise against the injected-noise kernel fed the exported eta, one step.
Run with -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PATTERNS = ["none", "lane0", "lane63", "every_second", "all64", "ragged_last"]
APIS = ["step", "async", "async_reset_info", "graph"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def _env(torch, n, **kw):
    from heligym_amd import HeliVecEnv
    return HeliVecEnv(n, task="hover", dt=0.01, device="cuda:0", **kw)


def _lone_n(torch):
    """An env count past the helper kernel's range (two tiles per CU) and inside the lone-wave step's, ragged."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * 4 * cus // 2 + 129
    assert 64 * 4 * cus // 2 < n <= 2 * 64 * 4 * cus and n % 64
    return n


def _crash_mask(pattern, n):
    lane = np.arange(n) % 64
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "lane0":
        return lane == 0
    if pattern == "lane63":
        return lane == 63
    if pattern == "every_second":
        return lane % 2 == 1
    if pattern == "all64":     # every lane of every second tile (and of the first)
        return (np.arange(n) // 64) % 2 == 0
    m = np.zeros(n, bool)      # the last active lane of the last (ragged, unless n % 64 == 0) tile
    m[n - 1] = True
    return m


def _bits(x):
    x = x.cpu().numpy()
    return x.view(np.int32) if x.dtype == np.float32 else x


def _one_step(torch, env, api, act, graph):
    """One step of `env` through `api`; returns (obs, reward, terminated, truncated, info bits, state, counters)."""
    if api == "step":
        env.step(act)
    elif api == "async":
        env.step_async(act, with_reset_info=False)
    elif api == "async_reset_info":
        env.step_async(act, with_reset_info=True)
    else:
        graph[0].replay()
    torch.cuda.synchronize()
    s, c = env.get_state()
    info = graph[1] if api == "graph" else env.info_u8   # (the captured step's info buffer of the env's two)
    return (_bits(env.obs), _bits(env.reward), _bits(env._term_b), _bits(env._trunc_b), _bits(info), _bits(s), _bits(c))


@pytest.mark.parametrize("specialised", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("size", [64, 65, 4097, "lone"])
def test_resets_take_the_template_and_leave_their_neighbours_alone(torch, size, specialised):
    """N = 64 (one full tile), 65 (a ragged tile), 4 097 (the helper kernel, many blocks) and a ragged count in
    the one-wave lone kernel's range.  For each reset pattern the chosen lanes are put beyond the map edge (they
    fail in this step) and the env is stepped once through step(), step_async() with and without the compacted
    reset info, and a graph replay of step_async().  Resetting lanes: state, wind state, carry and observation
    bitwise a freshly reset env's row (the template), counters (0, 0, episode + 1), terminated and the FAILED and
    RESET info bits.  Every other lane: bitwise the same lane of a twin env of the same state, seed and ids in
    which nothing resets."""
    from heligym_amd import _abi
    n = _lone_n(torch) if size == "lone" else size
    env, twin = _env(torch, n, autoreset=True, seed=11), _env(torch, n, autoreset=True, seed=11)
    assert env.set_specialized(specialised) == specialised and twin.set_specialized(specialised) == specialised
    env.reset()
    twin.reset()
    st0, c0 = env.get_state()
    st0, c0 = st0.cpu().numpy(), c0.cpu().numpy()
    tpl = env.template()
    # a freshly reset row is the template: heli state | zero wind state | carry = obs[4, 5, 6, 16]
    fresh = st0[0].copy()
    np.testing.assert_array_equal(st0, np.tile(fresh, (n, 1)))
    np.testing.assert_array_equal(fresh[:18], tpl["state"].astype(np.float32))
    np.testing.assert_array_equal(fresh[18:23], 0.0)
    tobs = tpl["obs"].astype(np.float32)
    np.testing.assert_array_equal(fresh[23:27], tobs[[4, 5, 6, 16]])
    # a state off the template for everyone (so that a template value in a non-resetting lane would show)
    rng = np.random.default_rng(3)
    base = st0.copy()
    base[:, 6:9] += rng.uniform(-3, 3, (n, 3)).astype(np.float32)      # u, v, w
    base[:, 9:12] += rng.uniform(-0.2, 0.2, (n, 3)).astype(np.float32)  # p, q, r
    base[:, 17] -= 50.0
    base[:, 18:23] = rng.uniform(-1, 1, (n, 5)).astype(np.float32)
    ctr = c0.copy()
    ctr[:, 0] = 7
    ctr[:, 2] = 3
    act = torch.zeros((n, 4), dtype=torch.float32, device=env.device)
    twin.set_state(base, ctr)
    ref = _one_step(torch, twin, "step", act, None)
    assert not ref[2].any() and not ref[3].any() and np.all(ref[6][:, 0] == 8)
    # the graph: one captured step_async (warmed on the capture's side stream first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step_async(act, with_reset_info=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.step_async(act, with_reset_info=False)
    graph = (graph, env.info_u8)
    for pattern in PATTERNS:
        crash = _crash_mask(pattern, n)
        st = base.copy()
        st[crash, 15] = 4000.0   # |x| past the map's half width: failed at once
        for api in APIS:
            env.set_state(st, ctr)
            obs, rew, term, trunc, info, s2, c2 = _one_step(torch, env, api, act, graph)
            tag = (size, specialised, pattern, api)
            np.testing.assert_array_equal(term.astype(bool), crash, err_msg=str(tag))
            assert not trunc.any(), tag
            np.testing.assert_array_equal((info & _abi.HG_INFO_RESET) != 0, crash, err_msg=str(tag))
            np.testing.assert_array_equal((info & _abi.HG_INFO_FAILED) != 0, crash, err_msg=str(tag))
            k = int(crash.sum())
            np.testing.assert_array_equal(s2[crash], np.tile(fresh.view(np.int32), (k, 1)), err_msg=str(tag))
            np.testing.assert_array_equal(obs[crash], np.tile(tobs.view(np.int32), (k, 1)), err_msg=str(tag))
            np.testing.assert_array_equal(c2[crash], np.tile(np.array([0, 0, 4], np.int32), (k, 1)), err_msg=str(tag))
            keep = ~crash
            for got, want, name in zip((obs, rew, term, trunc, info, s2, c2), ref,
                                       ("obs", "reward", "terminated", "truncated", "info", "state", "counters")):
                np.testing.assert_array_equal(got[keep], want[keep], err_msg=f"{tag} {name}")
    env.close()
    twin.close()


RATES = [1.0, 12.0, 40.0, float("nan")]   # rad/s: stage increments of 0.01, 0.12, 0.4 rad at dt 0.01, and NaN


@pytest.mark.parametrize("size", [256, "lone"])
def test_attitude_classes_mixed_in_one_wave_equal_one_class_per_wave(torch, size):
    """Body rates put the lanes of every tile in each class of att_step -- increments under 0.05 rad, between 0.05
    and 0.25, past 0.25, and a NaN rate -- lane l of tile k in class (l + k) % 4.  One step; every lane bitwise
    the same lane of an env whose lanes all have that lane's class (same state otherwise, same seed and ids):
    what a lane computes does not depend on the branches its wave takes for its neighbours."""
    n = _lone_n(torch) if size == "lone" else size
    idx = np.arange(n)
    cls = (idx % 64 + idx // 64) % 4
    envs = [_env(torch, n, autoreset=False, seed=5) for _ in range(5)]
    for e in envs:
        e.reset()
    st0, c0 = envs[0].get_state()
    st0, c0 = st0.cpu().numpy(), c0.cpu().numpy()
    st0[:, 17] -= 500.0   # off the ground
    act = torch.zeros((n, 4), dtype=torch.float32, device=envs[0].device)

    def run(env, classes):
        st = st0.copy()
        for c, rate in enumerate(RATES):
            st[classes == c, 9] = rate            # p
            st[classes == c, 11] = -0.5 * rate    # r
        env.set_state(st, c0)
        obs, rew, term, trunc, _ = env.step(act)
        s, c = env.get_state()
        return _bits(obs), _bits(rew), _bits(s)

    mixed = run(envs[0], cls)
    seen = 0
    for c in range(4):
        pure = run(envs[1 + c], np.full(n, c))
        rows = cls == c
        seen += int(rows.sum())
        for got, want, name in zip(mixed, pure, ("obs", "reward", "state")):
            np.testing.assert_array_equal(got[rows], want[rows], err_msg=f"class {c} {name}")
    assert seen == n
    # the classes did differ: the NaN lanes' attitude is NaN, the others' finite and distinct per class
    s = mixed[2].view(np.float32)
    assert np.all(np.isnan(s[cls == 3, 12])) and np.all(np.isfinite(s[cls != 3, 12]))
    assert len({float(s[cls == c, 12][0]) for c in range(3)}) == 3
    for e in envs:
        e.close()


@pytest.mark.parametrize("n", [4096, 65536])
def test_in_kernel_noise_equals_injected_one_step(torch, n):
    """tests/test_gpu_noise.py's comparison at one step: the population stepped with in-kernel noise (the helper
    kernel at 4 096 envs, the lone-wave kernel at 65 536) and a twin stepped by the injected-noise kernel fed the
    exported eta -- observations, rewards, flags, info bits and the state bitwise equal."""
    a, b = _env(torch, n, autoreset=True, seed=9), _env(torch, n, autoreset=True, seed=9)
    a.reset()
    b.reset()
    act = torch.empty((n, 4), dtype=torch.float32, device=a.device)
    eta = torch.empty((n, 3), dtype=torch.float32, device=a.device)
    a.random_actions(act, seed=21, step=0)
    a.debug_eta(eta)
    assert float(eta.abs().max()) > 0
    oa, ra, ta, ua, _ = a.step(act)
    ia = a.info_u8.clone()
    ob, rb, tb, ub, _ = b.step(act, eta=eta)
    assert torch.equal(oa.view(torch.int32), ob.view(torch.int32))
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert torch.equal(ta, tb) and torch.equal(ua, ub) and torch.equal(ia, b.info_u8)
    sa, ca = a.get_state()
    sb, cb = b.get_state()
    assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)) and torch.equal(ca, cb)
    a.close()
    b.close()
