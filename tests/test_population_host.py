"""CPU-side checks of the population / evolution-strategies surface (hg_policy_image_floats, hg_pop_pack,
hg_rollout_pop, hg_es_perturb, hg_es_noise, hg_pop_fitness, hg_es_workspace_bytes, hg_es_grad and the two
image diagnostics): the symbols are exported and declared with the header's argument counts; each call
refuses a NULL env and every out-of-range argument the header names (the arguments that need no handle are
checked before it, so a NULL env reaches them; the member range needs the env's N and is checked through
HeliVecEnv's wrappers, which refuse the same things with ValueError before the library is called); and the
NumPy restatements in heligym_amd.evolution do what the header says.  No device calls."""
import numpy as np
import pytest
import torch

from test_branch_host import _bare_env
from test_policy_host import header_arg_counts

import heligym_amd
from heligym_amd import _abi, es_grad_ref, es_utilities_ref, pop_fitness_ref

NEW = {"hg_policy_image_floats": 0, "hg_pop_pack": 8, "hg_rollout_pop": 13, "hg_es_perturb": 13, "hg_es_noise": 7,
       "hg_pop_fitness": 13, "hg_es_workspace_bytes": 1, "hg_es_grad": 11, "hg_debug_get_policy_image": 3,
       "hg_debug_set_policy_image": 3}
A16, A16B, A16C, A16D = 0x10000, 0x20000, 0x30000, 0x40000   # stand-ins for aligned device pointers: never dereferenced
ODD = 0x10004                                                # 4-byte but not 16-byte aligned


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _refused(lib, rc, text):
    assert rc == -1, (rc, text)
    assert text.encode() in lib.hg_last_error(), (lib.hg_last_error(), text)


def test_population_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    assert counts["hg_rollout_policy"] == 11   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == n, name
    assert lib.hg_abi_version() == 3   # purely additive
    assert lib.hg_policy_image_floats() == 7552 == _abi.HG_POLICY_IMAGE_FLOATS
    for name in ("ES", "es_utilities_ref", "es_grad_ref", "pop_fitness_ref"):
        assert name in heligym_amd.__all__ and hasattr(heligym_amd, name)


def _pack(lib, theta=A16, P=4, images=A16B, mean=None):
    return lib.hg_pop_pack(None, theta, P, 1, mean, None, images, None)


def _rollout(lib, images=A16, P=4, epm=64, nsteps=3, act=A16B, obs=A16C):
    return lib.hg_rollout_pop(None, images, P, epm, A16D, nsteps, act, obs, A16D, A16D, A16D, None, None)


def _perturb(lib, P=4, sigma=0.1, images=A16B, theta=A16, gen_dev=None, member=None):
    return lib.hg_es_perturb(None, theta, P, sigma, 1, 0, gen_dev, 1, None, None, images, member, None)


def _noise(lib, pair=0, out=A16):
    return lib.hg_es_noise(None, 1, 0, None, pair, out, None)


def _fitness(lib, K=3, P=4, epm=64, mode=0, alive=None, term=A16, sums=A16B, reward=A16):
    return lib.hg_pop_fitness(None, reward, term, term, K, P, epm, mode, 0, alive, sums, A16C, None)


def _grad(lib, P=4, sigma=0.1, ws=A16C, fitness=A16, grad=A16B):
    return lib.hg_es_grad(None, fitness, P, sigma, 1, 0, None, grad, None, ws, None)


def test_every_call_refuses_a_null_env(lib):
    for call in (_pack, _rollout, _perturb, _noise, _grad):
        _refused(lib, call(lib), "env is NULL")
    _refused(lib, _fitness(lib), "env is NULL")
    _refused(lib, _fitness(lib, mode=1, alive=A16D), "env is NULL")
    _refused(lib, lib.hg_debug_get_policy_image(None, A16, None), "env is NULL")
    _refused(lib, lib.hg_debug_set_policy_image(None, A16, None), "env is NULL")


def test_population_sizes(lib):
    for P in (0, -2, 65537):
        _refused(lib, _pack(lib, P=P), "P must be in 1 .. 65536")
        _refused(lib, _rollout(lib, P=P), "P must be in 1 .. 65536")
        _refused(lib, _fitness(lib, P=P), "P must be in 1 .. 65536")
    for P in (0, 1, 3, 5, 65537, 65538):   # odd P, and the range
        _refused(lib, _perturb(lib, P=P), "P must be even, in 2 .. 65536")
    _refused(lib, _perturb(lib, P=65536), "env is NULL")
    # hg_es_grad's cap, stated in the header: 16384
    for P in (0, 1, 3, 4095, 16385, 16386, 65536):
        _refused(lib, _grad(lib, P=P), "P must be even, in 2 .. 16384")
        assert lib.hg_es_workspace_bytes(P) == -1, P
    _refused(lib, _grad(lib, P=16384), "env is NULL")
    _refused(lib, _grad(lib, P=4096), "env is NULL")
    assert _abi.HG_ES_MAX_POP == 16384
    for pair in (-1, 32768):
        _refused(lib, _noise(lib, pair=pair), "pair must be in 0 .. 32767")


def test_workspace_bytes(lib):
    # u [P rounded up to 4] fp32, then one [5572] fp32 partial per chunk of 16 pairs
    for P, chunks in ((2, 1), (6, 1), (32, 1), (34, 2), (1024, 32), (16384, 512)):
        b = lib.hg_es_workspace_bytes(P)
        assert b == 4 * (((P + 3) // 4) * 4 + chunks * 5572), (P, b)
        assert b % 16 == 0


def test_sigma(lib):
    for sigma in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        _refused(lib, _perturb(lib, sigma=sigma), "sigma must be finite and > 0")
        _refused(lib, _grad(lib, sigma=sigma), "sigma must be finite and > 0")


def test_envs_per_member(lib):
    for epm in (0, -64, 1, 63, 65, 96, 100):
        _refused(lib, _rollout(lib, epm=epm), "envs_per_member must be a positive multiple of 64")
        _refused(lib, _fitness(lib, epm=epm), "envs_per_member must be a positive multiple of 64")


def test_pointers_and_alignment(lib):
    _refused(lib, _pack(lib, images=ODD), "images must be 16-byte aligned")
    _refused(lib, _pack(lib, theta=0x10002), "images must be 16-byte aligned, the other pointers 4-byte")
    _refused(lib, _pack(lib, mean=0x10001), "4-byte")
    _refused(lib, _pack(lib, images=None), "must be device pointers")
    _refused(lib, _rollout(lib, images=ODD), "images, actions_out and obs must be 16-byte aligned")
    _refused(lib, _rollout(lib, act=ODD), "16-byte aligned")
    _refused(lib, _rollout(lib, obs=ODD), "16-byte aligned")
    _refused(lib, _rollout(lib, images=None), "must be device pointers")
    _refused(lib, _rollout(lib, nsteps=0), "nsteps must be >= 1")
    _refused(lib, _perturb(lib, images=ODD), "images must be 16-byte aligned")
    _refused(lib, _perturb(lib, member=0x10002), "4-byte")
    _refused(lib, _perturb(lib, gen_dev=0x10002), "4-byte")
    _refused(lib, _perturb(lib, theta=None), "must be device pointers")
    _refused(lib, _noise(lib, out=None), "must be a device pointer")
    _refused(lib, _noise(lib, out=0x10002), "4-byte aligned")
    _refused(lib, _grad(lib, ws=ODD), "workspace must be 16-byte aligned")
    _refused(lib, _grad(lib, ws=None), "must be device pointers")
    _refused(lib, _grad(lib, grad=0x10002), "4-byte")
    _refused(lib, _fitness(lib, sums=ODD), "sum 8-byte")
    _refused(lib, _fitness(lib, reward=None), "must be device pointers")
    _refused(lib, _fitness(lib, K=0), "K must be >= 1")


def test_fitness_modes(lib):
    _refused(lib, _fitness(lib, mode=2), "unknown mode")
    _refused(lib, _fitness(lib, mode=-1), "unknown mode")
    _refused(lib, _fitness(lib, mode=1, alive=None), "needs terminated, truncated and alive")   # FIRST_EPISODE without alive
    _refused(lib, _fitness(lib, mode=1, alive=A16D, term=None), "needs terminated, truncated and alive")
    _refused(lib, _fitness(lib, mode=0, term=None), "env is NULL")   # the window does not read the flags


def test_wrappers_validate_first():
    """HeliVecEnv's wrappers refuse the same things with ValueError before the library is reached -- N outside
    the member range included, which the library can only check with a handle."""
    n = 200
    env = _bare_env(n)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)   # noqa: E731
    im4 = z(4, 7552)
    # N = 200 needs (P - 1) * m < 200 <= P * m
    for P, m in ((3, 64), (5, 64), (2, 64), (1, 128), (4, 128), (8, 64)):
        with pytest.raises(ValueError, match="do not cover"):
            env.rollout_population(3, z(P, 7552), m)
        with pytest.raises(ValueError, match="do not cover"):
            env.pop_fitness(z(3, n), None, None, P, m, z(P, dtype=torch.float64))
    for m in (0, 63, 65, 100, -64):
        with pytest.raises(ValueError, match="multiple of 64"):
            env.rollout_population(3, im4, m)
    with pytest.raises(AssertionError, match="hg_rollout_pop"):   # valid arguments do reach the library
        env.rollout_population(3, im4, 64, obs0=z(n, 17))
    with pytest.raises(AssertionError, match="hg_rollout_pop"):
        env.rollout_population(3, z(2, 7552), 128, obs0=z(n, 17))
    for bad in (z(4, 7551), z(4, 7552, dtype=torch.float64), z(7552), z(4, 2 * 7552)[:, ::2], np.zeros((4, 7552))):
        with pytest.raises(ValueError):
            env.rollout_population(3, bad, 64, obs0=z(n, 17))
    th = z(5641)
    for P in (0, 1, 3, 65538):
        with pytest.raises(ValueError, match="even"):
            env.es_perturb(th, P, 0.1, 0)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            env.es_perturb(th, 4, s, 0)
        with pytest.raises(ValueError, match="sigma"):
            env.es_grad(th, z(4), s, 0)
    with pytest.raises(ValueError, match="gen_dev"):
        env.es_perturb(th, 4, 0.1, 0, gen_dev=z(1))
    with pytest.raises(ValueError, match="member_theta"):
        env.es_perturb(th, 4, 0.1, 0, member_theta=z(4, 5640))
    with pytest.raises(AssertionError, match="hg_es_perturb"):
        env.es_perturb(th, 4, 0.1, 0, gen_dev=z(1, dtype=torch.int32), member_theta=z(4, 5641))
    for P in (3, 16386):   # odd; past the cap
        with pytest.raises(ValueError, match="even"):
            env.es_grad(th, z(P), 0.1, 0)
    with pytest.raises(ValueError, match="first_episode"):
        env.pop_fitness(z(3, n), z(3, n, dtype=torch.uint8), z(3, n, dtype=torch.uint8), 4, 64, z(4, dtype=torch.float64),
                        mode="first_episode")
    with pytest.raises(ValueError, match="mode"):
        env.pop_fitness(z(3, n), None, None, 4, 64, z(4, dtype=torch.float64), mode="episode")
    with pytest.raises(ValueError, match="sums"):
        env.pop_fitness(z(3, n), None, None, 4, 64, z(4))   # fp32 sums
    with pytest.raises(AssertionError, match="hg_pop_fitness"):
        env.pop_fitness(z(3, n), None, None, 4, 64, z(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="thetas"):
        env.pop_pack(z(3, 5640))
    with pytest.raises(AssertionError, match="hg_pop_pack"):
        env.pop_pack(z(3, 5641))


# ---- the NumPy restatements
def test_utilities_are_centred_ranks():
    rng = np.random.default_rng(4)
    for P in (2, 6, 34, 1001):
        f = rng.normal(size=P).astype(np.float32)
        u = es_utilities_ref(f)
        assert u.dtype == np.float32 and u.shape == (P,)
        expect = (np.arange(P, dtype=np.float32) / np.float32(P - 1) - np.float32(0.5)).astype(np.float32)
        assert np.array_equal(np.sort(u), expect)           # a permutation of the centred ranks
        assert abs(float(u.astype(np.float64).sum())) <= P * 2.0 ** -24
        assert np.array_equal(np.argsort(u), np.argsort(f))  # ordered as the fitness
        assert np.array_equal(es_utilities_ref(np.exp(f)), u)
    # non-finite values rank lowest, ties (among them too) by index
    f = np.array([1.0, np.nan, 1.0, -np.inf, 3.0, np.inf, -5.0, 1.0], dtype=np.float32)
    r = np.rint((es_utilities_ref(f).astype(np.float64) + 0.5) * 7).astype(int)
    assert r.tolist() == [4, 0, 5, 1, 7, 2, 3, 6]
    assert es_utilities_ref(np.array([0.0, -0.0], dtype=np.float32)).tolist() == [-0.5, 0.5]   # -0 == 0: by index
    assert es_utilities_ref(np.array([2.0, 1.0], dtype=np.float32)).tolist() == [0.5, -0.5]


def test_grad_ref_against_a_double_loop():
    rng = np.random.default_rng(9)
    P, sigma = 6, 0.07
    f = rng.normal(size=P).astype(np.float32)
    f[2] = f[4]
    eps = rng.normal(size=(P // 2, 5572)).astype(np.float32)
    g = es_grad_ref(f, eps, sigma)
    assert g.dtype == np.float64 and g.shape == (5641,)
    u = es_utilities_ref(f)
    s = float(np.float32(sigma))
    for i in (0, 1, 2, 3, 4, 777, 5570, 5571):
        acc = 0.0
        for j in range(P // 2):
            acc += float(np.float32(u[2 * j] - u[2 * j + 1])) * float(eps[j, i])
        assert abs(g[i] - (-acc / (P * s))) <= 1e-15 * (1 + abs(g[i])), i
    assert not g[5572:].any()
    # ascending the fitness: with fitness = eps-direction projections, -grad correlates with the direction
    d = rng.normal(size=5572)
    P = 64
    eps = rng.normal(size=(P // 2, 5572)).astype(np.float32)
    fit = np.empty(P, dtype=np.float32)
    fit[0::2], fit[1::2] = eps @ d, -(eps @ d)
    assert float(-es_grad_ref(fit, eps, 0.1)[:5572] @ d) > 0
    with pytest.raises(ValueError):
        es_grad_ref(f, eps, sigma)


def test_fitness_ref_on_a_hand_written_case():
    # N = 3 envs in P = 1 member... the wrappers need multiples of 64; the reference takes any block size
    # 3 steps, env 0 done at step 1 (the middle), env 1 never, env 2 done at step 0
    r = np.array([[1.0, 10.0, 100.0], [2.0, 20.0, 200.0], [4.0, 40.0, 400.0]], dtype=np.float32)
    term = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 0]], dtype=np.uint8)
    trunc = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=np.uint8)
    s, fit, al = pop_fitness_ref(r, term, trunc, 1, 64, mode="window")
    assert s.tolist() == [777.0] and fit.tolist() == [259.0] and al.tolist() == [1, 1, 1]
    s, fit, al = pop_fitness_ref(r, term, trunc, 1, 64, mode="first_episode")
    assert s.tolist() == [3.0 + 70.0 + 100.0] and al.tolist() == [0, 1, 0]
    assert fit.dtype == np.float32 and fit[0] == np.float32(173.0 / 3.0)
    # a second chunk continues: only env 1 still counts; members of one env each with a block of 64 per member
    s2, fit2, al2 = pop_fitness_ref(r, term, trunc, 1, 64, mode="first_episode", alive=al, sums=s)
    assert s2.tolist() == [173.0 + 70.0] and al2.tolist() == [0, 1, 0]
    # per member: two members of block 2 over 3 envs, the last short
    s, fit, _ = pop_fitness_ref(r, term, trunc, 2, 2, mode="first_episode")
    assert s.tolist() == [73.0, 100.0] and fit.tolist() == [36.5, 100.0]
    # a NaN poisons its member only; after the env is done it does not enter
    rn = r.copy()
    rn[2, 0] = np.nan
    s, fit, _ = pop_fitness_ref(rn, term, trunc, 2, 2, mode="first_episode")
    assert s.tolist() == [73.0, 100.0]
    s, fit, _ = pop_fitness_ref(rn, term, trunc, 2, 2, mode="window")
    assert np.isnan(s[0]) and np.isnan(fit[0]) and s[1] == 700.0
