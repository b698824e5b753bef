"""CPU-side checks of the device PPO update's surface (hg_ppo_opt_state_bytes, hg_ppo_opt_init, hg_ppo_shuffle,
hg_ppo_adam, hg_ppo_update, hg_set_policy_theta): the symbols are exported and declared with the header's
argument counts, refuse a NULL env, the optimiser state's layout in heligym_amd.policy is the header's, the
NumPy restatement of the shuffle (tests/ppo_shuffle_ref.py) is a permutation, and HeliVecEnv's wrappers
refuse bad arguments with ValueError before the library is called.  No device calls."""
import ctypes
import re

import numpy as np
import pytest
import torch

from ppo_shuffle_ref import shuffle_ref
from test_branch_host import _bare_env
from test_policy_host import HEADER, header_arg_counts

from heligym_amd import ActorCriticParams, PPOOptState, _abi, policy

NEW = {"hg_ppo_opt_state_bytes": 0, "hg_ppo_opt_init": 3, "hg_ppo_shuffle": 7, "hg_ppo_adam": 7, "hg_ppo_update": 23,
       "hg_set_policy_theta": 5}
SHUFFLE_SIZES = (1, 2, 3, 5, 63, 64, 65, 200, 777, 4099, 4200, 65536, 65537, 262145)


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_update_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    assert counts["hg_ppo_grad"] == 19   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == n, name
    assert lib.hg_abi_version() == 3   # purely additive


def test_update_calls_refuse_a_null_env(lib):
    cfg = _abi.hg_ppo_opt_cfg(3e-4, None, 0.9, 0.999, 1e-8, 0.5, 0.0)
    calls = {"hg_ppo_opt_init": (None, None, None),
             "hg_ppo_shuffle": (None, 8, 1, 0, None, None, None),
             "hg_ppo_adam": (None, None, None, None, None, ctypes.byref(cfg), None),
             "hg_ppo_update": (None,) * 9 + (8, 0.2, 1.0, 0.0, None, None, 1, 1, 0, None, None, None, ctypes.byref(cfg), None),
             "hg_set_policy_theta": (None,) * 5}
    for name, args in calls.items():
        lib.hg_num_envs(None)
        assert getattr(lib, name)(*args) == -1, name
        assert b"env is NULL" in lib.hg_last_error(), name


def test_state_bytes_and_layout_are_the_headers(lib):
    assert lib.hg_ppo_opt_state_bytes() == 45248 == _abi.HG_PPO_OPT_STATE_BYTES == 4 * policy.PPO_OPT_WORDS
    assert lib.hg_ppo_opt_state_bytes() % 16 == 0
    txt = open(HEADER).read()
    L = policy.PPO_OPT_LAYOUT
    assert list(L) == ["m", "v", "applied", "seen", "stop", "skipped_nonfinite", "skipped_stopped", "last_norm",
                       "last_clip_coef"]
    assert (L["m"], L["v"], policy.PPO_OPT_TAIL) == (0, 5648, 11296)
    for name in ("m", "v"):
        assert re.search(rf"\b{L[name]}: {name} \[5641\] fp32", txt), name
    assert re.search(r"\b11296: a tail of 16 words", txt)
    for name, off in L.items():
        if off >= policy.PPO_OPT_TAIL:
            kind = "fp32" if name in policy.PPO_OPT_FLOAT_WORDS else "i32"
            assert re.search(rf"\+{off - 11296} {name}\s+{kind}\b", txt), name
    assert L["v"] >= L["m"] + 5641 and policy.PPO_OPT_TAIL >= L["v"] + 5641
    # the ctypes mirror of hg_ppo_opt_cfg has the header's fields in the header's order
    body = re.search(r"typedef struct hg_ppo_opt_cfg \{(.*?)\} hg_ppo_opt_cfg;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) ==[f[0] for f in _abi.hg_ppo_opt_cfg._fields_]
    assert ctypes.sizeof(_abi.hg_ppo_opt_cfg) == 48


def test_opt_state_views_and_counters():
    s = PPOOptState("cpu")
    assert s.state.shape == (11312,) and s.state.dtype == torch.int32 and s.state.numel() * 4 == 45248
    assert s.m.shape == (5641,) and s.v.shape == (5641,) and s.m.dtype == torch.float32
    assert s.m.data_ptr() == s.state.data_ptr() and s.v.data_ptr() == s.state.data_ptr() + 4 * 5648
    assert s.seen.data_ptr() == s.state.data_ptr() + 4 * 11297
    s.state[11296:11301] = torch.tensor([3, 5, 1, 2, 7], dtype=torch.int32)
    s.state[11301:11303] = torch.tensor([1.5, 0.25]).view(torch.int32)
    assert s.counters() == dict(applied=3, seen=5, stop=1, skipped_nonfinite=2, skipped_stopped=7, last_norm=1.5,
                                last_clip_coef=0.25)
    s.m.fill_(1.0)
    assert int(s.zero_().state.abs().max()) == 0


@pytest.mark.parametrize("B", SHUFFLE_SIZES)
def test_shuffle_restatement_is_a_permutation(B):
    idx, passes = shuffle_ref(B, seed=0x1234567890ABCDEF, epoch=0)
    assert idx.dtype == np.int32 and idx.shape == (B,)
    assert np.array_equal(np.sort(idx), np.arange(B))
    assert passes.min() >= 1 and passes.mean() < 4.0   # the walk's domain is under 4 B


def test_shuffle_restatement_depends_on_epoch_and_seed():
    a, _ = shuffle_ref(4200, seed=7, epoch=0)
    b, _ = shuffle_ref(4200, seed=7, epoch=1)
    c, _ = shuffle_ref(4200, seed=8, epoch=0)
    d, _ = shuffle_ref(4200, seed=7 + 2 ** 32, epoch=0)
    e, _ = shuffle_ref(4200, seed=7, epoch=2 ** 32)
    for other in (b, c, d, e):
        assert np.mean(other == a) < 0.01   # (a random pair of permutations agrees at about 1 / B of the places)
    assert np.array_equal(a, shuffle_ref(4200, seed=7, epoch=0)[0])
    assert not np.array_equal(a, np.arange(4200))


def _params():
    nn = torch.nn
    torch.manual_seed(2)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
    return ActorCriticParams(actor, nn.Linear(64, 1), nn.Parameter(torch.full((4,), -1.0)))


def test_wrappers_validate_first():
    env = _bare_env(4)
    P, S = _params(), PPOOptState("cpu")
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)   # noqa: E731
    B = 12
    rows = (z(B, 17), z(B, 4), z(B), z(B), z(B))

    for bad in (0, -3, 2 ** 31 - 255):
        with pytest.raises(ValueError, match="B must be"):
            env.ppo_shuffle(bad, 0)
    with pytest.raises(ValueError, match="epoch_dev"):
        env.ppo_shuffle(8, 0, epoch_dev=z(1))
    with pytest.raises(ValueError, match="out"):
        env.ppo_shuffle(8, 0, out=z(8))
    with pytest.raises(ValueError, match="out"):
        env.ppo_shuffle(8, 0, out=z(9, dtype=torch.int32))
    with pytest.raises(AssertionError, match="hg_ppo_shuffle"):   # valid arguments do reach the library
        env.ppo_shuffle(8, 0, epoch_dev=S.seen, out=z(8, dtype=torch.int32))

    class Half:
        theta, grad = z(5641), z(5640)
    with pytest.raises(ValueError, match="params.grad"):
        env.ppo_adam(Half, S)
    with pytest.raises(ValueError, match="state"):
        env.ppo_adam(P, z(11312, dtype=torch.int32))
    with pytest.raises(ValueError, match="stats"):
        env.ppo_adam(P, S, stats=z(7))
    for kw, what in ((dict(lr=-1.0), "lr"), (dict(lr=float("inf")), "lr"), (dict(betas=(0.9, 1.0)), "betas"),
                     (dict(betas=(-0.1, 0.9)), "betas"), (dict(betas=(0.9,)), "betas"), (dict(eps=-1e-8), "eps"),
                     (dict(eps=float("nan")), "eps"), (dict(max_grad_norm=float("nan")), "max_grad_norm"),
                     (dict(target_kl=float("nan")), "target_kl"), (dict(lr_dev=z(2)), "lr_dev"),
                     (dict(lr_dev=z(1, dtype=torch.float64)), "lr_dev"), (dict(lr_dev=3e-4), "lr_dev")):
        with pytest.raises(ValueError, match=what):
            env.ppo_adam(P, S, **kw)
        with pytest.raises(ValueError, match=what):
            env.ppo_update(P, S, *rows, epochs=1, minibatches=2, **kw)
    with pytest.raises(AssertionError, match="hg_ppo_adam"):
        env.ppo_adam(P, S, stats=z(8), max_grad_norm=0.5, target_kl=0.02, lr_dev=z(1))

    with pytest.raises(ValueError, match="params.theta"):
        env.set_policy_theta(Half.grad)
    with pytest.raises(ValueError, match="obs_mean"):
        env.set_policy_theta(P, obs_mean=z(16))
    with pytest.raises(AssertionError, match="hg_set_policy_theta"):
        env.set_policy_theta(P, z(17), z(17))

    for k, wrong in enumerate((z(B, 16), z(B, 3), z(B + 1), z(B, dtype=torch.float64), z(2 * B)[::2])):
        bad_rows = list(rows)
        bad_rows[k] = wrong
        with pytest.raises(ValueError):
            env.ppo_update(P, S, *bad_rows, epochs=1, minibatches=2)
    with pytest.raises(ValueError, match="epochs"):
        env.ppo_update(P, S, *rows, epochs=0, minibatches=2)
    for n in (0, B + 1):
        with pytest.raises(ValueError, match="minibatches"):
            env.ppo_update(P, S, *rows, epochs=1, minibatches=n)
    with pytest.raises(ValueError, match="stats"):
        env.ppo_update(P, S, *rows, epochs=2, minibatches=3, stats=z(5, 8))
    with pytest.raises(ValueError, match="index"):
        env.ppo_update(P, S, *rows, epochs=2, minibatches=3, index=z(B))
    with pytest.raises(ValueError, match="state"):
        env.ppo_update(P, None, *rows, epochs=2, minibatches=3)
    with pytest.raises(ValueError, match="obs_scale"):
        env.ppo_update(P, S, *rows, epochs=2, minibatches=3, obs_scale=z(17, dtype=torch.float64))
    with pytest.raises(AssertionError, match="hg_ppo"):
        env.ppo_update(P, S, z(3, 4, 17), z(3, 4, 4), z(3, 4), z(3, 4), z(3, 4), epochs=2, minibatches=3,
                       stats=z(6, 8), index=z(B, dtype=torch.int32), obs_mean=z(17), obs_scale=z(17), publish=True)
