"""CPU-side checks of the closed-loop policy surface: the three entry points are exported, declared
in heligym_amd._abi with the header's argument counts, refuse a NULL env with a code, and the packing
helper (heligym_amd.policy) validates what it is given.  No device calls."""
import os
import re

import pytest
import torch

from conftest import ROOT

from heligym_amd import _abi, policy

HEADER = os.path.join(ROOT, "include", "heligym_amd.h")
NEW = ("hg_set_policy", "hg_policy_act", "hg_rollout_policy")


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def header_arg_counts():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(hg_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", txt):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_policy_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    assert counts["hg_rollout"] == 10   # (the parser reads a known prototype right)
    for name, n in zip(NEW, (11, 4, 11)):
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == counts[name], name
    assert lib.hg_abi_version() == 3   # purely additive


def test_policy_calls_refuse_a_null_env(lib):
    calls = {"hg_set_policy": (None,) * 11, "hg_policy_act": (None,) * 4,
             "hg_rollout_policy": (None, None, 4) + (None,) * 8}
    for name in NEW:
        lib.hg_num_envs(None)
        assert getattr(lib, name)(*calls[name]) == -1, name
        assert b"env is NULL" in lib.hg_last_error(), name


def _model(widths=(17, 64, 64, 4), dtype=torch.float32):
    nn = torch.nn
    torch.manual_seed(3)
    a, b, c, d = widths
    return nn.Sequential(nn.Linear(a, b), nn.Tanh(), nn.Linear(b, c), nn.Tanh(), nn.Linear(c, d)).to(dtype)


def test_pack_policy_accepts_pairs_and_sequential():
    m = _model()
    ref = [m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias]
    ls = torch.full((4,), -0.5)
    got_m = policy.pack_policy(m, log_std=ls)
    pairs = [(m[0].weight.detach().numpy(), m[0].bias.detach().numpy()), (m[2].weight, m[2].bias),
             (m[4].weight.t().contiguous().t(), m[4].bias)]   # numpy arrays, tensors, a non-contiguous view
    got_p = policy.pack_policy(pairs, obs_mean=torch.zeros(17), obs_scale=torch.ones(17))
    for got in (got_m, got_p):
        assert len(got) == 9
        for g, r in zip(got[:6], ref):
            assert g.dtype == torch.float32 and g.is_contiguous() and not g.requires_grad
            assert torch.equal(g, r.detach())
    assert torch.equal(got_m[6], ls) and got_m[7] is None and got_m[8] is None
    assert got_p[6] is None and got_p[7].shape == (17,) and got_p[8].shape == (17,)


def test_pack_policy_rejects_what_the_kernel_cannot_run():
    nn = torch.nn
    with pytest.raises(ValueError, match=r"\(32, 17\)"):          # a hidden layer of another width
        policy.pack_policy(_model((17, 32, 64, 4)))
    with pytest.raises(ValueError, match=r"\(64, 16\)"):          # another observation width
        policy.pack_policy(_model((16, 64, 64, 4)))
    m = _model()
    with pytest.raises(ValueError, match=r"\(64, 17\)"):          # a missing Tanh
        policy.pack_policy(nn.Sequential(m[0], m[2], m[3], m[4]))
    with pytest.raises(ValueError, match=r"\(64, 17\)"):          # another activation
        policy.pack_policy(nn.Sequential(m[0], nn.ReLU(), m[2], m[3], m[4]))
    with pytest.raises(ValueError, match=r"\(64, 17\).*float64"):  # fp64 weights
        policy.pack_policy(_model(dtype=torch.float64))
    w = [(m[0].weight, m[0].bias), (m[2].weight, m[2].bias), (m[4].weight, m[4].bias[:3])]
    with pytest.raises(ValueError, match=r"\(3,\)"):
        policy.pack_policy(w)
    with pytest.raises(ValueError, match=r"\(5,\)"):
        policy.pack_policy(m, log_std=torch.zeros(5))
    with pytest.raises(ValueError):
        policy.pack_policy(w[:2])
