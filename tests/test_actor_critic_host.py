"""CPU-side checks of the actor-critic surface: the four entry points are exported, declared in
heligym_amd._abi with the header's argument counts, refuse a NULL env with a code, and
heligym_amd.policy.pack_value_head validates what it is given.  No device calls."""
import pytest
import torch

from heligym_amd import _abi, policy
from test_policy_host import header_arg_counts

NEW = {"hg_set_value_head": 4, "hg_policy_eval": 6, "hg_rollout_ac": 14, "hg_gae": 12}


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_actor_critic_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    assert counts["hg_rollout_policy"] == 11   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == counts[name], name
    assert lib.hg_abi_version() == 3   # purely additive


def test_actor_critic_calls_refuse_a_null_env(lib):
    calls = {"hg_set_value_head": (None,) * 4, "hg_policy_eval": (None,) * 6,
             "hg_rollout_ac": (None, None, 4) + (None,) * 11,
             "hg_gae": (None,) * 6 + (4, 0.99, 0.95) + (None,) * 3}
    for name in NEW:
        lib.hg_num_envs(None)
        assert getattr(lib, name)(*calls[name]) == -1, name
        assert b"env is NULL" in lib.hg_last_error(), name


def test_pack_value_head_accepts_linear_and_pairs():
    torch.manual_seed(4)
    lin = torch.nn.Linear(64, 1)
    ref_w, ref_b = lin.weight.detach().reshape(64), lin.bias.detach()
    forms = (lin, (lin.weight, lin.bias), (lin.weight.detach().reshape(64), lin.bias),
             (lin.weight.detach().numpy(), lin.bias.detach().numpy()),
             (lin.weight.detach().reshape(64, 1).t(), lin.bias))   # a non-contiguous [1,64] view
    for head in forms:
        w, b = policy.pack_value_head(head)
        assert tuple(w.shape) == (64,) and tuple(b.shape) == (1,)
        assert w.dtype == torch.float32 and b.dtype == torch.float32
        assert w.is_contiguous() and b.is_contiguous() and not w.requires_grad and not b.requires_grad
        assert torch.equal(w, ref_w) and torch.equal(b, ref_b)


def test_pack_value_head_rejects_what_the_kernel_cannot_run():
    nn = torch.nn
    with pytest.raises(ValueError, match=r"\(1, 32\)"):             # another trunk width
        policy.pack_value_head(nn.Linear(32, 1))
    with pytest.raises(ValueError, match=r"\(2, 64\)"):             # two outputs
        policy.pack_value_head(nn.Linear(64, 2))
    with pytest.raises(ValueError, match=r"\(63,\)"):
        policy.pack_value_head((torch.zeros(63), torch.zeros(1)))
    with pytest.raises(ValueError, match=r"\(64,\) and \(2,\)"):    # a bias of another shape
        policy.pack_value_head((torch.zeros(64), torch.zeros(2)))
    with pytest.raises(ValueError, match=r"\(1, 64\).*float64"):    # fp64 weights
        policy.pack_value_head(nn.Linear(64, 1).double())
    with pytest.raises(ValueError, match=r"\(64,\).*float64"):
        policy.pack_value_head((torch.zeros(64), torch.zeros(1, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"\(1, 64\).*no bias"):    # a missing bias
        policy.pack_value_head(nn.Linear(64, 1, bias=False))
    with pytest.raises(ValueError, match="no bias"):
        policy.pack_value_head((torch.zeros(64), None))
    with pytest.raises(ValueError):
        policy.pack_value_head(nn.Tanh())
