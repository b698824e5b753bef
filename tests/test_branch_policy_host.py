"""CPU-side checks of the policy-guided planning surface (hg_policy_act_mean, hg_rollout_branch_policy,
PolicyMPPI): the header declares the two functions and heligym_amd._abi binds them with the header's
argument counts, the library exports them and the ABI version is still 3; they refuse bad arguments with
HG_E_INVALID and a message naming the argument without a device; HeliVecEnv's wrappers refuse wrong
shapes, dtypes and devices with ValueError before the library is called; PolicyMPPI.shift / reset / plan do
what they say on a stub env.  The refusals that need a handle (no policy set, no value head) are in
test_gpu_branch_policy.py.  No device calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from heligym_amd import MPPI, HeliVecEnv, PolicyMPPI, _abi

HEADER = os.path.join(ROOT, "include", "heligym_amd.h")
NEW = {"hg_policy_act_mean": 8, "hg_rollout_branch_policy": 15}


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def test_header_declares_and_abi_binds_the_two_calls(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    counts = {}
    for name, args in re.findall(r"\b(hg_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", txt):
        counts[name] = 0 if args.strip() in ("", "void") else len(args.split(","))
    assert counts["hg_rollout_branch"] == 10   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert counts.get(name) == n, (name, counts.get(name))
        assert name in _abi.EXPORTED_SYMBOLS
        assert len(_abi._SIGS[name][1]) == n, name
        assert hasattr(lib, name), name
    m = re.search(r"enum\s*\{\s*HG_BOOTSTRAP_NONE\s*=\s*(\d+)\s*,\s*HG_BOOTSTRAP_VALUE\s*=\s*(\d+)\s*\}", txt)
    assert m and (int(m.group(1)), int(m.group(2))) == (_abi.HG_BOOTSTRAP_NONE, _abi.HG_BOOTSTRAP_VALUE) == (0, 1)
    assert re.search(r"#define\s+HG_ABI_VERSION\s+3\b", txt) and lib.hg_abi_version() == 3   # purely additive


F4 = ctypes.c_float * 4
P16, P4, P2 = 0x1000, 0x1004, 0x1002   # never dereferenced: every call below is refused before any launch
NAN, INF = float("nan"), float("inf")


def _refused(lib, rc, text):
    assert rc == -1, (rc, text)
    assert text.encode() in lib.hg_last_error(), (text, lib.hg_last_error())


def test_rollout_branch_policy_refuses_bad_arguments_without_a_device(lib):
    one, neg = F4(1, 1, 1, 1), F4(-1, -1, -1, -1)

    def call(obs0=P16, res=P16, horizon=4, branches=3, gamma=1.0, noise=0, lo=neg, hi=one, boot=0, scale=1.0, ret=P16,
             alive=None, end=None):
        return lib.hg_rollout_branch_policy(None, obs0, res, horizon, branches, gamma, noise, lo, hi, boot, scale, ret,
                                            alive, end, None)

    # what hg_rollout_branch refuses
    _refused(lib, call(horizon=0), "horizon must be >= 1")
    _refused(lib, call(branches=0), "branches must be >= 1")
    _refused(lib, call(branches=-2), "branches must be >= 1")
    for g in (0.0, -0.5, 1.0000001, NAN, INF):
        _refused(lib, call(gamma=g), "gamma must be in (0, 1]")
    for m in (-1, 2):
        _refused(lib, call(noise=m), "noise_mode")
    # its own
    for b in (-1, 2, 7):
        _refused(lib, call(boot=b), "bootstrap must be")
    for s in (NAN, INF, -INF):
        _refused(lib, call(scale=s), "value_scale must be finite")
    _refused(lib, call(lo=None), "lo and hi go together")
    _refused(lib, call(hi=None), "lo and hi go together")
    _refused(lib, call(lo=F4(0, 0, NAN, 0)), "lo must be <= hi")
    _refused(lib, call(hi=F4(0, NAN, 0, 0)), "lo must be <= hi")
    _refused(lib, call(lo=one, hi=neg), "lo must be <= hi")
    _refused(lib, call(lo=F4(0, 0, 0, 0.5), hi=F4(1, 1, 1, 0.25)), "lo must be <= hi")
    _refused(lib, call(obs0=None), "obs0/return must be device pointers")
    _refused(lib, call(ret=None), "obs0/return must be device pointers")
    _refused(lib, call(res=P4), "residual must be 16-byte aligned")
    _refused(lib, call(ret=P2), "4-byte aligned")
    _refused(lib, call(alive=P2), "4-byte aligned")
    # everything else in order -- with or without a residual and a clamp: the handle is what is missing
    _refused(lib, call(), "env is NULL")
    _refused(lib, call(res=None, lo=None, hi=None, boot=1, scale=0.25), "env is NULL")


def test_policy_act_mean_refuses_bad_arguments_without_a_device(lib):
    one, neg = F4(1, 1, 1, 1), F4(-1, -1, -1, -1)

    def call(obs=P16, res=P16, lo=neg, hi=one, act=P16, val=None):
        return lib.hg_policy_act_mean(None, obs, res, lo, hi, act, val, None)

    _refused(lib, call(lo=None), "lo and hi go together")
    _refused(lib, call(hi=None), "lo and hi go together")
    _refused(lib, call(lo=F4(NAN, 0, 0, 0)), "lo must be <= hi")
    _refused(lib, call(lo=one, hi=neg), "lo must be <= hi")
    _refused(lib, call(obs=None), "obs must be a device pointer")
    _refused(lib, call(res=P4), "residual and actions must be 16-byte aligned")
    _refused(lib, call(act=P4), "residual and actions must be 16-byte aligned")
    _refused(lib, call(val=P2), "value must be 4-byte aligned")
    _refused(lib, call(), "env is NULL")
    _refused(lib, call(res=None, lo=None, hi=None, act=None, val=P4), "env is NULL")


class _NoLib:
    """Stands where the library would: a wrapper that reaches it did not validate first."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were validated")


def _bare_env(n):
    env = HeliVecEnv.__new__(HeliVecEnv)   # no handle, no device: the wrappers' validation only
    env.torch, env.device, env.num_envs, env.lib, env._h = torch, torch.device("cpu"), n, _NoLib(), None
    env.obs = torch.zeros((n, 17))
    return env


def test_wrappers_validate_shapes_dtypes_and_devices_first():
    n, B, H = 5, 3, 4
    env = _bare_env(n)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)   # noqa: E731
    bad_res = [z(H, n * B, 3), z(H, n * B + 1, 4), z(H, n * B), z(H, n * B, 4, dtype=torch.float64),
               z(H, n * B, 8)[:, :, ::2], z(H, n * B, 4).to("meta"), np.zeros((H, n * B, 4)), 4]
    for r in bad_res:
        with pytest.raises(ValueError):
            env.rollout_branch_policy(r, B)
    with pytest.raises(ValueError, match="horizon"):
        env.rollout_branch_policy(None, B)
    with pytest.raises(ValueError, match="horizon"):
        env.rollout_branch_policy(None, B, horizon=0)
    with pytest.raises(ValueError, match="horizon"):
        env.rollout_branch_policy(z(H, n * B, 4), B, horizon=H + 1)
    for b in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="branches"):
            env.rollout_branch_policy(z(H, n * B, 4), b)
    for o in (z(n + 1, 17), z(n, 16), z(n, 17, dtype=torch.float64), z(n, 17).to("meta"), z(n, 34)[:, ::2]):
        with pytest.raises(ValueError, match="obs0"):
            env.rollout_branch_policy(z(H, n * B, 4), B, obs0=o)
    with pytest.raises(ValueError, match="noise"):
        env.rollout_branch_policy(z(H, n * B, 4), B, noise="white")
    with pytest.raises(ValueError, match="lo and hi"):
        env.rollout_branch_policy(z(H, n * B, 4), B, lo=-1.0)
    with pytest.raises(ValueError, match="hi"):
        env.rollout_branch_policy(z(H, n * B, 4), B, lo=-1.0, hi=[1.0, 1.0])
    with pytest.raises(ValueError, match="value_scale"):
        env.rollout_branch_policy(z(H, n * B, 4), B, value_scale=float("inf"))
    ok_out = dict(returns=z(n, B), alive_steps=z(n, B, dtype=torch.int32), end_info=z(n, B, dtype=torch.uint8))
    for key, wrong in (("returns", z(n * B)), ("alive_steps", z(n, B)), ("end_info", z(n, B, dtype=torch.int8))):
        with pytest.raises(ValueError, match=key):
            env.rollout_branch_policy(z(H, n * B, 4), B, out={**ok_out, key: wrong})
    with pytest.raises(AssertionError, match="hg_rollout_branch_policy"):   # valid arguments do reach the library
        env.rollout_branch_policy(z(H, n * B, 4), B, lo=-1.0, hi=1.0, bootstrap=True, value_scale=0.25, out=ok_out)
    with pytest.raises(AssertionError, match="hg_rollout_branch_policy"):
        env.rollout_branch_policy(None, 1, horizon=H, obs0=z(n, 17))

    for o in (z(n + 1, 17), z(n, 17, dtype=torch.float16)):
        with pytest.raises(ValueError, match="obs"):
            env.policy_act_mean(o)
    for r in (z(n, 3), z(n + 1, 4), z(n, 4, dtype=torch.float64), z(n, 8)[:, ::2], np.zeros((n, 4))):
        with pytest.raises(ValueError, match="residual"):
            env.policy_act_mean(residual=r)
    with pytest.raises(ValueError, match="lo and hi"):
        env.policy_act_mean(hi=1.0)
    with pytest.raises(ValueError, match="out"):
        env.policy_act_mean(out=z(n, 3))
    with pytest.raises(AssertionError, match="hg_policy_act_mean"):
        env.policy_act_mean(z(n, 17), residual=z(n, 4), lo=-1.0, hi=[1, 1, 1, 1], value=True)


class _StubEnv:
    """What PolicyMPPI reads of an env, on the CPU: its calls are recorded, mppi_update writes a
    recognisable nominal, policy_act_mean returns residual + 10."""

    def __init__(self, n):
        self.torch, self.device, self.num_envs, self.calls = torch, torch.device("cpu"), n, []

    def template(self):
        raise AssertionError("PolicyMPPI's nominal is a residual: it does not start from the trim action")

    def mppi_sample(self, nominal, branches, sigma, lo, hi, seed, out=None):
        self.calls.append(("sample", seed, lo, hi))
        out.copy_(nominal.repeat_interleave(branches, dim=1))
        return out

    def rollout_branch_policy(self, residuals, branches, obs0=None, gamma=1.0, noise="env", lo=None, hi=None,
                              bootstrap=False, value_scale=1.0, out=None):
        self.calls.append(("branch_policy", obs0, gamma, noise, lo, hi, bootstrap, value_scale))
        return out or dict(returns=torch.zeros((self.num_envs, branches)))

    def mppi_update(self, actions, returns, lam, out=None):
        self.calls.append(("update", lam))
        out.copy_(actions[:, ::returns.shape[1]] + 1.0)
        return out

    def policy_act_mean(self, obs=None, residual=None, lo=None, hi=None, out=None, value=False):
        self.calls.append(("act", obs, lo, hi))
        out.copy_(residual + 10.0)
        return out


def test_policy_mppi_shift_reset_and_plan_on_a_stub_env():
    n, H, B = 6, 5, 4
    env = _StubEnv(n)
    m = PolicyMPPI(env, H, B, sigma=0.1, lam=2.0, res_lo=-0.25, res_hi=0.5, lo=-1.0, hi=1.0, gamma=0.5, noise="off",
                   seed=40, bootstrap=True, value_scale=0.125)
    assert isinstance(m, MPPI)
    assert m.nominal.shape == (H, n, 4) and m.nominal.is_contiguous() and not m.nominal.any()   # a zero residual
    assert m.actions.shape == (H, n * B, 4)

    obs = torch.ones((n, 17))
    a0 = m.plan(obs, iterations=2)   # the stub's update adds 1 per iteration, its act 10
    bp = ("branch_policy", obs, 0.5, "off", -1.0, 1.0, True, 0.125)
    assert env.calls == [("sample", 40, -0.25, 0.5), bp, ("update", 2.0), ("sample", 41, -0.25, 0.5), bp, ("update", 2.0),
                         ("act", obs, -1.0, 1.0)]
    assert a0.shape == (n, 4) and torch.equal(a0, torch.full((n, 4), 12.0)) and a0 is m.action
    assert torch.equal(m.nominal, torch.full((H, n, 4), 2.0))
    env.calls.clear()
    m.plan()   # obs=None: the env's own observations, in the scoring and in the act call alike
    assert env.calls[1][1] is None and env.calls[-1][:2] == ("act", None)

    seq = torch.arange(H * n * 4, dtype=torch.float32).reshape(H, n, 4)
    m.nominal.copy_(seq)
    m.shift()
    assert torch.equal(m.nominal[:-1], seq[1:]) and torch.equal(m.nominal[-1], seq[-1])
    assert m.nominal.is_contiguous()

    mask = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.uint8)
    before = m.nominal.clone()
    m.reset(mask)
    keep = mask == 0
    assert torch.equal(m.nominal[:, keep], before[:, keep])
    assert not m.nominal[:, ~keep].any()   # back to a zero residual
    with pytest.raises(ValueError, match="mask"):
        m.reset(torch.zeros(n + 1))
    m.reset()
    assert not m.nominal.any()
    with pytest.raises(ValueError):
        PolicyMPPI(env, 0, B, sigma=0.1, lam=1.0)
