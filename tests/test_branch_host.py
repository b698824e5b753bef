"""CPU-side checks of the branched planning surface (hg_rollout_branch, hg_mppi_sample, hg_mppi_update):
the header declares the three functions and heligym_amd._abi binds them with the header's argument
counts, the library exports them, they refuse bad arguments with HG_E_INVALID and a message without a
device, HeliVecEnv's wrappers refuse wrong shapes, dtypes and devices with ValueError before the library
is called, and MPPI.shift / reset do what they say on a stub env.  No device calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from heligym_amd import MPPI, HeliVecEnv, _abi

HEADER = os.path.join(ROOT, "include", "heligym_amd.h")
NEW = {"hg_rollout_branch": 10, "hg_mppi_sample": 10, "hg_mppi_update": 8}


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_and_abi_binds_the_three_calls(lib):
    txt = _header()
    counts = {}
    for name, args in re.findall(r"\b(hg_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", txt):
        counts[name] = 0 if args.strip() in ("", "void") else len(args.split(","))
    assert counts["hg_rollout"] == 10   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert counts.get(name) == n, (name, counts.get(name))
        assert name in _abi.EXPORTED_SYMBOLS
        assert len(_abi._SIGS[name][1]) == n, name
        assert hasattr(lib, name), name
    m = re.search(r"enum\s*\{\s*HG_BRANCH_NOISE_ENV\s*=\s*(\d+)\s*,\s*HG_BRANCH_NOISE_OFF\s*=\s*(\d+)\s*\}", txt)
    assert m and (int(m.group(1)), int(m.group(2))) == (_abi.HG_BRANCH_NOISE_ENV, _abi.HG_BRANCH_NOISE_OFF) == (0, 1)
    assert _abi.BRANCH_NOISE_MODES == {"env": 0, "off": 1}
    assert re.search(r"#define\s+HG_ABI_VERSION\s+3\b", txt) and lib.hg_abi_version() == 3   # purely additive


F4 = ctypes.c_float * 4
P16, P4 = 0x1000, 0x1004   # never dereferenced: every call below is refused before any launch


def _refused(lib, rc, text):
    assert rc == -1, (rc, text)
    assert text.encode() in lib.hg_last_error(), (text, lib.hg_last_error())


def test_rollout_branch_refuses_bad_arguments_without_a_device(lib):
    def call(env=None, actions=P16, horizon=4, branches=3, gamma=1.0, noise=0, ret=P16, alive=None, end=None):
        return lib.hg_rollout_branch(env, actions, horizon, branches, gamma, noise, ret, alive, end, None)

    _refused(lib, call(horizon=0), "horizon must be >= 1")
    _refused(lib, call(branches=0), "branches must be >= 1")
    _refused(lib, call(branches=-2), "branches must be >= 1")
    for g in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        _refused(lib, call(gamma=g), "gamma must be in (0, 1]")
    for m in (-1, 2):
        _refused(lib, call(noise=m), "noise_mode")
    _refused(lib, call(actions=None), "must be device pointers")
    _refused(lib, call(ret=None), "must be device pointers")
    _refused(lib, call(actions=P4), "16-byte aligned")
    _refused(lib, call(), "env is NULL")   # everything else in order: the handle is what is missing


def test_mppi_calls_refuse_bad_arguments_without_a_device(lib):
    one, zero = F4(1, 1, 1, 1), F4(0, 0, 0, 0)

    def sample(nominal=P16, horizon=4, branches=3, sigma=one, lo=zero, hi=one, out=P16):
        return lib.hg_mppi_sample(None, nominal, horizon, branches, sigma, lo, hi, 7, out, None)

    _refused(lib, sample(horizon=0), "horizon must be >= 1")
    _refused(lib, sample(branches=0), "branches must be >= 1")
    _refused(lib, sample(sigma=None), "sigma/lo/hi")
    _refused(lib, sample(sigma=F4(1, -1, 1, 1)), "sigma must be finite and >= 0")
    _refused(lib, sample(lo=one, hi=zero), "lo must be <= hi")
    _refused(lib, sample(lo=F4(0, 0, float("nan"), 0)), "lo must be <= hi")
    _refused(lib, sample(nominal=None), "must be device pointers")
    _refused(lib, sample(out=P4), "16-byte aligned")
    _refused(lib, sample(), "env is NULL")

    def update(actions=P16, ret=P16, horizon=4, branches=3, lam=1.0, out=0x2000):
        return lib.hg_mppi_update(None, actions, ret, horizon, branches, lam, out, None)

    _refused(lib, update(horizon=-1), "horizon must be >= 1")
    _refused(lib, update(branches=0), "branches must be >= 1")
    for lam in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
        _refused(lib, update(lam=lam), "lambda must be > 0")
    _refused(lib, update(ret=None), "must be device pointers")
    _refused(lib, update(out=None), "must be device pointers")
    _refused(lib, update(), "env is NULL")


class _NoLib:
    """Stands where the library would: a wrapper that reaches it did not validate first."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were validated")


def _bare_env(n):
    env = HeliVecEnv.__new__(HeliVecEnv)   # no handle, no device: the wrappers' validation only
    env.torch, env.device, env.num_envs, env.lib, env._h = torch, torch.device("cpu"), n, _NoLib(), None
    return env


def test_wrappers_validate_shapes_dtypes_and_devices_first():
    n, B, H = 5, 3, 4
    env = _bare_env(n)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)   # noqa: E731
    bad_actions = [z(H, n * B, 3), z(H, n * B + 1, 4), z(H, n * B), z(H, n * B, 4, dtype=torch.float64),
                   z(H, n * B, 8)[:, :, ::2], z(H, n * B, 4, dtype=torch.float32).to("meta"), np.zeros((H, n * B, 4))]
    for a in bad_actions:
        with pytest.raises(ValueError):
            env.rollout_branch(a, B)
    for b in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="branches"):
            env.rollout_branch(z(H, n * B, 4), b)
    with pytest.raises(ValueError, match="noise"):
        env.rollout_branch(z(H, n * B, 4), B, noise="white")
    ok_out = dict(returns=z(n, B), alive_steps=z(n, B, dtype=torch.int32), end_info=z(n, B, dtype=torch.uint8))
    for key, wrong in (("returns", z(n * B)), ("alive_steps", z(n, B)), ("end_info", z(n, B, dtype=torch.int8))):
        with pytest.raises(ValueError, match=key):
            env.rollout_branch(z(H, n * B, 4), B, out={**ok_out, key: wrong})
    with pytest.raises(AssertionError, match="hg_rollout_branch"):   # valid arguments do reach the library
        env.rollout_branch(z(H, n * B, 4), B, out=ok_out)

    for nominal in (z(H, n + 1, 4), z(H, n, 3), z(n, 4), z(H, n, 4, dtype=torch.float16)):
        with pytest.raises(ValueError, match="nominal"):
            env.mppi_sample(nominal, B, 0.1, -1.0, 1.0, 0)
    with pytest.raises(ValueError, match="sigma"):
        env.mppi_sample(z(H, n, 4), B, [0.1, 0.2], -1.0, 1.0, 0)
    with pytest.raises(ValueError, match="out"):
        env.mppi_sample(z(H, n, 4), B, 0.1, -1.0, 1.0, 0, out=z(H, n * B, 3))
    with pytest.raises(AssertionError, match="hg_mppi_sample"):
        env.mppi_sample(z(H, n, 4), B, 0.1, [-1, -1, -1, -1], 1.0, 0)

    with pytest.raises(ValueError, match="returns"):
        env.mppi_update(z(H, n * B, 4), z(n * B), 1.0)
    with pytest.raises(ValueError, match="returns"):
        env.mppi_update(z(H, n * B, 4), z(n + 1, B), 1.0)
    with pytest.raises(ValueError, match="actions"):
        env.mppi_update(z(H, n * (B + 1), 4), z(n, B), 1.0)
    with pytest.raises(ValueError, match="out"):
        env.mppi_update(z(H, n * B, 4), z(n, B), 1.0, out=z(H, n * B, 4))
    with pytest.raises(AssertionError, match="hg_mppi_update"):
        env.mppi_update(z(H, n * B, 4), z(n, B), 1.0)


class _StubEnv:
    """What MPPI reads of an env, on the CPU: the three planning calls are recorded, mppi_update writes
    a recognisable nominal."""
    TRIM = (0.25, -0.5, 0.125, 0.75)

    def __init__(self, n):
        self.torch, self.device, self.num_envs, self.calls = torch, torch.device("cpu"), n, []

    def template(self):
        return {"action": np.array(self.TRIM, dtype=np.float64)}

    def mppi_sample(self, nominal, branches, sigma, lo, hi, seed, out=None):
        self.calls.append(("sample", seed))
        out.copy_(nominal.repeat_interleave(branches, dim=1))
        return out

    def rollout_branch(self, actions, branches, gamma=1.0, noise="env", out=None):
        self.calls.append(("branch", gamma, noise))
        return out or dict(returns=torch.zeros((self.num_envs, branches)))

    def mppi_update(self, actions, returns, lam, out=None):
        self.calls.append(("update", lam))
        out.copy_(actions[:, ::returns.shape[1]] + 1.0)
        return out


def test_mppi_shift_reset_and_plan_on_a_stub_env():
    n, H, B = 6, 5, 4
    env = _StubEnv(n)
    m = MPPI(env, H, B, sigma=0.1, lam=2.0, gamma=0.5, noise="off", seed=40)
    trim = torch.tensor(_StubEnv.TRIM)
    assert m.nominal.shape == (H, n, 4) and m.nominal.is_contiguous() and torch.equal(m.nominal, trim.expand(H, n, 4))
    assert m.actions.shape == (H, n * B, 4)

    a0 = m.plan(iterations=2)   # the stub's update adds 1 per iteration
    assert env.calls == [("sample", 40), ("branch", 0.5, "off"), ("update", 2.0),
                         ("sample", 41), ("branch", 0.5, "off"), ("update", 2.0)]
    assert a0.shape == (n, 4) and torch.equal(a0, trim.expand(n, 4) + 2.0)

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
    assert torch.equal(m.nominal[:, ~keep], trim.expand(H, 2, 4))
    with pytest.raises(ValueError, match="mask"):
        m.reset(torch.zeros(n + 1))
    m.reset()
    assert torch.equal(m.nominal, trim.expand(H, n, 4))

    one = MPPI(env, 1, B, sigma=0.1, lam=1.0)   # a one-step horizon: shift repeats its only row
    one.nominal.fill_(3.0)
    one.shift()
    assert torch.equal(one.nominal, torch.full((1, n, 4), 3.0))
    with pytest.raises(ValueError):
        MPPI(env, 0, B, sigma=0.1, lam=1.0)
