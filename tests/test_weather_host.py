"""CPU-side checks of the per-env weather surface (hg_set_weather, hg_get_weather, hg_weather_constants,
HeliVecEnv.set_weather / get_weather, sample_weather): the symbols are exported and declared with the header's
argument counts; each call refuses a NULL env and every out-of-range argument that needs no handle; the
constants of a weather are bitwise the handle-wide ones derive() forms for an airframe document with that ENV
block; sample_weather is a function of its seed and stays inside its ranges.  No device calls."""
import ctypes

import numpy as np
import pytest

import golden_cases as gc
from test_branch_host import _bare_env
from test_policy_host import header_arg_counts

import heligym_amd
from heligym_amd import _abi, config, sample_weather

NEW = {"hg_set_weather": 5, "hg_get_weather": 4, "hg_weather_constants": 4}
A16 = 0x10000   # a stand-in for a device pointer: never dereferenced


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _refused(lib, rc, text):
    assert rc == -1, (rc, text)
    assert text.encode() in lib.hg_last_error(), (lib.hg_last_error(), text)


def test_weather_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    assert counts["hg_rollout_policy"] == 11   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == n, name
    assert lib.hg_abi_version() == 3 == _abi.HG_ABI_VERSION   # purely additive
    assert ctypes.sizeof(_abi.hg_weather) == 12
    assert [f[0] for f in _abi.hg_weather._fields_] == ["turb_level", "wind_dir_deg", "wind_spd"]
    assert "sample_weather" in heligym_amd.__all__ and hasattr(heligym_amd, "sample_weather")
    for name in ("set_weather", "get_weather"):
        assert callable(getattr(heligym_amd.HeliVecEnv, name))


def _constants(lib, cfg, turb, wdir, spd):
    w = _abi.hg_weather(turb, wdir, spd)
    rec, tep = (ctypes.c_float * 8)(), (ctypes.c_float * 16)()
    rc = lib.hg_weather_constants(ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(w), rec, tep)
    return rc, np.array(rec, dtype=np.float32), np.array(tep, dtype=np.float32)


def test_every_call_refuses_a_null_env_and_bad_arguments(lib):
    w = (_abi.hg_weather * 1)(_abi.hg_weather(1.0, 45.0, 20.0))
    _refused(lib, lib.hg_set_weather(None, w, None, None, None), "env is NULL")
    _refused(lib, lib.hg_set_weather(None, None, None, None, None), "env is NULL")
    _refused(lib, lib.hg_get_weather(None, w, A16, None), "env is NULL")
    cfg, _ = config.make_config()
    rec, tep = (ctypes.c_float * 8)(), (ctypes.c_float * 16)()
    _refused(lib, lib.hg_weather_constants(None, w, rec, tep), "NULL argument")
    _refused(lib, lib.hg_weather_constants(ctypes.byref(cfg), None, rec, tep), "NULL argument")
    _refused(lib, lib.hg_weather_constants(ctypes.byref(cfg), w, None, tep), "NULL argument")
    _refused(lib, lib.hg_weather_constants(ctypes.byref(cfg), w, rec, None), "NULL argument")
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 0, 0), (0, nan, 0), (0, 0, nan), (inf, 0, 0), (0, -inf, 0), (0, 0, inf)):
        _refused(lib, _constants(lib, cfg, *bad)[0], "non-finite")
    for turb in (-0.001, 7.001, -1.0, 8.0):
        _refused(lib, _constants(lib, cfg, turb, 0.0, 0.0)[0], "turb_level outside [0, 7]")
    _refused(lib, _constants(lib, cfg, 1.0, 0.0, -0.5)[0], "negative wind_spd")
    for ok in ((0.0, 0.0, 0.0), (7.0, 360.0, 200.0), (3.5, -90.0, 1.0)):   # the ends are inside; any finite direction
        assert _constants(lib, cfg, *ok)[0] == 0, ok


def test_wrappers_validate_shapes_first():
    env = _bare_env(5)
    env.cfg, _ = config.make_config()
    for kw in (dict(turb_level=np.zeros(4)), dict(wind_dir=np.zeros((5, 1))), dict(wind_spd=[1.0, 2.0])):
        with pytest.raises(ValueError, match="set_weather"):
            env.set_weather(**kw)
    with pytest.raises(ValueError, match="trim conditions"):
        env.set_weather(turb_level=1.0, conds=[{}] * 4)


WM_WORD = 107   # the word of Params<float>::wm[0] (csrc/physics.h: every field before it is a 4-byte word)


def _params_wind_fields(lib, cfg):
    """The wind fields of Params<float> for `cfg` through hg_debug_params, at their offsets: wm[3] | cos | sin |
    w20 | sigma_low | turb_level | eta_norm | tep_row[13], after hm_rows, hm_cols.  The neighbours whose values
    are known independently (the terrain's shape before, 1 / sqrt(dt) inside) pin the offset."""
    buf = None
    for size in range(256, 8192, 4):   # hg_debug_params accepts only sizeof(Params<float>)
        b = (ctypes.c_float * (size // 4))()
        if lib.hg_debug_params(ctypes.byref(cfg), 1024, 768, 0, b, size) == 0:
            buf = np.array(b, dtype=np.float32)
            break
    assert buf is not None
    k = WM_WORD
    assert list(buf[k - 2:k].view(np.int32)) == [1024, 768], "Params<float> moved: update WM_WORD"
    assert buf[k + 8] == np.float32(1.0 / np.sqrt(cfg.dt)) and buf[k + 2] == 0
    return {"wm": buf[k:k + 2], "wm2": buf[k + 2], "cos": buf[k + 3], "sin": buf[k + 4], "sigma_low": buf[k + 6],
            "turb_level": buf[k + 7], "tep_row": buf[k + 9:k + 22]}


@pytest.mark.parametrize("name", ["default", "turb0", "turb5", "turb7_wind"])
def test_weather_constants_bitwise_equal_the_handle_wide_ones(lib, name):
    """hg_weather_constants for an ENV block against hg_debug_params of a config built from the airframe
    document with that block: wm[0..1], the direction's cos / sin, sigma_low, turb_level and tep_row[0..12]
    bit for bit, through the default airframe's config (the weather is not read from it)."""
    doc = "aw109" if name == "default" else gc.load_variant(name)[1]
    cfg, _ = config.make_config(heli_name=doc)
    own, _ = config.make_config()
    f = _params_wind_fields(lib, cfg)
    af = cfg.af
    rc, rec, tep = _constants(lib, own, float(af.env_TURB_LVL), float(af.env_WIND_DIR_deg), float(af.env_WIND_SPD))
    assert rc == 0
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.int32)   # noqa: E731
    np.testing.assert_array_equal(i32(rec[0:2]), i32(f["wm"]))
    assert f["wm2"] == 0
    np.testing.assert_array_equal(i32(rec[2:6]), i32([f["cos"], f["sin"], f["sigma_low"], f["turb_level"]]))
    np.testing.assert_array_equal(i32(rec[6:8]), [0, 0])
    np.testing.assert_array_equal(i32(tep[:13]), i32(f["tep_row"]))
    np.testing.assert_array_equal(i32(tep[13:]), [0, 0, 0])
    if name == "turb7_wind":   # the recording's ENV edits did reach the config
        assert (af.env_TURB_LVL, af.env_WIND_SPD, af.env_WIND_DIR_deg) == (7, 35.0, 120.0)
        assert not np.array_equal(rec, _constants(lib, own, 1.0, 45.0, 20.0)[1])


def test_sample_weather_is_deterministic_and_in_range():
    a = sample_weather(1000, seed=3)
    b = sample_weather(1000, seed=3)
    c = sample_weather(1000, seed=4)
    assert sorted(a) == ["turb_level", "wind_dir", "wind_spd"]
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == (1000,)
        np.testing.assert_array_equal(a[k], b[k])
        assert not np.array_equal(a[k], c[k])
    for k, (lo, hi) in (("turb_level", (0.0, 7.0)), ("wind_spd", (0.0, 40.0)), ("wind_dir", (0.0, 360.0))):
        assert a[k].min() >= lo and a[k].max() <= hi and a[k].max() - a[k].min() > 0.9 * (hi - lo)
    d = sample_weather(4096, turb_level=(2.5, 2.6), wind_spd=(0.1, 0.3), wind_dir=90.0, seed=1)
    assert d["turb_level"].min() >= 2.5 and d["turb_level"].max() <= 2.6
    assert d["wind_spd"].astype(np.float64).min() >= 0.1 and d["wind_spd"].astype(np.float64).max() <= 0.3
    assert np.all(d["wind_dir"] == 90.0)
    assert len(sample_weather(0)["turb_level"]) == 0
    with pytest.raises(ValueError):
        sample_weather(4, turb_level=(3.0, 2.0))
