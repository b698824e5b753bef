"""CPU-side checks of the mixed-fleet surface (hg_set_fleet, hg_get_fleet, hg_fleet_constants,
HeliVecEnv.set_fleet / get_fleet, sample_fleet, ShardedHeliVecEnv.set_fleet's tile slicing): the symbols are
exported and declared with the header's argument counts; each call refuses a NULL env and the bad arguments
that need no handle; the wrappers validate before any library call; a class's constant image is bytewise
hg_debug_params of the config with the airframe swapped; sample_fleet is a function of its seed, stays inside
its spread and keeps the base as class 0.  No device calls."""
import ctypes

import numpy as np
import pytest

import golden_cases as gc
from test_branch_host import _bare_env
from test_policy_host import header_arg_counts

import heligym_amd
from heligym_amd import _abi, config, sample_fleet
from heligym_amd.distributed import fleet_shard_tiles
from heligym_amd.vector import FLEET_SPREAD, fleet_arrays

NEW = {"hg_set_fleet": 7, "hg_get_fleet": 5, "hg_fleet_constants": 6}
A16 = 0x10000   # a stand-in for a device pointer: never dereferenced


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _refused(lib, rc, text):
    assert rc == -1, (rc, text)
    assert text.encode() in lib.hg_last_error(), (lib.hg_last_error(), text)


def test_fleet_symbols_exported_and_declared(lib):
    counts = header_arg_counts()
    assert counts["hg_rollout_policy"] == 11   # (the parser reads a known prototype right)
    for name, n in NEW.items():
        assert hasattr(lib, name), name
        assert name in _abi.EXPORTED_SYMBOLS
        assert counts[name] == n, (name, counts.get(name))
        assert len(_abi._SIGS[name][1]) == n, name
    assert lib.hg_abi_version() == 3 == _abi.HG_ABI_VERSION   # purely additive
    assert "sample_fleet" in heligym_amd.__all__ and hasattr(heligym_amd, "sample_fleet")
    for name in ("set_fleet", "get_fleet"):
        assert callable(getattr(heligym_amd.HeliVecEnv, name))
    from heligym_amd.distributed import ShardedHeliVecEnv
    assert callable(ShardedHeliVecEnv.set_fleet)


def _params_size(lib, cfg):
    for size in range(256, 8192, 4):   # hg_debug_params accepts only sizeof(Params<float>)
        b = (ctypes.c_char * size)()
        if lib.hg_debug_params(ctypes.byref(cfg), 1024, 1024, 0, b, size) == 0:
            return size
    raise AssertionError("sizeof(Params<float>) not found")


def test_every_call_refuses_a_null_env_and_bad_arguments(lib):
    cfg, _ = config.make_config()
    af = (_abi.hg_airframe * 1)(cfg.af)
    tiles = (ctypes.c_int32 * 1)(0)
    status = (ctypes.c_int32 * 1)(-99)
    _refused(lib, lib.hg_set_fleet(None, af, None, 1, tiles, status, None), "env is NULL")
    _refused(lib, lib.hg_set_fleet(None, None, None, 0, None, None, None), "env is NULL")
    assert status[0] == -99   # outputs untouched
    n = ctypes.c_int32(-5)
    _refused(lib, lib.hg_get_fleet(None, ctypes.byref(n), tiles, af, A16), "env is NULL")
    assert n.value == -5
    size = _params_size(lib, cfg)
    out = (ctypes.c_char * size)()
    _refused(lib, lib.hg_fleet_constants(None, af, 1024, 1024, out, size), "hg_fleet_constants: bad arguments")
    _refused(lib, lib.hg_fleet_constants(ctypes.byref(cfg), None, 1024, 1024, out, size), "hg_fleet_constants: bad arguments")
    _refused(lib, lib.hg_fleet_constants(ctypes.byref(cfg), af, 1024, 1024, None, size), "hg_fleet_constants: bad arguments")
    for wrong in (size - 4, size + 4, 0):
        _refused(lib, lib.hg_fleet_constants(ctypes.byref(cfg), af, 1024, 1024, out, wrong), "hg_fleet_constants: bad arguments")
    assert lib.hg_fleet_constants(ctypes.byref(cfg), af, 1024, 1024, out, size) == 0


def test_wrappers_validate_before_any_library_call():
    N = 64 * 4 + 19   # 5 tiles
    env = _bare_env(N)
    env.cfg, _ = config.make_config()
    docs = sample_fleet(3)
    bad = [dict(tile_class=None, envs_per_class=None),                   # neither
           dict(tile_class=[0, 1, 2, 1, 0], envs_per_class=128),         # both
           dict(tile_class=[0, 1, 2, 1]),                                # one entry short
           dict(tile_class=np.zeros((5, 1), dtype=np.int32)),            # not 1-d
           dict(tile_class=[0, 1, 3, 1, 0]),                             # class out of range
           dict(tile_class=[0, -1, 2, 1, 0]),
           dict(tile_class=[0.0, 1.0, 2.0, 1.0, 0.0]),                   # not integers
           dict(envs_per_class=100), dict(envs_per_class=0), dict(envs_per_class=64.5),
           dict(envs_per_class=64)]                                      # 5 blocks for 3 classes
    for kw in bad:
        with pytest.raises(ValueError, match="set_fleet"):
            env.set_fleet(docs, **kw)
    with pytest.raises(ValueError, match="set_fleet"):
        env.set_fleet("aw109", tile_class=[0] * 5)                       # not a list
    with pytest.raises(ValueError, match="set_fleet"):
        env.set_fleet([], tile_class=[0] * 5)
    with pytest.raises(ValueError, match="set_fleet"):
        env.set_fleet(sample_fleet(6), tile_class=[0, 1, 2, 3, 4])       # more classes than tiles
    with pytest.raises(ValueError, match="trim conditions"):
        env.set_fleet(docs, tile_class=[0, 1, 2, 1, 0], conds=[{}] * 2)
    import copy
    nan_doc = copy.deepcopy(docs[1])
    nan_doc["airframe"]["WT"] = float("nan")
    with pytest.raises(ValueError, match="class 1: WT is not finite"):
        env.set_fleet([docs[0], nan_doc, docs[2]], tile_class=[0, 1, 2, 1, 0])
    with pytest.raises(KeyError):
        env.set_fleet([{"WT": 1.0}], tile_class=[0] * 5)                 # an airframe with fields missing
    # what the library would be given
    arr, tc = fleet_arrays(docs, N, tile_class=[0, 1, 2, 1, 0])
    assert len(arr) == 3 and tc.dtype == np.int32 and tc.tolist() == [0, 1, 2, 1, 0]
    assert arr[0].WT == 5401.0 and arr[1].WT == docs[1]["airframe"]["WT"] and arr[2].env_TURB_LVL == 1
    arr, tc = fleet_arrays(["aw109", docs[1]], 64 * 4, envs_per_class=128)
    assert tc.tolist() == [0, 0, 1, 1] and arr[0].mr_RPM == 385.0
    arr, tc = fleet_arrays(docs, 64 * 5 + 1, envs_per_class=128)         # a ragged last block is a class of its own
    assert tc.tolist() == [0, 0, 1, 1, 2, 2]


def test_sharded_tile_slices():
    assert fleet_shard_tiles(1024, 0, 512) == (0, 8)
    assert fleet_shard_tiles(1024, 512, 512) == (8, 16)
    assert fleet_shard_tiles(1000, 512, 488) == (8, 16)      # the last shard may end inside a tile
    for total, off, cnt in ((1000, 0, 500), (1000, 500, 500), (1024, 32, 64)):
        with pytest.raises(ValueError, match="set_fleet"):
            fleet_shard_tiles(total, off, cnt)


@pytest.mark.parametrize("name", ["heavy", "wing"])
@pytest.mark.parametrize("task,dt", [("hover", 0.01), ("forward_flight", 0.02)])
def test_fleet_constants_bytewise_equal_debug_params_of_the_swapped_config(lib, name, task, dt):
    """hg_fleet_constants(cfg of the default airframe, the variant's airframe) against hg_debug_params of a
    config made for the variant with the same run-time fields: every byte of Params<float>."""
    doc = gc.load_variant(name)[1]
    kw = dict(task=task, dt=dt, max_time=23.0, max_episode_steps=150, autoreset_mode="next_step", seed=9,
              target={"sea_alt": 3500.0, "vel": 80.0})
    own, _ = config.make_config(**kw)
    swapped, _ = config.make_config(heli_name=doc, **kw)
    size = _params_size(lib, own)
    got, want, base = ((ctypes.c_char * size)() for _ in range(3))
    assert lib.hg_fleet_constants(ctypes.byref(own), ctypes.byref(swapped.af), 1024, 1024, got, size) == 0
    assert lib.hg_debug_params(ctypes.byref(swapped), 1024, 1024, 0, want, size) == 0
    assert lib.hg_debug_params(ctypes.byref(own), 1024, 1024, 0, base, size) == 0
    assert bytes(got) == bytes(want)
    assert bytes(got) != bytes(base)   # the variant does change the constants
    # a class that is the handle's own airframe is the handle's own image
    assert lib.hg_fleet_constants(ctypes.byref(own), ctypes.byref(own.af), 1024, 1024, got, size) == 0
    assert bytes(got) == bytes(base)


def test_sample_fleet_is_deterministic_in_range_and_class_0_is_the_base():
    a, b, c = sample_fleet(200, seed=3), sample_fleet(200, seed=3), sample_fleet(200, seed=4)
    base = config.load_airframe("aw109")
    assert a == b and a != c
    assert a[0] == base and c[0] == base
    assert sample_fleet(5, seed=3) == a[:5]   # a class does not depend on how many are drawn
    assert sorted(FLEET_SPREAD) == sorted(["WT", "IX", "IY", "IZ", "FS_CG", "mr_RPM", "tr_RPM"])
    for k, s in FLEET_SPREAD.items():
        f = np.array([d["airframe"][k] / base["airframe"][k] for d in a[1:]])
        assert f.min() >= 1 - s and f.max() <= 1 + s and f.max() - f.min() > 1.6 * s, k
    for k in base["airframe"]:
        if k not in FLEET_SPREAD:
            assert all(d["airframe"][k] == base["airframe"][k] for d in a), k
    heavy = gc.load_variant("heavy")[1]
    d = sample_fleet(50, base=heavy, spread={"WT": 0.5, "mr_R": 0.0}, seed=1)
    assert d[0] == heavy
    w = np.array([x["airframe"]["WT"] for x in d[1:]]) / heavy["airframe"]["WT"]
    assert w.min() >= 0.5 and w.max() <= 1.5 and all(x["airframe"]["mr_R"] == heavy["airframe"]["mr_R"] for x in d)
    assert all(x["airframe"]["IX"] == heavy["airframe"]["IX"] for x in d)
    for bad in (dict(n_classes=0), dict(n_classes=2, spread={"WT": 1.0}), dict(n_classes=2, spread={"nope": 0.1}),
                dict(n_classes=2, spread={"env_WIND_SPD": 0.1}), dict(n_classes=2, spread={"WT": float("nan")})):
        with pytest.raises(ValueError, match="sample_fleet"):
            sample_fleet(**bad)
