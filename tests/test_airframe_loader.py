"""Generic airframe / terrain loading: documents in the reference's schema
(ENV / HELI / HELI.{MR,TR,FUS,HT,VT,WN,LG}, heligym/envs/helis/aw109.yaml) and in this package's
flat schema give the same hg_config; terrain from PNG / npz / arrays.  CPU only."""
import ctypes
import os

import numpy as np
import pytest
import yaml

from heligym_amd import _abi, config

REF_YAML = "/root/reference/heligym/envs/helis/aw109.yaml"
REF_RES = "/root/reference/heligym/envs/renderer/resources"


def _to_reference_schema(doc):
    af = doc["airframe"]
    env = {src: af[dst] for src, dst in config._REF_ENV_KEYS.items()}
    env["HMAP_PATH"] = "/models/terrain/terrain_hmap.png"
    heli = {}
    for k, v in af.items():
        for sec, pre in config._REF_SECTIONS.items():
            if k.startswith(pre):
                heli.setdefault(sec, {})[k[len(pre):]] = v
                break
        else:
            if not k.startswith("env_"):
                heli[k] = v
    return {"ENV": env, "HELI": heli}


def _cfg_fields(cfg):
    return {n: getattr(cfg.af, n) for n, _ in _abi.hg_airframe._fields_ if n != "_pad0"}


def test_reference_schema_round_trip(tmp_path):
    ours = config.load_airframe("aw109")
    p = tmp_path / "aw109_ref_schema.yaml"
    p.write_text(yaml.safe_dump(_to_reference_schema(ours)))
    doc = config.load_airframe(str(p))
    assert doc["airframe"] == {k: v for k, v in ours["airframe"].items()}
    a, _ = config.make_config(heli_name=str(p))
    b, _ = config.make_config()
    assert _cfg_fields(a) == _cfg_fields(b)
    np.testing.assert_array_equal(config.load_terrain(doc), config.load_terrain(ours))


@pytest.mark.skipif(not os.path.exists(REF_YAML), reason="reference checkout not present")
def test_reference_airframe_file_and_terrain_png():
    """The reference's own parameter file and heightmap PNG load to the bundled values."""
    doc = config.load_airframe(REF_YAML, resource_dir=REF_RES)
    ours = config.load_airframe("aw109")
    for k, v in ours["airframe"].items():
        assert float(doc["airframe"][k]) == float(v), k
    np.testing.assert_array_equal(config.load_terrain(doc), config.load_terrain(ours))


def test_reference_layout_file_and_terrain_png(tmp_path):
    """A parameter file and a 16-bit heightmap PNG laid out as the reference lays them out (the
    document's ENV.HMAP_PATH under a resource directory) load to the bundled values, the terrain
    from the PNG itself.  Both files are written here from the bundled data, so this covers the
    resource-directory and PNG paths of the loader wherever the suite runs; the comparison with
    independent data is test_reference_airframe_file_and_terrain_png's."""
    from PIL import Image
    ours = config.load_airframe("aw109")
    u16 = config.load_terrain(ours)
    res = tmp_path / "resources"
    png = res / "models" / "terrain" / "terrain_hmap.png"
    png.parent.mkdir(parents=True)
    Image.fromarray(u16).save(str(png))
    p = tmp_path / "helis" / "aw109.yaml"
    p.parent.mkdir()
    p.write_text(yaml.safe_dump(_to_reference_schema(ours)))
    doc = config.load_airframe(str(p), resource_dir=str(res))
    assert doc["terrain"]["file"] == str(png)
    assert set(doc["airframe"]) == set(ours["airframe"])
    for k, v in ours["airframe"].items():
        assert float(doc["airframe"][k]) == float(v), k
    got = config.load_terrain(doc)
    assert got.dtype == np.uint16 and got.shape == u16.shape
    np.testing.assert_array_equal(got, u16)


def test_missing_fields_are_reported(tmp_path):
    ref = _to_reference_schema(config.load_airframe("aw109"))
    del ref["HELI"]["MR"]["RPM"]
    with pytest.raises(ValueError, match="mr_RPM"):
        config.airframe_from_reference_schema(ref)


def test_other_airframe_and_flat_terrain_trim():
    """A heavier airframe over a flat 1000 ft terrain trims (host) with more collective and the
    commanded ground altitude."""
    lib = _abi.load_library()
    doc = config.load_airframe("aw109")
    heavy = {"airframe": dict(doc["airframe"], WT=6200.0), "terrain": doc["terrain"]}
    res = {}
    for name, d in (("base", doc), ("heavy", heavy)):
        cfg, _ = config.make_config(heli_name=d)
        flat = np.full((256, 256), 1000.0)
        r = _abi.hg_trim_result()
        w = (ctypes.c_double * 3)(cfg.af.env_WIND_SPD * np.cos(np.radians(45)), cfg.af.env_WIND_SPD * np.sin(np.radians(45)), 0)
        _abi.check(lib.hg_trim(ctypes.byref(cfg), flat.ctypes.data, 256, 256, w, ctypes.byref(r)), lib)
        res[name] = r
        assert abs(r.obs[16] - (100.0 + cfg.af.WL_CG / 12)) < 1e-3   # CG height: gr_alt + WL_CG (helicopter_dynamics.py:506)
        assert abs(r.state[17] + (1000.0 + cfg.af.WL_CG / 12 + 100.0)) < 1e-2
    assert res["heavy"].action[0] > res["base"].action[0] + 0.01
