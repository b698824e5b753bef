"""GPU: a plain bench.py run (no --full) measures the headline only, times exactly --steps steps, and
--dump-outputs writes the last timed step's outputs, the same from run to run.  bench.main() runs in
this process on a small population.  Run with -m gpu."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4160          # 65 waves: no multiple of the step kernel's tile
ARGS = ["--gpus", "1", "--envs", str(N), "--steps", "25", "--warmup", "3", "--age-seconds", "2", "--graph-steps", "10"]
FULL_ONLY = ("step_with_reset_info", "step_api_eager", "generic_kernel", "airframes", "rollout", "retrim",
             "retrim_next_step", "out_of_cache", "config5", "max_abs_step_err", "cpu_baseline")
SHAPES = {"obs": (N, 17), "reward": (N,), "terminated": (N,), "truncated": (N,), "info": (N,), "state": (N, 27),
          "counters": (N, 3)}


@pytest.fixture(scope="module")
def bench():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    import bench as b
    return b


def run(bench, monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", *ARGS, *extra])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def eager_reference(bench, monkeypatch, cut):
    """The last step of the run, computed without bench.py's graphs: a second env with the same seed
    and action bank stepped eagerly through every step the run makes, in its order -- 2 s of ageing
    at dt 0.01, the warm-up, the capture stream's B steps, then per replayed window the 1 000-step
    pre-roll and the K = 25 timed steps.  An uncut window is rehearsed once whole before the timed
    one; of a cut window (10 + 10 + 5) only the middle and tail graphs are.  The bank index of a
    window's step k is k mod B, restarting at the pre-roll and at the first timed step."""
    import torch
    monkeypatch.setattr(sys, "argv", ["bench.py", *ARGS])
    args = bench.parse()
    dev = torch.device("cuda:0")
    B, K, P = 10, 25, 1000
    env = bench.make_env(args, torch, N, 0, dev)
    bank = bench.action_bank(args, torch, env, N, dev, B)
    window = [k % B for k in range(P)] + [k % B for k in range(K)]
    seq = [k % B for k in range(200)] + list(range(3)) + list(range(B))
    seq += [k % B for k in range(10, 25)] + window if cut else window + window
    for k in seq:
        env.step_async(bank[k], with_reset_info=False)
    state, counters = env.get_state()
    ref = {"obs": env.obs, "reward": env.reward, "terminated": env.terminated_u8, "truncated": env.truncated_u8,
           "state": state, "counters": counters}
    ref = {k: v.cpu().numpy() for k, v in ref.items()}
    env.close()
    return ref


def check_against(ref, d):
    for name, want in ref.items():
        got = np.load(os.path.join(d, name + ".npy"))
        assert got.shape == want.shape
        assert np.array_equal(got, want.astype(got.dtype)), name   # bitwise: the same kernel, the same inputs


def test_plain_run_dumps_the_last_step_reproducibly(bench, monkeypatch, capsys, tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        line = run(bench, monkeypatch, capsys, "--dump-outputs", d)
        assert line["steps"] == 25 and line["timing"]["repeats"] == 1 and len(line["timing"]["window_s"]) == 1
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3))
        assert line["timing"]["median_window_s"] == pytest.approx(25 * line["ms_per_step"] * 1e-3)
        assert not [k for k in FULL_ONLY if k in line]
        assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in SHAPES)
    total = 0
    for name, shape in SHAPES.items():
        a, b = (np.load(os.path.join(d, name + ".npy")) for d in dirs)
        assert a.shape == shape and a.dtype == (np.float64 if name == "counters" else np.float32)
        assert np.all(np.isfinite(a))
        assert a.tobytes() == b.tobytes(), name
        total += a.nbytes
    assert total <= bench.DUMP_BYTES_MAX
    check_against(eager_reference(bench, monkeypatch, cut=False), dirs[0])
    obs, state = (np.load(os.path.join(dirs[0], k + ".npy")) for k in ("obs", "state"))
    assert np.ptp(obs[:, 16]) > 0 and np.ptp(state[:, 17]) > 0   # an aged population, not the reset template


def test_long_window_is_cut_into_graphs(bench, monkeypatch, capsys, tmp_path):
    """A window longer than one graph's limit (HG_TG_CHUNK, here 10 steps: 10 + 10 + 5) still runs
    exactly --steps steps after its pre-roll: the dump is the eager reference's last step."""
    monkeypatch.setenv("HG_TG_CHUNK", "10")
    line = run(bench, monkeypatch, capsys, "--dump-outputs", str(tmp_path / "c"))
    assert line["steps"] == 25 and "cut into graphs of at most 10 steps" in line["config"]["workload"]
    assert line["ms_per_step"] > 0 and line["timing"]["resets_in_window"] >= 0
    # the 100 MHz stamps around 25 launches of a 4 160-env step: microseconds each, not a graph's worth of pre-roll
    assert 1e-6 < line["ms_per_step"] * 1e-3 < 1e-3
    assert np.all(np.isfinite(np.load(str(tmp_path / "c" / "obs.npy"))))
    check_against(eager_reference(bench, monkeypatch, cut=True), str(tmp_path / "c"))
