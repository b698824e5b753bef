"""What a mixed fleet (HeliVecEnv.set_fleet) costs a step and a policy rollout.

Method of bench_weather.py: hover envs, dt 0.01, same-step auto-reset, every handle aged with random actions;
each arm is captured into one hipGraph between two hg_clock_stamp kernels, a replay's time is the stamps'
difference (GPU 100 MHz clock) per step captured; one untimed replay, then the median of --repeats replays with
the arms interleaved.  One handle per arm (a captured graph holds its handle's table pointer), same seed:

  (a)  the generic kernel: set_specialized(False), no fleet;
  (a2) a second handle like (a): the A/B's own spread is |a - a2|;
  (b)  a fleet of 1 class (the handle's own airframe): (a)'s code plus the class load and per-env templates;
  (c)  3 classes (aw109 and two sample_fleet draws), tiles round-robin;
  (d)  one class per tile from sample_fleet.

for hg_step and hg_rollout_policy at each of --envs.  Also the wall time of set_fleet for --trim-classes classes
(the host trims).  Writes one JSON document (--out) and prints it.

usage: python scripts/bench_fleet.py [--envs 4096 65536 262144] [--steps 100] [--repeats 7] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "heli-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ARMS = ("a_generic", "a2_generic_again", "b_fleet_1_class", "c_fleet_3_classes", "d_fleet_class_per_tile")


def one_size(torch, N, K, repeats, aged):
    import numpy as np
    from heligym_amd import HeliVecEnv, sample_fleet
    dev, dt = "cuda:0", 0.01
    tiles = (N + 63) // 64
    kw = dict(task="hover", dt=dt, autoreset=True, autoreset_mode="same_step", device=dev, seed=1)
    envs = {name: HeliVecEnv(N, **kw) for name in ARMS}
    for name in ARMS[:2]:
        envs[name].set_specialized(False)
    docs = sample_fleet(tiles, seed=2)
    set_fleet_s = {}
    for name, classes, tc in ((ARMS[2], docs[:1], np.zeros(tiles, dtype=np.int32)),
                              (ARMS[3], docs[:3], (np.arange(tiles) % 3).astype(np.int32)),
                              (ARMS[4], docs, np.arange(tiles, dtype=np.int32))):
        t0 = time.perf_counter()
        envs[name].set_fleet(classes, tile_class=tc)
        set_fleet_s[name] = time.perf_counter() - t0
    lib = envs[ARMS[0]].lib
    B = 16
    bank = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    for k in range(B):
        envs[ARMS[0]].random_actions(bank[k], seed=4, step=k)
    for env in envs.values():
        env.reset()
        for k in range(aged):
            env.step_async(bank[k % B], with_reset_info=False)
    torch.cuda.synchronize()
    torch.manual_seed(0)
    nn = torch.nn
    model = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    log_std = torch.full((4,), -1.0, device=dev)
    ref_obs = envs[ARMS[0]].obs
    mean = ref_obs.mean(0).contiguous()
    scale = (1.0 / ref_obs.std(0).clamp_min(1e-3)).contiguous()
    cur, outs = {}, {}
    for name, env in envs.items():
        env.set_policy(model, log_std=log_std, obs_mean=mean, obs_scale=scale)
        cur[name] = env.obs.clone()
        outs[name] = env.rollout_policy(K, obs0=cur[name])   # (allocates the buffers; an untimed warm-up)
        cur[name].copy_(outs[name][1][K - 1])
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), envs[ARMS[0]]._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    def steps(env):
        def run():
            for k in range(K):
                env.step_async(bank[k % B], with_reset_info=False)
        return run

    def rollout(name, env):
        def run():
            env.rollout_policy(K, obs0=cur[name], out=outs[name])
            cur[name].copy_(outs[name][1][K - 1])
        return run

    variants = {}
    for name, env in envs.items():
        variants["step/" + name] = steps(env)
        variants["rollout_policy/" + name] = rollout(name, env)
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in variants.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # eager warm-up on the capture stream
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            stamp(0)
            fn()
            stamp(1)
        graphs[name] = g
        g.replay()   # untimed
        torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(repeats):
        for name in variants:
            graphs[name].replay()
            torch.cuda.synchronize()
            t = stamps.cpu()
            times[name].append(float(t[1] - t[0]) * 1e-2 / K)   # 100 MHz ticks -> us per step of all N envs
    res = {"envs": N, "tiles": tiles,
           "us_per_step": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()},
           "set_fleet_seconds": set_fleet_s,
           "launches": {name: env.debug_launches() for name, env in envs.items()},
           "outputs_finite": bool(all(torch.isfinite(env.obs).all() and torch.isfinite(outs[name][1]).all()
                                      for name, env in envs.items()))}
    for call in ("step", "rollout_policy"):
        med = {a: res["us_per_step"][f"{call}/{a}"]["median"] for a in ARMS}
        res[call + "_ab_spread_us"] = abs(med[ARMS[0]] - med[ARMS[1]])
        for a in ARMS[2:]:
            res[f"{call}_{a}_minus_a_us"] = med[a] - med[ARMS[0]]
    for env in envs.values():
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--steps", type=int, default=100, help="K: steps per graph, and per rollout call")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--age-seconds", type=float, default=20.0)
    ap.add_argument("--trim-classes", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from heligym_amd import HeliVecEnv, sample_fleet
    assert torch.cuda.is_available(), "needs an MI355X"
    res = {"config": {"task": "hover", "dt": 0.01, "autoreset": "same_step", "steps_per_graph": args.steps,
                      "aged_steps": int(round(args.age_seconds / 0.01)), "repeats": args.repeats,
                      "classes": "sample_fleet(tiles, seed=2): WT, IX, IY, IZ +-15 %, FS_CG +-1 %, rotor speeds +-3 %",
                      "policy": "MLP 17-64-64-4 tanh fp32, log_std -1", "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per step of all the envs",
           "arms": list(ARMS), "sizes": []}
    for N in args.envs:
        res["sizes"].append(one_size(torch, N, args.steps, args.repeats, res["config"]["aged_steps"]))
        print(json.dumps(res["sizes"][-1]), flush=True)
    C = args.trim_classes
    env = HeliVecEnv(64 * C, task="hover", dt=0.01, device="cuda:0", seed=1)
    docs = sample_fleet(C, seed=2)
    t0 = time.perf_counter()
    env.set_fleet(docs, tile_class=np.arange(C, dtype=np.int32))
    res["set_fleet_wall_seconds"] = {"classes": C, "envs": 64 * C, "seconds": time.perf_counter() - t0}
    env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
