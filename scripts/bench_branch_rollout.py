"""Cost of scoring planner candidates: hg_rollout_branch against the routes that exist without it.

1 024 hover envs, dt 0.01, turbulence on, same-step auto-reset, aged 6 000 steps with random actions;
64 candidate action sequences per env (hg_mppi_sample around the trim action), horizon 50, gamma 1:
65 536 rows.  Per scoring of all candidates:

  (a) hg_rollout_branch on the 1 024-env handle;
  (b) the route without it: a second handle of 65 536 envs, get_state of the planner's envs ->
      repeat_interleave -> set_state, hg_rollout with all its outputs, then the returns in torch (the
      rewards summed up to each row's first terminated / truncated step);
  (c) the floor: a plain hg_rollout of the 65 536-env handle (no state copy, no reduction);
  (d) hg_mppi_sample + hg_mppi_update, the rest of a plan.

Method as bench_policy_rollout.py: each variant is one hipGraph between two hg_clock_stamp kernels (GPU
100 MHz clock), warmed by one untimed replay; the figure is the median of --repeats replays, the variants
alternating.  Writes one JSON document (--out) and prints it.

usage: python scripts/bench_branch_rollout.py [--envs 1024] [--branches 64] [--horizon 50] [--repeats 7] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "heli-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--branches", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--calls", type=int, default=4, help="scorings per graph")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--age-steps", type=int, default=6000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_rollout.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from heligym_amd import HeliVecEnv
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    N, M, H, G, dt = args.envs, args.branches, args.horizon, args.calls, 0.01
    R = N * M
    kw = dict(task="hover", dt=dt, autoreset=True, autoreset_mode="same_step", device=dev, seed=1)
    env = HeliVecEnv(N, **kw)
    wide = HeliVecEnv(R, **kw)
    lib = env.lib
    env.reset()
    wide.reset()
    bank = torch.empty((16, N, 4), dtype=torch.float32, device=dev)
    for k in range(16):
        env.random_actions(bank[k], seed=4, step=k)
    for k in range(args.age_steps):
        env.step_async(bank[k % 16], with_reset_info=False)
    torch.cuda.synchronize()

    trim = torch.as_tensor(np.asarray(env.template()["action"], dtype=np.float32), device=dev)
    nominal = trim.expand(H, N, 4).contiguous()
    actions = env.mppi_sample(nominal, M, 0.1, -1.0, 1.0, seed=9)
    score = env.rollout_branch(actions, M)
    new_nominal = torch.empty_like(nominal)
    f32, u8 = torch.float32, torch.uint8
    out_w = (torch.empty((H, R, 17), dtype=f32, device=dev), torch.empty((H, R), dtype=f32, device=dev),
             torch.empty((H, R), dtype=u8, device=dev), torch.empty((H, R), dtype=u8, device=dev),
             torch.empty((H, R), dtype=u8, device=dev))
    ret_b = torch.empty((R,), dtype=f32, device=dev)
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    def run_a():
        for _ in range(G):
            env.rollout_branch(actions, M, out=score)

    def run_b():
        for _ in range(G):
            s, c = env.get_state()
            wide.set_state(s.repeat_interleave(M, dim=0), c.repeat_interleave(M, dim=0))
            _, rew, term, trunc, _ = wide.rollout(actions, out=out_w)
            done = (term | trunc).to(torch.int32)
            alive = (done.cumsum(0) - done) == 0   # up to and including the first ending step
            torch.sum(rew * alive, dim=0, out=ret_b)

    def run_c():
        for _ in range(G):
            wide.rollout(actions, out=out_w)

    def run_d():
        for _ in range(G):
            env.mppi_sample(nominal, M, 0.1, -1.0, 1.0, seed=9, out=actions)
            env.mppi_update(actions, score["returns"], 0.05, out=new_nominal)

    variants = {"a_rollout_branch": run_a, "b_second_handle_expand_rollout_reduce": run_b,
                "c_plain_rollout_floor": run_c, "d_mppi_sample_update": run_d}
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

    # (b) computes what (a) computes -- same rows, same first-end cut, the sum in torch's order -- once both
    # see the same noise: the second handle's envs have ids (noise keys) of their own, so the two routes
    # can only be compared without noise (untimed)
    off = env.rollout_branch(actions, M, noise="off")["returns"].reshape(-1)
    s, c = env.get_state()
    wide.set_state(s.repeat_interleave(M, dim=0), c.repeat_interleave(M, dim=0))
    _, rew, term, trunc, _ = wide.rollout(actions, eta=torch.zeros((H, R, 3), dtype=f32, device=dev), out=out_w)
    done = (term | trunc).to(torch.int32)
    ref = (rew * ((done.cumsum(0) - done) == 0)).sum(0)
    torch.cuda.synchronize()
    agree = float(((off - ref).abs() / ref.abs().clamp_min(1.0)).max())

    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name in variants:
            graphs[name].replay()
            torch.cuda.synchronize()
            t = stamps.cpu()
            times[name].append(float(t[1] - t[0]) * 1e-2 / G)   # 100 MHz ticks -> us per scoring
    stat = {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()}
    med = {n: stat[n]["median"] for n in stat}
    res = {"config": {"envs": N, "branches": M, "rows": R, "horizon": H, "gamma": 1.0, "noise": "env", "task": "hover",
                      "dt": dt, "turbulence": "on (default level)", "autoreset": "same_step", "aged_steps": args.age_steps,
                      "scorings_per_graph": G, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per scoring of all rows (d: per sample + update)",
           "us_per_scoring": stat,
           "us_per_row_step": {n: med[n] / H for n in ("a_rollout_branch", "b_second_handle_expand_rollout_reduce",
                                                      "c_plain_rollout_floor")},
           "ratio_b_over_a": med["b_second_handle_expand_rollout_reduce"] / med["a_rollout_branch"],
           "ratio_a_over_c": med["a_rollout_branch"] / med["c_plain_rollout_floor"],
           "spread_a": (stat["a_rollout_branch"]["max"] - stat["a_rollout_branch"]["min"]) / med["a_rollout_branch"],
           "spread_c": (stat["c_plain_rollout_floor"]["max"] - stat["c_plain_rollout_floor"]["min"]) / med["c_plain_rollout_floor"],
           "row_steps_per_s_a": R * H / (med["a_rollout_branch"] * 1e-6),
           "max_rel_return_difference_a_b_noise_off": agree,
           "alive_steps_min_mean": [int(score["alive_steps"].min()), float(score["alive_steps"].float().mean())],
           "launches_planner_handle": env.debug_launches()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    env.close()
    wide.close()


if __name__ == "__main__":
    main()
