"""Per-step time of a closed-loop policy rollout against the open-loop rollout and the per-step loop.

65 536 hover envs, dt 0.01, turbulence on, same-step auto-reset, aged 60 simulated seconds with random
actions (as bench.py ages its headline population), then, on the same handle, K = 100 steps per call:

  (a) hg_rollout_policy: the MLP policy (17-64-64-4, tanh, Gaussian noise) evaluated in the kernel;
  (b) hg_rollout: open loop, the actions read from a bank fixed in advance;
  (c) the loop available without (a): per step hg_step_rows, then the same MLP as torch fp32 ops
      (normalise, three linear layers, two tanh) and the noise add from a pre-drawn bank of normals.

Each is captured into one hipGraph (so (c) pays no host cost per launch) between two hg_clock_stamp
kernels; a replay's time is the stamps' difference (GPU 100 MHz clock), per step = / steps captured.
Every variant is warmed by one untimed replay; the figure is the median of --repeats replays, the
variants alternating.  Writes one JSON document (--out) and prints it.

usage: python scripts/bench_policy_rollout.py [--envs 65536] [--steps 100] [--repeats 7] [--out FILE]
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
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100, help="K: steps per rollout call")
    ap.add_argument("--calls", type=int, default=5, help="rollout calls per graph for (a) and (b)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--age-seconds", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_rollout.json"))
    args = ap.parse_args()

    import torch
    from heligym_amd import HeliVecEnv
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    N, K, G, dt = args.envs, args.steps, args.calls, 0.01
    env = HeliVecEnv(N, task="hover", dt=dt, autoreset=True, autoreset_mode="same_step", device=dev, seed=1)
    lib = env.lib
    env.reset()
    B = 16
    bank = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    for k in range(B):
        env.random_actions(bank[k], seed=4, step=k)
    aged = int(round(args.age_seconds / dt))
    for k in range(aged):
        env.step_async(bank[k % B], with_reset_info=False)
    torch.cuda.synchronize()

    # the policy: torch's default init, the input normalised by the aged population's statistics
    torch.manual_seed(0)
    nn = torch.nn
    model = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    log_std = torch.full((4,), -1.0, device=dev)
    mean = env.obs.mean(0).contiguous()
    scale = (1.0 / env.obs.std(0).clamp_min(1e-3)).contiguous()
    env.set_policy(model, log_std=log_std, obs_mean=mean, obs_scale=scale)

    f32, u8 = torch.float32, torch.uint8
    out_a = (torch.empty((K, N, 4), dtype=f32, device=dev), torch.empty((K, N, 17), dtype=f32, device=dev),
             torch.empty((K, N), dtype=f32, device=dev), torch.empty((K, N), dtype=u8, device=dev),
             torch.empty((K, N), dtype=u8, device=dev), torch.empty((K, N), dtype=u8, device=dev))
    out_b = out_a[1:]
    acts_b = torch.empty((K, N, 4), dtype=f32, device=dev)
    for k in range(K):
        env.random_actions(acts_b[k], seed=5, step=k)
    z_bank = torch.randn((K, N, 4), dtype=f32, device=dev)
    std = log_std.exp()
    act_c = torch.empty((N, 4), dtype=f32, device=dev)
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    def run_a():   # each call continues from the last observation row of the one before (same buffer)
        for _ in range(G):
            env.rollout_policy(K, obs0=out_a[1][K - 1], out=out_a)

    def run_b():
        for _ in range(G):
            env.rollout(acts_b, out=out_b)

    def run_c():
        obs = env.obs
        for k in range(K):
            x = (obs - mean) * scale
            torch.addcmul(model(x), std, z_bank[k], out=act_c)
            obs = env.step(act_c)[0]

    variants = {"a_rollout_policy": (run_a, G * K), "b_rollout_open_loop": (run_b, G * K),
                "c_step_rows_torch_mlp": (run_c, K)}

    def sync_obs(name):
        """(untimed) the envs' current observations where the next variant reads them: the rollouts leave
        them in the last row of the shared obs stack, the step loop in env.obs"""
        if name == "c_step_rows_torch_mlp":
            out_a[1][K - 1].copy_(env.obs)
        else:
            env.obs.copy_(out_a[1][K - 1])
        torch.cuda.synchronize()

    graphs = {}
    side = torch.cuda.Stream()
    out_a[1][K - 1].copy_(env.obs)
    for name, (fn, _) in variants.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # eager warm-up on the capture stream (code objects, BLAS workspaces)
            fn()
        torch.cuda.current_stream().wait_stream(side)
        sync_obs(name)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            stamp(0)
            fn()
            stamp(1)
        graphs[name] = g
        g.replay()   # untimed
        sync_obs(name)

    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, (_, steps) in variants.items():
            graphs[name].replay()
            sync_obs(name)
            t = stamps.cpu()
            times[name].append(float(t[1] - t[0]) * 1e-2 / steps)   # 100 MHz ticks -> us per step
    _, ctr = env.get_state()
    res = {"config": {"envs": N, "task": "hover", "dt": dt, "turbulence": "on (default level)",
                      "autoreset": "same_step", "steps_per_call": K, "calls_per_graph_ab": G,
                      "aged_steps": aged, "repeats": args.repeats, "policy": "MLP 17-64-64-4 tanh fp32, log_std -1",
                      "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per env step",
           "us_per_step": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()},
           "episodes_begun_max": int(ctr[:, 2].max()), "actions_finite": bool(torch.isfinite(out_a[0]).all()),
           "obs_nonfinite_values": int((~torch.isfinite(out_a[1])).sum())}
    med = {n: res["us_per_step"][n]["median"] for n in times}
    res["ratio_c_over_a"] = med["c_step_rows_torch_mlp"] / med["a_rollout_policy"]
    res["ratio_a_over_b"] = med["a_rollout_policy"] / med["b_rollout_open_loop"]
    res["env_steps_per_s_a"] = N / (med["a_rollout_policy"] * 1e-6)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
