"""Time of hg_rollout_stats against the torch route it replaces and against a bare copy of the observations.

At each size (65 536 envs x 100 steps and 4 096 x 64 by default) one actor-critic rollout of hover envs with a
37-step TimeLimit (so that episodes end) provides the inputs; then, on those buffers:

  (a) HeliVecEnv.rollout_stats with every output: moments, scales, scaled rewards, obs_in, episode statistics;
  (b) the same quantities as torch ops: var_mean over the [K N, 17] rows and a Chan merge into running
      moments, a K-step loop for the discounted return and the per-env episode accumulators, var_mean of the
      return samples and its merge, the two shift copies, the reward scaling;
  (c) a bare copy_ of obs into obs_in: the same observation bytes read and written once, the floor;
  (gae) hg_gae on the same rollout, another one-lane-per-env pass, for its achieved bandwidth.

Each is captured into one hipGraph (--calls calls) between two hg_clock_stamp kernels; a replay's time is the
stamps' difference (GPU 100 MHz clock).  Every variant is warmed by one untimed replay; the figure is the
median of --repeats replays, the variants alternating.  Bytes are the algorithm's, from the shapes.  Writes one
JSON document (--out) and prints it.

usage: python scripts/bench_rollout_stats.py [--sizes 65536x100,4096x64] [--repeats 7] [--out FILE]
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


def measure(torch, N, K, calls, repeats, gamma):
    from heligym_amd import HeliVecEnv, RolloutStats
    dev = "cuda:0"
    f32, f64 = torch.float32, torch.float64
    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, autoreset_mode="same_step", max_episode_steps=37,
                     device=dev, seed=1)
    lib = env.lib
    torch.manual_seed(0)
    nn = torch.nn
    model = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    obs0 = env.reset()[0].clone()
    env.set_policy(model, log_std=torch.full((4,), -1.0, device=dev), obs_mean=obs0.mean(0).contiguous(),
                   obs_scale=torch.ones(17, device=dev))
    env.set_value_head(nn.Linear(64, 1).to(dev))
    out = env.rollout_actor_critic(K, gamma, 0.95, obs0=obs0)
    obs, rew, term, trunc, info = (out[k] for k in ("obs", "reward", "terminated", "truncated", "info"))
    obs_in = torch.empty((K, N, 17), dtype=f32, device=dev)
    rew_out = torch.empty((K, N), dtype=f32, device=dev)
    stats = RolloutStats(env)

    # (b)'s persistent state
    t_mean, t_m2, t_n = torch.zeros(17, dtype=f64, device=dev), torch.zeros(17, dtype=f64, device=dev), \
        torch.zeros((), dtype=f64, device=dev)
    r_mean, r_m2, r_n = (torch.zeros((), dtype=f64, device=dev) for _ in range(3))
    G = torch.zeros(N, dtype=f32, device=dev)
    ep_ret, ep_len = torch.zeros(N, dtype=f32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    Gs = torch.empty((K, N), dtype=f32, device=dev)
    agg = torch.zeros(6, dtype=f64, device=dev)   # episodes, sum return, sum return^2, sum length, terminated, success
    t_scale, t_rscale = torch.empty(17, dtype=f32, device=dev), torch.empty((), dtype=f32, device=dev)

    def chan(n, mean, m2, nb, mean_b, m2_b):
        tot = n + nb
        delta = mean_b - mean
        mean.add_(delta * (nb / tot))
        m2.add_(m2_b + delta * delta * (n * nb / tot))
        n.copy_(tot)

    def run_b():
        rows = obs.view(K * N, 17)
        var, mean = torch.var_mean(rows, dim=0, unbiased=False)
        chan(t_n, t_mean, t_m2, float(K * N), mean.double(), var.double() * (K * N))
        done = (term | trunc) != 0
        keep = (~done).to(f32)
        agg.zero_()
        G_, er, el = G, ep_ret, ep_len
        for k in range(K):
            G_ = torch.add(rew[k], G_, alpha=gamma, out=Gs[k])
            er = er + rew[k]
            el = el + 1
            d = done[k]
            agg[0] += d.sum()
            agg[1] += (er * d).sum()
            agg[2] += (er * er * d).sum()
            agg[3] += (el * d).sum()
            agg[4] += (term[k] != 0).sum()
            agg[5] += ((info[k] & 2) != 0).logical_and(d).sum()
            G_ = G_ * keep[k]
            er = er * keep[k]
            el = el * (~d)
        G.copy_(G_)
        ep_ret.copy_(er)
        ep_len.copy_(el)
        var, mean = torch.var_mean(Gs.view(-1), unbiased=False)
        chan(r_n, r_mean, r_m2, float(K * N), mean.double(), var.double() * (K * N))
        torch.rsqrt((t_m2 / t_n + 1e-8).float(), out=t_scale)
        torch.rsqrt((r_m2 / r_n + 1e-8).float(), out=t_rscale)
        torch.clamp(rew * t_rscale, -10.0, 10.0, out=rew_out)
        obs_in[0].copy_(obs0)
        obs_in[1:].copy_(obs[:-1])

    def run_a():
        env.rollout_stats(stats, out, gamma=gamma, obs0=obs0, obs_in=obs_in, reward_out=rew_out, clip_reward=10.0)

    def run_c():
        obs_in.copy_(obs)

    def run_gae():
        env.gae(rew, out["value"], out["next_value"], term, trunc, gamma, 0.95, out=(out["advantages"], out["returns"]))

    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    variants = {"a_hg_rollout_stats": run_a, "b_torch_route": run_b, "c_bare_copy": run_c, "hg_gae_alone": run_gae}
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
            for _ in range(calls):
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
            times[name].append(float(t[1] - t[0]) * 1e-2 / calls)   # 100 MHz ticks -> us per call
    rows = K * N
    nbytes = {"a_hg_rollout_stats": rows * (68 + 68 + 4 + 3) + rows * 8 + N * (68 + 24),   # pass + scaling + obs0, per-env
              "c_bare_copy": rows * 136, "hg_gae_alone": rows * (3 * 4 + 2 + 2 * 4)}
    us = {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()}
    a, b, c = (us[k] for k in ("a_hg_rollout_stats", "b_torch_route", "c_bare_copy"))
    m = stats.moments()
    e = stats.episode_dict()
    res = {"envs": N, "steps": K, "calls_per_graph": calls, "us_per_call": us,
           "algorithm_bytes": nbytes,
           "achieved_GB_per_s": {k: nbytes[k] / us[k]["median"] * 1e-3 for k in nbytes},
           "ratio_b_over_a": b["median"] / a["median"], "ratio_a_over_c": a["median"] / c["median"],
           "a_faster_than_b_by_more_than_either_spread": bool(b["min"] - a["max"] > max(a["max"] - a["min"], b["max"] - b["min"])),
           "check": {"episodes_last_call": e["episodes"], "return_mean": e["return_mean"], "length_mean": e["length_mean"],
                     "truncated": e["truncated"], "obs_count": m["obs_count"], "skipped_rows": m["skipped_rows"],
                     "torch_obs_mean_max_abs_diff": float((t_mean - stats.head[1:18]).abs().max()),
                     "torch_episodes_last_call": float(agg[0])}}
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536x100,4096x64", help="comma-separated ENVSxSTEPS")
    ap.add_argument("--calls", type=int, default=3, help="calls per graph")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_stats.json"))
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    sizes = [tuple(int(x) for x in s.split("x")) for s in args.sizes.split(",")]
    res = {"config": {"task": "hover", "dt": 0.01, "autoreset": "same_step", "max_episode_steps": 37, "gamma": args.gamma,
                      "repeats": args.repeats, "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per call",
           "sizes": [measure(torch, n, k, args.calls, args.repeats, args.gamma) for n, k in sizes]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
