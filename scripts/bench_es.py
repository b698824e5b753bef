"""Time of one evolution-strategies generation on the device against its floor and the route it replaces.

65 536 hover envs, dt 0.01, turbulence on, same-step auto-reset, aged 60 simulated seconds with random
actions (as bench.py ages its headline population).  Population P = 1 024 members x 64 envs, K = 100 steps:

  (a) one generation through the population calls: hg_es_perturb (images from counters), hg_rollout_pop,
      hg_pop_fitness, hg_es_grad (three launches), hg_ppo_adam;
  (b) the floor: the bare hg_rollout_policy of the same envs and K (one policy for all envs);
  (c) the route (a) replaces: a loop over --loop-members handles of 64 envs each, per member
      hg_set_policy_theta + hg_rollout_policy of K steps; reported per member, and scaled to P members;
  (d) (a) without its rollout: what the ES kernels themselves cost.

Each is captured into one hipGraph between two hg_clock_stamp kernels; a replay's time is the stamps'
difference (GPU 100 MHz clock).  Every variant is warmed by one untimed replay; the figure is the median
of --repeats replays, the variants alternating.  Writes one JSON document (--out) and prints it.

usage: python scripts/bench_es.py [--envs 65536] [--members 1024] [--steps 100] [--repeats 7] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "heli-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--members", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100, help="K: steps per generation")
    ap.add_argument("--loop-members", type=int, default=32, help="handles of 64 envs in variant (c)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--age-seconds", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "es_generation.json"))
    args = ap.parse_args()

    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv, PPOOptState
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    N, P, K, dt = args.envs, args.members, args.steps, 0.01
    epm = N // P
    assert epm * P == N and epm % 64 == 0, "envs must be members x a multiple of 64"
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
    del bank

    torch.manual_seed(0)
    nn = torch.nn
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
    cpu = ActorCriticParams(actor, nn.Linear(64, 1), torch.full((4,), -1.0))
    params = types.SimpleNamespace(theta=cpu.theta.detach().to(dev), grad=torch.zeros(5641, device=dev))
    state = PPOOptState(dev)
    mean = env.obs.mean(0).contiguous()
    scale = (1.0 / env.obs.std(0).clamp_min(1e-3)).contiguous()
    env.set_policy_theta(params, obs_mean=mean, obs_scale=scale)

    f32, u8 = torch.float32, torch.uint8
    out = (torch.empty((K, N, 4), dtype=f32, device=dev), torch.empty((K, N, 17), dtype=f32, device=dev),
           torch.empty((K, N), dtype=f32, device=dev), torch.empty((K, N), dtype=u8, device=dev),
           torch.empty((K, N), dtype=u8, device=dev), torch.empty((K, N), dtype=u8, device=dev))
    images = torch.empty((P, 7552), dtype=f32, device=dev)
    sums = torch.zeros((P,), dtype=torch.float64, device=dev)
    fitness = torch.zeros((P,), dtype=f32, device=dev)
    alive = torch.ones((N,), dtype=u8, device=dev)
    es_stats = torch.zeros((8,), dtype=f32, device=dev)
    gen_dev = state.tail[0:1]
    sigma, seed, lr = 0.05, 7, 1e-2
    env._es_workspace(P)
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    # (c): small handles, their member parameter vectors from the same perturbation
    Pc = args.loop_members
    member_theta = torch.empty((P, 5641), dtype=f32, device=dev)
    env.es_perturb(params, P, sigma, seed, obs_mean=mean, obs_scale=scale, out=images, member_theta=member_theta)
    small = [HeliVecEnv(64, task="hover", dt=dt, autoreset=True, autoreset_mode="same_step", device=dev, seed=1,
                        env_offset=64 * p) for p in range(Pc)]
    for e in small:
        e.reset()
    members = [types.SimpleNamespace(theta=member_theta[p]) for p in range(Pc)]
    outs_c = [tuple(torch.empty((K, 64) + x.shape[2:], dtype=x.dtype, device=dev) for x in out) for _ in range(Pc)]

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    def es_kernels_before():
        env.es_perturb(params, P, sigma, seed, gen_dev=gen_dev, obs_mean=mean, obs_scale=scale, out=images)

    def es_kernels_after():
        env.pop_fitness(out[2], out[3], out[4], P, epm, sums, mode="window", restart=True, alive=alive, out=fitness)
        env.es_grad(params, fitness, sigma, seed, gen_dev=gen_dev, stats=es_stats)
        env.ppo_adam(params, state, lr=lr)

    def run_a():
        es_kernels_before()
        env.rollout_population(K, images, epm, obs0=out[1][K - 1], out=out)
        es_kernels_after()

    def run_b():
        env.rollout_policy(K, obs0=out[1][K - 1], out=out)

    def run_c():
        for e, m, o in zip(small, members, outs_c):
            e.set_policy_theta(m, obs_mean=mean, obs_scale=scale)
            e.rollout_policy(K, obs0=o[1][K - 1], out=o)

    def run_d():
        es_kernels_before()
        es_kernels_after()

    variants = {"a_es_generation": run_a, "b_rollout_policy_floor": run_b, "c_loop_over_handles": run_c,
                "d_es_kernels_only": run_d}
    out[1][K - 1].copy_(env.obs)
    for e, o in zip(small, outs_c):
        o[1][K - 1].copy_(e.obs)
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in variants.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # eager warm-up on the capture stream (code objects)
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
    for _ in range(args.repeats):
        for name in variants:
            graphs[name].replay()
            torch.cuda.synchronize()
            t = stamps.cpu()
            times[name].append(float(t[1] - t[0]) * 1e-2)   # 100 MHz ticks -> us
    us = {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()}
    med = {n: us[n]["median"] for n in us}
    counters = state.counters()
    res = {"config": {"envs": N, "members": P, "envs_per_member": epm, "task": "hover", "dt": dt,
                      "turbulence": "on (default level)", "autoreset": "same_step", "steps": K, "aged_steps": aged,
                      "repeats": args.repeats, "loop_members": Pc, "sigma": sigma,
                      "policy": "MLP 17-64-64-4 tanh fp32, log_std -1", "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per replay",
           "us": us,
           "us_per_step_a": med["a_es_generation"] / K,
           "us_per_step_b": med["b_rollout_policy_floor"] / K,
           "es_overhead_us": med["a_es_generation"] - med["b_rollout_policy_floor"],
           "es_overhead_fraction_of_b": (med["a_es_generation"] - med["b_rollout_policy_floor"]) / med["b_rollout_policy_floor"],
           "c_us_per_member": med["c_loop_over_handles"] / Pc,
           "c_scaled_to_all_members_us": med["c_loop_over_handles"] / Pc * P,
           "ratio_c_scaled_over_a": med["c_loop_over_handles"] / Pc * P / med["a_es_generation"],
           "env_steps_per_s_a": N * K / (med["a_es_generation"] * 1e-6),
           "adam_steps_applied": counters["applied"], "adam_steps_skipped_nonfinite": counters["skipped_nonfinite"],
           "fitness_finite": bool(torch.isfinite(fitness).all()), "stats_row": [float(v) for v in es_stats.cpu()]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    for e in small:
        e.close()
    env.close()


if __name__ == "__main__":
    main()
