"""What per-env goals (HeliVecEnv.set_goals) cost a step and an actor-critic rollout.

Method of bench_weather.py: hover envs, dt 0.01, same-step auto-reset, every handle aged with random actions;
each variant is captured into one hipGraph between two hg_clock_stamp kernels, a replay's time is the stamps'
difference (GPU 100 MHz clock) per step captured; one untimed replay, then the median of --repeats replays with the
variants alternating.  Every handle has per-env reset templates (the shared template's rows), so each runs an
optional-features kernel:

  plain           hg_step on a plain handle: the parent commit's optional-features kernel, byte for byte;
  table_abs       a goal table (sample_goals around the start), absolute observations;
  table_rel       the same table, relative observations;
  plain_tl / box_rel_tl   a plain handle and a box handle (relative) under a TimeLimit of --timelimit steps with
                  staggered step counters, so that every launch resets 1 / timelimit of the envs (the box handle
                  draws and stores their goals).

Per size in --envs; at --rollout-envs also rollout_actor_critic(K) for the same variants.  Writes one JSON document
(--out) and prints it.

usage: python scripts/bench_goals.py [--envs 4096 65536 262144] [--rollout-envs 65536] [--steps 100] [--repeats 7]
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

BOX = dict(north_loc=(-200.0, 200.0), east_loc=(-200.0, 200.0), sea_alt=(1546.0, 1746.0))


def bench_size(torch, N, K, repeats, aged, timelimit, with_rollout):
    from heligym_amd import HeliVecEnv, sample_goals
    dev, dt = "cuda:0", 0.01
    kw = dict(task="hover", dt=dt, autoreset=True, autoreset_mode="same_step", device=dev, seed=1)
    envs = {"plain": HeliVecEnv(N, **kw), "table_abs": HeliVecEnv(N, **kw), "table_rel": HeliVecEnv(N, **kw),
            "plain_tl": HeliVecEnv(N, max_episode_steps=timelimit, **kw),
            "box_rel_tl": HeliVecEnv(N, max_episode_steps=timelimit, **kw)}
    first = envs["plain"]
    lib = first.lib
    tm = first.get_weather()["templates"]   # the shared template, one row per env
    for env in envs.values():
        env._check(lib.hg_set_reset_templates(env._h, ctypes.c_void_p(tm.data_ptr()), env._stream()))
    goals = sample_goals(N, "hover", around=dict(north_loc=0.0, east_loc=0.0, sea_alt=1646.0), seed=2)
    envs["table_abs"].set_goals(goals=goals)
    envs["table_rel"].set_goals(goals=goals, relative=True)
    envs["box_rel_tl"].set_goals(box=BOX, relative=True)
    B = 16
    bank = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    for k in range(B):
        first.random_actions(bank[k], seed=4, step=k)
    for name, env in envs.items():
        env.reset()
        for k in range(aged):
            env.step_async(bank[k % B], with_reset_info=False)
        if name.endswith("_tl"):   # staggered step counters: every launch resets 1 / timelimit of the envs
            st, ctr = env.get_state()
            ctr = ctr.clone()
            ctr[:, 0] = (torch.arange(N, device=dev) % timelimit).to(torch.int32)
            env.set_state(st, ctr)
    torch.cuda.synchronize()
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), first._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    def steps(env):
        def run():
            for k in range(K):
                env.step_async(bank[k % B], with_reset_info=False)
        return run

    variants = {"step_" + name: steps(env) for name, env in envs.items()}
    if with_rollout:
        torch.manual_seed(0)
        nn = torch.nn
        model = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
        log_std = torch.full((4,), -1.0, device=dev)
        head = nn.Linear(64, 1).to(dev)
        cur, outs = {}, {}

        def rollout(name, env):
            def run():
                env.rollout_actor_critic(K, obs0=cur[name], out=outs[name])
                cur[name].copy_(outs[name]["obs"][K - 1])
            return run
        for name, env in envs.items():
            mean = env.obs.mean(0).contiguous()
            scale = (1.0 / env.obs.std(0).clamp_min(1e-3)).contiguous()
            env.set_policy(model, log_std=log_std, obs_mean=mean, obs_scale=scale)
            env.set_value_head(head)
            cur[name] = env.obs.clone()
            outs[name] = env.rollout_actor_critic(K, obs0=cur[name])   # (allocates the buffers; an untimed warm-up)
            cur[name].copy_(outs[name]["obs"][K - 1])
            variants["rollout_ac_" + name] = rollout(name, env)
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
    res = {"envs": N,
           "us_per_step": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()},
           "launches": {name: env.debug_launches() for name, env in envs.items()},
           "outputs_finite": all(bool(torch.isfinite(env.obs).all()) for env in envs.values())}
    for env in envs.values():
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--rollout-envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100, help="K: steps per graph, and per rollout call")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--age-seconds", type=float, default=20.0)
    ap.add_argument("--timelimit", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goals.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X"
    aged = int(round(args.age_seconds / 0.01))
    res = {"config": {"task": "hover", "dt": 0.01, "autoreset": "same_step", "steps_per_graph": args.steps,
                      "aged_steps": aged, "repeats": args.repeats, "timelimit": args.timelimit, "box": BOX,
                      "goals": "sample_goals(envs, 'hover', around the start, seed=2)",
                      "policy": "MLP 17-64-64-4 tanh fp32, log_std -1, value head", "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per step of all the envs",
           "sizes": [bench_size(torch, n, args.steps, args.repeats, aged, args.timelimit, n == args.rollout_envs)
                     for n in args.envs]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
