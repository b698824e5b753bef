"""What per-env weather (HeliVecEnv.set_weather) costs a step, and what the route it replaces costs.

Method of bench_actor_critic.py: hover envs, dt 0.01, same-step auto-reset, every handle aged 60 simulated
seconds with random actions; each variant is captured into one hipGraph between two hg_clock_stamp kernels, a
replay's time is the stamps' difference (GPU 100 MHz clock) per step captured; one untimed replay, then the
median of --repeats replays with the variants alternating.

  (a) hg_step on a plain handle of --envs envs (its kernels are the parent commit's, byte for byte);
  (a2) hg_step on a plain handle given the weather handle's reset templates as per-env templates
      (hg_set_reset_templates): the optional-features kernel (b) runs too, without the weather records;
  (b) hg_step on a weather handle of the same size, every env its own weather from sample_weather over the
      full ranges (turbulence 0 .. 7, wind 0 .. 40 ft/s from any side);
  (c) hg_rollout_policy(K) on both;
  (d) the route (b) replaces: W plain handles of envs / W envs, one turbulence level each, stepped in a loop.

Writes one JSON document (--out) and prints it.

usage: python scripts/bench_weather.py [--envs 65536] [--steps 100] [--handles 16] [--repeats 7] [--out FILE]
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


def give_templates(env, templates):
    return env.lib.hg_set_reset_templates(env._h, ctypes.c_void_p(templates.data_ptr()), env._stream())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100, help="K: steps per graph, and per rollout call")
    ap.add_argument("--handles", type=int, default=16, help="W: plain handles of envs / W envs in (d)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--age-seconds", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weather.json"))
    args = ap.parse_args()

    import torch
    from heligym_amd import HeliVecEnv, sample_weather
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    N, K, W, dt = args.envs, args.steps, args.handles, 0.01
    assert N % W == 0
    kw = dict(task="hover", dt=dt, autoreset=True, autoreset_mode="same_step", device=dev, seed=1)
    plain = HeliVecEnv(N, **kw)
    weather = HeliVecEnv(N, **kw)
    wx = sample_weather(N, seed=2)
    weather.set_weather(**wx)
    templated = HeliVecEnv(N, **kw)
    tm = weather.get_weather()["templates"]
    templated._check(give_templates(templated, tm))
    small = [HeliVecEnv(N // W, env_offset=j * (N // W), turbulence_level=j % 8, **kw) for j in range(W)]
    lib = plain.lib
    B = 16
    bank = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    for k in range(B):
        plain.random_actions(bank[k], seed=4, step=k)
    parts = [bank[:, j * (N // W):(j + 1) * (N // W)].contiguous() for j in range(W)]
    aged = int(round(args.age_seconds / dt))
    for env in (plain, templated, weather):
        env.reset()
        for k in range(aged):
            env.step_async(bank[k % B], with_reset_info=False)
    for env, a in zip(small, parts):
        env.reset()
        for k in range(aged):
            env.step_async(a[k % B], with_reset_info=False)
    torch.cuda.synchronize()

    torch.manual_seed(0)
    nn = torch.nn
    model = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    log_std = torch.full((4,), -1.0, device=dev)
    mean = plain.obs.mean(0).contiguous()
    scale = (1.0 / plain.obs.std(0).clamp_min(1e-3)).contiguous()
    cur, outs = {}, {}
    for name, env in (("plain", plain), ("weather", weather)):
        env.set_policy(model, log_std=log_std, obs_mean=mean, obs_scale=scale)
        cur[name] = env.obs.clone()
        outs[name] = env.rollout_policy(K, obs0=cur[name])   # (allocates the buffers; an untimed warm-up)
        cur[name].copy_(outs[name][1][K - 1])
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), plain._stream()) != 0:
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

    def loop():
        for k in range(K):
            for env, a in zip(small, parts):
                env.step_async(a[k % B], with_reset_info=False)

    variants = {"a_step_plain": steps(plain), "a2_step_plain_per_env_templates": steps(templated), "b_step_weather": steps(weather),
                "c_rollout_policy_plain": rollout("plain", plain), "c_rollout_policy_weather": rollout("weather", weather),
                "d_loop_of_plain_handles": loop}
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
    for _ in range(args.repeats):
        for name in variants:
            graphs[name].replay()
            torch.cuda.synchronize()
            t = stamps.cpu()
            times[name].append(float(t[1] - t[0]) * 1e-2 / K)   # 100 MHz ticks -> us per step of all --envs envs
    launches = {"plain": plain.debug_launches(), "weather": weather.debug_launches()}
    res = {"config": {"envs": N, "task": "hover", "dt": dt, "autoreset": "same_step", "steps_per_graph": K,
                      "plain_handles_in_d": W, "aged_steps": aged, "repeats": args.repeats,
                      "weather": "sample_weather(envs, seed=2): turbulence 0 .. 7, wind 0 .. 40 ft/s, any direction",
                      "policy": "MLP 17-64-64-4 tanh fp32, log_std -1", "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per step of all the envs",
           "us_per_step": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()},
           "launches": launches,
           "outputs_finite": bool(torch.isfinite(weather.obs).all() and torch.isfinite(outs["weather"][1]).all())}
    med = {n: res["us_per_step"][n]["median"] for n in times}
    res["ratio_b_over_a"] = med["b_step_weather"] / med["a_step_plain"]
    res["ratio_b_over_a2"] = med["b_step_weather"] / med["a2_step_plain_per_env_templates"]
    res["ratio_c_weather_over_plain"] = med["c_rollout_policy_weather"] / med["c_rollout_policy_plain"]
    res["ratio_d_over_b"] = med["d_loop_of_plain_handles"] / med["b_step_weather"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    for env in [plain, templated, weather] + small:
        env.close()


if __name__ == "__main__":
    main()
