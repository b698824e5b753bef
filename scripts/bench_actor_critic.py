"""Per-step time of an actor-critic collection step against the plain policy rollout and the torch
post-processing it replaces.

Method and configuration of bench_policy_rollout.py: 65 536 hover envs, dt 0.01, turbulence on,
same-step auto-reset, aged 60 simulated seconds with random actions, then, on the same handle, K = 100
steps per call:

  (a) hg_rollout_policy, as it was before the actor-critic calls existed;
  (b) hg_rollout_ac + hg_gae (HeliVecEnv.rollout_actor_critic): log-probabilities, values, next values of
      the pre-reset observations, advantages and returns from the same launch and one more;
  (c) what a learner did without (b): hg_rollout_policy, then the actor and a value head again as torch
      fp32 ops over the stored [K,N,17] observations for log-probabilities and values, then GAE as a
      torch loop over K.  (c) cannot value a terminal observation -- a rollout does not return it -- and
      bootstraps a truncation from the reset observation instead: it is cheaper than a correct (c);
  (gae) hg_gae alone on (b)'s outputs.

Each is captured into one hipGraph between two hg_clock_stamp kernels; a replay's time is the stamps'
difference (GPU 100 MHz clock), per step = / steps captured.  Every variant is warmed by one untimed
replay; the figure is the median of --repeats replays, the variants alternating.  Writes one JSON
document (--out) and prints it.

usage: python scripts/bench_actor_critic.py [--envs 65536] [--steps 100] [--repeats 7] [--out FILE]
"""
import argparse
import ctypes
import json
import math
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
    ap.add_argument("--calls", type=int, default=5, help="collection steps per graph")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--age-seconds", type=float, default=60.0)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_critic_rollout.json"))
    args = ap.parse_args()

    import torch
    from heligym_amd import HeliVecEnv
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    N, K, G, dt = args.envs, args.steps, args.calls, 0.01
    gamma, lam = args.gamma, args.lam
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

    # the policy and its value head: torch's default init, the input normalised by the aged population
    torch.manual_seed(0)
    nn = torch.nn
    model = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    head = nn.Linear(64, 1).to(dev)
    for p in list(model.parameters()) + list(head.parameters()):
        p.requires_grad_(False)
    trunk = model[:4]
    log_std = torch.full((4,), -1.0, device=dev)
    mean = env.obs.mean(0).contiguous()
    scale = (1.0 / env.obs.std(0).clamp_min(1e-3)).contiguous()
    env.set_policy(model, log_std=log_std, obs_mean=mean, obs_scale=scale)
    env.set_value_head(head)

    f32, u8 = torch.float32, torch.uint8
    cur = env.obs.clone()   # the envs' current observations: every variant reads and leaves them here
    out_b = env.rollout_actor_critic(K, gamma, lam, obs0=cur)   # (allocates (b)'s buffers; an untimed warm-up)
    cur.copy_(out_b["obs"][K - 1])
    out_a = tuple(out_b[k] for k in ("actions", "obs", "reward", "terminated", "truncated", "info"))
    obs_in = torch.empty((K + 1, N, 17), dtype=f32, device=dev)   # (c): o_0 .. o_K
    adv_c, logp_c = torch.empty((K, N), dtype=f32, device=dev), torch.empty((K, N), dtype=f32, device=dev)
    std, ls_sum = log_std.exp(), float(log_std.sum())
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    def run_a():
        for _ in range(G):
            env.rollout_policy(K, obs0=cur, out=out_a)
            cur.copy_(out_a[1][K - 1])

    def run_b():
        for _ in range(G):
            env.rollout_actor_critic(K, gamma, lam, obs0=cur, out=out_b)
            cur.copy_(out_b["obs"][K - 1])

    def run_c():
        for _ in range(G):
            obs_in[0].copy_(cur)
            act, obs, rew, term, trunc, _ = env.rollout_policy(K, obs0=cur, out=out_a)
            obs_in[1:].copy_(obs)
            h = trunk((obs_in - mean) * scale)
            v = head(h).squeeze(-1)                                   # [K + 1, N]
            z = (act - model[4](h[:K])) / std
            torch.sub(z.square().sum(-1).mul_(-0.5), ls_sum + 2.0 * math.log(2.0 * math.pi), out=logp_c)
            nv = torch.where(term != 0, torch.zeros_like(rew), v[1:])
            delta = rew + gamma * nv - v[:K]
            keep = ((term | trunc) == 0).to(f32) * (gamma * lam)
            a_next = torch.zeros((N,), dtype=f32, device=dev)
            for k in range(K - 1, -1, -1):
                a_next = torch.addcmul(delta[k], keep[k], a_next, out=adv_c[k])
            cur.copy_(obs[K - 1])

    def run_gae():
        for _ in range(G):
            env.gae(out_b["reward"], out_b["value"], out_b["next_value"], out_b["terminated"], out_b["truncated"],
                    gamma, lam, out=(out_b["advantages"], out_b["returns"]))

    variants = {"a_rollout_policy": run_a, "b_rollout_ac_gae": run_b, "c_rollout_policy_torch_post": run_c,
                "hg_gae_alone": run_gae}
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in variants.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # eager warm-up on the capture stream (code objects, BLAS workspaces)
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
            times[name].append(float(t[1] - t[0]) * 1e-2 / (G * K))   # 100 MHz ticks -> us per step
    _, ctr = env.get_state()
    done = (out_b["terminated"] | out_b["truncated"]) != 0
    boot = ((out_b["info"] & 16) != 0) & (out_b["terminated"] == 0)
    res = {"config": {"envs": N, "task": "hover", "dt": dt, "turbulence": "on (default level)",
                      "autoreset": "same_step", "steps_per_call": K, "calls_per_graph": G, "aged_steps": aged,
                      "repeats": args.repeats, "gamma": gamma, "lam": lam,
                      "policy": "MLP 17-64-64-4 tanh fp32, log_std -1, value head on the trunk",
                      "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per env step (hg_gae_alone: per step of "
                    "the K its one launch covers)",
           "us_per_step": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()},
           "last_rollout": {"episode_ends": int(done.sum()), "terminal_observations_valued": int(boot.sum()),
                            "waves_with_one": int(boot.view(K, -1, 64).any(-1).sum()) if N % 64 == 0 else None,
                            "wave_steps": K * ((N + 63) // 64)},
           "episodes_begun_max": int(ctr[:, 2].max()),
           "outputs_finite": bool(all(torch.isfinite(out_b[k]).all() for k in ("logp", "value", "next_value",
                                                                                "advantages", "returns")))}
    med = {n: res["us_per_step"][n]["median"] for n in times}
    res["ratio_b_over_a"] = med["b_rollout_ac_gae"] / med["a_rollout_policy"]
    res["ratio_c_over_b"] = med["c_rollout_policy_torch_post"] / med["b_rollout_ac_gae"]
    res["hg_gae_us_per_call"] = med["hg_gae_alone"] * K
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
