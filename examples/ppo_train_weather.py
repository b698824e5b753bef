"""ppo_train_graph.py with the disturbance randomised per env: every env flies in its own weather.

    python examples/ppo_train_weather.py [--envs 4096] [--steps 64] [--iters 3]

What changes against ppo_train_graph.py:
  * env.set_weather(**sample_weather(N, ...)) before the capture: turbulence level, mean wind speed and direction
    drawn per env; every env is trimmed on the device against its own mean wind and resets to that trim.  The
    call synchronises and is made once, outside the graph; the captured iteration is unchanged, and
    rollout_actor_critic honours the weather;
  * the envs are sorted by turbulence level, so the terciles are contiguous ranges: the collection's mean reward
    is printed per tercile (calm, moderate, severe), beside the episode statistics RolloutStats keeps for the
    handle (env.rollout_stats, captured with the rest).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "heli-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64, help="K: steps per collection")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--minibatches", type=int, default=4)
    args = ap.parse_args()

    import numpy as np
    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv, PPOOptState, RolloutStats, sample_weather
    nn, dev = torch.nn, "cuda:0"
    N, K = args.envs, args.steps
    gamma, lam, clip, vf_coef, ent_coef, lr0 = 0.99, 0.95, 0.2, 0.5, 0.0, 3e-4

    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, max_episode_steps=500, device=dev, seed=7)
    wx = sample_weather(N, turb_level=(0.0, 7.0), wind_spd=(0.0, 40.0), wind_dir=(0.0, 360.0), seed=7)
    order = np.argsort(wx["turb_level"], kind="stable")
    wx = {k: v[order] for k, v in wx.items()}
    env.set_weather(**wx)
    thirds = [(j * N // 3, (j + 1) * N // 3) for j in range(3)]
    obs0 = env.reset()[0].clone()
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    critic = nn.Linear(64, 1).to(dev)                      # on the actor's trunk: actor[:4]
    log_std = nn.Parameter(torch.full((4,), -1.0, device=dev))
    obs_mean = obs0.mean(0).contiguous()
    obs_scale = (1.0 / obs0.std(0).clamp_min(1.0)).contiguous()   # fixed input normalisation, part of the policy
    params = ActorCriticParams(actor, critic, log_std)
    state = PPOOptState(dev)
    stats = RolloutStats(env)
    lr_dev = torch.full((1,), lr0, device=dev)
    obs_in = torch.empty((K, N, 17), dtype=torch.float32, device=dev)   # the observation each action was computed from
    adv = torch.empty((K, N), dtype=torch.float32, device=dev)
    by_third = torch.zeros((3,), dtype=torch.float32, device=dev)
    env.set_policy_theta(params, obs_mean, obs_scale)
    hold = {}

    def iteration():
        out = hold["out"] = env.rollout_actor_critic(K, gamma=gamma, lam=lam, obs0=obs0, out=hold.get("out"))
        env.rollout_stats(stats, out, gamma=gamma, obs0=obs0, update_obs=False)   # episode statistics only
        for j, (a, b) in enumerate(thirds):
            by_third[j:j + 1].copy_(out["reward"][:, a:b].mean().reshape(1))
        obs_in[0].copy_(obs0)
        obs_in[1:].copy_(out["obs"][:-1])
        a = out["advantages"]
        torch.div(a - a.mean(), a.std() + 1e-8, out=adv)
        hold["stats"] = env.ppo_update(params, state, obs_in, out["actions"], out["logp"], adv, out["returns"],
                                       epochs=args.epochs, minibatches=args.minibatches, seed=7, clip=clip,
                                       vf_coef=vf_coef, ent_coef=ent_coef, obs_mean=obs_mean, obs_scale=obs_scale,
                                       lr_dev=lr_dev, max_grad_norm=0.5, target_kl=0.03, publish=True)
        obs0.copy_(out["obs"][-1])

    # one eager iteration first: every kernel has run and every buffer exists before the capture
    iteration()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        iteration()

    lv = wx["turb_level"]
    print("turbulence terciles: " + ", ".join(f"[{lv[a]:.2f}, {lv[b - 1]:.2f}]" for a, b in thirds))
    for it in range(args.iters):
        if it:
            lr_dev.fill_(lr0 * (1.0 - it / args.iters))
            graph.replay()
        e, s, c, r3 = stats.episode_dict(), hold["stats"].cpu(), state.counters(), by_third.cpu().tolist()
        done = (f"episodes {int(e['episodes'])}, return {e['return_mean']:+.2f} +- {e['return_std']:.2f}"
                if e["episodes"] else "no episode ended")
        print(f"iter {it}: mean reward per tercile calm {r3[0]:+.4f} / moderate {r3[1]:+.4f} / severe {r3[2]:+.4f}; {done}; "
              f"loss {float(s[-1, 5]):.4f}, approx KL {float(s[-1, 2]):+.2e}; optimiser steps {c['applied']} of {c['seen']}")
    env.close()


if __name__ == "__main__":
    main()
