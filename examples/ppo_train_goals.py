"""ppo_train_graph.py's captured training iteration on a goal-conditioned task: hover to a waypoint that is
redrawn for every env at every episode, seen through goal-relative observations.

    python examples/ppo_train_goals.py [--envs 4096] [--steps 64] [--iters 3]

What changes against ppo_train_graph.py:
  * env.set_goals(box=..., relative=True): each env's waypoint is drawn in a box around the start (+-200 ft north
    and east, +-100 ft of altitude) by the kernel that resets the env, a function of (seed, global env id, episode)
    -- no host work, so the whole iteration is still one captured graph;
  * the observation rows carry position minus the waypoint, so the 17-input policy, the value head and the PPO
    update work unchanged; heligym_amd.goal_ref recomputes the waypoint of any stored row from its env id and
    episode, which the last lines below check against the env's table.

The printed mean episode return is what was observed over the episodes that ended in that iteration; a few
iterations of PPO from a random policy are not expected to hover, and nothing more is claimed.
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
    ap.add_argument("--episode-steps", type=int, default=32, help="TimeLimit: a new waypoint this often at the latest")
    args = ap.parse_args()

    import numpy as np
    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv, PPOOptState, goal_ref
    nn, dev = torch.nn, "cuda:0"
    N, K = args.envs, args.steps
    gamma, lam, clip, vf_coef, ent_coef, lr0 = 0.99, 0.95, 0.2, 0.5, 0.0, 3e-4
    seed = 7

    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, max_episode_steps=args.episode_steps, device=dev, seed=seed)
    start = env.template()["obs"]
    box = dict(north_loc=(start[13] - 200.0, start[13] + 200.0), east_loc=(start[14] - 200.0, start[14] + 200.0),
               sea_alt=(start[15] - 100.0, start[15] + 100.0))
    env.set_goals(box=box, relative=True)
    obs0 = env.reset()[0].clone()   # (already relative: the reset rows are in each env's goal frame)
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    critic = nn.Linear(64, 1).to(dev)                      # on the actor's trunk: actor[:4]
    log_std = nn.Parameter(torch.full((4,), -1.0, device=dev))
    obs_mean = obs0.mean(0).contiguous()
    obs_scale = (1.0 / obs0.std(0).clamp_min(1.0)).contiguous()   # fixed input normalisation, part of the policy
    params = ActorCriticParams(actor, critic, log_std)
    state = PPOOptState(dev)
    lr_dev = torch.full((1,), lr0, device=dev)
    obs_in = torch.empty((K, N, 17), dtype=torch.float32, device=dev)   # the observation each action was computed from
    adv = torch.empty((K, N), dtype=torch.float32, device=dev)
    # episode returns on the device: a running sum per env, flushed into (sum, count) where an episode ends
    run_ret = torch.zeros((N,), dtype=torch.float32, device=dev)
    ep_stats = torch.zeros((2,), dtype=torch.float32, device=dev)
    env.set_policy_theta(params, obs_mean, obs_scale)
    hold = {}

    def iteration():
        out = hold["out"] = env.rollout_actor_critic(K, gamma=gamma, lam=lam, obs0=obs0, out=hold.get("out"))
        obs_in[0].copy_(obs0)
        obs_in[1:].copy_(out["obs"][:-1])
        a = out["advantages"]
        torch.div(a - a.mean(), a.std() + 1e-8, out=adv)
        hold["stats"] = env.ppo_update(params, state, obs_in, out["actions"], out["logp"], adv, out["returns"],
                                       epochs=args.epochs, minibatches=args.minibatches, seed=7, clip=clip,
                                       vf_coef=vf_coef, ent_coef=ent_coef, obs_mean=obs_mean, obs_scale=obs_scale,
                                       lr_dev=lr_dev, max_grad_norm=0.5, target_kl=0.03, publish=True)
        obs0.copy_(out["obs"][-1])
        ep_stats.zero_()
        done = ((out["terminated"] | out["truncated"]) != 0).to(torch.float32)
        for k in range(K):   # (K small element-wise launches, captured with the rest)
            run_ret.add_(out["reward"][k])
            ep_stats[0] += (run_ret * done[k]).sum()
            ep_stats[1] += done[k].sum()
            run_ret.mul_(1.0 - done[k])

    # one eager iteration first: every kernel has run and every buffer exists before the capture
    iteration()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        iteration()

    returns = []
    for it in range(args.iters):
        if it:
            lr_dev.fill_(lr0 * (1.0 - it / args.iters))
            graph.replay()
        out, s, c = hold["out"], hold["stats"].cpu(), state.counters()
        tot, cnt = (float(v) for v in ep_stats.cpu())
        returns.append(tot / cnt if cnt else float("nan"))
        print(f"iter {it}: mean episode return {returns[-1]:+.4f} over {int(cnt)} episodes, mean reward "
              f"{float(out['reward'].mean()):+.4f}, loss {float(s[-1, 5]):.4f}, approx KL {float(s[-1, 2]):+.2e}; "
              f"optimiser steps {c['applied']} of {c['seen']}")
    print(f"mean episode return as observed: first iteration {returns[0]:+.4f}, last iteration {returns[-1]:+.4f}")
    # the waypoint of any row from its env id and episode alone
    g, ctr = env.get_goals(), env.get_state()[1].cpu().numpy()
    ref = goal_ref(seed, np.arange(N), ctr[:, 2], box, "hover")
    ok = all(np.array_equal(g[k].astype(np.float32), ref[k]) for k in box)
    print(f"goal table == goal_ref(seed, env id, episode): {ok}; episodes so far {int(ctr[:, 2].min())} .. {int(ctr[:, 2].max())}")
    env.close()


if __name__ == "__main__":
    main()
