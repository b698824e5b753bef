"""ppo_train.py's loop with the whole training iteration captured into one graph and replayed.

    python examples/ppo_train_graph.py [--envs 4096] [--steps 64] [--iters 3]

What changes against ppo_train.py:
  * the update phase is env.ppo_update(...): per epoch a device shuffle of the stored rows, per minibatch the
    fused gradient kernel and one optimiser kernel (approximate-KL early stop, non-finite guard, global
    gradient-norm clipping, Adam); no torch.randperm, no torch optimiser, no host decision in between;
  * publish=True ends the update with hg_set_policy_theta: the env's policy image is rebuilt from the flat
    vector on the same stream;
  * so collect -> GAE -> advantage normalisation -> E epochs x n minibatches -> publish is one stream of
    launches: it is captured once and every iteration is one graph replay.  The permutations are keyed by the
    optimiser state's `seen` counter, which lives on the device, so every replay shuffles anew; the learning
    rate is a device scalar the host rewrites between replays (a linear decay here).
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

    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv, PPOOptState
    nn, dev = torch.nn, "cuda:0"
    N, K = args.envs, args.steps
    gamma, lam, clip, vf_coef, ent_coef, lr0 = 0.99, 0.95, 0.2, 0.5, 0.0, 3e-4

    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, max_episode_steps=500, device=dev, seed=7)
    obs0 = env.reset()[0].clone()
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

    # one eager iteration first: every kernel has run and every buffer exists before the capture
    iteration()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        iteration()

    for it in range(args.iters):
        if it:
            lr_dev.fill_(lr0 * (1.0 - it / args.iters))
            graph.replay()
        out, s, c = hold["out"], hold["stats"].cpu(), state.counters()
        ends = int(((out["terminated"] | out["truncated"]) != 0).sum())
        print(f"iter {it}: mean reward {float(out['reward'].mean()):+.4f}, episode ends {ends}, loss {float(s[-1, 5]):.4f}, "
              f"approx KL {float(s[-1, 2]):+.2e}, clip fraction {float(s[-1, 3]):.3f}; optimiser steps {c['applied']} of "
              f"{c['seen']} (KL-stopped {c['skipped_stopped']}, non-finite {c['skipped_nonfinite']}), gradient norm "
              f"{c['last_norm']:.3f}, clip coefficient {c['last_clip_coef']:.3f}")
    env.close()


if __name__ == "__main__":
    main()
