"""ppo_train_graph.py with the dynamics randomised: a mixed fleet, one airframe class per block of envs.

    python examples/ppo_train_fleet.py [--envs 4096] [--classes 8] [--steps 64] [--iters 3]

What changes against ppo_train_graph.py:
  * env.set_fleet(sample_fleet(C), envs_per_class=N // C) before the capture: weight, inertias, CG station and
    both rotor speeds drawn per class around the AW109 (class 0 is the AW109 itself); every class is trimmed on
    the host and its envs reset to that trim.  The call synchronises and is made once, outside the graph; the
    captured iteration is unchanged, and rollout_actor_critic steps every env with its class's constants;
  * the collection's mean reward and the mean return of the episodes that ended in it are printed per class,
    beside the episode statistics RolloutStats keeps for the handle (env.rollout_stats, captured with the rest).
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
    ap.add_argument("--classes", type=int, default=8, help="C: airframe classes, consecutive blocks of envs / C envs")
    ap.add_argument("--steps", type=int, default=64, help="K: steps per collection")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--minibatches", type=int, default=4)
    args = ap.parse_args()

    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv, PPOOptState, RolloutStats, sample_fleet
    nn, dev = torch.nn, "cuda:0"
    N, K, C = args.envs, args.steps, args.classes
    assert N % (64 * C) == 0, "--envs must be a multiple of 64 * --classes (a class is whole 64-env tiles)"
    gamma, lam, clip, vf_coef, ent_coef, lr0 = 0.99, 0.95, 0.2, 0.5, 0.0, 3e-4

    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, max_episode_steps=500, device=dev, seed=7)
    docs = sample_fleet(C, seed=7)
    env.set_fleet(docs, envs_per_class=N // C)
    blocks = [(c * (N // C), (c + 1) * (N // C)) for c in range(C)]
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
    by_class = torch.zeros((C, 3), dtype=torch.float32, device=dev)   # mean reward | return sum, count of ended episodes
    ep_ret = torch.zeros((N,), dtype=torch.float32, device=dev)      # each env's running episode return
    env.set_policy_theta(params, obs_mean, obs_scale)
    hold = {}

    def iteration():
        out = hold["out"] = env.rollout_actor_critic(K, gamma=gamma, lam=lam, obs0=obs0, out=hold.get("out"))
        env.rollout_stats(stats, out, gamma=gamma, obs0=obs0, update_obs=False)   # episode statistics only
        done = (out["terminated"] | out["truncated"]).to(torch.float32)
        csum = torch.cumsum(out["reward"], dim=0) + ep_ret   # the running return if no episode had ended before
        # the return of an episode ending at step k: csum[k] minus csum at the env's previous ending step
        ended = torch.zeros_like(csum)
        base = torch.zeros((N,), dtype=torch.float32, device=dev)
        for k in range(K):   # (K small: a plain loop of device ops, captured with the rest)
            ended[k] = (csum[k] - base) * done[k]
            base = torch.where(done[k].bool(), csum[k], base)
        ep_ret.copy_(csum[-1] - base)
        for c, (a, b) in enumerate(blocks):
            by_class[c, 0:1].copy_(out["reward"][:, a:b].mean().reshape(1))
            by_class[c, 1:2].copy_(ended[:, a:b].sum().reshape(1))
            by_class[c, 2:3].copy_(done[:, a:b].sum().reshape(1))
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

    print("classes (weight lb, main rotor rpm): " + ", ".join(f"{c}: {d['airframe']['WT']:.0f}, {d['airframe']['mr_RPM']:.0f}"
                                                              for c, d in enumerate(docs)))
    for it in range(args.iters):
        if it:
            lr_dev.fill_(lr0 * (1.0 - it / args.iters))
            graph.replay()
        e, s, c, rc = stats.episode_dict(), hold["stats"].cpu(), state.counters(), by_class.cpu().tolist()
        done = (f"episodes {int(e['episodes'])}, return {e['return_mean']:+.2f} +- {e['return_std']:.2f}"
                if e["episodes"] else "no episode ended")
        per = " ".join(f"[{j}: r {r:+.4f}" + (f", ep {g / n:+.2f} x{int(n)}]" if n else "]") for j, (r, g, n) in enumerate(rc))
        print(f"iter {it}: per class mean reward, mean return of the episodes ended {per}; {done}; "
              f"loss {float(s[-1, 5]):.4f}, approx KL {float(s[-1, 2]):+.2e}; optimiser steps {c['applied']} of {c['seen']}")
    env.close()


if __name__ == "__main__":
    main()
