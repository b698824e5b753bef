"""ppo_train_graph.py with running normalisation of observations and rewards and episode statistics, still one
captured graph per iteration.

    python examples/ppo_train_norm.py [--envs 4096] [--steps 64] [--iters 3]

What changes against ppo_train_graph.py:
  * env.rollout_stats(stats, out, ...) follows the collection: one pass over what the rollout wrote keeps the
    running moments of the 17 observations and of the discounted return (what SB3's VecNormalize keeps), carries
    each env's episode return and length from launch to launch, and writes
      - stats.obs_mean / stats.obs_scale: the NEXT collection's input normalisation,
      - rew_n: the rewards times 1 / std(discounted return), clipped,
      - obs_in: the observation each action was computed from (the two [K,N,17] copies of ppo_train_graph.py),
      - stats.episode: episodes completed in this collection, their return's mean / std / min / max, mean
        length, terminated / truncated / success counts;
  * GAE runs on the scaled rewards (env.gae), so the critic learns returns of unit scale;
  * the policy's normalisation is a pair of device buffers the graph rewrites: see the comment in iteration().
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
    from heligym_amd import ActorCriticParams, HeliVecEnv, PPOOptState, RolloutStats
    nn, dev = torch.nn, "cuda:0"
    N, K = args.envs, args.steps
    gamma, lam, clip, vf_coef, ent_coef, lr0 = 0.99, 0.95, 0.2, 0.5, 0.0, 3e-4
    norm = dict(gamma=gamma, max_obs_scale=1e3, clip_reward=10.0)   # a column that never moves gets scale 1e3, not 1e4

    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, max_episode_steps=500, device=dev, seed=7)
    obs0 = env.reset()[0].clone()
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    critic = nn.Linear(64, 1).to(dev)                      # on the actor's trunk: actor[:4]
    log_std = nn.Parameter(torch.full((4,), -1.0, device=dev))
    params = ActorCriticParams(actor, critic, log_std)
    state = PPOOptState(dev)
    stats = RolloutStats(env)
    lr_dev = torch.full((1,), lr0, device=dev)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
    obs_in, rew_n, adv_raw, ret, adv = f32(K, N, 17), f32(K, N), f32(K, N), f32(K, N), f32(K, N)
    # the normalisation the env's policy image currently holds: the data of a collection was produced under it
    cur_mean, cur_scale = torch.zeros(17, device=dev), torch.ones(17, device=dev)
    hold = {}

    # seed the moments: one collection under the untrained policy on raw observations, then start over (the
    # first real collection is then normalised, and the env and the per-env accumulators are back at a reset)
    env.set_policy_theta(params, cur_mean, cur_scale)
    env.rollout_stats(stats, env.rollout_actor_critic(K, gamma=gamma, lam=lam, obs0=obs0), **norm)
    cur_mean.copy_(stats.obs_mean)
    cur_scale.copy_(stats.obs_scale)
    env.set_policy_theta(params, cur_mean, cur_scale)
    obs0.copy_(env.reset()[0])
    for per_env in (stats.G, stats.ep_ret, stats.ep_len):
        per_env.fill_(0)

    def iteration():
        out = hold["out"] = env.rollout_actor_critic(K, gamma=gamma, lam=lam, obs0=obs0, out=hold.get("out"))
        # moments <- this batch; stats.obs_mean / obs_scale are now the NEXT collection's normalisation
        env.rollout_stats(stats, out, obs0=obs0, obs_in=obs_in, reward_out=rew_n, **norm)
        env.gae(rew_n, out["value"], out["next_value"], out["terminated"], out["truncated"], gamma=gamma, lam=lam,
                out=(adv_raw, ret))
        torch.div(adv_raw - adv_raw.mean(), adv_raw.std() + 1e-8, out=adv)
        # The update must see the normalisation the data was collected under (cur_*), not the one the pass above
        # just produced: logp_old was computed through x = (obs - cur_mean) * cur_scale, and with another mean or
        # scale the first minibatch's ratio exp(logp - logp_old) would not be 1 and the clipping would bite on a
        # difference the optimiser did not make.  So: update under cur_*, THEN move next -> cur (two 68-byte
        # copies) and publish the new weights with the new normalisation for the next collection.
        hold["stats"] = env.ppo_update(params, state, obs_in, out["actions"], out["logp"], adv, ret,
                                       epochs=args.epochs, minibatches=args.minibatches, seed=7, clip=clip,
                                       vf_coef=vf_coef, ent_coef=ent_coef, obs_mean=cur_mean, obs_scale=cur_scale,
                                       lr_dev=lr_dev, max_grad_norm=0.5, target_kl=0.03, publish=False)
        cur_mean.copy_(stats.obs_mean)
        cur_scale.copy_(stats.obs_scale)
        env.set_policy_theta(params, cur_mean, cur_scale)
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
        e, s, c = stats.episode_dict(), hold["stats"].cpu(), state.counters()
        n = max(e["episodes"], 1.0)
        done = (f"return {e['return_mean']:+.3f} +- {e['return_std']:.3f} [{e['return_min']:+.3f}, {e['return_max']:+.3f}], "
                f"length {e['length_mean']:.1f}, success rate {e['success'] / n:.3f} (terminated {int(e['terminated'])}, "
                f"truncated {int(e['truncated'])})") if e["episodes"] else "none ended in this collection"
        print(f"iter {it}: episodes {int(e['episodes'])}, {done}; reward scale "
              f"{float(stats.reward_scale):.4f}, loss {float(s[-1, 5]):.4f}, approx KL {float(s[-1, 2]):+.2e}, "
              f"optimiser steps {c['applied']} of {c['seen']}")
    m = stats.moments()
    print(f"lifetime: {m['episodes']} episodes in {m['env_steps']} env-steps, {m['skipped_rows']} rows and "
          f"{m['skipped_returns']} return samples skipped")
    env.close()


if __name__ == "__main__":
    main()
