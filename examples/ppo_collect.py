"""Minimal PPO loop on the fused actor-critic rollout: collect -> torch update -> hand the weights back.

    python examples/ppo_collect.py [--envs 4096] [--steps 64] [--iters 5]

It shows the contract, not a tuned learner:
  * the env owns a copy of the actor (17-64-64-4 tanh, state-independent log_std) and of a value head on
    the actor's second hidden layer; set_policy / set_value_head copy the learner's weights in, once per
    update, on the stream the rollout runs on;
  * rollout_actor_critic(K) returns, from one rollout launch and one GAE launch, everything the update
    needs: observations, actions, log pi(a|s) of the actions as sampled, V(s), next_value (0 where
    terminated, the value of the pre-reset observation where truncated), advantages and returns;
  * the observation a step's action was computed from is obs0 for step 0 and obs[k - 1] after; `obs[-1]`
    is the next call's obs0.
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--minibatches", type=int, default=4)
    args = ap.parse_args()

    import torch
    from heligym_amd import HeliVecEnv
    nn, dev = torch.nn, "cuda:0"
    N, K = args.envs, args.steps
    gamma, lam, clip = 0.99, 0.95, 0.2

    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, max_episode_steps=500, device=dev, seed=7)
    obs0 = env.reset()[0].clone()
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    critic = nn.Linear(64, 1).to(dev)                      # on the actor's trunk: actor[:4]
    log_std = nn.Parameter(torch.full((4,), -1.0, device=dev))
    obs_mean = obs0.mean(0)
    obs_scale = 1.0 / obs0.std(0).clamp_min(1.0)           # fixed input normalisation, part of the policy
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    opt = torch.optim.Adam(params, lr=3e-4)

    def evaluate(o, a):
        """log pi(a|o) and V(o) of the learner's weights: the function the kernel evaluates."""
        h = actor[:4]((o - obs_mean) * obs_scale)
        dist = torch.distributions.Normal(actor[4](h), log_std.exp())
        return dist.log_prob(a).sum(-1), critic(h).squeeze(-1)

    out = None
    for it in range(args.iters):
        env.set_policy(actor, log_std=log_std.detach(), obs_mean=obs_mean, obs_scale=obs_scale)
        env.set_value_head(critic)
        out = env.rollout_actor_critic(K, gamma=gamma, lam=lam, obs0=obs0, out=out)
        obs_in = torch.cat([obs0[None], out["obs"][:-1]]).reshape(K * N, 17)
        act, logp_old = out["actions"].reshape(K * N, 4), out["logp"].reshape(K * N)
        adv, ret = out["advantages"].reshape(K * N), out["returns"].reshape(K * N)
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        if it == 0:   # the kernel's log-probabilities and values are the learner's, to fp32 rounding
            with torch.no_grad():
                lp, v = evaluate(obs_in, act)
            print(f"kernel vs torch: max |logp diff| {float((lp - logp_old).abs().max()):.2e}, "
                  f"max |value diff| {float((v - out['value'].reshape(-1)).abs().max()):.2e}")
        for _ in range(args.epochs):
            for idx in torch.randperm(K * N, device=dev).chunk(args.minibatches):
                lp, v = evaluate(obs_in[idx], act[idx])
                ratio = (lp - logp_old[idx]).exp()
                pg = -torch.min(ratio * adv[idx], ratio.clamp(1 - clip, 1 + clip) * adv[idx]).mean()
                loss = pg + 0.5 * (v - ret[idx]).square().mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
        ends = int(((out["terminated"] | out["truncated"]) != 0).sum())
        print(f"iter {it}: mean reward {float(out['reward'].mean()):+.4f}, episode ends {ends}, "
              f"loss {float(loss.detach()):.4f}")
        obs0 = out["obs"][-1].clone()
    env.close()


if __name__ == "__main__":
    main()
