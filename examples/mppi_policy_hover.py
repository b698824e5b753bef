"""The learner meets the planner: the same hover envs under a policy's mean action, under open-loop MPPI,
and under PolicyMPPI -- MPPI on a residual around the policy, with the value head behind the horizon.

    python examples/mppi_policy_hover.py [--envs 256] [--branches 32] [--horizon 25] [--steps 200] [--untrained]

  1. A short PPO run on a training handle (examples/ppo_train.py's loop), or with --untrained fixed random
     weights whose last layer is small around the trim action.  Either way the critic has seen little: the
     point is the wiring, not the score.
  2. Three fresh handles with the same seed, so the same turbulence, each stepped --steps times:
       policy      a = policy_act_mean(obs)                           the policy's mean, nothing drawn
       MPPI        a = MPPI.plan()                                    open-loop candidates around a nominal
       PolicyMPPI  a = PolicyMPPI.plan(obs)                           candidates policy + residual, rolled out
                                                                      closed-loop (hg_rollout_branch_policy),
                                                                      survivors scored gamma^H V(o_H)
     after each step shift() moves the planner's sequence on and reset(mask) clears it for the envs whose
     episode ended.  noise="off": the planners do not see the gusts ahead.
The printed figures are the mean return of the episodes (or of the whole run where none ended) per controller;
nothing is claimed about them.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "heli-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def train(args, actor, critic, log_std, obs_mean, obs_scale, dev):
    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv
    N, K = args.train_envs, 64
    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, max_episode_steps=500, device=dev, seed=7)
    obs0 = env.reset()[0].clone()
    params = ActorCriticParams(actor, critic, log_std)
    opt = torch.optim.Adam(params.parameters(), lr=3e-4, fused=True)
    obs_in = torch.empty((K, N, 17), dtype=torch.float32, device=dev)
    out = None
    for it in range(args.iters):
        env.set_policy(actor, log_std=log_std.detach(), obs_mean=obs_mean, obs_scale=obs_scale)
        env.set_value_head(critic)
        out = env.rollout_actor_critic(K, gamma=0.99, lam=0.95, obs0=obs0, out=out)
        obs_in[0].copy_(obs0)
        obs_in[1:].copy_(out["obs"][:-1])
        adv = out["advantages"]
        adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).contiguous()
        for _ in range(2):
            for idx in torch.randperm(K * N, device=dev).to(torch.int32).chunk(4):
                env.ppo_grad(params, obs_in, out["actions"], out["logp"], adv, out["returns"], index=idx.contiguous(),
                             clip=0.2, vf_coef=0.5, ent_coef=0.0, obs_mean=obs_mean, obs_scale=obs_scale)
                opt.step()
        print(f"PPO iter {it}: mean reward {float(out['reward'].mean()):+.4f}")
        obs0 = out["obs"][-1].clone()
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--branches", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=25)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--lam", type=float, default=0.02)
    ap.add_argument("--untrained", action="store_true", help="fixed random weights instead of the PPO run")
    ap.add_argument("--iters", type=int, default=3, help="PPO iterations")
    ap.add_argument("--train-envs", type=int, default=4096)
    args = ap.parse_args()

    import numpy as np
    import torch
    from heligym_amd import MPPI, HeliVecEnv, PolicyMPPI
    nn, dev, gamma = torch.nn, "cuda:0", 0.99
    kw = dict(task="hover", dt=0.01, autoreset=True, max_episode_steps=100, device=dev, seed=3)

    probe = HeliVecEnv(args.envs, **kw)
    obs = probe.reset()[0]
    obs_mean = obs.mean(0).contiguous()
    obs_scale = (1.0 / obs.std(0).clamp_min(1.0)).contiguous()
    trim = torch.as_tensor(np.asarray(probe.template()["action"], dtype=np.float32), device=dev)
    probe.close()
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    critic = nn.Linear(64, 1).to(dev)
    log_std = nn.Parameter(torch.full((4,), -1.0, device=dev))
    with torch.no_grad():   # start at the trim action
        actor[4].weight.mul_(0.05)
        actor[4].bias.copy_(trim)
    if not args.untrained:
        train(args, actor, critic, log_std, obs_mean, obs_scale, dev)

    def run(kind):
        env = HeliVecEnv(args.envs, **kw)
        obs = env.reset()[0]
        env.set_policy(actor, log_std=log_std.detach(), obs_mean=obs_mean, obs_scale=obs_scale)
        env.set_value_head(critic)
        common = dict(sigma=args.sigma, lam=args.lam, gamma=gamma, noise="off", seed=1)
        planner = {"policy": None, "MPPI": MPPI(env, args.horizon, args.branches, **common) if kind == "MPPI" else None,
                   "PolicyMPPI": PolicyMPPI(env, args.horizon, args.branches, res_lo=-0.25, res_hi=0.25, lo=-1.0, hi=1.0,
                                            bootstrap=True, **common) if kind == "PolicyMPPI" else None}[kind]
        ep = torch.zeros(args.envs, dtype=torch.float64, device=dev)
        done_sum = torch.zeros((), dtype=torch.float64, device=dev)
        done_n = torch.zeros((), dtype=torch.float64, device=dev)
        for _ in range(args.steps):
            if kind == "policy":
                action = env.policy_act_mean(obs, lo=-1.0, hi=1.0)
            elif kind == "MPPI":
                action = planner.plan()
            else:
                action = planner.plan(obs)
            obs, reward, terminated, truncated, _ = env.step(action)
            ended = terminated | truncated
            ep += reward.double()
            done_sum += (ep * ended).sum()
            done_n += ended.sum()
            ep *= ~ended
            if planner is not None:
                planner.shift()
                planner.reset(ended)
        env.close()
        n = float(done_n)
        return (float(done_sum) / n, int(n)) if n else (float(ep.mean()), 0)

    for kind in ("policy", "MPPI", "PolicyMPPI"):
        ret, n = run(kind)
        what = f"mean return of {n} episodes" if n else f"mean return of the unfinished {args.steps}-step run"
        print(f"{kind:>10}: {what} {ret:+.4f}")


if __name__ == "__main__":
    main()
