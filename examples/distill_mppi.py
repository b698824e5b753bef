"""Distil the planner into the policy: DAgger against PolicyMPPI on hover, all of it on the device.

    python examples/distill_mppi.py [--envs 256] [--branches 16] [--horizon 10] [--block 16] [--blocks 6]

Every control step the planner improves on the policy from the env's current state: PolicyMPPI.plan(obs) is the
label a*, the action the planner would apply, and PolicyMPPI.value() its n-step lookahead value y of that state
(the softmax-weighted return of its candidates, the value head behind the horizon).  The env is stepped with the
POLICY's own mean action, not the planner's: the states visited are the student's, the labels the expert's.
Every --block steps one bc_update on the collected [block, N] rows regresses the policy's mean onto a* (mode
"mse") and the critic onto y, and publishes the weights to the env, so the next block's planner starts from the
distilled policy and bootstraps from the distilled critic.

Printed per block: the last minibatch's mean squared action error (stats[2]: how far the policy is from what the
planner makes of it) and the planner's mean best - value (how much its best candidate stands out).  Nothing is
claimed about the figures: the point is the wiring.
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
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--branches", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--block", type=int, default=16, help="K: control steps per bc_update")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--lam", type=float, default=0.02)
    ap.add_argument("--lr", type=float, default=1e-3)
    args = ap.parse_args()

    import numpy as np
    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv, PolicyMPPI, PPOOptState
    nn, dev = torch.nn, "cuda:0"
    N, K = args.envs, args.block

    env = HeliVecEnv(N, task="hover", dt=0.01, autoreset=True, max_episode_steps=200, device=dev, seed=3)
    obs = env.reset()[0].clone()
    obs_mean = obs.mean(0).contiguous()
    obs_scale = (1.0 / obs.std(0).clamp_min(1.0)).contiguous()
    trim = torch.as_tensor(np.asarray(env.template()["action"], dtype=np.float32), device=dev)
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    critic = nn.Linear(64, 1).to(dev)
    with torch.no_grad():   # start at the trim action
        actor[4].weight.mul_(0.05)
        actor[4].bias.copy_(trim)
    params = ActorCriticParams(actor, critic, nn.Parameter(torch.full((4,), -1.0, device=dev)))
    state = PPOOptState(dev)
    env.set_policy_theta(params, obs_mean, obs_scale)
    planner = PolicyMPPI(env, args.horizon, args.branches, sigma=args.sigma, lam=args.lam, res_lo=-0.25, res_hi=0.25,
                         lo=-1.0, hi=1.0, gamma=0.99, noise="off", seed=1, bootstrap=True)

    obs_buf = torch.empty((K, N, 17), dtype=torch.float32, device=dev)
    label = torch.empty((K, N, 4), dtype=torch.float32, device=dev)
    y = torch.empty((K, N), dtype=torch.float32, device=dev)
    worth = None
    for block in range(args.blocks):
        gap = torch.zeros((), dtype=torch.float64, device=dev)
        for k in range(K):
            obs_buf[k].copy_(obs)
            label[k].copy_(planner.plan(obs_buf[k]))   # the expert's action at the student's state
            worth = planner.value(out=worth)
            y[k].copy_(worth["value"])
            gap += (worth["best"] - worth["value"]).double().mean()
            action = env.policy_act_mean(obs_buf[k], lo=-1.0, hi=1.0)   # the student's own
            obs, _, terminated, truncated, _ = env.step(action)
            planner.shift()
            planner.reset(terminated | truncated)
        stats = env.bc_update(params, state, obs_buf, label, value_target=y, epochs=4, minibatches=4, seed=block, mode="mse",
                              vf_coef=0.5, obs_mean=obs_mean, obs_scale=obs_scale, lr=args.lr, max_grad_norm=0.5, publish=True)
        s = stats[-1].cpu()
        print(f"block {block}: squared action error {float(s[2]):.3e}  value error {float(s[1]):.3e}  "
              f"planner's mean best - value {float(gap) / K:.3e}")
    env.close()


if __name__ == "__main__":
    main()
