"""N hover envs under the device MPPI planner in closed loop, against holding the trim action.

    python examples/mppi_hover.py [--envs 256] [--branches 64] [--horizon 30] [--steps 200]

It shows the contract, not a tuned controller:
  * every control step MPPI.plan() perturbs each env's nominal action sequence (hg_mppi_sample), scores all
    candidates from the env's current state in one launch that leaves the env as it is
    (hg_rollout_branch), and takes their softmax-weighted mean (hg_mppi_update);
  * the env is stepped with the nominal's first action, MPPI.shift() moves the nominal on by one step and
    MPPI.reset(mask) puts the nominal of the envs whose episode ended back to the trim action;
  * noise="env" scores the candidates against the turbulence the env is about to draw (the planner sees
    the gusts ahead), noise="off" against none.
The printed figures are the mean reward per step of the two runs; nothing is claimed about them.
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
    ap.add_argument("--branches", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--lam", type=float, default=0.02)
    ap.add_argument("--noise", choices=("env", "off"), default="off")
    args = ap.parse_args()

    import torch
    from heligym_amd import MPPI, HeliVecEnv
    dev = "cuda:0"
    kw = dict(task="hover", dt=0.01, autoreset=True, max_episode_steps=1000, device=dev, seed=3)

    def run(planned):
        env = HeliVecEnv(args.envs, **kw)
        env.reset()
        mppi = MPPI(env, args.horizon, args.branches, sigma=args.sigma, lam=args.lam, gamma=0.99, noise=args.noise, seed=1)
        hold = mppi.trim_action.expand(args.envs, 4).contiguous()
        total = torch.zeros((), device=dev, dtype=torch.float64)
        for _ in range(args.steps):
            action = mppi.plan() if planned else hold
            _, reward, terminated, truncated, _ = env.step(action)
            total += reward.double().mean()
            if planned:
                mppi.shift()
                mppi.reset(terminated | truncated)
        env.close()
        return float(total) / args.steps

    print(f"mean reward per step over {args.steps} steps of {args.envs} envs: "
          f"MPPI ({args.branches} branches, horizon {args.horizon}, noise {args.noise}) {run(True):+.5f}, "
          f"trim action held {run(False):+.5f}")


if __name__ == "__main__":
    main()
