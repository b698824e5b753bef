"""Cost of scoring closed-loop planner candidates: hg_rollout_branch_policy against its floor, against the
bare policy rollout, and against the route that exists without it.

1 024 hover envs, dt 0.01, turbulence on, same-step auto-reset, aged 6 000 steps with random actions;
64 residual sequences per env (hg_mppi_sample around zero), horizon 50, gamma 0.99: 65 536 rows.  The policy
is a fixed random 17-64-64-4 network (b3 = the trim action, a small W3) with a value head.  Per scoring of
all candidates:

  (a) hg_rollout_branch_policy with HG_BOOTSTRAP_VALUE on the 1 024-env handle;
  (b) hg_rollout_branch on the same rows (open-loop actions = trim + residual): the floor without the policy;
  (c) a bare hg_rollout_policy of a second handle of 65 536 envs for 50 steps (the same weights, deterministic);
  (d) the route (a) replaces: get_state of the planner's envs -> repeat_interleave -> set_state on the second
      handle, hg_rollout_policy with all its outputs, then in torch the discounted sum up to each row's first
      end and a value forward pass on each row's last observation (no residual: the policy alone);
  (e) a whole PolicyMPPI.plan(): sample, (a), update, act.

Method as bench_branch_rollout.py: each variant is one hipGraph between two hg_clock_stamp kernels (GPU
100 MHz clock), warmed by one untimed replay; the figure is the median of --repeats replays, the variants
alternating.  Writes one JSON document (--out) and prints it.

usage: python scripts/bench_branch_policy.py [--envs 1024] [--branches 64] [--horizon 50] [--repeats 7] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "heli-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--branches", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--calls", type=int, default=4, help="scorings per graph")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--age-steps", type=int, default=6000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_policy.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from heligym_amd import HeliVecEnv, PolicyMPPI
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    N, M, H, G, dt, gamma, vscale = args.envs, args.branches, args.horizon, args.calls, 0.01, 0.99, 0.5
    R = N * M
    kw = dict(task="hover", dt=dt, autoreset=True, autoreset_mode="same_step", device=dev, seed=1)
    env = HeliVecEnv(N, **kw)
    wide = HeliVecEnv(R, **{**kw, "autoreset": False})   # (its rows' last observations stay the terminal ones)
    lib = env.lib
    env.reset()
    wide.reset()
    bank = torch.empty((16, N, 4), dtype=torch.float32, device=dev)
    for k in range(16):
        env.random_actions(bank[k], seed=4, step=k)
    for k in range(args.age_steps):
        env.step_async(bank[k % 16], with_reset_info=False)
    torch.cuda.synchronize()
    obs0 = env.obs.clone()
    wide_obs0 = wide.obs.clone()

    f32, u8 = torch.float32, torch.uint8
    trim = torch.as_tensor(np.asarray(env.template()["action"], dtype=np.float32), device=dev)
    g = torch.Generator().manual_seed(31)
    r = lambda *s: torch.randn(s, generator=g).to(dev)   # noqa: E731
    W1, b1, W2, b2, W3, b3 = r(64, 17) / 17 ** 0.5, 0.1 * r(64), r(64, 64) / 8.0, 0.1 * r(64), 0.02 * r(4, 64), trim.clone()
    wv, bv = r(64) / 8.0, torch.tensor([0.3], device=dev)
    mean, scale = obs0.mean(0), 1.0 / obs0.std(0).clamp_min(1e-3)
    env.set_policy([(W1, b1), (W2, b2), (W3, b3)], log_std=torch.full((4,), -1.0), obs_mean=mean, obs_scale=scale)
    wide.set_policy([(W1, b1), (W2, b2), (W3, b3)], obs_mean=mean, obs_scale=scale)
    env.set_value_head((wv, bv))
    wide.set_value_head((wv, bv))

    zero_nominal = torch.zeros((H, N, 4), dtype=f32, device=dev)
    residuals = env.mppi_sample(zero_nominal, M, 0.1, -0.3, 0.3, seed=9)
    actions = (residuals + trim).clamp_(-1.0, 1.0).contiguous()
    score = env.rollout_branch_policy(residuals, M, obs0=obs0, gamma=gamma, lo=-1.0, hi=1.0, bootstrap=True,
                                      value_scale=vscale)
    score_b = env.rollout_branch(actions, M, gamma=gamma)
    out_w = (torch.empty((H, R, 4), dtype=f32, device=dev), torch.empty((H, R, 17), dtype=f32, device=dev),
             torch.empty((H, R), dtype=f32, device=dev), torch.empty((H, R), dtype=u8, device=dev),
             torch.empty((H, R), dtype=u8, device=dev), torch.empty((H, R), dtype=u8, device=dev))
    ret_d = torch.empty((R,), dtype=f32, device=dev)
    gpow = (torch.tensor(float(np.float32(gamma)), dtype=torch.float64) ** torch.arange(H + 1, dtype=torch.float64)).to(
        dev, f32)
    planner = PolicyMPPI(env, H, M, sigma=0.1, lam=0.05, res_lo=-0.3, res_hi=0.3, lo=-1.0, hi=1.0, gamma=gamma, seed=9,
                         bootstrap=True, value_scale=vscale)
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    def run_a():
        for _ in range(G):
            env.rollout_branch_policy(residuals, M, obs0=obs0, gamma=gamma, lo=-1.0, hi=1.0, bootstrap=True,
                                      value_scale=vscale, out=score)

    def run_b():
        for _ in range(G):
            env.rollout_branch(actions, M, gamma=gamma, out=score_b)

    def run_c():
        for _ in range(G):
            wide.rollout_policy(H, obs0=wide_obs0, out=out_w)

    def reduce_d(obs, rew, term, trunc):
        done = (term | trunc).to(torch.int32)
        before = done.cumsum(0) - done
        alive = before == 0   # up to and including the first ending step
        ret = (rew * alive * gpow[:H, None]).sum(0)
        T = alive.sum(0)
        last = obs.gather(0, (T - 1)[None, :, None].expand(1, R, 17))[0]
        h2 = torch.tanh(torch.tanh(((last - mean) * scale) @ W1.T + b1) @ W2.T + b2)
        v = h2 @ wv + bv
        ended_by_term = ((term != 0) & alive).any(0)
        torch.add(ret, torch.where(ended_by_term, torch.zeros_like(v), gpow[T] * (vscale * v)), out=ret_d)

    def run_d(eta=None):
        for _ in range(G):
            s, c = env.get_state()
            wide.set_state(s.repeat_interleave(M, dim=0), c.repeat_interleave(M, dim=0))
            _, obs, rew, term, trunc, _ = wide.rollout_policy(H, obs0=obs0.repeat_interleave(M, dim=0), eta=eta, out=out_w)
            reduce_d(obs, rew, term, trunc)

    def run_e():
        for _ in range(G):
            planner.plan(obs0)

    variants = {"a_rollout_branch_policy_bootstrap": run_a, "b_rollout_branch_floor": run_b,
                "c_bare_rollout_policy_second_handle": run_c, "d_second_handle_expand_rollout_policy_reduce_value": run_d,
                "e_policy_mppi_plan": run_e}
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in variants.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # eager warm-up on the capture stream
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            stamp(0)
            fn()
            stamp(1)
        graphs[name] = gr
        gr.replay()   # untimed
        torch.cuda.synchronize()

    # (d) computes what (a) computes for a zero residual once both see the same noise: the second handle's envs
    # have ids (noise keys) of their own, so the two routes can only be compared without noise (untimed)
    off = env.rollout_branch_policy(None, M, obs0=obs0, gamma=gamma, noise="off", bootstrap=True, value_scale=vscale,
                                    horizon=H)["returns"].reshape(-1).clone()
    G1, G = G, 1
    run_d(eta=torch.zeros((H, R, 3), dtype=f32, device=dev))
    G = G1
    torch.cuda.synchronize()
    agree = float(((off - ret_d).abs() / ret_d.abs().clamp_min(1.0)).max())

    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name in variants:
            graphs[name].replay()
            torch.cuda.synchronize()
            t = stamps.cpu()
            times[name].append(float(t[1] - t[0]) * 1e-2 / G)   # 100 MHz ticks -> us per scoring
    stat = {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()}
    med = {n: stat[n]["median"] for n in stat}
    a, b, c, d = list(variants)[:4]
    spread = lambda n: (stat[n]["max"] - stat[n]["min"]) / med[n]   # noqa: E731
    res = {"config": {"envs": N, "branches": M, "rows": R, "horizon": H, "gamma": gamma, "value_scale": vscale,
                      "noise": "env", "task": "hover", "dt": dt, "turbulence": "on (default level)",
                      "autoreset": "same_step (the second handle: none)", "aged_steps": args.age_steps, "scorings_per_graph": G,
                      "repeats": args.repeats, "policy": "fixed random 17-64-64-4, b3 = trim, W3 ~ 0.02 N(0,1), value head",
                      "policy_image_c_d": "deterministic (no log_std)", "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay; us per scoring of all rows (e: per plan)",
           "us_per_scoring": stat,
           "us_per_row_step": {n: med[n] / H for n in (a, b, c, d)},
           "ratio_a_over_c": med[a] / med[c],
           "ratio_a_over_b": med[a] / med[b],
           "ratio_d_over_a": med[d] / med[a],
           "spread_a": spread(a), "spread_b": spread(b), "spread_c": spread(c),
           "row_steps_per_s_a": R * H / (med[a] * 1e-6),
           "max_rel_return_difference_a_d_noise_off_zero_residual": agree,
           "alive_steps_min_mean": [int(score["alive_steps"].min()), float(score["alive_steps"].float().mean())],
           "launches_planner_handle": env.debug_launches()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    env.close()
    wide.close()


if __name__ == "__main__":
    main()
