"""Time of one imitation minibatch gradient: the fused kernel against the torch route it replaces and against
hg_ppo_grad on the same rows.

Stored rows: bench_ppo_grad.py's (B = envs * steps samples of synthetic collection data on the device), with the
actions as the targets, weights uniform in [0, 2] and the returns as the value targets.  For each minibatch size
M (a random int32 index of M distinct rows):

  (a) hg_bc_grad (HeliVecEnv.bc_grad) over the index, mode "nll" and mode "mse";
  (b) torch: gather obs / target / weight / value target by the same index, heligym_amd.policy.bc_loss ("nll")
      and autograd back through it, fp32;
  (c) hg_ppo_grad over the same index.

(a) and (c) issue the same matrix work (630 v_mfma_f32_32x32x2_f32 per 64-sample tile): the ratio a / c says
what the second loss head costs, b / a what the fused kernel saves.  Method of bench_ppo_grad.py: one hipGraph of
`calls` calls per variant between two hg_clock_stamp kernels; a replay's time is the stamps' difference (GPU
100 MHz clock) / calls; one untimed replay, then the median of --repeats replays with min and max, the variants
alternating.  Writes one JSON document (--out) and prints it.

usage: python scripts/bench_bc_grad.py [--envs 65536] [--steps 25] [--repeats 7] [--out FILE]
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
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=25, help="K: the stored rows are envs * K")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc_grad.json"))
    args = ap.parse_args()

    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv
    from heligym_amd.policy import LOG_2PI, bc_loss, ppo_views
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    B = args.envs * args.steps
    clip, vf, ent = 0.2, 0.5, 0.01
    env = HeliVecEnv(64, task="hover", dt=0.01, device=dev, seed=1)   # the handle: device and error convention only
    lib = env.lib
    nn = torch.nn
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
    critic = nn.Linear(64, 1).to(dev)
    P = ActorCriticParams(actor, critic, nn.Parameter(torch.full((4,), -1.0, device=dev)))
    with torch.no_grad():
        obs = torch.randn((B, 17), device=dev)
        p = ppo_views(P.theta + 0.02 * torch.randn_like(P.theta))
        h2 = torch.tanh(torch.tanh(obs @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"])
        z = torch.randn((B, 4), device=dev)
        actions = (h2 @ p["W3"].T + p["b3"] + torch.exp(p["log_std"]) * z).contiguous()
        logp_old = -0.5 * (z * z).sum(-1) - p["log_std"].sum() - 2 * LOG_2PI
        adv = torch.randn((B,), device=dev)
        ret = h2 @ p["w_v"] + p["b_v"] + 1.0 + 0.5 * torch.randn((B,), device=dev)
        weight = 2.0 * torch.rand((B,), device=dev)
        del h2, z
    theta_t = P.theta.detach().clone().requires_grad_(True)   # (b)'s leaf
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    res = {"config": {"stored_rows": B, "policy": "MLP 17-64-64-4 tanh fp32, log_std -1, value head on the trunk",
                      "vf_coef": vf, "ent_coef": ent, "ppo_clip": clip, "repeats": args.repeats,
                      "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay of `calls` calls; us per call",
           "sizes": {}}
    side = torch.cuda.Stream()
    for M, calls in ((B, 1), (args.envs, 8)):
        g = torch.Generator(device=dev).manual_seed(M)
        idx64 = torch.randperm(B, device=dev, generator=g)[:M].contiguous()
        idx32 = idx64.to(torch.int32)
        stats = torch.empty((8,), dtype=torch.float32, device=dev)
        keep = {}

        def run_bc(mode):
            for _ in range(calls):
                env.bc_grad(P, obs, actions, weight=weight, value_target=ret, index=idx32, mode=mode, vf_coef=vf,
                            ent_coef=ent, stats=stats)

        def run_b():
            for _ in range(calls):
                L, _ = bc_loss(theta_t, obs[idx64], actions[idx64], weight[idx64], ret[idx64], "nll", vf, ent)
                keep["grad"], = torch.autograd.grad(L, theta_t)

        def run_c():
            for _ in range(calls):
                env.ppo_grad(P, obs, actions, logp_old, adv, ret, index=idx32, clip=clip, vf_coef=vf, ent_coef=ent,
                             stats=stats)

        # (a_nll is captured last of the kernels: P.grad holds its gradient when the deviation from (b) is taken)
        variants = {"c_hg_ppo_grad": run_c, "a_hg_bc_grad_mse": lambda: run_bc("mse"),
                    "a_hg_bc_grad_nll": lambda: run_bc("nll"), "b_torch_gather_loss_backward": run_b}
        graphs = {}
        for name, fn in variants.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):   # eager warm-up on the capture stream (code objects, BLAS workspaces)
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
            if name == "a_hg_bc_grad_nll":
                keep["a"] = P.grad.clone()
        dev_rel = float(((keep["a"] - keep["grad"]).abs().max() / keep["grad"].abs().max()).cpu())
        times = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name in variants:
                graphs[name].replay()
                torch.cuda.synchronize()
                t = stamps.cpu()
                times[name].append(float(t[1] - t[0]) * 1e-2 / calls)   # 100 MHz ticks -> us per call
        med = {n: statistics.median(v) for n, v in times.items()}
        res["sizes"][str(M)] = {
            "calls_per_graph": calls,
            "us_per_call": {n: {"median": med[n], "min": min(v), "max": max(v)} for n, v in times.items()},
            "ns_per_sample": {n: med[n] * 1e3 / M for n in times},
            "ratio_a_nll_over_c": med["a_hg_bc_grad_nll"] / med["c_hg_ppo_grad"],
            "ratio_a_mse_over_c": med["a_hg_bc_grad_mse"] / med["c_hg_ppo_grad"],
            "ratio_b_over_a_nll": med["b_torch_gather_loss_backward"] / med["a_hg_bc_grad_nll"],
            "max_abs_deviation_over_max_abs_gradient": dev_rel,
            "skipped": float(stats[7].cpu())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
