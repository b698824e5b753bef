"""Time of one PPO minibatch gradient: the fused kernel against the torch route it replaces.

Stored rows: B = envs * steps samples of synthetic collection data on the device (normal observations,
actions drawn by a perturbed copy of the weights with their log-probabilities, normal advantages, returns
one unit off the critic's values), torch's default init for the 17-64-64-4 actor and its value head.
For each minibatch size M (a random int32 index of M distinct rows):

  (a) hg_ppo_grad (HeliVecEnv.ppo_grad) over the index: one gradient kernel and its reduction;
  (b) torch: gather obs / actions / logp_old / adv / ret by the same index, heligym_amd.policy.ppo_loss
      (five small GEMMs, two tanh, the clipped loss) and autograd back through it, fp32.

Method of bench_actor_critic.py: each variant is captured into one hipGraph of `calls` calls between two
hg_clock_stamp kernels; a replay's time is the stamps' difference (GPU 100 MHz clock) / calls.  Every
variant is warmed by one untimed replay; the figure is the median of --repeats replays, the variants
alternating.  (a)'s share of the fp32 matrix peak counts the matrix instructions it issues: 630
v_mfma_f32_32x32x2_f32 of 4096 flop per 64-sample tile, against 157.3 TFLOP/s.
Writes one JSON document (--out) and prints it.

usage: python scripts/bench_ppo_grad.py [--envs 65536] [--steps 25] [--repeats 7] [--out FILE]
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

MFMA_PER_TILE, FLOP_PER_MFMA, PEAK_TFLOPS = 630, 4096, 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=25, help="K: the stored rows are envs * K")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_grad.json"))
    args = ap.parse_args()

    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv
    from heligym_amd.policy import LOG_2PI, ppo_loss, ppo_views
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
        del h2, z
    theta_t = P.theta.detach().clone().requires_grad_(True)   # (b)'s leaf
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    res = {"config": {"stored_rows": B, "policy": "MLP 17-64-64-4 tanh fp32, log_std -1, value head on the trunk",
                      "clip": clip, "vf_coef": vf, "ent_coef": ent, "repeats": args.repeats,
                      "device": torch.cuda.get_device_name(0)},
           "clock": "hg_clock_stamp (100 MHz) around one hipGraph replay of `calls` calls; us per call",
           "flop_count": f"{MFMA_PER_TILE} v_mfma_f32_32x32x2_f32 x {FLOP_PER_MFMA} flop per 64-sample tile, issued; "
                         f"peak {PEAK_TFLOPS} TFLOP/s",
           "sizes": {}}
    side = torch.cuda.Stream()
    for M, calls in ((B, 1), (args.envs, 8)):
        g = torch.Generator(device=dev).manual_seed(M)
        idx64 = torch.randperm(B, device=dev, generator=g)[:M].contiguous()
        idx32 = idx64.to(torch.int32)
        stats = torch.empty((8,), dtype=torch.float32, device=dev)
        keep = {}

        def run_a():
            for _ in range(calls):
                env.ppo_grad(P, obs, actions, logp_old, adv, ret, index=idx32, clip=clip, vf_coef=vf, ent_coef=ent,
                             stats=stats)

        def run_b():
            for _ in range(calls):
                L, _ = ppo_loss(theta_t, obs[idx64], actions[idx64], logp_old[idx64], adv[idx64], ret[idx64], clip, vf,
                                ent)
                keep["grad"], = torch.autograd.grad(L, theta_t)

        variants = {"a_hg_ppo_grad": run_a, "b_torch_gather_loss_backward": run_b}
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
        dev_rel = float(((P.grad - keep["grad"]).abs().max() / keep["grad"].abs().max()).cpu())
        times = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name in variants:
                graphs[name].replay()
                torch.cuda.synchronize()
                t = stamps.cpu()
                times[name].append(float(t[1] - t[0]) * 1e-2 / calls)   # 100 MHz ticks -> us per call
        med = {n: statistics.median(v) for n, v in times.items()}
        tiles = (M + 63) // 64
        tflops = tiles * MFMA_PER_TILE * FLOP_PER_MFMA / (med["a_hg_ppo_grad"] * 1e-6) * 1e-12
        res["sizes"][str(M)] = {
            "calls_per_graph": calls,
            "us_per_call": {n: {"median": med[n], "min": min(v), "max": max(v)} for n, v in times.items()},
            "ns_per_sample": {n: med[n] * 1e3 / M for n in times},
            "ratio_b_over_a": med["b_torch_gather_loss_backward"] / med["a_hg_ppo_grad"],
            "a_issued_tflops": tflops, "a_share_of_fp32_matrix_peak": tflops / PEAK_TFLOPS,
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
