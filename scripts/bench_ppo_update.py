"""Time of a PPO update phase: hg_ppo_update against the route it replaces and against its floor.

Stored rows: B = envs * steps samples of synthetic collection data on the device (bench_ppo_grad.py's), torch's
default init for the 17-64-64-4 actor and its value head.  One update = epochs x minibatches optimiser steps:

  (a) hg_ppo_update (HeliVecEnv.ppo_update): per epoch a device shuffle, per minibatch the gradient kernel, its
      reduction and the optimiser kernel (gradient-norm clipping on, KL stop off);
  (b) the route of examples/ppo_train.py: torch.randperm -> int32 chunks -> .contiguous() -> HeliVecEnv.ppo_grad ->
      clip_grad_norm_ -> fused torch.optim.Adam over the nine parameter views; timed eager, as the example runs
      it, and captured into a graph (Adam capturable=True) if the capture succeeds;
  (c) epochs x minibatches bare HeliVecEnv.ppo_grad calls on fixed index slices: the floor.

Clock: hg_clock_stamp (the GPU's 100 MHz clock) before and after the update on the same stream; for the
captured variants the stamps are part of the graph, for (b) eager they are launched around the eager calls, so
the interval holds the host's launch gaps as the example's run does.  Every variant is warmed once; the figure
is the median of --repeats, the variants alternating.  Writes one JSON document (--out) and prints it.

usage: python scripts/bench_ppo_update.py [--envs 4096] [--steps 64] [--epochs 4] [--minibatches 4] [--repeats 9]
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
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64, help="K: the stored rows are envs * K")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update.json"))
    args = ap.parse_args()

    import torch
    from heligym_amd import ActorCriticParams, HeliVecEnv, PPOOptState
    from heligym_amd.policy import LOG_2PI, ppo_views
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = "cuda:0"
    B, E, NMB = args.envs * args.steps, args.epochs, args.minibatches
    steps = E * NMB
    clip, vf, ent, lr, max_norm = 0.2, 0.5, 0.01, 3e-4, 0.5
    env = HeliVecEnv(64, task="hover", dt=0.01, device=dev, seed=1)   # the handle: device and error convention only
    lib = env.lib
    nn = torch.nn

    def make_params():
        torch.manual_seed(0)
        actor = nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4)).to(dev)
        return ActorCriticParams(actor, nn.Linear(64, 1).to(dev), nn.Parameter(torch.full((4,), -1.0, device=dev)))

    Pa, Pb, Pbg, Pc = (make_params() for _ in range(4))
    with torch.no_grad():
        obs = torch.randn((B, 17), device=dev)
        p = ppo_views(Pa.theta + 0.02 * torch.randn_like(Pa.theta))
        h2 = torch.tanh(torch.tanh(obs @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"])
        z = torch.randn((B, 4), device=dev)
        actions = (h2 @ p["W3"].T + p["b3"] + torch.exp(p["log_std"]) * z).contiguous()
        logp_old = -0.5 * (z * z).sum(-1) - p["log_std"].sum() - 2 * LOG_2PI
        adv = torch.randn((B,), device=dev)
        ret = h2 @ p["w_v"] + p["b_v"] + 1.0 + 0.5 * torch.randn((B,), device=dev)
        del h2, z
    rows = (obs, actions, logp_old, adv, ret)
    kw = dict(clip=clip, vf_coef=vf, ent_coef=ent)
    stamps = torch.zeros((2,), dtype=torch.int64, device=dev)

    def stamp(j):
        if lib.hg_clock_stamp(ctypes.c_void_p(stamps[j:j + 1].data_ptr()), env._stream()) != 0:
            raise RuntimeError("hg_clock_stamp failed")

    state = PPOOptState(dev)
    stats_a = torch.empty((steps, 8), dtype=torch.float32, device=dev)
    index_a = torch.empty((B,), dtype=torch.int32, device=dev)

    def run_a():
        env.ppo_update(Pa, state, *rows, epochs=E, minibatches=NMB, seed=3, lr=lr, max_grad_norm=max_norm, stats=stats_a,
                       index=index_a, **kw)

    stats_b = torch.empty((8,), dtype=torch.float32, device=dev)

    def route_b(P, opt):
        for _ in range(E):
            for idx in torch.randperm(B, device=dev).to(torch.int32).chunk(NMB):
                idx = idx.contiguous()
                env.ppo_grad(P, *rows, index=idx, stats=stats_b, **kw)
                torch.nn.utils.clip_grad_norm_(P.parameters(), max_norm)
                opt.step()

    opt_b = torch.optim.Adam(Pb.parameters(), lr=lr, fused=True)
    opt_bg = torch.optim.Adam(Pbg.parameters(), lr=lr, fused=True, capturable=True)
    fixed = torch.randperm(B, device=dev).to(torch.int32)
    cuts = [j * B // NMB for j in range(NMB + 1)]

    def run_c():
        for _ in range(E):
            for j in range(NMB):
                env.ppo_grad(Pc, *rows, index=fixed[cuts[j]:cuts[j + 1]], stats=stats_b, **kw)

    side = torch.cuda.Stream()

    def capture(fn):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # eager warm-up on the capture stream (code objects, optimiser state)
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            stamp(0)
            fn()
            stamp(1)
        gr.replay()   # untimed
        torch.cuda.synchronize()
        return gr

    def eager(fn):
        def run():
            stamp(0)
            fn()
            stamp(1)
        return run

    def measure(variants, times):
        for _ in range(args.repeats):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                fn()
                torch.cuda.synchronize()
                t = stamps.cpu()
                times.setdefault(name, []).append(float(t[1] - t[0]) * 1e-2)   # 100 MHz ticks -> us per update

    def report(times, b_capture_error):
        med = {n: statistics.median(v) for n, v in times.items()}
        a, c = med["a_hg_ppo_update_graph"], med["c_bare_ppo_grad_graph"]
        res = {"config": {"stored_rows": B, "epochs": E, "minibatches": NMB, "optimiser_steps_per_update": steps,
                          "minibatch_rows": B // NMB, "clip": clip, "vf_coef": vf, "ent_coef": ent, "lr": lr,
                          "max_grad_norm": max_norm, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)},
               "clock": "hg_clock_stamp (100 MHz) before and after one update on the same stream; us per update",
               "us_per_update": {n: {"median": med[n], "min": min(v), "max": max(v)} for n, v in times.items()},
               "us_per_minibatch": {n: med[n] / steps for n in times},
               "a_over_c": a / c,
               "a_minus_c_us_per_minibatch": (a - c) / steps,
               "b_eager_over_a": med["b_torch_route_eager"] / a,
               "b_graph_over_a": med["b_torch_route_graph"] / a if "b_torch_route_graph" in med else None,
               "b_graph_capture_error": b_capture_error,
               "a_counters_after": state.counters()}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return res

    graph_a = capture(run_a)
    variants = {"a_hg_ppo_update_graph": graph_a.replay, "c_bare_ppo_grad_graph": capture(run_c).replay}
    route_b(Pb, opt_b)   # warm-up
    variants["b_torch_route_eager"] = eager(lambda: route_b(Pb, opt_b))
    times = {}
    measure(variants, times)
    res = report(times, "not attempted yet")
    # (b) captured, last: the file above stands if the route cannot be captured; timed alternating with (a) again
    try:
        graph_b = capture(lambda: route_b(Pbg, opt_bg))
        measure({"a_hg_ppo_update_graph": graph_a.replay, "b_torch_route_graph": graph_b.replay}, times)
        res = report(times, None)
    except Exception as e:
        res = report(times, f"{type(e).__name__}: {e}"[:400])
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
