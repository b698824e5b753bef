"""Latency attribution of one step launch with a HG_TIMING=1 diagnostic build of the library
(HELIGYM_AMD_LIB=<that .so>): per-wave s_memtime stamps at phase boundaries -> median / p90 of each
phase over the recorded waves, plus the spread of wave start / end times.  --tail, with a HG_TIMING=2 build
(no phase stamps: the production schedule): how much later the last wave of a launch ends than the median
one, which wave that is, and the start offsets by XCC, over 100 consecutive graph-replayed launches.
Diagnostic only."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "heli-gym_amd"))

PHASES = ["state loads", "philox", "wind step", "ground h_c", "RK stage 1", "RK stage 2", "RK stage 3",
          "RK stage 4 + update", "wraps + template fetch", "reward/flags/post-ground",
          "flag stores + reset + obs stores", "state stores", "store drain"]
ORDER = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 11, 12]   # stamp slots in program order
# the small-batch helper kernel's stepping waves (step_help_kernel: slots 2-4 mark the hand-off)
PHASES_HELP = ["state loads", "context + stage-1 wind-free part", "wait at the hand-off barrier",
               "wind read from LDS", "RK stage 1", "RK stage 2", "RK stage 3", "RK stage 4 + update",
               "wraps + template fetch", "reward/flags/post-ground", "flag stores + reset + obs stores",
               "state stores", "store drain"]
HELPER = ["helper: state loads (counters, carry, wind state)", "helper: noise + wind step",
          "helper: LDS hand-off + barrier"]


FLAG_NAMES = {1: "reset", 2: "gear", 4: "series", 8: "sincos"}   # stage_f32.h's HG_STAGE_FLAG sites
RING, RING_WAVES = 128, 1024   # step_kernels.h: HG_TAIL_RING, HG_TAIL_WAVES


def flag_str(f):
    return "+".join(v for b, v in FLAG_NAMES.items() if f & b) or "-"


def tail(args):
    """HG_TIMING=2 build: the end of the launch in the production schedule, over `--launches` consecutive
    graph-replayed launches of bench.py's aged population (its seed, action bank and graph length)."""
    import torch
    from heligym_amd import HeliVecEnv
    n, B = args.envs, 100
    nw = (n + 63) // 64
    assert nw <= RING_WAVES and args.launches <= RING - 1
    env = HeliVecEnv(n, task="hover", dt=args.dt, seed=1234, autoreset=True)
    env.reset()
    bank = torch.empty((B, n, 4), dtype=torch.float32, device=env.device)
    for k in range(B):
        env.random_actions(bank[k], seed=0x5EED, step=k)
    for k in range(int(round(args.age_seconds / args.dt))):
        env.step_async(bank[k % B], with_reset_info=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(B):
            env.step_async(bank[k], with_reset_info=False)
    for _ in range(2 + args.launches // B):
        g.replay()
    torch.cuda.synchronize()
    buf = np.zeros((RING, RING_WAVES, 4), dtype=np.uint64)
    cnt = ctypes.c_uint32(0)
    fn = env.lib.hg_debug_tail
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint32)]
    assert fn(buf.ctypes.data, buf.nbytes, ctypes.byref(cnt)) == 0
    total = cnt.value
    ids = list(range(total - args.launches - 1, total))   # one more than reported: the gap to the next launch
    rec = np.stack([buf[L % RING, :nw] for L in ids]).astype(np.int64)
    stale = int((((rec[:, :, 2] >> 32) & 0xffffffff) != np.array(ids)[:, None]).sum())
    st, en = rec[:, :, 0] * 10.0, rec[:, :, 1] * 10.0          # ns (100 MHz)
    fl = rec[:, :, 2] & 0xffffffff
    hw, xcc = rec[:, :, 3] & 0xffffffff, (rec[:, :, 3] >> 32) & 0xf
    cu = ((hw >> 13) & 7) * 100 + ((hw >> 12) & 1) * 16 + ((hw >> 8) & 15)   # SE * 100 + SH * 16 + CU
    t0 = st.min(axis=1, keepdims=True)
    so, eo, life = st - t0, en - t0, en - st
    print(f"launch tail, HG_TIMING=2: {n} envs, {nw} waves, launches {ids[0]}..{ids[-2]} of {total} "
          f"(graph-replayed, {B} per graph); records of another launch: {stale}")
    print(f"wave life median {np.median(life[:-1])/1e3:.2f} p90 {np.percentile(life[:-1], 90)/1e3:.2f} "
          f"max {life[:-1].max()/1e3:.2f} us; start offset p50 {np.median(so[:-1])/1e3:.2f} p90 "
          f"{np.percentile(so[:-1], 90)/1e3:.2f} max {so[:-1].max()/1e3:.2f} us")
    print("per launch: last end - median end (us) | the last-ending wave: tile xcc cu flags start-offset life (us) "
          "| waves starting > 0.4 us late, their XCCs | next launch's first start - last end (us)")
    tails, late_x, last_rows = [], [], []
    for j in range(len(ids) - 1):
        w = int(np.argmax(eo[j]))
        tl = eo[j, w] - np.median(eo[j])
        late = so[j] > 400.0
        gap = st[j + 1].min() - en[j].max()
        tails.append(tl)
        late_x.append(xcc[j][late])
        last_rows.append((int(fl[j, w]), so[j, w], int(xcc[j, w]), life[j, w]))
        print(f"  {ids[j]:6d}: {tl/1e3:5.2f} | {w:4d} {int(xcc[j, w])} {int(cu[j, w]):3d} {flag_str(int(fl[j, w])):18s} "
              f"{so[j, w]/1e3:5.2f} {life[j, w]/1e3:5.2f} | {int(late.sum()):3d} {sorted(set(xcc[j][late].tolist()))} | {gap/1e3:5.2f}")
    tails = np.array(tails)
    print(f"last end - median end over {len(tails)} launches: median {np.median(tails)/1e3:.2f} p90 "
          f"{np.percentile(tails, 90)/1e3:.2f} max {tails.max()/1e3:.2f} us; launch length (first start to last end) "
          f"median {np.median(eo[:-1].max(axis=1))/1e3:.2f} us; period (first start to next first start) median "
          f"{np.median(np.diff(st.min(axis=1)))/1e3:.2f} us")
    lf = np.array([r[0] for r in last_rows])
    ls = np.array([r[1] for r in last_rows])
    print("the last-ending wave: " + ", ".join(f"{flag_str(f)} {int((lf == f).sum())}" for f in sorted(set(lf.tolist())))
          + f"; started > 0.4 us late in {int((ls > 400).sum())} launches; on XCC "
          + ", ".join(f"{x}: {c}" for x, c in sorted(zip(*np.unique([r[2] for r in last_rows], return_counts=True)))))
    print("by XCC (medians over the launches): waves | start offset min / median / max (us) | end offset median / max "
          "| life median | late starters per launch | next launch's first start (any XCC) - this XCC's last end")
    for x in sorted(set(xcc.reshape(-1).tolist())):
        m = xcc == x
        per = lambda a, f: np.median([f(a[j][m[j]]) for j in range(len(ids) - 1)]) / 1e3   # noqa: E731
        gapx = np.median([st[j + 1].min() - en[j][m[j]].max() for j in range(len(ids) - 1)]) / 1e3
        nlate = np.median([int((so[j][m[j]] > 400.0).sum()) for j in range(len(ids) - 1)])
        print(f"  xcc {x}: {int(m[0].sum()):4d} | {per(so, np.min):5.2f} {per(so, np.median):5.2f} {per(so, np.max):5.2f} | "
              f"{per(eo, np.median):5.2f} {per(eo, np.max):5.2f} | {per(life, np.median):5.2f} | {nlate:5.1f} | {gapx:5.2f}")
    # the start offset against the dispatch order inside an XCC (tile // number of XCCs, round-robin workgroups)
    nx = len(set(xcc[0].tolist()))
    order = np.arange(nw) // max(nx, 1)
    q = np.linspace(0, order.max() + 1, 5).astype(int)
    print("start offset by dispatch order inside the XCC (tile // XCCs), median over waves and launches: "
          + ", ".join(f"{q[k]}-{q[k + 1] - 1}: {np.median(so[:-1][:, (order >= q[k]) & (order < q[k + 1])])/1e3:.2f} us"
                      for k in range(4)))
    for cls, sel in (("no flag", fl[:-1] == 0), ("reset", (fl[:-1] & 1) != 0), ("gear", (fl[:-1] & 2) != 0),
                     ("long series", (fl[:-1] & 4) != 0), ("full sincos", (fl[:-1] & 8) != 0)):
        if sel.any():
            print(f"  {cls:12s} {sel.sum() / (len(ids) - 1):7.1f} waves per launch: life median {np.median(life[:-1][sel])/1e3:.2f} "
                  f"p90 {np.percentile(life[:-1][sel], 90)/1e3:.2f} max {life[:-1][sel].max()/1e3:.2f} us")
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=3000, help="steps before the recorded launch (aged population)")
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--tail", action="store_true", help="a HG_TIMING=2 build: the launch-tail report")
    ap.add_argument("--launches", type=int, default=100, help="--tail: consecutive launches reported")
    ap.add_argument("--age-seconds", type=float, default=60.0, help="--tail: simulated time before the recording")
    args = ap.parse_args()
    if args.tail:
        return tail(args)
    import torch
    from heligym_amd import HeliVecEnv
    env = HeliVecEnv(args.envs, task="hover", dt=args.dt, seed=0)
    env.reset()
    act = torch.empty((args.envs, 4), dtype=torch.float32, device=env.device)
    for k in range(args.warm):
        env.random_actions(act, seed=1, step=k)
        env.step_async(act, with_reset_info=False)
    torch.cuda.synchronize()
    buf = np.zeros((2048, 17), dtype=np.uint64)
    fn = env.lib.hg_debug_timing
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    assert fn(buf.ctypes.data, buf.nbytes) == 0
    nw = min(2048, args.envs // 64)
    t = buf[:nw, ORDER].astype(np.int64)
    rt = buf[:nw, 14:16].astype(np.int64)        # [end, start] s_memrealtime (100 MHz)
    span_cyc = (t[:, -1] - t[:, 0]).astype(np.float64)
    span_ns = (rt[:, 0] - rt[:, 1]) * 10.0
    ghz = np.median(span_cyc / np.maximum(span_ns, 1))
    print(f"waves {nw}; memtime clock ~{ghz:.2f} GHz (from realtime); wave life median "
          f"{np.median(span_ns)/1e3:.2f} us p90 {np.percentile(span_ns, 90)/1e3:.2f} us")
    starts = (rt[:, 1] - rt[:, 1].min()) * 10.0
    ends = (rt[:, 0] - rt[:, 1].min()) * 10.0
    print(f"wave start spread: p50 {np.median(starts)/1e3:.2f} us p90 {np.percentile(starts, 90)/1e3:.2f} "
          f"max {starts.max()/1e3:.2f} us; last wave end {ends.max()/1e3:.2f} us")
    d = np.diff(t, axis=1).astype(np.float64) / ghz / 1e3   # us
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    helper = args.envs <= 64 * 4 * cus // 2   # heligym_amd.hip launch_step: HG_HELPER_DIV = 2
    if helper:
        hb = np.zeros((2048, 5), dtype=np.uint64)
        fh = env.lib.hg_debug_timing_help
        fh.argtypes = [ctypes.c_void_p, ctypes.c_int64]
        assert fh(hb.ctypes.data, hb.nbytes) == 0
        h = hb[:nw].astype(np.int64)
        hd = np.diff(h[:, 1:5], axis=1).astype(np.float64) / ghz / 1e3
        hstart = (h[:, 0] - rt[:, 1].min()) * 10.0
        print(f"helper waves: start p50 {np.median(hstart)/1e3:.2f} us (stepping waves {np.median(starts)/1e3:.2f}); "
              f"life to the barrier median {np.median((h[:, 4] - h[:, 1]) / ghz) / 1e3:.2f} us")
        for j, name in enumerate(HELPER):
            print(f"  {name:48s} median {np.median(hd[:, j]):6.3f} us   p90 {np.percentile(hd[:, j], 90):6.3f} us")
        print("stepping waves:")
    for j, name in enumerate(PHASES_HELP if helper else PHASES):
        print(f"  {name:24s} median {np.median(d[:, j]):6.3f} us   p90 {np.percentile(d[:, j], 90):6.3f} us   "
              f"max {d[:, j].max():6.3f} us")
    # which wave-uniform branches the waves took, and how long those waves lived
    fl = buf[:nw, 16].astype(np.int64)
    names = {1: "reset", 2: "gear contact", 4: "full sincos"}
    print(f"branch flags: " + ", ".join(f"{v} {int(((fl & b) != 0).sum())} waves" for b, v in names.items()))
    for cls, sel in (("no branch", fl == 0), ("reset only", fl == 1), ("gear", (fl & 2) != 0),
                     ("full sincos", (fl & 4) != 0)):
        if sel.any():
            print(f"  {cls:12s} {int(sel.sum()):5d} waves: life median {np.median(span_ns[sel])/1e3:.2f} us, "
                  f"max {span_ns[sel].max()/1e3:.2f} us; end median {np.median(ends[sel])/1e3:.2f} max {ends[sel].max()/1e3:.2f} us")
    last = np.argsort(ends)[-20:]
    print("the 20 last-ending waves: flags", fl[last].tolist(), "start", np.round(starts[last] / 1e3, 2).tolist())
    env.close()


if __name__ == "__main__":
    main()
