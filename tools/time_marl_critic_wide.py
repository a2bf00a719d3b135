#!/usr/bin/env python3
"""Time the SAC twin critic at 16 vehicles, (state, action) = (80, 288) with 1024-512-256: the chunked MFMA launch
(`BatchedTwinCritic(gemm="wide")`, `risvec_marl_critic_wide`) against the same computation with library kernels
(`gemm="library"`: torch.cat + torch.nn.functional, the default at this shape), by the method of tools/time_marl_critic.py
-- interleaved in one process, HIP events, medians of rounds -- for `forward` and `td_target` with FROZEN weights, and for
the learner's loop, blend -> pack -> `td_target` (`soft_update_from` marks both streams stale, the next `td_target` rebuilds
them), with `pack = "device"` against `pack = "host"` on wide objects and against the library mode, which packs nothing.

    python tools/time_marl_critic_wide.py [--out profiles/marl_critic_wide.json] [--rounds 7] [--steps 50] [--warmup 20]

Every size runs in a child process of its own under a time limit; the first child that fails ends the run.  `mfma_us` is
the matrix-core issue time of the wide launch by count: MFMAs of the busiest wavefront x 32 cycles (8 passes of
v_mfma_f32_32x32x16_f16) / 2.4 GHz x the workgroups a CU runs in turn (ceil(rows / 32 / 256)).  One JSON line per size."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (80, 288, 1024, 512, 256)                # 16 vehicles, the driver's hidden sizes
ROWS = [32768, 4096, 64]
CLOCK_HZ, CUS, MFMA_CYCLES = 2.4e9, 256, 32
CHILD_LIMIT_S = 300


def mfma_count(g, n_nets=2):
    """MFMAs the busiest wavefront issues: per net its fc1 groups over all k-steps, fc2, fc3 (3 split products each)"""
    return n_nets * 3 * (-(-g.ng // 4) * g.ks + 2 * g.ng * g.mt2 + 8 * g.mt2 * g.mt3)


def child(n, rounds, steps, warmup):
    import numpy as np
    import torch
    from ris_vec_marl_amd import BatchedTwinCritic
    from ris_vec_marl_amd import _native as N
    from ris_vec_marl_amd.marl_critic import marl_critic_geom
    if not torch.cuda.is_available():
        raise SystemExit("time_marl_critic_wide needs a HIP device: a timing taken elsewhere says nothing")
    dev = "cuda:0"
    S, A = DIMS[:2]

    def nets(mode, pack="host"):
        c = BatchedTwinCritic(*DIMS, device=dev, seed=5, gemm=mode)
        for net in c.nets:
            net.Wq.mul_(8.0)
        if pack != "host":
            c.pack = pack
        return c
    cw, cl = nets("wide"), nets("library")
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(0, 1.2, (n, S)).astype(np.float32)).to(dev)
    act = torch.from_numpy(rng.uniform(0, 1, (n, A)).astype(np.float32)).to(dev)
    reward = torch.from_numpy(rng.uniform(-6, 1, n).astype(np.float32)).to(dev)
    done = torch.from_numpy(rng.uniform(size=n) < 0.01).to(dev)
    lp = torch.from_numpy(rng.uniform(-8, 4, n).astype(np.float32)).to(dev)
    li = torch.from_numpy(rng.uniform(-12, 0, n).astype(np.float32)).to(dev)
    coef = torch.tensor([0.15, 0.06], device=dev)
    q_w, q_l = [tuple(torch.empty(n, 1, device=dev) for _ in range(2)) for _ in range(2)]
    y_w, y_l = torch.empty(n, device=dev), torch.empty(n, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps

    def race(forms):
        for fn in forms.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in forms}
        for _ in range(rounds):                                # interleaved: what drifts, drifts for all
            for k, fn in forms.items():
                us[k].append(timed(fn))
        return us
    row = dict(rows=n, S=S, A=A, dims=list(DIMS), n_nets=2, steps_per_form=rounds * steps, warmup=warmup)
    us = race({"wide": lambda: cw.forward(x, act, out=q_w), "library": lambda: cl.forward(x, act, out=q_l)})
    row["kernel"] = (cw.forward(x, act, out=q_w), N.last_kernel())[1]
    row["max_abs_q_diff"] = max(float((a - b).abs().max()) for a, b in zip(q_w, q_l))
    us.update({"td_" + k: v for k, v in race({
        "wide": lambda: cw.td_target(reward, x, act, done, 0.99, lp, li, coef, out=y_w),
        "library": lambda: cl.td_target(reward, x, act, done, 0.99, lp, li, coef, out=y_l)}).items()})
    row["max_abs_y_diff"] = float((y_w - y_l).abs().max())
    # the learner's loop: blend both target nets towards the online ones, then the target from the blended weights
    online = nets("library")
    loops = {"device": nets("wide", "device"), "host": nets("wide"), "library": nets("library")}

    def loop(c):
        def fn():
            c.soft_update_from(online, tau=0.005)
            c.td_target(reward, x, act, done, 0.99, lp, li, coef, out=y_w)
        return fn
    us.update({"loop_" + k: v for k, v in race({k: loop(c) for k, c in loops.items()}).items()})
    assert loops["device"].packs == loops["host"].packs > 2 * rounds * steps and loops["library"].packs == 0
    for k, v in us.items():
        row["%s_us" % k] = round(sorted(v)[len(v) // 2], 2)
        row["%s_us_rounds" % k] = [round(t, 2) for t in v]
    for pre, new, old in (("", "wide", "library"), ("td_", "td_wide", "td_library"), ("loop_device_vs_host_", "loop_device", "loop_host"),
                          ("loop_device_vs_library_", "loop_device", "loop_library")):
        f, l = us[new], us[old]
        row[pre + "speedup"] = round(row[old + "_us"] / row[new + "_us"], 2)
        row[pre + "speedup_rounds"] = [round(min(l) / max(f), 2), round(max(l) / min(f), 2)]      # the spread between rounds
        row[pre + "faster_every_round"] = all(a < b for a, b in zip(f, l))
        row[pre + "faster_by_more_than_the_spread"] = max(f) < min(l)
    g = marl_critic_geom(*DIMS)
    turns = -(-((n + 31) // 32) // CUS)
    row["mfma_per_wavefront"] = mfma_count(g)
    row["mfma_us"] = round(mfma_count(g) * MFMA_CYCLES * turns / CLOCK_HZ * 1e6, 2)
    row["mfma_share"] = round(row["mfma_us"] / row["wide_us"], 3)
    row["weight_stream_bytes"] = 2 * g.rows * 1024
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", type=int, default=None, metavar="ROWS")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.rounds, args.steps, args.warmup)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_marl_critic_wide needs a HIP device: a timing taken elsewhere says nothing")
    results = []
    for n in ROWS:                                             # a fresh process per size, each under its own limit
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--steps", str(args.steps),
                              "--warmup", str(args.warmup), "--child", str(n)], capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        if out.returncode != 0:
            raise SystemExit("%d rows failed with status %d; nothing further is run\n%s" % (n, out.returncode, out.stderr[-2000:]))
        line = out.stdout.strip().splitlines()[-1]
        results.append(json.loads(line))
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/time_marl_critic_wide.py", sizes=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
