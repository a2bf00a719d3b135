#!/usr/bin/env python3
"""Time the SAC twin critic forward (`BatchedTwinCritic.forward`) and the whole TD target (`td_target`: both nets, the
minimum, the entropy term and the select): the hand-written MFMA launch (`gemm="fused"`) against the same computation
with library kernels (`gemm="library"`: torch.cat + torch.nn.functional, what the reference's networks run as),
interleaved in one process, HIP events, median of rounds.  FROZEN weights: the host pack of the two weight streams is
timed separately (`pack_us`, wall clock with a synchronisation) -- a learner that soft-updates the target critics every
step pays it per step.

    python tools/time_marl_critic.py [--out profiles/marl_critic.json] [--rounds 7] [--steps 50] [--warmup 20]

Every size runs in a child process of its own under a time limit; the first child that fails ends the run.
`mfma_us` is the matrix-core issue time of the fused launch by count: MFMAs per wavefront x 32 cycles (8 passes of
v_mfma_f32_32x32x16_f16) / 2.4 GHz x the workgroups a CU runs in turn (ceil(rows / 32 / 256): one workgroup of four
wavefronts per 32 rows, one wavefront per SIMD); `mfma_share` = mfma_us / fused_us.  One JSON line per size."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = [(40, 80), (20, 24)]                     # (S, A) at 8 and 4 vehicles, hidden 1024-512-256: the driver's
ROWS = [32768, 4096, 64]
CLOCK_HZ, CUS, MFMA_CYCLES = 2.4e9, 256, 32
CHILD_LIMIT_S = 240


def mfma_count(g, n_nets=2):
    """MFMAs the busiest wavefront of the fused launch issues: per net its fc1 groups, fc2, fc3 (3 split products)"""
    return n_nets * 3 * (-(-g.ng // 4) * g.ks + 2 * g.ng * g.mt2 + 8 * g.mt2 * g.mt3)


def child(S, A, n, rounds, steps, warmup):
    import numpy as np
    import torch
    from ris_vec_marl_amd import BatchedTwinCritic
    from ris_vec_marl_amd import _native as N
    from ris_vec_marl_amd.marl_critic import marl_critic_geom, pack_marl_critic_weights
    if not torch.cuda.is_available():
        raise SystemExit("time_marl_critic needs a HIP device: a timing taken elsewhere says nothing")
    dev = "cuda:0"
    dims = (S, A, 1024, 512, 256)

    def nets(mode):
        c = BatchedTwinCritic(*dims, device=dev, seed=5, gemm=mode)
        for net in c.nets:
            net.Wq.mul_(8.0)
        return c
    cf, cl = nets("fused"), nets("library")
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(0, 1.2, (n, S)).astype(np.float32)).to(dev)
    act = torch.from_numpy(rng.uniform(0, 1, (n, A)).astype(np.float32)).to(dev)
    reward = torch.from_numpy(rng.uniform(-6, 1, n).astype(np.float32)).to(dev)
    done = torch.from_numpy(rng.uniform(size=n) < 0.01).to(dev)
    lp = torch.from_numpy(rng.uniform(-8, 4, n).astype(np.float32)).to(dev)
    li = torch.from_numpy(rng.uniform(-12, 0, n).astype(np.float32)).to(dev)
    coef = torch.tensor([0.15, 0.06], device=dev)
    q_f, q_l = [tuple(torch.empty(n, 1, device=dev) for _ in range(2)) for _ in range(2)]
    y_f, y_l = torch.empty(n, device=dev), torch.empty(n, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps

    def race(pair):
        for fn in pair.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in pair}
        for _ in range(rounds):                                # interleaved: what drifts, drifts for both
            for k, fn in pair.items():
                us[k].append(timed(fn))
        return us
    row = dict(rows=n, S=S, A=A, dims=list(dims), n_nets=2, steps_per_form=rounds * steps, warmup=warmup, weights="frozen")
    us = race({"fused": lambda: cf.forward(x, act, out=q_f), "library": lambda: cl.forward(x, act, out=q_l)})
    row["kernel"] = (cf.forward(x, act, out=q_f), N.last_kernel())[1]
    row["max_abs_q_diff"] = max(float((a - b).abs().max()) for a, b in zip(q_f, q_l))
    us.update({"td_" + k: v for k, v in race({
        "fused": lambda: cf.td_target(reward, x, act, done, 0.99, lp, li, coef, out=y_f),
        "library": lambda: cl.td_target(reward, x, act, done, 0.99, lp, li, coef, out=y_l)}).items()})
    row["max_abs_y_diff"] = float((y_f - y_l).abs().max())
    for k, v in us.items():
        row["%s_us" % k] = round(sorted(v)[len(v) // 2], 2)
        row["%s_us_rounds" % k] = [round(t, 2) for t in v]
    for pre in ("", "td_"):
        f, l = us[pre + "fused"], us[pre + "library"]
        row[pre + "speedup"] = round(row[pre + "library_us"] / row[pre + "fused_us"], 2)
        row[pre + "fused_faster_every_round"] = all(a < b for a, b in zip(f, l))
        row[pre + "fused_faster_by_more_than_the_spread"] = max(f) < min(l)
    g = marl_critic_geom(*dims)
    turns = -(-((n + 31) // 32) // CUS)
    row["mfma_per_wavefront"] = mfma_count(g)
    row["mfma_us"] = round(mfma_count(g) * MFMA_CYCLES * turns / CLOCK_HZ * 1e6, 2)
    row["mfma_share"] = round(row["mfma_us"] / row["fused_us"], 3)
    row["weight_stream_bytes"] = 2 * g.rows * 1024
    packs = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for net in cf.nets:
            pack_marl_critic_weights(net.W1, net.W2, net.W3)
        torch.cuda.synchronize()
        packs.append((time.perf_counter() - t0) * 1e6)
    row["pack_us"] = round(sorted(packs)[2], 1)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", nargs=3, type=int, default=None, metavar=("S", "A", "ROWS"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child, args.rounds, args.steps, args.warmup)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_marl_critic needs a HIP device: a timing taken elsewhere says nothing")
    results = []
    for S, A in DIMS:
        for n in ROWS:                                         # a fresh process per size, each under its own limit
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--steps", str(args.steps),
                                  "--warmup", str(args.warmup), "--child", str(S), str(A), str(n)], capture_output=True, text=True,
                                 timeout=CHILD_LIMIT_S)
            if out.returncode != 0:
                raise SystemExit("size (%d, %d) x %d failed with status %d; nothing further is run\n%s"
                                 % (S, A, n, out.returncode, out.stderr[-2000:]))
            line = out.stdout.strip().splitlines()[-1]
            results.append(json.loads(line))
            print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/time_marl_critic.py", sizes=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
