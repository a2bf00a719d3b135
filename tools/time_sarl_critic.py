#!/usr/bin/env python3
"""Time the DDPG critic forward (`BatchedCritic.forward`) and the whole TD target (`ddpg_td_target`: target actor +
target critic with the epilogue): the hand-written MFMA launches (`gemm="fused"`) against the same computation with
library kernels (`gemm="library"`: torch.nn.functional, what the reference's networks run as), interleaved in one
process, HIP events, median of rounds.  FROZEN weights: the host pack of the weight stream is timed separately
(`pack_us`, wall clock with a synchronisation) -- a learner that soft-updates the target critic every step pays it per step
unless the critic packs on the device (`pack="device"`): tools/time_critic_refresh.py times that step, blend included.

    python tools/time_sarl_critic.py [--out profiles/sarl_critic.json] [--rounds 7] [--steps 50] [--warmup 20]

Every size runs in a child process of its own under a time limit; the first child that fails ends the run.
`mfma_us` is the matrix-core issue time of the fused critic by count: MFMAs per wavefront x 32 cycles (8 passes of
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

DIMS = [(8, 40)]                                # (V, M): 80/1024/512/256 with 56 actions, the driver's
ROWS = [32768, 4096, 64]
CLOCK_HZ, CUS, MFMA_CYCLES = 2.4e9, 256, 32
CHILD_LIMIT_S = 240


def mfma_count(g):
    """MFMAs the busiest wavefront of the fused critic issues: action_value, its fc1 groups, fc2, fc3 (3 split products)"""
    return 3 * (g.ksa * g.mt2 + -(-g.ng // 4) * g.ks + 2 * g.ng * g.mt2 + 8 * g.mt2 * g.mt3)


def child(V, M, n, rounds, steps, warmup):
    import numpy as np
    import torch
    from ris_vec_marl_amd import BatchedActor, BatchedCritic, ddpg_td_target
    from ris_vec_marl_amd import _native as N
    from ris_vec_marl_amd.critic import critic_geom, pack_critic_weights
    if not torch.cuda.is_available():
        raise SystemExit("time_sarl_critic needs a HIP device: a timing taken elsewhere says nothing")
    dev = "cuda:0"
    IN, A, tn = V * (M // V + 5), 2 * V + M, M // V
    dims = (IN, 1024, 512, 256, A)

    def nets(mode):
        c = BatchedCritic(IN, A, 1024, 512, 256, device=dev, seed=5, gemm=mode)
        c.Wq.mul_(100.0)
        a = BatchedActor(IN, A, 512, 256, device=dev, seed=6, gemm=mode)
        a.Wmu.mul_(60.0)
        return c, a
    (cf, af), (cl, al) = nets("fused"), nets("library")
    rng = np.random.default_rng(1)
    o = np.empty((n, V, tn + 5), np.float32)
    o[:, :, :tn] = rng.uniform(0, 2 * np.pi, (n, V, tn))
    o[:, :, tn:] = rng.uniform(0, 1.2, (n, V, 5))
    x = torch.from_numpy(o).to(dev)
    act = torch.from_numpy(rng.uniform(-0.999, 0.999, (n, A)).astype(np.float32)).to(dev)
    reward = torch.from_numpy(rng.uniform(-6, 1, n).astype(np.float32)).to(dev)
    done = torch.from_numpy(rng.uniform(size=n) < 0.01).to(dev)
    q_f, q_l = torch.empty(n, 1, device=dev), torch.empty(n, 1, device=dev)
    y_f, y_l, a_f, a_l = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, A, device=dev), torch.empty(n, A, device=dev)

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
    row = dict(rows=n, V=V, M=M, dims=list(dims), steps_per_form=rounds * steps, warmup=warmup, weights="frozen")
    us = race({"fused": lambda: cf.forward(x, act, out=q_f), "library": lambda: cl.forward(x, act, out=q_l)})
    row["kernel"] = (cf.forward(x, act, out=q_f), N.last_kernel())[1]
    row["max_abs_q_diff"] = float((q_f - q_l).abs().max())
    us.update({"td_" + k: v for k, v in race({
        "fused": lambda: ddpg_td_target(af, cf, x, reward, done, 0.99, out=y_f, actions_=a_f),
        "library": lambda: ddpg_td_target(al, cl, x, reward, done, 0.99, out=y_l, actions_=a_l)}).items()})
    row["max_abs_y_diff"] = float((y_f - y_l).abs().max())
    for k, v in us.items():
        row["%s_us" % k] = round(sorted(v)[len(v) // 2], 2)
        row["%s_us_rounds" % k] = [round(t, 2) for t in v]
    for pre in ("", "td_"):
        f, l = us[pre + "fused"], us[pre + "library"]
        row[pre + "speedup"] = round(row[pre + "library_us"] / row[pre + "fused_us"], 2)
        row[pre + "fused_faster_every_round"] = all(a < b for a, b in zip(f, l))
        row[pre + "fused_faster_by_more_than_the_spread"] = max(f) < min(l)
    g = critic_geom(*dims)
    turns = -(-((n + 31) // 32) // CUS)
    row["mfma_per_wavefront"] = mfma_count(g)
    row["mfma_us"] = round(mfma_count(g) * MFMA_CYCLES * turns / CLOCK_HZ * 1e6, 2)
    row["mfma_share"] = round(row["mfma_us"] / row["fused_us"], 3)
    row["weight_stream_bytes"] = g.rows * 1024
    ws = tuple(getattr(cf, k) for k in cf._PACKED)
    packs = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pack_critic_weights(*ws)
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
    ap.add_argument("--child", nargs=3, type=int, default=None, metavar=("V", "M", "ROWS"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child, args.rounds, args.steps, args.warmup)
    results, device = [], None
    for V, M in DIMS:
        for n in ROWS:                                         # a fresh process per size, each under its own limit
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--steps", str(args.steps),
                                  "--warmup", str(args.warmup), "--child", str(V), str(M), str(n)], capture_output=True, text=True,
                                 timeout=CHILD_LIMIT_S)
            if out.returncode != 0:
                raise SystemExit("size (%d, %d) x %d failed with status %d; nothing further is run\n%s"
                                 % (V, M, n, out.returncode, out.stderr[-2000:]))
            line = out.stdout.strip().splitlines()[-1]
            results.append(json.loads(line))
            print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/time_sarl_critic.py", sizes=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
