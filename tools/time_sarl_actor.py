#!/usr/bin/env python3
"""Time the DDPG actor forward (`BatchedActor`): the one-launch MFMA kernel (`gemm="fused"`, `risvec_sarl_actor`) against
the same forward with library kernels (`gemm="library"`: three GEMMs, two LayerNorms, ReLUs and the sigmoid), interleaved
in one process, HIP events, median of rounds.

    python tools/time_sarl_actor.py [--out FILE.json] [--rounds 7] [--steps 50] [--warmup 20]

forward     `actor.forward(x, out=mu)` on observation-shaped rows, both modes on the same weights and inputs
loop step   actor + the one-launch rollout step (`bind_sarl_rollout` with noise and ring), the actor reading the
            observation the launch wrote and writing the `mu` it reads -- the driver's whole rollout step, both ways
`mfma_us` is the matrix-core issue time of the fused kernel by count: MFMAs per wavefront x 32 cycles (8 passes of
v_mfma_f32_32x32x16_f16) / 2.4 GHz x the wavefronts a SIMD runs in turn (ceil(rows / 32 / 1024) at one wavefront per
SIMD); `mfma_share` = mfma_us / fused_us.  One JSON line per size."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedActor, OUNoise, SarlReplayBuffer, VecEnviron, reference_lanes  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402
from ris_vec_marl_amd.actor import actor_geom  # noqa: E402

DIMS = [(8, 40), (8, 64)]                       # (V, M): 80/512/256/56 and 104/512/256/80
ROWS = [32768, 4096, 64]
CLOCK_HZ, SIMDS, MFMA_CYCLES = 2.4e9, 1024, 32


def make_actor(V, M, mode):
    a = BatchedActor(V * (M // V + 5), 2 * V + M, 512, 256, device="cuda:0", seed=5, gemm=mode)
    a.Wmu.mul_(60.0)
    return a


def obs_like(n, V, tn):
    rng = np.random.default_rng(1)
    o = np.empty((n, V, tn + 5), np.float32)
    o[:, :, :tn] = rng.uniform(0, 2 * np.pi, (n, V, tn))
    o[:, :, tn:] = rng.uniform(0, 1.2, (n, V, 5))
    o[:, :, tn + 3] = 0.0
    return torch.from_numpy(o).to("cuda:0")


def loop_step(E, V, M, actor):
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                     n_envs=E, device="cuda:0", seed=3)
    env.make_new_game()
    env.compute_parms()
    A, tn = 2 * V + M, M // V
    mu = torch.zeros(E, A, device="cuda:0")
    launch = env.bind_sarl_rollout(mu, noise=OUNoise(E, A, device="cuda:0", seed=3),
                                   replay=SarlReplayBuffer(4 * E, tn + 5, A, V, device="cuda:0"))

    def run():
        actor.forward(launch.obs, out=mu)
        launch()
    return run


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def mfma_count(g):
    """MFMAs one wavefront of the fused kernel issues: two fc1 passes, fc2, the head (3 split products each)."""
    return 3 * (2 * g.ng * g.ks + g.ng * 2 * g.mt + 2 * g.mt * g.ht)


def race(pair, rounds, steps, warmup):
    for fn in pair.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in pair}
    for _ in range(rounds):                                    # interleaved: what drifts, drifts for both
        for k, fn in pair.items():
            us[k].append(timed(fn, steps))
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sarl_actor needs a HIP device: a timing taken elsewhere says nothing")
    results = []
    for V, M in DIMS:
        fused, library = make_actor(V, M, "fused"), make_actor(V, M, "library")
        IN, A, tn = V * (M // V + 5), 2 * V + M, M // V
        g = actor_geom(IN, 512, 256, A)
        for n in ROWS:
            x, mu_f, mu_l = obs_like(n, V, tn), torch.empty(n, A, device="cuda:0"), torch.empty(n, A, device="cuda:0")
            row = dict(rows=n, V=V, M=M, dims=[IN, 512, 256, A], steps_per_form=args.rounds * args.steps, warmup=args.warmup)
            us = race({"fused": lambda: fused.forward(x, out=mu_f), "library": lambda: library.forward(x, out=mu_l)},
                      args.rounds, args.steps, args.warmup)
            row["kernel"] = (fused.forward(x, out=mu_f), N.last_kernel())[1]
            row["max_abs_mu_diff"] = float((mu_f - mu_l).abs().max())
            us.update({"loop_" + k: v for k, v in race({"fused": loop_step(n, V, M, fused), "library": loop_step(n, V, M, library)},
                                                       args.rounds, args.steps, args.warmup).items()})
            for k, v in us.items():
                row["%s_us" % k] = round(sorted(v)[len(v) // 2], 2)
                row["%s_us_rounds" % k] = [round(t, 2) for t in v]
            row["speedup"] = round(row["library_us"] / row["fused_us"], 2)
            row["fused_faster_every_round"] = all(f < l for f, l in zip(us["fused"], us["library"]))
            row["loop_speedup"] = round(row["loop_library_us"] / row["loop_fused_us"], 2)
            row["loop_fused_faster_every_round"] = all(f < l for f, l in zip(us["loop_fused"], us["loop_library"]))
            row["mfma_per_wavefront"] = mfma_count(g)
            turns = -(-((n + 31) // 32) // SIMDS)
            row["mfma_us"] = round(mfma_count(g) * MFMA_CYCLES * turns / CLOCK_HZ * 1e6, 2)
            row["mfma_share"] = round(row["mfma_us"] / row["fused_us"], 3)
            row["weight_stream_bytes"] = g.items * g.rows * 1024
            results.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/time_sarl_actor.py", device=torch.cuda.get_device_name(0), sizes=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
