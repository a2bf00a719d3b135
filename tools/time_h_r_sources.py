#!/usr/bin/env python3
"""Time the bound fused step (HIP events, device-resident inputs) with each h_r source the software pipeline has:
  read     h_r touched through torch after compute_parms() (`tensors["h_r"].mul_(1)`): the env stops sending
           RISVEC_STEP_H_R_STEER_CURRENT and the kernel reads the rows -- the path every caller that writes h_r by hand
           stays on
  rebuild  h_r as compute_parms() left it: the pipeline's GEN member makes the rows from steer_ang / z_r (24 bytes per
           vehicle instead of 8 M)
    python tools/time_h_r_sources.py [--waves N] [--forward] [n_envs] [n_veh] [n_ris] [reps] [rounds]
ONE env and one h_r allocation, both sources alternating round by round: compute_parms() gives the rebuilding source,
`tensors["h_r"].mul_(1)` after it the reading one, the same h_r bits every time.  theta is read by index in both.
--waves N forces the pipeline's wavefront count (RisVecForce::pipe_waves) for both sources: the knob the GEN member's
waves per CU were chosen with.  --forward pins the walk forward for both (RisVecForce::pipe_rev off).  Prints one JSON
line: per source the median / min / max over `rounds` of the mean step time of `reps` launches, the kernel name and what
risvec_last_h_r_rebuilt() said."""
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.environ.get("RISVEC_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import VecEnviron, apply_yaml_config, reference_lanes  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402

FORWARD = "--forward" in sys.argv[1:]
ARGV = [x for x in sys.argv[1:] if x != "--forward"]
WAVES = 0
if "--waves" in ARGV:
    i = ARGV.index("--waves")
    WAVES = int(ARGV[i + 1])
    ARGV = ARGV[:i] + ARGV[i + 2:]
E, V, M, REPS, ROUNDS = (int(x) for x in (ARGV[:5] + ["32768", "8", "64", "500", "9"][len(ARGV):]))
DEV = "cuda:0"


def make():
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3, n_envs=E,
                     device=DEV, seed=3)
    apply_yaml_config(env, None)
    env.make_new_game()
    env.renew_positions()
    env.compute_parms()
    env.Random_phase()
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    act = torch.rand((E, 2, V), device=DEV, generator=g)
    pt = torch.full((E, V), -1, dtype=torch.int32, device=DEV)
    pt[:, 0], pt[:, 1] = 1, 1 << 16
    ng = torch.full((E,), V - 1, dtype=torch.int32, device=DEV)
    return env, env.bind_step(act, pt, ng, None, fused=True, metrics=True, power_w=False, obs=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


def main():
    env, fn = make()

    def source(k):                                     # the same h_r bits either way
        env.compute_parms()
        if k == "read":
            env.tensors["h_r"].mul_(1)

    us = {"read": [], "rebuild": []}
    info = {}
    force = dict(pipe_waves=WAVES) if WAVES else {}
    if FORWARD:
        force["pipe_rev"] = False
    with (N.forced(**force) if force else contextlib.nullcontext()):
        for k in us:
            source(k)
            for _ in range(20):
                fn()
            info[k] = dict(kernel=N.last_kernel(), rebuilt=N.last_h_r_rebuilt(), by_index=N.last_theta_by_index())
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for k in us:
                source(k)
                fn()                                   # the first launch after the h_r write is not part of the window
                us[k].append(timed(fn))
    out = dict(E=E, V=V, M=M, reps=REPS, rounds=ROUNDS, pipe_waves=WAVES, forward=FORWARD)
    for k in us:
        out[k] = dict(info[k], us_median=round(statistics.median(us[k]), 3), us_min=round(min(us[k]), 3),
                      us_max=round(max(us[k]), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
