#!/usr/bin/env python3
"""Time the bound fused step (HIP events, device-resident inputs) with each walk the software pipeline has, on the SAME
env and the same h_r allocation, alternating round by round:
  forward   forced(pipe_rev=False): every launch serves its envs front to back (the kernel before the backward walk)
  reverse   forced(pipe_rev=True): every launch back to front -- the same re-walk of a stream five times the L2
  rule      the dispatch rule: forward on even steps, backward on odd ones, so a launch starts on the lines the launch
            before read last
    python tools/time_pipe_walk.py [n_envs] [n_veh] [n_ris] [reps] [rounds] [--tensor]
--tensor: theta touched through torch after Random_phase, so the kernel reads the complex64 tensor instead of the
indices.  Prints one JSON line: per walk the median / min / max over `rounds` of the mean step time of `reps` launches,
the kernel name, the theta source and the walks risvec_last_pipe_walk() reported for two consecutive launches."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import VecEnviron, apply_yaml_config, reference_lanes  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402

TENSOR = "--tensor" in sys.argv[1:]
ARGV = [x for x in sys.argv[1:] if x != "--tensor"]
E, V, M, REPS, ROUNDS = (int(x) for x in (ARGV[:5] + ["32768", "8", "64", "500", "9"][len(ARGV):]))
DEV = "cuda:0"
WALKS = {"forward": N.FORCE_OFF, "reverse": N.FORCE_ON, "rule": N.BY_RULE}


def make():
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3, n_envs=E,
                     device=DEV, seed=3)
    apply_yaml_config(env, None)
    env.make_new_game()
    env.renew_positions()
    env.compute_parms()
    env.Random_phase()
    if TENSOR:
        env.tensors["theta"].mul_(1)
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
    us = {k: [] for k in WALKS}
    info = {}
    for k, rev in WALKS.items():
        with N.forced(pipe_rev=rev):
            for _ in range(20):
                fn()
            walks = []
            for _ in range(2):
                fn()
                walks.append(N.last_pipe_walk())
            info[k] = dict(kernel=N.last_kernel(), by_index=N.last_theta_by_index(), walks=walks)
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                                # alternate the walks: drift hits all alike
        for k, rev in WALKS.items():
            with N.forced(pipe_rev=rev):
                fn()
                fn()                                       # the first launches after a change of walk are not in the window
                us[k].append(timed(fn))
    out = dict(E=E, V=V, M=M, reps=REPS, rounds=ROUNDS, theta="tensor" if TENSOR else "index")
    for k in us:
        out[k] = dict(info[k], us_median=round(statistics.median(us[k]), 3), us_min=round(min(us[k]), 3),
                      us_max=round(max(us[k]), 3))
    out["rule_over_forward"] = round(out["rule"]["us_median"] / out["forward"]["us_median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
