#!/usr/bin/env python3
"""Time the bound fused step (HIP events, device-resident inputs) with each theta source the software pipeline has:
  tensor   theta touched through torch after Random_phase (`tensors["theta"].mul_(1)`): the env drops the indices and
           the kernel reads the complex64 tensor -- the path every caller that writes theta by hand stays on
  index    indices current (Random_phase wrote both): RISVEC_STEP_THETA_IDX_CURRENT, 1 byte per element
    python tools/time_theta_sources.py [--one-env] [n_envs] [n_veh] [n_ris] [reps] [rounds]
Default: two envs, one per source -- fine while the stream is cache-resident.  --one-env, for streams beyond the Infinity
Cache: both sources are timed on the SAME env and the same h_r allocation, alternating round by round -- `Random_phase(idx)`
with one fixed injected index tensor gives the index source, `tensors["theta"].mul_(1)` after it the tensor source, the
same theta bits every time.  Such streams run at one of two levels about 8 % apart depending on the h_r allocation, which
is the size of the gain looked for: two envs (or two processes) cannot tell it from that lottery.
Prints one JSON line: per source the median / min / max over `rounds` of the mean step time of `reps` launches, the kernel
name and what risvec_last_theta_by_index() said.  RISVEC_TREE=<checkout> times that tree's package instead (a tree from
before the by-index reader reports the tensor source twice: the same-box A/B of the tensor path)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.environ.get("RISVEC_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import VecEnviron, apply_yaml_config, reference_lanes  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402

ONE_ENV = "--one-env" in sys.argv[1:]
ARGV = [x for x in sys.argv[1:] if x != "--one-env"]
E, V, M, REPS, ROUNDS = (int(x) for x in (ARGV[:5] + ["32768", "8", "64", "500", "9"][len(ARGV):]))
DEV = "cuda:0"


def make(touch):
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3, n_envs=E,
                     device=DEV, seed=3)
    apply_yaml_config(env, None)
    env.make_new_game()
    env.renew_positions()
    env.compute_parms()
    env.Random_phase()
    if touch:
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


def report(us, info, **extra):
    out = dict(E=E, V=V, M=M, reps=REPS, rounds=ROUNDS, **extra)
    for k in us:
        out[k] = dict(info[k], us_median=round(statistics.median(us[k]), 3), us_min=round(min(us[k]), 3),
                      us_max=round(max(us[k]), 3))
    print(json.dumps(out))


def main_one_env():
    query = getattr(N, "last_theta_by_index", lambda: None)
    env, fn = make(False)
    idx = torch.randint(0, 8, (E, M), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(2))

    def source(k):                                     # the same theta bits either way
        env.Random_phase(idx)
        if k == "tensor":
            env.tensors["theta"].mul_(1)

    us = {"tensor": [], "index": []}
    info = {}
    for k in us:
        source(k)
        for _ in range(20):
            fn()
        info[k] = dict(kernel=N.last_kernel(), by_index=query())
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k in us:
            source(k)
            fn()                                       # the first launch after a theta write is not part of the window
            us[k].append(timed(fn))
    report(us, info, one_env=True)


def main():
    if ONE_ENV:
        return main_one_env()
    query = getattr(N, "last_theta_by_index", lambda: None)
    cases = {"tensor": make(True), "index": make(False)}
    us = {k: [] for k in cases}
    info = {}
    for k, (_, fn) in cases.items():
        for _ in range(50):
            fn()
        info[k] = dict(kernel=N.last_kernel(), by_index=query())
    torch.cuda.synchronize()
    for _ in range(ROUNDS):                            # alternate the sources: drift hits both alike
        for k, (_, fn) in cases.items():
            us[k].append(timed(fn))
    report(us, info)


if __name__ == "__main__":
    main()
