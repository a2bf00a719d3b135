#!/usr/bin/env python3
"""Time the fused 3GPP step family (HIP events, device-resident inputs, bound launchers) against the forms it replaces,
alternating the forms in one process:
  single step   k_step_3gpp<VP>            vs  update_channel_gains() (k_gain_3gpp) + step(fused=False) (k_step<VP>)
  T-step        k_step_3gpp<VP,MULTI>      vs  the cached T-step k_step_multi<VP> (gains not refreshed)
    python tools/time_step_3gpp.py [n_envs] [n_veh] [n_ris] [multi_envs] [T]
Event times include the host's launch cadence; per-kernel times come from a rocprofv3 --kernel-trace --stats run."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import VecEnviron, apply_yaml_config, reference_lanes  # noqa: E402

E, V, M, EM, T = (int(x) for x in (sys.argv[1:6] + ["32768", "8", "64", "4096", "32"][len(sys.argv) - 1:]))
DEV = "cuda:0"


def bytes_per_env(V, metrics=True, power_w=True, obs=True, policy_action=False, injected_arrivals=False,
                  injected_fading=False, gain_in=False):
    """HBM bytes one env moves in one step of k_step_3gpp (gain_in=True: k_step on cached gains, no position)."""
    rd = 8 * V + 4 * V + 4 * V + 4 + 4 + 4 * V         # action, data_buf, partner, n_groups, mec_q, pl
    rd += 4 * V if gain_in else 16 * V                  # cached gain | position (two float64)
    rd += 4 * V if injected_arrivals else 0
    rd += 12 * V if injected_fading else 0
    wr = 4 * V * 6 + 4 * (0 if gain_in else V) + 4   # data_buf rate data_t data_p reward over_power (+ gain), mec_q
    wr += 20 * V if obs else 0
    wr += 64 if metrics else 0
    wr += 8 * V if power_w else 0
    return rd + wr


def make(n):
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3, n_envs=n,
                     device=DEV, seed=3)
    apply_yaml_config(env, None)
    env.channel_model = "3gpp_umi"
    env.make_new_game()
    env.renew_positions()
    return env


def inputs(n, steps=None):
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    shape = (n, 2, V) if steps is None else (steps, n, 2, V)
    act = torch.rand(shape, device=DEV, generator=g)
    pt = torch.full((n, V), -1, dtype=torch.int32, device=DEV)
    pt[:, 0], pt[:, 1] = 1, 1 << 16
    ng = torch.full((n,), V - 1, dtype=torch.int32, device=DEV)
    return act, pt, ng


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def best_of(forms, reps, rounds):
    for f in forms.values():                            # warm-up
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in forms}
    for _ in range(rounds):                             # alternate the forms
        for k, f in forms.items():
            best[k] = min(best[k], timed(f, reps))
    return {k + "_us": round(v, 2) for k, v in best.items()}


out = {"E": E, "V": V, "M": M, "model": "3gpp_umi"}
env = make(E)
act, pt, ng = inputs(E)
fused = env.bind_step(act, pt, ng, fused=True)
cached = env.bind_step(act, pt, ng, fused=False)


def two_launch():
    env.update_channel_gains()
    cached()


out.update(best_of({"fused_3gpp": fused, "gain_3gpp_plus_step": two_launch, "gain_3gpp": env.update_channel_gains,
                    "cached_step": cached}, 100, 5))
out["bytes_per_env_fused"] = bytes_per_env(V)
out["bytes_per_env_cached_step"] = bytes_per_env(V, gain_in=True)
out["fused_3gpp_GBps"] = round(out["bytes_per_env_fused"] * E / out["fused_3gpp_us"] / 1e3, 1)

envm = make(EM)
actm, ptm, ngm = inputs(EM, T)
rec = {k: torch.empty(s, device=DEV) for k, s in (("reward", (T, EM, V)), ("obs", (T, EM, V, 5)), ("metrics", (T, EM, 16)))}
multi3 = envm.bind_step_many(actm, ptm, ngm, out=rec, fused=True)
multic = envm.bind_step_many(actm, ptm, ngm, out=rec, fused=False)
m = best_of({"multi_3gpp": multi3, "multi_cached": multic}, 20, 5)
out.update({"multi_E": EM, "T": T})
out.update({k.replace("_us", "_us_per_step"): round(v / T, 3) for k, v in m.items()})
print(json.dumps(out))
