#!/usr/bin/env python3
"""Time the SARL rollout step (ddpg_train.py:114-185 between the actor's output and the replay buffer): the staged path
of this checkout against the one-launch form (`VecEnviron.bind_sarl_rollout`), interleaved in one process, HIP events.

    python tools/time_sarl_rollout.py [--out FILE.json] [--rounds 5] [--steps 50] [--warmup 20]

staged      OU update and noise add in torch, clamp, `sarl_action_map`, the bound `sarl_step`, `sarl_observe`, and the
            transition store as five `index_copy_` calls into a `SarlReplayBuffer`'s arrays
one launch  the same stages in `risvec_sarl_rollout` (Philox draws, ring store in the kernel)
Each is also timed without the noise stage.  One JSON line per size; `bytes_per_env_step` is the algorithmic traffic
8VM + 12M + 12A + 4V(tn+5) + 48V + 4 (+ the ring's 8V(tn+5) + 4A + 5) and `hbm_peak_fraction` what the one-launch time
makes of it against 8 TB/s."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import (OUNoise, SarlReplayBuffer, VecEnviron, reference_lanes, sarl_action_map,  # noqa: E402
                              sarl_observe)
from ris_vec_marl_amd import _native as N  # noqa: E402

SIZES = [(32768, 8, 40), (32768, 8, 64), (4096, 8, 40)]
HBM_PEAK = 8.0e12


def make_env(E, V, M):
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                     n_envs=E, device="cuda:0", seed=3)
    env.make_new_game()
    env.compute_parms()
    return env


def staged_step(E, V, M, noisy):
    """The parent's path, every tensor preallocated where torch allows it."""
    dev = torch.device("cuda:0")
    A, tn = 2 * V + M, M // V
    env = make_env(E, V, M)
    mu = torch.rand(E, A, device=dev) * 2 - 1
    x = torch.zeros(E, A, device=dev)
    power, phase = torch.empty(E, 2, V, device=dev), torch.empty(E, M, device=dev)
    step = env.bind_sarl_step(power, phase)
    rb = SarlReplayBuffer(4 * E, tn + 5, A, V, device=dev)
    ar = torch.arange(E, device=dev)
    th, dt, sg = 0.2, 1e-2, 0.15
    carry = [env.sarl_observation().clone()]

    def run(done=False):
        if noisy:
            x.mul_(1 - th * dt).add_(torch.randn_like(x), alpha=sg * math.sqrt(dt))     # noise.py:13-14 with mu = 0
            a = torch.clamp(mu + x, -0.999, 0.999)
        else:
            a = torch.clamp(mu, -0.999, 0.999)
        pw, ph = sarl_action_map(a, V, M)
        power.copy_(pw)
        phase.copy_(ph)
        step()
        obs = sarl_observe(env, phase)
        rows = (ar + rb.mem_cntr) % rb.mem_size
        rb.state_memory.index_copy_(0, rows, carry[0].view(E, -1))
        rb.action_memory.index_copy_(0, rows, a)
        rb.reward_memory.index_copy_(0, rows, env.tensors["metrics"][:, 0])
        rb.new_state_memory.index_copy_(0, rows, obs.view(E, -1))
        rb.terminal_memory.index_fill_(0, rows, bool(done))
        rb.mem_cntr += E
        carry[0] = obs

    return run


def fused_step(E, V, M, noisy):
    dev = torch.device("cuda:0")
    A, tn = 2 * V + M, M // V
    env = make_env(E, V, M)
    mu = torch.rand(E, A, device=dev) * 2 - 1
    noise = OUNoise(E, A, device=dev, seed=3) if noisy else None
    rb = SarlReplayBuffer(4 * E, tn + 5, A, V, device=dev)
    launch = env.bind_sarl_rollout(mu, noise=noise, replay=rb)
    launch()
    return launch, N.last_kernel()


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sarl_rollout needs a HIP device: a timing taken elsewhere says nothing")
    results = []
    for E, V, M in SIZES:
        A, tn = 2 * V + M, M // V
        row = dict(E=E, V=V, M=M, steps_per_form=args.rounds * args.steps, warmup=args.warmup)
        for noisy in (True, False):
            staged = staged_step(E, V, M, noisy)
            fused, kernel = fused_step(E, V, M, noisy)
            for fn in (staged, fused):
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            us = {"staged": [], "one_launch": []}
            for _ in range(args.rounds):                       # interleaved: what drifts, drifts for both
                us["staged"].append(timed(staged, args.steps))
                us["one_launch"].append(timed(fused, args.steps))
            tag = "" if noisy else "_no_noise"
            for k, v in us.items():
                row["%s_us%s" % (k, tag)] = round(sorted(v)[len(v) // 2], 2)
                row["%s_us%s_rounds" % (k, tag)] = [round(t, 2) for t in v]
            row["kernel"] = kernel
            del staged, fused
            torch.cuda.empty_cache()
        step_bytes = 8 * V * M + 12 * M + 12 * A + 4 * V * (tn + 5) + 48 * V + 4
        ring_bytes = 8 * V * (tn + 5) + 4 * A + 5
        row["bytes_per_env_step"] = step_bytes + ring_bytes
        row["bytes_per_env_step_ring_part"] = ring_bytes
        row["one_launch_GBps"] = round(E * (step_bytes + ring_bytes) / row["one_launch_us"] / 1e3, 1)
        row["hbm_peak_fraction"] = round(E * (step_bytes + ring_bytes) / (row["one_launch_us"] * 1e-6) / HBM_PEAK, 3)
        row["speedup"] = round(row["staged_us"] / row["one_launch_us"], 2)
        row["speedup_no_noise"] = round(row["staged_us_no_noise"] / row["one_launch_us_no_noise"], 2)
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/time_sarl_rollout.py", device=torch.cuda.get_device_name(0), sizes=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
