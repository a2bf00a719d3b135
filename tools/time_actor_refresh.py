#!/usr/bin/env python3
"""Time what a weight update costs the DDPG actor (`BatchedActor`): rebuilding the fused kernel's weight stream with
library kernels (`pack="host"`, `pack_actor_weights`) against the two-launch device pack (`pack="device"`,
`risvec_sarl_actor_pack`), interleaved in one process, HIP events, median of rounds.

    python tools/time_actor_refresh.py [--out FILE.json] [--rounds 7] [--steps 50] [--warmup 20]

refresh     the pack alone on the same weight tensors: `pack_actor_weights(...)` as `pack="host"` calls it (new tensors
            every call) against `pack_actor_weights_device(..., out=, workspace=)` as `pack="device"` calls it
loop step   update every weight tensor in place (one multi-tensor launch standing in for the optimiser step; the same on
            both sides) -> `actor.forward(launch.obs, out=mu)` -> the one-launch rollout step, at 4 096 and 32 768
            envs, both ways, the actors sharing the learner's tensors through `share_state_dict`
frozen      the same step without the update: the two-launch floor
The comparator is always `pack="host"`, the only path before the device pack existed.  Medians are over `rounds` windows
of `steps` iterations each after `warmup` iterations of every form.  One JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedActor, OUNoise, SarlReplayBuffer, VecEnviron, reference_lanes  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402
from ris_vec_marl_amd.actor import actor_geom, pack_actor_weights, pack_actor_weights_device  # noqa: E402

DIMS = [(8, 40), (8, 64)]                       # (V, M): 80/512/256/56 and 104/512/256/80
ENVS = [4096, 32768]
PACKED = ("W1", "b1", "ln1_w", "ln1_b", "W2", "Wmu")
DEV = "cuda:0"


def learner(V, M):
    """The learner's actor tensors under the reference's key names, on the device."""
    a = BatchedActor(V * (M // V + 5), 2 * V + M, 512, 256, device=DEV, seed=5)
    a.Wmu.mul_(60.0)
    return {k: getattr(a, v).clone() for k, v in BatchedActor._SD.items()}


def make_actor(V, M, sd, pack):
    a = BatchedActor(V * (M // V + 5), 2 * V + M, 512, 256, device=DEV, pack=pack)
    a.share_state_dict(sd)
    return a


def loop_step(E, V, M, actor, params):
    """The driver's rollout step around `actor`; params: the tensors updated in place first (None: frozen weights)."""
    L = reference_lanes()
    env = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3,
                     n_envs=E, device=DEV, seed=3)
    env.make_new_game()
    env.compute_parms()
    A, tn = 2 * V + M, M // V
    mu = torch.zeros(E, A, device=DEV)
    launch = env.bind_sarl_rollout(mu, noise=OUNoise(E, A, device=DEV, seed=3),
                                   replay=SarlReplayBuffer(4 * E, tn + 5, A, V, device=DEV))

    def run():
        if params is not None:
            torch._foreach_mul_(params, 1.0)                   # in place: every version counter moves, no value does
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


def race(forms, rounds, steps, warmup):
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(rounds):                                    # interleaved: what drifts, drifts for all
        for k, fn in forms.items():
            us[k].append(timed(fn, steps))
    return us


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_actor_refresh needs a HIP device: a timing taken elsewhere says nothing")
    sizes = []
    for V, M in DIMS:
        IN, A = V * (M // V + 5), 2 * V + M
        g = actor_geom(IN, 512, 256, A)
        sd = learner(V, M)
        host, device = make_actor(V, M, sd, "host"), make_actor(V, M, sd, "device")
        ws = [getattr(device, k) for k in PACKED]
        params = list(sd.values())
        out = (torch.zeros(g.items, g.rows, 64, 8, dtype=torch.float16, device=DEV), torch.zeros(3, device=DEV))
        work = torch.zeros(int(N.load().risvec_sarl_actor_pack_workspace(IN, 512, 256, A)), dtype=torch.uint8, device=DEV)
        row = dict(V=V, M=M, dims=[IN, 512, 256, A], weight_stream_bytes=g.items * g.rows * 1024,
                   iterations_per_form=args.rounds * args.steps, warmup=args.warmup)
        us = race({"refresh_host": lambda: pack_actor_weights(*ws),
                   "refresh_device": lambda: pack_actor_weights_device(*ws, out=out, workspace=work)},
                  args.rounds, args.steps, args.warmup)
        row["kernel"] = N.last_kernel()
        hs, hc = pack_actor_weights(*ws)
        row["scales_equal"] = bool(torch.equal(hc, out[1]))
        row["halfs_differing"] = int((hs.view(torch.int16) != out[0].view(torch.int16)).sum())
        for E in ENVS:
            forms = race({"loop_host_%d" % E: loop_step(E, V, M, host, params),
                          "loop_device_%d" % E: loop_step(E, V, M, device, params),
                          "frozen_%d" % E: loop_step(E, V, M, device, None)}, args.rounds, args.steps, args.warmup)
            us.update(forms)
            torch.cuda.empty_cache()
        for k, v in us.items():
            row["%s_us" % k] = round(median(v), 2)
            row["%s_us_rounds" % k] = [round(t, 2) for t in v]
        row["refresh_speedup"] = round(row["refresh_host_us"] / row["refresh_device_us"], 2)
        row["refresh_device_faster_every_round"] = all(d < h for d, h in zip(us["refresh_device"], us["refresh_host"]))
        for E in ENVS:
            row["loop_speedup_%d" % E] = round(row["loop_host_%d_us" % E] / row["loop_device_%d_us" % E], 2)
            row["loop_device_over_frozen_%d" % E] = round(row["loop_device_%d_us" % E] / row["frozen_%d_us" % E], 2)
        sizes.append(row)
    result = dict(tool="tools/time_actor_refresh.py", device=torch.cuda.get_device_name(0), sizes=sizes)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
