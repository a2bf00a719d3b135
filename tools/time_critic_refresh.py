#!/usr/bin/env python3
"""Time the target-network update of the DDPG learner, from "the optimiser stepped" to "the next TD target is ready":
the Polyak blend of both target networks, the rebuild of both weight streams and `ddpg_td_target`, interleaved in one
process, HIP events, median of rounds.

    python tools/time_critic_refresh.py [--out FILE.json] [--rounds 7] [--steps 50] [--warmup 20]

refresh     the critic's pack alone on the same weight tensors: `pack_critic_weights(...)` as `pack="host"` calls it (new
            tensors every call) against `pack_critic_weights_device(..., out=, workspace=)` as `pack="device"` calls it;
            with the bytes it reads and writes, so the rate can be set against a memory bandwidth
soft update the blend alone, all 26 tensors of both networks: the reference's statements with library kernels (per tensor
            `tau * online.clone() + (1 - tau) * target.clone()`, then the copy into the target that `load_state_dict`
            makes) against the one launch of `ddpg_soft_update`
loop step   blend both target networks -> `ddpg_td_target` on a batch of 64, 4 096 and 32 768 rows.  "parent": library
            blend, critic pack="host", actor pack="device" -- the step as it ran before the device pack of the critic and
            the one-launch blend existed.  "device": `ddpg_soft_update`, both packs on the device: seven launches.
frozen      `ddpg_td_target` alone, nothing updated: the two-launch floor
Medians are over `rounds` windows of `steps` iterations each after `warmup` iterations of every form.  One JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedActor, BatchedCritic, ddpg_soft_update, ddpg_td_target  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402
from ris_vec_marl_amd.critic import critic_geom, pack_critic_weights, pack_critic_weights_device  # noqa: E402

DIMS = [(8, 40), (8, 64)]                       # (V, M): critic 80-1024-512-256/56 and 104-1024-512-256/80
ROWS = [64, 4096, 32768]
F1, F2, F3, AF1, AF2 = 1024, 512, 256, 512, 256
TAU, GAMMA = 0.005, 0.99
DEV = "cuda:0"


def pair(IN, A, seed, critic_pack):
    """(actor, critic) at the driver's sizes; the actor always packs on the device (it did before this tool existed)"""
    actor = BatchedActor(IN, A, AF1, AF2, device=DEV, seed=seed, pack="device")
    actor.Wmu.mul_(60.0)
    return actor, BatchedCritic(IN, A, F1, F2, F3, device=DEV, seed=seed, pack=critic_pack)


def tensors(net):
    return [getattr(net, a) for a in net._WEIGHTS]


def library_blend(online, target):
    """update_network_parameters with library kernels: the blend into new tensors, then the copy into the target (which
    advances its version counters, so the next call repacks)."""
    def run():
        for on, tg in zip(online, target):
            tg.copy_(TAU * on.clone() + (1 - TAU) * tg.clone())
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


def beats(new, old):
    """The criterion of DESIGN.md 3.6: faster in every round, by more than either side's spread between rounds."""
    return bool(all(n < o for n, o in zip(new, old))
                and min(old) - max(new) > max(max(new) - min(new), max(old) - min(old)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_critic_refresh needs a HIP device: a timing taken elsewhere says nothing")
    lib = N.load()
    sizes = []
    for V, M in DIMS:
        IN, A = V * (M // V + 5), 2 * V + M
        dims = (IN, F1, F2, F3, A)
        g = critic_geom(*dims)
        actor, critic = pair(IN, A, 5, "device")               # the online networks: the learner's tensors
        t_actor_p, t_critic_p = pair(IN, A, 6, "host")         # the parent commit's targets
        t_actor_d, t_critic_d = pair(IN, A, 6, "device")
        ws = [getattr(critic, k) for k in BatchedCritic._PACKED]
        read_bytes = sum(t.numel() * 4 for t in ws)
        out = (torch.zeros(g.rows, 64, 8, dtype=torch.float16, device=DEV), torch.zeros(4, device=DEV))
        work = torch.zeros(int(lib.risvec_sarl_critic_pack_workspace(*dims)), dtype=torch.uint8, device=DEV)
        row = dict(V=V, M=M, dims=list(dims), actor_dims=[IN, AF1, AF2, A], weight_stream_bytes=g.rows * 1024,
                   packed_weight_bytes=read_bytes, iterations_per_form=args.rounds * args.steps, warmup=args.warmup, tau=TAU)
        us = race({"refresh_host": lambda: pack_critic_weights(*ws),
                   "refresh_device": lambda: pack_critic_weights_device(*ws, out=out, workspace=work)},
                  args.rounds, args.steps, args.warmup)
        row["kernel"] = N.last_kernel()
        hs, hc = pack_critic_weights(*ws)
        row["scales_equal"] = bool(torch.equal(hc, out[1]))
        row["halfs_differing"] = int((hs.view(torch.int16) != out[0].view(torch.int16)).sum())
        blended = sum(t.numel() for t in tensors(actor) + tensors(critic))
        row["blended_tensors"], row["blended_elements"] = len(tensors(actor) + tensors(critic)), blended
        lib_blend_p = library_blend(tensors(actor) + tensors(critic), tensors(t_actor_p) + tensors(t_critic_p))
        us.update(race({"soft_library": lib_blend_p,
                        "soft_device": lambda: ddpg_soft_update(actor, t_actor_d, critic, t_critic_d, TAU)},
                       args.rounds, args.steps, args.warmup))
        row["soft_kernel"] = N.last_kernel()
        for n in ROWS:
            gen = torch.Generator(device="cpu").manual_seed(n)
            states_ = torch.rand(n, IN, generator=gen).to(DEV)
            rewards, dones = -torch.rand(n, generator=gen).to(DEV), (torch.rand(n, generator=gen) < 0.1).to(DEV)
            y, act = torch.empty(n, device=DEV), torch.empty(n, A, device=DEV)

            def parent():
                lib_blend_p()
                ddpg_td_target(t_actor_p, t_critic_p, states_, rewards, dones, GAMMA, out=y, actions_=act)

            def device():
                ddpg_soft_update(actor, t_actor_d, critic, t_critic_d, TAU)
                ddpg_td_target(t_actor_d, t_critic_d, states_, rewards, dones, GAMMA, out=y, actions_=act)

            def frozen():
                ddpg_td_target(t_actor_d, t_critic_d, states_, rewards, dones, GAMMA, out=y, actions_=act)
            packs = (t_critic_p.packs, t_critic_d.packs)
            us.update(race({"loop_parent_%d" % n: parent, "loop_device_%d" % n: device, "frozen_%d" % n: frozen},
                           args.rounds, args.steps, args.warmup))
            calls = args.warmup + args.rounds * args.steps
            row["critic_rebuilds_per_blend_%d" % n] = [(t_critic_p.packs - packs[0]) / calls, (t_critic_d.packs - packs[1]) / calls]
            torch.cuda.empty_cache()
        for k, v in us.items():
            row["%s_us" % k] = round(median(v), 2)
            row["%s_us_rounds" % k] = [round(t, 2) for t in v]
        row["refresh_speedup"] = round(row["refresh_host_us"] / row["refresh_device_us"], 2)
        row["refresh_device_beats_host"] = beats(us["refresh_device"], us["refresh_host"])
        row["refresh_device_GBps_read_plus_written"] = round((read_bytes + g.rows * 1024) / row["refresh_device_us"] * 1e-3, 1)
        row["soft_speedup"] = round(row["soft_library_us"] / row["soft_device_us"], 2)
        row["soft_device_beats_library"] = beats(us["soft_device"], us["soft_library"])
        row["soft_device_GBps_read_plus_written"] = round(12 * blended / row["soft_device_us"] * 1e-3, 1)
        for n in ROWS:
            row["loop_speedup_%d" % n] = round(row["loop_parent_%d_us" % n] / row["loop_device_%d_us" % n], 2)
            row["loop_device_beats_parent_%d" % n] = beats(us["loop_device_%d" % n], us["loop_parent_%d" % n])
            row["loop_device_over_frozen_%d" % n] = round(row["loop_device_%d_us" % n] / row["frozen_%d_us" % n], 2)
        sizes.append(row)
    result = dict(tool="tools/time_critic_refresh.py", device=torch.cuda.get_device_name(0), sizes=sizes)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
