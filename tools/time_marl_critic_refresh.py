#!/usr/bin/env python3
"""Time the target-network update of the SAC learner, from "the optimiser stepped" to "the next TD target is ready": the
Polyak blend of both target critics, the rebuild of both weight streams and `BatchedTwinCritic.td_target`, with
`pack="device"` against `pack="host"` (the path as it ran before the device pack existed) on the same tensors,
interleaved in one process, HIP events, median of rounds.

    python tools/time_marl_critic_refresh.py [--out FILE.json] [--rounds 7] [--steps 50] [--warmup 20] [--lib-one LIB.so]

refresh     the pack of both nets alone on the same weight tensors: `pack_marl_critic_weights(...)` once per net as
            `pack="host"` calls it (new tensors every call) against `pack_marl_critic_weights_device(..., out=,
            workspace=)` as `pack="device"` calls it (two launches for both nets); with the bytes it reads and writes, so
            the rate can be set against a memory bandwidth
loop step   `soft_update_from` (one launch) -> `td_target` on a batch of 64, 4 096 and 32 768 rows: "host" rebuilds the
            streams with library kernels, "device" with the two launches -- four launches in all
frozen      `td_target` alone, nothing updated: the one-launch floor
pack call   the bare `risvec_marl_critic_pack` call on prepared arguments, without the Python checks around it, with the
            bytes the two launches read and write
max blocks  with --lib-one, a second build of the library whose statistics launch uses ONE workgroup per net (`make -C
            ris_vec_marl_amd/csrc mb1`, -DRISVEC_MARL_CRITIC_PACK_MAX_BLOCKS=1) is loaded beside the package's own and the
            same bare call is raced between the two; the counts are read back from the workspace sizes
Medians are over `rounds` windows of `steps` iterations each after `warmup` iterations of every form.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedTwinCritic  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402
from ris_vec_marl_amd.marl_critic import marl_critic_geom, pack_marl_critic_weights, pack_marl_critic_weights_device  # noqa: E402

DIMS = [(40, 80), (20, 24)]                     # (state_dims, action_dims): the driver at 8 and at 4 vehicles
ROWS = [64, 4096, 32768]
F1, F2, F3 = 1024, 512, 256
TAU, GAMMA = 0.005, 0.99
DEV = "cuda:0"


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


def raw_pack(lib, dims, weights, out, work):
    """The bare `risvec_marl_critic_pack` call of `lib` on prepared arguments (no Python checks in the timed part)."""
    nets = (N.RisVecMarlCriticPackNet * len(weights))()
    for c, (ws, (stream, scales)) in enumerate(zip(weights, out)):
        nets[c] = N.RisVecMarlCriticPackNet(ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(), stream.data_ptr(),
                                            stream.numel() * 2, scales.data_ptr())
    args = tuple(dims) + (len(weights), C.cast(nets, C.c_void_p), work.data_ptr(), work.numel(), N.stream(torch.device(DEV)))

    def run():
        if lib.risvec_marl_critic_pack(*args) != N.OK:
            raise SystemExit("risvec_marl_critic_pack: %s" % lib.risvec_last_error().decode())
    run.keep = nets
    return run


def load_other(path):
    lib = C.CDLL(path)
    for name in ("risvec_marl_critic_pack_workspace", "risvec_marl_critic_pack", "risvec_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = N._PROTOS[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lib-one", default=None, help="a build of librisvec.so with -DRISVEC_MARL_CRITIC_PACK_MAX_BLOCKS=1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_marl_critic_refresh needs a HIP device: a timing taken elsewhere says nothing")
    lib = N.load()
    one = load_other(args.lib_one) if args.lib_one else None
    sizes = []
    for S, A in DIMS:
        dims = (S, A, F1, F2, F3)
        g = marl_critic_geom(*dims)
        critic = BatchedTwinCritic(*dims, device=DEV, seed=5)              # the online critics: the learner's tensors
        t_host = BatchedTwinCritic(*dims, device=DEV, seed=6)              # the parent commit's targets
        t_dev = BatchedTwinCritic(*dims, device=DEV, seed=6)
        t_dev.pack = "device"
        assert t_host.pack == "host" and t_dev.pack == "device" and t_host.gemm == t_dev.gemm == "fused"
        weights = [tuple(getattr(net, k) for k in net._PACKED) for net in critic.nets]
        read_bytes = sum(t.numel() * 4 for ws in weights for t in ws)
        out = [(torch.zeros(g.rows, 64, 8, dtype=torch.float16, device=DEV), torch.zeros(3, device=DEV)) for _ in weights]
        need = int(lib.risvec_marl_critic_pack_workspace(*dims, 2))
        work = torch.zeros(need, dtype=torch.uint8, device=DEV)
        row = dict(state_dims=S, action_dims=A, dims=list(dims), n_nets=2, weight_stream_bytes_per_net=g.rows * 1024,
                   packed_weight_bytes=read_bytes, iterations_per_form=args.rounds * args.steps, warmup=args.warmup, tau=TAU,
                   max_blocks=int(lib.risvec_marl_critic_pack_workspace(*dims, 1)) // 12)

        def host_refresh():
            for ws in weights:
                pack_marl_critic_weights(*ws)
        us = race({"refresh_host": host_refresh,
                   "refresh_device": lambda: pack_marl_critic_weights_device(weights, out=out, workspace=work)},
                  args.rounds, args.steps, args.warmup)
        row["kernel"] = N.last_kernel()
        differing = 0
        for ws, (ds, dc) in zip(weights, out):
            hs, hc = pack_marl_critic_weights(*ws)
            differing += int((hs.view(torch.int16) != ds.view(torch.int16)).sum()) + int((hc.view(torch.int32) != dc.view(torch.int32)).sum())
        row["halfs_and_scales_differing_from_host"] = differing
        # the bare C call on prepared arguments: what the two launches take without the Python checks around them
        forms = {"pack_call_max_blocks_%d" % row["max_blocks"]: raw_pack(lib, dims, weights, out, work)}
        if one is not None:
            need1 = int(one.risvec_marl_critic_pack_workspace(*dims, 2))
            work1 = torch.zeros(max(need1, 16), dtype=torch.uint8, device=DEV)
            out1 = [(torch.zeros_like(s), torch.zeros_like(c)) for s, c in out]
            row["max_blocks_other"] = int(one.risvec_marl_critic_pack_workspace(*dims, 1)) // 12
            forms["pack_call_max_blocks_%d" % row["max_blocks_other"]] = raw_pack(one, dims, weights, out1, work1)
        us.update(race(forms, args.rounds, args.steps, args.warmup))
        if one is not None:
            torch.cuda.synchronize()
            row["max_blocks_builds_agree"] = bool(all(torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(c, d)
                                                      for (a, c), (b, d) in zip(out, out1)))
        for n in ROWS:
            gen = torch.Generator(device="cpu").manual_seed(n)
            states_ = torch.rand(n, S, generator=gen).to(DEV)
            actions_ = torch.rand(n, A, generator=gen).to(DEV)
            rewards, dones = -torch.rand(n, generator=gen).to(DEV), (torch.rand(n, generator=gen) < 0.1).to(DEV)
            lp, li = -torch.rand(n, generator=gen).to(DEV), -torch.rand(n, generator=gen).to(DEV)
            coef = torch.tensor([0.2, 0.2], device=DEV)
            y = torch.empty(n, device=DEV)

            def host():
                t_host.soft_update_from(critic, tau=TAU)
                t_host.td_target(rewards, states_, actions_, dones, GAMMA, lp, li, coef, out=y)

            def device():
                t_dev.soft_update_from(critic, tau=TAU)
                t_dev.td_target(rewards, states_, actions_, dones, GAMMA, lp, li, coef, out=y)

            def frozen():
                t_dev.td_target(rewards, states_, actions_, dones, GAMMA, lp, li, coef, out=y)
            packs = (t_host.packs, t_dev.packs)
            us.update(race({"loop_host_%d" % n: host, "loop_device_%d" % n: device, "frozen_%d" % n: frozen},
                           args.rounds, args.steps, args.warmup))
            calls = args.warmup + args.rounds * args.steps
            row["net_rebuilds_per_blend_%d" % n] = [(t_host.packs - packs[0]) / calls, (t_dev.packs - packs[1]) / calls]
            torch.cuda.empty_cache()
        for k, v in us.items():
            row["%s_us" % k] = round(median(v), 2)
            row["%s_us_rounds" % k] = [round(t, 2) for t in v]
        row["refresh_speedup"] = round(row["refresh_host_us"] / row["refresh_device_us"], 2)
        row["refresh_device_beats_host"] = beats(us["refresh_device"], us["refresh_host"])
        row["refresh_device_faster_in_every_round"] = bool(all(d < h for d, h in zip(us["refresh_device"], us["refresh_host"])))
        # both launches read the weights (the second mostly from cache), the second writes the streams
        row["pack_call_GBps_read_twice_plus_written"] = round((2 * read_bytes + 2 * g.rows * 1024)
                                                              / row["pack_call_max_blocks_%d_us" % row["max_blocks"]] * 1e-3, 1)
        if one is not None:
            a, b = us["pack_call_max_blocks_%d" % row["max_blocks"]], us["pack_call_max_blocks_%d" % row["max_blocks_other"]]
            row["max_blocks_%d_beats_%d" % (row["max_blocks"], row["max_blocks_other"])] = beats(a, b)
        for n in ROWS:
            row["loop_speedup_%d" % n] = round(row["loop_host_%d_us" % n] / row["loop_device_%d_us" % n], 2)
            row["loop_device_beats_host_%d" % n] = beats(us["loop_device_%d" % n], us["loop_host_%d" % n])
            row["loop_device_faster_in_every_round_%d" % n] = bool(all(d < h for d, h in zip(us["loop_device_%d" % n], us["loop_host_%d" % n])))
            row["loop_device_over_frozen_%d" % n] = round(row["loop_device_%d_us" % n] / row["frozen_%d_us" % n], 2)
        sizes.append(row)
    result = dict(tool="tools/time_marl_critic_refresh.py", device=torch.cuda.get_device_name(0), sizes=sizes)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
