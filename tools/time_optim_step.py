#!/usr/bin/env python3
"""Times `BatchedAdam.step` (csrc/k_adam.hip: two launches for any number of networks) against the reference's statements
with library kernels, at the learners' sizes -> profiles/optim_step.json.

Per network the reference runs `clip_grad_norm_(net.parameters(), 1.0)`, `optimizer.step()` and the blend loop
`target.copy_(tau * online + (1 - tau) * target)` per tensor (global_sac_critic.py:364-370 and :394-400,
sac_agent.py:296-312, global_sac_critic.py:246-249; the SARL learner steps without a clip, its critic with
`weight_decay=0.01`).  Forms, raced in alternating rounds on equal inputs (own copies of the parameters each):

    device          BatchedAdam.step(targets, tau)                                    2 launches (1 without a clip)
    torch_default   the statements above with torch.optim.Adam as constructed by default (foreach on a GPU)
    torch_fused     the same with torch.optim.Adam(fused=True)

Per call two times are taken separately: `event` -- device-timeline microseconds between two events around `steps` calls
(what the stream is busy or waiting for the host), and `host` -- wall-clock microseconds the Python thread spends issuing
the call (read before any synchronisation).  At 264 tensors the pointer check of `step()` is host work: `host` shows
whether it stays below the library path's.  Medians over `rounds` alternating rounds, every round listed, the ratio's
spread = [min, max] of the per-round ratios.  One JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedAdam  # noqa: E402

DEV = "cuda:0"
TAU = 0.005


def critic_shapes(inp, f1=1024, f2=512, f3=256):             # networks.py:7-49
    return [(f1, inp), (f1,), (f2, f1), (f2,), (f3, f2), (f3,), (1, f3), (1,)]


def policy_shapes(V, obs=5, f1=512, f2=256):                  # one agent's policy: two Linear + LayerNorm, mu | log_std | intent heads
    return [(f1, obs), (f1,), (f1,), (f1,), (f2, f1), (f2,), (f2,), (f2,), (V + 4, f2), (V + 4,)]


def sarl_actor_shapes(inp=80, act=56, f=(1024, 512, 256)):    # ddpg_torch.py: three Linear + LayerNorm, mu
    out, last = [], inp
    for w in f:
        out += [(w, last), (w,), (w,), (w,)]
        last = w
    return out + [(act, last), (act,)]


def sarl_critic_shapes(inp=80, act=56, f=(1024, 512, 256)):
    out, last = [], inp
    for w in f:
        out += [(w, last), (w,), (w,), (w,)]
        last = w
    return out + [(f[2], act), (f[2],), (1, f[2]), (1,)]


def sizes():
    yield "global_twin_critics_40_80", [critic_shapes(120)] * 2, dict(lr=3e-4, max_norm=1.0), True
    yield "global_twin_critics_20_24", [critic_shapes(44)] * 2, dict(lr=3e-4, max_norm=1.0), True
    yield "local_critics_V4", [critic_shapes(5 + 6)] * 8, dict(lr=3e-4, max_norm=1.0), True
    yield "local_critics_V8", [critic_shapes(5 + 10)] * 16, dict(lr=3e-4, max_norm=1.0), True
    yield "policies_V8", [policy_shapes(8)] * 8, dict(lr=1e-4, max_norm=1.0), False
    yield ("sarl_actor_and_critic", [sarl_actor_shapes(), sarl_critic_shapes()],
           dict(lr=[1e-4, 1e-3], weight_decay=[0.0, 0.01], max_norm=None), True)


def make(shapes, seed, targets):
    g = torch.Generator().manual_seed(seed)
    P = [[(torch.randn(*s, generator=g) * 0.05).to(DEV).requires_grad_() for s in grp] for grp in shapes]
    for grp in P:
        for p in grp:
            p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(DEV)
    T = [[p.detach().clone() for p in grp] for grp in P] if targets else None
    return P, T


def per_group(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def torch_form(P, T, hyper, fused):
    n = len(P)
    lr, wd, mn = per_group(hyper["lr"], n), per_group(hyper.get("weight_decay", 0.0), n), per_group(hyper["max_norm"], n)
    opts = [torch.optim.Adam(grp, lr=lr[i], weight_decay=wd[i], **({"fused": True} if fused else {})) for i, grp in enumerate(P)]

    def run():
        for i, (grp, opt) in enumerate(zip(P, opts)):
            if mn[i] is not None:
                torch.nn.utils.clip_grad_norm_(grp, mn[i])
            opt.step()
            if T is not None:
                for t, p in zip(T[i], grp):                   # update_network_parameters' loop
                    t.data.copy_(TAU * p.data + (1 - TAU) * t.data)
    return run


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    host = (time.perf_counter() - t0) * 1e6 / steps
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps, host


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_optim_step needs a HIP device: a timing taken elsewhere says nothing")
    rows = []
    for name, shapes, hyper, targets in sizes():
        forms, keep = {}, []
        P, T = make(shapes, 1, targets)
        opt = BatchedAdam(P, **hyper)
        forms["device"] = (lambda opt=opt, T=T: opt.step(targets=T, tau=TAU)) if targets else (lambda opt=opt: opt.step())
        for key, fused in (("torch_default", False), ("torch_fused", True)):
            P2, T2 = make(shapes, 1, targets)
            keep.append((P2, T2))
            forms[key] = torch_form(P2, T2, hyper, fused)
        for fn in forms.values():
            for _ in range(args.warmup):
                fn()
        ev, host = {k: [] for k in forms}, {k: [] for k in forms}
        for _ in range(args.rounds):                          # alternating: what drifts, drifts for all
            for k, fn in forms.items():
                e, h = timed(fn, args.steps)
                ev[k].append(e)
                host[k].append(h)
        numel = sum(p.numel() for grp in P for p in grp)
        clip = opt._clip
        bytes_per = 4 * (2 + (2 if clip else 1) + 2 + 2 + (2 if targets else 0))    # param, grad, m, v, target: read + written
        row = dict(size=name, n_groups=len(P), n_tensors=sum(len(g) for g in P), numel=numel, workgroups=opt.n_blocks,
                   kernel="k_adam_sqsum + k_adam_step" if clip else "k_adam_step",
                   clip=clip, blend=bool(targets), table_uploads=opt.table_uploads, bytes_per_element=bytes_per,
                   iterations_per_form=args.rounds * args.steps, warmup=args.warmup)
        for k in forms:
            row["%s_event_us" % k] = round(median(ev[k]), 2)
            row["%s_event_us_rounds" % k] = [round(x, 2) for x in ev[k]]
            row["%s_host_us" % k] = round(median(host[k]), 2)
            row["%s_host_us_rounds" % k] = [round(x, 2) for x in host[k]]
        row["device_GBps"] = round(numel * bytes_per / row["device_event_us"] * 1e-3, 1)
        for k in ("torch_default", "torch_fused"):
            r = [o / d for o, d in zip(ev[k], ev["device"])]
            row["%s_over_device_event" % k] = round(median(r), 2)
            row["%s_over_device_event_spread" % k] = [round(min(r), 2), round(max(r), 2)]
            rh = [o / d for o, d in zip(host[k], host["device"])]
            row["%s_over_device_host" % k] = round(median(rh), 2)
            row["%s_over_device_host_spread" % k] = [round(min(rh), 2), round(max(rh), 2)]
            row["device_host_below_%s_in_every_round" % k] = bool(all(d < o for d, o in zip(host["device"], host[k])))
        rows.append(row)
        del forms, keep, opt, P, T
        torch.cuda.empty_cache()
    result = dict(tool="tools/time_optim_step.py", device=torch.cuda.get_device_name(0), torch=torch.__version__, tau=TAU, sizes=rows)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
