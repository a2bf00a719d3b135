#!/usr/bin/env python3
"""Times `BatchedTwinCritic.action_grad` (csrc/k_marl_critic_action_grad.hip: two launches) against the statements it replaces,
with library kernels and autograd, in the same process -> profiles/marl_action_grad.json.

The reference runs, per learner step (global_sac_critic.py:174-176 and the backward() at :246), both online critics on (states,
actions_pi), `torch.min`, and a backward that walks both critics to reach actions_pi -- and, because the critics' parameters
require grad, forms their 16 weight gradients on the way.  Forms, raced in alternating rounds on equal inputs and weights:

    device          action_grad with current weight streams                           2 launches
    device_packed   the same after a weight update: both streams rebuilt first        2 + 2 launches (pack="device")
    library         (a) `action_grad_torch`: the gradient with respect to the action only, weights detached
    reference       (b) the reference's own form on torch.nn modules whose parameters require grad: q_min.sum().backward()
                    after zero_grad(set_to_none=True) on the modules and a fresh actions_pi leaf

Rows 64 / 256 / 4096 at the shapes of 8 and 4 vehicles.  Per form `event` is device-timeline microseconds between two events
around `steps` calls, `host` the wall-clock microseconds the Python thread spends issuing a call.  Medians over `rounds`
alternating rounds, every round listed; a ratio's spread = [min, max] of the per-round ratios.
`device_beats_library_beyond_the_spread` -- the device form faster than (a) in EVERY round by more than the spread between
rounds (the larger of the two forms' max - min) -- at both shapes is what `BatchedTwinCritic.ACTION_GRAD_AUTO_ROWS` follows.
One JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedTwinCritic  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = ((40, 80), (20, 24))
ROWS = (64, 256, 4096)


class CriticNetwork(torch.nn.Module):
    """networks.py:7-49: a ReLU MLP on cat([state, action])."""

    def __init__(self, in_dims, fc1=1024, fc2=512, fc3=256):
        super().__init__()
        self.fc1, self.fc2 = torch.nn.Linear(in_dims, fc1), torch.nn.Linear(fc1, fc2)
        self.fc3, self.q = torch.nn.Linear(fc2, fc3), torch.nn.Linear(fc3, 1)

    def forward(self, state, action):
        x = torch.relu(self.fc1(torch.cat([state, action], dim=1)))
        return self.q(torch.relu(self.fc3(torch.relu(self.fc2(x)))))


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


def forms_of(S, A, n):
    torch.manual_seed(1)
    online = [CriticNetwork(S + A).to(DEV) for _ in range(2)]
    critic = BatchedTwinCritic(S, A, device=DEV, gemm="fused")
    critic.pack = "device"
    critic.share_state_dict(*(m.state_dict() for m in online))
    lib = BatchedTwinCritic(S, A, device=DEV, gemm="library")
    lib.share_state_dict(*(m.state_dict() for m in online))
    g = torch.Generator().manual_seed(3)
    s, a = torch.rand(n, S, generator=g).to(DEV), torch.rand(n, A, generator=g).to(DEV)
    scale = -1.0 / n
    new = lambda: (torch.empty(n, A, device=DEV), torch.empty(n, device=DEV),      # noqa: E731
                   (torch.empty(n, 1, device=DEV), torch.empty(n, 1, device=DEV)))
    od, md, qd = new()
    ol, ml, ql = new()
    out = {"device": lambda: critic.action_grad(s, a, out=od, q_min=md, q=qd, scale=scale)}

    def packed():
        critic.mark_stale()
        critic.action_grad(s, a, out=od, q_min=md, q=qd, scale=scale)
    out["device_packed"] = packed
    out["library"] = lambda: lib.action_grad(s, a, out=ol, q_min=ml, q=ql, scale=scale)

    def reference():
        for m in online:
            m.zero_grad(set_to_none=True)
        pi = a.detach().requires_grad_(True)
        q_min = torch.min(online[0](s, pi), online[1](s, pi))
        (q_min.sum() * scale).backward()
        return pi.grad
    out["reference"] = reference
    return out, (online, critic, lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", type=int, default=0, metavar="ROWS",
                    help="run each form a few times at (40, 80) x ROWS and exit: the run a kernel trace is taken of")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_marl_action_grad needs a HIP device: a timing taken elsewhere says nothing")
    if args.once:
        forms, keep = forms_of(40, 80, args.once)
        for fn in forms.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        return
    rows = []
    for (S, A) in SHAPES:
        for n in ROWS:
            forms, keep = forms_of(S, A, n)
            for fn in forms.values():
                for _ in range(args.warmup):
                    fn()
            ev, host = {k: [] for k in forms}, {k: [] for k in forms}
            for _ in range(args.rounds):                      # alternating: what drifts, drifts for all
                for k, fn in forms.items():
                    e, h = timed(fn, args.steps)
                    ev[k].append(e)
                    host[k].append(h)
            row = dict(state_dims=S, action_dims=A, fc=[1024, 512, 256], rows=n, iterations_per_form=args.rounds * args.steps,
                       warmup=args.warmup)
            for k in forms:
                row["%s_event_us" % k] = round(median(ev[k]), 1)
                row["%s_event_us_rounds" % k] = [round(x, 1) for x in ev[k]]
                row["%s_host_us" % k] = round(median(host[k]), 1)
            for num, den in (("library", "device"), ("library", "device_packed"), ("reference", "device"), ("reference", "device_packed")):
                r = [o / d for o, d in zip(ev[num], ev[den])]
                row["%s_over_%s" % (num, den)] = round(median(r), 2)
                row["%s_over_%s_spread" % (num, den)] = [round(min(r), 2), round(max(r), 2)]
            for den in ("device", "device_packed"):
                spread = max(max(ev[k]) - min(ev[k]) for k in ("library", den))
                row["%s_beats_library_beyond_the_spread" % den] = bool(min(o - d for o, d in zip(ev["library"], ev[den])) > spread)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del forms, keep
            torch.cuda.empty_cache()
    result = dict(tool="tools/time_marl_action_grad.py", device=torch.cuda.get_device_name(0), torch=torch.__version__, sizes=rows)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
