#!/usr/bin/env python3
"""Times `BatchedTwinCritic.loss_backward` (csrc/k_marl_critic_grad.hip: two launches) against the statements it replaces,
with library kernels and autograd, in the same process -> profiles/marl_critic_grad.json.

The reference runs, per learner step (global_sac_critic.py:355-363), `zero_grad(set_to_none=True)` on both online critics,
two forwards, two `mse_loss` and one `backward()`.  Forms, raced in alternating rounds on equal inputs and equal weights:

    device          loss_backward with current weight streams                         2 launches
    device_packed   the same after a weight update: both streams rebuilt first        2 + 2 launches (pack="device")
    autograd        the reference's statements on torch.nn modules
    library         loss_backward of a gemm="library" critic on the same storage: the same statements through
                    `loss_backward_torch` (autograd.grad into caller-owned gradient tensors)

and the whole critic update between "the TD target is ready" and "the next TD target is ready":

    update_device   examples/marl_critic_grads.py: loss_backward, BatchedAdam.step(grads=, targets=, tau=), pack, td_target
    update_autograd examples/marl_critic_update.py: the autograd statements, BatchedAdam.step(targets=, tau=), pack, td_target

Rows 64 / 256 / 4096 at the shapes of 8 and 4 vehicles.  Per form `event` is device-timeline microseconds between two
events around `steps` calls, `host` the wall-clock microseconds the Python thread spends issuing a call.  Medians over
`rounds` alternating rounds, every round listed, the ratio's spread = [min, max] of the per-round ratios;
`device_packed_faster_than_*_in_every_round` is what `BatchedTwinCritic.GRAD_AUTO_ROWS` follows.  One JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import BatchedAdam, BatchedTwinCritic  # noqa: E402

DEV = torch.device("cuda:0")
TAU, GAMMA, LR = 0.005, 0.99, 3e-4
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


def side(S, A, n, seed):
    """One learner's critic side: modules, the critic object on their storage, target critics, optimiser, batch."""
    torch.manual_seed(seed)
    online = [CriticNetwork(S + A).to(DEV) for _ in range(2)]
    critic = BatchedTwinCritic(S, A, device=DEV, gemm="fused")
    critic.pack = "device"
    critic.share_state_dict(*(m.state_dict() for m in online))
    tgt = BatchedTwinCritic(S, A, device=DEV, seed=2)
    tgt.pack = "device"
    tgt.soft_update_from(critic, tau=1.0)
    opt = BatchedAdam([list(m.parameters()) for m in online], lr=LR, max_norm=1.0)
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.rand(*s, generator=g).to(DEV)        # noqa: E731
    batch = dict(s=r(n, S), a=r(n, A), s_=r(n, S), a_=r(n, A), rew=r(n) - 0.5, done=(r(n) < 0.05), y=r(n) * 2 - 1)
    return online, critic, tgt, opt, batch


def forms_of(S, A, n):
    out, keep = {}, []
    # -- the stage alone
    online, critic, tgt, opt, b = side(S, A, n, 1)
    grads, q, loss = critic.alloc_grads(), (torch.empty(n, 1, device=DEV), torch.empty(n, 1, device=DEV)), torch.empty(1, device=DEV)
    out["device"] = lambda: critic.loss_backward(b["s"], b["a"], b["y"], grads=grads, q=q, loss=loss)

    def packed():
        critic.mark_stale()
        critic.loss_backward(b["s"], b["a"], b["y"], grads=grads, q=q, loss=loss)
    out["device_packed"] = packed

    def autograd(online=online, b=b):
        for m in online:
            m.zero_grad(set_to_none=True)
        q1, q2 = (m(b["s"], b["a"]) for m in online)
        ls = torch.nn.functional.mse_loss(q1.view(-1), b["y"]) + torch.nn.functional.mse_loss(q2.view(-1), b["y"])
        ls.backward()
    out["autograd"] = autograd
    lib = BatchedTwinCritic(S, A, device=DEV, gemm="library")
    lib.share_state_dict(*(m.state_dict() for m in online))
    gl, ql, ll = lib.alloc_grads(), (torch.empty(n, 1, device=DEV), torch.empty(n, 1, device=DEV)), torch.empty(1, device=DEV)
    out["library"] = lambda: lib.loss_backward(b["s"], b["a"], b["y"], grads=gl, q=ql, loss=ll)
    keep.append((online, critic, lib, tgt, opt))
    # -- the whole update, each side on weights of its own (they move)
    on_d, cr_d, tg_d, op_d, bd = side(S, A, n, 1)
    gd, qd, ld, yd = cr_d.alloc_grads(), (torch.empty(n, 1, device=DEV), torch.empty(n, 1, device=DEV)), torch.empty(1, device=DEV), \
        torch.empty(n, device=DEV)

    def update_device():
        cr_d.loss_backward(bd["s"], bd["a"], bd["y"], grads=gd, q=qd, loss=ld)
        op_d.step(grads=gd, targets=tg_d, tau=TAU)
        tg_d.td_target(bd["rew"], bd["s_"], bd["a_"], bd["done"], GAMMA, out=yd)
    out["update_device"] = update_device
    on_a, cr_a, tg_a, op_a, ba = side(S, A, n, 1)
    ya = torch.empty(n, device=DEV)

    def update_autograd():
        autograd(on_a, ba)
        op_a.step(targets=tg_a, tau=TAU)
        tg_a.td_target(ba["rew"], ba["s_"], ba["a_"], ba["done"], GAMMA, out=ya)
    out["update_autograd"] = update_autograd
    keep.append((on_d, cr_d, tg_d, op_d, on_a, cr_a, tg_a, op_a))
    return out, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_marl_critic_grad needs a HIP device: a timing taken elsewhere says nothing")
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
            for num, den in (("autograd", "device"), ("autograd", "device_packed"), ("library", "device_packed"),
                             ("update_autograd", "update_device")):
                r = [o / d for o, d in zip(ev[num], ev[den])]
                row["%s_over_%s" % (num, den)] = round(median(r), 2)
                row["%s_over_%s_spread" % (num, den)] = [round(min(r), 2), round(max(r), 2)]
                row["%s_faster_than_%s_in_every_round" % (den, num)] = bool(min(r) > 1.0)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del forms, keep
            torch.cuda.empty_cache()
    result = dict(tool="tools/time_marl_critic_grad.py", device=torch.cuda.get_device_name(0), torch=torch.__version__, sizes=rows)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
