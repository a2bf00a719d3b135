#!/usr/bin/env python3
"""Time every agent's local TD target (`Agent.local_learn`'s target, sac_agent.py:269-284) two ways, interleaved in one
process, HIP events, every round reported:

  one_launch   `BatchedLocalCritics.td_target(heads=..., power=...)`: all V agents in ONE launch (`risvec_local_critics`),
               strided columns read in place, the one-hot built in the kernel;
  per_agent    what there was before it: per agent the one-hot from the masked logits with library operators
               (clone, index fill, argmax, one_hot, cat), contiguous copies of the agent's columns (obs, reward, the two
               log-probabilities) and one `BatchedTwinCritic(5, V + 2).td_target` launch -- V launches of the global
               kernel plus about ten library operators per agent.

Both read the same `heads` (the policy forward is not part of either) and FROZEN weights.  The two targets differ on
`done` rows with an infinite entropy term only (product against select), which the inputs here do not contain.

    python tools/time_local_critics.py [--out profiles/local_critics.json] [--rounds 7] [--steps 50] [--warmup 20]

Every size runs in a child process of its own under a time limit; the first child that fails ends the run.  The spread
between rounds is reported as (max - min) / median per form, and `one_launch_faster_by_more_than_the_spread` says whether
the slowest one-launch round beat the fastest per-agent round.  One JSON line per size."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AGENTS = [4, 8]
ROWS = [64, 4096, 32768]
HIDDEN = (1024, 512, 256)                         # the driver's
CHILD_LIMIT_S = 240


def child(V, n, rounds, steps, warmup):
    import numpy as np
    import torch
    from ris_vec_marl_amd import BatchedLocalCritics, BatchedTwinCritic
    from ris_vec_marl_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("time_local_critics needs a HIP device: a timing taken elsewhere says nothing")
    dev = "cuda:0"
    local = BatchedLocalCritics(V, 5, None, *HIDDEN, device=dev, seed=5, gemm="fused")
    twins = []
    for j in range(V):
        t = BatchedTwinCritic(5, V + 2, *HIDDEN, device=dev, gemm="fused")
        for net in local.nets[j]:
            net.Wq.mul_(8.0)
        t.load_state_dict(*[net.state_dict() for net in local.nets[j]])
        twins.append(t)
    rng = np.random.default_rng(1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)      # noqa: E731
    obs = f32(rng.uniform(0, 1.2, (n, V, 5)))
    heads = f32(rng.normal(0, 1.5, (V, n, 4 + V)))
    power = f32(np.tanh(rng.normal(0, 1, (n, V, 2))))
    reward = f32(rng.uniform(-6, 1, (n, V)))
    done = torch.from_numpy(rng.uniform(size=n) < 0.01).to(dev)
    lp, li = f32(rng.uniform(-8, 4, (n, V))), f32(rng.uniform(-12, 0, (n, V)))
    coef = torch.tensor([0.15, 0.06], device=dev)
    y_one = torch.empty(V, n, device=dev)
    y_per = torch.empty(V, n, device=dev)
    neg = torch.finfo(torch.float32).min / 2

    def one_launch():
        local.td_target(reward, obs, done, 0.99, heads=heads, power=power, logp_power=lp, logp_intent=li, coef=coef, out=y_one)

    def per_agent():
        for j, twin in enumerate(twins):
            logits = heads[j, :, 4:].clone()
            logits[:, j] = neg
            onehot = torch.nn.functional.one_hot(torch.argmax(logits, dim=-1), num_classes=V).float()
            action = torch.cat([onehot, power[:, j]], dim=1)
            twin.td_target(reward[:, j].contiguous(), obs[:, j].contiguous(), action, done, 0.99, lp[:, j].contiguous(),
                           li[:, j].contiguous(), coef, out=y_per[j])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps
    forms = {"one_launch": one_launch, "per_agent": per_agent}
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(rounds):                                    # interleaved: what drifts, drifts for both
        for k, fn in forms.items():
            us[k].append(timed(fn))
    one_launch()
    row = dict(rows=n, n_agents=V, hidden=list(HIDDEN), n_nets=2, steps_per_form=rounds * steps, warmup=warmup, weights="frozen",
               kernel=N.last_kernel(), workgroups=V * ((n + 31) // 32), max_abs_y_diff=float((y_one - y_per).abs().max()))
    for k, v in us.items():
        med = sorted(v)[len(v) // 2]
        row["%s_us" % k] = round(med, 2)
        row["%s_us_rounds" % k] = [round(t, 2) for t in v]
        row["%s_spread" % k] = round((max(v) - min(v)) / med, 4)
    row["speedup"] = round(row["per_agent_us"] / row["one_launch_us"], 2)
    row["one_launch_faster_every_round"] = all(a < b for a, b in zip(us["one_launch"], us["per_agent"]))
    row["one_launch_faster_by_more_than_the_spread"] = max(us["one_launch"]) < min(us["per_agent"])
    row["one_launch_slower_by_more_than_the_spread"] = min(us["one_launch"]) > max(us["per_agent"])
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", nargs=2, type=int, default=None, metavar=("V", "ROWS"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child, args.rounds, args.steps, args.warmup)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_local_critics needs a HIP device: a timing taken elsewhere says nothing")
    results = []
    for V in AGENTS:
        for n in ROWS:                                         # a fresh process per size, each under its own limit
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--steps", str(args.steps),
                                  "--warmup", str(args.warmup), "--child", str(V), str(n)], capture_output=True, text=True,
                                 timeout=CHILD_LIMIT_S)
            if out.returncode != 0:
                raise SystemExit("size V=%d x %d failed with status %d; nothing further is run\n%s"
                                 % (V, n, out.returncode, out.stderr[-2000:]))
            line = out.stdout.strip().splitlines()[-1]
            results.append(json.loads(line))
            print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/time_local_critics.py", sizes=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
