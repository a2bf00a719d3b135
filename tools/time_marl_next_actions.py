#!/usr/bin/env python3
"""Time part 1 of the SAC learner's TD target -- `policy.sample_normal` for every agent, next_actions, the log-prob sums
(global_sac_critic.py:296-336) -- and the whole target it feeds:

  sample   forward + `BatchedPolicy.sample_normal(out=...)` (one hand-written launch after the forward) against
           forward + `sample_normal_torch` (the same computation with library kernels), same heads, same injected draws;
  target   `sample_normal(out=...)` -> `BatchedTwinCritic.td_target` (three launches) against the path of
           examples/marl_td_target.py: `choose_action`, one_hot / cat / amax / log with library kernels, `td_target`.

Interleaved in one process, HIP events, `--warmup` untimed calls of each form first, `--rounds` rounds of `--steps` calls,
median and every round reported; `*_faster_by_more_than_the_spread` says whether the slowest round of one form beats the
fastest of the other.  `library_ops` counts the ATen operators the library form dispatches besides its hand-written
launches (views and bare allocations left out: each is at least one library kernel), `hand_launches` the launches of the
hand-written form by construction.  Sizes: B = 64 / 4 096 / 32 768 for 8
vehicles (40 + 80 critic inputs) and 4 (20 + 24), the driver's hidden sizes.  Every size runs in a child process of its
own under a time limit; the first child that fails ends the run.

    python tools/time_marl_next_actions.py [--out profiles/marl_next_actions.json] [--rounds 7] [--steps 50] [--warmup 20]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VEHICLES = [8, 4]
ROWS = [32768, 4096, 64]
CHILD_LIMIT_S = 240
VIEWS = {"view", "_unsafe_view", "reshape", "transpose", "slice", "select", "expand", "unsqueeze", "squeeze", "t", "alias",
         "detach", "as_strided", "permute", "_reshape_alias", "unbind", "split", "lift_fresh", "empty", "empty_like",
         "empty_strided"}


def child(V, n, rounds, steps, warmup):
    import numpy as np
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from ris_vec_marl_amd import BatchedPolicy, BatchedTwinCritic
    if not torch.cuda.is_available():
        raise SystemExit("time_marl_next_actions needs a HIP device: a timing taken elsewhere says nothing")
    dev = "cuda:0"
    pol = BatchedPolicy(V, 5, 512, 256, device=dev, seed=3)
    pol.Wh.mul_(30.0)
    pol.bh[:, 0, 2:4] -= 1.5
    critic = BatchedTwinCritic(5 * V, V * (V + 2), 1024, 512, 256, device=dev, seed=5)
    rng = np.random.default_rng(1)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    states_ = T(rng.uniform(0, 1.2, (n, V * 5)).astype(np.float32))
    obs = states_.view(n, V, 5)
    mask = T((rng.uniform(size=(n, V, V)) < 0.7).astype(np.uint8))
    eps = T(rng.normal(size=(n, V, 2)).astype(np.float32))
    expo = T(np.maximum(rng.exponential(size=(n, V, V)), 1e-6).astype(np.float32))
    reward = T(rng.uniform(-6, 1, n).astype(np.float32))
    done = T(rng.uniform(size=n) < 0.01)
    coef = torch.tensor([0.15, 0.06], device=dev)
    na, sp, si = torch.empty(n, V * (V + 2), device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    y_h, y_l = torch.empty(n, device=dev), torch.empty(n, device=dev)

    def sample_hand():
        return pol.sample_normal(obs, mask, eps, expo, out=(na, sp, si))

    def sample_lib():
        return pol.sample_normal_torch(obs, mask, eps, expo)

    def target_hand():
        pol.sample_normal(obs, mask, eps, expo, out=(na, sp, si))
        return critic.td_target(reward, states_, na, done, 0.99, sp, si, coef, out=y_h)

    def target_lib():                                          # examples/marl_td_target.py:72-78
        power, probs, _ = pol.choose_action(obs, mask, eps, expo, want_onehot=False)
        onehot = torch.nn.functional.one_hot(probs.argmax(-1), V).float()
        nxt = torch.cat([onehot, power], dim=-1).contiguous()
        li = probs.amax(-1).clamp_min(1e-8).log().sum(-1)
        lp = torch.zeros(n, device=dev)
        return critic.td_target(reward, states_, nxt, done, 0.99, lp, li, coef, out=y_l)

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func.overloadpacket.__name__ not in VIEWS:
                self.n += 1
            return func(*args, **(kwargs or {}))

    def ops(fn):
        with Count() as c:
            fn()
        return c.n

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps

    def race(pair):
        for fn in pair.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in pair}
        for _ in range(rounds):                                # interleaved: what drifts, drifts for both
            for k, fn in pair.items():
                us[k].append(timed(fn))
        return us

    row = dict(rows=n, V=V, policy=[5, 512, 256], critic=[5 * V, V * (V + 2), 1024, 512, 256], policy_gemm=pol.gemm,
               critic_fused=bool(critic._fused(n)), steps_per_form=rounds * steps, warmup=warmup)
    h, l = sample_hand(), sample_lib()
    row["max_abs_diff_hand_vs_library"] = {k: float((a - b).abs().max()) for k, a, b in
                                           zip(("power", "probs", "logp_power", "logp_intent", "next_actions", "logp_power_sum",
                                                "logp_intent_sum"), h, l)}
    us = {"sample_" + k: v for k, v in race({"hand": sample_hand, "library": sample_lib}).items()}
    us.update({"target_" + k: v for k, v in race({"hand": target_hand, "library": target_lib}).items()})
    row["sample_hand_launches"], row["sample_library_ops"] = 2, ops(sample_lib)       # forward + sample_normal
    row["target_hand_launches"], row["target_library_ops"] = 3, ops(target_lib)       # ... + td_target
    for k, v in us.items():
        row["%s_us" % k] = round(sorted(v)[len(v) // 2], 2)
        row["%s_us_rounds" % k] = [round(t, 2) for t in v]
    for pre in ("sample_", "target_"):
        f, lb = us[pre + "hand"], us[pre + "library"]
        row[pre + "speedup"] = round(row[pre + "library_us"] / row[pre + "hand_us"], 2)
        row[pre + "hand_faster_by_more_than_the_spread"] = max(f) < min(lb)
        row[pre + "library_faster_by_more_than_the_spread"] = max(lb) < min(f)
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
        raise SystemExit("time_marl_next_actions needs a HIP device: a timing taken elsewhere says nothing")
    results = []
    for V in VEHICLES:
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
            json.dump(dict(tool="tools/time_marl_next_actions.py", sizes=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
