"""Host cost of a bound step launch, without a device: the library is replaced by a stand-in whose entry points return
0, so what is timed is the launcher's own Python (the currency decision of `_currency.py` plus one call).  Three
launchers at (E, V, M) = (4, 8, 64): bind_step(fused=True), bind_step(bcd=True) under lazy_theta, bind_step_store(
fused=True).  Prints one JSON line: per launcher the median ns per call of each of `repeats` runs of `calls` launches.
RISVEC_TREE=<checkout> times that tree's package instead (the same-machine A/B: alternate the two)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.environ.get("RISVEC_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ris_vec_marl_amd import VecEnviron, reference_lanes  # noqa: E402
from ris_vec_marl_amd import _native as N  # noqa: E402
from ris_vec_marl_amd.replay import VecReplayBuffer  # noqa: E402


class StandIn:
    def __getattr__(self, name):
        fn = (lambda *a: 1) if name == "risvec_theta_by_index_supported" else (lambda *a: 0)
        self.__dict__[name] = fn
        return fn


def main(repeats=5, calls=200000):
    lib = StandIn()
    N.load, N.require_hip, N.stream = (lambda: lib), (lambda device: None), (lambda device: 0)
    E, V, M, L = 4, 8, 64, reference_lanes()
    act, part, ng = torch.zeros(E, 2, V), torch.full((E, V), -1, dtype=torch.int32), torch.full((E,), V, dtype=torch.int32)

    def env(lazy):
        e = VecEnviron(L["down_lanes"], L["up_lanes"], L["left_lanes"], L["right_lanes"], 400, 400, V, M, 3, n_envs=E,
                       device="cpu", seed=1, lazy_theta=lazy)
        e.make_new_game()
        e.compute_parms()
        e.Random_phase()
        return e

    a, b, c = env(False), env(True), env(False)
    ring = VecReplayBuffer(64, 5, V + 2, V, device="cpu")
    launchers = {"step_fused": a.bind_step(act, part, ng, fused=True),
                 "step_bcd_lazy": b.bind_step(act, part, ng, bcd=True),
                 "step_store": c.bind_step_store(ring, torch.zeros(E, V, 2), part, ng, torch.zeros(E, V, V), fused=True)}
    out = {}
    for name, launch in launchers.items():
        launch()
        launch()
        ns = []
        for _ in range(repeats):
            t0 = time.perf_counter_ns()
            for _ in range(calls):
                launch()
            ns.append(round((time.perf_counter_ns() - t0) / calls, 1))
        out[name] = ns
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:3]))
