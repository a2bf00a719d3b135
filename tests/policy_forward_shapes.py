"""The shapes at which the policy forward (`BatchedPolicy.forward_heads`: `k_policy_layer1_v4<NT,8,SPLIT16>`,
`k_policy_layer1<FPL>`, `k_policy_heads_v4<NT>`, `k_policy_heads<FPL>` of csrc/k_policy.hip and `k_policy_mlp<MT>` of
csrc/k_policy_mlp.hip) is swept: every template instantiation and every edge of the run-time parameters, inside the
domain the library's guards admit.  Shared by tests/test_policy_forward_hip.py (the kernels against float64) and
tests/test_policy_forward_host.py (the table, the float64 restatement and the headroom of these very inputs).  A plain
module: no fixtures, no test collection.

Each case is (IN, fc1, fc2, V) -- input_dims, the two hidden sizes and the number of agents, H = 4 + V head outputs --
and names the kernels the library must dispatch to and the edge it is there for.  A case may be swapped for another
only if every instantiation and every edge below is still hit, with the reason written beside it.

The policy launchers do not report their kernel (`_native.note_kernel()` would clear the step's flags bench.py reads), so
the instantiation a case reaches is established on the host from the dispatch rules, restated here from k_policy.hip
(`policy_nt`, `policy_fpl`, `launch_policy_layer1`, `launch_policy_heads`, `launch_policy_layer1_split16`)."""
from typing import NamedTuple, Optional, Tuple

from tests import mlp_sweep_shapes as SW

INMAX = 8            # the inputs `k_policy_layer1_v4<NT, 8, SPLIT16>` unrolls over
LDS_LIMIT = 64 * 1024


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch rules of k_policy.hip
def _first_fitting(need: int) -> int:
    for f in (1, 2, 4, 8, 16):
        if need <= f:
            return f
    return 0


def need16(F: int) -> int:
    """rounds of 16 float4 chunks a row of F features takes in the 16-lanes-per-row kernels"""
    return (F // 4 + 15) // 16


def need64(F: int) -> int:
    """rounds of 64 features a row takes in the one-wavefront-per-row kernels"""
    return (F + 63) // 64


def nt(F: int) -> int:
    return _first_fitting(need16(F))


def fpl(F: int) -> int:
    return _first_fitting(need64(F))


def layer1_kernel(IN: int, F1: int) -> str:
    return "v4<%d>" % nt(F1) if F1 % 4 == 0 and IN <= INMAX and nt(F1) > 0 else "<%d>" % fpl(F1)


def heads_kernel(F2: int) -> str:
    return "v4<%d>" % nt(F2) if F2 % 4 == 0 and nt(F2) > 0 else "<%d>" % fpl(F2)


def split16_kernel(IN: int, F1: int) -> Optional[str]:
    """`k_policy_layer1_v4<NT, 8, true>`, or None where `launch_policy_layer1_split16` refuses"""
    return "v4<%d,8,true>" % nt(F1) if F1 % 4 == 0 and IN <= INMAX and nt(F1) > 0 else None


def layer1_lds(IN: int, F1: int) -> int:
    """bytes of dynamic LDS of both layer-1 kernels, what `risvec_policy_layer1` holds under 64 KiB"""
    return (IN + 3) * F1 * 4


def heads_lds(F2: int, H: int) -> int:
    """bytes of dynamic LDS of `k_policy_heads_v4` (the general kernel keeps no fc2 bias: F2 floats fewer), what
    `risvec_policy_heads` holds under 64 KiB for either"""
    return (3 * F2 + F2 * H + H) * 4


class Case(NamedTuple):
    dims: Tuple[int, int, int, int]      # (IN, fc1, fc2, V)
    layer1: str                          # the layer-1 kernel of the three-launch forms: "v4<NT>" or "<FPL>"
    heads: str                           # the heads kernel of the three-launch forms
    fused: Optional[str]                 # "k_policy_mlp<MT>" where the fused kernel is built for the shape
    modes: Tuple[str, ...]               # every `gemm=` the shape admits; the first is what BatchedPolicy picks by default
    edge: str


THREE, ONE, ALL = ("fp16x3", "fp32"), ("fp32",), ("fused", "fp16x3", "fp32")

# ---------------------------------------------------------------------------------------------------------------------
# Three launches, the 16-lanes-per-row kernels: fc % 4 == 0 and IN <= 8.  need = ceil(fc / 4 / 16) rounds of 16 chunks,
# padded to NT; 64 rows per block.
V4 = (
    Case((5, 20, 12, 2), "v4<1>", "v4<1>", None, THREE,
         "5 and 3 chunks: 11 and 13 of the 16 lanes of a row idle; H = 6"),
    Case((8, 64, 68, 1), "v4<1>", "v4<2>", None, THREE,
         "IN = 8 = INMAX; fc1 fills round 0 exactly; fc2: the second round holds one chunk; V = 1, H = 5"),
    Case((5, 128, 132, 3), "v4<2>", "v4<4>", None, THREE,
         "need = 3 rounds in NT = 4: the third holds one chunk, the fourth none; H = 7"),
    Case((5, 256, 260, 16), "v4<4>", "v4<8>", None, THREE,
         "need = 5 in NT = 8; H = 20: the 16-output block loop runs twice (16 + 4)"),
    Case((5, 260, 256, 4), "v4<8>", "v4<4>", None, THREE,
         "the layer-1 twin of the row above; H = 8"),
    Case((5, 516, 512, 8), "v4<16>", "v4<8>", None, THREE,
         "need = 9 in NT = 16; H = 12"),
    Case((5, 1024, 1024, 8), "v4<16>", "v4<16>", None, THREE,
         "both full; heads LDS = 61 488 B: the largest H that the guard admits at fc2 = 1024"),
)

# Three launches, the one-wavefront-per-row kernels: fc % 4 != 0, or IN > 8 for layer 1.  need = ceil(fc / 64) rounds,
# padded to FPL; 32 rows per block.  gemm="fp16x3" is refused at these shapes.
GENERAL = (
    Case((5, 1, 63, 2), "<1>", "<1>", None, ONE,
         "one live lane; LayerNorm over one feature (variance 0, output = ReLU(bias)); 63 of 64 lanes"),
    Case((9, 128, 65, 5), "<2>", "<2>", None, ONE,
         "IN = 9 > INMAX with fc1 % 4 == 0 takes the general kernel; fc2: the second round holds one feature; H = 9"),
    Case((3, 130, 130, 16), "<4>", "<4>", None, ONE,
         "need = 3 in FPL = 4: round 3 holds two features, round 4 none; IN = 3"),
    Case((5, 258, 258, 33), "<8>", "<8>", None, ONE,
         "need = 5 in FPL = 8; V = 33: 37 outputs one wave reduction each, grid.y = 33"),
    Case((5, 1023, 514, 4), "<16>", "<16>", None, ONE,
         "need = 16 and 9"),
)

# `k_policy_mlp<MT>`, MT = fc2 / 32, NG = fc1 / 32 groups through a ring of kRing = 3 slots staged two groups ahead;
# 256 rows per workgroup.  Every fused shape is a split shape too, so all three modes run.
FUSED = (
    Case((1, 32, 128, 1), "v4<1>", "v4<2>", "k_policy_mlp<4>", ALL,
         "IN = 1; NG = 1: nothing prefetched, the head weight is staged by the `NG == 1` branch; H = 5: scalar stores"),
    Case((2, 64, 256, 20), "v4<1>", "v4<4>", "k_policy_mlp<8>", ALL,
         "IN = 2; NG = 2: the head weight is staged at g = 0; H = 24: all three float4 stores of both lane halves, and "
         "the largest H"),
    Case((3, 96, 128, 4), "v4<2>", "v4<2>", "k_policy_mlp<4>", ALL,
         "IN = 3; NG = 3: stage(2) lands on the slot that held the group-0 fc1 operand; H = 8"),
    Case((4, 128, 256, 5), "v4<2>", "v4<4>", "k_policy_mlp<8>", ALL,
         "IN = 4; NG = 4: the first reuse of a ring slot; H = 9: scalar path, one head in the second group of four"),
    Case((5, 992, 128, 19), "v4<16>", "v4<2>", "k_policy_mlp<4>", ALL,
         "NG = 31; H = 23"),
    Case((5, 1024, 256, 8), "v4<16>", "v4<4>", "k_policy_mlp<8>", ALL,
         "NG = 32; H = 12"),
)

LISTS = {"v4": V4, "general": GENERAL, "fused": FUSED}
#: every (kind, index) of the sweep, and its pytest id
RUNS = tuple((kind, i) for kind in ("v4", "general", "fused") for i in range(len(LISTS[kind])))

# Refusals, raised before any launch.
HEADS_LDS_OVER = (5, 1024, 1024, 9)          # H = 13: 65 588 B of heads LDS, one agent more than the last V4 case
LAYER1_LDS_LAST, LAYER1_LDS_OVER = (13, 1024), (14, 1024)    # (IN, fc1): 65 536 B is admitted, 69 632 B is not
FUSED_H_OVER = (5, 64, 128, 21)              # H = 25 > 24: gemm="fused" raises, the default is "fp16x3"

#: rows of every call.  `_v4`: four blocks of 64 and 33 rows, so the last wavefront's last group of four has one live row
#: and three dead ones in its DPP exchanges; general: nine blocks of 32 and one row; fused: one workgroup of 256, then a
#: full wavefront, one wavefront with a single live lane and six with none that still take part in every barrier.
ROWS = 289
#: the shorter calls whose rows must equal the long call's bit for bit
SHORT_ROWS = (1, 33)
#: sentinel words in front of and behind every output written through the C ABI
GUARD = 64


def case_of(kind: str, index: int) -> Case:
    return LISTS[kind][index]


def case_id(case: Case) -> str:
    return "x".join(str(d) for d in case.dims)


def run_id(run) -> str:
    return case_id(case_of(*run))


def heads_of(case: Case) -> int:
    return 4 + case.dims[3]


def seeds(kind: str, index: int) -> Tuple[int, int]:
    """(weight seed, batch seed) of case `index` of a list: fixed, so that the host check of the headroom (float32
    against float64 at these very inputs) and the GPU tests see the same numbers.  Agent a takes weight seed + a; the
    heads-only launch draws its `g` with batch seed + 1."""
    base = {"v4": 2100, "general": 3100, "fused": 4100}[kind]
    return _OTHER_WEIGHT_SEED.get((kind, index), base + 100 * index), base + 100 * index + 50


# Cases whose first weight seed left a float32 forward outside BAR / 8 of float64 (test_policy_forward_host.py holds
# every case to that headroom), with the figure that ruled the first seed out.
_OTHER_WEIGHT_SEED = {}


def agent_weights(dims, seed):
    """One agent's weight set under the reference's key names (sac_agent.py:36-50), float32 arrays, by the recipe of
    `mlp_sweep_shapes.actor_weights` with H = 4 + V head rows: the reference's init ranges (1 / sqrt(fc1), 1 / sqrt(fc2),
    0.003), the head weights widened 60 x, LayerNorm weights in [0.5, 1.5] and biases in +-0.2.  The head rows are dealt
    to mu (2), log_std (2) and intent_logits (V).  In both LayerNorms feature 0 has weight -1 and feature F - 1 weight
    2.0: the first and the last lane or chunk carry a parameter that no other feature has."""
    import numpy as np
    IN, F1, F2, V = dims
    w = SW.actor_weights((IN, F1, F2, 4 + V), seed)
    hw, hb = w.pop("mu.weight"), w.pop("mu.bias")
    for name, lo, hi in (("mu", 0, 2), ("log_std", 2, 4), ("intent_logits", 4, 4 + V)):
        w[name + ".weight"], w[name + ".bias"] = np.ascontiguousarray(hw[lo:hi]), np.ascontiguousarray(hb[lo:hi])
    for i in (1, 2):
        w["bn%d.weight" % i][0] = -1.0
        w["bn%d.weight" % i][-1] = 2.0
    return w


def case_weights(kind: str, index: int) -> list:
    """every agent of a case has its own weights"""
    dims = case_of(kind, index).dims
    return [agent_weights(dims, seeds(kind, index)[0] + a) for a in range(dims[3])]


def observations(dims, n, seed):
    """obs [n, V, IN] float32: row 0 all zero (LayerNorm-1 statistics from the bias row alone), row 1 all 1.2, the others
    uniform in [0, 1.2), the range of the env's observations"""
    import numpy as np
    IN, _, _, V = dims
    o = np.random.default_rng(seed).uniform(0.0, 1.2, (n, V, IN)).astype(np.float32)
    o[0] = 0.0
    if n > 1:
        o[1] = np.float32(1.2)
    return o


def random_g(dims, n, seed):
    """g [V, n, fc2] float32, the input of the heads launch on its own: an fc2 product without its bias, drawn on the
    host (no GEMM library in the comparison); standard normal halved, row 0 all zero (LayerNorm-2 of the bias alone)"""
    import numpy as np
    _, _, F2, V = dims
    g = (0.5 * np.random.default_rng(seed).standard_normal((V, n, F2))).astype(np.float32)
    g[:, 0] = 0.0
    return g
