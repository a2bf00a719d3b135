"""The shapes at which the five learner-side MFMA kernels (`k_marl_critic`, `k_sarl_critic`, `k_sarl_actor`,
`k_marl_critic_wide`, `k_local_critics`) are swept: every template instantiation and every edge of their run-time
parameters, inside the domain their `*_supported()` functions advertise.  Shared by tests/test_mlp_sweep_hip.py (the
kernels against float64) and the test_*_host.py files (geometry, stream size, packing and, where fc1 <= 160, the NumPy
walk of the stream).  A plain module: no fixtures, no test collection.

Each case names the instantiation the library must dispatch to and the edge it is there for.  A case may be swapped for
another only if every instantiation and every edge below is still hit, with the reason written beside it."""
from typing import NamedTuple, Tuple


class Case(NamedTuple):
    dims: tuple
    kernel: str            # what `_native.last_kernel()` must start with after the fused forward
    edge: str


# ---------------------------------------------------------------------------------------------------------------------
# k_marl_critic<MT2,MT3>: dims = (S, A, fc1, fc2, fc3); KS = ceil((S + A) / 16), NG = fc1 / 32, MT2 = fc2 / 128,
# MT3 = fc3 / 128; kAhead = 4 k-steps of prefetch.
MARL_CRITIC = (
    Case((1, 1, 32, 128, 128), "k_marl_critic<1,1>",
         "KS = 1: nst < kAhead, every fc1 prefetch slot clamped; NG = 1: three wavefronts own no fc1 group and fc2 has "
         "nks = 2 < kAhead; the state / action boundary at k = 1"),
    Case((1, 15, 32, 512, 128), "k_marl_critic<4,1>",
         "S + A = 16 exactly: one full k-step, no padding; s_h sized by fc2, since 2 NG < 8 MT2"),
    Case((16, 1, 64, 128, 256), "k_marl_critic<1,2>",
         "S + A = 17: the second k-step holds one value and 15 zeros; the action is its first element"),
    Case((127, 1, 160, 256, 128), "k_marl_critic<2,1>",
         "S + A = 128, no zero padding; the boundary at k = 127; NG = 5: wavefront 0 owns two groups, the others one"),
    Case((1, 127, 1024, 128, 256), "k_marl_critic<1,2>",
         "NG = 32; s_h sized by fc1; 148 480 bytes of dynamic LDS (the > 64 KiB attribute path)"),
    Case((33, 46, 992, 512, 128), "k_marl_critic<4,1>",
         "NG = 31: wavefront 3 owns one group fewer; KS = 5: groups end inside a prefetch round of kAhead"),
    Case((24, 40, 96, 256, 256), "k_marl_critic<2,2>",
         "S + A = 64: KS = 4 = kAhead exactly, every fc1 prefetch slot filled once and none clamped before the last round; "
         "NG = 3: wavefront 3 owns no fc1 group"),
)
#: (index into MARL_CRITIC, n_nets): every case as a twin, the smallest and the largest as one net too.  The table holds five
#: of the six instantiations; <4,2> is asserted at the driver's shape by test_marl_critic_hip.py.  (That file's SMALL shape
#: selects <2,2> as well, but nothing there asserts which kernel ran.)  `BatchedTwinCritic.loss_backward` is swept over the
#: same runs (tests/test_marl_critic_grad_sweep_hip.py; the edges only the backward has are named there).
MARL_CRITIC_RUNS = tuple((i, 2) for i in range(len(MARL_CRITIC))) + ((0, 1), (4, 1))

# ---------------------------------------------------------------------------------------------------------------------
# k_sarl_critic<MT2,MT3>: dims = (IN, fc1, fc2, fc3, A); KS = ceil((IN + 1) / 16) (the bias row is input IN),
# KSA = ceil(A / 16).
SARL_CRITIC = (
    Case((15, 32, 128, 128, 1), "k_sarl_critic<1,1>",
         "IN = 15: the bias row is the last element of a full k-step (KS = 1); NG = 1; A = 1 (KSA = 1, 15 zeros)"),
    Case((16, 64, 128, 256, 16), "k_sarl_critic<1,2>",
         "IN = 16: the bias row opens a k-step of its own (KS = 2); A = 16: one full action k-step"),
    Case((128, 160, 256, 128, 96), "k_sarl_critic<2,1>",
         "IN = 128: KS = 9; A = 96: KSA = 6; NG = 5"),
    Case((47, 96, 256, 256, 17), "k_sarl_critic<2,2>",
         "IN + 1 = 48 fills KS = 3; A = 17: the second action k-step holds one value; NG = 3"),
    Case((127, 1024, 512, 128, 33), "k_sarl_critic<4,1>",
         "IN + 1 = 128: KS = 8 full; NG = 32: s_h sized by fc1, dynamic LDS > 64 KiB; A = 33"),
    Case((5, 992, 128, 256, 96), "k_sarl_critic<1,2>",
         "KS = 1 with NG = 31; KSA = 6 > kAhead with MT2 = 1"),
)

# ---------------------------------------------------------------------------------------------------------------------
# k_sarl_actor<MT,KS>: dims = (IN, fc1, fc2, A); MT = fc2 / 32; KS = ceil((IN + 1) / 16) padded up to the next of
# {3, 6, 7, 9}; NG = fc1 / 32; p1 = groups per pass-1 item; HT = ceil(A / 32).  `obs` = (V, tn) with V (tn + 5) = IN:
# the observation shape the inputs are drawn in.
class ActorCase(NamedTuple):
    dims: tuple
    kernel: str
    edge: str
    obs: Tuple[int, int]


SARL_ACTOR = (
    ActorCase((5, 32, 128, 1), "k_sarl_actor<4,3>",
              "two all-zero k-steps; NG = 1: a pass-1 item with one group of p1 = 4 filled, T = 3 items; A = 1", (1, 0)),
    ActorCase((47, 96, 256, 33), "k_sarl_actor<8,3>",
              "IN + 1 = 48 fills KS = 3; NG = 3; A = 33: the second head tile holds one action", (1, 42)),
    ActorCase((48, 160, 128, 32), "k_sarl_actor<4,6>",
              "ks 4 padded to 6; NG = 5 with p1 = 2: the last pass-1 item half filled; A = 32: one full head tile", (8, 1)),
    ActorCase((96, 64, 128, 65), "k_sarl_actor<4,7>",
              "ks 7 exact, 15 zeros behind the bias row; NG = 2; A = 65: the third head tile holds one action", (8, 7)),
    ActorCase((111, 992, 256, 96), "k_sarl_actor<8,7>",
              "IN + 1 = 112 fills KS = 7; NG = 31 with p1 = 3: no multiple; A = 96: three full head tiles", (3, 32)),
    ActorCase((112, 1024, 128, 96), "k_sarl_actor<4,9>",
              "ks 8 padded to 9: one all-zero k-step; NG = 32", (8, 9)),
    ActorCase((128, 1024, 256, 96), "k_sarl_actor<8,9>",
              "IN = 128: the bias row alone in k-step 9; the 156 KiB ring; NG = 32", (8, 11)),
)

# ---------------------------------------------------------------------------------------------------------------------
# k_marl_critic_wide<MT2,MT3> (BatchedTwinCritic(gemm="wide")): dims = (S, A, fc1, fc2, fc3); KS = ceil((S + A) / 16) walked in
# chunks of kWideChunk = 8 k-steps; a wavefront keeps the accumulators of all its fc1 groups (wave, wave + 4, ..: at most 8)
# across the chunks, and its weight prefetch walks (chunk, group, position) with each group's k-steps of a chunk padded to
# a multiple of kAhead = 4 positions; a padded position neither loads nor multiplies.  s_in holds one chunk, so the LDS is
# (8 + max(2 NG, 8 MT2)) 2 KiB + 1 KiB.
MARL_CRITIC_WIDE = (
    Case((1, 1, 32, 128, 256), "k_marl_critic_wide<1,2>",
         "KS = 1: one chunk shorter than kAhead, three padded positions; NG = 1: three wavefronts never fetch; inside the "
         "fused rule too, so compared with k_marl_critic bit for bit"),
    Case((127, 2, 160, 256, 128), "k_marl_critic_wide<2,1>",
         "S + A = 129: chunks 8 + 1, the second chunk holds ONE live column; the boundary at k = 127; NG = 5: wavefront 0 "
         "owns two groups, the others one, so the group advance differs between wavefronts that share the chunk barriers"),
    Case((128, 64, 992, 512, 128), "k_marl_critic_wide<4,1>",
         "chunks 8 + 4: the last chunk is exactly kAhead; the state ends on the chunk edge; NG = 31: wavefront 3 owns 7 "
         "groups, the others 8"),
    Case((3, 205, 64, 128, 128), "k_marl_critic_wide<1,1>",
         "chunks 8 + 5: one k-step past a kAhead block; NG = 2: two wavefronts idle in fc1"),
    Case((250, 6, 96, 256, 256), "k_marl_critic_wide<2,2>",
         "S + A = 256: two full chunks; the boundary inside the second chunk (k-step 15)"),
    Case((1, 511, 1024, 128, 256), "k_marl_critic_wide<1,2>",
         "S + A = 512, the rule's maximum: four full chunks, no padding; NG = 32: all 8 accumulator slots of every "
         "wavefront; 148 480 bytes of dynamic LDS (the > 64 KiB attribute path)"),
    Case((511, 1, 32, 512, 256), "k_marl_critic_wide<4,2>",
         "the lone action is the last column of the last chunk; NG = 1; s_h sized by fc2"),
    Case((90, 83, 128, 512, 128), "k_marl_critic_wide<4,1>",
         "chunks 8 + 3: a last chunk shorter than kAhead but longer than one; the last k-step has 13 live columns; NG = 4: "
         "one group per wavefront"),
)
#: (index into MARL_CRITIC_WIDE, n_nets): every case as a twin (the second net restages the input and reuses the
#: accumulators), the smallest and the rule's maximum as one net too.  All six instantiations are in the table.
MARL_CRITIC_WIDE_RUNS = tuple((i, 2) for i in range(len(MARL_CRITIC_WIDE))) + ((0, 1), (5, 1))

# ---------------------------------------------------------------------------------------------------------------------
# k_local_critics<MT2,MT3> (BatchedLocalCritics): dims = (V, S, A, fc1, fc2, fc3): V agents on grid row blockIdx.y, each with
# its own nets from the table net[agent * n_nets + c]; per agent the walk of k_marl_critic at (S, A): KS = ceil((S + A) / 16).
# With A = V + 2 the action can be built from the policy's heads: a one-hot at k in [S, S + V), then two powers.
LOCAL_CRITICS = (
    Case((1, 1, 1, 32, 128, 256), "k_local_critics<1,2>x1",
         "one agent: a grid of one row; KS = 1; NG = 1"),
    Case((16, 5, 18, 160, 256, 128), "k_local_critics<2,1>x16",
         "the agent limit; A = V + 2: the one-hot at k = 5 .. 20 spans three 8-value fragments and the k-step edge at 16; "
         "NG = 5"),
    Case((3, 16, 1, 96, 256, 256), "k_local_critics<2,2>x3",
         "S = 16: the action opens a k-step of its own with one value; NG = 3: wavefront 3 owns no fc1 group"),
    Case((2, 64, 64, 992, 512, 128), "k_local_critics<4,1>x2",
         "S + A = 128, no zero padding; NG = 31; dynamic LDS > 64 KiB"),
    Case((16, 127, 1, 64, 128, 128), "k_local_critics<1,1>x16",
         "the boundary at k = 127 for 16 agents: the widest rows of obs, one action value per agent"),
    Case((9, 5, 11, 1024, 128, 256), "k_local_critics<1,2>x9",
         "A = V + 2: the from-policy form with an odd agent count; NG = 32: s_h sized by fc1, dynamic LDS > 64 KiB"),
)
#: (index into LOCAL_CRITICS, n_nets): every case with twin nets per agent, the first and the fourth with one net per agent
#: too (the net table's stride is n_nets).  The table holds five of the six instantiations; <4,2> is asserted at the
#: driver's sizes by test_local_critics_hip.py, as <4,2> of the global kernel is by test_marl_critic_hip.py.
LOCAL_CRITICS_RUNS = tuple((i, 2) for i in range(len(LOCAL_CRITICS))) + ((0, 1), (3, 1))

#: rows of the long call: critics 70 = two full 32-row tiles and one of 6 rows; actor 161 = one full 128-row workgroup, a
#: full wavefront and one row.  Row 0 is all zero; the outputs are PAD rows longer and keep their sentinel beyond n.
CRITIC_ROWS, ACTOR_ROWS, PAD = 70, 161, 40


def seeds(kind: str, index: int) -> Tuple[int, int]:
    """(weight seed, batch seed) of case `index` of a list: fixed, so that the host check of the headroom (float32
    against float64 at these very inputs) and the GPU tests see the same numbers.  A twin's second net takes weight
    seed + 1.  "local": the seeds step by 100 per case, and net c of agent j takes weight seed + 10 j + c (`local_nets`)."""
    if kind == "local":
        return 1900 + 100 * index, 1900 + 100 * index + 5
    base = {"marl": 1100, "critic": 1300, "actor": 1500, "wide": 1700}[kind]
    if (kind, index) in _OTHER_WEIGHT_SEED:
        return _OTHER_WEIGHT_SEED[kind, index], base + 10 * index + 5
    return base + 10 * index, base + 10 * index + 5


# The actor's error measure divides by the row's largest |logit|, and with ONE action that is the row's only logit: where
# it crosses zero inside the batch the measure is ill-conditioned for any float32 forward (weight seed 1500: float32
# against float64 6.3e-6, 1501: 9.2e-5).  At seed 1508 every logit of the batch has magnitude above 1 and the float32
# forward sits at 2.9e-7, as at the other shapes.  test_mlp_sweep_host.py holds every case to that headroom.
_OTHER_WEIGHT_SEED = {("actor", 0): 1508}


def actor_weights(dims, seed):
    """A weight set of the actor under the reference's key names, float32 arrays, by the recipe of `driver_actor`
    (test_sarl_actor_hip.py): the reference's init ranges (networks.py:115-125: 1 / sqrt(fc1), 1 / sqrt(fc2), 0.003), the
    head weight widened 60 x so that the outputs span (0, 1), LayerNorm weights in [0.5, 1.5] and biases in +-0.2."""
    import numpy as np
    IN, F1, F2, A = dims
    rng = np.random.default_rng(seed)
    u = lambda r, *s: rng.uniform(-r, r, s).astype(np.float32)     # noqa: E731
    w = {"fc1.weight": u(F1 ** -0.5, F1, IN), "fc1.bias": u(F1 ** -0.5, F1), "fc2.weight": u(F2 ** -0.5, F2, F1),
         "fc2.bias": u(F2 ** -0.5, F2), "mu.weight": u(0.003, A, F2) * np.float32(60.0), "mu.bias": u(0.003, A)}
    for i, f in ((1, F1), (2, F2)):
        w["bn%d.weight" % i] = rng.uniform(0.5, 1.5, f).astype(np.float32)
        w["bn%d.bias" % i] = u(0.2, f)
    return w


def local_nets(dims, seed, n_nets=2):
    """[agent][net] weight sets of a LOCAL_CRITICS case under the reference's key names (`random_net` of
    marl_critic_ref.py at (S, A, fc1, fc2, fc3)): every agent its own, so that a mix-up in net[agent * n_nets + c] shows."""
    from tests.marl_critic_ref import random_net
    return [[random_net(dims[1:], seed + 10 * j + c) for c in range(n_nets)] for j in range(dims[0])]


def local_batch(dims, n, seed):
    """(obs [n, V, S], action [n, V, A]) of a LOCAL_CRITICS case: `random_batch` of marl_critic_ref.py at the flattened
    widths (V S, V A), row 0 all zero, seen per agent."""
    from tests.marl_critic_ref import random_batch
    V, S, A = dims[:3]
    obs, act = random_batch((V * S, V * A), n, seed)
    return obs.reshape(n, V, S), act.reshape(n, V, A)


def local_policy_inputs(dims, n, seed):
    """(heads [V, n, 4 + V], power [n, V, 2], action [n, V, V + 2], idx [V, n]) of a LOCAL_CRITICS case with A = V + 2: the
    planted logits of test_local_critics_hip.py (rows 0 .. 2 of every agent: the own logit largest, a tie, every other
    logit below finfo.min / 2), powers in (-1, 1), and the action `sac_agent.py:270-274` builds from them, in NumPy."""
    import numpy as np
    from tests.test_local_critics_hip import numpy_next_action, planted_heads
    V = dims[0]
    heads = planted_heads(V, n, seed)
    power = np.tanh(np.random.default_rng(seed + 1).normal(0, 1, (n, V, 2))).astype(np.float32)
    return (heads, power) + numpy_next_action(heads, power)


def case_id(case) -> str:
    return "x".join(str(d) for d in case.dims)


def dims_of(cases) -> list:
    """The distinct shapes of a case list, in order."""
    seen = []
    for c in cases:
        if c.dims not in seen:
            seen.append(c.dims)
    return seen
