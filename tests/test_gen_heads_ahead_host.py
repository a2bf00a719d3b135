"""CPU test of the request schedule of the chunk heads in the HD row-per-lane GEN members (gen_leaf_rank(), gen_head_rank(),
k_step_gen.hip), restated in NumPy for (G, NP) of the three row-lane shapes and D in {1, 2} leaves ahead:

  * every chunk's head is requested exactly once;
  * no later than at the top of the leaf before its own (entry counts as before leaf 0);
  * the entry batch holds exactly the chunks of the first D leaves in execution order;
  * with D = 0 everything travels at entry (the code before).

The kernel asserts the same at compile time (gen_head_schedule_ok); this file keeps the rule readable and pins the order
row_tree_block() runs its leaves in: 0, 2, 1, 3 at G = 32."""
import numpy as np
import pytest

# (V, M) -> (G, NP): lanes per row of the reading form (fused_g) and float4 per row (M / 2)
SHAPES = {(8, 64): (32, 32), (16, 64): (32, 32), (4, 16): (16, 8)}
ENTRY = -1


def fused_g(V, M):
    p2 = lambda n: 1 << max(n - 1, 0).bit_length()          # noqa: E731
    g0 = min(p2(M // 2), 64)
    return max(g0, max(64 // p2(V), 8))


def bit_reverse(G, j):
    r, b = 0, 1
    while b < G // 8:
        r = (r << 1) | (1 if j & b else 0)
        b <<= 1
    return r


def leaf_rank(G, NP, J):
    """rank of leaf J among the leaves that run chains (8 J < NP), in row_tree_block()'s depth-first order"""
    return sum(1 for j in range(G // 8) if 8 * j < NP and bit_reverse(G, j) < bit_reverse(G, J))


def leaf_count(G, NP):
    return min(G, NP) // 8


def head_rank(G, NP, D, c):
    own = leaf_rank(G, NP, c % (G // 8))
    return ENTRY if D == 0 or own < D else own - D


def schedule(G, NP, D):
    """[ranks -1 .. NL - 1] -> chunks requested there, walking the kernel's control flow: the entry batch, then the top of
    every leaf in execution order"""
    NL, NCH = leaf_count(G, NP), NP // 8
    order = sorted((J for J in range(G // 8) if 8 * J < NP), key=lambda J: leaf_rank(G, NP, J))
    assert [leaf_rank(G, NP, J) for J in order] == list(range(NL))
    return {r: [c for c in range(NCH) if head_rank(G, NP, D, c) == r] for r in [ENTRY] + list(range(NL))}


@pytest.mark.parametrize("V,M", list(SHAPES))
def test_shapes_are_the_kernels(V, M):
    G, NP = SHAPES[(V, M)]
    assert G == fused_g(V, M) and NP == M // 2
    assert (NP + G - 1) // G == 1                           # NIT = 1: a leaf is one chunk at every row-lane shape


def test_leaf_order_at_four_leaves():
    assert sorted(range(4), key=lambda J: leaf_rank(32, 32, J)) == [0, 2, 1, 3]
    assert leaf_count(32, 32) == 4 and leaf_count(16, 8) == 1
    # NIT = 2 (no row-lane shape today): leaf J owns chunks J and J + G/8, and both heads travel together
    assert head_rank(32, 64, 1, 2) == head_rank(32, 64, 1, 6) == leaf_rank(32, 64, 2) - 1


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("V,M", list(SHAPES))
def test_every_chunk_once_and_before_its_leaf(V, M, D):
    G, NP = SHAPES[(V, M)]
    sch = schedule(G, NP, D)
    requested = np.sort(np.concatenate([np.asarray(v, dtype=np.int64) for v in sch.values()]))
    assert requested.tolist() == list(range(NP // 8))                             # each chunk exactly once
    for r, chunks in sch.items():
        for c in chunks:
            own = leaf_rank(G, NP, c % (G // 8))
            assert r <= own - 1, (r, c, own)                                      # no later than the leaf before its own
            assert r == max(own - D, ENTRY), (r, c, own)
    first = [c for c in range(NP // 8) if leaf_rank(G, NP, c % (G // 8)) < D]
    assert sch[ENTRY] == first and len(first) == min(D, leaf_count(G, NP)) * ((NP + G - 1) // G)


@pytest.mark.parametrize("V,M", list(SHAPES))
def test_distance_zero_is_everything_at_entry(V, M):
    G, NP = SHAPES[(V, M)]
    sch = schedule(G, NP, 0)
    assert sch[ENTRY] == list(range(NP // 8)) and all(not v for r, v in sch.items() if r != ENTRY)


def test_entry_burst_bytes_of_the_headline():
    """8 x 64: 836 B per env-step at entry, 512 of them heads; one leaf ahead leaves 128 B of heads there"""
    G, NP = SHAPES[(8, 64)]
    V, head_bytes = 8, 16
    for D, want in ((0, 512), (1, 128), (2, 256)):
        assert len(schedule(G, NP, D)[ENTRY]) * head_bytes * V == want
