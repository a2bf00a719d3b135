"""The order in which the fused step adds the partial sums of a row, stated twice in NumPy and compared bit for bit (no GPU).

The reading form (k_step_fused_pipe) and the GEN member's stage form add a row's G partials ACROSS lanes with
treduce<K, G/2> (risvec_step.hpp): a transposing butterfly from distance G/2 down to 1 whose partner at distance O is
lane ^ O, except the DPP mirrors at O = 8 (g <-> 15 - g within 16 lanes) and O = 4 (g <-> 7 - g within 8).  The GEN member's
row-per-lane form (row_tree / row_tree_block, k_step_gen.hip) adds the same partials IN one lane:

    s_G = p,    s_O[g] = s_2O[g] + s_2O[2 O - 1 - g if O in (8, 4) else g + O]  for g < O,    result s_1[0]

in blocks of 8 consecutive g, depth first.  A float add commutes but does not associate, so the two agree exactly when they
pair the same operands at every level.  `_treduce` restates the first (select form, and the row-swap form of distance 16 /
32), `_row_tree` the second; whoever changes one side has to change the other.  Covered: every (K, G, NIT, ragged) the
fixed GEN shapes have -- 8 x 64 and 16 x 64 (K 8, G 32), 4 x 16 (K 2, G 16, rows of 8 float4 on 16 lanes: ragged) and
16 x 256 (K 8, G 64, NIT 2), which the row-per-lane form does not take today but the tree is written for."""
import numpy as np
import pytest

F = np.float32

# (V, M) -> the tiling of PipeShape<V, M> (risvec_pipe.hpp): lanes per row G, loads per lane NIT, rows per unit PC
SHAPES = {(8, 64): dict(G=32, NIT=1, PC=4), (16, 64): dict(G=32, NIT=1, PC=4), (4, 16): dict(G=16, NIT=1, PC=1),
          (16, 256): dict(G=64, NIT=2, PC=4)}


def _partner(lane, O):
    """xchg<O> (risvec_step.hpp): quad permutes, the two DPP mirrors, ds_swizzle xor 16, __shfl_xor 32"""
    if O == 8:
        return (lane & ~15) | (15 - (lane & 15))
    if O == 4:
        return (lane & ~7) | (7 - (lane & 7))
    return lane ^ O


def _treduce(val, K, O, swap):
    """treduce<K, O> on val[lane, j] for the G lanes of one row group; returns val[:, 0] after the last stage"""
    val = val.copy()
    lanes = np.arange(val.shape[0])
    while O >= 1:
        p = _partner(lanes, O)
        hi = (lanes & O) != 0
        if K > 1 and swap and O in (16, 32):
            # v_permlane{16,32}_swap on (a, b) = (val[j], val[j + K/2]): the odd rows of a change places with the even rows of b
            for j in range(K // 2):
                a, b = val[:, j].copy(), val[:, j + K // 2].copy()
                a2 = np.where(hi, b[p], a)
                b2 = np.where(hi, b, a[p])
                val[:, j] = a2 + b2
            K //= 2
        elif K > 1:
            for j in range(K // 2):
                send = np.where(hi, val[:, j], val[:, j + K // 2])
                keep = np.where(hi, val[:, j + K // 2], val[:, j])
                val[:, j] = keep + send[p]
            K //= 2
        else:
            val[:, 0] = val[:, 0] + val[p, 0]
        O //= 2
    return val[:, 0]


def _cross_lane(p, K):
    """p[j, gl]: the partial of lane gl for value j (row in unit, re / im) -> the K sums, read where the kernel reads them:
    writer lane j * G / K"""
    outs = []
    for swap in (False, True):
        got = _treduce(np.ascontiguousarray(p.T), K, p.shape[1] // 2, swap)
        outs.append(np.array([got[j * (p.shape[1] // K)] for j in range(K)], dtype=F))
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), "select form and swap form of treduce differ"
    return outs[0]


def _row_tree_block(G, O, J, leaf):
    """row_tree_block<G, O, J> (k_step_gen.hip): s_O[8 J ... 8 J + 7]"""
    if O == G:
        return leaf(J)
    if O >= 16:
        return _row_tree_block(G, 2 * O, J, leaf) + _row_tree_block(G, 2 * O, J + O // 8, leaf)
    assert O == 8 and J == 0
    return _row_tree_block(G, 16, 0, leaf) + _row_tree_block(G, 16, 1, leaf)[::-1]


def _row_tree(p_row):
    """row_tree<G> on the G partials of one value"""
    G = len(p_row)
    s = _row_tree_block(G, 8, 0, lambda J: p_row[8 * J:8 * J + 8].copy())
    s = s[:4] + s[7:3:-1]                                  # O = 4: s[g] + s[7 - g]
    s = s[:2] + s[2:4]                                     # O = 2
    return F(s[0] + s[1])                                  # O = 1


def _partials(rng, G, NIT, NP, kind):
    """The partial of every lane gl for one value, formed as the kernels form it: from zero, one term per `it` in `it`
    order; the lanes past the end of a ragged row (gl + it G >= NP) multiply by b = 0 and hold an exact +0."""
    term = (rng.standard_normal((NIT, G)) * 10.0 ** rng.uniform(-3, 3, (NIT, G))).astype(F)
    if kind == "zeros":
        term[rng.random((NIT, G)) < 0.4] = F(0)
        term[:, 8:16] = F(0)                               # a whole chunk
    f4 = np.arange(G)[None, :] + np.arange(NIT)[:, None] * G
    term = np.where(f4 < NP, term, F(0))
    acc = np.zeros(G, dtype=F)
    for it in range(NIT):
        acc = acc + term[it]
    return acc


@pytest.mark.parametrize("kind", ["random", "zeros"])
@pytest.mark.parametrize("V,M", sorted(SHAPES))
def test_in_lane_order_gives_the_cross_lane_bits(V, M, kind):
    G, NIT, PC = SHAPES[(V, M)]["G"], SHAPES[(V, M)]["NIT"], SHAPES[(V, M)]["PC"]
    K, NP = 2 * PC, M // 2
    assert (NP % G != 0) == ((V, M) == (4, 16))            # the one ragged shape
    rng = np.random.default_rng(1000 * V + M + (kind == "zeros"))
    for _ in range(500):
        p = np.stack([_partials(rng, G, NIT, NP, kind) for _ in range(K)])
        want = _cross_lane(p, K)
        got = np.array([_row_tree(p[j]) for j in range(K)], dtype=F)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (V, M, kind, p)


def test_a_wrong_pairing_is_seen():
    """the yardstick itself: plain left-to-right summation, or xor partners where the mirrors stand, differs on these inputs"""
    rng = np.random.default_rng(7)
    differ_seq = differ_xor = 0
    for _ in range(200):
        p = _partials(rng, 32, 1, 32, "random")
        want = _cross_lane(np.stack([p] * 8), 8)[0]
        seq = F(0)
        for x in p:
            seq = F(seq + x)
        s = p[:16] + p[16:]
        s = s[:8] + s[8:]                                  # g + 8 instead of 15 - g
        s = s[:4] + s[4:]
        s = s[:2] + s[2:]
        differ_seq += seq.view(np.int32) != want.view(np.int32)
        differ_xor += F(s[0] + s[1]).view(np.int32) != want.view(np.int32)
    assert differ_seq > 100 and differ_xor > 50, (differ_seq, differ_xor)
