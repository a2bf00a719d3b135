"""CPU tests of the reducer of tools/gen_wave_timeline.py on synthetic stamps: a known spread and last-alone time come back
exactly, wavefronts are grouped by the SIMD they ran on and ranked by entry whatever order they were written in, and stamps
that decrease inside a wavefront raise."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_wave_timeline", os.path.join(ROOT, "tools", "gen_wave_timeline.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

N_STAMPS = 9                                              # entry, first wait, four leaves, tree, late, end (M = 64)


def _wave(entry, phases):
    return entry + np.concatenate([[0], np.cumsum(phases)])


def _simd(base, entries, lives):
    """four wavefronts of one SIMD: entry offsets and lives given, the life split into eight phases 1 : 2 : ... : 8"""
    rows = []
    for e, life in zip(entries, lives):
        assert life % 36 == 0
        rows.append(_wave(base + e, np.arange(1, N_STAMPS) * (life // 36)))
    return np.array(rows, dtype=np.int64)


def test_known_spread_and_last_alone_come_back_exactly():
    # every SIMD: entries 0, 10, 20, 30 and lives 3600, 3780, 3960, 4320 -> ends 3600, 3790, 3980, 4350
    stamps = np.concatenate([_simd(1_000_000 * (s + 1), [0, 10, 20, 30], [3600, 3780, 3960, 4320]) for s in range(5)])
    key = np.repeat(np.arange(5) * 7 + 3, 4)
    r = T.reduce_timeline(stamps, key)
    assert r["n_simds"] == 5 and r["n_simds_other"] == 0
    assert r["entry"] == [0, 10, 20, 30]
    assert r["end"] == [3600, 3790, 3980, 4350]
    assert r["life"] == [3600, 3780, 3960, 4320]
    assert r["spread"] == 750.0 and r["last_alone"] == 370.0 and r["last_end"] == 4350.0
    assert r["rank_ends_last"] == [0.0, 0.0, 0.0, 1.0]
    assert r["phases"][0] == [100 * k for k in range(1, 9)]             # rank 0: 3600 / 36 = 100 per unit
    assert r["phases"][3] == [120 * k for k in range(1, 9)]
    assert len(T.phase_names(N_STAMPS)) == N_STAMPS - 1


def test_grouping_and_age_rank_do_not_depend_on_the_order_written():
    rng = np.random.default_rng(0)
    # two SIMDs whose oldest wavefront ends LAST (spread 353, alone 248), one whose youngest does (spread 111, alone 37)
    a = _simd(5_000, [0, 7, 9, 40], [3960, 3600, 3636, 3672])            # ends 3960, 3607, 3645, 3712
    b = _simd(9_000_000, [0, 7, 9, 40], [3960, 3600, 3636, 3672])
    c = _simd(77, [0, 1, 2, 3], [3600, 3636, 3672, 3708])                # ends 3600, 3637, 3674, 3711
    stamps = np.concatenate([a, b, c])
    key = np.array([11] * 4 + [12] * 4 + [500] * 4)
    ref = T.reduce_timeline(stamps, key)
    assert ref["rank_ends_last"] == [2 / 3, 0.0, 0.0, 1 / 3]
    assert ref["end"] == [3960, 3607, 3645, 3712]                        # medians over the three SIMDs, per rank
    assert ref["spread"] == 3960 - 3607 and ref["last_alone"] == 3960 - 3712
    perm = rng.permutation(12)
    got = T.reduce_timeline(stamps[perm], key[perm])
    for k in ("entry", "end", "life", "phases", "spread", "last_alone", "rank_ends_last"):
        assert got[k] == ref[k], k
    # a SIMD that held three wavefronts is counted and left out
    got = T.reduce_timeline(stamps[:11], key[:11])
    assert got["n_simds"] == 2 and got["n_simds_other"] == 1
    assert got["rank_ends_last"] == [1.0, 0.0, 0.0, 0.0]


def test_hardware_id_fields():
    hw = (5 << 13) | (1 << 12) | (9 << 8) | (2 << 6) | (3 << 4) | 7       # se 5, sh 1, cu 9, pipe 2, simd 3, wave 7
    k0, simd = T.simd_key(np.array([hw, hw ^ 0xF, hw ^ (1 << 6), hw ^ (1 << 4), hw ^ (1 << 8)]), np.array([3, 3, 3, 3, 3]))
    assert simd.tolist() == [3, 3, 3, 2, 3]
    assert k0[0] == k0[1] == k0[2]                                        # wave slot and pipe do not name a SIMD
    assert len({int(k0[0]), int(k0[3]), int(k0[4])}) == 3
    k1, _ = T.simd_key(np.array([hw]), np.array([4]))
    assert int(k1[0]) != int(k0[0])


def test_split_raw_reads_the_buffer_layout():
    W = 8
    raw = np.zeros((W, T.SLOTS), dtype=np.uint64)
    st = np.concatenate([_simd(1000, [0, 5, 6, 9], [3600] * 4), _simd(1000, [1, 2, 3, 4], [3636] * 4)])
    raw[:, :N_STAMPS] = st.astype(np.uint64)
    raw[:, T.SLOT_RT0] = 50
    raw[:, T.SLOT_RT1] = 50 + 150                                         # 1.5 us at 100 MHz
    raw[:4, T.SLOT_XCC], raw[4:, T.SLOT_XCC] = 2, 6
    raw[:, T.SLOT_HW] = np.uint64((N_STAMPS << 32) | (1 << 4))
    stamps, key, simd, tpu = T.split_raw(raw.reshape(-1))
    assert stamps.shape == (W, N_STAMPS) and (stamps == st).all()
    assert simd.tolist() == [1] * W and len(set(key[:4])) == 1 and key[0] != key[4]
    assert tpu == pytest.approx(np.median([3600 / 1.5] * 4 + [3636 / 1.5] * 4))
    raw[3, T.SLOT_HW] = np.uint64(((N_STAMPS - 1) << 32) | (1 << 4))
    with pytest.raises(ValueError):
        T.split_raw(raw)


def test_non_monotone_stamps_raise():
    stamps = np.concatenate([_simd(0, [0, 10, 20, 30], [3600] * 4) for _ in range(2)])
    key = np.repeat([1, 2], 4)
    T.reduce_timeline(stamps, key)
    bad = stamps.copy()
    bad[5, 4] = bad[5, 3] - 1
    with pytest.raises(ValueError, match=r"decrease.*\[5\]"):
        T.reduce_timeline(bad, key)
    with pytest.raises(ValueError):
        T.reduce_timeline(stamps[:3], key[:3])                            # no SIMD with four wavefronts
