#!/usr/bin/env python3
"""Diagnostic: how the four wavefronts of a SIMD get through the row-per-lane GEN member of the headline shape
(32 768 x 8 x 64, k_step_fused_gen<8,64,MarlCore,TK,ONE,HD>).

Runs bench.py's default workload on the STAMPS build of the library (make -C ris_vec_marl_amd/csrc gen_stamps ->
librisvec_gen_stamps.so: the shipped kernel's schedule, with -DRISVEC_GEN_STAMPS=1): there gen_row_lane_form writes, per
wavefront, s_memtime at entry / behind the first vmcnt wait / behind each leaf in execution order / behind row_tree /
behind the wait for late_args() / behind the last store, and its hardware id.  The shipped kernel executes no stamp.

    python tools/gen_wave_timeline.py --lib ris_vec_marl_amd/csrc/librisvec_gen_stamps.so --tag r13a_parent

writes profiles/<tag>_gen_timeline.json: wavefronts grouped by (XCC, SE, SH, CU, SIMD), ranked by entry time ("age": 0 the
oldest), median over SIMDs and launches of each phase's duration per rank, each rank's end relative to the SIMD's first
entry, the spread (last end - first end) and the time the last wavefront runs alone (last end - the end before it).

Stamps cost wave cycles (about a tenth) and their fences forbid overlaps the real kernel has: compare BUILDS with this,
do not quote its times as the kernel's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLOTS = 16                      # uint64 per wavefront in the stamp buffer (kGenStampSlots, k_step_gen.hip)
SLOT_RT0, SLOT_RT1, SLOT_XCC, SLOT_HW = 12, 13, 14, 15
MAX_STAMPS = 12


def phase_names(n_stamps: int) -> list:
    """names of the n_stamps - 1 phases between consecutive stamps: entry, first wait, leaves ..., tree, late, end"""
    n_leaf = n_stamps - 5
    if n_leaf < 1:
        raise ValueError("a row-lane wavefront stamps at least one leaf (got %d stamps)" % n_stamps)
    return (["entry->first_wait", "first_wait->leaf0"] + ["leaf%d->leaf%d" % (i - 1, i) for i in range(1, n_leaf)]
            + ["leaf%d->row_tree" % (n_leaf - 1), "row_tree->late_args", "late_args->last_store"])


def simd_key(hw_id, xcc_id):
    """(XCC, SE, SH, CU, SIMD) of HW_REG_HW_ID / HW_REG_XCC_ID as one integer, and the SIMD id alone.
    HW_ID (gfx9): wave_id [3:0], simd_id [5:4], pipe_id [7:6], cu_id [11:8], sh_id [12], se_id [15:13]."""
    hw = np.asarray(hw_id, dtype=np.int64)
    xcc = np.asarray(xcc_id, dtype=np.int64) & 0xF
    simd = (hw >> 4) & 0x3
    cu = (hw >> 8) & 0xF
    sh = (hw >> 12) & 0x1
    se = (hw >> 13) & 0x7
    return ((((xcc * 8 + se) * 2 + sh) * 16 + cu) * 4 + simd), simd


def split_raw(raw):
    """the stamp buffer of one launch [W, SLOTS] uint64 -> (stamps [W, n] int64, key [W], simd [W], ticks per us or None)"""
    raw = np.asarray(raw, dtype=np.uint64).reshape(-1, SLOTS)
    n = (raw[:, SLOT_HW] >> np.uint64(32)).astype(np.int64)
    if (n != n[0]).any() or not (5 < n[0] <= MAX_STAMPS):
        raise ValueError("wavefronts disagree on the number of stamps, or wrote none: %r" % np.unique(n))
    hw = (raw[:, SLOT_HW] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    key, simd = simd_key(hw, raw[:, SLOT_XCC].astype(np.int64))
    stamps = raw[:, :n[0]].astype(np.int64)
    # s_memrealtime runs at 100 MHz: the shader clock over the wavefront's life, median over wavefronts
    rt = (raw[:, SLOT_RT1] - raw[:, SLOT_RT0]).astype(np.int64)
    life = stamps[:, -1] - stamps[:, 0]
    ok = rt > 0
    tpu = float(np.median(life[ok] / (rt[ok] / 100.0))) if ok.any() else None
    return stamps, key, simd, tpu


def reduce_timeline(stamps, key, per_simd: int = 4) -> dict:
    """stamps [W, S] ticks of one launch, key [W] the SIMD a wavefront ran on.  Wavefronts are grouped by key and ranked by
    entry (stamp 0; ties by index); only SIMDs that held exactly `per_simd` wavefronts are reduced.  All results are
    medians over those SIMDs, in ticks.  Raises ValueError if any wavefront's stamps decrease."""
    stamps = np.asarray(stamps, dtype=np.int64)
    key = np.asarray(key, dtype=np.int64)
    if stamps.ndim != 2 or stamps.shape[0] != key.shape[0] or stamps.shape[1] < 2:
        raise ValueError("stamps [W, S >= 2] and key [W] expected")
    bad = np.nonzero((np.diff(stamps, axis=1) < 0).any(axis=1))[0]
    if bad.size:
        raise ValueError("stamps decrease in wavefront(s) %s" % bad[:8].tolist())
    order = np.lexsort((np.arange(len(key)), stamps[:, 0], key))       # by key, then entry, then index
    ks = key[order]
    starts = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
    counts = np.diff(np.r_[starts, len(ks)])
    full = starts[counts == per_simd]
    if full.size == 0:
        raise ValueError("no SIMD held %d wavefronts (counts seen: %s)" % (per_simd, np.unique(counts).tolist()))
    idx = order[full[:, None] + np.arange(per_simd)[None, :]]         # [n_simd, rank] -> wavefront
    t = stamps[idx]                                                   # [n_simd, rank, S]
    t0 = t[:, :, 0].min(axis=1)
    entry = t[:, :, 0] - t0[:, None]
    end = t[:, :, -1] - t0[:, None]
    phases = np.diff(t, axis=2)
    end_sorted = np.sort(end, axis=1)
    spread = end_sorted[:, -1] - end_sorted[:, 0]
    alone = end_sorted[:, -1] - end_sorted[:, -2]
    last_rank = end.argmax(axis=1)
    med = lambda a, ax=0: np.median(a, axis=ax)                       # noqa: E731
    return dict(n_simds=int(full.size), n_simds_other=int((counts != per_simd).sum()), per_simd=per_simd,
                entry=med(entry).tolist(), end=med(end).tolist(), life=med(end - entry).tolist(),
                phases=med(phases).tolist(), spread=float(med(spread)), last_alone=float(med(alone)),
                last_end=float(med(end_sorted[:, -1])),
                rank_ends_last=[float((last_rank == r).mean()) for r in range(per_simd)],
                simd_rows=idx.tolist() if full.size <= 8 else None)


def summarize(launches: list, ticks_per_us) -> dict:
    """median over launches of reduce_timeline()'s figures; ticks, and microseconds where the clock is known"""
    keys = ("entry", "end", "life", "phases", "spread", "last_alone", "last_end", "rank_ends_last")
    out = {k: np.median(np.array([r[k] for r in launches], dtype=np.float64), axis=0).tolist() for k in keys}
    out["n_launches"] = len(launches)
    out["n_simds"] = int(np.median([r["n_simds"] for r in launches]))
    out["n_simds_other"] = int(np.median([r["n_simds_other"] for r in launches]))
    if ticks_per_us:
        out["ticks_per_us"] = ticks_per_us
        out["us"] = {k: (np.array(out[k]) / ticks_per_us).round(3).tolist() for k in keys if k != "rank_ends_last"}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", required=True, help="the STAMPS build of the library: librisvec_gen_stamps.so (make gen_stamps)")
    ap.add_argument("--tag", required=True, help="profiles/<tag>_gen_timeline.json")
    ap.add_argument("--launches", type=int, default=32, help="launches reduced (each the last of a back-to-back burst)")
    ap.add_argument("--burst", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.environ["RISVEC_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    from bench import build_env, synthetic_groups
    from ris_vec_marl_amd import _native as N

    E, V, M = 32768, 8, 64
    dev = torch.device("cuda:0")
    lib = N.load()
    set_buf = lib.risvec_gen_stamps_buffer                  # AttributeError: not a STAMPS build
    set_buf.restype, set_buf.argtypes = C.c_int, [C.c_void_p, C.c_longlong]
    env = build_env(E, V, M, dev, 0, 0)
    rng = np.random.default_rng(1234)
    action = torch.from_numpy(rng.uniform(0, 1, (E, 2, V)).astype(np.float32)).to(dev)
    p, n = synthetic_groups(E, V, rng)
    partner, ng = torch.from_numpy(p).to(dev), torch.from_numpy(n).to(dev)
    step = env.bind_step(action, partner, ng, None, fused=True, metrics=True, power_w=False, obs=True)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    assert N.last_gen_groups_per_wave() == 1, "the headline must run the one-group GEN member"
    kernel = N.last_kernel()
    n_waves = E * V // 64
    buf = torch.zeros(n_waves * SLOTS, dtype=torch.int64, device=dev)
    assert set_buf(buf.data_ptr(), n_waves) == 0
    launches, clocks = [], []
    for _ in range(a.launches):
        for _ in range(a.burst):
            step()
        torch.cuda.synchronize()
        stamps, key, _, tpu = split_raw(buf.cpu().numpy().view(np.uint64))
        launches.append(reduce_timeline(stamps, key))
        if tpu:
            clocks.append(tpu)
    set_buf(None, 0)
    tpu = float(np.median(clocks)) if clocks else None
    res = dict(tag=a.tag, lib=os.path.basename(a.lib), kernel=kernel, shape=[E, V, M], burst=a.burst,
               phase_names=phase_names(stamps.shape[1]), **summarize(launches, tpu))
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, "%s_gen_timeline.json" % a.tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
