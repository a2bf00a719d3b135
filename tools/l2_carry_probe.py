#!/usr/bin/env python3
"""Do clean L2 lines survive a kernel boundary, and is block -> XCD the same from launch to launch?

membench_read_walk gives workgroup b chunk b of the buffer in every launch and walks it front to back (reverse = 0) or
back to front (reverse = 1).  Per buffer size and grid, in ONE process: 200 back-to-back launches (a) always forward,
(b) alternating direction, five rounds each, interleaved; us per launch min / median / max over the rounds.  With lines
carried over in L2, (a) beats the fabric rate while the buffer fits the 8 x 4 MiB of L2, and (b) beats (a) above that
by about the L2's share of the buffer.  Also: whether the XCC id every block recorded was identical over 8 consecutive
launches, and whether blocks b and b + 8 shared one.  One JSON line per case; --out writes the list as well."""
import argparse
import ctypes as C
import json
import os
import statistics

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MB = 1000 * 1000
SIZES_MB = (16, 24, 40, 80, 155)
GRIDS = (512, 2048)
LAUNCHES, ROUNDS, WARM = 200, 5, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = C.CDLL(os.path.join(HERE, "membench", "libmembench.so"))
    lib.membench_read_walk.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.membench_read_walk.restype = C.c_int
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for mb in SIZES_MB:
        n4 = mb * MB // 16
        src = torch.empty(n4 * 4, dtype=torch.float32, device=dev).normal_()
        for blocks in GRIDS:
            sink = torch.empty(blocks * 256, dtype=torch.float32, device=dev)
            xcc = torch.full((8, blocks), -1, dtype=torch.int32, device=dev)

            def go(rev, xrow=None):
                rc = lib.membench_read_walk(src.data_ptr(), n4, sink.data_ptr(), blocks, rev,
                                            None if xrow is None else xcc[xrow].data_ptr(), stream)
                assert rc == 0, rc

            def timed(alternate):
                for i in range(WARM):
                    go(i & 1 if alternate else 0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(LAUNCHES):
                    go(i & 1 if alternate else 0)
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b) * 1e3 / LAUNCHES

            fwd, alt = [], []
            for _ in range(ROUNDS):
                fwd.append(timed(False))
                alt.append(timed(True))
            for i in range(8):
                go(i & 1, i)
            torch.cuda.synchronize()
            x = xcc.cpu()
            same = bool((x == x[0]).all())
            by_label = [sorted(set(x[0, r::8].tolist())) for r in range(8)]
            ref = float(sink.double().sum())
            go(1)
            torch.cuda.synchronize()
            rev_sum = float(sink.double().sum())

            def mmm(v):
                return [round(min(v), 2), round(statistics.median(v), 2), round(max(v), 2)]

            row = dict(MB=mb, bytes=n4 * 16, blocks=blocks, forward_us=mmm(fwd), alternating_us=mmm(alt),
                       forward_GBps=round(n4 * 16 / statistics.median(fwd) / 1e3),
                       alternating_GBps=round(n4 * 16 / statistics.median(alt) / 1e3),
                       alt_over_fwd=round(statistics.median(alt) / statistics.median(fwd), 4),
                       xcc_same_over_8_launches=same, launches_differing=int((x != x[0]).any(dim=1).sum()),
                       xcc_of_label=by_label, xcc_min=int(x.min()), xcc_max=int(x.max()),
                       sums_agree=abs(ref - rev_sum) <= 1e-3 * max(1.0, abs(ref)))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del src
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
