#!/usr/bin/env python3
"""Achieved HBM bandwidth of k_colwise_absmax (the statistic of --smooth) on one MI355X, beside k_minmax on the same tensors:
python scripts/smooth_bench.py [--rounds 7] [--calls 24]

Shapes: the LayerNorm output [64 * 197, 768] and the MLP input [64 * 197, 3072] of ViT-B/16 at batch 64 (38.7 MB, 154.9 MB).  Each
shape is held in several copies (more than the 256 MiB Infinity Cache together) and consecutive calls walk them in turn, so every
call reads from HBM.  A round times `calls` launches of dpl_colwise_absmax between two HIP events, then the same number of
k_minmax launches (CalibAccumulators.minmax_accumulate, plan built beforehand) between two more: the two kernels alternate, so a
drift of the machine hits both.  Bytes = 4 per element, one read; GB/s against the 8 TB/s HBM peak.  One JSON line per shape with
the median over the rounds and the spread (min .. max)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dipoorlet_amd import _hip, ops  # noqa: E402

PEAK = 8e12


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=24)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.lib()
    for rows, cols in ((64 * 197, 768), (64 * 197, 3072)):
        nbytes = 4 * rows * cols
        copies = max(2, -(-(320 << 20) // nbytes))
        xs = [torch.randn(rows, cols, device=dev) for _ in range(copies)]
        acc = torch.zeros(cols, device=dev)
        plan = ops.TensorSetPlan([rows * cols], 1, dev)
        mm = ops.CalibAccumulators(1, dev)
        stream = ops._stream()

        def colwise(i):
            x = xs[i % copies]
            _hip.check(lib.dpl_colwise_absmax(ops._ptr(x), rows, cols, ops._ptr(acc), stream), "dpl_colwise_absmax")

        def minmax(i):
            mm.minmax_accumulate(plan, [xs[i % copies]])

        for fn in (colwise, minmax):        # warm-up: code objects, the plan's work items and pointer tables for every copy
            timed(fn, 2 * copies)
        tc, tm = [], []
        for _ in range(a.rounds):
            tc.append(timed(colwise, a.calls))
            tm.append(timed(minmax, a.calls))
        ref = torch.stack(xs).abs().amax((0, 1))
        assert torch.equal(acc, ref), "k_colwise_absmax disagrees with torch"

        def row(ts):
            med = statistics.median(ts)
            return {"us": round(med * 1e6, 2), "GBps": round(nbytes / med / 1e9, 1), "of_8TBps": round(nbytes / med / PEAK, 3),
                    "GBps_min_max": [round(nbytes / max(ts) / 1e9, 1), round(nbytes / min(ts) / 1e9, 1)]}
        print(json.dumps({"shape": [rows, cols], "MB": round(nbytes / 1e6, 1), "copies": copies, "rounds": a.rounds, "calls": a.calls,
                          "k_colwise_absmax": row(tc), "k_minmax": row(tm)}), flush=True)


if __name__ == "__main__":
    main()
