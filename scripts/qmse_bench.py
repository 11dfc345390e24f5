#!/usr/bin/env python3
"""GPU time of the quantisation-MSE clip search (dpl_hist_qmse: k_hist_qmse + k_hist_kl_pick, on the integer grid and on E4M3)
beside the entropy search (dpl_hist_kl) and the percentile search (dpl_hist_percentile) on one MI355X, by HIP events around
alternating launches in one process:  python scripts/qmse_bench.py [--rounds 200] [--model-slots 123]

Histograms: 2048 bins over synthetic ResNet-50-shaped activations (123 tensors, one batch of 8 images); the 557-slot set (a
ViT-B/16's tensor count) repeats those 123 rows.  One JSON line per slot count."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dipoorlet_amd import ops  # noqa: E402
from dipoorlet_amd.synthetic import resnet50_tensors, synth_activations  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=200)
ap.add_argument("--model-slots", type=int, default=123, help="histograms the numpy model is timed on and compared with (0: skip)")
ap.add_argument("--bins", type=int, default=2048)
ap.add_argument("--first", type=int, default=128)
a = ap.parse_args()
dev = torch.device("cuda:0")
BINS, F, B = a.bins, a.first, 8
GRIDS = (("uniform", "Linear"), ("e4m3", "Float8E4M3FN"))

spec = resnet50_tensors()
plan = ops.TensorSetPlan([e for _, e, _ in spec], B, dev)
tensors = synth_activations(spec, B, dev, seed=1)
base = ops.CalibAccumulators(len(spec), dev, BINS)
base.minmax_accumulate(plan, tensors)
base.finalize_minmax()
base.hist_prepare()
base.abs_hist_accumulate(plan, tensors)
torch.cuda.synchronize()
del tensors

model_s_per_slot = {}
if a.model_slots:
    import qmse_model
    h = base.hist.cpu().numpy()
    lo, hi = base.gmin.cpu().numpy(), base.gmax.cpu().numpy()
    n = min(a.model_slots, len(spec))
    for key, qtype in GRIDS:
        grid, top = qmse_model.grid_of(qtype, 8)
        t0 = time.perf_counter()
        want = [qmse_model.qmse_clip(h[t], lo[t], hi[t], F, grid, top) for t in range(n)]
        model_s = time.perf_counter() - t0
        model_s_per_slot[key] = model_s / n
        got_clip, got_best, _ = (x.cpu().numpy() for x in base.hist_qmse(qtype, 8, F))
        agree = sum(int(got_best[t] == want[t][1] and np.array_equal(got_clip[t], want[t][0])) for t in range(n))
        print(json.dumps({"grid": key, "model_slots": n, "model_wall_s": round(model_s, 3), "kernel_equals_model_on": agree,
                          "median_best": float(np.median(got_best[:n]))}), flush=True)


def _stat(us):
    return {"median": round(float(np.median(us)), 1), "min": round(float(us.min()), 1), "max": round(float(us.max()), 1)}


for slots in (len(spec), 557):
    acc = ops.CalibAccumulators(slots, dev, BINS)
    idx = torch.arange(slots, device=dev) % len(spec)
    acc.set_minmax(base.gmin[idx], base.gmax[idx])
    acc.hist_prepare()
    acc.hist.copy_(base.hist[idx])
    calls = ([lambda q=q: acc.hist_qmse(q, 8, F) for _, q in GRIDS] + [lambda: acc.hist_kl(F), lambda: acc.hist_percentile(0.99999)])
    for _ in range(5):
        for c in calls:
            c()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)] for _ in range(a.rounds)]
    for row in ev:
        row[0].record()
        for k, c in enumerate(calls):
            c()
            row[k + 1].record()
    torch.cuda.synchronize()
    us = [np.array([row[k].elapsed_time(row[k + 1]) for row in ev]) * 1e3 for k in range(len(calls))]
    pairs = slots * (BINS - F + 1) * BINS                      # (candidate, bin) pairs: every candidate meets every bin
    live = int((acc.hist != 0).sum().item()) * (BINS - F + 1)  # ... of them with a non-zero count
    print(json.dumps({
        "slots": slots, "bins": BINS, "first": F, "rounds": a.rounds,
        "hist_qmse_uniform_us_per_launch": _stat(us[0]), "hist_qmse_e4m3_us_per_launch": _stat(us[1]),
        "hist_kl_us_per_launch": _stat(us[2]), "hist_percentile_us_per_launch": _stat(us[3]),
        "candidate_bin_pairs_per_launch": pairs, "pairs_with_a_count_per_launch": live,
        "host_model_wall_s": {k: round(v * slots, 2) for k, v in model_s_per_slot.items()} or None,
        "host_model_note": "numpy model (exact-integer statement), one thread; measured per slot on the 123 distinct histograms, "
                           "times the slot count"}), flush=True)
