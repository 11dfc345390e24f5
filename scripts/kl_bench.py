#!/usr/bin/env python3
"""GPU time of the entropy clip search (dpl_hist_kl: k_hist_kl + k_hist_kl_pick) beside the percentile search
(dpl_hist_percentile) on one MI355X, by HIP events around alternating launches, and the host model's wall time for the
same histograms:  python scripts/kl_bench.py [--rounds 200] [--model-slots 123]

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
ap.add_argument("--model-slots", type=int, default=123, help="histograms the fp64 numpy model is timed on (0: skip)")
ap.add_argument("--bins", type=int, default=2048)
ap.add_argument("--levels", type=int, default=128)
a = ap.parse_args()
dev = torch.device("cuda:0")
BINS, L, B = a.bins, a.levels, 8

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

model_s_per_slot = None
if a.model_slots:
    import kl_model
    h = base.hist.cpu().numpy()
    lo, hi = base.gmin.cpu().numpy(), base.gmax.cpu().numpy()
    n = min(a.model_slots, len(spec))
    t0 = time.perf_counter()
    want = [kl_model.kl_clip(h[t], lo[t], hi[t], L) for t in range(n)]
    model_s = time.perf_counter() - t0
    model_s_per_slot = model_s / n
    got_clip, got_best, _ = (x.cpu().numpy() for x in base.hist_kl(L))
    agree = sum(int(got_best[t] == want[t][1] and np.array_equal(got_clip[t], want[t][0])) for t in range(n))
    print(json.dumps({"model_slots": n, "model_wall_s": round(model_s, 3), "kernel_equals_model_on": agree}), flush=True)

for slots in (len(spec), 557):
    acc = ops.CalibAccumulators(slots, dev, BINS)
    idx = torch.arange(slots, device=dev) % len(spec)
    acc.set_minmax(base.gmin[idx], base.gmax[idx])
    acc.hist_prepare()
    acc.hist.copy_(base.hist[idx])
    for _ in range(5):
        acc.hist_kl(L)
        acc.hist_percentile(0.99999)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.rounds)]
    for e0, e1, e2 in ev:
        e0.record()
        acc.hist_kl(L)
        e1.record()
        acc.hist_percentile(0.99999)
        e2.record()
    torch.cuda.synchronize()
    kl = np.array([e0.elapsed_time(e1) for e0, e1, _ in ev]) * 1e3
    pc = np.array([e1.elapsed_time(e2) for _, e1, e2 in ev]) * 1e3
    terms = slots * (BINS * (BINS + 1) - L * (L - 1)) // 2        # (candidate, bin) pairs: sum of i over i in [levels, bins]
    live = int((torch.cumsum((acc.hist != 0).to(torch.int64), 1)[:, L - 1:]).sum().item())   # ... of them with a non-zero count
    print(json.dumps({
        "slots": slots, "bins": BINS, "levels": L, "rounds": a.rounds,
        "hist_kl_us_per_launch": {"median": round(float(np.median(kl)), 1), "min": round(float(kl.min()), 1), "max": round(float(kl.max()), 1)},
        "hist_percentile_us_per_launch": {"median": round(float(np.median(pc)), 1), "min": round(float(pc.min()), 1), "max": round(float(pc.max()), 1)},
        "candidate_bin_pairs_per_launch": terms, "pairs_with_a_count_per_launch": live,
        # per pair with a count: 2 subtractions, 4 divisions, 1 logarithm, 1 product, 1 addition — each counted as one operation
        "fp64_ops_per_launch": 9 * live,
        "host_model_wall_s": None if model_s_per_slot is None else round(model_s_per_slot * slots, 2),
        "host_model_note": "fp64 numpy model, one thread; measured per slot on the 123 distinct histograms, times the slot count"}), flush=True)
