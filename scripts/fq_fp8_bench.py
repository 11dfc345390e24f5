"""The FP8 Q/DQ kernel (dpl_fake_quant_fp8) beside the integer one (dpl_fake_quant) on the same tensors, HIP events around each.

Both kernels read 4 B and write 4 B per element, so the yardstick of the FP8 kernel is the integer kernel in this very run:
rounds of the two alternate in one process, each round times every case once per kernel, and the figure to read is whether the
FP8 kernel's median sits inside the round-to-round spread (min .. max) of the integer kernel's.  Cases: one activation of a
ResNet-50 forward at batch 64 per tensor and per channel (51 MB and 205 MB), and ResNet-50's whole tensor set at batch 4 in one
launch (the set forms).  Inputs rotate over distinct buffers so that no round finds its tensor in the cache.

    python scripts/fq_fp8_bench.py [--rounds 12] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dipoorlet_amd import ops  # noqa: E402
from dipoorlet_amd.synthetic import resnet50_tensor_elems, resnet50_tensor_shapes, synth_activations  # noqa: E402

PEAK_GBS = 8000.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)      # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fq_fp8_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    cases = []      # (name, bytes moved, {kernel: callable(round)})
    for shape in [(64, 256, 28, 28), (64, 256, 56, 56)]:
        xs = [torch.randn(shape, device=dev) for _ in range(3)]
        y = torch.empty_like(xs[0])
        c = shape[1]
        s1, z1 = torch.full((1,), 0.05, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        sc, zc = torch.full((c,), 0.05, device=dev) * torch.linspace(0.5, 2, c, device=dev), torch.zeros(c, dtype=torch.int32, device=dev)
        mb = 4 * xs[0].numel() / 1e6
        cases.append((f"{mb:.0f} MB per tensor", 8 * xs[0].numel(),
                      {"int8": lambda r, xs=xs, y=y, s1=s1, z1=z1: ops.fake_quant(xs[r % 3], s1, z1, -128, 127, out=y),
                       "fp8": lambda r, xs=xs, y=y, s1=s1: ops.fake_quant_fp8(xs[r % 3], s1, out=y)}))
        cases.append((f"{mb:.0f} MB per channel", 8 * xs[0].numel(),
                      {"int8": lambda r, xs=xs, y=y, sc=sc, zc=zc: ops.fake_quant(xs[r % 3], sc, zc, -128, 127, axis=1, out=y),
                       "fp8": lambda r, xs=xs, y=y, sc=sc: ops.fake_quant_fp8(xs[r % 3], sc, axis=1, out=y)}))
    elems, shapes, batch = resnet50_tensor_elems(), resnet50_tensor_shapes(), 4
    sets = [synth_activations(elems, batch, dev, seed=7 + k) for k in range(2)]
    outs = [torch.empty_like(x) for x in sets[0]]
    plan = ops.TensorSetPlan(elems, batch, dev)
    rows_i, rows_f = [], []
    for t, (ch, h, w) in enumerate(shapes):      # every other tensor per channel, as a graph mixes weights' and activations' rows
        n = ch if t % 2 else 1
        s = torch.full((n,), 0.05, device=dev)
        rows_i.append((s, torch.zeros(n, dtype=torch.int32, device=dev), h * w, -128, 127))
        rows_f.append((s, h * w))
    fq_i, fq_f = ops.FakeQuantSet(plan, rows_i), ops.FakeQuantSet(plan, rows_f, fmt="fp8")
    cases.append((f"ResNet-50 set, batch {batch}, one launch", 8 * batch * sum(elems),
                  {"int8": lambda r: fq_i(sets[r % 2], out=outs), "fp8": lambda r: fq_f(sets[r % 2], out=outs)}))
    for _, _, fns in cases:     # warm every shape of both kernels
        for f in fns.values():
            for r in range(3):
                f(r)
    torch.cuda.synchronize()
    ms = {(name, k): [] for name, _, fns in cases for k in fns}
    for r in range(a.rounds):
        for name, _, fns in cases:
            for k in (("int8", "fp8") if r % 2 == 0 else ("fp8", "int8")):      # alternate who goes first
                ms[(name, k)].append(timed(lambda: fns[k](r)))
    result = []
    for name, nbytes, _ in cases:
        row = {"case": name, "bytes": nbytes}
        for k in ("int8", "fp8"):
            gbs = sorted(nbytes / (t * 1e-3) / 1e9 for t in ms[(name, k)])
            row[k] = {"median_gbs": statistics.median(gbs), "min_gbs": gbs[0], "max_gbs": gbs[-1],
                      "median_of_peak": statistics.median(gbs) / PEAK_GBS}
        row["fp8_median_not_below_int8_spread"] = row["fp8"]["median_gbs"] >= row["int8"]["min_gbs"]
        row["fp8_over_int8_median"] = row["fp8"]["median_gbs"] / row["int8"]["median_gbs"]
        result.append(row)
        print(f"{name}: int8 {row['int8']['median_gbs']:.0f} GB/s [{row['int8']['min_gbs']:.0f} .. {row['int8']['max_gbs']:.0f}] = "
              f"{row['int8']['median_of_peak']:.3f} of 8 TB/s | fp8 {row['fp8']['median_gbs']:.0f} GB/s [{row['fp8']['min_gbs']:.0f} .. "
              f"{row['fp8']['max_gbs']:.0f}] = {row['fp8']['median_of_peak']:.3f} | fp8 / int8 {row['fp8_over_int8_median']:.3f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
