"""The MX Q/DQ kernel (dpl_fake_quant_mx, all four element formats, both paths) beside the static FP8 one (dpl_fake_quant_fp8) on the
same tensors, HIP events around each window.

All three read 4 B and write 4 B per element, so the yardstick of the MX kernel is the FP8 kernel on the same tensors in this
very run.  A case holds a pool of input and output buffers of more than 512 MB each way — twice the 256 MiB Infinity Cache —, and
every launch of every kernel takes the next pair of the pool, so that no launch finds its tensor in a cache; a timed window is
LAUNCHES launches in a row between two events; rounds rotate which kernel goes first.  Cases: the MatMul inputs of a ViT-B/16
forward at batch 64, [64 * 197, 768] and [64 * 197, 3072] (blocks contiguous), the attention operand [64 * 12, 64, 197] blocked
along axis -2 (blocks strided, one column per lane), and a [16, 3072, 768] weight stack blocked along axis -2 (strided, four
columns per lane).

    python scripts/mx_bench.py [--rounds 12] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dipoorlet_amd import ops  # noqa: E402

PEAK_GBS = 8000.0
KERNELS = ("fp8", "mxfp8", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4")
LAUNCHES = 16                  # per timed window
POOL_BYTES = 512 * 1024 * 1024  # of inputs (and as much of outputs) per case: twice the Infinity Cache


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
        raise SystemExit("mx_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    cases = []      # (name, bytes moved per launch, {kernel: callable()})
    s1 = torch.full((1,), 0.05, device=dev)
    for name, shape, axis in (("contiguous [64*197, 768]", (64 * 197, 768), -1), ("contiguous [64*197, 3072]", (64 * 197, 3072), -1),
                              ("strided [64*12, 64, 197] axis -2", (64 * 12, 64, 197), -2),
                              ("strided x4 [16, 3072, 768] axis -2", (16, 3072, 768), -2)):
        n = 1
        for d in shape:
            n *= d
        pool = -(-POOL_BYTES // (4 * n))
        xs = [torch.randn(shape, device=dev) for _ in range(pool)]
        ys = [torch.empty_like(xs[0]) for _ in range(pool)]
        turn = [0]

        def nxt(xs=xs, ys=ys, turn=turn):
            k = turn[0] = (turn[0] + 1) % len(xs)
            return xs[k], ys[k]

        def fp8(nxt=nxt):
            x, y = nxt()
            ops.fake_quant_fp8(x, s1, out=y)
        fns = {"fp8": fp8}
        for elem in KERNELS[1:]:
            def mx(nxt=nxt, axis=axis, elem=elem):
                x, y = nxt()
                ops.fake_quant_mx(x, axis, elem, out=y)
            fns[elem] = mx
        cases.append((name, 8 * n, fns))
    for _, _, fns in cases:     # warm every shape of every kernel
        for f in fns.values():
            for _ in range(3):
                f()
    torch.cuda.synchronize()

    def window(f):
        for _ in range(LAUNCHES):
            f()
    ms = {(name, k): [] for name, _, fns in cases for k in fns}
    for r in range(a.rounds):
        order = KERNELS[r % len(KERNELS):] + KERNELS[:r % len(KERNELS)]      # rotate who goes first
        for name, _, fns in cases:
            for k in order:
                ms[(name, k)].append(timed(lambda: window(fns[k])) / LAUNCHES)
    result = []
    for name, nbytes, _ in cases:
        row = {"case": name, "bytes": nbytes}
        for k in KERNELS:
            gbs = sorted(nbytes / (t * 1e-3) / 1e9 for t in ms[(name, k)])
            row[k] = {"median_gbs": statistics.median(gbs), "min_gbs": gbs[0], "max_gbs": gbs[-1],
                      "median_of_peak": statistics.median(gbs) / PEAK_GBS}
        for k in KERNELS[1:]:
            row[k + "_over_fp8_median"] = row[k]["median_gbs"] / row["fp8"]["median_gbs"]
        result.append(row)
        print(f"{name}: " + " | ".join(f"{k} {row[k]['median_gbs']:.0f} GB/s [{row[k]['min_gbs']:.0f} .. {row[k]['max_gbs']:.0f}] = "
                                       f"{row[k]['median_of_peak']:.3f} of 8 TB/s" for k in KERNELS)
              + " | " + ", ".join(f"{k} / fp8 {row[k + '_over_fp8_median']:.3f}" for k in KERNELS[1:]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "launches_per_window": LAUNCHES, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
