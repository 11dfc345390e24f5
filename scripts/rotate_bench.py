"""The block-Hadamard kernel of --mx_rotate (dpl_hadamard32) beside the MX Q/DQ kernel (dpl_fake_quant_mx, contiguous path, both
element formats) on the same tensors, HIP events around each window.

Both read 4 B and write 4 B per element and use the same layout (8 lanes of 16 bytes per block of 32), so the yardstick of the
rotation is the MX rows kernel on the same tensors in this very run.  The method is scripts/mx_bench.py's: a case holds a pool of
input and output buffers of more than 512 MB each way — twice the 256 MiB Infinity Cache —, every launch of every kernel takes the
next pair of the pool, a timed window is LAUNCHES launches in a row between two events, and rounds rotate which kernel goes first.
Cases: the MatMul inputs of a ViT-B/16 forward at batch 64, [64 * 197, 768] and [64 * 197, 3072].

    python scripts/rotate_bench.py [--rounds 12] [--json out.json]
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
KERNELS = ("mxfp8", "mxfp4", "hadamard32")
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
        raise SystemExit("rotate_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    cases = []      # (name, bytes moved per launch, {kernel: callable()})
    for name, shape in (("contiguous [64*197, 768]", (64 * 197, 768)), ("contiguous [64*197, 3072]", (64 * 197, 3072))):
        n = shape[0] * shape[1]
        pool = -(-POOL_BYTES // (4 * n))
        xs = [torch.randn(shape, device=dev) for _ in range(pool)]
        ys = [torch.empty_like(xs[0]) for _ in range(pool)]
        turn = [0]

        def nxt(xs=xs, ys=ys, turn=turn):
            k = turn[0] = (turn[0] + 1) % len(xs)
            return xs[k], ys[k]

        def had(nxt=nxt):
            x, y = nxt()
            ops.hadamard32(x, out=y)
        fns = {"hadamard32": had}
        for elem in ("mxfp8", "mxfp4"):
            def mx(nxt=nxt, elem=elem):
                x, y = nxt()
                ops.fake_quant_mx(x, -1, elem, out=y)
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
        order = KERNELS[r % 3:] + KERNELS[:r % 3]      # rotate who goes first
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
        for k in KERNELS[:2]:
            row["hadamard32_over_" + k + "_median"] = row["hadamard32"]["median_gbs"] / row[k]["median_gbs"]
        result.append(row)
        print(f"{name}: " + " | ".join(f"{k} {row[k]['median_gbs']:.0f} GB/s [{row[k]['min_gbs']:.0f} .. {row[k]['max_gbs']:.0f}] = "
                                       f"{row[k]['median_of_peak']:.3f} of 8 TB/s" for k in KERNELS)
              + f" | hadamard32 / mxfp8 {row['hadamard32_over_mxfp8_median']:.3f}, hadamard32 / mxfp4 {row['hadamard32_over_mxfp4_median']:.3f}",
              flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "launches_per_window": LAUNCHES, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
