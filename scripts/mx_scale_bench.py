"""The scale search of `--mx_scale_search` (dpl_mx_scale_search, both element formats, with and without its error output) beside
the MX Q/DQ kernel (dpl_fake_quant_mx) on the same tensors, HIP events around each window — scripts/mx_bench.py's method.

The search reads 4 B per element and writes one byte per block of 32 (and 16 B of fp64 errors per block when asked); the Q/DQ
kernel reads 4 B and writes 4 B per element.  Each is reported as time per launch and as GB/s on the bytes it moves itself.  A case
holds a pool of inputs of more than 512 MB — twice the 256 MiB Infinity Cache —, every launch takes the next tensor of the pool, a
timed window is LAUNCHES launches in a row between two events, and rounds rotate which kernel goes first.  Cases: the weight stack
of mx_bench.py, [16, 3072, 768] blocked along axis -2 (strided, four columns per lane) — what the pass is for: it runs once per
quant_graph over the constant operands only —, and that script's two ViT-B/16 activations, [64 * 197, 768] and [64 * 197, 3072]
(blocks contiguous), for the contiguous form.

    python scripts/mx_scale_bench.py [--rounds 12] [--json out.json]
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
LAUNCHES = 16                  # per timed window
POOL_BYTES = 512 * 1024 * 1024  # of inputs per case: twice the Infinity Cache


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
        raise SystemExit("mx_scale_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    cases = []      # (name, {kernel: (bytes moved per launch, callable())})
    for name, shape, axis in (("strided x4 [16, 3072, 768] axis -2", (16, 3072, 768), -2),
                              ("contiguous [64*197, 768]", (64 * 197, 768), -1), ("contiguous [64*197, 3072]", (64 * 197, 3072), -1)):
        n = 1
        for d in shape:
            n *= d
        nblocks = n // shape[axis] * -(-shape[axis] // ops.MX_BLOCK)
        pool = -(-POOL_BYTES // (4 * n))
        xs = [torch.randn(shape, device=dev) for _ in range(pool)]
        y = torch.empty_like(xs[0])
        err = torch.empty(nblocks * 2, dtype=torch.float64, device=dev)
        turn = [0]

        def nxt(xs=xs, turn=turn):
            k = turn[0] = (turn[0] + 1) % len(xs)
            return xs[k]
        fns = {}
        for elem in ("mxfp8", "mxfp4"):
            fns["qdq " + elem] = (8 * n, lambda nxt=nxt, axis=axis, elem=elem, y=y: ops.fake_quant_mx(nxt(), axis, elem, out=y))
            fns["search " + elem] = (4 * n + nblocks, lambda nxt=nxt, axis=axis, elem=elem: ops.mx_scale_search(nxt(), axis, elem))
            fns["search+err " + elem] = (4 * n + 17 * nblocks,
                                         lambda nxt=nxt, axis=axis, elem=elem, err=err: ops.mx_scale_search(nxt(), axis, elem, err=err))
        cases.append((name, fns))
    for _, fns in cases:     # warm every shape of every kernel
        for _, f in fns.values():
            for _ in range(3):
                f()
    torch.cuda.synchronize()

    def window(f):
        for _ in range(LAUNCHES):
            f()
    ms = {(name, k): [] for name, fns in cases for k in fns}
    for r in range(a.rounds):
        for name, fns in cases:
            keys = list(fns)
            for k in keys[r % len(keys):] + keys[:r % len(keys)]:      # rotate who goes first
                ms[(name, k)].append(timed(lambda: window(fns[k][1])) / LAUNCHES)
    result = []
    for name, fns in cases:
        row = {"case": name}
        for k, (nbytes, _) in fns.items():
            t = sorted(ms[(name, k)])
            med = statistics.median(t)
            row[k] = {"bytes": nbytes, "median_us": med * 1e3, "min_us": t[0] * 1e3, "max_us": t[-1] * 1e3,
                      "median_gbs": nbytes / (med * 1e-3) / 1e9, "median_of_peak": nbytes / (med * 1e-3) / 1e9 / PEAK_GBS}
            print(f"{name}: {k}: {row[k]['median_us']:.1f} us [{row[k]['min_us']:.1f} .. {row[k]['max_us']:.1f}] per launch, "
                  f"{row[k]['median_gbs']:.0f} GB/s on {nbytes} B = {row[k]['median_of_peak']:.3f} of 8 TB/s", flush=True)
        result.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "launches_per_window": LAUNCHES, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
