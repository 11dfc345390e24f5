"""The element-code kernels of --mx_pack (dpl_mx_encode, dpl_mx_decode) beside the MX Q/DQ kernel (dpl_fake_quant_mx) on the same
tensors, all four element formats, HIP events around each window.

scripts/mx_bench.py's method and tensors: every array a launch touches comes from a pool of more than 512 MB — twice the 256 MiB
Infinity Cache —, the fp32 tensors and the (four or eight times smaller, so that many more) code arrays alike, and every launch
takes the next member of each pool, so that no launch finds its data in a cache; a timed window is LAUNCHES launches in a row
between two events; rounds rotate which kernel goes first.  Encode and decode move fewer bytes than the Q/DQ kernel's 8 B per
element — 4 + 1 + 1/32 (E4M3), 4 + 0.75 + 1/32 (the two FP6) or 4 + 0.5 + 1/32 (E2M1) —, so GB/s on their own bytes says how well they stream, and the yardstick
is the Q/DQ kernel's time per launch on the same tensor in the same run: all three are printed.

    python scripts/mx_pack_bench.py [--rounds 12] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dipoorlet_amd import _hip, ops  # noqa: E402

PEAK_GBS = 8000.0
KERNELS = ("qdq", "encode", "decode")
LAUNCHES = 16                  # per timed window
POOL_BYTES = 512 * 1024 * 1024  # per pool: twice the Infinity Cache


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)      # ms


class Ring:
    def __init__(self, items):
        self.items, self.k = items, 0

    def __call__(self):
        self.k = (self.k + 1) % len(self.items)
        return self.items[self.k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_pack_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _hip.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    cases = []      # (name, elem, {kernel: bytes moved per launch}, {kernel: callable()})
    for name, shape, axis in (("contiguous [64*197, 768]", (64 * 197, 768), -1), ("contiguous [64*197, 3072]", (64 * 197, 3072), -1),
                              ("strided [64*12, 64, 197] axis -2", (64 * 12, 64, 197), -2),
                              ("strided x4 [16, 3072, 768] axis -2", (16, 3072, 768), -2)):
        ax = axis % len(shape)
        outer = inner = 1
        for d in shape[:ax]:
            outer *= d
        for d in shape[ax + 1:]:
            inner *= d
        k, n = shape[ax], outer * shape[ax] * inner
        pool = -(-POOL_BYTES // (4 * n))
        xs = [torch.randn(shape, device=dev) for _ in range(pool)]
        ys = [torch.empty_like(xs[0]) for _ in range(pool)]
        fx, fy = Ring(xs), Ring(ys)
        for elem in ("mxfp8", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4"):
            e = ops.MX_ELEM[elem]
            cs, ss = ops.mx_packed_shapes(shape, axis, elem)
            nc, ns = 1, 1
            for d in cs:
                nc *= d
            for d in ss:
                ns *= d
            packed = [ops.mx_encode(xs[i % pool], axis, elem) for i in range(-(-POOL_BYTES // nc))]      # every code array is valid
            fc = Ring(packed)

            def qdq(e=e, outer=outer, k=k, inner=inner, fx=fx, fy=fy):
                _hip.check(lib.dpl_fake_quant_mx(e, p(fx()), p(fy()), outer, k, inner, None, st), "dpl_fake_quant_mx")

            def encode(e=e, outer=outer, k=k, inner=inner, fx=fx, fc=fc):
                c, s = fc()
                _hip.check(lib.dpl_mx_encode(e, p(fx()), outer, k, inner, p(c), p(s), st), "dpl_mx_encode")

            def decode(e=e, outer=outer, k=k, inner=inner, fy=fy, fc=fc):
                c, s = fc()
                _hip.check(lib.dpl_mx_decode(e, p(c), p(s), outer, k, inner, p(fy()), st), "dpl_mx_decode")
            cases.append((name, elem, {"qdq": 8 * n, "encode": 4 * n + nc + ns, "decode": 4 * n + nc + ns},
                          {"qdq": qdq, "encode": encode, "decode": decode}))
    for _, _, _, fns in cases:     # warm every shape of every kernel
        for f in fns.values():
            for _ in range(3):
                f()
    torch.cuda.synchronize()

    def window(f):
        for _ in range(LAUNCHES):
            f()
    ms = {(name, elem, kn): [] for name, elem, _, fns in cases for kn in fns}
    for r in range(a.rounds):
        order = KERNELS[r % 3:] + KERNELS[:r % 3]      # rotate who goes first
        for name, elem, _, fns in cases:
            for kn in order:
                ms[(name, elem, kn)].append(timed(lambda: window(fns[kn])) / LAUNCHES)
    result = []
    for name, elem, nbytes, _ in cases:
        row = {"case": name, "elem": elem}
        for kn in KERNELS:
            t = sorted(ms[(name, elem, kn)])
            med = statistics.median(t)
            row[kn] = {"bytes": nbytes[kn], "median_us": med * 1e3, "min_us": t[0] * 1e3, "max_us": t[-1] * 1e3,
                       "median_gbs": nbytes[kn] / (med * 1e-3) / 1e9, "median_of_peak": nbytes[kn] / (med * 1e-3) / 1e9 / PEAK_GBS}
        for kn in KERNELS[1:]:
            row[kn + "_over_qdq_time"] = row[kn]["median_us"] / row["qdq"]["median_us"]
        result.append(row)
        print(f"{name} {elem}: " + " | ".join(f"{kn} {row[kn]['median_us']:.1f} us [{row[kn]['min_us']:.1f} .. {row[kn]['max_us']:.1f}] "
                                              f"{row[kn]['median_gbs']:.0f} GB/s = {row[kn]['median_of_peak']:.3f} of 8 TB/s" for kn in KERNELS)
              + f" | time / qdq: encode {row['encode_over_qdq_time']:.3f}, decode {row['decode_over_qdq_time']:.3f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "launches_per_window": LAUNCHES, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
