"""The block-scaled product of --mx_verify (dpl_mx_gemm) beside what a checker would run without it — ops.mx_decode of both
operands plus torch.matmul in fp32 — on the two large products of a ViT-B MLP at 64 images, all four element formats, HIP events
around each window.

scripts/mx_bench.py's method: every array a launch touches comes from a pool of more than 512 MB — twice the 256 MiB Infinity
Cache —, the code arrays and the fp32 outputs alike, and every launch takes the next member of each pool, so that no launch finds
its operands in a cache that the previous one filled; a timed window is LAUNCHES calls in a row between two events; rounds
alternate which of the two goes first.  Reported: time per call and TFLOP/s on 2 * M * N * Kp, and the kernel's time over the
yardstick's.

    python scripts/mx_gemm_bench.py [--rounds 10] [--json out.json]
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

KERNELS = ("mx_gemm", "decode_matmul")
LAUNCHES = 4                    # per timed window
POOL_BYTES = 512 * 1024 * 1024  # per pool: twice the Infinity Cache
CASES = (("[64*197, 768] x [3072, 768]^T", 64 * 197, 3072, 768), ("[64*197, 3072] x [768, 3072]^T", 64 * 197, 768, 3072))


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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_gemm_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _hip.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    result = []
    for name, m, n, k in CASES:
        cs = Ring([torch.empty(m, n, device=dev) for _ in range(-(-POOL_BYTES // (4 * m * n)))])
        a_hat, b_hat = torch.empty(m, k, device=dev), torch.empty(n, k, device=dev)      # the yardstick's decoded operands
        for elem in ("mxfp8", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4"):
            e = ops.MX_ELEM[elem]
            bits = ops.MX_CODE_BITS[elem]
            x, w = torch.randn(m, k, device=dev), torch.randn(n, k, device=dev)

            def pool(t, rows):      # valid code arrays, each its own data
                out = []
                for i in range(-(-POOL_BYTES // (rows * k * bits // 8))):
                    out.append(ops.mx_encode(t.roll(i, 0) if i else t, -1, elem))
                return Ring(out)
            fa, fb = pool(x, m), pool(w, n)
            del x, w

            def mx_gemm(e=e, fa=fa, fb=fb, cs=cs, m=m, n=n, k=k):
                (ac, asc), (bc, bsc) = fa(), fb()
                _hip.check(lib.dpl_mx_gemm(e, e, p(ac), p(asc), p(bc), p(bsc), 1, m, n, k, 0, p(cs()), st), "dpl_mx_gemm")

            def decode_matmul(elem=elem, fa=fa, fb=fb, cs=cs, m=m, n=n, k=k):
                (ac, asc), (bc, bsc) = fa(), fb()
                ops.mx_decode(ac, asc, elem, (m, k), -1, out=a_hat)
                ops.mx_decode(bc, bsc, elem, (n, k), -1, out=b_hat)
                torch.matmul(a_hat, b_hat.t(), out=cs())
            fns = {"mx_gemm": mx_gemm, "decode_matmul": decode_matmul}
            for f in fns.values():
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            # the two agree (to the instruction's truncation) before anything is timed
            (ac, asc), (bc, bsc) = fa.items[0], fb.items[0]
            got = ops.mx_gemm(ac, asc, bc, bsc, elem)
            ops.mx_decode(ac, asc, elem, (m, k), -1, out=a_hat)
            ops.mx_decode(bc, bsc, elem, (n, k), -1, out=b_hat)
            want = torch.matmul(a_hat, b_hat.t())
            rel = float((got - want).norm() / want.norm())
            assert rel < 1e-3, rel

            def window(f):
                for _ in range(LAUNCHES):
                    f()
            ms = {kn: [] for kn in KERNELS}
            for r in range(a.rounds):
                for kn in (KERNELS if r % 2 == 0 else KERNELS[::-1]):      # alternate who goes first
                    ms[kn].append(timed(lambda: window(fns[kn])) / LAUNCHES)
            flop = 2.0 * m * n * k
            row = {"case": name, "elem": elem, "m": m, "n": n, "kp": k, "rel_diff": rel}
            for kn in KERNELS:
                t = sorted(ms[kn])
                med = statistics.median(t)
                row[kn] = {"median_us": med * 1e3, "min_us": t[0] * 1e3, "max_us": t[-1] * 1e3, "median_tflops": flop / (med * 1e-3) / 1e12}
            row["mx_gemm_over_yardstick_time"] = row["mx_gemm"]["median_us"] / row["decode_matmul"]["median_us"]
            result.append(row)
            print(f"{name} {elem}: " + " | ".join(f"{kn} {row[kn]['median_us']:.0f} us [{row[kn]['min_us']:.0f} .. {row[kn]['max_us']:.0f}] "
                                                  f"{row[kn]['median_tflops']:.1f} TFLOP/s" for kn in KERNELS)
                  + f" | mx_gemm / yardstick time {row['mx_gemm_over_yardstick_time']:.3f} | relative difference {rel:.2e}", flush=True)
            del fa, fb, fns
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "launches_per_window": LAUNCHES, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
