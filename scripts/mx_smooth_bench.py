"""The fused candidate sweep of --smooth_search (dpl_mx_smooth_err, 12 candidates in one launch) beside the same sums composed
from the entry points there were before it — per candidate an fp32 division pass over X, an fp32 product pass over W, two
dpl_mx_encode launches and one dpl_mx_gemm_err —, on the two products a ViT-B LayerNorm site feeds at 16 images, both formats, HIP
events around each window.

scripts/mx_gemm_bench.py's method: the fp32 operands and the reference come from pools of more than 512 MB in all — twice the 256
MiB Infinity Cache — and every call takes the next member, so that no call finds its operands in a cache that the previous one
filled; a timed window is LAUNCHES calls in a row between two events; rounds alternate which of the two goes first.  Reported: time
per call (all 12 candidates), TFLOP/s on 2 * m * n * kp * n_cand, and the fused kernel's time over the composed path's.

    python scripts/mx_smooth_bench.py [--rounds 10] [--json out.json]
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

KERNELS = ("mx_smooth_err", "composed")
LAUNCHES = 2                    # per timed window
POOL_BYTES = 512 * 1024 * 1024  # over the three fp32 arrays of a pool member
N_CAND = 12
CASES = (("[16*197, 768] x [2304, 768]^T", 16 * 197, 2304, 768), ("[16*197, 768] x [3072, 768]^T", 16 * 197, 3072, 768))


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
        raise SystemExit("mx_smooth_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _hip.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    result = []
    for name, m, n, k in CASES:
        tiles = (-(-m // 64)) * (-(-n // 64))
        members = []
        for i in range(-(-POOL_BYTES // (4 * (m * k + n * k + m * n)))):
            x, w = torch.randn(m, k, device=dev), 0.05 * torch.randn(n, k, device=dev)
            x[:, (7 * i) % k] *= 50.0
            members.append((x, w, torch.matmul(x, w.t())))
        pool = Ring(members)
        s = (0.5 + torch.rand(N_CAND, k, device=dev)).contiguous()
        part = torch.empty(N_CAND, tiles, 2, dtype=torch.float64, device=dev)
        part_c = torch.empty_like(part)
        xs, ws = torch.empty(m, k, device=dev), torch.empty(n, k, device=dev)      # the composed path's four temporaries
        for elem in ("mxfp8", "mxfp4"):
            e = ops.MX_ELEM[elem]
            bytes_row = k * ops.MX_CODE_BITS[elem] // 8
            ac, asc = torch.empty(m, bytes_row, dtype=torch.uint8, device=dev), torch.empty(m, k // 32, dtype=torch.uint8, device=dev)
            bc, bsc = torch.empty(n, bytes_row, dtype=torch.uint8, device=dev), torch.empty(n, k // 32, dtype=torch.uint8, device=dev)

            def fused(e=e, out=part, m=m, n=n, k=k):
                x, w, ref = pool()
                _hip.check(lib.dpl_mx_smooth_err(e, p(x), p(w), p(s), N_CAND, m, n, k, p(ref), p(out), st), "dpl_mx_smooth_err")

            def composed(e=e, out=part_c, m=m, n=n, k=k):
                x, w, ref = pool()
                for c in range(N_CAND):
                    torch.div(x, s[c], out=xs)
                    torch.mul(w, s[c], out=ws)
                    _hip.check(lib.dpl_mx_encode(e, p(xs), m, k, 1, p(ac), p(asc), st), "dpl_mx_encode")
                    _hip.check(lib.dpl_mx_encode(e, p(ws), n, k, 1, p(bc), p(bsc), st), "dpl_mx_encode")
                    _hip.check(lib.dpl_mx_gemm_err(e, e, p(ac), p(asc), p(bc), p(bsc), 1, m, n, k, 0, p(ref), None, p(out[c]), st), "dpl_mx_gemm_err")
            fns = {"mx_smooth_err": fused, "composed": composed}
            # the two agree bit for bit on one member before anything is timed
            pool.k = -1
            fused()
            pool.k = -1
            composed()
            torch.cuda.synchronize()
            same = bool(torch.equal(part.view(torch.int64), part_c.view(torch.int64)))
            assert same, "the fused sums differ from the composed path's"
            for f in fns.values():
                f()
            torch.cuda.synchronize()

            def window(f):
                for _ in range(LAUNCHES):
                    f()
            ms = {kn: [] for kn in KERNELS}
            for r in range(a.rounds):
                for kn in (KERNELS if r % 2 == 0 else KERNELS[::-1]):      # alternate who goes first
                    ms[kn].append(timed(lambda: window(fns[kn])) / LAUNCHES)
            flop = 2.0 * m * n * k * N_CAND
            row = {"case": name, "elem": elem, "m": m, "n": n, "kp": k, "n_cand": N_CAND, "bit_identical": same}
            for kn in KERNELS:
                t = sorted(ms[kn])
                med = statistics.median(t)
                row[kn] = {"median_us": med * 1e3, "min_us": t[0] * 1e3, "max_us": t[-1] * 1e3, "median_tflops": flop / (med * 1e-3) / 1e12}
            row["fused_over_composed_time"] = row["mx_smooth_err"]["median_us"] / row["composed"]["median_us"]
            result.append(row)
            print(f"{name} {elem}: " + " | ".join(f"{kn} {row[kn]['median_us']:.0f} us [{row[kn]['min_us']:.0f} .. {row[kn]['max_us']:.0f}] "
                                                  f"{row[kn]['median_tflops']:.1f} TFLOP/s" for kn in KERNELS)
                  + f" | fused / composed time {row['fused_over_composed_time']:.3f}", flush=True)
        del pool, members
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "launches_per_window": LAUNCHES, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
