"""The fused error reduction of --mx_mixed (dpl_mx_gemm_err) beside dpl_mx_gemm alone and beside what a run without it would do —
dpl_mx_gemm, then torch's ((c - ref)^2).sum() and (ref^2).sum(): three passes over M * N * 4 bytes — on the two large products of a
ViT-B MLP at 64 images, both element formats, HIP events around each window.

scripts/mx_gemm_bench.py's method: every array a launch touches comes from a pool of more than 512 MB — twice the 256 MiB Infinity
Cache —, the code arrays, the fp32 references and outputs alike, and every launch takes the next member of each pool, so that no
launch finds its operands in a cache that the previous one filled; a timed window is LAUNCHES calls in a row between two events;
rounds rotate which of the three goes first.  Reported: time per call, and the fused kernel's time over dpl_mx_gemm's (expected: at
most 1.15) and over the three-pass path's.

    python scripts/mx_mixed_bench.py [--rounds 10] [--json out.json]
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

KERNELS = ("mx_gemm_err", "mx_gemm", "mx_gemm_then_torch")
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
        raise SystemExit("mx_mixed_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _hip.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    result = []
    for name, m, n, k in CASES:
        members = -(-POOL_BYTES // (4 * m * n))
        cs = Ring([torch.empty(m, n, device=dev) for _ in range(members)])
        x, w = torch.randn(m, k, device=dev), torch.randn(n, k, device=dev)
        exact = torch.matmul(x, w.t())
        refs = Ring([exact.clone() for _ in range(members)])
        del exact
        tiles = -(-m // 64) * -(-n // 64)
        part = torch.empty(tiles, 2, dtype=torch.float64, device=dev)
        for elem in ("mxfp8", "mxfp4"):
            e = ops.MX_ELEM[elem]
            per = 2 if elem == "mxfp4" else 1

            def pool(t, rows):      # valid code arrays, each its own data
                out = []
                for i in range(-(-POOL_BYTES // (rows * k // per))):
                    out.append(ops.mx_encode(t.roll(i, 0) if i else t, -1, elem))
                return Ring(out)
            fa, fb = pool(x, m), pool(w, n)

            def mx_gemm_err(e=e, fa=fa, fb=fb, m=m, n=n, k=k):
                (ac, asc), (bc, bsc) = fa(), fb()
                _hip.check(lib.dpl_mx_gemm_err(e, e, p(ac), p(asc), p(bc), p(bsc), 1, m, n, k, 0, p(refs()), None, p(part), st), "dpl_mx_gemm_err")

            def mx_gemm(e=e, fa=fa, fb=fb, m=m, n=n, k=k):
                (ac, asc), (bc, bsc) = fa(), fb()
                _hip.check(lib.dpl_mx_gemm(e, e, p(ac), p(asc), p(bc), p(bsc), 1, m, n, k, 0, p(cs()), st), "dpl_mx_gemm")

            def mx_gemm_then_torch(e=e, fa=fa, fb=fb, m=m, n=n, k=k):
                (ac, asc), (bc, bsc) = fa(), fb()
                c, ref = cs(), refs()
                _hip.check(lib.dpl_mx_gemm(e, e, p(ac), p(asc), p(bc), p(bsc), 1, m, n, k, 0, p(c), st), "dpl_mx_gemm")
                return ((c - ref) ** 2).sum(dtype=torch.float64), (ref ** 2).sum(dtype=torch.float64)
            fns = {"mx_gemm_err": mx_gemm_err, "mx_gemm": mx_gemm, "mx_gemm_then_torch": mx_gemm_then_torch}
            for f in fns.values():
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            # the two ways agree on the node's relative error before anything is timed (item 0 of the code pools is x and w themselves)
            (ac, asc), (bc, bsc) = fa.items[0], fb.items[0]
            got = ops.mx_gemm_err(ac, asc, bc, bsc, refs.items[0], elem).sum(dim=(0, 1))
            c = ops.mx_gemm(ac, asc, bc, bsc, elem)
            want = torch.stack([((c - refs.items[0]).double() ** 2).sum(), (refs.items[0].double() ** 2).sum()])
            rel = float(((got - want).abs() / want).max())
            assert rel < 1e-9, rel
            err = float(got[0] / got[1])
            del c

            def window(f):
                for _ in range(LAUNCHES):
                    f()
            ms = {kn: [] for kn in KERNELS}
            for r in range(a.rounds):
                order = KERNELS[r % 3:] + KERNELS[:r % 3]                  # rotate who goes first
                for kn in (order if (r // 3) % 2 == 0 else order[::-1]):
                    ms[kn].append(timed(lambda: window(fns[kn])) / LAUNCHES)
            row = {"case": name, "elem": elem, "m": m, "n": n, "kp": k, "relative_error_of_the_product": err, "rel_diff_of_the_sums": rel}
            for kn in KERNELS:
                t = sorted(ms[kn])
                med = statistics.median(t)
                row[kn] = {"median_us": med * 1e3, "min_us": t[0] * 1e3, "max_us": t[-1] * 1e3}
            row["err_over_mx_gemm_time"] = row["mx_gemm_err"]["median_us"] / row["mx_gemm"]["median_us"]
            row["err_over_three_pass_time"] = row["mx_gemm_err"]["median_us"] / row["mx_gemm_then_torch"]["median_us"]
            result.append(row)
            print(f"{name} {elem}: " + " | ".join(f"{kn} {row[kn]['median_us']:.0f} us [{row[kn]['min_us']:.0f} .. {row[kn]['max_us']:.0f}]"
                                                  for kn in KERNELS)
                  + f" | err / mx_gemm {row['err_over_mx_gemm_time']:.3f} | err / three-pass {row['err_over_three_pass_time']:.3f}"
                  + f" | e = {err:.3e}", flush=True)
            del fa, fb, fns
        del cs, refs, x, w
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "launches_per_window": LAUNCHES, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
