"""The block-scaled convolution of --mx_conv (dpl_mx_conv) beside what a checker would run without it — ops.mx_decode of both
operands plus torch's fp32 convolution — on ResNet-50 layer shapes at 64 images, all four element formats, HIP events around each
window.

scripts/mx_gemm_bench.py's method: every array a launch touches comes from a pool of more than 512 MB — twice the 256 MiB Infinity
Cache —, the code arrays and the fp32 outputs alike, and every launch takes the next member of each pool, so that no launch finds
its operands in a cache that the previous one filled; a timed window is LAUNCHES calls in a row between two events; rounds
alternate which of the two goes first.  Reported: time per call and TFLOP/s on 2 * n * oh * ow * cout * Kp (Kp = kh * kw * 32 *
ceil(c / 32): the padded channels are multiplied too), and the kernel's time over the yardstick's.

    python scripts/mx_conv_bench.py [--rounds 10] [--json out.json]
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

KERNELS = ("mx_conv", "decode_conv")
LAUNCHES = 4                    # per timed window
POOL_BYTES = 512 * 1024 * 1024  # per pool: twice the Infinity Cache
BATCH = 64
# (name, c, cout, k, stride, pad, image)
CASES = (("7x7 s2 3->64 @224", 3, 64, 7, 2, 3, 224), ("1x1 256->64 @56", 256, 64, 1, 1, 0, 56), ("3x3 64->64 @56", 64, 64, 3, 1, 1, 56),
         ("3x3 s2 128->128 @56", 128, 128, 3, 2, 1, 56), ("3x3 512->512 @7", 512, 512, 3, 1, 1, 7))


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
        raise SystemExit("mx_conv_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _hip.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    result = []
    for name, c, cout, k, stride, pad, img in CASES:
        n, h, w = BATCH, img, img
        oh = ow = (img + 2 * pad - k) // stride + 1
        cp = 32 * -(-c // 32)
        cs = Ring([torch.empty(n, oh, ow, cout, device=dev) for _ in range(-(-POOL_BYTES // (4 * n * oh * ow * cout)))])
        a_hat, b_hat = torch.empty(n, c, h, w, device=dev), torch.empty(cout, c, k, k, device=dev)      # its decoded operands
        for elem in ("mxfp8", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4"):
            e = ops.MX_ELEM[elem]
            bits = ops.MX_CODE_BITS[elem]
            x, wt = torch.randn(n, c, h, w, device=dev), torch.randn(cout, c, k, k, device=dev)

            def pool(t, nbytes):      # valid code arrays, each its own data
                out = []
                for i in range(-(-POOL_BYTES // nbytes)):
                    out.append(ops.mx_encode(t.roll(i, 0) if i else t, 1, elem))
                return Ring(out)
            fa, fb = pool(x, n * h * w * cp * bits // 8), pool(wt, cout * k * k * cp * bits // 8)
            del x, wt
            geo = (n, h, w, c, cout, k, k, stride, stride, pad, pad, 1, 1, oh, ow)

            def mx_conv(e=e, fa=fa, fb=fb, cs=cs, geo=geo):
                (ac, asc), (bc, bsc) = fa(), fb()
                _hip.check(lib.dpl_mx_conv(e, e, p(ac), p(asc), p(bc), p(bsc), *geo, p(cs()), st), "dpl_mx_conv")

            def decode_conv(elem=elem, fa=fa, fb=fb, shape_a=tuple(a_hat.shape), shape_b=tuple(b_hat.shape), stride=stride, pad=pad):
                (ac, asc), (bc, bsc) = fa(), fb()
                ops.mx_decode(ac, asc, elem, shape_a, 1, out=a_hat)
                ops.mx_decode(bc, bsc, elem, shape_b, 1, out=b_hat)
                torch.conv2d(a_hat, b_hat, None, stride, pad)      # (no out=: the allocator hands the same block out again)
            fns = {"mx_conv": mx_conv, "decode_conv": decode_conv}
            for f in fns.values():
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            # the two agree (to the instruction's truncation) before anything is timed
            (ac, asc), (bc, bsc) = fa.items[0], fb.items[0]
            got = ops.mx_conv(ac, asc, bc, bsc, elem, strides=(stride, stride), pads=(pad, pad), dilations=(1, 1), out_hw=(oh, ow))
            ops.mx_decode(ac, asc, elem, tuple(a_hat.shape), 1, out=a_hat)
            ops.mx_decode(bc, bsc, elem, tuple(b_hat.shape), 1, out=b_hat)
            want = torch.conv2d(a_hat, b_hat, None, stride, pad).permute(0, 2, 3, 1)
            rel = float((got - want).norm() / want.norm())
            assert rel < 1e-3, rel
            del got, want

            def window(f):
                for _ in range(LAUNCHES):
                    f()
            ms = {kn: [] for kn in KERNELS}
            for r in range(a.rounds):
                for kn in (KERNELS if r % 2 == 0 else KERNELS[::-1]):      # alternate who goes first
                    ms[kn].append(timed(lambda: window(fns[kn])) / LAUNCHES)
            kp = k * k * cp
            flop = 2.0 * n * oh * ow * cout * kp
            row = {"case": name, "elem": elem, "n": n, "c": c, "h": h, "w": w, "cout": cout, "kernel": k, "stride": stride, "pad": pad, "kp": kp,
                   "rel_diff": rel}
            for kn in KERNELS:
                t = sorted(ms[kn])
                med = statistics.median(t)
                row[kn] = {"median_us": med * 1e3, "min_us": t[0] * 1e3, "max_us": t[-1] * 1e3, "median_tflops": flop / (med * 1e-3) / 1e12}
            row["mx_conv_over_yardstick_time"] = row["mx_conv"]["median_us"] / row["decode_conv"]["median_us"]
            result.append(row)
            print(f"{name} {elem}: " + " | ".join(f"{kn} {row[kn]['median_us']:.0f} us [{row[kn]['min_us']:.0f} .. {row[kn]['max_us']:.0f}] "
                                                  f"{row[kn]['median_tflops']:.1f} TFLOP/s" for kn in KERNELS)
                  + f" | mx_conv / yardstick time {row['mx_conv_over_yardstick_time']:.3f} | relative difference {rel:.2e}", flush=True)
            del fa, fb, fns
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rounds": a.rounds, "launches_per_window": LAUNCHES, "batch": BATCH, "cases": result}, f, indent=1)


if __name__ == "__main__":
    main()
