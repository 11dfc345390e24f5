"""No GPU: csrc/mx_plan.hpp — the argument check, the launch plan and the dispatch the MX block kernels share (mx_kernels.hip,
mx_pack_kernels.hip, mx_search_kernels.hip), and those of the two kernels on the block-scaled MFMA (mx_gemm_kernels.hip,
mx_conv_kernels.hip) — compiled by the host compiler into a stand-alone program (tests/mx_plan_host.cpp, with the address and
undefined-behaviour sanitizers) and held, line by line, to the rules written out here: which launches run on 16-byte vectors, how
many column groups, groups or slots, tiles and workgroups they have, and what is refused with which words."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS_ITER, ROWS_BLOCK, COLS_BLOCK = 4, 256, 64          # groups per lane group; threads of a rows and of a cols workgroup
KS = (1, 4, 31, 32, 33, 36, 100, 768)
INNERS = (1, 2, 3, 4, 17, 64, 68)
OUTERS = (1, 3, 197)
BASES = (1 << 40, (1 << 40) + 4)                        # 16-byte aligned, and one float off
GRID_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("mxplan") / "mx_plan_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "mx_plan_host.cpp"), "-o", exe], check=True)

    def run(requests):
        r = subprocess.run([exe], input="".join(q + "\n" for q in requests), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(requests)
        return lines
    return run


def _plan(line):
    nums, _, msg = line.partition(" |")
    msg = msg.strip()
    rc, K, nblk, cs, vec, n, blocks = (int(v) for v in nums.split())
    return rc, K, nblk, cs, bool(vec), n, blocks, msg


def _want(fp, outer, k, inner, tiles):
    """The plan's rule, independently: (vec, cs, n, what the workgroup count must satisfy)."""
    nblk = -(-k // 32)
    aligned = fp % 16 == 0
    if inner == 1:
        vec = aligned and k % 4 == 0
        return nblk, vec, 1, outer * nblk, ROWS_ITER * ROWS_BLOCK * (4 if vec else 1) // 32
    vec = aligned and inner % 4 == 0
    cs = inner // 4 if vec else inner
    return nblk, vec, cs, outer * nblk * cs, None if (vec and tiles) else COLS_BLOCK


def test_plan_of_every_form(ask):
    cases = list(itertools.product(BASES, OUTERS, KS, INNERS, (0, 1)))
    seen = set()
    for (fp, outer, k, inner, tiles), line in zip(cases, ask([f"p {fp} {outer} {k} {inner} {tiles}" for fp, outer, k, inner, tiles in cases])):
        rc, K, nblk, cs, vec, n, blocks, msg = _plan(line)
        w_nblk, w_vec, w_cs, w_n, per_wg = _want(fp, outer, k, inner, tiles)
        what = (fp % 16, outer, k, inner, tiles, line)
        assert (rc, msg) == (0, ""), what
        assert (K, nblk, vec, cs, n) == (k, w_nblk, w_vec, w_cs, w_n), what
        if per_wg is None:                              # tiles of 4 K-blocks x 16 column groups
            assert blocks == outer * -(-nblk // 4) * -(-cs // 16), what
            assert blocks * 64 >= n, what               # a lane for every slot
        else:                                           # the rows and the slot grids: just enough workgroups
            assert blocks * per_wg >= n and (blocks - 1) * per_wg < n, what
        seen.add((inner == 1, vec, per_wg is None))
    assert seen == {(True, True, False), (True, False, False), (False, True, False), (False, True, True), (False, False, False)}


def test_plan_refuses_a_grid_above_2_31(ask):
    big = [(1 << 40, 2 ** 36, 32, 1, 0),                # 2^36 groups of 128 a workgroup: 2^29 workgroups
           (1 << 40, 2 ** 38, 32, 1, 0),                # 2^31 workgroups
           ((1 << 40) + 4, 2 ** 36, 32, 1, 1),          # 32 a workgroup: 2^31
           (1 << 40, 2 ** 31, 32, 64, 0),               # 2^35 slots: 2^29 workgroups
           (1 << 40, 2 ** 33, 32, 64, 0),               # 2^31
           (1 << 40, 2 ** 31, 32, 64, 1),               # 2^31 tiles
           (1 << 40, 2 ** 31 - 1, 32, 64, 1)]           # 2^31 - 1 tiles
    got = [_plan(line) for line in ask([f"p {fp} {outer} {k} {inner} {tiles}" for fp, outer, k, inner, tiles in big])]
    for (fp, outer, k, inner, tiles), (rc, _, _, _, _, n, blocks, msg) in zip(big, got):
        if blocks > GRID_MAX:
            assert rc == -2 and msg == "who: tensor too large", (outer, inner, tiles, rc, msg)
        else:
            assert rc == 0 and msg == "", (outer, inner, tiles, rc, msg)
    assert [g[6] > GRID_MAX for g in got] == [False, True, True, False, True, True, False]
    assert [g[6] for g in got] == [2 ** 29, 2 ** 31, 2 ** 31, 2 ** 29, 2 ** 31, 2 ** 31, 2 ** 31 - 1]


CHECKS = [  # elem, null pointers, outer, k, inner, padded, codes -> over, rc, the words of the message
    ((0, 0, 3, 100, 17, 0, 0), (0, 0, None)),
    ((1, 0, 3, 100, 17, 1, 1 << 20), (0, 0, None)),
    ((2, 0, 3, 100, 17, 0, 0), (1, -2, "elem must be DPL_MX_E4M3 or DPL_MX_E2M1")),
    ((-1 & 0xFFFFFFFF, 3, 0, 0, 0, 0, 8), (1, -2, "elem")),                 # elem comes first
    ((0, 3, 0, 100, 17, 0, 8), (1, 0, None)),                               # a zero size: nothing to do, whatever the pointers
    ((0, 3, 3, 0, 17, 1, 8), (1, 0, None)),
    ((1, 3, 3, 100, 0, 1, 8), (1, 0, None)),
    ((0, 1, 3, 100, 17, 0, 0), (1, -2, "a, b and c must not be null")),
    ((0, 2, 3, 100, 17, 0, 0), (1, -2, "null")),
    ((0, 3, 3, 2 ** 31, 17, 0, 0), (1, -2, "null")),                        # null before the ranges
    ((0, 0, 3, 2 ** 31, 17, 0, 0), (1, -2, "k and inner must be in [1, 2^31)")),
    ((0, 0, 3, 17, 2 ** 31, 0, 0), (1, -2, "2^31")),
    ((0, 0, 2, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0), (0, 0, None)),              # the largest k and inner: below 2^63 elements
    ((0, 0, 2 ** 58, 1, 1, 0, 0), (0, 0, None)),                            # 2^58 elements
    ((0, 0, 2 ** 58, 1, 1, 1, 0), (1, -2, "tensor too large")),             # padded to 32 along K: 2^63 elements, one too many
    ((0, 0, 2 ** 58, 33, 1, 0, 0), (1, -2, "tensor too large")),            # 33 * 2^58 > 2^63 - 1
    ((0, 0, 2 ** 58, 31, 1, 0, 0), (0, 0, None)),                           # 31 * 2^58 fits, padded to 32 * 2^58 = 2^63 it does not
    ((0, 0, 2 ** 58, 31, 1, 1, 0), (1, -2, "too large")),
    ((0, 0, 2 ** 58 - 1, 31, 1, 1, 0), (0, 0, None)),
    ((0, 0, 3, 100, 17, 1, (1 << 20) + 8), (1, -2, "d_codes must be 16-byte aligned")),
    ((0, 0, 2 ** 58, 31, 1, 1, 8), (1, -2, "too large")),                   # the size before the alignment
]


def test_check_order_codes_and_words(ask):
    for (args, (over, rc, words)), line in zip(CHECKS, ask(["c " + " ".join(str(a) for a in args) for args, _ in CHECKS])):
        nums, _, msg = line.partition(" |")
        assert [int(v) for v in nums.split()] == [over, rc], (args, line)
        if words is None:
            assert msg.strip() == "", (args, line)
        else:
            assert msg.startswith(" who: ") and words in msg, (args, line)


def test_dispatch_reaches_each_instantiation_once(ask):
    combos = list(itertools.product((0, 1), (0, 1), (0, 1)))
    got = [int(v) for v in ask([f"d {e} {r} {v}" for e, r, v in combos])]
    assert got == [100 * e + 10 * r + (4 if v else 1) for e, r, v in combos] and len(set(got)) == 8


# ------------------------------------------------------------------- the two kernels on the block-scaled MFMA (dpl_mx_gemm, dpl_mx_conv)
# The argument cases of test_refusals_launch_nothing in test_mx_gemm_gpu.py and test_mx_conv_gpu.py, held here without a GPU: the
# return code and the words of every refusal, in the order the entry points make them.
TILE = 64
BASE = 1 << 40                                          # a 16-byte aligned address; the scales and C are always valid or null
TOP = 2 ** 31 - 1
ELEM_WORDS = "elem_a and elem_b must be DPL_MX_E4M3 or DPL_MX_E2M1"
NULL_WORDS = "the codes, the scales and d_c must not be null"
ALIGN_WORDS = "d_a_codes and d_b_codes must be 16-byte aligned (a block's codes are loaded as 16-byte vectors)"
A_CODES, A_SCALES, B_CODES, B_SCALES, C_OUT = (1 << i for i in range(5))      # the <null> bits
ALL_NULL = 31


def _answers(ask, letter, cases):
    """-> per case (the numbers of the answer, its message); every refusal is rc -2 with the entry point's name in front."""
    out = []
    for args, line in zip(cases, ask([letter + " " + " ".join(str(a) for a in args) for args in cases])):
        nums, _, msg = line.partition(" |")
        out.append(([int(v) for v in nums.split()], msg.strip()))
    return out


def _held(who, cases, got):
    for (args, (over, rc, words)), (nums, msg) in zip(cases, got):
        assert nums[:2] == [over, rc], (args, nums, msg)
        if words is None:
            assert msg == "", (args, msg)
        else:
            assert rc == -2 and msg.startswith(who + ": ") and words in msg, (args, msg)


def _gemm(ea=0, eb=0, null=0, a=BASE, b=BASE, batch=1, m=8, n=6, k=64):
    return (ea, eb, null, a, b, batch, m, n, k)


GEMM_CHECKS = [
    (_gemm(), (0, 0, None)),
    (_gemm(1, 1, batch=3, m=130, n=65, k=100), (0, 0, None)),
    (_gemm(ea=2), (1, -2, ELEM_WORDS)), (_gemm(eb=-1), (1, -2, ELEM_WORDS)),
    (_gemm(ea=2, null=ALL_NULL, batch=0, m=1 << 31), (1, -2, "elem")),                       # elem comes first
    *[(_gemm(1, 1, ALL_NULL, 0, 0, **{z: 0}), (1, 0, None)) for z in ("batch", "m", "n", "k")],      # a zero size: 0 whatever the pointers
    (_gemm(null=ALL_NULL, m=1 << 31, k=0), (1, 0, None)),
    *[(_gemm(null=bit), (1, -2, NULL_WORDS)) for bit in (A_CODES, A_SCALES, B_CODES, B_SCALES, C_OUT)],
    (_gemm(null=C_OUT, m=1 << 31), (1, -2, "null")),                                         # null before the ranges
    (_gemm(m=1 << 31), (1, -2, "m, n and k must be in [1, 2^31)")), (_gemm(n=1 << 31), (1, -2, "2^31")), (_gemm(k=1 << 31), (1, -2, "2^31")),
    (_gemm(m=TOP, n=64, k=TOP), (0, 0, None)), (_gemm(m=65, n=TOP, k=TOP), (0, 0, None)),     # the largest m, n and k
    (_gemm(batch=1 << 40, m=1 << 20, k=1 << 20), (1, -2, "tensor too large")),               # the padded operand's codes
    (_gemm(batch=1 << 40, m=1 << 12, n=1 << 12, k=32), (1, -2, "tensor too large")),         # C's elements
    (_gemm(batch=1 << 40, m=1 << 20, k=1 << 20, a=BASE + 8), (1, -2, "too large")),          # the size before the alignment
    (_gemm(batch=1 << 30, m=1 << 10, n=1 << 10, k=32), (1, -2, "tensor too large")),         # the grid: 2^38 workgroups
    (_gemm(batch=1 << 30, m=1 << 10, n=1 << 10, k=32, b=BASE + 8), (1, -2, "16-byte aligned")),      # the alignment before the grid
    *[(_gemm(a=BASE + shift), (1, -2, ALIGN_WORDS)) for shift in (1, 4, 8)],
    *[(_gemm(b=BASE + shift, m=6, n=8), (1, -2, ALIGN_WORDS)) for shift in (1, 4, 8)],
    (_gemm(a=BASE + 16, b=BASE + 48), (0, 0, None)),                                         # and on a boundary it runs
]


def test_gemm_check_order_codes_and_words(ask):
    cases = [c for c, _ in GEMM_CHECKS]
    got = _answers(ask, "g", cases)
    _held("dpl_mx_gemm", GEMM_CHECKS, got)
    for args, (nums, _) in zip(cases, got):
        if nums[:2] == [0, 0]:                           # a call that goes on to launch: its grid
            batch, m, n = args[5:8]
            assert nums[2:] == [-(-m // TILE), -(-n // TILE), batch * -(-m // TILE) * -(-n // TILE)], (args, nums)


CONV_NAMES = ["n", "h", "w", "c", "cout", "kh", "kw", "sh", "sw", "pt", "pl", "dh", "dw", "oh", "ow"]
CONV_OK = [1, 4, 4, 64, 6, 3, 3, 1, 1, 1, 1, 1, 1, 4, 4]


def _conv(ea=0, eb=0, null=0, a=BASE, b=BASE, **change):
    dims = list(CONV_OK)
    for k, v in change.items():
        dims[CONV_NAMES.index(k)] = v
    return (ea, eb, null, a, b, *dims)


CONV_CHECKS = [
    (_conv(), (0, 0, None)),
    (_conv(1, 1, n=3, c=100, cout=130, oh=13, ow=5), (0, 0, None)),
    (_conv(ea=2), (1, -2, ELEM_WORDS)), (_conv(eb=-1), (1, -2, ELEM_WORDS)),
    (_conv(ea=2, null=ALL_NULL, n=0, kh=0, pt=-1), (1, -2, "elem")),                          # elem comes first
    *[(_conv(null=bit), (1, -2, NULL_WORDS)) for bit in (A_CODES, A_SCALES, B_CODES, B_SCALES, C_OUT)],
    *[(_conv(**{k: v}), (1, -2, "kh, kw, the strides and the dilations must be at least 1")) for k in ("kh", "kw", "sh", "sw", "dh", "dw") for v in (0, -1)],
    (_conv(kh=0, pt=-1, n=1 << 31), (1, -2, "at least 1")),                                   # before the pads and the ranges
    *[(_conv(**{k: -1}), (1, -2, "pad_top and pad_left must not be negative")) for k in ("pt", "pl")],
    (_conv(pt=-1, n=1 << 31), (1, -2, "negative")),
    *[(_conv(**{k: 1 << 31}), (1, -2, "every dimension, stride, pad and dilation must be in [0, 2^31)")) for k in CONV_NAMES],
    *[(_conv(**{k: -1}), (1, -2, "2^31")) for k in ("n", "h", "w", "c", "cout", "oh", "ow")],
    (_conv(null=ALL_NULL, n=0, h=1 << 31), (1, -2, "2^31")),                                  # the ranges before a zero size
    (_conv(null=A_CODES, kh=TOP, kw=TOP), (1, -2, "null")),                                   # null before the products
    (_conv(kh=TOP, kw=TOP), (1, -2, "tensor too large")),                                     # the K-blocks of a weight row
    (_conv(oh=TOP, ow=TOP), (1, -2, "tensor too large")),                                     # the output pixels of an image
    (_conv(n=TOP, h=TOP, w=TOP, c=TOP), (1, -2, "tensor too large")),                         # A's bytes
    (_conv(cout=TOP, kh=1 << 20, kw=1 << 10, c=TOP), (1, -2, "tensor too large")),            # kh * kw fits, times Cb it does not
    (_conv(cout=TOP, kh=1 << 15, kw=1 << 15, c=32), (1, -2, "tensor too large")),             # B's bytes
    (_conv(n=TOP, oh=1 << 15, ow=1 << 15, cout=TOP), (1, -2, "tensor too large")),            # C's bytes
    (_conv(n=1 << 20, oh=1 << 10, ow=1 << 10), (1, -2, "tensor too large (the grid)")),
    (_conv(n=1 << 20, oh=1 << 10, ow=1 << 10, a=BASE + 8), (1, -2, "the grid")),              # the grid before the alignment
    *[(_conv(1, 1, ALL_NULL, 0, 0, **{k: 0}), (1, 0, None)) for k in ("n", "h", "w", "c", "cout", "oh", "ow")],   # a zero size: 0 whatever the pointers
    *[(_conv(a=BASE + shift), (1, -2, ALIGN_WORDS)) for shift in (1, 4, 8)],
    *[(_conv(b=BASE + shift), (1, -2, ALIGN_WORDS)) for shift in (1, 4, 8)],
    (_conv(a=BASE + 16), (0, 0, None)),                                                       # and on a boundary it runs
]


def test_conv_check_order_codes_and_words(ask):
    cases = [c for c, _ in CONV_CHECKS]
    got = _answers(ask, "v", cases)
    _held("dpl_mx_conv", CONV_CHECKS, got)
    for (args, (_, _, words)), (nums, msg) in zip(CONV_CHECKS, got):
        if words == "tensor too large":                  # the five products, not the grid's refusal
            assert msg == "dpl_mx_conv: tensor too large", (args, msg)
        if nums[:2] == [0, 0]:                           # a call that goes on to launch: what the kernel is given
            d = dict(zip(CONV_NAMES, args[5:]))
            cb, m = -(-d["c"] // 32), d["oh"] * d["ow"]
            tiles = [-(-m // TILE), -(-d["cout"] // TILE)]
            assert nums[2:] == [cb, d["kh"] * d["kw"] * cb, m, *tiles, d["n"] * tiles[0] * tiles[1]], (args, nums)


def test_tile_grid(ask):
    cases = list(itertools.product((1, 3), (1, 63, 64, 65, 130), (1, 63, 64, 65, 130)))
    for (batch, m, n), (nums, msg) in zip(cases, _answers(ask, "t", cases)):
        tiles_m, tiles_n = -(-m // 64), -(-n // 64)
        assert (nums, msg) == ([0, tiles_m, tiles_n, tiles_m * tiles_n * batch], ""), (batch, m, n, nums, msg)
    # the refusal above 2^31 - 1 workgroups: per batch, and over the batches
    edge = [(1, 64 * 2 ** 15, 64 * 2 ** 16 - 64), (1, 64 * 2 ** 15, 64 * 2 ** 16), (TOP, 64, 1), (1 << 31, 1, 64), (2 ** 20, 64 * 2 ** 11, 1),
            (1 << 62, 1, 1), (1, TOP, TOP)]
    got = _answers(ask, "t", edge)
    for (batch, m, n), (nums, msg) in zip(edge, got):
        blocks = batch * -(-m // 64) * -(-n // 64)
        if blocks > GRID_MAX:
            assert (nums[0], nums[3], msg) == (-2, 0, "who: tensor too large"), (batch, m, n, nums, msg)
        else:
            assert (nums[0], nums[3], msg) == (0, blocks, ""), (batch, m, n, nums, msg)
    assert [nums[0] for nums, _ in got] == [0, -2, 0, -2, -2, -2, -2]


def test_pair_dispatch_reaches_each_instantiation_once(ask):
    combos = list(itertools.product((0, 1), (0, 1)))
    got = [int(v) for v in ask([f"e {ea} {eb}" for ea, eb in combos])]
    assert got == [10 * ea + eb for ea, eb in combos] and len(set(got)) == 4
