"""No GPU: csrc/mx_plan.hpp — the argument check, the launch plan and the dispatch the MX block kernels share (mx_kernels.hip,
mx_pack_kernels.hip, mx_search_kernels.hip) — compiled by the host compiler into a stand-alone program (tests/mx_plan_host.cpp, with
the address and undefined-behaviour sanitizers) and held, line by line, to the rules written out here: which launches run on 16-byte
vectors, how many column groups, groups or slots and workgroups they have, and what is refused with which words."""
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
