"""No GPU: csrc/mx_plan.hpp's mx_gemm_err_check — dpl_mx_gemm_err's argument rules — compiled by the host compiler into a stand-alone
program (tests/mx_mixed_host.cpp, with the address and undefined-behaviour sanitizers) and held to the rules written out here: the
return code, the words and the ORDER of every refusal (elem, a zero size, null pointers, ranges, "tensor too large", the codes'
alignment, the grid), and the grid of a call that goes on to launch."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WHO = "dpl_mx_gemm_err"
TILE = 64
BASE = 1 << 40                                          # a 16-byte aligned address
TOP = 2 ** 31 - 1
ELEM_WORDS = "elem_a and elem_b must be DPL_MX_E4M3 or DPL_MX_E2M1"
NULL_WORDS = "the codes, the scales, d_ref and d_part must not be null"
RANGE_WORDS = "m, n and k must be in [1, 2^31)"
ALIGN_WORDS = "d_a_codes and d_b_codes must be 16-byte aligned (a block's codes are loaded as 16-byte vectors)"
A_CODES, A_SCALES, B_CODES, B_SCALES, REF, PART = (1 << i for i in range(6))      # the <null> bits
ALL_NULL = 63


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("mxmixed") / "mx_mixed_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "mx_mixed_host.cpp"), "-o", exe], check=True)

    def run(cases):
        r = subprocess.run([exe], input="".join("r " + " ".join(str(a) for a in c) + "\n" for c in cases), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for line in lines:
            nums, _, msg = line.partition(" |")
            out.append(([int(v) for v in nums.split()], msg.strip()))
        return out
    return run


def _err(ea=0, eb=0, null=0, a=BASE, b=BASE, batch=1, m=8, n=6, k=64):
    return (ea, eb, null, a, b, batch, m, n, k)


CHECKS = [  # -> over, rc, the words of the message
    (_err(), (0, 0, None)),
    (_err(1, 1, batch=3, m=130, n=65, k=100), (0, 0, None)),
    (_err(0, 1), (0, 0, None)), (_err(1, 0), (0, 0, None)),
    (_err(ea=2), (1, -2, ELEM_WORDS)), (_err(eb=-1), (1, -2, ELEM_WORDS)),
    (_err(ea=2, null=ALL_NULL, batch=0, m=1 << 31), (1, -2, "elem")),                        # elem comes first
    *[(_err(1, 1, ALL_NULL, 0, 0, **{z: 0}), (1, 0, None)) for z in ("batch", "m", "n", "k")],      # a zero size: 0 whatever the pointers
    (_err(null=ALL_NULL, m=1 << 31, k=0), (1, 0, None)),                                     # ... before the ranges too
    *[(_err(null=bit), (1, -2, NULL_WORDS)) for bit in (A_CODES, A_SCALES, B_CODES, B_SCALES, REF, PART)],
    (_err(null=REF, m=1 << 31), (1, -2, "null")), (_err(null=PART, k=1 << 31), (1, -2, "null")),      # null before the ranges
    (_err(m=1 << 31), (1, -2, RANGE_WORDS)), (_err(n=1 << 31), (1, -2, RANGE_WORDS)), (_err(k=1 << 31), (1, -2, RANGE_WORDS)),
    (_err(m=1 << 31, batch=1 << 40, k=1 << 20), (1, -2, "2^31")),                            # the ranges before the size
    (_err(m=TOP, n=64, k=TOP), (0, 0, None)), (_err(m=65, n=TOP, k=TOP), (0, 0, None)),       # the largest m, n and k
    (_err(batch=1 << 40, m=1 << 20, k=1 << 20), (1, -2, "tensor too large")),                # the padded operand's codes
    (_err(batch=1 << 40, m=1 << 12, n=1 << 12, k=32), (1, -2, "tensor too large")),          # the reference's elements
    (_err(batch=1 << 40, m=1 << 20, k=1 << 20, a=BASE + 8), (1, -2, "too large")),           # the size before the alignment
    (_err(batch=1 << 30, m=1 << 10, n=1 << 10, k=32), (1, -2, "tensor too large")),          # the grid: 2^38 workgroups
    (_err(batch=1 << 30, m=1 << 10, n=1 << 10, k=32, b=BASE + 8), (1, -2, "16-byte aligned")),       # the alignment before the grid
    *[(_err(a=BASE + shift), (1, -2, ALIGN_WORDS)) for shift in (1, 4, 8)],
    *[(_err(b=BASE + shift, m=6, n=8), (1, -2, ALIGN_WORDS)) for shift in (1, 4, 8)],
    (_err(a=BASE + 16, b=BASE + 48), (0, 0, None)),                                          # and on a boundary it runs
]


def test_gemm_err_check_order_codes_and_words(ask):
    got = ask([c for c, _ in CHECKS])
    for (args, (over, rc, words)), (nums, msg) in zip(CHECKS, got):
        assert nums[:2] == [over, rc], (args, nums, msg)
        if words is None:
            assert msg == "", (args, msg)
        else:
            assert rc == -2 and msg.startswith(WHO + ": ") and words in msg, (args, msg)
        if nums[:2] == [0, 0]:                           # a call that goes on to launch: its grid, two doubles of d_part a workgroup
            batch, m, n = args[5:8]
            assert nums[2:] == [-(-m // TILE), -(-n // TILE), batch * -(-m // TILE) * -(-n // TILE)], (args, nums)
        else:
            assert nums[4] == 0, (args, nums)           # no grid is handed to a launch


def test_the_grid_stays_below_2_31(ask):
    edge = [_err(batch=TOP, m=64, n=64, k=32), _err(batch=1 << 31, m=64, n=64, k=32), _err(batch=1, m=64 * 2 ** 15, n=64 * 2 ** 16 - 64, k=32),
            _err(batch=1, m=64 * 2 ** 15, n=64 * 2 ** 16, k=32)]
    got = ask(edge)
    assert [nums[:2] for nums, _ in got] == [[0, 0], [1, -2], [0, 0], [1, -2]]
    assert got[0][0][4] == TOP and got[2][0][4] == 2 ** 31 - 2 ** 15 and all("tensor too large" in got[i][1] for i in (1, 3))
