"""No GPU: the two MXFP6 formats on the host — csrc/mx_format.hpp's arithmetic under the records Fmt<DPL_MX_E2M3> and
Fmt<DPL_MX_E3M2>, and csrc/mx_plan.hpp's checks and dispatches over all four formats, compiled into a stand-alone program
(tests/mx_fp6_host.cpp, with the address and undefined-behaviour sanitizers) and held to tests/mx_fp6_model.py on the same inputs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mx_fp6_model as F

HERE = os.path.dirname(os.path.abspath(__file__))
CODE = {"mxfp6_e2m3": 6, "mxfp6_e3m2": 7}


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("mxfp6") / "mx_fp6_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "mx_fp6_host.cpp"), "-o", exe], check=True)

    def run(requests):
        r = subprocess.run([exe], input="".join(q + "\n" for q in requests), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(requests)
        return lines
    return run


def _inputs(elem):
    """|v| patterns and shared exponents: the boundary points scaled into every se, random patterns, fp32 subnormals."""
    rng = np.random.default_rng(CODE[elem])
    pts = np.abs(F.boundary_points(elem)).astype(np.float64)
    ses = [-127, -126, -100, -3, 0, 1, 5, 100, 127 - F.EMAX[elem]]
    v, s = [], []
    for se in ses:
        with np.errstate(over="ignore"):
            scaled = np.ldexp(pts, se).astype(np.float32)                       # (rounds only where fp32 cannot hold it: still an input)
            extra = np.ldexp(rng.uniform(0, 2.0 * F.ELEM_MAX[elem], 300), se).astype(np.float32)
        scaled = scaled[np.isfinite(scaled)]
        allv = np.concatenate([scaled, extra[np.isfinite(extra)]])
        v.append(allv)
        s.append(np.full(allv.size, se))
    rnd = rng.integers(0, 0x7F800000, 2000, dtype=np.uint32).view(np.float32)
    v.append(rnd)
    s.append(rng.integers(-127, 128 - F.EMAX[elem], rnd.size))
    return np.concatenate(v).astype(np.float32), np.concatenate(s).astype(np.int64)


@pytest.mark.parametrize("elem", F.ELEMS)
def test_rounding_and_codes_against_the_model(ask, elem):
    v, se = _inputs(elem)
    got = np.array([[int(t) for t in line.split()] for line in ask([f"r {CODE[elem]} {int(b)} {int(e) + 127}" for b, e in zip(v.view(np.uint32), se)])],
                   np.int64)
    want = (F.round_elem(v.astype(np.float64) / np.ldexp(1.0, se), elem) * np.ldexp(1.0, se)).astype(np.float32)
    assert np.array_equal(got[:, 0].astype(np.uint32), want.view(np.uint32))
    c = F.codes(elem).astype(np.float64)
    idx = np.searchsorted(c, np.abs(F.round_elem(v.astype(np.float64) / np.ldexp(1.0, se), elem)))
    assert np.array_equal(got[:, 1], idx) and np.array_equal(got[:, 2], idx)    # round_code == encode_bits(round_bits) == the model's
    assert np.array_equal(got[:, 3], got[:, 0])                                  # decode_bits(round_code) is round_bits
    assert (idx == 31).any() and (idx == 0).any() and len(set(idx.tolist())) == 32


@pytest.mark.parametrize("elem", F.ELEMS)
def test_every_code_round_trips_and_decodes_as_the_model(ask, elem):
    bytes_ = (0, 1, 127, 254 - F.EMAX[elem])
    req = [(c, s) for c in range(64) for s in bytes_]
    got = np.array([[int(t) for t in line.split()] for line in ask([f"x {CODE[elem]} {c} {s}" for c, s in req])], np.int64)
    want = F.decode_elements(np.array([c for c, _ in req], np.uint8), np.array([s for _, s in req], np.uint8), elem)
    assert np.array_equal(got[:, 0].astype(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, 1], [c for c, _ in req])


@pytest.mark.parametrize("elem", F.ELEMS)
def test_shared_exponent(ask, elem):
    a = np.array([2.0 ** k for k in range(-149, 128, 7)] + [np.nextafter(np.float32(2.0 ** k), np.float32(0)) for k in range(-140, 128, 9)]
                 + [1e-45, 3.4e38, 7.5, 28.0, 1.0], np.float32)
    got = [int(line) for line in ask([f"s {CODE[elem]} {int(b)}" for b in a.view(np.uint32)])]
    assert got == F.shared_exponent(a, elem).tolist() and min(got) == -127


def test_the_records(ask):
    assert ask(["t 6", "t 7"]) == ["6 0 2", "6 0 3"]


def test_dispatch_reaches_each_instantiation_once(ask):
    cases = [(e, r, v) for e in (0, 1, 6, 7) for r in (0, 1) for v in (0, 1)]
    got = [int(line) for line in ask([f"d {e} {r} {v}" for e, r, v in cases])]
    assert got == [100 * e + 10 * r + (4 if v else 1) for e, r, v in cases] and len(set(got)) == 16
    pairs = [(a, b) for a in (0, 1, 6, 7) for b in (0, 1, 6, 7)]
    got = [int(line) for line in ask([f"e {a} {b}" for a, b in pairs])]
    assert got == [10 * a + b for a, b in pairs] and len(set(got)) == 16


def test_checks_accept_6_and_7_and_refuse_2_5_8(ask):
    words = "elem must be DPL_MX_E4M3 or DPL_MX_E2M1"
    for e in (0, 1, 6, 7):
        assert ask([f"c {e}"]) == ["0 0 | "]
    for e in (2, 5, 8, -1 % 2 ** 64):
        (line,) = ask([f"c {e}"])
        assert line.startswith("1 -2 | who: " + words) and "DPL_MX_E2M3 / DPL_MX_E3M2" in line
    pair_words = "elem_a and elem_b must be DPL_MX_E4M3 or DPL_MX_E2M1"
    for kind, who in (("g", "dpl_mx_gemm"), ("v", "dpl_mx_conv")):
        for a in (0, 1, 6, 7):
            for b in (0, 1, 6, 7):
                assert ask([f"{kind} {a} {b}"]) == ["0 0 | "], (kind, a, b)
        for a, b in ((2, 6), (7, 5), (8, 0), (6, 8)):
            (line,) = ask([f"{kind} {a} {b}"])
            assert line.startswith(f"1 -2 | {who}: {pair_words}") and "DPL_MX_E2M3 / DPL_MX_E3M2" in line
    # dpl_mx_gemm_err serves --mx_mixed only: its two formats, and it says so for an FP6 code
    for a in (0, 1):
        for b in (0, 1):
            assert ask([f"m {a} {b}"]) == ["0 0 | "]
    for a, b in ((6, 0), (1, 7), (6, 7), (2, 0)):
        (line,) = ask([f"m {a} {b}"])
        assert line.startswith(f"1 -2 | dpl_mx_gemm_err: {pair_words}") and "no FP6 format" in line
