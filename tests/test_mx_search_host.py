"""No GPU: csrc/mx_search.hpp — the per-block arithmetic of --mx_scale_search (the two roundings, the squared difference built from
bit patterns, the balanced tree, the choice) — compiled for the host into a stand-alone program (tests/mx_search_host.cpp, with the
address and undefined-behaviour sanitizers) and held to tests/mx_scale_model.py, bytes and fp64 errors bit for bit, on the block zoo
of tests/test_mx_format_host.py: random bit patterns, a few-binade spread, every code, tie and neighbour under the nine exponents,
subnormal maxima, zeros, NaN and inf."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mx_model as M
import mx_scale_model as S
from test_mx_format_host import _blocks

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("mxsearch") / "mx_search_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "mx_search_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("elem,code", [("mxfp8", "0"), ("mxfp4", "1")])
def test_host_build_of_the_search_arithmetic_equals_the_model(harness, tmp_path, elem, code):
    x = _blocks(elem)
    x.tofile(tmp_path / "in.f32")
    subprocess.run([harness, code, str(tmp_path / "in.f32"), str(tmp_path / "out.scales"), str(tmp_path / "out.err")], check=True)
    s = np.fromfile(tmp_path / "out.scales", np.uint8)
    err = np.fromfile(tmp_path / "out.err", np.float64).reshape(-1, 2)
    want_s, want_err = S.scale_search(x, 1, elem)
    want_s, want_err = want_s.reshape(-1), want_err.reshape(-1, 2)
    assert np.array_equal(s, want_s)
    assert np.array_equal(err.view(np.uint64), want_err.view(np.uint64))
    floor = S.floor_scales(x, 1, elem).reshape(-1)
    up = want_s != floor
    assert up.any() and (~up).any() and np.array_equal(want_s[up], floor[up] + 1)          # both choices occur
    assert (want_s == 0xFF).any() and np.isinf(want_err[want_s == 0xFF]).all()
    assert (floor == 127 - M.EMAX[elem] + 127).any() and not up[floor == 127 - M.EMAX[elem] + 127].any()    # no +1 at the top
    assert (want_err[:, 1] <= want_err[:, 0]).all() and (want_err[up, 1] < want_err[up, 0]).all()
