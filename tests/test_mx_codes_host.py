"""No GPU: encode_bits / decode_bits of csrc/mx_format.hpp — the integer step between a rounded MX value and its element code —
compiled for the host into a stand-alone program (tests/mx_codes_host.cpp, with the address and undefined-behaviour sanitizers)
and held to tests/mx_pack_model.py byte for byte: on the block zoo of tests/test_mx_format_host.py (random bit patterns, narrow
blocks anywhere in fp32's range, every code, tie and neighbour under nine shared exponents, subnormal maxima, zeros, NaN and
infinities) and, for decode, on every (code, scale byte) pair there is."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mx_model as M
import mx_pack_model as P
from test_mx_format_host import _blocks

HERE = os.path.dirname(os.path.abspath(__file__))
ELEMS = [("mxfp8", "0"), ("mxfp4", "1")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("mxcodes") / "mx_codes_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "mx_codes_host.cpp"), "-o", exe], check=True)
    return exe


def _decode(harness, d, elem_code, codes, scales):
    codes.tofile(d / "in.codes")
    scales.tofile(d / "in.scales")
    subprocess.run([harness, elem_code, "dec", str(d / "in.codes"), str(d / "in.scales"), str(d / "out.f32")], check=True)
    return np.fromfile(d / "out.f32", np.uint32)


@pytest.mark.parametrize("elem,code", ELEMS)
def test_host_encode_and_decode_equal_the_model_on_the_zoo(harness, tmp_path, elem, code):
    x = _blocks(elem)
    x.tofile(tmp_path / "in.f32")
    subprocess.run([harness, code, "enc", str(tmp_path / "in.f32"), str(tmp_path / "out.codes"), str(tmp_path / "out.scales")], check=True)
    c = np.fromfile(tmp_path / "out.codes", np.uint8)
    s = np.fromfile(tmp_path / "out.scales", np.uint8)
    want_c, want_s = P.encode(x, 1, elem)
    assert np.array_equal(s, want_s.reshape(-1))
    assert np.array_equal(c, want_c.reshape(-1)), np.flatnonzero(c != want_c.reshape(-1))[:5]
    assert (s == 0xFF).any() and (s == 0).any() and np.unique(c).size > (100 if elem == "mxfp8" else 200)
    y = _decode(harness, tmp_path, code, c, s)
    want = M.fake_quant_mx(x, 1, elem)
    nan = np.isnan(want).reshape(-1)
    assert nan.any() and np.array_equal(y[nan], np.full(int(nan.sum()), P.QNAN))
    assert np.array_equal(y[~nan], want.view(np.uint32).reshape(-1)[~nan])


@pytest.mark.parametrize("elem,code", ELEMS)
def test_host_decode_equals_the_model_on_every_pair(harness, tmp_path, elem, code):
    c, s = P.all_pairs(elem)
    y = _decode(harness, tmp_path, code, c, s)
    want = P.decode(c, s, elem, (s.size, 32), 1).view(np.uint32).reshape(-1)
    assert np.array_equal(y, want), np.flatnonzero(y != want)[:5]       # (NaN is 0x7FC00000 on both sides: patterns compare)
