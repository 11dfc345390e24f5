"""No GPU: csrc/mx_format.hpp — the integer arithmetic the MX kernels run on fp32 bit patterns — compiled for the host into a
stand-alone program (tests/mx_format_host.cpp, with the address and undefined-behaviour sanitizers) and held to tests/mx_model.py
bit for bit: random bit patterns, blocks whose elements share a few binades, every code, tie and neighbour of the element format
under nine shared exponents (the clamp at -127 and the largest one included), subnormal maxima, zeros, NaN and infinities."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mx_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("mxhost") / "mx_format_host")
    subprocess.run([cxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "mx_format_host.cpp"), "-o", exe], check=True)
    return exe


def _blocks(elem):
    rng = np.random.default_rng(1)
    out = [rng.integers(0, 2 ** 32, size=(2000, 32), dtype=np.uint64).astype(np.uint32).view(np.float32)]
    for spread in (1, 3, 8, 20):            # exponents of a block within `spread` binades of each other, anywhere in fp32's range
        e = rng.integers(0, 255, size=(1500, 1))
        ee = np.clip(e - rng.integers(0, spread, size=(1500, 32)), 0, 254)
        bits = (rng.integers(0, 2, size=(1500, 32)) << 31) | (ee << 23) | rng.integers(0, 2 ** 23, size=(1500, 32))
        out.append(bits.astype(np.uint32).view(np.float32))
    pts = M.boundary_points(elem)
    for se in (-127, -126, -120, -119, -118, -20, 0, 30, 127 - M.EMAX[elem]):
        n = -(-pts.size // 31)
        blk = np.zeros((n, 32), np.float64)
        blk[:, 0] = M.ELEM_MAX[elem]          # pins the block's shared exponent to se
        blk[:, 1:].reshape(-1)[:pts.size] = pts
        out.append(np.ldexp(blk, se).astype(np.float32))
    sub = rng.integers(0, 2 ** 23, size=(1000, 32)).astype(np.uint32) >> rng.integers(0, 23, size=(1000, 1)).astype(np.uint32)
    out.append((sub | (rng.integers(0, 2, size=(1000, 32)).astype(np.uint32) << 31)).view(np.float32))      # subnormal maxima
    z = np.zeros((4, 32), np.float32)
    z[0, ::2] = -0.0
    z[1, 3], z[2, 5], z[3, 7] = np.nan, np.inf, -np.inf
    out.append(z)
    return np.concatenate(out).astype(np.float32)


@pytest.mark.parametrize("elem,code", [("mxfp8", "0"), ("mxfp4", "1")])
def test_host_build_of_the_kernel_arithmetic_equals_the_model(harness, tmp_path, elem, code):
    x = _blocks(elem)
    x.tofile(tmp_path / "in.f32")
    subprocess.run([harness, code, str(tmp_path / "in.f32"), str(tmp_path / "out.f32"), str(tmp_path / "out.scales")], check=True)
    y = np.fromfile(tmp_path / "out.f32", np.float32).reshape(x.shape)
    s = np.fromfile(tmp_path / "out.scales", np.uint8)
    want_y, want_s = M.fake_quant_mx(x, 1, elem, return_scales=True)
    assert np.array_equal(s, want_s.reshape(-1))
    nan = np.isnan(want_y)
    assert nan.any() and np.array_equal(np.isnan(y), nan)
    assert np.array_equal(y.view(np.uint32)[~nan], want_y.view(np.uint32)[~nan])
    assert (s == 0).any() and (s == 127 - M.EMAX[elem] + 127).any() and (want_y[~nan] != 0).any()
