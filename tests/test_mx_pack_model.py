"""No GPU: tests/mx_pack_model.py — the bytes of `--mx_pack` — against tests/mx_model.py, the values: decode(encode(x)) is
fake_quant_mx(x) bit for bit on the block zoo of tests/test_mx_format_host.py and on a strided tensor with a short last block;
the nibble order, the pad codes and the NaN codes on hand-written blocks; decode on every (code, scale byte) pair; and what the
CLI and the binding declare."""
import os
import re

import numpy as np
import pytest

import mx_model as M
import mx_pack_model as P
from test_mx_format_host import _blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMS = ("mxfp8", "mxfp4")


def _same_bits(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert (got.view(np.uint32)[nan] == P.QNAN).all()


@pytest.mark.parametrize("elem", ELEMS)
def test_decode_of_encode_is_the_qdq_pair_on_the_zoo(elem):
    x = _blocks(elem)
    c, s = P.encode(x, 1, elem)
    assert c.dtype == np.uint8 and s.dtype == np.uint8
    assert c.shape == (x.shape[0], 32 if elem == "mxfp8" else 16) and s.shape == (x.shape[0], 1)
    assert np.array_equal(s, M.fake_quant_mx(x, 1, elem, return_scales=True)[1].reshape(-1, 1))
    assert (s == 0xFF).any() and (s == 0).any() and (s == 127 - M.EMAX[elem] + 127).any()
    _same_bits(P.decode(c, s, elem, x.shape, 1), M.fake_quant_mx(x, 1, elem))
    if elem == "mxfp8":          # every finite code of either sign is used somewhere, the NaN code only in 0xFF blocks
        assert set(np.unique(c).tolist()) == set(range(256)) - {0xFF}
        assert ((c == 0x7F) == (s == 0xFF)).all()
    else:
        assert set(np.unique(P.unpack_nibbles(c)).tolist()) == set(range(16))
        assert (c[s[:, 0] == 0xFF] == 0).all()


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("axis", [1, -2, 0, 2])
def test_decode_of_encode_on_a_strided_tensor_with_a_short_last_block(elem, axis):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 70, 5)) * np.exp2(rng.integers(-20, 20, (3, 70, 5)))).astype(np.float32)
    x.reshape(-1)[::37] = 0.0
    x.reshape(-1)[5::91] = -0.0
    c, s = P.encode(x, axis, elem)
    assert (c.shape, s.shape) == P.packed_shapes(x.shape, axis, elem)
    if axis in (1, -2):
        assert c.shape == (3, 5, 96 if elem == "mxfp8" else 48) and s.shape == (3, 5, 3)
        want_s = M.fake_quant_mx(x, axis, elem, return_scales=True)[1]                  # [outer, nblk, inner]
        assert np.array_equal(s, want_s.transpose(0, 2, 1))                             # K-innermost: the axis swap
        assert (c[:, :, (70 if elem == "mxfp8" else 35):] == 0).all()                   # the 26 pad codes of the last block
    _same_bits(P.decode(c, s, elem, x.shape, axis), M.fake_quant_mx(x, axis, elem))


def test_hand_written_blocks():
    """K = 34: one full block and a block of two elements; se = 0 under mxfp8's sentinel 448 resp. mxfp4's 6."""
    x = np.zeros((1, 34), np.float32)
    x[0, :8] = [6.0, -0.5, 1.0, -1.5, 0.0, -0.0, 3.0, -4.0]
    x[0, 32:] = [-2.0, 2.0]
    c, s = P.encode(x, 1, "mxfp4")
    assert c.shape == (1, 32) and s.tolist() == [[127, 126]]
    # the even index in the LOW nibble: (6, -0.5) -> 0x7 | 0x9 << 4, (1, -1.5) -> 0x2 | 0xB << 4, (0, -0) -> 0x0 | 0x8 << 4, (3, -4) -> 0x5 | 0xE << 4
    assert c[0, :4].tolist() == [0x97, 0xB2, 0x80, 0xE5] and (c[0, 4:16] == 0).all()
    # block 1: max 2 -> se = -1; -2 and 2 are -4 and 4 in its units: 0xE, 0x6; thirty pad codes of 0
    assert c[0, 16] == 0x6E and (c[0, 17:] == 0).all()
    x8 = x.copy()
    x8[0, 8] = 448.0
    c, s = P.encode(x8, 1, "mxfp8")
    assert c.shape == (1, 64) and s.tolist() == [[127, 120]]
    # OCP E4M3FN bytes: 6 = 1.5 * 2^2 -> 0x4C, -0.5 -> 0xB0, 1 -> 0x38, -1.5 -> 0xBC, 0, -0 -> 0x80, 3 -> 0x44, -4 -> 0xC8, 448 -> 0x7E
    assert c[0, :9].tolist() == [0x4C, 0xB0, 0x38, 0xBC, 0x00, 0x80, 0x44, 0xC8, 0x7E] and (c[0, 9:32] == 0).all()
    assert c[0, 32:34].tolist() == [0xF8, 0x78] and (c[0, 34:] == 0).all()              # -+2 = -+256 * 2^-7: S.1111.000
    for bad in (np.nan, np.inf, -np.inf):       # a 0xFF block: 0x7F for the elements that exist (0 in E2M1), pad codes stay 0
        x8[0, 33] = bad
        c, s = P.encode(x8, 1, "mxfp8")
        assert s.tolist() == [[127, 0xFF]] and c[0, 32:34].tolist() == [0x7F, 0x7F] and (c[0, 34:] == 0).all()
        c, s = P.encode(x8, 1, "mxfp4")
        assert s[0, 1] == 0xFF and (c[0, 16:] == 0).all()


def test_decode_on_every_code_and_scale_pair():
    for elem in ELEMS:
        c, s = P.all_pairs(elem)
        y = P.decode(c, s, elem, (s.size, 32), 1)
        codes = c if elem == "mxfp8" else P.unpack_nibbles(c)
        sc = np.broadcast_to(s, codes.shape)
        vals = M.codes(elem).astype(np.float64)
        nbits = 7 if elem == "mxfp8" else 3
        mag, neg = codes & ((1 << nbits) - 1), (codes >> nbits) & 1
        nan = (sc == 0xFF) | ((mag == 0x7F) if elem == "mxfp8" else False)
        assert np.isnan(y[nan]).all() and (y.view(np.uint32)[nan] == 0x7FC00000).all() and not np.isnan(y[~nan]).any()
        exact = np.where(neg == 1, -1.0, 1.0)[~nan] * vals[np.minimum(mag, vals.size - 1)][~nan] * np.exp2(sc[~nan].astype(np.float64) - 127)
        over = np.abs(exact) > np.finfo(np.float32).max
        assert over.any() and np.array_equal(y[~nan][over], np.sign(exact[over]) * np.inf)          # above fp32's range: +-inf
        assert np.array_equal(y[~nan][~over].astype(np.float64), exact[~over])                       # everything else exactly
        assert np.array_equal(np.signbit(y[~nan]), neg[~nan] == 1)                                   # (the zeros' signs too)
        assert np.abs(exact[exact != 0]).min() == 2.0 ** (-136 if elem == "mxfp8" else -128)         # subnormal, never flushed
        enc_reach = sc <= 127 - M.EMAX[elem] + 127        # what the encoder can emit never overflows
        assert not np.isinf(y[~nan & enc_reach]).any()


def _cli(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", *extra])


def test_mx_pack_needs_mx():
    from dipoorlet_amd.__main__ import check_args
    with pytest.raises(ValueError, match=r"--mx_pack needs --mx"):
        check_args(_cli("-D", "ocp_fp8", "-A", "hist", "--mx_pack"))
    for mx in ELEMS:
        check_args(_cli("-D", "ocp_fp8", "-A", "hist", "--mx", mx, "--mx_pack"))
        check_args(_cli("-D", "ocp_fp8", "-A", "hist", "--mx", mx, "--mx_pack", "--mx_rotate", "--smooth", "--bc"))
    assert _cli("-D", "ocp_fp8").mx_pack is False


def test_abi_declares_the_kernels():
    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 30
    header = open(os.path.join(ROOT, "include", "dipoorlet_hip.h")).read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION
    for sym in ("dpl_mx_encode", "dpl_mx_decode"):
        assert sym in _hip.SIGNATURES and re.search(r"\bint %s\(" % sym, header)
        assert len(_hip.SIGNATURES[sym][1]) == 8
