"""No GPU: tests/mx_fp6_model.py, the definition of `--mx mxfp6_e2m3` / `--mx mxfp6_e3m2` — its rounding against a brute-force
nearest-code search, the shared exponent at its edges, the packed bytes worked by hand, and what the package says about the two
formats without a device: the CLI's rules, the records, the ABI."""
import os
import re

import numpy as np
import pytest

import mx_fp6_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nearest(w, elem):
    """Brute force: the nearest of the 32 magnitudes, a tie to the even code (codes ascend with the mantissa: even index = even
    mantissa), saturating; the sign kept."""
    c = F.codes(elem).astype(np.float64)
    a = np.abs(np.asarray(w, np.float64))
    d = np.abs(a[:, None] - c[None, :])
    best = d.min(axis=1)
    out = np.empty(a.shape)
    for i in range(a.size):
        idx = np.flatnonzero(d[i] == best[i])
        pick = idx[0] if idx.size == 1 else [j for j in idx if j % 2 == 0][0]
        out[i] = c[pick]
    return np.copysign(out, w)


def test_the_code_tables():
    e2m3, e3m2 = F.codes("mxfp6_e2m3"), F.codes("mxfp6_e3m2")
    assert e2m3[:10].tolist() == [0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0, 1.125] and e2m3[-1] == 7.5 and e2m3[24] == 4.0
    assert e3m2[:6].tolist() == [0, 0.0625, 0.125, 0.1875, 0.25, 0.3125] and e3m2[-1] == 28.0 and e3m2[12] == 1.0 and e3m2[-2] == 24.0
    for c in (e2m3, e3m2):
        assert c.size == 32 and (np.diff(c) > 0).all()
    for v in (0, 1, 2, 3, 4, 6):                                                # the exact class exists in both
        assert v in e2m3 and v in e3m2


@pytest.mark.parametrize("elem", F.ELEMS)
def test_rounding_is_nearest_even_and_saturates(elem):
    pts = F.boundary_points(elem)
    assert pts.size > 300 and F.OVER[elem] in pts
    got = F.round_elem(pts.astype(np.float64), elem)
    assert np.array_equal(got, _nearest(pts.astype(np.float64), elem))
    assert np.array_equal(np.signbit(got), np.signbit(pts))                       # the sign of a zero too
    top = F.ELEM_MAX[elem]
    assert F.round_elem(np.array([F.OVER[elem], 1e30, np.inf, -np.inf]), elem).tolist() == [top, top, top, -top]
    assert np.isnan(F.round_elem(np.array([np.nan]), elem)).all()
    rng = np.random.default_rng(3)
    w = rng.uniform(-1.2 * top, 1.2 * top, 4000)
    assert np.array_equal(F.round_elem(w, elem), _nearest(w, elem))
    # ties: E2M3 0.0625 -> 0 and 0.1875 -> 0.25; E3M2 26 -> 24 (even mantissa) and 22 -> 24
    if elem == "mxfp6_e2m3":
        assert F.round_elem(np.array([0.0625, 0.1875, 7.25, 7.75]), elem).tolist() == [0.0, 0.25, 7.0, 7.5]
    else:
        assert F.round_elem(np.array([0.03125, 0.09375, 26.0, 22.0, 30.0]), elem).tolist() == [0.0, 0.125, 24.0, 24.0, 28.0]


@pytest.mark.parametrize("elem", F.ELEMS)
def test_shared_exponent_at_its_edges(elem):
    emax = F.EMAX[elem]
    for k in (-149, -140, -127, -126, -10, 0, 1, 7, 127):
        a = np.float32(2.0 ** k)
        below = np.nextafter(a, np.float32(0))
        assert F.shared_exponent(a, elem) == max(k - emax, -127)
        if below > 0:
            assert F.shared_exponent(below, elem) == max(k - 1 - emax, -127)
    assert F.shared_exponent(np.float32(0), elem) == -127
    # a block at the clamp: se = -127, subnormal inputs and subnormal outputs, exactly
    x = np.zeros((1, 32), np.float32)
    x[0, :4] = np.array([2.0 ** -127, 3 * 2.0 ** -129, 2.0 ** -149, -(2.0 ** -130)], np.float32)
    y, s = F.fake_quant_mx(x, 1, elem, return_scales=True)
    assert s.tolist() == [[[0]]]
    step = 2.0 ** (F.EMIN[elem] - F.MBITS[elem] - 127)                             # 2^-130 resp. 2^-131
    want = np.rint(x.astype(np.float64) / step) * step
    assert np.array_equal(y.astype(np.float64), want) and y[0, 0] == np.float32(2.0 ** -127) and y[0, 2] == 0 and y[0, 3] != 0
    # NaN / inf blocks, zero blocks with their signs
    x = np.ones((3, 40), np.float32)
    x[0, 33], x[1, 2], x[2, :32] = np.nan, -np.inf, -0.0
    y, s = F.fake_quant_mx(x, 1, elem, return_scales=True)
    assert s[:, :, 0].tolist() == [[127 - emax, 0xFF], [0xFF, 127 - emax], [0, 127 - emax]]
    assert np.isnan(y[0, 32:]).all() and np.isnan(y[1, :32]).all() and np.signbit(y[2, :32]).all() and (y[0, :32] == 1).all()


@pytest.mark.parametrize("elem", F.ELEMS)
def test_fake_quant_is_idempotent_and_blocks_along_any_axis(elem):
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((3, 70, 5)) * np.exp(rng.uniform(-20, 20, (3, 1, 5)))).astype(np.float32)
    for axis in (0, 1, 2, -2):
        y = F.fake_quant_mx(x, axis, elem)
        assert np.array_equal(F.fake_quant_mx(y, axis, elem).view(np.uint32), y.view(np.uint32))
    y1 = F.fake_quant_mx(x, 1, elem)
    yt = F.fake_quant_mx(np.ascontiguousarray(x.transpose(0, 2, 1)), 2, elem).transpose(0, 2, 1)
    assert np.array_equal(y1, yt)
    # every value is a value of the format times its block's scale, and the error is at most half a step of the top binade
    c, s = F.element_codes(x, 1, elem)
    assert c.max() < 64 and c.shape == (3, 5, 96) and (c[:, :, 70:] == 0).all()


HAND = [64, 32, 12, 68, 97, 28, 72, 162, 44, 76, 227, 60, 80, 36, 77, 84, 101, 93, 88, 166, 109, 92, 231, 125]


@pytest.mark.parametrize("elem", F.ELEMS)
def test_packed_bytes_worked_by_hand(elem):
    # codes 0 .. 3 are the 24 bits 0 | 1 << 6 | 2 << 12 | 3 << 18 = 0x0C2040: bytes 0x40, 0x20, 0x0C; codes 4 .. 7 give 0x1C6144
    assert HAND[:6] == [0x40, 0x20, 0x0C, 0x44, 0x61, 0x1C]
    assert HAND == list(sum(i << (6 * i) for i in range(32)).to_bytes(24, "little"))
    assert F.pack6(np.arange(32, dtype=np.uint8)).tolist() == HAND
    assert F.unpack6(np.array(HAND, np.uint8)).tolist() == list(range(32))
    x = F.codes(elem).reshape(1, 32)                                              # the largest is the top value: se = 0, the codes 0 .. 31
    codes, scales = F.encode(x, 1, elem)
    assert codes.tolist() == [HAND] and scales.tolist() == [[127]]
    assert np.array_equal(F.decode(codes, scales, elem, (1, 32), 1), x)
    # K = 34: two blocks a row, the second holds two elements and 30 pad codes of 0
    x = np.zeros((2, 34), np.float32)
    x[0, :32], x[0, 32:] = F.codes(elem)[::-1] * -1, [F.ELEM_MAX[elem] * 4, 0.0]
    x[1, 33] = -F.codes(elem)[1] * 2.0 ** -7
    codes, scales = F.encode(x, 1, elem)
    assert codes.shape == (2, 48) and scales.shape == (2, 2) and F.packed_shapes((2, 34), 1, elem) == ((2, 48), (2, 2))
    first = list(sum((32 | (31 - i)) << (6 * i) for i in range(32)).to_bytes(24, "little"))
    assert codes[0, :24].tolist() == first and codes[0, 24:].tolist() == [31] + [0] * 23 and scales[0].tolist() == [127, 129]
    # row 1: a zero block (byte 0, codes 0), then the smallest subnormal at k = 33 as the block's largest: the code is the top power of two
    emax = F.EMAX[elem]
    one = int(np.searchsorted(F.codes(elem), 2.0 ** emax))
    exp_small = int(np.log2(F.codes(elem)[1])) - 7
    assert codes[1, :24].tolist() == [0] * 24 and codes[1, 24:].tolist() == list(((32 | one) << 6).to_bytes(24, "little"))
    assert scales[1].tolist() == [0, exp_small - emax + 127]
    assert np.array_equal(F.decode(codes, scales, elem, (2, 34), 1).view(np.uint32), F.fake_quant_mx(x, 1, elem).view(np.uint32))
    # along a strided axis the codes are K-innermost: a transpose of the element order
    x3 = np.random.default_rng(5).standard_normal((2, 34, 3)).astype(np.float32)
    c3, s3 = F.encode(x3, 1, elem)
    ct, st = F.encode(np.ascontiguousarray(x3.transpose(0, 2, 1)), 2, elem)
    assert c3.shape == (2, 3, 48) and np.array_equal(c3, ct) and np.array_equal(s3, st)
    assert np.array_equal(F.decode(c3, s3, elem, x3.shape, 1).view(np.uint32), F.fake_quant_mx(x3, 1, elem).view(np.uint32))
    # a 0xFF block: every code 0
    x3[0, 5, 1] = np.inf
    c3, s3 = F.encode(x3, 1, elem)
    assert s3[0, 1, 0] == 0xFF and (c3[0, 1, :24] == 0).all() and np.isnan(F.decode(c3, s3, elem, x3.shape, 1)[0, :32, 1]).all()


@pytest.mark.parametrize("elem", F.ELEMS)
def test_scale_search_model_moves_some_blocks_up(elem):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, 96)).astype(np.float32)
    x[:3, 32:64] = 0                                                            # a lone value just under the end of the top binade, which
    x[:3, 35] = 0.999 * 2.0 ** (F.EMAX[elem] + 1)                               # the floor rule saturates and se0 + 1 holds almost exactly
    s, err = F.scale_search(x, 1, elem)
    floor = F.fake_quant_mx(x, 1, elem, return_scales=True)[1]
    assert set((s.astype(int) - floor).reshape(-1).tolist()) == {0, 1}           # both choices occur
    assert (err[..., 1] <= err[..., 0]).all() and (err[..., 1] < err[..., 0])[s != floor].all()
    y = F.fake_quant_mx_scaled(x, 1, elem, s)
    d = (x.astype(np.float64) - y).reshape(6, 3, 32)
    assert np.allclose((d * d).sum(-1), err[:, :, 0, 1], rtol=1e-12)
    assert np.array_equal(F.fake_quant_mx_scaled(x, 1, elem, floor), F.fake_quant_mx(x, 1, elem))
    bad = F.fake_quant_mx_scaled(x, 1, elem, np.full_like(s, 255 - F.EMAX[elem]), return_scales=True)
    assert np.isnan(bad[0]).all() and (bad[1] == 0xFF).all()


# ------------------------------------------------------------------------------------------------ the package, without a device
def _parse(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", "-D", "ocp_fp8", "-A", "hist", *extra])


@pytest.mark.parametrize("elem", F.ELEMS)
def test_cli_takes_the_formats_and_refuses_gptq_and_mixed(elem, capsys):
    from dipoorlet_amd.__main__ import check_args
    assert _parse("--mx", elem).mx == elem
    check_args(_parse("--mx", elem, "--mx_conv", "--mx_scale_search", "--mx_pack", "--mx_verify", "--mx_rotate", "--smooth", "--bc", "--we",
                      "--update_bn"))
    with pytest.raises(ValueError, match=rf"--mx_gptq is not supported with --mx {elem}: .*two grids"):
        check_args(_parse("--mx", elem, "--mx_gptq"))
    with pytest.raises(ValueError, match=rf"--mx_mixed is not supported with --mx {elem}: .*two-level"):
        check_args(_parse("--mx", elem, "--mx_mixed", "6"))
    with pytest.raises(ValueError, match=r"not supported with -D trt"):
        args = _parse("--mx", elem)
        args.deploy = "trt"
        check_args(args)
    with pytest.raises(SystemExit):
        _parse("--mx", "mxfp6")
    assert "invalid choice: 'mxfp6'" in capsys.readouterr().err


def test_the_records_and_the_one_lookup():
    from dipoorlet_amd import ops
    from dipoorlet_amd.platform_settings import MX_CHOICES, mx_fp6_setting_table, mx_setting, mx_setting_table
    from dipoorlet_amd.quantize import FORMATS, MX_FP6_TYPES, MX_TYPES, get_qnode_by_param, number_format
    assert mx_fp6_setting_table == {"mxfp6_e2m3": {"bit_width": 6, "type": "MXFP6E2M3", "block_size": 32},
                                    "mxfp6_e3m2": {"bit_width": 6, "type": "MXFP6E3M2", "block_size": 32}}
    assert MX_CHOICES == ("mxfp8", "mxfp4", "mxfp6_e2m3", "mxfp6_e3m2") and sorted(mx_setting_table) == ["mxfp4", "mxfp8"]
    assert sorted(MX_TYPES) == ["MXFP4E2M1", "MXFP8E4M3"] and not set(MX_FP6_TYPES) & set(FORMATS)
    assert {k: (f.elem, f.elem_type, f.top) for k, f in MX_FP6_TYPES.items()} == {
        "MXFP6E2M3": ("mxfp6_e2m3", "float6e2m3", 7.5), "MXFP6E3M2": ("mxfp6_e3m2", "float6e3m2", 28)}
    for name in MX_CHOICES:
        fmt = number_format(mx_setting(name)["type"])
        assert fmt.block_scaled and fmt.elem == name and not fmt.static and not fmt.integer
        q, lo, hi = get_qnode_by_param(mx_setting(name), "t", [2, 64], None, block_axis=-1)
        assert q.is_mx and q.format is fmt and (lo, hi) == (-fmt.top, fmt.top) and q.saturation() == (-fmt.top, fmt.top)
        (node,) = fmt.onnx_nodes(q)
        assert node.op_type == "MXQuantizeDequantize" and node.attrs["elem_type"] == fmt.elem_type and node.attrs["block_size"] == 32
    assert number_format("Linear") is FORMATS["Linear"] and number_format("MXFP6") is None
    assert mx_setting("mxfp6_e3m2")["bit_width"] == 6 and F.ELEM_MAX == {"mxfp6_e2m3": 7.5, "mxfp6_e3m2": 28.0}
    # ops: the names, the packed shapes, and what stays refused
    assert ops.MX_ELEM["mxfp6_e2m3"] == 6 and ops.MX_ELEM["mxfp6_e3m2"] == 7 and sorted(ops.MX_ELEM.values()) == [0, 1, 6, 7]
    for elem in F.ELEMS:
        for shape, axis in (((5, 34), 1), ((2, 33, 3), 1), ((64, 7), 0), ((1,), 0)):
            assert ops.mx_packed_shapes(shape, axis, elem) == F.packed_shapes(shape, axis, elem)
        assert ops.mx_packed_shapes((4, 96), -1, elem) == ((4, 72), (4, 3))
    from dipoorlet_amd import _hip
    for bad in ("mxfp6", "e5m2", "mxfp6_e2m1"):
        with pytest.raises(_hip.DipoorletHipError, match=r"'mxfp8' or 'mxfp4' \(or 'mxfp6_e2m3' / 'mxfp6_e3m2'\)"):
            ops.mx_packed_shapes((4, 96), -1, bad)


def test_binding_and_header_declare_abi_36():
    from dipoorlet_amd import _hip
    assert _hip.ABI_VERSION >= 36 and (_hip.MX_E2M3, _hip.MX_E3M2) == (6, 7)
    with open(os.path.join(ROOT, "include", "dipoorlet_hip.h")) as f:
        header = f.read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION
    assert re.search(r"#define DPL_MX_E2M3 6\b", header) and re.search(r"#define DPL_MX_E3M2 7\b", header)
