"""CPU: the definition of --mx_gptq (tests/mx_gptq_model.py) against its own claims, the CLI's refusals and the binding.

The claim everything rests on: fix a block's shared exponent by the floor rule when the column recursion enters the block, round
every column of it under that exponent (saturating), and the finished weight is a fixed point of the ordinary floor-rule Q/DQ —
mx_model.fake_quant_mx(Wq) == Wq bit for bit — although the result's own floor exponent may be lower than the entry one.  The
numeric caps are test_gptq_gpu.py's own: the fp32 path against the fp64 recursion differs in at most 1 % of the bit patterns and
its objective is at most 1.02 x (measured on these cases: mxfp4 0 %, ratio 1.00000; mxfp8 0 - 0.38 %, ratio 0.99998 - 1.0016); and
GPTQ's objective lies below round-to-nearest's (measured: ratios 0.02 - 0.62).

For E4M3 the claim needs one rule more than plain rounding under the entry exponent (mx_gptq_model.py's docstring: the format has
no 1.875 * 2^8, so 1.875 * 2^t must not end up as the largest value of a block that has shrunk below its entry binade);
test_the_e4m3_rule_... shows the block that is no fixed point without it."""
import numpy as np
import pytest

import mx_gptq_cases as C
import mx_gptq_model as G
import mx_model as M
import mx_scale_model as S


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("elem", C.ELEMS)
@pytest.mark.parametrize("case", C.LAYER_CASES + [C.RAGGED], ids=C.case_id)
def test_layer_is_a_fixed_point_within_the_caps_and_beats_nearest(case, elem):
    d = C.build(case, elem)
    W32, R = d["W32"], case[0]
    assert np.array_equal(_bits(M.fake_quant_mx(W32, 1, elem)), _bits(W32))                                  # the graph's own node
    assert np.array_equal(_bits(S.fake_quant_mx_scaled(W32, 1, elem, d["S32"].reshape(R, -1, 1))), _bits(W32))   # ... and the entry bytes
    assert d["S32"].shape == (R, -(-case[1] // 32)) and not (d["S32"] == 0xFF).any()
    floor = M.fake_quant_mx(W32, 1, elem, return_scales=True)[1].reshape(d["S32"].shape)
    assert (floor <= d["S32"]).all()                                                                         # se' <= se
    o32, o64, on = (G.objective(d[k], d["W"], d["H"]) for k in ("W32", "W64", "Wn"))
    differ = float(np.mean(_bits(W32) != _bits(d["W64"])))
    print(f"{C.case_id(case)} {elem}: fp32 vs fp64 {100 * differ:.4f} % differ, objective x {o32 / o64:.5f}; gptq / nearest {o32 / on:.4f}; "
          f"{int((floor < d['S32']).sum())} of {floor.size} blocks end below their entry exponent")
    assert differ <= 0.01 and o32 <= 1.02 * o64
    assert o32 < on
    assert not np.array_equal(_bits(W32), _bits(d["Wn"]))


@pytest.mark.parametrize("elem", C.ELEMS)
def test_a_smaller_call_size_keeps_the_fixed_point(elem):
    W, H, U = C.draw(C.RAGGED)
    W32, _, s = G.gptq_mx_layer32(W, U, elem, 32)
    assert np.array_equal(_bits(M.fake_quant_mx(W32, 1, elem)), _bits(W32))
    assert G.objective(W32, W, H) < G.objective(M.fake_quant_mx(W, 1, elem), W, H)


def _run(name, elem):
    W, U = C.constructed(name, elem)
    Wq = W.copy()
    err, scales = G.gptq_mx_block(Wq, U, 0, 32, elem, 32)
    assert np.array_equal(_bits(M.fake_quant_mx(Wq, 1, elem)), _bits(Wq)), name              # the fixed point, whatever happened
    return W, U, Wq, err, scales


@pytest.mark.parametrize("elem", C.ELEMS)
def test_constructed_compensation_shrinks_the_block_into_a_lower_binade(elem):
    W, U, Wq, err, scales = _run("shrink", elem)
    assert (scales[:, 0] == [127, 127, 107]).all()                                           # se = 0, 0, -20 at the entry
    floor = M.fake_quant_mx(Wq, 1, elem, return_scales=True)[1].reshape(-1)
    assert (floor < scales[:, 0]).all()                                                      # the result's own floor byte is lower
    assert np.array_equal(_bits(Wq[1]), _bits(-Wq[0])) and np.array_equal(_bits(Wq[2]), _bits(Wq[0] * np.float32(2.0 ** -20)))
    assert (np.abs(Wq[0, 5]) < 0.5 * np.abs(W[0, 5]))                                        # column 5 did lose most of its value


def test_the_e4m3_rule_keeps_the_open_end_of_the_top_binade_out_of_the_maximum():
    """Why the rule exists: the shrink case's column 5 arrives at 0.4 * 300 = 120 = 1.875 * 2^6 as the block's largest value; plain
    rounding under the entry exponent keeps 120, and the floor rule of the finished block (se' = -2: top 112) saturates it."""
    W, U, Wq, err, scales = _run("shrink", "mxfp8")
    plain = W.copy()
    se =np.zeros(3, np.int64) + [0, 0, -20]
    for c in range(32):
        w = plain[:, c].copy()
        q = S._qdq64(w.astype(np.float64), se, "mxfp8").astype(np.float32)
        e = ((w - q).astype(np.float32) / U[c, c]).astype(np.float32)
        plain[:, c] = q
        for k in range(c + 1, 32):
            plain[:, k] = (plain[:, k] - (e * U[c, k]).astype(np.float32)).astype(np.float32)
    assert plain[0, 5] == 120.0 and M.fake_quant_mx(plain, 1, "mxfp8")[0, 5] == 112.0          # no fixed point without the rule
    assert Wq[0, 5] in (112.0, 128.0) and np.array_equal(_bits(Wq[:, :5]), _bits(plain[:, :5]))
    # 1.875 * 2^t below the running maximum stays; as the maximum so far it moves to the nearer neighbour (a tie: down)
    U1 = np.eye(32, dtype=np.float32)
    row = np.zeros((4, 32), np.float32)
    row[0, :2], row[1, :2], row[2, :2], row[3, :2] = (300.0, 120.0), (120.0, 300.0), (123.0, 300.0), (-117.0, 300.0)
    G.gptq_mx_block(row, U1, 0, 32, "mxfp8", 32)
    assert row[:, :2].tolist() == [[288.0, 120.0], [112.0, 288.0], [128.0, 288.0], [-112.0, 288.0]]
    assert np.array_equal(_bits(M.fake_quant_mx(row, 1, "mxfp8")), _bits(row))


@pytest.mark.parametrize("elem", C.ELEMS)
def test_constructed_compensation_past_the_top_saturates(elem):
    W, U, Wq, err, scales = _run("saturate", elem)
    top = np.float32(M.ELEM_MAX[elem])
    assert (scales[:, 0] == [127, 127, 107]).all()
    assert np.array_equal(_bits(Wq[:, 3]), _bits(np.array([top, -top, top * np.float32(2.0 ** -20)], np.float32)))
    assert np.abs(W[0, 3]) < top                                                             # it was pushed there, not born there
    assert err[0, 3] * U[3, 3] > 1.0                                                         # ... and the clipped part is in the error


@pytest.mark.parametrize("elem", C.ELEMS)
def test_constructed_all_zero_rows(elem):
    W, U, Wq, err, scales = _run("zeros", elem)
    assert (scales == 0).all()
    assert np.array_equal(_bits(Wq), _bits(W)) and np.signbit(Wq).any() and not np.signbit(Wq).all()
    assert (err == 0).all()


@pytest.mark.parametrize("elem", C.ELEMS)
def test_constructed_ties_round_to_even(elem):
    W, U, Wq, err, scales = _run("ties", elem)
    want = np.array([q for _, q in C.TIES[elem]], np.float32)
    n = len(want)
    assert (scales[:, 0] == [127, 127, 107]).all()
    assert np.array_equal(_bits(Wq[0, :n]), _bits(want)) and np.array_equal(_bits(Wq[1, :n]), _bits(-want))
    assert np.array_equal(_bits(Wq[2, :n]), _bits(want * np.float32(2.0 ** -20)))


@pytest.mark.parametrize("elem", C.ELEMS)
def test_a_non_finite_block_is_a_nan_block(elem):
    W, U = C.constructed("shrink", elem)
    W = np.concatenate([W, W], axis=1)
    U2 = np.eye(64, dtype=np.float32)
    U2[:32, :32] = U
    W[0, 40], W[1, 33] = np.inf, np.nan
    err, scales = G.gptq_mx_block(W, U2, 0, 64, elem, 64)
    assert (scales[:2, 1] == 0xFF).all() and np.isnan(W[:2, 32:]).all()
    assert (scales[:, 0] != 0xFF).all() and scales[2, 1] != 0xFF and np.isfinite(W[2]).all() and np.isfinite(W[:, :32]).all()


# ------------------------------------------------------------------------------------------------ the CLI and the binding
def _parse(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", "-D", "ocp_fp8", "-A", "hist", *extra])


def test_check_args_refusals_and_the_valid_combination():
    from dipoorlet_amd.__main__ import check_args
    assert _parse().mx_gptq is False
    with pytest.raises(ValueError, match="--mx_gptq needs --mx"):
        check_args(_parse("--mx_gptq"))
    with pytest.raises(ValueError) as e:
        check_args(_parse("--mx", "mxfp4", "--mx_gptq", "--gptq"))
    assert "--mx_gptq" in str(e.value) and "--gptq " in str(e.value)
    with pytest.raises(ValueError) as e:
        check_args(_parse("--mx", "mxfp4", "--mx_gptq", "--mx_scale_search"))
    assert "--mx_gptq" in str(e.value) and "--mx_scale_search" in str(e.value)
    with pytest.raises(ValueError, match="--gptq_block"):
        check_args(_parse("--mx", "mxfp4", "--mx_gptq", "--gptq_block", "48"))
    with pytest.raises(ValueError, match="--gptq_damp"):
        check_args(_parse("--mx", "mxfp4", "--mx_gptq", "--gptq_damp", "0"))
    for fmt in ("mxfp4", "mxfp8"):
        for block in ("32", "64", "96", "128"):
            check_args(_parse("--mx", fmt, "--mx_gptq", "--gptq_block", block, "--smooth", "--mx_rotate", "--bc", "--mx_pack", "--mx_verify"))
    with pytest.raises(ValueError, match="GPTQ on MX grids is not built"):           # --gptq's own refusal and its text stay
        check_args(_parse("--mx", "mxfp4", "--gptq"))


def test_binding_declares_dpl_gptq_mx_block():
    import ctypes as ct
    import os
    import re

    from dipoorlet_amd import _hip, ops
    assert _hip.ABI_VERSION >= 33
    res, argtypes = _hip.SIGNATURES["dpl_gptq_mx_block"]
    P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
    assert res is ct.c_int and argtypes == [I32, P, I64, I64, I64, I64, I64, P, I64, P, P, I64, P]
    header = open(os.path.join(os.path.dirname(_hip.__file__), "..", "include", "dipoorlet_hip.h")).read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION
    proto = re.search(r"int dpl_gptq_mx_block\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == len(argtypes)
    assert callable(ops.gptq_mx_block) and callable(ops.gptq_mx_quantize) and callable(ops.gptq_mx_nearest)


def test_matmul_rows_and_rows_per_image():
    import torch
    from dipoorlet_amd.onnx_io import Node
    from dipoorlet_amd.weight_transform.gptq import input_rows, rows_per_image
    node = Node("MatMul", ["x", "w"], ["y"], name="m")
    x = torch.arange(2 * 3 * 5 * 4, dtype=torch.float32).reshape(2, 3, 5, 4)
    X = input_rows(node, x, (4, 7))
    assert X.shape == (30, 4) and torch.equal(X[7], x[0, 1, 2]) and rows_per_image(node, x, (4, 7)) == 15
    assert rows_per_image(node, x[:, 0, 0], (4, 7)) == 1 and input_rows(node, x[:, 0, 0], (4, 7)).shape == (2, 4)
