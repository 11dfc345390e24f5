"""No GPU: the numpy definition of --gptq (gptq_model.py) on the shared cases (gptq_cases.py), the host-side factorisation of the
driver, the CLI's acceptances and refusals, and the binding.

The two caps the GPU test holds the device to against the fp64 model — at most 1 % of the elements different, objective at most
1.02 x — are asserted HERE for the numpy fp32 path on the very same cases: the fp32 recursion (single fp32 operations, an fp32 GEMM
between blocks) is what the device computes, up to the GEMM's summation order.  Measured with these seeds: 0 % and 1.0000 on every
case."""
import warnings

import numpy as np
import pytest

import gptq_cases as C
import gptq_model as M

MAX_DIFF_SHARE, MAX_OBJ_RATIO = 0.01, 1.02


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_results_are_on_the_grid(case):
    d = C.build(case)
    Q = M.make_q(d["grid"])
    for k in ("W32", "W64", "Wn"):
        assert np.array_equal(_bits(Q(d[k])), _bits(d[k])), k        # idempotent under the graph's Q/DQ, bit for bit


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_gptq_lowers_the_objective_and_fp32_stays_with_fp64(case):
    d = C.build(case)
    o_near, o64, o32 = (M.objective(d[k], d["W"], d["H"]) for k in ("Wn", "W64", "W32"))
    share = float(np.mean(_bits(d["W32"]) != _bits(d["W64"])))
    print(f"{C.case_id(case)}: gptq64 / nearest {o64 / o_near:.4f}, fp32 vs fp64: {100 * share:.4f} % differ, objective x {o32 / o64:.5f}")
    assert o64 < o_near
    assert share <= MAX_DIFF_SHARE
    assert o32 <= MAX_OBJ_RATIO * o64


@pytest.mark.parametrize("kind", ["int4", "e4m3", "uint4"])
def test_a_diagonal_hessian_gives_round_to_nearest(kind):
    rng = np.random.default_rng(5)
    W = (0.05 * rng.standard_normal((7, 200))).astype(np.float32)
    H = np.diag(rng.uniform(0.5, 2.0, 200))
    Q = M.make_q(C.make_grid(W, kind))
    U, _ = M.factor(H, 0.01)
    assert np.array_equal(U, np.diag(np.diag(U)))            # nothing off the diagonal: no error is pushed anywhere
    w32, err = M.gptq_layer32(W, U, Q, 128)
    assert np.array_equal(_bits(w32), _bits(Q(W))) and np.array_equal(_bits(M.gptq_layer64(W, U, Q)), _bits(Q(W)))
    assert np.array_equal(err, ((W - Q(W)) / np.diag(U).astype(np.float32)).astype(np.float32))


def test_block_touches_its_own_columns_only_and_blocks_compose():
    d = C.build(C.LAYER_CASES[2])            # 48 x 300
    Q, U = M.make_q(d["grid"]), d["U"].astype(np.float32)
    W = d["W"].copy()
    before = W.copy()
    err = M.gptq_block(W, U, 128, 65, Q)
    assert err.shape == (48, 65)
    assert np.array_equal(_bits(W[:, :128]), _bits(before[:, :128])) and np.array_equal(_bits(W[:, 193:]), _bits(before[:, 193:]))
    assert np.array_equal(_bits(W[:, 128]), _bits(Q(before[:, 128])))          # the block's first column: plain rounding
    # a block size of 1 is the unblocked recursion: it must agree with the fp64 model as well as 128 does
    w1, _ = M.gptq_layer32(d["W"], d["U"], Q, 1)
    assert np.mean(_bits(w1) != _bits(d["W64"])) <= MAX_DIFF_SHARE


def _factors(H, damp):
    """The model's factor and the driver's (torch, host), as (U or None, damp) pairs."""
    import torch
    from dipoorlet_amd.weight_transform.gptq import factor
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        um, dm = M.factor(H, damp)
    ut, dt = factor(torch.from_numpy(np.array(H, np.float64)), damp)
    return (um, dm), (None if ut is None else ut.numpy(), dt)


def test_factor_is_the_upper_cholesky_factor_of_the_damped_inverse():
    d = C.build(C.LAYER_CASES[2])            # N = 64 < K = 300: singular before the damping
    H = d["H"]
    Hd = H + 0.01 * np.mean(np.diag(H)) * np.eye(len(H))
    for U, damp in _factors(H, 0.01):
        assert damp == 0.01 and np.array_equal(U, np.triu(U)) and (np.diag(U) > 0).all()
        assert np.allclose(U.T @ U @ Hd, np.eye(len(H)), atol=1e-8)


def test_dead_columns_are_rounded_to_nearest_and_not_zeroed():
    d = C.build(C.SINGLE_BLOCK)
    H = d["H"].copy()
    dead = [3, 77]
    H[dead, :] = 0
    H[:, dead] = 0
    Q = M.make_q(d["grid"])
    for U, _ in _factors(H, 0.01):
        # a dead column is decoupled: its row and column of U hold the diagonal entry only
        for j in dead:
            assert np.count_nonzero(U[j]) == 1 and np.count_nonzero(U[:, j]) == 1 and U[j, j] > 0
        w32, _ = M.gptq_layer32(d["W"], U, Q, 128)
        assert np.array_equal(_bits(w32[:, dead]), _bits(Q(d["W"])[:, dead]))
        assert np.abs(w32[:, dead]).max() > 0


def test_damping_is_retried_three_times_then_the_layer_is_given_up():
    K = 6
    # indefinite by a wide margin: mean(diag) = 1, smallest eigenvalue -4 — 0.01, 0.1 and 1 fail, 10 succeeds
    H = np.eye(K)
    H[0, 1] = H[1, 0] = 5.0
    for U, damp in _factors(H, 0.01):
        assert U is not None and damp == pytest.approx(10.0)
    H[0, 1] = H[1, 0] = 50.0        # smallest eigenvalue -49: 10 fails too
    for U, damp in _factors(H, 0.01):
        assert U is None
    with pytest.warns(UserWarning, match="round-to-nearest"):
        M.factor(H, 0.01)


# ------------------------------------------------------------------------------------------------ CLI, binding
def _parse(*extra):
    from dipoorlet_amd.__main__ import build_parser
    return build_parser().parse_args(["-I", "calib", "-N", "8", "-M", "m.onnx", *extra])


@pytest.mark.parametrize("deploy", ["trt", "stpu", "magicmind", "rv", "atlas", "snpe", "ti", "imx", "ocp_fp8"])
def test_cli_accepts_gptq_on_every_platform(deploy):
    from dipoorlet_amd.__main__ import check_args
    args = _parse("-D", deploy, "-A", "minmax", "--gptq")
    check_args(args)
    assert args.gptq is True and args.gptq_block == 128 and args.gptq_damp == 0.01
    check_args(_parse("-D", deploy, "-A", "hist", "--gptq", "--gptq_block", "1", "--gptq_damp", "0.1", "--bc", "--we"))


@pytest.mark.parametrize("other", ["--adaround", "--brecq", "--sparse"])
def test_cli_refuses_a_second_rounding_transform(other):
    from dipoorlet_amd.__main__ import check_args
    with pytest.raises(ValueError) as e:
        check_args(_parse("-D", "trt", "-A", "minmax", "--gptq", other))
    assert "--gptq" in str(e.value) and other in str(e.value)


def test_cli_refuses_gptq_with_mx_and_bad_parameters():
    from dipoorlet_amd.__main__ import check_args
    with pytest.raises(ValueError) as e:
        check_args(_parse("-D", "ocp_fp8", "-A", "minmax", "--gptq", "--mx", "mxfp4"))
    assert "--gptq" in str(e.value) and "--mx" in str(e.value)
    for extra in (("--gptq_block", "0"), ("--gptq_block", "129"), ("--gptq_damp", "0"), ("--gptq_damp", "-1"), ("--gptq_damp", "nan")):
        with pytest.raises(ValueError):
            check_args(_parse("-D", "trt", "-A", "minmax", "--gptq", *extra))
    assert _parse("-D", "trt").gptq is False


def test_the_fp8_refusals_are_unchanged():
    from dipoorlet_amd.__main__ import check_args
    with pytest.raises(ValueError) as e:
        check_args(_parse("-D", "ocp_fp8", "-A", "minmax", "--adaround"))
    assert "--adaround not supported" in str(e.value) and "--gptq" not in str(e.value)


def test_binding_declares_dpl_gptq_block():
    import ctypes as ct
    import os
    import re

    from dipoorlet_amd import _hip, ops
    assert _hip.ABI_VERSION >= 28
    res, argtypes = _hip.SIGNATURES["dpl_gptq_block"]
    P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
    assert res is ct.c_int and argtypes == [P, I64, I64, I64, I64, P, I64, P, P, I64, I32, I32, I32, P, P]
    header = open(os.path.join(os.path.dirname(_hip.__file__), "..", "include", "dipoorlet_hip.h")).read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION
    proto = re.search(r"int dpl_gptq_block\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == len(argtypes)
    assert int(re.search(r"#define DPL_GPTQ_MAX_BLOCK (\d+)", header).group(1)) == _hip.GPTQ_MAX_BLOCK == ops.GPTQ_MAX_BLOCK == 128
    assert callable(ops.gptq_block) and callable(ops.gptq_quantize)


# ------------------------------------------------------------------------------------------------ the driver's host-side pieces
@pytest.mark.parametrize("pads,strides,dil", [([1, 1, 1, 1], [1, 1], [1, 1]), ([0, 1, 2, 1], [2, 1], [1, 2]), ([2, 0, 0, 3], [2, 2], [2, 1])])
def test_conv_rows_times_weight_is_the_convolution(pads, strides, dil):
    """The Hessian is taken over the rows X with conv(x, W) = X @ W.reshape(C_out, -1)^T: asymmetric ONNX pads ([top, left, bottom,
    right]), strides and dilations included (CPU tensors: the same torch calls as on the device)."""
    import torch
    from dipoorlet_amd.executor import _conv
    from dipoorlet_amd.onnx_io import Node
    from dipoorlet_amd.weight_transform.gptq import input_rows, rows_per_image
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 5, 9, 8, generator=g, dtype=torch.float64)
    w = torch.randn(4, 5, 3, 2, generator=g, dtype=torch.float64)
    node = Node("Conv", ["x", "w"], ["y"], name="c", attrs={"pads": pads, "kernel_shape": [3, 2], "strides": strides, "dilations": dil, "group": 1})
    y = _conv(None, node, x, w)
    X = input_rows(node, x, tuple(w.shape))
    assert X.shape == (y.shape[0] * y.shape[2] * y.shape[3], 5 * 3 * 2)
    assert rows_per_image(node, x, tuple(w.shape)) == y.shape[2] * y.shape[3]        # (what sizes the Hessian's slabs)
    got = (X @ w.reshape(4, -1).t()).reshape(y.shape[0], y.shape[2], y.shape[3], 4).permute(0, 3, 1, 2)
    assert torch.allclose(got, y, rtol=1e-12, atol=1e-12)


def test_layer_grid_is_the_graphs_own_grid():
    """qlo / qhi: the platform's bit width inside the Q/DQ node's saturation; an asymmetric per-tensor platform gives [0, 2^b - 1]
    around its zero point; FP8 has a scale only."""
    import types
    import torch
    from dipoorlet_amd import models
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.weight_transform.gptq import layer_grid
    g = models.resnet18(seed=3, image=32, width=8, num_classes=10)
    node = next(n for n in g.graph.node if n.op_type == "Conv")
    cpu = torch.device("cpu")
    w = g.get_initializer(node.input[1])
    w2 = w.reshape(w.shape[0], -1).astype(np.float64)
    for deploy, plat in platform_setting_table.items():
        args = types.SimpleNamespace(deploy=deploy, skip_layers=[])
        clip = {node.input[1]: [w2.min(axis=1), w2.max(axis=1)]}          # per output channel, as the weight ranges are kept
        before = [np.copy(clip[node.input[1]][0]), np.copy(clip[node.input[1]][1])]
        grid, why = layer_grid(g, node, clip, args, cpu)
        assert why is None, (deploy, why)
        assert np.array_equal(before[0], clip[node.input[1]][0]) and np.array_equal(before[1], clip[node.input[1]][1])   # ranges untouched
        qw = plat["qw_params"]
        n_scale = g.get_initializer(node.input[1]).shape[0] if qw.get("per_channel") else 1
        assert grid.scale.numel() == n_scale
        if qw["type"].startswith("Float8"):
            assert grid.fmt == "e4m3" and grid.zero_point is None
            continue
        top = 2 ** (qw["bit_width"] - 1) - 1
        assert grid.fmt == "int" and grid.zero_point.numel() == n_scale
        if qw["symmetric"]:
            assert (grid.qlo, grid.qhi) == (-top, top) and not grid.zero_point.any()
        else:
            assert (grid.qlo, grid.qhi) == (0, 2 ** qw["bit_width"] - 1)
            assert 0 <= int(grid.zero_point.min()) and int(grid.zero_point.max()) <= grid.qhi
