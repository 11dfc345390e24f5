"""The number formats behind a fake-quant node (quantize.FORMATS): one record per "type" string of the platform tables, reached
through the node.  What a node of each format answers is written out here literally, not computed from the table."""
import numpy as np
import pytest
import torch

from dipoorlet_amd.platform_settings import mx_setting_table, platform_setting_table
from dipoorlet_amd.quantize import get_qnode_by_param

LAYER_GRID_MX_REASON = "its weight has no static grid"


def _param_sets():
    """Every parameter set of the two tables, by where it stands."""
    sets = [(f"{deploy}.{role}", plat[role]) for deploy, plat in platform_setting_table.items()
            for role in ("qi_params", "qw_params", "qb_params") if role in plat]
    return sets + [(f"mx.{k}", p) for k, p in mx_setting_table.items()]


PARAM_SETS = _param_sets()


def _ranges(param):
    """A clip range with a negative lower end (dynamic_sym keeps the grid symmetric): per channel where the set asks for it."""
    if param.get("per_channel"):
        return [np.array([-1.0, -0.5, -2.0]), np.array([0.5, 1.5, 2.0])]
    return [-1.5, 2.0]


# type, symmetric -> (saturation(), zp_dtype, is_mx)
EXPECTED = {
    ("Linear", True): ((-128, 127), "int8", False),
    ("Linear", False): ((0, 255), "uint8", False),
    ("Float8E4M3FN", True): ((-448, 448), "float8e4m3fn", False),
    ("MXFP8E4M3", True): ((-448, 448), None, True),
    ("MXFP4E2M1", True): ((-6, 6), None, True),
}


def test_the_tables_hold_every_kind():
    kinds = {(p["type"], bool(p.get("symmetric", True))) for _, p in PARAM_SETS}
    assert kinds == set(EXPECTED)


def test_every_type_of_the_tables_has_a_record():
    from dipoorlet_amd.quantize import FORMATS
    assert {p["type"] for _, p in PARAM_SETS} == {"Linear", "Float8E4M3FN", "MXFP8E4M3", "MXFP4E2M1"} == set(FORMATS)


@pytest.mark.parametrize("where,param", PARAM_SETS, ids=[w for w, _ in PARAM_SETS])
def test_node_of_every_parameter_set(where, param):
    q, q_min, q_max = get_qnode_by_param(param, "t", [3, 4], _ranges(param), block_axis=1)
    sat, zp_dtype, is_mx = EXPECTED[(param["type"], bool(param.get("symmetric", True)))]
    assert q.fmt == param["type"]
    assert q.saturation() == sat
    assert q.is_mx is is_mx
    if zp_dtype is not None:        # (a block-scaled node has no zero point to give a type to)
        assert q.zp_dtype == zp_dtype
    if is_mx:
        assert (q_min, q_max) == sat and q.block_axis == 1 and q.axis is None
    elif param["type"] == "Float8E4M3FN":
        assert (q_min, q_max) == (-448, 448)
    assert q.scale.size == (3 if param.get("per_channel") else 1)


def test_dynamic_sym_switches_a_non_negative_activation_to_the_unsigned_grid():
    qi = platform_setting_table["ti"]["qi_params"]
    q, q_min, q_max = get_qnode_by_param(qi, "t", [3, 4], [0.0, 2.0])
    assert q.fmt == "Linear" and q.saturation() == (0, 255) and q.zp_dtype == "uint8" and not q.is_mx


def test_unknown_type_has_no_node():
    assert get_qnode_by_param({"type": "Float8E5M2", "bit_width": 8, "symmetric": True}, "t", [3, 4], [-1.0, 1.0]) == (None, None, None)


@pytest.mark.parametrize("symmetric,per_channel", [(True, True), (True, False), (False, False), (False, True)])
def test_integer_gptq_grid(symmetric, per_channel):
    param = {"bit_width": 8, "type": "Linear", "symmetric": symmetric, "per_channel": per_channel}
    q, q_min, q_max = get_qnode_by_param(param, "w", [3, 4], _ranges(param))
    grid, why = q.format.gptq_grid(q, q_min, q_max, torch.device("cpu"))
    assert why is None and grid.fmt == "int"
    assert grid.scale.numel() == grid.zero_point.numel() == (3 if per_channel else 1)
    assert grid.zero_point.dtype == torch.int32 and np.array_equal(grid.scale.numpy(), q.scale)
    assert (grid.qlo, grid.qhi) == ((-127, 127) if symmetric else (0, 255))


def test_fp8_gptq_grid():
    param = platform_setting_table["ocp_fp8"]["qw_params"]
    q, q_min, q_max = get_qnode_by_param(param, "w", [3, 4], _ranges(param))
    grid, why = q.format.gptq_grid(q, q_min, q_max, torch.device("cpu"))
    assert why is None and grid.fmt == "e4m3" and grid.zero_point is None and grid.scale.numel() == 3


@pytest.mark.parametrize("mx", sorted(mx_setting_table))
def test_mx_has_no_gptq_grid(mx):
    q, q_min, q_max = get_qnode_by_param(mx_setting_table[mx], "w", [40, 6], None, block_axis=0)
    assert q.format.gptq_grid(q, q_min, q_max, torch.device("cpu")) == (None, LAYER_GRID_MX_REASON)


def test_the_axis_a_node_mixes():
    """Per-channel parameters along `axis`, blocks along `block_axis` (counted from the end too); a per-tensor node mixes none."""
    per_channel, _, _ = get_qnode_by_param(platform_setting_table["trt"]["qw_params"], "w", [3, 4], _ranges({"per_channel": True}))
    per_tensor, _, _ = get_qnode_by_param(platform_setting_table["trt"]["qi_params"], "t", [3, 4], [-1.0, 1.0])
    blocked, _, _ = get_qnode_by_param(mx_setting_table["mxfp8"], "t", [3, 4], None, block_axis=-1)
    assert [per_channel.mixes_axis(k, 2) for k in (0, 1)] == [True, False]
    assert [per_tensor.mixes_axis(k, 2) for k in (0, 1)] == [False, False]
    assert [blocked.mixes_axis(k, 2) for k in (0, 1)] == [False, True] and blocked.mixes_axis(2, 3)


def test_what_else_the_records_answer():
    """Static parameters, a fused producer, block scaling, the whole-set launch and the integer grid, per type."""
    from dipoorlet_amd.quantize import FORMATS, MX_TYPES
    got = {k: (f.static, f.takes_pre, f.block_scaled, f.set_fmt, f.integer) for k, f in FORMATS.items()}
    assert got == {"Linear": (True, True, False, "int", True), "Float8E4M3FN": (True, True, False, "fp8", False),
                   "MXFP8E4M3": (False, False, True, None, False), "MXFP4E2M1": (False, False, True, None, False)}
    assert {k: (f.elem, f.elem_type, f.top) for k, f in MX_TYPES.items()} == {
        "MXFP8E4M3": ("mxfp8", "float8e4m3fn", 448), "MXFP4E2M1": ("mxfp4", "float4e2m1", 6)}
