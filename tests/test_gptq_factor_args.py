"""CPU: --gptq_factor's parser default and refusal, and the three places that declare the C ABI of the device factorisation."""
import os
import re

import pytest


def test_flag_default_refusal_and_abi():
    from dipoorlet_amd import _hip
    from dipoorlet_amd.__main__ import build_parser, check_args
    base = ["-M", "m.onnx", "-I", "in", "-N", "1", "-D", "ocp_fp8", "-A", "minmax"]
    assert build_parser().parse_args(base).gptq_factor == "host"
    check_args(build_parser().parse_args(base + ["--gptq", "--gptq_factor", "device"]))
    check_args(build_parser().parse_args(base + ["--mx", "mxfp4", "--mx_gptq", "--gptq_factor", "device"]))
    with pytest.raises(ValueError, match="--gptq_factor device needs --gptq or --mx_gptq"):
        check_args(build_parser().parse_args(base + ["--gptq_factor", "device"]))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dipoorlet_hip.h")).read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION == 37
    assert int(re.search(r"#define DPL_GPTQ_FACTOR_MAX_K (\d+)", header).group(1)) == _hip.GPTQ_FACTOR_MAX_K >= 16384
    for name, n_args in (("dpl_gptq_factor_workspace", 1), ("dpl_gptq_factor", 8), ("dpl_gptq_factor_phase", 9)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl is not None and len(decl.group(1).split(",")) == n_args == len(_hip.SIGNATURES[name][1]), name
