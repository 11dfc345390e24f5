"""GPU: `--mx_verify` through the CLI on the mini-ViT of tests/test_mx_pack_e2e.py, under DPL_DETERMINISTIC=1.
mx_verify_report.json lists every MatMul / Gemm of quant_model.onnx whose inputs are both MXQuantizeDequantize outputs — the nine
with a constant operand, whose bytes come back from ocp_mx_weights.bin, under exactly the keys of ocp_mx_weights.json, and the four
two-activation products of the attention blocks (Q . K^T, and attention . V with K = 17 padded to 32) — none skipped, each within
the bound (twice Kp * 2^-23 * S: both sides carry an fp32 summation; S from |A^| . |B^| in the run itself) and at cosine >= 1 - 1e-6.
The same command without --mx_verify differs by the report file alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, IMG = 16, 32
REPORT = "mx_verify_report.json"
CONFIGS = {"mxfp4": ["--mx", "mxfp4", "--mx_pack"], "mxfp8_rotate_smooth_bc": ["--mx", "mxfp8", "--mx_rotate", "--smooth", "--bc", "--mx_pack"]}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mxverify")
    g = models.vit(image=IMG, patch=8, dim=64, depth=2, heads=2, mlp=128, num_classes=10)     # 17 tokens, head dimension 32
    g.output_dir = str(d)
    g.save_onnx_model("vit")
    os.makedirs(d / "calib" / "input")
    rng = np.random.default_rng(12)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(d / "calib" / "input" / f"{i}.bin")
    return d


def _cli(workdir, out, extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["DPL_DETERMINISTIC"] = "1"
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "vit.onnx"), "-I", str(workdir / "calib"),
           "-N", str(N), "-A", "hist", "-D", "ocp_fp8", "-O", str(out), "--calib_batch", "8", *extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _files(d):
    return {os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs}


@pytest.mark.two_forwards
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_cli_verifies_the_packed_operands_on_the_matrix_instruction(workdir, config):
    from dipoorlet_amd import onnx_io
    elem = CONFIGS[config][1]
    out = workdir / (config + "_verify")
    _cli(workdir, out, CONFIGS[config] + ["--mx_verify"])
    rep = json.load(open(out / REPORT))
    meta = json.load(open(out / "ocp_mx_weights.json"))
    assert rep["format"] == elem and rep["images"] == 8 and rep["skipped"] == {}
    # every MatMul / Gemm of the saved Q/DQ model whose inputs are both MX outputs
    model = onnx_io.load_model(str(out / "quant_model.onnx"))
    mx_out = {o for n in model.nodes if n.op_type == "MXQuantizeDequantize" for o in n.output}
    want = {n.name: n for n in model.nodes if n.op_type in ("MatMul", "Gemm") and n.input[0] in mx_out and n.input[1] in mx_out}
    assert set(rep["nodes"]) == set(want) and len(want) == 13
    keys = [v["constant"] for v in rep["nodes"].values() if v["constant"] is not None]
    assert sorted(keys) == sorted(meta["tensors"]) and len(keys) == 9
    worst = 0.0
    for name, v in rep["nodes"].items():
        assert v["op"] == want[name].op_type
        if v["constant"] is not None:
            t = meta["tensors"][v["constant"]]
            assert v["k"] == t["k"] and v["n"] == t["codes"]["shape"][0]
        print(f"{config} {name}: [{v['m']} x {v['n']} x {v['k']}] max |err| {v['max_abs_err']:.3e}, {v['max_err_over_bound']:.4g} of the bound, "
              f"1 - cosine {1 - v['cosine']:.2e}")
        assert v["within_bound"] is True and v["max_err_over_bound"] <= 1.0 and v["cosine"] >= 1 - 1e-6, (name, v)
        worst = max(worst, v["max_err_over_bound"])
    print(f"{config}: worst max_err_over_bound {worst:.4g}")
    assert {v["k"] for v in rep["nodes"].values()} >= {17, 32, 64, 128}       # attention . V pads K = 17 to 32
    if config == "mxfp4":        # without --mx_verify: no report, and every other file byte for byte
        plain = workdir / (config + "_plain")
        _cli(workdir, plain, CONFIGS[config])
        assert _files(out) - _files(plain) == {REPORT} and _files(plain) - _files(out) == set()
        for f in sorted(_files(plain) - {"log.txt"}):
            assert open(plain / f, "rb").read() == open(out / f, "rb").read(), f
