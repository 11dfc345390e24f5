"""GPU: the two MXFP6 formats through the CLI, under DPL_DETERMINISTIC=1.  On the mini-ViT of tests/test_mx_verify_e2e.py:
`--mx mxfp6_e2m3 --mx_scale_search --mx_pack --mx_verify` and `--mx mxfp6_e3m2 --mx_rotate --smooth --bc --mx_pack --mx_verify` —
every node of mx_verify_report.json within its bound (the format's own factor, mx_verify.BOUND_FACTOR) and none skipped, every codes
section of ocp_mx_weights.bin rows * Kp * 3 / 4 bytes on a 64-byte boundary and equal to the model's bytes of the weight the run
saved, and a run without --mx_verify differing by the report alone.  On the small ResNet of tests/test_mx_conv_e2e.py: `--mx_conv`
with mxfp6_e2m3, all 20 Convs and the Gemm verified on the block-scaled matrix instruction."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mx_fp6_model as F

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16
REPORT = "mx_verify_report.json"
VIT = {"mxfp6_e2m3": ["--mx", "mxfp6_e2m3", "--mx_scale_search", "--mx_pack"],
       "mxfp6_e3m2": ["--mx", "mxfp6_e3m2", "--mx_rotate", "--smooth", "--bc", "--mx_pack"]}
ELEM_TYPE = {"mxfp6_e2m3": "float6e2m3", "mxfp6_e3m2": "float6e3m2"}


def _calib(d, image, seed):
    os.makedirs(d / "calib" / "input")
    rng = np.random.default_rng(seed)
    for i in range(N):
        rng.standard_normal(3 * image * image).astype(np.float32).tofile(d / "calib" / "input" / f"{i}.bin")


@pytest.fixture(scope="module")
def vit_dir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mxfp6vit")
    g = models.vit(image=32, patch=8, dim=64, depth=2, heads=2, mlp=128, num_classes=10)
    g.output_dir = str(d)
    g.save_onnx_model("vit")
    _calib(d, 32, 12)
    return d


@pytest.fixture(scope="module")
def resnet_dir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mxfp6conv")
    g = models.resnet18(width=24, image=64, num_classes=10)
    g.output_dir = str(d)
    g.save_onnx_model("resnet")
    _calib(d, 64, 14)
    return d


def _cli(workdir, model, out, extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["DPL_DETERMINISTIC"] = "1"
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / model), "-I", str(workdir / "calib"),
           "-N", str(N), "-A", "hist", "-D", "ocp_fp8", "-O", str(out), "--calib_batch", "8", *extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _files(d):
    return {os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs}


def _within(rep, config):
    worst = 0.0
    for name, v in rep["nodes"].items():
        print(f"{config} {name}: max |err| {v['max_abs_err']:.3e}, {v['max_err_over_bound']:.4g} of the bound, 1 - cosine {1 - v['cosine']:.2e}")
        assert v["within_bound"] is True and v["max_err_over_bound"] <= 1.0 and v["cosine"] >= 1 - 1e-6, (name, v)
        worst = max(worst, v["max_err_over_bound"])
    print(f"{config}: worst max_err_over_bound {worst:.4g}")


def _sections(out, elem):
    """Every entry of ocp_mx_weights.json: the codes section is rows * Kp * 3 / 4 bytes, both sections on 64-byte boundaries."""
    meta = json.load(open(out / "ocp_mx_weights.json"))
    blob = np.fromfile(out / "ocp_mx_weights.bin", dtype=np.uint8)
    assert meta["format"] == elem and meta["layout"] == "k_innermost"
    for key, t in meta["tensors"].items():
        rows = int(np.prod(t["shape"])) // t["k"]
        assert t["k_padded"] == 32 * -(-t["k"] // 32)
        assert t["codes"]["nbytes"] == rows * t["k_padded"] * 3 // 4 and t["codes"]["shape"][-1] == t["k_padded"] * 3 // 4, key
        assert t["scales"]["nbytes"] == rows * t["k_padded"] // 32
        assert t["codes"]["offset"] % 64 == 0 and t["scales"]["offset"] % 64 == 0
        assert t["scales"]["offset"] + t["scales"]["nbytes"] <= blob.size
    return meta, blob


@pytest.mark.parametrize("config", sorted(VIT))
def test_cli_on_the_vit(vit_dir, config):
    from dipoorlet_amd import onnx_io
    out = vit_dir / (config + "_verify")
    _cli(vit_dir, "vit.onnx", out, VIT[config] + ["--mx_verify"])
    rep = json.load(open(out / REPORT))
    assert rep["format"] == config and rep["images"] == 8 and rep["skipped"] == {}
    model = onnx_io.load_model(str(out / "quant_model.onnx"))
    mx_nodes = [n for n in model.nodes if n.op_type == "MXQuantizeDequantize"]
    assert mx_nodes and all(n.attrs["elem_type"] == ELEM_TYPE[config] and int(n.attrs["block_size"]) == 32 for n in mx_nodes)
    mx_out = {o for n in mx_nodes for o in n.output}
    want = {n.name for n in model.nodes if n.op_type in ("MatMul", "Gemm") and n.input[0] in mx_out and n.input[1] in mx_out}
    assert set(rep["nodes"]) == want and len(want) == 13
    _within(rep, config)
    meta, blob = _sections(out, config)
    keys = [v["constant"] for v in rep["nodes"].values() if v["constant"] is not None]
    assert sorted(keys) == sorted(meta["tensors"]) and len(keys) == 9
    assert json.load(open(out / "ocp_mx_blocks.json"))["format"] == config
    # the file's bytes are the model's bytes of the weights quant_model.onnx holds, under the scale bytes it holds for them
    inits = model.initializers
    scale_of = {n.input[0]: n.input[1] for n in mx_nodes if len(n.input) == 2}
    searched = "--mx_scale_search" in VIT[config]
    if searched:
        scale_rep = json.load(open(out / "mx_scale_report.json"))
        assert scale_rep["format"] == config and sorted(scale_rep["tensors"]) == sorted(meta["tensors"])
        assert all(v["err_chosen"] <= v["err_floor"] for v in scale_rep["tensors"].values())
        assert sorted(scale_of) == sorted({t["initializer"] for t in meta["tensors"].values()})
    else:
        assert scale_of == {}
    for key, t in meta["tensors"].items():
        w = np.asarray(inits[t["initializer"]], np.float32).reshape(t["shape"])
        given = np.asarray(inits[scale_of[t["initializer"]]], np.uint8) if searched else None
        wc, ws = F.encode(w, t["axis"], config, scales=given)
        c = blob[t["codes"]["offset"]:t["codes"]["offset"] + t["codes"]["nbytes"]].reshape(t["codes"]["shape"])
        s = blob[t["scales"]["offset"]:t["scales"]["offset"] + t["scales"]["nbytes"]].reshape(t["scales"]["shape"])
        assert np.array_equal(c, wc) and np.array_equal(s, ws), key
    if config == "mxfp6_e2m3":        # without --mx_verify: no report, and every other file byte for byte
        plain = vit_dir / (config + "_plain")
        _cli(vit_dir, "vit.onnx", plain, VIT[config])
        assert _files(out) - _files(plain) == {REPORT} and _files(plain) - _files(out) == set()
        for f in sorted(_files(plain) - {"log.txt"}):
            assert open(plain / f, "rb").read() == open(out / f, "rb").read(), f


def test_cli_block_scales_and_verifies_every_conv(resnet_dir):
    elem = "mxfp6_e2m3"
    out = resnet_dir / "conv"
    _cli(resnet_dir, "resnet.onnx", out, ["--mx", elem, "--mx_conv", "--mx_pack", "--mx_verify"])
    rep = json.load(open(out / REPORT))
    blocks = json.load(open(out / "ocp_mx_blocks.json"))
    assert rep["format"] == elem and rep["images"] == 8 and rep["skipped"] == {}
    convs = {k: v for k, v in rep["nodes"].items() if v["op"] == "Conv"}
    assert len(rep["nodes"]) == 21 and len(convs) == 20 and sorted(blocks["conv"]["nodes"]) == sorted(convs) and blocks["conv"]["left"] == {}
    _within(rep, "resnet " + elem)
    meta, _ = _sections(out, elem)
    for v in convs.values():
        t = meta["tensors"][v["constant"]]
        kh, kw = v["kernel"]
        assert t["codes"]["shape"] == [v["cout"], kh, kw, 24 * -(-v["c"] // 32)] and t["axis"] == 1
    assert {v["c"] for v in convs.values()} >= {3, 24, 48, 96, 192}
