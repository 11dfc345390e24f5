"""GPU: `--mx_pack` through the CLI on the mini-ViT of tests/test_mx_gpu.py, under DPL_DETERMINISTIC=1.  ocp_mx_weights.bin /
.json hold exactly the constant operands of ocp_mx_blocks.json, and every tensor's sections, decoded by the numpy model
(tests/mx_pack_model.py), are mx_model.fake_quant_mx of the initializer quant_model.onnx holds — the weights after --smooth,
--mx_rotate and --bc —, bit for bit.  The same command without --mx_pack writes neither file and every other file byte for byte
(log.txt apart: it records the run's wall-clock seconds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mx_model as M
import mx_pack_model as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, IMG = 16, 32
NEW = {"ocp_mx_weights.bin", "ocp_mx_weights.json"}
CONFIGS = {"mxfp4": ["--mx", "mxfp4"], "mxfp8_rotate_smooth_bc": ["--mx", "mxfp8", "--mx_rotate", "--smooth", "--bc"]}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mxpack")
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


def _files(d):
    return {os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs}


@pytest.mark.two_forwards
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_cli_writes_the_weights_of_quant_model_as_codes(workdir, config):
    from dipoorlet_amd import onnx_io
    elem = CONFIGS[config][1]
    packed, plain = workdir / (config + "_pack"), workdir / (config + "_plain")
    _cli(workdir, packed, CONFIGS[config] + ["--mx_pack"])
    meta = json.load(open(packed / "ocp_mx_weights.json"))
    blocks = json.load(open(packed / "ocp_mx_blocks.json"))
    assert (meta["format"], meta["block_size"], meta["layout"]) == (elem, 32, "k_innermost")
    assert set(meta["tensors"]) == {k for k, v in blocks["tensors"].items() if v["constant"]} and len(meta["tensors"]) == 9
    blob = open(packed / "ocp_mx_weights.bin", "rb").read()
    inits = onnx_io.load_model(str(packed / "quant_model.onnx")).initializers
    used = np.zeros(len(blob), bool)
    for key, t in meta["tensors"].items():
        w = np.asarray(inits[t["initializer"]], np.float32)
        assert key.startswith(t["initializer"]) and list(w.shape) == t["shape"] and t["axis"] == blocks["tensors"][key]["axis"]
        assert t["k"] == w.shape[t["axis"]] and t["k_padded"] == 32 * -(-t["k"] // 32)
        cs, ss = P.packed_shapes(w.shape, t["axis"], elem)
        arr = {}
        for name, shape in (("codes", cs), ("scales", ss)):
            sec = t[name]
            assert sec["offset"] % 64 == 0 and sec["shape"] == list(shape) and sec["nbytes"] == int(np.prod(shape))
            assert not used[sec["offset"]:sec["offset"] + sec["nbytes"]].any()
            used[sec["offset"]:sec["offset"] + sec["nbytes"]] = True
            arr[name] = np.frombuffer(blob, np.uint8, sec["nbytes"], sec["offset"]).reshape(shape)
        want_c, want_s = P.encode(w, t["axis"], elem)
        assert np.array_equal(arr["codes"], want_c) and np.array_equal(arr["scales"], want_s), key
        got, want = P.decode(arr["codes"], arr["scales"], elem, w.shape, t["axis"]), M.fake_quant_mx(w, t["axis"], elem)
        assert not np.isnan(want).any() and np.array_equal(got.view(np.uint32), want.view(np.uint32)), key
    assert not np.frombuffer(blob, np.uint8)[~used].any()                             # zero fill between the sections, none behind
    assert len(blob) == max(t[n]["offset"] + t[n]["nbytes"] for t in meta["tensors"].values() for n in ("codes", "scales"))
    if "--mx_rotate" in CONFIGS[config]:        # (the folded weights are what was encoded: they differ from the model's own)
        orig = onnx_io.load_model(str(workdir / "vit.onnx")).initializers
        assert any(not np.array_equal(np.asarray(inits[k]), np.asarray(orig[k])) for k in blocks["rotation"]["weights"])
    # without --mx_pack: neither file, and every other file byte for byte
    _cli(workdir, plain, CONFIGS[config])
    assert _files(packed) - _files(plain) == NEW and _files(plain) - _files(packed) == set()
    for f in sorted(_files(plain) - {"log.txt"}):
        assert open(plain / f, "rb").read() == open(packed / f, "rb").read(), f
