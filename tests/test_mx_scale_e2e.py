"""GPU: `--mx_scale_search` through the CLI on the mini-ViT of tests/test_mx_verify_e2e.py, with the same images and
DPL_DETERMINISTIC=1.  The searched bytes travel explicitly: every MX node of quant_model.onnx that reads an initializer has a second
input, a uint8 initializer that equals the model's search (tests/mx_scale_model.py) on the weight of that same file, and every node
on an activation has one input; every section of ocp_mx_weights.bin decodes to the model's Q/DQ of that weight under those bytes
and carries them transposed; --mx_verify lists its 13 nodes, none skipped, each within the existing bound; mx_scale_report.json
never reports a larger error than the floor rule's.  The same command without the flag writes none of it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mx_pack_model as P
import mx_scale_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, IMG = 16, 32
CONFIGS = {"mxfp4": ["--mx", "mxfp4", "--mx_scale_search", "--mx_pack", "--mx_verify"],
           "mxfp8_rotate_smooth_bc": ["--mx", "mxfp8", "--mx_rotate", "--smooth", "--bc", "--mx_scale_search", "--mx_pack", "--mx_verify"]}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mxscale")
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


def _mx_nodes(path):
    from dipoorlet_amd import onnx_io
    model = onnx_io.load_model(str(path))
    return model, [n for n in model.nodes if n.op_type == "MXQuantizeDequantize"]


@pytest.mark.two_forwards
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_cli_carries_the_searched_scales_into_every_file(workdir, config):
    elem = CONFIGS[config][1]
    out = workdir / config
    _cli(workdir, out, CONFIGS[config])
    # quant_model.onnx
    model, nodes = _mx_nodes(out / "quant_model.onnx")
    on_const = [n for n in nodes if n.input[0] in model.initializers]
    assert len(nodes) == 26 and len(on_const) == 9
    searched = {}
    for n in nodes:
        if n not in on_const:
            assert len(n.input) == 1, n.name
            continue
        assert len(n.input) == 2 and n.input[1] in model.initializers, n.name
        w, b = model.initializers[n.input[0]], model.initializers[n.input[1]]
        axis = n.attrs["axis"] % w.ndim
        assert b.dtype == np.uint8 and b.shape == tuple(-(-d // 32) if i == axis else d for i, d in enumerate(w.shape)), n.name
        want = S.scale_search(w, axis, elem)[0]
        assert np.array_equal(b.reshape(-1), want.reshape(-1)), n.name
        searched[n.input[0]] = (n.input[1], w, axis, want)
    # ocp_mx_blocks.json
    blocks = json.load(open(out / "ocp_mx_blocks.json"))
    assert blocks["weight_scales"] == "search"
    for key, t in blocks["tensors"].items():
        assert ("scales" in t) == t["constant"], key
        if t["constant"]:
            assert t["scales"] == searched[key][0]
    # ocp_mx_weights.bin: every section decodes to the model's Q/DQ under those bytes and carries them transposed
    meta = json.load(open(out / "ocp_mx_weights.json"))
    blob = np.fromfile(out / "ocp_mx_weights.bin", dtype=np.uint8)
    assert sorted(meta["tensors"]) == sorted(searched)
    for key, t in meta["tensors"].items():
        _, w, axis, s = searched[t["initializer"]]
        codes = blob[t["codes"]["offset"]:t["codes"]["offset"] + t["codes"]["nbytes"]].reshape(t["codes"]["shape"])
        packed = blob[t["scales"]["offset"]:t["scales"]["offset"] + t["scales"]["nbytes"]].reshape(t["scales"]["shape"])
        want_y, eff = S.fake_quant_mx_scaled(w, axis, elem, s, return_scales=True)
        got_y = P.decode(codes, packed, elem, w.shape, axis)
        assert not np.isnan(want_y).any() and np.array_equal(got_y.view(np.uint32), want_y.view(np.uint32)), key
        assert np.array_equal(packed.reshape(-1), eff.transpose(0, 2, 1).reshape(-1)) and np.array_equal(eff.reshape(-1), s.reshape(-1)), key
        want_c, want_p = S.encode_scaled(w, axis, elem, s)
        assert np.array_equal(codes, want_c) and np.array_equal(packed, want_p), key
    # mx_verify_report.json: the constant operand from the file, the node's own output under the same bytes
    rep = json.load(open(out / "mx_verify_report.json"))
    assert rep["format"] == elem and rep["skipped"] == {} and len(rep["nodes"]) == 13
    for name, v in rep["nodes"].items():
        print(f"{config} {name}: {v['max_err_over_bound']:.4g} of the bound, 1 - cosine {1 - v['cosine']:.2e}")
        assert v["within_bound"] is True and v["max_err_over_bound"] <= 1.0 and v["cosine"] >= 1 - 1e-6, (name, v)
    # mx_scale_report.json
    report = json.load(open(out / "mx_scale_report.json"))
    assert report["format"] == elem and sorted(report["tensors"]) == sorted(searched)
    for key, t in report["tensors"].items():
        _, w, axis, s = searched[key]
        floor = S.floor_scales(w, axis, elem)
        print(f"{config} {key}: {t['moved_up']} of {t['blocks']} blocks moved up, squared error {t['err_chosen']:.6g} / {t['err_floor']:.6g} "
              f"= {t['err_chosen'] / t['err_floor']:.4f}")
        assert t["blocks"] == s.size and t["moved_up"] == int((s != floor).sum())
        assert t["err_chosen"] <= t["err_floor"], key
        err = S.scale_search(w, axis, elem)[1]
        # (sums of the kernel's exact per-block errors: only the order of the final fp64 additions is the device's own)
        assert np.isclose(t["err_floor"], err[..., 0].sum(), rtol=1e-12) and np.isclose(t["err_chosen"], err[..., 1].sum(), rtol=1e-12)
    assert any(t["moved_up"] > 0 for t in report["tensors"].values())
    if config == "mxfp4":        # the same command without the flag
        plain = workdir / (config + "_plain")
        _cli(workdir, plain, [a for a in CONFIGS[config] if a != "--mx_scale_search"])
        assert not os.path.exists(plain / "mx_scale_report.json")
        assert "weight_scales" not in json.load(open(plain / "ocp_mx_blocks.json"))
        assert not any("scales" in t for t in json.load(open(plain / "ocp_mx_blocks.json"))["tensors"].values())
        pm, pn = _mx_nodes(plain / "quant_model.onnx")
        assert len(pn) == 26 and all(len(n.input) == 1 for n in pn)
        assert not any(k.endswith("_scale") and v.dtype == np.uint8 and k[:-len("_scale")] in searched for k, v in pm.initializers.items())
        assert open(plain / "act_clip_val.json", "rb").read() == open(out / "act_clip_val.json", "rb").read()
