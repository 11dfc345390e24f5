"""What --smooth_search buys end to end, recorded and not asserted: the mini-ViT of DESIGN.md 3u (patch 8, dim 64, depth 2, heads 2,
mlp 128; one fc2 weight with four input rows scaled by 64; 16 images, -A hist, --calib_batch 8) through the CLI under
`--mx mxfp4`, `--mx mxfp4 --smooth` and `--mx mxfp4 --smooth --smooth_search`, and the cosine of each fake-quantised network's logits
against the fp32 network's over the 16 images.  A second model adds what --smooth is for — outlier channels in every LayerNorm
site (g_j, b_j * 16 and the readers' rows j / 16 on four channels: the same function) — and goes through the same three runs.

    python scripts/mx_smooth_cosine.py WORKDIR [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dipoorlet_amd import models  # noqa: E402
from dipoorlet_amd.forward_net import load_input_batch  # noqa: E402
from dipoorlet_amd.graph import ONNXGraph  # noqa: E402
from dipoorlet_amd.quantize import quant_graph  # noqa: E402
from dipoorlet_amd.utils import load_clip_val  # noqa: E402
from dipoorlet_amd.weight_transform.smooth import find_smooth_sites  # noqa: E402
from dipoorlet_amd.weight_transform.utils import update_weight  # noqa: E402

N, IMG = 16, 32
RUNS = (("--mx mxfp4", []), ("--mx mxfp4 --smooth", ["--smooth"]), ("--mx mxfp4 --smooth --smooth_search", ["--smooth", "--smooth_search"]))


def build(with_site_outliers):
    g = models.vit(image=IMG, patch=8, dim=64, depth=2, heads=2, mlp=128, num_classes=10)
    w = np.array(g.get_initializer("blocks.1.mlp.fc2.weight"), np.float32)
    w[[3, 40, 77, 114]] *= 64.0
    update_weight(g, w, "blocks.1.mlp.fc2.weight")
    if with_site_outliers:
        ch = [3, 17, 30, 61]
        for site in find_smooth_sites(g):
            for name in (site.gamma, site.beta):
                v = np.array(g.get_initializer(name), np.float32)
                v.reshape(-1)[ch] *= 16.0
                update_weight(g, v, name)
            for r in site.readers:
                v = np.array(g.get_initializer(r.weight), np.float32)
                if r.transposed:
                    v[:, ch] /= 16.0
                else:
                    v[ch, :] /= 16.0
                update_weight(g, v, r.weight)
    g.update_model()
    return g


def cosine(model, calib, out, smoothed):
    """Cosine of the logits of the fake-quantised network of run `out` against the fp32 `model`'s over the N images."""
    args = types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx="mxfp4", output_dir=out)
    act, wt = load_clip_val(args)
    g = ONNXGraph.load(model)
    gs = ONNXGraph.load(os.path.join(out, "smooth_model.onnx")) if smoothed else g
    gq, _ = quant_graph(gs, {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**act, **wt}.items()}, args)
    inp = load_input_batch(calib, g.network_inputs, {"input": g.get_tensor_shape("input")}, 0, N, torch.device("cuda:0"))
    fp = g.make_session().run_named(inp, [g.network_outputs[0]])[0].double().reshape(-1)
    q = gq.make_session().run_named(inp, [gq.network_outputs[0]])[0].double().reshape(-1)
    return float((fp * q).sum() / (fp.norm() * q.norm()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workdir")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_smooth_cosine needs the GPU: nothing is measured without one")
    calib = os.path.join(a.workdir, "calib")
    os.makedirs(os.path.join(calib, "input"), exist_ok=True)
    rng = np.random.default_rng(12)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(os.path.join(calib, "input", f"{i}.bin"))
    env = dict(os.environ, DPL_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    result = {}
    for tag, outliers in (("weight outliers", False), ("weight and LayerNorm outliers", True)):
        d = os.path.join(a.workdir, "sites" if outliers else "plain")
        os.makedirs(d, exist_ok=True)
        g = build(outliers)
        g.output_dir = d
        g.save_onnx_model("vit")
        model = os.path.join(d, "vit.onnx")
        for k, (name, extra) in enumerate(RUNS):
            out = os.path.join(d, f"run{k}")
            cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", model, "-I", calib, "-N", str(N), "-A", "hist",
                   "-D", "ocp_fp8", "-O", out, "--calib_batch", "8", "--skip_profiling", "--mx", "mxfp4", *extra]
            r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:      # (nothing more is started after a run that failed)
                raise SystemExit(f"{name}: exit {r.returncode}\n{r.stdout[-3000:]}")
            entry = {"cosine": cosine(model, calib, out, bool(extra))}
            if "--smooth_search" in extra:
                with open(os.path.join(out, "smooth_search_report.json")) as f:
                    entry["chosen"] = {s["gamma"]: s["alpha"] for s in json.load(f)["sites"]}
            result.setdefault(tag, {})[name] = entry
            print(f"{tag}: {name}: logits against fp32, cosine {entry['cosine']:.4f}" + (f"  chosen {entry['chosen']}" if "chosen" in entry else ""),
                  flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
