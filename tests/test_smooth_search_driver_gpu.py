"""GPU: `--smooth --smooth_search --mx mxfp4` through smooth_quant on the mini-ViT with one planted LayerNorm outlier channel, 4 images:
the report's choice is the argmin of its own errors under the tie rule, smooth_model.onnx is apply_smooth of the reported choices, a
second run writes the same files.  Nothing is asserted about which strength wins."""
import json
import os
import types

import numpy as np
import pytest

import smooth_model as M
from dipoorlet_amd.weight_transform.smooth import SEARCH_ALPHAS, apply_smooth, find_smooth_sites, smooth_quant, smooth_statistics

pytestmark = pytest.mark.gpu
N, IMG = 4, 32


def test_report_choice_model_and_repeat(tmp_path):
    from dipoorlet_amd.graph import ONNXGraph
    plain = M.mini_vit()
    g = M.plant_outliers(plain, find_smooth_sites(plain), channels=(17,))
    os.makedirs(tmp_path / "calib" / "input")
    rng = np.random.default_rng(9)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(str(tmp_path / "calib" / "input" / f"{i}.bin"))
    files = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        os.makedirs(out)
        args = types.SimpleNamespace(input_dir=str(tmp_path / "calib"), data_num=N, rank=0, local_rank=0, world_size=1, calib_batch=4,
                                     output_dir=str(out), smooth_alpha=0.5, smooth=True, smooth_search=True, mx="mxfp4", deploy="ocp_fp8")
        smooth_quant(g, args)
        with open(out / "smooth_search_report.json", "rb") as f:
            files.append((f.read(), open(out / "smooth_model.onnx", "rb").read()))
    assert files[0] == files[1]
    report = json.loads(files[0][0])
    sites = find_smooth_sites(g)
    assert report["format"] == "mxfp4" and report["images"] == N and len(report["candidates"]) == len(SEARCH_ALPHAS) == 12
    chosen = {}
    for e, s in zip(report["sites"], sites):
        assert len(e["E"]) == 12 and (e["gamma"], e["channels"], e["readers"]) == (s.gamma, s.channels, [r.node for r in s.readers])
        finite = [v for v in e["E"] if v is not None]                    # (a NaN is null in the file)
        assert finite and e["chosen"] == e["E"].index(min(finite)) and e["alpha"] == SEARCH_ALPHAS[e["chosen"]]
        chosen[s.tensor] = e["alpha"]
    want, _ = apply_smooth(g, sites, smooth_statistics(g, sites, args), chosen)
    written = ONNXGraph.load(str(tmp_path / "run1" / "smooth_model.onnx"), str(tmp_path), "ocp_fp8", None)
    for name, v in want.initializer.items():
        assert np.asarray(written.get_initializer(name)).tobytes() == np.asarray(want.get_initializer(name)).tobytes(), name
