"""GPU: --gptq --gptq_factor device end to end on the small ResNet-18 of test_gptq_e2e.py (its work directory, its CLI call, its
checks), -D ocp_fp8: every layer is rounded by GPTQ on a U the device factorised, no layer's objective is more than 1.02 x what the
same process reaches with the host factorisation (the cap tests/test_gptq_model.py holds the fp32 path to against fp64), and the
network's output error stays below round-to-nearest's."""
import json
import types

import pytest

from test_gptq_e2e import _check_weights, _cli, _network_error, workdir  # noqa: F401  (workdir: the module's fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]


def test_gptq_cli_with_the_device_factorisation(workdir):  # noqa: F811
    from dipoorlet_amd.utils import load_clip_val
    out_host, out = workdir / "out_factor_host", workdir / "out_factor_device"
    assert _cli(workdir, out_host, "ocp_fp8", ["--gptq"]) == 0
    assert _cli(workdir, out, "ocp_fp8", ["--gptq", "--gptq_factor", "device"]) == 0
    host, report = json.load(open(out_host / "gptq_report.json")), json.load(open(out / "gptq_report.json"))
    assert "factor" not in host and report["factor"] == "device"
    assert len(report["layers"]) == len(host["layers"]) == 21 and report["left"] == []
    for e, h in zip(report["layers"], host["layers"]):
        assert e["node"] == h["node"] and e["kept"] == "gptq" and e["damp"] == h["damp"], e
        assert e["objective_gptq"] <= 1.02 * h["objective_gptq"], (e, h)
    args = types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], output_dir=str(out))
    act, wt = load_clip_val(args)
    assert _check_weights(str(out / "gptq.onnx"), workdir, wt, "ocp_fp8") > 100
    err_nearest = _network_error(str(workdir / "model.onnx"), workdir, act, wt, args)
    err_gptq = _network_error(str(out / "gptq.onnx"), workdir, act, wt, args)
    print(f"device factor: gptq / nearest output error {err_gptq / err_nearest:.4f}; layer objectives device / host "
          f"{sum(e['objective_gptq'] for e in report['layers']) / sum(h['objective_gptq'] for h in host['layers']):.6f}")
    assert err_gptq < 1.0 * err_nearest, (err_gptq, err_nearest)
