"""GPU: ops.gptq_factor / dpl_gptq_factor (csrc/gptq_factor_kernels.hip) against tests/gptq_model.py factor, numpy fp64.  The residual
r(U) = max |U H' U^T - I| (H' the damped matrix, products in np.longdouble) is held to r(device) <= 4 * max(r(model), K * 2^-52): both
routes are backward-stable in one unit round-off and differ in summation order (measured on the MI355X, DESIGN.md 3w: 0.16 .. 1.26 of
the model's); 4 leaves room for the blocked order, the floor keeps a lucky reference from setting the bar."""
import ctypes as ct
import functools
import warnings

import numpy as np
import pytest
import torch

import gptq_cases as C
import gptq_model as M
from test_gptq_gpu import _bits, _dev_grid

pytestmark = pytest.mark.gpu

XTX_K = (1, 2, 63, 64, 65, 129)      # one block, the block edge, a one-row last block, three block steps
H_IDS = [C.case_id(c) for c in C.ALL_CASES] + [f"xtx-{k}" for k in XTX_K] + ["dead-200"]


@functools.lru_cache(maxsize=None)
def _hessian(hid):
    """-> (H fp64 [K, K], read-only; the model's (U, damp) on it)."""
    if hid.startswith("xtx-") or hid == "dead-200":
        K = int(hid.split("-")[1])
        X = np.random.default_rng(1000 + K).standard_normal((4 * K, K))
        if hid == "dead-200":
            X[:, [3, 77, 199]] = 0.0
        H = X.T @ X / (4 * K)
    else:
        H = np.array(C.build(C.ALL_CASES[H_IDS.index(hid)])["H"])
    H.setflags(write=False)
    return H, M.factor(H, 0.01)


def _damped(H, damp):
    Hd = np.array(H, np.float64)
    d = np.arange(len(Hd))
    Hd[d, d] = np.where(Hd[d, d] == 0, 1.0, Hd[d, d])
    Hd[d, d] += damp * float(np.mean(Hd[d, d]))
    return Hd


def _residual(U, Hd):
    U = np.asarray(U, np.longdouble)
    return float(np.abs(U @ Hd.astype(np.longdouble) @ U.T - np.eye(len(Hd))).max())


def _device_factor(H, damp=0.01):
    from dipoorlet_amd import ops
    U, used = ops.gptq_factor(torch.from_numpy(np.array(H)).to("cuda:0"), damp)
    return (None if U is None else U.cpu().numpy()), used


@pytest.mark.parametrize("hid", H_IDS)
def test_factor_against_the_model(hid):
    H, (Um, damp_m) = _hessian(hid)
    U, damp = _device_factor(H)
    assert U is not None and damp == damp_m
    K = len(H)
    assert np.all(np.tril(U, -1) == 0.0) and np.all(np.diag(U) > 0.0)
    Hd = _damped(H, damp)
    r_dev, r_model, bound = _residual(U, Hd), _residual(Um, Hd), 4 * max(_residual(Um, Hd), K * 2.0 ** -52)
    print(f"{hid}: residual device {r_dev:.3e} model {r_model:.3e} ratio {r_dev / r_model:.3f}, {r_dev / bound:.3f} of the bound")
    assert r_dev <= bound


@pytest.mark.parametrize("name", ["retry", "minus_identity", "nan"])
def test_retry_and_failure_follow_the_model(name):
    H = {"retry": np.diag(np.r_[np.ones(64), -0.05]),       # fails at damp 0.01 (the last pivot is -0.05 + 0.01 * mean), not at 0.1
         "minus_identity": -np.eye(64), "nan": np.array(_hessian("xtx-65")[0])}[name]
    if name == "nan":
        H[40, 7] = H[7, 40] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the model warns when it gives up)
        Um, damp_m = M.factor(H, 0.01)
    U, damp = _device_factor(H)
    assert (U is None) == (Um is None) == (name != "retry") and damp == damp_m
    if name == "retry":
        Hd = _damped(H, damp)
        assert damp > 0.01 and _residual(U, Hd) <= 4 * max(_residual(Um, Hd), 65 * 2.0 ** -52)


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(300)
    X = rng.standard_normal((1200, 300)) @ (np.eye(300) + 0.05 * rng.standard_normal((300, 300)))
    H = X.T @ X / 1200
    (U1, _), (U2, _) = _device_factor(H), _device_factor(H)
    assert torch.equal(torch.from_numpy(U1), torch.from_numpy(U2))


@pytest.mark.parametrize("case", C.LAYER_CASES, ids=C.case_id)
def test_gptq_on_the_device_factor_stays_within_the_model_caps(case):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    d = C.build(case)
    U, _ = ops.gptq_factor(torch.from_numpy(np.array(d["H"])).to(dev), 0.01)
    wq, _ = ops.gptq_quantize(torch.from_numpy(d["W"].copy()).to(dev), U.to(torch.float32).contiguous(), _dev_grid(d["grid"], dev))
    wq = wq.cpu().numpy()
    differ = float(np.mean(_bits(wq) != _bits(d["W32"])))
    o_dev, o_model = M.objective(wq, d["W"], d["H"]), M.objective(d["W32"], d["W"], d["H"])
    print(f"{C.case_id(case)}: {100 * differ:.4f} % of the weights differ from gptq_layer32's, objective x {o_dev / o_model:.5f}")
    assert differ <= 0.01 and o_dev <= 1.02 * o_model


@pytest.mark.parametrize("what", ["null_h", "null_u", "null_status", "null_workspace", "k_zero", "k_too_large", "damp_zero", "damp_negative",
                                  "damp_nan", "workspace_small"])
def test_refused_calls_launch_nothing(what):
    from dipoorlet_amd import _hip
    dev, K = torch.device("cuda:0"), 65
    lib = _hip.lib()
    nbytes = int(lib.dpl_gptq_factor_workspace(K))
    assert nbytes == (2 * 128 * 128 + 128 * 64) * 8 and lib.dpl_gptq_factor_workspace(0) == 0
    assert lib.dpl_gptq_factor_workspace(_hip.GPTQ_FACTOR_MAX_K) > 0 and lib.dpl_gptq_factor_workspace(_hip.GPTQ_FACTOR_MAX_K + 1) == 0
    H = torch.eye(K, dtype=torch.float64, device=dev)
    U = torch.full((K, K), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), 123, dtype=torch.int32, device=dev)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    a = dict(h=H.data_ptr(), k=K, damp=0.01, u=U.data_ptr(), status=status.data_ptr(), ws=ws.data_ptr(), nbytes=nbytes)
    a.update({"null_h": dict(h=None), "null_u": dict(u=None), "null_status": dict(status=None), "null_workspace": dict(ws=None),
              "k_zero": dict(k=0), "k_too_large": dict(k=_hip.GPTQ_FACTOR_MAX_K + 1), "damp_zero": dict(damp=0.0),
              "damp_negative": dict(damp=-0.01), "damp_nan": dict(damp=float("nan")), "workspace_small": dict(nbytes=nbytes - 1)}[what])
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dpl_gptq_factor(a["h"], a["k"], a["damp"], a["u"], a["status"], a["ws"], a["nbytes"], stream) == -2
    assert b"dpl_gptq_factor" in lib.dpl_last_error()
    torch.cuda.synchronize()
    assert bool((U == 7.0).all()) and int(status.item()) == 123 and not bool(ws.any())
