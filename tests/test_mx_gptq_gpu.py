"""GPU: the MX GPTQ kernel (csrc/gptq_kernels.hip k_gptq_mx_block, dpl_gptq_mx_block) against its numpy definition
(mx_gptq_model.py).

One call has no floating-point reduction in it (the block maximum is an integer maximum of bit patterns), so the kernel is held to
mx_gptq_model.gptq_mx_block BIT FOR BIT — W, Err and the E8M0 bytes — and the columns outside the call must come back untouched.  A
whole layer (ops.gptq_mx_quantize) adds one fp32 GEMM between calls, whose summation order is the BLAS library's: a single-call
layer is still exact; the others must be a fixed point of ops.fake_quant_mx on the device, within the caps test_gptq_gpu.py holds
its layers to against the fp64 model (at most 1 % of the elements, objective at most 1.02 x) and at most 0.5 % of the elements away
from the numpy fp32 path."""
import ctypes as ct

import numpy as np
import pytest
import torch

import mx_gptq_cases as C
import mx_gptq_model as G

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 64)                    # fewer than, and no multiple of, the 4 rows of a workgroup; several workgroups
CALLS = ((0, 128, 256), (128, 128, 256), (64, 32, 288), (256, 32, 288), (64, 8, 72))      # (c0, nb, K): the last one a short last block


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def factor_u():
    """U fp32 [300, 300] of the 48 x 300 case (a singular Hessian under damping: entries of very different sizes)."""
    return np.ascontiguousarray(C.draw(C.LAYER_CASES[1])[2], np.float32)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("elem", C.ELEMS)
def test_call_is_the_model_bit_for_bit(elem, rows, factor_u):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(200 + rows)
    for c0, nb, K in CALLS:
        # magnitudes that differ from block to block and row to row: several shared exponents per call
        W = (0.05 * rng.standard_normal((rows, K)) * np.exp2(rng.integers(-6, 7, (rows, -(-K // 32))).repeat(32, axis=1)[:, :K])).astype(np.float32)
        U = np.ascontiguousarray(factor_u[:K, :K])
        want = W.copy()
        want_err, want_s = G.gptq_mx_block(want, U, c0, nb, elem, K)
        w, u = torch.from_numpy(W).to(dev), torch.from_numpy(U).to(dev)
        scales = torch.full((rows, -(-K // 32)), 0xAB, dtype=torch.uint8, device=dev)
        err, s = ops.gptq_mx_block(w, c0, nb, u, elem, scales=scales)
        got, got_err, got_s = w.cpu().numpy(), err.cpu().numpy(), s.cpu().numpy()
        assert _same(got, want), (c0, nb, K)                                              # the columns outside the call included
        assert _same(got_err, want_err), (c0, nb, K)
        b0, b1 = c0 // 32, c0 // 32 + -(-nb // 32)
        assert np.array_equal(got_s[:, b0:b1], want_s), (c0, nb, K)
        assert (got_s[:, :b0] == 0xAB).all() and (got_s[:, b1:] == 0xAB).all()            # ... and the bytes of other blocks
        assert np.array_equal(_bits(got[:, :c0]), _bits(W[:, :c0])) and np.array_equal(_bits(got[:, c0 + nb:]), _bits(W[:, c0 + nb:]))


@pytest.mark.parametrize("elem", C.ELEMS)
@pytest.mark.parametrize("name", C.CONSTRUCTED)
def test_constructed_blocks_are_the_model_bit_for_bit(name, elem):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    W, U = C.constructed(name, elem)
    want = W.copy()
    want_err, want_s = G.gptq_mx_block(want, U, 0, 32, elem, 32)
    w = torch.from_numpy(W).to(dev)
    err, s = ops.gptq_mx_block(w, 0, 32, torch.from_numpy(U).to(dev), elem)
    assert _same(w.cpu().numpy(), want) and _same(err.cpu().numpy(), want_err) and np.array_equal(s.cpu().numpy(), want_s)
    assert np.array_equal(_bits(ops.fake_quant_mx(w, 1, elem).cpu().numpy()), _bits(want))        # the fixed point, on the device


def test_refused_calls_return_minus_two_and_touch_nothing(factor_u):
    from dipoorlet_amd import _hip
    dev = torch.device("cuda:0")
    rows, K = 5, 300
    W = (0.05 * np.random.default_rng(3).standard_normal((rows, K))).astype(np.float32)
    w, u = torch.from_numpy(W).to(dev), torch.from_numpy(factor_u).to(dev)
    err = torch.full((rows, 128), 7.0, device=dev)
    scales = torch.full((rows, 10), 0xAB, dtype=torch.uint8, device=dev)
    L = _hip.lib()
    P = lambda t: None if t is None else ct.c_void_p(t.data_ptr())     # noqa: E731

    def call(elem=_hip.MX_E2M1, w_=w, rows_=rows, ldw=K, k=K, c0=0, nb=64, u_=u, ldu=K, err_=err, scales_=scales, lds=10):
        return L.dpl_gptq_mx_block(elem, P(w_), rows_, ldw, k, c0, nb, P(u_), ldu, P(err_), P(scales_), lds, None)

    bad = [dict(elem=2), dict(elem=-1), dict(w_=None), dict(u_=None), dict(err_=None), dict(scales_=None), dict(nb=0), dict(nb=129), dict(nb=-32),
           dict(c0=16), dict(c0=-32), dict(nb=48), dict(c0=256, nb=40), dict(k=K + 1), dict(c0=288, nb=32), dict(c0=256, nb=64),
           dict(ldu=100, c0=64), dict(lds=9), dict(rows_=2 ** 31), dict(k=0, nb=1)]
    for kw in bad:
        assert call(**kw) == -2, kw
        assert b"dpl_gptq_mx_block" in L.dpl_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(W)) and bool((err == 7.0).all()) and bool((scales == 0xAB).all())
    assert call(rows_=0) == 0                                           # nothing to do: not an error, nothing launched
    torch.cuda.synchronize()
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(W)) and bool((scales == 0xAB).all())
    assert call(c0=288, nb=12) == 0 and call(elem=_hip.MX_E4M3, c0=0, nb=32) == 0      # a short last block; the other element format
    torch.cuda.synchronize()
    got = w.cpu().numpy()
    assert not np.array_equal(_bits(got[:, 288:]), _bits(W[:, 288:])) and not np.array_equal(_bits(got[:, :32]), _bits(W[:, :32]))
    assert np.array_equal(_bits(got[:, 32:288]), _bits(W[:, 32:288]))


@pytest.mark.parametrize("elem", C.ELEMS)
def test_a_non_finite_block_is_a_nan_block(elem, factor_u):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    W = (0.05 * np.random.default_rng(4).standard_normal((3, 64))).astype(np.float32)
    W[0, 40], W[1, 33] = np.inf, np.nan
    U = np.eye(64, dtype=np.float32)                                    # (nothing of block 0 reaches block 1)
    U[:32, :32] = factor_u[:32, :32]
    w = torch.from_numpy(W).to(dev)
    _, s = ops.gptq_mx_block(w, 0, 64, torch.from_numpy(U).to(dev), elem)
    got, s = w.cpu().numpy(), s.cpu().numpy()
    assert (s[:2, 1] == 0xFF).all() and np.isnan(got[:2, 32:]).all()
    assert (s[:, 0] != 0xFF).all() and s[2, 1] != 0xFF and np.isfinite(got[2]).all() and np.isfinite(got[:, :32]).all()
    with pytest.raises(Exception):
        ops.gptq_mx_quantize(torch.from_numpy(W).to(dev), torch.from_numpy(U).to(dev), elem)


@pytest.mark.parametrize("elem", C.ELEMS)
def test_a_single_call_layer_is_the_model_exactly(elem):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    d = C.build(C.SINGLE_CALL, elem)
    w = torch.from_numpy(d["W"].copy()).to(dev)
    wq, err, s = ops.gptq_mx_quantize(w, torch.from_numpy(np.ascontiguousarray(d["U"], np.float32)).to(dev), elem)
    assert _same(wq.cpu().numpy(), d["W32"]) and _same(err.cpu().numpy(), d["E32"]) and np.array_equal(s.cpu().numpy(), d["S32"])
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(d["W"]))        # the input is not modified


@pytest.mark.parametrize("elem", C.ELEMS)
@pytest.mark.parametrize("case", C.LAYER_CASES, ids=C.case_id)
def test_layer_is_a_fixed_point_and_within_the_caps(case, elem):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    d = C.build(case, elem)
    w = torch.from_numpy(d["W"].copy()).to(dev)
    u = torch.from_numpy(np.ascontiguousarray(d["U"], np.float32)).to(dev)
    o64 = G.objective(d["W64"], d["W"], d["H"])
    for block in (128, 32):
        wq_d, err, s = ops.gptq_mx_quantize(w, u, elem, block=block)
        assert torch.equal(ops.fake_quant_mx(wq_d, 1, elem).view(torch.int32), wq_d.view(torch.int32))      # the graph's node leaves it alone
        wq = wq_d.cpu().numpy()
        assert err.shape == wq.shape == d["W"].shape and tuple(s.shape) == d["S32"].shape
        o_dev = G.objective(wq, d["W"], d["H"])
        s64, s32 = float(np.mean(_bits(wq) != _bits(d["W64"]))), float(np.mean(_bits(wq) != _bits(d["W32"])))
        print(f"{C.case_id(case)} {elem} block {block}: device vs fp64 model {100 * s64:.4f} % differ, objective x {o_dev / o64:.5f}; "
              f"vs numpy fp32 (block 128) {100 * s32:.4f} % differ")
        assert s64 <= 0.01 and o_dev <= 1.02 * o64
        if block == 128:
            assert s32 <= 0.005
            assert np.array_equal(_bits(wq[:, :128]), _bits(d["W32"][:, :128]))          # no GEMM in front of the first call: exact
            assert np.array_equal(s.cpu().numpy()[:, :4], d["S32"][:, :4])
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(d["W"]))                          # the input is not modified
    for bad in (0, 16, 48, 160):
        with pytest.raises(Exception):
            ops.gptq_mx_quantize(w, u, elem, block=bad)


def test_the_torch_op(factor_u):
    import dipoorlet_amd.torch_ops  # noqa: F401  (registers torch.ops.dipoorlet.*)
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    w = torch.from_numpy(C.draw(C.LAYER_CASES[1])[0].copy()).to(dev)
    u = torch.from_numpy(factor_u).to(dev)
    for elem, c0, nb in (("mxfp4", 128, 96), ("mxfp8", 288, 12)):
        a, b = w.clone(), w.clone()
        ea, sa = ops.gptq_mx_block(a, c0, nb, u, elem)
        eb, sb = torch.ops.dipoorlet.gptq_mx_block(b, c0, nb, u, elem)
        assert torch.equal(a, b) and torch.equal(ea, eb) and torch.equal(sa, sb) and not torch.equal(a, w)
