"""GPU: the GPTQ kernel (csrc/gptq_kernels.hip, dpl_gptq_block) against its numpy definition (gptq_model.py).

One block has no reduction in it, so the kernel is held to gptq_model.gptq_block BIT FOR BIT, the error matrix included, and the
columns outside the block must come back untouched.  A whole layer (ops.gptq_quantize) adds one fp32 GEMM between blocks, whose
summation order is the BLAS library's: a single-block layer is still exact; the others must be on the grid, within the caps
test_gptq_model.py asserts for the numpy fp32 path against the fp64 model (at most 1 % of the elements, objective at most 1.02 x),
and at most 0.5 % of the elements away from the numpy fp32 path."""
import ctypes as ct

import numpy as np
import pytest
import torch

import gptq_cases as C
import gptq_model as M

pytestmark = pytest.mark.gpu

K = 300
NBS = (1, 2, 63, 64, 65, 128)       # around one column per lane / two columns per lane
ROWS = (1, 3, 5, 64)                # fewer than, and no multiple of, the rows of a workgroup; several workgroups


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev_grid(grid, dev):
    from dipoorlet_amd import ops
    scale = torch.from_numpy(np.asarray(grid["scale"], np.float32)).to(dev)
    if grid["fmt"] == M.E4M3:
        return ops.GptqGrid("e4m3", scale)
    return ops.GptqGrid("int", scale, torch.from_numpy(np.asarray(grid["zp"], np.int32)).to(dev), grid["qlo"], grid["qhi"])


def _block_grid(W, kind):
    if kind == "int4_per_tensor":
        return {"fmt": M.INT, "scale": np.array([np.abs(W).max() / np.float32(7)], np.float32), "zp": np.zeros(1, np.int32), "qlo": -7, "qhi": 7}
    if kind == "uint4_per_channel":      # a zero point per row
        a = np.abs(W).max(axis=1).astype(np.float32)
        return {"fmt": M.INT, "scale": (a / np.float32(7)).astype(np.float32), "zp": (np.arange(len(a)) % 5 + 2).astype(np.int32), "qlo": 0, "qhi": 15}
    return C.make_grid(W, kind)


@pytest.fixture(scope="module")
def factor_u():
    """U fp32 [300, 300] of the 48 x 300 case (a singular Hessian under damping: entries of very different sizes)."""
    return np.ascontiguousarray(C.build(C.LAYER_CASES[2])["U"], np.float32)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kind", ["int4", "int4_per_tensor", "uint4", "uint4_per_channel", "e4m3"])
def test_block_is_the_model_bit_for_bit(kind, rows, factor_u):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(100 + rows)
    W = (0.05 * rng.standard_normal((rows, K))).astype(np.float32)
    grid = _block_grid(W, kind)
    Q, g = M.make_q(grid), _dev_grid(grid, dev)
    u = torch.from_numpy(factor_u).to(dev)
    for nb in NBS:
        for c0 in sorted({0, 128, K - nb}):
            want = W.copy()
            want_err = M.gptq_block(want, factor_u, c0, nb, Q)
            w = torch.from_numpy(W).to(dev)
            err = ops.gptq_block(w, c0, nb, u, g)
            got, got_err = w.cpu().numpy(), err.cpu().numpy()
            assert got_err.shape == (rows, nb)
            assert np.array_equal(_bits(got), _bits(want)), (nb, c0)            # the columns outside the block included
            assert np.array_equal(_bits(got_err), _bits(want_err)), (nb, c0)
            assert np.array_equal(_bits(got[:, :c0]), _bits(W[:, :c0])) and np.array_equal(_bits(got[:, c0 + nb:]), _bits(W[:, c0 + nb:]))


def test_refused_calls_return_minus_two_and_touch_nothing(factor_u):
    from dipoorlet_amd import _hip
    dev = torch.device("cuda:0")
    rows = 5
    W = (0.05 * np.random.default_rng(3).standard_normal((rows, K))).astype(np.float32)
    w, u = torch.from_numpy(W).to(dev), torch.from_numpy(factor_u).to(dev)
    scale = torch.full((rows,), 0.01, device=dev)
    zp = torch.zeros(rows, dtype=torch.int32, device=dev)
    err = torch.full((rows, 128), 7.0, device=dev)
    L = _hip.lib()
    P = lambda t: None if t is None else ct.c_void_p(t.data_ptr())     # noqa: E731

    def call(w_=w, rows_=rows, ldw=K, c0=0, nb=64, u_=u, ldu=K, scale_=scale, zp_=zp, nch=rows, qlo=-7, qhi=7, fmt=_hip.GRID_UNIFORM, err_=err):
        return L.dpl_gptq_block(P(w_), rows_, ldw, c0, nb, P(u_), ldu, P(scale_), P(zp_), nch, qlo, qhi, fmt, P(err_), None)

    bad = [dict(w_=None), dict(u_=None), dict(scale_=None), dict(err_=None), dict(zp_=None), dict(nb=0), dict(nb=129), dict(nb=-1),
           dict(c0=K - 63), dict(c0=-1), dict(ldu=100, c0=64), dict(nch=2), dict(nch=0), dict(qlo=0, qhi=0), dict(qlo=7, qhi=-7), dict(fmt=2)]
    for kw in bad:
        assert call(**kw) == -2, kw
        assert b"dpl_gptq_block" in L.dpl_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(W)) and bool((err == 7.0).all())
    assert call(rows_=0) == 0                                           # nothing to do: not an error, nothing launched
    assert call(zp_=None, qlo=0, qhi=0, fmt=_hip.GRID_E4M3) == 0        # FP8 reads neither the zero point nor the bounds
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(w.cpu().numpy()), _bits(W))


def test_a_single_block_layer_is_the_model_exactly():
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    d = C.build(C.SINGLE_BLOCK)
    w = torch.from_numpy(d["W"].copy()).to(dev)
    wq, err = ops.gptq_quantize(w, torch.from_numpy(np.ascontiguousarray(d["U"], np.float32)).to(dev), _dev_grid(d["grid"], dev))
    assert np.array_equal(_bits(wq.cpu().numpy()), _bits(d["W32"])) and np.array_equal(_bits(err.cpu().numpy()), _bits(d["E32"]))
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(d["W"]))        # the input is not modified


@pytest.mark.parametrize("case", C.LAYER_CASES, ids=C.case_id)
def test_layer_is_on_the_grid_and_within_the_caps(case):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    d = C.build(case)
    Q = M.make_q(d["grid"])
    wq, err = ops.gptq_quantize(torch.from_numpy(d["W"].copy()).to(dev), torch.from_numpy(np.ascontiguousarray(d["U"], np.float32)).to(dev),
                                _dev_grid(d["grid"], dev))
    wq = wq.cpu().numpy()
    assert err.shape == wq.shape == d["W"].shape
    assert np.array_equal(_bits(Q(wq)), _bits(wq))                                    # on the grid
    o64, o_dev = M.objective(d["W64"], d["W"], d["H"]), M.objective(wq, d["W"], d["H"])
    s64, s32 = float(np.mean(_bits(wq) != _bits(d["W64"]))), float(np.mean(_bits(wq) != _bits(d["W32"])))
    print(f"{C.case_id(case)}: device vs fp64 model {100 * s64:.4f} % differ, objective x {o_dev / o64:.5f}; vs numpy fp32 {100 * s32:.4f} % differ")
    assert s64 <= 0.01 and o_dev <= 1.02 * o64
    assert s32 <= 0.005
    # the first block has no GEMM in front of it: exact
    assert np.array_equal(_bits(wq[:, :128]), _bits(d["W32"][:, :128]))


def test_a_smaller_block_size_and_the_torch_op(factor_u):
    import dipoorlet_amd.torch_ops  # noqa: F401  (registers torch.ops.dipoorlet.*)
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    d = C.build(C.LAYER_CASES[2])
    g = _dev_grid(d["grid"], dev)
    u = torch.from_numpy(factor_u).to(dev)
    w = torch.from_numpy(d["W"].copy()).to(dev)
    # block = 37: eight kernel calls and a ragged last block; the same caps against the fp64 model
    wq, _ = ops.gptq_quantize(w, u, g, block=37)
    assert float(np.mean(_bits(wq.cpu().numpy()) != _bits(d["W64"]))) <= 0.01
    with pytest.raises(Exception):
        ops.gptq_quantize(w, u, g, block=129)
    a, b = w.clone(), w.clone()
    ea = ops.gptq_block(a, 128, 65, u, g)
    eb = torch.ops.dipoorlet.gptq_block(b, 128, 65, u, g.scale, g.zero_point, g.qlo, g.qhi, "int")
    assert torch.equal(a, b) and torch.equal(ea, eb) and not torch.equal(a, w)
    g8 = _dev_grid(C.build(C.LAYER_CASES[3])["grid"], dev)
    a, b = w.clone(), w.clone()
    ea = ops.gptq_block(a, 0, 128, u, g8)
    eb = torch.ops.dipoorlet.gptq_block(b, 0, 128, u, g8.scale, torch.zeros(1, dtype=torch.int32, device=dev), 0, 0, "e4m3")
    assert torch.equal(a, b) and torch.equal(ea, eb)
