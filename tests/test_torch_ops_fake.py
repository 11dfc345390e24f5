"""The fake kernels (register_fake) of `torch.ops.dipoorlet.*` alone, no GPU: under a FakeTensorMode, on fake device="cuda" tensors
built from the table of sample calls (tests/torch_op_cases.py), every op returns what the docstrings of dipoorlet_amd/torch_ops.py
and dipoorlet_amd/ops.py state — how many outputs, their shapes, dtypes and device — and CONTIGUOUS strides whatever the strides
of its inputs: the real ops compute on x.contiguous() and return contiguous tensors, and a compiler that trusts the fake kernel
indexes the real output by the fake one's strides.  (torch.library.opcheck's fake-tensor utility does not compare strides.)
EXPECT below is written from those docstrings, not from the fake kernels."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import dipoorlet_amd.torch_ops  # noqa: F401
import torch_op_cases as T

F32, U8 = torch.float32, torch.uint8


def _like_x(a):
    return [(tuple(a[0].shape), F32)]


def _gemm_shape(a):
    return tuple(a[0].shape[:-1]) + (a[2].shape[-2],)


# op -> args -> [(shape, dtype) of every output]; [] for an op that returns nothing
EXPECT = {
    "minmax": lambda a: [((2,), F32)],
    "minmax_batched": lambda a: [],
    "abs_hist_": lambda a: [],
    "abs_hist_batched_": lambda a: [],
    "hist_percentile": lambda a: [((2,), F32)],
    "hist_kl": lambda a: [((2,), F32)],
    "hist_qmse": lambda a: [((2,), F32)],
    "octav": lambda a: [((3,), F32)],
    "octav_batched": lambda a: [((a[0][0].shape[0], len(a[0]), 3), F32)],
    "rowwise_minmax": lambda a: [((a[0].shape[0],), F32)] * 2,
    "colwise_absmax": lambda a: [((a[0].shape[-1],), F32)],
    "fake_quant": _like_x,
    "fake_quant_relu": _like_x,
    "fake_quant_add_relu": _like_x,
    "fake_quant_fp8": _like_x,
    "fake_quant_set": lambda a: [(tuple(x.shape), F32) for x in a[0]],
    "fake_quant_mx": _like_x,
    "mx_encode": lambda a: [(s, U8) for s in T.packed_shapes(tuple(a[0].shape), a[1], a[2])],
    "mx_decode": lambda a: [(tuple(a[3]), F32)],
    "mx_gemm": lambda a: [(_gemm_shape(a), F32)],
    "mx_scale_search": lambda a: [(T.block_shape(tuple(a[0].shape), a[1]), U8)],
    "fake_quant_mx_scaled": _like_x,
    "hadamard32": _like_x,
    "gptq_block": lambda a: [((a[0].shape[0], a[2]), F32)],
    "gptq_mx_block": lambda a: [((a[0].shape[0], a[2]), F32), ((a[0].shape[0], -(-a[0].shape[1] // 32)), U8)],
}


def outputs_of(result):
    """What an op returned as a flat list of tensors (None: an op that returns nothing)."""
    if result is None:
        return []
    return list(result) if isinstance(result, (tuple, list)) else [result]


def contiguous_strides(shape):
    out, n = [], 1
    for d in reversed(shape):
        out.append(n)
        n *= max(int(d), 1)
    return tuple(reversed(out))


def test_the_table_names_exactly_the_registered_ops():
    assert sorted(T.CASES) == T.registered_ops() and len(T.CASES) == 25
    assert sorted(EXPECT) == sorted(T.CASES)
    for op, cases in T.CASES.items():
        assert cases and len({c.id for c in cases}) == len(cases), op
        assert cases[0].layout == "contig", op
    for op in T.TAKES_ANY_LAYOUT:
        assert any(c.layout != "contig" for c in T.CASES[op]), op


def test_the_builders_give_the_layouts_they_name():
    for op, c in T.all_cases():
        args, _ = c.build("cpu")
        flat = [t for a in args for t in (a if isinstance(a, (list, tuple)) else [a]) if isinstance(t, torch.Tensor)]
        dense = all(t.numel() == t.untyped_storage().nbytes() // t.element_size() for t in flat)
        assert dense and all(t.is_contiguous() for t in flat) == (c.layout == "contig"), (op, c.id)


@pytest.mark.parametrize("op,case", T.all_cases(), ids=T.case_ids())
def test_fake_kernel_returns_what_the_docstrings_state(op, case):
    with FakeTensorMode():
        args, kwargs = case.build("cuda")
        outs = outputs_of(getattr(torch.ops.dipoorlet, op)(*args, **kwargs))
    want = EXPECT[op](args)
    assert len(outs) == len(want), (op, case.id, len(outs), len(want))
    for i, (y, (shape, dtype)) in enumerate(zip(outs, want)):
        tag = (op, case.id, i)
        assert isinstance(y, torch._subclasses.FakeTensor), tag
        assert tuple(y.shape) == tuple(int(d) for d in shape), (tag, tuple(y.shape), shape)
        assert y.dtype == dtype, (tag, y.dtype, dtype)
        assert y.device == torch.device("cuda", 0), (tag, y.device)
        assert tuple(y.stride()) == contiguous_strides(shape), (tag, tuple(y.stride()), contiguous_strides(shape))


def test_the_stride_expectation_is_torchs_own():
    for shape in ((2,), (3, 40), (2, 8, 5, 5), (2, 3, 1, 4)):
        assert contiguous_strides(shape) == torch.empty(shape).stride()
