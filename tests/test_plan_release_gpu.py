"""GPU: a dropped TensorSetPlan gives its OCTAV workspace back at once.  The plan and its OctavTailPlan must not refer to each
other: a cycle would leave tens of MB per dropped plan to the cycle collector, which frees them at a moment of its own — inside
whatever watches torch.cuda.memory_allocated() then (tests/test_octav_routes.py's reference check)."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("inline", [False, True])
def test_dropped_plan_frees_its_octav_workspace_without_the_cycle_collector(inline):
    from dipoorlet_amd import ops
    dev = torch.device("cuda:0")
    x = [torch.from_numpy(np.random.default_rng(3).standard_normal((3, n)).astype(np.float32)).to(dev) for n in (25088, 150528)]
    ops.octav_batch(ops.TensorSetPlan([25088, 150528], 3, dev), x, False, inline=inline)      # (first use of the kernels, outside the window)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        before = torch.cuda.memory_allocated()
        plan = ops.TensorSetPlan([25088, 150528], 3, dev)
        rows = ops.octav_batch(plan, x, False, inline=inline)
        torch.cuda.synchronize()
        assert plan.octav_tail() is not None and torch.cuda.memory_allocated() > before + (1 << 20)     # the workspace exists
        assert torch.isfinite(rows).all()
        del plan, rows
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        gc.enable()
