"""The node-major walk of the fake-quantised network behind --bc, --update_bn, AdaRound / BRECQ / --sparse (reconstruct) and --gptq."""
import numpy as np
import torch

from .. import dist_helper
from ..executor import Frontier, GraphSession, load_chunks
from ..graph import ONNXGraph
from ..quantize import quant_graph
from .utils import update_weight


class QuantWalk:
    """A copy of `graph` that receives the new constants (graph_new), its fake-quantised form under the given ranges (graph_q) with
    a session (s_q), and — after start() — a Frontier (qf) over a shard of the calibration images.  A transform visits graph_q's
    nodes in order, writes a node's new constant with set_const() and runs the node with qf.run(), so everything downstream sees
    the new constants.  clip_val: the merged ranges, untouched (quant_graph, which collapses per-tensor ranges in place, gets a
    copy of its own).  The walk itself is no collective: a transform that only rank 0 runs may use it."""

    @torch.no_grad()
    def __init__(self, graph, act_clip_val, weight_clip_val, args):
        self.clip_val = {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**act_clip_val, **weight_clip_val}.items()}
        self.graph_new = ONNXGraph()
        self.graph_new.copy_from(graph)
        self.args = args
        self.rank, self.world = dist_helper.rank(), dist_helper.world()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.graph_q, _ = quant_graph(self.graph_new, {k: [np.copy(v[0]), np.copy(v[1])] for k, v in self.clip_val.items()}, args)
        self.s_q = GraphSession(self.graph_q, device=self.dev)

    @torch.no_grad()
    def start(self, st, ed, on_host=False):
        """Load images [st, ed) in chunks (bounds: load_chunks') -> the Frontier over them: its `env` holds the input chunks and
        nothing else yet.  on_host: Frontier's."""
        self.bounds, inputs = load_chunks(self.graph_new, self.args, st, ed, self.dev, on_host)
        self.qf = Frontier(self.s_q, self.bounds, inputs, on_host)
        return self.qf

    def set_const(self, name, value):
        """value (device tensor) becomes initializer `name` of the result, of the fake-quantised graph and of its session."""
        update_weight(self.graph_new, value.cpu().numpy(), name)
        update_weight(self.graph_q, value.cpu().numpy(), name)
        self.s_q.set_const(name, value)

    def finish(self, save_name):
        """-> the graph with the new constants; rank 0 saves it as <save_name>.onnx."""
        self.graph_new.update_model()
        if self.rank == 0 and getattr(self.args, "output_dir", None):
            self.graph_new.output_dir = self.args.output_dir
            self.graph_new.save_onnx_model(save_name)
        return self.graph_new
