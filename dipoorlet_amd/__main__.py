"""`python -m dipoorlet_amd -M model.onnx -I calib_dir -N 1024 -A hist -D trt` — the reference's CLI
(dipoorlet/__main__.py:23-161) over the MI355X calibration core (`-A kl`, the entropy search, `-A qmse`, the quantisation-MSE search on the platform's grid, `-D ocp_fp8`, static OCP FP8 E4M3 scales, `--mx`, OCP Microscaling on MatMul / Gemm operands, `--mx_rotate`, a block-Hadamard rotation of those operands, `--mx_pack`, the constant ones as packed element codes and E8M0 scales, `--mx_verify`, those bytes multiplied on the block-scaled matrix instruction and compared with the fake-quantised graph, `--mx_scale_search`, error-minimising block scales for the constant ones, `--gptq`, Hessian-compensated weight rounding, `--mx_gptq`, the same on the block-scaled grids, and `--mx_mixed`, MXFP4 or MXFP8 per node under a weight-bit budget, are this project's additions).

Same flags; same phases where they are in scope: load model -> tensor calibration (sharded over ranks)
-> per-rank clip JSON -> rank-0 reduce -> load -> profiling (cosine similarity of the fake-quantised
model, optional) -> weight transforms (--smooth, --mx_rotate, --mx_mixed, --bc, --we, --update_bn, --adaround, --brecq [--drop], --sparse, --gptq, --mx_gptq) -> platform deploy file.
Extra flags: --calib_batch, --resident_gb, --merge {allreduce,reference}, --skip_profiling, --timing_json.
"""
import argparse
import copy
import os
import sys
import time

import torch.distributed as dist

from . import dist_helper
from .deploy import to_deploy
from .graph import ONNXGraph
from .tensor_cali import tensor_calibration
from .utils import MARKS, load_clip_val, logger, mark, reduce_clip_val, save_clip_val, setup_logger


def build_parser():
    from .platform_settings import MX_CHOICES
    p = argparse.ArgumentParser(prog="dipoorlet_amd")
    p.add_argument("-M", "--model", help="onnx model")
    p.add_argument("-I", "--input_dir", help="calibration data", required=True)
    p.add_argument("-O", "--output_dir", help="output data path")
    p.add_argument("-N", "--data_num", help="num of calibration pics", type=int, required=True)
    for flag in ("--we", "--bc", "--update_bn", "--adaround", "--brecq", "--drop", "--savefp", "--stpu_wg",
                 "--skip_prof_layer", "--slurm", "--mpirun", "--sparse", "--optim_transformer", "--smooth", "--gptq"):
        p.add_argument(flag, default=False, action="store_true")
    p.add_argument("-A", "--act_quant", choices=["minmax", "hist", "mse", "kl", "qmse"], default="mse",
                   help="minmax / hist: bit-exact clip ranges; mse (OCTAV): within 1e-5 * max(1, |ref|) of the reference's, repeating "
                        "to about 1e-6 relative from run to run (DPL_OCTAV_FORM=bracket: the bit-stable two-read form); kl: entropy "
                        "search on the |x| histogram (not in the reference; honours --bins, ignores --threshold); qmse: the clip of least "
                        "quantisation error of that histogram on the platform's own grid, integer or FP8 (not in the reference; -D trt, "
                        "stpu, ocp_fp8; honours --bins, ignores --threshold)")
    p.add_argument("-D", "--deploy", choices=["trt", "stpu", "magicmind", "rv", "atlas", "snpe", "ti", "imx", "ocp_fp8"],
                   required=True, help="ocp_fp8 (not in the reference): static OCP FP8 E4M3 scales, clip / 448; with -A minmax, -A hist or -A qmse")
    p.add_argument("--bins", default=2048, type=int)  # the reference omits type= and crashes on a CLI value
    p.add_argument("--threshold", default=0.99999, type=float)
    p.add_argument("--ada_bs", type=int, default=64)
    p.add_argument("--ada_epoch", type=int, default=5000)
    p.add_argument("--skip_layers", default=[], type=str, nargs="+")
    p.add_argument("--sparse_rate", type=float, default=0.5)
    p.add_argument("--smooth_alpha", type=float, default=0.5,
                   help="--smooth (not in the reference): fold per-channel scales s = max|x|^alpha / max|w|^(1 - alpha) of every LayerNorm "
                        "affine that feeds only MatMul / Gemm weights into those weights; alpha in [0, 1]")
    p.add_argument("--mx", choices=list(MX_CHOICES), default=None,
                   help="(not in the reference; with -D ocp_fp8 only) OCP Microscaling on both operands of every MatMul / Gemm, constant "
                        "ones included: blocks of 32 along the reduction axis share a power-of-two scale taken from the data, the elements "
                        "are FP8 E4M3 (mxfp8), FP6 E2M3 or E3M2 (mxfp6_e2m3, mxfp6_e3m2: no --mx_gptq, no --mx_mixed) or FP4 E2M1 (mxfp4); every "
                        "other node keeps the platform's static E4M3 scales")
    p.add_argument("--mx_rotate", default=False, action="store_true",
                   help="(not in the reference; with --mx only) rotate every MX block of both operands of every MatMul / Gemm that has a "
                        "constant 2-D weight and a reduction length K that is a multiple of 32, by the 32-point Hadamard matrix H32: "
                        "(X . H) . (H . W / 32) = X . W, the same function in real arithmetic, with a large channel spread over its block.  "
                        "The weight side is folded offline, the activation side is a BlockHadamard node (domain dipoorlet.amd) that a "
                        "runtime applies in front of its MX quantiser.  Runs after --smooth and before --bc; writes rotate_model.onnx and "
                        "rotate_report.json, and a \"rotation\" entry in ocp_mx_blocks.json")
    p.add_argument("--mx_pack", default=False, action="store_true",
                   help="(not in the reference; with --mx only) also write the constant MX operands as the bytes a block-scaled GEMM reads: "
                        "ocp_mx_weights.bin (per tensor its OCP E4M3 bytes or packed E2M1 nibbles, then its E8M0 scale bytes, both "
                        "K-innermost, every section on a 64-byte boundary) and ocp_mx_weights.json (offsets and shapes, keyed as "
                        "ocp_mx_blocks.json).  Encoded on the device from the weights as they stand after every weight transform")
    p.add_argument("--mx_verify", default=False, action="store_true",
                   help="(not in the reference; with --mx_pack only) after the deploy files are written, read ocp_mx_weights.bin back and "
                        "run every MatMul / Gemm (ops.mx_gemm) and, under --mx_conv, every Conv (ops.mx_conv) whose two operands are "
                        "block-scaled on CDNA4's block-scaled matrix instruction — the activation operand encoded on the device, the constant one from the file's bytes — over the "
                        "first --calib_batch images, and compare with that node's output in the fake-quantised graph: writes "
                        "mx_verify_report.json, changes no other file")
    p.add_argument("--mx_scale_search", default=False, action="store_true",
                   help="(not in the reference; with --mx only) give every block of every CONSTANT MatMul / Gemm operand whichever of the "
                        "floor-rule shared exponent and the next one up gives the smaller squared Q/DQ error (the floor rule clips "
                        "everything above 6 of 8 (mxfp4) resp. 448 of 512 (mxfp8) in the top binade; ties keep the floor).  Activations "
                        "keep the floor rule, which a runtime can recompute.  The bytes travel explicitly: as the second input of the "
                        "weight's MXQuantizeDequantize node in quant_model.onnx, into ocp_mx_weights.bin under --mx_pack, and through "
                        "--mx_verify; writes mx_scale_report.json and \"weight_scales\": \"search\" in ocp_mx_blocks.json")
    p.add_argument("--mx_gptq", default=False, action="store_true",
                   help="(not in the reference; with --mx only) GPTQ on the block-scaled grids: every Gemm and every MatMul with a constant "
                        "2-D weight is rounded column by column with each column's error pushed onto the columns not yet rounded, a "
                        "block's shared exponent being fixed by the floor rule when the recursion enters the block; the result is a fixed "
                        "point of the graph's MXQuantizeDequantize node, so nothing but the weights changes.  Conv weights go through "
                        "--gptq's path on their static E4M3 grid.  Honours --gptq_block (32, 64, 96 or 128) and --gptq_damp; writes "
                        "gptq.onnx and gptq_report.json.  Not with --gptq or --mx_scale_search")
    p.add_argument("--mx_conv", default=False, action="store_true",
                   help="(not in the reference; with --mx only) block-scale both operands of every Conv over two spatial axes with group 1 "
                        "and a constant weight too: the [N, C, H, W] activation and the [Cout, C, kh, kw] weight along axis 1, so a block "
                        "is 32 consecutive channels at one pixel resp. at one (cout, ky, kx), a short last one holding the channels that exist.  "
                        "Every other Conv (grouped or depthwise, 1-D or 3-D, a weight that is no constant) keeps its static E4M3 nodes and "
                        "is logged with its reason.  --mx_scale_search, --mx_pack and --mx_verify cover these operands as they cover a "
                        "MatMul's (--mx_verify multiplies them on the block-scaled matrix instruction: ops.mx_conv); --mx_rotate leaves "
                        "Convs alone.  Adds \"conv\": {\"nodes\", \"left\"} to ocp_mx_blocks.json.  Not with --mx_gptq")
    p.add_argument("--mx_mixed", type=float, default=None, metavar="BITS",
                   help="(not in the reference; with --mx mxfp4 only) MXFP4 or MXFP8 per node under a weight-bit budget: BITS in [4, 8] is "
                        "the average element bits allowed over the weights of the candidate nodes — every Gemm (no transA, alpha = beta = "
                        "1, a bias absent or [n]) and every MatMul whose right operand is a constant 2-D weight that nothing else reads.  "
                        "Over the first --calib_batch images each candidate's product is formed in both formats on the block-scaled "
                        "matrix instruction and held against its fp32 output (ops.mx_gemm_err); the nodes that gain most per weight bit "
                        "are promoted, both operands, to mxfp8 while the budget lasts.  Runs after --smooth / --mx_rotate and before "
                        "--bc; everything else stays at mxfp4 and is logged with its reason.  Writes mx_mixed_report.json; "
                        "ocp_mx_blocks.json, ocp_mx_weights.json, mx_scale_report.json and mx_verify_report.json then say \"format\": "
                        "\"mixed\" and name each entry's own format")
    p.add_argument("--gptq_block", type=int, default=128,
                   help="--gptq (not in the reference; every platform, -D ocp_fp8 included): round every Conv (group 1) / Gemm weight column "
                        "by column onto the platform's weight grid, pushing each column's rounding error onto the columns not yet rounded "
                        "along the inverse Hessian of the layer's fake-quantised inputs (GPTQ); writes gptq.onnx.  --gptq_block: columns "
                        "per kernel call, 1 .. 128")
    p.add_argument("--gptq_damp", type=float, default=0.01,
                   help="--gptq: damp * mean(diag H) is added to the Hessian's diagonal before it is factorised; > 0")
    p.add_argument("--pattern", choices=["unstruction", "nv24"], default="unstruction")
    p.add_argument("--model_type", choices=["unet"], default=None)
    p.add_argument("--quant_format", default="QDQ", type=str, choices=["QOP", "QDQ"])
    # MI355X-side knobs
    p.add_argument("--calib_batch", type=int, default=None,
                   help="calibration images per forward (default: by the graph's size — about 8 GB of exposed activations per batch, at most 64); "
                        "--bc, --update_bn, profiling and AdaRound / BRECQ walk the set in chunks of this size too (16 when not given)")
    p.add_argument("--resident_gb", type=float, default=160.0, help="HBM budget for keeping pass-1 activations")
    p.add_argument("--merge", choices=["allreduce", "reference"], default="allreduce")
    p.add_argument("--skip_profiling", default=False, action="store_true")
    p.add_argument("--timing_json", default=None, help="rank 0 writes where the calibration time went (host .bin ingest, GPU "
                                                        "forward, GPU statistics, wall) to this file")
    p.add_argument("--keep_bn", default=False, action="store_true",
                   help="do not fold BatchNormalization into the preceding Conv / Gemm (the reference always simplifies; "
                        "note: --update_bn also keeps the BN nodes, which it re-estimates — unlike the reference, whose "
                        "onnxsim pass has fused them before --update_bn runs)")
    return p


def check_args(args):
    """What a platform cannot do, said before any device work.  `-A qmse` models a symmetric grid with a free scale and a fixed
    sign: the integer grid of `-D trt` / `stpu` and the E4M3 codes of `-D ocp_fp8`.  A floating-point grid (`-D ocp_fp8`) is reached through the
    FakeQuant nodes only: the clip sweeps that know nothing of the grid and the transforms that run the fake-quantised forward
    work unchanged; what assumes or learns an integer grid does not."""
    from .platform_settings import mx_fp6_setting_table, platform_setting_table
    from .quantize import number_format
    alpha = getattr(args, "smooth_alpha", 0.5)
    if not 0.0 <= alpha <= 1.0:      # (a NaN too)
        raise ValueError(f"--smooth_alpha must lie in [0, 1], got {alpha}")
    if getattr(args, "mx_gptq", False) and getattr(args, "gptq", False):
        raise ValueError("--mx_gptq and --gptq cannot be combined: --mx_gptq runs --gptq's driver over the block-scaled weights and "
                         "the static ones alike")
    if getattr(args, "gptq", False):
        for flag in ("adaround", "brecq", "sparse"):
            if getattr(args, flag, False):
                raise ValueError(f"--gptq and --{flag} cannot be combined: two transforms would each decide how the weights are rounded")
        if getattr(args, "mx", None):
            raise ValueError(f"--gptq and --mx {args.mx} cannot be combined: block-scaled operands are not on a static grid (GPTQ on MX "
                             "grids is not built)")
        if not 1 <= getattr(args, "gptq_block", 128) <= 128:
            raise ValueError(f"--gptq_block must lie in [1, 128], got {args.gptq_block}")
        if not getattr(args, "gptq_damp", 0.01) > 0.0:      # (a NaN too)
            raise ValueError(f"--gptq_damp must be positive, got {args.gptq_damp}")
    if getattr(args, "mx_gptq", False):
        if not getattr(args, "mx", None):
            raise ValueError("--mx_gptq needs --mx mxfp8 or --mx mxfp4: it rounds the weights that --mx block-scales (--gptq serves a "
                             "static grid)")
        if args.mx in mx_fp6_setting_table:
            raise ValueError(f"--mx_gptq is not supported with --mx {args.mx}: the recursion's model and kernel are held to the two grids "
                             "of mxfp8 and mxfp4 (E4M3, E2M1); an FP6 grid is not built")
        for flag in ("adaround", "brecq", "sparse"):
            if getattr(args, flag, False):
                raise ValueError(f"--mx_gptq and --{flag} cannot be combined: two transforms would each decide how the weights are rounded")
        if getattr(args, "mx_scale_search", False):
            raise ValueError("--mx_gptq and --mx_scale_search cannot be combined: the searched scale bytes are computed from the weights "
                             "before GPTQ replaces them and are not refreshed afterwards")
        if getattr(args, "gptq_block", 128) not in (32, 64, 96, 128):
            raise ValueError(f"--gptq_block must be 32, 64, 96 or 128 with --mx_gptq (whole MX blocks per kernel call), got {args.gptq_block}")
        if not getattr(args, "gptq_damp", 0.01) > 0.0:      # (a NaN too)
            raise ValueError(f"--gptq_damp must be positive, got {args.gptq_damp}")
    if getattr(args, "mx_rotate", False) and not getattr(args, "mx", None):
        raise ValueError("--mx_rotate needs --mx mxfp8 or --mx mxfp4: it rotates the 32-element blocks that --mx scales, and does "
                         "nothing for a static grid")
    if getattr(args, "mx_pack", False) and not getattr(args, "mx", None):
        raise ValueError("--mx_pack needs --mx mxfp8 or --mx mxfp4: it writes the element codes and block scales of the operands that "
                         "--mx scales, and a static grid has neither")
    if getattr(args, "mx_scale_search", False) and not getattr(args, "mx", None):
        raise ValueError("--mx_scale_search needs --mx mxfp8 or --mx mxfp4: it chooses the block scales of the constant operands that "
                         "--mx scales, and a static grid has none")
    if getattr(args, "mx_conv", False):
        if not getattr(args, "mx", None):
            raise ValueError("--mx_conv needs --mx mxfp8 or --mx mxfp4: it block-scales the Conv operands the way --mx block-scales a "
                             "MatMul's, and a static grid has no blocks")
        if getattr(args, "mx_gptq", False):
            raise ValueError("--mx_conv and --mx_gptq cannot be combined: the MX GPTQ kernel wants a weight's blocks contiguous along K of "
                             "[N, K], and a Conv weight's channel blocks are strided there (not built)")
    if getattr(args, "mx_mixed", None) is not None:
        if not getattr(args, "mx", None):
            raise ValueError("--mx_mixed needs --mx mxfp4: it promotes nodes of a block-scaled graph from the base format mxfp4 to "
                             "mxfp8, and a static grid has neither")
        if args.mx in mx_fp6_setting_table:
            raise ValueError(f"--mx_mixed is not supported with --mx {args.mx}: its budget arithmetic is two-level, 4 bits (mxfp4) or 8 "
                             "(mxfp8) per weight element, and its error kernel is built for those two formats")
        if args.mx != "mxfp4":
            raise ValueError(f"--mx_mixed is not supported with --mx {args.mx}: the base format is mxfp4 and the budget buys mxfp8 "
                             "where it helps most; with mxfp8 everywhere there is nothing to promote to")
        if not 4.0 <= args.mx_mixed <= 8.0:      # (a NaN too)
            raise ValueError(f"--mx_mixed must lie in [4, 8], the average element bits of mxfp4 everywhere and of mxfp8 everywhere, "
                             f"got {args.mx_mixed}")
    if getattr(args, "mx_verify", False) and not getattr(args, "mx_pack", False):
        raise ValueError("--mx_verify needs --mx_pack: it reads ocp_mx_weights.bin back and multiplies those bytes on the block-scaled "
                         "matrix instruction, and without --mx_pack there is no such file")
    if getattr(args, "mx", None) and args.deploy != "ocp_fp8":
        raise ValueError(f"--mx {args.mx} is not supported with -D {args.deploy}: block-scaled MatMul / Gemm operands sit beside static "
                         "FP8 scales on every other node.  Supported: -D ocp_fp8")
    qi = platform_setting_table[args.deploy]["qi_params"]
    if args.act_quant == "qmse":
        # the search models ONE grid per format: symmetric about zero, any real scale, the sign fixed
        why = ("its activations are asymmetric (a zero point)" if not qi["symmetric"] else
               "its activation scales are powers of two (log_scale)" if qi.get("log_scale") else
               "the sign of its activations is decided per tensor (dynamic_sym)" if "dynamic_sym" in qi else None)
        if why:
            raise ValueError(f"-A qmse is not supported with -D {args.deploy}: {why}, and the search models a symmetric grid with a "
                             "free scale.  Supported: -D trt, -D stpu, -D ocp_fp8")
    if number_format(qi["type"]).integer:
        return
    bad = [flag for flag, on in (("-A mse", args.act_quant == "mse"),        # OCTAV's fixed point assumes a uniform grid
                                 ("-A kl", args.act_quant == "kl"),          # its levels are integer levels
                                 ("--adaround", args.adaround), ("--brecq", args.brecq), ("--sparse", args.sparse)) if on]
    if bad:     # (the three transforms learn integer rounding)
        raise ValueError(f"-D {args.deploy} is a floating-point grid: {', '.join(bad)} not supported (they assume or learn an integer "
                         "grid).  Supported: -A minmax, -A hist, -A qmse, --bc, --we, --update_bn and profiling")


def main(argv=None):
    """One rank of a calibration run.  A rank that fails must not leave its peers parked at the next barrier (the
    reference's ranks hang until the launcher is killed, __main__.py:105-110): the error is logged and the process exits
    non-zero at once, which makes torch.distributed.run / mpirun / srun take the whole group down."""
    try:
        return _main(argv)
    except SystemExit:
        _join_helpers()
        raise
    except BaseException as e:   # noqa: BLE001
        import traceback
        traceback.print_exc()
        logger.error("rank %s failed: %s", os.environ.get("RANK", "0"), e)
        sys.stdout.flush()
        sys.stderr.flush()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            os._exit(1)   # no atexit / destructor may wait on a collective the peers will never join
        _join_helpers()
        raise


def _join_helpers():
    """The warm-up threads (executor.warm_libraries, GraphSession.prewarm_convs) are done within tenths of a second; a run that
    fails before its first forward must not exit underneath them."""
    ex = sys.modules.get(__package__ + ".executor")
    if ex is not None:
        ex.join_helpers()


def _process_age_s():
    """Seconds since this process was created (interpreter start-up and imports included)."""
    try:
        with open("/proc/self/stat") as f:
            start_ticks = int(f.read().rsplit(")", 1)[1].split()[19])
        with open("/proc/uptime") as f:
            up = float(f.read().split()[0])
        return up - start_ticks / os.sysconf("SC_CLK_TCK")
    except Exception:   # noqa: BLE001
        return None


def _main(argv=None):
    t_enter = time.time()
    mark("main:enter")
    age_at_enter = _process_age_s()       # interpreter + imports (torch, the package) up to here
    args = build_parser().parse_args(argv)
    check_args(args)
    if args.quant_format == "QOP":
        raise SystemExit("--quant_format QOP (onnxruntime's QOperator export, dipoorlet/utils.py:415-435) is not built: "
                         "use the default QDQ format")
    if args.slurm:
        dist_helper.init_from_slurm()
    elif args.mpirun:
        dist_helper.init_from_mpi()
    else:
        dist_helper.init_default()
    t_dist = time.time()
    mark("main:group_and_device")
    rank, world = dist.get_rank(), dist.get_world_size()
    import torch
    if os.environ.get("DPL_DETERMINISTIC") == "1":
        # MIOpen's default convolution kernels are not bit-reproducible from call to call (1e-6 relative on an activation): a run
        # that has to repeat bit for bit asks the library for its deterministic algorithms (slower; the first use compiles them)
        torch.backends.cudnn.deterministic = True
    warm = None
    if torch.cuda.is_available():
        # the HIP context and the libraries' first calls: on a helper thread from here on, beside the model load and the
        # session build (executor.warm_libraries; its own clock reports the context's seconds)
        from . import executor
        dev0 = torch.device("cuda", rank % max(1, torch.cuda.device_count()))
        executor.warm_libraries(dev0, blas=False)
        warm = executor._WARM
        try:    # the op types of the model file, without its tensors (milliseconds): a transformer's matrix products go to the BLAS
            # library, whose first call (0.2 s) then starts now, beside the model load.  (A convolutional network's one or two run
            # on ops.gemm_small; the session starts this thread if they turn out not to.)
            from . import onnx_io
            ops_seen = onnx_io.scan_op_types(args.model)
            if ops_seen.get("MatMul", 0) + ops_seen.get("Gemm", 0) > 4:
                executor.warm_blas(dev0)
        except Exception:   # noqa: BLE001  (best effort: the load below reports what is wrong with the file)
            pass
    t_ctx = time.time()
    if args.output_dir is None:
        args.output_dir = os.path.join(os.path.abspath(os.path.dirname(args.model)), "results")
    if args.model_type is not None:      # __main__.py:71-73 (the onnxruntime transformer optimiser step is not run:
        args.optim_transformer = True    # the graph is executed as it is)
        args.skip_prof_layer = True
    if rank == 0:
        os.makedirs(args.output_dir, exist_ok=True)
        setup_logger(args)
    dist.barrier()
    start = time.time()
    onnx_graph = ONNXGraph.load(args.model, args.output_dir, args.deploy, args.model_type)
    if not args.keep_bn and not args.update_bn:     # __main__.py:101 — onnxsim's Conv + BN fusion
        n_folded = onnx_graph.fold_batchnorm()
        if n_folded and rank == 0:
            logger.info("Folded {} BatchNormalization nodes into their producers.".format(n_folded))
    args.rank, args.world_size = rank, world
    args.local_rank = rank % max(1, torch.cuda.device_count())
    if rank == 0:
        logger.info("Do tensor calibration...")
    t_cal = time.time()
    mark("main:calibration_starts")
    prof_path = os.environ.get("DPL_PROFILE_HOST")     # (a tuning aid: cProfile of this rank's calibration phase, top entries to that file)
    if prof_path:
        import cProfile
        import pstats
        prof = cProfile.Profile()
        act_clip_val, weight_clip_val = prof.runcall(tensor_calibration, onnx_graph, args)
        with open(prof_path, "w") as f:
            pstats.Stats(prof, stream=f).sort_stats("cumtime").print_stats(60)
    else:
        act_clip_val, weight_clip_val = tensor_calibration(onnx_graph, args)
    if args.timing_json and rank == 0:
        import json
        from .forward_net import CalibrationRun
        mark("main:calibration_done")
        tm = CalibrationRun.last.timing() if CalibrationRun.last is not None else {}
        # seconds after main() was entered at which each point of a fresh process was first passed (warm:* = the helper thread)
        tm["timeline_s"] = {k: round(v - t_enter, 4) for k, v in sorted(MARKS.items(), key=lambda kv: kv[1])}
        tm.update(tensor_calibration_wall_s=time.time() - t_cal, load_model_wall_s=t_cal - start, act_quant=args.act_quant,
                  calib_batch=getattr(CalibrationRun.last, "batch", args.calib_batch), world_size=world,
                  # the fixed costs of a fresh process, itemised: interpreter + imports, process group, HIP context (the
                  # first batch's MIOpen algorithm search is forward_first_batch_gpu_s above)
                  startup={"interpreter_and_imports_s": age_at_enter,
                           "process_group_init_s": dist_helper.TIMES.get("group", t_dist - t_enter),
                           "process_group_backend": dist.get_backend(),
                           # first touch of the HIP runtime + the context (seconds longer right after a process that held
                           # most of the HBM has exited: the driver is still releasing it)
                           "hip_context_s": dist_helper.TIMES.get("device", 0.0) + (t_ctx - t_dist) + ((warm or {}).get("context_s") or 0.0),
                           "library_warm_threads_s": {k: round(v, 4) for k, v in (warm or {}).items() if k in ("kernels_s", "blas_s")},
                           "until_calibration_starts_s": t_cal - t_enter})
        with open(args.timing_json, "w") as f:
            json.dump(tm, f)
        CalibrationRun.last = None     # (a run pins its session, accumulators and every plan's scratch)
    tensor_range = copy.deepcopy(act_clip_val)
    save_clip_val(act_clip_val, weight_clip_val, args, act_fname=f"act_clip_val.json.rank{rank}",
                  weight_fname=f"weight_clip_val.json.rank{rank}")
    dist.barrier()
    if rank == 0:
        reduce_clip_val(world, args, already_merged=(args.merge != "reference"))
    dist.barrier()
    act_clip_val, weight_clip_val = load_clip_val(args)
    from .weight_transform import weight_calibration
    if rank == 0:
        logger.info("Weight transform...")
    graph_after_wt, graph_ori, act_clip_val, weight_clip_val = weight_calibration(onnx_graph, act_clip_val,
                                                                                  weight_clip_val, args)
    dist.barrier()
    if not args.skip_profiling:
        from .profiling import (quantize_profiling_multipass, quantize_profiling_transformer, show_model_profiling_res,
                                show_model_ranges, weight_need_perchannel)
        if rank == 0:
            logger.info("Profiling...")
        prof = quantize_profiling_transformer if args.model_type is not None else quantize_profiling_multipass   # :141-146
        layer_cos, model_cos, qnodes = prof(graph_after_wt, graph_ori, act_clip_val, weight_clip_val, args)
        if rank == 0:
            show_model_profiling_res(graph_after_wt, layer_cos, model_cos, qnodes, args)
            show_model_ranges(graph_after_wt, act_clip_val, weight_clip_val, args)
            weight_need_perchannel(graph_after_wt, args)
    if rank == 0:
        logger.info("Deploy to " + args.deploy + "...")
        to_deploy(graph_after_wt, act_clip_val, weight_clip_val, args)
        if getattr(args, "mx_verify", False):
            from .mx_verify import mx_verify
            logger.info("Verifying the packed MX operands on the block-scaled matrix instruction...")
            mx_verify(graph_after_wt, act_clip_val, weight_clip_val, args)
        logger.info("Total time cost: {} seconds.".format(int(time.time() - start)))
    dist.barrier()
    _ = tensor_range
    _join_helpers()
    return 0


if __name__ == "__main__":
    sys.exit(main())
