"""Weight transforms that run between calibration and deployment (dipoorlet/weight_transform/)."""
from .adaround import adaround
from .bias_correction import bias_correction
from .brecq import brecq
from .gptq import gptq
from .rotate import mx_rotate
from .smooth import smooth_quant
from .sparse_quant import sparse_quant
from .update_bn import update_bn
from .weight_equalization import weight_equalization
from .weight_trans_base import weight_calibration

__all__ = ["adaround", "bias_correction", "brecq", "gptq", "mx_rotate", "smooth_quant", "sparse_quant", "update_bn", "weight_calibration", "weight_equalization"]
