from .tensor_cali_base import tensor_calibration  # noqa: F401
from .basic_algorithm import (find_clip_val_hist, find_clip_val_kl, find_clip_val_minmax,  # noqa: F401
                              find_clip_val_minmax_weight, find_clip_val_octav, find_clip_val_qmse,
                              tensor_cali_dispatcher, tensor_cali_extensions, tensor_cali_grid_aware)
