"""``fdiff.utils.tensors`` mirror (reference src/fdiff/utils/tensors.py:5-22)."""
from __future__ import annotations

import numpy as np
import torch


def check_flat_array(x):
    """tensors.py:5-22: the samples as a 2-d array (N, everything else flattened).  Host tensors and numpy arrays come
    back as numpy arrays, as in the reference; a tensor that already lives on the device stays a device tensor, so
    that the metrics consume sampler output without a round trip through the host."""
    on_device = isinstance(x, torch.Tensor) and x.device.type == "cuda"
    if isinstance(x, torch.Tensor):
        x = x.detach() if on_device else x.detach().cpu().numpy()
    assert on_device or isinstance(x, np.ndarray), f"x must be a numpy array or a torch tensor. Got {type(x)}"
    flat = x.reshape(x.shape[0], -1) if x.ndim >= 3 else x
    assert flat.ndim == 2, f"x must be a 2d array. Got {flat.ndim}d array."
    return flat
