"""The stated per-launch error bounds shared by the detector and recogniser audits (tests/test_craft_layers_gpu.py,
tests/test_crnn_layers_gpu.py, tests/test_crnn_layer_bounds_cpu.py): a launch is judged by the bound of the kernel
family that ran it, named by the tap's profiler row."""
import numpy as np
import torch
import torch.nn.functional as F

WINDOW = 3  # T|x|: +-3 columns of a Winograd tile
U32 = 2.0 ** -24


def pool2(t):
    """floor 2x2 max pooling of an NHWC array (keras 'valid')"""
    return F.max_pool2d(torch.from_numpy(np.ascontiguousarray(t)).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).numpy()


def kernel_row(kernel):
    rows = [r for r in kernel.split("+") if r not in ("absmax", "maxpool2x2")]
    return rows[0] if rows else kernel


def family(row, weight_shape):
    """(k, window) of the stated bound of the kernel that wrote a convolution (profiler row)"""
    if row.startswith(("conv_w4", "conv_wh_", "conv_ws_")):
        return 5e-6, WINDOW
    if row.startswith(("conv_dh_", "conv_ds_", "conv_hh_", "conv_hs_", "conv_k5")):
        return 1.5e-6, 0
    if row.startswith("conv_mfma"):
        cout, cin, kh, kw = weight_shape
        return cin * kh * kw * U32, 0
    raise AssertionError(f"no stated bound for kernel row {row}")
