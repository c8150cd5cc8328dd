"""The reference's SIFT descriptor module with its constructor and call signature (pytorch_sift.py:10-94), executed by
csrc/sift.hip: SIFTNet(patch_size=32) is the descriptor the reference's test() functions construct
(train_AffNet_test_on_graffity.py:122) and the only one whose parameters exist - it has no learned weights."""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn

from . import engine
from ._lib import lib, check, ptr


class L2Norm(nn.Module):
    """x / sqrt(|sum x^2| + 1e-10) along dim 1 (pytorch_sift.py:10-17); a small host-side helper on whatever device x lives."""

    def __init__(self):
        super(L2Norm, self).__init__()
        self.eps = 1e-10

    def forward(self, x):
        return x / torch.sqrt(torch.abs((x * x).sum(dim=1, keepdim=True)) + self.eps)


def getPoolingKernel(kernel_size=25):
    """(k,k) float64 bilinear pooling weights (pytorch_sift.py:19-25): outer product of a ramp step/2, 3 step/2, .. up to 1 and down
    again, step = 1 / floor(k / 2).  k = 11: (.1 .3 .5 .7 .9 1 .9 .7 .5 .3 .1)."""
    step = 1.0 / float(kernel_size // 2)
    up = np.arange(step / 2.0, 1.0, step)
    ramp = np.concatenate([up, [1.0], up[::-1]])
    return np.maximum(0, np.outer(ramp, ramp))


def get_bin_weight_kernel_size_and_stride(patch_size, num_spatial_bins):
    """pytorch_sift.py:26-29: stride = round(2 floor(patch_size / 2) / (num_spatial_bins + 1)), kernel size = 2 stride - 1."""
    stride = int(round(2.0 * math.floor(patch_size / 2) / float(num_spatial_bins + 1)))
    return int(2 * stride - 1), stride


class SIFTNet(nn.Module):
    def __init__(self, patch_size=65, num_ang_bins=8, num_spatial_bins=4, clipval=0.2):
        super(SIFTNet, self).__init__()
        if (patch_size, num_ang_bins, num_spatial_bins) != (32, 8, 4):
            raise NotImplementedError("the HIP SIFT kernel is specialised for patch_size=32, num_ang_bins=8, num_spatial_bins=4 (the "
                                      "SIFTNet(patch_size=32) the reference's test() functions construct), got patch_size=%r, num_ang_bins=%r, "
                                      "num_spatial_bins=%r" % (patch_size, num_ang_bins, num_spatial_bins))
        self.PS = patch_size
        self.num_ang_bins, self.num_spatial_bins, self.clipval = num_ang_bins, num_spatial_bins, clipval
        self.bin_weight_kernel_size, self.bin_weight_stride = get_bin_weight_kernel_size_and_stride(patch_size, num_spatial_bins)
        buf = (C.c_float * (patch_size * patch_size))()
        check(lib.affnet_sift_host_window(patch_size, buf), None, "affnet_sift_host_window")
        self.gk = torch.from_numpy(np.array(buf, dtype=np.float32).reshape(patch_size, patch_size))     # CircularGaussKernel(kernlen=32)
        self._windows = {}           # device -> the window as one device tensor

    def window(self, device):
        """The 32 x 32 window on `device` (uploaded once per device): the d_window of affnet_sift_forward / _pyr."""
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._windows:
            self._windows[key] = self.gk.to(device).contiguous()
        return self._windows[key]

    def forward(self, x):
        """(n,1,32,32) or (n,32,32) -> (n,128) descriptors, plain fp32."""
        engine.require_cuda(x, "patches")
        if x.dim() == 4:
            if x.size(1) != 1:
                raise ValueError("expected single-channel patches")
            x = x[:, 0]
        if x.dim() != 3 or tuple(x.shape[1:]) != (self.PS, self.PS):
            raise ValueError("expected (n,1,32,32) patches, got %s" % (tuple(x.shape),))
        x = x.contiguous().float()
        n, dev = x.size(0), x.device
        out = torch.empty(n, 128, dtype=torch.float32, device=dev)
        if n:
            ctx = engine.utility_ctx(dev)
            rc = lib.affnet_sift_forward(ctx, ptr(x), n, ptr(self.window(dev)), float(self.clipval), ptr(out), engine.stream_of(dev))
            check(rc, ctx, "affnet_sift_forward")
        return out
