"""HardNet descriptor with the reference's state-dict layout (HardNet.py:61-101), executed by the
fused HIP trunk kernel + head GEMM (BN and L2 normalisation fused), and HardTFeatNet (HardNet.py:30-59), the network behind the reference's
`--descriptor TFeat` and its trained HardTFeat.pth, executed by csrc/tfeat.hip."""
import torch
import torch.nn as nn

from . import _lib, engine
from ._lib import lib, check, ptr
from .architectures import _HipPatchNet, _container


class HardNet(_HipPatchNet):
    KIND = _lib.NET_HARDNET

    def __init__(self):
        super(HardNet, self).__init__()
        self.features = _container([32, 32, 64, 64, 128, 128], 128, 8, 0, False, head_bn=True)
        self.features[18].p = 0.1
        self.PS = 32
        self.eval()

    def forward(self, input):
        """(n,1,32,32) -> (n,128) L2-normalised descriptors."""
        return self._run(input)


class HardTFeatNet(_HipPatchNet):
    """HardTFeatNet(sm) with the reference's constructor and parameter names (`features.{0,3}`, `classifier.1`); the two nn.Sequential are
    parameter containers only.  `sm` (the reference passes a SIFTNet that forward() never uses) is kept as `.SIFT` outside the module tree:
    state_dict() holds the six learned tensors, and load_state_dict() accepts the reference checkpoint's state dict unchanged - its three
    `SIFT.*` entries are ignored.  Exact fp32 only: `.arith` other than "fp32" raises NotImplementedError."""
    KEYS = ("features.0.weight", "features.0.bias", "features.3.weight", "features.3.bias", "classifier.1.weight", "classifier.1.bias")
    CHUNK = 32768            # rows per launch of a stand-alone call (bounds the scratch: 18 KB per row); rows do not depend on each other

    def __init__(self, sm):
        super(HardTFeatNet, self).__init__()
        self.features = nn.Sequential(nn.Conv2d(1, 32, kernel_size=7), nn.Tanh(), nn.MaxPool2d(kernel_size=2, stride=2),
                                      nn.Conv2d(32, 64, kernel_size=6), nn.Tanh())
        self.classifier = nn.Sequential(nn.Dropout(0.1), nn.Conv2d(64, 128, kernel_size=8), nn.Tanh())
        self.__dict__["SIFT"] = sm
        self.PS = 32
        self.eval()

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super(HardTFeatNet, self).load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("SIFT.")}, strict=strict, **kw)

    def packed_weights(self, device):
        """The packed weight blob (affnet_tfeat_pack_weights) on `device`, cached until the parameters change."""
        stamp = self._weights_stamp()
        if self._packed is None or self._packed_version != stamp or self._packed.device != device:
            sd = self.state_dict()
            t = [sd[k].detach().to("cpu", torch.float32).contiguous() for k in self.KEYS]
            blob = torch.empty(lib.affnet_tfeat_packed_floats(), dtype=torch.float32)
            check(lib.affnet_tfeat_pack_weights(*([ptr(x) for x in t] + [ptr(blob)])), None, "affnet_tfeat_pack_weights")
            self._packed = blob.to(device)
            self._packed_version = stamp
        return self._packed

    def check_usable(self):
        if self.training:
            raise RuntimeError("affnet_amd nets are inference-only (call .eval()); training is out of scope")
        if _lib.arith_code(self.arith) != _lib.ARITH_FP32_MFMA:
            raise NotImplementedError("HardTFeatNet runs in exact fp32 only (arith=%r); the split arithmetic modes cover AffNet / OriNet / HardNet" % (self.arith,))

    def forward(self, input):
        """(n,1,32,32) or (n,32,32) cuda patches -> (n,128) L2-normalised descriptors."""
        self.check_usable()
        x = input
        if not isinstance(x, torch.Tensor):
            engine.require_cuda(x, "patches")
        if x.dim() == 4:
            if x.size(1) != 1:
                raise ValueError("expected single-channel patches")
            x = x[:, 0]
        if x.dim() != 3 or tuple(x.shape[1:]) != (self.PS, self.PS):
            raise ValueError("expected (n,1,32,32) patches, got %s" % (tuple(input.shape),))
        engine.require_cuda(x, "patches")
        x = x.contiguous().float()
        n, dev = x.size(0), x.device
        out = torch.empty(n, 128, dtype=torch.float32, device=dev)
        if n:
            ctx, packed, st = engine.utility_ctx(dev), self.packed_weights(dev), engine.stream_of(dev)
            rows = min(n, self.CHUNK)
            scratch = torch.empty(lib.affnet_tfeat_scratch_floats(rows), dtype=torch.float32, device=dev)
            for s in range(0, n, rows):
                m = min(rows, n - s)
                check(lib.affnet_tfeat_forward(ctx, ptr(packed), ptr(x[s:s + m]), None, m, ptr(out[s:s + m]), ptr(scratch), st), ctx, "affnet_tfeat_forward")
        return out
