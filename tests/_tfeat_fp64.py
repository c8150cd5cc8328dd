"""float64 numpy evaluation of HardTFeatNet.forward in eval mode (HardNet.py:30-59): the referee of the HardTFeat tests.  Our own code:
the steps a reader of the reference's forward() would list, evaluated in double from the six learned tensors.

  1. input norm per patch: (x - mean) / (unbiased std + 1e-7);
  2. conv1 1 -> 32, 7 x 7 valid, + bias, tanh: 32 x 32 -> 26 x 26;   3. max-pool 2 x 2 stride 2 -> 13 x 13;
  4. conv2 32 -> 64, 6 x 6 valid, + bias, tanh -> 8 x 8;   (dropout: identity)
  5. classifier 64 -> 128, 8 x 8 valid, + bias, tanh -> 1 x 1: a 4096 x 128 product over k = c * 64 + y * 8 + x;
  6. x / sqrt(sum x^2 + 1e-8).

Convolutions are cross-correlations (torch's Conv2d), written as sums over the taps of shifted views: no torch call."""
import numpy as np

KEYS = ("features.0.weight", "features.0.bias", "features.3.weight", "features.3.bias", "classifier.1.weight", "classifier.1.bias")


def _conv_valid(x, w, b):
    """x (n,cin,H,W), w (cout,cin,kh,kw), b (cout,) -> (n,cout,H-kh+1,W-kw+1) in float64."""
    cout, cin, kh, kw = w.shape
    ho, wo = x.shape[2] - kh + 1, x.shape[3] - kw + 1
    out = np.zeros((x.shape[0], cout, ho, wo))
    for ky in range(kh):
        for kx in range(kw):
            out += np.einsum("nchw,oc->nohw", x[:, :, ky:ky + ho, kx:kx + wo], w[:, :, ky, kx], optimize=True)
    return out + b[None, :, None, None]


def tfeat_fp64(patches, sd):
    """patches (n,32,32) or (n,1,32,32); sd: mapping with the six KEYS (numpy or torch tensors) -> (n,128) float64."""
    w = {k: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float64) for k in KEYS}
    p = np.asarray(patches, dtype=np.float64).reshape(-1, 1, 32, 32)
    flat = p.reshape(p.shape[0], -1)
    mean = flat.mean(axis=1)
    std = flat.std(axis=1, ddof=1) + 1e-7
    x = (p - mean[:, None, None, None]) / std[:, None, None, None]
    x = np.tanh(_conv_valid(x, w[KEYS[0]], w[KEYS[1]]))
    x = x.reshape(x.shape[0], 32, 13, 2, 13, 2).max(axis=(3, 5))
    x = np.tanh(_conv_valid(x, w[KEYS[2]], w[KEYS[3]]))
    x = np.tanh(x.reshape(x.shape[0], -1) @ w[KEYS[4]].reshape(128, -1).T + w[KEYS[5]][None, :])
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True) + 1e-8)


def random_state_dict(seed=0):
    """Seeded random weights, U(-a, a) with a = 1 / sqrt(fan_in) per layer (weights and biases): every index is distinguishable and the
    tanh layers stay out of saturation."""
    rs = np.random.RandomState(seed)
    shapes = {KEYS[0]: (32, 1, 7, 7), KEYS[2]: (64, 32, 6, 6), KEYS[4]: (128, 64, 8, 8)}
    out = {}
    for kw, kb in ((KEYS[0], KEYS[1]), (KEYS[2], KEYS[3]), (KEYS[4], KEYS[5])):
        s = shapes[kw]
        a = 1.0 / np.sqrt(s[1] * s[2] * s[3])
        out[kw] = rs.uniform(-a, a, s).astype(np.float32)
        out[kb] = rs.uniform(-a, a, (s[0],)).astype(np.float32)
    return out


def load_golden_weights(golden_dir):
    """The trained tensors of the reference's HardTFeat.pth from the three weight fixtures (split by classifier output channel to keep every
    file small), joined into one state dict of float32 numpy arrays."""
    import os
    parts = [np.load(os.path.join(golden_dir, "tfeat_weights_%d.npz" % i)) for i in range(3)]
    sd = {k: parts[0][k] for k in KEYS[:4]}
    sd[KEYS[4]] = np.concatenate([p["classifier.1.weight.part"] for p in parts], axis=0)
    sd[KEYS[5]] = parts[2][KEYS[5]]
    return sd
