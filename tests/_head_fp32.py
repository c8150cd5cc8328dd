"""Plain numpy restatement of the split-K head GEMMs - HardNet's (affnet_amd/csrc/cnn_heads.hip: hardnet_head_kernel<MP>, hardnet_head_s3_kernel<MP, TERMS>,
hardnet_finish_kernel, the dispatch of aff_hardnet_head) and HardTFeat's classifier (affnet_amd/csrc/tfeat.hip: tfeat_head_kernel) - operation by operation in
float32, and the inputs of the tests that use it.  numpy, tests/_fp32_chain.py and tests/_match_fp32.py only: no torch, no affnet_amd, no GPU.
tests/test_head_mirror_host.py ties every function here to something the project already trusts (libm fmaf, float64, the oracle, weights_layout.h) and proves
that the inputs contain the cases they claim; tests/test_gpu_head.py compares the kernels with it on the bytes.

What the kernels do, as restated here:
  partials   K is cut into four quarters (blockIdx.y); per (row, output, quarter) ONE fmaf chain from 0 over the quarter's k in the order the fragments feed
             v_mfma_f32_16x16x4_f32: for t: for j: for kq: k = quarter start + 16 t + 4 kq + j (tests/_match_fp32.py: k_order; one MFMA = that chain over kq is
             shown on the device by tests/test_gpu_matcher.py).  The order does not depend on the patches per workgroup (MP 64 / 32 / 16): a row's tile only
             decides which wave holds its accumulator.  Scratch: [quarter][row][128] behind the trunk tensor [row][K].
  finish     v = (((0 + p0) + p1) + p2) + p3, + bias; lane l of 64 holds v0 = v[l], v1 = v[64 + l]; t = v0 * v0 + v1 * v1 with every operation rounded on its
             own (-ffp-contract=off); wave_sum of csrc/cnn_mfma.h: t += t[lane ^ 1]; t += t[lane ^ 2]; t += t[lane ^ 7] (the 8-lane mirror); t += t[lane ^ 15]
             (the 16-lane mirror); tot = (t[0] + t[16]) + (t[32] + t[48]); nrm = sqrtf(tot + 1e-8f); v0 / nrm, v1 / nrm.
  split      the same sums on split operands: x = three bf16 terms (nearest even, exact remainders) or two fp16 terms (activations as they are, weights times
             2^e); the term pairs (a_i, w_j), i + j <= TERMS - 1; products exact, fp32 accumulation on the matrix core.  Emulated here in float64 (the
             "ideal split": no accumulation error), with a variant that leaves one named pair out.
  dispatch   MP = 64 iff cdiv(n_max, 64) * 4 * B >= 256, else 32 iff cdiv(n_max, 32) * 4 * B >= 256, else 16."""
import os

import numpy as np

from _fp32_chain import F32, _round_odd_sum
from _match_fp32 import k_order

KSPLIT = 4
HARDNET_K, TFEAT_K = 8192, 4096
U32 = 2.0 ** -24                                       # unit roundoff of float32
# E_mirror: the worst |head_partials - float64| / sum |a| |w| over the conv5 activations of the golden patches (tests/test_head_mirror_host.py measures
# 2.4207e-07 on the authoring host and asserts that this constant is that figure to within a quarter); the split-mode bar on partials is 8 x this, the convention of tests/test_gpu_tfeat.py
E_MIRROR = 2.43e-7
N_ROWS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]  # row counts of the tile sweep: around every edge of the 16 / 32 / 64-row tiles, and more than two tiles of each
PAIRS = {3: [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)], 2: [(0, 0), (0, 1), (1, 0)]}       # (activation term, weight term) in the kernel's term-major order


def gamma(k):
    """The standard bound of k roundings in float32: gamma_k = k u / (1 - k u)."""
    return k * U32 / (1.0 - k * U32)


def head_mp(n_max, B):
    """aff_hardnet_head's choice of the patches per workgroup."""
    cdiv = lambda a, b: (a + b - 1) // b
    if cdiv(n_max, 64) * KSPLIT * B >= 256:
        return 64
    return 32 if cdiv(n_max, 32) * KSPLIT * B >= 256 else 16


def _layout_head_offset(kind):
    """Float offset of the head weights in the packed blob (csrc/weights_layout.h: net_layout / tfeat_layout) and the head's K."""
    if kind == "tfeat":
        return 52 * 32 + 32 + 36 * 32 * 64 + 64, TFEAT_K
    assert kind == "hardnet", kind
    ch, off = [1, 32, 32, 64, 64, 128, 128], 0
    for i in range(6):
        off += (12 if i == 0 else 9 * ch[i]) * ch[i + 1] + ch[i + 1]
        off = (off + 3) & ~3
    return off, HARDNET_K


def unpack_head(blob, kind):
    """(W (K, 128), bias (128,)) float32 out of the packed blob of HardNet ("hardnet": BN folded) or HardTFeat ("tfeat"): the floats the head kernel reads, from
    [k / 16][(k / 4) % 4][n][k % 4] (weights_layout.h: head_index) back to [k][n], k = pixel * channels + channel; the bias sits behind the weights."""
    blob = np.asarray(blob).reshape(-1)
    assert blob.dtype == F32
    off, K = _layout_head_offset(kind)
    W = blob[off: off + K * 128].reshape(K // 16, 4, 128, 4).transpose(0, 1, 3, 2).reshape(K, 128)
    return np.ascontiguousarray(W), blob[off + K * 128: off + K * 128 + 128].copy()


def head_index(k, n, K=HARDNET_K):
    """weights_layout.h: w_tap_index(0, k, n, K, 128), restated."""
    return (((k // 16) * 4 + (k // 4) % 4) * 128 + n) * 4 + k % 4


def _quarters(A, W, ksplit):
    A, W = np.ascontiguousarray(A, dtype=F32), np.ascontiguousarray(W, dtype=F32)
    n, K = A.shape
    assert W.shape == (K, 128) and K % (16 * ksplit) == 0
    kq = K // ksplit
    return A.astype(np.float64).reshape(n, ksplit, kq).transpose(1, 0, 2), W.astype(np.float64).reshape(ksplit, kq, 128), kq


def head_partials(A, W, ksplit=KSPLIT, k_quarter=None, natural=False):
    """A (n, K), W (K, 128) float32 -> (ksplit, n, 128) float32: per (quarter, row, output) one fmaf chain from 0 over the quarter's k in k_order, shifted by
    the quarter's start.  HardNet: K 8192 = 4 x 2048; HardTFeat: K 4096 = 4 x 1024.  natural: the variant that walks k ascending."""
    A64, W64, kq = _quarters(A, W, ksplit)
    assert k_quarter is None or k_quarter == kq
    acc = np.zeros((ksplit, A64.shape[1], 128), np.float64)          # always holds fp32 values
    for k in k_order(kq, natural):
        acc = _round_odd_sum(A64[:, :, k, None] * W64[:, None, k, :], acc).astype(F32).astype(np.float64)
    return acc.astype(F32)


def exact_partials(A, W, ksplit=KSPLIT):
    """The same sums in float64 (products of two floats are exact there; 2048 additions of 53 bits): (partials, sum |a| |w|), each (ksplit, n, 128)."""
    A64, W64, _ = _quarters(A, W, ksplit)
    return np.matmul(A64, W64), np.matmul(np.abs(A64), np.abs(W64))


def wave_sum(t):
    """(n, 64) float32 -> (n,): csrc/cnn_mfma.h wave_sum."""
    lanes = np.arange(64)
    for x in (1, 2, 7, 15):
        t = t + t[:, lanes ^ x]
        assert t.dtype == F32
    return (t[:, 0] + t[:, 16]) + (t[:, 32] + t[:, 48])


def hardnet_finish(partials, bias, swap12=False):
    """(4, n, 128) float32 partials, (128,) bias -> (n, 128) float32 descriptors: hardnet_finish_kernel on the rows below the count.  swap12: the variant that adds
    quarter 2 before quarter 1."""
    p, bias = np.ascontiguousarray(partials, dtype=F32), np.asarray(bias, dtype=F32)
    v = np.zeros(p.shape[1:], F32)
    for s in ((0, 2, 1, 3) if swap12 else (0, 1, 2, 3)):
        v = v + p[s]
    v = v + bias[None, :]
    v0, v1 = v[:, :64], v[:, 64:]
    tot = wave_sum(v0 * v0 + v1 * v1)
    nrm = np.sqrt(tot + F32(1e-8))
    out = v / nrm[:, None]
    assert out.dtype == F32 and tot.dtype == F32
    return out


def finish_fp64(partials64, bias):
    """The finish in float64: (n, 128)."""
    v = partials64.sum(axis=0) + np.asarray(bias, np.float64)[None, :]
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True) + 1e-8)


# ---- the operand splits, in float64 ----------------------------------------------------------------------------------------------------
def _bf16(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(F32)


def split_terms(x, terms, scale=1.0):
    """(terms, ...) float64: three bf16 terms of x (each the nearest bf16 of the exact remainder), or two fp16 terms of scale * x (a power of two; h = fp16(x),
    l = fp16(x - h), the remainder exact in float32)."""
    x = np.ascontiguousarray(x, dtype=F32)
    out, r = [], x if terms == 3 else (x * F32(scale)).astype(F32)
    for t in range(terms):
        h = _bf16(r) if terms == 3 else r.astype(np.float16).astype(F32)
        out.append(h.astype(np.float64))
        r = r - h
        assert r.dtype == F32
    return np.stack(out)


def h2_scale(W):
    """The power of two 2^e that brings the largest |w| into [2^13, 2^14) (weights_layout.h: head_h2)."""
    return 2.0 ** (13 - int(np.floor(np.log2(float(np.abs(W).max())))))


def split_partials(A, W, terms, drop=None, ksplit=KSPLIT):
    """The "ideal split" partials in float64, (ksplit, n, 128): the sum over the term pairs of PAIRS[terms] of (activation term) x (weight term), every
    product and sum exact to float64; two-term mode: times 2^-e behind the sum.  drop: a pair of PAIRS[terms] to leave out."""
    A, W = np.ascontiguousarray(A, dtype=F32), np.ascontiguousarray(W, dtype=F32)
    n, K = A.shape
    scale = h2_scale(W) if terms == 2 else 1.0
    At = split_terms(A, terms).reshape(terms, n, ksplit, K // ksplit).transpose(0, 2, 1, 3)
    Wt = split_terms(W, terms, scale).reshape(terms, ksplit, K // ksplit, 128)
    assert drop is None or tuple(drop) in PAIRS[terms]
    out = np.zeros((ksplit, n, 128), np.float64)
    for (i, j) in PAIRS[terms]:
        if drop is None or (i, j) != tuple(drop):
            out += np.matmul(At[i], Wt[j])
    return out / scale


def planted_split_rows(W, n0=0):
    """(3, K) float32 activation rows aimed at output n0, one per small term pair of the three-term mode - (0, 2), (1, 1), (2, 0), each about 2^-17 of a
    product, which real activations add up with random signs to less than a float32 chain's own error.  Every row lines the signs of its pair's products up:
      (0, 2)  a = 1 where the weight's third term is positive and at least 2^-18 of the weight, else 0
      (1, 1)  a = 1 + s (2^-8 - 2^-16) = terms (1, s (2^-8 - 2^-16), 0), s the sign of the weight's second term, where that is at least 2^-10 of the weight
      (2, 0)  a = 1 + 2^-9 + s 2^-18 = terms (1, 2^-9, s 2^-18), s the sign of the weight
    Values a ReLU could have produced (all >= 0)."""
    Wt = split_terms(W, 3)[:, :, n0]
    w = np.abs(W[:, n0].astype(np.float64))
    r02 = np.where((Wt[2] > 0) & (np.abs(Wt[2]) >= 2.0 ** -18 * w), 1.0, 0.0)
    r11 = np.where(np.abs(Wt[1]) >= 2.0 ** -10 * w, 1.0 + np.sign(Wt[1]) * (2.0 ** -8 - 2.0 ** -16), 0.0)
    r20 = 1.0 + 2.0 ** -9 + np.sign(W[:, n0].astype(np.float64)) * 2.0 ** -18
    rows = np.stack([r02, r11, r20])
    assert np.array_equal(rows.astype(F32).astype(np.float64), rows)
    return rows.astype(F32)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_PATCHES = {}


def patch_set():
    """(80, 32, 32) float32, made once and never modified: the 76 golden patches of tests/golden/sift_graf16_n500.npz (64 graf patches, 12 edge patches with
    all 0 at row 64 and all 255 at row 65), then the planted ones: constant 97, all 0, all 255 (a constant patch is exactly zero behind the input norm: the
    three share one trunk row and one descriptor), and a vertical step 0 | 255."""
    if "p" not in _PATCHES:
        g = np.load(os.path.join(GOLDEN, "sift_graf16_n500.npz"))
        step = np.zeros((32, 32), F32)
        step[:, 16:] = 255.0
        planted = np.stack([np.full((32, 32), 97.0, F32), np.zeros((32, 32), F32), np.full((32, 32), 255.0, F32), step])
        p = np.concatenate([g["patches1"], g["patches2"], g["edge_patches"], planted]).astype(F32)
        assert p.shape == (80, 32, 32)
        p.setflags(write=False)
        _PATCHES["p"] = p
    return _PATCHES["p"]


CONSTANT_ROWS = (64, 65, 76, 77, 78)      # rows of patch_set() that hold one value everywhere


def tiled_patches(n):
    """(n, 32, 32): row i = patch_set()[i % 80]."""
    p = patch_set()
    return np.ascontiguousarray(p[np.arange(n) % p.shape[0]])


def edge_rows(n, tiles=(16, 32, 64)):
    """The rows of 0 .. n - 1 worth a look: first, last, and both sides of every tile edge."""
    rows = {0, n - 1}
    for t in tiles:
        for e in range(t, n, t):
            rows |= {e - 1, e}
    return sorted(rows)
