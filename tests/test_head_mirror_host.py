"""CPU: tests/_head_fp32.py, the float32 restatement of the split-K head GEMMs (HardNet's head, HardTFeat's classifier), tied to what the project already
trusts, so that tests/test_gpu_head.py may compare the kernels with it on the bytes:

  head_partials       libm fmaf (ctypes) called value by value in the stated order, and float64 within the gamma_2048 bound of a 2048-term chain
  hardnet_finish      a scalar lane-by-lane restatement of wave_sum, float64, and (through both) oracle.hardnet_forward's descriptors
  unpack_head         weights_layout.h's head_index, inverted for every (k, n) on a ramp blob; the BN-folded weights the packer wrote
  head_mp             the dispatch arithmetic at both ends of the two row ranges in which one image / two images take the 32-patch shape
  split emulation     the ideal three-term / two-term sums stay inside the split-mode bar (8 x E_mirror on sum |a| |w|), every sum with one term pair left
                      out exceeds it: the bar of tests/test_gpu_head.py is neither vacuous nor blind

and the inputs are shown to contain what they claim (constant patches with one shared descriptor, a zero activation row whose descriptor is bias / |bias|,
rows whose partials differ between the two k orders).

Measured on the authoring host (48 golden patches + the 4 planted ones, synthetic HardNet weights): E_mirror 2.42e-07 of sum |a| |w| (gamma_2048 = 1.22e-04);
descriptors of the mirror against the oracle's 3.13e-07; ideal split 1.24e-09 (three bf16 terms) and 1.71e-08 (two fp16 terms); bar 8 x E_mirror = 1.94e-06.
With one pair left out, golden activations and planted rows: three terms (0,0) 0.386, (0,1) 5.15e-04, (0,2) 5.01e-06, (1,0) 3.97e-04, (1,1) 3.79e-06,
(2,0) 3.81e-06; two terms (0,0) 0.386, (0,1) 6.65e-05, (1,0) 4.71e-05.  On the golden activations alone the three small pairs give 5.05e-07, 5.65e-07 and
5.07e-07: inside the bar (see test_split_bar_is_neither_vacuous_nor_blind)."""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest
import torch

import affnet_oracle as orc
import _head_fp32 as hf
from _fp32_chain import F32
from _match_fp32 import k_order

SPLIT_BAR = 8.0 * hf.E_MIRROR
DESC_BAR = 2e-5          # the suite's bar for stand-alone HardNet descriptors against the oracle (tests/test_gpu_parity.py)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def head(weights):
    """(W (8192, 128), bias) of the synthetic HardNet, out of the packed blob."""
    from affnet_amd import engine
    return hf.unpack_head(engine.pack_state_dict(2, weights["HardNet"]), "hardnet")


@pytest.fixture(scope="module")
def acts(weights, golden_dir):
    """conv5 activations (n, 8192), k = pixel * 128 + channel, of the 48 golden patches and the 4 planted ones, and the oracle's descriptors: the oracle's own
    layer outputs, so that only the head differs."""
    g = np.load(os.path.join(golden_dir, "cnn_random_patches.npz"))
    p = torch.cat([torch.from_numpy(g["patches"]), torch.from_numpy(hf.patch_set()[76:].copy()).unsqueeze(1)])
    with torch.no_grad():
        y = orc.cnn_trunk(weights["HardNet"], orc.input_norm(p))
        want = orc.hardnet_forward(weights["HardNet"], p)
    A = y.permute(0, 2, 3, 1).reshape(p.size(0), -1).contiguous().numpy()
    return A, want.numpy()


@pytest.fixture(scope="module")
def mirror(acts, head):
    A, W = acts[0], head[0]
    part = hf.head_partials(A, W)
    exact, mag = hf.exact_partials(A, W)
    return part, exact, mag


def test_chain_equals_libm_fmaf_on_the_bytes(acts, head):
    """Quarter 1 of one golden row against 2048 libm fmaf calls per output in k_order; the natural order differs on it."""
    path = ctypes.util.find_library("m")
    assert path, "libm not found"
    libm = ctypes.CDLL(path)
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    A, W = acts[0][3:4], head[0]
    cols = [0, 17, 64, 127]
    want = {False: np.zeros(len(cols), F32), True: np.zeros(len(cols), F32)}
    for natural in (False, True):
        for i, c in enumerate(cols):
            s = 0.0
            for k in k_order(2048, natural):
                s = libm.fmaf(float(A[0, 2048 + k]), float(W[2048 + k, c]), s)
            want[natural][i] = s
    assert same(hf.head_partials(A, W)[1, 0, cols], want[False])
    assert same(hf.head_partials(A, W, natural=True)[1, 0, cols], want[True])
    assert same(hf.head_partials(A, W, hf.KSPLIT, 2048)[1, 0, cols], want[False])
    assert not same(want[False], want[True]), "the two K orders give the same bits on this sample: it cannot tell them apart"


def test_mirror_against_float64_and_the_oracle(acts, head, mirror):
    A, want = acts
    W, bias = head
    part, exact, mag = mirror
    # partials: |chain - exact| <= gamma_2048 sum |a| |w| (2048 fused multiply-adds, one rounding each)
    err = np.abs(part.astype(np.float64) - exact)
    assert np.all(err <= hf.gamma(2048) * mag)
    e_mirror = float((err / np.maximum(mag, 1e-300)).max())
    # descriptors: the finish against float64 on the same partials (4 + 1 additions, the 128-term norm, sqrt, division: gamma_140 per element and on the norm)
    d = hf.hardnet_finish(part, bias)
    d64 = hf.finish_fp64(part.astype(np.float64), bias)
    assert float(np.abs(d - d64).max()) <= 2.0 * hf.gamma(140)
    # and against the oracle's descriptors of the same patches
    d_err = float(np.abs(d - want).max())
    print("E_mirror = %.3g of sum |a| |w| (gamma_2048 = %.3g); mirror descriptors vs the oracle: max abs %.3g" % (e_mirror, hf.gamma(2048), d_err))
    # the constant the split-mode bar of tests/test_gpu_head.py is built on is this measurement on the authoring host; the activations come from this host's
    # torch convolutions, whose last bits may differ from that host's and move the worst of 26624 chains: the constant must stay the figure, not a bound on it
    assert 0.8 * hf.E_MIRROR <= e_mirror <= 1.25 * hf.E_MIRROR, e_mirror
    assert d_err <= DESC_BAR
    assert float(np.abs(hf.finish_fp64(exact, bias) - want).max()) <= DESC_BAR


def test_wave_sum_and_finish_against_a_scalar_restatement(head):
    """hardnet_finish lane by lane with numpy float32 scalars: the xor-1, xor-2, 8-lane mirror, 16-lane mirror steps and the four row sums; the quarter order
    matters on this input."""
    rng = np.random.default_rng(11)
    p = (rng.normal(size=(4, 3, 128)) * np.exp2(rng.integers(-3, 4, (4, 3, 128)))).astype(F32)
    bias = head[1]
    want = np.zeros((3, 128), F32)
    for r in range(3):
        v = [F32(F32(F32(F32(F32(0.0) + p[0, r, c]) + p[1, r, c]) + p[2, r, c]) + p[3, r, c]) for c in range(128)]
        v = [F32(v[c] + bias[c]) for c in range(128)]
        t = [F32(F32(v[l] * v[l]) + F32(v[64 + l] * v[64 + l])) for l in range(64)]
        t = [F32(t[l] + t[l ^ 1]) for l in range(64)]
        t = [F32(t[l] + t[l ^ 2]) for l in range(64)]
        t = [F32(t[l] + t[(l & ~7) | (7 - (l & 7))]) for l in range(64)]
        t = [F32(t[l] + t[(l & ~15) | (15 - (l & 15))]) for l in range(64)]
        tot = F32(F32(t[0] + t[16]) + F32(t[32] + t[48]))
        nrm = np.sqrt(F32(tot + F32(1e-8)))
        want[r] = [F32(v[c] / nrm) for c in range(128)]
    got = hf.hardnet_finish(p, bias)
    assert same(got, want)
    assert not same(hf.hardnet_finish(p, bias, swap12=True), want), "adding quarter 2 before quarter 1 gives the same bits on this input"
    assert np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(1)) - 1.0).max() < 1e-6


def test_input_conditions(acts, head, mirror):
    A, want = acts
    W, bias = head
    part = mirror[0]
    p = hf.patch_set()
    for r in hf.CONSTANT_ROWS:
        assert p[r].min() == p[r].max(), r
    assert p[64].max() == 0.0 and p[65].min() == 255.0 and p[77].max() == 0.0 and p[78].min() == 255.0 and p[76].min() == 97.0
    assert p[79].min() == 0.0 and p[79].max() == 255.0
    # constant patches are exactly zero behind the input norm: one trunk row (the BN shifts behind ReLU, not zero), one descriptor
    assert same(A[48], A[49]) and same(A[48], A[50]) and A[48].max() > 0.0 and not same(A[48], A[51])
    d = hf.hardnet_finish(part, bias)
    assert same(d[48], d[49]) and same(d[48], d[50])
    # an all-zero trunk row (what the head reads for rows past the count's tile edge): every partial + 0, the descriptor bias / |bias|
    zero = hf.head_partials(np.zeros((1, hf.HARDNET_K), F32), W)
    assert not zero.any()
    dz = hf.hardnet_finish(zero, bias)[0].astype(np.float64)
    b64 = bias.astype(np.float64)
    assert np.abs(dz - b64 / np.sqrt((b64 * b64).sum() + 1e-8)).max() <= 2.0 * hf.gamma(140)
    # rows whose partials differ between the k orders: a natural-order chain fails the byte test on every row but the constant ones' shared zeros
    nat = hf.head_partials(A[:8], W, natural=True)
    differs = [not same(nat[:, r], part[:, r]) for r in range(8)]
    assert all(differs), differs


def test_unpack_head_inverts_head_index():
    for kind, K in (("hardnet", hf.HARDNET_K), ("tfeat", hf.TFEAT_K)):
        off, k_ = hf._layout_head_offset(kind)
        assert k_ == K
        blob = np.full(off + K * 128 + 128 + 7, -1.0, F32)
        blob[off: off + K * 128 + 128] = np.arange(K * 128 + 128, dtype=F32)            # a ramp: every value names its position (exact below 2^24)
        W, bias = hf.unpack_head(blob, kind)
        k, n = np.meshgrid(np.arange(K), np.arange(128), indexing="ij")
        assert np.array_equal(W, hf.head_index(k, n, K).astype(F32))
        assert np.array_equal(bias, np.arange(K * 128, K * 128 + 128, dtype=F32))
    # the restated index is the header's: its parts and its one literal
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "affnet_amd", "csrc", "weights_layout.h")).read()
    assert "return ((((size_t)p * (cin / 16) + c / 16) * 4 + (c / 4) % 4) * cout + n) * 4 + c % 4;" in src
    assert "constexpr size_t head_index(size_t k, int n) { return w_tap_index(0, (int)k, n, HEAD_K, 128); }" in src


def test_unpack_head_offsets_are_the_library_s(weights):
    """The offsets restated in _head_fp32 against the blobs the packers write: HardNet's folded head = features.19 / sqrt(var + 1e-5) in [pixel][channel] order,
    HardTFeat's classifier transposed to k = pixel * 64 + channel."""
    from affnet_amd import engine
    from _tfeat_fp64 import random_state_dict
    from affnet_amd._lib import lib, check, ptr
    sd = weights["HardNet"]
    W, bias = hf.unpack_head(engine.pack_state_dict(2, sd), "hardnet")
    inv = 1.0 / torch.sqrt(sd["features.20.running_var"].double() + 1e-5)
    ref = (sd["features.19.weight"].double() * inv.view(-1, 1, 1, 1)).permute(2, 3, 1, 0).reshape(8192, 128).numpy()
    assert np.abs(W - ref).max() <= 2.0 * hf.U32 * np.abs(ref).max()
    assert np.abs(bias - (-sd["features.20.running_mean"].double() * inv).numpy()).max() <= 4.0 * hf.U32
    tsd = random_state_dict(0)
    keys = ("features.0.weight", "features.0.bias", "features.3.weight", "features.3.bias", "classifier.1.weight", "classifier.1.bias")
    t = [torch.from_numpy(np.ascontiguousarray(tsd[k], dtype=np.float32)) for k in keys]
    blob = torch.empty(lib.affnet_tfeat_packed_floats(), dtype=torch.float32)
    check(lib.affnet_tfeat_pack_weights(*([ptr(x) for x in t] + [ptr(blob)])), None, "affnet_tfeat_pack_weights")
    Wt, bt = hf.unpack_head(blob, "tfeat")
    assert np.array_equal(Wt, t[4].permute(2, 3, 1, 0).reshape(4096, 128).numpy()) and np.array_equal(bt, t[5].numpy())
    assert hf._layout_head_offset("tfeat")[0] + 4096 * 128 + 128 == blob.numel()


@pytest.mark.parametrize("n_max,B,mp", [(2016, 1, 16), (2017, 1, 32), (4032, 1, 32), (4033, 1, 64), (992, 2, 16), (993, 2, 32), (1984, 2, 32), (1985, 2, 64)])
def test_head_mp_dispatch(n_max, B, mp):
    wg = lambda rows: -(-n_max // rows) * 4 * B
    want = 64 if wg(64) >= 256 else (32 if wg(32) >= 256 else 16)
    assert hf.head_mp(n_max, B) == want == mp
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "affnet_amd", "csrc", "cnn_heads.hip")).read()
    assert "(aff_cdiv(n_max, 64) * HEAD_KSPLIT * B >= 256) ? 64 : ((aff_cdiv(n_max, 32) * HEAD_KSPLIT * B >= 256) ? 32 : 16)" in src


def test_split_terms_are_exact_and_nearest():
    rng = np.random.default_rng(5)
    x = (rng.normal(size=100000) * np.exp2(rng.integers(-10, 6, 100000))).astype(F32)
    t3 = hf.split_terms(x, 3)
    assert np.array_equal(t3.sum(axis=0), x.astype(np.float64)), "three bf16 terms carry 24 bits exactly"
    assert np.all((t3.astype(F32).view(np.uint32) & 0xFFFF) == 0)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(t3[0].astype(F32), want), "the first term is torch's round-to-nearest-even bf16"
    t2 = hf.split_terms(x, 2, 4.0)
    assert np.array_equal(t2[0], (x * F32(4.0)).astype(np.float16).astype(np.float64))
    assert np.all(np.abs(t2.sum(axis=0) - 4.0 * x.astype(np.float64)) <= np.abs(4.0 * x) * 2.0 ** -23 + 2.0 ** -25)


@pytest.mark.parametrize("terms", [3, 2])
def test_split_bar_is_neither_vacuous_nor_blind(acts, head, mirror, terms):
    """8 x E_mirror on sum |a| |w|: the ideal split sums stay inside, every sum with one term pair left out goes outside - on the golden activations together with
    the planted rows of hf.planted_split_rows.  On the golden activations ALONE the three small pairs of the three-term mode, (0, 2), (1, 1), (2, 0), stay
    inside (5.1e-07, 5.7e-07, 5.1e-07 against a bar of 1.94e-06: products of 2^-17 with random signs add up to less than the float32 chain's own error); the
    planted rows line their signs up.  Asserted as found, so that a change of either shows."""
    A, W = acts[0], head[0]
    exact, mag = mirror[1], mirror[2]
    P = hf.planted_split_rows(W)
    p_exact, p_mag = hf.exact_partials(P, W)
    rel = lambda p, q: max(float((np.abs(p - exact) / np.maximum(mag, 1e-300)).max()), float((np.abs(q - p_exact) / np.maximum(p_mag, 1e-300)).max()))
    ideal = rel(hf.split_partials(A, W, terms), hf.split_partials(P, W, terms))
    dropped = {pair: rel(hf.split_partials(A, W, terms, drop=pair), hf.split_partials(P, W, terms, drop=pair)) for pair in hf.PAIRS[terms]}
    golden_only = {pair: float((np.abs(hf.split_partials(A, W, terms, drop=pair) - exact) / np.maximum(mag, 1e-300)).max()) for pair in hf.PAIRS[terms]}
    print("terms %d: ideal split %.3g, one pair left out %s (golden activations alone %s), bar %.3g"
          % (terms, ideal, {k: "%.3g" % v for k, v in dropped.items()}, {k: "%.3g" % v for k, v in golden_only.items()}, SPLIT_BAR))
    assert ideal <= SPLIT_BAR
    for pair, e in dropped.items():
        assert e > SPLIT_BAR, (pair, e)
    blind = sorted(pair for pair, e in golden_only.items() if e <= SPLIT_BAR)
    assert blind == ([(0, 2), (1, 1), (2, 0)] if terms == 3 else []), golden_only
    # the planted rows themselves: the float32 chain on them is no worse than on the golden rows (the bar is not stretched by them)
    assert float((np.abs(hf.head_partials(P, W).astype(np.float64) - p_exact) / p_mag).max()) <= hf.E_MIRROR
    if terms == 2:
        assert hf.h2_scale(W) == 2.0 ** round(np.log2(hf.h2_scale(W))) and 2.0 ** 13 <= np.abs(W).max() * hf.h2_scale(W) < 2.0 ** 14


@pytest.mark.parametrize("terms", [3, 2])
def test_nearest_sum_names_the_missing_pair(acts, head, mirror, terms):
    """The comparison tests/test_gpu_head.py::test_split_head_sums_every_term_pair makes, on the golden activations alone, with the float32 chain standing in
    for the device (its error is of the size of the matrix core's fp32 accumulation and as little aligned with any pair's products): the chain is nearer to
    the ideal sum of all pairs than to a sum without one; and the chain minus pair p's products - a kernel that leaves p out - is nearest to the sum without
    p, for every p, the three 2^-17 pairs included."""
    A, W = acts[0], head[0]
    part, mag = mirror[0].astype(np.float64), mirror[2]
    dist = lambda a, b: float(np.sqrt((((a - b) / np.maximum(mag, 1e-300)) ** 2).mean()))
    full = hf.split_partials(A, W, terms)
    without = {pair: hf.split_partials(A, W, terms, drop=pair) for pair in hf.PAIRS[terms]}
    d_full = dist(part, full)
    assert all(d_full < dist(part, w) for w in without.values())
    for pair, w in without.items():
        broken = part - (full - w)
        d = {q: dist(broken, v) for q, v in without.items()}
        assert min(d, key=d.get) == pair and d[pair] < dist(broken, full), (pair, d)
    print("terms %d: rms distance of the chain to the ideal sum %.3g, to the sums without one pair %s" % (terms, d_full, {k: "%.3g" % dist(part, w) for k, w in without.items()}))
