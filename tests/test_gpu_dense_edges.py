"""GPU (run with -m gpu on an MI355X): csrc/fullconv.hip at the image sizes where its edge logic decides - tile-exact and tile-plus-one
extents of every layer's tiling, all four parities of the two stride-2 layers, head widths of one segment / a segment plus one column,
and the smallest accepted image (tests/test_dense_geometry.py holds the list and proves what it reaches) - plus LocalNorm2d and NMS2d
at the borders of their own tilings.

References, all run live: oracle/onepass_oracle.py (pinned bit for bit to the reference's classes).  Bars are the project's existing
ones (tests/test_gpu_onepass.py): dense map max |got - want| < 5e-5 over EVERY element with channel 1 exactly 0, LocalNorm2d within
1e-6, NMS2d bit-equal.  On the sizes used here the fp32 oracle of the dense map lies within 3e-7 of a float64 evaluation of the same
network from the same normalised image (float64 trunk, head, interpolation, tanh, rectification; measured on the CPU) - under 1 % of
the bar, so a pass is no accident of a loose tolerance and a failure is not reference noise."""
import numpy as np
import pytest
import torch

import affnet_oracle as orc
import onepass_oracle as opo
from conftest import record_parity
from test_dense_geometry import DENSE_EDGE_SIZES, dense_geom, locate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITH = ["fp32", "fp32_split3", "fp32_split2h"]
BAR = 5e-5


@pytest.fixture(scope="module")
def amd():
    import affnet_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return affnet_amd


@pytest.fixture(scope="module")
def FC(amd, weights):
    net = amd.AffNetFastFullConv()
    net.load_state_dict(weights["AffNet"])
    return net.to(DEV)


_DENSE_ORACLE = {}            # (h, w, seed) -> (image, oracle map): shared by the arithmetic-mode parametrisation, never modified


def _oracle(weights, h, w, seed):
    if (h, w, seed) not in _DENSE_ORACLE:
        x = orc.synthetic_image(h, w, seed)
        with torch.no_grad():
            want = opo.affnet_fullconv_forward(weights["AffNet"], x).numpy()
        want.setflags(write=False)
        _DENSE_ORACLE[(h, w, seed)] = (x, want)
    return _DENSE_ORACLE[(h, w, seed)]


def _describe_worst(d, h, w):
    c, y, x = np.unravel_index(int(np.argmax(d[0])), d[0].shape)
    where = locate(y, x, h, w)
    bad = d[0].max(axis=0) >= BAR
    ys, xs = np.nonzero(bad)
    box = "none" if not len(ys) else "rows %d..%d, columns %d..%d (%d pixels)" % (ys.min(), ys.max(), xs.min(), xs.max(), len(ys))
    return "worst %.3g at channel %d, pixel (y %d, x %d) of %dx%d (h x w); geometry %s; pixels over the bar: %s; source: %s" % (
        d[0, c, y, x], c, y, x, h, w, dense_geom(h, w), box, where)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("h,w,seed", DENSE_EDGE_SIZES, ids=["%dx%d" % (h, w) for (h, w, _) in DENSE_EDGE_SIZES])
def test_dense_map_at_edge_sizes(FC, weights, h, w, seed, arith):
    x, want = _oracle(weights, h, w, seed)
    FC.arith = arith
    try:
        got = FC(x.to(DEV)).cpu().numpy()
    finally:
        FC.arith = "fp32"
    assert got.shape == want.shape == (1, 4, h, w)
    assert np.isfinite(got).all(), "non-finite values in the map at %s" % (np.argwhere(~np.isfinite(got))[:4].tolist(),)
    d = np.abs(got - want)
    print("dense map %dx%d (h x w) [%s]: max_abs_diff_vs_oracle %.4g" % (h, w, arith, d.max()))
    record_parity("AffNetFastFullConv dense map, edge size %dx%d%s" % (w, h, "" if arith == "fp32" else " [arith %s]" % arith),
                  max_abs_diff_vs_oracle=float(d.max()), elements=int(d.size))
    assert d.max() < BAR, _describe_worst(d, h, w)                     # every element: no percentile, no mask
    assert np.all(got[0, 1] == 0.0)                                     # a12 = 0 * det


@pytest.mark.parametrize("h,w", [(33, 64), (64, 33)])
def test_one_pixel_below_the_minimum_is_refused_on_the_host(FC, h, w):
    """The library requires 34 px per side (the reference's LocalNorm2d(33) needs 17); 34 x 34 itself runs in the test above.  The
    refusal is affnet_fullconv_scratch_bytes == 0 in engine.fullconv_forward: no kernel is launched."""
    from affnet_amd import _lib
    assert _lib.lib.affnet_fullconv_scratch_bytes(h, w) == 0
    with pytest.raises(ValueError, match="too small"):
        FC(torch.zeros(1, 1, h, w, device=DEV))


def _check_local_norm(x, name):
    from affnet_amd import engine
    got = engine.local_norm(x.to(DEV)).cpu().numpy()[0, 0]
    want = opo.local_norm2d(x).numpy()[0, 0]
    assert got.shape == want.shape and np.isfinite(got).all()
    d = np.abs(got - want)
    print("LocalNorm2d(33) %s: max_abs_diff_vs_oracle %.4g, %d of %d differ" % (name, d.max(), int((d > 0).sum()), d.size))
    record_parity("LocalNorm2d(33) edge size " + name, max_abs_diff_vs_oracle=float(d.max()), mismatching_vs_oracle=int((d > 0).sum()), elements=int(d.size))
    y, xx = np.unravel_index(int(np.argmax(d)), d.shape)
    assert d.max() <= 1e-6, "LocalNorm2d %s differs from the oracle by %g at (y %d, x %d): got %r, want %r" % (name, d.max(), y, xx, got[y, xx], want[y, xx])
    return got, want


# 17 x 17: the minimum - every window reflects on both sides and reflect_idx reaches index 0 and n - 1 from outside; 64 x 65 / 65 x 64: one
# row / column past the LN_T = 64 tile forms a tile of its own; 17 x 130: three tiles of the minimum height, the last two columns wide
@pytest.mark.parametrize("h,w,seed", [(17, 17, 21), (64, 65, 22), (65, 64, 23), (17, 130, 24)])
def test_local_norm_at_tile_edges_and_minimum(amd, h, w, seed):
    got, want = _check_local_norm(orc.synthetic_image(h, w, seed), "%dx%d" % (w, h))
    assert np.abs(want).max() > 1.0                                     # the comparison is not one of two flat images


def test_local_norm_saturated_block(amd):
    """Integer-valued 80 x 80 image with a 40 x 40 block at 255: a 33 x 33 window wholly inside the block sums 1089 x 255 exactly
    (< 2^24), so x - mean is 0 whatever rounding residue sum(x^2) / 1089 - mean^2 leaves (65025 x 1089 > 2^24): the output is exactly 0
    there, in the reference and in the kernel."""
    g = torch.Generator().manual_seed(25)
    x = torch.randint(0, 255, (1, 1, 80, 80), generator=g).float()
    x[0, 0, 20:60, 20:60] = 255.0
    got, want = _check_local_norm(x, "80x80 saturated block")
    inside = (slice(36, 44), slice(36, 44))                             # centres whose window is rows / columns 20 .. 59 at the most
    assert np.all(want[inside] == 0.0) and np.all(got[inside] == 0.0), (want[inside], got[inside])
    assert np.abs(got[0:20]).max() > 0.5


@pytest.mark.parametrize("h,w", [(12, 40), (16, 40), (40, 16)])
def test_local_norm_refuses_what_cannot_be_reflect_padded(amd, h, w):
    from affnet_amd import engine
    with pytest.raises(Exception, match="too small"):
        engine.local_norm(torch.zeros(1, 1, h, w, device=DEV))           # reflect padding of 16 needs >= 17 px


def _nms_input(h, w, seed):
    """Seeded values in (-1, 1) with 2 x 2 plateaus of one value above all of them (clipped to the image): at the top left corner, at
    the bottom right corner, across the kernel's 64-column block boundary and across its 4-row block boundary.  x - max + 1e-5 > 0 keeps all
    four members of a plateau."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, 1, h, w, generator=g) * 2.0 - 1.0
    member = torch.zeros(h, w, dtype=torch.bool)
    for (y0, x0) in ((0, 0), (h - 2, w - 2), (h // 2 - 1, 63), (3, w // 3), (h - 2, 2 * (w // 3))):
        member[max(y0, 0):max(y0, 0) + 2, max(x0, 0):max(x0, 0) + 2] = True        # slices clip at the image border
    x[0, 0][member] = 1.5
    return x, member


@pytest.mark.parametrize("th", [0.0, 0.5])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 65), (5, 64), (4, 65), (3, 130)])
def test_nms2d_at_block_edges(amd, h, w, th):
    from affnet_amd.HandCraftedModules import NMS2d
    x, member = _nms_input(h, w, 30 + h + w)
    assert member[0, 0] and member[h - 1, w - 1]
    got = NMS2d(threshold=th)(x.to(DEV)).cpu()
    want = opo.nms2d(x, th)
    assert torch.equal(got, want), "NMS2d(threshold=%g) differs at %s" % (th, torch.nonzero(got != want)[:8].tolist())
    assert torch.equal(got[0, 0][member], x[0, 0][member]), "a plateau member was suppressed"
    kept = got[0, 0] > 0
    assert bool(kept[h - 1].any()) and bool(kept[:, w - 1].any())
    if h * w > 64:
        assert int(kept.sum()) > int(member.sum())                      # maxima besides the planted ones
        assert int((got[0, 0] == 0).sum()) > 0
