"""CPU: the image sizes at which tests/test_gpu_dense_edges.py runs the dense AffNet map (csrc/fullconv.hip), pinned to the constants
of that file.

Every kernel of fullconv.hip runs on arbitrary image sizes, and everything in it beyond the shared conv3x3_mfma* loops is edge logic:
32 / 16 / 8-pixel square input tiles (16-row rectangles for conv1 / conv2 of the split modes) with a 1-px apron whose out-of-image
reads become zeros, stores that skip pixels past Hout / Wout, two stride-2 layers whose last output row exists or not with the parity
of their input, and an 8 x 8 head that works in segments of FH_SEG = 57 outputs.  `dense_geom` below mirrors dense_geom() of
fullconv.hip; DENSE_EDGE_SIZES is the closed list the GPU test imports, and the tests here assert - from the mirror alone - that the
list reaches every residue class those constants make special, on the row axis and on the column axis separately.  A size may be
added to the list; a class may not be dropped."""
import ctypes as C
import re
import os

import pytest
import torch

import affnet_oracle as orc
import onepass_oracle as opo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FH_SEG = 57                      # fullconv.hip: outputs per head segment (64 loaded columns - 7)
MIN_SIDE = 34                    # affnet_fullconv_scratch_bytes: smallest accepted side

# (h, w, seed of orc.synthetic_image)          rows Hp/H2/H4/Hf   columns Wp/W2/W4/Wf
DENSE_EDGE_SIZES = (
    (34, 34, 11),                            # 62/31/16/9       same                the minimum accepted size; Hp even, H2 odd
    (36, 228, 12),                           # 64/32/16/9       256/128/64/57       every layer an exact multiple of its tile; Wf = one head segment
    (37, 229, 13),                           # 65/33/17/10      257/129/65/58       one row / column past the tile at every layer; Wf = a segment + 1; odd / odd
    (228, 36, 14),                           # transposes of the two above: row / column mix-ups; Hf = 57 / 58 (tail waves of the head's
    (229, 37, 15),                           # 4-row blocks: 57 = 14 x 4 + 1, 58 = 14 x 4 + 2)
    (35, 260, 16),                           # 63/32/16/9       288/144/72/65       Hp mod 32 = 31 with Wp mod 32 = 0; Hp odd, H2 even; second head segment 8 wide
    (260, 35, 17),                           # the transpose
)


def dense_geom(h, w):
    """dense_geom() of csrc/fullconv.hip: reflect padding by 14, two stride-2 3 x 3 convolutions with padding 1, the 8 x 8 valid head."""
    g = {"h": h, "w": w, "Hp": h + 28, "Wp": w + 28}
    g["H2"], g["W2"] = (g["Hp"] - 1) // 2 + 1, (g["Wp"] - 1) // 2 + 1
    g["H4"], g["W4"] = (g["H2"] - 1) // 2 + 1, (g["W2"] - 1) // 2 + 1
    g["Hf"], g["Wf"] = g["H4"] - 7, g["W4"] - 7
    return g


def locate(y, x, h, w):
    """Where pixel (y, x) of an h x w dense map comes from - for the failure messages of the GPU test.  The finish kernel reads
    ff[y0 .. y0 + 1][x0 .. x0 + 1] with src = (Hf / h)(y + 0.5) - 0.5 clamped at 0; ff row r is the head over rows r .. r + 7 of the
    H4 grid, whose rows come from rows ~2r of the H2 grid and ~4r of the Hp grid.  Returns a dict with the ff coordinate, the range of
    tile indices that window covers in the 32- (Hp), 16- (H2, also the split modes' 16-row tiles on Hp) and 8-pixel (H4) tilings per
    axis, and whether it touches the last tile row / column of a layer, the head's last segment or the head's last 4-row block."""
    g = dense_geom(h, w)
    out = {"pixel": (int(y), int(x))}
    for ax, p, n, nf, n4, n2, npad in (("y", y, h, g["Hf"], g["H4"], g["H2"], g["Hp"]), ("x", x, w, g["Wf"], g["W4"], g["W2"], g["Wp"])):
        src = max(float(nf) / n * (int(p) + 0.5) - 0.5, 0.0)
        f0 = min(int(src), nf - 1)
        f1 = min(f0 + 1, nf - 1)
        lo4, hi4 = f0, f1 + 7                                                    # rows / columns of the H4 grid under the head window
        lo2, hi2 = max(2 * lo4 - 1, 0), min(2 * hi4 + 1, n2 - 1)                  # 3 x 3, stride 2, padding 1
        lop, hip_ = max(2 * lo2 - 1, 0), min(2 * hi2 + 1, npad - 1)
        t8, t16, t32, t16p = (lo4 // 8, hi4 // 8), (lo2 // 16, hi2 // 16), (lop // 32, hip_ // 32), (lop // 16, hip_ // 16)
        out["ff_" + ax] = round(src, 3)
        out["tiles_" + ax] = {"8px(H4)": t8, "16px(H2)": t16, "32px(Hp)": t32, "16px(Hp, split modes)": t16p}
        out["in_last_tile_" + ax] = {"8px": t8[1] == (n4 - 1) // 8, "16px": t16[1] == (n2 - 1) // 16, "32px": t32[1] == (npad - 1) // 32}
        if ax == "x":
            out["head_segment"] = (f0 // FH_SEG, f1 // FH_SEG)
            out["in_head_last_segment"] = f1 // FH_SEG == (nf - 1) // FH_SEG
            out["head_segment_lane"] = (f0 % FH_SEG, f1 % FH_SEG)
        else:
            out["in_head_last_row_block"] = f1 // 4 == (nf - 1) // 4
    return out


def _axis_values(axis):
    return [dense_geom(h, w) for (h, w, _) in DENSE_EDGE_SIZES], ("H" if axis == 0 else "W")


@pytest.mark.parametrize("axis", [0, 1])
def test_edge_sizes_reach_every_class_on_each_axis(axis):
    geoms, A = _axis_values(axis)
    P, S2, S4, SF = [g[A + "p"] for g in geoms], [g[A + "2"] for g in geoms], [g[A + "4"] for g in geoms], [g[A + "f"] for g in geoms]
    # 32-pixel tiles of conv0 / conv1 / conv2: exactly full, one row / column over, one short
    assert {0, 1, 31} <= {p % 32 for p in P}, sorted({p % 32 for p in P})
    # 16-row tiles of conv1 / conv2 in the split modes
    assert {0, 1} <= {p % 16 for p in P}
    # 16-pixel tiles of conv3 / conv4
    assert {0, 1, 15} <= {s % 16 for s in S2}, sorted({s % 16 for s in S2})
    # 8-pixel tiles of conv5
    assert {0, 1} <= {s % 8 for s in S4}
    # both stride-2 layers: (input parity of conv2, input parity of conv4)
    assert {(p % 2, s % 2) for p, s in zip(P, S2)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the head: exactly one segment, and a second segment of one column (rows: the 4-row blocks' tail waves, 57 = 14 x 4 + 1)
    assert {FH_SEG, FH_SEG + 1} <= set(SF)
    assert any(FH_SEG + 1 < f < 2 * FH_SEG for f in SF), "a partial second head segment wider than one column"


def test_edge_sizes_include_the_minimum_and_stay_small():
    assert any(min(h, w) == MIN_SIDE for (h, w, _) in DENSE_EDGE_SIZES)
    assert (MIN_SIDE, MIN_SIDE) in [(h, w) for (h, w, _) in DENSE_EDGE_SIZES]
    assert all(MIN_SIDE <= min(h, w) and max(h, w) <= 260 for (h, w, _) in DENSE_EDGE_SIZES)
    assert len({(h, w) for (h, w, _) in DENSE_EDGE_SIZES}) == len(DENSE_EDGE_SIZES)
    # every size has its transpose in the list: what holds on one axis holds on the other
    assert {(h, w) for (h, w, _) in DENSE_EDGE_SIZES} == {(w, h) for (h, w, _) in DENSE_EDGE_SIZES}


def test_mirror_constants_are_the_kernel_file_s():
    src = open(os.path.join(ROOT, "affnet_amd", "csrc", "fullconv.hip")).read()
    assert re.search(r"#define FH_SEG %d\b" % FH_SEG, src)
    assert re.search(r"if \(h < %d \|\| w < %d\) return 0;" % (MIN_SIDE, MIN_SIDE), src)
    for frag in ("g.Hp = h + 28; g.Wp = w + 28;", "g.H2 = (g.Hp - 1) / 2 + 1; g.W2 = (g.Wp - 1) / 2 + 1;", "g.H4 = (g.H2 - 1) / 2 + 1; g.W4 = (g.W2 - 1) / 2 + 1;",
                 "g.Hf = g.H4 - 7; g.Wf = g.W4 - 7;"):
        assert frag in src, frag


def test_mirror_agrees_with_the_oracle_s_feature_shape(weights):
    for (h, w, seed) in DENSE_EDGE_SIZES:
        g = dense_geom(h, w)
        with torch.no_grad():
            norm, ff = opo.affnet_fullconv_features(weights["AffNet"], orc.synthetic_image(h, w, seed))
        assert tuple(norm.shape) == (1, 1, h, w)
        assert tuple(ff.shape) == (1, 3, g["Hf"], g["Wf"]), ((h, w), tuple(ff.shape), g)


def test_scratch_bytes_is_the_host_side_size_gate():
    """engine.fullconv_forward refuses a size by affnet_fullconv_scratch_bytes == 0, on the host, before any launch."""
    from affnet_amd import _lib
    f = _lib.lib.affnet_fullconv_scratch_bytes
    assert f(33, 34) == 0 and f(34, 33) == 0 and f(33, 64) == 0 and f(64, 33) == 0
    n = f(34, 34)
    g = dense_geom(34, 34)
    # normalised image + two ping-pong buffers of the largest activation tensor (16 x Hp x Wp floats), each aligned to 256 bytes
    assert 0 <= n - 4 * (34 * 34 + 2 * 16 * g["Hp"] * g["Wp"]) < 3 * 256
    for (h, w, _) in DENSE_EDGE_SIZES:
        g = dense_geom(h, w)
        assert f(h, w) >= 4 * (h * w + 2 * 16 * g["Hp"] * g["Wp"]), (h, w)


def test_locate_maps_corners_to_the_ends_of_every_tiling():
    h, w = 37, 229                                                               # Hf = 10, Wf = 58: second head segment of one column
    first, last = locate(0, 0, h, w), locate(h - 1, w - 1, h, w)
    assert first["ff_y"] == 0.0 and first["ff_x"] == 0.0 and first["head_segment"] == (0, 0)
    assert not first["in_head_last_segment"] and not first["in_last_tile_x"]["32px"]
    assert last["head_segment"] == (1, 1) and last["in_head_last_segment"] and last["head_segment_lane"] == (0, 0)
    assert last["in_head_last_row_block"] and all(last["in_last_tile_y"].values()) and all(last["in_last_tile_x"].values())
    assert last["tiles_x"]["32px(Hp)"][1] == 8 and last["tiles_x"]["16px(H2)"][1] == 8 and last["tiles_x"]["8px(H4)"][1] == 8
