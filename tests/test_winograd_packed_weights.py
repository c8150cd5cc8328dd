"""The packed HardNet blob carries the Winograd F(2x2, 3x3) weights U = G g G^T of conv1 / conv3 / conv5 as its LAST section
(include/affnet_hip.h, NetLayout::w_wino): bitwise the Python mirror's U in the kernel's fragment order, behind a prefix that is
byte for byte the blob of the library before that section existed; the other networks' blobs are unchanged.  CPU only."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import winograd_numerics as wn  # noqa: E402

# blob sizes (floats) and SHA-256 of the blobs that the library packed BEFORE the Winograd section was added (synthetic HardNet state 0,
# shipped AffNet / OriNet checkpoints; kind 3 = AffNetFastFullConv on the AffNet checkpoint), recorded from that library
OLD = {
    0: (264632, "5b1639d9a43ee57782de87a6dbff52dc4b6ef6f7aa0716acfaeb69cbb308d894"),
    1: (260536, "6e8605deaa6fda2724511f5b8af06467ba4754b0a5dbf86f9d62132b151234be"),
    2: (4670936, "21db96b37c7132e66f4c3f86271e64de7c845b543f746d2b8c0866289d57a823"),
    3: (268728, "544dcf0d07ca5f5665f8dd733bdc73d5c1aa14f98b12307cb5c1f402f375fa28"),
}
WINO_SHAPES = {1: (32, 32), 3: (64, 64), 5: (128, 128)}          # layer: (cin, cout)


def _old_total(kind):
    """Size of the blob without the Winograd section, from the layout rules (trunk + head + three-term + two-term copies)."""
    cb = 32 if kind == 2 else 16
    ch = [1, cb, cb, 2 * cb, 2 * cb, 4 * cb, 4 * cb]
    off = 0
    for i in range(6):
        off += 12 * ch[1] if i == 0 else 9 * ch[i] * ch[i + 1]
        off = (off + ch[i + 1] + 3) & ~3
    off += {0: 3 * 4096 + 4, 1: 2 * 4096 + 4, 2: 8192 * 128 + 128, 3: 8 * 64 * 32 + 4}[kind]
    s3 = lambda ci, co, terms: (5 if ci == 16 else 9 * (ci // 32)) * terms * 4 * co * 4
    off += sum(s3(ch[i], ch[i + 1], 3) for i in range(1, 6))
    if kind == 2:
        off += 8192 * 128 * 3 // 2
    off += sum(s3(ch[i], ch[i + 1], 2) + 4 for i in range(1, 6))
    if kind == 2:
        off += 8192 * 128 + 4
    return off


def _sha(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def test_layout_rule_reproduces_the_old_sizes():
    for kind, (n, _) in OLD.items():
        assert _old_total(kind) == n, kind


@pytest.mark.parametrize("kind,name", [(0, "AffNet"), (1, "OriNet"), (3, "AffNet")])
def test_other_networks_blobs_are_unchanged(kind, name, weights):
    from affnet_amd import _lib, engine
    assert _lib.lib.affnet_cnn32_packed_floats(kind) == OLD[kind][0]
    blob = engine.pack_state_dict(kind, weights[name], winograd=True)
    assert blob.numel() == OLD[kind][0] and _sha(blob) == OLD[kind][1]
    assert torch.equal(engine.pack_state_dict(kind, weights[name]), blob)
    for layer in range(-1, 7):
        assert _lib.lib.affnet_cnn32_winograd_offset(kind, layer) == -1


def test_hardnet_winograd_section_offsets():
    from affnet_amd import _lib
    off = OLD[2][0]                                                # appended: the first section starts at the old total
    for layer in range(6):
        got = _lib.lib.affnet_cnn32_winograd_offset(2, layer)
        if layer in WINO_SHAPES:
            ci, co = WINO_SHAPES[layer]
            assert got == off and got % 4 == 0, (layer, got, off)
            off += 16 * ci * co
        else:
            assert got == -1, (layer, got)
    assert _lib.lib.affnet_cnn32_packed_floats(2) == off == OLD[2][0] + 16 * 21504
    assert _lib.lib.affnet_cnn32_winograd_offset(2, 6) == -1 and _lib.lib.affnet_cnn32_winograd_offset(9, 1) == -1


def test_hardnet_prefix_is_the_old_blob(weights):
    """Every section that existed before sits where it sat and holds what it held: the prefix up to the old total is the old blob."""
    from affnet_amd import _lib, engine
    blob = engine.pack_state_dict(2, weights["HardNet"], winograd=True)
    assert blob.numel() == _lib.lib.affnet_cnn32_packed_floats(2)
    assert _sha(blob[:OLD[2][0]]) == OLD[2][1]
    # the weight sections alone (the default of pack_state_dict) are that prefix
    assert torch.equal(engine.pack_state_dict(2, weights["HardNet"]), blob[:OLD[2][0]])
    # and the fp32 tap copies of the Winograd layers are still what the split modes / debug paths read: the folded taps in tap order
    ch = [1, 32, 32, 64, 64, 128, 128]
    off = 0
    for i in range(6):
        ci, co = ch[i], ch[i + 1]
        n = 12 * co if i == 0 else 9 * ci * co
        if i in WINO_SHAPES:
            W = blob[off:off + n].view(9, ci // 16, 4, co, 4).permute(3, 1, 2, 4, 0).reshape(co, ci, 3, 3)
            assert np.array_equal(W.numpy().view(np.uint32), wn.packed_taps(weights["HardNet"], i).numpy().view(np.uint32)), i
        off = (off + n + co + 3) & ~3


@pytest.mark.parametrize("state,sha", [(0, "6882f2dcf7bc036b1101dc33e64021f4447bd9c4ac532be332f82f5084941b79"),
                                       (3, "1079eb2a5c9e38196e295022772c9743531b3ec4d2a830920d56487af746c726")])
def test_whole_hardnet_blob_is_pinned(state, sha):
    """Every section of the HardNet blob, the split copies of the head and the Winograd section included, byte for byte what the library
    packed before the packer became a host-only unit (weights_pack.hip; hashes recorded from that library)."""
    from affnet_amd import engine
    import affnet_oracle as orc
    blob = engine.pack_state_dict(2, orc.synthetic_hardnet_state(state), winograd=True)
    assert blob.numel() == 5015000 and _sha(blob) == sha


def test_hardnet_winograd_sections_are_bitwise_the_mirror(weights):
    """U in the blob == tools/winograd_numerics.py: weight_transform of the BN-folded fp32 taps (the operation order of the loop that used
    to compute it per K group; taps folded with the packer's roundings, packed_taps), bit for bit, in [xi][cin/16][(c/4)%4][cout][c%4]."""
    from affnet_amd import _lib, engine
    blob = engine.pack_state_dict(2, weights["HardNet"], winograd=True).numpy()
    want = wn.packed_weight_transform(weights["HardNet"])
    assert sorted(want) == sorted(WINO_SHAPES)
    for layer, (ci, co) in WINO_SHAPES.items():
        off = _lib.lib.affnet_cnn32_winograd_offset(2, layer)
        got = blob[off:off + 16 * ci * co]
        w = want[layer].numpy()
        assert w.dtype == np.float32 and w.shape == got.shape
        diff = np.flatnonzero(got.view(np.uint32) != w.view(np.uint32))
        assert diff.size == 0, (layer, diff.size, diff[:4], got[diff[:4]], w[diff[:4]])
        # spot check of the layout against the [4][4][co][ci] form: position xi = 4 i + j, input channel c, output channel n
        U = wn.weight_transform(wn.packed_taps(weights["HardNet"], layer)).numpy()
        g = got.reshape(16, ci // 16, 4, co, 4)
        for xi, c, n in ((0, 0, 0), (5, 17, 3), (10, ci - 1, co - 1), (15, 6, co // 2)):
            assert g[xi, c // 16, (c // 4) % 4, n, c % 4] == U[xi // 4, xi % 4, n, c]


def test_winograd_sections_keep_what_the_transform_cannot_round():
    """Corner taps pass through G g G^T untouched (U[0], U[3], U[12], U[15] are g[0][0], g[0][2], g[2][0], g[2][2]): checked on the blob
    against its own tap copy, an identity that holds whatever the weights are."""
    from affnet_amd import _lib, engine
    import affnet_oracle as orc
    blob = engine.pack_state_dict(2, orc.synthetic_hardnet_state(3), winograd=True).numpy()
    ch = [1, 32, 32, 64, 64, 128, 128]
    off = 0
    for i in range(6):
        ci, co = ch[i], ch[i + 1]
        n = 12 * co if i == 0 else 9 * ci * co
        if i in WINO_SHAPES:
            taps = blob[off:off + n].reshape(9, -1)
            wo = _lib.lib.affnet_cnn32_winograd_offset(2, i)
            U = blob[wo:wo + 16 * ci * co].reshape(16, -1)
            for xi, tap in ((0, 0), (3, 2), (12, 6), (15, 8)):
                assert np.array_equal(U[xi].view(np.uint32), taps[tap].view(np.uint32)), (i, xi)
        off = (off + n + co + 3) & ~3
