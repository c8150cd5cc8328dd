"""The split-K head GEMMs on the MI355X against their float32 restatement (tests/_head_fp32.py, pinned on the host by tests/test_head_mirror_host.py), on the
bytes: hardnet_head_kernel<MP>, hardnet_head_s3_kernel<MP, TERMS>, hardnet_finish_kernel and the dispatch of aff_hardnet_head (csrc/cnn_heads.hip), and
tfeat_head_kernel (csrc/tfeat.hip).  Every call goes through affnet_cnn32_forward / _forward_pyr / affnet_tfeat_forward with torch-owned buffers: the whole
scratch pre-filled with a NaN pattern, guard rows behind d_out.  The head's input is read back from the scratch (the trunk tensor [row][K], k = pixel *
channels + channel), its split-K partials from behind it ([quarter][row][128]); the mirror runs on exactly those floats and the floats of the uploaded blob.

Which of the nine head instantiations a test runs (MP forced through AFFNET_HEAD_MP, which the launcher reads per launch, except where noted):
  test_exact_head_on_the_bytes            hardnet_head_kernel<16>, <32>, <64>
  test_shape_invariance                   all nine: hardnet_head_kernel<16 / 32 / 64>, hardnet_head_s3_kernel<16 / 32 / 64, 3>, hardnet_head_s3_kernel<16 / 32 / 64, 2>
  test_split_head_sums_every_term_pair    hardnet_head_s3_kernel<16, 3>, <16, 2>
  test_natural_dispatch                   no variable set: 2016 rows <16>, 2017 and 4032 rows <32>, 4033 rows <64>
  test_count_semantics                    hardnet_head_kernel<16>, <32>, <64>
  test_batch_of_two_images                no variable set: hardnet_head_kernel<32> (B = 2, 1000 rows per image) against <16> (the patches form, one image)
  test_row_limit                          no variable set: hardnet_head_kernel<64> at 65535 rows
Exact mode: np.array_equal on the raw bits, no mask, no percentile.  Split modes: the partials within 8 x E_mirror of float64 on sum |a| |w| (the bar whose
sensitivity the host test shows), the descriptors = hardnet_finish(device partials) on the bytes (the finish kernel is the same fp32 code in every mode).

Measured on an MI355X (130 rows, worst |device - float64| / sum |a| |w| on the device's own trunk tensor; bar 1.94e-06): exact 2.62e-07, three bf16 terms
3.44e-07, two fp16 terms 2.51e-07; rms distance to the ideal sum of all term pairs 3.52e-08 / 2.67e-08, to the nearest sum without one pair 1.37e-07 /
1.12e-05.  The 65535-row call with the read-back of its partials and descriptors: 0.08 s."""
import os
import time

import numpy as np
import pytest
import torch

import _head_fp32 as hf
from _fp32_chain import F32, noise_image
from _tfeat_fp64 import load_golden_weights
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FC0BEEF                    # a quiet NaN no kernel produces
GUARD = 3                                # rows behind n_max in d_out
ARITHS = ["fp32", "fp32_split3", "fp32_split2h"]
SPLIT_BAR = 8.0 * hf.E_MIRROR


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class forced_mp(object):
    """AFFNET_HEAD_MP set for the calls inside, restored behind them (in-process: the launcher calls getenv per launch)."""

    def __init__(self, mp):
        self.mp = mp

    def __enter__(self):
        self.old = os.environ.get("AFFNET_HEAD_MP")
        if self.mp is None:
            os.environ.pop("AFFNET_HEAD_MP", None)
        else:
            os.environ["AFFNET_HEAD_MP"] = str(self.mp)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("AFFNET_HEAD_MP", None)
        else:
            os.environ["AFFNET_HEAD_MP"] = self.old


@pytest.fixture(scope="module")
def hard(weights):
    """(packed blob on the device, W (8192, 128), bias) of the synthetic HardNet: the mirror's weights are read out of the blob the kernels read."""
    import affnet_amd
    net = affnet_amd.HardNet()
    net.load_state_dict(weights["HardNet"])
    packed = net.to(DEV).packed_weights(torch.device(DEV))
    W, bias = hf.unpack_head(packed.cpu().numpy(), "hardnet")
    return packed, W, bias


def sentinel_buffer(n_int32):
    return torch.full((int(n_int32),), SENTINEL, dtype=torch.int32, device=DEV)


def run_hardnet(hard, patches, n_max, arith="fp32", mp=None, count=None, read_trunk=True):
    """affnet_cnn32_forward(HardNet) on `patches` (torch, device, (n_max, 32, 32)): dict(rc, trunk (n_max, 8192), part (4, n_max, 128), out (n_max + GUARD, 128),
    all numpy float32 views of what the call left in the sentinel-filled buffers)."""
    from affnet_amd import _lib, engine
    from affnet_amd._lib import lib, ptr
    dev = torch.device(DEV)
    ctx = engine.utility_ctx(dev, arith)
    scratch = sentinel_buffer(n_max * (hf.HARDNET_K + 512))
    out = sentinel_buffer((n_max + GUARD) * 128)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    with forced_mp(mp):
        rc = lib.affnet_cnn32_forward(ctx, _lib.NET_HARDNET, ptr(hard[0]), ptr(patches), None if cnt is None else ptr(cnt), n_max, ptr(out.view(torch.float32)),
                                      ptr(scratch.view(torch.float32)), engine.stream_of(dev))
    torch.cuda.synchronize()
    res = dict(rc=rc, ctx=ctx, out=out.cpu().numpy().view(F32).reshape(n_max + GUARD, 128), scratch=scratch)
    res["part"] = scratch[n_max * hf.HARDNET_K:].cpu().numpy().view(F32).reshape(4, n_max, 128)
    if read_trunk:
        res["trunk"] = scratch[:n_max * hf.HARDNET_K].cpu().numpy().view(F32).reshape(n_max, hf.HARDNET_K)
    return res


_MIRROR = {}


def mirror_rows(trunk, W, tag="hardnet"):
    """head_partials of the rows of `trunk`, (4, n, 128): computed once per distinct row (the tiled patch set repeats its 80 rows)."""
    keys = [(tag, r.tobytes()) for r in trunk]
    todo = {}
    for i, k in enumerate(keys):
        if k not in _MIRROR and k not in todo:
            todo[k] = i
    if todo:
        idx = list(todo.values())
        part = hf.head_partials(trunk[idx], W)
        for j, k in enumerate(todo):
            _MIRROR[k] = part[:, j].copy()
    return np.stack([_MIRROR[k] for k in keys], axis=1) if keys else np.zeros((4, 0, 128), F32)


_PATCHES = {}


def device_patches(n):
    if n not in _PATCHES:
        _PATCHES[n] = torch.from_numpy(hf.tiled_patches(n)).to(DEV)
    return _PATCHES[n]


_RUNS = {}


def tile_run(hard, arith, mp, n):
    key = (arith, mp, n)
    if key not in _RUNS:
        r = run_hardnet(hard, device_patches(n), n, arith, mp)
        assert r["rc"] == 0
        r.pop("scratch")
        _RUNS[key] = r
    return _RUNS[key]


def check_untouched(r, n_max, count):
    """What the head leaves alone: guard rows of d_out and partial rows >= count keep the sentinel; d_out rows >= count are exactly 0."""
    assert np.all(bits(r["out"][n_max:]) == SENTINEL), "guard rows of d_out were written"
    assert np.all(bits(r["out"][count:n_max]) == 0), "d_out rows past the count are not exactly 0"
    assert np.all(bits(r["part"][:, count:]) == SENTINEL), "partial rows past the count were written"
    assert not np.any(bits(r["part"][:, :count]) == SENTINEL) and not np.any(bits(r["out"][:count]) == SENTINEL)


@pytest.mark.parametrize("n", hf.N_ROWS)
@pytest.mark.parametrize("mp", [16, 32, 64])
def test_exact_head_on_the_bytes(hard, mp, n):
    _, W, bias = hard
    r = tile_run(hard, "fp32", mp, n)
    check_untouched(r, n, n)
    assert not np.any(bits(r["trunk"]) == SENTINEL)
    want = mirror_rows(r["trunk"], W)
    assert same(r["part"], want), "hardnet_head_kernel<%d>, %d rows: %d partials differ from the fmaf chains" % (mp, n, int((bits(r["part"]) != bits(want)).sum()))
    assert same(r["out"][:n], hf.hardnet_finish(r["part"], bias))
    if n >= 80:         # the constant patches share one descriptor, and the tiled rows repeat the first 80
        for c in hf.CONSTANT_ROWS[1:]:
            assert same(r["out"][c], r["out"][hf.CONSTANT_ROWS[0]])
        assert same(r["out"][80:n], r["out"][:n - 80])


@pytest.mark.parametrize("n", hf.N_ROWS)
@pytest.mark.parametrize("arith", ARITHS)
def test_shape_invariance(hard, arith, n):
    """MP 16 / 32 / 64 leave the same bytes in every arithmetic mode; split modes: partials within 8 x E_mirror of float64 on the device's own trunk tensor."""
    _, W, bias = hard
    runs = [tile_run(hard, arith, mp, n) for mp in (16, 32, 64)]
    for r in runs:
        check_untouched(r, n, n)
        assert same(r["trunk"], runs[0]["trunk"])
        assert same(r["part"], runs[0]["part"]), "the partials depend on the patches per workgroup"
        assert same(r["out"], runs[0]["out"])
        assert same(r["out"][:n], hf.hardnet_finish(r["part"], bias))
    exact, mag = hf.exact_partials(runs[0]["trunk"], W)
    err = float((np.abs(runs[0]["part"].astype(np.float64) - exact) / np.maximum(mag, 1e-300)).max())
    print("head partials, %s, %d rows: worst |device - float64| / sum |a| |w| = %.3g (bar %.3g)" % (arith, n, err, SPLIT_BAR))
    if n == max(hf.N_ROWS):
        record_parity("HardNet head partials vs float64 on the device's trunk tensor, %s, %d rows" % (arith, n), rel_to_sum_abs=err, bar=SPLIT_BAR, e_mirror=hf.E_MIRROR)
    assert err <= SPLIT_BAR
    if arith != "fp32":
        assert not same(runs[0]["part"], tile_run(hard, "fp32", 16, n)["part"]), "arith %s did not switch the head kernel" % arith


@pytest.mark.parametrize("arith,terms", [("fp32_split3", 3), ("fp32_split2h", 2)])
def test_split_head_sums_every_term_pair(hard, arith, terms):
    """What the 8 x E_mirror bar cannot see on real activations (the three 2^-17 pairs of the three-term mode), without a bar: over the 4 x 130 x 128 partials
    the device's sums lie nearer (L2 of the error over sum |a| |w|) to the ideal sum of ALL term pairs than to the ideal sum without any one of them.  A
    kernel that leaves pair p out differs from "all but p" by its fp32 accumulation alone and from "all" by that and p's products, which the accumulation
    errors do not line up with: the comparison needs no threshold.  The tile shape does not matter here (test_shape_invariance: the same bytes)."""
    _, W, _ = hard
    r = tile_run(hard, arith, 16, max(hf.N_ROWS))
    _, mag = hf.exact_partials(r["trunk"], W)
    dev = r["part"].astype(np.float64)
    dist = lambda p: float(np.sqrt((((dev - p) / np.maximum(mag, 1e-300)) ** 2).mean()))
    full = dist(hf.split_partials(r["trunk"], W, terms))
    without = {pair: dist(hf.split_partials(r["trunk"], W, terms, drop=pair)) for pair in hf.PAIRS[terms]}
    print("%s: rms distance to the ideal sum %.3g, to the sums without one pair %s" % (arith, full, {k: "%.3g" % v for k, v in without.items()}))
    record_parity("HardNet head, %s: rms distance of the partials to the ideal split sum and to the sums without one term pair" % arith, all_pairs=full,
                  **{"without_%d_%d" % k: v for k, v in without.items()})
    for pair, d in without.items():
        assert full < d, "the partials are nearer to the sum without pair %s (%.3g) than to the sum of all pairs (%.3g)" % (pair, d, full)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("n_max,mp", [(2016, 16), (2017, 32), (4032, 32), (4033, 64)])
def test_natural_dispatch(hard, n_max, mp, full):
    """No variable set: the launcher's own choice at both ends of the range in which one image takes the 32-patch shape.  2017 and 4033 leave one row in the
    last 32- / 64-row tile.  count = 70 (six rows into a tile of every shape) and count = n_max."""
    _, W, bias = hard
    assert "AFFNET_HEAD_MP" not in os.environ
    assert hf.head_mp(n_max, 1) == mp
    count = n_max if full else 70
    r = run_hardnet(hard, device_patches(n_max), n_max, count=count)
    assert r["rc"] == 0
    check_untouched(r, n_max, count)
    rows = hf.edge_rows(count)                      # first, last, both sides of every 16 / 32 / 64-row tile edge below the count
    assert rows[0] == 0 and rows[-1] == count - 1 and {63, 64} <= set(rows) and (count % 32 != 1 or count - 2 in rows)
    want = mirror_rows(r["trunk"][rows], W)
    assert same(r["part"][:, rows], want)
    assert same(r["out"][:count], hf.hardnet_finish(r["part"][:, :count], bias))
    if count > 80:                                  # the tiled rows repeat the first 80
        assert same(r["part"][:, 80:count], r["part"][:, :count - 80]), "a row's partials depend on its position"


@pytest.mark.parametrize("count", [0, 1, 70, 75])
@pytest.mark.parametrize("mp", [16, 32, 64])
def test_count_semantics(hard, mp, count):
    """n_max = 70, a device count of 0, 1, n_max and n_max + 5 (clamped): rows >= count of d_out exactly 0, of the partial area untouched, guard rows untouched."""
    _, W, bias = hard
    n_max = 70
    r = run_hardnet(hard, device_patches(n_max), n_max, mp=mp, count=count)
    assert r["rc"] == 0
    n = min(count, n_max)
    check_untouched(r, n_max, n)
    assert np.all(bits(r["trunk"][n:]) == SENTINEL), "trunk rows past the count were written"
    assert same(r["part"][:, :n], mirror_rows(r["trunk"][:n], W))
    assert same(r["out"][:n], hf.hardnet_finish(r["part"][:, :n], bias))
    assert same(r["out"][:n], tile_run(hard, "fp32", 16, 130)["out"][:n])          # a row does not depend on the count


@pytest.mark.parametrize("counts", [(1000, 517), (0, 993), (33, 1005)])
def test_batch_of_two_images(hard, counts):
    """B = 2, n_max = 1000 (32 x 4 x 2 = 256 workgroups: the 32-patch shape) through affnet_cnn32_forward_pyr with ragged counts (0 for one image in one case,
    a count above n_max in another) against the patches form (one image, the 16-patch shape) on the patches affnet_pyr_grid_sample returns for the same frames."""
    from affnet_amd import _lib, engine
    from affnet_amd._lib import lib, check, ptr
    _, W, bias = hard
    B, n_max, h, w = 2, 1000, 96, 128
    assert hf.head_mp(n_max, B) == 32 and "AFFNET_HEAD_MP" not in os.environ
    dev = torch.device(DEV)
    ctx = engine.Context(h, w, dev, 3, 1.6, 5, 5.192, 0.0, 60, 60, batch=B)
    st = engine.stream_of(dev)
    x = torch.from_numpy(np.stack([noise_image(h, w, s) for s in (3, 4)])).to(DEV).contiguous()
    check(lib.affnet_pyramid_build(ctx.handle, ptr(x), st), ctx.handle, "affnet_pyramid_build")
    rng = np.random.default_rng(7)
    ang, sc = rng.uniform(0, 2 * np.pi, (B, n_max)), rng.uniform(0.08, 0.3, (B, n_max))
    lafs = np.zeros((B, n_max, 2, 3), F32)
    lafs[..., 0, 0], lafs[..., 0, 1], lafs[..., 1, 0], lafs[..., 1, 1] = sc * np.cos(ang), -sc * np.sin(ang), 1.3 * sc * np.sin(ang), 1.3 * sc * np.cos(ang)
    lafs[..., 2] = rng.uniform(0.05, 0.95, (B, n_max, 2))                       # some frames reach over the border (zero padding)
    ids = np.zeros((B, n_max, 3), np.int32)
    ids[..., 0], ids[..., 1] = rng.integers(0, len(ctx.plan.sizes), (B, n_max)), rng.integers(0, ctx.plan.levels_per_octave, (B, n_max))
    d_lafs, d_ids = torch.from_numpy(lafs).to(DEV), torch.from_numpy(ids).to(DEV)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    scratch = sentinel_buffer(B * n_max * (hf.HARDNET_K + 512))
    out = sentinel_buffer((B * n_max + GUARD) * 128)
    check(lib.affnet_cnn32_forward_pyr(ctx.handle, _lib.NET_HARDNET, ptr(hard[0]), ptr(d_lafs), ptr(d_ids), ptr(cnt), n_max, ptr(out.view(torch.float32)),
                                       ptr(scratch.view(torch.float32)), st), ctx.handle, "affnet_cnn32_forward_pyr")
    patches = torch.zeros(B, n_max, 32, 32, dtype=torch.float32, device=DEV)
    check(lib.affnet_pyr_grid_sample(ctx.handle, ptr(d_lafs), ptr(d_ids), None, n_max, 32, ptr(patches), st), ctx.handle, "affnet_pyr_grid_sample")
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(F32).reshape(B * n_max + GUARD, 128)
    part = scratch[B * n_max * hf.HARDNET_K:].cpu().numpy().view(F32).reshape(4, B, n_max, 128)
    assert np.all(bits(o[B * n_max:]) == SENTINEL)
    for b in range(B):
        n = min(counts[b], n_max)
        ob = o[b * n_max:(b + 1) * n_max]
        assert np.all(bits(ob[n:]) == 0) and np.all(bits(part[:, b, n:]) == SENTINEL), "image %d: rows past its count" % b
        if n == 0:
            continue
        one = run_hardnet(hard, patches[b, :n].contiguous(), n)
        assert one["rc"] == 0 and hf.head_mp(n, 1) == 16
        assert same(part[:, b, :n], one["part"]), "image %d: the partials differ from the patches form's" % b
        assert same(ob[:n], one["out"][:n])
        assert same(ob[:n], hf.hardnet_finish(part[:, b, :n], bias))
        rows = [r for r in hf.edge_rows(n) if r < 70 or r >= n - 2]
        assert same(part[:, b, rows], mirror_rows(one["trunk"][rows], W))


def test_row_limit(hard):
    """65535 rows, the most cnn_check lets through: the buffer descriptor of the trunk tensor covers 65535 * 8192 * 4 = 2^31 - 32768 bytes and the last tile's
    lane offsets end at 2^31 - 512.  Rows 0, 65471, 65472 (the last 64-row tile's edge) and 65534 against the mirror; every row against the row 80 places in
    front of it (the tiled patch set), on the device.  65536 rows: AFFNET_ERR_INVALID with the head's message, nothing launched."""
    from affnet_amd import _lib, engine
    from affnet_amd._lib import lib, ptr
    _, W, bias = hard
    n_max = 65535
    assert hf.head_mp(n_max, 1) == 64 and "AFFNET_HEAD_MP" not in os.environ
    t0 = time.time()
    r = run_hardnet(hard, device_patches(n_max), n_max, read_trunk=False)
    wall = time.time() - t0
    assert r["rc"] == 0
    check_untouched(r, n_max, n_max)
    rows = [0, 65471, 65472, 65534]
    scratch = r["scratch"]
    trunk = scratch[:n_max * hf.HARDNET_K].view(n_max, hf.HARDNET_K)[rows].cpu().numpy().view(F32)
    assert same(r["part"][:, rows], mirror_rows(trunk, W))
    assert same(r["out"][:n_max], hf.hardnet_finish(r["part"], bias))
    assert same(r["part"][:, 80:], r["part"][:, :n_max - 80]), "a row's partials depend on its position"
    tr = scratch[:n_max * hf.HARDNET_K].view(n_max, hf.HARDNET_K)
    assert torch.equal(tr[80:], tr[:n_max - 80]) and not bool((tr[-1] == SENTINEL).any())
    print("HardNet forward of 65535 rows incl. the read-back: %.2f s" % wall)
    record_parity("HardNet head at the 65535-row limit", wall_seconds_with_readback=wall, rows_mirrored=rows)
    del r, scratch, tr
    _PATCHES.pop(n_max, None)
    torch.cuda.empty_cache()
    # one row more: refused before anything is launched (small buffers: nothing may touch them)
    ctx = engine.utility_ctx(torch.device(DEV))
    small, out, p = sentinel_buffer(1 << 16), sentinel_buffer(1 << 12), device_patches(16)
    rc = lib.affnet_cnn32_forward(ctx, _lib.NET_HARDNET, ptr(hard[0]), ptr(p), None, 65536, ptr(out.view(torch.float32)), ptr(small.view(torch.float32)),
                                  engine.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID
    msg = lib.affnet_last_error(ctx).decode()
    assert "n_max=65536" in msg and "HardNet head: max 65535 rows per image" in msg, msg
    assert bool((small == SENTINEL).all()) and bool((out == SENTINEL).all())


@pytest.mark.parametrize("n", [1, 3, 65, 76])
def test_tfeat_head_partials_on_the_bytes(golden_dir, n):
    """tfeat_head_kernel (64-patch tiles, K = 4 x 1024): the partials behind the device's own conv2 tensor against head_partials on the bytes; rows past n of the
    scratch untouched.  The tanhf finish stays under the referee test of tests/test_gpu_tfeat.py."""
    import affnet_amd
    from affnet_amd import engine
    from affnet_amd._lib import lib, check, ptr
    dev = torch.device(DEV)
    net = affnet_amd.HardTFeatNet(sm=None)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in load_golden_weights(golden_dir).items()})
    packed = net.to(DEV).packed_weights(dev)
    W, _ = hf.unpack_head(packed.cpu().numpy(), "tfeat")
    x = torch.from_numpy(hf.patch_set()[:n].copy()).to(DEV)
    floats = lib.affnet_tfeat_scratch_floats(n)
    assert floats == n * (hf.TFEAT_K + 512)
    scratch, out = sentinel_buffer(floats + 1024), sentinel_buffer((n + GUARD) * 128)
    ctx = engine.utility_ctx(dev)
    check(lib.affnet_tfeat_forward(ctx, ptr(packed), ptr(x), None, n, ptr(out.view(torch.float32)), ptr(scratch.view(torch.float32)), engine.stream_of(dev)), ctx,
          "affnet_tfeat_forward")
    torch.cuda.synchronize()
    s = scratch.cpu().numpy()
    trunk = s[:n * hf.TFEAT_K].view(F32).reshape(n, hf.TFEAT_K)
    part = s[n * hf.TFEAT_K: floats].view(F32).reshape(4, n, 128)
    assert np.all(s[floats:] == SENTINEL) and not np.any(s[:floats] == SENTINEL)
    assert np.all(out.cpu().numpy()[n * 128:] == SENTINEL)
    want = mirror_rows(trunk, W, "tfeat")
    assert want.shape == part.shape and same(hf.head_partials(trunk[:1], W, hf.KSPLIT, 1024), want[:, :1])
    assert same(part, want), "%d partials differ from the fmaf chains" % int((bits(part) != bits(want)).sum())
