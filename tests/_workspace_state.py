"""Helpers of the workspace-state tests (tests/test_workspace_ledger_host.py on the CPU, tests/test_gpu_workspace_state.py on the GPU).

The fused calls work inside one caller-owned workspace whose areas are, with few exceptions, never cleared: every byte that a kernel reads must have been
written by a kernel of the same call.  These helpers make that checkable:

* ledger():       the areas of a context's workspace, from the table the library itself carves it from (affnet_probe_workspace_areas);
* the three images (rich / poor / flat) and the conditions they must meet under the oracle alone;
* Guarded:        a context re-bound to the middle of a larger buffer with guard bands, with the prior states of the tests (zeros, NaN floats; a stale
                  state is simply a complete call on the same context) - integer, byte and record areas only ever get zeros or the library's own bytes;
* Outputs / run:  the boundary driven through ctypes as SparseImgRepresenter.enqueue does it, into guard-banded output buffers filled with 0xFF bytes;
                  a "result" is every output array in full plus the counters, compared on bytes only.
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import affnet_oracle as orc  # noqa: E402

from _shape_margin import BORDER, H, MR_SIZE, N_FEATURES, W  # noqa: E402  (240 x 320, 300 features, the benchmark's extractor settings)

N_PREFILTER = int(1.5 * N_FEATURES)            # candidates the detector hands to the shape stage (SparseImgRepresenter.py: 1.5 N)
LAZY_ROWS = N_FEATURES + (N_FEATURES + 4) // 5  # first window of the lazy shape pass (pipeline.hip: N + ceil(N / 5))
ALIGN = 256                                    # the library's alignment (common.h: aff_align)
GUARD = 64 * 1024                              # bytes of each guard band, a multiple of ALIGN
BAND_BYTE = 0x5A
KIND_NAMES = {0: "f32", 1: "i32", 2: "u8", 3: "records", 4: "group"}
CNT_TOTAL = 16 + 24 + 6 * 16 + 8 * 16          # common.h: int32 counters per image
SEL_HIST_BINS = 2048
RAWMAX_BYTES = 32


# ---- the ledger ------------------------------------------------------------------------------------------------------------------------------------
def load_probes():
    from affnet_amd import _lib
    assert os.path.isfile(_lib.PROBES_LIB_PATH), "libaffnet_hip_probes.so is missing (AFFNET_PROBES=1 bash affnet_amd/csrc/build.sh)"
    pl = C.CDLL(_lib.PROBES_LIB_PATH)
    for name in ("affnet_probe_workspace_areas", "affnet_probe_shape_offsets"):
        fn = getattr(pl, name)
        fn.restype, fn.argtypes = _lib.PROBE_SYMBOLS[name]
    return pl


def ledger(probes, handle):
    """[{name, offset, bytes, kind ('f32' / 'i32' / 'u8' / 'records' / 'group'), cleared, parent (index or -1)}] in table order"""
    from affnet_amd import _lib
    n = probes.affnet_probe_workspace_areas(handle, 0, None)
    assert n > 0, "affnet_probe_workspace_areas: %d" % n
    buf = (_lib.WsArea * n)()
    assert probes.affnet_probe_workspace_areas(handle, n, C.cast(buf, C.c_void_p)) == n
    return [{"name": a.name.decode(), "offset": int(a.offset), "bytes": int(a.bytes), "kind": KIND_NAMES[a.kind], "cleared": int(a.cleared),
             "parent": int(a.parent)} for a in buf]


def leaves(areas):
    """The records that describe bytes of one kind: everything but the group units"""
    return [a for a in areas if a["kind"] != "group"]


# ---- the three images ------------------------------------------------------------------------------------------------------------------------------
def rich_image():
    """Fills every list: smooth noise (an 80 x 106 uniform field enlarged three times), far more maxima than candidates are kept and a shape filter
    that passes nine in ten of them, so that the first lazy window already holds its N survivors (the multi-octave noise of the other tests passes
    seven in ten and needs the second pass)"""
    g = torch.Generator().manual_seed(9)
    n = torch.rand(1, 1, H // 3, W // 3, generator=g)
    return (torch.nn.functional.interpolate(n, size=(H, W), mode="bicubic", align_corners=False).clamp(0.0, 1.0) * 255.0).contiguous()


def poor_image():
    """One raised-cosine bump of compact support on a constant background: the image is exactly constant away from it, so the few dozen maxima around
    the bump are all there is and every list ends far below its capacity (Gaussian blobs will not do: their tails ripple everywhere in fp32)"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    r = torch.sqrt(((yy - 120.0) / 12.0) ** 2 + ((xx - 160.0) / 12.0) ** 2)
    bump = torch.where(r < 1.0, torch.cos(0.5 * np.pi * r) ** 2, torch.zeros(()))
    return (96.0 + 90.0 * bump).view(1, 1, H, W).contiguous()


def flat_image():
    return torch.full((1, 1, H, W), 128.0)


def busy_image():
    """A prior state only, never a target: the multi-octave noise of the other suites fills every list too, but the shape filter passes only seven in
    ten of its candidates, so the second lazy pass runs and leaves verdicts in the rows that a call on rich skips"""
    return orc.synthetic_image(H, W, 1)


IMAGES = {"rich": rich_image, "poor": poor_image, "flat": flat_image}


def oracle_counts(img, affnet_sd, **kw):
    """What the reference restatement alone does with the image: (candidates the detector emits, survivors of the shape filter among the first LAZY_ROWS
    candidates, survivors among all, rows returned).  An image without a single detection makes the reference raise in torch.cat of an empty list
    (SparseImgRepresenter.py:100): that one error, and no other, is answered with zeros."""
    ex = orc.OracleExtractor(num_features=N_FEATURES, num_Baum_iters=1, affnet_sd=affnet_sd, mrSize=MR_SIZE, border=BORDER, **kw)
    try:
        _, resp = ex(img)
    except (RuntimeError, ValueError) as e:
        if "torch.cat" not in str(e) or "non-empty list" not in str(e):
            raise
        return 0, 0, 0, 0
    good = ex.shape_stage["good"]
    return int(good.numel()), int(good[:LAZY_ROWS].sum()), int(good.sum()), int(resp.numel())


# ---- guard-banded buffers --------------------------------------------------------------------------------------------------------------------------
class Banded(object):
    """`nbytes` payload bytes between two guard bands of GUARD bytes; the payload starts on an ALIGN boundary"""

    def __init__(self, nbytes, device):
        self.nbytes = int(nbytes)
        pad = (-self.nbytes) % ALIGN
        self.raw = torch.empty(GUARD + self.nbytes + pad + GUARD, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % ALIGN == 0
        self.raw[:GUARD] = BAND_BYTE
        self.raw[GUARD + self.nbytes:] = BAND_BYTE
        self.mid = self.raw[GUARD:GUARD + self.nbytes]

    def intact(self):
        return bool((self.raw[:GUARD] == BAND_BYTE).all()) and bool((self.raw[GUARD + self.nbytes:] == BAND_BYTE).all())


class Guarded(object):
    """An engine.Context re-bound to the middle of a guard-banded buffer, before its first call (and never after a graph capture)"""

    def __init__(self, probes, ctx):
        from affnet_amd._lib import lib, check, ptr
        self.ctx = ctx
        self.ws_bytes = int(lib.affnet_workspace_bytes(ctx.handle))
        self.buf = Banded(self.ws_bytes, ctx.device)
        check(lib.affnet_bind_workspace(ctx.handle, ptr(self.buf.mid), self.ws_bytes), ctx.handle, "affnet_bind_workspace")
        ctx.workspace = self.buf.mid
        ctx._ws_f32 = self.buf.mid.view(torch.float32)
        self.areas = ledger(probes, ctx.handle)
        self.zero()

    def zero(self):
        self.buf.mid.zero_()

    def nan_floats(self):
        """0xFF bytes (a NaN in every float) in the areas the ledger calls f32, zeros everywhere else - written last, so that an integer view that shares
        bytes with a float view of the CNN scratch stays zero"""
        self.buf.mid.zero_()
        for a in leaves(self.areas):
            if a["kind"] == "f32":
                self.buf.mid[a["offset"]:a["offset"] + a["bytes"]] = 0xFF
        for a in leaves(self.areas):
            if a["kind"] != "f32":
                self.buf.mid[a["offset"]:a["offset"] + a["bytes"]] = 0

    def intact(self):
        return self.buf.intact()

    def free(self):
        self.buf = None
        self.ctx.workspace = self.ctx._ws_f32 = None


class Outputs(object):
    """The caller's buffers of one fused call, each between guard bands, each filled with 0xFF bytes before every call"""
    SHAPES = {"LAFs": (6, torch.float32), "responses": (1, torch.float32), "ids": (3, torch.int32), "descriptors": (128, torch.float32)}

    def __init__(self, B, F, device):
        self.B, self.F = B, F
        self.buf = {k: Banded(B * F * n * 4, device) for k, (n, _) in self.SHAPES.items()}
        self.buf["count"] = Banded(B * 4, device)

    def poison(self):
        for b in self.buf.values():
            b.mid.fill_(0xFF)

    def ptr(self, k):
        return C.c_void_p(self.buf[k].mid.data_ptr())

    def intact(self):
        return all(b.intact() for b in self.buf.values())


def collect(ctx, outs, with_desc):
    """A result: count, the overflow flag and counters 1 .. 4 of every image, and every output array in full, as bytes"""
    torch.cuda.synchronize()
    r = {"count": outs.buf["count"].mid.cpu().numpy().view(np.int32).copy()}
    for which in range(5):
        r["counter%d" % which] = ctx.counter_view(which).cpu().numpy().copy()
    for k in ("LAFs", "responses", "ids") + (("descriptors",) if with_desc else ()):
        r[k] = outs.buf[k].mid.cpu().numpy().copy()
    return r


def same_result(a, b):
    """'' when the two results are equal bit for bit, else the names of the entries that differ"""
    bad = [k for k in a if k not in b or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    return ", ".join(sorted(bad + [k for k in b if k not in a]))


def rows_past_count_are_zero(r, B, F):
    """'' when rows >= count[b] of every output array are zero bytes"""
    bad = []
    for k, (n, _) in Outputs.SHAPES.items():
        if k not in r:
            continue
        rows = r[k].reshape(B, F, n * 4)
        for b in range(B):
            c = int(r["count"][b])
            if not (0 <= c <= F) or rows[b, c:].any():
                bad.append("%s[image %d, rows >= %d]" % (k, b, c))
    return ", ".join(bad)


def extract(ctx, nets, img, do_ori, outs, with_desc):
    """affnet_extract_features as SparseImgRepresenter.enqueue calls it, into `outs` (poisoned first)"""
    from affnet_amd import engine
    from affnet_amd._lib import lib, check
    outs.poison()
    rc = lib.affnet_extract_features(ctx.handle, C.byref(nets), C.c_void_p(img.data_ptr()), int(bool(do_ori)), outs.ptr("LAFs"), outs.ptr("responses"),
                                     outs.ptr("ids"), outs.ptr("descriptors") if with_desc else None, outs.ptr("count"), engine.stream_of(ctx.device))
    check(rc, ctx.handle, "affnet_extract_features")
    return collect(ctx, outs, with_desc)
