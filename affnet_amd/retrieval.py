"""Descriptor index over many images (csrc/knn.hip): k nearest neighbours of a query image's descriptors among the concatenated descriptors of
a database, one vote per image from them, and the vote shortlist handed to the batched matching + spatial verification of ReprojectionStuff
(enqueue_match_and_verify_many) - the loop extract -> index -> shortlist -> verify.  The same index on int8 descriptors (csrc/knn_q8.hip)
and behind an inverted file over k-means cells (csrc/ivf.hip) further down, and last the two combined: int8 rows in the cells."""
import numpy as np
import torch

from . import engine, _lib
from ._lib import lib, check, ptr
from . import ReprojectionStuff as RS

DIM = 128


def _device_tensor(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise ValueError("affnet_amd.retrieval: %s must be a device tensor (tensor.cuda()); this implementation has no CPU path" % what)


def _check_k(k, what):
    if not (isinstance(k, (int, np.integer)) and 1 <= int(k) <= _lib.KNN_MAX_K):
        raise ValueError("%s: k must be an integer in 1..%d" % (what, _lib.KNN_MAX_K))
    return int(k)


def _check_shape(t, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.size(1) != DIM:
        raise ValueError("affnet_amd.retrieval: %s must be an (n,%d) tensor" % (what, DIM))


def _check_desc(t, what):
    _check_shape(t, what)
    _device_tensor(t, what)
    return t.contiguous().float()


def index_offsets(counts):
    """Rows per image -> (counts, offsets) as int lists, offsets[i] = first row of image i in the concatenated buffers, offsets[-1] = all rows."""
    c = [int(x) for x in counts]
    if any(x < 0 for x in c):
        raise ValueError("index_offsets: negative row count")
    off = np.concatenate([[0], np.cumsum(c, dtype=np.int64)])
    if off[-1] > 0x7fffffff:
        raise ValueError("index_offsets: more than 2^31 - 1 rows")
    return c, [int(o) for o in off]


def skip_range(counts, exclude):
    """The rows (first, n) of image `exclude` in the concatenated buffers - the skip range of a leave-one-image-out query; None -> (0, 0)."""
    c, off = index_offsets(counts)
    if exclude is None:
        return 0, 0
    if not (isinstance(exclude, (int, np.integer)) and 0 <= int(exclude) < len(c)):
        raise ValueError("exclude = %r with %d images in the index" % (exclude, len(c)))
    return off[int(exclude)], c[int(exclude)]


def knn(desc_q, desc_db, k=2, skip=None, n_chunks=0):
    """For every row of desc_q (n1,128) the k rows of desc_db (n2,128) at the smallest distance (Losses.distance_matrix_vector's, bit for bit),
    ascending by (distance, row): (dist (n1,k) float32, idx (n1,k) int32), slots without a candidate hold (+inf, -1).  skip = (row, n): database
    rows [row, row + n) are no candidates.  n_chunks: column chunks of the search grid, 0 = the library's choice; the result does not depend on it.
    Enqueued on the current stream, no synchronisation."""
    k = _check_k(k, "knn")
    a, b = _check_desc(desc_q, "desc_q"), _check_desc(desc_db, "desc_db")
    if a.device != b.device:
        raise ValueError("knn: desc_q and desc_db live on different devices")
    row, n = (0, 0) if skip is None else (int(skip[0]), int(skip[1]))
    if n < 0 or int(n_chunks) < 0:
        raise ValueError("knn: negative skip length or n_chunks")
    n1, n2, dev = a.size(0), b.size(0), a.device
    dist = torch.empty(n1, k, dtype=torch.float32, device=dev)
    idx = torch.empty(n1, k, dtype=torch.int32, device=dev)
    if n1 == 0:
        return dist, idx
    ctx = engine.utility_ctx(dev)
    nc = int(n_chunks) or lib.affnet_knn_chunks(ctx, n1, n2)
    scratch = torch.empty(lib.affnet_knn_scratch_bytes(n1, n2, k, nc), dtype=torch.uint8, device=dev)
    one = torch.zeros(8, dtype=torch.float32, device=dev)           # stands in for an empty database: never read, but the boundary refuses NULL
    rc = lib.affnet_knn(ctx, ptr(a), n1, ptr(b if n2 else one), n2, DIM, k, row, n, nc, ptr(dist), ptr(idx), ptr(scratch), engine.stream_of(dev))
    check(rc, ctx, "affnet_knn")
    return dist, idx


class DescriptorIndex(object):
    """The descriptors (and, for retrieve, the frames) of M images, concatenated once.  descs: list of (n_i,128) device tensors, LAFs: list of
    (n_i,2,3) device tensors or None; empty images are allowed.  D (N,128), n_rows = N, L (N,2,3) or None, counts, offsets (M + 1) and the device table
    row_image (N,) int32 = the image of every row."""

    def __init__(self, descs, LAFs=None):
        descs = list(descs)
        if not descs:
            raise ValueError("DescriptorIndex: no image")
        for i, d in enumerate(descs):
            _check_shape(d, "descs[%d]" % i)
        self.counts, self.offsets = index_offsets([d.size(0) for d in descs])
        if LAFs is not None:
            LAFs = list(LAFs)
            if len(LAFs) != len(descs):
                raise ValueError("DescriptorIndex: one LAF tensor per descriptor tensor (%d for %d)" % (len(LAFs), len(descs)))
            for i, l in enumerate(LAFs):
                if not isinstance(l, torch.Tensor) or l.numel() != 6 * self.counts[i]:
                    raise ValueError("DescriptorIndex: one LAF per descriptor row (image %d: %d descriptors)" % (i, self.counts[i]))
        ds = [_check_desc(d, "descs[%d]" % i) for i, d in enumerate(descs)]
        dev = ds[0].device
        if any(d.device != dev for d in ds):
            raise ValueError("DescriptorIndex: the images live on different devices")
        self.L = None
        if LAFs is not None:
            for i, l in enumerate(LAFs):
                _device_tensor(l, "LAFs[%d]" % i)
            self.L = torch.cat([l.contiguous().float().reshape(-1, 2, 3) for l in LAFs], 0)
        self.D = torch.cat(ds, 0)
        self.n_rows = self.D.size(0)          # kept beside D: a subclass may drop D
        self.device = dev
        self.row_image = torch.repeat_interleave(torch.arange(len(ds), dtype=torch.int32, device=dev),
                                                 torch.tensor(self.counts, dtype=torch.int64, device=dev)).contiguous()

    def __len__(self):
        return len(self.counts)

    def skip_range(self, exclude):
        return skip_range(self.counts, exclude)

    def _search(self, q, k, skip):
        """(dist (n1,k), idx (n1,k)) of the checked query rows q against the index's rows: here knn against the whole of D.  What a subclass
        replaces; everything else of enqueue_votes is shared."""
        return knn(q, self.D, k, skip)

    def enqueue_votes(self, desc_q, k=4, ratio=0.8, exclude=None):
        """The index's search (_search: knn of desc_q against the whole index), then affnet_knn_vote: row r's neighbour j < k-1 votes for its
        image iff !(dist[r][j] > ratio * dist[r][k-1]) and no earlier neighbour of the row voted for that image (so k - 1 is the largest number
        of images that can show the same feature and all receive its vote).  exclude: an image whose rows are no candidates.
        Returns device tensors (votes (M,) int32, dist (n1,k), idx (n1,k)); no synchronisation."""
        k = _check_k(k, "enqueue_votes")
        skip = self.skip_range(exclude)
        q = _check_desc(desc_q, "desc_q")
        if q.device != self.device:
            raise ValueError("enqueue_votes: desc_q and the index live on different devices")
        dist, idx = self._search(q, k, skip)
        votes = torch.empty(len(self.counts), dtype=torch.int32, device=self.device)
        ctx = engine.utility_ctx(self.device)
        one = torch.zeros(8, dtype=torch.int32, device=self.device)     # stands in for empty inputs: never read, but the boundary refuses NULL
        n1, n2 = q.size(0), self.n_rows
        rc = lib.affnet_knn_vote(ctx, ptr(dist if n1 else one), ptr(idx if n1 else one), n1, k, float(ratio), ptr(self.row_image if n2 else one), n2,
                                 len(self.counts), ptr(votes), engine.stream_of(self.device))
        check(rc, ctx, "affnet_knn_vote")
        return votes, dist, idx

    def shortlist(self, desc_q, top=10, k=4, ratio=0.8, exclude=None):
        """(images, votes): the images with at least one vote by descending votes, ties by ascending image index, at most `top`.  One read-back."""
        votes = self.enqueue_votes(desc_q, k, ratio, exclude)[0].cpu().tolist()          # the one read-back
        order = sorted((i for i, v in enumerate(votes) if v > 0), key=lambda i: (-votes[i], i))[:max(int(top), 0)]
        return order, [votes[i] for i in order]

    def retrieve(self, desc_q, LAFs_q, top=10, k=4, ratio=0.8, exclude=None, SNN_threshold=0.8, inl_th=3.0, model="homography", lo_iters=3, rounds=8, seed=0,
                 guided=False, guided_threshold=0.9, radius=None, matcher="reference", fginn_radius=10.0, mutual=False):
        """shortlist, then every shortlisted image matched against the query and verified in one device call chain
        (enqueue_match_and_verify_many: the query is side 1, the index side 2).  model: 'homography', 'affine' or 'fundamental' (a scene with
        depth; it alone reads `rounds` and `seed`).  Returns a list of dicts {image, votes, num_inliers, H, tent_in_1, tent_in_2, inliers}, by
        descending num_inliers, ties in shortlist order; each entry's matching and verification outputs are what
        match_and_verify(desc_q, descs[image], LAFs_q, LAFs[image]) returns.
        guided=True: the chain is enqueue_match_verify_guided_many (guided_threshold, radius as in match_verify_guided), each entry's outputs are
        what match_verify_guided returns for the image, and the entry also has seed_stage = {tentatives, num_inliers, flags} of the first stage.
        matcher, fginn_radius, mutual: the first stage of the unguided chain, as in match_and_verify ('reference', 'snn' or 'fginn')."""
        RS._matcher_radius("retrieve", matcher, fginn_radius, mutual, guided)
        if self.L is None:
            raise ValueError("retrieve: the index was built without LAFs")
        _check_k(k, "retrieve")
        self.skip_range(exclude)
        q = _check_desc(desc_q, "desc_q")
        _device_tensor(LAFs_q, "LAFs_q")
        if LAFs_q.numel() != 6 * q.size(0):
            raise ValueError("retrieve: one LAF per descriptor row (%d frames for %d descriptors)" % (LAFs_q.numel() // 6, q.size(0)))
        lq = LAFs_q.contiguous().float().reshape(-1, 2, 3)
        images, votes = self.shortlist(q, top, k, ratio, exclude)
        if not images:
            return []
        pairs = [(0, s) for s in images]
        if guided:
            tent, cnt, H, inl, _, summary, cnt0, summary0 = RS.enqueue_match_verify_guided_many(q, lq, [q.size(0)], self.D, self.L, self.counts, pairs, SNN_threshold,
                                                                                                inl_th, model, guided_threshold, radius, True, lo_iters, rounds,
                                                                                                seed)
            first = torch.cat([cnt0.view(-1, 1), summary0], 1)
        else:
            tent, cnt, H, inl, _, summary = RS.enqueue_match_and_verify_many(q, lq, [q.size(0)], self.D, self.L, self.counts, pairs, SNN_threshold, inl_th, model,
                                                                             lo_iters, rounds, seed, matcher, fginn_radius, mutual)
            first = summary[:, :0]
        host = torch.cat([cnt.view(-1, 1), summary, first], 1).cpu().tolist()
        out = []
        for p, row in enumerate(host):
            t = row[0]
            out.append({"image": images[p], "votes": votes[p], "num_inliers": row[3], "H": H[p], "tent_in_1": tent[p, :t, 0].long(),
                        "tent_in_2": tent[p, :t, 1].long(), "inliers": inl[p, :t].bool()})
            if guided:
                out[-1]["seed_stage"] = {"tentatives": row[5], "num_inliers": row[8], "flags": row[9]}
        return sorted(out, key=lambda e: -e["num_inliers"])          # sorted() is stable: ties keep the shortlist's order


# ---- int8 descriptors: exact integer k-NN on the i8 matrix instruction (csrc/knn_q8.hip) ----

def _check_scale(scale, what):
    try:
        s = float(scale)
    except (TypeError, ValueError):
        s = float("nan")
    with np.errstate(over="ignore"):
        f = float(np.float32(s))          # what the library receives
    if not (np.isfinite(f) and f > 0):
        raise ValueError("%s: scale must be a finite number > 0 (got %r)" % (what, scale))
    return f


def _check_q8(q, sq, what):
    if not (isinstance(q, torch.Tensor) and q.dim() == 2 and q.size(1) == DIM and q.dtype == torch.int8):
        raise ValueError("affnet_amd.retrieval: %s must be an (n,%d) int8 tensor" % (what, DIM))
    if not (isinstance(sq, torch.Tensor) and sq.dtype == torch.int32 and sq.numel() == q.size(0)):
        raise ValueError("affnet_amd.retrieval: %s needs one int32 sum of squares per row" % what)


def quantization_scale(descs):
    """127 / max|x| over the given tensor or list of tensors: the largest scale at which the quantiser clips no entry.  One read-back; an
    index-build-time call."""
    ds = [descs] if isinstance(descs, torch.Tensor) else list(descs)
    m = max([float(d.abs().max()) for d in ds if d.numel()] or [0.0])
    if not (np.isfinite(m) and m > 0):
        raise ValueError("quantization_scale: the descriptors have no finite non-zero entry")
    return _check_scale(127.0 / m, "quantization_scale")


def quantize(desc, scale):
    """desc (n,128) -> (q (n,128) int8, sq (n,) int32): q = clamp(rint(x * scale), -127, 127) in fp32 (round half to even, NaN -> 0, +-inf ->
    +-127), sq = the rows' sums of q^2 (affnet_quantize_desc).  Enqueued on the current stream, no synchronisation."""
    scale = _check_scale(scale, "quantize")
    d = _check_desc(desc, "desc")
    n, dev = d.size(0), d.device
    q = torch.empty(n, DIM, dtype=torch.int8, device=dev)
    sq = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        ctx = engine.utility_ctx(dev)
        check(lib.affnet_quantize_desc(ctx, ptr(d), n, DIM, scale, ptr(q), ptr(sq), engine.stream_of(dev)), ctx, "affnet_quantize_desc")
    return q, sq


def knn_q8(q, qsq, db, dbsq, k=2, scale=None, skip=None, n_chunks=0):
    """For every row of q (n1,128) int8 the k rows of db (n2,128) int8 at the smallest d2 = (qsq + dbsq) - 2 q.db (exact, int32), ascending by
    (d2, row): (dist2 (n1,k) int32, dist (n1,k) float32 = sqrt(float32(d2)) / scale, idx (n1,k) int32); slots without a candidate hold
    (2^31 - 1, +inf, -1).  qsq / dbsq: the rows' sums of squares as quantize returns them; scale: the scale both sides were quantised with.
    skip, n_chunks as in knn; the result does not depend on n_chunks.  Enqueued on the current stream, no synchronisation."""
    k = _check_k(k, "knn_q8")
    if scale is None:
        raise ValueError("knn_q8: scale must be given (the scale the descriptors were quantised with)")
    scale = _check_scale(scale, "knn_q8")
    _check_q8(q, qsq, "q")
    _check_q8(db, dbsq, "db")
    for t, what in ((q, "q"), (qsq, "qsq"), (db, "db"), (dbsq, "dbsq")):
        _device_tensor(t, what)
    a, asq, b, bsq = q.contiguous(), qsq.contiguous(), db.contiguous(), dbsq.contiguous()
    if len({a.device, asq.device, b.device, bsq.device}) != 1:
        raise ValueError("knn_q8: the tensors live on different devices")
    row, n = (0, 0) if skip is None else (int(skip[0]), int(skip[1]))
    if n < 0 or int(n_chunks) < 0:
        raise ValueError("knn_q8: negative skip length or n_chunks")
    n1, n2, dev = a.size(0), b.size(0), a.device
    dist2 = torch.empty(n1, k, dtype=torch.int32, device=dev)
    dist = torch.empty(n1, k, dtype=torch.float32, device=dev)
    idx = torch.empty(n1, k, dtype=torch.int32, device=dev)
    if n1 == 0:
        return dist2, dist, idx
    ctx = engine.utility_ctx(dev)
    nc = int(n_chunks)          # 0: the library's choice for this k, at most affnet_knn_q8_chunks
    scratch = torch.empty(lib.affnet_knn_q8_scratch_bytes(n1, n2, k, nc or lib.affnet_knn_q8_chunks(ctx, n1, n2)), dtype=torch.uint8, device=dev)
    one = torch.zeros(16, dtype=torch.int32, device=dev)          # stands in for an empty database: never read, but the boundary refuses NULL
    rc = lib.affnet_knn_q8(ctx, ptr(a), ptr(asq), n1, ptr(b if n2 else one), ptr(bsq if n2 else one), n2, DIM, k, row, n, nc, scale, ptr(dist2), ptr(dist),
                           ptr(idx), ptr(scratch), engine.stream_of(dev))
    check(rc, ctx, "affnet_knn_q8")
    return dist2, dist, idx


class QuantizedDescriptorIndex(DescriptorIndex):
    """DescriptorIndex whose search runs on int8 descriptors: Dq (N,128) int8, sq (N,) int32 and scale (None: quantization_scale(descs)) beside
    the tables of the base class.  enqueue_votes quantises the query with the index's scale, searches with affnet_knn_q8 and votes with
    affnet_knn_vote; shortlist and retrieve are inherited, so retrieve re-ranks with the exact fp32 matcher on D.  keep_float=False drops D after
    quantising (132 bytes per row instead of 512); such an index searches identically and cannot retrieve."""

    def __init__(self, descs, LAFs=None, scale=None, keep_float=True):
        DescriptorIndex.__init__(self, descs, LAFs)
        if scale is None:
            if self.D.size(0) == 0:
                raise ValueError("QuantizedDescriptorIndex: scale must be given for an index without rows")
            scale = quantization_scale(self.D)
        self.scale = _check_scale(scale, "QuantizedDescriptorIndex")
        self.Dq, self.sq = quantize(self.D, self.scale)
        if not keep_float:
            self.D = None

    def _search(self, q, k, skip):
        """On the quantised rows: q quantised with the index's scale, then knn_q8; dist (n1,k) = sqrt(d2) / scale."""
        qq, qsq = quantize(q, self.scale)
        _, dist, idx = knn_q8(qq, qsq, self.Dq, self.sq, k, self.scale, skip)
        return dist, idx

    def retrieve(self, desc_q, LAFs_q, *args, **kwargs):
        if self.D is None:
            raise ValueError("retrieve: the index was built with keep_float=False - the exact re-ranking needs the float descriptors")
        return DescriptorIndex.retrieve(self, desc_q, LAFs_q, *args, **kwargs)


# ---- inverted file: the search over the rows of a few k-means cells (csrc/ivf.hip) ----

def _check_nprobe(nprobe, what):
    if not (isinstance(nprobe, (int, np.integer)) and 1 <= int(nprobe) <= _lib.IVF_MAX_PROBE):
        raise ValueError("%s: nprobe must be an integer in 1..%d" % (what, _lib.IVF_MAX_PROBE))
    return int(nprobe)


def _check_cells(n_cells, what):
    if not (isinstance(n_cells, (int, np.integer)) and int(n_cells) >= 1):
        raise ValueError("%s: n_cells must be an integer >= 1" % what)
    return int(n_cells)


def default_cells(n):
    """The codebook size of an index over n rows: the power of two nearest sqrt(n), at least 1."""
    s = float(np.sqrt(max(int(n), 1)))
    lo = 1 << int(np.floor(np.log2(s)))
    return lo if s - lo <= 2 * lo - s else 2 * lo


def ivf_layout(assign, n_cells):
    """assign (n,) = the cell of every row -> (perm (n,) int32, cell_start (n_cells + 1,) int32): perm lists the rows cell by cell and ascends
    inside every cell (a stable sort), cell c owns the positions [cell_start[c], cell_start[c + 1]).  Works on CPU tensors too; one read-back
    on the device (the range check), a build-time call."""
    n_cells = _check_cells(n_cells, "ivf_layout")
    if not isinstance(assign, torch.Tensor) or assign.dim() != 1 or assign.is_floating_point():
        raise ValueError("ivf_layout: assign must be a 1-D integer tensor")
    a = assign.long()
    if a.numel() and not (0 <= int(a.min()) and int(a.max()) < n_cells):
        raise ValueError("ivf_layout: a cell outside 0..%d" % (n_cells - 1))
    return _ivf_layout(a, n_cells)


def _ivf_layout(a, n_cells):
    perm = torch.sort(a, stable=True)[1].to(torch.int32)
    start = torch.zeros(n_cells + 1, dtype=torch.int64, device=a.device)
    start[1:] = torch.cumsum(torch.bincount(a, minlength=n_cells), 0)
    return perm.contiguous(), start.to(torch.int32).contiguous()


def _cell_means(rows, perm, cell_start, centroids):
    ctx = engine.utility_ctx(rows.device)
    rc = lib.affnet_ivf_cell_means(ctx, ptr(rows), rows.size(0), DIM, ptr(perm), ptr(cell_start), centroids.size(0), ptr(centroids),
                                   engine.stream_of(rows.device))
    check(rc, ctx, "affnet_ivf_cell_means")


def initial_cells(n, n_cells):
    """The rows the centroids start as: centroid i = row floor(i * n / n_cells).  No random numbers."""
    return [(i * int(n)) // int(n_cells) for i in range(int(n_cells))]


def train_cells(rows, n_cells, iters=10, train_rows=None):
    """k-means codebook of rows (n,128): centroids (n_cells,128).  Deterministic: centroid i starts as training row floor(i * n / n_cells); every
    Lloyd iteration assigns with knn(rows, centroids, k=1) (ties go to the smaller cell) and updates with affnet_ivf_cell_means (double sums in
    row order, an empty cell keeps its centroid).  train_rows: None = all rows, an integer = about that many rows at a fixed stride."""
    n_cells = _check_cells(n_cells, "train_cells")
    if not (isinstance(iters, (int, np.integer)) and int(iters) >= 0):
        raise ValueError("train_cells: iters must be an integer >= 0")
    x = _check_desc(rows, "rows")
    if x.size(0) == 0:
        raise ValueError("train_cells: no rows")
    if train_rows is not None:
        if not (isinstance(train_rows, (int, np.integer)) and int(train_rows) >= 1):
            raise ValueError("train_cells: train_rows must be None or an integer >= 1")
        x = x[::max(-(-x.size(0) // int(train_rows)), 1)].contiguous()
    cent = x[torch.tensor(initial_cells(x.size(0), n_cells), dtype=torch.int64, device=x.device)].contiguous()
    for _ in range(int(iters)):
        assign = knn(x, cent, 1)[1][:, 0]
        perm, start = _ivf_layout(assign.long(), n_cells)
        _cell_means(x, perm, start, cent)
    return cent


class IVFParts(object):
    """The tables of an inverted file over D (n2,128) (include/affnet_hip.h, affnet_ivf_search): centroids (n_cells,128), sorted (n2,128),
    sorted_sq (n2,), perm (n2,) int32, cell_start (n_cells + 1,) int32."""

    def __init__(self, D, centroids):
        D, c = _check_desc(D, "D"), _check_desc(centroids, "centroids")
        if c.size(0) < 1 or c.device != D.device:
            raise ValueError("IVFParts: the centroids must be at least one row on the device of D")
        self.centroids, self.n_cells = c, c.size(0)
        assign = knn(D, c, 1)[1][:, 0] if D.size(0) else torch.zeros(0, dtype=torch.int32, device=D.device)
        self.perm, self.cell_start = _ivf_layout(assign.long(), self.n_cells)
        self.sorted = D[self.perm.long()].contiguous()
        self.sorted_sq = torch.empty(D.size(0), dtype=torch.float32, device=D.device)
        if D.size(0):
            ctx = engine.utility_ctx(D.device)
            check(lib.affnet_ivf_sqnorm(ctx, ptr(self.sorted), D.size(0), DIM, ptr(self.sorted_sq), engine.stream_of(D.device)), ctx, "affnet_ivf_sqnorm")


def ivf_knn(desc_q, index_or_parts, k=2, nprobe=8, skip=None, return_probes=False):
    """knn restricted to the database rows in the nprobe cells nearest to each query row: (dist (n1,k) float32, idx (n1,k) int32 = ORIGINAL
    database rows), distances, order and unfilled slots as knn's.  index_or_parts: an IVFDescriptorIndex or IVFParts.  return_probes: also the
    cells (n1,nprobe) int32 that were looked at, -1 where the codebook has fewer than nprobe cells.  Enqueued on the current stream, no
    synchronisation."""
    k, nprobe = _check_k(k, "ivf_knn"), _check_nprobe(nprobe, "ivf_knn")
    p = getattr(index_or_parts, "ivf", index_or_parts)
    if not isinstance(p, IVFParts):
        raise ValueError("ivf_knn: index_or_parts must be an IVFDescriptorIndex or IVFParts")
    a = _check_desc(desc_q, "desc_q")
    if a.device != p.sorted.device:
        raise ValueError("ivf_knn: desc_q and the index live on different devices")
    row, n = (0, 0) if skip is None else (int(skip[0]), int(skip[1]))
    if n < 0:
        raise ValueError("ivf_knn: negative skip length")
    n1, n2, dev = a.size(0), p.sorted.size(0), a.device
    dist = torch.empty(n1, k, dtype=torch.float32, device=dev)
    idx = torch.empty(n1, k, dtype=torch.int32, device=dev)
    probes = torch.empty(n1, nprobe, dtype=torch.int32, device=dev)
    if n1:
        ctx = engine.utility_ctx(dev)
        scratch = torch.empty(lib.affnet_ivf_scratch_bytes(n1, p.n_cells, nprobe, k), dtype=torch.uint8, device=dev)
        one = torch.zeros(8, dtype=torch.int32, device=dev)          # stands in for an empty database: never read, but the boundary refuses NULL
        rc = lib.affnet_ivf_search(ctx, ptr(a), n1, ptr(p.sorted if n2 else one), ptr(p.sorted_sq if n2 else one), ptr(p.perm if n2 else one), n2,
                                   ptr(p.cell_start), ptr(p.centroids), p.n_cells, DIM, k, nprobe, row, n, ptr(dist), ptr(idx), ptr(probes),
                                   ptr(scratch), engine.stream_of(dev))
        check(rc, ctx, "affnet_ivf_search")
    return (dist, idx, probes) if return_probes else (dist, idx)


class IVFDescriptorIndex(DescriptorIndex):
    """DescriptorIndex whose search looks at the rows of the nprobe nearest k-means cells of every query row (affnet_ivf_search): ivf (IVFParts:
    centroids, sorted, sorted_sq, perm, cell_start) beside the tables of the base class, D included - retrieve's matcher reads image segments.
    n_cells: None = default_cells(N); centroids: a trained codebook (n_cells,128), None = train_cells(D, n_cells, iters, train_rows).
    nprobe may be changed after the build.  enqueue_votes searches with ivf_knn and votes with affnet_knn_vote; shortlist and retrieve are
    inherited, so retrieve re-ranks with the exact fp32 matcher on D."""

    def __init__(self, descs, LAFs=None, n_cells=None, nprobe=8, iters=10, train_rows=None, centroids=None):
        self.nprobe = _check_nprobe(nprobe, "IVFDescriptorIndex")
        if n_cells is not None:
            n_cells = _check_cells(n_cells, "IVFDescriptorIndex")
        DescriptorIndex.__init__(self, descs, LAFs)
        if centroids is None:
            if self.D.size(0) == 0:
                raise ValueError("IVFDescriptorIndex: centroids must be given for an index without rows")
            centroids = train_cells(self.D, n_cells or default_cells(self.D.size(0)), iters, train_rows)
        elif n_cells is not None and (not isinstance(centroids, torch.Tensor) or centroids.dim() != 2 or centroids.size(0) != n_cells):
            raise ValueError("IVFDescriptorIndex: centroids must have n_cells = %d rows" % n_cells)
        self.ivf = IVFParts(self.D, centroids)
        self.n_cells = self.ivf.n_cells

    def _search(self, q, k, skip):
        """Restricted to self.nprobe (checked here: it may have been changed since the build) cells per query row: ivf_knn."""
        return ivf_knn(q, self.ivf, k, _check_nprobe(self.nprobe, "enqueue_votes"), skip)


# ---- inverted file over int8 rows: the cells of ivf.hip hold knn_q8.hip's rows (csrc/ivf.hip, affnet_ivf_search_q8) ----

class IVFQ8Parts(object):
    """The tables of an inverted file over the int8 rows of D (n2,128) (include/affnet_hip.h, affnet_ivf_search_q8): centroids (n_cells,128)
    float, sorted_q (n2,128) int8, sorted_sq (n2,) int32, perm (n2,) int32, cell_start (n_cells + 1,) int32 and scale.  The rows are assigned by
    knn(D, centroids, 1) on the float rows, exactly as in IVFParts, so perm and cell_start are IVFParts(D, centroids)'s; sorted_q / sorted_sq are
    the gather of quantize(D, scale) through perm (Dq, sq: that pair when the caller has it already).  136 bytes per row."""

    def __init__(self, D, centroids, scale, Dq=None, sq=None):
        self.scale = _check_scale(scale, "IVFQ8Parts")
        D, c = _check_desc(D, "D"), _check_desc(centroids, "centroids")
        if c.size(0) < 1 or c.device != D.device:
            raise ValueError("IVFQ8Parts: the centroids must be at least one row on the device of D")
        self.centroids, self.n_cells = c, c.size(0)
        assign = knn(D, c, 1)[1][:, 0] if D.size(0) else torch.zeros(0, dtype=torch.int32, device=D.device)
        self.perm, self.cell_start = _ivf_layout(assign.long(), self.n_cells)
        if Dq is None or sq is None:
            Dq, sq = quantize(D, self.scale)
        self.sorted_q = Dq[self.perm.long()].contiguous()
        self.sorted_sq = sq[self.perm.long()].contiguous()


def ivf_knn_q8(desc_q, index_or_parts, k=2, nprobe=8, skip=None, return_probes=False):
    """knn_q8 restricted to the database rows in the nprobe cells nearest to each query row: (dist2 (n1,k) int32, dist (n1,k) float32 =
    sqrt(float32(d2)) / scale, idx (n1,k) int32 = ORIGINAL database rows), order (d2, original row) and unfilled slots (2^31 - 1, +inf, -1) as
    knn_q8's.  desc_q: the float query rows; the coarse step reads them as they are (the cells are ivf_knn's), the search inside the cells their
    quantisation with the parts' scale.  index_or_parts: an IVFQuantizedDescriptorIndex or IVFQ8Parts.  return_probes: also the cells
    (n1,nprobe) int32 that were looked at, -1 where the codebook has fewer than nprobe cells.  Enqueued on the current stream, no
    synchronisation."""
    k, nprobe = _check_k(k, "ivf_knn_q8"), _check_nprobe(nprobe, "ivf_knn_q8")
    p = getattr(index_or_parts, "ivf", index_or_parts)
    if not isinstance(p, IVFQ8Parts):
        raise ValueError("ivf_knn_q8: index_or_parts must be an IVFQuantizedDescriptorIndex or IVFQ8Parts")
    a = _check_desc(desc_q, "desc_q")
    if a.device != p.sorted_q.device:
        raise ValueError("ivf_knn_q8: desc_q and the index live on different devices")
    row, n = (0, 0) if skip is None else (int(skip[0]), int(skip[1]))
    if n < 0:
        raise ValueError("ivf_knn_q8: negative skip length")
    n1, n2, dev = a.size(0), p.sorted_q.size(0), a.device
    dist2 = torch.empty(n1, k, dtype=torch.int32, device=dev)
    dist = torch.empty(n1, k, dtype=torch.float32, device=dev)
    idx = torch.empty(n1, k, dtype=torch.int32, device=dev)
    probes = torch.empty(n1, nprobe, dtype=torch.int32, device=dev)
    if n1:
        qq, qsq = quantize(a, p.scale)
        ctx = engine.utility_ctx(dev)
        scratch = torch.empty(lib.affnet_ivf_q8_scratch_bytes(n1, p.n_cells, nprobe, k), dtype=torch.uint8, device=dev)
        one = torch.zeros(16, dtype=torch.int32, device=dev)          # stands in for an empty database: never read, but the boundary refuses NULL
        rc = lib.affnet_ivf_search_q8(ctx, ptr(a), ptr(qq), ptr(qsq), n1, ptr(p.sorted_q if n2 else one), ptr(p.sorted_sq if n2 else one),
                                      ptr(p.perm if n2 else one), n2, ptr(p.cell_start), ptr(p.centroids), p.n_cells, DIM, k, nprobe, row, n, p.scale,
                                      ptr(dist2), ptr(dist), ptr(idx), ptr(probes), ptr(scratch), engine.stream_of(dev))
        check(rc, ctx, "affnet_ivf_search_q8")
    return (dist2, dist, idx, probes) if return_probes else (dist2, dist, idx)


class IVFQuantizedDescriptorIndex(QuantizedDescriptorIndex):
    """QuantizedDescriptorIndex whose search looks at the int8 rows of the nprobe nearest k-means cells of every query row
    (affnet_ivf_search_q8): ivf (IVFQ8Parts: centroids, sorted_q, sorted_sq, perm, cell_start, scale) beside the tables of the base classes.
    The codebook is trained on the float rows exactly as IVFDescriptorIndex trains it (n_cells, iters, train_rows, centroids as there); nprobe
    may be changed after the build.  enqueue_votes, shortlist and retrieve are inherited: retrieve re-ranks with the exact fp32 matcher on D.
    keep_float=False drops D and the unpermuted Dq / sq after the build: what remains is ivf and the image tables, 136 bytes per row; such an
    index searches identically and cannot retrieve."""

    def __init__(self, descs, LAFs=None, scale=None, keep_float=True, n_cells=None, nprobe=8, iters=10, train_rows=None, centroids=None):
        self.nprobe = _check_nprobe(nprobe, "IVFQuantizedDescriptorIndex")
        if n_cells is not None:
            n_cells = _check_cells(n_cells, "IVFQuantizedDescriptorIndex")
        QuantizedDescriptorIndex.__init__(self, descs, LAFs, scale, True)
        if centroids is None:
            if self.D.size(0) == 0:
                raise ValueError("IVFQuantizedDescriptorIndex: centroids must be given for an index without rows")
            centroids = train_cells(self.D, n_cells or default_cells(self.D.size(0)), iters, train_rows)
        elif n_cells is not None and (not isinstance(centroids, torch.Tensor) or centroids.dim() != 2 or centroids.size(0) != n_cells):
            raise ValueError("IVFQuantizedDescriptorIndex: centroids must have n_cells = %d rows" % n_cells)
        self.ivf = IVFQ8Parts(self.D, centroids, self.scale, self.Dq, self.sq)
        self.n_cells = self.ivf.n_cells
        if not keep_float:
            self.D = self.Dq = self.sq = None

    def _search(self, q, k, skip):
        """Restricted to self.nprobe (checked here: it may have been changed since the build) cells per query row: ivf_knn_q8."""
        return ivf_knn_q8(q, self.ivf, k, _check_nprobe(self.nprobe, "enqueue_votes"), skip)[1:]
