"""Descriptor index over many images (csrc/knn.hip): k nearest neighbours of a query image's descriptors among the concatenated descriptors of
a database, one vote per image from them, and the vote shortlist handed to the batched matching + spatial verification of ReprojectionStuff
(enqueue_match_and_verify_many) - the loop extract -> index -> shortlist -> verify."""
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
    (n_i,2,3) device tensors or None; empty images are allowed.  D (N,128), L (N,2,3) or None, counts, offsets (M + 1) and the device table
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
        self.device = dev
        self.row_image = torch.repeat_interleave(torch.arange(len(ds), dtype=torch.int32, device=dev),
                                                 torch.tensor(self.counts, dtype=torch.int64, device=dev)).contiguous()

    def __len__(self):
        return len(self.counts)

    def skip_range(self, exclude):
        return skip_range(self.counts, exclude)

    def enqueue_votes(self, desc_q, k=4, ratio=0.8, exclude=None):
        """knn of desc_q against the whole index, then affnet_knn_vote: row r's neighbour j < k-1 votes for its image iff
        !(dist[r][j] > ratio * dist[r][k-1]) and no earlier neighbour of the row voted for that image (so k - 1 is the largest number of
        images that can show the same feature and all receive its vote).  exclude: an image whose rows are no candidates.
        Returns device tensors (votes (M,) int32, dist (n1,k), idx (n1,k)); no synchronisation."""
        k = _check_k(k, "enqueue_votes")
        skip = self.skip_range(exclude)
        q = _check_desc(desc_q, "desc_q")
        if q.device != self.device:
            raise ValueError("enqueue_votes: desc_q and the index live on different devices")
        dist, idx = knn(q, self.D, k, skip)
        votes = torch.empty(len(self.counts), dtype=torch.int32, device=self.device)
        ctx = engine.utility_ctx(self.device)
        one = torch.zeros(8, dtype=torch.int32, device=self.device)     # stands in for empty inputs: never read, but the boundary refuses NULL
        n1, n2 = q.size(0), self.D.size(0)
        rc = lib.affnet_knn_vote(ctx, ptr(dist if n1 else one), ptr(idx if n1 else one), n1, k, float(ratio), ptr(self.row_image if n2 else one), n2,
                                 len(self.counts), ptr(votes), engine.stream_of(self.device))
        check(rc, ctx, "affnet_knn_vote")
        return votes, dist, idx

    def shortlist(self, desc_q, top=10, k=4, ratio=0.8, exclude=None):
        """(images, votes): the images with at least one vote by descending votes, ties by ascending image index, at most `top`.  One read-back."""
        votes = self.enqueue_votes(desc_q, k, ratio, exclude)[0].cpu().tolist()          # the one read-back
        order = sorted((i for i, v in enumerate(votes) if v > 0), key=lambda i: (-votes[i], i))[:max(int(top), 0)]
        return order, [votes[i] for i in order]

    def retrieve(self, desc_q, LAFs_q, top=10, k=4, ratio=0.8, exclude=None, SNN_threshold=0.8, inl_th=3.0, model="homography", lo_iters=3):
        """shortlist, then every shortlisted image matched against the query and spatially verified in one device call
        (enqueue_match_and_verify_many: the query is side 1, the index side 2).  Returns a list of dicts {image, votes, num_inliers, H, tent_in_1,
        tent_in_2, inliers}, by descending num_inliers, ties in shortlist order; each entry's matching and verification outputs are what
        match_and_verify(desc_q, descs[image], LAFs_q, LAFs[image]) returns."""
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
        tent, cnt, H, inl, _, summary = RS.enqueue_match_and_verify_many(q, lq, [q.size(0)], self.D, self.L, self.counts, [(0, s) for s in images],
                                                                         SNN_threshold, inl_th, model, lo_iters)
        host = torch.cat([cnt.view(-1, 1), summary], 1).cpu().tolist()
        out = []
        for p, row in enumerate(host):
            t = row[0]
            out.append({"image": images[p], "votes": votes[p], "num_inliers": row[3], "H": H[p], "tent_in_1": tent[p, :t, 0].long(),
                        "tent_in_2": tent[p, :t, 1].long(), "inliers": inl[p, :t].bool()})
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
        self.n_rows = self.D.size(0)
        if not keep_float:
            self.D = None

    def enqueue_votes(self, desc_q, k=4, ratio=0.8, exclude=None):
        """DescriptorIndex.enqueue_votes on the quantised rows: (votes (M,) int32, dist (n1,k) = sqrt(d2) / scale, idx (n1,k)); no synchronisation."""
        k = _check_k(k, "enqueue_votes")
        skip = self.skip_range(exclude)
        q = _check_desc(desc_q, "desc_q")
        if q.device != self.device:
            raise ValueError("enqueue_votes: desc_q and the index live on different devices")
        qq, qsq = quantize(q, self.scale)
        _, dist, idx = knn_q8(qq, qsq, self.Dq, self.sq, k, self.scale, skip)
        votes = torch.empty(len(self.counts), dtype=torch.int32, device=self.device)
        ctx = engine.utility_ctx(self.device)
        one = torch.zeros(8, dtype=torch.int32, device=self.device)     # stands in for empty inputs: never read, but the boundary refuses NULL
        n1, n2 = q.size(0), self.n_rows
        rc = lib.affnet_knn_vote(ctx, ptr(dist if n1 else one), ptr(idx if n1 else one), n1, k, float(ratio), ptr(self.row_image if n2 else one), n2,
                                 len(self.counts), ptr(votes), engine.stream_of(self.device))
        check(rc, ctx, "affnet_knn_vote")
        return votes, dist, idx

    def retrieve(self, desc_q, LAFs_q, *args, **kwargs):
        if self.D is None:
            raise ValueError("retrieve: the index was built with keep_float=False - the exact re-ranking needs the float descriptors")
        return DescriptorIndex.retrieve(self, desc_q, LAFs_q, *args, **kwargs)
