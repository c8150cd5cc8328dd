"""CPU: pins of tests/_match_fp32.py, the float32 restatement of the single-pair matcher (affnet_amd/csrc/match.hip).
tests/test_gpu_matcher.py compares affnet_distance_matrix and affnet_match_snn with that restatement on the bytes, and the descriptor index,
the inverted file and the batched matcher are all tested against those two calls - so a wrong mirror, or an input without the case it is
there for, would empty every one of those tests.  Here each function is tied to something the project already trusts:

  dots, sqnorm        libm fmaf (ctypes) called value by value in the stated order
  distance            oracle.distance_matrix_vector and the float64 restatement (tests/_knn_fp64.py), within the project's bar for this quantity
  match_from_matrix   oracle.match_snn on the oracle's own float32 matrix, and torch.min on the mirror's: the bytes
  match               the 63 tentatives of the unmodified reference on the golden graf pair

and the planted inputs are shown to contain ties (in one lane's columns, across lanes, with min2 == min1), rows with two NaN columns,
unused columns, selection rounds with kept and refused rows on both sides of row 1024, and bits that each wrong variant changes."""
import ctypes
import ctypes.util
import os

import numpy as np
import torch

import _knn_fp64 as kf
import _match_fp32 as mf
import affnet_oracle as orc
from _fp32_chain import F32

FP64_BAR = 2e-6 * 2 + 1e-5         # tests/test_gpu_parity.py: the distance matrix against the oracle
THR = 0.8


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == F32 else np.int32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_GOLD = {}


def golden():
    if not _GOLD:
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_graf16_n500.npz"))
        _GOLD.update(g=g, d1=np.ascontiguousarray(g["desc1"], F32), d2=np.ascontiguousarray(g["desc2"], F32))
        _GOLD["m"] = mf.match(_GOLD["d1"], _GOLD["d2"], THR)
        _GOLD["M"] = _GOLD["m"]["M"]
    return _GOLD


def test_dots_and_sqnorm_equal_the_scalar_fmaf_loops():
    path = ctypes.util.find_library("m")
    assert path, "libm not found"
    libm = ctypes.CDLL(path)
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    fmaf = lambda x, y, z: libm.fmaf(float(x), float(y), float(z))
    rng = np.random.default_rng(3)
    a = (rng.normal(size=(5, 128)) * np.exp2(rng.integers(-6, 7, (5, 128)))).astype(F32)
    b = (rng.normal(size=(7, 128)) * np.exp2(rng.integers(-6, 7, (7, 128)))).astype(F32)
    b[2] = a[1]                                            # a self-product: every term positive
    want = np.zeros((5, 7), F32)
    for r in range(5):
        for c in range(7):
            s = 0.0
            for t in range(8):
                for j in range(4):
                    for kq in range(4):
                        k = 16 * t + 4 * kq + j
                        s = fmaf(a[r, k], b[c, k], s)
            want[r, c] = s
    assert same(mf.dots(a, b), want)
    nat = np.array([[np.nan] * 7] * 5, F32)
    for r in range(5):
        for c in range(7):
            s = 0.0
            for k in range(128):
                s = fmaf(a[r, k], b[c, k], s)
            nat[r, c] = s
    assert same(mf.dots(a, b, natural=True), nat)
    assert not same(nat, want), "the two K orders give the same bits on this input: it cannot tell them apart"
    x = np.concatenate([a, b])
    sq, seq = np.zeros(12, F32), np.zeros(12, F32)
    for r in range(12):
        lane = [F32(fmaf(x[r, l + 64], x[r, l + 64], fmaf(x[r, l], x[r, l], 0.0))) for l in range(64)]
        for o in (32, 16, 8, 4, 2, 1):
            lane = [F32(lane[l] + lane[l ^ o]) for l in range(64)]
        sq[r] = lane[0]
        s = 0.0
        for k in range(128):
            s = fmaf(x[r, k], x[r, k], s)
        seq[r] = s
    assert same(mf.sqnorm(x), sq) and same(mf.sqnorm(x, sequential=True), seq)
    assert not same(sq, seq)


def test_distance_against_the_oracle_and_float64():
    g = golden()
    cases = [("golden graf 1-6, 500 x 500", g["d1"], g["d2"], g["M"])]
    q, db = mf.planted(200, 415, self_copies=False)
    cases.append(("planted 200 x 415 without self-copies", q, db, mf.distance(q, db)))
    for name, a, b, M in cases:
        assert M.dtype == F32 and not np.isnan(M).any(), name
        d_orc = np.abs(M.astype(np.float64) - orc.distance_matrix_vector(torch.tensor(a), torch.tensor(b)).numpy()).max()
        d_f64 = np.abs(M - kf.distance(a, b)).max()
        print("%s: mirror against the oracle worst |diff| %.3g, against float64 %.3g (bar %.3g)" % (name, d_orc, d_f64, FP64_BAR))
        assert d_orc < FP64_BAR and d_f64 < FP64_BAR, name
    assert mf.planted(200, 415, self_copies=False)[1][0] @ mf.planted(200, 415, self_copies=False)[1][0] > 250.0, "the long row is in the case"


def _against_oracle_selection(name, a, b):
    ta, tb = torch.tensor(a), torch.tensor(b)          # copies: the planted arrays are read-only
    M = orc.distance_matrix_vector(ta, tb).numpy()
    w_md, w_idx, w_md2, w_t1, w_t2 = orc.match_snn(ta, tb, THR)
    m = mf.match_from_matrix(M, THR)
    assert same(m["md"], w_md.numpy()) and same(m["md2"], w_md2.numpy()), name
    assert np.array_equal(m["idx"], w_idx.numpy()), name
    assert np.array_equal(m["tent"][:, 0], w_t1.numpy()) and np.array_equal(m["tent"][:, 1], w_t2.numpy()) and m["count"] == len(w_t1), name
    tie = int((((M == m["md"][:, None]).sum(1) >= 2) | (np.isnan(M).sum(1) >= 2)).sum())
    return tie, int(np.isnan(m["md"]).sum())


def test_selection_logic_against_the_oracle_on_the_oracles_matrix():
    g = golden()
    ties, nans = _against_oracle_selection("golden", g["d1"], g["d2"])
    for n1, n2 in mf.MATRIX_SHAPES:
        q, db = mf.planted(n1, n2)
        t, n = _against_oracle_selection((n1, n2), q, db)
        ties, nans = ties + t, nans + n
    print("rows of the oracle's own matrices with a tied or doubled-NaN minimum: %d, with a NaN minimum: %d" % (ties, nans))
    # and torch's row minimum on the MIRROR's matrices, whose ties and NaN rows test_input_conditions counts
    for n1, n2 in mf.MATRIX_SHAPES:
        m = mf.planted_mirror(n1, n2)
        v, c = torch.min(torch.tensor(m["M"]), 1)
        assert same(v.numpy(), m["md"]) and np.array_equal(c.numpy(), m["idx"]), (n1, n2)
        M2 = torch.from_numpy(m["M"].copy())
        M2[:, c] = 100000
        assert same(torch.min(M2, 1)[0].numpy(), m["md2"]), (n1, n2)
    assert ties >= 1


def test_golden_tentatives():
    g = golden()
    m, ref = g["m"], g["g"]
    assert m["count"] == 63 and np.array_equal(m["tent"][:, 0], ref["tent1"]) and np.array_equal(m["tent"][:, 1], ref["tent2"])
    print("golden pair: idx equal to the reference's on %d of 500 rows, min_dist within %.3g, min_2nd within %.3g"
          % ((m["idx"] == ref["idx"]).sum(), np.abs(m["md"] - ref["min_dist"]).max(), np.abs(m["md2"] - ref["min_2nd"]).max()))
    assert np.abs(m["md"] - ref["min_dist"]).max() < 1e-5 and np.abs(m["md2"] - ref["min_2nd"]).max() < 1e-5


def _tie_rows(m):
    """Rows whose minimum is a number attained at two or more columns -> (same lane: two of them 16 apart, other lanes)."""
    M = m["M"]
    same_lane, other_lane = [], []
    for r in np.nonzero((M == m["md"][:, None]).sum(1) >= 2)[0]:
        cols = np.nonzero(M[r] == m["md"][r])[0]
        lanes = cols % 16
        if any(c + 16 in cols for c in cols):
            same_lane.append(int(r))
        if len(set(lanes.tolist())) >= 2:
            other_lane.append(int(r))
    return same_lane, other_lane


def test_input_conditions():
    same_lane, other_lane, tie_min2, nan2, nan2_lanes, nan2_lane = 0, 0, 0, 0, 0, 0
    for n1, n2 in mf.MATCH_SHAPES:
        m = mf.planted_mirror(n1, n2)
        M, keep = m["M"], m["keep"]
        sl, ol = _tie_rows(m)
        same_lane, other_lane = same_lane + len(sl), other_lane + len(ol)
        tie_min2 += int((m["md2"][sl + ol] == m["md"][sl + ol]).sum())
        nan_rows = np.nonzero(np.isnan(M).sum(1) >= 2)[0]
        for r in nan_rows:
            nan2 += 1
            cols = np.nonzero(np.isnan(M[r]))[0]
            nan2_lanes += len(set((cols % 16).tolist())) >= 2
            nan2_lane += len(set((cols % 16).tolist())) < len(cols)
            assert np.isnan(m["md"][r]) and m["idx"][r] == np.nonzero(np.isnan(M[r]))[0][0] and not keep[r]
        if n2 >= 33:
            assert np.unique(m["idx"]).size < n2, "no column is left unmasked"
            assert not (m["md2"] == mf.MASKED).any()
        if n2 >= 40:            # every shape with the planted duplicates has all three kinds of row
            assert len(nan_rows) >= 1 and len(sl) >= 1 and len(ol) >= 1, (n1, n2)
        for i0 in range(0, n1, 1024):
            k = keep[i0:i0 + 1024]
            if n1 >= 1023 and k.size >= 2:
                assert 0 < k.sum() < k.size, "a selection round of one state"
        if n1 > 1024:
            assert not keep[1023] and keep[1024], "the rows on the two sides of the first round's end"
            assert keep[n1 - 1]
    print("tie rows: %d with two columns of one lane, %d across lanes, %d of them with min2 == min1; rows with two NaN columns: %d (%d across lanes, %d in one lane)"
          % (same_lane, other_lane, tie_min2, nan2, nan2_lanes, nan2_lane))
    assert same_lane >= 1 and other_lane >= 1 and tie_min2 >= 1 and nan2 >= 1 and nan2_lanes >= 1 and nan2_lane >= 1
    m = mf.planted_mirror(130, 1)
    assert (m["md2"] == mf.MASKED).all() and (m["idx"] == 0).all() and m["count"] == 130
    assert mf.planted_mirror(1025, 200)["keep"][1024] and mf.planted_mirror(2049, 200)["keep"][2048]


def test_every_wrong_variant_changes_bits():
    n1, n2 = 65, 200
    q, db = mf.planted(n1, n2)
    m = mf.planted_mirror(n1, n2)
    nat = mf.distance(q, db, natural=True)
    print("natural K order: %d of %d distances change" % ((bits(nat) != bits(m["M"])).sum(), nat.size))
    assert (bits(nat) != bits(m["M"])).sum() >= 1
    seq = (bits(mf.sqnorm(db, sequential=True)) != bits(mf.sqnorm(db))).sum()
    print("sequential sum of squares: %d of %d norms change" % (seq, n2))
    assert seq >= 1
    big = mf.match_from_matrix(m["M"], THR, larger_column=True)
    print("ties to the larger column: idx changes on %d rows" % (big["idx"] != m["idx"]).sum())
    assert (big["idx"] != m["idx"]).sum() >= 1
    r, thr = boundary_row(m)
    at, strict = mf.match_from_matrix(m["M"], thr), mf.match_from_matrix(m["M"], thr, strict=True)
    assert at["keep"][r] and not strict["keep"][r] and not same(at["tent"], strict["tent"])
    below = mf.match_from_matrix(m["M"], float(np.nextafter(F32(thr), F32(-np.inf))))
    assert not below["keep"][r]


def boundary_row(m):
    """(row, its float32 ratio as a Python float) of the kept row with the largest finite, positive ratio."""
    ok = m["keep"] & np.isfinite(m["ratio"]) & (m["ratio"] > 0)
    r = int(np.nonzero(ok)[0][np.argmax(m["ratio"][ok])])
    return r, float(m["ratio"][r])


def test_mfma_input_separates_the_chain_from_its_neighbours():
    A, B = mf.mfma_input()
    assert A.shape == (16, 4) and B.shape == (4, 16) and A.dtype == F32 and B.dtype == F32
    e = np.log2(np.abs(np.concatenate([A.ravel(), B.ravel()])))
    assert e.min() < -10 and e.max() > 10 and np.isfinite(e).all()
    want = mf.mfma_chain(A, B)
    assert np.isfinite(want).all()
    differ = {o: int((bits(mf.mfma_chain(A, B, o)) != bits(want)).sum()) for o in mf.K_ORDERS if o != (0, 1, 2, 3)}
    unf = int((bits(mf.mfma_unfused(A, B)) != bits(want)).sum())
    print("elements of 256 that differ from the stated chain: per K order %s; unfused %d" % (sorted(differ.values()), unf))
    assert min(differ.values()) >= 1 and unf >= 1, "an order, or the unfused form, that this input cannot tell from the stated chain"
    f64 = A.astype(np.float64) @ B.astype(np.float64)
    assert (np.abs(f64) < 1e-3 * (np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)))).sum() >= 6, "the cancelling rows cancel"
