"""CPU: the recurrence / cross-similarity kernels (csrc/kernels_segment.h) on the SIMT emulator, through the C entries'
twins, against the definition in tests/segment_ref.py.  D for the model comes from the emulated DTW cost kernel
(emu_dtw_bind): the records (tau, t), connectivity, distance, med_k_scalar and the lag arrays must equal the model in
every bit; affinity and the two mean bandwidths lie within the bounds derived there.  Every buffer lies between poisoned
bands and every row has poisoned pad columns behind it (tests/emu/emu_segment_bind.py): a write outside a row is seen
directly, and a NaN pad read into a sum makes the distance NaN, which is never a neighbour.

`check_case` takes the engine (this emulator, or the device in test_gpu_segment.py) as an argument: the two run the same
sweeps."""

import os
import sys

import numpy as np
import pytest

import dtw_ref
import segment_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_dtw_bind as db  # noqa: E402
import emu_segment_bind as sb  # noqa: E402

CONSTS = sb.constants()
TI = CONSTS["tile_rows"]
SIZES = (1, 2, TI - 1, TI, TI + 1, 2 * TI + 3)
DS = (1, 2, 12, 13, 128)
METRICS = dtw_ref.METRICS
K_KINDS = ("one", "two", "default", "eligible", "above")

# (d, n_ref, n, metric, B, k kind, full, pad_ref, pad_data, pad_out)
CROSS_CASES = (
    (1, 1, 1, "euclidean", 1, "one", False, 0, 0, 0),
    (2, 1, TI + 1, "sqeuclidean", 3, "default", False, 1, 0, 2),
    (12, TI + 1, 1, "cityblock", 1, "two", False, 0, 3, 0),
    (13, 2, 2, "cosine", 3, "above", False, 2, 1, 1),
    (128, TI - 1, TI, "euclidean", 1, "default", False, 0, 0, 0),
    (12, TI, TI - 1, "cosine", 1, "default", True, 1, 1, 0),
    (13, 2 * TI + 3, TI + 1, "sqeuclidean", 1, "eligible", False, 0, 0, 3),
    (2, TI + 1, 2 * TI + 3, "cityblock", 3, "two", True, 3, 0, 0),
    (128, 2 * TI + 3, 2, "cosine", 1, "one", False, 0, 2, 0),
    (1, TI, TI, "cityblock", 1, "above", False, 0, 0, 1),
    (12, 2 * TI + 3, 2 * TI + 3, "euclidean", 1, "default", False, 2, 2, 2),
    (13, TI - 1, TI + 1, "cosine", 3, "two", False, 0, 1, 0),
)
CROSS_IDS = ["d%d-R%d-N%d-%s-B%d-k%s-full%d-pad%d.%d.%d" % c for c in CROSS_CASES]

# (d, n, metric, B, k kind, width kind, sym, self, full, pad, pad_out)
REC_CASES = (
    (1, 1, "euclidean", 1, "default", "one", False, False, False, 0, 0),
    (2, 2, "cityblock", 3, "one", "max", True, True, False, 1, 0),
    (12, TI - 1, "cosine", 1, "default", "one", False, False, False, 0, 2),
    (13, TI, "sqeuclidean", 3, "two", "three", True, False, False, 2, 1),
    (128, TI + 1, "euclidean", 1, "default", "max", False, True, False, 0, 0),
    (12, 2 * TI + 3, "euclidean", 1, "default", "one", True, True, False, 1, 1),
    (2, 2 * TI + 3, "sqeuclidean", 1, "eligible", "three", False, False, False, 0, 0),
    (13, 2 * TI + 3, "cosine", 3, "two", "three", True, False, True, 0, 3),
    (1, TI + 1, "cityblock", 1, "above", "one", False, True, True, 3, 0),
    (128, TI - 1, "cityblock", 1, "one", "three", True, True, False, 0, 0),
    (12, TI, "cosine", 1, "above", "max", True, False, False, 1, 0),
    (2, TI + 1, "euclidean", 3, "default", "three", False, False, True, 0, 1),
)
REC_IDS = ["d%d-N%d-%s-B%d-k%s-w%s-sym%d-self%d-full%d-pad%d.%d" % c for c in REC_CASES]


def pick_k(kind, n_eligible, default):
    return {"one": 1, "two": 2, "default": default, "eligible": max(n_eligible, 1), "above": n_eligible + 5}[kind]


def pick_width(kind, n):
    return {"one": 1, "three": min(3, R.max_width(n)), "max": R.max_width(n)}[kind]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_cost_cache = {}


def cost(X, Y, metric):
    """D (B, n_ref, n) from the emulated DTW cost kernel, once per input; a NaN column of the features (which that
    kernel's binding refuses) is computed as zeros and its row / column of D set to NaN, as any sum with a NaN is."""
    key = (X.tobytes(), Y.tobytes(), X.shape, Y.shape, metric)
    if key not in _cost_cache:
        bad_x, bad_y = np.isnan(X).any(axis=1), np.isnan(Y).any(axis=1)
        D = db.cost(np.nan_to_num(X), np.nan_to_num(Y), metric)
        for b in range(X.shape[0]):
            D[b, bad_x[b], :] = np.nan
            D[b, :, bad_y[b]] = np.nan
        _cost_cache[key] = D
    return _cost_cache[key]


def cosine_gaps_hold(X, Y, k, width):
    """The float64 gap either side of every tau_j exceeds the cost bounds of the two distances it separates: whatever
    rounding a cosine kernel within dtw_ref.cost's bound commits, it selects the same frames."""
    want, bound = dtw_ref.cost(X, Y, "cosine")
    for b in range(want.shape[0]):
        n_ref, n = want[b].shape
        for j in range(n):
            idx = np.array([i for i in range(n_ref) if abs(i - j) >= width])
            if idx.size == 0:
                continue
            o = idx[np.argsort(want[b, idx, j], kind="stable")]
            r = min(k, idx.size) - 1
            for lo, hi in ((r - 1, r), (r, r + 1)):
                if lo >= 0 and hi < o.size and not want[b, o[hi], j] - want[b, o[lo], j] > bound[b, o[hi], j] + bound[b, o[lo], j]:
                    return False
    return True


def check_case(eng, X, Y, metric, k, *, width=0, full=False, sym=False, self_diag=False, pads=(0, 0, 0), what="", lags=True, means=True):
    """One pair through every entry of the engine `eng` (threshold, bandwidth, write, lag) against the model.  X: ref
    (B, d, n_ref) or None for a recurrence pair; returns the worst error / bound seen."""
    Xr = Y if X is None else X
    D = cost(Xr, Y, metric)
    B = Y.shape[0]
    pair = eng.Pair(X, Y, pads[0], pads[1])
    tau, t = eng.threshold(pair, metric, k, width)
    model = [R.neighbours(D[b], k, width, full) for b in range(B)]
    for b in range(B):
        assert same_bits(tau[b], model[b][1]) and np.array_equal(t[b], model[b][2]), f"{what} pair {b}: the records differ from the model's"
    kw = dict(width=width, full=full, sym=sym, self_diag=self_diag, pad_out=pads[2])
    mkw = dict(width=width, full=full, sym=sym, self_diag=self_diag)
    conn = eng.write(pair, metric, "connectivity", tau, t, **kw)
    dist = eng.write(pair, metric, "distance", tau, t, **kw)
    for b in range(B):
        assert conn.dtype == np.bool_ and np.array_equal(conn[b], R.matrix(D[b], k, mode="connectivity", **mkw)[0]), f"{what} pair {b}: connectivity"
        assert same_bits(dist[b], R.matrix(D[b], k, mode="distance", **mkw)[0]), f"{what} pair {b}: distance"
    worst = 0.0
    bws = {}
    for kind in R.BANDWIDTHS if means else R.BANDWIDTHS[:1]:
        bws[kind] = eng.bandwidth(tau, t, kind)
        for b in range(B):
            want, bound = R.bandwidth(tau[b], t[b], kind)
            got = bws[kind][b]
            if np.isnan(want):
                assert np.isnan(got), f"{what} pair {b}: {kind} is {got!r}, the model says NaN"
            elif bound == 0.0:
                assert same_bits(np.float32(got), np.float32(want)), f"{what} pair {b}: {kind} is {got!r}, the model says {want!r}"
            elif np.isfinite(want):
                worst = max(worst, abs(float(got) - want) / bound)
                assert abs(float(got) - want) <= bound, f"{what} pair {b}: {kind} is {got!r}, the model says {want!r} +- {bound:.3g}"
            else:
                assert not np.isfinite(got)
    med = bws["med_k_scalar"]
    if np.isfinite(med).all() and (med > 0).all():
        aff = eng.write(pair, metric, "affinity", tau, t, bw=med, **kw)
        for b in range(B):
            (want, bound), _, _ = R.matrix(D[b], k, mode="affinity", bw=med[b], **mkw)
            worst = max(worst, R.check_affinity(aff[b], want, bound, f"{what} pair {b}: affinity, estimated bandwidth"))
    aff = eng.write(pair, metric, "affinity", tau, t, bandwidth_value=0.37, **kw)
    for b in range(B):
        (want, bound), _, _ = R.matrix(D[b], k, mode="affinity", bw=0.37, **mkw)
        worst = max(worst, R.check_affinity(aff[b], want, bound, f"{what} pair {b}: affinity, bandwidth 0.37"))
    if lags and X is None:
        for src in (conn, dist):
            for pad in (True, False):
                lag = eng.lag(src, True, pad, pad_in=0, pad_out=pads[2])
                assert same_bits(lag, R.to_lag(src, pad)), f"{what}: recurrence_to_lag(pad={pad})"
                assert same_bits(eng.lag(lag, False, pad_in=pads[2]), src), f"{what}: lag_to_recurrence(pad={pad})"
    return worst


def cross_inputs(case):
    d, n_ref, n, metric, B, kk, full, *pads = case
    i = CROSS_CASES.index(case)
    X, Y = dtw_ref.features(B, d, n_ref, 100 + 2 * i), dtw_ref.features(B, d, n, 101 + 2 * i)
    return X, Y, metric, pick_k(kk, n_ref, R.default_k_cross(n_ref)), dict(full=full, pads=tuple(pads))


def rec_inputs(case):
    d, n, metric, B, kk, wk, sym, self_diag, full, pad, pad_out = case
    i = REC_CASES.index(case)
    width = pick_width(wk, n)
    Y = dtw_ref.features(B, d, n, 200 + i)
    n_el = max(n - 2 * width + 1, 0)
    return Y, metric, pick_k(kk, n_el, R.default_k_recurrence(n, width)), dict(width=width, full=full, sym=sym, self_diag=self_diag,
                                                                                 pads=(pad, pad, pad_out))


def test_the_sweeps_cover_what_they_claim():
    col = lambda i, cases: {c[i] for c in cases}                 # noqa: E731
    assert col(0, CROSS_CASES) == set(DS) and col(0, REC_CASES) == set(DS)
    assert col(1, CROSS_CASES) >= set(SIZES) and col(2, CROSS_CASES) >= set(SIZES) and col(1, REC_CASES) >= set(SIZES)
    assert col(3, CROSS_CASES) == set(METRICS) and col(2, REC_CASES) == set(METRICS)
    assert col(4, CROSS_CASES) == {1, 3} and col(3, REC_CASES) == {1, 3}
    assert col(5, CROSS_CASES) == set(K_KINDS) and col(4, REC_CASES) == set(K_KINDS)
    assert col(5, REC_CASES) == {"one", "three", "max"}
    for i in (6, 7, 8):
        assert col(i, REC_CASES) == {False, True}
    assert col(6, CROSS_CASES) == {False, True}
    assert any(c[7] for c in CROSS_CASES) and any(c[8] for c in CROSS_CASES) and any(c[9] for c in CROSS_CASES)
    assert any(c[9] for c in REC_CASES) and any(c[10] for c in REC_CASES)
    assert SIZES == (1, 2, 63, 64, 65, 131) and 13 <= CONSTS["chunk"] < 128, "d = 128 takes more than one chunk"
    assert CONSTS["max_features"] == db.constants()["max_features"], "the cap on d is the cost kernel's"
    assert CONSTS["max_len"] >= 16384
    for case in CROSS_CASES:
        if case[3] == "cosine":
            X, Y, metric, k, kw = cross_inputs(case)
            assert cosine_gaps_hold(X, Y, k, 0), f"{case}: choose another seed"
    for case in REC_CASES:
        if case[2] == "cosine":
            Y, metric, k, kw = rec_inputs(case)
            assert cosine_gaps_hold(Y, Y, k, kw["width"]), f"{case}: choose another seed"


@pytest.mark.parametrize("case", CROSS_CASES, ids=CROSS_IDS)
def test_emu_cross_similarity_sweep(case):
    X, Y, metric, k, kw = cross_inputs(case)
    print(f"worst error / bound {check_case(sb, X, Y, metric, k, what=str(case), **kw):.4f}")


@pytest.mark.parametrize("case", REC_CASES, ids=REC_IDS)
def test_emu_recurrence_sweep(case):
    Y, metric, k, kw = rec_inputs(case)
    print(f"worst error / bound {check_case(sb, None, Y, metric, k, what=str(case), **kw):.4f}")


# ---------------------------------------------------------------------------------------------------------------------
# ties: inputs whose distances are exact, so that every summation order agrees
# ---------------------------------------------------------------------------------------------------------------------
TN = 41                                                         # frames of a tie case: one tile, a query per workgroup


def tie_inputs(kind, seed=0):
    """Y (1, d, TN) with many tied distances."""
    rng = np.random.default_rng(300 + seed)
    if kind == "integers":
        return rng.integers(-2, 3, (1, 3, TN)).astype(np.float32)
    if kind == "duplicates":
        Y = dtw_ref.features(1, 5, TN, 40)
        Y[:, :, 1::3] = Y[:, :, 0::3][:, :, :Y[:, :, 1::3].shape[2]]      # every third column repeats its neighbour: distance 0
        Y[:, :, 30:34] = Y[:, :, 5:6]
        return Y
    if kind == "constant":
        return np.full((1, 4, TN), 0.75, np.float32)
    if kind == "nan":
        Y = dtw_ref.features(1, 5, TN, 41)
        Y[0, 2, 9] = np.nan
        Y[0, :, 33] = np.nan
        return Y
    if kind == "zero":
        Y = rng.integers(-2, 3, (1, 3, TN)).astype(np.float32)
        Y[:, :, 4] = 0.0
        Y[:, :, 35] = 0.0
        return Y
    raise ValueError(kind)


EXACT = ("sqeuclidean", "cityblock", "euclidean")
TIE_CASES = [(kind, m) for kind in ("integers", "duplicates") for m in EXACT] + [("constant", m) for m in METRICS] + \
    [("nan", m) for m in METRICS] + [("zero", "cosine")]


def check_ties(eng, kind, metric):
    Y = tie_inputs(kind)
    n = Y.shape[2]
    D = cost(Y, Y, metric)
    if kind == "zero":
        # cosine of small integers is not exact: the zero vector's distances (exactly 1, many of them) are the point
        assert (np.delete(D[0, 4, :], [4, 35]) == 1.0).all() and (D[0, :, 35] == 1.0).all()
    for k, width, sym, self_diag in ((5, 1, True, True), (R.default_k_recurrence(n, 3), 3, False, False)):
        check_case(eng, None, Y, metric, k, width=width, sym=sym, self_diag=self_diag, pads=(1, 1, 2), what=f"{kind} {metric} k={k}",
                   lags=False, means=False)
    check_case(eng, Y[:, :, :TN - 3].copy(), Y, metric, 4, pads=(0, 2, 1), what=f"{kind} {metric} cross", means=False)
    return D


@pytest.mark.parametrize("kind, metric", TIE_CASES)
def test_emu_ties_go_to_the_smaller_index(kind, metric):
    D = check_ties(sb, kind, metric)
    Y = tie_inputs(kind)
    pair = sb.Pair(None, Y)
    if kind == "constant" and metric == "euclidean":
        # every distance ties: the index alone decides
        tau, t = sb.threshold(pair, metric, 3, 2)
        conn = sb.write(pair, metric, "connectivity", tau, t, width=2)
        assert (tau == 0.0).all()
        assert np.flatnonzero(conn[0][:, 0]).tolist() == [2, 3, 4] and np.flatnonzero(conn[0][:, 5]).tolist() == [0, 1, 2]
        assert np.flatnonzero(conn[0][:, 3]).tolist() == [0, 1, 5] and t[0, 3] == 5 and t[0, 0] == 4
    if kind == "integers":
        assert all(len(np.unique(D[0][:, j])) < D.shape[1] - 5 for j in range(D.shape[2])), "every query has tied distances"
    if kind == "nan" and metric == "euclidean":
        assert np.isnan(D[0][9]).all() and np.isnan(D[0][:, 33]).all()
        tau, t = sb.threshold(pair, metric, 4, 1)
        assert np.isnan(tau[0, [9, 33]]).all() and (t[0, [9, 33]] == -1).all() and not np.isnan(np.delete(tau[0], [9, 33])).any()
        conn = sb.write(pair, metric, "connectivity", tau, t, width=1, full=True)
        assert not conn[0][9].any() and not conn[0][:, 9].any() and conn[0][0, 5]


def test_emu_median_of_an_even_count_and_bandwidths_without_neighbours():
    tau = np.array([[3.0, 1.0, np.nan, 2.0, 8.0, 0.5], [np.nan] * 6, [4.0, 4.0, 1.0, 1.0, 1.0, 9.0]], np.float32)
    t = np.array([[0, 1, -1, 2, 3, -1], [-1] * 6, [0, 0, 0, 0, -1, 0]], np.int32)
    med = sb.bandwidth(tau, t, "med_k_scalar")
    assert med[0] == np.float32(2.5) and np.isnan(med[1]) and med[2] == np.float32(4.0)      # {1, 2, 3, 8}; none; {1, 1, 4, 4, 9}
    for kind in ("mean_k", "gmean_k"):
        got = sb.bandwidth(tau, t, kind)
        assert np.isnan(got[1])
        for b in (0, 2):
            want, bound = R.bandwidth(tau[b], t[b], kind)
            assert abs(float(got[b]) - want) <= bound
    big = np.array([[3.0e38, 3.2e38]], np.float32)                        # fl(a + b) overflows: the definition says so
    assert np.isinf(sb.bandwidth(big, np.zeros((1, 2), np.int32), "med_k_scalar")[0]) and np.isinf(R.bandwidth(big[0], [0, 0], "med_k_scalar")[0])
    tau = dtw_ref.cost_matrix(2, 1, 5 * TI + 1, 3)[:, 0, :]
    t = np.zeros(tau.shape, np.int32)
    t[0, ::7] = -1
    for kind in R.BANDWIDTHS:
        got = sb.bandwidth(tau, t, kind)
        for b in range(2):
            want, bound = R.bandwidth(tau[b], t[b], kind)
            assert (same_bits(np.float32(got[b]), np.float32(want)) if bound == 0.0 else abs(float(got[b]) - want) <= bound), (kind, b)


@pytest.mark.parametrize("grid", [1, 3])
def test_emu_grid_overrides_and_a_pair_alone(grid):
    Y = dtw_ref.features(3, 5, TI + 9, 50)
    pair = sb.Pair(None, Y, 0, 1)
    tau, t = sb.threshold(pair, "euclidean", 6, 2)
    tau_g, t_g = sb.threshold(pair, "euclidean", 6, 2, grid=grid)
    assert sb.geometry()["grid"] == grid and same_bits(tau, tau_g) and np.array_equal(t, t_g)
    a = sb.write(pair, "euclidean", "distance", tau, t, width=2, sym=True)
    assert same_bits(a, sb.write(pair, "euclidean", "distance", tau, t, width=2, sym=True, grid=grid))
    assert same_bits(sb.lag(a, True, grid=grid), sb.lag(a, True))
    assert same_bits(sb.bandwidth(tau, t, "med_k_scalar", grid=grid), sb.bandwidth(tau, t, "med_k_scalar"))
    one = sb.Pair(None, Y[1:2])
    tau1, t1 = sb.threshold(one, "euclidean", 6, 2)
    assert same_bits(tau1[0], tau[1]) and np.array_equal(t1[0], t[1])
    assert same_bits(sb.write(one, "euclidean", "distance", tau1, t1, width=2, sym=True)[0], a[1])


def test_emu_hand_case():
    # four points on a line: 0, 1, 3, 7
    Y = np.array([[[0.0, 1.0, 3.0, 7.0]]], np.float32)
    pair = sb.Pair(None, Y)
    tau, t = sb.threshold(pair, "cityblock", 1, 1)
    np.testing.assert_array_equal(tau[0], [1, 1, 2, 4])
    np.testing.assert_array_equal(t[0], [1, 0, 1, 2])
    conn = sb.write(pair, "cityblock", "connectivity", tau, t, width=1)
    np.testing.assert_array_equal(conn[0].astype(int), [[0, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]])
    sym = sb.write(pair, "cityblock", "distance", tau, t, width=1, sym=True, self_diag=True)
    np.testing.assert_array_equal(sym[0], [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    aff = sb.write(pair, "cityblock", "affinity", tau, t, width=1, self_diag=True, bandwidth_value=2.0)
    np.testing.assert_allclose(aff[0], [[1, np.exp(-0.5), 0, 0], [np.exp(-0.5), 1, np.exp(-1), 0], [0, 0, 1, np.exp(-2)], [0, 0, 0, 1]], rtol=1e-6)
    lag = sb.lag(conn, True)
    np.testing.assert_array_equal(lag[0].astype(int), [[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0],
                                                       [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 1, 1]])
    np.testing.assert_array_equal(sb.lag(conn, True, pad=False)[0].astype(int), [[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 1, 1, 1]])


def test_emu_prepare_rejects():
    f = np.zeros(64, np.float32).ctypes.data
    w = np.zeros(64, np.uint32).ctypes.data
    INV, UNS = -1, -2
    cap_d, cap = CONSTS["max_features"], CONSTS["max_len"]
    thr = lambda *a: sb.raw_status("emu_segment_threshold_f32", *a, 0)          # noqa: E731
    for args, rc, word in (
        ((None, f, 1, 2, 3, 4, 3, 4, 0, 1, 0, w), INV, "NULL"), ((f, f, 1, 2, 3, 4, 3, 4, 0, 1, 0, None), INV, "NULL"),
        ((f, f, 0, 2, 3, 4, 3, 4, 0, 1, 0, w), INV, "non-empty"), ((f, f, 1, 2, 0, 4, 3, 4, 0, 1, 0, w), INV, "non-empty"),
        ((f, f, 1, 0, 3, 4, 3, 4, 0, 1, 0, w), INV, "d must"), ((f, f, 1, cap_d + 1, 3, 4, 3, 4, 0, 1, 0, w), INV, "d must"),
        ((f, f, 1, 2, 3, 4, 3, 4, 4, 1, 0, w), INV, "metric"), ((f, f, 1, 2, 3, 4, 2, 4, 0, 1, 0, w), INV, "ref_row_stride"),
        ((f, f, 1, 2, 3, 4, 3, 3, 0, 1, 0, w), INV, "data_row_stride"), ((f, f, 1, 2, 3, 4, 3, 4, 0, 0, 0, w), INV, "k must"),
        ((f, f, 1, 2, 3, 4, 3, 4, 0, 1, 1, w), INV, "width"), ((f, f, 1, 2, 4, 4, 4, 4, 0, 1, -1, w), INV, "width"),
        ((f, f, 1, 2, cap + 1, 4, cap + 1, 4, 0, 1, 0, w), UNS, "exceed"), ((f, f, 1, 2, 4, cap + 1, 4, cap + 1, 0, 1, 0, w), UNS, "exceed"),
    ):
        assert thr(*args) == rc and word in sb.last_error(), (args, sb.last_error())
    wr = lambda *a: sb.raw_status("emu_segment_write_f32", *a, 0)               # noqa: E731
    for args, rc, word in (
        ((f, f, 1, 2, 4, 4, 4, 4, 0, 0, 1, 0, 0, 0, None, None, 1.0, f, 4), INV, "NULL"),
        ((f, f, 1, 2, 4, 4, 4, 4, 0, 3, 1, 0, 0, 0, w, None, 1.0, f, 4), INV, "mode"),
        ((f, f, 1, 2, 3, 4, 3, 4, 0, 0, 0, 0, 1, 0, w, None, 1.0, f, 4), INV, "sym"),
        ((f, f, 1, 2, 3, 4, 3, 4, 0, 0, 0, 0, 0, 1, w, None, 1.0, f, 4), INV, "self"),
        ((f, f, 1, 2, 4, 4, 4, 4, 0, 0, 1, 0, 0, 0, w, None, 1.0, f, 3), INV, "out_row_stride"),
        ((f, f, 1, 2, 4, 4, 4, 4, 0, 2, 1, 0, 0, 0, w, None, 0.0, f, 4), INV, "bandwidth"),
        ((f, f, 1, 2, 4, 4, 4, 4, 0, 2, 1, 0, 0, 0, w, None, float("nan"), f, 4), INV, "bandwidth"),
    ):
        assert wr(*args) == rc and word in sb.last_error(), (args, sb.last_error())
    bw = lambda *a: sb.raw_status("emu_segment_bandwidth_f32", *a, 0)           # noqa: E731
    for args, rc, word in (((None, 1, 4, 0, f), INV, "NULL"), ((w, 0, 4, 0, f), INV, "non-empty"), ((w, 1, 4, 3, f), INV, "kind"),
                           ((w, 1, cap + 1, 0, f), UNS, "exceed")):
        assert bw(*args) == rc and word in sb.last_error(), (args, sb.last_error())
    lg = lambda *a: sb.raw_status("emu_segment_lag", *a, 0)                     # noqa: E731
    for args, rc, word in (((None, 1, 4, 4, 4, 1, 4, f, 4), INV, "NULL"), ((f, 1, 0, 0, 4, 1, 4, f, 4), INV, "non-empty"),
                           ((f, 1, 4, 5, 4, 1, 4, f, 4), INV, "n or 2 n"), ((f, 1, 4, 8, 2, 1, 4, f, 4), INV, "1 or 4"),
                           ((f, 1, 4, 8, 4, 1, 3, f, 4), INV, "in_row_stride"), ((f, 1, 4, 8, 4, 1, 4, f, 3), INV, "out_row_stride"),
                           ((f, 1, cap + 1, cap + 1, 4, 1, cap + 1, f, cap + 1), UNS, "exceed")):
        assert lg(*args) == rc and word in sb.last_error(), (args, sb.last_error())
