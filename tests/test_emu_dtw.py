"""CPU: the DTW kernels (csrc/kernels_dtw.h) on the SIMT emulator, through the C entries' twins, against the definition
in tests/dtw_ref.py.  D, the step codes and the paths must equal the model in every bit; the cost kernel lies within
the bound derived there.  Every buffer lies between NaN bands and every row has NaN pad columns behind it
(tests/emu/emu_dtw_bind.py): a write outside a row is seen directly, and a -inf pad (which wins every comparison it
enters) shows a read outside one."""

import os
import sys

import numpy as np
import pytest

import dtw_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_dtw_bind as eb  # noqa: E402

CONSTS = eb.constants()
TW, TH, CAP = CONSTS["tile_w"], CONSTS["tile_h"], CONSTS["max_step"]
WIN = CONSTS["window"]
DEFAULT = ((1, 1), (0, 1), (1, 0))
SPARSE = ((1, 1), (1, 2), (2, 1))                               # leaves unreachable cells
WIDE = ((1, 1), (0, CAP), (CAP, 0), (2, 3), (1, 0))             # a component at the cap, non-trivial weights
WIDE_ADD = (0.5, 0.25, 1.0, 0.0, 0.125)
WIDE_MUL = (1.0, 2.0, 1.5, 3.0, 0.75)
TABLES = {"default": (DEFAULT, None, None), "sparse": (SPARSE, None, None), "wide": (WIDE, WIDE_ADD, WIDE_MUL),
          "weighted": (DEFAULT, (0.5, 0.25, 1.0), (1.0, 2.0, 1.5))}
SIZES = (1, 2, TW - 1, TW, TW + 1, TH + 1, 2 * TW + 3)

# (N, M, B, table, subseq, band_rad or None, pad_in, pad_out)
ACC_CASES = (
    (1, 1, 1, "default", False, None, 0, 0),
    (1, 2 * TW + 3, 1, "default", True, None, 1, 0),
    (2 * TW + 3, 1, 3, "default", False, None, 0, 2),
    (1, TW + 1, 1, "wide", False, None, 0, 0),
    (TH + 1, 1, 1, "sparse", False, None, 3, 1),
    (2, 2, 3, "sparse", True, 1.0, 0, 0),
    (2, TW, 1, "wide", True, None, 2, 0),
    (TW - 1, TW - 1, 1, "default", False, 0.25, 0, 0),
    (TW, TW, 3, "default", True, 0.1, 1, 3),
    (TW + 1, TW + 1, 1, "sparse", False, None, 0, 0),
    (TH + 1, TW - 1, 1, "wide", False, 1.0, 5, 0),
    (TW - 1, 2 * TW + 3, 3, "weighted", False, 0.25, 0, 1),
    (2 * TW + 3, TW + 1, 1, "default", False, 0.1, 2, 2),
    (2 * TW + 3, 2 * TW + 3, 1, "default", False, None, 0, 0),
    (2 * TW + 3, 2 * TW + 3, 3, "sparse", True, 0.25, 1, 0),
    (2 * TW + 3, TW, 1, "wide", True, 0.1, 0, 4),
    (TW, 2 * TW + 3, 1, "wide", False, 0.25, 3, 0),
    (TW + 1, 2, 3, "weighted", True, None, 0, 0),
    (4 * TH + 5, 3, 1, "default", False, None, 1, 1),             # N much larger than M
    (4 * TH + 5, 2, 1, "sparse", True, 1.0, 0, 0),
    (TH + 1, 2 * TW + 3, 3, "sparse", False, 1.0, 0, 0),
)
ACC_IDS = ["N%d-M%d-B%d-%s-sub%d-band%s-pad%d.%d" % c for c in ACC_CASES]


def acc_case(case, kind="uniform"):
    """(C, keyword arguments shared by eb.accumulate and R.accumulate, the layout arguments of eb.accumulate)."""
    N, M, B, tab, subseq, band_rad, pad_in, pad_out = case
    i = ACC_CASES.index(case) if case in ACC_CASES else 99
    steps, add, mul = TABLES[tab]
    band_r = None if band_rad is None else R.band_radius(band_rad, N, M)
    return R.cost_matrix(B, N, M, i, kind), dict(steps=steps, add=add, mul=mul, subseq=subseq, band_r=band_r), dict(pad_in=pad_in, pad_out=pad_out)


_ref_cache = {}


def reference(C, kw):
    """R.accumulate of every pair of C, computed once per input."""
    key = (C.tobytes(), C.shape, repr(sorted(kw.items(), key=lambda p: p[0])))
    if key not in _ref_cache:
        pairs = [R.accumulate(C[b], **kw) for b in range(C.shape[0])]
        _ref_cache[key] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    return _ref_cache[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same(D, S, Dr, Sr, what=""):
    bad = np.argwhere(D.view(np.uint32) != Dr.view(np.uint32))
    assert bad.size == 0, f"{what}: D differs in {len(bad)} cells, first at {tuple(bad[0])}: {D[tuple(bad[0])]!r} != {Dr[tuple(bad[0])]!r}"
    bad = np.argwhere(S != Sr)
    assert bad.size == 0, f"{what}: steps differ in {len(bad)} cells, first at {tuple(bad[0])}: {S[tuple(bad[0])]} != {Sr[tuple(bad[0])]}"


def assert_paths(got, S, D, steps, subseq, what=""):
    """The emulated paths of a batch against the model's, and the properties of a path."""
    for b, p in enumerate(got):
        want = R.backtrack(S[b], steps, D=D[b], subseq=subseq)
        if want is None:
            assert p is None, f"{what} pair {b}: a path where the model has none"
            continue
        assert p is not None and np.array_equal(p, want), f"{what} pair {b}: the path differs from the model's"
        assert S[b][tuple(p[-1])] == R.START and p[0][0] == S.shape[1] - 1
        assert (np.diff(p[:, 0]) <= 0).all() and (np.diff(p[:, 1]) <= 0).all()


def test_the_sweeps_cover_what_they_claim():
    col = lambda i, cases: {c[i] for c in cases}                 # noqa: E731
    assert col(0, ACC_CASES) >= set(SIZES) and col(1, ACC_CASES) >= set(SIZES) and col(2, ACC_CASES) == {1, 3}
    assert col(3, ACC_CASES) == set(TABLES) and col(4, ACC_CASES) == {False, True} and col(5, ACC_CASES) == {None, 0.1, 0.25, 1.0}
    assert any(c[6] for c in ACC_CASES) and any(c[7] for c in ACC_CASES)
    assert any(c[0] == 1 and c[1] > TW for c in ACC_CASES) and any(c[1] == 1 and c[0] > TH for c in ACC_CASES)
    assert any(c[0] >= 4 * TH and c[1] <= 3 for c in ACC_CASES), "N much larger than M"
    for tab in TABLES:                                          # every table with and without subseq, with and without a band
        mine = [c for c in ACC_CASES if c[3] == tab]
        assert col(4, mine) == {False, True} and None in col(5, mine) and len(col(5, mine)) > 1, tab
    assert max(max(s) for s in WIDE) == CAP and CAP >= 2
    assert any(eb_fast(c) for c in ACC_CASES) and any(not eb_fast(c) for c in ACC_CASES)
    assert col(0, COST_CASES) == {1, 2, 12, 13, 128} and col(3, COST_CASES) == set(R.METRICS)
    edge = {1, CONSTS["cost_tile_rows"] - 1, CONSTS["cost_tile_rows"], CONSTS["cost_tile_rows"] + 1}
    assert col(1, COST_CASES) >= edge and col(2, COST_CASES) >= edge and CONSTS["cost_tile_rows"] == CONSTS["cost_tile_cols"]
    assert 13 <= CONSTS["cost_chunk"] < 128, "d = 128 takes more than one chunk, 12 and 13 one"


def eb_fast(case):
    return TABLES[case[3]][0] == DEFAULT


@pytest.mark.parametrize("case", ACC_CASES, ids=ACC_IDS)
def test_emu_accumulate_and_backtrack_sweep(case):
    C, kw, lay = acc_case(case)
    D, S = eb.accumulate(C, **kw, **lay)
    assert eb.geometry()["fast"] == int(eb_fast(case))
    Dr, Sr = reference(C, kw)
    assert_same(D, S, Dr, Sr, case)
    paths = eb.backtrack(S, kw["steps"], D=D, subseq=kw["subseq"], pad=lay["pad_out"])
    assert_paths(paths, S, D, kw["steps"], kw["subseq"], case)
    if case[3] in ("default", "weighted") and kw["band_r"] is None:
        assert all(p is not None for p in paths), "the default steps reach every cell"


@pytest.mark.parametrize("tab", sorted(TABLES))
@pytest.mark.parametrize("kind", ["ties", "signed"])
def test_emu_ties_and_negative_costs(tab, kind):
    """Costs in {0, 1, 2}: ties everywhere, the first step index must win.  Costs in [-1, 1): nothing assumes c >= 0."""
    steps, add, mul = TABLES[tab]
    for subseq in (False, True):
        C = R.cost_matrix(2, TW + 3, TH + 7, 7, kind)
        kw = dict(steps=steps, add=add, mul=mul, subseq=subseq, band_r=None)
        D, S = eb.accumulate(C, **kw, pad_in=1)
        Dr, Sr = reference(C, kw)
        assert_same(D, S, Dr, Sr, (tab, kind, subseq))
        if kind == "ties" and tab == "default" and not subseq:
            tied = 0
            for i in range(1, C.shape[1]):
                for j in range(1, C.shape[2]):
                    preds = (Dr[0, i - 1, j - 1], Dr[0, i, j - 1], Dr[0, i - 1, j])
                    if preds.count(min(preds)) > 1:
                        tied += 1
                        assert Sr[0, i, j] == preds.index(min(preds))
            assert tied > 100, "the input has ties"
        assert_paths(eb.backtrack(S, steps, D=D, subseq=subseq), S, D, steps, subseq, (tab, kind))


@pytest.mark.parametrize("tab", ["default", "wide"])
def test_emu_nan_and_inf_costs_make_the_cells_the_definition_says(tab):
    steps, add, mul = TABLES[tab]
    C = R.cost_matrix(1, TH + 9, TW + 9, 11)
    C[0, 3, :] = np.inf                                         # a wall: only the steps that jump over a row cross it
    C[0, TH + 2, 5] = np.nan
    C[0, 10:20, TW - 1:TW + 2] = np.nan
    C[0, 30, 40] = -np.inf
    kw = dict(steps=steps, add=add, mul=mul, subseq=False, band_r=None)
    D, S = eb.accumulate(C, **kw)
    Dr, Sr = reference(C, kw)
    assert_same(D, S, Dr, Sr, tab)
    assert not np.isnan(D).any() and (S[np.isnan(C)] == R.NONE).all() and np.isinf(D[np.isnan(C)]).all()
    assert (S[0, 3, :] == R.NONE).all()
    if tab == "default":
        assert (S[0, 4:, :] == R.NONE).all(), "nothing crosses the wall with steps of one row"
        assert eb.backtrack(S) == [None]
    else:
        assert (S[0, 4:, :] != R.NONE).any()


def test_emu_reads_stay_inside_the_payload():
    """-inf behind every row of C: it would win every comparison it entered."""
    for tab in ("default", "wide"):
        steps, add, mul = TABLES[tab]
        C = R.cost_matrix(2, TH + 3, TW + 5, 5)
        kw = dict(steps=steps, add=add, mul=mul, subseq=True, band_r=None)
        D, S = eb.accumulate(C, **kw, pad_in=7, pad_out=5, poison=-np.inf)
        assert_same(D, S, *reference(C, kw), tab)


def test_emu_a_pair_alone_and_in_a_batch():
    for tab in ("default", "sparse"):
        steps, add, mul = TABLES[tab]
        C = R.cost_matrix(3, TH + 5, 2 * TW + 1, 13)
        kw = dict(steps=steps, add=add, mul=mul, subseq=False, band_r=R.band_radius(0.25, TH + 5, 2 * TW + 1))
        D, S = eb.accumulate(C, **kw)
        for b in range(3):
            D1, S1 = eb.accumulate(C[b:b + 1], **kw)
            assert same_bits(D1[0], D[b]) and np.array_equal(S1[0], S[b])
            p1, = eb.backtrack(S1, steps)
            pb = eb.backtrack(S, steps)[b]
            assert (p1 is None and pb is None) or np.array_equal(p1, pb)


@pytest.mark.parametrize("grid", [1, 2, 5])
def test_emu_grid_overrides(grid):
    for tab in ("default", "wide"):
        steps, add, mul = TABLES[tab]
        C = R.cost_matrix(3, 2 * TH + 3, 2 * TW + 3, 17)
        kw = dict(steps=steps, add=add, mul=mul, subseq=True, band_r=None)
        Dr, Sr = reference(C, kw)
        D, S = eb.accumulate(C, **kw, grid=grid)
        assert eb.geometry()["grid"] == grid and eb.geometry()["launches"] == 5
        assert_same(D, S, Dr, Sr, (tab, grid))
        assert_paths(eb.backtrack(S, steps, D=D, subseq=True, grid=grid), S, D, steps, True, (tab, grid))
    X, Y = R.features(3, 5, TW + 1, 1), R.features(3, 5, 2 * TW + 1, 2)
    assert same_bits(eb.cost(X, Y, "euclidean", grid=grid), eb.cost(X, Y, "euclidean"))


def test_emu_hand_case():
    C = np.array([[[1, 2, 3], [4, 1, 2], [7, 5, 1]]], np.float32)
    D, S = eb.accumulate(C)
    np.testing.assert_array_equal(D[0], np.array([[1, 3, 6], [5, 2, 4], [12, 7, 3]], np.float32))
    np.testing.assert_array_equal(S[0], np.array([[254, 1, 1], [2, 0, 1], [2, 2, 0]], np.uint8))
    path, = eb.backtrack(S)
    np.testing.assert_array_equal(path, [[2, 2], [1, 1], [0, 0]])
    assert path.dtype == np.int32
    np.testing.assert_array_equal(R.accumulate(C[0])[0], D[0])


def test_emu_backtrack_crosses_window_seams_and_starts_at_the_first_minimum():
    # a staircase that runs along row 0, down a column and along the last row: it leaves every window through a side
    N, M = 2 * WIN + 5, 2 * WIN + 9
    S = np.full((1, N, M), 1, np.uint8)                         # (0, 1): left
    S[0, 1:, WIN + 3] = 2                                       # (1, 0): up
    S[0, 0, 0] = R.START
    path, = eb.backtrack(S)
    want = R.backtrack(S[0])
    assert len(want) == N + M - 1, "the longest path there is"
    np.testing.assert_array_equal(path, want)
    # the diagonal leaves every window through its corner
    S = np.zeros((2, 3 * WIN + 1, 3 * WIN + 1), np.uint8)
    S[:, 0, 0] = R.START
    S[1, WIN + 7, WIN + 7] = R.NONE                             # pair 1: the path runs into a dead cell
    paths = eb.backtrack(S)
    np.testing.assert_array_equal(paths[0], np.repeat(np.arange(3 * WIN, -1, -1), 2).reshape(-1, 2))
    assert paths[1] is None
    # steps that would leave the matrix, and a code that is no step
    S = np.zeros((1, 3, 5), np.uint8)
    assert eb.backtrack(S) == [None]
    S[0, 2, 4] = 3
    assert eb.backtrack(S) == [None]
    # subseq: the first minimum of a tied last row; start columns given instead of D
    C = R.cost_matrix(2, 5, 3 * WIN + 2, 19)
    C[:, -1, :] = 0.0
    D, S = eb.accumulate(C, subseq=True)
    Dr, Sr = reference(C, dict(steps=None, add=None, mul=None, subseq=True, band_r=None))
    assert_same(D, S, Dr, Sr)
    D[:, -1, :] = 5.0
    D[0, -1, [70, 2 * WIN + 1, 7, 64]] = 1.0                    # ties in several lanes' columns: the smallest j wins
    D[1, -1, [WIN + 1, WIN + 65]] = -np.inf
    paths = eb.backtrack(S, D=D, subseq=True, pad=3)
    assert paths[0][0].tolist() == [4, 7] and paths[1][0].tolist() == [4, WIN + 1]
    for b in range(2):
        np.testing.assert_array_equal(paths[b], R.backtrack(S[b], D=D[b], subseq=True))
    D[:] = np.inf                                               # nothing below +inf: column 0, as argmin says
    assert eb.backtrack(S, D=D, subseq=True)[0][0].tolist() == [4, 0]
    given = eb.backtrack(S, start=[9, 3 * WIN + 1])
    assert given[0][0].tolist() == [4, 9] and given[1][0].tolist() == [4, 3 * WIN + 1]
    np.testing.assert_array_equal(given[0], R.backtrack(S[0], start=9))


def test_emu_unreachable_end_gives_minus_one():
    C = R.cost_matrix(2, 5, 40, 23)
    D, S = eb.accumulate(C, SPARSE)                             # 5 rows, 40 columns: (4, 39) needs at most 2 columns per row
    assert S[0, 4, 39] == R.NONE and np.isinf(D[0, 4, 39])
    assert eb.backtrack(S, SPARSE) == [None, None]
    r = R.band_radius(0.1, 40, 40)
    D, S = eb.accumulate(R.cost_matrix(1, 40, 40, 24), band_r=r)
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    np.testing.assert_array_equal(S[0] == R.NONE, ~R.in_band(i, j, 40, 40, r))


# ---------------------------------------------------------------------------------------------------------------------
# cost
# ---------------------------------------------------------------------------------------------------------------------
CT = CONSTS["cost_tile_rows"]
# (d, N, M, metric, B, pad_x, pad_y, pad_out)
COST_CASES = (
    (1, 1, 1, "euclidean", 1, 0, 0, 0),
    (2, CT - 1, CT + 1, "sqeuclidean", 3, 1, 0, 2),
    (12, CT, CT, "cityblock", 1, 0, 3, 0),
    (13, CT + 1, CT - 1, "cosine", 3, 2, 1, 1),
    (128, CT + 1, 1, "euclidean", 1, 0, 0, 0),
    (128, 1, CT + 1, "cosine", 1, 1, 1, 0),
    (12, 2 * CT + 3, CT - 1, "cosine", 1, 0, 0, 3),
    (13, CT - 1, 2 * CT + 3, "euclidean", 1, 3, 0, 0),
    (128, CT, CT + 1, "sqeuclidean", 1, 0, 2, 0),
    (128, CT + 1, CT, "cityblock", 3, 0, 0, 1),
    (1, CT + 1, CT + 1, "cityblock", 1, 0, 0, 0),
    (2, 1, CT, "cosine", 3, 0, 0, 0),
    (1, CT, 1, "sqeuclidean", 1, 0, 1, 0),
)
COST_IDS = ["d%d-N%d-M%d-%s-B%d-pad%d.%d.%d" % c for c in COST_CASES]


def cost_case(case):
    d, N, M, metric, B, pad_x, pad_y, pad_out = case
    i = COST_CASES.index(case)
    return R.features(B, d, N, 2 * i), R.features(B, d, M, 2 * i + 1), dict(pad_x=pad_x, pad_y=pad_y, pad_out=pad_out)


@pytest.mark.parametrize("case", COST_CASES, ids=COST_IDS)
def test_emu_cost_sweep(case):
    X, Y, lay = cost_case(case)
    got = eb.cost(X, Y, case[3], **lay)
    want, bound = R.cost(X, Y, case[3])
    print(f"cost {COST_IDS[COST_CASES.index(case)]}: worst error / bound {R.check_cost(got, want, bound, case):.4f}")


def test_emu_cost_special_values():
    X = R.features(2, 13, CT + 3, 31)
    for metric in ("euclidean", "sqeuclidean", "cityblock"):
        got = eb.cost(X, X, metric)
        assert (np.diagonal(got, axis1=1, axis2=2) == 0.0).all(), f"{metric}: x == y gives exactly 0"
        assert (got >= 0.0).all()
    Y = X.copy()
    Y[:, :, 5] = 0.0                                            # a zero vector: the product of norms counts as 1
    got = eb.cost(X, Y, "cosine")
    assert (got[:, :, 5] == 1.0).all()
    got = eb.cost(Y, Y, "cosine")
    assert got[0, 5, 5] == 1.0 and abs(got[0, 6, 6]) <= 16 * R.U
    want, bound = R.cost(X, Y, "cosine")
    R.check_cost(eb.cost(X, Y, "cosine"), want, bound, "zero column")
    same = eb.cost(X, X.copy(), "euclidean")
    assert np.array_equal(same, np.swapaxes(same, 1, 2)), "(x - y)^2 == (y - x)^2"


def test_emu_prepare_rejects():
    f = np.zeros(64, np.float32).ctypes.data
    u = np.zeros(64, np.uint8).ctypes.data
    i = np.zeros(64, np.int32).ctypes.data
    INV, UNS = -1, -2
    cap_d, cap_len = CONSTS["max_features"], CONSTS["max_len"]
    for args, rc, word in (
        ((None, f, 1, 2, 3, 4, 3, 4, 0, f, 4), INV, "NULL"), ((f, f, 1, 2, 3, 4, 3, 4, 0, None, 4), INV, "NULL"),
        ((f, f, 0, 2, 3, 4, 3, 4, 0, f, 4), INV, "non-empty"), ((f, f, 1, 2, 0, 4, 3, 4, 0, f, 4), INV, "non-empty"),
        ((f, f, 1, 0, 3, 4, 3, 4, 0, f, 4), INV, "d must"), ((f, f, 1, cap_d + 1, 3, 4, 3, 4, 0, f, 4), INV, "d must"),
        ((f, f, 1, 2, 3, 4, 3, 4, 4, f, 4), INV, "metric"), ((f, f, 1, 2, 3, 4, 3, 4, -1, f, 4), INV, "metric"),
        ((f, f, 1, 2, 3, 4, 2, 4, 0, f, 4), INV, "x_row_stride"), ((f, f, 1, 2, 3, 4, 3, 3, 0, f, 4), INV, "y_row_stride"),
        ((f, f, 1, 2, 3, 4, 3, 4, 0, f, 3), INV, "c_row_stride"),
        ((f, f, 1, 2, cap_len + 1, 4, cap_len + 1, 4, 0, f, 4), UNS, "exceed"),
    ):
        assert eb.cost_raw(*args) == rc and word in eb.last_error(), (args, eb.last_error())
    for args, kw, rc, word in (
        ((None, 1, 3, 4, 4, DEFAULT, f, 4, u, 4), {}, INV, "NULL"), ((f, 1, 3, 4, 4, DEFAULT, None, 4, u, 4), {}, INV, "NULL"),
        ((f, 1, 3, 4, 4, DEFAULT, f, 4, None, 4), {}, INV, "NULL"), ((f, 1, 3, 4, 4, DEFAULT, f, 4, u, 4), dict(weights=False), INV, "weights"),
        ((f, 0, 3, 4, 4, DEFAULT, f, 4, u, 4), {}, INV, "non-empty"), ((f, 1, 3, 0, 4, DEFAULT, f, 4, u, 4), {}, INV, "non-empty"),
        ((f, 1, 3, 4, 3, DEFAULT, f, 4, u, 4), {}, INV, "c_row_stride"), ((f, 1, 3, 4, 4, DEFAULT, f, 3, u, 4), {}, INV, "d_row_stride"),
        ((f, 1, 3, 4, 4, DEFAULT, f, 4, u, 3), {}, INV, "steps_row_stride"),
        ((f, 1, 3, 4, 4, (), f, 4, u, 4), {}, INV, "n_steps"), ((f, 1, 3, 4, 4, ((1, 1),) * 9, f, 4, u, 4), {}, INV, "n_steps"),
        ((f, 1, 3, 4, 4, ((1, 1), (0, 0)), f, 4, u, 4), {}, INV, "not both 0"), ((f, 1, 3, 4, 4, ((1, -1),), f, 4, u, 4), {}, INV, ">= 0"),
        ((f, 1, 3, 4, 4, ((1, CAP + 1),), f, 4, u, 4), {}, UNS, "exceed"), ((f, 1, 3, 4, 4, ((CAP + 1, 0),), f, 4, u, 4), {}, UNS, "exceed"),
        ((f, 1, 3, 4, 4, DEFAULT, f, 4, u, 4), dict(band_r=-1), INV, "radius"),
        ((f, 1, cap_len + 1, 4, 4, DEFAULT, f, 4, u, 4), {}, UNS, "exceed"),
    ):
        assert eb.accumulate_raw(*args, **kw) == rc and word in eb.last_error(), (args, eb.last_error())
    for args, rc, word in (
        ((None, None, 1, 3, 4, 4, 4, DEFAULT, 0, i, i), INV, "NULL"), ((None, u, 1, 3, 4, 4, 4, DEFAULT, 0, None, i), INV, "NULL"),
        ((None, u, 1, 3, 4, 4, 4, DEFAULT, 0, i, None), INV, "NULL"), ((None, u, 1, 3, 4, 4, 4, DEFAULT, 1, i, i), INV, "subseq needs"),
        ((None, u, 1, 0, 4, 4, 4, DEFAULT, 0, i, i), INV, "non-empty"), ((None, u, 1, 3, 4, 4, 3, DEFAULT, 0, i, i), INV, "steps_row_stride"),
        ((f, u, 1, 3, 4, 3, 4, DEFAULT, 1, i, i), INV, "d_row_stride"), ((None, u, 1, 3, 4, 4, 4, ((0, 0),), 0, i, i), INV, "not both 0"),
        ((None, u, 1, 3, 4, 4, 4, ((0, CAP + 1),), 0, i, i), UNS, "exceed"), ((None, u, 1, 3, cap_len + 1, 4, cap_len + 1, DEFAULT, 0, i, i), UNS, "exceed"),
    ):
        assert eb.backtrack_raw(*args) == rc and word in eb.last_error(), (args, eb.last_error())
