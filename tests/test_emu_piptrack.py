"""CPU: the piptrack kernels (csrc/kernels_piptrack.h) on the SIMT emulator, through the C entries' twins, against the
NumPy model of tests/piptrack_ref.py: every comparison is assert_array_equal on the float32 bits or on integer counts.
Every buffer lies between NaN bands and every row has NaN pad columns behind it (tests/emu/emu_piptrack_bind.py)."""

import os
import sys

import numpy as np
import pytest

import piptrack_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_piptrack_bind as eb  # noqa: E402

CONSTS = eb.constants()
TILE = CONSTS["tile"]
SR = 22050


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def spectrum_case(B, F, T, cplx, seed):
    """A peaky random spectrum: magnitudes (B, F, T) float32, or complex64 values whose |z| has no double-rounding tie."""
    rng = np.random.default_rng(1000 + seed)
    mag = rng.gamma(0.5, 1.0, (B, F, T)) * (1.0 + 4.0 * (rng.uniform(size=(B, F, T)) < 0.1))
    if not cplx:
        return mag.astype(np.float32)
    ph = rng.uniform(0, 2 * np.pi, (B, F, T))
    return (mag * np.exp(1j * ph)).astype(np.complex64)


def model_input(x):
    """The float32 magnitudes the model works on; for complex input the fixture must be free of double-rounding ties."""
    if np.iscomplexobj(x):
        S, wrong = R.magnitude(x)
        assert not wrong.any(), "the fixture holds a double-rounding tie of im im + fl(re re)"
        return S
    return x


# (F, T, B, complex, threshold, ref: None / "scalar" / "tensor", k range: "freq" or (k_lo, k_hi) with -1 = F and -2 = F - 1,
#  pad_in, pad_out, grid)
DENSE_CASES = (
    (2, 1, 1, False, 0.1, None, "freq0", 0, 0, 0),
    (2, 65, 3, True, 0.0, None, (0, -1), 1, 2, 0),
    (3, 63, 1, False, 0.5, None, (1, -1), 0, 0, 0),
    (3, 130, 3, True, 0.1, "scalar", (0, -2), 2, 0, 1),
    (9, 64, 1, True, 0.0, "tensor", (1, -2), 0, 3, 0),
    (9, 1, 3, False, 0.5, None, (-1, -1), 3, 1, 0),
    (33, 65, 3, False, 0.1, None, "freq", 1, 1, 0),
    (33, 130, 1, True, 0.5, "tensor", (-2, -1), 0, 0, 1),
    (257, 63, 1, True, 0.1, None, "freq", 5, 0, 0),
    (257, 130, 3, False, 0.0, "scalar", (0, -1), 0, 2, 1),
    (257, 64, 3, True, 0.5, None, (0, 1), 2, 2, 0),
    (33, TILE + 1, 1, False, 0.1, None, (0, 0), 0, 0, 0),
    (1025, 70, 1, True, 0.1, None, "freq", 2, 0, 0),
)
DENSE_IDS = ["F%d-T%d-B%d-%s-thr%s-ref%s-k%s-grid%d" % (c[0], c[1], c[2], "cplx" if c[3] else "real", c[4], c[5], c[6], c[9])
             for c in DENSE_CASES]


def dense_case(case):
    """(x, model magnitudes, k_lo, k_hi, bin_hz, ref, keyword arguments of the model)."""
    F, T, B, cplx, thr, ref_kind, kr, pad_in, pad_out, grid = case
    i = DENSE_CASES.index(case)
    x = spectrum_case(B, F, T, cplx, i)
    S = model_input(x)
    n_fft = 2 * (F - 1)
    if kr == "freq":
        k_lo, k_hi = R.bin_range(SR, n_fft, 150.0, 4000.0, F)
    elif kr == "freq0":
        k_lo, k_hi = R.bin_range(SR, n_fft, 0.0, 1e9, F)
    else:
        k_lo, k_hi = [F + 1 + v if v < 0 else v for v in kr]
    rng = np.random.default_rng(i)
    ref = None if ref_kind is None else np.float32(-0.7) if ref_kind == "scalar" else \
        (rng.uniform(0.1, 2.0, (B, T)) * rng.choice([-1.0, 1.0], (B, T))).astype(np.float32)      # |ref| is what counts
    return x, S, k_lo, k_hi, np.float32(SR / n_fft), ref, dict(threshold=thr, ref=ref, k_range=(k_lo, k_hi), sr=SR)


def test_the_sweep_covers_what_it_claims():
    col = lambda i: {c[i] for c in DENSE_CASES}                 # noqa: E731
    assert {2, 3, 9, 33, 257, 1025} == col(0) and {1, 63, 64, 65, 130} <= col(1) and {TILE - 1, TILE, TILE + 1} <= col(1)
    assert col(2) == {1, 3} and col(3) == {False, True} and {0.0, 0.5} <= col(4) and col(5) == {None, "scalar", "tensor"}
    assert any(c[7] for c in DENSE_CASES) and any(c[8] for c in DENSE_CASES) and 1 in col(9)
    ks = [c[6] for c in DENSE_CASES if isinstance(c[6], tuple)]
    assert {0, 1, -2, -1} <= {k[0] for k in ks} and {0, 1, -2, -1} <= {k[1] for k in ks}
    assert (1025, 70) in {(c[0], c[1]) for c in DENSE_CASES}


@pytest.mark.parametrize("case", DENSE_CASES, ids=DENSE_IDS)
def test_emu_dense_sweep(case):
    x, S, k_lo, k_hi, bin_hz, ref, kw = dense_case(case)
    want_p, want_m = R.piptrack(S, **kw)
    got_p, got_m = eb.dense(x, k_lo, k_hi, bin_hz, threshold=kw["threshold"], ref=ref, pad_in=case[7], pad_out=case[8], grid=case[9])
    np.testing.assert_array_equal(bits(got_p), bits(want_p))
    np.testing.assert_array_equal(bits(got_m), bits(want_m))
    assert not want_p[:, 0].any() and not (want_p[:, :k_lo].any() or want_p[:, k_hi:].any())


def test_emu_hand_made_columns():
    """A plateau (its first bin only), a peak at F - 1 (shift 0), a zero frame, den = 0 (a step: avg / 1)."""
    cols = np.array([[0, 1, 3, 3, 3, 1, 0, 0],        # plateau at 2 .. 4
                     [0, 1, 0, 0, 0, 1, 2, 4],        # peaks at 1 and at F - 1
                     [0, 0, 0, 0, 0, 0, 0, 0],
                     [1, 2, 3, 4, 5, 6, 7, 7]], np.float32).T[None]      # den = 0 on the ramp; 6 and 7: a plateau at the top
    want_p, want_m = R.piptrack(cols, k_range=(0, 8), threshold=0.0, sr=14)
    got_p, got_m = eb.dense(cols, 0, 8, np.float32(1.0), threshold=0.0)
    np.testing.assert_array_equal(bits(got_p), bits(want_p))
    np.testing.assert_array_equal(bits(got_m), bits(want_m))
    assert list(np.nonzero(got_p[0, :, 0])[0]) == [2] and list(np.nonzero(got_p[0, :, 1])[0]) == [1, 7]
    assert got_p[0, 7, 1] == 7.0 and got_m[0, 7, 1] == 4.0 and not got_p[0, :, 2].any()
    assert list(np.nonzero(got_p[0, :, 3])[0]) == [6] and got_p[0, 2, 0] == 2.5


def edge_columns():
    """(S (1, F, T), calls) for the comparisons that only equal or subnormal values tell apart; each call is
    (keyword arguments of the model, ref as the C entry takes it, threshold).  Frame 0: a value equal to the threshold is
    not above it (ref = 2, and threshold 1 times the maximum: no peak at all).  Frame 1: subnormal magnitudes, where
    |den| < FLT_MIN divides by 1 (shift = avg, not 1 / 6)."""
    S = np.array([[0, 1, 2, 1, 0, 0], [0, 2e-40, 1e-40, 0, 0, 0]], np.float32).T[None]
    return S, (dict(ref=np.float32(2.0)), dict(threshold=1.0), dict(threshold=0.0))


def test_emu_equal_to_the_threshold_and_subnormal_den():
    S, calls = edge_columns()
    assert S[0, 1, 1] > 0 and S[0, 1, 1] < np.finfo(np.float32).tiny
    for kw in calls:
        want_p, want_m = R.piptrack(S, k_range=(0, 6), sr=10, **kw)
        got_p, got_m = eb.dense(S, 0, 6, np.float32(1.0), threshold=kw.get("threshold", 0.1), ref=kw.get("ref"))
        np.testing.assert_array_equal(bits(got_p), bits(want_p))
        np.testing.assert_array_equal(bits(got_m), bits(want_m))
        if kw.get("threshold") == 0.0:
            assert want_p[0, 1, 1] == 1.0 and want_p[0, 2, 0] == 2.0, "shift = avg / 1 on the subnormal frame"
        else:
            assert not want_p[0, :, 0].any(), "a bin equal to the threshold is not above it"


def low_frequencies():
    """Frequencies on both sides of 27.5 Hz (negative octave numbers, where fmod leaves a negative residual), zeros,
    negatives, a NaN and an infinity, none of the residuals within 1e-9 of an edge."""
    f = (27.5 * 2.0 ** np.random.default_rng(21).uniform(-4.0, 4.0, 3000)).astype(np.float32)
    f[::97] = 0.0
    f[5::101] = -f[5::101]
    f[7], f[8] = np.nan, np.inf
    return f


def test_emu_histogram_below_27_5_hz_and_of_junk():
    f = low_frequencies()
    ok = f[np.isfinite(f)]
    assert (ok[ok > 0] < 27.5).sum() > 1000
    for res, bpo in ((0.01, 12), (0.3, 36)):
        assert R.nearest_edge_distance(ok, res, bpo) > 1e-9
        np.testing.assert_array_equal(eb.pitch_hist(f, R.edges(res), bpo), R.counts(ok, res, bpo))
    rec = np.stack([np.ones_like(ok), ok], axis=1)[None]
    thr, counts = eb.tuning(rec, np.array([len(ok)], np.uint64), R.edges(0.01))
    np.testing.assert_array_equal(counts[0], R.counts(ok))


def test_emu_a_nan_stays_in_its_frame():
    x = spectrum_case(1, 33, 70, False, 77)
    want_p, want_m = R.piptrack(x, k_range=(0, 33))
    x[0, 5, 9] = np.nan
    x[0, 7, 66] = np.inf
    B, F, T = x.shape
    raw_p = np.full((B, F, T), np.nan, np.float32)
    raw_m = np.full((B, F, T), np.nan, np.float32)
    xs = np.ascontiguousarray(x)
    eb._check(eb.lib().emu_piptrack_f32(xs.ctypes.data, 0, B, F, T, T, 0, F, 0.1, 0, 0.0, None, float(np.float32(SR / 64)),
                                        raw_p.ctypes.data, raw_m.ctypes.data, T, 0))
    keep = np.ones(T, bool)
    keep[[9, 66]] = False
    np.testing.assert_array_equal(bits(raw_p[..., keep]), bits(want_p[..., keep]))
    np.testing.assert_array_equal(bits(raw_m[..., keep]), bits(want_m[..., keep]))


# ---------------------------------------------------------------------------------------------------------------------
# compact mode, the selection and the histogram
# ---------------------------------------------------------------------------------------------------------------------
_tonal = {}


def tonal(B=3, n_fft=512, frames=173, seed=5):
    """(complex spectrum, model magnitudes, model pitches, model magnitudes at the peaks, k_lo, k_hi, bin_hz), computed once."""
    key = (B, n_fft, frames, seed)
    if key not in _tonal:
        y = R.tones(B, frames * (n_fft // 4), seed, detune=0.2)
        X = R.spectrum(y, n_fft, n_fft // 4)
        S = model_input(X)
        k_lo, k_hi = R.bin_range(SR, n_fft, 150.0, 4000.0, S.shape[1])
        p, m = R.piptrack(S, sr=SR)
        for a in (X, S, p, m):
            a.setflags(write=False)
        _tonal[key] = (X, S, p, m, k_lo, k_hi, np.float32(SR / n_fft))
    return _tonal[key]


def as_words(pairs):
    return np.sort(np.ascontiguousarray(pairs, np.float32).view(np.uint64).ravel())


def dense_pairs(p, m):
    sel = p > 0
    return np.stack([m[sel], p[sel]], axis=1)


@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
def test_emu_records_are_the_dense_peaks(per_clip, cplx):
    X, S, p, m, k_lo, k_hi, bin_hz = tonal()
    cnt, rec = eb.records(X if cplx else S, k_lo, k_hi, bin_hz, 4096, per_clip=per_clip, pad_in=3, grid=0 if cplx else 2)
    groups = [(p[b], m[b]) for b in range(3)] if per_clip else [(p, m)]
    for g, (pg, mg) in enumerate(groups):
        want = dense_pairs(pg, mg)
        assert int(cnt[g]) == len(want) > 100
        np.testing.assert_array_equal(as_words(rec[g, :len(want)]), as_words(want))
        assert np.isnan(rec[g, len(want):]).all()


@pytest.mark.parametrize("resolution,bpo", [(0.01, 12), (0.3, 12), (0.01, 36), (0.3, 36)])
def test_emu_tuning_global_and_per_clip(resolution, bpo):
    X, S, p, m, k_lo, k_hi, bin_hz = tonal()
    assert R.nearest_edge_distance(p, resolution, bpo) > 1e-9, "a residual of the fixture lies on an edge"
    e = R.edges(resolution)
    for per_clip in (False, True):
        cnt, rec = eb.records(X, k_lo, k_hi, bin_hz, 4096, per_clip=per_clip)
        thr, counts = eb.tuning(rec, cnt, e, bpo)
        groups = [(p[b], m[b]) for b in range(3)] if per_clip else [(p, m)]
        for g, (pg, mg) in enumerate(groups):
            n, wthr, wc = R.tuning_parts(pg, mg, resolution, bpo)
            assert int(cnt[g]) == n
            np.testing.assert_array_equal(bits(thr[g]), bits(wthr))
            np.testing.assert_array_equal(counts[g], wc)
            assert counts[g].sum() >= n // 2
    np.testing.assert_array_equal(eb.pitch_hist(p, e, bpo), R.counts(p, resolution, bpo))
    np.testing.assert_array_equal(eb.pitch_hist(p, e, bpo, grid=1), R.counts(p, resolution, bpo))


def test_emu_too_small_a_capacity_counts_on_and_the_rerun_agrees():
    X, S, p, m, k_lo, k_hi, bin_hz = tonal()
    want = dense_pairs(p, m)
    cnt, rec = eb.records(X, k_lo, k_hi, bin_hz, 100)
    assert int(cnt[0]) == len(want) > 100 and not np.isnan(rec).any()
    e = R.edges(0.01)
    thr, counts = eb.tuning(rec, cnt, e)
    assert np.isnan(thr[0]), "a group whose records did not fit must be left alone"
    cnt2, rec2 = eb.records(X, k_lo, k_hi, bin_hz, int(cnt[0]))
    thr, counts = eb.tuning(rec2, cnt2, e)
    n, wthr, wc = R.tuning_parts(p, m)
    np.testing.assert_array_equal(bits(thr[0]), bits(wthr))
    np.testing.assert_array_equal(counts[0], wc)


_dense = {}


def dense_fixture(cplx):
    """(input, model magnitudes, model pitches, model peak magnitudes, peaks per wave and tile) of the peak-dense case:
    B = 2, F = 513, T = 130, every bin in range, to be run with threshold 0.  Asserts that every wave of every full tile
    stages more than three times what its LDS stage holds, so that it flushes several times inside the tile."""
    if cplx not in _dense:
        S = R.dense_peaks(2, 513, 130, 11)
        x = S
        if cplx:
            ph = np.random.default_rng(12).uniform(0, 2 * np.pi, S.shape)
            x = (S * np.exp(1j * ph)).astype(np.complex64)
            S = model_input(x)
        p, m = R.piptrack(S, k_range=(0, 513), threshold=0.0, sr=1024)      # sr / n_fft = 1
        nk = -(-513 // CONSTS["waves"])
        per = np.array([[(p[b, q * nk:(q + 1) * nk, t0:t0 + TILE] > 0).sum() for q in range(CONSTS["waves"])]
                        for b in range(2) for t0 in (0, TILE)])
        assert per.min() > 3 * CONSTS["stage"], per.min()
        for a in (x, S, p, m):
            a.setflags(write=False)
        _dense[cplx] = (x, S, p, m, per)
    return _dense[cplx]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("per_clip", [False, True])
def test_emu_peak_dense_records_flush_mid_tile(per_clip, cplx):
    """A third of the bins are peaks: the waves hand their LDS stage over several times inside a tile and use it again.
    The records equal the dense peaks as a multiset with a capacity above the count; with one below it the counter counts
    on and every slot holds a different peak."""
    x, S, p, m, _ = dense_fixture(cplx)
    groups = [(p[b], m[b]) for b in range(2)] if per_clip else [(p, m)]
    want = [dense_pairs(pg, mg) for pg, mg in groups]
    big = max(len(w) for w in want) + 7
    for capacity, grid in ((big, 0), (1000, 3)):
        cnt, rec = eb.records(x, 0, 513, np.float32(1.0), capacity, threshold=0.0, per_clip=per_clip, pad_in=1, grid=grid)
        for g, w in enumerate(want):
            assert int(cnt[g]) == len(w) > 1000
            if capacity == big:
                np.testing.assert_array_equal(as_words(rec[g, :len(w)]), as_words(w))
                assert np.isnan(rec[g, len(w):]).all()
            else:
                got = as_words(rec[g])
                assert len(np.unique(got)) == capacity and np.isin(got, as_words(w)).all()


MEDIAN_NS = [0, 1, 2, 3, 4, 1000, 1001, 2500]


@pytest.mark.parametrize("n", MEDIAN_NS)
def test_emu_median_of_hand_made_records(n):
    """Odd and even n, n in {0, 1, 2}, many equal magnitudes (the two middle ones equal, or the run of equal keys ending
    exactly at the lower one), more records than one pass of the workgroup."""
    rng = np.random.default_rng(n)
    for flavour in ("random", "equal", "two-valued"):
        mags = {"random": rng.gamma(1.0, 3.0, n), "equal": np.full(n, 2.5),
                "two-valued": np.where(np.arange(n) < n // 2, 1.25, 7.0)}[flavour].astype(np.float32)
        rng.shuffle(mags)
        pit = (440.0 * 2.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
        rec = np.full((1, max(n, 1) + 5, 2), np.nan, np.float32)
        rec[0, :n, 0], rec[0, :n, 1] = mags, pit
        thr, counts = eb.tuning(rec, np.array([n], np.uint64), R.edges(0.01))
        want = R.median(mags)
        np.testing.assert_array_equal(bits(thr[0]), bits(want))
        assert R.nearest_edge_distance(pit) > 1e-9
        np.testing.assert_array_equal(counts[0], R.counts(pit[mags >= want]))


def test_emu_prepare_rejects_by_name():
    x = np.ones((1, 4, 4), np.float32)
    o = np.zeros((1, 4, 4), np.float32)
    ok = [x.ctypes.data, 0, 1, 4, 4, 4, 0, 4, 0.1, 0, 0.0, None, 1.0, o.ctypes.data, o.ctypes.data, 4, 0]

    def bad(i, v, word):
        a = list(ok)
        a[i] = v
        assert eb.raw_dense(a) != 0 and word in eb.lib().emu_piptrack_last_error().decode(), (i, v)

    assert eb.raw_dense(ok) == 0
    bad(0, None, "NULL"); bad(3, 1, "2 frequency bins"); bad(5, 3, "in_row_stride"); bad(15, 3, "out_row_stride")
    bad(6, 5, "k_lo"); bad(7, 5, "k_hi"); bad(8, -1.0, "threshold"); bad(9, 3, "ref_mode"); bad(9, 2, "ref"); bad(1, 2, "in_kind")
    bad(2, 0, "non-empty")
    with pytest.raises(eb.Status, match="cap"):
        eb.pitch_hist(np.ones(4, np.float32), np.linspace(-0.5, 0.5, CONSTS["max_bins"] + 2))
