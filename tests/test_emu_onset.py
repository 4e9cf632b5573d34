"""CPU: the onset kernel source (kernels_onset.h) on the SIMT emulator of tests/emu against the float64 definitions in
tests/onset_ref.py.

Every buffer lies between NaN bands and, in the padded-row variants, has NaN pad columns: emu_onset_bind asserts that
none of them was written and that no NaN comes out (a read of one would surface as a NaN in the envelope).

onset strength.  Given the float32 (dB) input, every term max(0, S - R) is non-negative, so
|env32 - env64| <= (M + 2) 2^-24 env64 for any summation order (onset_ref.strength_bound): one rounding for a
difference, M - 1 for the sum, one for the division; the running maximum is exact.  In dB mode the reference takes the
kernel's own float32 dB values, computed by the same ap_db_* helpers through the binding.  Worst error over bound seen
on the emulator and on an MI355X alike: 0.33 (printed per case with -s).

peak picking.  The mask must equal the reference's exactly.  Precondition, asserted per row and case: the float64
reference is decisive (onset_ref.decisive: no frame that passes the max test has x[n] - (mean + delta) within 1e-4 of
zero, except where the comparison is exact in both precisions by construction - a window of equal values whose float32
sum is exact, which is what a plateau, a constant row and the one-frame window (0, 1, 0, 1) are there to test).  The
rows are drawn by seed and re-drawn in the generator (onset_ref.peak_rows) until that holds; no case is skipped.
"""

import os
import sys

import numpy as np
import pytest

import hpss_ref
import onset_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_onset_bind as eb  # noqa: E402

from onset_ref import (DELTAS, PEAK_T, PEAK_WINDOWS, SHAPES, SHIFT_KINDS, lags, max_sizes, rows_for, spectrum,  # noqa: E402
                       strength_check as check)

IDS = ["x".join(map(str, s)) for s in SHAPES]


def test_reference_self_check():
    """The explicit maximum filter == scipy.ndimage.maximum_filter1d for M in 1 .. 40 and every window size of this file
    wherever SciPy implements the reflection (hpss_ref.scipy_reflects); the even windows cover [m - 2, m + 1] and
    [m - 1, m]; the reference peak_pick against hand-worked rows."""
    from scipy.ndimage import maximum_filter1d

    rng = np.random.default_rng(7)
    n_scipy = 0
    for M in range(1, 41):
        S = rng.standard_normal((2, M, 3))
        for size in (1, 2, 3, 4, 5, 8, 31):
            if hpss_ref.scipy_reflects(size, M):
                n_scipy += 1
                assert np.array_equal(R.max_filter(S, size), maximum_filter1d(S, size, axis=-2, mode="reflect")), (M, size)
    assert n_scipy >= 270
    col = np.array([5.0, 1.0, 2.0, 9.0, 3.0, 4.0])[:, None]
    assert list(R.max_filter(col, 4)[:, 0]) == [5.0, 5.0, 9.0, 9.0, 9.0, 9.0]            # [m - 2, m + 1]
    assert list(R.max_filter(col, 2)[:, 0]) == [5.0, 5.0, 2.0, 9.0, 9.0, 4.0]            # [m - 1, m]
    assert list(R.max_filter(col, 3)[:, 0]) == [5.0, 5.0, 9.0, 9.0, 9.0, 4.0]
    # flux by hand: M = 2, lag = 1
    S = np.array([[0.0, 2.0, 1.0, 4.0], [1.0, 0.0, 3.0, 3.0]])
    assert list(R.onset_strength(S, lag=1)) == [0.0, 1.0, 1.5, 1.5]
    assert list(R.onset_strength(S, lag=1, shift=3)) == [0.0, 0.0, 0.0, 1.0]
    assert list(R.onset_strength(S, lag=2)) == [0.0, 0.0, 1.5, 2.5]
    assert list(R.onset_strength(S, lag=4)) == [0.0] * 4 and list(R.onset_strength(S, lag=9)) == [0.0] * 4
    assert R.shift_of(1) == 3 and R.shift_of(2, False) == 2 and R.shift_of(1, True, 512, 128) == 3
    # peak_pick by hand
    x = np.array([0.0, 1.0, 0.0, 2.0, 2.0, 0.0, 3.0, 0.0])
    assert list(np.flatnonzero(R.peak_pick(x, 1, 2, 1, 2, 0.0, 0))) == [1, 3, 4, 6]       # the plateau: both frames
    assert list(np.flatnonzero(R.peak_pick(x, 1, 2, 1, 2, 0.0, 1))) == [1, 3, 6]          # 4 is not wait + 1 after 3
    assert list(np.flatnonzero(R.peak_pick(x, 1, 2, 1, 2, 0.0, 2))) == [1, 4]             # 3 is not, 4 is; then 6 is not
    assert list(np.flatnonzero(R.peak_pick(x, 1, 2, 1, 2, 1.0, 0))) == [6]                # 2 < 4/3 + 1 on the plateau, 3 >= 1 + 1
    assert list(np.flatnonzero(R.peak_pick(x, 0, 1, 0, 1, 0.0, 0))) == list(range(8))     # x[n] >= x[n]
    assert list(np.flatnonzero(R.peak_pick(x, 0, 1, 0, 1, 0.0, 8))) == [0]
    assert R.local_minima([3.0, 1.0, 1.0, 2.0, 0.0, 5.0, 5.0]) == [0, 2, 4]               # <= on the left, < on the right
    assert list(np.flatnonzero(R.backtrack(np.array([0, 1, 0, 1, 0, 1, 1], bool), [3.0, 1.0, 1.0, 2.0, 0.0, 5.0, 5.0]))) == [0, 2, 4]
    assert R.local_minima([1.0]) == [0] and R.local_minima([2.0, 1.0]) == [0]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emu_onset_strength(shape):
    """Every lag x max_size of the shape, the four shifts in turn, dense and padded rows, one workgroup walking all tiles."""
    S = spectrum(shape)
    B, M, T = shape
    worst, k = 0.0, 0
    for lag in lags(T):
        for ms in max_sizes(M):
            for center, n_fft, hop in (SHIFT_KINDS if (lag, ms) in ((1, 1), (2, 3)) else [SHIFT_KINDS[k % 4]]):
                shift = R.shift_of(lag, center, n_fft, hop)
                want = R.onset_strength(S, lag, ms, shift=shift)
                pads = ((0, 0), (3, 5))[k % 2]
                got = eb.onset_strength(S, lag=lag, max_size=ms, shift=shift, pad_in=pads[0], pad_out=pads[1], grid=(k % 3 == 0))
                assert eb.geometry()["staged"] == (ms > 1)
                worst = max(worst, check(got, want, M, (lag, ms, shift)))
                if lag >= T:
                    assert not got.any()
                assert not got[:, :min(shift, T)].any()
                k += 1
    assert eb.lds_overruns() == 0
    print(f"onset strength {shape}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emu_onset_strength_ref_route(shape):
    """ref= replaces the running maximum whatever max_size says."""
    S = spectrum(shape)
    B, M, T = shape
    ref = (S + np.random.default_rng(3).standard_normal(shape).astype(np.float32) * 10).astype(np.float32)
    worst = 0.0
    for lag in lags(T):
        for ms in (1, 5):
            want = R.onset_strength(S, lag, ms, ref=ref, shift=lag + 2)
            got = eb.onset_strength(S, lag=lag, max_size=ms, shift=lag + 2, ref=ref, pad_in=1, pad_ref=4, pad_out=2)
            assert eb.geometry()["staged"] == 0
            worst = max(worst, check(got, want, M, (lag, ms)))
    print(f"onset strength ref route {shape}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emu_onset_strength_db_mode(shape):
    """Power in, dB on load: the key makes a good part of the array clip at max - 80 dB.  The reference runs on the
    kernel's own float32 dB values (emu_onset_bind.db_values, the same helpers)."""
    B, M, T = shape
    rng = np.random.default_rng(11 + sum(shape))
    P = (10.0 ** rng.uniform(-14.0, 2.0, shape)).astype(np.float32)
    P[rng.random(shape) < 0.1] = 0.0
    db = dict(smax=float(P.max()), top_db=80.0)
    D = eb.db_values(P, db)
    floor = D.min()
    assert np.isfinite(D).all() and (P.size < 60 or 0.2 < np.mean(D == floor) < 0.8)
    np.testing.assert_allclose(D, np.maximum(10 * np.log10(np.maximum(P.astype(np.float64), 1e-10)),
                                             10 * np.log10(float(P.max())) - 80.0), atol=1e-4)
    worst = 0.0
    for lag in lags(T):
        for ms in (1, 2, 3, min(2 * M + 1, 255)):
            want = R.onset_strength(D, lag, ms, shift=lag + 1)
            got = eb.onset_strength(P, lag=lag, max_size=ms, shift=lag + 1, db=db, pad_in=2, pad_out=1)
            worst = max(worst, check(got, want, M, (lag, ms)))
            same = eb.onset_strength(D, lag=lag, max_size=ms, shift=lag + 1)
            assert np.array_equal(got, same), "dB on load and dB beforehand differ"
    got = eb.onset_strength(P, lag=1, db=dict(smax=float(P.max()), top_db=None))              # no clip
    want = R.onset_strength(eb.db_values(P, dict(smax=0.0, top_db=None)), 1)
    check(got, want, M, "no clip")
    print(f"onset strength dB mode {shape}: worst error / bound {worst:.3f}")


def test_emu_onset_strength_nan_guard_is_live():
    """What the NaN bands rely on: a NaN that is read, as either operand and on the staged path too, comes out as a NaN
    (the kernel's maximum and its rectification keep it), and the binding refuses it."""
    for m, t in ((0, 0), (4, 61), (2, 30)):
        S = spectrum((2, 5, 63)).copy()
        S[1, m, t] = np.nan
        for ms in (1, 2, 5):
            with pytest.raises(AssertionError, match="NaN"):
                eb.onset_strength(S, lag=1, max_size=ms, shift=1)
            with pytest.raises(AssertionError, match="NaN"):
                eb.onset_strength(spectrum((2, 5, 63)), lag=1, max_size=ms, shift=1, ref=S)


def test_emu_onset_strength_clip_alone_equals_clip_in_batch():
    for shape in [(2, 5, 63), (3, 4, 1), (3, 9, 130)]:
        S = spectrum(shape)
        for lag, ms in ((1, 1), (2, 4)):
            batch = eb.onset_strength(S, lag=lag, max_size=ms, shift=lag + 2)
            for b in range(shape[0]):
                assert np.array_equal(eb.onset_strength(S[b:b + 1], lag=lag, max_size=ms, shift=lag + 2)[0], batch[b])


def test_emu_onset_strength_rejects_before_launching():
    buf = np.zeros(4096, np.float32)
    s, o = buf.ctypes.data, buf.ctypes.data + 8192
    INVALID, UNSUPPORTED = -1, -2

    def rc(*a):
        return eb.strength_raw(*a), eb.last_error()

    #          S  B  M  T rs ref rsr lag ms shift db top key out rso
    assert rc(None, 1, 4, 8, 8, None, 0, 1, 1, 1, 0, -1.0, None, o, 8)[0] == INVALID
    assert rc(s, 1, 4, 8, 8, None, 0, 1, 1, 1, 0, -1.0, None, None, 8)[0] == INVALID
    for bad in ((0, 4, 8), (1, 0, 8), (1, 4, 0)):
        assert "non-empty" in rc(s, *bad, 8, None, 0, 1, 1, 1, 0, -1.0, None, o, 8)[1]
    assert "lag must be a positive integer" in rc(s, 1, 4, 8, 8, None, 0, 0, 1, 1, 0, -1.0, None, o, 8)[1]
    for ms in (0, 256, -1):
        assert "max_size must be an integer in 1 .. 255" in rc(s, 1, 4, 8, 8, None, 0, 1, ms, 1, 0, -1.0, None, o, 8)[1]
    assert "must be >= lag" in rc(s, 1, 4, 8, 8, None, 0, 2, 1, 1, 0, -1.0, None, o, 8)[1]
    assert "row strides" in rc(s, 1, 4, 8, 7, None, 0, 1, 1, 1, 0, -1.0, None, o, 8)[1]
    assert "row strides" in rc(s, 1, 4, 8, 8, None, 0, 1, 1, 1, 0, -1.0, None, o, 7)[1]
    assert "row strides" in rc(s, 1, 4, 8, 8, s, 7, 1, 1, 1, 0, -1.0, None, o, 8)[1]
    assert "top_db needs the key" in rc(s, 1, 4, 8, 8, None, 0, 1, 1, 1, 1, 80.0, None, o, 8)[1]
    assert "overlaps" in rc(s, 1, 4, 8, 8, None, 0, 1, 1, 1, 0, -1.0, None, s + 64, 8)[1]
    r, msg = rc(s, 1, (1 << 28) + 1, 8, 8, None, 0, 1, 1, 1, 0, -1.0, None, s + (1 << 50), 8)
    assert r == UNSUPPORTED and "2^28" in msg
    # the padding behind the last row is not part of an input: an output right behind the last value is no overlap
    assert rc(s, 1, 4, 6, 8, None, 0, 1, 1, 1, 0, -1.0, None, s + 4 * 30, 8)[0] == 0
    assert "overlaps" in rc(s, 1, 4, 6, 8, None, 0, 1, 1, 1, 0, -1.0, None, s + 4 * 29, 8)[1]
    r, msg = rc(s, 1 << 33, 4, 8, 8, None, 0, 1, 1, 1, 0, -1.0, None, s + (1 << 50), 8)
    assert r == UNSUPPORTED and "tiles" in msg


# ---- peak picking ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("windows", PEAK_WINDOWS, ids=["-".join(map(str, w)) for w in PEAK_WINDOWS])
@pytest.mark.parametrize("T", PEAK_T)
def test_emu_peak_pick(T, windows):
    """wait x delta x normalize x backtrack on random, spiky, plateau, constant, all-zero and NaN-bearing rows, all rows of
    a case in one launch.  normalize on is onset_detect (guard on: the NaN and the all-zero row yield nothing); normalize
    off is peak_pick (guard off: the NaN row is picked as NumPy's max and mean say)."""
    rows = rows_for(T, windows)
    names = list(rows)
    x = np.stack([rows[k] for k in names])
    energy = np.random.default_rng(T).random(x.shape).astype(np.float32)
    n_picked = 0
    for norm in (False, True):
        for delta in DELTAS:
            seen, cand = {}, {}
            for k in names:
                v = R.seen(rows[k], norm) if norm else rows[k].astype(np.float64)
                if v is not None:
                    assert R.decisive(v, windows, delta, on_grid=not norm), (k, norm, delta)     # the precondition
                    cand[k] = R.candidates(v, *windows, delta)[0]
                seen[k] = v
            for wait in sorted({0, 1, 10, T}):
                for bt in (False, True):
                    for en in ((None, energy) if bt and wait == 1 else (None,)):
                        got, count = eb.peak_pick(x, pre_max=windows[0], post_max=windows[1], pre_avg=windows[2],
                                                  post_avg=windows[3], delta=delta, wait=wait, normalize=norm, guard=norm,
                                                  backtrack=bt, energy=en, pad_in=(wait % 2) * 3, grid=1 + wait % 2)
                        for i, k in enumerate(names):
                            if seen[k] is None:
                                want = np.zeros(T, bool)
                            else:
                                want = R.greedy(cand[k], wait)
                                if bt:
                                    want = R.backtrack(want, seen[k] if en is None else en[i])
                            assert np.array_equal(got[i], want), (k, norm, delta, wait, bt, en is not None,
                                                                  np.flatnonzero(got[i]), np.flatnonzero(want))
                            n_picked += int(want.sum())
    assert n_picked > 0
    assert eb.lds_overruns() == 0


def test_emu_peak_pick_row_alone_equals_row_in_batch():
    rows = rows_for(130, (1, 1, 4, 5))
    x = np.stack(list(rows.values()))
    kw = dict(pre_max=1, post_max=1, pre_avg=4, post_avg=5, delta=0.07, wait=1, normalize=True, guard=True, backtrack=True)
    batch = eb.peak_pick(x, **kw)[0]
    for b in range(len(x)):
        assert np.array_equal(eb.peak_pick(x[b:b + 1], **kw)[0][0], batch[b])


def test_emu_peak_pick_rejects_before_launching():
    buf = np.zeros(4096, np.float32)
    s, m = buf.ctypes.data, buf.ctypes.data + 8192
    INVALID, UNSUPPORTED = -1, -2

    def rc(*a):
        return eb.peak_pick_raw(*a), eb.last_error()

    #          x  B  T rs  pre post pre post wait mask
    assert rc(None, 1, 8, 8, 1, 1, 1, 1, 0, m)[0] == INVALID and rc(s, 1, 8, 8, 1, 1, 1, 1, 0, None)[0] == INVALID
    assert "non-empty" in rc(s, 0, 8, 8, 1, 1, 1, 1, 0, m)[1] and "non-empty" in rc(s, 1, 0, 8, 1, 1, 1, 1, 0, m)[1]
    assert "non-negative" in rc(s, 1, 8, 8, -1, 1, 1, 1, 0, m)[1] and "non-negative" in rc(s, 1, 8, 8, 1, 1, -1, 1, 0, m)[1]
    assert "positive" in rc(s, 1, 8, 8, 1, 0, 1, 1, 0, m)[1] and "positive" in rc(s, 1, 8, 8, 1, 1, 1, 0, 0, m)[1]
    assert "wait must be" in rc(s, 1, 8, 8, 1, 1, 1, 1, -1, m)[1]
    assert "row strides" in rc(s, 1, 8, 7, 1, 1, 1, 1, 0, m)[1]
    assert "overlaps" in rc(s, 1, 8, 8, 1, 1, 1, 1, 0, s + 4)[1]
    assert rc(s, 2, 6, 8, 1, 1, 1, 1, 0, s + 4 * 14)[0] == 0 and "overlaps" in rc(s, 2, 6, 8, 1, 1, 1, 1, 0, s + 4 * 13)[1]
    limit = eb.max_frames()
    assert limit >= 16384
    r, msg = rc(s, 1, limit + 1, limit + 1, 1, 1, 1, 1, 0, s + (1 << 40))
    assert r == UNSUPPORTED and str(limit) in msg
