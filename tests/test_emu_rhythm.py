"""CPU: the rhythm kernel source (kernels_rhythm.h) on the SIMT emulator of tests/emu against the float64 definitions
in tests/rhythm_ref.py.  Every buffer lies between guard bands (emu_rhythm_bind asserts that none was written and that
no NaN comes out of a tempogram: a read of a band or a pad column would surface as one).

tempogram.  Per element |tg32 - tg64| <= atol = max(8 x the worst error of the float32 NumPy route (rfft / irfft at 1024
points) against float64 on the same case, 1e-6), on the max-normalised values; with norm=None the same relative to
ac[0, t] (rhythm_ref.tg_case).  The bound never comes from the kernel's own figures.  Worst error / atol seen on the
emulator / on an MI355X: 0.27 / 0.30 on the wave kernel, 0.13 / 0.13 on the general one (printed per case with -s).

tempo.  The picked lag must equal the reference's; precondition, asserted: the reference's best and second-best score
differ by more than 64 x 2^-24 x max|score|.

beat_track.  L within (2P + 4) 2^-24 sum|taps x o'| (+ float32's underflow for the taps below FLT_MIN, rhythm_ref.L_bound), C within the chain
bound of rhythm_ref.C_bound.  The mask must equal the reference's exactly; precondition, asserted per row: the float64
reference is decisive.  rhythm_ref.decisive_all (a margin at every argmax of the DP, every flank, the 1 % test, every
tail test, every trim threshold) wherever one of 9 draws meets it; rhythm_ref.decisive_chain (the decisions the mask
depends on, with its premise |C32 - C64| < thr / 2 asserted here) on the rows named in rhythm_ref.CHAIN_RULE_CASES, where
none does.  More than 8 redraws fail the test.
"""

import os
import sys

import numpy as np
import pytest

import rhythm_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_rhythm_bind as eb  # noqa: E402

INVALID, UNSUPPORTED = -1, -2


def test_reference_self_check():
    """The restated definitions against np.correlate, scipy.signal.convolve(..., "same"), np.convolve and np.pad on small
    rows, a row shorter than 2P + 1 included (there NumPy's and SciPy's "same" differ: the definition is length T)."""
    from scipy.signal import convolve

    rng = np.random.default_rng(5)
    for n, W, center in ((9, 4, True), (9, 5, True), (9, 5, False), (3, 8, True), (1, 1, True), (7, 7, False)):
        e = rng.random(n)
        w = 0.5 + rng.random(W)
        p = R.padded(e, W, center)
        h = W // 2
        if center:
            assert len(p) == n + 2 * h
            assert np.allclose(p[:h], e[0] * np.arange(h) / max(h, 1)) and np.allclose(p[h:h + n], e)
            assert np.allclose(p[h + n:], e[-1] * (h - 1 - np.arange(h)) / max(h, 1))
            assert h == 0 or p[0] == 0.0
        ac = R.tempogram(e, W, center, w, None)
        assert ac.shape == (W, R.n_frames(n, W, center))
        for t in range(ac.shape[1]):
            x = w * p[t:t + W]
            np.testing.assert_allclose(ac[:, t], np.correlate(x, x, "full")[W - 1:], rtol=1e-12, atol=1e-15)
        tg = R.tempogram(e, W, center, w, np.inf)
        assert np.allclose(np.max(np.abs(tg), axis=0), 1.0)
        np.testing.assert_allclose(R.tempogram_f32(e, W, center, w.astype(np.float32), np.inf), tg, atol=1e-5)
    assert not R.tempogram(np.zeros(6), 4).any()
    assert R.tempo_frequencies(4)[0] == np.inf and np.allclose(R.tempo_frequencies(4)[1:], 60 * 22050 / 512 / np.arange(1, 4))
    assert R.tempo_window() == 344
    assert [R.half(P) for P in (2, 3, 4, 5, 6, 7, 9, 200)] == [1, 2, 2, 2, 3, 4, 4, 100]
    for T, P in ((40, 3), (40, 8), (5, 8), (2, 2), (17, 8), (16, 8)):
        o = rng.random(T)
        on, L = R.local_score(o, P)
        assert len(L) == T
        np.testing.assert_allclose(L, np.convolve(on, R.taps(P), "full")[P:P + T], rtol=1e-12)
        if T >= 2 * P + 1:
            np.testing.assert_allclose(L, convolve(on, R.taps(P), "same"), rtol=1e-12)
    # a perfect click train: the beats are the clicks
    o = np.zeros(101)
    o[4::8] = 1.0
    o += 1e-3 * rng.random(101)
    st = R.beat_stages(o, 8, 100.0, trim=False)
    assert list(st["beats"]) == list(range(4, 101, 8))          # (the last click is the last frame: the tail)
    assert R.beat_stages(np.zeros(9), 8) is None and R.beat_stages(np.full(9, 0.5), 8) is None and R.beat_stages([1.0], 2) is None


# ---- tempogram ------------------------------------------------------------------------------------------------------
def _tg_variants(n, W):
    """(center, norm_inf, window kind, pad_in) of one (n, W): every centre / norm combination with hann, the array
    window on the default one; strided rows on every second variant."""
    out = [(True, True, "hann", 0), (True, False, "hann", 3), (True, True, "array", 5)]
    if n >= W:
        out += [(False, True, "hann", 2), (False, False, "array", 0)]
    return out


def _tile_sums_are_the_stored_values(got, agg, T, what):
    """The tile sums: the stored values of a tile added in frame order, in every bit."""
    for tile in range(agg.shape[1]):
        seq = np.zeros(got.shape[:2], np.float32)
        for t in range(64 * tile, min(64 * tile + 64, T)):
            seq = seq + got[:, :, t]
        assert np.array_equal(agg[:, tile], seq), (what, tile)


@pytest.mark.parametrize("shape", R.TG_SHAPES, ids=["x".join(map(str, s)) for s in R.TG_SHAPES])
def test_emu_tempogram(shape):
    """W <= 512 on the wave kernel and, forced, on the general one (each against the reference, and against each other
    within the same atol); 513 and 600 on the general kernel only (the wave route answers AP_ERR_UNSUPPORTED)."""
    worst = {"wave": 0.0, "general": 0.0}
    for k, W in enumerate(R.TG_WAVE_W + R.TG_GENERAL_W):
        for center, norm_inf, kind, pad_in in _tg_variants(shape[1], W):
            e, want, atol, window = R.tg_case(shape, W, center, norm_inf, kind)
            w = R.window_of(window, W).astype(np.float32)
            got = {}
            for route in (("wave", "general") if W in R.TG_WAVE_W else ("general",)):
                got[route], agg = eb.tempogram(e, w, center=center, norm=norm_inf, pad_in=pad_in, agg=True, grid=(k % 3 == 0),
                                               wave=route == "wave")
                assert got[route].shape == want.shape
                ratio = float(np.max(np.abs(got[route] - want) / atol))
                worst[route] = max(worst[route], ratio)
                assert ratio <= 1.0, (route, shape, W, center, norm_inf, kind, ratio)
                _tile_sums_are_the_stored_values(got[route], agg, want.shape[-1], (route, shape, W))
                only_agg = eb.tempogram(e, w, center=center, norm=norm_inf, out=False, agg=True, wave=route == "wave")[1]
                assert np.array_equal(only_agg, agg)
            if "wave" in got:
                assert float(np.max(np.abs(got["wave"] - got["general"]) / atol)) <= 1.0, (shape, W, center, norm_inf, kind)
            else:
                with pytest.raises(eb.Status) as err:
                    eb.tempogram(e, w, center=center, norm=norm_inf, wave=True)
                assert err.value.rc == UNSUPPORTED
    assert eb.lds_overruns() == 0
    print(f"tempogram {shape}: worst error / atol, wave {worst['wave']:.3f}, general {worst['general']:.3f}")


def test_emu_tempogram_clip_alone_equals_clip_in_batch():
    for shape, W in (((3, 130), 64), ((3, 130), 384), ((2, 5), 3)):
        e = R.tg_envelope(shape)
        w = R.window_of("hann", W).astype(np.float32)
        for wave in (True, False):
            batch, bagg = eb.tempogram(e, w, agg=True, wave=wave)
            for b in range(shape[0]):
                one, oagg = eb.tempogram(e[b:b + 1], w, agg=True, pad_in=1, wave=wave, grid=1 + b)
                assert np.array_equal(one[0], batch[b]) and np.array_equal(oagg[0], bagg[b])


def test_emu_tempogram_zero_row_gives_zeros():
    e = R.tg_envelope((3, 70)).copy()
    e[1] = 0.0
    for norm in (True, False):
        for wave in (True, False):
            got, agg = eb.tempogram(e, R.window_of("hann", 16).astype(np.float32), norm=norm, agg=True, wave=wave)
            assert not got[1].any() and not agg[1].any() and got[0].any()


def test_emu_tempogram_rejects_before_launching():
    buf = np.zeros(4096, np.float32)
    s, w, o = buf.ctypes.data, buf.ctypes.data + 4096, buf.ctypes.data + 8192

    def rc(*a):
        return eb.tempogram_raw(*a), eb.last_error()

    #          e  B  n rs  w  W  c out agg
    assert rc(None, 1, 8, 8, w, 4, 1, o, None)[0] == INVALID and rc(s, 1, 8, 8, None, 4, 1, o, None)[0] == INVALID
    assert rc(s, 1, 8, 8, w, 4, 1, None, None)[0] == INVALID
    assert "non-empty" in rc(s, 0, 8, 8, w, 4, 1, o, None)[1] and "non-empty" in rc(s, 1, 0, 8, w, 4, 1, o, None)[1]
    assert "win_length must be a positive integer" in rc(s, 1, 8, 8, w, 0, 1, o, None)[1]
    r, msg = rc(s, 1, 8, 8, w, eb.max_win() + 1, 1, o, None)
    assert r == UNSUPPORTED and str(eb.max_win()) in msg and eb.max_win() >= 8192
    assert "row stride" in rc(s, 2, 8, 7, w, 4, 1, o, None)[1]
    assert "shorter than win_length" in rc(s, 1, 8, 8, w, 9, 0, o, None)[1] and rc(s, 1, 8, 8, w, 8, 0, o, None)[0] == 0
    assert "overlaps" in rc(s, 1, 8, 8, w, 4, 1, s + 16, None)[1] and "overlaps" in rc(s, 1, 8, 8, w, 4, 1, None, s + 16)[1]


# ---- tempo ------------------------------------------------------------------------------------------------------------
class _LogNormal:
    """A prior object: logpdf over bpm, as a frozen scipy.stats distribution has."""

    def logpdf(self, bpm):
        with np.errstate(divide="ignore", invalid="ignore"):
            return -0.5 * ((np.log(bpm) - np.log(100.0)) / 0.4) ** 2 - np.log(bpm)


def _emu_tempo(e, lp, per_frame=False, stored=False, wave=True):
    """The picks of the emulated kernels from an envelope (1, n): the tile-sum route, or a stored tempogram."""
    W = len(lp)
    w = R.window_of("hann", W).astype(np.float32)
    tg, agg = eb.tempogram(e, w, agg=True, wave=wave)
    T = tg.shape[-1]
    if per_frame:
        return eb.tempo_pick(tg, lp, n_col=T, sb=W * T, sk=T, sc=1, n_red=1, sr=0, div=1.0, grid=3)
    if stored:
        return eb.tempo_pick(tg, lp, n_col=1, sb=W * T, sk=T, sc=0, n_red=T, sr=1, div=float(T))
    nt = agg.shape[1]
    return eb.tempo_pick(agg, lp, n_col=1, sb=nt * W, sk=1, sc=0, n_red=nt, sr=W, div=float(T))


@pytest.mark.parametrize("period,n", R.TEMPO_CASES)
def test_emu_tempo(period, n):
    W = R.tempo_window()
    assert W == 344
    e = R.click_train(n, period, seed=1)[None]
    tg = R.tempogram(e, W)
    g = tg.mean(axis=-1, keepdims=True)
    for kw in (dict(), dict(max_tempo=None), dict(prior=_LogNormal()), dict(start_bpm=90.0, std_bpm=0.5)):
        lp = R.log_prior(W, **kw)
        want, ok = R.tempo_pick(g, lp)
        assert ok, (period, n, kw)                                   # the precondition
        assert np.array_equal(_emu_tempo(e, lp), want), (period, n, kw)
        assert np.array_equal(_emu_tempo(e, lp, wave=False), want), (period, n, kw)
        assert np.array_equal(_emu_tempo(e, lp, stored=True), want)  # tg= given against the envelope route


def test_emu_tempo_per_frame():
    """aggregate=None: every frame is a column.  The columns whose reference pick is decisive must match (nearly all are:
    asserted)."""
    W = R.tempo_window()
    e = R.click_train(130, 11, seed=1)[None]
    tg = R.tempogram(e, W)
    lp = R.log_prior(W)
    s = R.tempo_scores(tg, lp)[0]
    want = np.argmax(s, axis=0)
    srt = np.sort(np.where(np.isfinite(s), s, -np.inf), axis=0)
    ok = srt[-1] - srt[-2] > 64 * R.EPS * np.max(np.abs(np.where(np.isfinite(s), s, 0.0)), axis=0)
    assert ok.mean() > 0.9
    got = _emu_tempo(e, lp, per_frame=True)[0]
    assert np.array_equal(got[ok], want[ok])
    print(f"per-frame tempo: {int((~ok).sum())} of {len(ok)} columns not compared (no decisive reference): {np.flatnonzero(~ok).tolist()}")


def test_emu_tempo_pick_first_maximum_and_prior():
    """Ties go to the first lag; a lag the prior excludes never wins; all excluded: lag 0 (np.argmax)."""
    g = np.zeros((2, 300), np.float32)
    g[0, [7, 270, 299]] = 0.5
    g[1, 299] = 0.9
    lp = np.zeros(300, np.float32)
    assert list(eb.tempo_pick(g, lp, n_col=1, sb=300, sk=1, sc=0, n_red=1, sr=0, div=1.0)[:, 0]) == [7, 299]
    lp[:8] = -np.inf
    assert list(eb.tempo_pick(g, lp, n_col=1, sb=300, sk=1, sc=0, n_red=1, sr=0, div=1.0)[:, 0]) == [270, 299]
    lp[:] = -np.inf
    assert list(eb.tempo_pick(g, lp, n_col=1, sb=300, sk=1, sc=0, n_red=1, sr=0, div=1.0)[:, 0]) == [0, 0]


# ---- beat tracking -----------------------------------------------------------------------------------------------------
BEAT_SETTINGS = [(100.0, True), (100.0, False), (400.0, True), (400.0, False)]


def test_emu_beat_half_period_rounds_halves_to_even():
    """h = rint(P / 2): 2.5 -> 2, 3.5 -> 4 (half-up would give 3 at P = 5; P = 3 cannot tell: 1.5 -> 2 either way)."""
    periods = (2, 3, 4, 5, 6, 7, 9, 13, 200, 201, 203)
    assert [eb.half(P) for P in periods] == [R.half(P) for P in periods] == [1, 2, 2, 2, 3, 4, 4, 6, 100, 100, 102]


@pytest.mark.parametrize("T", R.BEAT_T)
def test_emu_beat_track(T):
    """Every period x (tightness, trim) x generator, all rows of a case in one launch; intermediates within their bounds,
    masks exact."""
    worst_L = worst_C = 0.0
    n_beats = 0
    for P in R.BEAT_P:
        assert eb.half(P) == R.half(P)
        for tightness, trim in BEAT_SETTINGS:
            cases = [(kind,) + R.beat_case(kind, T, P, tightness, trim) for kind in R.BEAT_KINDS]
            x = np.stack([c[1] for c in cases])
            mask, count, L, C, link = eb.beat_track(x, [P] * len(cases), tightness=tightness, trim=trim, pad_in=(P % 2) * 3,
                                                    stages=True, grid=1 + P % 2)
            for i, (kind, o, st, redraws) in enumerate(cases):
                assert redraws <= 8
                if st is None:                                        # all zero, constant, NaN-bearing, T < 2
                    assert kind in ("zero", "constant", "nan") or T < 2
                    assert not mask[i].any() and count[i] == 0 and not L[i].any() and not C[i].any() and (link[i] == -1).all()
                    continue
                R.check_rule(kind, T, P, st, C[i])                    # the precondition (and which rule it is)
                rl = float(np.max(np.abs(L[i] - st["L"]) / R.L_bound(st, P)))
                rc = float(np.max(np.abs(C[i] - st["C"]) / R.C_bound(st, P, tightness)))
                worst_L, worst_C = max(worst_L, rl), max(worst_C, rc)
                assert rl <= 1.0 and rc <= 1.0, (kind, T, P, tightness, rl, rc)
                chain = st["all_beats"]
                assert np.array_equal(link[i][chain], st["link"][chain]) and np.array_equal(link[i] < 0, st["link"] < 0)
                assert np.array_equal(mask[i], st["mask"]), (kind, T, P, tightness, trim, np.flatnonzero(mask[i]), st["beats"])
                assert count[i] == len(st["beats"])
                n_beats += len(st["beats"])
    assert n_beats > 0 or T < 3
    assert eb.lds_overruns() == 0
    print(f"beat_track T = {T}: worst L error / bound {worst_L:.3f}, C {worst_C:.3f}")


def test_emu_beat_track_bare_spike_pins_the_tie_break():
    """One onset among exact zeros: the DP ties exactly (two orders of the same two steps, candidates that all read
    C = 0), and the tie goes to the largest d.  float64 may break such a tie differently from float32, so the links, C
    and L are compared in every bit with the float32 restatement rhythm_ref.beat_dp_f32, and L and C with the float64
    definition within their bounds."""
    n_ties = 0
    for T, P, tightness in ((65, 8, 100.0), (130, 22, 100.0), (63, 2, 400.0), (64, 3, 100.0), (431, 64, 100.0)):
        o = R.beat_row("bare_spike", T, P, seed=T)
        st = R.beat_stages(o, P, tightness)
        L32, C32, link32 = R.beat_dp_f32(o, P, tightness)
        mask, count, L, C, link = eb.beat_track(o[None], [P], tightness=tightness, stages=True)
        assert np.all(np.abs(L[0] - st["L"]) <= R.L_bound(st, P)) and np.all(np.abs(C[0] - st["C"]) <= R.C_bound(st, P, tightness))
        assert np.array_equal(L[0], L32) and np.array_equal(C[0], C32), (T, P)
        assert np.array_equal(link[0], link32), (T, P, np.flatnonzero(link[0] != link32))
        # how many frames have an exact float32 tie at the maximum (the test is about them)
        d = np.arange(2 * P, R.half(P) - 1, -1)
        tx = (-tightness * np.log(d / P) ** 2).astype(np.float32)
        for i in range(T):
            j = i - d
            v = tx + np.where(j >= 0, np.concatenate([C32[:i], np.zeros(T - i, np.float32)])[np.maximum(j, 0)], np.float32(0))
            n_ties += int(np.sum(v == v.max()) > 1)
    assert n_ties > 0


def test_emu_beat_track_periods_per_row_and_row_alone_equals_row_in_batch():
    T = 130
    rows = [R.beat_case("clicks", T, P)[0] for P in (8, 22, 3)] + [R.beat_case("random", T, 8)[0]]
    periods = [8, 22, 3, 8]
    x = np.stack(rows)
    mask, count, L, C, link = eb.beat_track(x, periods, stages=True)
    for b, P in enumerate(periods):
        one = eb.beat_track(x[b:b + 1], [P], stages=True, pad_in=1)
        for got, all_ in zip(one, (mask, count, L, C, link)):
            assert np.array_equal(got[0], all_[b])
        assert np.array_equal(mask[b], R.beat_stages(rows[b], P)["mask"])


def test_emu_beat_track_period_outside_the_range():
    """A device period below 2 or beyond the limit: no beats and count -1 (the kernel cannot return a status)."""
    o = R.beat_case("clicks", 64, 8)[0]
    x = np.stack([o, o, o, o])
    mask, count = eb.beat_track(x, [1, 8, eb.max_period() + 1, 0])
    assert list(count < 0) == [True, False, True, True] and not mask[[0, 2, 3]].any() and mask[1].any()
    assert eb.max_period() >= 2048


def test_emu_beat_track_longest_row():
    """16 384 frames, the limit; one more frame is refused with a message that names it."""
    T = eb.max_frames()
    assert T == 16384
    o, st, redraws = R.beat_case("clicks", T, 64, 400.0)
    assert st is not None and redraws <= 8
    mask, count, L, C, link = eb.beat_track(o[None], [64], tightness=400.0, stages=True)
    R.check_rule("clicks", T, 64, st, C[0])             # (at P = 22 the premise fails: |C32 - C64| = 0.0104 against thr / 2 = 0.0071)
    assert np.array_equal(mask[0], st["mask"]) and count[0] == len(st["beats"]) > 200
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    r = eb.beat_track_raw(p, 1, T + 1, T + 1, p, 100.0, p + (1 << 40), p)
    assert r == UNSUPPORTED and str(T) in eb.last_error()


def test_emu_beat_track_rejects_before_launching():
    buf = np.zeros(4096, np.float32)
    s, m, c = buf.ctypes.data, buf.ctypes.data + 8192, buf.ctypes.data + 12288

    def rc(*a):
        return eb.beat_track_raw(*a), eb.last_error()

    #          x  B  T rs per tight mask count
    assert rc(None, 1, 8, 8, c, 100.0, m, c)[0] == INVALID and rc(s, 1, 8, 8, None, 100.0, m, c)[0] == INVALID
    assert rc(s, 1, 8, 8, c, 100.0, None, c)[0] == INVALID and rc(s, 1, 8, 8, c, 100.0, m, None)[0] == INVALID
    assert "non-empty" in rc(s, 0, 8, 8, c, 100.0, m, c)[1] and "non-empty" in rc(s, 1, 0, 8, c, 100.0, m, c)[1]
    assert "row stride" in rc(s, 2, 8, 7, c, 100.0, m, c)[1]
    assert "tightness" in rc(s, 1, 8, 8, c, 0.0, m, c)[1]
    assert "overlaps" in rc(s, 1, 8, 8, c, 100.0, s + 4, c)[1]
