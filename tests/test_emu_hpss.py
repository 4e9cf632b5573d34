"""CPU: the HPSS kernel source (kernels_hpss.h) on the SIMT emulator of tests/emu against the definition in
tests/hpss_ref.py: the medians and the hard mask bit for bit, the soft mask within the bound of hpss_ref.soft_bound.

The tile height is forced to 8 bins (a tile is always 64 frames wide) so that the small arrays span several tiles in
both directions; (1,7,63), (1,8,64), (1,9,65) sit just below, at and just past the tile edge on both axes.  Every
buffer lies between NaN bands and, in the padded-row variants, has NaN pad columns: emu_hpss_bind.hpss asserts that
none of them was written, and a read of one would surface as a NaN in a result.

Worst soft-mask error seen on the emulator, in units of the bound: power 1 / 2 (bound 4 eps) 0.19; power 0.5 / 3.7
(bound 4 x the float32 NumPy route's own worst error) 0.25 - the emulator's powf is NumPy's."""

import os
import sys

import numpy as np
import pytest

import hpss_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_hpss_bind as eb  # noqa: E402

FT = 8
SHAPES = [(2, 70, 65), (1, 1, 40), (1, 33, 3), (1, 9, 1), (3, 5, 7), (1, FT - 1, 63), (1, FT, 64), (1, FT + 1, 65)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
GENERAL_K = [(1, 1), (2, 2), (3, 3), (4, 4), (30, 30), (31, 31), (32, 32), (63, 63), (255, 255), (3, 17), (32, 5), (255, 1), (2, 63)]
MARGINS = [(1.0, 1.0), (2.0, 5.0)]

_cache = {}


def case(shape, is_complex=False):
    """(input, magnitudes the kernels see, harm, perc at (31, 31)): computed once, never modified."""
    key = (shape, is_complex)
    if key not in _cache:
        S = R.make_input(shape, seed=sum(shape), is_complex=is_complex)
        M = R.magnitude32(S) if is_complex else S
        harm, perc = R.medians(M, 31, 31)
        for a in (S, M, harm, perc):
            a.setflags(write=False)
        _cache[key] = (S, M, harm, perc)
    return _cache[key]


def test_reference_self_check():
    """SciPy's filter == the explicit reflect index + sort wherever the window stays within four axis lengths
    (hpss_ref.scipy_reflects): every axis length 1 .. 40 against every window size of this file, with continuous
    values so that a wrong index cannot hide behind a tie."""
    rng = np.random.default_rng(5)
    n_scipy = 0
    for n in list(range(1, 41)) + [65, 70]:
        M = rng.random((n, 3)).astype(np.float32)
        for k in (1, 2, 3, 4, 5, 17, 30, 31, 32, 63, 101, 255):
            if R.scipy_reflects(k, n):
                n_scipy += 1
                assert np.array_equal(R.median_filter(M, size=(k, 1), mode="reflect"), R.medians_explicit(M, 1, k)[1]), (n, k)
                assert np.array_equal(R.median_filter(M.T, size=(1, k), mode="reflect"), R.medians_explicit(M.T, k, 1)[0]), (n, k)
            for a, b in zip(R.medians(M, 1, k), R.medians_explicit(M, 1, k)):
                assert np.array_equal(a, b)
    assert n_scipy >= 400
    # 31-windows, the default: SciPy is the reference for every axis longer than 3
    assert all(R.scipy_reflects(31, n) for n in (1, 4, 5, 7, 9, 33)) and not R.scipy_reflects(31, 3)
    for shape in [(5, 7), (33, 3), (1, 40), (70, 65), (9, 1), (3, 5, 7)]:
        M = R.make_input(shape, seed=3)
        for k in (1, 2, 3, 4, 17, 30, 31, 32, 63, 101, 255):
            for a, b in zip(R.medians(M, k, k), R.medians_explicit(M, k, k)):
                assert np.array_equal(a, b), (shape, k)
    assert list(R.reflect(np.arange(-9, 9), 4)) == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0]


def test_network_is_the_documented_one():
    """DESIGN.md 9.3 quotes these: comparators kept of Batcher's 191, and min / max operations per median."""
    assert eb.network() == (152, 274)
    assert eb.default_tile() == 32
    assert eb.lib().emu_hpss_fused(31, 31) == 1 and eb.lib().emu_hpss_fused(31, 17) == 0


@pytest.mark.parametrize("is_complex", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emu_fused_medians_are_scipys(shape, is_complex):
    S, M, harm, perc = case(shape, is_complex)
    for pad_in, pad_out in ((0, 0), (3, 5)):
        h, p = eb.hpss(S, mode=2, f_tile=FT, pad_in=pad_in, pad_out=pad_out)
        assert eb.geometry()["fused"] == 1 and eb.geometry()["f_tile"] == FT
        assert np.array_equal(h, harm) and np.array_equal(p, perc)
    h, p = eb.hpss(S, mode=2, f_tile=FT, grid=2)             # grid-stride over the tiles
    assert np.array_equal(h, harm) and np.array_equal(p, perc)
    h, p = eb.hpss(S, mode=2)                                 # the default tile
    assert np.array_equal(h, harm) and np.array_equal(p, perc)
    assert eb.lds_overruns() == 0


@pytest.mark.parametrize("k", GENERAL_K, ids=[f"{a}-{b}" for a, b in GENERAL_K])
def test_emu_general_medians_are_scipys(k):
    for shape in SHAPES:
        if max(k) == 255 and shape == (2, 70, 65):
            continue                                           # 65 000 comparisons per output: the small shapes hold the same paths
        for is_complex in (False, True):
            S, M, _, _ = case(shape, is_complex)
            harm, perc = R.medians(M, *k)
            h, p = eb.hpss(S, kernel_size=k, mode=2, general=True, f_tile=FT, pad_in=1, pad_out=2)
            assert eb.geometry()["fused"] == 0
            assert np.array_equal(h, harm) and np.array_equal(p, perc), (shape, is_complex)
    assert eb.lds_overruns() == 0


@pytest.mark.parametrize("general", [False, True], ids=["fused", "general"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emu_hard_mask_is_exact(shape, general):
    S, M, harm, perc = case(shape)
    for mh, mp in MARGINS:
        want = R.masks(harm, perc, mh, mp, np.inf)
        got = eb.hpss(S, margin=(mh, mp), power=np.inf, mode=1, general=general, f_tile=FT)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert set(np.unique(got[0])) <= {0.0, 1.0}


def soft_cases():
    return [(shape, c, mh, mp) for shape in SHAPES for c in (False, True) for mh, mp in MARGINS]


@pytest.mark.parametrize("power", [1.0, 2.0, 0.5, 3.7])
@pytest.mark.parametrize("general", [False, True], ids=["fused", "general"])
def test_emu_soft_mask(general, power):
    bound = R.soft_bound([case(shape, c)[2:] + (mh, mp) for shape, c, mh, mp in soft_cases()], power)
    worst = 0.0
    for shape, is_complex, mh, mp in soft_cases():
        S, M, harm, perc = case(shape, is_complex)
        want = R.masks(harm, perc, mh, mp, power, np.float64)
        got = eb.hpss(S, margin=(mh, mp), power=power, mode=1, general=general, f_tile=FT, pad_out=3)
        for g, w, X, Rf in zip(got, want, (harm, perc), (perc * np.float32(mh), harm * np.float32(mp))):
            err = float(np.max(np.abs(g.astype(np.float64) - w)))
            worst = max(worst, err)
            assert err <= bound, (shape, is_complex, mh, mp, err, bound)
            tiny = np.maximum(X, Rf) < R.FLT_MIN          # not excluded above; exactly 0.5 or 0 here
            assert tiny.any() or shape[0] == 1
            assert np.all(g[tiny] == (0.5 if (mh == 1 and mp == 1) else 0.0))
    print(f"soft mask power={power} general={general}: worst error {worst:.3g}, bound {bound:.3g}, ratio {worst / bound:.3f}")


@pytest.mark.parametrize("is_complex", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emu_components_masks_and_null_outputs(shape, is_complex):
    """Mode 0 == S * mask of mode 1 in every bit; an output that is not asked for changes nothing about the other;
    the network kernel and the rank-counting kernel return identical bits in every mode."""
    S, M, harm, perc = case(shape, is_complex)
    for mh, mp in MARGINS:
        kw = dict(margin=(mh, mp), f_tile=FT)
        mask = eb.hpss(S, mode=1, **kw)
        comp = eb.hpss(S, mode=0, pad_in=2, pad_out=2, **kw)
        for c, m in zip(comp, mask):
            if is_complex:
                assert c.dtype == np.complex64
                assert np.array_equal(c.real, S.real * m) and np.array_equal(c.imag, S.imag * m)
            else:
                assert np.array_equal(c, S * m)
        for mode, both in ((0, comp), (1, mask), (2, (harm, perc))):
            only_h = eb.hpss(S, mode=mode, want=(True, False), **kw)
            only_p = eb.hpss(S, mode=mode, want=(False, True), **kw)
            assert only_h[1] is None and only_p[0] is None
            assert np.array_equal(only_h[0], both[0]) and np.array_equal(only_p[1], both[1])
            gen = eb.hpss(S, mode=mode, general=True, **kw)
            assert eb.geometry()["fused"] == 0
            assert np.array_equal(gen[0], both[0]) and np.array_equal(gen[1], both[1])
            gen_h = eb.hpss(S, mode=mode, general=True, want=(True, False), **kw)
            gen_p = eb.hpss(S, mode=mode, general=True, want=(False, True), **kw)
            assert np.array_equal(gen_h[0], both[0]) and np.array_equal(gen_p[1], both[1])
    assert eb.lds_overruns() == 0


@pytest.mark.parametrize("general", [False, True], ids=["fused", "general"])
def test_emu_clip_alone_equals_clip_in_batch(general):
    for shape in [(2, 70, 65), (3, 5, 7)]:
        for is_complex in (False, True):
            S = case(shape, is_complex)[0]
            for mode, power in ((2, 2.0), (1, 2.0), (0, 3.7)):
                kw = dict(mode=mode, power=power, general=general, f_tile=FT)
                batch = eb.hpss(S, **kw)
                for b in range(shape[0]):
                    alone = eb.hpss(S[b:b + 1], **kw)
                    assert np.array_equal(alone[0][0], batch[0][b]) and np.array_equal(alone[1][0], batch[1][b])


def test_emu_prepare_rejects_before_launching():
    """Statuses of ap_prepare_hpss; the pointers are never dereferenced on these paths."""
    buf = np.zeros(4096, np.float32)
    s, h, p = buf.ctypes.data, buf.ctypes.data + 4096, buf.ctypes.data + 8192
    INVALID, UNSUPPORTED = -1, -2

    def rc(*a, **k):
        r = eb.raw_call(*a, **k)
        return r, eb.last_error()

    ok = (s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, h, p, 8)
    assert rc(None, *ok[1:])[0] == INVALID
    assert rc(*ok[:13], None, None, 8)[0] == INVALID
    for bad in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (-1, 4, 8)):
        assert rc(s, 0, *bad, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, h, p, 8)[0] == INVALID
    for k in ((0, 31), (31, 256), (-3, 31)):
        r, msg = rc(s, 0, 1, 4, 8, 8, *k, 1.0, 1.0, 2.0, 2, 0, h, p, 8)
        assert r == INVALID and "kernel_size must be an integer in 1 .. 255" in msg
    assert "row strides" in rc(s, 0, 1, 4, 8, 7, 31, 31, 1.0, 1.0, 2.0, 2, 0, h, p, 8)[1]
    assert "row strides" in rc(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, h, p, 7)[1]
    assert "Margins must be >= 1.0" in rc(s, 0, 1, 4, 8, 8, 31, 31, 0.5, 1.0, 2.0, 0, 0, h, p, 8)[1]
    assert "power must be strictly positive" in rc(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 0.0, 0, 0, h, p, 8)[1]
    assert "mode" in rc(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 3, 0, h, p, 8)[1]
    r, msg = rc(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, s, p, 8)
    assert r == INVALID and "overlaps S" in msg
    assert rc(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, h, s + 64, 8)[0] == INVALID      # inside S
    assert "outputs overlap" in rc(s, 0, 1, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, h, h + 4, 8)[1]
    r, msg = rc(s, 0, 1, (1 << 28) + 1, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, h + (1 << 40), None, 8)
    assert r == UNSUPPORTED and "2^28" in msg
    r, msg = rc(s, 0, 1 << 33, 4, 8, 8, 31, 31, 1.0, 1.0, 2.0, 2, 0, h + (1 << 50), None, 8)
    assert r == UNSUPPORTED and "tiles" in msg
