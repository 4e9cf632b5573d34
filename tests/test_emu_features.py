"""CPU: the feature kernels (kernels_features.h) on the SIMT emulator of tests/emu against float64 restatements.

Every kernel of the header runs here with the geometry the product's heuristics never choose on a test-sized
input: the full 256-slot tile of the block RMS / ZCR kernel, rows longer than one chunk and shorter than the filter
in the Savitzky-Golay kernels, de-emphasis on chunk borders and from unaligned pointers, spectral statistics with
empty stripes.  Inputs sit between NaN bands and outputs between sentinel bands (emu_features_bind.Guarded), so a
read or a write outside an array fails the comparison.  Tolerances are those of the GPU tests of the same operation
(test_gpu_features.py / test_gpu_next_rows.py); counts, copies and bit-defined results are compared exactly.

Clip 0 of every batch of signals carries a run of exact zeros and a -0.0: (x >= 0) is the sign test."""

import importlib
import os
import sys

import numpy as np
import pytest
from scipy import signal

from oracle import audio_oracle as ao

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_features_bind as eb  # noqa: E402

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def clips(B, L, seed, scale=0.3):
    y = (np.random.default_rng(seed).standard_normal((B, L)) * scale).astype(F32)
    if L >= 8:
        a = L // 3
        n = max(2, min(L // 5, 40))
        y[0, a:a + n] = 0.0
        y[0, a + n // 2] = -0.0
    return y


# ====================================================================================== frame statistics, block kernel
def _check_frames(y, fl, hop, center, pad_mode, G=0, rms=True, zcr=True, expect_route=eb.ROUTE_BLOCKS, force_span=False):
    r, z, route, g = eb.frame_stats(y, frame_length=fl, hop=hop, center=center, pad_mode=pad_mode, rms=rms, zcr=zcr, G=G,
                                    force_span=force_span)
    assert route == expect_route
    kw = dict(frame_length=fl, hop_length=hop, center=center, pad_mode=pad_mode)
    if rms:
        np.testing.assert_allclose(r, ao.rms(y, **kw)[:, 0, :], rtol=1e-5, atol=1e-7)
    else:
        assert r is None
    if zcr:
        np.testing.assert_array_equal(z, ao.zero_crossing_rate(y, **kw)[:, 0, :])      # counts: exact
    else:
        assert z is None
    return r, z, g


@pytest.mark.parametrize("fl,hop,L,center,pad_mode", [
    (64, 4, 1200, True, "constant"),         # m = 16, hop = 4: one group of four samples per block
    (64, 4, 964, True, "edge"),              # the same with a last tile of one frame (T = 242)
    (2048, 512, 140000, True, "edge"),       # m = 4, two trips of the g0 loop (the carry hand-over); ragged last tile
    (1024, 64, 1024 + 64 * 245, False, "constant"),   # m = 16; the last block ends exactly at L
])
def test_block_kernel_full_tile(fl, hop, L, center, pad_mode):
    """G = APF_MAX_BLOCKS - m + 1 frames per workgroup - all 256 slots of bss / bzin / bzb - with T > G, so a second,
    ragged tile follows.  The product halves G until 1024 workgroups exist; the emulator twin keeps what
    ap_prepare_frame_stats sizes before that loop.  (Block kernel == span kernel is asserted on the smaller shapes
    below; here both would be compared with the same exact oracle counts.)"""
    m = fl // hop
    T = eb.n_frames(L, fl, hop, center)
    y = clips(1, L, 100 + hop)
    r, z, g = _check_frames(y, fl, hop, center, pad_mode)
    assert g == eb.max_blocks() - m + 1 and T > g


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("pad_mode", ["constant", "edge"])
def test_block_kernel_tiles_hops_and_outputs(center, pad_mode):
    B = 2
    # hop = 260: 65 groups of four, the second trip of the g0 loop has one live lane; hop = 512: two full trips
    for fl, hop, L, G in ((520, 260, 2600, 5), (1024, 512, 4096, 0), (16, 4, 163, 7), (400, 100, 1500, 3)):
        y = clips(B, L, 7 * hop + fl)
        y[1, 0] = -0.5                       # a first sample whose left neighbour (padding: 0 or itself) differs in sign or not
        r, z, g = _check_frames(y, fl, hop, center, pad_mode, G=G)
        _, zs, _ = _check_frames(y, fl, hop, center, pad_mode, rms=False, force_span=True, expect_route=eb.ROUTE_SPAN)
        np.testing.assert_array_equal(z, zs)
        if hop < 100:
            continue
        # each output alone: the other pointer is NULL
        r1, _, _ = _check_frames(y, fl, hop, center, pad_mode, G=G, zcr=False)
        _, z1, _ = _check_frames(y, fl, hop, center, pad_mode, G=G, rms=False)
        np.testing.assert_array_equal(r1, r)
        np.testing.assert_array_equal(z1, z)


def test_block_kernel_last_tile_of_one_frame_and_ragged():
    """With a forced small tile, so that many tiles run (test_block_kernel_full_tile has the full-sized ones)."""
    fl, hop = 64, 4
    for T, G in ((41, 8), (45, 8), (48, 8), (17, 16)):       # last tile: one frame, ragged, full, one frame
        L = (T - 1) * hop + 2                # centred: T = 1 + L // hop
        assert eb.n_frames(L, fl, hop, True) == T
        _check_frames(clips(2, L, T), fl, hop, True, "edge", G=G)


def test_block_kernel_refuses_a_tile_beyond_its_arrays():
    """The twin checks G + m - 1 <= APF_MAX_BLOCKS before it launches: static LDS arrays have no guard band."""
    with pytest.raises(ValueError, match="slots"):
        eb.frame_stats(clips(1, 2000, 1), frame_length=64, hop=4, G=eb.max_blocks() - 14)


# ====================================================================================== frame statistics, span kernel
@pytest.mark.parametrize("fl,hop,L,center,pad_mode,G_expect", [
    (100, 33, 2300, True, "edge", 64),           # frame_length no multiple of hop; G = 64
    (3, 1, 80, True, "constant", 64),            # hop = 1, frame_length = 3
    (50, 1, 120, False, "edge", 64),
    (16384, 100, 17000, False, "constant", 1),   # G = 1: the frame alone fills the budget
    (16500, 64, 16500 + 3 * 64, False, "edge", 1),
    (2048, 512, 6000, True, "constant", 12),     # the block kernel's shape through the span kernel (force_span)
])
def test_span_kernel(fl, hop, L, center, pad_mode, G_expect):
    y = clips(2, L, fl + hop)
    before = eb.lds_overruns()
    _, _, g = _check_frames(y, fl, hop, center, pad_mode, expect_route=eb.ROUTE_SPAN, force_span=True)
    assert g == min(G_expect, eb.n_frames(L, fl, hop, center))
    _check_frames(y, fl, hop, center, pad_mode, expect_route=eb.ROUTE_SPAN, force_span=True, G=3)
    assert eb.lds_overruns() == before


def test_frame_stats_sign_of_zero():
    x = np.array([0.0, -0.0, 1.0, -1.0, 0.0, 0.0, -2.0, 3.0] * 40, F32)
    for force_span in (False, True):
        _check_frames(x[None], 16, 8, True, "edge", force_span=force_span,
                      expect_route=eb.ROUTE_SPAN if force_span else eb.ROUTE_BLOCKS)


# ====================================================================================== de-emphasis
def _deemph64(y, coef, zi):
    """scipy.signal.lfilter([1], [1, -coef]) in float64 on the float32 samples, with the float32 coefficient the
    kernel receives.  zi None: zero state and librosa's correction ((2-c) y0 - y1) / (3-c) c^n (none for a one-sample
    clip, which has no y1).  zf is lfilter's final state, before the correction."""
    c = float(F32(coef))
    y64 = y.astype(np.float64)
    B, L = y.shape
    z = np.zeros((B, 1)) if zi is None else np.broadcast_to(np.asarray(zi, F32).astype(np.float64).reshape(-1, 1), (B, 1))
    out, zf = signal.lfilter([1.0], [1.0, -c], y64, zi=z, axis=-1)
    if zi is None and L > 1:
        out = out - ((2 - c) * y64[:, 0:1] - y64[:, 1:2]) / (3 - c) * c ** np.arange(L, dtype=np.float64)
    return out, zf[:, 0]


def _check_deemph(y, coef, zi, off_in=0, off_out=0):
    want, zfw = _deemph64(y, coef, zi)
    scale = max(1.0, float(np.abs(want).max()))
    got = {}
    for force in (1, 2):                     # one workgroup per clip; end states + chunks
        d, zf, chunked = eb.deemphasis(y, coef=coef, zi=zi, off_in=off_in, off_out=off_out, force=force)
        assert chunked == (force == 2)
        np.testing.assert_allclose(d, want, rtol=1e-4, atol=2e-5 * scale, err_msg=f"force={force}")
        np.testing.assert_allclose(zf, zfw, rtol=1e-4, atol=2e-5 * scale, err_msg=f"zf force={force}")
        got[force] = d
    np.testing.assert_allclose(got[2], got[1], rtol=1e-4, atol=2e-5 * scale)
    return got


DE_L = [1, 2, 15, 16, 17, 4096, 4097, 16384, 16385, 32768, 32769, 100001]


@pytest.mark.parametrize("L", DE_L)
def test_deemphasis_lengths(L):
    """Every tile / chunk border: 4096 = one tile, 16384 = one chunk, one sample past each, a ragged seventh chunk."""
    y = clips(2, L, L, scale=0.1)
    for zi in (None, np.array([0.3, -0.2], F32)):
        _check_deemph(y, 0.97, zi)
    # the product's own choice of route: chunked exactly when the clip has more than one chunk and a workspace exists
    _, _, chunked = eb.deemphasis(y, coef=0.97, force=0)
    assert chunked == (L > 16384)
    _, _, chunked = eb.deemphasis(y, coef=0.97, force=0, workspace=False)
    assert not chunked


def test_deemphasis_chunks_in_any_order():
    """Workgroups of a launch finish in any order on the GPU; the emulator runs them ascending unless told otherwise.
    The second pass run descending: out and zf (which only the chunk that holds sample L - 1 may write) stay the same."""
    for L, zi in ((32769, None), (40000, np.array([0.3, -0.2], F32))):
        y = clips(2, L, L + 9, scale=0.1)
        want, zfw = _deemph64(y, 0.97, zi)
        d, zf, chunked = eb.deemphasis(y, coef=0.97, zi=zi, force=3)
        assert chunked
        np.testing.assert_allclose(d, want, rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(zf, zfw, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("coef", [0.0, 0.5, 0.999, 1.0])
def test_deemphasis_coefficients(coef):
    """coef = 1 never decays (state crosses every chunk border undiminished), 0.999 decays over thousands of samples,
    0 makes the filter the identity."""
    for L in (17, 4097, 16385, 32769):
        y = clips(2, L, L + 1, scale=0.1)
        for zi in (None, 0.25):
            got = _check_deemph(y, coef, zi)
            if coef == 0.0 and zi is not None:
                np.testing.assert_array_equal(got[1][:, 1:], y[:, 1:])


@pytest.mark.parametrize("off_in,off_out", [(1, 0), (0, 1), (1, 1), (2, 3)])
def test_deemphasis_unaligned_pointers(off_in, off_out):
    """The 16-byte tile moves need both pointers aligned; any other combination takes the 4-byte form.  Clip 1 of a
    clip length that is no multiple of 4 starts unaligned whatever the base pointer is."""
    for L in (4096, 16384, 32769):
        y = clips(2, L, L + off_in, scale=0.1)
        _check_deemph(y, 0.97, None, off_in, off_out)
    _check_deemph(clips(3, 4097, 3, scale=0.1), 0.9, 0.1, off_in, off_out)


# ====================================================================================== pre-emphasis
@pytest.mark.parametrize("L", [1, 2, 4, 5, 4096, 4097])
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 0), (0, 1)])
def test_preemphasis(L, off_in, off_out):
    B = 3
    y = clips(B, L, 40 + L)
    for zi in (None, np.array([0.1, -0.2, 0.3], F32)):
        for coef in (0.97, 0.0, 1.0):
            for grid in (0, 1):              # grid = 1: every thread makes several trips of the stride loop
                out, zf, quads = eb.preemphasis(y, coef=coef, zi=zi, off_in=off_in, off_out=off_out, grid=grid)
                assert quads == (L % 4 == 0 and off_in == 0 and off_out == 0)
                if L == 1 and zi is None:
                    # a one-sample clip has no y[1]; the kernel's rule is zi = y[0] (and it must not read the next clip)
                    want, zfw = y + y, y[:, -1]
                else:
                    want, zfw = ao.preemphasis(y, coef=coef, zi=zi, return_zf=True)
                    zfw = zfw[:, 0]
                np.testing.assert_allclose(out, want, rtol=1e-6, atol=1e-6)
                np.testing.assert_array_equal(zf, zfw)
    out, zf, _ = eb.preemphasis(y, want_zf=False, off_in=off_in, off_out=off_out)
    assert zf is None


# ====================================================================================== Savitzky-Golay
_mfcc_mod = importlib.import_module("mlx_audio_primitives_amd.mfcc")


def _tables(width, order):
    taps, edge = _mfcc_mod._savgol_tables(width, order, order, 1.0, "cpu")
    return taps.numpy(), edge.numpy()


def _check_savgol(x, width, order, mode, cval, **kw):
    """x (outer, n, inner).  Reference: scipy.signal.savgol_filter on the float64 samples, deriv = order."""
    taps, edge = _tables(width, order)
    got, rows = eb.savgol(x, taps, edge, mode=mode, cval=cval, **kw)
    want = signal.savgol_filter(x.astype(np.float64), width, polyorder=order, deriv=order, axis=1, mode=mode, cval=cval)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4, err_msg=f"n={x.shape[1]} w={width} o={order} {mode}")
    return got, rows


@pytest.mark.parametrize("n", [1, 3, 5, 44, 1024, 1025, 2500, 4097])
@pytest.mark.parametrize("width,order", [(3, 1), (9, 1), (9, 2), (63, 1), (63, 2), (3, 2)])
def test_savgol_rows_kernel(n, width, order):
    """Rows of one sample, shorter than the filter, exactly one chunk (1024), one past it, several chunks with a ragged
    last one.  The rows kernel and the generic kernel on the same input."""
    x = np.random.default_rng(n * 100 + width).standard_normal((2, n, 1)).astype(F32)
    for mode in ("interp", "nearest", "mirror", "constant", "wrap"):
        if mode == "interp" and width > n:
            with pytest.raises(ValueError, match="cannot exceed"):
                eb.savgol(x, *_tables(width, order), mode=mode)
            continue
        got, rows = _check_savgol(x, width, order, mode, 0.75)
        assert rows
        gen, rows = _check_savgol(x, width, order, mode, 0.75, force_generic=True, grid=3)
        assert not rows
        np.testing.assert_allclose(gen, got, rtol=1e-6, atol=1e-6)        # same taps, same order of the sum


@pytest.mark.parametrize("mode", ["interp", "nearest", "mirror", "constant", "wrap"])
def test_savgol_generic_kernel(mode):
    rng = np.random.default_rng(77)
    # a strided axis (inner > 1)
    for n, width in ((44, 9), (7, 9), (130, 63)):
        if mode == "interp" and width > n:
            continue
        _, rows = _check_savgol(rng.standard_normal((3, n, 5)).astype(F32), width, 2, mode, -1.5, off=1)
        assert not rows
    # width 65 on a contiguous axis: more taps than the rows kernel keeps in LDS
    for n in (100, 30):
        if mode == "interp" and 65 > n:
            continue
        _, rows = _check_savgol(rng.standard_normal((2, n, 1)).astype(F32), 65, 1, mode, 0.5)
        assert not rows


# ====================================================================================== spectral statistics
def _rolloff_agrees(got, want, freq, frac=0.02):
    """The condition of test_gpu_features._rolloff_agrees: never more than one bin away, a neighbouring bin in at
    most 2 % of the frames."""
    assert got.shape == want.shape
    step = freq[1] - freq[0] if len(freq) > 1 else 0.0
    diff = np.abs(got - want)
    assert (diff <= step * 1.001).all(), diff.max()
    assert (diff > 0).mean() <= frac, (diff > 0).mean()


def _spectrum(B, F, T, seed, complex_in):
    rng = np.random.default_rng(seed)
    if complex_in:
        Z = rng.standard_normal((B, F, T, 2)).astype(F32)
    else:
        Z = np.abs(rng.standard_normal((B, F, T))).astype(F32)
    if T >= 3:
        Z[0, :, 1] = 0.0                     # an all-zero frame
        Z[1, :, T - 1] = 0.0                 # all energy in the last bin
        Z[1, F - 1, T - 1] = 3.0
    return Z


def _check_spectral(Z, freq, complex_in, power, p, norm, roll, want, given_centroid=False):
    B, F, T = Z.shape[:3]
    mag = np.sqrt(Z[..., 0].astype(np.float64) ** 2 + Z[..., 1].astype(np.float64) ** 2) if complex_in else Z.astype(np.float64)
    S = (mag ** power).astype(F32)           # what the oracle's callers hand it: |X|^power in float32
    cin = None
    if given_centroid:
        cin = (np.random.default_rng(5).uniform(0, float(freq[-1]) + 1.0, (B, 1, T))).astype(F32)
    got = eb.spectral_stats(Z, freq, is_complex=complex_in, power=power, p=p, norm=norm, roll_percent=roll,
                            centroid_in=cin, want=want)
    assert set(got) == set(want)
    if "centroid" in want:
        np.testing.assert_allclose(got["centroid"], ao.spectral_centroid(S=S, freq=freq)[:, 0], rtol=1e-4, atol=1e-2)
    if "bandwidth" in want:
        wb = ao.spectral_bandwidth(S=S, freq=freq, p=p, norm=norm, centroid=cin)[:, 0]
        np.testing.assert_allclose(got["bandwidth"], wb, rtol=2e-4, atol=1e-2 if norm else 0.0)
    if "flatness" in want:
        # (the kernel's flatness is over the spectrum it was given: S with amin, no further power)
        np.testing.assert_allclose(got["flatness"], ao.spectral_flatness(S=S, amin=1e-10)[:, 0], rtol=2e-4, atol=1e-6)
    if "rolloff" in want:
        _rolloff_agrees(got["rolloff"], ao.spectral_rolloff(S=S, freq=freq, roll_percent=roll)[:, 0], freq)
    return got


ALL4 = ("centroid", "bandwidth", "rolloff", "flatness")
SPEC_SHAPES = [(1025, 45), (513, 32), (201, 1), (9, 70), (8, 32), (5, 33), (1, 3)]


@pytest.mark.parametrize("F,T", SPEC_SHAPES)
@pytest.mark.parametrize("complex_in", [False, True])
def test_spectral_stats_shapes(F, T, complex_in):
    """F < 8 leaves stripes without bins, F = 9 gives stripes of two bins and empty ones, F not a multiple of 4 runs
    the scalar tail of the bin loop; T = 1 / 33 / 45 / 70 leave dead frames in the last tile."""
    freq = np.linspace(0, 11025.0, F).astype(F32)
    Z = _spectrum(2, F, T, F * 1000 + T, complex_in)
    for power, p, norm in ((1.0, 2.0, True), (2.0, 1.0, False), (1.5, 3.0, True)):
        for roll in (0.1, 0.85) if power == 1.0 else (0.85,):
            got = _check_spectral(Z, freq, complex_in, power, p, norm, roll, ALL4)
        # each output alone gives what it gave together with the others
        for name in ALL4:
            one = _check_spectral(Z, freq, complex_in, power, p, norm, 0.85, (name,))
            np.testing.assert_array_equal(one[name], got[name])
    _check_spectral(Z, freq, complex_in, 1.0, 2.0, True, 0.85, ("bandwidth",), given_centroid=True)
    _check_spectral(Z, freq, complex_in, 1.0, 1.0, False, 0.85, ("bandwidth", "rolloff"), given_centroid=True)


@pytest.mark.parametrize("roll", [0.0, 0.1, 0.85, 1.0])
def test_spectral_rolloff_percentages(roll):
    for F, T in ((1025, 45), (9, 70), (5, 33)):
        freq = np.linspace(0, 11025.0, F).astype(F32)
        Z = _spectrum(2, F, T, F + T, False)
        got = _check_spectral(Z, freq, False, 1.0, 2.0, True, roll, ("rolloff",))["rolloff"]
        assert got[0, 1] == freq[0]                                      # the all-zero frame: bin 0
        if roll > 0.0:
            assert got[1, T - 1] == freq[-1]                             # all energy in the last bin
    with pytest.raises(ValueError, match="roll_percent must be between 0 and 1"):
        eb.spectral_stats(Z, freq, roll_percent=1.5)
    with pytest.raises(ValueError, match="p must be positive"):
        eb.spectral_stats(Z, freq, p=0.0)


# ====================================================================================== spectral contrast
def _contrast64(S, bands, linear):
    """Mean of the k smallest and of the k largest values of the band's bins in float64 (k clipped to the band), rounded
    to float32 as the kernel's sums are; bands without bins give 0 (both clamp to 1e-10 in dB)."""
    B, F, T = S.shape
    out = np.zeros((B, len(bands), T))
    for j, (lo, hi, k) in enumerate(bands):
        valley = peak = np.zeros((B, T))
        if hi > lo:
            k = min(k, hi - lo)
            ranked = np.sort(S[:, lo:hi, :].astype(np.float64), axis=1)
            valley = ranked[:, :k, :].mean(axis=1).astype(F32).astype(np.float64)
            peak = ranked[:, -k:, :].mean(axis=1).astype(F32).astype(np.float64)
        if linear:
            out[:, j, :] = peak - valley
        else:
            out[:, j, :] = 10 * np.log10(np.maximum(peak, 1e-10)) - 10 * np.log10(np.maximum(valley, 1e-10))
    return out


@pytest.mark.parametrize("linear", [False, True])
def test_spectral_contrast_hand_bands(linear):
    B, F, T = 2, 64, 150                     # B T = 300: two workgroups, the second one ragged
    S = np.abs(np.random.default_rng(21).standard_normal((B, F, T))).astype(F32)
    S[0, :, 3] = 0.5                         # a constant column: every selection is a tie
    S[1, 10:30, 9] = 2.0                     # ties inside a band, among the largest
    S[1, 30:50, 11] = 0.0                    # ties among the smallest
    bands = [(0, 0, 1), (7, 5, 2),           # hi <= lo: no bins
             (2, 5, 9),                      # k larger than the band
             (5, 40, 1), (10, 60, 3), (0, F, 2), (0, F, F), (63, 64, 1)]
    got = eb.spectral_contrast(S, bands, linear=linear)
    want = _contrast64(S, bands, linear)
    if linear:
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-5 * float(S.max()))
    else:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-4)
    assert (got[:, :2] == 0).all()
    # a column with a NaN: the selection must end (the launch returning is the check) and every other column must
    # be what it was
    Sn = S.copy()
    Sn[0, 20, 5] = np.nan
    gn = eb.spectral_contrast(Sn, bands, linear=linear)
    keep = np.ones((B, T), bool)
    keep[0, 5] = False
    np.testing.assert_array_equal(gn.transpose(0, 2, 1)[keep], got.transpose(0, 2, 1)[keep])
    np.testing.assert_array_equal(gn[0, [0, 1, 2, 7], 5], got[0, [0, 1, 2, 7], 5])    # bands that do not hold bin 20


def test_spectral_contrast_octave_bands_against_oracle():
    features = importlib.import_module("mlx_audio_primitives_amd.features")
    F, T = 257, 37
    freq = ao.fft_frequencies(16000, 512)
    S = np.abs(np.random.default_rng(8).standard_normal((3, F, T))).astype(F32)
    for n_bands, fmin, q in ((5, 100.0, 0.02), (7, 200.0, 0.3), (3, 20.0, 1.0)):
        bands = features._contrast_bands(freq, fmin, n_bands, q)
        got = eb.spectral_contrast(S, bands)
        np.testing.assert_allclose(got, ao.spectral_contrast(S=S, sr=16000, n_fft=512, freq=freq, fmin=fmin, n_bands=n_bands,
                                                             quantile=q), rtol=1e-5, atol=2e-4)


# ====================================================================================== ACF peak pick
def _acf_walk(row, min_lag, max_lag, thr, sr):
    """The definition, on one row of raw autocorrelation: v[lag] = r[lag] / r[0] as a float32 division (0 past the
    row); the FIRST interior lag of [min_lag, max_lag] with v strictly above both neighbours and above thr, else the
    global maximum if it is above thr.  Ties: a plateau is no local maximum (the comparisons are strict), and of equal
    global maxima the smallest lag counts.  Lag 0 never voices.  periodicity = the global maximum."""
    r0 = row[0]
    thr = F32(thr)
    if not (r0 > F32(1e-10)) or max_lag < min_lag:
        return F32(0), 0, F32(0)
    v = [row[lag] / r0 if lag < len(row) else F32(0) for lag in range(min_lag, max_lag + 1)]
    first = -1
    for i in range(1, len(v) - 1):
        if v[i] > v[i - 1] and v[i] > v[i + 1] and v[i] > thr:
            first = min_lag + i
            break
    best = max(v)
    arg = min_lag + v.index(best)
    lag = first if first >= 0 else (arg if best > thr else -1)
    return (F32(sr) / F32(lag), 1, best) if lag > 0 else (F32(0), 0, best)


def _acf_rows(n_lag):
    rng = np.random.default_rng(12)
    rows = []
    base = np.full(n_lag, 0.05, F32)
    base[0] = 2.0
    a = base.copy(); a[6] = 0.9; a[12] = 1.5; rows.append(a)                    # first local maximum above thr (not the largest)
    b = base.copy(); b[2:21] = np.linspace(1.2, 0.3, 19); rows.append(b)        # monotone: no local, the global (at min_lag) above thr
    c = base.copy(); rows.append(c)                                              # nothing above thr
    d = base.copy(); d[8] = d[9] = 1.0; rows.append(d)                           # plateau: cur > prev false / cur > next false
    e = base.copy(); e[5] = 0.8; rows.append(e)                                  # the peak at lag 5 (min_lag == max_lag case)
    f = base.copy(); f[0] = 1e-11; rows.append(f)                                # r[0] <= 1e-10: silence
    g = base.copy(); g[0] = 0.0; rows.append(g)
    h = base.copy(); h[n_lag - 1] = 1.9; rows.append(h)                          # maximum on the last lag of the row
    i = base.copy(); i[4] = i[14] = 1.1; i[3] = i[5] = 1.1; rows.append(i)       # equal global maxima, plateau around the first
    j = -base.copy(); j[0] = 2.0; rows.append(j)                                 # all negative
    k = base.copy(); k[7] = 0.6000001; rows.append(k)                            # just above a threshold of 0.3
    rnd = rng.standard_normal((300 - len(rows), n_lag)).astype(F32)
    rnd[:, 0] = np.abs(rnd[:, 0]) + 1.0
    return np.concatenate([np.stack(rows), rnd])                                 # 300 rows: two workgroups


@pytest.mark.parametrize("min_lag,max_lag,thr", [(2, 20, 0.3), (5, 5, 0.3), (2, 40, 0.3), (9, 3, 0.3), (0, 10, 0.1),
                                                 (31, 31, 0.0), (30, 33, -1.0), (1, 2, 0.3)])
def test_acf_peak_rows_exact(min_lag, max_lag, thr):
    n_lag, sr = 32, 22050.0
    r = _acf_rows(n_lag)
    got = eb.acf_peaks(r, min_lag=min_lag, max_lag=max_lag, threshold=thr, sr=sr)
    want = [_acf_walk(row, min_lag, max_lag, thr, sr) for row in r]
    np.testing.assert_array_equal(got["f0"], np.array([w[0] for w in want], F32))
    np.testing.assert_array_equal(got["voiced"], np.array([w[1] for w in want], np.uint8))
    np.testing.assert_array_equal(got["periodicity"], np.array([w[2] for w in want], F32))
    for name in ("f0", "voiced", "periodicity"):                                # each output pointer NULL in turn
        rest = tuple(k for k in ("f0", "voiced", "periodicity") if k != name)
        part = eb.acf_peaks(r, min_lag=min_lag, max_lag=max_lag, threshold=thr, sr=sr, want=rest)
        assert set(part) == set(rest)
        for k in rest:
            np.testing.assert_array_equal(part[k], got[k])


def test_acf_peak_hand_rows_have_the_intended_answers():
    """The walk above applied to the hand-built rows gives what the rows were built for (the reference is not vacuous)."""
    r = _acf_rows(32)
    w = [_acf_walk(row, 2, 20, 0.3, 22050.0) for row in r[:11]]
    assert w[0][:2] == (F32(22050.0) / F32(6), 1) and w[0][2] == F32(1.5) / F32(2.0)
    assert w[1][:2] == (F32(22050.0) / F32(2), 1)
    assert w[2][1] == 0 and w[2][2] == F32(0.05) / F32(2.0)
    assert w[3][:2] == (F32(22050.0) / F32(8), 1)                                # no local maximum; the global one, first of the tie
    assert w[5] == (0, 0, 0) and w[6] == (0, 0, 0)
    assert w[7][1] == 0                                                          # lag 31 lies outside 2..20
    assert w[8][:2] == (F32(22050.0) / F32(14), 1)                               # 3-4-5 is a plateau; 14 is a strict local maximum
    assert w[9][1] == 0
    with pytest.raises(ValueError, match="negative lag"):
        eb.acf_peaks(r, min_lag=-1, max_lag=5, threshold=0.1, sr=1.0)


# ====================================================================================== signal extension
@pytest.mark.parametrize("mode", list(eb.EXT_MODES))
def test_extend_bit_exact(mode):
    from scipy.signal._upfirdn_apply import _pad_test
    rng = np.random.default_rng(11)
    for L, P in ((1000, 70), (5, 19), (2, 7), (333, 333), (3, 50), (4, 0)):
        x = rng.standard_normal((3, L)).astype(F32)
        for grid in (0, 2):
            got = eb.extend(x, P, mode, grid=grid)
            for b in range(3):
                np.testing.assert_array_equal(got[b], _pad_test(x[b], npre=P, npost=P, mode=mode))
                np.testing.assert_array_equal(got[b], ao.upfirdn_extend(x[b], P, mode))
    one = rng.standard_normal((2, 1)).astype(F32)
    if mode in ("smooth", "reflect", "antireflect", "line"):
        with pytest.raises(ValueError, match="at least two samples"):
            eb.extend(one, 3, mode)
    else:
        got = eb.extend(one, 3, mode)
        for b in range(2):
            np.testing.assert_array_equal(got[b], _pad_test(one[b], npre=3, npost=3, mode=mode))


# ====================================================================================== PCM16 ingest
@pytest.mark.parametrize("n", [1, 7, 8, 9, 1000, 4099])
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 0), (0, 1), (4, 2)])
def test_pcm16_exact(n, off_in, off_out):
    """off_in counts int16 samples, off_out floats: (0, 0) takes eight samples per thread, anything else one."""
    x = np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16)
    for i, v in enumerate((-32768, 32767, -1, 1, -2, 0, 255, -256)):
        if i < n:
            x[(i * 5) % n if n > 8 else i % n] = v
    x[-1] = -1
    want = x.astype(F32) * F32(1.0 / 32768.0)
    for grid in (0, 1):
        np.testing.assert_array_equal(eb.pcm16(x, off_in=off_in, off_out=off_out, grid=grid), want)
    np.testing.assert_array_equal(eb.pcm16(x, scale=1.0, off_in=off_in, off_out=off_out), x.astype(F32))


# ====================================================================================== autocorrelation glue
@pytest.mark.parametrize("n", [1, 255, 1000, 4099])
def test_row_mean_and_pad(n):
    y = (np.random.default_rng(n).standard_normal((3, n)) + 0.3).astype(F32)
    m = eb.row_mean(y)
    # a thread adds ceil(n / 256) terms in sequence, the tree adds 8 levels, then one division: first-order bound
    bound = (np.ceil(n / 256) + 9) * EPS32 * np.abs(y).astype(np.float64).mean(axis=1)
    assert (np.abs(m - y.astype(np.float64).mean(axis=1)) <= bound + 1e-45).all()
    N = int(eb.lib().emu_autocorrelation_nfft(n))
    for mean in (m, None):
        for grid in (0, 1):
            p = eb.autocorr_pad(y, N, mean, grid=grid)
            np.testing.assert_array_equal(p[:, :n], y - (m[:, None] if mean is not None else F32(0)))
            assert (p[:, n:] == 0).all()


def test_power_spectrum_and_finish():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((3, 700, 2)).astype(F32)
    for grid in (0, 2):
        P = eb.power_spectrum(X, grid=grid)
        # two products and a sum, or one product and a fused multiply-add: at most two roundings apart
        np.testing.assert_allclose(P[..., 0], X[..., 0].astype(np.float64) ** 2 + X[..., 1].astype(np.float64) ** 2,
                                   rtol=2 * EPS32, atol=0)
        assert (P[..., 1] == 0).all()
    r = rng.standard_normal((3, 64)).astype(F32)
    r[:, 0] = [5.0, 0.0, 1e-12]                              # r[0] = 0 and below the floor: divided by 1e-10
    for grid in (0, 1):
        np.testing.assert_array_equal(eb.autocorr_finish(r, 40, False, grid=grid), r[:, :40])
        np.testing.assert_array_equal(eb.autocorr_finish(r, 40, True, grid=grid),
                                      r[:, :40] / np.maximum(r[:, :1], F32(1e-10)))
    np.testing.assert_array_equal(eb.autocorr_finish(r, 64, True), r / np.maximum(r[:, :1], F32(1e-10)))


@pytest.mark.parametrize("n,kw", [(300, dict()), (300, dict(normalize=False, center=False)), (1, dict()),
                                  (513, dict(max_lag=100))])
def test_autocorrelation_end_to_end(n, kw):
    """The launch sequence of ap_autocorrelation_f32 - mean, pad, two forward legs of the four-step FFT, power, two
    inverse legs, finish - with the tolerance of test_gpu_next_rows.test_autocorrelation."""
    y = (np.random.default_rng(n).standard_normal((2, n)) + 0.3).astype(F32)
    max_lag = kw.pop("max_lag", n)
    got = eb.autocorrelation(y, max_lag, **kw)
    want = ao.autocorrelation(y, max_lag=max_lag, **kw)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * max(float(np.abs(want).max()), 1.0))


# ====================================================================================== last: the LDS guard
def test_lds_guard_clean_and_alive():
    """No launch of this file wrote past the dynamic LDS its host code asked for, and the guard would have seen it."""
    assert eb.lds_overruns() == 0
    assert eb.guard_selftest() == 1
    assert eb.lds_overruns() == 0
