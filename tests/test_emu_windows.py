"""CPU: every transform kernel that takes a window, run from its source on the SIMT emulator of tests/emu with
windows that are NOT a periodic Hann (tests/window_cases.py: a rough array in [0.25, 1], "boxcar", a short rough
window with an odd zero-pad), against the oracle.

Hann hides what these windows show: its first and last weights are ~0 (a frame's edge samples taken from the
wrong place go unseen), it is mirror-symmetric (an i <-> N - i slip in a window copy goes unseen), and its
overlap-add envelope vanishes at the ends of a non-centred stream (the existing inverse tests mask those samples).
Here every output sample is compared; each inverse test first asserts from the float64 envelope alone that
sum w^2 >= 0.0625 (>= 1 for boxcar) over the compared span.

Bars (the project's own): STFT and mel rtol = atol = 1e-4; ISTFT against the oracle rtol = 1e-4, atol = 1e-5;
round trip to the signal 1e-5 max abs.  The spectral statistics keep the bars of
test_emu_spectral_statistics_from_audio.

How far a plain float32 CPU transform (torch.stft / torch.fft.irfft + the oracle's overlap-add) sits from the
oracle on these very cases, as the worst |error| / (atol + rtol |reference|) per family, all three windows:
  STFT (all engines, stft16 included)            0.080
  mel (all kernels)                              0.011
  ISTFT of a signal's STFT, against the oracle   0.075 (fused 0.072, istft16 0.052, irfft + overlap-add 0.042, stream 0.075)
  ISTFT of a random spectrum, against the oracle 0.009
  round trip to the signal, against 1e-5         0.12
None exceeds half its bar, so no family needed a bar of its own.
"""

import os
import sys

import numpy as np
import pytest

from oracle import audio_oracle as ao

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_bind as eb  # noqa: E402
import emu_istft_stream_bind as esb  # noqa: E402
import window_cases as wc  # noqa: E402

PM = {"constant": 0, "edge": 1, "reflect": 2}
KINDS = wc.KINDS


def signal(B, L, seed):
    return np.random.default_rng(seed).standard_normal((B, L)).astype(np.float32)


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)


# ---- forward ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_fft,hop,L,B,pad_mode,center", wc.EMU_STFT_CASES)
def test_emu_stft_windows(n_fft, hop, L, B, pad_mode, center, kind):
    """ap_stft2048_wave_kernel, ap_stft1024_wave_kernel, ap_stft8_wave_kernel<25 / 32 / 16> and the generic engine."""
    w = wc.make_window(kind, n_fft)
    y = signal(B, L, n_fft + hop)
    S = eb.stft(y, n_fft, hop, w.padded, center, PM[pad_mode])
    R = ao.stft(y, n_fft=n_fft, hop_length=hop, win_length=w.win_length, window=w.arg, center=center, pad_mode=pad_mode)
    assert S.shape == R.shape
    close(S, R)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop,L,B,pad_mode,center,Ts,grid_cap,misalign,force_unaligned", wc.EMU_STFT16_CASES)
def test_emu_stft16_windows(hop, L, B, pad_mode, center, Ts, grid_cap, misalign, force_unaligned, kind):
    """kernels_stft16.h, dense and padded rows, the carry path and the whole-group tile."""
    w = wc.make_window(kind, 2048)
    y = signal(B, L, hop + L)
    S, raw, off, aligned = eb.stft16(y, hop, w.padded, center, PM[pad_mode], Ts, grid_cap, misalign, force_unaligned)
    R = ao.stft(y, n_fft=2048, hop_length=hop, win_length=w.win_length, window=w.arg, center=center, pad_mode=pad_mode)
    assert S.shape == R.shape
    close(S, R)
    T = R.shape[-1]
    Tr = T if Ts is None else Ts
    n = B * 1025 * Tr
    assert np.all(raw[:off] == -777.0) and np.all(raw[off + 2 * n:] == -777.0)
    assert np.all(raw[off:off + 2 * n].reshape(B, 1025, Tr, 2)[:, :, T:] == -777.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop,L,B,pad_mode,center,grid_cap", [
    (512, 10753, 3, "constant", True, 2), (512, 11300, 2, "constant", False, 1), (512, 9001, 2, "reflect", True, 3),
    (255, 5000, 2, "constant", True, 2)])
def test_emu_stft16_gl_windows(hop, L, B, pad_mode, center, grid_cap, kind):
    """kernels_stft16.h with the Griffin-Lim projection in its store phase (GL = 1 and GL = 2): the raw spectrum."""
    w = wc.make_window(kind, 2048)
    rng = np.random.default_rng(hop + L)
    y = rng.standard_normal((B, L)).astype(np.float32)
    R = ao.stft(y, n_fft=2048, hop_length=hop, win_length=w.win_length, window=w.arg, center=center, pad_mode=pad_mode)
    prev = (rng.standard_normal(R.shape) + 1j * rng.standard_normal(R.shape)).astype(np.complex64)
    mag = rng.random(R.shape).astype(np.float32)
    outs = []
    for variant in (1, 2):
        raw, reb, _, _ = eb.stft16_gl(y, hop, w.padded, prev, mag, 0.99, center=center, pad_mode=PM[pad_mode],
                                      grid_cap=grid_cap, variant=variant)
        assert raw.shape == R.shape
        close(raw, R)
        unit = lambda z: z / np.maximum(np.abs(z), 1e-30)  # noqa: E731
        P = mag * unit(raw.astype(np.complex128))
        np.testing.assert_allclose(reb, P + 0.99 * (P - mag * unit(prev.astype(np.complex128))), rtol=2e-3, atol=2e-3)
        outs.append((raw, reb))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_fft,sr,M,hop,L,B,power,pad_mode,center", wc.EMU_MEL_CASES)
def test_emu_mel_windows(n_fft, sr, M, hop, L, B, power, pad_mode, center, kind):
    """The fused mel kernel of each n_fft (2048 run kernel, wave512, frames8 at 400 / 512 / 256) and the kernel it
    replaces (2048 tile kernel, compile-time LDS engine)."""
    w = wc.make_window(kind, n_fft)
    y = signal(B, L, n_fft + M + hop)
    fb = ao.mel_filterbank(sr, n_fft, M)
    R = ao.melspectrogram(y, sr=sr, n_fft=n_fft, hop_length=hop, win_length=w.win_length, window=w.arg, n_mels=M,
                          power=power, center=center, pad_mode=pad_mode)
    A, amax = eb.melspec(y, n_fft, hop, w.padded, fb, center=center, pad_mode=PM[pad_mode], power=power, return_max=True)
    assert A.shape == R.shape
    close(A, R)
    assert amax == A.max()
    if n_fft != 1024:                      # (the n_fft = 1024 kernel has no second engine behind this flag)
        A2 = eb.melspec(y, n_fft, hop, w.padded, fb, center=center, pad_mode=PM[pad_mode], power=power, tile_kernel=True)
        close(A2, R)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hop,L,B,center", [(512, 20001, 2, True), (300, 9001, 2, True), (512, 6001, 3, False),
                                            (333, 7001, 2, False)])
def test_emu_spectral_from_audio_windows(hop, L, B, center, kind):
    """ap_spec2048_run_kernel: it has no index-remapping loader, so constant padding only, and an odd hop only
    without centring."""
    w = wc.make_window(kind, 2048)
    rng = np.random.default_rng(hop + L)
    t = np.arange(L) / 22050.0
    y = (0.5 * np.sin(2 * np.pi * 440.0 * t)[None] + 0.05 * rng.standard_normal((B, L))).astype(np.float32)
    kw = dict(sr=22050, n_fft=2048, hop_length=hop, win_length=w.win_length, window=w.arg, center=center)
    got = eb.spectral_from_audio(y, 22050, hop, w.padded, center=center)
    for b in range(B):
        np.testing.assert_allclose(got["centroid"][b], ao.spectral_centroid(y[b], **kw)[0], rtol=2e-4, atol=1e-2)
        np.testing.assert_allclose(got["bandwidth"][b], ao.spectral_bandwidth(y[b], **kw)[0], rtol=2e-4, atol=1e-2)
        off = np.abs(got["rolloff"][b] - ao.spectral_rolloff(y[b], **kw)[0]) / (22050 / 2048)
        assert off.max() <= 1.001 and (off > 0.5).mean() < 0.02


# ---- inverse ---------------------------------------------------------------------------------------------------------

def inverse_inputs(n_fft, hop, L, B, w, center, seed):
    """(name, spectrum, signal or None): the STFT of a signal, and a random spectrum of the same shape."""
    y = signal(B, L, seed)
    S = ao.stft(y, n_fft=n_fft, hop_length=hop, win_length=w.win_length, window=w.arg, center=center)
    return [("stft", S, y), ("random", wc.spectrum(B, n_fft, S.shape[-1], seed + 1), None)]


def centers(kind):
    return (True,) if kind == "short" else (True, False)


def lengths(name, n_fft, hop, T, L, center):
    """`length` arguments of one (input, centring) pair: between them the four pairs cover the natural span, a longer
    centred output (the whole signal) and a shorter one with and without centring."""
    natural = (T - 1) * hop + (0 if center else n_fft)
    if name == "stft":
        return (L, natural - 333) if center else (None,)
    return (None,) if center else (natural - 333,)


def check_inverse(run, n_fft, hop, L, B, kind, seed):
    """run(S, center, out_len) -> (B, out_len) from the kernel under test; every sample against the oracle's istft,
    and against the signal where the spectrum is a signal's STFT."""
    w = wc.make_window(kind, n_fft)
    for center in centers(kind):
        for name, S, y in inverse_inputs(n_fft, hop, L, B, w, center, seed):
            T = S.shape[-1]
            for length in lengths(name, n_fft, hop, T, L, center):
                lo, hi = wc.istft_span(n_fft, hop, T, center, length)
                wc.assert_envelope_floor(w, n_fft, hop, T, lo, hi)
                want = ao.istft(S, hop_length=hop, win_length=w.win_length, n_fft=n_fft, window=w.arg, center=center,
                                length=length)
                got = run(S, center, hi - lo)
                assert got.shape == want.shape, (name, center, length)
                np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg=f"{name} center={center} length={length}")
                if y is not None:
                    n = min(hi - lo, L)
                    assert np.max(np.abs(got[:, :n] - y[:, :n])) < 1e-5, (name, center, length)


def short_ok(kind, n_fft, hop):
    return kind != "short" or 2 * hop <= wc.short_length(n_fft)


def with_kinds(cases, n_fft_of, hop_of):
    return [c + (k,) for c in cases for k in KINDS if short_ok(k, n_fft_of(c), hop_of(c))]


@pytest.mark.parametrize("n_fft,hop,L,B,grid_cap,kind",
                         with_kinds(wc.EMU_ISTFT_FUSED_CASES, lambda c: c[0], lambda c: c[1]))
def test_emu_istft_fused_windows(n_fft, hop, L, B, grid_cap, kind):
    """ap_irfft2048_wave_kernel<1>, ap_istft1024_wave_kernel, ap_istft8_wave_kernel<32 / 25 / 16>."""
    w = wc.make_window(kind, n_fft)
    run = lambda S, center, n: eb.istft_fused(S, hop, w.padded, n, out_offset=n_fft // 2 if center else 0,  # noqa: E731
                                              grid_cap=grid_cap)
    check_inverse(run, n_fft, hop, L, B, kind, n_fft + hop + L)


@pytest.mark.parametrize("hop,L,B,grid_cap,Ts,variant,kind",
                         with_kinds(wc.EMU_ISTFT16_CASES, lambda c: 2048, lambda c: c[0]))
def test_emu_istft16_windows(hop, L, B, grid_cap, Ts, variant, kind):
    """kernels_istft16.h, every variant, dense and padded rows; the clip-start and `emit && clip_last` tail samples
    of a non-centred clip are compared like any other."""
    w = wc.make_window(kind, 2048)
    run = lambda S, center, n: eb.istft16(S, hop, w.padded, n, out_offset=1024 if center else 0,  # noqa: E731
                                          grid_cap=grid_cap, Ts=Ts, variant=variant)
    check_inverse(run, 2048, hop, L, B, kind, hop + L)


@pytest.mark.parametrize("n_fft,hop,L,B,kind", with_kinds(wc.EMU_ISTFT_UNFUSED_CASES, lambda c: c[0], lambda c: c[1]))
def test_emu_irfft_overlap_add_windows(n_fft, hop, L, B, kind):
    """ap_irfft2048_wave_kernel<0> / ap_irfft8_wave_kernel / the generic irfft, then ap_overlap_add_kernel."""
    w = wc.make_window(kind, n_fft)
    run = lambda S, center, n: eb.overlap_add(eb.irfft_frames(S, n_fft), w.padded, hop, n,  # noqa: E731
                                              out_offset=n_fft // 2 if center else 0)
    check_inverse(run, n_fft, hop, L, B, kind, n_fft + L)


def run_stream(S, n_fft, hop, w, chunks, center, G=2):
    st = esb.Stream(n_fft, hop, w.padded, center=center, G=G)
    outs, t = [], 0
    for c in chunks:
        outs.append(st.process(S[:, :, t:t + c]))
        t += c
    assert t == S.shape[2]
    outs.append(st.flush())
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_fft,hop,chunkings", wc.EMU_STREAM_CASES)
def test_emu_istft_stream_windows(n_fft, hop, chunkings, kind):
    """kernels_istft_stream.h: the start-of-stream and final envelopes included, bit-equal over the chunkings."""
    if not short_ok(kind, n_fft, hop):
        hop = wc.SHORT_HOP[n_fft]
    w = wc.make_window(kind, n_fft)
    K = sum(chunkings[0])
    for center in centers(kind):
        L = (K - 1) * hop + (0 if center else n_fft)
        for name, S, y in inverse_inputs(n_fft, hop, L, 2, w, center, n_fft + hop):
            assert S.shape[-1] == K
            lo, hi = wc.istft_span(n_fft, hop, K, center, None)
            wc.assert_envelope_floor(w, n_fft, hop, K, lo, hi)
            ys = [run_stream(S, n_fft, hop, w, ch, center) for ch in chunkings]
            for ch, got in zip(chunkings[1:], ys[1:]):
                assert np.array_equal(got, ys[0]), (name, center, ch)
            want = ao.istft(S, hop_length=hop, win_length=w.win_length, n_fft=n_fft, window=w.arg, center=center)
            assert ys[0].shape == want.shape
            np.testing.assert_allclose(ys[0], want, rtol=1e-4, atol=1e-5, err_msg=f"{name} center={center}")
            if y is not None:
                assert np.max(np.abs(ys[0] - y[:, :hi - lo])) < 1e-5, (name, center)
    assert esb.lib().emu_istft_stream_lds_overruns() == 0


def test_zz_no_kernel_wrote_past_its_dynamic_lds():
    """Runs last in this file (see test_emu_kernels.py)."""
    assert eb.lds_overruns() == 0
