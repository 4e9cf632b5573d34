"""GPU: the public transforms with windows that are NOT a periodic Hann (tests/window_cases.py: a rough array in
[0.25, 1], "boxcar", a short rough window with an odd zero-pad), against the oracle, one small shape per dispatch
branch of ap_stft_f32 / ap_stft_rows_f32 / ap_melspec_rows_f32 / ap_istft_f32 / ap_istft_rows_f32 /
ap_istft_stream_f32 (audioprims.hip; the branch is named in each case's comment).  Why these windows:
test_emu_windows.py, which runs the same kernels from source on the CPU.

Every output sample is compared: no mask, no slice, no relaxed region.  Each inverse test first asserts from the
float64 envelope alone that sum w^2 >= 0.0625 (>= 1 for boxcar) over the compared span.  Bars: STFT and mel
rtol = atol = 1e-4; ISTFT against the oracle rtol = 1e-4, atol = 1e-5; round trip to the signal 1e-5 max abs.

A plain float32 CPU transform (torch.stft / torch.fft.irfft + the oracle's overlap-add) sits this far from the
oracle on this module's cases, as the worst |error| / (atol + rtol |reference|) over the three windows: STFT 0.093,
mel 0.014, ISTFT of a signal's STFT 0.12, of a random spectrum 0.007, round trip against 1e-5 0.13, streaming shapes
0.055 / 0.007 / 0.12.  None is near half its bar, so every family keeps the project's bar.

The A/B environment switches (AP_STFT2048_G8, AP_MEL2048_WAVE, AP_STFT8_CT) are read once per process: the kernels
behind them are left to the emulator module."""

import importlib
import os
import sys

import numpy as np
import pytest

from oracle import audio_oracle as ao

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mlx_audio_primitives_amd as ap  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_cases as wc  # noqa: E402
from test_gpu_istft_stream import SHAPES as STREAM_SHAPES  # noqa: E402

stft_mod = importlib.import_module("mlx_audio_primitives_amd.stft")
windows_mod = importlib.import_module("mlx_audio_primitives_amd.windows")

KINDS = wc.KINDS


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def signal(B, L, seed):
    return np.random.default_rng(seed).standard_normal((B, L)).astype(np.float32)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    assert ap.HAS_HIP_EXT
    yield
    torch.cuda.synchronize()


def wkw(w):
    return dict(window=w.arg, win_length=w.win_length)


# ---- stft ------------------------------------------------------------------------------------------------------------

STFT_CASES = [   # n_fft, hop, B, L, pad_mode, padded rows expected (centred, not centred)
    (2048, 512, 2, 20001, "constant", (False, False)),    # ap_launch_stft16, dense rows: carried 128-byte windows
    (2048, 441, 2, 20001, "constant", (False, False)),    # ... odd hop: index-remapped loads for the centred frames
    (2048, 512, 14, 22050, "constant", (True, True)),     # ap_stft_rows_f32 -> ap_launch_stft16: T = 44 / 40 on rows of 48
    (2048, 512, 2, 9001, "reflect", (False, False)),      # ap_launch_stft16, index-remapped edge frames
    (1024, 256, 2, 10001, "constant", (False, False)),    # ap_stft1024_wave_kernel<0>
    (1024, 300, 2, 10001, "constant", (False, False)),    # ... a hop that is no divisor of n_fft
    (1024, 255, 2, 6001, "constant", (False, False)),     # ap_stft1024_wave_kernel<1> when centred (odd hop)
    (512, 128, 2, 8001, "constant", (False, False)),      # ap_launch_stft8<32>, dense
    (512, 128, 9, 8001, "constant", (True, True)),        # ap_stft_rows_f32 -> ap_launch_stft8<32>: T = 63 / 59 on rows of 64
    (400, 160, 2, 8200, "constant", (False, False)),      # ap_launch_stft8<25>, dense
    (400, 160, 11, 8200, "constant", (True, True)),       # ... rows: T = 52 / 49 on rows of 64
    (256, 64, 2, 4001, "constant", (False, False)),       # ap_launch_stft8<16>, dense
    (256, 64, 9, 4001, "constant", (True, True)),         # ... rows: T = 63 / 59 on rows of 64
    # reflect / edge at n_fft = 512: the PADGEN instantiation ap_stft8_wave_kernel<32, 1> (the compile-time engine
    # of kernels_ct.h is behind it and only takes over past 2^19 frames or under AP_STFT8_CT)
    (512, 128, 2, 4001, "reflect", (False, False)),
    (512, 100, 2, 4001, "edge", (False, False)),
    (154, 30, 2, 2001, "constant", (False, False)),       # ap_stft_generic_kernel<0>, mixed radix 2 * 7 * 11
    (4096, 1024, 2, 20001, "constant", (False, False)),   # ap_stft_generic_kernel<0>, 16 * 16 * 16
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n_fft,hop,B,L,pad_mode,rows", STFT_CASES)
def test_stft_windows(n_fft, hop, B, L, pad_mode, rows, center, kind):
    w = wc.make_window(kind, n_fft)
    y = signal(B, L, n_fft + hop + B)
    S = ap.stft(dev(y), n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode, **wkw(w))
    want = ao.stft(y, n_fft=n_fft, hop_length=hop, center=center, pad_mode=pad_mode, **wkw(w))
    assert S.shape == want.shape
    lines = rows[0 if center else 1] and stft_mod._spectrum_layout() == "lines"
    assert (stft_mod._padded_row_stride(S) is not None) == lines                          # the branch the case names
    np.testing.assert_allclose(host(S), want, rtol=1e-4, atol=1e-4)


# ---- melspectrogram --------------------------------------------------------------------------------------------------

MEL_CASES = [
    dict(sr=22050, n_fft=2048, hop_length=512, n_mels=128, power=2.0),      # ap_launch_mel_run<2>
    dict(sr=22050, n_fft=2048, hop_length=512, n_mels=128, power=1.0),      # ap_launch_mel_run<1>
    dict(sr=22050, n_fft=2048, hop_length=300, n_mels=128, power=2.0),      # run kernel, full reload per frame
    dict(sr=22050, n_fft=2048, hop_length=512, n_mels=128, power=2.0, pad_mode="reflect"),   # ap_launch_mel_run<2, 2>
    dict(sr=22050, n_fft=2048, hop_length=512, n_mels=128, power=1.5),      # ap_prepare_mel_wave: the tile kernel
    dict(sr=22050, n_fft=1024, hop_length=256, n_mels=80, power=2.0),       # ap_mel1024_wave_kernel<2, 2, 0>
    dict(sr=22050, n_fft=1024, hop_length=200, n_mels=64, power=1.0),       # ap_mel1024_wave_kernel<1, 0, 0>
    dict(sr=16000, n_fft=400, hop_length=160, n_mels=80, power=2.0),        # ap_launch_mel8<25>
    dict(sr=22050, n_fft=512, hop_length=128, n_mels=64, power=2.0),        # ap_launch_mel8<32>
    dict(sr=8000, n_fft=256, hop_length=64, n_mels=32, power=1.0),          # ap_launch_mel8<16>
    dict(sr=22050, n_fft=1024, hop_length=256, n_mels=160, power=2.0),      # > 128 filters: off the wave kernels (ct / generic)
    dict(sr=22050, n_fft=2048, hop_length=512, n_mels=160, power=2.0),      # > 128 filters at 2048: the tile kernel
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("kw", MEL_CASES)
def test_melspectrogram_windows(kw, center, kind):
    w = wc.make_window(kind, kw["n_fft"])
    y = signal(2, 20001, kw["n_fft"] + kw["n_mels"])
    got = ap.melspectrogram(dev(y), center=center, **kw, **wkw(w))
    want = ao.melspectrogram(y, center=center, **kw, **wkw(w))
    assert got.shape == want.shape
    np.testing.assert_allclose(host(got), want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("center", [True, False])
def test_melspectrogram_windows_padded_rows_and_pcm16(center, kind):
    """ap_melspec_rows_f32 with row_stride != T (B T >= 512, T % 8 != 0), and int16 PCM on the fused n_fft = 2048
    route, where the register-resident window carries the 1 / 32768 scale."""
    w = wc.make_window(kind, 2048)
    kw = dict(sr=22050, n_fft=2048, hop_length=512, n_mels=128, center=center, **wkw(w))
    y = signal(14, 22050 if center else 24069, 5)                 # T = 44 either way
    got = ap.melspectrogram(dev(y), **kw)
    assert got.shape[-1] == 44 and got.is_contiguous() == (stft_mod._spectrum_layout() != "lines")
    np.testing.assert_allclose(host(got), ao.melspectrogram(y, **kw), rtol=1e-4, atol=1e-4)
    x = np.clip(np.random.default_rng(16).standard_normal((3, 20000)) * 6000.0, -32768, 32767).astype(np.int16)
    got = ap.melspectrogram(dev(x), **kw)
    np.testing.assert_allclose(host(got), ao.melspectrogram(x.astype(np.float32) / 32768.0, **kw), rtol=1e-4, atol=1e-4)


# ---- istft -----------------------------------------------------------------------------------------------------------

ISTFT_CASES = [   # n_fft, hop, B, L, line-padded input
    (2048, 512, 16, 20001, False),     # ap_istft_fused_shape (80 groups >= 64): ap_launch_istft16, dense rows
    (2048, 256, 16, 10001, False),
    (2048, 1024, 16, 40001, False),
    (2048, 512, 2, 20001, False),      # below the threshold: ap_irfft_frames_f32 (wave) + ap_overlap_add_f32
    (2048, 512, 3, 20001, True),       # ap_istft_rows_f32 -> ap_launch_istft16, rows of 48
    (2048, 256, 2, 10001, True),
    (2048, 1024, 2, 40001, True),
    (1024, 256, 16, 10001, False),     # ap_istft1024_fused_shape: ap_istft1024_wave_kernel
    (1024, 128, 16, 5001, False),
    (1024, 512, 16, 20001, False),
    (1024, 256, 2, 10001, False),      # below the threshold: generic irfft + overlap-add
    (512, 128, 2, 8001, False),        # ap_istft8_wave_kernel<32>
    (512, 128, 2, 8001, True),         # ap_istft_rows_f32 -> ap_istft8_wave_kernel<32>
    (400, 160, 2, 8200, False),        # ap_istft8_wave_kernel<25>
    (400, 100, 2, 8200, True),
    (256, 64, 2, 4001, False),         # ap_istft8_wave_kernel<16>
    (256, 64, 2, 4001, True),
    (64, 16, 2, 2001, False),          # unfused: generic irfft + ap_overlap_add_kernel
]


def line_padded(S):
    """S (B, F, T) as a view of a buffer whose rows are padded to a multiple of 16 frames, the padding filled
    with values no kernel may use."""
    B, F, T = S.shape
    Ts = -(-T // 16) * 16 + (16 if T % 16 == 0 else 0)
    buf = torch.full((B, F, Ts), 7e3, dtype=torch.complex64, device=S.device)
    buf[:, :, :T] = S
    v = buf[:, :, :T]
    assert stft_mod._padded_row_stride(v) == Ts
    return v


def istft_cases():
    out = []
    for c in ISTFT_CASES:
        for kind in KINDS:
            n_fft, hop = c[0], c[1]
            if kind == "short" and 2 * hop > wc.short_length(n_fft):
                if (n_fft, hop) == (400, 160):
                    c = (400, 100) + c[2:]       # the short window's hop at n_fft = 400
                else:
                    continue
            out.append(c + (kind,))
    return out


@pytest.mark.parametrize("n_fft,hop,B,L,lines,kind", istft_cases())
def test_istft_windows(n_fft, hop, B, L, lines, kind):
    w = wc.make_window(kind, n_fft)
    for center in ((True,) if kind == "short" else (True, False)):
        T = 1 + (L + (n_fft if center else 0) - n_fft) // hop
        Lc = L if center else (T - 1) * hop + n_fft          # without centring nothing lies beyond the last frame
        y = signal(B, Lc, n_fft + hop + B)
        S_sig = ao.stft(y, n_fft=n_fft, hop_length=hop, center=center, **wkw(w))
        assert S_sig.shape[-1] == T
        for name, S in (("stft", S_sig), ("random", wc.spectrum(B, n_fft, T, n_fft + hop))):
            Sd = line_padded(dev(S)) if lines else dev(S)
            for length in (None, Lc, Lc - 999):
                lo, hi = wc.istft_span(n_fft, hop, T, center, length)
                wc.assert_envelope_floor(w, n_fft, hop, T, lo, hi)
                got = host(ap.istft(Sd, hop_length=hop, n_fft=n_fft, center=center, length=length, **wkw(w)))
                want = ao.istft(S, hop_length=hop, n_fft=n_fft, center=center, length=length, **wkw(w))
                assert got.shape == want.shape
                np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg=f"{name} center={center} length={length}")
                if name == "stft":
                    n = min(hi - lo, Lc)
                    assert np.max(np.abs(got[:, :n] - y[:, :n])) < 1e-5, (center, length)


# ---- streaming -------------------------------------------------------------------------------------------------------

K = 40
CHUNKINGS = [[K], [0, 5, 1, 17, 0, 2, 15]]


def stream(S, n_fft, hop, w, chunks, center):
    st = ap.StreamingISTFT(n_fft=n_fft, hop_length=hop, center=center, **wkw(w))
    outs, t = [], 0
    for c in chunks:
        outs.append(st.process(S[..., t:t + c]))
        t += c
    outs.append(st.flush())
    assert st.frames_consumed == S.shape[-1]
    return torch.cat(outs, dim=-1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_fft,hop", STREAM_SHAPES)
def test_streaming_istft_windows(n_fft, hop, kind):
    """ap_istft_stream_f32, the start-of-stream and final envelopes included."""
    if kind == "short" and 2 * hop > wc.short_length(n_fft):
        hop = wc.SHORT_HOP[n_fft]
    w = wc.make_window(kind, n_fft)
    for center in ((True,) if kind == "short" else (False, True)):
        lo, hi = wc.istft_span(n_fft, hop, K, center, None)
        wc.assert_envelope_floor(w, n_fft, hop, K, lo, hi)
        S = wc.spectrum(3, n_fft, K, n_fft + hop)
        ys = [stream(dev(S), n_fft, hop, w, ch, center) for ch in CHUNKINGS]
        assert torch.equal(ys[1], ys[0])
        off = ap.istft(dev(S), hop_length=hop, n_fft=n_fft, center=center, **wkw(w))
        want = ao.istft(S, hop_length=hop, n_fft=n_fft, center=center, **wkw(w))
        assert ys[0].shape == off.shape == want.shape
        np.testing.assert_allclose(host(ys[0]), host(off), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(host(ys[0]), want, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_fft,hop", STREAM_SHAPES)
def test_streaming_stft_windows(n_fft, hop, kind):
    """StreamingSTFT under two chunkings, centred and not: the offline transform's bits, the oracle's values; its
    frames through StreamingISTFT give the signal back."""
    if kind == "short" and 2 * hop > wc.short_length(n_fft):
        hop = wc.SHORT_HOP[n_fft]
    w = wc.make_window(kind, n_fft)
    L = 39 * hop + n_fft // 2 + 17
    y = signal(3, L, n_fft + hop)
    for center in (False, True):
        whole = ap.stft(dev(y), n_fft=n_fft, hop_length=hop, center=center, **wkw(w))
        np.testing.assert_allclose(host(whole), ao.stft(y, n_fft=n_fft, hop_length=hop, center=center, **wkw(w)),
                                   rtol=1e-4, atol=1e-4)
        for cuts in ([0, L], [0, 100, 2500, 2501, n_fft + 2600, L]):
            st = ap.StreamingSTFT(n_fft=n_fft, hop_length=hop, center=center, **wkw(w))
            got = torch.cat([st.process(dev(y[:, a:b])) for a, b in zip(cuts[:-1], cuts[1:])] + [st.flush()], dim=-1)
            assert got.shape == whole.shape
            assert torch.equal(torch.view_as_real(got), torch.view_as_real(whole.contiguous()))
        if center:
            T = whole.shape[-1]
            lo, hi = wc.istft_span(n_fft, hop, T, True, None)
            wc.assert_envelope_floor(w, n_fft, hop, T, lo, hi)
            yr = stream(got, n_fft, hop, w, [7, T - 7], True)
            assert yr.shape == (3, hi - lo)
            assert np.max(np.abs(host(yr) - y[:, :hi - lo])) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kw", [dict(sr=22050, n_fft=2048, hop_length=512, n_mels=80),
                                dict(sr=16000, n_fft=400, hop_length=160, n_mels=40, power=1.0),
                                dict(sr=22050, n_fft=1024, hop_length=256, n_mels=64)])
def test_streaming_mel_windows(kw, kind):
    """StreamingSTFT(n_mels=...) equals the offline melspectrogram bit for bit, which matches the oracle."""
    w = wc.make_window(kind, kw["n_fft"])
    y = signal(2, 30001, kw["n_mels"])
    for center in (False, True):
        whole = ap.melspectrogram(dev(y), center=center, **kw, **wkw(w))
        np.testing.assert_allclose(host(whole), ao.melspectrogram(y, center=center, **kw, **wkw(w)), rtol=1e-4, atol=1e-4)
        st = ap.StreamingSTFT(center=center, **kw, **wkw(w))
        got = torch.cat([st.process(dev(y[:, a:a + 7000])) for a in range(0, 30001, 7000)] + [st.flush()], dim=-1)
        assert got.shape == whole.shape
        assert torch.equal(got, whole.contiguous())


# ---- one call each ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_griffinlim_iter_windows(kind):
    """griffinlim_iter against the oracle's (the bars of test_griffinlim_iter_matches_oracle), n_fft = 2048: the
    fused ISTFT and the STFT with the projection in its store phase."""
    w = wc.make_window(kind, 2048)
    rng = np.random.default_rng(9)
    y = rng.standard_normal((2, 20001)).astype(np.float32)
    S = np.abs(ao.stft(y, n_fft=2048, hop_length=512, **wkw(w))).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, S.shape).astype(np.float32)
    tprev = (S * np.exp(1j * rng.uniform(-np.pi, np.pi, S.shape))).astype(np.complex64)
    a, r, e = ap.griffinlim_iter(dev(S), dev(ang), 512, w.win_length, 2048, window=w.arg, momentum=0.99, tprev=dev(tprev))
    ra, rr, re = ao.griffinlim_iter(S, ang, 512, w.win_length, 2048, window=w.arg, momentum=0.99, tprev=tprev)
    np.testing.assert_allclose(float(e), float(re), rtol=1e-4)
    strong = np.abs(host(r)) > 1e-3
    np.testing.assert_allclose(np.exp(1j * host(a))[strong], np.exp(1j * ra)[strong], atol=2e-3)
    np.testing.assert_allclose(host(r), rr, rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("kind", KINDS)
def test_spectral_statistics_from_audio_windows(kind):
    """spectral_centroid / spectral_rolloff straight from audio (ap_spec2048_run_kernel), the bars of
    test_gpu_features.py."""
    w = wc.make_window(kind, 2048)
    rng = np.random.default_rng(4)
    L = 20001
    t = np.arange(L) / 22050.0
    y = (0.5 * np.sin(2 * np.pi * 440.0 * t)[None] + 0.05 * rng.standard_normal((2, L))).astype(np.float32)
    kw = dict(sr=22050, n_fft=2048, hop_length=512, **wkw(w))
    np.testing.assert_allclose(host(ap.spectral_centroid(dev(y), **kw)), ao.spectral_centroid(y, **kw), rtol=1e-4, atol=1e-2)
    got, want = host(ap.spectral_rolloff(dev(y), **kw)), ao.spectral_rolloff(y, **kw)
    assert got.shape == want.shape
    diff = np.abs(got - want)
    assert (diff <= (22050 / 2048) * 1.001).all() and (diff > 0).mean() <= 0.02


@pytest.mark.parametrize("kind", KINDS)
def test_mfcc_windows(kind):
    w = wc.make_window(kind, 2048)
    y = signal(2, 20001, 8)
    kw = dict(sr=22050, n_mfcc=13, n_fft=2048, hop_length=512, n_mels=128, **wkw(w))
    np.testing.assert_allclose(host(ap.mfcc(dev(y), **kw)), ao.mfcc(y, **kw), rtol=1e-4, atol=2e-3)


# ---- window handling -------------------------------------------------------------------------------------------------

def test_one_array_window_in_every_form_gives_the_same_bits():
    w = wc.rough_window(1024, seed=77)
    y = dev(signal(2, 10001, 1))
    base = ap.stft(y, n_fft=1024, hop_length=256, window=w)
    np.testing.assert_allclose(host(base), ao.stft(host(y), n_fft=1024, hop_length=256, window=w), rtol=1e-4, atol=1e-4)
    w2 = torch.zeros(2048, dtype=torch.float32, device="cuda")
    w2[::2] = dev(w)
    forms = dict(cpu=torch.from_numpy(w.copy()), device=dev(w), float64=dev(w.astype(np.float64)), view=w2[::2])
    assert not forms["view"].is_contiguous()
    for name, form in forms.items():
        stft_mod._padded_window_cache.clear()           # every form converts its own way, not through the first one's entry
        got = ap.stft(y, n_fft=1024, hop_length=256, window=form)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(base)), name
        m = ap.melspectrogram(y, n_fft=1024, hop_length=256, n_mels=64, window=form)
        assert torch.equal(m, ap.melspectrogram(y, n_fft=1024, hop_length=256, n_mels=64, window=w)), name


def test_array_window_written_after_use_does_not_change_the_cache():
    """The padded-window cache is keyed by the window's values: it must own what it stores, or a caller's later
    write to their tensor changes what every window with the old values hits."""
    y = dev(signal(2, 10001, 2))
    vals = wc.rough_window(2048, seed=123)
    want = ao.stft(host(y), window=vals)
    w = dev(vals)
    first = ap.stft(y, window=w).clone()
    np.testing.assert_allclose(host(first), want, rtol=1e-4, atol=1e-4)
    w.mul_(2)
    again = ap.stft(y, window=dev(vals))                  # a fresh tensor with the old values: a cache hit
    assert torch.equal(torch.view_as_real(again), torch.view_as_real(first))
    doubled = ap.stft(y, window=w)                        # the caller's tensor, now other values
    assert torch.equal(torch.view_as_real(doubled), torch.view_as_real(first) * 2)
    yr = ap.istft(first, window=dev(vals), length=10001)
    assert float((yr - y).abs().max()) < 1e-5


def test_named_window_written_by_the_caller_does_not_change_later_transforms():
    y = dev(signal(2, 10001, 3))
    want = ao.stft(host(y))
    try:
        g = ap.get_window("hann", 2048)
        np.testing.assert_array_equal(host(g), ao.get_window("hann", 2048))
        g.mul_(0)
        np.testing.assert_array_equal(host(ap.get_window("hann", 2048)), ao.get_window("hann", 2048))
        stft_mod._padded_window_cache.clear()             # stft builds its padded window anew from the named cache
        np.testing.assert_allclose(host(ap.stft(y)), want, rtol=1e-4, atol=1e-4)
        ap.get_window("hann", 2048).mul_(0)
        np.testing.assert_allclose(host(ap.stft(y)), want, rtol=1e-4, atol=1e-4)
    finally:                                              # a failure here must not spoil the window of later tests
        windows_mod._device_window_cache.clear()
        stft_mod._padded_window_cache.clear()


def test_two_array_windows_used_alternately_each_give_their_own_result():
    y = dev(signal(2, 10001, 4))
    wa, wb = wc.rough_window(512, seed=1), wc.rough_window(512, seed=2)
    ra, rb = (ao.stft(host(y), n_fft=512, hop_length=128, window=v) for v in (wa, wb))
    da, db = dev(wa), dev(wb)
    for _ in range(3):
        np.testing.assert_allclose(host(ap.stft(y, n_fft=512, hop_length=128, window=da)), ra, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(host(ap.stft(y, n_fft=512, hop_length=128, window=wb)), rb, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(host(ap.stft(y, n_fft=512, hop_length=128, window=wa)), ra, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(host(ap.stft(y, n_fft=512, hop_length=128, window=db)), rb, rtol=1e-4, atol=1e-4)
