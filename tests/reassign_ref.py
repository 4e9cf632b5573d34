"""The reassigned spectrogram of DESIGN.md 9.15 in NumPy: float64 (the reference), or float32 (`dtype`: NumPy 2 transforms
float32 input in float32) as the twin whose own error calibrates the bound.

Bound per element: |d Im(S_dh / S_h)| <= m (E_dh + |S_dh / S_h| E_h) / |S_h|, E_x = 2^-24 log2(n) ||frame w_x||_2, the same form
with E_th for Re(S_th / S_h).  m = 4 x the worst ratio the float32 twin reaches against the bound with m = 1 over the cases of
test_gpu_reassign.py (the margin for another, equally valid float32 summation order).  Measured twin ratios, worst case per n_fft:

    n_fft   frequency   time
    2048      0.69      0.67
     512      0.34      0.29
     400      0.38      0.33
      77      0.49      0.29
      27      0.40      0.38
"""

import numpy as np

import mlx_audio_primitives_amd as ap

M_FREQ = {2048: 4 * 0.69, 512: 4 * 0.34, 400: 4 * 0.38, 77: 4 * 0.49, 27: 4 * 0.40}
M_TIME = {2048: 4 * 0.67, 512: 4 * 0.29, 400: 4 * 0.33, 77: 4 * 0.29, 27: 4 * 0.38}


def tables(window, win_length, n_fft):
    """h centre-padded to n_fft, dh, th: float64 arithmetic on the float32 window, rounded to float32."""
    h = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    h[left:left + win_length] = ap.get_window(window, win_length, device="cpu").numpy()
    tau = np.arange(0.5 - n_fft // 2, n_fft // 2) if n_fft % 2 == 0 else np.arange(-(n_fft // 2), n_fft // 2 + 1)
    return h.astype(np.float32), ((np.roll(h, -1) - np.roll(h, 1)) / 2).astype(np.float32), (h * tau).astype(np.float32)


def signal(L, n_fft, hop, sr=22050, head=None, batch=1, ref_power=1e-6):
    """Noise (sigma 0.3) + a 1 kHz tone + one click of height 5; the first `head` (n_fft) samples exactly zero; the last three
    hops scaled down so that |S_h| of the last frame straddles sqrt(ref_power)."""
    rng = np.random.default_rng(L + n_fft)
    y = 0.3 * rng.standard_normal((batch, L)) + 0.2 * np.sin(2 * np.pi * 1000.0 * np.arange(L) / sr)
    y[:, (L * 2) // 3] += 5.0
    y[:, :n_fft if head is None else head] = 0.0
    y[:, L - 3 * hop:] *= 1.2 * np.sqrt(max(ref_power, 1e-6)) / (0.3 * np.sqrt(0.1875 * n_fft))
    return y.astype(np.float32)


def reference(y, sr=22050, n_fft=2048, hop=None, win_length=None, window="hann", center=True, pad_mode="constant", ref_power=1e-6,
              fill_nan=False, clip=True, rf=True, rt=True, dtype=np.float64):
    """dict: freqs, times, mags (B, F, T); the quotients qf = S_dh / S_h, qt = S_th / S_h; E_h, E_dh, E_th (B, 1, T)."""
    win_length = win_length or n_fft
    hop = hop or win_length // 4
    y = np.atleast_2d(y).astype(dtype)
    L = y.shape[1]
    if center:
        y = np.pad(y, ((0, 0), (n_fft // 2, n_fft // 2)), mode=pad_mode)
    T = 1 + (y.shape[1] - n_fft) // hop
    frames = np.stack([y[:, t * hop:t * hop + n_fft] for t in range(T)], axis=1)               # (B, T, n)
    S, E = [], []
    for w in tables(window, win_length, n_fft):
        fw = frames * w.astype(dtype)
        S.append(np.fft.rfft(fw, axis=-1).transpose(0, 2, 1))
        E.append(2.0 ** -24 * np.log2(n_fft) * np.linalg.norm(fw.astype(np.float64), axis=-1)[:, None, :])
    mags = np.abs(S[0])
    with np.errstate(all="ignore"):
        qf, qt = S[1] / S[0], S[2] / S[0]
    bin_f = (np.arange(n_fft // 2 + 1) * sr / n_fft)[None, :, None]
    frame_t = ((np.arange(T) * hop + (0 if center else n_fft // 2)) / sr)[None, None, :]
    bad = (mags < np.sqrt(ref_power)) | (S[0] == 0)
    freqs = np.where(bad, np.nan, bin_f - qf.imag * sr / (2 * np.pi)) if rf else np.broadcast_to(bin_f, mags.shape)
    times = np.where(bad, np.nan, frame_t + qt.real / sr) if rt else np.broadcast_to(frame_t, mags.shape)
    if fill_nan:
        freqs, times = np.where(np.isnan(freqs), bin_f, freqs), np.where(np.isnan(times), frame_t, times)
    lim = (sr / 2, L / sr) if clip else (np.inf, np.inf)
    return dict(freqs=freqs, times=times, mags=mags, qf=qf, qt=qt, E_h=E[0], E_dh=E[1], E_th=E[2], bad=bad, lim=lim,
                bin_f=bin_f, frame_t=frame_t, ref_power=ref_power)


def quotient_bounds(r):
    """(bound of Im qf, bound of Re qt) with m = 1, and the mask of the bins no comparison is made at."""
    thr_gap = (r["ref_power"] > 0) & (np.abs(r["mags"] - np.sqrt(r["ref_power"])) <= 8 * r["E_h"])   # no threshold, no gap
    with np.errstate(all="ignore"):
        bf = (r["E_dh"] + np.abs(r["qf"]) * r["E_h"]) / r["mags"]
        bt = (r["E_th"] + np.abs(r["qt"]) * r["E_h"]) / r["mags"]
    return bf, bt, thr_gap | ((r["mags"] < 64 * r["E_h"]) & ~r["bad"])
