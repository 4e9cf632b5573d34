"""Time-frequency reassigned spectrogram (librosa 0.10 ``reassigned_spectrogram``).

Three STFTs of the same frames - with the window, its derivative and its time-weighted copy - are formed
on chip by one kernel (csrc/kernels_reassign.h) that writes only the three float planes; this file keeps
the argument handling and the window tables.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _extension as _x
from .stft import _WindowCache, _frame_count, _get_padded_window, _get_twiddles, _resolve_stft_args

_FLAG_FREQ, _FLAG_TIME, _FLAG_FILL, _FLAG_CLIP = 1, 2, 4, 8      # include/audioprims.h

_table_cache = _WindowCache()


def _derivative_tables_host(h: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(dh, th) of a centre-padded window h, float64 arithmetic, float32 results:
    dh[i] = (h[i+1] - h[i-1]) / 2 cyclically, th[i] = h[i] tau[i]."""
    h = np.asarray(h, dtype=np.float64)
    n = h.shape[0]
    dh = (np.roll(h, -1) - np.roll(h, 1)) / 2.0
    tau = np.arange(0.5 - n // 2, n // 2) if n % 2 == 0 else np.arange(-(n // 2), n // 2 + 1)
    return dh.astype(np.float32), (h * tau).astype(np.float32)


def _get_reassign_tables(window, win_length: int, n_fft: int, device):
    """(h, dh, th) on `device`, built once per (window, win_length, n_fft, device)."""
    key = _WindowCache._key(window, win_length, n_fft, device)
    hit = _table_cache.get(key)
    if hit is None:
        h = _get_padded_window(window, win_length, n_fft, device)
        dh, th = _derivative_tables_host(h.detach().cpu().numpy())
        hit = (h, torch.from_numpy(dh).to(device), torch.from_numpy(th).to(device))
        _table_cache.put(key, hit)
    return hit


def reassigned_spectrogram(y, *, sr: float = 22050, S=None, n_fft: int = 2048, hop_length: int | None = None,
                           win_length: int | None = None, window="hann", center: bool = True,
                           reassign_frequencies: bool = True, reassign_times: bool = True, ref_power=1e-6,
                           fill_nan: bool = False, clip: bool = True, dtype=None, pad_mode: str = "constant"):
    """Reassigned spectrogram of y, (samples,) or (batch, samples): returns (freqs, times, mags), float32
    tensors of shape (n_fft//2+1, n_frames) or (batch, n_fft//2+1, n_frames).

    With S_h, S_dh, S_th the STFTs (frames and padding as `stft`) with the window h, its cyclic central
    difference dh and h times the sample offset from the frame's centre:
      mags = |S_h|;  freqs = k sr / n_fft - Im(S_dh / S_h) sr / (2 pi);
      times = (t hop + (0 if center else n_fft // 2)) / sr + Re(S_th / S_h) / sr.
    freqs and times are NaN where mags < sqrt(ref_power), and wherever S_h is 0 - also where NumPy, dividing
    a non-zero S_dh or S_th by an exact zero, would give an infinity: we return NaN there on purpose.  With
    `fill_nan` a NaN becomes the bin frequency (the frame time); with `clip` freqs is then clipped to
    [0, sr / 2] and times to [0, len(y) / sr].  With reassign_frequencies=False (reassign_times=False) that
    plane is the broadcast bin frequency (frame time) and its transform is never run.
    Not served here: a precomputed `S`, a callable `ref_power`, a dtype other than float32."""
    if S is not None:
        raise ValueError("reassigned_spectrogram: a precomputed S is not supported, pass the audio y")
    if callable(ref_power):
        raise ValueError("reassigned_spectrogram: a callable ref_power is not supported, pass a number")
    if ref_power < 0:
        raise ValueError(f"ref_power must be non-negative, got {ref_power}")
    if not reassign_frequencies and not reassign_times:
        raise ValueError("reassign_frequencies or reassign_times must be True")
    if dtype is not None and dtype is not torch.float32 and np.dtype(dtype) != np.float32:
        raise ValueError(f"reassigned_spectrogram returns float32, got dtype={dtype}")
    if not sr > 0:
        raise ValueError(f"sr must be positive, got {sr}")
    hop_length, win_length = _resolve_stft_args(n_fft, hop_length, win_length)
    y = _x.to_device_f32(y)
    one_d = y.ndim == 1
    if one_d:
        y = y[None, :]
    if y.ndim != 2:
        raise ValueError(f"y must be 1D or 2D, got {y.ndim}D")
    B, L = y.shape
    dev = y.device
    T = _frame_count(L, n_fft, hop_length, center, pad_mode)
    F = n_fft // 2 + 1
    h, dh, th = _get_reassign_tables(window, win_length, n_fft, dev)
    tw = _get_twiddles(n_fft, dev)
    mags = torch.empty((B, F, T), dtype=torch.float32, device=dev)
    freqs = torch.empty_like(mags) if reassign_frequencies else None
    times = torch.empty_like(mags) if reassign_times else None
    flags = (_FLAG_FREQ if reassign_frequencies else 0) | (_FLAG_TIME if reassign_times else 0) \
        | (_FLAG_FILL if fill_nan else 0) | (_FLAG_CLIP if clip else 0)
    _x.check(_x.dlib(dev).ap_reassign_f32(
        _x.ptr(y), B, L, int(n_fft), hop_length, _x.ptr(h), _x.ptr(dh) if reassign_frequencies else None,
        _x.ptr(th) if reassign_times else None, _x.ptr(tw), int(bool(center)), _x.PAD_MODES[pad_mode], T, float(sr),
        float(ref_power), flags, _x.ptr(freqs) if reassign_frequencies else None,
        _x.ptr(times) if reassign_times else None, _x.ptr(mags), T, _x.stream_ptr(dev)))
    if freqs is None:          # the bin frequencies, broadcast (never written by the kernel)
        grid = (np.arange(F, dtype=np.float64) * float(sr) / n_fft).astype(np.float32)
        freqs = torch.from_numpy(grid).to(dev)[None, :, None].expand(B, F, T).contiguous()
    if times is None:          # the frame times, broadcast
        grid = ((np.arange(T, dtype=np.float64) * hop_length + (0 if center else n_fft // 2)) / float(sr)).astype(np.float32)
        times = torch.from_numpy(grid).to(dev)[None, None, :].expand(B, F, T).contiguous()
    if one_d:
        return freqs[0], times[0], mags[0]
    return freqs, times, mags
