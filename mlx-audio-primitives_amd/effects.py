"""Time and pitch effects (no counterpart in the reference; the signatures of librosa 0.10's phase_vocoder,
effects.time_stretch and effects.pitch_shift).

phase_vocoder is one kernel (csrc/kernels_pv.h).  librosa accumulates a phase per bin,
acc += phi + wrap(angle(D[i+1]) - angle(D[i]) - phi), and emits mag exp(j acc); wrap only removes multiples of 2 pi, so
exp(j acc) is the running product of the unit phasors u[i+1] conj(u[i]), u = D / |D|, and the expected advance phi,
which is all that hop_length and n_fft feed, drops out of the result.  The kernel forms that product as a wave-wide
scan, without atan2 / sin / cos; in float32 the product keeps 1e-6 of max |D| over thousands of steps where the angle
recurrence loses all digits after a few hundred.

Deviation from librosa, on purpose: a bin that is -0.0 + 0j counts as zero (phase 0), where NumPy's angle is pi.
"""

from __future__ import annotations

import inspect
import math

import numpy as np
import torch

from . import _extension as _x
from .resample import _resample_fft_length
from .stft import _LINES_N_FFT, _padded_row_stride, _spectrum_layout, istft, stft

_ISTFT_KWARGS = frozenset(inspect.signature(istft).parameters) - {"stft_matrix", "length"}


def _rate(rate) -> float:
    if isinstance(rate, bool) or not isinstance(rate, (int, float, np.integer, np.floating)) \
            or not float(rate) > 0.0 or not math.isfinite(float(rate)):
        raise ValueError("rate must be a positive number")
    return float(rate)


def _positive_int(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return int(v)


def phase_vocoder(D, *, rate, hop_length=None, n_fft=None) -> torch.Tensor:
    """Speed an STFT up by `rate` (librosa.phase_vocoder).

    D: complex (F, T) or (batch, F, T), a tensor or an array; a line-padded view (what `stft` returns) is read in
    place.  Returns complex64 (…, F, T_out), T_out = len(np.arange(0, T, rate)); column k is taken at position k rate:
    the magnitudes of the two columns around it interpolated linearly, the phase advanced by the phase step between
    them.  For n_fft = 2048 / 512 / 400 / 256 spectra the result is a view of rows padded to 16 frames (under `stft`'s
    "lines" layout), which `istft` reads in place.

    hop_length, n_fft: accepted for librosa's signature and validated, otherwise unused: they only set the expected
    phase advance, which cancels out of the result (see the module docstring)."""
    rate = _rate(rate)
    if hop_length is not None:
        _positive_int(hop_length, "hop_length")
    if n_fft is not None:
        _positive_int(n_fft, "n_fft")
    if not isinstance(D, torch.Tensor):
        D = torch.as_tensor(np.asarray(D))
    if not D.is_complex():
        raise ValueError(f"D must be complex, got {D.dtype}")
    if D.ndim not in (2, 3):
        raise ValueError(f"D must be 2D or 3D, got {D.ndim}D")
    two_d = D.ndim == 2
    if two_d:
        D = D[None]
    dev = D.device if D.is_cuda else _x.require_device()
    lib = _x.lib()
    S = D.to(device=dev, dtype=torch.complex64)
    B, F, T = S.shape
    T_out = int(lib.ap_phase_vocoder_frames(T, rate))
    if T_out < 0:
        raise ValueError(f"phase_vocoder: {T} frames at rate {rate} are too many")
    Ts = T_out
    if 2 * (F - 1) in _LINES_N_FFT and _spectrum_layout() == "lines" and T_out % 16 and T_out < 490000 - 16:
        Ts = -(-T_out // 16) * 16               # (no size threshold as in `stft`: the padding costs this kernel nothing)
    out = torch.empty((B, F, Ts, 2), dtype=torch.float32, device=dev)
    if B * F * T_out:
        rs = _padded_row_stride(S)
        if rs is None:
            S = S.contiguous()
            rs = T
        _x.check(_x.dlib(dev).ap_phase_vocoder_f32(_x.ptr(torch.view_as_real(S)), B * F, T, rs, rate, T_out, _x.ptr(out), Ts,
                                                   _x.stream_ptr(dev)))
    out = torch.view_as_complex(out)[:, :, :T_out]
    return out[0] if two_d else out


def time_stretch(y, *, rate, **kwargs) -> torch.Tensor:
    """Change the speed of y (samples,) or (batch, samples) by `rate` without changing its pitch
    (librosa.effects.time_stretch): stft(y, **kwargs), phase_vocoder, istft to round(len / rate) samples with the
    keyword arguments `istft` shares with `stft`."""
    rate = _rate(rate)
    y = _x.to_device_f32(y)
    D = stft(y, **kwargs)
    D = phase_vocoder(D, rate=rate, hop_length=kwargs.get("hop_length"), n_fft=kwargs.get("n_fft"))
    return istft(D, length=int(round(y.shape[-1] / rate)), **{k: v for k, v in kwargs.items() if k in _ISTFT_KWARGS})


def pitch_shift(y, *, sr, n_steps, bins_per_octave: int = 12, res_type: str = "fft", scale: bool = False, **kwargs) -> torch.Tensor:
    """Shift the pitch of y by n_steps steps of an octave cut in bins_per_octave (librosa.effects.pitch_shift):
    time_stretch by rate = 2^(-n_steps / bins_per_octave), then resample from sr / rate to sr (scipy.signal.resample to
    ceil(len rate) samples), cropped or zero-padded to len(y).  scale=True divides by sqrt(rate), as librosa's resample
    does.  res_type: only "fft"; the package's other resamplers do not take a non-integer ratio."""
    if isinstance(sr, bool) or not isinstance(sr, (int, float, np.integer, np.floating)) or not float(sr) > 0.0:
        raise ValueError(f"sr must be strictly positive, got {sr!r}")
    _positive_int(bins_per_octave, "bins_per_octave")
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, float, np.integer, np.floating)) or not math.isfinite(float(n_steps)):
        raise ValueError(f"n_steps must be a finite number, got {n_steps!r}")
    if res_type != "fft":
        raise ValueError(f"res_type={res_type!r} cannot resample at a non-integer ratio here; use \"fft\"")
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    y = _x.to_device_f32(y)
    n = y.shape[-1]
    out = time_stretch(y, rate=rate, **kwargs)
    n_out = int(math.ceil(out.shape[-1] * rate))
    if n_out != out.shape[-1]:
        out = _resample_fft_length(out, n_out)
    if scale:
        out = out / np.float32(math.sqrt(rate))
    if n_out > n:
        out = out[..., :n]
    elif n_out < n:
        out = torch.nn.functional.pad(out, (0, n - n_out))
    return out.contiguous()


__all__ = ["phase_vocoder", "time_stretch", "pitch_shift"]
