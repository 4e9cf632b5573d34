"""Chunked (streaming) STFT / mel front end and its inverse (the reference only
lists "Streaming support - process audio in chunks" as future work, ARCHITECTURE.md:537-540).

A stream is framed WITHOUT centring: frame t covers samples [t*hop, t*hop + n_fft) of the
concatenation of every chunk fed so far.  Each ``process(chunk)`` call returns exactly the frames the
new samples complete, computed by the same fused kernels as the offline calls, so concatenating the
outputs over any chunking equals ``stft(whole, center=False)`` / ``melspectrogram(whole,
center=False)`` bit for bit; only the n_fft - hop (or fewer) samples that later frames still need stay
in HBM between calls.  ``center=True`` semantics are obtained by feeding n_fft//2 zeros first and
calling ``flush()`` (which pads n_fft//2 zeros) at the end.

``StreamingISTFT`` is the synthesis half: spectrum frames fed in chunks come back as the samples they
finish, bit-identical over any chunking and equal to the offline ``istft`` of all frames; the unnormalised
overlap-add tail (n_fft - hop samples per stream) stays in HBM between calls (ap_istft_stream_f32).
"""

from __future__ import annotations

import numpy as np
import torch

from . import _extension as _x
from .mel import melspectrogram
from .onset import _spectrum
from .pcen import _axes as _pcen_axes, _parameters as _pcen_parameters, _run as _pcen_run
from .stft import _get_padded_window, _get_twiddles, _padded_row_stride, _resolve_stft_args, stft


class StreamingSTFT:
    """Incremental ``stft(..., center=False)``: feed (samples,) or (batch, samples) chunks."""

    def __init__(self, n_fft: int = 2048, hop_length: int | None = None, win_length: int | None = None,
                 window="hann", center: bool = False, **mel_kwargs):
        self.n_fft = int(n_fft)
        self.hop_length, self.win_length = _resolve_stft_args(self.n_fft, hop_length, win_length)
        self.window = window
        self.center = bool(center)
        self._mel = dict(mel_kwargs) if mel_kwargs else None      # n_mels=..., sr=..., power=... -> mel frames
        self._tail = None                                          # (B, < n_fft) samples not yet consumed
        self._one_d = None
        self._started = False
        self.frames_emitted = 0

    # -- internals ---------------------------------------------------------------------------------
    def _transform(self, y):
        if self._mel is not None:
            return melspectrogram(y, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length,
                                  window=self.window, center=False, **self._mel)
        return stft(y, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length,
                    window=self.window, center=False)

    def _empty(self, B, device):
        if self._mel is not None:
            n_rows = int(self._mel.get("n_mels", 128))
            return torch.empty((B, n_rows, 0), dtype=torch.float32, device=device)
        return torch.empty((B, self.n_fft // 2 + 1, 0), dtype=torch.complex64, device=device)

    def process(self, chunk) -> torch.Tensor:
        """Feed the next samples; returns the newly completed frames, (F|M, T_new) or (B, F|M, T_new)
        (T_new may be 0)."""
        chunk = _x.to_device_f32(chunk)
        if self._one_d is None:
            self._one_d = chunk.ndim == 1
        if chunk.ndim == 1:
            chunk = chunk[None, :]
        if chunk.ndim != 2:
            raise ValueError(f"chunk must be 1D or 2D, got {chunk.ndim}D")
        if not self._started and self.center:                      # the left half of the centre padding
            chunk = torch.nn.functional.pad(chunk, (self.n_fft // 2, 0))
        self._started = True
        buf = chunk if self._tail is None else torch.cat([self._tail, chunk], dim=1)
        if self._tail is not None and buf.shape[0] != self._tail.shape[0]:
            raise ValueError("every chunk must have the same batch size")
        n = buf.shape[1]
        T = 0 if n < self.n_fft else 1 + (n - self.n_fft) // self.hop_length
        if T == 0:
            self._tail = buf.contiguous()
            out = self._empty(buf.shape[0], buf.device)
        else:
            used = (T - 1) * self.hop_length + self.n_fft
            out = self._transform(buf[:, :used].contiguous())
            self._tail = buf[:, T * self.hop_length:].contiguous()
            self.frames_emitted += T
        return out[0] if self._one_d else out

    def flush(self) -> torch.Tensor:
        """End of stream.  center=True: pad the right half (n_fft//2 zeros) and emit the last frames;
        center=False: nothing is pending (a partial frame is dropped, as offline)."""
        if self._tail is None:
            raise ValueError("flush() before any chunk")
        if not self.center:
            return self._empty(self._tail.shape[0], self._tail.device)[0] if self._one_d else \
                self._empty(self._tail.shape[0], self._tail.device)
        pad = torch.zeros((self._tail.shape[0], self.n_fft // 2), dtype=torch.float32, device=self._tail.device)
        one_d, self._one_d = self._one_d, False
        self.center = False                                        # the padding is explicit from here on
        out = self.process(pad)
        self._one_d, self.center = one_d, True
        return out[0] if one_d else out

    def reset(self) -> None:
        self._tail, self._one_d, self._started, self.frames_emitted = None, None, False, 0


class StreamingISTFT:
    """Incremental ``istft``: feed (F, T) or (B, F, T) spectrum chunks (T may be 0), get the samples they finish.

    After K frames every sample p < K*hop is final, so ``process`` returns the samples the chunk finished
    ((n,) or (B, n), possibly n = 0) and ``flush()`` the pending n_fft - hop, normalised with the end-of-stream
    envelope.  The concatenation equals ``istft(S_all, center=center)`` (no ``length``: trim it yourself);
    ``center=True`` drops n_fft//2 samples at the start and at the flush.  The carry lives in two device
    buffers used in turn; nothing is synchronised and nothing is read back."""

    def __init__(self, n_fft: int = 2048, hop_length: int | None = None, win_length: int | None = None,
                 window="hann", center: bool = False):
        self.n_fft = int(n_fft)
        self.hop_length, self.win_length = _resolve_stft_args(self.n_fft, hop_length, win_length)
        self.window = window
        self.center = bool(center)
        if self.center and self.hop_length > self.n_fft - self.n_fft // 2:
            raise ValueError(f"center=True needs hop_length <= n_fft - n_fft//2 = {self.n_fft - self.n_fft // 2}, "
                             f"got {self.hop_length}")
        self.reset()

    def reset(self) -> None:
        """Forget the stream: the next chunk starts a new one (any batch size)."""
        self._carry = None                  # [in, out]: (B, n_fft - hop) partial sums, swapped after every call
        self._B = None
        self._one_d = None
        self._device = None
        self._flushed = False
        self.frames_consumed = 0
        self.samples_emitted = 0

    # -- internals ---------------------------------------------------------------------------------
    def _trim(self) -> int:
        return self.n_fft // 2 if self.center else 0

    def _run(self, S, T: int, final: bool) -> torch.Tensor:
        n, hop, dev, B = self.n_fft, self.hop_length, self._device, self._B
        frame0 = self.frames_consumed
        K = frame0 + T
        lo = max(frame0 * hop, self._trim())
        hi = (K - 1) * hop + n - self._trim() if final else K * hop
        hi = max(hi, lo)
        out = torch.empty((B, hi - lo), dtype=torch.float32, device=dev)
        if self._carry is None:
            self._carry = [torch.empty((B, max(n - hop, 1)), dtype=torch.float32, device=dev) for _ in range(2)]
        win = _get_padded_window(self.window, self.win_length, n, dev)
        tw = _get_twiddles(n, dev)
        if S is not None:
            row_stride = _padded_row_stride(S)
            n_ws = int(_x.lib().ap_istft_stream_workspace_floats(B, T, n, hop))
            if row_stride is None or n_ws:
                S = S.contiguous()
                row_stride = T
            ws = torch.empty(n_ws, dtype=torch.float32, device=dev) if n_ws else None
            s_ptr = _x.ptr(torch.view_as_real(S))
        else:
            row_stride, ws, s_ptr = 0, None, None
        _x.check(_x.dlib(dev).ap_istft_stream_f32(
            s_ptr, B, T, row_stride, n, hop, _x.ptr(win), _x.ptr(tw), frame0, _x.ptr(self._carry[0]),
            _x.ptr(self._carry[1]), int(final), lo, hi, None if ws is None else _x.ptr(ws), _x.ptr(out),
            _x.stream_ptr(dev)))
        self._carry.reverse()
        self.frames_consumed = K
        self.samples_emitted += hi - lo
        return out[0] if self._one_d else out

    def process(self, S_chunk) -> torch.Tensor:
        """Feed the next frames (complex (F, T) or (B, F, T), dense or a strided view, on the device or the
        host); returns the samples they finish, (n,) or (B, n)."""
        if self._flushed:
            raise ValueError("process() after flush(): call reset() to start a new stream")
        S = S_chunk if isinstance(S_chunk, torch.Tensor) else torch.as_tensor(np.asarray(S_chunk))
        if S.ndim not in (2, 3):
            raise ValueError(f"S_chunk must be 2D or 3D, got {S.ndim}D")
        one_d = S.ndim == 2
        if one_d:
            S = S[None]
        B, F, T = S.shape
        if F != self.n_fft // 2 + 1:
            raise ValueError(f"S_chunk has {F} frequency bins but n_fft={self.n_fft} needs {self.n_fft // 2 + 1}")
        if self._B is None:
            self._B, self._one_d = B, one_d
            self._device = S.device if S.is_cuda else _x.require_device()
        elif B != self._B or one_d != self._one_d:
            raise ValueError(f"every chunk must have the same batch layout: got {tuple(S_chunk.shape)} after "
                             f"{'(F, T)' if self._one_d else f'({self._B}, F, T)'} chunks")
        S = S.to(device=self._device, dtype=torch.complex64)
        if T == 0:
            e = torch.empty((B, 0), dtype=torch.float32, device=self._device)
            return e[0] if one_d else e
        return self._run(S, T, final=False)

    def flush(self) -> torch.Tensor:
        """End of stream: the last n_fft - hop samples (fewer with center=True), normalised with the envelope of
        the frames actually fed.  The stream is finished afterwards (reset() starts a new one)."""
        if self._flushed:
            raise ValueError("flush() called twice: call reset() to start a new stream")
        if self.frames_consumed == 0:
            raise ValueError("flush() before any frame")
        out = self._run(None, 0, final=True)
        self._flushed = True
        return out


class StreamingPCEN:
    """Incremental ``pcen``: feed (M, T) or (batch, M, T) spectrogram chunks (the mel frames of a ``StreamingSTFT``,
    scaled as the model expects); every row's filter state (zf) stays on the device between calls, so the chunks
    equal the offline call on all frames to rounding, whatever the chunking.  Takes the parameters of ``pcen``;
    ``zi`` is the state the stream (and every ``reset()``) starts from.  max_size > 1 is allowed: the maximum runs
    over bins, not time.  ref= is not taken: a reference array has no streaming counterpart."""

    def __init__(self, *, sr: float = 22050, hop_length: int = 512, gain: float = 0.98, bias: float = 2,
                 power: float = 0.5, time_constant: float = 0.400, eps: float = 1e-6, b=None, max_size: int = 1,
                 axis: int = -1, max_axis=None, zi=None):
        self.b, self.gain, self.bias, self.power, self.eps, self.max_size = _pcen_parameters(
            sr, hop_length, gain, bias, power, time_constant, eps, b, max_size, axis, max_axis, zi is not None)
        self._axis, self._max_axis = int(axis), None if max_axis is None else int(max_axis)
        self._zi = zi
        self.reset()

    def reset(self) -> None:
        """Forget the kept state: the next chunk starts a new stream."""
        self._state = self._zi
        self._shape = None
        self.frames_consumed = 0

    def process(self, S_chunk) -> torch.Tensor:
        """Feed the next frames; returns their normalised values, of the chunk's shape."""
        S, two_d = _spectrum(S_chunk, "S_chunk")
        _pcen_axes(S.ndim, self._axis, self._max_axis, self.max_size)
        lead = tuple(S.shape[:-1])
        if self._shape is None:
            self._shape = lead
        elif lead != self._shape:
            raise ValueError(f"every chunk must have the same leading shape: got {lead} after {self._shape}")
        if S.shape[-1] == 0:                                      # nothing to do, the state stays
            dev = S.device if S.is_cuda else _x.require_device()
            return torch.empty(S.shape, dtype=torch.float32, device=dev)
        out, self._state = _pcen_run(S, two_d, None, self._state, True, self.b, self.gain, self.bias, self.power,
                                     self.eps, self.max_size)
        self.frames_consumed += int(S.shape[-1])
        return out
