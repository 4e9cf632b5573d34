"""Harmonic / percussive source separation by median filtering (no counterpart in the reference; the signatures
of librosa.decompose.hpss and librosa.effects.hpss / harmonic / percussive).

On M = |S|: `harm` is the running median of every row along time, `perc` of every column along frequency
(scipy.ndimage.median_filter with mode="reflect", bit for bit), and librosa's soft mask of one against the other
(times its margin) splits S.  One fused kernel per call (csrc/kernels_hpss.h): a comparator network
on registers for the default 31 x 31 windows, rank counting for every other size up to 255; the medians and masks
never reach HBM unless they are what is asked for.

Deviations from librosa, on purpose: the components are S * mask (librosa: |S| * mask * S / |S|, one rounding more,
the same zero at |S| = 0); non-negativity of a real S is not checked (a synchronising readback): results are defined
for finite, non-negative magnitudes.

`nmf` / `decompose` (librosa.decompose.decompose's signature): non-negative matrix factorisation by multiplicative
updates, Frobenius or Kullback-Leibler, up to 64 components, all iterations enqueued by one C call on float32
matrix-core kernels (csrc/kernels_nmf.h).  `decompose` stays the name of this module at the package's
top level; the function is `decompose.decompose`.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _extension as _x
from .stft import _padded_row_stride, istft, stft

_MODE_COMPONENTS, _MODE_MASKS, _MODE_MEDIANS = 0, 1, 2


def _kernel_sizes(kernel_size):
    pair = tuple(kernel_size) if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
    if len(pair) != 2 or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 255
                             for k in pair):
        raise ValueError(f"kernel_size must be an integer in 1 .. 255, or a (harmonic, percussive) pair of them, "
                         f"got {kernel_size!r}")
    return int(pair[0]), int(pair[1])


def _margins(margin):
    pair = tuple(margin) if isinstance(margin, (tuple, list)) else (margin, margin)
    if len(pair) != 2:
        raise ValueError(f"margin must be a number or a (harmonic, percussive) pair, got {margin!r}")
    if not all(float(m) >= 1.0 for m in pair):
        raise ValueError("Margins must be >= 1.0. A typical range is between 1 and 10.")
    return float(pair[0]), float(pair[1])


def _power(power):
    if not float(power) > 0.0:
        raise ValueError("power must be strictly positive")
    return float(power)


def _spectrum(S):
    """Validated (S as a torch tensor, was it 2D?) - still wherever the caller had it."""
    if not isinstance(S, torch.Tensor):
        S = torch.as_tensor(np.asarray(S))
    if S.ndim not in (2, 3):
        raise ValueError(f"S must be 2D or 3D, got {S.ndim}D")
    if S.dtype not in (torch.float32, torch.complex64):
        raise ValueError(f"S must be float32 or complex64, got {S.dtype}")
    return S, S.ndim == 2


def _run(S, kh, kp, mh, mp, power, mode, want_h=True, want_p=True, general=False):
    """One ap_hpss_f32 call on a validated 2D / 3D spectrum: (out_h, out_p), None for an output not asked for.
    `general` forces the rank-counting kernel (the cross-check of the network kernel)."""
    S, two_d = _spectrum(S)
    dev = S.device if S.is_cuda else _x.require_device()
    _x.lib()
    S = S.to(dev)
    if two_d:
        S = S[None]
    B, F, T = S.shape
    cplx = S.is_complex()
    cplx_out = cplx and mode == _MODE_COMPONENTS
    row_stride = _padded_row_stride(S) if B * F * T else None
    if row_stride is None:
        S = S.contiguous()
    rs_in = row_stride if row_stride is not None else T
    # line-padded complex rows in -> line-padded complex rows out (istft reads them in place); everything else dense
    rs_out = rs_in if cplx_out else T

    def alloc():
        if cplx_out and B * F * T:
            return torch.view_as_complex(torch.empty((B, F, rs_out, 2), dtype=torch.float32, device=dev))[:, :, :T]
        return torch.empty((B, F, T), dtype=torch.complex64 if cplx_out else torch.float32, device=dev)

    def raw(t):
        return _x.ptr(torch.view_as_real(t) if t.is_complex() else t)

    out_h = alloc() if want_h else None
    out_p = alloc() if want_p else None
    if B * F * T:
        _x.check(_x.dlib(dev).ap_hpss_f32(raw(S), int(cplx), B, F, T, rs_in, kh, kp, mh, mp, power, mode,
                                          int(bool(general)), None if out_h is None else raw(out_h),
                                          None if out_p is None else raw(out_p), rs_out, _x.stream_ptr(dev)))
    if two_d:
        out_h, out_p = (None if o is None else o[0] for o in (out_h, out_p))
    return out_h, out_p


def hpss(S, *, kernel_size=31, power: float = 2.0, mask: bool = False, margin=1.0):
    """Harmonic / percussive separation of a spectrum (librosa.decompose.hpss).

    S: (F, T) or (batch, F, T), real float32 (a magnitude) or complex64, dense or the line-padded view `stft`
    returns.  kernel_size and margin: a number or a (harmonic, percussive) pair; power: exponent of the soft mask
    (inf: hard mask).  Returns (harmonic, percussive) of S's dtype, or the two real masks with mask=True.  For a
    line-padded complex S the components are line-padded views of the same row stride, which `istft` reads in place."""
    kh, kp = _kernel_sizes(kernel_size)
    mh, mp = _margins(margin)
    power = _power(power)
    _spectrum(S)
    return _run(S, kh, kp, mh, mp, power, _MODE_MASKS if mask else _MODE_COMPONENTS)


def hpss_medians(S, *, kernel_size=31):
    """The two median filters of `hpss` alone: (harm, perc), real and dense; harm = the median of |S| over
    kernel_size[0] frames along time, perc over kernel_size[1] bins along frequency, both with SciPy's "reflect"
    boundary (equal to scipy.ndimage.median_filter in every bit)."""
    kh, kp = _kernel_sizes(kernel_size)
    _spectrum(S)
    return _run(S, kh, kp, 1.0, 1.0, 2.0, _MODE_MEDIANS)


def _audio(y, want_h, want_p, kernel_size, power, margin, n_fft, hop_length, win_length, window, center, pad_mode):
    kh, kp = _kernel_sizes(kernel_size)
    mh, mp = _margins(margin)
    power = _power(power)
    ndim = len(np.shape(y)) if not isinstance(y, torch.Tensor) else y.ndim
    if ndim not in (1, 2):
        raise ValueError(f"y must be 1D or 2D, got {ndim}D")
    L = int(y.shape[-1]) if hasattr(y, "shape") else len(y)
    S = stft(y, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=center,
             pad_mode=pad_mode)
    H, P = _run(S, kh, kp, mh, mp, power, _MODE_COMPONENTS, want_h, want_p)
    back = dict(hop_length=hop_length, win_length=win_length, n_fft=n_fft, window=window, center=center, length=L)
    return (None if H is None else istft(H, **back)), (None if P is None else istft(P, **back))


def hpss_audio(y, *, kernel_size=31, power: float = 2.0, margin=1.0, n_fft: int = 2048,
               hop_length: int | None = None, win_length: int | None = None, window="hann", center: bool = True,
               pad_mode: str = "constant"):
    """(y_harmonic, y_percussive) of a signal (samples,) or (batch, samples), each of y's length
    (librosa.effects.hpss): stft -> hpss -> istft of both components."""
    return _audio(y, True, True, kernel_size, power, margin, n_fft, hop_length, win_length, window, center, pad_mode)


def harmonic(y, *, kernel_size=31, power: float = 2.0, margin=1.0, n_fft: int = 2048,
             hop_length: int | None = None, win_length: int | None = None, window="hann", center: bool = True,
             pad_mode: str = "constant"):
    """The harmonic part of a signal (librosa.effects.harmonic); the percussive component is neither masked nor stored."""
    return _audio(y, True, False, kernel_size, power, margin, n_fft, hop_length, win_length, window, center, pad_mode)[0]


def percussive(y, *, kernel_size=31, power: float = 2.0, margin=1.0, n_fft: int = 2048,
               hop_length: int | None = None, win_length: int | None = None, window="hann", center: bool = True,
               pad_mode: str = "constant"):
    """The percussive part of a signal (librosa.effects.percussive); the harmonic component is neither masked nor stored."""
    return _audio(y, False, True, kernel_size, power, margin, n_fft, hop_length, win_length, window, center, pad_mode)[1]


# ----------------------------------------------------------------------------------------------------------------------
# NMF by multiplicative updates (csrc/kernels_nmf.h)
# ----------------------------------------------------------------------------------------------------------------------
_BETA_LOSS = {"frobenius": 0, 2: 0, 2.0: 0, "kullback-leibler": 1, 1: 1, 1.0: 1}
MAX_COMPONENTS = 64                     # ap_nmf_max_components()
_TOL_BLOCK = 10                         # iterations between two looks at the objective (scikit-learn's)


def _factor(x, name, shapes, dev):
    """A given W / H as a float32 tensor of one of `shapes` (ValueError otherwise), on `dev` when there is one."""
    if x is None:
        raise ValueError(f"{name} must be given")
    x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if x.dtype != torch.float32 or tuple(x.shape) not in shapes:
        raise ValueError(f"{name} must be float32 of shape {' or '.join(map(str, shapes))}, got {x.dtype} {tuple(x.shape)}")
    return x if dev is None else x.to(dev)


def _nmf_args(S, n_components, beta_loss, max_iter, tol, init, W, H, update_components, eps):
    """Everything that can be refused without a device: (S, two_d, K, loss, init)."""
    S, two_d = _spectrum(S)
    if S.is_complex():
        raise ValueError("S must be real (a magnitude or power spectrum), got complex64")
    if 0 in S.shape:
        raise ValueError(f"S must be non-empty, got {tuple(S.shape)}")
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or not 1 <= n_components <= MAX_COMPONENTS:
        raise ValueError(f"n_components must be an integer in 1 .. {MAX_COMPONENTS}, got {n_components!r}")
    if beta_loss not in _BETA_LOSS:
        raise ValueError(f"beta_loss must be 'frobenius' or 'kullback-leibler', got {beta_loss!r}")
    if int(max_iter) < 0 or not float(tol) >= 0.0 or not float(eps) > 0.0:
        raise ValueError("max_iter and tol must be >= 0 and eps > 0")
    if init is None:
        init = "random" if update_components and W is None and H is None else "custom"
    if init not in ("random", "custom"):
        raise ValueError(f"init must be 'random' or 'custom', got {init!r}")
    B, F, T = (1,) + tuple(S.shape) if two_d else tuple(S.shape)
    K = int(n_components)
    lead = () if two_d else (B,)
    if not update_components or init == "custom":
        _factor(W, "W", [lead + (F, K)] if update_components else [(F, K), lead + (F, K)], None)
    if init == "custom":
        _factor(H, "H", [lead + (K, T)], None)
    return S, two_d, K, _BETA_LOSS[beta_loss], init


def nmf(S, n_components, *, beta_loss="frobenius", max_iter: int = 200, tol: float = 1e-4, init="random", W=None, H=None,
        update_components: bool = True, eps: float = 1e-10, random_state=None, return_n_iter: bool = False):
    """S ~ components @ activations by multiplicative updates (Lee and Seung; scikit-learn's solver="mu").

    S: (F, T) or (batch, F, T), real float32, dense or the line-padded view `magnitude(stft(..))` returns; results are
    defined for finite, non-negative S (not checked: that would be a synchronising readback).  Returns (components
    (.., F, K), activations (.., K, T)), K = n_components <= 64, and the number of iterations with return_n_iter.
    One iteration updates the activations, then the components from the new activations; beta_loss "frobenius" or
    "kullback-leibler".  init="random": sqrt(mean(S) / K) * |N(0, 1)| per item from a torch.Generator seeded with
    random_state; init="custom": W and H are the starting point (copied).  update_components=False keeps W, (F, K) for
    all items or (batch, F, K), as a fixed dictionary.  tol=0 runs exactly max_iter iterations with no readback;
    tol > 0 looks at the objectives of all items every 10 iterations and stops when (previous - current) / initial <
    tol for every one of them: all items of a batch run the same number of iterations."""
    S, two_d, K, loss, init = _nmf_args(S, n_components, beta_loss, max_iter, tol, init, W, H, update_components, eps)
    dev = S.device if S.is_cuda else _x.require_device()
    L = _x.dlib(dev)
    _x.lib()
    S = S.to(dev)
    if two_d:
        S = S[None]
    B, F, T = S.shape
    row_stride = _padded_row_stride(S)
    if row_stride is None:
        S, row_stride = S.contiguous(), T
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0 if random_state is None else int(random_state))
    scale = None

    def draw(*shape):
        nonlocal scale
        if scale is None:
            scale = torch.sqrt(S.mean(dim=(1, 2), keepdim=True) / K)
        return (scale * torch.randn(shape, generator=gen, dtype=torch.float32).abs().to(dev)).contiguous()

    lead = () if two_d else (B,)
    if not update_components:
        Wd = _factor(W, "W", [(F, K), lead + (F, K)], dev).reshape(-1, F, K).expand(B, F, K).contiguous().clone()
    elif init == "custom":
        Wd = _factor(W, "W", [lead + (F, K)], dev).reshape(B, F, K).contiguous().clone()
    else:
        Wd = draw(B, F, K)
    Hd = _factor(H, "H", [lead + (K, T)], dev).reshape(B, K, T).contiguous().clone() if init == "custom" else draw(B, K, T)

    ws = torch.empty((int(L.ap_nmf_workspace_bytes(B, F, T, K, loss)) + 7) // 8, dtype=torch.float64, device=dev)
    stream = _x.stream_ptr(dev)

    def run(n):
        _x.check(L.ap_nmf_mu_f32(_x.ptr(S), B, F, T, row_stride, K, _x.ptr(Wd), _x.ptr(Hd), int(n), loss,
                                 int(bool(update_components)), float(eps), _x.ptr(ws), stream))

    def objective():
        out = torch.empty(B, dtype=torch.float64, device=dev)
        _x.check(L.ap_nmf_objective_f32(_x.ptr(S), B, F, T, row_stride, K, _x.ptr(Wd), _x.ptr(Hd), loss, float(eps),
                                        _x.ptr(out), _x.ptr(ws), stream))
        return out.cpu()

    n_iter, max_iter = 0, int(max_iter)
    if float(tol) > 0.0 and max_iter > 0:
        first = previous = objective()
        while n_iter < max_iter:
            step = min(_TOL_BLOCK, max_iter - n_iter)
            run(step)
            n_iter += step
            current = objective()
            if bool((((previous - current) / first) < float(tol)).all()):
                break
            previous = current
    else:
        run(max_iter)
        n_iter = max_iter
    if two_d:
        Wd, Hd = Wd[0], Hd[0]
    return (Wd, Hd, n_iter) if return_n_iter else (Wd, Hd)


def decompose(S, n_components=None, transformer=None, sort=False, fit=True, **kwargs):
    """librosa.decompose.decompose on `nmf`: (components (.., F, K), activations (.., K, T)).

    n_components=None means F (refused above 64); `transformer` must be None (there is no host estimator on this
    path); fit=False needs the fixed dictionary as W=; sort=True orders the components by the bin of their peak (a
    stable sort) and the activations alike; further keywords go to `nmf`."""
    if transformer is not None:
        raise ValueError("transformer must be None: decompose runs the package's own NMF kernels, not a host estimator")
    S_t, two_d = _spectrum(S)
    if n_components is None:
        n_components = int(S_t.shape[-2])
        if n_components > MAX_COMPONENTS:
            raise ValueError(f"n_components=None means the {n_components} bins of S, above the limit of {MAX_COMPONENTS} "
                             f"components: pass n_components")
    if not fit:
        if kwargs.get("W") is None:
            raise ValueError("fit=False needs the fixed components as W=")
        kwargs["update_components"] = False
    W, H = nmf(S_t, n_components, **kwargs)[:2]
    if sort:
        order = torch.argsort(torch.argmax(W, dim=-2), dim=-1, stable=True)               # (.., K)
        W = torch.gather(W, -1, order.unsqueeze(-2).expand_as(W))
        H = torch.gather(H, -2, order.unsqueeze(-1).expand_as(H))
    return W, H


__all__ = ["hpss", "hpss_medians", "hpss_audio", "harmonic", "percussive", "nmf", "decompose"]


