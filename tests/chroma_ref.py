"""Float64 definitions of the chroma features (chroma.py, csrc/kernels_chroma.h) and the error bound of their tests.

The definitions restate librosa 0.10's filters.chroma, filters.cq_to_chroma, feature.chroma_stft / chroma_cqt /
chroma_cens / tonnetz and util.normalize (fill=None, float32 tiny) independently of the package; no numeric parity
with librosa is claimed.

Error bound, u = 2^-24 (float32 unit roundoff), derived, not tuned.

Fold.  The kernel forms a_c = sum_k w[c,k] v_k with one fmaf per term; a wave adds its terms in ascending k and the
waves' partial sums are joined in wave order, so the longest chain of dependent additions is
    d = run ceil(K / (run waves)) + (waves - 1)
(run = 4 consecutive bins per wave and step, waves = 4: the emulator twin reports both).  A sum of products evaluated
with chains of at most d additions obeys |fl(a) - a| <= gamma_d sum |w||v|, gamma_d = d u / (1 - d u) (Higham, Accuracy
and Stability, 3.1; the fused product adds no rounding of its own).  v itself is rounded: |z|^2 = fma(im, im, fl(re^2))
has relative error <= 2u, |z| = sqrt of it <= u + u = 2u (IEEE sqrt); a real input none.  The reference is always given
the float32 matrix the kernel gets, so w carries no error against it (the builders' one rounding is checked on its own
in test_chroma_api.py; with a real input the 2 would cover it as well):
    |a32 - a64| <= (d + 2) u sum_k |w||v|     =: da         (first order; the tests scale it by 1 / (1 - (d + 2) u)).
The same holds for p = sum |v_k| with all weights 1: dp = (d + 2) u p.

Divisions.  For q = a / n with |fl(a) - a| <= da and |fl(n) - n| <= dn, one IEEE division gives
    |fl(q) - q| <= (da + |q| dn) / n + 2u |q|
(first order: the perturbation of the quotient, plus u for the division and u for second-order slack).  It is applied
twice: for pre_l1 (n = p) and for the norm.  The norm's own error: a norm is 1-Lipschitz in its own metric, so the
perturbation da moves it by at most the same norm of da; adding n_out terms in sequence costs (n_out) u n for the
L1 norm, (n_out / 2 + 1) u n for sqrt(sum of squares) (half the relative error of the sum plus the sqrt; bounded here
by (n_out + 2) u n), nothing for the maximum:
    dn = norm(da) + (n_out + 2) u n      (inf: dn = max da).
A norm below FLT_MIN counts as 1 with dn = 0.

Discontinuities.  a_c < threshold -> 0 and the four quantiser steps of CENS are not continuous: an element whose float64
value lies within its bound of the step may fall on either side.  Such elements are left out of the comparison; when
a norm (or the smoothing) follows, their whole frame (and every frame the smoothing window carries it into) is left
out, since the norm then differs by up to the step.  The tests assert that at most 1 % is left out.

CENS.  v = x / p: p is a sequential sum of n terms, so dv = (n + 2) u |v|.  The quantised values are exact
(0, .25, .5, .75, 1).  s = sum_j taps[j] q[.] is a chain of n_taps fmafs: ds = (n_taps + 1) u sum |taps| q.  The
final norm propagates as above.

Underflow: every bound gets (d + 2) 2^-149 added, one denormal spacing per operation.
"""

from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
DENORM = 2.0 ** -149
C1 = 32.70319566257483
STEPS = (0.4, 0.2, 0.1, 0.05)
NORMS = (None, 1, 2, np.inf)


# ---------------------------------------------------------------------------------------------------------------------
# definitions
# ---------------------------------------------------------------------------------------------------------------------
def norm_of(a, norm, axis):
    """The norm along `axis` (kept), values below TINY replaced by 1; (n, replaced?)."""
    m = np.abs(a)
    if norm == np.inf:
        n = m.max(axis=axis, keepdims=True)
    elif norm == 1:
        n = m.sum(axis=axis, keepdims=True)
    elif norm == 2:
        n = np.sqrt((m * m).sum(axis=axis, keepdims=True))
    else:
        raise ValueError(norm)
    small = n < TINY
    return np.where(small, 1.0, n), small


def normalize(a, norm, axis):
    if norm is None:
        return a
    return a / norm_of(a, norm, axis)[0]


def convolve_same(rows, taps):
    """SciPy's "same" along the last axis: s[t] = sum_j taps[j] q[t + (n - 1) // 2 - j], q = 0 outside."""
    rows = np.asarray(rows, np.float64)
    taps = np.asarray(taps, np.float64)
    n, T = len(taps), rows.shape[-1]
    full = np.zeros(rows.shape[:-1] + (T + n - 1,))
    for j in range(n):
        full[..., j:j + T] += taps[j] * rows
    h = (n - 1) // 2
    return full[..., h:h + T]


def chroma_filterbank(sr, n_fft, n_chroma=12, tuning=0.0, ctroct=5.0, octwidth=2, norm=2, base_c=True):
    fr = np.linspace(0.0, float(sr), int(n_fft), endpoint=False)[1:]
    a440 = 440.0 * 2.0 ** (tuning / n_chroma)
    fb = n_chroma * np.log2(fr / (a440 / 16.0))
    fb = np.concatenate(([fb[0] - 1.5 * n_chroma], fb))
    bw = np.concatenate((np.maximum(np.diff(fb), 1.0), [1.0]))
    h = np.round(n_chroma / 2.0)
    w = np.empty((n_chroma, n_fft))
    for c in range(n_chroma):
        D = np.remainder(fb - c + h + 10 * n_chroma, n_chroma) - h
        w[c] = np.exp(-0.5 * (2.0 * D / bw) ** 2)
    w = normalize(w, norm, 0)
    if octwidth is not None:
        w = w * np.exp(-0.5 * ((fb / n_chroma - ctroct) / octwidth) ** 2)
    if base_c:
        w = np.roll(w, -3 * (n_chroma // 12), axis=0)
    return w[:, :1 + n_fft // 2]


def cq_to_chroma(n_input, bins_per_octave=12, n_chroma=12, fmin=None, window=None, base_c=True):
    m = bins_per_octave // n_chroma
    w = np.zeros((n_chroma, bins_per_octave))
    for c in range(n_chroma):
        w[c, c * m:(c + 1) * m] = 1.0
    w = np.roll(w, -(m // 2), axis=1)
    w = np.tile(w, int(math.ceil(n_input / bins_per_octave)))[:, :n_input]
    r = np.mod(69.0 + 12.0 * math.log2((C1 if fmin is None else fmin) / 440.0), 12.0)
    if not base_c:
        r -= 9.0
    w = np.roll(w, int(np.round(r * n_chroma / 12.0)), axis=0)
    if window is not None:
        w = convolve_same(w, window)
    return w


def phi(n_chroma=12):
    V = np.outer([7.0 / 6, 7.0 / 6, 3.0 / 2, 3.0 / 2, 2.0 / 3, 2.0 / 3], np.linspace(0.0, 12.0, n_chroma, endpoint=False))
    V[::2] -= 0.5
    return np.array([1.0, 1.0, 1.0, 1.0, 0.5, 0.5])[:, None] * np.cos(np.pi * V)


def values(x, in_kind):
    """v of the fold in float64 from the float32 / complex64 input."""
    if in_kind == 0:
        return np.asarray(x, np.float64)
    z = np.asarray(x, np.complex128)
    m2 = z.real ** 2 + z.imag ** 2
    return np.sqrt(m2) if in_kind == 1 else m2


def chain(K, consts):
    """d of the fold for K bins, from the emulator twin's tile constants."""
    run, waves = consts["fold_run"], consts["fold_waves"]
    return run * math.ceil(K / (run * waves)) + waves - 1


def _divide(a, da, n, dn):
    q = a / n
    return q, (da + np.abs(q) * dn) / n + 2.0 * U * np.abs(q)


def _norm_step(a, da, norm, n_terms):
    """a / norm(a) along axis 1 with its bound."""
    n, small = norm_of(a, norm, 1)
    if norm == np.inf:
        dn = da.max(axis=1, keepdims=True)
    elif norm == 1:
        dn = da.sum(axis=1, keepdims=True) + (n_terms + 2) * U * n
    else:
        dn = np.sqrt((da * da).sum(axis=1, keepdims=True)) + (n_terms + 2) * U * n
    dn = np.where(small, 0.0, dn)
    return _divide(a, da, n, dn)


def fold(x, in_kind, w, consts, *, pre_l1=False, threshold=None, norm=None):
    """(want, bound, keep) of the fold for x (B, K, T) and w (n_out, K) or None, all float64; keep marks the elements
    that are compared (module docstring).  w: the float32 matrix the kernel gets."""
    v = values(x, in_kind)
    B, K, T = v.shape
    w = np.eye(K) if w is None else np.asarray(w, np.float64)
    n_out = w.shape[0]
    d = chain(K, consts)
    g = (d + 2) * U / (1.0 - (d + 2) * U)
    a = np.einsum("ck,bkt->bct", w, v)
    da = g * np.einsum("ck,bkt->bct", np.abs(w), np.abs(v)) + (d + 2) * DENORM
    keep = np.ones(a.shape, bool)
    if pre_l1:
        p = np.abs(v).sum(axis=1, keepdims=True)
        dp = g * p
        small = p < TINY
        assert not np.any((p > 0) & (p < 4 * TINY)), "a frame's sum lies at the edge of the normal range"
        a, da = _divide(a, da, np.where(small, 1.0, p), np.where(small, 0.0, dp))
    if threshold is not None:
        near = np.abs(a - threshold) <= da
        keep &= ~(near.any(axis=1, keepdims=True) if norm is not None else near)
        zero = a < threshold
        a = np.where(zero, 0.0, a)
        da = np.where(zero, 0.0, da)
    if norm is not None:
        a, da = _norm_step(a, da, norm, n_out)
    return a, da, np.broadcast_to(keep, a.shape)


def quantise(v):
    return 0.25 * sum((v > s).astype(np.float64) for s in STEPS)


def cens(x, taps, norm, *, consts=None):
    """(want, bound, keep) of the CENS kernel for chroma x (B, n, T) float32 and float32 taps (or None)."""
    x = np.asarray(x, np.float64)
    B, n, T = x.shape
    p, _ = norm_of(x, 1, 1)
    v = x / p
    dv = (n + 2) * U * np.abs(v) + DENORM
    near = np.zeros((B, 1, T), bool)
    for s in STEPS:
        near |= (np.abs(v - s) <= dv).any(axis=1, keepdims=True)
    q = quantise(v)
    if taps is not None and len(taps):
        t64 = np.asarray(taps, np.float64)
        s = convolve_same(q, t64)
        ds = (len(t64) + 1) * U * convolve_same(q, np.abs(t64)) + (len(t64) + 1) * DENORM
        near = convolve_same(near.astype(np.float64), np.ones(len(t64))) > 0      # every frame the window carries it into
    else:
        s, ds = q, np.zeros(q.shape)
    if norm is not None:
        s, ds = _norm_step(s, ds, norm, n)
    return s, ds, np.broadcast_to(~near, s.shape)


def check(got, want, bound, keep, label, max_left_out=0.01):
    """Assert |got - want| <= bound on the elements kept and that at most 1 % was left out; worst error / bound."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    left_out = 1.0 - keep.mean()
    assert left_out <= max_left_out, f"{label}: {100 * left_out:.2f} % of the elements lie at a step; pick other inputs"
    err = np.abs(got - want)[keep]
    b = bound[keep]
    assert np.all(np.isfinite(got[keep])), f"{label}: a value is not finite"
    ratio = float(np.max(err / np.maximum(b, DENORM))) if err.size else 0.0
    assert np.all(err <= b), f"{label}: worst error / bound {ratio:.3f} at {np.unravel_index(np.argmax(err / np.maximum(b, DENORM)), err.shape)}"
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# shared inputs (read-only, computed once)
# ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def spectrum(B, K, T, in_kind, seed=0):
    """(B, K, T) float32 (non-negative, a magnitude-like spread over three decades, levels that differ by frame) or
    complex64."""
    rng = np.random.default_rng(10_000 + seed)
    mag = 10.0 ** rng.uniform(-3.0, 0.0, (B, K, T)) * (0.25 + rng.uniform(0.0, 1.0, (B, 1, T)))
    if in_kind == 0:
        x = mag.astype(np.float32)
    else:
        x = (mag * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (B, K, T)))).astype(np.complex64)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def matrix(n_out, K, seed=0):
    """(n_out, K) float32, dense, both signs."""
    w = np.random.default_rng(20_000 + seed).standard_normal((n_out, K)).astype(np.float32)
    w.setflags(write=False)
    return w


@lru_cache(maxsize=None)
def chroma_input(B, n, T, seed=0):
    """(B, n, T) float32 chroma-like input: uniform, log-uniform and 60 % sparse frames in turn, a few silent frames.
    Frames whose L1-normalised float64 value lies within 64 u of a quantiser step are drawn again, so that the
    comparison leaves (almost) nothing out; the rule looks at the input alone."""
    rng = np.random.default_rng(30_000 + seed)

    def draw(kind, shape):
        if kind == 0:
            return rng.uniform(0.0, 1.0, shape)
        if kind == 1:
            return 10.0 ** rng.uniform(-3.0, 0.0, shape)
        return rng.uniform(0.0, 1.0, shape) * (rng.uniform(0.0, 1.0, shape) > 0.6)

    x = np.empty((B, n, T), np.float32)
    for b in range(B):
        for t in range(T):
            for _ in range(100):
                col = draw((b + t) % 3, n).astype(np.float32)
                v = col.astype(np.float64) / max(np.abs(col.astype(np.float64)).sum(), TINY)
                if all(np.all(np.abs(v - s) > 64 * U) for s in STEPS):
                    break
            x[b, :, t] = col
    if T > 4:
        x[:, :, 3] = 0.0
    x.setflags(write=False)
    return x


def hann_taps(n):
    """The symmetric Hann window of n + 2 points divided by its sum, float32 (chroma_cens' smoothing taps)."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n + 2) / (n + 1))
    return (w / w.sum()).astype(np.float32)


@lru_cache(maxsize=None)
def random_taps(n, seed=0):
    t = np.random.default_rng(40_000 + seed).uniform(-0.5, 1.0, n).astype(np.float32)
    t.setflags(write=False)
    return t
