"""The definition of piptrack / pitch_tuning / estimate_tuning as a NumPy model.

float32 throughout, every operation rounded on its own in the order of the definition (NumPy's float32 ufuncs round
each result; nothing is fused); the residuals and edges of pitch_tuning are float64.  The model knows nothing of
tiles, waves or records.  It restates librosa 0.10's piptrack / pitch_tuning / estimate_tuning; no parity with
librosa's numbers is claimed beyond that."""

import math

import numpy as np

F32 = np.float32
TINY = np.finfo(np.float32).tiny


def bin_range(sr, n_fft, fmin, fmax, F):
    """(k_lo, k_hi) by brute force: the bins with max(fmin, 0) <= k sr / n_fft < min(fmax, sr / 2) are k_lo .. k_hi - 1."""
    f = np.arange(F, dtype=np.float64) * float(sr) / n_fft
    lo, hi = max(float(fmin), 0.0), min(float(fmax), float(sr) / 2.0)
    mask = (f >= lo) & (f < hi)
    k_lo = int(np.argmax(f >= lo)) if (f >= lo).any() else F
    k_hi = int(np.argmax(f >= hi)) if (f >= hi).any() else F
    assert np.array_equal(mask, (np.arange(F) >= k_lo) & (np.arange(F) < k_hi))
    return k_lo, k_hi


def magnitude(z):
    """|z| of complex64 as the kernel forms it, sqrtf(fmaf(im, im, re re)) with re re rounded first: the fused operation
    is evaluated in float64 (exact product of two float32, one float64 addition) and rounded once.  Returns (|z|,
    mask of elements where that float64 sum could have double-rounded: it lies exactly on a float32 rounding tie)."""
    z = np.asarray(z, np.complex64)
    re, im = z.real.astype(F32), z.imag.astype(F32)
    rr = (re * re).astype(F32).astype(np.float64)
    s64 = im.astype(np.float64) * im.astype(np.float64) + rr
    s32 = s64.astype(F32)
    # a float64 that is not exact (53 bits used) and sits on a float32 tie is the only way to double-round
    up = np.nextafter(s32, F32(np.inf)).astype(np.float64)
    dn = np.nextafter(s32, F32(-np.inf)).astype(np.float64)
    tie = (s64 == 0.5 * (s32.astype(np.float64) + up)) | (s64 == 0.5 * (s32.astype(np.float64) + dn))
    # on such a tie the exact sum decides: it is the tie itself (half-to-even was right) or lies to one side of it
    from fractions import Fraction

    wrong = np.zeros(s32.shape, bool)
    for i in zip(*np.nonzero(tie)):
        exact = Fraction(float(im[i])) ** 2 + Fraction(float(rr[i]))
        mid = Fraction(float(s64[i]))
        other = up[i] if s64[i] > s32[i] else dn[i]
        lo, hi = min(float(s32[i]), other), max(float(s32[i]), other)
        right = hi if exact > mid else lo if exact < mid else float(s32[i])
        wrong[i] = right != float(s32[i])
    return np.sqrt(s32).astype(F32), wrong


def piptrack(S, *, sr=22050, fmin=150.0, fmax=4000.0, threshold=0.1, ref=None, k_range=None):
    """(pitches, magnitudes) float32 (B, F, T) of magnitudes S (B, F, T) float32.  ref: None, a number, or an array
    broadcastable to (B, T).  k_range: (k_lo, k_hi) instead of fmin / fmax."""
    S = np.asarray(S, F32)
    B, F, T = S.shape
    n_fft = 2 * (F - 1)
    k_lo, k_hi = bin_range(sr, n_fft, fmin, fmax, F) if k_range is None else k_range
    a, b, c = S[:, :-2], S[:, 1:-1], S[:, 2:]
    avg = np.zeros_like(S)
    shift = np.zeros_like(S)
    with np.errstate(all="ignore"):
        avg[:, 1:-1] = F32(0.5) * (c - a)
        den = (F32(2.0) * b - c) - a
        den = den + np.where(np.abs(den) < TINY, F32(1.0), F32(0.0))
        shift[:, 1:-1] = avg[:, 1:-1] / den
        dskew = (F32(0.5) * avg) * shift
        if ref is None:
            ref_value = F32(threshold) * S.max(axis=1, keepdims=True)
        else:
            ref_value = np.broadcast_to(np.abs(np.asarray(ref, F32)), (B, T))[:, None, :] if np.ndim(ref) else np.full((B, 1, T), abs(F32(ref)), F32)
        X = np.where(S > ref_value, S, F32(0.0))
        below = np.concatenate([X[:, :1], X[:, :-1]], axis=1)
        above = np.concatenate([X[:, 1:], X[:, -1:]], axis=1)
        k = np.arange(F)[None, :, None]
        peak = (X > below) & (X >= above) & (k >= k_lo) & (k < k_hi)
        bin_hz = F32(float(sr) / n_fft)
        pitches = np.where(peak, (k.astype(F32) + shift) * bin_hz, F32(0.0)).astype(F32)
        mags = np.where(peak, S + dskew, F32(0.0)).astype(F32)
    return pitches, mags


def residuals(f, bins_per_octave=12):
    """The float64 residuals of the frequencies f > 0 (float32), in [-0.5, 0.5)."""
    f = np.asarray(f, F32).ravel()
    f = f[f > 0].astype(np.float64)
    r = np.mod(bins_per_octave * np.log2(f / 27.5), 1.0)
    r[r >= 0.5] -= 1.0
    return r


def edges(resolution):
    return np.linspace(-0.5, 0.5, int(math.ceil(1.0 / resolution)) + 1)


def counts(f, resolution=0.01, bins_per_octave=12):
    return np.histogram(residuals(f, bins_per_octave), bins=edges(resolution))[0].astype(np.int64)


def pitch_tuning(f, resolution=0.01, bins_per_octave=12):
    c = counts(f, resolution, bins_per_octave)
    return float(edges(resolution)[int(np.argmax(c))]) if c.any() else 0.0


def median(m):
    """The float32 median as the definition has it."""
    m = np.sort(np.asarray(m, F32))
    n = m.size
    if n == 0:
        return F32(0.0)
    return m[n // 2] if n % 2 else F32((m[n // 2 - 1] + m[n // 2]) * F32(0.5))


def tuning_parts(pitches, mags, resolution=0.01, bins_per_octave=12):
    """(n, threshold, counts) of one group of dense piptrack outputs."""
    sel = pitches > 0
    thr = median(mags[sel])
    keep = sel & (mags >= thr)
    return int(sel.sum()), thr, counts(pitches[keep], resolution, bins_per_octave)


def estimate_tuning(S, *, resolution=0.01, bins_per_octave=12, per_clip=False, **kw):
    p, m = piptrack(S, **kw)
    groups = [(p[b], m[b]) for b in range(p.shape[0])] if per_clip else [(p, m)]
    out = []
    for pg, mg in groups:
        n, _, c = tuning_parts(pg, mg, resolution, bins_per_octave)
        out.append(float(edges(resolution)[int(np.argmax(c))]) if n else 0.0)
    return np.array(out) if per_clip else out[0]


def nearest_edge_distance(f, resolution=0.01, bins_per_octave=12):
    r = residuals(f, bins_per_octave)
    return float(np.abs(r[:, None] - edges(resolution)[None, :]).min()) if r.size else np.inf


def tones(B, L, seed, sr=22050, detune=0.0, noise=0.02):
    """Fixed-seed sums of detuned sinusoids plus noise, float32 (B, L)."""
    rng = np.random.default_rng(seed)
    n = np.arange(L) / float(sr)
    y = np.zeros((B, L))
    for b in range(B):
        for midi in rng.choice(np.arange(45, 84), size=4, replace=False):
            f0 = 440.0 * 2.0 ** ((midi - 69 + detune + 0.01 * rng.standard_normal()) / 12.0)
            for h in (1, 2, 3):
                y[b] += rng.uniform(0.2, 1.0) / h * np.cos(2 * np.pi * f0 * h * n + rng.uniform(0, 6.28))
    y += noise * rng.standard_normal((B, L))
    return (y / np.abs(y).max()).astype(F32)


def harmonics(d, L=22050 * 2, sr=22050):
    """Four notes with three harmonics each, all detuned by d semitone bins: float32 (L,)."""
    n = np.arange(L) / float(sr)
    y = sum(a / h * np.cos(2 * np.pi * 440.0 * 2.0 ** ((note + d) / 12.0) * h * n)
            for note, a in ((-12, 1.0), (-5, 0.8), (0, 0.9), (4, 0.7)) for h in (1, 2, 3))
    return (y / np.abs(y).max()).astype(F32)


def dense_peaks(B, F, T, seed):
    """A spectrum of independent magnitudes, about a third of whose bins are peaks at threshold 0: float32 (B, F, T)."""
    return np.random.default_rng(seed).gamma(2.0, 1.0, (B, F, T)).astype(F32)


def spectrum(y, n_fft, hop):
    """A float64 STFT (hann, centred, zero padding) rounded to complex64: (B, F, T)."""
    y = np.asarray(y, np.float64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    yp = np.pad(y, ((0, 0), (n_fft // 2, n_fft // 2)))
    T = 1 + (yp.shape[1] - n_fft) // hop
    fr = np.stack([yp[:, t * hop:t * hop + n_fft] * w for t in range(T)], axis=1)
    return np.fft.rfft(fr, axis=-1).transpose(0, 2, 1).astype(np.complex64)
