"""The definition of cqt / vqt in float64 (NumPy / SciPy only), the cases the emulator and the GPU tests share, and the
error bound both are held to.  This file is the specification; mlx-audio-primitives_amd/cqt.py and csrc/kernels_cqt.h
are checked against it, never the other way round.

Definition (the filter bank of librosa 0.10's cqt / vqt, evaluated exactly: no octave recursion, no resampling, no
sparsified basis; librosa's own output approximates this bank and is no reference here):

    r = 2^(1 / bins_per_octave);  f_k = fmin 2^(tuning / bins_per_octave) r^k;  alpha = (r^2 - 1) / (r^2 + 1)
    Q = filter_scale / alpha;  N_k = Q sr / (f_k + gamma / alpha)          (a float; cqt: gamma = 0;
                                                                            vqt, gamma=None: gamma = alpha 24.7 / 0.108)
    m0_k = floor(-N_k / 2), m1_k = floor(N_k / 2), L_k = m1_k - m0_k
    g_k[m] = w[m - m0_k] exp(2 pi i f_k m / sr), w = get_window(window, L_k) (periodic), normalised by `norm`
             (1: sum |g|; 2: the L2 norm; inf: the maximum; None: as it is)
    C[k, t] = s_k sum_{m = m0_k}^{m1_k - 1} ypad[t hop + m] conj(g_k[m]),  s_k = sqrt(N_k) if scale else N_k
    t = 0 .. L // hop;  ypad: y outside [0, L) by pad_mode (numpy.pad's constant / edge / reflect)

Error bound, derived, for any summation order (u = 2^-24, up to O(u^2)):

    |C32 - C64| <= (d_k + 3) u s_k sum_m |ypad| |g_k[m]|

A float32 sum of n terms computed along any tree whose longest chain of dependent additions is d has error at most
d u sum |terms| (every term passes through at most d roundings, each relative to a partial sum that is bounded by the
sum of the absolute terms; a fused multiply-add rounds once, so the products add nothing).  The 3 covers the rounding
of a tap to float32, of s_k to float32 and of the final product.  The bound holds for the complex error with complex
|g|: the real and imaginary sums obey it with |Re g| and |Im g|, and the norm of a sum is at most the sum of the norms.

d_k comes from the tile constants the emulator twin reports (emu_cqt_bind.geometry()), not from the result: the bins
are grouped K at a time; a group's tap range [lo, hi) = [min m0, max (m0 + L)) is walked in chunks of C taps; a lane
adds C / lanes products per chunk to its partial sum, then one lane adds 32 lanes' sums in turn (31 additions) and
the two halves meet (1):  d_k = (C / lanes) ceil((hi - lo) / C) + red,  red = 32.  d_k = L_k would always be valid and
is useless: with 4103 equal taps a lost tap changes the sum by 1 / 4103 of the bound's scale, which only a bound
below that can see.  sharp() states the condition: 1 / L_k >= 2 (d_k + 3) u for every band of an equal-magnitude bank.
"""

from functools import lru_cache

import numpy as np
from scipy.signal import get_window as _scipy_window

U = 2.0 ** -24
C1 = 32.70319566257483
PAD_MODES = ("constant", "edge", "reflect")


def frequencies(n_bins, fmin, bins_per_octave=12, tuning=0.0):
    return fmin * 2.0 ** (tuning / bins_per_octave) * 2.0 ** (np.arange(n_bins, dtype=np.float64) / bins_per_octave)


def default_gamma(bins_per_octave):
    r2 = 2.0 ** (2.0 / bins_per_octave)
    return (r2 - 1.0) / (r2 + 1.0) * 24.7 / 0.108


def lengths(sr, fmin, n_bins, bins_per_octave=12, tuning=0.0, filter_scale=1.0, gamma=0.0):
    """(f_k, N_k (float), m0_k, L_k)."""
    f = frequencies(n_bins, fmin, bins_per_octave, tuning)
    r2 = 2.0 ** (2.0 / bins_per_octave)
    alpha = (r2 - 1.0) / (r2 + 1.0)
    N = (filter_scale / alpha) * sr / (f + gamma / alpha)
    m0 = np.floor(-N / 2.0).astype(np.int64)
    m1 = np.floor(N / 2.0).astype(np.int64)
    return f, N, m0, m1 - m0


def bank(sr, fmin, n_bins, bins_per_octave=12, tuning=0.0, filter_scale=1.0, norm=1, window="hann", gamma=0.0, scale=True):
    """([g_k complex128], m0 int64 (n_bins), s float64 (n_bins))."""
    f, N, m0, L = lengths(sr, fmin, n_bins, bins_per_octave, tuning, filter_scale, gamma)
    taps = []
    for k in range(n_bins):
        m = m0[k] + np.arange(L[k], dtype=np.float64)
        g = _scipy_window(window, int(L[k]), fftbins=True).astype(np.float64) * np.exp(2j * np.pi * f[k] * m / sr)
        if norm == 1:
            g = g / np.abs(g).sum()
        elif norm == 2:
            g = g / np.sqrt((np.abs(g) ** 2).sum())
        elif norm == np.inf:
            g = g / np.abs(g).max()
        else:
            assert norm is None
        taps.append(g)
    return taps, m0, np.sqrt(N) if scale else N


def pad_index(i, L, mode):
    """(index into y, is the sample one of y's?) for positions i of the padded signal."""
    i = np.asarray(i, np.int64)
    if mode == "constant":
        inside = (i >= 0) & (i < L)
        return np.clip(i, 0, L - 1), inside
    if mode == "edge":
        return np.clip(i, 0, L - 1), np.ones(i.shape, bool)
    assert mode == "reflect"
    if L == 1:
        return np.zeros_like(i), np.ones(i.shape, bool)
    p = 2 * (L - 1)
    r = np.mod(i, p)
    return np.where(r < L, r, p - r), np.ones(i.shape, bool)


def transform(y, hop, pad_mode, taps, m0, s):
    """(C (B, n_bins, T) complex128, A (B, n_bins, T) = s_k sum |ypad| |g_k|) of y (B, L) for a bank given as a list
    of complex tap arrays (any float type, used as float64)."""
    y = np.asarray(y, np.float64)
    B, L = y.shape
    T = 1 + L // hop
    C = np.empty((B, len(taps), T), np.complex128)
    A = np.empty((B, len(taps), T), np.float64)
    for k, g in enumerate(taps):
        g = np.asarray(g).astype(np.complex128)
        pos = (np.arange(T, dtype=np.int64) * hop)[:, None] + int(m0[k]) + np.arange(len(g), dtype=np.int64)[None, :]
        idx, own = pad_index(pos, L, pad_mode)
        frames = y[:, idx] * own                                      # (B, T, L_k)
        C[:, k] = float(s[k]) * (frames @ np.conj(g))
        A[:, k] = float(s[k]) * (np.abs(frames) @ np.abs(g))
    return C, A


def chain(m0, Ls, geom):
    """d_k of every band from the tile constants (module docstring)."""
    m0, Ls = np.asarray(m0, np.int64), np.asarray(Ls, np.int64)
    K, Cc, lanes, red = geom["bins_per_group"], geom["chunk"], geom["lanes"], geom["reduction_chain"]
    d = np.empty(len(Ls), np.int64)
    for g0 in range(0, len(Ls), K):
        sl = slice(g0, g0 + K)
        live = Ls[sl] > 0
        span = int((m0[sl] + Ls[sl])[live].max() - m0[sl][live].min()) if live.any() else 0
        d[sl] = (Cc // lanes) * -(-span // Cc) + red
    return d


def sharp(Ls, d):
    """The bound can see one lost or doubled tap of an equal-magnitude bank: 1 / L_k >= 2 (d_k + 3) u for every band."""
    Ls = np.asarray(Ls, np.float64)
    return bool(np.all(1.0 / Ls[Ls > 0] >= 2.0 * (np.asarray(d)[Ls > 0] + 3.0) * U))


def check(got, want, A, d, what=""):
    """Worst |got - want| / bound over all elements; asserts that it is at most 1."""
    got = np.asarray(got).astype(np.complex128)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got.view(np.float64)).all(), (what, "a value is not finite")
    bound = (np.asarray(d, np.float64)[None, :, None] + 3.0) * U * A
    err = np.abs(got - want)
    tiny = np.finfo(np.float64).tiny
    ratio = float(np.max(err / np.maximum(bound, tiny)))
    assert ratio <= 1.0, (what, ratio, np.unravel_index(np.argmax(err / np.maximum(bound, tiny)), err.shape))
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------------
HAND_LENGTHS = (1, 2, 63, 64, 65, 128, 277, 4103)


def hand_bank(n_bins, seed, centred=True):
    """A bank of n_bins filters with lengths drawn in turn from HAND_LENGTHS (rotated by the seed, so a group of bins
    holds unequal lengths), taps random complex of equal magnitude 1 / L as float32, scale in [0.5, 2).
    centred: m0 = -ceil(L / 2); otherwise deliberately off-centre, positive and negative."""
    rng = np.random.default_rng(1000 + seed)
    Ls = np.array([HAND_LENGTHS[(seed + 3 * k) % len(HAND_LENGTHS)] for k in range(n_bins)], np.int64)
    taps = []
    for L in Ls:
        ph = rng.uniform(0.0, 2.0 * np.pi, L)
        taps.append((np.exp(1j * ph) / L).astype(np.complex64))
    if centred:
        m0 = -((Ls + 1) // 2)
    else:
        m0 = np.array([(-L - 3 - 5 * k) if k % 2 else (7 + 11 * k) for k, L in enumerate(Ls)], np.int64)
    s = rng.uniform(0.5, 2.0, n_bins).astype(np.float32)
    return taps, m0.astype(np.int32), s


def pack(taps, dtype=np.complex64):
    """(taps back to back, offsets int64 (n_bins + 1))."""
    off = np.zeros(len(taps) + 1, np.int64)
    off[1:] = np.cumsum([len(g) for g in taps])
    flat = np.concatenate([np.asarray(g).astype(dtype) for g in taps]) if off[-1] else np.zeros(0, dtype)
    return flat, off


@lru_cache(maxsize=None)
def signal(B, L, seed=0):
    """(B, L) float32: noise with a slow envelope, so that frames differ in level; read-only."""
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((B, L)) * (0.25 + np.abs(np.sin(np.arange(L) / 37.0)))).astype(np.float32)
    y.setflags(write=False)
    return y


# (n_bins, T, hop): T in {1, 33, 65} x hop in {1, 64, 100, 512} x n_bins in {1, 5, 17}, every value met, L = (T - 1) hop + rest
HAND_CASES = (
    (1, 1, 1), (5, 1, 512), (17, 1, 100), (5, 33, 1), (17, 33, 64), (1, 33, 100), (5, 33, 512), (17, 65, 1), (5, 65, 64),
    (17, 65, 100), (1, 65, 512),
)
HAND_IDS = ["bins%d-T%d-hop%d" % c for c in HAND_CASES]


def hand_length(T, hop):
    """A clip length with 1 + L // hop = T that is no multiple of the hop (when the hop leaves room)."""
    return max(1, (T - 1) * hop + min(hop - 1, 37))


# real banks: (name, function, kwargs); sr = 8000 throughout
REAL_CASES = (
    ("hann", "cqt", dict(sr=8000, fmin=500.0, n_bins=17, window="hann")),
    ("boxcar", "cqt", dict(sr=8000, fmin=500.0, n_bins=17, window="boxcar")),
    ("hamming", "cqt", dict(sr=8000, fmin=500.0, n_bins=17, window="hamming")),
    ("vqt", "vqt", dict(sr=8000, fmin=100.0, n_bins=25, window="hann")),
)
REAL_IDS = [c[0] for c in REAL_CASES]


def real_bank(func, kw, **more):
    kw = dict(kw, **more)
    gamma = default_gamma(kw.get("bins_per_octave", 12)) if func == "vqt" and kw.get("gamma") is None else kw.get("gamma", 0.0)
    return bank(kw["sr"], kw["fmin"], kw["n_bins"], kw.get("bins_per_octave", 12), kw.get("tuning", 0.0),
                kw.get("filter_scale", 1.0), kw.get("norm", 1), kw.get("window", "hann"), gamma or 0.0, kw.get("scale", True))
