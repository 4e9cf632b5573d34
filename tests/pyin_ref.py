"""The definition of pyin (pitch.py, csrc/kernels_pyin.h) in NumPy: not a test module, not product code.
observe64: the observation stage in float64 on a float32 curve and the float32 host tables (thr, beta, ea, nz), which
test_pyin_api.py holds to their closed forms.  expected: the float64 outputs and the bounds DESIGN.md 9.17 derives from the
count of float32 operations.  decode_f32: the sequential float32 model of the banded decode, which the kernel equals in
every bit."""

import math

import numpy as np

import viterbi_ref as V

TINY, U = V.TINY, V.U


def observe64(curve, lo, sr, fmin, bps, n_bins, tabs, no_trough):
    """curve (n_lags, T) float32 -> (p (T, n_bins) float64 bin probabilities, unclipped voiced sum (T), decisive (T) bool:
    no candidate's fractional bin within 1e-9 of a half)."""
    thr, (b64, e64, z64) = tabs["thr"], (tabs[k].astype(np.float64) for k in ("beta", "ea", "nz"))
    d = np.asarray(curve, np.float32)
    n_lags, T = d.shape
    P, dec = np.zeros((T, n_bins)), np.ones(T, bool)
    for t in range(T):
        c = d[:, t]
        tr = np.concatenate([[c[0] < c[1]], (c[1:-1] < c[:-2]) & (c[1:-1] <= c[2:]), [c[-1] < c[-2]]])
        xs = np.flatnonzero(tr)
        if not xs.size:
            continue
        passed = c[xs][:, None] < thr[None, :]                      # float32 comparison
        rank = np.maximum(np.cumsum(passed, axis=0) - 1, 0)
        p = np.where(passed, b64[None, :] * z64[passed.sum(axis=0)][None, :] * e64[rank], 0.0).sum(axis=1)
        g = int(np.argmin(c[xs]))
        p[g] += no_trough * b64[~passed[g]].sum()
        for x, pi in zip(xs.tolist(), p.tolist()):                  # lag order: the larger lag overwrites
            if not pi > 0:
                continue
            shift = 0.0
            if 0 < x < n_lags - 1:
                dm, d0, dp = float(c[x - 1]), float(c[x]), float(c[x + 1])
                a, b = dp + dm - 2.0 * d0, (dp - dm) / 2.0
                shift = -b / a if abs(b) < abs(a) else 0.0
            fb = 12.0 * bps * math.log2(sr / (lo + x + shift) / fmin)
            dec[t] &= abs(fb - math.floor(fb) - 0.5) >= 1e-9
            k = int(min(max(np.rint(fb), 0), n_bins))
            if k < n_bins:
                P[t, k] = pi
    return P, P.sum(axis=1), dec


def expected(P, vsum, n, n_lags):
    """(E64 (T, n_bins + 1), its bound, voiced_prob64 (T), its bound) from observe64's output."""
    nb = P.shape[1]
    g_p, g_v = (1 + U) ** (n + 3) - 1, (1 + U) ** (n + 3 + (n_lags + 1) // 2) - 1
    v, dv = np.clip(vsum, 0.0, 1.0), g_v * vsum + 2.0 ** -126
    q = (1.0 - v) / nb
    dq = (dv + U * (1.0 - v)) / nb * (1 + 5 * U) + 5 * U * q
    L = np.log(np.concatenate([P, q[:, None]], axis=1) + TINY)
    e = np.concatenate([np.full_like(P, 1.001 * (g_p + 2.0 ** -149 / TINY + U)), (1.001 * (dq / (q + TINY) + U))[:, None]], axis=1)
    return L, e + V.LOGF_ULPS * 2.0 ** -23 * (np.abs(L) + e), v, dv


def decode_f32(E, lw, lz, ls, li, h):
    """The float32 model on E (T, n_bins + 1): (ptr uint16 (T, 2 n_bins), states int32 (T), logp float64)."""
    E, lw, lz, ls = (np.asarray(a, np.float32) for a in (E, lw, lz, np.reshape(ls, (2, 2))))
    T, nb, li = E.shape[0], E.shape[1] - 1, np.float32(li)
    j, first = np.arange(nb), np.maximum(h - np.arange(nb), 0)      # first: the first source inside the bins, as an offset from j - h
    ptr = np.zeros((T, 2 * nb), np.uint16)
    v = np.stack([E[0, :nb] + li, np.full(nb, E[0, nb] + li, np.float32)])
    m, acc = v.max(), np.float64(v.max())
    for t in range(1, T):
        x = np.full((2, nb + 2 * h), -np.inf, np.float32)
        x[:, h:h + nb] = (v - m) - lz[None, :]
        cand = np.lib.stride_tricks.sliding_window_view(x, 2 * h + 1, axis=1) + lw[::-1][None, None, :]
        c, k = cand.max(axis=2), j[None, :] - h + np.maximum(cand.argmax(axis=2), first[None, :])
        for b in range(2):
            a0, a1 = c[0] + ls[0, b], c[1] + ls[1, b]
            v[b] = (E[t, :nb] if b == 0 else E[t, nb]) + np.where(a1 > a0, a1, a0)
            ptr[t, b * nb:(b + 1) * nb] = np.where(a1 > a0, nb + k[1], k[0])
        m = v.max()
        acc = acc + np.float64(m)
    assert v.dtype == np.float32 and not np.isnan(v).any()
    states = np.empty(T, np.int32)
    states[-1] = int(v.reshape(-1).argmax())
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return ptr, states, np.float64(acc + np.float64(v.reshape(-1)[states[-1]] - m))
