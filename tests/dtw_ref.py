"""The definition of dynamic time warping (dtw.py, csrc/kernels_dtw.h) as an independent numpy model, and the error
bound of the cost kernel's tests.

The recursion is restated from librosa 0.10's sequence.dtw; no numeric parity with librosa is claimed.  For the step
table s = 0 .. n_steps - 1 with (a_s, b_s), add_s, mul_s:

    in_band(i,j):  r = int(round_half_even(band_rad min(N, M)));  -r - max(N - M, 0) < j - i < r + max(M - N, 0)
    c(i,j)     = C[i,j] inside the band (or with no band), +inf outside
    start(i,j) = (i == 0 and j == 0) or (subseq and i == 0)
    best = c(i,j) if start(i,j) else +inf;  code = 254 if start(i,j) else 255
    for s ascending:  cand = D[i - a_s, j - b_s] (+inf outside the matrix)  (+)  ((mul_s (*) c(i,j)) (+) add_s)
                      if cand < best: best = cand; code = s
    D[i,j] = best; steps[i,j] = code;  if not best < +inf: D[i,j] = +inf, steps[i,j] = 255

(+) and (*) are single float32 operations.  The model walks the anti-diagonals i + j = k in ascending k (a cell reads
only cells of smaller i + j) and evaluates each with numpy float32 array operations, which round one at a time; it knows
nothing of tiles.  The device result must equal it in every bit.

Cost metrics, float64, with a derived bound (u = 2^-24).  The kernel takes e_k = fl(x_k - y_k) (relative error u) and
sums the d terms in ascending k, products fused: a chain of d additions, so with the rounding of e (2u on e^2, u on |e|)
    |fl(s) - s| <= (d + 2) u sum_k |term_k|                      sqeuclidean, cityblock (first order; scaled by 1 / (1 - (d + 2) u))
    euclidean:  sqrt halves the relative error and adds u:  ((d + 2) / 2 + 2) u sqrt(s)      (one u of slack)
    cosine:     dot, |x|^2, |y|^2 as above (inputs exact: (d + 2) u sum |x_k y_k| etc.); each norm ((d + 2) / 2 + 1) u;
                den = |x| |y| rounded once: e_den = (d + 5) u;  q = dot / den:  (d_dot + |q| den e_den) / den + 2u |q|
                (the rule of chroma_ref for a division);  1 - q rounded once: + u |1 - q|.  den < FLT_MIN counts as 1.
Underflow: (d + 2) 2^-149 is added to every sum's bound (and its square root to the euclidean one).
"""

from __future__ import annotations

import numpy as np

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
DENORM = 2.0 ** -149
F32 = np.float32
INF32 = np.float32(np.inf)
START, NONE = 254, 255
DEFAULT_STEPS = ((1, 1), (0, 1), (1, 0))
METRICS = ("euclidean", "sqeuclidean", "cityblock", "cosine")


def band_radius(band_rad, N, M):
    return int(round(band_rad * min(N, M)))                 # Python's round: half to even


def in_band(i, j, N, M, r):
    return (-r - max(N - M, 0) < j - i) & (j - i < r + max(M - N, 0))


def table(steps=None, add=None, mul=None):
    steps = DEFAULT_STEPS if steps is None else tuple((int(a), int(b)) for a, b in steps)
    add = np.zeros(len(steps), F32) if add is None else np.asarray(add, F32)
    mul = np.ones(len(steps), F32) if mul is None else np.asarray(mul, F32)
    assert len(add) == len(mul) == len(steps)
    return steps, add, mul


def accumulate(C, steps=None, add=None, mul=None, *, subseq=False, band_r=None):
    """(D float32 (N, M), codes uint8 (N, M)) of one cost matrix C (N, M); band_r: the band's radius r, or None."""
    steps, add, mul = table(steps, add, mul)
    C = np.asarray(C, F32)
    N, M = C.shape
    c = C.copy()
    if band_r is not None:
        ii, jj = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
        c[~in_band(ii, jj, N, M, band_r)] = INF32
    D = np.full((N, M), INF32, F32)
    S = np.full((N, M), NONE, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(N + M - 1):
            i = np.arange(max(0, k - M + 1), min(N - 1, k) + 1)
            j = k - i
            cc = c[i, j]
            start = (i == 0) & ((j == 0) | bool(subseq))
            best = np.where(start, cc, INF32).astype(F32)
            code = np.where(start, START, NONE).astype(np.int64)
            for s, (a, b) in enumerate(steps):
                pi, pj = i - a, j - b
                ok = (pi >= 0) & (pj >= 0)
                pred = np.where(ok, D[np.maximum(pi, 0), np.maximum(pj, 0)], INF32).astype(F32)
                w = (mul[s] * cc).astype(F32)
                w = (w + add[s]).astype(F32)
                cand = (pred + w).astype(F32)
                win = cand < best
                best = np.where(win, cand, best)
                code = np.where(win, s, code)
            dead = ~(best < INF32)
            best[dead] = INF32
            code[dead] = NONE
            D[i, j] = best
            S[i, j] = code
    return D, S


def backtrack(S, steps=None, *, D=None, subseq=False, start=None):
    """The path (L, 2) int32 from the end cell to a cell with code 254, or None when there is none."""
    steps = DEFAULT_STEPS if steps is None else steps
    N, M = S.shape
    i = N - 1
    if start is not None:
        j = int(start)
    elif subseq:
        j = int(np.argmin(D[N - 1]))                        # the first minimum
    else:
        j = M - 1
    path = []
    while True:
        code = int(S[i, j])
        if code == NONE or (code != START and code >= len(steps)):
            return None
        path.append((i, j))
        if code == START:
            return np.asarray(path, np.int32).reshape(-1, 2)
        i -= steps[code][0]
        j -= steps[code][1]
        if i < 0 or j < 0:
            return None


def cost(X, Y, metric):
    """(C float64 (B, N, M), bound) of X (B, d, N), Y (B, d, M), given as the float32 values the kernel gets."""
    X = np.asarray(X, F32)
    Y = np.asarray(Y, F32)
    d = X.shape[1]
    x = X.astype(np.float64)[:, :, :, None]
    y = Y.astype(np.float64)[:, :, None, :]
    g = (d + 2) * U / (1.0 - (d + 2) * U)
    under = (d + 2) * DENORM
    if metric in ("euclidean", "sqeuclidean"):
        s = ((x - y) ** 2).sum(axis=1)
        if metric == "sqeuclidean":
            return s, g * s + under
        return np.sqrt(s), ((d + 2) / 2.0 + 2.0) * U * np.sqrt(s) / (1.0 - (d + 2) * U) + np.sqrt(under)
    if metric == "cityblock":
        s = np.abs(x - y).sum(axis=1)
        return s, g * s + under
    if metric == "cosine":
        dot = (x * y).sum(axis=1)
        ddot = g * np.abs(x * y).sum(axis=1) + under
        den = np.sqrt((x * x).sum(axis=1)) * np.sqrt((y * y).sum(axis=1))
        small = den < TINY
        den = np.where(small, 1.0, den)
        e_den = np.where(small, 0.0, (d + 5) * U / (1.0 - (d + 5) * U))
        q = dot / den
        dq = (ddot + np.abs(q) * den * e_den) / den + 2 * U * np.abs(q)
        return 1.0 - q, dq + U * (np.abs(1.0 - q) + dq) + DENORM
    raise ValueError(metric)


def check_cost(got, want, bound, what=""):
    """Asserts |got - want| <= bound everywhere; returns the worst error / bound."""
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all(), f"{what}: a value is not finite"
    ratio = err / np.maximum(bound, DENORM)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"{what}: worst error / bound {worst:.3f} at {np.unravel_index(int(ratio.argmax()), ratio.shape)}"
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def cost_matrix(B, N, M, seed, kind="uniform"):
    """C (B, N, M) float32: "uniform" in [0, 1); "ties": integers of {0, 1, 2}; "signed": in [-1, 1)."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "ties":
        return rng.integers(0, 3, (B, N, M)).astype(F32)
    if kind == "signed":
        return (2.0 * rng.random((B, N, M)) - 1.0).astype(F32)
    return rng.random((B, N, M)).astype(F32)


def features(B, d, T, seed):
    return np.random.default_rng(2000 + seed).standard_normal((B, d, T)).astype(F32)
