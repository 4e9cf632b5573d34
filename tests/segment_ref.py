"""The definition of recurrence_matrix / cross_similarity / recurrence_to_lag / lag_to_recurrence (segment.py,
csrc/kernels_segment.h) as an independent numpy model over a GIVEN float32 distance matrix D (n_ref, n),
D[i, j] = metric(ref[:, i], data[:, j]): the tests take D from the DTW cost kernel, whose own tests bound it.

    eligible(i, j)  = |i - j| >= width (width = 0: cross-similarity) and D[i, j] is no NaN
    k               = min(k, number of eligible i); default 2 ceil(sqrt(n - 2 width + 1)) / 2 ceil(sqrt(n_ref))
    neighbours(j)   = the first k eligible i in the order (D[i, j], i)            (full: every eligible i)
    record(j)       = (tau_j, t_j): the distance of the k-th neighbour and the largest neighbour index with that
                      distance; (NaN, -1) without neighbours.  i is a neighbour iff eligible and (D, i) <= (tau_j, t_j)
    sym             = keep (i, j) only if i is a neighbour of j and j one of i    (R = min(R, R^T) for symmetric D)
    self            = last: the diagonal is 1 (connectivity, affinity) or 0 (distance)
    bandwidth       = over kth = tau_j of the queries with a neighbour: the median (even count: fl(fl(a + b) 0.5f)),
                      the mean, the geometric mean
    affinity        = exp(-D / bw)
    lag             = lag[(i - j) mod t', j] = rec[i, j], t' = 2 n (pad) or n; the other rows 0

Everything but the affinity and the two mean bandwidths is exact and must be met in every bit.

Bounds (u = 2^-24, c = pcen_ref.C_ULP units of u for one v_exp_f32, the assumption stated there).  The kernel computes
2^(fl(D s)) with s = fl32(-log2(e) / bw) (bw taken as float64): s carries u, the product another u, so the exponent
p = -D log2(e) / bw is off by at most |p| (2 u + u^2) and the result by the factor 2^that; the instruction adds c u; a
result below FLT_MIN may come out as 0:
    |got - a| <= a (expm1(ln 2 |p| (2 u + u^2)) + c u) (1 + 2^-10) + FLT_MIN
mean_k / gmean_k are float64 sums of m float32 values in a fixed order, rounded to float32 once: relative
u + (m + 2) 2^-53 for the mean; for the geometric mean the float64 log and exp are taken to be within 2 ulp (assumed, as
the libm and the device library document), so the mean of the logs is off by (m + 6) 2^-52 (1 + mean |log v|), which
is the relative error of its exp.
"""

from __future__ import annotations

import math

import numpy as np

from pcen_ref import C_ULP

U = 2.0 ** -24
F32 = np.float32
TINY = float(np.finfo(np.float32).tiny)
DENORM = 2.0 ** -149
SECOND_ORDER = 1.0 + 2.0 ** -10
LOG2E = 1.4426950408889634
MODES = ("connectivity", "distance", "affinity")
BANDWIDTHS = ("med_k_scalar", "mean_k", "gmean_k")


def default_k(n_eligible):
    t = max(int(n_eligible), 0)
    r = math.isqrt(t)
    return 2 * (r if r * r == t else r + 1)


def default_k_recurrence(n, width):
    return max(default_k(n - 2 * width + 1), 1)


def default_k_cross(n_ref):
    return max(default_k(n_ref), 1)


def max_width(n):
    """The largest width the kernels are tested with (the public function also refuses n == 2, where (n - 1) // 2 is 0)."""
    return max((n - 1) // 2, 1)


def eligible(D, width):
    n_ref, n = D.shape
    i, j = np.meshgrid(np.arange(n_ref), np.arange(n), indexing="ij")
    return (np.abs(i - j) >= width) & ~np.isnan(D)


def neighbours(D, k, width=0, full=False):
    """(mask (n_ref, n) of the neighbours, tau (n) float32, t (n) int32) of one float32 D."""
    D = np.asarray(D, F32)
    n_ref, n = D.shape
    ok = eligible(D, width)
    mask = np.zeros((n_ref, n), bool)
    tau = np.full(n, np.nan, F32)
    t = np.full(n, -1, np.int32)
    for j in range(n):
        idx = np.flatnonzero(ok[:, j])
        if idx.size == 0:
            continue
        col = D[idx, j] + F32(0.0)                           # -0 and +0 tie
        order = idx[np.argsort(col, kind="stable")]          # (D, i) ascending: idx is ascending and the sort stable
        chosen = order[:min(int(k), idx.size)]
        tau[j] = D[chosen[-1], j] + F32(0.0)
        t[j] = chosen[D[chosen, j] == tau[j]].max()
        mask[idx if full else chosen, j] = True
    return mask, tau, t


def bandwidth(tau, t, kind):
    """(value, bound): float32 and 0 for med_k_scalar (exact), float64 and the derived bound for the two means; NaN
    when no query has a neighbour."""
    kth = np.asarray(tau, F32)[np.asarray(t) >= 0]
    m = kth.size
    if m == 0:
        return F32(np.nan), 0.0
    if kind == "med_k_scalar":
        s = np.sort(kth)
        lo, hi = s[(m - 1) // 2], s[m // 2]
        with np.errstate(over="ignore", invalid="ignore"):
            return (lo if m % 2 else F32(F32(lo + hi) * F32(0.5))), 0.0
    v = kth.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "mean_k":
            mean = v.sum() / m
            return mean, abs(mean) * (U + (m + 2) * 2.0 ** -53) * SECOND_ORDER + DENORM
        if kind == "gmean_k":
            if (v < 0.0).any():
                return F32(np.nan), 0.0                      # (a cosine distance can round below 0)
            if (v == 0.0).any():
                return 0.0, 0.0                              # log 0 = -inf, exp -inf = 0: exact
            logs = np.log(v)
            g = float(np.exp(logs.sum() / m))
            rel = U + (m + 6) * 2.0 ** -52 * (1.0 + float(np.abs(logs).mean()))
            return g, abs(g) * rel * SECOND_ORDER + DENORM
    raise ValueError(kind)


def affinity(D, bw):
    """(a float64, bound) of exp(-D / bw) for float32 D and the bandwidth the kernel gets (a float32 estimate or the
    caller's float64)."""
    D = np.asarray(D, F32).astype(np.float64)
    bw = float(bw)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.abs(D * LOG2E / bw)
        a = np.exp(-D / bw)
        grow = np.where(np.isfinite(p), np.expm1(math.log(2.0) * p * (2 * U + U * U)), 0.0)
        bound = np.where(a > 0.0, a * (grow + C_ULP * U) * SECOND_ORDER, 0.0) + TINY
    return a, bound


def matrix(D, k, *, width=0, mode="connectivity", full=False, sym=False, self_diag=False, bw=None):
    """R (n_ref, n) of one float32 D: bool for connectivity, float32 for distance (both exact); for affinity
    (float64 values, bound) with the bandwidth bw.  Also returns (tau, t)."""
    D = np.asarray(D, F32)
    mask, tau, t = neighbours(D, k, width, full)
    if sym:
        mask = mask & mask.T
    diag = np.eye(D.shape[0], D.shape[1], dtype=bool) & bool(self_diag)
    if mode == "connectivity":
        return mask | diag, tau, t
    if mode == "distance":
        R = np.where(mask, D, F32(0.0)).astype(F32)
        R[diag] = 0.0
        return R, tau, t
    a, bound = affinity(D, bw)
    a = np.where(mask, a, 0.0)
    bound = np.where(mask, bound, 0.0)
    a[diag] = 1.0
    bound[diag] = 0.0
    return (a, bound), tau, t


def check_affinity(got, want, bound, what=""):
    """Asserts |got - want| <= bound everywhere and that exactly the cells outside the selection are 0; returns the
    worst error / bound."""
    got = np.asarray(got)
    assert got.dtype == F32 and np.isfinite(got).all(), f"{what}: not finite float32"
    assert (got[bound == 0.0] == want[bound == 0.0].astype(F32)).all(), f"{what}: a cell outside the selection, or the diagonal, is off"
    ratio = np.abs(got.astype(np.float64) - want) / np.maximum(bound, DENORM)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"{what}: worst error / bound {worst:.3f} at {np.unravel_index(int(ratio.argmax()), ratio.shape)}"
    return worst


def to_lag(rec, pad=True):
    rec = np.asarray(rec)
    n = rec.shape[-1]
    tp = 2 * n if pad else n
    lag = np.zeros(rec.shape[:-2] + (tp, n), rec.dtype)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    lag[..., (i - j) % tp, j] = rec[..., i, j]
    return lag


def to_recurrence(lag):
    lag = np.asarray(lag)
    tp, n = lag.shape[-2:]
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.ascontiguousarray(lag[..., (i - j) % tp, j])


# ---------------------------------------------------------------------------------------------------------------------
# the model against sklearn (CPU, tie-free data): the selection is the one librosa gets from NearestNeighbors
# ---------------------------------------------------------------------------------------------------------------------
def sklearn_neighbours(ref, data, k, metric, width=0):
    """The neighbour mask (n_ref, n) from sklearn.neighbors.NearestNeighbors(algorithm="brute") on float64 features."""
    from sklearn.neighbors import NearestNeighbors

    n_ref, n = ref.shape[1], data.shape[1]
    nn = NearestNeighbors(n_neighbors=n_ref, metric=metric, algorithm="brute").fit(ref.T.astype(np.float64))
    order = nn.kneighbors(data.T.astype(np.float64), return_distance=False)          # (n, n_ref), nearest first
    mask = np.zeros((n_ref, n), bool)
    for j in range(n):
        keep = [i for i in order[j] if abs(int(i) - j) >= width][:k]
        mask[keep, j] = True
    return mask
