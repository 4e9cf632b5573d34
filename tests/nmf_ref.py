"""The definition of nmf in numpy: the multiplicative updates, the objectives and the inputs of the
tests.  Never touches the package.  dtype=float64 is the reference, dtype=float32 the route whose own error sets the
five-iteration bound.

The one-step bound (`one_step_bounds`), per element and relative, u = 2^-24, g(n) = n u / (1 - n u).  Every term is
non-negative, so a float32 dot product of n terms, in any order, fused or not, is the exact one times (1 + d), |d| <= g(n)
(Higham, Accuracy and Stability of Numerical Algorithms, 3.1); adding eps, a product and a quotient cost one u each.
  Frobenius H:  the numerator W^T V has g(F); (W^T W) has g(F), times H summed over K: g(F + K), plus eps: g(F + K + 1);
                H * num / den adds two roundings:           e_H = (1 + g(F + 2)) / (1 - g(F + K + 1)) - 1
  KL H:         W H + eps has g(K + 1), the ratio (1 + u) / (1 - g(K + 1)); W^T ratio adds g(F); W^T 1 + eps has g(F + 1):
                                                            e_H = (1 + g(F + 2)) (1 + u) / ((1 - g(K + 1)) (1 - g(F + 1))) - 1
  W:            the mirror with T for F, on an H that is already off by e_H where the reference's is not.  A relative
                change of e_H in every element of H changes V H^T by at most (1 + e_H), H H^T by (1 + e_H)^2 either way,
                W H by (1 +- e_H) and the sums of H by (1 +- e_H); eps only dampens that.  So
                Frobenius  e_W = (1 + e_H) (1 + g(T + 2)) / ((1 - e_H)^2 (1 - g(T + K + 1))) - 1
                KL         e_W = (1 + e_H) (1 + g(T + 2)) (1 + u) / ((1 - e_H)^2 (1 - g(K + 1)) (1 - g(T + 1))) - 1
That is (2 F + K + 3) u for H and about (2 T + K + 3) u + 3 e_H for W, to first order; used with no factor on top."""

import functools

import numpy as np

U = 2.0 ** -24
EPS = float(np.float32(1e-10))                  # what the kernels add: the float32 nearest to 1e-10
SHAPES = [(1, 33, 70, 3), (3, 130, 97, 17), (1, 257, 200, 64), (2, 5, 3, 1)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
LOSSES = ["frobenius", "kullback-leibler"]


def g(n):
    return n * U / (1.0 - n * U)


def one_step_bounds(F, T, K, loss):
    """(e_H, e_W): the relative bounds of the docstring for one iteration from exact inputs."""
    if loss == "frobenius":
        e_h = (1 + g(F + 2)) / (1 - g(F + K + 1)) - 1
        e_w = (1 + e_h) * (1 + g(T + 2)) / ((1 - e_h) ** 2 * (1 - g(T + K + 1))) - 1
    else:
        e_h = (1 + g(F + 2)) * (1 + U) / ((1 - g(K + 1)) * (1 - g(F + 1))) - 1
        e_w = (1 + e_h) * (1 + g(T + 2)) * (1 + U) / ((1 - e_h) ** 2 * (1 - g(K + 1)) * (1 - g(T + 1))) - 1
    return e_h, e_w


def update_h(V, W, H, loss, eps):
    Wt = np.swapaxes(W, -1, -2)
    if loss == "frobenius":
        return H * (Wt @ V) / ((Wt @ W) @ H + eps)
    return H * (Wt @ (V / (W @ H + eps))) / (W.sum(-2)[..., None] + eps)


def update_w(V, W, H, loss, eps):
    Ht = np.swapaxes(H, -1, -2)
    if loss == "frobenius":
        return W * (V @ Ht) / (W @ (H @ Ht) + eps)
    return W * ((V / (W @ H + eps)) @ Ht) / (H.sum(-1)[..., None, :] + eps)


def iterate(V, W, H, loss, n_iter=1, update_components=True, dtype=np.float64):
    V, W, H, eps = V.astype(dtype), W.astype(dtype), H.astype(dtype), dtype(EPS)
    for _ in range(n_iter):
        H = update_h(V, W, H, loss, eps)
        if update_components:
            W = update_w(V, W, H, loss, eps)
    return W, H


def objective(V, W, H, loss):
    """Per item, float64: ||V - W H||_F^2, or sum V log(V / (W H + eps)) - V + W H with 0 log 0 = 0."""
    V, P = V.astype(np.float64), W.astype(np.float64) @ H.astype(np.float64)
    if loss == "frobenius":
        return ((V - P) ** 2).sum((-1, -2))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.where(V > 0, V * np.log(V / (P + EPS)), 0.0) - V + P).sum((-1, -2))


@functools.lru_cache(maxsize=None)
def case(shape):
    """(V, W0, H0) float32, read-only: low rank plus noise, and scikit-learn's random initialisation."""
    B, F, T, K = shape
    rng = np.random.default_rng(0)
    A, C, N = rng.random((B, F, K)), rng.random((B, K, T)), rng.random((B, F, T))
    V = (A ** 4 @ C ** 2 + 0.01 * N).astype(np.float32)
    s = np.sqrt(V.mean((-1, -2), keepdims=True) / K)
    W0 = (s * np.abs(rng.standard_normal((B, F, K)))).astype(np.float32)
    H0 = (s * np.abs(rng.standard_normal((B, K, T)))).astype(np.float32)
    for a in (V, W0, H0):
        a.setflags(write=False)
    return V, W0, H0


def rel_err(x, ref):
    """The worst relative error per element (the reference's elements are positive for the inputs of `case`)."""
    return float((np.abs(x.astype(np.float64) - ref) / ref).max())
