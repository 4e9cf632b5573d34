"""The definition of the fused NNLS kernel in numpy, and the banks and inputs of its tests.  float64 is
the reference; float32 is the route whose own error against float64, measured once (F32_ERR), sets the kernel's bound."""

import functools

import numpy as np

N_ITERS = (0, 1, 32, 100)
BANKS = ("slaney-2048-128", "htk-400-80", "mel-64-8", "mel-256-128", "bark-512-24", "dense-5-33")
# err(fista(A, s, n, np.float32), fista(A, s, n)) on s = case(bank, 3, 17), measured once (NumPy 2, x86-64), per bank in the
# order of N_ITERS; the kernel is allowed 4 x these: another, fixed, summation order and fused multiply-adds
F32_ERR = dict(zip(((b, n) for b in BANKS for n in N_ITERS), (
    2.3e-07, 2.4e-07, 2.6e-06, 2.7e-05, 1.2e-07, 1.2e-07, 6.7e-07, 7.6e-06, 1.6e-07, 1.3e-07, 1.6e-06, 1.3e-05,
    8.7e-08, 8.7e-08, 9.9e-07, 2.8e-06, 2.5e-07, 2.5e-07, 2.9e-06, 2.9e-05, 3.2e-07, 3.5e-07, 2.5e-06, 1.8e-05)))


def inputs(A):
    """What the kernel is handed besides s: (P = pinv(A) float32, step = 1 / lambda_max(A A^T)), from float64."""
    A = A.astype(np.float64)
    return np.linalg.pinv(A).astype(np.float32), float(np.float32(1.0 / np.linalg.eigvalsh(A @ A.T)[-1]))


def fista(A, s, n_iter, dtype=np.float64):
    """x (.., F, T) >= 0 after n_iter accelerated projected-gradient steps on ||A x - s||^2 from max(P s, 0)."""
    P, step = inputs(A)
    A, P, s, step = A.astype(dtype), P.astype(dtype), s.astype(dtype), dtype(step)
    x = z = np.maximum(P @ s, 0)
    t = 1.0
    for _ in range(n_iter):
        x_new = np.maximum(z - step * (A.T @ (A @ z - s)), 0)
        t_new = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        z = x_new + dtype(np.float32((t - 1.0) / t_new)) * (x_new - x)
        x, t = x_new, t_new
    return x


def err(got, ref):
    """max over frames with a non-zero reference of max|got - ref| / max|ref|."""
    top = np.abs(ref).max(-2)
    return float((np.abs(got.astype(np.float64) - ref).max(-2)[top > 0] / top[top > 0]).max())


@functools.lru_cache(maxsize=None)
def bank(name):
    import mlx_audio_primitives_amd as ap
    kind, a, b = name.split("-")
    if kind == "dense":
        A = np.random.default_rng(5).random((int(a), int(b)), dtype=np.float32) + np.float32(0.01)
    elif kind == "bark":
        A = ap.bark_filterbank(16000, int(a), n_bands=int(b), device="cpu").numpy().copy()
    else:
        A = ap.mel_filterbank(22050, int(a), int(b), htk=kind == "htk", device="cpu").numpy().copy()
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def case(name, B, T):
    """s = A x_true (B, M, T) float32, x_true gamma(0.5) under a decaying envelope; the last frame of every clip is all
    zero and frame 0 has its middle mel row zeroed."""
    A = bank(name)
    rng = np.random.default_rng(7)
    x_true = rng.standard_gamma(0.5, (B, A.shape[1], T)).astype(np.float32) * np.exp(-4.0 * np.arange(A.shape[1]) / A.shape[1])[:, None]
    s = (A.astype(np.float64) @ x_true).astype(np.float32)
    if T > 1:
        s[:, :, -1] = 0
    s[:, A.shape[0] // 2, 0] = 0
    s.setflags(write=False)
    return s

