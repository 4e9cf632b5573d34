"""References for phase_vocoder (test_gpu_phase_vocoder.py, tools/pv_bench.py): librosa 0.10's angle recurrence in
float64, a float32 twin of the phasor product (sequential, renormalised every step) whose error calibrates the bound,
and the inputs with their traps."""

import functools

import numpy as np

MARGIN = 4.0        # over the float32 twin's error: the kernel's log-depth scan multiplies in another order
# (B, F, T, rate, waves per row the launch must pick); F = 33 rows never reach the 4096 rows where every shape takes 1
CASES = [
    (1, 33, 1, 0.5, 1),             # a zero column is read
    (1, 33, 3, 4.0, 1),             # T_out = 1
    (1, 33, 70, 1.0, 1),            # identity across the 64-step chunk edge
    (1, 33, 70, 0.5, 1),            # two carries
    (1, 33, 200, 1.3, 1),
    (1, 33, 200, 2.0, 1),
    (1, 33, 200, 0.77, 1),
    (1, 33, 130, 1.0 / 3.0, 1),     # an inexact step: the arange length rule
    (1, 33, 300, 3.7, 1),           # a chunk's input span in two sub-spans
    (1, 33, 700, 1.25, 4),          # 9 chunks
    (1, 33, 3000, 0.9, 16),         # 53 chunks
]


def case_id(c):
    return f"B{c[0]}-F{c[1]}-T{c[2]}-rate{c[3]:.3g}-W{c[4]}"


def frames(T, rate):
    return len(np.arange(0, T, rate))


def make_input(B, F, T, seed=0):
    """Complex normal complex64 (B, F, T) with two all-zero columns (T >= 4), a zero row, a row times 1e-30 and a row
    times 1e+25; the zeros are +0.0."""
    rng = np.random.default_rng(seed)
    D = (rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))).astype(np.complex64)
    D[:, 2] *= np.float32(1e-30)
    D[:, 3] *= np.float32(1e25)
    if T >= 4:
        D[:, :, T // 3] = 0
        D[:, :, (2 * T) // 3] = 0
    D[:, 1] = 0
    return D


def pv64(D, rate):
    """librosa.phase_vocoder(D, rate=rate) with angles, in float64 on the complex64 values."""
    D = np.asarray(D).astype(np.complex128)
    F, T = D.shape[-2:]
    steps = np.arange(0, T, rate, dtype=np.float64)
    out = np.zeros(D.shape[:-1] + (len(steps),), np.complex128)
    phi = np.linspace(0, np.pi * ((2 * (F - 1)) // 4), F)
    acc = np.angle(D[..., 0])
    Dp = np.concatenate([D, np.zeros(D.shape[:-1] + (2,), np.complex128)], -1)
    for t, step in enumerate(steps):
        c0, c1 = Dp[..., int(step)], Dp[..., int(step) + 1]
        alpha = np.mod(step, 1.0)
        out[..., t] = ((1.0 - alpha) * np.abs(c0) + alpha * np.abs(c1)) * np.exp(1j * acc)
        d = np.angle(c1) - np.angle(c0) - phi
        acc = acc + phi + (d - 2.0 * np.pi * np.round(d / (2.0 * np.pi)))
    return out


def pv32(D, rate):
    """The phasor product in float32, one step after the other, the phasor renormalised at every step."""
    f = np.float32
    D = np.asarray(D).astype(np.complex64)
    T = D.shape[-1]
    Dp = np.concatenate([D, np.zeros(D.shape[:-1] + (2,), np.complex64)], -1)
    mag = np.abs(Dp).astype(f)
    safe = np.where(mag > 0, mag, f(1))
    ur = np.where(mag > 0, Dp.real / safe, f(1)).astype(f)
    ui = np.where(mag > 0, Dp.imag / safe, f(0)).astype(f)
    steps = np.arange(0, T, rate, dtype=np.float64)
    out = np.zeros(D.shape[:-1] + (len(steps),), np.complex64)
    pr, pi = ur[..., 0].copy(), ui[..., 0].copy()
    for t, step in enumerate(steps):
        i = int(step)
        a = f(step - np.floor(step))
        m = (f(1) - a) * mag[..., i] + a * mag[..., i + 1]
        out[..., t] = m * pr + 1j * (m * pi)
        qr = ur[..., i + 1] * ur[..., i] + ui[..., i + 1] * ui[..., i]
        qi = ui[..., i + 1] * ur[..., i] - ur[..., i + 1] * ui[..., i]
        pr, pi = pr * qr - pi * qi, pr * qi + pi * qr
        n = np.sqrt(pr * pr + pi * pi)
        pr, pi = pr / n, pi / n
    return out


@functools.lru_cache(maxsize=None)
def reference(B, F, T, rate):
    """(input, float64 result, the twin's error), computed once and shared: read-only.  The twin's error is relative to
    max |D| row by row, the worst row counting: one max |D| for rows that span 55 orders of magnitude would measure the
    row times 1e+25 alone (at T_out = 1 its two floats are exact: 8e-17, which the twin itself misses in every other row)."""
    D = make_input(B, F, T)
    want = pv64(D, rate)
    err = np.max(np.abs(pv32(D, rate) - want), axis=-1)
    rowmax = np.max(np.abs(D).astype(np.float64), axis=-1)
    twin = float(np.max(err[rowmax > 0] / rowmax[rowmax > 0]))
    for a in (D, want):
        a.setflags(write=False)
    return D, want, twin


def worst_ratio(got, D, want, twin):
    """max over rows of |got - want| / (twin error x the row's max |D|); the zero row must be exactly zero."""
    assert got.shape == want.shape and got.dtype == np.complex64
    err = np.max(np.abs(got.astype(np.complex128) - want), axis=-1)
    rowmax = np.max(np.abs(D).astype(np.float64), axis=-1)
    assert np.all(got[rowmax == 0] == 0)
    live = rowmax > 0
    return float(np.max(err[live] / (twin * rowmax[live])))
