"""The definitions of onset_strength, peak_pick and onset_detect (mlx-audio-primitives_amd/onset.py,
include/audioprims.h) in float64 NumPy, shared by test_emu_onset.py and test_gpu_onset.py.

  max_filter(S, size)            explicit reflect indices; == scipy.ndimage.maximum_filter1d(S, size, axis=-2)
  onset_strength(S, ...)         the flux, shifted and zero-filled to length T
  peak_pick(x, ...)              the literal loop
  onset_detect_frames(env, ...)  normalise, pick, backtrack: the bool mask of one row
  peak_rows(T, windows, ...)     the rows the peak-picking tests use, drawn until the reference alone is decisive
"""

import numpy as np

from hpss_ref import reflect

TINY = float(np.finfo(np.float32).tiny)
MARGIN = 1e-4


def max_filter(S, size):
    """R[..., m, t] = max S[..., reflect(j), t] over j in [m - size // 2, m + (size - 1) // 2]."""
    S = np.asarray(S)
    M = S.shape[-2]
    idx = reflect(np.arange(M)[:, None] - size // 2 + np.arange(size)[None, :], M)         # (M, size)
    return np.moveaxis(S, -2, -1)[..., idx].max(axis=-1).swapaxes(-1, -2)


def shift_of(lag, center=True, n_fft=2048, hop_length=512):
    return lag + (n_fft // (2 * hop_length) if center else 0)


def onset_strength(S, lag=1, max_size=1, ref=None, shift=None):
    """S (..., M, T) -> (..., T) float64."""
    S = np.asarray(S, np.float64)
    T = S.shape[-1]
    shift = lag if shift is None else shift
    R = np.asarray(ref, np.float64) if ref is not None else (S if max_size == 1 else max_filter(S, max_size))
    env = np.zeros(S.shape[:-2] + (T,), np.float64)
    if lag < T:
        flux = np.maximum(0.0, S[..., lag:] - R[..., :T - lag]).mean(axis=-2)             # (..., T - lag)
        n = T - shift
        if n > 0:
            env[..., shift:] = flux[..., :n]
    return env


def strength_bound(env64, M):
    """|env32 - env64| for non-negative terms in any order: one rounding for every difference, M - 1 for the sum, one
    for the division."""
    return (M + 2) * 2.0 ** -24 * env64


def candidates(x, pre_max, post_max, pre_avg, post_avg, delta):
    """(is candidate, passes the max test, x[n] - (mean + delta)) per frame, float64."""
    x = np.asarray(x, np.float64)
    T = len(x)
    cand, is_max, gap = np.zeros(T, bool), np.zeros(T, bool), np.zeros(T)
    for n in range(T):
        with np.errstate(invalid="ignore"):
            mx = np.max(x[max(0, n - pre_max):min(n + post_max, T)])
            av = np.mean(x[max(0, n - pre_avg):min(n + post_avg, T)])
        is_max[n] = x[n] == mx
        gap[n] = x[n] - (av + delta)
        cand[n] = is_max[n] and x[n] >= av + delta
    return cand, is_max, gap


def greedy(cand, wait):
    """From the left: a candidate is accepted iff it lies at least wait + 1 frames after the last accepted one."""
    out = np.zeros(len(cand), bool)
    last = None
    for n in np.flatnonzero(cand):
        if last is None or n >= last + wait + 1:
            out[n] = True
            last = n
    return out


def peak_pick(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    """Bool mask of one row: the literal loop."""
    return greedy(candidates(x, pre_max, post_max, pre_avg, post_avg, delta)[0], wait)


def normalize(x):
    x = np.asarray(x, np.float64)
    return (x - x.min()) / (x.max() - x.min() + TINY)


def local_minima(e):
    e = np.asarray(e, np.float64)
    T = len(e)
    return [0] + [k for k in range(1, T - 1) if e[k] <= e[k - 1] and e[k] < e[k + 1]]


def backtrack(mask, energy):
    mins = np.asarray(local_minima(energy))
    out = np.zeros(len(mask), bool)
    for n in np.flatnonzero(mask):
        out[mins[mins <= n].max()] = True
    return out


def seen(x, normalize_row):
    """The values peak-picking sees, float64, or None for a row that yields nothing under onset_detect's rule."""
    x = np.asarray(x, np.float32)
    if not np.all(np.isfinite(x)) or not x.any():
        return None
    return normalize(x) if normalize_row else x.astype(np.float64)


def onset_detect_frames(env, windows, delta, wait, normalize_row=True, do_backtrack=False, energy=None, guard=True):
    """Bool mask of one float32 row."""
    env = np.asarray(env, np.float32)
    x = seen(env, normalize_row) if guard else (normalize(env) if normalize_row else env.astype(np.float64))
    if x is None:
        return np.zeros(len(env), bool)
    mask = peak_pick(x, *windows, delta, wait)
    if do_backtrack:
        mask = backtrack(mask, x if energy is None else energy)
    return mask


def decisive(x, windows, delta, on_grid):
    """The precondition of an exact comparison of masks.  For every frame that passes the max test, x[n] - (mean +
    delta) is at least MARGIN away from zero (float32 sums of up to 201 values in [0, 8) are within 2e-4 / 16 of the
    float64 mean), or the comparison is exact in float32 and float64 alike: every value of the mean's window equals
    x[n] and their sum is exact, because the window holds one value, the value is zero, or the values lie on the
    1 / 4096 grid (`on_grid`: at most 15 bits each, 23 for 256 of them) - then mean == x[n] in both precisions, the gap
    is -delta, and `>=` decides a plateau the way it is written."""
    x = np.asarray(x, np.float64)
    T = len(x)
    _, is_max, gap = candidates(x, *windows, delta)
    for n in np.flatnonzero(is_max & (np.abs(gap) < MARGIN)):        # (a NaN gap is no candidate in any precision)
        w = x[max(0, n - windows[2]):min(n + windows[3], T)]
        if not (np.all(w == x[n]) and (len(w) == 1 or x[n] == 0.0 or on_grid) and (delta == 0.0 or abs(delta) >= MARGIN)):
            return False
    return True


def peak_rows(T, windows, deltas=(0.0, 0.07), seed=0):
    """Named float32 rows of length T: random ones on a grid of 1 / 4096 (so that distinct values stay distinct under the
    float32 normalisation and equal ones are exact ties), plateaus (runs of one to four equal values), a constant and an all-zero row,
    and one with NaNs (never normalised: NumPy's minimum would be NaN).  A random row is drawn again until the float64
    reference is decisive for it, raw and normalised, at every delta: the generator, not the test, does the
    re-drawing."""
    rng = np.random.default_rng(1000 * T + seed)
    rows = {}

    def ok(x, normalised=True):
        if not all(decisive(x, windows, d, True) for d in deltas):
            return False
        return not normalised or all(decisive(normalize(x), windows, d, False) for d in deltas)

    def draw(make, normalised=True):
        for _ in range(1000):
            x = make().astype(np.float32)
            if ok(x, normalised):
                return x
        raise AssertionError("no decisive row found")

    def grid(a):
        return np.floor(a * 4096.0) / 4096.0

    def with_nans():
        x = grid(rng.random(T) * 4.0)
        x[rng.integers(0, T, max(1, T // 40))] = np.nan
        return x

    rows["random"] = draw(lambda: grid(rng.random(T) * 4.0))
    rows["spiky"] = draw(lambda: grid(rng.random(T) ** 6 * 8.0 + 0.125))
    rows["plateaus"] = draw(lambda: np.repeat(grid(rng.random(T) * 2.0), rng.integers(1, 5, T))[:T])
    rows["constant"] = np.full(T, 0.75, np.float32)
    rows["zero"] = np.zeros(T, np.float32)
    rows["nan"] = draw(with_nans, normalised=False)
    for name in ("constant", "zero"):
        assert ok(rows[name]), name
    return rows


# ---- the cases test_emu_onset.py and test_gpu_onset.py share: computed once, never modified ---------------------------
SHAPES = [(1, 1, 2), (1, 3, 5), (2, 5, 63), (1, 7, 64), (1, 8, 65), (1, 128, 70), (1, 129, 130), (3, 4, 1)]
SHIFT_KINDS = [(True, 2048, 512), (False, 2048, 512), (True, 512, 128), (False, 512, 128)]

PEAK_T = [1, 2, 5, 63, 64, 65, 130, 1000]
PEAK_WINDOWS = [(0, 1, 0, 1), (1, 1, 4, 5), (3, 3, 3, 5), (30, 30, 100, 101)]
DELTAS = (0.0, 0.07)

_cache = {}


def lags(T):
    return sorted({1, 2, 5, max(T - 1, 1), T, T + 3})


def max_sizes(M):
    """2 M + 1 (the window wraps the whole axis, reflected twice) where the interface admits it: max_size <= 255."""
    return sorted({1, 2, 3, 4, 5, min(2 * M + 1, 255), 255})


def spectrum(shape):
    """A dB-like float32 array (about -80 .. 0), computed once, never modified."""
    if shape not in _cache:
        rng = np.random.default_rng(sum(shape))
        S = (-80.0 * rng.random(shape) ** 2).astype(np.float32)
        S.setflags(write=False)
        _cache[shape] = S
    return _cache[shape]


def strength_check(got, want, M, what):
    """Asserts the bound of strength_bound and exact zeros; returns the worst error over bound."""
    bound = strength_bound(want, M)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), (what, float(np.max(err - bound)))
    assert np.all(got[want == 0.0] == 0.0), what
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def rows_for(T, windows):
    key = ("rows", T, windows)
    if key not in _cache:
        rows = peak_rows(T, windows, DELTAS)
        for v in rows.values():
            v.setflags(write=False)
        _cache[key] = rows
    return _cache[key]
