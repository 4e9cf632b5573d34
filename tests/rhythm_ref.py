"""Float64 NumPy restatement of the definitions rhythm.py implements (librosa.feature.tempogram, librosa.feature.tempo,
librosa.beat.beat_track, librosa.tempo_frequencies; librosa itself is not a dependency), a float32 NumPy route of the
tempogram that sets the tolerance, the `decisive` precondition of the exact-match tests and the case generators.
Shared by tests/test_emu_rhythm.py (the kernel source on the CPU emulator) and tests/test_gpu_rhythm.py."""

from __future__ import annotations

import functools

import numpy as np

EPS = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)

# ---- tempogram ------------------------------------------------------------------------------------------------------
TG_SHAPES = [(1, 1), (1, 2), (2, 5), (1, 63), (1, 64), (1, 65), (3, 130), (1, 431)]
TG_WAVE_W = [1, 2, 3, 8, 64, 344, 384, 385, 512]
TG_GENERAL_W = [513, 600]


def tempo_frequencies(n_bins, hop_length=512, sr=22050):
    bpm = np.full(n_bins, np.inf)
    bpm[1:] = 60.0 * sr / (hop_length * np.arange(1.0, n_bins))
    return bpm


def window_of(window, W):
    if isinstance(window, np.ndarray):
        assert window.shape == (W,)
        return window.astype(np.float64)
    from scipy.signal import get_window

    return get_window(window, W, fftbins=True).astype(np.float64)


def padded(e, W, center):
    """p of the definition, float64, along the last axis."""
    e = np.asarray(e, np.float64)
    if not center:
        return e
    h = W // 2
    return np.pad(e, [(0, 0)] * (e.ndim - 1) + [(h, h)], mode="linear_ramp", end_values=0)


def n_frames(n, W, center):
    return n if center else n - W + 1


def tempogram(e, W, center=True, window="hann", norm=np.inf):
    """(..., W, T) float64 by the definition: direct sums."""
    e = np.asarray(e, np.float64)
    w = window_of(window, W)
    p = padded(e, W, center)
    T = n_frames(e.shape[-1], W, center)
    assert T >= 1
    X = np.lib.stride_tricks.sliding_window_view(p, W, axis=-1)[..., :T, :] * w          # (..., T, W)
    ac = np.empty(e.shape[:-1] + (W, T))
    for k in range(W):
        ac[..., k, :] = np.sum(X[..., :W - k] * X[..., k:], axis=-1)
    return normalise(ac, norm)


def normalise(ac, norm):
    if norm is None:
        return ac
    assert norm == np.inf
    m = np.max(np.abs(ac), axis=-2, keepdims=True)
    return np.where(m < FLT_MIN, ac, ac / np.where(m < FLT_MIN, 1.0, m))


def tempogram_f32(e, W, center=True, window="hann", norm=np.inf):
    """The same formulas in float32 arrays, the autocorrelation by rfft / irfft at 1024 points (the next power of two
    >= 2 W beyond W = 512): the route whose error against float64 sets the tolerance of the kernels."""
    e = np.asarray(e, np.float32)
    w = window_of(window, W).astype(np.float32)
    h = W // 2
    n = e.shape[-1]
    if center and h:
        i = np.arange(h, dtype=np.float32)
        left = e[..., :1] * i / np.float32(h)
        right = e[..., -1:] * (np.float32(h - 1) - i) / np.float32(h)
        p = np.concatenate([left, e, right], axis=-1).astype(np.float32)
    else:
        p = e
    T = n_frames(n, W, center)
    X = (np.lib.stride_tricks.sliding_window_view(p, W, axis=-1)[..., :T, :] * w).astype(np.float32)
    N = 1024 if W <= 512 else 1 << int(np.ceil(np.log2(2 * W)))
    F = np.fft.rfft(X, n=N, axis=-1)
    assert F.dtype == np.complex64
    pw = (F.real * F.real + F.imag * F.imag).astype(np.float32)
    ac = np.fft.irfft(pw, n=N, axis=-1)[..., :W].astype(np.float32)
    ac = np.swapaxes(ac, -1, -2)
    if norm is None:
        return ac
    m = np.max(np.abs(ac), axis=-2, keepdims=True)
    return np.where(m < np.float32(FLT_MIN), ac, ac / np.where(m < np.float32(FLT_MIN), np.float32(1), m)).astype(np.float32)


def tg_envelope(shape, seed=0):
    """Non-negative envelopes with structure: a click train per row plus |N(0, 0.15)|; float32."""
    B, n = shape
    rng = np.random.default_rng(1000 * n + 10 * B + seed)
    e = np.abs(rng.normal(0.0, 0.15, shape))
    for b in range(B):
        period = (7, 11, 22)[b % 3]
        e[b, rng.integers(0, period)::period] += rng.uniform(0.6, 1.4)
    return e.astype(np.float32)


def array_window(W):
    return (0.25 + np.random.default_rng(W).random(W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tg_case(shape, W, center, norm_inf, window_kind):
    """(envelope float32, float64 reference, atol) of one tempogram case; computed once and shared (read-only).
    atol = max(8 x the float32 NumPy route's worst error against float64 on this case, 1e-6) on the normalised
    values; with norm=None the same relative to ac[0, t] per frame (the returned atol then has shape (..., 1, T))."""
    e = tg_envelope(shape)
    window = "hann" if window_kind == "hann" else array_window(W)
    norm = np.inf if norm_inf else None
    want = tempogram(e, W, center, window, norm)
    got32 = tempogram_f32(e, W, center, window, norm).astype(np.float64)
    if norm_inf:
        atol = max(8.0 * float(np.max(np.abs(got32 - want))), 1e-6)
    else:
        scale = np.maximum(np.abs(want[..., :1, :]), FLT_MIN)
        atol = max(8.0 * float(np.max(np.abs(got32 - want) / scale)), 1e-6) * scale
    for a in (e, want):
        a.setflags(write=False)
    return e, want, atol, window


# ---- tempo ------------------------------------------------------------------------------------------------------------
TEMPO_CASES = [(8, 130), (11, 130), (22, 130), (8, 431), (11, 431), (22, 431), (43, 431), (86, 431)]      # (period, n)


def click_train(n, period, seed=0, jitter=1, noise=0.15):
    rng = np.random.default_rng(seed + 7919 * period + n)
    o = np.abs(rng.normal(0.0, noise, n))
    start = int(rng.integers(0, period))
    pos = np.arange(start, n, period)
    pos = np.clip(pos + rng.integers(-jitter, jitter + 1, pos.shape), 0, n - 1)
    o[pos] += rng.uniform(0.8, 1.2, pos.shape)
    return o.astype(np.float32)


def log_prior(W, sr=22050, hop_length=512, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, prior=None):
    bpm = tempo_frequencies(W, hop_length, sr)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = -0.5 * ((np.log2(bpm) - np.log2(start_bpm)) / std_bpm) ** 2 if prior is None else np.array(prior.logpdf(bpm), np.float64)
    if max_tempo is not None:
        lp[:int(np.argmax(bpm < max_tempo))] = -np.inf
    lp[0] = -np.inf
    return lp


def tempo_scores(g, lp):
    """log1p(1e6 g[k]) + logprior[k] along axis -2 of g (..., W, n_col)."""
    return np.log1p(1e6 * np.asarray(g, np.float64)) + lp[:, None]


def tempo_pick(g, lp):
    """(picked index per column, is the pick decisive?): the best and the second-best score differ by more than
    64 x 2^-24 x max|score| (finite scores)."""
    s = tempo_scores(g, lp)
    idx = np.argmax(s, axis=-2)
    fin = np.where(np.isfinite(s), s, -np.inf)
    srt = np.sort(fin, axis=-2)
    best, second = srt[..., -1, :], srt[..., -2, :] if s.shape[-2] > 1 else -np.inf
    scale = np.max(np.abs(np.where(np.isfinite(s), s, 0.0)), axis=-2)
    return idx, bool(np.all(best - second > 64 * EPS * scale))


def tempo_window(ac_size=8.0, sr=22050, hop_length=512):
    return int(np.floor(ac_size * sr / hop_length))


# ---- beat tracking -----------------------------------------------------------------------------------------------------
BEAT_T = [1, 2, 3, 5, 63, 64, 65, 130, 431, 1000]
BEAT_P = [2, 3, 8, 22, 64, 200]
BEAT_KINDS = ["clicks", "random", "constant", "zero", "spike", "nan"]


def half(P):
    return int(np.rint(P / 2.0))


def taps(P):
    k = np.arange(-P, P + 1)
    return np.exp(-0.5 * (32.0 * k / P) ** 2)


def local_score(o, P, dtype=np.float64):
    """(o', L): L[i] = sum_{k=-P..P} taps[k] o'[i - k], o' = 0 outside the row; length T."""
    o = np.asarray(o, dtype)
    T = len(o)
    on = o / np.std(o, ddof=1)
    w = taps(P).astype(dtype)
    ext = np.concatenate([np.zeros(P, dtype), on, np.zeros(P, dtype)])
    L = np.array([np.dot(w[::-1], ext[i:i + 2 * P + 1]) for i in range(T)], dtype)
    return on, L


def degenerate(o):
    o = np.asarray(o, np.float64)
    return len(o) < 2 or not np.isfinite(o).all() or not o.any() or not np.std(o, ddof=1) > 0


def beat_stages(o, P, tightness=100.0, trim=True):
    """Every stage of the definition in float64, with the margins `decisive` needs.  None for a degenerate row."""
    if degenerate(o):
        return None
    o = np.asarray(o, np.float64)
    T = len(o)
    h = half(P)
    on, L = local_score(o, P)
    d = np.arange(2 * P, h - 1, -1)
    tx = -tightness * np.log(d / P) ** 2
    C = np.zeros(T)
    link = np.full(T, -1)
    dp_margin = np.full(T, np.inf)                      # best - second-best candidate per frame
    lmax = L.max()
    first = T
    for i in range(T):
        j = i - d
        v = tx + np.where(j >= 0, C[np.maximum(j, 0)], 0.0)
        c = int(np.argmax(v))                           # the first maximum: the largest d
        if len(v) > 1:
            dp_margin[i] = v[c] - np.max(np.delete(v, c))
        C[i] = L[i] + v[c]
        if first == T and L[i] >= 0.01 * lmax:
            first = i
        link[i] = i - d[c] if i >= first else -1
    M = np.zeros(T, bool)
    M[1:-1] = (C[1:-1] > C[:-2]) & (C[1:-1] >= C[2:])
    M[T - 1] = C[T - 1] > C[T - 2]
    st = dict(on=on, L=L, C=C, link=link, first=first, M=M, h=h, tx=tx, dp_margin=dp_margin,
              one_pct_margin=np.min(np.abs(L[:min(first + 1, T)] - 0.01 * lmax)), flank=np.abs(np.diff(C)), tail=-1,
              tail_margin=np.inf, trim_margin=np.inf, all_beats=np.zeros(0, int), beats=np.zeros(0, int), mask=np.zeros(T, bool))
    if not M.any():
        return st
    med = np.median(C[M])
    st["tail_margin"] = np.min(np.abs(2 * C[M] - med))
    ok = np.flatnonzero(M & (2 * C > med))
    if not len(ok):
        return st
    beats = [int(ok[-1])]
    while link[beats[-1]] >= 0:
        beats.append(int(link[beats[-1]]))
    beats = np.array(beats[::-1])
    Lb = np.concatenate([[0.0], L[beats], [0.0]])
    s = 0.5 * Lb[:-2] + Lb[1:-1] + 0.5 * Lb[2:]
    thr = 0.5 * np.sqrt(np.mean(s ** 2)) if trim else 0.0
    st.update(tail=int(ok[-1]), all_beats=beats, s=s, trim_margin=np.min(np.abs(s - thr)))
    keep = np.flatnonzero(s > thr)
    if len(keep):
        st["beats"] = beats[keep[0]:keep[-1] + 1]                # both ends inclusive
        st["mask"][st["beats"]] = True
    return st


def margin_threshold(st):
    return 64 * EPS * max(1.0, float(np.max(np.abs(st["C"]))))


def decisive_all(st):
    """The rule as the beat tracker's specification states it, plus the flanks: a float64 margin above
    thr = 64 x 2^-24 x max(1, max|C|) at EVERY argmax of the DP (all T frames), at every flank C[i] - C[i-1] (they decide
    the local maxima), at the 1 % first-beat test up to the first frame that passes, at the tail test of every local
    maximum and at the trim threshold of every beat."""
    thr = margin_threshold(st)
    return bool(np.all(st["dp_margin"] > thr) and np.all(st["flank"] > thr) and st["one_pct_margin"] > thr
                and st["tail_margin"] > thr and st["trim_margin"] > thr)


def decisive_chain(st):
    """The fallback for rows on which decisive_all cannot be met in 9 draws (long rows at long periods: neighbouring
    candidates differ by about tightness / P^2 while thr grows with max|C|).  Premise, asserted by the tests that use this
    rule wherever they see C: |C32 - C64| < thr / 2 at every frame.  Under it a comparison of two C-expressions whose
    float64 margin exceeds thr has the same outcome in float32.  Required, with margins above thr:
      * the argmax of the DP at every frame of the backtracked chain (the tail and every link before it).  Off the chain a
        near-tie may resolve either way: C[i] is the maximum, which moves by no more than its candidates do (the premise
        covers it), and that frame's link is never followed;
      * the 1 % first-beat test at every frame up to the first one that passes;
      * the flanks from the tail's to the end of the row: the tail stays a local maximum and no later frame becomes one
        (the whole row when there is no tail);
      * the tail test, where it decides: the tail is the LARGEST i that is a local maximum and passes, so the tail must
        pass and every local maximum after it must fail; what the maxima before it do is immaterial.  Before the tail,
        each of the r flanks within thr may add, remove or move one local maximum, so the set under the median changes
        by at most r members and every value by thr / 2: the median stays between the values r ranks below and above
        the middle ranks, give or take thr / 2.  2 C[tail] must exceed the upper end of that interval by 2 thr and
        2 C[i] of every later local maximum must stay 2 thr below its lower end (not decisive when r ranks leave the
        set);
      * the trim threshold at every beat of the chain."""
    thr = margin_threshold(st)
    tail = st["tail"]
    flank = st["flank"][max(tail - 1, 0):] if tail >= 0 else st["flank"]
    if not (np.all(st["dp_margin"][st["all_beats"]] > thr) and st["one_pct_margin"] > thr and np.all(flank > thr)
            and st["trim_margin"] > thr):
        return False
    if not st["M"].any():
        return bool(np.all(st["flank"] > thr))          # no local maximum may appear
    v = np.sort(st["C"][st["M"]])
    n = len(v)
    r = int(np.sum(st["flank"][:max(tail - 1, 0)] <= thr)) if tail >= 0 else 0
    lo_rank, hi_rank = (n - 1) // 2 - r, n // 2 + r
    if lo_rank < 0 or hi_rank > n - 1:
        return False
    if tail < 0:                                        # no tail: no local maximum may pass
        return bool(np.all(2 * st["C"][st["M"]] < v[lo_rank] - 2 * thr))
    later = np.flatnonzero(st["M"])
    later = later[later > tail]
    return bool(2 * st["C"][tail] > v[hi_rank] + 2 * thr and np.all(2 * st["C"][later] < v[lo_rank] - 2 * thr))


def decisive(st):
    """The precondition under the rule the case was drawn with (beat_case records it; decisive_all otherwise)."""
    return decisive_chain(st) if st.get("rule") == "chain" else decisive_all(st)


def beat_row(kind, T, P, seed):
    rng = np.random.default_rng(seed)
    if kind == "clicks":
        return click_train(T, P, seed=seed, jitter=1 if P > 3 else 0)
    if kind == "random":
        return rng.random(T).astype(np.float32)
    if kind == "constant":
        return np.full(T, 0.5, np.float32)
    if kind == "zero":
        return np.zeros(T, np.float32)
    if kind == "spike":                                 # one onset over a low floor
        o = np.abs(rng.normal(0.0, 0.01, T)).astype(np.float32)
        o[int(rng.integers(0, T))] = 1.0
        return o
    if kind == "bare_spike":                            # exact zeros around it: ties by construction (intermediates only)
        o = np.zeros(T, np.float32)
        o[int(rng.integers(0, T))] = 1.0
        return o
    if kind == "nan":
        o = rng.random(T).astype(np.float32)
        o[int(rng.integers(0, T))] = np.nan
        return o
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def beat_case(kind, T, P, tightness=100.0, trim=True):
    """(row float32, stages or None, redraws).  The row is redrawn (up to 8 times) until its float64 reference is decisive
    under decisive_all; only when none of the 9 draws is, the draws are walked again under decisive_chain.  stages["rule"]
    says which ("all" / "chain"); no row under either is a generator bug.  Degenerate rows (stages None) need no margin."""
    for rule, test in (("all", decisive_all), ("chain", decisive_chain)):
        for redraw in range(9):
            o = beat_row(kind, T, P, seed=100003 * redraw + 31 * T + P)
            st = beat_stages(o, P, tightness, trim)
            if st is None or test(st):
                if st is not None:
                    st["rule"] = rule
                o.setflags(write=False)
                return o, st, redraw
    raise AssertionError(f"generator bug: no decisive {kind} row of {T} frames at period {P} in 9 draws")


# the (T, P) on which some generator needs the fallback rule (decisive_chain): asserted by the tests, so that the rows
# that rest on it are named; every other case meets decisive_all
CHAIN_RULE_CASES = {(431, 200): {"clicks"}, (1000, 22): {"spike"}, (1000, 64): {"clicks", "random", "spike"},
                    (1000, 200): {"clicks", "random", "spike"}, (16384, 64): {"clicks"}}


def check_rule(kind, T, P, st, C32=None):
    """Asserts of a drawn case: its precondition holds; the fallback rule is used on the named rows only; where the
    float32 C is at hand, the fallback's premise |C32 - C64| < thr / 2."""
    assert decisive(st), (kind, T, P)
    if st["rule"] == "chain":
        assert kind in CHAIN_RULE_CASES.get((T, P), ()), (kind, T, P)
        if C32 is not None:
            worst = float(np.max(np.abs(C32 - st["C"])))
            assert worst < margin_threshold(st) / 2, (kind, T, P, worst, margin_threshold(st))


def L_bound(st, P):
    """|L32 - L64| <= (2P + 4) 2^-24 sum_k |taps[k] o'[i - k]| + FLT_MIN sum_{k: taps[k] < FLT_MIN} |o'[i - k]|.  The second
    term is float32's underflow and applies to the taps below FLT_MIN only (exp(-128) at P = 2 already): such a tap is
    not held to 2^-24 of its value, or is 0."""
    a = np.abs(st["on"])
    ext = np.concatenate([np.zeros(P), a, np.zeros(P)])
    w = taps(P)[::-1]
    tiny = (w < FLT_MIN).astype(np.float64)
    return np.array([(2 * P + 4) * EPS * np.dot(w, ext[i:i + 2 * P + 1]) + FLT_MIN * np.dot(tiny, ext[i:i + 2 * P + 1])
                     for i in range(len(a))])


def beat_dp_f32(o, P, tightness=100.0):
    """(L, C, link) by the kernel's float32 arithmetic: the deviation in float64 rounded once, taps and costs rounded once
    from float64, o' = o / std, L and C in float32 with every product and sum rounded (taps in index order, a term outside
    the row contributes an exact 0), the first maximum over d = 2P .. h.  For rows with exact ties (one onset among exact
    zeros), where float64 and float32 may break a tie between the two orders of the same two steps differently: this
    restatement reproduces float32's ties, so the links can be pinned."""
    f = np.float32
    o = np.asarray(o, f)
    T = len(o)
    h = half(P)
    std = f(np.sqrt(np.sum((o.astype(np.float64) - np.mean(o.astype(np.float64))) ** 2) / (T - 1)))
    on = (o / std).astype(f)
    w = taps(P).astype(f)
    ext = np.concatenate([np.zeros(P, f), on, np.zeros(P, f)])
    L = np.zeros(T, f)
    for k in range(-P, P + 1):                          # L[i] += tap[k] o'[i - k]
        L = (L + (w[k + P] * ext[P - k:P - k + T]).astype(f)).astype(f)
    d = np.arange(2 * P, h - 1, -1)
    tx = (-float(tightness) * np.log(d / P) ** 2).astype(f)
    C = np.zeros(T, f)
    link = np.full(T, -1)
    thr = f(0.01) * L.max()
    first = T
    for i in range(T):
        j = i - d
        v = (tx + np.where(j >= 0, C[np.maximum(j, 0)], f(0))).astype(f)
        c = int(np.argmax(v))
        C[i] = L[i] + v[c]
        if first == T and L[i] >= thr:
            first = i
        link[i] = i - d[c] if i >= first else -1
    return L, C, link


def C_bound(st, P, tightness):
    """C[i] = L[i] + (tx[d] + C[i - d]) is a chain of at most floor(i / h) + 1 links back to C[j < 0] = 0.  A link adds
    the error of its L (L_bound), the rounding of tx to float32 (2^-24 |tx| <= 2^-24 tightness ln(2)^2) and two
    additions (each 2^-24 of a partial result <= max|C| + max|tx|); the maximum of perturbed candidates moves by no more
    than the largest perturbation.  So |C32[i] - C64[i]| <= (floor(i / h) + 1) (max L_bound + 3 2^-24 (max|C| + tightness
    ln(2)^2))."""
    T = len(st["C"])
    txmax = tightness * np.log(2.0) ** 2
    per_link = float(np.max(L_bound(st, P))) + 3 * EPS * (float(np.max(np.abs(st["C"]))) + txmax)
    return (np.arange(T) // st["h"] + 1) * per_link
