"""The definition of the sequence decoders (sequence.py, csrc/kernels_viterbi.h) in numpy.

Emissions, with tiny = np.finfo(np.float32).tiny (librosa's guard: a zero probability is -87.3, never -inf):

    viterbi                  E[t, j] = log(prob[j, t] + tiny)
    viterbi_discriminative   E[t, j] = log(prob[j, t] + tiny) - log(p_state[j] + tiny)
    viterbi_binary, label l  E[t, l, 1] = log(p + tiny) - log(p_state[l] + tiny)
                             E[t, l, 0] = log(1 - p + tiny) - log(1 - p_state[l] + tiny)

    lt[i, j] = float32(log(float64(transition[i, j]) + tiny)),   li[j] = float32(log(p_init[j] + tiny))

The float32 model (decode_f32): v_0 = E_0 + li; at t >= 1 ptr[t, j] = the smallest i maximising v[i] + lt[i, j] and
v'[j] = E[t, j] + that maximum; after every step (0 included) m_t = max_j v[j] is subtracted from v in float32 and added to
a float64 sum in time order; the last state is the first maximum of the final v, s[t] = ptr[t + 1, s[t + 1]], and
logp = the sum + float64(v[s[T - 1]]).  There is no multiplication: every operation is one rounded float32 addition, the
kernels' outputs equal this model in every bit.  decode_f64 is the plain float64 recursion on float64 emissions.

The emission bound (emission_bound).  u = 2^-24.  Against the float64 value of the definition on the float32 input p:
  * the argument a = fl(p + tiny) has a relative error <= u, so log a is off by <= u / (1 - u) < 1.001 u
    (state 0 of the binary mode rounds 1 - p first: twice that);
  * logf is within 3 ulp of log a (the OpenCL full-profile bound the device's math library is written to; glibc's is
    within 1): <= 3 * 2^-23 * (|L| + 1.001 u), L the exact log;
  * the float32 log prior differs from the float64 one by <= u |lp|, and the subtraction rounds once more:
    <= u (|E| + the errors above).
  bound = (e_log + u |lp|) (1 + u) + u |E|,  e_log = k 1.001 u + 3 * 2^-23 (|L| + k 1.001 u),  k = 1 (2 for state 0).

The path bound (path_bound).  Rounding to float32 is monotone, so fl(E + max_i fl(fl(v_i - m) + lt_ij)) is the maximum
over i of the same expression: the model returns exactly the path that maximises the sequentially rounded path score c(P)
(m_t is common to all paths of a step).  For every path |c(P) + sum m_t - score64(P)| <= T eps, where a step contributes
at most eps = max emission error + u max|lt| (lt's rounding) + 3 u R (the three rounded additions; every intermediate
is at most R = (max E - min E) + (max lt - min lt) + max|lt| + max|E| in magnitude, because after the renormalisation
max v = 0 and v >= min E + min lt - max E - max lt).  Hence score64(returned) >= score64(optimal) - 2 T eps.
"""

from __future__ import annotations

import numpy as np

TINY = float(np.finfo(np.float32).tiny)
U = 2.0 ** -24
LOGF_ULPS = 3.0
COLSUM_TOL = 1e-8 + 1e-5        # numpy's allclose(sum, 1)


# ---------------------------------------------------------------------------------------------------------------------
# transition builders (librosa.sequence.transition_*)
# ---------------------------------------------------------------------------------------------------------------------
def transition_uniform(n):
    return np.full((n, n), 1.0 / n, np.float64)


def transition_loop(n, prob):
    p = np.broadcast_to(np.asarray(prob, np.float64), (n,))
    out = np.empty((n, n), np.float64)
    for i in range(n):
        out[i] = (1.0 - p[i]) / (n - 1)
        out[i, i] = p[i]
    return out


def transition_cycle(n, prob):
    p = np.broadcast_to(np.asarray(prob, np.float64), (n,))
    out = np.zeros((n, n), np.float64)
    for i in range(n):
        out[i, (i + 1) % n] = 1.0 - p[i]
        out[i, i] = p[i]
    return out


def triangle(M):
    """scipy.signal.get_window("triangle", M, fftbins=False)."""
    n = np.arange(1, (M + 1) // 2 + 1, dtype=np.float64)
    if M % 2 == 0:
        w = (2 * n - 1.0) / M
        return np.concatenate([w, w[::-1]])
    w = 2 * n / (M + 1.0)
    return np.concatenate([w, w[-2::-1]])


def transition_local(n, width, window=triangle, wrap=False):
    """`window`: a function of the length.  Row i: the window centred on i (cut at the edges, or wrapped), normalised."""
    widths = np.broadcast_to(np.asarray(width, np.int64), (n,))
    out = np.zeros((n, n), np.float64)
    for i, w in enumerate(widths):
        row = np.zeros(n, np.float64)
        lpad = (n - w) // 2
        row[lpad:lpad + w] = window(int(w))
        row = np.roll(row, n // 2 + i + 1)
        if not wrap:
            row[min(n, i + w // 2 + 1):] = 0
            row[:max(0, i - w // 2)] = 0
        out[i] = row
    return out / out.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------
# parameters and emissions
# ---------------------------------------------------------------------------------------------------------------------
def log32(x):
    """float32(log(float64(x) + tiny))."""
    return np.log(np.asarray(x, np.float64) + TINY).astype(np.float32)


def log_state(p_state, binary=False):
    """lps of the emission kernel: (S) float32, or (S, 2) with [l, 0] = log(1 - p + tiny), [l, 1] = log(p + tiny)."""
    p = np.asarray(p_state, np.float64)
    return np.stack([log32(1.0 - p), log32(p)], axis=-1) if binary else log32(p)


def emissions64(prob, mode, p_state=None):
    """The float64 emissions of prob (S, T) (float32 values): (T, S), or (T, S, 2) for mode 2."""
    p = np.asarray(prob, np.float32).astype(np.float64).T
    if mode == 0:
        return np.log(p + TINY)
    ps = np.asarray(p_state, np.float64)
    if mode == 1:
        return np.log(p + TINY) - np.log(ps + TINY)[None, :]
    return np.stack([np.log(1.0 - p + TINY) - np.log(1.0 - ps + TINY)[None, :], np.log(p + TINY) - np.log(ps + TINY)[None, :]], axis=-1)


def emissions32(prob, mode, p_state=None):
    """The emission kernel's arithmetic with numpy's float32 log standing in for logf."""
    p = np.asarray(prob, np.float32).T
    tiny = np.float32(TINY)
    e1 = np.log(p + tiny)
    if mode == 0:
        return e1
    if mode == 1:
        return e1 - log_state(p_state)[None, :]
    lps = log_state(p_state, True)
    return np.stack([np.log((np.float32(1) - p) + tiny) - lps[None, :, 0], e1 - lps[None, :, 1]], axis=-1)


def emission_bound(prob, mode, p_state=None):
    """The bound derived in the module docstring, shaped like emissions64."""
    p = np.asarray(prob, np.float32).astype(np.float64).T

    def one(L, lp, k):
        e_log = k * 1.001 * U + LOGF_ULPS * 2.0 ** -23 * (np.abs(L) + k * 1.001 * U)
        return (e_log + U * np.abs(lp)) * (1 + U) + U * np.abs(L - lp)

    if mode == 0:
        return one(np.log(p + TINY), 0.0, 1)
    ps = np.asarray(p_state, np.float64)
    if mode == 1:
        return one(np.log(p + TINY), np.log(ps + TINY)[None, :], 1)
    return np.stack([one(np.log(1.0 - p + TINY), np.log(1.0 - ps + TINY)[None, :], 2), one(np.log(p + TINY), np.log(ps + TINY)[None, :], 1)], axis=-1)


def emission_flags(prob, mode):
    """The flag word of one sequence prob (S, T)."""
    p = np.asarray(prob, np.float32)
    flag = 0 if ((p >= 0) & (p <= 1)).all() else 1
    if mode == 1 and not (np.abs(p.astype(np.float64).sum(axis=0) - 1.0) <= COLSUM_TOL).all():
        flag |= 2
    return flag


# ---------------------------------------------------------------------------------------------------------------------
# decoders
# ---------------------------------------------------------------------------------------------------------------------
def decode_f32(E, lt, li):
    """The float32 model on E (T, S), lt (S, S), li (S) float32: (ptr uint16 (T, S), states int32 (T), logp float64)."""
    E, lt, li = (np.asarray(a, np.float32) for a in (E, lt, li))
    T, S = E.shape
    ptr = np.zeros((T, S), np.uint16)
    v = E[0] + li
    m = v.max()
    acc = np.float64(m)
    v = v - m
    for t in range(1, T):
        cand = v[:, None] + lt
        ptr[t] = cand.argmax(axis=0)
        v = E[t] + cand.max(axis=0)
        m = v.max()
        acc = acc + np.float64(m)
        v = v - m
    assert v.dtype == np.float32
    states = np.empty(T, np.int32)
    states[-1] = int(v.argmax())
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return ptr, states, np.float64(acc + np.float64(v[states[-1]]))


def decode_binary_f32(E, lt, li):
    """The float32 model of the binary decode on E (T, S, 2), lt (2, 2) or (S, 2, 2), li (S, 2):
    (bits uint32 (ceil(T / 16), S), states int32 (S, T), logp float64 (S))."""
    E, lt, li = (np.asarray(a, np.float32) for a in (E, lt, li))
    T, S, _ = E.shape
    lt = np.broadcast_to(lt.reshape(-1, 2, 2), (S, 2, 2))
    ptr = np.zeros((T, S, 2), np.uint32)
    v = E[0] + li
    m = v.max(axis=1)
    acc = m.astype(np.float64)
    v = v - m[:, None]
    for t in range(1, T):
        cand = v[:, :, None] + lt
        ptr[t] = cand.argmax(axis=1)
        v = E[t] + cand.max(axis=1)
        m = v.max(axis=1)
        acc = acc + m.astype(np.float64)
        v = v - m[:, None]
    assert v.dtype == np.float32
    states = np.empty((S, T), np.int32)
    states[:, -1] = v.argmax(axis=1)
    lab = np.arange(S)
    for t in range(T - 2, -1, -1):
        states[:, t] = ptr[t + 1, lab, states[:, t + 1]]
    bits = np.zeros(((T + 15) // 16, S), np.uint32)
    for t in range(T):
        bits[t // 16] |= (ptr[t, :, 0] | (ptr[t, :, 1] << np.uint32(1))) << np.uint32(2 * (t % 16))
    return bits, states, acc + v[lab, states[:, -1]].astype(np.float64)


def decode_f64(E, lt, li):
    """The plain float64 recursion on float64 E (T, S), lt (S, S), li (S): (states int32 (T), logp)."""
    E, lt, li = (np.asarray(a, np.float64) for a in (E, lt, li))
    T, S = E.shape
    ptr = np.zeros((T, S), np.int64)
    v = E[0] + li
    for t in range(1, T):
        cand = v[:, None] + lt
        ptr[t] = cand.argmax(axis=0)
        v = E[t] + cand.max(axis=0)
    states = np.empty(T, np.int32)
    states[-1] = int(v.argmax())
    for t in range(T - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return states, float(v[states[-1]])


def path_score(E, lt, li, states):
    """The float64 score of a path: li[s_0] + E[0, s_0] + sum_t lt[s_(t-1), s_t] + E[t, s_t]."""
    E, lt, li = (np.asarray(a, np.float64) for a in (E, lt, li))
    s = np.asarray(states, np.int64)
    t = np.arange(len(s))
    return float(li[s[0]] + E[t, s].sum() + lt[s[:-1], s[1:]].sum())


def path_bound(T, emission_err, E, lt):
    """2 T eps of the module docstring: emission_err is the largest emission error, E and lt the float64 scores."""
    E, lt = np.asarray(E, np.float64), np.asarray(lt, np.float64)
    R = (E.max() - E.min()) + (lt.max() - lt.min()) + np.abs(lt).max() + np.abs(E).max()
    return 2.0 * T * (float(emission_err) + U * np.abs(lt).max() + 3 * U * R)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def random_problem(S, T, seed=0, B=None, normalise=False):
    """Uniform random prob (S, T) (or (B, S, T)) float32, a random row-normalised transition, uniform p_init:
    default_rng(seed).  normalise: the columns of prob sum to 1 (viterbi_discriminative)."""
    rng = np.random.default_rng(seed)
    prob = rng.uniform(size=((S, T) if B is None else (B, S, T)))
    if normalise:
        prob = prob / prob.sum(axis=-2, keepdims=True)
    trans = rng.uniform(size=(S, S))
    trans /= trans.sum(axis=1, keepdims=True)
    return prob.astype(np.float32), trans, np.full(S, 1.0 / S)


SEEDED_SHAPES = ((2, 200), (5, 300), (65, 257), (300, 64))
