"""Sequence decoding: hidden-Markov Viterbi decoders and transition-matrix builders (no counterpart in the reference; the
signatures of librosa 0.10's librosa.sequence).

Three kernels (csrc/kernels_viterbi.h):

    emission   prob (B, S, T) -> time-major log emissions, transposed through LDS; one flag word per sequence
    decode     one workgroup per sequence: v in LDS, uint16 back-pointers, the backtrack in the same launch
    binary     one lane per (sequence, label) two-state chain, two pointer bits per step

With tiny = the smallest normal float32 (librosa's guard: a zero probability costs -87.3, it is not forbidden):

    viterbi                  E[t, j] = log(prob[j, t] + tiny)
    viterbi_discriminative   E[t, j] = log(prob[j, t] + tiny) - log(p_state[j] + tiny)
    viterbi_binary           E[t, l, 1] = log(p + tiny) - log(p_state[l] + tiny),  E[t, l, 0] the same of 1 - p and 1 - p_state[l]

and the decode is v_0 = E_0 + log(p_init + tiny), v_t[j] = E[t, j] + max_i (v_(t-1)[i] + log(transition[i, j] + tiny)) with
ties going to the smallest i, the last state the first maximum of v_(T-1).  transition, p_init and p_state are host data:
validated on the host with librosa's rules, their logs taken in float64, rounded to float32 and cached per device under
their content.  Only prob is read on the device.

Deviations from librosa, on purpose.  The arithmetic is float32, not float64: after every step the maximum of v is
subtracted from v and summed in float64, so the float32 spacing stays near the spread of the values instead of near
87 T, and the results equal the sequential float32 model (tests/viterbi_ref.py) in every bit.  States come back as int32,
not uint16.  The dense decoders take at most ap_viterbi_max_states() states and every decoder at most
ap_viterbi_max_steps() steps.  The values of prob are checked by the emission kernel (flag words, read once after
everything is enqueued: the one synchronisation, skipped with check=False).  Errors are ValueError, not ParameterError.
No parity with librosa's numbers is claimed beyond what the tests pin against the float64 definition.
"""

from __future__ import annotations

import hashlib

import numpy as np
import torch

from . import _extension as _x
from .onset import _rows

_TINY = float(np.finfo(np.float32).tiny)
_param_cache: dict[tuple, tuple] = {}


# ---------------------------------------------------------------------------------------------------------------------
# transition builders (host, float64)
# ---------------------------------------------------------------------------------------------------------------------
def _n_states(n_states, at_least):
    if isinstance(n_states, bool) or not isinstance(n_states, (int, np.integer)) or n_states < at_least:
        raise ValueError(f"n_states={n_states!r} must be an integer >= {at_least}")
    return int(n_states)


def _self_prob(prob, n):
    p = np.asarray(prob, np.float64)
    if p.ndim == 0:
        p = np.full(n, float(p))
    if p.shape != (n,):
        raise ValueError(f"prob={prob!r} must have length equal to n_states={n}")
    if not ((p >= 0) & (p <= 1)).all():
        raise ValueError(f"prob={prob!r} must have values in the range [0, 1]")
    return p


def transition_uniform(n_states):
    """The (n_states, n_states) float64 matrix with every entry 1 / n_states."""
    n = _n_states(n_states, 1)
    return np.full((n, n), 1.0 / n, np.float64)


def transition_loop(n_states, prob):
    """Self-loop transitions: transition[i, i] = prob[i] (a number or one per state), the rest of a row shared equally
    among the other states.  float64 (n_states, n_states), n_states >= 2."""
    n = _n_states(n_states, 2)
    p = _self_prob(prob, n)
    out = np.repeat(((1.0 - p) / (n - 1))[:, None], n, axis=1)
    out[np.arange(n), np.arange(n)] = p
    return out


def transition_cycle(n_states, prob):
    """Cyclic transitions: transition[i, i] = prob[i], transition[i, (i + 1) mod n_states] = 1 - prob[i].  float64."""
    n = _n_states(n_states, 2)
    p = _self_prob(prob, n)
    out = np.zeros((n, n), np.float64)
    idx = np.arange(n)
    out[idx, (idx + 1) % n] = 1.0 - p
    out[idx, idx] = p
    return out


def _local_window(window, M: int) -> np.ndarray:
    """The symmetric window of M points in float64: "triangle" / "triang" and "boxcar" / "ones" / "rectangular" are built
    here, any other scipy.signal.get_window specification goes to SciPy where it is installed."""
    if isinstance(window, str) and window.lower() in ("triangle", "triang"):
        n = np.arange(1, (M + 1) // 2 + 1, dtype=np.float64)
        if M % 2 == 0:
            w = (2 * n - 1.0) / M
            return np.concatenate([w, w[::-1]])
        w = 2 * n / (M + 1.0)
        return np.concatenate([w, w[-2::-1]])
    if isinstance(window, str) and window.lower() in ("boxcar", "ones", "rectangular"):
        return np.ones(M, np.float64)
    if isinstance(window, (str, tuple, float, int)) and not isinstance(window, bool):
        try:
            from scipy.signal import get_window as _scipy_window
        except ImportError as e:
            raise ValueError(f"window {window!r} is not one the library builds (triangle, boxcar) and SciPy is not installed") from e
        return np.asarray(_scipy_window(window, M, fftbins=False), np.float64)
    raise TypeError(f"window must be a name, a tuple or a number, got {type(window).__name__}")


def transition_local(n_states, width, *, window="triangle", wrap=False):
    """Band-limited transitions: row i is `window` of width[i] points (a number or one per state) centred on state i,
    cut off at the ends of the state space or, with wrap, continued around it, and normalised.  float64."""
    n = _n_states(n_states, 2)
    w = np.asarray(width)
    if w.dtype.kind not in "iu" or w.ndim > 1:
        raise ValueError(f"width={width!r} must be a positive integer or one per state")
    w = np.full(n, int(w)) if w.ndim == 0 else w.astype(np.int64)
    if w.shape != (n,):
        raise ValueError(f"width={width!r} must have length equal to n_states={n}")
    if (w < 1).any() or (w > n).any():
        raise ValueError(f"width={width!r} must lie in [1, n_states={n}]")
    out = np.zeros((n, n), np.float64)
    for i, wi in enumerate(w.tolist()):
        row = np.zeros(n, np.float64)
        lpad = (n - wi) // 2
        row[lpad:lpad + wi] = _local_window(window, wi)
        row = np.roll(row, n // 2 + i + 1)
        if not wrap:
            row[min(n, i + wi // 2 + 1):] = 0
            row[:max(0, i - wi // 2)] = 0
        out[i] = row
    return out / out.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------
# validation (no device)
# ---------------------------------------------------------------------------------------------------------------------
def _host64(a, name):
    """A host parameter as float64 numpy (a device tensor is copied to the host)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    try:
        a = np.asarray(a)
        if a.dtype.kind not in "fiu":
            raise TypeError
        return a.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an array of real numbers") from None


def _prob_tensor(prob, binary):
    if not isinstance(prob, torch.Tensor):
        prob = torch.as_tensor(np.asarray(prob))
    if prob.is_complex() or prob.dtype == torch.bool:
        raise ValueError(f"prob must be real, got {prob.dtype}")
    if binary and prob.ndim == 1:
        prob = prob[None]
    if prob.ndim < 2:
        raise ValueError(f"prob must be (n_states, n_steps) or (..., n_states, n_steps), got {prob.ndim}D")
    if 0 in prob.shape:
        raise ValueError(f"prob must not be empty, got shape {tuple(prob.shape)}")
    return prob


def _check_transition(t, shape, name="transition"):
    if t.shape != shape:
        raise ValueError(f"{name}.shape={t.shape}, must be (n_states, n_states)={shape}")
    if not np.isfinite(t).all() or (t < 0).any() or not np.allclose(t.sum(axis=-1), 1):
        raise ValueError(f"Invalid {name}: must be non-negative and sum to 1 on each row.")


def _check_dist(p, S, name, sums_to_one):
    if p.shape != (S,):
        raise ValueError(f"Invalid {name}: shape {p.shape} must be (n_states,)=({S},)")
    if not ((p >= 0) & (p <= 1)).all():
        raise ValueError(f"Invalid {name}: values must lie in [0, 1]")
    if sums_to_one and not np.allclose(p.sum(), 1):
        raise ValueError(f"Invalid {name}: must be a probability distribution (sum to 1)")


def _check_caps(S, T, dense):
    lib = _x.lib()
    cap_s, cap_t = int(lib.ap_viterbi_max_states()), int(lib.ap_viterbi_max_steps())
    if dense and S > cap_s:
        raise ValueError(f"n_states={S} is above the kernel's cap of {cap_s}")
    if T > cap_t:
        raise ValueError(f"n_steps={T} is above the kernel's cap of {cap_t}")


def _log32(x):
    return np.ascontiguousarray(np.log(x + _TINY).astype(np.float32))


def _on_device_cached(arrays, dev):
    """float32 host arrays (or None) on `dev`, cached under their content (bounded, oldest out first)."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(b"-" if a is None else a.tobytes() + repr(a.shape).encode())
    key = (h.digest(), str(dev))
    hit = _param_cache.get(key)
    if hit is None:
        hit = tuple(None if a is None else torch.from_numpy(a.copy()).to(dev) for a in arrays)
        if len(_param_cache) >= 32:
            _param_cache.pop(next(iter(_param_cache)))
        _param_cache[key] = hit
    return hit


# ---------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------
def _emissions(pt, mode, lps_host, extra_host):
    """prob on the device, its emissions and flags enqueued: (device, B, E, flags, `extra_host` on the device).  lps_host
    and extra_host are the float32 host parameters; they go to the device through the content cache."""
    S, T = int(pt.shape[-2]), int(pt.shape[-1])
    dev = pt.device if pt.is_cuda else _x.require_device()
    x = pt if (pt.is_cuda and pt.dtype == torch.float32) else pt.to(device=dev, dtype=torch.float32)
    x = x.reshape((-1, S, T))                                  # a padded-row view stays a view
    B = int(x.shape[0])
    x, rs = _rows(x)
    params = _on_device_cached((lps_host,) + tuple(extra_host), dev)
    E = torch.empty((B, T, S, 2) if mode == 2 else (B, T, S), dtype=torch.float32, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    _x.check(_x.dlib(dev).ap_viterbi_emission_f32(_x.ptr(x), B, S, T, rs, mode, None if params[0] is None else _x.ptr(params[0]),
                                                  _x.ptr(E), _x.ptr(flags), _x.stream_ptr(dev)))
    return dev, B, E, flags, params[1:]


def _raise_flags(flags, name, mode):
    """The one synchronisation of a call: the flag words of the emission kernel."""
    bad = flags.cpu().numpy()
    hit = np.flatnonzero(bad)
    if hit.size:
        b = int(hit[0])
        what = "holds a value outside [0, 1] (or a NaN)" if bad[b] & 1 else "has a column (a time step) that does not sum to 1"
        raise ValueError(f"Invalid prob for {name}: sequence {b} {what}")


def _dense(prob, transition, p_init, p_state, mode, name, return_logp, check):
    pt = _prob_tensor(prob, False)
    S, T = int(pt.shape[-2]), int(pt.shape[-1])
    trans = _host64(transition, "transition")
    _check_transition(trans, (S, S))
    if p_init is None:
        init = np.full(S, 1.0 / S)
    else:
        init = _host64(p_init, "p_init")
        _check_dist(init, S, "p_init", True)
    lps = None
    if mode == 1:
        if p_state is None:
            state = np.full(S, 1.0 / S)
        else:
            state = _host64(p_state, "p_state")
            _check_dist(state, S, "p_state", True)
        lps = _log32(state)
    _check_caps(S, T, True)
    dev, B, E, flags, (lt, li) = _emissions(pt, mode, lps, (_log32(trans), _log32(init)))
    ptr = torch.empty((B, T, S), dtype=torch.int16, device=dev)        # uint16 scratch
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    logp = torch.empty((B,), dtype=torch.float64, device=dev)
    _x.check(_x.dlib(dev).ap_viterbi_decode_f32(_x.ptr(E), B, S, T, _x.ptr(lt), _x.ptr(li), _x.ptr(ptr), _x.ptr(states), _x.ptr(logp),
                                                _x.stream_ptr(dev)))
    if check:
        _raise_flags(flags, name, mode)
    lead = tuple(pt.shape[:-2])
    states = states.reshape(lead + (T,))
    return (states, logp.reshape(lead)) if return_logp else states


def viterbi(prob, transition, *, p_init=None, return_logp=False, check=True):
    """Viterbi decoding from observation likelihoods (librosa.sequence.viterbi's signature).

    prob: (n_states, n_steps) or (..., n_states, n_steps), prob[j, t] = P(observation t | state j) in [0, 1].  A float32
    tensor on the device is read in place (rows may be padded); anything else is copied to the device.  transition:
    (n_states, n_states), non-negative, rows summing to 1, transition[i, j] = P(j at t + 1 | i at t); p_init:
    (n_states,) summing to 1, default uniform.  Both are host data: a tensor on the device is copied to the host.

    Returns the most likely states, int32 (..., n_steps); with return_logp also their log-likelihood, float64 (...).
    check (an addition to librosa's signature): read the emission kernel's flags back, the one synchronisation of the
    call, and raise ValueError naming the first sequence with a value outside [0, 1]; check=False skips it.  Everything
    runs on the input's device and current stream."""
    return _dense(prob, transition, p_init, None, 0, "viterbi", return_logp, check)


def viterbi_discriminative(prob, transition, *, p_state=None, p_init=None, return_logp=False, check=True):
    """Viterbi decoding from state posteriors (librosa.sequence.viterbi_discriminative's signature).

    prob: (n_states, n_steps) or (..., n_states, n_steps), prob[j, t] = P(state j | observation t): in [0, 1] and every
    column sums to 1 (to 1e-8 + 1e-5, numpy's allclose).  p_state: (n_states,) the marginal of the states, summing to 1,
    default uniform; transition, p_init, return_logp, check and the outputs as for viterbi (the flags also name a
    sequence with a column that does not sum to 1).  transition, p_state and p_init are host data: a tensor on the device
    is copied to the host."""
    return _dense(prob, transition, p_init, p_state, 1, "viterbi_discriminative", return_logp, check)


def viterbi_binary(prob, transition, *, p_state=None, p_init=None, return_logp=False, check=True):
    """Independent binary (multi-label) Viterbi decoding (librosa.sequence.viterbi_binary's signature).

    prob: (n_labels, n_steps) or (..., n_labels, n_steps) (or (n_steps,): one label), prob[l, t] = P(label l active |
    observation t) in [0, 1]; every label is its own chain of two states.  transition: (2, 2) shared, or (n_labels, 2, 2),
    each a valid transition matrix; p_state, p_init: a number or (n_labels,) in [0, 1], the marginal and the initial
    probability of the active state, default 0.5.  All three are host data: a tensor on the device is copied to the host.

    Returns the states int32 (..., n_labels, n_steps); with return_logp also float64 (..., n_labels).  check as for viterbi."""
    pt = _prob_tensor(prob, True)
    S, T = int(pt.shape[-2]), int(pt.shape[-1])
    trans = _host64(transition, "transition")
    if trans.shape == (2, 2):
        _check_transition(trans, (2, 2))
    elif trans.shape == (S, 2, 2):
        for t in trans:
            _check_transition(t, (2, 2))
    else:
        raise ValueError(f"transition.shape={trans.shape}, must be (2, 2) or (n_states, 2, 2)=({S}, 2, 2)")
    dists = []
    for p, pname in ((p_state, "p_state"), (p_init, "p_init")):
        if p is None:
            p = np.full(S, 0.5)
        else:
            p = _host64(p, pname)
            p = np.full(S, float(p)) if p.ndim == 0 else p
            _check_dist(p, S, pname, False)
        dists.append(np.ascontiguousarray(np.stack([_log32(1.0 - p), _log32(p)], axis=-1)))
    _check_caps(S, T, False)
    dev, B, E, flags, (lt, li) = _emissions(pt, 2, dists[0], (_log32(trans), dists[1]))
    bits = torch.empty((B, (T + 15) // 16, S), dtype=torch.int32, device=dev)
    states = torch.empty((B, S, T), dtype=torch.int32, device=dev)
    logp = torch.empty((B, S), dtype=torch.float64, device=dev)
    _x.check(_x.dlib(dev).ap_viterbi_binary_f32(_x.ptr(E), B, S, T, _x.ptr(lt), int(trans.ndim == 3), _x.ptr(li), _x.ptr(bits),
                                                _x.ptr(states), _x.ptr(logp), _x.stream_ptr(dev)))
    if check:
        _raise_flags(flags, "viterbi_binary", 2)
    lead = tuple(pt.shape[:-2])
    states = states.reshape(lead + (S, T))
    return (states, logp.reshape(lead + (S,))) if return_logp else states


__all__ = ["viterbi", "viterbi_discriminative", "viterbi_binary", "transition_uniform", "transition_loop", "transition_cycle",
           "transition_local"]
