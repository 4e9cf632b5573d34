"""GPU: the sequence decoders on the device against the definition in tests/viterbi_ref.py and against the emulator.

The sweeps of test_emu_viterbi.py go through the C entries on the device.  The device's own emission buffer is
downloaded and fed to the float32 model and to the emulator: back-pointers, states and logp must equal both in every bit
(only the emission kernel takes a logarithm, and it is held to the bound derived in viterbi_ref.py instead).  Then the
public functions: 2-D, batched and host input, a non-default stream, padded rows read in place, the flags, the float64
definition on the seeded shapes, and the properties a user of a decoder relies on."""

import os
import sys

import numpy as np
import pytest
import torch

import viterbi_ref as R
import test_emu_viterbi as E

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x
from mlx_audio_primitives_amd.onset import _rows

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_viterbi_bind as eb  # noqa: E402

pytestmark = pytest.mark.gpu
TAIL = 64           # poisoned elements behind every device output


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def out(n, dtype, fill):
    return torch.full((n + TAIL,), fill, dtype=dtype, device="cuda")


def body(t, shape, fill):
    a = t.cpu().numpy()
    n = int(np.prod(shape))
    tail = a[n:]
    assert (np.isnan(tail) if np.isnan(fill) else tail == fill).all(), "an element behind an output was written"
    return a[:n].reshape(shape).copy()


def device_emission(prob, mode, lps=None, pad=0):
    """(E, flags) through ap_viterbi_emission_f32; NaN columns behind the rows of prob."""
    B, S, T = prob.shape
    buf = torch.full((B, S, T + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :, :T] = dev(prob)
    shape = (B, T, S, 2) if mode == 2 else (B, T, S)
    Ed = out(int(np.prod(shape)), torch.float32, float("nan"))
    fd = out(B, torch.int32, -7)
    ld = None if lps is None else dev(np.asarray(lps, np.float32))
    _x.check(_x.dlib(buf.device).ap_viterbi_emission_f32(_x.ptr(buf), B, S, T, T + pad, mode, None if ld is None else _x.ptr(ld),
                                                         _x.ptr(Ed), _x.ptr(fd), _x.stream_ptr(buf.device)))
    return body(Ed, shape, np.nan), body(fd, (B,), -7)


def device_decode(Eh, lt, li):
    B, T, S = Eh.shape
    Ed, ltd, lid = dev(Eh), dev(lt), dev(li)
    ptr = out(B * T * S, torch.int16, -4370)                    # 0xEEEE
    st = out(B * T, torch.int32, -7)
    lp = out(B, torch.float64, float("nan"))
    _x.check(_x.dlib(Ed.device).ap_viterbi_decode_f32(_x.ptr(Ed), B, S, T, _x.ptr(ltd), _x.ptr(lid), _x.ptr(ptr), _x.ptr(st), _x.ptr(lp),
                                                      _x.stream_ptr(Ed.device)))
    return body(ptr, (B, T, S), -4370).view(np.uint16), body(st, (B, T), -7), body(lp, (B,), np.nan)


def device_binary(Eh, lt, li):
    B, T, S, _ = Eh.shape
    Ed, ltd, lid = dev(Eh), dev(lt), dev(li)
    nw = (T + 15) // 16
    bits = out(B * nw * S, torch.int32, -7)
    st = out(B * S * T, torch.int32, -7)
    lp = out(B * S, torch.float64, float("nan"))
    _x.check(_x.dlib(Ed.device).ap_viterbi_binary_f32(_x.ptr(Ed), B, S, T, _x.ptr(ltd), int(np.ndim(lt) == 3), _x.ptr(lid), _x.ptr(bits),
                                                      _x.ptr(st), _x.ptr(lp), _x.stream_ptr(Ed.device)))
    return body(bits, (B, nw, S), -7).view(np.uint32), body(st, (B, S, T), -7), body(lp, (B, S), np.nan)


def same(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("case", E.DENSE_CASES, ids=E.DENSE_IDS)
def test_gpu_dense_sweep(case):
    S, T, B, _ = case
    prob, trans, p_init = R.random_problem(S, T, E.DENSE_CASES.index(case), B=B)
    Ed, flags = device_emission(prob, 0, pad=case[2] - 1)
    assert not flags.any()
    for b in range(B):
        assert (np.abs(Ed[b].astype(np.float64) - R.emissions64(prob[b], 0)) <= R.emission_bound(prob[b], 0)).all()
    lt, li = R.log32(trans), R.log32(p_init)
    got = device_decode(Ed, lt, li)
    E.assert_dense(got, Ed, lt, li, case)
    assert same(got, eb.decode(Ed, lt, li)), "the device and the emulator differ"


@pytest.mark.parametrize("S", (3, 40, 64, 300))
def test_gpu_ties_go_to_the_smallest_index(S):
    rng = np.random.default_rng(S)
    T = E.CHUNK + 3
    Eh = rng.integers(-2, 1, size=(2, T, S)).astype(np.float32)
    Eh[1] = 0.0
    lt = rng.integers(-2, 1, size=(S, S)).astype(np.float32)
    li = np.zeros(S, np.float32)
    got = device_decode(Eh, lt, li)
    E.assert_dense(got, Eh, lt, li, "ties")
    flat = device_decode(np.zeros((1, T, S), np.float32), np.zeros((S, S), np.float32), li)     # everything ties
    assert not flat[0].any() and not flat[1].any() and flat[2][0] == 0.0


def test_gpu_deterministic_cycle():
    n, T = 70, 2 * E.CHUNK + 3
    p_init = np.zeros(n)
    p_init[n - 2] = 1.0
    states = ap.viterbi(np.full((n, T), 0.5, np.float32), R.transition_cycle(n, 0.0), p_init=p_init)
    assert np.array_equal(states.cpu().numpy(), (n - 2 + np.arange(T)) % n)


@pytest.mark.parametrize("case", E.BINARY_CASES, ids=E.BINARY_IDS)
def test_gpu_binary_sweep(case):
    L, T, B, per = case
    rng = np.random.default_rng(1000 + E.BINARY_CASES.index(case))
    prob = rng.uniform(size=(B, L, T)).astype(np.float32)
    p_state, p_init = rng.uniform(0.2, 0.8, size=L), rng.uniform(0.2, 0.8, size=L)
    trans = rng.uniform(size=(L, 2, 2) if per else (2, 2))
    trans /= trans.sum(axis=-1, keepdims=True)
    Ed, flags = device_emission(prob, 2, R.log_state(p_state, True), pad=B - 1)
    assert not flags.any()
    for b in range(B):
        assert (np.abs(Ed[b].astype(np.float64) - R.emissions64(prob[b], 2, p_state)) <= R.emission_bound(prob[b], 2, p_state)).all()
    lt, li = R.log32(trans), R.log_state(p_init, True)
    got = device_binary(Ed, lt, li)
    for b in range(B):
        rb, rs, rl = R.decode_binary_f32(Ed[b], lt, li)
        assert np.array_equal(got[0][b], rb) and np.array_equal(got[1][b], rs) and got[2][b].tobytes() == rl.tobytes(), (case, b)
    assert same(got, eb.binary(Ed, lt, li)), "the device and the emulator differ"


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_gpu_emission_bound_and_flags(mode):
    S, T, B = E.ETILE + 3, 2 * E.ETILE + 1, 6
    prob, _, _ = R.random_problem(S, T, 9, B=B, normalise=mode == 1)
    p_state = np.random.default_rng(1).uniform(0.05, 0.95, size=S)
    lps = None if mode == 0 else R.log_state(p_state, mode == 2)
    if mode != 1:
        prob[0].reshape(-1)[::7] = 0.0
        prob[0].reshape(-1)[3::11] = 1.0
    Ed, flags = device_emission(prob, mode, lps, pad=1)
    assert not flags.any()
    err = np.abs(Ed[0].astype(np.float64) - R.emissions64(prob[0], mode, p_state))
    assert (err <= R.emission_bound(prob[0], mode, p_state)).all(), err.max()
    prob[1, S - 1, T - 1] = 1.5
    prob[2, 0, 0] = -1e-3
    prob[3, 5, E.ETILE] = np.nan
    prob[4, :, T - 1] *= np.float32(1.001)
    prob[5, :, 3] *= np.float32(1.000001)
    _, flags = device_emission(prob, mode, lps, pad=1)
    assert flags.tolist() == [R.emission_flags(prob[b], mode) for b in range(B)] == ([0, 3, 3, 3, 2, 0] if mode == 1 else [0, 1, 1, 1, 0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------------------------------
def expected(prob, trans, p_init, mode=0, p_state=None):
    """The float32 model on the device's own emissions of prob (S, T)."""
    lps = None if mode == 0 else R.log_state(p_state)
    Ed, _ = device_emission(prob[None], mode, lps)
    _, states, logp = R.decode_f32(Ed[0], R.log32(trans), R.log32(p_init))
    return states, logp


def test_gpu_public_input_kinds():
    S, T = 12, 75
    prob, trans, p_init = R.random_problem(S, T, 3, B=6)
    want = [expected(prob[b], trans, p_init) for b in range(6)]
    ws, wl = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    s, lp = ap.viterbi(dev(prob[0]), trans, p_init=p_init, return_logp=True)                  # 2-D, on the device
    assert s.dtype == torch.int32 and lp.dtype == torch.float64 and s.shape == (T,) and lp.shape == () and s.is_cuda
    assert np.array_equal(s.cpu().numpy(), ws[0]) and lp.item() == wl[0]
    s, lp = ap.viterbi(prob.reshape(2, 3, S, T), trans, p_init=p_init, return_logp=True)      # batched, from the host
    assert s.shape == (2, 3, T) and lp.shape == (2, 3) and s.is_cuda
    assert np.array_equal(s.cpu().numpy().reshape(6, T), ws) and np.array_equal(lp.cpu().numpy().reshape(6), wl)
    s = ap.viterbi(prob.astype(np.float64)[1], torch.from_numpy(trans).cuda(), p_init=list(p_init))   # float64, a device transition
    assert np.array_equal(s.cpu().numpy(), ws[1])
    side = torch.cuda.Stream()                                                               # a non-default stream
    with torch.cuda.stream(side):
        s = ap.viterbi(dev(prob), trans, p_init=p_init)
    side.synchronize()
    assert np.array_equal(s.cpu().numpy(), ws)
    buf = torch.full((6, S, T + 5), float("nan"), dtype=torch.float32, device="cuda")        # padded rows, read in place
    buf[:, :, :T] = dev(prob)
    view = buf[:, :, :T]
    assert _rows(view)[0].data_ptr() == view.data_ptr() and _rows(view)[1] == T + 5
    s = ap.viterbi(view, trans, p_init=p_init)
    assert np.array_equal(s.cpu().numpy(), ws)
    assert torch.isnan(buf[:, :, T:]).all()


def test_gpu_check_flag_and_no_synchronisation():
    S, T = 5, 40
    prob, trans, _ = R.random_problem(S, T, 4, B=3, normalise=True)
    bad = prob.copy()
    bad[1, 2, 7] = 1.25
    with pytest.raises(ValueError, match="sequence 1"):
        ap.viterbi(bad, trans)
    with pytest.raises(ValueError, match="sequence 1"):
        ap.viterbi_binary(bad, [[0.9, 0.1], [0.2, 0.8]])
    off = prob.copy()
    off[2, :, 5] *= np.float32(0.9)
    with pytest.raises(ValueError, match="sequence 2.*sum to 1"):
        ap.viterbi_discriminative(off, trans)
    ap.viterbi(off, trans)                                       # the plain decoder has no rule about the sums
    # check=False: no exception for the same input, and nothing that synchronises (the host parameters are on the device
    # after the first call)
    xd = dev(bad)
    calls = ((ap.viterbi, trans), (ap.viterbi_discriminative, trans), (ap.viterbi_binary, np.array([[0.9, 0.1], [0.2, 0.8]])))
    for fn, tr in calls:
        fn(xd, tr, check=False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [fn(xd, tr, check=False, return_logp=True) for fn, tr in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(s.is_cuda and lp.is_cuda for s, lp in outs)


@pytest.mark.parametrize("shape", R.SEEDED_SHAPES, ids=["S%d-T%d" % s for s in R.SEEDED_SHAPES])
def test_gpu_against_the_float64_definition(shape):
    S, T = shape
    prob, trans, p_init = R.random_problem(S, T, 0)
    E64, lt64, li64 = R.emissions64(prob, 0), np.log(trans + R.TINY), np.log(p_init + R.TINY)
    _, best = R.decode_f64(E64, lt64, li64)
    states, logp = ap.viterbi(prob, trans, p_init=p_init, return_logp=True)
    states, logp = states.cpu().numpy(), logp.item()
    bound = R.path_bound(T, R.emission_bound(prob, 0).max(), E64, lt64)
    gap = best - R.path_score(E64, lt64, li64, states)
    print(f"S={S} T={T}: optimum {best:.6f}, returned path {best - gap:.6f}, gap {gap:.3e}, bound {bound:.3e}, logp {logp:.6f}")
    assert 0.0 <= gap + 1e-9 and gap <= bound
    assert abs(logp - best) <= bound
    want, wl = expected(prob, trans, p_init)
    assert np.array_equal(states, want) and logp == wl


def test_gpu_discriminative_and_binary_public():
    S, T = 9, 130
    prob, trans, p_init = R.random_problem(S, T, 8, normalise=True)
    p_state = np.random.default_rng(2).dirichlet(np.ones(S))
    s, lp = ap.viterbi_discriminative(prob, trans, p_state=p_state, p_init=p_init, return_logp=True)
    want, wl = expected(prob, trans, p_init, 1, p_state)
    assert np.array_equal(s.cpu().numpy(), want) and lp.item() == wl
    # one label of viterbi_binary = viterbi_discriminative on the stacked [1 - p, p] problem
    p = np.random.default_rng(3).uniform(size=(1, T)).astype(np.float32)
    t2 = np.array([[0.9, 0.1], [0.3, 0.7]])
    sb, lb = ap.viterbi_binary(p, t2, p_state=0.3, p_init=0.4, return_logp=True)
    stacked = np.stack([np.float32(1) - p[0], p[0]])
    sd, ld = ap.viterbi_discriminative(stacked, t2, p_state=[0.7, 0.3], p_init=[0.6, 0.4], return_logp=True, check=False)
    assert sb.shape == (1, T) and lb.shape == (1,)
    assert np.array_equal(sb.cpu().numpy()[0], sd.cpu().numpy()) and lb.cpu().numpy()[0] == ld.item()
    s1 = ap.viterbi_binary(p[0], t2)                             # librosa's 1-D form
    assert s1.shape == (1, T)


def test_gpu_properties():
    S, T = 11, 90
    prob, trans, p_init = R.random_problem(S, T, 12)
    p_init = np.random.default_rng(4).dirichlet(np.ones(S))
    base = ap.viterbi(prob, trans, p_init=p_init).cpu().numpy()
    perm = np.random.default_rng(5).permutation(S)               # new state k is old state perm[k]
    got = ap.viterbi(prob[perm], trans[np.ix_(perm, perm)], p_init=p_init[perm]).cpu().numpy()
    assert np.array_equal(perm[got], base)
    flat = ap.viterbi(prob, ap.transition_uniform(S)).cpu().numpy()
    assert np.array_equal(flat, prob.argmax(axis=0))
