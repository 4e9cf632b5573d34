"""CPU: the sequence-decoding kernels (csrc/kernels_viterbi.h) on the SIMT emulator, through the C entries' twins,
against the definition in tests/viterbi_ref.py.  Back-pointers, states and logp must equal the float32 model in every
bit; the emission kernel lies within the bound derived there and raises its flags for exactly the offending sequences.
Every buffer lies between poisoned bands and prob has NaN pad columns behind its rows (tests/emu/emu_viterbi_bind.py)."""

import os
import sys

import numpy as np
import pytest

import viterbi_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_viterbi_bind as eb  # noqa: E402

CONSTS = eb.constants()
BLOCK, CAP, CHUNK, LT_LDS = CONSTS["block"], CONSTS["max_states"], CONSTS["chunk"], CONSTS["lt_lds_max"]
WORD, LABELS, ETILE = CONSTS["word"], CONSTS["labels"], CONSTS["emission_tile"]
DENSE_S = (1, 2, 3, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, CAP)
DENSE_T = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, 2 * CHUNK + 3)

# (S, T, B, lt in LDS?)
DENSE_CASES = (
    (1, 1, 1, True), (1, CHUNK + 1, 3, False), (2, 2, 1, True), (2, 2 * CHUNK + 3, 3, False), (3, CHUNK, 1, True),
    (3, CHUNK + 2, 1, False), (5, CHUNK - 1, 3, True), (17, 2 * CHUNK + 3, 1, True), (63, CHUNK + 1, 1, False), (64, CHUNK, 3, True),
    (64, CHUNK + 2, 1, False), (65, 2 * CHUNK + 3, 1, True), (100, CHUNK - 1, 1, False), (LT_LDS, CHUNK + 2, 3, True),
    (LT_LDS + 1, CHUNK + 2, 1, True), (BLOCK - 1, CHUNK + 1, 1, True),
    (BLOCK, 2, 3, True), (BLOCK, CHUNK + 2, 1, True), (BLOCK + 1, CHUNK, 1, True), (2 * BLOCK + 44, 3, 1, True), (CAP, 1, 1, True),
    (CAP, 3, 1, True),
)
DENSE_IDS = ["S%d-T%d-B%d-lds%d" % c for c in DENSE_CASES]
BINARY_LABELS = (1, LABELS - 1, LABELS, LABELS + 1, 2 * LABELS + 2)
# (labels, T, B, per-label transitions?)
BINARY_CASES = (
    (1, 1, 1, False), (1, WORD + 1, 3, True), (LABELS - 1, 2, 1, True), (LABELS - 1, LABELS, 1, False), (LABELS, WORD, 3, False),
    (LABELS, LABELS + 1, 1, True), (LABELS + 1, LABELS - 1, 1, False), (LABELS + 1, WORD - 1, 1, True),
    (2 * LABELS + 2, 2 * LABELS + 3, 1, True), (2 * LABELS + 2, WORD + 1, 3, False),
)
BINARY_IDS = ["L%d-T%d-B%d-per%d" % c for c in BINARY_CASES]
# (S, T, B, pad)
EMISSION_CASES = ((1, 1, 1, 0), (3, ETILE - 1, 3, 2), (ETILE - 1, ETILE, 1, 0), (ETILE, ETILE + 1, 1, 1), (ETILE + 1, 2 * ETILE + 2, 1, 0),
                  (2 * ETILE + 2, 5, 3, 3))


def dense_inputs(S, T, B, seed):
    """Float32 emissions, log transitions and log initial distribution of a random problem."""
    prob, trans, p_init = R.random_problem(S, T, seed, B=B)
    E = np.stack([R.emissions32(prob[b], 0) for b in range(B)])
    return E, R.log32(trans), R.log32(p_init)


def assert_dense(got, E, lt, li, what=""):
    ptr, states, logp = got
    for b in range(E.shape[0]):
        rp, rs, rl = R.decode_f32(E[b], lt, li)
        bad = np.argwhere(ptr[b] != rp)
        assert bad.size == 0, f"{what} sequence {b}: {len(bad)} back-pointers differ, first at {tuple(bad[0])}"
        assert np.array_equal(states[b], rs), f"{what} sequence {b}: the states differ from the model's"
        assert logp[b].tobytes() == np.float64(rl).tobytes(), f"{what} sequence {b}: logp {logp[b]!r} != {rl!r}"


def test_the_sweeps_cover_what_they_claim():
    col = lambda i, cases: {c[i] for c in cases}                 # noqa: E731
    assert col(0, DENSE_CASES) >= set(DENSE_S) and col(1, DENSE_CASES) >= set(DENSE_T) and col(2, DENSE_CASES) == {1, 3}
    assert any(c[3] and c[0] <= LT_LDS for c in DENSE_CASES) and any(not c[3] and c[0] <= LT_LDS for c in DENSE_CASES)
    assert any(BLOCK < c[0] < CAP and c[0] % BLOCK for c in DENSE_CASES), "several passes, the last one partial"
    assert {LT_LDS, LT_LDS + 1} <= col(0, DENSE_CASES) and LT_LDS < BLOCK, "both sides of the lt-in-LDS threshold"
    assert col(0, BINARY_CASES) == set(BINARY_LABELS) and col(2, BINARY_CASES) == {1, 3} and col(3, BINARY_CASES) == {False, True}
    assert col(1, BINARY_CASES) >= {1, 2, WORD - 1, WORD, WORD + 1, LABELS - 1, LABELS, LABELS + 1, 2 * LABELS + 3}
    assert CAP >= 1024 and CHUNK >= 2 and WORD == 16


@pytest.mark.parametrize("case", DENSE_CASES, ids=DENSE_IDS)
def test_dense_decode_equals_the_model_in_every_bit(case):
    S, T, B, lds = case
    E, lt, li = dense_inputs(S, T, B, DENSE_CASES.index(case))
    got = eb.decode(E, lt, li, lt_lds_max=None if lds else 0)
    geo = eb.geometry()
    assert geo["lt_lds"] == int(lds and S <= LT_LDS) and geo["lanes_per_state"] == min(max(BLOCK // S, 1), S, CONSTS["max_g"])
    assert geo["lds_bytes"] <= (160 if geo["lt_lds"] else 48) * 1024
    assert_dense(got, E, lt, li)


def test_dense_decode_does_not_depend_on_the_grid():
    E, lt, li = dense_inputs(7, CHUNK + 3, 5, 77)
    a = eb.decode(E, lt, li)
    b = eb.decode(E, lt, li, grid=2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert_dense(b, E, lt, li)


@pytest.mark.parametrize("S", (2, 3, 5, 40, 64, 100, 300))
def test_ties_go_to_the_smallest_index(S):
    """Integer-valued logs: whole rows of exact ties, in the (value, index) reduction, across the lanes that share a
    state, and in the last state's argmax."""
    rng = np.random.default_rng(S)
    T = CHUNK + 3
    E = rng.integers(-2, 1, size=(2, T, S)).astype(np.float32)
    lt = rng.integers(-2, 1, size=(S, S)).astype(np.float32)
    li = np.zeros(S, np.float32)
    E[1] = 0.0                                                   # everything ties: the path is all zeros
    got = eb.decode(E, lt, li, lt_lds_max=0 if S == 40 else None)
    assert_dense(got, E, lt, li, "ties")
    flat = eb.decode(np.zeros((1, T, S), np.float32), np.zeros((S, S), np.float32), li)
    assert not flat[0].any() and not flat[1].any() and flat[2][0] == 0.0
    assert S == 2 or ((lt == lt.max(axis=0)).sum(axis=0) > 1).any(), "a column of lt holds its maximum more than once"


@pytest.mark.parametrize("n", (3, 64, 70, 300))
def test_a_deterministic_cycle_is_followed(n):
    """transition_cycle(n, 0): state i is always left for i + 1.  With flat emissions and all the initial mass on state k
    the path is (k + t) mod n."""
    T, k = 2 * CHUNK + 3, n - 2
    lt = R.log32(R.transition_cycle(n, 0.0))
    p_init = np.zeros(n)
    p_init[k] = 1.0
    E = np.stack([R.emissions32(np.full((n, T), 0.5, np.float32), 0)])
    ptr, states, logp = eb.decode(E, lt, R.log32(p_init))
    assert np.array_equal(states[0], (k + np.arange(T)) % n)
    assert_dense((ptr, states, logp), E, lt, R.log32(p_init))
    np.testing.assert_allclose(logp[0], T * np.log(0.5), rtol=1e-6)


@pytest.mark.parametrize("case", BINARY_CASES, ids=BINARY_IDS)
def test_binary_decode_equals_the_model_in_every_bit(case):
    L, T, B, per = case
    rng = np.random.default_rng(1000 + BINARY_CASES.index(case))
    prob = rng.uniform(size=(B, L, T)).astype(np.float32)
    p_state, p_init = rng.uniform(0.2, 0.8, size=L), rng.uniform(0.2, 0.8, size=L)
    trans = rng.uniform(size=(L, 2, 2) if per else (2, 2))
    trans /= trans.sum(axis=-1, keepdims=True)
    E = np.stack([R.emissions32(prob[b], 2, p_state) for b in range(B)])
    lt, li = R.log32(trans), R.log_state(p_init, True)
    bits, states, logp = eb.binary(E, lt, li)
    for b in range(B):
        rb, rs, rl = R.decode_binary_f32(E[b], lt, li)
        assert np.array_equal(bits[b], rb), f"sequence {b}: the pointer bits differ"
        assert np.array_equal(states[b], rs), f"sequence {b}: the states differ"
        assert logp[b].tobytes() == rl.tobytes(), f"sequence {b}: logp differs"
    assert states.min() >= 0 and states.max() <= 1


def test_binary_ties_and_the_stacked_dense_problem():
    """Integer logs (ties go to state 0), and one label against the dense decode of the same two-state chain."""
    rng = np.random.default_rng(5)
    T, L = 2 * LABELS + 5, 3
    E = rng.integers(-1, 1, size=(1, T, L, 2)).astype(np.float32)
    lt = rng.integers(-1, 1, size=(2, 2)).astype(np.float32)
    li = np.zeros((L, 2), np.float32)
    bits, states, logp = eb.binary(E, lt, li)
    rb, rs, rl = R.decode_binary_f32(E[0], lt, li)
    assert np.array_equal(bits[0], rb) and np.array_equal(states[0], rs) and logp[0].tobytes() == rl.tobytes()
    for lab in range(L):
        _, ds, dl = eb.decode(E[:, :, lab, :], lt, li[lab])
        assert np.array_equal(ds[0], states[0, lab]) and dl[0] == logp[0, lab]


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("case", EMISSION_CASES, ids=["S%d-T%d-B%d-pad%d" % c for c in EMISSION_CASES])
def test_emission_kernel_within_the_derived_bound(case, mode):
    S, T, B, pad = case
    prob, _, _ = R.random_problem(S, T, 31 * S + T + mode, B=B, normalise=mode == 1)
    if mode != 1:
        prob.reshape(-1)[::7] = 0.0                              # the guard: log(tiny)
        prob.reshape(-1)[3::11] = 1.0
    p_state = None if mode == 0 else np.random.default_rng(S).uniform(0.05, 0.95, size=S)
    lps = None if mode == 0 else R.log_state(p_state, mode == 2)
    E, flags = eb.emission(prob, mode, lps, pad=pad)
    assert not flags.any()
    for b in range(B):
        err = np.abs(E[b].astype(np.float64) - R.emissions64(prob[b], mode, p_state))
        bound = R.emission_bound(prob[b], mode, p_state)
        assert (err <= bound).all(), f"sequence {b}: error {err.max():.3e} at {np.unravel_index((err - bound).argmax(), err.shape)}"


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_emission_flags_name_exactly_the_offending_sequences(mode):
    S, T, B = ETILE + 3, 2 * ETILE + 1, 6
    prob, _, _ = R.random_problem(S, T, 9, B=B, normalise=mode == 1)
    prob[1, S - 1, T - 1] = 1.5                                  # the last element of a sequence
    prob[2, 0, 0] = -1e-3
    prob[3, 5, ETILE] = np.nan
    prob[4, :, T - 1] *= np.float32(1.001)                       # a column sum off by 1e-3 (no value above 1)
    prob[5, :, 3] *= np.float32(1.000001)                        # off by 1e-6: inside the tolerance
    lps = None if mode == 0 else R.log_state(np.full(S, 1.0 / S), mode == 2)
    _, flags = eb.emission(prob, mode, lps, pad=1, grid=3)
    want = [R.emission_flags(prob[b], mode) for b in range(B)]
    assert want == ([0, 3, 3, 3, 2, 0] if mode == 1 else [0, 1, 1, 1, 0, 0])   # (a value out of range moves its column's sum too)
    assert flags.tolist() == want


def test_status_codes_without_a_launch():
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data
    INVALID, UNSUPPORTED = -1, -2
    assert eb.emission_raw(None, 1, 2, 2, 2, 0, None, p, p) == INVALID and "NULL" in eb.last_error()
    assert eb.emission_raw(p, 0, 2, 2, 2, 0, None, p, p) == INVALID
    assert eb.emission_raw(p, 1, 2, 3, 2, 0, None, p, p) == INVALID and "row_stride" in eb.last_error()
    assert eb.emission_raw(p, 1, 2, 2, 2, 3, p, p, p) == INVALID and "mode" in eb.last_error()
    assert eb.emission_raw(p, 1, 2, 2, 2, 1, None, p, p) == INVALID and "prior" in eb.last_error()
    assert eb.emission_raw(p, 1, 2, CONSTS["max_steps"] + 1, CONSTS["max_steps"] + 1, 0, None, p, p) == UNSUPPORTED
    assert eb.decode_raw(p, 1, 2, 2, p, p, p, p, None) == INVALID and "NULL" in eb.last_error()
    assert eb.decode_raw(p, 1, 0, 2, p, p, p, p, p) == INVALID
    assert eb.decode_raw(p, 1, CAP + 1, 2, p, p, p, p, p) == UNSUPPORTED and str(CAP) in eb.last_error()
    assert eb.decode_raw(p, 1, 2, CONSTS["max_steps"] + 1, p, p, p, p, p) == UNSUPPORTED and str(CONSTS["max_steps"]) in eb.last_error()
    assert eb.binary_raw(p, 1, 2, 2, None, p, p, p, p) == INVALID and "NULL" in eb.last_error()
    assert eb.binary_raw(p, 1, 2, 0, p, p, p, p, p) == INVALID
    assert eb.binary_raw(p, 1, 2, CONSTS["max_steps"] + 1, p, p, p, p, p) == UNSUPPORTED
    assert not buf.any(), "a rejected call wrote something"


@pytest.mark.parametrize("shape", R.SEEDED_SHAPES, ids=["S%d-T%d" % s for s in R.SEEDED_SHAPES])
def test_the_model_reaches_the_float64_path_on_the_seeded_shapes(shape):
    """The float32 model with per-step renormalisation against the plain float64 recursion: the same path, logp to 1e-6,
    and the path's float64 score within the derived bound of the optimum."""
    S, T = shape
    prob, trans, p_init = R.random_problem(S, T, 0)
    E64 = R.emissions64(prob, 0)
    lt64, li64 = np.log(trans + R.TINY), np.log(p_init + R.TINY)
    want, best = R.decode_f64(E64, lt64, li64)
    E32 = R.emissions32(prob, 0)
    _, states, logp = R.decode_f32(E32, R.log32(trans), R.log32(p_init))
    assert np.array_equal(states, want)
    np.testing.assert_allclose(logp, best, rtol=1e-6)
    err = np.abs(E32.astype(np.float64) - E64).max()
    assert err <= R.emission_bound(prob, 0).max()
    assert best - R.path_score(E64, lt64, li64, states) <= R.path_bound(T, err, E64, lt64)
