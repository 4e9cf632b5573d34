"""CPU: the public surface of sequence.py: exports, librosa's signatures, the build and ABI lists, every rejected argument
(named, and rejected before a device is asked for), and the transition builders against hand-computed cases."""

import inspect

import numpy as np
import pytest
import torch

import viterbi_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _build, _extension as _x
from mlx_audio_primitives_amd import sequence as MOD

NAMES = ("viterbi", "viterbi_discriminative", "viterbi_binary", "transition_uniform", "transition_loop", "transition_cycle",
         "transition_local")


@pytest.fixture
def no_device(monkeypatch):
    """Any request for a device fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device was asked for before the arguments were validated")
    monkeypatch.setattr(_x, "require_device", boom)
    monkeypatch.setattr(_x, "dlib", boom)


def test_exports_signatures_and_defaults():
    for n in NAMES:
        assert n in ap.__all__ and n in MOD.__all__ and getattr(ap, n) is getattr(MOD, n)
    want = {
        "viterbi": (["prob", "transition"], {"p_init": None, "return_logp": False, "check": True}),
        "viterbi_discriminative": (["prob", "transition"], {"p_state": None, "p_init": None, "return_logp": False, "check": True}),
        "viterbi_binary": (["prob", "transition"], {"p_state": None, "p_init": None, "return_logp": False, "check": True}),
        "transition_uniform": (["n_states"], {}),
        "transition_loop": (["n_states", "prob"], {}),
        "transition_cycle": (["n_states", "prob"], {}),
        "transition_local": (["n_states", "width"], {"window": "triangle", "wrap": False}),
    }
    for n, (pos, kw) in want.items():
        ps = inspect.signature(getattr(ap, n)).parameters
        assert [k for k, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD] == pos, n
        assert {k: p.default for k, p in ps.items() if p.kind == p.KEYWORD_ONLY} == kw, n
        assert list(ps) == pos + list(kw), n                     # `check` comes last
    for n in NAMES[:3]:
        doc = getattr(ap, n).__doc__
        assert "copied to the host" in doc and "check" in doc
    for word in ("float32", "int32", "ValueError", "ap_viterbi_max_states"):
        assert word in MOD.__doc__


def test_build_and_abi_lists():
    assert "viterbi.hip" in _build.SOURCES
    lib = _x.lib()
    for sym in ("ap_viterbi_max_states", "ap_viterbi_max_steps", "ap_viterbi_emission_f32", "ap_viterbi_decode_f32", "ap_viterbi_binary_f32"):
        assert sym in _x.ABI_SYMBOLS and getattr(lib, sym) is not None
    assert lib.ap_viterbi_max_states() >= 1024 and lib.ap_viterbi_max_steps() >= 1 << 16


def test_rejections_come_before_the_device(no_device):
    S, T = 4, 6
    prob = np.full((S, T), 0.25, np.float32)
    tr = ap.transition_uniform(S)
    cap_s, cap_t = _x.lib().ap_viterbi_max_states(), _x.lib().ap_viterbi_max_steps()
    bad = [
        (ap.viterbi, (np.zeros(T), tr), {}, "prob must be"),
        (ap.viterbi, (np.zeros((S, 0)), tr), {}, "empty"),
        (ap.viterbi, (prob.astype(np.complex64), tr), {}, "real"),
        (ap.viterbi, (prob, np.ones((S, S + 1))), {}, "transition.shape"),
        (ap.viterbi, (prob, ap.transition_uniform(S + 1)), {}, "transition.shape"),
        (ap.viterbi, (prob, -tr), {}, "Invalid transition"),
        (ap.viterbi, (prob, 2 * tr), {}, "Invalid transition"),
        (ap.viterbi, (prob, "abc"), {}, "transition must be"),
        (ap.viterbi, (prob, tr), {"p_init": np.ones(S)}, "Invalid p_init"),
        (ap.viterbi, (prob, tr), {"p_init": np.full(S + 1, 1 / (S + 1))}, "Invalid p_init"),
        (ap.viterbi, (prob, tr), {"p_init": [1.5, -0.5, 0, 0]}, "Invalid p_init"),
        (ap.viterbi, (np.zeros((cap_s + 1, 2), np.float32), ap.transition_uniform(cap_s + 1)), {}, f"cap of {cap_s}"),
        (ap.viterbi, (torch.zeros((2, 1)).expand(2, cap_t + 1), ap.transition_uniform(2)), {}, f"cap of {cap_t}"),
        (ap.viterbi_discriminative, (prob, tr), {"p_state": np.ones(S)}, "Invalid p_state"),
        (ap.viterbi_discriminative, (prob, tr), {"p_state": np.full(S - 1, 1 / (S - 1))}, "Invalid p_state"),
        (ap.viterbi_discriminative, (prob, tr), {"p_init": np.zeros(S)}, "Invalid p_init"),
        (ap.viterbi_discriminative, (prob, tr[:2]), {}, "transition.shape"),
        (ap.viterbi_binary, (prob, tr), {}, r"must be \(2, 2\)"),
        (ap.viterbi_binary, (prob, np.ones((S + 1, 2, 2)) / 2), {}, r"must be \(2, 2\)"),
        (ap.viterbi_binary, (prob, np.array([[0.5, 0.6], [0.5, 0.5]])), {}, "Invalid transition"),
        (ap.viterbi_binary, (prob, np.stack([np.eye(2)] * (S - 1) + [np.ones((2, 2))])), {}, "Invalid transition"),
        (ap.viterbi_binary, (prob, np.eye(2)), {"p_state": 1.5}, "Invalid p_state"),
        (ap.viterbi_binary, (prob, np.eye(2)), {"p_state": np.full(S + 1, 0.5)}, "Invalid p_state"),
        (ap.viterbi_binary, (prob, np.eye(2)), {"p_init": [-0.1, 0.5, 0.5, 0.5]}, "Invalid p_init"),
        (ap.viterbi_binary, (np.zeros((2, cap_t + 1), np.float32), np.eye(2)), {}, f"cap of {cap_t}"),
    ]
    for fn, args, kw, match in bad:
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)
    # a label count above the dense cap is fine for the binary decoder: it reaches the device request
    with pytest.raises(AssertionError, match="a device was asked for"):
        ap.viterbi_binary(np.zeros((cap_s + 1, 2), np.float32), np.eye(2))


def test_builders_reject_what_librosa_rejects():
    for fn, args, kw in [
        (ap.transition_uniform, (0,), {}), (ap.transition_uniform, (2.5,), {}), (ap.transition_uniform, (True,), {}),
        (ap.transition_loop, (1, 0.5), {}), (ap.transition_loop, (3, 1.5), {}), (ap.transition_loop, (3, [0.5, 0.5]), {}),
        (ap.transition_cycle, (1, 0.5), {}), (ap.transition_cycle, (3, -0.1), {}), (ap.transition_cycle, (3, [0.1] * 4), {}),
        (ap.transition_local, (1, 1), {}), (ap.transition_local, (5, 0), {}), (ap.transition_local, (5, 6), {}),
        (ap.transition_local, (5, 2.5), {}), (ap.transition_local, (5, [1, 2, 3]), {}),
    ]:
        with pytest.raises(ValueError):
            fn(*args, **kw)
    with pytest.raises(TypeError):
        ap.transition_local(5, 3, window=None)


def test_builders_match_hand_computed_cases():
    np.testing.assert_array_equal(ap.transition_uniform(4), np.full((4, 4), 0.25))
    np.testing.assert_allclose(ap.transition_loop(3, 0.8), [[0.8, 0.1, 0.1], [0.1, 0.8, 0.1], [0.1, 0.1, 0.8]], rtol=1e-15)
    np.testing.assert_allclose(ap.transition_loop(3, [0.5, 1.0, 0.0]), [[0.5, 0.25, 0.25], [0, 1, 0], [0.5, 0.5, 0]], rtol=1e-15)
    np.testing.assert_allclose(ap.transition_cycle(3, [0.5, 0.25, 0.1]), [[0.5, 0.5, 0], [0, 0.25, 0.75], [0.9, 0, 0.1]], rtol=1e-15)
    np.testing.assert_array_equal(ap.transition_cycle(4, 0.0), np.roll(np.eye(4), 1, axis=1))
    # triangle of 3 points = (0.5, 1, 0.5), cut at the ends of the state space and normalised
    third = 1.0 / 3.0
    np.testing.assert_allclose(ap.transition_local(5, 3), [[2 * third, third, 0, 0, 0], [0.25, 0.5, 0.25, 0, 0], [0, 0.25, 0.5, 0.25, 0],
                                                           [0, 0, 0.25, 0.5, 0.25], [0, 0, 0, third, 2 * third]], rtol=1e-15)
    np.testing.assert_allclose(ap.transition_local(5, 3, wrap=True)[0], [0.5, 0.25, 0, 0, 0.25], rtol=1e-15)
    # an even width leans to the right: [0, 1, 1, 0] rolled by n // 2 + i + 1 = 4 for i = 1 (librosa's construction)
    np.testing.assert_allclose(ap.transition_local(4, [1, 2, 1, 1], window="boxcar"), [[1, 0, 0, 0], [0, 0.5, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    for t in (ap.transition_loop(7, 0.3), ap.transition_cycle(7, np.linspace(0, 1, 7)), ap.transition_local(9, 5),
              ap.transition_local(9, [1, 2, 3, 4, 5, 6, 7, 8, 9], wrap=True), ap.transition_local(6, 4, window="hann", wrap=True)):
        assert t.dtype == np.float64 and (t >= 0).all()
        np.testing.assert_allclose(t.sum(axis=1), 1.0, rtol=1e-14)
    # against the reference's own statement of the builders
    for n, w, wrap in ((9, 5, False), (8, [1, 2, 3, 4, 5, 6, 7, 8], True), (6, 4, False)):
        np.testing.assert_allclose(ap.transition_local(n, w, wrap=wrap), R.transition_local(n, w, wrap=wrap), rtol=1e-15)
    np.testing.assert_allclose(ap.transition_loop(5, 0.2), R.transition_loop(5, 0.2), rtol=1e-15)
    np.testing.assert_allclose(ap.transition_cycle(5, 0.2), R.transition_cycle(5, 0.2), rtol=1e-15)
    from scipy.signal import get_window
    np.testing.assert_allclose(R.triangle(6), get_window("triangle", 6, fftbins=False), rtol=1e-15)
    np.testing.assert_allclose(R.triangle(7), get_window("triangle", 7, fftbins=False), rtol=1e-15)


def test_host_parameters_are_logged_in_float64_and_cached_by_content():
    tr = ap.transition_loop(3, 0.9)
    np.testing.assert_array_equal(MOD._log32(tr), R.log32(tr))
    assert MOD._log32(np.zeros(1))[0] == np.float32(np.log(np.finfo(np.float32).tiny))
    a = MOD._on_device_cached((MOD._log32(tr), None), "cpu")
    b = MOD._on_device_cached((MOD._log32(tr.copy()), None), "cpu")
    c = MOD._on_device_cached((MOD._log32(ap.transition_loop(3, 0.8)), None), "cpu")
    assert a[0] is b[0] and a[1] is None and c[0] is not a[0]
