"""CPU: the host side of pcen / StreamingPCEN (mlx-audio-primitives_amd/pcen.py, streaming.py): the signature, the
parameter validation and its exceptions, the b formula, the default state against scipy.signal.lfilter_zi, the shapes
of zi and zf, the axes that are not implemented, the exported names.  Every check happens before a device is asked
for, so nothing here needs one; the no-launch paths (an empty axis) run against a stand-in for the device lookup."""

import inspect

import numpy as np
import pytest
import torch
from scipy.signal import lfilter_zi

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x
from mlx_audio_primitives_amd.pcen import _parameters, _state, smoothing_coefficient

S = np.abs(np.random.default_rng(0).standard_normal((2, 5, 7))).astype(np.float32)


def test_names_are_exported():
    assert "pcen" in ap.__all__ and "StreamingPCEN" in ap.__all__
    assert callable(ap.pcen) and inspect.isclass(ap.StreamingPCEN)
    assert "ap_pcen_f32" in _x.ABI_SYMBOLS and getattr(_x.lib(), "ap_pcen_f32") is not None


def test_signature_is_librosas():
    sig = inspect.signature(ap.pcen)
    names = list(sig.parameters)
    assert names == ["S", "sr", "hop_length", "gain", "bias", "power", "time_constant", "eps", "b", "max_size", "ref", "axis",
                     "max_axis", "zi", "return_zf"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[1:])
    d = {n: sig.parameters[n].default for n in names[1:]}
    assert d == dict(sr=22050, hop_length=512, gain=0.98, bias=2, power=0.5, time_constant=0.400, eps=1e-6, b=None,
                     max_size=1, ref=None, axis=-1, max_axis=None, zi=None, return_zf=False)
    ctor = inspect.signature(ap.StreamingPCEN.__init__).parameters
    assert set(names[1:]) - {"ref", "return_zf"} <= set(ctor)
    for n in ("process", "reset"):
        assert callable(getattr(ap.StreamingPCEN, n))


def test_b_formula():
    """b = (sqrt(1 + 4 t^2) - 1) / (2 t^2), t = time_constant sr / hop_length: the positive root of t^2 b^2 + b - 1."""
    for tc, sr, hop in ((0.400, 22050, 512), (0.06, 16000, 160), (1.0, 44100, 256), (0.01, 8000, 400)):
        t = tc * sr / hop
        b = smoothing_coefficient(tc, sr, hop)
        assert 0.0 < b < 1.0
        assert abs(t * t * b * b + b - 1.0) < 1e-12
        assert _parameters(sr, hop, 0.98, 2, 0.5, tc, 1e-6, None, 1, -1, None, False)[0] == b
    assert abs(smoothing_coefficient(0.400, 22050, 512) - 0.05638943879134889) < 1e-15
    assert _parameters(22050, 512, 0.98, 2, 0.5, 0.4, 1e-6, 0.25, 1, -1, None, False)[0] == 0.25      # b given: taken as is


def test_default_state_is_scipys_steady_state():
    """zi=None starts every row at 1 - b = scipy.signal.lfilter_zi([b], [1, b - 1]) for 0 < b <= 1; at b = 0 SciPy's
    system is singular and the call needs a state."""
    for b in (1e-6, 1e-3, smoothing_coefficient(0.4, 22050, 512), 0.5, 0.999, 1.0):
        np.testing.assert_allclose(lfilter_zi([b], [1.0, b - 1.0]), [1.0 - b], rtol=1e-9, atol=1e-16)
    with pytest.raises((ValueError, np.linalg.LinAlgError)):
        z = lfilter_zi([0.0], [1.0, -1.0])
        if not np.all(np.isfinite(z)):
            raise ValueError("singular")
    with pytest.raises(ValueError, match="b = 0 needs zi"):
        ap.pcen(S, b=0.0)
    ap_b0 = _parameters(22050, 512, 0.98, 2, 0.5, 0.4, 1e-6, 0.0, 1, -1, None, True)               # with a state: allowed
    assert ap_b0[0] == 0.0


@pytest.mark.parametrize("kw, match", [
    (dict(power=-0.5), "power must be"), (dict(gain=-1.0), "gain must be"), (dict(bias=-2), "bias must be"),
    (dict(eps=0.0), "eps must be"), (dict(eps=-1e-6), "eps must be"), (dict(eps=1e-60), "eps must be"), (dict(eps=1e-40), "eps must be"),
    (dict(time_constant=0.0), "time_constant must be"), (dict(time_constant=-0.4), "time_constant must be"),
    (dict(b=-0.1), "b must lie"), (dict(b=1.5), "b must lie"), (dict(b=float("nan")), "b must lie"),
    (dict(max_size=0), "max_size must be"), (dict(max_size=256), "max_size must be"), (dict(max_size=2.0), "max_size must be"),
    (dict(max_size=True), "max_size must be"), (dict(gain=float("nan")), "gain must be"), (dict(power="1"), "power must be"),
    (dict(hop_length=0), "hop_length must be"), (dict(sr=0), "sr must be"),
    (dict(ref=np.ones((2, 5, 6), np.float32)), "ref must have the shape"),
    (dict(ref=np.ones((5, 7), np.float32)), "ref must have the shape"),
    (dict(zi=np.ones((2, 5, 2), np.float32)), "zi must broadcast"), (dict(zi=np.ones((3, 5, 1), np.float32)), "zi must broadcast"),
    (dict(zi=np.ones((2, 5), np.float32)), "zi must broadcast"), (dict(axis=3), "out of range"), (dict(max_axis=-4), "out of range"),
])
def test_invalid_arguments_raise_value_error(kw, match):
    with pytest.raises(ValueError, match=match):
        ap.pcen(S, **kw)
    ctor = {k: v for k, v in kw.items() if k not in ("ref", "zi", "axis", "max_axis")}
    if ctor:
        with pytest.raises(ValueError, match=match):
            ap.StreamingPCEN(**ctor)


def test_input_kinds():
    with pytest.raises(ValueError, match="must be real"):
        ap.pcen(S.astype(np.complex64))
    with pytest.raises(ValueError, match="2D or 3D"):
        ap.pcen(S[0, 0])
    with pytest.raises(ValueError, match="2D or 3D"):
        ap.pcen(S[None])


@pytest.mark.parametrize("kw", [dict(axis=0), dict(axis=1), dict(axis=-2), dict(max_axis=0), dict(max_axis=-1), dict(max_axis=2),
                                dict(max_size=3, max_axis=0)])
def test_other_axes_are_not_implemented(kw):
    with pytest.raises(NotImplementedError):
        ap.pcen(S, **kw)
    with pytest.raises(NotImplementedError):
        ap.StreamingPCEN(**kw).process(S)


def test_the_implemented_axes_pass_validation():
    """axis = -1 / ndim - 1 and max_axis = None / -2 / ndim - 2 get as far as the device lookup (and, where there is a
    device, through the call)."""
    for kw in (dict(), dict(axis=2), dict(max_axis=-2), dict(max_axis=1, max_size=3), dict(zi=np.ones((5, 1))),
               dict(zi=np.ones((2, 1, 1))), dict(zi=2.0), dict(b=0.0, zi=np.ones((2, 5, 1)))):
        try:
            out = ap.pcen(S, **kw)
        except RuntimeError as e:
            assert not torch.cuda.is_available() and "no HIP device" in str(e)
        else:
            assert tuple(out.shape) == S.shape


def test_state_shapes():
    """zi broadcasts to (batch, M, 1) / (M, 1); zf has exactly that shape."""
    assert tuple(_state(np.ones((5, 1)), 1, 5, True).shape) == (5, 1)
    assert torch.broadcast_shapes(tuple(_state(np.float32(3.0), 2, 5, False).shape), (2, 5, 1)) == (2, 5, 1)
    with pytest.raises(ValueError, match="zi must broadcast"):
        _state(np.ones((2, 5, 1)), 1, 5, True)                 # a batch of states for 2D input
    with pytest.raises(ValueError, match="zi must be real"):
        _state(np.ones((5, 1), np.complex64), 1, 5, True)


def test_empty_input_launches_nothing(monkeypatch):
    """An empty batch, band or time axis: an empty result of the right shape and the state passed through, without a
    launch - the library handle is taken away for the duration, so a launch would fail."""
    monkeypatch.setattr(_x, "require_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(_x, "dlib", lambda device: (_ for _ in ()).throw(AssertionError("a launch")))
    for shape in ((2, 5, 0), (0, 5, 7), (2, 0, 7), (5, 0), (0, 7)):
        E = np.zeros(shape, np.float32)
        out = ap.pcen(E)
        assert tuple(out.shape) == shape and out.dtype == torch.float32
        out, zf = ap.pcen(E, return_zf=True, b=0.25)
        assert tuple(out.shape) == shape and tuple(zf.shape) == shape[:-1] + (1,) and zf.dtype == torch.float32
        assert bool((zf == 0.75).all())
    zi = np.arange(10, dtype=np.float32).reshape(2, 5, 1)
    out, zf = ap.pcen(np.zeros((2, 5, 0), np.float32), zi=zi, return_zf=True)
    assert np.array_equal(zf.numpy(), zi)
    stream = ap.StreamingPCEN(b=0.5)
    assert tuple(stream.process(np.zeros((5, 0), np.float32)).shape) == (5, 0)
    assert stream.frames_consumed == 0 and stream._state is None                # T = 0: a no-op
    with pytest.raises(ValueError, match="same leading shape"):
        stream.process(np.zeros((4, 0), np.float32))
    stream.reset()
    assert tuple(stream.process(np.zeros((4, 0), np.float32)).shape) == (4, 0)
