"""GPU: pcen / StreamingPCEN through the public API against the float64 definition in tests/pcen_ref.py: the cases and
bounds of test_emu_pcen.py, and what only the device shows (a padded-row view straight from melspectrogram, 2D input,
streams).  Worst error / bound seen on an MI355X: 0.27 for the values, 0.15 for zf (printed per case with -s)."""

import numpy as np
import pytest
import torch

import pcen_ref as R

import mlx_audio_primitives_amd as ap

pytestmark = pytest.mark.gpu

IDS = ["x".join(map(str, s)) for s in R.SHAPES]


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()          # (the shared cases are read-only)


def host(t):
    return t.cpu().numpy()


def padded(a, pad):
    """The array as a view of NaN-padded rows."""
    B, M, T = a.shape
    buf = torch.full((B, M, T + pad), float("nan"), device="cuda")
    view = buf[:, :, :T]
    view.copy_(dev(a))
    return view


def run(S, name, Sd=None, **kw):
    p = R.params(name)
    zi = kw.pop("zi", R.zi_for(S.shape) if p["b"] == 0.0 else None)
    out, zf = ap.pcen(dev(S) if Sd is None else Sd, zi=zi, return_zf=True, **p, **kw)
    assert out.shape == S.shape and zf.shape == S.shape[:2] + (1,) and out.dtype == zf.dtype == torch.float32
    return host(out), host(zf), p, zi


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_gpu_pcen(shape):
    S = R.cases()["wide"][shape]
    views = (dev(S), padded(S, 5))
    worst = worst_zf = 0.0
    for k, name in enumerate(R.PARAMS if shape in R.SMALL else ("defaults", "b=1e-3")):
        got, zf, p, zi = run(S, name, views[k % 2])
        r, rz, _ = R.check(got, zf, S, p, (shape, name), zi=zi)
        worst, worst_zf = max(worst, r), max(worst_zf, rz)
        if k < 2:
            assert np.array_equal(got, run(S, name, views[1 - k % 2])[0])            # dense and padded rows: the same bits
    print(f"pcen {shape}: worst error / bound {worst:.3f}, zf {worst_zf:.3f}")


@pytest.mark.parametrize("kind", ["quiet", "zeros"])
def test_gpu_pcen_quiet_input(kind):
    S = R.cases()[kind][R.QUIET_SHAPE]
    worst = 0.0
    for name in ("defaults", "b=1e-3", "power=2", "bias=0", "power=0", "speech"):
        got, zf, p, zi = run(S, name)
        worst = max(worst, R.check(got, zf, S, p, (kind, name))[0])
        assert np.all((got == 0.0) == (S == 0.0))
    print(f"pcen {kind} input: worst error / bound {worst:.3f}")


def test_gpu_pcen_max_size_ref_and_zi():
    worst = 0.0
    for shape in R.SMALL:
        S = R.cases()["wide"][shape]
        for k, ms in enumerate(R.max_sizes(shape[1])):
            for name in ("defaults", "b=1"):
                got, zf, p, _ = run(S, name, (None, padded(S, 3))[k % 2], max_size=ms, max_axis=(None, -2, 1)[k % 3])
                worst = max(worst, R.check(got, zf, S, dict(p, max_size=ms), (shape, ms, name))[0])
    for shape in ((3, 5, 64), (3, 3, 129)):
        S, ref, zi = R.cases()["wide"][shape], R.cases()["zeros"][shape], R.zi_for(shape)
        for refd in (dev(ref), padded(ref, 4), ref):
            got, zf, p, _ = run(S, "defaults", ref=refd, max_size=3, zi=dev(zi))
            worst = max(worst, R.check(got, zf, S, p, (shape, "ref"), zi=zi, ref=ref)[0])
        got, zf, p, _ = run(S, "b=1e-3", zi=zi[0])                                # (M, 1): the same state for every clip
        worst = max(worst, R.check(got, zf, S, p, (shape, "zi"), zi=zi[0])[0])
        with pytest.raises(ValueError, match="ref must have the shape of S"):
            ap.pcen(dev(S), ref=torch.zeros((shape[0], shape[1] + 1, shape[2]), device="cuda"))
    print(f"pcen max_size / ref / zi: worst error / bound {worst:.3f}")


def test_gpu_pcen_2d_input_is_row_0_of_the_batch():
    S = R.cases()["wide"][(3, 5, 64)]
    zi = R.zi_for(S.shape)
    for kw in (dict(), dict(max_size=3), dict(power=0.0, b=0.5)):
        out, zf = ap.pcen(dev(S), return_zf=True, zi=zi, **kw)
        for b in range(3):
            o2, z2 = ap.pcen(dev(S[b]), return_zf=True, zi=zi[b], **kw)
            assert o2.shape == (5, 64) and z2.shape == (5, 1)
            assert torch.equal(o2, out[b]) and torch.equal(z2, zf[b])
        assert torch.equal(ap.pcen(S[0], **kw), ap.pcen(dev(S), **kw)[0])          # a host array; no state: 1 - b
    assert ap.pcen(dev(S[:, :, :0])).shape == (3, 5, 0)
    o, z = ap.pcen(dev(S[:, :, :0]), return_zf=True, zi=zi)
    assert o.shape == (3, 5, 0) and o.is_cuda and np.array_equal(host(z), zi)


def test_gpu_pcen_on_a_mel_view():
    """melspectrogram's padded-row view (T = 259, rows 264 apart) times 2^31, used in place, against the definition on
    the same float32 mel values; the silent half of clip 1 gives exact zeros."""
    rng = np.random.default_rng(42)
    y = (rng.standard_normal((2, 132096)) * np.linspace(1.0, 0.01, 132096)).astype(np.float32)
    y[1, 66048:] = 0.0
    mel = ap.melspectrogram(dev(y))
    assert mel.shape == (2, 128, 259) and not mel.is_contiguous() and mel.stride(1) == 264
    S = torch.empty_strided(mel.shape, mel.stride(), dtype=torch.float32, device="cuda")       # the same padded rows
    torch.mul(mel, 2.0 ** 31, out=S)
    assert S.stride(1) == 264 and not S.is_contiguous()
    Sh = host(S)
    assert (Sh == 0.0).mean() > 0.1
    worst = 0.0
    for kw in (dict(), dict(max_size=3), dict(gain=0.8, bias=10.0, power=0.25, time_constant=0.06, eps=1e-12)):
        out, zf = ap.pcen(S, return_zf=True, **kw)
        p = dict(R.params("defaults"), **{k: v for k, v in kw.items() if k != "time_constant"})
        if "time_constant" in kw:
            p["b"] = float(R.b_of(kw["time_constant"]))
        worst = max(worst, R.check(host(out), host(zf), Sh, p, ("mel", kw))[0])
        assert torch.equal(out, ap.pcen(S.contiguous(), **kw))
    print(f"pcen on a mel view: worst error / bound {worst:.3f}")


def test_gpu_streaming_pcen():
    """Uneven chunks (1, 63, 64, 65 frames, an empty one, the rest) against the float64 definition on all frames, every
    piece within the bound that carries the state's error along; two streams keep their states apart; reset()."""
    S = R.cases()["wide"][(1, 5, 431)]
    other = R.cases()["zeros"][(1, 5, 431)]
    p = R.params("b=1e-3")
    want, zf64, _ = R.pcen(S, max_size=3, **p)
    a = ap.StreamingPCEN(b=1e-3, max_size=3)
    c = ap.StreamingPCEN(b=1e-3, max_size=3)
    pieces, pos, k_in, zi64, worst = [], 0, 1.0, None, 0.0
    for n in (1, 63, 0, 64, 65, 431 - 193):
        chunk = S[..., pos:pos + n]
        got = a.process(dev(chunk))
        c.process(dev(other[..., pos:pos + n]))                    # another stream in between
        assert got.shape == chunk.shape
        if n:
            r, rz, k_in = R.check(host(got), host(a._state), chunk, dict(p, max_size=3), ("stream", pos), zi=zi64, k_in=k_in)
            zi64 = R.pcen(chunk, max_size=3, zi=zi64, **p)[1]
            worst = max(worst, r, rz)
        pieces.append(host(got))
        pos += n
    assert a.frames_consumed == c.frames_consumed == 431
    np.testing.assert_allclose(zi64, zf64, rtol=1e-12)
    whole = np.concatenate(pieces, -1)
    offline = host(ap.pcen(dev(S), b=1e-3, max_size=3))
    assert np.array_equal(whole[..., :1], offline[..., :1])
    assert whole.shape == want.shape
    # the other stream saw its own input only
    c2 = ap.StreamingPCEN(b=1e-3, max_size=3)
    assert torch.equal(c2.process(dev(other[..., :193])), ap.pcen(dev(other[..., :193]), b=1e-3, max_size=3))
    # (1e-4: ten times the bound six pieces add up to; the two inputs' states differ in the first digit)
    np.testing.assert_allclose(host(c._state), R.pcen(other, max_size=3, **p)[1], rtol=1e-4)
    assert not np.allclose(host(c._state), host(a._state), rtol=1e-1)
    a.reset()
    assert a.frames_consumed == 0 and torch.equal(a.process(dev(S[0])), ap.pcen(dev(S[0]), b=1e-3, max_size=3))   # 2D after reset
    print(f"streaming pcen: worst error / bound {worst:.3f}")
