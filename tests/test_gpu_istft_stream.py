"""GPU: StreamingISTFT (ap_istft_stream_f32).  Concatenated outputs are bit-identical over chunkings (0- and
1-frame chunks, one chunk holding everything), equal to the offline istft, read line-padded views in place, and
invert StreamingSTFT."""

import numpy as np
import pytest
import torch

from oracle import audio_oracle as ao

import mlx_audio_primitives_amd as ap

pytestmark = pytest.mark.gpu

SHAPES = [(2048, 512), (1024, 256), (512, 128), (400, 160), (256, 64), (300, 75)]   # 300: two-launch path
K = 40
CHUNKINGS = [[K], [1] * K, [0, 5, 1, 17, 0, 2, 15], [16, 16, 0, 8]]


def spectrum(B, n_fft, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    F = n_fft // 2 + 1
    return torch.complex(torch.randn((B, F, T), device="cuda", generator=g),
                         torch.randn((B, F, T), device="cuda", generator=g))


def stream(S, n_fft, hop, chunks, center, dense=False):
    st = ap.StreamingISTFT(n_fft=n_fft, hop_length=hop, center=center)
    outs, t = [], 0
    for c in chunks:
        chunk = S[..., t:t + c]                     # a strided view: rows K frames apart
        outs.append(st.process(chunk.contiguous() if dense else chunk))
        t += c
    outs.append(st.flush())
    assert st.frames_consumed == S.shape[-1]
    assert st.samples_emitted == sum(o.shape[-1] for o in outs)
    return torch.cat(outs, dim=-1)


def tiny_envelope_mask(n_fft, hop, T, center, n_out):
    """False where the window's sum of squares is tiny (first / last samples of a hann stream): there the
    division amplifies float32 rounding of the transforms and no two implementations agree to 1e-5."""
    w2 = ao.padded_window("hann", n_fft, n_fft).astype(np.float64) ** 2
    wss = np.zeros((T - 1) * hop + n_fft)
    for t in range(T):
        wss[t * hop:t * hop + n_fft] += w2
    off = n_fft // 2 if center else 0
    return wss[off:off + n_out] > 1e-2


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("n_fft,hop", SHAPES)
def test_chunk_invariant_and_matches_offline(n_fft, hop, center):
    S = spectrum(3, n_fft, K, n_fft + hop)
    ys = [stream(S, n_fft, hop, ch, center) for ch in CHUNKINGS]
    for ch, y in zip(CHUNKINGS[1:], ys[1:]):
        assert torch.equal(y, ys[0]), ch
    off = ap.istft(S, hop_length=hop, n_fft=n_fft, center=center)
    want = ao.istft(S.cpu().numpy(), hop_length=hop, n_fft=n_fft, center=center)
    assert ys[0].shape == off.shape == want.shape
    ok = tiny_envelope_mask(n_fft, hop, K, center, want.shape[1])
    got = ys[0].cpu().numpy()
    np.testing.assert_allclose(got[:, ok], off.cpu().numpy()[:, ok], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[:, ok], want[:, ok], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("n_fft,hop", SHAPES)
def test_dense_and_line_padded_views_are_bit_identical(n_fft, hop):
    S = spectrum(3, n_fft, K, 7)
    chunks = [3, 0, 21, 16]
    assert torch.equal(stream(S, n_fft, hop, chunks, False), stream(S, n_fft, hop, chunks, False, dense=True))
    # the line-padded view ap.stft returns (rows padded to whole 128-byte lines), read in place
    y = torch.randn((3, hop * 199), device="cuda")
    Sl = ap.stft(y, n_fft=n_fft, hop_length=hop)
    a = stream(Sl, n_fft, hop, [200], True)
    b = stream(Sl.contiguous(), n_fft, hop, [200], True)
    assert torch.equal(a, b)


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (2048, 512), (400, 160)])
def test_round_trip_with_streaming_stft(n_fft, hop):
    L = 3 * 16000 + 37
    y = torch.randn((3, L), device="cuda") * 0.3
    fwd = ap.StreamingSTFT(n_fft=n_fft, hop_length=hop, center=True)
    inv = ap.StreamingISTFT(n_fft=n_fft, hop_length=hop, center=True)
    outs, pos = [], 0
    for c in [1000, 0, 1, 4999, 777, 12000, 300]:
        outs.append(inv.process(fwd.process(y[:, pos:pos + c])))
        pos += c
    outs.append(inv.process(fwd.process(y[:, pos:])))
    outs.append(inv.process(fwd.flush()))
    outs.append(inv.flush())
    yr = torch.cat(outs, dim=1)
    n = hop * (L // hop)
    assert yr.shape == (3, n)
    np.testing.assert_allclose(yr.cpu().numpy(), y[:, :n].cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_many_streams_eight_frame_chunks():
    n_fft, hop, T = 512, 128, 48
    S = spectrum(1024, n_fft, T, 3)
    y = stream(S, n_fft, hop, [8] * (T // 8), False)
    off = ap.istft(S, hop_length=hop, n_fft=n_fft, center=False)
    ok = tiny_envelope_mask(n_fft, hop, T, False, off.shape[1])
    np.testing.assert_allclose(y.cpu().numpy()[:, ok], off.cpu().numpy()[:, ok], rtol=1e-5, atol=1e-5)


def test_host_input_and_one_d_output():
    S = spectrum(1, 512, 10, 11)[0]
    st = ap.StreamingISTFT(n_fft=512, hop_length=128)
    a = st.process(S[:, :4].cpu().numpy())
    assert a.ndim == 1 and a.shape == (4 * 128,) and a.is_cuda
    b = st.process(S[:, 4:])
    c = st.flush()
    assert c.shape == (512 - 128,)
    y = torch.cat([a, b, c])
    assert torch.equal(y, stream(S[None], 512, 128, [10], False)[0])
    assert st.samples_emitted == 9 * 128 + 512


def test_errors():
    with pytest.raises(ValueError, match="hop_length"):
        ap.StreamingISTFT(n_fft=512, hop_length=600)
    with pytest.raises(ValueError, match="hop_length"):
        ap.StreamingISTFT(n_fft=512, hop_length=0)
    with pytest.raises(ValueError, match="center=True"):
        ap.StreamingISTFT(n_fft=512, hop_length=300, center=True)
    ap.StreamingISTFT(n_fft=512, hop_length=300, center=False)            # allowed without centring
    st = ap.StreamingISTFT(n_fft=512, hop_length=128)
    with pytest.raises(ValueError, match="before any frame"):
        st.flush()
    with pytest.raises(ValueError, match="frequency bins"):
        st.process(spectrum(2, 1024, 4, 0))
    st.process(spectrum(2, 512, 4, 0))
    with pytest.raises(ValueError, match="same batch"):
        st.process(spectrum(3, 512, 4, 0))
    with pytest.raises(ValueError, match="same batch"):
        st.process(spectrum(1, 512, 4, 0)[0])
    st.flush()
    with pytest.raises(ValueError, match="reset"):
        st.process(spectrum(2, 512, 4, 0))
    st.reset()
    assert st.frames_consumed == 0 and st.samples_emitted == 0
    assert st.process(spectrum(1, 512, 4, 0)[0]).shape == (4 * 128,)
