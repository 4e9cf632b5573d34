"""CPU: the streaming ISTFT kernel source (kernels_istft_stream.h) on the SIMT emulator of tests/emu.

Two frames per workgroup (the GPU uses 16) so that every workgroup needs a halo from its neighbour's frames,
calls shorter than the halo pass part of the carry through, and 0-frame calls pass all of it.  Concatenated
outputs must be bit-identical over the chunkings and match the oracle's offline istft."""

import os
import sys

import numpy as np
import pytest

from oracle import audio_oracle as ao

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_istft_stream_bind as eb  # noqa: E402


def spectrum(B, n_fft, K, seed):
    rng = np.random.default_rng(seed)
    F = n_fft // 2 + 1
    return (rng.standard_normal((B, F, K)) + 1j * rng.standard_normal((B, F, K))).astype(np.complex64)


def envelope(n_fft, hop, K, window):
    wss = np.zeros((K - 1) * hop + n_fft)
    for t in range(K):
        wss[t * hop:t * hop + n_fft] += window.astype(np.float64) ** 2
    return wss


def run(S, n_fft, hop, chunks, center, G=2, row_pad=0):
    win = ao.padded_window("hann", n_fft, n_fft)
    st = eb.Stream(n_fft, hop, win, center=center, G=G)
    outs, t = [], 0
    for c in chunks:
        outs.append(st.process(S[:, :, t:t + c], row_stride=c + row_pad if row_pad else None))
        t += c
    assert t == S.shape[2]
    outs.append(st.flush())
    return np.concatenate(outs, axis=1)


CASES = [  # n_fft, hop, chunkings of K frames (0- and 1-frame chunks, one chunk holding everything)
    (2048, 512, [[9], [1] * 9, [0, 2, 0, 1, 1, 4, 1], [3, 0, 6]]),
    (512, 128, [[11], [1] * 11, [0, 1, 2, 0, 5, 3], [4, 7]]),
    (1024, 256, [[6], [1, 0, 5], [2, 4]]),
    (400, 160, [[7], [1, 0, 2, 4], [2, 2, 2, 1]]),
    (256, 64, [[8], [1] * 8, [0, 3, 5]]),
    (300, 75, [[7], [1] * 7, [0, 3, 0, 4]]),          # the two-launch path (irfft frames + carried overlap-add)
]


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("n_fft,hop,chunkings", CASES)
def test_emu_istft_stream_chunk_invariant_and_matches_oracle(n_fft, hop, chunkings, center):
    K = sum(chunkings[0])
    S = spectrum(2, n_fft, K, n_fft + hop)
    ys = [run(S, n_fft, hop, ch, center) for ch in chunkings]
    for ch, y in zip(chunkings[1:], ys[1:]):
        assert np.array_equal(y, ys[0]), (ch, np.max(np.abs(y - ys[0])))
    want = ao.istft(S, hop_length=hop, n_fft=n_fft, center=center)
    assert ys[0].shape == want.shape
    # where the window's sum of squares is tiny (the first / last samples of a hann-windowed stream) the
    # division amplifies the float32 transform's rounding: compare where it is not
    off = n_fft // 2 if center else 0
    wss = envelope(n_fft, hop, K, ao.padded_window("hann", n_fft, n_fft))
    ok = wss[off:off + want.shape[1]] > 1e-2
    np.testing.assert_allclose(ys[0][:, ok], want[:, ok], rtol=1e-5, atol=1e-5)
    assert eb.lib().emu_istft_stream_lds_overruns() == 0


def test_emu_istft_stream_padded_rows_and_tile_sizes():
    """Rows further apart than the chunk (line-padded views) and other tile sizes give the same bits."""
    n_fft, hop, K = 512, 128, 10
    S = spectrum(3, n_fft, K, 5)
    base = run(S, n_fft, hop, [3, 1, 6], False)
    assert np.array_equal(run(S, n_fft, hop, [3, 1, 6], False, row_pad=13), base)
    assert np.array_equal(run(S, n_fft, hop, [3, 1, 6], False, G=16), base)
    assert np.array_equal(run(S, n_fft, hop, [10], False, G=3), base)


def test_emu_istft_stream_argument_checks():
    win = ao.padded_window("hann", 512, 512)
    st = eb.Stream(512, 128, win)
    with pytest.raises(ValueError, match="final call needs at least one frame"):
        st.flush()
    st = eb.Stream(512, 600, win)
    with pytest.raises(ValueError, match="hop_length"):
        st.process(spectrum(1, 512, 2, 0))
