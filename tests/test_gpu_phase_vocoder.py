"""GPU: phase_vocoder against librosa's float64 angle recurrence (tests/pv_ref.py).  Per row, max |out - ref64| <=
4 x (the float32 sequential twin's max error over the case, relative to max |D|) x (the row's max |D|); the zero row is
exactly zero.  Every input carries two zero columns, a zero row, a row times 1e-30 and a row times 1e+25.  The worst
error / (twin error x row max) per case is printed with -s and recorded in profiles/pv_timings.txt."""

import numpy as np
import pytest
import torch

import pv_ref as R

import mlx_audio_primitives_amd as ap
from mlx_audio_primitives_amd import _extension as _x

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def padded(a, pad):                                                    # a view of NaN-padded rows
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + pad,), complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
    view = buf[..., :a.shape[-1]]
    view.copy_(dev(a))
    return view


def check(got, case):
    D, want, twin = R.reference(*case[:4])
    assert got.shape[-1] == R.frames(case[2], case[3]) and got.dtype == torch.complex64
    ratio = R.worst_ratio(got.cpu().numpy(), D, want, twin)
    print(f"phase_vocoder {R.case_id(case)}: twin {twin:.2e}, worst error / twin {ratio:.2f}")
    assert ratio <= R.MARGIN


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gpu_phase_vocoder(case):
    B, F, T, rate, W = case
    assert _x.lib().ap_phase_vocoder_waves(B * F, R.frames(T, rate)) == W
    D = R.reference(B, F, T, rate)[0]
    got = ap.phase_vocoder(dev(D), rate=rate)
    check(got, case)
    assert torch.equal(ap.phase_vocoder(D[0].copy(), rate=rate, hop_length=8, n_fft=64), got[0])      # 2D, a host array


def test_gpu_phase_vocoder_padded_view_and_batches():
    """A B = 2 strided, row-padded view; the same bits on a second run, and for a clip alone or in a batch of two (66
    and 33 rows take the same waves per row), with one wave per row and with sixteen."""
    for case in ((2, 33, 200, 1.3, 1), (2, 33, 3000, 0.9, 16)):
        B, F, T, rate, W = case
        n = R.frames(T, rate)
        assert _x.lib().ap_phase_vocoder_waves(B * F, n) == _x.lib().ap_phase_vocoder_waves(F, n) == W
        D = R.reference(B, F, T, rate)[0]
        view = padded(D, 5)
        assert not view.is_contiguous()
        got = ap.phase_vocoder(view, rate=rate)
        check(got, case)
        assert torch.equal(ap.phase_vocoder(view, rate=rate), got)
        assert torch.equal(ap.phase_vocoder(dev(D), rate=rate), got)
        for b in range(B):
            assert torch.equal(ap.phase_vocoder(dev(D[b:b + 1]), rate=rate), got[b:b + 1])


def test_gpu_phase_vocoder_output_feeds_istft():
    """F = 1025: the result is a view of rows padded to 16 frames, which istft reads as it is."""
    case = (1, 1025, 40, 0.8, 1)
    D = R.reference(*case[:4])[0]
    got = ap.phase_vocoder(dev(D), rate=0.8)
    assert got.shape == (1, 1025, 50) and got.stride(1) == 64 and not got.is_contiguous()
    check(got, case)
    y = ap.istft(got).cpu().numpy().astype(np.float64)
    want = ap.istft(got.contiguous()).cpu().numpy().astype(np.float64)
    assert y.shape == (1, 49 * 512) and np.all(np.isfinite(y))
    assert np.max(np.abs(y - want)) <= 1e-5 * np.max(np.abs(want))
    out = ap.phase_vocoder(dev(D[:, :, :0]), rate=0.5)                 # no frames, no clips: no launch
    assert out.shape == (1, 1025, 0) and out.dtype == torch.complex64 and out.is_cuda
    assert ap.phase_vocoder(dev(D[:0]), rate=0.5).shape == (0, 1025, 80)
