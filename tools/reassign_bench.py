"""Time reassigned_spectrogram (one fused launch) beside the composition it replaces: three `stft` calls with the windows
h, dh, th and the pointwise torch chain on their results.

    python tools/reassign_bench.py [--seconds 10] [--reps 9]

Device events around `inner` back-to-back calls after a warm-up, the two versions alternating; prints the median and the
range over the repetitions.  Needs a GPU."""

import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_audio_primitives_amd as ap  # noqa: E402
from mlx_audio_primitives_amd import _extension as _x  # noqa: E402
from mlx_audio_primitives_amd.reassign import _get_reassign_tables  # noqa: E402
from mlx_audio_primitives_amd.stft import _get_twiddles  # noqa: E402

SR = 22050


def stft_with(y, n_fft, hop, win):
    """`stft` with a window table already on the device, rows padded to whole 128-byte lines as `stft` lays them out
    (the public call would hash an array window on the host at every call: not the baseline's fault)."""
    B, L = y.shape
    T, F = 1 + L // hop, n_fft // 2 + 1
    Ts = -(-T // 16) * 16
    out = torch.empty((B, F, Ts, 2), dtype=torch.float32, device=y.device)
    _x.check(_x.dlib(y.device).ap_stft_rows_f32(_x.ptr(y), B, L, n_fft, hop, _x.ptr(win), _x.ptr(_get_twiddles(n_fft, y.device)), 1, 0,
                                                T, Ts, _x.ptr(out), _x.stream_ptr(y.device)))
    return torch.view_as_complex(out)[:, :, :T]


def composed(y, n_fft, hop, ref_power=1e-6):
    h, dh, th = _get_reassign_tables("hann", n_fft, n_fft, y.device)
    Sh, Sdh, Sth = (stft_with(y, n_fft, hop, w) for w in (h, dh, th))
    mags = Sh.abs()
    F, T = Sh.shape[-2:]
    bin_f = torch.arange(F, device=y.device, dtype=torch.float32)[:, None] * (SR / n_fft)
    frame_t = torch.arange(T, device=y.device, dtype=torch.float32)[None, :] * (hop / SR)
    nan = torch.full((), float("nan"), device=y.device)
    bad = mags < math.sqrt(ref_power)
    freqs = torch.where(bad, nan, bin_f - (Sdh / Sh).imag * (SR / (2 * math.pi))).clamp(0, SR / 2)
    times = torch.where(bad, nan, frame_t + (Sth / Sh).real / SR).clamp(0, y.shape[-1] / SR)
    return freqs, times, mags


def timed_pair(fns, reps, inner):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):                      # alternating: both versions see the same machine state
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / inner)
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--reps", type=int, default=9)
    a = p.parse_args()
    L = int(a.seconds * SR)
    for n_fft, hop in ((2048, 512), (400, 160)):
        for B in (64, 256):
            y = torch.from_numpy(np.random.default_rng(0).standard_normal((B, L)).astype(np.float32)).cuda()
            fused = lambda: ap.reassigned_spectrogram(y, sr=SR, n_fft=n_fft, hop_length=hop)  # noqa: E731
            comp = lambda: composed(y, n_fft, hop)  # noqa: E731
            f, c = fused(), comp()
            ok = ~torch.isnan(f[0]) & ~torch.isnan(c[0]) & (f[2] > 1.0)
            worst = float((f[0] - c[0])[ok].abs().max())
            (fm, flo, fhi), (cm, clo, chi) = timed_pair([fused, comp], a.reps, 10)
            T = f[2].shape[-1]
            print(f"n_fft={n_fft} hop={hop} B={B} T={T}: fused {fm:.3f} ms (range {flo:.3f} - {fhi:.3f}), {12 * B * (n_fft // 2 + 1) * T / fm * 1e-6:.0f} GB/s "
                  f"of output; composed {cm:.3f} ms (range {clo:.3f} - {chi:.3f}); max |freqs difference| where |S_h| > 1: {worst:.3g} Hz",
                  flush=True)
            del f, c


if __name__ == "__main__":
    main()
