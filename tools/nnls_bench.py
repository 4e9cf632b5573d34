"""Time mel_to_stft (one launch of the fused NNLS kernel) beside one griffinlim call at the same shape.

    python tools/nnls_bench.py [--batch 64] [--frames 216] [--n-iter 100] [--reps 9]

Device events around `inner` back-to-back calls after a warm-up; prints the median, the range over the repetitions and
frames per second.  Needs a GPU."""

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_audio_primitives_amd as ap  # noqa: E402


def timed(fn, reps, inner):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms)), min(ms), max(ms)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--frames", type=int, default=216)
    p.add_argument("--n-iter", type=int, default=100)
    p.add_argument("--reps", type=int, default=9)
    a = p.parse_args()
    y = torch.from_numpy(np.random.default_rng(0).standard_normal((a.batch, (a.frames - 1) * 512)).astype(np.float32)).cuda()
    mel = ap.melspectrogram(y, n_fft=2048, hop_length=512).contiguous()
    assert mel.shape == (a.batch, 128, a.frames), mel.shape
    for n_iter in sorted({0, a.n_iter}):
        med, lo, hi = timed(lambda: ap.mel_to_stft(mel, n_iter=n_iter), a.reps, 20)
        print(f"mel_to_stft B={a.batch} M=128 T={a.frames} n_fft=2048 n_iter={n_iter}: {med:.3f} ms (range {lo:.3f} - {hi:.3f}), "
              f"{a.batch * a.frames / med * 1e3:.3e} frames/s")
    S = ap.mel_to_stft(mel, n_iter=a.n_iter)
    med, lo, hi = timed(lambda: ap.griffinlim(S, n_iter=32, hop_length=512, random_state=0), a.reps, 3)
    print(f"griffinlim (32 iterations) on the result: {med:.3f} ms (range {lo:.3f} - {hi:.3f})")


if __name__ == "__main__":
    main()
