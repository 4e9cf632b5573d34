"""Steady-state time of yin on the headline batch (256 clips x 220 500 samples @22.05 kHz, frame_length 2048,
hop 512), next to pitch_detect_acf on the same input and the headline melspectrogram of the same run.

Protocol of tools/bench_configs.py (`steady`): inputs resident in HBM, three rotating input buffers, ramp-up with
the operator itself, median of 5 back-to-back streams timed with HIP events.  One JSON line.

  python tools/yin_bench.py                 # everything
  python tools/yin_bench.py --only yin      # one operator (for a kernel trace of it alone)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mlx_audio_primitives_amd as ap  # noqa: E402
from tools.bench_configs import N_ROT, steady  # noqa: E402

OPS = ("yin", "yin_cmnd", "yin_general", "yin1024", "pitch_detect_acf", "mel")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--samples", type=int, default=220500)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=OPS, action="append")
    a = p.parse_args()
    which = set(a.only or OPS)
    g = torch.Generator(device="cuda").manual_seed(42)
    ys = [torch.randn((a.batch, a.samples), device="cuda", generator=g) * 0.1 for _ in range(N_ROT)]
    T = 1 + a.samples // 512
    kw = dict(fmin=65.0, fmax=2093.0, sr=22050, frame_length=2048, hop_length=512)
    rep = {"batch": a.batch, "samples": a.samples, "frames": a.batch * T}

    def put(name, ms):
        rep[name + "_ms"] = round(ms, 4)
        rep[name + "_Mframes_per_s"] = round(rep["frames"] / ms / 1e3, 2)

    if "yin" in which:
        put("yin", steady(lambda i: ap.yin(ys[i % N_ROT], **kw), ramp_s=a.ramp))
    if "yin_cmnd" in which:
        put("yin_cmnd", steady(lambda i: ap.yin_cmnd(ys[i % N_ROT], **kw), ramp_s=a.ramp))
    if "yin_general" in which:
        os.environ["AP_YIN_GENERAL"] = "1"
        put("yin_general", steady(lambda i: ap.yin(ys[i % N_ROT], **kw), ramp_s=a.ramp))
        del os.environ["AP_YIN_GENERAL"]
    if "yin1024" in which:                                # twice the frames of the other rows
        ms = steady(lambda i: ap.yin(ys[i % N_ROT], fmin=100.0, fmax=2000.0, sr=22050, frame_length=1024,
                                     hop_length=256), ramp_s=a.ramp)
        rep["yin1024_ms"] = round(ms, 4)
    if "pitch_detect_acf" in which:
        put("pitch_detect_acf", steady(lambda i: ap.pitch_detect_acf(ys[i % N_ROT], sr=22050, fmin=65.0, fmax=2093.0,
                                                                     frame_length=2048, hop_length=512), ramp_s=a.ramp))
    if "mel" in which:
        put("mel", steady(lambda i: ap.melspectrogram(ys[i % N_ROT], sr=22050, n_fft=2048, hop_length=512, n_mels=128),
                          ramp_s=a.ramp))
    if "yin_ms" in rep and "mel_ms" in rep:
        rep["yin_over_mel"] = round(rep["yin_ms"] / rep["mel_ms"], 2)
    if "yin_ms" in rep and "pitch_detect_acf_ms" in rep:
        rep["pitch_detect_acf_over_yin"] = round(rep["pitch_detect_acf_ms"] / rep["yin_ms"], 2)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
