"""Steady-state times of the chroma features on 256 clips x 10 s @22.05 kHz (hop 512, T = 431 frames per clip; the
shapes of tools/cqt_bench.py).

Protocol of tools/bench_configs.py (`steady`): inputs resident in HBM, three rotating input buffers, ramp-up with the
operator itself, 5 back-to-back streams timed with HIP events; reported: the median stream and the spread (min .. max)
of the five.  Both kernels do a few FMAs per byte they read, so the yardstick is memory traffic: the bytes a step has
to move (its input once, its output once) at the rate `preemphasis` reaches on 256 x 220 500 samples in the same
session (one read and one write of the signal).  Each step is also compared with the same arithmetic composed in torch:
  torch_cqt_fold     abs(C), matmul with the (12, 252) matrix, where(< threshold), division by amax
  torch_stft_fold    matmul of the (12, 1025) matrix with the power spectrogram, division by amax
  torch_cens         L1 normalisation, four comparisons, conv1d with the 43 taps, L2 normalisation
  torch_tonnetz      L1 normalisation, matmul with the (6, 12) basis

  python tools/chroma_bench.py                      # every step, each in a child process under its own time limit;
                                                    # writes profiles/chroma_timings.txt (--out to choose another file)
  python tools/chroma_bench.py --only cqt_fold      # one step in this process, one JSON line (for a kernel trace of it)
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pcen_bench import streams  # noqa: E402

# step -> time limit in seconds
STEPS = {"preemphasis": 120, "chroma_cqt_y": 240, "cqt_fold": 120, "torch_cqt_fold": 180, "stft_fold": 120, "torch_stft_fold": 180,
         "cens": 120, "torch_cens": 120, "tonnetz": 120, "torch_tonnetz": 120}
PAIRS = (("torch_cqt_fold", "cqt_fold"), ("torch_stft_fold", "stft_fold"), ("torch_cens", "cens"), ("torch_tonnetz", "tonnetz"))


def run_step(name, a):
    import torch

    import mlx_audio_primitives_amd as ap
    from tools.bench_configs import N_ROT

    M = importlib.import_module("mlx_audio_primitives_amd.chroma")
    g = torch.Generator(device="cuda").manual_seed(42)
    B, L = a.batch, a.samples
    T = 1 + L // 512
    rep = {"step": name, "batch": B, "samples": L, "T": T}

    def rand(*shape):
        return torch.rand(shape, device="cuda", generator=g)

    if name == "preemphasis":
        ys = [rand(B, L) for _ in range(N_ROT)]
        fn = lambda i: ap.preemphasis(ys[i % N_ROT])                                       # noqa: E731
        rep["bytes"] = 8.0 * B * L
    elif name == "chroma_cqt_y":
        ys = [rand(B, L) * 0.2 - 0.1 for _ in range(N_ROT)]
        fn = lambda i: ap.chroma_cqt(y=ys[i % N_ROT])                                      # noqa: E731
        rep["bytes"] = 4.0 * B * L + 4.0 * B * 12 * T
    elif name in ("cqt_fold", "torch_cqt_fold"):
        Cs = [torch.view_as_complex(rand(B, 252, T, 2) - 0.5) for _ in range(N_ROT)]
        rep["bytes"] = 8.0 * B * 252 * T + 4.0 * B * 12 * T
        if name == "cqt_fold":
            fn = lambda i: ap.chroma_cqt(C=Cs[i % N_ROT])                                  # noqa: E731
        else:
            w = torch.from_numpy(np.array(ap.cq_to_chroma(252, bins_per_octave=36))).cuda()

            def fn(i):
                c = torch.matmul(w, Cs[i % N_ROT].abs())
                c = torch.where(c < 0.0, torch.zeros_like(c), c)
                n = c.abs().amax(dim=1, keepdim=True)
                return c / torch.where(n < M._TINY, torch.ones_like(n), n)
    elif name in ("stft_fold", "torch_stft_fold"):
        Ss = [rand(B, 1025, T) for _ in range(N_ROT)]
        rep["bytes"] = 4.0 * B * 1025 * T + 4.0 * B * 12 * T
        if name == "stft_fold":
            fn = lambda i: ap.chroma_stft(S=Ss[i % N_ROT])                                 # noqa: E731
        else:
            w = torch.from_numpy(np.array(ap.chroma_filterbank(sr=22050, n_fft=2048))).cuda()

            def fn(i):
                c = torch.matmul(w, Ss[i % N_ROT])
                n = c.abs().amax(dim=1, keepdim=True)
                return c / torch.where(n < M._TINY, torch.ones_like(n), n)
    elif name in ("cens", "torch_cens"):
        xs = [rand(B, 12, T) for _ in range(N_ROT)]
        taps = M._smoothing_taps(41, "hann")
        rep["bytes"] = 8.0 * B * 12 * T
        if name == "cens":
            fn = lambda i: M._cens(xs[i % N_ROT], taps, 2)                                 # noqa: E731
        else:
            k = torch.from_numpy(np.array(taps[::-1])).cuda()[None, None, :]

            def fn(i):
                x = xs[i % N_ROT]
                p = x.abs().sum(dim=1, keepdim=True)
                v = x / torch.where(p < M._TINY, torch.ones_like(p), p)
                q = 0.25 * ((v > 0.4).float() + (v > 0.2).float() + (v > 0.1).float() + (v > 0.05).float())
                s = torch.nn.functional.conv1d(q.reshape(B * 12, 1, T), k, padding=21).reshape(B, 12, T)
                n = s.pow(2).sum(dim=1, keepdim=True).sqrt()
                return s / torch.where(n < M._TINY, torch.ones_like(n), n)
    else:
        xs = [rand(B, 12, T) for _ in range(N_ROT)]
        rep["bytes"] = 4.0 * B * 12 * T + 4.0 * B * 6 * T
        if name == "tonnetz":
            fn = lambda i: ap.tonnetz(chroma=xs[i % N_ROT])                                # noqa: E731
        else:
            phi = torch.from_numpy(M._phi64(12).astype(np.float32)).cuda()

            def fn(i):
                x = xs[i % N_ROT]
                p = x.abs().sum(dim=1, keepdim=True)
                return torch.matmul(phi, x / torch.where(p < M._TINY, torch.ones_like(p), p))
    ts = streams(fn, a.ramp)
    rep.update(ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1])
    return rep


def report(rows):
    """The text of profiles/chroma_timings.txt for {step: row of run_step}."""
    lines = ["chroma timings (tools/chroma_bench.py): ms per call, steady state, HIP events, three rotating inputs;",
             "median of 5 back-to-back streams, spread = (max - min) / median of the five",
             "GB/s = (input once + output once) / time; stream = share of the rate preemphasis reaches in the same session", ""]
    rate = rows["preemphasis"]["bytes"] / rows["preemphasis"]["ms"] / 1e6 if "preemphasis" in rows else None
    lines.append(f"{'step':<18}{'batch':>6}{'T':>6}{'MB':>9}{'ms':>10}{'min':>10}{'max':>10}{'spread':>8}{'GB/s':>9}{'stream':>8}")
    for name, r in rows.items():
        gbs = r["bytes"] / r["ms"] / 1e6
        share = f"{gbs / rate:>8.1%}" if rate and not name.startswith("torch") else f"{'':>8}"
        lines.append(f"{name:<18}{r['batch']:>6}{r['T']:>6}{r['bytes'] / 1e6:>9.1f}{r['ms']:>10.4f}{r['ms_min']:>10.4f}{r['ms_max']:>10.4f}"
                     f"{(r['ms_max'] - r['ms_min']) / r['ms']:>8.1%}{gbs:>9.1f}{share}")
    lines.append("")
    for t, k in PAIRS:
        if t in rows and k in rows:
            lines.append(f"{t} / {k} = {rows[t]['ms'] / rows[k]['ms']:.2f}")
    if "chroma_cqt_y" in rows and "cqt_fold" in rows:
        lines.append(f"cqt_fold / chroma_cqt_y = {rows['cqt_fold']['ms'] / rows['chroma_cqt_y']['ms']:.3f} (the fold's share of chroma_cqt from audio)")
    return "\n".join(lines) + "\n"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--samples", type=int, default=220500)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--skip", choices=list(STEPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "chroma_timings.txt"))
    a = p.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a)))
        return 0
    rows = {}
    for name, limit in STEPS.items():
        if name in a.skip:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", name,
               "--batch", str(a.batch), "--samples", str(a.samples), "--ramp", str(a.ramp)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:           # a fault, an abort or the time limit: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            print(f"step {name} ended with status {r.returncode}; stopping", file=sys.stderr)
            return 1
        rows[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rows[name]), flush=True)
    text = report(rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
