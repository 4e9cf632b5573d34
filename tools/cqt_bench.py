"""Steady-state times of cqt at its defaults on 256 clips x 10 s @22.05 kHz (84 bands, 97 to 11 685 taps, hop 512,
T = 431 frames per clip).

Protocol of tools/bench_configs.py (`steady`): inputs resident in HBM, three rotating input buffers, ramp-up with the
operator itself, 5 back-to-back streams timed with HIP events; reported: the median stream and the spread (min .. max)
of the five.  The transform needs 4 sum L_k flops per frame (one complex tap times one real sample = 2 FMAs) against
8 n_bins output bytes: compute bound by three orders of magnitude, so the yardstick is the float32 FMA peak
(157.3 TFLOP/s, MI355X_MICROARCH).  It is compared with something that is not itself:
  torch_unfold       the same arithmetic composed in torch on the same device: the signal padded once, then per octave of
                     bins `unfold` (a strided view of the frames) times the octave's zero-padded bank as one matmul,
                     real and imaginary parts as columns

  python tools/cqt_bench.py                         # every step, each in a child process under its own time limit;
                                                    # writes profiles/cqt_timings.txt (--out to choose another file)
  python tools/cqt_bench.py --only cqt_kernel       # one step in this process, one JSON line (for a kernel trace of it)
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
STEPS = {"cqt": 180, "cqt_kernel": 180, "cqt_hop256": 180, "vqt": 180, "torch_unfold": 300}
PEAK_TFLOPS = 157.3


def torch_bank(taps, off, m0, s, device):
    """(pad, [(first padded sample of frame 0, width, (width, 2 bins) weights)]) per octave of 12 bins: the scaled,
    conjugated taps on the octave's common tap range, zero outside a band's own."""
    import torch

    Ls = np.diff(off)
    m0 = m0.astype(np.int64)
    pad = int(max((-m0).max(), (m0 + Ls).max()))
    groups = []
    for k0 in range(0, len(m0), 12):
        ks = range(k0, min(k0 + 12, len(m0)))
        lo = min(int(m0[k]) for k in ks)
        hi = max(int(m0[k] + Ls[k]) for k in ks)
        W = np.zeros((hi - lo, 2 * len(ks)), np.float32)
        for j, k in enumerate(ks):
            gk = taps[off[k]:off[k + 1]] * s[k]
            W[m0[k] - lo:m0[k] - lo + Ls[k], 2 * j] = gk.real
            W[m0[k] - lo:m0[k] - lo + Ls[k], 2 * j + 1] = -gk.imag
        groups.append((pad + lo, hi - lo, torch.from_numpy(W).to(device)))
    return pad, groups


def torch_cqt(y, pad, groups, hop, chunk):
    """(B, T, 2 n_bins) float32, (re, im) interleaved along the last axis: constant padding, then per octave the
    strided view of the frames times the octave's bank."""
    import torch

    B, L = y.shape
    T = 1 + L // hop
    yp = torch.nn.functional.pad(y, (pad, pad))
    outs = []
    for b0 in range(0, B, chunk):
        cols = [torch.matmul(yp[b0:b0 + chunk, start:].unfold(-1, width, hop)[:, :T], W) for start, width, W in groups]
        outs.append(torch.cat(cols, -1))
    return torch.cat(outs, 0)


def run_step(name, a):
    import torch

    import mlx_audio_primitives_amd as ap
    from mlx_audio_primitives_amd import _extension as _x
    from tools.bench_configs import N_ROT

    C = importlib.import_module("mlx_audio_primitives_amd.cqt")
    g = torch.Generator(device="cuda").manual_seed(42)
    B, L = a.batch, a.samples
    hop = 256 if name == "cqt_hop256" else 512
    T = 1 + L // hop
    func = "vqt" if name == "vqt" else "cqt"
    args, pad_code = C._parameters(22050, hop, None, 84, 12, 0.0, 1, 1, 0.01, "hann", True, "constant", None,
                                   None if func == "vqt" else 0.0, "equal")
    host = C._bank(*args)
    taps, off, m0, s, _ = host
    Ls = np.diff(off)
    flops = 4.0 * float(Ls.sum()) * T * B
    rep = {"step": name, "batch": B, "samples": L, "hop": hop, "T": T, "n_bins": 84, "sum_taps": int(Ls.sum()), "flops": flops}
    ys = [torch.randn((B, L), device="cuda", generator=g) * 0.1 for _ in range(N_ROT)]
    if name == "torch_unfold":
        pad, groups = torch_bank(taps, off, m0, s, "cuda")
        chunk = max(1, min(B, a.torch_chunk))

        def compose(i):
            return torch_cqt(ys[i % N_ROT], pad, groups, hop, chunk)
        ts = streams(compose, a.ramp)
        rep["torch_chunk"] = chunk
    elif name == "cqt_kernel":
        dev = ys[0].device
        bank = C._device_bank(host, dev)
        outs = [torch.empty((B, 84, T), dtype=torch.complex64, device=dev) for _ in range(N_ROT)]

        def kernel(i):
            y = ys[i % N_ROT]
            _x.check(_x.dlib(dev).ap_cqt_f32(_x.ptr(y), B, L, hop, pad_code, _x.ptr(bank[0]), _x.ptr(bank[1]), _x.ptr(bank[2]),
                                             _x.ptr(bank[3]), 84, T, _x.ptr(outs[i % N_ROT]), T, _x.stream_ptr(dev)))
        ts = streams(kernel, a.ramp)
    else:
        f = getattr(ap, func)
        ts = streams(lambda i: f(ys[i % N_ROT], hop_length=hop), a.ramp)
    rep.update(ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1])
    return rep


def report(rows):
    """The text of profiles/cqt_timings.txt for {step: row of run_step}."""
    lines = ["cqt timings (tools/cqt_bench.py): ms per call, steady state, HIP events, three rotating inputs;",
             "median of 5 back-to-back streams, spread = (max - min) / median of the five",
             f"TFLOP/s = 4 sum L_k flops per frame / time; peak = share of the float32 FMA peak ({PEAK_TFLOPS} TFLOP/s)", ""]
    lines.append(f"{'step':<16}{'batch':>6}{'hop':>5}{'T':>6}{'sum L_k':>9}{'ms':>10}{'min':>10}{'max':>10}{'spread':>8}{'TFLOP/s':>9}{'peak':>7}")
    for name, r in rows.items():
        tf = r["flops"] / r["ms"] / 1e9
        lines.append(f"{name:<16}{r['batch']:>6}{r['hop']:>5}{r['T']:>6}{r['sum_taps']:>9}{r['ms']:>10.4f}{r['ms_min']:>10.4f}"
                     f"{r['ms_max']:>10.4f}{(r['ms_max'] - r['ms_min']) / r['ms']:>8.1%}{tf:>9.2f}{tf / PEAK_TFLOPS:>7.1%}")
    lines.append("")
    if "cqt" in rows and "torch_unfold" in rows:
        lines.append(f"torch_unfold / cqt = {rows['torch_unfold']['ms'] / rows['cqt']['ms']:.2f} "
                     f"(torch: pad, then unfold x zero-padded bank per octave, batch chunks of {rows['torch_unfold']['torch_chunk']})")
    return "\n".join(lines) + "\n"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--samples", type=int, default=220500)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--torch-chunk", type=int, default=32, help="clips per matmul of the torch composition")
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--skip", choices=list(STEPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "cqt_timings.txt"))
    a = p.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a)))
        return 0
    rows = {}
    for name, limit in STEPS.items():
        if name in a.skip:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", name,
               "--batch", str(a.batch), "--samples", str(a.samples), "--ramp", str(a.ramp), "--torch-chunk", str(a.torch_chunk)]
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
