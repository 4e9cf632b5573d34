"""Steady-state times of piptrack / estimate_tuning on 256 clips x 10 s @22.05 kHz (n_fft 2048, hop 512: 431 frames x 1025
bins per clip).

Protocol of tools/bench_configs.py (`steady`, through tools/pcen_bench.streams): inputs resident in HBM, three rotating
input buffers, ramp-up with the operator itself, 5 back-to-back streams timed with HIP events; reported: the median
stream and the spread of the five.  The peak kernel does a dozen operations per bin, so the yardstick is memory
traffic: the bytes a step has to move (its input once, its outputs once; the compact mode writes next to nothing) at
the rate `preemphasis` reaches on 256 x 220 500 samples in the same session.  Each step is also timed against the same
steps composed from torch operators on the same device (the STFT in front of them is this package's in both).
estimate_tuning returns a host float: its time includes the read-back of the counters and counts, and so does the
torch composition's (.item()).

  python tools/piptrack_bench.py                    # every step, each in a child process under its own time limit;
                                                    # writes profiles/piptrack_timings.txt (--out to choose another file)
  python tools/piptrack_bench.py --only piptrack_S  # one step in this process, one JSON line
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pcen_bench import streams  # noqa: E402

STEPS = {"preemphasis": 120, "stft": 120, "piptrack_S": 180, "torch_piptrack_S": 240, "piptrack_y": 180, "torch_piptrack_y": 240,
         "estimate_tuning_y": 180, "estimate_tuning_per_clip_y": 180, "torch_estimate_tuning_y": 300}
PAIRS = (("torch_piptrack_S", "piptrack_S"), ("torch_piptrack_y", "piptrack_y"), ("torch_estimate_tuning_y", "estimate_tuning_y"))
SR, N_FFT, HOP = 22050, 2048, 512


def torch_piptrack(S, k_lo, k_hi, threshold=0.1):
    """librosa's piptrack on a magnitude tensor (B, F, T) with torch operators."""
    import torch

    tiny = torch.finfo(torch.float32).tiny
    avg = torch.zeros_like(S)
    shift = torch.zeros_like(S)
    a, b, c = S[:, :-2], S[:, 1:-1], S[:, 2:]
    avg[:, 1:-1] = 0.5 * (c - a)
    den = 2.0 * b - c - a
    shift[:, 1:-1] = avg[:, 1:-1] / (den + (den.abs() < tiny).float())
    dskew = 0.5 * avg * shift
    X = torch.where(S > threshold * S.amax(dim=1, keepdim=True), S, torch.zeros_like(S))
    peak = torch.zeros_like(S, dtype=torch.bool)
    peak[:, 1:-1] = (X[:, 1:-1] > X[:, :-2]) & (X[:, 1:-1] >= X[:, 2:])
    peak[:, -1] = X[:, -1] > X[:, -2]
    peak[:, :k_lo] = False
    peak[:, k_hi:] = False
    k = torch.arange(S.shape[1], device=S.device, dtype=torch.float32)[None, :, None]
    zero = torch.zeros_like(S)
    return torch.where(peak, (k + shift) * (SR / N_FFT), zero), torch.where(peak, S + dskew, zero)


def torch_estimate_tuning(S, k_lo, k_hi):
    import torch

    p, m = torch_piptrack(S, k_lo, k_hi)
    sel = p > 0
    thr = torch.median(m[sel])
    f = p[sel & (m >= thr)].double()
    r = torch.remainder(12.0 * torch.log2(f / 27.5), 1.0)
    r = torch.where(r >= 0.5, r - 1.0, r)
    counts = torch.histc(r, bins=100, min=-0.5, max=0.5)
    return -0.5 + 0.01 * float(counts.argmax().item())


def run_step(name, a):
    import importlib

    import torch

    import mlx_audio_primitives_amd as ap
    from tools.bench_configs import N_ROT

    M = importlib.import_module("mlx_audio_primitives_amd.pitch")
    g = torch.Generator(device="cuda").manual_seed(42)
    B, L = a.batch, a.samples
    T, F = 1 + L // HOP, N_FFT // 2 + 1
    k_lo, k_hi = M._bin_range(SR, N_FFT, 150.0, 4000.0, F)
    rep = {"step": name, "batch": B, "samples": L, "T": T}

    def rand(*shape):
        return torch.rand(shape, device="cuda", generator=g)

    def tonal():
        n = torch.arange(L, device="cuda") / SR
        f0 = 110.0 * 2.0 ** (rand(B, 1) * 3.0)
        return sum(torch.cos(2 * torch.pi * f0 * h * n + h) / h for h in (1, 2, 3, 4)) * 0.2 + 0.01 * (rand(B, L) - 0.5)

    if name == "preemphasis":
        ys = [rand(B, L) for _ in range(N_ROT)]
        fn = lambda i: ap.preemphasis(ys[i % N_ROT])                                       # noqa: E731
        rep["bytes"] = 8.0 * B * L
    elif name == "stft":
        ys = [tonal() for _ in range(N_ROT)]
        fn = lambda i: ap.stft(ys[i % N_ROT], n_fft=N_FFT, hop_length=HOP)                 # noqa: E731
        rep["bytes"] = 4.0 * B * L + 8.0 * B * F * T
    elif name in ("piptrack_S", "torch_piptrack_S"):
        Ss = [ap.magnitude(ap.stft(tonal(), n_fft=N_FFT, hop_length=HOP)).contiguous() for _ in range(N_ROT)]
        rep["bytes"] = 12.0 * B * F * T
        if name == "piptrack_S":
            fn = lambda i: ap.piptrack(S=Ss[i % N_ROT], sr=SR)                             # noqa: E731
        else:
            fn = lambda i: torch_piptrack(Ss[i % N_ROT], k_lo, k_hi)                       # noqa: E731
        rep["peaks"] = float((ap.piptrack(S=Ss[0], sr=SR)[0] > 0).float().mean())
    else:
        ys = [tonal() for _ in range(N_ROT)]
        if name in ("piptrack_y", "torch_piptrack_y"):
            rep["bytes"] = 4.0 * B * L + 16.0 * B * F * T + 8.0 * B * F * T              # stft out + in again, two outputs
            if name == "piptrack_y":
                fn = lambda i: ap.piptrack(y=ys[i % N_ROT], sr=SR, hop_length=HOP)         # noqa: E731
            else:
                fn = lambda i: torch_piptrack(ap.stft(ys[i % N_ROT], n_fft=N_FFT, hop_length=HOP).abs(), k_lo, k_hi)   # noqa: E731
        else:
            rep["bytes"] = 4.0 * B * L + 16.0 * B * F * T                                  # stft out + in again; records are ~2 %
            if name == "estimate_tuning_y":
                fn = lambda i: ap.estimate_tuning(y=ys[i % N_ROT], sr=SR, hop_length=HOP)  # noqa: E731
            elif name == "estimate_tuning_per_clip_y":
                fn = lambda i: ap.estimate_tuning(y=ys[i % N_ROT], sr=SR, hop_length=HOP, per_clip=True)   # noqa: E731
            else:
                fn = lambda i: torch_estimate_tuning(ap.stft(ys[i % N_ROT], n_fft=N_FFT, hop_length=HOP).abs(), k_lo, k_hi)   # noqa: E731
    ts = streams(fn, a.ramp)
    rep.update(ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1])
    return rep


def report(rows):
    lines = ["piptrack timings (tools/piptrack_bench.py): ms per call, steady state, HIP events, three rotating inputs;",
             "median of 5 back-to-back streams, spread = (max - min) / median of the five",
             "GB/s = (bytes a step must move: input once + outputs once, an stft result written and read again) / time;",
             "stream = share of the rate preemphasis reaches in the same session", ""]
    rate = rows["preemphasis"]["bytes"] / rows["preemphasis"]["ms"] / 1e6 if "preemphasis" in rows else None
    lines.append(f"{'step':<28}{'batch':>6}{'T':>6}{'MB':>9}{'ms':>10}{'min':>10}{'max':>10}{'spread':>8}{'GB/s':>9}{'stream':>8}")
    for name, r in rows.items():
        gbs = r["bytes"] / r["ms"] / 1e6
        share = f"{gbs / rate:>8.1%}" if rate and not name.startswith("torch") else f"{'':>8}"
        lines.append(f"{name:<28}{r['batch']:>6}{r['T']:>6}{r['bytes'] / 1e6:>9.1f}{r['ms']:>10.4f}{r['ms_min']:>10.4f}{r['ms_max']:>10.4f}"
                     f"{(r['ms_max'] - r['ms_min']) / r['ms']:>8.1%}{gbs:>9.1f}{share}")
    lines.append("")
    if "piptrack_S" in rows and "peaks" in rows["piptrack_S"]:
        lines.append(f"peaks: {rows['piptrack_S']['peaks']:.4%} of the bins of the benchmark's input")
    for t, k in PAIRS:
        if t in rows and k in rows:
            lines.append(f"{t} / {k} = {rows[t]['ms'] / rows[k]['ms']:.2f}")
    for k in ("piptrack_y", "estimate_tuning_y", "estimate_tuning_per_clip_y"):
        if k in rows and "stft" in rows:
            lines.append(f"{k} - stft = {rows[k]['ms'] - rows['stft']['ms']:.4f} ms")
    return "\n".join(lines) + "\n"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--samples", type=int, default=220500)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--skip", choices=list(STEPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "piptrack_timings.txt"))
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
