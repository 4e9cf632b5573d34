"""Accuracy and steady-state times of phase_vocoder / time_stretch (csrc/kernels_pv.h, effects.py).

Protocol of tools/pcen_bench.py (`streams`): inputs resident in HBM, three rotating buffers, ramp-up with the operator
itself, 5 back-to-back streams timed with HIP events; reported: the median stream and the spread of the five.  The
kernel reads 8 T and writes 8 T_out bytes per row; GB/s is that over the time, the share of HBM over 8 TB/s.  Beside each
kernel time: the same recurrence composed in torch on the same GPU (gather, angle, wrap, cumsum, polar), float32.
Shapes: n_fft 2048 spectra (1025 rows per clip) of 10 s clips (431 frames) in `stft`'s line-padded layout at rates 0.8 and
1.25, and 10 min clips at rate 0.8 (n_fft 2048: 25840 frames; n_fft 512, hop 128: 257 rows of 103360 frames) under the
host's choice of waves per row and with each other choice forced through AP_PV_WAVES.

  python tools/pv_bench.py                 # every step, each in a child process under its own time limit; writes
                                           # profiles/pv_timings.txt (--out to choose another file)
  python tools/pv_bench.py --only b64_r0.8 # one step in this process, one JSON line
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12
# step -> (batch, bins, frames, rate, waves per row forced through AP_PV_WAVES or 0 for the host's rule)
KERNEL_STEPS = {"b64_r0.8": (64, 1025, 431, 0.8, 0), "b64_r1.25": (64, 1025, 431, 1.25, 0), "b256_r0.8": (256, 1025, 431, 0.8, 0),
                "b256_r1.25": (256, 1025, 431, 1.25, 0), "long_b4": (4, 1025, 25840, 0.8, 0),
                "long_b1": (1, 1025, 25840, 0.8, 0), "long_b1_w1": (1, 1025, 25840, 0.8, 1), "long_b1_w16": (1, 1025, 25840, 0.8, 16),
                "n512_b1": (1, 257, 103360, 0.8, 0), "n512_b1_w4": (1, 257, 103360, 0.8, 4), "n512_b1_w1": (1, 257, 103360, 0.8, 1)}
STEPS = ["accuracy"] + list(KERNEL_STEPS) + ["stretch_b64"]
LIMIT = 180          # seconds per step


def torch_pv(D, rate):
    """librosa's recurrence in torch ops: what a torch user would write."""
    import torch

    F, T = D.shape[-2:]
    steps = torch.arange(0, T, rate, dtype=torch.float64, device=D.device)
    idx = steps.floor().long()
    a = (steps - steps.floor()).float()
    Dp = torch.nn.functional.pad(D, (0, 2))
    c0, c1 = Dp[..., idx], Dp[..., idx + 1]
    mag = (1.0 - a) * c0.abs() + a * c1.abs()
    phi = torch.linspace(0, math.pi * ((2 * (F - 1)) // 4), F, device=D.device)[:, None]
    d = c1.angle() - c0.angle() - phi
    d = d - 2.0 * math.pi * torch.round(d / (2.0 * math.pi)) + phi
    acc = D[..., :1].angle() + torch.cumsum(d, -1) - d
    return torch.polar(mag, acc)


def run_step(name, a):
    import numpy as np
    import torch

    if KERNEL_STEPS.get(name, (0,) * 5)[4]:
        os.environ["AP_PV_WAVES"] = str(KERNEL_STEPS[name][4])      # read once, at the library's first launch
    import mlx_audio_primitives_amd as ap
    from mlx_audio_primitives_amd import _extension as _x
    from tools.bench_configs import N_ROT
    from tools.pcen_bench import streams

    rep = {"step": name}
    if name == "accuracy":
        import pv_ref as R

        rep["cases"] = {}
        for c in R.CASES:
            D, want, twin = R.reference(*c[:4])
            got = ap.phase_vocoder(torch.from_numpy(np.array(D)).cuda(), rate=c[3]).cpu().numpy()
            rep["cases"][R.case_id(c)] = [twin, R.worst_ratio(got, D, want, twin)]
        return rep
    g = torch.Generator(device="cuda").manual_seed(42)
    if name == "stretch_b64":
        ys = [torch.randn((64, 220500), device="cuda", generator=g) * 0.1 for _ in range(N_ROT)]
        for rate in (0.8, 1.25):
            ts = streams(lambda i: ap.time_stretch(ys[i % N_ROT], rate=rate), a.ramp)
            ts_rt = streams(lambda i: ap.istft(ap.stft(ys[i % N_ROT]), length=220500), a.ramp)
            rep[f"rate{rate}"] = dict(ms=ts[2], ms_min=ts[0], ms_max=ts[-1], stft_istft_ms=ts_rt[2])
        return rep
    B, F, T, rate, _ = KERNEL_STEPS[name]
    Ts = -(-T // 16) * 16
    T_out = int(_x.lib().ap_phase_vocoder_frames(T, rate))
    Ds = [torch.view_as_complex(torch.randn((B, F, Ts, 2), device="cuda", generator=g))[:, :, :T] for _ in range(N_ROT)]
    ts = streams(lambda i: ap.phase_vocoder(Ds[i % N_ROT], rate=rate), a.ramp)
    rep.update(batch=B, T=T, T_out=T_out, rate=rate, waves=int(_x.lib().ap_phase_vocoder_waves(B * F, T_out)),
               bytes=8 * (T + T_out) * B * F, ms=ts[2], ms_min=ts[0], ms_max=ts[-1])
    dense = [d.contiguous() for d in Ds]
    del Ds
    diff = (torch_pv(dense[0][:1], rate) - ap.phase_vocoder(dense[0][:1], rate=rate)).abs().max().item()
    rep["torch_max_diff"] = diff              # (float32 angles: grows with T_out)
    tt = streams(lambda i: torch_pv(dense[i % N_ROT], rate), a.ramp)
    rep.update(torch_ms=tt[2])
    return rep


def report(rows):
    lines = ["phase_vocoder / time_stretch (tools/pv_bench.py) on an MI355X", "",
             "accuracy: max over rows of |out - ref64| / (float32 twin's error x row max |D|), bound 4 (tests/pv_ref.py)",
             f"{'case':<34}{'twin error':>12}{'worst ratio':>13}"]
    for cid, (twin, ratio) in rows.get("accuracy", {}).get("cases", {}).items():
        lines.append(f"{cid:<34}{twin:>12.2e}{ratio:>13.2f}")
    lines += ["", "kernel (public call on a line-padded view, output allocated by the call): ms per call, steady state, HIP events,",
              "median of 5 streams; GB/s = 8 (T + T_out) bytes per row / time; HBM = share of 8 TB/s; torch = the torch composition", "",
              f"{'step':<12}{'batch':>6}{'T':>7}{'T_out':>7}{'W':>4}{'ms':>10}{'min':>10}{'max':>10}{'GB/s':>8}{'HBM':>7}{'torch ms':>10}{'torch/ours':>11}"]
    for name in KERNEL_STEPS:
        r = rows.get(name)
        if r:
            gbs = r["bytes"] / r["ms"] / 1e6
            lines.append(f"{name:<12}{r['batch']:>6}{r['T']:>7}{r['T_out']:>7}{r['waves']:>4}{r['ms']:>10.4f}{r['ms_min']:>10.4f}"
                         f"{r['ms_max']:>10.4f}{gbs:>8.0f}{gbs * 1e9 / HBM_BYTES_PER_S:>7.1%}{r['torch_ms']:>10.3f}{r['torch_ms'] / r['ms']:>11.1f}")
    lines += ["", "long_b1* / n512_b1*: one 10 min clip (n_fft 2048 hop 512; n_fft 512 hop 128) under the host's rule and with the",
              "waves per row forced (_w1, _w4, _w16): what the multi-wave variants buy where rows alone do not fill the chip"]
    if "stretch_b64" in rows:
        lines += ["", "time_stretch, 64 clips x 220 500 samples, n_fft 2048 (stft + phase_vocoder + istft); beside it stft + istft alone:"]
        for k, r in rows["stretch_b64"].items():
            if k.startswith("rate"):
                lines.append(f"  {k:<10}{r['ms']:>9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f}); stft + istft {r['stft_istft_ms']:.3f} ms")
    return "\n".join(lines) + "\n"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ramp", type=float, default=0.3)
    p.add_argument("--only", choices=STEPS)
    p.add_argument("--skip", choices=STEPS, action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pv_timings.txt"))
    a = p.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a)))
        return 0
    rows = {}
    for name in STEPS:
        if name in a.skip:
            continue
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--only", name, "--ramp", str(a.ramp)]
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
