"""Steady-state times of hpss on the headline spectrum (256 clips x 220 500 samples @22.05 kHz, n_fft 2048, hop 512:
256 x 1025 x 431 complex64 in `stft`'s line-padded layout), on the network kernel and on the rank-counting kernel.

Protocol of tools/bench_configs.py (`steady`): inputs resident in HBM, three rotating input buffers, ramp-up with the
operator itself, median of 5 back-to-back streams timed with HIP events.  Every row is reported against the byte
floor of the full operator (8 B read + 2 x 8 B written per element = 24 B, at 6 TB/s) and, where both ran, against
the general kernel.

  python tools/hpss_bench.py                     # every step, each in a child process under its own time limit;
                                                 # writes profiles/hpss_timings.txt (--out to choose another file)
  python tools/hpss_bench.py --only fused_mode0  # one step in this process, one JSON line (for a kernel trace of it)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# step -> time limit in seconds
STEPS = {"fused_mode0": 120, "fused_mode1": 120, "fused_harmonic_only": 120, "fused_medians": 120,
         "general_mode0": 240, "general_mode1": 240, "harmonic_audio": 180, "hpss_audio": 180, "torch_unfold_median_b32": 180}
FLOOR_BYTES = 24
HBM = 6e12


def run_step(name, a):
    import torch

    import mlx_audio_primitives_amd as ap
    from mlx_audio_primitives_amd import decompose as dec
    from tools.bench_configs import N_ROT, steady

    g = torch.Generator(device="cuda").manual_seed(42)
    B, L = a.batch, a.samples
    rep = {"step": name, "batch": B, "samples": L}
    if name == "torch_unfold_median_b32":
        B = min(B, 32)
        rep["batch"] = B
    ys = [torch.randn((B, L), device="cuda", generator=g) * 0.1 for _ in range(N_ROT)]
    if name in ("hpss_audio", "harmonic_audio"):
        fn = ap.hpss_audio if name == "hpss_audio" else ap.harmonic
        rep["ms"] = steady(lambda i: fn(ys[i % N_ROT]), ramp_s=a.ramp)
        rep["elements"] = B * 1025 * (1 + L // 512)
        return rep
    Ss = [ap.stft(y, n_fft=2048, hop_length=512) for y in ys]
    del ys
    _, F, T = Ss[0].shape
    rep.update(F=F, T=T, row_stride=int(Ss[0].stride(1)), elements=B * F * T)
    if name == "torch_unfold_median_b32":
        # for scale only: one of the two filters, no reflect padding (T - 30 outputs per row), 31 copies of |S| in HBM
        def comp(i):
            return Ss[i % N_ROT].abs().unfold(-1, 31, 1).median(-1).values
        rep["ms"] = steady(comp, n_launch=2, ramp_s=0.0, streams=3)
        return rep
    general = name.startswith("general")
    mode = {"mode0": 0, "mode1": 1, "harmonic_only": 0, "medians": 2}[name.split("_", 1)[1]]
    want_p = not name.endswith("harmonic_only")
    rep["ms"] = steady(lambda i: dec._run(Ss[i % N_ROT], 31, 31, 1.0, 1.0, 2.0, mode, True, want_p, general),
                       ramp_s=a.ramp)
    return rep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--samples", type=int, default=220500)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--skip", choices=list(STEPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpss_timings.txt"))
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
    lines = ["hpss timings (tools/hpss_bench.py): ms per call, steady state, HIP events, three rotating inputs",
             f"floor = {FLOOR_BYTES} B per element (complex in, two complex out) at {HBM / 1e12:.0f} TB/s", ""]
    lines.append(f"{'step':<26}{'batch':>6}{'ms':>10}{'ns/elem':>10}{'x floor':>9}{'x general':>11}")
    for name, r in rows.items():
        floor_ms = r["elements"] * FLOOR_BYTES / HBM * 1e3
        gen = rows.get(name.replace("fused", "general")) if name.startswith("fused") else None
        lines.append(f"{name:<26}{r['batch']:>6}{r['ms']:>10.3f}{r['ms'] * 1e6 / r['elements']:>10.4f}{r['ms'] / floor_ms:>9.1f}"
                     + (f"{gen['ms'] / r['ms']:>11.2f}" if gen else f"{'':>11}"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
