"""Steady-state times of tempogram, tempo and beat_track on the headline batch's envelopes (256 clips x 431 frames: 10 s
at 22.05 kHz, hop 512).

Protocol of tools/bench_configs.py (`steady`): inputs resident in HBM, three rotating input buffers, ramp-up with the
operator itself, median of 5 back-to-back streams timed with HIP events.  The tempogram rows are reported against their
byte floor (4 B written per element of the tempogram, at 5 TB/s), against the general kernel forced onto the same shape
and against a torch composition on the same inputs
(unfold x window, rfft / irfft at 1024 points, slice, max-normalise).

  python tools/rhythm_bench.py                       # every step, each in a child process under its own time limit;
                                                     # writes profiles/rhythm_timings.txt (--out to choose another file)
  python tools/rhythm_bench.py --only tempogram      # one step in this process, one JSON line (for a kernel trace of it)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# step -> time limit in seconds
STEPS = {"tempogram": 180, "tempogram_344": 180, "tempogram_general": 180, "composed_torch": 180, "tempo_envelope": 180, "tempo_stored_tg": 180,
         "beat_track_envelope": 180, "beat_track_bpm": 180, "onset_strength": 180, "beat_track_audio": 180}
HBM = 5e12


def envelopes(B, T, n_rot):
    """Click trains at 90 .. 180 bpm over a noise floor, float32 on the device."""
    import numpy as np
    import torch

    rng = np.random.default_rng(42)
    out = []
    for _ in range(n_rot):
        e = np.abs(rng.normal(0.0, 0.15, (B, T)))
        for b in range(B):
            period = rng.uniform(14.0, 29.0)
            pos = np.round(np.arange(rng.uniform(0, period), T, period)).astype(int)
            e[b, pos[pos < T]] += 1.0
        out.append(torch.from_numpy(e.astype(np.float32)).cuda())
    return out


def run_step(name, a):
    import numpy as np
    import torch

    import mlx_audio_primitives_amd as ap
    from tools.bench_configs import N_ROT, steady

    B, T = a.batch, a.frames
    rep = {"step": name, "batch": B, "frames": T}
    if name in ("onset_strength", "beat_track_audio"):
        g = torch.Generator(device="cuda").manual_seed(42)
        ys = [torch.randn((B, (T - 1) * 512), device="cuda", generator=g) * 0.1 for _ in range(N_ROT)]
        if name == "onset_strength":
            rep["ms"] = steady(lambda i: ap.onset_strength(y=ys[i % N_ROT]), ramp_s=a.ramp)
        else:
            rep["ms"] = steady(lambda i: ap.beat_track(y=ys[i % N_ROT], sparse=False), ramp_s=a.ramp)
        return rep
    envs = envelopes(B, T, N_ROT)
    W = 344 if name in ("tempogram_344", "tempo_envelope", "tempo_stored_tg") else 384
    rep["win_length"] = W
    if name == "tempogram_general":
        os.environ["AP_TEMPOGRAM_GENERAL"] = "1"       # the direct-sum kernel on the wave kernel's shape
    if name in ("tempogram", "tempogram_344", "tempogram_general"):
        rep["ms"] = steady(lambda i: ap.tempogram(onset_envelope=envs[i % N_ROT], win_length=W), ramp_s=a.ramp)
        rep["elements"] = B * W * T
    elif name == "composed_torch":
        w = ap.get_window("hann", W, device="cuda")
        h = W // 2
        ramp = torch.arange(h, device="cuda", dtype=torch.float32) / h

        def composed(i):
            e = envs[i % N_ROT]
            p = torch.cat([e[:, :1] * ramp, e, e[:, -1:] * ramp.flip(0)], dim=1)
            x = p.unfold(1, W, 1)[:, :T] * w
            ac = torch.fft.irfft(torch.fft.rfft(x, n=1024).abs().square(), n=1024)[..., :W]
            tg = ac / ac.abs().amax(dim=-1, keepdim=True).clamp_min(1.17549435e-38)
            return tg.transpose(1, 2).contiguous()
        rep["ms"] = steady(composed, ramp_s=a.ramp)
        rep["elements"] = B * W * T
        got, want = composed(0), ap.tempogram(onset_envelope=envs[0], win_length=W)
        rep["max_abs_diff"] = float((got - want).abs().max())
    elif name == "tempo_envelope":
        rep["ms"] = steady(lambda i: ap.tempo(onset_envelope=envs[i % N_ROT]), ramp_s=a.ramp)
    elif name == "tempo_stored_tg":
        def stored(i):
            return ap.tempo(tg=ap.tempogram(onset_envelope=envs[i % N_ROT], win_length=W))
        rep["ms"] = steady(stored, ramp_s=a.ramp)
    elif name == "beat_track_envelope":
        rep["ms"] = steady(lambda i: ap.beat_track(onset_envelope=envs[i % N_ROT], sparse=False), ramp_s=a.ramp)
    elif name == "beat_track_bpm":
        bpm = np.full(B, 120.0)
        rep["ms"] = steady(lambda i: ap.beat_track(onset_envelope=envs[i % N_ROT], bpm=bpm, sparse=False), ramp_s=a.ramp)
    return rep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--frames", type=int, default=431)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--skip", choices=list(STEPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "rhythm_timings.txt"))
    a = p.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a)))
        return 0
    rows = {}
    for name, limit in STEPS.items():
        if name in a.skip:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", name,
               "--batch", str(a.batch), "--frames", str(a.frames), "--ramp", str(a.ramp)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:           # a fault, an abort or the time limit: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            print(f"step {name} ended with status {r.returncode}; stopping", file=sys.stderr)
            return 1
        rows[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rows[name]), flush=True)
    lines = ["rhythm timings (tools/rhythm_bench.py): ms per call, steady state, HIP events, three rotating inputs",
             f"floor = 4 B per element of the tempogram at {HBM / 1e12:.0f} TB/s (tempogram rows only)", ""]
    lines.append(f"{'step':<24}{'batch':>6}{'frames':>8}{'W':>6}{'ms':>10}{'x floor':>9}")
    for name, r in rows.items():
        floor = f"{r['ms'] / (r['elements'] * 4 / HBM * 1e3):>9.1f}" if "elements" in r else f"{'':>9}"
        lines.append(f"{name:<24}{r['batch']:>6}{r['frames']:>8}{r.get('win_length', ''):>6}{r['ms']:>10.4f}{floor}")
    lines.append("")
    if "composed_torch" in rows:
        lines.append(f"composed_torch against tempogram: max |difference| {rows['composed_torch']['max_abs_diff']:.2e}")
        if "tempogram" in rows:
            lines.append(f"composed_torch / tempogram = {rows['composed_torch']['ms'] / rows['tempogram']['ms']:.2f}")
    if "tempogram_general" in rows and "tempogram" in rows:
        lines.append(f"tempogram_general / tempogram = {rows['tempogram_general']['ms'] / rows['tempogram']['ms']:.2f}")
    if "tempo_envelope" in rows and "tempogram_344" in rows:
        lines.append(f"tempo_envelope / tempogram_344 = {rows['tempo_envelope']['ms'] / rows['tempogram_344']['ms']:.2f}")
    if "beat_track_audio" in rows and "onset_strength" in rows:
        lines.append(f"beat_track_audio - onset_strength = {rows['beat_track_audio']['ms'] - rows['onset_strength']['ms']:.4f} ms")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
