"""Steady-state times of onset_strength and onset_detect on the headline batch (256 clips x 220 500 samples @22.05 kHz,
n_fft 2048, hop 512: a 256 x 128 x 431 mel spectrogram in `melspectrogram`'s line-padded layout).

Protocol of tools/bench_configs.py (`steady`): inputs resident in HBM, three rotating input buffers, ramp-up with the
operator itself, median of 5 back-to-back streams timed with HIP events.  The flux rows are reported against their byte
floor (4 B read per element of S, at 6 TB/s) and against the composed route: the package's own power_to_db followed by
torch slicing / maximum / mean.

  python tools/onset_bench.py                        # every step, each in a child process under its own time limit;
                                                     # writes profiles/onset_timings.txt (--out to choose another file)
  python tools/onset_bench.py --only strength_S      # one step in this process, one JSON line (for a kernel trace of it)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# step -> time limit in seconds
STEPS = {"strength_y": 120, "melspectrogram": 120, "strength_S": 120, "strength_S_max3": 120, "strength_mel_db_on_load": 120,
         "composed_db_torch": 120, "composed_torch_only": 120, "detect_envelope": 120, "detect_envelope_backtrack": 120}
FLOOR_BYTES = 4
HBM = 6e12


def run_step(name, a):
    import torch

    import mlx_audio_primitives_amd as ap
    from mlx_audio_primitives_amd import _extension as _x
    from tools.bench_configs import N_ROT, steady

    g = torch.Generator(device="cuda").manual_seed(42)
    B, L = a.batch, a.samples
    rep = {"step": name, "batch": B, "samples": L}
    ys = [torch.randn((B, L), device="cuda", generator=g) * 0.1 for _ in range(N_ROT)]
    if name == "strength_y":
        rep["ms"] = steady(lambda i: ap.onset_strength(y=ys[i % N_ROT]), ramp_s=a.ramp)
        rep["elements"] = B * 128 * (1 + L // 512)
        return rep
    if name == "melspectrogram":
        rep["ms"] = steady(lambda i: ap.melspectrogram(ys[i % N_ROT]), ramp_s=a.ramp)
        rep["elements"] = B * 128 * (1 + L // 512)
        return rep
    mels = [ap.melspectrogram(y) for y in ys]
    del ys
    _, M, T = mels[0].shape
    rep.update(M=M, T=T, row_stride=int(mels[0].stride(1)), elements=B * M * T)
    if name == "strength_mel_db_on_load":
        # the flux kernel alone on the route from audio: mel power in, dB on load against the key of max(mel)
        keys = []
        for m in mels:
            k = torch.empty(1, dtype=torch.int32, device="cuda")
            _x.check(_x.dlib(m.device).ap_reduce_max_f32(_x.ptr(m.contiguous()), m.numel(), k.data_ptr(), _x.stream_ptr(m.device)))
            keys.append(k)
        outs = [torch.empty((B, T), device="cuda") for _ in range(N_ROT)]

        def flux(i):
            m = mels[i % N_ROT]
            _x.check(_x.dlib(m.device).ap_onset_strength_f32(_x.ptr(m), B, M, T, int(m.stride(1)), None, 0, 1, 1, 3, 1, 10.0,
                                                             1e-10, 1.0, 80.0, keys[i % N_ROT].data_ptr(),
                                                             _x.ptr(outs[i % N_ROT]), T, _x.stream_ptr(m.device)))
        rep["ms"] = steady(flux, ramp_s=a.ramp)
        return rep
    dbs = [ap.power_to_db(m) for m in mels]
    if name == "strength_S":
        rep["ms"] = steady(lambda i: ap.onset_strength(S=dbs[i % N_ROT]), ramp_s=a.ramp)
    elif name == "strength_S_max3":
        rep["ms"] = steady(lambda i: ap.onset_strength(S=dbs[i % N_ROT], max_size=3), ramp_s=a.ramp)
    elif name in ("composed_db_torch", "composed_torch_only"):
        with_db = name == "composed_db_torch"

        def composed(i):
            S = ap.power_to_db(mels[i % N_ROT]) if with_db else dbs[i % N_ROT]
            flux = torch.clamp_min(S[..., 1:] - S[..., :-1], 0.0).mean(dim=-2)
            return torch.nn.functional.pad(flux, (3, 0))[..., :T]
        rep["ms"] = steady(composed, ramp_s=a.ramp)
    else:
        envs = [ap.onset_strength(S=d) for d in dbs]
        del dbs, mels
        bt = name.endswith("backtrack")
        rep["ms"] = steady(lambda i: ap.onset_detect(onset_envelope=envs[i % N_ROT], sparse=False, backtrack=bt), ramp_s=a.ramp)
        rep["elements"] = B * T
    return rep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--samples", type=int, default=220500)
    p.add_argument("--ramp", type=float, default=0.5)
    p.add_argument("--only", choices=list(STEPS))
    p.add_argument("--skip", choices=list(STEPS), action="append", default=[])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "onset_timings.txt"))
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
    lines = ["onset timings (tools/onset_bench.py): ms per call, steady state, HIP events, three rotating inputs",
             f"floor = {FLOOR_BYTES} B per element of S at {HBM / 1e12:.0f} TB/s (flux rows only)", ""]
    lines.append(f"{'step':<28}{'batch':>6}{'ms':>10}{'ns/elem':>10}{'x floor':>9}")
    for name, r in rows.items():
        floor_ms = r["elements"] * FLOOR_BYTES / HBM * 1e3
        flux = name.startswith(("strength_S", "strength_mel", "composed"))
        lines.append(f"{name:<28}{r['batch']:>6}{r['ms']:>10.4f}{r['ms'] * 1e6 / r['elements']:>10.4f}"
                     + (f"{r['ms'] / floor_ms:>9.1f}" if flux else f"{'':>9}"))
    if "strength_S" in rows:
        lines.append("")
        for other in ("composed_db_torch", "composed_torch_only"):
            if other in rows:
                lines.append(f"{other} / strength_S = {rows[other]['ms'] / rows['strength_S']['ms']:.2f}")
    if "strength_y" in rows and "melspectrogram" in rows:
        lines.append(f"strength_y - melspectrogram = {rows['strength_y']['ms'] - rows['melspectrogram']['ms']:.4f} ms")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
