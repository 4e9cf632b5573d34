"""LDS bank-conflict calculator for gfx950 access patterns (MI355X_MICROARCH.md §LDS).

cycles(kind, byte_addresses[64]) -> LDS-array cycles of one wave64 instruction, using the
guide's lane groups and bank moduli:
  ds_read_b32 : 2 groups of 32 lanes, bank = (a/4) % 32
  ds_read_b64 : 2 groups of 32 lanes, bank = (a/4) % 64, each lane covers 2 banks
  ds_read_b128: 4 groups {0-3,12-15,20-27},{4-11,16-19,28-31},(+32), bank % 64, 4 banks/lane
  ds_write_b32: 2 x 32, % 32 ; ds_write_b64: 4 x 16 contiguous, % 32 ; ds_write_b128: 8 x 8, % 32
Identical addresses broadcast (reads).  Used to choose the paddings in kernels_wave.h.
"""
import numpy as np

G128 = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
        list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
G128 = G128 + [[x + 32 for x in g] for g in G128]


def _groups(kind):
    if kind in ("r32", "r64", "w32"):
        return [list(range(0, 32)), list(range(32, 64))]
    if kind == "r128":
        return G128
    if kind == "w64":
        return [list(range(i, i + 16)) for i in range(0, 64, 16)]
    if kind == "w128":
        return [list(range(i, i + 8)) for i in range(0, 64, 8)]
    raise ValueError(kind)


def cycles(kind, addrs, active=None):
    width = {"r32": 1, "w32": 1, "r64": 2, "w64": 2, "r128": 4, "w128": 4}[kind]
    mod = 64 if kind in ("r64", "r128") else 32
    total = 0
    for g in _groups(kind):
        per_bank = {}
        for lane in g:
            if active is not None and not active[lane]:
                continue
            a = int(addrs[lane]) // 4
            for i in range(width):
                per_bank.setdefault((a + i) % mod, set()).add(a + i)
        total += max([len(v) for v in per_bank.values()] + [1])
    return total


def mel_plan_reads(plan, desc, partial_off=1152, slot_bytes=4):
    """Bank cycles of the filterbank passes of ap_mel2048_run_kernel for a real plan (ap_mel_plan_host): per
    pass the four plane reads (|X|^p groups gA, gA + 1, gB, gB + 1 of the lane's entry, 16 bytes each), the
    four weight reads (row i of pass p at quad 256 p + 64 i + lane) and the two partial-sum stores (slots of
    `slot_bytes` at float offset `partial_off` of the wave's buffer; 8 bytes = the pair contraction).
    Returns a list of (plane cycles, weight cycles, store cycles) per pass; ideal (16, 16, 4 or 8)."""
    n_parts, n_slots = int(desc[12]), int(desc[7])
    parts = np.asarray(plan[desc[11]:desc[11] + 4 * n_parts]).reshape(n_parts, 4)
    lanes = np.arange(64)
    out = []
    for ps in range((n_parts + 63) // 64):
        d = np.tile(np.array([n_slots, 0, n_slots, 0]), (64, 1))          # idle lanes: group 0, dump slot
        n = min(64, n_parts - 64 * ps)
        d[:n] = parts[64 * ps:64 * ps + n]
        plane = sum(cycles("r128", 16 * (d[:, c] + j)) for c in (1, 3) for j in (0, 1))
        weights = sum(cycles("r128", 16 * (256 * ps + 64 * i + lanes)) for i in range(4))
        sb = np.where(d[:, 2] < 0, n_slots, d[:, 2])
        kind = "w32" if slot_bytes == 4 else "w64"
        stores = sum(cycles(kind, 4 * partial_off + slot_bytes * s) for s in (d[:, 0], sb))
        out.append((plane, weights, stores))
    return out


def headline_plan():
    """The plan of bench.py's headline: Slaney bank, sr 22 050, n_fft 2048, 128 mels (needs the built library)."""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from mlx_audio_primitives_amd import _extension as _x
    fb = _x.mel_filterbank_host(22050, 2048, 128)
    return _x.mel_plan_host(np.ascontiguousarray(fb, np.float32))


if __name__ == "__main__":
    import sys
    if "--mel-plan" in sys.argv:
        plan, desc = headline_plan()
        print(f"headline plan: {desc[12]} entries, {desc[7]} slots, {(desc[12] + 63) // 64} passes")
        for sb in (4, 8):
            for ps, (pl, wt, st) in enumerate(mel_plan_reads(plan, desc, slot_bytes=sb)):
                print(f"  slots of {sb} bytes, pass {ps}: plane reads {pl} (ideal 16)  weight reads {wt} (ideal 16)  "
                      f"partial stores {st} (ideal {sb})")
        sys.exit(0)
    lanes = np.arange(64)
    # exchange-1 of the 1024-point wave FFT: rows of 16 complex, padded row stride S (complex)
    for S in (16, 17, 18, 20):
        a, b = lanes & 3, lanes >> 2
        w = sum(cycles("w64", ((k1 * 4 + a) * S + b) * 8) for k1 in range(16))
        r = sum(cycles("r128", (lanes * S + 2 * i) * 8) for i in range(8)) if S % 2 == 0 else -1
        print(f"exch1 S={S}: write {w} (ideal 64)  read {r} (ideal 32)")
    # twiddle rows of the n_fft = 2048 run kernels: one row of S complex per lane, eight ds_read_b128 per lane
    for S in (16, 18, 20):
        r = sum(cycles("r128", (lanes * S + 2 * i) * 8) for i in range(8))
        print(f"tw1 rows S={S}: read {r} bank cycles (ideal 32) for 8 ds_read_b128 = 8 x 1024 bytes")
    # second table of the run kernels: 12 twiddles per lane (W_64^(a c) of its four radix-4 groups), six reads
    for S in (12, 14, 16, 18):
        r = sum(cycles("r128", (lanes * S + 2 * i) * 8) for i in range(6))
        print(f"tw2 rows S={S}: read {r} bank cycles (ideal 24) for 6 ds_read_b128 = 6 x 1024 bytes")
    # The old [16][64] table: 15 ds_read_b64 of consecutive lanes.  cycles() counts BANK passes only (one per
    # group of lanes without a conflict), not the issue rate of the instruction form: 30 conflict-free passes
    # here move 15 x 512 bytes, 256 bytes per pass, the rows above 32 passes of 256 bytes.  The compiler pairs
    # these reads into ds_read2st64_b64 / ds_read2_b64, which the guide's instruction table rates at 128
    # bytes per clock against 256 for ds_read_b128: that rate, not conflicts, is what the row layout buys
    # (measured: SQ_LDS_IDX_ACTIVE -54 per frame for the two tables, profiles/README.md "Round 5").
    r = sum(cycles("r64", (k * 64 + lanes) * 8) for k in range(1, 16))
    print(f"tw1 [16][64]: read {r} bank cycles (ideal 30) for 15 ds_read_b64 = 15 x 512 bytes; "
          f"at the paired forms' 128 B/clk: {15 * 512 // 128} clocks against {8 * 1024 // 256} for the rows")
