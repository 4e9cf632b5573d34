"""The definition of yin / yin_cmnd as NumPy code, shared by test_emu_yin.py, test_gpu_yin.py and test_yin_api.py
(not a test module, not product code).

cmnd64 is the definition itself (float64, direct sums); cmnd32 is the textbook float32 route (scipy.fft, cumsum)
whose distance from cmnd64 sets the tolerances; neither is the code under test.  `compare` applies the checks of
both test files: the curve within atol = max(8 max|cmnd32 - cmnd64|, 1e-5), f0 on the decisive frames within
rtol = max(8 max rel err of pick(cmnd32), 1e-5), the aperiodicity within atol, and returns the share of frames
that were not decisive."""

import math

import numpy as np
import scipy.fft as sf

SR = 22050
MARGIN = 0.002          # 20 x the largest float32 curve error seen on the test inputs
THRESHOLD = 0.1
# (frame_length, hop_length, fmin, fmax)
SHAPES = [(2048, 512, 65.0, 2093.0), (1024, 256, 100.0, 2000.0), (512, 128, 200.0, 2000.0),
          (1536, 384, 100.0, 2000.0), (400, 160, 200.0, 2000.0)]
# largest share of non-decisive frames per signal (full-length cases)
CAPS = {"vibrato": 0.05, "glide": 0.05, "loud": 0.05, "quiet": 0.05, "bursts": 0.15, "noise": 0.30}
NAMES = ["vibrato", "glide", "bursts", "noise", "loud", "quiet"]



def frames_of(y, fl, hop, center):
    if center:
        y = np.pad(y, (fl // 2, fl // 2))
    T = 1 + (len(y) - fl) // hop
    idx = np.arange(fl)[None, :] + hop * np.arange(T)[:, None]
    return y[idx]            # (T, fl)

def periods(sr, fmin, fmax, fl):
    W = fl // 2
    lo = max(int(math.floor(sr / fmax)), 1)
    hi = min(int(math.ceil(sr / fmin)), fl - W - 1)
    return lo, hi, W

def cmnd64(fr, lo, hi, W):
    fr = fr.astype(np.float64)
    T, fl = fr.shape
    d = np.zeros((T, hi + 2))
    for tau in range(hi + 2):
        df = fr[:, :W] - fr[:, tau:tau + W]
        d[:, tau] = (df * df).sum(1)
    cs = np.cumsum(d[:, 1:], axis=1)
    taus = np.arange(1, hi + 2)
    dp = np.ones_like(d)
    with np.errstate(all="ignore"):
        dp[:, 1:] = np.where(cs > 0, d[:, 1:] * taus / np.where(cs > 0, cs, 1), 1.0)
    return dp               # (T, hi+2), dp[:,0] = 1

def cmnd32(fr, lo, hi, W):
    fr = fr.astype(np.float32)
    T, fl = fr.shape
    A = sf.rfft(fr, axis=1)
    w = fr.copy(); w[:, W:] = 0
    Bf = sf.rfft(w, axis=1)
    r = sf.irfft(A * np.conj(Bf), n=fl, axis=1).astype(np.float32)
    sq = fr * fr
    c = np.concatenate([np.zeros((T, 1), np.float32), np.cumsum(sq, axis=1, dtype=np.float32)], axis=1)
    e = (c[:, W:W + hi + 2] - c[:, 0:hi + 2]).astype(np.float32)
    d = (e[:, :1] + e - np.float32(2) * r[:, :hi + 2]).astype(np.float32)
    d = np.maximum(d, 0)
    cs = np.cumsum(d[:, 1:], axis=1, dtype=np.float32)
    taus = np.arange(1, hi + 2, dtype=np.float32)
    dp = np.ones_like(d)
    dp[:, 1:] = np.where(cs > 0, d[:, 1:] * taus / np.where(cs > 0, cs, 1), 1.0)
    return dp

def pick(dp, lo, hi, thr, sr):
    T = dp.shape[0]
    f0 = np.zeros(T); tau_i = np.zeros(T, int); ap = np.zeros(T); fb = np.zeros(T, bool)
    for t in range(T):
        x = dp[t]
        cand = None
        for tau in range(lo, hi + 1):
            left = x[tau - 1] if tau > lo else np.inf
            right = x[tau + 1] if tau < hi else np.inf
            if x[tau] < thr and x[tau] < left and x[tau] <= right:
                cand = tau; break
        if cand is None:
            cand = lo + int(np.argmin(x[lo:hi + 1])); fb[t] = True
        sh = 0.0
        if lo < cand < hi:
            a = (x[cand - 1] + x[cand + 1] - 2 * x[cand]) / 2
            b = (x[cand + 1] - x[cand - 1]) / 2
            if abs(b) < abs(a):
                sh = -b / (2 * a)
        tau_i[t] = cand; f0[t] = sr / (cand + sh); ap[t] = x[cand]
    return f0, tau_i, ap, fb

def signals(sr, n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    out = {}
    # harmonic tone with vibrato + noise
    f = 220 * (1 + 0.03 * np.sin(2 * np.pi * 5 * t))
    ph = 2 * np.pi * np.cumsum(f) / sr
    out["vibrato"] = sum(np.sin(k * ph) / k for k in range(1, 6)) + 0.05 * rng.standard_normal(n)
    # glide 80 -> 800 Hz, exponential
    f = 80 * (10 ** (t / t[-1]))
    ph = 2 * np.pi * np.cumsum(f) / sr
    out["glide"] = sum(np.sin(k * ph) / k ** 1.5 for k in range(1, 4)) + 0.02 * rng.standard_normal(n)
    # tone bursts separated by noise (voiced / unvoiced)
    env = (np.sin(2 * np.pi * 1.5 * t) > 0).astype(float)
    out["bursts"] = env * np.sin(2 * np.pi * 330 * t) + 0.1 * rng.standard_normal(n)
    out["noise"] = rng.standard_normal(n)
    out["loud"] = 1000 * out["vibrato"]
    out["quiet"] = 1e-3 * out["vibrato"]
    return out


def decisive(d64, lo, hi, sr=SR, thr=THRESHOLD, m=MARGIN):
    """(mask, f0, lag, aperiodicity) of the float64 pick: the frames whose integer lag does not depend on
    errors of the curve below m."""
    picks = [pick(d64, lo, hi, th, sr) for th in (thr - m, thr, thr + m)]
    f64, t64, a64, fb = picks[1]
    dec = (picks[0][1] == t64) & (picks[2][1] == t64)
    for t in np.nonzero(fb)[0]:
        x = d64[t, lo:hi + 1].copy()
        i = t64[t] - lo
        x[max(i - 2, 0):i + 3] = np.inf
        if x.min() - a64[t] < m:
            dec[t] = False
    return dec, f64, t64, a64


class Case:
    """Reference results of one clip at one shape."""

    def __init__(self, y, fl, hop, fmin, fmax, center, sr=SR):
        self.lo, self.hi, W = periods(sr, fmin, fmax, fl)
        fr = frames_of(np.asarray(y, np.float32), fl, hop, center)
        lo, hi = self.lo, self.hi
        self.d64 = cmnd64(fr, lo, hi, W)
        d32 = cmnd32(fr, lo, hi, W)
        self.atol = max(8 * float(np.abs(d32 - self.d64)[:, lo:hi + 1].max()), 1e-5)
        self.dec, self.f0, self.lag, self.ap = decisive(self.d64, lo, hi, sr)
        f32 = pick(d32.astype(np.float64), lo, hi, THRESHOLD, sr)[0]
        rel = np.abs(f32 - self.f0) / self.f0
        self.rtol = max(8 * float(rel[self.dec].max()) if self.dec.any() else 0.0, 1e-5)

    def compare(self, curve, f0, aper, label=""):
        """curve (n_lags, T), f0 (T,), aper (T,) of the code under test; prints every figure, then asserts.
        Returns the share of frames left out as non-decisive."""
        ref = self.d64[:, self.lo:self.hi + 1].T
        assert curve.shape == ref.shape, (label, curve.shape, ref.shape)
        assert f0.shape == self.f0.shape and aper.shape == self.f0.shape, (label, f0.shape, self.f0.shape)
        assert np.isfinite(curve).all() and np.isfinite(f0).all() and np.isfinite(aper).all(), label
        cerr = float(np.abs(curve - ref).max())
        dec = self.dec
        rel = np.abs(f0 - self.f0) / self.f0
        ferr = float(rel[dec].max()) if dec.any() else 0.0
        aerr = float(np.abs(aper - self.ap)[dec].max()) if dec.any() else 0.0
        out = 1.0 - float(dec.mean())
        print(f"{label}: curve err {cerr:.3e} (atol {self.atol:.3e})  f0 rel err {ferr:.3e} (rtol {self.rtol:.3e})  "
              f"aper err {aerr:.3e}  non-decisive {out:.3f}")
        assert cerr <= self.atol, (label, "curve", cerr, self.atol)
        assert ferr <= self.rtol, (label, "f0", ferr, self.rtol)
        assert aerr <= self.atol, (label, "aperiodicity", aerr, self.atol)
        return out
