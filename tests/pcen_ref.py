"""The definition of pcen (mlx-audio-primitives_amd/pcen.py, include/audioprims.h) in float64 on scipy.signal.lfilter
and scipy.ndimage.maximum_filter1d, the cases test_emu_pcen.py and test_gpu_pcen.py share, and the error bound.

  max_filter(S, size)       SciPy's filter where it implements the reflection (hpss_ref.scipy_reflects), the explicit
                            mirror of onset_ref.max_filter beyond; self_check() pins the two against each other
  pcen(S, ...)              (out, zf, Msm) in float64
  bound(...)                |out32 - out64| and |zf32 - zf64| allowed, derived below
  textbook32 / yardstick32  float32 NumPy evaluations that are NOT the definition: the subtraction that cancels, and
                            SciPy's float32 lfilter with a float32 log1p / expm1 chain (information only)

The bound (u = 2^-24, the unit roundoff of float32; every count is a number of u, first order, times 1 + 2^-10 for
the second-order terms, which is ample while the total stays below 2^-11).

Smoother.  For S >= 0 and zi >= 0 every term of Msm is non-negative, so relative errors of the terms bound the
relative error of the sum.  Counting the roundings on the longest path of the kernel's scan (kernels_pcen.h):
  b rounded to float32, b R                                                   2
  six Hillis-Steele steps, each: the table value a^(2^j) rounded from its
    float64 power, the product, the sum                                       6 x 3 = 18      -> 20 inside a tile
  the incoming state: its own error k_in (1 for the default zi = float32(1 - b), 0 for a given float32 zi, K + 2 for
    the zf of an earlier piece), the table value a^lane or a^(lane+1), the product: k_in + 2; then one sum:
  K_0 = max(20, k_in + 2) + 1,  K_n = max(20, K_(n-1) + 2) + 1 in the n-th tile of 64 frames: 21 + 3 n for k_in <= 18.
  |Msm32 - Msm64| <= K_n u Msm64;  zf = a Msm[T-1] with a rounded and one product: K_last + 2.
A fused multiply-add only removes roundings from this count.

Chain.  The kernel's transcendentals are v_log_f32 (log2), v_exp_f32 (2^x) and v_rcp_f32; the emulator build calls
log2f, exp2f and a division in their place.  c u per such instruction with c = 4, i.e. 2 ulp each.  (AMD's ISA
guide gives 1 ulp for all three; it is not part of this repository, so twice that is assumed and stated here.
glibc's functions are within 1 ulp, a division within half.)  A product or a sum adds 1, a rounded constant or parameter 1.
  A = eps + Msm: eps rounded (1) against K, one sum                            K + 1   relative
  log2 A: absolute error ((K + 1) / ln 2) + c |log2 A|
  gain log2 A: gain rounded, one product; 2^(.) turns an absolute error d of its argument into ln 2 d, relative:
  smooth = 2^(-gain log2 A): relative  e_s = gain (K + 1) + gain |ln A| (c + 2) + c   (the |ln(eps + M)| conditioning)
  x = S smooth: e_x = e_s + 1;   gain = 0: smooth = 1 and x = S exactly, e_x = 0
  log1p(u) = ln(w) u / (w - 1), w = fl(1 + u) (appc_log1p).  With w = (1 + u)(1 + d) the quotient ln(w) / (w - 1) is
              taken at the increment ln(w) really saw; ln(1 + x) / x has a relative condition below 1, so d costs 1.
              log2 (c), ln 2 rounded and its product (2), w - 1 (exact in [1/2, 2], else 1), rcp (c), two products (2):
              LOG1P = 2 c + 6, on top of the relative error of u (the condition of log1p is below 1 as well);
              w = 1 returns u, off by u / 2 < 1
  expm1(q) = (e - 1) q / ln(e), e = fl(2^(q log2 e)) (appc_expm1).  An error d of e moves the result by
              (kappa - 1) / q d relative (expm1(x) / x has the relative condition kappa - 1), kappa = q / (1 - e^-q),
              and (kappa - 1) / q <= 1.  d = c (2^x) + 2 q (log2 e rounded, its product: 2 q' absolute in the exponent):
              c + 2 (kappa - 1); e - 1 (1); log2 (c), ln 2 and its product (2); rcp (c); two products (2):
              EXPM1 = 3 c + 2 kappa + 3, on top of kappa times the relative error of q; e = 1 returns q, off by q / 2 < 1
  power = 0:  log1p(x):  e_out = e_x + LOG1P
  bias = 0:   2^(power log2 x): absolute error of the exponent, in natural units, power (e_x + c |ln x|) + 2 power |ln x|
              (power rounded, one product), e_out = that + c;  x = 0 gives exactly 0
  general:    x / bias as x times the rounded reciprocal: e_x + 2;  log1p: + LOG1P;  power rounded, product:
              e_q = e_x + 4 + LOG1P;  e_w = kappa e_q + EXPM1  (kappa -> 1 for q -> 0, -> q for large q: the
              max(1, power ln(1 + u)) factor, exactly);  bias^power rounded from float64, one product:  e_out = e_w + 2
"""

import numpy as np
from scipy.ndimage import maximum_filter1d
from scipy.signal import lfilter, lfilter_zi

import hpss_ref
import onset_ref

U = 2.0 ** -24
C_ULP = 4.0                    # u per v_log_f32 / v_exp_f32 / v_rcp_f32: 2 ulp (assumed, see above)
SECOND_ORDER = 1.0 + 2.0 ** -10
TILE = 64


def max_filter(S, size):
    S = np.asarray(S)
    if size == 1:
        return S
    if hpss_ref.scipy_reflects(size, S.shape[-2]):
        return maximum_filter1d(S, size, axis=-2, mode="reflect")
    return onset_ref.max_filter(S, size)


def b_of(time_constant=0.400, sr=22050, hop_length=512):
    t = time_constant * sr / hop_length
    return (np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


B_DEFAULT = float(b_of())


def pcen(S, *, b=B_DEFAULT, gain=0.98, bias=2.0, power=0.5, eps=1e-6, max_size=1, ref=None, zi=None):
    """(out, zf (..., M, 1), Msm) in float64 of S (..., M, T)."""
    S = np.asarray(S, np.float64)
    R = np.asarray(ref, np.float64) if ref is not None else max_filter(S, max_size)
    z = np.full(S.shape[:-1] + (1,), 1.0 - b) if zi is None else \
        np.broadcast_to(np.asarray(zi, np.float64), S.shape[:-1] + (1,)).copy()
    Msm, zf = lfilter([b], [1.0, b - 1.0], R, zi=z, axis=-1)
    with np.errstate(divide="ignore"):
        smooth = np.exp(-gain * (np.log(eps) + np.log1p(Msm / eps)))
        if power == 0:
            out = np.log1p(S * smooth)
        elif bias == 0:
            out = np.exp(power * (np.log(S) + np.log(smooth)))
        else:
            out = bias ** power * np.expm1(power * np.log1p(S * smooth / bias))
    return out, zf, Msm


def smoother_K(T, k_in):
    """K per frame (T,) and the K of zf."""
    K, k = np.empty(T), float(k_in)
    for n in range((T + TILE - 1) // TILE):
        k = max(20.0, k + 2.0) + 1.0
        K[n * TILE:(n + 1) * TILE] = k
    return K, K[-1] + 2.0


def bound(S, out, zf, Msm, *, gain=0.98, bias=2.0, power=0.5, eps=1e-6, k_in=1.0, **_):
    """(bound on |out32 - out|, bound on |zf32 - zf|, K of zf) for the float64 results of pcen() on the float32 S."""
    S = np.asarray(S, np.float64)
    K, k_zf = smoother_K(S.shape[-1], k_in)
    c = C_ULP
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.abs(np.log(eps + Msm))
        if gain == 0:
            e_x = np.zeros_like(S)
            x = S
        else:
            e_x = gain * (K + 1.0) + gain * L * (c + 2.0) + c + 1.0
            x = S * np.exp(-gain * np.log(eps + Msm))
        log1p_cost = 2.0 * c + 6.0
        if power == 0:
            e_out = e_x + log1p_cost
        elif bias == 0:
            lx = np.abs(np.log(x))
            e_out = np.where(x > 0, power * (e_x + c * lx) + 2.0 * power * lx + c, 0.0)
        else:
            q = power * np.log1p(x / bias)
            kappa = np.where(q > 0, q / -np.expm1(-q), 1.0)
            e_out = kappa * (e_x + 4.0 + log1p_cost) + (3.0 * c + 2.0 * kappa + 3.0) + 2.0
    return e_out * U * SECOND_ORDER * np.abs(out), k_zf * U * SECOND_ORDER * np.abs(zf), k_zf


def check(got, got_zf, S, params, what, zi=None, ref=None, k_in=None):
    """Asserts the bounds against the float64 definition on the float32 inputs; exact zeros where the definition is 0.
    Returns (worst error / bound of out, of zf, K of zf for a following piece)."""
    want, zf, Msm = pcen(S, ref=ref, zi=zi, **params)
    if k_in is None:
        k_in = 1.0 if zi is None else 0.0
    b_out, b_zf, k_zf = bound(S, want, zf, Msm, k_in=k_in, **params)
    err = np.abs(got.astype(np.float64) - want)
    r = float(np.max(err[b_out > 0] / b_out[b_out > 0])) if np.any(b_out > 0) else 0.0
    rz = 0.0
    if got_zf is not None:
        ez = np.abs(got_zf.astype(np.float64).reshape(zf.shape) - zf)
        rz = float(np.max(ez[b_zf > 0] / b_zf[b_zf > 0])) if np.any(b_zf > 0) else 0.0
        assert np.all(ez <= b_zf), (what, "zf", rz)
    assert np.all(err <= b_out), (what, r)
    assert np.all(got[want == 0.0] == 0.0), what
    return r, rz, k_zf


# ---- evaluations that are not the definition -------------------------------------------------------------------------
def textbook32(S, *, b=B_DEFAULT, gain=0.98, bias=2.0, power=0.5, eps=1e-6, **_):
    """(S / (eps + M)^gain + bias)^power - bias^power in float32 on the float64 smoother: the subtraction cancels."""
    S = np.asarray(S, np.float32)
    Msm = pcen(S, b=b, gain=gain, bias=bias, power=power, eps=eps)[2].astype(np.float32)
    f = np.float32
    return (S / (f(eps) + Msm) ** f(gain) + f(bias)) ** f(power) - f(bias) ** f(power)


def yardstick32(S, *, b=B_DEFAULT, gain=0.98, bias=2.0, power=0.5, eps=1e-6, **_):
    """SciPy's float32 lfilter (a plain recursion) and the log1p / expm1 chain in NumPy float32."""
    S = np.asarray(S, np.float32)
    f = np.float32
    z = np.full(S.shape[:-1] + (1,), f(1.0 - b), np.float32)
    Msm, _ = lfilter(np.array([b], np.float32), np.array([1.0, b - 1.0], np.float32), S, zi=z, axis=-1)
    Msm = Msm.astype(np.float32)
    smooth = np.exp(-f(gain) * np.log(f(eps) + Msm))
    return (f(bias ** power) * np.expm1(f(power) * np.log1p(S * smooth / f(bias)))).astype(np.float32), Msm


def self_check():
    """The default state is SciPy's steady state; the maximum filter's mirror equals SciPy's wherever SciPy implements
    it; the smoother by hand; the reference is exactly chunk-invariant in its state and to rounding in its values.
    Returns {name: worst error / bound} of the two float32 evaluations above (not asserted to pass)."""
    for b in (1e-3, B_DEFAULT, 0.5, 0.9, 1.0):
        np.testing.assert_allclose(lfilter_zi([b], [1.0, b - 1.0]), [1.0 - b], rtol=1e-12, atol=1e-15)
    rng = np.random.default_rng(5)
    n = 0
    for M in (1, 2, 3, 5, 9, 65):
        X = rng.random((2, M, 3))
        for size in (2, 3, 4, 5, min(2 * M + 1, 255)):
            if hpss_ref.scipy_reflects(size, M):
                n += 1
                assert np.array_equal(onset_ref.max_filter(X, size), maximum_filter1d(X, size, axis=-2, mode="reflect")), (M, size)
    assert n >= 25
    out, zf, Msm = pcen(np.array([[1.0, 0.0, 4.0]]), b=0.5, zi=np.array([[0.25]]), gain=0.0, power=0.0)
    assert list(Msm[0]) == [0.75, 0.375, 2.1875] and zf[0, 0] == 1.09375 and out[0, 1] == 0.0
    S = cases()["wide"][(3, 3, 129)]
    whole, zf_w, _ = pcen(S)
    for k in (1, 64, 128):
        head, zf_h, _ = pcen(S[..., :k])
        tail, zf_t, _ = pcen(S[..., k:], zi=zf_h)
        np.testing.assert_allclose(np.concatenate([head, tail], -1), whole, rtol=1e-13)
        np.testing.assert_allclose(zf_t, zf_w, rtol=1e-13)
    ratios = {}
    for name, b in (("b=default", B_DEFAULT), ("b=1e-3", 1e-3)):
        S = cases()["wide"][(1, 5, 431)]
        want, zf, Msm = pcen(S, b=b)
        bo, _, _ = bound(S, want, zf, Msm)
        got, M32 = yardstick32(S, b=b)
        K, _ = smoother_K(S.shape[-1], 1.0)
        ratios[f"float32 lfilter + chain, {name}"] = float(np.max(np.abs(got - want) / bo))
        ratios[f"float32 lfilter smoother alone / (K u), {name}"] = float(np.max(np.abs(M32 - Msm) / (K * U * Msm)))
    S = cases()["quiet"][(2, 3, 130)]
    want, zf, Msm = pcen(S)
    bo, _, _ = bound(S, want, zf, Msm)
    ratios["textbook subtraction, quiet input"] = float(np.max(np.abs(textbook32(S) - want) / bo))
    ratios["textbook subtraction, quiet input, relative error"] = float(np.max(np.abs(textbook32(S) - want) / want))
    return ratios


# ---- the cases test_emu_pcen.py and test_gpu_pcen.py share: computed once, never modified ------------------------------
# T in {1, 2, 63, 64, 65, 128, 129, 431} and one row of 4097 (64 carries); M in {1, 2, 3, 5, 65}; B in {1, 3}
SHAPES = [(1, 1, 1), (3, 2, 2), (1, 3, 63), (3, 5, 64), (1, 65, 65), (1, 2, 128), (3, 3, 129), (1, 5, 431), (1, 1, 4097)]
SMALL = [s for s in SHAPES if s[0] * s[1] * s[2] <= 1200]
QUIET_SHAPE = (2, 3, 130)
CHUNK_SHAPE = (3, 3, 129)

# every parameter set as keywords of pcen(); b = 0 needs the per-row zi of zi_for()
PARAMS = {
    "defaults": dict(),
    "b=1e-3": dict(b=1e-3),
    "b=0.5": dict(b=0.5),
    "b=1": dict(b=1.0),
    "b=0": dict(b=0.0),
    "power=0": dict(power=0.0),
    "bias=0": dict(bias=0.0),
    "gain=0": dict(gain=0.0),
    "power=2": dict(power=2.0),
    "power=0,bias=0": dict(power=0.0, bias=0.0),
    "speech": dict(gain=0.8, bias=10.0, power=0.25, b=0.025, eps=1e-12),
}
_cache = {}


def params(name):
    return dict(dict(b=B_DEFAULT, gain=0.98, bias=2.0, power=0.5, eps=1e-6), **PARAMS[name])


def max_sizes(M):
    return sorted({1, 2, 3, 4, min(2 * M + 1, 255)})


def cases():
    """{"wide": {shape: S}, "quiet": {...}, "zeros": {...}}, float32, read-only.  wide: log-uniform in [1e-8, 1e9]
    (a mel spectrogram times 2^31 lies inside); quiet: log-uniform in [1e-8, 1e-3]; zeros: wide with a third of the
    values, one whole row and one whole leading tile exactly 0."""
    if not _cache:
        wide, quiet, zeros = {}, {}, {}
        for shape in SHAPES + [QUIET_SHAPE]:
            rng = np.random.default_rng(100 + sum(shape))
            wide[shape] = (10.0 ** rng.uniform(-8.0, 9.0, shape)).astype(np.float32)
            quiet[shape] = (10.0 ** rng.uniform(-8.0, -3.0, shape)).astype(np.float32)
            z = wide[shape].copy()
            z[rng.random(shape) < 1 / 3] = 0.0
            z[0, 0, :] = 0.0
            z[..., :64] *= (np.arange(shape[1]) % 2)[:, None]
            zeros[shape] = z
        for d in (wide, quiet, zeros):
            for v in d.values():
                v.setflags(write=False)
        _cache.update(wide=wide, quiet=quiet, zeros=zeros)
    return _cache


def zi_for(shape):
    """A float32 state that differs per row, (B, M, 1), between 1e-3 and 1e3."""
    rng = np.random.default_rng(7 + sum(shape))
    return (10.0 ** rng.uniform(-3.0, 3.0, shape[:2] + (1,))).astype(np.float32)
