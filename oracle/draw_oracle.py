"""Pointwise reference of the sampler's draw contract (test infrastructure,
imported by the tests only).

The engine draws candidate g of (seed, label stream, round) from two words of
one Philox4x32-10 call (counter (g >> 1, 0, stream, round), key = seed; words
x, y for even g, z, w for odd g; a categorical label: counter (g, 0, stream,
round), word x).  The first word picks the component through the integer
thresholds thr = ceil(cdf 2^32) of the folded mixture, the second one is the
uniform of the component's inverse-CDF draw (tpe_device.h: samp_trunc,
samp_fold_block, icdf_draw).  Three restatements of that contract live here:

* `philox4x32_10` / `draw_words`: the words, vectorised over numpy arrays;
* `fold` / `draw_fp64`: the fold, the pick and the draw in numpy fp64, in the
  device's operation order (the "port");
* `draw_exact`: the mathematical value of the same draw in mpmath -- the
  arbiter between the port and a kernel.
"""
import math

import numpy as np

M32 = 0xFFFFFFFF
_U = np.uint64


# ------------------------------------------------------------------ Philox ----
def philox4x32_10(counter, key):
    """Philox4x32-10 over arrays: counter = (c0, c1, c2, c3), key = (k0, k1),
    each a scalar or an array of 32-bit values (broadcast together); returns
    the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=_U) & _U(M32) for v in counter]
    k0, k1 = (np.asarray(v, dtype=_U) & _U(M32) for v in key)
    c = list(np.broadcast_arrays(*c))
    m0, m1 = _U(0xD2511F53), _U(0xCD9E8D57)
    s32, m32 = _U(32), _U(M32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]      # (32 x 32 bits: no overflow in 64)
        c = [((p1 >> s32) ^ c[1] ^ k0) & m32, p1 & m32, ((p0 >> s32) ^ c[3] ^ k1) & m32, p0 & m32]
        k0 = (k0 + _U(0x9E3779B9)) & m32
        k1 = (k1 + _U(0xBB67AE85)) & m32
    return c


def draw_words(seed, stream, round, g, categorical=False):
    """(wp, wu): the pick word and the uniform word of candidate(s) g (a
    categorical draw uses wp only; its wu is the call's second word).  g,
    stream and round broadcast together."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g, stream, round = np.broadcast_arrays(*(np.asarray(v, dtype=_U) & _U(M32) for v in (g, stream, round)))
    key = (seed & M32, seed >> 32)
    if categorical:
        r = philox4x32_10((g, 0, stream, round), key)
        return r[0], r[1]
    r = philox4x32_10((g >> _U(1), 0, stream, round), key)
    odd = (g & _U(1)) != 0
    return np.where(odd, r[2], r[0]), np.where(odd, r[3], r[1])


# -------------------------------------------------------------------- fold ----
def _ncdf(x):
    """Phi(x) = erfc(-x / sqrt 2) / 2 (the device's expression)."""
    return 0.5 * math.erfc(-x * 0.70710678118654752440)


class Fold(object):
    """A folded below mixture: per component mu, sigma, ssg (-sigma when
    mirrored), p0, q0, m, cdf and the integer thresholds thr (Python ints in
    an object-free uint64 array; thr[K - 1] = 2^32), plus the label's
    attributes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def K(self):
        return len(self.thr)

    def tlo(self, k):
        k = np.asarray(k)
        return np.where(k > 0, self.thr[np.maximum(k - 1, 0)], _U(0)).astype(_U)

    def width(self, k):
        return self.thr[np.asarray(k)] - self.tlo(k)


def fold(w, mu=None, sigma=None, low=None, high=None, log=False, q=None):
    """samp_trunc + samp_fold_block in fp64, in their operation order.  mu =
    None: a categorical label (w = p).  low / high bound the draw space (the
    log space of an LGMM1 label); only a label with both bounds is
    truncated."""
    w = np.asarray(w, dtype=np.float64)
    K = len(w)
    cat = mu is None
    mu = np.zeros(K) if cat else np.asarray(mu, dtype=np.float64)
    sigma = np.zeros(K) if cat else np.asarray(sigma, dtype=np.float64)
    bounded = (not cat) and low is not None and high is not None
    ssg, p0, q0, m = sigma.copy(), np.zeros(K), np.zeros(K), np.ones(K)
    flip = np.zeros(K, dtype=bool)
    if bounded:
        for k in range(K):
            s = float(sigma[k])
            if not (s > 0.0 and s < math.inf):
                ssg[k] = 0.0
                m[k] = 1.0 if (low <= mu[k] < high) else 0.0
                continue
            a, b = (low - float(mu[k])) / s, (high - float(mu[k])) / s
            flip[k] = a >= 0.0
            a2, b2 = (-b, -a) if flip[k] else (a, b)
            ssg[k] = -s if flip[k] else s
            p0[k] = _ncdf(a2)
            q0[k] = _ncdf(-b2)
            mk = _ncdf(b2) - p0[k] if b2 <= 0.0 else (1.0 - p0[k]) - q0[k]
            m[k] = mk if mk > 0.0 else 0.0
    Z = 0.0
    for k in range(K):
        Z += float(w[k]) * float(m[k])
    if not Z > 0.0:
        raise ValueError('the bounds hold none of the mixture\'s mass')
    cdf = np.empty(K)
    run = 0.0
    for k in range(K):
        run += float(w[k]) * float(m[k])
        cdf[k] = 1.0 if k == K - 1 else run / Z
    thr = np.array([int(math.ceil(c * 4294967296.0)) for c in cdf], dtype=_U)
    return Fold(w=w, mu=mu, sigma=sigma, ssg=ssg, p0=p0, q0=q0, m=m, cdf=cdf, thr=thr, Z=Z, flip=flip,
                low=low, high=high, bounded=bounded, log=bool(log), q=q, categorical=cat)


# ----------------------------------------------------------- the fp64 draw ----
def _horner(c, r):
    acc = np.full_like(r, c[0])
    for v in c[1:]:
        acc = acc * r + v
    return acc


_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4,
      4.5921953931549871457e+4, 1.3731693765509461125e+4, 1.9715909503065514427e+3,
      1.3314166789178437745e+2, 3.3871328727963666080e0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4,
      2.1213794301586595867e+4, 5.3941960214247511077e+3, 6.8718700749205790830e+2,
      4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1,
      1.27045825245236838258e0, 3.64784832476320460504e0, 5.76949722146069140550e0,
      4.63033784615654529590e0, 1.42343711074968357734e0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2,
      1.48103976427480074590e-1, 6.89767334985100004550e-1, 1.67638483018380384940e0,
      2.05319162663775882187e0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3,
      2.65321895265761230930e-2, 2.96560571828504891230e-1, 1.78482653991729133580e0,
      5.46378491116411436990e0, 6.65790464350110377720e0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5,
      7.86869131145613259100e-4, 1.48753612908506148525e-2, 1.36929880922735805310e-1,
      5.99832206555887937690e-1, 1.0)


def ndtri_lower(t):
    """Phi^-1(t) for t in (0, 1/2]: Wichura's AS241 (PPND16), the published
    coefficients, three regions."""
    t = np.asarray(t, dtype=np.float64)
    out = np.empty_like(t)
    qq = t - 0.5
    cen = qq >= -0.425
    r = 0.180625 - qq[cen] * qq[cen]
    out[cen] = qq[cen] * _horner(_A, r) / _horner(_B, r)
    with np.errstate(divide='ignore', invalid='ignore'):
        rr = np.sqrt(-np.log(t))
    mid = ~cen & (rr <= 5.0)
    r = rr[mid] - 1.6
    out[mid] = -(_horner(_C, r) / _horner(_D, r))
    far = ~cen & ~mid
    r = rr[far] - 5.0
    out[far] = -(_horner(_E, r) / _horner(_F, r))
    return out


def pick(f, wp):
    """The first k with thr[k] > wp."""
    return np.searchsorted(f.thr, np.asarray(wp, dtype=_U), side='right').astype(np.int64)


def value_of(f, x):
    """The label's value of a draw-space x: exp for LGMM1, then rint(x / q) q."""
    v = np.exp(x) if f.log else x
    if f.q is not None:
        v = np.rint(v / f.q) * f.q
    return v


def draw_fp64(f, wp, wu):
    """The pick and icdf_draw in fp64: (k, z, x, value).  z is the standard
    normal deviate in the component's own frame (x = mu + sigma z, a mirrored
    component's sign undone), x the draw-space value after the clamp of a
    bounded label, value the label's (exp, quantization).  Categorical: (k,
    None, None, k)."""
    wp = np.asarray(wp, dtype=_U)
    wu = np.asarray(wu, dtype=_U)
    k = pick(f, wp)
    if f.categorical:
        return k, None, None, k
    tlo = f.tlo(k)
    n = f.thr[k] - tlo
    iw = 1.0 / n.astype(np.float64)
    pos = (wp - tlo).astype(np.float64)
    r = (pos + 0.5) * iw
    rb = ((n - _U(1) - (wp - tlo)).astype(np.float64) + 0.5) * iw
    v = (wu.astype(np.float64) + r) * 2.0 ** -32
    vb = ((_U(M32) - wu).astype(np.float64) + rb) * 2.0 ** -32
    m = f.m[k]
    p = m * v + f.p0[k]
    qq = m * vb + f.q0[k]
    lower = p <= 0.5
    zf = np.where(lower, ndtri_lower(np.where(lower, p, 0.25)), -ndtri_lower(np.where(lower, 0.25, qq)))
    x = f.ssg[k] * zf + f.mu[k]
    if f.bounded:
        x = np.where(x < f.low, f.low, x)
        x = np.where(x >= f.high, np.nextafter(f.high, -np.inf), x)
    x = np.where(m > 0.0, x, np.nan)
    z = np.where(f.flip[k], -zf, zf)
    return k, z, x, value_of(f, x)


def excluded(f, wp, wu, x=None):
    """The draws a device comparison may leave out: wp within 1 of a
    threshold (the device's erfc may move a threshold by one), wu at an end
    of its range, and -- quantized labels -- a value within 1e-9 of a rounding
    boundary of x / q."""
    wp = np.asarray(wp, dtype=np.int64)
    thr = f.thr[:-1].astype(np.int64)
    out = np.zeros(wp.shape, dtype=bool)
    if len(thr):
        i = np.clip(np.searchsorted(thr, wp), 0, len(thr) - 1)
        for j in (np.maximum(i - 1, 0), i):
            out |= np.abs(wp - thr[j]) <= 1
    if f.categorical:
        return out
    wu = np.asarray(wu, dtype=np.int64)
    out |= (wu == 0) | (wu == M32)
    if f.q is not None and x is not None:
        out |= near_rounding(f, x)
    return out


def near_rounding(f, x):
    """Quantized labels: x / q (after the exp of an LGMM1 label) within 1e-9
    of a half-integer, where rint may go either way."""
    t = (np.exp(x) if f.log else np.asarray(x, dtype=np.float64)) / f.q
    return np.abs(np.abs(t - np.floor(t)) - 0.5) <= 1e-9


# -------------------------------------------------------------- exact draw ----
DPS = 140


def _mp():
    import mpmath
    return mpmath


def _ncdf_mp(mp, z):
    return mp.erfc(-z / mp.sqrt(2)) / 2


def ndtri_exact(p, upper=False):
    """Phi^-1(p) (upper: Phi^-1(1 - p)) for an mpf p in (0, 1/2] by Newton's
    iteration on Phi(z) = p from scipy's fp64 quantile."""
    mp = _mp()
    from scipy.special import ndtri
    pf = float(p)
    dps = mp.mp.dps
    if pf > 1e-300:
        # scipy's quantile is good to ~1e-15; Newton squares the error
        # (times |z| / 2), so three steps at rising precision reach ~1e-100
        # -- the last step's size (the error before it, ~1e-52) is checked
        z = mp.mpf(float(ndtri(pf)))
        for step_dps in (40, 80, dps):
            with mp.workdps(min(step_dps, dps)):
                d = (_ncdf_mp(mp, z) - p) * mp.sqrt(2 * mp.pi) * mp.exp(z * z / 2)
                z = z - d
        if not abs(d) < mp.mpf(10) ** -45:
            raise ArithmeticError('Newton iteration did not converge (last step %s)' % mp.nstr(d, 5))
    else:
        z = -mp.sqrt(-2 * mp.log(p))
        tol = mp.mpf(10) ** (-(dps - 15))
        for _ in range(200):
            d = (_ncdf_mp(mp, z) - p) * mp.sqrt(2 * mp.pi) * mp.exp(z * z / 2)
            z -= d
            if abs(d) < tol:
                break
        else:
            raise ArithmeticError('no convergence')
    return -z if upper else z


def exact_masses(f):
    """mpf (Phi(a_k), Phi(b_k)) per component of a bounded label, else (0,
    1); a, b from the fp64 inputs, exactly."""
    mp = _mp()
    out = []
    for k in range(f.K):
        if not f.bounded:
            out.append((mp.mpf(0), mp.mpf(1)))
            continue
        mu, s = mp.mpf(float(f.mu[k])), mp.mpf(float(f.sigma[k]))
        out.append((_ncdf_mp(mp, (mp.mpf(f.low) - mu) / s), _ncdf_mp(mp, (mp.mpf(f.high) - mu) / s)))
    return out


def draw_exact(f, k, wp, wu):
    """The mathematical draw of component k from the words, thresholds from
    `f`: arrays (z, x) of fp64 roundings of the mpmath values, z in the
    component's own frame and x in the draw space (before exp and
    quantization).  `exact_value` applies those."""
    mp = _mp()
    k = np.atleast_1d(np.asarray(k))
    wp = np.atleast_1d(np.asarray(wp, dtype=_U))
    wu = np.atleast_1d(np.asarray(wu, dtype=_U))
    zs, xs = np.empty(len(k)), np.empty(len(k))
    with mp.workdps(DPS):
        masses = {}
        two32 = mp.mpf(2) ** 32
        sq2 = mp.sqrt(2)
        for i in range(len(k)):
            kk = int(k[i])
            tlo = int(f.thr[kk - 1]) if kk else 0
            thi = int(f.thr[kk])
            v = (int(wu[i]) + (mp.mpf(int(wp[i]) - tlo) + mp.mpf(1) / 2) / (thi - tlo)) / two32
            mu, s = mp.mpf(float(f.mu[kk])), mp.mpf(float(f.sigma[kk]))
            if f.bounded:
                if kk not in masses:
                    a, b = (mp.mpf(f.low) - mu) / s, (mp.mpf(f.high) - mu) / s
                    # (lower and upper masses outside [a, b): each small where it matters)
                    masses[kk] = (mp.erfc(-a / sq2) / 2, mp.erfc(b / sq2) / 2, a >= 0)
                Pa, Qb, mirrored = masses[kk]
                mass = 1 - Pa - Qb
                if mirrored:
                    v = 1 - v
                p, qq = Pa + mass * v, Qb + mass * (1 - v)
            else:
                p, qq = v, 1 - v
            z = ndtri_exact(p) if p <= qq else ndtri_exact(qq, upper=True)
            zs[i] = float(z)
            xs[i] = float(mu + s * z)
    return zs, xs


def exact_value(f, x):
    return value_of(f, np.asarray(x, dtype=np.float64))
