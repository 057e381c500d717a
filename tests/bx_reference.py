"""An exact reference for the expansion index's tests: plain numpy and
mpmath, no GPU.

For one dense label (below and above mixtures (w, mu, sigma), the bounds and
the family):

* score_exact(x): lpdf_below - lpdf_above as oracle/tpe_oracle.py defines
  gmm1_lpdf and lgmm1_lpdf (the dense LGMM1 branch ignores p_accept, as the
  reference does), evaluated in np.longdouble with a max-shifted
  log-sum-exp.  p_accept is the fp64 value oracle.tpe_oracle._p_accept
  returns: the library reproduces it bit for bit, so it belongs to the
  function's definition.
* interval_mass(a, b): the mass of [a, b] in draw space (x for GMM1, log x
  for LGMM1) under the truncated below mixture the sampler draws from, a
  bounded label renormalised by its accepted mass; mpmath's ncdf at 40
  digits.
* score_range(a, b): min and max of score_exact over [a, b] (draw space)
  from 33 evenly spaced points -- a lower estimate of the score's true
  oscillation over the interval.
"""
import numpy as np
from mpmath import mp, mpf

from oracle import tpe_oracle as O

LD = np.longdouble
EPS = LD(O.EPS)
_LOG_SQRT_2PI = LD(0.5) * np.log(LD(2) * LD(np.pi))   # (the fp64 pi, as the oracle's sqrt(2 pi))
MP_DPS = 40
# a component whose standardised distance from both ends of an interval
# exceeds this, on the same side, holds less than ncdf(-14) = 8e-45 of mass
# there: left out of interval sums (far below the 40 digits carried)
_Z_FAR = 14.0
# terms more than this many nats below the largest are left out of the
# mpmath sums: together below n e^-60 < 2e-22 of the sum for n <= 2^14 + 2
_MP_DROP = 60.0


class LabelRef(object):
    """The exact reference of one dense LabelPosterior."""

    def __init__(self, p):
        assert p.family in ('GMM1', 'LGMM1') and p.q is None
        self.p = p
        self.family = p.family
        self.low, self.high = p.low, p.high
        self.bounded = p.low is not None
        self.side = []
        for w, m, s in (p.below, p.above):
            w, m, s = (np.asarray(a, dtype=np.float64) for a in (w, m, s))
            pacc = O._p_accept(w, m, s, p.low, p.high) if (self.bounded and p.family == 'GMM1') else 1.0
            sl = np.maximum(s.astype(LD), EPS)
            with np.errstate(divide='ignore'):
                if p.family == 'GMM1':   # log(w / sqrt(2 pi sigma^2) / p_accept), sigma unclamped there
                    lc = np.log(w.astype(LD)) - np.log(s.astype(LD)) - _LOG_SQRT_2PI - np.log(LD(pacc))
                else:                    # log w - log(max(sigma, EPS) sqrt(2 pi)); - log x per candidate
                    lc = np.log(w.astype(LD)) - np.log(sl) - _LOG_SQRT_2PI
            self.side.append({'w': w, 'mu': m, 'sigma': s, 'sl': sl, 'lc': lc, 'pacc': float(pacc)})

    # -- draw space <-> value space ------------------------------------------
    def to_value(self, d):
        d = np.asarray(d, dtype=np.float64)
        return np.exp(d) if self.family == 'LGMM1' else d

    def to_draw(self, x):
        x = np.asarray(x, dtype=np.float64)
        if self.family == 'LGMM1':
            with np.errstate(divide='ignore', invalid='ignore'):
                return np.log(x)
        return x

    # -- exact log densities --------------------------------------------------
    def lpdf_exact(self, x, side, chunk=2048):
        """lpdf of the below (side 0) or above (side 1) mixture at value(s) x,
        np.longdouble."""
        x = np.atleast_1d(np.asarray(x, dtype=np.float64)).astype(LD)
        S = self.side[side]
        out = np.empty(x.shape, dtype=LD)
        for i in range(0, len(x), chunk):
            xs = x[i:i + chunk]
            with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
                if self.family == 'GMM1':
                    y, shift = xs, LD(0)
                else:
                    y = np.log(xs)
                    shift = -y
                z = (y[:, None] - S['mu'].astype(LD)[None, :]) / S['sl'][None, :]
                t = S['lc'][None, :] - LD(0.5) * z * z
                m = np.max(t, axis=1)
                ms = np.where(np.isfinite(m), m, LD(0))
                out[i:i + chunk] = np.log(np.sum(np.exp(t - ms[:, None]), axis=1)) + ms + shift
        return out

    def score_exact(self, x):
        with np.errstate(invalid='ignore'):
            return self.lpdf_exact(x, 0) - self.lpdf_exact(x, 1)

    def score_range(self, a, b):
        """(min, max) of score_exact over [a, b] in draw space, 33 evenly
        spaced points; a and b may be arrays (one interval per entry)."""
        a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
        t = np.linspace(0.0, 1.0, 33)
        d = a[:, None] + (b - a)[:, None] * t[None, :]
        s = self.score_exact(self.to_value(d.ravel())).reshape(d.shape)
        return np.min(s, axis=1), np.max(s, axis=1)

    # -- mpmath ---------------------------------------------------------------
    def lpdf_mp(self, x, side):
        """lpdf at one value x (a float) in mpmath, MP_DPS digits."""
        S = self.side[side]
        with mp.workdps(MP_DPS):
            xv = mpf(float(x))
            y = xv if self.family == 'GMM1' else mp.log(xv)
            # (which terms to leave out is decided in long double)
            yl = LD(float(x)) if self.family == 'GMM1' else np.log(LD(float(x)))
            zl = (yl - S['mu'].astype(LD)) / S['sl']
            tl = S['lc'] - LD(0.5) * zl * zl
            keep = np.where(tl >= np.max(tl) - _MP_DROP)[0]
            lcs, ms, sls = self._mp_consts(side)
            ts = []
            for k in keep:
                z = (y - ms[k]) / sls[k]
                ts.append(lcs[k] - z * z / 2)
            mx = max(ts)
            r = mp.log(mp.fsum(mp.exp(t - mx) for t in ts)) + mx
            return r if self.family == 'GMM1' else r - y

    def _mp_consts(self, side):
        """Per component, once: its log coefficient, mean and clamped sigma
        as mpf."""
        S = self.side[side]
        if 'mp' not in S:
            lcs, ms, sls = [], [], []
            with mp.workdps(MP_DPS):
                half_log_2pi = mp.log(2 * mpf(float(np.pi))) / 2
                log_pacc = mp.log(mpf(S['pacc']))
                for w, m, s in zip(S['w'], S['mu'], S['sigma']):
                    w, m, s = mpf(float(w)), mpf(float(m)), mpf(float(s))
                    sl = max(s, mpf(O.EPS))
                    lw = mp.log(w) if w > 0 else mp.ninf
                    if self.family == 'GMM1':
                        lcs.append(lw - mp.log(s) - half_log_2pi - log_pacc)
                    else:
                        lcs.append(lw - mp.log(sl) - half_log_2pi)
                    ms.append(m)
                    sls.append(sl)
            S['mp'] = (lcs, ms, sls)
        return S['mp']

    def score_mp(self, x):
        with mp.workdps(MP_DPS):
            return self.lpdf_mp(x, 0) - self.lpdf_mp(x, 1)

    def _cdf_mp(self, edges):
        """sum_k w_k Phi((e - mu_k) / sigma_k) at each sorted draw-space edge,
        up to a constant per component that cancels in differences: a
        component farther than _Z_FAR sigma from every edge on one side is
        left out (its Phi is the same 0 or 1, to 8e-45, at all of them)."""
        S = self.side[0]
        e = np.asarray(edges, dtype=np.float64)
        out = [mpf(0)] * len(e)
        with mp.workdps(MP_DPS):
            for w, m, s in zip(S['w'], S['mu'], S['sigma']):
                if not (w > 0.0):
                    continue
                if (e[0] - m) / s > _Z_FAR or (e[-1] - m) / s < -_Z_FAR:
                    continue
                wm, mm, sm = mpf(float(w)), mpf(float(m)), mpf(float(s))
                for i, ei in enumerate(e):
                    out[i] += wm * mp.ncdf((mpf(float(ei)) - mm) / sm)
        return out

    def _accepted_mp(self):
        if getattr(self, '_acc', None) is None:
            S = self.side[0]
            with mp.workdps(MP_DPS):
                if self.bounded:
                    lo, hi = mpf(float(self.low)), mpf(float(self.high))
                    self._acc = mp.fsum(mpf(float(w)) * (mp.ncdf((hi - mpf(float(m))) / mpf(float(s))) -
                                                         mp.ncdf((lo - mpf(float(m))) / mpf(float(s))))
                                        for w, m, s in zip(S['w'], S['mu'], S['sigma']) if w > 0.0)
                else:
                    self._acc = mp.fsum(mpf(float(w)) for w in S['w'])
        return self._acc

    def interval_masses(self, edges):
        """Exact masses of the consecutive draw-space intervals [e_i, e_i+1]
        of the sorted array `edges` under the truncated below mixture
        (fp64 array of len(edges) - 1)."""
        e = np.asarray(edges, dtype=np.float64)
        if self.bounded:
            e = np.clip(e, float(self.low), float(self.high))
        c = self._cdf_mp(e)
        with mp.workdps(MP_DPS):
            acc = self._accepted_mp()
            return np.array([float((c[i + 1] - c[i]) / acc) for i in range(len(e) - 1)])

    def interval_mass(self, a, b):
        return float(self.interval_masses([a, b])[0])
