"""Joint TPE with quantized dimensions: the definition in numpy fp64 (test
infrastructure, imported by the tests only; the dense definition is
tests/joint_reference.py, which this builds beside).

A dimension d of a joint group is dense or quantized with step q_d > 0.  The
mixtures (W_k, mu_kd, s_kd), the masses m_kd, A and the component pick are
the dense group's.  A quantized dimension's label value x_d has the interval

    ub = x + q/2, lb = x - q/2
    linear kinds: clipped to [low, high] when the label has both bounds
    log kinds:    clipped to [exp(low), exp(high)] when bounded, lb = max(0, lb),
                  ub = log(max(ub, EPS)), lb = log(max(lb, EPS))

in the working space, and its factor in component k is the mass

    g_kd(x_d) = Phi((ub - mu_kd)/s_kd) - Phi((lb - mu_kd)/s_kd),   0 when ub <= lb

    f(x)  = (1/A) sum_k W_k prod_d g_kd(x_d)          (g = phi(y_d; mu_kd, s_kd) for dense d)
    lpdf  = log f(x) - sum_{d dense log kind} y_d

Dimension d of candidate g is drawn from the one-component fold `draw_oracle.
fold([1], [mu_kd], [s_kd], low, high, log, q=q_d)`: the dense draw, exp for a
log kind, then rint(v / q) q.
"""
import math

import numpy as np
from scipy.special import erf, erfc

from oracle import draw_oracle as D
from tests import joint_reference as JR

EPS = 1e-12
JOINT_QUANT_KINDS = ('quniform', 'qloguniform', 'qnormal', 'qlognormal')
SQRT2 = math.sqrt(2.0)


class QDim(JR.Dim):
    """A Dim with its step q (None: dense)."""

    def __init__(self, log, low, high, stream, q=None):
        JR.Dim.__init__(self, log, low, high, stream)
        self.q = None if q is None else float(q)


def zmass(zl, zu):
    """Phi(zu sqrt 2) - Phi(zl sqrt 2) for arrays of interval ends z = (bound
    - mu) / (s sqrt 2), from the side of the mean the interval lies on: both
    ends above the mean the difference of the upper tails, both below that of
    the lower tails, a straddling interval the sum of two positive erf terms;
    0 for an empty interval.  No two values near 1/2 or 1 are subtracted: the
    error is a few ulp of the larger tail on one side and a few ulp of the
    mass when straddling (mass_tolerance)."""
    zl, zu = np.broadcast_arrays(np.asarray(zl, dtype=np.float64), np.asarray(zu, dtype=np.float64))
    out = np.zeros(zl.shape)
    ok = zu > zl
    up = ok & (zl >= 0.0)
    dn = ok & (zu <= 0.0)
    mid = ok & ~up & ~dn
    out[up] = 0.5 * (erfc(zl[up]) - erfc(zu[up]))
    out[dn] = 0.5 * (erfc(-zu[dn]) - erfc(-zl[dn]))
    out[mid] = 0.5 * (erf(zu[mid]) + erf(-zl[mid]))
    return out


ERF_ULPS = 4.0     # the error granted to one libm erf / erfc value, in ulp


def mass_tolerance(zl, zu, mass):
    """The absolute error zmass may have at exact ends (zl, zu).  An erf
    value is within ERF_ULPS ulp of its own size.  An erfc value in the tail is
    exp(-z^2) times a slowly varying factor, and a library that rounds z^2
    before the exp carries z^2 2^-53 of relative error from that rounding
    alone: ERF_ULPS + 2 z^2 ulp are granted per tail.  The difference (or
    sum) and the halving add one rounding of the mass."""
    zl, zu = float(zl), float(zu)
    u = 2.0 ** -52
    if zl >= 0.0 or zu <= 0.0:
        a = zl if zl >= 0.0 else -zu      # the end nearer the mean: the larger tail
        return (2.0 * (ERF_ULPS + 2.0 * a * a) * 0.5 * math.erfc(a) + 2.0 * float(mass)) * u
    return (2.0 * ERF_ULPS + 2.0) * float(mass) * u


def interval(dim, x):
    """(ub, lb) of label values x of a quantized dimension, in its working
    space."""
    x = np.asarray(x, dtype=np.float64)
    ub, lb = x + dim.q / 2.0, x - dim.q / 2.0
    if not dim.log:
        if dim.bounded:
            ub, lb = np.minimum(ub, dim.high), np.maximum(lb, dim.low)
        return ub, lb
    if dim.bounded:
        ub, lb = np.minimum(ub, np.exp(dim.high)), np.maximum(lb, np.exp(dim.low))
    lb = np.maximum(0.0, lb)
    return np.log(np.maximum(ub, EPS)), np.log(np.maximum(lb, EPS))


class JointQuantRef(JR.JointRef):
    """dims: list of QDim; below / above: (W [K], mu [K, D], s [K, D])."""

    @property
    def steps(self):
        return np.array([dim.q or 0.0 for dim in self.dims])

    def log_terms(self, values, side):
        """log(W_k prod_d g_kd(x_d)) [n, K] and the Jacobian sum [n] of
        label values x [n, D]; NaN rows for NaN values."""
        W, mu, s = self.sides[side]
        x = np.atleast_2d(np.asarray(values, dtype=np.float64))
        with np.errstate(divide='ignore', invalid='ignore'):
            e = np.tile(np.log(W)[None, :], (len(x), 1))
            jac = np.zeros(len(x))
            for d, dim in enumerate(self.dims):
                if dim.q is None:
                    y = np.log(x[:, d]) if dim.log else x[:, d]
                    z = (y[:, None] - mu[None, :, d]) / s[None, :, d]
                    e += -0.5 * z * z - np.log(s[None, :, d]) - 0.5 * math.log(2.0 * math.pi)
                    if dim.log:
                        jac += y
                else:
                    ub, lb = interval(dim, x[:, d])
                    zu = (ub[:, None] - mu[None, :, d]) / (s[None, :, d] * SQRT2)
                    zl = (lb[:, None] - mu[None, :, d]) / (s[None, :, d] * SQRT2)
                    e += np.log(zmass(zl, zu))
                    e[np.isnan(x[:, d])] = np.nan
        return e, jac

    def joint_lpdf(self, values, side):
        e, jac = self.log_terms(values, side)
        logA = math.log(math.fsum(self.pick_weights(side).tolist()))
        out = np.empty(len(e))
        for i in range(len(e)):
            if np.isnan(e[i]).any() or np.isnan(jac[i]):
                out[i] = np.nan
                continue
            top = np.max(e[i])
            lse = top + math.log(math.fsum(np.exp(e[i] - top).tolist())) if np.isfinite(top) else top
            out[i] = lse - logA - jac[i]
        return out

    def fold(self, k, d):
        _, mu, s = self.sides['below']
        dim = self.dims[d]
        return D.fold([1.0], [mu[k, d]], [s[k, d]], dim.low if dim.bounded else None,
                      dim.high if dim.bounded else None, log=dim.log, q=dim.q)


def prior_of(kind, args):
    """(log, low, high, prior_mu, prior_sigma, q, observation transform) of a
    label of a quantized joint group: the priors of tests/joint_reference.py,
    the quantized kinds those of their kind without q; the transform of a
    quantized log kind floors the observation (an observed 0 is legal)."""
    q = float(args['q']) if kind in JOINT_QUANT_KINDS else None
    base = kind[1:] if kind in JOINT_QUANT_KINDS else kind
    log, low, high, pmu, psig = JR.prior_of(base, args)
    if kind == 'qloguniform':
        floor = max(EPS, math.exp(low))
        tr = lambda o: np.log(np.maximum(np.asarray(o, dtype=np.float64), floor))
    elif kind == 'qlognormal':
        tr = lambda o: np.log(np.maximum(np.asarray(o, dtype=np.float64), EPS))
    elif log:
        tr = lambda o: np.log(np.asarray(o, dtype=np.float64))
    else:
        tr = lambda o: np.asarray(o, dtype=np.float64)
    return log, low, high, pmu, psig, q, tr
