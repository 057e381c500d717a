"""The joint (multivariate) TPE definition in numpy fp64, written without
posterior.joint_mixture (test infrastructure, imported by the tests only).

A joint group is D dense continuous labels, each with a working space (y =
log x for the log kinds) and, when it has both bounds, the interval [low,
high) of that space.  The joint mixture of a side has K components (0: the
prior): weights W[k], means mu[k, d], sigmas s[k, d], and

    f(y)  = (1/A) sum_k W_k prod_d phi(y_d; mu_kd, s_kd)
    A     = sum_k W_k prod_d m_kd,   m_kd = Phi((high_d - mu_kd)/s_kd) - Phi((low_d - mu_kd)/s_kd)
    lpdf  = log f(y) - sum_{d log kind} y_d

Candidate g picks a below component with the pick word of the stream
JOINT_STREAM through thresholds over W_k prod_d m_kd, and draws dimension d
with the words of the label's own stream from the one-component mixture
(mu_kd, s_kd) truncated to [low_d, high_d): `draw_oracle.fold([1], ...)`.
"""
import math

import numpy as np

from oracle import draw_oracle as D

JOINT_STREAM = 0x7FFFFFFF
JOINT_KINDS = ('uniform', 'loguniform', 'normal', 'lognormal')


class Dim(object):
    """One label of a joint group: log (bool), low / high (working-space
    bounds, None without), stream."""

    def __init__(self, log, low, high, stream):
        self.log, self.low, self.high, self.stream = bool(log), low, high, int(stream)

    @property
    def bounded(self):
        return self.low is not None and self.high is not None


def _tail(x):
    """1 - Phi(x) = erfc(x / sqrt 2) / 2, accurate for x > 0."""
    return 0.5 * math.erfc(x / math.sqrt(2.0))


def mass(mu, s, low, high):
    """Phi((high - mu)/s) - Phi((low - mu)/s) without cancellation: from the
    two tails on the side of the mean the interval lies on."""
    a, b = (low - mu) / s, (high - mu) / s
    if a >= 0.0:
        return _tail(a) - _tail(b)
    if b <= 0.0:
        return _tail(-b) - _tail(-a)
    return 1.0 - _tail(-a) - _tail(b)


class JointRef(object):
    """dims: list of Dim; below / above: (W [K], mu [K, D], s [K, D])."""

    def __init__(self, dims, below, above):
        self.dims = list(dims)
        self.sides = {'below': tuple(np.asarray(a, dtype=np.float64) for a in below),
                      'above': tuple(np.asarray(a, dtype=np.float64) for a in above)}
        self.D = len(self.dims)

    def masses(self, side):
        W, mu, s = self.sides[side]
        m = np.ones(mu.shape)
        for d, dim in enumerate(self.dims):
            if dim.bounded:
                for k in range(len(W)):
                    m[k, d] = mass(float(mu[k, d]), float(s[k, d]), dim.low, dim.high)
        return m

    def pick_weights(self, side='below'):
        """W_k prod_d m_kd: unnormalised pick probabilities / the terms of A."""
        W = self.sides[side][0]
        return W * np.prod(self.masses(side), axis=1)

    def working(self, values):
        """y [n, D] of label values x [n, D]."""
        y = np.array(values, dtype=np.float64, copy=True)
        for d, dim in enumerate(self.dims):
            if dim.log:
                with np.errstate(divide='ignore', invalid='ignore'):
                    y[:, d] = np.log(y[:, d])
        return y

    def joint_lpdf(self, values, side):
        W, mu, s = self.sides[side]
        y = self.working(np.atleast_2d(values))
        logA = math.log(math.fsum(self.pick_weights(side).tolist()))
        with np.errstate(divide='ignore'):
            logw = np.log(W)
        out = np.empty(len(y))
        for i in range(len(y)):
            z = (y[i][None, :] - mu) / s
            e = logw + np.sum(-0.5 * z * z - np.log(s) - 0.5 * math.log(2.0 * math.pi), axis=1)
            top = np.max(e)
            lse = top + math.log(math.fsum(np.exp(e - top).tolist())) if np.isfinite(top) else top
            out[i] = lse - logA - sum(y[i, d] for d, dim in enumerate(self.dims) if dim.log)
        return out

    def score(self, values):
        return self.joint_lpdf(values, 'below') - self.joint_lpdf(values, 'above')

    def pick_fold(self):
        """The categorical fold of the component pick."""
        return D.fold(self.pick_weights('below'))

    def fold(self, k, d):
        """The one-component fold dimension d of below component k draws from."""
        _, mu, s = self.sides['below']
        dim = self.dims[d]
        return D.fold([1.0], [mu[k, d]], [s[k, d]], dim.low if dim.bounded else None,
                      dim.high if dim.bounded else None, log=dim.log)

    def port_draw(self, seed, round, g):
        """(component [n], values [n, D], excluded [n]) of candidates g by
        the fp64 draw port -- what a device draws, up to the port's error."""
        g = np.asarray(g, dtype=np.uint64)
        pf = self.pick_fold()
        wp, wu = D.draw_words(seed, JOINT_STREAM, round, g)
        comp = D.pick(pf, wp)
        excl = D.excluded(pf, wp, wu)
        vals = np.empty((len(g), self.D))
        for d, dim in enumerate(self.dims):
            wpd, wud = D.draw_words(seed, dim.stream, round, g)
            for k in np.unique(comp):
                sel = comp == k
                f = self.fold(int(k), d)
                _, _, x, v = D.draw_fp64(f, wpd[sel], wud[sel])
                vals[sel, d] = v
                excl[sel] |= D.excluded(f, wpd[sel], wud[sel], x)
        return comp, vals, excl


# ------------------------------------------------- the mixture of a history ----
def prior_of(kind, args):
    """(log, low, high, prior_mu, prior_sigma) of a joint-group label (the
    ap_*_sampler registry's priors, tpe.py:493-576)."""
    log = kind in ('loguniform', 'lognormal')
    if kind in ('uniform', 'loguniform'):
        low, high = float(args['low']), float(args['high'])
        return log, low, high, 0.5 * (high + low), 1.0 * (high - low)
    return log, None, None, float(args['mu']), float(args['sigma'])


def side_mixture(cols, priors, prior_weight, parzen):
    """cols[d]: the side's observations of label d in trial order, already in
    the working space; priors[d] = (prior_mu, prior_sigma); parzen: the
    univariate build adaptive_parzen_normal.  Returns (W, mu, s) with W taken
    from the first label."""
    n, Dn = len(cols[0]), len(cols)
    mu = np.empty((n + 1, Dn))
    s = np.empty((n + 1, Dn))
    Ws = []
    for d in range(Dn):
        o = np.asarray(cols[d], dtype=np.float64)
        pmu, psig = priors[d]
        w, srt, sig = parzen(o, prior_weight, pmu, psig)
        # the sorted sequence as the build forms it: its own argsort, the
        # prior inserted at its searchsorted position
        if n >= 2:
            seq = [int(i) for i in np.argsort(o)]
            seq.insert(int(np.searchsorted(o[seq], pmu)), -1)
        elif n == 1:
            seq = [-1, 0] if pmu < o[0] else [0, -1]
        else:
            seq = [-1]
        W = np.empty(n + 1)
        for at, t in enumerate(seq):
            row = 0 if t < 0 else t + 1
            W[row] = w[at]
            mu[row, d] = pmu if t < 0 else o[t]
            s[row, d] = sig[at]
            assert srt[at] == mu[row, d]
        Ws.append(W)
    return Ws, mu, s
