"""The Scott-rule mixtures of a joint group, restated in plain loops from the
rule itself ("Bandwidth of joint groups"), not from
posterior.joint_mixture:

  a side with n trials (in Splitter.split order) in a group of D labels,
  categorical ones counted, has K = n + 1 components, component 0 the prior;
  means   row 0 the prior mean, row t + 1 observation t in the working space;
  sigmas  non-categorical dimension d, rows 1..n:
            s_d = clip(f prior_sigma_d, prior_sigma_d / min(100, 1 + K), prior_sigma_d),
            f = 0.2 n^(-1/(D+4))  (0.2 for n <= 1),
          row 0 prior_sigma_d; a quantized kind with its unquantized prior;
  weights w = (prior_weight, linear_forgetting_weights(n, 25)), W = w / sum(w),
          the sum in np.sum's order;
  a categorical dimension: the observed category in the mean column (row 0:
          0), sigma 1.

Every float64 operation is written out once, in the order numpy performs it.
"""
import math

import numpy as np

EPS = 1e-12
LF = 25


def factor(n, D):
    if n <= 1:
        return 0.2
    return 0.2 * math.pow(float(n), -1.0 / (D + 4))


def prior(kind, args):
    """(mean, sigma, log kind, categorical) of a label in its working space."""
    if kind in ('randint', 'categorical'):
        return 0.0, 1.0, False, True
    base = kind[1:] if kind[0] == 'q' else kind
    if base in ('uniform', 'loguniform'):
        low, high = float(args['low']), float(args['high'])
        return 0.5 * (high + low), 1.0 * (high - low), base == 'loguniform', False
    assert base in ('normal', 'lognormal'), kind
    return float(args['mu']), float(args['sigma']), base == 'lognormal', False


def working(kind, args, column):
    """A label's observations in its working space (the log of a whole column
    at once: numpy's vector log, which is what the library is handed)."""
    v = np.asarray(column, dtype=np.float64)
    if kind in ('loguniform', 'lognormal'):
        return np.log(v)
    if kind == 'qloguniform':
        return np.log(np.maximum(v, max(EPS, float(np.exp(float(args['low']))))))
    if kind == 'qlognormal':
        return np.log(np.maximum(v, EPS))
    return v


def forgetting_weights(n, lf=LF):
    """linear_forgetting_weights(n, lf): np.linspace(1/n, 1, n - lf) -- element
    i is i * step + start, the last one the stop itself -- then lf ones."""
    if n < lf:
        return [1.0] * n
    num = n - lf
    start = 1.0 / n
    ramp = []
    if num == 1:
        ramp = [start]
    elif num > 1:
        step = (1.0 - start) / (num - 1)
        ramp = [i * step + start for i in range(num)]
        ramp[-1] = 1.0
    return ramp + [1.0] * lf


def _pairwise(a, lo, n):
    """numpy's pairwise_sum of a[lo : lo + n] (loops_utils.h.src)."""
    if n < 8:
        res = 0.0
        for i in range(n):
            res += a[lo + i]
        return res
    if n <= 128:
        r = [a[lo + j] for j in range(8)]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] += a[lo + i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += a[lo + i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a, lo, n2) + _pairwise(a, lo + n2, n - n2)


def np_sum(a):
    """np.sum of a contiguous float64 vector: buffer-sized chunks of 8192
    added in order to 0.0, each summed pairwise."""
    res = 0.0
    for lo in range(0, len(a), 8192):
        res += _pairwise(a, lo, min(8192, len(a) - lo))
    return res


def side(group, rows, prior_weight):
    """(W [K], mu [K, D], sigma [K, D]) of one side: group = [(kind, args)],
    rows = the side's trials in order, each the D raw values of the labels."""
    D, n = len(group), len(rows)
    K = n + 1
    w = [float(prior_weight)] + forgetting_weights(n)
    total = np_sum(w)
    W = np.array([x / total for x in w], dtype=np.float64)
    mu = np.empty((K, D))
    sig = np.empty((K, D))
    f = factor(n, D)
    for d, (kind, args) in enumerate(group):
        pm, ps, _, cat = prior(kind, args)
        if cat:
            mu[0, d], sig[0, d] = 0.0, 1.0
            for t in range(n):
                mu[t + 1, d], sig[t + 1, d] = float(rows[t][d]), 1.0
            continue
        lo = ps / min(100.0, 1.0 + K)
        s = f * ps
        if s < lo:
            s = lo
        if s > ps:
            s = ps
        mu[0, d], sig[0, d] = pm, ps
        y = working(kind, args, [r[d] for r in rows])
        for t in range(n):
            mu[t + 1, d], sig[t + 1, d] = y[t], s
    return W, mu, sig
