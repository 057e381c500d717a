"""Plain restatement of tpe.importance / tpe_importance: the split, the
counts and alpha from the definition ("Hyperparameter
importance"), the lpdfs from the CPU oracle (a merged cell of a quantized
label: the oracle's quantized lpdf with q = merge q), the per-cell term and
the sum as loops.  Nothing here touches the engine."""
import math

import numpy as np

from hyperopt_amd import posterior as P
from oracle import tpe_oracle as O


def term(lb, la, w, alpha):
    """w p (m - alpha)^2 of one cell from its two lpdfs: the arithmetic of the
    definition, operation by operation."""
    if lb == -np.inf and la == -np.inf:
        return 0.0
    if lb != lb or la != la:
        return float('nan')
    om = 1.0 - alpha
    d = lb - la
    if d <= 0.0:
        t = math.expm1(d)
        dev = alpha * om * t / (1.0 + alpha * t)
    else:
        t = math.expm1(-d)
        dev = -(alpha * om * t) / (1.0 + om * t)
    p = alpha * math.exp(lb) + om * math.exp(la)
    return w * p * (dev * dev)


def terms(lb, la, w, alpha):
    return np.array([term(float(b), float(a), float(wj), alpha) for b, a, wj in zip(lb, la, w)])


def v_of(lb, la, w, alpha):
    """The sum of the terms, in math.fsum: correctly rounded, so the whole
    summation error of a comparison is the other side's."""
    t = terms(lb, la, w, alpha)
    return float('nan') if np.isnan(t).any() else math.fsum(t)


def density(lb, la, alpha):
    """p = alpha l + (1 - alpha) g at the cells."""
    return alpha * np.exp(lb) + (1.0 - alpha) * np.exp(la)


def planes(post, x, merge=1):
    """(lb, la) of a posterior.LabelPosterior at the cells x through the
    oracle's lpdfs."""
    x = np.asarray(x, dtype=float)
    if post.family == 'categorical':
        return O.categorical_lpdf(x, post.below), O.categorical_lpdf(x, post.above)
    f = O.gmm1_lpdf if post.family == 'GMM1' else O.lgmm1_lpdf
    q = None if post.q is None else merge * post.q
    return (f(x, *post.below, low=post.low, high=post.high, q=q),
            f(x, *post.above, low=post.low, high=post.high, q=q))


def split(hist, quantile):
    """(below tids, above tids) of a tests.helpers history: the ceil(quantile
    n) best by loss, ties by trial order."""
    n = len(hist.tids)
    n_below = int(math.ceil(quantile * n))
    order = sorted(range(n), key=lambda i: (hist.losses[i], i))
    return hist.tids[order[:n_below]], hist.tids[order[n_below:]]


def label_inputs(hist, quantile=0.1, prior_weight=1.0):
    """Per label of the history: (posterior, nb, na, observations) -- the two
    observation lists in trial order, split by membership of the trial."""
    below, above = (set(t.tolist()) for t in split(hist, quantile))
    out = []
    for name, kind, args in hist.labels:
        oi, ov = hist.obs[name]
        b = np.asarray([v for t, v in zip(oi.tolist(), ov.tolist()) if t in below])
        a = np.asarray([v for t, v in zip(oi.tolist(), ov.tolist()) if t in above])
        keep = np.asarray([t in below or t in above for t in oi.tolist()], dtype=bool)
        out.append((P.label_posterior(name, kind, args, b, a, prior_weight), len(b), len(a), ov[keep]))
    return out


def importance(hist, quantile=0.1, n_grid=4096, prior_weight=1.0, normalize=True):
    """{label: importance} of a history, and the raw V per label."""
    n = len(hist.tids)
    raw, vs = [], {}
    for (name, kind, args), (post, nb, na, ov) in zip(hist.labels, label_inputs(hist, quantile, prior_weight)):
        v = 0.0
        if nb and na:
            x, w, merge = P.importance_cells(kind, args, ov, n_grid)
            lb, la = planes(post, x, merge)
            v = v_of(lb, la, w, nb / (nb + na))
        vs[name] = v
        raw.append((nb + na) / n * v)
    raw = np.asarray(raw)
    if normalize:
        raw = raw / raw.sum() if raw.sum() != 0 else np.zeros(len(raw))
    return {name: float(r) for (name, _, _), r in zip(hist.labels, raw)}, vs


def planted(n=400, seed=11):
    """The history of the issue: ALL_KINDS, each label active in 80 % of the
    trials, loss (u - 2)^2 + 0.3 |log lu| + 0.05 noise with u = 0 and lu = 1
    where the label is absent."""
    from tests.helpers import ALL_KINDS, make_history
    h = make_history(ALL_KINDS, n, seed=seed, active_frac=0.8)
    u = np.zeros(n)
    lu = np.ones(n)
    pos = {int(t): i for i, t in enumerate(h.tids)}
    for t, v in zip(*h.obs['u']):
        u[pos[int(t)]] = v
    for t, v in zip(*h.obs['lu']):
        lu[pos[int(t)]] = v
    h.losses = (u - 2.0) ** 2 + 0.3 * np.abs(np.log(lu)) + 0.05 * np.random.RandomState(seed + 1).normal(size=n)
    return h
