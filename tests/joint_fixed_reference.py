"""Conditioning a joint group on fixed dimensions: the rule in plain loops
with `math` only (test infrastructure, imported by the tests only; it builds
beside tests/joint_reference.py, joint_quant_reference.py and
joint_cat_reference.py, whose dimension records and mass it reuses).

A side's mixture has K components (0: the prior) with weights W_k and, per
dimension d, a factor g_kd(x_d) of the label value x_d:

    dense        phi(y_d; mu_kd, s_kd),  y = log x for a log kind
    quantized    Phi((ub - mu_kd)/s_kd) - Phi((lb - mu_kd)/s_kd) over the value's
                 rounding interval (joint_quant_reference), 0 when it is empty
    categorical  r_0d[x] = p_d[x],  r_td[x] = ([x == o_td] + a p_d[x]) / (1 + a),
                 a = C_d prior_weight / K  (joint_cat_reference)

Given the fixed dimensions F at values x_F the conditional over the free
dimensions is the mixture of the same components' free columns with

    L_k  = log W_k + sum_{d in F} log g_kd(x_d)
    lse  = L_max + log(sum_k exp(L_k - L_max))
    W'_k = max(exp(L_k - lse), 2^-1022)

A side on which every L_k is -inf has no conditional: ValueError.
"""
import math

from tests import joint_reference as JR

EPS = 1e-12
FLOOR = 2.0 ** -1022
NEG_INF = float('-inf')


def _log(v):
    return math.log(v) if v > 0.0 else NEG_INF


def interval(dim, x):
    """(ub, lb) of the rounding interval of label value x in the working
    space of a quantized dimension."""
    ub, lb = x + dim.q / 2.0, x - dim.q / 2.0
    if not dim.log:
        if dim.bounded:
            ub, lb = min(ub, dim.high), max(lb, dim.low)
        return ub, lb
    if dim.bounded:
        ub, lb = min(ub, math.exp(dim.high)), max(lb, math.exp(dim.low))
    lb = max(0.0, lb)
    return math.log(max(ub, EPS)), math.log(max(lb, EPS))


def log_factor(dim, x, k, K, mu, s, prior_weight):
    """log g_kd(x) of component k of a side of K components; mu, s: the
    component's entries of the dimension."""
    upper = getattr(dim, 'upper', None)
    q = getattr(dim, 'q', None)
    if upper:
        if not (0.0 <= x < upper and x == math.floor(x)):
            return NEG_INF
        c = int(x)
        if k == 0:
            return math.log(dim.p[c])
        a = upper * prior_weight / K
        return math.log(((1.0 if c == int(mu) else 0.0) + a * dim.p[c]) / (1.0 + a))
    if q:
        ub, lb = interval(dim, x)
        if not ub > lb:
            return NEG_INF
        return _log(JR.mass(mu, s, lb, ub))
    if dim.log and not x > 0.0:
        return NEG_INF
    y = math.log(x) if dim.log else x
    z = (y - mu) / s
    return -0.5 * z * z - math.log(s) - 0.5 * math.log(2.0 * math.pi)


def condition_side(dims, W, mu, s, fixed, values, prior_weight):
    """(L_k - lse [K], W'_k [K]) of one side; fixed: dimension indices,
    values: their label values."""
    K = len(W)
    L = []
    for k in range(K):
        lk = _log(float(W[k]))
        for d, x in zip(fixed, values):
            lk += log_factor(dims[d], float(x), k, K, float(mu[k][d]), float(s[k][d]), prior_weight)
        L.append(lk)
    top = max(L)
    if not top > NEG_INF:
        raise ValueError('no component reaches the fixed values')
    lse = top + math.log(math.fsum(math.exp(lk - top) for lk in L))
    rel = [lk - lse for lk in L]
    return rel, [max(math.exp(r), FLOOR) if r > NEG_INF else FLOOR for r in rel]


def condition(dims, below, above, fixed, values, prior_weight=1.0):
    """The conditioned group: (free dimension indices, below', above', (rel
    below, rel above)) -- a side' is (W' [K], mu [K][R], s [K][R]) as lists,
    rel the L_k - lse the weights were formed from."""
    fixed = [int(d) for d in fixed]
    free = [d for d in range(len(dims)) if d not in fixed]
    sides, rels = [], []
    for W, mu, s in (below, above):
        rel, Wp = condition_side(dims, W, mu, s, fixed, values, prior_weight)
        sides.append((Wp, [[float(mu[k][d]) for d in free] for k in range(len(W))],
                      [[float(s[k][d]) for d in free] for k in range(len(W))]))
        rels.append(rel)
    return free, sides[0], sides[1], tuple(rels)
