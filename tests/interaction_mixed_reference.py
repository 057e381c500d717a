"""Plain restatement of tpe_interactions_mixed ("Pairwise
interactions"): the three factor kinds with math.erf / math.erfc, the planes
and marginals cell by cell with math.fsum over the components.  The dense
parts and the per-cell terms are tests/interaction_reference.py's.  Nothing
here touches the engine; an axis is a posterior.InteractionAxis."""
import math

import numpy as np

from tests import interaction_reference as IR
from tests.joint_quant_reference import mass_tolerance

EPS = 1e-12
DENSE, QUANTIZED, CATEGORICAL = 0, 1, 2


def interval(ax, x):
    """(lb, ub) of the cell at label value x of a quantized axis, in the working space."""
    ub, lb = x + ax.step / 2.0, x - ax.step / 2.0
    bounded = ax.low == ax.low and ax.high == ax.high
    if not ax.log:
        return (max(lb, ax.low), min(ub, ax.high)) if bounded else (lb, ub)
    if bounded:
        ub, lb = min(ub, math.exp(ax.high)), max(lb, math.exp(ax.low))
    return math.log(max(max(0.0, lb), EPS)), math.log(max(ub, EPS))


def zmass(zl, zu):
    """Phi(zu sqrt 2) - Phi(zl sqrt 2) from the side of the mean the interval lies on; 0 when empty."""
    if not zu > zl:
        return 0.0
    if zl >= 0.0:
        return 0.5 * (math.erfc(zl) - math.erfc(zu))
    if zu <= 0.0:
        return 0.5 * (math.erfc(-zu) - math.erfc(-zl))
    return 0.5 * (math.erf(zu) + math.erf(-zl))


def quantized_factor(ax, mu, s):
    """(u [K, G], tol [K, G]): the interval masses and the absolute error one may have (mass_tolerance)."""
    u, tol = np.zeros((len(mu), len(ax.x))), np.zeros((len(mu), len(ax.x)))
    for i, x in enumerate(ax.x):
        lb, ub = interval(ax, float(x))
        for k in range(len(mu)):
            r2 = float(s[k]) * math.sqrt(2.0)
            zl, zu = (lb - float(mu[k])) / r2, (ub - float(mu[k])) / r2
            u[k, i] = zmass(zl, zu)
            tol[k, i] = mass_tolerance(zl, zu, u[k, i]) if zu > zl else 0.0
    return u, tol


def categorical_factor(ax, obs, pw):
    """r [K, C]: row 0 the prior p, row t ([c == o_t] + a p[c]) / (1 + a), a = C pw / K."""
    K, p = len(obs), np.asarray(ax.p, dtype=np.float64)
    a = ax.upper * pw / K
    r = np.array([[((1.0 if c == int(obs[k]) else 0.0) + a * p[c]) / (1.0 + a) for c in range(ax.upper)]
                  for k in range(K)])
    r[0] = p
    return r


def factor(ax, mu, s, pw):
    """(u [K, G], tol [K, G] or None, m [K]) of one label of one side."""
    if ax.kind == CATEGORICAL:
        return categorical_factor(ax, mu, pw), None, np.ones(len(mu))
    m = IR.masses(mu, s, ax.low, ax.high)
    if ax.kind == QUANTIZED:
        return quantized_factor(ax, mu, s) + (m,)
    return IR.factor(ax.x, mu, s), None, m


def side_planes(side, d, e, axes, pw):
    """(L [G_d, G_e], L_d, L_e, slack) of one side (W, mu [K, D], s [K, D]); slack: the largest relative error,
    in units of 2^-52, that the interval masses' own error leaves in a marginal (0 without a quantized axis)."""
    W, mu, s = side
    ud, td, md = factor(axes[d], mu[:, d], s[:, d], pw)
    ue, te, me = factor(axes[e], mu[:, e], s[:, e], pw)
    A = math.fsum(((W * md) * me).tolist())
    wud = W[:, None] * ud
    Gd, Ge = ud.shape[1], ue.shape[1]
    L = np.array([[math.fsum((wud[:, i] * ue[:, j]).tolist()) for j in range(Ge)] for i in range(Gd)]) / A
    Ld = np.array([math.fsum((wud[:, i] * me).tolist()) for i in range(Gd)]) / A
    Le = np.array([math.fsum(((W * ue[:, j]) * md).tolist()) for j in range(Ge)]) / A
    slack = 0.0
    for t, mo, marg in ((td, me, Ld), (te, md, Le)):
        if t is not None:
            err = np.array([math.fsum(((W * t[:, i]) * mo).tolist()) for i in range(t.shape[1])]) / A
            slack += max([er / v for er, v in zip(err, marg) if v > 0.0] + [0.0]) * 2.0 ** 52
    return L, Ld, Le, slack


def sums(L, G, below, above, alpha, area):
    """(V, H, mass = area sum p) of a pair from its [G_d, G_e] planes and (L_d, L_e), (G_d, G_e), by math.fsum."""
    t = np.array([IR.terms(float(L[i, j]), float(G[i, j]), float(below[0][i]), float(below[1][j]),
                           float(above[0][i]), float(above[1][j]), alpha)
                  for i in range(L.shape[0]) for j in range(L.shape[1])])
    if np.isnan(t).any():
        return float('nan'), float('nan'), float('nan')
    return area * math.fsum(t[:, 1]), area * math.fsum(t[:, 2]), area * math.fsum(t[:, 0])
