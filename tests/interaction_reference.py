"""Plain restatement of tpe_interactions ("Pairwise
interactions"): densities and marginals cell by cell with math.fsum over the
components, the terms operation by operation.  Nothing here touches the engine."""
import math

import numpy as np

from tests.joint_reference import mass

SQRT_2PI = 2.5066282746310002


def factor(y, mu, s):
    """u[k, i] = exp(-((y_i - mu_k) / s_k)^2 / 2) / (s_k sqrt(2 pi))."""
    with np.errstate(invalid='ignore'):
        z = (np.asarray(y)[None, :] - mu[:, None]) / s[:, None]
        return np.exp(-0.5 * (z * z)) / (s[:, None] * SQRT_2PI)


def masses(mu, s, low, high):
    bounded = low == low and high == high
    return np.array([mass(float(m), float(v), low, high) if bounded else 1.0 for m, v in zip(mu, s)])


def side_planes(side, d, e, y_d, y_e, bounds):
    """(L [G, G], L_d [G], L_e [G]) of one side (W, mu [K, D], s [K, D]) for
    the pair (d, e); bounds[d] = (low, high), NaN without."""
    W, mu, s = side
    ud, ue = factor(y_d, mu[:, d], s[:, d]), factor(y_e, mu[:, e], s[:, e])
    md, me = masses(mu[:, d], s[:, d], *bounds[d]), masses(mu[:, e], s[:, e], *bounds[e])
    A = math.fsum(((W * md) * me).tolist())
    wud = W[:, None] * ud
    G = len(y_d)
    L = np.array([[math.fsum((wud[:, i] * ue[:, j]).tolist()) for j in range(G)] for i in range(G)]) / A
    Ld = np.array([math.fsum((wud[:, i] * me).tolist()) for i in range(G)]) / A
    Le = np.array([math.fsum(((W * ue[:, j]) * md).tolist()) for j in range(G)]) / A
    return L, Ld, Le


def terms(L, G, Ld, Le, Gd, Ge, alpha):
    """(p, p (m - alpha)^2, p (m - m_ind)^2) of one cell, operation by operation."""
    if any(v != v for v in (L, G, Ld, Le, Gd, Ge)):
        return (float('nan'),) * 3
    om = 1.0 - alpha
    ao = alpha * om
    aL = alpha * L
    p = aL + om * G
    if p == 0.0:
        return 0.0, 0.0, 0.0
    dev = (ao * (L - G)) / p
    qi, ri = alpha * (Ld * Le), om * (Gd * Ge)
    den = qi + ri
    if den == 0.0:
        dif = dev
    else:
        mi, ci = qi / den, ri / den
        log = lambda v: math.log(v) if v > 0.0 else -math.inf
        lo = log(L) - log(G)
        loi = (log(Ld) + log(Le)) - (log(Gd) + log(Ge))
        if not math.isfinite(lo) or not math.isfinite(loi):
            dif = aL / p - mi
        else:
            dl = lo - loi
            if dl <= 0.0:
                t = math.expm1(dl)
                dif = ((mi * ci) * t) / (1.0 + mi * t)
            else:
                t = math.expm1(-dl)
                dif = -((mi * ci) * t) / (1.0 + ci * t)
    return p, p * (dev * dev), p * (dif * dif)


def sums(L, G, below, above, alpha, h_d, h_e):
    """(V, H, mass = h_d h_e sum p) of a pair from its planes and (L_d, L_e), (G_d, G_e), by math.fsum."""
    n = len(L)
    t = np.array([terms(float(L[i, j]), float(G[i, j]), float(below[0][i]), float(below[1][j]),
                        float(above[0][i]), float(above[1][j]), alpha) for i in range(n) for j in range(n)])
    if np.isnan(t).any():
        return float('nan'), float('nan'), float('nan')
    hh = h_d * h_e
    return hh * math.fsum(t[:, 1]), hh * math.fsum(t[:, 2]), hh * math.fsum(t[:, 0])


def pair(below, above, d, e, y_d, y_e, h_d, h_e, bounds, alpha):
    L, Ld, Le = side_planes(below, d, e, y_d, y_e, bounds)
    G, Gd, Ge = side_planes(above, d, e, y_d, y_e, bounds)
    return sums(L, G, (Ld, Le), (Gd, Ge), alpha, h_d, h_e)[:2]
