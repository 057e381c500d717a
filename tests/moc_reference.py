"""Plain numpy statement of the order behind tpe.suggest(constraints=...)
(tpe_mo_keys_constrained, posterior.mo_keys(F, G=G)): the violation by the
explicit left-to-right loop over the constraints, the full dominance matrix of
the feasible rows (tests/mo_reference.py), and the order as one np.lexsort.  It
is the yardstick: nothing here calls the code under test."""
import numpy as np

from tests import mo_reference as R


def violation(F, G):
    """v[i] = ((0.0 + max(G[i, 0], 0)) + max(G[i, 1], 0)) + ... in float64, one
    row at a time; NaN for a dead row (a NaN anywhere in F[i] or G[i])."""
    F = np.asarray(F, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    v = np.empty(len(G))
    for i in range(len(G)):
        if np.isnan(F[i]).any() or np.isnan(G[i]).any():
            v[i] = np.nan
            continue
        s = np.float64(0.0)
        with np.errstate(over='ignore'):
            for g in G[i]:
                s = s + max(np.float64(g), np.float64(0.0))
        v[i] = s
    return v


def counts(F, G):
    """(by, do, v): dead rows -1, -1, NaN; feasible rows (v == 0) their
    dominance counts among the feasible rows; infeasible rows the number of
    live rows of strictly smaller violation, and 0."""
    F = np.asarray(F, dtype=np.float64)
    v = violation(F, G)
    by = np.full(len(F), -1, dtype=np.int64)
    do = np.full(len(F), -1, dtype=np.int64)
    feas = v == 0.0
    D = R.dominance(F[feas])
    by[feas] = D.sum(axis=0)
    do[feas] = D.sum(axis=1)
    live = ~np.isnan(v)
    for i in np.flatnonzero(v > 0.0):
        by[i] = int((v[live] < v[i]).sum())
        do[i] = 0
    return by, do, v


def order_keys(by, do):
    """The positions under ascending by, descending do, ascending row
    position; NaN where by is -1."""
    pos = np.flatnonzero(by >= 0)
    order = np.lexsort((pos, -do[pos], by[pos]))
    out = np.full(len(by), np.nan)
    out[pos[order]] = np.arange(len(pos))
    return out


def keys(F, G):
    """keys[i]: the position of row i in the order; NaN for a dead row."""
    by, do, _ = counts(F, G)
    return order_keys(by, do)


def front(F, G):
    """Row positions of the feasible rows that no feasible row dominates."""
    by, _, v = counts(F, G)
    return np.flatnonzero((by == 0) & (v == 0.0))


# -- the cases both test files run ---------------------------------------------

SHIFTS = (1.0, 0.5, 0.0)          # G = uniform - s: all feasible, mixed, none feasible


def grid_case(n, M, K, s):
    rng = np.random.RandomState(100000 * K + 1000 * M + n)
    F = rng.uniform(size=(n, M))
    G = rng.uniform(size=(n, K)) - s
    return F, G


def tied_case():
    """Integer-valued rows: 224 feasible, 7 distinct violations, repeated rows."""
    rng = np.random.RandomState(4)
    G = rng.randint(-3, 3, (700, 3)).astype(float)
    F = rng.randint(0, 4, (700, 3)).astype(float)
    return F, G


def special_case():
    """+-inf, -0.0, an overflowing sum; NaN in G alone, in F alone, in both."""
    inf, nan = np.inf, np.nan
    F = np.array([(0.0, 1.0), (1.0, 0.0), (0.5, 0.5), (2.0, 2.0), (0.0, 0.0), (3.0, 3.0), (0.1, 0.1),
                  (0.2, 0.2), (nan, 0.0), (0.3, 0.3), (nan, nan), (-inf, -inf), (inf, -1.0), (1.0, 1.0)])
    G = np.array([(-inf, -0.0), (0.0, -1.0), (-0.0, 0.0), (inf, -1.0), (1e308, 1e308), (1e308, -inf),
                  (nan, -1.0), (1.0, nan), (-1.0, -1.0), (-1.0, -1.0), (nan, nan), (2.0, 0.5),
                  (-1.0, -inf), (0.5, 2.0)])
    return F, G
