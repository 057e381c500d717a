"""Plain statement of the hypervolume tie-break (tpe_mo_keys_hv,
posterior.mo_keys(..., tiebreak='hypervolume')): ranks from the n x n
comparison matrices, hypervolumes by coordinate compression (the covered cells
of the compressed grid, counted), greedy selection with gain(c) = vol(c) -
HV({max(c, p)}), on the (by, do) order of tests/mo_reference.py and
tests/moc_reference.py.  It is the yardstick: nothing here calls the code
under test."""
import functools

import numpy as np

from tests import mo_reference as R
from tests import moc_reference as RC


def ranks(F, ok):
    """r[i][m] = the rows j of `ok` with F[j][m] < F[i][m] (IEEE <)."""
    F = np.asarray(F, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.stack([(F[ok, m][None, :] < F[:, m][:, None]).sum(axis=1) for m in range(F.shape[1])], axis=1)


def hv(points, ref):
    """The integer cells in the union of the boxes [points[k], ref): on the
    grid of the points' own coordinates a cell is covered when some point is
    <= its lower corner on every axis."""
    points = np.asarray(points, dtype=np.int64).reshape(-1, np.shape(points)[-1])
    if not len(points):
        return 0
    M, widths, below = points.shape[1], None, []
    for m in range(M):
        edges = np.unique(np.append(points[:, m], ref))
        below.append((points[:, m][None, :] <= edges[:-1, None]).astype(np.int64))      # [cells, points]
        w = np.diff(edges)
        widths = w if widths is None else np.multiply.outer(widths, w)
    covered = np.einsum('ak,bk->ab' if M == 2 else 'ak,bk,ck->abc', *below) > 0
    return int((widths * covered).sum())


def select(F, n_select, G=None):
    """dict(keys, by, do, picked, gains, straddles): the rule, start to end."""
    F = np.asarray(F, dtype=np.float64)
    if G is None:
        by, do = R.counts(F)
        ok = ~np.isnan(F).any(axis=1)
    else:
        by, do, v = RC.counts(F, G)
        ok = v == 0.0
    keys = RC.order_keys(by, do)
    out = dict(keys=keys, by=by, do=do, picked=np.zeros(0, dtype=np.int64), gains=[], straddles=False)
    live = np.flatnonzero(by >= 0)
    if n_select <= 0 or n_select >= len(live):
        return out
    order = live[np.argsort(keys[live])]
    s, t = order[n_select - 1], order[n_select]
    if by[s] != by[t] or not ok[s] or not ok[t]:
        return out
    level = [int(i) for i in order if by[i] == by[s]]
    a = int(keys[level[0]])
    q = n_select - a
    n_f = int(ok.sum())
    r = ranks(F, ok)
    vol = lambda c: int(np.prod([n_f - int(x) for x in r[c]]))
    picks, gains = [], []
    for _ in range(q):
        best = None
        for c in level:
            if c in picks:
                continue
            gain = vol(c) - hv(np.maximum(r[c][None, :], r[picks]), n_f)
            cand = (gain, int(do[c]), -c)
            if best is None or cand > best:
                best = cand
        picks.append(-best[2])
        gains.append(best[0])
    keys = keys.copy()
    rest = [c for c in level if c not in picks]
    keys[picks + rest] = a + np.arange(len(level))
    out.update(keys=keys, picked=np.asarray(picks, dtype=np.int64), gains=gains, straddles=True)
    return out


# -- the cases both test files run ---------------------------------------------

SIZES = [(n, k) for n in (2, 3, 65, 300) for k in (1, 5, 25) if k < n]
# uniform rows: the first seed at which a level straddles n_select (found on the CPU; asserted by the tests)
SEEDS = {(n, k, M): 0 for n, k in SIZES for M in (2, 3)}
SEEDS.update({(65, 5, 2): 2, (65, 25, 2): 3, (65, 25, 3): 1})


def antichain(n, M, seed):
    """n mutually non-dominated rows in random order: points on sum(f) =
    const.  M = 3: most rows near the middles of the triangle's edges (small
    on one axis only), a few at its centre -- those have about n / 3 rows
    below them on every axis, so boxes of (2 n / 3)^3 cells: more than 2^32
    at n = 3000."""
    rng = np.random.RandomState(seed)
    if M == 2:
        x = rng.permutation(n).astype(float)
        return np.stack([x, n - x], axis=1)
    small, t = rng.uniform(0, 0.2, n), rng.uniform(0.45, 0.55, n)
    u = np.stack([small, (1 - small) * t, (1 - small) * (1 - t)], axis=1)
    u = np.stack([np.roll(u[i], i % 3) for i in range(n)])
    u[:n // 30] = rng.dirichlet([300, 300, 300], n // 30)
    return u[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def case(name, M):
    """(F, G or None, n_select) of a named case."""
    rng = np.random.RandomState(1000 + M)
    if name.startswith('uniform'):
        n, k = (int(x) for x in name.split('-')[1:])
        return np.random.RandomState(SEEDS[n, k, M]).uniform(size=(n, M)), None, k
    if name == 'quantized':                  # equal ranks, duplicate rows, zero gains, ties on do and row
        return rng.randint(0, 4, (120, M)).astype(float), None, 12
    if name == 'special':                    # a column of -0.0, 0.0 and +-inf; NaN rows
        F = np.random.RandomState(40 + M).randint(0, 5, (90, M)).astype(float)
        F[:, 0] = rng.choice([-0.0, 0.0, np.inf, -np.inf, 1.0, -1.0], 90)
        F[:, 1] = -F[:, 0] + rng.choice([0.0, -0.0, 1.0], 90)
        F[rng.choice(90, 6, replace=False), M - 1] = np.nan
        return F, None, 4
    if name == 'second-level':               # a front smaller than n_select: the level is not the front
        F = rng.uniform(size=(60, M))
        F[:3] = np.eye(3)[:, :M] * 0.01 - 1.0 if M == 3 else [(-1.0, -0.99), (-0.99, -1.0), (-0.98, -1.01)]
        return F, None, 6
    if name == 'between-levels':             # the boundary between two levels: the keys stay
        F = rng.uniform(size=(60, M))
        k = int((R.counts(F)[0] == 0).sum())
        return F, None, k
    if name == 'none':
        return rng.uniform(size=(40, M)), None, 0
    if name == 'all':                        # n_select = the rows with a key
        F = rng.uniform(size=(40, M))
        F[7, 0] = np.nan
        return F, None, 39
    if name == 'wide':                       # wider than the workgroup; boxes of more than 2^32 cells
        return antichain(3000, 3, 5), None, 8
    if name == 'limit':                      # 64 picks: P's LDS limit, the sorted insert at every position
        return antichain(200, 2, 6), None, 64
    if name == 'constrained':                # ranks and n_f among the feasible rows
        F = rng.uniform(size=(150, M))
        return F, rng.uniform(size=(150, 2)) - 0.7, 9
    if name == 'infeasible-level':           # the boundary inside an equal-violation infeasible level
        F = rng.uniform(size=(30, M))
        G = np.where(np.arange(30)[:, None] < 4, -1.0, 2.0) * np.ones((30, 1))
        return F, G, 10
    raise KeyError(name)


NAMED = ('quantized', 'special', 'second-level', 'between-levels', 'none', 'all', 'constrained',
         'infeasible-level')
STAY = ('between-levels', 'none', 'all', 'infeasible-level')       # the keys are the old keys, nothing is picked
CASES = [('uniform-%d-%d' % s, M) for s in SIZES for M in (2, 3)] + [(c, M) for c in NAMED for M in (2, 3)] + [
    ('wide', 3), ('limit', 2)]


@functools.lru_cache(maxsize=None)
def expected(name, M):
    F, G, k = case(name, M)
    return select(F, k, G)
