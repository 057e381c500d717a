"""Plain statement of the sampled hypervolume tie-break (tpe_mo_keys_hvs,
posterior.mo_keys(..., tiebreak='hypervolume_mc')) in Python loops and Python
ints, on the (by, do) order of tests/mo_reference.py and
tests/moc_reference.py and the ranks of tests/mo_hv_reference.py.  The Philox
words are the oracle's.  It is the yardstick: nothing here calls the code
under test."""
import functools

import numpy as np

from oracle.draw_oracle import philox4x32_10
from tests import mo_hv_reference as H
from tests import mo_reference as R
from tests import moc_reference as RC

STREAM = 0x7FFFFFBE
KEY = (0x4D4F4856, 0x53414D50)


def points(lo, n_f, S):
    """x[s][m] = lo[m] + (word * (n_f - lo[m]) >> 32), word = word m % 4 of the
    counter (s, m // 4, 0, STREAM)."""
    blocks = [[w.tolist() for w in philox4x32_10((np.arange(S), b, 0, STREAM), KEY)]
              for b in range((len(lo) + 3) // 4)]
    return [[lo[m] + ((int(blocks[m // 4][m % 4][s]) * (n_f - lo[m])) >> 32) for m in range(len(lo))]
            for s in range(S)]


def select(F, n_select, S, G=None):
    """dict(keys, by, do, picked, gains, straddles, level, box): the rule,
    start to end; box = the samples inside the first pick's box."""
    F = np.asarray(F, dtype=np.float64)
    if G is None:
        by, do = R.counts(F)
        ok = ~np.isnan(F).any(axis=1)
    else:
        by, do, v = RC.counts(F, G)
        ok = v == 0.0
    keys = RC.order_keys(by, do)
    out = dict(keys=keys, by=by, do=do, picked=[], gains=[], straddles=False, level=0, box=None)
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
    n_f, M = int(ok.sum()), F.shape[1]
    r = H.ranks(F, ok).tolist()
    lo = [min(r[c][m] for c in level) for m in range(M)]
    x = points(lo, n_f, S)
    mask = {}
    for c in level:
        bits = 0
        for j in range(S):
            if all(r[c][m] <= x[j][m] for m in range(M)):
                bits |= 1 << j
        mask[c] = bits
    picks, gains, covered = [], [], 0
    for _ in range(q):
        best = max((bin(mask[c] & ~covered).count('1'), int(do[c]), -c) for c in level if c not in picks)
        picks.append(-best[2])
        gains.append(best[0])
        covered |= mask[picks[-1]]
    keys = keys.copy()
    keys[picks + [c for c in level if c not in picks]] = a + np.arange(len(level))
    out.update(keys=keys, picked=picks, gains=gains, straddles=True, level=len(level),
               box=bin(mask[picks[0]]).count('1'))
    return out


# -- the cases both test files run ---------------------------------------------

# name: (rows, M, seed, n_select, samples, the level's size) -- integer rows randint(0, 40); the seeds at
# which the level that straddles n_select has that size were found on the CPU and are asserted by the tests
SIZED = {
    'two': (300, 2, 1, 1, 64, 2),
    'planar': (300, 2, 2, 1, 64 * 65, 4),
    'one-block': (200, 4, 0, 5, 64 * 65, 28),
    'below-tile': (67, 8, 4, 5, 64 * 65, 63),
    'tile': (172, 5, 4, 25, 64 * 65, 64),
    'above-tile': (69, 8, 4, 64, 128, 65),
    'wide-ties': (443, 8, 0, 25, 64, 300),
    'wide': (443, 8, 0, 5, 128, 300),
}
NAMED = ('special', 'second-level', 'between-levels', 'none', 'all', 'constrained', 'infeasible-level')
STAY = ('between-levels', 'none', 'all', 'infeasible-level')       # the keys are the old keys, nothing is picked
CASES = tuple(SIZED) + NAMED


@functools.lru_cache(maxsize=None)
def case(name):
    """(F, G or None, n_select, samples) of a named case; the named edge cases
    have four objectives and 128 samples."""
    if name in SIZED:
        n, M, seed, k, S, _ = SIZED[name]
        return np.random.RandomState(seed).randint(0, 40, (n, M)).astype(float), None, k, S
    rng, M, S = np.random.RandomState(1004), 4, 128
    if name == 'special':                    # a column of -0.0, 0.0 and +-inf; NaN rows
        F = np.random.RandomState(44).randint(0, 5, (90, M)).astype(float)
        F[:, 0] = rng.choice([-0.0, 0.0, np.inf, -np.inf, 1.0, -1.0], 90)
        F[:, 1] = -F[:, 0] + rng.choice([0.0, -0.0, 1.0], 90)
        F[rng.choice(90, 6, replace=False), M - 1] = np.nan
        return F, None, 4, S
    if name == 'second-level':               # a front smaller than n_select: the level is not the front
        F = rng.uniform(size=(60, M))
        F[:3] = np.eye(3, M) * 0.01 - 1.0
        return F, None, 6, S
    if name == 'between-levels':             # the boundary between two levels: the keys stay
        F = rng.uniform(size=(60, M))
        return F, None, int((R.counts(F)[0] == 0).sum()), S
    if name == 'none':
        return rng.uniform(size=(40, M)), None, 0, S
    if name == 'all':                        # n_select = the rows with a key
        F = rng.uniform(size=(40, M))
        F[7, 0] = np.nan
        return F, None, 39, S
    if name == 'constrained':                # ranks and n_f among the feasible rows
        return rng.uniform(size=(150, M)), rng.uniform(size=(150, 2)) - 0.7, 9, S
    if name == 'infeasible-level':           # the boundary inside an equal-violation infeasible level
        G = np.where(np.arange(30)[:, None] < 4, -1.0, 2.0) * np.ones((30, 1))
        return rng.uniform(size=(30, M)), G, 10, S
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    F, G, k, S = case(name)
    return select(F, k, S, G)
