"""Plain numpy restatement of the draw on a candidate pool (tpe_pool_draw,
tpe.suggest(pool=..., pool_candidates=m)): the Philox words from the draw
oracle, the 52-bit uniform, the Gumbel noise and the keys as the header
defines them, the selection as a sort on (NaN first, key descending, index
ascending), the pick as tests/pool_reference.py's ranking inside the drawn
set.  Nothing here touches the engine."""
import numpy as np

from oracle.draw_oracle import philox4x32_10
from tests import pool_reference as R

TPE_POOL_STREAM = 0x7FFFFFBF


def words(seed, round, index):
    """(w0, w1) of the entries `index` in round `round` under `seed`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    index = np.asarray(index, dtype=np.uint64)
    w = philox4x32_10((index, 0, TPE_POOL_STREAM, int(round) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))
    return w[0], w[1]


def uniform(w0, w1):
    """u = (t + 0.5) 2^-52 with t = (w0 << 20) | (w1 >> 12): exact in fp64, strictly inside (0, 1)."""
    t = (np.asarray(w0, dtype=np.uint64) << np.uint64(20)) | (np.asarray(w1, dtype=np.uint64) >> np.uint64(12))
    return (t.astype(np.float64) + 0.5) * 2.0 ** -52


def gumbel(seed, round, n):
    """G[i] = -log(-log u_i), i in [0, n)."""
    return -np.log(-np.log(uniform(*words(seed, round, np.arange(n)))))


def lsum(values, lb, kinds, groups=()):
    """(lsum, sum |term|) [n]: from 0.0, left to right, the below terms in
    pool_reference.scores' order, each in the label's working space: lb, plus
    log v for a dense log kind; a group's plane plus (from 0.0) the log v of
    its dense log columns in the order it lists them."""
    values = np.asarray(values, dtype=float)
    n, L = values.shape
    log_col = [k in ('loguniform', 'lognormal') for k in kinds]
    covered = set(c for cols, _ in groups for c in cols)
    out, mag = np.zeros(n), np.zeros(n)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(n):
            s, a = 0.0, 0.0
            for c in range(L):
                if c in covered or values[i, c] != values[i, c]:
                    continue
                term = lb[i, c]
                if log_col[c]:
                    term = term + np.log(values[i, c])
                s, a = s + term, a + abs(term)
            for cols, at in groups:
                if any(values[i, c] != values[i, c] for c in cols):
                    continue
                jac = 0.0
                for c in cols:
                    if log_col[c]:
                        jac = jac + np.log(values[i, c])
                term = lb[i, at] + jac
                s, a = s + term, a + abs(term)
            out[i], mag[i] = s, a
    return out, mag


def select(keys, d, free):
    """The d entries of `free` first in the order: key descending (NaN greatest), then index ascending."""
    free = set(free)
    return R.rank(keys, d, taken=[i for i in range(len(keys)) if i not in free])


def draw(keys, score, m, taken=(), distinct=True):
    """(best, drawn) of the rounds whose keys are the rows of `keys`: the rounds
    in order, ending at the first one with nothing free."""
    keys = np.atleast_2d(np.asarray(keys, dtype=float))
    n = keys.shape[1]
    out_of = set(int(t) for t in taken if 0 <= int(t) < n)
    best, drawn = [], []
    for k in keys:
        free = [i for i in range(n) if i not in out_of]
        if not free:
            break
        d = select(k, min(int(m), len(free)), free)
        b = int(R.rank(score, 1, taken=set(range(n)) - set(d.tolist()))[0])
        best.append(b)
        drawn.append(d)
        if distinct:
            out_of.add(b)
    return np.asarray(best, dtype=np.int64), drawn
