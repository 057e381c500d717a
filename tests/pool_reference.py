"""Plain numpy restatement of the candidate-pool ranking (tpe_pool_rank,
tpe.suggest(pool=...)): per-label lpdfs from the CPU oracle, the score as a
Python left-to-right loop, the ranking as a sort on (NaN first, score
descending, index ascending).  Nothing here touches the engine."""
import numpy as np

from oracle import tpe_oracle as O


def oracle_planes(hist, values, gamma=0.25, prior_weight=1.0):
    """(lb, la) [n, L] of a pool `values` under the oracle's posteriors of the
    history `hist` (tests.helpers.make_history): NaN where a cell is NaN."""
    values = np.asarray(values, dtype=float)
    lb = np.full(values.shape, np.nan)
    la = np.full(values.shape, np.nan)
    for c, (name, kind, args) in enumerate(hist.labels):
        oi, ov = hist.obs[name]
        r = O.label_posteriors(kind, args, oi, ov, hist.tids, hist.losses, gamma, prior_weight)
        act = ~np.isnan(values[:, c])
        if not act.any():
            continue
        if r[0] == 'CAT':
            lb[act, c] = O.categorical_lpdf(values[act, c], r[1])
            la[act, c] = O.categorical_lpdf(values[act, c], r[2])
        else:
            lb[act, c], la[act, c] = O.score_candidates(r[0], r[1], values[act, c])
    return lb, la


def posterior_planes(posts, values):
    """(lb, la) [n, L] under a list of hyperopt_amd.posterior.LabelPosterior
    (tpe.build_posteriors), through the oracle's lpdf functions."""
    values = np.asarray(values, dtype=float)
    lb = np.full(values.shape, np.nan)
    la = np.full(values.shape, np.nan)
    for c, p in enumerate(posts):
        act = ~np.isnan(values[:, c])
        if not act.any():
            continue
        v = values[act, c]
        if p.family == 'categorical':
            lb[act, c] = O.categorical_lpdf(v, p.below)
            la[act, c] = O.categorical_lpdf(v, p.above)
            continue
        f = O.gmm1_lpdf if p.family == 'GMM1' else O.lgmm1_lpdf
        lb[act, c] = f(v, *p.below, low=p.low, high=p.high, q=p.q)
        la[act, c] = f(v, *p.above, low=p.low, high=p.high, q=p.q)
    return lb, la


def scores(values, lb, la, groups=()):
    """score[i]: from 0.0, left to right, lb - la of the uncovered non-NaN
    cells of row i in ascending column order, then of the listed groups
    [(columns, plane column)] in the order listed -- a group counts when none
    of its columns is NaN."""
    values = np.asarray(values, dtype=float)
    n, L = values.shape
    covered = set(c for cols, _ in groups for c in cols)
    out = np.zeros(n)
    for i in range(n):
        s = 0.0
        for c in range(L):
            if c in covered or values[i, c] != values[i, c]:
                continue
            with np.errstate(invalid='ignore'):
                s = s + (lb[i, c] - la[i, c])
        for cols, at in groups:
            if any(values[i, c] != values[i, c] for c in cols):
                continue
            with np.errstate(invalid='ignore'):
                s = s + (lb[i, at] - la[i, at])
        out[i] = s
    return out


def rank(score, k, taken=()):
    """Indices of the k best entries not in `taken`: NaN greatest, then the
    larger score, then the lowest index (broadcast_best's order)."""
    score = np.asarray(score, dtype=float)
    out_of = set(int(t) for t in taken)
    free = [i for i in range(len(score)) if i not in out_of]
    key = lambda i: (0 if score[i] != score[i] else 1, -score[i] if score[i] == score[i] else 0.0, i)
    return np.asarray(sorted(free, key=key)[:max(int(k), 0)], dtype=np.int64)
