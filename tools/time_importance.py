"""Timings of the hyperparameter importance (tpe.importance; needs the GPU).

    python tools/time_importance.py --gpus 1 [--configs 3,5] [--n-grid 4096] [--reps 10] [--out FILE]

On the histories of config 3 (workloads.mixed_history: 32 labels x 10000
trials) and config 5 (128 labels x 50000 trials), quantile 0.1:

* tpe.importance end to end on a Trials object holding the history (wall:
  the gather, the split, every label's mixtures on the host, the upload, the
  device call; median of --reps calls after a warm-up call -- the history
  cache is warm, as it is in a running study);
* Engine.importance alone on the posterior that call left resident (wall,
  cells uploaded, one synchronisation, v read back);
* the alternative without the new kernels: the cells as a pool (Engine.pool_set
  once, timed apart), Engine.pool_rank(want_terms=True) for the planes and
  the per-cell arithmetic in numpy -- possible here because no label of these
  spaces needs merged cells;
* the numpy reference: the oracle's lpdfs at the cells and the same
  arithmetic, on the first --host-labels labels (one of each kind of the
  space's cycle), scaled to all labels by the label count.

One JSON object per config is printed; --out is written anew by every run, one
line per config of that run (profiles/importance_timing.json: --configs 3,5)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUANTILE = 0.1


def timed(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def terms(lb, la, w, alpha):
    """The per-cell arithmetic of tpe_importance, vectorised."""
    with np.errstate(invalid='ignore', over='ignore'):
        d = lb - la
        om = 1.0 - alpha
        t = np.expm1(-np.abs(d))
        dev = np.where(d <= 0, alpha * om * t / (1.0 + alpha * t), -(alpha * om * t) / (1.0 + om * t))
        p = alpha * np.exp(lb) + om * np.exp(la)
        out = w * p * (dev * dev)
    return np.where((lb == -np.inf) & (la == -np.inf), 0.0, out)


def inputs(hist, n_grid):
    """(posteriors, cells, alpha) of every label, as tpe.importance forms them."""
    from hyperopt_amd import posterior as P
    n = len(hist.tids)
    sp = P.Splitter(hist.tids, hist.losses, 0.0, n_below=int(np.ceil(QUANTILE * n)))
    posts, cells, alpha = [], [], []
    for name, kind, args in hist.labels:
        oi, ov = hist.obs[name]
        b, a = sp.split(oi, ov)
        posts.append(P.label_posterior(name, kind, args, b, a, 1.0))
        cells.append(P.importance_cells(kind, args, ov, n_grid))
        alpha.append(len(b) / (len(b) + len(a)))
    return posts, cells, alpha


def host_reference(posts, cells, alpha, labels):
    from oracle import tpe_oracle as O
    out = []
    for li in labels:
        p, (x, w, merge) = posts[li], cells[li]
        if p.family == 'categorical':
            lb, la = O.categorical_lpdf(x, p.below), O.categorical_lpdf(x, p.above)
        else:
            f = O.gmm1_lpdf if p.family == 'GMM1' else O.lgmm1_lpdf
            q = None if p.q is None else merge * p.q
            lb = f(x, *p.below, low=p.low, high=p.high, q=q)
            la = f(x, *p.above, low=p.low, high=p.high, q=q)
        out.append(float(np.sum(terms(lb, la, w, alpha[li]))))
    return out


def run(n_labels, n_trials, args):
    from hyperopt_amd import Domain, tpe
    from hyperopt_amd.engine import Engine, get_engine
    from hyperopt_amd.workloads import history_trials, hp_space, mixed_history
    hist = mixed_history(n_labels, n_trials, seed=0)
    rec = dict(what='importance', labels=n_labels, trials=n_trials, n_grid=args.n_grid, quantile=QUANTILE)
    t0 = time.perf_counter()
    trials = history_trials(hist)
    domain = Domain(None, hp_space(hist.labels))
    rec['make_trials_s'] = time.perf_counter() - t0
    names = list(tpe.specs_of(domain))
    rec['tpe_importance'] = timed(lambda: tpe.importance(domain, trials, quantile=QUANTILE, n_grid=args.n_grid),
                                  args.reps)
    got = tpe.importance(domain, trials, quantile=QUANTILE, n_grid=args.n_grid, normalize=False)
    posts, cells, alpha = inputs(hist, args.n_grid)
    order = [[l[0] for l in hist.labels].index(k) for k in names]   # the engine's label order is the space's
    cells_e, alpha_e = [cells[i] for i in order], [alpha[i] for i in order]
    eng = get_engine(0, 'f64', 'importance')
    L = len(names)
    rec['cells'] = int(sum(len(c[0]) for c in cells))
    rec['components'] = int(sum(len(p.below[0]) + len(p.above[0]) if p.family != 'categorical' else 0 for p in posts))
    rec['engine_importance'] = timed(lambda: eng.importance(range(L), cells_e, alpha_e), args.reps)
    rec['engine_importance_planes'] = timed(lambda: eng.importance(range(L), cells_e, alpha_e, want_planes=True),
                                            args.reps)
    v = eng.importance(range(L), cells_e, alpha_e)
    rec['same_as_public'] = bool([got[k] for k in names] == v.tolist())   # (every label always active: n_d = n)

    # the alternative: the cells as a pool, the planes from pool_rank, numpy for the rest
    assert all(c[2] == 1 for c in cells_e)
    rows = max(len(c[0]) for c in cells_e)
    pool = np.full((rows, L), np.nan)
    wts = np.zeros((rows, L))
    for c, (x, w, _) in enumerate(cells_e):
        pool[:len(x), c] = x
        wts[:len(x), c] = w
    alt = Engine(0, 'f64')
    from hyperopt_amd import posterior as P
    alt.set_posterior(*P.pack([posts[i] for i in order]))
    t0 = time.perf_counter()
    alt.pool_set(pool)
    rec['pool_set_ms'] = (time.perf_counter() - t0) * 1e3
    a_row = np.asarray(alpha_e)[None, :]

    def by_pool():
        _, _, lb, la = alt.pool_rank(1, want_terms=True)
        return np.nansum(np.where(np.isnan(pool), 0.0, terms(lb, la, wts, a_row)), axis=0)
    rec['pool_rank_terms_numpy'] = timed(by_pool, args.reps)
    vp = by_pool()
    rec['pool_path_max_rel_diff'] = float(np.max(np.abs(vp - v) / np.maximum(v, 1e-300)))
    alt.close()

    sub = list(range(min(args.host_labels, L)))
    t0 = time.perf_counter()
    ref = host_reference([posts[i] for i in order], cells_e, alpha_e, sub)
    dt = (time.perf_counter() - t0) * 1e3
    rec['host_reference'] = dict(labels=len(sub), ms=dt, ms_scaled_to_all_labels=dt * L / len(sub))
    rec['host_max_rel_diff'] = float(max(abs(r - v[i]) / max(v[i], 1e-300) for i, r in zip(sub, ref)))
    rec['host_over_engine'] = rec['host_reference']['ms_scaled_to_all_labels'] / rec['engine_importance']['median_ms']
    rec['pool_path_over_engine'] = rec['pool_rank_terms_numpy']['median_ms'] / rec['engine_importance']['median_ms']
    top = sorted(got, key=lambda k: -got[k])[:3]
    rec['top3'] = [(k, got[k]) for k in top]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--configs', default='3,5')
    ap.add_argument('--n-grid', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-labels', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    shapes = {3: (32, 10000), 5: (128, 50000)}
    lines = []
    for cfg in (int(c) for c in args.configs.split(',')):
        rec = run(*shapes[cfg], args)
        rec['config'] = cfg
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if args.out:   # (rewritten after every config: a run that is cut short keeps what it has)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
