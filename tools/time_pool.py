"""Timings of the candidate-pool ranking (Engine.pool_rank; needs the GPU).

    python tools/time_pool.py --gpus 1 [--sizes 17,20] [--reps 20] [--out FILE]
    python tools/time_pool.py --gpus 1 --draw 24 [--sizes 17,20] [--reps 20] [--out FILE]
    python tools/time_pool.py --gpus 1 --explore 24 [--seeds 20] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \\
        python tools/time_pool.py --gpus 1 --trace-leg [--sizes 17]
    python tools/time_pool.py --kernel-stats DIR/.../run_kernel_stats.csv --sizes 17 --out FILE

On the config-3 history (workloads.mixed_history: 32 labels x 10000 trials,
posterior built on the device) and pools of 2^17 and 2^20 prior draws:

* the one-time Engine.pool_set (wall);
* Engine.pool_rank at k = 1 and k = 64: wall time, median of --reps calls
  after a warm-up call, with the smallest and the largest;
* what a caller can do without the pool: Engine.score per label on the
  label's column (one upload, one round and one read-back each), the
  left-to-right sum and np.argpartition in numpy -- the same medians; the
  two rankings' best entry is compared.

--trace-leg: three pool_rank calls and one Engine.score per dense label on one
pool, nothing timed -- the run to put under rocprofv3 --kernel-trace --stats.
--kernel-stats: reads that run's kernel table and records, for the dense
labels, the (entry, component) terms per second of k_pool_dense beside those
of the plain fp64 round on supplied candidates (k_round<double, DENSE_*,
false>, what tpe_score launches): terms = entries x the components of both
mixtures of every dense label, over the kernels' average time per call.

--draw M: Engine.pool_draw (M entries drawn from l per round, the best l/g of
them) at 1 and 8 rounds beside Engine.pool_rank at k = 1 and k = 8 on the same
pools, the same medians, and their differences -- nothing else is run.
--explore M: fmin over a pool of 4096 prior draws of the config-3 space (32
labels, loss = the sum of the labels' bowls, no noise), per seed once with the
ranking (pool_candidates=None) and once with pool_candidates=M: the best loss
after 50, 100 and 200 evaluations, and how many distinct entries two workers
with different seeds propose from the same 100 trials.

Results are appended to --out as one JSON object per line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(n_labels=32, n_trials=10000):
    from hyperopt_amd.engine import Engine
    from hyperopt_amd.workloads import mixed_history
    hist = mixed_history(n_labels, n_trials, seed=0)
    eng = Engine(0, 'f64')
    eng.set_option('timing', 0)
    eng.build_posterior(*hist.device_inputs(), gamma=0.25, prior_weight=1.0)
    return eng, hist


def draw_pool(hist, n, seed=5):
    from hyperopt_amd.workloads import prior_draw
    rng = np.random.RandomState(seed)
    return np.stack([prior_draw(kind, args, rng, n) for _, kind, args in hist.labels], axis=1)


def dense_components(eng, hist):
    """Components of both mixtures over the dense labels, and those labels."""
    from hyperopt_amd.workloads import DENSE_KINDS
    dense = [i for i, (_, kind, _) in enumerate(hist.labels) if kind in DENSE_KINDS]
    return sum(len(eng.get_mixture(i, side)[0]) for i in dense for side in (0, 1)), dense


def timed(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def by_label(eng, cols, k):
    """The ranking without the pool: Engine.score per label, numpy for the rest."""
    total = np.zeros(len(cols[0]))
    for c, col in enumerate(cols):
        lb, la, _ = eng.score(c, col)
        total += lb - la
    top = np.argpartition(-total, k - 1)[:k] if k < len(total) else np.arange(len(total))
    return top[np.argsort(-total[top], kind='stable')], total


def timings(args):
    eng, hist = setup()
    comps, dense = dense_components(eng, hist)
    out = []
    for lg in args.sizes:
        n = 1 << lg
        vals = draw_pool(hist, n)
        cols = [np.ascontiguousarray(vals[:, c]) for c in range(vals.shape[1])]
        t0 = time.perf_counter()
        eng.pool_set(vals)
        rec = dict(what='pool_rank', labels=len(hist.labels), trials=len(hist.tids), n=n,
                   dense_labels=len(dense), dense_components=comps,
                   pool_set_ms=(time.perf_counter() - t0) * 1e3)
        for k in (1, 64):
            rec['pool_rank_k%d' % k] = timed(lambda: eng.pool_rank(k), args.reps)
            rec['score_per_label_k%d' % k] = timed(lambda: by_label(eng, cols, k), args.reps)
        idx, top = eng.pool_rank(64)
        ref, total = by_label(eng, cols, 64)
        rec['same_best'] = bool(idx[0] == ref[0])
        rec['max_score_diff'] = float(np.max(np.abs(top - total[idx])))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    eng.close()
    return out


def draw_timings(args):
    eng, hist = setup()
    out = []
    for lg in args.sizes:
        n = 1 << lg
        eng.pool_set(draw_pool(hist, n))
        rec = dict(what='pool_draw', labels=len(hist.labels), trials=len(hist.tids), n=n, m=args.draw)
        for k in (1, 8):
            rounds = list(range(100, 100 + k))
            rec['pool_rank_k%d' % k] = timed(lambda: eng.pool_rank(k), args.reps)
            rec['pool_draw_r%d' % k] = timed(lambda: eng.pool_draw(7, rounds, args.draw), args.reps)
            rec['draw_minus_rank_r%d_ms' % k] = (rec['pool_draw_r%d' % k]['median_ms']
                                                 - rec['pool_rank_k%d' % k]['median_ms'])
        # everything drawn: the ranking's entries
        rec['pool_sized_draw_is_rank'] = bool(np.array_equal(eng.pool_draw(7, list(range(8)), n)[0],
                                                             eng.pool_rank(8)[0]))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    eng.close()
    return out


def explore(args):
    from functools import partial
    from hyperopt_amd import Trials, fmin, tpe
    from hyperopt_amd.base import Domain
    from hyperopt_amd.workloads import bowl, hp_space, mixed_space, prior_draw
    labels = mixed_space(32)
    kinds = {name: kind for name, kind, _ in labels}
    space = hp_space(labels)

    def loss(cfg):
        return float(sum(bowl(kinds[k], np.asarray(float(v))) for k, v in cfg.items()))
    rng = np.random.RandomState(5)
    cols = {name: prior_draw(kind, a, rng, 4096) for name, kind, a in labels}
    pts = [{k: (int(v[i]) if kinds[k] == 'randint' else float(v[i])) for k, v in cols.items()} for i in range(4096)]
    domain = Domain(loss, space)
    pool = tpe.Pool(domain, pts)
    marks = (50, 100, 200)
    rec = dict(what='pool_explore', n=len(pool), labels=len(labels), m=args.explore, seeds=args.seeds,
               pool_best=min(loss(p) for p in pts))
    for name, m in (('rank', None), ('draw', args.explore)):
        best = {k: [] for k in marks}
        distinct = []
        for seed in range(args.seeds):
            algo = partial(tpe.suggest, pool=pool, pool_candidates=m)
            trials, rstate = Trials(), np.random.RandomState(seed)
            for k in marks:
                fmin(loss, space, algo=algo, max_evals=k, trials=trials, rstate=rstate)
                best[k].append(min(trials.losses()))
                if k == 100:   # two workers, the same trials, different seeds
                    a = algo([1000], domain, trials, 2 * seed + 1)
                    b = algo([1000], domain, trials, 2 * seed + 2)
                    distinct.append(len({a[0]['misc']['pool_index'], b[0]['misc']['pool_index']}))
        rec[name] = dict(best_loss={str(k): dict(mean=float(np.mean(v)), median=float(np.median(v)),
                                                 min=float(min(v)), max=float(max(v))) for k, v in best.items()},
                         distinct_of_two_workers=float(np.mean(distinct)))
    print(json.dumps(rec), flush=True)
    return [rec]


def trace_leg(args):
    eng, hist = setup()
    _, dense = dense_components(eng, hist)
    n = 1 << args.sizes[0]
    vals = draw_pool(hist, n)
    eng.pool_set(vals)
    for _ in range(3):
        eng.pool_rank(1)
    for c in dense:
        eng.score(c, np.ascontiguousarray(vals[:, c]))
    eng.close()
    return []


def kernel_stats(args):
    import csv
    rows = list(csv.DictReader(open(args.kernel_stats)))
    eng, hist = setup()
    comps, dense = dense_components(eng, hist)
    eng.close()
    n = 1 << args.sizes[0]
    rec = dict(what='pool_kernels', n=n, dense_labels=len(dense), dense_components=comps, kernels={})
    rnd_ns = 0.0
    for r in rows:
        name = r['Name']
        if 'k_pool_' in name or 'k_round<double' in name:
            rec['kernels'][name.replace('(anonymous namespace)::', '')[:80]] = dict(
                calls=int(r['Calls']), avg_ms=float(r['AverageNs']) / 1e6)
        if 'k_pool_dense' in name:
            # one launch covers every dense label
            rec['pool_dense_terms_per_s'] = n * comps / (float(r['AverageNs']) * 1e-9)
        if 'k_round<double, 0, false' in name or 'k_round<double, 1, false' in name:
            rnd_ns += float(r['TotalDurationNs'])
    if rnd_ns:
        # one launch per dense label, each over its own components: all of them together
        rec['round_dense_terms_per_s'] = n * comps / (rnd_ns * 1e-9)
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--sizes', default='17,20', help='log2 of the pool sizes')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--trace-leg', action='store_true')
    ap.add_argument('--kernel-stats')
    ap.add_argument('--draw', type=int, default=0, metavar='M', help='time pool_draw with M drawn per round')
    ap.add_argument('--explore', type=int, default=0, metavar='M', help='fmin over a pool: ranking against pool_candidates=M')
    ap.add_argument('--seeds', type=int, default=20)
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.gpus != 1:
        ap.error('the pool is ranked on one device: --gpus 1')
    args.sizes = [int(s) for s in args.sizes.split(',')]
    recs = (kernel_stats(args) if args.kernel_stats else trace_leg(args) if args.trace_leg
            else draw_timings(args) if args.draw else explore(args) if args.explore else timings(args))
    if args.out:
        with open(args.out, 'a') as f:
            for r in recs:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
