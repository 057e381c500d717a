"""Timings of the multi-objective keys (Engine.mo_keys; needs the GPU).

    python tools/time_mo.py --gpus 1 [--reps 20] [--host-max-n 10000] [--out FILE]
    python tools/time_mo.py --gpus 1 --quality [--out FILE]
    python tools/time_mo.py --gpus 1 --constraints K [--out FILE]
    python tools/time_mo.py --gpus 1 --quality-constrained [--evals 100] [--out FILE]

* Engine.mo_keys (tpe_mo_keys: upload, all-pairs kernel, pack, radix sort,
  scatter, read-back; one synchronisation) at n in {1000, 10000, 50000} x M in
  {2, 4} uniform rows: wall time around the call, which ends in its stream
  synchronisation -- median of --reps calls after a warm-up call, with the
  smallest and the largest;
* posterior.mo_keys, the chunked numpy builder, on the same inputs up to
  --host-max-n rows (three calls; 50000 rows take minutes of comparisons and
  are left out by default), and whether both give the same keys;
* the crossover: both builders at n = 16 .. 4096, M = 2; the smallest n from
  which the kernel is the faster one at every larger size measured -- what
  tpe.MO_DEVICE_MIN_TRIALS is set from;
* a whole tpe.suggest step on the config-3 history (workloads.mixed_history:
  32 labels x 10000 trials, a second objective 'cost' in every result), with
  objectives=('loss', 'cost') and without, the two alternating on the same
  trials and engine, default posterior_builder; and the key call alone on the
  step's own rows, to say whether the step costs the plain step plus one key
  call.

--quality (reported, not asserted): the hypervolume dominated after 200
evaluations of a two-objective toy problem (ZDT1 in four dimensions, reference
point (1.1, 6)), for tpe.suggest(objectives=('loss', 'cost')), for tpe.suggest
on loss + cost and for rand.suggest, over 10 seeds.

--constraints K (tpe.suggest(constraints=...), K constraint columns):
* Engine.mo_keys(F, G=G) against Engine.mo_keys(F) on the same F, the two
  alternating in one process, at n in {1000, 10000, 50000} x 2 objectives, G =
  uniform - 0.6 (about a third of the rows feasible at K = 2); the host builder
  posterior.mo_keys(F, G=G) up to --host-max-n rows;
* the crossover with constraints at 64, 128 and 512 rows, both builders;
* a whole tpe.suggest step on the config-3 history with objectives=('loss',
  'cost') and with K constraints as well, alternating; and tpe.objective_rows
  alone with and without the constraint columns -- the share of the difference
  that is the host reading K more columns.

--quality-constrained (reported, not asserted): minimise (x - 1)^2 + (y - 1)^2
on [0, 1]^2 under c = x + y - 1 <= 0 (the optimum 0.5 lies on the boundary);
the best feasible loss after --evals evaluations over --seeds seeds for
tpe.suggest(constraints=('c',)), for tpe.suggest on loss + 10 max(c, 0) and for
rand.suggest.

Results are appended to --out as one JSON object per line."""
import argparse
import json
import os
import sys
import time
from functools import partial

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (1000, 10000, 50000)
OBJECTIVES = (2, 4)
CROSS = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)


def timed(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def key_times(eng, args):
    from hyperopt_amd import posterior as P
    out = []
    for n in SIZES:
        for M in OBJECTIVES:
            F = np.random.RandomState(n + M).uniform(size=(n, M))
            rec = dict(what='mo_keys', n=n, M=M, pair_tests=n * n, device=timed(lambda: eng.mo_keys(F), args.reps))
            if n <= args.host_max_n:
                rec['host'] = timed(lambda: P.mo_keys(F), 3)
                rec['same_keys'] = bool(np.array_equal(P.mo_keys(F), eng.mo_keys(F)))
                rec['host_over_device'] = rec['host']['median_ms'] / rec['device']['median_ms']
            else:
                rec['host'] = 'not measured'
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def crossover(eng, args):
    from hyperopt_amd import posterior as P
    rec = dict(what='mo_crossover', M=2, sizes={})
    for n in CROSS:
        F = np.random.RandomState(n).uniform(size=(n, 2))
        d = timed(lambda: eng.mo_keys(F), args.reps)['median_ms']
        h = timed(lambda: P.mo_keys(F), max(3, args.reps // 4))['median_ms']
        rec['sizes'][n] = dict(device_ms=d, host_ms=h)
    faster = [n for n in CROSS if rec['sizes'][n]['device_ms'] <= rec['sizes'][n]['host_ms']]
    first = None
    for n in reversed(CROSS):          # the smallest n with the kernel faster from there on
        if n not in faster:
            break
        first = n
    rec['device_faster_from'] = first
    print(json.dumps(rec), flush=True)
    return [rec]


def step_times(args):
    from hyperopt_amd import engine as E, tpe, workloads
    from hyperopt_amd.base import Domain
    hist = workloads.mixed_history(32, 10000, seed=0)
    trials = workloads.history_trials(hist)
    cost = np.random.RandomState(1).uniform(size=len(trials.trials))
    for d, c in zip(trials.trials, cost):
        d['result']['cost'] = float(c)
    domain = Domain(lambda d: 0.0, workloads.hp_space(hist.labels))
    n = len(trials.trials)
    legs = dict(plain=lambda: tpe.suggest([n], domain, trials, 3),
                objectives=lambda: tpe.suggest([n], domain, trials, 3, objectives=('loss', 'cost')),
                objectives_host_keys=lambda: tpe.suggest([n], domain, trials, 3, objectives=('loss', 'cost'),
                                                         posterior_builder='host'),
                plain_host=lambda: tpe.suggest([n], domain, trials, 3, posterior_builder='host'))
    ts = {k: [] for k in legs}
    for pair, reps in ((('plain', 'objectives'), args.reps), (('plain_host', 'objectives_host_keys'), 3)):
        for k in pair:
            legs[k]()                  # warm-up
        for _ in range(reps):          # alternating
            for k in pair:
                t0 = time.perf_counter()
                legs[k]()
                ts[k].append((time.perf_counter() - t0) * 1e3)
    rec = dict(what='mo_step', labels=32, trials=n, min_trials_for_device_keys=tpe.MO_DEVICE_MIN_TRIALS)
    for k, v in ts.items():
        rec[k] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), reps=len(v))
    # the parts of the keyword on the step's own rows
    docs, F = tpe.objective_rows(trials.trials, ('loss', 'cost'), domain)
    eng = E.get_engine(0, 'f64')
    rec['rows_ms'] = timed(lambda: tpe.objective_rows(trials.trials, ('loss', 'cost'), domain), args.reps)['median_ms']
    rec['key_call_ms'] = timed(lambda: eng.mo_keys(F), args.reps)['median_ms']
    keys = eng.mo_keys(F)
    src = trials.trials
    rec['keyed_domain_ms'] = timed(lambda: tpe._KeyedDomain(domain, docs, keys, src).loss_column(src),
                                   args.reps)['median_ms']
    rec['step_minus_plain_ms'] = rec['objectives']['median_ms'] - rec['plain']['median_ms']
    print(json.dumps(rec), flush=True)
    return [rec]


def constrained_key_times(eng, args):
    from hyperopt_amd import posterior as P
    K, out = args.constraints, []
    for n in SIZES:
        rng = np.random.RandomState(n + 2)
        F = rng.uniform(size=(n, 2))
        G = rng.uniform(size=(n, K)) - 0.6
        legs = dict(unconstrained=lambda: eng.mo_keys(F), constrained=lambda: eng.mo_keys(F, G=G))
        ts = {k: [] for k in legs}
        for k in legs:
            legs[k]()                  # warm-up
        for _ in range(args.reps):     # alternating
            for k in legs:
                t0 = time.perf_counter()
                legs[k]()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        rec = dict(what='mo_keys_constrained', n=n, M=2, K=K,
                   feasible=int(np.count_nonzero(P.mo_violation(G, F) == 0.0)))
        for k, v in ts.items():
            rec[k] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), reps=len(v))
        rec['constrained_over_unconstrained'] = rec['constrained']['median_ms'] / rec['unconstrained']['median_ms']
        if n <= args.host_max_n:
            rec['host'] = timed(lambda: P.mo_keys(F, G=G), 3)
            rec['same_keys'] = bool(np.array_equal(P.mo_keys(F, G=G), eng.mo_keys(F, G=G)))
        else:
            rec['host'] = 'not measured'
        print(json.dumps(rec), flush=True)
        out.append(rec)
    rec = dict(what='mo_crossover_constrained', M=2, K=K, sizes={})
    for n in (64, 128, 512):
        rng = np.random.RandomState(n)
        F = rng.uniform(size=(n, 2))
        G = rng.uniform(size=(n, K)) - 0.6
        rec['sizes'][n] = dict(device_ms=timed(lambda: eng.mo_keys(F, G=G), args.reps)['median_ms'],
                               host_ms=timed(lambda: P.mo_keys(F, G=G), args.reps)['median_ms'])
    print(json.dumps(rec), flush=True)
    return out + [rec]


def constrained_step_times(args):
    from hyperopt_amd import tpe, workloads
    from hyperopt_amd.base import Domain
    K = args.constraints
    names = tuple('c%d' % k for k in range(K))
    hist = workloads.mixed_history(32, 10000, seed=0)
    trials = workloads.history_trials(hist)
    rng = np.random.RandomState(1)
    cost = rng.uniform(size=len(trials.trials))
    G = rng.uniform(size=(len(trials.trials), K)) - 0.6
    for d, c, g in zip(trials.trials, cost, G):
        d['result']['cost'] = float(c)
        d['result'].update(zip(names, map(float, g)))
    domain = Domain(lambda d: 0.0, workloads.hp_space(hist.labels))
    n = len(trials.trials)
    legs = dict(objectives=lambda: tpe.suggest([n], domain, trials, 3, objectives=('loss', 'cost')),
                objectives_and_constraints=lambda: tpe.suggest([n], domain, trials, 3, objectives=('loss', 'cost'),
                                                               constraints=names))
    ts = {k: [] for k in legs}
    for k in legs:
        legs[k]()                      # warm-up
    for _ in range(args.reps):         # alternating
        for k in legs:
            t0 = time.perf_counter()
            legs[k]()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    rec = dict(what='mo_step_constrained', labels=32, trials=n, K=K)
    for k, v in ts.items():
        rec[k] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), reps=len(v))
    rows = dict(rows_ms=lambda: tpe.objective_rows(trials.trials, ('loss', 'cost'), domain),
                rows_with_constraints_ms=lambda: tpe.objective_rows(trials.trials, ('loss', 'cost'), domain,
                                                                    constraints=names))
    tr = {k: [] for k in rows}
    for _ in range(args.reps + 1):     # alternating; the first pair is the warm-up
        for k in rows:
            t0 = time.perf_counter()
            rows[k]()
            tr[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in tr.items():
        rec[k] = float(np.median(v[1:]))
    rec['step_difference_ms'] = rec['objectives_and_constraints']['median_ms'] - rec['objectives']['median_ms']
    rec['rows_difference_ms'] = rec['rows_with_constraints_ms'] - rec['rows_ms']
    print(json.dumps(rec), flush=True)
    return [rec]


def quality_constrained(args):
    from hyperopt_amd import STATUS_OK, Trials, fmin, hp, rand, tpe
    space = {'x': hp.uniform('x', 0, 1), 'y': hp.uniform('y', 0, 1)}

    def parts(cfg):
        return (cfg['x'] - 1) ** 2 + (cfg['y'] - 1) ** 2, cfg['x'] + cfg['y'] - 1

    def constrained(cfg):
        f, c = parts(cfg)
        return {'loss': f, 'f': f, 'c': c, 'status': STATUS_OK}

    def penalised(cfg):
        f, c = parts(cfg)
        return {'loss': f + 10.0 * max(c, 0.0), 'f': f, 'c': c, 'status': STATUS_OK}
    algos = dict(constraints=(constrained, partial(tpe.suggest, constraints=('c',))),
                 tpe_on_the_penalty=(penalised, tpe.suggest), random=(constrained, rand.suggest))
    rec = dict(what='mo_quality_constrained', problem='(x-1)^2 + (y-1)^2 under x + y <= 1, optimum 0.5',
               evaluations=args.evals, seeds=args.seeds)
    for name, (fn, algo) in algos.items():
        best, feasible = [], []
        for seed in range(args.seeds):
            trials = Trials()
            fmin(fn, space, algo=algo, max_evals=args.evals, trials=trials, rstate=np.random.RandomState(seed))
            ok = [d['result']['f'] for d in trials.trials if d['result']['c'] <= 0]
            feasible.append(len(ok))
            best.append(min(ok) if ok else float('nan'))
        rec[name] = dict(mean=float(np.nanmean(best)), std=float(np.nanstd(best)), min=float(np.nanmin(best)),
                         max=float(np.nanmax(best)), feasible_trials_mean=float(np.mean(feasible)),
                         runs_without_a_feasible_trial=int(np.isnan(best).sum()))
    print(json.dumps(rec), flush=True)
    return [rec]


def hypervolume(F, ref):
    """The area dominated by the rows of F [n, 2] inside the box below `ref`."""
    F = F[(F < ref).all(axis=1)]
    if not len(F):
        return 0.0
    F = F[np.lexsort((F[:, 1], F[:, 0]))]
    area, low = 0.0, ref[1]
    for f1, f2 in F:
        if f2 < low:
            area += (ref[0] - f1) * (low - f2)
            low = f2
    return float(area)


def quality(args):
    from hyperopt_amd import STATUS_OK, Trials, fmin, hp, rand, tpe
    space = {'x%d' % i: hp.uniform('x%d' % i, 0, 1) for i in range(4)}
    ref = np.array([1.1, 6.0])

    def zdt1(cfg):
        f1 = cfg['x0']
        g = 1.0 + 9.0 * (cfg['x1'] + cfg['x2'] + cfg['x3']) / 3.0
        return f1, g * (1.0 - np.sqrt(f1 / g))

    def both(cfg):
        f1, f2 = zdt1(cfg)
        return {'loss': f1, 'cost': f2, 'status': STATUS_OK}

    def summed(cfg):
        f1, f2 = zdt1(cfg)
        return {'loss': f1 + f2, 'f1': f1, 'cost': f2, 'status': STATUS_OK}
    algos = dict(objectives=(both, partial(tpe.suggest, objectives=('loss', 'cost')), 'loss'),
                 tpe_on_the_sum=(summed, tpe.suggest, 'f1'), random=(both, rand.suggest, 'loss'))
    rec = dict(what='mo_quality', problem='ZDT1, 4 dimensions', evaluations=args.evals, reference_point=ref.tolist(),
               seeds=args.seeds)
    for name, (fn, algo, first) in algos.items():
        hv = []
        for seed in range(args.seeds):
            trials = Trials()
            fmin(fn, space, algo=algo, max_evals=args.evals, trials=trials, rstate=np.random.RandomState(seed))
            F = np.array([(d['result'][first], d['result']['cost']) for d in trials.trials])
            hv.append(hypervolume(F, ref))
        rec[name] = dict(mean=float(np.mean(hv)), min=float(min(hv)), max=float(max(hv)),
                         std=float(np.std(hv)))
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-max-n', type=int, default=10000)
    ap.add_argument('--quality', action='store_true')
    ap.add_argument('--constraints', type=int, default=0, metavar='K')
    ap.add_argument('--quality-constrained', action='store_true')
    ap.add_argument('--evals', type=int)
    ap.add_argument('--seeds', type=int, default=10)
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.gpus != 1:
        ap.error('the keys are computed on one device: --gpus 1')
    if args.evals is None:
        args.evals = 100 if args.quality_constrained else 200
    if args.constraints and not 1 <= args.constraints <= 8:
        ap.error('--constraints: 1 to 8 columns')
    if args.quality_constrained:
        recs = quality_constrained(args)
    elif args.constraints:
        from hyperopt_amd.engine import Engine
        eng = Engine(0, 'f64')
        recs = constrained_key_times(eng, args)
        eng.close()
        recs += constrained_step_times(args)
    elif args.quality:
        recs = quality(args)
    else:
        from hyperopt_amd.engine import Engine
        eng = Engine(0, 'f64')
        recs = key_times(eng, args) + crossover(eng, args)
        eng.close()
        recs += step_times(args)
    if args.out:
        with open(args.out, 'a') as f:
            for r in recs:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
