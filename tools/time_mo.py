"""Timings of the multi-objective keys (Engine.mo_keys; needs the GPU).

    python tools/time_mo.py --gpus 1 [--reps 20] [--host-max-n 10000] [--out FILE]
    python tools/time_mo.py --gpus 1 --quality [--out FILE]
    python tools/time_mo.py --gpus 1 --constraints K [--out FILE]
    python tools/time_mo.py --gpus 1 --quality-constrained [--evals 100] [--out FILE]
    python tools/time_mo.py --gpus 1 --density [--out FILE]
    python tools/time_mo.py --gpus 1 --indicator [--indicator-m 4] [--host-max-n 10000] [--out FILE]
    python tools/time_mo.py --gpus 1 --indicator --indicator-method sampled [--indicator-m 8] [--out FILE]

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
tpe.suggest(constraints=('c',)), the same with constraint_model='density', for
tpe.suggest on loss + 10 max(c, 0) and for rand.suggest; then the same four on a
tighter problem of the same form, x + y <= 0.3 (4.5 % of the square feasible,
optimum 1.445).

--density (tpe.suggest(constraints=..., constraint_model='density')): a whole
tpe.suggest step on the config-3 history with two constraints, 'rank' against
'density', alternating in one process; Engine.cmodel_suggest alone on the models
the step left on the engine; and the host time of building the two constraint
models (posterior.label_posterior and pack for every label).

--tiebreak hypervolume (tpe.suggest(mo_tiebreak='hypervolume')): the timing
leg times Engine.mo_keys(F, tiebreak='hypervolume', n_select=n_below) against
the default Engine.mo_keys(F), alternating, at the sizes above x 2 and 3
objectives, with the level size and the picks of each input, and the worst case
of a 100 000-row antichain (one level) at 3 objectives; with --quality it adds
the row objectives_hypervolume to the ZDT1 table.

--tiebreak hypervolume_mc (tpe.suggest(mo_tiebreak='hypervolume_mc')): the
timing leg times Engine.mo_keys(F, tiebreak='hypervolume_mc', n_select=n_below,
n_samples=--samples) against the default Engine.mo_keys(F), alternating, at
the sizes above x --objectives M (default 4 and 8), with the level size, the
picks, the bytes of the coverage matrix and, up to --host-max-n rows, whether
the numpy builder gives the same keys; with --quality it runs DTLZ2 with four
objectives in six dimensions under 'dominates', 'hypervolume_mc' and random
search and reports the hypervolume dominated (tpe.hypervolume, reference 1.5
on every axis).

--indicator (tpe.hypervolume): Engine.mo_exclusive (tpe_mo_exclusive: upload,
validity, domination pass, live-row list, a workgroup per live row, read-back)
against posterior.mo_exclusive, the numpy builder, alternating, at the sizes
above x 2, 3 and 4 objectives x both modes (4: tpe_mo_exclusive4), on a
3000-row antichain at 3 objectives and on the 2736 integer points of [0, 16)^4
with sum 30 at 4 (every row live); median of --reps calls, the numpy builder up
to --host-max-n rows; with the live rows, the overflow count and whether both
give the same bits.  --indicator-m M keeps the rows with M objectives.
--indicator-method sampled (tpe.hypervolume(method='sampled')):
Engine.mo_exclusive_mc (tpe_mo_exclusive_mc) at the sizes above x 4 and 8
objectives (or --indicator-m, 2 .. 8) x 65 536 and 2^20 samples x both modes,
alternating with posterior.mo_exclusive_mc where a call is at most 2^27 row x
sample tests and, at four objectives, with the exact Engine.mo_exclusive; with
the estimate, its standard error and the exact value.

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


def hv_key_times(eng, args):
    from hyperopt_amd import posterior as P
    inputs = [('uniform', n, M, np.random.RandomState(n + M).uniform(size=(n, M))) for n in SIZES for M in (2, 3)]
    u = np.random.RandomState(7).dirichlet(np.ones(3), 100000)
    inputs.append(('antichain', 100000, 3, u))
    out = []
    for kind, n, M, F in inputs:
        k = P.n_below_of(n, 0.25)
        legs = dict(default=lambda: eng.mo_keys(F),
                    hypervolume=lambda: eng.mo_keys(F, tiebreak='hypervolume', n_select=k))
        ts = {name: [] for name in legs}
        for name in legs:
            legs[name]()               # warm-up
        for _ in range(args.reps):     # alternating
            for name in legs:
                t0 = time.perf_counter()
                legs[name]()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        keys, by, do, picked, gains = eng.mo_keys(F, want_counts=True, tiebreak='hypervolume', n_select=k,
                                                  want_picks=True)
        rec = dict(what='mo_keys_hv', rows=kind, n=n, M=M, n_select=k, picks=len(picked),
                   level=int(np.count_nonzero(by == by[picked[0]])) if len(picked) else 0)
        for name, v in ts.items():
            rec[name] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), reps=len(v))
        rec['hypervolume_minus_default_ms'] = rec['hypervolume']['median_ms'] - rec['default']['median_ms']
        if n <= args.host_max_n:
            rec['same_keys'] = bool(np.array_equal(P.mo_keys(F, tiebreak='hypervolume', n_select=k), keys))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def hvs_key_times(eng, args):
    from hyperopt_amd import posterior as P
    S = args.samples
    out = []
    for n in SIZES:
        for M in ((args.objectives,) if args.objectives else (4, 8)):
            F = np.random.RandomState(n + M).uniform(size=(n, M))
            k = P.n_below_of(n, 0.25)
            legs = dict(default=lambda: eng.mo_keys(F),
                        hypervolume_mc=lambda: eng.mo_keys(F, tiebreak='hypervolume_mc', n_select=k, n_samples=S))
            ts = {name: [] for name in legs}
            for name in legs:
                legs[name]()               # warm-up
            for _ in range(args.reps):     # alternating
                for name in legs:
                    t0 = time.perf_counter()
                    legs[name]()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            keys, by, do, picked, gains = eng.mo_keys(F, want_counts=True, tiebreak='hypervolume_mc', n_select=k,
                                                      n_samples=S, want_picks=True)
            level = int(np.count_nonzero(by == by[picked[0]])) if len(picked) else 0
            rec = dict(what='mo_keys_hvs', rows='uniform', n=n, M=M, n_select=k, n_samples=S, picks=len(picked),
                       level=level, matrix_bytes=level * S // 8, first_gains=[int(g) for g in gains[:3]])
            for name, v in ts.items():
                rec[name] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)),
                                 reps=len(v))
            rec['hypervolume_mc_minus_default_ms'] = rec['hypervolume_mc']['median_ms'] - rec['default']['median_ms']
            if n <= args.host_max_n:
                t0 = time.perf_counter()
                host = P.mo_keys(F, tiebreak='hypervolume_mc', n_select=k, n_samples=S)
                rec['host_ms'] = (time.perf_counter() - t0) * 1e3
                rec['same_keys'] = bool(np.array_equal(host, keys))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def quality4(args):
    """DTLZ2, four objectives, six dimensions: the hypervolume dominated."""
    from hyperopt_amd import STATUS_OK, Trials, fmin, hp, rand, tpe
    names = ('loss', 'f1', 'f2', 'f3')
    space = {'x%d' % i: hp.uniform('x%d' % i, 0, 1) for i in range(6)}

    def dtlz2(cfg):
        x = np.array([cfg['x%d' % i] for i in range(6)])
        g = float(((x[3:] - 0.5) ** 2).sum())
        c, s = np.cos(0.5 * np.pi * x[:3]), np.sin(0.5 * np.pi * x[:3])
        f = (1 + g) * np.array([c[0] * c[1] * c[2], c[0] * c[1] * s[2], c[0] * s[1], s[0]])
        return dict(zip(names, f.tolist()), status=STATUS_OK)
    algos = dict(dominates=partial(tpe.suggest, objectives=names),
                 hypervolume_mc=partial(tpe.suggest, objectives=names, mo_tiebreak='hypervolume_mc',
                                        mo_samples=args.samples),
                 random=rand.suggest)
    rec = dict(what='mo_quality4', problem='DTLZ2, 4 objectives, 6 dimensions', evaluations=args.evals,
               reference_point=[1.5] * 4, seeds=args.seeds, n_samples=args.samples)
    for name, algo in algos.items():
        hv = []
        for seed in range(args.seeds):
            trials = Trials()
            fmin(dtlz2, space, algo=algo, max_evals=args.evals, trials=trials, rstate=np.random.RandomState(seed))
            hv.append(tpe.hypervolume(trials, names, reference=[1.5] * 4)['hypervolume'])
        rec[name] = dict(mean=float(np.mean(hv)), min=float(min(hv)), max=float(max(hv)), std=float(np.std(hv)))
    print(json.dumps(rec), flush=True)
    return [rec]


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


def density_step_times(args):
    from hyperopt_amd import engine as E, history, posterior as P, tpe, workloads
    from hyperopt_amd.base import Domain
    names = ('c0', 'c1')
    hist = workloads.mixed_history(32, 10000, seed=0)
    trials = workloads.history_trials(hist)
    G = np.random.RandomState(1).uniform(size=(len(trials.trials), 2)) - 0.6
    for d, g in zip(trials.trials, G):
        d['result'].update(zip(names, map(float, g)))
    domain = Domain(lambda d: 0.0, workloads.hp_space(hist.labels))
    n = len(trials.trials)
    legs = dict(rank=lambda: tpe.suggest([n], domain, trials, 3, constraints=names),
                density=lambda: tpe.suggest([n], domain, trials, 3, constraints=names, constraint_model='density'))
    ts = {k: [] for k in legs}
    for k in legs:
        legs[k]()                      # warm-up
    for _ in range(args.reps):         # alternating
        for k in legs:
            t0 = time.perf_counter()
            legs[k]()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    rec = dict(what='cmodel_step', labels=32, trials=n, K=2)
    for k, v in ts.items():
        rec[k] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), reps=len(v))
    # the round alone, on the models the last density step left on the engine
    eng = E.get_engine(0, 'f64')
    gammas = np.full((32, 3), 0.4)
    rec['cmodel_suggest'] = timed(lambda: eng.cmodel_suggest(3, [n], 24, gammas), args.reps)
    # the host build of the two constraint models
    specs = tpe.specs_of(domain)
    tids, _, obs = history.gather(domain, trials, list(specs))
    live, split = P.cmodel_split(G, 0.25)

    def build():
        for below, _ in split:
            b_tids = tids[below]
            a_tids = np.setdiff1d(tids[live], b_tids)
            P.pack([P.label_posterior(k, sp.kind, sp.args, *P.split_label(obs[k][0], obs[k][1], b_tids, a_tids),
                                      prior_weight=1.0) for k, sp in specs.items()])
    rec['host_model_build'] = timed(build, max(3, args.reps // 4))
    rec['step_difference_ms'] = rec['density']['median_ms'] - rec['rank']['median_ms']
    print(json.dumps(rec), flush=True)
    return [rec]


def quality_constrained(args):
    return [quality_constrained_at(args, 1.0), quality_constrained_at(args, 0.3)]


def quality_constrained_at(args, limit):
    from hyperopt_amd import STATUS_OK, Trials, fmin, hp, rand, tpe
    space = {'x': hp.uniform('x', 0, 1), 'y': hp.uniform('y', 0, 1)}

    def parts(cfg):
        return (cfg['x'] - 1) ** 2 + (cfg['y'] - 1) ** 2, cfg['x'] + cfg['y'] - limit

    def constrained(cfg):
        f, c = parts(cfg)
        return {'loss': f, 'f': f, 'c': c, 'status': STATUS_OK}

    def penalised(cfg):
        f, c = parts(cfg)
        return {'loss': f + 10.0 * max(c, 0.0), 'f': f, 'c': c, 'status': STATUS_OK}
    algos = dict(constraints=(constrained, partial(tpe.suggest, constraints=('c',))),
                 density=(constrained, partial(tpe.suggest, constraints=('c',), constraint_model='density')),
                 tpe_on_the_penalty=(penalised, tpe.suggest), random=(constrained, rand.suggest))
    rec = dict(what='mo_quality_constrained',
               problem='(x-1)^2 + (y-1)^2 under x + y <= %g, optimum %g' % (limit, 2 * (1 - limit / 2) ** 2),
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
    return rec


def indicator_times(args):
    """tpe.hypervolume's two columns (Engine.mo_exclusive against posterior.mo_exclusive), alternating."""
    from hyperopt_amd import posterior as P
    from hyperopt_amd.engine import Engine
    eng = Engine(0, 'f64')
    inputs = [('uniform', n, M, np.random.RandomState(n + M).uniform(size=(n, M))) for n in SIZES for M in (2, 3)]
    t = np.arange(3000.0)
    inputs.append(('antichain', 3000, 3, np.column_stack([t, 3000 - t, np.random.RandomState(7).uniform(size=3000)])))
    # M = 4 (tpe_mo_exclusive4): the same sizes, and the 2736 integer points of [0, 16)^4 with sum 30, shuffled
    inputs += [('uniform', n, 4, np.random.RandomState(n + 4).uniform(size=(n, 4))) for n in SIZES]
    grid = np.indices((16,) * 4).reshape(4, -1).T
    lattice = np.random.RandomState(7).permutation(grid[grid.sum(axis=1) == 30]).astype(float)
    inputs.append(('antichain', len(lattice), 4, lattice))
    if args.indicator_m:
        inputs = [i for i in inputs if i[2] == args.indicator_m]
    out = []
    for kind, n, M, F in inputs:
        ref = tuple((F.max(axis=0) + 0.1 * (F.max(axis=0) - F.min(axis=0))).tolist())
        for mode in P.MO_EXCLUSIVE_MODES:
            legs = dict(device=lambda: eng.mo_exclusive(F, ref, mode, want_overflow=True))
            if n <= args.host_max_n:   # (the numpy builder takes half a minute a call and more at 50 000 rows)
                legs['host'] = lambda: P.mo_exclusive(F, ref, mode)
            ts = {name: [] for name in legs}
            got = {name: legs[name]() for name in legs}               # warm-up
            for _ in range(args.reps):                                 # alternating
                for name in legs:
                    t0 = time.perf_counter()
                    legs[name]()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            rec = dict(what='mo_exclusive', rows=kind, n=n, M=M, mode=mode,
                       live=int(np.count_nonzero(got['device'][0])), n_overflow=int(got['device'][1]))
            for name, v in ts.items():
                rec[name] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), reps=len(v))
            if 'host' in legs:
                rec['same_bits'] = bool(np.array_equal(got['device'][0], got['host']))
                rec['host_over_device'] = rec['host']['median_ms'] / rec['device']['median_ms']
            else:
                rec['host'] = 'not measured'
            print(json.dumps(rec), flush=True)
            out.append(rec)
    eng.close()
    return out


def sampled_indicator_times(args):
    """tpe.hypervolume(method='sampled')'s two columns: Engine.mo_exclusive_mc against posterior.mo_exclusive_mc
    (up to 2^27 row x sample tests a call) and, at four objectives, against the exact Engine.mo_exclusive --
    alternating; the value is V x the column's sum / S (the hypervolume for 'before')."""
    from hyperopt_amd import posterior as P
    from hyperopt_amd.engine import Engine
    eng = Engine(0, 'f64')
    out = []
    for n in SIZES:
        for M in ([args.indicator_m] if args.indicator_m else [4, 8]):
            F = np.random.RandomState(n + M).uniform(size=(n, M))
            ref = tuple((F.max(axis=0) + 0.1 * (F.max(axis=0) - F.min(axis=0))).tolist())
            V = P.mo_hvm_thresholds(F, ref)[2]
            for S in (65536, 1 << 20):
                for mode in P.MO_EXCLUSIVE_MODES:
                    legs = dict(device=lambda: eng.mo_exclusive_mc(F, ref, mode, S))
                    if n * S <= 1 << 27:
                        legs['host'] = lambda: P.mo_exclusive_mc(F, ref, mode, S)
                    if M == 4:
                        legs['exact'] = lambda: eng.mo_exclusive(F, ref, mode)
                    ts = {name: [] for name in legs}
                    got = {name: legs[name]() for name in legs}               # warm-up
                    for _ in range(args.reps):                                 # alternating
                        for name in legs:
                            t0 = time.perf_counter()
                            legs[name]()
                            ts[name].append((time.perf_counter() - t0) * 1e3)
                    count, covered = got['device']
                    p = covered / S
                    rec = dict(what='mo_exclusive_mc', rows='uniform', n=n, M=M, S=S, mode=mode, covered=covered,
                               owners=int(np.count_nonzero(count)), value=V * float(count.sum()) / S,
                               stderr=V * float(np.sqrt(p * (1 - p) / S)))
                    for name, v in ts.items():
                        rec[name] = dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)),
                                         reps=len(v))
                    if 'host' in legs:
                        rec['same_counts'] = bool(np.array_equal(count, got['host'][0]) and covered == got['host'][1])
                    if 'exact' in legs:
                        rec['exact_value'] = float(np.sum(got['exact']))
                    print(json.dumps(rec), flush=True)
                    out.append(rec)
    eng.close()
    return out


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
    if args.tiebreak == 'hypervolume':
        algos['objectives_hypervolume'] = (both, partial(tpe.suggest, objectives=('loss', 'cost'),
                                                         mo_tiebreak='hypervolume'), 'loss')
    rec = dict(what='mo_quality', problem='ZDT1, 4 dimensions', evaluations=args.evals, reference_point=ref.tolist(),
               seeds=args.seeds)
    for name, (fn, algo, first) in algos.items():
        hv = []
        for seed in range(args.seeds):
            trials = Trials()
            fmin(fn, space, algo=algo, max_evals=args.evals, trials=trials, rstate=np.random.RandomState(seed))
            hv.append(tpe.hypervolume(trials, (first, 'cost'), reference=ref)['hypervolume'])
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
    ap.add_argument('--density', action='store_true')
    ap.add_argument('--indicator', action='store_true')
    ap.add_argument('--indicator-m', type=int, default=0, metavar='M', help='--indicator: only the rows with M objectives')
    ap.add_argument('--indicator-method', choices=('exact', 'sampled'), default='exact',
                    help="--indicator: 'sampled' times tpe_mo_exclusive_mc at M in {4, 8} (--indicator-m: 2 .. 8)")
    ap.add_argument('--tiebreak', choices=('dominates', 'hypervolume', 'hypervolume_mc'), default='dominates')
    ap.add_argument('--objectives', type=int, default=0, metavar='M', help='--tiebreak hypervolume_mc: only M objectives')
    ap.add_argument('--samples', type=int, default=65536, metavar='S', help='--tiebreak hypervolume_mc: n_samples')
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
    if args.indicator and args.indicator_method == 'sampled':
        if args.indicator_m and not 2 <= args.indicator_m <= 8:
            ap.error('--indicator-m: 2 to 8 objectives')
        recs = sampled_indicator_times(args)
    elif args.indicator:
        recs = indicator_times(args)
    elif args.quality_constrained:
        recs = quality_constrained(args)
    elif args.density:
        recs = density_step_times(args)
    elif args.constraints:
        from hyperopt_amd.engine import Engine
        eng = Engine(0, 'f64')
        recs = constrained_key_times(eng, args)
        eng.close()
        recs += constrained_step_times(args)
    elif args.quality:
        recs = quality4(args) if args.tiebreak == 'hypervolume_mc' else quality(args)
    elif args.tiebreak == 'hypervolume_mc':
        from hyperopt_amd.engine import Engine
        eng = Engine(0, 'f64')
        recs = hvs_key_times(eng, args)
        eng.close()
    elif args.tiebreak == 'hypervolume':
        from hyperopt_amd.engine import Engine
        eng = Engine(0, 'f64')
        recs = hv_key_times(eng, args)
        eng.close()
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
