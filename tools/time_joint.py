"""Timings and a quality record of multivariate (joint) TPE (needs the GPU).

    python tools/time_joint.py [--dims 32] [--trials 10000] [--reps 20] [--quality] [--out FILE]
    python tools/time_joint.py --groups [--legs loop,batch] [--reps 20] [--out FILE]
    python tools/time_joint.py --quantized | --categorical [--legs dense,...] [--reps 20] [--out FILE]
    python tools/time_joint.py --no-timings --quality-quantized | --quality-categorical [--out FILE]
    python tools/time_joint.py --build [--legs device_build,...] [--dims 32] [--trials 10000] [--reps 20] [--out FILE]
    python tools/time_joint.py --no-timings --quality-bandwidth [--out FILE]
    python tools/time_joint.py --devices 0,0 --quantized --legs dense | --build [--out FILE]
    python tools/time_joint.py --fixed [--dims 32] [--trials 10000] [--fix 8] [--reps 20] [--out FILE]

On a synthetic history of `--trials` trials over `--dims` dense continuous
labels (kinds cycled over uniform / loguniform / normal / lognormal):

* the host build of the joint mixtures (posterior.joint_mixture, wall time)
  and Engine.set_joint_posterior (upload + device fold, wall time), apart;
* Engine.joint_suggest at 24 and at 2^16 candidates: device time between HIP
  events on the engine's stream (tpe_last_timing) and wall time, medians;
  for the 2^16 shape the fp64 rate over 4 flops (two FMAs) per (candidate,
  component, dimension) and its fraction of the MI355X's fp64 vector peak;
* the independent round (Engine.suggest) on the same labels, history and
  candidate counts;
* the numpy definition (tests/joint_reference.py) on one CPU core, scoring
  the 24 candidates of one round under both mixtures.

--quality: fmin for 100 evaluations over seeds 0..9 on the coupled objective
(x - y)^2 + 0.01 (x + y)^2 over uniform(-5, 5)^2, with and without
multivariate=True; the medians of the best losses.  A record, not a gate.

--groups: several joint groups and new ids per call (groups_timings): the
loop over single-posterior calls against set_joint_group +
joint_suggest_batch, 24 candidates, 1 / 24 / 4096 ids.

--quantized: the d32 shape (32 labels, 10000 trials: K 26 / 9976) dense and
with every second label quantized (quantized_timings), at 24 candidates for
one id, 24 candidates for 4096 ids (batched) and 2^16 candidates in one
round; --legs dense,quantized selects.  The dense leg uses the entry points
of a checkout without quantized groups, so it runs unchanged there.

--quality-quantized: fmin for 100 evaluations over seeds 0..9 on
(x - n)^2 + 0.01 (x + n)^2 with x uniform(-5, 5) and n quniform(-5, 5, 1):
independent, multivariate=True, and multivariate=True with
joint_quantized=True.  A record, not a gate.

--categorical: the d32 shape dense and with every fourth label replaced by
randint(8) (categorical_timings), the shapes of --quantized; --legs
dense,categorical selects.  The dense leg is --quantized --legs dense, which a
checkout without categorical groups runs too.

--quality-categorical: fmin for 100 evaluations over seeds 0..9 on
(x - [-3, 0, 3][k])^2 + 0.1 k with x uniform(-5, 5) and k a 3-way choice:
independent, multivariate=True, and multivariate=True with
joint_categorical=True.  A record, not a gate.

--build: on the --dims x --trials history (default d32: 32 x 10000),
Engine.build_joint_groups on the resident history against
posterior.joint_mixture + Engine.set_joint_posterior, and a whole
tpe.suggest(multivariate=True) call with posterior_builder='device' against
'host' (build_timings); medians of --reps calls after a warm-up call.  Both
builders are timed under joint_bandwidth 'neighbour' and 'scott'; --legs
device_build,device_build_scott times the two device builds alone.

--quality-bandwidth: the three quality objectives above, fmin for 100
evaluations over seeds 0..9, with joint_bandwidth='neighbour' and 'scott' (and
the independent call).  A record, not a gate.

--devices 0,0 (or 0,1 on a machine with two GPUs): the legs of --quantized,
--categorical and --build on a multi-device engine, Engine([0, 0]) -- the
joint rounds sharded over the devices (each leg records how:
Engine.joint_last_shards), the joint build behind a label-sharded univariate
build; the tpe.suggest legs of --build get devices=[...] too.  Two contexts on
one GPU show what the fork, the merge and the duplicated launches cost, not a
speed-up.

--fixed: on the --dims x --trials history (default d32), after the device
build of the group: Engine.joint_condition with the first --fix labels held
(fixed_timings) against what it replaces -- Engine.joint_get_group of both
sides, the rule in numpy, Engine.set_joint_group of the result -- and a whole
tpe.suggest(multivariate=True) call with and without fixed=.  Medians, the
smallest and the largest of --reps calls.  --devices applies.

Prints one JSON document (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time
from functools import partial

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VECTOR_PEAK = 78.6e12   # MI355X data sheet, fp64 vector FLOP/s
KINDS = ('uniform', 'loguniform', 'normal', 'lognormal')
DEVICES = None   # --devices: the ordinals of a multi-device engine


def make_engine():
    from hyperopt_amd.engine import Engine
    return Engine(list(DEVICES) if DEVICES else 0, 'f64')


def history(n_dims, n_trials, seed=0):
    rng = np.random.RandomState(seed)
    tids = np.arange(n_trials)
    losses = rng.randn(n_trials)
    group, obs = [], {}
    for d in range(n_dims):
        kind = KINDS[d % 4]
        label = 'h%03d' % d
        if kind == 'uniform':
            args, v = dict(low=-5.0, high=5.0), rng.uniform(-5, 5, n_trials)
        elif kind == 'loguniform':
            args, v = dict(low=-3.0, high=2.0), np.exp(rng.uniform(-3, 2, n_trials))
        elif kind == 'normal':
            args, v = dict(mu=1.0, sigma=2.0), 1.0 + 2.0 * rng.randn(n_trials)
        else:
            args, v = dict(mu=0.0, sigma=1.0), np.exp(rng.randn(n_trials))
        group.append((label, kind, args))
        obs[label] = (tids, v)
    return group, tids, losses, obs


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def timings(n_dims, n_trials, reps):
    from hyperopt_amd import posterior as P
    from hyperopt_amd.engine import Engine
    from tests import joint_reference as JR
    group, tids, losses, obs = history(n_dims, n_trials)
    splitter = P.Splitter(tids, losses, 0.25)
    res = dict(dims=n_dims, trials=n_trials, reps=reps)
    mix = P.joint_mixture(group, obs, splitter, 1.0)
    res['host_build_ms'] = median_ms(lambda: P.joint_mixture(group, obs, splitter, 1.0), max(3, reps // 4))
    res['k_below'], res['k_above'] = len(mix.wb), len(mix.wa)
    eng = Engine(0, 'f64')
    eng.set_joint_posterior(*mix)
    res['upload_fold_ms'] = median_ms(lambda: eng.set_joint_posterior(*mix), reps)
    terms = (res['k_below'] + res['k_above']) * n_dims
    for n in (24, 1 << 16):
        eng.joint_suggest(1, n, round=0)
        dev, wall = [], []
        for r in range(reps):
            t = time.perf_counter()
            eng.joint_suggest(1, n, round=r + 1)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(eng.last_timing()[1])
        key = 'joint_%d' % n
        res[key] = dict(device_ms=float(np.median(dev)), wall_ms=float(np.median(wall)))
        if n > 24:
            rate = 4.0 * n * terms / (res[key]['device_ms'] * 1e-3)
            res[key].update(fp64_flops=rate, fraction_of_fp64_vector_peak=rate / FP64_VECTOR_PEAK)
    # the independent round on the same labels and counts
    posts = []
    for label, kind, args in group:
        b, a = splitter.split(*obs[label])
        posts.append(P.label_posterior(label, kind, args, b, a, 1.0))
    eng.set_posterior(*P.pack(posts))
    for n in (24, 1 << 16):
        eng.suggest(1, n, round=0)
        dev, wall = [], []
        for r in range(reps):
            t = time.perf_counter()
            eng.suggest(1, n, round=r + 1)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(eng.last_timing()[1])
        res['independent_%d' % n] = dict(device_ms=float(np.median(dev)), wall_ms=float(np.median(wall)))
    # the numpy definition, one core, the 24-candidate shape
    dims = []
    for d, (label, kind, args) in enumerate(group):
        log, low, high, _, _ = JR.prior_of(kind, args)
        dims.append(JR.Dim(log, low, high, d))
    ref = JR.JointRef(dims, (mix.wb, mix.mub, mix.sigb), (mix.wa, mix.mua, mix.siga))
    eng.set_joint_posterior(*mix)
    vals, _ = eng.joint_draw(1, 24, round=1)
    t = time.perf_counter()
    ll, lg = ref.joint_lpdf(vals, 'below'), ref.joint_lpdf(vals, 'above')
    res['numpy_24_ms'] = (time.perf_counter() - t) * 1e3
    dl, dg = eng.joint_score(vals)
    res['numpy_vs_device_max_abs'] = float(max(np.max(np.abs(ll - dl)), np.max(np.abs(lg - dg))))
    eng.close()
    return res


def group_shapes():
    """name -> list of joint mixtures, one per group: `c4`, the two D = 2
    groups inside the branches of config 4 (workloads.conditional_history(5000):
    svm_C with svm_gamma, gbm_lr with gbm_subsample); `d32`, one group of 32
    dimensions over 10000 trials."""
    from hyperopt_amd import posterior as P, workloads
    hist = workloads.conditional_history(5000)
    by = {n: (n, k, a) for n, k, a in hist.labels}
    names = [n for n, _, _ in hist.labels]
    splitter = P.Splitter(hist.tids, hist.losses, 0.25)
    c4 = [P.joint_mixture([by[k] for k in g], hist.obs, splitter, 1.0, streams=[names.index(k) for k in g])
          for g in (('svm_C', 'svm_gamma'), ('gbm_lr', 'gbm_subsample'))]
    group, tids, losses, obs = history(32, 10000)
    d32 = [P.joint_mixture(group, obs, P.Splitter(tids, losses, 0.25), 1.0)]
    return {'c4': c4, 'd32': d32}


def groups_timings(reps, legs=('loop', 'batch'), rounds=(1, 24, 4096), n=24):
    """Per shape and number of new ids, medians over `reps` calls of the wall
    time of a whole call (uploads and folds included) and of the device time
    of its rounds between HIP events:

    * loop: per group one set_joint_posterior, then one joint_suggest per id
      -- entry points a context with a single joint posterior has, so this
      leg runs unchanged on an older checkout (the baseline);
    * batch: set_joint_group once per group and one joint_suggest_batch."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import Engine
    eng = Engine(0, 'f64')
    out = {}
    for name, mixes in sorted(group_shapes().items()):
        terms = sum((len(m.wb) + len(m.wa)) * len(m.dims) for m in mixes)
        res = out[name] = dict(groups=len(mixes), dims=[len(m.dims) for m in mixes],
                               k_below=[len(m.wb) for m in mixes], k_above=[len(m.wa) for m in mixes])
        for R in rounds:
            ids = list(range(1000, 1000 + R))

            def loop():
                dev = 0.0
                for m in mixes:
                    eng.set_joint_posterior(*m)
                    for i in ids:
                        eng.joint_suggest(1, n, round=i)
                        dev += eng.last_timing()[1]
                return dev

            def batch():
                eng.clear_joint_groups()
                for j, m in enumerate(mixes):
                    eng.set_joint_group(j, L.TPE_JOINT_STREAM - j, *m)
                eng.joint_suggest_batch(1, ids, n)
                return eng.last_timing()[1]

            for leg, fn in (('loop', loop), ('batch', batch)):
                if leg not in legs or (leg == 'batch' and not hasattr(eng, 'joint_suggest_batch')):
                    continue
                fn()
                dev, wall = [], []
                for _ in range(reps):
                    t = time.perf_counter()
                    dev.append(fn())
                    wall.append((time.perf_counter() - t) * 1e3)
                rec = dict(device_ms=float(np.median(dev)), wall_ms=float(np.median(wall)),
                           wall_min_ms=float(np.min(wall)), wall_max_ms=float(np.max(wall)))
                rate = 4.0 * n * R * terms / (rec['device_ms'] * 1e-3)
                rec.update(fp64_flops=rate, fraction_of_fp64_vector_peak=rate / FP64_VECTOR_PEAK)
                res['%s_%d' % (leg, R)] = rec
            if 'loop_%d' % R in res and 'batch_%d' % R in res:
                res['loop_over_batch_wall_%d' % R] = res['loop_%d' % R]['wall_ms'] / res['batch_%d' % R]['wall_ms']
    eng.close()
    return out


QKINDS = {'uniform': 'quniform', 'loguniform': 'qloguniform', 'normal': 'qnormal', 'lognormal': 'qlognormal'}


def quantized_history(n_dims, n_trials, step=0.25):
    """history() with every second label (odd d) of the quantized kind of
    its kind, step `step`, its observations on the grid."""
    group, tids, losses, obs = history(n_dims, n_trials)
    out = []
    for d, (label, kind, args) in enumerate(group):
        if d % 2:
            kind, args = QKINDS[kind], dict(args, q=step)
            obs[label] = (tids, np.rint(obs[label][1] / step) * step)
        out.append((label, kind, args))
    return out, tids, losses, obs


def _round_shapes(eng, reps):
    """Slot 0's rounds: joint_suggest at 24 candidates, joint_suggest_batch
    at 24 candidates for 4096 ids, joint_suggest at 2^16 candidates -- medians
    and the range over `reps` calls of the device time between HIP events and
    of the wall time."""
    res = {}
    ids = list(range(1000, 1000 + 4096))
    shapes = (('one_24', lambda r: eng.joint_suggest(1, 24, round=r)),
              ('batch_4096x24', lambda r: eng.joint_suggest_batch(1, [i + r for i in ids], 24)),
              ('one_65536', lambda r: eng.joint_suggest(1, 1 << 16, round=r)))
    for name, fn in shapes:
        fn(0)
        dev, wall = [], []
        for r in range(reps):
            t = time.perf_counter()
            fn(r + 1)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(eng.last_timing()[1])
        res[name] = dict(device_ms=float(np.median(dev)), device_min_ms=float(np.min(dev)),
                         device_max_ms=float(np.max(dev)), wall_ms=float(np.median(wall)),
                         wall_min_ms=float(np.min(wall)), wall_max_ms=float(np.max(wall)))
        if hasattr(eng, 'joint_last_shards'):   # (mode, devices): how the leg's rounds were split
            res[name]['shards'] = list(eng.joint_last_shards())
    return res


def quantized_timings(reps, legs=('dense', 'quantized'), n_dims=32, n_trials=10000):
    """Medians (and the range) over `reps` calls of the device time between
    HIP events and of the wall time of: joint_suggest at 24 candidates,
    joint_suggest_batch at 24 candidates for 4096 ids, joint_suggest at 2^16
    candidates -- the dense d32 group and the group with half of its labels
    quantized."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd import posterior as P
    eng = make_engine()
    out = {}
    for leg in legs:
        group, tids, losses, obs = (history if leg == 'dense' else quantized_history)(n_dims, n_trials)
        mix = P.joint_mixture(group, obs, P.Splitter(tids, losses, 0.25), 1.0, quantized=True)
        eng.clear_joint_groups()
        eng.set_joint_group(0, L.TPE_JOINT_STREAM, *mix)
        res = out[leg] = dict(dims=n_dims, k_below=len(mix.wb), k_above=len(mix.wa),
                              quantized_dims=int(np.count_nonzero(mix.q)))
        res.update(_round_shapes(eng, reps))
    if 'dense' in out and 'quantized' in out:
        for name in ('one_24', 'batch_4096x24', 'one_65536'):
            out['quantized_over_dense_device_' + name] = (out['quantized'][name]['device_ms'] /
                                                          out['dense'][name]['device_ms'])
    eng.close()
    return out


def categorical_history(n_dims, n_trials, upper=8):
    """history() with every fourth label (d % 4 == 3) replaced by
    randint(upper), its observations uniform over the categories."""
    group, tids, losses, obs = history(n_dims, n_trials)
    rng = np.random.RandomState(1)
    out = []
    for d, (label, kind, args) in enumerate(group):
        if d % 4 == 3:
            kind, args = 'randint', dict(upper=upper)
            obs[label] = (tids, rng.randint(0, upper, n_trials))
        out.append((label, kind, args))
    return out, tids, losses, obs


def categorical_timings(reps, legs=('dense', 'categorical'), n_dims=32, n_trials=10000):
    """quantized_timings' shapes for the dense d32 group and the group with
    every fourth label a randint(8) (`mixed`)."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd import posterior as P
    eng = make_engine()
    out = {}
    for leg in legs:
        group, tids, losses, obs = (history if leg == 'dense' else categorical_history)(n_dims, n_trials)
        mix = P.joint_mixture(group, obs, P.Splitter(tids, losses, 0.25), 1.0, categorical=True)
        eng.clear_joint_groups()
        eng.set_joint_group(0, L.TPE_JOINT_STREAM, *mix, prior_weight=1.0)
        res = out[leg] = dict(dims=n_dims, k_below=len(mix.wb), k_above=len(mix.wa),
                              categorical_dims=int(np.count_nonzero(mix.upper)))
        res.update(_round_shapes(eng, reps))
    if 'dense' in out and 'categorical' in out:
        for name in ('one_24', 'batch_4096x24', 'one_65536'):
            out['categorical_over_dense_device_' + name] = (out['categorical'][name]['device_ms'] /
                                                            out['dense'][name]['device_ms'])
    eng.close()
    return out


BUILD_LEGS = ('device_build', 'device_build_scott', 'host_build', 'host_build_scott', 'upload_fold',
              'host_build_plus_upload', 'suggest')


def build_timings(reps, n_dims=32, n_trials=10000, legs=BUILD_LEGS):
    """The joint build on the device against the host's, on the d32 shape,
    medians (and the range) of the wall time over `reps` calls after one
    warm-up call each (`legs` selects):

    * device_build: Engine.build_joint_groups on the resident history, its
      univariate posterior built once before (gather launch + fold + the
      call's one synchronisation);
    * device_build_scott / host_build_scott: that call and
      posterior.joint_mixture with bandwidth='scott';
    * host_build + upload_fold: posterior.joint_mixture, then
      Engine.set_joint_posterior with its arrays -- what the same call costs
      without the device build (the expectation to report against);
    * suggest_device / suggest_host: a whole tpe.suggest(multivariate=True)
      call for one new id on that history as Trials, posterior_builder
      'device' against 'host' (each on a warm engine: the history resident,
      nothing new to upload).

    Checks first that both builds give the same winner bits."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd import posterior as P, tpe, workloads
    from hyperopt_amd.base import Domain
    group, tids, losses, obs = history(n_dims, n_trials)
    splitter = P.Splitter(tids, losses, 0.25)
    dev_kw = dict(devices=list(DEVICES)) if DEVICES else {}

    class Owner(object):
        pass
    view = (tids, losses, n_trials, obs, Owner())
    eng = make_engine()
    P.DeviceHistoryUploader().build(eng, group, view, 0.25, 1.0)
    ids = list(range(n_dims))
    args = [(0, L.TPE_JOINT_STREAM, ids, ids)]
    assert not eng.build_joint_groups(args)[0], 'the device flagged the timing history'
    won_dev = eng.joint_suggest(1, 24, round=5)
    mix = P.joint_mixture(group, obs, splitter, 1.0)
    eng.set_joint_posterior(*mix)
    won_host = eng.joint_suggest(1, 24, round=5)
    assert np.array_equal(won_dev[0], won_host[0]) and won_dev[1:] == won_host[1:]
    scott = dict(bandwidth='scott', prior_weight=1.0)
    assert not eng.build_joint_groups(args, **scott)[0]
    won_dev = eng.joint_suggest(1, 24, round=5)
    eng.set_joint_posterior(*P.joint_mixture(group, obs, splitter, 1.0, bandwidth='scott'))
    won_host = eng.joint_suggest(1, 24, round=5)
    assert np.array_equal(won_dev[0], won_host[0]) and won_dev[1:] == won_host[1:]

    def spread(fn, n):
        fn()
        out = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3)
        return dict(median_ms=float(np.median(out)), min_ms=float(np.min(out)), max_ms=float(np.max(out)), reps=n)
    res = dict(dims=n_dims, trials=n_trials, k_below=len(mix.wb), k_above=len(mix.wa))
    if DEVICES:   # where the group's labels live: -1 everywhere on a replicated context
        res['devices'] = list(DEVICES)
        res['label_devices'] = [int(eng.lib.tpe_label_device(eng.h, i)) for i in ids]
    timed = (('device_build', lambda: eng.build_joint_groups(args)),
             ('device_build_scott', lambda: eng.build_joint_groups(args, **scott)),
             ('host_build', lambda: P.joint_mixture(group, obs, splitter, 1.0)),
             ('host_build_scott', lambda: P.joint_mixture(group, obs, splitter, 1.0, bandwidth='scott')),
             ('upload_fold', lambda: eng.set_joint_posterior(*mix)),
             ('host_build_plus_upload', lambda: eng.set_joint_posterior(*P.joint_mixture(group, obs, splitter, 1.0))))
    for leg, fn in timed:
        if leg in legs:
            res[leg] = spread(fn, reps)
    if 'host_build_plus_upload' in res and 'device_build' in res:
        res['host_over_device'] = res['host_build_plus_upload']['median_ms'] / res['device_build']['median_ms']
    if 'device_build_scott' in res and 'device_build' in res:
        res['scott_over_neighbour_device'] = res['device_build_scott']['median_ms'] / res['device_build']['median_ms']
    eng.close()
    if 'suggest' not in legs:
        return res
    hist = workloads.History(group, tids, losses, obs)
    trials = workloads.history_trials(hist)
    space = workloads.hp_space(group)
    domain = Domain(lambda d: 0.0, space)

    def leg_trials():
        # --devices: every leg starts from trials of its own (a first upload, taken by the warm-up call).
        # A posterior set from the host (posterior_builder='host') leaves a multi-device context
        # replicated, and a resident history sharded before it is only re-partitioned by an upload.
        return workloads.history_trials(hist) if DEVICES else trials
    for builder in ('device', 'host'):
        trials = leg_trials()
        res['suggest_' + builder] = spread(
            lambda: tpe.suggest([n_trials], domain, trials, 3, multivariate=True, posterior_builder=builder, **dev_kw), reps)
    # the device univariate build with the joint groups built on the host: what
    # posterior_builder='device' did before the joint build moved to the device
    tpe.JOINT_DEVICE_BUILD = False
    trials = leg_trials()
    try:
        res['suggest_device_joint_on_host'] = spread(
            lambda: tpe.suggest([n_trials], domain, trials, 3, multivariate=True, posterior_builder='device', **dev_kw),
            reps)
    finally:
        tpe.JOINT_DEVICE_BUILD = True
    trials = leg_trials()
    res['suggest_independent_device'] = spread(
        lambda: tpe.suggest([n_trials], domain, trials, 3, posterior_builder='device', **dev_kw), reps)
    trials = leg_trials()
    res['suggest_device_scott'] = spread(
        lambda: tpe.suggest([n_trials], domain, trials, 3, multivariate=True, posterior_builder='device',
                            joint_bandwidth='scott', **dev_kw), reps)
    res['suggest_host_over_device'] = res['suggest_host']['median_ms'] / res['suggest_device']['median_ms']
    return res


FIXED_VALUE = {'uniform': 1.75, 'loguniform': 0.4, 'normal': 0.25, 'lognormal': 1.5}


def numpy_condition(group, fixed, values, side):
    """The conditioning rule on one side's read-back arrays (dense labels):
    (W', the free columns of mu and sigma)."""
    W, mu, sig = side
    with np.errstate(divide='ignore'):
        L = np.log(W)
    for d, x in zip(fixed, values):
        y = np.log(x) if group[d][1] in ('loguniform', 'lognormal') else x
        z = (y - mu[:, d]) / sig[:, d]
        L = L - 0.5 * z * z - np.log(sig[:, d] * 2.50662827463100050242)
    top = np.max(L)
    rel = L - (top + np.log(np.sum(np.exp(L - top))))
    free = [d for d in range(len(group)) if d not in fixed]
    return (np.maximum(np.exp(rel), 2.0 ** -1022), np.ascontiguousarray(mu[:, free]),
            np.ascontiguousarray(sig[:, free]))


def fixed_timings(reps, n_dims=32, n_trials=10000, n_fixed=8):
    """Engine.joint_condition on the device-built d32 group with the first
    n_fixed labels held, against the path it replaces, wall time of `reps`
    calls after one warm-up call each:

    * condition: joint_condition(0, ..., dst=1) -- the three kernels, the
      fold and the call's two synchronisations;
    * get_group / numpy_rule / set_group: the read-back of both sides, the
      rule in numpy on them, set_joint_group of the result (host_path: the
      three in one call);
    * suggest / suggest_fixed: a whole tpe.suggest(multivariate=True,
      posterior_builder='device') call for one new id without and with
      fixed= on that history as Trials.

    Checks first that the conditioned slot and the host path's slot give the
    same winner index and values to 1e-9."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd import posterior as P, tpe, workloads
    from hyperopt_amd.base import Domain
    group, tids, losses, obs = history(n_dims, n_trials)
    dev_kw = dict(devices=list(DEVICES)) if DEVICES else {}

    class Owner(object):
        pass
    view = (tids, losses, n_trials, obs, Owner())
    eng = make_engine()
    P.DeviceHistoryUploader().build(eng, group, view, 0.25, 1.0)
    ids = list(range(n_dims))
    args = [(0, L.TPE_JOINT_STREAM, ids, ids)]
    assert not eng.build_joint_groups(args)[0], 'the device flagged the timing history'
    fixed = list(range(n_fixed))
    values = [FIXED_VALUE[group[d][1]] for d in fixed]
    free = [d for d in ids if d not in fixed]
    dims = P.joint_mixture(group, obs, P.Splitter(tids, losses, 0.25), 1.0).dims[free]

    def host_path():
        b, a = (numpy_condition(group, fixed, values, eng.joint_get_group(0, side)) for side in (0, 1))
        eng.set_joint_group(2, L.TPE_JOINT_STREAM, dims, *(b + a))
    eng.joint_condition(0, fixed, values, dst=1)
    host_path()
    won_dev, won_host = eng.joint_suggest(1, 24, round=5, slot=1), eng.joint_suggest(1, 24, round=5, slot=2)
    assert won_dev[1] == won_host[1] and np.allclose(won_dev[0], won_host[0], rtol=1e-9, atol=0.0)

    def spread(fn, n):
        fn()
        out = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3)
        return dict(median_ms=float(np.median(out)), min_ms=float(np.min(out)), max_ms=float(np.max(out)), reps=n)
    sides = [eng.joint_get_group(0, side) for side in (0, 1)]
    cond = [numpy_condition(group, fixed, values, s) for s in sides]
    res = dict(dims=n_dims, trials=n_trials, fixed=n_fixed, k_below=len(sides[0][0]), k_above=len(sides[1][0]))
    if DEVICES:
        res['devices'] = list(DEVICES)
    res['device_build'] = spread(lambda: eng.build_joint_groups(args), reps)
    res['condition'] = spread(lambda: eng.joint_condition(0, fixed, values, dst=1), reps)
    res['get_group'] = spread(lambda: [eng.joint_get_group(0, side) for side in (0, 1)], reps)
    res['numpy_rule'] = spread(lambda: [numpy_condition(group, fixed, values, s) for s in sides], reps)
    res['set_group'] = spread(lambda: eng.set_joint_group(2, L.TPE_JOINT_STREAM, dims, *(cond[0] + cond[1])), reps)
    res['host_path'] = spread(host_path, reps)
    res['host_path_over_condition'] = res['host_path']['median_ms'] / res['condition']['median_ms']
    eng.close()
    hist = workloads.History(group, tids, losses, obs)
    domain = Domain(lambda d: 0.0, workloads.hp_space(group))
    held = {group[d][0]: v for d, v in zip(fixed, values)}
    for leg, kw in (('suggest', {}), ('suggest_fixed', dict(fixed=held))):
        trials = workloads.history_trials(hist)
        kw = dict(kw, **dev_kw)
        res[leg] = spread(lambda: tpe.suggest([n_trials], domain, trials, 3, multivariate=True,
                                              posterior_builder='device', **kw), reps)
    return res


def quality_bandwidth(evals=100, seeds=10):
    """The three quality objectives above with joint_bandwidth 'neighbour' and
    'scott' (each with the joint keyword its space needs), and the independent
    call beside them: the best losses of `seeds` runs and their medians."""
    import hyperopt_amd as H
    from hyperopt_amd import hp, tpe
    centre = (-3.0, 0.0, 3.0)
    objectives = (
        ('coupled', '(x-y)^2 + 0.01 (x+y)^2 on uniform(-5,5)^2',
         {'x': hp.uniform('x', -5, 5), 'y': hp.uniform('y', -5, 5)},
         lambda d: (d['x'] - d['y']) ** 2 + 0.01 * (d['x'] + d['y']) ** 2, {}),
        ('quantized', '(x-n)^2 + 0.01 (x+n)^2, x uniform(-5,5), n quniform(-5,5,1)',
         {'x': hp.uniform('x', -5, 5), 'n': hp.quniform('n', -5, 5, 1)},
         lambda d: (d['x'] - d['n']) ** 2 + 0.01 * (d['x'] + d['n']) ** 2, dict(joint_quantized=True)),
        ('categorical', '(x - [-3,0,3][k])^2 + 0.1 k, x uniform(-5,5), k choice(3)',
         {'x': hp.uniform('x', -5, 5), 'k': hp.choice('k', [0, 1, 2])},
         lambda d: (d['x'] - centre[d['k']]) ** 2 + 0.1 * d['k'], dict(joint_categorical=True)))
    out = dict(evals=evals, seeds=seeds)
    for name, text, space, loss, joint_kw in objectives:
        rec = out[name] = dict(objective=text)
        modes = (('independent', {}),
                 ('neighbour', dict(multivariate=True, joint_bandwidth='neighbour', **joint_kw)),
                 ('scott', dict(multivariate=True, joint_bandwidth='scott', **joint_kw)))
        for mode, kw in modes:
            best = []
            for seed in range(seeds):
                trials = H.Trials()
                H.fmin(loss, space, algo=partial(tpe.suggest, **kw), max_evals=evals, trials=trials,
                       rstate=np.random.RandomState(seed))
                best.append(float(min(trials.losses())))
            rec[mode] = dict(best=best, median=float(np.median(best)))
    return out


def quality_categorical(evals=100, seeds=10):
    import hyperopt_amd as H
    from hyperopt_amd import hp, tpe
    space = {'x': hp.uniform('x', -5, 5), 'k': hp.choice('k', [0, 1, 2])}
    centre = (-3.0, 0.0, 3.0)

    def loss(d):
        return (d['x'] - centre[d['k']]) ** 2 + 0.1 * d['k']

    out = {}
    modes = (('independent', {}), ('multivariate', dict(multivariate=True)),
             ('multivariate_joint_categorical', dict(multivariate=True, joint_categorical=True)))
    for name, kw in modes:
        best = []
        for seed in range(seeds):
            trials = H.Trials()
            H.fmin(loss, space, algo=partial(tpe.suggest, **kw), max_evals=evals, trials=trials,
                   rstate=np.random.RandomState(seed))
            best.append(float(min(trials.losses())))
        out[name] = dict(best=best, median=float(np.median(best)))
    out.update(evals=evals, seeds=seeds, objective='(x - [-3,0,3][k])^2 + 0.1 k, x uniform(-5,5), k choice(3)')
    return out


def quality_quantized(evals=100, seeds=10):
    import hyperopt_amd as H
    from hyperopt_amd import hp, tpe
    space = {'x': hp.uniform('x', -5, 5), 'n': hp.quniform('n', -5, 5, 1)}

    def loss(d):
        return (d['x'] - d['n']) ** 2 + 0.01 * (d['x'] + d['n']) ** 2

    out = {}
    modes = (('independent', {}), ('multivariate', dict(multivariate=True)),
             ('multivariate_joint_quantized', dict(multivariate=True, joint_quantized=True)))
    for name, kw in modes:
        best = []
        for seed in range(seeds):
            trials = H.Trials()
            H.fmin(loss, space, algo=partial(tpe.suggest, **kw), max_evals=evals, trials=trials,
                   rstate=np.random.RandomState(seed))
            best.append(float(min(trials.losses())))
        out[name] = dict(best=best, median=float(np.median(best)))
    out.update(evals=evals, seeds=seeds, objective='(x-n)^2 + 0.01 (x+n)^2, x uniform(-5,5), n quniform(-5,5,1)')
    return out


def quality(evals=100, seeds=10):
    import hyperopt_amd as H
    from hyperopt_amd import hp, tpe
    space = {'x': hp.uniform('x', -5, 5), 'y': hp.uniform('y', -5, 5)}

    def loss(d):
        return (d['x'] - d['y']) ** 2 + 0.01 * (d['x'] + d['y']) ** 2

    out = {}
    for name, mv in (('independent', False), ('multivariate', True)):
        best = []
        for seed in range(seeds):
            trials = H.Trials()
            H.fmin(loss, space, algo=partial(tpe.suggest, multivariate=mv), max_evals=evals, trials=trials,
                   rstate=np.random.RandomState(seed))
            best.append(float(min(trials.losses())))
        out[name] = dict(best=best, median=float(np.median(best)))
    out.update(evals=evals, seeds=seeds, objective='(x-y)^2 + 0.01 (x+y)^2 on uniform(-5,5)^2')
    return out


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', type=int, default=32)
    ap.add_argument('--trials', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--quality', action='store_true')
    ap.add_argument('--no-timings', action='store_true')
    ap.add_argument('--groups', action='store_true', help='the loop and batch legs over several groups and ids')
    ap.add_argument('--quantized', action='store_true', help='the dense and quantized d32 legs')
    ap.add_argument('--quality-quantized', action='store_true')
    ap.add_argument('--categorical', action='store_true', help='the dense and categorical d32 legs')
    ap.add_argument('--quality-categorical', action='store_true')
    ap.add_argument('--build', action='store_true', help='the device joint build against the host build')
    ap.add_argument('--fixed', action='store_true', help='Engine.joint_condition against the host path it replaces')
    ap.add_argument('--fix', type=int, default=8, help='--fixed: how many labels are held')
    ap.add_argument('--quality-bandwidth', action='store_true',
                    help="the three quality objectives with joint_bandwidth 'neighbour' and 'scott'")
    ap.add_argument('--legs', default=None,
                    help='--groups: loop,batch; --quantized: dense,quantized; --categorical: dense,categorical; '
                         '--build: ' + ','.join(BUILD_LEGS))
    ap.add_argument('--devices', default=None, help='ordinals of a multi-device engine, e.g. 0,0 (--quantized, '
                                                    '--categorical, --build)')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if a.devices:
        global DEVICES
        DEVICES = [int(d) for d in a.devices.split(',')]
    res = {}
    if a.groups:
        res['groups'] = groups_timings(a.reps, legs=tuple((a.legs or 'loop,batch').split(',')))
    elif a.quantized:
        res['quantized'] = quantized_timings(a.reps, legs=tuple((a.legs or 'dense,quantized').split(',')))
    elif a.categorical:
        res['categorical'] = categorical_timings(a.reps, legs=tuple((a.legs or 'dense,categorical').split(',')))
    elif a.build:
        res['build'] = build_timings(a.reps, a.dims, a.trials, legs=tuple(a.legs.split(',')) if a.legs else BUILD_LEGS)
    elif a.fixed:
        res['fixed'] = fixed_timings(a.reps, a.dims, a.trials, a.fix)
    elif not a.no_timings:
        res['timings'] = timings(a.dims, a.trials, a.reps)
    if a.quality:
        res['quality'] = quality()
    if a.quality_quantized:
        res['quality_quantized'] = quality_quantized()
    if a.quality_categorical:
        res['quality_categorical'] = quality_categorical()
    if a.quality_bandwidth:
        res['quality_bandwidth'] = quality_bandwidth()
    txt = json.dumps(res, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
