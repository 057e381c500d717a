"""Timings of the pairwise interactions (tpe.interactions; needs the GPU).

    python tools/time_interactions.py --gpus 1 [--configs 3,5] [--n-grid 256] [--reps 10] [--out FILE] [--mixed]

On the histories of config 3 (workloads.mixed_history: 32 labels x 10000
trials) and config 5 (128 labels x 50000 trials), quantile 0.1, the dense
labels forming one group:

* tpe.interactions end to end on a Trials object holding the history (wall;
  median of --reps calls after a warm-up call, the history cache warm);
* Engine.interactions alone on the same group (wall: upload, kernels, one
  synchronisation);
* the pair kernel's device time (HIP events around it,
  Engine.interactions_last_pair_ms; median over the same calls) and its fp64
  rate, 2 G^2 (Kb + Ka) FLOP per pair, next to the 78.6 TFLOP/s of the
  project's roofline; and what grows with the pairs in all -- the norm,
  marginal, pair and sum kernels -- as the slope of Engine.interactions
  between the pair list and the pair list given twice;
* the numpy path: U_d^T diag(W) U_e with np.dot, the marginals and the
  per-cell arithmetic vectorised, on the first --host-pairs pairs, scaled to
  all pairs; and the largest relative difference of H and V between it and
  the device.

--mixed times tpe.interactions(mixed=True) instead: every label of the config
(its quantized and categorical ones included) in one group,
Engine.interactions_mixed, its pair kernels, the numpy path with the interval
masses by scipy.special and the categorical rows, and next to them the
dense-only call on the same history (profiles/interactions_mixed_timing.json).

One JSON object per config is printed; --out is written anew by every run, one
line per config of that run (profiles/interactions_timing.json)."""
import argparse
import itertools
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUANTILE = 0.1
PEAK_FP64_MATRIX = 78.6e12


def timed(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def factor(y, mu, s):
    """u[k, i]: the normal densities of the components at the cells."""
    with np.errstate(invalid='ignore'):
        z = (np.asarray(y)[None, :] - mu[:, None]) / s[:, None]
        return np.exp(-0.5 * (z * z)) / (s[:, None] * 2.5066282746310002)


def masses(mu, s, low, high):
    """The components' mass inside [low, high] (1 without bounds), from tails."""
    if low != low or high != high:
        return np.ones(len(mu))
    tail = np.vectorize(lambda x: 0.5 * math.erfc(x / math.sqrt(2.0)))
    a, b = (low - mu) / s, (high - mu) / s
    return np.where(a >= 0, tail(a) - tail(b), np.where(b <= 0, tail(-b) - tail(-a), 1.0 - tail(-a) - tail(b)))


def host_pair(below, above, d, e, y, h, bounds, alpha):
    """(H, V) of one pair in numpy: the matrix products by np.dot, the
    per-cell arithmetic of tpe_interactions vectorised."""
    planes = []
    for W, mu, s in (below, above):
        ud, ue = factor(y[d], mu[:, d], s[:, d]), factor(y[e], mu[:, e], s[:, e])
        md, me = masses(mu[:, d], s[:, d], *bounds[d]), masses(mu[:, e], s[:, e], *bounds[e])
        planes.append(host_planes(W, ud, ue, md, me))
    return host_cells(planes, alpha, h[d] * h[e])


def host_planes(W, ud, ue, md, me):
    A = np.sum(W * md * me)
    return np.dot((W[:, None] * ud).T, ue) / A, np.dot(ud.T, W * me) / A, np.dot(ue.T, W * md) / A


def mixed_factor(ax, mu, s, pw):
    """(u [K, G], m [K]) of one label under mixed=True (an InteractionAxis)."""
    from scipy.special import erf, erfc
    if ax.upper:
        a = ax.upper * pw / len(mu)
        r = (np.equal.outer(mu, np.arange(ax.upper)) + a * ax.p[None, :]) / (1.0 + a)
        r[0] = ax.p
        return r, np.ones(len(mu))
    m = masses(mu, s, ax.low, ax.high)
    if not ax.step:
        return factor(ax.x, mu, s), m
    ub, lb = ax.x + ax.step / 2.0, ax.x - ax.step / 2.0
    if ax.low == ax.low:
        ub, lb = np.minimum(ub, np.exp(ax.high) if ax.log else ax.high), np.maximum(lb, np.exp(ax.low) if ax.log else ax.low)
    if ax.log:
        ub, lb = np.log(np.maximum(ub, 1e-12)), np.log(np.maximum(np.maximum(lb, 0.0), 1e-12))
    zu, zl = (ub[None, :] - mu[:, None]) / (s[:, None] * math.sqrt(2.0)), (lb[None, :] - mu[:, None]) / (s[:, None] * math.sqrt(2.0))
    up, dn = zl >= 0, zu <= 0
    g = np.where(up, 0.5 * (erfc(zl) - erfc(zu)), np.where(dn, 0.5 * (erfc(-zu) - erfc(-zl)), 0.5 * (erf(zu) + erf(-zl))))
    return np.where(zu > zl, g, 0.0), m


def host_pair_mixed(below, above, d, e, axes, pw, alpha):
    planes = []
    for W, mu, s in (below, above):
        (ud, md), (ue, me) = mixed_factor(axes[d], mu[:, d], s[:, d], pw), mixed_factor(axes[e], mu[:, e], s[:, e], pw)
        planes.append(host_planes(W, ud, ue, md, me))
    return host_cells(planes, alpha, axes[d].measure * axes[e].measure)


def host_cells(planes, alpha, hh):
    (L, Ld, Le), (G, Gd, Ge) = planes
    om = 1.0 - alpha
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        p = alpha * L + om * G
        dev = alpha * om * (L - G) / p
        qi, ri = alpha * np.outer(Ld, Le), om * np.outer(Gd, Ge)
        mi, ci = qi / (qi + ri), ri / (qi + ri)
        dl = (np.log(L) - np.log(G)) - (np.log(np.outer(Ld, Le)) - np.log(np.outer(Gd, Ge)))
        t = np.expm1(-np.abs(dl))
        dif = np.where(dl <= 0, mi * ci * t / (1.0 + mi * t), -(mi * ci * t) / (1.0 + ci * t))
        dif = np.where(np.isfinite(dl), dif, alpha * L / p - mi)
        dif = np.where(qi + ri == 0, dev, dif)
        return hh * np.sum(np.where(p == 0, 0.0, p * dif * dif)), hh * np.sum(np.where(p == 0, 0.0, p * dev * dev))


def run(n_labels, n_trials, args):
    from hyperopt_amd import Domain, posterior as P, tpe
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.workloads import history_trials, hp_space, mixed_history
    hist = mixed_history(n_labels, n_trials, seed=0)
    rec = dict(what='interactions', labels=n_labels, trials=n_trials, n_grid=args.n_grid, quantile=QUANTILE)
    trials = history_trials(hist)
    domain = Domain(None, hp_space(hist.labels))
    rec['tpe_interactions'] = timed(lambda: tpe.interactions(domain, trials, quantile=QUANTILE, n_grid=args.n_grid),
                                    args.reps)
    got = tpe.interactions(domain, trials, quantile=QUANTILE, n_grid=args.n_grid)
    names = list(tpe.specs_of(domain))
    dense = [l for l in sorted(hist.labels, key=lambda l: names.index(l[0])) if l[1] in P.JOINT_KINDS]
    n = len(hist.tids)
    nb = int(np.ceil(QUANTILE * n))
    sp = P.Splitter(hist.tids, hist.losses, 0.0, n_below=nb)
    mixes = [P.joint_mixture([dense[0], l], hist.obs, sp, 1.0, bandwidth='scott') for l in dense[1:]]
    below = (mixes[0].wb, np.column_stack([mixes[0].mub[:, 0]] + [m.mub[:, 1] for m in mixes]),
             np.column_stack([mixes[0].sigb[:, 0]] + [m.sigb[:, 1] for m in mixes]))
    above = (mixes[0].wa, np.column_stack([mixes[0].mua[:, 0]] + [m.mua[:, 1] for m in mixes]),
             np.column_stack([mixes[0].siga[:, 0]] + [m.siga[:, 1] for m in mixes]))
    ax = [P.interaction_axis(l[1], l[2], hist.obs[l[0]][1], args.n_grid) for l in dense]
    y, h = [a[0] for a in ax], [a[1] for a in ax]
    pri = [P.joint_prior(l[1], l[2]) for l in dense]
    bounds = [(p.low, p.high) if p.bounded else (np.nan, np.nan) for p in pri]
    lo, hi = zip(*bounds)
    pairs = list(itertools.combinations(range(len(dense)), 2))
    alpha = nb / n
    eng = get_engine(0, 'f64', 'importance')
    call = lambda pr: eng.interactions(y, h, lo, hi, below, above, alpha, pr)
    rec.update(dense_labels=len(dense), pairs=len(pairs), Kb=len(below[0]), Ka=len(above[0]))
    pair_ms = []
    rec['engine_interactions'] = timed(lambda: (call(pairs), pair_ms.append(eng.interactions_last_pair_ms())),
                                       args.reps)
    rec['engine_interactions_pairs_twice'] = timed(lambda: call(pairs + pairs), args.reps)
    H, V = call(pairs)
    rec['same_as_public'] = bool([got[dense[d][0], dense[e][0]] for d, e in pairs] == H.tolist())
    slope_ms = rec['engine_interactions_pairs_twice']['median_ms'] - rec['engine_interactions']['median_ms']
    flop = 2.0 * args.n_grid ** 2 * (len(below[0]) + len(above[0])) * len(pairs)
    ms = float(np.median(pair_ms[1:]))
    rec['pair_kernel'] = dict(median_ms=ms, min_ms=float(min(pair_ms[1:])), max_ms=float(max(pair_ms[1:])),
                              gemm_flop=flop, fp64_flops=flop / (ms * 1e-3),
                              share_of_matrix_peak=flop / (ms * 1e-3) / PEAK_FP64_MATRIX)
    rec['per_pair_kernels_slope_ms'] = slope_ms
    sub = pairs[:args.host_pairs]
    t0 = time.perf_counter()
    ref = [host_pair(below, above, d, e, y, h, bounds, alpha) for d, e in sub]
    dt = (time.perf_counter() - t0) * 1e3
    rec['host_reference'] = dict(pairs=len(sub), ms=dt, ms_scaled_to_all_pairs=dt * len(pairs) / len(sub))
    rec['host_max_rel_diff_H'] = float(max(abs(r[0] - H[i]) / H[i] for i, r in enumerate(ref)))
    rec['host_max_rel_diff_V'] = float(max(abs(r[1] - V[i]) / V[i] for i, r in enumerate(ref)))
    rec['host_over_engine'] = rec['host_reference']['ms_scaled_to_all_pairs'] / rec['engine_interactions']['median_ms']
    rec['top3'] = [(list(k), v) for k, v in list(got.items())[:3]]
    return rec


def run_mixed(n_labels, n_trials, args):
    from hyperopt_amd import Domain, posterior as P, tpe
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.workloads import history_trials, hp_space, mixed_history
    hist = mixed_history(n_labels, n_trials, seed=0)
    rec = dict(what='interactions_mixed', labels=n_labels, trials=n_trials, n_grid=args.n_grid, quantile=QUANTILE)
    trials = history_trials(hist)
    domain = Domain(None, hp_space(hist.labels))
    kw = dict(quantile=QUANTILE, n_grid=args.n_grid)
    rec['tpe_interactions_mixed'] = timed(lambda: tpe.interactions(domain, trials, mixed=True, **kw), args.reps)
    rec['tpe_interactions_dense_only'] = timed(lambda: tpe.interactions(domain, trials, **kw), args.reps)
    got = tpe.interactions(domain, trials, mixed=True, **kw)
    names = list(tpe.specs_of(domain))
    group = sorted(hist.labels, key=lambda l: names.index(l[0]))
    n = len(hist.tids)
    nb = int(np.ceil(QUANTILE * n))
    sp = P.Splitter(hist.tids, hist.losses, 0.0, n_below=nb)
    mixes = [P.joint_mixture([group[0], l], hist.obs, sp, 1.0, quantized=True, categorical=True, bandwidth='scott')
             for l in group[1:]]
    below = (mixes[0].wb, np.column_stack([mixes[0].mub[:, 0]] + [m.mub[:, 1] for m in mixes]),
             np.column_stack([mixes[0].sigb[:, 0]] + [m.sigb[:, 1] for m in mixes]))
    above = (mixes[0].wa, np.column_stack([mixes[0].mua[:, 0]] + [m.mua[:, 1] for m in mixes]),
             np.column_stack([mixes[0].siga[:, 0]] + [m.siga[:, 1] for m in mixes]))
    axes = [P.interaction_axis_record(l[1], l[2], hist.obs[l[0]][1], args.n_grid) for l in group]
    pairs = list(itertools.combinations(range(len(group)), 2))
    alpha = nb / n
    eng = get_engine(0, 'f64', 'importance')
    call = lambda pr: eng.interactions_mixed(axes, below, above, 1.0, alpha, pr)
    narrow = [len(a.x) <= 16 for a in axes]
    shape = [int(narrow[d]) + int(narrow[e]) for d, e in pairs]
    rec.update(group_labels=len(group), pairs=len(pairs), Kb=len(below[0]), Ka=len(above[0]),
               cells=[len(a.x) for a in axes], pairs_wide_wide=shape.count(0), pairs_narrow_wide=shape.count(1),
               pairs_narrow_narrow=shape.count(2))
    pair_ms = []
    rec['engine_interactions_mixed'] = timed(lambda: (call(pairs), pair_ms.append(eng.interactions_last_pair_ms())),
                                             args.reps)
    H, V = call(pairs)
    rec['same_as_public'] = bool([got[group[d][0], group[e][0]] for d, e in pairs] == H.tolist())
    flop = 2.0 * (len(below[0]) + len(above[0])) * sum(len(axes[d].x) * len(axes[e].x) for d, e in pairs)
    ms = float(np.median(pair_ms[1:]))
    rec['pair_kernels'] = dict(median_ms=ms, min_ms=float(min(pair_ms[1:])), max_ms=float(max(pair_ms[1:])),
                               gemm_flop=flop, fp64_flops=flop / (ms * 1e-3),
                               share_of_matrix_peak=flop / (ms * 1e-3) / PEAK_FP64_MATRIX)
    for name, want in (('wide_wide', 0), ('narrow_wide', 1), ('narrow_narrow', 2)):   # each shape's pairs alone
        sub = [p for p, sh in zip(pairs, shape) if sh == want]
        if sub:
            one = []
            timed(lambda: (call(sub), one.append(eng.interactions_last_pair_ms())), args.reps)
            rec['pair_kernel_' + name] = dict(pairs=len(sub), median_ms=float(np.median(one[1:])),
                                              min_ms=float(min(one[1:])), max_ms=float(max(one[1:])))
    sub = [pairs[i] for i in np.linspace(0, len(pairs) - 1, args.host_pairs).astype(int)]
    t0 = time.perf_counter()
    ref = [host_pair_mixed(below, above, d, e, axes, 1.0, alpha) for d, e in sub]
    dt = (time.perf_counter() - t0) * 1e3
    rec['host_reference'] = dict(pairs=len(sub), ms=dt, ms_scaled_to_all_pairs=dt * len(pairs) / len(sub))
    at = [pairs.index(p) for p in sub]
    rec['host_max_rel_diff_H'] = float(max(abs(r[0] - H[i]) / H[i] for i, r in zip(at, ref)))
    rec['host_max_rel_diff_V'] = float(max(abs(r[1] - V[i]) / V[i] for i, r in zip(at, ref)))
    rec['host_over_engine'] = rec['host_reference']['ms_scaled_to_all_pairs'] / \
        rec['engine_interactions_mixed']['median_ms']
    rec['top3'] = [(list(k), v) for k, v in list(got.items())[:3]]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--configs', default='3')
    ap.add_argument('--n-grid', type=int, default=256)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-pairs', type=int, default=4)
    ap.add_argument('--out', default=None)
    ap.add_argument('--mixed', action='store_true')
    args = ap.parse_args()
    shapes = {3: (32, 10000), 5: (128, 50000)}
    lines = []
    for cfg in (int(c) for c in args.configs.split(',')):
        rec = (run_mixed if args.mixed else run)(*shapes[cfg], args)
        rec['config'] = cfg
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if args.out:   # (rewritten after every config: a run that is cut short keeps what it has)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
