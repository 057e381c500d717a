"""Posteriors at the smallest shapes that still take each branch of the
expansion index (hyperopt_amd/csrc/tpe_expand.hip): the case table of
tests/test_bx_index_gpu.py and tests/test_bx_reference_host.py.

A case is a list of LabelPosterior (posterior.pack packs it).  Observations
come from workloads.prior_draw with a fixed RandomState; the first
n_below = ceil(0.25 sqrt(N)) of them are the below set (the draws are
i.i.d., so this is a random split), the rest the above set; the mixtures are
posterior.label_posterior's unless the case is hand-built.

index_shape() restates bx_build's host arithmetic (the clipped scale, the
counts, the bins it wants) so that the host test can check that every case
reaches the branch it is listed for without a GPU.
"""
import math

import numpy as np

from hyperopt_amd import posterior as P
from hyperopt_amd.workloads import prior_draw

K_MIN_BINS, K_MAX_BINS, K_MAX_UNCLIPPED, K_SUB = 64, 1 << 16, 16384, 16
K_STAGE_BELOW = K_SAMP_LDS = 64
K_RANGE_TAIL = 1e-10
T_TILE = 64.0


def want_factor(T=T_TILE):
    """bx_build: want = range / sigma* x sqrt(2 T ln 2) (9.42 at T = 64)."""
    return math.sqrt(2.0 * T * math.log(2.0))


def _split(kind, args, N, seed, edit=None):
    obs = prior_draw(kind, args, np.random.RandomState(seed), N)
    if edit is not None:
        edit(obs)
    nb = int(math.ceil(0.25 * math.sqrt(N)))
    return obs[:nb], obs[nb:]


def _label(name, kind, args, N, seed, edit=None):
    below, above = _split(kind, args, N, seed, edit)
    return P.label_posterior(name, kind, args, below, above, 1.0)


def _norm(w):
    w = np.asarray(w, dtype=float)
    return w / w.sum()


def uniform300():
    return _label('uniform300', 'uniform', dict(low=-5.0, high=5.0), 300, 11)


def uniform3():
    return _label('uniform3', 'uniform', dict(low=-5.0, high=5.0), 3, 13)


def normal30():
    return _label('normal30', 'normal', dict(mu=0.0, sigma=3.0), 30, 32)


def lognormal150():
    return _label('lognormal150', 'lognormal', dict(mu=0.0, sigma=1.0), 150, 14)


def loguniform_far():
    return _label('loguniform_far', 'loguniform', dict(low=-20.0, high=-10.0), 120, 15)


def offset1e6():
    return _label('offset1e6', 'uniform', dict(low=1e6, high=1e6 + 1.0), 300, 16)


def ties50():
    def edit(obs):
        obs[10:60] = obs[10]          # 50 equal observations, all in the above set
    return _label('ties50', 'uniform', dict(low=0.0, high=1.0), 120, 17, edit)


def at_bounds():
    def edit(obs):
        obs[10:20] = 0.0
        obs[20:30] = 1.0
    return _label('at_bounds', 'uniform', dict(low=0.0, high=1.0), 120, 18, edit)


def all_clipped():
    """Hand-built: 200 above components at one sigma (n_nc = 0), 5 below."""
    rng = np.random.RandomState(19)
    mu_a = np.sort(rng.uniform(0.0, 1.0, 200))
    above = (_norm(np.ones(200)), mu_a, np.full(200, 0.02))
    below = (_norm([1.0, 1.0, 1.0, 1.0, 1.0]), np.array([0.21, 0.33, 0.5, 0.52, 0.8]),
             np.array([0.05, 0.08, 1.0, 0.03, 0.1]))
    return P.LabelPosterior('all_clipped', 'GMM1', below, above, low=0.0, high=1.0)


def zero_weight():
    p = uniform300()
    wb, mb, sb = (np.array(a) for a in p.below)
    wa, ma, sa = (np.array(a) for a in p.above)
    wb[2] = 0.0
    wa[[7, 150, 290]] = 0.0
    return P.LabelPosterior('zero_weight', 'GMM1', (_norm(wb), mb, sb), (_norm(wa), ma, sa),
                            low=p.low, high=p.high)


def zero_above():
    """zero_weight's three zero above weights alone: the below mixture keeps
    every weight, so the expansion screen certifies (a zero below weight
    makes its one-pass below sum NaN) and its tables and lists are checked
    with c = -inf records among the sorted above records."""
    p = uniform300()
    wa, ma, sa = (np.array(a) for a in p.above)
    wa[[7, 150, 290]] = 0.0
    return P.LabelPosterior('zero_above', 'GMM1', p.below, (_norm(wa), ma, sa), low=p.low, high=p.high)


def _wide_below(n, seed):
    """n below components over uniform300's range: sigmas 0.1 .. 0.3, at
    least 100 of that index's sub-bins (10 / 960 / 16 = 6.5e-4) wide."""
    rng = np.random.RandomState(seed)
    mu = np.linspace(-4.5, 4.5, n)
    sg = rng.uniform(0.1, 0.3, n)
    w = _norm(rng.uniform(0.5, 1.5, n))
    return w, mu, sg


def below_n(n):
    p = uniform300()
    return P.LabelPosterior('below%d' % n, 'GMM1', _wide_below(n, 20 + n), p.above, low=p.low, high=p.high)


def _one_wide_many_clipped(name, want, seed):
    """Hand-built uniform(0, 1): a wide above component (so that no
    candidate's lpdf_above underflows) and 40 clipped ones whose sigma puts
    bx_build's `want` where the case needs it."""
    rng = np.random.RandomState(seed)
    sig = want_factor() / want
    mu_c = np.sort(rng.uniform(0.0, 1.0, 40))
    k = int(np.searchsorted(mu_c, 0.5))
    mu_a = np.insert(mu_c, k, 0.5)
    sg_a = np.insert(np.full(40, sig), k, 1.0)
    w_a = _norm(np.insert(np.ones(40), k, 40.0))
    below = (_norm([1.0, 2.0, 1.0, 1.0, 1.0]), np.array([0.1, 0.3, 0.5, 0.62, 0.9]),
             np.array([0.02, 0.01, 1.0, 0.04, 0.05]))
    return P.LabelPosterior(name, 'GMM1', below, (w_a, mu_a, sg_a), low=0.0, high=1.0)


def max_bins():
    return _one_wide_many_clipped('max_bins', 65100.0, 21)


def over_bins():
    return _one_wide_many_clipped('over_bins', 66500.0, 22)


def over_unclipped():
    """Hand-built: kMaxUnclipped + 1 = 16385 above components with distinct
    sigmas beside the one that carries the smallest (the clipped one)."""
    n = K_MAX_UNCLIPPED + 2
    rng = np.random.RandomState(23)
    mu_a = np.sort(rng.uniform(0.0, 1.0, n))
    sg_a = 0.004 + 0.012 * (rng.permutation(n) + 1.0) / n
    below = (_norm([1.0, 1.0, 1.0]), np.array([0.3, 0.5, 0.7]), np.array([0.05, 1.0, 0.1]))
    return P.LabelPosterior('over_unclipped', 'GMM1', below, (_norm(np.ones(n)), mu_a, sg_a),
                            low=0.0, high=1.0)


def permuted():
    p = uniform300()
    order = np.random.RandomState(24).permutation(len(p.above[0]))
    above = tuple(np.asarray(a)[order] for a in p.above)
    return P.LabelPosterior('permuted', 'GMM1', p.below, above, low=p.low, high=p.high)


def _quniform():
    return _label('q', 'quniform', dict(low=0.0, high=100.0, q=1.0), 120, 25)


def _randint():
    return _label('r', 'randint', dict(upper=5), 120, 26)


def three_labels():
    return [uniform3(), _quniform(), lognormal150(), _randint(), all_clipped()]


# name -> (builder, eligible for the expansion index)
CASES = {
    'uniform300': (uniform300, True),
    'uniform3': (uniform3, True),
    'normal30': (normal30, True),
    'lognormal150': (lognormal150, True),
    'loguniform_far': (loguniform_far, True),
    'offset1e6': (offset1e6, True),
    'ties50': (ties50, True),
    'at_bounds': (at_bounds, True),
    'all_clipped': (all_clipped, True),
    'zero_weight': (zero_weight, True),
    'zero_above': (zero_above, True),
    'below64': (lambda: below_n(64), True),
    'below65': (lambda: below_n(65), True),
    'below200': (lambda: below_n(200), True),
    'max_bins': (max_bins, True),
    'over_bins': (over_bins, False),
    'over_unclipped': (over_unclipped, False),
    'three_labels': (three_labels, True),
    # an above mixture out of mu order gets no index (tpe_set_posterior)
    'permuted': (permuted, False),
}
ELIGIBLE = [n for n, (_, e) in CASES.items() if e]
INELIGIBLE = [n for n, (_, e) in CASES.items() if not e]

_cache = {}


def posts(name):
    """The case's LabelPosterior list (built once, never modified)."""
    if name not in _cache:
        p = CASES[name][0]()
        _cache[name] = p if isinstance(p, list) else [p]
    return _cache[name]


def dense_labels(ps):
    return [i for i, p in enumerate(ps) if p.family != 'categorical' and p.q is None]


def index_shape(p, T=T_TILE):
    """bx_build's host arithmetic for one dense label: the clipped sigma
    (the smallest above sigma, i.e. the largest record scale), the clipped
    and unclipped counts, the recentred-free range of the bins, `want`, the
    bins and the sub-bin width."""
    wb, mb, sb = (np.asarray(a, dtype=float) for a in p.below)
    sa = np.asarray(p.above[2], dtype=float)
    sig = float(np.min(sa))
    n_cl = int(np.sum(sa == sig))
    n_nc = len(sa) - n_cl
    if p.low is not None:
        lo, hi = float(p.low), float(p.high)
    else:   # k_bx_scan: each sampling component to z sigma, w Q(z) <= kRangeTail
        with np.errstate(divide='ignore', invalid='ignore'):
            z = np.where(wb > K_RANGE_TAIL, np.minimum(8.0, np.sqrt(2.0 * np.log(wb / K_RANGE_TAIL))), 0.0)
        lo, hi = float(np.min(mb - z * sb)), float(np.max(mb + z * sb))
    want = (hi - lo) / sig * want_factor(T)
    nbins = max(K_MIN_BINS, (int(math.ceil(want)) + 63) // 64 * 64)
    return {'sigma': sig, 'n_cl': n_cl, 'n_nc': n_nc, 'lo': lo, 'hi': hi, 'want': want,
            'nbins': nbins, 'sub_width': (hi - lo) / nbins / K_SUB,
            'eligible': want <= K_MAX_BINS and n_nc <= K_MAX_UNCLIPPED and n_cl >= 1}
