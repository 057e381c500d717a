"""The mixtures the draw tests share (test_draw_oracle.py on the CPU,
test_gpu_draws.py on the device), as keyword arguments of
oracle.draw_oracle.fold / Engine.GMM1 / Engine.LGMM1."""
import numpy as np

from tests import golden_io

W4, MU4, S4 = [.1, .3, .4, .2], [1.0, 2.0, 3.0, 4.0], [.1, .4, .8, 2.0]


def _k26():
    """A 26-component below posterior as the Parzen estimator builds one: 25
    observations of the golden uniform(4, 7) label (every 11th of its
    300-trial above mixture's means, the prior's left out) plus the prior."""
    from hyperopt_amd.posterior import adaptive_parzen_normal
    rec = next(r for m, r in golden_io.cases('labels_small.npz')
               if m['kind'] == 'uniform' and m['n_hist'] == 300 and m['variant'] == 'plain')
    mus = rec['mu_a'][rec['mu_a'] != 5.5][::11][:25]
    assert len(mus) == 25
    w, m, s = adaptive_parzen_normal(mus, 1.0, 5.5, 3.0)
    return dict(w=w, mu=m, sigma=s, low=4.0, high=7.0)


def _random(K, seed, low=None, high=None):
    rng = np.random.RandomState(seed)
    mu = np.sort(rng.uniform(-5.0, 5.0, K))
    if low is not None:
        mu[0], mu[1] = low, low - 0.25          # (a mean on the lower bound and one below it: mirrored)
    sigma = np.exp(rng.uniform(np.log(0.01), np.log(3.0), K))
    w = rng.gamma(0.7, size=K)
    return dict(w=w / w.sum(), mu=mu, sigma=sigma, low=low, high=high)


# six cumulative weights strictly inside the cell [128, 129) / 256: the
# staged pick's guide would need six comparisons there (the branch-free search)
CELL6 = dict(w=[.5] + [1e-4] * 6 + [.5 - 6e-4], mu=[0., 1., 2., 3., 4., 5., 6., 7.],
             sigma=[1., .5, .25, 2., .1, 1., 3., .5])

_CELL6_W64 = np.array([0.5 / 29] * 29 + [1e-4] * 6 + [(0.5 - 6e-4) / 29] * 29)

MIXTURES = {
    'one': dict(w=[1.0], mu=[0.0], sigma=[1.0]),
    'w4': dict(w=W4, mu=MU4, sigma=S4),
    'w4_2.5_3.5': dict(w=W4, mu=MU4, sigma=S4, low=2.5, high=3.5),
    'w4_-1_0.5': dict(w=W4, mu=MU4, sigma=S4, low=-1.0, high=0.5),
    'w4_9_12': dict(w=W4, mu=MU4, sigma=S4, low=9.0, high=12.0),
    'tiny_w': dict(w=[2.0 ** -30, 1 - 2.0 ** -30, 2.0 ** -31], mu=[0.0, 5.0, -3.0], sigma=[1.0, .5, 2.0]),
    'narrow': dict(w=[.5, .5], mu=[0.0, 1.0], sigma=[1e-3, 1e-3], low=0.0, high=1.0),
    'k26': _k26(),
    'k65': _random(65, 65, low=-5.0, high=5.0),
    'k200': _random(200, 200),
    'cell6': CELL6,
    # 64 near-equal weights, staged, at most one cumulative weight per guide cell: the guided pick
    'k64': dict(w=(1.0 + 0.25 * np.cos(np.arange(64))) / np.sum(1.0 + 0.25 * np.cos(np.arange(64))),
                mu=np.linspace(-4.0, 4.0, 64), sigma=np.full(64, 0.3)),
    # the same weights on well-separated components, quantized: a pick of the
    # neighbouring component always changes the value (the quantized kernels stage the guided pick)
    'k64_q': dict(w=(1.0 + 0.25 * np.cos(np.arange(64))) / np.sum(1.0 + 0.25 * np.cos(np.arange(64))),
                  mu=np.linspace(-63.0, 63.0, 64), sigma=np.full(64, 0.3), q=0.5),
    # quantized, well-separated components (a neighbouring pick changes the value) for the two other
    # picks of the quantized kernels: 64 components with six cumulative weights inside one 1/256 cell
    # (steps > kGuideSteps: the staged branch-free search over all 64), and 65 components (not staged:
    # the binary search on the records in global memory)
    'cell6_q': dict(w=_CELL6_W64, mu=np.linspace(-63.0, 63.0, 64), sigma=np.full(64, 0.3), q=0.5),
    'k65_q': dict(w=(1.0 + 0.25 * np.cos(np.arange(65))) / np.sum(1.0 + 0.25 * np.cos(np.arange(65))),
                  mu=np.linspace(-64.0, 64.0, 65), sigma=np.full(65, 0.3), q=0.5),
    'w4_log': dict(w=W4, mu=[-2.0, 1.0, 0.0, 3.0], sigma=S4, log=True),
    'w4_q': dict(w=W4, mu=MU4, sigma=S4, q=0.5),
    'w4_2.5_3.5_log': dict(w=W4, mu=MU4, sigma=S4, low=2.5, high=3.5, log=True),
    'w4_2.5_3.5_q': dict(w=W4, mu=MU4, sigma=S4, low=2.5, high=3.5, q=0.5),
    'w4_2.5_3.5_logq': dict(w=W4, mu=MU4, sigma=S4, low=2.5, high=3.5, log=True, q=0.5),
}

P3 = np.array([.2, .5, .3])
_p70 = np.random.RandomState(70).gamma(0.5, size=70) + 1e-6
P70 = _p70 / _p70.sum()


def fold_of(name):
    from oracle import draw_oracle as D
    return D.fold(**MIXTURES[name])


def engine_kwargs(name):
    """(sampler name, positional (w, mu, sigma), keyword bounds / q)."""
    c = MIXTURES[name]
    kw = {k: c[k] for k in ('low', 'high', 'q') if c.get(k) is not None}
    return ('LGMM1' if c.get('log') else 'GMM1'), (c['w'], c['mu'], c['sigma']), kw


def fold_posterior(p):
    """The fold of a LabelPosterior's below mixture."""
    from oracle import draw_oracle as D
    if p.family == 'categorical':
        return D.fold(p.below)
    w, mu, sigma = p.below
    return D.fold(w, mu, sigma, low=p.low, high=p.high, log=p.family == 'LGMM1', q=p.q)


# -- the device tests' words: (offset, stream, round, seed) corners of the
# entry points, the small rounds' posterior, the tile rounds' workload ------
BIG_SEED = 0x9e3779b97f4a7c15          # key word k1 != 0
N_ENTRY = (1 << 16) + 1
TOP = (1 << 32) - (1 << 16) - 2        # offset + N_ENTRY = 2^32 - 1, the counter's top
CORNERS = [(0, 0, 0, 234), (1, 0, 0, 234), (TOP, 0, 0, 234), (0, 7, 0, 234), (0, 0, 0xfffffffe, BIG_SEED),
           (0, 0, 0, BIG_SEED), (1, 7, 0, 234), (TOP, 0, 0xfffffffe, BIG_SEED), (1, 7, 0xfffffffe, BIG_SEED),
           (TOP, 7, 0xfffffffe, 234)]
ENTRY_NAMES = sorted(MIXTURES) + ['p3', 'p70']


def entry_fold(name):
    from oracle import draw_oracle as D
    if name in ('p3', 'p70'):
        return D.fold(P3 if name == 'p3' else P70)
    return fold_of(name)


# small rounds: every label's below mixture is one of the above; the above
# mixtures are wide (a one-candidate round returns its candidate whatever it
# scores)
ROUND_LABELS = ['one', 'k26', 'cell6', 'k65', 'w4_2.5_3.5', 'w4_9_12', 'w4_log', 'w4_q', 'w4_2.5_3.5_logq',
                'p3', 'p70', 'k64', 'k64_q', 'cell6_q', 'k65_q']
ROUND_G = list(range(64)) + [(1 << 32) - 2]
ROUND_IDS = list(range(64))
ROUND_SEEDS = (2024, BIG_SEED)


# The packed map draws and scores its quantized labels in one kernel
# (k_qfused) when every quantized label has both bounds and a grid of at most
# half the round's slots; else k_qsample draws them.  The second posterior
# swaps the unbounded quantized labels for bounded ones at the same places
# (so the same Philox streams): the bounds of the three wide ones lie more
# than 20 sigma outside every component, so each m_k is exactly 1 and the
# thresholds -- and THRESHOLD_WORDS -- are the unbounded labels'.
FUSED_ONLY = {name + 'b': dict(MIXTURES[name], low=-70.0, high=70.0) for name in ('k64_q', 'cell6_q', 'k65_q')}
FUSED_LABELS = [{'w4_q': 'w4_2.5_3.5_q', 'k64_q': 'k64_qb', 'cell6_q': 'cell6_qb', 'k65_q': 'k65_qb'}.get(n, n)
                for n in ROUND_LABELS]
FUSED_IDS = list(range(600))            # 600 slots per label: twice the widest grid (283 values)
FUSED_G = [0, 1, 2, 3, (1 << 32) - 2]


def round_posterior(labels=None):
    from hyperopt_amd.posterior import LabelPosterior
    posts = []
    for name in (ROUND_LABELS if labels is None else labels):
        if name in ('p3', 'p70'):
            p = P3 if name == 'p3' else P70
            posts.append(LabelPosterior(name, 'categorical', p, np.full(len(p), 1.0 / len(p)), upper=len(p)))
            continue
        c = MIXTURES[name] if name in MIXTURES else FUSED_ONLY[name]
        mu = np.asarray(c['mu'], float)
        above = (np.array([.5, .5]), np.array([mu.min() - 1.0, mu.max() + 1.0]), np.array([4.0, 4.0]))
        below = tuple(np.asarray(c[k], float) for k in ('w', 'mu', 'sigma'))
        posts.append(LabelPosterior(name, 'LGMM1' if c.get('log') else 'GMM1', below, above,
                                    low=c.get('low'), high=c.get('high'), q=c.get('q')))
    return posts


# tile rounds: the smallest mixed workload whose rounds of >= 8192 candidates
# run the expansion screen behind the hot-bin prefilter (5 labels, one of each
# kind; ~296 above components per label)
TILE_WORKLOAD = (5, 300, 0)
TILE_ROUNDS = [(1024, 17, 3), (8192, BIG_SEED, 4), (8193, 17, 5), (1 << 16, BIG_SEED, 0xfffffffe)]   # (C, seed, round)


def tile_posteriors():
    from hyperopt_amd.workloads import mixed_history
    return mixed_history(*TILE_WORKLOAD).posteriors()


# Candidates whose pick word lands on a threshold (thr[k] - 1 or thr[k]): found
# by scanning g for (seed ROUND_SEEDS[0], round 0, stream = the label's place
# in ROUND_LABELS).  The labels are unbounded or categorical, so their
# thresholds hold no erfc and are the same integers on every machine; random
# draws never reach these words (~K 2^-32 each).
THRESHOLD_WORDS = {
    'cell6': [18682500],
    'p3': [62693116],
    'p70': [61681521, 76653018, 103036276, 132567950, 190956479, 204747033, 256462505],
    'k64': [19683270, 47799345, 57396504, 86826280, 92587096, 108886289, 170465361, 172292556, 212769099],
    'k64_q': [25362739, 105801177, 125224430, 128159603, 133931155, 138366456, 165159890],
    'cell6_q': [97521711, 114216308, 131990068, 140631736, 141596083, 151359531, 165390644],
    'k65_q': [30828660, 38513005, 86325147, 115394174, 147105093, 148275077, 150814855, 233413371, 242314191],
}


def golden_fold(meta, rec):
    """The fold of a golden label case's below mixture (golden_io.cases)."""
    from oracle import draw_oracle as D
    if meta['sampler'] == 'categorical':
        return D.fold(rec['p_below'])
    kw = meta['lpdf_kwargs']
    return D.fold(rec['w_b'], rec['mu_b'], rec['sigma_b'], low=kw.get('low'), high=kw.get('high'),
                  log=meta['sampler'] == 'LGMM1', q=kw.get('q'))


def fused_round_cases():
    """test_gpu_parity.test_fused_round_matches_oracle's labels, seed, round
    and candidate counts."""
    pairs = [(m, r) for fx in ('labels_small.npz', 'labels_medium.npz') for m, r in golden_io.cases(fx)
             if m['n_hist'] in (26, 300) and m['variant'] == 'plain']
    return pairs, 12345, 7, (24, 700, 3000)
