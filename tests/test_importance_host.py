"""Hyperparameter importance, host side (no GPU): posterior.importance_cells,
the n_below argument of the split, the reference restatement itself
(tests/importance_reference.py) and tpe.importance's argument checks.  Nothing
here reaches an engine."""
import math

import numpy as np
import pytest

from hyperopt_amd import posterior as P
from tests import golden_io
from tests import importance_reference as R
from tests.helpers import ALL_KINDS, make_history

KINDS = {name: (kind, args) for name, kind, args in ALL_KINDS}
QUANT = ('qu', 'qlu', 'qn', 'qln')
GRIDS = (16, 64, 4096)


@pytest.fixture(scope='module')
def hist():
    return R.planted()


def working_range(name, obs):
    """[a, b] of the definition in the working space, written out per kind."""
    kind, args = KINDS[name]
    if 'low' in args:
        return args['low'], args['high']
    t = np.asarray(obs, dtype=float)
    if kind == 'lognormal':
        t = np.log(t)
    if kind == 'qlognormal':
        t = np.log(np.maximum(t, 1e-12))
    return (min(args['mu'], t.min()) - 4 * args['sigma'], max(args['mu'], t.max()) + 4 * args['sigma'])


def support(name, obs):
    """(k0, k1) of a quantized label: round(a / q) .. round(b / q) in x."""
    kind, args = KINDS[name]
    a, b = working_range(name, obs)
    if kind in ('qloguniform', 'qlognormal'):
        a, b = math.exp(a), math.exp(b)
        return max(int(np.round(a / args['q'])), 0), max(int(np.round(b / args['q'])), 0)
    return int(np.round(a / args['q'])), int(np.round(b / args['q']))


@pytest.mark.parametrize('n_grid', (1,) + GRIDS)
@pytest.mark.parametrize('name', ['u', 'lu', 'n', 'ln'])
def test_dense_cells(hist, name, n_grid):
    kind, args = KINDS[name]
    obs = hist.obs[name][1]
    x, w, merge = P.importance_cells(kind, args, obs, n_grid)
    a, b = working_range(name, obs)
    assert merge == 1 and len(x) == len(w) == n_grid
    h = (b - a) / n_grid
    mid = a + (np.arange(n_grid) + 0.5) * h
    if kind in ('uniform', 'normal'):
        assert np.array_equal(x, mid) and np.all(w == h)
        # the cells tile the range: their widths add up to it
        assert abs(w.sum() - (b - a)) <= 4 * n_grid * np.spacing(b - a)
    else:
        assert np.array_equal(x, np.exp(mid)) and np.array_equal(w, h * np.exp(mid))
    assert np.all(np.diff(x) > 0) or n_grid == 1
    if 'low' in args:
        lo, hi = (a, b) if kind == 'uniform' else (math.exp(a), math.exp(b))
        assert lo < x[0] and x[-1] < hi


def test_dense_known_ranges(hist):
    x, w, _ = P.importance_cells('uniform', KINDS['u'][1], [], 4)
    assert x.tolist() == [-3.75, -1.25, 1.25, 3.75] and w.tolist() == [2.5] * 4
    # no observation: the prior's mean +- 4 sigma
    x, w, _ = P.importance_cells('normal', KINDS['n'][1], [], 2)
    assert x.tolist() == [-6.0, 6.0] and w.tolist() == [12.0, 12.0]
    # an observation past mu + 4 sigma stretches the range by its own 4 sigma
    x, w, _ = P.importance_cells('normal', KINDS['n'][1], [20.0, -1.0], 1)
    assert x.tolist() == [(-13.0 + 32.0) / 2] and w.tolist() == [45.0]
    x, w, _ = P.importance_cells('lognormal', KINDS['ln'][1], [math.exp(2.0)], 1)
    assert abs(w[0] - 10.0 * x[0]) <= 1e-13 * w[0] and abs(x[0] - math.e) <= 1e-14 * math.e


@pytest.mark.parametrize('n_grid', (1,) + GRIDS)
@pytest.mark.parametrize('name', QUANT)
def test_quantized_cells(hist, name, n_grid):
    kind, args = KINDS[name]
    obs = hist.obs[name][1]
    x, w, merge = P.importance_cells(kind, args, obs, n_grid)
    k0, k1 = support(name, obs)
    S = k1 - k0 + 1
    assert merge == -(-S // n_grid) and len(x) == len(w) == -(-S // merge) <= n_grid
    assert np.all(w == 1.0)
    # a cell is `merge` consecutive support values, x their mean; together
    # they cover the support once (the last cell may reach past it)
    ks = k0 + np.arange(len(x) * merge).reshape(len(x), merge)
    assert np.array_equal(x, ks.mean(axis=1) * args['q'])
    assert ks[0, 0] == k0 and ks[-1, 0] <= k1 <= ks[-1, -1]
    if n_grid == 1:
        assert len(x) == 1 and merge == S


def test_quantized_known_counts():
    # quniform(0, 20, q=1): 21 values; qloguniform(0, 4, q=1): 1 .. round(e^4) = 55
    want = {('qu', 16): (2, 11), ('qu', 64): (1, 21), ('qu', 4096): (1, 21),
            ('qlu', 16): (4, 14), ('qlu', 64): (1, 55), ('qlu', 4096): (1, 55)}
    for (name, n_grid), (merge, cells) in want.items():
        x, w, m = P.importance_cells(*KINDS[name], [], n_grid)
        assert (m, len(x)) == (merge, cells), (name, n_grid)
    x, _, _ = P.importance_cells(*KINDS['qu'], [], 16)
    assert x[:2].tolist() == [0.5, 2.5] and x[-1] == 20.5
    x, _, _ = P.importance_cells(*KINDS['qlu'], [], 64)
    assert x[0] == 1.0 and x[-1] == 55.0
    # qlognormal with an observed 0: the floor's log puts the support's start at 0
    x, _, m = P.importance_cells(*KINDS['qln'], [0.0, 2.0], 4096)
    assert x[0] == 0.0 and m == 1 and x[-1] == np.round(math.exp(1.0 + 4.0))


@pytest.mark.parametrize('n_grid', (1, 16, 4096))
def test_categorical_cells(n_grid):
    for name in ('ri', 'pc'):
        kind, args = KINDS[name]
        x, w, merge = P.importance_cells(kind, args, [], n_grid)
        assert x.tolist() == list(range(args['upper'])) and np.all(w == 1.0) and merge == 1


def test_cells_refuse_bad_arguments():
    with pytest.raises(ValueError):
        P.importance_cells('uniform', KINDS['u'][1], [], 0)
    with pytest.raises(ValueError):
        P.importance_cells('beta', {}, [], 4)


# -- the split ---------------------------------------------------------------
@pytest.mark.parametrize('fixture', ['labels_small.npz', 'labels_medium.npz'])
def test_split_default_is_unchanged(fixture):
    """n_below=None: the reference's size and np.argsort, as before."""
    for meta, rec in golden_io.cases(fixture):
        idxs, vals, gamma = np.asarray(rec['l_idxs']), np.asarray(rec['l_vals']), meta['gamma']
        nb = min(int(np.ceil(gamma * np.sqrt(len(vals)))), 25)
        order = np.argsort(vals)
        for got in (P.split_history(idxs, vals, gamma), P.split_history(idxs, vals, gamma, n_below=None)):
            assert np.array_equal(got[0], idxs[order[:nb]]) and np.array_equal(got[1], idxs[order[nb:]])
        sp, sp0 = P.Splitter(idxs, vals, gamma), P.Splitter(idxs, vals, gamma, n_below=None)
        assert np.array_equal(sp.tids, sp0.tids) and np.array_equal(sp.side, sp0.side)


def test_split_n_below_is_stable():
    tids = np.arange(10) * 2 + 1
    losses = np.array([3., 1., 2., 1., 1., 0., 2., 5., 1., 4.])
    for nb in range(0, 11):
        b, a = P.split_history(tids, losses, 0.25, n_below=nb)
        order = sorted(range(10), key=lambda i: (losses[i], i))
        assert b.tolist() == tids[order[:nb]].tolist() and a.tolist() == tids[order[nb:]].tolist()
    sp = P.Splitter(tids, losses, 0.25, n_below=4)   # the four best: tids 11, 3, 7, 9
    b, a = sp.split(tids, np.arange(10.0))
    assert b.tolist() == [1.0, 3.0, 4.0, 5.0] and len(a) == 6


# -- the reference itself ----------------------------------------------------
def test_identical_mixtures_give_zero():
    mix = ([0.25, 0.75], [0.0, 1.5], [1.0, 0.5])
    for post, kind in ((P.LabelPosterior('a', 'GMM1', mix, mix, low=-5.0, high=5.0), 'uniform'),
                       (P.LabelPosterior('a', 'GMM1', mix, mix, low=0.0, high=20.0, q=1.0), 'quniform'),
                       (P.LabelPosterior('a', 'categorical', np.array([.2, .8]), np.array([.2, .8]), upper=2),
                        'randint')):
        args = dict(low=post.low, high=post.high, q=post.q, upper=2)
        x, w, merge = P.importance_cells(kind, args, [], 64)
        lb, la = R.planes(post, x, merge)
        assert R.v_of(lb, la, w, 0.3) == 0.0


def test_two_categories_closed_form():
    l, g, alpha = np.array([0.7, 0.3]), np.array([0.2, 0.8]), 0.25
    post = P.LabelPosterior('c', 'categorical', l, g, upper=2)
    x, w, merge = P.importance_cells('randint', dict(upper=2), [], 4096)
    got = R.v_of(*R.planes(post, x, merge), w, alpha)
    p = alpha * l + (1 - alpha) * g
    want = float(np.sum(p * (alpha * l / p - alpha) ** 2))
    assert abs(got - want) <= 8 * np.spacing(want)
    # alpha^2 times the Pearson divergence of l from p
    assert abs(got - alpha ** 2 * float(np.sum((l - p) ** 2 / p))) <= 8 * np.spacing(want)


def test_term_edges():
    assert R.term(-np.inf, -np.inf, 1.0, 0.3) == 0.0
    assert math.isnan(R.term(float('nan'), 0.0, 1.0, 0.3))
    # only g reaches the cell: m = 0, the term (1 - alpha) g alpha^2; only l: m = 1
    assert R.term(-np.inf, 0.0, 2.0, 0.25) == 2.0 * 0.75 * 0.25 ** 2
    assert abs(R.term(0.0, -np.inf, 2.0, 0.25) - 2.0 * 0.25 * 0.75 ** 2) <= 1e-16
    # both branches of d agree with the direct form
    for lb, la in ((-1.0, -3.0), (-3.0, -1.0), (-2.0, -2.0)):
        a = 0.4
        p = a * math.exp(lb) + (1 - a) * math.exp(la)
        direct = p * (a * math.exp(lb) / p - a) ** 2
        assert abs(R.term(lb, la, 1.0, a) - direct) <= 1e-15


@pytest.mark.parametrize('name', QUANT)
def test_merged_cells_conserve_mass_and_never_raise_v(hist, name):
    kind, args = KINDS[name]
    (post, nb, na, ov), = [r for (n_, _, _), r in zip(hist.labels, R.label_inputs(hist, 0.1)) if n_ == name]
    alpha = nb / (nb + na)
    k0, k1 = support(name, ov)
    for n_grid in (1, 5, 16, 1 << 20):
        x, w, merge = P.importance_cells(kind, args, ov, n_grid)
        assert (merge > 1) == (n_grid < 1 << 20)
        mb, ma = R.planes(post, x, merge)
        # the support values the cells cover, one by one (the last cell may reach past the support's end)
        ks = k0 + np.arange(len(x) * merge)
        if 'low' in args:   # (a bounded label's intervals are clipped at the bound: nothing lies past it)
            ks = ks[ks <= k1]
        xs = ks * args['q']
        lb, la = R.planes(post, xs, 1)
        mass, v = R.density(lb, la, alpha).sum(), R.v_of(lb, la, np.ones(len(xs)), alpha)
        assert v > 0
        assert abs(R.density(mb, ma, alpha).sum() - mass) <= 1e-12
        assert R.v_of(mb, ma, w, alpha) <= v * (1 + 1e-12)


def test_planted_history_ranks_u_first(hist):
    imp, vs = R.importance(hist, quantile=0.1, n_grid=1024)
    names = sorted(imp, key=lambda k: -imp[k])
    assert names[0] == 'u' and imp['u'] >= 0.5
    assert abs(sum(imp.values()) - 1.0) <= 1e-12 and min(imp.values()) >= 0.0
    # the sum is converged at this grid: 4096 cells move V_u in the sixth digit at most
    fine = R.importance(hist, quantile=0.1, n_grid=4096)[1]['u']
    assert abs(fine - vs['u']) <= 1e-5 * fine


# -- tpe.importance's checks --------------------------------------------------
def _space():
    from hyperopt_amd import hp
    return {'u': hp.uniform('u', -5, 5), 'c': hp.choice('c', [0, 1, 2])}


def _trials(losses):
    from hyperopt_amd.workloads import History, history_trials
    n = len(losses)
    tids = np.arange(n, dtype=np.int64)
    rng = np.random.RandomState(3)
    labels = [('u', 'uniform', dict(low=-5.0, high=5.0)), ('c', 'randint', dict(upper=3))]
    obs = {'u': (tids, rng.uniform(-5, 5, n)), 'c': (tids, rng.randint(3, size=n).astype(float))}
    return history_trials(History(labels, tids, np.asarray(losses, dtype=float), obs))


def test_importance_refuses_before_any_engine(monkeypatch):
    from hyperopt_amd import engine, tpe

    def no_engine(*a, **k):
        raise AssertionError('an engine was asked for')
    monkeypatch.setattr(engine, 'get_engine', no_engine)
    monkeypatch.setattr(engine, 'Engine', no_engine)
    trials = _trials(np.linspace(0, 1, 30))
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, float('nan'), '0.1', None, True):
        with pytest.raises(ValueError, match='quantile'):
            tpe.importance(_space(), trials, quantile=bad)
    for bad in (0, -4, 1.5, 64.0, '64', None, True):
        with pytest.raises(ValueError, match='n_grid'):
            tpe.importance(_space(), trials, n_grid=bad)
    for few in (_trials([]), _trials([1.0])):
        with pytest.raises(ValueError, match='at least 2 complete trials'):
            tpe.importance(_space(), few)
        with pytest.raises(ValueError, match='at least 2 complete trials'):
            tpe.importance(_space(), few, objectives=('loss',))
    # a pending trial is not complete
    two = _trials([1.0, 2.0])
    two.trials[1]['result'] = {'status': 'new'}
    with pytest.raises(ValueError, match='at least 2 complete trials'):
        tpe.importance(_space(), two)
    for kw in (dict(objectives='loss'), dict(objectives=()), dict(objectives=('loss', 'loss')),
               dict(constraints=('loss',)), dict(objectives=('loss', 'cost')),
               dict(constraints=('c',))):
        with pytest.raises(ValueError):
            tpe.importance(_space(), trials, **kw)
    # a Domain is taken as it is
    from hyperopt_amd import Domain
    with pytest.raises(ValueError, match='quantile'):
        tpe.importance(Domain(None, _space()), trials, quantile=2)


def test_a_nan_label_comes_last_and_leaves_the_shares_alone(monkeypatch):
    """The device sums replaced by given numbers: the label with a NaN sum
    keeps NaN, is listed last and takes no part in the normalising sum."""
    from hyperopt_amd import Domain, engine, tpe

    class Sums(object):
        def __init__(self, v):
            self.v = v

        def set_posterior(self, *a):
            pass

        def importance(self, labels, cells, alpha, want_planes=False):
            return np.asarray([self.v[int(l)] for l in labels])
    trials = _trials(np.linspace(0, 1, 30))
    names = list(tpe.specs_of(Domain(None, _space())))
    for nan_at in (0, 1):
        v = [0.25, 0.25]
        v[nan_at] = float('nan')
        monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: Sums(v))
        got = tpe.importance(_space(), trials)
        assert list(got) == [names[1 - nan_at], names[nan_at]]
        assert got[names[1 - nan_at]] == 1.0 and math.isnan(got[names[nan_at]])
        raw = tpe.importance(_space(), trials, normalize=False)
        assert raw[names[1 - nan_at]] == 0.25 and math.isnan(raw[names[nan_at]]) and list(raw) == list(got)
