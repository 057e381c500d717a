"""Hyperparameter importance on the device (tpe_importance, Engine.importance,
tpe.importance) against the plain restatement in tests/importance_reference.py
and against Engine.score: the planes at the project's lpdf bar and bit for bit,
the sums within the bound derived below, determinism, the edges and errors,
and the public function."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import posterior as P
from tests import importance_reference as R
from tests.helpers import ALL_KINDS, assert_lpdf_close, make_history

pytestmark = pytest.mark.gpu

NS = (2, 40, 700)
GRIDS = (1, 63, 64, 65, 255, 256, 257, 1025)   # around the wave (64), the granule (256) and the dense tile (512)
QUANTILE = 0.1
QUANTIZED = ('quniform', 'qloguniform', 'qnormal', 'qlognormal')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


class Case(object):
    """A history's posteriors resident on an engine, and the inputs of its
    importance calls per n_grid."""

    def __init__(self, n):
        from hyperopt_amd.engine import Engine
        self.hist = make_history(ALL_KINDS, n, seed=100 + n, active_frac=0.7)
        self.inputs = R.label_inputs(self.hist, QUANTILE)
        self.posts = [r[0] for r in self.inputs]
        # (a label seen on one side only is never sent by tpe.importance: any alpha serves its planes)
        self.alpha = [nb / (nb + na) if nb and na else 0.5 for _, nb, na, _ in self.inputs]
        self.eng = Engine(0, 'f64')
        self.eng.set_posterior(*P.pack(self.posts))
        self.calls = {}

    def cells(self, n_grid):
        return [P.importance_cells(kind, args, r[3], n_grid)
                for (_, kind, args), r in zip(self.hist.labels, self.inputs)]

    def call(self, n_grid):
        if n_grid not in self.calls:
            cells = self.cells(n_grid)
            self.calls[n_grid] = (cells,) + self.eng.importance(range(len(cells)), cells, self.alpha,
                                                                 want_planes=True)
        return self.calls[n_grid]


@pytest.fixture(scope='module')
def cases():
    made = {}

    def get(n):
        if n not in made:
            made[n] = Case(n)
        return made[n]
    yield get
    for c in made.values():
        c.eng.close()


@pytest.mark.parametrize('n_grid', GRIDS)
@pytest.mark.parametrize('n', NS)
def test_planes_against_the_oracle(cases, n, n_grid):
    c = cases(n)
    cells, v, lb, la = c.call(n_grid)
    for li, (name, kind, _) in enumerate(c.hist.labels):
        x, w, merge = cells[li]
        rb, ra = R.planes(c.posts[li], x, merge)
        assert len(lb[li]) == len(x)
        assert_lpdf_close(lb[li], rb, quantized=kind in QUANTIZED)
        assert_lpdf_close(la[li], ra, quantized=kind in QUANTIZED)


@pytest.mark.parametrize('n_grid', GRIDS)
@pytest.mark.parametrize('n', NS)
def test_planes_are_engine_score_bit_for_bit(cases, n, n_grid):
    c = cases(n)
    cells, v, lb, la = c.call(n_grid)
    seen = 0
    for li in range(len(c.hist.labels)):
        x, w, merge = cells[li]
        if merge != 1:
            continue
        sb, sa, _ = c.eng.score(li, x)
        assert bits(lb[li]) == bits(sb) and bits(la[li]) == bits(sa), c.hist.labels[li][0]
        seen += 1
    assert seen >= 6   # every dense and categorical label, and the quantized ones the grid does not merge


@pytest.mark.parametrize('n_grid', GRIDS)
@pytest.mark.parametrize('n', NS)
def test_sum_is_the_reference_epilogue_of_the_planes(cases, n, n_grid):
    """rtol = (C + 32) 2^-52 for a label of C cells: the terms are
    non-negative, so each side's summation error is at most (C - 1) 2^-53
    relative, and a term is at most 16 roundings of <= 1 ulp away from the
    exact one on each side."""
    c = cases(n)
    cells, v, lb, la = c.call(n_grid)
    for li, (name, _, _) in enumerate(c.hist.labels):
        x, w, merge = cells[li]
        want = R.v_of(lb[li], la[li], w, c.alpha[li])
        assert want == want and want >= 0.0
        print('%s n=%d n_grid=%d: v %.17g reference %.17g' % (name, n, n_grid, v[li], want))
        assert abs(v[li] - want) <= (len(x) + 32) * 2.0 ** -52 * want, (name, v[li], want)


@pytest.mark.parametrize('n', (40, 700))
def test_importance_against_the_whole_reference(cases, n):
    """End to end against the oracle's lpdfs: the engine's lpdfs are within
    1e-9 of the oracle's, a term's relative derivative in them is at most 3
    (p, and twice m - alpha), so the sums agree to a few 1e-9; 1e-7 here."""
    c = cases(n)
    cells, v, lb, la = c.call(257)
    _, vs = R.importance(c.hist, QUANTILE, 257, normalize=False)
    for li, (name, _, _) in enumerate(c.hist.labels):
        nb, na = c.inputs[li][1:3]
        if nb and na:
            assert abs(v[li] - vs[name]) <= 1e-7 * vs[name] + 1e-13, name


def test_the_same_bits_every_time_alone_and_reversed(cases):
    c = cases(700)
    for n_grid in (65, 1025):
        cells, v, lb, la = c.call(n_grid)
        L = len(cells)
        again = c.eng.importance(range(L), cells, c.alpha)
        assert bits(again) == bits(v)
        rev = list(range(L))[::-1]
        back = c.eng.importance(rev, [cells[i] for i in rev], [c.alpha[i] for i in rev])
        assert bits(back[::-1]) == bits(v)
        for li in range(L):
            alone = c.eng.importance([li], [cells[li]], [c.alpha[li]])
            assert bits(alone) == bits(v[li:li + 1]), c.hist.labels[li][0]
        # the planes do not depend on the company either
        _, lb1, la1 = c.eng.importance([3, 0], [cells[3], cells[0]], [c.alpha[3], c.alpha[0]], want_planes=True)
        assert bits(lb1[1]) == bits(lb[0]) and bits(la1[0]) == bits(la[3])


def test_empty_selection_and_a_label_without_cells(cases):
    c = cases(40)
    assert len(c.eng.importance([], [], [])) == 0
    v, lb, la = c.eng.importance([], [], [], want_planes=True)
    assert len(v) == 0 and lb == [] and la == []
    cells = c.cells(64)
    none = (np.zeros(0), np.zeros(0), 1)
    ref = c.eng.importance([0, 4], [cells[0], cells[4]], [c.alpha[0], c.alpha[4]])
    v, lb, la = c.eng.importance([0, 1, 4, 8], [cells[0], none, cells[4], none],
                                 [c.alpha[0], 0.5, c.alpha[4], 0.5], want_planes=True)
    assert v[1] == 0.0 and v[3] == 0.0 and len(lb[1]) == 0 and len(la[3]) == 0
    assert bits(v[[0, 2]]) == bits(ref)
    assert bits(c.eng.importance([1], [none], [0.5])) == bits([0.0])


def test_one_trial_on_each_side(cases):
    """N = 2: one good trial, one other; most labels are seen on one side at
    most, and the mixtures are the prior and at most one observation."""
    c = cases(2)
    counts = [(nb, na) for _, nb, na, _ in c.inputs]
    assert any(na == 0 for nb, na in counts) and any(nb == 0 for nb, na in counts)
    cells, v, lb, la = c.call(64)
    assert np.all(np.isfinite(v)) and np.all(v >= 0.0)
    for li, (nb, na) in enumerate(counts):
        if nb == 0 and na == 0:   # the prior on both sides: m = alpha everywhere
            assert bits(lb[li]) == bits(la[li]) and v[li] == 0.0


def edge_engine():
    from hyperopt_amd.engine import Engine
    narrow = ([1.0], [0.0], [0.01])
    posts = [P.LabelPosterior('q', 'GMM1', narrow, ([1.0], [1.0], [0.01]), low=0.0, high=1000.0, q=1.0),
             P.LabelPosterior('c', 'categorical', np.array([0.75, 0.0, 0.25]), np.array([0.5, 0.0, 0.5]), upper=3),
             P.LabelPosterior('d', 'GMM1', ([1.0], [0.0], [1.0]), ([1.0], [1.0], [2.0]))]
    eng = Engine(0, 'f64')
    eng.set_posterior(*P.pack(posts))
    return eng


def test_cells_no_mixture_reaches_and_nan():
    eng = edge_engine()
    try:
        xq = np.array([0.0, 1.0, 500.0, 2.0])
        cells = [(xq, np.ones(4), 1), (np.arange(3.0), np.ones(3), 1)]
        v, lb, la = eng.importance([0, 1], cells, [0.3, 0.6], want_planes=True)
        assert lb[0][2] == -np.inf and la[0][2] == -np.inf       # no mass 500 sigma away
        assert lb[1][1] == -np.inf and la[1][1] == -np.inf       # a category neither side ever saw
        for s in range(2):
            want = R.v_of(lb[s], la[s], cells[s][1], [0.3, 0.6][s])
            assert want > 0 and abs(v[s] - want) <= (len(cells[s][0]) + 32) * 2.0 ** -52 * want
        # only one side reaches a cell: still a number
        assert la[0][0] == -np.inf and np.isfinite(lb[0][0])
        # a NaN lpdf makes the label's sum NaN, and only that label's
        v, lb, la = eng.importance([2, 1], [(np.array([0.5, 1e200]), np.ones(2), 1), cells[1]], [0.5, 0.6],
                                   want_planes=True)
        assert np.isnan(lb[0][1]) and np.isnan(v[0]) and np.isfinite(v[1])
    finally:
        eng.close()


def test_argument_errors_name_the_function(cases):
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import Engine, EngineError
    c = cases(40)
    eng = c.eng
    cells = c.cells(16)
    ok = eng.importance([0, 1], cells[:2], [0.4, 0.4])

    def refused(*a):
        with pytest.raises(EngineError, match='tpe_importance'):
            eng.importance(*a)
    refused([len(cells)], [cells[0]], [0.4])                      # out of range
    refused([-1], [cells[0]], [0.4])
    refused([0, 1, 0], [cells[0], cells[1], cells[0]], [0.4] * 3)  # listed twice
    for alpha in (0.0, 1.0, -0.1, 1.5, float('nan')):
        refused([0], [cells[0]], [alpha])
    refused([1], [(cells[1][0], cells[1][1], 0)], [0.4])           # merge < 1
    refused([0], [(cells[0][0], cells[0][1], 2)], [0.4])           # merge on a dense label
    refused([8], [(cells[8][0], cells[8][1], 2)], [0.4])           # and on a categorical one
    # decreasing offsets and a first offset that is not 0: the raw entry point
    lab = np.array([0, 1], dtype=np.int32)
    x, w = np.zeros(8), np.ones(8)
    merge, alpha, v = np.ones(2, dtype=np.int32), np.full(2, 0.4), np.full(2, -7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for off in ([0, 5, 3], [1, 3, 8]):
        off = np.array(off, dtype=np.int64)
        rc = eng.lib.tpe_importance(eng.h, 2, p(lab), p(off), p(x), p(w), p(merge), p(alpha), p(v), None, None)
        assert rc == L.TPE_ERR_ARG and b'tpe_importance' in eng.lib.tpe_last_error(eng.h)
    off = np.array([0, 4, 8], dtype=np.int64)
    plane = np.zeros(8)
    rc = eng.lib.tpe_importance(eng.h, 2, p(lab), p(off), p(x), p(w), p(merge), p(alpha), p(v), p(plane), None)
    assert rc == L.TPE_ERR_ARG and b'tpe_importance' in eng.lib.tpe_last_error(eng.h)
    assert np.all(v == -7.0)                                       # untouched
    # a categorical point that is no category
    for bad in (7.0, -1.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match='tpe_importance'):
            eng.importance([8], [(np.array([0.0, bad]), np.ones(2), 1)], [0.4])
    # no posterior
    fresh = Engine(0, 'f64')
    try:
        with pytest.raises(EngineError, match='tpe_importance'):
            fresh.importance([0], [cells[0]], [0.4])
        with pytest.raises(EngineError, match='tpe_importance'):
            fresh.importance([], [], [])
    finally:
        fresh.close()
    # none of it changed what the next call returns
    assert bits(eng.importance([0, 1], cells[:2], [0.4, 0.4])) == bits(ok)


def test_a_built_posterior_and_the_pool_are_left_alone(cases):
    """On a posterior the device built from its resident history: the planes
    are Engine.score's there too, and the mixtures, the pool and its ranking
    are what they were before the call."""
    from hyperopt_amd.engine import Engine
    c = cases(40)
    hist = c.hist
    eng = Engine(0, 'f64')
    try:
        eng.build_posterior(*hist.device_inputs(), 0.25, 1.0)
        L = len(hist.labels)
        rng = np.random.RandomState(5)
        pool = np.stack([np.stack([o[1][rng.randint(len(o[1]))] for o in (hist.obs[n] for n, _, _ in hist.labels)])
                         for _ in range(50)])
        eng.pool_set(pool)
        before = [eng.get_mixture(li, side) for li in range(L) for side in (0, 1)]
        rank = eng.pool_rank(50, want_scores=True)
        cells = [P.importance_cells(kind, args, hist.obs[name][1], 65) for name, kind, args in hist.labels]
        v, lb, la = eng.importance(range(L), cells, [0.25] * L, want_planes=True)
        assert np.all(np.isfinite(v)) and np.all(v >= 0)
        for li in range(L):
            if cells[li][2] == 1:
                sb, sa, _ = eng.score(li, cells[li][0])
                assert bits(lb[li]) == bits(sb) and bits(la[li]) == bits(sa)
        after = [eng.get_mixture(li, side) for li in range(L) for side in (0, 1)]
        for m0, m1 in zip(before, after):
            assert all(bits(a) == bits(b) for a, b in zip(m0, m1))
        assert eng.pool_size() == (50, L)
        again = eng.pool_rank(50, want_scores=True)
        assert np.array_equal(rank[0], again[0]) and bits(rank[2]) == bits(again[2])
    finally:
        eng.close()


# -- the public function ------------------------------------------------------
def space_of(labels):
    from hyperopt_amd import hp
    from hyperopt_amd.workloads import hp_space
    space = hp_space([l for l in labels if l[1] != 'categorical'])
    for name, kind, args in labels:
        if kind == 'categorical':
            space[name] = hp.pchoice(name, [(p, i) for i, p in enumerate(args['p'])])
    return space


@pytest.fixture(scope='module')
def study():
    from hyperopt_amd import Domain, tpe
    from hyperopt_amd.workloads import history_trials
    hist = R.planted()
    domain = Domain(None, space_of(hist.labels))
    return hist, domain, history_trials(hist), list(tpe.specs_of(domain))


def test_public_function_is_the_engines_sums_normalised(study):
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import get_engine
    hist, domain, trials, names = study
    got, curves = tpe.importance(domain, trials, n_grid=257, curves=True)
    assert list(got)[0] == 'u' and got['u'] >= 0.5
    assert list(got) == sorted(names, key=lambda k: (-got[k], names.index(k)))
    # the same from the pieces: the counts by the reference's loops, the cells,
    # one Engine.importance call on the context the function left its posterior on
    by_name = {l[0]: (l, r) for l, r in zip(hist.labels, R.label_inputs(hist, 0.1))}
    n = len(hist.tids)
    cells = [P.importance_cells(by_name[k][0][1], by_name[k][0][2], by_name[k][1][3], 257) for k in names]
    alpha = [by_name[k][1][1] / (by_name[k][1][1] + by_name[k][1][2]) for k in names]
    active = np.array([(by_name[k][1][1] + by_name[k][1][2]) / n for k in names])
    eng = get_engine(0, 'f64', 'importance')
    v, lb, la = eng.importance(range(len(names)), cells, alpha, want_planes=True)
    raw = active * v
    want = raw / np.sum(raw)
    assert [got[k] for k in names] == want.tolist()
    plain = tpe.importance(domain, trials, n_grid=257, normalize=False)
    assert [plain[k] for k in names] == raw.tolist()
    # a space in place of the domain; the keys of distinct losses are their ranks: the same split
    assert tpe.importance(space_of(hist.labels), trials, n_grid=257) == got
    assert tpe.importance(domain, trials, n_grid=257, objectives=('loss',)) == got
    # the partial-dependence view
    assert sorted(curves) == sorted(names)
    for k, name in enumerate(names):
        x, w, p, m = curves[name]
        assert bits(x) == bits(cells[k][0]) and bits(w) == bits(cells[k][1])
        lik = alpha[k] * np.exp(lb[k])
        assert np.all(np.abs(p - (lik + (1 - alpha[k]) * np.exp(la[k]))) <= 4 * np.spacing(p))
        assert np.all(np.abs(m - lik / p) <= 4 * np.spacing(m)) and np.all((m >= 0) & (m <= 1))


def test_public_function_with_two_trials():
    from hyperopt_amd import tpe
    from hyperopt_amd.workloads import history_trials
    hist = make_history(ALL_KINDS, 2, seed=102, active_frac=0.7)
    got = tpe.importance(space_of(hist.labels), history_trials(hist), n_grid=64)
    counts = {l[0]: r[1:3] for l, r in zip(hist.labels, R.label_inputs(hist, 0.1))}
    assert set(got) == set(counts)
    for name, (nb, na) in counts.items():
        assert got[name] >= 0.0 and (got[name] == 0.0 or (nb and na))


def test_main_context_is_untouched(study):
    from hyperopt_amd import tpe
    hist, domain, trials, names = study
    kw = dict(posterior_builder='device', n_EI_candidates=64)
    before = tpe.suggest([5000], domain, trials, 3, **kw)
    tpe.importance(domain, trials, n_grid=64)
    after = tpe.suggest([5000], domain, trials, 3, **kw)
    assert before[0]['misc']['vals'] == after[0]['misc']['vals']
    assert before[0]['misc']['idxs'] == after[0]['misc']['idxs']


def test_abi_version_is_unchanged():
    from hyperopt_amd import _lib as L
    assert L.load().tpe_abi_version() == 5
