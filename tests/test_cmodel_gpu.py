"""The constraint-density round on the device (tpe_cmodel_*, Engine.cmodel_*,
tpe.suggest(constraint_model='density')) against the oracle's lpdfs fed to
posterior.cmodel_acquisition, and against the existing samplers for the draws."""
import numpy as np
import pytest

from hyperopt_amd import _lib as L
from hyperopt_amd import posterior as P
from tests import importance_reference as R
from tests.helpers import assert_lpdf_close

pytestmark = pytest.mark.gpu

LABELS = [('u', 'uniform', dict(low=-5.0, high=5.0)),
          ('n', 'normal', dict(mu=0.0, sigma=3.0)),
          ('lu', 'loguniform', dict(low=-5.0, high=2.0)),
          ('qu', 'quniform', dict(low=0.0, high=20.0, q=1.0)),
          ('qln', 'qlognormal', dict(mu=1.0, sigma=1.0, q=1.0)),
          ('c', 'randint', dict(upper=5))]
QUANTIZED = ('quniform', 'qlognormal')
SKIP = (1, 0)   # model 1 has no mixture for label 0
# (above components, candidates, constraints): the chunk of 1024 components from
# both sides and two chunks plus one; one lane, a wave less and plus one, 216
SHAPES = [(1023, 1, 1), (1024, 63, 1), (1025, 65, 8), (2049, 216, 8)]


class Case(object):
    """Models 0 .. K of the six labels on one engine: model k's above side has
    `na` components (the prior and na - 1 observations), its below side 9."""

    def __init__(self, na, K):
        from hyperopt_amd.engine import Engine
        from hyperopt_amd.workloads import prior_draw
        rng = np.random.RandomState(1000 + na + K)
        self.K = K
        self.posts = [[P.label_posterior(name, kind, args, prior_draw(kind, args, rng, 8),
                                         prior_draw(kind, args, rng, na - 1), 1.0)
                       for name, kind, args in LABELS] for _ in range(K + 1)]
        self.gammas = np.concatenate([[0.25], rng.uniform(0.05, 0.95, size=K)])
        self.eng = Engine(0, 'f64')
        self.eng.set_posterior(*P.pack(self.posts[0]))
        for k in range(1, K + 1):
            self.eng.cmodel_set(k, *P.pack(self.posts[k]), skip=[SKIP[1]] if k == SKIP[0] else [])

    def models(self, label):
        return [k for k in range(self.K + 1) if (k, label) != SKIP]

    def reference(self, label, x):
        ms = self.models(label)
        planes = [R.planes(self.posts[k][label], x) for k in ms]
        ll, lg = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
        return ms, ll, lg, P.cmodel_acquisition(ll, lg, self.gammas[ms])

    def draws(self, label, seed, rnd, n):
        return sampler_draws(self.eng, [(k, self.posts[k][label]) for k in self.models(label)], label, seed, rnd, n)


def sampler_draws(eng, models, label, seed, rnd, n):
    """The round's candidates of one cell from the existing samplers: n draws
    of each (k, posterior)'s below mixture with model k's stream."""
    out = []
    for k, p in models:
        stream = label if k == 0 else L.TPE_CMODEL_STREAM + (k - 1) * L.TPE_CMODEL_STREAM_SPAN + label
        if p.family == 'categorical':
            out.append(eng.categorical(p.below, seed=seed, size=(n,), stream=stream, round=rnd).astype(np.float64))
        else:
            fn = eng.GMM1 if p.family == 'GMM1' else eng.LGMM1
            out.append(fn(*p.below, low=p.low, high=p.high, q=p.q, seed=seed, size=(n,), stream=stream, round=rnd))
    return np.concatenate(out)


@pytest.fixture(scope='module')
def cases():
    made = {}

    def get(na, K):
        if (na, K) not in made:
            made[na, K] = Case(na, K)
        return made[na, K]
    yield get
    for c in made.values():
        c.eng.close()


def best_of(a):
    """broadcast_best's order on a: the first NaN, else the first maximum."""
    nan = np.flatnonzero(np.isnan(a))
    return int(nan[0]) if len(nan) else int(np.argmax(a))


@pytest.mark.parametrize('na,n,K', SHAPES)
def test_score_against_the_oracle(cases, na, n, K):
    """ll, lg at the project's lpdf bar (1e-9 relative; a quantized label's
    probability to the reference's own accuracy, tests.helpers); a within 1e-9
    relative with an absolute floor of 1e-12."""
    from hyperopt_amd.workloads import prior_draw
    c = cases(na, K)
    rng = np.random.RandomState(na + n)
    for li, (name, kind, args) in enumerate(LABELS):
        x = prior_draw(kind, args, rng, n).astype(np.float64)
        a, ll, lg = c.eng.cmodel_score(li, x, c.gammas)
        ms, rl, rg, ra = c.reference(li, x)
        off = [k for k in range(9) if k not in ms]
        assert np.all(np.isnan(ll[off])) and np.all(np.isnan(lg[off]))
        assert_lpdf_close(ll[ms], rl, quantized=kind in QUANTIZED, atol=0.0)
        assert_lpdf_close(lg[ms], rg, quantized=kind in QUANTIZED, atol=0.0)
        err = np.abs(a - ra)
        print('%s na=%d n=%d K=%d: max |a - ref| %.3g, max |a| %.3g' % (name, na, n, K, err.max(), np.abs(ra).max()))
        assert np.all(err <= 1e-9 * np.abs(ra) + 1e-12), (name, a, ra)


def test_score_where_one_side_has_no_mass():
    """A quantized label 500 sigma from the below mixture: ll = -inf, so
    t = +inf and a = -inf; the reverse under the constraint model: f = -log gamma."""
    from hyperopt_amd.engine import Engine
    narrow, wide = ([1.0], [0.0], [0.01]), ([1.0], [250.0], [400.0])
    post = lambda b, a: [P.LabelPosterior('q', 'GMM1', b, a, low=0.0, high=1000.0, q=1.0)]
    eng = Engine(0, 'f64')
    try:
        eng.set_posterior(*P.pack(post(narrow, wide)))
        x = np.array([0.0, 500.0])
        a, ll, lg = eng.cmodel_score(0, x, [0.3])
        assert ll[0, 1] == -np.inf and np.isfinite(lg[0, 1]) and a[1] == -np.inf and np.isfinite(a[0])
        eng.cmodel_set(1, *P.pack(post(wide, narrow)))
        a1, ll, lg = eng.cmodel_score(0, x, [0.3, 0.6])
        assert lg[1, 1] == -np.inf and a1[1] == -np.inf          # (-inf from model 0 stays)
        eng.set_posterior(*P.pack(post(wide, wide)))
        a2, ll, lg = eng.cmodel_score(0, x, [0.3, 0.6])
        assert ll[0, 1] == lg[0, 1] and abs(a2[1] - -np.log(0.6)) <= 1e-12
    finally:
        eng.close()


SEED, ROUNDS, N = 7, [3, 4, 11, 12], 24


@pytest.mark.parametrize('na,K', [(65, 2), (1025, 2)])
def test_round_draws_and_winner(cases, na, K):
    """Every (round, label) cell: the candidates rebuilt from the existing
    samplers (model M'[j // n]'s below mixture, its stream, draw j % n), the
    reference a over them, broadcast_best's winner -- index, and the value bit
    for bit.  Equal candidates (the categorical label, a quantized grid value
    drawn twice) have equal a: the lower index wins."""
    c = cases(na, K)
    g = np.tile(np.concatenate([c.gammas, np.ones(8 - K)]), (len(LABELS), 1))
    res = c.eng.cmodel_suggest(SEED, ROUNDS, N, g)
    assert res.shape == (len(ROUNDS), len(LABELS))
    # a model's wrong stream or round would show only where its candidates win: every model wins somewhere
    assert set((res['index'] // N).ravel().tolist()) == {0, 1, 2}
    for r, rnd in enumerate(ROUNDS):
        for li, (name, kind, _) in enumerate(LABELS):
            x = c.draws(li, SEED, rnd, N)
            assert len(x) == N * len(c.models(li))
            _, rl, rg, ra = c.reference(li, x)
            j = best_of(ra)
            top = np.unique(ra)[::-1]
            print('%s round %d: winner %d, gap %.3g' % (name, rnd, j, top[0] - top[1]))
            assert top[0] - top[1] > 1e-6, 'the seeds must leave a clear winner'
            if kind == 'randint':
                assert np.count_nonzero(ra == ra[j]) > 1     # the tie the lower index must win
            got = res[r][li]
            assert got['index'] == j and got['label'] == li, (name, rnd, got, j)
            assert got['value'].tobytes() == x[j].tobytes()
            assert abs(got['lpdf_below'] - rl[0, j]) <= 1e-9 * abs(rl[0, j])


def conditional_study(satisfied):
    from hyperopt_amd import Domain, hp
    from hyperopt_amd.base import JOB_STATE_DONE, STATUS_OK, Trials
    from hyperopt_amd import rand
    space = {'x': hp.uniform('x', -5, 5), 'b': hp.quniform('b', 1, 32, 1),
             'opt': hp.choice('opt', [{'kind': 'sgd', 'lr': hp.loguniform('lr', -7, 0)}, {'kind': 'adam'}])}
    domain = Domain(None, space)
    trials = Trials()
    docs = rand.suggest(list(range(60)), domain, trials, 5)
    rng = np.random.RandomState(9)
    for d in docs:
        x = d['misc']['vals']['x'][0]
        d['state'] = JOB_STATE_DONE
        d['result'] = {'status': STATUS_OK, 'loss': float(x * x + rng.normal()),
                       'c1': -1.0 if satisfied else float(x - 1.0),
                       'c2': -0.5 if satisfied else float(d['misc']['vals']['b'][0] - 20.0)}
    trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def vals(docs):
    return [(d['tid'], d['misc']['vals']) for d in docs]


@pytest.mark.parametrize('batch', [False, True])
def test_equivalence_when_every_trial_satisfies(batch):
    from hyperopt_amd import tpe
    domain, trials = conditional_study(True)
    ids = [100, 101, 102] if batch else [100]
    plain = tpe.suggest(ids, domain, trials, 3, batch=batch)
    dens = tpe.suggest(ids, domain, trials, 3, batch=batch, constraints=('c1', 'c2'), constraint_model='density')
    assert vals(dens) == vals(plain) and len(dens) == len(ids)
    rank = tpe.suggest(ids, domain, trials, 3, batch=batch, constraints=('c1', 'c2'))
    assert vals(tpe.suggest(ids, domain, trials, 3, batch=batch, constraints=('c1', 'c2'),
                            constraint_model='rank')) == vals(rank)


def test_density_call_with_violations():
    """Violated constraints: both models are built and used; a batch's first
    document is the single call's (the round is a function of the id), a fixed
    value replaces its label's winner and leaves the others, and the call
    repeats bit for bit."""
    from hyperopt_amd import tpe
    domain, trials = conditional_study(False)
    kw = dict(constraints=('c1', 'c2'), constraint_model='density')
    one = tpe.suggest([100], domain, trials, 3, **kw)
    many = tpe.suggest([100, 101], domain, trials, 3, batch=True, **kw)
    assert vals(many[:1]) == vals(one) == vals(tpe.suggest([100], domain, trials, 3, **kw))
    assert vals(one) != vals(tpe.suggest([100], domain, trials, 3))
    fixed = tpe.suggest([100], domain, trials, 3, fixed={'x': 0.5}, **kw)[0]['misc']['vals']
    assert fixed['x'] == [0.5] and fixed['b'] == one[0]['misc']['vals']['b']
    pend = tpe.suggest([100, 101], domain, trials, 3, batch='pending', **kw)
    assert vals(pend[:1]) == vals(one) and len(pend) == 2


def test_end_to_end_against_the_host_rebuild():
    """60 trials, 2 constraints, a conditional space: every value of the
    document equals the one rebuilt here from the rule -- the splits written
    out, posterior.label_posterior, the existing samplers, the oracle's lpdfs
    and posterior.cmodel_acquisition."""
    from hyperopt_amd import history, tpe
    from hyperopt_amd import labels as _labels
    from hyperopt_amd.engine import get_engine
    domain, trials = conditional_study(False)
    names, gamma, n, seed, new_id = ('c1', 'c2'), 0.25, 24, 3, 100
    doc = tpe.suggest([new_id], domain, trials, seed, constraints=names, constraint_model='density',
                      posterior_builder='host')[0]
    specs = tpe.specs_of(domain)
    tids, losses, obs = history.gather(domain, trials, list(specs))
    assert tids.tolist() == [d['tid'] for d in trials.trials] and len(tids) == 60
    G = np.array([[d['result'][k] for k in names] for d in trials.trials])
    order = np.argsort(losses)
    n_below = int(min(np.ceil(gamma * np.sqrt(60)), 25))
    sides = [(tids[order[:n_below]], tids[order[n_below:]], n_below / 60)]
    for k in range(2):
        ok = G[:, k] <= 0.0
        assert 0 < ok.sum() < 60
        sides.append((tids[ok], tids[~ok], ok.sum() / 60))
    eng = get_engine(0, 'f64', 'importance')      # (any context: the samplers keep no state)
    want = {}
    for li, (name, sp) in enumerate(specs.items()):
        oi, ov = obs[name]
        models, gammas = [], []
        for k, (bt, at, g) in enumerate(sides):
            b, a = ov[np.isin(oi, bt)], ov[np.isin(oi, at)]
            if k == 0 or (len(b) and len(a)):
                models.append((k, P.label_posterior(name, sp.kind, sp.args, b, a, 1.0)))
                gammas.append(g)
        x = sampler_draws(eng, models, li, seed, new_id, n)
        planes = [R.planes(p, x) for _, p in models]
        a = P.cmodel_acquisition([p[0] for p in planes], [p[1] for p in planes], gammas)
        top = np.unique(a)[::-1]
        print('%s: models %s, winner %d, gap %.3g' % (name, [k for k, _ in models], best_of(a), top[0] - top[1]))
        assert top[0] - top[1] > 1e-6
        want[name] = _labels.coerce(sp.kind, x[best_of(a)])
    vals = doc['misc']['vals']
    assert set(vals) == set(want)
    active = {k for k in vals if len(vals[k])}
    assert {'x', 'b', 'opt'} <= active and ('lr' in active) == (want['opt'] == 0)
    for k in active:
        assert vals[k] == [want[k]], (k, vals[k], want[k])
