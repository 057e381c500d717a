"""Constraints on the device: Engine.mo_keys(F, G=G) (tpe_mo_keys_constrained,
hyperopt_amd/csrc/tpe_mo.hip) against the plain numpy statement of the rule
(tests/moc_reference.py), exactly -- keys and both counts are integers, the
violation is compared bit for bit -- and tpe.suggest(constraints=...) against
its definition: the plain call on a copy of the trials whose 'loss' is the
reference key."""
import ctypes
from functools import partial

import numpy as np
import pytest

from tests import mo_reference as R
from tests import moc_reference as C
from tests.test_mo_gpu import VARIANTS, points, space

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 1000, 4097)     # one row; the wave and block edges; several j-slices


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


def same(got, F, G):
    keys, by, do, v = got
    rby, rdo, rv = C.counts(F, G)
    assert keys.dtype == np.float64 and by.dtype == np.int32 and do.dtype == np.int32 and v.dtype == np.float64
    assert np.array_equal(v, rv, equal_nan=True) and np.array_equal(np.signbit(v), np.signbit(rv))
    assert np.array_equal(by, rby) and np.array_equal(do, rdo)
    assert np.array_equal(keys, C.order_keys(rby, rdo), equal_nan=True)
    live = ~np.isnan(rv)
    assert sorted(keys[live].tolist()) == list(range(int(live.sum())))


@pytest.mark.parametrize('K', (1, 3, 8))
@pytest.mark.parametrize('M', (1, 2, 8))
@pytest.mark.parametrize('n', SIZES)
def test_keys_counts_and_violation_are_the_reference(eng, n, M, K):
    for s in C.SHIFTS:
        F, G = C.grid_case(n, M, K, s)
        got = eng.mo_keys(F, G=G, want_counts=True)
        same(got, F, G)
        assert np.array_equal(eng.mo_keys(F, G=G), got[0])                  # (without the counts)
        if s == 1.0:                                       # all feasible: the unconstrained keys
            assert np.array_equal(got[0], R.keys(F))
        elif s == 0.0:                                     # none feasible: ascending violation, then position
            rank = np.empty(n)
            rank[np.argsort(got[3], kind='stable')] = np.arange(n)
            assert (got[3] > 0).all() and np.array_equal(got[0], rank)


def test_tied_violations_and_repeated_rows(eng):
    F, G = C.tied_case()
    got = eng.mo_keys(F, G=G, want_counts=True)
    assert int((got[3] == 0).sum()) == 224 and len(np.unique(got[3])) == 7
    same(got, F, G)


def test_special_values_and_dead_rows(eng):
    F, G = C.special_case()
    keys, by, do, v = eng.mo_keys(F, G=G, want_counts=True)
    same((keys, by, do, v), F, G)
    assert v[[3, 4, 5]].tolist() == [np.inf, np.inf, 1e308] and not np.signbit(v[:3]).any()
    dead = [6, 7, 8, 10]
    assert np.isnan(keys[dead]).all() and np.isnan(v[dead]).all() and (by[dead] == -1).all() \
        and (do[dead] == -1).all()
    # dead rows count for nobody: without them the others keep their keys
    rng = np.random.RandomState(2)
    F = rng.randint(0, 7, (300, 2)).astype(float)
    G = rng.randint(-4, 3, (300, 2)).astype(float)
    bad = rng.choice(300, 60, replace=False)
    F2, G2 = F.copy(), G.copy()
    F2[bad[:20], rng.randint(0, 2, 20)] = np.nan
    G2[bad[20:40], rng.randint(0, 2, 20)] = np.nan
    F2[bad[40:], 0] = np.nan
    G2[bad[40:], 1] = np.nan
    keep = np.setdiff1d(np.arange(300), bad)
    got = eng.mo_keys(F2, G=G2, want_counts=True)
    same(got, F2, G2)
    assert np.array_equal(got[0][keep], C.keys(F[keep], G[keep]))
    assert np.array_equal(got[0][keep], eng.mo_keys(F[keep], G=G[keep]))
    # every row dead
    nan = np.full((3, 2), np.nan)
    for F3, G3 in ((nan, np.zeros((3, 1))), (np.zeros((3, 2)), nan), (nan, nan)):
        keys, by, do, v = eng.mo_keys(F3, G=G3, want_counts=True)
        assert np.isnan(keys).all() and np.isnan(v).all() and by.tolist() == [-1] * 3 and do.tolist() == [-1] * 3


def test_two_calls_give_equal_arrays(eng):
    rng = np.random.RandomState(5)
    F = rng.randint(0, 30, (4097, 2)).astype(float)
    G = rng.randint(-20, 10, (4097, 2)).astype(float)
    a = eng.mo_keys(F, G=G, want_counts=True)
    b = eng.mo_keys(F, G=G, want_counts=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_builders_give_the_same_integers(eng):
    from hyperopt_amd import posterior as P
    rng = np.random.RandomState(7)
    F = rng.randint(0, 12, (1500, 3)).astype(float)
    G = rng.uniform(size=(1500, 2)) - 0.6
    keys, by, do, v = eng.mo_keys(F, G=G, want_counts=True)
    hby, hdo = P.mo_counts(F, G)
    assert np.array_equal(by, hby) and np.array_equal(do, hdo) and np.array_equal(keys, P.mo_keys(F, G=G))
    assert np.array_equal(v, P.mo_violation(G, F))


def test_the_unconstrained_call_is_untouched(eng):
    rng = np.random.RandomState(9)
    F = rng.uniform(size=(3000, 2))
    G = rng.uniform(size=(3000, 3)) - 0.7
    before = eng.mo_keys(F, want_counts=True)
    assert np.array_equal(before[0], R.keys(F))
    eng.mo_keys(F, G=G)
    held = eng.device_bytes()
    after = eng.mo_keys(F, want_counts=True)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    eng.mo_keys(F[:2000], G=G[:2000])
    eng.mo_keys(F, G=G)
    eng.mo_keys(F, G=G[:, :1])
    eng.mo_keys(F)
    assert eng.device_bytes() == held
    assert held >= 3000 * (2 * 8 + 8 + 2 * 4 + 2 * 8) + 3000 * (5 * 8 + 8 + 2 * 4)


def test_its_buffers_are_not_allocated_by_the_unconstrained_call():
    from hyperopt_amd.engine import Engine
    F = np.random.RandomState(10).uniform(size=(3000, 2))
    e = Engine(0, 'f64')
    e.mo_keys(F)
    plain = e.device_bytes()
    e.mo_keys(F)
    assert e.device_bytes() == plain
    e.mo_keys(F, G=F - 0.5)
    assert e.device_bytes() >= plain + 3000 * (4 * 8 + 8 + 2 * 4)
    e.close()


def test_abi_errors_leave_the_outputs_alone(eng):
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import EngineError
    rng = np.random.RandomState(8)
    F, G = rng.uniform(size=(10, 2)), rng.uniform(size=(10, 2)) - 0.5
    keys, v = np.full(10, 7.0), np.full(10, 7.0)
    by = np.full(10, 7, dtype=np.int32)
    do = np.full(10, 7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = (p(keys), p(by), p(do), p(v))
    call = eng.lib.tpe_mo_keys_constrained
    for args in ((p(F), 10, 2, None, 2) + out, (p(F), 10, 2, p(G), 2, None, p(by), p(do), p(v)),
                 (None, 10, 2, p(G), 2) + out,
                 (p(F), 10, 2, p(G), 0) + out, (p(F), 10, 2, p(G), 9) + out,
                 (p(F), 10, 0, p(G), 2) + out, (p(F), 10, 9, p(G), 2) + out,
                 (p(F), 0, 2, p(G), 2) + out, (p(F), (1 << 20) + 1, 2, p(G), 2) + out):
        assert call(eng.h, *args) == L.TPE_ERR_ARG
        assert b'tpe_mo_keys_constrained' in eng.lib.tpe_last_error(eng.h)
    assert (keys == 7.0).all() and (by == 7).all() and (do == 7).all() and (v == 7.0).all()
    assert call(eng.h, p(F), 10, 2, p(G), 2, p(keys), None, None, None) == L.TPE_OK       # each is optional
    assert np.array_equal(keys, C.keys(F, G)) and (by == 7).all() and (v == 7.0).all()
    assert call(eng.h, p(F), 10, 2, p(G), 2, p(keys), None, None, p(v)) == L.TPE_OK
    assert np.array_equal(v, C.violation(F, G)) and (do == 7).all()
    with pytest.raises(ValueError):
        eng.mo_keys(F, G=np.zeros(10))
    with pytest.raises(ValueError):
        eng.mo_keys(F, G=np.zeros((9, 2)))
    with pytest.raises(EngineError):
        eng.mo_keys(np.zeros((0, 2)), G=np.zeros((0, 2)))
    with pytest.raises(EngineError):
        eng.mo_keys(F, G=np.zeros((10, 9)))
    assert L.ABI_VERSION == 5


def test_a_multi_device_context_runs_it_on_its_primary():
    from hyperopt_amd.engine import Engine
    rng = np.random.RandomState(10)
    F = rng.randint(0, 9, (300, 2)).astype(float)
    G = rng.randint(-5, 3, (300, 2)).astype(float)
    two = Engine([0, 0], 'f64')
    same(two.mo_keys(F, G=G, want_counts=True), F, G)
    two.close()


# -- tpe.suggest(constraints=...) ----------------------------------------------

def make_study(shift):
    """300 finished trials with 'loss', 'cost', 'c0' and 'c1', one more whose
    cost is NaN, two pending; and the copy whose 'loss' is the reference key."""
    from hyperopt_amd import tpe
    from hyperopt_amd.base import Domain
    F = np.random.RandomState(0).uniform(size=(300, 2))
    G = np.random.RandomState(1).uniform(size=(300, 2)) - shift
    rows = np.vstack([np.hstack([F, G]), [(0.5, np.nan, -1.0, -1.0)]])
    trials = R.make_trials(space(), rows, names=('loss', 'cost', 'c0', 'c1'), n_pending=2)
    ref = C.keys(rows[:, :2], rows[:, 2:])
    assert np.isnan(ref[300]) and np.array_equal(ref[:300], C.keys(F, G))
    keyed = R.with_loss(trials, ref)
    assert [d['result'].get('loss') for d in keyed.trials[301:]] == [None, None]
    n_below = 5                                    # ceil(0.25 sqrt(303)), the pending ones counted
    below = set(np.argsort(ref[:300])[:n_below].tolist())
    return dict(trials=trials, keyed=keyed, domain=Domain(lambda cfg: 0.0, space()), F=F, G=G, below=below,
                pool=tpe.Pool(space(), points(200, 1)))


@pytest.fixture(scope='module')
def study():
    s = make_study(0.6)
    assert int((C.violation(s['F'], s['G']) == 0).sum()) == 106 and len(C.front(s['F'], s['G'])) == 7
    assert s['below'] == {83, 86, 102, 153, 199}
    unconstrained = set(np.argsort(R.keys(s['F']))[:5].tolist())
    assert unconstrained == {83, 102, 199, 208, 293}
    assert s['below'] != unconstrained             # the test would pass on a call that ignores the keyword otherwise
    return s


@pytest.fixture(scope='module')
def tight_study():
    s = make_study(0.08)
    v = C.violation(s['F'], s['G'])
    assert int((v == 0).sum()) == 2
    assert s['below'] == {13, 60, 72, 211, 263}
    feasible = set(np.flatnonzero(v == 0).tolist())
    assert feasible < s['below'] and len(s['below'] - feasible) == 3      # infeasible trials enter the below set
    return s


def _definition(s, variant, builder):
    from hyperopt_amd import tpe
    kw = dict(VARIANTS[variant], posterior_builder=builder)
    if kw.get('pool') == 'POOL':
        kw['pool'] = s['pool']
    ids = [400, 401, 402]
    got = tpe.suggest(ids, s['domain'], s['trials'], 11, objectives=('loss', 'cost'), constraints=('c0', 'c1'), **kw)
    want = tpe.suggest(ids, s['domain'], s['keyed'], 11, **kw)
    assert len(got) == (3 if 'batch' in kw else 1) and got == want


@pytest.mark.parametrize('builder', ('host', 'device'))
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_the_call_is_the_plain_call_on_the_keys(study, variant, builder):
    _definition(study, variant, builder)


@pytest.mark.parametrize('builder', ('host', 'device'))
@pytest.mark.parametrize('variant', ('plain', 'scott', 'pending'))
def test_infeasible_trials_enter_the_below_set(tight_study, variant, builder):
    _definition(tight_study, variant, builder)


@pytest.fixture(scope='module')
def single():
    from hyperopt_amd.base import Domain
    loss = np.random.RandomState(12).permutation(300) / 7.0          # distinct
    G = np.random.RandomState(1).uniform(size=(300, 1)) - 0.5
    trials = R.make_trials(space(), np.hstack([loss[:, None], G]), names=('loss', 'c'), n_pending=1)
    ref = C.keys(loss[:, None], G)
    assert int((C.violation(loss[:, None], G) == 0).sum()) == 139
    assert set(np.argsort(ref)[:5].tolist()) == {6, 35, 48, 144, 219}
    assert set(np.argsort(loss)[:5].tolist()) == {6, 35, 172, 199, 219}
    return dict(trials=trials, keyed=R.with_loss(trials, ref), domain=Domain(lambda cfg: 0.0, space()), loss=loss)


@pytest.mark.parametrize('kw', [dict(posterior_builder='host'), dict(posterior_builder='device'),
                                dict(posterior_builder='device', multivariate=True)])
def test_one_objective(single, kw):
    from hyperopt_amd import tpe
    s = single
    got = tpe.suggest([400, 401], s['domain'], s['trials'], 3, batch=True, constraints=('c',), **kw)
    assert len(got) == 2 and got == tpe.suggest([400, 401], s['domain'], s['keyed'], 3, batch=True, **kw)
    assert got == tpe.suggest([400, 401], s['domain'], s['trials'], 3, batch=True, constraints=('c',),
                              objectives=('loss',), **kw)
    # every trial feasible, distinct losses: the call without the keyword
    G = -np.random.RandomState(1).uniform(size=(300, 1)) - 0.01
    trials = R.make_trials(space(), np.hstack([s['loss'][:, None], G]), names=('loss', 'c'), n_pending=1)
    got = tpe.suggest([400, 401], s['domain'], trials, 3, batch=True, constraints=('c',), **kw)
    assert len(got) == 2 and got == tpe.suggest([400, 401], s['domain'], trials, 3, batch=True, **kw)


def test_auto_takes_the_kernel_from_its_threshold(study, monkeypatch):
    from hyperopt_amd import engine as E, tpe
    s = study
    asked = []
    real = E.Engine.mo_keys
    monkeypatch.setattr(E.Engine, 'mo_keys',
                        lambda self, F, **k: asked.append((len(F), sorted(k))) or real(self, F, **k))
    kw = dict(objectives=('loss', 'cost'), constraints=('c0', 'c1'))
    want = tpe.suggest([400], s['domain'], s['keyed'], 11)
    monkeypatch.setattr(tpe, 'MO_DEVICE_MIN_TRIALS', 302)
    assert tpe.suggest([400], s['domain'], s['trials'], 11, **kw) == want and not asked
    monkeypatch.setattr(tpe, 'MO_DEVICE_MIN_TRIALS', 301)
    assert tpe.suggest([400], s['domain'], s['trials'], 11, **kw) == want
    assert asked == [(301, ['G'])]                 # once per call, the complete trials (the NaN one too)
    tpe.suggest([400, 401, 402], s['domain'], s['trials'], 11, batch='pending', **kw)
    assert asked == [(301, ['G'])] * 2


def test_a_short_fmin():
    from hyperopt_amd import STATUS_OK, Trials, fmin, hp, tpe
    sp = {'x': hp.uniform('x', 0, 1), 'y': hp.uniform('y', 0, 1)}

    def fn(cfg):
        return {'loss': (cfg['x'] - 1) ** 2 + (cfg['y'] - 1) ** 2, 'c': cfg['x'] + cfg['y'] - 1, 'status': STATUS_OK}
    trials = Trials()
    # (posterior_builder='device': the keys from the kernel at every size, not from the threshold on)
    fmin(fn, sp, algo=partial(tpe.suggest, constraints=('c',), n_startup_jobs=10, posterior_builder='device'),
         max_evals=40, trials=trials, rstate=np.random.RandomState(2))
    assert len(trials.trials) == 40
    F = np.array([[d['result']['loss']] for d in trials.trials])
    G = np.array([[d['result']['c']] for d in trials.trials])
    feasible = np.flatnonzero(G[:, 0] <= 0)
    assert len(feasible)
    best = feasible[F[feasible, 0] == F[feasible, 0].min()]
    assert C.front(F, G).tolist() == best.tolist()
    front = tpe.pareto_front(trials, ('loss',), constraints=('c',))
    assert [d['tid'] for d in front] == [trials.trials[i]['tid'] for i in best]
