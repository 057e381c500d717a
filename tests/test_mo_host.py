"""Several objectives, host side: the rule (posterior.mo_counts / mo_keys
against tests/mo_reference.py and a worked example), the rows that stay out of
the ranking, tpe.suggest(objectives=...)'s validation and startup phase, and
tpe.pareto_front.  No GPU: nothing here reaches an engine."""
import inspect

import numpy as np
import pytest

from hyperopt_amd import hp, posterior as P, tpe
from hyperopt_amd.base import Domain
from tests import mo_reference as R

WORKED = np.array([(1, 5), (2, 2), (5, 1), (3, 3), (2, 2)], dtype=float)


def space():
    return {'lr': hp.loguniform('lr', -5, 0), 'wd': hp.uniform('wd', 0, 1)}


def domain():
    return Domain(lambda cfg: 0.0, space())


@pytest.fixture
def no_engine(monkeypatch):
    from hyperopt_amd import engine
    monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))


def test_worked_example():
    for counts, keys in ((R.counts, R.keys), (P.mo_counts, P.mo_keys)):
        by, do = counts(WORKED)
        assert by.tolist() == [0, 0, 0, 2, 0]
        assert do.tolist() == [0, 1, 0, 0, 1]
        assert keys(WORKED).tolist() == [2, 0, 3, 4, 1]


@pytest.mark.parametrize('n, M, seed', [(1, 2, 0), (2, 3, 1), (257, 1, 2), (257, 2, 3), (500, 8, 4), (3000, 2, 5),
                                        (3000, 3, 6)])
def test_builder_is_the_reference(n, M, seed):
    rng = np.random.RandomState(seed)
    for F in (rng.uniform(size=(n, M)), rng.randint(0, 6, (n, M)).astype(float)):
        by, do = P.mo_counts(F)
        rby, rdo = R.counts(F)
        assert by.dtype == np.int32 and do.dtype == np.int32
        assert np.array_equal(by, rby) and np.array_equal(do, rdo)
        keys = P.mo_keys(F)
        assert keys.dtype == np.float64 and np.array_equal(keys, R.keys(F))
        assert sorted(keys.tolist()) == list(range(n))


def test_3000_rows_cross_the_chunk_boundary():
    assert 1 <= P.MO_CHUNK_BYTES // (8 * 3000) < 3000
    assert P.MO_CHUNK_BYTES <= 64 << 20


def test_one_objective_is_the_stable_argsort():
    v = np.random.RandomState(0).randint(0, 20, 200).astype(float)
    rank = np.empty(200)
    rank[np.argsort(v, kind='stable')] = np.arange(200)
    assert np.array_equal(P.mo_keys(v[:, None]), rank)
    assert np.array_equal(R.keys(v[:, None]), rank)


def test_objective_order_and_increasing_maps_change_nothing():
    rng = np.random.RandomState(1)
    F = rng.randint(0, 9, (400, 3)).astype(float)
    want = P.mo_keys(F)
    assert np.array_equal(P.mo_keys(F[:, [2, 0, 1]]), want)
    G = F.copy()
    G[:, 1] = np.exp(0.5 * G[:, 1]) - 3.0
    assert np.array_equal(P.mo_keys(G), want)


def test_special_values():
    F = np.array([(0.0, 1.0), (-0.0, 1.0), (-np.inf, np.inf), (np.inf, -np.inf), (np.inf, np.inf),
                  (-np.inf, -np.inf), (np.nan, 0.0), (0.0, np.nan)])
    by, do = P.mo_counts(F)
    rby, rdo = R.counts(F)
    assert np.array_equal(by, rby) and np.array_equal(do, rdo)
    assert by.tolist() == [1, 1, 1, 1, 5, 0, -1, -1]       # -0.0 equals 0.0: rows 0 and 1 do not dominate each other
    assert do.tolist() == [1, 1, 1, 1, 0, 5, -1, -1]
    keys = P.mo_keys(F)
    assert np.array_equal(keys, R.keys(F), equal_nan=True)
    assert np.isnan(keys[6:]).all() and sorted(keys[:6].tolist()) == list(range(6))


def test_nan_rows_count_for_nobody():
    rng = np.random.RandomState(2)
    F = rng.randint(0, 7, (300, 2)).astype(float)
    bad = rng.choice(300, 40, replace=False)
    G = F.copy()
    G[bad, rng.randint(0, 2, 40)] = np.nan
    keep = np.setdiff1d(np.arange(300), bad)
    by, do = P.mo_counts(G)
    wby, wdo = R.counts(F[keep])
    assert np.array_equal(by[keep], wby) and np.array_equal(do[keep], wdo)
    assert (by[bad] == -1).all() and (do[bad] == -1).all()
    keys = P.mo_keys(G)
    assert np.isnan(keys[bad]).all() and np.array_equal(keys[keep], R.keys(F[keep]))


def _trials(F=WORKED, **kw):
    return R.make_trials(space(), F, **kw)


def test_rows_of_pending_failed_and_nan_trials():
    trials = _trials(np.vstack([WORKED, [(np.nan, 0.0), (0.0, 0.0)]]), n_pending=2)
    failed = trials.trials[6]
    failed['result'] = {'status': 'fail'}
    trials.refresh()
    docs, F = tpe.objective_rows(trials.trials, ('loss', 'cost'), domain())
    assert [d['tid'] for d in docs] == [0, 1, 2, 3, 4, 5]
    assert np.array_equal(F[:5], WORKED) and np.isnan(F[5, 0]) and F[5, 1] == 0.0
    keys = tpe.objective_keys(F, 'host')
    assert keys[:5].tolist() == [2, 0, 3, 4, 1] and np.isnan(keys[5])
    # the keyed domain: the key for a complete trial, NaN kept, None for the rest
    keyed = tpe._KeyedDomain(domain(), docs, keys)
    col = keyed.loss_column(trials.trials)
    assert col[:5] == [2.0, 0.0, 3.0, 4.0, 1.0] and np.isnan(col[5]) and col[6:] == [None] * 3
    assert [keyed.loss(d['result'], d['spec']) for d in trials.trials[:5]] == col[:5]
    from hyperopt_amd import history
    tids, losses, _ = history.gather(keyed, trials, ['lr', 'wd'])
    assert tids.tolist() == [0, 1, 2, 3, 4, 6, 7, 8]
    assert losses.tolist() == [2, 0, 3, 4, 1, np.inf, np.inf, np.inf]
    view = history.device_view(keyed, trials, ['lr', 'wd'])
    assert view[2] == 8 and np.isnan(view[1][5]) and view[1][:5].tolist() == [2, 0, 3, 4, 1]
    assert keyed.expr is keyed._domain.expr


@pytest.mark.parametrize('bad', [(), [], 'loss', ('loss', 'loss'), ('loss', 3), (b'loss',), {'loss', 'cost'},
                                 tuple('o%d' % i for i in range(9))])
def test_objectives_validation(no_engine, bad):
    with pytest.raises(ValueError, match='objectives'):
        tpe.suggest([10], domain(), _trials(), 1, n_startup_jobs=2, objectives=bad)
    with pytest.raises(ValueError, match='objectives'):
        tpe.pareto_front(_trials(), bad)


def test_objectives_are_checked_before_anything_else(no_engine):
    with pytest.raises(ValueError, match='objectives'):
        tpe.suggest([10], domain(), _trials(), 1, objectives=(), fixed={'nope': 1}, precision='f16')
    assert tpe.check_objectives(None) is None
    assert tpe.check_objectives(['loss', 'cost']) == ('loss', 'cost')
    assert tpe.check_objectives(tuple('o%d' % i for i in range(8))) == tuple('o%d' % i for i in range(8))


def test_a_missing_key_names_the_trial(no_engine):
    trials = _trials(n_pending=1)
    del trials.trials[3]['result']['cost']
    for call in (lambda: tpe.suggest([10], domain(), trials, 1, n_startup_jobs=2, objectives=('loss', 'cost')),
                 lambda: tpe.pareto_front(trials, ('loss', 'cost'))):
        with pytest.raises(ValueError) as e:
            call()
        assert 'trial 3' in str(e.value) and "'cost'" in str(e.value)
    # a pending trial needs none of the keys
    assert len(tpe.objective_rows(trials.trials[:3] + trials.trials[4:], ('loss', 'cost'), domain())[0]) == 4


def test_from_tid_documents_are_refused(no_engine):
    trials = _trials()
    trials.trials[2]['misc']['from_tid'] = 0
    with pytest.raises(ValueError, match='from_tid'):
        tpe.suggest([10], domain(), trials, 1, n_startup_jobs=2, objectives=('loss', 'cost'))
    trials.trials[2]['misc']['from_tid'] = 2       # its own tid: no group
    assert len(tpe.objective_rows(trials.trials, ('loss', 'cost'), domain())[0]) == 5


def test_signature():
    params = list(inspect.signature(tpe.suggest).parameters.values())
    assert params[-1].name == 'objectives' and params[-1].default is None


def test_startup_phase_is_unchanged(no_engine):
    trials = _trials(n_pending=1)
    for extra in (dict(), dict(batch=True), dict(batch='pending'), dict(fixed={'wd': 0.25})):
        plain = tpe.suggest([10, 11, 12], domain(), trials, 5, posterior_builder='host', **extra)
        multi = tpe.suggest([10, 11, 12], domain(), trials, 5, posterior_builder='host',
                            objectives=('loss', 'cost'), **extra)
        assert len(plain) == 3 and multi == plain


def test_pareto_front():
    trials = _trials(n_pending=1)
    assert [d['tid'] for d in tpe.pareto_front(trials, ('loss', 'cost'))] == [0, 1, 2, 4]
    assert [d['tid'] for d in tpe.pareto_front(trials, ['cost'])] == [2]
    assert [d['tid'] for d in tpe.pareto_front(trials, ('cost', 'loss'))] == R.front(WORKED).tolist()
    trials.trials[1]['result']['cost'] = float('nan')
    assert [d['tid'] for d in tpe.pareto_front(trials, ('loss', 'cost'))] == [0, 2, 4]
    from hyperopt_amd import Trials
    assert tpe.pareto_front(Trials(), ('loss', 'cost')) == []
