"""tpe.Pool and the host side of tpe.suggest(pool=...): validation, the
values matrix, the taken set, the startup phase and the early errors -- no
GPU is touched (the startup phase ranks nothing) -- and the reference
ranking of tests/pool_reference.py against the oracle's broadcast_best."""
import types
from functools import partial

import numpy as np
import pytest

from hyperopt_amd import Trials, fmin, hp, tpe
from hyperopt_amd.base import Domain, JOB_STATE_DONE, JOB_STATE_ERROR, JOB_STATE_NEW, JOB_STATE_RUNNING
from oracle import tpe_oracle as O
from tests import pool_reference as R


def space():
    return {'lr': hp.loguniform('lr', -5, 0),
            'width': hp.quniform('width', 16, 64, 16),
            'opt': hp.choice('opt', [{'momentum': hp.uniform('momentum', 0, 1)},
                                     {'beta': hp.uniform('beta', 0.5, 1), 'eps': hp.lognormal('eps', -8, 1)}])}


LABELS = ['beta', 'eps', 'lr', 'momentum', 'opt', 'width']


def points(n, seed=0):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        p = {'lr': float(np.exp(rng.uniform(-5, 0))), 'width': float(16 * rng.randint(1, 5)),
             'opt': int(rng.randint(2))}
        if p['opt'] == 0:
            p['momentum'] = float(rng.uniform(0, 1))
        else:
            p['beta'] = float(rng.uniform(0.5, 1))
            p['eps'] = float(np.exp(rng.normal(-8, 1)))
        out.append(p)
    return out


def loss(cfg):
    return (np.log(cfg['lr']) + 2.0) ** 2 + cfg['width'] / 64.0


def test_pool_values_matrix_and_points():
    pts = points(7)
    pool = tpe.Pool(space(), pts)
    assert len(pool) == 7 and pool.labels == LABELS
    assert pool.values.shape == (7, 6) and pool.values.dtype == np.float64
    for i, p in enumerate(pts):
        for c, k in enumerate(LABELS):
            if k in p:
                assert pool.values[i, c] == float(p[k])
            else:
                assert np.isnan(pool.values[i, c])
        assert pool.points[i] == p and isinstance(pool.points[i]['opt'], int)
    # a Domain gives the same pool; tokens are unique per object
    other = tpe.Pool(Domain(loss, space()), pts)
    assert np.array_equal(other.values, pool.values, equal_nan=True)
    assert other.token != pool.token


@pytest.mark.parametrize('bad, words', [
    (dict(lr=0.1, width=32.0, opt=0, momentum=0.5, nope=1.0), ('entry 1', "'nope'", 'unknown')),
    (dict(lr=0.1, width=32.0, opt=0, momentum=1.5), ('entry 1', "'momentum'", 'outside')),
    (dict(lr=-0.1, width=32.0, opt=0, momentum=0.5), ('entry 1', "'lr'", 'not positive')),
    (dict(lr=0.1, width=33.0, opt=0, momentum=0.5), ('entry 1', "'width'", 'grid')),
    (dict(lr=0.1, width=32.0, opt=2, momentum=0.5), ('entry 1', "'opt'", 'integer')),
    (dict(lr=0.1, width=32.0, opt=0.5, momentum=0.5), ('entry 1', "'opt'", 'integer')),
    (dict(lr=float('nan'), width=32.0, opt=0, momentum=0.5), ('entry 1', "'lr'", 'finite')),
    (dict(lr='x', width=32.0, opt=0, momentum=0.5), ('entry 1', "'lr'", 'number')),
    # the wrong active set: a label of the other branch, a missing one
    (dict(lr=0.1, width=32.0, opt=0, momentum=0.5, beta=0.7), ('entry 1', "'beta'", 'not active')),
    (dict(lr=0.1, width=32.0, opt=1, beta=0.7), ('entry 1', "'eps'", 'no value')),
    (dict(lr=0.1, width=32.0, momentum=0.5), ('entry 1', "'opt'", 'no value')),
])
def test_pool_validation(bad, words):
    good = points(1)[0]
    with pytest.raises(ValueError) as e:
        tpe.Pool(space(), [good, bad])
    for w in words:
        assert w in str(e.value), str(e.value)


def test_pool_refuses_empty_and_non_dicts():
    with pytest.raises(ValueError):
        tpe.Pool(space(), [])
    with pytest.raises(ValueError):
        tpe.Pool(space(), [[0.1, 32.0]])


def test_check_fixed_keeps_its_messages():
    specs = tpe.specs_of(Domain(loss, space()))
    assert tpe.check_fixed(specs, {'opt': 1.0, 'lr': 0.5}) == {'opt': 1, 'lr': 0.5}
    for fixed, msg in [({'lr': 3.0}, "fixed['lr']: 3.0 is outside ["),
                       ({'width': 33}, "fixed['width']: 33 is not on the grid of step 16"),
                       ({'opt': 2}, "fixed['opt']: 2 is not an integer in [0, 2)"),
                       ({'zz': 1}, "fixed: unknown label 'zz'"),
                       ({'lr': 'a'}, "fixed['lr']: 'a' is not a number")]:
        with pytest.raises(ValueError) as e:
            tpe.check_fixed(specs, fixed)
        assert str(e.value).startswith(msg), str(e.value)


def _with_docs(domain, pool, marks):
    """Trials holding one document per (state, pool_index value)."""
    trials = Trials()
    docs = []
    for tid, (state, mark) in enumerate(marks):
        d = tpe._pool_doc(tid, domain, trials, tpe.specs_of(domain), pool, 0)[0]
        d['misc'].pop('pool_index')
        if mark is not None:
            d['misc']['pool_index'] = mark
        d['state'] = state
        if state == JOB_STATE_DONE:
            d['result'] = {'loss': 1.0, 'status': 'ok'}
        docs.append(d)
    trials.insert_trial_docs(docs)
    trials.refresh()
    return trials


def test_taken_set_from_documents_in_every_state():
    domain = Domain(loss, space())
    pool = tpe.Pool(domain, points(10))
    marks = [(JOB_STATE_NEW, 3), (JOB_STATE_RUNNING, 5), (JOB_STATE_DONE, 7), (JOB_STATE_ERROR, 1),
             (JOB_STATE_DONE, 3),                      # twice
             (JOB_STATE_DONE, None), (JOB_STATE_DONE, 10), (JOB_STATE_DONE, -1), (JOB_STATE_DONE, 'x'),
             (JOB_STATE_DONE, 2.0), (JOB_STATE_DONE, np.int64(8))]
    trials = _with_docs(domain, pool, marks)
    # (Trials.refresh keeps errored documents out of trials.trials: entry 1 is free again)
    assert tpe.pool_taken(pool, trials) == [3, 5, 7, 8]
    # the state itself is not looked at: a view that lists the errored document too
    every = types.SimpleNamespace(trials=list(trials._dynamic_trials))
    assert len(every.trials) == len(marks)
    assert tpe.pool_taken(pool, every) == [1, 3, 5, 7, 8]


def test_startup_documents():
    domain = Domain(loss, space())
    pool = tpe.Pool(domain, points(6))
    trials = _with_docs(domain, pool, [(JOB_STATE_DONE, 4), (JOB_STATE_NEW, 0)])
    kw = dict(n_startup_jobs=100, pool=pool)
    docs = tpe.suggest([10, 11, 12], domain, trials, 7, **kw)
    # seeded: free[rng.randint(len(free))] of the untaken, in ascending order, without replacement
    rng, free, want = np.random.RandomState(7), [1, 2, 3, 5], []
    for _ in range(3):
        want.append(free.pop(int(rng.randint(len(free)))))
    assert [d['misc']['pool_index'] for d in docs] == want and len(set(want)) == 3
    assert [d['tid'] for d in docs] == [10, 11, 12]
    for d, i in zip(docs, want):
        vals = {k: v[0] for k, v in d['misc']['vals'].items() if v}
        assert vals == pool.points[i]
        assert {k for k, v in d['misc']['idxs'].items() if v} == set(pool.points[i])
        assert all(v == [d['tid']] for v in d['misc']['idxs'].values() if v)
    again = tpe.suggest([10, 11, 12], domain, trials, 7, **kw)
    assert [d['misc']['pool_index'] for d in again] == want
    # batch='pending' answers a startup batch the same way
    pend = tpe.suggest([10, 11, 12], domain, trials, 7, batch='pending', **kw)
    assert [d['misc']['pool_index'] for d in pend] == want
    # fewer when the pool runs out, [] when nothing is free
    docs = tpe.suggest(list(range(10, 16)), domain, trials, 3, **kw)
    assert sorted(d['misc']['pool_index'] for d in docs) == [1, 2, 3, 5]
    full = _with_docs(domain, pool, [(JOB_STATE_DONE, i) for i in range(6)])
    assert tpe.suggest([20], domain, full, 3, **kw) == []
    assert tpe.suggest([20], domain, full, 3, n_startup_jobs=0, pool=pool) == []   # (before any engine)
    # pool_replace takes nothing
    docs = tpe.suggest(list(range(20, 28)), domain, full, 3, pool_replace=True, **kw)
    assert sorted(d['misc']['pool_index'] for d in docs) == [0, 1, 2, 3, 4, 5]


def test_fmin_visits_every_entry_once_and_stops():
    pts = points(15, seed=3)
    pool = tpe.Pool(space(), pts)
    trials = Trials()
    fmin(loss, space(), algo=partial(tpe.suggest, pool=pool, n_startup_jobs=100), max_evals=30,
         trials=trials, rstate=np.random.RandomState(0))
    assert len(trials.trials) == 15
    assert sorted(d['misc']['pool_index'] for d in trials.trials) == list(range(15))
    got = sorted(trials.losses())
    assert got == sorted(loss(p) for p in pts)


def test_early_errors_touch_no_engine(monkeypatch):
    from hyperopt_amd import engine
    monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    domain = Domain(loss, space())
    pool = tpe.Pool(domain, points(5))
    trials = Trials()
    with pytest.raises(ValueError, match='filter the pool'):
        tpe.suggest([0], domain, trials, 1, pool=pool, fixed={'opt': 0})
    with pytest.raises(ValueError, match='one device'):
        tpe.suggest([0], domain, trials, 1, pool=pool, devices=[0, 1])
    with pytest.raises(ValueError, match='needs a pool'):
        tpe.suggest([0], domain, trials, 1, pool_replace=True)
    other = tpe.Pool({'x': hp.uniform('x', 0, 1)}, [{'x': 0.5}])
    with pytest.raises(ValueError, match="not the domain's"):
        tpe.suggest([0], domain, trials, 1, pool=other)
    with pytest.raises(ValueError, match='tpe.Pool'):
        tpe.suggest([0], domain, trials, 1, pool=points(5))


def test_reference_rank_is_broadcast_best():
    rng = np.random.RandomState(11)
    inf, nan = np.inf, np.nan
    cases = [[1.0, 3.0, 3.0, 2.0], [0.0, -0.0, -1.0], [-0.0, 0.0], [-inf, -inf], [inf, 1.0, inf],
             [1.0, nan, inf, nan], [nan], [-inf, nan, inf], [2.0, inf, -inf, inf]]
    cases += [rng.choice([-inf, -1.0, 0.0, 0.5, 0.5, inf, nan], size=9).tolist() for _ in range(40)]
    for s in cases:
        s = np.asarray(s)
        assert R.rank(s, 1)[0] == O.broadcast_best_index(s, np.zeros(len(s))), s
        full = R.rank(s, len(s))
        assert sorted(full.tolist()) == list(range(len(s)))
        # taken entries leave the order of the others as it is
        assert R.rank(s, len(s), taken=[0]).tolist() == [i for i in full.tolist() if i != 0]
    assert R.rank([1.0, 2.0], 5, taken=[1, 1, 7, -3]).tolist() == [0]
