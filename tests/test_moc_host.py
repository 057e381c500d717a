"""Constraints, host side: the rule (posterior.mo_violation / mo_counts /
mo_keys with G against tests/moc_reference.py), the rows that stay out of the
ranking, tpe.suggest(constraints=...)'s validation and startup phase, and
tpe.pareto_front with constraints.  No GPU: nothing here reaches an engine."""
import inspect

import numpy as np
import pytest

from hyperopt_amd import hp, posterior as P, tpe
from hyperopt_amd.base import Domain
from tests import mo_reference as R
from tests import moc_reference as C

# loss, cost | c: rows 1 and 4 are equal, row 3 would dominate nobody, row 5
# dominates every other row on F but violates its constraint
WORKED_F = np.array([(1, 5), (2, 2), (5, 1), (3, 3), (2, 2), (0, 0), (4, 4)], dtype=float)
WORKED_G = np.array([(-1,), (0,), (2,), (-1,), (-2,), (1,), (2,)], dtype=float)


def space():
    return {'lr': hp.loguniform('lr', -5, 0), 'wd': hp.uniform('wd', 0, 1)}


def domain():
    return Domain(lambda cfg: 0.0, space())


@pytest.fixture
def no_engine(monkeypatch):
    from hyperopt_amd import engine
    monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))


def same(F, G):
    """The host builder on (F, G) is the reference, exactly; returns (keys, by, do, v)."""
    rby, rdo, rv = C.counts(F, G)
    by, do = P.mo_counts(F, G)
    v = P.mo_violation(G, F)
    keys = P.mo_keys(F, G=G)
    assert by.dtype == np.int32 and do.dtype == np.int32 and keys.dtype == np.float64 and v.dtype == np.float64
    assert np.array_equal(by, rby) and np.array_equal(do, rdo)
    assert np.array_equal(v, rv, equal_nan=True) and np.array_equal(np.signbit(v), np.signbit(rv))
    assert np.array_equal(keys, C.order_keys(rby, rdo), equal_nan=True)
    live = ~np.isnan(rv)
    assert sorted(keys[live].tolist()) == list(range(int(live.sum()))) and np.isnan(keys[~live]).all()
    return keys, by, do, v


def test_worked_example():
    for by, do, v, keys in ((*C.counts(WORKED_F, WORKED_G), C.keys(WORKED_F, WORKED_G)),
                            (*P.mo_counts(WORKED_F, WORKED_G), P.mo_violation(WORKED_G, WORKED_F),
                             P.mo_keys(WORKED_F, G=WORKED_G))):
        assert v.tolist() == [0, 0, 2, 0, 0, 1, 2]
        assert by.tolist() == [0, 0, 5, 2, 0, 4, 5]      # feasible: among 0, 1, 3, 4; infeasible: smaller v
        assert do.tolist() == [0, 1, 0, 0, 1, 0, 0]
        assert keys.tolist() == [2, 0, 5, 3, 1, 4, 6]


@pytest.mark.parametrize('M', (1, 2, 8))
@pytest.mark.parametrize('n', (1, 2, 65, 257, 1000))
def test_builder_is_the_reference(n, M):
    for K in (1, 3, 8):
        for s in C.SHIFTS:
            F, G = C.grid_case(n, M, K, s)
            keys, by, do, v = same(F, G)
            if s == 1.0:                                   # all feasible: the unconstrained keys
                assert (v == 0).all()
                assert np.array_equal(keys, R.keys(F)) and np.array_equal(keys, P.mo_keys(F))
            elif s == 0.0:                                 # none feasible: ascending violation, then position
                assert (v > 0).all() and (do == 0).all()
                rank = np.empty(n)
                rank[np.argsort(v, kind='stable')] = np.arange(n)
                assert np.array_equal(keys, rank)
            elif K == 1 and n >= 65:                       # mixed
                assert 0 < int((v == 0).sum()) < n


def test_tied_violations_and_repeated_rows():
    F, G = C.tied_case()
    keys, by, do, v = same(F, G)
    assert int((v == 0).sum()) == 224 and len(np.unique(v)) == 7
    assert len(F) - len(np.unique(np.hstack([F, G]), axis=0)) > 0
    order = np.argsort(keys)
    bad = order[224:]
    assert (v[order[:224]] == 0).all() and (np.diff(v[bad]) >= 0).all()
    tied = np.flatnonzero(np.diff(v[bad]) == 0)
    assert len(tied) > 400 and (bad[tied] < bad[tied + 1]).all()       # trial order decides ties
    assert (by[bad] >= 224).all() and by[order[:224]].max() < 224


def test_an_infeasible_row_dominates_nobody():
    rng = np.random.RandomState(3)
    F = rng.uniform(size=(200, 2))
    G = rng.uniform(size=(200, 2)) - 0.6
    feas = np.flatnonzero(C.violation(F, G) == 0)
    before = P.mo_counts(F, G)
    F2, G2 = np.vstack([F, [(-1.0, -1.0)]]), np.vstack([G, [(0.25, -1.0)]])
    assert R.dominance(F2)[200, :200].all()                # on F alone it dominates every row
    by, do = same(F2, G2)[1:3]
    assert np.array_equal(by[feas], before[0][feas]) and np.array_equal(do[feas], before[1][feas])
    assert do[200] == 0 and by[200] >= len(feas)
    # feasible, the same row dominates them all
    G2[200] = (-0.25, -1.0)
    by = same(F2, G2)[1]
    assert np.array_equal(by[feas], before[0][feas] + 1) and by[200] == 0


def test_special_values():
    F, G = C.special_case()
    keys, by, do, v = same(F, G)
    inf = np.inf
    want_v = [0, 0, 0, inf, inf, 1e308, np.nan, np.nan, np.nan, 0, np.nan, 2.5, 0, 2.5]
    assert np.array_equal(v, want_v, equal_nan=True) and not np.signbit(v[:3]).any()
    dead = [6, 7, 8, 10]
    assert np.isnan(keys[dead]).all() and (by[dead] == -1).all() and (do[dead] == -1).all()
    # feasible rows 0, 1, 2, 9, 12; 9 = (0.3, 0.3) dominates 2 = (0.5, 0.5), nothing else
    assert by[[0, 1, 2, 9, 12]].tolist() == [0, 0, 1, 0, 0] and do[[0, 1, 2, 9, 12]].tolist() == [0, 0, 0, 1, 0]
    # infeasible: 2.5 (rows 11, 13) < 1e308 (row 5) < inf (rows 3, 4), all behind the 5 feasible rows
    assert by[[11, 13, 5, 3, 4]].tolist() == [5, 5, 7, 8, 8] and (do[[11, 13, 5, 3, 4]] == 0).all()
    assert keys[[11, 13, 5, 3, 4]].tolist() == [5, 6, 7, 8, 9]
    # every row dead
    nan = np.full((3, 2), np.nan)
    for F3, G3 in ((nan, np.zeros((3, 1))), (np.zeros((3, 2)), nan), (nan, nan)):
        keys, by, do, v = same(F3, G3)
        assert np.isnan(keys).all() and np.isnan(v).all() and by.tolist() == [-1] * 3 and do.tolist() == [-1] * 3


def test_dead_rows_count_for_nobody():
    rng = np.random.RandomState(2)
    F = rng.randint(0, 7, (300, 2)).astype(float)
    G = rng.randint(-4, 3, (300, 2)).astype(float)
    bad = rng.choice(300, 60, replace=False)
    F2, G2 = F.copy(), G.copy()
    F2[bad[:20], rng.randint(0, 2, 20)] = np.nan           # NaN only in F
    G2[bad[20:40], rng.randint(0, 2, 20)] = np.nan         # only in G
    F2[bad[40:], 0] = np.nan                               # in both
    G2[bad[40:], 1] = np.nan
    keep = np.setdiff1d(np.arange(300), bad)
    keys, by, do, v = same(F2, G2)
    wby, wdo, wv = C.counts(F[keep], G[keep])
    assert 0 < int((wv == 0).sum()) < len(keep)
    assert np.array_equal(by[keep], wby) and np.array_equal(do[keep], wdo) and np.array_equal(v[keep], wv)
    assert np.array_equal(keys[keep], C.keys(F[keep], G[keep]))
    assert np.isnan(keys[bad]).all() and np.isnan(v[bad]).all() and (by[bad] == -1).all()


def test_shapes_are_checked():
    with pytest.raises(ValueError):
        P.mo_violation(np.zeros((3, 9)))
    with pytest.raises(ValueError):
        P.mo_violation(np.zeros(3))
    with pytest.raises(ValueError):
        P.mo_counts(np.zeros((3, 2)), np.zeros((4, 1)))
    assert P.MO_MAX_CONSTRAINTS == 8
    assert len(P.mo_keys(np.zeros((0, 2)), G=np.zeros((0, 1)))) == 0


# -- tpe.suggest(constraints=...) ----------------------------------------------

def _trials(F=WORKED_F, G=WORKED_G, **kw):
    return R.make_trials(space(), np.hstack([F, G]), names=('loss', 'cost', 'c'), **kw)


@pytest.mark.parametrize('bad', [(), [], 'c', ('c', 'c'), ('c', 3), (b'c',), {'c', 'd'},
                                 tuple('c%d' % i for i in range(9)), ('loss',), ('c', 'loss'), ('cost',),
                                 ('c', 'cost')])
def test_constraints_validation(no_engine, bad):
    with pytest.raises(ValueError, match='constraints'):
        tpe.suggest([10], domain(), _trials(), 1, n_startup_jobs=2, objectives=('loss', 'cost'), constraints=bad)
    with pytest.raises(ValueError, match='constraints'):
        tpe.pareto_front(_trials(), ('loss', 'cost'), constraints=bad)
    if bad not in (('cost',), ('c', 'cost')):              # (without objectives 'cost' is a key like any other)
        with pytest.raises(ValueError, match='constraints'):
            tpe.suggest([10], domain(), _trials(), 1, n_startup_jobs=2, constraints=bad)


def test_constraints_are_checked_before_anything_else(no_engine):
    with pytest.raises(ValueError, match='constraints'):
        tpe.suggest([10], domain(), _trials(), 1, constraints=(), fixed={'nope': 1}, precision='f16')
    with pytest.raises(ValueError, match='objectives'):     # (the objectives first)
        tpe.suggest([10], domain(), _trials(), 1, constraints=(), objectives=())
    assert tpe.check_constraints(None) is None and tpe.check_constraints(None, ('loss',)) is None
    assert tpe.check_constraints(['c', 'd']) == ('c', 'd')
    assert tpe.check_constraints(('cost',)) == ('cost',)
    eight = tuple('c%d' % i for i in range(8))
    assert tpe.check_constraints(eight, ('loss', 'cost')) == eight


def test_a_missing_key_names_the_trial(no_engine):
    trials = _trials(n_pending=1)
    del trials.trials[3]['result']['c']
    for call in (lambda: tpe.suggest([10], domain(), trials, 1, n_startup_jobs=2, constraints=('c',)),
                 lambda: tpe.suggest([10], domain(), trials, 1, n_startup_jobs=2, objectives=('loss', 'cost'),
                                     constraints=('c',)),
                 lambda: tpe.pareto_front(trials, ('loss', 'cost'), constraints=('c',))):
        with pytest.raises(ValueError) as e:
            call()
        assert 'trial 3' in str(e.value) and "'c'" in str(e.value)
    # a pending trial needs none of the keys
    docs, F, G = tpe.objective_rows(trials.trials[:3] + trials.trials[4:], ('loss', 'cost'), domain(),
                                    constraints=('c',))
    assert len(docs) == 6 and F.shape == (6, 2) and G.shape == (6, 1)
    assert np.array_equal(G[:, 0], np.delete(WORKED_G[:, 0], 3))


def test_from_tid_documents_are_refused(no_engine):
    trials = _trials()
    trials.trials[2]['misc']['from_tid'] = 0
    with pytest.raises(ValueError, match='from_tid'):
        tpe.suggest([10], domain(), trials, 1, n_startup_jobs=2, constraints=('c',))


def test_signature():
    params = list(inspect.signature(tpe.suggest).parameters.values())
    assert [p.name for p in params[-3:]] == ['pool_replace', 'constraints', 'objectives']
    assert params[-2].default is None
    front = list(inspect.signature(tpe.pareto_front).parameters.values())
    assert [p.name for p in front] == ['trials', 'objectives', 'constraints'] and front[-1].default is None


def test_startup_phase_is_unchanged(no_engine):
    trials = _trials(n_pending=1)
    for extra in (dict(), dict(batch=True), dict(batch='pending'), dict(fixed={'wd': 0.25})):
        plain = tpe.suggest([10, 11, 12], domain(), trials, 5, posterior_builder='host', **extra)
        for kw in (dict(constraints=('c',)), dict(constraints=('c',), objectives=('loss', 'cost'))):
            got = tpe.suggest([10, 11, 12], domain(), trials, 5, posterior_builder='host', **dict(extra, **kw))
            assert len(plain) == 3 and got == plain


def test_rows_keys_and_incomplete_trials():
    trials = _trials(np.vstack([WORKED_F, [(0.0, 0.0), (1.0, 1.0)]]), np.vstack([WORKED_G, [(np.nan,), (-1.0,)]]),
                     n_pending=2)
    trials.trials[8]['result'] = {'status': 'fail'}
    trials.refresh()
    docs, F, G = tpe.objective_rows(trials.trials, ('loss', 'cost'), domain(), constraints=('c',))
    assert [d['tid'] for d in docs] == list(range(8)) and np.isnan(G[7, 0])
    keys = tpe.objective_keys(F, 'host', G=G)
    assert keys[:7].tolist() == [2, 0, 5, 3, 1, 4, 6] and np.isnan(keys[7])
    # one objective: 'loss' through the domain
    docs, F1, G1 = tpe.objective_rows(trials.trials, ('loss',), domain(), constraints=('c',))
    assert np.array_equal(F1[:, 0], F[:, 0]) and np.array_equal(G1, G, equal_nan=True)
    assert tpe.objective_keys(F1, 'host', G=G1)[:7].tolist() == [0, 1, 5, 3, 2, 4, 6]


def test_pareto_front_with_constraints():
    trials = _trials(n_pending=1)
    assert [d['tid'] for d in tpe.pareto_front(trials, ('loss', 'cost'))] == [5]
    assert [d['tid'] for d in tpe.pareto_front(trials, ('loss', 'cost'), constraints=('c',))] == [0, 1, 4]
    assert [d['tid'] for d in tpe.pareto_front(trials, ('loss', 'cost'), constraints=['c'])] \
        == C.front(WORKED_F, WORKED_G).tolist()
    # one objective: the best feasible trial(s)
    assert [d['tid'] for d in tpe.pareto_front(trials, ('loss',), constraints=('c',))] == [0]
    assert [d['tid'] for d in tpe.pareto_front(trials, ('cost',), constraints=('c',))] == [1, 4]
    # 'cost' as the constraint: only trial 5's cost of 0 satisfies it
    assert [d['tid'] for d in tpe.pareto_front(trials, ('loss',), constraints=('cost',))] == [5]
    # nothing feasible: no front, although the least-violating trial has by == 0
    for d in trials.trials[:7]:
        d['result']['c'] = abs(d['result']['c']) + 1.0
    assert P.mo_counts(WORKED_F, np.abs(WORKED_G) + 1.0)[0].min() == 0
    assert tpe.pareto_front(trials, ('loss', 'cost'), constraints=('c',)) == []
    # a NaN constraint takes a trial off the front
    for d, c in zip(trials.trials, WORKED_G[:, 0]):
        d['result']['c'] = float(c)
    trials.trials[1]['result']['c'] = float('nan')
    assert [d['tid'] for d in tpe.pareto_front(trials, ('loss', 'cost'), constraints=('c',))] == [0, 4]
    from hyperopt_amd import Trials
    assert tpe.pareto_front(Trials(), ('loss',), constraints=('c',)) == []
