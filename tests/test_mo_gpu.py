"""Several objectives on the device: Engine.mo_keys (tpe_mo_keys,
hyperopt_amd/csrc/tpe_mo.hip) against the plain numpy statement of the rule
(tests/mo_reference.py), exactly -- keys and both counts are integers -- and
tpe.suggest(objectives=...) against its definition: the plain call on a copy
of the trials whose 'loss' is the reference key."""
import ctypes
from functools import partial

import numpy as np
import pytest

from tests import mo_reference as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 1000, 4097)     # one row; the wave and block edges; several j-slices
OBJ = (1, 2, 3, 8)


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


def same(got, want):
    keys, by, do = got
    rby, rdo = R.counts(want)
    assert keys.dtype == np.float64 and by.dtype == np.int32 and do.dtype == np.int32
    assert np.array_equal(by, rby) and np.array_equal(do, rdo)
    assert np.array_equal(keys, R.keys(want), equal_nan=True)


@pytest.mark.parametrize('M', OBJ)
@pytest.mark.parametrize('n', SIZES)
def test_keys_and_counts_are_the_reference(eng, n, M):
    F = np.random.RandomState(1000 * M + n).uniform(size=(n, M))
    got = eng.mo_keys(F, want_counts=True)
    same(got, F)
    assert sorted(got[0].tolist()) == list(range(n))
    assert np.array_equal(eng.mo_keys(F), got[0])          # (without the counts)


def test_repeated_rows_position_decides():
    from hyperopt_amd.engine import Engine
    F = np.random.RandomState(6).randint(0, 6, (500, 2)).astype(float)
    assert len(F) - len(np.unique(F, axis=0)) == 464
    by, do = R.counts(F)
    order = np.argsort(R.keys(F))
    a, b = order[5], order[6]                      # either side of a cut at 6
    assert (by[a], do[a]) == (by[b], do[b]) and a < b
    e = Engine(0, 'f64')
    same(e.mo_keys(F, want_counts=True), F)
    e.close()


def test_a_wide_front(eng):
    F = np.random.RandomState(3).uniform(size=(257, 8))
    by, do = R.counts(F)
    assert int((by == 0).sum()) == 198
    order = np.argsort(R.keys(F))
    assert (by[order[4]], do[order[4]]) == (by[order[5]], do[order[5]])      # a tie at the cut of 5
    same(eng.mo_keys(F, want_counts=True), F)


def test_special_values_and_nan_rows(eng):
    rng = np.random.RandomState(4)
    F = rng.randint(0, 4, (700, 3)).astype(float)
    F[rng.choice(700, 60, replace=False), rng.randint(0, 3, 60)] = np.inf
    F[rng.choice(700, 60, replace=False), rng.randint(0, 3, 60)] = -np.inf
    F[rng.choice(700, 100, replace=False), rng.randint(0, 3, 100)] = -0.0
    bad = rng.choice(700, 50, replace=False)
    G = F.copy()
    G[bad, rng.randint(0, 3, 50)] = np.nan
    G[bad[0]] = np.nan
    keys, by, do = eng.mo_keys(G, want_counts=True)
    same((keys, by, do), G)
    assert np.isnan(keys[bad]).all() and (by[bad] == -1).all() and (do[bad] == -1).all()
    keep = np.setdiff1d(np.arange(700), bad)
    wby, wdo = R.counts(F[keep])                   # the history without them
    assert np.array_equal(by[keep], wby) and np.array_equal(do[keep], wdo)
    assert np.array_equal(keys[keep], R.keys(F[keep]))
    # -0.0 equals 0.0
    Z = F.copy()
    Z[Z == 0.0] = 0.0
    assert np.array_equal(eng.mo_keys(Z), eng.mo_keys(F))
    # every row NaN
    keys, by, do = eng.mo_keys(np.full((3, 2), np.nan), want_counts=True)
    assert np.isnan(keys).all() and by.tolist() == [-1] * 3 and do.tolist() == [-1] * 3


def test_two_calls_give_equal_arrays(eng):
    F = np.random.RandomState(5).randint(0, 30, (4097, 2)).astype(float)
    a = eng.mo_keys(F, want_counts=True)
    b = eng.mo_keys(F, want_counts=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_builders_give_the_same_integers(eng):
    from hyperopt_amd import posterior as P
    F = np.random.RandomState(7).randint(0, 12, (1500, 3)).astype(float)
    keys, by, do = eng.mo_keys(F, want_counts=True)
    hby, hdo = P.mo_counts(F)
    assert np.array_equal(by, hby) and np.array_equal(do, hdo) and np.array_equal(keys, P.mo_keys(F))


def test_abi_errors_leave_the_outputs_alone(eng):
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import EngineError
    F = np.random.RandomState(8).uniform(size=(10, 2))
    keys = np.full(10, 7.0)
    by = np.full(10, 7, dtype=np.int32)
    do = np.full(10, 7, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call = eng.lib.tpe_mo_keys
    for args in ((p(F), 10, 0, p(keys), p(by), p(do)), (p(F), 10, 9, p(keys), p(by), p(do)),
                 (p(F), 0, 2, p(keys), p(by), p(do)), (p(F), (1 << 20) + 1, 2, p(keys), p(by), p(do)),
                 (None, 10, 2, p(keys), p(by), p(do)), (p(F), 10, 2, None, p(by), p(do))):
        assert call(eng.h, *args) == L.TPE_ERR_ARG
        assert b'tpe_mo_keys' in eng.lib.tpe_last_error(eng.h)
    assert (keys == 7.0).all() and (by == 7).all() and (do == 7).all()
    assert call(eng.h, p(F), 10, 2, p(keys), None, None) == L.TPE_OK          # the counts are optional
    assert np.array_equal(keys, R.keys(F)) and (by == 7).all()
    with pytest.raises(ValueError):
        eng.mo_keys(np.zeros(4))
    with pytest.raises(EngineError):
        eng.mo_keys(np.zeros((0, 2)))
    assert L.ABI_VERSION == 5


def test_buffers_are_counted_and_reused(eng):
    F = np.random.RandomState(9).uniform(size=(3000, 2))
    eng.mo_keys(F)
    held = eng.device_bytes()
    assert held >= 3000 * (2 * 8 + 8 + 2 * 4 + 2 * 8)
    eng.mo_keys(F[:2000])
    eng.mo_keys(F)
    assert eng.device_bytes() == held


def test_a_multi_device_context_runs_it_on_its_primary():
    from hyperopt_amd.engine import Engine
    F = np.random.RandomState(10).randint(0, 9, (300, 2)).astype(float)
    two = Engine([0, 0], 'f64')
    same(two.mo_keys(F, want_counts=True), F)
    two.close()


# -- tpe.suggest(objectives=...) -----------------------------------------------

def space():
    from hyperopt_amd import hp
    return {'lr': hp.loguniform('lr', -5, 0), 'wd': hp.uniform('wd', 0, 1), 'mom': hp.normal('mom', 0.5, 0.2),
            'bs': hp.quniform('bs', 8, 256, 8), 'act': hp.choice('act', ['relu', 'gelu', 'tanh'])}


def points(n, seed):
    from hyperopt_amd import labels as LB
    from hyperopt_amd.space import as_apply
    expr = as_apply(space())
    specs = LB.compile_space(expr)
    rng = np.random.RandomState(seed)
    return [LB.sample_config(expr, specs, rng) for _ in range(n)]


@pytest.fixture(scope='module')
def study():
    """300 finished trials with 'loss' and 'cost', one more whose cost is NaN,
    two pending; and the copy whose 'loss' is the reference key (NaN kept for
    the NaN trial, nothing for the pending ones)."""
    from hyperopt_amd import tpe
    from hyperopt_amd.base import Domain
    F = np.random.RandomState(0).uniform(size=(300, 2))
    rows = np.vstack([F, [(0.5, np.nan)]])
    trials = R.make_trials(space(), rows, n_pending=2)
    ref = R.keys(rows)
    assert np.isnan(ref[300]) and np.array_equal(ref[:300], R.keys(F))
    keyed = R.with_loss(trials, ref)
    assert [d['result'].get('loss') for d in keyed.trials[301:]] == [None, None]
    n_below = 5                                    # ceil(0.25 sqrt(302)), the pending ones counted
    assert len(R.front(F)) == 9
    below = np.argsort(ref[:300])[:n_below]
    assert (R.counts(F)[0][below] == 0).all()      # the whole below set is on the front
    # the test would pass on a call that ignores the keyword otherwise
    assert set(below.tolist()) != set(np.argsort(F[:, 0], kind='stable')[:n_below].tolist())
    return dict(trials=trials, keyed=keyed, domain=Domain(lambda cfg: 0.0, space()), F=F,
                pool=tpe.Pool(space(), points(200, 1)))


VARIANTS = {
    'plain': dict(),
    'scott': dict(multivariate=True, joint_bandwidth='scott'),
    'fixed': dict(fixed={'wd': 0.5, 'act': 1}),
    'pool': dict(pool='POOL'),
    'batch': dict(batch=True),
    'pending': dict(batch='pending'),
    'devices': dict(devices=[0, 0]),
}


@pytest.mark.parametrize('builder', ('host', 'device'))
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_the_call_is_the_plain_call_on_the_keys(study, variant, builder):
    from hyperopt_amd import tpe
    s = study
    kw = dict(VARIANTS[variant], posterior_builder=builder)
    if kw.get('pool') == 'POOL':
        kw['pool'] = s['pool']
    ids = [400, 401, 402]
    got = tpe.suggest(ids, s['domain'], s['trials'], 11, objectives=('loss', 'cost'), **kw)
    want = tpe.suggest(ids, s['domain'], s['keyed'], 11, **kw)
    assert len(got) == (3 if 'batch' in kw else 1) and got == want


def test_auto_takes_the_kernel_from_its_threshold(study, monkeypatch):
    from hyperopt_amd import engine as E, tpe
    s = study
    asked = []
    real = E.Engine.mo_keys
    monkeypatch.setattr(E.Engine, 'mo_keys', lambda self, F, **k: asked.append(len(F)) or real(self, F, **k))
    want = tpe.suggest([400], s['domain'], s['keyed'], 11)
    monkeypatch.setattr(tpe, 'MO_DEVICE_MIN_TRIALS', 302)
    assert tpe.suggest([400], s['domain'], s['trials'], 11, objectives=('loss', 'cost')) == want and not asked
    monkeypatch.setattr(tpe, 'MO_DEVICE_MIN_TRIALS', 301)
    assert tpe.suggest([400], s['domain'], s['trials'], 11, objectives=('loss', 'cost')) == want
    assert asked == [301]                          # once per call, the complete trials (the NaN one too)
    tpe.suggest([400, 401, 402], s['domain'], s['trials'], 11, objectives=('loss', 'cost'), batch='pending')
    assert asked == [301, 301]


@pytest.mark.parametrize('kw', [dict(posterior_builder='host'), dict(posterior_builder='device'),
                                dict(posterior_builder='device', multivariate=True)])
def test_one_objective_is_the_plain_call(kw):
    from hyperopt_amd import tpe
    from hyperopt_amd.base import Domain
    loss = np.random.RandomState(12).permutation(300) / 7.0          # distinct
    trials = R.make_trials(space(), loss[:, None], names=('loss',), n_pending=1)
    domain = Domain(lambda cfg: 0.0, space())
    got = tpe.suggest([400, 401], domain, trials, 3, batch=True, objectives=('loss',), **kw)
    assert len(got) == 2 and got == tpe.suggest([400, 401], domain, trials, 3, batch=True, **kw)


def test_a_short_fmin():
    from hyperopt_amd import STATUS_OK, Trials, fmin, hp, tpe
    sp = {'x': hp.uniform('x', 0, 1), 'y': hp.uniform('y', 0, 1)}

    def fn(cfg):
        return {'loss': cfg['x'] ** 2 + cfg['y'], 'cost': (cfg['x'] - 1) ** 2 + cfg['y'], 'status': STATUS_OK}
    trials = Trials()
    # (posterior_builder='device': the keys from the kernel at every size, not from the threshold on)
    fmin(fn, sp, algo=partial(tpe.suggest, objectives=('loss', 'cost'), n_startup_jobs=10,
                              posterior_builder='device'), max_evals=40, trials=trials,
         rstate=np.random.RandomState(2))
    assert len(trials.trials) == 40
    F = np.array([(d['result']['loss'], d['result']['cost']) for d in trials.trials])
    front = tpe.pareto_front(trials, ('loss', 'cost'))
    assert [d['tid'] for d in front] == [trials.trials[i]['tid'] for i in R.front(F)] and front
