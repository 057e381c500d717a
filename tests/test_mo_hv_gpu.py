"""The hypervolume tie-break on the device: Engine.mo_keys(...,
tiebreak='hypervolume') (tpe_mo_keys_hv, hyperopt_amd/csrc/tpe_mo_hv.hip)
against the plain statement of the rule (tests/mo_hv_reference.py), exactly --
keys, counts, picks and gains are integers -- and tpe.suggest(...,
mo_tiebreak='hypervolume') against its definition: the plain call on a copy of
the trials whose 'loss' is the reference key."""
import ctypes

import numpy as np
import pytest

from tests import mo_hv_reference as H
from tests import mo_reference as R
from tests.test_mo_gpu import VARIANTS, space

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


def hv(eng, F, G, k):
    return eng.mo_keys(F, G=G, want_counts=True, tiebreak='hypervolume', n_select=k, want_picks=True)


@pytest.mark.parametrize('name,M', H.CASES)
def test_keys_counts_picks_and_gains_are_the_reference(eng, name, M):
    F, G, k = H.case(name, M)
    want = H.expected(name, M)
    assert want['straddles'] == (name not in H.STAY)       # (no case silently tests the unchanged path)
    got = hv(eng, F, G, k)
    keys, by, do, picked, gains = got[:3] + got[-2:]
    assert picked.dtype == np.int32 and gains.dtype == np.uint64
    assert np.array_equal(by, want['by']) and np.array_equal(do, want['do'])
    assert picked.tolist() == want['picked'].tolist() and gains.tolist() == want['gains']
    assert np.array_equal(keys, want['keys'], equal_nan=True)
    if name in H.STAY:
        assert not len(picked) and np.array_equal(keys, eng.mo_keys(F, G=G), equal_nan=True)


def test_two_calls_give_equal_arrays(eng):
    F, G, k = H.case('quantized', 2)
    assert all(np.array_equal(x, y) for x, y in zip(hv(eng, F, G, k), hv(eng, F, G, k)))


@pytest.mark.parametrize('n', (127, 128, 300))
def test_the_builders_give_the_same_integers(eng, n):
    from hyperopt_amd import posterior as P
    for M in (2, 3):
        F = np.random.RandomState(n + M).randint(0, 40, (n, M)).astype(float)
        k = P.n_below_of(n, 0.25)
        by, do = P.mo_counts(F)
        want = P.mo_hypervolume_order(F, by, do, P.mo_keys(F), k)
        got = hv(eng, F, None, k)
        assert all(np.array_equal(x, y) for x, y in zip((got[0],) + got[3:], want))
        assert np.array_equal(eng.mo_keys(F, tiebreak='hypervolume', n_select=k), want[0])


def test_abi_errors_leave_the_outputs_alone(eng):
    from hyperopt_amd import _lib as L
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    keys, by, do = np.full(10, 7.0), np.full(10, 7, dtype=np.int32), np.full(10, 7, dtype=np.int32)
    picked, gains, n_picked = np.full(64, 7, dtype=np.int32), np.full(64, 7, dtype=np.uint64), ctypes.c_int32(7)
    for M, k in ((1, 3), (4, 3), (2, 65), (2, -1)):
        F = np.random.RandomState(8).uniform(size=(10, M))
        assert eng.lib.tpe_mo_keys_hv(eng.h, p(F), 10, M, None, 0, k, p(keys), p(by), p(do), None, p(picked),
                                      p(gains), ctypes.byref(n_picked)) == L.TPE_ERR_ARG
        assert b'tpe_mo_keys_hv' in eng.lib.tpe_last_error(eng.h)
    assert (keys == 7.0).all() and (by == 7).all() and (do == 7).all()
    assert (picked == 7).all() and (gains == 7).all() and n_picked.value == 7
    # the picks past n_picked: -1 and 0
    F = H.case('second-level', 2)[0]
    keys = np.empty(len(F))
    assert eng.lib.tpe_mo_keys_hv(eng.h, p(F), len(F), 2, None, 0, 6, p(keys), None, None, None, p(picked),
                                  p(gains), ctypes.byref(n_picked)) == L.TPE_OK
    assert n_picked.value == 3 and picked[3:6].tolist() == [-1] * 3 and gains[3:6].tolist() == [0] * 3
    assert (picked[6:] == 7).all()


def test_its_buffers_are_counted_and_left_alone_by_the_default_call():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    F = np.random.RandomState(9).uniform(size=(3000, 3))
    e.mo_keys(F)
    held = e.device_bytes()
    e.mo_keys(F, tiebreak='hypervolume', n_select=8)
    more = e.device_bytes()
    assert more - held >= 3000 * (3 * 8 + 3 * 4 + 2 * 4 + 3 * 4 + 1) + 4 * 4 + 64 * 12
    e.mo_keys(F)
    e.mo_keys(F, tiebreak='hypervolume', n_select=8)
    assert e.device_bytes() == more
    e.close()


@pytest.fixture(scope='module')
def study():
    """tests/test_mo_gpu.py's study (300 finished trials, one with a NaN cost,
    two pending) and its copies whose 'loss' is either tie-break's reference key."""
    from hyperopt_amd.base import Domain
    F = np.random.RandomState(0).uniform(size=(300, 2))
    rows = np.vstack([F, [(0.5, np.nan)]])
    trials = R.make_trials(space(), rows, n_pending=2)
    want = H.select(rows, 5)
    assert want['straddles'] and len(want['picked']) == 5 and np.isnan(want['keys'][300])
    below = set(np.argsort(want['keys'][:300])[:5].tolist())
    assert below == set(want['picked'].tolist())           # the below set is the pick set
    assert below != set(np.argsort(R.keys(F))[:5].tolist())
    return dict(trials=trials, keyed=R.with_loss(trials, want['keys']), plain=R.with_loss(trials, R.keys(rows)),
                domain=Domain(lambda cfg: 0.0, space()))


@pytest.mark.parametrize('builder', ('host', 'device'))
@pytest.mark.parametrize('variant', ('plain', 'scott', 'fixed', 'pending'))
def test_the_call_is_the_plain_call_on_the_keys(study, variant, builder):
    from hyperopt_amd import tpe
    s = study
    kw = dict(VARIANTS[variant], posterior_builder=builder)
    ids = [400, 401, 402]
    got = tpe.suggest(ids, s['domain'], s['trials'], 11, objectives=('loss', 'cost'), mo_tiebreak='hypervolume', **kw)
    assert got == tpe.suggest(ids, s['domain'], s['keyed'], 11, **kw)
    # without the keyword: the parent's documents, and other ones
    old = tpe.suggest(ids, s['domain'], s['trials'], 11, objectives=('loss', 'cost'), **kw)
    assert old == tpe.suggest(ids, s['domain'], s['plain'], 11, **kw)
    if variant == 'plain':
        assert got != old
