"""The sampled hypervolume tie-break on the device: Engine.mo_keys(...,
tiebreak='hypervolume_mc') (tpe_mo_keys_hvs, hyperopt_amd/csrc/tpe_mo_hvs.hip)
against the plain statement of the rule (tests/mo_hvs_reference.py), exactly --
keys, counts, picks and gains are integers -- and tpe.suggest(...,
mo_tiebreak='hypervolume_mc') with four objectives under both builders."""
import ctypes

import numpy as np
import pytest

from tests import mo_hvs_reference as V
from tests import mo_reference as R
from tests.test_mo_gpu import space

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


@pytest.mark.parametrize('name', V.CASES)
def test_keys_counts_picks_and_gains_are_the_reference(eng, name):
    F, G, k, S = V.case(name)
    want = V.expected(name)
    assert want['straddles'] == (name not in V.STAY)       # (no case silently tests the unchanged path)
    assert name not in V.SIZED or want['level'] == V.SIZED[name][5]
    got = eng.mo_keys(F, G=G, want_counts=True, tiebreak='hypervolume_mc', n_select=k, n_samples=S, want_picks=True)
    keys, by, do, picked, gains = got[:3] + got[-2:]
    assert picked.dtype == np.int32 and gains.dtype == np.uint64
    assert np.array_equal(by, want['by']) and np.array_equal(do, want['do'])
    assert picked.tolist() == want['picked'] and gains.tolist() == want['gains']
    assert np.array_equal(keys, want['keys'], equal_nan=True)
    assert sorted(keys[by >= 0].tolist()) == list(range(int((by >= 0).sum())))
    if name in V.STAY:
        assert not len(picked) and np.array_equal(keys, eng.mo_keys(F, G=G), equal_nan=True)
    else:
        assert all(a >= b for a, b in zip(gains[:-1], gains[1:])) and int(gains[0]) == want['box']
    # a second call, on buffers that are no longer fresh: equal arrays
    again = eng.mo_keys(F, G=G, tiebreak='hypervolume_mc', n_select=k, n_samples=S, want_picks=True)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(again, (keys, picked, gains)))


def test_abi_errors_leave_the_outputs_alone(eng):
    from hyperopt_amd import _lib as L
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    keys, by, do = np.full(10, 7.0), np.full(10, 7, dtype=np.int32), np.full(10, 7, dtype=np.int32)
    picked, gains, n_picked = np.full(64, 7, dtype=np.int32), np.full(64, 7, dtype=np.uint64), ctypes.c_int32(7)
    for M, k, S in ((1, 3, 64), (9, 3, 64), (4, 3, 0), (4, 3, 63), (4, 3, (1 << 20) + 64), (4, 65, 64), (4, -1, 64)):
        F = np.random.RandomState(8).uniform(size=(10, M))
        assert eng.lib.tpe_mo_keys_hvs(eng.h, p(F), 10, M, None, 0, k, S, p(keys), p(by), p(do), None, p(picked),
                                       p(gains), ctypes.byref(n_picked)) == L.TPE_ERR_ARG
        assert b'tpe_mo_keys_hvs' in eng.lib.tpe_last_error(eng.h)
    assert (keys == 7.0).all() and (by == 7).all() and (do == 7).all()
    assert (picked == 7).all() and (gains == 7).all() and n_picked.value == 7


@pytest.mark.parametrize('builder', ('host', 'device'))
def test_suggest_with_four_objectives(builder):
    """The call is the plain call on the reference's keys under either builder,
    and its documents are not the 'dominates' call's."""
    from hyperopt_amd import tpe
    from hyperopt_amd.base import Domain
    rows = np.random.RandomState(0).uniform(size=(300, 4))
    trials = R.make_trials(space(), rows, n_pending=2, names=('loss', 'cost', 'mem', 'lat'))
    want = V.select(rows, 5, 128)
    assert want['straddles'] and set(want['picked']) != set(np.argsort(R.keys(rows))[:5].tolist())
    domain, kw = Domain(lambda cfg: 0.0, space()), dict(posterior_builder=builder)
    ids = [400, 401, 402]
    got = tpe.suggest(ids, domain, trials, 11, objectives=('loss', 'cost', 'mem', 'lat'),
                      mo_tiebreak='hypervolume_mc', mo_samples=128, **kw)
    assert got == tpe.suggest(ids, domain, R.with_loss(trials, want['keys']), 11, **kw)
    assert got != tpe.suggest(ids, domain, trials, 11, objectives=('loss', 'cost', 'mem', 'lat'), **kw)
