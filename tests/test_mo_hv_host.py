"""The hypervolume tie-break, host side: posterior.mo_keys(...,
tiebreak='hypervolume') against the plain statement of the rule
(tests/mo_hv_reference.py), exactly, and the keyword's errors."""
import numpy as np
import pytest

from tests import mo_hv_reference as H
from tests import mo_reference as R


@pytest.mark.parametrize('name,M', H.CASES)
def test_keys_and_picks_are_the_reference(name, M):
    from hyperopt_amd import posterior as P
    F, G, k = H.case(name, M)
    want = H.expected(name, M)
    assert want['straddles'] == (name not in H.STAY)       # (no case silently tests the unchanged path)
    old = P.mo_keys(F, G=G)
    assert np.array_equal(P.mo_keys(F, G=G, tiebreak='hypervolume', n_select=k), want['keys'], equal_nan=True)
    by, do = P.mo_counts(F, G)
    keys, picked, gains = P.mo_hypervolume_order(F, by, do, old, k, G)
    assert picked.tolist() == want['picked'].tolist() and gains.tolist() == want['gains']
    if name in H.STAY:
        assert np.array_equal(keys, old, equal_nan=True) and not len(picked)
    assert sorted(keys[by >= 0].tolist()) == list(range(int((by >= 0).sum())))


def test_the_default_keys_and_the_errors():
    from hyperopt_amd import posterior as P, tpe
    F = H.case('uniform-300-5', 2)[0]
    assert np.array_equal(P.mo_keys(F, tiebreak='dominates', n_select=5), R.keys(F))
    assert not np.array_equal(P.mo_keys(F, tiebreak='hypervolume', n_select=5), R.keys(F))
    for bad in (dict(tiebreak='hv'), dict(tiebreak='hypervolume', n_select=65),
                dict(tiebreak='hypervolume', n_select=-1)):
        with pytest.raises(ValueError):
            P.mo_keys(F, **bad)
    for M in (1, 4):
        with pytest.raises(ValueError):
            P.mo_keys(np.zeros((5, M)), tiebreak='hypervolume', n_select=2)
    # tpe.suggest: before the domain, the trials or an engine are touched
    for bad in (dict(mo_tiebreak='hv'), dict(mo_tiebreak='hypervolume'),
                dict(mo_tiebreak='hypervolume', objectives=('loss',)),
                dict(mo_tiebreak='hypervolume', objectives=('a', 'b', 'c', 'd')),
                dict(mo_tiebreak='hypervolume', objectives=('loss', 'cost'), constraints=('c',),
                     constraint_model='density')):
        with pytest.raises(ValueError, match='mo_tiebreak'):
            tpe.suggest([0], None, None, 0, **bad)
