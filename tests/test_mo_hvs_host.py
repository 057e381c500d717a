"""The sampled hypervolume tie-break, host side: posterior.mo_keys(...,
tiebreak='hypervolume_mc') and mo_hypervolume_mc_order against the plain
statement of the rule (tests/mo_hvs_reference.py), exactly; the keyword's
errors; and the estimate against the exact box share."""
import numpy as np
import pytest

from tests import mo_hv_reference as H
from tests import mo_hvs_reference as V
from tests import mo_reference as R


@pytest.mark.parametrize('name', V.CASES)
def test_keys_picks_and_gains_are_the_reference(name):
    from hyperopt_amd import posterior as P
    F, G, k, S = V.case(name)
    want = V.expected(name)
    assert want['straddles'] == (name not in V.STAY)       # (no case silently tests the unchanged path)
    assert name not in V.SIZED or want['level'] == V.SIZED[name][5]
    old = P.mo_keys(F, G=G)
    assert np.array_equal(P.mo_keys(F, G=G, tiebreak='hypervolume_mc', n_select=k, n_samples=S), want['keys'],
                          equal_nan=True)
    by, do = P.mo_counts(F, G)
    keys, picked, gains = P.mo_hypervolume_mc_order(F, by, do, old, k, S, G)
    assert picked.tolist() == want['picked'] and gains.tolist() == want['gains']
    assert picked.dtype == np.int32 and gains.dtype == np.uint64
    if name in V.STAY:
        assert np.array_equal(keys, old, equal_nan=True) and not len(picked)
    assert sorted(keys[by >= 0].tolist()) == list(range(int((by >= 0).sum())))


def test_the_other_values_are_unchanged_and_the_errors():
    from hyperopt_amd import posterior as P, tpe
    F = V.case('one-block')[0]
    assert np.array_equal(P.mo_keys(F, tiebreak='dominates', n_select=5), R.keys(F))
    assert not np.array_equal(P.mo_keys(F, tiebreak='hypervolume_mc', n_select=5, n_samples=64), R.keys(F))
    F2 = H.case('uniform-300-5', 2)[0]
    assert np.array_equal(P.mo_keys(F2, tiebreak='hypervolume', n_select=5), H.expected('uniform-300-5', 2)['keys'])
    for bad in (dict(n_select=65), dict(n_select=-1), dict(n_samples=0), dict(n_samples=63),
                dict(n_samples=(1 << 20) + 64)):
        with pytest.raises(ValueError):
            P.mo_keys(F, tiebreak='hypervolume_mc', **dict(dict(n_select=5, n_samples=64), **bad))
    for M in (1, 9):
        with pytest.raises(ValueError):
            P.mo_keys(np.zeros((5, M)), tiebreak='hypervolume_mc', n_select=2)
    # tpe.suggest: before the domain, the trials or an engine are touched
    four = ('a', 'b', 'c', 'd')
    for bad in (dict(mo_tiebreak='hypervolume_mc'), dict(mo_tiebreak='hypervolume_mc', objectives=('loss',)),
                dict(mo_tiebreak='hypervolume_mc', objectives=four, constraints=('g',), constraint_model='density'),
                dict(mo_tiebreak='hypervolume_mc', objectives=four, mo_samples=100),
                dict(mo_tiebreak='hypervolume_mc', objectives=four, mo_samples=(1 << 20) + 64),
                dict(mo_tiebreak='hypervolume', objectives=four[:2], mo_samples=128),
                dict(objectives=four, mo_samples=128), dict(mo_samples=128)):
        with pytest.raises(ValueError, match='mo_tiebreak'):
            tpe.suggest([0], None, None, 0, **bad)


@pytest.mark.parametrize('name,M', [('uniform-300-5', 2), ('uniform-65-5', 3), ('uniform-300-25', 3), ('constrained', 3)])
def test_the_first_gain_estimates_the_box_share(name, M):
    """gain / S against p = vol(c) / prod(span), vol(c) the exact tie-break's
    integer for the same first pick: gain is a sum of S draws that fall into the
    box with probability p each (up to the floor of the coordinate rule), so
    within 5 sqrt(p (1 - p) / S) -- five binomial standard deviations.  The
    inputs are fixed: a deterministic pass, of the reference and of the builder."""
    from hyperopt_amd import posterior as P
    F, G, k = H.case(name, M)
    S = 65536 if M == 2 else 4096
    exact, want = H.expected(name, M), V.select(F, k, S, G)
    assert want['picked'][0] == exact['picked'][0]          # the same row: exact['gains'][0] is its box
    by, do = P.mo_counts(F, G)
    got = P.mo_hypervolume_mc_order(F, by, do, P.mo_keys(F, G=G), k, S, G)
    ok = ~np.isnan(F).any(axis=1) if G is None else P.mo_violation(G, F) == 0.0
    level = np.flatnonzero(by == by[want['picked'][0]])
    span = int(ok.sum()) - H.ranks(F, ok)[level].min(axis=0)
    p = exact['gains'][0] / float(np.prod(span))
    bound = 5 * np.sqrt(p * (1 - p) / S)
    for gain in (want['gains'][0], int(got[2][0])):
        print(name, M, gain / S, p, bound)
        assert abs(gain / S - p) <= bound
