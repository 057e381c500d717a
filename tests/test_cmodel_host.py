"""The host side of tpe.suggest(constraint_model='density'): the keyword's
errors, posterior.cmodel_split and posterior.cmodel_acquisition."""
import numpy as np
import pytest

from hyperopt_amd import posterior as P


def test_keyword_errors_before_any_engine():
    from hyperopt_amd import Domain, hp, tpe
    from hyperopt_amd.base import Trials
    domain = Domain(None, {'x': hp.uniform('x', 0, 1)})
    pool = tpe.Pool({'x': hp.uniform('x', 0, 1)}, [{'x': 0.5}])
    for kw in (dict(constraint_model='soft', constraints=('c',)),
               dict(constraint_model='density'),
               dict(constraint_model='density', constraints=('c',), multivariate=True),
               dict(constraint_model='density', constraints=('c',), pool=pool),
               dict(constraint_model='density', constraints=('c',), devices=[0, 1])):
        with pytest.raises(ValueError, match='constraint_model'):
            tpe.suggest([0], domain, Trials(), 1, **kw)


def test_split():
    nan = float('nan')
    G = np.array([[-1.0, 2.0, -1.0], [0.0, 1.0, -2.0], [3.0, 1.0, 0.0], [nan, 0.5, -1.0], [2.0, 3.0, -0.0]])
    live, out = P.cmodel_split(G, 0.25)
    assert live.tolist() == [True, True, True, False, True]          # the NaN row is not live
    assert out[0][0].tolist() == [True, True, False, False, False] and out[0][1] == 2 / 4
    # none satisfied: n_below_of(4, 0.25) = 1 smallest, the tie at 1.0 by trial order
    assert P.n_below_of(4, 0.25) == 1
    assert out[1][0].tolist() == [False, True, False, False, False] and out[1][1] == 1 / 4
    assert out[2] == (None, 1.0)                                     # all satisfied: skipped
    live, out = P.cmodel_split(G[:, :1], 0.25, F=np.array([[0.0], [nan], [0.0], [0.0], [0.0]]))
    assert live.tolist() == [True, False, True, False, True] and out[0][1] == 1 / 3
    # a larger fallback set keeps trial order among equal violations
    live, out = P.cmodel_split(np.full((100, 1), 1.0), 0.25)
    assert P.n_below_of(100, 0.25) == 3 and np.flatnonzero(out[0][0]).tolist() == [0, 1, 2]


TS = (-800.0, -1.0, 0.0, 1.0, 800.0)
GAMMAS = (1e-3, 0.5, 1 - 1e-3)


def exact_f(g, t):
    try:
        import mpmath
    except ImportError:
        g, t = np.longdouble(g), np.longdouble(t)
        return float(-np.log(g + (1 - g) * np.exp(t)) if t <= 0 else -(t + np.log((1 - g) + g * np.exp(-t))))
    mpmath.mp.dps = 60
    g, t = mpmath.mpf(g), mpmath.mpf(t)
    return float(-mpmath.log(g + (1 - g) * mpmath.exp(t)))


@pytest.mark.parametrize('g', GAMMAS)
def test_acquisition_against_the_exact_formula(g):
    t = np.array(TS)
    a = P.cmodel_acquisition(np.zeros((1, len(t))), t[None], [g])
    assert np.all(np.isfinite(a))
    want = np.array([exact_f(g, x) for x in TS])
    # the logarithm's argument carries a few roundings of 2^-53 relative, which the
    # logarithm turns into as much absolute error; then a few ulp of the result
    assert np.all(np.abs(a - want) <= 4 * 2.0 ** -52 + 4 * np.spacing(np.abs(want))), (a, want)
    # both branches at t = 0
    neg = -np.log(g + (1.0 - g) * np.exp(0.0))
    pos = -(0.0 + np.log((1.0 - g) + g * np.exp(-0.0)))
    assert abs(neg - pos) <= 2 ** -52 and abs(a[2]) <= 2 ** -52
    # models add up in order; a NaN term makes a NaN; infinities as the rule says
    two = P.cmodel_acquisition(np.zeros((2, len(t))), np.stack([t, t[::-1]]), [g, 0.25])
    assert np.array_equal(two, a + P.cmodel_acquisition(np.zeros((1, len(t))), t[::-1][None], [0.25]))
    edge = P.cmodel_acquisition([[-np.inf, 0.0, -np.inf, np.nan]], [[0.0, -np.inf, -np.inf, 0.0]], [g])
    assert edge[0] == -np.inf and edge[1] == -np.log(g) and np.isnan(edge[2]) and np.isnan(edge[3])
