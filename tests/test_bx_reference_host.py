"""The exact reference of the expansion index's tests (tests/bx_reference.py)
checked without a GPU, and the input conditions the GPU tests
(tests/test_bx_index_gpu.py) rely on checked with the reference alone, so
that those tests are not vacuous."""
import numpy as np
import pytest
from mpmath import mp, mpf

from oracle import tpe_oracle as O
from tests import bx_cases as C
from tests.bx_reference import LabelRef, MP_DPS

ALL = list(C.CASES)


def _refs(name):
    ps = C.posts(name)
    return [(li, ps[li], LabelRef(ps[li])) for li in C.dense_labels(ps)]


def _grid(p, n):
    """n value-space points over the label's candidate range (evenly spaced
    in draw space)."""
    sh = C.index_shape(p)
    d = np.linspace(sh['lo'], sh['hi'], n)
    return np.exp(d) if p.family == 'LGMM1' else d


@pytest.mark.parametrize('name', ALL)
def test_score_exact_matches_the_oracle(name):
    """score_exact against the oracle's fp64 lpdf_below - lpdf_above, to
    1e-12 (1 + |score|): a grid over the range and every component mean
    (a coarser grid where the above mixture has 16k components)."""
    worst = 0.0
    for li, p, ref in _refs(name):
        big = len(p.above[0]) > 4096
        x = _grid(p, 129 if big else 1025)
        if not big:
            mus = np.concatenate([p.below[1], p.above[1]])
            x = np.concatenate([x, np.exp(mus) if p.family == 'LGMM1' else mus])
        f = O.gmm1_lpdf if p.family == 'GMM1' else O.lgmm1_lpdf
        with np.errstate(invalid='ignore', divide='ignore'):
            s64 = f(x, *p.below, low=p.low, high=p.high) - f(x, *p.above, low=p.low, high=p.high)
        s = ref.score_exact(x)
        fin = np.isfinite(s64) & np.isfinite(s)
        assert fin.mean() > 0.9
        d = np.abs(s64[fin] - s[fin].astype(np.float64)) / (1.0 + np.abs(s64[fin]))
        worst = max(worst, float(d.max()))
        assert d.max() <= 1e-12, (name, li, float(d.max()))
    print('%s: worst |score_exact - oracle| / (1 + |score|) = %.3g' % (name, worst))


@pytest.mark.parametrize('name', ALL)
def test_score_exact_matches_mpmath(name):
    """score_exact against a 40-digit mpmath evaluation of the same
    definition at 64 points per dense label: 1e-17 relative."""
    worst = 0.0
    for li, p, ref in _refs(name):
        x = _grid(p, 66)[1:-1]
        s = ref.score_exact(x)
        with mp.workdps(MP_DPS):
            for xi, si in zip(x, s):
                if not np.isfinite(si):
                    continue
                sm = ref.score_mp(float(xi))
                # (long double -> mpf exactly: high and low halves)
                hi = float(si)
                got = mpf(hi) + mpf(float(si - np.longdouble(hi)))
                rel = float(abs(got - sm) / (1 + abs(sm)))
                worst = max(worst, rel)
                assert rel <= 1e-17, (name, li, float(xi), rel)
    print('%s: worst |score_exact - mpmath| / (1 + |score|) = %.3g' % (name, worst))


@pytest.mark.parametrize('name', ALL)
def test_interval_mass_sums_to_one(name):
    for li, p, ref in _refs(name):
        if p.low is None:
            continue
        assert abs(ref.interval_mass(p.low, p.high) - 1.0) <= 1e-15
        m = ref.interval_masses(np.linspace(p.low, p.high, 18))
        assert np.all(m >= 0.0) and abs(m.sum() - 1.0) <= 1e-14
        # beyond the bounds there is nothing
        w = p.high - p.low
        assert ref.interval_mass(p.low - w, p.low) == 0.0 and ref.interval_mass(p.high, p.high + w) == 0.0


def test_interval_mass_closed_form():
    """One standard normal, unbounded and cut to [-1, 2]."""
    from hyperopt_amd import posterior as P
    one = (np.array([1.0]), np.array([0.0]), np.array([1.0]))
    free = LabelRef(P.LabelPosterior('n', 'GMM1', one, one))
    assert abs(free.interval_mass(-1.0, 1.0) - 0.6826894921370859) <= 1e-15
    cut = LabelRef(P.LabelPosterior('n', 'GMM1', one, one, low=-1.0, high=2.0))
    whole = 0.9772498680518208 - 0.15865525393145707
    assert abs(cut.interval_mass(-1.0, 1.0) - 0.6826894921370859 / whole) <= 1e-15
    lg = LabelRef(P.LabelPosterior('n', 'LGMM1', one, one))     # draw space: log x
    assert abs(lg.interval_mass(-1.0, 1.0) - 0.6826894921370859) <= 1e-15


@pytest.mark.parametrize('name', ALL)
def test_case_reaches_its_branch(name):
    """The conditions the GPU tests rely on, and each case's branch of
    bx_build, from the reference and bx_build's host arithmetic alone."""
    ps = C.posts(name)
    eligible = C.CASES[name][1]
    shapes = {}
    for li, p, ref in _refs(name):
        sh = shapes[p.label] = C.index_shape(p)
        if not eligible:
            continue
        # at least 95 % of the grid has both exact lpdfs above -300
        x = _grid(p, 4097)
        ok = (ref.lpdf_exact(x, 0) > -300) & (ref.lpdf_exact(x, 1) > -300)
        assert ok.mean() >= 0.95, (name, li, ok.mean())
        # the narrowest below sigma is at least 100 sub-bins wide (the
        # premise of the mass's midpoint rule)
        wb, _, sb = p.below
        assert np.min(np.asarray(sb)[np.asarray(wb) > 0]) >= 100.0 * sh['sub_width'], (name, li)
        assert sh['eligible'], (name, li, sh)
    one = shapes.get(name)
    if name == 'uniform300':
        assert one['n_cl'] + one['n_nc'] == 296 and one['n_cl'] > 250 and one['n_nc'] >= 8 and one['nbins'] == 960
    elif name == 'uniform3':
        assert one['n_cl'] == 1 and one['want'] < C.K_MIN_BINS and one['nbins'] == C.K_MIN_BINS
    elif name == 'normal30':
        assert ps[0].low is None and one['n_cl'] == 1 and 3000 < one['nbins'] < 5000
    elif name == 'lognormal150':
        assert ps[0].family == 'LGMM1' and ps[0].low is None
        assert one['n_cl'] + one['n_nc'] == 147 and one['n_cl'] >= 2 and one['n_nc'] >= 100
        assert 12000 < one['nbins'] < 18000
    elif name == 'loguniform_far':
        assert ps[0].family == 'LGMM1' and ps[0].high == -10.0
    elif name == 'offset1e6':
        assert one['lo'] == 1e6 and one['nbins'] == 960
    elif name == 'ties50':
        assert np.sum(np.diff(ps[0].above[1]) == 0.0) >= 49
    elif name == 'at_bounds':
        assert np.sum(ps[0].above[1] == 0.0) == 10 and np.sum(ps[0].above[1] == 1.0) == 10
    elif name == 'all_clipped':
        assert one['n_nc'] == 0 and one['n_cl'] == 200
    elif name == 'zero_weight':
        assert np.sum(ps[0].above[0] == 0.0) == 3 and np.sum(ps[0].below[0] == 0.0) == 1
        assert np.all(np.diff(ps[0].above[1]) >= 0.0)
    elif name == 'zero_above':
        assert np.sum(ps[0].above[0] == 0.0) == 3 and np.all(np.asarray(ps[0].below[0]) > 0.0)
        assert np.all(np.diff(ps[0].above[1]) >= 0.0)
        # the zeroed records include a clipped and an unclipped one
        z = np.asarray(ps[0].above[2])[np.asarray(ps[0].above[0]) == 0.0]
        assert np.any(z == one['sigma']) and np.any(z != one['sigma'])
    elif name.startswith('below'):
        n = int(name[5:])
        assert len(ps[0].below[0]) == n and (n > C.K_STAGE_BELOW) == (name != 'below64')
    elif name == 'max_bins':
        assert 65000 < one['want'] <= 0.995 * C.K_MAX_BINS and 65000 < one['nbins'] <= C.K_MAX_BINS
    elif name == 'over_bins':
        assert one['want'] >= 1.005 * C.K_MAX_BINS and not one['eligible']
        assert one['n_nc'] <= C.K_MAX_UNCLIPPED
    elif name == 'over_unclipped':
        assert one['n_nc'] == C.K_MAX_UNCLIPPED + 1 and one['n_cl'] == 1 and one['want'] <= C.K_MAX_BINS
        assert not one['eligible']
    elif name == 'three_labels':
        assert [p.family for p in ps] == ['GMM1', 'GMM1', 'LGMM1', 'categorical', 'GMM1']
        assert ps[1].q is not None
        assert len({(s['nbins'], s['n_nc']) for s in shapes.values()}) == 3
    elif name == 'permuted':
        # the same mixture as a function, out of mu order
        base = C.posts('uniform300')[0]
        assert np.any(np.diff(ps[0].above[1]) < 0.0)
        for a, b in zip(ps[0].above, base.above):
            assert np.array_equal(np.sort(a), np.sort(b))
        x = _grid(base, 257)
        sa, sb = LabelRef(ps[0]).score_exact(x), LabelRef(base).score_exact(x)
        assert np.max(np.abs(sa - sb)) <= 1e-15   # (p_accept: one fp64 sum in another order)
        assert one['eligible']       # (by bx_build's shape alone: only the order rules it out)
