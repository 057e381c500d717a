"""Quantized hyperparameters in joint TPE groups, host side (CPU): the mass
function of the numpy definition (tests/joint_quant_reference.py) against
mpmath, posterior.joint_mixture(quantized=True) against the univariate
posteriors, the widened joint_group / joint_groups, and -- through the fp64
draw port -- the conditions test_joint_quant_gpu.py rests on: the committed
draw seeds exclude nothing, every committed round's best configuration leads
every other by a clear margin, and the fine group's products of factors
underflow fp64 while its lpdf is finite."""
import inspect
import math

import numpy as np
import pytest

from hyperopt_amd import hp, posterior as P, tpe
from hyperopt_amd.base import Domain, Trials
from tests import joint_quant_cases as QC
from tests import joint_quant_reference as QR
from tests import joint_group_cases as GC

SQRT2 = math.sqrt(2.0)


# -- the mass function ------------------------------------------------------------
def _intervals():
    """(zl, zu, regime) in z = x / sqrt 2 units: centres c and widths w in
    sigmas; w from 1e-7 (the fine grid against the widest sigma) to 4 (a
    coarse grid against a narrow component)."""
    out = []
    for w in (1e-7, 1e-5, 1e-3, 0.07, 1.0, 4.0):
        for c in (0.0, 0.25 * w, -0.49 * w, 0.49 * w):
            out.append((c - 0.5 * w, c + 0.5 * w, 'straddling'))
        for c in (0.5 * w, 0.5 * w + 0.01, 0.5 * w + 0.5, 1.0):
            if c - 0.5 * w >= 0.0 and c - 0.5 * w <= 1.0:
                out.append((c - 0.5 * w, c + 0.5 * w, 'within 1 sigma'))
                out.append((-c - 0.5 * w, -c + 0.5 * w, 'within 1 sigma'))
        for c in (2.0, 5.0, 8.0, 12.0, 20.0, 30.0):
            out.append((c, c + w, 'tail'))
            out.append((-c - w, -c, 'tail'))
    return [(a / SQRT2, b / SQRT2, r) for a, b, r in out]


def test_mass_function_against_mpmath():
    """zmass at exact ends against 50-digit arithmetic, in the three regimes,
    for coarse and fine q / s: within mass_tolerance -- a few ulp of the larger
    tail on one side of the mean, a few ulp of the mass when straddling."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    worst = {}
    for zl, zu, regime in _intervals():
        got = float(QR.zmass(zl, zu))
        a, b = mp.mpf(zl), mp.mpf(zu)
        if zl >= 0.0:
            exact = (mp.erfc(a) - mp.erfc(b)) / 2
        elif zu <= 0.0:
            exact = (mp.erfc(-b) - mp.erfc(-a)) / 2
        else:
            exact = (mp.erf(b) - mp.erf(a)) / 2
        assert exact > 0
        tol = QR.mass_tolerance(zl, zu, float(exact))
        err = abs(float(mp.mpf(got) - exact))
        worst[regime] = max(worst.get(regime, 0.0), err / tol)
        assert err <= tol, (regime, zl, zu, got, float(exact), err / tol)
        assert got > 0.0
    print('zmass worst err / tolerance per regime:', worst)
    assert set(worst) == {'straddling', 'within 1 sigma', 'tail'}
    # empty and reversed intervals, NaN
    assert QR.zmass(0.3, 0.3) == 0.0 and QR.zmass(0.4, 0.3) == 0.0 and QR.zmass(np.nan, 0.3) == 0.0


def test_interval_is_the_reference_one():
    lin = QR.QDim(False, 0.0, 6.0, 0, q=2.0)
    ub, lb = QR.interval(lin, np.array([0.0, 2.0, 6.0, 8.0]))
    assert ub.tolist() == [1.0, 3.0, 6.0, 6.0] and lb.tolist() == [0.0, 1.0, 5.0, 7.0]
    free = QR.QDim(False, None, None, 0, q=2.0)
    assert [v.tolist() for v in QR.interval(free, np.array([8.0]))] == [[9.0], [7.0]]
    log = QR.QDim(True, math.log(0.2), math.log(2.4), 0, q=1.0)
    ub, lb = QR.interval(log, np.array([0.0, 1.0, 2.0, -2.0]))
    assert np.allclose(ub[:3], np.log([0.5, 1.5, 2.4]), rtol=1e-15)
    assert np.allclose(lb[:3], np.log([0.2, 0.5, 1.5]), rtol=1e-15)
    assert not ub[3] > lb[3]                      # a negative value: empty
    lfree = QR.QDim(True, None, None, 0, q=1.0)
    ub, lb = QR.interval(lfree, np.array([0.0]))
    assert ub[0] == math.log(0.5) and lb[0] == math.log(QR.EPS)


# -- joint_mixture(quantized=True) ---------------------------------------------------
QKINDS = ('uniform', 'quniform', 'qloguniform', 'qnormal', 'qlognormal', 'loguniform')


def _history(n_trials, seed):
    """(group, tids, losses, obs): tied quantized observations and a
    qlognormal (and qloguniform) observation of 0."""
    rng = np.random.RandomState(seed)
    tids = np.arange(n_trials) * 2 + 1
    losses = np.round(rng.randn(n_trials), 1)
    args = {'uniform': dict(low=-5.0, high=5.0), 'quniform': dict(low=0.0, high=10.0, q=2.0),
            'qloguniform': dict(low=math.log(0.2), high=math.log(40.0), q=1.0),
            'qnormal': dict(mu=1.0, sigma=2.0, q=0.5), 'qlognormal': dict(mu=0.0, sigma=1.0, q=0.5),
            'loguniform': dict(low=-3.0, high=2.0)}
    group, obs = [], {}
    for d, kind in enumerate(QKINDS):
        a = args[kind]
        if kind == 'uniform':
            v = rng.uniform(-5, 5, n_trials)
        elif kind == 'loguniform':
            v = np.exp(rng.uniform(-3, 2, n_trials))
        elif kind == 'quniform':
            v = np.rint(rng.uniform(0, 10, n_trials) / 2.0) * 2.0
        elif kind == 'qloguniform':
            v = np.rint(np.exp(rng.uniform(a['low'], a['high'], n_trials)))
        elif kind == 'qnormal':
            v = np.rint((1.0 + 2.0 * rng.randn(n_trials)) / 0.5) * 0.5
        else:
            v = np.rint(np.exp(rng.randn(n_trials)) / 0.5) * 0.5
        if n_trials > 4 and kind in ('qloguniform', 'qlognormal'):
            v[3] = 0.0
        group.append(('h%d' % d, kind, a))
        obs['h%d' % d] = (tids.copy(), v)
    return group, tids, losses, obs


def _sorted_rows(mu, s):
    order = np.lexsort((s, mu))
    return np.asarray(mu)[order], np.asarray(s)[order]


@pytest.mark.parametrize('n_trials,gamma', [(40, 0.25), (40, 4.0), (1, 0.25), (0, 0.25)])
def test_quantized_marginals_equal_univariate_posteriors(n_trials, gamma):
    group, tids, losses, obs = _history(n_trials, 200 + n_trials)
    if n_trials >= 40:
        assert 0.0 in obs['h4'][1] and 0.0 in obs['h2'][1]
        assert len(np.unique(obs['h1'][1])) < n_trials // 2        # ties
    splitter = P.Splitter(tids, losses, gamma)
    out = P.joint_mixture(group, obs, splitter, 1.0, quantized=True)
    assert len(out) == 10 and out.upper.tolist() == [0] * 6 and len(out.cat_p) == 0
    dims, wb, mub, sigb, wa, mua, siga, q = out.dims, out.wb, out.mub, out.sigb, out.wa, out.mua, out.siga, out.q
    assert q.tolist() == [0.0, 2.0, 1.0, 0.5, 0.5, 0.0] and q.dtype == np.float64
    assert list(dims['flags']) == [3, 3, 3, 0, 0, 3]
    assert [bool(k) for k in dims['kind']] == [False, False, True, False, True, True]
    assert (dims[2]['low'], dims[2]['high']) == (math.log(0.2), math.log(40.0))
    assert np.all(np.isfinite(mub)) and np.all(np.isfinite(mua))
    for d, (label, kind, args) in enumerate(group):
        b, a = splitter.split(*obs[label])
        post = P.label_posterior(label, kind, args, b, a, 1.0)
        assert (post.q or 0.0) == q[d]
        for (W, mu, s), (w1, m1, s1) in (((wb, mub, sigb), post.below), ((wa, mua, siga), post.above)):
            assert len(W) == len(w1)
            gm, gs = _sorted_rows(mu[:, d], s[:, d])
            em, es = _sorted_rows(m1, s1)
            assert np.array_equal(gm, em) and np.array_equal(gs, es), (label, 'mu / sigma')
    # the definition's own transform (not plain np.log)
    for d, (label, kind, args) in enumerate(group):
        tr = QR.prior_of(kind, args)[6]
        for side, (mu, _) in enumerate(((mub, sigb), (mua, siga))):
            o = splitter.split(*obs[label])[side]
            assert np.array_equal(mu[1:, d], tr(o))


def test_default_call_is_unchanged():
    group, tids, losses, obs = _history(30, 5)
    splitter = P.Splitter(tids, losses, 0.25)
    with pytest.raises(ValueError):
        P.joint_mixture(group, obs, splitter, 1.0)
    with pytest.raises(ValueError):
        P.joint_prior('quniform', dict(low=0.0, high=1.0, q=0.5))
    with pytest.raises(ValueError):
        P.joint_prior('randint', dict(upper=3), quantized=True)
    dense = [g for g in group if g[1] in P.JOINT_KINDS]
    a = P.joint_mixture(dense, obs, splitter, 1.0)
    b = P.joint_mixture(dense, obs, splitter, 1.0, quantized=True)
    assert len(a) == len(b) == 10 and a.q.tolist() == b.q.tolist() == [0.0, 0.0]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    pri = P.joint_prior('uniform', dict(low=0.0, high=2.0))
    assert (pri.log, pri.bounded, pri.low, pri.high, pri.mu, pri.sigma) == (False, True, 0.0, 2.0, 1.0, 2.0)
    assert pri.q == 0.0 and pri.upper == 0 and pri.p is None
    pri = P.joint_prior('qlognormal', dict(mu=0.5, sigma=2.0, q=3.0), quantized=True)
    assert (pri.log, pri.bounded, pri.low, pri.high, pri.mu, pri.sigma) == (True, False, 0.0, 0.0, 0.5, 2.0)
    assert pri.q == 3.0 and pri.upper == 0 and pri.p is None
    assert P.JOINT_KINDS == ('uniform', 'loguniform', 'normal', 'lognormal')
    assert P.JOINT_QUANT_KINDS == ('quniform', 'qloguniform', 'qnormal', 'qlognormal')


# -- groups ---------------------------------------------------------------------------
WIDE = P.JOINT_KINDS + P.JOINT_QUANT_KINDS


def test_groups_with_and_without_the_widened_kinds():
    domain = Domain(GC.loss, GC.space())
    specs = tpe.specs_of(domain)
    assert tpe.joint_groups(domain, specs) == GC.GROUPS
    assert tpe.joint_groups(domain, specs, None, WIDE) == [(0, ['ly', 'x']), (1, ['a', 'b', 'qa']),
                                                           (2, ['d1', 'd2'])]
    assert tpe.joint_group(domain, specs) == tpe.joint_group(domain, specs, None, WIDE) == ['ly', 'x']
    # the signatures are unchanged but for the new, last, defaulted argument
    for fn in (tpe.joint_group, tpe.joint_groups):
        ps = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in ps[:3]] == ['domain', 'specs', 'obs'] and ps[3].default == P.JOINT_KINDS
    # a (uniform, quniform) pair inside one hp.choice branch: a group only with the keyword's kinds
    space = {'x': hp.uniform('x', 0, 1),
             'c': hp.choice('c', [{'u': hp.uniform('u', 0, 1), 'n': hp.quniform('n', 0, 8, 1)}, {'k': 1}])}
    d2 = Domain(lambda d: 0.0, space)
    s2 = tpe.specs_of(d2)
    assert tpe.joint_groups(d2, s2) == []
    assert tpe.joint_groups(d2, s2, None, WIDE) == [(0, ['n', 'u'])]
    # unconditional: x with a quantized label
    d3 = Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'q': hp.quniform('q', 0, 9, 1),
                                'r': hp.randint('r', 4)})
    s3 = tpe.specs_of(d3)
    assert tpe.joint_group(d3, s3) is None
    assert tpe.joint_group(d3, s3, None, WIDE) == ['q', 'x']


def test_keyword_needs_multivariate():
    domain = Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'q': hp.quniform('q', 0, 9, 1)})
    with pytest.raises(ValueError):
        tpe.suggest([0], domain, Trials(), 0, joint_quantized=True, multivariate=False)
    with pytest.raises(ValueError):
        tpe.suggest([0], domain, Trials(), 0, joint_quantized=True)
    with pytest.raises(ValueError):
        tpe.suggest([0], domain, Trials(), 0, devices=[0, 1], multivariate=True, joint_quantized=True)


# -- what the GPU tests rest on --------------------------------------------------------
def test_group_shapes():
    for name, (Dn, Kb, Ka, kinds, _) in QC.GROUPS.items():
        ref = QC.group(name)
        assert ref.D == Dn and len(ref.sides['below'][0]) == Kb and len(ref.sides['above'][0]) == Ka
        nq = int(np.count_nonzero(ref.steps))
        assert nq >= 1 and Dn + nq <= 128
    assert QC.group('q60_fine').D + int(np.count_nonzero(QC.group('q60_fine').steps)) == 120
    assert 0 < np.count_nonzero(QC.group('q2_mixed').steps) < 2
    co = QC.group(QC.COARSE)
    vals = co.port_draw(6, 5, np.arange(300, dtype=np.uint64))[1]
    for d in range(3):
        assert 2 <= len(np.unique(vals[:, d])) <= 4, (d, np.unique(vals[:, d]))
    assert 0.0 in vals[:, 1]                      # the qloguniform grid holds 0
    assert len(np.unique(vals, axis=0)) < 100      # duplicate candidates


@pytest.mark.parametrize('case', range(len(QC.DRAWS)))
def test_committed_draw_seeds_exclude_nothing(case):
    name, seed, rnd, offset, n = QC.DRAWS[case]
    ref = QC.group(name)
    _, vals, excl = ref.port_draw(seed, rnd, offset + np.arange(n, dtype=np.uint64))
    assert not excl.any() and np.all(np.isfinite(vals))
    for d, dim in enumerate(ref.dims):
        if dim.q is not None:
            assert np.array_equal(np.rint(vals[:, d] / dim.q) * dim.q, vals[:, d])


@pytest.mark.parametrize('case', range(len(QC.ROUNDS)))
def test_committed_round_seeds_leave_a_margin(case):
    """The reference alone: the port's candidates exclude nothing and the
    best reference score leads the best different configuration by more than
    1e-9 (|ll| + |lg|)."""
    name, seed, rnd, n = QC.ROUNDS[case]
    ref = QC.group(name)
    _, vals, excl = ref.port_draw(seed, rnd, np.arange(n, dtype=np.uint64))
    assert not excl.any()
    ll, lg = ref.joint_lpdf(vals, 'below'), ref.joint_lpdf(vals, 'above')
    assert not np.isnan(ll - lg).any()
    ok, _ = QC.margin_ok(vals, ll, lg)
    assert ok


def test_layout_round_excludes_nothing():
    name, seed, rnd, n, first = QC.LAYOUT
    ref = QC.group(name)
    _, vals, excl = ref.port_draw(seed, rnd, np.arange(first, dtype=np.uint64))
    assert not excl.any() and np.all(np.isfinite(vals))


def test_fine_group_underflows_and_is_finite():
    """q60_fine at its test points: every component's product of the 60
    quantized factors, in 30-digit arithmetic, is below 1e-320 -- a plain fp64
    product is 0 -- and the definition's lpdf is finite."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 30
    ref = QC.group(QC.FINE)
    name, seed, rnd, n = [r for r in QC.ROUNDS if r[0] == QC.FINE][0]
    drawn = ref.port_draw(seed, rnd, np.arange(n, dtype=np.uint64))[1]
    fixed = QC.fixed_points(ref, np.random.RandomState(1))
    pts = np.concatenate([fixed[:3], fixed[8:9], drawn[:2]])
    for side in ('below', 'above'):
        assert np.all(np.isfinite(ref.joint_lpdf(np.concatenate([fixed, drawn]), side)))
        W, mu, s = ref.sides[side]
        for x in pts:
            ends = [QR.interval(dim, x[d:d + 1]) for d, dim in enumerate(ref.dims)]
            for k in range(len(W)):
                prod = mp.mpf(1)
                for d in range(ref.D):
                    ub, lb = float(ends[d][0][0]), float(ends[d][1][0])
                    a = (mp.mpf(lb) - mp.mpf(float(mu[k, d]))) / (mp.mpf(float(s[k, d])) * mp.sqrt(2))
                    b = (mp.mpf(ub) - mp.mpf(float(mu[k, d]))) / (mp.mpf(float(s[k, d])) * mp.sqrt(2))
                    prod *= (mp.erfc(a) - mp.erfc(b)) / 2
                assert 0 <= prod < mp.mpf('1e-320'), (side, k, prod)
