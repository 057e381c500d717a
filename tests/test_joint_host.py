"""Multivariate (joint) TPE, host side (CPU): the joint group of a space, the
host build of the joint mixtures against the definition in
tests/joint_reference.py and against the univariate posteriors, the fallback
rules of tpe.suggest(multivariate=True), and -- through the fp64 draw port --
that the seeds test_joint_gpu.py uses exclude no draw and leave every round's
winner a clear margin."""
import logging

import numpy as np
import pytest

from hyperopt_amd import hp, labels as LB, posterior as P, rand, tpe
from hyperopt_amd.base import Domain, Trials
from tests import joint_cases as JC
from tests import joint_reference as JR


def nested_space():
    return {'x': hp.uniform('x', -5, 5), 'ly': hp.loguniform('ly', -3, 2),
            'q': hp.quniform('q', 0, 10, 1),
            'c': hp.choice('c', [
                {'a': hp.uniform('a', 0, 1),
                 'inner': hp.choice('inner', [hp.normal('deep', 0, 1), 2.0])},
                {'b': hp.lognormal('b', 0, 1)}]),
            'n': hp.normal('n', 0, 2)}


def test_unconditional_labels_nested_choice():
    domain = Domain(lambda d: 0.0, nested_space())
    free = LB.unconditional_labels(domain.expr)
    assert free == {'x', 'ly', 'q', 'c', 'n'}
    specs = tpe.specs_of(domain)
    assert set(specs) == free | {'a', 'inner', 'deep', 'b'}
    # the joint group: unconditional and of a dense continuous kind, in the specs' order
    assert tpe.joint_group(domain, specs) == ['ly', 'n', 'x']


def test_unconditional_labels_reference_graph():
    """On the reference's own pyll graph (tests/golden/reference_domain_graph.json)."""
    from tests.test_api import _reference_expr
    assert LB.unconditional_labels(_reference_expr()) == {'a', 'k', 'n'}


def _history(n_trials, kinds, seed, ties=True):
    """(group [(label, kind, args)], tids, losses, obs) of a synthetic history
    whose observations hold exact ties."""
    rng = np.random.RandomState(seed)
    tids = np.arange(n_trials) * 2 + 1
    losses = np.round(rng.randn(n_trials), 1)
    group, obs = [], {}
    for d, kind in enumerate(kinds):
        label = 'h%d' % d
        if kind == 'uniform':
            args = dict(low=-5.0, high=5.0)
            v = rng.uniform(-5, 5, n_trials)
        elif kind == 'loguniform':
            args = dict(low=-3.0, high=2.0)
            v = np.exp(rng.uniform(-3, 2, n_trials))
        elif kind == 'normal':
            args = dict(mu=1.0, sigma=2.0)
            v = 1.0 + 2.0 * rng.randn(n_trials)
        else:
            args = dict(mu=0.0, sigma=1.0)
            v = np.exp(rng.randn(n_trials))
        if ties:
            v = np.round(v, 1) if kind in ('uniform', 'normal') else np.exp(np.round(np.log(v), 1))
            v[5] = v[17]
            v[n_trials - 1] = v[2]
        group.append((label, kind, args))
        obs[label] = (tids.copy(), v)
    return group, tids, losses, obs


def _sorted_rows(w, mu, s):
    order = np.lexsort((w, s, mu))
    return np.asarray(w)[order], np.asarray(mu)[order], np.asarray(s)[order]


@pytest.mark.parametrize('n_trials,gamma', [(40, 0.25), (40, 4.0), (20, 0.25), (1, 0.25), (2, 0.25)])
def test_marginals_equal_univariate_posteriors(n_trials, gamma):
    """An all-unbounded group: per dimension the joint components (W, mu_kd,
    s_kd) are the univariate label_posterior mixture of that label.  mu and
    sigma match bit for bit in every dimension, and so do the weights of the
    group's first label, whose normalisation the joint mixture takes.  The
    other labels' weights are the same numbers divided by the sum of the same
    terms taken in that label's own sorted order (adaptive_parzen_normal's
    `weights / weights.sum()`), so they are bit-identical whenever that sum
    is exact -- a side without the linear-forgetting ramp, n_S <= 25: all
    terms are 1 -- and otherwise agree to the rounding of two sums of K terms,
    2 K 2^-53 relative (on random histories with a ramp the last bit differs
    in about two calls of three, so no single W can equal every label's)."""
    kinds = ('normal', 'lognormal', 'normal')
    if n_trials >= 20:
        group, tids, losses, obs = _history(n_trials, kinds, 100 + n_trials)
    else:
        group, tids, losses, obs = _history(n_trials, kinds, 100 + n_trials, ties=False)
    splitter = P.Splitter(tids, losses, gamma)
    mix = P.joint_mixture(group, obs, splitter, 1.0)
    assert list(mix.dims['flags']) == [0, 0, 0]
    ramp = False
    for d, (label, kind, args) in enumerate(group):
        b, a = splitter.split(*obs[label])
        post = P.label_posterior(label, kind, args, b, a, 1.0)
        for (W, mu, s), (w1, m1, s1) in (((mix.wb, mix.mub, mix.sigb), post.below),
                                         ((mix.wa, mix.mua, mix.siga), post.above)):
            assert len(W) == len(w1)
            gw, gm, gs = _sorted_rows(W, mu[:, d], s[:, d])
            ew, em, es = _sorted_rows(w1, m1, s1)
            assert np.array_equal(gm, em) and np.array_equal(gs, es), (label, 'mu / sigma')
            if d == 0 or len(W) - 1 <= P.DEFAULT_LF:
                assert np.array_equal(gw, ew), (label, 'weights')
            else:
                ramp = True
                assert np.all(np.abs(gw - ew) <= 2 * len(W) * 2.0 ** -53 * ew), (label, 'weights')
    assert ramp == (n_trials == 40 and gamma == 0.25)


def test_weights_identical_across_dimensions():
    """Each label's own weights at the joint positions: identical across the
    labels without a ramp; with one, equal to the rounding of their sums."""
    kinds = ('uniform', 'loguniform', 'normal', 'lognormal')
    for n_trials, exact in ((24, True), (40, False)):
        group, tids, losses, obs = _history(n_trials, kinds, 7)
        splitter = P.Splitter(tids, losses, 0.25)
        for side in (0, 1):
            cols, priors = [], []
            for label, kind, args in group:
                log, low, high, pmu, psig = JR.prior_of(kind, args)
                o = np.asarray(splitter.split(*obs[label])[side], dtype=float)
                cols.append(np.log(o) if log else o)
                priors.append((pmu, psig))
            Ws, _, _ = JR.side_mixture(cols, priors, 1.0, P.adaptive_parzen_normal)
            for W in Ws[1:]:
                if exact or len(W) - 1 <= P.DEFAULT_LF:
                    assert np.array_equal(W, Ws[0])
                else:
                    assert np.all(np.abs(W - Ws[0]) <= 2 * len(W) * 2.0 ** -53 * Ws[0])


@pytest.mark.parametrize('n_trials', [0, 1, 2, 40, 300])
def test_joint_mixture_equals_reference(n_trials):
    kinds = ('uniform', 'loguniform', 'normal', 'lognormal')
    group, tids, losses, obs = _history(n_trials, kinds, 31 + n_trials, ties=n_trials >= 20)
    splitter = P.Splitter(tids, losses, 0.25)
    out = P.joint_mixture(group, obs, splitter, 0.7, streams=[4, 9, 1, 6])
    dims = out.dims
    assert list(dims['stream']) == [4, 9, 1, 6]
    for d, (label, kind, args) in enumerate(group):
        log, low, high, _, _ = JR.prior_of(kind, args)
        assert bool(dims[d]['kind']) == log
        assert (dims[d]['flags'] == 3) == (low is not None)
        if low is not None:
            assert (dims[d]['low'], dims[d]['high']) == (low, high)
    for side in (0, 1):
        cols, priors = [], []
        for label, kind, args in group:
            log, low, high, pmu, psig = JR.prior_of(kind, args)
            o = np.asarray(splitter.split(*obs[label])[side], dtype=float)
            cols.append(np.log(o) if log else o)
            priors.append((pmu, psig))
        Ws, mu, s = JR.side_mixture(cols, priors, 0.7, P.adaptive_parzen_normal)
        W, gm, gs = (out.wa, out.mua, out.siga) if side else (out.wb, out.mub, out.sigb)
        assert np.array_equal(W, Ws[0])
        assert np.array_equal(gm, mu) and np.array_equal(gs, s)
        assert abs(W.sum() - 1.0) < 1e-12 and gm.shape == (len(W), 4)


def _same_fields(a, b):
    assert type(a) is type(b) and a._fields == b._fields
    for name, x, y in zip(a._fields, a, b):
        if name == 'dims':
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), name
        else:
            assert type(x) is type(y) and x == y, name


def test_joint_records_do_not_depend_on_the_flags():
    """The quantized / categorical flags say which kinds may join; the record
    of a dense group, and of a kind of any family, is the same under every
    flag that accepts it: ten and nine fields, bit for bit."""
    D, _, _, kinds, gseed = JC.GROUPS['d5_k300']
    group, tids, losses, obs = _history(40, [kinds[d % len(kinds)] for d in range(D)], gseed)
    splitter = P.Splitter(tids, losses, 0.25)
    plain = P.joint_mixture(group, obs, splitter, 1.0)
    assert plain._fields == ('dims', 'wb', 'mub', 'sigb', 'wa', 'mua', 'siga', 'q', 'upper', 'cat_p')
    assert plain.q.dtype == np.float64 and plain.q.tolist() == [0.0] * D
    assert plain.upper.dtype == np.int32 and plain.upper.tolist() == [0] * D
    assert plain.cat_p.dtype == np.float64 and plain.cat_p.shape == (0,)
    assert plain.mub.shape == (len(plain.wb), D) and plain.siga.shape == (len(plain.wa), D)
    _same_fields(plain, P.joint_mixture(group, obs, splitter, 1.0, quantized=True))
    _same_fields(plain, P.joint_mixture(group, obs, splitter, 1.0, quantized=True, categorical=True))

    fields = ('log', 'bounded', 'low', 'high', 'mu', 'sigma', 'q', 'upper', 'p')
    every = (dict(), dict(quantized=True), dict(categorical=True), dict(quantized=True, categorical=True))
    dense = P.joint_prior('loguniform', dict(low=-3.0, high=2.0))
    assert dense._fields == fields and tuple(dense) == (True, True, -3.0, 2.0, -0.5, 5.0, 0.0, 0, None)
    for kw in every[1:]:
        _same_fields(dense, P.joint_prior('loguniform', dict(low=-3.0, high=2.0), **kw))
    quant = P.joint_prior('qnormal', dict(mu=1.0, sigma=2.0, q=0.5), quantized=True)
    assert quant._fields == fields and tuple(quant) == (False, False, 0.0, 0.0, 1.0, 2.0, 0.5, 0, None)
    _same_fields(quant, P.joint_prior('qnormal', dict(mu=1.0, sigma=2.0, q=0.5), quantized=True, categorical=True))
    cat = P.joint_prior('categorical', dict(upper=2, p=[0.25, 0.75]), categorical=True)
    assert cat._fields == fields and tuple(cat)[:8] == (False, False, 0.0, 0.0, 0.0, 1.0, 0.0, 2)
    assert cat.p.tolist() == [0.25, 0.75]
    both = P.joint_prior('categorical', dict(upper=2, p=[0.25, 0.75]), quantized=True, categorical=True)
    assert tuple(both)[:8] == tuple(cat)[:8] and np.array_equal(both.p, cat.p)


def test_joint_mixture_refuses_mismatched_trials():
    group, tids, losses, obs = _history(30, ('uniform', 'normal'), 3)
    obs['h1'] = (obs['h1'][0][:-1], obs['h1'][1][:-1])
    with pytest.raises(ValueError):
        P.joint_mixture(group, obs, P.Splitter(tids, losses, 0.25), 1.0)


def test_fallback_rules(caplog):
    # fewer than two joint labels
    d1 = Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'q': hp.quniform('q', 0, 9, 1),
                                'c': hp.choice('c', [hp.uniform('u', 0, 1), hp.normal('v', 0, 1)])})
    with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
        assert tpe.joint_group(d1, tpe.specs_of(d1)) is None
    assert any('independent path' in r.message for r in caplog.records)
    # labels observed in different trials
    d2 = Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'y': hp.normal('y', 0, 1)})
    specs = tpe.specs_of(d2)
    same = {'x': (np.arange(5), np.zeros(5)), 'y': (np.arange(5), np.zeros(5))}
    assert tpe.joint_group(d2, specs, same) == ['x', 'y']
    diff = {'x': (np.arange(5), np.zeros(5)), 'y': (np.arange(1, 6), np.zeros(5))}
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
        assert tpe.joint_group(d2, specs, diff) is None
    assert any('different trials' in r.message for r in caplog.records)


def test_multi_device_raises_value_error():
    domain = Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'y': hp.normal('y', 0, 1)})
    with pytest.raises(ValueError):
        tpe.suggest([0], domain, Trials(), 0, devices=[0, 1], multivariate=True)


def test_startup_phase_is_random_search():
    space = nested_space()
    domain = Domain(lambda d: 0.0, space)
    trials = Trials()
    got = tpe.suggest([0, 1, 2], domain, trials, 123, multivariate=True)
    want = rand.suggest([0, 1, 2], domain, trials, 123)
    assert [d['misc']['vals'] for d in got] == [d['misc']['vals'] for d in want]
    assert [d['misc']['idxs'] for d in got] == [d['misc']['idxs'] for d in want]


@pytest.mark.parametrize('case', range(len(JC.DRAWS)))
def test_committed_draw_seeds_exclude_nothing(case):
    name, seed, rnd, offset, n = JC.DRAWS[case]
    ref = JC.group(name)
    _, vals, excl = ref.port_draw(seed, rnd, offset + np.arange(n, dtype=np.uint64))
    assert not excl.any() and np.all(np.isfinite(vals))


@pytest.mark.parametrize('case', range(len(JC.ROUNDS)))
def test_committed_round_seeds_leave_a_margin(case):
    """The reference alone: the port's candidates exclude nothing and the
    best reference score leads the runner-up by more than 1e-9 (|ll| +
    |lg|)."""
    name, seed, rnd, n = JC.ROUNDS[case]
    ref = JC.group(name)
    _, vals, excl = ref.port_draw(seed, rnd, np.arange(n, dtype=np.uint64))
    assert not excl.any()
    ok, _ = JC.margin_ok(ref.joint_lpdf(vals, 'below'), ref.joint_lpdf(vals, 'above'))
    assert ok


def test_tiny_mass_component():
    ref = JC.group(JC.TINY)
    m = ref.masses('below')
    assert 0.0 < m[3, 0] < 1e-12
