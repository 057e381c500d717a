"""tpe.suggest(fixed=...) without a GPU: the conditioning rule restated in
tests/joint_fixed_reference.py satisfies the constant-difference identity
under the dense definition JointRef.joint_lpdf; the keyword's validation; the
startup documents; an empty `fixed`; and what _joint_rounds asks of an engine."""
import logging
import math

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, labels, tpe
from hyperopt_amd import posterior as P
from hyperopt_amd.base import Domain
from tests import joint_fixed_reference as FR
from tests import joint_reference as JR
from tests import test_joint_bandwidth_host as BH

PW = 1.0
FIVE = ['uniform', 'loguniform', 'normal', 'lognormal', 'uniform']
TYPICAL = {'uniform': 1.75, 'loguniform': 0.4, 'normal': 0.25, 'lognormal': 1.5}
# the far edge of the range: a bound itself, six prior sigmas out without one
EDGE = {'uniform': -5.0, 'loguniform': math.exp(2.0), 'normal': 1.0 + 6.0 * 2.0, 'lognormal': math.exp(-6.0)}

CASES = [(kinds, n, fixed, edge)
         for kinds, subsets in ((FIVE[:2], [(0,), (1,)]), (FIVE, [(0,), (1, 3), (0, 2, 4), (0, 1, 2, 4)]))
         for n in (1, 2, 30, 300, 1100)
         for fixed in subsets
         for edge in (False, True)]


def dense_case(kinds, n, seed):
    """(dims, below, above) of the neighbour-rule mixtures of n trials."""
    specs = BH.specs_of(kinds)
    tids, losses, cols = BH.history(specs, n, seed)
    mix = P.joint_mixture(list(specs.values()), cols, P.Splitter(tids, losses, 0.25), PW)
    dims = [JR.Dim(log, low, high, d) for d, (log, low, high, _, _) in
            enumerate(JR.prior_of(s.kind, s.args) for s in specs.values())]
    return dims, (mix.wb, mix.mub, mix.sigb), (mix.wa, mix.mua, mix.siga)


@pytest.mark.parametrize('kinds,n,fixed,edge', CASES,
                         ids=['D%d-n%d-F%s-%s' % (len(k), n, ''.join(map(str, f)), 'edge' if e else 'mid')
                              for k, n, f, e in CASES])
def test_conditioned_mixture_differs_by_a_constant(kinds, n, fixed, edge):
    """lpdf_full(x_F, x_R) - lpdf_cond(x_R) is one number for all 24
    candidates drawn from the conditioned mixture, on both sides, within 1e-9
    max(1, |lpdf|)."""
    dims, below, above = dense_case(kinds, n, 3000 + n)
    values = [(EDGE if edge else TYPICAL)[kinds[d]] for d in fixed]
    free, cb, ca, (rb, ra) = FR.condition(dims, below, above, fixed, values, PW)
    assert free == [d for d in range(len(kinds)) if d not in fixed]
    for W, rel in ((cb[0], rb), (ca[0], ra)):
        assert min(W) >= FR.FLOOR and abs(math.fsum(W) - 1.0) <= 1e-12
        assert all(w == FR.FLOOR for w, r in zip(W, rel) if r < -745.0)
    full = JR.JointRef(dims, below, above)
    cond = JR.JointRef([dims[d] for d in free], cb, ca)
    _, xr, _ = cond.port_draw(11, 5, np.arange(24))
    x = np.empty((24, len(kinds)))
    x[:, free] = xr
    x[:, list(fixed)] = values
    for side in ('below', 'above'):
        lf, lc = full.joint_lpdf(x, side), cond.joint_lpdf(xr, side)
        assert np.all(np.isfinite(lf)) and np.all(np.isfinite(lc))
        diff = lf - lc
        bar = 1e-9 * max(1.0, float(np.max(np.abs(lf))), float(np.max(np.abs(lc))))
        assert float(np.max(diff) - np.min(diff)) <= bar, (side, float(np.max(diff) - np.min(diff)), bar)


def test_weights_underflow_in_linear_space():
    """What makes the log-space form and the floor necessary: from 300 trials
    on most above components lie more than 745 nats below the largest."""
    dims, below, above = dense_case(FIVE, 300, 3300)
    _, _, ca, (_, ra) = FR.condition(dims, below, above, (0, 2, 4), [EDGE[FIVE[d]] for d in (0, 2, 4)], PW)
    under = [r for r in ra if r < -745.0]
    assert len(under) > len(ra) // 2
    assert all(w == FR.FLOOR for w, r in zip(ca[0], ra) if r < -745.0)


def test_reference_factors():
    from tests import joint_cat_reference as CR
    lin = CR.CDim(False, 0.0, 6.0, 0, q=2.0)
    assert FR.interval(lin, 6.0) == (6.0, 5.0) and FR.interval(lin, 8.0) == (6.0, 7.0)
    assert FR.log_factor(lin, 8.0, 1, 4, 3.0, 1.0, PW) == FR.NEG_INF          # an empty interval
    cat = CR.CDim(False, None, None, 0, upper=3, p=[0.2, 0.5, 0.3])
    a = 3 * PW / 4
    assert FR.log_factor(cat, 1.0, 0, 4, 0.0, 1.0, PW) == math.log(0.5)
    assert FR.log_factor(cat, 1.0, 2, 4, 1.0, 1.0, PW) == math.log((1.0 + a * 0.5) / (1.0 + a))
    assert FR.log_factor(cat, 1.0, 2, 4, 2.0, 1.0, PW) == math.log(a * 0.5 / (1.0 + a))
    assert FR.log_factor(cat, 3.0, 2, 4, 2.0, 1.0, PW) == FR.NEG_INF
    with pytest.raises(ValueError):
        FR.condition_side([lin, lin], [0.5, 0.5], [[3.0, 3.0]] * 2, [[1.0, 1.0]] * 2, [0], [8.0], PW)


# -- the keyword ---------------------------------------------------------------------------------
def kw_space():
    return {'u': hp.uniform('u', -5, 5), 'lu': hp.loguniform('lu', -3, 2), 'n': hp.normal('n', 0, 1),
            'ln': hp.lognormal('ln', 0, 1), 'qu': hp.quniform('qu', 8, 512, 8),
            'qlu': hp.qloguniform('qlu', 0, 5, 2), 'qn': hp.qnormal('qn', 0, 3, 0.5),
            'qln': hp.qlognormal('qln', 0, 1, 1), 'ri': hp.randint('ri', 5),
            'opt': hp.choice('opt', [{'kind': 0, 'a': hp.uniform('a', -2, 2)}, {'kind': 1, 'b': hp.normal('b', 0, 1)}])}


def kw_domain():
    return Domain(lambda d: 0.0, kw_space())


BAD = [
    ([('u', 1.0)], 'dict'),                       # not a dict
    ('u=1', 'dict'),
    ({'nope': 1.0}, 'unknown label'),
    ({'u': float('nan')}, 'not finite'),
    ({'n': float('inf')}, 'not finite'),
    ({'u': 'x'}, 'not a number'),
    ({'u': 5.5}, 'outside'),
    ({'u': -5.0001}, 'outside'),
    ({'lu': math.exp(2.0) * 1.01}, 'outside'),
    ({'lu': math.exp(-3.0) * 0.99}, 'outside'),
    ({'lu': 0.0}, 'not positive'),
    ({'ln': -1.0}, 'not positive'),
    ({'qu': 12.0}, 'grid'),
    ({'qn': 0.3}, 'grid'),
    ({'qu': 520.0}, 'misses'),                    # on the grid, [516, 524] beyond 512
    ({'qu': 0.0}, 'misses'),                      # [-4, 4] below 8
    ({'qlu': 160.0}, 'misses'),                   # [159, 161] beyond exp(5) = 148.4
    ({'qln': -1.0}, 'misses'),                    # [-1.5, -0.5]: no positive value rounds to it
    ({'ri': 5}, 'integer in'),
    ({'ri': -1}, 'integer in'),
    ({'ri': 1.5}, 'integer in'),
    ({'opt': 2}, 'integer in'),
]


@pytest.mark.parametrize('fixed,match', BAD, ids=[str(i) for i in range(len(BAD))])
@pytest.mark.parametrize('multivariate', [False, True])
def test_keyword_validation(fixed, match, multivariate):
    """Every error, on an empty Trials: raised before anything else runs."""
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], kw_domain(), H.Trials(), 1, fixed=fixed, multivariate=multivariate)


def test_validation_comes_first():
    """(the other keywords' own errors come after it)"""
    with pytest.raises(ValueError, match='unknown label'):
        tpe.suggest([0], kw_domain(), H.Trials(), 1, fixed={'nope': 1}, precision='f16')


def test_valid_values_pass():
    specs = tpe.specs_of(kw_domain())
    ok = {'u': 5.0, 'lu': math.exp(2.0), 'n': -40.0, 'ln': 1e-9, 'qu': 512.0, 'qlu': 0.0, 'qn': -1.5, 'qln': 0.0,
          'ri': np.int64(4), 'opt': 1.0, 'a': -2.0, 'b': 3}
    got = tpe.check_fixed(specs, ok)
    assert got == {k: float(v) for k, v in ok.items() if k not in ('ri', 'opt')} | {'ri': 4, 'opt': 1}
    assert type(got['ri']) is int and type(got['opt']) is int and type(got['b']) is float
    assert tpe.check_fixed(specs, None) == {} and tpe.check_fixed(specs, {}) == {}


def _vals(docs):
    return [d['misc']['vals'] for d in docs]


def test_startup_documents_hold_the_fixed_values():
    domain = kw_domain()
    ids = list(range(12))
    for opt, inside, outside in ((0, 'a', 'b'), (1, 'b', 'a')):
        fixed = {'lu': 0.25, 'qu': 64.0, 'ri': 3, 'opt': opt, 'a': 1.5, 'b': -0.5}
        docs = tpe.suggest(ids, domain, H.Trials(), 7, fixed=fixed)
        assert len(docs) == len(ids)
        for v in _vals(docs):
            assert v['lu'] == [0.25] and v['qu'] == [64.0] and v['ri'] == [3] and v['opt'] == [opt]
            assert v[inside] == [fixed[inside]] and v[outside] == []      # the fixed choice selects the branch
            assert all(len(v[k]) == 1 for k in ('u', 'n', 'ln', 'qlu', 'qn', 'qln'))
        assert len(set(v['u'][0] for v in _vals(docs))) == len(ids)       # distinct draws
    # a fixed label under a branch the document does not enter is dropped, like any other
    docs = tpe.suggest(ids, domain, H.Trials(), 7, fixed={'a': 1.5})
    opts = [v['opt'][0] for v in _vals(docs)]
    assert set(opts) == {0, 1}
    assert all(v['a'] == ([1.5] if v['opt'] == [0] else []) for v in _vals(docs))
    # batch='pending' passes the keyword on through its startup phase
    docs = tpe.suggest(ids[:3], domain, H.Trials(), 7, fixed={'u': 2.0}, batch='pending')
    assert [v['u'] for v in _vals(docs)] == [[2.0]] * 3


def test_a_fixed_label_consumes_no_random_numbers():
    """The other labels are drawn in the order they always are: fixing the
    label drawn last leaves every other value of the first document as it was."""
    domain = kw_domain()
    specs = tpe.specs_of(domain)
    plain = labels.sample_config(domain.expr, specs, np.random.RandomState(3))
    rng = np.random.RandomState(3)
    order = []
    impls = dict(labels.IMPLS)
    try:
        for kind, fn in impls.items():
            labels.IMPLS[kind] = (lambda fn: lambda rng, **a: (order.append(1), fn(rng=rng, **a))[1])(fn)
        labels.sample_config(domain.expr, specs, np.random.RandomState(3))
    finally:
        labels.IMPLS.update(impls)
    assert len(order) == len(plain)
    # fix every active label but one: that one is the first draw of the state
    for free in plain:
        fixed = {k: v for k, v in plain.items() if k != free}
        got = labels.sample_config(domain.expr, specs, np.random.RandomState(3), fixed)
        s = specs[free]
        want = labels.coerce(s.kind, labels.IMPLS[s.kind](rng=np.random.RandomState(3), **s.args))
        assert got[free] == want and all(got[k] == plain[k] for k in fixed)
    assert labels.sample_config(domain.expr, specs, rng, {}) == plain


def test_empty_fixed_is_no_keyword():
    domain = kw_domain()
    ids = [0, 1, 2]
    want = _vals(tpe.suggest(ids, domain, H.Trials(), 5))
    assert want == _vals(H.rand.suggest(ids, domain, H.Trials(), 5))
    for empty in (None, {}):
        assert _vals(tpe.suggest(ids, domain, H.Trials(), 5, fixed=empty)) == want
        assert _vals(tpe.suggest(ids, domain, H.Trials(), 5, fixed=empty, batch='pending')) == want


def test_empty_fixed_is_not_handed_on(monkeypatch):
    """batch='pending' recurses with the call's keywords: an empty `fixed` is
    not among them."""
    domain = kw_domain()
    trials = H.Trials()
    H.fmin(lambda d: 0.0, kw_space(), algo=H.rand.suggest, max_evals=3, trials=trials,
           rstate=np.random.RandomState(1))
    seen = []
    real = tpe.suggest

    def spy(new_ids, domain, trials, seed, **kw):
        seen.append(kw)
        if len(seen) > 1:
            return []
        return real(new_ids, domain, trials, seed, **kw)
    monkeypatch.setattr(tpe, 'suggest', spy)
    tpe.suggest([10, 11], domain, trials, 5, fixed={}, batch='pending', n_startup_jobs=0)
    assert len(seen) > 1 and all('fixed' not in kw for kw in seen[1:])
    del seen[:]
    tpe.suggest([10, 11], domain, trials, 5, fixed={'u': 1.0}, batch='pending', n_startup_jobs=0)
    assert len(seen) > 1 and all(kw['fixed'] == {'u': 1.0} for kw in seen[1:])


# -- what _joint_rounds asks of an engine --------------------------------------------------------
class StubEngine(BH.StubEngine):
    def joint_condition(self, slot, dims, values, dst=None):
        assert dst is None
        self.calls.append(('condition', (slot, list(dims), list(values))))
        self.D[slot] -= len(dims)


def test_joint_rounds_condition_and_map_the_free_labels(caplog):
    from hyperopt_amd import history as history_mod
    space = {'x': hp.uniform('x', -5, 5), 'ly': hp.loguniform('ly', -3, 2), 'z': hp.normal('z', 0, 1)}

    def loss(d):
        return float(d['x'] ** 2 + np.log(d['ly']) ** 2 + d['z'] ** 2)
    trials = H.Trials()
    H.fmin(loss, space, algo=H.rand.suggest, max_evals=30, trials=trials, rstate=np.random.RandomState(4))
    domain = Domain(loss, space)
    specs = tpe.specs_of(domain)
    view = history_mod.device_view(domain, trials, list(specs))
    assert list(specs) == ['ly', 'x', 'z']
    for v in (view, None):
        eng = StubEngine()
        caplog.clear()
        with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
            out = tpe._joint_rounds(eng, domain, trials, specs, None, 0.25, PW, 7, [50, 51], 24, view=v,
                                    fixed={'x': 1.5})
        assert [c[0] for c in eng.calls] == ['build' if v is not None else 'set', 'condition']
        assert eng.calls[1][1] == (0, [1], [1.5])
        assert out == [{'ly': 0.5, 'z': 0.5}] * 2                  # the winner's columns are the free labels'
        assert any('1 group(s) conditioned' in r.getMessage() for r in caplog.records)
        # every label of the group fixed: not built, the independent path's answer
        eng = StubEngine()
        assert tpe._joint_rounds(eng, domain, trials, specs, None, 0.25, PW, 7, [50], 24, view=v,
                                 fixed={'x': 1.5, 'ly': 0.5, 'z': 0.0}) is None
        assert eng.calls == []
        # no fixed label in the group: the call without the keyword
        eng = StubEngine()
        tpe._joint_rounds(eng, domain, trials, specs, None, 0.25, PW, 7, [50], 24, view=v, fixed={})
        assert [c[0] for c in eng.calls] == ['build' if v is not None else 'set']
