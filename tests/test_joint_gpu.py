"""Multivariate (joint) TPE on the GPU (`-m gpu`): the joint score against
the numpy definition (tests/joint_reference.py), the joint draw against the
pointwise draw reference, the fused round against its own draw and score
entry points and against numpy, ties, errors, and tpe.suggest(...,
multivariate=True) end to end.  Groups, seeds and rounds: tests/joint_cases.py
(test_joint_host.py checks on the CPU that those seeds exclude no draw and
leave every winner a clear margin)."""
import logging
from functools import partial

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import hp, tpe
from oracle import draw_oracle as D
from tests import joint_cases as JC
from tests import joint_reference as JR
from tests.draw_check import check_draws

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


def _set(eng, name):
    ref = JC.group(name)
    eng.set_joint_posterior(*JC.engine_args(ref))
    return ref


def _assert_lpdf(got, ref, what):
    err = np.abs(got - ref)
    bound = 1e-9 * np.maximum(1.0, np.abs(ref))
    print('%s: %d points, worst |err| / bound %.3g' % (what, len(ref), float(np.max(err / bound))))
    bad = np.flatnonzero(~(err <= bound))
    assert len(bad) == 0, (what, bad[:5].tolist(), got[bad[:5]].tolist(), ref[bad[:5]].tolist())


# -- score --------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(JC.GROUPS))
def test_score_matches_definition(eng, name):
    """joint_score at box corners, 8-sigma outliers, component means and
    drawn candidates: |err| <= 1e-9 max(1, |ref|) on both lpdfs."""
    ref = _set(eng, name)
    pts = JC.fixed_points(ref, np.random.RandomState(1))
    drawn, _ = eng.joint_draw(77, 65, round=2)
    for what, vals in (('fixed', pts), ('drawn', drawn), ('one', drawn[:1])):
        ll, lg = eng.joint_score(vals)
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(lg))
        _assert_lpdf(ll, ref.joint_lpdf(vals, 'below'), '%s %s below' % (name, what))
        _assert_lpdf(lg, ref.joint_lpdf(vals, 'above'), '%s %s above' % (name, what))


def test_score_same_bits_split_and_fused(eng):
    """A candidate's lpdfs do not depend on how the round is laid out: scored
    among 100 (one workgroup per slice of components, merged by a second
    kernel) and among 40000 (one workgroup per tile, all slices) it has the
    same bits."""
    _set(eng, 'd33')
    vals, _ = eng.joint_draw(5, 40000, round=1)
    ll, lg = eng.joint_score(vals)
    ll2, lg2 = eng.joint_score(vals[:100])
    assert np.array_equal(ll[:100], ll2) and np.array_equal(lg[:100], lg2)
    assert np.isnan(eng.joint_score(np.full((1, 33), np.nan))[0][0])


# -- draw ---------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(JC.DRAWS)))
def test_draws_match_reference(eng, case):
    name, seed, rnd, offset, n = JC.DRAWS[case]
    ref = _set(eng, name)
    vals, comp = eng.joint_draw(seed, n, round=rnd, cand_offset=offset)
    g = offset + np.arange(n, dtype=np.uint64)
    pf = ref.pick_fold()
    wp, wu = D.draw_words(seed, JR.JOINT_STREAM, rnd, g)
    assert not D.excluded(pf, wp, wu).any()
    assert np.array_equal(comp, D.pick(pf, wp)), name
    for d, dim in enumerate(ref.dims):
        wpd, wud = D.draw_words(seed, dim.stream, rnd, g)
        for k in np.unique(comp):
            sel = comp == k
            check_draws(ref.fold(int(k), d), wpd[sel], wud[sel], vals[sel, d], 'joint',
                        '%s dim %d component %d' % (name, d, k))


def test_cand_offset_consistency(eng):
    _set(eng, 'd5_k300')
    whole, cw = eng.joint_draw(9, 300, round=4)
    part, cp = eng.joint_draw(9, 237, round=4, cand_offset=63)
    assert np.array_equal(whole[63:], part) and np.array_equal(cw[63:], cp)
    other, _ = eng.joint_draw(9, 300, round=5)
    assert not np.array_equal(whole, other)


# -- round --------------------------------------------------------------------
def _round_check(eng, ref, seed, rnd, n):
    vals, _ = eng.joint_draw(seed, n, round=rnd)
    ll, lg = eng.joint_score(vals)
    s = ll - lg
    assert not np.isnan(s).any()
    want = int(np.argmax(s))                  # the first of the largest
    v, idx, wl, wg = eng.joint_suggest(seed, n, round=rnd)
    assert idx == want
    assert np.array_equal(v, vals[idx]) and wl == ll[idx] and wg == lg[idx]
    return vals, idx


@pytest.mark.parametrize('case', range(len(JC.ROUNDS)))
def test_round_is_argmax_of_draw_and_score(eng, case):
    """joint_suggest(n) is the argmax (lowest index on ties) of
    joint_score(joint_draw(n)), its values and lpdfs bit-identical to those
    calls; and the index is numpy's argmax of the reference score on the
    device's candidates (the reference's margin is above 1e-9 (|ll| + |lg|)
    in every cell)."""
    name, seed, rnd, n = JC.ROUNDS[case]
    ref = _set(eng, name)
    vals, idx = _round_check(eng, ref, seed, rnd, n)
    ok, want = JC.margin_ok(ref.joint_lpdf(vals, 'below'), ref.joint_lpdf(vals, 'above'))
    assert ok, 'reference margin too small: pick another seed'
    assert idx == want


@pytest.mark.parametrize('name,n', [('d33', 40000), ('d70', 33000), ('d20', 140000), ('d5_k300', 140000)])
def test_round_many_workgroups_fused(eng, name, n):
    """Enough candidates for the fused layout -- one workgroup per tile runs
    every slice -- in each variant of the kernel: y' in LDS beside the exp
    table, in LDS alone, in 32 and in 8 registers."""
    ref = _set(eng, name)
    _round_check(eng, ref, 11, 3, n)


@pytest.mark.parametrize('n', [1, 24, 65, 5000])
def test_ties_go_to_the_lowest_index(eng, n):
    """Both sides the prior alone: both lpdfs of a candidate come from the
    same records by the same arithmetic, every score is exactly 0, and the
    winner is candidate 0 -- over one workgroup and over many."""
    _set(eng, 'd1_tie')
    vals, _ = eng.joint_draw(2, n, round=1)
    ll, lg = eng.joint_score(vals)
    assert np.array_equal(ll, lg)
    v, idx, wl, wg = eng.joint_suggest(2, n, round=1)
    assert idx == 0 and v[0] == vals[0, 0] and wl == wg == ll[0]


def test_ties_in_the_split_round(eng):
    """Equal mixtures on both sides with enough components for the split
    layout (one workgroup per slice, the merge kernel's reduce)."""
    ref = JC.group('d5_k300')
    dims, wa, mua, siga = JC.engine_args(ref)[0], *ref.sides['above']
    eng.set_joint_posterior(dims, wa[:60] / wa[:60].sum(), mua[:60], siga[:60],
                            wa[:60] / wa[:60].sum(), mua[:60], siga[:60])
    for n in (24, 3000):
        vals, _ = eng.joint_draw(6, n, round=2)
        ll, lg = eng.joint_score(vals)
        assert np.array_equal(ll, lg)
        assert eng.joint_suggest(6, n, round=2)[1] == 0


# -- errors -------------------------------------------------------------------
def test_errors():
    from hyperopt_amd.engine import Engine, EngineError
    e = Engine(0, 'f64')
    try:
        with pytest.raises(EngineError):
            e.joint_suggest(0, 24)
        lib, h = e.lib, e.h
        import ctypes
        buf = np.zeros(8)
        idx = ctypes.c_int64()
        a, b = ctypes.c_double(), ctypes.c_double()
        assert lib.tpe_joint_suggest_group(h, 0, 0, 0, 24, buf.ctypes.data, ctypes.byref(idx), ctypes.byref(a),
                                           ctypes.byref(b)) == L.TPE_ERR_ARG
        assert lib.tpe_joint_score_group(h, 0, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data) == L.TPE_ERR_ARG
        comp = np.zeros(8, dtype=np.int32)
        assert lib.tpe_joint_draw_group(h, 0, 0, 0, 1, 0, buf.ctypes.data, comp.ctypes.data) == L.TPE_ERR_ARG
        # a box that holds none of the below mixture's mass: the sampler error
        ref = JC.group('d1_prior')
        dims, wb, mub, sigb, wa, mua, siga = JC.engine_args(ref)
        far = mub + 1e6 * (dims['high'][0] - dims['low'][0])
        with pytest.raises(EngineError, match='truncated sampler'):
            e.set_joint_posterior(dims, wb, far, np.full_like(sigb, 1e-3), wa, mua, siga)
        with pytest.raises(EngineError, match='truncated sampler'):
            e.joint_suggest(0, 24)
        with pytest.raises(EngineError, match='truncated sampler'):
            e.joint_draw(0, 24)
        with pytest.raises(ValueError):
            e.set_joint_posterior(dims, wb, mub, -sigb, wa, mua, siga)
        # and a good posterior replaces it
        e.set_joint_posterior(dims, wb, mub, sigb, wa, mua, siga)
        assert e.joint_suggest(0, 24)[1] >= 0
    finally:
        e.close()


# -- end to end -----------------------------------------------------------------
def e2e_space():
    return {'x': hp.uniform('x', -5, 5), 'y': hp.uniform('y', -5, 5), 'z': hp.lognormal('z', 0, 1),
            'q': hp.quniform('q', 0, 10, 2),
            'c': hp.choice('c', [{'kind': 'a', 'u': hp.uniform('u', 0, 1)}, {'kind': 'b'}])}


def e2e_loss(d):
    return (d['x'] - d['y']) ** 2 + 0.01 * (d['x'] + d['y']) ** 2 + 0.1 * np.log(d['z']) ** 2 + 0.01 * d['q']


def _run(multivariate, seed=5, evals=40):
    trials = H.Trials()
    H.fmin(e2e_loss, e2e_space(), algo=partial(tpe.suggest, multivariate=multivariate), max_evals=evals,
           trials=trials, rstate=np.random.RandomState(seed))
    return trials


def test_fmin_end_to_end():
    trials = _run(True)
    assert len(trials) == 40
    labels = {'x', 'y', 'z', 'q', 'c', 'u'}
    for doc in trials.trials:
        vals, idxs = doc['misc']['vals'], doc['misc']['idxs']
        assert set(vals) == set(idxs) == labels
        for k in ('x', 'y', 'z', 'q', 'c'):
            assert len(vals[k]) == 1 and idxs[k] == [doc['tid']]
        active = vals['c'][0] == 0
        assert len(vals['u']) == (1 if active else 0) and len(idxs['u']) == len(vals['u'])
        assert -5 <= vals['x'][0] < 5 and -5 <= vals['y'][0] < 5 and vals['z'][0] > 0
        assert 0 <= vals['q'][0] <= 10 and vals['q'][0] % 2 == 0
        if active:
            assert 0 <= vals['u'][0] < 1
        assert isinstance(vals['x'][0], float)
    again = _run(True)
    assert [d['misc']['vals'] for d in again.trials] == [d['misc']['vals'] for d in trials.trials]
    # the joint labels really come from the joint round
    plain = _run(False)
    assert [d['misc']['vals'] for d in plain.trials] != [d['misc']['vals'] for d in trials.trials]


def test_suggest_documents_given_the_same_history():
    """One history, three calls: multivariate=False before and after a
    multivariate call returns the same documents (and those of a call
    without the keyword); the multivariate call's non-group labels equal
    them, its group labels are the joint round's winner."""
    from hyperopt_amd.base import Domain
    from hyperopt_amd import engine as E, history, posterior as P
    trials = _run(False, seed=9, evals=30)
    domain = Domain(e2e_loss, e2e_space())
    ids = [100, 101, 102]
    kw = dict(batch=True, posterior_builder='host')
    before = tpe.suggest(ids, domain, trials, 17, multivariate=False, **kw)
    multi = tpe.suggest(ids, domain, trials, 17, multivariate=True, **kw)
    after = tpe.suggest(ids, domain, trials, 17, multivariate=False, **kw)
    default = tpe.suggest(ids, domain, trials, 17, **kw)
    vals = lambda docs: [d['misc']['vals'] for d in docs]
    assert vals(before) == vals(after) == vals(default)
    specs = tpe.specs_of(domain)
    labels = list(specs)
    tids, losses, obs = history.gather(domain, trials, labels)
    group = tpe.joint_group(domain, specs, obs)
    assert group == ['x', 'y', 'z']
    eng = E.get_engine(0, 'f64')
    eng.set_joint_posterior(*P.joint_mixture([specs[k] for k in group], obs, P.Splitter(tids, losses, 0.25),
                                             1.0, streams=[labels.index(k) for k in group]))
    for j, new_id in enumerate(ids):
        got, ref = multi[j]['misc']['vals'], before[j]['misc']['vals']
        for k in ('q', 'c', 'u'):
            assert got[k] == ref[k]
        win = eng.joint_suggest(17, 24, round=new_id)[0]
        assert [got[k][0] for k in group] == [float(v) for v in win]
    # through the device builder too
    dev = tpe.suggest(ids, domain, trials, 17, multivariate=True, batch=True, posterior_builder='device')
    assert vals(dev) == vals(multi)


def test_fallback_is_the_independent_call(caplog):
    from hyperopt_amd.base import Domain
    space = {'x': hp.uniform('x', -5, 5), 'q': hp.quniform('q', 0, 10, 2)}
    trials = H.Trials()
    H.fmin(lambda d: d['x'] ** 2 + d['q'], space, algo=tpe.suggest, max_evals=25, trials=trials,
           rstate=np.random.RandomState(1))
    domain = Domain(lambda d: 0.0, space)
    with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
        a = tpe.suggest([50], domain, trials, 3, multivariate=True)
    assert any('independent path' in r.message for r in caplog.records)
    b = tpe.suggest([50], domain, trials, 3)
    assert a[0]['misc']['vals'] == b[0]['misc']['vals']
