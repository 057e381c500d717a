"""Quantized hyperparameters in joint TPE groups on the GPU (`-m gpu`): the
joint score against the numpy definition (tests/joint_quant_reference.py),
the same bits in every layout, the quantized draw against the pointwise draw
reference, the fused round against its own draw and score entry points and
against numpy, the batch over a dense and a quantized slot, the new C call,
and tpe.suggest(..., multivariate=True, joint_quantized=True) end to end.
Groups, seeds and rounds: tests/joint_quant_cases.py (test_joint_quant_host.py
checks on the CPU that those seeds exclude no draw and leave every winner a
clear margin over every other configuration)."""
import ctypes
from functools import partial

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import hp, tpe
from oracle import draw_oracle as D
from tests import joint_cases as JC
from tests import joint_quant_cases as QC
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
    ref = QC.group(name)
    args, q = QC.engine_args(ref)
    eng.set_joint_posterior(*args, q=q)
    return ref


def _assert_lpdf(got, ref, what):
    """|err| <= 1e-9 max(1, |ref|) where the definition is finite; its -inf
    and NaN are matched exactly."""
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (what, got[~fin], ref[~fin])
    err = np.abs(got[fin] - ref[fin])
    bound = 1e-9 * np.maximum(1.0, np.abs(ref[fin]))
    print('%s: %d points, worst |err| / bound %.3g' % (what, len(ref), float(np.max(err / bound, initial=0.0))))
    bad = np.flatnonzero(~(err <= bound))
    assert len(bad) == 0, (what, bad[:5].tolist(), got[fin][bad[:5]].tolist(), ref[fin][bad[:5]].tolist())


def _empty_interval_point(ref, base):
    """`base` with one quantized dimension moved to a value whose interval
    is empty: past the upper bound of a bounded kind, negative for a log kind."""
    x = np.array(base, dtype=np.float64, copy=True)
    for d, dim in enumerate(ref.dims):
        if dim.q is None:
            continue
        if dim.bounded:
            top = np.exp(dim.high) if dim.log else dim.high
            x[d] = (np.rint(top / dim.q) + 3.0) * dim.q
            return x
        if dim.log:
            x[d] = -2.0 * dim.q
            return x
    raise AssertionError('no dimension with an empty interval')


# -- score --------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(QC.GROUPS))
def test_score_matches_definition(eng, name):
    """joint_score at grid corners, on component means, at 8-sigma outliers
    and at drawn candidates: |err| <= 1e-9 max(1, |ref|) on both lpdfs; a
    value with an empty interval scores -inf, a NaN scores NaN."""
    ref = _set(eng, name)
    pts = QC.fixed_points(ref, np.random.RandomState(1))
    drawn, _ = eng.joint_draw(77, 65, round=2)
    for what, vals in (('fixed', pts), ('drawn', drawn), ('one', drawn[:1])):
        ll, lg = eng.joint_score(vals)
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(lg))
        _assert_lpdf(ll, ref.joint_lpdf(vals, 'below'), '%s %s below' % (name, what))
        _assert_lpdf(lg, ref.joint_lpdf(vals, 'above'), '%s %s above' % (name, what))
    odd = np.stack([_empty_interval_point(ref, drawn[0]), np.full(ref.D, np.nan), drawn[1]])
    odd[1, :-1] = drawn[0, :-1]                    # one NaN value is enough
    ll, lg = eng.joint_score(odd)
    assert ll[0] == -np.inf and lg[0] == -np.inf
    assert np.isnan(ll[1]) and np.isnan(lg[1])
    _assert_lpdf(ll, ref.joint_lpdf(odd, 'below'), '%s odd below' % name)
    _assert_lpdf(lg, ref.joint_lpdf(odd, 'above'), '%s odd above' % name)


def test_fine_group_product_does_not_underflow(eng):
    """q60_fine: every component's product of factors is below 1e-320
    (test_joint_quant_host.py), the lpdfs are finite and in the bound."""
    ref = _set(eng, QC.FINE)
    pts = QC.fixed_points(ref, np.random.RandomState(1))
    ll, lg = eng.joint_score(pts)
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(lg)) and np.all(ll < -700.0)
    _assert_lpdf(ll, ref.joint_lpdf(pts, 'below'), 'fine below')


# -- layouts --------------------------------------------------------------------
def test_score_same_bits_in_every_layout(eng):
    """A candidate's lpdfs do not depend on how the round is laid out: scored
    among 100 (one workgroup per slice of components, merged by a second
    kernel), among 40000 (one workgroup per tile, all slices) and as the
    winner of a packed batch it has the same bits; and the round of 40000 is
    the argmax of its own draw and score."""
    name, seed, rnd, n, first = QC.LAYOUT
    ref = _set(eng, name)
    vals, idx = _round_check(eng, ref, seed, rnd, n)
    ll, lg = eng.joint_score(vals)
    ll2, lg2 = eng.joint_score(vals[:first])
    assert np.array_equal(ll[:first], ll2) and np.array_equal(lg[:first], lg2)
    rounds = [rnd, rnd + 1, rnd + 2]
    values, index, bl, bg = eng.joint_suggest_batch(seed, rounds, first)[0]
    for r, rr in enumerate(rounds):
        v, _ = eng.joint_draw(seed, first, round=rr)
        a, b = eng.joint_score(v)
        i = int(index[r])
        assert np.array_equal(values[r], v[i]) and bl[r] == a[i] and bg[r] == b[i]
        if rr == rnd:
            assert np.array_equal(a, ll[:first])


# -- draw ---------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(QC.DRAWS)))
def test_draws_match_reference(eng, case):
    name, seed, rnd, offset, n = QC.DRAWS[case]
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
            check_draws(ref.fold(int(k), d), wpd[sel], wud[sel], vals[sel, d],
                        'joint' if dim.q is None else 'joint_q', '%s dim %d component %d' % (name, d, k))


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
    # identical configurations have identical bits
    same = np.all(vals == vals[idx], axis=1)
    assert np.all(ll[same] == ll[idx]) and np.all(lg[same] == lg[idx])
    return vals, idx


@pytest.mark.parametrize('case', range(len(QC.ROUNDS)))
def test_round_is_argmax_of_draw_and_score(eng, case):
    """joint_suggest(n) is the first argmax of joint_score(joint_draw(n)),
    its values and lpdfs bit-identical to those calls; its configuration is
    that of numpy's argmax of the definition on the device's candidates (the
    reference's margin over every other configuration is above 1e-9 (|ll| +
    |lg|) in every round), at the lowest index that holds it."""
    name, seed, rnd, n = QC.ROUNDS[case]
    ref = _set(eng, name)
    vals, idx = _round_check(eng, ref, seed, rnd, n)
    ok, first = QC.margin_ok(vals, ref.joint_lpdf(vals, 'below'), ref.joint_lpdf(vals, 'above'))
    assert ok, 'reference margin too small: pick another seed'
    assert idx == first
    if name == QC.COARSE and n > 24:
        assert np.count_nonzero(np.all(vals == vals[idx], axis=1)) > 1    # a real tie


# -- batch ----------------------------------------------------------------------
def _set_two_slots(e):
    """Slot 0 dense-only, slot 1 quantized, both through set_joint_group(q=)."""
    e.clear_joint_groups()
    dense = QC.dense_group()
    e.set_joint_group(0, L.TPE_JOINT_STREAM, *JC.engine_args(dense), q=np.zeros(dense.D))
    args, q = QC.engine_args(QC.group('q9'))
    e.set_joint_group(1, L.TPE_JOINT_STREAM - 1, *args, q=q)


def _assert_batch_equals_single(e, rounds, n):
    got = e.joint_suggest_batch(19, rounds, n)
    assert sorted(got) == [0, 1]
    for slot in (0, 1):
        values, index, ll, lg = got[slot]
        for r, rnd in enumerate(rounds):
            v, i, a, b = e.joint_suggest(19, n, round=rnd, slot=slot)
            assert np.array_equal(values[r], v) and index[r] == i and ll[r] == a and lg[r] == b, (slot, r)
    return got


@pytest.mark.parametrize('n_rounds', [1, 24, 70])
def test_batch_equals_single_calls(eng, n_rounds):
    _set_two_slots(eng)
    rounds = [(7 * r + 3) % 101 for r in range(n_rounds)]
    got = _assert_batch_equals_single(eng, rounds, 24)
    q = QC.group('q9').steps
    v = got[1][0][:, q > 0]
    assert np.array_equal(np.rint(v / q[q > 0]) * q[q > 0], v)


def test_batch_chunked_under_a_low_cap():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    try:
        e.set_option('joint_cap', 100)
        _set_two_slots(e)
        rounds = [(7 * r + 3) % 101 for r in range(24)]
        got = _assert_batch_equals_single(e, rounds, 24)
        e.set_option('joint_cap', 0)
        whole = e.joint_suggest_batch(19, rounds, 24)
        for slot in got:
            for a, b in zip(got[slot], whole[slot]):
                assert np.array_equal(a, b)
    finally:
        e.close()


# -- ABI ------------------------------------------------------------------------
def test_zero_steps_give_the_dense_bits(eng):
    dense = QC.dense_group()
    args = JC.engine_args(dense)
    eng.clear_joint_groups()
    eng.set_joint_group(0, L.TPE_JOINT_STREAM, *args)
    vals, comp = eng.joint_draw(4, 300, round=2)
    ll, lg = eng.joint_score(vals)
    win = eng.joint_suggest(4, 300, round=2)
    for q in (np.zeros(dense.D), None):
        eng.clear_joint_groups()
        if q is None:
            eng.set_joint_posterior(*args, q=np.zeros(dense.D))
        else:
            eng.set_joint_group(0, L.TPE_JOINT_STREAM, *args, q=q)
        v2, c2 = eng.joint_draw(4, 300, round=2)
        l2, g2 = eng.joint_score(v2)
        w2 = eng.joint_suggest(4, 300, round=2)
        assert np.array_equal(vals, v2) and np.array_equal(comp, c2)
        assert np.array_equal(ll, l2) and np.array_equal(lg, g2)
        assert np.array_equal(win[0], w2[0]) and win[1:] == w2[1:]


def test_abi_errors():
    from hyperopt_amd.engine import Engine, EngineError
    e = Engine(0, 'f64')
    try:
        ref = QC.group('q2_mixed')
        (dims, wb, mub, sigb, wa, mua, siga), q = QC.engine_args(ref)

        def rc(dims, q, wb, mub, sigb, wa, mua, siga):
            q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
            keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (wb, mub, sigb, wa, mua, siga)]
            p = [a.ctypes.data for a in keep]
            return e.lib.tpe_joint_set_group(e.h, 0, L.TPE_JOINT_STREAM, dims.ctypes.data,
                                             q.ctypes.data if q is not None else None, None, None, 0.0, len(dims),
                                             len(wb), p[0], p[1], p[2], len(wa), p[3], p[4], p[5])
        assert rc(dims, q, wb, mub, sigb, wa, mua, siga) == L.TPE_OK
        assert rc(dims, None, wb, mub, sigb, wa, mua, siga) == L.TPE_OK
        for bad in (-1.0, np.nan, np.inf):
            assert rc(dims, [0.0, bad], wb, mub, sigb, wa, mua, siga) == L.TPE_ERR_ARG
        with pytest.raises(EngineError):
            e.set_joint_group(0, L.TPE_JOINT_STREAM, dims, wb, mub, sigb, wa, mua, siga, q=[0.0, -2.0])
        with pytest.raises(EngineError):
            e.joint_suggest(0, 24)                 # the refused call left the slot unset
        with pytest.raises(ValueError):
            e.set_joint_group(0, L.TPE_JOINT_STREAM, dims, wb, mub, sigb, wa, mua, siga, q=[1.0])
        # D + quantized dimensions: 64 + 64 = 128 is accepted, 65 + 64 is not
        for Dn, want in ((64, L.TPE_OK), (65, L.TPE_ERR_ARG)):
            big = np.zeros(Dn, dtype=dims.dtype)
            big['stream'] = np.arange(Dn)
            qq = np.where(np.arange(Dn) < 64, 0.5, 0.0)
            one = np.ones(1)
            assert rc(big, qq, one, np.zeros((1, Dn)), np.ones((1, Dn)), one, np.zeros((1, Dn)),
                      np.ones((1, Dn))) == want
        big = np.zeros(128, dtype=dims.dtype)
        big['stream'] = np.arange(128)
        one = np.ones(1)
        assert rc(big, np.zeros(128), one, np.zeros((1, 128)), np.ones((1, 128)), one, np.zeros((1, 128)),
                  np.ones((1, 128))) == L.TPE_OK
        qq = np.zeros(128)
        qq[5] = 1.0
        assert rc(big, qq, one, np.zeros((1, 128)), np.ones((1, 128)), one, np.zeros((1, 128)),
                  np.ones((1, 128))) == L.TPE_ERR_ARG
    finally:
        e.close()


# -- end to end -----------------------------------------------------------------
def e2e_space():
    return {'x': hp.uniform('x', -5, 5), 'q': hp.quniform('q', 0, 10, 2), 'n': hp.qloguniform('n', 0, 4, 2),
            'r': hp.randint('r', 3),
            'c': hp.choice('c', [{'kind': 'a', 'u': hp.uniform('u', 0, 1)}, {'kind': 'b'}])}


def e2e_loss(d):
    return (d['x'] - 0.5 * d['q']) ** 2 + 0.01 * (d['x'] + d['q']) ** 2 + 0.05 * (np.log(d['n'] + 1.0) - 2.0) ** 2 \
        + 0.01 * d['r']


def _run(seed=5, evals=40, space=None, loss=None, **kw):
    trials = H.Trials()
    H.fmin(loss or e2e_loss, space or e2e_space(), algo=partial(tpe.suggest, **kw), max_evals=evals,
           trials=trials, rstate=np.random.RandomState(seed))
    return trials


def _vals(docs):
    return [d['misc']['vals'] for d in docs]


def test_suggest_documents_given_the_same_history():
    """One history: joint_quantized=False before and after a True call
    returns the documents of a call without the keyword; the True call's group
    labels are Engine.joint_suggest's winner for the mixture
    joint_mixture(quantized=True) builds, on their grids; its other labels
    equal the independent documents."""
    from hyperopt_amd.base import Domain
    from hyperopt_amd import engine as E, history, posterior as P
    trials = _run(seed=9, evals=30)
    domain = Domain(e2e_loss, e2e_space())
    ids = [100, 101, 102]
    for extra in (dict(batch=True), dict(batch='pending')):
        kw = dict(posterior_builder='host', multivariate=True, **extra)
        before = tpe.suggest(ids, domain, trials, 17, joint_quantized=False, **kw)
        quant = tpe.suggest(ids, domain, trials, 17, joint_quantized=True, **kw)
        after = tpe.suggest(ids, domain, trials, 17, joint_quantized=False, **kw)
        default = tpe.suggest(ids, domain, trials, 17, **kw)
        assert _vals(before) == _vals(after) == _vals(default)
        assert _vals(quant) != _vals(before) and len(quant) == 3
        for doc in quant:
            v = doc['misc']['vals']
            assert v['q'][0] in (0.0, 2.0, 4.0, 6.0, 8.0, 10.0) and v['n'][0] % 2 == 0 and v['n'][0] >= 0
            assert isinstance(v['q'][0], float) and -5 <= v['x'][0] < 5
    kw = dict(posterior_builder='host', multivariate=True, batch=True)
    before = tpe.suggest(ids, domain, trials, 17, **kw)
    quant = tpe.suggest(ids, domain, trials, 17, joint_quantized=True, **kw)
    specs = tpe.specs_of(domain)
    labels = list(specs)
    tids, losses, obs = history.gather(domain, trials, labels)
    wide = P.JOINT_KINDS + P.JOINT_QUANT_KINDS
    assert tpe.joint_group(domain, specs, obs) is None
    group = tpe.joint_group(domain, specs, obs, wide)
    assert group == ['n', 'q', 'x']
    eng = E.get_engine(0, 'f64')
    mix = P.joint_mixture([specs[k] for k in group], obs, P.Splitter(tids, losses, 0.25), 1.0,
                          streams=[labels.index(k) for k in group], quantized=True)
    assert mix.q.tolist() == [2.0, 2.0, 0.0]
    eng.set_joint_posterior(*mix)
    for j, new_id in enumerate(ids):
        got, ref = quant[j]['misc']['vals'], before[j]['misc']['vals']
        for k in ('r', 'c', 'u'):
            assert got[k] == ref[k]
        win = eng.joint_suggest(17, 24, round=new_id)[0]
        assert [got[k][0] for k in group] == [float(v) for v in win]


def cond_space():
    return {'x': hp.uniform('x', -5, 5), 'w': hp.quniform('w', 1, 9, 1),
            'c': hp.choice('c', [{'u': hp.uniform('u', 0, 4), 'm': hp.quniform('m', 0, 4, 1)}, {'e': hp.uniform('e', 0, 1)}])}


def cond_loss(d):
    out = (d['x'] - d['w'] + 4.0) ** 2 * 0.1
    c = d['c']
    return float(out + ((c['u'] - c['m']) ** 2 if 'u' in c else 0.5 + c['e']))


def test_composes_with_group_on_a_conditional_space():
    from hyperopt_amd.base import Domain
    trials = _run(seed=3, evals=30, space=cond_space(), loss=cond_loss)
    domain = Domain(cond_loss, cond_space())
    specs = tpe.specs_of(domain)
    from hyperopt_amd import posterior as P
    wide = P.JOINT_KINDS + P.JOINT_QUANT_KINDS
    assert tpe.joint_groups(domain, specs) == []
    assert tpe.joint_groups(domain, specs, None, wide) == [(0, ['w', 'x']), (1, ['m', 'u'])]
    ids = [60, 61, 62, 63]
    kw = dict(multivariate=True, group=True, batch=True)
    plain = tpe.suggest(ids, domain, trials, 11, **kw)
    quant = tpe.suggest(ids, domain, trials, 11, joint_quantized=True, **kw)
    again = tpe.suggest(ids, domain, trials, 11, joint_quantized=True, **kw)
    assert _vals(quant) == _vals(again) and _vals(quant) != _vals(plain)
    assert _vals(plain) == _vals(tpe.suggest(ids, domain, trials, 11, batch=True))
    for a, b in zip(quant, plain):
        v, p = a['misc']['vals'], b['misc']['vals']
        assert v['c'] == p['c'] and v['e'] == p['e']
        assert v['w'][0] in range(1, 10)
        assert len(v['m']) == len(v['u']) == (1 if v['c'][0] == 0 else 0)
        if v['m']:
            assert v['m'][0] in range(0, 5) and 0 <= v['u'][0] < 4


def test_fmin_end_to_end():
    kw = dict(multivariate=True, joint_quantized=True)
    trials = _run(**kw)
    assert len(trials) == 40
    for doc in trials.trials:
        v = doc['misc']['vals']
        assert v['q'][0] % 2 == 0 and 0 <= v['q'][0] <= 10 and v['n'][0] % 2 == 0
    again = _run(**kw)
    assert _vals(again.trials) == _vals(trials.trials)
    plain = _run(multivariate=True)
    assert _vals(plain.trials) != _vals(trials.trials)
