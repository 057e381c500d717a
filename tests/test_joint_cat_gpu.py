"""Categorical labels in joint TPE groups on the GPU (`-m gpu`): the joint
score against the numpy definition (tests/joint_cat_reference.py), the same
bits in every layout, the categorical draw against the pointwise draw
reference, the fused round against its own draw and score entry points and
against numpy, the batch over a dense and a categorical slot, the new C call,
and tpe.suggest(..., multivariate=True, joint_categorical=True) end to end.
Groups, seeds and rounds: tests/joint_cat_cases.py (test_joint_cat_host.py
checks on the CPU that those seeds exclude no draw and leave every winner a
clear margin over every other configuration).

Accuracy observed on an MI355X (worst |err| / bound over the fixed, drawn and
single points of test_score_matches_definition, bound 1e-9 max(1, |ref|)):
see DESIGN.md section 6b, "Categorical labels in joint groups"."""
from functools import partial

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import hp, tpe
from oracle import draw_oracle as D
from tests import joint_cases as JC
from tests import joint_cat_cases as CC
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
    ref = CC.group(name)
    args, kw = CC.engine_args(ref)
    eng.set_joint_posterior(*args, **kw)
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


# -- score --------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CC.GROUPS))
def test_score_matches_definition(eng, name):
    """joint_score at every category corner, on component categories, at
    drawn candidates and at a single point: |err| <= 1e-9 max(1, |ref|) on both
    lpdfs; an out-of-range and a non-integer category score -inf on both
    sides, a NaN scores NaN."""
    ref = _set(eng, name)
    pts = CC.fixed_points(ref, np.random.RandomState(1))
    drawn, _ = eng.joint_draw(77, 65, round=2)
    for what, vals in (('fixed', pts), ('drawn', drawn), ('one', drawn[:1])):
        ll, lg = eng.joint_score(vals)
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(lg))
        _assert_lpdf(ll, ref.joint_lpdf(vals, 'below'), '%s %s below' % (name, what))
        _assert_lpdf(lg, ref.joint_lpdf(vals, 'above'), '%s %s above' % (name, what))
    cat = int(np.flatnonzero(ref.uppers)[-1])
    odd = np.stack([drawn[0]] * 5 + [drawn[1]])
    odd[0, cat] = ref.uppers[cat]           # one past the last category
    odd[1, cat] = -1.0
    odd[2, cat] = 0.5
    odd[3, cat] = np.nan
    odd[4, cat] = np.inf
    ll, lg = eng.joint_score(odd)
    for i in (0, 1, 2, 4):
        assert ll[i] == -np.inf and lg[i] == -np.inf, (i, ll[i], lg[i])
    assert np.isnan(ll[3]) and np.isnan(lg[3])
    _assert_lpdf(ll, ref.joint_lpdf(odd, 'below'), '%s odd below' % name)
    _assert_lpdf(lg, ref.joint_lpdf(odd, 'above'), '%s odd above' % name)


# -- layouts --------------------------------------------------------------------
def test_score_same_bits_in_every_layout(eng):
    """A candidate's lpdfs do not depend on how the round is laid out: scored
    among 100 (one workgroup per slice of components, merged by a second
    kernel), among 40000 (one workgroup per tile, all slices) and as the
    winner of a packed batch it has the same bits; and the round of 40000 is
    the argmax of its own draw and score."""
    name, seed, rnd, n, first = CC.LAYOUT
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
@pytest.mark.parametrize('case', range(len(CC.DRAWS)))
def test_draws_match_reference(eng, case):
    name, seed, rnd, offset, n = CC.DRAWS[case]
    ref = _set(eng, name)
    vals, comp = eng.joint_draw(seed, n, round=rnd, cand_offset=offset)
    g = offset + np.arange(n, dtype=np.uint64)
    pf = ref.pick_fold()
    wp, wu = D.draw_words(seed, JR.JOINT_STREAM, rnd, g)
    assert not D.excluded(pf, wp, wu).any()
    assert np.array_equal(comp, D.pick(pf, wp)), name
    for d, dim in enumerate(ref.dims):
        wpd, wud = D.draw_words(seed, dim.stream, rnd, g, categorical=bool(dim.upper))
        path = 'joint_c' if dim.upper else ('joint' if dim.q is None else 'joint_q')
        for k in np.unique(comp):
            sel = comp == k
            check_draws(ref.fold(int(k), d), wpd[sel], wud[sel], vals[sel, d], path,
                        '%s dim %d component %d' % (name, d, k))


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


@pytest.mark.parametrize('case', range(len(CC.ROUNDS)))
def test_round_is_argmax_of_draw_and_score(eng, case):
    """joint_suggest(n) is the first argmax of joint_score(joint_draw(n)),
    its values and lpdfs bit-identical to those calls; its configuration is
    that of numpy's argmax of the definition on the device's candidates, at
    the lowest index that holds it -- in the all-categorical group among
    real ties."""
    name, seed, rnd, n = CC.ROUNDS[case]
    ref = _set(eng, name)
    vals, idx = _round_check(eng, ref, seed, rnd, n)
    ok, first = CC.margin_ok(vals, ref.joint_lpdf(vals, 'below'), ref.joint_lpdf(vals, 'above'))
    assert ok, 'reference margin too small: pick another seed'
    assert idx == first
    if name == CC.ALL_CAT and n > 24:
        assert np.count_nonzero(np.all(vals == vals[idx], axis=1)) > 1    # a real tie
        assert idx == int(np.flatnonzero(np.all(vals == vals[idx], axis=1))[0])


# -- batch ----------------------------------------------------------------------
def _set_two_slots(e):
    """Slot 0 dense-only, slot 1 with categorical dimensions."""
    e.clear_joint_groups()
    dense = JC.group('d5_k300')
    e.set_joint_group(0, L.TPE_JOINT_STREAM, *JC.engine_args(dense))
    args, kw = CC.engine_args(CC.group('c9'))
    e.set_joint_group(1, L.TPE_JOINT_STREAM - 1, *args, **kw)


def _assert_batch_equals_single(e, rounds, n):
    got = e.joint_suggest_batch(19, rounds, n)
    assert sorted(got) == [0, 1]
    for slot in (0, 1):
        values, index, ll, lg = got[slot]
        for r, rnd in enumerate(rounds):
            v, i, a, b = e.joint_suggest(19, n, round=rnd, slot=slot)
            assert np.array_equal(values[r], v) and index[r] == i and ll[r] == a and lg[r] == b, (slot, r)
    return got


@pytest.mark.parametrize('n_rounds', [1, 24])
def test_batch_equals_single_calls(eng, n_rounds):
    _set_two_slots(eng)
    rounds = [(7 * r + 3) % 101 for r in range(n_rounds)]
    got = _assert_batch_equals_single(eng, rounds, 24)
    up = CC.group('c9').uppers
    v = got[1][0][:, up > 0]
    assert np.array_equal(np.floor(v), v) and np.all(v >= 0) and np.all(v < up[up > 0])


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
def test_zero_uppers_give_the_quantized_bits(eng):
    from tests import joint_quant_cases as QC
    ref = QC.group('q9')
    args, q = QC.engine_args(ref)
    eng.clear_joint_groups()
    eng.set_joint_group(0, L.TPE_JOINT_STREAM, *args, q=q)
    vals, comp = eng.joint_draw(4, 300, round=2)
    ll, lg = eng.joint_score(vals)
    win = eng.joint_suggest(4, 300, round=2)
    for how in ('group', 'posterior'):
        eng.clear_joint_groups()
        if how == 'group':
            eng.set_joint_group(0, L.TPE_JOINT_STREAM, *args, q=q, upper=np.zeros(ref.D, dtype=np.int32))
        else:
            eng.set_joint_posterior(*args, q=q, upper=np.zeros(ref.D, dtype=np.int32), cat_p=[], prior_weight=1.0)
        v2, c2 = eng.joint_draw(4, 300, round=2)
        l2, g2 = eng.joint_score(v2)
        w2 = eng.joint_suggest(4, 300, round=2)
        assert np.array_equal(vals, v2) and np.array_equal(comp, c2)
        assert np.array_equal(ll, l2) and np.array_equal(lg, g2)
        assert np.array_equal(win[0], w2[0]) and win[1:] == w2[1:]
    # and without steps: the dense group's bits
    dense = JC.group('d5_k300')
    dargs = JC.engine_args(dense)
    eng.clear_joint_groups()
    eng.set_joint_group(0, L.TPE_JOINT_STREAM, *dargs)
    w1 = eng.joint_suggest(4, 300, round=2)
    eng.clear_joint_groups()
    eng.set_joint_group(0, L.TPE_JOINT_STREAM, *dargs, upper=np.zeros(dense.D, dtype=np.int32))
    w2 = eng.joint_suggest(4, 300, round=2)
    assert np.array_equal(w1[0], w2[0]) and w1[1:] == w2[1:]
    # all-zero steps together with all-zero uppers, as every dense group is set: the bits of neither
    small = JC.group('d2')
    sargs = JC.engine_args(small)
    eng.clear_joint_groups()
    eng.set_joint_group(0, L.TPE_JOINT_STREAM, *sargs)
    w1 = eng.joint_suggest(4, 300, round=2)
    eng.clear_joint_groups()
    eng.set_joint_group(0, L.TPE_JOINT_STREAM, *sargs, q=np.zeros(small.D), upper=np.zeros(small.D, dtype=np.int32),
                        cat_p=np.zeros(0), prior_weight=1.0)
    w2 = eng.joint_suggest(4, 300, round=2)
    assert np.array_equal(w1[0], w2[0]) and w1[1:] == w2[1:]


def test_abi_errors():
    from hyperopt_amd.engine import Engine, EngineError
    e = Engine(0, 'f64')
    try:
        ref = CC.group('c2_mixed')
        (dims, wb, mub, sigb, wa, mua, siga), kw = CC.engine_args(ref)

        def rc(dims, q, upper, cat_p, pw, wb, mub, sigb, wa, mua, siga):
            q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
            upper = None if upper is None else np.ascontiguousarray(upper, dtype=np.int32)
            cat_p = None if cat_p is None else np.ascontiguousarray(cat_p, dtype=np.float64)
            keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (wb, mub, sigb, wa, mua, siga)]
            p = [a.ctypes.data for a in keep]
            return e.lib.tpe_joint_set_group(e.h, 0, L.TPE_JOINT_STREAM, dims.ctypes.data,
                                             q.ctypes.data if q is not None else None,
                                             upper.ctypes.data if upper is not None else None,
                                             cat_p.ctypes.data if cat_p is not None and len(cat_p) else None,
                                             float(pw), len(dims), len(wb), p[0], p[1], p[2], len(wa), p[3], p[4],
                                             p[5])
        mix = (wb, mub, sigb, wa, mua, siga)
        up, p4 = [0, 4], [0.25] * 4
        assert rc(dims, None, up, p4, 1.0, *mix) == L.TPE_OK
        assert rc(dims, [0.0, 0.0], up, p4, 1.0, *mix) == L.TPE_OK
        assert rc(dims, None, None, None, 0.0, *mix) == L.TPE_OK                 # upper NULL: the dense group
        assert rc(dims, None, [0, 0], None, 0.0, *mix) == L.TPE_OK
        assert rc(dims, None, [0, -1], p4, 1.0, *mix) == L.TPE_ERR_ARG
        assert rc(dims, [0.0, 0.5], up, p4, 1.0, *mix) == L.TPE_ERR_ARG          # quantized and categorical
        for bad in (0.0, -0.25, np.nan, np.inf):
            assert rc(dims, None, up, [0.25, 0.25, 0.25, bad], 1.0, *mix) == L.TPE_ERR_ARG
        assert rc(dims, None, up, [0.25, 0.25, 0.25, 0.25 + 1e-8], 1.0, *mix) == L.TPE_ERR_ARG
        assert rc(dims, None, up, [0.25, 0.25, 0.25, 0.25 + 1e-11], 1.0, *mix) == L.TPE_OK
        for bad in (4.0, -1.0, 1.5, np.nan):
            m2 = np.array(mub, copy=True)
            m2[1, 1] = bad
            assert rc(dims, None, up, p4, 1.0, wb, m2, sigb, wa, mua, siga) == L.TPE_ERR_ARG
            m2 = np.array(mua, copy=True)
            m2[1, 1] = bad
            assert rc(dims, None, up, p4, 1.0, wb, mub, sigb, wa, m2, siga) == L.TPE_ERR_ARG
        m2 = np.array(mub, copy=True)
        m2[0, 1] = np.nan                        # row 0 and the sigmas of a categorical dimension are not read
        s2 = np.array(sigb, copy=True)
        s2[:, 1] = -1.0
        assert rc(dims, None, up, p4, 1.0, wb, m2, s2, wa, mua, siga) == L.TPE_OK
        for bad in (0.0, -1.0, np.nan, np.inf):
            assert rc(dims, None, up, p4, bad, *mix) == L.TPE_ERR_ARG
        with pytest.raises(EngineError):
            e.set_joint_group(0, L.TPE_JOINT_STREAM, dims, *mix, upper=[0, -1], cat_p=[], prior_weight=1.0)
        with pytest.raises(EngineError):
            e.joint_suggest(0, 24)                 # the refused call left the slot unset
        with pytest.raises(ValueError):
            e.set_joint_group(0, L.TPE_JOINT_STREAM, dims, *mix, upper=[4], cat_p=p4, prior_weight=1.0)
        with pytest.raises(ValueError):
            e.set_joint_group(0, L.TPE_JOINT_STREAM, dims, *mix, upper=up, cat_p=p4[:3], prior_weight=1.0)
        # 33 categorical dimensions are accepted and run
        big = CC.group('c33_cat')
        args, kw = CC.engine_args(big)
        e.set_joint_group(0, L.TPE_JOINT_STREAM, *args, **kw)
        v, i, a, b = e.joint_suggest(3, 24, round=1)
        assert np.all((v >= 0) & (v < big.uppers) & (v == np.floor(v))) and np.isfinite(a) and np.isfinite(b)
        # the budget: D + quantized dimensions <= 128, a categorical dimension counting 1
        for nq, want in ((32, L.TPE_OK), (33, L.TPE_ERR_ARG)):
            Dn = 96
            bd = np.zeros(Dn, dtype=dims.dtype)
            bd['stream'] = np.arange(Dn)
            qq = np.where(np.arange(Dn) < nq, 0.5, 0.0)
            uu = np.where(np.arange(Dn) >= 64, 2, 0)
            one = np.ones(1)
            assert rc(bd, qq, uu, np.full(64, 0.5), 1.0, one, np.zeros((1, Dn)), np.ones((1, Dn)), one,
                      np.zeros((1, Dn)), np.ones((1, Dn))) == want
        Dn = 128
        bd = np.zeros(Dn, dtype=dims.dtype)
        bd['stream'] = np.arange(Dn)
        one = np.ones(1)
        assert rc(bd, None, np.full(Dn, 2), np.full(2 * Dn, 0.5), 1.0, one, np.zeros((1, Dn)), np.ones((1, Dn)), one,
                  np.zeros((1, Dn)), np.ones((1, Dn))) == L.TPE_OK
    finally:
        e.close()


# -- end to end -----------------------------------------------------------------
def e2e_space():
    return {'lr': hp.loguniform('lr', -7, 0), 'opt': hp.choice('opt', ['sgd', 'adam', 'rms']),
            'n': hp.quniform('n', 1, 9, 1), 'r': hp.randint('r', 3),
            'z': hp.pchoice('z', [(0.5, 'a'), (0.5, 'b'), (0.0, 'c')]),
            'c': hp.choice('c', [{'kind': 'a', 'u': hp.uniform('u', 0, 1)}, {'kind': 'b'}])}


_BEST_LR = {'sgd': -1.0, 'adam': -5.0, 'rms': -3.0}


def e2e_loss(d):
    return (np.log(d['lr']) - _BEST_LR[d['opt']]) ** 2 + 0.05 * (d['n'] - 4.0) ** 2 + 0.01 * d['r']


def _run(seed=5, evals=40, space=None, loss=None, **kw):
    trials = H.Trials()
    H.fmin(loss or e2e_loss, space or e2e_space(), algo=partial(tpe.suggest, **kw), max_evals=evals,
           trials=trials, rstate=np.random.RandomState(seed))
    return trials


def _vals(docs):
    return [d['misc']['vals'] for d in docs]


def test_suggest_documents_given_the_same_history():
    """One 40-trial history: joint_categorical=False before and after a True
    call returns the documents of a call without the keyword; the True call's
    (lr, opt, n) are Engine.joint_suggest_batch's winners for the mixture
    joint_mixture(quantized=True, categorical=True) builds, opt an int in
    range; its other labels (z, whose zero probability keeps it out, and u
    inside a branch) are bit for bit the multivariate=False values;
    batch=True with 3 ids equals three single calls."""
    from hyperopt_amd.base import Domain
    from hyperopt_amd import engine as E, history, posterior as P
    trials = _run(seed=9, evals=40)
    domain = Domain(e2e_loss, e2e_space())
    ids = [100, 101, 102]
    kw = dict(posterior_builder='host', multivariate=True, joint_quantized=True, batch=True)
    before = tpe.suggest(ids, domain, trials, 17, joint_categorical=False, **kw)
    cat = tpe.suggest(ids, domain, trials, 17, joint_categorical=True, **kw)
    after = tpe.suggest(ids, domain, trials, 17, joint_categorical=False, **kw)
    default = tpe.suggest(ids, domain, trials, 17, **kw)
    indep = tpe.suggest(ids, domain, trials, 17, posterior_builder='host', batch=True)
    assert _vals(before) == _vals(after) == _vals(default)
    assert _vals(cat) != _vals(before) and len(cat) == 3
    single = [tpe.suggest([i], domain, trials, 17, joint_categorical=True, **dict(kw, batch=False))[0] for i in ids]
    assert _vals(single) == _vals(cat)
    specs = tpe.specs_of(domain)
    labels = list(specs)
    tids, losses, obs = history.gather(domain, trials, labels)
    wide = P.JOINT_KINDS + P.JOINT_QUANT_KINDS + P.JOINT_CAT_KINDS
    group = tpe.joint_group(domain, specs, obs, wide)
    assert sorted(group) == ['c', 'lr', 'n', 'opt', 'r']
    eng = E.get_engine(0, 'f64')
    mix = P.joint_mixture([specs[k] for k in group], obs, P.Splitter(tids, losses, 0.25), 1.0,
                          streams=[labels.index(k) for k in group], quantized=True, categorical=True)
    eng.set_joint_posterior(*mix, prior_weight=1.0)
    values = eng.joint_suggest_batch(17, ids, 24)[0][0]
    for j in range(3):
        got, ref = cat[j]['misc']['vals'], indep[j]['misc']['vals']
        win = dict(zip(group, values[j]))
        opt = got['opt'][0]
        assert isinstance(opt, int) and 0 <= opt < 3 and opt == win['opt']
        assert got['lr'][0] == float(win['lr']) and got['n'][0] == float(win['n']) and got['n'][0] in range(1, 10)
        assert isinstance(got['r'][0], int) and got['r'][0] == win['r'] and got['c'][0] == win['c']
        assert got['z'] == ref['z']                         # outside every group: the independent round's bits
        if got['c'][0] == ref['c'][0]:
            assert got['u'] == ref['u']
        assert len(got['u']) == (1 if got['c'][0] == 0 else 0)


def cond_space():
    return {'x': hp.uniform('x', -5, 5),
            'o': hp.choice('o', [{'k': hp.choice('k', ['a', 'b', 'c']), 'u': hp.uniform('u', 0, 4)},
                                 {'e': hp.uniform('e', 0, 1)}])}


def cond_loss(d):
    o = d['o']
    if 'u' in o:
        return float(0.1 * d['x'] ** 2 + (o['u'] - {'a': 1.0, 'b': 2.0, 'c': 3.0}[o['k']]) ** 2)
    return float(0.1 * d['x'] ** 2 + 0.5 + o['e'])


def test_composes_with_group_on_a_conditional_space():
    from hyperopt_amd.base import Domain
    trials = _run(seed=3, evals=30, space=cond_space(), loss=cond_loss)
    domain = Domain(cond_loss, cond_space())
    ids = [60, 61, 62, 63]
    kw = dict(multivariate=True, group=True, batch=True)
    plain = tpe.suggest(ids, domain, trials, 11, **kw)
    cat = tpe.suggest(ids, domain, trials, 11, joint_categorical=True, **kw)
    again = tpe.suggest(ids, domain, trials, 11, joint_categorical=True, **kw)
    assert _vals(cat) == _vals(again) and _vals(cat) != _vals(plain)
    assert _vals(plain) == _vals(tpe.suggest(ids, domain, trials, 11, batch=True))
    for doc in cat:
        v = doc['misc']['vals']
        assert v['o'][0] in (0, 1) and isinstance(v['o'][0], int) and -5 <= v['x'][0] < 5
        inside = 1 if v['o'][0] == 0 else 0
        assert len(v['k']) == len(v['u']) == inside and len(v['e']) == 1 - inside
        if inside:
            assert v['k'][0] in (0, 1, 2) and isinstance(v['k'][0], int) and 0 <= v['u'][0] < 4


def test_fmin_end_to_end():
    kw = dict(multivariate=True, joint_categorical=True, joint_quantized=True)
    trials = _run(**kw)
    assert len(trials) == 40
    for doc in trials.trials:
        v = doc['misc']['vals']
        assert v['opt'][0] in (0, 1, 2) and v['n'][0] in range(1, 10)
    again = _run(**kw)
    assert _vals(again.trials) == _vals(trials.trials)
    plain = _run(multivariate=True, joint_quantized=True)
    assert _vals(plain.trials) != _vals(trials.trials)
