"""Joint groups built on the device from the resident history (`-m gpu`):
Engine.build_joint_groups against posterior.joint_mixture on the same history
-- Engine.joint_get_group with np.array_equal on both sides, no tolerance (the
joint mixture is the univariate build's, which is numpy's bit for bit) -- and
the batched round of the device-built slot against a host-set slot's, bit for
bit; which groups the device flags (every tie-free case must come back
unflagged); the C ABI's errors; and tpe.suggest(multivariate=True) with
posterior_builder='device' against 'host', document for document."""
import collections

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import history as history_mod
from hyperopt_amd import hp, tpe
from hyperopt_amd import posterior as P
from hyperopt_amd.base import Domain
from hyperopt_amd.engine import EngineError
from tests import joint_group_cases as GC

pytestmark = pytest.mark.gpu

GAMMA, PW = 0.25, 1.0
SEED, ROUNDS, N_CAND = 23, [3, 0, 4294967295, 11], 24
HOST = 32          # slot s + HOST holds the host-built mixture of slot s, on the same pick stream
Spec = collections.namedtuple('Spec', 'label kind args')


class Owner(object):
    """Stands for the history cache a device view belongs to."""


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


ARGS = {'uniform': dict(low=-5.0, high=5.0), 'loguniform': dict(low=-3.0, high=2.0),
        'normal': dict(mu=1.0, sigma=2.0), 'lognormal': dict(mu=0.0, sigma=1.0),
        'quniform': dict(low=0.0, high=4000.0, q=2.0), 'randint': dict(upper=5)}


def draw(kind, args, n, rng):
    """n tie-free raw values of a label (a quantized one: distinct grid values)."""
    if kind == 'uniform':
        return rng.uniform(args['low'], args['high'], n)
    if kind == 'loguniform':
        return np.exp(rng.uniform(args['low'], args['high'], n))
    if kind == 'normal':
        return args['mu'] + args['sigma'] * rng.randn(n)
    if kind == 'lognormal':
        return np.exp(args['mu'] + args['sigma'] * rng.randn(n))
    if kind == 'quniform':
        grid = np.arange(int(args['low'] / args['q']), int(args['high'] / args['q']) + 1)
        pick = rng.permutation(grid)[:n] if len(grid) >= n else rng.choice(grid, n)   # (too few: ties)
        return pick * args['q']
    return rng.randint(0, args['upper'], n).astype(float)


def dense_specs(kinds):
    return collections.OrderedDict(('h%d' % d, Spec('h%d' % d, k, ARGS[k])) for d, k in enumerate(kinds))


def make_view(specs, n, seed, owner=None, active=None):
    """A device view (history.HistoryCache.device_view's tuple) of n trials:
    distinct losses, every label observed in every trial (or where
    active[label] says)."""
    rng = np.random.RandomState(seed)
    tids = np.arange(n, dtype=np.int64) * 2 + 1
    losses = rng.permutation(n).astype(np.float64) * 0.5 - 3.0
    cols = {}
    for k, s in specs.items():
        v = np.asarray(draw(s.kind, s.args, n, rng), dtype=np.float64)
        on = np.ones(n, dtype=bool) if active is None else active[k]
        cols[k] = (tids[on], v[on])
    return tids, losses, n, cols, owner or Owner()


def grow_view(view, specs, n, seed):
    """`view` with trials appended up to n (the columns keep their prefix)."""
    tids, losses, _, cols, owner = view
    more = make_view(specs, n, seed, owner)
    m = len(tids)
    new_losses = np.concatenate([losses, 1000.0 + np.arange(m, n)])   # (distinct; the new trials go above)
    new_cols = {k: (np.concatenate([cols[k][0], more[3][k][0][m:]]),
                    np.concatenate([cols[k][1], more[3][k][1][m:]])) for k in cols}
    return more[0], new_losses, n, new_cols, owner


def check(eng, up, specs, view, groups, quantized=False, categorical=False, want_flags=None):
    """Build the univariate posterior of `view` on the device (the uploader,
    tie orders included), the joint groups [(slot, [labels])] from it in one
    build_joint_groups call, and compare every unflagged slot with
    posterior.joint_mixture and with the host-set slot + HOST.  want_flags:
    per group the expected flag word (default: none set).  Returns the flags."""
    names = list(specs)
    table = [(s.label, s.kind, s.args) for s in specs.values()]
    up.build(eng, table, view, GAMMA, PW)
    args, kw = tpe._joint_device_args(specs, names, groups, quantized, categorical, PW)
    assert [(a[0], a[1]) for a in args] == [(slot, L.TPE_JOINT_STREAM - slot) for slot, _ in groups]
    eng.clear_joint_groups()
    flags = eng.build_joint_groups(args, **kw)
    want = [0] * len(groups) if want_flags is None else list(want_flags)
    assert list(flags) == want, 'device flags %r, expected %r' % (list(flags), want)
    tids, losses, _, cols, _ = view
    splitter = P.Splitter(tids, losses, GAMMA)
    built = []
    for (slot, g), f in zip(groups, flags):
        if f:
            with pytest.raises(EngineError):
                eng.joint_get_group(slot, 0)
            continue
        mix = P.joint_mixture([specs[k] for k in g], cols, splitter, PW, streams=[names.index(k) for k in g],
                              quantized=quantized, categorical=categorical)
        eng.set_joint_group(slot + HOST, L.TPE_JOINT_STREAM - slot, *mix, prior_weight=PW)
        for side in (0, 1):
            ref = (mix.wa, mix.mua, mix.siga) if side else (mix.wb, mix.mub, mix.sigb)
            for where in (slot, slot + HOST):
                got = eng.joint_get_group(where, side)
                for name, a, b in zip(('W', 'mu', 'sigma'), got, ref):
                    assert a.shape == np.asarray(b).shape, (where, side, name)
                    assert np.array_equal(a, b), (where, side, name)
        built.append(slot)
    if built:
        won = eng.joint_suggest_batch(SEED, ROUNDS, N_CAND)
        assert sorted(won) == sorted(built + [s + HOST for s in built])
        for slot in built:
            for a, b in zip(won[slot], won[slot + HOST]):
                assert np.array_equal(a, b), slot
    return flags


# -- the contract over shapes ---------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 26, 30, 300])
def test_two_labels(eng, n):
    """uniform + loguniform: an above side that is the prior alone (n = 1),
    n_above on both sides of the 25-trial linear-forgetting ramp (26: 24
    above, 30: 28 above), more rows than one workgroup (300)."""
    specs = dense_specs(['uniform', 'loguniform'])
    check(eng, P.DeviceHistoryUploader(), specs, make_view(specs, n, 100 + n), [(0, list(specs))])


def test_four_kinds_2000_trials(eng):
    """The four dense kinds at N = 2000: several grid strides, 1988 above components."""
    specs = dense_specs(['uniform', 'loguniform', 'normal', 'lognormal'])
    check(eng, P.DeviceHistoryUploader(), specs, make_view(specs, 2000, 7), [(0, list(specs))])


@pytest.mark.parametrize('D', [9, 33])
def test_past_the_register_instantiations(eng, D):
    kinds = ['uniform', 'loguniform', 'normal', 'lognormal']
    specs = dense_specs([kinds[d % 4] for d in range(D)])
    check(eng, P.DeviceHistoryUploader(), specs, make_view(specs, 40, 200 + D), [(0, list(specs))])


@pytest.mark.parametrize('where', ['below_all', 'above_all', 'between', 'on_one'])
@pytest.mark.parametrize('n', [3, 40])
def test_prior_position(eng, where, n):
    """A normal label whose prior_mu sorts first, last, in the middle, and
    exactly on an observation (np.searchsorted left: the prior goes first;
    a side's only observation goes before the prior, as the reference's
    n = 1 branch puts it) -- on either side, at n = 40 and with the
    one-observation below side of n = 3."""
    specs = dense_specs(['normal', 'uniform'])
    view = make_view(specs, n, 300 + n)
    tids, v = view[3]['h0']
    v = np.abs(v - 1.0) + 0.5                   # distinct, all above 0.5
    s = np.sort(v)
    mu = {'below_all': 0.25, 'above_all': s[-1] + 1.0, 'between': 0.5 * (s[n // 2] + s[n // 2 + 1])}.get(where)
    if mu is None:   # exactly the best trial's observation: the below side's only one at n = 3
        mu = float(v[np.argmin(view[1])])
    view[3]['h0'] = (tids, v)
    specs['h0'] = Spec('h0', 'normal', dict(mu=float(mu), sigma=2.0))
    check(eng, P.DeviceHistoryUploader(), specs, view, [(0, list(specs))])
    if where == 'on_one':   # the losses reversed: the same observation now on the above side
        view[1][:] = -view[1]
        check(eng, P.DeviceHistoryUploader(), specs, view, [(0, list(specs))])


def conditional_case(n, seed, never_inner, c0_not_below):
    """A history of joint_group_cases.space(): (domain, specs, view)."""
    domain = Domain(GC.loss, GC.space())
    specs = tpe.specs_of(domain)
    rng = np.random.RandomState(seed)
    c = rng.randint(0, 2, n)
    inner = np.zeros(n, dtype=int) if never_inner else rng.randint(0, 2, n)
    k = rng.randint(0, 3, n)
    active = {'x': c >= 0, 'ly': c >= 0, 'c': c >= 0, 'k': c >= 0, 'a': c == 0, 'b': c == 0, 'qa': c == 0,
              'inner': c == 0, 'd1': (c == 0) & (inner == 1), 'd2': (c == 0) & (inner == 1), 'e': c == 1,
              'sh': k < 2}
    assert set(active) == set(specs)
    flat = collections.OrderedDict((name, Spec(name, s.kind, s.args)) for name, s in specs.items())
    view = make_view(flat, n, seed + 1, active=active)
    for name, col in (('c', c), ('inner', inner), ('k', k)):
        view[3][name] = (view[3][name][0], col[active[name]].astype(np.float64))
    if c0_not_below:   # every trial of branch c = 0 loses to every trial of c = 1
        view[1][:] = view[1] + 1000.0 * (c == 0)
    return domain, specs, view


@pytest.mark.parametrize('never_inner,c0_not_below', [(False, False), (True, True)])
def test_conditional_groups(eng, never_inner, c0_not_below):
    """joint_group_cases.space() with group=True, all groups in one call, in
    the slots tpe.suggest gives them: groups observed in subsets of the
    trials; (second case) the branch c = 0 without a below trial and the
    group (d1, d2) never observed."""
    domain, specs, view = conditional_case(60, 11, never_inner, c0_not_below)
    groups = tpe.joint_groups(domain, specs, view[3])
    assert groups == GC.GROUPS
    n_d = len(view[3]['d1'][0])
    assert (n_d == 0) == never_inner and 0 < len(view[3]['a'][0]) < 60
    check(eng, P.DeviceHistoryUploader(), specs, view, groups)
    if c0_not_below:
        assert eng.joint_get_group(1, 0)[0].shape == (1,)                  # the prior alone below
        assert eng.joint_get_group(2, 0)[0].shape == eng.joint_get_group(2, 1)[0].shape == (1,)


def test_resident_appends_and_regrow(eng):
    """One uploader: a first upload, then appends of one trial each, rebuilt
    and compared every time, across the pool's regrow (its capacity after the
    first upload of 127 observations per label is 256)."""
    specs = dense_specs(['loguniform', 'normal', 'uniform'])
    up = P.DeviceHistoryUploader()
    view = make_view(specs, 127, 5)
    gen = eng.history_generation
    check(eng, up, specs, view, [(0, list(specs))])
    resets = eng.history_generation
    assert resets > gen
    for n in (128, 255, 256, 257, 258):
        view = grow_view(view, specs, n, 5)
        check(eng, up, specs, view, [(0, list(specs))])
    assert eng.history_generation == resets, 'the uploader reset the history instead of appending'


def test_mixed_categorical_group(eng):
    specs = collections.OrderedDict([('lr', Spec('lr', 'loguniform', ARGS['loguniform'])),
                                     ('opt', Spec('opt', 'randint', ARGS['randint'])),
                                     ('pc', Spec('pc', 'categorical', dict(upper=3, p=[0.2, 0.5, 0.3])))])
    view = make_view(specs, 60, 21)
    check(eng, P.DeviceHistoryUploader(), specs, view, [(0, list(specs))], categorical=True)
    # quantized and categorical keywords together, a dense label last
    specs2 = collections.OrderedDict([('opt', specs['opt']), ('lr', specs['lr'])])
    check(eng, P.DeviceHistoryUploader(), specs2, make_view(specs2, 60, 22), [(0, list(specs2))], quantized=True,
          categorical=True)


def test_mixed_quantized_group(eng):
    """uniform + quniform, the quantized column distinct grid values."""
    specs = dense_specs(['uniform', 'quniform'])
    view = make_view(specs, 60, 31)
    assert len(set(view[3]['h1'][1])) == 60
    check(eng, P.DeviceHistoryUploader(), specs, view, [(0, list(specs))], quantized=True)


# -- ties ------------------------------------------------------------------------------------
def tie_view(specs, n, seed, side):
    """Label h0 with two equal values, both on `side` (0 below, 1 above)."""
    view = make_view(specs, n, seed)
    order = np.argsort(view[1])
    n_below = P.n_below_of(n, GAMMA)
    pair = order[:2] if side == 0 else order[n_below + 1:n_below + 3]
    assert n_below >= 2
    view[3]['h0'][1][pair[1]] = view[3]['h0'][1][pair[0]]
    return view


def test_tie_below_is_flagged(eng):
    specs = dense_specs(['uniform', 'normal'])
    check(eng, P.DeviceHistoryUploader(), specs, tie_view(specs, 40, 41, 0), [(0, list(specs))],
          want_flags=[L.TPE_JOINT_FLAG_TIE])


def test_tie_above_without_an_order_is_flagged(eng):
    """n_above = 18 <= 25: the weights are equal, the univariate mixture does
    not depend on the tie order and is built without one -- which trial gets
    which sigma does."""
    specs = dense_specs(['uniform', 'normal'])
    flags = check(eng, P.DeviceHistoryUploader(), specs, tie_view(specs, 20, 42, 1), [(0, list(specs))],
                  want_flags=[L.TPE_JOINT_FLAG_TIE])
    assert list(flags) == [1]


def test_tie_above_with_the_supplied_order_is_built(eng):
    """n_above = 58 > 25: the univariate build reports the tie, gets numpy's
    order and rebuilds the label with it -- the joint build follows that
    order: unflagged, the host's bits.  A second group without the tie is
    untouched by it."""
    specs = dense_specs(['uniform', 'normal', 'lognormal', 'uniform'])
    up = P.DeviceHistoryUploader()
    view = tie_view(specs, 60, 43, 1)
    check(eng, up, specs, view, [(0, ['h0', 'h1']), (1, ['h2', 'h3'])])
    assert up.tie_labels == frozenset([0])
    # the next call supplies the known label's order with the first build
    check(eng, up, specs, grow_view(view, specs, 61, 43), [(0, ['h0', 'h1']), (1, ['h2', 'h3'])])


def test_flagged_group_leaves_the_others_built(eng):
    specs = dense_specs(['uniform', 'normal', 'lognormal', 'uniform'])
    check(eng, P.DeviceHistoryUploader(), specs, tie_view(specs, 40, 44, 0), [(0, ['h0', 'h1']), (3, ['h2', 'h3'])],
          want_flags=[L.TPE_JOINT_FLAG_TIE, 0])


def test_labels_with_different_side_counts_are_flagged(eng):
    """(tpe.suggest never sends such a group: its labels are observed in the
    same trials.)  h1 misses one above trial: the count flag, the other
    group built."""
    specs = dense_specs(['uniform', 'normal', 'lognormal', 'uniform'])
    view = make_view(specs, 40, 45)
    worst = int(np.argmax(view[1]))
    keep = np.arange(40) != worst
    view[3]['h1'] = (view[3]['h1'][0][keep], view[3]['h1'][1][keep])
    check(eng, P.DeviceHistoryUploader(), specs, view, [(0, ['h0', 'h1']), (1, ['h2', 'h3'])],
          want_flags=[L.TPE_JOINT_FLAG_COUNT, 0])


# -- errors ------------------------------------------------------------------------------------
def test_errors():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    try:
        specs = collections.OrderedDict([('u', Spec('u', 'uniform', ARGS['uniform'])),
                                         ('n', Spec('n', 'normal', ARGS['normal'])),
                                         ('c', Spec('c', 'randint', ARGS['randint'])),
                                         ('d', Spec('d', 'randint', ARGS['randint']))])
        table = [(s.label, s.kind, s.args) for s in specs.values()]
        one = [(0, L.TPE_JOINT_STREAM, [0, 1], [0, 1])]
        with pytest.raises(EngineError, match='no current build'):
            e.build_joint_groups(one)
        up = P.DeviceHistoryUploader()
        view = make_view(specs, 30, 51)
        up.build(e, table, view, GAMMA, PW)
        assert list(e.build_joint_groups(one)) == [0]
        for bad in ([0, 4], [0, -1]):
            with pytest.raises(EngineError, match='out of range'):
                e.build_joint_groups([(0, L.TPE_JOINT_STREAM, bad, bad)])
        with pytest.raises(EngineError, match='listed twice'):
            e.build_joint_groups([(0, L.TPE_JOINT_STREAM, [0, 0], [0, 0])])
        with pytest.raises(EngineError, match='listed twice'):
            e.build_joint_groups([(0, L.TPE_JOINT_STREAM, [0, 1], [0, 1]), (1, L.TPE_JOINT_STREAM - 1, [1], [1])])
        cat = dict(upper=[[5, 5]], cat_p=[np.full(10, 0.2)], prior_weight=PW)
        with pytest.raises(EngineError, match='not categorical'):
            e.build_joint_groups([(0, L.TPE_JOINT_STREAM, [2, 3], [2, 3])], **cat)
        with pytest.raises(EngineError, match='slots are distinct'):
            e.build_joint_groups([(0, L.TPE_JOINT_STREAM, [0], [0]), (0, L.TPE_JOINT_STREAM, [1], [1])])
        with pytest.raises(EngineError, match="label's categories"):
            e.build_joint_groups([(0, L.TPE_JOINT_STREAM, [0, 2], [0, 2])],
                                 upper=[[0, 4]], cat_p=[np.full(4, 0.25)], prior_weight=PW)
        with pytest.raises(EngineError, match='no joint posterior set'):
            e.joint_get_group(5, 0)
        # a stale generation: the history moved on since the build
        e.history_append(np.array([1, 1, 1, 1], dtype=np.int64), np.full(4, 30, dtype=np.int32),
                         np.array([0.5, 0.25, 1.0, 2.0]))
        with pytest.raises(EngineError, match='no current build'):
            e.build_joint_groups(one)
        # an observed category outside [0, upper): flagged, the slot unset, nothing raised
        view = make_view(specs, 30, 52)
        view[3]['c'][1][7] = 5.0
        up = P.DeviceHistoryUploader()
        up.build(e, table, view, GAMMA, PW)
        e.clear_joint_groups()
        flags = e.build_joint_groups([(0, L.TPE_JOINT_STREAM, [0, 2], [0, 2]), (1, L.TPE_JOINT_STREAM - 1, [1, 3], [1, 3])],
                                     upper=[[0, 5], [0, 5]], cat_p=[np.full(5, 0.2), np.full(5, 0.2)], prior_weight=PW)
        assert list(flags) == [L.TPE_JOINT_FLAG_CATEGORY, 0]
        assert sorted(e.joint_slots) == [1]
        with pytest.raises(EngineError):
            e.joint_get_group(0, 1)
    finally:
        e.close()


# -- tpe.suggest end to end ---------------------------------------------------------------------
def e2e_space():
    return {'lr': hp.loguniform('lr', -6, 0), 'mom': hp.uniform('mom', 0, 1),
            'width': hp.quniform('width', 8, 512, 8),
            'opt': hp.choice('opt', [{'kind': 0, 'a': hp.uniform('a', -2, 2), 'b': hp.normal('b', 0, 1)},
                                     {'kind': 1}])}


def e2e_loss(d):
    out = (np.log(d['lr']) + 3.0) ** 2 * 0.1 + (d['mom'] - 0.6) ** 2 + 1e-5 * (d['width'] - 200.0) ** 2
    if 'a' in d['opt']:
        out += (d['opt']['a'] - d['opt']['b']) ** 2 * 0.3
    else:
        out += 0.4
    return float(out)


def _vals(docs):
    return [d['misc']['vals'] for d in docs]


MODES = [dict(), dict(group=True), dict(group=True, joint_quantized=True),
         dict(group=True, joint_quantized=True, joint_categorical=True), dict(batch=True, group=True),
         dict(batch='pending', group=True)]


def test_suggest_device_equals_host_along_a_run():
    """45 trials on a small conditional space: n_above crosses the 25-trial
    ramp, the quantized label ties.  At every step past startup the documents
    of posterior_builder='device' and 'host' are identical in every mode."""
    compared = []

    def algo(new_ids, domain, trials, seed):
        if len(trials.trials) >= 20:
            for mode in MODES:
                ids = [new_ids[0] + j for j in range(3)] if mode.get('batch') else list(new_ids)
                got = [_vals(tpe.suggest(ids, domain, trials, seed, multivariate=True, posterior_builder=b, **mode))
                       for b in ('device', 'host')]
                assert got[0] == got[1], (len(trials.trials), mode)
                assert len(got[0]) == len(ids)
            compared.append(len(trials.trials))
        return tpe.suggest(new_ids, domain, trials, seed, multivariate=True, group=True, posterior_builder='device')
    trials = H.Trials()
    H.fmin(e2e_loss, e2e_space(), algo=algo, max_evals=45, trials=trials, rstate=np.random.RandomState(5))
    assert len(trials) == 45 and compared == list(range(20, 45))


def test_suggest_device_path_does_not_gather(monkeypatch, caplog):
    """A dense tie-free history: with posterior.joint_mixture and
    history.gather made to raise, the 'device' call still answers -- and
    answers what the 'host' call does."""
    import logging
    space = {'x': hp.uniform('x', -5, 5), 'ly': hp.loguniform('ly', -3, 2), 'z': hp.normal('z', 0, 1)}

    def loss(d):
        return float(0.1 * d['x'] ** 2 + np.log(d['ly']) ** 2 + (d['z'] - 0.3) ** 2)
    trials = H.Trials()
    H.fmin(loss, space, algo=H.rand.suggest, max_evals=40, trials=trials, rstate=np.random.RandomState(3))
    domain = Domain(loss, space)
    host = _vals(tpe.suggest([100, 101], domain, trials, 9, multivariate=True, batch=True,
                             posterior_builder='host'))

    def refuse(*a, **k):
        raise AssertionError('the device path reached the host build')
    monkeypatch.setattr(P, 'joint_mixture', refuse)
    monkeypatch.setattr(history_mod, 'gather', refuse)
    with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
        dev = _vals(tpe.suggest([100, 101], domain, trials, 9, multivariate=True, batch=True,
                                posterior_builder='device'))
    assert dev == host
    assert any('1 group(s) built on the device, 0 on the host' in r.getMessage() for r in caplog.records)
