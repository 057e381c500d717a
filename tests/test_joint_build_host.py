"""Which joint groups tpe.suggest(multivariate=True) builds on the device and
which on the host, decided without a GPU against a stub engine: the groups
with a label that is not categorical go to one Engine.build_joint_groups call
when the call's posterior came from the resident history; a flagged group, a
group of categorical labels alone and every group of a host-built call go
through posterior.joint_mixture + set_joint_group; and the "observed in the
same trials" test on the view's columns decides what it decides on the
gathered observations."""
import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import history, hp, tpe
from hyperopt_amd import posterior as P
from hyperopt_amd.base import Domain
from hyperopt_amd.engine import RESULT_DTYPE


def space():
    return {'x': hp.uniform('x', -5, 5), 'ly': hp.loguniform('ly', -3, 2), 'o': hp.randint('o', 4),
            'c': hp.choice('c', [{'a': hp.uniform('a', -2, 2), 'b': hp.normal('b', 0, 1)},
                                 {'r1': hp.randint('r1', 3), 'r2': hp.randint('r2', 5)}])}


def loss(d):
    out = 0.05 * d['x'] ** 2 + np.log(d['ly']) ** 2 + 0.1 * d['o']
    c = d['c']
    return float(out + ((c['a'] - c['b']) ** 2 if 'a' in c else 0.3 + 0.1 * c['r1'] + 0.05 * c['r2']))


class StubEngine(object):
    """Records the joint calls of tpe._joint_rounds; `flags` is what
    build_joint_groups answers (default: nothing flagged)."""
    devices = (0,)

    def __init__(self, flags=None):
        self.flags, self.calls, self.D = flags, [], {}

    def clear_joint_groups(self):
        self.calls.append(('clear',))
        self.D = {}

    def build_joint_groups(self, groups, q=None, upper=None, cat_p=None, prior_weight=None):
        self.calls.append(('build', [tuple(g) for g in groups], q, upper, cat_p, prior_weight))
        flags = np.zeros(len(groups), dtype=np.int32) if self.flags is None else np.asarray(self.flags, dtype=np.int32)
        assert len(flags) == len(groups)
        for g, f in zip(groups, flags):
            if not f:
                self.D[g[0]] = len(g[2])
        return flags

    def set_joint_group(self, slot, pick_stream, dims, wb, mub, sigb, wa, mua, siga, q=None, upper=None, cat_p=None,
                        prior_weight=None):
        self.calls.append(('set', slot, pick_stream, (wb, mub, sigb, wa, mua, siga)))
        self.D[slot] = len(dims)

    def joint_suggest_batch(self, seed, rounds, n_candidates):
        R = len(rounds)
        return {slot: (np.full((R, D), 0.5), np.zeros(R, dtype=np.int64), np.zeros(R), np.zeros(R))
                for slot, D in sorted(self.D.items())}

    def of(self, what):
        return [c for c in self.calls if c[0] == what]


@pytest.fixture(scope='module')
def case():
    trials = H.Trials()
    H.fmin(loss, space(), algo=H.rand.suggest, max_evals=30, trials=trials, rstate=np.random.RandomState(4))
    domain = Domain(loss, space())
    specs = tpe.specs_of(domain)
    labels = list(specs)
    view = history.device_view(domain, trials, labels)
    assert view is not None
    return domain, trials, specs, labels, view


def rounds(eng, case, view, **kw):
    domain, trials, specs, labels, _ = case
    return tpe._joint_rounds(eng, domain, trials, specs, None, 0.25, 1.0, 7, [50, 51], 24, view=view, **kw)


def refuse(*a, **k):
    raise AssertionError('the host build ran')


def test_groups_with_a_continuous_label_go_to_the_device(case, monkeypatch):
    domain, trials, specs, labels, view = case
    monkeypatch.setattr(history, 'gather', refuse)
    monkeypatch.setattr(P, 'joint_mixture', refuse)
    eng = StubEngine()
    out = rounds(eng, case, view, group=True)
    assert [c[0] for c in eng.calls] == ['clear', 'build']
    groups = tpe.joint_groups(domain, specs, view[3])
    assert [g for _, g in groups] == [['ly', 'x'], ['a', 'b']]
    want = [(slot, L.TPE_JOINT_STREAM - slot, [labels.index(k) for k in g], [labels.index(k) for k in g])
            for slot, g in groups]
    assert eng.of('build')[0][1] == want
    assert eng.of('build')[0][2:] == (None, None, None, None)
    assert len(out) == 2 and set(out[0]) == {'ly', 'x', 'a', 'b'}
    # group=False: the unconditional group alone, slot 0
    eng = StubEngine()
    rounds(eng, case, view)
    assert eng.of('build')[0][1] == want[:1]


def test_steps_and_categories_travel_with_the_device_call(case, monkeypatch):
    domain, trials, specs, labels, view = case
    monkeypatch.setattr(history, 'gather', refuse)
    eng = StubEngine()
    rounds(eng, case, view, quantized=True, categorical=True)
    _, groups, q, upper, cat_p, pw = eng.of('build')[0]
    names = [labels[i] for i in groups[0][2]]
    assert sorted(names) == ['c', 'ly', 'o', 'x']
    assert list(q[0]) == [0.0] * 4
    assert list(upper[0]) == [{'c': 2, 'o': 4}.get(k, 0) for k in names]
    assert np.array_equal(cat_p[0], np.concatenate([np.full(u, 1.0 / u) for u in upper[0] if u]))
    assert pw == 1.0


def test_a_flagged_group_is_built_on_the_host(case):
    domain, trials, specs, labels, view = case
    eng = StubEngine(flags=[0, L.TPE_JOINT_FLAG_TIE])
    out = rounds(eng, case, view, group=True)
    assert [c[0] for c in eng.calls] == ['clear', 'build', 'set']
    _, slot, pick, arrays = eng.of('set')[0]
    assert (slot, pick) == (1, L.TPE_JOINT_STREAM - 1)
    tids, losses, obs = history.gather(domain, trials, labels)
    mix = P.joint_mixture([specs['a'], specs['b']], obs, P.Splitter(tids, losses, 0.25), 1.0,
                          streams=[labels.index('a'), labels.index('b')])
    for got, ref in zip(arrays, (mix.wb, mix.mub, mix.sigb, mix.wa, mix.mua, mix.siga)):
        assert np.array_equal(got, ref)
    assert set(out[0]) == {'ly', 'x', 'a', 'b'}


def test_a_group_of_categorical_labels_alone_is_built_on_the_host(case):
    domain, trials, specs, labels, view = case
    eng = StubEngine()
    rounds(eng, case, view, group=True, categorical=True)
    groups = tpe.joint_groups(domain, specs, view[3], P.JOINT_KINDS + P.JOINT_CAT_KINDS)
    by_labels = {tuple(g): slot for slot, g in groups}
    assert ('r1', 'r2') in by_labels
    built = [labels[g[2][0]] for g in eng.of('build')[0][1]]
    assert len(built) == len(groups) - 1 and 'r1' not in built
    assert [c[1] for c in eng.of('set')] == [by_labels[('r1', 'r2')]]


def test_without_a_view_every_group_is_built_on_the_host(case):
    eng = StubEngine()
    rounds(eng, case, None, group=True)
    assert [c[0] for c in eng.calls] == ['clear', 'set', 'set']
    assert [c[1] for c in eng.of('set')] == [0, 1]


@pytest.mark.parametrize('builder,resident,device', [('host', False, False), ('device', True, True),
                                                     ('device', False, False), ('auto', True, True)])
def test_suggest_takes_the_device_path_only_behind_a_resident_build(case, monkeypatch, builder, resident, device):
    """tpe.suggest hands the view to the joint rounds when its univariate
    posterior was built on the device from the resident history -- not with
    posterior_builder='host', nor when that build fell back to the host."""
    domain, trials, specs, labels, view = case
    eng = StubEngine()
    monkeypatch.setattr(tpe._engine, 'get_engine', lambda *a, **k: eng)

    def fake_posterior(eng_, domain_, trials_, specs_, view_, gathered, gamma, pw, builder_, info=None, **kw):
        assert (view_ is None) == (builder_ == 'host')
        if resident:
            info['resident'] = True
        return 30, np.zeros((1, len(specs_)), dtype=RESULT_DTYPE)
    monkeypatch.setattr(tpe, '_resident_posterior', fake_posterior)
    docs = tpe.suggest([60], domain, trials, 3, multivariate=True, group=True, posterior_builder=builder)
    assert len(docs) == 1
    assert bool(eng.of('build')) == device and bool(eng.of('set')) == (not device)


def test_same_trials_check_on_view_columns_and_gathered_observations():
    """A document without y breaks the group on both paths; when that
    document has a NaN loss the gather drops it, and so must the view's
    columns: the group stands on both paths."""
    sp = {'x': hp.uniform('x', -5, 5), 'y': hp.normal('y', 0, 1)}

    def f(d):
        return float(d['x'] ** 2 + d['y'] ** 2)
    for nan in (False, True):
        trials = H.Trials()
        H.fmin(f, sp, algo=H.rand.suggest, max_evals=25, trials=trials, rstate=np.random.RandomState(8))
        doc = trials.trials[6]
        doc['misc']['idxs']['y'], doc['misc']['vals']['y'] = [], []
        if nan:
            doc['result']['loss'] = float('nan')
        domain = Domain(f, sp)
        specs = tpe.specs_of(domain)
        labels = list(specs)
        view = history.device_view(domain, trials, labels)
        cols = tpe._view_columns(view)
        obs = history.gather(domain, trials, labels)[2]
        for k in labels:
            assert np.array_equal(cols[k][0], obs[k][0]) and np.array_equal(cols[k][1], obs[k][1])
        want = ['x', 'y'] if nan else None
        assert tpe.joint_group(domain, specs, obs) == want
        assert tpe.joint_group(domain, specs, cols) == want
        assert tpe.joint_groups(domain, specs, cols) == tpe.joint_groups(domain, specs, obs) == \
            ([(0, ['x', 'y'])] if nan else [])
