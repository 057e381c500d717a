"""posterior.joint_mixture(bandwidth='scott') without a GPU: equal, by
np.array_equal, to the plain-loop restatement of the rule in
tests/joint_bandwidth_reference.py for every label kind a group takes, at the
side sizes where a path changes (the lower clip at n = 1 and 2, the
linear-forgetting ramp from 26 trials, the block edges 8 / 9 and 128 / 129 of
numpy's pairwise sum); what the rule promises of its arrays; the default
untouched; and the keyword's errors, tpe.suggest's included."""
import collections

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from hyperopt_amd import hp, tpe
from hyperopt_amd import posterior as P
from hyperopt_amd.base import Domain
from tests import joint_bandwidth_reference as R

PW = 1.0
SIZES = [0, 1, 2, 7, 8, 9, 25, 26, 127, 128, 129, 300]
Spec = collections.namedtuple('Spec', 'label kind args')

ARGS = {'uniform': dict(low=-5.0, high=5.0), 'loguniform': dict(low=-3.0, high=2.0),
        'normal': dict(mu=1.0, sigma=2.0), 'lognormal': dict(mu=0.0, sigma=1.0),
        'quniform': dict(low=0.0, high=40.0, q=2.0),      # 21 grid values: ties from 22 trials at the latest
        'randint': dict(upper=5)}                          # (hp.choice's index label)
GROUPS = collections.OrderedDict([
    ('uniform_loguniform', ['uniform', 'loguniform']),
    ('normal_lognormal', ['normal', 'lognormal']),
    ('uniform_quniform', ['uniform', 'quniform']),
    ('choice_loguniform', ['randint', 'loguniform']),
    ('five', ['uniform', 'loguniform', 'normal', 'lognormal', 'quniform']),
])


def specs_of(kinds):
    return collections.OrderedDict(('h%d' % d, Spec('h%d' % d, k, ARGS[k])) for d, k in enumerate(kinds))


def draw(kind, args, n, rng):
    if kind == 'uniform':
        return rng.uniform(args['low'], args['high'], n)
    if kind == 'loguniform':
        return np.exp(rng.uniform(args['low'], args['high'], n))
    if kind == 'normal':
        return args['mu'] + args['sigma'] * rng.randn(n)
    if kind == 'lognormal':
        return np.exp(args['mu'] + args['sigma'] * rng.randn(n))
    if kind == 'quniform':
        return rng.randint(0, int(args['high'] / args['q']) + 1, n) * args['q']
    return rng.randint(0, args['upper'], n).astype(float)


def history(specs, n, seed):
    """(tids, losses, columns) of n trials: distinct losses, every label
    observed in every trial."""
    rng = np.random.RandomState(seed)
    tids = np.arange(n, dtype=np.int64) * 2 + 1
    losses = rng.permutation(n).astype(np.float64) * 0.5 - 3.0
    cols = collections.OrderedDict((k, (tids, np.asarray(draw(s.kind, s.args, n, rng), dtype=np.float64)))
                                   for k, s in specs.items())
    return tids, losses, cols


class FirstBelow(object):
    """A splitter with the side sizes a test asks for: the first n_below
    observations below, the others above (joint_mixture asks a splitter for
    nothing but split)."""

    def __init__(self, n_below):
        self.n_below = n_below

    def split(self, o_idxs, o_vals):
        o_vals = np.asarray(o_vals)
        return o_vals[:self.n_below], o_vals[self.n_below:]


def reference(specs, cols, splitter):
    """Both sides by the restatement: ((W, mu, sigma) below, (...) above)."""
    group = [(s.kind, s.args) for s in specs.values()]
    split = [splitter.split(*cols[k]) for k in specs]
    out = []
    for side in (0, 1):
        columns = [np.asarray(sp[side], dtype=np.float64) for sp in split]
        rows = [[c[t] for c in columns] for t in range(len(columns[0]))]
        out.append(R.side(group, rows, PW))
    return out


def assert_equal(mix, ref):
    got = ((mix.wb, mix.mub, mix.sigb), (mix.wa, mix.mua, mix.siga))
    for side in (0, 1):
        for name, a, b in zip(('W', 'mu', 'sigma'), got[side], ref[side]):
            assert np.asarray(a).shape == b.shape, (side, name)
            assert np.array_equal(a, b), (side, name)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', list(GROUPS))
def test_scott_equals_the_restated_rule(name, n):
    """Both sides with n trials each (the first n below, the next n above)."""
    specs = specs_of(GROUPS[name])
    _, _, cols = history(specs, 2 * n, 1000 + n)
    if 'quniform' in GROUPS[name] and n >= 25:
        v = cols['h%d' % GROUPS[name].index('quniform')][1]
        assert len(set(v[:n])) < n and len(set(v[n:])) < n      # tied observations on both sides
    sp = FirstBelow(n)
    mix = P.joint_mixture(list(specs.values()), cols, sp, PW, quantized=True, categorical=True, bandwidth='scott')
    assert_equal(mix, reference(specs, cols, sp))
    D = len(specs)
    assert mix.mub.shape == mix.sigb.shape == (n + 1, D) and mix.wa.shape == (n + 1,)


def test_scott_with_the_history_split():
    """The real Splitter: 300 trials, 5 below and 295 above in loss order."""
    specs = specs_of(GROUPS['five'])
    tids, losses, cols = history(specs, 300, 5)
    sp = P.Splitter(tids, losses, 0.25)
    mix = P.joint_mixture(list(specs.values()), cols, sp, PW, quantized=True, bandwidth='scott')
    assert len(mix.wb) == 6 and len(mix.wa) == 296
    assert_equal(mix, reference(specs, cols, sp))


@pytest.mark.parametrize('n', SIZES)
def test_what_the_rule_promises(n):
    specs = specs_of(GROUPS['five'])
    _, _, cols = history(specs, 2 * n, 2000 + n)
    mix = P.joint_mixture(list(specs.values()), cols, FirstBelow(n), PW, quantized=True, bandwidth='scott')
    K, D = n + 1, len(specs)
    for W, mu, sig in ((mix.wb, mix.mub, mix.sigb), (mix.wa, mix.mua, mix.siga)):
        assert abs(float(np.sum(W)) - 1.0) <= K * np.finfo(np.float64).eps
        for d, s in enumerate(specs.values()):
            _, psig, _, _ = R.prior(s.kind, s.args)
            assert sig[0, d] == psig
            if n:
                assert np.all(sig[1:, d] == sig[1, d])           # one sigma per (side, dimension)
                assert psig / min(100.0, 1.0 + K) <= sig[1, d] <= psig
        if n == 1:                                               # the lower clip: prior_sigma / 3
            assert all(sig[1, d] == sig[0, d] / 3.0 for d in range(D))
        if n == 300:                                             # past the clip: the factor itself
            assert all(sig[1, d] == R.factor(n, D) * sig[0, d] for d in range(D))


def test_a_label_with_every_observation_equal_builds():
    specs = specs_of(['uniform', 'loguniform'])
    _, _, cols = history(specs, 60, 7)
    cols['h0'] = (cols['h0'][0], np.full(60, 1.25))
    sp = FirstBelow(20)
    mix = P.joint_mixture(list(specs.values()), cols, sp, PW, bandwidth='scott')
    assert_equal(mix, reference(specs, cols, sp))
    assert np.all(mix.mua[1:, 0] == 1.25) and np.all(mix.siga > 0.0)


@pytest.mark.parametrize('name', list(GROUPS))
def test_neighbour_is_the_call_without_the_keyword(name):
    specs = specs_of(GROUPS[name])
    tids, losses, cols = history(specs, 90, 11)
    if 'quniform' in GROUPS[name]:   # (tie-free, as the neighbour rule's weight assertion wants them)
        k = 'h%d' % GROUPS[name].index('quniform')
        cols[k] = (tids, np.random.RandomState(3).permutation(90)[:90] * 2.0)
        specs[k] = Spec(k, 'quniform', dict(low=0.0, high=400.0, q=2.0))
    sp = P.Splitter(tids, losses, 0.25)
    kw = dict(quantized=True, categorical=True)
    plain = P.joint_mixture(list(specs.values()), cols, sp, PW, **kw)
    named = P.joint_mixture(list(specs.values()), cols, sp, PW, bandwidth='neighbour', **kw)
    for a, b in zip(plain, named):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    scott = P.joint_mixture(list(specs.values()), cols, sp, PW, bandwidth='scott', **kw)
    assert not np.array_equal(scott.siga, plain.siga)
    for f in ('dims', 'q', 'upper', 'cat_p'):                    # the mode touches W and sigma alone
        assert np.array_equal(getattr(scott, f), getattr(plain, f))
    assert np.array_equal(scott.mua, plain.mua) and np.array_equal(scott.mub, plain.mub)


def test_keyword_errors():
    assert P.JOINT_BANDWIDTHS == ('neighbour', 'scott')
    assert (L.TPE_JOINT_BW_NEIGHBOUR, L.TPE_JOINT_BW_SCOTT) == (0, 1)
    specs = specs_of(['uniform', 'normal'])
    _, _, cols = history(specs, 10, 1)
    with pytest.raises(ValueError, match='bandwidth'):
        P.joint_mixture(list(specs.values()), cols, FirstBelow(3), PW, bandwidth='silverman')
    space = {'x': hp.uniform('x', -5, 5), 'y': hp.normal('y', 0, 1)}
    domain = Domain(lambda d: d['x'] ** 2 + d['y'] ** 2, space)
    import hyperopt_amd as H
    with pytest.raises(ValueError, match='multivariate=True'):
        tpe.suggest([0], domain, H.Trials(), 1, joint_bandwidth='scott')
    with pytest.raises(ValueError, match='joint_bandwidth'):
        tpe.suggest([0], domain, H.Trials(), 1, multivariate=True, joint_bandwidth='silverman')


def test_factor():
    assert P.joint_bandwidth_factor(0, 3) == P.joint_bandwidth_factor(1, 3) == 0.2
    assert P.joint_bandwidth_factor(16, 0) == 0.1                # 16^(-1/4) = 1/2
    for n in (2, 9, 300, 9976):
        for D in (2, 5, 32):
            assert P.joint_bandwidth_factor(n, D) == R.factor(n, D)


class StubEngine(object):
    """The joint calls of tpe._joint_rounds, recorded."""
    devices = (0,)

    def __init__(self):
        self.calls, self.D = [], {}

    def clear_joint_groups(self):
        self.D = {}

    def build_joint_groups(self, groups, **kw):
        self.calls.append(('build', kw))
        for g in groups:
            self.D[g[0]] = len(g[2])
        return np.zeros(len(groups), dtype=np.int32)

    def set_joint_group(self, slot, pick_stream, *mix, **kw):
        self.calls.append(('set', mix))
        self.D[slot] = len(mix[0])

    def joint_suggest_batch(self, seed, rounds, n_candidates):
        R_ = len(rounds)
        return {slot: (np.full((R_, D), 0.5), np.zeros(R_, dtype=np.int64), np.zeros(R_), np.zeros(R_))
                for slot, D in sorted(self.D.items())}


def test_joint_rounds_hand_the_mode_to_both_builders(caplog):
    import logging
    import hyperopt_amd as H
    from hyperopt_amd import history as history_mod
    space = {'x': hp.uniform('x', -5, 5), 'ly': hp.loguniform('ly', -3, 2)}

    def loss(d):
        return float(d['x'] ** 2 + np.log(d['ly']) ** 2)
    trials = H.Trials()
    H.fmin(loss, space, algo=H.rand.suggest, max_evals=30, trials=trials, rstate=np.random.RandomState(4))
    domain = Domain(loss, space)
    specs = tpe.specs_of(domain)
    labels = list(specs)
    view = history_mod.device_view(domain, trials, labels)
    for v in (view, None):
        for bw in ('scott', 'neighbour'):
            eng = StubEngine()
            caplog.clear()
            with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
                tpe._joint_rounds(eng, domain, trials, specs, None, 0.25, PW, 7, [50], 24, view=v, bandwidth=bw)
            assert any(('%s bandwidth' % bw) in r.getMessage() for r in caplog.records)
            (what, got), = eng.calls
            if v is not None:
                assert what == 'build'
                assert got == (dict(q=None, upper=None, cat_p=None, prior_weight=PW, bandwidth='scott')
                               if bw == 'scott' else dict(q=None, upper=None, cat_p=None, prior_weight=None))
            else:
                tids, losses, obs = history_mod.gather(domain, trials, labels)
                ref = P.joint_mixture([specs[k] for k in ('ly', 'x')], obs, P.Splitter(tids, losses, 0.25), PW,
                                      streams=[labels.index('ly'), labels.index('x')], bandwidth=bw)
                assert what == 'set' and all(np.array_equal(a, b) for a, b in zip(got, ref))
