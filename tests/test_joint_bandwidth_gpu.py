"""The Scott-rule bandwidth of joint groups on the device (`-m gpu`): the
library's factor against the Python expression, float for float;
Engine.build_joint_groups(bandwidth='scott') against
posterior.joint_mixture(bandwidth='scott') by np.array_equal for the groups and
side sizes of tests/test_joint_bandwidth_host.py, tied quantized observations
included (which the neighbour rule flags); conditional groups; joint_score of
scott mixtures against the numpy definition; and tpe.suggest's documents, host
builder against device builder, along a run in every mode."""
import logging
import math

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import posterior as P
from hyperopt_amd import tpe
from hyperopt_amd.engine import EngineError
from tests import joint_group_cases as GC
from tests import joint_reference as JR
from tests import test_joint_bandwidth_host as BH
from tests import test_joint_build_gpu as BG

pytestmark = pytest.mark.gpu

PW = BH.PW
# (trials, gamma) -> (below, above) observations: n_below = min(ceil(gamma sqrt(trials)), 25), never
# more than the trials; the larger gammas reach the below sizes 7, 8, 9 and 25 with few trials
HISTORIES = [(1, 0.25), (2, 0.25), (3, 0.25), (8, 0.25), (9, 0.25), (10, 0.25), (27, 0.25), (28, 0.25), (130, 0.25),
             (131, 0.25), (132, 0.25), (305, 0.25), (49, 1.0), (64, 1.0), (81, 1.0), (34, 5.0)]


def side_sizes(n, gamma):
    nb = P.n_below_of(n, gamma)
    assert nb <= n
    return nb, n - nb


def test_histories_cover_the_side_sizes():
    sizes = [side_sizes(n, g) for n, g in HISTORIES]
    assert set(BH.SIZES) - {0} <= {na for _, na in sizes}                 # above: every size
    assert {1, 2, 7, 8, 9, 25} <= {nb for nb, _ in sizes}                 # below: up to its cap of 25
    assert 0 in {na for _, na in sizes}                                   # (below 0: the conditional cases)


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


def test_factor_is_the_python_expression(eng):
    f = eng.lib.tpe_joint_bandwidth_factor
    for D in (2, 3, 8, 32, 128):
        for n in range(1, 4097):
            want = 0.2 * math.pow(float(n), -1.0 / (D + 4))
            assert f(n, D) == want == P.joint_bandwidth_factor(n, D), (n, D)
        assert f(0, D) == f(-3, D) == 0.2


def view_of(specs, n, seed):
    tids, losses, cols = BH.history(specs, n, seed)
    return tids, losses, n, dict(cols), BG.Owner()


def build_scott(eng, specs, view, groups, gamma=BG.GAMMA, quantized=False, categorical=False):
    """The univariate posterior of `view` built on the device, the joint
    groups from it under the Scott rule: every group unflagged and equal, on
    both sides, to the host's arrays.  Returns the host mixtures by slot."""
    names = list(specs)
    table = [(s.label, s.kind, s.args) for s in specs.values()]
    P.DeviceHistoryUploader().build(eng, table, view, gamma, PW)
    args, kw = tpe._joint_device_args(specs, names, groups, quantized, categorical, PW, 'scott')
    assert kw['bandwidth'] == 'scott' and kw['prior_weight'] == PW
    eng.clear_joint_groups()
    flags = eng.build_joint_groups(args, **kw)
    assert list(flags) == [0] * len(groups)
    tids, losses, _, cols, _ = view
    splitter = P.Splitter(tids, losses, gamma)
    mixes = {}
    for slot, g in groups:
        mix = P.joint_mixture([specs[k] for k in g], cols, splitter, PW, streams=[names.index(k) for k in g],
                              quantized=quantized, categorical=categorical, bandwidth='scott')
        for side in (0, 1):
            ref = (mix.wa, mix.mua, mix.siga) if side else (mix.wb, mix.mub, mix.sigb)
            got = eng.joint_get_group(slot, side)
            for name, a, b in zip(('W', 'mu', 'sigma'), got, ref):
                assert a.shape == np.asarray(b).shape, (slot, side, name)
                assert np.array_equal(a, b), (slot, side, name)
        mixes[slot] = mix
    return mixes


@pytest.mark.parametrize('name', list(BH.GROUPS))
def test_device_build_equals_host_build(eng, name):
    specs = BH.specs_of(BH.GROUPS[name])
    for n, gamma in HISTORIES:
        view = view_of(specs, n, 3000 + n)
        mix = build_scott(eng, specs, view, [(0, list(specs))], gamma, quantized=True, categorical=True)[0]
        assert (len(mix.wb) - 1, len(mix.wa) - 1) == side_sizes(n, gamma), (n, gamma)


def test_tied_quantized_observations_build_where_the_neighbour_rule_flags(eng):
    """A quniform label with repeated values on both sides: built under the
    Scott rule, the host's bits; the same history under the neighbour rule
    comes back with TPE_JOINT_FLAG_TIE."""
    specs = BH.specs_of(BH.GROUPS['uniform_quniform'])
    view = view_of(specs, 60, 77)
    tids, losses, _, cols, _ = view
    below = np.argsort(losses)[:P.n_below_of(60, BG.GAMMA)]
    assert len(below) == 2
    v = cols['h1'][1].copy()
    v[below[1]] = v[below[0]]
    cols['h1'] = (tids, v)
    above = np.delete(v, below)
    assert len(set(above)) < len(above)
    groups = [(0, list(specs))]
    build_scott(eng, specs, view, groups, quantized=True)
    won = eng.joint_suggest_batch(BG.SEED, BG.ROUNDS, BG.N_CAND)
    assert sorted(won) == [0] and np.all(np.isfinite(won[0][2])) and np.all(np.isfinite(won[0][3]))
    # mode 0 on the build the scott call just read
    args, kw = tpe._joint_device_args(specs, list(specs), groups, True, False, PW)
    assert 'bandwidth' not in kw
    eng.clear_joint_groups()
    assert list(eng.build_joint_groups(args, **kw)) == [L.TPE_JOINT_FLAG_TIE]
    assert list(eng.build_joint_groups(args, bandwidth='neighbour', **kw)) == [L.TPE_JOINT_FLAG_TIE]
    with pytest.raises(EngineError):
        eng.joint_get_group(0, 0)


def test_keyword_errors(eng):
    specs = BH.specs_of(['uniform', 'normal'])
    view = view_of(specs, 30, 5)
    table = [(s.label, s.kind, s.args) for s in specs.values()]
    P.DeviceHistoryUploader().build(eng, table, view, BG.GAMMA, PW)
    one = [(0, L.TPE_JOINT_STREAM, [0, 1], [0, 1])]
    with pytest.raises(ValueError, match='bandwidth'):
        eng.build_joint_groups(one, bandwidth='silverman')
    with pytest.raises(ValueError, match='prior_weight'):
        eng.build_joint_groups(one, bandwidth='scott')
    with pytest.raises(EngineError, match='prior weight'):
        eng.build_joint_groups(one, bandwidth='scott', prior_weight=0.0)
    slots, picks = np.zeros(1, dtype=np.int32), np.full(1, L.TPE_JOINT_STREAM, dtype=np.uint32)
    off, labels = np.array([0, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32)
    flags = np.zeros(1, dtype=np.int32)
    for bad in (2, -1):
        assert eng.lib.tpe_joint_build_groups_bw(eng.h, 1, slots.ctypes.data, picks.ctypes.data, off.ctypes.data,
                                                 labels.ctypes.data, labels.ctypes.data, None, None, None, PW, bad,
                                                 flags.ctypes.data) == L.TPE_ERR_ARG
    assert list(eng.build_joint_groups(one, bandwidth='scott', prior_weight=PW)) == [0]
    assert eng.lib.tpe_abi_version() == 5


@pytest.mark.parametrize('never_inner,c0_not_below', [(False, False), (True, True)])
def test_conditional_groups(eng, never_inner, c0_not_below):
    """group=True: groups observed in subsets of the trials; (second case) a
    branch without a below trial, and a group never observed -- K = 1 on both
    sides, every score 0, candidate 0 wins."""
    domain, specs, view = BG.conditional_case(60, 11, never_inner, c0_not_below)
    groups = tpe.joint_groups(domain, specs, view[3])
    assert groups == GC.GROUPS
    build_scott(eng, specs, view, groups)
    if c0_not_below:
        assert eng.joint_get_group(1, 0)[0].shape == (1,)
        assert eng.joint_get_group(2, 0)[0].shape == eng.joint_get_group(2, 1)[0].shape == (1,)
        _, index, ll, lg = eng.joint_suggest_batch(BG.SEED, BG.ROUNDS, BG.N_CAND)[2]
        assert np.all(index == 0) and np.array_equal(ll, lg)


@pytest.mark.parametrize('n', [40, 300])
def test_score_of_scott_mixtures_against_the_numpy_definition(eng, n):
    """Scott mixtures through set_joint_group: joint_score on 24 drawn
    candidates against tests/joint_reference.py, at the bound its other users
    apply (1e-9 relative to max(1, |lpdf|))."""
    kinds = ['uniform', 'loguniform', 'normal', 'lognormal']
    specs = BH.specs_of(kinds)
    tids, losses, cols = BH.history(specs, n, 91)
    mix = P.joint_mixture(list(specs.values()), cols, P.Splitter(tids, losses, BG.GAMMA), PW, bandwidth='scott')
    eng.clear_joint_groups()
    eng.set_joint_group(0, L.TPE_JOINT_STREAM, *mix)
    dims = [JR.Dim(log, low, high, d) for d, (log, low, high, _, _) in
            enumerate(JR.prior_of(s.kind, s.args) for s in specs.values())]
    ref = JR.JointRef(dims, (mix.wb, mix.mub, mix.sigb), (mix.wa, mix.mua, mix.siga))
    vals, _ = eng.joint_draw(17, 24)
    ll, lg = eng.joint_score(vals)
    for got, side in ((ll, 'below'), (lg, 'above')):
        want = ref.joint_lpdf(vals, side)
        err, bound = np.abs(got - want), 1e-9 * np.maximum(1.0, np.abs(want))
        print('n = %d, %s: worst |err| / bound %.3g' % (n, side, float(np.max(err / bound))))
        assert np.all(np.isfinite(got)) and np.all(err <= bound)


def _vals(docs):
    return [d['misc']['vals'] for d in docs]


@pytest.mark.parametrize('mode', BG.MODES, ids=lambda m: '-'.join(sorted(m)) or 'plain')
def test_suggest_documents_along_a_run(mode, caplog):
    """45 trials on the conditional space of test_joint_build_gpu.py, at every
    step past startup: the scott documents of the host and the device builder
    are equal; joint_bandwidth='neighbour' gives the call without the keyword;
    and scott differs from neighbour somewhere along the run.  No scott build
    is flagged by the device."""
    differed, flagged = [], []

    def algo(new_ids, domain, trials, seed):
        if len(trials.trials) >= 20:
            ids = [new_ids[0] + j for j in range(3)] if mode.get('batch') else list(new_ids)

            def docs(**kw):
                return _vals(tpe.suggest(ids, domain, trials, seed, multivariate=True, **dict(mode, **kw)))
            caplog.clear()
            with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
                scott = docs(posterior_builder='device', joint_bandwidth='scott')
            lines = [r.getMessage() for r in caplog.records if 'group(s) built on the device' in r.getMessage()]
            assert lines and all('scott bandwidth' in m for m in lines)
            flagged.extend(int(m.split('(')[2].split(' ')[0]) for m in lines)
            assert scott == docs(posterior_builder='host', joint_bandwidth='scott'), (len(trials.trials), mode)
            plain = docs(posterior_builder='device')
            assert plain == docs(posterior_builder='device', joint_bandwidth='neighbour')
            assert len(scott) == len(plain) == len(ids)
            differed.append(scott != plain)
        return tpe.suggest(new_ids, domain, trials, seed, multivariate=True, group=True, posterior_builder='device',
                           joint_bandwidth='scott')
    trials = H.Trials()
    H.fmin(BG.e2e_loss, BG.e2e_space(), algo=algo, max_evals=45, trials=trials, rstate=np.random.RandomState(5))
    assert len(trials) == 45 and len(differed) == 25
    assert any(differed), 'joint_bandwidth reached nothing'
    assert flagged and max(flagged) == 0
