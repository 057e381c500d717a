"""Conditioning a joint slot on fixed dimensions on the device (`-m gpu`):
Engine.joint_condition against the plain-loop rule of
tests/joint_fixed_reference.py, the conditioned slot against the slot
set_joint_group makes of its read-back arrays (bit for bit), the
constant-difference identity on the device's own scores, the weight floor, the
C ABI's errors, several devices, and tpe.suggest(fixed=...) document for
document."""
import itertools
import math

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import tpe
from hyperopt_amd import posterior as P
from hyperopt_amd.engine import JOINT_DIM_DTYPE, EngineError
from tests import joint_cat_reference as CR
from tests import joint_fixed_reference as FR
from tests import test_joint_bandwidth_host as BH
from tests import test_joint_build_gpu as BG

pytestmark = pytest.mark.gpu

PW = 1.0
STREAM = L.TPE_JOINT_STREAM - 1
SRC, OUT, SET, INPLACE = 0, 1, 2, 3
SEED = 29
BELOW = [1, 2, 26]
# the prior alone, one trial, around a wave and around the 256-thread block of
# the weights' kernel: one and two strides, a stride partly filled, several
ABOVE = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
VALUE = {'uniform': 1.75, 'loguniform': 0.4, 'normal': 0.25, 'lognormal': 1.5, 'quniform': 1000.0, 'randint': 2.0}
QUNIFORM = dict(low=0.0, high=4000.0, q=2.0)      # 2001 grid values: tie-free columns, as the neighbour rule wants


def subsets(D):
    if D <= 3:
        return [c for r in range(1, D) for c in itertools.combinations(range(D), r)]
    return [(0,), (1, 3), (0, 1, 2, 4)]


GROUP_CASES = [(name, f) for name, kinds in BH.GROUPS.items() for f in subsets(len(kinds))]


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


_mixtures = {}


def mixture(name, nb, na):
    """(specs, the JointMixture) of group `name` with nb below and na above
    components (the prior included): the neighbour rule on a tie-free history."""
    key = (name, nb, na)
    if key not in _mixtures:
        specs = BH.specs_of(BH.GROUPS[name])
        n = nb - 1 + na - 1
        _, _, cols = BH.history(specs, n, 7000 + 10 * nb + na)
        for k, s in list(specs.items()):
            if s.kind == 'quniform':
                specs[k] = BH.Spec(k, 'quniform', QUNIFORM)
                cols[k] = (cols[k][0], np.random.RandomState(na).permutation(2001)[:n] * 2.0)
        mix = P.joint_mixture(list(specs.values()), cols, BH.FirstBelow(nb - 1), PW, quantized=True, categorical=True)
        assert len(mix.wb) == nb and len(mix.wa) == na
        _mixtures[key] = (specs, mix)
    return _mixtures[key]


def ref_dims(mix):
    """The reference's dimension records of a JointMixture."""
    out, at = [], 0
    for d in range(len(mix.dims)):
        C = int(mix.upper[d])
        if C:
            out.append(CR.CDim(False, None, None, d, upper=C, p=mix.cat_p[at:at + C]))
            at += C
            continue
        j = mix.dims[d]
        bounded = int(j['flags']) == 3
        out.append(CR.CDim(int(j['kind']) == L.TPE_LGMM1, float(j['low']) if bounded else None,
                           float(j['high']) if bounded else None, d, q=float(mix.q[d]) or None))
    return out


def free_args(mix, free, sides):
    """set_joint_group's arguments of the group over `free` with the sides
    [(W, mu, sigma)] * 2."""
    cat, at = [], 0
    for d in range(len(mix.dims)):
        C = int(mix.upper[d])
        if C and d in free:
            cat.append(mix.cat_p[at:at + C])
        at += C
    (wb, mub, sigb), (wa, mua, siga) = sides
    return (mix.dims[free], wb, mub, sigb, wa, mua, siga), dict(
        q=mix.q[free], upper=mix.upper[free], cat_p=np.concatenate(cat) if cat else None, prior_weight=PW)


def same_slots(eng, a, b, n=24):
    """Draws and scores of two slots, bit for bit."""
    for rnd in (0, 4294967295):
        va, ca = eng.joint_draw(SEED, n, round=rnd, slot=a)
        vb, cb = eng.joint_draw(SEED, n, round=rnd, slot=b)
        assert np.array_equal(va, vb) and np.array_equal(ca, cb)
        for x, y in zip(eng.joint_score(va, slot=a), eng.joint_score(va, slot=b)):
            assert np.array_equal(x, y)
    return va


def condition_case(eng, name, fixed, nb, na):
    specs, mix = mixture(name, nb, na)
    kinds = [s.kind for s in specs.values()]
    fixed = list(fixed)
    values = [VALUE[kinds[d]] for d in fixed]
    free = [d for d in range(len(kinds)) if d not in fixed]
    eng.clear_joint_groups()
    eng.set_joint_group(SRC, STREAM, *mix, prior_weight=PW)
    eng.joint_condition(SRC, fixed, values, dst=OUT)
    assert eng.joint_slots == {SRC: len(kinds), OUT: len(free)}
    src = [(mix.wb, mix.mub, mix.sigb), (mix.wa, mix.mua, mix.siga)]
    _, rb, ra, rels = FR.condition(ref_dims(mix), src[0], src[1], fixed, values, PW)
    got = []
    for side in (0, 1):
        W, mu, sig = eng.joint_get_group(OUT, side)
        assert np.array_equal(mu, src[side][1][:, free]) and np.array_equal(sig, src[side][2][:, free])
        rel = np.asarray(rels[side])
        assert W.shape == rel.shape and np.all(W >= FR.FLOOR)
        big = rel > -700.0
        assert big.any()
        err = np.abs(np.log(W[big]) - rel[big])
        bar = 1e-9 * np.maximum(1.0, np.abs(rel[big]))
        assert np.all(err <= bar), (side, float(np.max(err / bar)))
        assert np.all(W[~big] <= 2.0 ** -1000)
        assert np.array_equal(eng.joint_get_group(SRC, side)[0], src[side][0])      # the source is untouched
        got.append((W, mu, sig))
    # the slot set_joint_group makes of the read-back weights and the free columns
    args, kw = free_args(mix, free, got)
    eng.set_joint_group(SET, STREAM, *args, **kw)
    same_slots(eng, OUT, SET)
    # in place
    eng.set_joint_group(INPLACE, STREAM, *mix, prior_weight=PW)
    eng.joint_condition(INPLACE, fixed, values)
    assert eng.joint_slots[INPLACE] == len(free)
    for side in (0, 1):
        for a, b in zip(eng.joint_get_group(INPLACE, side), got[side]):
            assert np.array_equal(a, b)
    same_slots(eng, OUT, INPLACE)


@pytest.mark.parametrize('name,fixed', GROUP_CASES, ids=['%s-F%s' % (n, ''.join(map(str, f))) for n, f in GROUP_CASES])
def test_device_against_reference(eng, name, fixed):
    """Every above size with the below sizes in turn, and every below size
    with an above side past one block."""
    pairs = [(BELOW[i % 3], na) for i, na in enumerate(ABOVE)] + [(nb, 300) for nb in BELOW]
    for nb, na in pairs:
        condition_case(eng, name, fixed, nb, na)


@pytest.mark.parametrize('name,fixed', GROUP_CASES, ids=['%s-F%s' % (n, ''.join(map(str, f))) for n, f in GROUP_CASES])
def test_device_identity(eng, name, fixed):
    """score(source at (x_F, x_R)) - score(conditioned at x_R) is one number
    over the round's 24 candidates, per side; the conditioned round's winner
    is the argmax of the source's score over them."""
    specs, mix = mixture(name, 26, 257)
    kinds = [s.kind for s in specs.values()]
    fixed = list(fixed)
    values = [VALUE[kinds[d]] for d in fixed]
    free = [d for d in range(len(kinds)) if d not in fixed]
    eng.clear_joint_groups()
    eng.set_joint_group(SRC, STREAM, *mix, prior_weight=PW)
    eng.joint_condition(SRC, fixed, values, dst=OUT)
    xr, _ = eng.joint_draw(SEED, 24, round=6, slot=OUT)
    x = np.empty((24, len(kinds)))
    x[:, free] = xr
    x[:, fixed] = values
    full = eng.joint_score(x, slot=SRC)
    cond = eng.joint_score(xr, slot=OUT)
    for side in (0, 1):
        assert np.all(np.isfinite(full[side])) and np.all(np.isfinite(cond[side]))
        diff = full[side] - cond[side]
        bar = 1e-9 * max(1.0, float(np.max(np.abs(full[side]))), float(np.max(np.abs(cond[side]))))
        spread = float(np.max(diff) - np.min(diff))
        print('%s F=%s side %d: spread %.3g, bar %.3g' % (name, fixed, side, spread, bar))
        assert spread <= bar, (side, spread, bar)
    win, index, ll, lg = eng.joint_suggest(SEED, 24, round=6, slot=OUT)
    assert index == int(np.argmax(full[0] - full[1]))
    assert np.array_equal(win, xr[index]) and ll == cond[0][index] and lg == cond[1][index]


# -- the floor -----------------------------------------------------------------------------------
def clip_group(Kb, Ka, near=None):
    """Two uniform labels on [-5, 5), every trial kernel at the lower sigma
    clip 10 / 100 with its mean in [3.5, 4.5] -- 85 sigmas and more from the
    far edge -5 of dimension 0 -- except trial `near` of each side, at -4.95."""
    dims = np.zeros(2, dtype=JOINT_DIM_DTYPE)
    dims['kind'], dims['flags'], dims['low'], dims['high'], dims['stream'] = L.TPE_GMM1, 3, -5.0, 5.0, [0, 1]
    rng = np.random.RandomState(Kb + Ka)
    sides = []
    for K in (Kb, Ka):
        mu = rng.uniform(3.5, 4.5, (K, 2))
        sig = np.full((K, 2), 0.1)
        mu[0], sig[0] = 0.0, 10.0
        if near is not None:
            mu[near, 0] = -4.95
        sides.append((np.full(K, 1.0 / K), mu, sig))
    return (dims,) + sides[0] + sides[1]


@pytest.mark.parametrize('near', [None, 7])
def test_floor(eng, near):
    Kb, Ka = 26, 300
    eng.clear_joint_groups()
    eng.set_joint_group(SRC, STREAM, *clip_group(Kb, Ka, near))
    eng.joint_condition(SRC, [0], [-5.0], dst=OUT)
    alive = []
    for side, K in ((0, Kb), (1, Ka)):
        W = eng.joint_get_group(OUT, side)[0]
        floored = W == FR.FLOOR
        # every trial kernel far from the edge underflows: exp(-0.5 85^2) = 0 in fp64
        assert int(floored.sum()) == (K - 1 if near is None else K - 2)
        assert not floored[0] and (near is None or not floored[near])
        if near is None:
            assert W[0] == 1.0
        else:      # the trial kernel is 100 times narrower than the prior: it dominates
            assert W[near] > 0.9 and 0.0 < W[0] < 0.1
        assert abs(float(W.sum()) - 1.0) <= 1e-12
        alive.append(np.flatnonzero(~floored))
    vals, comp = eng.joint_draw(SEED, 4096, slot=OUT)
    assert set(comp.tolist()) <= set(alive[0].tolist())
    if near is not None:
        assert set(comp.tolist()) == {0, near}
    ll, lg = eng.joint_score(vals, slot=OUT)
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(lg))
    win, index, wl, wg = eng.joint_suggest(SEED, 4096, slot=OUT)
    assert math.isfinite(wl) and math.isfinite(wg) and index == int(np.argmax(ll - lg))


# -- errors --------------------------------------------------------------------------------------
def test_errors(eng):
    specs, mix = mixture('uniform_quniform', 26, 65)
    _, other = mixture('normal_lognormal', 2, 63)
    eng.clear_joint_groups()
    eng.set_joint_group(SRC, STREAM, *mix, prior_weight=PW)
    eng.set_joint_group(OUT, STREAM, *other, prior_weight=PW)
    before = [eng.joint_get_group(s, side) for s in (SRC, OUT) for side in (0, 1)]
    drawn = eng.joint_draw(SEED, 24, slot=OUT)

    def unchanged():
        assert eng.joint_slots == {SRC: 2, OUT: 2}
        after = [eng.joint_get_group(s, side) for s in (SRC, OUT) for side in (0, 1)]
        assert all(np.array_equal(a, b) for x, y in zip(before, after) for a, b in zip(x, y))
        assert all(np.array_equal(a, b) for a, b in zip(drawn, eng.joint_draw(SEED, 24, slot=OUT)))
    # a grid value whose rounding interval [4999, 5001] lies beyond high = 4000: no component reaches it
    for dst in (OUT, None):
        with pytest.raises(ValueError, match='reaches'):
            eng.joint_condition(SRC, [1], [5000.0], dst=dst)
        unchanged()
    with pytest.raises(ValueError, match='NaN'):
        eng.joint_condition(SRC, [0], [float('nan')], dst=OUT)
    unchanged()
    for dims, values, match in (([], [], 'n_dims - 1'), ([0, 1], [1.0, 2.0], 'n_dims - 1'),
                                ([0, 0], [1.0, 1.0], 'n_dims - 1'), ([2], [1.0], 'distinct'),
                                ([-1], [1.0], 'distinct')):
        with pytest.raises(EngineError, match=match):
            eng.joint_condition(SRC, dims, values, dst=OUT)
        unchanged()
    _, five = mixture('five', 2, 63)
    eng.set_joint_group(SET, STREAM, *five, prior_weight=PW)
    with pytest.raises(EngineError, match='distinct'):
        eng.joint_condition(SET, [1, 3, 1], [0.4, 1.5, 0.4], dst=INPLACE)      # a repeated dimension
    for src, dst in ((5, OUT), (SRC, L.TPE_JOINT_MAX_GROUPS), (-1, OUT)):
        with pytest.raises(EngineError, match='no joint posterior set|slot'):
            eng.joint_condition(src, [0], [1.0], dst=dst)
    rc = eng.lib.tpe_joint_condition_group(eng.h, SRC, OUT, 1, None, None)
    assert rc == L.TPE_ERR_ARG
    with pytest.raises(ValueError, match='one value per'):
        eng.joint_condition(SRC, [0], [1.0, 2.0])
    eng.clear_joint_groups()


# -- several devices -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def engs():
    from hyperopt_amd.engine import Engine
    made = {'one': Engine(0, 'f64'), 'two': Engine([0, 0], 'f64'), 'two_replicated': Engine([0, 0], 'f64')}
    made['two_replicated'].set_option('label_shards', 0)
    yield made
    for e in made.values():
        e.close()


def built_and_conditioned(eng, specs, view, groups, held, **kw):
    """The device build of `groups`, the groups of `held` ({slot: (dims,
    values)}) conditioned in place: the slots' arrays and their rounds."""
    names = list(specs)
    table = [(s.label, s.kind, s.args) for s in specs.values()]
    P.DeviceHistoryUploader().build(eng, table, view, BG.GAMMA, PW)
    args, akw = tpe._joint_device_args(specs, names, groups, kw.get('quantized', False),
                                       kw.get('categorical', False), PW)
    eng.clear_joint_groups()
    assert not any(eng.build_joint_groups(args, **akw))
    for slot, (dims, values) in held.items():
        eng.joint_condition(slot, dims, values)
    mix = {slot: [eng.joint_get_group(slot, side) for side in (0, 1)] for slot, _ in groups}
    return mix, eng.joint_suggest_batch(SEED, [3, 0, 4294967295], 4096), eng.joint_suggest_batch(SEED, [5, 6], 24)


@pytest.mark.parametrize('key', ['two', 'two_replicated'])
def test_several_devices(engs, key):
    specs = BG.dense_specs(['uniform', 'loguniform', 'normal', 'lognormal', 'quniform', 'uniform'])
    view = BG.make_view(specs, 300, 77)
    groups = [(0, ['h0', 'h1', 'h4']), (1, ['h2', 'h3', 'h5'])]
    held = {0: ([0, 2], [1.75, 1000.0]), 1: ([1], [1.5])}
    ref = built_and_conditioned(engs['one'], specs, view, groups, held, quantized=True)
    e = engs[key]
    got = built_and_conditioned(e, specs, view, groups, held, quantized=True)
    where = [e.lib.tpe_label_device(e.h, li) for li in range(len(specs))]
    assert (set(where) == {-1}) if key == 'two_replicated' else (set(where) == {0, 1})
    assert e.joint_slots == engs['one'].joint_slots == {0: 1, 1: 2}
    for slot in (0, 1):
        for side in (0, 1):
            for a, b in zip(got[0][slot][side], ref[0][slot][side]):
                assert a.shape == b.shape and np.array_equal(a, b)
    for g, r in zip(got[1:], ref[1:]):
        assert sorted(g) == sorted(r) == [0, 1]
        for slot in g:
            assert all(np.array_equal(a, b) for a, b in zip(g[slot], r[slot]))
    # an error on the devices is the call's, the slots stay
    with pytest.raises(ValueError, match='reaches'):
        e.joint_condition(1, [0], [float('inf')])
    assert e.joint_slots == {0: 1, 1: 2}


# -- tpe.suggest end to end ----------------------------------------------------------------------
def _vals(docs):
    return [d['misc']['vals'] for d in docs]


def fixed_of(mode):
    fixed = {'lr': 0.01}
    if mode.get('joint_quantized'):
        fixed['width'] = 128.0
    if mode.get('joint_categorical'):
        fixed['opt'] = 0
    return fixed


def test_documents_along_a_run():
    """45 trials on BG.e2e_space(), every mode, at every third step past
    startup: both builders give the same documents; the fixed labels hold their values;
    the labels outside the conditioned groups are the unfixed call's; the
    conditioned group's free labels differ from it somewhere along the run."""
    differs = {i: False for i in range(len(BG.MODES))}

    def algo(new_ids, domain, trials, seed):
        if len(trials.trials) >= 20 and len(trials.trials) % 3 == 2:
            for i, mode in enumerate(BG.MODES):
                ids = [new_ids[0] + j for j in range(3)] if mode.get('batch') else list(new_ids)
                fixed = fixed_of(mode)
                got = [_vals(tpe.suggest(ids, domain, trials, seed, multivariate=True, posterior_builder=b,
                                         fixed=fixed, **mode)) for b in ('device', 'host')]
                assert got[0] == got[1], (len(trials.trials), mode)
                assert len(got[0]) == len(ids)
                plain = _vals(tpe.suggest(ids, domain, trials, seed, multivariate=True, posterior_builder='device',
                                          **mode))
                for v, p in zip(got[0], plain):
                    for k, x in fixed.items():
                        assert v[k] == [x] and type(v[k][0]) is type(x)
                    if mode.get('batch') == 'pending' or 'opt' in fixed:
                        # (pending: a later id sees the earlier, different, documents; a fixed
                        # choice: the branch may differ from the unfixed call's)
                        continue
                    group = {'lr', 'mom'} | ({'width'} if mode.get('joint_quantized') else set())
                    for k in v:
                        if k not in group:
                            assert v[k] == p[k], (k, mode)
                    differs[i] |= any(v[k] != p[k] for k in group - set(fixed))
                if 'opt' in fixed:
                    for v, p in zip(got[0], plain):
                        assert len(v['a']) == len(v['b']) == 1                  # the fixed index selects its branch
                        if p['opt'] == [0]:      # the same branch: its own group (a, b) has no fixed label
                            assert v['a'] == p['a'] and v['b'] == p['b']
                        differs[i] |= v['mom'] != p['mom']
                if mode.get('batch') == 'pending':
                    differs[i] |= got[0][0]['mom'] != plain[0]['mom']
                    assert all(got[0][0][k] == plain[0][k] for k in ('width', 'opt', 'a', 'b'))
        return tpe.suggest(new_ids, domain, trials, seed, multivariate=True, group=True, posterior_builder='device')
    trials = H.Trials()
    H.fmin(BG.e2e_loss, BG.e2e_space(), algo=algo, max_evals=45, trials=trials, rstate=np.random.RandomState(5))
    assert len(trials) == 45 and all(differs.values()), differs


def run_of(n, seed):
    trials = H.Trials()
    H.fmin(BG.e2e_loss, BG.e2e_space(), algo=H.rand.suggest, max_evals=n, trials=trials,
           rstate=np.random.RandomState(seed))
    return trials


def test_documents_on_two_devices_and_without_multivariate(caplog):
    import logging
    from hyperopt_amd.base import Domain
    trials = run_of(40, 8)
    domain = Domain(BG.e2e_loss, BG.e2e_space())
    mode = dict(multivariate=True, group=True, joint_quantized=True, joint_categorical=True, batch=True)
    fixed = {'lr': 0.01, 'width': 128.0, 'opt': 0}
    ids = [100, 101, 102]
    for builder in ('device', 'host'):
        with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
            caplog.clear()
            one = _vals(tpe.suggest(ids, domain, trials, 3, fixed=fixed, posterior_builder=builder, **mode))
            assert any('1 group(s) conditioned' in r.getMessage() for r in caplog.records)
        two = _vals(tpe.suggest(ids, domain, trials, 3, fixed=fixed, posterior_builder=builder, devices=[0, 0],
                                **mode))
        assert one == two
    # every label of a group fixed: the group is not built, the others are the unfixed call's
    plain = _vals(tpe.suggest(ids, domain, trials, 3, multivariate=True, group=True))
    held = _vals(tpe.suggest(ids, domain, trials, 3, multivariate=True, group=True, fixed={'lr': 0.01, 'mom': 0.5}))
    for v, p in zip(held, plain):
        assert v['lr'] == [0.01] and v['mom'] == [0.5]
        assert all(v[k] == p[k] for k in v if k not in ('lr', 'mom'))
    # multivariate=False: the fixed labels' winners replaced, every other label untouched
    plain = _vals(tpe.suggest(ids, domain, trials, 3, batch=True))
    held = _vals(tpe.suggest(ids, domain, trials, 3, batch=True, fixed={'lr': 0.01, 'width': 64.0}))
    for v, p in zip(held, plain):
        assert v['lr'] == [0.01] and v['width'] == [64.0]
        assert all(v[k] == p[k] for k in v if k not in ('lr', 'width'))
    # a fixed choice index selects its branch, whatever the round's winner was
    for opt in (0, 1):
        for v in _vals(tpe.suggest(ids, domain, trials, 3, batch=True, fixed={'opt': opt, 'a': 0.5})):
            assert v['opt'] == [opt] and v['a'] == ([0.5] if opt == 0 else []) and len(v['b']) == 1 - opt
    assert _vals(tpe.suggest(ids, domain, trials, 3, batch=True, fixed={})) == plain
