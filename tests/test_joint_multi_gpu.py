"""Joint (multivariate) TPE on multi-device contexts (`-m gpu`): the joint
posteriors replicated on every device, the joint rounds split by candidate
ranges or by whole rounds (Engine.joint_last_shards tells which), and the
device build of the joint groups behind a replicated and a label-sharded
univariate build.  Every comparison is np.array_equal against the one-device
engine: values, index, lpdf_below, lpdf_above, the unfolded mixtures, the flags.

The engines are Engine(0), Engine([0, 0]) and Engine([0, 0, 0]) -- several
contexts on the one GPU, as in test_multi.py -- and Engine([0, 1]) where the
machine has two GPUs (the only place a copy between devices really crosses one).
"""
import collections
import logging
from functools import partial

import numpy as np
import pytest
import torch

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import posterior as P
from hyperopt_amd import tpe
from hyperopt_amd.engine import EngineError
from tests import joint_cases as JC
from tests import joint_cat_cases as CC
from tests import joint_group_cases as GC
from tests import joint_quant_cases as QC
from tests import test_joint_build_gpu as BG

pytestmark = pytest.mark.gpu

DEVICES = {'one': 0, 'two': [0, 0], 'three': [0, 0, 0], 'real2': [0, 1], 'two_replicated': [0, 0]}
real2 = pytest.param('real2', marks=pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs'))
SEED = 19
BATCH_ROUNDS = [3, 4294967295, 0]


@pytest.fixture(scope='module')
def engs():
    """The engines by name, made when first asked for."""
    from hyperopt_amd.engine import Engine
    made = {}

    def get(key):
        if key not in made:
            made[key] = Engine(DEVICES[key], 'f64')
            if key == 'two_replicated':
                made[key].set_option('label_shards', 0)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def set_named(eng, name, slot=0):
    """A group of one of the case modules in `slot`."""
    stream = GC.pick_stream(slot)
    if name in JC.GROUPS:
        eng.set_joint_group(slot, stream, *JC.engine_args(JC.group(name)))
    elif name in QC.GROUPS:
        args, q = QC.engine_args(QC.group(name))
        eng.set_joint_group(slot, stream, *args, q=q)
    else:
        args, kw = CC.engine_args(CC.group(name))
        eng.set_joint_group(slot, stream, *args, **kw)


def same_single(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def same_batch(a, b):
    return sorted(a) == sorted(b) and all(same_single(a[s], b[s]) for s in a)


_ref = {}


def reference(one, name, n):
    """The one-device rounds of group `name` at n candidates, computed once."""
    if (name, n) not in _ref:
        one.clear_joint_groups()
        set_named(one, name)
        single = one.joint_suggest(SEED, n, round=5)
        assert one.joint_last_shards() == (0, 1)
        _ref[(name, n)] = (single, one.joint_suggest_batch(SEED, BATCH_ROUNDS, n))
    return _ref[(name, n)]


# -- 1. candidate shards ----------------------------------------------------------------
# (engine, candidates, mode, devices that ran a shard)
SPLITS = [('two', 2047, 0, 1), ('two', 2048, 1, 2), ('three', 3073, 1, 3),
          pytest.param('real2', 2048, 1, 2, marks=real2.marks)]
# the one-device round runs the fused map (513 tiles), the two shards the split map (257 tiles each)
CROSSING = {'d5_k300': 131072 + 3, 'd33': 32768 + 3}


def check_candidate_shards(engs, name, key, n, mode, nd):
    single, batch = reference(engs('one'), name, n)
    e = engs(key)
    e.clear_joint_groups()
    set_named(e, name)
    got = e.joint_suggest(SEED, n, round=5)
    assert e.joint_last_shards() == (mode, nd)
    assert same_single(got, single), (name, key, n, got[1], single[1])
    got = e.joint_suggest_batch(SEED, BATCH_ROUNDS, n)
    # (too few candidates for candidate shards: the batch's 3 rounds go round by round)
    devs = len(DEVICES[key])
    assert e.joint_last_shards() == ((mode, nd) if mode == 1 else (2, devs) if len(BATCH_ROUNDS) >= devs else (0, 1))
    assert same_batch(got, batch), (name, key, n)


@pytest.mark.parametrize('key,n,mode,nd', SPLITS)
@pytest.mark.parametrize('name', ['d5_k300', 'd33', 'q2_mixed', 'c2_mixed'])
def test_candidate_shards(engs, name, key, n, mode, nd):
    """n = 2047 stays on the primary, 2048 is two shards of 1024, 3073 three
    uneven shards of 1025 / 1024 / 1024; one round, and a batch of 3 rounds
    (the round number 2^32 - 1 among them)."""
    check_candidate_shards(engs, name, key, n, mode, nd)


@pytest.mark.parametrize('name', sorted(CROSSING))
def test_candidate_shards_across_the_layout_boundary(engs, name):
    """The shards land in another layout than the one-device round (fused
    against split map) and still return its bits."""
    check_candidate_shards(engs, name, 'two', CROSSING[name], 1, 2)


# -- 2. round shards --------------------------------------------------------------------
@pytest.mark.parametrize('key,nd', [('two', 2), ('three', 3), pytest.param('real2', 2, marks=real2.marks)])
def test_round_shards(engs, key, nd):
    """Four slots, 24 candidates, 11 rounds: 6 + 5 rounds on two devices,
    4 + 4 + 3 on three, every device writing its own rows."""
    one, e = engs('one'), engs(key)
    GC.set_slots(one)
    GC.set_slots(e)
    assert len(GC.ROUNDS) == 11
    ref = one.joint_suggest_batch(GC.SEED, GC.ROUNDS, 24)
    got = e.joint_suggest_batch(GC.SEED, GC.ROUNDS, 24)
    assert e.joint_last_shards() == (2, nd)
    assert sorted(got) == [0, 1, 2, 3] and same_batch(got, ref)
    # fewer rounds than devices, too few candidates: the primary alone
    got = e.joint_suggest_batch(GC.SEED, GC.ROUNDS[2:3], 24)
    assert e.joint_last_shards() == (0, 1)
    assert same_batch(got, one.joint_suggest_batch(GC.SEED, GC.ROUNDS[2:3], 24))


# -- 3. ties and NaN order across shards --------------------------------------------------
@pytest.mark.parametrize('key,nd', [('two', 2), ('three', 3)])
def test_ties_across_shards_go_to_the_lowest_index(engs, key, nd):
    """Both sides the same mixture: every score is exactly 0 in every shard,
    and the merge returns candidate 0."""
    e = engs(key)
    GC.set_slots(e, ['d1_tie'])
    values, index, ll, lg = e.joint_suggest(2, 5000, round=4)
    assert e.joint_last_shards() == (1, nd)
    assert index == 0 and ll == lg
    got = e.joint_suggest_batch(2, GC.TIE_ROUNDS, 5000)[0]
    assert e.joint_last_shards() == (1, nd)
    assert got[1].tolist() == [0] * len(GC.TIE_ROUNDS) and np.array_equal(got[2], got[3])
    one = engs('one')
    GC.set_slots(one, ['d1_tie'])
    assert same_single(got, one.joint_suggest_batch(2, GC.TIE_ROUNDS, 5000)[0])


@pytest.mark.parametrize('key,nd', [('two', 2), ('three', 3)])
def test_merged_round_on_the_tiny_mass_group(engs, key, nd):
    check_candidate_shards(engs, JC.TINY, key, 5000, 1, nd)


# -- 4. replication ---------------------------------------------------------------------
def test_set_and_clear_reach_every_device(engs):
    one, two = engs('one'), engs('two')
    single, _ = reference(one, 'd20', 4096)
    one.clear_joint_groups()
    set_named(one, 'd20')
    two.clear_joint_groups()
    set_named(two, 'd20')
    # (the second shard's winner comes from the second device's replica)
    assert same_single(two.joint_suggest(SEED, 4096, round=5), single)
    assert two.joint_last_shards() == (1, 2)
    for side in (0, 1):
        assert same_single(two.joint_get_group(0, side), one.joint_get_group(0, side))
    buf, idx = np.zeros(64), np.zeros(64, dtype=np.int64)
    rounds = np.arange(3, dtype=np.uint32)
    for e in (one, two):
        e.clear_joint_groups()
        with pytest.raises(EngineError):
            e.joint_suggest(SEED, 4096, round=5)
        with pytest.raises(EngineError):
            e.joint_get_group(0, 0)
        assert e.lib.tpe_joint_suggest_batch(e.h, 0, rounds.ctypes.data, 3, 4096, buf.ctypes.data, idx.ctypes.data,
                                             buf.ctypes.data, buf.ctypes.data) == L.TPE_ERR_ARG


def test_sampler_error_on_a_multi_device_engine(engs):
    """A box that holds none of the below mass: set_joint_group raises it on
    the multi-device engine as on one device, and so does the round."""
    dims, wb, mub, sigb, wa, mua, siga = JC.engine_args(JC.group('d1_prior'))
    far = mub + 1e6 * (dims['high'][0] - dims['low'][0])
    for key in ('one', 'two'):
        e = engs(key)
        e.clear_joint_groups()
        with pytest.raises(EngineError, match='truncated sampler'):
            e.set_joint_group(0, L.TPE_JOINT_STREAM, dims, wb, far, np.full_like(sigb, 1e-3), wa, mua, siga)
        with pytest.raises(EngineError, match='truncated sampler'):
            e.joint_suggest(0, 4096)
        e.clear_joint_groups()


# -- 5. the device build behind a multi-device univariate build -----------------------------
BUILD_ROUNDS = [3, 0, 4294967295]
BUILD_ENGINES = ['two', 'three', 'two_replicated', real2]


def build_on(eng, specs, view, groups, quantized=False, categorical=False, bandwidth='neighbour'):
    """The univariate posterior of `view` built on the engine's device(s),
    the joint groups from it under `bandwidth`: (flags, {slot: both sides'
    unfolded arrays}, the 4096-candidate rounds of the built slots)."""
    names = list(specs)
    table = [(s.label, s.kind, s.args) for s in specs.values()]
    P.DeviceHistoryUploader().build(eng, table, view, BG.GAMMA, BG.PW)
    args, kw = tpe._joint_device_args(specs, names, groups, quantized, categorical, BG.PW, bandwidth)
    eng.clear_joint_groups()
    flags = [int(f) for f in eng.build_joint_groups(args, **kw)]
    built = [slot for (slot, _), f in zip(groups, flags) if not f]
    for (slot, _), f in zip(groups, flags):
        if f:
            with pytest.raises(EngineError):
                eng.joint_get_group(slot, 0)
    mix = {slot: [eng.joint_get_group(slot, side) for side in (0, 1)] for slot in built}
    assert sorted(eng.joint_slots) == sorted(built)
    rounds = eng.joint_suggest_batch(SEED, BUILD_ROUNDS, 4096) if built else {}
    return flags, mix, rounds


def check_build(engs, key, specs, view, groups, want_flags=None, **kw):
    names = list(specs)
    ref_flags, ref_mix, ref_rounds = build_on(engs('one'), specs, view, groups, **kw)
    assert ref_flags == (list(want_flags) if want_flags is not None else [0] * len(groups))
    e = engs(key)
    flags, mix, rounds = build_on(e, specs, view, groups, **kw)
    where = [e.lib.tpe_label_device(e.h, li) for li in range(len(names))]
    if key == 'two_replicated':
        assert set(where) == {-1}
    else:   # label shards: a group's labels really sit on different devices
        assert min(where) >= 0 and len(set(where)) == len(DEVICES[key]), where
        assert any(len(set(where[names.index(k)] for k in g)) > 1 for _, g in groups), (groups, where)
    assert flags == ref_flags
    assert sorted(mix) == sorted(ref_mix)
    for slot in mix:
        for side in (0, 1):
            for name, a, b in zip(('W', 'mu', 'sigma'), mix[slot][side], ref_mix[slot][side]):
                assert a.shape == b.shape and np.array_equal(a, b), (key, slot, side, name)
    if ref_rounds:
        assert e.joint_last_shards() == (1, len(DEVICES[key]))
    assert same_batch(rounds, ref_rounds)


EIGHT = ['uniform', 'loguniform', 'normal', 'lognormal'] * 2


@pytest.mark.parametrize('key', BUILD_ENGINES)
@pytest.mark.parametrize('n', [300, 2000])
def test_build_four_kinds_twice(engs, key, n):
    specs = BG.dense_specs(EIGHT)
    check_build(engs, key, specs, BG.make_view(specs, n, 60 + n), [(0, list(specs))])


@pytest.mark.parametrize('key', BUILD_ENGINES)
def test_build_mixed_quantized_group(engs, key):
    specs = BG.dense_specs(['uniform', 'quniform', 'normal'])
    view = BG.make_view(specs, 60, 31)
    assert len(set(view[3]['h1'][1])) == 60
    check_build(engs, key, specs, view, [(0, list(specs))], quantized=True)


@pytest.mark.parametrize('key', BUILD_ENGINES)
def test_build_mixed_categorical_group(engs, key):
    specs = collections.OrderedDict([('lr', BG.Spec('lr', 'loguniform', BG.ARGS['loguniform'])),
                                     ('opt', BG.Spec('opt', 'randint', BG.ARGS['randint'])),
                                     ('pc', BG.Spec('pc', 'categorical', dict(upper=3, p=[0.2, 0.5, 0.3])))])
    check_build(engs, key, specs, BG.make_view(specs, 60, 21), [(0, list(specs))], categorical=True)


@pytest.mark.parametrize('key', BUILD_ENGINES)
def test_build_conditional_groups(engs, key):
    domain, specs, view = BG.conditional_case(60, 11, False, False)
    groups = tpe.joint_groups(domain, specs, view[3])
    assert groups == GC.GROUPS and len(groups) >= 2
    check_build(engs, key, specs, view, groups)


@pytest.mark.parametrize('bandwidth', ['neighbour', 'scott'])
def test_build_on_a_device_that_owns_no_dimension(engs, bandwidth):
    """Three labels on three devices and one group of the first two: the
    third device gathers nothing -- an empty task list, no gather launch -- and
    still fetches, interleaves, folds and commits its replica, which scores a
    third of every round's candidates."""
    specs = BG.dense_specs(['uniform', 'normal', 'lognormal'])
    check_build(engs, 'three', specs, BG.make_view(specs, 40, 47), [(0, ['h0', 'h1'])], bandwidth=bandwidth)
    e = engs('three')
    where = [e.lib.tpe_label_device(e.h, li) for li in range(3)]
    assert where[2] not in where[:2], where


FOUR = ['uniform', 'normal', 'lognormal', 'uniform']
TWO_GROUPS = [(0, ['h0', 'h1']), (3, ['h2', 'h3'])]


def missing_trial_view(specs):
    """h1 misses one above trial: its side counts are not the group's."""
    view = BG.make_view(specs, 40, 45)
    keep = np.arange(40) != int(np.argmax(view[1]))
    view[3]['h1'] = (view[3]['h1'][0][keep], view[3]['h1'][1][keep])
    return view


@pytest.mark.parametrize('key', BUILD_ENGINES)
@pytest.mark.parametrize('case', ['tie_below', 'tie_above_no_order', 'side_counts'])
def test_build_flagged_groups(engs, key, case):
    """The flags of one device, OR-ed over the devices; the flagged group is
    unset on every device and the other group of the call is built."""
    specs = BG.dense_specs(FOUR)
    if case == 'tie_below':
        view, flag = BG.tie_view(specs, 40, 41, 0), L.TPE_JOINT_FLAG_TIE
    elif case == 'tie_above_no_order':   # (n_above = 18 <= 25: built without the tie's order)
        view, flag = BG.tie_view(specs, 20, 42, 1), L.TPE_JOINT_FLAG_TIE
    else:
        view, flag = missing_trial_view(specs), L.TPE_JOINT_FLAG_COUNT
    check_build(engs, key, specs, view, TWO_GROUPS, want_flags=[flag, 0])
    e = engs(key)
    with pytest.raises(EngineError):   # (unset on every device: no shard finds it)
        e.joint_suggest(SEED, 4096, slot=0)
    assert e.joint_suggest(SEED, 4096, slot=3)[1] >= 0


# -- 6. end to end ------------------------------------------------------------------------
def test_fmin_multivariate_on_several_devices(caplog):
    """40 evaluations on a space with a uniform, a loguniform, a quniform and
    a choice with inner labels: the documents of one device and of two, of the
    device and of the host builder, are the same trial by trial."""
    runs = {}
    for devs in ([0], [0, 0]):
        for builder in ('device', 'host'):
            algo = partial(tpe.suggest, multivariate=True, group=True, joint_quantized=True, joint_categorical=True,
                           n_EI_candidates=4096, devices=devs, posterior_builder=builder)
            trials = H.Trials()
            caplog.clear()
            with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
                H.fmin(BG.e2e_loss, BG.e2e_space(), algo=algo, max_evals=40, trials=trials,
                       rstate=np.random.RandomState(5))
            assert len(trials) == 40
            runs[(len(devs), builder)] = [t['misc']['vals'] for t in trials.trials]
            on_device = [r.getMessage() for r in caplog.records if 'group(s) built on the device' in r.getMessage()]
            assert on_device
            counts = [int(m.split('multivariate TPE: ')[1].split(' ')[0]) for m in on_device]
            if builder == 'device':
                assert max(counts) >= 1, 'no group was built on the device with devices=%r' % (devs,)
            else:
                assert max(counts) == 0
    first = runs[(1, 'host')]
    for key, vals in runs.items():
        assert vals == first, key
