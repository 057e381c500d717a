"""The Scott-rule bandwidth of joint groups on multi-device contexts (`-m
gpu`): Engine([0, 0]) -- two contexts on the one GPU, as in
test_joint_multi_gpu.py -- with label shards (the owners gather their labels'
columns, the owner of the first non-categorical label the W column) and
without (every device builds its replica).  The unfolded mixtures
(joint_get_group answers from the primary device), the rounds split over
both devices' replicas and tpe.suggest's documents are the one-device ones,
np.array_equal.
(The peer copy between two real cards is the neighbour rule's, unchanged, and
as unmeasured here as there.)"""
from functools import partial

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import posterior as P
from hyperopt_amd import tpe
from tests import test_joint_bandwidth_host as BH
from tests import test_joint_build_gpu as BG

pytestmark = pytest.mark.gpu

PW = BH.PW
SEED, ROUNDS = 19, [3, 0, 4294967295]


@pytest.fixture(scope='module')
def engs():
    from hyperopt_amd.engine import Engine
    made = {'one': Engine(0, 'f64'), 'sharded': Engine([0, 0], 'f64'), 'replicated': Engine([0, 0], 'f64')}
    made['replicated'].set_option('label_shards', 0)
    yield made
    for e in made.values():
        e.close()


def build_on(eng, specs, view, groups, **kinds):
    names = list(specs)
    table = [(s.label, s.kind, s.args) for s in specs.values()]
    P.DeviceHistoryUploader().build(eng, table, view, BG.GAMMA, PW)
    args, kw = tpe._joint_device_args(specs, names, groups, kinds.get('quantized', False),
                                      kinds.get('categorical', False), PW, 'scott')
    eng.clear_joint_groups()
    assert list(eng.build_joint_groups(args, **kw)) == [0] * len(groups)
    mix = {slot: [eng.joint_get_group(slot, side) for side in (0, 1)] for slot, _ in groups}
    return mix, eng.joint_suggest_batch(SEED, ROUNDS, 4096)


def view_of(specs, n, seed):
    tids, losses, cols = BH.history(specs, n, seed)
    return tids, losses, n, dict(cols), BG.Owner()


CASES = {'five_300': (BH.GROUPS['five'], 300, dict(quantized=True)),
         'choice_first_60': (BH.GROUPS['choice_loguniform'] + ['normal'], 60, dict(categorical=True)),
         'dense_26': (['uniform', 'loguniform', 'normal', 'lognormal'], 28, dict())}


@pytest.mark.parametrize('key', ['sharded', 'replicated'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_build_equals_one_device(engs, key, case):
    kinds, n, kw = CASES[case]
    specs = BH.specs_of(kinds)
    view = view_of(specs, n, 400 + n)
    groups = [(0, list(specs))]
    ref_mix, ref_rounds = build_on(engs['one'], specs, view, groups, **kw)
    e = engs[key]
    mix, rounds = build_on(e, specs, view, groups, **kw)
    where = [e.lib.tpe_label_device(e.h, li) for li in range(len(specs))]
    if key == 'replicated':
        assert set(where) == {-1}
    else:   # the group's labels really sit on both devices
        assert sorted(set(where)) == [0, 1], where
    for side in (0, 1):
        for name, a, b in zip(('W', 'mu', 'sigma'), mix[0][side], ref_mix[0][side]):
            assert a.shape == b.shape and np.array_equal(a, b), (key, side, name)
    # the second device's replica: the rounds ran as candidate shards, half of the
    # 4096 candidates scored against it, and are the one-device rounds bit for bit
    assert e.joint_last_shards() == (1, 2)
    assert sorted(rounds) == sorted(ref_rounds) == [0]
    assert all(np.array_equal(a, b) for a, b in zip(rounds[0], ref_rounds[0]))


def test_suggest_on_two_devices_returns_the_one_device_documents():
    runs = {}
    for devs in ([0], [0, 0]):
        algo = partial(tpe.suggest, multivariate=True, group=True, joint_quantized=True, joint_categorical=True,
                       joint_bandwidth='scott', n_EI_candidates=4096, devices=devs, posterior_builder='device')
        trials = H.Trials()
        H.fmin(BG.e2e_loss, BG.e2e_space(), algo=algo, max_evals=32, trials=trials, rstate=np.random.RandomState(5))
        assert len(trials) == 32
        runs[len(devs)] = [t['misc']['vals'] for t in trials.trials]
    assert runs[1] == runs[2]
