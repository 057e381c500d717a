"""multivariate=True with several devices, the part that needs no GPU: the
keyword combination is accepted where the listed devices exist (it used to
raise ValueError always, and still does for a device the machine lacks), and
the C ABI declares the diagnostic the multi-device joint rounds are tested
through."""
import os

import pytest

from hyperopt_amd import _lib as L
from hyperopt_amd import engine, hp, rand, tpe
from hyperopt_amd.base import Domain, Trials

HERE = os.path.dirname(os.path.abspath(__file__))


def _domain():
    return Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'y': hp.normal('y', 0, 1)})


def test_multi_device_multivariate_is_accepted(monkeypatch):
    """With both devices on the machine the call no longer raises: in the
    startup phase it is rand.suggest's whatever the devices (no engine is made)."""
    import torch
    monkeypatch.setattr(torch.cuda, 'device_count', lambda: 2)
    assert engine.missing_devices([0, 1]) == []
    got = tpe.suggest([0], _domain(), Trials(), 0, devices=[0, 1], multivariate=True, group=True,
                      joint_quantized=True)
    want = rand.suggest([0], _domain(), Trials(), 0)
    assert [d['misc']['vals'] for d in got] == [d['misc']['vals'] for d in want]


def test_multi_device_multivariate_needs_its_devices(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'device_count', lambda: 2)
    assert engine.missing_devices([0, 2, -1, 1]) == [2, -1]
    with pytest.raises(ValueError, match=r'no GPU \[2\]'):
        tpe.suggest([0], _domain(), Trials(), 0, devices=[0, 2], multivariate=True)
    # the independent call and a single device are not checked here, as before
    assert tpe.suggest([0], _domain(), Trials(), 0, devices=[0, 2])
    assert tpe.suggest([0], _domain(), Trials(), 0, devices=[2], multivariate=True)


def test_last_shards_is_declared():
    assert 'tpe_joint_last_shards' in L.SIGNATURES
    with open(os.path.join(HERE, '..', 'include', 'hyperopt_tpe.h')) as f:
        header = f.read()
    assert 'int tpe_joint_last_shards(const tpe_ctx *ctx, int32_t *mode, int32_t *n_devices);' in header
