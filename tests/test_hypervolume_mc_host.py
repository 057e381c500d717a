"""tpe.hypervolume(method='sampled') and its numpy builder (posterior.mo_exclusive_mc) against the plain
reference of tests/mo_hvm_reference.py: integer counts on the fixed sample set."""
import numpy as np
import pytest

from tests import mo_hvm_reference as R


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', R.CASES)
def test_the_numpy_builder_gives_the_reference_integers(name, mode):
    from hyperopt_amd import posterior as P
    R.check_case(P.mo_exclusive_mc, name, mode)


@pytest.mark.parametrize('M', (2, 3, 4))
def test_the_estimate_lies_within_five_standard_deviations_of_the_exact_volume(M):
    from hyperopt_amd import posterior as P
    R.check_estimator(P.mo_exclusive_mc, M)


def check_public(got, want, trials):
    V, S = want['V'], got['n_samples']
    assert got['method'] == 'sampled' and got['skipped'] == 2 and 0 < V <= 101.0 ** 5
    assert got['hypervolume'] == V * want['covered'] / S == got['history'][-1] > 0
    assert (np.diff(got['history']) >= 0).all() and got['history'][4] == got['history'][3]
    assert got['history'].tolist() == [V * float(c) / S for c in np.cumsum(want['before'])]
    p = want['covered'] / S
    assert got['stderr'] == V * float(np.sqrt(p * (1 - p) / S))
    tids = got['tids']
    pairs = sorted(((-V * float(c) / S, tids[i]) for i, c in enumerate(want['others']) if c))
    assert list(got['contributions'].items()) == [(t, -v) for v, t in pairs] and pairs
    assert trials.trials[4]['tid'] not in got['contributions']


def test_the_public_function_on_the_host(monkeypatch):
    from hyperopt_amd import engine, tpe
    monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    got, want, trials = R.public('host', n_samples=64 * 65)
    check_public(got, want, trials)
    assert R.public('host')[0]['n_samples'] == 65536
    names = ('loss', 'latency', 'memory', 'energy', 'cost')
    for kw, match in ((dict(method='mc'), 'method must be'), (dict(n_samples=128), "needs method='sampled'"),
                      (dict(method='sampled', n_samples=100), 'multiple of 64'),
                      (dict(method='sampled', n_samples=True), 'multiple of 64'),
                      (dict(method='sampled', n_samples=1 << 21), 'multiple of 64'),
                      (dict(method='sampled', objectives=('loss',)), '2 .. 8 objectives'),
                      (dict(method='sampled', objectives=tuple('abcdefghi')), 'at most 8'),
                      (dict(), '2, 3 or 4 objectives')):
        with pytest.raises(ValueError, match=match):
            tpe.hypervolume(trials, kw.pop('objectives', names), builder='device', **kw)
