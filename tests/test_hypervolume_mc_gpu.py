"""tpe_mo_exclusive_mc (hyperopt_amd/csrc/tpe_mo_hvm.hip) through Engine.mo_exclusive_mc and
tpe.hypervolume(method='sampled', builder='device'), on tests/mo_hvm_reference.py's cases and integers."""
import ctypes

import numpy as np
import pytest

from tests import mo_hvm_reference as R
from tests.test_hypervolume_mc_host import check_public

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', R.CASES)
def test_the_kernel_gives_the_reference_integers(eng, name, mode):
    R.check_case(eng.mo_exclusive_mc, name, mode)


@pytest.mark.parametrize('mode', R.MODES)
def test_the_kernel_on_floats_gives_the_host_integers(eng, mode):
    """300 uniform rows, five objectives: the device's fp64 difference, quotient, product and ceil are numpy's."""
    from hyperopt_amd import posterior as P
    F, ref = R.float_rows(), (1.0,) * 5
    count, covered = eng.mo_exclusive_mc(F, ref, mode, 64 * 65)
    want, want_covered = P.mo_exclusive_mc(F, ref, mode, 64 * 65)
    assert np.array_equal(count, want) and covered == want_covered and 0 < covered < 64 * 65


@pytest.mark.parametrize('M', (2, 3, 4))
def test_the_estimate_lies_within_five_standard_deviations_of_the_exact_volume(eng, M):
    R.check_estimator(eng.mo_exclusive_mc, M)


def test_the_public_function_gives_the_same_dict_on_both_builders():
    host, dev = R.public('host', n_samples=64 * 65), R.public('device', n_samples=64 * 65)
    check_public(*dev)
    host, dev = host[0], dev[0]
    assert sorted(host) == sorted(dev) and list(host['contributions']) == list(dev['contributions'])
    for key in host:
        assert np.array_equal(host[key], dev[key]) if key == 'history' else host[key] == dev[key]


def test_abi_errors_and_buffers():
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import Engine
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    F, ref, out = np.ones((10, 5)), np.full(5, 2.0), np.full(10, 7, dtype=np.uint64)
    cov, alive = np.full(1, 7, dtype=np.uint64), ctypes.c_int32(7)
    bad_ref = np.array([2.0, 2.0, 2.0, 2.0, np.inf])
    eng = Engine(0, 'f64')
    for f, n, M, r, mode, S, o, c in ((None, 10, 5, ref, 0, 64, out, cov), (F, 10, 5, None, 0, 64, out, cov),
                                      (F, 10, 5, ref, 0, 64, None, cov), (F, 10, 5, ref, 0, 64, out, None),
                                      (F, 0, 5, ref, 0, 64, out, cov), (F, (1 << 20) + 1, 5, ref, 1, 64, out, cov),
                                      (F, 10, 1, ref, 0, 64, out, cov), (F, 10, 9, ref, 0, 64, out, cov),
                                      (F, 10, 5, bad_ref, 0, 64, out, cov), (F, 10, 5, ref, 2, 64, out, cov),
                                      (F, 10, 5, ref, 0, 0, out, cov), (F, 10, 5, ref, 0, 100, out, cov),
                                      (F, 10, 5, ref, 0, (1 << 20) + 64, out, cov)):
        assert eng.lib.tpe_mo_exclusive_mc(eng.h, p(f), n, M, p(r), None, 0, mode, S, p(o), p(c),
                                           ctypes.byref(alive)) == L.TPE_ERR_ARG
        assert b'tpe_mo_exclusive_mc' in eng.lib.tpe_last_error(eng.h)
    assert eng.lib.tpe_mo_exclusive_mc(eng.h, p(F), 10, 5, p(ref), p(F), 9, 0, 64, p(out), p(cov),
                                       ctypes.byref(alive)) == L.TPE_ERR_ARG
    assert (out == 7).all() and cov[0] == 7 and alive.value == 7 and L.ABI_VERSION == 5
    F = np.random.RandomState(3).uniform(size=(3000, 5))
    held = eng.device_bytes()
    eng.mo_exclusive_mc(F, (1.0,) * 5, 'before', 4096)
    more = eng.device_bytes()
    assert more - held >= 3000 * (8 * 4 + 4 + 4) + 4096 * 8
    eng.mo_exclusive_mc(F, (1.0,) * 5, 'others', 4096)
    assert eng.device_bytes() == more
    eng.close()
