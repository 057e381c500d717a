"""tpe_mo_exclusive4 (hyperopt_amd/csrc/tpe_mo_hvx4.hip) through Engine.mo_exclusive and
tpe.hypervolume(builder='device'), on tests/test_hypervolume4_host.py's cases and exact reference."""
import ctypes

import numpy as np
import pytest

from tests import test_hypervolume4_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


@pytest.mark.parametrize('mode', H.MODES)
@pytest.mark.parametrize('name', H.CASES)
def test_the_kernel_gives_the_exact_integers(eng, name, mode):
    H.check_case(lambda *a, **k: eng.mo_exclusive(*a, want_overflow=True, **k), name, mode)


def test_the_kernel_on_floats_gives_the_host_bits(eng):
    from hyperopt_amd import posterior as P
    F = H.check_floats(eng.mo_exclusive)
    for mode in H.MODES:
        assert np.array_equal(eng.mo_exclusive(F, (1.0,) * 4, mode), P.mo_exclusive(F, (1.0,) * 4, mode))


def test_a_kept_set_past_the_capacity_is_recomputed_on_the_host():
    """The simplex, 'others', a capacity of 1 point: the numpy builder's column, the count reported."""
    from hyperopt_amd import posterior as P
    from hyperopt_amd.engine import Engine
    F, _, ref = H.case('simplex')
    want = P.mo_exclusive(F, (float(ref),) * 4, 'others')
    e = Engine(0, 'f64')
    e.set_option('mo_hvx_cap', 1)
    merged, n_over = e.mo_exclusive(F, (float(ref),) * 4, 'others', want_overflow=True)
    e.close()
    assert 0 < n_over <= len(F) and np.array_equal(merged, want) and (want > 0).all()


def test_the_public_function_gives_the_same_dict_on_both_builders():
    host, dev = H.check_public('host'), H.check_public('device')
    assert sorted(host) == sorted(dev) and list(host['contributions']) == list(dev['contributions'])
    for key in host:
        assert np.array_equal(host[key], dev[key]) if key == 'history' else host[key] == dev[key]


def test_abi_errors_and_buffers():
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import Engine
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    F, ref, out, n_over = np.ones((10, 4)), np.full(4, 2.0), np.full(10, 7.0), ctypes.c_int32(7)
    bad_ref = np.array([2.0, 2.0, 2.0, np.inf])
    eng = Engine(0, 'f64')
    for f, n, M, r, mode, o in ((None, 10, 4, ref, 0, out), (F, 10, 4, None, 0, out), (F, 10, 4, ref, 0, None),
                                (F, 0, 4, ref, 0, out), (F, (1 << 20) + 1, 4, ref, 1, out),
                                (F, 10, 3, ref, 0, out), (F, 10, 4, bad_ref, 0, out), (F, 10, 4, ref, 2, out)):
        assert eng.lib.tpe_mo_exclusive4(eng.h, p(f), n, M, p(r), None, 0, mode, p(o),
                                         ctypes.byref(n_over)) == L.TPE_ERR_ARG
        assert b'tpe_mo_exclusive4' in eng.lib.tpe_last_error(eng.h)
    assert (out == 7.0).all() and n_over.value == 7 and L.ABI_VERSION == 5
    F = np.random.RandomState(3).uniform(size=(3000, 4))
    held = eng.device_bytes()
    eng.mo_exclusive(F, (1.0,) * 4, 'before')
    more = eng.device_bytes()
    assert more - held >= 3000 * (4 * 8 + 4 + 4 + 8) + 2 * 4
    eng.mo_exclusive(F, (1.0,) * 4, 'others')
    assert eng.device_bytes() == more
    eng.close()
