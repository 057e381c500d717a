"""The device-resident history (tpe_history_reset / tpe_history_append: k_hist_append,
the segmented or chip-wide sort of the new batch, k_hist_merge, k_hist_regrow)
read back with the diagnostic Engine.history_get and compared, append by
append, with the numpy model of tests/history_reference.py -- counts, trial
positions and values bit for bit (signed zeros included), the sorted view
equal to the stable argsort, regions large enough and disjoint -- and the
mixtures built from it with the CPU oracle in both tie orders.  Everything is
exact: no tolerances.  The scenarios are tests/history_cases.py; their
preconditions are asserted on the host (tests/test_history_cases_host.py).

Timing on an MI355X, same run (pytest --durations=0): test_stepwise 2.1 s
(522 appends with 14 readbacks each, 193 steps with two builds and two
oracle passes, the oracle 0.5 s of it), test_shards_and_replicas 2.1 s (four
contexts), every other case below 0.1 s;
test_gpu_build.py::test_resident_history_incremental 0.04 s.  The two long
cases keep the check schedule their sequences were given; beyond the oracle
their time is device calls (readbacks, builds, get_mixture)."""
import numpy as np
import pytest

from tests import history_cases as C
from tests.helpers import ALL_KINDS, _check_bit_exact
from tests.history_reference import PoolModel

pytestmark = pytest.mark.gpu

GAMMA, PW, LF = 0.25, 1.0, 25


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


def _reset(e, labels):
    from hyperopt_amd import posterior as P
    specs, cat_p, _ = P.spec_table(labels)
    e.history_reset(specs, cat_p)


def _append(e, model, st):
    e.history_append(st.n_new, st.trial, st.val)
    if model is not None:
        model.append(st.n_new, st.trial, st.val, st.raw)


def _check_readback(e, model, device=0):
    """Engine.history_get of every label equals the model; returns what was
    read (for comparing replicas and engines)."""
    got, regions = [], {}
    for l in range(len(model.labels)):
        trial, val, key, idx, cap, off = e.history_get(l, device)
        name = model.labels[l][0]
        assert len(trial) == len(val) == model.count(l), (name, len(trial), model.count(l))
        assert np.array_equal(trial, model.trial[l]), name
        assert np.array_equal(val.view(np.uint64), model.val[l].view(np.uint64)), name
        view = model.sorted_view(l)
        if view is None:
            assert len(key) == 0 and len(idx) == 0, name
        else:
            assert np.array_equal(idx, view[0]), (name, 'sorted order')
            assert np.array_equal(key.view(np.uint64), val[idx].view(np.uint64)), (name, 'keys')
        assert cap >= model.count(l) and off >= 0, (name, cap, off)
        d = e.lib.tpe_label_device(e.h, l)          # (-1: one pool, or one per replica)
        regions.setdefault(d, []).append((off, cap, name))
        got.append((trial, val, key, idx))
    for regs in regions.values():                   # regions of one pool do not overlap
        regs = sorted(r for r in regs if r[1] > 0)
        for (a, ca, na), (b, _, nb) in zip(regs, regs[1:]):
            assert a + ca <= b, (na, nb)
    return got


def _mixtures(e, n_labels):
    return [e.get_mixture(l, side) for l in range(n_labels) for side in (0, 1)]


def _same_mixtures(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))


def _check_builds(e, model, losses, oracle=True):
    """build_posterior_resident (ties by position) against the stable-order
    oracle, then posterior.build_reference_order against the default-order
    oracle.  Returns (labels that needed numpy's order, the two sets of
    mixtures)."""
    from hyperopt_amd import posterior as P
    losses = np.asarray(losses, float)
    n_valid = int(np.count_nonzero(losses == losses))
    nb = e.build_posterior_resident(losses, n_valid, GAMMA, PW)
    assert nb == C.n_below_of(losses)
    if oracle:
        h, want = model.mixtures(losses, 'stable', GAMMA, PW)
        _check_bit_exact(e, h, want)
    first = _mixtures(e, len(model.labels))
    nb, need = P.build_reference_order(e, losses, n_valid, GAMMA, PW, LF, model.obs_of())
    assert nb == C.n_below_of(losses)
    if oracle:
        h, want = model.mixtures(losses, None, GAMMA, PW)
        _check_bit_exact(e, h, want)
    return need, (first, _mixtures(e, len(model.labels)))


def _run(e, scn, check=None):
    """Reset, then every append with the readback check; the builds at the
    steps in `check` (default: all).  Returns (model, tie labels seen)."""
    model = PoolModel(scn.labels)
    _reset(e, scn.labels)
    seen = set()
    for k, st in enumerate(scn.steps):
        _append(e, model, st)
        _check_readback(e, model)
        if check is None or k in check:
            seen |= set(_check_builds(e, model, st.losses)[0])
    return model, seen


def test_stepwise(eng):
    """One trial per append across both regrows of `every`: the readback
    after every append, the mixtures at the steps of oracle_steps."""
    scn = C.stepwise()
    _, seen = _run(eng, scn, set(C.oracle_steps(scn)))
    assert seen                                        # numpy's tie order was needed somewhere


@pytest.mark.parametrize('total', [4095, 4096, 4097])
def test_sort_switch(eng, total):
    """A bulk append staging exactly `total` observations (segmented sort
    below kGlobalSortMin = 4096, two chip-wide sorts from it), then a small
    append merged over the bulk-sorted view."""
    _run(eng, C.threshold(total))


def test_merge_edges(eng):
    _run(eng, C.merge_edges())


def test_lone_regrow(eng):
    _run(eng, C.lone_regrow())


def test_reuse_after_reset(eng):
    """history_reset with fewer, then with more labels after a long history:
    nothing of the old one shows."""
    old = C.stepwise(stride=9)
    _reset(eng, old.labels)
    m = PoolModel(old.labels)
    for st in old.steps:
        _append(eng, m, st)
    _check_readback(eng, m)
    for scn in (C.short(C.LABELS[:5], 31), C.short(C.LABELS + C.EXTRA, 32)):
        _reset(eng, scn.labels)
        _check_readback(eng, PoolModel(scn.labels))    # empty, every label
        _run(eng, scn)


def test_changing_losses_over_unchanged_pool(eng):
    """Between builds only the losses change (pending -> finite into the
    below set, pending -> finite staying above, a tie across the split made
    and removed): every rebuild equals the oracle, the pool stays as it was."""
    scn = C.short(C.LABELS, 17, n=200, cuts=(200,))
    model = PoolModel(scn.labels)
    _reset(eng, scn.labels)
    _append(eng, model, scn.steps[0])
    before = _check_readback(eng, model)
    base = scn.steps[0].losses + 1e-6 * np.arange(200)       # distinct losses
    fin = np.flatnonzero(np.isfinite(base))
    a, b, c = (int(t) for t in fin[[20, 21, 60]])
    l0 = base.copy()
    l0[[a, b]] = np.inf
    l1 = l0.copy()
    l1[a] = np.nanmin(base) - 1.0                            # enters the below set
    l2 = l1.copy()
    l2[b] = np.nanmax(base[np.isfinite(base)]) + 1.0         # stays above
    nb = C.n_below_of(l2)
    s = np.sort(l2[l2 == l2])
    assert l2[c] > s[nb] and not C.split_tie(l2)
    l3 = l2.copy()
    l3[c] = s[nb - 1]                                        # a tie across the split
    assert C.split_tie(l3)
    l4 = l3.copy()
    l4[c] = s[nb - 1] + 5e-7                                 # ... and gone again
    assert not C.split_tie(l4)
    for losses in (l0, l1, l2, l3, l4):
        _check_builds(eng, model, losses)
    after = _check_readback(eng, model)
    for x, y in zip(before, after):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))


def test_guarded_errors_leave_engine_usable():
    """The inputs the library rejects without touching memory: a negative
    count, an append before a reset, a trial position past the losses at
    build time (k_partition's err word).  After a reset and a correct upload
    the build equals the oracle."""
    from hyperopt_amd.engine import Engine, EngineError
    scn = C.short(C.LABELS, 19)
    e = Engine(0, 'f64')
    try:
        L = len(scn.labels)
        with pytest.raises((EngineError, ValueError)):       # before any reset
            e.history_append(np.zeros(L, np.int64), np.zeros(0, np.int32), np.zeros(0))
        _reset(e, scn.labels)
        bad = np.zeros(L, np.int64)
        bad[2] = -1
        with pytest.raises((EngineError, ValueError)):
            e.history_append(bad, np.zeros(0, np.int32), np.zeros(0))
        _run(e, scn)
        # an observation of a trial the losses do not reach
        _reset(e, scn.labels)
        model = PoolModel(scn.labels)
        for st in scn.steps:
            _append(e, model, st)
        _check_readback(e, model)
        short_losses = scn.steps[-1].losses[:30]
        assert max(int(t.max()) for t in model.trial if len(t)) >= 30
        with pytest.raises((EngineError, ValueError)):
            e.build_posterior_resident(short_losses, int(np.count_nonzero(short_losses == short_losses)),
                                       GAMMA, PW)
        _check_readback(e, model)
        _run(e, scn)
    finally:
        e.close()


def test_shards_and_replicas():
    """The thinned stepwise sequence (4 trials per append) and lone_regrow on
    two and three label shards and on a replicated context: readback equal to
    the model (so to the one-device context's) after every append, on every
    replica; mixtures equal to the one-device context's at the checked
    steps.  lone_regrow's last append leaves a shard without observations."""
    from hyperopt_amd.engine import Engine
    engs = [Engine(0), Engine([0, 0]), Engine([0, 0, 0]), Engine([0, 0])]
    engs[3].set_option('label_shards', 0)
    try:
        for scn in (C.stepwise(stride=4), C.lone_regrow()):
            check = set(C.oracle_steps(scn))
            model = PoolModel(scn.labels)
            L = len(scn.labels)
            for e in engs:
                _reset(e, scn.labels)
            lib = engs[0].lib
            assert sorted({lib.tpe_label_device(engs[1].h, l) for l in range(L)}) == [0, 1]
            assert sorted({lib.tpe_label_device(engs[2].h, l) for l in range(L)}) == [0, 1, 2]
            assert {lib.tpe_label_device(engs[3].h, l) for l in range(L)} == {-1}
            for k, st in enumerate(scn.steps):
                model.append(st.n_new, st.trial, st.val, st.raw)
                for e in engs:
                    _append(e, None, st)
                for e in engs[:3]:
                    _check_readback(e, model)
                for d in (0, 1):
                    _check_readback(engs[3], model, device=d)
                if k in check:
                    _, ref = _check_builds(engs[0], model, st.losses)
                    for e in engs[1:]:
                        _, got = _check_builds(e, model, st.losses, oracle=False)
                        _same_mixtures(got[0], ref[0])
                        _same_mixtures(got[1], ref[1])
            if scn.name == 'lone_regrow':
                fed = np.flatnonzero(scn.steps[-1].n_new)
                for e, nd in ((engs[1], 2), (engs[2], 3)):
                    assert len({lib.tpe_label_device(e.h, int(l)) for l in fed}) < nd
    finally:
        for e in engs:
            e.close()


def test_two_labels_on_two_and_three_devices():
    """Exactly two labels: sharded on two devices (one label each), the
    replicated fallback on three."""
    from hyperopt_amd.engine import Engine
    labels = [ALL_KINDS[0], ALL_KINDS[5]]
    scn = C.short(labels, 23, n=300, cuts=(1, 2, 40, 299, 300), frac=1.0)
    e2, e3 = Engine([0, 0]), Engine([0, 0, 0])
    try:
        for e in (e2, e3):
            _reset(e, labels)
        assert sorted(e2.lib.tpe_label_device(e2.h, l) for l in (0, 1)) == [0, 1]
        assert [e3.lib.tpe_label_device(e3.h, l) for l in (0, 1)] == [-1, -1]
        model = PoolModel(labels)
        for st in scn.steps:
            model.append(st.n_new, st.trial, st.val, st.raw)
            _append(e2, None, st)
            _append(e3, None, st)
            _check_readback(e2, model)
            for d in (0, 1, 2):
                _check_readback(e3, model, device=d)
            _check_builds(e2, model, st.losses)
            _check_builds(e3, model, st.losses)
    finally:
        e2.close()
        e3.close()


def test_report_after_sharded_subset_rebuild():
    """A full ordered build, then tpe_rebuild_labels of labels that all lie
    on one shard: build_report() of the sharded context equals the
    one-device context's and what rebuild_labels returned (a skipped device
    used to keep the previous build's tie bits)."""
    from hyperopt_amd import posterior as P
    from hyperopt_amd.engine import Engine
    scn = C.short(C.LABELS, 41, n=400, cuts=(400,))
    losses = scn.steps[0].losses + 1e-6 * np.arange(400)     # no tie across the split
    n_valid = int(np.count_nonzero(losses == losses))
    one, two = Engine(0), Engine([0, 0])
    try:
        model = PoolModel(scn.labels)
        model.append(scn.steps[0].n_new, scn.steps[0].trial, scn.steps[0].val, scn.steps[0].raw)
        full = []
        for e in (one, two):
            _reset(e, scn.labels)
            _append(e, None, scn.steps[0])
            _check_readback(e, model)
            full.append(e.build_posterior_ordered(losses, n_valid, GAMMA, PW, LF))
        assert full[0][0] == full[1][0] and np.array_equal(full[0][1], full[1][1])
        nb, ties = full[0]
        assert ties[-1] == 0
        need = [int(l) for l in np.flatnonzero(ties[:-1] & 2)]
        devs = [two.lib.tpe_label_device(two.h, l) for l in need]
        assert sorted(set(devs)) == [0, 1]                   # flagged labels on both shards
        subset = [l for l, d in zip(need, devs) if d == devs[0]]
        _, off, order = P.reference_orders(losses, nb, model.obs_of(), set(subset))
        r1 = one.rebuild_labels(losses, n_valid, GAMMA, PW, LF, off, order, subset)
        r2 = two.rebuild_labels(losses, n_valid, GAMMA, PW, LF, off, order, subset)
        rep1, rep2 = one.build_report(), two.build_report()
        assert r1[0] == r2[0] == rep1[0] == rep2[0] == nb
        assert np.array_equal(r1[1], r2[1])
        assert np.array_equal(rep1[1], r1[1])
        assert np.array_equal(rep2[1], rep1[1])
        assert np.array_equal(rep2[1], r2[1])
        _same_mixtures(_mixtures(two, len(scn.labels)), _mixtures(one, len(scn.labels)))
    finally:
        one.close()
        two.close()
