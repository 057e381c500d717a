"""Several joint groups on the GPU (`-m gpu`): the batched, packed joint round
(Engine.joint_suggest_batch) against single joint_suggest calls bit for bit --
over tile, wave and workgroup boundaries, in the split and the fused layout,
chunked under a low memory cap --, its winners against the numpy definition,
the draws under a slot's own pick stream, ties, errors, and
tpe.suggest(..., multivariate=True, group=True) end to end.  Cases, seed and
rounds: tests/joint_group_cases.py (test_joint_groups_host.py checks the seed
on the CPU)."""
import ctypes
from functools import partial

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import _lib as L
from hyperopt_amd import tpe
from oracle import draw_oracle as D
from tests import joint_cases as JC
from tests import joint_group_cases as GC
from tests.draw_check import check_draws

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


def _assert_rows_equal_single(eng, got, seed, rounds, n, slots, which=None):
    """Rows `which` (default all) of a batch result against joint_suggest."""
    for slot in slots:
        values, index, ll, lg = got[slot]
        assert values.shape[0] == len(rounds) == len(index) == len(ll) == len(lg)
        for r in (range(len(rounds)) if which is None else which):
            v, i, a, b = eng.joint_suggest(seed, n, round=rounds[r], slot=slot)
            assert np.array_equal(values[r], v), (slot, r)
            assert index[r] == i and ll[r] == a and lg[r] == b, (slot, r)


# -- batch == single calls ---------------------------------------------------------
@pytest.mark.parametrize('n', GC.COUNTS)
def test_batch_equals_single_calls(eng, n):
    """Four slots -- 8 and 32 registers, LDS beside the exp table, LDS alone --
    with their own pick streams, 11 rounds: 264 flat candidates at n = 24 (a
    round straddles the 256-lane tile and every wave boundary), n = 1, n = 65
    (a round straddles the LDS variants' 64-lane workgroups), n = 300 (one
    round spans tiles); the last tile partly filled."""
    GC.set_slots(eng)
    got = eng.joint_suggest_batch(GC.SEED, GC.ROUNDS, n)
    assert sorted(got) == list(range(len(GC.SLOTS)))
    _assert_rows_equal_single(eng, got, GC.SEED, GC.ROUNDS, n, range(len(GC.SLOTS)))
    first, second = [i for i, r in enumerate(GC.ROUNDS) if r == 7]
    for slot in got:
        for arr in got[slot]:
            assert np.array_equal(arr[first], arr[second])


def _fused_rows():
    name, seed, n, R = GC.FUSED
    rows = {0, R - 1}
    for edge in (256, 512, 768):
        rows |= {(edge - 1) // n, edge // n}
    return sorted(rows)


def test_batch_fused_layout(eng):
    """132000 flat candidates in 516 tiles: one workgroup per tile runs every
    slice.  The first and last round and those on both sides of (or across)
    the first three tile boundaries against single calls."""
    name, seed, n, R = GC.FUSED
    eng.clear_joint_groups()
    eng.set_joint_group(0, L.TPE_JOINT_STREAM, *JC.engine_args(JC.group(name)))
    assert R * n >= 512 * 256
    rounds = list(range(R))
    got = eng.joint_suggest_batch(seed, rounds, n)
    _assert_rows_equal_single(eng, got, seed, rounds, n, [0], which=_fused_rows())


@pytest.mark.parametrize('n', [24, 300])
def test_batch_chunked_under_a_low_cap(n):
    """A private cap of 100 flat candidates: four rounds of 24 per packed
    launch, three chunks; rounds of 300 exceed it and run alone."""
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    try:
        e.set_option('joint_cap', 100)
        GC.set_slots(e)
        got = e.joint_suggest_batch(GC.SEED, GC.ROUNDS, n)
        _assert_rows_equal_single(e, got, GC.SEED, GC.ROUNDS, n, range(len(GC.SLOTS)))
        e.set_option('joint_cap', 0)
        whole = e.joint_suggest_batch(GC.SEED, GC.ROUNDS, n)
        for slot in got:
            for a, b in zip(got[slot], whole[slot]):
                assert np.array_equal(a, b)
    finally:
        e.close()


# -- winners and draws against the definition -------------------------------------
def test_batch_winner_is_the_reference_argmax(eng):
    """n = 24: every cell's index is numpy's argmax of the reference score on
    the device's own candidates (margins checked on the CPU)."""
    refs = GC.set_slots(eng)
    got = eng.joint_suggest_batch(GC.SEED, GC.ROUNDS, 24)
    for slot, ref in enumerate(refs):
        for r, rnd in enumerate(GC.ROUNDS):
            vals, _ = eng.joint_draw(GC.SEED, 24, round=rnd, slot=slot)
            ok, want = JC.margin_ok(ref.joint_lpdf(vals, 'below'), ref.joint_lpdf(vals, 'above'))
            assert ok, 'reference margin too small: pick another seed'
            assert got[slot][1][r] == want, (slot, rnd)
            assert np.array_equal(got[slot][0][r], vals[want])


def test_draws_under_the_slots_pick_stream(eng):
    refs = GC.set_slots(eng)
    slot, rnd, n = GC.DRAW_SLOT, 7, 65
    ref = refs[slot]
    vals, comp = eng.joint_draw(GC.SEED, n, round=rnd, slot=slot)
    g = np.arange(n, dtype=np.uint64)
    pf = ref.pick_fold()
    wp, wu = D.draw_words(GC.SEED, L.TPE_JOINT_STREAM - slot, rnd, g)
    assert not D.excluded(pf, wp, wu).any()
    assert np.array_equal(comp, D.pick(pf, wp))
    # (the default stream picks other components: the slot's stream is in use)
    assert not np.array_equal(comp, D.pick(pf, D.draw_words(GC.SEED, L.TPE_JOINT_STREAM, rnd, g)[0]))
    for d, dim in enumerate(ref.dims):
        wpd, wud = D.draw_words(GC.SEED, dim.stream, rnd, g)
        for k in np.unique(comp):
            sel = comp == k
            check_draws(ref.fold(int(k), d), wpd[sel], wud[sel], vals[sel, d], 'joint',
                        'slot %d dim %d component %d' % (slot, d, k))


@pytest.mark.parametrize('n', GC.TIE_COUNTS)
def test_batch_ties_go_to_the_lowest_index(eng, n):
    GC.set_slots(eng, ['d1_tie', 'd1_tie'])
    got = eng.joint_suggest_batch(2, GC.TIE_ROUNDS, n)
    for slot in (0, 1):
        values, index, ll, lg = got[slot]
        assert index.tolist() == [0] * len(GC.TIE_ROUNDS)
        assert np.array_equal(ll, lg)
    # (two pick streams, one component: the same candidates)
    assert np.array_equal(got[0][0], got[1][0])


# -- errors --------------------------------------------------------------------------
def test_group_errors():
    from hyperopt_amd.engine import Engine, EngineError
    e = Engine(0, 'f64')
    try:
        lib, h = e.lib, e.h
        rounds = np.arange(3, dtype=np.uint32)
        buf, idx = np.zeros(64), np.zeros(64, dtype=np.int64)

        def batch_rc():
            return lib.tpe_joint_suggest_batch(h, 0, rounds.ctypes.data, 3, 24, buf.ctypes.data, idx.ctypes.data,
                                               buf.ctypes.data, buf.ctypes.data)
        assert batch_rc() == L.TPE_ERR_ARG                      # no slot set
        with pytest.raises(EngineError):
            e.joint_suggest_batch(0, [0, 1, 2], 24)
        ref = JC.group('d1_prior')
        args = JC.engine_args(ref)
        dims, wb, mub, sigb, wa, mua, siga = args
        raw = e._joint_args(*args)
        for slot in (-1, L.TPE_JOINT_MAX_GROUPS):
            assert lib.tpe_joint_set_group(h, slot, 5, *raw) == L.TPE_ERR_ARG
            a, b, i = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
            assert lib.tpe_joint_suggest_group(h, slot, 0, 0, 24, buf.ctypes.data, ctypes.byref(i),
                                               ctypes.byref(a), ctypes.byref(b)) == L.TPE_ERR_ARG
            with pytest.raises(EngineError):
                e.set_joint_group(slot, 5, *args)
        assert batch_rc() == L.TPE_ERR_ARG                      # still none
        # a good slot 0 and a slot 1 whose box holds none of the below mass
        e.set_joint_group(0, L.TPE_JOINT_STREAM, *args)
        assert sorted(e.joint_suggest_batch(0, [0, 1, 2], 24)) == [0]
        far = mub + 1e6 * (dims['high'][0] - dims['low'][0])
        with pytest.raises(EngineError, match='truncated sampler'):
            e.set_joint_group(1, L.TPE_JOINT_STREAM - 1, dims, wb, far, np.full_like(sigb, 1e-3), wa, mua, siga)
        with pytest.raises(EngineError, match='truncated sampler'):
            e.joint_suggest_batch(0, [0, 1, 2], 24)
        assert batch_rc() == L.TPE_ERR_SAMPLE
        assert e.joint_suggest(0, 24, slot=0)[1] >= 0           # (slot 0 itself is fine)
        # set_joint_posterior: slot 0 alone
        e.set_joint_posterior(*args)
        with pytest.raises(EngineError):
            e.joint_suggest(0, 24, slot=1)
        a, b, i = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        assert lib.tpe_joint_suggest_group(h, 1, 0, 0, 24, buf.ctypes.data, ctypes.byref(i), ctypes.byref(a),
                                           ctypes.byref(b)) == L.TPE_ERR_ARG
        got = e.joint_suggest_batch(0, [0, 1, 2], 24)
        assert sorted(got) == [0]
        _assert_rows_equal_single(e, got, 0, [0, 1, 2], 24, [0])
        e.clear_joint_groups()
        assert batch_rc() == L.TPE_ERR_ARG
    finally:
        e.close()


# -- end to end ------------------------------------------------------------------------
def _run(evals=40, seed=5, **kw):
    trials = H.Trials()
    H.fmin(GC.loss, GC.space(), algo=partial(tpe.suggest, **kw), max_evals=evals, trials=trials,
           rstate=np.random.RandomState(seed))
    return trials


def _vals(docs):
    return [d['misc']['vals'] for d in docs]


def test_fmin_with_groups_end_to_end():
    trials = _run(multivariate=True, group=True)
    assert len(trials) == 40
    for doc in trials.trials:
        vals, idxs = doc['misc']['vals'], doc['misc']['idxs']
        assert set(vals) == set(idxs) == set(GC.SIGNATURES)
        for k in ('x', 'ly', 'c', 'k'):
            assert len(vals[k]) == 1 and idxs[k] == [doc['tid']]
        c0 = vals['c'][0] == 0
        inner1 = c0 and vals['inner'][0] == 1
        active = {'a': c0, 'b': c0, 'qa': c0, 'inner': c0, 'd1': inner1, 'd2': inner1, 'e': not c0,
                  'sh': vals['k'][0] in (0, 1)}
        for k, on in active.items():
            assert len(vals[k]) == len(idxs[k]) == (1 if on else 0), k
            assert idxs[k] == ([doc['tid']] if on else [])
        assert -5 <= vals['x'][0] < 5 and vals['ly'][0] > 0
        if c0:
            assert -2 <= vals['a'][0] < 2 and vals['qa'][0] % 2 == 0 and isinstance(vals['a'][0], float)
        if inner1:
            assert 0 <= vals['d1'][0] < 4 and vals['d2'][0] > 0
    again = _run(multivariate=True, group=True)
    assert _vals(again.trials) == _vals(trials.trials)
    ungrouped = _run(multivariate=True, group=False)
    assert _vals(ungrouped.trials) != _vals(trials.trials)


def test_suggest_documents_given_the_same_history():
    """One history, batch of three ids.  group=True: labels outside all
    groups equal the independent call's, each group's labels are joint_suggest
    of an engine given the same mixtures in the same slot; the device builder
    gives the same documents; group=False models slot 0 alone."""
    from hyperopt_amd.base import Domain
    from hyperopt_amd import history, posterior as P
    from hyperopt_amd.engine import Engine
    trials = _run(evals=30, seed=9)
    domain = Domain(GC.loss, GC.space())
    ids = [100, 101, 102]
    kw = dict(batch=True, posterior_builder='host')
    plain = _vals(tpe.suggest(ids, domain, trials, 17, multivariate=False, **kw))
    multi = _vals(tpe.suggest(ids, domain, trials, 17, multivariate=True, group=True, **kw))
    single = _vals(tpe.suggest(ids, domain, trials, 17, multivariate=True, group=False, **kw))
    default = _vals(tpe.suggest(ids, domain, trials, 17, multivariate=True, **kw))
    assert single == default
    specs = tpe.specs_of(domain)
    labels = list(specs)
    tids, losses, obs = history.gather(domain, trials, labels)
    groups = tpe.joint_groups(domain, specs, obs)
    assert groups == GC.GROUPS
    grouped = {k for _, g in groups for k in g}
    e = Engine(0, 'f64')
    try:
        splitter = P.Splitter(tids, losses, 0.25)
        for slot, g in groups:
            e.set_joint_group(slot, L.TPE_JOINT_STREAM - slot,
                              *P.joint_mixture([specs[k] for k in g], obs, splitter, 1.0,
                                               streams=[labels.index(k) for k in g]))
        seen = 0
        for j, new_id in enumerate(ids):
            for k in labels:
                if k not in grouped:
                    assert multi[j][k] == plain[j][k], k
                if k not in groups[0][1]:
                    assert single[j][k] == plain[j][k], k
            for slot, g in groups:
                win = e.joint_suggest(17, 24, round=new_id, slot=slot)[0]
                for k, v in zip(g, win):
                    # (a group's labels are active where the independent call's are)
                    assert multi[j][k] == ([float(v)] if plain[j][k] else []), (slot, k)
                    seen += bool(plain[j][k]) and slot > 0
                    if slot == 0:
                        assert single[j][k] == [float(v)]
        assert seen > 0, 'no conditional group active in any document: pick another seed'
    finally:
        e.close()
    dev = _vals(tpe.suggest(ids, domain, trials, 17, multivariate=True, group=True, batch=True,
                            posterior_builder='device'))
    assert dev == multi


def test_only_the_unconditional_group():
    """tests/test_joint_gpu.py's space: its one conditional label is alone, so
    group=True and group=False give the same documents."""
    from hyperopt_amd.base import Domain
    from tests.test_joint_gpu import _run as run_plain, e2e_loss, e2e_space
    trials = run_plain(False, seed=9, evals=30)
    domain = Domain(e2e_loss, e2e_space())
    kw = dict(batch=True, posterior_builder='host', multivariate=True)
    a = _vals(tpe.suggest([100, 101, 102], domain, trials, 17, group=True, **kw))
    b = _vals(tpe.suggest([100, 101, 102], domain, trials, 17, group=False, **kw))
    assert a == b
