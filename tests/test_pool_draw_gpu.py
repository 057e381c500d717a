"""The draw on a candidate pool on the device (tpe_pool_draw,
hyperopt_amd/csrc/tpe_pool.hip) and tpe.suggest(pool=..., pool_candidates=m),
against tests/pool_draw_reference.py.

Weights: lsum is the left-to-right sum of the engine's own below planes in the
working space -- bit for bit where the entry has no dense log column, else
within 2^-48 max(1, sum |term|) (16 ulp: the device's log and numpy's are each
under 1 ulp, at most 2 ulp apart per log term, carried through at most 10
additions).  Keys: lsum + the reference's Gumbel noise within
2^-48 max(1, |key|, |G|), and the same bits whatever `taken`, the other rounds
and `distinct` are.  Selection and pick: exactly the reference's on the
returned keys and scores.  With everything drawn the call is the ranking, bit
for bit."""
import ctypes
from functools import partial

import numpy as np
import pytest

from tests import pool_draw_reference as D
from tests import pool_reference as R
from tests.helpers import ALL_KINDS, make_history
from tests.test_pool_gpu import (GROUP_COLS, SEED, bits, draw_pool, engine_for, loss, picks, points, same_bits,
                                 set_group, space, study)  # noqa: F401  (study: a fixture)

pytestmark = pytest.mark.gpu

L = len(ALL_KINDS)
KINDS = [k for _, k, _ in ALL_KINDS]
LOG = [k in ('loguniform', 'lognormal') for k in KINDS]
SIZES = (1, 255, 256, 257, 700)
ROUNDS = ([3], [1, 3, 5], list(range(10, 18)))
TOL = 2.0 ** -48


def sizes_m(n):
    return sorted(set(m for m in (1, 24, n - 1, n, n + 5) if m >= 1))


def close(a, b, tol):
    """Equal, or both finite and within tol (elementwise)."""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid='ignore'):
        return bool(np.all((a == b) | (np.abs(a - b) <= tol)))


@pytest.fixture(scope='module')
def hist():
    return make_history(ALL_KINDS, 700, seed=700, active_frac=0.7)


@pytest.fixture(scope='module')
def eng(hist):
    e = engine_for(hist)
    yield e
    e.close()


@pytest.fixture(scope='module')
def base(eng):
    """Per n: the pool, the engine's planes and one draw call with every
    vector -- computed once, never changed."""
    out = {}
    for n in SIZES:
        vals = draw_pool(n)
        eng.pool_set(vals)
        _, _, score, lb, la = eng.pool_rank(1, want_scores=True, want_terms=True)
        idx, top, drawn, lsum, keys, score2 = eng.pool_draw(11, [1, 3, 5], 24, want_drawn=True, want_lsum=True,
                                                             want_keys=True, want_scores=True)
        out[n] = dict(vals=vals, score=score, lb=lb, la=la, idx=idx, top=top, drawn=drawn, lsum=lsum, keys=keys,
                      score2=score2)
    return out


@pytest.mark.parametrize('n', SIZES)
def test_lsum_is_the_working_space_sum_of_the_below_plane(base, n):
    b = base[n]
    assert same_bits(b['score2'], b['score'])
    ref, mag = D.lsum(b['vals'], b['lb'], KINDS)
    assert close(b['lsum'], ref, TOL * np.maximum(1.0, mag))


def test_lsum_without_a_log_column_is_bit_for_bit(eng, base):
    """Inactive (NaN) cells are skipped; an entry whose dense log columns are
    all inactive adds plain plane values: the reference's bits."""
    b = base[700]
    vals = b['vals'].copy()
    hole = np.random.RandomState(2).uniform(size=vals.shape) < 0.5
    hole[5] = True                   # an entry with no term: lsum 0.0
    vals[hole] = np.nan
    eng.pool_set(vals)
    lsum = eng.pool_draw(11, [1], 24, want_lsum=True)[2]
    ref, mag = D.lsum(vals, b['lb'], KINDS)      # (the planes of the full pool: active cells keep their bits)
    has_log = (~np.isnan(vals[:, LOG])).any(axis=1)
    assert has_log.sum() > 100 and (~has_log).sum() > 100
    assert same_bits(lsum[~has_log], ref[~has_log])
    assert close(lsum, ref, TOL * np.maximum(1.0, mag))
    assert bits(lsum[5:6])[0] == 0


@pytest.mark.parametrize('n', SIZES)
def test_keys_are_lsum_plus_the_reference_noise(eng, base, n):
    b = base[n]
    assert b['keys'].shape == (3, n)
    for row, r in zip(b['keys'], (1, 3, 5)):
        G = D.gumbel(11, r, n)
        assert close(row, b['lsum'] + G, TOL * np.maximum(1.0, np.maximum(np.abs(row), np.abs(G))))
    # the same bits with entries taken, in another set of rounds, with and without distinct
    eng.pool_set(b['vals'])
    for kw in (dict(taken=[0, n // 2, n - 1]), dict(distinct=False), dict()):
        keys = eng.pool_draw(11, [5, 2], 3, want_keys=True, **kw)[2]
        assert same_bits(keys[0], b['keys'][2]), kw
    # another seed, another round: other keys
    if n > 1:
        assert not same_bits(eng.pool_draw(12, [5], 3, want_keys=True)[2][0], b['keys'][2])
        assert not same_bits(b['keys'][0], b['keys'][1])


@pytest.mark.parametrize('n', SIZES)
def test_selection_and_pick_are_the_references(eng, base, n):
    b = base[n]
    eng.pool_set(b['vals'])
    variants = [dict(), dict(distinct=False), dict(taken=[0, n // 2, n // 2, n - 1, -1, n, 1 << 40])]
    for m in sizes_m(n):
        for rounds in ROUNDS:
            for kw in variants:
                idx, top, drawn, keys, score = eng.pool_draw(7, rounds, m, want_drawn=True, want_keys=True,
                                                             want_scores=True, **kw)
                assert same_bits(score, b['score'])
                best, want = D.draw(keys, score, m, taken=kw.get('taken', ()), distinct=kw.get('distinct', True))
                what = (n, m, rounds, kw)
                assert idx.dtype == np.int64 and idx.tolist() == best.tolist(), what
                assert len(drawn) == len(want) and all(g.tolist() == w.tolist() for g, w in zip(drawn, want)), what
                assert same_bits(top, score[best]), what
                assert all(i in d for i, d in zip(idx.tolist(), drawn)), what
    # the pool runs out: fewer picks than rounds, the last drawn sets shrink
    idx, _, drawn = eng.pool_draw(7, list(range(n + 3)), 2, want_drawn=True)[:3]
    assert sorted(idx.tolist()) == list(range(n))
    assert [len(d) for d in drawn] == [min(2, n - j) for j in range(n)]
    idx, _ = eng.pool_draw(7, [1, 2], 2, taken=list(range(n)))
    assert len(idx) == 0


ORACLE = dict(n=700, m=24, seed=1, round=3)    # chosen on the CPU (asserted below)


def test_drawn_set_and_pick_are_the_oracles(hist, base):
    n, m, seed, rnd = (ORACLE[k] for k in ('n', 'm', 'seed', 'round'))
    b = base[n]
    rlb, rla = R.oracle_planes(hist, b['vals'])
    keys = D.lsum(b['vals'], rlb, KINDS)[0] + D.gumbel(seed, rnd, n)
    score = R.scores(b['vals'], rlb, rla)
    order = D.select(keys, m + 1, range(n))
    assert keys[order[m - 1]] - keys[order[m]] > 1e-6
    best, drawn = D.draw(keys[None], score, m)
    top2 = np.sort(score[drawn[0]])[-2:]
    assert top2[1] - top2[0] > 1e-6
    e = engine_for(hist)
    e.pool_set(b['vals'])
    idx, _, got = e.pool_draw(seed, [rnd], m, want_drawn=True)
    e.close()
    assert sorted(got[0].tolist()) == sorted(drawn[0].tolist())
    assert idx.tolist() == best.tolist()


@pytest.mark.parametrize('n', (257, 700))
def test_everything_drawn_is_the_ranking(eng, base, n):
    b = base[n]
    eng.pool_set(b['vals'])
    widx, wtop, wscore = eng.pool_rank(4, want_scores=True)
    for m in (n, n + 5):
        for seed in (1, 2):
            idx, top, score = eng.pool_draw(seed, [0, 1, 2, 3], m, distinct=True, want_scores=True)
            assert idx.tolist() == widx.tolist() and same_bits(top, wtop) and same_bits(score, wscore)
    tk = [int(widx[0]), 5]
    widx, wtop = eng.pool_rank(4, taken=tk)
    idx, top = eng.pool_draw(3, [9, 9, 9, 9], n, taken=tk)
    assert idx.tolist() == widx.tolist() and same_bits(top, wtop)


def test_distinct_rounds_are_sequential_calls(eng, base):
    b = base[700]
    eng.pool_set(b['vals'])
    rounds = [1, 3, 5, 8]
    idx, top, drawn = eng.pool_draw(11, rounds, 24, taken=[2], want_drawn=True)
    assert len(set(idx.tolist())) == 4 and 2 not in idx.tolist()
    taken = [2]
    for j, r in enumerate(rounds):
        i1, t1, d1 = eng.pool_draw(11, [r], 24, taken=taken, want_drawn=True)
        assert i1.tolist() == [idx[j]] and same_bits(t1, top[j:j + 1]) and d1[0].tolist() == drawn[j].tolist()
        taken.append(int(i1[0]))
    # with replacement a round alone is the round inside a batch
    idx, top, drawn = eng.pool_draw(11, rounds, 24, distinct=False, want_drawn=True)
    for j, r in enumerate(rounds):
        i1, t1, d1 = eng.pool_draw(11, [r], 24, distinct=False, want_drawn=True)
        assert i1.tolist() == [idx[j]] and same_bits(t1, top[j:j + 1]) and d1[0].tolist() == drawn[j].tolist()


def test_joint_group_stands_in_for_its_columns(hist, base):
    vals = base[700]['vals'].copy()
    hole = np.random.RandomState(4).uniform(size=vals.shape) < 0.15
    hole[5] = True                   # an entry with no term: lsum 0.0
    vals[hole] = np.nan
    e = engine_for(hist)
    set_group(e, 3)
    e.pool_set(vals)
    groups = [(3, GROUP_COLS)]
    _, _, score, lb, la = e.pool_rank(1, groups=groups, want_scores=True, want_terms=True)
    idx, top, drawn, lsum, keys, score2 = e.pool_draw(5, [1, 2], 24, groups=groups, want_drawn=True,
                                                       want_lsum=True, want_keys=True, want_scores=True)
    plain = e.pool_draw(5, [1], 24, want_lsum=True)[2]
    e.close()
    assert same_bits(score2, score)
    ref, mag = D.lsum(vals, lb, KINDS, groups=[(GROUP_COLS, L)])
    act = ~np.isnan(vals[:, GROUP_COLS]).any(axis=1)
    rest = [c for c in range(L) if LOG[c] and c not in GROUP_COLS]
    has_log = (~np.isnan(vals[:, rest])).any(axis=1) | act      # (the group holds the log column 'lu')
    assert 0 < act.sum() < 700 and (~has_log).sum() > 1
    assert same_bits(lsum[~has_log], ref[~has_log])
    assert close(lsum, ref, TOL * np.maximum(1.0, mag))
    assert bits(lsum[5:6])[0] == 0
    assert not same_bits(lsum, plain)        # the group's term is in use
    best, want = D.draw(keys, score, 24)
    assert idx.tolist() == best.tolist() and all(g.tolist() == w.tolist() for g, w in zip(drawn, want))


def raw_draw(e, m=3, rounds=(1, 2), null=None, n_rounds=None, groups=()):
    """tpe_pool_draw through the C ABI with outputs filled beforehand: (rc, outputs)."""
    n, _ = e.pool_size()
    n = max(n, 1)
    R_ = len(rounds)
    slots = np.asarray([s for s, _ in groups], dtype=np.int32)
    off = np.cumsum([0] + [len(c) for _, c in groups]).astype(np.int64)
    gc = np.asarray([c for _, cs in groups for c in cs], dtype=np.int32)
    rd = np.asarray(rounds, dtype=np.uint32)
    out = dict(index=np.full(max(R_, 1), -7, dtype=np.int64), top=np.full(max(R_, 1), -7.0),
               drawn=np.full((max(R_, 1), n), -7, dtype=np.int64), n_drawn=np.full(max(R_, 1), -7, dtype=np.int32),
               lsum=np.full(n, -7.0), keys=np.full((max(R_, 1), n), -7.0), score=np.full(n, -7.0))
    n_best = ctypes.c_int32(-7)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    g = lambda k: None if null == k else p(out[k])
    rc = e.lib.tpe_pool_draw(e.h, len(groups), p(slots) if len(groups) else None, p(off) if len(groups) else None,
                             p(gc) if len(groups) else None, None, 0, 9, None if null == 'rounds' else p(rd),
                             R_ if n_rounds is None else n_rounds, m, 1, g('index'), g('top'),
                             None if null == 'n_best' else ctypes.byref(n_best), g('drawn'), g('n_drawn'),
                             g('lsum'), g('keys'), g('score'))
    out['n_best'] = n_best.value
    return rc, out


def untouched(out):
    return out['n_best'] == -7 and all((out[k] == -7).all() for k in out if k != 'n_best')


def test_errors_leave_the_outputs_untouched(hist, base):
    from hyperopt_amd import _lib
    from hyperopt_amd.engine import Engine, EngineError
    vals = base[257]['vals']
    e = Engine(0, 'f64')
    with pytest.raises(EngineError, match='no pool'):
        e.pool_draw(1, [1], 3)
    e.pool_set(vals)
    with pytest.raises(EngineError, match='no posterior'):
        e.pool_draw(1, [1], 3)
    e.build_posterior(*hist.device_inputs(), gamma=0.25, prior_weight=1.0)
    set_group(e, 3)
    bad = [dict(m=0), dict(m=-4), dict(n_rounds=0), dict(n_rounds=-1), dict(rounds=[1] * 4097),
           dict(null='rounds'), dict(null='index'), dict(null='top'), dict(null='n_best'), dict(null='drawn'),
           dict(null='n_drawn'), dict(groups=[(5, GROUP_COLS)]), dict(groups=[(3, [0, 2])]),
           dict(groups=[(3, [0, 2, L])])]
    for kw in bad:
        rc, out = raw_draw(e, **kw)
        assert rc == _lib.TPE_ERR_ARG and untouched(out), kw
    for kw in (dict(), dict(rounds=[1] * 4096, m=1), dict(groups=[(3, GROUP_COLS)]), dict(null='lsum')):
        rc, out = raw_draw(e, **kw)              # (the same calls without a fault)
        assert rc == _lib.TPE_OK and out['n_best'] == min(len(kw.get('rounds', (1, 2))), 257), kw   # (distinct)
        assert not (out['score'] == -7).any() and not (out['keys'] == -7).any()
    # a value the ranking refuses: the same error, nothing written
    names = [n for n, _, _ in ALL_KINDS]
    for label, v in (('ri', 7.0), ('pc', 1.5), ('qlu', -3.0)):
        wrong = vals.copy()
        wrong[256, names.index(label)] = v
        e.pool_set(wrong)
        rc, out = raw_draw(e)
        assert rc == _lib.TPE_ERR_VALUE and untouched(out), (label, v)
        with pytest.raises(ValueError):
            e.pool_draw(1, [1], 3)
    e.pool_set(vals)
    assert e.pool_draw(11, [1, 3, 5], 24)[0].tolist() == base[257]['idx'].tolist()
    e.close()
    with pytest.raises(EngineError, match='F64'):
        f = Engine(0, 'f32')
        try:
            f.pool_draw(1, [1], 3)
        finally:
            f.close()


def test_multi_device_context_is_refused(hist, base):
    from hyperopt_amd.engine import Engine, EngineError
    two = Engine([0, 0], 'f64')
    two.build_posterior(*hist.device_inputs(), gamma=0.25, prior_weight=1.0)
    with pytest.raises(EngineError, match='multi-device'):
        two.pool_draw(1, [1], 3)
    two.close()


# -- tpe.suggest(pool=..., pool_candidates=m) --------------------------------

def test_suggest_with_everything_drawn_is_the_ranking(study):
    from hyperopt_amd import tpe
    s = study
    kw = dict(pool=s['pool'], posterior_builder='host')
    ids = [100, 101, 102, 103, 104]
    for m in (len(s['pool']), len(s['pool']) + 7):
        assert tpe.suggest([100], s['domain'], s['trials'], 9, pool_candidates=m, **kw) == \
            tpe.suggest([100], s['domain'], s['trials'], 9, **kw)
        assert tpe.suggest(ids, s['domain'], s['trials'], 3, batch=True, pool_candidates=m, **kw) == \
            tpe.suggest(ids, s['domain'], s['trials'], 9, batch=True, **kw)
    pend = tpe.suggest(ids[:3], s['domain'], s['trials'], 9, batch='pending', pool_candidates=len(s['pool']), **kw)
    assert pend == tpe.suggest(ids[:3], s['domain'], s['trials'], 9, batch='pending', **kw)


def test_suggest_is_the_engines_draw(study):
    from hyperopt_amd import engine as E, tpe
    s = study
    kw = dict(pool=s['pool'], pool_candidates=24, posterior_builder='host')
    sets = {}
    for seed in (9, 10):
        doc = tpe.suggest([100], s['domain'], s['trials'], seed, **kw)
        eng = E.get_engine(0, 'f64')      # the call's engine: its posterior and pool are resident
        idx, _, drawn = eng.pool_draw(seed, [100], 24, want_drawn=True)
        assert picks(doc) == idx.tolist() and len(drawn[0]) == 24 and picks(doc)[0] in drawn[0].tolist()
        assert doc[0]['tid'] == 100
        vals = {k: v[0] for k, v in doc[0]['misc']['vals'].items() if v}
        assert vals == s['pool'].points[picks(doc)[0]]
        assert doc == tpe.suggest([100], s['domain'], s['trials'], seed, **kw)      # seeded
        sets[seed] = sorted(drawn[0].tolist())
    assert sets[9] != sets[10]
    # every id its own draw: a batch is distinct, and each id's pick comes from its own round
    four = tpe.suggest([100, 101, 102, 103], s['domain'], s['trials'], 9, batch=True, **kw)
    assert len(set(picks(four))) == 4 and [d['tid'] for d in four] == [100, 101, 102, 103]
    eng = E.get_engine(0, 'f64')
    idx, _, drawn = eng.pool_draw(9, [100, 101, 102, 103], 24, want_drawn=True)
    assert picks(four) == idx.tolist() and len(set(tuple(d.tolist()) for d in drawn)) == 4
    # with replacement an id's pick is its one-id call's, so picks may repeat
    rep = tpe.suggest([100, 101, 102, 103], s['domain'], s['trials'], 9, batch=True, pool_replace=True, **kw)
    for j, new_id in enumerate([100, 101, 102, 103]):
        one = tpe.suggest([new_id], s['domain'], s['trials'], 9, pool_replace=True, **kw)
        assert picks(one) == picks(rep)[j:j + 1]
    pend = tpe.suggest([100, 101, 102], s['domain'], s['trials'], 9, batch='pending', **kw)
    assert len(set(picks(pend))) == 3 and picks(pend)[0] == picks(four)[0]


def test_fmin_with_a_draw_visits_every_entry_once_and_stops(study):
    from hyperopt_amd import Trials, fmin, tpe
    pool = tpe.Pool(study['domain'], points(40, SEED + 2))
    trials = Trials()
    fmin(loss, space(), algo=partial(tpe.suggest, pool=pool, pool_candidates=5, n_startup_jobs=5), max_evals=60,
         trials=trials, rstate=np.random.RandomState(1))
    assert sorted(picks(trials.trials)) == list(range(40))


def test_pool_candidates_none_documents_are_unchanged(study):
    from hyperopt_amd import tpe
    s = study
    kw = dict(pool=s['pool'], posterior_builder='host')
    want = R.rank(s['ref'], 2)
    before = tpe.suggest([100, 101], s['domain'], s['trials'], 9, batch=True, **kw)
    tpe.suggest([100], s['domain'], s['trials'], 9, pool_candidates=24, **kw)
    after = tpe.suggest([100, 101], s['domain'], s['trials'], 9, batch=True, pool_candidates=None, **kw)
    assert before == after and picks(after) == want.tolist()
