"""Candidate pools on the device (tpe_pool_set / tpe_pool_rank,
hyperopt_amd/csrc/tpe_pool.hip) and tpe.suggest(pool=...).

Terms: each per-label plane against the CPU oracle at the project's lpdf bar
(helpers.assert_lpdf_close).  Structure, bit for bit: the score is the
left-to-right sum of lb - la over the planes the engine returns, and it does
not depend on n, on the entry's position or on the other entries.  Rank:
exactly the reference ranking (tests/pool_reference.py) of the returned
scores.  At n = 700 the oracle's own four best scores are 4.784, 4.765, 4.491
and 3.817 (gaps >= 0.018, seven orders above the lpdf bar), so the first four
indices must be the oracle's."""
import ctypes
from functools import partial

import numpy as np
import pytest

from tests import pool_reference as R
from tests.helpers import ALL_KINDS, assert_lpdf_close, make_history

pytestmark = pytest.mark.gpu

L = len(ALL_KINDS)
QUANT = [k in ('quniform', 'qloguniform', 'qnormal', 'qlognormal') for _, k, _ in ALL_KINDS]
SIZES = (1, 255, 256, 257, 700)


def draw_pool(n, seed=5):
    from hyperopt_amd.workloads import prior_draw
    rng = np.random.RandomState(seed)
    return np.stack([prior_draw(kind, args, rng, n) for _, kind, args in ALL_KINDS], axis=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_values(a, b):
    """Equal as numbers, NaN equal to NaN (the payload of a NaN is not part of the contract)."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope='module')
def hist():
    return make_history(ALL_KINDS, 700, seed=700, active_frac=0.7)


def engine_for(h):
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    e.build_posterior(*h.device_inputs(), gamma=0.25, prior_weight=1.0)
    return e


@pytest.fixture(scope='module')
def eng(hist):
    e = engine_for(hist)
    yield e
    e.close()


@pytest.fixture(scope='module')
def ranked(eng, hist):
    """Per n: the pool, the engine's full ranking with scores and planes, the
    oracle's planes -- computed once, never changed."""
    out = {}
    for n in SIZES:
        vals = draw_pool(n)
        eng.pool_set(vals)
        assert eng.pool_size() == (n, L)
        idx, top, score, lb, la = eng.pool_rank(n, want_scores=True, want_terms=True)
        rlb, rla = R.oracle_planes(hist, vals)
        out[n] = dict(vals=vals, idx=idx, top=top, score=score, lb=lb, la=la, rlb=rlb, rla=rla)
    return out


@pytest.mark.parametrize('n', SIZES)
def test_terms_against_the_oracle(ranked, n):
    r = ranked[n]
    if n == 700:
        assert np.isfinite(r['rlb']).all() and np.isfinite(r['rla']).all()
    assert r['lb'].shape == (n, L) and r['la'].shape == (n, L)
    for c in range(L):
        assert_lpdf_close(r['lb'][:, c], r['rlb'][:, c], quantized=QUANT[c])
        assert_lpdf_close(r['la'][:, c], r['rla'][:, c], quantized=QUANT[c])


@pytest.mark.parametrize('n', SIZES)
def test_score_is_the_left_to_right_sum_of_the_planes(ranked, n):
    r = ranked[n]
    assert same_bits(r['score'], R.scores(r['vals'], r['lb'], r['la']))


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('k', ('1', '4', 'n'))
def test_rank_is_the_reference_ranking_of_the_scores(eng, ranked, n, k):
    r = ranked[n]
    k = n if k == 'n' else int(k)
    want = R.rank(r['score'], k)
    if k == n:
        idx, top = r['idx'], r['top']
    else:
        eng.pool_set(r['vals'])
        idx, top = eng.pool_rank(k)
    assert idx.dtype == np.int64 and idx.tolist() == want.tolist()
    assert same_bits(top, r['score'][want])


def test_first_four_are_the_oracles(ranked):
    r = ranked[700]
    ref = R.scores(r['vals'], r['rlb'], r['rla'])
    want = R.rank(ref, 5)
    gaps = -np.diff(ref[want])
    assert np.allclose(ref[want[:4]], [4.784, 4.765, 4.491, 3.817], atol=5e-4) and gaps[:4].min() >= 0.011
    assert r['idx'][:4].tolist() == want[:4].tolist()


@pytest.mark.parametrize('n', (257, 700))
def test_planes_are_engine_score_bit_for_bit(eng, ranked, n):
    """Both call the same device functions: a plane column is
    Engine.score(label, column) -- at 257 entries its packed map with three
    slots per thread, at 700 the one with four."""
    r = ranked[n]
    for c in range(L):
        lb, la, _ = eng.score(c, r['vals'][:, c])
        assert same_bits(r['lb'][:, c], lb) and same_bits(r['la'][:, c], la), ALL_KINDS[c][0]


def test_position_independence(eng, ranked):
    r = ranked[700]
    perm = np.random.RandomState(1).permutation(700)
    eng.pool_set(r['vals'][perm])
    _, _, score = eng.pool_rank(1, want_scores=True)
    assert same_bits(score, r['score'][perm])
    for i in (0, 313, 699):          # a one-entry pool: that entry's bits
        eng.pool_set(r['vals'][i:i + 1])
        idx, top, score = eng.pool_rank(3, want_scores=True)
        assert idx.tolist() == [0] and same_bits(score, r['score'][i:i + 1]) and same_bits(top, score)
    eng.pool_set(r['vals'][:257])    # another n, a prefix
    _, _, score = eng.pool_rank(1, want_scores=True)
    assert same_bits(score, r['score'][:257])


def test_inactive_cells_are_skipped(eng, ranked):
    r = ranked[700]
    vals = r['vals'].copy()
    hole = np.random.RandomState(2).uniform(size=vals.shape) < 0.3
    hole[5] = True                   # an entry with no term scores 0.0
    vals[hole] = np.nan
    eng.pool_set(vals)
    idx, top, score, lb, la = eng.pool_rank(700, want_scores=True, want_terms=True)
    assert np.isnan(lb[hole]).all() and np.isnan(la[hole]).all()
    assert same_bits(lb[~hole], r['lb'][~hole]) and same_bits(la[~hole], r['la'][~hole])
    assert same_bits(score, R.scores(vals, r['lb'], r['la']))
    assert bits(score[5:6])[0] == 0
    assert idx.tolist() == R.rank(score, 700).tolist()


def test_quantized_columns_listed_and_direct():
    """tpe_pool_set lists the distinct values of a column that has at most 4096
    of them, and a quantized label's lpdfs are then computed once per listed
    value; a column with more is scored entry by entry.  Both against the
    oracle, and the same bits for the same value on either path."""
    labels = [('qf', 'qnormal', dict(mu=0.0, sigma=3.0, q=0.001)),
              ('qlf', 'qlognormal', dict(mu=1.0, sigma=1.0, q=0.001)),
              ('qu', 'quniform', dict(low=0.0, high=20.0, q=1.0))]
    h = make_history(labels, 120, seed=12, active_frac=0.8)
    from hyperopt_amd.workloads import prior_draw
    rng = np.random.RandomState(6)
    n = 6000
    vals = np.stack([prior_draw(kind, args, rng, n) for _, kind, args in labels], axis=1)
    assert len(np.unique(vals[:, 0])) > 4096 and len(np.unique(vals[:, 1])) > 4096
    assert len(np.unique(vals[:700, 0])) <= 700 and len(np.unique(vals[:, 2])) <= 21
    vals[::7, 1] = np.nan
    e = engine_for(h)
    e.pool_set(vals)
    idx, top, score, lb, la = e.pool_rank(n, want_scores=True, want_terms=True)
    rlb, rla = R.oracle_planes(h, vals)
    for c in range(3):
        assert_lpdf_close(lb[:, c], rlb[:, c], quantized=True)
        assert_lpdf_close(la[:, c], rla[:, c], quantized=True)
    assert same_bits(score, R.scores(vals, lb, la)) and idx.tolist() == R.rank(score, n).tolist()
    e.pool_set(vals[:700])      # every column listed now
    _, _, score7, lb7, la7 = e.pool_rank(1, want_scores=True, want_terms=True)
    e.close()
    keep = ~np.isnan(vals[:700])
    assert same_bits(lb7[keep], lb[:700][keep]) and same_bits(la7[keep], la[:700][keep])
    assert same_bits(score7, score[:700])


def test_ties_nan_and_taken(eng, ranked, hist):
    r = ranked[257]
    best = int(r['idx'][0])
    # copies of the best entry below and above it: the lowest index first
    vals = np.concatenate([r['vals'][best:best + 1], r['vals'], r['vals'][best:best + 1]])
    eng.pool_set(vals)
    idx, top, score = eng.pool_rank(4, want_scores=True)
    assert idx[:3].tolist() == [0, best + 1, 258] and idx[3] == r['idx'][1] + 1
    assert len(set(bits(top[:3]).tolist())) == 1
    assert idx.tolist() == R.rank(score, 4).tolist()
    # taken entries are left out; duplicates and indices outside the pool are ignored
    taken = [0, best + 1, best + 1, 259, -1, 1 << 40, int(idx[3])]
    idx2, top2, score2 = eng.pool_rank(3, taken=taken, want_scores=True)
    assert same_bits(score2, score)
    assert idx2.tolist() == R.rank(score, 3, taken=taken).tolist() and idx2[0] == 258
    # k larger than what is free
    free = [3, 100, 258]
    idx3, top3 = eng.pool_rank(50, taken=[i for i in range(259) if i not in free])
    assert idx3.tolist() == R.rank(score, 50, taken=[i for i in range(259) if i not in free]).tolist()
    assert len(idx3) == 3 and sorted(idx3.tolist()) == free
    idx4, _ = eng.pool_rank(1, taken=list(range(259)))
    assert len(idx4) == 0


def test_resident_across_rebuilds(ranked):
    r = ranked[700]
    second = make_history(ALL_KINDS, 300, seed=301, active_frac=0.8)
    first = make_history(ALL_KINDS, 700, seed=700, active_frac=0.7)
    e = engine_for(first)
    e.pool_set(r['vals'])
    a = e.pool_rank(4, want_scores=True)
    assert same_bits(a[2], r['score'])
    e.build_posterior(*second.device_inputs(), gamma=0.25, prior_weight=1.0)   # no pool_set
    assert e.pool_size() == (700, L)
    got = e.pool_rank(4, want_scores=True)
    e.close()
    fresh = engine_for(second)
    fresh.pool_set(r['vals'])
    want = fresh.pool_rank(4, want_scores=True)
    fresh.close()
    assert not same_bits(got[2], r['score'])
    assert got[0].tolist() == want[0].tolist() and same_bits(got[1], want[1]) and same_bits(got[2], want[2])


GROUP_COLS = [0, 2, 1]   # 'u' dense, 'lu' log, 'qu' quantized


def set_group(e, slot, seed=3):
    from hyperopt_amd import _lib, posterior as P
    labels = [ALL_KINDS[c] for c in GROUP_COLS]
    h = make_history(labels, 60, seed=seed)
    mix = P.joint_mixture(labels, h.obs, P.Splitter(h.tids, h.losses, 0.25), 1.0, streams=GROUP_COLS,
                          quantized=True)
    e.set_joint_group(slot, _lib.TPE_JOINT_STREAM - slot, *mix, prior_weight=1.0)


def test_joint_group_stands_in_for_its_columns(hist, ranked):
    r = ranked[700]
    vals = r['vals'].copy()
    hole = np.random.RandomState(4).uniform(size=vals.shape) < 0.15
    vals[hole] = np.nan
    e = engine_for(hist)
    set_group(e, 3)
    e.pool_set(vals)
    idx, top, score, lb, la = e.pool_rank(700, groups=[(3, GROUP_COLS)], want_scores=True, want_terms=True)
    assert lb.shape == (700, L + 1)
    act = ~np.isnan(vals[:, GROUP_COLS]).any(axis=1)
    assert 0 < act.sum() < 700
    ll, lg = e.joint_score(vals[act][:, GROUP_COLS], slot=3)
    e.close()
    assert same_bits(lb[act, L], ll) and same_bits(la[act, L], lg)
    assert np.isnan(lb[~act, L]).all() and np.isnan(la[~act, L]).all()
    assert np.isnan(lb[:, GROUP_COLS]).all() and np.isnan(la[:, GROUP_COLS]).all()
    rest = [c for c in range(L) if c not in GROUP_COLS]
    keep = ~np.isnan(vals[:, rest])
    assert same_bits(lb[:, rest][keep], r['lb'][:, rest][keep])
    assert same_values(score, R.scores(vals, lb, la, groups=[(GROUP_COLS, L)]))
    finite = np.isfinite(score)
    assert same_bits(score[finite], R.scores(vals, lb, la, groups=[(GROUP_COLS, L)])[finite])
    assert idx.tolist() == R.rank(score, 700).tolist()


def raw_rank(e, k, groups=(), null=None, n_out=8):
    """tpe_pool_rank through the C ABI with outputs filled beforehand: (rc, outputs)."""
    n, cols = e.pool_size()
    slots = np.asarray([s for s, _ in groups], dtype=np.int32)
    off = np.cumsum([0] + [len(c) for _, c in groups]).astype(np.int64)
    gc = np.asarray([c for _, cs in groups for c in cs], dtype=np.int32)
    out = dict(index=np.full(n_out, -7, dtype=np.int64), top=np.full(n_out, -7.0),
               score=np.full(max(n, 1), -7.0), lb=np.full((max(n, 1), cols + len(groups)), -7.0),
               la=np.full((max(n, 1), cols + len(groups)), -7.0))
    n_top = ctypes.c_int32(-7)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = e.lib.tpe_pool_rank(e.h, len(groups), p(slots) if len(groups) else None,
                             p(off) if len(groups) else None, p(gc) if len(groups) else None, None, 0, k,
                             None if null == 'index' else p(out['index']),
                             None if null == 'top' else p(out['top']),
                             None if null == 'n_top' else ctypes.byref(n_top), p(out['score']), p(out['lb']),
                             None if null == 'la' else p(out['la']))
    out['n_top'] = n_top.value
    return rc, out


def untouched(out):
    return out['n_top'] == -7 and all((out[k] == -7).all() for k in ('index', 'top', 'score', 'lb', 'la'))


def test_argument_errors(hist, ranked):
    from hyperopt_amd import _lib
    from hyperopt_amd.engine import Engine, EngineError
    vals = ranked[257]['vals']
    e = Engine(0, 'f64')
    assert e.pool_size() == (0, 0)
    with pytest.raises(EngineError, match='no pool'):
        e.pool_rank(1)
    with pytest.raises(EngineError):
        e.pool_set(np.zeros((0, L)))
    e.pool_set(vals)
    with pytest.raises(EngineError, match='no posterior'):
        e.pool_rank(1)
    e.build_posterior(*hist.device_inputs(), gamma=0.25, prior_weight=1.0)
    e.pool_set(vals[:, :3])
    with pytest.raises(EngineError, match='columns'):
        e.pool_rank(1)
    e.pool_clear()
    assert e.pool_size() == (0, 0)
    with pytest.raises(EngineError, match='no pool'):
        e.pool_rank(1)
    e.pool_set(vals)
    set_group(e, 3)
    set_group(e, 4, seed=8)
    bad = [(1, [(5, GROUP_COLS)]),                           # a slot that is not set
           (1, [(-1, GROUP_COLS)]), (1, [(64, GROUP_COLS)]),
           (1, [(3, GROUP_COLS), (3, [4, 6, 5])]),            # a slot listed twice
           (1, [(3, [0, 2, L])]), (1, [(3, [0, 2, -1])]),     # a column out of range
           (1, [(3, GROUP_COLS), (4, [4, 2, 5])]),            # a column in two groups
           (1, [(3, [0, 0, 1])]),
           (1, [(3, [0, 2])]), (1, [(3, [0, 2, 1, 4])]),      # not the slot's D columns
           (0, []), (-2, [])]                                 # top_k < 1
    for k, groups in bad:
        rc, out = raw_rank(e, k, groups)
        assert rc == _lib.TPE_ERR_ARG and untouched(out), (k, groups)
    for null in ('index', 'top', 'n_top', 'la'):
        rc, out = raw_rank(e, 1, null=null)
        assert rc == _lib.TPE_ERR_ARG and untouched(out), null
    rc, out = raw_rank(e, 2, [(3, GROUP_COLS), (4, [4, 6, 5])])   # (the same call without a fault)
    assert rc == _lib.TPE_OK and out['n_top'] == 2 and not (out['score'] == -7).any()
    e.close()


def test_value_errors(eng, ranked):
    from hyperopt_amd import _lib
    vals = ranked[257]['vals']
    names = [n for n, _, _ in ALL_KINDS]
    for v in (np.inf, -np.inf):
        bad = vals.copy()
        bad[200, 4] = v
        with pytest.raises(ValueError, match='infinite'):
            eng.pool_set(bad)
    eng.pool_set(vals)
    good = eng.pool_rank(2, want_scores=True)
    for label, v in (('ri', 7.0), ('ri', -1.0), ('pc', 1.5), ('qlu', -3.0)):
        bad = vals.copy()
        bad[256, names.index(label)] = v
        eng.pool_set(bad)
        rc, out = raw_rank(eng, 2)
        assert rc == _lib.TPE_ERR_VALUE and untouched(out), (label, v)
        with pytest.raises(ValueError):
            eng.pool_rank(2)
    # the context is as good as before
    eng.pool_set(vals)
    again = eng.pool_rank(2, want_scores=True)
    assert again[0].tolist() == good[0].tolist() and same_bits(again[2], good[2])


def test_multi_device_context_is_refused(hist, ranked):
    from hyperopt_amd.engine import Engine, EngineError
    two = Engine([0, 0], 'f64')
    two.build_posterior(*hist.device_inputs(), gamma=0.25, prior_weight=1.0)
    with pytest.raises(EngineError, match='multi-device'):
        two.pool_set(ranked[257]['vals'])
    with pytest.raises(EngineError, match='multi-device'):
        two.pool_rank(1)
    two.close()


# -- tpe.suggest(pool=...) ---------------------------------------------------

def space():
    from hyperopt_amd import hp
    return {'lr': hp.loguniform('lr', -5, 0), 'wd': hp.uniform('wd', 0, 1),
            'opt': hp.choice('opt', [{'momentum': hp.uniform('momentum', 0, 1), 'damp': hp.uniform('damp', 0, 1)},
                                     {'beta': hp.uniform('beta', 0.5, 1), 'eps': hp.lognormal('eps', -8, 1)}])}


def loss(cfg):
    o = cfg['opt']
    extra = (o['momentum'] - 0.9) ** 2 + o['damp'] if 'momentum' in o else (o['beta'] - 0.7) ** 2 + 0.3
    return (np.log(cfg['lr']) + 2.0) ** 2 + cfg['wd'] + extra


def points(n, seed):
    from hyperopt_amd import labels as LB
    from hyperopt_amd.space import as_apply
    expr = as_apply(space())
    specs = LB.compile_space(expr)
    rng = np.random.RandomState(seed)
    return [LB.sample_config(expr, specs, rng) for _ in range(n)]


SEED = 0     # chosen on the CPU: the reference's six best scores differ by more than 1e-6 (asserted)


@pytest.fixture(scope='module')
def study():
    from hyperopt_amd import Trials, fmin, rand, tpe
    from hyperopt_amd.base import Domain
    trials = Trials()
    fmin(loss, space(), algo=rand.suggest, max_evals=40, trials=trials, rstate=np.random.RandomState(SEED))
    domain = Domain(loss, space())
    pool = tpe.Pool(domain, points(300, SEED + 1))
    specs, n_docs, posts = tpe.build_posteriors(domain, trials)
    assert n_docs == 40 and list(specs) == pool.labels
    lb, la = R.posterior_planes(posts, pool.values)
    ref = R.scores(pool.values, lb, la)
    return dict(trials=trials, domain=domain, pool=pool, ref=ref)


def picks(docs):
    return [d['misc']['pool_index'] for d in docs]


def test_suggest_is_the_reference_argmax(study):
    from hyperopt_amd import tpe
    s = study
    want = R.rank(s['ref'], 6)
    assert (-np.diff(s['ref'][want])).min() > 1e-6
    docs = {}
    for builder in ('host', 'device'):
        d = tpe.suggest([100], s['domain'], s['trials'], 9, pool=s['pool'], posterior_builder=builder)
        assert picks(d) == [int(want[0])] and d[0]['tid'] == 100
        vals = {k: v[0] for k, v in d[0]['misc']['vals'].items() if v}
        assert vals == s['pool'].points[want[0]]
        five = tpe.suggest([100, 101, 102, 103, 104], s['domain'], s['trials'], 9, pool=s['pool'], batch=True,
                           posterior_builder=builder, n_EI_candidates=3)
        assert picks(five) == want[:5].tolist() and [x['tid'] for x in five] == [100, 101, 102, 103, 104]
        pend = tpe.suggest([100, 101, 102], s['domain'], s['trials'], 9, pool=s['pool'], batch='pending',
                           posterior_builder=builder)
        assert len(set(picks(pend))) == 3 and picks(pend)[0] == want[0]
        docs[builder] = (d, five, pend)
    assert docs['host'] == docs['device']
    # another seed: the same documents past the startup phase
    assert tpe.suggest([100], s['domain'], s['trials'], 10, pool=s['pool']) == docs['host'][0]


def test_suggest_skips_taken_entries_and_replaces(study):
    from hyperopt_amd import tpe
    from hyperopt_amd.base import Trials
    s = study
    want = R.rank(s['ref'], 3)
    held = Trials()
    held.insert_trial_docs([dict(d) for d in s['trials'].trials])
    first = tpe.suggest([100], s['domain'], s['trials'], 9, pool=s['pool'])
    held.insert_trial_docs(first)       # still pending
    held.refresh()
    assert tpe.pool_taken(s['pool'], held) == [int(want[0])]
    # (a pending document changes the posterior: the next pick is the engine's, not the old ranking's)
    nxt = tpe.suggest([101], s['domain'], held, 9, pool=s['pool'])
    assert picks(nxt)[0] != want[0]
    again = tpe.suggest([101], s['domain'], held, 9, pool=s['pool'], pool_replace=True)
    full = tpe.suggest([101, 102], s['domain'], held, 9, pool=s['pool'], pool_replace=True, batch=True)
    assert picks(again) == picks(full)[:1] and len(set(picks(full))) == 2


def test_fmin_over_a_pool_repeats_no_index(study):
    from hyperopt_amd import Trials, fmin, tpe
    trials = Trials()
    fmin(loss, space(), algo=partial(tpe.suggest, pool=study['pool'], n_startup_jobs=5), max_evals=30,
         trials=trials, rstate=np.random.RandomState(1))
    got = picks(trials.trials)
    assert len(got) == 30 and len(set(got)) == 30


@pytest.mark.parametrize('extra', [dict(), dict(group=True, joint_categorical=True)])
def test_multivariate_pick_is_the_argmax_of_the_engines_planes(study, extra):
    from hyperopt_amd import engine as E, history, posterior as P, tpe
    s = study
    domain, pool = s['domain'], s['pool']
    doc = tpe.suggest([100], domain, s['trials'], 9, pool=pool, multivariate=True, posterior_builder='host',
                      **extra)
    specs = tpe.specs_of(domain)
    labels = list(specs)
    obs = history.gather(domain, s['trials'], labels)[2]
    if extra:
        groups = tpe.joint_groups(domain, specs, obs, P.JOINT_KINDS + P.JOINT_CAT_KINDS)
        assert [g for _, g in groups] == [['lr', 'opt', 'wd'], ['beta', 'eps'], ['damp', 'momentum']]
    else:
        groups = [(0, tpe.joint_group(domain, specs, obs))]
        assert groups[0][1] == ['lr', 'wd']
    cols = [(slot, [labels.index(k) for k in g]) for slot, g in groups]
    eng = E.get_engine(0, 'f64')      # the call's engine: its posterior, groups and pool are resident
    idx, top, score, lb, la = eng.pool_rank(1, groups=cols, want_scores=True, want_terms=True)
    n_l = len(labels)
    covered = sorted(c for _, cs in cols for c in cs)
    assert np.isnan(lb[:, covered]).all() and np.isnan(la[:, covered]).all()
    for g, (_, cs) in enumerate(cols):
        act = ~np.isnan(pool.values[:, cs]).any(axis=1)
        assert act.any() and np.isfinite(lb[act, n_l + g]).all() and np.isnan(lb[~act, n_l + g]).all()
    want = R.scores(pool.values, lb, la, groups=[(cs, n_l + g) for g, (_, cs) in enumerate(cols)])
    assert same_bits(score, want)
    assert picks(doc) == [int(R.rank(want, 1)[0])] == idx.tolist()
    # the independent ranking is another one: the groups' terms are in use
    assert not same_bits(score, eng.pool_rank(1, want_scores=True)[2])


def test_pool_none_documents_are_unchanged(study):
    from hyperopt_amd import tpe
    s = study
    kw = dict(posterior_builder='host')
    before = tpe.suggest([100, 101], s['domain'], s['trials'], 9, batch=True, **kw)
    tpe.suggest([100], s['domain'], s['trials'], 9, pool=s['pool'], **kw)
    after = tpe.suggest([100, 101], s['domain'], s['trials'], 9, batch=True, pool=None, pool_replace=False, **kw)
    assert before == after
    assert all('pool_index' not in d['misc'] for d in after)
