"""Value-only packed rounds (TPE_OPT_VALUE_ONLY, what tpe.suggest runs)
against the unscreened fp64 round and an exact reference, at the edge
posteriors of tests/bx_cases.py.

k_pick_win settles a (round, label) cell from the screen's bounds alone:
one candidate whose lower bound clears every other upper bound by
kValueMargin = 1e-9 (relative) is reported by index and value and no fp64
lpdf is computed for the cell, so nothing downstream can notice a bound
that does not hold.  Both of its screens are run here -- the expansion
screen ('bx', bounds as double2) and the windowed fp32 screen ('win',
expand off, bounds as float2) -- beside k_pick_packed ('plain', which
decides nothing), on 352 rounds of 24 candidates: 8448 slots, just past
kWinMinN = 8192, the second workgroup of k_pick_win partial, the last two
ids 7 + 2^20 and 2^31 - 1.

Per case and setting, three runs of the same call: screen off (the
baseline, independent of every screen), screen on, screen on with
value-only.  Index and value are the baseline's bytewise for every label;
the two exact runs are the same records; a decided cell carries status 1 and
NaN lpdfs and every other cell is the exact record (helpers.value_only_cells).
Independently of the GPU's scoring, each round's candidates are drawn again
through the sampler entry point and scored by tests/bx_reference.py in long
double (value_only_cases.check_cells): the value is the draw at the index,
the winner is within 1e-9 of the exact best, and a decided winner is the
strict exact argmax by at least half of kValueMargin -- the bounds are
rigorous against the fp64 score, which is within ~1e-12 of the exact one, so
a smaller exact lead means an unsound bound.  A cell is left out of that
check only when one of its candidates has no finite exact score, at most 1 %
of a label's cells.  over_unclipped (16386 above components) is scored for
its first 64 rounds and the two large ids only: the long-double reference
takes ~16 s for all of its cells.

Every (case, setting) under 'bx' and 'win' decides at least one cell per
dense label -- under expand = 0 that also shows the windowed packed path
ran -- but zero_weight under 'bx', whose screen certifies nothing
(test_bx_index_gpu.test_screen_score_within_its_bound).  The decided shares
are printed, not asserted (DESIGN.md section 4 records them).

Candidate counts: the packed map holds C < kTile = 1024 candidates per round
(round_args), so C = 1023 is the last size k_pick_win sees and the last the
packed expansion screen (kBxR x kBlock = 1024 slots per workgroup) takes;
C = 1024 runs the tile map, whose rounds of 1024 < kWinMinN candidates take
the plain fp32 screen and re-score every near-tie: value-only changes
nothing there, and the test holds it to exactly that.
"""
import numpy as np
import pytest

from tests import bx_cases as C
from tests import value_only_cases as V
from tests.bx_reference import LabelRef
from tests.helpers import value_only_cells

pytestmark = pytest.mark.gpu

SETTINGS = {'bx': {}, 'win': {'expand': 0}, 'plain': {'expand': 0, 'window': 0}}
DEFAULTS = {'screen': 1, 'value_only': 0, 'expand': 1, 'window': 1, 'rescore_cap': 1 << 16, 'pk_sliced': 8192}
SEED = 4711


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


_refs, _packed, _draws, _scores = {}, {}, {}, {}


def _ref(name, li):
    if (name, li) not in _refs:
        _refs[(name, li)] = LabelRef(C.posts(name)[li])
    return _refs[(name, li)]


def _set(eng, name):
    from hyperopt_amd import posterior as P
    if name not in _packed:
        _packed[name] = P.pack(C.posts(name))
    eng.set_posterior(*_packed[name])
    return C.posts(name)


def _restore(eng):
    for k, v in DEFAULTS.items():
        eng.set_option(k, v)


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _three_runs(eng, ids, n_cand, opts):
    """(baseline, exact, value-only, screen mode of the exact run) of one call."""
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.set_option('screen', 0)
        base = eng.suggest_batch(SEED, ids, n_cand)
        assert eng.last_screen_mode() == 0
        eng.set_option('screen', 1)
        exact = eng.suggest_batch(SEED, ids, n_cand)
        mode = eng.last_screen_mode()
        eng.set_option('value_only', 1)
        vo = eng.suggest_batch(SEED, ids, n_cand)
    finally:
        _restore(eng)
    return base, exact, vo, mode


def _same_rounds(base, exact, vo):
    """The bytewise assertions; returns the decided mask [rounds, labels]."""
    for f in ('index', 'value'):
        assert _bytes(base[f]) == _bytes(exact[f]) == _bytes(vo[f]), f
    assert _bytes(base) == _bytes(exact)
    return value_only_cells(exact, vo)


def _checked_rows(name, n_rounds):
    if name == 'over_unclipped':     # (module docstring: the first 64 rounds and the two large ids)
        return np.r_[0:V.N_CHECKED_OVER_UNCLIPPED, n_rounds - 2:n_rounds]
    return np.arange(n_rounds)


def _redraw(eng, name, li, ids, n_cand):
    """Each round's candidates of one dense label from the sampler entry
    point [rounds, n_cand] (drawn once per shape, never modified)."""
    key = (name, li, len(ids), n_cand)
    if key not in _draws:
        p = C.posts(name)[li]
        samp = eng.GMM1 if p.family == 'GMM1' else eng.LGMM1
        x = np.empty((len(ids), n_cand))
        for r, rid in enumerate(ids):
            x[r] = samp(*p.below, low=p.low, high=p.high, q=None, seed=SEED, size=(n_cand,), stream=li, round=rid)
        x.setflags(write=False)
        _draws[key] = x
    return _draws[key]


def _exact_scores(name, li, x, rows):
    """LabelRef.score_exact of the checked rounds' candidates [len(rows), n_cand]."""
    key = (name, li) + x.shape
    if key not in _scores:
        ref = _ref(name, li)
        flat = x[rows].ravel()
        chunk = 2048 if len(ref.side[1]['w']) <= 4096 else 128     # (long-double temporaries of chunk x components)
        with np.errstate(invalid='ignore'):
            s = ref.lpdf_exact(flat, 0, chunk) - ref.lpdf_exact(flat, 1, chunk)
        s = s.reshape(len(rows), x.shape[1])
        s.setflags(write=False)
        _scores[key] = s
    return _scores[key]


def _independent(eng, name, setting, posts, ids, n_cand, vo, decided):
    """The value-only round against the re-drawn candidates' exact scores;
    returns per dense label (cells checked, cells skipped)."""
    out = []
    rows = _checked_rows(name, len(ids))
    for li in C.dense_labels(posts):
        x = _redraw(eng, name, li, ids, n_cand)
        idx = vo['index'][:, li]
        assert np.all((idx >= 0) & (idx < n_cand)), (name, setting, li)
        got = x[np.arange(len(ids)), idx]
        assert _bytes(got) == _bytes(vo['value'][:, li]), '%s %s label %d: value is not the draw at index' % (
            name, setting, li)
        s = _exact_scores(name, li, x, rows)
        skipped, fails = V.check_cells(s, idx[rows], decided[rows, li])
        if fails:
            r, what, w, sw, o, so = fails[0]
            raise AssertionError(
                '%s %s: %d of %d cells fail; first: round id %d, label %d (%s): %s; winner %d x = %r exact score '
                '%.17g, rival %d x = %r exact score %.17g' % (
                    name, setting, len(fails), len(rows), ids[rows[r]], li,
                    'decided' if decided[rows[r], li] else 'not decided', what, w, x[rows[r], w], sw, o,
                    x[rows[r], o] if o >= 0 else None, so))
        assert skipped.mean() <= V.MAX_SKIPPED, (name, setting, li, float(skipped.mean()))
        out.append((len(rows), int(skipped.sum())))
    return out


def _case(eng, name, setting, ids, n_cand, decides=None):
    """One (case, setting, shape): every assertion of the module docstring.
    decides: False -- no cell may be decided; True -- at least one per dense
    label; None -- by the setting.  Returns (decided mask, screen mode)."""
    posts = _set(eng, name)
    base, exact, vo, mode = _three_runs(eng, ids, n_cand, SETTINGS[setting])
    decided = _same_rounds(base, exact, vo)
    dense = C.dense_labels(posts)
    other = [li for li in range(len(posts)) if li not in dense]
    assert not decided[:, other].any()
    checked = _independent(eng, name, setting, posts, ids, n_cand, vo, decided)
    per = [int(decided[:, li].sum()) for li in dense]
    print('value-only %-14s %-5s C = %-4d: decided %6d of %6d dense cells (%.4f); per label %s; screen mode %d; '
          'exact check left out %s of %s cells' % (
              name, setting, n_cand, sum(per), len(ids) * len(dense), sum(per) / float(len(ids) * len(dense)), per,
              mode, [k for _, k in checked], [n for n, _ in checked]))
    if decides is None:
        decides = setting != 'plain' and not (name == 'zero_weight' and setting == 'bx')
    if decides:
        assert min(per) >= 1, (name, setting, per)
    else:
        assert sum(per) == 0, (name, setting, per)
    return decided, mode


# ('bx' for the posteriors that get an index: without one the defaults run the windowed screen, which is 'win')
CASE_SETTINGS = [(n, s) for n in C.CASES for s in SETTINGS if s != 'bx' or n in C.ELIGIBLE]


@pytest.mark.parametrize('name,setting', CASE_SETTINGS)
def test_value_only_round_is_exact(eng, name, setting):
    _, mode = _case(eng, name, setting, V.default_ids(), V.C_DEFAULT)
    if setting == 'bx':
        assert mode == 3


@pytest.mark.parametrize('n_cand', V.COUNTS + [V.K_TILE - 1])
def test_value_only_candidate_counts(eng, n_cand):
    """C = 1: a cell with a certified candidate is decided with second =
    -inf and its value is still the draw.  C = 256, 257: one round per
    workgroup slot row of the packed maps and one past it.  C = 1023: the
    last packed size.  C = 1024: the tile map (module docstring): nothing
    decided, the plain fp32 screen."""
    ids = V.default_ids(V.rounds_for(n_cand))
    packed = n_cand < V.K_TILE
    for name in ('uniform3', 'three_labels'):
        for setting in ('bx', 'win'):
            decided, mode = _case(eng, name, setting, ids, n_cand, decides=packed)
            if packed:
                assert mode == (3 if setting == 'bx' else 0), (name, setting, mode)
            else:
                assert mode == 1, (name, setting, mode)


def test_value_only_below_the_threshold(eng):
    """341 x 24 = 8184 slots: k_pick_packed, no screen mode, nothing decided,
    the three runs the same records."""
    _set(eng, 'uniform300')
    ids = V.default_ids(V.N_BELOW_THRESHOLD)
    base, exact, vo, mode = _three_runs(eng, ids, V.C_DEFAULT, {})
    assert mode == 0
    assert not value_only_cells(exact, vo).any()
    assert _bytes(base) == _bytes(exact) == _bytes(vo)


@pytest.mark.parametrize('name', ['three_labels', 'below200'])
def test_value_only_rescore_paths(eng, name):
    """The windowed value-only round with its re-score buffers forced to
    overflow (rescore_cap = 1: the round runs again) and with the chunked
    re-score in place of the sliced one (pk_sliced = 0): the default run's
    bytes, decided and undecided cells mixed in one label's list."""
    posts = _set(eng, name)
    ids = V.default_ids()
    try:
        eng.set_option('expand', 0)
        exact = eng.suggest_batch(SEED, ids, V.C_DEFAULT)
        eng.set_option('value_only', 1)
        a = eng.suggest_batch(SEED, ids, V.C_DEFAULT)
        listed = eng.last_screen()[1]
        eng.set_option('rescore_cap', 1)
        b = eng.suggest_batch(SEED, ids, V.C_DEFAULT)
        eng.set_option('rescore_cap', DEFAULTS['rescore_cap'])
        eng.set_option('pk_sliced', 0)
        c = eng.suggest_batch(SEED, ids, V.C_DEFAULT)
    finally:
        _restore(eng)
    decided = value_only_cells(exact, a)
    per = [int(decided[:, li].sum()) for li in C.dense_labels(posts)]
    print('%s: decided per label %s of %d, %d candidates re-scored' % (name, per, len(ids), listed))
    assert any(0 < k < len(ids) for k in per), per
    assert listed > 1       # (past rescore_cap = 1: the overflow rerun)
    assert _bytes(a) == _bytes(b)
    assert _bytes(a) == _bytes(c)


def test_suggest_batch_documents_do_not_depend_on_value_only():
    """tpe.suggest as shipped (the cached engine: value-only on) just after
    the 20 startup trials -- 1 to 3 below components, a handful above -- for
    512 new ids of 24 candidates: the documents of the exact rounds and of the
    unscreened rounds carry the same values."""
    import hyperopt_amd as H
    from hyperopt_amd import hp, tpe
    from hyperopt_amd.engine import get_engine
    space = {'u': hp.uniform('u', -5, 5), 'lu': hp.loguniform('lu', -3, 3), 'n': hp.normal('n', 0, 2),
             'ln': hp.lognormal('ln', 0, 1), 'q': hp.quniform('q', 0, 10, 1), 'c': hp.choice('c', [0, 1, 2])}

    def loss(d):
        return d['u'] ** 2 + abs(np.log(d['lu'])) + d['n'] ** 2 + d['ln'] + 0.1 * d['q'] + d['c']
    dom = H.Domain(lambda d: 0, space)
    trials = H.Trials()
    ids = list(range(1000, 1512))
    eng = get_engine(0, 'f64')
    try:
        for n_trials in (21, 30):
            H.fmin(loss, space, algo=tpe.suggest, max_evals=n_trials, trials=trials,
                   rstate=np.random.RandomState(8))
            assert len(trials.trials) == n_trials
            for builder in ('host', 'device'):
                def vals():
                    docs = tpe.suggest(ids, dom, trials, 31 + n_trials, batch=True, posterior_builder=builder)
                    assert [d['tid'] for d in docs] == ids
                    return [d['misc']['vals'] for d in docs]
                eng.set_option('value_only', 1)
                eng.set_option('screen', 1)
                shipped = vals()
                assert eng.last_screen_mode() == 3      # (the packed expansion screen: k_pick_win ran)
                eng.set_option('value_only', 0)
                exact = vals()
                eng.set_option('screen', 0)
                plain = vals()
                assert shipped == exact, (n_trials, builder)
                assert shipped == plain, (n_trials, builder)
    finally:
        eng.set_option('value_only', 1)
        eng.set_option('screen', 1)
