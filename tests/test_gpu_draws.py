"""Every sampling path of the engine against the pointwise draw reference
(oracle/draw_oracle.py).  Requires a real MI355X (`-m gpu`).

The common rule: a device value is compared elementwise with the fp64 port
(draw_fp64 on the candidate's own Philox words) over all draws, and with the
140-digit exact draw on a subset of at most 2000 per case that always holds
the 200 largest |z|, the 200 draws nearest each bound and every draw of a
component whose pick interval is at most 16 words wide.  The tolerance is
T_DEV = 4 T_PORT (tests/test_draw_oracle.py: the port's own measured error
against the exact draw, doubled) in the two-term form T sigma_k max(1, |z|)
+ 2^-51 (|mu_k| + |x|); LGMM1 values relative, with 2^-51 (1 + |log x|)
added; quantized values and categorical indices equal.  A draw may be left
out only where the words sit on a threshold, at an end of the uniform word
or on a rounding boundary of a quantized value -- and the committed seeds
leave none out (test_draw_oracle.py checks that without a GPU).

* entry points: Engine.GMM1 / LGMM1 / categorical (k_sample_only, the
  binary search on the fp64 cdf) at the corners of (offset, stream, round,
  seed);
* small rounds: a round of one candidate returns that candidate, so rounds
  of one candidate at offset g show every candidate the round draws.  The
  split-K map, and the dense and categorical labels of the packed map, pick
  by the binary search on the fp64 cdf in global memory (SampGlobal /
  cdf_search); the staged pick in LDS (SampShared) runs for the quantized
  labels of the packed maps: its guided search (w4_q, w4_2.5_3.5_logq,
  k64_q), its branch-free search (cell6_q: six cumulative weights in one
  guide cell) and the unstaged fallback at K_b > 64 (k65_q) each have a
  quantized label here, with threshold words (test_threshold_words) where
  an off-by-one compare shows.  The round posterior's quantized labels are
  drawn by k_qsample (one of them has no bounds); a second posterior with
  every quantized label bounded, the same thresholds and streams, runs the
  same draws and threshold words through k_qfused, and the round's
  evaluation count shows that it did (test_fused_quantized_rounds);
* tile rounds: the winner of the tile map, of the hot-bin prefilter and of
  its fallback is the port's candidate at the reported index, and that
  index's oracle score is the round's best.

Seen through winners only (no draw but the winning one is observable
without a new entry point): the dense labels' staged picks in the expansion
screen and the prefilter (k_screen_bx, k_hot_bx, k_hot_draw), the quantized
tile kernel (k_qfused_tiles) and k_cat_tiles' 64-entry guide, which no small
round runs -- a small round draws its categorical labels by cdf_search, so
the 70-option label checks that search, not the guide.
"""
import numpy as np
import pytest

from oracle import draw_oracle as D
from oracle import tpe_oracle as O
from tests import draw_cases as C
from tests.draw_check import T_DEV, WORST, check_draws, ratio
from tests.test_draw_oracle import T_PORT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    """(the worst device error per path, for the record: printed with -s)"""
    yield
    for path, (rp, re) in sorted(WORST.items()):
        print('%-16s worst %.3g x T_port against the port, %.3g x T_port against the exact draw' % (path, rp, re))


_folds = {}


def _fold(key, make):
    if key not in _folds:
        _folds[key] = make()
    return _folds[key]


# -- a. entry points ---------------------------------------------------------
@pytest.mark.parametrize('corner', range(len(C.CORNERS)))
@pytest.mark.parametrize('name', C.ENTRY_NAMES)
def test_entry_point_draws(eng, name, corner):
    offset, stream, rnd, seed = C.CORNERS[corner]
    f = _fold(name, lambda: C.entry_fold(name))
    g = offset + np.arange(C.N_ENTRY, dtype=np.uint64)
    wp, wu = D.draw_words(seed, stream, rnd, g, categorical=f.categorical)
    kw = dict(seed=seed, size=(C.N_ENTRY,), stream=stream, round=rnd, offset=offset)
    if f.categorical:
        got = eng.categorical(f.w, **kw)
    else:
        fn, args, bounds = C.engine_kwargs(name)
        got = getattr(eng, fn)(*args, **bounds, **kw)
    check_draws(f, wp, wu, got, 'entry', '%s %s' % (name, C.CORNERS[corner]))


# -- b. small rounds ----------------------------------------------------------
# The maps of a small round: split-K (the default up to 2048 slots per
# label), packed (splitk 0) and packed without the grid-value table (dedup
# 0).  Both packed maps draw the quantized labels of the round posterior in
# k_qsample (with dedup 0 k_qscan then scores every candidate instead of
# reading a table); k_qfused needs every quantized label bounded and runs in
# test_fused_quantized_rounds.
MAPS = {'splitk': {}, 'packed': {'splitk': 0}, 'packed_direct': {'splitk': 0, 'dedup': 0}}


@pytest.fixture(scope='module')
def round_case():
    from hyperopt_amd import posterior as P
    posts = C.round_posterior()
    return posts, P.pack(posts), [C.fold_posterior(p) for p in posts]


class _round_map(object):
    """The module's engine with the small rounds' posterior on the given map
    (the options restored on exit)."""

    def __init__(self, eng, packed, name):
        self.eng, self.packed, self.opts = eng, packed, MAPS[name]

    def __enter__(self):
        for k, v in self.opts.items():
            self.eng.set_option(k, v)
        self.eng.set_posterior(*self.packed)
        return self.eng

    def __exit__(self, *exc):
        for k in self.opts:
            self.eng.set_option(k, 1)


@pytest.mark.parametrize('seed', C.ROUND_SEEDS)
@pytest.mark.parametrize('rmap', sorted(MAPS))
def test_one_candidate_rounds(eng, round_case, rmap, seed):
    """64 rounds of one candidate at every offset g: value = the port's
    candidate g of that round, index = g."""
    posts, packed, folds = round_case
    with _round_map(eng, packed, rmap) as e:
        res = np.stack([e.suggest_batch(seed, C.ROUND_IDS, 1, cand_offset=g) for g in C.ROUND_G])
    g = np.asarray(C.ROUND_G, dtype=np.uint64)[:, None]
    rounds = np.asarray(C.ROUND_IDS, dtype=np.uint64)[None, :]
    assert res.shape == (len(C.ROUND_G), len(C.ROUND_IDS), len(posts))
    for li, f in enumerate(folds):
        assert np.array_equal(res[:, :, li]['index'], np.broadcast_to(g.astype(np.int64), res.shape[:2])), li
        assert np.all(res[:, :, li]['label'] == li)
        wp, wu = D.draw_words(seed, li, rounds, g, categorical=f.categorical)
        got = res[:, :, li]['value'].ravel()
        check_draws(f, wp.ravel(), wu.ravel(), got.astype(np.int64) if f.categorical else got,
                    rmap, '%s seed %#x' % (posts[li].label, seed))


@pytest.mark.parametrize('n', [2, 3])
@pytest.mark.parametrize('rmap', sorted(MAPS))
def test_few_candidate_rounds(eng, round_case, rmap, n):
    """Rounds of two and three candidates: the winner is the port's
    candidate at the reported index."""
    posts, packed, folds = round_case
    seed = C.ROUND_SEEDS[n & 1]
    offs = list(range(16)) + [(1 << 32) - 1 - n]
    with _round_map(eng, packed, rmap) as e:
        res = np.stack([e.suggest_batch(seed, C.ROUND_IDS, n, cand_offset=g) for g in offs])
    g0 = np.asarray(offs, dtype=np.int64)[:, None]
    rounds = np.broadcast_to(np.asarray(C.ROUND_IDS, dtype=np.uint64)[None, :], res.shape[:2])
    for li, f in enumerate(folds):
        idx = res[:, :, li]['index']
        assert np.all((idx >= g0) & (idx < g0 + n)), li
        wp, wu = D.draw_words(seed, li, rounds.ravel(), idx.ravel().astype(np.uint64), categorical=f.categorical)
        got = res[:, :, li]['value'].ravel()
        check_draws(f, wp, wu, got.astype(np.int64) if f.categorical else got, rmap,
                    '%s n %d' % (posts[li].label, n))


@pytest.mark.parametrize('rmap', sorted(MAPS))
def test_threshold_words(eng, round_case, rmap):
    """Candidates whose pick word is a threshold's last word below or first
    word at it (draw_cases.THRESHOLD_WORDS; unbounded and categorical labels,
    whose thresholds are exact integers): an off-by-one compare in a pick
    moves these draws to a neighbouring component.  Reached this way: the
    binary search on the fp64 cdf (the entry points, every label of a split-K
    round, the dense and categorical labels of a packed one, and k65_q, which
    is not staged), and in the quantized kernels of the packed maps the
    staged guided search (k64_q) and the staged branch-free search
    (cell6_q); the quantized labels' neighbouring components give different
    values."""
    posts, packed, folds = round_case
    seed = C.ROUND_SEEDS[0]
    with _round_map(eng, packed, rmap) as e:
        for li, (p, f) in enumerate(zip(posts, folds)):
            for g in C.THRESHOLD_WORDS.get(p.label, ()):
                wp, wu = D.draw_words(seed, li, 0, np.array([g], dtype=np.uint64), categorical=f.categorical)
                k, z, x, val = D.draw_fp64(f, wp, wu)
                res = e.suggest_batch(seed, [0], 1, cand_offset=g)[0, li]
                kw = dict(seed=seed, size=(1,), stream=li, round=0, offset=g)
                if f.categorical:       # (the single ops leave the resident posterior in place)
                    entry = e.categorical(p.below, **kw)
                    assert int(res['value']) == int(k[0]) == int(entry[0]), (p.label, g)
                    continue
                entry = e.GMM1(*p.below, low=p.low, high=p.high, q=p.q, **kw)
                for got in (res['value'], entry[0]):
                    r = ratio(f, k, z, x, np.array([got]))
                    assert r[0] <= T_DEV / T_PORT, (p.label, g, got, val[0], int(k[0]))


def _fused_grid(p):
    """The grid a bounded quantized label's table spans in the fused path:
    floor(low / q) - 1 .. ceil(high / q) + 1 (LGMM1: of exp(low), exp(high))."""
    lo, hi = (np.exp(p.low), np.exp(p.high)) if p.family == 'LGMM1' else (p.low, p.high)
    return int(np.ceil(hi / p.q) + 1) - int(np.floor(lo / p.q) - 1) + 1


def test_fused_quantized_rounds(eng):
    """k_qfused, the packed map's kernel for posteriors whose quantized
    labels all have bounds: 600 rounds of one candidate at a few offsets
    (every draw under the common rule) and at the threshold words of the
    three wide labels (round 0's draw), on draw_cases.FUSED_LABELS.  That the
    fused path ran: it counts grid values x components per label, with the
    grid taken from the bounds (the sampled path's grid, taken from the
    drawn values, is narrower, and its untabled count is slots x components)."""
    from hyperopt_amd import posterior as P
    posts = C.round_posterior(C.FUSED_LABELS)
    quant = [(li, p, C.fold_posterior(p)) for li, p in enumerate(posts) if p.q is not None]
    assert len(quant) == 5 and all(p.low is not None and p.high is not None for _, p, _ in quant)
    want = {fam: sum(_fused_grid(p) * (len(p.below[0]) + len(p.above[0])) for _, p, _ in quant if p.family == fam)
            for fam in ('GMM1', 'LGMM1')}
    seed = C.ROUND_SEEDS[0]
    assert C.FUSED_IDS[0] == 0
    words = sorted((g, li) for li, p, _ in quant for g in C.THRESHOLD_WORDS.get(p.label[:-1], ())
                   if p.label.endswith('_qb'))
    assert len(words) == sum(len(C.THRESHOLD_WORDS[n]) for n in ('k64_q', 'cell6_q', 'k65_q'))
    res = {}
    with _round_map(eng, P.pack(posts), 'packed') as e:
        for g in C.FUSED_G + [g for g, _ in words]:
            res[g] = e.suggest_batch(seed, C.FUSED_IDS, 1, cand_offset=g)
            stats = e.last_mode_stats()
            assert (stats['quant_gmm1'][1], stats['quant_lgmm1'][1]) == (want['GMM1'], want['LGMM1']), (g, stats)
    rounds = np.asarray(C.FUSED_IDS, dtype=np.uint64)[None, :]
    gg = np.asarray(C.FUSED_G, dtype=np.uint64)[:, None]
    for li, p, f in quant:
        got = np.stack([res[g][:, li] for g in C.FUSED_G])
        assert np.array_equal(got['index'], np.broadcast_to(gg.astype(np.int64), got.shape))
        wp, wu = D.draw_words(seed, li, rounds, gg)
        check_draws(f, wp.ravel(), wu.ravel(), got['value'].ravel(), 'packed fused', p.label)
    folds = {li: f for li, p, f in quant}
    for g, li in words:
        f = folds[li]
        wp, wu = D.draw_words(seed, li, 0, np.array([g], dtype=np.uint64))
        k, z, x, val = D.draw_fp64(f, wp, wu)
        got = res[g][0, li]
        assert int(got['index']) == g
        assert ratio(f, k, z, x, np.array([got['value']]))[0] <= T_DEV / T_PORT, (posts[li].label, g, got['value'], val[0])


# -- c. tile rounds and the hot-bin prefilter --------------------------------
@pytest.fixture(scope='module')
def tile_case():
    from hyperopt_amd import posterior as P
    posts = C.tile_posteriors()
    return posts, P.pack(posts), [C.fold_posterior(p) for p in posts]


def _oracle_scores(p, cand):
    if p.family == 'categorical':
        c = cand.astype(np.int64)
        return O.categorical_lpdf(c, p.below) - O.categorical_lpdf(c, p.above)
    f = O.gmm1_lpdf if p.family == 'GMM1' else O.lgmm1_lpdf
    kw = dict(low=p.low, high=p.high, q=p.q)
    vals, inv = np.unique(cand, return_inverse=True) if p.q is not None else (cand, slice(None))
    return (f(vals, *p.below, **kw) - f(vals, *p.above, **kw))[inv]


@pytest.mark.parametrize('C_seed_round', C.TILE_ROUNDS, ids=lambda v: 'C%d' % v[0])
def test_tile_round_winners(eng, tile_case, C_seed_round):
    """The round with the hot-bin prefilter, with its forced fallback and
    with the screen off, against the same port candidates: the winner's
    value is the port's candidate at the reported index, and that index's
    oracle score is within 1e-9 (the parity bar) of the best over all C."""
    n, seed, rnd = C_seed_round
    posts, packed, folds = tile_case
    eng.set_posterior(*packed)
    g = np.arange(n, dtype=np.uint64)
    runs = {}
    try:
        runs['hot'] = eng.suggest(seed, n, round=rnd)
        mode, hot, screened = eng.last_screen_mode(), eng.last_hot(), eng.last_screen()
        eng.set_option('hot', 2)
        runs['fallback'] = eng.suggest(seed, n, round=rnd)
        mode_f, hot_f = eng.last_screen_mode(), eng.last_hot()
        eng.set_option('hot', 1)
        eng.set_option('screen', 0)
        runs['unscreened'] = eng.suggest(seed, n, round=rnd)
        assert eng.last_screen() == (0, 0)
    finally:
        eng.set_option('hot', 1)
        eng.set_option('screen', 1)
    print('C %d: screen mode %d, hot %s; fallback: mode %d, hot %s' % (n, mode, hot, mode_f, hot_f))
    if n >= 8192:       # the expansion screen behind the prefilter, no fallback; then the forced fallback
        assert mode == 3 and hot[0] > 0 and hot[1] == 0, (mode, hot)
        assert mode_f == 3 and hot_f[1] == 1, (mode_f, hot_f)
        assert screened[0] > 0
    else:               # below the tile screens' threshold: no prefilter
        assert hot[0] == -1 and hot[1] == 0, hot
    for li, (p, f) in enumerate(zip(posts, folds)):
        wp, wu = D.draw_words(seed, li, rnd, g, categorical=f.categorical)
        k, z, x, val = D.draw_fp64(f, wp, wu)
        assert not D.excluded(f, wp, wu, x).any()
        score = _oracle_scores(p, np.asarray(val, dtype=np.float64))
        best = np.nanmax(score)
        for path, res in runs.items():
            i = int(res[li]['index'])
            assert 0 <= i < n
            got = np.array([int(res[li]['value']) if f.categorical else res[li]['value']])
            check_draws(f, wp[i:i + 1], wu[i:i + 1], got, 'tile ' + path, '%s C %d' % (p.label, n))
            assert abs(score[i] - best) <= 1e-9, (path, li, i, score[i], best)
