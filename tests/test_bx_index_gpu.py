"""The expansion index (hyperopt_amd/csrc/tpe_expand.hip) against an exact
reference (tests/bx_reference.py) at the posteriors of tests/bx_cases.py:
the smallest shapes that still take each branch of bx_build and of the
index's kernels.

Per eligible case and dense label, candidates aimed at every edge the code
has (range bounds, component means, bin and sub-bin edges from
Engine.bx_layout and their neighbouring doubles), and:

* the sub-bin intervals of tpe_hot_probe bracket the exact score, exist
  wherever both exact lpdfs are representable, and are no wider than the
  score's own oscillation plus a cap;
* the sub-bin sampling masses agree with the exact interval masses of the
  truncated below mixture;
* the expansion screen's score is within its own bound of the exact score;
* the round is the unscreened fp64 round, bytewise, in every screen setting,
  and its winner is the exact reference's best candidate;
* a replaced posterior never sees the previous posterior's index.

Ineligible posteriors (too many bins, too many unclipped components, an above
mixture out of mu order) get no index: the probe fails, the round takes the
windowed screen and still equals the fp64 round.

A failing bound is reported with its label, bin and sub-bin.
"""
import numpy as np
import pytest

from tests import bx_cases as C
from tests.bx_reference import LD, LabelRef
from tests.helpers import _assert_same

pytestmark = pytest.mark.gpu

K_SUB = C.K_SUB
N_ROUND = 1 << 14          # >= kWinMinN = 8192: the smallest rounds that use the index
# The median over a case's probed sub-bins of (U - L) - osc, osc the exact
# score's oscillation over the sub-bin, as measured per case (DESIGN.md
# section 4; a case of several labels: its largest).  The test asserts twice
# the case's own figure -- the factor covers the last bits of the tables
# from one build to the next -- and so never more than twice the largest of
# them, 3.8e-3.  The excess is the price of bounding the mixtures term by
# term -- every component's largest term over the sub-bin above, its
# smallest below -- and shrinks with the sub-bin; the kernel's own widening
# 2 x 1e-7 (1 + |v|) and the float rounding of U and L are its floor
# (max_bins).
WIDTH_MEDIAN = {
    'uniform300': 8.16e-4, 'uniform3': 1.84e-3, 'normal30': 1.82e-3, 'lognormal150': 3.81e-4,
    'loguniform_far': 1.26e-3, 'offset1e6': 7.97e-4, 'ties50': 1.29e-3, 'at_bounds': 1.65e-3,
    'all_clipped': 7.98e-4, 'zero_weight': 8.22e-4, 'zero_above': 8.06e-4, 'below64': 3.80e-3,
    'below65': 3.43e-3, 'below200': 3.42e-3, 'max_bins': 9.05e-7, 'three_labels': 1.84e-3,
}
# the cases whose below mixture is past kStageBelow = kSampLds = 64 components
NO_PREFILTER = ('below65', 'below200')


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


_refs, _packed = {}, {}


def _ref(name, li):
    if (name, li) not in _refs:
        _refs[(name, li)] = LabelRef(C.posts(name)[li])
    return _refs[(name, li)]


def _set(eng, name, **opts):
    """The case's posterior made resident (its index is then built by the
    first probe or round, with the options in force)."""
    from hyperopt_amd import posterior as P
    if name not in _packed:
        _packed[name] = P.pack(C.posts(name))
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.set_posterior(*_packed[name])
    return C.posts(name)


def _sub_edges(lay, bins):
    """Draw-space edges of the 16 sub-bins of each bin in `bins`: [len(bins), 17]."""
    sw = lay['bw'] / K_SUB
    j = np.asarray(bins, dtype=np.int64)[:, None] * K_SUB + np.arange(K_SUB + 1)[None, :]
    return lay['centre'] + lay['xlo'] + j * sw


def _probed_bins(lay):
    return np.unique(np.linspace(0, lay['nbins'] - 1, 64).astype(np.int64))


def _candidates(eng, li, p, ref, lay):
    """Value-space candidates of one label (module docstring)."""
    nsb = lay['nbins'] * K_SUB
    sw = lay['bw'] / K_SUB
    lo = lay['centre'] + lay['xlo']
    hi = lo + lay['nbins'] * lay['bw']
    inf = np.inf
    parts = [ref.to_value(np.linspace(lo, hi, 4097))]
    ends = ref.to_value(np.array([p.low, p.high] if p.low is not None else [lo, hi]))
    parts.append(np.concatenate([ends, np.nextafter(ends, -inf), np.nextafter(ends, inf)]))
    mu_a = np.sort(np.asarray(p.above[1], dtype=float))
    parts.append(ref.to_value(np.concatenate([p.below[1], mu_a, 0.5 * (mu_a[:-1] + mu_a[1:])])))
    samp = eng.GMM1 if p.family == 'GMM1' else eng.LGMM1
    parts.append(samp(*p.below, low=p.low, high=p.high, q=None, seed=5, size=(2048,), stream=li))
    e = ref.to_value(_sub_edges(lay, _probed_bins(lay)).ravel())
    parts.append(np.concatenate([e, np.nextafter(e, -inf), np.nextafter(e, inf)]))
    parts.append(ref.to_value(lo + (np.array([0, 1, nsb - 1, nsb]) * sw)))                # first, last sub-bin: edges
    parts.append(ref.to_value(lo + (np.array([0.5, nsb - 0.5]) * sw)))                    # and midpoints
    outside = ref.to_value(np.array([lo - lay['bw'], lo - 100 * lay['bw'], hi + lay['bw'], hi + 100 * lay['bw']]))
    x = np.concatenate(parts + [outside])
    assert len(x) < 16384
    return x, len(x) - 4


def _position(ref, lay, x):
    """Fractional sub-bin index of value(s) x as the host computes it (the
    device's differs by rounding only: ~1e-6 of a sub-bin at |centre| = 1e6)."""
    return (ref.to_draw(x) - lay['centre'] - lay['xlo']) * (K_SUB / lay['bw'])


def _where(ref, lay, x):
    f = float(_position(ref, lay, np.array([x]))[0])
    j = int(np.floor(f)) if np.isfinite(f) else -1
    return 'x = %r: bin %d, sub-bin %d (position %.6f of %d sub-bins)' % (x, j // K_SUB, j % K_SUB, f,
                                                                          lay['nbins'] * K_SUB)


def _check_bracket(name, li, ref, lay, x, u, l, s):
    fin = np.isfinite(s)
    bad = fin & ~((l.astype(LD) <= s) & (s <= u.astype(LD)))
    if bad.any():
        k = int(np.where(bad)[0][0])
        raise AssertionError('%s label %d: %d of %d bounds miss the exact score; first: %s, L %.9g, exact %.12g, '
                             'U %.9g' % (name, li, int(bad.sum()), int(fin.sum()), _where(ref, lay, float(x[k])),
                                         l[k], float(s[k]), u[k]))


def _probe_case(eng, name, posts):
    """Per dense label: (li, p, ref, lay, candidates x, how many of them lie inside the bins, u, l, m)."""
    out = []
    for li in C.dense_labels(posts):
        p, ref = posts[li], _ref(name, li)
        lay = eng.bx_layout(li)
        x, n_in = _candidates(eng, li, p, ref, lay)
        u, l, m = eng.hot_probe(li, x)
        out.append((li, p, ref, lay, x, n_in, u, l, m))
    return out


def _bounds_hold_and_exist(eng, name, posts, exist=True):
    shares = []
    for li, p, ref, lay, x, n_in, u, l, m in _probe_case(eng, name, posts):
        lb, la = ref.lpdf_exact(x, 0), ref.lpdf_exact(x, 1)
        with np.errstate(invalid='ignore'):
            s = lb - la
        _check_bracket(name, li, ref, lay, x, u, l, s)
        # outside the bins: no bound, no mass
        assert np.all(u[n_in:] == np.inf) and np.all(l[n_in:] == -np.inf) and np.all(m[n_in:] == 0.0), (name, li)
        assert np.all(m >= 0.0)
        # inside, wherever both lpdfs are far from underflow: finite bounds
        f = _position(ref, lay, x)
        inside = (f >= 1e-3) & (f <= lay['nbins'] * K_SUB - 1e-3)
        want = inside & (lb > -300) & (la > -300)
        if name == 'offset1e6':
            # |centre| = 1e6: the absolute slack 1e-15 |centre| of a sub-bin's
            # edges is past the 0.5e-9 bw allowance of rmax, so the first and
            # last sub-bin of every bin get no bound (slower, never wrong):
            # the 14 interior ones must have one
            sub = np.floor(f).astype(np.int64) % K_SUB
            frac = f - np.floor(f)
            want &= (sub >= 1) & (sub <= K_SUB - 2) & (frac > 0.01) & (frac < 0.99)
        have = np.isfinite(u) & np.isfinite(l)
        shares.append(float(have[inside].mean()))
        miss = want & ~have
        if exist and miss.any():
            k = int(np.where(miss)[0][0])
            raise AssertionError('%s label %d: %d candidates without a finite bound; first: %s, lpdfs %.6g %.6g'
                                 % (name, li, int(miss.sum()), _where(ref, lay, float(x[k])), float(lb[k]),
                                    float(la[k])))
        assert want.sum() >= 0.9 * inside.sum() or name == 'offset1e6', (name, li, want.mean())
    return shares


@pytest.mark.parametrize('name', C.ELIGIBLE)
def test_bounds_hold_and_exist(eng, name):
    posts = _set(eng, name)
    shares = _bounds_hold_and_exist(eng, name, posts)
    for li in C.dense_labels(posts):   # the layout is the one bx_build's arithmetic gives
        lay, sh = eng.bx_layout(li), C.index_shape(posts[li])
        assert lay['nbins'] == sh['nbins'] and lay['n_nc'] == sh['n_nc'] and lay['tcut'] == C.T_TILE, (lay, sh)
        assert abs(lay['bw'] - sh['sub_width'] * K_SUB) <= 1e-9 * lay['bw']
    print('%s: finite share of the in-range candidates per label %s' % (name, ['%.4f' % s for s in shares]))


@pytest.mark.parametrize('name', ['uniform300', 'lognormal150', 'three_labels'])
@pytest.mark.parametrize('split,cut', [(1, 0), (3, 0), (8, 0), (0, 32), (0, 128)])
def test_bounds_hold_split_and_cut(eng, name, split, cut):
    """The split window of k_bx_table / k_bx_table_fin and a forced cut T.
    (A smaller T leaves fewer terms in a bin's window and list: at T = 32 the
    above sum has no lower bound where every term is below 2^-32 of the
    largest, e.g. lognormal150 at lpdf_above = -30, so finite bounds are
    required at the default cut only.)"""
    try:
        posts = _set(eng, name, bx_split=split, bx_t=cut)
        _bounds_hold_and_exist(eng, name, posts, exist=cut == 0)
        for li in C.dense_labels(posts):
            assert eng.bx_layout(li)['tcut'] == (cut if cut else C.T_TILE)
    finally:
        eng.set_option('bx_split', 0)
        eng.set_option('bx_t', 0)


@pytest.mark.parametrize('name', C.ELIGIBLE)
def test_width_and_mass(eng, name):
    """Per probed sub-bin, at its midpoint: the interval is not much wider
    than the score's oscillation over the sub-bin, and the mass is the
    exact interval mass of the truncated below mixture."""
    posts = _set(eng, name)
    for li in C.dense_labels(posts):
        p, ref = posts[li], _ref(name, li)
        lay = eng.bx_layout(li)
        bins = _probed_bins(lay)
        edges = _sub_edges(lay, bins)                      # [bins, 17], draw space
        mids = 0.5 * (edges[:, :-1] + edges[:, 1:])
        u, l, m = (a.reshape(mids.shape) for a in eng.hot_probe(li, ref.to_value(mids.ravel())))
        smin, smax = ref.score_range(edges[:, :-1].ravel(), edges[:, 1:].ravel())
        fin = (np.isfinite(u) & np.isfinite(l)).ravel() & np.isfinite(smin) & np.isfinite(smax)
        # (the bracket over the whole sub-bin, not just its midpoint)
        assert np.all(l.ravel()[fin].astype(LD) <= smin[fin]) and np.all(smax[fin] <= u.ravel()[fin].astype(LD))
        excess = (u - l).ravel()[fin] - (smax - smin)[fin].astype(np.float64)
        med = float(np.median(excess))
        interior = np.isfinite(u[:, 1:-1]) & np.isfinite(l[:, 1:-1])
        print('%s label %d: median (U - L) - osc = %.3g over %d of %d sub-bins; finite share %.4f '
              '(interior sub-bins %.4f)' % (name, li, med, int(fin.sum()), fin.size, fin.mean(),
                                           interior.mean()))
        assert fin.mean() > 0.8
        assert med <= 2.0 * WIDTH_MEDIAN[name], (name, li, med)
        # -- mass --
        sw = lay['bw'] / K_SUB
        wb, _, sb = (np.asarray(a, dtype=float) for a in p.below)
        assert sw <= np.min(sb[wb > 0]) / 100.0, (name, li)      # the midpoint rule's premise
        rows = range(0, len(bins), 4 if len(wb) > 64 else 1)     # (every 4th bin past 64 components: mpmath's time)
        worst, n = 0.0, 0
        for r in rows:
            exact = ref.interval_masses(edges[r])
            for k in np.where(exact >= 1e-6)[0]:
                ratio = abs(m[r, k] - exact[k]) / exact[k]
                worst, n = max(worst, ratio), n + 1
                assert ratio <= 1e-3, '%s label %d: mass %.9g, exact %.9g at bin %d sub-bin %d' % (
                    name, li, m[r, k], exact[k], bins[r], k)
        print('%s label %d: worst |mass - exact| / exact = %.3g over %d sub-bins' % (name, li, worst, n))
        assert n > 0
        # -- the label's masses sum to 1 (probes of 2^14 midpoints) --
        nsb = lay['nbins'] * K_SUB
        base = lay['centre'] + lay['xlo']
        total = 0.0
        for j0 in range(0, nsb, 1 << 14):
            j = np.arange(j0, min(nsb, j0 + (1 << 14)))
            total += float(eng.hot_probe(li, ref.to_value(base + (j + 0.5) * sw))[2].sum())
        tail = 0.0 if p.low is not None else len(wb) * C.K_RANGE_TAIL
        print('%s label %d: masses sum to %.9f' % (name, li, total))
        assert 1.0 - 1e-3 - tail <= total <= 1.0 + 1e-3, (name, li, total)


@pytest.mark.parametrize('name', C.ELIGIBLE)
def test_screen_score_within_its_bound(eng, name):
    """The median bound is ~1e-12 whatever the label's position: at
    offset1e6 (|centre| = 1e6) it was 3.33e-9 while the bound of a GMM1 label
    still carried the candidate's own magnitude (bx_score's mag).

    zero_weight certifies nothing, and is held to exactly that: a
    zero-weight below record (c = -inf) turns the one-pass below sum into
    NaN (tpe_device.h exp_scaled), which the fp64 round answers with its
    two-pass fallback and the screen by leaving the candidate uncertified.
    zero_above -- the same zero above weights, every below weight kept -- is
    held to the full bar: the screen reads tables and lists built over
    c = -inf records."""
    posts = _set(eng, name)
    for li in C.dense_labels(posts):
        p, ref = posts[li], _ref(name, li)
        lay = eng.bx_layout(li)
        x, _ = _candidates(eng, li, p, ref, lay)
        assert len(x) >= 2048
        sc, err = eng.screen_probe(li, x)
        s = ref.score_exact(x)
        ok = np.isfinite(err) & np.isfinite(s)
        gap = np.abs(sc[ok].astype(LD) - s[ok]).astype(np.float64)
        lim = err[ok] + 1e-13 * (1.0 + np.abs(s[ok].astype(np.float64)))
        bad = gap > lim
        if bad.any():
            k = int(np.where(ok)[0][np.where(bad)[0][0]])
            raise AssertionError('%s label %d: %d screen scores outside their bound; first: %s, score %.15g, '
                                 'exact %.15g, bound %.3g' % (name, li, int(bad.sum()),
                                                              _where(ref, lay, float(x[k])), sc[k], float(s[k]),
                                                              err[k]))
        if name == 'zero_weight':
            assert not np.isfinite(err).any() and np.isnan(sc).all(), (name, li, float(np.isfinite(err).mean()))
            continue
        print('%s label %d: certified %.4f, median bound %.3g, worst |s - exact| / bound %.3g' % (
            name, li, ok.mean(), np.median(err[ok]), float(np.max(gap / lim))))
        assert ok.mean() > 0.9, (name, li, ok.mean())
        assert np.median(err[ok]) < 1e-9


SETTINGS = [{}, {'hot': 0}, {'hot': 2}, {'expand': 0}, {'expand': 0, 'window': 0}, {'hot_div': 1 << 20}]
DEFAULTS = {'hot': 1, 'expand': 1, 'window': 1, 'hot_div': 16}


def _rounds_equal_fp64(eng, name, seed, rnd):
    """The round in every screen setting against the unscreened round;
    returns (the round, screen mode, last_hot, last_screen) of the default setting."""
    eng.set_option('screen', 0)
    ref_round = eng.suggest(seed, N_ROUND, round=rnd)
    assert eng.last_screen_mode() == 0
    eng.set_option('screen', 1)
    first = None
    for opts in SETTINGS:
        try:
            for k, v in opts.items():
                eng.set_option(k, v)
            res = eng.suggest(seed, N_ROUND, round=rnd)
            state = (res, eng.last_screen_mode(), eng.last_hot(), eng.last_screen())
        finally:
            for k in opts:
                eng.set_option(k, DEFAULTS[k])
        try:
            _assert_same(res, ref_round)
        except AssertionError as e:
            raise AssertionError('%s, options %r: field %s differs from the fp64 round' % (name, opts, e))
        first = first or state
    return first


@pytest.mark.parametrize('name', C.ELIGIBLE)
def test_round_is_the_fp64_round_and_the_exact_winner(eng, name):
    posts = _set(eng, name)
    seed, rnd = 1000 + len(name), 3
    res, mode, hot, (screened, rescored) = _rounds_equal_fp64(eng, name, seed, rnd)
    assert mode == 3
    print('%s: screened %d, listed %d (fallback %d), re-scored %d' % (name, screened, hot[0], hot[1], rescored))
    assert screened == N_ROUND * len(C.dense_labels(posts))
    if name == 'zero_weight':       # nothing certified: every candidate the prefilter lists is re-scored
        assert hot[1] == 0 and rescored == hot[0] > 0
    else:                           # the screen decides: near-ties only (test_screen.py's bar per label)
        assert 0 < rescored <= 64 * len(C.dense_labels(posts)), (name, rescored)
    if name in NO_PREFILTER:        # sampling records past kSampLds: no prefilter
        assert hot == (-1, 0)
    else:
        assert hot[0] >= 0
    # the winner among the round's own candidates, by the exact reference
    for li in C.dense_labels(posts):
        p, ref = posts[li], _ref(name, li)
        samp = eng.GMM1 if p.family == 'GMM1' else eng.LGMM1
        x = samp(*p.below, low=p.low, high=p.high, q=None, seed=seed, size=(N_ROUND,), stream=li, round=rnd)
        w = int(res[li]['index'])
        assert x[w] == res[li]['value']
        s = ref.score_exact(x)
        best = np.max(s[np.isfinite(s)])
        assert float(best - s[w]) <= 1e-9, (name, li, float(best), float(s[w]))
        assert abs(float(LD(res[li]['score']) - s[w])) <= 1e-9 * (1.0 + abs(float(s[w])))


@pytest.mark.parametrize('name', ['uniform300', 'lognormal150', 'three_labels'])
def test_packed_rounds_are_the_fp64_rounds(eng, name):
    """512 rounds of 24 candidates: the packed map's use of the index."""
    _set(eng, name)
    a = eng.suggest_batch(77, range(512), 24)
    mode = eng.last_screen_mode()
    eng.set_option('screen', 0)
    b = eng.suggest_batch(77, range(512), 24)
    eng.set_option('screen', 1)
    _assert_same(a, b)
    assert mode == 3


@pytest.mark.parametrize('name', C.INELIGIBLE)
def test_ineligible_posterior_has_no_index(eng, name):
    """Past kMaxBins, past kMaxUnclipped, or an above mixture out of mu
    order: no index, the windowed screen runs, the round is the fp64 round."""
    from hyperopt_amd.engine import EngineError
    posts = _set(eng, name)
    li = C.dense_labels(posts)[0]
    x = np.linspace(posts[li].low, posts[li].high, 2048)
    for call in (lambda: eng.hot_probe(li, x), lambda: eng.bx_layout(li)):
        with pytest.raises((EngineError, ValueError), match='no expansion index'):
            call()
    res, mode, hot, _ = _rounds_equal_fp64(eng, name, 77, 2)
    assert mode == 2 and hot == (-1, 0)
    # the probe of the screen takes the windowed screen too: its bound holds
    ref = _ref(name, li)
    sc, err = eng.screen_probe(li, x)
    s = ref.score_exact(x)
    ok = np.isfinite(err) & np.isfinite(s)
    assert ok.mean() > 0.5
    assert np.all(np.abs(sc[ok].astype(LD) - s[ok]) <= err[ok] + 1e-13 * (1.0 + np.abs(s[ok])))
    assert np.median(err[ok]) > 1e-9        # (an fp32 bound: not the expansion screen's)


def test_no_stale_index(eng):
    """The same posterior with one above mean moved by 0.3 of the range:
    the bounds bracket the new posterior's exact score, and the original's
    again when it returns."""
    from hyperopt_amd import posterior as P
    base = C.posts('uniform300')[0]
    wa, ma, sa = (np.array(a) for a in base.above)
    k = int(np.argmin(np.abs(ma + 2.0)))
    ma[k] += 3.0
    order = np.argsort(ma, kind='stable')     # (kept in mu order: only mu-ordered mixtures get an index)
    moved = P.LabelPosterior('moved', 'GMM1', base.below, (wa[order], ma[order], sa[order]),
                             low=base.low, high=base.high)
    x = np.linspace(base.low, base.high, 4097)
    for p in (base, moved, base):
        eng.set_posterior(*P.pack([p]))
        ref = LabelRef(p)
        lay = eng.bx_layout(0)
        u, l, _ = eng.hot_probe(0, x)
        _check_bracket(p.label, 0, ref, lay, x, u, l, ref.score_exact(x))
        assert np.isfinite(u).mean() > 0.9
