"""The draw reference against the mathematics (CPU only).

oracle/draw_oracle.py restates the sampler's draw contract twice: in numpy
fp64 in the device's operation order (the port, which the GPU tests compare
every device draw with) and in 140-digit mpmath (the exact draw).  Here the
port is held to the exact draw on every listed mixture -- random words plus
the words at both sides of every pick threshold and at both ends of the
uniform word -- and the two resolution bounds of the draw are checked:

* the pick: thr = ceil(cdf 2^32), so a K-component mixture's pick
  probabilities are within total variation K 2^-33 of w_k m_k / Z (a
  component of relative mass below 2^-32 is picked with probability 2^-32 or
  never);
* the tail: a component whose threshold interval holds n_k words draws
  |z| <= -Phi^-1(2^-33 / n_k) on an unbounded label -- 9.155 for one
  component, 6.55 for n_k = 4.
"""
import zlib

import numpy as np
import pytest

from oracle import draw_oracle as D
from tests import draw_cases as C
from tests.test_device_math import _philox

# The port's worst error against the exact draw over the mixtures of
# draw_cases.MIXTURES, in |z - z_exact| / max(1, |z|): measured 6.50e-16 (the
# AS241 approximation's own error) when this test was written; the
# constant is twice that.  The device comparisons use 4 T_PORT.
T_PORT_MEASURED = 6.50e-16
T_PORT = 2 * T_PORT_MEASURED
EPS51 = 2.0 ** -51
N_RANDOM = 1500


def x_tolerance(f, k, z, x, T):
    """The two-term bound on a draw-space x: T sigma_k max(1, |z|) from the
    quantile, 2^-51 (|mu_k| + |x|) from forming mu + sigma z."""
    return T * f.sigma[k] * np.maximum(1.0, np.abs(z)) + EPS51 * (np.abs(f.mu[k]) + np.abs(x))


def forced_words(f, rng):
    """Random word pairs, then every threshold's two neighbours crossed with
    the four extreme uniform words."""
    wp = [rng.randint(0, 1 << 32, N_RANDOM, dtype=np.uint64)]
    wu = [rng.randint(0, 1 << 32, N_RANDOM, dtype=np.uint64)]
    ends = np.array([0, 1, (1 << 32) - 2, (1 << 32) - 1], dtype=np.uint64)
    edge = set()
    for t in f.thr.tolist():
        edge.update(v for v in (t - 1, t) if 0 <= v < (1 << 32))
    edge.update((0, (1 << 32) - 1))
    edge = np.array(sorted(edge), dtype=np.uint64)
    wp.append(np.repeat(edge, len(ends)))
    wu.append(np.tile(ends, len(edge)))
    return np.concatenate(wp), np.concatenate(wu)


@pytest.fixture(scope='module')
def drawn():
    """Per mixture: the fold, the words, the port's draw and the exact one
    (computed once, shared by the tests below)."""
    out = {}
    for name in sorted(C.MIXTURES):
        f = C.fold_of(name)
        wp, wu = forced_words(f, np.random.RandomState(zlib.crc32(name.encode())))
        k, z, x, val = D.draw_fp64(f, wp, wu)
        ze, xe = D.draw_exact(f, k, wp, wu)
        out[name] = (f, wp, wu, k, z, x, val, ze, xe)
    return out


@pytest.mark.parametrize('name', sorted(C.MIXTURES))
def test_port_matches_exact_draw(drawn, name):
    f, wp, wu, k, z, x, val, ze, xe = drawn[name]
    assert np.all(f.width(k) > 0)
    ez = np.abs(z - ze) / np.maximum(1.0, np.abs(ze))
    print('%s: K %d, %d draws, max |z| %.3f, worst z error %.3g' % (name, f.K, len(k), np.abs(ze).max(),
                                                                   ez.max()))
    assert ez.max() <= T_PORT
    if f.bounded:      # the exact draw lies inside the bounds; the port's clamp moves an end's rounding only
        assert np.all((xe >= f.low) & (xe <= f.high))
        assert np.all((x >= f.low) & (x < f.high))
    assert np.all(np.abs(x - xe) <= x_tolerance(f, k, ze, xe, T_PORT))
    ve = D.exact_value(f, xe)
    if f.q is not None:
        far = ~D.near_rounding(f, xe)      # (not at a rounding boundary of x / q)
        assert np.array_equal(val[far], ve[far])
    elif f.log:
        rel = x_tolerance(f, k, ze, xe, T_PORT) + EPS51 * (1.0 + np.abs(xe))
        assert np.all(np.abs(val - ve) <= rel * ve)
    else:
        assert np.array_equal(val, x)


def test_measured_t_port(drawn):
    """T_PORT is twice the worst case over the listed mixtures (a change of
    the port or of the mixtures that moves it shows here)."""
    worst = max(float(np.max(np.abs(z - ze) / np.maximum(1.0, np.abs(ze))))
                for f, wp, wu, k, z, x, val, ze, xe in drawn.values())
    print('worst port error %.4g' % worst)
    assert worst <= T_PORT
    assert worst >= 0.25 * T_PORT_MEASURED      # (the comment's figure is of this order)


@pytest.mark.parametrize('name', sorted(C.MIXTURES))
def test_pick_resolution(name):
    """1/2 sum_k |n_k / 2^32 - w_k m_k / Z| <= K 2^-33 with the exact masses."""
    import mpmath as mp
    f = C.fold_of(name)
    with mp.workdps(D.DPS):
        mass = [f.w[k] * (b - a) for k, (a, b) in enumerate(D.exact_masses(f))]
        Z = mp.fsum(mass)
        n = np.diff(np.concatenate([[0], f.thr.astype(np.int64)]))
        tv = mp.fsum(abs(mp.mpf(int(n[k])) / 2 ** 32 - mass[k] / Z) for k in range(f.K)) / 2
        assert tv <= f.K * mp.mpf(2) ** -33, (name, float(tv))
    assert int(n.sum()) == 1 << 32 and np.all(n >= 0)


def test_pick_resolution_zero_width():
    """W4 / MU4 / S4 in [9, 12): the thresholds are [0, 1, 1, 2^32] -- the
    component of relative mass 1.7e-66 takes one word (probability 2^-32),
    the one of relative mass 1.0e-11 none."""
    import mpmath as mp
    f = C.fold_of('w4_9_12')
    assert f.thr.tolist() == [0, 1, 1, 1 << 32]
    with mp.workdps(D.DPS):
        mass = [f.w[k] * (b - a) for k, (a, b) in enumerate(D.exact_masses(f))]
        rel = [float(m / mp.fsum(mass)) for m in mass]
    assert rel[0] < 1e-300 and 1.7e-66 < rel[1] < 1.8e-66 and 1.0e-11 < rel[2] < 1.1e-11 and rel[3] > 1 - 1e-10
    assert D.pick(f, np.array([0, 1, 2], dtype=np.uint64)).tolist() == [1, 3, 3]


@pytest.mark.parametrize('name', ['one', 'w4', 'tiny_w', 'k200', 'cell6'])
def test_tail_cap_per_component(drawn, name):
    """Unbounded labels: |z| <= -Phi^-1(2^-33 / n_k), reached at the extreme
    words (wu = 0 at the interval's first word, wu = 2^32 - 1 at its last)."""
    import mpmath as mp
    f, wp, wu, k, z, x, val, ze, xe = drawn[name]
    assert not f.bounded
    n = f.width(k).astype(np.int64)
    with mp.workdps(D.DPS):
        cap = {int(v): float(-D.ndtri_exact(mp.mpf(2) ** -33 / int(v))) for v in np.unique(n)}
    capk = np.array([cap[int(v)] for v in n])
    assert np.all(np.abs(ze) <= capk * (1 + 1e-15))
    assert np.all(np.abs(z) <= capk * (1 + T_PORT))
    ext = ((wu == 0) & (wp == f.tlo(k))) | ((wu == D.M32) & (wp == f.thr[k] - np.uint64(1)))
    assert ext.any() and np.allclose(np.abs(ze[ext]), capk[ext], rtol=1e-14, atol=0)
    if name == 'one':
        assert abs(cap[1 << 32] - 9.155293772686072) < 1e-12
    if name == 'tiny_w':
        from scipy.special import ndtri
        assert cap[4] == pytest.approx(-ndtri(2.0 ** -35), rel=1e-9) and 6.5 < cap[4] < 6.6


def test_vectorised_philox():
    """The Random123 known answers, the scalar restatement of
    test_device_math, and seeds >= 2^32 (key word k1 != 0)."""
    for c, key, out in (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                        ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                        ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
                         [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        assert [int(v) for v in D.philox4x32_10(c, key)] == out
    rng = np.random.RandomState(3)
    g = np.concatenate([np.arange(9), [(1 << 32) - 2, (1 << 32) - 1],
                        rng.randint(0, 1 << 32, 40, dtype=np.uint64)]).astype(np.uint64)
    for seed in (234, 1 << 32, 0x9e3779b97f4a7c15, (1 << 64) - 1):
        for stream, rnd in ((0, 0), (7, 0xfffffffe)):
            wp, wu = D.draw_words(seed, stream, rnd, g)
            cp, _ = D.draw_words(seed, stream, rnd, g, categorical=True)
            for i, gi in enumerate(g.tolist()):
                r = _philox([gi >> 1, 0, stream, rnd], [seed & D.M32, seed >> 32])
                assert (int(wp[i]), int(wu[i])) == ((r[2], r[3]) if gi & 1 else (r[0], r[1]))
                assert int(cp[i]) == _philox([gi, 0, stream, rnd], [seed & D.M32, seed >> 32])[0]
    a = D.draw_words(234, 0, 0, g)
    b = D.draw_words(234 + (1 << 32), 0, 0, g)
    assert not np.array_equal(a[0], b[0])


def test_categorical_pick():
    """A categorical draw is the pick alone: index = the first k with
    thr[k] > word, thr from the cumulative p."""
    for p in (C.P3, C.P70):
        f = D.fold(p)
        assert f.categorical and int(f.thr[-1]) == 1 << 32
        w = np.concatenate([f.thr[:-1] - np.uint64(1), f.thr[:-1], [0, D.M32]]).astype(np.uint64)
        k = D.draw_fp64(f, w, w)[0]
        ref = [next(j for j in range(f.K) if int(f.thr[j]) > int(v)) for v in w]
        assert k.tolist() == ref
        n = np.diff(np.concatenate([[0], f.thr.astype(np.int64)]))
        assert 0.5 * np.abs(n / 2.0 ** 32 - p).sum() <= f.K * 2.0 ** -33


def _none_excluded(f, wp, wu):
    x = D.draw_fp64(f, wp, wu)[2]
    return not D.excluded(f, wp, wu, x).any()


def test_committed_words_exclude_no_draw():
    """The device tests (test_gpu_draws.py) may leave a draw out of the
    comparison where its words sit on a pick threshold, at an end of the
    uniform word or on a quantized value's rounding boundary; with the seeds,
    offsets and sizes committed in draw_cases no draw is (a seed that does
    is changed, the cap stays zero)."""
    for name in C.ENTRY_NAMES:
        f = C.entry_fold(name)
        for offset, stream, rnd, seed in C.CORNERS:
            g = offset + np.arange(C.N_ENTRY, dtype=np.uint64)
            assert int(g[-1]) == offset + C.N_ENTRY - 1 < (1 << 32) - 1
            assert _none_excluded(f, *D.draw_words(seed, stream, rnd, g, categorical=f.categorical)), name
    rounds = np.asarray(C.ROUND_IDS, dtype=np.uint64)[None, :]
    g = np.concatenate([np.arange(64 + 3), (1 << 32) - 1 - np.arange(1, 5)]).astype(np.uint64)[:, None]
    assert set(C.ROUND_G) <= set(g.ravel().tolist())
    for li, p in enumerate(C.round_posterior()):
        f = C.fold_posterior(p)
        for seed in C.ROUND_SEEDS:
            wp, wu = D.draw_words(seed, li, rounds, g, categorical=f.categorical)
            assert _none_excluded(f, wp.ravel(), wu.ravel()), p.label
    for li, p in enumerate(C.tile_posteriors()):
        f = C.fold_posterior(p)
        for n, seed, rnd in C.TILE_ROUNDS:
            wp, wu = D.draw_words(seed, li, rnd, np.arange(n, dtype=np.uint64), categorical=f.categorical)
            assert _none_excluded(f, wp, wu), (p.label, n)
    rounds = np.asarray(C.FUSED_IDS, dtype=np.uint64)[None, :]
    g = np.asarray(C.FUSED_G, dtype=np.uint64)[:, None]
    for li, p in enumerate(C.round_posterior(C.FUSED_LABELS)):
        if p.q is not None:
            f = C.fold_posterior(p)
            wp, wu = D.draw_words(C.ROUND_SEEDS[0], li, rounds, g)
            assert _none_excluded(f, wp.ravel(), wu.ravel()), p.label
    pairs, seed, rnd, counts = C.fused_round_cases()
    for li, (meta, rec) in enumerate(pairs):
        f = C.golden_fold(meta, rec)
        wp, wu = D.draw_words(seed, li, rnd, np.arange(max(counts), dtype=np.uint64), categorical=f.categorical)
        assert _none_excluded(f, wp, wu), (li, meta['kind'])


def _guide_steps(f):
    """stage_samp's `steps` of a staged mixture: the most cumulative weights
    strictly inside one of the 256 guide cells (a cell's first k is the
    count of cdf <= j / 256, its last the count of cdf < (j + 1) / 256)."""
    c = f.cdf[:-1]
    j = np.arange(256)
    k0 = (c[None, :] <= (j / 256.0)[:, None]).sum(1)
    k1 = (c[None, :] < ((j + 1) / 256.0)[:, None]).sum(1)
    return int(np.max(k1 - k0))


def test_device_cases_cover_the_paths():
    """What the small rounds' labels hold between them, and which pick each
    quantized one takes in the packed maps' quantized kernels (the only
    small-round kernels that stage the pick in LDS): guided up to
    kGuideSteps = 3 comparisons, branch-free beyond, no staging beyond
    kSampLds = 64 components.  The dense and categorical labels (cell6, k65,
    p70 among them) are drawn there by the binary search on the fp64 cdf,
    whatever their shape."""
    folds = {p.label: C.fold_posterior(p) for p in C.round_posterior()}
    assert folds['one'].K == 1 and folds['k26'].K == 26 and folds['k65'].K == 65
    assert _guide_steps(folds['cell6']) == 6
    assert folds['w4_2.5_3.5'].flip.tolist() == [True, True, False, False] and folds['w4_9_12'].flip.all()
    assert folds['k65'].flip[:2].all() and not folds['k65'].flip[2:].any()
    assert folds['w4_q'].q == 0.5 and not folds['w4_q'].log
    assert folds['w4_2.5_3.5_logq'].q == 0.5 and folds['w4_2.5_3.5_logq'].log
    assert folds['p3'].K == 3 and folds['p70'].K == 70
    for name, K, steps in (('w4_q', 4, 1), ('k64_q', 64, 1), ('cell6_q', 64, 6), ('k65_q', 65, None)):
        f = folds[name]
        assert f.q is not None and not f.bounded and f.K == K
        if steps is not None:
            assert _guide_steps(f) == steps, (name, _guide_steps(f))
    assert _guide_steps(folds['k64_q']) <= 3 < _guide_steps(folds['cell6_q']) and folds['k65_q'].K > 64
    # a neighbouring pick changes the quantized value: the components lie 2 apart, 6.7 sigma, q = 0.5
    for name in ('k64_q', 'cell6_q', 'k65_q'):
        f = folds[name]
        assert np.all(np.diff(f.mu) >= 2.0) and np.all(f.sigma == 0.3) and f.q == 0.5


def test_threshold_words_are_threshold_words():
    """draw_cases.THRESHOLD_WORDS: each listed candidate's pick word is
    thr[k] - 1 or thr[k] of its label, both sides occur, and the pick on
    either side is the one the definition gives."""
    sides = set()
    for li, p in enumerate(C.round_posterior()):
        if p.label not in C.THRESHOLD_WORDS:
            continue
        f = C.fold_posterior(p)
        assert not f.bounded
        g = np.asarray(C.THRESHOLD_WORDS[p.label], dtype=np.uint64)
        wp, _ = D.draw_words(C.ROUND_SEEDS[0], li, 0, g, categorical=f.categorical)
        thr = f.thr[:-1].astype(np.int64)
        for v, k in zip(wp.astype(np.int64).tolist(), D.pick(f, wp).tolist()):
            assert v in thr or v + 1 in thr, (p.label, v)
            at = v in thr                        # (at a threshold: the next component's first word)
            sides.add((p.label, at))
            assert (int(f.thr[k - 1]) == v) if at else (int(f.thr[k]) == v + 1)
    assert {(name, at) for name in ('k64', 'k64_q', 'cell6_q', 'k65_q', 'p70') for at in (True, False)} <= sides
    assert set(C.THRESHOLD_WORDS) <= set(C.ROUND_LABELS)


def test_fused_posterior_keeps_streams_and_thresholds():
    """draw_cases.FUSED_LABELS: every quantized label bounded (what the
    packed map's fused quantized kernel needs), each at its ROUND_LABELS
    place, and the three wide ones with the unbounded labels' thresholds
    exactly, so THRESHOLD_WORDS holds for them too."""
    a, b = C.round_posterior(), C.round_posterior(C.FUSED_LABELS)
    assert len(a) == len(b)
    grid = 0
    for pa, pb in zip(a, b):
        assert (pa.family, pa.q is None) == (pb.family, pb.q is None)
        if pb.q is None:
            assert pa.label == pb.label
            continue
        assert pb.low is not None and pb.high is not None
        lo, hi = (np.exp(pb.low), np.exp(pb.high)) if pb.family == 'LGMM1' else (pb.low, pb.high)
        grid = max(grid, int(np.ceil(hi / pb.q) + 1) - int(np.floor(lo / pb.q) - 1) + 1)
        if pb.label.endswith('_qb'):
            fa, fb = C.fold_posterior(pa), C.fold_posterior(pb)
            assert pa.label + 'b' == pb.label and pa.label in C.THRESHOLD_WORDS
            assert np.array_equal(fa.thr, fb.thr) and np.all(fb.m == 1.0) and not fb.flip.any()
    assert 2 * grid <= len(C.FUSED_IDS)
