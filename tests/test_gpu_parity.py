"""GPU parity of the HIP engine against the reference's golden vectors and the
CPU oracle, through the C ABI.  Requires a real MI355X (`-m gpu`)."""
import numpy as np
import pytest

from oracle import tpe_oracle as O
from tests import golden_io
from tests.helpers import assert_lpdf_close, desc_from_case, is_quantized, stack_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


@pytest.fixture(scope='module')
def eng32():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f32')
    yield e
    e.close()


def _all_cases():
    for fx in ('labels_small.npz', 'labels_medium.npz'):
        for meta, rec in golden_io.cases(fx):
            yield fx, meta, rec


@pytest.mark.parametrize('fixture', ['labels_small.npz', 'labels_medium.npz'])
def test_score_matches_reference_golden(eng, fixture):
    """Identical candidate sets: both lpdf vectors within the fp64 bar and the
    broadcast_best winner bit-identical to the reference's."""
    for meta, rec in golden_io.cases(fixture):
        d, w, m, s = desc_from_case(meta, rec)
        eng.set_posterior(d, w, m, s)
        cand = rec['samples']
        lb, la, res = eng.score(0, cand)
        q = is_quantized(meta)
        assert_lpdf_close(lb, rec['lpdf_below'], quantized=q)
        assert_lpdf_close(la, rec['lpdf_above'], quantized=q)
        assert int(res['index']) == int(rec['best_idx']), (meta['kind'], meta['n_hist'])
        assert res['value'] == cand[int(rec['best_idx'])]


def test_quantized_absolute_branch_is_reference_cancellation(eng):
    """How many quantized lpdfs pass only through the absolute branch of the
    bar (|exp(got) - exp(ref)| <= 1e-13), and why: every such case is a
    probability the reference itself computes with cancellation -- its
    linear-space sum of CDF differences is below 1e-4, where the
    reference's own ~K ulp(1) rounding is already more than 1e-9 of it."""
    n_q = n_abs = 0
    worst = 0.0
    for fx in ('labels_small.npz', 'labels_medium.npz'):
        for meta, rec in golden_io.cases(fx):
            if not is_quantized(meta):
                continue
            d, w, m, s = desc_from_case(meta, rec)
            eng.set_posterior(d, w, m, s)
            lb, la, _ = eng.score(0, rec['samples'])
            for got, ref in ((lb, rec['lpdf_below']), (la, rec['lpdf_above'])):
                a = assert_lpdf_close(got, ref, quantized=True)
                n_q += a.size
                n_abs += int(a.sum())
                if a.any():
                    p_ref = np.exp(ref[a])
                    assert np.all(p_ref < 1e-4), p_ref.max()
                    worst = max(worst, float(np.max(np.abs(got[a] - ref[a]))))
    print('quantized lpdfs: %d checked, %d pass only through the absolute branch '
          '(all with reference probability < 1e-4; worst log difference %.3g)'
          % (n_q, n_abs, worst))
    assert n_abs <= 0.01 * n_q


def test_reference_op_entry_points(eng):
    """tpe_gmm1_lpdf / tpe_lgmm1_lpdf on the reference's edge inputs (far
    tails, quantized cancellation to -inf, x=0 for LGMM1 -> NaN)."""
    z, meta = golden_io.load('lpdf_edges.npz')
    w, mu, sg = (np.asarray(meta[k]) for k in ('w', 'mu', 'sigma'))
    for cid, call in enumerate(meta['calls']):
        x = z['e%03d/x' % cid]
        f = eng.GMM1_lpdf if call['fn'] == 'GMM1_lpdf' else eng.LGMM1_lpdf
        got = f(x, w, mu, sg, **call['kwargs'])
        assert_lpdf_close(got, z['e%03d/out' % cid], quantized='q' in call['kwargs'])


def test_broadcast_best_semantics(eng):
    z, meta = golden_io.load('lpdf_edges.npz')
    for i in range(meta['n_bb']):
        s = z['bb%02d/score' % i]
        samples = list(range(len(s)))
        got = eng.broadcast_best(samples, s, np.zeros_like(s))
        assert got == [int(z['bb%02d/best' % i])] * len(s)
    assert eng.broadcast_best([], [], []) == []
    with pytest.raises(ValueError):
        eng.broadcast_best([1, 2], [0.0], [0.0])


def test_categorical_lpdf(eng):
    p = np.array([0.1, 0.2, 0.7])
    s = np.array([0, 2, 1, 2])
    assert np.array_equal(eng.categorical_lpdf(s, p), np.log(p[s]))
    assert len(eng.categorical_lpdf(np.array([], dtype=int), p)) == 0


@pytest.mark.parametrize('C', [24, 700, 3000])
def test_fused_round_matches_oracle(eng, C):
    """Full round (in-kernel Philox sampling -> both lpdfs -> maxloc) over a
    multi-label posterior; the candidates are re-drawn through the sampler
    entry point with the same (seed, stream, round) and scored by the CPU
    oracle, whose argmax must equal the engine's."""
    from oracle import draw_oracle as D
    from tests import draw_cases
    from tests.draw_check import check_draws
    # (the labels with n_hist in (26, 300), variant 'plain'; seed 12345, round 7)
    pairs, seed, rnd, counts = draw_cases.fused_round_cases()
    assert C in counts and (seed, rnd) == (12345, 7) and len(pairs) == 20
    d, w, m, s = stack_cases(pairs)
    eng.set_posterior(d, w, m, s)
    res = eng.suggest(seed, C, round=rnd)
    for li, (meta, rec) in enumerate(pairs):
        kw = meta['lpdf_kwargs']
        if meta['sampler'] == 'categorical':
            cand = eng.categorical(rec['p_below'], seed=seed, size=(C,), stream=li, round=rnd)
            lb = O.categorical_lpdf(cand, rec['p_below'])
            la = O.categorical_lpdf(cand, rec['p_above'])
        else:
            samp = eng.GMM1 if meta['sampler'] == 'GMM1' else eng.LGMM1
            cand = samp(rec['w_b'], rec['mu_b'], rec['sigma_b'], seed=seed, size=(C,),
                        stream=li, round=rnd, **kw)
            f = O.gmm1_lpdf if meta['sampler'] == 'GMM1' else O.lgmm1_lpdf
            lb = f(cand, rec['w_b'], rec['mu_b'], rec['sigma_b'], **kw)
            la = f(cand, rec['w_a'], rec['mu_a'], rec['sigma_a'], **kw)
        # the re-drawn candidates are the draw reference's (not only the
        # engine's own): the chain round -> candidates -> oracle is not circular
        f = draw_cases.golden_fold(meta, rec)
        wp, wu = D.draw_words(seed, li, rnd, np.arange(C, dtype=np.uint64), categorical=f.categorical)
        check_draws(f, wp, wu, cand, 'fused round', '%s C %d' % (meta['kind'], C))
        best = O.broadcast_best_index(lb, la)
        assert int(res[li]['index']) == best, (li, meta['kind'])
        assert res[li]['value'] == cand[best]
        assert_lpdf_close([res[li]['lpdf_below']], [lb[best]], quantized=is_quantized(meta))


def test_splitk_equals_packed_map(eng, monkeypatch):
    """Small rounds (C = 24, the tpe.suggest default) run on the split-K map
    (component slices summed by separate waves); forcing the packed map
    (one workgroup walks every component) gives the same winners and lpdfs
    up to the summation order."""
    from hyperopt_amd.engine import Engine
    pairs = [(m, r) for fx, m, r in _all_cases()
             if m['variant'] in ('medium', 'plain') and m['n_hist'] in (26, 300, 2000)]
    d, w, m, s = stack_cases(pairs)
    eng.set_posterior(d, w, m, s)
    e2 = Engine(0, 'f64')
    try:
        e2.set_option('splitk', 0)
        e2.set_posterior(d, w, m, s)
        for C, rounds in ((24, [5]), (24, list(range(40))), (500, [1, 2, 3])):
            a = eng.suggest_batch(77, rounds, C)
            b = e2.suggest_batch(77, rounds, C)
            assert np.array_equal(a['index'], b['index']), C
            assert np.array_equal(a['value'], b['value']), C
            np.testing.assert_allclose(a['lpdf_below'], b['lpdf_below'], rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(a['lpdf_above'], b['lpdf_above'], rtol=1e-9, atol=1e-9)
    finally:
        e2.close()


def test_shard_invariance(eng):
    """Candidate i is the same draw whatever the sharding: splitting the set
    over 'GPUs' via cand_offset and merging gives the single-shard winner."""
    from hyperopt_amd.engine import merge_results
    pairs = [(m, r) for fx, m, r in _all_cases() if m['variant'] == 'medium'][:4]
    d, w, m, s = stack_cases(pairs)
    eng.set_posterior(d, w, m, s)
    C = 10000
    full = eng.suggest(99, C, round=3)
    parts = np.stack([eng.suggest(99, C // 4, round=3, cand_offset=k * (C // 4))
                      for k in range(4)])
    merged = merge_results(parts)
    assert np.array_equal(merged['index'], full['index'])
    assert np.array_equal(merged['value'], full['value'])
    assert np.array_equal(merged['score'], full['score'])


def test_batch_rounds_equal_single_rounds(eng):
    pairs = [(m, r) for fx, m, r in _all_cases() if m['variant'] == 'medium'][:3]
    d, w, m, s = stack_cases(pairs)
    eng.set_posterior(d, w, m, s)
    rounds = [5, 9, 11]
    batch = eng.suggest_batch(4, rounds, 2048)
    for j, r in enumerate(rounds):
        single = eng.suggest(4, 2048, round=r)
        assert np.array_equal(batch[j]['index'], single['index'])
        assert np.array_equal(batch[j]['value'], single['value'])


# -- sampler distributions: the reference's own statistical checks -----------
# (test_tpe.py:203-528: histogram of draws vs exp(lpdf); same thresholds)

def _hist_check(samples, lpdf_fn, per_bin, centers=False):
    samples = np.sort(samples)
    edges = samples[::per_bin]
    xs = .5 * edges[:-1] + .5 * edges[1:] if centers else edges[:-1]
    pdf = np.exp(lpdf_fn(xs))
    dx = edges[1:] - edges[:-1]
    y = 1 / dx / len(dx)
    err = (pdf - y) ** 2
    assert np.max(err) < .1 and np.mean(err) < .01 and np.median(err) < .01


W4, MU4, S4 = [.1, .3, .4, .2], [1.0, 2.0, 3.0, 4.0], [.1, .4, .8, 2.0]


@pytest.mark.parametrize('bounds', [{}, dict(low=2.5, high=3.5)])
def test_gmm1_sampler_distribution(eng, bounds):
    x = eng.GMM1(W4, MU4, S4, seed=234, size=(10001,), **bounds)
    if bounds:
        assert x.min() >= bounds['low'] and x.max() < bounds['high']
    _hist_check(x, lambda v: O.gmm1_lpdf(v, W4, MU4, S4, **bounds), 500)


@pytest.mark.parametrize('kw', [dict(q=1), dict(q=2), dict(q=0.5), dict(q=1, low=2, high=4),
                                dict(q=2, low=1, high=4.1)])
def test_qgmm1_sampler_distribution(eng, kw):
    n = 1001
    x = eng.GMM1(W4, MU4, S4, seed=234, size=(n,), **kw) / kw['q']
    assert np.all(x == x.astype(int))
    lo = int(x.min())
    counts = np.bincount(x.astype(int) - lo)
    xc = np.arange(lo, int(x.max()) + 1) * kw['q']
    prob = np.exp(O.gmm1_lpdf(xc, W4, MU4, S4, **kw))
    err = (prob - counts / float(n)) ** 2
    assert np.max(err) < .1 and np.mean(err) < .01 and np.median(err) < .01


@pytest.mark.parametrize('bounds', [{}, dict(low=2, high=4)])
def test_lgmm1_sampler_distribution(eng, bounds):
    # the reference's histogram check (test_tpe.py:371-434) at 16x its sample
    # size and 8x its bin size (the same ~100 bins): at 10001 draws / 200 per
    # bin its max-err bar sits at the sampling noise and the bin-centre bias
    # of the narrow first component, so it passes or fails by seed (numpy's
    # own exact sampler fails 40004 / 800 ~3 % of seeds, 160016 / 1600 none
    # of 40; the exact-CDF KS test below is the sharp check).
    mus = [-2.0, 1.0, 0.0, 3.0]
    x = eng.LGMM1(W4, mus, S4, seed=234, size=(160016,), **bounds)
    _hist_check(x, lambda v: O.lgmm1_lpdf(v, W4, mus, S4, **bounds), 1600, centers=True)


def _mix_cdf(w, mu, sg, low, high, log):
    from scipy.stats import norm
    w, mu, sg = (np.asarray(a, float) for a in (w, mu, sg))

    def F(x):
        y = np.log(x) if log else x
        c = (w * norm.cdf((y[:, None] - mu) / sg)).sum(1)
        if low is None:
            return c
        c0 = (w * norm.cdf((low - mu) / sg)).sum()
        c1 = (w * norm.cdf((high - mu) / sg)).sum()
        return (c - c0) / (c1 - c0)
    return F


@pytest.mark.parametrize('log', [False, True])
@pytest.mark.parametrize('bounds', [(None, None), (2.5, 3.5), (-1.0, 0.5)])
def test_sampler_ks(eng, log, bounds):
    """Kolmogorov-Smirnov test of the truncated-mixture samplers against the
    exact mixture CDF (the distribution the reference's rejection loop
    produces, tpe.py:88-93 / 246-250)."""
    from scipy.stats import kstest
    low, high = bounds
    mus = [-2.0, 1.0, 0.0, 3.0] if log else MU4
    f = eng.LGMM1 if log else eng.GMM1
    x = f(W4, mus, S4, low=low, high=high, seed=99, size=(50000,))
    if low is not None:
        y = np.log(x) if log else x
        assert y.min() >= low and y.max() < high
    assert kstest(x, _mix_cdf(W4, mus, S4, low, high, log)).pvalue > 1e-4


# The inverse-CDF draw (tpe_device.h icdf_draw) takes v = (wu + r) 2^-32
# with wu one 32-bit Philox word and r = (wp - tlo + 1/2) / (thi - tlo) the
# pick word's position in its component's interval: a one-component normal
# reaches v = 2^-65 at the least, so every draw has |z| <= -Phi^-1(2^-65)
# = 9.1553 (the reference's MT19937 normals reach ~8.3 sigma in practice).
# The bound is per mixture: a component that holds n_k of the 2^32 pick
# words has v >= 2^-33 / n_k, so its cap is -Phi^-1(2^-33 / n_k) (9.155 only
# for n_k = 2^32; 6.55 for n_k = 4), the tail mass cut off is 2^-64 per
# component (K 2^-64 per draw of a K-component mixture), and the pick itself
# is within total variation K 2^-33 of w_k m_k / sum w m
# (test_oracle.py test_normal_draw_cap_mass; test_draw_oracle.py).
Z_CAP = 9.155293772686072


def test_normal_draw_cap(eng):
    """Every draw within the cap (a bound, not a tendency), and the tail up to
    it present: the count beyond 4.5 sigma is N(0, 1)'s (Poisson, 5 sd)."""
    n = 1 << 22
    x = eng.GMM1([1.0], [0.0], [1.0], seed=7, size=(n,))
    assert np.abs(x).max() <= Z_CAP * (1 + 1e-12)
    lam = n * 2 * 3.3976731247300535e-06           # 2 sf(4.5)
    k = int(np.count_nonzero(np.abs(x) > 4.5))
    assert abs(k - lam) < 5 * np.sqrt(lam)


def test_categorical_sampler_distribution(eng):
    p = np.array([0.1, 0.2, 0.3, 0.4])
    x = eng.categorical(p, seed=5, size=(200000,))
    freq = np.bincount(x, minlength=4) / len(x)
    assert np.max(np.abs(freq - p)) < 0.005


def test_sampler_errors(eng):
    with pytest.raises(ValueError):
        eng.GMM1([1.0], [0.0], [1.0], low=2.0, high=1.0, seed=0, size=(4,))
    with pytest.raises(TypeError):
        eng.GMM1_lpdf([1.0], [[1.0]], [0.0], [1.0])


# -- fp32 fast path: 1e-4 relative on the dense lpdfs, argmax agreement -------

def test_fp32_dense_path(eng32):
    agree = total = 0
    for fx, meta, rec in _all_cases():
        if is_quantized(meta) or meta['sampler'] == 'categorical' or meta['n_hist'] < 26:
            continue
        d, w, m, s = desc_from_case(meta, rec)
        eng32.set_posterior(d, w, m, s)
        lb, la, res = eng32.score(0, rec['samples'])
        assert_lpdf_close(lb, rec['lpdf_below'], rtol=1e-4, atol=1e-4)
        assert_lpdf_close(la, rec['lpdf_above'], rtol=1e-4, atol=1e-4)
        total += 1
        agree += int(res['index']) == int(rec['best_idx'])
    assert total > 0 and agree >= 0.8 * total


def test_quantized_dedup_equals_direct(eng, monkeypatch):
    """The grid-value table path (sampled rounds) picks the same winners as
    per-candidate evaluation (set_option('dedup', 0)), on quantized labels of all
    four quantized kinds."""
    from hyperopt_amd.engine import Engine
    pairs = [(m, r) for fx, m, r in _all_cases()
             if is_quantized(m) and m['n_hist'] in (26, 300)]
    assert len(pairs) >= 8
    d, w, m, s = stack_cases(pairs)
    eng.set_posterior(d, w, m, s)
    fast = eng.suggest(31, 20000, round=2)
    stats = eng.last_mode_stats()
    slow_eng = Engine(0, 'f64')
    slow_eng.set_option('dedup', 0)
    slow_eng.set_posterior(d, w, m, s)
    slow = slow_eng.suggest(31, 20000, round=2)
    slow_stats = slow_eng.last_mode_stats()
    slow_eng.close()
    assert np.array_equal(fast['index'], slow['index'])
    assert np.array_equal(fast['value'], slow['value'])
    np.testing.assert_allclose(fast['score'], slow['score'], rtol=1e-11, atol=1e-12)
    # executed work is reported, not skipped work
    q_fast = stats['quant_gmm1'][1] + stats['quant_lgmm1'][1]
    q_slow = slow_stats['quant_gmm1'][1] + slow_stats['quant_lgmm1'][1]
    assert q_fast < q_slow
    # batched small rounds share one table per label across the rounds
    rounds = list(range(500, 2500))
    fast_b = eng.suggest_batch(31, rounds, 24)
    sb = eng.last_mode_stats()
    slow_eng = Engine(0, 'f64')
    slow_eng.set_option('dedup', 0)
    slow_eng.set_posterior(d, w, m, s)
    slow_b = slow_eng.suggest_batch(31, rounds, 24)
    slow_eng.close()
    assert np.array_equal(fast_b['index'], slow_b['index'])
    assert np.array_equal(fast_b['value'], slow_b['value'])
    assert sb['quant_gmm1'][1] + sb['quant_lgmm1'][1] < q_slow


def _oracle_winner(eng, meta, rec, li, C, seed, rnd):
    kw = meta['lpdf_kwargs']
    if meta['sampler'] == 'categorical':
        cand = eng.categorical(rec['p_below'], seed=seed, size=(C,), stream=li, round=rnd)
        lb = O.categorical_lpdf(cand, rec['p_below'])
        la = O.categorical_lpdf(cand, rec['p_above'])
    else:
        samp = eng.GMM1 if meta['sampler'] == 'GMM1' else eng.LGMM1
        cand = samp(rec['w_b'], rec['mu_b'], rec['sigma_b'], seed=seed, size=(C,),
                    stream=li, round=rnd, **kw)
        f = O.gmm1_lpdf if meta['sampler'] == 'GMM1' else O.lgmm1_lpdf
        lb = f(cand, rec['w_b'], rec['mu_b'], rec['sigma_b'], **kw)
        la = f(cand, rec['w_a'], rec['mu_a'], rec['sigma_a'], **kw)
    best = O.broadcast_best_index(lb, la)
    return best, cand[best]


@pytest.mark.parametrize('C', [1, 2, 24, 33, 64, 65, 256, 257, 700, 1023, 1024])
def test_batched_small_candidate_sets(eng, C):
    """Batched rounds with candidate sets smaller than a tile use the packed
    slot map (whole rounds per workgroup, per-round maxloc through LDS; one
    candidate per thread up to 256, four above); every round's winner must
    equal the oracle's on the same draws, for dense, quantized and
    categorical labels."""
    pairs = [(m, r) for fx, m, r in _all_cases()
             if m['n_hist'] == 300 and m['variant'] == 'plain']
    d, w, m, s = stack_cases(pairs)
    eng.set_posterior(d, w, m, s)
    rounds = [3, 8, 100, 7, 7 + 2 ** 20]
    seed = 2024
    batch = eng.suggest_batch(seed, rounds, C)
    for j, rnd in enumerate(rounds):
        for li, (meta, rec) in enumerate(pairs):
            best, val = _oracle_winner(eng, meta, rec, li, C, seed, rnd)
            assert int(batch[j][li]['index']) == best, (C, rnd, meta['kind'])
            assert batch[j][li]['value'] == val


def test_single_ops_leave_resident_posterior(eng):
    """GMM1_lpdf / samplers between rounds do not disturb the uploaded
    posterior (they run on the context's one-label slot)."""
    pairs = [(m, r) for fx, m, r in _all_cases() if m['variant'] == 'medium'][:4]
    d, w, m, s = stack_cases(pairs)
    eng.set_posterior(d, w, m, s)
    before = eng.suggest(5, 4096, round=1)
    eng.GMM1_lpdf(np.array([0.1, 0.2]), [0.5, 0.5], [0.0, 1.0], [1.0, 1.0])
    eng.GMM1([1.0], [0.0], [1.0], seed=1, size=(16,))
    eng.categorical(np.array([0.3, 0.7]), seed=2, size=(8,))
    after = eng.suggest(5, 4096, round=1)
    assert np.array_equal(before, after)


def _chunk_engine(monkeypatch, prec, chunks, hist):
    from hyperopt_amd.engine import Engine
    e = Engine(0, prec)
    e.set_option('chunks', 0 if chunks is None else chunks)
    e.build_posterior(*hist.device_inputs(), gamma=0.25, prior_weight=1.0)
    return e


@pytest.mark.parametrize('prec,C,n_rounds', [('f64', 24, 300), ('f32', 24, 300), ('f64', 700, 12)])
def test_chunked_packed_map(monkeypatch, prec, C, n_rounds):
    """Batched small rounds over long above mixtures (the config-5 shape,
    scaled down): the packed map cuts each above mixture into chunks along
    grid.z (k_round_chunk) and adds them in order (k_finish_chunks).  Forced
    chunk counts, the automatic choice and the unchunked map give the same
    winners and lpdfs up to the summation order; the f64 winners equal the
    oracle's argmax on the re-drawn candidates."""
    from hyperopt_amd.workloads import mixed_history
    hist = mixed_history(10, 6000, seed=5)
    # C = 24: 7200 slots per label, the narrow packed map (2 slots per
    # thread), not split-K; C = 700: one round per workgroup, 4 slots per thread
    rounds = list(range(n_rounds))
    seed = 4242
    res = {}
    for ch in (1, 3, 7, None):
        e = _chunk_engine(monkeypatch, prec, ch, hist)
        try:
            res[ch] = e.suggest_batch(seed, rounds, C)
            if ch is None and prec == 'f64':
                mix = {li: e.get_mixture(li, 0) for li in range(len(hist.labels))}
                a_mix = {li: e.get_mixture(li, 1) for li in range(len(hist.labels))}
                draws = {}
                for li, (name, kind, args) in enumerate(hist.labels):
                    if kind not in ('uniform', 'loguniform', 'normal'):
                        continue
                    samp = e.LGMM1 if kind == 'loguniform' else e.GMM1
                    for rnd in (0, n_rounds // 2, n_rounds - 1):
                        draws[li, rnd] = samp(*mix[li], low=args.get('low'), high=args.get('high'),
                                              seed=seed, size=(C,), stream=li, round=rnd)
        finally:
            e.close()
    base = res[1]
    tol = 1e-12 if prec == 'f64' else 2e-5
    for ch in (3, 7, None):
        r = res[ch]
        same = r['index'] == base['index']
        if prec == 'f64':
            assert same.all(), ch
        else:                            # fp32 sums in another order may flip near-ties
            assert same.mean() > 0.99, (ch, same.mean())
        for f in ('lpdf_below', 'lpdf_above'):
            np.testing.assert_allclose(r[f][same], base[f][same], rtol=tol, atol=tol)
    if prec != 'f64':
        return
    r = res[None]
    for (li, rnd), cand in draws.items():
        name, kind, args = hist.labels[li]
        f = O.lgmm1_lpdf if kind == 'loguniform' else O.gmm1_lpdf
        kw = dict(low=args.get('low'), high=args.get('high'))
        lb = f(cand, *mix[li], **kw)
        la = f(cand, *a_mix[li], **kw)
        best = O.broadcast_best_index(lb, la)
        assert int(r[rnd, li]['index']) == best, (name, rnd)
        assert r[rnd, li]['value'] == cand[best]
        np.testing.assert_allclose(r[rnd, li]['lpdf_above'], la[best], rtol=1e-9, atol=1e-9)


def test_quantized_tables_over_runs_match_oracle(eng):
    """The quantized tables sum the above mixture's runs of equal (mu,
    sigma) (k_qcompress): at 20k trials a quniform(0, 100, q=1) label's above
    mixture holds ~15k records on 101 values.  The round's quantized winners
    (fused table path, 2^13 candidates) are the oracle's argmax over the
    same re-drawn candidates and their lpdfs the oracle's within the
    quantized bar (tpe.py:110-172 at the reference's term-by-term sum)."""
    from hyperopt_amd import posterior as P
    from hyperopt_amd.workloads import mixed_history
    hist = mixed_history(10, 20000, seed=5)
    posts = hist.posteriors()
    eng.set_posterior(*P.pack(posts))
    C, seed, rnd = 1 << 13, 21, 4
    res = eng.suggest(seed, C, round=rnd)
    checked = 0
    for li, post in enumerate(posts):
        if post.q is None or post.family != 'GMM1':
            continue
        kw = dict(low=post.low, high=post.high, q=post.q)
        wb, mb, sb = post.below
        wa, ma, sa = post.above
        cand = eng.GMM1(wb, mb, sb, seed=seed, size=(C,), stream=li, round=rnd, **kw)
        vals, inv = np.unique(cand, return_inverse=True)      # (<= 101 grid values: the oracle on those)
        lb = O.gmm1_lpdf(vals, wb, mb, sb, **kw)[inv]
        la = O.gmm1_lpdf(vals, wa, ma, sa, **kw)[inv]
        best = O.broadcast_best_index(lb, la)
        assert res[li]['value'] == cand[best], li
        assert_lpdf_close([res[li]['lpdf_below']], [lb[best]], quantized=True)
        assert_lpdf_close([res[li]['lpdf_above']], [la[best]], quantized=True)
        assert len(np.unique(ma)) < len(ma) / 50          # (heavy ties: the runs are long)
        checked += 1
    assert checked == 2
