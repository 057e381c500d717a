"""The split build on the device (tpe_build_split_resident, Engine.build_split)
against posterior.label_posterior on the host in fp64: weights, mus, sigmas
and component counts of both sides of every label, np.array_equal."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from hyperopt_amd import posterior as P
from hyperopt_amd.workloads import prior_draw

pytestmark = pytest.mark.gpu

T = L.TPE_SPLIT_TILE
PW, LF = 1.0, P.DEFAULT_LF
# (below, above) sizes of the labels active in every trial: each side runs over
# 0, 1, 2, the ramp's start (25, 26), the old 64-entry row and the wave (63,
# 64, 65) and the tile's edges (T - 1, T, T + 1, 2 T + 1); (80, 120) is the
# tied quniform label's case
SIZES = [(0, 2 * T + 1), (1, T + 1), (2, T), (25, T - 1), (26, 65), (63, 64), (64, 63), (65, 26), (T - 1, 25),
         (T, 2), (T + 1, 1), (2 * T + 1, 0), (80, 120)]
KINDS = [('u', 'uniform', dict(low=-5.0, high=5.0)),
         ('qu', 'quniform', dict(low=0.0, high=9.0, q=1.0)),
         ('lu', 'loguniform', dict(low=-5.0, high=2.0)),
         ('qlu', 'qloguniform', dict(low=0.0, high=4.0, q=1.0)),
         ('n', 'normal', dict(mu=0.0, sigma=3.0)),
         ('qn', 'qnormal', dict(mu=0.0, sigma=3.0, q=0.5)),
         ('ln', 'lognormal', dict(mu=0.0, sigma=1.0)),
         ('qln', 'qlognormal', dict(mu=1.0, sigma=1.0, q=1.0)),
         ('ri', 'randint', dict(upper=7)),                                      # < kCatFewBins bins
         ('pc', 'categorical', dict(upper=40, p=(np.arange(1, 41) / 820.0).tolist()))]   # > kCatFewBins bins


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd.engine import Engine
    e = Engine(0, 'f64')
    yield e
    e.close()


def history(nb, na, seed):
    """n = nb + na + 7 trials, the sides interleaved by a seeded shuffle (7
    trials in neither set).  Labels: the ten kinds active in every trial; a
    conditional one seen in every third trial and one seen in below trials
    only; five uniform labels over values in (0, 1) whose prior mean -- chosen
    through low / high -- falls before all values, in the first tile, on the
    boundary of the first two tiles of the longer side, in the last tile and
    after all values."""
    rng = np.random.RandomState(seed)
    n = nb + na + 7
    side = rng.permutation(np.repeat([1, 2, 0], [nb, na, 7])).astype(np.uint8)
    tids = np.arange(n, dtype=np.int64)
    labels, obs = list(KINDS), {}
    for name, kind, args in KINDS:
        obs[name] = (tids, prior_draw(kind, args, rng, n))
    v = rng.uniform(size=n)
    longer = np.sort(v[side == (1 if nb >= na else 2)])
    edge = 0.5 * (longer[T - 1] + longer[T]) if len(longer) > T else 0.5
    for name, pmu in (('before', -2.0), ('first', 0.01), ('edge', edge), ('last', 0.99), ('after', 3.0)):
        labels.append((name, 'uniform', dict(low=pmu - 0.5, high=pmu + 0.5)))
        obs[name] = (tids, v)
    labels += [('third', 'normal', dict(mu=0.0, sigma=1.0)), ('onlyb', 'uniform', dict(low=0.0, high=1.0))]
    obs['third'] = (tids[::3], rng.normal(size=len(tids[::3])))
    obs['onlyb'] = (tids[side == 1], rng.uniform(size=nb))
    return labels, tids, side, obs


def check(eng, labels, side, obs, which):
    for li, (name, kind, args) in enumerate(labels):
        if li not in which:
            continue
        oi, ov = obs[name]
        ref = P.label_posterior(name, kind, args, ov[side[oi] == 1], ov[side[oi] == 2], PW)
        for sd, want in enumerate((ref.below, ref.above)):
            w, m, s = eng.get_mixture(li, sd)
            if kind in P.CATEGORICAL:
                want = (want, np.zeros_like(want), np.zeros_like(want))
            assert len(w) == len(want[0]), (name, sd)
            for got, exp, what in zip((w, m, s), want, ('weights', 'mus', 'sigmas')):
                assert np.array_equal(got, exp), (name, sd, what)


@pytest.mark.parametrize('nb,na', SIZES)
def test_split_build_is_label_posterior(eng, nb, na):
    labels, tids, side, obs = history(nb, na, seed=nb * 7 + na)
    sp, cat_p, _, off, otrial, oval = P.device_inputs(labels, tids, np.zeros(len(tids)), obs)
    eng.history_reset(sp, cat_p)
    eng.history_append(np.diff(off), otrial, oval)
    obs_of = P._ObsOf(off, otrial, oval)
    # the route of every mixture: a ramp (n > lf) over tied values needs numpy's order, nothing else does
    want = np.zeros(len(labels), dtype=np.int32)
    for li, (name, kind, _) in enumerate(labels):
        pos, val = obs_of(li)
        for sd in (1, 2):
            x = val[side[pos] == sd]
            if kind not in P.CATEGORICAL and len(x) > LF and len(np.unique(x)) < len(x):
                want[li] |= sd
    ties = eng.build_split(side, PW, LF)
    assert np.array_equal(ties, want)
    names = [l[0] for l in labels]
    assert not ties[[names.index(k) for k in ('u', 'lu', 'n', 'ln', 'before', 'first', 'edge', 'last', 'after')]].any()
    if (nb, na) == (80, 120):
        assert ties[names.index('qu')] == 3
    check(eng, labels, side, obs, set(np.flatnonzero(ties == 0).tolist()))
    if ties.any():
        again = eng.build_split(side, PW, LF, P.split_orders(side, obs_of, set(np.flatnonzero(ties & 1).tolist()), 1),
                                P.split_orders(side, obs_of, set(np.flatnonzero(ties & 2).tolist()), 2))
        assert not again.any()
    check(eng, labels, side, obs, set(range(len(labels))))


def test_split_built_records_score_as_uploaded_ones(eng):
    """The records the split build folds on the device (long lists on both
    sides) against the same mixtures uploaded and folded on the host:
    Engine.score at the project's fp64 bar (helpers.assert_lpdf_close; the two
    folds take log and erf from different libraries, so not bit for bit)."""
    from hyperopt_amd.engine import Engine
    from tests.helpers import assert_lpdf_close
    labels, tids, side, obs = history(T + 1, 65, seed=3)
    sp, cat_p, _, off, otrial, oval = P.device_inputs(labels, tids, np.zeros(len(tids)), obs)
    eng.history_reset(sp, cat_p)
    eng.history_append(np.diff(off), otrial, oval)
    P.build_split_reference_order(eng, side, PW, LF, P._ObsOf(off, otrial, oval))
    up = Engine(0, 'f64')
    try:
        up.set_posterior(*P.pack([P.label_posterior(k, kind, args, obs[k][1][side[obs[k][0]] == 1],
                                                    obs[k][1][side[obs[k][0]] == 2], PW)
                                  for k, kind, args in labels]))
        for li, (name, kind, _) in enumerate(labels):
            cand = obs[name][1][:96]
            got, want = eng.score(li, cand), up.score(li, cand)
            for g, w in zip(got[:2], want[:2]):
                assert_lpdf_close(g, w, quantized=kind.startswith('q'))
    finally:
        up.close()


def test_split_build_errors(eng):
    from hyperopt_amd.engine import Engine, EngineError
    labels, tids, side, obs = history(30, 40, seed=1)
    sp, cat_p, _, off, otrial, oval = P.device_inputs(labels, tids, np.zeros(len(tids)), obs)
    eng.history_reset(sp, cat_p)
    eng.history_append(np.diff(off), otrial, oval)
    with pytest.raises(EngineError, match='out of range'):       # side shorter than the history
        eng.build_split(side[:-1], PW, LF)
    short = (np.arange(len(labels) + 1, dtype=np.int64) > 0) * 29, np.arange(29, dtype=np.int32)
    with pytest.raises(EngineError, match='order'):              # 29 entries for label 0's 30 below observations
        eng.build_split(side, PW, LF, orders_below=short)
    with pytest.raises(ValueError):                              # offsets that do not end at len(order)
        eng.build_split(side, PW, LF, orders_above=(short[0], short[1][:5]))
    with pytest.raises(ValueError):
        eng.build_split(side, PW, 0)
    p = side.ctypes.data_as(ctypes.c_void_p)
    assert eng.lib.tpe_build_split_resident(eng.h, p, len(side), PW, 0, None, None, None, None, None) == L.TPE_ERR_ARG
    two = Engine([0, 0], 'f64')
    try:
        two.history_reset(sp, cat_p)
        with pytest.raises(ValueError):
            two.build_split(side, PW, LF)
        assert two.lib.tpe_build_split_resident(two.h, p, len(side), PW, LF, None, None, None, None,
                                                None) == L.TPE_ERR_ARG
    finally:
        two.close()
    assert not eng.build_split(side, PW, LF)[[0, 2, 4, 6]].any()   # the context still builds
