"""tpe_interactions, Engine.interactions and tpe.interactions against the plain
restatement in tests/interaction_reference.py."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import posterior as P
from tests import interaction_reference as R
from tests.helpers import assert_lpdf_close, make_history

pytestmark = pytest.mark.gpu

KINDS = [('u', 'uniform', dict(low=-5.0, high=5.0)), ('ln', 'lognormal', dict(mu=0.0, sigma=1.0)),
         ('lu', 'loguniform', dict(low=-5.0, high=2.0))]
BOUNDS = [(-5.0, 5.0), (np.nan, np.nan), (-5.0, 2.0)]
PAIRS = [(0, 1), (0, 2), (1, 2)]
GRIDS = (1, 15, 16, 17, 33, 64, 65, 130)   # the MFMA block, the wave's sub-tile, the tile, a ragged last tile
# K = n + 1 components a side; (5, 16): one past the LDS chunk of 16; 258: past sixteen chunks
SIDES = ((1, 1), (1, 3), (2, 5), (3, 4), (5, 16), (7, 60), (13, 257))
CASES = [(s, g) for g in GRIDS for s in ((2, 5), (3, 4))] + [(s, g) for s in SIDES for g in (17, 65) if s[0] not in (2, 3)]
EPS = 2.0 ** -52


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


class Case(object):
    """A history of the three labels split nb : na, its mixtures, the engine's calls, the reference's planes."""

    def __init__(self, eng, nb, na, zero=False):
        self.eng, self.alpha = eng, nb / (nb + na)
        hist = make_history(KINDS, nb + na, seed=10 * nb + na)
        if zero:
            hist.obs['ln'][1][0] = 0.0
        self.obs = hist.obs
        m = P.joint_mixture(KINDS, hist.obs, P.Splitter(hist.tids, hist.losses, 0.0, n_below=nb), 1.0,
                            bandwidth='scott')
        self.below, self.above = (m.wb, m.mub, m.sigb), (m.wa, m.mua, m.siga)
        self.made = {}

    def axes(self, n_grid):
        ax = [P.interaction_axis(kind, args, self.obs[name][1], n_grid) for name, kind, args in KINDS]
        return [a[0] for a in ax], [a[1] for a in ax]

    def call(self, n_grid, pairs=PAIRS, planes=True):
        y, h = self.axes(n_grid)
        lo, hi = zip(*BOUNDS)
        return self.eng.interactions(y, h, lo, hi, self.below, self.above, self.alpha, pairs, want_planes=planes)

    def get(self, n_grid):
        if n_grid not in self.made:
            y, _ = self.axes(n_grid)
            ref = [[R.side_planes(s, d, e, y[d], y[e], BOUNDS) for s in (self.below, self.above)] for d, e in PAIRS]
            self.made[n_grid] = (self.call(n_grid), ref)
        return self.made[n_grid]


@pytest.fixture(scope='module')
def cases():
    from hyperopt_amd.engine import Engine
    eng, made = Engine(0, 'f64'), {}

    def get(nb, na, **kw):
        key = (nb, na, tuple(kw))
        if key not in made:
            made[key] = Case(eng, nb, na, **kw)
        return made[key]
    yield get
    eng.close()


@pytest.mark.parametrize('sides,n_grid', CASES)
def test_planes_and_sums_against_the_reference(cases, sides, n_grid):
    """With C = n_grid^2 cells and the engine's own planes as the input of both
    sides: V within (C + 24) 2^-52 V -- the terms are non-negative, so the
    fixed-order sum is within (C - 1) 2^-53, and a term takes 10 roundings and
    the cell area 2 on each side (aL, om G, p, L - G, om, ao, the product, the
    quotient, dev^2, p dev^2; h_d h_e and its product with the sum).
    H within (C + c') 2^-52 of the grid's mass h_d h_e sum p, c' = 5000 + Kb +
    Ka: a term p dif^2 moves by at most 2 p |delta dif|, and dif by at most a
    quarter of what the two log-odds move by.  lo: two logs on each side, each
    within an ulp of a value below 745.2, <= 512 * 2^-52 each, and a
    subtraction: 2560 * 2^-52.  loi: four more such logs and three sums on
    each side, 7168 * 2^-52, and the four marginals, each within (2 K + 24)
    2^-53 of the reference's (the fixed-order sums over K terms of the
    marginal and of A, and a few ulps of exp, erfc and the products in each
    term): (2 (Kb + Ka) + 48) 2^-52.  A quarter of the total, doubled, plus the
    eight roundings of the last formula: below (5000 + Kb + Ka) 2^-52 p."""
    c = cases(*sides)
    (H, V, L, G), ref = c.get(n_grid)
    _, h = c.axes(n_grid)
    C, cp = n_grid * n_grid, 5000 + len(c.below[0]) + len(c.above[0])
    for k, (d, e) in enumerate(PAIRS):
        (rL, rLd, rLe), (rG, rGd, rGe) = ref[k]
        assert_lpdf_close(np.log(L[k]), np.log(rL))
        assert_lpdf_close(np.log(G[k]), np.log(rG))
        wantV, wantH, mass = R.sums(L[k], G[k], (rLd, rLe), (rGd, rGe), c.alpha, h[d], h[e])
        print('pair %s: V %.17g ref %.17g; H %.17g ref %.17g; mass %.17g' % ((d, e), V[k], wantV, H[k], wantH, mass))
        assert wantV >= 0.0 and wantH >= 0.0 and mass > 0.0
        assert abs(V[k] - wantV) <= (C + 24) * EPS * wantV
        assert abs(H[k] - wantH) <= (C + cp) * EPS * mass


def test_the_same_bits_alone_among_others_reversed_and_transposed(cases):
    c = cases(7, 60)
    for n_grid in (17, 130):
        (H, V, L, G), _ = c.get(n_grid)
        assert bits(np.stack(c.call(n_grid, planes=False))) == bits(np.stack([H, V]))
        assert c.eng.interactions_last_pair_ms() > 0.0
        back = c.call(n_grid, PAIRS[::-1])
        assert all(bits(a[::-1]) == bits(b) for a, b in zip(back, (H, V, L, G)))
        _, h = c.axes(n_grid)
        for k, (d, e) in enumerate(PAIRS):
            alone = c.call(n_grid, [(d, e)])
            assert all(bits(a[0]) == bits(b[k]) for a, b in zip(alone, (H, V, L, G)))
            Ht, Vt, Lt, Gt = c.call(n_grid, [(e, d)])
            assert_lpdf_close(np.log(Lt[0].T), np.log(L[k]))
            assert_lpdf_close(np.log(Gt[0].T), np.log(G[k]))
            mass = h[d] * h[e] * np.sum(c.alpha * L[k] + (1 - c.alpha) * G[k])
            C, cp = n_grid * n_grid, 5000 + len(c.below[0]) + len(c.above[0])
            assert abs(Vt[0] - V[k]) <= (C + 24) * EPS * V[k] and abs(Ht[0] - H[k]) <= (C + cp) * EPS * mass


@pytest.mark.parametrize('edge', ('factorising', 'zero', 'errors'))
def test_edges(cases, edge):
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import EngineError
    if edge == 'factorising':
        # one trial a side; H is 0 only when each side is ONE product, so the sides go without their prior
        c = cases(1, 1)
        y, h = c.axes(33)
        lo, hi = zip(*BOUNDS)
        one = lambda s: (np.array([0.5, 0.5]), np.repeat(s[1][1:], 2, axis=0), np.repeat(s[2][1:], 2, axis=0))
        H, V, Lp, Gp = c.eng.interactions(y, h, lo, hi, one(c.below), one(c.above), 0.5, PAIRS, want_planes=True)
        mass = [h[d] * h[e] * np.sum(0.5 * Lp[k] + 0.5 * Gp[k]) for k, (d, e) in enumerate(PAIRS)]
        assert np.all(V > 0.0) and np.all(H >= 0.0)
        assert all(H[k] <= (33 * 33 + 5004) * EPS * mass[k] for k in range(3))
    elif edge == 'zero':
        H, V = cases(3, 4, zero=True).call(16, planes=False)
        assert np.isnan(H[[0, 2]]).all() and np.isnan(V[[0, 2]]).all() and np.isfinite(H[1]) and V[1] > 0.0
    else:
        c = cases(3, 4)
        y, h = c.axes(16)
        lo, hi = zip(*BOUNDS)
        good = dict(y=y, h=h, low=lo, high=hi, below=c.below, above=c.above, alpha=c.alpha, pairs=PAIRS)
        bad_sig = (c.below[0], c.below[1], np.where(np.arange(12).reshape(4, 3) == 4, 0.0, c.below[2]))
        inf_sig = (c.below[0], c.below[1], np.where(np.arange(12).reshape(4, 3) == 4, np.inf, c.below[2]))
        refused = [dict(alpha=a) for a in (0.0, 1.0, -0.1, float('nan'))]
        refused += [dict(pairs=p) for p in ([(0, 3)], [(-1, 0)], [(1, 1)])]
        refused += [dict(below=bad_sig), dict(below=inf_sig), dict(below=tuple(a[:1] for a in c.below)),
                    dict(y=[a[:0] for a in y]), dict(y=y[:1], h=h[:1], low=lo[:1], high=hi[:1],
                                                    below=tuple(a[:, :1] if a.ndim == 2 else a for a in c.below),
                                                    above=tuple(a[:, :1] if a.ndim == 2 else a for a in c.above))]
        for kw in refused:
            with pytest.raises(EngineError, match='tpe_interactions'):
                c.eng.interactions(**dict(good, **kw))
        p = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)
        pairs = np.array(PAIRS, dtype=np.int32)
        H, V, plane = np.full(3, -7.0), np.full(3, -7.0), np.full(3 * 256, -7.0)
        Y, Hh = np.stack(y), np.array(h)
        for null, half in ((True, False), (False, True)):
            rc = c.eng.lib.tpe_interactions(
                c.eng.h, 3, 16, None if null else p(Y), p(Hh), p(lo), p(hi), 4, p(c.below[0]), p(c.below[1]),
                p(c.below[2]), 5, p(c.above[0]), p(c.above[1]), p(c.above[2]), c.alpha, 3,
                pairs.ctypes.data_as(ctypes.c_void_p), p(H), p(V), p(plane) if half else None, None)
            assert rc == L.TPE_ERR_ARG and b'tpe_interactions' in c.eng.lib.tpe_last_error(c.eng.h)
        assert np.all(H == -7.0) and np.all(V == -7.0) and np.all(plane == -7.0)
        assert bits(np.stack(c.eng.interactions(**good))) == bits(np.stack(c.get(16)[0][:2]))


def test_public_function_is_the_engines_sums_per_group_and_leaves_main_alone():
    """Two groups (an hp.choice branch's labels, the unconditional ones), no pair across them; each value is
    (n_g / n) H of an Engine.interactions call on the pair's own joint_mixture, exactly."""
    from hyperopt_amd import Domain, Trials, fmin, history, hp, rand, tpe
    from hyperopt_amd.engine import get_engine
    space = dict(a=hp.uniform('a', 0, 1), b=hp.lognormal('b', 0, 1),
                 c=hp.choice('c', [dict(p=hp.normal('p', 0, 2), q=hp.loguniform('q', -3, 1)), dict()]))
    domain = Domain(lambda cfg: (cfg['a'] - 0.5) ** 2 + 0.1 * cfg['c'].get('p', 1.0) ** 2, space)
    trials = Trials()
    fmin(domain.fn, space, algo=rand.suggest, max_evals=60, trials=trials, rstate=np.random.RandomState(3))
    kw = dict(posterior_builder='device', n_EI_candidates=64)
    before = tpe.suggest([5000], domain, trials, 3, **kw)
    got, joint = tpe.interactions(domain, trials, quantile=0.25, n_grid=33, joint=True)
    after = tpe.suggest([5000], domain, trials, 3, **kw)
    assert before[0]['misc']['vals'] == after[0]['misc']['vals']
    specs = tpe.specs_of(domain)
    names = list(specs)
    pq = tuple(sorted('pq', key=names.index))
    assert set(got) == {tuple(sorted('ab', key=names.index)), pq} and list(got) == sorted(got, key=lambda k: -got[k])
    assert tpe.interactions(space, trials, quantile=0.25, n_grid=33, labels=['p', 'q']) == {pq: got[pq]}
    tids, losses, obs = history.gather(domain, trials, list(specs))
    sp = P.Splitter(tids, losses, 0.0, n_below=15)
    for d, e in got:
        m = P.joint_mixture([specs[d], specs[e]], obs, sp, 1.0, bandwidth='scott')
        ax = [P.interaction_axis(specs[k].kind, specs[k].args, obs[k][1], 33) for k in (d, e)]
        pri = [P.joint_prior(specs[k].kind, specs[k].args) for k in (d, e)]
        nb, na = (len(o) for o in sp.split(*obs[d]))
        H, V = get_engine(0, 'f64', 'importance').interactions(
            [a[0] for a in ax], [a[1] for a in ax], [p.low if p.bounded else np.nan for p in pri],
            [p.high if p.bounded else np.nan for p in pri], (m.wb, m.mub, m.sigb), (m.wa, m.mua, m.siga),
            nb / (nb + na), [(0, 1)])
        assert got[d, e] == (nb + na) / 60 * H[0] and joint[d, e] == (nb + na) / 60 * V[0]


def test_planted_interaction_is_found():
    """loss (x - y)^2 + 0.3 (z - 0.5)^2 over 400 prior draws, seed 11: the
    numpy reference gives H_xy / H_xz = 15.19 and H_xy / H_yz = 30.09; half of
    each is asked for."""
    from hyperopt_amd import tpe
    from hyperopt_amd.workloads import history_trials, hp_space
    labels = [(k, 'uniform', dict(low=0.0, high=1.0)) for k in 'xyz']
    hist = make_history(labels, 400, seed=11)
    x, y, z = (hist.obs[k][1] for k in 'xyz')
    hist.losses = (x - y) ** 2 + 0.3 * (z - 0.5) ** 2
    space, trials = hp_space(labels), history_trials(hist)
    got = tpe.interactions(space, trials, n_grid=64)
    # (a label's columns built once for the group of three are those of the pair's own joint_mixture)
    assert tpe.interactions(space, trials, n_grid=64, labels=['y', 'z']) == {('y', 'z'): got['y', 'z']}
    print(got)
    assert list(got)[0] == ('x', 'y')
    assert got['x', 'y'] >= 7.59 * got['x', 'z'] and got['x', 'y'] >= 15.04 * got['y', 'z']
