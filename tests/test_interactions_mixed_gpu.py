"""tpe_interactions_mixed, Engine.interactions_mixed and tpe.interactions(mixed=True) against the plain
restatement in tests/interaction_mixed_reference.py."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import posterior as P
from tests import interaction_mixed_reference as R
from tests.helpers import assert_lpdf_close, make_history

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
PW = 1.0
U, LN, QU, QLN, RI, PC = range(6)
# narrow x wide in both orders, narrow x narrow, dense x quantized, quantized x quantized, quantized x categorical,
# dense x dense (with 17 categories the categorical axes are wide ones)
PAIRS = [(RI, U), (LN, PC), (RI, PC), (U, QLN), (QU, QLN), (QU, RI), (U, LN)]
# (C, q of the quniform label, n_grid): q gives 1, 5, 17 and 65 cells, 10 / 30 at n_grid 17 sixteen cells of
# merge 2, 10 / 64 at n_grid 17 seventeen of merge 4
SHAPES = [(c, 2.5, 17) for c in (1, 2, 3, 15, 16, 17)] + \
         [(3, q, g) for q, g in ((20.0, 17), (10.0 / 30, 17), (10.0 / 16, 17), (10.0 / 64, 17), (10.0 / 64, 65))]
# K = n + 1 components a side: one chunk of 16, the four waves' split (63 / 64 / 65), many chunks
SIDES = ((1, 1), (5, 16), (13, 63), (63, 64), (13, 257))
CASES = [((3, 4), s) for s in SHAPES] + [(s, (3, 10.0 / 16, 17)) for s in SIDES] + [((13, 63), (16, 10.0 / 64, 65))]


def kinds(C, q):
    return [('u', 'uniform', dict(low=-5.0, high=5.0)), ('ln', 'lognormal', dict(mu=0.0, sigma=1.0)),
            ('qu', 'quniform', dict(low=-5.0, high=5.0, q=q)), ('qln', 'qlognormal', dict(mu=0.0, sigma=1.0, q=0.5)),
            ('ri', 'randint', dict(upper=C)),
            ('pc', 'categorical', dict(upper=C, p=(np.arange(C) + 1.0) / np.sum(np.arange(C) + 1.0)))]


def bits(a):
    return b''.join(np.ascontiguousarray(v, dtype=np.float64).tobytes() for v in a)


class Case(object):
    """A history of the six labels split nb : na, its mixtures and axes, the engine's call, the reference's planes."""

    def __init__(self, eng, sides, shape):
        (nb, na), (C, q, n_grid) = sides, shape
        self.eng, self.alpha, labels = eng, nb / (nb + na), kinds(C, q)
        hist = make_history(labels, nb + na, seed=10 * nb + na)
        hist.obs['qln'][1][0] = 0.0
        m = P.joint_mixture(labels, hist.obs, P.Splitter(hist.tids, hist.losses, 0.0, n_below=nb), PW, quantized=True,
                            categorical=True, bandwidth='scott')
        self.below, self.above = (m.wb, m.mub, m.sigb), (m.wa, m.mua, m.siga)
        self.axes = [P.interaction_axis_record(kind, args, hist.obs[name][1], n_grid) for name, kind, args in labels]
        self.made = None

    def call(self, pairs=PAIRS, planes=True, **kw):
        a = dict(axes=self.axes, below=self.below, above=self.above, prior_weight=PW, alpha=self.alpha, pairs=pairs)
        return self.eng.interactions_mixed(want_planes=planes, **dict(a, **kw))

    def get(self):
        if self.made is None:
            ref = [[R.side_planes(s, d, e, self.axes, PW) for s in (self.below, self.above)] for d, e in PAIRS]
            self.made = (self.call(), ref)
        return self.made


@pytest.fixture(scope='module')
def cases():
    from hyperopt_amd.engine import Engine
    eng, made = Engine(0, 'f64'), {}

    def get(sides, shape):
        if (sides, shape) not in made:
            made[sides, shape] = Case(eng, sides, shape)
        return made[sides, shape]
    yield get
    eng.close()


def bounds(c, k, ref):
    """(C + 24, C + c'): tests/test_interactions_gpu.py's constants with C = G_d G_e cells.  V takes the engine's
    own planes on both sides: unchanged.  H: c' = 5000 + Kb + Ka as derived there, plus the reference's slack --
    an interval mass is a difference of two erfc values, each within joint_quant_reference.mass_tolerance of its
    size, which the marginal of a quantized axis carries relative to its own value on both sides of the
    comparison (side_planes sums it: the largest relative error of each quantized marginal, in 2^-52).  The
    categorical factor is five roundings of exact inputs: inside the few ulps a term already has.  The slack
    has no bound of its own (it grows with z^2 in the tails), so it is capped at the 5000 of the logs it is added
    to: it may at most double the dense bound, and a case whose slack is larger has to be dropped, not passed."""
    d, e = PAIRS[k]
    C = len(c.axes[d].x) * len(c.axes[e].x)
    slack = 2.0 * (ref[k][0][3] + ref[k][1][3])
    assert slack <= 5000.0
    return C + 24, C + 5000 + len(c.below[0]) + len(c.above[0]) + slack


@pytest.mark.parametrize('sides,shape', CASES)
def test_planes_and_sums_against_the_reference(cases, sides, shape):
    c = cases(sides, shape)
    (H, V, L, G), ref = c.get()
    for k, (d, e) in enumerate(PAIRS):
        (rL, rLd, rLe, _), (rG, rGd, rGe, _) = ref[k]
        quant = R.QUANTIZED in (c.axes[d].kind, c.axes[e].kind)
        with np.errstate(divide='ignore'):
            assert_lpdf_close(np.log(L[k]), np.log(rL), quantized=quant)
            assert_lpdf_close(np.log(G[k]), np.log(rG), quantized=quant)
        area = c.axes[d].measure * c.axes[e].measure
        wantV, wantH, mass = R.sums(L[k], G[k], (rLd, rLe), (rGd, rGe), c.alpha, area)
        cv, ch = bounds(c, k, ref)
        print('pair %s %s: V %.17g ref %.17g; H %.17g ref %.17g; mass %.17g; bounds %g %g'
              % ((d, e), L[k].shape, V[k], wantV, H[k], wantH, mass, cv, ch))
        assert wantV >= 0.0 and wantH >= 0.0 and mass > 0.0
        assert abs(V[k] - wantV) <= cv * EPS * wantV
        assert abs(H[k] - wantH) <= ch * EPS * mass


@pytest.mark.parametrize('sides,shape', [((13, 63), (3, 10.0 / 16, 17)), ((13, 63), (16, 10.0 / 64, 65))])
def test_the_same_bits_alone_among_others_reversed_and_transposed(cases, sides, shape):
    c = cases(sides, shape)
    (H, V, L, G), ref = c.get()
    assert bits(c.call(planes=False)) == bits([H, V])
    assert c.eng.interactions_last_pair_ms() > 0.0
    back = c.call(PAIRS[::-1])
    assert all(bits(a[::-1]) == bits(b) for a, b in zip(back, (H, V, L, G)))
    for k, (d, e) in enumerate(PAIRS):
        alone = c.call([(d, e)])
        assert all(bits(a[:1]) == bits(b[k:k + 1]) for a, b in zip(alone, (H, V, L, G)))
        Ht, Vt, Lt, Gt = c.call([(e, d)])
        quant = R.QUANTIZED in (c.axes[d].kind, c.axes[e].kind)
        with np.errstate(divide='ignore'):
            assert_lpdf_close(np.log(Lt[0].T), np.log(L[k]), quantized=quant)
            assert_lpdf_close(np.log(Gt[0].T), np.log(G[k]), quantized=quant)
        mass = c.axes[d].measure * c.axes[e].measure * np.sum(c.alpha * L[k] + (1 - c.alpha) * G[k])
        cv, ch = bounds(c, k, ref)
        assert abs(Vt[0] - V[k]) <= cv * EPS * V[k] and abs(Ht[0] - H[k]) <= ch * EPS * mass


def test_a_side_of_one_product_has_no_interaction(cases):
    """One trial a side, passed as that trial's kernel twice: component 0 of a categorical axis is its prior, so
    a side is one product for every pair with at most one categorical label (all but (RI, PC))."""
    c = cases((1, 1), (3, 10.0 / 16, 17))
    one = lambda s: (np.array([0.5, 0.5]), np.repeat(s[1][1:], 2, axis=0), np.repeat(s[2][1:], 2, axis=0))
    pairs = [p for p in PAIRS if p != (RI, PC)]
    H, V, L, G = c.call(pairs, below=one(c.below), above=one(c.above), alpha=0.5)
    for k, (d, e) in enumerate(pairs):
        mass = c.axes[d].measure * c.axes[e].measure * np.sum(0.5 * L[k] + 0.5 * G[k])
        slack = [R.side_planes(one(s), d, e, c.axes, PW)[3] for s in (c.below, c.above)]
        assert 2.0 * sum(slack) <= 5000.0
        assert V[k] > 0.0 and 0.0 <= H[k] <= (L[k].size + 5004 + 2.0 * sum(slack)) * EPS * mass


def history_of(labels, n, seed, loss):
    from hyperopt_amd import hp
    from hyperopt_amd.workloads import history_trials, hp_space
    hist = make_history(labels, n, seed=seed)
    hist.losses = loss({k: hist.obs[k][1] for k, _, _ in labels})
    space = hp_space([l for l in labels if l[1] != 'categorical'])
    for k, _, args in [l for l in labels if l[1] == 'categorical']:
        space[k] = hp.pchoice(k, [(p, i) for i, p in enumerate(args['p'])])
    return hist, space, history_trials(hist)


def test_public_function_is_the_engines_sums_and_dense_pairs_keep_their_bits():
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import get_engine
    labels = kinds(3, 0.5)
    hist, space, trials = history_of(labels, 40, 3, lambda o: (o['u'] - o['qu']) ** 2 + o['ri'])
    got, joint = tpe.interactions(space, trials, quantile=0.25, n_grid=33, joint=True, mixed=True)
    dense = tpe.interactions(space, trials, quantile=0.25, n_grid=33, joint=True)
    names = [k for k in got]
    assert len(got) == 15 and set(dense[0]) == {p for p in got if set(p) == {'u', 'ln'}}
    assert all(got[p] == dense[0][p] and joint[p] == dense[1][p] for p in dense[0])
    assert tpe.interactions(space, trials, quantile=0.25, n_grid=33, labels=['qu', 'pc'], mixed=True) == \
        {p: got[p] for p in got if set(p) == {'qu', 'pc'}}
    with pytest.raises(ValueError, match="label 'qu' is of kind 'quniform'"):
        tpe.interactions(space, trials, quantile=0.25, n_grid=33, labels=['u', 'qu'])
    by = {k: (kind, args) for k, kind, args in labels}
    sp = P.Splitter(hist.tids, hist.losses, 0.0, n_below=10)
    for d, e in names:
        m = P.joint_mixture([(k,) + by[k] for k in (d, e)], hist.obs, sp, PW, quantized=True, categorical=True,
                            bandwidth='scott')
        axes = [P.interaction_axis_record(by[k][0], by[k][1], hist.obs[k][1], 33) for k in (d, e)]
        H, V = get_engine(0, 'f64', 'importance').interactions_mixed(
            axes, (m.wb, m.mub, m.sigb), (m.wa, m.mua, m.siga), PW, 0.25, [(0, 1)])
        assert got[d, e] == H[0] and joint[d, e] == V[0]


def test_planted_choice_by_number_interaction_is_found():
    """loss (log lr - c[opt])^2 with c = (-6, -4, -2) over 200 prior draws, and a batch size that does not matter."""
    from hyperopt_amd import tpe
    labels = [('opt', 'randint', dict(upper=3)), ('lr', 'loguniform', dict(low=-8.0, high=0.0)),
              ('bs', 'quniform', dict(low=16.0, high=256.0, q=16.0))]
    c = np.array([-6.0, -4.0, -2.0])
    _, space, trials = history_of(labels, 200, 11, lambda o: (np.log(o['lr']) - c[o['opt'].astype(int)]) ** 2)
    got = tpe.interactions(space, trials, n_grid=64, mixed=True)
    print(got)
    assert len(got) == 3 and set(list(got)[0]) == {'opt', 'lr'}


def test_errors(cases):
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import EngineError
    c = cases((3, 4), (3, 2.5, 17))
    ax = c.axes
    swap = lambda d, **kw: [a._replace(**kw) if i == d else a for i, a in enumerate(ax)]
    cat_mu = lambda v: (c.below[0], np.where(np.arange(24).reshape(4, 6) == 6 + RI, v, c.below[1]), c.below[2])
    refused = [dict(axes=swap(QU, kind=3)), dict(axes=swap(U, x=ax[U].x[:0])), dict(axes=swap(U, x=np.zeros(1025))),
               dict(axes=swap(RI, upper=2)), dict(below=cat_mu(0.5)), dict(below=cat_mu(3.0)), dict(below=cat_mu(-1.0)),
               dict(axes=swap(QU, step=0.0)), dict(axes=swap(QU, step=np.inf)), dict(axes=swap(QU, step=np.nan)), dict(axes=swap(U, measure=0.0)),
               dict(axes=swap(QLN, measure=np.nan)),
               dict(axes=swap(PC, p=np.array([0.5, 0.0, 0.5]))), dict(axes=swap(PC, p=np.array([0.5, np.inf, 0.5]))),
               dict(alpha=1.0), dict(pairs=[(0, 6)]), dict(pairs=[(1, 1)]), dict(prior_weight=0.0),
               dict(below=tuple(a[:1] for a in c.below))]
    for kw in refused:
        with pytest.raises(EngineError, match='tpe_interactions_mixed'):
            c.call(planes=False, **kw)
    # the outputs of a refused call are untouched
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    from hyperopt_amd.engine import AXIS_DTYPE
    rec = np.zeros(6, dtype=AXIS_DTYPE)
    rec['kind'], rec['n_cells'] = 7, 4
    H, V, pairs = np.full(1, -7.0), np.full(1, -7.0), np.array([[0, 1]], dtype=np.int32)
    rc = c.eng.lib.tpe_interactions_mixed(
        c.eng.h, 6, p(rec), p(np.zeros(24)), None, 0, 4, p(c.below[0]), p(c.below[1]), p(c.below[2]), 5, p(c.above[0]),
        p(c.above[1]), p(c.above[2]), PW, c.alpha, 1, p(pairs), p(H), p(V), None, None, None)
    assert rc == L.TPE_ERR_ARG and b'tpe_interactions_mixed' in c.eng.lib.tpe_last_error(c.eng.h)
    assert H[0] == -7.0 and V[0] == -7.0
    assert bits(c.call(planes=False)) == bits(c.get()[0][:2])
