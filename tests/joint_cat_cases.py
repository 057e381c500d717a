"""Joint-TPE test groups with categorical dimensions, shared by
test_joint_cat_host.py (which checks on the CPU, through the draw port, that
the committed seeds exclude no draw and leave every round's winner a clear
margin over every other configuration) and test_joint_cat_gpu.py.

Shapes: the smallest at which each path can go wrong -- one categorical
dimension, dense beside categorical, an all-categorical group (real ties in
every round, the all-categorical weight rule), dense, quantized and
categorical together over several slices of 32 components with the groups of
4 and the weight ramp, 9 and 33 dimensions of all ten kinds (past the 8- and
32-register variants of the dense kernel), 33 categorical dimensions (the
acceptance rule) and 1000 categories (the cumulative search)."""
import numpy as np

from tests import joint_quant_cases as QC
from tests.joint_cat_reference import CDim, JointCatRef
from tests.joint_quant_reference import JOINT_QUANT_KINDS

ALL10 = ('uniform', 'randint', 'quniform', 'loguniform', 'categorical', 'qloguniform', 'normal', 'qnormal',
         'lognormal', 'qlognormal')

# name -> (D, K_below, K_above, kinds cycled over the dimensions, generator seed, prior weight)
# a categorical kind may fix its shape: ('randint', C) or ('categorical', p)
GROUPS = {
    'c1': (1, 2, 1, (('randint', 3),), 60, 1.0),
    'c2_mixed': (2, 2, 2, ('uniform', ('randint', 4)), 61, 1.0),
    'c3_all': (3, 5, 40, (('randint', 2), ('categorical', (0.5, 0.3, 0.2)), ('randint', 5)), 62, 1.0),
    'c5_k300': (5, 26, 300, ('uniform', 'quniform', ('randint', 6), 'lognormal', 'categorical'), 63, 1.0),
    'c9': (9, 5, 40, ALL10, 64, 0.7),
    'c33': (33, 26, 65, ALL10, 65, 1.0),
    'c33_cat': (33, 2, 2, ('randint', 'categorical'), 66, 1.0),
    'c_wide': (2, 5, 40, ('uniform', ('randint', 1000)), 67, 1.0),
}
ALL_CAT = 'c3_all'
# COND_NOTE.  As joint_quant_cases.FINE_NOTE says, a quantized factor is a
# difference over an interval of width w in the working space, formed in fp64
# from ends of size |e|, and any fp64 evaluation of it -- the numpy
# definition's and the device's alike -- carries about 2^-52 |e| / w of
# relative error.  At the 8-sigma outlier of a qlognormal prior the interval is
# w = q / x = c psig exp(-8 psig) wide (q = c exp(pmu) psig, c in [0.2, 0.6]):
# 1e-11 for psig = 3, where a single factor of the definition itself is off by
# 1e-5, far above 1e-9 |lpdf|.  These groups draw a qlognormal's psig from
# [0.3, 1]: w >= 6e-5 and |e| <= 10, below 4e-11 per factor -- the score test
# then checks the device against a definition that is itself good to the bound.

# (group, seed, round, n) of the rounds test_joint_cat_gpu runs
ROUNDS = [('c1', 3, 0, 1), ('c1', 3, 1, 24), ('c2_mixed', 5, 2, 24), ('c2_mixed', 5, 3, 65),
          ('c3_all', 6, 4, 24), ('c3_all', 6, 5, 300), ('c5_k300', 7, 40, 24), ('c5_k300', 7, 41, 5000),
          ('c9', 9, 5, 24), ('c9', 9, 6, 300), ('c33', 21, 7, 24), ('c33', 21, 8, 65), ('c_wide', 23, 9, 65)]
# (group, seed, round, cand_offset, n) of the draw checks (n D draws each)
DRAWS = [('c1', 3, 0, 0, 24), ('c1', 3, 0, (1 << 32) - 2, 1), ('c2_mixed', 5, 2, 0, 1000),
         ('c3_all', 6, 4, 0, 300), ('c5_k300', 7, 40, 7, 300), ('c9', 9, 5, 0, 65), ('c33', 21, 7, 1, 65),
         ('c33_cat', 2, 3, 0, 65), ('c_wide', 23, 9, 0, 300)]
# (group, seed, round, n, first) of the layout check, as joint_quant_cases.LAYOUT
LAYOUT = ('c33', 5, 1, 40000, 100)

_built = {}


def group(name):
    """The JointCatRef of a named group."""
    if name in _built:
        return _built[name]
    Dn, Kb, Ka, kinds, gseed, pw = GROUPS[name]
    rng = np.random.RandomState(gseed)
    dims, prior = [], []
    for d in range(Dn):
        kind = kinds[d % len(kinds)]
        shape = None
        if isinstance(kind, tuple):
            kind, shape = kind
        if kind in ('randint', 'categorical'):
            if kind == 'randint':
                C = int(shape) if shape is not None else int(rng.randint(2, 8))
                p = np.full(C, 1.0 / C)
            elif shape is not None:
                p = np.asarray(shape, dtype=np.float64)
                C = len(p)
            else:
                C = int(rng.randint(2, 8))
                p = rng.uniform(0.2, 1.0, C)
                p = p / p.sum()
            dims.append(CDim(False, None, None, stream=d + 3, upper=C, p=p))
            prior.append(None)
            continue
        quant = kind in JOINT_QUANT_KINDS
        base = kind[1:] if quant else kind
        log = base in ('loguniform', 'lognormal')
        if base in ('uniform', 'loguniform'):
            low = float(rng.uniform(-6.0, 2.0))
            high = low + float(rng.uniform(0.5, 8.0))
            span = np.exp(high) - np.exp(low) if log else high - low
            q = span / float(rng.uniform(5.0, 9.0))
            pmu, psig = 0.5 * (high + low), high - low
            lo_hi = (low, high)
        else:
            # (qlognormal: COND_NOTE)
            pmu = float(rng.uniform(-2.0, 2.0))
            psig = float(rng.uniform(0.3, 1.0) if kind == 'qlognormal' else rng.uniform(0.5, 3.0))
            q = float(rng.uniform(0.2, 0.6)) * (np.exp(pmu) if log else 1.0) * psig
            lo_hi = (None, None)
        dims.append(CDim(log, lo_hi[0], lo_hi[1], stream=d + 3, q=float(q) if quant else None))
        prior.append((float(pmu), float(psig)))
    sides = []
    for K in (Kb, Ka):
        mu, s = np.empty((K, Dn)), np.empty((K, Dn))
        for d, pr in enumerate(prior):
            if pr is None:
                mu[0, d], s[:, d] = 0.0, 1.0
                mu[1:, d] = rng.randint(0, dims[d].upper, K - 1)
                continue
            pmu, psig = pr
            mu[0, d], s[0, d] = pmu, psig
            if dims[d].bounded:
                mu[1:, d] = rng.uniform(dims[d].low, dims[d].high, K - 1)
            else:
                mu[1:, d] = pmu + psig * rng.randn(K - 1)
            s[1:, d] = psig * np.exp(rng.uniform(np.log(0.01), 0.0, K - 1))
        w = np.ones(K) if K <= 26 else np.concatenate([[1.0], np.linspace(1.0 / K, 1.0, K - 26), np.ones(25)])
        sides.append((w / w.sum(), mu, s))
    ref = JointCatRef(dims, sides[0], sides[1], prior_weight=pw)
    _built[name] = ref
    return ref


def engine_args(ref):
    """Engine.set_joint_group's mixture arguments and the keywords q, upper,
    cat_p, prior_weight for a JointCatRef."""
    from tests import joint_cases as JC
    return JC.engine_args(ref), dict(q=ref.steps, upper=ref.uppers, cat_p=ref.cat_p, prior_weight=ref.pw)


margin_ok = QC.margin_ok


def fixed_points(ref, rng):
    """joint_quant_cases.fixed_points with the categorical dimensions at their
    category corners (0, C - 1, the middle, random corners) and, in the rows on
    a component, at that component's category."""
    y = QC.fixed_points(ref, rng)
    for d, dim in enumerate(ref.dims):
        if dim.upper:
            y[:4, d] = [0, dim.upper - 1, dim.upper // 2, dim.upper - 1]
            y[4:8, d] = (dim.upper - 1) * rng.randint(0, 2, 4)
    return y
