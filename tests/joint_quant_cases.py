"""Joint-TPE test groups with quantized dimensions, shared by
test_joint_quant_host.py (which checks on the CPU, through the draw port, that
the committed seeds exclude no draw and leave every round's winner a clear
margin over every other configuration) and test_joint_quant_gpu.py.

Shapes: the smallest at which each path can go wrong -- one dimension, dense
beside quantized, coarse grids (duplicate candidates, exact ties, a
qloguniform grid that holds 0), several slices of 32 components with the
groups of 4 and the weight ramp, 9 and 33 dimensions (past the 8- and
32-register variants of the dense kernel), and 60 fine-grid dimensions: 120
per-candidate values, the LDS-alone variant, a product of factors below
1e-320 in every component."""
import numpy as np

from tests.joint_quant_reference import JOINT_QUANT_KINDS, JointQuantRef, QDim

DENSE = ('uniform', 'loguniform', 'normal', 'lognormal')
ALL8 = ('uniform', 'quniform', 'loguniform', 'qloguniform', 'normal', 'qnormal', 'lognormal', 'qlognormal')

# name -> (D, K_below, K_above, kinds cycled over the dimensions, generator seed)
GROUPS = {
    'q1': (1, 2, 1, ('quniform',), 40),
    'q2_mixed': (2, 2, 2, ('uniform', 'quniform'), 41),
    'q3_coarse': (3, 5, 40, ('quniform', 'qloguniform', 'qnormal'), 42),
    'q5_k300': (5, 26, 300, JOINT_QUANT_KINDS + ('uniform',), 43),
    'q9': (9, 5, 40, ALL8, 44),
    'q33': (33, 26, 65, ALL8, 45),
    'q60_fine': (60, 2, 65, JOINT_QUANT_KINDS, 46),
}
COARSE, FINE = 'q3_coarse', 'q60_fine'
# FINE_NOTE.  A factor is a difference over an interval of width w in the
# working space, formed in fp64 from ends of size |e|: any fp64 evaluation --
# the numpy definition's and the device's alike -- carries about 2^-52 |e| / w
# of relative error in it.  With q = 1e-7 sigma a linear kind has w = q and
# |e| <= 8 sigma at the test points: 2e-8 per factor.  A log kind has w = q / x:
# at a value x = e^9 (an 8-sigma outlier of lognormal(1, 1)) the interval is
# 1e-11 wide and a single factor is off by 1e-4, far above 1e-9 |lpdf|, in
# numpy as on the device.  The fine group therefore keeps its log kinds' values
# below 1 (bounds and 8-sigma outliers of the priors included), where w >= q.

# (group, seed, round, n) of the rounds test_joint_quant_gpu runs
ROUNDS = [('q1', 3, 0, 1), ('q1', 3, 1, 24), ('q2_mixed', 5, 2, 24), ('q2_mixed', 5, 3, 65),
          ('q3_coarse', 6, 4, 24), ('q3_coarse', 6, 5, 300), ('q5_k300', 7, 40, 24), ('q5_k300', 7, 41, 5000),
          ('q9', 9, 5, 24), ('q9', 9, 6, 1000), ('q33', 21, 7, 24), ('q33', 21, 8, 65), ('q60_fine', 23, 9, 24)]
# (group, seed, round, cand_offset, n) of the draw checks (n D draws each)
DRAWS = [('q1', 3, 0, 0, 24), ('q1', 3, 0, (1 << 32) - 2, 1), ('q2_mixed', 5, 2, 0, 1000),
         ('q3_coarse', 6, 4, 0, 300), ('q5_k300', 7, 40, 7, 300), ('q9', 9, 5, 0, 65), ('q33', 21, 7, 1, 65),
         ('q60_fine', 23, 9, 0, 24)]
# (group, seed, round, n, first) of the layout check: the round of n candidates
# (one workgroup per tile runs every slice) against its first `first` (one
# workgroup per slice, merged by the second kernel)
LAYOUT = ('q33', 5, 1, 40000, 100)

_built = {}


def group(name):
    """The JointQuantRef of a named group."""
    if name in _built:
        return _built[name]
    Dn, Kb, Ka, kinds, gseed = GROUPS[name]
    rng = np.random.RandomState(gseed)
    fine, coarse = name == FINE, name == COARSE
    dims, prior = [], []
    for d in range(Dn):
        kind = kinds[d % len(kinds)]
        quant = kind in JOINT_QUANT_KINDS
        base = kind[1:] if quant else kind
        log = base in ('loguniform', 'lognormal')
        if base in ('uniform', 'loguniform'):
            if coarse:
                # quniform: the grid 0, 2, 4, 6; qloguniform: exp(low) = 0.2 rounds to 0: the grid 0, 1, 2
                low, high, q = (np.log(0.2), np.log(2.4), 1.0) if log else (0.0, 6.0, 2.0)
            elif fine and log:
                low = float(rng.uniform(-3.0, -1.5))          # values below 1: see FINE_NOTE
                high = low + float(rng.uniform(0.5, 1.5))
            else:
                low = float(rng.uniform(-6.0, 2.0))
                high = low + float(rng.uniform(0.5, 8.0))
                span = np.exp(high) - np.exp(low) if log else high - low
                q = span / float(rng.uniform(5.0, 9.0))
            psig = high - low
            pmu = 0.5 * (high + low)
            lo_hi = (float(low), float(high))
        else:
            if fine and log:
                pmu, psig = float(rng.uniform(-3.0, -2.0)), float(rng.uniform(0.1, 0.25))   # 8 sigma: below 1
            else:
                pmu, psig = float(rng.uniform(-2.0, 2.0)), float(rng.uniform(0.5, 3.0))
            q = (3.0 if coarse else float(rng.uniform(0.2, 0.6))) * (np.exp(pmu) if log else 1.0) * psig
            lo_hi = (None, None)
        if fine:
            q = 1e-7 * psig
        dims.append(QDim(log, lo_hi[0], lo_hi[1], stream=d + 3, q=float(q) if quant else None))
        prior.append((float(pmu), float(psig)))
    sides = []
    for K in (Kb, Ka):
        mu, s = np.empty((K, Dn)), np.empty((K, Dn))
        for d, (pmu, psig) in enumerate(prior):
            mu[0, d], s[0, d] = pmu, psig
            if dims[d].bounded:
                mu[1:, d] = rng.uniform(dims[d].low, dims[d].high, K - 1)
            else:
                mu[1:, d] = pmu + psig * rng.randn(K - 1)
            s[1:, d] = psig * np.exp(rng.uniform(np.log(0.01), 0.0, K - 1))
        w = np.ones(K) if K <= 26 else np.concatenate([[1.0], np.linspace(1.0 / K, 1.0, K - 26), np.ones(25)])
        sides.append((w / w.sum(), mu, s))
    ref = JointQuantRef(dims, sides[0], sides[1])
    _built[name] = ref
    return ref


def dense_group():
    """A dense-only group (tests/joint_cases.py's d5_k300) for the slot beside
    a quantized one."""
    from tests import joint_cases as JC
    return JC.group('d5_k300')


def engine_args(ref):
    """Engine.set_joint_group's mixture arguments and q for a JointQuantRef."""
    from tests import joint_cases as JC
    return JC.engine_args(ref), ref.steps


def margin_ok(vals, ll, lg):
    """Whether the best score leads the best *different configuration* by
    more than 1e-9 (|ll| + |lg|) of the best: (ok, index of the first row that
    holds the best configuration)."""
    s = ll - lg
    i = int(np.argmax(s))
    other = ~np.all(vals == vals[i], axis=1)
    first = int(np.flatnonzero(~other)[0])
    if not other.any():
        return True, first
    return bool(s[i] - s[other].max() > 1e-9 * (abs(ll[i]) + abs(lg[i]))), first


def fixed_points(ref, rng):
    """Grid corners, grid points nearest every component mean and 8-sigma
    outliers of the unbounded priors, as label values [n, D] (quantized
    dimensions on their grids, dense ones as tests/joint_cases.fixed_points)."""
    W, mu, s = ref.sides['below']
    lo, hi, mid, far = [], [], [], []
    for d, dim in enumerate(ref.dims):
        if dim.bounded:
            a, b = dim.low, np.nextafter(dim.high, -np.inf)
            lo.append(a), hi.append(b), mid.append(0.5 * (a + b)), far.append(b)
        else:
            lo.append(mu[0, d] - 8.0 * s[0, d]), hi.append(mu[0, d] + 8.0 * s[0, d])
            mid.append(mu[0, d]), far.append(mu[0, d] + 8.0 * s[0, d])
    rows = [lo, hi, mid, far]
    for _ in range(4):   # random corners
        pick = rng.randint(0, 2, ref.D)
        rows.append([hi[d] if pick[d] else lo[d] for d in range(ref.D)])
    for side in ('below', 'above'):   # on a component's mean
        m = ref.sides[side][1]
        for k in range(min(len(m), 4)):
            rows.append(list(m[k]))
    y = np.array(rows, dtype=np.float64)
    for d, dim in enumerate(ref.dims):
        if dim.log:
            y[:, d] = np.exp(y[:, d])
        if dim.q is not None:
            y[:, d] = np.rint(y[:, d] / dim.q) * dim.q
    return y
