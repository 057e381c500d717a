"""Joint-TPE test groups shared by test_joint_host.py (which checks, on the
CPU through the draw port, that the committed seeds exclude no draw and leave
every round's winner a clear margin) and test_joint_gpu.py.

Shapes: D in {1, 2, 5, 20, 33, 70} (registers up to 8 and up to 32
dimensions, LDS beside the exp table up to 64, LDS alone beyond), K_below in
{1, 2, 5, 26}, K_above in {1, 2, 40, 65, 300} (the slices hold 32 components,
the inner loop 4), kinds mixed over uniform / loguniform / normal /
lognormal, bounded and unbounded."""
import numpy as np

from tests.joint_reference import Dim, JointRef

KINDS = ('uniform', 'loguniform', 'normal', 'lognormal')

# name -> (D, K_below, K_above, kinds cycled over the dimensions, generator seed)
GROUPS = {
    'd1_tie': (1, 1, 1, ('uniform',), 10),      # both sides the prior alone: every score ties
    'd1_prior': (1, 2, 1, ('uniform',), 11),
    'd2': (2, 2, 2, ('loguniform', 'normal'), 12),
    'd5_k300': (5, 26, 300, KINDS, 13),
    'd20': (20, 5, 40, KINDS, 14),
    'd33': (33, 26, 65, KINDS, 15),
    'd70': (70, 2, 65, KINDS, 16),
}
TINY = 'd5_k300'     # its below component 3 has mass < 1e-12 in dimension 0's interval

# (group, seed, round, n) of the rounds test_joint_gpu runs
ROUNDS = [('d1_prior', 3, 0, 1), ('d1_prior', 3, 1, 24), ('d2', 5, 2, 24), ('d2', 5, 3, 65),
          ('d5_k300', 7, 40, 24), ('d5_k300', 7, 41, 5000), ('d20', 9, 5, 24), ('d20', 9, 6, 1000),
          ('d33', 21, 7, 24), ('d33', 21, 8, 65), ('d70', 23, 9, 24)]
# (group, seed, round, cand_offset, n) of the draw checks (n D draws each)
DRAWS = [('d1_tie', 4, 0, 0, 65), ('d1_prior', 3, 0, 0, 24), ('d1_prior', 3, 0, (1 << 32) - 2, 1), ('d2', 5, 2, 0, 1000),
         ('d5_k300', 7, 40, 7, 300), ('d20', 9, 5, 0, 65), ('d33', 21, 7, 1, 65), ('d70', 23, 9, 0, 24)]

_built = {}


def group(name):
    """The JointRef of a named group."""
    if name in _built:
        return _built[name]
    Dn, Kb, Ka, kinds, gseed = GROUPS[name]
    rng = np.random.RandomState(gseed)
    dims, prior = [], []
    for d in range(Dn):
        kind = kinds[d % len(kinds)]
        log = kind in ('loguniform', 'lognormal')
        if kind in ('uniform', 'loguniform'):
            low = float(rng.uniform(-6.0, 2.0))
            high = low + float(rng.uniform(0.5, 8.0))
            dims.append(Dim(log, low, high, stream=d + 3))
            prior.append((0.5 * (high + low), high - low))
        else:
            dims.append(Dim(log, None, None, stream=d + 3))
            prior.append((float(rng.uniform(-2.0, 2.0)), float(rng.uniform(0.5, 3.0))))
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
    if name == TINY:
        # a below component 7.6 sigma outside dimension 0's interval
        _, mu, s = sides[0]
        s[3, 0] = 0.01 * prior[0][1]
        mu[3, 0] = dims[0].low - 7.6 * s[3, 0]
    ref = JointRef(dims, sides[0], sides[1])
    _built[name] = ref
    return ref


def engine_args(ref):
    """Engine.set_joint_posterior's arguments for a JointRef."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd.engine import JOINT_DIM_DTYPE
    dims = np.zeros(ref.D, dtype=JOINT_DIM_DTYPE)
    for d, dim in enumerate(ref.dims):
        dims[d]['kind'] = L.TPE_LGMM1 if dim.log else L.TPE_GMM1
        if dim.bounded:
            dims[d]['flags'] = L.TPE_HAS_LOW | L.TPE_HAS_HIGH
            dims[d]['low'], dims[d]['high'] = dim.low, dim.high
        dims[d]['stream'] = dim.stream
    return (dims,) + ref.sides['below'] + ref.sides['above']


def margin_ok(ll, lg):
    """Whether the best score leads the runner-up by more than 1e-9 (|ll| +
    |lg|) of the best: (ok, index of the best)."""
    s = ll - lg
    i = int(np.argmax(s))
    if len(s) == 1:
        return True, i
    rest = np.delete(s, i)
    return bool(s[i] - rest.max() > 1e-9 * (abs(ll[i]) + abs(lg[i]))), i


def fixed_points(ref, rng):
    """Box corners, 8-sigma outliers of the prior and points near every
    bound, as label values [n, D]."""
    rows = []
    lo, hi, mid, far = [], [], [], []
    W, mu, s = ref.sides['below']
    for d, dim in enumerate(ref.dims):
        if dim.bounded:
            a, b = dim.low, np.nextafter(dim.high, -np.inf)
            lo.append(a), hi.append(b), mid.append(0.5 * (a + b)), far.append(b)
        else:
            lo.append(mu[0, d] - 8.0 * s[0, d]), hi.append(mu[0, d] + 8.0 * s[0, d])
            mid.append(mu[0, d]), far.append(mu[0, d] + 8.0 * s[0, d])
    rows += [lo, hi, mid, far]
    for _ in range(4):   # random corners
        pick = rng.randint(0, 2, ref.D)
        rows.append([hi[d] if pick[d] else lo[d] for d in range(ref.D)])
    for k in range(min(len(W), 4)):   # on a component's mean
        rows.append(list(mu[k]))
    y = np.array(rows, dtype=np.float64)
    for d, dim in enumerate(ref.dims):
        if dim.log:
            y[:, d] = np.exp(y[:, d])
    return y
