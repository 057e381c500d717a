"""Plain statement of the sampled hypervolume indicator (tpe_mo_exclusive_mc,
posterior.mo_exclusive_mc) in Python loops, floats and ints.  The Philox words
are the oracle's.  It is the yardstick: nothing here calls the code under
test."""
import functools
import itertools
import math

import numpy as np

from oracle.draw_oracle import philox4x32_10

STREAM = 0x7FFFFFBD
KEY = (0x4D4F4856, 0x53414D50)
MODES = ('before', 'others')


@functools.lru_cache(maxsize=None)
def points(M, S):
    """x[s][m] = word m % 4 of the counter (s, m // 4, 0, STREAM)."""
    blocks = [[w.tolist() for w in philox4x32_10((np.arange(S), b, 0, STREAM), KEY)] for b in range((M + 3) // 4)]
    return [[int(blocks[m // 4][m % 4][s]) for m in range(M)] for s in range(S)]


def counts(F, ref, S, G=None):
    """{'before': count, 'others': count, 'covered': int, 'alive': rows, 'V': float}: the rule, start to end."""
    F = [[float(v) for v in row] for row in F]
    n, M = len(F), len(ref)
    valid = [i for i in range(n) if all(math.isfinite(f) and f < r for f, r in zip(F[i], ref))
             and (G is None or all(g <= 0 for g in G[i]))]                  # (a NaN constraint fails)
    out = dict(before=[0] * n, others=[0] * n, covered=0, alive=[], V=0.0)
    if not valid:
        return out
    lo = [min(F[i][m] for i in valid) for m in range(M)]
    span = [float(ref[m]) - lo[m] for m in range(M)]
    T = {i: [math.ceil(((F[i][m] - lo[m]) / span[m]) * 4294967296.0) for m in range(M)] for i in valid}
    alive = [i for i in valid if max(T[i]) < 1 << 32]
    for x in points(M, S):
        hit = [i for i in alive if all(a >= t for a, t in zip(x, T[i]))]
        if hit:
            out['covered'] += 1
            out['before'][hit[0]] += 1
            if len(hit) == 1:
                out['others'][hit[0]] += 1
    out.update(alive=alive, V=functools.reduce(lambda a, b: a * b, span, 1.0))
    return out


# -- the cases both test files run ---------------------------------------------

# rows x objectives x samples, rows randint(0, 40) against (40,) * M.  130 rows: at 64 samples the launcher cuts
# the rows into slices of 44, 44 and 42 (tpe_mo_hvm.h, hvm_slices); 64 x 65 samples: 17 workgroups, the last of one wave
SIZED = ['%d-%d-%d' % c for c in itertools.product((1, 63, 64, 65, 130, 300), (2, 5, 8), (64, 128, 64 * 65))]
NAMED = ('equal', 'dominating', 'single', 'none', 'special', 'constrained', 'thin')
CASES = tuple(SIZED) + NAMED


@functools.lru_cache(maxsize=None)
def case(name):
    """(F, G or None, reference, samples); the named cases have five objectives and 128 samples."""
    if name in SIZED:
        n, M, S = map(int, name.split('-'))
        return np.random.RandomState(n + M).randint(0, 40, (n, M)).astype(float), None, (40.0,) * M, S
    M, S = 5, 128
    F = np.random.RandomState(1005).randint(1, 40, (70, M)).astype(float)
    G = None
    if name == 'equal':                       # 'others': neither of two equal rows is the sole cover
        F = np.array([[5.0] * M, [5.0] * M, [30.0, 1.0, 30.0, 1.0, 30.0]])
    elif name == 'dominating':                # row 0 covers every sample: 'before' leaves its loop at once
        F[0] = 0
    elif name == 'single':                    # T = 0 on every axis: count == S
        F = F[:1]
    elif name == 'none':
        F[:, 2] = 40
    elif name == 'special':                   # six rows that are not valid
        F[3, 0], F[7, 4], F[11, 1], F[12, 2], F[20, 3], F[69, 0] = 40, 1500, np.nan, np.inf, -np.inf, np.nan
    elif name == 'constrained':               # the infeasible row 5 would cover every sample
        F[5] = 0
        G = np.full((70, 2), -1.0)
        G[5, 1], G[9, 0], G[10, 0] = 0.5, np.nan, -0.0
    else:                                     # a valid row that covers no sample, before a row equal to the minimum
        assert name == 'thin'
        F[2, 3] = np.nextafter(40.0, -np.inf)
        F[3] = 1
    return F, G, (40.0,) * M, S


@functools.lru_cache(maxsize=None)
def expected(name):
    F, G, ref, S = case(name)
    return counts(F.tolist(), ref, S, None if G is None else G.tolist())


def check_case(builder, name, mode):
    """The builder's (count, covered) are the reference's integers."""
    F, G, ref, S = case(name)
    want = expected(name)
    count, covered = builder(F, ref, mode, S, G=G)
    assert count.dtype == np.uint64 and count.tolist() == want[mode] and covered == want['covered']
    if mode == 'before':
        assert sum(want[mode]) == covered
    valid = {'none': 0, 'special': 64, 'constrained': 68}.get(name, len(F))
    assert len(want['alive']) == (valid - 1 if name == 'thin' else valid)
    if name in ('single', 'dominating'):
        assert want['before'][0] == S
    if name == 'equal':
        assert want['others'][:2] == [0, 0] and want['before'][0] > 0


def float_rows():
    return np.random.RandomState(305).uniform(size=(300, 5))


def check_estimator(builder, M):
    """200 uniform rows, 65 536 samples: V covered / S within five binomial standard deviations, p from the exact
    value, of the exact hypervolume (the sum of posterior.mo_exclusive's gains)."""
    from hyperopt_amd import posterior as P
    F, ref, S = np.random.RandomState(M).uniform(size=(200, M)), (1.0,) * M, 65536
    exact = float(np.sum(P.mo_exclusive(F, ref, 'before')))
    V = P.mo_hvm_thresholds(F, ref)[2]
    p = exact / V
    got, sd = V * builder(F, ref, 'before', S)[1] / S, V * math.sqrt(p * (1 - p) / S)
    print('M = %d: exact %.6f, sampled %.6f, %.2f standard deviations' % (M, exact, got, abs(got - exact) / sd))
    assert 0 < p < 1 and abs(got - exact) <= 5 * sd


def public(builder, **kw):
    """40 documents, five objectives and one constraint; rows 4 and 17 infeasible, row 4 below every other row."""
    from hyperopt_amd import tpe
    from tests import mo_reference as R
    from tests.test_hypervolume_host import small_space
    F = np.random.RandomState(40).randint(0, 101, (40, 5)).astype(float)
    F[4] = 0
    g = np.full(40, -1.0)
    g[[4, 17]] = 2.0
    names = ('loss', 'latency', 'memory', 'energy', 'cost')
    trials = R.make_trials(small_space(), np.column_stack([F, g]), names=names + ('g',))
    got = tpe.hypervolume(trials, names, reference=(101,) * 5, constraints=('g',), history=True, contributions=True,
                          builder=builder, method='sampled', **kw)
    want = counts(F.tolist(), (101.0,) * 5, got['n_samples'], g[:, None].tolist())
    return got, want, trials
