"""tpe.hypervolume with four objectives and its numpy builder against a plain
exact reference: the rows' coordinates and the reference point cut the box into
cells, a cell belongs to the first ('before') or the only ('others') row whose
box holds it, and the cells' volumes are added as integers."""
import functools
import itertools
from fractions import Fraction

import numpy as np
import pytest

from tests import mo_reference as R
from tests.test_hypervolume_host import small_space

MODES = ('before', 'others')
CASES = ['uniform-1', 'uniform-2', 'uniform-3', 'uniform-65', 'ties', 'simplex', 'origin', 'origin-344', 'beyond',
         'constrained', 'chain', 'reverse-chain']


def exact_exclusive4(rows, ref, mode):
    """excl of every row of `rows` (4-tuples of integers; all valid) as Python integers."""
    n = len(rows)
    axes = [sorted({r[m] for r in rows} | {ref[m]}) for m in range(4)]
    owner = np.full([len(ax) - 1 for ax in axes], n, dtype=np.int16)
    many = np.zeros(owner.shape, dtype=bool)
    for i in reversed(range(n)):                      # (the smallest i is written last)
        box = tuple(slice(axes[m].index(rows[i][m]), None) for m in range(4))
        many[box] |= owner[box] < n
        owner[box] = i
    if mode == 'others':
        owner[many] = n
    small = ref[0] * ref[1] * ref[2] * ref[3] < 2 ** 52           # every sum below exact in int64 and float64
    w = [np.diff(np.array(ax, dtype=object)).astype(np.int64 if small else object) for ax in axes]
    vol = np.multiply.outer(np.multiply.outer(w[1], w[2]), w[3]).ravel()
    out = np.zeros(n + 1, dtype=object)
    for ix in range(len(w[0])):
        own = owner[ix].ravel()
        if small:
            out += np.bincount(own, weights=w[0][ix] * vol, minlength=n + 1).astype(np.int64).astype(object)
        else:
            np.add.at(out, own, w[0][ix] * vol)
    return [int(v) for v in out[:n]]


def sum_points(side, total, rng):                     # the integer points of [0, side)^4 with that sum, shuffled
    pts = [p for p in itertools.product(range(side), repeat=4) if sum(p) == total]
    return rng.permutation(np.array(pts, dtype=float))


def case(name):
    """(F, G or None, the reference's value on every axis): integer-valued rows."""
    rng = np.random.RandomState(len(name) * 7 + 4)
    if name.startswith('uniform'):
        return rng.randint(0, 1001, (int(name.split('-')[1]), 4)).astype(float), None, 1001
    if name == 'ties':                                # ties and duplicates on every axis, two chunks
        return rng.randint(0, 5, (300, 4)).astype(float), None, 1001
    if name == 'simplex':                             # 670 mutually non-dominated rows, three chunks
        return sum_points(10, 18, rng), None, 10
    if name.startswith('origin'):                     # the last row keeps the whole antichain
        side, total = (6, 10) if name == 'origin' else (8, 14)
        return np.vstack([sum_points(side, total, rng) + 1, np.zeros((1, 4))]), None, side + 1
    if name.endswith('chain'):                        # every row dominates all earlier ones; reverse: is dominated
        t = 10 * np.arange(40.0)[:, None]
        return np.repeat(t if name == 'reverse-chain' else 1000 - t, 4, axis=1), None, 1001
    F = rng.randint(0, 1001, (30, 4)).astype(float)
    if name == 'beyond':                              # on and past the reference, NaN, +inf, -inf: five rows skipped
        F[3, 0], F[7, 3], F[11, 1], F[12, 2], F[20, 3] = 1001, 1500, np.nan, np.inf, -np.inf
        return F, None, 1001
    assert name == 'constrained'                      # the infeasible row 5 would dominate every other row
    F[5] = 0
    G = np.full((30, 1), -1.0)
    G[5], G[9] = 0.5, np.nan
    return F, G, 1001


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """The case's exact excl column (0 for the rows that are not valid) and the number of valid rows."""
    F, G, ref = case(name)
    ok = np.isfinite(F).all(axis=1) & np.array([all(v < ref for v in row) for row in F])
    if G is not None:
        ok &= np.array([all(g <= 0 for g in row) for row in G])      # (a NaN fails)
    out = np.zeros(len(F), dtype=object)
    out[ok] = exact_exclusive4([tuple(int(v) for v in row) for row in F[ok]], (ref,) * 4, mode)
    return out, int(ok.sum())


def check_case(builder, name, mode):
    """The builder's column, and for 'before' its running sum, are the exact integers; its overflow count, if any, 0."""
    F, G, ref = case(name)
    want, n_valid = expected(name, mode)
    got = builder(F, (float(ref),) * 4, mode, G=G)
    if isinstance(got, tuple):
        assert got[1] == 0 or name == 'origin-344'
        got = got[0]
    assert got.dtype == np.float64 and np.isfinite(got).all() and [int(v) for v in got] == want.tolist()
    assert n_valid == {'beyond': 25, 'constrained': 28}.get(name, len(F))
    if mode == 'before':
        assert [int(v) for v in np.cumsum(got)] == np.cumsum(want).tolist()
        if name.startswith('origin'):                 # the antichain's size and the last row's gain
            assert (len(F) - 1, want[-1]) == ((146, 1680) if name == 'origin' else (344, 4341))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', CASES)
def test_the_numpy_builder_gives_the_exact_integers(name, mode):
    from hyperopt_amd import posterior as P
    check_case(P.mo_exclusive, name, mode)


@functools.lru_cache(maxsize=None)
def float_case():
    """24 uniform rows in [0, 1)^4 against (1, 1, 1, 1): exact excl as Fractions on the rows' own lattice."""
    F = np.random.RandomState(24).uniform(size=(24, 4))
    den = max(Fraction(float(v)).denominator for v in F.ravel())     # (powers of two: the largest is the lcm)
    rows = [tuple(int(Fraction(float(v)) * den) for v in row) for row in F]
    return F, {mode: [Fraction(v, den ** 4) for v in exact_exclusive4(rows, (den,) * 4, mode)] for mode in MODES}


def check_floats(builder):
    """Per row |excl - exact| <= (3 m + 8) 2^-53 exact, m the rows of J ("Four objectives": k + 3
    roundings a cell, + 2 + k along s, + 2 + k along t, k <= m kept points, non-negative terms only)."""
    F, exact = float_case()
    for mode in MODES:
        got = builder(F, (1.0,) * 4, mode)
        for i, (g, e) in enumerate(zip(got, exact[mode])):
            m = i if mode == 'before' else len(F) - 1
            assert abs(Fraction(float(g)) - e) <= (3 * m + 8) * e / 2 ** 53
    return F


def test_the_numpy_builder_on_floats():
    from hyperopt_amd import posterior as P
    check_floats(P.mo_exclusive)


def check_public(builder):
    """30 documents, four objectives and one constraint; rows 4 and 17 infeasible, row 4 below every other row."""
    from hyperopt_amd import tpe
    F = np.random.RandomState(30).randint(0, 101, (30, 4)).astype(float)
    F[4] = 0
    g = np.full(30, -1.0)
    g[[4, 17]] = 2.0
    names = ('loss', 'latency', 'memory', 'energy')
    trials = R.make_trials(small_space(), np.column_stack([F, g]), names=names + ('g',))
    got = tpe.hypervolume(trials, names, reference=(101,) * 4, constraints=('g',), history=True, contributions=True,
                          builder=builder)
    rows = [tuple(int(v) for v in row) for row in F[g <= 0]]
    assert got['skipped'] == 2 and got['hypervolume'] == sum(exact_exclusive4(rows, (101,) * 4, 'before')) > 0
    assert got['hypervolume'] == got['history'][-1] and got['history'][4] == got['history'][3]
    assert got['contributions'] and trials.trials[4]['tid'] not in got['contributions']
    return got


def test_the_public_function_on_the_host(monkeypatch):
    from hyperopt_amd import engine, tpe
    check_public('host')
    monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    trials = R.make_trials(small_space(), np.ones((3, 5)), names=tuple('abcde'))
    with pytest.raises(ValueError, match='2, 3 or 4 objectives'):
        tpe.hypervolume(trials, tuple('abcde'), builder='device')
