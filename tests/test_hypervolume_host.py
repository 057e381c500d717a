"""tpe.hypervolume and its numpy builder (posterior.mo_exclusive) against a
plain exact reference: the rows' own coordinates and the reference point cut
the space into cells, a cell belongs to the first row (mode 'before') or the
only row (mode 'others') whose box holds it, and the cells' volumes are added
as Python integers -- no sweep, no staircase, nothing shared with a builder."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from tests import mo_reference as R

REF = 1001
MODES = ('before', 'others')
UNIFORM = (1, 2, 3, 64, 65, 300)
CASES = ['uniform-%d' % n for n in UNIFORM] + ['chain', 'reverse-chain', 'antichain', 'ties', 'duplicates',
                                               'beyond', 'constrained', 'none-valid']


def exact_exclusive(rows, ref, mode):
    """excl of every row of `rows` (tuples of integers; all valid) as Python
    integers.  Cell volumes below 2^53 are added by np.bincount in float64,
    exactly; larger ones as Python integers."""
    n, M = len(rows), len(ref)
    axes = [sorted({r[m] for r in rows} | {ref[m]}) for m in range(M)]
    owner = np.full([len(ax) - 1 for ax in axes], n, dtype=np.int32)
    count = np.zeros(owner.shape, dtype=np.int32)
    for i in reversed(range(n)):                      # (the smallest i is written last)
        box = tuple(slice(axes[m].index(rows[i][m]), None) for m in range(M))
        owner[box] = i
        count[box] += 1
    if mode == 'others':
        owner[count != 1] = n
    small = np.prod([float(ax[-1] - ax[0]) for ax in axes]) < 2.0 ** 52
    w = [np.array([ax[c + 1] - ax[c] for c in range(len(ax) - 1)], dtype=np.int64 if small else object)
         for ax in axes]
    rest = w[1] if M == 2 else np.multiply.outer(w[1], w[2]).ravel()
    out = np.zeros(n + 1, dtype=object)
    for ix in range(len(w[0])):
        own, vol = owner[ix].ravel(), w[0][ix] * rest
        if small:
            out += np.bincount(own, weights=vol, minlength=n + 1).astype(np.int64).astype(object)
        else:
            np.add.at(out, own, vol)
    return [int(v) for v in out[:n]]


def case(name, M):
    """(F, G or None): integer-valued rows in [0, 1000] unless the case says otherwise."""
    rng = np.random.RandomState(len(name) * 7 + M)
    t = np.arange(40.0)
    if name.startswith('uniform'):
        return rng.randint(0, 1001, (int(name.split('-')[1]), M)).astype(float), None
    if name == 'chain':                               # every row dominates all earlier ones
        return np.repeat(1000 - 10 * t[:, None], M, axis=1), None
    if name == 'reverse-chain':                       # every gain after the first is 0
        return np.repeat(10 * t[:, None], M, axis=1), None
    if name == 'antichain':
        return np.column_stack([10 * t, 1000 - 10 * t, (37 * t) % 101][:M]), None
    if name == 'ties':
        return rng.randint(0, 5, (60, M)).astype(float), None
    if name == 'duplicates':
        return rng.permutation(np.repeat(rng.randint(0, 1001, (20, M)), 2, axis=0)).astype(float), None
    F = rng.randint(0, 1001, (30, M)).astype(float)
    if name == 'beyond':                              # on and past the reference, NaN, +inf, -inf: five rows skipped
        F[3, 0], F[7, M - 1], F[11, 1], F[12, 0], F[20, 1] = REF, 1500, np.nan, np.inf, -np.inf
        return F, None
    if name == 'constrained':                         # the infeasible row 5 would dominate every other row
        F[5] = 0
        G = np.full((30, 1), -1.0)
        G[5], G[9] = 0.5, np.nan
        return F, G
    assert name == 'none-valid'
    return F + REF, None


def valid_rows(F, G, ref):
    ok = np.isfinite(F).all(axis=1) & np.array([all(v < r for v, r in zip(row, ref)) for row in F])
    if G is not None:
        ok &= np.array([all(g <= 0 for g in row) for row in G])      # (a NaN fails)
    return ok


@functools.lru_cache(maxsize=None)
def expected(name, M, mode):
    """The case's exact excl column (0 for the rows that are not valid) and the valid mask."""
    F, G = case(name, M)
    ok = valid_rows(F, G, (REF,) * M)
    out = np.zeros(len(F), dtype=object)
    out[ok] = exact_exclusive([tuple(int(v) for v in row) for row in F[ok]], (REF,) * M, mode)
    return out, ok


def check_case(builder, name, M, mode):
    """`builder(F, reference, mode, G=G)` gives the exact integers; 'before': so does their running sum."""
    F, G = case(name, M)
    want, ok = expected(name, M, mode)
    got = builder(F, (float(REF),) * M, mode, G=G)
    assert got.dtype == np.float64 and [int(v) for v in got] == want.tolist() and np.isfinite(got).all()
    if mode == 'before':
        assert [int(v) for v in np.cumsum(got)] == np.cumsum(want).tolist()
    assert ok.sum() == {'beyond': 25, 'constrained': 28, 'none-valid': 0}.get(name, len(F))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('M', (2, 3))
@pytest.mark.parametrize('name', CASES)
def test_the_numpy_builder_gives_the_exact_integers(name, M, mode):
    from hyperopt_amd import posterior as P
    check_case(P.mo_exclusive, name, M, mode)


def float_case():
    """65 uniform rows in [0, 1)^3 against (1, 1, 1): exact excl per mode as Fractions, on the lattice of
    the rows' own denominators."""
    F = np.random.RandomState(65).uniform(size=(65, 3))
    den = max(Fraction(float(v)).denominator for v in F.ravel())     # (powers of two: the largest is the lcm)
    rows = [tuple(int(Fraction(float(v)) * den) for v in row) for row in F]
    return F, {mode: [Fraction(v, den ** 3) for v in exact_exclusive(rows, (den,) * 3, mode)] for mode in MODES}


def check_floats(builder):
    """Per row |excl - exact| <= (2 m + 6) 2^-53 exact, m the rows of J: the builders add only non-negative
    terms -- per slab at most m + 1 products of two rounded differences (three roundings a term, at most m
    additions), times a rounded thickness (two more), at most m + 1 slabs added up (m more): relative error
    gamma(2 m + 5) <= (2 m + 6) 2^-53 of the exact value, itself at most vol(box i) -- never more than
    8 (m + 1)^2 2^-53 vol(box i).  A row that J weakly dominates is 0 exactly."""
    F, exact = float_case()
    for mode in MODES:
        got = builder(F, (1.0, 1.0, 1.0), mode)
        for i, (g, e) in enumerate(zip(got, exact[mode])):
            m = i if mode == 'before' else len(F) - 1
            print(mode, i, float(g), float(abs(Fraction(float(g)) - e)), float((2 * m + 6) * e / 2 ** 53))
            assert abs(Fraction(float(g)) - e) <= (2 * m + 6) * e / 2 ** 53
    return F, exact


def test_the_numpy_builder_on_floats_and_the_history():
    """history is np.cumsum of the builder's gains, bit for bit, and within the rows' bounds 8 (m + 1)^2 2^-53
    vol(box i) added up of the exact running sum."""
    from hyperopt_amd import posterior as P, tpe
    F, exact = check_floats(P.mo_exclusive)
    trials = R.make_trials(small_space(), F, names=('loss', 'b', 'c'))
    got = tpe.hypervolume(trials, ('loss', 'b', 'c'), reference=(1, 1, 1), history=True, builder='host')
    assert np.array_equal(got['history'], np.cumsum(P.mo_exclusive(F, (1.0, 1.0, 1.0), 'before')))
    run = bound = Fraction(0)
    for i, (h, e) in enumerate(zip(got['history'], exact['before'])):
        run += e
        bound += 8 * (i + 1) ** 2 * np.prod([1 - Fraction(float(v)) for v in F[i]]) / 2 ** 53
        assert abs(Fraction(float(h)) - run) <= bound
    assert got['hypervolume'] == got['history'][-1] and got['skipped'] == 0


def small_space():
    from hyperopt_amd import hp
    return {'x': hp.uniform('x', 0, 1)}


def study():
    """30 documents, two objectives and one constraint; rows 4 and 17 infeasible, row 4 below every other row."""
    rng = np.random.RandomState(30)
    F = rng.randint(0, 1001, (30, 2)).astype(float)
    F[4] = 0
    g = np.full(30, -1.0)
    g[[4, 17]] = 2.0
    return R.make_trials(small_space(), np.column_stack([F, g]), names=('loss', 'cost', 'g')), F, g


def check_public(builder):
    from hyperopt_amd import tpe
    trials, F, g = study()
    got = tpe.hypervolume(trials, ('loss', 'cost'), constraints=('g',), history=True, contributions=True,
                          builder=builder)
    ok = g <= 0
    hi, lo = F[ok].max(axis=0), F[ok].min(axis=0)
    assert got['reference'] == tuple((hi + 0.1 * (hi - lo)).tolist()) and got['skipped'] == 2
    assert got['tids'] == sorted(d['tid'] for d in trials.trials) and len(got['history']) == 30
    assert got['hypervolume'] == got['history'][-1] > 0
    front = {d['tid'] for d in tpe.pareto_front(trials, ('loss', 'cost'), constraints=('g',))}
    assert got['contributions'] and set(got['contributions']) <= front
    assert list(got['contributions'].values()) == sorted(got['contributions'].values(), reverse=True)
    fixed = tpe.hypervolume(trials, ('loss', 'cost'), reference=(REF, REF), constraints=('g',), builder=builder)
    rows = [tuple(int(v) for v in row) for row in F[ok]]
    assert fixed['hypervolume'] == sum(exact_exclusive(rows, (REF, REF), 'before')) and 'history' not in fixed
    return got


def test_the_public_function_on_the_host():
    check_public('host')


def test_no_valid_row_and_equal_values():
    from hyperopt_amd import tpe
    trials = R.make_trials(small_space(), np.full((5, 2), 3.0))
    got = tpe.hypervolume(trials, ('loss', 'cost'), contributions=True, builder='host')
    assert got['reference'] == (4.0, 4.0) and got['hypervolume'] == 1.0 and got['contributions'] == {}
    got = tpe.hypervolume(trials, ('loss', 'cost'), reference=(3, 3), history=True, builder='host')
    assert got['hypervolume'] == 0.0 and got['skipped'] == 5 and not got['history'].any()


@pytest.mark.parametrize('kw', (dict(objectives=('loss',)), dict(objectives=('loss', 'cost', 'a', 'b')),
                                dict(objectives='loss'), dict(constraints=('cost',)), dict(reference=(1.0,)),
                                dict(reference=(1.0, np.inf)), dict(reference=(1.0, np.nan)),
                                dict(objectives=('loss', 'absent')), dict(builder='gpu')))
def test_bad_arguments_raise_before_an_engine_exists(kw, monkeypatch):
    from hyperopt_amd import engine, tpe
    monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    trials = R.make_trials(small_space(), np.ones((3, 2)))
    with pytest.raises(ValueError, match='hypervolume' if kw.get('objectives') == ('loss',) else None):
        tpe.hypervolume(trials, **dict(dict(objectives=('loss', 'cost'), builder='device'), **kw))
