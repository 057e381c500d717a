"""The host side of the draw on a candidate pool (tpe_pool_draw,
tpe.suggest(pool=..., pool_candidates=m)): the numpy reference of
tests/pool_draw_reference.py -- its bit layout, the softmax law of the
Gumbel keys, its identity with the ranking when everything is drawn -- and the
keyword's early errors.  No GPU is touched."""
import numpy as np
import pytest

from hyperopt_amd import Trials, _lib, tpe
from hyperopt_amd.base import Domain
from tests import pool_draw_reference as D
from tests import pool_reference as R
from tests.test_pool_host import loss, points, space


def test_stream_is_the_first_below_the_joint_pick_streams():
    assert D.TPE_POOL_STREAM == _lib.TPE_POOL_STREAM == _lib.TPE_JOINT_STREAM - _lib.TPE_JOINT_MAX_GROUPS


def test_uniform_bit_layout():
    M = 0xFFFFFFFF
    cases = [(0, 0), (M, M), (0, M), (M, 0), (1, 0), (0, 1 << 12), (0, (1 << 12) - 1), (0x80000000, 0),
             (0x12345678, 0x9ABCDEF0), (0xDEADBEEF, 0x00000FFF)]
    w0 = np.asarray([a for a, _ in cases], dtype=np.uint64)
    w1 = np.asarray([b for _, b in cases], dtype=np.uint64)
    u = D.uniform(w0, w1)
    for (a, b), got in zip(cases, u):
        t = (a << 20) | (b >> 12)                 # Python integers: 52 bits
        assert 0 <= t < 1 << 52
        num = 2 * t + 1                           # u = (2 t + 1) / 2^53, exactly
        assert float(got).as_integer_ratio() == (num // (num & -num), (1 << 53) // (num & -num))
        assert 0.0 < got < 1.0
    assert u[0] == 2.0 ** -53 and u[1] == 1.0 - 2.0 ** -53
    # the words of real counters: inside (0, 1), and the noise finite
    w = D.words(7, 3, np.arange(5000))
    uu = D.uniform(*w)
    assert (uu > 0).all() and (uu < 1).all() and np.isfinite(D.gumbel(7, 3, 5000)).all()
    # a key's noise depends on (seed, round, entry) alone
    assert np.array_equal(D.gumbel(7, 3, 100), D.gumbel(7, 3, 5000)[:100])
    assert not np.array_equal(D.gumbel(7, 3, 100), D.gumbel(7, 4, 100))
    assert not np.array_equal(D.gumbel(7, 3, 100), D.gumbel(8, 3, 100))
    assert not np.array_equal(D.gumbel(7, 3, 100), D.gumbel(7 + (1 << 32), 3, 100))


@pytest.mark.parametrize('seed', (1, 2, 3))
def test_one_draw_follows_softmax(seed):
    """m = 1 with replacement: P(i) = l_i / sum l.  4096 rounds on 8 weights,
    every frequency within 5 binomial standard deviations (the reference
    measured on these inputs: max |z| between 1.31 and 1.65, smallest top-two
    key gap 3.6e-6)."""
    n, rounds = 8, 4096
    ls = np.random.RandomState(0).normal(0, 1.5, n)
    p = np.exp(ls - ls.max())
    p /= p.sum()
    keys = np.stack([ls + D.gumbel(seed, r, n) for r in range(rounds)])
    best, drawn = D.draw(keys, np.zeros(n), 1, distinct=False)
    assert len(best) == rounds and all(len(d) == 1 and d[0] == b for d, b in zip(drawn, best))
    assert best.tolist() == np.argmax(keys, axis=1).tolist()
    freq = np.bincount(best, minlength=n) / rounds
    z = (freq - p) / np.sqrt(p * (1 - p) / rounds)
    assert np.abs(z).max() <= 5.0, z


def test_pool_sized_draw_is_the_ranking():
    rng = np.random.RandomState(4)
    for n, taken in ((1, ()), (9, ()), (40, (3, 17, 17, 39, -2, 400))):
        score = rng.choice([-np.inf, -1.0, 0.0, 0.5, 0.5, 2.0, np.inf, np.nan], size=n)
        ls = rng.normal(0, 2, n)
        ls[::5] = -np.inf
        keys = np.stack([ls + D.gumbel(5, r, n) for r in range(n + 2)])
        for m in (n, n + 5):
            best, drawn = D.draw(keys, score, m, taken=taken, distinct=True)
            assert best.tolist() == R.rank(score, n + 2, taken=taken).tolist()
            free = n - len(set(t for t in taken if 0 <= t < n))
            assert [len(d) for d in drawn] == list(range(free, 0, -1))


def test_reference_selection_order():
    inf, nan = np.inf, np.nan
    keys = np.asarray([1.0, nan, 3.0, 3.0, -inf, 2.0, -inf])
    assert D.select(keys, 7, range(7)).tolist() == [1, 2, 3, 5, 0, 4, 6]
    assert D.select(keys, 2, [0, 3, 4, 6]).tolist() == [3, 0]
    # an entry with l = 0 is drawn only when the finite keys run out
    score = np.asarray([0.0, 0.0, 0.0, 0.0, 9.0, 0.0, 9.0])
    best, drawn = D.draw(keys[None], score, 4, taken=[1])
    assert drawn[0].tolist() == [2, 3, 5, 0] and best.tolist() == [0]
    best, drawn = D.draw(keys[None], score, 5, taken=[1])
    assert drawn[0].tolist() == [2, 3, 5, 0, 4] and best.tolist() == [4]


def test_keyword_errors_touch_no_engine(monkeypatch):
    from hyperopt_amd import engine
    monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    domain = Domain(loss, space())
    pool = tpe.Pool(domain, points(5))
    trials = Trials()
    with pytest.raises(ValueError, match='needs a pool'):
        tpe.suggest([0], domain, trials, 1, pool_candidates=4)
    for bad in (True, False, 2.0, '3', [3], 0, -1, np.float64(3.0)):
        with pytest.raises(ValueError, match='pool_candidates'):
            tpe.suggest([0], domain, trials, 1, pool=pool, pool_candidates=bad, n_startup_jobs=0)
        with pytest.raises(ValueError, match='pool_candidates'):
            tpe.suggest([0], domain, trials, 1, pool=pool, pool_candidates=bad, objectives=('loss', 'x'))
    # the startup phase is the pool's own, with the keyword or without
    a = tpe.suggest([0, 1], domain, trials, 1, pool=pool, pool_candidates=np.int64(3))
    assert a == tpe.suggest([0, 1], domain, trials, 1, pool=pool) and len(a) == 2


def test_none_is_not_handed_on(monkeypatch):
    from hyperopt_amd import engine
    monkeypatch.setattr(engine, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    domain = Domain(loss, space())
    pool = tpe.Pool(domain, points(5))
    seen = []
    real = tpe.suggest
    monkeypatch.setattr(tpe, 'suggest', lambda *a, **k: seen.append(k) or [])
    kw = dict(pool=pool, batch='pending', n_startup_jobs=0, posterior_builder='host')
    real([0, 1], domain, Trials(), 1, **kw)
    real([0, 1], domain, Trials(), 1, pool_candidates=None, **kw)
    assert len(seen) == 4 and all('pool_candidates' not in k and k['pool'] is pool for k in seen)
    del seen[:]
    real([0, 1], domain, Trials(), 1, pool_candidates=3, **kw)
    assert len(seen) == 2 and all(k['pool_candidates'] == 3 for k in seen)
