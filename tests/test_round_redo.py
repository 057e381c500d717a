"""The statistics a round reports after it ran again.  A round has two redo
paths: the hot-bin prefilter's fallback (the dense families run again with
every candidate through the expansion screen; the quantized and categorical
labels' part stays the first run's) and the packed re-score's plan overflow
(the whole round runs again with larger buffers).  Either way the caller
must see the bytes AND the statistics of a round that took the plain path
at once: evaluations, draw counts, screen counts, per-family evaluations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LABELS = 8            # uniform, loguniform, quniform, normal, randint, uniform, loguniform, quniform
N_TILE = 8192           # the smallest round the expansion screen and the prefilter take (kWinMinN)
SIDE_FREE = 31 & ~16    # a family mask without the categorical labels


@pytest.fixture(scope='module')
def eng():
    from hyperopt_amd import posterior as P
    from hyperopt_amd.engine import Engine
    from hyperopt_amd.workloads import mixed_history
    e = Engine(0, 'f64')
    e.set_posterior(*P.pack(mixed_history(N_LABELS, 300, seed=3).posteriors()))
    yield e
    e.close()


def _stats(eng):
    return {'screen_mode': eng.last_screen_mode(), 'drawn': eng.last_drawn(), 'evals': eng.last_evals(),
            'mode_evals': {m: v[1] for m, v in eng.last_mode_stats().items()}, 'screen': eng.last_screen(),
            'rescore_terms': eng.last_rescore_terms()}


def _run(eng, fn, **opts):
    """fn() under the options; (bytes, statistics, last_hot)."""
    for k, v in opts.items():
        eng.set_option(k, v)
    out = fn()
    return np.ascontiguousarray(out).tobytes(), _stats(eng), eng.last_hot()


@pytest.fixture()
def tile_defaults(eng):
    yield
    for k, v in (('hot', 1), ('hot_div', 16), ('mode_mask', 31)):
        eng.set_option(k, v)


def test_hot_fallback_reports_the_plain_rounds_statistics(eng, tile_defaults):
    fn = lambda: eng.suggest(21, N_TILE, round=4)
    plain, st_plain, hot_plain = _run(eng, fn, hot=0)
    fell, st_fell, hot_fell = _run(eng, fn, hot=2)
    print('hot=0: %s %s\nhot=2: %s %s' % (st_plain, hot_plain, st_fell, hot_fell))
    assert fell == plain
    assert st_plain['screen_mode'] == 3 and st_fell['screen_mode'] == 3
    for key in ('drawn', 'evals', 'mode_evals', 'screen'):
        assert st_fell[key] == st_plain[key], key
    assert hot_plain == (-1, 0)
    assert hot_fell[0] >= 0 and hot_fell[1] == 1, hot_fell
    again, st_again, hot_again = _run(eng, fn, hot=1)
    assert again == plain
    assert hot_again[1] == 0, hot_again


@pytest.mark.parametrize('n', [N_TILE, 1 << 22])
def test_hot_list_overflow_reports_the_plain_rounds_statistics(eng, tile_defaults, n):
    """Lists as short as they get (hot_div 2^20).  A round of 8192
    candidates still fits them (a list never holds fewer than 4096); 2^22
    candidates overflow them, and the round falls back (flag bit 2)."""
    fn = lambda: eng.suggest(21, n, round=4)
    plain, st_plain, _ = _run(eng, fn, hot=0)
    over, st_over, hot_over = _run(eng, fn, hot=1, hot_div=1 << 20)
    print('n %d, hot_div 2^20: %s %s' % (n, st_over, hot_over))
    assert over == plain
    assert hot_over[0] >= 0 and (hot_over[1] & 2 if n > N_TILE else hot_over[1] == 0), hot_over
    for key in ('screen_mode', 'drawn', 'evals', 'mode_evals', 'screen'):
        assert st_over[key] == st_plain[key], key


def test_mode_mask_survives_a_fallback_round(eng, tile_defaults):
    """The fallback runs the dense families alone; the caller's family mask
    is what the rounds after it launch."""
    fn = lambda: eng.suggest(22, N_TILE, round=6)
    _, st_whole, _ = _run(eng, fn, hot=0)
    _, st_masked, _ = _run(eng, fn, hot=0, mode_mask=SIDE_FREE)
    assert st_masked['evals'] < st_whole['evals'] and st_masked['drawn'][1] == 0
    _, st_fell, hot_fell = _run(eng, fn, hot=2)
    assert hot_fell[1] == 1
    assert st_fell['evals'] == st_masked['evals'] and st_fell['drawn'] == st_masked['drawn']
    for hot in (2, 1, 0):   # the rounds after a fallback round: still the masked round
        _, st_after, _ = _run(eng, fn, hot=hot)
        assert st_after['evals'] == st_masked['evals'], hot
        assert st_after['drawn'] == st_masked['drawn'], hot
    eng.set_option('mode_mask', 31)
    _, st_back, _ = _run(eng, fn, hot=0)
    assert st_back['evals'] == st_whole['evals'] and st_back['drawn'] == st_whole['drawn']


@pytest.mark.parametrize('value_only', [0, 1])
def test_plan_overflow_reports_the_roomy_rounds_statistics(eng, value_only):
    """128 rounds of 24 candidates: 3072 slots per label, past the split-K
    map's 2048, below one tile per round (the packed map)."""
    ids = list(range(500, 628))
    fn = lambda: eng.suggest_batch(31, ids, 24)
    eng.set_option('value_only', value_only)
    try:
        roomy, st_roomy, _ = _run(eng, fn, rescore_cap=1 << 20)
        over, st_over, _ = _run(eng, fn, rescore_cap=1)
        grown, st_grown, _ = _run(eng, fn)   # (the grown buffers, no second run)
    finally:
        eng.set_option('value_only', 0)
        eng.set_option('rescore_cap', 1 << 16)
    print('roomy: %s\nover:  %s\ngrown: %s' % (st_roomy, st_over, st_grown))
    assert over == roomy and grown == roomy
    for st in (st_over, st_grown):
        for key in ('evals', 'screen', 'rescore_terms', 'drawn', 'mode_evals'):
            assert st[key] == st_roomy[key], key
