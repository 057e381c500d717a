"""The cell check and the shapes of tests/test_value_only_edges_gpu.py,
without a GPU: check_cells on synthetic score arrays (so that the GPU test's
verdicts are not vacuous), and every shape on the side of kWinMinN = 8192
slots -- and of the packed map's C < kTile -- it is meant to be on."""
import numpy as np

from tests import bx_cases as C
from tests import value_only_cases as V
from tests.bx_reference import LD


def _one(scores, index, decided):
    skipped, fails = V.check_cells(np.asarray([scores], dtype=LD), [index], [decided])
    return bool(skipped[0]), [f[1] for f in fails]


def test_clear_winner_passes_decided_or_not():
    s = [0.0, 1.0, 3.0, 2.5]
    assert _one(s, 2, True) == (False, [])
    assert _one(s, 2, False) == (False, [])


def test_wrong_winner_fails_decided_or_not():
    s = [0.0, 1.0, 3.0, 2.5]
    for decided in (False, True):
        skipped, what = _one(s, 3, decided)
        assert not skipped and what == ['winner below the exact best']
    # the report names both candidates
    _, fails = V.check_cells(np.asarray([s], dtype=LD), [3], [True])
    assert fails[0][2] == 3 and fails[0][4] == 2 and fails[0][3] == 2.5 and fails[0][5] == 3.0


def test_tie_may_be_picked_but_not_decided():
    s = [1.0, 7.0, 7.0, -2.0]
    for w in (1, 2):     # either of the tied candidates is within the winner's bar
        assert _one(s, w, False) == (False, [])
        assert _one(s, w, True) == (False, ['decided without the exact lead'])


def test_near_tie_inside_and_outside_the_margin():
    # a lead below half of kValueMargin (relative to max(1, |s|)) may not be decided
    for top, lead, ok in ((1.0, 0.4e-9, False), (1.0, 0.6e-9, True), (100.0, 0.6e-9, False),
                          (100.0, 0.6e-7, True), (-100.0, 0.4e-7, False), (0.0, 0.6e-9, True)):
        s = np.array([LD(top), LD(top) - LD(lead), LD(top) - LD(5)], dtype=LD)
        assert _one(s, 0, False) == (False, [])
        assert _one(s, 0, True) == (False, [] if ok else ['decided without the exact lead']), (top, lead)
    # the runner-up within 1e-9 is an acceptable winner, past it is not
    s = np.array([LD(1), LD(1) - LD(0.5e-9), LD(1) - LD(2e-9)], dtype=LD)
    assert _one(s, 1, False) == (False, [])
    assert _one(s, 2, False) == (False, ['winner below the exact best'])
    # (long double: a lead of 1e-12 is seen, where fp64 at |s| = 1e4 would not hold it)
    s = np.array([LD(1e4), LD(1e4) - LD(1e-13)], dtype=LD)
    assert _one(s, 0, True) == (False, ['decided without the exact lead'])
    assert _one(s, 1, False) == (False, [])


def test_non_finite_candidate_skips_the_cell_only():
    for bad in (np.nan, -np.inf, np.inf):
        assert _one([0.0, bad, 3.0], 0, True) == (True, [])
    s = np.asarray([[0.0, np.nan, 3.0], [0.0, 1.0, 3.0], [0.0, 1.0, 3.0]], dtype=LD)
    skipped, fails = V.check_cells(s, [0, 0, 2], [True, False, True])
    assert skipped.tolist() == [True, False, False]
    assert [(f[0], f[1]) for f in fails] == [(1, 'winner below the exact best')]


def test_one_candidate_rounds():
    s = np.asarray([[2.5], [-1e300], [np.nan]], dtype=LD)
    skipped, fails = V.check_cells(s, [0, 0, 0], [True, False, True])
    assert skipped.tolist() == [False, False, True] and fails == []
    _, fails = V.check_cells(s[:1], [1], [True])
    assert [f[1] for f in fails] == ['index out of range']


def test_index_out_of_range_fails():
    assert _one([0.0, 1.0], 2, False) == (False, ['index out of range'])
    assert _one([0.0, 1.0], -1, True) == (False, ['index out of range'])


def test_shapes_are_on_the_intended_side_of_the_threshold():
    ids = V.default_ids()
    assert len(ids) == V.N_ROUNDS == 352 and len(set(ids)) == 352
    assert ids[:350] == list(range(350)) and tuple(ids[-2:]) == (7 + 2 ** 20, 2 ** 31 - 1)
    assert max(ids) < 2 ** 32      # (rounds travel as uint32)
    # just past kWinMinN, the second workgroup of k_pick_win partial, the
    # expansion screen's slot map (kBxR x kBlock slots: 42 rounds of 24) ending mid-workgroup
    assert V.N_ROUNDS * V.C_DEFAULT == 8448 >= V.K_WIN_MIN_N > (V.N_ROUNDS - 11) * V.C_DEFAULT
    assert V.K_BLOCK < V.N_ROUNDS < 2 * V.K_BLOCK and V.N_ROUNDS % V.K_BLOCK != 0
    assert V.N_ROUNDS % ((V.K_BX_R * V.K_BLOCK) // V.C_DEFAULT) != 0
    # one round short of it
    assert V.N_BELOW_THRESHOLD * V.C_DEFAULT == 8184 < V.K_WIN_MIN_N <= (V.N_BELOW_THRESHOLD + 1) * V.C_DEFAULT
    assert V.COUNTS == [1, 2, 33, 256, 257, 1024]
    for n_cand in V.COUNTS + [V.K_TILE - 1]:
        n = V.rounds_for(n_cand)
        assert n == -(-8192 // n_cand) + 3
        assert (n - 3) * n_cand >= V.K_WIN_MIN_N > (n - 4) * n_cand
        assert len(V.default_ids(n)) == n
    # the packed map (k_pick_win) up to C = 1023; C = 1024 = kBxR x kBlock is the tile map's first size
    assert V.K_TILE == V.K_BX_R * V.K_BLOCK == 1024
    assert [c for c in V.COUNTS if c >= V.K_TILE] == [1024]
    assert V.N_CHECKED_OVER_UNCLIPPED + 2 <= V.N_ROUNDS


def test_cases_are_the_edge_posteriors():
    """19 cases, 16 with an index; the product's first posteriors (1 to 3
    below components) are among them."""
    assert len(C.CASES) == 19 and len(C.ELIGIBLE) == 16
    assert set(C.INELIGIBLE) == {'over_bins', 'over_unclipped', 'permuted'}
    assert len(C.posts('uniform3')[0].below[0]) <= 3
    assert len(C.posts('over_unclipped')[0].above[0]) == 16386
    assert len(C.dense_labels(C.posts('three_labels'))) == 3
    assert V.DECIDED_GAP == 0.5e-9 and V.WINNER_BAR == 1e-9 and V.MAX_SKIPPED == 0.01
