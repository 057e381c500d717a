"""Preconditions of the resident-history scenarios (tests/history_cases.py), on
the host: the GPU tests of tests/test_history_gpu.py cannot pass vacuously --
the named counts are crossed one trial at a time, the staged totals sit on the
sort switch, ties straddle the split, every kind meets equal keys across an
append, both signed zeros meet each other from both sides, and the model's
sorted view is the lexicographic (value, arrival) order.  These are
conditions of the chosen seeds, not measurements."""
import numpy as np
import pytest

from tests import history_cases as C
from tests.history_reference import PoolModel


def _replay(scn):
    """(model, step index, step) after each append."""
    m = PoolModel(scn.labels)
    for k, st in enumerate(scn.steps):
        before = [m.val[l].copy() for l in range(len(scn.labels))]
        m.append(st.n_new, st.trial, st.val, st.raw)
        yield m, k, st, before


@pytest.fixture(scope='module')
def stepwise():
    return C.stepwise()


def test_label_set():
    names = [n for n, _, _ in C.LABELS]
    kinds = {k for _, k, _ in C.LABELS}
    assert len(kinds) == 10 and len(names) == len(set(names)) == 14
    # the zero-width regions lie between populated neighbours
    for name in ('late', 'never'):
        i = C.index_of(C.LABELS, name)
        assert 0 < i < len(names) - 1 and names[i - 1] not in ('late', 'never') \
            and names[i + 1] not in ('late', 'never')


def test_stepwise_crosses_regrows_one_trial_at_a_time(stepwise):
    ie = C.index_of(C.LABELS, 'every')
    caps = C.capacities(stepwise)
    counts = [c[0][ie] for c in caps]
    assert all(int(st.n_new[ie]) == 1 for st in stepwise.steps)
    for a, b in ((256, 257), (514, 515)):
        k = counts.index(b)
        assert counts[k - 1] == a and caps[k - 1][1][ie] == a and caps[k][1][ie] == 2 * b
        assert k in C.regrow_steps(stepwise)
    assert counts[-1] > 515 + 2
    ir, il, inv = (C.index_of(C.LABELS, n) for n in ('rare', 'late', 'never'))
    assert 0 < caps[-1][0][ir] <= 256 and caps[-1][1][ir] == 256          # never leaves 256
    assert caps[-1][0][inv] == 0 and caps[-1][1][inv] == 0               # never observed
    first = next(k for k, c in enumerate(caps) if c[0][il] > 0)
    assert len(stepwise.steps[first].losses) > C.LATE_FIRST               # zero-width for 300 trials
    assert all(c[1][il] == 0 for c in caps[:first])
    # most labels get nothing at most steps
    zero = np.mean([[int(st.n_new[l]) == 0 for l in range(len(C.LABELS))] for st in stepwise.steps], axis=0)
    assert zero[ir] > 0.9 and np.sum(zero > 0.3) >= 10
    # orphans and NaN-loss trials are there
    assert sum(int((st.trial < 0).sum()) for st in stepwise.steps) >= 6
    assert np.isnan(stepwise.steps[-1].losses).sum() == len(C.STEPWISE_NAN)


def test_stepwise_checked_steps_cover_split_changes(stepwise):
    chk = C.oracle_steps(stepwise)
    steps = stepwise.steps
    assert all(k in chk for k in range(80))
    for r in C.regrow_steps(stepwise):
        assert all(k in chk for k in range(max(r - 2, 0), min(r + 3, len(steps))))
    assert any(C.split_tie(steps[k].losses) for k in chk)                 # a loss tie straddles the split
    assert any(C.n_below_of(steps[k].losses) != C.n_below_of(steps[k - 1].losses) for k in chk if k)
    assert len(chk) < 0.45 * len(steps)


def test_stepwise_pending_turns_finite(stepwise):
    """A pending trial turns finite and enters the below set (another stays
    above), at a checked step."""
    from hyperopt_amd import posterior as P
    chk = set(C.oracle_steps(stepwise))
    entered = stayed = 0
    for t, (v, r) in C.STEPWISE_PENDING.items():
        k = r - 1                                     # the step with r trials
        prev, now = stepwise.steps[k - 1].losses, stepwise.steps[k].losses
        assert len(now) == r and np.isinf(prev[t]) and now[t] == v and k in chk
        below = P.reference_orders(now, C.n_below_of(now), _NoObs(), ())[0]
        entered += int(below[t] == 1)
        stayed += int(below[t] == 0)
    assert entered >= 1 and stayed >= 1


class _NoObs(object):
    n_labels = 0


def test_stepwise_equal_keys_and_signed_zeros_across_appends(stepwise):
    dup = set()
    zeros = set()     # (sign of an old zero, sign of a new zero)
    for m, k, st, before in _replay(stepwise):
        for l, (name, kind, _) in enumerate(C.LABELS):
            _, new, _ = st.part(l)
            if len(new) and len(before[l]) and np.isin(new, before[l]).any():
                dup.add(kind)
            oz, nz = before[l][before[l] == 0], new[new == 0]
            for a in oz:
                for b in nz:
                    zeros.add((bool(np.signbit(a)), bool(np.signbit(b))))
    assert dup == {k for _, k, _ in C.LABELS}
    assert (False, True) in zeros and (True, False) in zeros            # +0 meets -0, and the reverse


@pytest.mark.parametrize('total', [4095, 4096, 4097])
def test_threshold_totals(total):
    scn = C.threshold(total)
    assert C.GLOBAL_SORT_MIN == 4096
    assert int(scn.steps[0].n_new.sum()) == total
    assert np.count_nonzero(scn.steps[0].n_new) >= 10                    # over several labels
    assert 0 < int(scn.steps[1].n_new.sum()) < 64
    qn = C.index_of(C.LABELS, 'qn')
    v = scn.steps[0].part(qn)[1]
    z = v[v == 0]
    assert np.signbit(z).any() and not np.signbit(z).all()               # both zeros inside the sorted batch


def test_merge_edges_batches():
    scn = C.merge_edges()
    ie = C.index_of(C.LABELS, 'every')
    reps = list(_replay(scn))
    assert len(reps) == 7 and int(scn.steps[0].n_new[ie]) == C.MERGE_BASE
    new = [st.part(ie)[1] for _, _, st, _ in reps]
    old = [b[ie] for _, _, _, b in reps]
    assert new[1].max() < old[1].min() and len(set(new[1])) < len(new[1])
    assert new[2].min() > old[2].max()
    assert len(set(new[3])) == 1 and np.count_nonzero(old[3] == new[3][0]) >= 2
    both = np.intersect1d(new[4], old[4])
    assert len(both) >= 3 and len(set(new[4])) < len(new[4]) and old[4].min() < new[4].min() \
        and new[4].max() < old[4].max()
    z = new[4][new[4] == 0]
    assert list(np.signbit(z)) == [False, True, False]
    kinds = [C.LABELS[l][1] for l in np.flatnonzero(scn.steps[5].n_new)]
    assert kinds and all(k in ('randint', 'categorical') for k in kinds)
    assert int(scn.steps[6].n_new.sum()) == 0


def test_lone_regrow_shape():
    scn = C.lone_regrow()
    il = C.index_of(C.LABELS, C.LONE)
    caps = C.capacities(scn)
    assert len(scn.steps) == 3
    assert caps[1][0][il] == 200 and caps[2][0][il] == 300
    assert caps[1][1][il] == 256 and caps[2][1][il] == 600
    assert [l for l in range(len(C.LABELS)) if scn.steps[2].n_new[l]] == [il]
    for l in range(len(C.LABELS)):
        if l != il:
            assert caps[1][1][l] == caps[2][1][l] and caps[1][0][l] == caps[2][0][l]
    assert sum(1 for c in caps[1][1] if c > 256) >= 1                    # a neighbour past its first capacity
    assert sum(1 for c in caps[1][1] if c == 0) >= 1                     # a zero-width region in the layout


@pytest.mark.parametrize('make', [C.stepwise, C.merge_edges, C.lone_regrow, lambda: C.threshold(4096),
                                  lambda: C.short(C.LABELS[:5], 31), lambda: C.short(C.LABELS + C.EXTRA, 32)])
def test_model_sorted_view_is_lexsort(make):
    scn = make()
    for m, k, st, _ in _replay(scn):
        if k % 16 and k != len(scn.steps) - 1:
            continue
        for l in range(len(scn.labels)):
            view = m.sorted_view(l)
            if m.is_categorical(l):
                assert view is None
                continue
            idx, key = view
            v = m.val[l]
            assert np.array_equal(idx, np.lexsort((np.arange(len(v)), v)))
            assert np.array_equal(key.view(np.uint64), v[idx].view(np.uint64))
            assert not np.isnan(v).any() and not np.isneginf(v).any()
        # trial positions: one observation per trial and label, in order
        for l in range(len(scn.labels)):
            t = m.trial[l][m.trial[l] >= 0]
            assert np.all(np.diff(t) > 0) and (len(t) == 0 or t[-1] < len(st.losses))


def test_model_mixtures_run_on_host(stepwise):
    """The expected mixtures come from the CPU oracle in both orders."""
    m = PoolModel(C.LABELS)
    for st in stepwise.steps[:120]:
        m.append(st.n_new, st.trial, st.val, st.raw)
    h, stable = m.mixtures(st.losses, 'stable')
    _, default = m.mixtures(st.losses, None)
    assert len(stable) == len(default) == len(C.LABELS)
    assert len(h.tids) == int(np.count_nonzero(st.losses == st.losses))
    inv = C.index_of(C.LABELS, 'never')
    assert len(stable[inv][0][0]) == 1 and len(stable[inv][1][0]) == 1   # the prior alone
