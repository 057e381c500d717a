"""Joint groups of conditional spaces, host side (CPU): condition signatures
and the (slot, labels) groups of a nested conditional space and of the
reference's own graph, stable slots, the joint mixtures of conditional groups
against the univariate posteriors, the error of group=True without
multivariate=True, and -- through the fp64 draw port -- that the seed and
rounds test_joint_groups_gpu.py uses exclude no draw and leave every winner a
clear margin under each slot's own pick stream."""
import logging

import numpy as np
import pytest

from hyperopt_amd import labels as LB, posterior as P, tpe, workloads
from hyperopt_amd.base import Domain, Trials
from tests import joint_cases as JC
from tests import joint_group_cases as GC


# -- signatures and groups ---------------------------------------------------------
def test_condition_signatures_nested_space():
    domain = Domain(GC.loss, GC.space())
    sigs = LB.condition_signatures(domain.expr)
    assert LB.UNCONDITIONAL == GC.UNCONDITIONAL
    assert sigs == GC.SIGNATURES
    free = {k for k, s in sigs.items() if s == LB.UNCONDITIONAL}
    assert free == LB.unconditional_labels(domain.expr) == {'x', 'ly', 'c', 'k'}
    specs = tpe.specs_of(domain)
    assert set(specs) == set(sigs)
    assert tpe.joint_groups(domain, specs) == GC.GROUPS
    # the existing single group is slot 0's
    assert tpe.joint_group(domain, specs) == GC.GROUPS[0][1]


def test_condition_signatures_reference_graph():
    """On the reference's own pyll graph (tests/golden/reference_domain_graph.json):
    a: choice [{u}, {v: qloguniform}], k: pchoice, n: qnormal."""
    from tests.test_api import _reference_expr
    expr = _reference_expr()
    sigs = LB.condition_signatures(expr)
    assert sigs == {'a': LB.UNCONDITIONAL, 'k': LB.UNCONDITIONAL, 'n': LB.UNCONDITIONAL,
                    'u': frozenset([frozenset([('a', 0)])]), 'v': frozenset([frozenset([('a', 1)])])}
    assert {k for k, s in sigs.items() if s == LB.UNCONDITIONAL} == LB.unconditional_labels(expr)

    class _D(object):
        pass
    domain = _D()
    domain.expr = expr
    # one dense label per signature: no group
    assert tpe.joint_groups(domain, LB.compile_space(expr)) == []


def _obs_for(groups, odd=None):
    obs = {}
    for j, (_, g) in enumerate(groups):
        for k in g:
            obs[k] = (np.arange(5) + 10 * j, np.ones(5))
    if odd:
        obs[odd] = (obs[odd][0][1:], obs[odd][1][1:])
    return obs


def test_slots_are_stable(caplog):
    domain = Domain(GC.loss, GC.space())
    specs = tpe.specs_of(domain)
    assert tpe.joint_groups(domain, specs, _obs_for(GC.GROUPS)) == GC.GROUPS
    with caplog.at_level(logging.INFO, logger='hyperopt_amd.tpe'):
        got = tpe.joint_groups(domain, specs, _obs_for(GC.GROUPS, odd='b'))
    assert got == [GC.GROUPS[0], GC.GROUPS[2]]
    msgs = [r.message for r in caplog.records if 'different trials' in r.message]
    assert len(msgs) == 1 and "'a'" in msgs[0] and "'b'" in msgs[0]


# -- conditional group mixtures ---------------------------------------------------
def _sorted_rows(w, mu, s):
    order = np.lexsort((w, s, mu))
    return np.asarray(w)[order], np.asarray(mu)[order], np.asarray(s)[order]


def _check_group(group, obs, splitter, want_kb):
    """Per dimension (mu, sigma) of the joint components are the univariate
    label_posterior's, bit for bit; the weights by test_joint_host.py's rule:
    bit-identical for the first label and wherever a side has no ramp (n_S <=
    25), else equal to the rounding of two sums of K terms."""
    m = P.joint_mixture(group, obs, splitter, 1.0)
    wb, mub, sigb, wa, mua, siga = m.wb, m.mub, m.sigb, m.wa, m.mua, m.siga
    assert len(wb) == want_kb
    for d, (label, kind, args) in enumerate(group):
        b, a = splitter.split(*obs[label])
        post = P.label_posterior(label, kind, args, b, a, 1.0)
        for (W, mu, s), (w1, m1, s1) in (((wb, mub, sigb), post.below), ((wa, mua, siga), post.above)):
            assert len(W) == len(w1)
            gw, gm, gs = _sorted_rows(W, mu[:, d], s[:, d])
            ew, em, es = _sorted_rows(w1, m1, s1)
            assert np.array_equal(gm, em) and np.array_equal(gs, es), (label, 'mu / sigma')
            if d == 0 or len(W) - 1 <= P.DEFAULT_LF:
                assert np.array_equal(gw, ew), (label, 'weights')
            else:
                assert np.all(np.abs(gw - ew) <= 2 * len(W) * 2.0 ** -53 * ew), (label, 'weights')
    return wb, mub, sigb, wa, mua, siga


def test_conditional_group_mixtures():
    hist = workloads.conditional_history(400)
    by = {n: (n, k, a) for n, k, a in hist.labels}
    splitter = P.Splitter(hist.tids, hist.losses, 0.25)
    # the svm branch holds all 5 below trials
    _check_group([by['svm_C'], by['svm_gamma']], hist.obs, splitter, 6)
    # the gbm branch none: its below side is the prior alone
    wb, mub, sigb, wa, _, _ = _check_group([by['gbm_lr'], by['gbm_subsample']], hist.obs, splitter, 1)
    assert wb.tolist() == [1.0] and len(wa) > 26
    lo, hi = by['gbm_subsample'][2]['low'], by['gbm_subsample'][2]['high']
    assert mub[0, 1] == 0.5 * (lo + hi) and sigb[0, 1] == hi - lo
    # a group never observed: the prior alone on both sides, the same records
    obs = dict(hist.obs)
    for k in ('gbm_lr', 'gbm_subsample'):
        obs[k] = (np.zeros(0, dtype=np.int64), np.zeros(0))
    wb, mub, sigb, wa, mua, siga = _check_group([by['gbm_lr'], by['gbm_subsample']], obs, splitter, 1)
    assert wa.tolist() == [1.0] and np.array_equal(mub, mua) and np.array_equal(sigb, siga)


# -- seeds ---------------------------------------------------------------------------
@pytest.mark.parametrize('slot', range(len(GC.SLOTS)))
def test_committed_seed_excludes_nothing_and_leaves_margins(slot):
    """Every (round, n) cell of the batched GPU test, under the slot's own
    pick stream: no draw excluded, the winner's margin above 1e-9 (|ll| +
    |lg|).  The candidates of n are the first n of the round's 300."""
    ref = JC.group(GC.SLOTS[slot])
    for rnd in sorted(set(GC.ROUNDS)):
        _, vals, excl = GC.port_draw(ref, GC.SEED, rnd, np.arange(max(GC.COUNTS), dtype=np.uint64),
                                     GC.pick_stream(slot))
        assert not excl.any(), (slot, rnd)
        ll, lg = ref.joint_lpdf(vals, 'below'), ref.joint_lpdf(vals, 'above')
        for n in GC.COUNTS:
            ok, _ = JC.margin_ok(ll[:n], lg[:n])
            assert ok, 'slot %d round %d n %d: pick another seed' % (slot, rnd, n)


# -- errors --------------------------------------------------------------------------
def test_group_needs_multivariate():
    domain = Domain(GC.loss, GC.space())
    with pytest.raises(ValueError):
        tpe.suggest([0], domain, Trials(), 0, group=True)
    with pytest.raises(ValueError):
        tpe.suggest([0], domain, Trials(), 0, multivariate=False, group=True)
