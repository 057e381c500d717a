"""Host-side drop-in API (CPU): spaces, Trials, fmin with random search, the
history gather and per-label split against the reference's own suggest
(tests/golden/suggest_history.npz), and the label compiler."""
import json
import os

import numpy as np
import pytest

import hyperopt_amd as H
from hyperopt_amd import hp, labels as LB, posterior as P, rand, tpe
from hyperopt_amd.base import Domain, Trials, trials_from_docs
from oracle import tpe_oracle as O
from tests import golden_io


def many_dists():
    return {'a': hp.choice('a', [0, 1, 2]), 'b': hp.randint('b', 10),
            'c': hp.uniform('c', 4, 7), 'd': hp.loguniform('d', -2, 0),
            'e': hp.quniform('e', 0, 10, 3), 'f': hp.qloguniform('f', 0, 3, 2),
            'g': hp.normal('g', 4, 7), 'h': hp.lognormal('h', -2, 2),
            'i': hp.qnormal('i', 0, 10, 2), 'j': hp.qlognormal('j', 0, 2, 1),
            'k': hp.pchoice('k', [(.1, 0), (.9, 1)])}


def conditional():
    return {'clf': hp.choice('clf', [
        {'type': 'svm', 'C': hp.loguniform('svm_C', -5, 5),
         'kernel': hp.choice('svm_kernel', [
             {'k': 'rbf', 'gamma': hp.loguniform('svm_gamma', -8, 2)},
             {'k': 'poly', 'degree': hp.quniform('svm_degree', 2, 5, 1)}])},
        {'type': 'rf', 'n': hp.qloguniform('rf_n', np.log(10), np.log(1000), 1),
         'depth': hp.quniform('rf_depth', 1, 30, 1), 'feat': hp.uniform('rf_feat', .1, 1)},
    ]), 'lr': hp.normal('lr', 0, 1)}


SPACES = {'many_dists': many_dists, 'conditional': conditional}


def _trials_from_json(docs):
    full = []
    for d in docs:
        d = dict(d)
        d.setdefault('spec', None)
        d.setdefault('exp_key', None)
        d.setdefault('owner', None)
        d.setdefault('book_time', None)
        d.setdefault('refresh_time', None)
        d['misc'] = dict(d['misc'], cmd=None)
        full.append(d)
    return trials_from_docs(full, validate=False)


@pytest.mark.parametrize('name', ['many_dists', 'conditional'])
def test_gather_and_split_match_reference_suggest(name):
    z, meta = golden_io.load('suggest_history.npz')
    m = meta[name]
    trials = _trials_from_json(m['docs'])
    domain = Domain(lambda d: 0.0, SPACES[name]())
    specs = tpe.specs_of(domain)
    assert set(m['labels']) <= set(specs)
    from hyperopt_amd import history
    tids, losses, obs = history.gather(domain, trials, list(specs))
    bt, at = P.split_history(tids, losses, 0.25)
    for label in m['labels']:
        pre = '%s/%s/' % (name, label)
        assert np.array_equal(tids, z[pre + 'l_idxs'])
        assert np.array_equal(losses, z[pre + 'l_vals'])
        oi, ov = obs[label]
        assert np.array_equal(oi, z[pre + 'o_idxs']), label
        assert np.array_equal(ov, z[pre + 'o_vals']), label
        b, a = P.split_label(oi, ov, bt, at)
        assert np.array_equal(np.asarray(b, float), z[pre + 'below']), label
        assert np.array_equal(np.asarray(a, float), z[pre + 'above']), label
        # and the product's Parzen posterior equals the oracle's on that split
        s = specs[label]
        post = P.label_posterior(label, s.kind, s.args, b, a, 1.0)
        if post.family == 'categorical':
            exp_b = O.categorical_posterior(s.kind, b, 1.0, s.args['upper'], s.args.get('p'))
            assert np.array_equal(post.below, exp_b)
        else:
            exp_b = O.parzen_for_kind(s.kind, b, 1.0, s.args)
            for got, want in zip(post.below, exp_b[1:4]):
                assert np.array_equal(got, want)


def test_history_cache_incremental_and_errors():
    from hyperopt_amd import history
    space = {'x': hp.uniform('x', 0, 1), 'c': hp.choice('c', [hp.normal('n', 0, 1), 1.0])}
    domain = Domain(lambda d: 0.0, space)
    trials = Trials()
    H.fmin(lambda d: d['x'], space, algo=rand.suggest, max_evals=15, trials=trials,
           rstate=np.random.RandomState(1))
    specs = list(tpe.specs_of(domain))
    t1, l1, o1 = history.gather(domain, trials, specs)
    # same result from a cold cache
    history._caches.pop(trials, None)
    t2, l2, o2 = history.gather(domain, trials, specs)
    assert np.array_equal(t1, t2) and np.array_equal(l1, l2)
    for k in specs:
        assert np.array_equal(o1[k][0], o2[k][0]) and np.array_equal(o1[k][1], o2[k][1])
    # an errored trial disappears from the history
    trials._dynamic_trials[3]['state'] = H.JOB_STATE_ERROR
    trials.refresh()
    t3, _, o3 = history.gather(domain, trials, specs)
    assert 3 not in t3 and 3 not in o3['x'][0]
    # a NaN loss drops the trial (reference: `loss <= best` is False for NaN)
    trials.trials[0]['result']['loss'] = float('nan')
    t4, _, o4 = history.gather(domain, trials, specs)
    assert trials.trials[0]['tid'] not in t4


def test_fmin_random_search_and_space_eval():
    trials = Trials()
    space = {'x': hp.uniform('x', -5, 5), 'k': hp.choice('k', ['a', 'b'])}
    best = H.fmin(lambda d: (d['x'] - 3) ** 2, space, algo=rand.suggest, max_evals=50,
                  trials=trials, rstate=np.random.RandomState(0))
    assert len(trials) == 50 and set(best) == {'x', 'k'}
    pt = H.space_eval(space, best)
    assert pt['k'] in ('a', 'b') and pt['x'] == best['x']
    assert trials.best_trial['result']['loss'] == min(trials.losses())
    d = trials.trials[0]
    for key in ('tid', 'spec', 'result', 'misc', 'state', 'owner', 'book_time',
                'refresh_time', 'exp_key', 'version'):
        assert key in d
    assert d['misc']['cmd'] == ('domain_attachment', 'FMinIter_Domain')


def test_fmin_failures_and_points_to_evaluate():
    def f(d):
        if d['x'] > 4:
            return {'status': H.STATUS_FAIL}
        return {'loss': d['x'] ** 2, 'status': H.STATUS_OK}
    trials = Trials()
    H.fmin(f, {'x': hp.uniform('x', -5, 5)}, algo=rand.suggest, max_evals=40, trials=trials,
           rstate=np.random.RandomState(2))
    assert any(s == H.STATUS_FAIL for s in trials.statuses())
    best = H.fmin(lambda d: d['x'] ** 2, {'x': hp.uniform('x', -5, 5)}, algo=rand.suggest,
                  max_evals=3, points_to_evaluate=[{'x': 0.0}, {'x': 1.0}],
                  rstate=np.random.RandomState(0))
    assert best['x'] == 0.0

    def boom(d):
        raise RuntimeError('x')
    trials = Trials()
    H.fmin(boom, {'x': hp.uniform('x', 0, 1)}, algo=rand.suggest, max_evals=3, trials=trials,
           catch_eval_exceptions=True, rstate=np.random.RandomState(0), return_argmin=False)
    assert len(trials) == 0 and len(trials._dynamic_trials) == 3
    with pytest.raises(RuntimeError):
        H.fmin(boom, {'x': hp.uniform('x', 0, 1)}, algo=rand.suggest, max_evals=1,
               rstate=np.random.RandomState(0))


def test_duplicate_label_and_dependent_bounds():
    with pytest.raises(H.DuplicateLabel):
        Domain(lambda d: 0, [hp.uniform('x', 0, 1), hp.uniform('x', 0, 2)])
    with pytest.raises(ValueError):
        Domain(lambda d: 0, hp.uniform('b', 0, hp.uniform('a', 1, 2)))


def test_active_labels_follow_choice():
    space = conditional()
    specs = LB.compile_space(space)
    vals = {k: 0 for k in specs}
    vals.update(svm_C=1.0, svm_gamma=.1, svm_degree=3.0, rf_n=10.0, rf_depth=3.0, rf_feat=.5,
                lr=0.0)
    assert LB.active_labels(space, vals) == {'clf', 'svm_C', 'svm_kernel', 'svm_gamma', 'lr'}
    vals.update(svm_kernel=1)
    assert LB.active_labels(space, vals) == {'clf', 'svm_C', 'svm_kernel', 'svm_degree', 'lr'}
    vals.update(clf=1)
    assert LB.active_labels(space, vals) == {'clf', 'rf_n', 'rf_depth', 'rf_feat', 'lr'}


def test_compile_space_kinds():
    specs = LB.compile_space(many_dists())
    kinds = {k: s.kind for k, s in specs.items()}
    assert kinds == {'a': 'randint', 'b': 'randint', 'c': 'uniform', 'd': 'loguniform',
                     'e': 'quniform', 'f': 'qloguniform', 'g': 'normal', 'h': 'lognormal',
                     'i': 'qnormal', 'j': 'qlognormal', 'k': 'categorical'}
    assert specs['a'].args == {'upper': 3}
    assert specs['k'].args == {'p': [.1, .9], 'upper': 2}
    assert specs['e'].args == {'low': 0.0, 'high': 10.0, 'q': 3.0}


def test_scope_arithmetic_spaces():
    from hyperopt_amd import scope
    x = hp.uniform('x', -15, 15)
    f = 1.0 / (1.0 + scope.exp(-x)) + 2 * scope.exp(-(x + 10) ** 2)
    out = H.space_eval({'loss': -f, 'arr': [x, x * 2]}, {'x': 0.5})
    assert abs(out['loss'] + (1 / (1 + np.exp(-.5)) + 2 * np.exp(-(10.5) ** 2))) < 1e-12
    assert out['arr'] == (0.5, 1.0)
    a, b = H.space_eval(hp.choice('c', [(1, hp.uniform('u', 0, 1)), (2, 3)]), {'c': 1})
    assert (a, b) == (2, 3)


def _reference_gather(domain, trials):
    """tpe.py:839-861 restated: best doc per from_tid group, None -> +inf,
    sorted by group key."""
    best_docs, best_loss = {}, {}
    for doc in trials.trials:
        tid = doc['misc'].get('from_tid', doc['tid'])
        loss = domain.loss(doc['result'], doc['spec'])
        loss = float('inf') if loss is None else float(loss)
        best_loss.setdefault(tid, loss)
        if loss <= best_loss[tid]:
            best_loss[tid] = loss
            best_docs[tid] = doc
    items = sorted(best_docs.items())
    return (np.asarray([k for k, _ in items], dtype=np.int64),
            np.asarray([best_loss[k] for k, _ in items]))


def test_history_gather_fast_path_incremental():
    """The vectorised gather (own-group docs, incrementally cached tids)
    against the reference's loop while trials are appended, left pending
    (loss None -> +inf), given NaN losses, and re-ordered."""
    from hyperopt_amd import history
    space = {'x': hp.uniform('x', 0, 1), 'k': hp.choice('k', [0, 1, 2])}
    domain = Domain(lambda d: 0.0, space)
    trials = Trials()
    H.fmin(lambda d: d['x'] + d['k'], space, algo=rand.suggest, max_evals=30, trials=trials,
           rstate=np.random.RandomState(2))
    specs = list(tpe.specs_of(domain))
    for step in range(4):
        if step == 1:                      # append more trials
            H.fmin(lambda d: d['x'], space, algo=rand.suggest, max_evals=45, trials=trials,
                   rstate=np.random.RandomState(3))
        if step == 2:                      # pending (no loss) and NaN loss
            trials.trials[4]['result'] = {'status': 'new'}
            trials.trials[9]['result']['loss'] = float('nan')
        if step == 3:                      # out-of-order doc list
            trials._trials = trials._trials[::-1]
        tids, losses, obs = history.gather(domain, trials, specs)
        rt, rl = _reference_gather(domain, trials)
        assert np.array_equal(tids, rt) and np.array_equal(losses, rl), step
        xi, xv = obs['x']
        assert np.all(np.diff(xi) > 0) and set(xi.tolist()) <= set(tids.tolist())


class _ForeignNode(object):
    """A graph node that is not ours: only the attributes the reference's
    pyll nodes share with hyperopt_amd.space.Node (`name`, `pos_args`,
    `named_args`, and `obj` on a literal)."""

    def __init__(self, name):
        self.name = name


def _reference_expr():
    """The reference Domain.expr of
        {'a': hp.choice('a', [{'u': hp.uniform('u', 0, 1)}, {'v': hp.qloguniform('v', 0, 3, 2)}]),
         'k': hp.pchoice('k', [(.1, 0), (.9, 1)]), 'n': hp.qnormal('n', 0, 10, 2)}
    built by the reference's own hp.* (tests/golden/gen_reference_graph.py
    recorded its nodes), rebuilt node for node, shared nodes shared."""
    with open(os.path.join(golden_io.GOLDEN, 'reference_domain_graph.json')) as f:
        g = json.load(f)
    nodes = [_ForeignNode(r['name']) for r in g['nodes']]
    for n, r in zip(nodes, g['nodes']):
        n.pos_args = [nodes[i] for i in r['pos_args']]
        n.named_args = [[k, nodes[i]] for k, i in r['named_args']]
        if r['name'] == 'literal':
            n.obj = r['obj']
    return nodes[g['root']]


def test_compile_reference_domain():
    """The label compiler reads the reference's own pyll graphs (so
    hyperopt_amd.tpe.suggest can be handed a reference Domain)."""
    expr = _reference_expr()
    specs = LB.compile_space(expr)
    res = {k: [s.kind, s.args] for k, s in specs.items()}
    res['active'] = sorted(LB.active_labels(expr, {'a': 1, 'u': .5, 'v': 2.0, 'k': 0, 'n': 0.0}))
    res = json.loads(json.dumps(res))
    assert res['u'] == ['uniform', {'low': 0.0, 'high': 1.0}]
    assert res['v'] == ['qloguniform', {'low': 0.0, 'high': 3.0, 'q': 2.0}]
    assert res['k'] == ['categorical', {'p': [.1, .9], 'upper': 2}]
    assert res['a'] == ['randint', {'upper': 2}]
    assert res['active'] == ['a', 'k', 'n', 'v']
