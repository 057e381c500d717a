"""Tree-structured Parzen Estimator: drop-in `tpe.suggest` running on MI355X.

    from hyperopt_amd import fmin, hp, tpe, Trials
    fmin(fn, space, algo=tpe.suggest, max_evals=100, trials=Trials())

`suggest` keeps the reference's signature, defaults and returned document
(hyperopt/tpe.py:823-916).  Per call:
  1. history: tids, losses (None -> +inf, min per from_tid group) and per-label
     observations, from a columnar cache (history.py);
  2. fewer than n_startup_jobs docs -> random search (rand.suggest);
  3. posteriors: split by loss rank + adaptive Parzen mixtures / categorical
     pseudocounts per label, bit-identical to the reference (posterior.py);
  4. one fused GPU round over ALL labels (engine.Engine.suggest): sample
     n_EI_candidates per label from l(x) (Philox, stream = label, counter =
     candidate index, round = new_id), lpdf under l and g, broadcast_best;
  5. labels under an un-chosen hp.choice branch are dropped (the reference
     routes every candidate id to the winning branch, vectorize.py:25-43;
     labels are independent given the history, so evaluating every branch
     and keeping the selected one is the same distribution).

Extra keyword arguments (not in the reference): `multivariate` (True: the
unconditional dense continuous labels are modelled jointly, see `suggest`
(joint_quantized=True: the quantized continuous ones with them,
joint_categorical=True: the categorical ones too; joint_bandwidth='scott':
the joint kernels' sigmas from the number of trials and the dimension);
with `group=True` also those that share an hp.choice branch, one joint group
per branch),
`fixed` ({label: value}: the suggestion with those hyperparameters held; the
free labels of a joint group then come from its conditional density),
`pool` (a `Pool` of configurations: the suggestion is the untaken entry with
the largest log l(x) - log g(x), ranked on the device; `pool_replace=True`
takes no entry out; `pool_candidates=m`: that many entries are first drawn from
l, seeded, and the best of them is suggested),
`objectives` (result-dict keys minimised together: each complete trial's loss
becomes its position in a Pareto-compliant order of the objective vectors,
computed on the device; `pareto_front` lists the non-dominated trials),
`constraints` (result-dict keys that must be <= 0: feasible trials rank before
every infeasible one, those by ascending total violation),
`precision` ('f64'; 'f32'
is accepted and runs the same exact path -- see `suggest`), `device` (HIP ordinal), `devices` (a list of ordinals: one
multi-device context splits every round over those GPUs, same documents as
one GPU; tpe_ctx_create_multi), `batch` (True: one independent
suggestion per new_id instead of only new_ids[0]), `posterior_builder`:
'host' (numpy, posterior.py -- the reference's own np.argsort tie order),
'device' (the GPU build: split, sort, Parzen and fold in HIP kernels on the
device-resident history; the device flags every mixture whose value depends
on the order of tied losses or observations, and for exactly those the host
supplies numpy's np.argsort orders and the device builds again --
posterior.build_reference_order -- so the mixtures are the host build's bit
for bit) or 'auto' (device once the history holds DEVICE_BUILD_MIN_OBS
observations over all labels, where the host build starts to dominate the
suggestion).

`importance(space, trials)` (not in the reference) tells which hyperparameters
mattered: per label the variance of the model's good-trial probability under
the label's observed values, from the same Parzen mixtures, summed on the
device (`Engine.importance`).
"""
import itertools
import logging
import operator
import time

import numpy as np

from . import engine as _engine
from . import history as _history
from . import labels as _labels
from . import posterior as _post
from . import rand
from .base import miscs_update_idxs_vals
from .space import as_apply

logger = logging.getLogger(__name__)

EPS = 1e-12
DEFAULT_LF = 25
_default_prior_weight = 1.0
_default_n_EI_candidates = 24
_default_gamma = 0.25
_default_n_startup_jobs = 20
_default_linear_forgetting = DEFAULT_LF
DEVICE_BUILD_MIN_OBS = 16384
# multivariate=True behind a device build of the resident history: the joint
# groups are built on the device from it too (False: always on the host -- the
# same documents; for timing one against the other, tools/time_joint.py)
JOINT_DEVICE_BUILD = True
# objectives=... under posterior_builder='auto': complete trials from which
# the keys come from the kernel (Engine.mo_keys) instead of posterior.mo_keys
# -- the crossover tools/time_mo.py measured on an MI355X at two objectives
# (profiles/mo_keys_timing.json): 64 rows 0.037 ms on the device against 0.030
# ms in numpy, 128 rows 0.041 against 0.051, 1024 rows 0.066 against 1.69.
# (With two constraints, profiles/mo_constraints_timing.json: 128 rows 0.063
# against 0.044, 512 rows 0.095 against 0.127 -- the one threshold serves both
# calls; DESIGN.md, "Constraints".)
MO_DEVICE_MIN_TRIALS = 128

# host-side restatements, exported under the reference's names
ap_filter_trials_split = _post.split_history
adaptive_parzen_normal = _post.adaptive_parzen_normal
linear_forgetting_weights = _post.linear_forgetting_weights


def ap_filter_trials(o_idxs, o_vals, l_idxs, l_vals, gamma, gamma_cap=DEFAULT_LF):
    """tpe.py:624-648."""
    bt, at = _post.split_history(l_idxs, l_vals, gamma, gamma_cap)
    return _post.split_label(o_idxs, o_vals, bt, at)


def specs_of(domain):
    specs = getattr(domain, 'specs', None)
    if isinstance(specs, dict) and specs and isinstance(next(iter(specs.values())),
                                                        _labels.LabelSpec):
        return specs
    cached = getattr(domain, '_hyperopt_amd_specs', None)
    if cached is None:
        cached = _labels.compile_space(domain.expr)
        try:
            domain._hyperopt_amd_specs = cached
        except AttributeError:
            pass
    return cached


def build_posteriors(domain, trials, prior_weight=_default_prior_weight,
                     gamma=_default_gamma):
    """(specs, n_docs, posteriors) for the current history."""
    specs = specs_of(domain)
    tids, losses, obs = _history.gather(domain, trials, list(specs))
    if len(tids) == 0:
        return specs, 0, None
    splitter = _post.Splitter(tids, losses, gamma)
    posts = []
    for label, s in specs.items():
        oi, ov = obs[label]
        b, a = splitter.split(oi, ov)
        posts.append(_post.label_posterior(label, s.kind, s.args, b, a, prior_weight))
    return specs, len(tids), posts


def device_inputs(specs, tids, losses, obs):
    """Arguments of Engine.build_posterior for a gathered history."""
    labels = [(s.label, s.kind, s.args) for s in specs.values()]
    return _post.device_inputs(labels, tids, losses, obs)


def _doc(new_id, domain, trials, specs, values, pool_index=None):
    flat = getattr(domain, '_hyperopt_amd_flat', None)
    if flat is None:
        flat = _labels.always_active(domain.expr)
        try:
            domain._hyperopt_amd_flat = flat
        except AttributeError:
            pass
    active = specs if flat else _labels.active_labels(domain.expr, values)
    idxs = {k: ([new_id] if k in active else []) for k in specs}
    vals = {k: ([values[k]] if k in active else []) for k in specs}
    misc = dict(tid=new_id, cmd=domain.cmd, workdir=domain.workdir)
    if pool_index is not None:
        misc['pool_index'] = pool_index
    miscs_update_idxs_vals([misc], idxs, vals)
    return trials.new_trial_docs([new_id], [None], [domain.new_result()], [misc])


class _PendingView(object):
    """The trials a sequential caller would see after inserting a batch's
    earlier suggestions: the real documents plus those, still pending (state
    new, result {'status': 'new'}: loss None -> +inf, tpe.py:844-847)."""

    def __init__(self, trials):
        self._base = trials
        self.trials = list(trials.trials)

    def new_trial_docs(self, *args, **kwargs):
        return self._base.new_trial_docs(*args, **kwargs)

    def __len__(self):
        return len(self.trials)


PREPARE_MIN = 8192   # candidate slots of a round from which it uses the expansion index


def _resident_posterior(eng, domain, trials, specs, view, gathered, gamma, prior_weight,
                        builder, n_candidates=0, n_rounds=1, round_call=None, info=None):
    """Put the posterior of the current history on the engine, from the
    device-resident history's `view` or the general gather (tids, losses,
    obs); returns (the number of trial documents it was built from, the
    results of round_call when the incremental device build ran it -- the
    dense labels' round under the host's tie-order argsorts -- else None).
    info (a dict, optional): info['resident'] is set when the posterior was
    built on the device from the resident history of `view` -- what the
    joint groups' device build reads (_joint_rounds)."""
    labels = list(specs)
    if view is not None:
        n_docs = view[2]
        n_obs = sum(len(view[3][k][0]) for k in labels)
    if view is None or n_docs == 0:
        tids, losses, obs = gathered or _history.gather(domain, trials, labels)
        n_docs = len(tids)
        n_obs = sum(len(obs[k][0]) for k in labels)
    on_device = n_docs > 0 and (builder == 'device' or (builder == 'auto' and
                                                         n_obs >= DEVICE_BUILD_MIN_OBS))
    if on_device:
        try:
            if view is not None:   # upload only the observations that are new
                up = getattr(eng, '_history_uploader', None)
                if up is None:
                    up = eng._history_uploader = _post.DeviceHistoryUploader()
                _, res = up.build(eng, [(s.label, s.kind, s.args) for s in specs.values()], view, gamma,
                                  prior_weight, prepare=((n_candidates, n_rounds)
                                                         if n_candidates * n_rounds >= PREPARE_MIN else None),
                                  round_call=round_call)
                if info is not None:
                    info['resident'] = True
                return n_docs, res
            eng.build_posterior(*device_inputs(specs, tids, losses, obs), gamma=gamma,
                                prior_weight=prior_weight)
            return n_docs, None
        except _post.NonFiniteObservation:
            # NaN observations: the host build raises what the reference's
            # adaptive_parzen_normal raises (tpe.py:469)
            if view is not None:
                tids, losses, obs = _history.gather(domain, trials, labels)
    elif view is not None and n_docs > 0:
        tids, losses, obs = _history.gather(domain, trials, labels)
    splitter = _post.Splitter(tids, losses, gamma)
    posts = []
    for label, sp in specs.items():
        b, a = splitter.split(*obs[label])
        posts.append(_post.label_posterior(label, sp.kind, sp.args, b, a, prior_weight))
    eng.set_posterior(*_post.pack(posts))
    return n_docs, None


def _joins(spec, kinds):
    """Whether a label's kind is one of `kinds` and the label can join a
    joint group: a 'categorical' label (hp.pchoice) whose p has a zero entry
    cannot -- its rows would not be strictly positive -- and keeps the
    independent round (logged)."""
    if spec.kind not in kinds:
        return False
    if spec.kind == 'categorical' and not np.all(np.asarray(spec.args['p'], dtype=float) > 0.0):
        logger.info('multivariate TPE: label %r has a zero prior probability, using the independent '
                    'path for it' % (spec.label,))
        return False
    return True


def joint_group(domain, specs, obs=None, kinds=_post.JOINT_KINDS):
    """The joint group of a space: its unconditional labels of a dense
    continuous kind (or of any of `kinds`: joint_quantized=True passes the
    quantized kinds too, joint_categorical=True the categorical ones), in the
    order of `specs` -- or None (with the reason logged) when multivariate
    TPE falls back to the independent path: fewer than two such labels, or
    (obs given: label -> (idxs, vals)) labels that are not observed in
    exactly the same trials."""
    free = getattr(domain, '_hyperopt_amd_free', None)
    if free is None:
        free = _labels.unconditional_labels(domain.expr)
        try:
            domain._hyperopt_amd_free = free
        except AttributeError:
            pass
    group = [k for k, s in specs.items() if k in free and _joins(s, kinds)]
    if len(group) < 2:
        logger.info('multivariate TPE: %d joint label(s), using the independent path' % len(group))
        return None
    if obs is not None:
        ids0 = np.asarray(obs[group[0]][0])
        for k in group[1:]:
            if not np.array_equal(ids0, np.asarray(obs[k][0])):
                logger.info('multivariate TPE: labels %r and %r are observed in different trials, '
                            'using the independent path' % (group[0], k))
                return None
    return group


def joint_groups(domain, specs, obs=None, kinds=_post.JOINT_KINDS):
    """The joint groups of a space, [(slot, [labels])]: a structural group is
    the labels of a dense continuous kind (posterior.JOINT_KINDS; or of any
    of `kinds`, which then also decide the slot numbering) that share
    one condition signature (labels.condition_signatures: active in exactly
    the same configurations), at least two of them, in the order of `specs`.
    Slots number the structural groups -- the unconditional group first when
    it qualifies, the others by their first label in `specs` -- and do not
    depend on `obs`.  With obs (label -> (idxs, vals)) a group whose labels
    are not observed in exactly the same trials is left out (logged): its
    labels take the independent path and its slot stays unused."""
    sigs = getattr(domain, '_hyperopt_amd_sigs', None)
    if sigs is None:
        sigs = _labels.condition_signatures(domain.expr)
        try:
            domain._hyperopt_amd_sigs = sigs
        except AttributeError:
            pass
    by_sig = {}
    for k, s in specs.items():
        if _joins(s, kinds):
            by_sig.setdefault(sigs[k], []).append(k)
    groups = [g for sig, g in by_sig.items() if len(g) >= 2]
    # (by_sig keeps the order of each signature's first label in specs)
    groups.sort(key=lambda g: sigs[g[0]] != _labels.UNCONDITIONAL)
    out = []
    for slot, g in enumerate(groups):
        if slot >= _engine.L.TPE_JOINT_MAX_GROUPS:
            logger.info('multivariate TPE: %d groups beyond the %d joint slots use the independent path'
                        % (len(groups) - slot, slot))
            break
        if obs is not None:
            ids0 = np.asarray(obs[g[0]][0])
            odd = [k for k in g[1:] if not np.array_equal(ids0, np.asarray(obs[k][0]))]
            if odd:
                logger.info('multivariate TPE: group %r: labels %r and %r are observed in different '
                            'trials, using the independent path for it' % (g, g[0], odd[0]))
                continue
        out.append((slot, g))
    return out


def _view_columns(view):
    """label -> (tids, vals) of a device view, restricted to the trials the
    general gather keeps (HistoryCache._gather_own: a NaN loss, or a document
    no longer among the trials, drops its observations) -- the columns
    themselves when it keeps every one."""
    tids, losses, n_valid, cols, owner = view
    if n_valid == len(tids) and len(tids) == len(getattr(owner, 'seen', tids)):
        return cols
    keep = tids[losses == losses]
    out = {}
    for k, (ti, tv) in cols.items():
        m = np.isin(ti, keep)
        out[k] = (ti[m], tv[m])
    return out


def _joint_device_args(specs, labels, groups, quantized, categorical, prior_weight, bandwidth='neighbour'):
    """Arguments of Engine.build_joint_groups for [(slot, [label names])]:
    (groups, keywords).  Label indices and streams are positions in the space
    (the resident history holds the labels in that order), slot j's pick
    stream TPE_JOINT_STREAM - j; steps and categorical priors from the same
    joint_prior the host build asks (it raises what that raises).  A
    bandwidth other than the default travels as a keyword, with the prior
    weight its W needs."""
    at = {k: i for i, k in enumerate(labels)}
    args, qs, uppers, cat_ps = [], [], [], []
    for slot, g in groups:
        ids = [at[k] for k in g]
        args.append((slot, _engine.L.TPE_JOINT_STREAM - slot, ids, ids))
        pri = [_post.joint_prior(specs[k].kind, specs[k].args, quantized, categorical) for k in g]
        qs.append([p.q for p in pri])
        uppers.append([p.upper for p in pri])
        ps = [p.p for p in pri if p.upper > 0]
        cat_ps.append(np.concatenate(ps) if ps else np.zeros(0))
    # (None where the call's kinds hold no such label: Engine.build_joint_groups' defaults)
    kw = dict(q=qs if quantized else None, upper=uppers if categorical else None,
              cat_p=cat_ps if categorical else None, prior_weight=prior_weight if categorical else None)
    if bandwidth != 'neighbour':
        kw.update(bandwidth=bandwidth, prior_weight=prior_weight)
    return args, kw


def check_fixed(specs, fixed):
    """tpe.suggest's `fixed` after validation: {label: value as documents
    carry it} (labels.coerce), {} for None.  ValueError for anything that is
    not a dict, an unknown label, a value that is not a finite number, a
    bounded dense kind outside [low, high] (a log kind: [exp(low),
    exp(high)]), a dense log kind that is not positive (a quantized one may be
    0, its rounding interval reaching into the support), a quantized kind
    whose value is not on its grid (v == round(v / q) * q) or whose rounding
    interval [v - q/2, v + q/2] misses the support, and a category that is no
    integer in [0, upper)."""
    if fixed is None:
        return {}
    if not isinstance(fixed, dict):
        raise ValueError('fixed must be a dict of label -> value')
    out = {}
    for label, value in fixed.items():
        if label not in specs:
            raise ValueError('fixed: unknown label %r' % (label,))
        out[label] = check_label_value(specs[label], value, 'fixed[%r]' % (label,))
    return out


def check_label_value(s, value, who):
    """One label's value as documents carry it (labels.coerce), after the
    checks check_fixed lists for the label's kind -- s its LabelSpec; `who`
    opens the ValueError's message (check_fixed: 'fixed[<label>]', Pool: the
    entry and the label)."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s: %r is not a number' % (who, value))
    if not np.isfinite(v):
        raise ValueError('%s: %r is not finite' % (who, value))
    a = s.args
    if s.kind in ('randint', 'categorical'):
        if v != np.floor(v) or not 0 <= v < a['upper']:
            raise ValueError('%s: %r is not an integer in [0, %d)' % (who, value, a['upper']))
        return _labels.coerce(s.kind, v)
    log = s.kind in ('loguniform', 'qloguniform', 'lognormal', 'qlognormal')
    q = a.get('q')
    lo, hi = -np.inf, np.inf
    if 'low' in a:
        lo, hi = (np.exp(a['low']), np.exp(a['high'])) if log else (a['low'], a['high'])
    if q is None:
        if log and not v > 0.0:
            raise ValueError('%s: %r is not positive' % (who, value))
        if not lo <= v <= hi:
            raise ValueError('%s: %r is outside [%r, %r]' % (who, value, lo, hi))
    else:
        if v != np.round(v / q) * q:
            raise ValueError('%s: %r is not on the grid of step %r' % (who, value, q))
        if log:
            lo = max(lo, 0.0)
        if v + q / 2.0 < lo or v - q / 2.0 > hi or (log and not v + q / 2.0 > 0.0):
            raise ValueError("%s: the rounding interval of %r misses the label's support"
                             % (who, value))
    return _labels.coerce(s.kind, v)


_pool_tokens = itertools.count(1)


class Pool(object):
    """A finite set of configurations for tpe.suggest(pool=...) to choose
    from (a tabular benchmark, the architectures that fit, checkpoints that
    exist): the suggestion is then the untaken entry with the largest
    acquisition log l(x) - log g(x), not a draw from l.

    space: the space given to fmin, or a Domain.  points: a non-empty list of
    dicts label -> value, each holding exactly the labels active in that
    configuration, in the form trials.argmin and space_eval use (an hp.choice
    as its index).  ValueError, naming the entry and the label, for an unknown
    label, a value check_fixed would refuse for the label, and an entry whose
    labels are not labels.active_labels(expr, point).

    values: [n, L] float64, NaN where a label is not active, columns in the
    order of specs_of(domain); labels: that order; points: the validated
    entries (values through labels.coerce); token: unique per object -- an
    engine uploads the pool once and keeps it while the token is the same."""

    def __init__(self, space, points):
        if not _labels.is_node(space) and hasattr(space, 'expr'):   # a Domain
            self.expr = space.expr
            specs = specs_of(space)
        else:
            self.expr = as_apply(space)
            specs = _labels.compile_space(self.expr)
        points = list(points)
        if not points:
            raise ValueError('Pool: points must not be empty')
        self.labels = list(specs)
        col = {k: i for i, k in enumerate(self.labels)}
        self.values = np.full((len(points), len(self.labels)), np.nan)
        self.points = []
        for i, point in enumerate(points):
            if not isinstance(point, dict):
                raise ValueError('Pool: entry %d is not a dict of label -> value' % i)
            out = {}
            for label, value in point.items():
                if label not in specs:
                    raise ValueError('Pool: entry %d: unknown label %r' % (i, label))
                out[label] = check_label_value(specs[label], value, 'Pool: entry %d, label %r' % (i, label))
            try:
                active = _labels.active_labels(self.expr, out)
            except KeyError as e:
                raise ValueError('Pool: entry %d: label %r is active in this configuration and has no value'
                                 % (i, e.args[0]))
            if set(out) != active:
                odd = sorted(set(out) ^ active)[0]
                raise ValueError('Pool: entry %d: label %r is %s' % (
                    i, odd, 'not active in this configuration' if odd in out
                    else 'active in this configuration and has no value'))
            for label, v in out.items():
                self.values[i, col[label]] = float(v)
            self.points.append(out)
        self.token = ('pool', next(_pool_tokens))

    def __len__(self):
        return len(self.points)


def pool_taken(pool, trials):
    """The entries of `pool` the trials hold already, ascending: every index
    some document of trials.trials, whatever its state, carries in
    misc['pool_index'] (other values of that key are ignored)."""
    taken = set()
    for doc in trials.trials:
        i = doc['misc'].get('pool_index')
        if isinstance(i, (int, np.integer)) and not isinstance(i, bool) and 0 <= i < len(pool):
            taken.add(int(i))
    return sorted(taken)


def check_pool_candidates(pool_candidates, pool):
    """suggest's pool_candidates as an int >= 1, or None; ValueError for a
    bool, a non-integer, a value below 1, or a value without a pool."""
    if pool_candidates is None:
        return None
    if isinstance(pool_candidates, bool) or not isinstance(pool_candidates, (int, np.integer)):
        raise ValueError('pool_candidates=%r: an integer >= 1, or None' % (pool_candidates,))
    if pool_candidates < 1:
        raise ValueError('pool_candidates=%r: must be at least 1' % (pool_candidates,))
    if pool is None:
        raise ValueError('pool_candidates=%r needs a pool' % (pool_candidates,))
    return int(pool_candidates)


def _pool_doc(new_id, domain, trials, specs, pool, index):
    return _doc(new_id, domain, trials, specs, dict(pool.points[index]), pool_index=int(index))


def _pool_startup_docs(new_ids, domain, trials, seed, pool, taken):
    """The startup phase over a pool: with rng = RandomState(seed), each new
    id in order takes free[rng.randint(len(free))] of the untaken indices in
    ascending order, and that index is removed; fewer documents when the pool
    runs out."""
    rng = np.random.RandomState(seed)
    specs = specs_of(domain)
    out_of = set(taken)
    free = [i for i in range(len(pool)) if i not in out_of]
    rval = []
    for new_id in new_ids:
        if not free:
            break
        index = free.pop(int(rng.randint(len(free))))
        rval.extend(_pool_doc(new_id, domain, trials, specs, pool, index))
    return rval


def _startup_docs(new_ids, domain, trials, seed, fixed):
    """The startup phase's documents: rand.suggest's, unchanged, without
    `fixed`; with it the same prior draws with the fixed labels held
    (labels.sample_config: a fixed label consumes no random numbers, the
    others are drawn in rand.suggest's order from one RandomState(seed))."""
    if not fixed:
        return rand.suggest(new_ids, domain, trials, seed)      # tpe.py:869-871
    rng = np.random.RandomState(seed)
    specs = specs_of(domain)
    rval = []
    for new_id in new_ids:
        values = _labels.sample_config(domain.expr, specs, rng, fixed)
        idxs = {k: ([new_id] if k in values else []) for k in specs}
        vals = {k: ([values[k]] if k in values else []) for k in specs}
        misc = dict(tid=new_id, cmd=domain.cmd, workdir=domain.workdir)
        miscs_update_idxs_vals([misc], idxs, vals)
        rval.extend(trials.new_trial_docs([new_id], [None], [domain.new_result()], [misc]))
    return rval


def _joint_rounds(eng, domain, trials, specs, gathered, gamma, prior_weight, seed, ids, n_candidates,
                  group=False, quantized=False, categorical=False, view=None, bandwidth='neighbour',
                  fixed=None):
    """One joint round per id and joint group: [label -> value] per id, or
    None when the call falls back to the independent path.  group=False: the
    unconditional group alone (joint_group), slot 0; group=True: every group
    of joint_groups in its slot, slot j's component pick on the Philox stream
    TPE_JOINT_STREAM - j.  A label's Philox stream is its position in the
    space, as in the independent round.

    view: the device view this call's univariate posterior was built from, on
    the engine's resident history (None: it was not).  With it the groups are
    read off the view's columns and every group with a label that is not
    categorical is built on the device from that build
    (Engine.build_joint_groups: one call, no gather, nothing uploaded); a
    group the device flags (a tie whose order it was not given, a category
    out of range) and a group of categorical labels alone are built on the
    host like every group without a view: posterior.joint_mixture from the
    gathered observations, one set_joint_group each.  The mixtures are the
    same bits either way.  One joint_suggest_batch for all groups and ids.

    quantized=True: the groups take the quantized kinds too
    (posterior.JOINT_QUANT_KINDS), their values rounded to the label's grid;
    categorical=True: and the categorical kinds (posterior.JOINT_CAT_KINDS; a
    label with a zero prior probability stays out), their values category
    indices; every group value enters the document through labels.coerce.

    bandwidth: the rule of the groups' sigmas (posterior.JOINT_BANDWIDTHS),
    handed to both builders.  Under 'scott' no sorted position enters a
    mixture, so the device flags no tie: the groups with tied observations
    (the rule for quantized labels) stay on the device.

    fixed (label -> value, validated: check_fixed): a group all of whose
    labels are fixed is not built; a group with fixed and free labels is
    built like any other, by either builder, and then conditioned in place
    on the device (Engine.joint_condition): its slot holds the free labels in
    their order in the group, and its winner's columns are theirs (one
    logger.info line says how many groups were conditioned).  Groups without
    a fixed label are untouched.  The fixed labels' values are the caller's
    to put into the document."""
    fixed = fixed or {}
    groups = _joint_build(eng, domain, trials, specs, gathered, gamma, prior_weight, group=group,
                          quantized=quantized, categorical=categorical, view=view, bandwidth=bandwidth,
                          fixed=fixed)
    if not groups:
        return None
    free = {slot: [k for k in g if k not in fixed] for slot, g in groups}
    if fixed:
        n_cond = 0
        for slot, g in groups:
            held = [k for k in g if k in fixed]
            if held:
                eng.joint_condition(slot, [g.index(k) for k in held], [float(fixed[k]) for k in held])
                n_cond += 1
        logger.info('multivariate TPE: %d group(s) conditioned on fixed labels' % n_cond)
    won = eng.joint_suggest_batch(seed, ids, n_candidates)
    out = [{} for _ in ids]
    for slot, g in groups:
        values = won[slot][0]
        for j in range(len(ids)):
            out[j].update({k: _labels.coerce(specs[k].kind, v) for k, v in zip(free[slot], values[j])})
    return out


def _joint_build(eng, domain, trials, specs, gathered, gamma, prior_weight, group=False, quantized=False,
                 categorical=False, view=None, bandwidth='neighbour', fixed=None):
    """The building half of _joint_rounds, shared with the pool ranking: the
    call's joint groups [(slot, [labels])], each built into its slot of the
    engine by the device or the host as _joint_rounds describes -- or None
    when there is none (the independent path).  Groups all of whose labels
    are in `fixed` are left out; nothing is conditioned and no round runs."""
    fixed = fixed or {}
    kinds = _post.JOINT_KINDS + (_post.JOINT_QUANT_KINDS if quantized else ()) + \
        (_post.JOINT_CAT_KINDS if categorical else ())
    labels = list(specs)
    if view is None:
        gathered = gathered or _history.gather(domain, trials, labels)
    obs = _view_columns(view) if view is not None else gathered[2]
    if group:
        groups = joint_groups(domain, specs, obs, kinds)
    else:
        g = joint_group(domain, specs, obs, kinds)
        groups = [(0, g)] if g is not None else []
    if group and not groups:
        logger.info('multivariate TPE: no joint group, using the independent path')
    groups = [(slot, g) for slot, g in groups if not all(k in fixed for k in g)]
    if not groups:
        return None
    eng.clear_joint_groups()
    on_device = [(slot, g) for slot, g in groups
                 if view is not None and any(specs[k].kind not in _post.JOINT_CAT_KINDS for k in g)]
    flagged = []
    if on_device:
        args, kw = _joint_device_args(specs, labels, on_device, quantized, categorical, prior_weight, bandwidth)
        flags = eng.build_joint_groups(args, **kw)
        flagged = [sg for sg, f in zip(on_device, flags) if f]
    built = [sg for sg in on_device if sg not in flagged]
    on_host = [sg for sg in groups if sg not in built]
    logger.info('multivariate TPE: %d group(s) built on the device, %d on the host (%d flagged by the device), '
                '%s bandwidth' % (len(built), len(on_host), len(flagged), bandwidth))
    if on_host:
        tids, losses, obs = gathered or _history.gather(domain, trials, labels)
        splitter = _post.Splitter(tids, losses, gamma)
        for slot, g in on_host:
            mix = _post.joint_mixture([specs[k] for k in g], obs, splitter, prior_weight,
                                      streams=[labels.index(k) for k in g], quantized=quantized,
                                      categorical=categorical, bandwidth=bandwidth)
            eng.set_joint_group(slot, _engine.L.TPE_JOINT_STREAM - slot, *mix, prior_weight=prior_weight)
    return groups


def check_objectives(objectives):
    """tpe.suggest's `objectives` after validation: a tuple of 1 to
    posterior.MO_MAX_OBJECTIVES distinct result-dict keys, None for None.
    ValueError for anything that is not a sequence of strings (one string is
    not one), an empty one, a repeated key and too many."""
    if objectives is None:
        return None
    if isinstance(objectives, (str, bytes)) or not isinstance(objectives, (list, tuple)):
        raise ValueError('objectives must be a list or tuple of result keys')
    objectives = tuple(objectives)
    if not objectives:
        raise ValueError('objectives must not be empty')
    for key in objectives:
        if not isinstance(key, str):
            raise ValueError('objectives: %r is not a string' % (key,))
    if len(set(objectives)) != len(objectives):
        raise ValueError('objectives: %r names a key twice' % (objectives,))
    if len(objectives) > _post.MO_MAX_OBJECTIVES:
        raise ValueError('objectives: at most %d, got %d' % (_post.MO_MAX_OBJECTIVES, len(objectives)))
    return objectives


def check_constraints(constraints, objectives=None):
    """tpe.suggest's `constraints` after validation, by check_objectives'
    rules: a tuple of 1 to posterior.MO_MAX_CONSTRAINTS distinct result-dict
    keys, None for None.  ValueError also for 'loss' as a constraint and for a
    name that is one of the (validated) `objectives` as well."""
    if constraints is None:
        return None
    if isinstance(constraints, (str, bytes)) or not isinstance(constraints, (list, tuple)):
        raise ValueError('constraints must be a list or tuple of result keys')
    constraints = tuple(constraints)
    if not constraints:
        raise ValueError('constraints must not be empty')
    for key in constraints:
        if not isinstance(key, str):
            raise ValueError('constraints: %r is not a string' % (key,))
    if len(set(constraints)) != len(constraints):
        raise ValueError('constraints: %r names a key twice' % (constraints,))
    if len(constraints) > _post.MO_MAX_CONSTRAINTS:
        raise ValueError('constraints: at most %d, got %d' % (_post.MO_MAX_CONSTRAINTS, len(constraints)))
    for key in constraints:
        if key == 'loss' or key in (objectives or ()):
            raise ValueError('constraints: %r is an objective' % (key,))
    return constraints


def objective_rows(docs, objectives, domain=None, check_from=True, constraints=None):
    """The objective vectors of the complete documents among `docs`:
    (complete documents in the order of docs, F [their number, len(objectives)]
    float64).  A document is complete when its loss -- domain.loss(result,
    spec), result.get('loss') without a domain -- is not None (a pending or
    failed one has none); 'loss' among the objectives is that value, every
    other key is read from the result.  ValueError for a complete document
    that lacks a key (the message names its tid and the key) and, with
    check_from, for any document with a from_tid other than its tid: the best
    of a group is not defined for vectors (tpe.suggest asks the history
    cache, which has looked at every document once already).  With
    `constraints` the answer is (documents, F, G [their number,
    len(constraints)]), G read from the results like the other keys."""
    # (C-level passes over the documents, as history.raw_losses reads the
    # losses: at 10k trials a Python loop per document costs more than the
    # ranking itself)
    docs = list(docs)
    results = list(map(_history._result_of, docs))
    if domain is None or type(domain).loss is _history._plain_loss:
        raw = list(map(dict.get, results, itertools.repeat('loss')))
    else:
        raw = _history.raw_losses(domain, docs)
    if check_from:
        froms = list(map(dict.get, map(_misc_of, docs), itertools.repeat('from_tid')))
        if froms.count(None) != len(froms):
            for d, f in zip(docs, froms):
                if f is not None and f != d['tid']:
                    raise ValueError('objectives: trial %r has from_tid %r; groups of trials are not '
                                     'supported with several objectives' % (d['tid'], f))
    if None in raw:
        done = [i for i, v in enumerate(raw) if v is not None]
        docs = [docs[i] for i in done]
        raw = [raw[i] for i in done]
        results = [results[i] for i in done]
    F = np.empty((len(docs), len(objectives)))
    for m, key in enumerate(objectives):
        col = raw if key == 'loss' else list(map(dict.get, results, itertools.repeat(key)))
        if None in col:
            raise ValueError('objectives: trial %r has no %r in its result'
                             % (docs[col.index(None)]['tid'], key))
        F[:, m] = col
    if constraints is None:
        return docs, F
    G = np.empty((len(docs), len(constraints)))
    for k, key in enumerate(constraints):
        col = list(map(dict.get, results, itertools.repeat(key)))
        if None in col:
            raise ValueError('constraints: trial %r has no %r in its result'
                             % (docs[col.index(None)]['tid'], key))
        G[:, k] = col
    return docs, F, G


_misc_of = operator.itemgetter('misc')


def objective_keys(F, builder='auto', engine=None, G=None):
    """posterior.mo_keys(F) by the builder the call selects: 'host' numpy,
    'device' the kernel (Engine.mo_keys on `engine`, a callable returning the
    Engine), 'auto' the kernel from MO_DEVICE_MIN_TRIALS rows on.  The same
    integers either way.  G: the constraint rows (posterior.mo_keys(F, G=G),
    Engine.mo_keys(F, G=G))."""
    if len(F) and (builder == 'device' or (builder == 'auto' and len(F) >= MO_DEVICE_MIN_TRIALS)):
        if len(F) > _post.MO_MAX_ROWS:
            raise ValueError('objectives: at most %d complete trials' % _post.MO_MAX_ROWS)
        return engine().mo_keys(F) if G is None else engine().mo_keys(F, G=G)
    return _post.mo_keys(F) if G is None else _post.mo_keys(F, G=G)


class _KeyedDomain(object):
    """A domain whose loss is a column computed beforehand: the complete
    documents' keys by the identity of their result dicts, None (pending:
    +inf) for every other document -- also the ones a batch='pending' view
    adds.  Everything else is the wrapped domain's, attribute writes (the
    caches specs_of and _doc keep on a domain) included.  src: the list the
    complete documents `docs` were taken from; when every one of its
    documents is complete the keys are its column as they stand, and the
    lookup by identity is built only for another list."""

    def __init__(self, domain, docs, keys, src=None):
        keys = keys.tolist()
        whole = src is not None and len(src) == len(docs)
        object.__setattr__(self, '_domain', domain)
        object.__setattr__(self, '_src', src if whole else None)
        object.__setattr__(self, '_column', keys)
        object.__setattr__(self, '_docs', docs)
        object.__setattr__(self, '_lookup', None)

    def __getattr__(self, name):
        return getattr(self._domain, name)

    def __setattr__(self, name, value):
        setattr(self._domain, name, value)

    @property
    def _key_of(self):
        if self._lookup is None:
            object.__setattr__(self, '_lookup', dict(zip(map(id, map(_history._result_of, self._docs)),
                                                         self._column)))
        return self._lookup

    def loss(self, result, config=None):
        return self._key_of.get(id(result))

    def loss_column(self, docs):
        if docs is self._src:
            return self._column
        return list(map(self._key_of.get, map(id, map(_history._result_of, docs))))


def pareto_front(trials, objectives, constraints=None):
    """The complete trials of `trials` that no other one dominates under the
    objectives (all minimised; posterior.mo_counts: by == 0), in tid order.
    Complete as in objective_rows, 'loss' read as result.get('loss'); a trial
    with a NaN objective is on no front.  With `constraints` (result keys,
    <= 0 satisfied): the feasible trials that no feasible trial dominates --
    with objectives=('loss',) the best feasible trial(s) -- and [] when no
    trial is feasible (by == 0 alone would then name the least-violating
    one: the violation has to be 0 as well)."""
    objectives = check_objectives(objectives)
    if objectives is None:
        raise ValueError('pareto_front needs objectives')
    constraints = check_constraints(constraints, objectives)
    if constraints is None:
        docs, F = objective_rows(trials.trials, objectives)
        by, _ = _post.mo_counts(F) if len(docs) else (np.zeros(0, dtype=np.int32), None)
        return sorted((d for d, b in zip(docs, by) if b == 0), key=lambda d: d['tid'])
    docs, F, G = objective_rows(trials.trials, objectives, constraints=constraints)
    if not len(docs):
        return []
    by, _ = _post.mo_counts(F, G)
    v = _post.mo_violation(G, F)
    return sorted((d for d, b, vi in zip(docs, by, v) if b == 0 and vi == 0), key=lambda d: d['tid'])


def importance(space, trials, quantile=0.1, n_grid=4096, prior_weight=_default_prior_weight,
               normalize=True, curves=False, device=0, objectives=None, constraints=None):
    """Which hyperparameters mattered (not in the reference; Optuna's
    get_param_importances with the PED-ANOVA evaluator asks the same
    question): {label: importance}, sorted descending, ties in label order.

    space: the space given to fmin, or a Domain.  The n complete trials (a
    loss that is not None; a NaN loss stays out as always) are split at the
    quantile: the n_below = ceil(quantile n) best by loss are "good" (stable
    sort, ties by trial order).  For a label observed nb times among them and
    na times among the rest, alpha = nb / (nb + na), l and g are
    posterior.label_posterior's mixtures of the two observation lists (the
    estimator tpe.suggest samples from, with prior_weight and linear
    forgetting), p = alpha l + (1 - alpha) g models the label's observed
    values and m(x) = alpha l(x) / p(x) is the model's probability that a
    trial with that value is good.  The label's raw importance is the variance
    of m under p, weighted by how often the label is active,
        V = sum_cells w_j p(x_j) (m(x_j) - alpha)^2,    I = (nb + na) / n  V
    -- alpha^2 times the Pearson divergence of l from p, PED-ANOVA's quantity
    with the global baseline -- summed over posterior.importance_cells' cells
    (n_grid of them for a dense label; DESIGN.md section 6b, "Hyperparameter
    importance").  A label with nb = 0 or na = 0 has V = 0.  normalize=True
    returns I / np.sum(I) (the labels in the space's order), all zeros when
    the sum is 0.  A label whose sum is NaN (a NaN lpdf at one of its cells: a
    NaN or non-positive observation of a log kind, say) keeps NaN, comes
    last in the dict and is left out of the normalising sum: the other
    labels' shares are those among themselves.

    The mixtures of every label are uploaded to a context of their own
    (engine.get_engine(device, 'f64', 'importance'): the history tpe.suggest
    keeps resident on the 'main' one stays there) and one Engine.importance
    call sums every label's cells on the device.

    curves=True returns (importances, {label: (x, w, p, m)}) for the labels
    with observations on both sides: the cells and, at each, the density p
    and the good-trial probability m -- the partial-dependence view.

    objectives / constraints replace the loss by the keys tpe.suggest ranks
    the trials with under the same keywords.

    ValueError, before any engine is touched: quantile outside (0, 1), n_grid
    not an integer >= 1, fewer than 2 complete trials, and what
    check_objectives, check_constraints and objective_rows refuse."""
    objectives = check_objectives(objectives)
    constraints = check_constraints(constraints, objectives)
    if isinstance(quantile, bool) or not isinstance(quantile, (int, float, np.integer, np.floating)) \
            or not 0.0 < quantile < 1.0:
        raise ValueError('importance: quantile must lie in (0, 1), got %r' % (quantile,))
    if isinstance(n_grid, bool) or not isinstance(n_grid, (int, np.integer)) or n_grid < 1:
        raise ValueError('importance: n_grid must be an integer >= 1, got %r' % (n_grid,))
    if not _labels.is_node(space) and hasattr(space, 'expr'):   # a Domain
        domain = space
    else:
        from .base import Domain
        domain = Domain(None, space)
    specs = specs_of(domain)
    names = list(specs)

    def engine():
        return _engine.get_engine(device, 'f64', 'importance')
    if objectives is not None or constraints is not None:
        src = trials.trials
        check_from = _history.has_from_tid(trials, names)
        if constraints is None:
            docs, F = objective_rows(src, objectives, domain, check_from=check_from)
            G = None
        else:
            docs, F, G = objective_rows(src, objectives or ('loss',), domain, check_from=check_from,
                                        constraints=constraints)
        if len(docs) < 2:
            raise ValueError('importance: needs at least 2 complete trials, got %d' % len(docs))
        domain = _KeyedDomain(domain, docs, objective_keys(F, 'auto', engine, G=G), src)
    tids, losses, obs = _history.gather(domain, trials, names)
    done = losses < np.inf                       # (pending and failed trials carry +inf)
    tids, losses = tids[done], losses[done]
    n = len(tids)
    if n < 2:
        raise ValueError('importance: needs at least 2 complete trials, got %d' % n)
    splitter = _post.Splitter(tids, losses, 0.0, n_below=int(np.ceil(quantile * n)))
    posts, sel, cells, alphas, active = [], [], [], [], np.zeros(len(names))
    for li, (label, s) in enumerate(specs.items()):
        oi, ov = obs[label]
        if not done.all():
            keep = np.isin(oi, tids)
            oi, ov = oi[keep], ov[keep]
        b, a = splitter.split(oi, ov)
        posts.append(_post.label_posterior(label, s.kind, s.args, b, a, prior_weight))
        active[li] = (len(b) + len(a)) / n
        if len(b) and len(a):
            sel.append(li)
            cells.append(_post.importance_cells(s.kind, s.args, ov, n_grid))
            alphas.append(len(b) / (len(b) + len(a)))
    raw = np.zeros(len(names))
    planes = None
    if sel:
        eng = engine()
        eng.set_posterior(*_post.pack(posts))
        out = eng.importance(sel, cells, alphas, want_planes=curves)
        v, planes = (out[0], out[1:]) if curves else (out, None)
        raw[sel] = active[sel] * v
    bad = np.isnan(raw)
    if normalize:
        # (a NaN label stays NaN and takes no part in the others' shares)
        total = np.sum(raw[~bad])
        raw = np.where(bad, np.nan, raw / total if total != 0 else 0.0)
    order = sorted(range(len(names)), key=lambda i: (bool(bad[i]), 0.0 if bad[i] else -raw[i], i))
    result = {names[i]: float(raw[i]) for i in order}
    if not curves:
        return result
    views = {}
    for k, li in enumerate(sel):
        x, w, _ = cells[k]
        with np.errstate(invalid='ignore', divide='ignore'):
            lik = alphas[k] * np.exp(planes[0][k])
            p = lik + (1.0 - alphas[k]) * np.exp(planes[1][k])
            m = np.where(p > 0, lik / p, alphas[k])
        views[names[li]] = (x, w, p, m)
    return result, views


def suggest(new_ids, domain, trials, seed,
            prior_weight=_default_prior_weight,
            n_startup_jobs=_default_n_startup_jobs,
            n_EI_candidates=_default_n_EI_candidates,
            gamma=_default_gamma,
            linear_forgetting=_default_linear_forgetting,
            precision='f64', device=0, batch=False, posterior_builder='auto', devices=None,
            multivariate=False, group=False, joint_quantized=False, joint_categorical=False,
            joint_bandwidth='neighbour', fixed=None, pool=None, pool_candidates=None, pool_replace=False,
            constraints=None, objectives=None):
    """tpe.py:823-916.  Past the startup phase one document for new_ids[0],
    like the reference; `batch` (not in the reference) asks for one document
    per new_id:

    * batch=True -- the documents K sequential calls suggest([new_ids[j]],
      domain, trials, seed) would return with `trials` unchanged between
      them: one posterior, the batch's other suggestions excluded from it;
    * batch='pending' -- past the startup phase, the documents K sequential
      calls return when each call's document is inserted into the trials,
      still pending, before the next call (the reference's view of queued
      trials: loss None -> +inf, tpe.py:844-847; fmin with max_queue_len,
      fmin.py:193-202).  The first k = n_startup_jobs - len(docs) ids (the
      calls that would still be in the startup phase) are answered by ONE
      rand.suggest(new_ids[:k], ...) call -- distinct draws, as the
      reference answers a startup batch -- not by k sequential calls.

    During the startup phase (fewer than n_startup_jobs documents) the
    reference's rand.suggest(new_ids, ...) answers, for every new_id.

    multivariate=True (not in the reference) models the joint group -- the
    unconditional labels of kind uniform, loguniform, normal or lognormal --
    together: one product kernel per trial, whole configurations drawn from
    one below trial's neighbourhood and scored under the joint densities
    ("Multivariate TPE"; Engine.joint_suggest).  Every other label
    keeps its independent round, bit for bit.  The call is the independent
    one when the group has fewer than two labels or its labels are not
    observed in the same trials.  With `devices` the joint posteriors are
    replicated on every device and each joint round is split over them --
    by candidate ranges from 1024 candidates per device, else by whole
    rounds of a batch -- with the one-device documents bit for bit
    (Engine.joint_last_shards tells how the last round ran).  Such a call
    raises ValueError when a listed device is not on the machine (before it
    was supported the combination always raised it).

    group=True (with multivariate=True) models the labels inside hp.choice
    branches too: every set of at least two such labels that are active in
    exactly the same configurations (joint_groups) is one joint group with
    its own mixtures, built from the trials that entered its branch -- a
    branch without a below trial has the prior alone as its below side, a
    group never observed the prior on both sides (every score 0: candidate
    0).  All groups and new ids run in one batched device call
    (Engine.joint_suggest_batch); labels of an un-chosen branch are dropped
    from the document as always.  A space whose only group is the
    unconditional one gives the documents of group=False.

    joint_quantized=True (with multivariate=True) lets the joint groups hold
    the quantized kinds quniform, qloguniform, qnormal and qlognormal as well
    (batch size, depth, width beside a learning rate): a quantized label is
    drawn from its component and rounded to its grid, and its factor in the
    joint density is the component's mass on the value's rounding interval
    ("Quantized labels").  The groups and their slots
    are those of the widened kinds.  With the default every call returns
    the documents it always did: a quantized label then keeps its
    independent round.

    joint_categorical=True (with multivariate=True) lets the joint groups
    hold hp.choice, hp.pchoice and hp.randint labels as well (optimizer x
    learning rate, kernel x C): a trial's kernel in such a dimension puts
    ([c == observed] + a p[c]) / (1 + a) on category c, a = C prior_weight /
    K with K the side's components -- Optuna's categorical kernel with this
    label's prior p in place of the uniform one -- and the prior component p
    itself ("Categorical labels in joint groups").
    With group=True an unconditional hp.choice index joins the
    unconditional group, the labels inside its branches keep the group of
    their own signature.  An hp.pchoice label with a zero probability stays
    out of every group.  The groups and their slots are those of the widened
    kinds; the keyword composes with joint_quantized and group, and with the
    default every call returns the documents it always did.

    Where the call's posterior is built on the device from the resident
    history (posterior_builder 'device', or 'auto' past its threshold), the
    joint groups are built there too, from that build
    (Engine.build_joint_groups: no gather, no upload, one synchronisation
    for all groups) -- the same mixtures bit for bit, so the same documents.
    With several devices each one builds its replica; under label shards
    (the default of `devices` on a resident history) the owners of a group's
    labels gather their columns and the devices exchange them directly.
    A group in which a label's side holds two equal observations whose
    np.argsort order the univariate build did not need (common for quantized
    labels), one with an out-of-range category and one of categorical labels
    alone are built on the host as before (_joint_rounds; one logger.info
    line per call names the path).

    joint_bandwidth='scott' (with multivariate=True; default 'neighbour')
    takes the sigmas of the joint kernels from the number of trials and the
    dimension -- s_d = clip(0.2 n^(-1/(D+4)) prior_sigma_d, prior_sigma_d /
    min(100, 2 + n), prior_sigma_d) for every trial of a side of n trials in
    a group of D labels -- instead of the univariate build's neighbour gaps,
    which in a product over D dimensions collapse to the lower clip
    (posterior.joint_mixture, DESIGN.md section 6b, "Bandwidth of joint
    groups").  It composes with group, joint_quantized, joint_categorical,
    batch and devices, and both builders give the same documents.  The rule
    needs no sorted position, so groups with tied observations (quantized
    labels) are built on the device too; a group of categorical labels alone
    still goes to the host.  With the default every call returns the
    documents it always did.

    fixed={label: value} (not in the reference; Optuna's PartialFixedSampler,
    BoTorch's fixed_features) asks for the suggestion with those
    hyperparameters already decided; it applies to every new id of the call
    and composes with every other keyword.  The values are validated first
    (check_fixed: ValueError before any engine is touched) and enter the
    document through labels.coerce; the active labels are resolved from the
    final values, so a fixed hp.choice index selects its branch and a fixed
    label under a branch the document does not enter is dropped.  A fixed
    label outside every joint group (all of them with multivariate=False)
    still runs its independent round and its winner is replaced: every other
    label's value is the unfixed call's, bit for bit.  In a joint group the
    free labels come from the group's conditional density given the fixed
    ones -- the point of modelling them together: each side's mixture keeps
    its kernels and re-weights them by the fixed dimensions' factors, W'_k ~
    W_k prod_{d fixed} g_kd(x_d), on the device (Engine.joint_condition,
    DESIGN.md section 6b, "Fixed hyperparameters"), after either builder;
    a group all of whose labels are fixed is not built, one without a fixed
    label is untouched.  During the startup phase the documents are prior
    draws with the fixed labels held (a fixed choice selects the branch that
    is sampled; a fixed label consumes no random numbers, the others are
    drawn in rand.suggest's order).  fixed=None and fixed={} return what the
    call returns without the keyword.

    pool=tpe.Pool(space, points) (not in the reference) restricts the call to
    a finite set of configurations: the document is the pool entry with the
    largest acquisition log l(x) - log g(x) -- the sum over the entry's active
    labels of lpdf_below - lpdf_above under this call's posterior, a joint
    group's ll - lg in place of its labels' terms under multivariate=True --
    instead of a draw from l ("Candidate pools").  The
    posterior is built exactly as without the keyword, by whichever builder
    the call selects, and the joint groups with it; no round is drawn: one
    Engine.pool_rank call ranks the whole pool, which the engine holds on the
    device from the first call on (it is uploaded again only for another Pool
    object).  An entry is taken when any document of trials.trials, whatever
    its state, carries its index in misc['pool_index'], as the documents of
    such a call do: the call is a function of the trials like every other,
    fmin visits no entry twice, and batch='pending' keeps its sequential
    meaning with nothing extra.  batch=True returns the K best distinct
    entries of one ranking, best first.  During the startup phase each new id
    in order takes free[rng.randint(len(free))] of the untaken indices in
    ascending order, rng = RandomState(seed), without replacement.  The call
    returns fewer documents than ids when the pool runs out and [] when
    nothing is free, which ends fmin's run.  pool_replace=True takes nothing:
    every call then ranks the whole pool.  n_EI_candidates is ignored with a
    pool, and without pool_candidates seed is read in the startup phase only.
    ValueError, before any engine is touched: pool with a non-empty fixed
    (filter the pool instead), pool with more than one device, a pool whose
    labels are not the domain's, pool_replace without a pool.  With pool=None
    every call returns what it returned before.

    pool_candidates=m (an integer >= 1; None: the ranking above, unchanged)
    makes the pool call TPE's own step ("Drawing from
    the pool"): m of the free entries are drawn from the good-trial density l
    -- with probability proportional to l(x) in the labels' working space
    (log x for the log kinds), without replacement, seeded by (seed, new_id,
    entry) -- and the document is the drawn entry with the largest
    log l(x) - log g(x).  One Engine.pool_draw call answers every id, each
    with its own draw: two workers with different seeds, and the ids of a
    batch, explore different parts of the pool.  batch=True picks distinct
    entries (every id's draw leaves out the earlier ids' picks);
    pool_replace=True lets them repeat.  m at least the number of free
    entries draws them all and returns the ranking's documents; the call
    returns fewer documents than ids when the pool runs out.  The posterior,
    the joint groups, the taken set and the startup phase are those of the
    pool call without the keyword.  ValueError, before any engine is touched:
    pool_candidates without a pool, a bool, a non-integer, a value below 1.

    objectives=('loss', 'latency', ...) (not in the reference; Optuna's MOTPE
    serves the same studies) minimises several entries of the result dict at
    once: 1 to 8 distinct keys, 'loss' read through domain.loss, the others
    from the result -- the objective function returns {'loss': err, 'latency':
    ms, 'status': STATUS_OK}.  Past the startup phase the call is the call
    without the keyword on another loss column: every complete trial's loss is
    replaced by its key, its position in a Pareto-compliant total order of the
    trials' objective vectors ("Several objectives") --
    ascending number of trials that dominate it (0 exactly on the Pareto
    front), then descending number of trials it dominates, then trial order.
    The front usually holds more trials than the below set, so the second
    criterion decides most below sets: it favours front points that dominate
    many trials (the knee) over the front's extremes.  The keys are distinct
    integers, so the split meets no tie.  They are computed once per call from
    all the trials (results arrive in any order) and reach every reader of the
    losses -- the resident view, the general gather, the joint builds,
    batch='pending''s view -- so the keyword composes with every other one
    unchanged.  posterior_builder 'host' computes them in numpy
    (posterior.mo_keys), 'device' with one all-pairs kernel and a radix sort
    (Engine.mo_keys), 'auto' on the device from MO_DEVICE_MIN_TRIALS complete
    trials on; the same integers, so the same documents.  A trial without a
    loss (pending, failed) keeps +inf and takes no part in the ranking; one
    with a NaN in any objective keeps NaN and stays out of the history, as a
    NaN loss does.  ValueError, before any engine is touched: objectives that
    are not such a sequence, a complete trial that lacks one of the keys (the
    message names the tid and the key), a document with a from_tid (the best
    of a group is not defined for vectors).  The startup phase is unchanged,
    and objectives=('loss',) with distinct losses returns the plain call's
    documents.  tpe.pareto_front(trials, objectives) lists the front.  With
    objectives=None every call returns what it returned before.

    constraints=('mem_over', 'lat_over') (not in the reference; Optuna's
    constraints_func) names 1 to 8 further result-dict keys, each a hard limit
    in Optuna's convention: c <= 0 satisfied, c > 0 violated by that amount --
    the objective function returns {'loss': err, 'mem_over': gb - 16.0,
    'status': STATUS_OK}.  With or without `objectives` (None: the one
    objective 'loss', read through domain.loss).  The call is again the plain
    call on a column of keys, now from the order feasibility first (DESIGN.md
    section 6b, "Constraints"): the feasible trials -- total violation v =
    sum_k max(c_k, 0) equal to 0 -- in the order above, dominance counted
    among feasible trials only; then the infeasible ones by ascending v, then
    trial order.  An infeasible trial never enters the below set before a
    feasible one however good its objectives are, and when fewer feasible
    trials exist than the below set holds, the least-violating infeasible
    ones fill it.  A trial with a NaN in an objective or a constraint keeps
    NaN.  The builders are those of `objectives` (posterior.mo_keys(F, G=G),
    Engine.mo_keys(F, G=G); the same integers), and so is the validation
    (check_constraints; also ValueError: 'loss' or an objective named as a
    constraint, a complete trial without one of the keys, a from_tid).  The
    startup phase is unchanged.  Domain, Trials, fmin's argmin and
    trials.best_trial know nothing of feasibility: they still report the
    smallest loss; tpe.pareto_front(trials, ('loss',), constraints=...) gives
    the best feasible trial.  With constraints=None every call returns what
    it returned before.

    precision='f32' runs the exact fp64 path: a round draws every candidate
    and proves all but ~0.5 % of them out of the race from per-sub-bin score
    bounds before any lpdf is summed, so scoring the rest in fp32 would save
    nothing measurable while giving up the bit-exact
    winner; the fp32 lpdf contract (1e-4 relative) holds trivially.  The raw
    fp32 round stays available as Engine(precision='f32')."""
    t0 = time.time()
    objectives = check_objectives(objectives)   # (first: nothing else has run when it raises)
    constraints = check_constraints(constraints, objectives)
    pool_candidates = check_pool_candidates(pool_candidates, pool)
    pool_kw = {} if pool_candidates is None else dict(pool_candidates=pool_candidates)   # (None is not handed on)
    if objectives is not None or constraints is not None:
        # the call below on another loss column: the keys once, from all the
        # trials; every place that reads losses reads them through the domain
        src = trials.trials
        builder = posterior_builder if posterior_builder in ('host', 'device') else 'auto'

        def engine():
            return _engine.get_engine(list(devices) if devices else device, 'f64', 'main')
        # (a from_tid: flagged by the history cache, named by the full check)
        check_from = _history.has_from_tid(trials, list(specs_of(domain)))
        if constraints is None:
            docs, F = objective_rows(src, objectives, domain, check_from=check_from)
            keys = objective_keys(F, builder, engine)
            logger.info('tpe.suggest: %d objectives, %d complete trials ranked, %.1f ms' % (
                len(objectives), len(docs), (time.time() - t0) * 1e3))
        else:
            names = objectives or ('loss',)
            docs, F, G = objective_rows(src, names, domain, check_from=check_from, constraints=constraints)
            keys = objective_keys(F, builder, engine, G=G)
            if logger.isEnabledFor(logging.INFO):      # (the count is a pass over the rows)
                logger.info('tpe.suggest: %d objectives, %d constraints, %d complete trials ranked, %d of them '
                            'feasible, %.1f ms' % (len(names), len(constraints), len(docs),
                                                   int(np.count_nonzero(_post.mo_violation(G, F) == 0.0)),
                                                   (time.time() - t0) * 1e3))
        return suggest(new_ids, _KeyedDomain(domain, docs, keys, src), trials, seed, prior_weight=prior_weight,
                       n_startup_jobs=n_startup_jobs, n_EI_candidates=n_EI_candidates, gamma=gamma,
                       linear_forgetting=linear_forgetting, precision=precision, device=device, batch=batch,
                       posterior_builder=posterior_builder, devices=devices, multivariate=multivariate,
                       group=group, joint_quantized=joint_quantized, joint_categorical=joint_categorical,
                       joint_bandwidth=joint_bandwidth, fixed=fixed, pool=pool, pool_replace=pool_replace,
                       **pool_kw)
    specs = specs_of(domain)
    fixed = check_fixed(specs, fixed)
    if precision not in ('f64', 'f32'):
        raise ValueError("precision must be 'f64' or 'f32'")
    if posterior_builder not in ('auto', 'host', 'device'):
        raise ValueError('posterior_builder must be auto, host or device')
    if batch not in (False, True, 'pending'):
        raise ValueError("batch must be False, True or 'pending'")
    if group and not multivariate:
        raise ValueError('group=True needs multivariate=True')
    if joint_quantized and not multivariate:
        raise ValueError('joint_quantized=True needs multivariate=True')
    if joint_categorical and not multivariate:
        raise ValueError('joint_categorical=True needs multivariate=True')
    if joint_bandwidth not in _post.JOINT_BANDWIDTHS:
        raise ValueError('joint_bandwidth must be one of %r' % (_post.JOINT_BANDWIDTHS,))
    if joint_bandwidth != 'neighbour' and not multivariate:
        raise ValueError('joint_bandwidth=%r needs multivariate=True' % (joint_bandwidth,))
    if pool_replace and pool is None:
        raise ValueError('pool_replace=True needs a pool')
    if pool is not None:
        if not isinstance(pool, Pool):
            raise ValueError('pool must be a tpe.Pool')
        if fixed:
            raise ValueError('pool with fixed: filter the pool instead')
        if devices and len(list(devices)) > 1:
            raise ValueError('pool with devices=%r: a pool is ranked on one device' % (list(devices),))
        if pool.labels != list(specs):
            raise ValueError("pool: its labels %r are not the domain's %r" % (pool.labels, list(specs)))
    if multivariate and devices and len(list(devices)) > 1:
        # every device holds a replica of every joint group and runs a shard
        # of every joint round: the call needs all of them, startup phase or not
        missing = _engine.missing_devices(devices)
        if missing:
            raise ValueError('multivariate=True with devices=%r: no GPU %r on this machine'
                             % (list(devices), missing))
    kw = dict(prior_weight=prior_weight, n_startup_jobs=n_startup_jobs,
              n_EI_candidates=n_EI_candidates, gamma=gamma, linear_forgetting=linear_forgetting,
              precision=precision, device=device, posterior_builder=posterior_builder,
              devices=devices, multivariate=multivariate, group=group, joint_quantized=joint_quantized,
              joint_categorical=joint_categorical, joint_bandwidth=joint_bandwidth)
    if fixed:   # (an empty one is not handed on)
        kw['fixed'] = fixed
    taken = []
    if pool is not None:
        kw.update(pool=pool, pool_replace=pool_replace, **pool_kw)
        taken = [] if pool_replace else pool_taken(pool, trials)
        if len(taken) == len(pool):
            return []   # (nothing is free: fmin's _ask stops on an empty answer)

    def startup_docs(ids):
        if pool is not None:
            return _pool_startup_docs(ids, domain, trials, seed, pool, taken)
        return _startup_docs(ids, domain, trials, seed, fixed)
    labels = list(specs)
    # the device-resident history's view of the trials (None when the fast
    # layout does not apply); otherwise the general gather
    view = _history.device_view(domain, trials, labels) if posterior_builder != 'host' else None
    gathered = None
    if view is not None:
        n_docs = view[2]
    else:
        gathered = _history.gather(domain, trials, labels)
        n_docs = len(gathered[0])
    if batch == 'pending' and len(new_ids) > 1:
        # the calls that would still see fewer than n_startup_jobs documents
        # are the startup phase: one rand.suggest over their ids, as the
        # reference answers a startup batch (tpe.py:869-871; distinct draws
        # from one RandomState(seed), the documents batch=True returns) --
        # then one TPE call per remaining id, each seeing the earlier ones
        # as pending trials
        k = max(0, min(len(new_ids), n_startup_jobs - n_docs))
        rval = list(startup_docs(list(new_ids[:k]))) if k else []
        if k < len(new_ids):
            pview = _PendingView(trials)
            pview.trials.extend(rval)
            for new_id in new_ids[k:]:
                docs = suggest([new_id], domain, pview, seed, batch=False, **kw)
                pview.trials.extend(docs)
                rval.extend(docs)
        return rval
    if n_docs < n_startup_jobs:
        return startup_docs(new_ids)
    if n_docs == 0:
        logger.info('TPE using 0 trials')                     # the prior-only posterior
    # a pending view (batch='pending') keeps its own context: its history
    # (the trials plus the batch's earlier suggestions) would otherwise
    # replace the real trials' device-resident history, and the next call
    # on those would upload it whole again
    eng = _engine.get_engine(list(devices) if devices else device, 'f64',
                             'pending' if isinstance(trials, _PendingView) else 'main')
    ids = list(new_ids) if batch else [new_ids[0]]

    def round_call():
        if len(ids) == 1:
            return eng.suggest(seed, n_EI_candidates, round=ids[0])[None]
        return eng.suggest_batch(seed, ids, n_EI_candidates)
    info = {}
    if pool is not None:
        # the posterior and the joint groups as below, by the same builders;
        # no round: one ranking of the resident pool, its best entries to the
        # ids in order
        _resident_posterior(eng, domain, trials, specs, view, gathered, gamma, prior_weight,
                            posterior_builder, info=info)
        jview = view if (JOINT_DEVICE_BUILD and info.get('resident')) else None
        groups = _joint_build(eng, domain, trials, specs, gathered, gamma, prior_weight, group=group,
                              quantized=bool(joint_quantized), categorical=bool(joint_categorical),
                              view=jview, bandwidth=joint_bandwidth) if multivariate else None
        if getattr(eng, 'pool_token', None) != pool.token:
            eng.pool_set(pool.values)
            eng.pool_token = pool.token
        cols = [(slot, [labels.index(k) for k in g]) for slot, g in groups or []]
        if pool_candidates is None:
            index, _ = eng.pool_rank(len(ids), groups=cols, taken=taken)
            how = ''
        else:
            # TPE's own step on the pool: per id (its round) pool_candidates
            # entries drawn from l, the best l/g among them
            index, _ = eng.pool_draw(seed, ids, pool_candidates, groups=cols, taken=taken,
                                     distinct=not pool_replace)
            how = ', %d drawn per id' % min(pool_candidates, len(pool) - len(taken))
        rval = []
        for new_id, i in zip(ids, index):
            rval.extend(_pool_doc(new_id, domain, trials, specs, pool, int(i)))
        logger.info('tpe.suggest: %d trials, %d labels, pool of %d (%d taken)%s, %.1f ms' % (
            n_docs, len(specs), len(pool), len(taken), how, (time.time() - t0) * 1e3))
        return rval
    _, res = _resident_posterior(eng, domain, trials, specs, view, gathered, gamma, prior_weight,
                                 posterior_builder, n_candidates=n_EI_candidates, n_rounds=len(ids),
                                 round_call=round_call, info=info)
    if res is None:
        res = round_call()
    # the joint groups are built on the device(s) when this call's univariate
    # posterior was: from the resident history (on several devices, label
    # shards or not, every device builds its replica of every group)
    jview = view if (JOINT_DEVICE_BUILD and info.get('resident')) else None
    joint = _joint_rounds(eng, domain, trials, specs, gathered, gamma, prior_weight, seed, ids,
                          n_EI_candidates, group=group, quantized=bool(joint_quantized),
                          categorical=bool(joint_categorical), view=jview,
                          bandwidth=joint_bandwidth, fixed=fixed) if multivariate else None
    rval = []
    for j, new_id in enumerate(ids):
        values = {s.label: _labels.coerce(s.kind, res[j][i]['value'])
                  for i, s in enumerate(specs.values())}
        values.update(fixed)
        if joint is not None:
            values.update(joint[j])
        rval.extend(_doc(new_id, domain, trials, specs, values))
    logger.info('tpe.suggest: %d trials, %d labels, %.1f ms' % (
        n_docs, len(specs), (time.time() - t0) * 1e3))
    return rval


# -- reference operators on the GPU engine (tpe.py:56-307, 769-778) ----------

def _eng():
    return _engine.get_engine(0, 'f64')


def GMM1_lpdf(samples, weights, mus, sigmas, low=None, high=None, q=None):
    return _eng().GMM1_lpdf(samples, weights, mus, sigmas, low, high, q)


def LGMM1_lpdf(samples, weights, mus, sigmas, low=None, high=None, q=None):
    return _eng().LGMM1_lpdf(samples, weights, mus, sigmas, low, high, q)


def categorical_lpdf(sample, p, upper=None):
    return _eng().categorical_lpdf(sample, p, upper)


def broadcast_best(samples, below_llik, above_llik):
    return _eng().broadcast_best(samples, below_llik, above_llik)


def _seed_from(rng):
    if rng is None:
        return np.random.randint(2 ** 31 - 1)
    return int(rng.randint(2 ** 31 - 1))


def GMM1(weights, mus, sigmas, low=None, high=None, q=None, rng=None, size=()):
    """Draws from the truncated mixture (Philox stream seeded from `rng`)."""
    out = _eng().GMM1(weights, mus, sigmas, low, high, q, seed=_seed_from(rng),
                      size=size if size != () else (1,))
    return out if size != () else out[0]


def LGMM1(weights, mus, sigmas, low=None, high=None, q=None, rng=None, size=()):
    out = _eng().LGMM1(weights, mus, sigmas, low, high, q, seed=_seed_from(rng),
                       size=size if size != () else (1,))
    return out if size != () else out[0]
