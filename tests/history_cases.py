"""Scenarios for the device-resident history (tests/test_history_gpu.py; their
preconditions are asserted on the host by tests/test_history_cases_host.py).

A scenario is a label list plus a sequence of steps; a step is one
tpe_history_append (n_new per label, trial positions and values label-major)
and the loss vector of the builds that follow it.  Plain numpy, importable
without a GPU.

The labels are the ten kinds of ALL_KINDS (active in ~0.6 of the trials) plus
  every  in every trial: its region regrows at counts 257 and 515 (capacity
         max(2 need, 256): 256 -> 514 -> 1030),
  rare   in ~0.05 of the trials: never leaves capacity 256,
  late   first observed after trial 300: until then a zero-width region at
         its right neighbour's offset,
  never  never observed,
the last two placed between populated neighbours.  Losses are rounded to one
decimal (ties, also across the split), a few trials never get a loss (NaN), a
few are pending (+inf) for some steps after they arrive, a few observations
are orphans (trial -1), and some observations repeat an earlier value of
their label so that every kind meets equal keys across an append (qnormal
with q = 0.5 around 0 supplies -0.0 and +0.0)."""
import numpy as np

from hyperopt_amd import posterior as P
from hyperopt_amd.workloads import prior_draw
from tests.helpers import ALL_KINDS

EVERY = ('every', 'normal', dict(mu=0.0, sigma=3.0))
RARE = ('rare', 'normal', dict(mu=1.0, sigma=2.0))
LATE = ('late', 'quniform', dict(low=0.0, high=10.0, q=1.0))
NEVER = ('never', 'loguniform', dict(low=-3.0, high=1.0))
LABELS = ALL_KINDS[:2] + [LATE] + ALL_KINDS[2:5] + [NEVER] + ALL_KINDS[5:] + [EVERY, RARE]
EXTRA = [('x1', 'uniform', dict(low=0.0, high=1.0)), ('x2', 'randint', dict(upper=3)),
         ('x3', 'qnormal', dict(mu=0.0, sigma=2.0, q=0.5))]

LATE_FIRST = 300
ACTIVITY = {'every': (1.0, 0), 'rare': (0.05, 0), 'late': (0.6, LATE_FIRST), 'never': (0.0, 0)}
ORPHAN_LABELS = ('u', 'qn', 'pc')
GLOBAL_SORT_MIN = 4096     # tpe_build.hip kGlobalSortMin
MIN_CAP = 256              # tpe_build.hip: capacity max(2 need, 256)


def index_of(labels, name):
    return [n for n, _, _ in labels].index(name)


class Step(object):
    """One append and the losses of the builds after it."""

    def __init__(self, n_new, trial, val, raw, losses):
        self.n_new = np.asarray(n_new, dtype=np.int64)
        self.trial = np.asarray(trial, dtype=np.int32)
        self.val = np.asarray(val, dtype=np.float64)
        self.raw = np.asarray(raw, dtype=np.float64)
        self.losses = np.asarray(losses, dtype=np.float64)
        assert self.n_new.sum() == len(self.trial) == len(self.val) == len(self.raw)

    def part(self, l):
        a = int(self.n_new[:l].sum())
        b = a + int(self.n_new[l])
        return self.trial[a:b], self.val[a:b], self.raw[a:b]


class Scenario(object):
    def __init__(self, name, labels, steps):
        self.name, self.labels, self.steps = name, list(labels), list(steps)


# ------------------------------------------------------------- generation --
def draw_columns(labels, n_trials, seed, frac=0.6, dup=0.04, orphans=2):
    """Per label the observations of n_trials trials in arrival order:
    arrive (the trial they arrive with), pos (trial position, -1 for an
    orphan), raw and val (the transformed value the device is given)."""
    rng = np.random.RandomState(seed)
    trs = P.spec_table(labels)[2]
    cols = []
    for i, (name, kind, args) in enumerate(labels):
        f, first = ACTIVITY.get(name, (frac, 0))
        t = np.arange(n_trials)
        act = t[(rng.uniform(size=n_trials) < f) & (t >= first)]
        raw = prior_draw(kind, args, rng, len(act))
        for j in range(1, len(raw)):                   # repeat an earlier value
            if rng.uniform() < dup:
                raw[j] = raw[rng.randint(j)]
        arrive, pos = act.copy(), act.astype(np.int32)
        if orphans and name in ORPHAN_LABELS and n_trials > orphans:
            at = np.sort(rng.choice(n_trials, orphans, replace=False))
            arrive = np.concatenate([arrive, at])
            pos = np.concatenate([pos, np.full(orphans, -1, np.int32)])
            raw = np.concatenate([raw, prior_draw(kind, args, rng, orphans)])
            o = np.argsort(arrive, kind='stable')
            arrive, pos, raw = arrive[o], pos[o], raw[o]
        val = np.asarray(trs[i](raw), float) if trs[i] is not None and len(raw) else raw.astype(float)
        cols.append(dict(arrive=arrive, pos=pos, raw=raw, val=val))
    return cols


def drop(col, mask):
    """Remove the masked observations of one label's column."""
    for k in ('arrive', 'pos', 'raw', 'val'):
        col[k] = col[k][~mask]


class Losses(object):
    """Losses rounded to one decimal; nan: trials that never get one;
    pending: trial -> the trial count from which its loss is finite (+inf
    before); fixed: trial -> loss."""

    def __init__(self, n_trials, seed, nan=(), pending=None, fixed=None):
        rng = np.random.RandomState(seed + 1000)
        self.base = np.round(rng.normal(size=n_trials), 1)
        for t, v in (fixed or {}).items():
            self.base[t] = v
        self.nan = [t for t in nan if t < n_trials]
        self.pending = dict(pending or {})

    def at(self, n):
        l = self.base[:n].copy()
        for t, r in self.pending.items():
            if t < n and n < r:
                l[t] = np.inf
        for t in self.nan:
            if t < n:
                l[t] = np.nan
        return l


def steps_from_cuts(cols, cuts, losses):
    """Step k appends the observations that arrive with trials [cuts[k-1],
    cuts[k]); its losses are those of the first cuts[k] trials."""
    steps, prev = [], 0
    for c in cuts:
        n_new, tr, va, ra = [], [], [], []
        for col in cols:
            sel = (col['arrive'] >= prev) & (col['arrive'] < c)
            n_new.append(int(sel.sum()))
            tr.append(col['pos'][sel])
            va.append(col['val'][sel])
            ra.append(col['raw'][sel])
        steps.append(Step(n_new, np.concatenate(tr), np.concatenate(va), np.concatenate(ra), losses.at(c)))
        prev = c
    return steps


# -------------------------------------------------------------- scenarios --
STEPWISE_TRIALS = 522
STEPWISE_SEED = 4
# trial -> (loss once finite, the trial count from which it is): two enter
# the below set when they turn finite, two stay above
STEPWISE_PENDING = {5: (-3.3, 9), 40: (2.9, 47), 300: (-3.4, 306), 260: (2.8, 263)}
STEPWISE_NAN = (12, 100, 258, 400)


def stepwise(stride=1, seed=STEPWISE_SEED):
    """`stride` trials per append from 0 to past the second regrow of
    `every`; most labels get nothing at many steps."""
    n = STEPWISE_TRIALS
    cols = draw_columns(LABELS, n, seed, orphans=3)
    losses = Losses(n, seed, nan=STEPWISE_NAN, pending={t: r for t, (_, r) in STEPWISE_PENDING.items()},
                    fixed={t: v for t, (v, _) in STEPWISE_PENDING.items()})
    cuts = list(range(stride, n + 1, stride))
    if cuts[-1] != n:
        cuts.append(n)
    return Scenario('stepwise/%d' % stride, LABELS, steps_from_cuts(cols, cuts, losses))


def threshold(total, seed=9):
    """One bulk append staging exactly `total` observations (the sort switch
    is at GLOBAL_SORT_MIN), then one small append merged over it."""
    n = 640
    cols = draw_columns(LABELS, n, seed, frac=0.7, orphans=3)
    count = lambda c: sum(int((col['arrive'] < c).sum()) for col in cols)
    cut = next(c for c in range(1, n + 1) if count(c) >= total)
    excess = count(cut) - total
    for col in cols[::-1]:                 # trim the bulk's last trial to the exact total
        last = np.flatnonzero(col['arrive'] == cut - 1)
        if excess and len(last):
            m = np.zeros(len(col['arrive']), bool)
            m[last[-1]] = True
            drop(col, m)
            excess -= 1
    assert excess == 0 and count(cut) == total
    losses = Losses(n, seed, nan=(7, 333), pending={20: cut + 1})
    return Scenario('threshold/%d' % total, LABELS, steps_from_cuts(cols, [cut, cut + 3], losses))


MERGE_BASE = 300


def merge_edges(seed=6):
    """Six small appends onto `every` holding MERGE_BASE observations."""
    n = MERGE_BASE
    cols = draw_columns(LABELS, n, seed, orphans=2)
    losses = Losses(n + 64, seed, nan=(50,))
    steps = steps_from_cuts(cols, [n], losses)
    ie, L = index_of(LABELS, 'every'), len(LABELS)
    old = cols[ie]['val']
    s = np.sort(old)
    u, c = np.unique(old, return_counts=True)
    rep = float(u[np.argmax(c)])           # a key `every` already holds more than once
    T = [n]

    def batch(per_label):
        """per_label: label index -> values, one new trial per value (the
        labels share the batch's trials from its first on)."""
        k = max([len(v) for v in per_label.values()] + [0])
        n_new, tr, va = [0] * L, [], []
        for l in sorted(per_label):
            v = np.asarray(per_label[l], float)
            n_new[l] = len(v)
            tr.append(np.arange(T[0], T[0] + len(v), dtype=np.int32))
            va.append(v)
        T[0] += k
        cat = lambda x: np.concatenate(x) if x else np.zeros(0)
        steps.append(Step(n_new, cat(tr), cat(va), cat(va), losses.at(T[0])))

    batch({ie: [s[0] - 1.0, s[0] - 3.0, s[0] - 2.0, s[0] - 3.0, s[0] - 0.5]})        # all below the old keys
    batch({ie: [s[-1] + 2.0, s[-1] + 1.0, s[-1] + 2.0, s[-1] + 5.0]})                # all above
    batch({ie: [rep] * 4})                                                             # one repeated old key
    batch({ie: [s[10], 0.0, s[200], -0.0, s[10], 0.0, 0.5 * (s[150] + s[151]), s[200], rep]})   # interleaved
    batch({index_of(LABELS, 'ri'): [3.0, 0.0, 3.0], index_of(LABELS, 'pc'): [1.0, 2.0]})       # categorical only
    batch({})                                                                          # nothing
    return Scenario('merge_edges', LABELS, steps)


LONE = 'u'


def lone_regrow(seed=11):
    """LONE (capacity 256 from a first small append) jumps from 200 to 300
    observations in one append in which no other label gets any: the pool is
    re-laid out for it alone.  The lone append is the last step."""
    n = 600
    cols = draw_columns(LABELS, n, seed, orphans=2)
    il = index_of(LABELS, LONE)
    arr = cols[il]['arrive']
    c1, c2 = int(arr[199]) + 1, int(arr[299]) + 1
    assert int((arr < c1).sum()) == 200 and int((arr < c2).sum()) == 300
    for l, col in enumerate(cols):
        if l != il:
            drop(col, (col['arrive'] >= c1) & (col['arrive'] < c2))
    losses = Losses(n, seed, nan=(30,), pending={10: c1 + 1})
    return Scenario('lone_regrow', LABELS, steps_from_cuts(cols, [20, c1, c2], losses))


def short(labels, seed, n=40, cuts=(1, 2, 10, 40), frac=0.6):
    """A short history of `labels` (the reuse and the two-label cases)."""
    cols = draw_columns(labels, n, seed, frac=frac, orphans=1)
    losses = Losses(n, seed, nan=(3,) if n > 8 else (), pending={1: 5} if n > 8 else None)
    return Scenario('short/%d/%d' % (len(labels), n), labels, steps_from_cuts(cols, list(cuts), losses))


# ------------------------------------------------------- derived quantities --
def n_below_of(losses):
    losses = np.asarray(losses)
    return P.n_below_of(int(np.count_nonzero(losses == losses)), 0.25)


def split_tie(losses):
    """Equal losses on both sides of the n_below boundary."""
    losses = np.asarray(losses)
    s = np.sort(losses[losses == losses])
    nb = n_below_of(losses)
    return 0 < nb < len(s) and s[nb - 1] == s[nb]


def capacities(scn):
    """Per step the per-label (count, capacity) after it, by the pool's rule:
    a label that outgrows its region gets max(2 need, MIN_CAP)."""
    L = len(scn.labels)
    cnt, cap, out = [0] * L, [0] * L, []
    for st in scn.steps:
        for l in range(L):
            cnt[l] += int(st.n_new[l])
            if cnt[l] > cap[l]:
                cap[l] = max(2 * cnt[l], MIN_CAP)
        out.append((list(cnt), list(cap)))
    return out


def regrow_steps(scn):
    """Steps whose append re-lays the pool out (some capacity changes)."""
    caps = capacities(scn)
    return [k for k in range(1, len(caps)) if caps[k][1] != caps[k - 1][1]]


def oracle_steps(scn, dense_until=80, every=8, near=2):
    """The steps whose mixtures are compared with the oracle: every step up
    to `dense_until` trials, within `near` of each regrow and of each change
    of n_below, the steps at which an earlier trial's loss changes (pending
    -> finite), and every `every`-th otherwise."""
    nb = [n_below_of(st.losses) for st in scn.steps]
    hot = set(regrow_steps(scn)) | {k for k in range(1, len(nb)) if nb[k] != nb[k - 1]}
    out = []
    for k, st in enumerate(scn.steps):
        prev = scn.steps[k - 1].losses if k else st.losses[:0]
        edited = not np.array_equal(prev, st.losses[:len(prev)], equal_nan=True)
        if (len(st.losses) <= dense_until or k % every == 0 or k == len(scn.steps) - 1 or edited
                or any(abs(k - h) <= near for h in hot)):
            out.append(k)
    return out
