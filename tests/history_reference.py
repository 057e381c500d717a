"""A plain numpy model of the device-resident history (tpe_history_reset /
tpe_history_append, hyperopt_amd/csrc/tpe_build.hip): what Engine.history_get
must read back after every append, and the oracle mixtures of what the pool
then holds.  Importable without a GPU.

Per label the pool keeps (trial position, value) in arrival order; a
non-categorical label also has a sorted view -- np.argsort(values,
kind='stable') and the values in that order, i.e. equal keys (-0.0 == +0.0
among them) in observation order across every append.  The expected mixtures
are the existing CPU oracle's (oracle.tpe_oracle.label_posteriors through
tests.helpers.oracle_mixtures): sort_kind='stable' for the device's position
order, None for the reference's own order."""
import numpy as np

from hyperopt_amd.workloads import History
from tests.helpers import oracle_mixtures

CATEGORICAL = ('randint', 'categorical')


class PoolModel(object):
    def __init__(self, labels):
        self.reset(labels)

    def reset(self, labels):
        """tpe_history_reset: nothing of an earlier history remains."""
        self.labels = list(labels)
        L = len(self.labels)
        self.trial = [np.zeros(0, np.int32) for _ in range(L)]
        self.val = [np.zeros(0) for _ in range(L)]     # what the device holds (transformed)
        self.raw = [np.zeros(0) for _ in range(L)]     # what the oracle transforms itself

    def append(self, n_new, trial, val, raw):
        """tpe_history_append's arguments (label-major concatenation) plus
        the untransformed values of the same observations."""
        o = 0
        for l, m in enumerate(n_new):
            m = int(m)
            self.trial[l] = np.concatenate([self.trial[l], np.asarray(trial[o:o + m], np.int32)])
            self.val[l] = np.concatenate([self.val[l], np.asarray(val[o:o + m], float)])
            self.raw[l] = np.concatenate([self.raw[l], np.asarray(raw[o:o + m], float)])
            o += m
        assert o == len(trial) == len(val) == len(raw)

    def count(self, l):
        return len(self.trial[l])

    def is_categorical(self, l):
        return self.labels[l][1] in CATEGORICAL

    def sorted_view(self, l):
        """(idx int32, key f64) of a non-categorical label; None otherwise."""
        if self.is_categorical(l):
            return None
        idx = np.argsort(self.val[l], kind='stable').astype(np.int32)
        return idx, self.val[l][idx]

    # -- what the builds see -------------------------------------------------
    def obs_of(self):
        """posterior.build_reference_order's observation accessor."""
        def f(l):
            return self.trial[l], self.val[l]
        f.n_labels = len(self.labels)
        return f

    def history(self, losses):
        """The oracle's view: the trials with a loss (NaN: outside the
        history; +inf: pending, inside), tids = trial positions; orphan
        observations (trial -1) belong to no trial."""
        losses = np.asarray(losses, float)
        ok = losses == losses
        tids = np.flatnonzero(ok).astype(np.int64)
        obs = {name: (self.trial[l].astype(np.int64), self.raw[l])
               for l, (name, _, _) in enumerate(self.labels)}
        return History(self.labels, tids, losses[ok], obs)

    def mixtures(self, losses, sort_kind, gamma=0.25, pw=1.0):
        h = self.history(losses)
        return h, oracle_mixtures(h, gamma, pw, sort_kind=sort_kind)
