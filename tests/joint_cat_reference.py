"""Joint TPE with categorical dimensions: the definition in numpy fp64 (test
infrastructure, imported by the tests only; it builds beside the dense and
quantized definitions, tests/joint_reference.py and joint_quant_reference.py).

A dimension d of a joint group is dense, quantized, or categorical with C_d
categories 0 .. C_d - 1 and prior p_d.  For a side with K components
(component 0 the prior) and pw = prior_weight,

    a_d      = C_d * pw / K
    r_0d[c]  = p_d[c]
    r_td[c]  = ([c == o_td] + a_d p_d[c]) / (1 + a_d)      (trial t observed o_td)

    f(x)  = (1/A) sum_k W_k prod_d g_kd(x_d),   g_kd(x_d) = r_kd[x_d] for a categorical d
    m_kd  = 1 for a categorical d: A and the component pick are untouched
    lpdf  = log f(x) - sum_{d dense log kind} y_d

evaluated here from the rows r_kd themselves.  A value that is no integer in
[0, C_d) has factor 0, NaN gives NaN.  Dimension d of candidate g is drawn
with word x of the Philox counter (g, 0, stream_d, round) from the categorical
fold `draw_oracle.fold(r_kd)`.  The observed categories travel in the means.
"""
import numpy as np

from oracle import draw_oracle as D
from tests import joint_quant_reference as QR
from tests import joint_reference as JR

JOINT_CAT_KINDS = ('randint', 'categorical')


class CDim(QR.QDim):
    """A QDim that may be categorical: upper categories with prior p (None:
    not categorical)."""

    def __init__(self, log, low, high, stream, q=None, upper=None, p=None):
        QR.QDim.__init__(self, log, low, high, stream, q)
        self.upper = None if upper is None else int(upper)
        self.p = None if upper is None else np.asarray(p, dtype=np.float64)
        assert self.upper is None or (self.q is None and len(self.p) == self.upper)


class JointCatRef(QR.JointQuantRef):
    """dims: list of CDim; below / above: (W [K], mu [K, D], s [K, D]), a
    categorical dimension's mu column the observed categories (row 0 unused);
    prior_weight: pw of the categorical kernels."""

    def __init__(self, dims, below, above, prior_weight=1.0):
        QR.JointQuantRef.__init__(self, dims, below, above)
        self.pw = float(prior_weight)

    @property
    def uppers(self):
        return np.array([dim.upper or 0 for dim in self.dims], dtype=np.int32)

    @property
    def cat_p(self):
        ps = [dim.p for dim in self.dims if dim.upper]
        return np.concatenate(ps) if ps else np.zeros(0)

    def rows(self, side, d):
        """r_kd [K, C_d] of a categorical dimension."""
        W, mu, _ = self.sides[side]
        dim = self.dims[d]
        K = len(W)
        a = dim.upper * self.pw / K
        r = np.tile(a * dim.p, (K, 1))
        r[np.arange(1, K), mu[1:, d].astype(np.int64)] += 1.0
        r /= 1.0 + a
        r[0] = dim.p
        return r

    def log_terms(self, values, side):
        W, mu, s = self.sides[side]
        x = np.atleast_2d(np.asarray(values, dtype=np.float64))
        dense = [d for d, dim in enumerate(self.dims) if not dim.upper]
        if dense:
            sub = QR.JointQuantRef([self.dims[d] for d in dense], (W, mu[:, dense], s[:, dense]),
                                   (W, mu[:, dense], s[:, dense]))
            e, jac = QR.JointQuantRef.log_terms(sub, x[:, dense], 'below')
        else:
            with np.errstate(divide='ignore'):
                e, jac = np.tile(np.log(W)[None, :], (len(x), 1)), np.zeros(len(x))
        for d, dim in enumerate(self.dims):
            if not dim.upper:
                continue
            v = x[:, d]
            with np.errstate(invalid='ignore'):
                ok = (v >= 0) & (v < dim.upper) & (v == np.floor(v))
            idx = np.where(ok, v, 0).astype(np.int64)
            lr = np.log(self.rows(side, d))[:, idx].T          # [n, K]
            e = e + np.where(ok[:, None], lr, -np.inf)
            e[np.isnan(v)] = np.nan
        return e, jac

    def fold(self, k, d):
        if self.dims[d].upper:
            return D.fold(self.rows('below', d)[k])
        return QR.JointQuantRef.fold(self, k, d)

    def port_draw(self, seed, round, g):
        """JointRef.port_draw with the categorical dimensions' own words."""
        g = np.asarray(g, dtype=np.uint64)
        pf = self.pick_fold()
        wp, wu = D.draw_words(seed, JR.JOINT_STREAM, round, g)
        comp = D.pick(pf, wp)
        excl = D.excluded(pf, wp, wu)
        vals = np.empty((len(g), self.D))
        for d, dim in enumerate(self.dims):
            wpd, wud = D.draw_words(seed, dim.stream, round, g, categorical=bool(dim.upper))
            for k in np.unique(comp):
                sel = comp == k
                f = self.fold(int(k), d)
                _, _, x, v = D.draw_fp64(f, wpd[sel], wud[sel])
                vals[sel, d] = v
                excl[sel] |= D.excluded(f, wpd[sel], wud[sel], x)
        return comp, vals, excl
