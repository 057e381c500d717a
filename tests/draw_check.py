"""The common rule of the device draw comparisons (test_gpu_draws.py and
test_gpu_parity.py): a device value against the fp64 port on every draw and
against the 140-digit exact draw on a subset, at T_DEV = 4 T_PORT."""
import numpy as np

from oracle import draw_oracle as D
from tests.test_draw_oracle import EPS51, T_PORT, x_tolerance

T_DEV = 4 * T_PORT
WORST = {}      # path -> worst device error, in units of the T_PORT bound (vs port, vs exact)


def ratio(f, k, z, x, got):
    """|got - reference| over the T_PORT bound of the reference draw (z, x):
    <= 4 passes.  Quantized labels: 0 where the values are equal, inf else."""
    ref = D.value_of(f, x)
    if f.q is not None:
        return np.where(got == ref, 0.0, np.inf)
    tol = x_tolerance(f, k, z, x, T_PORT)
    if f.log:
        return np.abs(got - ref) / ((tol + EPS51 * (1.0 + np.abs(x))) * ref)
    return np.abs(got - ref) / tol


def _subset(f, k, z, x):
    pick = set(np.argsort(-np.abs(z))[:200].tolist())
    if f.bounded:
        pick.update(np.argsort(np.abs(x - f.low))[:200].tolist())
        pick.update(np.argsort(np.abs(f.high - x))[:200].tolist())
    pick.update(np.flatnonzero(f.width(k) <= 16).tolist())
    s = np.array(sorted(pick), dtype=np.int64)
    assert len(s) <= 2000
    return s


def check_draws(f, wp, wu, got, path, what):
    """The common rule over one case's draws."""
    got = np.asarray(got)
    assert np.all(np.isfinite(got)), what
    k, z, x, val = D.draw_fp64(f, wp, wu)
    assert not D.excluded(f, wp, wu, x).any(), what
    if f.categorical:
        assert np.array_equal(got, k), what
        return
    if f.bounded and f.q is None:
        lo, hi = (np.exp(f.low) * (1 - 1e-15), np.exp(f.high) * (1 + 1e-15)) if f.log else (f.low, f.high)
        assert np.all((got >= lo) & (got < hi)), what
    rp = ratio(f, k, z, x, got)
    s = _subset(f, k, z, x)
    ze, xe = D.draw_exact(f, k[s], wp[s], wu[s])
    re = ratio(f, k[s], ze, xe, got[s])
    w = WORST.setdefault(path, [0.0, 0.0])
    w[0], w[1] = float(np.fmax(w[0], rp.max())), float(np.fmax(w[1], re.max()))
    print('%s %s: %d draws, worst %.3g x T_port against the port, %.3g against the exact draw (%d)'
          % (path, what, len(got), rp.max(), re.max(), len(s)))
    bad = np.flatnonzero(~(rp <= T_DEV / T_PORT))
    assert len(bad) == 0, (what, 'port', bad[:5].tolist(), got[bad[:5]].tolist(), val[bad[:5]].tolist())
    bad = np.flatnonzero(~(re <= T_DEV / T_PORT))
    assert len(bad) == 0, (what, 'exact', s[bad[:5]].tolist(), got[s[bad[:5]]].tolist(), xe[bad[:5]].tolist())
