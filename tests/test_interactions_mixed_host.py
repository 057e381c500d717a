"""The axis helper of tpe.interactions(mixed=True) against the cells the project already tests, and
tests/interaction_mixed_reference.py's quantized and categorical factors against the joint references'."""
import numpy as np
import pytest

from hyperopt_amd import posterior as P
from tests import interaction_mixed_reference as MR
from tests import joint_cat_reference as CR
from tests import joint_quant_reference as QR

OBS = np.array([0.0, 0.5, 3.0, 41.0])   # (the 0 for qlognormal alone: its transform floors it)
LABELS = [('uniform', dict(low=-5.0, high=5.0)), ('lognormal', dict(mu=0.0, sigma=1.0)),
          ('quniform', dict(low=-5.0, high=5.0, q=0.25)), ('qlognormal', dict(mu=0.0, sigma=1.0, q=0.5)),
          ('qloguniform', dict(low=-1.0, high=3.0, q=1.0)), ('randint', dict(upper=5)),
          ('categorical', dict(upper=3, p=[0.2, 0.3, 0.5]))]


@pytest.mark.parametrize('kind,args', LABELS)
@pytest.mark.parametrize('n_grid', (1, 16, 40))
def test_axis_record_is_the_cells_the_project_defines(kind, args, n_grid):
    obs = OBS if kind == 'qlognormal' else OBS[1:]
    ax = P.interaction_axis_record(kind, args, obs, n_grid)
    if kind in P.JOINT_KINDS:
        y, h = P.interaction_axis(kind, args, obs, n_grid)
        assert ax.kind == MR.DENSE and np.array_equal(ax.x, y) and ax.measure == h and not ax.upper and ax.step == 0.0
    else:
        x, w, merge = P.importance_cells(kind, args, obs, n_grid)
        assert np.array_equal(ax.x, x) and ax.measure == 1.0 and np.all(w == 1.0)
        if kind in P.JOINT_CAT_KINDS:
            assert ax.kind == MR.CATEGORICAL and ax.upper == len(x) == args['upper'] and merge == 1
            assert np.array_equal(ax.p, P.joint_cat_prior(kind, args)[1])
        else:
            assert ax.kind == MR.QUANTIZED and ax.step == merge * args['q'] and ax.log == kind.startswith('qlog')
            assert len(x) <= n_grid
    pri = P.joint_prior(kind, args, quantized=True, categorical=True)
    want = (pri.low, pri.high) if pri.bounded else (np.nan, np.nan)
    assert np.array_equal([ax.low, ax.high], want, equal_nan=True)


def test_reference_factors_are_the_joint_references():
    rng = np.random.RandomState(5)
    K = 6
    W = np.full(K, 1.0 / K)
    for kind, args in LABELS[2:5]:
        ax = P.interaction_axis_record(kind, args, OBS, 64)
        mu, s = rng.normal(size=K), rng.uniform(0.2, 2.0, size=K)
        dim = QR.QDim(ax.log, ax.low if ax.low == ax.low else None, ax.high if ax.high == ax.high else None, 0, q=ax.step)
        ref = QR.JointQuantRef([dim], (W, mu[:, None], s[:, None]), (W, mu[:, None], s[:, None]))
        e, _ = ref.log_terms(ax.x[:, None], 'below')
        got, _ = MR.quantized_factor(ax, mu, s)
        np.testing.assert_allclose(W[:, None] * got, np.exp(e).T, rtol=1e-12, atol=1e-300)
    for kind, args in LABELS[5:]:
        ax = P.interaction_axis_record(kind, args, OBS, 64)
        obs = np.concatenate([[0.0], rng.randint(ax.upper, size=K - 1)])
        dim = CR.CDim(False, None, None, 0, upper=ax.upper, p=ax.p)
        ref = CR.JointCatRef([dim], (W, obs[:, None], np.ones((K, 1))), (W, obs[:, None], np.ones((K, 1))), 0.7)
        assert np.array_equal(MR.categorical_factor(ax, obs, 0.7), ref.rows('below', 0))
