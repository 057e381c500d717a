"""bench.py --dump-outputs / --full (CPU): the winners of a step are written
as float64 .npy files, a larger result as a fixed sample that is the same
from run to run, and the legs beyond the timed steps are off unless --full
is given."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402
from hyperopt_amd.engine import RESULT_DTYPE  # noqa: E402


def _records(shape, seed=0):
    rng = np.random.RandomState(seed)
    res = np.zeros(shape, dtype=RESULT_DTYPE)
    for f in ('value', 'score', 'lpdf_below', 'lpdf_above'):
        res[f] = rng.standard_normal(shape)
    res['index'] = rng.randint(0, 1 << 40, size=shape)
    return res


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_fields(tmp_path):
    res = _records((5, 7))
    bench.dump_outputs(str(tmp_path / 'vo'), res, value_only=1)
    got = _load(str(tmp_path / 'vo'))
    assert sorted(got) == ['index', 'value']
    bench.dump_outputs(str(tmp_path / 'all'), res, value_only=0)
    got = _load(str(tmp_path / 'all'))
    assert sorted(got) == ['index', 'lpdf_above', 'lpdf_below', 'score', 'value']
    for f, a in got.items():
        assert a.dtype == np.float64 and a.shape == (5, 7)
        assert np.array_equal(a, res[f].astype(np.float64))
    assert np.array_equal(got['index'].astype(np.int64), res['index'])   # (exact below 2^53)


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 16 * 100)   # room for 100 cells of two fields
    res = _records((40, 9))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), res, value_only=1)
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sum(x.nbytes for x in a.values()) <= 16 * 100
    for f in a:
        assert a[f].shape == (100,) and a[f].tobytes() == b[f].tobytes()
    # the sample keeps the cells' order and each cell's fields together
    flat = res.reshape(-1)
    pos = np.searchsorted(np.sort(flat['index']), a['index'].astype(np.int64))
    assert np.all(np.sort(flat['index'])[pos] == a['index'].astype(np.int64))
    cell = {int(i): float(v) for i, v in zip(flat['index'], flat['value'])}
    assert all(cell[int(i)] == v for i, v in zip(a['index'], a['value']))


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1'])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out'])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == 'out'
