"""bench.py --dump-outputs: what dump_outputs writes, on arrays laid out like the GPU state ([nvar][z][y][x] with
ghost cells) -- the whole grid when it fits, the same seeded sample from one rank or from z-slabs over four ranks,
ghost cells never read, float64 files only."""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


class _Sim:
    def __init__(self, A):
        self.A = A

    def download(self, which=0):
        assert which == 0
        return self.A.copy()


class _Gather:
    """all_gather_object across ranks that are run one after another, rank 0 last"""

    def __init__(self, world):
        self.parts = [None] * world
        self.rank = None

    def all_gather_object(self, every, part):
        self.parts[self.rank] = part
        every[:] = self.parts


def _grid(nvar=3, nx=6, ny=5, nz=8, nb=2, ndim=3, seed=5):
    """the interior of the global grid, and a function cutting rank r's array (ghost cells = NaN) out of it"""
    G = np.random.default_rng(seed).standard_normal((nvar, nz, ny, nx))

    def rank_array(r, world):
        nzl = nz // world
        bz = nb if ndim == 3 else 0
        A = np.full((nvar, nzl + 2 * bz, ny + 2 * nb, nx + 2 * nb), np.nan)
        A[:, bz:bz + nzl, nb:nb + ny, nb:nb + nx] = G[:, r * nzl:(r + 1) * nzl]
        cfg = types.SimpleNamespace(nbc=nb, ndim=ndim, ng=[nx, ny, nzl], nvar=nvar)
        return A, cfg
    return G, types.SimpleNamespace(ng=[nx, ny, nz]), rank_array


def _dump(tmp, world, G, cfg_g, rank_array, dt=0.25):
    d = str(tmp / ("w%d" % world))
    gather = _Gather(world)
    for r in reversed(range(world)):
        A, cfg = rank_array(r, world)
        gather.rank = r
        bench.dump_outputs(d, _Sim(A), cfg, cfg_g, r, world, dt, gather if world > 1 else None)
    out = {}
    for f in sorted(os.listdir(d)):
        a = np.load(os.path.join(d, f))
        assert a.dtype == np.float64, f
        out[f[:-4]] = a
    return out


def test_whole_grid_when_it_fits(tmp_path):
    G, cfg_g, rank_array = _grid()
    out = _dump(tmp_path, 1, G, cfg_g, rank_array)
    assert sorted(out) == ["dt", "state_max", "state_min", "state_sample", "state_sample_cells", "state_sum"]
    assert np.array_equal(out["state_sample_cells"], np.arange(G[0].size))
    assert np.array_equal(out["state_sample"], G.reshape(G.shape[0], -1))
    assert np.allclose(out["state_sum"], G.reshape(G.shape[0], -1).sum(axis=1), rtol=1e-14, atol=1e-14)
    assert np.array_equal(out["state_min"], G.reshape(G.shape[0], -1).min(axis=1))
    assert np.array_equal(out["state_max"], G.reshape(G.shape[0], -1).max(axis=1))
    assert np.array_equal(out["dt"], [0.25])


def test_sample_is_seeded_and_the_same_over_slabs(tmp_path, monkeypatch):
    nvar = 3
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * (nvar + 1) * 50)   # 50 of the 240 cells
    G, cfg_g, rank_array = _grid(nvar=nvar)
    one = _dump(tmp_path, 1, G, cfg_g, rank_array)
    four = _dump(tmp_path, 4, G, cfg_g, rank_array)
    cells = one["state_sample_cells"].astype(np.int64)
    assert cells.size == 50 and np.all(np.diff(cells) > 0)
    assert np.array_equal(one["state_sample"], G.reshape(nvar, -1)[:, cells])
    for k in ("state_sample", "state_sample_cells", "state_min", "state_max", "dt"):
        assert np.array_equal(one[k], four[k]), k
    assert np.allclose(one["state_sum"], four["state_sum"], rtol=1e-14, atol=1e-14)
    again = _dump(tmp_path / "again", 1, G, cfg_g, rank_array)
    assert all(np.array_equal(one[k], again[k]) for k in one)


def test_two_d_grid(tmp_path):
    G, cfg_g, rank_array = _grid(nz=1, ndim=2)
    out = _dump(tmp_path, 1, G, cfg_g, rank_array)
    assert np.array_equal(out["state_sample"], G.reshape(G.shape[0], -1))
