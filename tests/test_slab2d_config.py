"""slab.slab_config / slab_slice on 2-D grids (no GPU): the slab axis of a 2-D grid is y.  Per rank: ng, xmin[1], the
face types (a middle rank has BC_SLAB on both y faces; the axis of a cylindrical grid and the internal DMR2 cells are
rank 0's alone, the DMACH face the last rank's), and the slices tile the on-grid rows of the global array."""
import numpy as np
import pytest

from pion_amd import abi, problems, slab


def _cases():
    cyl, Pc = problems.blast_axi2d(12, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)       # 12 x 6, axis / outflow
    per, Pp = problems.mhd_blastwave(12, 2, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)  # 12 x 12, periodic
    dmr, Pd = problems.double_mach_reflection(39, strict_fp=1)                         # 39 x 12, reflecting / DMACH
    return {"cyl": (cyl, Pc), "periodic": (per, Pp), "dmr": (dmr, Pd)}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", ["cyl", "periodic", "dmr"])
def test_slab_config_2d(case, world):
    cfg, P = _cases()[case]
    ny, nb = cfg.ng[1], cfg.nbc
    assert ny % world == 0
    nyl = ny // world
    periodic = case == "periodic"
    assert slab.slab_periodic(cfg) == periodic
    seen = np.zeros(ny, dtype=int)
    for r in range(world):
        c = slab.slab_config(cfg, r, world)
        assert c.ndim == 2 and c.ng[0] == cfg.ng[0] and c.ng[1] == nyl
        assert c.xmin[0] == cfg.xmin[0] and c.xmin[1] == cfg.xmin[1] + r * nyl * cfg.dx
        assert c.dx == cfg.dx and c.coord_sys == cfg.coord_sys
        # x faces untouched
        assert c.bc_type[0] == cfg.bc_type[0] and c.bc_type[1] == cfg.bc_type[1]
        lo_slab = periodic or r > 0
        hi_slab = periodic or r < world - 1
        assert c.bc_type[2] == (abi.BC_SLAB if lo_slab else cfg.bc_type[2])
        assert c.bc_type[3] == (abi.BC_SLAB if hi_slab else cfg.bc_type[3])
        if 0 < r < world - 1:
            assert c.bc_type[2] == abi.BC_SLAB and c.bc_type[3] == abi.BC_SLAB
        if case == "cyl":
            assert (c.bc_type[2] == abi.BC_AXISYMMETRIC) == (r == 0)
        if case == "dmr":
            assert c.bc_dmach2 == (1 if r == 0 else 0)
            assert (c.bc_type[3] == abi.BC_DMACH) == (r == world - 1)
        S = slab.slab_slice(P, cfg, r, world)
        assert S.shape == (cfg.nvar, 1, nyl + 2 * nb, cfg.ng[0] + 2 * nb)
        assert np.array_equal(S, P[:, :, r * nyl:r * nyl + nyl + 2 * nb])
        seen[r * nyl:(r + 1) * nyl] += 1
        # the on-grid rows of the slice are the global on-grid rows [r nyl, (r + 1) nyl)
        assert np.array_equal(S[:, :, nb:nb + nyl], P[:, :, nb + r * nyl:nb + (r + 1) * nyl])
    assert np.all(seen == 1)
    # the global configuration is left as it was
    assert cfg.ng[1] == ny


def test_slab_config_2d_errors():
    cfg, _ = problems.mhd_blastwave(10, 2, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)
    with pytest.raises(ValueError):
        slab.slab_config(cfg, 0, 3)          # 10 rows over 3 ranks
    c1 = abi.make_config(1, [16], abi.EQEUL, abi.FLUX_RSroe, xmin=(0.0, 0, 0), xmax=(1.0, 0, 0), bcs=["outflow"] * 2,
                         refvec=[1.0] * 5)
    with pytest.raises(ValueError):
        slab.slab_config(c1, 0, 2)           # 1-D grids have no slab axis


def test_torch_transport_refuses_2d():
    """the torch.distributed transport stays 3-D-only and says so where the grid is known: driver.SimControl refuses a
    SlabComm for a 2-D configuration before anything is exchanged, and takes it for a 3-D one"""
    from pion_amd import driver
    comm = slab.SlabComm(0, 2, True, 16, "cpu")          # the call shape every existing caller uses
    cfg2, _ = problems.mhd_blastwave(8, 2, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)
    with pytest.raises(NotImplementedError, match="3-D"):
        driver.SimControl(None, slab.slab_config(cfg2, 0, 2), comm=comm)
    cfg3, _ = problems.mhd_blastwave(8, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)
    assert driver.SimControl(None, slab.slab_config(cfg3, 0, 2), comm=comm).comm is comm


def test_slab_config_3d_unchanged():
    cfg, P = problems.mhd_blastwave(8, 3, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=1)
    c0 = slab.slab_config(cfg, 0, 2)
    assert c0.ng[2] == 4 and c0.ng[1] == 8 and c0.bc_type[4] == abi.BC_SLAB and c0.bc_type[5] == abi.BC_SLAB
    assert c0.bc_type[2] == abi.BC_PERIODIC and c0.bc_type[3] == abi.BC_PERIODIC
    assert slab.slab_slice(P, cfg, 1, 2).shape == (cfg.nvar, 4 + 2 * cfg.nbc, 8 + 2 * cfg.nbc, 8 + 2 * cfg.nbc)
