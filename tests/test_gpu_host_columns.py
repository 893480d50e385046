"""Ray-traced column densities of the C++ host loop on the GPU: the sources live on the device handle
(pion_gpu_add_rt_source), the columns are traced there from P after the boundary update (pion_gpu_raytrace) and leave
image after image, a chunk of planes at a time (pion_gpu_pack_columns through the staging slots of
pion_backend_gpu.cpp).  tests/test_host_columns.py holds the cases, the checks against the restatement and the CPU loop;
everything is compared with ==.  PION_SNAPSHOT_CHUNK_PLANES=3 makes the 8 planes (3-D) and 8 rows (2-D) of the cases
three chunks, the last one short."""
import pytest

from pion_amd import host_rccl
from test_host_columns import check_run, column_cases, nosetup
from test_host_snapshot import orc_loop

pytestmark = pytest.mark.gpu


class _GpuLoop:
    """the product's loop on device 0, as a context manager like the oracle-bound one"""

    def __init__(self, cfg, setup):
        self.s = host_rccl.HostSim(cfg, 0)

    def __enter__(self):
        return self.s

    def __exit__(self, *a):
        self.s.close()


@pytest.mark.parametrize("chunk", [None, "3"])
@pytest.mark.parametrize("name", ["box3d", "axi2d"])
def test_device_files_equal_the_restatement_and_the_cpu_files(name, chunk, tmp_path, monkeypatch):
    if chunk:
        monkeypatch.setenv("PION_SNAPSHOT_CHUNK_PLANES", chunk)
    (tmp_path / "gpu").mkdir()
    gpu = check_run(_GpuLoop, name, tmp_path / "gpu")
    # the strict build: the GPU's columns files are byte for byte the CPU loop's (same base name: the header holds it)
    for f in (tmp_path / "gpu").iterdir():
        f.unlink()
    cpu = check_run(orc_loop, name, tmp_path / "gpu")
    assert sorted(gpu) == sorted(cpu)
    for f in gpu:
        assert gpu[f] == cpu[f], f


def test_fast_build_writes_the_same_columns_for_the_same_state(tmp_path):
    """both builds trace with the same code object: from one uploaded state the files differ in pion_strict_fp only"""
    from pion_amd import fits
    import numpy as np
    images = {}
    for strict in (1, 0):
        cfg, P, sources = column_cases(strict)["box3d"]
        with _GpuLoop(cfg, nosetup) as s:
            for src in sources:
                s.add_rt_source(src)
            s.init(P)
            path = str(tmp_path / ("c%d.fits" % strict))
            s.write_columns(path)
            images[strict] = fits.read(path)[1]
    assert list(images[0]) == list(images[1])
    for n in images[1]:
        assert np.array_equal(images[0][n], images[1][n]), n
