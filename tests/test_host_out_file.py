"""The file object of the C++ host loop's writers (pion_amd/host/out_file.h) where its rename fails, on the CPU over
the oracle's backend table: the target path is a non-empty directory, so the ".part" file is written whole and cannot
take the target's place.  Every writer answers "<writer>: cannot rename to ...", leaves no ".part" name behind, and
the same sim then writes to a fresh path the file it wrote before the failure, byte for byte."""
import os

import pytest

import projection_restate as pr
from test_host_columns import column_cases, nosetup
from test_host_snapshot import orc_loop


@pytest.mark.parametrize("writer", ["write_snapshot", "write_fits", "write_projection", "write_columns"])
def test_failed_rename_leaves_no_part_file_and_the_sim_writes_on(writer, tmp_path):
    cfg, P, sources = column_cases()["box3d"]   # 12 x 10 x 8, one tracer
    with orc_loop(cfg, nosetup) as s:
        s.add_rt_source(sources[0])
        s.init(P)
        args = (2, pr.fields_of(cfg)[:2]) if writer == "write_projection" else ()
        write = lambda name: getattr(s, writer)(str(tmp_path / name), *args)
        write("before")
        (tmp_path / "target").mkdir()
        (tmp_path / "target" / "kept").write_text("x")
        with pytest.raises(RuntimeError, match=writer + ": cannot rename to"):
            write("target")
        assert sorted(os.listdir(tmp_path)) == ["before", "target"]
        assert os.listdir(tmp_path / "target") == ["kept"]
        write("after")
    assert sorted(os.listdir(tmp_path)) == ["after", "before", "target"]
    assert (tmp_path / "after").read_bytes() == (tmp_path / "before").read_bytes()
