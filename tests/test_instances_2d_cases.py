"""The case table of instances_2d_cases.py on the oracle alone (no GPU): what test_gpu_instances_2d.py runs the device on.

  * The table matches the dispatch: the solver labels of PION_SOLVER_CASES_HD / _MHD and the tracer labels of every
    `switch (a.ntracer)` in kernels_fp.hip, and the `specialise` expression of stage_rows2_go_z and stage_rows2_go_cyl
    (stage_rows2.h), are read from the sources.  A solver, tracer count or specialisation added to the dispatch without
    a row in the table fails here, so the sweep cannot silently become partial.
  * The oracle runs every case: three steps, strict configuration, finite, rho and p positive, no error raised.
  * Every case is well conditioned for the reference: every input value moved by -1, 0 or +1 ulp (seeded) and the
    oracle rerun on the unperturbed run's time steps changes the result after three steps by at most 5e-12 of each
    variable's largest magnitude.  This is what makes a cell-wise gate on the fast build mean something (compare
    test_reference_conditioning.py); it is a condition on the inputs, not a tolerance on a kernel.  A case that
    breaks the cap gets other data (a weaker blast, fewer steps), noted in the table -- not another cap."""
import functools
import os
import re

import numpy as np
import pytest

import instances_2d_cases as ic
from cpu_backends import CpuSim
from pion_amd import abi, driver

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pion_amd", "csrc")
CASES = list(ic.all_cases())
IDS = [ic.case_id(*c) for c in CASES]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _macro_body(src, name):
    """the text of a multi-line #define: from its name to the first line that does not end in a backslash"""
    m = re.search(r"#define\s+%s\b(.*?[^\\])\n" % re.escape(name), src, re.S)
    assert m, name
    return m.group(1)


def _case_labels(text):
    return [int(x) for x in re.findall(r"\bcase\s+(\d+)\s*:", text)]


def _function_body(src, start):
    """the brace-balanced body that follows position `start`"""
    i = src.index("{", start)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[i:j + 1]
        j += 1


def _specialised_pairs(src, fn):
    """the (equation set, solver) pairs for which the `specialise` expression of function fn is true, over every
    pair the dispatch instantiates: the C++ expression evaluated with the ABI's values"""
    m = re.search(r"static\s+int\s+%s\s*\(" % fn, src)
    assert m, fn
    body = _function_body(src, m.end())
    e = re.search(r"constexpr\s+bool\s+specialise\s*=(.*?);", body, re.S)
    assert e, fn
    expr = " ".join(e.group(1).split()).replace("&&", " and ").replace("||", " or ")
    expr = re.sub(r"!(?!=)", " not ", expr)
    names = {k: getattr(abi, k) for k in dir(abi) if k.startswith("FLUX_") or k.startswith("EQ")}
    assert set(re.findall(r"[A-Za-z_]\w*", expr)) <= set(names) | {"SOLVER", "EQ", "and", "or", "not"}, expr
    out = []
    for eq in ic.EQS:
        for solver in ic.solvers(eq):
            if eval(expr, {"__builtins__": {}}, dict(names, EQ=eq, SOLVER=solver)):
                out.append((eq, solver))
    return out


def test_solver_and_tracer_tables_match_the_dispatch():
    src = _read("kernels_fp.hip")
    assert _case_labels(_macro_body(src, "PION_SOLVER_CASES_HD")) == ic.HD_SOLVERS
    assert _case_labels(_macro_body(src, "PION_SOLVER_CASES_MHD")) == ic.MHD_SOLVERS
    # which table each equation set's object uses
    sel = re.findall(r"#define\s+PION_EQ\s+(\w+)\s*\n\s*#define\s+PION_CASES\s+(\w+)", src)
    assert sorted(sel) == sorted([("EQEUL", "PION_SOLVER_CASES_HD"), ("EQMHD", "PION_SOLVER_CASES_MHD"),
                                  ("EQGLM", "PION_SOLVER_CASES_MHD")]), sel
    assert ic.solvers(abi.EQEUL) == ic.HD_SOLVERS
    assert ic.solvers(abi.EQMHD) == ic.MHD_SOLVERS and ic.solvers(abi.EQGLM) == ic.MHD_SOLVERS
    # the tracer switch of every launcher of the full build (the probe build's launcher has none)
    switches = [m.end() for m in re.finditer(r"switch\s*\(\s*a\.ntracer\s*\)", src)]
    stage = [m.end() for m in re.finditer(r"int\s+PION_CAT\(launch_stage_,\s*PION_SUFFIX\)", src)]
    assert len(stage) == 2 and len(switches) >= 1
    in_stage = 0
    for pos in switches:
        body = _function_body(src, pos)
        labels = _case_labels(re.sub(r"PION_CASES\(.*?\)", "", body))
        assert labels == ic.NTR, (src[:pos].count("\n") + 1, labels)
        in_stage += any(pos > s and "PION_CASES(stage_go" in body for s in stage)
    assert in_stage == 1, "launch_stage_* has no a.ntracer switch over stage_go"


@pytest.mark.parametrize("fn", ["stage_rows2_go_z", "stage_rows2_go_cyl"])
def test_flavours_match_the_specialised_instances(fn):
    pairs = _specialised_pairs(_read("stage_rows2.h"), fn)
    assert sorted(pairs) == sorted(ic.SPECIALISED)
    for eq in ic.EQS:
        for solver in ic.solvers(eq):
            want = ["plain", "hcorr"] if (eq, solver) in pairs else ["plain"]
            assert ic.flavours(eq, solver) == want, (eq, solver)


def test_table_is_the_full_product():
    assert len(CASES) == 132 and len(set(IDS)) == 132
    plain = [c for c in CASES if c[4] == "plain"]
    hcorr = [c for c in CASES if c[4] == "hcorr"]
    assert len(plain) == 2 * (8 + 5 + 5) * 3 and len(hcorr) == 2 * 4 * 3
    for geom in ic.GEOMS:
        for eq in ic.EQS:
            for solver in ic.solvers(eq):
                for ntr in ic.NTR:
                    for fl in ic.flavours(eq, solver):
                        assert (geom, eq, solver, ntr, fl) in CASES
    # the cylindrical instances of one build: plain = SO 1 and SO 2 instances, hcorr / not specialised = the SO 0 one
    ncyl = sum((3 if (eq, s) in ic.SPECIALISED else 1) * len(ic.NTR) for eq in ic.EQS for s in ic.solvers(eq))
    assert ncyl == 78


def test_case_shapes_and_tracers():
    for geom, eq, solver, ntr, fl in CASES:
        cfg, P = ic.case(geom, eq, solver, ntr, fl, 1)
        assert [cfg.ng[0], cfg.ng[1]] == ([70, 35] if geom == "cyl" else [70, 19]) and cfg.ndim == 2
        assert (cfg.eqntype, cfg.solver, cfg.ntracer, cfg.strict_fp) == (eq, solver, ntr, 1)
        assert cfg.artvisc == (abi.AV_HCORR_FKJ98 if fl == "hcorr" else abi.AV_FKJ98_1D)
        base = cfg.nvar - ntr
        for t in range(ntr):
            assert sorted(np.unique(P[base + t]).tolist()) == sorted([1.0 - 0.25 * t, 0.1 * t])
        if ntr == 2:
            assert not np.array_equal(P[base], P[base + 1])
    assert ic.case("cart", abi.EQGLM, 7, 1, "plain", 0)[0].strict_fp == 0
    with pytest.raises(KeyError):
        ic.case("cart", abi.EQEUL, abi.FLUX_RS_HLL, 0, "hcorr", 1)


def _oracle(cfg, P, dts=None):
    """NSTEPS steps of the oracle; with dts, on those time steps (as run_pair of test_gpu_parity.py hands the
    device's step to the oracle)"""
    out = []
    with CpuSim(cfg, "orc") as o:
        sc = driver.SimControl(o, cfg)
        sc.init(P)
        for it in range(ic.NSTEPS):
            sc.calculate_timestep()
            if dts is not None:
                sc.dt = dts[it]
            out.append(sc.dt)
            sc.advance_time()
        return o.download(0).copy(), out


@functools.lru_cache(maxsize=None)
def _unperturbed(i):
    cfg, P = ic.case(*CASES[i], 1)
    A, dts = _oracle(cfg, P)
    A.setflags(write=False)
    return cfg, P, A, tuple(dts)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_oracle_runs_the_case(i):
    cfg, P, A, dts = _unperturbed(i)
    assert all(np.isfinite(dt) and dt > 0.0 for dt in dts), dts
    assert np.isfinite(A).all()
    assert (A[abi.RO] > 0.0).all() and (A[abi.PG] > 0.0).all()
    assert not np.array_equal(A[:, 0, 2:-2, 2:-2], P[:, 0]), "three steps changed nothing"


def _ulp_perturbed(P, seed):
    step = np.random.default_rng(seed).integers(-1, 2, P.shape)
    Q = np.where(step > 0, np.nextafter(P, np.inf), np.where(step < 0, np.nextafter(P, -np.inf), P))
    assert (step == 0).any() and (Q != P).any()
    return Q


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_case_is_well_conditioned(i):
    cfg, P, A, dts = _unperturbed(i)
    B, _ = _oracle(cfg, _ulp_perturbed(P, 20 + i), dts)
    scale = np.abs(A).reshape(cfg.nvar, -1).max(axis=1).reshape(-1, 1, 1, 1) + 1e-300
    s = float((np.abs(A - B) / scale).max())
    print("%s: 1 ulp in -> %.3g out" % (IDS[i], s))
    assert s <= ic.CONDITIONING_CAP, s
