"""Case table of the per-instance sweep of the 2-D stage kernels (no GPU needed to import or build a case).

One row per template instance that a 2-D grid can reach: equation set x Riemann solver x tracer count, on a Cartesian
grid (the 3-D instance of k_stage_rows2 down its run-time `noz` path) and on a cylindrical (z,R) grid (the CYL
instances), each in the flavours that stage_rows2_go_z / stage_rows2_go_cyl make separate instances of:

  "plain"  a second-order step = the SO=1 instance in the half stage, the SO=2 instance in the full stage (for the
           solvers that are not specialised: the one SO=0 instance in both);
  "hcorr"  artvisc = AV_HCORR_FKJ98: the non-plain instances (cylindrical: SO=0 in both stages), for Euler Roe-CV
           also the H-correction prepass.  Only the specialised (equation set, solver) pairs have it.

The same cases run the cell-per-thread kernel k_stage (PION_STAGE_KERNEL=cell, PION_ROWS_2D=0), whose instances are
templates on the same (equation set, tracer count, solver).

Shapes: 70 x 35 (cylindrical) and 70 x 19 (Cartesian) are the smallest in the suite that run one full 62-cell x tile
and the packed remainder wavefront (8 cells) in one launch; 35 and 19 rows are no multiple of any rows-per-wavefront
choice.

Used by test_instances_2d_cases.py (oracle alone: the table matches the dispatch, every case runs and is well
conditioned) and test_gpu_instances_2d.py (both kernels of both builds against the oracle).

Per-case gates: every case uses the project's gates (GATE_FAST, GATE_LIBM); CASE_GATES holds the exceptions with the
measurements behind them -- none at present."""
import numpy as np

from pion_amd import abi, problems

HD_SOLVERS = [0, 1, 2, 3, 4, 5, 6, 8]
MHD_SOLVERS = [0, 1, 4, 7, 8]
NTR = [0, 1, 2]
GEOMS = ["cart", "cyl"]
EQS = [abi.EQEUL, abi.EQMHD, abi.EQGLM]
EQ_NAMES = {abi.EQEUL: "hd", abi.EQMHD: "mhd", abi.EQGLM: "glm"}
SOLVER_NAMES = {0: "lf", 1: "linear", 2: "exact", 3: "hybrid", 4: "roe", 5: "roepv", 6: "fvs", 7: "hlld", 8: "hll"}

# (equation set, solver) pairs with compile-time spatial order and a separate "plain" instance
# (the `specialise` expression of stage_rows2_go_z and stage_rows2_go_cyl)
SPECIALISED = [(abi.EQEUL, abi.FLUX_RSroe), (abi.EQEUL, abi.FLUX_FVS), (abi.EQMHD, abi.FLUX_RS_HLLD),
               (abi.EQGLM, abi.FLUX_RS_HLLD)]

# Euler linear / exact / hybrid: exp, log and pow of the device maths library differ from glibc in the last bits
LIBM_SOLVERS = (abi.FLUX_RSlinear, abi.FLUX_RSexact, abi.FLUX_RShybrid)

NSTEPS = 3
CART_NG = [70, 19]
CYL_N = 70

# the project's gates (tests/test_gpu_xtile.py, tests/test_gpu_parity.py)
GATE_FAST = 3e-11        # fast build against the oracle, of each variable's scale
GATE_LIBM = 1e-9         # both builds, Euler solvers 1, 2, 3 (test_hd_exact_hybrid)
GATE_ROWS_VS_CELL = 1e-12
# 1-ulp amplification of the oracle over NSTEPS steps that a case may have (a condition on the inputs)
CONDITIONING_CAP = 5e-12

# case id -> (gate, fast-build error measured against the oracle, the case's 1-ulp amplification, the best-conditioned
# case's): a case whose fast-build rounding alone exceeds GATE_FAST while rows-vs-cell and the strict run hold
CASE_GATES = {}


def solvers(eq):
    return HD_SOLVERS if eq == abi.EQEUL else MHD_SOLVERS


def flavours(eq, solver):
    return ["plain", "hcorr"] if (eq, solver) in SPECIALISED else ["plain"]


def uses_libm(eq, solver):
    return eq == abi.EQEUL and solver in LIBM_SOLVERS


def case_id(geom, eq, solver, ntr, flavour):
    return "%s-%s-%s-tr%d-%s" % (geom, EQ_NAMES[eq], SOLVER_NAMES[solver], ntr, flavour)


def all_cases():
    """(geom, eq, solver, ntr, flavour): 2 x (8 + 5 + 5) x 3 plain + 2 x 4 x 3 hcorr = 132"""
    for geom in GEOMS:
        for eq in EQS:
            for solver in solvers(eq):
                for ntr in NTR:
                    for flavour in flavours(eq, solver):
                        yield geom, eq, solver, ntr, flavour


def fast_gate(geom, eq, solver, ntr, flavour):
    cid = case_id(geom, eq, solver, ntr, flavour)
    if cid in CASE_GATES:
        return CASE_GATES[cid][0]
    return GATE_LIBM if uses_libm(eq, solver) else GATE_FAST


def _distinct_tracers(cfg, P):
    """tracer t = 1 - 0.25 t inside the blast, 0.1 t outside (as _with_tracers of test_gpu_parity.py): two tracers
    never hold the same field, so swapped tracer registers cannot reproduce the answer"""
    base = cfg.nvar - cfg.ntracer
    hot = P[abi.PG] > 2.0 * P[abi.PG].min()
    for t in range(cfg.ntracer):
        P[base + t] = np.where(hot, 1.0 - 0.25 * t, 0.1 * t)
    return P


def case(geom, eq, solver, ntr, flavour, strict):
    """(cfg, P) of one row of the table"""
    if flavour not in flavours(eq, solver):
        raise KeyError((eq, solver, flavour))
    av = abi.AV_HCORR_FKJ98 if flavour == "hcorr" else abi.AV_FKJ98_1D
    if geom == "cyl":
        cfg, P = problems.blast_axi2d(CYL_N, eq, solver, ntracer=ntr, artvisc=av, strict_fp=strict)
    elif geom == "cart" and eq == abi.EQEUL:
        cfg, P = problems.hd_blast_box(CART_NG, solver=solver, ntracer=ntr, strict_fp=strict)
        cfg.artvisc = av
    elif geom == "cart":
        cfg, P = problems.mhd_blast_generic(CART_NG, eq, solver, strict_fp=strict, ntracer=ntr)
        cfg.artvisc = av
    else:
        raise KeyError(geom)
    return cfg, _distinct_tracers(cfg, P)
