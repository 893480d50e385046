"""CPU test of the host part of the wind sources (pion_amd/csrc/wind_host.cpp) through tests/native/wind_host_probe,
a stand-alone program: set-up and update steps of a source, value for value (==) against the restatements of the
reference (tests/wind_restate.Source, tests/wind_angle_restate.Source), the pre-check of a rotating source, and every
EINVAL of the two entry points that needs no device, with its text.

PION_WIND_HOST_PROBE=<path> runs another build of the probe, e.g. tests/native/wind_host_probe_san (address and
undefined-behaviour sanitisers)."""
import copy
import math
import os
import subprocess

import numpy as np
import pytest

import wind_angle_restate as ar
import wind_restate as wr
from pion_amd import abi, wind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
WND = os.path.join(ROOT, "tests", "golden", "eta_car.wnd.txt")
MSUN_YR = 1.9891e33 / 3.1558150e7
CYL2 = (2, 2, abi.EQEUL, 1)      # ndim, coord_sys, eqntype, ntracer
CART3 = (3, 1, abi.EQEUL, 2)
TABLE_COLUMNS = ("time", "Teff", "Mdot", "vrot", "vinf", "R", "vcrit") + wind.ELEMENTS


def _probe():
    """the probe, built on demand (a second)"""
    exe = os.environ.get("PION_WIND_HOST_PROBE")
    if exe:
        return exe
    exe = os.path.join(NATIVE, "wind_host_probe")
    deps = [os.path.join(NATIVE, "wind_host_probe.cpp")] + [os.path.join(ROOT, "pion_amd", "csrc", f)
                                                             for f in ("wind_host.cpp", "wind_host.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["make", "-C", NATIVE, "wind_host_probe"])
    return exe


def _eta_car(time_offset=1.0e9):
    """tests/golden/eta_car.wnd.txt as read_evolution_file leaves it: 8 columns, R from L and Teff, no elements"""
    rows = np.array([[float(v) for v in line.split()] for line in open(WND).read().splitlines()[2:]
                     if line.split() and not line.startswith("#")])
    cols = {c: np.zeros(len(rows)) for c in wind.COLUMNS}
    for c, name in enumerate(wind.COLUMNS[:8]):
        cols[name] = rows[:, c].copy()
    cols["time"] = cols["time"] + time_offset
    cols["R"] = np.array([math.sqrt(L / (4.0 * wr.PI * 5.670367e-5 * math.exp(4.0 * math.log(T))))
                          for L, T in zip(cols["L"], cols["Teff"])])
    return wind.WindEvolution(cols)


def _three_rows(**kw):
    """a hand-made table: three rows, two element columns"""
    t = np.array([1.0e11, 3.0e11, 4.0e11])
    cols = {c: np.zeros(3) for c in wind.COLUMNS}
    cols.update(time=t, Teff=np.array([2.5e4, 3.0e4, 2.0e5]), Mdot=np.array([1.0e-6, 1.2e-6, 0.7e-6]) * MSUN_YR,
                vrot=np.array([1.5e7, 1.8e7, 0.9e7]), vcrit=np.array([3.0e7, 3.1e7, 2.9e7]),
                vinf=np.array([1.0e8, 0.9e8, 1.1e8]), R=np.array([7.0e11, 7.5e11, 6.5e11]),
                X_H=np.array([0.7, 0.6, 0.65]), X_He=np.array([0.28, 0.38, 0.33]))
    cols.update({k: np.array(v, float) for k, v in kw.items()})
    return wind.WindEvolution(cols)


def _src(cfg, type_, ev=None, t_now=0.0, update_freq=1.0e9, elements=None, **kw):
    ntr = cfg[3]
    a = dict(pos=(0.0, 0.0, 0.0) if cfg[1] != 1 else (1.0e15, -2.0e15, 3.0e15), radius=3.0e16, mdot=1.0e-6,
             vinf=1500.0, vrot=30.0, Tw=3.0e4, Rstar=7.0e11, Bstar=0.1, tracers=[0.5, 0.25][:ntr], type=type_,
             evolution=ev, elements=elements if elements is not None else [None] * ntr, t_now=t_now,
             update_freq=update_freq, xi=-0.43)
    a.update(kw)
    return wind.WindSource(**a)


def _case(cfg, src, rotating, times=(), present=(), xi_present=0.0, drop=(), elem=None):
    """the probe's input (tests/native/wind_host_probe.cpp); drop: columns handed over as null pointers; elem: the
    tracer selectors as numbers, where a bad one is wanted"""
    h = float.hex
    w = [str(v) for v in cfg] + [str(len(present))] + [str(p) for p in present] + [h(float(xi_present))]
    w += [str(int(rotating)), h(src.xi)] + [h(float(v)) for v in src.pos] + [h(float(src.radius)), str(src.type)]
    w += [h(float(v)) for v in (src.mdot, src.vinf, src.vrot, src.Tw, src.Rstar, src.Bstar, src.t_now,
                                src.update_freq) + src.orbit]
    ntr = cfg[3]
    w += [h(float(v)) for v in (src.tracers + [0.0] * ntr)[:ntr]]
    sel = elem if elem is not None else [-1 if e is None else wind.ELEMENTS.index(e) for e in src.elements]
    w += [str(v) for v in (list(sel) + [-1] * ntr)[:ntr]]
    ev = src.evolution
    w.append(str(ev.npt if ev is not None else 0))
    for c in TABLE_COLUMNS:
        if ev is None or c in drop:
            w.append("0")
        else:
            w += ["1"] + [h(float(v)) for v in ev.cols[c][:ev.npt]]
    w += [str(len(times))] + [h(float(t)) for t in times]
    return " ".join(w) + "\n"


def _run(text):
    """(rc, error text, [state tuples], [check flags]); a state: (active, t_next, Mdot, Vinf, vrot, vcrit, Tw, Rstar,
    [tracers])"""
    out = subprocess.run([_probe()], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.splitlines()
    head = lines[0].split(" ", 2)
    assert head[0] == "rc"
    states, checks = [], []
    for line in lines[1:]:
        f = line.split()
        if f[0] == "check":
            checks.append(int(f[1]))
        else:
            v = [float.fromhex(x) for x in f[2:]]
            states.append((int(f[1]),) + tuple(v[:7]) + (v[7:],))
    return int(head[1]), (head[2] if len(head) > 2 else ""), states, checks


def _expected(rs, ntracer):
    W = rs.W
    st = (int(rs.active), rs.t_next, W["Mdot"], W["Vinf"], W["v_rot"], W.get("vcrit", 0.0), W["Tw"], W["Rstar"],
          [float(v) for v in rs.tr[:ntracer]])
    flat = list(st[1:8]) + st[8]
    assert not any(math.isnan(v) for v in flat), "a case whose reference arithmetic gives NaN: compare bit patterns"
    return st


def _accepts(rs, t):
    """wind_angle_check for one rotating source: what update_source would leave, without changing the source"""
    c = copy.copy(rs)
    c.W, c.tr = dict(rs.W), list(rs.tr)
    if not c.update(t):
        return True
    with np.errstate(all="ignore"):
        omega = ar.cmin(ar.cmin(0.9999, float(np.float64(c.W["v_rot"]) / np.float64(c.W["vcrit"]))), 0.999)
    return bool(omega > c.T.omega[0] and c.W["Tw"] > c.T.Teff[0])


def _times(ev, uf):
    """across tstart and tfinish, one time twice"""
    t0, t1 = float(ev.time[0]), float(ev.time[-1])
    mid = 0.5 * (float(ev.time[1]) + float(ev.time[2]))
    return [t0 - 3.0 * uf, t0 - 0.5 * uf, t0, t0 + 0.25 * uf, t0 + 0.25 * uf, float(ev.time[1]), mid,
            t1 - 0.5 * uf, t1, t1 + uf, t1 + 40.0 * uf]


def _follow(cfg, src, rotating, times):
    rc, msg, states, checks = _run(_case(cfg, src, rotating, times))
    assert (rc, msg) == (0, "")
    rs = (ar.Source if rotating else wr.Source)(src, cfg[3])
    assert len(states) == len(times) + 1 and len(checks) == len(times)
    assert states[0] == _expected(rs, cfg[3]), ("set-up", states[0], _expected(rs, cfg[3]))
    for k, t in enumerate(times):
        ok = _accepts(rs, t) if rotating else True
        assert checks[k] == int(ok), (k, t)
        if ok:
            rs.update(t)
        assert states[k + 1] == _expected(rs, cfg[3]), (k, t, states[k + 1], _expected(rs, cfg[3]))
    return rs, states, checks


TABLES = {"eta_car": (CYL2, _eta_car, [None]), "three_rows": (CART3, _three_rows, ["X_He", None])}


@pytest.mark.parametrize("when", ["inside", "long_before", "just_before", "at_tfinish", "after_tfinish"])
@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("type_", [wind.EVOLVING, wind.ANGLE])
def test_setup_and_updates_equal_the_restatement(type_, table, when):
    cfg, make, elements = TABLES[table]
    ev = make()
    t0, t1, uf = float(ev.time[0]), float(ev.time[-1]), 1.0e8
    t_now = {"inside": 0.5 * (float(ev.time[1]) + float(ev.time[2])), "long_before": t0 - 2.5 * uf,
             "just_before": t0 - 0.5 * uf, "at_tfinish": t1, "after_tfinish": t1 + 7.0 * uf}[when]
    src = _src(cfg, type_, ev=ev, t_now=t_now, update_freq=uf, elements=elements)
    rs, states, checks = _follow(cfg, src, type_ == wind.ANGLE, _times(ev, uf))
    active0 = states[0][0]
    assert active0 == int(when in ("inside", "just_before"))
    if not active0:
        # the sentinels of an inactive source, per kind
        if type_ == wind.EVOLVING:
            assert states[0][2:8] == (-100.0 * 1.9891e33 / 3.1558150e7, -100.0 * 1.0e5, 0.0, 0.0, -100.0, 0.0)
        else:
            assert states[0][2:8] == (-100.0, -100.0, -100.0, 0.0, -100.0, 0.0)
    assert states[-1][0] == 1 and all(checks)          # every source has started by the last time
    # clamped after tfinish: the table at tfinish, cgs, no conversion
    t = list(ev.time)
    assert states[-1][2] == wr.root_find_linear_vec(t, ev.Mdot, t1) and abs(states[-1][2] / ev.Mdot[-1] - 1.0) < 1e-15
    if table == "three_rows":
        # the element tracer follows its column, the other stays
        assert states[-1][8] == [wr.root_find_linear_vec(t, ev.X_He, t1), 0.25]
        if type_ == wind.ANGLE:
            assert states[-1][6] == 150000.0           # Tw = min(Tw, Teff_vec.back())


def test_constant_source():
    for cfg in (CYL2, CART3, (1, 3, abi.EQEUL, 1)):
        src = _src(cfg, wind.CONSTANT)
        rs, states, _ = _follow(cfg, src, False, [0.0, 1.0e10, 1.0e10, 1.0e12])
        assert states[0] == states[-1] and states[0][:2] == (1, 1.0e99)
        assert states[0][2:5] == (1.0e-6 * 1.9891e33 / 3.1558150e7, 1500.0 * 1.0e5, 30.0 * 1.0e5)
    # an orbit on a Cartesian grid is accepted
    assert _run(_case(CART3, _src(CART3, wind.CONSTANT, orbit=(1.2, 1.0e15, 1.0e14, 1.0)), False))[0] == 0


@pytest.mark.parametrize("bad", ["omega", "Tw"])
def test_precheck_refuses_what_the_tables_cannot_evaluate(bad):
    """as test_update_error_writes_nothing of tests/test_gpu_wind_angle.py builds them"""
    kw = dict(vrot=(0.0, 0.0)) if bad == "omega" else dict(Teff=(900.0, 900.0))
    two = dict(time=(-1.0e12, 1.0e12), Teff=(2.5e4, 3.0e4), Mdot=(1.0e-6 * MSUN_YR, 1.2e-6 * MSUN_YR),
               vrot=(1.5e7, 1.8e7), vcrit=(3.0e7, 3.0e7), vinf=(1.0e8, 0.9e8), R=(7.0e11, 7.0e11), X_H=(0.7, 0.7),
               X_He=(0.28, 0.28))
    two.update(kw)
    ev = _three_rows(**two)
    src = _src(CART3, wind.ANGLE, ev=ev, t_now=0.0, update_freq=1.0, elements=["X_H", None])
    rs, states, checks = _follow(CART3, src, True, [1.0e11, 1.0e11, 2.0e12])
    assert checks == [0, 0, 0]
    assert states[0] == states[-1]                     # a refused update leaves the source as set-up left it
    # the same table with good values is accepted
    good = _three_rows(**dict(two, vrot=(1.5e7, 1.8e7), Teff=(2.5e4, 3.0e4)))
    _, _, checks = _follow(CART3, _src(CART3, wind.ANGLE, ev=good, update_freq=1.0, elements=["X_H", None]), True,
                           [1.0e11, 2.0e12])
    assert checks == [1, 1]


LIMIT = "wind source: at most PION_MAX_WIND_SOURCES sources"
ANGLE_PLAIN = "wind source: angle / latitude-dependent winds are not supported"
WHAT_TYPE = "What type of source is this?  add a new type?"
MIXED = "wind source: evolving and rotating sources cannot share a grid"
RADIUS = "wind source: radius must be > 0"
ORIGIN = "Spherical symmetry but source not at origin!"
AXIS = "Axisymmetry but source not at R=0!"
MHD_1D = "1D spherical but MHD?"
ORBIT = "wind source: orbital motion needs a 2-D or 3-D Cartesian grid"
ROWS = "evolving wind source: the table needs at least 2 rows"
COLUMN = "evolving wind source: missing table column"
SELECTOR = "evolving wind source: bad tracer selector"
BAD_TYPE = "Bad wind type for evolving stellar wind (rotating star)!"
ROT_1D = "rotating wind source: needs a 2-D or 3-D grid (theta = 0 in 1-D)"
ROT_ORBIT = "rotating wind source: add_rotating_source takes no orbit"
XI = "rotating wind source: xi differs from an earlier source's"
SPH1, CART1_MHD = (1, 3, abi.EQEUL, 1), (1, 1, abi.EQMHD, 1)
AN_ORBIT = (1.2, 1.0e15, 1.0e14, 1.0)


def _one_row():
    ev = _three_rows()
    return wind.WindEvolution({k: v[:1].copy() for k, v in ev.cols.items()})


def _einval_cases():
    """(id, expected text, cfg, source, rotating entry point, keywords of _case)"""
    ev, E, A, C = _three_rows(), wind.EVOLVING, wind.ANGLE, wind.CONSTANT
    el = ["X_He", None]
    c = [
        ("limit", LIMIT, CART3, _src(CART3, C), False, dict(present=[0] * 8)),
        ("limit_rotating", LIMIT, CART3, _src(CART3, A, ev=ev, elements=el), True, dict(present=[0] * 8)),
        ("type2_plain", ANGLE_PLAIN, CART3, _src(CART3, A, ev=ev, elements=el), False, {}),
        ("type3_plain", ANGLE_PLAIN, CART3, _src(CART3, 3), False, {}),
        ("unknown_type", WHAT_TYPE, CART3, _src(CART3, 7), False, {}),
        ("negative_type", WHAT_TYPE, CART3, _src(CART3, -1), False, {}),
        ("evolving_beside_rotating", MIXED, CART3, _src(CART3, E, ev=ev, elements=el), False,
         dict(present=[0, 2], xi_present=-0.43)),
        ("rotating_beside_evolving", MIXED, CART3, _src(CART3, A, ev=ev, elements=el), True, dict(present=[1, 0])),
        ("radius_zero", RADIUS, CART3, _src(CART3, C, radius=0.0), False, {}),
        ("radius_negative_rotating", RADIUS, CART3, _src(CART3, A, ev=ev, elements=el, radius=-1.0), True, {}),
        ("radius_nan", RADIUS, CART3, _src(CART3, C, radius=float("nan")), False, {}),
        ("off_origin", ORIGIN, SPH1, _src(SPH1, C, pos=(1.0e15, 0.0, 0.0)), False, {}),
        ("off_axis", AXIS, CYL2, _src(CYL2, C, pos=(0.0, 1.0e15, 0.0)), False, {}),
        ("off_axis_rotating", AXIS, CYL2, _src(CYL2, A, ev=_eta_car(), pos=(0.0, 1.0e15, 0.0)), True, {}),
        ("mhd_1d", MHD_1D, CART1_MHD, _src(CART1_MHD, C), False, {}),
        ("orbit_cylindrical", ORBIT, CYL2, _src(CYL2, C, orbit=AN_ORBIT), False, {}),
        ("orbit_1d", ORBIT, (1, 1, abi.EQEUL, 1), _src((1, 1, abi.EQEUL, 1), C, pos=(1.0e15, 0, 0), orbit=AN_ORBIT),
         False, {}),
        ("one_row", ROWS, CART3, _src(CART3, E, ev=_one_row(), elements=el), False, {}),
        ("one_row_rotating", ROWS, CART3, _src(CART3, A, ev=_one_row(), elements=el), True, {}),
        ("no_vcrit", COLUMN, CART3, _src(CART3, A, ev=ev, elements=el), True, dict(drop=("vcrit",))),
        ("selector_out_of_range", SELECTOR, CART3, _src(CART3, E, ev=ev, elements=el), False, dict(elem=[7, -1])),
        ("selector_below", SELECTOR, CART3, _src(CART3, A, ev=ev, elements=el), True, dict(elem=[-1, -2])),
        ("selector_null_column", SELECTOR, CART3, _src(CART3, E, ev=ev, elements=el), False, dict(drop=("X_He",))),
        ("wrong_type_rotating", BAD_TYPE, CART3, _src(CART3, E, ev=ev, elements=el), True, {}),
        ("rotating_1d", ROT_1D, SPH1, _src(SPH1, A, ev=_eta_car()), True, {}),
        ("rotating_orbit", ROT_ORBIT, CART3, _src(CART3, A, ev=ev, elements=el, orbit=AN_ORBIT), True, {}),
        ("xi_differs", XI, CART3, _src(CART3, A, ev=ev, elements=el), True, dict(present=[2], xi_present=0.0)),
        # Two rules broken at once: the message the entry points gave before the set-up path was shared.  The plain
        # entry point looks for a rotating neighbour before the radius, the rotating one for an evolving neighbour
        # last; the rotating one checks the axis before the radius, the plain one after it.
        ("both_mixed_and_radius_plain", MIXED, CART3, _src(CART3, E, ev=ev, elements=el, radius=0.0), False,
         dict(present=[2], xi_present=-0.43)),
        ("both_mixed_and_radius_rotating", RADIUS, CART3, _src(CART3, A, ev=ev, elements=el, radius=0.0), True,
         dict(present=[1])),
        ("both_axis_and_radius_plain", RADIUS, CYL2, _src(CYL2, C, pos=(0.0, 1.0e15, 0.0), radius=0.0), False, {}),
        ("both_axis_and_radius_rotating", AXIS, CYL2, _src(CYL2, A, ev=_eta_car(), pos=(0.0, 1.0e15, 0.0), radius=0.0),
         True, {}),
        ("both_mixed_and_xi", MIXED, CART3, _src(CART3, A, ev=ev, elements=el), True,
         dict(present=[1], xi_present=0.0)),
        ("both_rows_and_column", ROWS, CART3, _src(CART3, E, ev=_one_row(), elements=el), False, dict(drop=("R",))),
    ]
    c += [("no_%s%s" % (col, "_rotating" if rot else ""), COLUMN, CART3, _src(CART3, A if rot else E, ev=ev, elements=el),
           rot, dict(drop=(col,))) for col in ("time", "Teff", "Mdot", "vrot", "vinf", "R") for rot in (False, True)]
    return c


@pytest.mark.parametrize("case", _einval_cases(), ids=lambda c: c[0])
def test_einval_and_its_text(case):
    _, text, cfg, src, rotating, kw = case
    rc, msg, states, checks = _run(_case(cfg, src, rotating, [1.0e11], **kw))
    assert (rc, msg) == (-1, text)
    assert states == [] and checks == []


def test_neighbours_that_are_allowed():
    ev, el = _three_rows(), ["X_He", None]
    # a rotating source with the xi of the one present, constant sources beside either kind, no vcrit for type 1
    for src, rot, kw in ((_src(CART3, wind.ANGLE, ev=ev, elements=el), True, dict(present=[2, 0], xi_present=-0.43)),
                         (_src(CART3, wind.CONSTANT), False, dict(present=[2, 1], xi_present=-0.43)),
                         (_src(CART3, wind.EVOLVING, ev=ev, elements=el), False, dict(present=[1, 0], drop=("vcrit",)))):
        assert _run(_case(CART3, src, rot, **kw))[:2] == (0, "")
