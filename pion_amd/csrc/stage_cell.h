// stage_cell.h -- the body of the cell-per-thread stage kernel, included by kernels_fp.hip into k_stage and, with
// PION_STAGE_DE defined, into k_stage_dE: there the microphysics source arrives as dE per cell from k_cooling_dE
// (EP.cooling = 2, 4..7) instead of being integrated in place.  A textual include and not a function template, so
// that k_stage compiles from exactly the text it had: its code is pinned (profiles/tools/isa_diff.py).
// In scope: the template parameters EQ, NTR, SOLVER and the kernel argument `const StageArgs a`.
  typedef Eqn<EQ, NTR> E;
  typedef Flux<EQ, NTR, SOLVER> FX;
  constexpr int NV = E::NV;
  constexpr int BASE = E::BASE;
  constexpr bool MHD = E::MHD;

  // ---- which cell -------------------------------------------------------
  const int nbx = (a.g.ng[0] + 63) / 64, nby = (a.g.ng[1] + 3) / 4;
  const long ntiles = (long)nbx * nby * a.g.ng[2];
  const long tile = xcd_tile(blockIdx.x, ntiles);
  if (tile >= ntiles) return;
  const int bx = (int)(tile % nbx), by = (int)((tile / nbx) % nby), bz = (int)(tile / ((long)nbx * nby));
  const int ix = bx * 64 + (threadIdx.x & 63), iy = by * 4 + (threadIdx.x >> 6), iz = bz;
  if (ix >= a.g.ng[0] || iy >= a.g.ng[1]) return;
  const long nc = a.g.ncell;
  const long c = (long)(ix + a.g.nbc[0]) + a.g.sy * (iy + a.g.nbc[1]) + a.g.sz * (iz + a.g.nbc[2]);
  const double g = a.fc.gamma, dx = a.g.dx, dt = a.dt;
  int err = 0;

  // start-of-step state of this cell (lab frame)
  double P0[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) P0[v] = a.Pc[v * nc + c];

  const uint8_t fl = a.flags[c];
  if (!(fl & 4 /*ISDOMAIN*/) || !(fl & 16 /*ISLEAF*/)) {
    // grid_update_state_vector skips the cell (time_integrator.cpp:905-908): Ph keeps its value
#pragma unroll
    for (int v = 0; v < NV; v++) a.out[v * nc + c] = P0[v];
    return;
  }

  double dU[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) dU[v] = 0.0;

  // ---- microphysics source (calc_noRT_microphysics_dU) --------------------
#ifdef PION_STAGE_DE
  // only the energy differs between PtoU(p_new) and PtoU(P): the other components of the difference are exact zeros
  dU[uERG] += a.dE[c];
#else
  if (a.cooling != 0) {
    const double pg_new = Cooling::time_update(a.cool, P0[qRO], P0[qPG], dt, g, err);
    double pn[NV], ui[NV], uf[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) pn[v] = P0[v];
    pn[qPG] = pg_new;
    E::PtoU(P0, ui, g);
    E::PtoU(pn, uf, g);
#pragma unroll
    for (int v = 0; v < NV; v++) dU[v] += uf[v] - ui[v];
  }
#endif

  // ---- sweeps -------------------------------------------------------------
  const bool oa2 = (a.space_ooa == 2);
#pragma unroll 1
  for (int ax = 0; ax < a.g.ndim; ax++) {
    const long st = (ax == 0) ? 1 : ((ax == 1) ? a.g.sy : a.g.sz);
    // R sweep of a cylindrical (z,R) grid: geometry enters slopes, edge states, the flux divergence and
    // the source terms (VectorOps_Cyl, cyl_FV_solver_*); jy = all-cell y index of this cell
    const bool cylR = (a.g.cyl == 1 && ax == 1);
    const bool sphR = (a.g.cyl == 2 && ax == 0);   // spherical symmetry: the only axis is R
    const int jy = sphR ? ix + a.g.nbc[0] : iy + a.g.nbc[1];
    double Rm1 = 0.0, R0 = 0.0, Rp1 = 0.0;
    if (cylR) {
      Rm1 = cyl_R(a.g, jy - 1);
      R0 = cyl_R(a.g, jy);
      Rp1 = cyl_R(a.g, jy + 1);
    }
    else if (sphR) {
      Rm1 = sph_R(a.g, jy - 1);
      R0 = sph_R(a.g, jy);
      Rp1 = sph_R(a.g, jy + 1);
    }
    double qm1[NV], q0[NV], qp1[NV], sm1[NV], s0[NV], sp1[NV];
    {
      double qm2[NV], qp2[NV];
#pragma unroll
      for (int s = 0; s < NV; s++) {
        const double *b = a.S + (long)rotvar<MHD>(ax, s) * nc + c;
        qm1[s] = b[-st];
        q0[s] = b[0];
        qp1[s] = b[st];
        if (oa2) {
          qm2[s] = b[-2 * st];
          qp2[s] = b[2 * st];
        }
        else {
          qm2[s] = qp2[s] = 0.0;
        }
      }
      // SetSlope (VectorOps.cpp:578-617; along R of a cylindrical grid VectorOps_Cyl::SetSlope
      // :1103-1204: differences of the cells' centres of mass)
      if (cylR || sphR) {
        // (VectorOps_Sph::SetSlope, VectorOps_spherical.cpp:358-440, has the same form with its own R_com)
        const double c_m2 = sphR ? sph_Rcom(sph_R(a.g, jy - 2), dx) : cyl_Rcom(cyl_R(a.g, jy - 2), dx),
                     c_m1 = sphR ? sph_Rcom(Rm1, dx) : cyl_Rcom(Rm1, dx),
                     c_0 = sphR ? sph_Rcom(R0, dx) : cyl_Rcom(R0, dx),
                     c_p1 = sphR ? sph_Rcom(Rp1, dx) : cyl_Rcom(Rp1, dx),
                     c_p2 = sphR ? sph_Rcom(sph_R(a.g, jy + 2), dx) : cyl_Rcom(cyl_R(a.g, jy + 2), dx);
#pragma unroll
        for (int s = 0; s < NV; s++) {
          if (oa2) {
            sm1[s] = avg_falle((qm1[s] - qm2[s]) / (c_m1 - c_m2), (q0[s] - qm1[s]) / (c_0 - c_m1));
            s0[s] = avg_falle((q0[s] - qm1[s]) / (c_0 - c_m1), (qp1[s] - q0[s]) / (c_p1 - c_0));
            sp1[s] = avg_falle((qp1[s] - q0[s]) / (c_p1 - c_0), (qp2[s] - qp1[s]) / (c_p2 - c_p1));
          }
          else {
            sm1[s] = s0[s] = sp1[s] = 0.0;
          }
        }
      }
      else {
#pragma unroll
        for (int s = 0; s < NV; s++) {
          if (oa2) {
            sm1[s] = avg_falle((qm1[s] - qm2[s]) / dx, (q0[s] - qm1[s]) / dx);
            s0[s] = avg_falle((q0[s] - qm1[s]) / dx, (qp1[s] - q0[s]) / dx);
            sp1[s] = avg_falle((qp1[s] - q0[s]) / dx, (qp2[s] - qp1[s]) / dx);
          }
          else {
            sm1[s] = s0[s] = sp1[s] = 0.0;
          }
        }
      }
    }
    // two interfaces: face 0 = (c-st | c), face 1 = (c | c+st)
    double Fm[NV], Fp[NV];
#pragma unroll 1
    for (int face = 0; face < 2; face++) {
      double eL[NV], eR[NV], f[NV], pstar[NV];
      // SetEdgeState (VectorOps.cpp:535-571)
#pragma unroll
      for (int s = 0; s < NV; s++) {
        const double ql = face ? q0[s] : qm1[s], sl = face ? s0[s] : sm1[s];
        const double qr = face ? qp1[s] : q0[s], sr = face ? sp1[s] : s0[s];
        if (oa2 && cylR) {
          // VectorOps_Cyl::SetEdgeState (VectorOps.cpp:1052-1092): distance of the face from the centre of mass
          const double Rl = face ? R0 : Rm1, Rr = face ? Rp1 : R0;
          eL[s] = ql + sl * (Rl + dx * 0.5 - cyl_Rcom(Rl, dx));
          eR[s] = qr + sr * (Rr - dx * 0.5 - cyl_Rcom(Rr, dx));
        }
        else if (oa2 && sphR) {
          // VectorOps_Sph::SetEdgeState (VectorOps_spherical.cpp:294-350)
          const double Rl = face ? R0 : Rm1, Rr = face ? Rp1 : R0;
          eL[s] = ql + sl * (Rl + 0.5 * dx - sph_Rcom(Rl, dx));
          eR[s] = qr + sr * (Rr - 0.5 * dx - sph_Rcom(Rr, dx));
        }
        else if (oa2) {
          eL[s] = ql + sl * dx * 0.5;
          eR[s] = qr - sr * dx * 0.5;
        }
        else {
          eL[s] = ql;
          eR[s] = qr;
        }
      }
      const long cl = face ? c : c - st;
      double hc_eta = 0.0;
      if (a.fc.artvisc == AV_HCORRECTION || a.fc.artvisc == AV_HCORR_FKJ98) hc_eta = select_hcorr_eta(a, ax, cl, st);
      bool use_hll = false;
      if constexpr (MHD && SOLVER == FLUX_RS_HLLD) use_hll = (a.hllflag[cl] | a.hllflag[cl + st]) != 0;
      FX::intercell_flux(eL, eR, f, pstar, a.fc, hc_eta, use_hll, err);
#pragma unroll
      for (int s = 0; s < NV; s++) {
        if (face == 0) Fm[s] = f[s];
        else Fp[s] = f[s];
      }
    }
    // accumulate in the sweep frame, in the reference's order
    double d[NV];
    to_sweep<NV, MHD>(ax, dU, d);
#ifdef PION_FAST_MATH
    // fast build, Cartesian axis: the same regrouped source + flux-difference update as k_stage_rows2
    // (apply_axis), so that the two kernels agree to rounding
    const bool fast_cart = !cylR && !sphR;
#else
    const bool fast_cart = false;
#endif
    if (fast_cart) {
      double bnm_ = 0.0, bnp_ = 0.0, sim_ = 0.0, sip_ = 0.0;
      if constexpr (MHD) {
        bnm_ = qm1[qBN];
        bnp_ = qp1[qBN];
      }
      if constexpr (EQ == EQGLM) {
        sim_ = qm1[qSI];
        sip_ = qp1[qSI];
      }
      apply_axis<EQ, NV>(d, q0, bnm_, sim_, bnp_, sip_, Fm, Fp, dt, dx);
    }
    else {
    if constexpr (MHD) {
      // MHDsource (solver_eqn_mhd_adi.cpp:396-443, GLM :782-813): this cell is the right cell
      // of face 0 and the left cell of face 1
      const double uB = q0[qBN] * q0[qVN] + q0[qBT1] * q0[qVT1] + q0[qBT2] * q0[qVT2];
      const double bm0 = 0.5 * (qm1[qBN] + q0[qBN]);
      if (cylR) {
        // cyl_FV_solver_mhd_ideal_adi::MHDsource, Rcyl (solver_eqn_mhd_adi.cpp:1081-1092): this cell as
        // the right cell of its lower face ...
        double rp = Rm1 + dx * 0.5;
        const double rn = rp;
        rp += dx;
        d[uMN] += dt * bm0 * (q0[qBN]) * 2.0 * rn / (rp * rp - rn * rn);
        d[uMT1] += dt * bm0 * (q0[qBT1]) * 2.0 * rn / (rp * rp - rn * rn);
        d[uMT2] += dt * bm0 * (q0[qBT2]) * 2.0 * rn / (rp * rp - rn * rn);
        d[uERG] += dt * bm0 * (uB) * 2.0 * rn / (rp * rp - rn * rn);
        d[uBN] += dt * bm0 * (q0[qVN]) * 2.0 * rn / (rp * rp - rn * rn);
        d[uBT1] += dt * bm0 * (q0[qVT1]) * 2.0 * rn / (rp * rp - rn * rn);
        d[uBT2] += dt * bm0 * (q0[qVT2]) * 2.0 * rn / (rp * rp - rn * rn);
      }
      else {
        d[uMN] += dt * bm0 * (q0[qBN]) / dx;
        d[uMT1] += dt * bm0 * (q0[qBT1]) / dx;
        d[uMT2] += dt * bm0 * (q0[qBT2]) / dx;
        d[uERG] += dt * bm0 * (uB) / dx;
        d[uBN] += dt * bm0 * (q0[qVN]) / dx;
        d[uBT1] += dt * bm0 * (q0[qVT1]) / dx;
        d[uBT2] += dt * bm0 * (q0[qVT2]) / dx;
      }
      if constexpr (EQ == EQGLM) {
        const double sm0 = 0.5 * (qm1[qSI] + q0[qSI]);
        d[uERG] += dt * sm0 * (q0[qVN] * q0[qSI]) / dx;
        d[uPSI] += dt * sm0 * q0[qVN] / dx;
      }
      const double bm1 = 0.5 * (q0[qBN] + qp1[qBN]);
      if (cylR) {
        // ... and as the left cell of its upper face
        const double rp = R0 + dx * 0.5;
        const double rn = rp - dx;
        d[uMN] -= dt * bm1 * (q0[qBN]) * 2.0 * rp / (rp * rp - rn * rn);
        d[uMT1] -= dt * bm1 * (q0[qBT1]) * 2.0 * rp / (rp * rp - rn * rn);
        d[uMT2] -= dt * bm1 * (q0[qBT2]) * 2.0 * rp / (rp * rp - rn * rn);
        d[uERG] -= dt * bm1 * (uB) * 2.0 * rp / (rp * rp - rn * rn);
        d[uBN] -= dt * bm1 * (q0[qVN]) * 2.0 * rp / (rp * rp - rn * rn);
        d[uBT1] -= dt * bm1 * (q0[qVT1]) * 2.0 * rp / (rp * rp - rn * rn);
        d[uBT2] -= dt * bm1 * (q0[qVT2]) * 2.0 * rp / (rp * rp - rn * rn);
      }
      else {
        d[uMN] -= dt * bm1 * (q0[qBN]) / dx;
        d[uMT1] -= dt * bm1 * (q0[qBT1]) / dx;
        d[uMT2] -= dt * bm1 * (q0[qBT2]) / dx;
        d[uERG] -= dt * bm1 * (uB) / dx;
        d[uBN] -= dt * bm1 * (q0[qVN]) / dx;
        d[uBT1] -= dt * bm1 * (q0[qVT1]) / dx;
        d[uBT2] -= dt * bm1 * (q0[qVT2]) / dx;
      }
      if constexpr (EQ == EQGLM) {
        const double sm1g = 0.5 * (q0[qSI] + qp1[qSI]);
        d[uERG] -= dt * sm1g * (q0[qVN] * q0[qSI]) / dx;
        d[uPSI] -= dt * sm1g * q0[qVN] / dx;
      }
    }
    // dU_Cell + DivStateVectorComponent (VectorOps.cpp:624-644)
    if (sphR) {
      // VectorOps_Sph::DivStateVectorComponent (VectorOps_spherical.cpp:449-475; the cell's shell volume
      // (rp^3-rn^3)/3 comes from the host, where pow() is the reference's) and
      // sph_FV_solver_Hydro_Euler::geometric_source (solver_eqn_hydro_adi.cpp:648-675)
      double u1[NV];
      const double rp = R0 + 0.5 * dx;
      const double rn = rp - dx;
      const double rc = a.g.sph_vol[jy];
#pragma unroll
      for (int s = 0; s < NV; s++) u1[s] = (rn * rn * Fm[s] - rp * rp * Fp[s]) / rc;
      if (oa2) u1[uMN] += 2.0 * ((q0[qPG] - s0[qPG] * sph_Rcom(R0, dx)) / sph_R3(R0, dx) + s0[qPG]);
      else u1[uMN] += 2.0 * q0[qPG] / sph_R3(R0, dx);
#pragma unroll
      for (int s = 0; s < NV; s++) d[s] += dt * u1[s];
    }
    else if (cylR) {
      // VectorOps_Cyl::DivStateVectorComponent, Rcyl (VectorOps.cpp:1211-1245) + geometric_source of the
      // cyl_FV_solver_* classes (solver_eqn_hydro_adi.cpp:560-590, solver_eqn_mhd_adi.cpp:1001-1030, 1175-1210)
      double u1[NV];
      const double rp = R0 + dx * 0.5;
      const double rn = rp - dx;
#pragma unroll
      for (int s = 0; s < NV; s++) u1[s] = 2.0 * (rn * Fm[s] - rp * Fp[s]) / (rp * rp - rn * rn);
      const double Rc = cyl_Rcom(R0, dx);
      if constexpr (!MHD) {
        if (oa2) u1[uMN] += (q0[qPG] + (R0 - Rc) * s0[qPG]) / R0;
        else u1[uMN] += q0[qPG] / R0;
      }
      else {
        const double pm = (q0[qBN] * q0[qBN] + q0[qBT1] * q0[qBT1] + q0[qBT2] * q0[qBT2]) / 2.;
        if (oa2) {
          u1[uMN] += (q0[qPG] + pm +
                      (R0 - Rc) * (s0[qPG] + q0[qBN] * s0[qBN] + q0[qBT1] * s0[qBT1] + q0[qBT2] * s0[qBT2])) /
                     R0;
          if constexpr (EQ == EQGLM) u1[uBN] += a.fc.chyp * (q0[qSI] + (R0 - Rc) * s0[qSI]) / R0;
        }
        else {
          u1[uMN] += (q0[qPG] + pm) / R0;
          if constexpr (EQ == EQGLM) u1[uBN] += a.fc.chyp * q0[qSI] / R0;
        }
      }
#pragma unroll
      for (int s = 0; s < NV; s++) d[s] += dt * u1[s];
    }
    else {
#pragma unroll
      for (int s = 0; s < NV; s++) {
        const double u1 = (Fm[s] - Fp[s]) / dx;
        d[s] += dt * u1;
      }
    }
    }
    from_sweep<NV, MHD>(ax, d, dU);
  }

  // ---- CellAdvanceTime (solver_eqn_hydro_adi.cpp:372-448, solver_eqn_mhd_adi.cpp:452-504, :822-844)
  double u1[NV], Pf[NV];
  if (a.fc.mp.present) {
    double Pi[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) Pi[v] = P0[v];
    E::apply_sCMA(Pi);
    E::PtoU(Pi, u1, g);
  }
  else E::PtoU(P0, u1, g);
#pragma unroll
  for (int v = 0; v < NV; v++) u1[v] += dU[v];
  E::UtoP(u1, Pf, a.fc.min_temp, g, a.fc.mp, err);
  if (a.fc.mp.present) E::apply_sCMA(Pf);
  if constexpr (EQ == EQGLM) Pf[qSI] *= a.glm_damp;  // GLMsource (eqns_mhd_adiabatic.cpp:651-660)
  if (a.fc.mp.present) {
    // grid_update_state_vector: T > MaxTemperature clamp (time_integrator.cpp:926-932)
    const double T = Pf[qPG] * a.fc.mp.Mu_tot_over_kB / Pf[qRO];
    if (T > a.max_temp) Pf[qPG] = Pf[qRO] * a.max_temp / a.fc.mp.Mu_tot_over_kB;
  }
#pragma unroll
  for (int v = 0; v < NV; v++) a.out[v * nc + c] = Pf[v];
  if (err) atomicOr(a.errword, err);
