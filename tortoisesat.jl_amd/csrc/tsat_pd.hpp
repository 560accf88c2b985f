// tsat_pd.hpp — the PROJECTION PD LAW on the dispersed plants (tsat_pd_ensemble, include/tortoise_hip.h): the feedback every
// magnetorquer CubeSat carries, flown on the plants, limits, noise, gravity field and statistic of tsat_tvlqr_ensemble_gg, as the
// baseline the tracked plans are compared against. The reference's form of it:
//   psiaki_controller, src/comparison/psiaki_dynamics.jl:1-26       T_req = -(C1 w~ + C2 inv(J) q~[2:4]), m = (B x T_req) / |B|^2
//   the loop around a reference trajectory, src/comparison/psiaki2005.jl:139-164
//   nominal_input_psiaki, src/comparison/psiaki_dynamics.jl:127-143  the direction-preserving limit
// Deviations from those scripts, which are experimental (the law below is the one include/tortoise_hip.h defines):
//   - the rate term there enters with the opposite sign of the attitude term (it drives the rate error up); here both oppose;
//   - q~ = q (x) q_guess there has no inverse on either factor; here e = conj(q_ref) (x) q, the product of the TVLQR feedback;
//   - the attitude term takes the shortest rotation, s = sign(e0); the scripts have no sign rule;
//   - inv(J) is folded into the gain: a caller who wants the reference's form passes kp = C2 / J_ii;
//   - m_limit is an unused argument of nominal_input_psiaki; here limit_mode = 1 applies that rule to the limits of the call.
//
// Per knot k, x the lane's state (the TRUE state, as the TVLQR feedback sees it), xr the reference record (X[:,k,t], or xf when
// the call regulates):
//   dw = x[0:3] - xr[0:3];  e = conj(xr[3:7]) (x) x[3:7];  s = (e0 < 0) ? -1 : 1
//   Treq[c] = -(kd[c] dw[c] + kp[c] (s e[1+c]))
//   b = qrot(x[3:7] / |x[3:7]|, b0)         b0: the stage-0 field row the step has loaded anyway, no noise
//   m = (b x Treq) / (b . b), 0 where b . b == 0        [A m^2]
//   u_cmd = (feedforward ? U_k : 0) + m / u_scale
// (what the law sees of x — the errors' state and the body-frame field — comes from the `Sensor` of the roll-out: TrueState of
// tsat_ensemble.hpp, which holds the qrot lines above, for tsat_pd_ensemble; Sensed of tsat_sensed.hpp for tsat_pd_ensemble_sensed)
// then the limit (0: the component clip of DispersedPlant::command; 1: u / beta when beta = max_c u_c / (u_c > 0 ? hi_c : lo_c)
// exceeds 1) and the parent's G u_sat + m_res / u_scale held over the four stages.
//
// Lane = realisation, and the loop restates ensemble_rollout of tsat_ensemble.hpp with the command lines replaced, so
// that ensemble_rollout and every kernel built on it keep their instruction streams. The
// plant types are the parents' own, DispersedPlant and GgPlant, used as they are: load, traj, command, actuate, disturb, store.
// No gain rows: per knot the wave reads the reference record (when tracking) and three field rows by scalar loads; the gains,
// the limits, their reciprocals and xf are loaded once per wave. X == null, feedforward and limit_mode are launch-uniform and
// taken by uniform branches: one kernel per plant type, so that a regulating call and a tracking call of the same record, or the
// two limit rules below their threshold, run the same instructions on the same values.
#pragma once
#include <string>
#include "tsat_host_pack.hpp"
#include "tsat_gg.hpp"

namespace tsat {

constexpr int PDGW = 6;          // gains of a slew: kd[3], kp[3]

template <typename real>
struct PdArgs {
  DispArgs<real> d;      // the dispersed ensemble's block; d.e.XUR null: regulation to xf; d.e.KD unused
  const real* GT;        // [n_btab][n_tab][4] packed gravity rows (GgPlant only)
  const real* GAIN;      // [T][PDGW]
  const real* X0N;       // [T][7] start of the noise-free model plant (slot M)
  int feedforward, limit_mode;
};

template <typename real, typename Plant, typename Sensor = TrueState>
TSAT_DEV void pd_rollout(const PdArgs<real>& pa, Plant& plant, int traj, int wave, Sensor sensor = Sensor()) {
  constexpr int DIAGJ = Plant::DIAGJ;
  const EnsArgs<real>& a = pa.d.e;
  const int lane = TSAT_LANE();
  const int NS = a.N, n_tab = a.n_tab, M = a.M;
  const int N = a.nk ? a.nk[traj] : a.N;                       // own horizon; slabs keep the stride NS
  const int R = M + 1;
  // lanes past the last realisation compute a duplicate of it and store nothing (no divergent exit)
  const int r_own = wave * WAVE + lane;
  const bool live = r_own < R;
  const int r = live ? r_own : R - 1;
  const bool noisy = r < M;
  const TSAT_CONSTMEM real* Pc = (const TSAT_CONSTMEM real*)(a.P + (size_t)traj * PSTRIDE);
  const TSAT_CONSTMEM real* xu = a.XUR ? (const TSAT_CONSTMEM real*)(a.XUR + (size_t)traj * NS * XUW) : nullptr;
  const TSAT_CONSTMEM real* gn = (const TSAT_CONSTMEM real*)(pa.GAIN + (size_t)traj * PDGW);
  const TSAT_CONSTMEM real* bt = (const TSAT_CONSTMEM real*)(a.BT + (size_t)a.bidx[traj] * n_tab * 4);
  const Traj<real> tr = ensemble_traj<real>(Pc, a.us, N, n_tab);
  plant.load(tr, traj, r);
  sensor.load(traj, r);
  const Traj<real>& tp = plant.traj(tr);                       // what dyn_sim_h reads
  const long long gid = (a.nid0 ? a.nid0[traj] : (long long)traj * (long long)M) + (long long)r;
  TSAT_GLOBAL real* xs = (a.XS && live && noisy) ? (TSAT_GLOBAL real*)(a.XS + ((size_t)traj * M + r) * NS * 7) : nullptr;
  real x[7];
  if (noisy) {
    const TSAT_GLOBAL real* x0 = (const TSAT_GLOBAL real*)(a.X0 + ((size_t)traj * M + r) * 7);
    for (int i = 0; i < 7; ++i) x[i] = x0[i];
  } else {
    const TSAT_CONSTMEM real* x0 = (const TSAT_CONSTMEM real*)(pa.X0N + (size_t)traj * 7);
    for (int i = 0; i < 7; ++i) x[i] = x0[i];
  }
  const real cs = control_scale<real, DIAGJ>(tr);
  // the law's constants, once per wave: gains, 1 / u_scale, and for limit_mode 1 the reciprocals of the limits
  real kd[3], kp[3], ilo[3] = {0, 0, 0}, ihi[3] = {0, 0, 0};
  for (int c = 0; c < 3; ++c) { kd[c] = gn[c]; kp[c] = gn[3 + c]; }
  const real ius = rcp_(a.us);
  const int ff = pa.feedforward, mode1 = pa.limit_mode;
  if (mode1)
    for (int c = 0; c < 3; ++c) { ilo[c] = rcp_(plant.lo[c]); ihi[c] = rcp_(plant.hi[c]); }
  int first = 0;                                               // the statistic, evaluated while the roll-out runs
  TSAT_NO_UNROLL
  for (int k = 0; k < N - 1; ++k) {
    {  // sample j = k + 1 (1-based): src/monte_carlo.jl:242-262
      const real wj = sqrt_(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
      if (first == 0 && k + 1 > a.min_steps && wj < a.w_tol) {
        if (ensemble_angle<real>(tr, x) < a.ang_tol) first = k + 1;
      }
    }
    if (xs)
      for (int i = 0; i < 7; ++i) xs[(size_t)k * 7 + i] = x[i];
    real xr[7], uc[3] = {0, 0, 0};
    if (xu) {
      const TSAT_CONSTMEM real* rec = xu + (size_t)k * XUW;
      for (int i = 0; i < 7; ++i) xr[i] = rec[i];
      if (ff)
        for (int c = 0; c < 3; ++c) uc[c] = rec[7 + c];
    } else {
      for (int i = 0; i < 7; ++i) xr[i] = tr.xf[i];
    }
    // rows at tau, tau + dtau/2, tau + dtau: wave-uniform indices, said so (the clock is fp64 arithmetic on the vector unit)
    const TSAT_CONSTMEM real* p0 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 0.0)) * 4;
    const TSAT_CONSTMEM real* p1 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 0.5)) * 4;
    const TSAT_CONSTMEM real* p2 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 1.0)) * 4;
    const real b0[3] = {p0[0], p0[1], p0[2]}, b1[3] = {p1[0], p1[1], p1[2]}, b2[3] = {p2[0], p2[1], p2[2]};
    {  // the law, on what the sensor gives of x: y for the errors, B for the body-frame field
      real tq[3], y[7], B[3];
      sensor.state(gid, k, noisy, x, y);
      {
        // e = q_ref^-1 (x) q_sim: the vector part as ensemble_rollout forms it, and the scalar part for the sign rule
        const real s1 = xr[3], a1 = -xr[4], a2 = -xr[5], a3 = -xr[6];
        const real e0 = s1 * y[3] - (a1 * y[4] + a2 * y[5] + a3 * y[6]);
        const real e1 = s1 * y[4] + y[3] * a1 + (a2 * y[6] - a3 * y[5]);
        const real e2 = s1 * y[5] + y[3] * a2 + (a3 * y[4] - a1 * y[6]);
        const real e3 = s1 * y[6] + y[3] * a3 + (a1 * y[5] - a2 * y[4]);
        const bool neg = e0 < 0;                               // shortest rotation
        tq[0] = -(kd[0] * (y[0] - xr[0]) + kp[0] * (neg ? -e1 : e1));
        tq[1] = -(kd[1] * (y[1] - xr[1]) + kp[1] * (neg ? -e2 : e2));
        tq[2] = -(kd[2] * (y[2] - xr[2]) + kp[2] * (neg ? -e3 : e3));
      }
      sensor.field(gid, k, noisy, x, b0, B);                   // TrueState: qrot(q, b0)
      const real B0 = B[0], B1 = B[1], B2 = B[2];
      const real bb = B0 * B0 + B1 * B1 + B2 * B2;
      // the one reciprocal of the knot; a zero row (the last of a magnetic_simulation table) gives no dipole
      const real sc = (bb == 0) ? (real)0 : rcp_(bb) * ius;
      uc[0] = uc[0] + (B1 * tq[2] - B2 * tq[1]) * sc;
      uc[1] = uc[1] + (B2 * tq[0] - B0 * tq[2]) * sc;
      uc[2] = uc[2] + (B0 * tq[1] - B1 * tq[0]) * sc;
    }
    real us[3];
    if (mode1) {
      // direction-preserving: the largest ratio of a component to the limit on its side
      real beta = 0;
      for (int c = 0; c < 3; ++c) {
        const real rc = uc[c] > 0 ? uc[c] * ihi[c] : (uc[c] < 0 ? uc[c] * ilo[c] : (real)0);
        beta = rc > beta ? rc : beta;
      }
      if (beta > 1) {
        const real ib = rcp_(beta);
        for (int c = 0; c < 3; ++c) uc[c] = uc[c] * ib;
        plant.hit = 1;
      }
    } else {
      for (int c = 0; c < 3; ++c) uc[c] = plant.command(c, uc[c], cs);
    }
    sensor.commanded(k, uc);                                   // as ensemble_rollout hands it over
    plant.actuate(uc, cs, us);
    real k1[7], k2[7], k3[7], k4[7], t[7], nz[9];
    for (int i = 0; i < 9; ++i) nz[i] = 0;
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 0, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, DIAGJ>(tp, x, us, b0, noisy, nz, k1);
    plant.disturb(tr, k, 0.0, x, k1);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k1[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 1, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, DIAGJ>(tp, t, us, b1, noisy, nz, k2);
    plant.disturb(tr, k, 0.5, t, k2);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + (real)0.5 * k2[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 2, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, DIAGJ>(tp, t, us, b1, noisy, nz, k3);
    plant.disturb(tr, k, 0.5, t, k3);
    for (int i = 0; i < 7; ++i) t[i] = x[i] + k3[i];
    if (noisy) plant_noise<real>(a.k0, a.k1, gid, k, 3, a.sg, a.sa, a.fa, nz);
    dyn_sim_h<real, DIAGJ>(tp, t, us, b2, noisy, nz, k4);
    plant.disturb(tr, k, 1.0, t, k4);
    for (int i = 0; i < 7; ++i) x[i] = x[i] + (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) * (real)(1.0 / 6.0);
  }
  // last sample j = N
  const real wN = sqrt_(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const real angN = ensemble_angle<real>(tr, x);
  if (first == 0 && N > a.min_steps && wN < a.w_tol && angN < a.ang_tol) first = N;
  if (xs)
    for (int i = 0; i < 7; ++i) xs[(size_t)(N - 1) * 7 + i] = x[i];
  if (live) {
    tsat_tvlqr_stats st;
    st.slew_index = first;
    st.failed = first ? 0 : 1;
    st.slew_time = (double)tr.h * (first ? (double)first : (double)N);
    st.final_w_norm = (double)wN;
    st.final_angle = (double)angN;
    if (noisy) {
      a.stats[(size_t)traj * M + r] = st;
      plant.store((size_t)traj * M + r);
    } else {
      a.stats_nom[traj] = st;
    }
  }
}

// Everything tsat_pd_ensemble rejects besides a null handle, before anything is allocated or launched: "" or the reason. The
// checks of tsat_tvlqr_ensemble_gg in their order (a null plant and a null Rtab with gm == 0 are allowed here), then the law's own.
inline std::string check_pd(const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M, const double* X, const double* U,
                            const double* xf, const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                            const double* dt, const double* Jmat, const double* kd, const double* kp, int32_t feedforward,
                            int32_t limit_mode, const double* x0_sim, const double* x0_nom, const int32_t* n_knots, const double* plant,
                            const double* sat_lo, const double* sat_hi, const void* stats, const double* summary,
                            const void* stats_nominal, const double* Rtab, double gm) {
  if (!o) return "null handle or options";
  const std::string why = check_tv_options(*o);
  if (!why.empty()) return why;
  if (o->noise_mode != 1) return "noise_mode must be 1: the ensemble draws its noise in the kernel";
  if (o->rate_as_written != 0) return "rate_as_written must be 0: the statistic is evaluated while the roll-out runs";
  if (M < 1 || M > 65535) return "M must be in [1, 65535]";
  if (T < 1 || T > 0x7fffffff || n_btab < 1) return "bad batch dimensions";
  if (!xf || !Btab || !tau0 || !dtau || !dt || !Jmat || !x0_sim || !stats || !summary) return "null array";
  if (!btab_idx && n_btab != T) return "btab_idx is NULL but n_btab != T";
  for (int64_t t = 0; t < T; ++t) {
    const int64_t v = btab_idx ? btab_idx[t] : t;
    if (v < 0 || v >= n_btab) return "btab_idx out of range";
    if (!(dt[t] > 0.0)) return "dt must be positive";
    if (n_knots && (n_knots[t] < 2 || n_knots[t] > o->n_knots)) return "n_knots[t] must be in [2, N]";
  }
  const std::string lim = check_limits(sat_lo, sat_hi, T);
  if (!lim.empty()) return lim;
  if (plant)
    for (int64_t t = 0; t < T; ++t)
      for (int m = 0; m < M; ++m) {
        const std::string bad = check_plant_record(plant + ((size_t)t * M + m) * TSAT_PLANT_W);
        if (!bad.empty()) return bad + " at (t, m) = (" + std::to_string(t) + ", " + std::to_string(m) + ")";
      }
  if (Rtab) {
    const std::string bad = check_gravity(Rtab, gm, n_btab * (int64_t)o->n_tab);
    if (!bad.empty()) return bad;
  } else if (!(gm == 0.0)) {
    return "Rtab is NULL but gm != 0: the gravity-gradient term needs the orbit table";
  }
  if (!kd || !kp) return "null kd or kp";
  for (int64_t i = 0; i < 3 * T; ++i)
    if (!std::isfinite(kd[i]) || !std::isfinite(kp[i]) || kd[i] < 0.0 || kp[i] < 0.0)
      return "kd and kp must be finite and >= 0 (t = " + std::to_string(i / 3) + ")";
  if (feedforward != 0 && feedforward != 1) return "feedforward must be 0 (the law alone) or 1 (U + the law)";
  if (feedforward == 1 && (!X || !U)) return "feedforward = 1 needs the plan: X and U";
  if (limit_mode != 0 && limit_mode != 1) return "limit_mode must be 0 (component clip) or 1 (direction-preserving)";
  if (limit_mode == 1) {
    if (!sat_lo) return "limit_mode = 1 needs sat_lo and sat_hi";
    for (int64_t i = 0; i < 3 * T; ++i)
      if (!(sat_lo[i] < 0.0 && 0.0 < sat_hi[i])) return "limit_mode = 1 needs sat_lo < 0 < sat_hi in every component (t = " + std::to_string(i / 3) + ")";
  }
  if (!X && stats_nominal && !x0_nom) return "X is NULL (regulation): stats_nominal needs x0_nom, the start of the noise-free plant";
  return "";
}

// Rtab == null at the call: the plants of tsat_tvlqr_ensemble_dispersed ...
template <typename real>
TSAT_DEV void pd_wave(const PdArgs<real>& pa, int traj, int wave) {
  DispersedPlant<real> plant(pa.d);
  pd_rollout<real>(pa, plant, traj, wave);
}

// ... otherwise those of tsat_tvlqr_ensemble_gg, whatever gm is
template <typename real>
TSAT_DEV void pd_gg_wave(const PdArgs<real>& pa, int traj, int wave) {
  const GgEnsArgs<real> g{pa.d, pa.GT};
  GgPlant<real> plant(g);
  pd_rollout<real>(pa, plant, traj, wave);
}

}  // namespace tsat
