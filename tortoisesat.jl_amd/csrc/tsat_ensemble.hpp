// tsat_ensemble.hpp — closed-loop tracking of a solved slew under an ENSEMBLE of plant-noise realisations
// (tsat_tvlqr_ensemble, include/tortoise_hip.h): one Monte-Carlo trial of src/monte_carlo.jl:199-262 per lane.
//
// The tracking kernel of tsat_device.hpp (tvlqr_trajectory) rolls ONE realisation out with all 64 lanes computing the same
// state. Here lane = realisation: wavefront (t, w) simulates realisations 64 w .. 64 w + 63 of slew t — one instruction
// stream, 64 different plants. Everything a knot needs besides the lane's own state and noise is addressed by (t, k) only:
// reference record (10), gain rows (18), three field rows (9). Those are read through constant-address-space pointers built
// from the block index and the loop counter, i.e. by scalar LOADS into SGPRs (no LDS, no vector memory traffic in the loop;
// the kernel's only vector stores are the debugging X_sim path and the statistic at the end).
// The per-lane noise is drawn where it is consumed, one RK4 stage at a time (3 Philox blocks + 3 Box-Muller pairs), so that
// only nine noise values are live instead of 36.
//
// The roll-out (ensemble_rollout) is ONE function template over a small plant type: ModelPlant here, DispersedPlant in
// tsat_dispersed.hpp (tsat_tvlqr_ensemble_dispersed). The statistic, the attitude error, the gain product, the table clock, the
// noise draws and the RK4 stages exist once; ensemble_wave and dispersed_wave construct their plant and call it.
//
// Written over the lane abstraction of tsat_device.hpp (TSAT_DEV, TSAT_LANE, TSAT_CONSTMEM, ...) so that the CPU lane
// emulator runs the same source (tests/emu/tsat_emu_ensemble.cpp). The plant, the generator and the table clock are the
// device functions the tracking kernel uses: dyn_sim_h, plant_noise, brow_index, control_scale.
#pragma once
#include "tsat_device.hpp"

namespace tsat {

template <typename real>
struct EnsArgs {
  int T, N, n_tab, M, min_steps;   // realisation index M of every slew is the noise-free plant started at the plan's first state
  real us, w_tol, ang_tol;
  const real* P;      // [T][PSTRIDE]   parameter records (pack_tv_params)
  const real* BT;     // [n_btab][n_tab][4]
  const int* bidx;    // [T]
  const int* nk;      // [T] per-slew knot counts or null (all N)
  const real* XUR;    // [T][N][10]     optimised (X,U) records
  const real* KD;     // [T][N-1][24]   gains, solver sign (-K_lqr), rows of 7
  const real* X0;     // [T][M][7]      perturbed initial states
  unsigned k0, k1;    // generator key
  const long long* nid0;   // [T] first generator id of each slew or null (t * M)
  real sg, sa, fa;    // sigma_gyro, sigma_att, field_amp
  real* XS;           // [T][M][N][7] every simulated state, or null
  tsat_tvlqr_stats* stats;      // [T][M]
  tsat_tvlqr_stats* stats_nom;  // [T]
};

// waves per slew: M realisations + the nominal one over 64 lanes
inline int ensemble_waves(int M) { return (M + 1 + WAVE - 1) / WAVE; }

// the constants of a slew straight from its parameter record (wave-uniform: scalar loads), with the derived values formed as
// stage_traj / load_traj form them (h inv(J), h / 2, the control scales)
template <typename real>
TSAT_DEV Traj<real> ensemble_traj(const TSAT_CONSTMEM real* p, real u_scale, int N, int n_tab) {
  Traj<real> tr;
  const real h = p[P_DT];
  for (int i = 0; i < 7; ++i) { tr.xf[i] = p[P_XF + i]; tr.Qd[i] = 0; tr.Qfd[i] = 0; }
  for (int i = 0; i < 3; ++i) { tr.Rd[i] = 0; tr.ulo[i] = 0; tr.uhi[i] = 0; }
  for (int i = 0; i < 9; ++i) { tr.J[i] = p[P_J + i]; tr.hJi[i] = h * p[P_JI + i]; }
  tr.h = h; tr.hh = (real)0.5 * h; tr.us = u_scale; tr.usj = tr.us * tr.hJi[0];
  tr.tau0 = (double)p[P_TAU0] + (double)p[P_TAU0L]; tr.dtau = (double)p[P_DTAU] + (double)p[P_DTAUL];
  tr.N = N; tr.n_tab = n_tab; tr.bt = nullptr;
  return tr;
}

// the error angle of a sample, as the statistic of tvlqr_trajectory evaluates it
template <typename real>
TSAT_DEV real ensemble_angle(const Traj<real>& tr, const real x[7]) {
  const real qf0 = tr.xf[3], qf1 = -tr.xf[4], qf2 = -tr.xf[5], qf3 = -tr.xf[6];
  const real e0 = qf0 * x[3] - (qf1 * x[4] + qf2 * x[5] + qf3 * x[6]);
  return 2 * acos_(e0 < 1 ? e0 : (real)1);
}

// The MODEL plant: every realisation flies the satellite the plan was made for. A plant type answers what differs between the
// entry points and nothing else (the other one is DispersedPlant, tsat_dispersed.hpp): the instantiation of dyn_sim_h /
// control_scale it flies, what it loads once per lane, the Traj the dynamics read, what becomes of the feedback command on its
// way to the torquers, what besides m x B acts on the body in an RK4 stage (`disturb`: knot, stage fraction c of the table
// clock, the stage state as integrated, the stage's increment — GgPlant of tsat_gg.hpp adds the gravity-gradient term there),
// and what it stores per realisation besides the statistic.
template <typename real, int DIAGJ_>
struct ModelPlant {
  static constexpr int DIAGJ = DIAGJ_;
  TSAT_DEV void load(const Traj<real>&, int, int) {}
  TSAT_DEV const Traj<real>& traj(const Traj<real>& tr) const { return tr; }
  TSAT_DEV real command(int, real v, real cs) { return v * cs; }          // component c of U - K dX, in the plant's units
  TSAT_DEV void actuate(const real uc[3], real, real us[3]) {
    for (int c = 0; c < 3; ++c) us[c] = uc[c];
  }
  TSAT_DEV void disturb(const Traj<real>&, int, double, const real*, real*) const {}   // no torque besides m x B
  TSAT_DEV void store(size_t) const {}
};

// What the LAW sees of the lane's state, as a plant type answers what the plant is. TrueState: the state itself (`state`) and
// the stage-0 field row in the body frame of the true attitude (`field`, used by the PD law of tsat_pd.hpp) — every entry point
// but the sensed ones (Sensed of tsat_sensed.hpp: biases, noise and a one-knot delay). `load` is called once per lane after the
// plant's; gid, k and noisy name the realisation's generator id, the knot and whether the lane draws noise at all. `commanded`
// is told the command of knot k where it goes to plant.actuate (ModelFiltered of tsat_model_filtered.hpp predicts with it).
struct TrueState {
  TSAT_DEV void load(int, int) {}
  template <typename real>
  TSAT_DEV void commanded(int, const real*) {}                 // the command of knot k on its way to plant.actuate: not used
  template <typename real>
  TSAT_DEV void flown(const real*, const real*, const real*, const real*) {}   // mpc_held_block's hook (tsat_mpc_held.hpp): not used
  template <typename real>
  TSAT_DEV void state(long long, int, bool, const real x[7], real y[7]) {
    for (int i = 0; i < 7; ++i) y[i] = x[i];
  }
  // B = qrot(x[3:7] / |x[3:7]|, b0) = b0 + 2 v x (v x b0 + s b0), as dyn_h rotates it
  template <typename real>
  TSAT_DEV void field(long long, int, bool, const real x[7], const real b0[3], real B[3]) {
    const real rn = rsqrt_<real>(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
    const real q0 = x[3] * rn, q1 = x[4] * rn, q2 = x[5] * rn, q3 = x[6] * rn;
    const real c0 = (q2 * b0[2] - q3 * b0[1]) + q0 * b0[0];
    const real c1 = (q3 * b0[0] - q1 * b0[2]) + q0 * b0[1];
    const real c2 = (q1 * b0[1] - q2 * b0[0]) + q0 * b0[2];
    B[0] = b0[0] + 2 * (q2 * c2 - q3 * c1);
    B[1] = b0[1] + 2 * (q3 * c0 - q1 * c2);
    B[2] = b0[2] + 2 * (q1 * c1 - q2 * c0);
  }
};

// One closed loop per lane: realisation 64 wave + lane of slew traj on the plant `plant`, the feedback reading `sensor` (the
// choices are template arguments: nothing in the loop asks which entry point it serves).
template <typename real, typename Plant, typename Sensor = TrueState>
TSAT_DEV void ensemble_rollout(const EnsArgs<real>& a, Plant& plant, int traj, int wave, Sensor sensor = Sensor()) {
  constexpr int DIAGJ = Plant::DIAGJ;
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
  const TSAT_CONSTMEM real* xu = (const TSAT_CONSTMEM real*)(a.XUR + (size_t)traj * NS * XUW);
  const TSAT_CONSTMEM real* kdg = (const TSAT_CONSTMEM real*)(a.KD + (size_t)traj * (NS - 1) * KDW);
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
    for (int i = 0; i < 7; ++i) x[i] = xu[i];
  }
  const real cs = control_scale<real, DIAGJ>(tr);
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
    const TSAT_CONSTMEM real* xr = xu + (size_t)k * XUW;
    const TSAT_CONSTMEM real* kd = kdg + (size_t)k * KDW;
    real y[7], dX[6];                                          // y: what the feedback sees of x
    sensor.state(gid, k, noisy, x, y);
    for (int i = 0; i < 3; ++i) dX[i] = y[i] - xr[i];
    {  // vector part of q_ref^-1 (x) q_sim  (src/attitude_controller.jl:42)
      const real s1 = xr[3], a1 = -xr[4], a2 = -xr[5], a3 = -xr[6];
      dX[3] = s1 * y[4] + y[3] * a1 + (a2 * y[6] - a3 * y[5]);
      dX[4] = s1 * y[5] + y[3] * a2 + (a3 * y[4] - a1 * y[6]);
      dX[5] = s1 * y[6] + y[3] * a3 + (a1 * y[5] - a2 * y[4]);
    }
    real uc[3], us[3];
    for (int c = 0; c < 3; ++c) {
      real v = xr[7 + c];
      for (int j = 0; j < 6; ++j) v += kd[c * 7 + j] * dX[j];   // kd = -K_lqr
      uc[c] = plant.command(c, v, cs);
    }
    sensor.commanded(k, uc);                                   // the command as the law issued it, for a sensor that models the plant
    plant.actuate(uc, cs, us);
    // rows at tau, tau + dtau/2, tau + dtau: wave-uniform indices, said so (the clock is fp64 arithmetic on the vector unit)
    const TSAT_CONSTMEM real* p0 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 0.0)) * 4;
    const TSAT_CONSTMEM real* p1 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 0.5)) * 4;
    const TSAT_CONSTMEM real* p2 = bt + (size_t)TSAT_UNIFORM_INT(brow_index(tr, k, 1.0)) * 4;
    const real b0[3] = {p0[0], p0[1], p0[2]}, b1[3] = {p1[0], p1[1], p1[2]}, b2[3] = {p2[0], p2[1], p2[2]};
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

template <typename real, int DIAGJ>
TSAT_DEV void ensemble_wave(const EnsArgs<real>& a, int traj, int wave) {
  ModelPlant<real, DIAGJ> plant;
  ensemble_rollout<real>(a, plant, traj, wave);
}

// gains of one slew, exactly as tvlqr_trajectory computes them before its roll-out: terminal S = Qf_lqr, then chunks of
// Jacobian lanes (tv_jacobian_chunk) + the element-oriented Riccati recursion (riccati_chunk<real, 6, TvRec>), written to KD
// in the solver's sign. One wavefront per slew; uses the wave's LDS block of tsat_device.hpp (wide layout).
#if !defined(TSAT_DENSE)
template <typename real, int DIAGJ>
TSAT_DEV void ensemble_gains(const real* Pg, const real* BTg, const int* bidx, const int* nkg, const real* XUR, real* KDg,
                             int NS, int n_tab, real u_scale, int lin_sq, int traj) {
  real* lds = lds_base<real>();
  const int lane = TSAT_LANE();
  const int N = nkg ? nkg[traj] : NS;
  TPtrs<real> p;
  p.XU = (TSAT_GLOBAL real*)(XUR + (size_t)traj * NS * XUW);
  p.KD = (TSAT_GLOBAL real*)(KDg + (size_t)traj * (NS - 1) * KDW);
  p.LAM = nullptr; p.CAND = nullptr; p.XU0 = p.XU; p.cur = 0;
  p.bt = (const TSAT_GLOBAL real*)(BTg + (size_t)bidx[traj] * n_tab * 4);
  stage_traj<real>((const TSAT_GLOBAL real*)(Pg + (size_t)traj * PSTRIDE), u_scale);
  TSAT_SYNC();
  const real h = lds[L_TR + P_DT];
  const real hl = lin_sq ? h * h : h;
  const real frac = hl / h;
  {
    const int r1 = lane & 7, c1 = lane >> 3;
    if (c1 < 6 && r1 <= 6) lds[L_ST + r1 * 9 + c1] = (r1 == c1) ? lds[L_TR + P_QFD + c1] : (real)0;
    if (lane == 0) { lds[L_ZERO] = 0; lds[L_SINK] = 0; }
  }
  TSAT_SYNC();
  constexpr int CHB = TV_CHB;
  BwdOut<real> acc;
  acc.dV1 = 0; acc.dV2 = 0; acc.pd_ok = 1;
  for (int ch = (N - 1 + CHB - 1) / CHB - 1; ch >= 0 && acc.pd_ok; --ch) {
    const int k0 = ch * CHB;
    const int nk = (N - 1 - k0 < CHB) ? (N - 1 - k0) : CHB;
    tv_jacobian_chunk<real, DIAGJ>(p, N, n_tab, k0, nk, hl, frac);
    TSAT_SYNC();
    acc = riccati_chunk<real, 6, TvRec>(p.KD, k0, nk, (real)0, acc.dV1, acc.dV2);
    TSAT_SYNC();
  }
}
#endif

// `summary` (8 per slew) from `stats` (M per slew), summed in realisation order — the definitions of include/tortoise_hip.h
inline void ensemble_summary(int64_t T, int M, const tsat_tvlqr_stats* stats, double* summary) {
  for (int64_t t = 0; t < T; ++t) {
    const tsat_tvlqr_stats* s = stats + (size_t)t * M;
    double* o = summary + 8 * t;
    int fails = 0;
    double sum_ok = 0, mn = 0, mx = 0, sum_all = 0, ang = 0, w = 0;
    bool any = false;
    for (int m = 0; m < M; ++m) {
      sum_all += s[m].slew_time;
      if (m == 0 || s[m].final_angle > ang) ang = s[m].final_angle;
      if (m == 0 || s[m].final_w_norm > w) w = s[m].final_w_norm;
      if (s[m].failed) { ++fails; continue; }
      sum_ok += s[m].slew_time;
      if (!any || s[m].slew_time < mn) mn = s[m].slew_time;
      if (!any || s[m].slew_time > mx) mx = s[m].slew_time;
      any = true;
    }
    o[0] = (double)M; o[1] = (double)fails;
    o[2] = any ? sum_ok / (double)(M - fails) : 0.0;
    o[3] = mn; o[4] = mx;
    o[5] = sum_all / (double)M;
    o[6] = ang; o[7] = w;
  }
}

}  // namespace tsat
