// tsat_emu_line_search.cpp — the keep rule of the one-trajectory builds' line search (solve_trajectory in
// tortoisesat.jl_amd/csrc/tsat_device.hpp) under the CPU lane emulator (TEST INFRASTRUCTURE). Takes run_wave / for_each_wave,
// the emulated solve (run_block) and the packing code from tsat_emu.cpp as they are and adds a solve that is launched as the
// library launches it: the candidate slabs sized by tsat_batch_reserve's own function (reserved_slots of tsat_host_pack.hpp,
// a slab per candidate for a small batch) and the rule that tsat_set_store_policy sets, checked by the library's own
// check_store_policy. emu_solve_batch of tsat_emu.cpp itself stays at 12 slabs at most and the default rule.
// One-trajectory builds only (wide, and dense with -DTSAT_DENSE): the packed builds keep PK_STORE roll-outs whatever is reserved.
#include "tsat_emu.cpp"
#ifdef TSAT_PACKED
#error "the keep rule belongs to the one-trajectory builds"
#endif

// for the emulated launches that follow: the keep rule (few, hold) and the candidate slabs reserved per trajectory
// (slots; 0: as tsat_batch_reserve sizes them)
static int emu_store_few = N_FEW, emu_store_hold = LS_HOLD, emu_store_slots = 0;
extern "C" int emu_set_store_policy(int few, int hold, int slots) {
  if (!check_store_policy(few).empty() || slots < 0) return -1;
  emu_store_few = few; emu_store_hold = hold; emu_store_slots = slots;
  return 0;
}
extern "C" void emu_reset_store_policy(void) { emu_store_few = N_FEW; emu_store_hold = LS_HOLD; emu_store_slots = 0; }
extern "C" int emu_reserved_slots(int64_t T, int max_linesearch) { return reserved_slots(T, max_linesearch); }     // tsat_batch_reserve

// arguments: as emu_solve_batch
extern "C" int emu_ls_solve_batch(const tsat_options* o, int64_t T, int64_t n_btab, const double* x0, const double* xf,
                                  const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                                  const double* dt, const double* Jmat, const double* Qd, const double* Qfd,
                                  const double* Rd, const double* ulo, const double* uhi, const double* U0, double* X,
                                  double* U, double* K, tsat_stats* stats, double* trace, int trace_rows,
                                  const int32_t* n_knots) {
  const int N = o->n_knots, n_tab = o->n_tab;
  if (!check_options(*o, N, n_tab, o->max_linesearch).empty()) return -1;
  const int max_ls = emu_store_slots > 0 ? emu_store_slots : reserved_slots(T, o->max_linesearch);   // stored candidate slots
  std::vector<R> P((size_t)T * PSTRIDE), BT((size_t)n_btab * n_tab * 4), U0r(U0, U0 + (size_t)T * (N - 1) * 3);
  std::vector<int> bidx(T);
  pack_params<R>(T, x0, xf, tau0, dtau, dt, Jmat, Qd, Qfd, Rd, ulo, uhi, P.data());
  pack_btab<R>(n_btab, n_tab, Btab, BT.data());
  for (int64_t t = 0; t < T; ++t) bidx[t] = btab_idx ? btab_idx[t] : (int)t;
  std::vector<R> XU((size_t)T * xu_stride<R>(N), (R)0), KD((size_t)T * kd_stride<R>(N), (R)0),
      LAM((size_t)T * lam_stride<R>(N), (R)0), CAND((size_t)T * max_ls * xu_stride<R>(N), (R)0);
  KArgs<R> a;
  a.T = (int)T; a.N = N; a.n_tab = n_tab; a.max_ls = max_ls; a.opt = *o;
  a.ls_few = emu_store_few; a.ls_hold = emu_store_hold;
  a.P = P.data(); a.BT = BT.data(); a.bidx = bidx.data(); a.nk = n_knots; a.U0 = U0r.data();
  a.XU = XU.data(); a.KD = KD.data(); a.LAM = LAM.data(); a.CAND = CAND.data();
  a.stats = stats; a.trace = trace; a.trace_rows = trace_rows;
  std::vector<R> JW((size_t)((T + 3) / 4) * TSAT_JW_REALS_PER_4, (R)0);
  a.JW = JW.data();
  const int cls = inertia_class(T, Jmat);   // same variant selection as tsat_batch_upload
  using blk_t = void (*)(const KArgs<R>&, int);
  static const blk_t variants[2][3][2] = {
      {{run_block<3, 0, 0>, run_block<3, 0, 1>}, {run_block<3, 1, 0>, run_block<3, 1, 1>}, {run_block<3, 2, 0>, run_block<3, 2, 1>}},
      {{run_block<4, 0, 0>, run_block<4, 0, 1>}, {run_block<4, 1, 0>, run_block<4, 1, 1>}, {run_block<4, 2, 0>, run_block<4, 2, 1>}}};
  const blk_t blk = variants[o->integrator == 4 ? 1 : 0][cls][o->error_state ? 1 : 0];
  tsat_emu::for_each_wave((int)T, [&](int t) { blk(a, t); });
  for (int64_t e = 0; e < T * (int64_t)N; ++e) export_record<R>(e, N, n_knots, XU.data(), KD.data(), X, U, K);
  return 0;
}
