/*
 * tortoise_hip.h — C ABI of the MI355X-native batched AL-iLQR attitude-slew solver.
 *
 * This is the drop-in boundary for the ONE hot path of RoboticExplorationLab/TortoiseSat.jl:
 * the `TrajectoryOptimization.solve!(prob, solver)` call of src/TortoiseSat.jl:199 (and the old-API
 * `solve(solver,U)` of src/monte_carlo.jl:196) together with the dynamics callback it drives
 * (src/DerivFunction.jl:1-48).  A host (Julia `ccall`, Python `ctypes`, C++) builds the problem exactly
 * as the reference scripts do and then hands a whole *batch* of independent slews to `tsat_solve_batch`.
 *
 * Conventions
 *   - plain C, plain pointers and sizes, no callbacks, no torch/HIP types in signatures;
 *   - every function returns 0 on success, <0 on API error (text via tsat_last_error);
 *     per-trajectory outcomes are reported in tsat_stats.status, never as an error code;
 *   - arrays are Julia/Fortran column-major with the component fastest, then knot, then trajectory:
 *     X is reshape(X,7,N,T); U is reshape(U,3,N-1,T); K is reshape(K,3,7,N-1,T);
 *   - state x = [omega(3); q(4, scalar first)] — the reference's 8th "time" state
 *     (src/DerivFunction.jl:6,44) is folded into (tau0, dtau): the B-table row used at knot k, RK stage
 *     offset c in {0, 1/2, 1} is floor(fma(k + c, dtau, tau0)), clamped to [0, n_tab-1]
 *     (reference: B_ECI[floor(Int, t*N + 1), :], src/DerivFunction.jl:28);
 *   - controls are in units of u_scale A*m^2 (u_scale = 1e-2, src/DerivFunction.jl:37);
 *   - the library is synchronous and keeps no caller pointers after a call returns;
 *   - one handle per (host thread, GPU). Handles are not thread-safe.
 *
 * There is NO CPU fallback behind this ABI: if no gfx950 device is usable, tsat_create fails.
 */
#ifndef TORTOISE_HIP_H
#define TORTOISE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSAT_NX 7 /* omega(3) + quaternion(4)            (src/DerivFunction.jl:4-5)   */
#define TSAT_NU 3 /* magnetic dipole command (3)         (src/DerivFunction.jl:37)    */
#define TSAT_NC 6 /* control box rows per knot: u<=uhi, u>=ulo (src/TortoiseSat.jl:178) */
#define TSAT_MAX_LINESEARCH 32

/* per-trajectory outcome codes (tsat_stats.status) */
enum {
  TSAT_CONVERGED = 0,   /* c_max < constraint_tol after an inner solve                       */
  TSAT_MAX_OUTER = 1,   /* outer budget exhausted (src/TortoiseSat.jl:196 `iterations`)      */
  TSAT_REG_FAIL  = 2,   /* backward-pass regularisation exceeded reg_max                     */
  TSAT_DIVERGED  = 3    /* non-finite cost in the initial rollout (no backward sweep ran: K of
                           such a trajectory is undefined, X / U hold the overflowed rollout) */
};

/*
 * Solver options. Replaces AugmentedLagrangianSolverOptions{Float64}() + .opts_uncon
 * (src/TortoiseSat.jl:194-196) and solver.opts.* of the old API (src/monte_carlo.jl:187-192).
 * Field defaults (tsat_default_options) follow the published AL-iLQR/ALTRO algorithm, SURVEY.md App. A.
 */
typedef struct tsat_options {
  int32_t n_knots;          /* N, knot points incl. terminal (src/TortoiseSat.jl:85)                */
  int32_t n_tab;            /* rows in each B table                                                 */
  int32_t integrator;       /* 3 = rk3 (src/TortoiseSat.jl:146), 4 = rk4 (src/attitude_controller.jl:122) */
  int32_t precision;        /* 64 (fp64) or 32 (mixed precision, BASELINE.json configs[2]): float LINEARISATION — the   */
                            /* Jacobian lanes and the knot records they leave for the Riccati recursion — while the      */
                            /* roll-out, the costs, the recursion, the gains and every array in HBM stay double, so the   */
                            /* line-search decisions follow the fp64 path; tsat_mpc_run takes 64 only                     */
  int32_t max_outer;        /* opts_al.iterations            (src/TortoiseSat.jl:196; 20)           */
  int32_t max_inner;        /* opts_al.opts_uncon.iterations (src/TortoiseSat.jl:195; 50)           */
  int32_t max_linesearch;   /* backtracking trials alpha = 2^-j, j < max_linesearch (<= 32)         */
  int32_t dj_counter_limit; /* solver.opts.dJ_counter_limit  (src/monte_carlo.jl:191)               */
  double  cost_tol;         /* inner: stop when 0 < dJ < cost_tol                                   */
  double  grad_tol;         /* inner: stop when mean_k max_i |d|/(|u|+1) < grad_tol                 */
  double  constraint_tol;   /* outer: stop when c_max < constraint_tol                              */
  double  penalty_init, penalty_scale, penalty_max, dual_max;
  double  reg_init, reg_scale, reg_min, reg_max, reg_fp;
  double  ls_lower, ls_upper;
  double  max_state;        /* rollout rejected when |x_i| or |u_i| exceeds this                     */
  double  u_scale;          /* 1e-2 (src/DerivFunction.jl:37)                                        */
  int32_t terminal_mask;    /* bit i set: state component i has a terminal equality x_N[i]=xf[i]
                               (goal_constraint, src/TortoiseSat.jl:182,188)                         */
  int32_t error_state;      /* 0: plain 7-state differences (Model(DerivFunction,8,3), src/TortoiseSat.jl:145)
                               1: the quaternion hooks Model(f!,n,m,quaternion_error,quaternion_expansion)
                                  (src/monte_carlo.jl:158): state difference [dw; MRP(q^-1 (x) q_new)]
                                  (src/quaternion_toolbox.jl:58-75), dynamics blocks E(q_{k+1})'AE(q_k), E(q_{k+1})'B
                                  (src/attitude_controller.jl:59-81), cost expansion projected through E(q)
                                  (src/quaternion_toolbox.jl:15-50); gains K act on the 6 error coordinates and
                                  are returned with a zero 7th column */
} tsat_options;

/* per-trajectory result record */
typedef struct tsat_stats {
  int32_t status;       /* TSAT_* code                                                    */
  int32_t outer_iters;  /* AL outer iterations executed                                   */
  int32_t inner_iters;  /* total iLQR iterations over all outer iterations                */
  int32_t ls_trials;    /* line-search candidates a sequential backtracking search would
                           have rolled out (index of accepted alpha + 1, summed)          */
  int32_t n_backward;   /* backward sweeps executed (incl. regularisation restarts)       */
  int32_t n_forward;    /* forward sweeps executed on this backend: 1 + one per line search,
                           + one for each search whose winner the sweep had not kept
                           (tsat_set_store_policy; none below 2048 trajectories when the
                           searches that follow a deep one are deep too)                  */
  int32_t bp_restarts;  /* backward sweeps abandoned on a non-PD Quu                      */
  int32_t fp_fails;     /* line searches in which no alpha was accepted                   */
  double  cost;         /* LQR objective of the returned trajectory (no AL terms)         */
  double  cost_al;      /* augmented-Lagrangian cost at exit                              */
  double  c_max;        /* max constraint violation of the returned trajectory            */
  double  grad;         /* last Todorov gradient                                          */
} tsat_stats;

typedef struct tsat_handle tsat_handle;

/* library/ABI version: major*100 + minor */
int  tsat_version(void);

/* fill *o with defaults (rk3, 20 x 50 budget as src/TortoiseSat.jl:195-196, ALTRO constants) */
void tsat_default_options(tsat_options* o);

/* open GPU `device_id` (must be a gfx950 device); replaces AugmentedLagrangianSolver(prob,opts)
 * (src/TortoiseSat.jl:197) as the object that owns solver workspace. */
int  tsat_create(tsat_handle** h, int device_id);
int  tsat_destroy(tsat_handle* h);
const char* tsat_last_error(const tsat_handle* h);

/*
 * One-call drop-in for solve!(prob, solver) over a batch of T independent slews
 * (src/TortoiseSat.jl:199; loop body of src/monte_carlo.jl:118-235). Host pointers in, host pointers out.
 *   x0, xf  7 x T            initial / goal state              (src/TortoiseSat.jl:124,130)
 *   Btab    3 x n_tab x n_btab  ECI field tables [T]           (global B_ECI, src/TortoiseSat.jl:89)
 *   btab_idx T (or NULL)     table used by trajectory t (NULL: t, requires n_btab == T)
 *   tau0, dtau  T            table row of knot 0 and rows per knot (see header comment)
 *   dt      T                step [s]                          (src/TortoiseSat.jl:84)
 *   Jmat    9 x T            inertia, column-major 3x3         (src/input_parameters.jl:29-51)
 *   Qd,Qfd  7 x T, Rd 3 x T  diagonal LQR weights              (src/TortoiseSat.jl:157-169)
 *   ulo,uhi 3 x T            control box                       (src/TortoiseSat.jl:178)
 *   U0      3 x (N-1) x T    initial controls                  (initial_controls!, src/TortoiseSat.jl:191)
 *   X       7 x N x T  out;  U  3 x (N-1) x T out;  K 3 x 7 x (N-1) x T out (may be NULL);  stats T out
 */
int  tsat_solve_batch(tsat_handle* h, const tsat_options* o, int64_t T, int64_t n_btab,
                      const double* x0, const double* xf, const double* Btab, const int32_t* btab_idx,
                      const double* tau0, const double* dtau, const double* dt, const double* Jmat,
                      const double* Qd, const double* Qfd, const double* Rd,
                      const double* ulo, const double* uhi, const double* U0,
                      double* X, double* U, double* K, tsat_stats* stats);

/*
 * Resident-batch API (what tsat_solve_batch is made of). Lets a caller keep a batch in HBM, re-run it,
 * time only the solve, and export results straight into device buffers it owns (e.g. for an RCCL all-gather).
 */
int  tsat_batch_reserve(tsat_handle* h, int64_t T, int32_t n_knots, int32_t n_tab, int64_t n_btab,
                        int32_t max_linesearch);
int  tsat_batch_upload(tsat_handle* h,
                       const double* x0, const double* xf, const double* Btab, const int32_t* btab_idx,
                       const double* tau0, const double* dtau, const double* dt, const double* Jmat,
                       const double* Qd, const double* Qfd, const double* Rd,
                       const double* ulo, const double* uhi, const double* U0);
/* Ragged batches: give trajectory t its own knot count n_knots[t] in [2, N] (NULL: all N again). Replaces the
 * per-run horizon of the reference's Monte-Carlo, t_total[i] = 0:0.2:t_final[i] (src/monte_carlo.jl:140-145).
 * Arrays keep the common stride N; U0 entries beyond a trajectory's horizon are ignored and its X/U/K slabs are
 * returned zero-filled beyond it. Call after tsat_batch_upload. */
int  tsat_batch_knots(tsat_handle* h, const int32_t* n_knots /* T */);
/* run the solve on the resident batch; blocks until done. It starts from the RESIDENT x0 / tau0 / U0: those are the uploaded
 * ones unless tsat_mpc_run has advanced them since (see there) — upload again to start over.
 * *kernel_ms (may be NULL) receives the HIP-event time of the solve kernel on the handle's stream. */
int  tsat_batch_run(tsat_handle* h, const tsat_options* o, float* kernel_ms);
/* unpack results to HOST buffers (any may be NULL) */
int  tsat_batch_download(tsat_handle* h, double* X, double* U, double* K, tsat_stats* stats);
/* unpack results to DEVICE buffers owned by the caller on the same GPU (any may be NULL); blocks */
int  tsat_batch_export_device(tsat_handle* h, void* X_dev, void* U_dev, void* K_dev, void* stats_dev);
/* bytes of HBM currently reserved by the handle for the resident batch */
int64_t tsat_batch_bytes(const tsat_handle* h);
/* The stages around the solve (downloads, gathers, tracking, horizon, field tables, receding-horizon history) keep grow-only
 * device workspaces in the handle so that repeated calls pay no allocation; after ONE large download or gather they hold
 * multi-GB staging buffers for the life of the handle. tsat_workspace_bytes reports them; tsat_workspace_trim frees them:
 *   what = 0  the staging buffers of tsat_batch_download and tsat_sweep_allgather only
 *   what = 1  every workspace — including the resident field tables of tsat_btable_batch(Btab = NULL), which are then gone
 * They are allocated again on the next call that needs them. */
int64_t tsat_workspace_bytes(const tsat_handle* h);
int  tsat_workspace_trim(tsat_handle* h, int32_t what);
/* optional per-iteration trace for debugging parity: rows of 8 doubles
 * [outer, inner, J_prev, J_new, alpha_index(-1 = none), rho, dV1, dV2], `rows` per trajectory.
 * Pass rows = 0 to disable. Call before tsat_batch_run; read back with tsat_batch_trace_download. */
int  tsat_batch_trace(tsat_handle* h, int32_t rows);
int  tsat_batch_trace_download(tsat_handle* h, double* trace /* 8 x rows x T */);

/* ------------------------------------------------------------------------------------------------------------
 * Closed-loop tracking of a solved slew (the caller right after solve! in the reference): TVLQR gains around the
 * optimised trajectory + simulation + the slew-time statistic.
 *   attitude_simulation(f!, f_gains!, :rk4, X, U, dt, x0_lqr, t0, tf, Q_lqr, R_lqr, Qf_lqr)   src/attitude_controller.jl:1-48
 *   attitude_lqr (Jacobians + G(q) reduction + Riccati)                                         src/attitude_controller.jl:50-119
 *   simulator / gain_simulator (plant with / without injected noise)                            src/simulator.jl, src/gain_simulator.jl
 *   slew-time / failure statistic                                                               src/monte_carlo.jl:242-262
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct tsat_tvlqr_options {
  int32_t n_knots;          /* N                                                                              */
  int32_t n_tab;            /* rows in each B table                                                           */
  int32_t linearize_dt_sq;  /* 1: gains linearised over a step of dt^2 (the reference's `dt = S[end]^2`,
                               src/attitude_controller.jl:137); 0: over dt                    */
  int32_t min_steps;        /* statistic ignores the first min_steps samples (10, src/monte_carlo.jl:251)     */
  double  u_scale;          /* 1e-2: `u/100` (src/gain_simulator.jl:42)                                       */
  double  w_tol;            /* 0.05 rad/s   (src/monte_carlo.jl:70)                                           */
  double  angle_tol;        /* 0.08727 rad  (src/monte_carlo.jl:71)                                           */
  int32_t noise_mode;       /* 0: the `noise` array (NULL = noise-free plant); 1: drawn inside the kernel, below */
  int32_t rate_as_written;  /* (a reserved word before version 300: values other than 0 / 1 are rejected — fill the struct with
                               tsat_tvlqr_default_options first.) statistic: 0 (default) |w| of sample j; 1 the line as the reference has it,
                               `omega_norm_vec[j] = norm(sim_states[i][1:3,i])` (src/monte_carlo.jl:247): for every j the
                               rate of sample i, the 1-based number of the trial (`noise_id` + 1, or the position in the
                               batch + 1) — past the end of a shorter trajectory Julia raises a BoundsError, here the
                               last sample is taken                                                           */
  uint64_t noise_seed;      /* key of the counter-based generator                                             */
  double  sigma_gyro;       /* (0.38 deg)^2: `randn(3,1)*(.38*pi/180)^2`, src/simulator.jl:5                  */
  double  sigma_att;        /* (1 deg)^2:    `randn(3,1)*(1*pi/180)^2`,   src/simulator.jl:10                 */
  double  field_amp;        /* (1e-5)^2:     `rand(3)*1e-5^2`,            src/simulator.jl:22                 */
} tsat_tvlqr_options;

/* noise_mode = 1: the nine draws of plant evaluation (trajectory id, knot k, RK4 stage s) come from Philox4x32-10 with
 * key (noise_seed lo, hi) and counters (id lo, id hi, k, 4 s + j), j = 0, 1, 2 -> words w[j][0..3]:
 *   U(w) = (w + 0.5) 2^-32;  (z, z') = sqrt(-2 ln U(a)) (cos, sin)(2 pi U(b))          (Box-Muller)
 *   gyro   = sigma_gyro (z(w00,w01), z'(w00,w01), z(w02,w03))
 *   att    = sigma_att  (z'(w02,w03), z(w10,w11), z'(w10,w11))
 *   field  = field_amp  (U(w12), U(w13), U(w20))
 * The plant turns the normalised attitude by the rotation vector att: q (x) [cos(th/2); att * (th == 0 ? 1/2 : sin(th/2)/th)],
 * th = |att| as computed (a triple whose squares underflow counts as zero). sigma_att = 0 — "gyro noise only", or a wrapper's
 * sigma_scale = 0 — is therefore no rotation, and all three levels zero is the noise-free plant up to the one extra
 * normalisation of the quaternion, where the reference's r_noise = q_noise / th_noise (src/simulator.jl:12) is 0/0.
 * id = noise_id[t] (NULL: t), so a sweep draws the same noise however it is sharded or chunked. The reference draws
 * from Julia's global generator inside `simulator`; any generator is as faithful, this one is reproducible. */

typedef struct tsat_tvlqr_stats {
  int32_t slew_index;       /* first 1-based sample j > min_steps with |w| < w_tol (rate_as_written: see the options) and
                               error angle < angle_tol; 0 = none                                              */
  int32_t failed;           /* 1 when no such sample exists (`fails[i]`, src/monte_carlo.jl:258-261)           */
  double  slew_time;        /* dt * slew_index, or dt * N when failed (`slew_time[i]`, :237,252)               */
  double  final_w_norm;     /* |w| of the last simulated sample                                                */
  double  final_angle;      /* error angle of the last simulated sample                                        */
} tsat_tvlqr_stats;

void tsat_tvlqr_default_options(tsat_tvlqr_options* o);

/*
 * Host pointers in and out, column-major as everywhere in this ABI.
 *   X 7xNxT, U 3x(N-1)xT        the optimised trajectories (outputs of tsat_solve_batch)
 *   xf 7xT                       goal state: its quaternion is `q_final` of the statistic
 *   Btab, btab_idx, tau0, dtau, dt, Jmat   as for tsat_solve_batch
 *   Qd, Qfd 6xT, Rd 3xT          diagonals of Q_lqr, Qf_lqr, R_lqr (src/TortoiseSat.jl:251-260)
 *   x0_sim 7xT                   perturbed initial state x0_lqr (src/TortoiseSat.jl:227-234)
 *   noise 9x4x(N-1)xT or NULL    per step and RK4 stage: gyro noise(3), attitude-noise rotation vector(3), field
 *                                noise(3) — the values the reference draws inside `simulator` (src/simulator.jl:5,10,22);
 *                                an attitude triple of norm zero (as computed: squares that underflow included) is no
 *                                rotation, the rule stated at noise_mode = 1 above; zeros are valid values;
 *                                NULL = noise-free plant (`gain_simulator`)
 *   X_sim 7xNxT, U_sim 3x(N-1)xT, K_lqr 3x6x(N-1)xT (each may be NULL: only what is asked for travels back), stats T   outputs
 *   n_knots T or NULL            per-trajectory horizons as for tsat_batch_knots (`t_total[i]`, src/monte_carlo.jl:145):
 *                                trajectory t is tracked over its first n_knots[t] samples, the rest of its slabs is
 *                                zero and its statistic counts n_knots[t] samples; NULL = all N
 *   noise_id T or NULL           generator ids of the trajectories when options.noise_mode = 1
 */
int  tsat_tvlqr_batch(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab,
                      const double* X, const double* U, const double* xf,
                      const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                      const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                      const double* x0_sim, const double* noise,
                      double* X_sim, double* U_sim, double* K_lqr, tsat_tvlqr_stats* stats,
                      const int32_t* n_knots, const int64_t* noise_id);

/* Build of the solve kernel used by tsat_batch_run / tsat_solve_batch / tsat_mpc_run. 0 = automatic (default), by batch size:
 *   1 wide    one trajectory per wavefront, one wavefront per SIMD (40 KB of LDS, full register file): up to 1024 trajectories;
 *   2 dense   one trajectory per wavefront, two wavefronts per SIMD (20 KB, 256 registers): 1025 .. 2047;
 *   3 packed  four trajectories per wavefront share every forward sweep (16 line-search candidates each) and run their
 *             backward sweeps together (Jacobian lanes = trajectory x knot x column quarter, Riccati recursion on 16 lanes per
 *             trajectory), two wavefronts per SIMD: never automatically;
 *   4 packed8 the same with eight trajectories per wavefront (eight candidates each, two backward passes): 8193 .. 16383;
 *   5 packed8w  eight trajectories per wavefront at ONE wavefront per SIMD (40 KB of LDS: twelve of a backward pass's sixteen knot
 *             records stay on the chip instead of four, all sixteen float ones; the whole register file: no spills): 4097 .. 8192;
 *   6 packed16w sixteen trajectories per wavefront (four candidates each) at one wavefront per SIMD: from 16384, unless the
 *             iteration budget max_outer * max_inner is 100 or more (then packed8: a wavefront lasts as long as its slowest trajectory).
 *   7 packed4w  four trajectories per wavefront at one wavefront per SIMD: 2048 .. 4096 (the receding-horizon loop of 4096).
 * precision = 32 has the dense layout and the packed ones (below 2048 trajectories the dense one; `variant` 1 means 2 there).
 * The builds of one precision give bit-identical results (X, U, K, iteration counts; `n_forward` counts the sweeps a build
 * executed and differs). The switch exists for tuning and for the tests. */
int  tsat_set_kernel_variant(tsat_handle* h, int32_t variant);

/* Endgame of the packed builds (variants 3 to 7). The trajectories of one launch need different numbers of iterations (21 .. 150
 * on the inclination sweep of src/paper_images/heatmap.jl:139-185 with its 3 x 50 budget), and a wavefront that holds four or
 * eight of them lasts as long as its slowest: towards the end of a launch a few wavefronts with several long trajectories keep
 * running while the rest of the machine is idle. Once at most `suspend_at` trajectories of the batch are still iterating, every
 * wavefront therefore parks its live ones (state in HBM) and ends, and a second kernel, queued behind the first on the same
 * stream, continues each of them on a wavefront of its own.
 *   -1  automatic (default): an eighth of the batch, at most 2048, when max_outer * max_inner >= 20; never otherwise;
 *    0  never;  n > 0: at n live trajectories.
 * Results do not depend on it (X, U, K, costs, iteration counts: bit-identical); `n_forward`, the sweeps that were executed,
 * does. For tuning and for the tests. */
int  tsat_set_endgame(tsat_handle* h, int32_t suspend_at);

/* Keep rule of the one-trajectory builds (variants 1 and 2, and the continuation of a packed launch's last trajectories). One
 * forward sweep rolls out every candidate of a line search at once; how many of the roll-outs it keeps in HBM (80 B per knot
 * each) decides whether the accepted one is at hand or takes another sweep — half an iteration, on the trajectory the whole
 * launch may be waiting for. A sweep keeps
 *   `few` roll-outs                while the trajectory's line searches end early (default 4), and
 *   every reserved slot            in the iteration after a search that accepted index >= few - 1 or none at all, and in the
 *                                  `hold` iterations after that one (default 8; 0: that iteration only; negative: in every
 *                                  iteration that follows, to the end of the solve).
 * few >= max_linesearch keeps every roll-out always. Batches of fewer than 2048 trajectories reserve a slot for each of the
 * max_linesearch candidates (tsat_batch_reserve), larger ones 12 at most: there a deeper search still takes a further sweep.
 * Results do not depend on the rule (X, U, K, costs, iteration counts: bit-identical); `n_forward`, the sweeps that were
 * executed, does. For tuning and for the tests. */
int  tsat_set_store_policy(tsat_handle* h, int32_t few, int32_t hold);

/* What the next tsat_batch_run / tsat_mpc_run with options `o` will launch on the reserved batch: *build = 1 wide, 2 dense,
 * 3 packed, 4 packed8, 5 packed8w, 6 packed16w, 7 packed4w (of the precision `o` names), *endgame_at = the live count at which a packed launch parks its trajectories
 * (0: no endgame). For reports (bench.py labels its lines with it); either pointer may be NULL. */
int  tsat_selected_build(tsat_handle* h, const tsat_options* o, int32_t* build, int32_t* endgame_at);

/* The same tracking for the RESIDENT batch right after tsat_batch_run: reference trajectories, field tables, table
 * clocks, inertias, goal states and per-trajectory horizons are the ones already on the device — nothing of the solve
 * travels back and forth between the two calls (src/monte_carlo.jl:196 -> :230). n_knots / n_tab of `o` are ignored. */
int  tsat_tvlqr_resident(tsat_handle* h, const tsat_tvlqr_options* o, const double* Qd, const double* Qfd,
                         const double* Rd, const double* x0_sim, const double* noise,
                         double* X_sim, double* U_sim, double* K_lqr, tsat_tvlqr_stats* stats, const int64_t* noise_id);

/* Closed-loop tracking of T solved slews under M noise realisations each: TVLQR gains once per slew, then M plants
 * (one Monte-Carlo trial of src/monte_carlo.jl:199-262 per realisation; lane of a wavefront = realisation).
 *   everything up to Rd        as for tsat_tvlqr_batch (same shapes, same meaning)
 *   M                          realisations per slew, 1 .. 65535
 *   x0_sim     7 x M x T       perturbed initial state of realisation m of slew t (x0_lqr, src/monte_carlo.jl:204-210)
 *   noise_id0  T or NULL       realisation m of slew t draws generator id noise_id0[t] + m  (NULL: t * M + m),
 *                              with the draw layout documented at tsat_tvlqr_options (Philox4x32-10, counters id, knot, stage)
 *   n_knots    T or NULL       per-slew horizons as for tsat_tvlqr_batch
 *   stats      M x T   out     the slew-time statistic of every realisation (realisation fastest)
 *   summary    8 x T   out     per slew, from `stats`, summed in realisation order on the host:
 *                              [0] M  [1] failures  [2] mean slew_time of the realisations that did not fail (0 if none)
 *                              [3] min and [4] max of the same (0 if none)
 *                              [5] mean slew_time of all M (a failure counts dt * n_knots, as `slew_time[i]` does, src/monte_carlo.jl:237)
 *                              [6] max final_angle  [7] max final_w_norm
 *   stats_nominal T out, may be NULL   statistic of the noise-free plant started at the plan's own first state X[:,1,t]
 *   K_lqr      3 x 6 x (N-1) x T out, may be NULL     the gains, as tsat_tvlqr_batch returns them
 *   X_sim      7 x N x M x T out, may be NULL         every simulated state (for tests and plots; not a fast path)
 * Realisation (t, m) is exactly what tsat_tvlqr_batch computes for slew t with x0_sim = x0_sim[:, m, t], noise_mode = 1,
 * noise_id = noise_id0[t] + m; the statistic is evaluated while the roll-out runs.
 * o->noise_mode must be 1 (the noise is drawn in the kernel; an array would be 36 (N-1) M T doubles) and
 * o->rate_as_written must be 0 (that reading needs a sample that may lie after the one being judged); both are rejected with -1. */
int  tsat_tvlqr_ensemble(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim);
/* text of the last failure of tsat_tvlqr_ensemble / tsat_tvlqr_ensemble_dispersed / tsat_tvlqr_ensemble_gg on the calling thread ("" if none) */
const char* tsat_ensemble_last_error(void);

/* The same ensemble with a PLANT OF ITS OWN per realisation and the actuator's limit on the feedback command: what decides
 * whether a magnetorquer-only slew arrives is plant / model mismatch, which the noise of tsat_tvlqr_ensemble does not contain.
 * Realisation (t, m) is the closed loop of tsat_tvlqr_ensemble (same gains — computed once per slew from the MODEL inertia
 * Jmat[t] —, same x0_sim, generator id, draw layout, noise injection, RK4 plant integrator and statistic) except that per knot
 *   u_cmd = U_k - K_k dX_k                                    (units of u_scale A m^2, as before)
 *   u_sat = min(max(u_cmd, sat_lo[t]), sat_hi[t])             component-wise; a knot counts as clipped when any component changed
 *   dipole seen by the plant, all four RK4 stages of the knot = G[t,m] u_sat u_scale + m_res[t,m]   (A m^2)
 * and the rigid body has inertia Jp[t,m] instead of Jmat[t].
 *   plant      21 x M x T      per realisation: Jp (9, column-major 3x3, symmetric positive definite, kg m^2),
 *                              G (9, column-major 3x3: applied dipole = G * limited command; identity = ideal),
 *                              m_res (3, A m^2, body frame)
 *   sat_lo, sat_hi  3 x T each, units of u_scale; both NULL = unlimited (an infinite entry leaves that side open)
 *   n_clipped  M x T out, may be NULL    clipped knots of every realisation
 *   everything else            exactly as tsat_tvlqr_ensemble
 * stats_nominal is the noise-free MODEL plant (Jmat — taken as the symmetric tensor of its upper triangle —, G = I, m_res = 0)
 * from X[:,1,t], with the limits applied.
 * Rejected with -1 (text with the offending (t, m) in tsat_ensemble_last_error): plant NULL, a non-finite plant entry, Jp not
 * symmetric (|Jp - Jp'| > 1e-12 max|Jp|) or not positive definite, exactly one of the two limit arrays NULL, sat_lo > sat_hi,
 * and everything tsat_tvlqr_ensemble rejects. */
#define TSAT_PLANT_W 21
int  tsat_tvlqr_ensemble_dispersed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped);

/* tsat_tvlqr_ensemble_dispersed UNDER GRAVITY-GRADIENT TORQUE: the one external disturbance torque of the library. Every plant
 * above feels m x B alone; for an elongated body in low orbit the gravity gradient is the largest missing term (3 GM / r^3 =
 * 3.85e-6 s^-2 at 400 km: 8e-8 N m on a 3U inertia, a fifth of the authority of 0.01 A m^2 in 4e-5 T). It depends on the
 * realisation's own inertia Jp, so it is a dispersion like the others; the solver's model and the gains do NOT contain it.
 *   Rtab   3 x n_tab x n_btab   orbit positions, km, ECI: row i is the position at which field row i of Btab was evaluated
 *                               (`pos` of tsat_btable_batch); indexed exactly like Btab — same btab_idx, same row
 *                               floor(fma(c, dtau, tau)) clamped to [0, n_tab - 1]
 *   gm     km^3 / s^2           (3.986004418e5 for the Earth); 0 switches the term off
 * A pack launch turns row i into r^ = r / |r| and g = 3 gm / |r|^3 (s^-2). In every RK4 stage of a plant step, with x the stage's
 * state as integrated (BEFORE the noise injection), q = x[3:7] / |x[3:7]| and the row of the stage (c = 0, 1/2, 1/2, 1: the index of
 * the stage's field row):
 *   r_b    = qrot(q, r^)                     the rotation the field row gets
 *   tau_gg = g (r_b x (Jp r_b))              N m, Jp the realisation's inertia in kg m^2
 *   k[0:3] += (h inv(Jp)) tau_gg             added to the stage's increment after the plant's own evaluation
 * Everything else of realisation (t, m) is that of tsat_tvlqr_ensemble_dispersed: command rule, limits, G, m_res, noise draws and
 * their injection, statistic, table clock. stats_nominal is the noise-free MODEL plant flying through the same gravity field with
 * Jmat: the environment is not the model's choice. gm = 0 reproduces tsat_tvlqr_ensemble_dispersed bit for bit (through the same
 * kernel as any other gm). The packed rows (32 n_tab n_btab bytes) are a grow-only workspace of the handle: counted by
 * tsat_workspace_bytes, freed by tsat_workspace_trim(h, 1).
 * Rejected with -1 (text in tsat_ensemble_last_error): Rtab NULL, a non-finite entry of Rtab, a row with |r| = 0, gm non-finite or
 * negative, and everything tsat_tvlqr_ensemble_dispersed rejects. */
int  tsat_tvlqr_ensemble_gg(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm);

/* The PROJECTION PD LAW on the plants of tsat_tvlqr_ensemble_gg: the baseline the tracked plans are compared against — the
 * feedback every magnetorquer satellite carries needs no plan, no gains, no Jacobian pass and no Riccati recursion. The
 * reference's form of it: psiaki_controller (src/comparison/psiaki_dynamics.jl:1-26), flown around a reference trajectory by
 * src/comparison/psiaki2005.jl:139-164, with the direction-preserving limit nominal_input_psiaki (psiaki_dynamics.jl:127-143).
 * Those scripts are experimental; this is the law as defined HERE (deviations: their rate term has the opposite sign of their
 * attitude term, their q~ = q (x) q_guess has no inverse, they have no shortest-rotation rule, inv(J) is folded into kp here,
 * and their m_limit is an unused argument).
 * At knot k, x the realisation's current TRUE state (as the TVLQR feedback sees it), xr the reference record of the knot:
 *   dw      = x[0:3] - xr[0:3]
 *   e       = conj(xr[3:7]) (x) x[3:7]                 the product of the TVLQR feedback, with its scalar part e0
 *   s       = (e0 < 0) ? -1 : 1                        shortest rotation
 *   Treq[c] = -(kd[c] dw[c] + kp[c] (s e[1+c]))        N m
 *   b       = qrot(x[3:7] / |x[3:7]|, field row floor(fma(k, dtau, tau0)) clamped)     the stage-0 row, no noise
 *   m       = (b x Treq) / (b . b)                     A m^2;  m = 0 when b . b == 0 (the last row of a magnetic_simulation
 *                                                      table is zero, and the clock clamps onto it)
 *   u_cmd   = (feedforward ? U_k : 0) + m / o->u_scale        units of u_scale, as every command of this ABI
 * then the limit:
 *   limit_mode 0   the component clip of tsat_tvlqr_ensemble_dispersed
 *   limit_mode 1   beta = max_c r_c, r_c = u_c / hi_c if u_c > 0, u_c / lo_c if u_c < 0, 0 if u_c == 0; if beta > 1 every component
 *                  becomes u_c (1 / beta) (the direction is kept), otherwise the command is unchanged
 * a knot counts as clipped when the limit changed any component; after it G u_sat + m_res / u_scale is held over the four RK4
 * stages. Everything not named below keeps its meaning, shape, layout and validation from tsat_tvlqr_ensemble_gg: the plant
 * record, the draw layout and its per-stage injection, the RK4 plant, the table clock, the gravity-gradient term, the statistic
 * evaluated while the roll-out runs, summary, ragged n_knots, zero fill beyond a horizon. Of `o`, noise_mode must be 1 and
 * rate_as_written 0; linearize_dt_sq is ignored.
 *   X      7 x N x T or NULL       reference record of knot k = X[:,k,t]; NULL = REGULATION: the record of every knot is xf[:,t],
 *                                  and nothing of size N is uploaded (N = 100 000 costs no device memory beyond X_sim, if asked for)
 *   U      3 x (N-1) x T           read only when feedforward = 1; may be NULL otherwise
 *   kd, kp 3 x T each              per-axis rate gain (N m s / rad) and attitude gain (N m), finite and >= 0; the reference's
 *                                  form is kp = C2 / J_ii
 *   feedforward  0 | 1             limit_mode  0 | 1
 *   x0_nom 7 x T or NULL           start of the noise-free MODEL plant of stats_nominal; NULL = X[:,1,t]
 *   plant  21 x M x T or NULL      NULL: every realisation flies the model's plant (Jmat as the symmetric tensor of its upper
 *                                  triangle, G = I, m_res = 0), as in tsat_mpc_run_dispersed
 *   Rtab   may be NULL only with gm == 0: then the kernel without the gravity rows is launched; with Rtab the one with them,
 *                                  whatever gm is (gm = 0 gives the same states bit for bit)
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): kd or kp NULL, non-finite or
 * negative; feedforward not 0 or 1; feedforward = 1 with X or U NULL; limit_mode not 0 or 1; limit_mode = 1 with the limits NULL
 * or without lo < 0 < hi in every component; X NULL with stats_nominal non-NULL and x0_nom NULL; Rtab NULL with gm != 0; and
 * everything tsat_tvlqr_ensemble_gg rejects except the NULL plant and NULL Rtab above. */
int  tsat_pd_ensemble(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm);

/* The ASYMPTOTIC PERIODIC LQR on the plants of tsat_pd_ensemble: the model-based constant-P regulator that the reference's
 * comparison figure plots against the tracked plans ("APLQR", src/comparison/psiaki2001_Period_LQR.jl). Two calls: the gain
 * synthesis on the device (tsat_aplqr_gains) and the roll-out (tsat_aplqr_ensemble), which flies whatever gain it is handed.
 * Restated from magnetic_control_effectiveness (src/comparison/psiaki_dynamics.jl:75-98), Pss_psiaki (:101-125) and
 * nominal_input_psiaki (:127-143); this is the law as defined HERE. Deviations:
 *   frame             the reference's goal is fixed in the local-level frame and its A carries orbit-rate and gravity-gradient
 *                     terms; every goal of this ABI is inertial (xf), so A is the double integrator [[0, I], [0, 0]] and the field
 *                     is averaged in the goal's body frame
 *   no square root    the reference forms B~ = sqrt(alpha) and hands it to care; only B~ B~' = Gamma enters the equation
 *   attitude error    quaternion_euler(q) there; here the rotation vector to first order, 2 s e[1:4], with the PD law's sign s
 *   general inertia   inv(J) is the full inverse of Jmat, not 1 / J_ii row scalings
 *   limits            the reference scales the command back against U_max; here limit_mode 0 or 1 is tsat_pd_ensemble's
 * SYNTHESIS, per slew t (one wavefront each; state z = [theta (3); dw (3)]):
 *   beta_j = qrot(xf[3:7,t] / |xf[3:7,t]|, row j of the slew's table)
 *   B_j    = -inv(J) hat(beta_j)                                           3 x 3
 *   Gamma  = (1/n) sum_{j = avg_lo .. avg_hi-1} B_j diag(1/rd) B_j'        n = avg_hi - avg_lo
 *   G = blockdiag(0, Gamma),  Q = diag(qd)
 *   P      : A'P + P A - P G P + Q = 0,  P symmetric, A - G P stable
 *   Kg     = alpha inv(J) P[3:6, 0:6]                                      3 x 6
 * P by the matrix sign function of the Hamiltonian [[A, -G], [-Q, -A']]: Z <- (c Z + inv(Z) / c) / 2, c = |det Z|^(-1/12), the
 * inverse by Gauss-Jordan with partial pivoting, until |dZ|_1 <= 1e-14 |Z|_1 or 32 iterations; then [W12; W22 + I] P =
 * -[W11 + I; W21] in the least-squares sense by a Gram-Schmidt QR (the normal equations would square its condition), symmetrised.
 *   avg_lo, avg_hi  int32 x T, or both NULL for the whole table [0, n_tab)
 *   qd 6 x T, rd 3 x T   finite and > 0          alpha T   finite and >= 0          res_tol > 0
 *   Kg 3 x 6 x T         P_ss 6 x 6 x T or NULL          Gamma 3 x 3 x T or NULL
 *   info   T records of tsat_aplqr_info: status 0 ok; 1 not converged in 32 iterations; 2 a zero or non-finite pivot;
 *          3 residual > res_tol, with residual = |A'P + P A - P G P + Q|_F / (2 |A|_F |P|_F + |G|_F |P|_F^2 + |Q|_F). pivot_min is
 *          the smallest |pivot| of all eliminations of the slew and of the diagonal of the QR's triangular factor. On any status other than 0 the slew's Kg and P_ss are zero-filled,
 *          never non-finite, and the call still returns 0.
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): a null handle or array; exactly
 * one of avg_lo / avg_hi NULL; a window without 0 <= avg_lo < avg_hi <= n_tab; btab_idx out of range, or NULL with n_btab != T;
 * qd or rd non-finite or <= 0; alpha non-finite or negative; res_tol not > 0; a non-finite or singular Jmat; a zero or non-finite
 * goal quaternion. */
struct tsat_aplqr_info {
  int32_t status;
  int32_t iterations;       /* of the sign iteration, the one a failed elimination stopped included */
  double  residual;         /* 0 unless the iteration converged and the QR that P is solved from went through */
  double  pivot_min;
};
typedef struct tsat_aplqr_info tsat_aplqr_info;
int  tsat_aplqr_gains(tsat_handle* h, int64_t T, int64_t n_btab, int32_t n_tab, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const int32_t* avg_lo, const int32_t* avg_hi,
                         const double* Jmat, const double* qd, const double* rd, const double* alpha, double res_tol,
                         double* Kg, double* P_ss, double* Gamma, void* info);

/* ROLL-OUT: tsat_pd_ensemble with the command of knot k replaced. y and B are what the law sees of the realisation's state and of
 * the stage-0 field row, exactly as the PD law takes them; xr the record X[:,k,t], or xf[:,t] when regulating:
 *   dw    = y[0:3] - xr[0:3];   e = conj(xr[3:7]) (x) y[3:7];   s = (e0 < 0) ? -1 : 1;   theta = 2 s e[1:4]
 *   v     = Kg [theta; dw]
 *   m[c]  = -(1 / rd[c]) (B x v)[c]                 A m^2; a zero field row gives m = 0 by itself
 *   u_cmd = (feedforward ? U_k : 0) + m / o->u_scale
 * Everything after u_cmd, and every argument not named here, is tsat_pd_ensemble's, unchanged in meaning, shape and validation.
 *   Kg 3 x 6 x T   from tsat_aplqr_gains or the caller's own, finite          rd 3 x T   finite and > 0
 * Rejected with -1: everything tsat_pd_ensemble rejects (its kd / kp rules apart); Kg or rd NULL; Kg non-finite; rd non-finite
 * or <= 0. */
int  tsat_aplqr_ensemble(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* Kg, const double* rd, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm);

/* The ensemble controllers fed MEASUREMENTS: every closed loop above commands from the realisation's TRUE state — a perfect
 * attitude solution, a perfect gyro, a perfect magnetometer. The two calls below are tsat_tvlqr_ensemble_gg and tsat_pd_ensemble
 * with the feedback reading a biased, noisy, optionally one-knot-old measurement instead. The reference's noise figures ARE
 * sensor figures — a gyro figure of 0.38 deg and an attitude figure of 1 deg (src/simulator.jl:5,10), which it squares and injects
 * into the dynamics —; read UN-SQUARED, sigma_gyro = 0.38 pi / 180 rad/s and sigma_att = pi / 180 rad are the levels
 * examples/sensed_slew.py flies. No estimator or filter: the law sees the raw measurement.
 *   sigma_gyro  rad/s             sigma_att  rad (rotation vector)             sigma_mag  units of Btab
 *   latency     0: the command of knot k is computed from y_k; 1: from y_max(k-1, 0). The reference record (and U_k) stay knot k's.
 * tsat_sensor_default_options fills the ideal sensor: all zero.
 *   sensor  9 x M x T or NULL (zeros)   per realisation: gyro bias bw (3, rad/s), attitude-sensor bias ba (3, rotation vector,
 *                                       rad, body frame), magnetometer bias bm (3, units of Btab)
 * Knot k of realisation (t, m), true state x, generator id gid, key o->noise_seed. The draw layout documented at
 * tsat_tvlqr_options is used at two stage indices the plant never uses: stage 4 — counters (gid lo, gid hi, k, 16 + j) — gives n_w
 * (its gyro triple, at the sensor's sigma_gyro) and n_a (its attitude triple, at the sensor's sigma_att); stage 5 — counter
 * (..., k, 20) — gives n_m (its gyro triple, at sigma_mag). The measurement y_k:
 *   w_m = x[0:3] + bw + n_w
 *   phi = ba + n_a;  th = |phi|;  dq = [cos(th/2); phi * (th == 0 ? 1/2 : sin(th/2)/th)]
 *   q_m = x[3:7] (x) dq                                    not normalised: the TVLQR feedback uses x[3:7] raw
 *   b_m = qrot(x[3:7] / |x[3:7]|, field row floor(fma(k, dtau, tau0)) clamped) + bm + n_m       the TRUE body field, as a
 *                                                                                                magnetometer reads it
 * TVLQR law:  dX = [w_m - xr[0:3]; vec(conj(xr[3:7]) (x) q_m)],  u_cmd = U_k - K_k dX
 * PD law:     dw, e and the sign rule from (w_m, q_m), b = b_m, m = 0 where b_m . b_m == 0
 * Everything after u_cmd is the parent's: the limit rule, G u_sat + m_res / u_scale held over four stages, the plant draws of
 * stages 0..3 and their injection, the gravity-gradient term, the table clock, the statistic evaluated on the TRUE state, X_sim
 * (true states), n_clipped, summary, ragged n_knots, zero fill. stats_nominal flies the noise-free model plant with the IDEAL
 * sensor (no draws, zero biases) at the call's latency. With sensor NULL or zero, zero sigmas and latency 0 the measurement is the
 * state (x + 0 + 0 z, x (x) (1,0,0,0) and b + 0 + 0 z are exact) and the calls repeat their parents.
 * tsat_tvlqr_ensemble_sensed also allows plant == NULL (every realisation flies the model's plant) and Rtab == NULL with gm == 0
 * (the kernel without the gravity rows), as tsat_pd_ensemble does.
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): s NULL; a sigma non-finite or
 * negative; latency not 0 or 1; a non-finite sensor entry (the text carries (t, m)); and everything the parent rejects. */
struct tsat_sensor_options {
  double  sigma_gyro;
  double  sigma_att;
  double  sigma_mag;
  int32_t latency;
  int32_t reserved;         /* 0 */
};
typedef struct tsat_sensor_options tsat_sensor_options;
#define TSAT_SENSOR_W 9
void tsat_sensor_default_options(tsat_sensor_options* s);
int  tsat_tvlqr_ensemble_sensed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor);
int  tsat_pd_ensemble_sensed(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor);

/* A multiplicative EKF between sensor and law: the two sensed calls above with the standard six-state filter — attitude error
 * plus gyro bias, propagated by the gyro, updated by the attitude measurement — between the measurement and the command. It
 * removes attitude-sensor noise and estimates the gyro bias. It does NOT smooth white gyro noise: the rate the law sees is
 * w_m - b^, one gyro sample less the bias estimate (a numpy run of the recursion at dt = 0.2 s, sigma_gyro = 0.38 deg/s,
 * sigma_att = 1 deg, a 2e-3 rad/s bias, 400 knots: attitude error 1.74 deg raw, 0.48 deg filtered; gyro-bias error 3.5e-3 against
 * 0.7e-3 rad/s; rate error 1.20e-2 against 1.15e-2 rad/s).
 * Options (launch-uniform, all standard deviations):
 *   sigma_v   gyro white noise the filter assumes (rad/s)          sigma_u   bias random walk per knot (rad/s)
 *   sigma_a   attitude measurement noise it assumes (rad), > 0     p0_att    initial attitude standard deviation (rad)
 *   p0_bias   initial bias standard deviation (rad/s)              reserved  0
 * tsat_filter_default_options fills the reference's figures: sigma_v = 0.38 pi / 180, sigma_a = p0_att = pi / 180, the rest 0.
 * State per realisation: q^ (4, unit, scalar first), b^ (3), w^ (3) and the 6 x 6 covariance as blocks A (theta theta),
 * B (theta b), D (b b). h is dt[t]; dq(.) is the rotation-vector quaternion of the measurement above, including its th == 0
 * select; (x) is the quaternion product in the operand order of q_m = x[3:7] (x) dq. The filter runs over the samples
 * m_j = (w_m, q_m) of the measurement above, j = 0, 1, ...
 *   First sample m_0:  q^ = q_m / |q_m|, b^ = 0, w^ = w_m;  A = p0_att^2 I, B = 0, D = p0_bias^2 I.
 *   Step on sample m_j, j >= 1:
 *     1. phi = h w^, d = dq(phi), q- = q^ (x) d;  C = I + 2 d0 [v]x + 2 [v]x^2 with v = d[1:4];  Phi = C^T
 *     2. A- = Phi A Phi^T - h (Phi B + (Phi B)^T) + h^2 D + (sigma_v h)^2 I;  B- = Phi B - h D;  D- = D + sigma_u^2 I
 *     3. e = conj(q-) (x) (q_m / |q_m|);  s = (e0 < 0 ? -1 : 1);  z = 2 s e[1:4]
 *     4. S = A- + sigma_a^2 I, 3 x 3 and positive definite;  Ktheta = A- S^-1, Kb = B-^T S^-1;  dtheta = Ktheta z, db = Kb z
 *     5. q^ = (q- (x) [1; dtheta / 2]), normalised;  b^ <- b^ + db;  w^ = w_m - b^
 *     6. P <- P- - K S K^T by blocks (the upper triangles of A and D only: P is symmetric by construction)
 *   What the law sees at knot k — latency 0: the filter is at sample k, y_k = (w^_k, q^_k). Latency 1: y_0 = (w^_0, q^_0), the
 *   first knot sees its own sample; for k >= 1 the filter is at sample k - 1 and y_k = (w^_{k-1}, q^_{k-1} (x) dq(h w^_{k-1})),
 *   the estimate predicted across the delay (its attitude is step 1's q- of the next step). The measurement at latency 1 hands
 *   m_0 over twice, at k = 0 and at k = 1; the second hand-over makes no step.
 * The PD law's magnetometer reading b_m is not filtered. stats_nominal flies the ideal sensor through the same filter: it differs
 * from the sensed call's, because gyro propagation is not the plant's RK4. Everything after y_k is the sensed call's.
 *   X_hat       7 x N x M x T or NULL   row k holds y_k for k < n_knots[t] - 1, the rest is zero (the layout of X_sim)
 *   filt_final  9 x M x T or NULL       b^ (3), sqrt(diag A) (3), sqrt(diag D) (3) after the last sample processed
 * f == NULL is the sensed call, byte for byte (it is dispatched there); X_hat and filt_final must then be NULL.
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): a non-finite or negative
 * option; sigma_a == 0; reserved != 0; f NULL with X_hat or filt_final non-NULL; and everything the sensed call rejects. */
struct tsat_filter_options {
  double  sigma_v;
  double  sigma_u;
  double  sigma_a;
  double  p0_att;
  double  p0_bias;
  int32_t reserved;         /* 0 */
};
typedef struct tsat_filter_options tsat_filter_options;
#define TSAT_FILTER_W 9
void tsat_filter_default_options(tsat_filter_options* f);
int  tsat_tvlqr_ensemble_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_filter_options* f, double* X_hat, double* filt_final);
int  tsat_pd_ensemble_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_filter_options* f, double* X_hat, double* filt_final);

/* A MODEL-BASED rate filter between sensor and law: the two sensed calls with a nine-state multiplicative EKF that uses what the
 * flight software knows — the model inertia, the field table and the command it has just issued. It carries the body rate as a
 * state and takes the gyro as a measurement of it, so (unlike the six-state filter above) it smooths white gyro noise, down to
 * what sigma_w — the un-modelled angular acceleration it assumes — allows.
 * Options (launch-uniform, all standard deviations):
 *   sigma_v   attitude process noise (rad/s)                        sigma_w   un-modelled angular acceleration (rad/s^2)
 *   sigma_u   bias random walk per knot (rad/s)                     sigma_a   attitude measurement noise it assumes (rad), > 0
 *   sigma_g   gyro measurement noise it assumes (rad/s), > 0        p0_att    initial attitude standard deviation (rad)
 *   p0_bias   initial bias standard deviation (rad/s)               reserved  0
 * tsat_model_filter_default_options fills the reference's figures: sigma_g = 0.38 pi / 180, sigma_a = p0_att = pi / 180, the rest
 * 0 — sigma_w included: no default for it can be derived, a caller has to choose it.
 * State per realisation: q^ (4, unit, scalar first), w^ (3), b^ (3). Error state (dtheta, dw, db) in the body frame:
 * q_true = q^ (x) dq(dtheta), dw = w - w^, db = b - b^. P is 9 x 9 symmetric with blocks theta, w, b, kept as its upper triangle
 * (45 values). h, dq(.), (x), C(.) and the 3 x 3 inverse by cofactors with one reciprocal are those of the six-state filter.
 *   first(m_0):  q^ = q_m / |q_m|, w^ = w_m, b^ = 0;  P_tt = p0_att^2 I, P_bb = p0_bias^2 I, P_ww = (sigma_g^2 + p0_bias^2) I,
 *     P_wb = -p0_bias^2 I, P_tw = P_tb = 0 (the consistent start, since w - w_m = -(n + b)).
 *   predict(u):  u is the command of the knot being crossed as the law issued it: after the limit rule, before the plant's actuator
 *     matrix and residual dipole. Mean: (w-, q-) is one step from (w^, q^) of the plant's integrator on the MODEL — four stages
 *     h dyn7(., u, b_c, J_model, u_scale) with the knot's field rows at c = 0, 1/2, 1/2, 1, combined as the roll-out combines them;
 *     no noise, no disturbance torque, G = I, m_res = 0 (what the noise-free realisation of a dispersed call flies); q- is
 *     normalised, b- = b^. Covariance: P- = Phi P Phi^T + Q with Phi_tt = C(h w^)^T, Phi_tw = h I,
 *     Phi_ww = I + h J^-1 ([J w^]x - [w^]x J), Phi_bb = I, every other block 0 (the dependence of the magnetic torque on dtheta is
 *     neglected in Phi and kept in the mean); Q = diag((sigma_v h)^2 I, (sigma_w h)^2 I, sigma_u^2 I).
 *   update(m):  two 3-vector updates in this order, each applying its whole 9-vector delta = K z:
 *     a. attitude  e = conj(q-) (x) q_m / |q_m|, z = 2 s e[1:4] with s = (e0 < 0 ? -1 : 1);  S = P_tt + sigma_a^2 I;
 *                  K = P[:, theta] S^-1
 *     b. gyro      z = w_m - (w^ + b^);  S = P_ww + P_wb + P_wb^T + P_bb + sigma_g^2 I;  K = (P[:, w] + P[:, b]) S^-1
 *     both: q^ <- normalise(q^ (x) [1; dtheta / 2]), w^ += dw, b^ += db;  P <- P - K S K^T.
 *   What the law sees at knot k, the measurement delivering m_k at latency 0 and m_max(k-1,0) at latency 1 — latency 0: k = 0
 *   first; k >= 1 predict(u_{k-1}) with the rows of knot k - 1, then update(m_k); y_k = (w^, q^). Latency 1: y_0 from first(m_0);
 *   k = 1: m_0 arrives a second time and makes no update, then predict(u_0); k >= 2: update(m_{k-1}) on the prior made at knot
 *   k - 1, then predict(u_{k-1}); for k >= 1, y_k = (w-, q-): the model prediction across the delay, rate included.
 * The PD law's magnetometer reading b_m is not filtered. stats_nominal flies the ideal sensor through the same filter. The
 * gravity-gradient torque is not in the filter's model: it is un-modelled torque that sigma_w has to cover.
 *   X_hat       7 x N x M x T or NULL   row k holds y_k for k < n_knots[t] - 1, the rest is zero (the layout of X_sim)
 *   filt_final  12 x M x T or NULL      b^ (3), sqrt(diag P_tt) (3), sqrt(diag P_ww) (3), sqrt(diag P_bb) (3), taken directly after
 *                                       the last update made up to and including the call at k = n_knots[t] - 2; the record of
 *                                       first when none was made
 * f == NULL is the sensed call, byte for byte (it is dispatched there); X_hat and filt_final must then be NULL.
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): a non-finite or negative
 * option; sigma_a == 0; sigma_g == 0; reserved != 0; f NULL with X_hat or filt_final non-NULL; and everything the sensed call
 * rejects. */
struct tsat_model_filter_options {
  double  sigma_v;
  double  sigma_w;
  double  sigma_u;
  double  sigma_a;
  double  sigma_g;
  double  p0_att;
  double  p0_bias;
  int32_t reserved;         /* 0 */
};
typedef struct tsat_model_filter_options tsat_model_filter_options;
#define TSAT_MODEL_FILTER_W 12
void tsat_model_filter_default_options(tsat_model_filter_options* f);
int  tsat_tvlqr_ensemble_model_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_model_filter_options* f, double* X_hat, double* filt_final);
int  tsat_pd_ensemble_model_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_model_filter_options* f, double* X_hat, double* filt_final);

/* A MAGNETOMETER-UPDATED attitude filter between sensor and law: the two filtered calls (tsat_filter_options above) with the
 * attitude update replaced by a magnetometer update. The reference's satellite carries a gyro and a magnetometer and no sensor
 * that hands over a quaternion: this filter takes ONE attitude fix, the first sample's q_m, and from then on corrects the
 * gyro-propagated attitude by the measured body field b_m against the slew's own field table. One field vector fixes two of the
 * three angles; the third comes from the field turning along the orbit, so the estimate is far coarser than the six-state
 * filter's (the reference loop of tests/mag_filtered_common.py, 400 knots at dt = 0.2 s, sigma_mag = 5e-7 T on a 2.5e-5 T field,
 * a 2e-3 rad/s gyro bias: rms attitude error over the last half 3.0 deg against 7.1 deg for gyro dead reckoning from the same fix).
 * Options (launch-uniform, all standard deviations):
 *   sigma_v   gyro white noise the filter assumes (rad/s)          sigma_u   bias random walk per knot (rad/s)
 *   sigma_m   magnetometer noise it assumes, in units of Btab, > 0 p0_att    initial attitude standard deviation (rad)
 *   p0_bias   initial bias standard deviation (rad/s)              reserved  0
 * tsat_mag_filter_default_options fills the six-state filter's figures — sigma_v = 0.38 pi / 180, p0_att = pi / 180, the rest 0 —
 * and LEAVES sigma_m 0, which the calls reject: it is in the units of the caller's table and has no default.
 * State per realisation: the six-state filter's — q^, b^, w^ and A, B, D — in the same 31-value record. h, dq(.), (x) and the
 * 3 x 3 inverse by cofactors are those of the six-state filter. The filter runs over the samples m_j = (w_m, q_m, b_m) of the
 * measurement of the sensed calls, j = 0, 1, ...; r_j is the stage-0 field row of knot j, the row b_m of knot j was formed with.
 *   First sample m_0:  q^ = q_m / |q_m|, b^ = 0, w^ = w_m;  A = p0_att^2 I, B = 0, D = p0_bias^2 I. This is the one attitude fix,
 *     at acquisition: q_m of every later sample is ignored. No magnetometer update is made at the first sample.
 *   Step on sample m_j, j >= 1:
 *     1. phi = h w^, d = dq(phi), q- = q^ (x) d;  C = I + 2 d0 [v]x + 2 [v]x^2 with v = d[1:4];  Phi = C^T
 *     2. A- = Phi A Phi^T - h (Phi B + (Phi B)^T) + h^2 D + (sigma_v h)^2 I;  B- = Phi B - h D;  D- = D + sigma_u^2 I
 *     3. n = q- / |q-|;  b^ = qrot(n, r_j), as the true body field is formed;  z = b_m - b^;
 *        H = -C(n) [r_j]x with C(n) = I + 2 n0 [v]x + 2 [v]x^2, v = n[1:4], the matrix for which qrot(n, v) = C(n) v
 *        (equivalently H = -[b^]x C(n)): the derivative of qrot(q- (x) [1; dtheta / 2], r_j) in dtheta at 0
 *     4. G = A- H^T, Gb = B-^T H^T;  S = H G + sigma_m^2 I, 3 x 3 (its upper triangle, mirrored) and positive definite because
 *        sigma_m > 0;  Ktheta = G S^-1, Kb = Gb S^-1;  dtheta = Ktheta z, db = Kb z
 *     5. q^ = (q- (x) [1; dtheta / 2]), normalised;  b^ <- b^ + db;  w^ = w_m - b^
 *     6. P <- P- - K S K^T by blocks (the upper triangles of A and D only)
 *   A zero field row gives H = 0 and K = 0, an update that changes nothing, without a branch (the last row of a
 *   magnetic_simulation table is such a row). Nothing asks whether a sigma is zero.
 *   What the law sees at knot k is the six-state filter's rule word for word — latency 0: the filter is at sample k. Latency 1:
 *   y_0 from the first sample; m_0 is handed over twice and makes no step the second time; for k >= 1 the filter is at sample
 *   k - 1 and the estimate is predicted across the delay by q^ (x) dq(h w^). The sample that arrives at knot k at latency 1 is
 *   knot k - 1's: it is updated against row r_{k-1}, not r_k.
 * The magnetometer is sampled ONCE per knot: the PD law's b_m is the very reading the filter used (not filtered). Under the TVLQR
 * law the reading is drawn too (the sensed and filtered TVLQR calls draw none). stats_nominal flies the ideal sensor through the
 * same filter. The magnetometer bias of `sensor` is not estimated: it enters z unmodelled.
 *   X_hat       7 x N x M x T or NULL   row k holds y_k for k < n_knots[t] - 1, the rest is zero (the layout of X_sim)
 *   filt_final  9 x M x T or NULL       b^ (3), sqrt(diag A) (3), sqrt(diag D) (3) after the last sample processed (TSAT_FILTER_W)
 * f == NULL is the sensed call, byte for byte (it is dispatched there); X_hat and filt_final must then be NULL.
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): a non-finite or negative
 * option; sigma_m == 0; reserved != 0; f NULL with X_hat or filt_final non-NULL; and everything the sensed call rejects. */
struct tsat_mag_filter_options {
  double  sigma_v;
  double  sigma_u;
  double  sigma_m;
  double  p0_att;
  double  p0_bias;
  int32_t reserved;         /* 0 */
};
typedef struct tsat_mag_filter_options tsat_mag_filter_options;
void tsat_mag_filter_default_options(tsat_mag_filter_options* f);
int  tsat_tvlqr_ensemble_mag_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_mag_filter_options* f, double* X_hat, double* filt_final);
int  tsat_pd_ensemble_mag_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_mag_filter_options* f, double* X_hat, double* filt_final);

/* The magnetometer-updated filter WITH THE MAGNETOMETER BIAS AS A STATE: the two mag-filtered calls (tsat_mag_filter_options above)
 * with a nine-state multiplicative EKF — attitude error theta, gyro bias b, magnetometer bias c — between sensor and law. On a
 * magnetorquer-only satellite the magnetometer sits next to the torquers and a constant bias of several percent of the field is
 * the normal case; the six-state mag filter lets it enter z unmodelled, this one estimates it (the reference loop of
 * tests/mag_bias_filtered_common.py, 400 knots, a 3e-6 T bias on a 2.5e-5 T field: rms attitude error over the last half 3.3 deg
 * against 6.4 deg, |c^ - c| at the end at most 0.28 |c|; the price without a bias at all is 3.0 -> 3.3 deg).
 * Options (launch-uniform, all standard deviations): those of tsat_mag_filter_options and
 *   sigma_c   magnetometer-bias random walk per knot              p0_mag    initial magnetometer-bias standard deviation
 * both in the units of the caller's field table, both >= 0. tsat_mag_bias_filter_default_options fills the figures of
 * tsat_mag_filter_default_options, sigma_c = p0_mag = 0, and LEAVES sigma_m 0, which the calls reject.
 * State per realisation, 58 values: q^ 4, b^ 3, w^ 3, c^ 3, and the covariance as 45 values in blocks — the upper triangles of
 * A (theta theta), D (b b), M (c c) and, row-major 3 x 3, B (theta b), E (theta c), F (b c). Samples m_j = (w_m, q_m, b_m), rows
 * r_j, h, dq(.), (x), the 3 x 3 inverse by cofactors and the latency rule are the mag filter's, word for word.
 *   First sample m_0:  as the mag filter — q^ = q_m / |q_m|, b^ = 0, w^ = w_m;  A = p0_att^2 I, B = 0, D = p0_bias^2 I — and
 *     c^ = 0, M = p0_mag^2 I, E = F = 0. No magnetometer update is made at the first sample.
 *   Step on sample m_j, j >= 1:
 *     1. q- and Phi as the mag filter
 *     2. A-, B-, D- as the mag filter;  E- = Phi E - h F;  F- = F;  M- = M + sigma_c^2 I
 *     3. n = q- / |q-|;  b^f = qrot(n, r_j);  z = b_m - c^ - b^f;  H = -C(n) [r_j]x;  the measurement matrix is [H 0 I]
 *     4. Gtheta = A- H^T + E-;  Gb = B-^T H^T + F-;  Gc = E-^T H^T + M-;  S = H Gtheta + Gc + sigma_m^2 I, 3 x 3 (its upper
 *        triangle, mirrored) and positive definite because sigma_m > 0;  K. = G. S^-1 for each of theta, b and c;
 *        dtheta, db, dc = K. z
 *     5. q^, b^ and w^ as the mag filter;  c^ <- c^ + dc
 *     6. P <- P- - K S K^T by blocks, with W. = K. S: the upper triangles of A, D and M;  B -= Wtheta Kb^T;  E -= Wtheta Kc^T;
 *        F -= Wb Kc^T
 *   A ZERO FIELD ROW IS NO LONGER A NO-OP: H = 0 leaves z = b_m - c^ observing c directly. That is correct — the plant's field is
 *   zero there too, so the reading is bias and noise alone (the last row of a magnetic_simulation table is such a row). Nothing
 *   asks whether a sigma is zero; with p0_mag = sigma_c = 0 the blocks E, F, M and c^ stay zero and the recursion is the mag
 *   filter's.
 *   What the law sees is (w^, q^) by the mag filter's rule, the prediction across the delay and r_{k-1} for the delayed sample
 *   included. The magnetometer is sampled ONCE per knot; the PD law's b_m is the raw reading the filter used, NOT corrected by c^.
 *   X_hat       7 x N x M x T or NULL   as the mag-filtered calls'
 *   filt_final  15 x M x T or NULL      b^ (3), sqrt(diag A) (3), sqrt(diag D) (3), c^ (3), sqrt(diag M) (3) after the last sample
 *                                       processed (TSAT_MAG_BIAS_FILTER_W)
 * f == NULL is the sensed call, byte for byte (it is dispatched there); X_hat and filt_final must then be NULL.
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): a non-finite or negative
 * option; sigma_m == 0; reserved != 0; f NULL with X_hat or filt_final non-NULL; and everything the sensed call rejects. */
#define TSAT_MAG_BIAS_FILTER_W 15
struct tsat_mag_bias_filter_options {
  double  sigma_v;
  double  sigma_u;
  double  sigma_m;
  double  sigma_c;
  double  p0_att;
  double  p0_bias;
  double  p0_mag;
  int32_t reserved;         /* 0 */
};
typedef struct tsat_mag_bias_filter_options tsat_mag_bias_filter_options;
void tsat_mag_bias_filter_default_options(tsat_mag_bias_filter_options* f);
int  tsat_tvlqr_ensemble_mag_bias_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_mag_bias_filter_options* f, double* X_hat, double* filt_final);
int  tsat_pd_ensemble_mag_bias_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_mag_bias_filter_options* f, double* X_hat, double* filt_final);

/* The MODEL-BASED rate filter UPDATED BY THE MAGNETOMETER: the two model-filtered calls (tsat_model_filter_options above) with
 * update a. (attitude) replaced by the magnetometer update of the mag-filtered calls. It is the filter a magnetorquer-only satellite
 * can fly — a gyro, a magnetometer and ONE attitude fix at acquisition — and it still smooths the gyro: the law reads a rate that
 * was propagated on the model, not w_m - b^ (the reference loop of tests/model_mag_filtered_common.py, 400 knots at dt = 0.2 s,
 * 0.38 deg/s gyro noise, 5e-7 T magnetometer noise, a 2e-3 rad/s gyro bias: rms rate error over the last half 9.2e-4 rad/s against
 * the raw sample's 1.17e-2, rms attitude error 2.8 deg against the mag filter's 3.0 deg).
 * Options (launch-uniform, all standard deviations): sigma_v, sigma_w, sigma_u, sigma_g, p0_att, p0_bias of tsat_model_filter_options
 * and
 *   sigma_m   magnetometer noise the filter assumes, in units of Btab, > 0
 * tsat_model_mag_filter_default_options fills sigma_g = 0.38 pi / 180, p0_att = pi / 180 and the rest 0. sigma_w and sigma_m have
 * no default: sigma_w is the caller's choice, sigma_m is in the units of the caller's table and is rejected at 0.
 * State per realisation: the model filter's, in the same 58-value record (TSAT_MODEL_FILTER_STATE_W) — q^ 4, w^ 3, b^ 3, the last
 * command 3, and P over (dtheta, dw, db) as the upper triangles of A (theta theta), W (w w), D (b b) and, row-major 3 x 3,
 * X (theta w), B (theta b), Y (w b). The recursion of tsat_model_filter_options applies unchanged except as stated here. The filter
 * runs over the samples m_j = (w_m, q_m, b_m) of the measurement of the sensed calls; r_j is the stage-0 field row of knot j, the
 * row b_m of knot j was formed with.
 *   first(m_0):  the model filter's: the one attitude fix comes from q_m of sample 0, w^ = w_m, the consistent start with the
 *     -p0_bias^2 cross block included. q_m of every later sample is ignored. No magnetometer update is made at sample 0.
 *   predict(u):  the model filter's, with the rows of the knot being crossed.
 *   update(m_j), j >= 1:  two 3-vector updates in this order, each applying its whole 9-vector delta = K z:
 *     a. magnetometer  n = q^ / |q^|;  z = b_m - qrot(n, r_j), as the true body field is formed;  Hm = -C(n) [r_j]x, the mag
 *                      filter's H;  P H^T = [A Hm^T; X^T Hm^T; B^T Hm^T];  S = Hm A Hm^T + sigma_m^2 I (its upper triangle,
 *                      mirrored; positive definite because sigma_m > 0);  K = P H^T S^-1
 *     b. gyro          the model filter's b., operation for operation
 *     both: q^ <- normalise(q^ (x) [1; dtheta / 2]), w^ += dw, b^ += db;  P <- P - K S K^T.
 *   A zero field row gives Hm = 0 and K = 0 in a.: an update that changes nothing, without a branch. Nothing asks whether a sigma
 *   is zero.
 *   What the law sees at knot k is the model filter's rule — latency 0: k = 0 first; k >= 1 predict(u_{k-1}), then update(m_k)
 *   against r_k. Latency 1: y_0 from first(m_0); k = 1: m_0 arrives a second time and makes no update, then predict(u_0); k >= 2:
 *   update(m_{k-1}) against r_{k-1} — the delayed sample's own row, not r_k — then predict(u_{k-1}); for k >= 1, y_k is the model
 *   prediction across the delay, rate included.
 * The magnetometer is sampled ONCE per knot: the PD law's b_m is the very reading the filter used (not filtered). Under the TVLQR
 * law the reading is drawn too (the sensed and model-filtered TVLQR calls draw none). stats_nominal flies the ideal sensor through
 * the same filter. The magnetometer bias of `sensor` is not estimated: it enters z unmodelled.
 *   X_hat       7 x N x M x T or NULL   row k holds y_k for k < n_knots[t] - 1, the rest is zero (the layout of X_sim)
 *   filt_final  12 x M x T or NULL      b^ (3), sqrt(diag A) (3), sqrt(diag W) (3), sqrt(diag D) (3), taken directly after the last
 *                                       update made up to and including the call at k = n_knots[t] - 2; the record of first when
 *                                       none was made (TSAT_MODEL_FILTER_W)
 * f == NULL is the sensed call, byte for byte (it is dispatched there); X_hat and filt_final must then be NULL.
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): a non-finite or negative
 * option; sigma_g == 0; sigma_m == 0; reserved != 0; f NULL with X_hat or filt_final non-NULL; and everything the sensed call
 * rejects. */
struct tsat_model_mag_filter_options {
  double  sigma_v;
  double  sigma_w;
  double  sigma_u;
  double  sigma_g;
  double  sigma_m;
  double  p0_att;
  double  p0_bias;
  int32_t reserved;         /* 0 */
};
typedef struct tsat_model_mag_filter_options tsat_model_mag_filter_options;
void tsat_model_mag_filter_default_options(tsat_model_mag_filter_options* f);
int  tsat_tvlqr_ensemble_model_mag_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_model_mag_filter_options* f, double* X_hat, double* filt_final);
int  tsat_pd_ensemble_model_mag_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_model_mag_filter_options* f, double* X_hat, double* filt_final);

/* The magnetometer-updated model filter WITH A SUN SENSOR THAT ECLIPSE BLINDS: the two model-mag-filtered calls above with a second
 * body vector. One field vector does not observe the rotation about itself; a coarse sun sensor closes that gap while the satellite
 * is lit and hands over nothing in the Earth's shadow (the reference loop of tests/model_mag_sun_filtered_common.py, the 400-knot
 * case of the model-mag filter with a 0.5 deg sun sensor 35 deg from the field: rms attitude error over the last half 0.26 deg lit
 * throughout and 0.66 deg when dark from knot 100 on, against 2.8 deg without the sun sensor).
 * Stab (n_btab x n_tab x 3) is the sun table: the shape and the indexing of Btab — the same btab_idx, the same table clock; the row
 * of knot j is s_j, the stage-0 row of that knot. A row is the sun direction in ECI where the satellite is lit (a unit vector in the
 * intended use; the filter does not normalise it) and EXACTLY (0, 0, 0) where it is in shadow.
 * The sensor: one sun sample per knot, s_m = qrot(x[3:7] / |x[3:7]|, s_k) + sigma_sun n_s, formed as the true body field is; n_s
 * is the gyro triple of stage index 6 of the documented draw layout (Philox counter 24 of (gid, k)). sigma_sun >= 0 is
 * launch-uniform and dimensionless (radians for small angles); it is an argument of the calls because tsat_sensor_options keeps its
 * layout. There is NO per-realisation sun-sensor bias. Where the row is zero nothing is drawn and no sample exists. At latency 1 the
 * delayed sample is paired with its own row s_{k-1}, not s_k. stats_nominal flies the ideal sensor (no draw) through the same filter.
 * Options: those of tsat_model_mag_filter_options and
 *   sigma_s   sun-sensor noise the filter assumes, dimensionless, > 0 when Stab is given; it has no default
 * tsat_model_mag_sun_filter_default_options fills the parent's defaults and sigma_s = 0.
 * The recursion of tsat_model_mag_filter_options applies unchanged — first, predict, the 58-value record, the latency rule —
 * except that update(m_j), j >= 1, is three 3-vector updates in this order, each applying its whole 9-vector delta = K z:
 *     a. magnetometer, b. gyro   the parent's, operation for operation
 *     c. sun, ONLY IF s_j != 0   n = q^ / |q^|;  z = s_m - qrot(n, s_j);  Hs = -C(n) [s_j]x;
 *                                P H^T = [A Hs^T; X^T Hs^T; B^T Hs^T];  S = Hs A Hs^T + sigma_s^2 I (its upper triangle,
 *                                mirrored; positive definite because sigma_s > 0);  K = P H^T S^-1
 *     then q^ <- normalise(q^ (x) [1; dtheta / 2]), w^ += dw, b^ += db;  P <- P - K S K^T, as after a. and b.
 *   A dark knot SKIPS c. by a branch (uniform over the wavefront: the row is read by scalar loads), not by K = 0: the correction
 *   renormalises q^, and a table dark throughout is the model-mag-filtered call bit for bit.
 *   No sun update is made at sample 0 and none at k = 1 of latency 1, as for the magnetometer.
 *   X_hat, filt_final (12, TSAT_MODEL_FILTER_W): the parent's.
 * f == NULL is the sensed call, byte for byte (it is dispatched there); X_hat, filt_final and Stab must then be NULL and sigma_sun 0.
 * Stab == NULL with f given is the model-mag-filtered call on the seven shared options, byte for byte (it is dispatched there);
 * sigma_sun must then be 0 and sigma_s is not looked at.
 * Rejected with -1 (text in tsat_ensemble_last_error; nothing is launched and no workspace grows): a non-finite or negative
 * option; sigma_g == 0; sigma_m == 0; sigma_s == 0 with Stab given; a negative or non-finite sigma_sun; a non-finite Stab entry;
 * reserved != 0; and everything the model-mag-filtered call rejects. The packed sun rows live in a grow-only workspace of the handle
 * (tsat_workspace_bytes counts them, tsat_workspace_trim(h, 1) frees them). */
struct tsat_model_mag_sun_filter_options {
  double  sigma_v;
  double  sigma_w;
  double  sigma_u;
  double  sigma_g;
  double  sigma_m;
  double  sigma_s;
  double  p0_att;
  double  p0_bias;
  int32_t reserved;         /* 0 */
};
typedef struct tsat_model_mag_sun_filter_options tsat_model_mag_sun_filter_options;
void tsat_model_mag_sun_filter_default_options(tsat_model_mag_sun_filter_options* f);
int  tsat_tvlqr_ensemble_model_mag_sun_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat, const double* Qd, const double* Qfd, const double* Rd,
                         const double* x0_sim, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* K_lqr, double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_model_mag_sun_filter_options* f, double* X_hat, double* filt_final,
                         const double* Stab, double sigma_sun);
int  tsat_pd_ensemble_model_mag_sun_filtered(tsat_handle* h, const tsat_tvlqr_options* o, int64_t T, int64_t n_btab, int32_t M,
                         const double* X, const double* U, const double* xf,
                         const double* Btab, const int32_t* btab_idx, const double* tau0, const double* dtau,
                         const double* dt, const double* Jmat,
                         const double* kd, const double* kp, int32_t feedforward, int32_t limit_mode,
                         const double* x0_sim, const double* x0_nom, const int64_t* noise_id0, const int32_t* n_knots,
                         const double* plant, const double* sat_lo, const double* sat_hi,
                         tsat_tvlqr_stats* stats, double* summary, tsat_tvlqr_stats* stats_nominal,
                         double* X_sim, int32_t* n_clipped, const double* Rtab, double gm,
                         const tsat_sensor_options* s, const double* sensor,
                         const tsat_model_mag_sun_filter_options* f, double* X_hat, double* filt_final,
                         const double* Stab, double sigma_sun);

/* ------------------------------------------------------------------------------------------------------------
 * Receding-horizon re-solve on the RESIDENT batch (BASELINE.json configs[4]). NOT in the reference —
 * it tracks its plan with TVLQR (src/attitude_controller.jl:1-48); defined here as: n_steps times
 *   1. solve the horizon from the current x0 with the current initial controls, budget and options of `o`
 *      (exactly tsat_batch_run);
 *   2. record x_t = x0 and u_t = U[0];
 *   3. advance the noise-free plant one step with u_t: rk3 or rk4 (plant_integrator 3 | 4) of the model dynamics
 *      (src/DerivFunction.jl:1-48) over dt, table rows at the current table time;
 *   4. warm start of the next solve = the plan shifted by one knot, last control repeated; tau0 += dtau.
 * Nothing returns to the host between steps. tsat_mpc_run MUTATES the resident batch: afterwards it holds the advanced
 * x0 / tau0, the shifted warm start in place of the uploaded U0, and the last plan (tsat_batch_download); a further call
 * continues the simulation, tsat_batch_run re-solves from the advanced state, and tsat_tvlqr_resident tracks the last plan
 * from the advanced table clock (the handle's host copies of x0 / tau0 are refreshed from the device after the loop).
 *   X_hist 7 x (n_steps+1) x T   states x_0 .. x_{n_steps}
 *   U_hist 3 x n_steps x T       applied controls
 *   stats_last T (may be NULL)   statistics of the last solve
 *   solve_ms (may be NULL)       device time of the whole loop
 * ------------------------------------------------------------------------------------------------------------ */
int  tsat_mpc_run(tsat_handle* h, const tsat_options* o, int32_t n_steps, int32_t plant_integrator,
                  double* X_hist, double* U_hist, tsat_stats* stats_last, float* solve_ms);
/* executed counts of the last tsat_mpc_run, summed over its control steps on the device: per trajectory
 * [backward sweeps, forward sweeps, AL dual updates (outer_iters - 1), inner iterations]  (4 x T, int64) — what a measurement
 * needs to price the loop's memory traffic without bringing per-step statistics to the host */
int  tsat_mpc_tally(tsat_handle* h, int64_t* tally /* 4 x T */);

/* The same receding-horizon loop on a NOISY, DISPERSED plant with limits: the plant of one realisation of
 * tsat_tvlqr_ensemble_dispersed per trajectory, re-planned against instead of tracked with fixed gains. Steps 1 and 4 are those of
 * tsat_mpc_run (the solver keeps the MODEL inertia of the uploaded batch; the gains play no part); per control step s
 *   2. u_cmd = U[0], u_sat = min(max(u_cmd, sat_lo[t]), sat_hi[t]) component-wise — a step counts as clipped when any component
 *      changed; x_t goes to X_hist, u_sat to U_hist;
 *   3. the plant advances over dt by RK4 (the noise layout is per RK4 stage: no integrator argument) of the model dynamics with
 *      inertia Jp[t] and dipole G[t] u_sat + m_res[t] / u_scale, field rows floor(fma(c, dtau, tau0)), c = 0, 1/2, 1, clamped;
 *      with po->noise_mode = 1 the nine draws of (generator id noise_id[t], knot step0 + s, stage) enter every stage's state and
 *      field row exactly as in the ensemble roll-out (draw layout at tsat_tvlqr_options); noise_mode = 0 is the noise-free plant;
 *   5. the slew-time statistic of tsat_tvlqr_stats on the history, evaluated while the loop runs: sample j (1-based) is x_{j-1},
 *      n_steps + 1 samples, slew_index = first j > po->min_steps with |w| < w_tol and error angle to the resident xf < angle_tol,
 *      slew_time = dt * index (dt * (n_steps + 1) on failure), final_* from x_{n_steps}.
 *   plant      21 x T (TSAT_PLANT_W: Jp 9, G 9, m_res 3, as tsat_tvlqr_ensemble_dispersed) or NULL = the model's plant
 *              (Jmat as the symmetric tensor of its upper triangle, G = I, m_res = 0)
 *   sat_lo, sat_hi   3 x T each, units of u_scale; both NULL = unlimited
 *   noise_id   T or NULL (= t)
 *   step0      knot of the first control step for the noise draws: a second call with step0 = the steps already made continues
 *              the simulation as tsat_mpc_run does and draws the noise of the later steps; its statistic counts its own samples
 *   X_hist, U_hist, stats_last, solve_ms   as tsat_mpc_run;  stats T out (may be NULL), n_clipped T out (may be NULL)
 * Of `po` n_knots, n_tab and linearize_dt_sq are ignored. Rejected with -1 (text in tsat_last_error): rate_as_written != 0,
 * noise_mode not 0 or 1, a non-finite plant entry, Jp not symmetric or not positive definite (the checks of
 * tsat_tvlqr_ensemble_dispersed), exactly one limit array NULL, sat_lo > sat_hi, n_steps < 1, step0 < 0 or step0 + n_steps
 * beyond the 32-bit knot counter of the generator, precision != 64, and everything tsat_mpc_run rejects. Afterwards the resident
 * batch is in the state tsat_mpc_run leaves (advanced x0 / tau0 with the host copies refreshed, shifted warm start, last plan,
 * tsat_mpc_tally). */
int  tsat_mpc_run_dispersed(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                            const double* plant, const double* sat_lo, const double* sat_hi, const int64_t* noise_id,
                            double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats, int32_t* n_clipped,
                            float* solve_ms);

/* tsat_mpc_run_dispersed that RE-PLANS EVERY replan_every = R CONTROL STEPS and flies the solver's own gains in between: the
 * controller between TVLQR tracking of one stale plan and a re-solve at every step. Arguments, plant, noise draw layout,
 * statistic and the state left in the resident batch are those of tsat_mpc_run_dispersed; the control steps are grouped into
 * blocks. Block b starts at step s_b = b R and has r = min(R, n_steps - s_b) steps:
 *   1. solve the horizon from the current x0, warm start and tau0 (exactly tsat_batch_run): plan X_j, U_j and gains K_j as
 *      tsat_batch_download returns them;
 *   2. for j = 0 .. r-1, control step s = s_b + j: sample s + 1 (the current state x) is judged; the command is
 *        j = 0:                 u_cmd = U_0 (no gain product is evaluated)
 *        j > 0, feedback = 1:   u_cmd[a] = U_j[a] + sum_{i < nh} K_j[a][i] dx[i], the sum started from U_j[a], i ascending, with the
 *                               solver's own state difference dx: x - X_j, nh = 7 (error_state = 0), or [dw; v / (1 + s)] of
 *                               conj(q_j) (x) q, nh = 6 (error_state = 1) — the policy of the solver's forward sweep at alpha = 0
 *        j > 0, feedback = 0:   u_cmd = U_j, the open-loop hold
 *      clipped to sat_lo / sat_hi (counted, x to X_hist, the limited command to U_hist), then one RK4 step of the dispersed plant
 *      with the draws of (generator id, knot step0 + s, stage). The table clock of a step is the one the every-step loop has there:
 *      rows floor(fma(c, dtau, tau)), c = 0, 1/2, 1, clamped, then tau <- tau + dtau — one rounded addition per step, so for a
 *      given state and command the plant step is the same function of s for every R;
 *   3. warm start of the next solve: U0[k] = U[min(k + r, n_t - 2)] inside each trajectory's own horizon n_t; x0 and tau0 as
 *      advanced by the r steps.
 * The last step of the call writes `stats` and `n_clipped`; tsat_mpc_tally afterwards holds the sums over the ceil(n_steps / R)
 * solves that ran. replan_every = 1 reproduces tsat_mpc_run_dispersed bit for bit for either value of feedback. A call always
 * begins with a solve: a continuation (step0 = the steps already made, no new upload) equals one longer run only when the first
 * call's n_steps is a multiple of R.
 * Rejected with -1 (text in tsat_last_error): replan_every < 1, replan_every > min_t n_knots[t] - 1 (gains exist for n_t - 1 knots
 * only), feedback not 0 or 1, and everything tsat_mpc_run_dispersed rejects.
 * UNSPECIFIED: the held commands (j > 0, feedback = 1) of a trajectory whose block solve ended TSAT_REG_FAIL or TSAT_DIVERGED — its
 * K is undefined (tsat_batch_download); reading it is harmless. */
int  tsat_mpc_run_held(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                       int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                       const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                       int32_t* n_clipped, float* solve_ms);

/* tsat_mpc_run_held with the gravity-gradient torque of tsat_tvlqr_ensemble_gg in every plant step (all four RK4 stages, the rows
 * of the step's table clock, Jp of the trajectory's plant — the model's inertia when `plant` is NULL). The solve does not see the
 * term: the question is whether re-planning survives it. Rtab is 3 x n_tab x n_btab of the RESIDENT batch (its btab_idx), gm as
 * above; replan_every = 1 is the every-step loop under gravity gradient. gm = 0 reproduces tsat_mpc_run_held bit for bit (through
 * the same kernel as any other gm). The packed rows share the handle's workspace with tsat_tvlqr_ensemble_gg.
 * Rejected with -1 (text in tsat_last_error): Rtab NULL, a non-finite entry of Rtab, a row with |r| = 0, gm non-finite or negative,
 * and everything tsat_mpc_run_held rejects. */
int  tsat_mpc_run_held_gg(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                       int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                       const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                       int32_t* n_clipped, float* solve_ms, const double* Rtab, double gm);

/* tsat_mpc_run_held / tsat_mpc_run_held_gg FED MEASUREMENTS: the two places at which the held loop reads the plant's state — the
 * x0 the solve of a block starts from, and the state the held steps' U_j + K_j dx is evaluated on — read the sensor of the sensed
 * ensembles (tsat_sensor_options above) instead. The true state and the state the solver is given become two different things.
 * Everything not named here is the parent's, operation for operation: blocks, the j = 0 rule, the clip, the dispersed RK4 plant
 * step with the draws of stages 0..3, the table clock, the shift, n_clipped, tsat_mpc_tally, and the statistic, which is evaluated
 * on the TRUE state. s: control step RELATIVE TO THE CALL, kappa = step0 + s the generator's knot, x_s the true state:
 *   m_s = (w_m, q_m) of x_s      the raw measurement of the sensed ensembles, word for word (w_m = x[0:3] + bw + n_w,
 *                                q_m = x[3:7] (x) dq(ba + n_a), the th == 0 select); n_w, n_a from stage index 4 — counters 16, 17 —
 *                                of (generator id, kappa) at s->sigma_gyro / s->sigma_att, key po->noise_seed, drawn only when
 *                                po->noise_mode == 1 (biases apply either way)
 *   y_s = m_s (latency 0), m_max(s-1, 0) (latency 1): the first step of a call sees its own measurement
 *   block at s_b: the solve starts from x0 := y_{s_b} (warm start and tau0 as the parent); step j = 0 applies U_0; step j > 0 with
 *                 feedback applies U_j + K_j dx, dx the solver's own state difference between y_s and X_j; without, U_j
 *   the plant advances the TRUE state: X_hist holds true states, Y_hist[s] = y_s, what that step's command or solve used
 * The loop has no law that reads the field: sigma_mag and bm (sensor rows 6..8) are validated and nothing reads them; no stage-5
 * block is generated.
 *   Rtab, gm   as tsat_mpc_run_held_gg; Rtab NULL is allowed iff gm == 0: the kernel without the gravity rows
 *   sensor     9 x T or NULL (zeros): bw, ba, bm of each trajectory (TSAT_SENSOR_W)
 *   Y_hist     7 x n_steps x T out, may be NULL
 * While the call runs the resident x0 carries measurements; the true state lives in a workspace of the handle. The last block
 * writes the TRUE x_{n_steps} back (host copies refreshed), so afterwards the resident batch is in the state tsat_mpc_run_held
 * leaves: tsat_tvlqr_resident, tsat_batch_run and a continuation keep their meaning. A continuation (step0 = the steps made, no
 * upload) equals one longer run when the first call's n_steps is a multiple of R AND latency = 0: latency 1 RESTARTS ITS MEMORY
 * with every call (the first step of the second call sees its own measurement, where the longer run sees the step before).
 * With sensor NULL or zero, zero sigmas and latency 0 the call repeats tsat_mpc_run_held (Rtab NULL) or tsat_mpc_run_held_gg:
 * x + 0 + 0 z and x (x) (1,0,0,0) are exact, as argued for the ensembles.
 * Rejected with -1 (text in tsat_last_error; nothing is launched and no workspace grows): everything the sensed ensembles reject of
 * s and sensor (M = 1: the text of a non-finite entry carries (t, 0)); Rtab NULL with gm != 0; and everything the parents reject. */
int  tsat_mpc_run_held_sensed(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                       int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                       const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                       int32_t* n_clipped, float* solve_ms, const double* Rtab, double gm,
                       const tsat_sensor_options* s, const double* sensor, double* Y_hist);

/* tsat_mpc_run_held_sensed BEHIND THE FILTER of tsat_tvlqr_ensemble_filtered: the loop above with one change — what the controller
 * is handed. The raw measurements m_s are the parent's (stage-4 draws at knot step0 + s, biases from `sensor`, the first step of a
 * call measures itself), and so are the blocks and the j = 0 rule, the clip, the dispersed RK4 step, the gravity rows (Rtab NULL
 * iff gm == 0), the table clock, the shift, n_clipped, tsat_mpc_tally, the statistic on the TRUE state and the true state written
 * back at the end of the call. The recursion written out at tsat_filter_options (`first`, `step` 1-6, the prediction across the
 * delay, h = dt[t]) runs over the samples m_0, m_1, ..., one per control step; the solve's x0 at a block start, the state
 * U_j + K_j dx acts on, and Y_hist[s] all read the filter's y_s. s is the step RELATIVE TO THE CALL, whatever step0 is:
 *   latency 0: the filter is at sample s, y_s = (w^_s, q^_s)
 *   latency 1: y_0 = (w^_0, q^_0); at s = 1 the sensor hands m_0 over a second time, which makes no filter step; for s >= 1 the
 *              filter is at sample s - 1 and y_s = (w^_{s-1}, q^_{s-1} (x) dq(h w^_{s-1})), predicted across the delay
 * State between calls: one flat record of TSAT_FILTER_STATE_W = 31 values per trajectory, q^ 4, b^ 3, w^ 3, then A 6, B 9, D 6
 * (A and D as upper triangles 00 01 02 11 12 22, B row-major).
 *   filt_init   31 x T or NULL   NULL: the filter starts on the call's m_0 (`first`) and so restarts with every call, as the
 *                                latency memory does. Given: the record of trajectory t is loaded before the first sample, and m_0
 *                                makes a `step` instead of `first`; nothing else differs
 *   filt_state  31 x T out or NULL   the record after the last sample processed
 *   filt_final  9 x T out or NULL    b^, sqrt(diag A), sqrt(diag D) of that record (the layout of the ensembles' filt_final)
 * At latency 0 a continuation equals one longer run when step0 = the steps made, there is no upload, filt_init = the previous
 * call's filt_state, and the first call's n_steps is a multiple of R. Latency 1 STILL RESTARTS THE SENSOR'S MEMORY with every call
 * (the first step of the second call sees its own measurement), filt_init or not: such a continuation is not the longer run.
 * f == NULL is tsat_mpc_run_held_sensed, byte for byte (it is dispatched there); the three filter arrays must then be NULL.
 * Rejected with -1 (text in tsat_last_error; nothing is launched and no workspace grows): a non-finite or negative filter option,
 * sigma_a == 0, reserved != 0; f NULL with a filter array non-NULL; a non-finite entry of filt_init; a q^ of zero norm in filt_init
 * (reported with its t); and everything tsat_mpc_run_held_sensed rejects. */
#define TSAT_FILTER_STATE_W 31
int  tsat_mpc_run_held_filtered(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                       int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                       const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                       int32_t* n_clipped, float* solve_ms, const double* Rtab, double gm,
                       const tsat_sensor_options* s, const double* sensor, double* Y_hist,
                       const tsat_filter_options* f, const double* filt_init, double* filt_state, double* filt_final);

/* tsat_mpc_run_held_sensed BEHIND THE NINE-STATE FILTER of tsat_tvlqr_ensemble_model_filtered: the loop of tsat_mpc_run_held_sensed
 * with one change — what the controller is handed. The raw measurements m_s are the parent's, and so are the blocks and the j = 0
 * rule, the clip, the dispersed RK4 step, the gravity rows (Rtab NULL iff gm == 0), the table clock, the shift, n_clipped,
 * tsat_mpc_tally, the statistic on the TRUE state and the true state written back at the end of the call. The recursion written out
 * at tsat_model_filter_options (`first`, `predict`, `update`, h = dt[t]) runs over the samples, s counted FROM THE CALL whatever
 * step0 is. The filter's model is trajectory t's parameter record: Jmat and u_scale, no actuator matrix, no residual dipole, no
 * gravity-gradient term — never the dispersed `plant`. In predict(u_s), u is the limited command of step s as U_hist[s] holds it, and
 * the field rows are the three rows the plant's own step s read (c = 0, 1/2, 1 at the table clock step s had).
 *   latency 0: s = 0: first(m_0); s >= 1: predict(u_{s-1}), then update(m_s); y_s = (w^, q^)
 *   latency 1: y_0 from first(m_0); s = 1: m_0 arrives a second time and makes no update, then predict(u_0); s >= 2:
 *              update(m_{s-1}), then predict(u_{s-1}); for s >= 1, y_s = (w-, q-): the model prediction across the delay
 * The solve's x0 at a block start, the state U_j + K_j dx acts on, and Y_hist[s] all read y_s.
 * After the last control step the filter makes ONE MORE predict(u_{n_steps-1}) with that step's rows and no update, at either latency:
 * the record a call leaves is the prior for x_{n_steps}, the state written back to the batch.
 * State between calls: one flat record of TSAT_MODEL_FILTER_STATE_W = 58 values per trajectory: q^ 4, w^ 3, b^ 3, the command of the
 * last predict 3, then the covariance by blocks A (theta theta) 6, W (w w) 6, D (b b) 6 as upper triangles 00 01 02 11 12 22 and
 * X (theta w) 9, B (theta b) 9, Y (w b) 9 row-major.
 *   filt_init   58 x T or NULL   NULL: the filter starts on the call's m_0 (`first`) and so restarts with every call. Given: the
 *                                record of trajectory t is loaded and sample 0 makes update(m_0) on it in place of first(m_0);
 *                                nothing else differs
 *   filt_state  58 x T out or NULL   the record the call leaves
 *   filt_final  12 x T out or NULL   b^, sqrt(diag P_tt), sqrt(diag P_ww), sqrt(diag P_bb) of that record (TSAT_MODEL_FILTER_W)
 * At latency 0 a continuation equals one longer run BIT FOR BIT when step0 = the steps made, there is no upload, filt_init = the
 * previous call's filt_state, and the first call's n_steps is a multiple of R. Latency 1 STILL RESTARTS THE SENSOR'S MEMORY with
 * every call (the first step of the second call sees its own measurement), filt_init or not: such a continuation is not the longer run.
 * f == NULL is tsat_mpc_run_held_sensed, byte for byte (it is dispatched there); the three filter arrays must then be NULL.
 * Rejected with -1 (text in tsat_last_error; nothing is launched and no workspace grows): a non-finite or negative filter option,
 * sigma_a == 0, sigma_g == 0, reserved != 0; f NULL with a filter array non-NULL; a non-finite entry of filt_init; a q^ of zero norm
 * in filt_init (reported with its t); and everything tsat_mpc_run_held_sensed rejects. */
#define TSAT_MODEL_FILTER_STATE_W 58
int  tsat_mpc_run_held_model_filtered(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps, int64_t step0,
                       int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo, const double* sat_hi,
                       const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last, tsat_tvlqr_stats* stats,
                       int32_t* n_clipped, float* solve_ms, const double* Rtab, double gm,
                       const tsat_sensor_options* s, const double* sensor, double* Y_hist,
                       const tsat_model_filter_options* f, const double* filt_init, double* filt_state, double* filt_final);

/* tsat_mpc_run_held_model_filtered WITH ITS ATTITUDE UPDATE REPLACED BY THE MAGNETOMETER'S — the filter of
 * tsat_tvlqr_ensemble_model_mag_filtered in the held re-planning loop: the filter a satellite with a gyro, a magnetometer and one
 * attitude fix could fly. It is the parent with one change: update(m) becomes the `update` written out at
 * tsat_model_mag_filter_options — a. the magnetometer block against a row of the slew's field table, then b. the gyro block. The
 * blocks and the j = 0 rule, the clip, the dispersed RK4 step, the gravity rows, the table clock, the shift, the tally, the statistic
 * on the TRUE state, the true state written back, the model (Jmat, u_scale, the limited command, the three rows the plant's step
 * read), `first`, `predict`, the one closing predict, the 58-value record and the 12-value filt_final are the parent's. s counted
 * FROM THE CALL:
 *   the magnetometer sample: one reading per control step, b_m,s = qrot(x_s / |x_s|, r_s) + bm + n_m(step0 + s) on the TRUE state
 *     x_s, n_m the draw the ensembles make for that generator id and knot (a tiled held run sees the ensemble's magnetometer noise at
 *     the same ids). r_s is the stage-0 row of the table clock at step s: the row the plant's step s reads at c = 0.
 *   latency 0: s = 0: first(m_0) — THE ONE ATTITUDE FIX: no magnetometer update, and q_m of every later sample is ignored;
 *              s >= 1: predict(u_{s-1}, rows_{s-1}), then update(w_m,s, b_m,s, r_s); y_s = (w^, q^)
 *   latency 1: y_0 from first(m_0); s = 1: m_0 arrives a second time and makes no update, then predict(u_0) — the field is still
 *              sampled, so the one-knot memory holds b_m,1; s >= 2: update(w_m,s-1, b_m,s-1, r_{s-1}), then predict(u_{s-1}): the
 *              delayed sample is paired with the row it was formed with; for s >= 1, y_s = (w-, q-)
 *   NO NEW TABLE READ IN THE HOLD: the hold hands the filter the three rows of each step it flies. The row at c = 1 of step s - 1 is
 *     bit for bit the row at c = 0 of step s (fma(1, dtau, tau0) is the clock's own rounded addition tau0 + dtau), and the row at
 *     c = 0 of step s - 1 is r_{s-1}: r_s and r_{s-1} are taken from the rows of the step just flown.
 *   filt_init given: sample 0 makes update(w_m,0, b_m,0, r_0) on the record in place of first, r_0 the stage-0 row of the clock as the
 *     call finds it. At latency 0 a continuation is the longer run BIT FOR BIT under the parent's conditions (step0 = the steps made,
 *     no upload, the first call's n_steps a multiple of R). At latency 1 the sensor's memory — now the field's too — restarts with
 *     every call.
 * filt_init, filt_state (TSAT_MODEL_FILTER_STATE_W x T) and filt_final (TSAT_MODEL_FILTER_W x T) are the parent's; no new width.
 * f == NULL is tsat_mpc_run_held_sensed, byte for byte (it is dispatched there); the three filter arrays must then be NULL.
 * Rejected with -1 (text in tsat_last_error; nothing is launched and no workspace grows): a non-finite or negative filter option,
 * sigma_g == 0, sigma_m == 0, reserved != 0; f NULL with a filter array non-NULL; a non-finite entry of filt_init; a q^ of zero norm
 * in filt_init (reported with its t); and everything tsat_mpc_run_held_sensed rejects. */
int  tsat_mpc_run_held_model_mag_filtered(tsat_handle* h, const tsat_options* o, const tsat_tvlqr_options* po, int32_t n_steps,
                       int64_t step0, int32_t replan_every, int32_t feedback, const double* plant, const double* sat_lo,
                       const double* sat_hi, const int64_t* noise_id, double* X_hist, double* U_hist, tsat_stats* stats_last,
                       tsat_tvlqr_stats* stats, int32_t* n_clipped, float* solve_ms, const double* Rtab, double gm,
                       const tsat_sensor_options* s, const double* sensor, double* Y_hist,
                       const tsat_model_mag_filter_options* f, const double* filt_init, double* filt_state, double* filt_final);

/* ------------------------------------------------------------------------------------------------------------
 * Sweep exchange across GPUs. The reference's Monte-Carlo is a serial loop whose iterations share nothing but the result
 * lists they append to (src/monte_carlo.jl:52-66, 199-235; src/paper_images/heatmap.jl:114-243). Here each rank — one
 * process, one handle, one GPU — solves a contiguous shard of equal size T, and ONE collective at the end appends
 * everybody's results in rank order: an RCCL all-gather over xGMI, issued on the handle's stream straight from the
 * resident batch (export kernel -> ncclAllGather, no host staging between them).
 *   tsat_comm_unique_id   rank 0 creates the 128-byte communicator id; the host distributes it to the other ranks by
 *                         whatever it has (MPI.bcast, a shared file, Distributed.jl, torch.distributed)
 *   tsat_comm_init        every rank, collectively: binds a communicator of `world` ranks to the handle's GPU
 *   tsat_sweep_allgather  every rank, collectively, after tsat_batch_run: X_all 7 x N x (world T), U_all 3 x (N-1) x (world T),
 *                         stats_all (world T) in rank order; any of the three may be NULL. on_device = 0: host buffers;
 *                         on_device = 1: device buffers of the caller on the handle's GPU. Blocks until the data is there.
 *   tsat_comm_destroy     releases the communicator (tsat_destroy does it too)
 *   tsat_comm_available   0 when RCCL can be loaded in this process, -11 otherwise: a LOCAL probe without any communication, so that
 *                         the ranks can agree (by their own means) to use this exchange before any of them enters the collective
 *                         tsat_comm_init — a rank that fails on its own would leave the others waiting inside ncclCommInitRank
 * RCCL is loaded at the first tsat_comm_* call (librccl.so.1, or $TSAT_RCCL_LIB); the library has no link-time dependency
 * on it, error code -11 reports that it is missing or that a collective failed. Every rank must hold a shard of the same
 * shape (T, N) — ragged totals: pad the last shard; tsat_sweep_allgather verifies it with a 16-byte all-gather whenever the shape
 * is new to the communicator and fails with -1 on EVERY rank when the shapes differ.
 * ------------------------------------------------------------------------------------------------------------ */
#define TSAT_COMM_ID_BYTES 128
int  tsat_comm_available(void);
int  tsat_comm_unique_id(void* id_out /* TSAT_COMM_ID_BYTES */);
int  tsat_comm_init(tsat_handle* h, const void* id /* TSAT_COMM_ID_BYTES */, int32_t rank, int32_t world);
int  tsat_sweep_allgather(tsat_handle* h, void* X_all, void* U_all, void* stats_all, int32_t on_device);
int  tsat_comm_destroy(tsat_handle* h);

/* ------------------------------------------------------------------------------------------------------------
 * Horizon selection (the caller right before the solve): cumulative magnetic Gramian of a field table and the first
 * row at which its condition number drops below `cutoff`.
 *   magnetic_gramian(B_N, dt)          src/magnetic_toolbox.jl:1-12   G_1 = hat(B_1)hat(B_1)', G_i = G_{i-1} + hat(B_i)hat(B_i)' dt
 *   condition_based_time(B_gram, cut)  src/magnetic_toolbox.jl:14-31  first 1-based i with cond(G_i) < cut, 0 if none
 * Call sites src/TortoiseSat.jl:73-82, src/monte_carlo.jl:137-140 (t_final = index * (tf - t0) / N).
 *   Btab 3 x n_rows x T (one coarse table per trajectory), dt_row T, cutoff T
 *   tf_index T out (1-based, 0 = never), cond_at T out (condition number at that row; may be NULL)
 * ------------------------------------------------------------------------------------------------------------ */
int  tsat_horizon_batch(tsat_handle* h, int64_t T, int32_t n_rows, const double* Btab, const double* dt_row,
                        const double* cutoff, int32_t* tf_index, double* cond_at);

/* ------------------------------------------------------------------------------------------------------------
 * Field-table generation (the first step of the reference's per-run setup): orbit from Keplerian elements, fixed-step
 * Euler propagation, GMST rotation, geocentric latitude/longitude, IGRF-12 (degree 13, epoch 2015 + secular variation),
 * NED -> ENU -> ECEF -> ECI.
 *   magnetic_simulation(p, t0, tf, N, mag_field)   src/magnetic_toolbox.jl:33-106   (2N rows, the last one left zero)
 *   kep_ECI(kep, t0, GM)                           src/kep_ECI.jl:1-35
 *   OrbitPlotter(x, p, t)                          src/OrbitPlotter.jl:1-52
 *   igrf12(date, r, lat, lon) (geocentric)         src/igrf.jl:70-274, src/legendre.jl:254-292, src/dlegendre.jl:221-309
 * Reference quirks are reproduced: the fixed IGRF radius (alt + R_E), the GMST expression as written, the J2 term as
 * written, element 6 used as mean anomaly.
 *   kep 6 x T   [e, a (km), i, RAAN, argp, anomaly] in degrees     t0, tf T   seconds
 *   Btab 3 x 2N x T out [Tesla, ECI] — directly usable as the `Btab` of tsat_solve_batch with n_tab = 2N
 *   pos  3 x (2N+1) x T out [km, ECI] (may be NULL)
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct tsat_btable_options {
  int32_t n_half;       /* N of magnetic_simulation: step (tf - t0)/N, 2N table rows                              */
  int32_t reserved;
  double  mjd;          /* p.MJD  (58155.0, src/TortoiseSat.jl:44)                                                */
  double  gm;           /* p.GM   km^3/s^2 (3.986004418e5, src/input_parameters.jl:26)                            */
  double  r_igrf_km;    /* alt + R_E = 400 + 6371 (src/magnetic_toolbox.jl:44,81)                                 */
  double  date;         /* decimal year handed to igrf12 (2019); 2015 <= date < 2020 is supported                 */
} tsat_btable_options;

void tsat_btable_default_options(tsat_btable_options* o);
/* ------------------------------------------------------------------------------------------------------------
 * Script arithmetic of the Monte-Carlo loop body, batched on the host (no GPU work): Bryson weights of the versine eigen-axis
 * guess (src/eigen_axis_slew.jl:1-38; Q = alpha / w_max^2, Qf = 10 Q, R = 1 / m_max^2 with the SIGNED maximum torque of the
 * guess as written, src/monte_carlo.jl:165-176) for T slews between the same two attitudes that differ only in their horizon
 * t = t0 : dt : t0 + (n_knots[t] - 1) dt. theta_f = rotation angle and axis(3) = rotation axis of the slew (computed once by
 * the caller), Jrm = inertia, row-major 3 x 3. Outputs Qd 7 x T, Qfd 7 x T, Rd 3 x T. Returns -2 when a guess is degenerate
 * (no positive torque sample), -1 on bad arguments (n_knots >= 3).
 * ------------------------------------------------------------------------------------------------------------ */
int  tsat_bryson_eigen_axis_batch(int64_t T, const int32_t* n_knots, double t0, double dt, double theta_f, const double* axis,
                                  const double* Jrm, double alpha, double beta, double* Qd, double* Qfd, double* Rd);

/* Resident field tables: with Btab = NULL, tsat_btable_batch leaves its tables on the device ([T][2 n_half][3], in the handle's
 * workspace) instead of downloading them; tsat_horizon_batch with Btab = NULL (same T, n_rows = 2 n_half) reads them there,
 * and tsat_batch_upload with Btab = NULL (n_btab = T, n_tab <= 2 n_half, btab_idx = NULL or identity) packs their first n_tab
 * rows into the solver's tables device to device — the Monte-Carlo's chain magnetic_simulation -> condition_based_time ->
 * magnetic_simulation -> solve! (src/monte_carlo.jl:134-196) without a table crossing PCIe.
 * The resident tables are the LAST call's, identified to the NULL-Btab consumers by shape only: any later tsat_btable_batch on
 * the handle replaces them (a failed or rejected call leaves none). tsat_btable_generation returns a counter that every
 * tsat_btable_batch call (and a trim of the workspace) bumps: a host that interleaves table generations records it after its
 * call and compares before the consuming call (tortoisesat.jl_amd/monte_carlo.py does). */
int64_t tsat_btable_generation(const tsat_handle* h);
int  tsat_btable_batch(tsat_handle* h, const tsat_btable_options* o, int64_t T, const double* kep, const double* t0,
                       const double* tf, double* Btab, double* pos);

#ifdef __cplusplus
}
#endif
#endif /* TORTOISE_HIP_H */
