/* pqd.h — C-ABI of libpqd, the MI355X-native process-tensor propagator behind pyaceqd's
 * `system_ace_stream` driver and its two-time sweeps.
 *
 * Drop-in boundary. Each entry point replaces one reference interface:
 *
 *   pqd_propagate / pqd_plan_*      replace the ACE engine process boundary
 *                                   `subprocess.check_output(["ACE", param_file])` + outfile parse
 *                                   (pyaceqd/general_system/general_system.py:337-343, params :227-290,
 *                                   parse read_result :104-110), batched over trajectories so the
 *                                   ThreadPoolExecutor fan-out of two_time/correlations.py:153-169 becomes
 *                                   one launch.
 *   pqd_pt_create                   replaces `add_PT <file>` + the PT files ACE writes
 *                                   (general_system.py:146-197, 236); device-resident, shared per context.
 *   pqd_ace_pt_shape / _read        read ACE's own PT files (general_system.py:153-157, 194-197) under a
 *                                   stated layout assumption (ACE_PTB_V0)
 *   pqd_free_propagators            exposes the free propagator ACEutils.FreePropagator.update(t,dt).M
 *                                   (general_system.py:324-327, `get_M_t`).
 *   pqd_dressed_states              replaces the second binary `timedep_eigenstates` and its `.ds` file
 *                                   (general_system.py:297-304) and the per-time eigenvector / occupation loops of
 *                                   general_dressed_states.py:62-70, 161-165: H(t) of every (system, output time)
 *                                   diagonalised in one launch.
 *   pqd_propagate_tau               f2py propagate_tau_module.propagate_tau   (two_time/propagate_tau.f90:3)
 *   pqd_calc_onetime_parallel       ... .calc_onetime_parallel                 (propagate_tau.f90:110)
 *   pqd_calc_onetime_parallel_block ... .calc_onetime_parallel_block           (propagate_tau.f90:189)
 *   pqd_calc_twotime_phonon_block   ... .calc_twotime_phonon_block             (propagate_tau.f90:374)
 *   pqd_four_time_8op               f2py timebin_tl.four_time_8op              (timebin/timebin_tl.f90:216)
 *   pqd_four_time                   ... .four_time                             (timebin_tl.f90:145)
 *   pqd_dynamics_t1                 ... .dynamics_t1                           (timebin_tl.f90:305)
 *
 * Conventions: complex numbers are interleaved doubles {re, im}; N x N operators row-major;
 * Liouville vectors row-major vec(rho)[i*N+j] = rho[i][j]; map-chain arguments keep the
 * reference's Fortran (column-major) layouts and index semantics, with the f2py-hidden
 * dimensions passed explicitly. All host buffers are caller-owned. Every function returns 0 on
 * success or a PQD_ERR_* code; pqd_last_error() (thread-local) describes the last failure.
 * Nothing here ever calls exit().
 */
#ifndef PQD_H
#define PQD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PQD_OK 0
#define PQD_ERR_ARG 1
#define PQD_ERR_HIP 2
#define PQD_ERR_UNSUPPORTED 3
#define PQD_ERR_NOMEM 4
#define PQD_ERR_NUMERIC 5

typedef struct { double re, im; } pqd_c128;
typedef struct pqd_ctx pqd_ctx;
typedef struct pqd_pt pqd_pt;
typedef struct pqd_plan pqd_plan;

/* The system: what the param file's add_Hamiltonian / add_Lindblad / add_Pulse lines say
 * (general_system.py:241-279). H(t) = H0 + sum_p (f_p(t) X_p + conj(f_p(t)) X_p^dagger). */
typedef struct {
    int32_t dim;                 /* N (Hilbert-space dimension) */
    double hbar;                 /* meV ps, constants.py:1 */
    const pqd_c128* H0;          /* N*N */
    int32_t n_lind;
    const double* lind_rates;    /* n_lind       (add_Lindblad <rate> {L}) */
    const pqd_c128* lind_ops;    /* n_lind*N*N */
    int32_t n_chan;              /* pulse / rotating-frame channels */
    const pqd_c128* chan_ops;    /* n_chan*N*N: X_p (already scaled, e.g. -0.5*pi*hbar*op) */
    const pqd_c128* chan_samples;/* n_chan*n_samples: f_p at sample_t0 + k*sample_dt */
    int32_t n_samples;
    double sample_t0, sample_dt; /* linear interpolation, clamped at both ends */
} pqd_system;

/* dt / ta / te of the param file; n_steps = round((te-ta)/dt). Output rows are steps 0..n_steps. */
typedef struct {
    double ta, dt;
    int32_t n_steps;
    int32_t n_sub;               /* exponential-midpoint sub-steps per half step (>= 1) */
} pqd_grid;

/* Process-tensor MPO for a diagonal system-bath coupling: per slice s and dictionary index g a
 * chi x chi matrix Q[s][g][d][d']; g = gmap[alpha] for Liouville index alpha. */
typedef struct {
    int32_t chi, D, n_slices;
    const pqd_c128* Q;           /* n_slices*D*chi*chi */
    const pqd_c128* closure;     /* n_slices*chi: bond closure after a step that used slice s */
    const pqd_c128* closure0;    /* chi: closure for the output at step 0 */
    const pqd_c128* bond0;       /* chi: initial bond vector */
    const int32_t* gmap;         /* N*N */
} pqd_pt_desc;

/* A batch of trajectories sharing system, grid, PT and initial state. Trajectory t is propagated
 * from step 0 to out_end[t] and writes n_out expectation values per step of [out_begin, out_end]
 * to out[out_offset[t] + (n - out_begin[t])*n_out + k]. MTOs = apply_Operator lines
 * (general_system.py:281-286): kind 0 "" (A rho A^dag), 1 "_left" (A rho), 2 "_right" (rho A);
 * before=1 is applyBefore true (visible at step), 0 visible one step later; same (traj, step,
 * before) operators apply in array order. */
typedef struct {
    int32_t n_traj;
    const int32_t* out_begin;
    const int32_t* out_end;
    const int64_t* out_offset;
    int32_t n_mto;
    const int32_t* mto_traj;
    const int32_t* mto_step;
    const int32_t* mto_before;
    const int32_t* mto_kind;
    const pqd_c128* mto_ops;     /* n_mto*N*N */
} pqd_traj;

int32_t pqd_version(void);
const char* pqd_last_error(void);
/* HIP version libpqd was built against (HIP_VERSION) and the one its loaded runtime reports (hipRuntimeGetVersion);
 * the Python loader warns when their major.minor differ (the process may have loaded another runtime first) */
int pqd_hip_versions(int32_t* build, int32_t* runtime);

int pqd_ctx_create(int32_t device, pqd_ctx** out);
void pqd_ctx_destroy(pqd_ctx* ctx);
int pqd_ctx_synchronize(pqd_ctx* ctx);

int pqd_pt_create(pqd_ctx* ctx, int32_t dim, const pqd_pt_desc* desc, pqd_pt** out);
/* The same PT for the Hilbert-space path with a PT (PQD_PATH_HILBERT_PT): dim in [2, 24] (PQD_ERR_UNSUPPORTED "dim %d
 * not in [2, 24]" otherwise), chi in [1, 256], pqd_pt_create's argument checks, all before any device call. The slices
 * are stored as given (no bond padding). A plan or propagate call handed such a handle runs that path at any dim,
 * dim <= 6 included; pqd_pt_create's handles choose as before. Destroyed with pqd_pt_destroy. */
int pqd_pt_create_wide(pqd_ctx* ctx, int32_t dim, const pqd_pt_desc* desc, pqd_pt** out);
void pqd_pt_destroy(pqd_pt* pt);

/* Reading the PT files ACE writes with `write_PT <name>`: <name>_initial, <name>_initial_0, <name>_repeated,
 * <name>_repeated_0 (reference general_system.py:146-157, 190, 194-197; detection :153-156). ACE's layout is
 * undocumented offline; the reader implements ONE stated assumption, "ACE_PTB_V0" (csrc/ace_pt.cpp header,
 * INTEGRATION.md), and returns PQD_ERR_UNSUPPORTED, naming the file and the mismatch, for anything else
 * (PQD_ERR_ARG when a file is missing). Host-only, no context. pqd_ace_pt_shape sizes the buffers;
 * pqd_ace_pt_read fills a pqd_pt_desc-shaped set of caller buffers (Q: n_slices*D*chi*chi, closure:
 * n_slices*chi, closure0/bond0: chi, gmap: dim*dim) with slices [0, n_init) from _initial and slice n_init (the
 * repeated slice) from _repeated; smaller bonds are zero-padded to chi. */
typedef struct {
    int32_t n_init, n_slices, chi, D;
} pqd_ace_pt_dims;
int pqd_ace_pt_shape(const char* name, int32_t dim, pqd_ace_pt_dims* shape);
int pqd_ace_pt_read(const char* name, int32_t dim, const pqd_ace_pt_dims* shape, pqd_c128* Q, pqd_c128* closure,
                    pqd_c128* closure0, pqd_c128* bond0, int32_t* gmap);

/* M_out: 2*n_steps matrices (N^2 x N^2, row-major): [2n] first half step, [2n+1] second. */
int pqd_free_propagators(pqd_ctx* ctx, const pqd_system* sys, const pqd_grid* grid, pqd_c128* M_out);

/* Dressed states: the instantaneous eigenstates of H(t_n) = H0 + sum_p (f_p(t_n) X_p + conj(f_p(t_n)) X_p^dagger) of
 * every system at every output time t_n = ta + n dt, n = 0 .. n_steps (f_p sampled as the free propagators sample it).
 * Replaces the `timedep_eigenstates` run (general_system.py:297-304) and the eigenvector loops of
 * general_dressed_states.py:62-70, 161-165. Systems of equal dim in [2, 6]; lind_* and grid->n_sub are ignored.
 * Per problem (s, n): eigenvalues ascending (ties by the solver's column index); eigenvectors of unit 2-norm,
 * the first component of magnitude > 1e-12 real and positive; occ[j] = Re sum_{i,k} v_j[i] conj(v_j[k]) rho[i][k]
 * (the reference's formula on the array compose_dm returns). Every output is optional (at least one is needed, occ
 * needs rho). PQD_ERR_NUMERIC (outputs still copied) when an H entry is not finite or a problem did not converge. */
int pqd_dressed_states(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const pqd_grid* grid,
                       const pqd_c128* rho,   /* n_sys*(n_steps+1)*N*N or NULL */
                       double* evals,         /* n_sys*(n_steps+1)*N        or NULL */
                       pqd_c128* evecs,       /* n_sys*(n_steps+1)*N*N, [s][n][j][i] = component i of eigenvector j, or NULL */
                       double* occ);          /* n_sys*(n_steps+1)*N, needs rho; or NULL */
/* Dressed states of the cavity and sensor models: pqd_dressed_states for systems of equal dim in [7, 24]
 * (PQD_ERR_UNSUPPORTED "dim %d not in [7, 24]" otherwise), with its signature, layouts, argument checks, order, norm,
 * phase and occupation rule. Serves tls_photons_dressed_states (two_level_system/tls.py:207-212),
 * biexciton_photons_dressed_states and biexciton_photons_extended_dressed_states (four_level_system/linear.py:105-109,
 * 157-159) and dressed_states(system, dim, ...) for any model of that size (general_dressed_states.py:26-44). The
 * solver is a round-robin Jacobi in LDS (csrc/dressed_wide.hip) with the same stop rule, 40 sweeps at most;
 * PQD_ERR_NUMERIC (outputs still copied) when an H entry is not finite or a problem did not converge in them. */
int pqd_dressed_states_wide(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const pqd_grid* grid,
                            const pqd_c128* rho, double* evals, pqd_c128* evecs, double* occ);
/* duration (ms, HIP events on the context stream) of the kernel of the context's last pqd_dressed_states or
 * pqd_dressed_states_wide call, whichever ran last */
int pqd_dressed_timing(pqd_ctx* ctx, double* ms_kernel);

/* one-shot: upload, propagate, download. pt may be NULL (no phonons); sched[n_steps] selects the
 * PT slice per step (NULL: min(n, n_slices-1)). rho0: N*N. out_ops: n_out*N*N.
 * Limits (PQD_ERR_UNSUPPORTED beyond them), for this call and every propagate / plan call below: with a PT of
 * pqd_pt_create dim in [2, 6]; without one dim in [2, 24], where dim > 6 takes at most 8 jump operators and a
 * Liouvillian whose norm bound times a sub-step stays below 4096 (PQD_PATH_HILBERT); with a PT of pqd_pt_create_wide
 * dim in [2, 24] equal to the PT's, at most 8 jump operators and the same norm bound at every dim, chi <= 256
 * (PQD_PATH_HILBERT_PT; its workspace of n_traj chi dim^2 16 bytes: PQD_ERR_NOMEM when it cannot be allocated);
 * n_chan <= 4. pqd_pt_create, pqd_free_propagators, pqd_dressed_states and the map-chain calls keep dim <= 6, except
 * pqd_calc_onetime_parallel and pqd_propagate_tau, which take dim in [2, 24] (see the map-chain sweeps below).
 * Dynamical maps at dim in [2, 24] come from pqd_dynmap_wide (below), which runs the same two paths. */
int pqd_propagate(pqd_ctx* ctx, const pqd_system* sys, const pqd_grid* grid, const pqd_pt* pt,
                  const int32_t* sched, const pqd_c128* rho0, int32_t n_out, const pqd_c128* out_ops,
                  const pqd_traj* traj, pqd_c128* out, int64_t out_len);

/* Dynamical maps on the Hilbert-space paths, dim in [2, 24]: dm[m][n][alpha][beta] (row-major, n_maps x n_steps x
 * N^2 x N^2, acting on row-major vec(rho)) = element alpha of the state that started as the basis element beta
 * (|i><j|, beta = i N + j) at ta[m], after step n + 1 of grid->n_steps steps of grid->dt: the map E(ta[m] + (n + 1) dt,
 * ta[m]). ta NULL: every map starts at grid->ta. The n_mto MTOs (pqd_traj's step, before, kind and operator arrays,
 * without a trajectory index) are applied inside every map, in the order of a step. pt NULL (PQD_PATH_HILBERT's
 * arithmetic) or a pqd_pt_create_wide handle (PQD_PATH_HILBERT_PT's: the closed reduced state is read out). One launch
 * of n_maps N^2 workgroups; the maps are assembled on the device and downloaded once.
 * PQD_ERR_ARG: n_maps < 1, n_steps < 1, dm_len != n_maps n_steps N^4, bad MTO arrays, a PT of pqd_pt_create.
 * PQD_ERR_UNSUPPORTED: dim outside [2, 24], more than 8 jump operators, more than 4 channels, a norm bound times a
 * sub-step above 4096, n_maps N^2 workgroups above the grid limit. PQD_ERR_NOMEM: the device buffers (twice
 * n_maps n_steps N^4 16 bytes, with a PT the workspace of n_maps N^2 chi N^2 16 bytes) cannot be allocated.
 * PQD_ERR_NUMERIC (maps still copied): a non-finite value. pqd_dynmap_timing: duration (ms, HIP events) of the
 * propagation kernel of the context's last pqd_dynmap_wide call. */
int pqd_dynmap_wide(pqd_ctx* ctx, const pqd_system* sys, const pqd_grid* grid,
                    const pqd_pt* pt /* NULL or a pqd_pt_create_wide handle */,
                    const int32_t* sched,
                    int32_t n_maps, const double* ta /* n_maps start times; NULL: grid->ta */,
                    int32_t n_mto, const int32_t* mto_step, const int32_t* mto_before,
                    const int32_t* mto_kind, const pqd_c128* mto_ops,
                    pqd_c128* dm, int64_t dm_len /* n_maps*n_steps*N^4 */);
int pqd_dynmap_timing(pqd_ctx* ctx, double* ms_kernel);

/* multi-system batch (pulse / field parameter scans): n_sys systems of equal dim share
 * grid, PT, initial state and output operators; trajectory t uses systems[traj_sys[t]]. This replaces the
 * caller-side scan loops over ACE runs (rabi_rotations.py:172-198, the C5 pulse/B-field scan). */
int pqd_propagate_multi(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                        const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                        int32_t n_out, const pqd_c128* out_ops, const pqd_traj* traj, pqd_c128* out,
                        int64_t out_len);

/* pqd_propagate_multi returning ACE's output table instead of the flat output buffer: per trajectory t, at offset
 * sum_{u<t} (1 + n_out) * L_u (L = out_end - out_begin + 1), (1 + n_out) rows of L values, row 0 = the times
 * ta + dt * step (imaginary part 0), row 1 + k = output k. Replaces reading the ACE outfile
 * (general_system.py:343: `np.loadtxt(outfile, dtype=complex).T`, one table per ACE run); the transposition runs on
 * the device, so a caller gets every trajectory's table as a view of one buffer. table_len >= sum of the tables. */
int pqd_propagate_table(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                        const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                        int32_t n_out, const pqd_c128* out_ops, const pqd_traj* traj, pqd_c128* table,
                        int64_t table_len);

/* pqd_propagate_table's run reduced on the device to trapezoid integrals over each trajectory's output window, in
 * place of the tables: with y_k(s) = output k at window step s (s = 0 .. L_t - 1) and a uniform spacing dx,
 *   res[t * n_pairs + q] = dx * (y_{k_head[q]}(0) / 2 + sum_{s=1}^{L_t-2} y_{k_tail[q]}(s) + y_{k_tail[q]}(L_t - 1) / 2)
 * (0 when L_t < 2). This is the tau integral of G2_reuse (pol_entanglement/G2.py:484-505: tau = 0 from
 * <op1 op2 op3 op4> at t1, tau > 0 from <op2 op3>, np.trapz over t2) for every t1 trajectory at once; only
 * n_traj * n_pairs values leave the device. pqd_plan_trapz: the same reduction of an executed plan's outputs. */
int pqd_propagate_trapz(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                        const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                        int32_t n_out, const pqd_c128* out_ops, const pqd_traj* traj, int32_t n_pairs,
                        const int32_t* k_head, const int32_t* k_tail, double dx, pqd_c128* res);

/* device-resident plan for repeated execution (bench, scans): same arguments as pqd_propagate(_multi). */
int pqd_plan_create(pqd_ctx* ctx, const pqd_system* sys, const pqd_grid* grid, const pqd_pt* pt,
                    const int32_t* sched, const pqd_c128* rho0, int32_t n_out, const pqd_c128* out_ops,
                    const pqd_traj* traj, int64_t out_len, pqd_plan** out);
int pqd_plan_create_multi(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                          const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                          int32_t n_out, const pqd_c128* out_ops, const pqd_traj* traj, int64_t out_len,
                          pqd_plan** out);
/* enqueue free-propagator build (if rebuild_free) + sweep on the context stream (asynchronous) */
int pqd_plan_execute(pqd_plan* plan, int32_t rebuild_free);
/* device pointer of the plan's output buffer (out_len complex values); valid after pqd_plan_synchronize */
void* pqd_plan_output_device(pqd_plan* plan);
/* wait for the last execute and check it: a split-group launch (PQD_PATH_SPLIT) that timed out because its
 * workgroups could not all be resident (device shared with other work) is re-run on the batched kernel, and
 * the plan stays batched; a NaN/Inf output returns PQD_ERR_NUMERIC. Replaces the reference's
 * CalledProcessError on a failed ACE run (general_system.py:339-341). */
int pqd_plan_synchronize(pqd_plan* plan);
/* pqd_plan_synchronize + copy of the outputs (also on PQD_ERR_NUMERIC, which is still returned) */
int pqd_plan_download(pqd_plan* plan, pqd_c128* out, int64_t out_len);
/* pqd_plan_synchronize + copy of the outputs into `dst`, a device buffer of the plan's device (or host memory) of
 * out_len complex values, e.g. a torch tensor that a collective then gathers over xGMI (scan.py). Replaces the
 * reference's result lists assembled from per-process CSV files (correlations.py:171-183). */
int pqd_plan_copy_output(pqd_plan* plan, void* dst, int64_t out_len);
/* the plan's ACE-table length (complex values, layout of pqd_propagate_table) and pqd_plan_synchronize + the tables */
int pqd_plan_table_len(const pqd_plan* plan, int64_t* table_len);
int pqd_plan_download_table(pqd_plan* plan, pqd_c128* table, int64_t table_len);
int pqd_plan_trapz(pqd_plan* plan, int32_t n_pairs, const int32_t* k_head, const int32_t* k_tail, double dx,
                   pqd_c128* res);
#define PQD_PATH_NOPT 0     /* no PT: one wave per trajectory */
#define PQD_PATH_BATCHED 1  /* lock-step PT sweep, bt trajectories per workgroup */
#define PQD_PATH_SPLIT 2    /* one trajectory over N^2 workgroups (latency path) */
#define PQD_PATH_QUAD 3     /* two-level system: four trajectories per wave set, state in registers (pt_quad.hip) */
#define PQD_PATH_MSPLIT 4   /* several trajectories per split group: row g of TB trajectories per workgroup (pt_msplit.hip) */
#define PQD_PATH_HILBERT 5  /* no PT, dim 7..24 (dim <= 6 under PQD_HILBERT=1): one workgroup per trajectory, rho as an
                               N x N matrix, exp(L w) applied matrix-free (lind_hilbert.hip). bt is 1, there are no free
                               propagators (rebuild_free is ignored, ms_free is 0, no windows, no lean instance) */
#define PQD_PATH_HILBERT_PT 6  /* a PT of pqd_pt_create_wide, dim 2..24: one workgroup per trajectory, rho (x) bond as chi
                               N x N slices in a workspace, the half steps of PQD_PATH_HILBERT on every slice, the PT
                               slice per element (lind_hilbert_pt.hip). bt, free propagators, windows, lean: as path 5 */
/* the path the plan runs now, its trajectories per workgroup, how many split launches fell back, and the
 * trajectory-steps one execute propagates (trajectories of one system that share a lock-step workgroup propagate
 * their common MTO-free trunk once: PQD_BRANCH) */
int pqd_plan_info(const pqd_plan* plan, int32_t* path, int32_t* bt, int32_t* split_fallbacks, int64_t* traj_steps);
/* 1 when the plan builds its free propagators through pulse windows (half steps outside a system's first..last driven
 * half step are not built; its kernels read the idle operators there: DESIGN.md §4.2, PQD_WIN), else 0 */
int pqd_plan_windows(const pqd_plan* plan, int32_t* on);
/* 1 when the plan's batched sweep (PQD_PATH_BATCHED) runs the lean instance of the lock-step kernel: the one compiled
 * for the headline configuration only (N^2 = 16, chi = 64, 8 trajectories per workgroup, default switches; DESIGN.md
 * §4.1, PQD_SWEEP_LEAN=0 forces the general instance), else 0 */
int pqd_plan_sweep_lean(const pqd_plan* plan, int32_t* on);
/* 1 when the lean instance's launches of this plan read the outputs inside the fused column phase: some workgroup has
 * steps after its last MTO and activation and before its last two steps (PQD_LEAN_RO=0 keeps the separate
 * closure pass on every step), else 0. Results agree with the other readout to rounding (the order of two sums) */
int pqd_plan_sweep_readout(const pqd_plan* plan, int32_t* on);
/* the number of workgroups of the plan whose fast steps (pqd_plan_sweep_readout) take the fused column operator, the
 * output rows W(n) and the closure vector from LDS, staged there during the PT phase of the step before: every workgroup
 * with fast steps whose trajectories all belong to one system (PQD_LEAN_STAGE=0 keeps the loads where
 * they are used, and so do workgroups that mix systems). 0 where the plan reads no outputs in the column phase. Results
 * are bit-identical either way */
int pqd_plan_sweep_stage(const pqd_plan* plan, int32_t* n_blocks);
/* every decision plan creation took, as one line of space-separated key=value pairs in a fixed order: the device's
 * CU count, path (PQD_PATH_*), workgroup shape, split / quad / multi-trajectory split / trunk layout, windows, the
 * A/B switches as the kernels will see them, and 64-bit FNV-1a hashes (hex) of the block arrays, the PT row-unit list
 * and the multi-trajectory group tables (0 where the plan has none). The decisions set speed, not results; tests pin
 * them with this line. PQD_ERR_ARG if the line and its terminating NUL do not fit len bytes */
int pqd_plan_describe(const pqd_plan* plan, char* buf, int32_t len);
/* Liouville rows that can ever be nonzero: live[a] = 1 for the rows alpha = i N + j reachable from the
 * nonzero entries of rho0 through L0 of every system, S_p and T_p of every channel with a nonzero sample anywhere in its
 * array, and the superoperators of the trajectories' MTOs (traj may be NULL: none), each entry judged by exact != 0 as
 * it is uploaded; 0 for the rows that are exactly zero at every step of every trajectory. live: N*N bytes. Host only: no
 * context, no device. The batched sweep gives rows with 0 no PT unit (PQD_LIVE_ROWS=0: all rows; 2: synchronize also
 * checks that no stored free propagator leads from a live column into such a row, PQD_ERR_NUMERIC otherwise).
 * pqd_plan_live_rows: the mask the plan's sweep uses (len = N*N): all 1 where it leaves nothing out (another path, no
 * PT, a wide PT, PQD_LIVE_ROWS=0). pqd_plan_describe ends with " live=<hex mask> parts=<0|1>" for a plan that leaves
 * rows out (parts: the lean instance deals the live rows in quarters, PQD_LIVE_PART=0: whole rows), and is the line it
 * always was for every other plan. */
int pqd_live_rows(int32_t n_sys, const pqd_system* systems, const pqd_c128* rho0, const pqd_traj* traj, uint8_t* live);
int pqd_plan_live_rows(const pqd_plan* plan, uint8_t* live, int32_t len);
/* The compact row index in which the lean instance applies the fused column operator F(n) where rows stay zero
 * (DESIGN.md §4.1). pqd_live_col_map: rho (len bytes) lists the rows with live[a] != 0 in increasing order, then the
 * others in increasing order; *kc = ceil(n_live / 4), the k-steps of four compact rows the product needs. Host only.
 * pqd_plan_sweep_colk: the k-steps the plan's fast steps (pqd_plan_sweep_readout) run: 3 where the lean instance runs
 * partial units (parts=1) with 9 to 12 live rows of 16, else 4 (also PQD_LIVE_COL=0). Results are bit-identical either
 * way; pqd_plan_describe then ends with " colk=3" behind parts=. */
int pqd_live_col_map(const uint8_t* live, int32_t len, uint8_t* rho, int32_t* kc);
int pqd_plan_sweep_colk(const pqd_plan* plan, int32_t* colk);
/* average kernel durations (ms) of the executions since the last reset (the most recent 64 at most),
 * from HIP events on the launch stream: [0] free-propagator kernel, [1] sweep kernel; n = executions */
int pqd_plan_timing(pqd_plan* plan, double* ms_free, double* ms_sweep, int32_t* n, int32_t reset);
void pqd_plan_destroy(pqd_plan* plan);

/* ---- map-chain sweeps: reference Fortran signatures, hidden dims explicit, Fortran layouts ----
 * Dimension limits (PQD_ERR_UNSUPPORTED outside them): pqd_propagate_tau and pqd_calc_onetime_parallel take dim in
 * [2, 24] ("dim %d not in [2, 24]"): dim <= 6 on the packed one-wave kernels (mapchain.hip), dim 7..24 on the sweep by
 * position (mapchain_wide.hip: one matrix-core product per map position for all trajectories in flight; PQD_MC_WIDE=1
 * sends dim <= 6 there as well). pqd_calc_onetime_parallel_block, pqd_calc_twotime_phonon_block, the time-bin calls and
 * pqd_map_tail keep dim in [2, 6] ("dim %d not in [2, 6]"; N2 <= 36).
 * Above dim 6 only the maps the sweep reads are uploaded (max_i j_i - 1 + n_tau of them, n_tau for pqd_propagate_tau);
 * PQD_ERR_NOMEM, naming the bytes, when the device buffers cannot be allocated. */
int pqd_propagate_tau(pqd_ctx* ctx, const pqd_c128* dm_tl, int32_t n_maps, const pqd_c128* rho_init,
                      int32_t n_tau, int32_t dim, int32_t j_start, pqd_c128* rho_out);
/* PQD_ERR_ARG when a trajectory would read a map past dm_tl(:, :, n_tfull - 1) (time_sparse beyond time, or
 * j_i - 1 + n_tau > n_tfull - 1; the Fortran reads out of bounds there), on the blocked sweep and on the map-by-map
 * kernels (PQD_MC_BLOCKED=0) alike */
int pqd_calc_onetime_parallel(pqd_ctx* ctx, const pqd_c128* dm_tl, const pqd_c128* rho_init, int32_t n_tau,
                              int32_t n_t, int32_t n_tfull, int32_t dim, const pqd_c128* opA,
                              const pqd_c128* opB, const pqd_c128* opC, const double* time,
                              const double* time_sparse, pqd_c128* result);
/* The schedule of the sweep by position, as pqd_calc_onetime_parallel at dim 7..24 runs it. Host-only: no context, no
 * device. pos (n_t, may be NULL): the trunk ends p_i = j_i - 1 by the Fortran's comparisons (never decreasing).
 * *n_rows = Q + 1 with Q = max_i p_i + n_tau. sched (may be NULL; sched_rows rows of 5 int32, PQD_ERR_ARG when fewer
 * than *n_rows): row q = (live_lo, live_hi, trunk, spawn_lo, spawn_hi): before the step of position q the trajectories
 * [spawn_lo, spawn_hi), those with p_i == q, start from the trunk state; the step (q < Q) multiplies map q + 1 into
 * the trajectories [live_lo, live_hi), those with p_i <= q < p_i + n_tau, and into the trunk state when trunk = 1
 * (q < max_i p_i). Row Q holds spawns only (n_tau = 0).
 * pqd_mc_wide_timing: duration (ms, HIP events) and number of the kernel launches of the context's last
 * pqd_calc_onetime_parallel, pqd_calc_onetime_parallel_block_wide or pqd_propagate_tau call that ran on the sweep by
 * position; PQD_ERR_ARG before one has. */
int pqd_mc_wide_schedule(const double* time, int32_t n_tfull, const double* time_sparse, int32_t n_t, int32_t n_tau,
                         int32_t* pos, int32_t* n_rows, int32_t* sched, int32_t sched_rows);
int pqd_mc_wide_timing(pqd_ctx* ctx, double* ms_kernel, int32_t* launches);
int pqd_calc_onetime_parallel_block(pqd_ctx* ctx, const pqd_c128* dm_block, const pqd_c128* dm_s,
                                    const pqd_c128* rho_init, int32_t n_tb, int32_t nx_tau, int32_t n_map,
                                    int32_t n_t, int32_t n_tfull, int32_t dim, const pqd_c128* opA,
                                    const pqd_c128* opB, const pqd_c128* opC, const double* time,
                                    const double* time_sparse, pqd_c128* result);
/* The periodic sweep at dim in [2, 24] ("dim %d not in [2, 24]"), always as the sweep by position of mapchain_wide.hip;
 * arguments, NULL and size checks of pqd_calc_onetime_parallel_block, which itself keeps dim in [2, 6] (PQD_MC_WIDE
 * does not reach it). Two map cursors: the trunk and the trajectories whose trunk ends at p_i >= n_tb follow the
 * straight one (dm_block(:, :, q + 1) while q < n_map, dm_s after), those with p_i < n_tb the ring one (the same rule
 * at q mod n_tb); a position where the two name different maps still costs one step launch. Only the block maps the
 * call reads and dm_s are uploaded: the device footprint does not grow with the number of positions (PQD_ERR_NOMEM
 * names the bytes). pqd_mc_wide_timing reports the call.
 * pqd_mc_wide_block_schedule: the schedule that call walks. Host-only, as pqd_mc_wide_schedule: pos, *n_rows = Q + 1
 * with Q = max_i p_i + n_tb nx_tau, sched rows of 9 int32 (ring_lo, ring_hi, ring_map, str_lo, str_hi, trunk, str_map,
 * spawn_lo, spawn_hi): the step of position q multiplies map ring_map into the trajectories [ring_lo, ring_hi) (inside
 * [0, n_ring), n_ring = the number of p_i < n_tb) and map str_map into [str_lo, str_hi) (inside [n_ring, n_t)) and,
 * when trunk = 1, into the trunk state. A map index m < n_map is dm_block(:, :, m + 1), m = n_map is dm_s. */
int pqd_calc_onetime_parallel_block_wide(pqd_ctx* ctx, const pqd_c128* dm_block, const pqd_c128* dm_s,
                                         const pqd_c128* rho_init, int32_t n_tb, int32_t nx_tau, int32_t n_map,
                                         int32_t n_t, int32_t n_tfull, int32_t dim, const pqd_c128* opA,
                                         const pqd_c128* opB, const pqd_c128* opC, const double* time,
                                         const double* time_sparse, pqd_c128* result);
int pqd_mc_wide_block_schedule(const double* time, int32_t n_tfull, const double* time_sparse, int32_t n_t,
                               int32_t n_tb, int32_t nx_tau, int32_t n_map, int32_t* pos, int32_t* n_rows,
                               int32_t* sched, int32_t sched_rows);
/* n_tauc = 0 is the Fortran's empty loop over the per-trajectory maps: dm_taucs2 is not read and may be NULL */
int pqd_calc_twotime_phonon_block(pqd_ctx* ctx, const pqd_c128* dm_taucs2, const pqd_c128* dm_sep1,
                                  const pqd_c128* dm_sep2, const pqd_c128* dm_s, const pqd_c128* rho_init,
                                  int32_t n_tb, int32_t nx_tau, int32_t n_map, int32_t n_t, int32_t n_tfull,
                                  int32_t n_tauc, int32_t dim, const pqd_c128* opA, const pqd_c128* opB,
                                  const pqd_c128* opC, const double* time, const double* time_sparse,
                                  pqd_c128* result);
/* The time-bin entry points (this one, _rows, pqd_four_time, pqd_dynamics_t1) propagate over the segments (0, t1_i),
 * (t1_i, t1_j), (t1_j, tb) resp. (t1_i, t1_i+1) as propagate_tb does (timebin_tl.f90:50-77): n_map explicit maps, then
 * one precalc map per set bit of the steps left. PQD_ERR_ARG, before anything is launched, when a segment the call
 * reaches leaves 2^n_precalc steps or more (the Fortran reads past dm_tl_precalc; the reference's own
 * n_precalc = int(log2(tb / dt)) + 1 never does for t1 <= tb) or applies explicit maps from a negative time */
int pqd_four_time_8op(pqd_ctx* ctx, const pqd_c128* dm_1, const pqd_c128* dm_2, const pqd_c128* rho_init,
                      const double* t1, const pqd_c128* precalc, int32_t n_t, double dt, int32_t n_map,
                      int32_t dim, const pqd_c128* ops8, int32_t early_only, int32_t late_t1_only, double tb,
                      int32_t n_precalc, pqd_c128* result);
/* pqd_four_time_8op restricted to the rows i in [row_lo, row_hi) of the (t1, t2 >= t1) triangle: result(i, i + j)
 * for those rows, every other element 0. One rank's share of the pair grid split over GPUs (a
 * load-balanced triangular row split of timebin_tl.f90:255-302's loop over i; python: scan.triangular_rows). */
int pqd_four_time_8op_rows(pqd_ctx* ctx, const pqd_c128* dm_1, const pqd_c128* dm_2, const pqd_c128* rho_init,
                           const double* t1, const pqd_c128* precalc, int32_t n_t, double dt, int32_t n_map,
                           int32_t dim, const pqd_c128* ops8, int32_t early_only, int32_t late_t1_only, double tb,
                           int32_t n_precalc, int32_t row_lo, int32_t row_hi, pqd_c128* result);
int pqd_four_time(pqd_ctx* ctx, const pqd_c128* dm_1, const pqd_c128* dm_2, const pqd_c128* rho_init,
                  const double* t1, const pqd_c128* precalc, int32_t n_t, double dt, int32_t n_map, int32_t dim,
                  const pqd_c128* ops4, double tb, int32_t n_precalc, pqd_c128* result);
int pqd_dynamics_t1(pqd_ctx* ctx, const pqd_c128* dm_1, const pqd_c128* dm_2, const pqd_c128* rho_init,
                    const double* t1, const pqd_c128* precalc, int32_t n_t, double dt, int32_t n_map,
                    int32_t dim, double tb, int32_t n_precalc, pqd_c128* result);

/* ---- tau tails on one constant map (the `for j: X = tl_map2 @ X; G[:, n_tauc + j + 1] = Bt @ X` loops of
 * tl_three_op_two_time_phonons / tl_threeoptwotime_phonons_dm, reference two_time/correlations.py:866-1186) ----
 * out[i][j] = w . M^{j+1} x_i for i < n_x, j < n_steps. M: N2 x N2 row-major, X: [n_x][N2] row-major, w: N2,
 * out: [n_x][n_steps] row-major. N2 in {4, 9, 16, 25, 36}. */
int pqd_map_tail(pqd_ctx* ctx, const pqd_c128* M, int32_t N2, const pqd_c128* X, int32_t n_x, const pqd_c128* w,
                 int32_t n_steps, pqd_c128* out);

/* ---- time-local dynamical maps (replaces tools.calc_tl_dynmap_pseudo, reference tools.py:446-484) ----
 * dm: n_maps row-major n x n maps, dm[i] = E(t_{i+1}, t0). out (n_maps maps): out[0] = dm[0],
 * out[i] = dm[i] pinv(dm[i-1]) with singular values <= rcond * max(s) dropped (numpy pinv, rcond
 * 1e-12 in the reference). 1 <= n <= 576 (N <= 24; any n, not only squares): n <= 36 on the single-wave
 * kernel (tlmap.hip), 37 <= n <= 576 on the block-Jacobi kernel (tlmap_wide.hip), whose workspace is sized
 * by its persistent grid, not by n_maps. n_maps == 0 returns PQD_OK without touching the device.
 * PQD_ERR_ARG: a NULL argument, n_maps < 0, rcond negative or NaN. PQD_ERR_UNSUPPORTED: n < 1 or n > 576
 * ("map size %d (max 576)"). PQD_ERR_NOMEM: the input maps, the output maps (n_maps n^2 16 bytes each) or
 * the workspace cannot be allocated; the message names the bytes asked for. PQD_ERR_NUMERIC (every n; out
 * still copied): a map's Jacobi SVD was still rotating after 40 sweeps, or a singular value was not finite.
 * pqd_tl_dynmap_timing: duration (ms, HIP events) of the kernel of the context's last pqd_tl_dynmap_pseudo
 * call (either kernel); PQD_ERR_ARG before any call has completed. pqd_tl_dynmap_sweeps: the largest sweep
 * count over the maps of that call (either kernel; the sweeps run, the last one without a rotation; 0 when
 * n_maps == 1, where no kernel runs). */
int pqd_tl_dynmap_pseudo(pqd_ctx* ctx, const pqd_c128* dm, int32_t n_maps, int32_t n, double rcond,
                         pqd_c128* out);
int pqd_tl_dynmap_timing(pqd_ctx* ctx, double* ms_kernel);
int pqd_tl_dynmap_sweeps(pqd_ctx* ctx, int32_t* max_sweeps);

/* ---- PT generator factorizations (replaces the factorizations inside `ACE <generate.param>` with
 * `dont_propagate true` + `write_PT`, reference general_system.py:152-211; driven by pyaceqd_amd/ptgen_gpu.py,
 * whose host restatement is pyaceqd_amd/ptgen.py). Device pointers, column-major matrices (ld = rows), all work
 * enqueued on `stream` (a hipStream_t). pqd_ptg_qr with pivot = 0 returns with its work still queued (its rank is
 * min(m, n)); with pivot = 1, and pqd_ptg_jacobi, it synchronises with the stream (the rank / sweep count decides
 * what the caller does next).
 *
 * pqd_ptg_qr: Householder QR of W (m x n, overwritten). pivot = 0: W = Q R with rank = min(m, n) (LAPACK zgeqrf
 * reflectors, R real diagonal). pivot = 1: column pivoting on the trailing column norms, stopping at the first step
 * whose largest trailing column norm is <= tol (a rank-revealing truncation): W P ~= Q R; tol < 0 means |tol| times
 * the largest column norm of W (found on the device: no host pass over W). pivot = 2: the same, with R returned in
 * W's own column order (R P^T: column perm[j] of the output is column j of R), so that W ~= Q R directly. Outputs: Q (m x rank),
 * R (rank x n, columns in pivoted order), perm (n: column j of W P is column perm[j] of W), *rank (host).
 * Kernel choice (environment, read per call; every combination is parity-tested): PQD_PTG_SMALL=0 (no
 * single-workgroup LDS kernel), PQD_PTG_WG=0 (per-wave column steps instead of workgroup-per-column steps with the
 * columns in registers), PQD_PTG_PAIR=0 (one reflector per launch), PQD_PTG_BLOCKED=1 (plain QRs factorized in
 * panels of 32 columns with a compact-WY trailing update), PQD_PTG_QFB=0 (Q by the per-wave reflector kernel
 * instead of blocks of 32 reflectors). */
int pqd_ptg_qr(void* stream, pqd_c128* W, int32_t m, int32_t n, int32_t pivot, double tol, pqd_c128* Q,
               pqd_c128* R, int32_t* perm, int32_t* rank);
/* pqd_ptg_jacobi: one-sided Jacobi SVD of a square n x n X (overwritten): X V = U diag(sigma), columns rotated
 * until every pair satisfies |x_p^H x_q| <= tol |x_p| |x_q|; a column with |x_j| < zero_tol ||X||_F is treated as
 * zero (never rotated). Outputs: X <- U (unit columns, unsorted), V (n x n), sigma (n, unsorted), *sweeps (host):
 * the sweeps run, the last one without a rotation, or max_sweeps + 1 when max_sweeps sweeps did not converge.
 * Scratch is kept per (device, stream): calls on different streams or devices never share a buffer. */
int pqd_ptg_jacobi(void* stream, pqd_c128* X, int32_t n, pqd_c128* V, double* sigma, double tol, double zero_tol,
                   int32_t max_sweeps, int32_t* sweeps);
/* pqd_ptg_jacobi runs its sweeps in one persistent launch (a grid barrier per round) when n <= 1024; if a barrier
 * wait times out (the workgroups were not all resident), the launch is rerun from a saved copy of X with one launch
 * per round. pqd_ptg_counters: how many times that happened in this process (diagnostics, tests). */
int pqd_ptg_counters(int32_t* jacobi_fallbacks);
/* With PQD_PTG_QPERSIST=1, pqd_ptg_qr runs a column-pivoted QR whose columns fit in registers (m <= 4096) in one
 * persistent launch (workgroup g holds physical column g; a grid barrier per step) when its n workgroups can all be
 * resident; a timed-out barrier wait reruns it from a saved copy with one launch per step (the default path, which
 * measured faster: profiles/r04/ptgen/qpersist/). PQD_PTG_QPERSIST=2 also takes plain QRs.
 * pqd_ptg_qr_counters: how many reruns happened in this process (diagnostics, tests). */
int pqd_ptg_qr_counters(int32_t* qrcp_fallbacks);

#ifdef __cplusplus
}
#endif
#endif
