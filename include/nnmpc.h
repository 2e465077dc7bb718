/* nnmpc.h -- C ABI of libnnmpc_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the offline-MPC hot path of
 * pratyushkumar211/industrial_nnmpc_2021.  Every entry point replaces one
 * reference interface (file:line into the reference repo):
 *
 *   nnmpc_qp_create        <- DenseQPRegulator.__init__/_setup_fixed_matrices
 *                             (lib/linearMPC.py:339-395): takes the condensed
 *                             P (n x n) and tq (n x n_aug) the reference builds.
 *   nnmpc_qp_solve_batch   <- DenseQPRegulator.solve -> cvxopt.solvers.qp(P, tq@x0, G, h)
 *                             (lib/linearMPC.py:495-512, :503-504) with the
 *                             box G = blockdiag([I;-I]), h = tile([uub;-ulb])
 *                             (:476-493), for B independent (x0, ulb, uub).
 *   nnmpc_nn_create        <- RegulatorLayerWith/WithoutUprev.__init__
 *                             (lib/LinearMPCLayers.py:22-32, :73-83) /
 *                             NeuralNetworkController regulator_weights, xscale
 *                             (lib/controller_evaluation.py:780-839).
 *   nnmpc_nn_forward       <- RegulatorLayerWith/WithoutUprev.call
 *                             (lib/LinearMPCLayers.py:40-61, :91-112) ==
 *                             NeuralNetworkController._get_control_input
 *                             (lib/controller_evaluation.py:863-892).
 *   nnmpc_nn_create_ex     <- the same, or UnstdRegulatorLayer (lib/LinearMPCLayers.py:135-159) /
 *                             NeuralNetworkControllerUnstd (lib/controller_evaluation.py:895-916)
 *                             by its `form`; nnmpc_nn_forward serves every form.
 *
 * Conventions: plain pointers and sizes only; all matrices row-major; the
 * caller owns every buffer it passes; a handle owns its device copies and
 * workspace; functions return 0 on success or a negative NNMPC_E* code and
 * never throw; nnmpc_last_error() describes the last failure of the calling
 * thread.  A handle is bound to the HIP device current at create time and is
 * not re-entrant.  `ptr_kind` says where the per-call buffers live:
 * NNMPC_HOST (the library stages them through PCIe) or NNMPC_DEVICE (HBM
 * resident, used in place).
 */
#ifndef NNMPC_H
#define NNMPC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NNMPC_OK 0
#define NNMPC_EINVAL (-1)   /* bad argument */
#define NNMPC_EHIP (-2)     /* HIP runtime error */
#define NNMPC_ENOMEM (-3)
#define NNMPC_ENOTIMPL (-4)

#define NNMPC_HOST 0
#define NNMPC_DEVICE 1

/* per-problem status written by nnmpc_qp_solve_batch */
#define NNMPC_ST_OPTIMAL 0   /* KKT conditions verified in fp64 */
#define NNMPC_ST_MAXITER 1   /* round / polish budget exhausted (method 2: or an active set beyond asm_max_active), not certified */
#define NNMPC_ST_NUMERIC 2   /* non-positive pivot or NaN; nnmpc_ts_*: also an infeasible or rank-deficient problem (see there) */

typedef struct nnmpc_qp nnmpc_qp;
typedef struct nnmpc_nn nnmpc_nn;

typedef struct {
  int32_t max_batch;         /* resident problems per wave (rounded up to 128); 0 = 1024 */
  int32_t nb;                /* Cholesky block 64 | 128; 0 = auto */
  int32_t max_ipm_iters;     /* 0 = 40 */
  int32_t max_polish_rounds; /* 0 = 150 (the single-exchange fallback against cycling may take one round per bound) */
  int32_t max_refine;        /* PCG steps per active set and factor; 0 = 60.  On a fresh factor the cap ends the refinement (the KKT check judges
                                what it reached); on a reused factor (stale_max_changes) it asks for the factor of the current set first */
  int32_t max_rounds;        /* lock-step rounds a problem may stay resident; 0 = 1000 */
  int32_t sub_steps;         /* solve sub-steps (PCG steps / KKT check) per round; 0 = 8 */
  int32_t stale_max_changes; /* polish: reuse the previous factor as PCG preconditioner when at most
                                this many bounds changed; 0 = 4, < 0 = always refactor */
  int32_t stale_cg_limit;    /* ... and refactor anyway after this many PCG steps; 0 = 16 */
  int32_t method;            /* 0 = auto: shared-inverse active-set pass (needs nnmpc_qp_set_inverse),
                                PDIP for what it leaves; 1 = PDIP only; 2 = active-set pass only */
  int32_t asm_max_active;    /* active-set pass: largest active set handled (<= 768, rounded down to a multiple of 16, at least 16);
                                0 = 768.  A set of exactly this many bounds is solved by the pass; a problem whose set is larger
                                at ANY iteration (not only at the optimum) leaves it: method 0 solves it on the PDIP path, method 2
                                reports NNMPC_ST_MAXITER for it -- its u and active rows are then not an answer */
  int32_t asm_max_rounds;    /* ... and its budget; 0 = 200 lock-step rounds (all-at-once exchanges settle in ~5) and 50 000
                                iterations per problem in the device tail (the single-exchange fallback against cycling is
                                finite but can take tens of thousands of ~30 us iterations on ill-conditioned Hessians with
                                half of the bounds active); > 0: that many of either; what is left goes to the PDIP path */
  int32_t asm_f32_rounds;    /* 0 = the rounds run in f32 until a problem's set settles, then in fp64 (only fp64
                                results are accepted); < 0 = fp64 from the first round */
  int32_t seg_max;           /* problems per segment (one lock-step pass; ~0.3 MB of workspace each at n = 4480);
                                0 = as many as a quarter of the free HBM holds (at most 2^20) */
  int32_t asm_tail_batch;    /* a call (segment) of at most this many problems is finished on the device from the start
                                (asm_tail_k, one workgroup per problem, no lock-step rounds): the chains of a task, a
                                controller's single QP; 0 = 256 (the most the kernel's slabs hold), < 0 = never */
  int32_t asm_predict_iters; /* iterations of the dual accelerated-projected-gradient predictor that names the FIRST active sets of
                                the rounds (bf16 MFMA, csrc/qp_predict.h): 0 = adaptive (0.3 per bound x_unc violates, 8 .. 64, by workgroup of 64
                                problems), > 0 = that many (<= 64), < 0 = off (first sets = the bounds x_unc violates).
                                Affects only the number of rounds, never a result; used when n >= 512, nu <= 64, no caller's guess */
  int32_t asm_overlap;       /* 0 = a far-field full-width pass runs on a side stream while the next round of the problems that did
                                not settle runs beside it in a second, small row space (csrc/qp_solver.hip: solve_segment_asm);
                                < 0 = off (every pass and round in sequence on one stream).  Affects only the order of the work */
  float ipm_tol;             /* PDIP exit, objective scaled by 1/median(diag P):
                                |r_d|_inf and mu <= tol*max(1,|q|_inf); 0 = 1e-2 */
  double refine_tol;         /* PCG exit: |step|_inf <= tol*max(1,|x|_inf); 0 = 1e-10 */
  double bound_tol;          /* primal feasibility slack of the KKT check; 0 = 1e-9 */
} nnmpc_qp_opts;

typedef struct {
  int64_t problems;          /* problems solved since the last reset */
  int64_t rounds;            /* lock-step rounds executed */
  int64_t factorizations;    /* per-problem Cholesky factorisations */
  int64_t ipm_iterations;    /* per-problem PDIP iterations */
  int64_t panel_launches;    /* launches of the dominant kernel (chol_panel) */
  double panel_ms;           /* hipEvent time of those launches (profiling on) */
  double diag_ms;            /* same for chol_diag */
  double trsv_ms;            /* same for trsv */
  double total_ms;           /* hipEvent time of whole solve_batch calls */
  double panel_flops;        /* algorithmic flops executed by chol_panel launches */
  int64_t trsv_solves;       /* per-problem triangular solve pairs (L y = r, L'x = y) executed */
  int64_t asm_solved;        /* problems finished (and certified) by the active-set pass */
  int64_t asm_rounds;        /* lock-step rounds of the active-set pass */
  int64_t asm_gemm_launches; /* launches of its dominant kernel (gemm_nt_f64_k: LAM * Hinv) */
  double asm_gemm_ms;        /* hipEvent time of those (profiling on) */
  double asm_gemm_flops;     /* algorithmic flops: 2 * columns evaluated * k_max per problem and round (+ one full-width pass) */
  double asm_lambda_ms;      /* hipEvent time of the multiplier-system kernels (asm_lambda_reg*_k, asm_lambda_wg*_k, asm_lambda_tile_k<1>) */
  double asm_update_ms;      /* hipEvent time of the set bookkeeping (asm_count_k, asm_bins_*_k, asm_update_k, asm_wide_k) */
  double asm_lambda_flops;   /* algorithmic fp64 flops of the multiplier systems: sum of m^3/3 + 2 m^2 */
  double asm_lambda_bytes;   /* ... and their algorithmic bytes (gathered Pinv block + rhs/result) */
  double asm_e1max;          /* max |P Kunc + tq| of the verified inverse (nnmpc_qp_set_inverse) */
  double asm_e2max;          /* max |P Pinv - I| */
  int64_t asm_full_checks;   /* finished problems the inverse-error bound could not certify: checked with P itself */
  double asm_lambda32_ms;    /* hipEvent time of the f32 instance of the main multiplier kernel (asm_lambda_reg32_k) alone */
  double asm_lambda64_ms;    /* ... and of the fp64 instance (asm_lambda_reg_k) */
  double asm_lambda32_flops; /* the part of asm_lambda_flops solved in f32 rounds (price it against the f32 MFMA peak) */
  int64_t asm_lambda32_launches, asm_lambda64_launches;
  int64_t asm_far_passes;    /* full-width passes that ran in the far-field form (nnmpc_qp_set_farfield) */
  double asm_side_ms;        /* hipEvent time of the multiplier kernels of the larger sets on the three side streams (they run
                                beside asm_lambda_reg32_k / asm_lambda_reg_k; sum over the streams) */
  int64_t asm_small_passes;  /* segments that went through the one-wave-per-problem kernel of small problems (asm_small_k: padded n <= 724, i.e. n <= 704) */
  int64_t asm_predict_launches; /* launches of the first-set predictor (asm_predict_k) */
  double asm_predict_ms;     /* their hipEvent time (profiling on) */
  double asm_predict_flops;  /* bf16 MFMA flops they executed: 2 * 64 * 512 * (columns of Y in use) per workgroup and iteration */
  int64_t asm_overlapped_passes; /* full-width passes that ran beside the round of the problems still running (asm_overlap) */
  double mult_ms;            /* hipEvent time of the bound-multiplier kernel (asm_mult_k: nnmpc_qp_solve_batch_dual, nnmpc_qp_multipliers; profiling on) */
  int64_t mult_launches;     /* ... and its launches (one per segment) */
  double sens_ms;            /* hipEvent time of the sensitivity kernels (sens_k, both instances: nnmpc_qp_sensitivity; profiling on) */
  int64_t sens_launches;     /* ... and their launches (at most one per instance and segment) */
  int64_t sens_lds_problems; /* problems nnmpc_qp_sensitivity ran in the LDS instance (sets of at most 160 bounds, and the flagged ones); counted always */
  int64_t sens_slab_problems; /* ... and in the slab instance (161 to 768 bounds) */
  double sens_total_ms;      /* hipEvent time of whole nnmpc_qp_sensitivity calls on the handle's stream, the host's sorting between the launches included (profiling on) */
  double adj_ms;             /* hipEvent time of the adjoint kernels (adj_k, both instances: nnmpc_qp_adjoint; profiling on) */
  int64_t adj_launches;      /* ... and their launches (at most one per instance and segment) */
  int64_t adj_lds_problems;  /* problems nnmpc_qp_adjoint ran in the LDS instance (sets of at most 160 bounds, and the flagged ones); counted always */
  int64_t adj_slab_problems; /* ... and in the slab instance (161 to 768 bounds) */
  double adj_total_ms;       /* hipEvent time of whole nnmpc_qp_adjoint calls on the handle's stream, the host's sorting between the launches included (profiling on) */
  int64_t asm_carried;       /* problems whose round was a copy of the corrected multipliers the f32 screen before it had kept for the same set (NNMPC_CARRY) */
  int64_t asm_shared_passes; /* full-width passes beside which a second iteration ran, in the third row space (NNMPC_VIEWS) */
} nnmpc_qp_stats;

const char* nnmpc_last_error(void);

/* P: n x n (only the lower triangle is read, like cvxopt does), tq: n x n_aug,
 * Kunc: n x n_aug warm-start gain (u_unc = Kunc x0 = -P^-1 tq x0) or NULL.
 * n = N * nu (horizon * inputs per stage); bounds are per stage and tiled. */
int nnmpc_qp_create(nnmpc_qp** out, int32_t n, int32_t nu, int32_t n_aug, const double* P,
                    const double* tq, const double* Kunc, const nnmpc_qp_opts* opts);
int nnmpc_qp_destroy(nnmpc_qp* h);

/* x0: B x n_aug, lb/ub: B x nu  ->  u: B x n, active: B x ceil(2n/32) words
 * (bit i = row i of the reference's G: stage k, rows [k*2nu, k*2nu+nu) upper,
 * [k*2nu+nu, (k+1)*2nu) lower), status: B, iters: B x 2 (PDIP iterations,
 * factorisations).  active/status/iters may be NULL. */
int nnmpc_qp_solve_batch(nnmpc_qp* h, int32_t B, const double* x0, const double* lb,
                         const double* ub, double* u, uint32_t* active, int32_t* status,
                         int32_t* iters, int32_t ptr_kind);

/* Same, warm-started: guess (B x n bytes; 0 free, 1 at upper, 2 at lower bound; NULL = cold; a row whose first byte
 * is 255 = no guess for that problem) is the
 * caller's estimate of the active set -- e.g. the previous step's set of a closed-loop chain shifted by
 * one stage (simulate_offline, lib/linearMPC.py:845-866, solves a slowly varying sequence of QPs).
 * The PDIP phase is skipped, the polish starts on the guess; the result is KKT-certified as always. */
int nnmpc_qp_solve_batch_warm(nnmpc_qp* h, int32_t B, const double* x0, const double* lb,
                              const double* ub, const uint8_t* guess, double* u, uint32_t* active,
                              int32_t* status, int32_t* iters, int32_t ptr_kind);

/* Same with a choice of what comes back in u:
 *   NNMPC_OUT_SEQUENCE    u: B x n  -- the whole input sequence DenseQPRegulator.solve returns (lib/linearMPC.py:506-512)
 *   NNMPC_OUT_FIRST_MOVE  u: B x nu -- useq[0:Nu], all that simulate_offline (:856) and control_law (:662-665) keep;
 *                         every problem is still solved and certified over all n variables, only the write-out shrinks
 *                         (3.6 GB -> 26 MB per 100 000 CDU-size problems).
 * guess may be NULL (cold start).  Problems whose inputs hold a NaN / Inf or a bound pair with lb > ub are not solved:
 * status NNMPC_ST_NUMERIC, u = NaN. */
#define NNMPC_OUT_SEQUENCE 0
#define NNMPC_OUT_FIRST_MOVE 1
int nnmpc_qp_solve_batch_ex(nnmpc_qp* h, int32_t B, const double* x0, const double* lb,
                            const double* ub, const uint8_t* guess, double* u, uint32_t* active,
                            int32_t* status, int32_t* iters, int32_t ptr_kind, int32_t out_kind);

/* Bound multipliers of delivered results.  With q = tq x0 and g = P u + q (P as the handle holds it: the lower triangle, mirrored),
 * for problem b and variable i = k nu + c (stage k, input c):
 *     mult[b, i] = -g_i   upper bound of i active (bit k 2nu + c of `active`)        = z of that row of the reference's G
 *     mult[b, i] = +g_i   lower bound active      (bit k 2nu + nu + c)               = z of that row
 *     mult[b, i] = +0.0   variable free
 * i.e. P u + q + z_up - z_lo = 0 on the active rows, and z >= 0 at an optimum.  The side is taken from `active`, never from the sign
 * of the value: a weakly active bound may come back as a tiny negative number (rounding of an fp64 dot product of n + n_aug terms:
 * |error| <= (n + n_aug + 2) 2^-53 (|P_i| |u| + |tq_i| |x0|)).  The values are formed from what was delivered and from P itself --
 * one gathered fp64 row product per active bound (csrc/qp_mult.h) -- not taken from a solver path's own multipliers, so they are the
 * same whichever path solved a problem and need neither an inverse nor far-field factors.
 * x0: B x n_aug, u: B x n, active: B x ceil(2n/32) words, status: B or NULL  ->  mult: B x n, every entry written.
 * A row with status NNMPC_ST_NUMERIC, a non-finite u or both bits of one variable set is no answer: its mult row is quiet NaN
 * throughout.  A row with status NNMPC_ST_MAXITER is computed from what was delivered like any other and is as little certified as
 * its u.  A pure function of the handle's P and tq and the arguments; B = 0: NNMPC_OK, nothing is written. */
int nnmpc_qp_multipliers(nnmpc_qp* h, int32_t B, const double* x0, const double* u, const uint32_t* active,
                         const int32_t* status /* may be NULL */, double* mult, int32_t ptr_kind);
/* nnmpc_qp_solve_batch_ex that also hands back those multipliers (mult: B x n): it solves exactly as nnmpc_qp_solve_batch_ex does --
 * same kernels, same launches, same u / active / status / iters -- and then forms mult from each segment's device-resident u and
 * active words before anything is copied out (a host caller never uploads u again).  active and status may be NULL: the library
 * keeps them in its own workspace (allocated when first asked for, like mult's staging).  mult = NULL: nnmpc_qp_solve_batch_ex.
 * out_kind = NNMPC_OUT_FIRST_MOVE with a non-NULL mult: NNMPC_EINVAL (the whole sequence is not delivered on that path).
 * With a non-NULL mult and NNMPC_DEVICE pointers the call is synchronous: it waits for the handle's stream before it returns, so
 * mult is there (nnmpc_qp_solve_batch_ex only enqueues).  With profiling on, total_ms of such a call includes mult_ms. */
int nnmpc_qp_solve_batch_dual(nnmpc_qp* h, int32_t B, const double* x0, const double* lb, const double* ub,
                              const uint8_t* guess, double* u, uint32_t* active, int32_t* status,
                              int32_t* iters, double* mult, int32_t ptr_kind, int32_t out_kind);

/* Directional derivatives of the solution map (x0, lb, ub) -> u* restricted to a delivered active set.  For problem b, variable
 * i = k nu + c and direction d with perturbations dx0 (n_aug), dlb (nu), dub (nu); A = the variables with a bit set, F = the rest:
 *     du_i = dub_c (upper bit of i set) | dlb_c (lower bit set)            -- copied, bit for bit (a NULL dlb / dub: +0.0)
 *     du_F = -P_FF^-1 (tq_F dx0 + P_FA du_A)
 * evaluated through the inverse on the handle:  t = Kunc dx0,  lam = (Hinv_AA)^-1 (t_A - du_A),  du = t - Hinv[:, A] lam,  so that
 * P du + tq dx0 = 0 on the free rows and = -lam on the active ones.  It equals the directional derivative of u* wherever the set is
 * locally constant (strict complementarity); for a finite step u + du is the exact optimum at the perturbed data as long as it is
 * feasible and mult + dmult >= 0.  One factorisation of Hinv_AA per problem serves all D directions (csrc/qp_sens.h); sets of up
 * to 160 bounds are factored in LDS, up to 768 in a slab of device memory.
 * active: B x ceil(2n/32) words as delivered; status: B or NULL; dx0: B x D x n_aug; dlb, dub: B x D x nu each or NULL (zeros)
 *   ->  du: B x D x n (NNMPC_OUT_SEQUENCE) or B x D x nu (NNMPC_OUT_FIRST_MOVE: the first stage alone, without the two products of
 *       the sequence);  dmult: B x D x n or NULL, the definition of nnmpc_qp_multipliers applied to (dx0, du, active) -- it is linear,
 *       so this is the change of mult, and (du, dmult) satisfies stationarity on the active rows by construction
 *       (NNMPC_OUT_SEQUENCE only: NNMPC_EINVAL with NNMPC_OUT_FIRST_MOVE, as the solves);  flag: B or NULL:
 *       0 computed | 1 more than 768 bounds | 2 no answer: status NNMPC_ST_NUMERIC, both bits of one variable, or a non-finite
 *       perturbation in any of the problem's directions | 3 non-positive pivot of Hinv_AA.  Every row of a problem whose flag is not 0
 *       is quiet NaN throughout (du and dmult); the other problems are not affected.
 * A row with status NNMPC_ST_MAXITER is computed from its delivered set like any other and is as little certified as its u.
 * Needs an accepted inverse (nnmpc_qp_set_inverse; NNMPC_EINVAL without) and no far-field factors.  D < 1, a NULL active, dx0 or du,
 * a bad ptr_kind or out_kind: NNMPC_EINVAL.  B = 0: NNMPC_OK, nothing is written.  Synchronous, and a pure function of the handle's
 * P, tq, Hinv, Kunc and the arguments. */
int nnmpc_qp_sensitivity(nnmpc_qp* h, int32_t B, int32_t D, const uint32_t* active, const int32_t* status, const double* dx0,
                         const double* dlb, const double* dub, double* du, double* dmult, int32_t* flag,
                         int32_t ptr_kind, int32_t out_kind);

/* The adjoint (vector-Jacobian) product of the same map: the transpose of what nnmpc_qp_sensitivity evaluates, on the same delivered
 * active set.  For problem b and cotangent d, v a cotangent of the sequence (n entries; in_kind = NNMPC_OUT_FIRST_MOVE: of the first
 * stage alone, nu entries, the rest zero); A = the variables with a bit set:
 *     w = (Hinv_AA)^-1 (Hinv[A, :] v),      z = v - E_A w  (w subtracted on the active entries),      gx0 = Kunc' z
 *     gbound_i = w_i on A, +0.0 on the free variables         -- the cotangent of each variable's own bound
 *     gub_c = sum { w_i : upper bit of i set, i mod nu = c },   glb_c = sum { w_i : lower bit of i set, i mod nu = c }
 * so that for every direction (dx0, dlb, dub) of nnmpc_qp_sensitivity and its du
 *     <v, du> = <gx0, dx0> + <glb, dlb> + <gub, dub>
 * (with NNMPC_OUT_FIRST_MOVE on both sides: v against the first moves).  One cotangent gives the gradient of a scalar loss of u*
 * with respect to x0 and the bounds; the nu unit cotangents of the first stage give the local feedback gain du0/dx0 (nu x n_aug)
 * of the critical region.  One factorisation of Hinv_AA per problem serves all D cotangents (csrc/qp_adj.h, the factorisation of
 * csrc/qp_sens.h); sets of up to 160 bounds are factored in LDS, up to 768 in a slab of device memory.  Every sum has one order that
 * depends on the problem alone (no atomics): a problem's rows do not depend on its place in the batch.
 * active: B x ceil(2n/32) words as delivered; status: B or NULL; v: B x D x n (NNMPC_OUT_SEQUENCE) or B x D x nu (NNMPC_OUT_FIRST_MOVE:
 * without the two products of the sequence)
 *   ->  gx0: B x D x n_aug;  glb, gub: B x D x nu each or NULL;  gbound: B x D x n or NULL, every entry written;  flag: B or NULL:
 *       0 computed | 1 more than 768 bounds | 2 no answer: status NNMPC_ST_NUMERIC, both bits of one variable, or a non-finite
 *       cotangent in any of the problem's D rows | 3 non-positive pivot of Hinv_AA.  Every row of a problem whose flag is not 0 is quiet
 *       NaN throughout (every output); the other problems are not affected.
 * A row with status NNMPC_ST_MAXITER is computed from its delivered set like any other.  Needs an accepted inverse
 * (nnmpc_qp_set_inverse; NNMPC_EINVAL without) and no far-field factors.  D < 1, a NULL active, v or gx0, a bad ptr_kind or in_kind:
 * NNMPC_EINVAL, nothing is written.  B = 0: NNMPC_OK, nothing is written.  Synchronous, and a pure function of the handle's Hinv,
 * Kunc and the arguments. */
int nnmpc_qp_adjoint(nnmpc_qp* h, int32_t B, int32_t D, const uint32_t* active, const int32_t* status /* may be NULL */,
                     const double* v, double* gx0, double* glb, double* gub, double* gbound, int32_t* flag,
                     int32_t ptr_kind, int32_t in_kind);

/* Enables the shared-inverse active-set pass: Hinv = P^-1 (n x n, fp64), Kunc = -Hinv tq (n x n_aug).
 * All samples share P (reference lib/linearMPC.py:472), so on an active set A the equality-constrained
 * optimum is x = x_unc - Hinv[:,A] lam with lam = (Hinv_AA)^-1 (x_unc,A - b_A): a primal-dual active-set
 * iteration needs no n^3 factorisation.  The inverse is verified once on the device (|P Pinv - I|,
 * |P Kunc + tq|); those bounds certify each result's KKT residual and multiplier signs, results too
 * close to call are re-checked against P itself in fp64, and problems the pass cannot finish go
 * through the PDIP path.  A pair with |P Pinv - I|_max >= 1e-6 (or a NaN in P Kunc + tq) is refused.
 * The call may be repeated on a live handle.  Whatever was derived from the previous pair goes when it starts: an ACCEPTED
 * call releases every far-field factorisation (nnmpc_qp_set_farfield: they were verified against the previous inverse) and
 * queues their windows in nnmpc_qp_farfield_missing again; a REFUSED call leaves the handle without an inverse, without
 * far-field factors and without predictor images -- it solves by the PDIP path alone until a later call is accepted (the
 * statistics keep the refused pair's asm_e1max / asm_e2max). */
int nnmpc_qp_set_inverse(nnmpc_qp* h, const double* Hinv, const double* Kunc);

/* Far-field form of the full-width pass.  A problem whose active set lies inside the leading W variables (the column
 * window of the active-set rounds) has, for the variables beyond,
 *     x[W:] = M [x0 ; lam[0:W]],      M = [Kunc[W:] | -Hinv[W:, 0:W]]      ((n - W) x (n_aug + W)),
 * and M has numerical rank ~Nx: beyond the last active bound the optimum of the reference's condensed problem
 * (lib/linearMPC.py:430-474, terminal penalty = the DARE solution, :356) follows the unconstrained recursion, a linear
 * function of the state at the window's end.  With M = U [Vx | Vl] (r columns; e.g. a truncated SVD, U = U_r S_r) the pass
 * costs 2 r (n_aug + W + n - W) instead of 2 (n_aug + W)(n - W) flops per problem.  U: (n - W) x r, Vx: r x n_aug,
 * Vl: r x W, host, row-major.  The library verifies the factors on the device (max |U [Vx | Vl] - M|, refused above 1e-9,
 * and that bound enters every certificate that rests on them; a problem that bound cannot certify gets its far variables
 * again from Hinv itself, and those -- the ones the check with P then sees -- are the ones delivered).  W must be a multiple of 128 below n; several windows
 * may be set.  Trailing exact zeros in the rows of U shorten the work: a 128-column tile of the pass only multiplies the
 * leading columns of U that any of its rows uses (a basis ordered so that far tiles need few coordinates -- a staircase --
 * pays: the closed loop forgets its fast modes first).  First-move calls (NNMPC_OUT_FIRST_MOVE) additionally skip the
 * 128-column tiles that |x_j| <= |U_j| |T_p| + e_far (|x0|_1 + |lam|_1) <= min_k min(ub_k, -lb_k) - bound_tol certifies feasible
 * (e_far = the verified max |U [Vx | Vl] - M|) -- nothing out there is delivered.  Replacing a window's factors releases the old
 * ones; a refused set leaves nothing behind. */
int nnmpc_qp_set_farfield(nnmpc_qp* h, int32_t W, int32_t r, const double* U, const double* Vx, const double* Vl);
/* *W = a window whose full-width pass had to run in the dense form for want of such factors (0: none left; each window is
 * handed out once per time it is met); the host wrapper factors M for it and calls nnmpc_qp_set_farfield (one-time setup,
 * like the inverse itself).  The library never factors M itself: a caller that binds the C ABI directly -- or drives
 * nnmpc_chain_run -- has to poll this after its calls (at most 16 windows are queued), otherwise its full-width passes stay in
 * the dense form (correct, 2.6 x the flops at the CDU size). */
int nnmpc_qp_farfield_missing(nnmpc_qp* h, int32_t* W);

/* out (B x nu) = u[:, 0:nu] + us for HBM-resident sequences u (B rows of ldu doubles): the absolute first moves, i.e.
 * get_control_sequence's "+ tile(us)" (lib/linearMPC.py:689) restricted to what simulate_offline keeps (:856).
 * us may be NULL.  Device pointers; returns after the kernel has finished. */
int nnmpc_qp_first_moves(const double* u, int64_t ldu, const double* us, int32_t B, int32_t nu, double* out);
int nnmpc_qp_dims(nnmpc_qp* h, int32_t* n, int32_t* nu, int32_t* n_aug);   /* sizes the handle was created with */
int nnmpc_qp_set_profiling(nnmpc_qp* h, int32_t on);
int nnmpc_qp_get_stats(nnmpc_qp* h, nnmpc_qp_stats* out, int32_t reset);

/* Kernel-level test hook: factor K_b = mask_b mask_b' o P + diag(dvec_b) and
 * solve K_b sol_b = rhs_b for b < B <= max_batch (all B x n, host pointers). */
int nnmpc_qp_debug_factor_solve(nnmpc_qp* h, int32_t B, const float* dvec, const float* mask,
                                const float* rhs, float* sol);
/* ... and the per-problem flags of that call (B host int32): 1 = the factorisation of K_b met a non-positive pivot (the pivot is
 * replaced by 1e-30 and the kernels run on: sol_b is then finite or not, but never an answer), 0 otherwise.  In a solve the same
 * flag makes the problem's status NNMPC_ST_NUMERIC. */
int nnmpc_qp_debug_factor_fail(nnmpc_qp* h, int32_t B, int32_t* fail);
/* Kernel-level test hook: the first-set predictor alone.  Does what a solve does up to and including the predictor's launch -- x_unc for
 * the window's columns, the bound states cleared, the extent kernel if asked, the launch itself through the solve's own launch code --
 * whether or not a solve of this size would run the predictor, and hands back the bound states it wrote.  Host pointers,
 * 1 <= B <= the segment size.  NNMPC_EINVAL when the handle has no inverse, no predictor window (n < 512, nu < 4 or > 64,
 * asm_predict_iters < 0), or wide = 1 without the 1024-column window (n < 1024 or nu not a multiple of 4). */
int nnmpc_qp_debug_predict(nnmpc_qp* h, int32_t B, const double* x0, const double* lb, const double* ub,
                           int32_t iters,   /* as opts.asm_predict_iters: 0 adaptive, 1 .. 64 fixed */
                           int32_t wide,    /* 0: 512-column window, 1: 1024-column window, -1: chosen by the extent kernel as a call does */
                           uint8_t* state,  /* out [B][n]: 0 free, 1 upper, 2 lower */
                           int32_t* info,   /* out [4]: W, problems per workgroup, the extent kernel's count (-1 if not run), window chosen (0 / 1) */
                           double* L);      /* out: the step constant of that window, 1.05 lambda_max(D^-1/2 Pinv_WW D^-1/2) */
/* Kernel-level test hook: the GEMM kernels of the active-set path alone, through the launch code of a solve.
 *   C[M x N] = A[M x K] B[N x K]'      row-major, K contiguous in A and B; host pointers; any handle will do.
 * The call uploads A (a_rows rows), B (N rows), C (c_rows rows, ITS CONTENTS included: what a kernel leaves alone comes back as it
 * went in) and the integer arrays into device memory of its own, launches, waits and copies C back.  Of a row only its first K (A, B)
 * or N (C) entries belong to the operand; the last row ends there (so B and C may point into wider arrays).
 * kind 0: what the solves' gemm64() does with these arguments -- the 128 x 128 LDS-DMA kernel when M, N are multiples of 128, K of 16
 *         and there are 200 tiles or more (or a rowmap), else the 64 x 64 kernel (M, N multiples of 64; K is walked in whole chunks of
 *         16, a remainder is dropped).  A rowmap off the 128-grid is refused as in a solve: NNMPC_EINVAL with gemm64's message, nothing
 *         launched, C untouched; the refusal does not stick to the handle (its flag is left as it was found).
 * kind 1 / 2: gemm_nt_f64_t128_k / gemm_nt_f64_k forced (M, N multiples of 128 / 64, K of 16; kind 2 has no rowmap).
 * kind 3 / 4: gemm_nt_f32_kdyn_k<128> / <64> as the end of a round launches them: A, B, C are f32, kdyn is required and holds one bound
 *         per 64 rows (kper 2 / 1); N a multiple of 128 / 64, K of 32; M is the number of rows in use, the grid rounds it up to whole
 *         tiles and A, C and kdyn reach that far.  No rowphase, mdyn, rowmap.
 * For tile edge T (128 / 64) and chunk c (16 fp64, 32 f32):
 *   rowphase [M] : a row tile in which no row has tag `want` is left alone (no entry of C in it is written);
 *   mdyn [1]     : a row tile whose first row is >= *mdyn is left alone; every other tile is written whole, all T rows;
 *   kdyn         : bound on the last non-zero column of A.  kblocks = 0: one entry for the launch; else one per 64 rows, and a row tile
 *                  takes the largest of its T / 64 entries.  The product runs over k < min(K, (bound / c + 1) c); -1: zeros, written;
 *   rowmap [M]   : (128 x 128 kernel) row i of A and of C is row rowmap[i] of the arrays; an entry < 0 or a row >= *mdyn stores nothing.
 * NNMPC_EINVAL, with a message that names this function, for a shape off the kind's grid, a leading dimension shorter than its row
 * or not a multiple of 16 bytes (A, B), kind 3 / 4 without kdyn, null operands, a rowmap entry beyond the arrays. */
int nnmpc_qp_debug_gemm(nnmpc_qp* h, int32_t kind, int32_t M, int32_t N, int32_t K,
                        const void* A, int64_t lda, int64_t a_rows,   /* a_rows, c_rows: rows of the arrays A and C (>= M rounded up to T; */
                        const void* B, int64_t ldb,                   /* with a rowmap: more than its largest entry) */
                        void* C, int64_t ldc, int64_t c_rows,
                        const int32_t* rowphase, int32_t want, const int32_t* kdyn, int32_t kblocks,
                        const int32_t* mdyn, const int32_t* rowmap,   /* each nullable */
                        int32_t* info);   /* out [4]: kernel (1 t128, 2 64 x 64, 3 f32 <128>, 4 f32 <64>; 0 refused), workgroups, kper, tile edge */

/* Structured NN controller.  dims = [d_in, h1, ..., h_{L-1}, nu]; W[l] is
 * dims[l] x dims[l+1] row-major (Keras kernel layout), b[l] has dims[l+1]
 * entries for l < L-1 (the output layer has no bias).  with_uprev selects
 * RegulatorLayerWithUprev (d_in = 2 nx + 2 nu) or WithoutUprev (2 nx + nu).
 * xscale (nx) divides x and xs; NULL = ones.  ulb/uub (nu) clip the output;
 * NULL = no clipping (the Keras layer).
 * use_bf16: 0 = f32 MFMA GEMMs; 1 = bf16 operands with f32 accumulation (~2e-2 relative error on the CDU architecture);
 * 2 = split bf16: activations and weights as pairs hi + lo of bf16 numbers, every layer ONE bf16 GEMM of three times the
 * depth (hi hi' + hi lo' + lo hi'; only lo lo' is dropped): f32-grade results (~1e-5) from the bf16 matrix pipes. */
int nnmpc_nn_create(nnmpc_nn** out, int32_t nlayers, const int32_t* dims,
                    const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                    int32_t with_uprev, const double* xscale, const double* ulb,
                    const double* uub, int32_t use_bf16, int32_t max_batch);
/* The same with the controller's form.  NNMPC_NN_STRUCTURED: nnmpc_nn_create.  NNMPC_NN_UNSTD: the unstructured controller
 * u = clip(MLP([x / xscale, (uprev), xs / xscale, us])) -- ONE pass, no us +, hidden layers relu(W'z + b), linear head WITH a
 * bias: b[nlayers - 1] (nu entries) is required (NeuralNetworkControllerUnstd, lib/controller_evaluation.py:895-916).
 * NNMPC_NN_UNSTD_RELU: the same with relu on the head as well, which is what the Keras UnstdRegulatorLayer computes
 * (lib/LinearMPCLayers.py:147-148).  dims as above (dims[0] = 2 nx + (2 | 1) nu, dims[L] = nu); any other form: NNMPC_EINVAL. */
#define NNMPC_NN_STRUCTURED 0
#define NNMPC_NN_UNSTD 1
#define NNMPC_NN_UNSTD_RELU 2
int nnmpc_nn_create_ex(nnmpc_nn** out, int32_t nlayers, const int32_t* dims,
                       const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                       int32_t with_uprev, const double* xscale, const double* ulb,
                       const double* uub, int32_t use_bf16, int32_t max_batch, int32_t form);
int nnmpc_nn_destroy(nnmpc_nn* h);
/* x, xs: B x nx; uprev (ignored when !with_uprev), us: B x nu; u: B x nu.
 * Non-finite inputs are not rejected and not laundered: a NaN (or an Inf that meets an opposite Inf) in a row of x, uprev, xs
 * or us comes back as non-finite entries of that row of u, as numpy / Keras return them (the ReLU lets a NaN through; the
 * clip keeps it); the other rows of the batch are unaffected.  The NN slots of nnmpc_cl_run behave the same. */
int nnmpc_nn_forward(nnmpc_nn* h, int32_t B, const double* x, const double* uprev,
                     const double* xs, const double* us, double* u, int32_t ptr_kind);
int nnmpc_nn_last_ms(nnmpc_nn* h, double* gemm_ms, double* total_ms);
/* hipEvent time of the hidden-layer GEMM launches of the last forward and their number (bench.py: roofline of the
 * dominant kernel from its own launches; the reference only has time.time() pairs around the whole call,
 * lib/controller_evaluation.py:849-860) */
int nnmpc_nn_last_hidden_ms(nnmpc_nn* h, double* hidden_ms, int32_t* launches);

/* ---- Training step of the structured network, device resident  <-  train_nn_controller (cdu_train.py:40-62): Keras
 * RegulatorModel compiled with Adam + MSE and fit(batch_size, validation_split), here one handle that holds the f32 master
 * weights, the Adam moments, the dataset and every workspace in HBM.  Arithmetic: f32 storage and accumulation on the exact-f32
 * matrix pipes, losses summed in fp64;  pred = us + MLP(pass 1) - MLP(pass 2) without clip,  loss = mean over B nu of
 * (pred - u)^2;  ReLU derivative 0 at 0;  Adam as torch.optim.Adam computes it:
 *     m = m + (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;  W -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * with the bias-correction scalars computed on the host in double.  Every sum has one fixed order (no atomics): results are
 * bit-identical from run to run, and the gradient a step applies is bit-identical to the one nnmpc_train_grad returns.
 * dims / W / b: as nnmpc_nn_create (Keras layout, W_l: dims[l] x dims[l+1], b[nlayers-1] ignored); they become the initial
 * weights and the initial snapshot.  Batches hold at most max_batch rows (the workspaces are sized for it rounded up to 128,
 * the limit itself is not rounded).  lr > 0, 0 <= beta1, beta2 < 1, eps > 0 (NNMPC_EINVAL otherwise).
 * Non-finite data are not rejected and not hidden: a NaN in a row gives a NaN loss and NaN weights, as in torch.
 * Environment: NNMPC_TRAIN_DW_SLICES=n (read by create) forces n row slices of the weight-gradient reduction (tests). */
typedef struct nnmpc_train nnmpc_train;
int nnmpc_train_create(nnmpc_train** out, int32_t nlayers, const int32_t* dims,
                       const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                       int32_t with_uprev, int32_t max_batch, double lr, double beta1, double beta2,
                       double eps);
/* The same with the network's form, the values nnmpc_nn_create_ex takes  <-  train_nn_controller of cstrs_train_unstd.py:24-57
 * (Keras UnstdRegulatorModel compiled with Adam + MSE).  NNMPC_NN_STRUCTURED: nnmpc_train_create.  NNMPC_NN_UNSTD:
 * pred = MLP([x, (uprev), xs, us]) -- ONE pass (a batch is Bp stacked rows, not 2 Bp), no us +, a linear head WITH a bias:
 * b[nlayers - 1] (nu entries) is required here and is read and written by get_weights, set_weights and grad like every other
 * bias.  NNMPC_NN_UNSTD_RELU: relu on the head as well (the Keras layer as written, lib/LinearMPCLayers.py:147-148); its
 * derivative is 0 where the prediction is <= 0.  Everything else (dataset, Adam, sums in one fixed order) as above.  Any
 * other form, or a missing head bias: NNMPC_EINVAL. */
int nnmpc_train_create_ex(nnmpc_train** out, int32_t nlayers, const int32_t* dims,
                          const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                          int32_t with_uprev, int32_t max_batch, double lr, double beta1,
                          double beta2, double eps, int32_t form);
int nnmpc_train_destroy(nnmpc_train* h);
/* The dataset, n rows as _get_data_for_training leaves them (already scaled): x, xs n x nx; uprev (NULL unless with_uprev),
 * us, u n x nu.  Converted to f32 and kept in HBM; replaces an earlier dataset.  A with-uprev network without uprev: NNMPC_EINVAL. */
int nnmpc_train_set_data(nnmpc_train* h, int32_t n, const double* x, const double* uprev,
                         const double* xs, const double* us, const double* u, int32_t ptr_kind);
/* Loss and gradient of the batch made of dataset rows rows[0..B) (host pointer), no update.  gW[l]: dims[l] x dims[l+1],
 * gb[l]: dims[l+1] for l < nlayers - 1, and for the head too in the unstructured forms (Keras layout; NULL entries and NULL
 * lists are skipped).  B > max_batch or a row
 * index outside [0, n): NNMPC_EINVAL before any launch (also for step and epoch).  rows / perm are copied into a pinned
 * buffer of the handle before the call returns: the caller may reuse or free them at once, also after a step without loss. */
int nnmpc_train_grad(nnmpc_train* h, int32_t B, const int32_t* rows, double* loss,
                     double* const* gW, double* const* gb);
/* One Adam update on that batch.  loss == NULL: enqueued without waiting for the device. */
int nnmpc_train_step(nnmpc_train* h, int32_t B, const int32_t* rows, double* loss);
/* Every step of an epoch back to back: batches perm[0..batch), perm[batch..2 batch), ... (the last one is the short one),
 * one upload of perm, one wait at the end; *loss = sum_i loss_i rows_i / nrows, accumulated on the device. */
int nnmpc_train_epoch(nnmpc_train* h, int32_t nrows, const int32_t* perm, int32_t batch,
                      double* loss);
/* Forward only: mean squared error over dataset rows [first, first + count) (the validation loss). */
int nnmpc_train_eval(nnmpc_train* h, int32_t first, int32_t count, double* mse);
/* Keras layout, the f32 master weights as doubles; set_weights keeps the moments and the step count. */
int nnmpc_train_get_weights(nnmpc_train* h, double* const* W, double* const* b);
int nnmpc_train_set_weights(nnmpc_train* h, const double* const* W, const double* const* b);
/* Device-side copy of the current weights (ModelCheckpoint(save_best_only=True)) / back; the moments are not part of it. */
int nnmpc_train_snapshot(nnmpc_train* h);
int nnmpc_train_restore(nnmpc_train* h);
/* hipEvent times of the last grad / step / epoch / eval (waits for it): the whole call on the device, and the spans of its
 * forward GEMMs and of its backward pass (dW, bias column sums, dA). */
int nnmpc_train_last_ms(nnmpc_train* h, double* gemm_ms, double* total_ms);
/* Row slices of the dW reduction per layer (nlayers entries) in the last backward pass. */
int nnmpc_train_dw_slices(nnmpc_train* h, int32_t* slices);
/* Largest |entry| over the padding rows and columns of every weight, bias and moment image (a NaN there: NaN).  The
 * padding has zero gradients by construction and must stay exactly zero through updates; this is the check. */
int nnmpc_train_padding_max(nnmpc_train* h, double* maxabs);
/* The tangent loss (Sobolev training)  <-  train_nn_controller's targets are MPC solves (cdu_train.py:40-62), and inside a
 * critical region the MPC law is affine: a sample carries a slope as well as a value, and nnmpc_qp_sensitivity delivers it
 * (du0 along a direction).  A handle built here trains the structured network on both:
 *     L = mean over B nu of (pred - u)^2  +  w mean over B nu of (J d - t)^2,
 * d = [dx, (duprev)] one direction per dataset row in the units of the dataset's x, t (nu entries) the target, J d the tangent of
 * pred along d, propagated forward through the same weights: a'_0 = [dx, (duprev), 0, 0], a'_l = (a'_{l-1} W_l) * [a_l(pass 1) > 0],
 * J d = a'_{L-1} W_L -- no bias, ReLU derivative 0 at 0; pass 2 does not depend on x or uprev.  The masks are constants of the
 * backward pass (ReLU has no second derivative), so the gradient is the one autograd gives.  Arguments as nnmpc_train_create_ex;
 * form must be NNMPC_NN_STRUCTURED (anything else: NNMPC_EINVAL before a device is looked for).  Workspaces for 3 stacked row
 * blocks of max_batch rows.  The weight w is 0 after create, and with w == 0 every call runs the plain step: the bytes of an
 * nnmpc_train_create handle.  With w > 0 a step keeps the plain step's number of launches and its fixed summation orders. */
int nnmpc_train_create_tan(nnmpc_train** out, int32_t nlayers, const int32_t* dims,
                           const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                           int32_t with_uprev, int32_t max_batch, double lr, double beta1,
                           double beta2, double eps, int32_t form);
/* The directions and targets of the dataset nnmpc_train_set_data gave, one per row (train.tangent_data makes them from a solved
 * batch): dx n x nx, duprev n x nu (NULL unless with_uprev), t n x nu, f64 on the host or in HBM, converted to f32 and kept.
 * A plain handle, no dataset yet, n != the dataset's rows, or a with-uprev network without duprev: NNMPC_EINVAL.  A later
 * nnmpc_train_set_data drops them.  Non-finite entries are not rejected and not hidden: a NaN gives a NaN tan_mse and L. */
int nnmpc_train_set_tangents(nnmpc_train* h, int32_t n, const double* dx, const double* duprev,
                             const double* t, int32_t ptr_kind);
/* The tangent loss with several directions per row, and over the whole network input.
 *   dirs = D directions per dataset row, each with its own target: both means of L run over B D nu, and a batch stacks the D
 *     tangent blocks behind ONE primal pair, (2 + D) Bp rows instead of the 3 D Bp of a dataset that repeats each row D times.
 *   whole_input = 1: a direction is d = [dx, (duprev), dxs, dus].  pred = us + N(x, uprev, xs, us) - N(xs, us, xs, us) depends on
 *     xs and us through both passes, so pass 2 carries tangents too, a''_0 = [dxs, (dus), dxs, dus] under the masks of pass 2, and
 *     J d = dus + (a'_{L-1} W_L - a''_{L-1} W_L) in f32 in that order: (2 + 2D) Bp stacked rows.  The matching target is the
 *     change of the MPC's absolute first move, dus + du0 along train.whole_input_perturbation (nnmpc_qp_sensitivity with dlb / dub).
 * Everything else as nnmpc_train_create_tan, which is dirs = 1, whole_input = 0 (such a handle computes its bytes).  dirs
 * outside 1 .. NNMPC_TAN_MAX_DIRS, whole_input neither 0 nor 1, or form != NNMPC_NN_STRUCTURED: NNMPC_EINVAL before a device
 * is looked for.  set_tan_weight, grad, step, epoch, eval, last_losses and last_ms serve the handle with their meaning there;
 * a step keeps its 6 nlayers launches. */
#define NNMPC_TAN_MAX_DIRS 16
int nnmpc_train_create_tan_ex(nnmpc_train** out, int32_t nlayers, const int32_t* dims,
                              const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                              int32_t with_uprev, int32_t max_batch, double lr, double beta1,
                              double beta2, double eps, int32_t form, int32_t dirs, int32_t whole_input);
/* nnmpc_train_set_tangents for such a handle: dx n x dirs x nx, duprev n x dirs x nu (NULL unless with_uprev), dxs n x dirs x nx
 * and dus n x dirs x nu (required on a whole-input handle, NULL otherwise), t n x dirs x nu.  NNMPC_EINVAL: dirs differs from
 * the handle's, a plain handle, no dataset yet, n != the dataset's rows, a with-uprev network without duprev, dxs / dus
 * missing on a whole-input handle or given on another.  nnmpc_train_set_tangents itself serves only a handle with dirs == 1
 * and whole_input == 0; on any other tangent handle it returns NNMPC_EINVAL and names this function.  Non-finite entries are
 * not rejected and not hidden. */
int nnmpc_train_set_tangents_ex(nnmpc_train* h, int32_t n, int32_t dirs, const double* dx,
                                const double* duprev, const double* dxs, const double* dus,
                                const double* t, int32_t ptr_kind);
/* The weight w of the tangent term: finite and >= 0, on a tangent handle (NNMPC_EINVAL otherwise).  With w > 0 and no
 * tangents, grad, step, epoch and eval return NNMPC_EINVAL before any launch. */
int nnmpc_train_set_tan_weight(nnmpc_train* h, double w);
/* The two parts of what the last grad / step (that batch), epoch (row-weighted means) or eval (over its rows) returned
 * (waits for it): grad, step and epoch return L = mse + w tan_mse, and so does eval.  With w == 0, and on a plain handle,
 * mse is that loss and tan_mse 0.  Before the first such call: NNMPC_EINVAL. */
int nnmpc_train_last_losses(nnmpc_train* h, double* mse, double* tan_mse);

/* ---- A sweep of networks trained in lock step  <-  the loop `for (regulator_dim, num_sample) in
 * itertools.product(regulator_dims, num_samples)` around train_nn_controller (cstrs_train.py / cdu_train.py main): G networks
 * in ONE handle, every layer of every network in one launch (one per tile class present) instead of G.  All members share nx,
 * nu, with_uprev, the depth, max_batch, the Adam parameters and one dataset; they differ in widths, weights, rows, step count
 * and snapshot.  Arithmetic, padding, validation and error codes are nnmpc_train's, and so are the bytes: a member's weights
 * and losses do not depend on the rest of the group and equal what an nnmpc_train handle computes from the same weights and
 * rows (same tile functions, same summation orders, dW slices from the member's own shape).
 * dims: G x (nlayers + 1), member after member; W, b: G x nlayers pointers (b of a member's last layer is ignored: the
 * structured head has no bias; nnmpc_train_create_group_ex builds the groups whose head has one).  Replaces
 * G calls of nnmpc_train_create.  G < 1, or a member whose dims[0] / dims[L] disagree with nx, nu: NNMPC_EINVAL. */
typedef struct nnmpc_train_group nnmpc_train_group;
int nnmpc_train_group_create(nnmpc_train_group** out, int32_t G, int32_t nlayers, const int32_t* dims,
                             const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                             int32_t with_uprev, int32_t max_batch, double lr, double beta1,
                             double beta2, double eps);
int nnmpc_train_group_destroy(nnmpc_train_group* h);
/* The same with the members' form, the values nnmpc_train_create_ex takes: ONE form per group (a sweep that mixes forms is one
 * group per form, as it is one group per depth)  <-  the loop of cstrs_train.py run with the comparison network of
 * cstrs_train_unstd.py.  NNMPC_NN_STRUCTURED: nnmpc_train_group_create.  NNMPC_NN_UNSTD / NNMPC_NN_UNSTD_RELU: every member is
 * the one-pass network of nnmpc_train_create_ex with a bias on the head (and relu on it): b[g * nlayers + nlayers - 1] (nu entries)
 * is required for every member and is read and written by nnmpc_train_group_get_weights / _set_weights like every other bias; a
 * lock-step step is 6 nlayers + 2 launches (the head's bias column sums and bias update) against 6 nlayers.  A member's bytes
 * equal those of an nnmpc_train_create_ex handle of that form.  Every other nnmpc_train_group_* function serves both.  Any other
 * form, or a member without a head bias in an unstructured form: NNMPC_EINVAL, the message names the member. */
int nnmpc_train_create_group_ex(nnmpc_train_group** out, int32_t G, int32_t nlayers, const int32_t* dims,
                                const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                                int32_t with_uprev, int32_t max_batch, double lr, double beta1,
                                double beta2, double eps, int32_t form);
/* The shared dataset, as nnmpc_train_set_data takes it (what _get_data_for_training(num_samples = the largest) hands the
 * sweep; member g then uses rows [0, n_g)).  Replaces G uploads. */
int nnmpc_train_group_set_data(nnmpc_train_group* h, int32_t n, const double* x,
                               const double* uprev, const double* xs, const double* us,
                               const double* u, int32_t ptr_kind);
/* One epoch of every member, replacing G calls of nnmpc_train_epoch: perm holds the members' row lists one after another,
 * nrows[g] entries for member g.  Member g runs ceil(nrows[g] / batch) lock-step steps (its last batch is the short one) and
 * then sits out; nrows[g] == 0: the member skips the epoch (weights, moments and step count untouched, loss[g] = NaN).
 * loss[g]: the row-weighted mean of the member's step losses, accumulated on the device.  One upload, one wait.
 * batch > max_batch, a row index outside [0, n), no dataset: NNMPC_EINVAL before any launch. */
int nnmpc_train_group_epoch(nnmpc_train_group* h, const int32_t* nrows, const int32_t* perm,
                            int32_t batch, double* loss);
/* Forward only, replacing G calls of nnmpc_train_eval: mse[g] over dataset rows [first[g], first[g] + count[g]) in chunks
 * of max_batch rows; count[g] == 0: skipped (mse[g] = NaN). */
int nnmpc_train_group_eval(nnmpc_train_group* h, const int32_t* first, const int32_t* count,
                           double* mse);
/* Member g's weights as nnmpc_train_get_weights / nnmpc_train_set_weights exchange them: in a group of an unstructured form
 * b[nlayers - 1] is the head's bias (required by set_weights), in a structured group it is ignored. */
int nnmpc_train_group_get_weights(nnmpc_train_group* h, int32_t g, double* const* W,
                                  double* const* b);
int nnmpc_train_group_set_weights(nnmpc_train_group* h, int32_t g, const double* const* W,
                                  const double* const* b);
/* nnmpc_train_snapshot / nnmpc_train_restore for the members with mask[g] != 0 (per-member
 * ModelCheckpoint(save_best_only=True)); one device-side copy per member. */
int nnmpc_train_group_snapshot(nnmpc_train_group* h, const int32_t* mask);
int nnmpc_train_group_restore(nnmpc_train_group* h, const int32_t* mask);
/* nnmpc_train_padding_max over every member. */
int nnmpc_train_group_padding_max(nnmpc_train_group* h, double* maxabs);
/* nnmpc_train_last_ms for the last epoch / eval of the group. */
int nnmpc_train_group_last_ms(nnmpc_train_group* h, double* gemm_ms, double* total_ms);
/* Kernel launches the last epoch / eval enqueued (counted where they are launched): what a loop over G handles multiplies by G. */
int nnmpc_train_group_last_launches(nnmpc_train_group* h, int64_t* n);
/* The tangent loss of nnmpc_train_create_tan for a sweep: a structured group whose members each carry their OWN weight
 * w[g] >= 0 of the tangent term; one set of tangents is shared, as the dataset is.  Arguments as nnmpc_train_create_group_ex;
 * form must be NNMPC_NN_STRUCTURED (anything else: NNMPC_EINVAL before a device is looked for).  Workspaces for 3 stacked row
 * blocks of max_batch rows per member.  Every weight is 0 after create.  In a lock-step step a member with w[g] > 0 stacks
 * 3 Bp rows, a member with w[g] == 0 the plain 2 Bp; the step keeps its 6 nlayers launches whatever the mix.  A member's bytes
 * do not depend on the rest of the group: with w[g] > 0 its weights and losses (L, mse, tan_mse) equal those of an
 * nnmpc_train_create_tan handle at that weight fed the same rows, with w[g] == 0 those of an nnmpc_train_create handle, which
 * are those of a member of a plain group.  Every nnmpc_train_group_* function serves the handle. */
int nnmpc_train_create_group_tan(nnmpc_train_group** out, int32_t G, int32_t nlayers, const int32_t* dims,
                                 const double* const* W, const double* const* b, int32_t nx, int32_t nu,
                                 int32_t with_uprev, int32_t max_batch, double lr, double beta1,
                                 double beta2, double eps, int32_t form);
/* nnmpc_train_set_tangents for the group's shared dataset, with its errors: a plain group, no dataset yet, n != the dataset's
 * rows, a with-uprev group without duprev: NNMPC_EINVAL.  A later nnmpc_train_group_set_data drops them. */
int nnmpc_train_set_group_tangents(nnmpc_train_group* h, int32_t n, const double* dx,
                                   const double* duprev, const double* t, int32_t ptr_kind);
/* The members' weights, G entries, each finite and >= 0 (NNMPC_EINVAL names the member; nothing is changed); a plain group:
 * NNMPC_EINVAL.  With any w[g] > 0 and no tangents, nnmpc_train_group_epoch and _eval return NNMPC_EINVAL before any launch.
 * They return L = mse + w[g] tan_mse where they return the plain group's loss. */
int nnmpc_train_set_group_tan_weights(nnmpc_train_group* h, const double* w);
/* nnmpc_train_last_losses per member (G entries each, either may be NULL): the two parts of what the last epoch (row-weighted
 * means) or eval (over its rows) returned.  A member with w[g] == 0, and any member of a plain group: mse is that loss and
 * tan_mse 0.  A member without rows in that call: both NaN.  Before the first epoch or eval: NNMPC_EINVAL. */
int nnmpc_train_last_group_losses(nnmpc_train_group* h, double* mse, double* tan_mse);

/* ---- Lock-step closed-loop chains, device resident  <-  simulate_offline (lib/linearMPC.py:827-880), one OS process
 * per chain in the reference (:814-825).  All nc chains of a task advance together; per step (loop :845-866):
 *     x0 = [x - xs; uprev - us], bounds ulb - us / uub - us   (get_control_sequence :682-689)
 *     regulator QP for all chains in ONE batched solve, warm-started on the previous step's active set shifted by one
 *     stage; ut = useq[0:Nu] + us (:856, :689);  x+ = A x + B ut + Bd d (:860);  uprev+ = ut
 * State (x, uprev), the target pairs (xs, us) and disturbances d of ALL T steps and the recorded trajectories stay in
 * HBM; the host sees nothing until nnmpc_chain_run returns.  Records are [T][nc][.] like the arrays the reference
 * saves per chain (:868-872) with the chain index in the middle. */
typedef struct nnmpc_chain nnmpc_chain;
/* A: nx x nx, B: nx x nu, Bd: nx x nd (row-major, host); ulb/uub: nu; x0: nx, uprev0: nu (every chain starts there,
 * :808-813).  qp: the regulator handle (n_aug = nx + nu); it is borrowed, not owned. */
int nnmpc_chain_create(nnmpc_chain** out, nnmpc_qp* qp, int32_t nc, int32_t nx, int32_t nu, int32_t nd,
                       const double* A, const double* B, const double* Bd, const double* ulb,
                       const double* uub, const double* x0, const double* uprev0);
int nnmpc_chain_destroy(nnmpc_chain* c);
/* xs: T x nc x nx, us: T x nc x nu, d: T x nc x nd  ->  x_rec: T x nc x nx, uprev_rec, u_rec: T x nc x nu (state and
 * previous input BEFORE the move of step t, and that move), status: T x nc, all host or all device (ptr_kind).
 * The chain state carries over between calls (T steps at a time); nnmpc_chain_reset puts every chain back to (x0, uprev0).
 * warm_start = 0 solves every step cold (same results: every solve is certified). */
int nnmpc_chain_run(nnmpc_chain* c, int32_t T, const double* xs, const double* us, const double* d,
                    double* x_rec, double* uprev_rec, double* u_rec, int32_t* status,
                    int32_t warm_start, int32_t ptr_kind);
int nnmpc_chain_reset(nnmpc_chain* c);
/* hipEvent time of the last nnmpc_chain_run and the part of it spent inside the regulator solves */
int nnmpc_chain_last_ms(nnmpc_chain* c, double* total_ms, double* solve_ms);

/* ---- Steady-state target problems, batched  <-  TargetSelector.solve -> cvxopt.solvers.qp(P, q, G, h, A, b)
 * (lib/linearMPC.py:298-311), the other QP of every simulation step (:851).  With F = [I - A; H C] of full column rank
 * the equalities [I - A, -B; HC, 0][xs; us] = b (:262-266) fix xs = Xb b + Xu us and leave nz = Nz equalities E us = Eb b
 * on the inputs, so each (ysp, dhat) pair is the small QP
 *     min 1/2 us' Pr us + (Qb b + Qy y + q0)' us   s.t.  E us = Eb b,  ulb <= us <= uub          (nu variables)
 * with b = tb [ysp; dhat], y = ysp - Cd dhat; the shared matrices are formed once on the host (fp64).  One wave per
 * problem: primal-dual active-set iterations on the KKT system of the free inputs and the equalities (<= nu + nz
 * unknowns, Gaussian elimination with partial pivoting in LDS), fp64 throughout, KKT-certified.
 *
 * Multipliers: Pr us + q + E' lam_eq + mu_ub - mu_lb = 0 with mu_ub, mu_lb >= 0 (mu_ub only where active = 1, mu_lb only
 * where active = 2): lam_eq carries the sign of "+ E' lam_eq" in the gradient of the Lagrangian.
 * Bounds: an input flagged active (1 / 2) equals its bound bitwise; a free input (0) satisfies ulb - 1e-9 <= us <= uub + 1e-9:
 * the feasibility slack of this solver is the fixed 1e-9 (absolute, in the units of us; bound_tol of nnmpc_qp_opts belongs to
 * the regulator only).  A bound met within the slack (weakly active, multiplier 0) may come back in either state.
 * Status per problem: NNMPC_ST_OPTIMAL = KKT point, certified; NNMPC_ST_NUMERIC = no answer -- a NaN / Inf in q or e, some
 * ulb_i > uub_i or a NaN bound (then every problem of the handle), E without full row rank (a repeated or a zero row, nz > the
 * number of inputs), or NO point of the box satisfies E us = e (infeasible: an unreachable setpoint): us = NaN, active = 0;
 * NNMPC_ST_MAXITER = the 600 steps ran out or the final certificate failed: us is the last iterate, not certified.
 * Scaling: the rows of E are equilibrated against Pr by powers of two when the handle is created (lam_eq is returned in the
 * caller's units), so (Pr, q) -> beta (Pr, q) and (E, e) -> alpha (E, e) change nothing but rounding: solved with
 * max|Pr| / max|E| from 1e-16 to 1e17 (tests/test_target_kernel_gpu.py; before the equilibration every problem beyond
 * about 1e6 was refused as NNMPC_ST_NUMERIC). */
typedef struct nnmpc_ts nnmpc_ts;
/* Pr: nu x nu (symmetric positive definite), E: nz x nu (full row rank, so nz <= nu), lb/ub: nu.  nu >= 1, nz >= 0 and
 * nu + nz <= 64 -- the KKT system of a step sits on the 64 lanes of one wave; that is the only size limit (NNMPC_EINVAL beyond). */
int nnmpc_ts_create(nnmpc_ts** out, int32_t nu, int32_t nz, const double* Pr, const double* E,
                    const double* lb, const double* ub);
int nnmpc_ts_destroy(nnmpc_ts* h);
/* q: B x nu, e: B x nz (may be NULL when nz = 0)  ->  us: B x nu, lam_eq: B x nz (multipliers of the equalities in the
 * convention above, may be NULL), active: B x nu bytes (0 free / 1 at uub / 2 at ulb, may be NULL), status: B (NNMPC_ST_*).
 * The problems of a batch are independent: a row's outputs do not depend on its position or its neighbours.  B = 0: NNMPC_OK,
 * nothing is written. */
int nnmpc_ts_solve_batch(nnmpc_ts* h, int32_t B, const double* q, const double* e, double* us,
                         double* lam_eq, uint8_t* active, int32_t* status, int32_t ptr_kind);

/* ---- Lock-step closed-loop evaluation  <-  online_simulation (lib/linearMPC.py:703-718) with LinearMPCController.control_law
 * (:646-701), NeuralNetworkController (lib/controller_evaluation.py:841-892), SatDlqrController / SteadyStateController
 * (:918-1087), one (controller, scenario, noise seed) per call in the reference (_simulate_scenarios / _simulate_neural_networks,
 * :322-523).  All nb instances advance together; plant, estimator, running cost and records stay in HBM.  Per step t:
 *   filter   xp = Aaug xhat + Baug uprev,  xhat = xp + L (y_t - Caug xp) = [x^; d^]                          (:133-176, :646-650)
 *   target   b = tb [ysp_t; d^],  q = Qb b + Qy (ysp_t - Cd d^) + q0,  e = Eb b,  us = the reduced target QP (nnmpc_ts),
 *            xs = Xb b + Xu us                                                                                 (:298-311)
 *   control  MPC: first move of the regulator QP at [x^ - xs; uprev - us], bounds ulb - us / uub - us, + us (:682-689), warm-
 *            started on the instance's previous active set shifted by one stage;  NN: clip(us + NN(x^, uprev, xs, us) -
 *            NN(xs, us, xs, us)) (:863-892);  SATDLQR: clip(Kaug [x^ - xs; uprev - us] + us) (:1003-1005);  US: us (:1076);
 *            NN_UNSTD: clip(NN(x^, uprev, xs, us)), one pass, head with a bias (:895-916)
 *   cost     z = [x^ - xs; uprev - us], w = u - us, ell = z'Qaug z + w'Raug w + z'Maug w + w'Maug'z,
 *            avg_{t+1} = (avg_t t + ell) / (t + 1), t counted from create / reset (not from this call: a chunked run
 *            continues the mean of the chunks before it)                                                       (:691-701)
 *   plant    uprev = u,  x = A x + B u + Bp p_t,  y_{t+1} = C x + sigma o v_{t+1}                               (:87-131)
 * Nothing random runs on the device: v holds the standard-normal draws of every instance. */
typedef struct nnmpc_cl nnmpc_cl;
#define NNMPC_CL_MPC 0
#define NNMPC_CL_NN 1
#define NNMPC_CL_SATDLQR 2
#define NNMPC_CL_US 3
#define NNMPC_CL_NN_UNSTD 4     /* clip(NN(x^, uprev, xs, us)): one pass, head with a bias (lib/controller_evaluation.py:895-916) */
/* Shared model data (fp64, row-major, host), na = nx + nd, nb_ = nx + nz:
 *   plant   A nx x nx, B nx x nu, C ny x nx, Bp nx x nd
 *   filter  Aaug na x na, Baug na x nu, Caug ny x na, L na x ny (steady-state gain, dlqe)
 *   target  tb nb_ x (ny + nd), Qb nu x nb_, Qy nu x ny, q0 nu, Cd ny x nd, Eb nz x nb_, Xb nx x nb_, Xu nx x nu
 *           (target.ReducedTargetProblem; the QP itself is the borrowed nnmpc_ts handle, created with nu, nz)
 *   cost    Qaug (nx + nu)^2, Raug nu x nu, Maug (nx + nu) x nu
 *   bounds  ulb, uub (nu);  initial values x0 (nx), xhat0 (na), uprev0 (nu) shared by every instance
 * Bp and Cd may be NULL when nd = 0, Eb when nz = 0 (dist of nnmpc_cl_run too when nd = 0); every other pointer is required. */
typedef struct {
  int32_t nx, nu, ny, nd, nz;
  const double *A, *B, *C, *Bp;
  const double *Aaug, *Baug, *Caug, *L;
  const double *tb, *Qb, *Qy, *q0, *Cd, *Eb, *Xb, *Xu;
  const double *Qaug, *Raug, *Maug;
  const double *ulb, *uub, *x0, *xhat0, *uprev0;
} nnmpc_cl_model;
/* One controller of the evaluation.  MPC: qp = the borrowed regulator handle (n_aug = nx + nu; any horizon).  NN: dims / W / b
 * as nnmpc_nn_create (copied to HBM in f32; hidden widths <= 2048), with_uprev, xscale (nx, NULL = ones).  SATDLQR: Kaug
 * (nu x (nx + nu)).  US: nothing.  NN_UNSTD: the fields of NN; b has nlayers entries, all required (the head's bias too). */
typedef struct {
  int32_t kind;
  nnmpc_qp* qp;
  int32_t nlayers;
  const int32_t* dims;
  const double* const* W;
  const double* const* b;
  int32_t with_uprev;
  const double* xscale;
  const double* Kaug;
} nnmpc_cl_slot;
/* inst_slot: nb slot indices, non-decreasing (the instances of a slot are contiguous; the host wrapper sorts and un-sorts) */
int nnmpc_cl_create(nnmpc_cl** out, const nnmpc_cl_model* m, nnmpc_ts* ts, int32_t nslots, const nnmpc_cl_slot* slots,
                    int32_t nb, const int32_t* inst_slot);
int nnmpc_cl_destroy(nnmpc_cl* h);
/* T steps.  setpoints: nscen x T x ny, dist: nscen x T x nd (this call's rows of every scenario), scen: nb scenario indices,
 * v: (T + 1) x nb x ny standard-normal draws -- row 0 gives y_0 = C x0 + sigma o v_0 on the first call after create / reset and
 * is ignored otherwise (a chunked run passes rows [t0, t0 + T] of the whole draw), row t + 1 the noise of y_{t+1}; sigma: ny
 * (sqrt(diag(Rv))).  y0 (nb x ny, may be NULL): the first measurement of every instance instead of C x0 + sigma o v_0 (row 0 of
 * v is then unused) -- the reference's evaluation scripts load a plant whose y[0] was drawn when it was pickled and seed the
 * noise afterwards (_simulate_scenarios, lib/controller_evaluation.py:353-360).  Records (NULL = not recorded): y_rec, x_rec, xhat_rec, avg_rec (T + 1) x nb x {ny, nx, na, 1} (row 0 = the
 * state at the start of the call); u_rec, xs_rec, us_rec T x nb x {nu, nx, nu}; ts_status, reg_status T x nb (NNMPC_ST_*;
 * reg_status is 0 for other kinds).  All host or all device (ptr_kind).  The state carries over between calls. */
int nnmpc_cl_run(nnmpc_cl* h, int32_t T, int32_t nscen, const double* setpoints, const double* dist, const int32_t* scen,
                 const double* v, const double* sigma, const double* y0, double* y_rec, double* x_rec, double* xhat_rec, double* u_rec,
                 double* xs_rec, double* us_rec, double* avg_rec, int32_t* ts_status, int32_t* reg_status, int32_t ptr_kind);
/* every instance back to (x0, xhat0, uprev0), avg = 0, step 0, no warm start */
int nnmpc_cl_reset(nnmpc_cl* h);
/* hipEvent times of the last run: total; phase_ms[6] summed over its steps = filter + target reduction, target QP, expansion
 * and controller inputs (incl. SATDLQR / US), grouped NN forward, MPC solves (to the last slot's end), clip + cost + plant;
 * slot_step_ms (T x nslots, may be NULL): each step's controller phase of each slot for the whole batch (MPC: its solve,
 * NN: the grouped forward, SATDLQR / US: the expansion kernel).  The phase events of at most 256 steps are alive at a time: a
 * longer run drains its stream once per 256 steps to add them up, so the handle holds (7 + MPC slots, + 1 with the nonlinear
 * plant) x 256 + 2 events at most. */
int nnmpc_cl_last_ms(nnmpc_cl* h, double* total_ms, double* phase_ms, double* slot_step_ms);
/* ---- Nonlinear plant of the closed loop: the CSTRs-with-flash plant of the reference's study (cstrs_parameters.py,
 * NonlinearPlantSimulator, lib/nonlinearMPC.py:11-48).  Its 12-state ODE is integrated over each sample by classical RK4 with
 * `substeps` fixed steps in fp64 (the host's nonlinearMPC.DiscreteSimulator: same tableau, same substeps), in deviation
 * variables: states x (12) about xs, inputs u (6) scaled, U = u o uscale + us, disturbances p (5), P = p o pscale + ps.
 * Parameter block (NNMPC_CSTRS_NPAR doubles, in this order):
 *   [0..16]  alphaA alphaB alphaC pho Cp Ar Am Ab kr km kb delH1 delH2 EbyR k1star k2star Td   (cstrs_parameters.CONSTANTS)
 *   [17..28] xs (the rectified steady state), [29..34] us, [35..39] ps, [40..45] uscale, [46..50] pscale
 * All finite; pho, Cp, Ar, Am, Ab > 0; sample_time > 0; 1 <= substeps <= 4096 (NNMPC_EINVAL otherwise).  A level that goes
 * non-positive makes that instance's state NaN from then on (no clamping, no data-dependent loop count). */
#define NNMPC_CL_PLANT_LINEAR 0
#define NNMPC_CL_PLANT_CSTRS_FLASH 1
#define NNMPC_CSTRS_NPAR 51
/* Plant of a closed-loop handle: NNMPC_CL_PLANT_LINEAR (the default; par may be NULL) or NNMPC_CL_PLANT_CSTRS_FLASH (the
 * handle must have nx = 12, nu = 6, nd = 5).  With the nonlinear plant a step's plant part is x = Phi(x, u_t, p_t) and
 * y_{t+1} = C x + sigma o v_{t+1} with the model's C (diag(1 / yscale)); the model's A, B, Bp (the linearisation) are not
 * used for the plant.  Phase "post" of nnmpc_cl_last_ms is then clip + cost + records without the integration, which
 * nnmpc_cl_last_plant_ms reports.  Takes effect at the next nnmpc_cl_run. */
int nnmpc_cl_set_plant(nnmpc_cl* h, int32_t kind, const double* par, int32_t npar, double sample_time, int32_t substeps);
/* device time of the nonlinear plant's step kernel (integration + measurement) summed over the last run's steps; 0 when the
 * plant is linear */
int nnmpc_cl_last_plant_ms(nnmpc_cl* h, double* plant_ms);
/* batched flow map: x_out[i] = Phi(x[i], u[i], p[i]) for nb instances, x / x_out nb x 12, u nb x 6, p nb x 5 (row-major),
 * all host or all device (ptr_kind).  Instances are independent: one lane each. */
int nnmpc_cstrs_flow(int32_t nb, const double* par, int32_t npar, double sample_time, int32_t substeps, const double* x,
                     const double* u, const double* p, double* x_out, int32_t ptr_kind);

/* ---- Device plumbing: HBM buffers, copies and synchronisation for host programs that bind only this library. */
int nnmpc_device_count(void);
int nnmpc_set_device(int32_t dev);
int nnmpc_device_synchronize(void);
int nnmpc_dev_mem_info(uint64_t* free_bytes, uint64_t* total_bytes);
int nnmpc_dev_malloc(void** out, uint64_t bytes);
int nnmpc_dev_free(void* p);
int nnmpc_dev_memset(void* p, int32_t value, uint64_t bytes);
int nnmpc_memcpy_h2d(void* dst, const void* src, uint64_t bytes);
int nnmpc_memcpy_d2h(void* dst, const void* src, uint64_t bytes);
int nnmpc_memcpy_d2d(void* dst, const void* src, uint64_t bytes);
int nnmpc_host_alloc_pinned(void** out, uint64_t bytes);
int nnmpc_host_free_pinned(void* p);

/* ---- One process per GPU, results gathered over xGMI (RCCL)  <-  the reference's parallel model: independent OS
 * processes / cluster jobs on contiguous slices of the scenario signal (OfflineSimulator._split_scenarios,
 * generate_data, lib/linearMPC.py:786-825) whose per-task files are concatenated afterwards (_post_process_data,
 * lib/controller_evaluation.py:273-295).  Here every rank solves its contiguous shard with no communication and the
 * first moves meet on one rank in ONE gather.  nnmpc_comm_unique_id is called by one rank, the 128 bytes reach the
 * others by any side channel (bench.py: a file under /tmp, all ranks are on one node), then every rank calls
 * nnmpc_comm_init with the HIP device it will use already current (nnmpc_set_device). */
typedef struct nnmpc_comm nnmpc_comm;
int nnmpc_comm_unique_id(void* id128);
int nnmpc_comm_init(nnmpc_comm** out, const void* id128, int32_t rank, int32_t world);
int nnmpc_comm_destroy(nnmpc_comm* c);
int nnmpc_comm_rank(nnmpc_comm* c);
int nnmpc_comm_world(nnmpc_comm* c);
/* send: rows[rank] x row_doubles (device) -> recv on root: sum(rows) x row_doubles (device), rank blocks in rank
 * order; rows: world entries (host), the same on every rank; ragged shards allowed.  Blocking. */
int nnmpc_comm_gather_rows(nnmpc_comm* c, const double* send, const int64_t* rows, int32_t row_doubles,
                           double* recv, int32_t root);
int nnmpc_comm_allreduce_max(nnmpc_comm* c, double* value);   /* host scalar in/out */
int nnmpc_comm_barrier(nnmpc_comm* c);                        /* device idle and every rank arrived */

#ifdef __cplusplus
}
#endif
#endif
