/*
 * vmp_hip.h -- C ABI of libvmp_hip.so: the MI355X (gfx950) VMP hot path.
 *
 * The reference (bayespy/bayespy) has no FFI: its "operator interface" for this
 * path is the Python Distribution / Deterministic node protocol
 * (bayespy/inference/vmp/nodes/stochastic.py:16-80, expfamily.py:17-70,
 * deterministic.py:16-96) whose bodies are NumPy/SciPy call sites.  Each entry
 * point below replaces one group of those call sites; the citation next to it
 * names the reference code it stands in for.  INTEGRATION.md shows the ctypes
 * binding a bayespy maintainer would add.
 *
 * Conventions
 *  - all device pointers are plain `double*` / `int64_t*` into HBM, IEEE fp64;
 *  - every function returns an int32 status (VMP_OK or a negative VMP_ERR_*),
 *    is asynchronous on the context's HIP stream, never owns caller memory and
 *    is thread-compatible (one context per host thread);
 *  - "plates" are the reference's leading broadcast axes; the big observation
 *    plate N is always the contiguous (coalescing) axis of device arrays.
 */
#ifndef VMP_HIP_H
#define VMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VMP_OK               0
#define VMP_ERR_INVALID     -1  /* shape / plate mismatch      -> ValueError (node.py:343-356)            */
#define VMP_ERR_NOT_POSDEF  -2  /* "Matrix not positive definite" (utils/linalg.py:58-59)                 */
#define VMP_ERR_HIP         -3  /* HIP runtime failure         -> RuntimeError                            */
#define VMP_ERR_UNSUPPORTED -4  /* size outside the built kernels -> NotImplementedError (wishart.py:138) */
#define VMP_ERR_FLOATING    -5  /* invalid / divide            -> FloatingPointError (gamma.py:142-144)   */
#define VMP_ERR_NOT_POSITIVE -6 /* "Natural parameters should be positive" (dirichlet.py:147-148)         */

typedef struct vmp_ctx vmp_ctx;

/* ---- context, memory ----------------------------------------------------- */

/* Create a context on `device`.  `stream` is a hipStream_t (NULL = the null
 * stream); the caller keeps ownership of the stream. */
int32_t vmp_ctx_create(int32_t device, void *stream, vmp_ctx **out);
int32_t vmp_ctx_destroy(vmp_ctx *ctx);
int32_t vmp_ctx_set_stream(vmp_ctx *ctx, void *stream);
int32_t vmp_ctx_sync(vmp_ctx *ctx);
/* Number of compute units of the context's device (256 on MI355X). */
int32_t vmp_ctx_num_cu(vmp_ctx *ctx);
/* Human-readable text of the last error recorded on this context. */
const char *vmp_last_error(vmp_ctx *ctx);
const char *vmp_version(void);

int32_t vmp_malloc(vmp_ctx *ctx, size_t bytes, void **ptr);
int32_t vmp_free(vmp_ctx *ctx, void *ptr);
int32_t vmp_memcpy_h2d(vmp_ctx *ctx, void *dst, const void *src, size_t bytes);
int32_t vmp_memcpy_d2h(vmp_ctx *ctx, void *dst, const void *src, size_t bytes);
int32_t vmp_memset_zero(vmp_ctx *ctx, void *dst, size_t bytes);

/* ---- collective: plate sums over ranks ------------------------------------- *
 *
 * One process per GPU, the outermost observation plate sharded over the ranks.  Every sum
 * the reference takes over that plate -- child -> parent messages (node.py:650 ->
 * utils/misc.py:805, dot.py:581) and per-node lower-bound terms (expfamily.py:470-480) --
 * is a local partial sum followed by vmp_allreduce_sum_f64: an fp64 sum all-reduce (RCCL
 * over xGMI) enqueued on the context's stream, in place.  The communicator lives in the
 * context: rank 0 calls vmp_comm_unique_id, the caller ships the 128 bytes to the other
 * ranks by any means (MPI, a file, torch.distributed), every rank calls vmp_comm_init_rank.
 * A context without a communicator is a world of one rank (the all-reduce is the identity).
 * RCCL is loaded on first use (dlopen "librccl.so.1"); single-GPU use never touches it. */
typedef struct vmp_comm_id { char bytes[128]; } vmp_comm_id;
int32_t vmp_comm_unique_id(vmp_ctx *ctx, vmp_comm_id *id);
int32_t vmp_comm_init_rank(vmp_ctx *ctx, const vmp_comm_id *id, int32_t rank, int32_t world);
int32_t vmp_comm_destroy(vmp_ctx *ctx);
int32_t vmp_comm_info(vmp_ctx *ctx, int32_t *rank, int32_t *world);
int32_t vmp_allreduce_sum_f64(vmp_ctx *ctx, double *buf, int64_t count);

/* ---- fused probabilistic-PCA / factor-analysis block --------------------- *
 *
 * Model block  Y = GaussianARD(SumMultiply('i,i', W, X), tau),  W ~ GaussianARD(0, alpha),
 * X ~ GaussianARD(0, x_prec), tau, alpha ~ Gamma   (bayespy/demos/pca.py:22-61),
 * fully observed (scalar mask).  One VB iteration reads Y exactly once.
 *
 * All replicated (small) quantities live in ONE device block of doubles, the
 * "state", whose layout is given by vmp_pca_get_layout(); the caller allocates
 * `total` doubles.  The statistics region S is what ranks all-reduce (sum)
 * when the observation plate N is sharded.
 */
typedef struct vmp_pca_layout {
    int64_t DP, KP;     /* padded dims the kernels use (DP mult. of 32, KP of 16)            */
    int64_t off_S;      /* (DP+KP) x KP : rows [0,D) = sum_n y_n <x_n>^T (dot.py:581 msg to W) */
                        /*               rows [DP,DP+K) = sum_n <x_n><x_n>^T                   */
    int64_t len_S;      /* (DP+KP)*KP                                                          */
    int64_t off_Syy;    /* 1 : sum_dn y_dn^2  (constant)                                       */
    int64_t off_tau;    /* 4 : a, b, <tau>, <log tau>                (gamma.py:142-148)        */
    int64_t off_alpha;  /* 4*KP : a[KP], b[KP], <alpha>[KP], <log alpha>[KP]                   */
    int64_t off_W;      /* D x KP   <W>, row-major ld=KP             (gaussian.py:692-699)     */
    int64_t off_CW;     /* KP x KP  Cov_W (shared by all d)                                    */
    int64_t off_Sww;    /* KP x KP  sum_d <w_d w_d^T>                                          */
    int64_t off_CX;     /* KP x KP  Cov_X (shared by all n; zero for delta-initialised X)      */
    int64_t off_A;      /* KP x DP  A = <tau> Cov_X <W>^T, zero padded                         */
    int64_t off_G;      /* DP x DP  Gram matrix G = Y Y^T (constant; summed over ranks once)   */
    int64_t off_scal;   /* 8 : [0] log|Lambda_W|  [1] log|Lambda_X|  [2] residual  [3] status  */
    int64_t off_L;      /* 8 : L_Y, L_X, L_W, L_tau, L_alpha, L_total                          */
    int64_t total;      /* doubles in the state block                                          */
    int64_t off_mu;     /* D x KP   constant prior mean of W (zero unless the caller writes it;  */
                        /*          read by vmp_pca_small_ops_mean with has_mean = 1)           */
    int64_t off_mstat;  /* 2*KP : sum_d mu_dk <w_dk> | sum_d mu_dk^2 (written by the W update)   */
} vmp_pca_layout;

int32_t vmp_pca_get_layout(int32_t D, int32_t K, vmp_pca_layout *out);
/* Bytes of scratch (per-workgroup partial statistics) the pass needs. */
int32_t vmp_pca_workspace_bytes(vmp_ctx *ctx, int32_t D, int32_t K, size_t *bytes);

/* Prior moments for tau / alpha (ExponentialFamily.initialize_from_prior,
 * expfamily.py:168-184), zero Cov_X, zero statistics. */
int32_t vmp_pca_init_state(vmp_ctx *ctx, int32_t D, int32_t K,
                           double a0_tau, double b0_tau,
                           double a0_alpha, double b0_alpha, double *state);

/* sum_dn y^2 over the local shard -> state[off_Syy]  (part of E9/E16,
 * gaussian.py:628-635).  Y is (D, N) row-major with leading dimension ldy. */
int32_t vmp_pca_syy(vmp_ctx *ctx, const double *Y, int64_t ldy, int64_t N,
                    int32_t D, int32_t K, double *state, void *workspace);

/* Statistics of a GIVEN X (delta moments after initialize_from_value,
 * expfamily.py:193-204): S <- [Y X^T ; X X^T] over the local shard.
 * X is (K, N) row-major, leading dimension ldx. */
int32_t vmp_pca_stats_from_x(vmp_ctx *ctx, const double *Y, int64_t ldy, int64_t N,
                             int32_t D, int32_t K, const double *X, int64_t ldx,
                             double *state, void *workspace);

/* The replicated-node updates below (W, the replicated half of X, tau, alpha, the lower
 * bound) are latency-bound K x K work.  vmp_pca_small_ops runs a list of them, in the
 * order given (the order VB.update visits the nodes, vmp.py:154-160), inside ONE
 * single-workgroup launch; the five named entry points that follow are the one-operation
 * forms of the same kernel. */
enum vmp_pca_op {
    VMP_PCA_OP_W = 1,      /* vmp_pca_update_w     */
    VMP_PCA_OP_XPREP = 2,  /* vmp_pca_prepare_x    */
    VMP_PCA_OP_TAU = 3,    /* vmp_pca_update_tau   */
    VMP_PCA_OP_ALPHA = 4,  /* vmp_pca_update_alpha */
    VMP_PCA_OP_ELBO = 5    /* vmp_pca_lower_bound  */
};
#define VMP_PCA_MAX_OPS 8
int32_t vmp_pca_small_ops(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                          double a0_tau, double b0_tau, double a0_alpha, double b0_alpha,
                          int32_t nops, const int32_t *ops, double *state);

/* The same with a constant NON-ZERO prior mean of W (GaussianARD(mu, alpha, ...): gaussian.py:649-670
 * phi0_d = <alpha> * mu_d + message; the Gamma message to alpha and the bound term of W see
 * <(w - mu)^2>, gaussian.py:2344-2369).  mu lies in state[off_mu] (D x KP, written by the caller
 * after vmp_pca_init_state); has_mean = 0 is vmp_pca_small_ops.  The operations then run as the
 * general single-workgroup kernel (the LDS-resident fused forms are built for mu = 0). */
int32_t vmp_pca_small_ops_mean(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                               double a0_tau, double b0_tau, double a0_alpha, double b0_alpha,
                               int32_t nops, const int32_t *ops, int32_t has_mean, double *state);

/* W.update(): GaussianARDDistribution.compute_phi_from_parents + messages E3/E4
 * + compute_moments_and_cgf (gaussian.py:649-706, dot.py:581).  Uses S (already
 * summed over ranks), <tau>, <alpha>; writes W, CW, Sww, log|Lambda_W|. */
int32_t vmp_pca_update_w(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total,
                         double *state);

/* X.update(), replicated half: Lambda_X = x_prec I + <tau> Sww, Cov_X, A
 * (gaussian.py:649-706 with messages E5/E6 of dot.py:581). */
int32_t vmp_pca_prepare_x(vmp_ctx *ctx, int32_t D, int32_t K, double x_prec,
                          double *state);

/* G <- Y Y^T over the local shard (set-up; the caller all-reduces G once when the
 * plate is sharded).  With a scalar mask every <x_n> is the same linear map of y_n,
 * so the messages to W (dot.py:581) collapse onto G:  sum y<x>^T = G A^T and
 * sum <x><x>^T = A G A^T. */
int32_t vmp_pca_gram(vmp_ctx *ctx, const double *Y, int64_t ldy, int64_t N,
                     int32_t D, int32_t K, double *state, void *workspace);

/* X.update(), plate half, Gram form (default): for every local n  <x_n> = A y_n
 * is written to X ((K,N) row-major) -- read Y once, write <x> once, HBM-bound --
 * then S <- [G A^T ; A G A^T] from the (already global) Gram matrix: no
 * per-iteration collective.  fp64 MFMA (v_mfma_f64_16x16x4_f64).
 *
 * Padding: with D, K at their padded sizes and ldy, ldx >= 32 * ceil(N / 32) the ragged last
 * tile runs through the predication-free kernel as well, which also writes the pad columns
 * X[:, N .. 32*ceil(N/32)) (= A times the pad columns of Y); with smaller leading dimensions
 * only columns < N are touched.
 *
 * Ordering: in this form no other update of the iteration reads X, so the plate pass is
 * issued on the context's internal plate stream (from a private copy of A) and the call
 * returns with S queued on the main stream; the replicated-node updates of the next
 * iteration overlap the pass.  Passes are ordered among themselves.  Anything that reads
 * X outside this library on the context's stream must call vmp_pca_xjoin first
 * (vmp_ctx_sync, vmp_pca_pass and vmp_pca_stats_from_x join implicitly). */
int32_t vmp_pca_xpass(vmp_ctx *ctx, const double *Y, int64_t ldy, int64_t N,
                      int32_t D, int32_t K, double *X, int64_t ldx,
                      double *state, void *workspace);

/* Make the context's stream wait for the outstanding vmp_pca_xpass (no host block). */
int32_t vmp_pca_xjoin(vmp_ctx *ctx);
/* Every Gram-form latent pass overwrites all of <x>, and nothing in an iteration reads it.  With
 * on != 0 (default off), vmp_pca_xpass / vmp_pca_xpass_tiled on the plate stream still do their
 * main-stream part (private copy of A, S or its pending flag) but HOLD the pass kernel: it is
 * launched, on the plate stream and bit for bit as it would have been, by whatever may read or
 * release its X next -- vmp_pca_xjoin and every call that joins implicitly (vmp_pca_pass,
 * vmp_pca_stats_from_x, vmp_pca_tile_x), vmp_ctx_sync, vmp_ctx_destroy, the pass timing read-outs
 * and vmp_pca_hold_passes(ctx, 0) (which launches without joining).  A later pass into the same X
 * with the same N, D, K, ldx and layout, which writes at least the same elements, takes the place
 * of a held one (the held one is dropped: superseded); a pass that targets anything else launches
 * the held one first.  The arrays a held pass names (Y, X, the workspace) must stay allocated and
 * unchanged until one of the calls above; X must not be read before one of them.
 * VMP_PCA_HOLD_PASSES=0 / tune key "pca_hold_passes" = 0 turn on != 0 into a no-op; so does
 * VMP_PCA_PLATE_STREAM=0. */
int32_t vmp_pca_hold_passes(vmp_ctx *ctx, int32_t on);
/* Latent passes (vmp_pca_xpass*) launched / superseded on this context since it was created. */
int32_t vmp_pca_pass_counts(vmp_ctx *ctx, int64_t *launched, int64_t *superseded);
/* A batch of n VB sweeps over (W, X, tau, alpha) in the Gram form, enqueued on the context's stream
 * with NO synchronisation and no host read between them: per sweep the sequence W, XPREP,
 * S = [G A^T ; A G A^T], TAU, ALPHA, ELBO of vmp_pca_small_ops / vmp_pca_xpass* as at most three
 * launches and no copies.  Results are bit for bit those of n per-sweep calls.
 *
 * ring: n slots of VMP_PCA_SWEEP_SLOT doubles on the device.  Every sweep writes its slot: the bound
 * terms [Y, X, W, tau, alpha, total], the status word (0 or a VMP_ERR_* code) and 1.0 for "executed";
 * a sweep that was skipped writes 0.0 for "executed" only.
 *
 * Stopping: after its slot the last kernel of a sweep forms L = 0.0 + t[order[0]] + ... (the order
 * the caller adds the terms in; order[i] = -1 stands for a constant 0.0) and stops the batch when
 * the status is non-zero or, with compare != 0, when (L - L0) / (0.5 (|L0| + |L|)) < tol in fp64
 * (csrc/vmp_stop_rule.h; a NaN compares false).  L0 is l0 for the first sweep -- pass NaN for
 * "none" -- and the previous sweep's L after it.  Every kernel of a sweep after a stop returns at
 * once: the state is what the stopping sweep left.
 *
 * The latent pass: only the last sweep of the batch issues one, after its W / XPREP kernel, exactly
 * as vmp_pca_xpass (lay = 0: Y row-major with ldy), vmp_pca_xpass_tiled (lay = 1: tile-major Y,
 * lay = 3: tile-major X as well; ldy unused) would -- so it is held under vmp_pca_hold_passes and
 * it reads the A of the last EXECUTED sweep.  The passes of the other sweeps are counted as
 * superseded (vmp_pca_pass_counts).
 *
 * Covers the shapes of the LDS-resident kernels (K <= 32, D <= 128, zero prior mean of W); returns
 * VMP_PCA_SWEEPS_NOT_BUILT, having done nothing, for anything else and when VMP_PCA_SWEEPS=0 / tune
 * key "pca_sweeps" = 0 turns the entry off: the caller then runs the sweeps one by one. */
#define VMP_PCA_SWEEPS_NOT_BUILT 1
#define VMP_PCA_SWEEP_SLOT 8
#define VMP_PCA_MAX_SWEEPS 4096
int32_t vmp_pca_sweeps(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                       double a0_tau, double b0_tau, double a0_alpha, double b0_alpha,
                       const double *Y, int64_t ldy, int64_t N, double *X, int64_t ldx, int32_t lay,
                       double *state, void *workspace, int32_t n, double *ring, double tol,
                       int32_t compare, double l0, int32_t norder, const int32_t *order);
/* Sweeps enqueued by vmp_pca_sweeps on this context since it was created, and how many of them the
 * device executed / skipped after a stop (waits for the context's stream). */
int32_t vmp_pca_sweep_counts(vmp_ctx *ctx, int64_t *enqueued, int64_t *executed, int64_t *skipped);
/* Sweeps 1 .. n-1 of a batch of n are one launch each: the Gram statistics on DP / 8 workgroups, and
 * in the workgroup that draws the last ticket the tail of the sweep and the head of the next (tune
 * key "pca_sweep_ticket" / VMP_PCA_SWEEP_TICKET, default 1; 0: three launches per sweep, the same
 * arithmetic).  A state block that is not 16-byte aligned also takes the three launches, without an
 * error: this count is where that shows.  Launches of that kernel on this context since it was
 * created (no device read). */
int32_t vmp_pca_sweep_mid_count(vmp_ctx *ctx, int64_t *launches);
/* That launch is built for a GPU it has to itself.  Its workgroups form the rows of sum y<x>^T on the
 * matrix cores (v_mfma_f64_4x4x4_4b_f64) and store no partial blocks of sum <x><x>^T: the workgroup
 * that runs phase B loads everything its tail needs in one batch and forms that sum from the A and the
 * rows of sum y<x>^T it holds in LDS (v_mfma_f64_16x16x4_f64), the partials added in the order of the
 * three-launch sweep.  Both instructions add their four products to C in ascending order of the
 * k-slots, every step fused (vmp_mfma_order_probe below), so every chain keeps the bits of the scalar
 * chains of the three-launch sweep.  The tail hands over to the head, which keeps its D x K operand
 * whole in LDS, as soon as <tau>, <alpha>, Cov_X and sum <x><x>^T are ready; <log tau>, <log alpha>, the
 * bound, the ring slot and the stop rule are formed by one wavefront beside the head's first inverse.
 * A stop is read behind that inverse, before the head's first store, so a stopped loop leaves what
 * the three launches leave.  The special functions whose arguments do not change from sweep to sweep
 * (digamma and lgamma of the two Gamma shapes, lgamma(a0), log(b0), log(2 pi), log(x_prec)) are
 * computed by one small launch when the priors, D, the plate size or x_prec differ from those of the
 * previous call on the context, and read from a buffer of the context (not the state block) after
 * that.  The first head of a batch runs the same head body, in a launch of its own, unless a latent
 * pass is still in flight.  The one launch and the three launches agree bitwise.
 *
 * Measurement: while tune key "pca_sweep_stamps" is 1, vmp_pca_sweeps launches a stamped build of that
 * kernel, in which one lane records wall_clock64() (a constant 100 MHz counter) at the boundaries of
 * its phases: VMP_PCA_SWEEP_NSTAMP words per launch of the latest batch, 0 where a boundary was not
 * passed (order: csrc/vmp_pca_small.hip, enum SP_*).  At 2 the launch also records, in words 19
 * and 20, where its side wavefront has stored the tau / alpha state and where it has written the ring
 * slot and the stop word.  This call waits for the stream and copies up to
 * max_rows rows out.  The buffer belongs to the context and exists only once the key has been on:
 * *allocated (may be null) says whether it does. */
#define VMP_PCA_SWEEP_NSTAMP 24
int32_t vmp_pca_sweep_stamps(vmp_ctx *ctx, uint64_t *out, int32_t max_rows, int32_t *rows,
                             int32_t *allocated);
/* The Gram statistics of one sweep alone, from the A and G of the state block.
 * form 0: the kernel of the three-launch sweep -- the rows of sum y<x>^T into the state, the DP / 8
 * partial blocks of sum <x><x>^T into the workspace (not added up).  form 1: phase A of the one-launch
 * sweep (K <= 32, D <= 128, 16-byte aligned state) -- the rows of sum y<x>^T into the state and nothing
 * else: it does not write the workspace.  The rows agree bitwise.  Any other form: VMP_ERR_INVALID. */
int32_t vmp_pca_gram_stats_form(vmp_ctx *ctx, int32_t D, int32_t K, double *state, void *workspace,
                                int32_t form);
/* Test entry: D = A B + C by ONE fp64 matrix instruction per tile, one wavefront, `ntiles` tiles in
 * a row (device pointers, row-major doubles).  form 0: v_mfma_f64_16x16x4_f64, A 16 x 4, B 4 x 16,
 * C and D 16 x 16 per tile.  form 1: v_mfma_f64_4x4x4_4b_f64, four independent blocks per tile,
 * A[b][i][k], B[b][k][j], C and D [b][i][j], 64 doubles each.  tests/test_mfma_order_gpu.py reads
 * the order in which the four products of an output are accumulated off the bits. */
int32_t vmp_mfma_order_probe(vmp_ctx *ctx, int32_t form, int32_t ntiles, const double *A,
                             const double *B, const double *C, double *D);
/* Gram form: the messages to W of the latest latent pass, S = [G A^T ; A G A^T] in the state block
 * (dot.py:581 collapsed onto the Gram matrix), are formed lazily -- by the fused tau / alpha / bound
 * kernel when it comes next, else by this call, which every other entry point that reads S makes
 * itself (vmp_pca_small_ops*, vmp_pca_xjoin, vmp_ctx_sync).  A binding that reads the state block
 * directly (vmp_memcpy_d2h) calls it first.  No-op when nothing is pending. */
int32_t vmp_pca_ensure_gram(vmp_ctx *ctx);

/* Tile-major layout of the plate arrays.  Y is constant after Y.observe()
 * (stochastic.py:223-250), so it is re-laid-out ONCE into blocks of 32 plate elements,
 *     Yt[tile][d][j] = Y[d][32 tile + j],   tile < ceil(N/32), d < DP, j < 32,
 * zero padded in d and in the last tile.  The plate pass then streams one contiguous
 * 8*32*DP-byte span per tile (every load instruction of a wavefront covers 1 KB of consecutive
 * addresses) instead of DP row streams that lie 8*ldy bytes apart.  X may use the same layout
 * with KP rows per tile ([tile][k][j]).  vmp_pca_tiled_doubles gives the array sizes. */
int32_t vmp_pca_tiled_doubles(int32_t D, int32_t K, int64_t N, int64_t *y_doubles,
                              int64_t *x_doubles);
int32_t vmp_pca_tile_y(vmp_ctx *ctx, const double *Y, int64_t ldy, int64_t N,
                       int32_t D, int32_t K, double *Yt);
/* to_tiled != 0: Xt <- X (K rows of the row-major (K, ldx) array); else X <- Xt. */
int32_t vmp_pca_tile_x(vmp_ctx *ctx, int32_t to_tiled, double *X, int64_t ldx, int64_t N,
                       int32_t D, int32_t K, double *Xt);
/* vmp_pca_xpass on a tile-major Y.  x_tiled != 0: X is tile-major too (ldx ignored);
 * x_tiled == 0: X is row-major with KP rows and ldx >= 32*ceil(N/32) (pad rows / columns are
 * written).  Results are bit-identical to vmp_pca_xpass. */
int32_t vmp_pca_xpass_tiled(vmp_ctx *ctx, const double *Yt, int64_t N, int32_t D, int32_t K,
                            double *X, int64_t ldx, int32_t x_tiled,
                            double *state, void *workspace);

/* X.update(), plate half, streaming-statistics form: for every local n
 *   <x_n> = A y_n  (written to X, (K,N) row-major),
 *   S <- [sum y_n <x_n>^T ; sum <x_n><x_n>^T]  (local partial; caller all-reduces:
 *   the child->parent message sum over the sharded plate, node.py:650, dot.py:581).
 * fp64 MFMA (v_mfma_f64_16x16x4_f64), MFMA-bound. */
int32_t vmp_pca_pass(vmp_ctx *ctx, const double *Y, int64_t ldy, int64_t N,
                     int32_t D, int32_t K, double *X, int64_t ldx,
                     double *state, void *workspace);

/* tau.update(): message gaussian.py:2363-2369 collapsed to traces (dot.py:355,403)
 * + gamma.py:116-148. */
int32_t vmp_pca_update_tau(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total,
                           double a0, double b0, double *state);
/* alpha.update(): gaussian.py:2361-2369 + gamma.py:116-148. */
int32_t vmp_pca_update_alpha(vmp_ctx *ctx, int32_t D, int32_t K,
                             double a0, double b0, double *state);
/* VB.loglikelihood_lowerbound (vmp.py:192-199) = sum of
 * ExponentialFamily.lower_bound_contribution (expfamily.py:400-480) over
 * Y, X, W, tau, alpha -> state[off_L .. off_L+5]. */
int32_t vmp_pca_lower_bound(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total,
                            double x_prec,
                            double a0_tau, double b0_tau,
                            double a0_alpha, double b0_alpha, double *state);


/* ---- fused PCA block WITH MISSING VALUES ---------------------------------------------- *
 *
 * The model block of the fused PCA entry points above with Y.observe(y, mask=array)
 * (bayespy/demos/pca.py:80-82; masks: node.py:457-526, stochastic.py:223-250).  Every plate
 * n (and every row d) has its own K x K posterior; the reference materialises (1,N,K,K)
 * second moments, contracts them with einsum (dot.py:355,403,581) and loops in Python over
 * the plates for the Cholesky factorisations (utils/linalg.py:31-63).  Here X.update() runs
 * chunk by chunk over the plates, three kernels per chunk on the fp64 matrix cores
 * (bayespy_amd/csrc/vmp_mpca.hip), and only the statistics
 *     M_d = sum_n m_dn <x x^T>_n  (packed lower triangle),   r_d = sum_n m_dn y_dn <x_n>
 * survive a chunk (state[off_M]: what ranks all-reduce).  D <= 128, K <= 32.
 * Array layouts (Ymt, the two bit layouts of the mask, Xm, the scratch of a chunk) are
 * documented at the top of vmp_mpca.hip; vmp_mpca_sizes gives their sizes. */
typedef struct vmp_mpca_layout {
    int64_t DP, KP;      /* padded dims: DP in {32,64,128}, KP in {16,32}                        */
    int64_t P, PT, LR;   /* packed triangle size KP(KP+1)/2, its 16-column tiles, row length
                            LR = 16 (PT + KP/16) of [packed | K-vector] rows                      */
    int64_t off_tau;     /* 8 : a, b, <tau>, <log tau>                                            */
    int64_t off_alpha;   /* 4*KP : a, b, <alpha>, <log alpha>                                     */
    int64_t off_scal;    /* 16: [0] sum m y^2 [1] sum m [2] sum_n tr<xx>_n [3] sum_n log|Cov_n|
                            [4] plates N [5] status [6] <tau> of the last X pass [7] residual     */
    int64_t off_L;       /* 8 : L_Y, L_X, L_W, L_tau, L_alpha, L_total                            */
    int64_t off_W;       /* DP x KP      <w_d>                                                    */
    int64_t off_WW;      /* DP x KP x KP <w_d w_d^T>                                              */
    int64_t off_ldW;     /* DP           log|Cov_d|                                               */
    int64_t off_M;       /* DP x LR      packed M_d | r_d                                         */
    int64_t off_panel;   /* B operands of the precision GEMM (fragment order), current W          */
    int64_t off_panel_x; /* ... as seen by the last X.update()                                    */
    int64_t off_Sxx;     /* KP x KP      sum_n <x x^T>_n (all plates; rotations)                  */
    int64_t off_rowobs;  /* DP           observations per dimension d (summed over ranks by the
                            caller); rows with none are ignored plates of W (node.py:457-526)      */
    int64_t total;
} vmp_mpca_layout;

typedef struct vmp_mpca_sizes_t {
    int64_t ymt_doubles;        /* tile-major m*y                                                 */
    int64_t mask_words;         /* uint32 words of EACH of the two bit layouts of the mask        */
    int64_t xm_doubles;         /* <x_n>, plate-major (32 ceil(N/32)) x KP                        */
    int64_t lam_doubles;        /* scratch of one chunk: chunk x LR                               */
    int64_t xxf_doubles;        /* scratch of one chunk: packed <xx>_n                            */
    int64_t workspace_doubles;  /* per-workgroup partial statistics                               */
} vmp_mpca_sizes_t;

enum vmp_mpca_op { VMP_MPCA_OP_TAU = 1, VMP_MPCA_OP_ALPHA = 2, VMP_MPCA_OP_ELBO = 3 };

int32_t vmp_mpca_get_layout(int32_t D, int32_t K, vmp_mpca_layout *out);
int32_t vmp_mpca_sizes(vmp_ctx *ctx, int32_t D, int32_t K, int64_t N, int64_t chunk,
                       vmp_mpca_sizes_t *out);
int32_t vmp_mpca_init_state(vmp_ctx *ctx, int32_t D, int32_t K, double a0_tau, double b0_tau,
                            double a0_alpha, double b0_alpha, double *state);
/* Set-up after Y.observe(y, mask): Ymt <- m*y tile-major (values at masked entries are never
 * read: NaN placeholders are fine), the two bit layouts of the mask, sum m y^2, sum m and the
 * observation count of every dimension into the state.  mask: uint8 (D, ldm) row-major, NULL = all observed. */
int32_t vmp_mpca_prepare(vmp_ctx *ctx, const double *Y, int64_t ldy, const uint8_t *mask,
                         int64_t ldm, int64_t N, int32_t D, int32_t K, double *Ymt,
                         uint32_t *Mb1, uint32_t *Mb2, double *state, void *workspace);
/* X.update() = vmp_mpca_x_begin (snapshot of <tau>, <w>, <ww> and the plate count, summed over
 * ranks by the caller) + vmp_mpca_x_chunk over consecutive chunks of plates (n0 a multiple of
 * 32; VMP_MPCA_FIRST on the first).  VMP_MPCA_FROM_VALUE: statistics of the <x_n> already in Xm
 * (initialize_from_value, expfamily.py:193-204) instead of an update. */
int32_t vmp_mpca_x_begin(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_plates, double *state);
#define VMP_MPCA_FIRST      1   /* first chunk of a pass: statistics are overwritten, not added to */
#define VMP_MPCA_FROM_VALUE 2   /* delta moments of the <x_n> in Xm instead of an update           */
#define VMP_MPCA_PRIOR      4   /* prior moments: <x_n> = 0, <xx>_n = I / x_prec                   */
#define VMP_MPCA_INSPECT    8   /* recompute <x_n>, <xx>_n of the chunk only (no statistics)       */
int32_t vmp_mpca_x_chunk(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n0, int64_t nplates,
                         int32_t flags, double x_prec, const double *Ymt,
                         const uint32_t *Mb1, const uint32_t *Mb2, double *Xm, double *Lam,
                         double *XXf, double *state, void *workspace);
/* All chunks of one pass over the plates [0, N) (flags as above, VMP_MPCA_FIRST implied).
 * nsets = 1: Lam / XXf hold one chunk, the chunks run in order on the context's stream.
 * nsets = 2: they hold two chunks each and consecutive chunks are pipelined over three library
 * streams: the matrix-core GEMMs of the neighbouring chunks run beside the vector-ALU-bound sweep
 * of a chunk.  The statistics accumulate in chunk order either way (identical results). */
int32_t vmp_mpca_x_pass(vmp_ctx *ctx, int32_t D, int32_t K, int64_t N, int64_t chunk,
                        int32_t nsets, int32_t flags, double x_prec, const double *Ymt,
                        const uint32_t *Mb1, const uint32_t *Mb2, double *Xm, double *Lam,
                        double *XXf, double *state, void *workspace);
/* W.update() (mode 0); mode 1: delta moments of the <w_d> in state[off_W]; mode 2: prior. */
int32_t vmp_mpca_update_w(vmp_ctx *ctx, int32_t D, int32_t K, int32_t mode, double *state);
/* tau.update(), alpha.update(), the lower bound terms: a list of vmp_mpca_op, one launch. */
int32_t vmp_mpca_small_ops(vmp_ctx *ctx, int32_t D, int32_t K, double x_prec, double a0_tau,
                           double b0_tau, double a0_alpha, double b0_alpha, int32_t nops,
                           const int32_t *ops, double *state);
/* <x x^T>_n of the first nplates plates of the chunk scratch, unpacked to (nplates, K, K). */
int32_t vmp_mpca_unpack_xx(vmp_ctx *ctx, int32_t D, int32_t K, int64_t nplates,
                           const double *XXf, double *out);

/* ---- fused linear state-space model block (BASELINE.json config 5) ----------------------- *
 *
 * bayespy/demos/lssm.py:34-103 with a plate of B sequences: X = GaussianMarkovChain(mu0, Lam0,
 * A, nu, n=T, plates=(B,)), Y = GaussianARD(SumMultiply('i,i', C, X), tau) fully observed.
 * Dynamics, noise and mask are shared by the sequences, so the covariance recursion of
 * linalg.block_banded_solve (utils/linalg.py:468-575, gaussian_markov_chain.py:89-123) runs ONCE
 * (vmp_lssm_cov) and only the means are per-sequence (vmp_lssm_smooth: one thread per
 * sequence, time-major arrays Yt[t][m][b], Z[t][i][b], b contiguous); the other nodes and the
 * bound read plate sums only.  D <= 16 states (round 6: for 8 < D <= 16 the sweeps carry the state
 * only -- on the projected data tau C^T Y -- and the plate sums are formed behind them, the shared
 * covariance recursion runs on one workgroup with its blocks in LDS), M <= 64 observations per step (beyond M = 8, or 16
 * at D <= 4, the sweeps run on the projected data tau C^T y with a separate y <x>^T pass).  Details: bayespy_amd/csrc/vmp_lssm.hip, formulas: oracle/lssm.py. */
typedef struct vmp_lssm_layout {
    int64_t off_tau;      /* 4: a, b, <tau>, <log tau>                                             */
    int64_t off_gamma, off_alpha, off_nu;   /* 4*D each: a[D], b[D], mean[D], log-mean[D]          */
    int64_t off_mu0, off_Lam0, off_ldLam0;  /* D, D*D, 1: constants of the initial state           */
    int64_t off_Cm, off_CovC, off_SCC;      /* M*D <c_m>, D*D shared Cov_C, D*D sum_m <c c^T>      */
    int64_t off_Am, off_AA, off_ldA;        /* D*D <a_i>, D*D*D <a_i a_i^T>, D log|Cov_A_i|        */
    int64_t off_Dg;       /* 4*D*D: diagonal blocks of the chain precision (t=0, inner, last), E   */
    int64_t off_h0;       /* D: Lam0 mu0                                                           */
    int64_t off_covsums;  /* 5*D*D+8: output of vmp_lssm_cov (+ its state between segments)       */
    int64_t off_raw, len_raw;  /* mean-part plate sums of vmp_lssm_smooth (what ranks all-reduce)  */
    int64_t off_S;        /* Sxx | Spp | Snn | Snp | S00 (D*D each) | s0 (D) | Syx (M*D)           */
    int64_t off_scal;     /* 8: [0] sum y^2 [1] log|Phi| [2] status [3] <tau> of the last X pass
                                [4] log|Cov_C|                                                     */
    int64_t off_L;        /* 16: L_Y, L_C, L_A, L_X, L_gamma, L_alpha, L_tau, L_nu, total          */
    int64_t total;
} vmp_lssm_layout;

enum vmp_lssm_op {
    VMP_LSSM_OP_STATS = 1, VMP_LSSM_OP_C, VMP_LSSM_OP_GAMMA, VMP_LSSM_OP_XPREP, VMP_LSSM_OP_A,
    VMP_LSSM_OP_ALPHA, VMP_LSSM_OP_TAU, VMP_LSSM_OP_NU, VMP_LSSM_OP_ELBO
};

int32_t vmp_lssm_limits(int32_t *max_D, int32_t *max_M);
int32_t vmp_lssm_get_layout(int32_t D, int32_t M, vmp_lssm_layout *out);
int32_t vmp_lssm_workspace_doubles(int32_t D, int32_t M, int64_t B, int32_t T, int64_t *n);
/* Y (M, B, T) -> Yt (T, M, BL) time-major (once: Y is constant after observe); sum y^2 -> *syy. */
int32_t vmp_lssm_relayout_y(vmp_ctx *ctx, const double *Y, int32_t M, int64_t B, int32_t T,
                            int64_t BL, double *Yt, double *syy, void *workspace);
/* X (B, T, D) <-> Z (T, D, BL) */
int32_t vmp_lssm_x_layout(vmp_ctx *ctx, double *X, int32_t D, int64_t B, int32_t T, int64_t BL,
                          double *Z, int32_t to_time_major);
/* The shared D x D recursion over T.  Dg0 / Dgm / DgT: diagonal blocks of the precision at t = 0,
 * 0 < t < T-1, t = T-1; E = Phi[t, t+1].  Out: Sinv (T,D,D), J (T-1,D,D), sums (5 D^2 + 4). */
int32_t vmp_lssm_cov(vmp_ctx *ctx, int32_t T, int32_t D, const double *Dg0, const double *Dgm,
                     const double *DgT, const double *E, double *Sinv, double *J, double *sums);
/* Forward + backward vector recursions of all sequences and their plate sums (given != 0: the
 * sums of the <x> already in Z, no recursion: initialize_from_value). */
int32_t vmp_lssm_smooth(vmp_ctx *ctx, int32_t given, const double *Yt, int32_t M, int64_t B,
                        int32_t T, int64_t BL, int32_t D, const double *Cm, const double *tau,
                        const double *h0, const double *Sinv, const double *J, double *Z,
                        double *stats, void *workspace);
/* X.update() in one call = vmp_lssm_cov + vmp_lssm_smooth(given = 0), with the backward half of the
 * covariance recursion (not needed by the per-sequence passes) on a side stream beside them;
 * stream-ordered: everything is complete for later work on the context's stream. */
int32_t vmp_lssm_x_update(vmp_ctx *ctx, int32_t T, int32_t D, const double *Dg0, const double *Dgm,
                          const double *DgT, const double *E, double *Sinv, double *J,
                          double *covsums, const double *Yt, int32_t M, int64_t B, int64_t BL,
                          const double *Cm, const double *tau, const double *h0, double *Z,
                          double *stats, void *workspace);
/* <x_bt> <- R <x_bt> on the time-major means Z (T, D, BL): the state-space rotation of
 * transformations.py:1167-1176 applied to the plate-sized array; R: D x D row-major, device. */
int32_t vmp_lssm_rotate_x(vmp_ctx *ctx, int32_t D, int32_t T, int64_t B, int64_t BL, const double *R,
                          double *Z);
/* Replicated-node updates / the bound, a list of vmp_lssm_op in one launch.  priors: host array
 * of 8 doubles, the Gamma (a0, b0) of tau, gamma, alpha, nu. */
int32_t vmp_lssm_small_ops(vmp_ctx *ctx, int32_t D, int32_t M, int32_t T, double B_total,
                           const double *priors, int32_t nu_latent, int32_t nops,
                           const int32_t *ops, double *state);

/* ---- fused linear state-space model block, ARRAY masks ----------------- *
 *
 * The same model observed through ``Y.observe(y, mask=array)`` (bayespy/demos/lssm.py:132,
 * :239-246: ``mask = random.mask(M, N, p=0.3); mask[:, 30:80] = False``), the mask
 * broadcastable to (M, B, T).  A message is multiplied by the child's mask before the plate
 * sum (node.py:570-655), so
 *   - every sequence has its own block-tridiagonal precision: diagonal blocks
 *     prior + <tau> sum_m mask_mbt <c_m c_m^T> (gaussian_markov_chain.py:542-627, dot.py:425-633),
 *     hence its own D x D covariance recursion (linalg.block_banded_solve, utils/linalg.py:468-575),
 *     run by a group of FOUR LANES PER SEQUENCE (the rows of the blocks dealt over a DPP quad) in
 *     registers beside the mean recursion; vmp_tune_set("lssmm_lanes", 1): one thread per sequence
 *     (D <= 4);
 *   - every row of C has its own posterior (gaussian.py:649-706 with the per-row message
 *     sum_bt mask_mbt <x_bt x_bt^T>);
 *   - rows / sequences without any observation are ignored plates (node.py:486-526,
 *     expfamily.py:470-480).
 * Time-major arrays, b contiguous: Yt[t][m][b] (zero where masked), Mw[t][b] (uint64, bit m =
 * mask_mbt), F[t][NS + D][b] (forward sweep: S_t^-1 packed lower triangle | z_t), Z[t][D][b] (<x>),
 * P[t][NS][b] (<x x^T> packed), NS = D (D + 1) / 2.  D <= 8 states, M <= 64 observed dimensions,
 * M D^2 <= 2048 (the tables of the sweeps in LDS).
 * Details: bayespy_amd/csrc/vmp_lssmm.hip, vmp_lssmm_dev.h; formulas: oracle/lssm.py
 * (MaskedLSSMOracle).  Ops: enum vmp_lssm_op (STATS is a no-op here). */
typedef struct vmp_lssmm_layout {
    int64_t NS;           /* D (D + 1) / 2                                                          */
    int64_t off_tau;      /* 4: a, b, <tau>, <log tau>                                              */
    int64_t off_gamma, off_alpha, off_nu;   /* 4*D each: a[D], b[D], mean[D], log-mean[D]           */
    int64_t off_mu0, off_Lam0, off_ldLam0;  /* D, D*D, 1                                            */
    int64_t off_Cm;       /* M*D  <c_m>                                                             */
    int64_t off_CovC;     /* M*D*D  Cov(c_m) per row                                                */
    int64_t off_ldC;      /* M  log|Cov(c_m)|                                                       */
    int64_t off_SCC;      /* D*D  sum over the observed rows of <c_m c_m^T>                         */
    int64_t off_Am, off_AA, off_ldA;        /* D*D, D*D*D, D                                        */
    int64_t off_tab, len_tab;   /* tables of the sweeps, written by XPREP (full matrices, rows
                                   contiguous): base (3*D*D: t = 0, inner, last) | E (D*D) | h0 (D) |
                                   tau c_m (M*D) | tau <c_m c_m^T> (M*D*D)                          */
    int64_t off_setup, len_setup;  /* vmp_lssmm_prepare (summed over ranks): sum mask y^2 |
                                   sequences with data | observations per row n_m (M)              */
    int64_t off_raw, len_raw;   /* plate sums of an X pass (summed over ranks):
                                   sum_t P (NS) | sum <x_t+1 x_t^T> (D*D) | P_0 (NS) | P_T-1 (NS) |
                                   x_0 (D) | sum_b log|Phi_b| (1)   -- sequences with data only --
                                   | XX_m = sum_bt mask P (M*NS) | Syx_m = sum_bt y x (M*D)         */
    int64_t off_scal;     /* 8: [0] status [1] <tau> of the last XPREP                              */
    int64_t off_L;        /* 16: L_Y, L_C, L_A, L_X, L_gamma, L_alpha, L_tau, L_nu, total           */
    int64_t total;
} vmp_lssmm_layout;

int32_t vmp_lssmm_limits(int32_t *max_D, int32_t *max_M);
int32_t vmp_lssmm_get_layout(int32_t D, int32_t M, vmp_lssmm_layout *out);
int32_t vmp_lssmm_workspace_doubles(int32_t D, int32_t M, int64_t B, int32_t T, int64_t *n);
/* Set-up (the data are constant after observe): Y (M, B, T) row-major and the mask as bytes with
 * ELEMENT strides (sm, sb, st; 0 = broadcast axis) -> Yt (zero where masked; values there are
 * never read, NaN placeholders are fine), Mw, seqobs[b] = 1.0 if sequence b has any observation,
 * state[off_setup ...]. */
int32_t vmp_lssmm_prepare(vmp_ctx *ctx, const double *Y, const uint8_t *mask, int64_t sm,
                          int64_t sb, int64_t st, int32_t M, int64_t B, int32_t T, int64_t BL,
                          int32_t D, double *Yt, uint64_t *Mw, double *seqobs, double *state,
                          void *workspace);
/* X.update(): forward sweep (per-sequence covariance + mean recursions -> F), backward sweep
 * (-> Z, P, chain sums; for D <= 4, M <= 8 also XX_m, Syx_m), otherwise a statistics pass over the
 * stored Z, P (XX_m, Syx_m); the sums land in state[off_raw ...].
 * given = 1: the sums of the <x> already in Z as point masses (initialize_from_value);
 * given = 2: q(X) unchanged, only XX_m / Syx_m again from the stored Z, P (Y re-observed). */
int32_t vmp_lssmm_x_update(vmp_ctx *ctx, int32_t given, const double *Yt, const uint64_t *Mw,
                           const double *seqobs, int32_t M, int64_t B, int32_t T, int64_t BL,
                           int32_t D, double *state, double *F, double *Z, double *P,
                           void *workspace);
/* <x x^T> <- R <x x^T> R^T on the packed plate array P (T, NS, BL): the state rotation of
 * inference/transformations.py (reference: gaussian_markov_chain.py rotate, gaussian.py:1693-1741)
 * applied on the device; the means go through vmp_lssm_rotate_x. */
int32_t vmp_lssmm_rotate_p(vmp_ctx *ctx, int32_t D, int32_t T, int64_t B, int64_t BL, const double *R,
                           double *P);
/* Replicated-node updates / the bound: a list of vmp_lssm_op in one launch. */
int32_t vmp_lssmm_small_ops(vmp_ctx *ctx, int32_t D, int32_t M, int32_t T, const double *priors,
                            int32_t nu_latent, int32_t nops, const int32_t *ops, double *state);

/* ---- fused full-covariance Gaussian-mixture block -------------------------- *
 *
 * Model block  Y = Mixture(z, Gaussian, mu, Lambda), z = Categorical(alpha),
 * alpha = Dirichlet(a0), mu = GaussianARD(0, beta0, shape=(D,), plates=(K,)),
 * Lambda = Wishart(n0, V0, plates=(K,))   (bayespy/demos/mog.py:17-64), Y fully
 * observed, D <= 32, K <= 64.  One VB iteration reads Y exactly once and writes the
 * responsibilities once.  Y is (N, D) row-major (the reference's layout), the
 * responsibilities R are (N, K) row-major.
 */
typedef struct vmp_gmm_layout {
    int64_t DP, KP;        /* padded D (4 or 8) and K (16, 32, 64)                          */
    int64_t FS;            /* 1 + D + D*D : row length of the statistics                      */
    int64_t FP, F2P;       /* padded feature count [y_a y_b (a<=b), y_d, 1] of both MFMA phases */
    int64_t off_T, len_T;  /* KP x FS : per cluster [R_k, sum_n r y (D), sum_n r y y^T (D*D)] */
                           /*   -- the plate sums of mixture.py:126-158 + node.py:650          */
    int64_t off_zs;        /* sum_n logsumexp(phi_n), sum_nk r phi   (for L_z)                */
    int64_t off_alpha;     /* alpha[KP], <log pi>[KP]                  (dirichlet.py:150-158) */
    int64_t off_mu;        /* KP x D   <mu_k>                                                 */
    int64_t off_Cmu;       /* KP x D x D  Cov(mu_k)                                           */
    int64_t off_logdetLmu; /* KP  log|Lambda_mu_k|                                            */
    int64_t off_nk;        /* KP  Wishart degrees of freedom                                  */
    int64_t off_Vk;        /* KP x D x D  Wishart inverse scale                               */
    int64_t off_Lam;       /* KP x D x D  <Lambda_k> = n_k V_k^-1        (wishart.py:184)     */
    int64_t off_logdetLam; /* KP  <log|Lambda_k|>                          (wishart.py:185)   */
    int64_t off_logdetV;   /* KP  log|V_k|                                                    */
    int64_t off_C;         /* KP x F2P coefficients of ell_nk in the compact feature order     */
    int64_t off_prior;     /* alpha0[KP], beta0, n0, log|V0|, 5 pad, V0[D*D]                  */
    int64_t off_scal;      /* 8 : [3] status                                                  */
    int64_t off_L;         /* 8 : L_Y, L_z, L_alpha, L_mu, L_Lambda, L_total                  */
    int64_t total;
} vmp_gmm_layout;

int32_t vmp_gmm_get_layout(int32_t D, int32_t K, vmp_gmm_layout *out);
int32_t vmp_gmm_workspace_bytes(vmp_ctx *ctx, int32_t D, int32_t K, size_t *bytes);
/* Store the priors (host arrays alpha0[K], V0[D*D]) and initialise every node from its
 * prior (expfamily.py:168-184). */
int32_t vmp_gmm_init_state(vmp_ctx *ctx, int32_t D, int32_t K, const double *alpha0_host,
                           double beta0, double n0, const double *V0_host, double *state);
/* z.initialize_from_value(labels): one-hot responsibilities (categorical.py:30-46,
 * bit-exact) written to R and their statistics to T. */
int32_t vmp_gmm_stats_from_labels(vmp_ctx *ctx, const double *Y, int64_t N, int32_t D, int32_t K,
                                  const int64_t *labels, double *R, double *state,
                                  void *workspace);
/* mu.update(): gaussian.py:649-706 with the mixture-weighted messages of
 * gaussian.py:2451-2454 / mixture.py:126-158. */
int32_t vmp_gmm_update_mu(vmp_ctx *ctx, int32_t D, int32_t K, double *state);
/* Lambda.update(): wishart.py:153-188 with the messages gaussian.py:2516-2520. */
int32_t vmp_gmm_update_lambda(vmp_ctx *ctx, int32_t D, int32_t K, double *state);
/* z.update(), replicated half: coefficients of E[log p(y_n | k)] + <log pi_k>
 * (mixture.py:67-104, expfamily.py:45-61).  prior_only != 0 keeps only <log pi_k>
 * (q(z) initialised from its prior). */
int32_t vmp_gmm_prepare_z(vmp_ctx *ctx, int32_t D, int32_t K, int32_t prior_only, double *state);
/* z.update(), plate half -- THE pass: phi = C feat(y), r = normalized_exp(phi)
 * (multinomial.py:114-120, utils/misc.py:1388-1401) written to R, and the statistics
 * T = r^T [1, y, y y^T] (local partial; the caller all-reduces T and zs). fp64 MFMA. */
int32_t vmp_gmm_pass(vmp_ctx *ctx, const double *Y, int64_t N, int32_t D, int32_t K, double *R,
                     double *state, void *workspace);
/* alpha.update(): dirichlet.py:113-160 with the message categorical -> [r]. */
int32_t vmp_gmm_update_alpha(vmp_ctx *ctx, int32_t D, int32_t K, double *state);
/* Stochastic variational inference (vmp.py:432-440): ONE launch moves the global nodes in the bit
 * set `nodes` (1 = mu, 2 = Lambda, 4 = alpha) by a step of length `scale` along their natural
 * gradients, phi <- phi + scale (phi* - phi).  The optimum phi* is that of the update entry points
 * above with the statistics T weighted by `mult` (the plates_multiplier of a mini-batch), and every
 * optimum is taken from the moments present at entry -- the simultaneous step of the reference, not
 * a sequence of updates.  The moments of the stepped nodes are formed again from the new
 * parameters.  `phi_mu` (device, K * (D + D*D) doubles, cluster-major: h_k = Lambda_mu,k m_k, then
 * Lambda_mu,k) holds the natural parameters of q(mu); those of Lambda and alpha are the state's own
 * (off_nk, off_Vk), (off_alpha).  scale == 1 takes phi* itself, and with mult == 1 the step of one
 * node then equals vmp_gmm_update_mu / _lambda / _alpha bit for bit.  A matrix that is not positive
 * definite sets the status word of the state (VMP_ERR_NOT_POSDEF), as in the update entry points.
 * vmp_gmm_natural_init sets phi_mu to the prior of the means (h = 0, Lambda_mu = beta0 I) from an
 * initialised state. */
int32_t vmp_gmm_natural_init(vmp_ctx *ctx, int32_t D, int32_t K, const double *state,
                             double *phi_mu);
int32_t vmp_gmm_natural_step(vmp_ctx *ctx, int32_t D, int32_t K, int32_t nodes, double mult,
                             double scale, double *state, double *phi_mu);
/* Lower bound of Y, z, alpha, mu, Lambda (expfamily.py:400-480). */
int32_t vmp_gmm_lower_bound(vmp_ctx *ctx, int32_t D, int32_t K, double *state);
/* Deterministic annealing (vmp.py:665-677, expfamily.py:343-350, :400-480): a node with the
 * coefficient `annealing` = b in (0, 1] updates to b times its natural parameters, and its bound term
 * weighs the q part by the temperature T = 1 / b.  The plate pass is the one of vmp_gmm_pass: the
 * factor of z sits in the C table.
 *   vmp_gmm_prepare_z_annealed   C = b (<log pi_k> + E[log p(y | k)]), every constant included; the
 *                                -inf of padded clusters stays; prior_only != 0 ignores b
 *   vmp_gmm_update_annealed      node 1: mu, precision b (beta0 I + R_k <Lambda_k>), the mean as at
 *                                b = 1; node 2: Lambda, n_k = b (n0 + R_k), V_k = b (V0 + ...), both
 *                                stored annealed; node 4: alpha_k = b (alpha0_k + R_k)
 *   vmp_gmm_lower_bound_annealed every term as [cgf_p + phi_p . u] - T [phi_q . u + g_q] with the
 *                                temperature of its node, q being what the state holds
 * With b = 1 (T = 1) each gives the bits of the entry point it stands beside.  An annealed Wishart
 * with b (n0 + R_k) <= D - 1 sets the status word of the state to VMP_ERR_INVALID (the reference
 * goes on with NaN). */
int32_t vmp_gmm_prepare_z_annealed(vmp_ctx *ctx, int32_t D, int32_t K, int32_t prior_only,
                                   double annealing, double *state);
int32_t vmp_gmm_update_annealed(vmp_ctx *ctx, int32_t D, int32_t K, int32_t node, double annealing,
                                double *state);
int32_t vmp_gmm_lower_bound_annealed(vmp_ctx *ctx, int32_t D, int32_t K, double T_z, double T_alpha,
                                     double T_mu, double T_lambda, double *state);

/* ---- generic plate-broadcast kernels -------------------------------------- *
 *
 * Arrays are fp64 with explicit ELEMENT strides per axis; stride 0 marks a
 * broadcast axis (the reference's unit / missing plate axes).
 */
#define VMP_MAX_DIMS          8
#define VMP_MAX_OPERANDS      6
#define VMP_EWISE_MAX_OPS     48
#define VMP_EWISE_MAX_CONSTS  8

/* out[kept axes] = scale * sum_{axes in reduce_mask} prod_i in_i[...]
 * -- misc.sum_multiply (utils/misc.py:851-933, np.einsum call site :906) and the
 * plate sum of Node._message_to_parent via misc.sum_multiply_to_plates
 * (node.py:650, utils/misc.py:805-844); `scale` carries broadcasting_multiplier
 * (utils/misc.py:761-802).  in_strides is [nin][ndim] row-major; out_strides[ndim]
 * (ignored on reduced axes).  Deterministic (fixed-order) reduction. */
int32_t vmp_sum_multiply(vmp_ctx *ctx, int32_t ndim, const int64_t *shape, int32_t nin,
                         const double *const *in, const int64_t *in_strides,
                         const int64_t *out_strides, uint32_t reduce_mask, double scale,
                         double *out, void *workspace, size_t workspace_bytes);
size_t vmp_sum_multiply_workspace_bytes(void);

/* Fused broadcast elementwise formula: a postfix program (opcode | operand<<8)
 * over <= VMP_MAX_OPERANDS inputs evaluated per output element with a 4-deep
 * stack; `out` is contiguous with the given shape.  Replaces the NumPy ufunc
 * chains inside the Distribution formulas (e.g. gaussian.py:675-678, :2344-2369,
 * gamma.py:142-148, dirichlet.py:150-158, expfamily.py:449-468). */
enum {
    VMP_OP_IN = 0, VMP_OP_CONST, VMP_OP_ADD, VMP_OP_SUB, VMP_OP_MUL, VMP_OP_DIV, VMP_OP_NEG,
    VMP_OP_LOG, VMP_OP_EXP, VMP_OP_SQR, VMP_OP_SQRT, VMP_OP_RECIP, VMP_OP_DIGAMMA,
    VMP_OP_LGAMMA, VMP_OP_MAX, VMP_OP_MIN, VMP_OP_WHERE_NZ, VMP_OP_DUP, VMP_OP_SWAP,
    VMP_OP_TRIGAMMA,
    VMP_OP__COUNT
};
int32_t vmp_ewise(vmp_ctx *ctx, int32_t ndim, const int64_t *shape, int32_t nin,
                  const double *const *in, const int64_t *in_strides, int32_t nops,
                  const int32_t *ops, int32_t nconsts, const double *consts, double *out);

/* A sequence of calls recorded into a HIP graph and replayed: the launches of a VB sweep are the
 * same every iteration -- same kernels, same shapes, only the contents of the arrays move -- so a
 * binding records one sweep (every call of this library between begin and end is recorded on the
 * context's stream instead of run; the arrays must be allocated before, nothing may be read on
 * the host inside) and launches the graph once per iteration afterwards.  The context needs a
 * stream of its own (vmp_ctx_create / vmp_ctx_set_stream: not the legacy default stream).  A binding
 * that manages its own arrays uses these four.  The Python front end (plans/graph_iter.py) cannot:
 * its sweeps ALLOCATE -- every array operation of the engine returns a fresh device array -- and an
 * allocation inside a stream capture must come from a pool that lives as long as the graph, which
 * is what torch.cuda.graph provides (torch's caching allocator is the allocator of this package:
 * DESIGN.md section 1).  It therefore opens the capture through torch and issues the SAME library
 * calls on the capturing stream; vmp_copy_many / vmp_pack_outputs / vmp_queue_commit are the pieces
 * of such a recording that live behind this boundary. */
int32_t vmp_graph_begin(vmp_ctx *ctx);
int32_t vmp_graph_end(vmp_ctx *ctx, void **graph);
int32_t vmp_graph_launch(vmp_ctx *ctx, void *graph);
int32_t vmp_graph_destroy(vmp_ctx *ctx, void *graph);

/* n device-to-device copies of `count[i]` doubles each (contiguous, non-overlapping) as ONE launch
 * per 24 of them on the context's stream -- the copy-back of the state arrays of a recorded sweep
 * (graph_iter.py; the reference has no analogue: it rebinds NumPy arrays, stochastic.py:223-273). */
int32_t vmp_copy_many(vmp_ctx *ctx, int32_t n, const double *const *src, double *const *dst,
                      const int64_t *count);

/* out[i] for i < n: kind[i] = 0: the double at src[i]; 1 / 2: 1.0 if any of the count[i] int32 /
 * double values at src[i] is non-zero (NaN included), else 0.0 -- the lower-bound terms and the
 * validity flags of a recorded sweep (expfamily.py:400-480; "Matrix not positive definite",
 * utils/linalg.py:58-59) gathered by ONE launch for the single device-to-host read of a replay. */
int32_t vmp_pack_outputs(vmp_ctx *ctx, int32_t n, const void *const *src, const int64_t *count,
                         const int32_t *kind, double *out);

/* Queue of SMALL operations.  Between vmp_queue_begin and vmp_queue_end, vmp_ewise and
 * vmp_sum_multiply calls on small arrays (<= 2048 outputs, <= 32768 products) and vmp_spd_batched
 * calls on a few small matrices (8 < n <= 32, batch <= 4) are recorded on the host and run, in
 * order, by ONE launch of an interpreter kernel -- when any other entry point of the generic part
 * of this library needs the stream (it flushes first), when 128 of them are collected, at
 * vmp_queue_flush or at the outermost vmp_queue_end.  A VB sweep of the generic engine
 * is ~90 such operations on scalars and K x K arrays (the Gamma / ARD formulas of gamma.py:142-148,
 * gaussian.py:2344-2369, the bound terms of expfamily.py:449-468) between a dozen plate-sized
 * kernels.  The interpreter keeps the small arrays of a launch in LDS: results are written to
 * memory AND to a 112 KB arena, a record reads what an earlier record of the launch produced --
 * or a small array from outside, copied in when the launch starts -- from there, and only a record
 * that reads MEMORY written earlier in the launch waits for those stores; the records themselves are
 * staged through LDS.  ("small_queue_lds" = 0: every operand from memory, a fence per record.)
 * Results do not depend on the grouping.  The caller must flush before it reads an
 * output on the host or hands it to work outside this library.  begin / end nest; a context whose
 * stream records a HIP graph keeps the records of its flushes for the life of the context; their
 * device copies are made by vmp_queue_commit, which belongs between the end of the recording and
 * the first launch of the graph (vmp_graph_end calls it; a binding that records through another
 * API calls it itself).  vmp_tune_set("small_queue", 0) makes begin / end no-ops;
 * "small_queue_ew" / "small_queue_sm" = 0 keep formulas / sums and inverses out of the queue. */
int32_t vmp_queue_begin(vmp_ctx *ctx);
int32_t vmp_queue_flush(vmp_ctx *ctx);
int32_t vmp_queue_end(vmp_ctx *ctx);
int32_t vmp_queue_commit(vmp_ctx *ctx);
int32_t vmp_queue_stats(vmp_ctx *ctx, int64_t *launches, int64_t *ops);

/* Batched SPD inverse and log-determinant of `batch` contiguous n x n matrices
 * (n <= 64): linalg.chol + chol_inv + chol_logdet (utils/linalg.py:31-223), one
 * workgroup / wavefront per matrix instead of a Python loop over plates.
 * Ainv / logdet may be NULL; info[b] = 1 where a matrix is not positive definite
 * ("Matrix not positive definite", utils/linalg.py:58-59). */
int32_t vmp_spd_batched(vmp_ctx *ctx, int32_t n, int64_t batch, const double *A, double *Ainv,
                        double *logdet, int32_t *info);

/* Moments and log-normaliser of a Gaussian with a full covariance per plate from its natural
 * parameters, one pass (GaussianARDDistribution.compute_moments_and_cgf, gaussian.py:680-706,
 * i.e. linalg.chol + chol_inv + chol_solve + outer + chol_logdet fused):
 *   Cov = (-2 phi1)^-1,  u0 = Cov phi0,  u1 = u0 u0^T + Cov,
 *   g = -1/2 u0 . phi0 + 1/2 log|-2 phi1|.
 * phi0, u0: batch x n; phi1, u1: batch x n x n; g: batch; info[b] = 1 where -2 phi1 is not
 * positive definite.  Built for 8 < n <= 32 (row-per-lane kernel); other sizes go through
 * vmp_spd_batched + vmp_sum_multiply. */
int32_t vmp_gaussian_moments(vmp_ctx *ctx, int32_t n, int64_t batch, const double *phi0,
                             const double *phi1, double *u0, double *u1, double *g,
                             int32_t *info);

/* ONE pass for the update of a Gaussian node whose posterior covariance is SHARED by its N plates
 * (a plate-free precision: GaussianARD / Gaussian under a scalar mask) -- the natural parameters
 * from the prior and the message (GaussianARDDistribution.compute_phi_from_parents,
 * gaussian.py:649-670), the posterior means (compute_moments_and_cgf, gaussian.py:672-706:
 * <x> = Cov phi0), the Dot / SumMultiply message the node receives when it is given as its
 * operands (dot.py:581: m_n = B^T y_n), and the plate sums its neighbours ask for next (dot.py:581
 * for the other parent, expfamily.py:449-468):
 *     m_n = B^T y_n                 Y form: Y (D x N, element strides y_sd, y_sn, one of them 1),
 *                                   B (D x K, strides b_sd, b_sk); m0 = NULL
 *         | m0[n, :]                message form: rows of a given array (strides m0_sn, m0_sk); Y = NULL
 *     x_n = Cov (p0 + m_n)          p0: K doubles or NULL (= 0); Cov: K x K contiguous
 *     stats = [ sum_n x_n (K) ; sum_n x_n x_n^T (K x K) ; sum_n y_n x_n^T (D x K; Y form only) ]
 * x: N x K with element strides (x_sn, x_sk).  Y form: fp64 MFMA tile kernel (8 N (D + K) bytes of
 * algorithmic traffic, 4 N D K + 2 N K^2 flops), D <= 256; message form: 16 N K bytes.  K <= 64.
 * Partial sums are combined in fixed order.  `workspace`: at least
 * vmp_gaussian_shared_update_workspace_bytes(D, K) bytes (D = 0 for the message form). */
size_t vmp_gaussian_shared_update_workspace_bytes(int32_t D, int32_t K);
int32_t vmp_gaussian_shared_update(vmp_ctx *ctx, int64_t N, int32_t K, int32_t D,
                                   const double *Y, int64_t y_sd, int64_t y_sn, const double *B,
                                   int64_t b_sd, int64_t b_sk, const double *m0, int64_t m0_sn,
                                   int64_t m0_sk, const double *p0, const double *cov, double *x,
                                   int64_t x_sn, int64_t x_sk, double *stats, void *workspace,
                                   size_t workspace_bytes);

/* Row softmax moments of Multinomial/Categorical: p = normalized_exp(phi),
 * lse = logsumexp(phi) (multinomial.py:114-120, utils/misc.py:1366-1401). */
int32_t vmp_softmax_moments(vmp_ctx *ctx, int64_t rows, int32_t K, const double *phi, double *p,
                            double *lse);

/* One-hot fixed moments of Categorical (categorical.py:30-46, :93-114); integer
 * indexing, bit-exact.  *info != 0 when a label is outside [0, K). */
int32_t vmp_onehot_i64(vmp_ctx *ctx, int64_t n, int32_t K, const int64_t *labels, double *out,
                       int32_t *info);

/* Plate re-indexing of the deterministic nodes that move plates.  Arrays are contiguous and
 * seen as (outer, axis, inner).
 *   vmp_take_axis:  dst[o, dst_off + j, i] = src[o, idx ? idx[j] : j, i]  for j < n; dst has
 *     dst_len rows on the axis.  np.take on a plate axis (Take._compute_moments, take.py:72-81);
 *     with idx = NULL the block copy of Concatenate._compute_moments (concatenate.py:130-167).
 *     idx is a device array of n valid row numbers in [0, src_len).
 *   vmp_segment_sum_axis:  dst[o, l, i] = sum over t in [ptr[l], ptr[l+1]) of
 *     src[o, perm[t], i]  for l < out_len -- misc.put_simple (utils/misc.py:549-585), the
 *     accumulating inverse of take used by Take._compute_message_to_parent (take.py:83-94).
 *     ptr (out_len + 1) and perm (src_len) are device arrays: the CSR map from target row to
 *     its source rows, built once on the host; the order of the additions is fixed, so the
 *     result is bit-reproducible. */
int32_t vmp_take_axis(vmp_ctx *ctx, int64_t outer, int64_t src_len, int64_t inner,
                      const double *src, int64_t n, const int64_t *idx, double *dst,
                      int64_t dst_len, int64_t dst_off);
int32_t vmp_segment_sum_axis(vmp_ctx *ctx, int64_t outer, int64_t src_len, int64_t inner,
                             const double *src, int64_t out_len, const int64_t *ptr,
                             const int64_t *perm, double *dst);

/* Strided batched fp64 contraction on the matrix cores (v_mfma_f64_16x16x4_f64):
 *     C[b, m, n] = scale * sum_k A[b, m, k] * B[b, k, n]
 * with arbitrary ELEMENT strides on every axis (0 = broadcast batch axis), up to three
 * batch axes, split-K with fixed-order combination.  The dense N x K x D contractions
 * that SumMultiply / sum_multiply collapse to (dot.py:355, :403, :581 with array masks;
 * mixture.py:126-158; gaussian_markov_chain.py:462-475) instead of
 * np.einsum(optimize=False) (utils/misc.py:906).  `workspace` holds split-K partials. */
int32_t vmp_gemm_strided(vmp_ctx *ctx, int32_t nbatch_dims, const int64_t *bshape, int64_t M,
                         int64_t N, int64_t K, const double *A, const int64_t *a_bstride,
                         int64_t a_ms, int64_t a_ks, const double *B, const int64_t *b_bstride,
                         int64_t b_ks, int64_t b_ns, double *C, const int64_t *c_bstride,
                         int64_t c_ms, int64_t c_ns, double scale, void *workspace,
                         size_t workspace_bytes);

/* Forward-backward recursion of `nchains` categorical Markov chains with K states and N
 * transitions (N + 1 time instances): random.alpha_beta_recursion (utils/random.py:357-422),
 * the moments of CategoricalMarkovChain (categorical_markov_chain.py:107-117).
 *   logp0: K unnormalised log-probabilities of the first state per chain (chain stride
 *          p0_bstride elements, 0 = shared);
 *   logP:  N x K x K slices per chain, logP[n, i, j] = log p(z_{n+1} = j | z_n = i) + evidence
 *          of instance n + 1, each slice contiguous (chain stride P_bstride, time stride
 *          P_tstride elements; 0 = shared / time-invariant).
 * Out: z0 (nchains x K) = q(z_0), zz (nchains x N x K x K) = q(z_n, z_{n+1}), g (nchains) = minus
 * the log-normaliser.  workspace: nchains * N * K doubles.  K <= 64. */
int32_t vmp_alpha_beta_recursion(vmp_ctx *ctx, int32_t N, int32_t K, int64_t nchains,
                                 const double *logp0, int64_t p0_bstride, const double *logP,
                                 int64_t P_bstride, int64_t P_tstride, double *z0, double *zz,
                                 double *g, void *workspace, size_t workspace_bytes);

/* Block-tridiagonal SPD solve = Kalman filter + RTS smoother of the Gaussian Markov chain
 * (linalg.block_banded_solve, utils/linalg.py:468-575, called by
 * gaussian_markov_chain.py:89-123).  A: nm x T x K x K diagonal blocks, B: nm x (T-1) x K x K
 * super-diagonal blocks, y: ny x T x K right-hand sides; nm == 1 (shared dynamics) or
 * nm == ny.  Out: V (diagonal blocks of the inverse), C (super-diagonal blocks), x
 * (solutions), ldet[nm] (log-determinant); info[b] = 1 where a block is not positive
 * definite.  K <= 16 (a wavefront per matrix sequence up to K = 8, a workgroup above). */
int32_t vmp_block_banded_solve(vmp_ctx *ctx, int32_t T, int32_t K, int64_t nm, int64_t ny,
                               const double *A, const double *B, const double *y, double *V,
                               double *C, double *x, double *ldet, int32_t *info);

/* Maximum-likelihood hyperparameter nodes (gamma.py:273-334, dirichlet.py:234-330; details:
 * bayespy_amd/csrc/vmp_ml.hip).  Dense fp64 arrays; the summed messages of the children m0, m1
 * and the node's own terms r0, r1 ("prior" m0 / m1 of GammaShape, the regularization of
 * Concentration) come broadcast to the node's shape.
 *   vmp_ml_invpsi:        y = invpsi(x) elementwise (misc.invpsi, utils/misc.py:1404-1429).
 *   vmp_ml_gamma_shape:   a = invpsi(-(m0 + r0) / (m1 + r1)), lga = lgamma(a); n elements.
 *   vmp_ml_concentration: rows x K concentrations by the fixed point a <- invpsi(psi(sum a) +
 *     (m0 + r0) / (m1 + r1)) from a = 1, stopped at the first iteration where no element of ANY row
 *     moved by more than 1e-5 of its new value, at most max_iter iterations (one workgroup, one
 *     lane per element); z[r] = lgamma(sum a) - sum lgamma(a).  m0, r0, alpha and the scratch
 *     array work: rows x K, m1, r1, z: rows.  status (3 int32):
 *     [some mean_logp infinite (nothing iterated), max_iter reached, iterations run]. */
int32_t vmp_ml_invpsi(vmp_ctx *ctx, int64_t n, const double *x, double *y);
int32_t vmp_ml_gamma_shape(vmp_ctx *ctx, int64_t n, const double *m0, const double *m1,
                           const double *r0, const double *r1, double *a, double *lga);
int32_t vmp_ml_concentration(vmp_ctx *ctx, int64_t rows, int32_t K, const double *m0,
                             const double *m1, const double *r0, const double *r1, int32_t max_iter,
                             double *alpha, double *work, double *z, int32_t *status);

/* Plate sums of a Gaussian Markov chain's messages to time-varying dynamics shared by ny sequences
 * (gaussian_markov_chain.py:462-527; details: bayespy_amd/csrc/vmp_chain_tv.hip).
 *   vmp_chain_pair_stats: x (ny, N, D) row-major ->  Sxx (N, D, D) = sum_b x_{b,t} x_{b,t}^T  and
 *     Sxp (N-1, D, D) = sum_b x_{b,t} x_{b,t+1}^T  (Sxp may be NULL when N = 1).  x is read once;
 *     no atomics: two calls on the same input give the same bits.  ny = 0 is legal (zeros).
 *     `work`: scratch of at least the `work_doubles` the limits query reports for (ny, N, D).
 *     D above the limit: VMP_ERR_UNSUPPORTED; null / negative arguments: VMP_ERR_INVALID.
 *   vmp_chain_pair_stats_limits (host only): *max_d = the largest D with an instance (16),
 *     *enabled = the tune key "chain_pair_stats" (default 1; 0 keeps callers on the general
 *     operations), *work_doubles = the scratch the call needs for (ny, N, D). */
int32_t vmp_chain_pair_stats_limits(int64_t ny, int32_t N, int32_t D, int32_t *max_d,
                                    int32_t *enabled, int64_t *work_doubles);
int32_t vmp_chain_pair_stats(vmp_ctx *ctx, int64_t ny, int32_t N, int32_t D, const double *x,
                             double *Sxx, double *Sxp, double *work, int64_t work_doubles);

/* Plate sums of the input cross terms in a driven Gaussian Markov chain's messages to [A | B] and nu
 * shared by ny sequences (gaussian_markov_chain.py:485-498; details: bayespy_amd/csrc/vmp_chain_in.hip).
 *   vmp_chain_input_stats: x (ny, N, D) and z (zrows, N-1, K) row-major, zrows = ny or 1 (1: every
 *     sequence has the same inputs)  ->  Snz (N-1, D, K) = sum_b x_{b,t+1} z_{b,t}^T,
 *     Spz (N-1, D, K) = sum_b x_{b,t} z_{b,t}^T  and, unless Szz is NULL,
 *     Szz (N-1, K, K) = sum_b z_{b,t} z_{b,t}^T.  x and z are read once; no atomics: two calls on the
 *     same input give the same bits.  ny = 0 is legal (zeros).  `work`: scratch of at least the
 *     `work_doubles` the limits query reports for (ny, zrows, N, D, K).
 *     D or K above the limit: VMP_ERR_UNSUPPORTED; null / negative arguments, zrows not in {1, ny},
 *     N < 2 or a short workspace: VMP_ERR_INVALID.
 *   vmp_chain_input_stats_limits (host only): *max_d, *max_k = the largest D and K with an instance
 *     (16, 16), *enabled = the tune key "chain_input_stats" (default 1; 0 keeps callers on the
 *     general operations), *work_doubles = the scratch the call needs. */
int32_t vmp_chain_input_stats_limits(int64_t ny, int64_t zrows, int32_t N, int32_t D, int32_t K,
                                     int32_t *max_d, int32_t *max_k, int32_t *enabled,
                                     int64_t *work_doubles);
int32_t vmp_chain_input_stats(vmp_ctx *ctx, int64_t ny, int64_t zrows, int32_t N, int32_t D,
                              int32_t K, const double *x, const double *z, double *Snz,
                              double *Spz, double *Szz, double *work, int64_t work_doubles);

/* Latent Dirichlet allocation: the token pass and the Dirichlet rows of the fused block
 * (doc/source/examples/lda.rst; details: bayespy_amd/csrc/vmp_lda.hip, vmp_lda_dev.h).  n tokens, D
 * documents, V vocabulary entries, K topics; no tokens x K, tokens x V or tokens x D array exists.
 *   vmp_lda_limits (host only): *max_K = the largest K with an instance (64), *max_chunk = the
 *     largest number of tokens one lane group walks in order (256).
 *   vmp_lda_plan (host only): for (n, K) the lane group *group (power of two >= K), the tokens per
 *     chunk *chunk (a function of (n, K) alone) and the scratch *workspace_doubles of the pass.
 *   vmp_lda_token_pass: for every token l_k = elog_theta[doc, k] + elog_beta_t[word, k] (elog_theta:
 *     D x K, elog_beta_t: V x K, i.e. <log beta> transposed; NULL = no word term, the moments of
 *     `topics` under its prior), lse = max + log sum exp(l - max), phi_k = exp(l_k - lse).  Out:
 *     Ndk (D x K) and Nvk (V x K), the sums of phi over the tokens of a document / of a word;
 *     scal[0] = sum of lse, scal[1] = sum Ndk * elog_theta, scal[2] = sum Nvk * elog_beta_t (0
 *     without the word term); lse (n doubles, document order); with `phi` (n x K) also phi itself,
 *     row orig[i] for the i-th token in document order.  `labels` (document order) non-NULL: phi is
 *     the one-hot array of these topics instead and lse = 0.
 *     Layouts, built once per observation: tokens sorted by document -- doc_d, word_d (n) with the
 *     offsets doc_off (D + 1); tokens sorted by word -- word_w, doc_w and pos_w (n; position of that
 *     token in document order) with word_off (V + 1).  Indices are NOT checked against D, V, K on
 *     the device: the caller validates them.  `phases`: 1 = document pass, 2 = word pass, 4 = the two
 *     scal dot products; 7 = all (the parts exist for measurements).  ws: vmp_lda_plan's doubles.
 *     No atomics: the bits of every output depend on (inputs, n, K, layouts) only; two calls give
 *     the same bits.  Empty documents / unused words give zero rows; n = 0 gives zeros.  A topic
 *     with l_k = -inf gets phi_k = 0; a token whose logits are ALL -inf gets NaN (lse and phi), as in
 *     the reference.  K above the limit or n >= 2^31: VMP_ERR_UNSUPPORTED; null / negative
 *     arguments: VMP_ERR_INVALID.
 *   vmp_lda_dirichlet: rows x cols Dirichlet rows, element (r, c) of prior / counts / alpha / elog
 *     at r * row_stride + c * col_stride: alpha = prior + counts (counts NULL: the prior), elog =
 *     psi(alpha) - psi(sum_c alpha), *bound = sum over rows of the node's lower-bound term
 *     sum_c (prior - alpha) elog + [lgamma(sum prior) - sum lgamma(prior)] - [the same of alpha]
 *     (dirichlet.py:107-231).  ws: at least `rows` doubles.
 *   vmp_lda_dirichlet_step: the same rows after a step of length `scale` along the natural gradient
 *     (expfamily.py:296-340), with the counts of a mini-batch standing for `mult` times as many
 *     tokens: q = prior + mult * counts (counts NULL: the prior); scale == 1: alpha = q, the old
 *     alpha is not read and may be NaN; otherwise alpha = a + scale * (q - a) from the alpha `a`
 *     that is there.  elog and *bound as in vmp_lda_dirichlet, taken with the new alpha.  A table
 *     stored transposed with at most 64 rows (row_stride == 1, col_stride == rows: p_word as V x K)
 *     is walked along its memory by a kernel pair with a fixed-order combine between them; other
 *     strides use the kernels of vmp_lda_dirichlet.  No atomics: the bits of every output depend on
 *     the inputs and the shape only.  rows == 0: *bound = 0.  Null / negative arguments, mult <= 0
 *     or a NaN: VMP_ERR_INVALID.
 *   vmp_lda_dirichlet_step_workspace (host only): the doubles of `ws` that call needs.
 *   vmp_lda_dot: *out = sum a * b over m elements, added in an order that depends on m alone
 *     (ws: 1024 doubles). */
int32_t vmp_lda_limits(int32_t *max_K, int32_t *max_chunk);
int32_t vmp_lda_plan(int64_t n, int32_t K, int32_t *group, int32_t *chunk,
                     int64_t *workspace_doubles);
int32_t vmp_lda_token_pass(vmp_ctx *ctx, int64_t n, int64_t D, int64_t V, int32_t K,
                           const int32_t *doc_d, const int32_t *word_d, const int64_t *doc_off,
                           const int32_t *word_w, const int32_t *doc_w, const int32_t *pos_w,
                           const int64_t *word_off, const int32_t *labels,
                           const double *elog_theta, const double *elog_beta_t, int32_t phases,
                           double *lse, double *ws, double *Ndk, double *Nvk, double *scal,
                           const int32_t *orig, double *phi);
int32_t vmp_lda_dirichlet(vmp_ctx *ctx, int64_t rows, int64_t cols, int64_t row_stride,
                          int64_t col_stride, const double *prior, const double *counts,
                          double *alpha, double *elog, double *ws, double *bound);
int32_t vmp_lda_dirichlet_step_workspace(int64_t rows, int64_t cols, int64_t row_stride,
                                         int64_t col_stride, int64_t *workspace_doubles);
int32_t vmp_lda_dirichlet_step(vmp_ctx *ctx, int64_t rows, int64_t cols, int64_t row_stride,
                               int64_t col_stride, const double *prior, const double *counts,
                               double mult, double scale, double *alpha, double *elog, double *ws,
                               double *bound);
int32_t vmp_lda_dot(vmp_ctx *ctx, int64_t m, const double *a, const double *b, double *ws,
                    double *out);

/* Latent Dirichlet allocation with 65 .. 1024 topics: the wide-topic token pass (details:
 * bayespy_amd/csrc/vmp_lda_wide.hip, vmp_lda_wide_dev.h).  One wavefront walks a chunk of tokens,
 * lane j holds the topics j + 64 r in R registers; the Dirichlet rows and dot products are those of
 * the block above (vmp_lda_dirichlet, vmp_lda_dot), which are general in K.
 *   vmp_lda_wide_limits (host only): *min_K = 65, *max_K = 1024, *max_chunk = 256.
 *   vmp_lda_wide_plan (host only): for (n, K) the registers per lane *regs (the smallest of 2, 4, 8,
 *     16 with 64 * regs >= K), the tokens per chunk *chunk (a function of n alone) and the scratch
 *     *workspace_doubles of the pass.  K < 65, K > 1024 or n >= 2^31: VMP_ERR_UNSUPPORTED; null
 *     pointers or negative n: VMP_ERR_INVALID.
 *   vmp_lda_wide_token_pass: the arguments, outputs, layouts, `phases`, -inf / NaN behaviour and
 *     error codes of vmp_lda_token_pass, for 65 <= K <= 1024 (other K: VMP_ERR_UNSUPPORTED).  ws:
 *     vmp_lda_wide_plan's doubles.  No atomics: the bits of every output depend on (inputs, n, K,
 *     layouts) only. */
int32_t vmp_lda_wide_limits(int32_t *min_K, int32_t *max_K, int32_t *max_chunk);
int32_t vmp_lda_wide_plan(int64_t n, int32_t K, int32_t *regs, int32_t *chunk,
                          int64_t *workspace_doubles);
int32_t vmp_lda_wide_token_pass(vmp_ctx *ctx, int64_t n, int64_t D, int64_t V, int32_t K,
                                const int32_t *doc_d, const int32_t *word_d,
                                const int64_t *doc_off, const int32_t *word_w,
                                const int32_t *doc_w, const int32_t *pos_w,
                                const int64_t *word_off, const int32_t *labels,
                                const double *elog_theta, const double *elog_beta_t,
                                int32_t phases, double *lse, double *ws, double *Ndk, double *Nvk,
                                double *scal, const int32_t *orig, double *phi);

/* Latent Dirichlet allocation with a learnt concentration: the plate-sized step between the
 * Dirichlet tables of the block and vmp_ml_concentration (details: bayespy_amd/csrc/vmp_lda_hyper.hip,
 * vmp_lda_hyper_dev.h).  Tables in the stride convention of vmp_lda_dirichlet, in one of two forms:
 * row-major (col_stride == 1, row_stride == cols, cols <= 1024) or transposed (row_stride == 1,
 * col_stride == rows, rows <= 1024); other strides: VMP_ERR_UNSUPPORTED.
 *   vmp_lda_concentration_stats: one pass over alpha and elog leaves S[c] = sum_rows elog[r, c]
 *     (cols doubles; the message m0 of the Dirichlets to their concentration, m1 = rows) and
 *     *qterm = sum_rows ( lgamma(sum_c alpha_rc) - sum_c lgamma(alpha_rc) + sum_c (alpha_rc - 1)
 *     elog_rc ), the part of the Dirichlets' lower-bound term that does not depend on the prior.
 *     No atomics: chunk partials and a combine in a fixed order, the bits of both outputs depend on
 *     the inputs and the shape only.  rows == 0: zeros.  A NaN in a table reaches *qterm (and S where
 *     it stands in elog).  Null / negative arguments: VMP_ERR_INVALID.
 *   vmp_lda_concentration_stats_workspace (host only): the doubles of `ws` that call needs.
 *   vmp_lda_prior_fill: prior[r * row_stride + c * col_stride] = a[c] for every row r (any strides). */
int32_t vmp_lda_concentration_stats_workspace(int64_t rows, int64_t cols, int64_t row_stride,
                                              int64_t col_stride, int64_t *workspace_doubles);
int32_t vmp_lda_concentration_stats(vmp_ctx *ctx, int64_t rows, int64_t cols, int64_t row_stride,
                                    int64_t col_stride, const double *alpha, const double *elog,
                                    double *ws, double *S, double *qterm);
int32_t vmp_lda_prior_fill(vmp_ctx *ctx, int64_t rows, int64_t cols, int64_t row_stride,
                           int64_t col_stride, const double *a, double *prior);

/* Bernoulli mixture: the plate pass of the fused block (doc/source/examples/bmm.rst; details:
 * bayespy_amd/csrc/vmp_bmm.hip, vmp_bmm_dev.h).  N rows of D binary observations, K clusters; x is
 * kept as bits, no (N, D, K) or (N, K) array exists.
 *   vmp_bmm_limits (host only): *max_K = 64, *max_D = 1024.
 *   vmp_bmm_plan (host only): for (N, D, K) the rows of a chunk *chunk_rows (one workgroup, a
 *     function of (N, D, K) alone) and the scratch *workspace_doubles of the pass (below 2^25 + a
 *     few thousand doubles at every size).
 *   vmp_bmm_pack: x (N x D, row-major; dtype 0 = float64, 1 = int64, 2 = bool / uint8) to
 *     ceil(D / 64) 64-bit words per row, bit d of a row in bit d & 63 of word d >> 6, unused high
 *     bits zero; *flag (device int32, cleared by the caller) is set when a value is neither 0 nor
 *     1 -- the check of Bernoulli's observe (binomial.py: "Invalid count").
 *   vmp_bmm_tables: from the Beta moments elog_p ((D K, 2): <log p>, <log(1 - p)>; NULL = no
 *     observation term, the moments of Z under its prior) and elog_pi (K) the tables of the pass,
 *     w[d, k] = <log p> - <log(1 - p)> (D x K) and c[k] = <log pi_k> + sum_d <log(1 - p_dk)> --
 *     what mixture.py's (N, D, K) broadcast of x <log p> + (1 - x) <log(1 - p)> summed over D and
 *     the message of the Categorical parent amount to for binary x.  c is written less its largest
 *     element: r, the statistics and the entropy sum lse - sum Nk c - sum S w do not depend on a
 *     constant in c, and a <log pi> near -1e5 (a Dirichlet prior of 1e-5) stays out of the
 *     rounding of every logit; lse is relative to that constant.
 *   vmp_bmm_pass: for every row logit = c + x w, lse = max + log sum exp(logit - max), r =
 *     exp(logit - lse) (categorical.py: the update of Z), both products on the fp64 matrix cores.
 *     Out: S (D x K) = sum_n r_nk x_nd and Nk (K) = sum_n r_nk; counts ((D K, 2)) = (S, Nk - S),
 *     the message of the mixture to the Beta parent (mixture.py, bernoulli.py / binomial.py);
 *     scal[0] = sum lse, scal[1] = sum Nk c, scal[2] = sum S w; with r_out (N x K, the caller's
 *     row order) also r itself.  `labels` (N int32) non-NULL: r is the one-hot array of these
 *     classes instead and lse = 0.  ws: vmp_bmm_plan's doubles.  No atomics: the bits of every
 *     output depend on the inputs and (N, D, K) only, with or without r_out.  N = 0 gives zeros.
 *     Tables that are not finite (a point mass at p = 0 or 1) are outside the contract: the
 *     reference forms 0 * -inf = NaN there as well.  K or D above the limits:
 *     VMP_ERR_UNSUPPORTED; null / negative arguments: VMP_ERR_INVALID. */
int32_t vmp_bmm_limits(int32_t *max_K, int32_t *max_D);
int32_t vmp_bmm_plan(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                     int64_t *workspace_doubles);
int32_t vmp_bmm_pack(vmp_ctx *ctx, int64_t N, int32_t D, int32_t dtype, const void *x,
                     uint64_t *xw, int32_t *flag);
int32_t vmp_bmm_tables(vmp_ctx *ctx, int32_t D, int32_t K, const double *elog_p,
                       const double *elog_pi, double *w, double *c);
int32_t vmp_bmm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, const uint64_t *xw,
                     const int32_t *labels, const double *w, const double *c, double *ws,
                     double *S, double *Nk, double *counts, double *scal, double *r_out);

/* Bernoulli mixture with missing observations: X.observe(x, mask=m), m of the full shape (N, D),
 * 1 = observed (details: vmp_bmm_dev.h).  A row is two bit planes, 2 ceil(D / 64) words: x & m,
 * then m; with xm = x & m
 *     logit_nk = c[k] + sum_d xm_nd w[d, k] + sum_d m_nd l0[d, k]
 *     S_dk = sum_n r_nk xm_nd,  M_dk = sum_n r_nk m_nd,  N_k = sum over the observed rows of r_nk.
 *   vmp_bmm_limits_masked (host only): *max_K = 64, *max_D = 1024.
 *   vmp_bmm_plan_masked (host only): as vmp_bmm_plan for partials of 2 D K + K + 1 doubles per
 *     chunk, under the same caps.
 *   vmp_bmm_pack_masked: x as for vmp_bmm_pack and mask (N x D uint8, non-zero = observed) to
 *     2 W words per row, W = ceil(D / 64): words 0 .. W-1 hold x & m, words W .. 2W-1 hold m,
 *     unused high bits zero.  *flag is set only for an OBSERVED value that is neither 0 nor 1.  A
 *     hidden position is never interpreted: NaN, -1 or 7 may stand there.  (The reference checks
 *     hidden values as well and raises "Invalid count" for them.)
 *   vmp_bmm_tables_masked: w[d, k] = <log p> - <log(1 - p)>, l0[d, k] = <log(1 - p)> (both D x K)
 *     and c[k] = <log pi_k> - max_k <log pi_k>; sum_d l0 is not in c.  elog_p == NULL gives
 *     w = l0 = 0, the moments of Z under its prior.
 *   vmp_bmm_pass_masked: the pass of vmp_bmm_pass on the two planes: plane 0 against w in
 *     ascending d, then plane 1 against l0 in ascending d, then c.  Out: S, M (D x K), Nk (K),
 *     counts ((D K, 2)) = (S, M - S), scal[0] = sum lse over the observed rows, scal[1] = Nk . c,
 *     scal[2] = S . w + M . l0; r_out (N x K) if not NULL.  A row with no observed bit has
 *     r = softmax(c) (with labels: its one-hot row), written to r_out, and adds exactly nothing
 *     to Nk, sum lse, S and M.  ws: vmp_bmm_plan_masked's doubles.  No atomics: the bits of every
 *     output depend on the inputs and (N, D, K) only, with or without r_out and whatever stands
 *     at hidden positions.  Limits and argument errors as for vmp_bmm_pass. */
int32_t vmp_bmm_limits_masked(int32_t *max_K, int32_t *max_D);
int32_t vmp_bmm_plan_masked(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                            int64_t *workspace_doubles);
int32_t vmp_bmm_pack_masked(vmp_ctx *ctx, int64_t N, int32_t D, int32_t dtype, const void *x,
                            const uint8_t *mask, uint64_t *xw, int32_t *flag);
int32_t vmp_bmm_tables_masked(vmp_ctx *ctx, int32_t D, int32_t K, const double *elog_p,
                              const double *elog_pi, double *w, double *l0, double *c);
int32_t vmp_bmm_pass_masked(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, const uint64_t *xw,
                            const int32_t *labels, const double *w, const double *l0,
                            const double *c, double *ws, double *S, double *M, double *Nk,
                            double *counts, double *scal, double *r_out);

/* Diagonal-Gaussian mixture: the fused block of
 *     alpha = Dirichlet(a);  Z = Categorical(alpha, plates=(N, 1))
 *     mu = GaussianARD(m0, beta0, plates=(D, K));  tau = Gamma(a0, b0, plates=(D, K))
 *     Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y)
 * (details: bayespy_amd/csrc/vmp_dgmm.hip, vmp_dgmm_dev.h).  N rows of D real observations, K
 * clusters; no (N, D, K) or (N, K) array exists.  With h = <tau><mu>, q = -1/2 <tau> and
 * g = 1/2 <log tau> - 1/2 <tau><mu^2> (D x K) the logit of row n is c[k] + sum_d y_nd h[d, k] +
 * y_nd^2 q[d, k]; the constant -1/2 log 2 pi per element is the same for every k and is left to
 * the caller (-1/2 N D log 2 pi in the bound term of Y).
 *   vmp_dgmm_limits (host only): *max_K = 64, *max_D = 1024.
 *   vmp_dgmm_plan (host only): for (N, D, K) the rows of a chunk *chunk_rows (one workgroup, a
 *     function of (N, D, K) alone; at most 1024 chunks and 2^25 doubles of partials of 2 D K + K +
 *     1 doubles each) and the scratch *workspace_doubles of the pass.
 *   vmp_dgmm_tables: from the moments of mu ((D K, 2): <mu>, <mu^2>), of tau ((D K, 2): <tau>,
 *     <log tau>) and elog_pi (K) the tables h, q (D x K) and c[k] = <log pi_k> + sum_d g[d, k] less
 *     its largest element (r, the statistics and the entropy do not depend on a constant in c; lse
 *     is relative to it); gsum (K), if not NULL, receives sum_d g[d, k].  A NULL moment table gives
 *     h = q = 0, gsum = 0 and c from <log pi> alone: Z under its prior.
 *   vmp_dgmm_pass: per tile of 64 rows logit = Y h + (Y o Y) q, then + c; lse = max + log sum
 *     exp(logit - max), r = exp(logit - lse); S1 += r^T Y, S2 += r^T (Y o Y), all four products on
 *     the fp64 matrix cores.  Out: S1, S2 (D x K), Nk (K), scal[0] = sum lse, scal[1] = Nk . c,
 *     scal[2] = S1 . h + S2 . q; with r_out (N x K) also r itself.  `labels` (N int32) non-NULL: r
 *     is the one-hot array of these classes and lse = 0.  ws: vmp_dgmm_plan's doubles.  No atomics:
 *     the bits of every output depend on the inputs and (N, D, K) only, with or without r_out.
 *     N = 0 gives zeros.  y or tables that are not finite are outside the contract.
 *   vmp_dgmm_update: one launch for one node, from the statistics and the present moments
 *     `other_mom` ((D K, 2)) of the other node; priors as dense (D, K) tables.
 *       which = 0, q(mu): prior_a = m0, prior_b = beta0, other_mom = moments of tau;
 *         lambda = beta0 + <tau> Nk, m = (beta0 m0 + <tau> S1) / lambda; par = (m, lambda),
 *         mom = (m, m^2 + 1 / lambda).
 *       which = 1, q(tau): prior_a = a0, prior_b = b0, other_mom = moments of mu;
 *         a = a0 + Nk / 2, b = b0 + (S2 - 2 <mu> S1 + <mu^2> Nk) / 2; par = (a, b),
 *         mom = (a / b, psi(a) - log b).
 *     *bound = <log p(node)> - <log q(node)> (expfamily.py:400-480) summed over (D, K) in a fixed
 *     order.  NULL statistics (any of S1, S2, Nk, other_mom) give the prior.
 *   K or D above the limits: VMP_ERR_UNSUPPORTED; null / negative arguments: VMP_ERR_INVALID. */
int32_t vmp_dgmm_limits(int32_t *max_K, int32_t *max_D);
int32_t vmp_dgmm_plan(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                      int64_t *workspace_doubles);
int32_t vmp_dgmm_tables(vmp_ctx *ctx, int32_t D, int32_t K, const double *mu_mom,
                        const double *tau_mom, const double *elog_pi, double *h, double *q,
                        double *c, double *gsum);
int32_t vmp_dgmm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, const double *y,
                      const int32_t *labels, const double *h, const double *q, const double *c,
                      double *ws, double *S1, double *S2, double *Nk, double *scal, double *r_out);
int32_t vmp_dgmm_update(vmp_ctx *ctx, int32_t D, int32_t K, int32_t which, const double *prior_a,
                        const double *prior_b, const double *S1, const double *S2,
                        const double *Nk, const double *other_mom, double *par, double *mom,
                        double *bound);
/* Deterministic annealing on this block (see vmp_gmm_*_annealed above for the semantics).
 *   vmp_dgmm_tables_annealed: h, q and c times `annealing` (c less its maximum AFTER the scaling);
 *       gsum is not scaled, it feeds L_Y.
 *   vmp_dgmm_update_annealed: which 0 (mu) / 1 (tau): the update with every natural parameter times
 *       `annealing`; the bound term comes in two parts, ab[0] = A (cgf from the parents + phi_p . u)
 *       and ab[1] = B (phi_q . u + g_q): the caller forms A - T B with the temperature the node has
 *       when the bound is asked for.  which 2 (mu) / 3 (tau): A and B alone of the q that par and mom
 *       hold (whatever update or initialisation made it); the statistics are not read.
 * With annealing = 1 the tables, par and mom are those of the plain entry points bit for bit. */
int32_t vmp_dgmm_tables_annealed(vmp_ctx *ctx, int32_t D, int32_t K, double annealing,
                                 const double *mu_mom, const double *tau_mom, const double *elog_pi,
                                 double *h, double *q, double *c, double *gsum);
int32_t vmp_dgmm_update_annealed(vmp_ctx *ctx, int32_t D, int32_t K, int32_t which,
                                 double annealing, const double *prior_a, const double *prior_b,
                                 const double *S1, const double *S2, const double *Nk,
                                 const double *other_mom, double *par, double *mom, double *ab);

/* The same block with missing observations, Y.observe(y, mask=m) with m of the full shape (N, D)
 * (details: bayespy_amd/csrc/vmp_dgmm_masked.hip, vmp_dgmm_masked_dev.h).  With yt = m o y the logit
 * of row n is c[k] + sum_d m_nd g[d, k] + yt_nd h[d, k] + yt_nd^2 q[d, k]: sum_d g leaves c and
 * becomes a third product, and the count of an element M[d, k] = sum_n r_nk m_nd takes the place of
 * N_k in both updates.  A row with nothing observed has r = softmax(c) (one-hot under labels) and
 * enters neither Nk nor sum lse; a column with nothing observed has M = S1 = S2 = 0 exactly.
 *   vmp_dgmm_limits_masked (host only): *max_K = 64, *max_D = 1024.
 *   vmp_dgmm_plan_masked (host only): as vmp_dgmm_plan, for partials of 3 D K + K + 1 doubles.
 *   vmp_dgmm_pack_masked: y_packed (N x D) = y where mask (N x D bytes) is non-zero and one fixed
 *     quiet-NaN bit pattern elsewhere, chosen by a select: what y holds at a hidden position (NaN,
 *     inf, 1e300) reaches nothing.  *n_observed (device) receives the number of observed entries.
 *     The pass finds the mask again as y_packed == y_packed and reads no other array of size N D.
 *   vmp_dgmm_tables_masked: h, q, g (D x K) and c = elog_pi less its largest element.  A NULL moment
 *     table gives h = q = g = 0: Z under its prior.
 *   vmp_dgmm_pass_masked: the pass of vmp_dgmm_pass on y_packed with the three products.  Out: S1,
 *     S2, M (D x K), Nk (K, over the rows with an observed entry), scal[0] = sum lse over the same
 *     rows, scal[1] = Nk . c, scal[2] = S1 . h + S2 . q + M . g; r_out and labels as in
 *     vmp_dgmm_pass.  ws: vmp_dgmm_plan_masked's doubles.  No atomics: the bits of every output
 *     depend on y_packed, the tables and (N, D, K) only.
 *   vmp_dgmm_update_masked: vmp_dgmm_update with M (D x K) in the place of Nk (K).
 *   K or D above the limits: VMP_ERR_UNSUPPORTED; null / negative arguments: VMP_ERR_INVALID. */
int32_t vmp_dgmm_limits_masked(int32_t *max_K, int32_t *max_D);
int32_t vmp_dgmm_plan_masked(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                             int64_t *workspace_doubles);
int32_t vmp_dgmm_pack_masked(vmp_ctx *ctx, int64_t N, int32_t D, const double *y,
                             const uint8_t *mask, double *y_packed, int64_t *n_observed);
int32_t vmp_dgmm_tables_masked(vmp_ctx *ctx, int32_t D, int32_t K, const double *mu_mom,
                               const double *tau_mom, const double *elog_pi, double *h, double *q,
                               double *g, double *c);
int32_t vmp_dgmm_pass_masked(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, const double *y_packed,
                             const int32_t *labels, const double *h, const double *q,
                             const double *g, const double *c, double *ws, double *S1, double *S2,
                             double *M, double *Nk, double *scal, double *r_out);
int32_t vmp_dgmm_update_masked(vmp_ctx *ctx, int32_t D, int32_t K, int32_t which,
                               const double *prior_a, const double *prior_b, const double *S1,
                               const double *S2, const double *M, const double *other_mom,
                               double *par, double *mom, double *bound);

/* Hidden Markov model with Gaussian emissions: the chain pass of the fused block
 * (doc/source/examples/hmm.rst; details: bayespy_amd/csrc/vmp_hmm_fused.hip, vmp_hmm_fused_dev.h).
 * B chains of T time instances, D-dimensional observations, K states.  No (B, T-1, K, K) array is
 * read or written unless `zz` is asked for; the forward state kept per step is K doubles.
 *   vmp_hmm_fused_limits (host only): *max_K = 64, *max_D = 8.
 *   vmp_hmm_fused_plan (host only): for (B, T, D, K) the chains of a workgroup *chains_per_wg (a
 *     function of the shape alone) and the scratch *workspace_doubles of the pass
 *     (B T K + partials + 1024).
 *   vmp_hmm_fused_pass: Y (B, T, D) row-major; C (K rows of stride ldc) the coefficients of
 *     e_t[k] = E[log p(y_t | k)] in the compact feature order of vmp_gmm_prepare_z (y_a y_b for
 *     a <= b, then y_d, then 1: the C table of a vmp_gmm_layout state whose <log pi> slot is
 *     zero), or NULL for no emission term (the moments of Z under its prior); elog_a0 (K),
 *     elog_A (K x K).  The forward-backward recursion of random.alpha_beta_recursion on
 *     logp0 = elog_a0 + e_0, logP[n] = elog_A + e_{n+1}, in the log domain throughout.
 *     Out: z0sum (K) = sum_b gamma_{b,0}; xisum (K x K) = sum_{b,t} xi_{b,t}; Tstat (K rows
 *     [sum gamma, sum gamma y, sum gamma y y^T] of length 1 + D + D^2: the T of vmp_gmm_layout);
 *     scal[0] = sum_b log Z_b, scal[1] = sum gamma . e, scal[2] = z0sum . elog_a0,
 *     scal[3] = xisum . elog_A.  With gamma (B, T, K), z0 (B, K), zz (B, T-1, K, K) non-NULL also
 *     these.  `labels` (B x T int32) non-NULL: gamma and xi are the one-hot arrays of these states
 *     instead, log Z = 0 and scal[1] = 0.  ws: vmp_hmm_fused_plan's doubles.  No atomics: the bits
 *     of every output depend on the inputs and (B, T, D, K) only, with or without the optional
 *     outputs.  A state with -inf in elog_a0 or in a column of elog_A gets 0 in gamma, xi and the
 *     sums; scal[2] and scal[3] are plain dot products with the tables as given, so they are
 *     0 * -inf = NaN for such tables (the tables of a Dirichlet node are finite).  A step whose
 *     logits are all -inf gives NaN, as in the reference.  B = 0 gives zeros.  The shape is judged
 *     before the pointers: T < 2 or a negative size: VMP_ERR_INVALID; K or D above the limits:
 *     VMP_ERR_UNSUPPORTED; then ldc below the number of features or a null argument:
 *     VMP_ERR_INVALID.  Nothing is launched after a refusal.
 *   vmp_hmm_fused_pass_masked: the same pass with missing observations.  mask (B x T bytes,
 *     1 = observed) or NULL, which is vmp_hmm_fused_pass.  A masked step has e_t = 0 (a zero
 *     message to Z) and adds nothing to Tstat or scal[1]; it stays a step of the chain, so
 *     trailing masked steps propagate through elog_A and their xi counts.  Y at a masked step is
 *     never read: NaN may stand there.  A chain without an observed step adds nothing to z0sum,
 *     xisum, scal[0] or scal[1]; its gamma, z0 and zz are what the recursion gives with e = 0
 *     throughout.  With `labels` the one-hot sums of Tstat run over the observed steps, and z0sum
 *     and xisum skip the chains without one.  A mask of ones gives the bits of
 *     vmp_hmm_fused_pass.  The same limits (64, 8), the same workspace, the same checks in the
 *     same order; no atomics. */
int32_t vmp_hmm_fused_limits(int32_t *max_K, int32_t *max_D);
int32_t vmp_hmm_fused_plan(int64_t B, int32_t T, int32_t D, int32_t K, int64_t *chains_per_wg,
                           int64_t *workspace_doubles);
int32_t vmp_hmm_fused_pass(vmp_ctx *ctx, int64_t B, int32_t T, int32_t D, int32_t K,
                           const double *Y, const double *C, int32_t ldc, const double *elog_a0,
                           const double *elog_A, const int32_t *labels, double *ws,
                           double *z0sum, double *xisum, double *Tstat, double *scal,
                           double *gamma, double *z0, double *zz);
int32_t vmp_hmm_fused_pass_masked(vmp_ctx *ctx, int64_t B, int32_t T, int32_t D, int32_t K,
                                  const double *Y, const double *C, int32_t ldc,
                                  const double *elog_a0, const double *elog_A,
                                  const int32_t *labels, const uint8_t *mask, double *ws,
                                  double *z0sum, double *xisum, double *Tstat, double *scal,
                                  double *gamma, double *z0, double *zz);

/* Hidden Markov model with categorical emissions (the discrete HMM of hmm.rst's first half): the
 * chain pass of the fused block (bayespy_amd/csrc/vmp_hmm_cat.hip, vmp_hmm_fused_dev.h).  B chains
 * of T time instances, words y_t in [0, M), K states.  The recursion, the lane mapping, the mask
 * rules and the order of the additions are those of vmp_hmm_fused_pass_masked; the emission term
 * is a table lookup.
 *   vmp_hmm_fused_cat_limits (host only): *max_K = 64, *max_M = 128 (a workgroup keeps 512 M
 *     bytes of count accumulators in LDS).
 *   vmp_hmm_fused_cat_plan (host only): for (B, T, M, K) the chains of a workgroup *chains_per_wg
 *     (a function of the shape alone) and the scratch *workspace_doubles of the pass
 *     (B T K + partials + 1024).
 *   vmp_hmm_fused_pass_categorical: y (B, T) int32 words; elogPt (M, K) = <log P> WORD-MAJOR
 *     (element (m, k) at m K + k), or NULL for no emission term; elog_a0 (K), elog_A (K x K);
 *     labels (B x T int32) or NULL; mask (B x T bytes, 1 = observed) or NULL (everything
 *     observed).  e_t[k] = elogPt[y_t][k] at an observed step, 0 at a masked one, whose y_t is
 *     never read (any integer may stand there).  PRECONDITION: every observed word lies in
 *     [0, M); the caller validates them.  A word outside that range never indexes anything: its
 *     step is treated as masked (the chain weight is taken from the mask alone).
 *     Out: z0sum (K), xisum (K x K) as in vmp_hmm_fused_pass; S (M, K) word-major =
 *     sum over the observed (b, t) with y = m of gamma_{b,t,k}; scal[0] = sum_b log Z_b,
 *     scal[1] = sum gamma . e, scal[2] = z0sum . elog_a0, scal[3] = xisum . elog_A; with gamma
 *     (B, T, K), z0 (B, K), zz (B, T-1, K, K) non-NULL also these.  A chain without an observed
 *     step adds nothing to any sum.  ws: vmp_hmm_fused_cat_plan's doubles.  No atomics: the bits
 *     of every output depend on the inputs and (B, T, M, K) only; a mask of ones gives the bits of
 *     a NULL mask.  B = 0 gives zeros.  The shape is judged before the pointers: T < 2 or a
 *     size below 1 (B below 0): VMP_ERR_INVALID; K or M above the limits: VMP_ERR_UNSUPPORTED;
 *     then a null required argument: VMP_ERR_INVALID.  Nothing is launched after a refusal. */
int32_t vmp_hmm_fused_cat_limits(int32_t *max_K, int32_t *max_M);
int32_t vmp_hmm_fused_cat_plan(int64_t B, int32_t T, int32_t M, int32_t K, int64_t *chains_per_wg,
                               int64_t *workspace_doubles);
int32_t vmp_hmm_fused_pass_categorical(vmp_ctx *ctx, int64_t B, int32_t T, int32_t M, int32_t K,
                                       const int32_t *y, const double *elogPt,
                                       const double *elog_a0, const double *elog_A,
                                       const int32_t *labels, const uint8_t *mask, double *ws,
                                       double *z0sum, double *xisum, double *S, double *scal,
                                       double *gamma, double *z0, double *zz);

/* Categorical mixture (latent class model): the plate pass of the fused block
 *     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
 *     P = Dirichlet(conc, plates=(D, K));  X = Mixture(Z, Categorical, P);  X.observe(x[, mask])
 * (details: bayespy_amd/csrc/vmp_cmm.hip, vmp_cmm_dev.h).  N rows of D observations in [0, M), K
 * clusters; x is kept as one byte per entry, 255 = hidden; <log P> and the counts S are
 * CATEGORY-MAJOR, element (m, d, k) at (m D + d) K + k.  No (N, K), (N, D, K) or (N, D, M) array
 * exists.
 *   vmp_cmm_limits (host only): *max_K = 64, *min_M = 2, *max_M = 32 and *max_cells, the doubles of
 *     the count table a workgroup keeps in LDS: roundup(D, 64 / KP) M KP <= *max_cells with
 *     KP = 16, 32 or 64 the lanes that hold the K clusters.
 *   vmp_cmm_plan (host only): for (N, D, K, M) the rows of a chunk *chunk_rows (one workgroup, a
 *     function of the shape alone) and the scratch *workspace_doubles of the pass.  A shape above
 *     the limits: VMP_ERR_UNSUPPORTED.
 *   vmp_cmm_pack: x (N x D, row-major; dtype 0 = float64, 1 = int64, 2 = uint8, 3 = int32) and
 *     mask (N x D bytes, non-zero = observed, or NULL: everything observed) to N D bytes.  A hidden
 *     position gets 255 by a select whatever stands there (NaN, -1, 1e300).  An OBSERVED value that
 *     is no integer in [0, M) gets 255 as well and sets *flag (device int32, cleared by the
 *     caller): categorical.py's "Invalid category index".
 *   vmp_cmm_tables: L = elog_p ((M, D K) category-major; NULL: zeros, the moments of Z under its
 *     prior) and c[k] = elog_pi[k] - max_k elog_pi[k].
 *   vmp_cmm_pass: logit_nk = c[k] + sum over the observed d of L[x_nd, d, k] (ascending d, c last),
 *     lse and r = exp(logit - lse) over a lane group.  A byte b is observed when (unsigned) b < M;
 *     no other byte ever becomes an address.  Out: S (M, D K) = sum_n r_nk [x_nd = m], Nk (K) and
 *     scal[0] = sum lse over the rows with an observed entry, scal[1] = Nk . c, scal[2] = S . L;
 *     with r_out (N x K) also r.  A row with nothing observed has r = softmax(c) (with labels: its
 *     one-hot row), written to r_out, and adds exactly nothing to any sum.  `labels` (N int32)
 *     non-NULL: r is one-hot, lse = 0 and L is not read.  ws: vmp_cmm_plan's doubles.  No atomics,
 *     in LDS or in memory: the bits of every output depend on the inputs and (N, D, K, M) only,
 *     with or without r_out.  N = 0 gives zeros.  The shape is judged before the pointers: a size
 *     below 1 (N below 0): VMP_ERR_INVALID; above the limits: VMP_ERR_UNSUPPORTED; then a null
 *     required argument: VMP_ERR_INVALID.  Nothing is launched after a refusal. */
int32_t vmp_cmm_limits(int32_t *max_K, int32_t *min_M, int32_t *max_M, int32_t *max_cells);
int32_t vmp_cmm_plan(int64_t N, int32_t D, int32_t K, int32_t M, int64_t *chunk_rows,
                     int64_t *workspace_doubles);
int32_t vmp_cmm_pack(vmp_ctx *ctx, int64_t N, int32_t D, int32_t M, int32_t dtype, const void *x,
                     const uint8_t *mask, uint8_t *xb, int32_t *flag);
int32_t vmp_cmm_tables(vmp_ctx *ctx, int32_t D, int32_t K, int32_t M, const double *elog_p,
                       const double *elog_pi, double *L, double *c);
int32_t vmp_cmm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, int32_t M, const uint8_t *xb,
                     const int32_t *labels, const double *L, const double *c, double *ws,
                     double *S, double *Nk, double *scal, double *r_out);

/* Poisson mixture: the plate pass and the update of the fused block
 *     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
 *     lam = Gamma(a0, b0, plates=(D, K));  X = Mixture(Z, Poisson, lam);  X.observe(x[, mask])
 * (details: bayespy_amd/csrc/vmp_pmm.hip, vmp_pmm_dev.h).  N rows of D counts, K clusters; x is
 * kept as one uint16 per entry, 0xFFFF = hidden; tables and statistics are (D x K), element (d, k)
 * at d K + k; moment and parameter tables are (D K, 2): (<lam>, <log lam>) and (a, b).  No (N, K)
 * or (N, D, K) array exists.
 *   vmp_pmm_limits (host only): *max_K = 64, *max_D = 1024, *max_count = 65534.
 *   vmp_pmm_plan (host only): for (N, D, K) the rows of a chunk *chunk_rows (one workgroup, a
 *     function of the shape alone) and the scratch *workspace_doubles of the pass, which is never
 *     below what vmp_pmm_pack needs (2048 doubles).
 *   vmp_pmm_pack: x (N x D, row-major; dtype 0 = float64, 1 = int64, 2 = uint8, 3 = int32) and
 *     mask (N x D bytes, non-zero = observed, or NULL: everything observed) to N D uint16.  A
 *     hidden position gets 0xFFFF by a select whatever stands there (NaN, -1, 1e300).  An OBSERVED
 *     value that is negative or no integer gets 0xFFFF as well and sets flags[0] (and flags[2] when
 *     it is no integer: which of poisson.py's two messages applies); one above 65534 sets flags[1].
 *     The checks come before any conversion to an integer.  flags: three device int32, cleared by
 *     the caller.  counts[0] = the observed entries, counts[1] = the hidden ones (device int64);
 *     *lgam = sum over the observed entries of lgamma(x + 1), per-block partials added in block
 *     order, no atomics.  ws: 2048 doubles.
 *   vmp_pmm_tables: l = <log lam>, lb = <lam>, lsum[k] = sum_d lb[d, k] (or NULL) and
 *     c = elog_pi - lsum (nothing hidden) or elog_pi (bit 1 of form: hidden entries), less its
 *     largest element.  Bit 2 of form: the tables of the pass, CENTRED -- column 0 of every row is
 *     taken out of l and lb (and so of lsum), which moves all logits of a row alike: r and
 *     scal[0] - scal[1] - scal[2] of the pass do not change, the logits stay small.  A NULL
 *     lam_mom gives l = lb = 0: Z under its prior.
 *   vmp_pmm_pass: hidden = 0: logit_nk = c[k] + sum_d x_nd l[d, k]; Out: S (D x K) = r^T x, Nk and
 *     scal[0] = sum lse, scal[1] = Nk . c, scal[2] = S . l; M and lb are not touched.  hidden = 1:
 *     logit_nk = c[k] + sum_d xt_nd l[d, k] - m_nd lb[d, k] with m = (x != 0xFFFF), xt = m o x; Out:
 *     S = r^T xt, M = r^T m, Nk and scal[0] over the rows with an observed entry, scal[2] =
 *     S . l - M . lb.  A row with nothing observed has r = softmax(c) (with labels: its one-hot
 *     row), written to r_out, and adds nothing to Nk and scal[0].  `labels` (N int32) non-NULL: r
 *     is one-hot, lse = 0.  r_out (N x K) is written on request only.  ws: vmp_pmm_plan's doubles.
 *     No atomics: the bits of every output depend on x_packed, the tables and (N, D, K) only, with
 *     or without r_out.  N = 0 gives zeros.  x_packed must be 2-byte aligned (8 for the fast loads).
 *   vmp_pmm_update: one launch; a = a0 + S, b = b0 + cnt with cnt = Nk (K; per_element = 0) or M
 *     (D x K; per_element = 1); par = (a, b), mom = (a / b, psi(a) - log b), *bound = <log p(lam)> -
 *     <log q(lam)>, exactly zero for an element at its prior.  S or cnt NULL: the prior.
 *   The shape is judged before the pointers: a size below 1 (N below 0): VMP_ERR_INVALID; K or D
 *   above the limits: VMP_ERR_UNSUPPORTED; then a null required argument: VMP_ERR_INVALID.  Nothing
 *   is launched after a refusal. */
int32_t vmp_pmm_limits(int32_t *max_K, int32_t *max_D, int32_t *max_count);
int32_t vmp_pmm_plan(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                     int64_t *workspace_doubles);
int32_t vmp_pmm_pack(vmp_ctx *ctx, int64_t N, int32_t D, int32_t dtype, const void *x,
                     const uint8_t *mask, uint16_t *x_packed, int32_t *flags, int64_t *counts,
                     double *lgam, double *ws);
int32_t vmp_pmm_tables(vmp_ctx *ctx, int32_t D, int32_t K, int32_t form, const double *lam_mom,
                       const double *elog_pi, double *l, double *lb, double *c, double *lsum);
int32_t vmp_pmm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, int32_t hidden,
                     const uint16_t *x_packed, const int32_t *labels, const double *l,
                     const double *lb, const double *c, double *ws, double *S, double *M,
                     double *Nk, double *scal, double *r_out);
int32_t vmp_pmm_update(vmp_ctx *ctx, int32_t D, int32_t K, int32_t per_element,
                       const double *prior_a, const double *prior_b, const double *S,
                       const double *cnt, double *par, double *mom, double *bound);

/* The fused multinomial-mixture block (mixture of unigrams, count-vector clustering):
 *     R = Dirichlet(a);  Z = Categorical(R, plates=(N,))
 *     P = Dirichlet(a0, plates=(K,)) over M words;  X = Mixture(Z, Multinomial, n, P);  X.observe(x)
 * (details: bayespy_amd/csrc/vmp_mmm.hip, vmp_mmm_dev.h).  N rows of M counts that add up to the
 * row's number of trials, K clusters; x is kept as one uint16 per entry.  <log p> and the statistic
 * S are (K x M), element (k, m) at k M + m: K Dirichlet rows for vmp_lda_dirichlet (rows K, cols M,
 * row_stride M, col_stride 1).  The table of the pass is (M x K), word-major.  No (N, K) or
 * (N, K, M) array exists.
 *   vmp_mmm_limits (host only): *max_K = 64, *max_M = 1024, *max_count = 65534.
 *   vmp_mmm_plan (host only): for (N, M, K) the rows of a chunk *chunk_rows (one workgroup, a
 *     function of the shape alone) and the scratch *workspace_doubles of the pass, which is never
 *     below what vmp_mmm_pack needs (1024 doubles).
 *   vmp_mmm_pack: x (N x M, row-major; dtype 0 = float64, 1 = int64, 2 = uint8, 3 = int32) and
 *     trials (N int64) to N M uint16.  A value that is negative or no integer sets flags[0] (no
 *     integer: flags[2] as well), one above 65534 sets flags[1]; such an entry is packed as zero.
 *     A row of valid counts that do not add up to its trials sets flags[3].  flags (4 int32) are
 *     only ever set.  *lcoef = sum_n [lgamma(trials_n + 1) - sum_m lgamma(x_nm + 1)], per-block
 *     partials added in block order, no atomics.  ws: 1024 doubles.
 *   vmp_mmm_tables: L[m, k] = elog_p[k, m] - elog_p[0, m] (CENTRED: cluster 0 taken out of every
 *     word, which moves all logits of a row by one amount, so r and scal[0] - scal[1] - scal[2] of
 *     the pass do not change) and c = elog_pi less its largest element.  A NULL elog_p gives
 *     L = 0: Z under its prior.
 *   vmp_mmm_pass: logit_nk = c[k] + sum_m x_nm L[m, k]; Out: S (K x M) = r^T x, Nk and
 *     scal[0] = sum lse, scal[1] = Nk . c, scal[2] = S . L.  `labels` (N int32) non-NULL: r is
 *     one-hot, lse = 0.  r_out (N x K) is written on request only.  ws: vmp_mmm_plan's doubles.
 *     No atomics: the bits of every output depend on x_packed, the tables and (N, M, K) only, with
 *     or without r_out.  N = 0 gives zeros.  x_packed must be 2-byte aligned (8 for the fast loads).
 *   Order of the checks: null context, negative or zero sizes: VMP_ERR_INVALID; then K or M above
 *   the limits: VMP_ERR_UNSUPPORTED; then a null required argument: VMP_ERR_INVALID.  Nothing is
 *   launched after a refusal. */
int32_t vmp_mmm_limits(int32_t *max_K, int32_t *max_M, int32_t *max_count);
int32_t vmp_mmm_plan(int64_t N, int32_t M, int32_t K, int64_t *chunk_rows,
                     int64_t *workspace_doubles);
int32_t vmp_mmm_pack(vmp_ctx *ctx, int64_t N, int32_t M, int32_t dtype, const void *x,
                     const int64_t *trials, uint16_t *x_packed, int32_t *flags, double *lcoef,
                     double *ws);
int32_t vmp_mmm_tables(vmp_ctx *ctx, int32_t M, int32_t K, const double *elog_p,
                       const double *elog_pi, double *L, double *c);
int32_t vmp_mmm_pass(vmp_ctx *ctx, int64_t N, int32_t M, int32_t K, const uint16_t *x_packed,
                     const int32_t *labels, const double *L, const double *c, double *ws,
                     double *S, double *Nk, double *scal, double *r_out);

/* Binomial mixture (successes out of trials): the pack, the tables and the plate pass of the fused block
 *     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
 *     P = Beta(a0, plates=(D, K));  X = Mixture(Z, Binomial, n, P);  X.observe(x[, mask])
 * (details: bayespy_amd/csrc/vmp_binm.hip, vmp_binm_dev.h).  N rows of D counts x_nd out of n_nd
 * trials, K clusters; counts and trials are kept as one uint16 per entry each (two planes), a hidden
 * entry as count 0 and trials 0xFFFF; tables and statistics are (D x K), element (d, k) at d K + k;
 * elog_p and counts are (D K, 2): (<log p>, <log(1 - p)>) and (S, T - S), the Dirichlet rows of two
 * columns that vmp_lda_dirichlet updates (alpha = alpha0 + S, beta = beta0 + T - S, the bound
 * exactly zero for an element at its prior) as for the Bernoulli block.  No (N, K) or (N, D, K)
 * array exists.
 *   vmp_binm_limits (host only): *max_K = 64, *max_D = 1024, *max_trials = 65534.
 *   vmp_binm_plan (host only): for (N, D, K) the rows of a chunk *chunk_rows (one workgroup, a
 *     function of the shape alone) and the scratch *workspace_doubles of the pass, which is never
 *     below what vmp_binm_pack needs (3072 doubles).
 *   vmp_binm_pack: x (N x D, row-major; dtype 0 = float64, 1 = int64, 2 = uint8, 3 = int32), the
 *     trials of entry (n, d) at trials[n trials_stride_n + d trials_stride_d] (int64, strides in
 *     elements, zero for an axis the trials do not vary along: a scalar, (D, 1), (N, 1, 1) and
 *     (N, D, 1) are read in place) and mask (N x D bytes, non-zero = observed, or NULL) to two planes
 *     of N D uint16.  A hidden position gets trials 0xFFFF and count 0 by a select whatever stands
 *     there (NaN, -1, 1e300).  An OBSERVED entry that fails a check is packed as hidden and sets
 *     one flag: flags[0] a negative count, flags[1] a count that is no integer, flags[2] a count
 *     above its trials, flags[3] trials above 65534.  The checks come before any conversion to an
 *     integer.  flags: four device int32, cleared by the caller.  counts (three device int64):
 *     the observed entries, the hidden ones, and 1 when the trials of every entry equal those of
 *     row 0 of its column (constant along the rows), else 0.  *lcoef = sum over the observed entries
 *     of lgamma(n + 1) - lgamma(x + 1) - lgamma(n - x + 1), per-block partials added in block order,
 *     no atomics.  ws: 3072 doubles.
 *   vmp_binm_tables: l1 = <log p> - <log(1 - p)>, l0 = <log(1 - p)> and c = elog_pi less its
 *     largest element.  Bit 1 of form: the tables of the pass, CENTRED -- column 0 of every row is
 *     taken out of l1 and l0, which moves all logits of a row alike (vmp_pmm_tables).  With ncol
 *     (D doubles, the trials of a column) and cfold non-NULL also cfold[k] = elog_pi[k] +
 *     sum_d ncol[d] l0[d, k] (l0 as written), less its largest element: the c of the one-plane form.
 *     A NULL elog_p gives l1 = l0 = 0: Z under its prior.
 *   vmp_binm_pass: one_plane = 0: logit_nk = c[k] + sum_d xt_nd l1[d, k] + nt_nd l0[d, k] with
 *     m = (n_packed != 0xFFFF), xt = m o x, nt = m o n; Out: S = r^T xt, T = r^T nt (D x K), Nk and
 *     scal[0] = sum lse over the rows with an observed entry, scal[1] = Nk . c, scal[2] = S . l1 +
 *     T . l0 (formed row by row inside the pass as sum_n r_n . (logit_n - c), the same number with
 *     less rounding; with labels from S and T), counts = (S, T - S).  A row with nothing observed has r = softmax(c) (with labels: its
 *     one-hot row), written to r_out, and adds nothing to Nk and scal[0] and zeros to S and T.
 *     ncol is not read.  one_plane = 1, for trials that are constant along the rows with nothing
 *     hidden: c is the cfold of vmp_binm_tables and ncol the trials of the columns; only x_packed is
 *     read, by the kernel of vmp_pmm_pass (hidden = 0, l = l1): logit_nk = c[k] + sum_d x_nd l1[d, k];
 *     Out: S, Nk, scal[0], scal[1] = Nk . c, scal[2] = S . l1, then T[d, k] = ncol[d] Nk[k] and
 *     counts.  `labels` (N int32) non-NULL: r is one-hot, lse = 0.  r_out (N x K) is written on
 *     request only.  ws: vmp_binm_plan's doubles.  No atomics: the bits of every output depend on
 *     the packed planes, the tables and (N, D, K) only, with or without r_out.  N = 0 gives zeros.
 *   Order of the checks: null context, a size below 1 (N below 0), a form, dtype or stride out of
 *   range: VMP_ERR_INVALID; then K or D above the limits: VMP_ERR_UNSUPPORTED; then a null required
 *   argument: VMP_ERR_INVALID.  Nothing is launched after a refusal. */
int32_t vmp_binm_limits(int32_t *max_K, int32_t *max_D, int32_t *max_trials);
int32_t vmp_binm_plan(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                      int64_t *workspace_doubles);
int32_t vmp_binm_pack(vmp_ctx *ctx, int64_t N, int32_t D, int32_t dtype, const void *x,
                      const int64_t *trials, int64_t trials_stride_n, int64_t trials_stride_d,
                      const uint8_t *mask, uint16_t *x_packed, uint16_t *n_packed, int32_t *flags,
                      int64_t *counts, double *lcoef, double *ws);
int32_t vmp_binm_tables(vmp_ctx *ctx, int32_t D, int32_t K, int32_t form, const double *elog_p,
                        const double *elog_pi, const double *ncol, double *l1, double *l0,
                        double *c, double *cfold);
int32_t vmp_binm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, int32_t one_plane,
                      const uint16_t *x_packed, const uint16_t *n_packed, const double *ncol,
                      const int32_t *labels, const double *l1, const double *l0, const double *c,
                      double *ws, double *S, double *T, double *Nk, double *counts, double *scal,
                      double *r_out);

/* Stochastic VI on the count-mixture blocks: the global half of a step in one launch (details:
 * bayespy_amd/csrc/vmp_mix_svi.hip).  The parameter table of the block and the Dirichlet row of the
 * mixing weights move by phi <- phi + scale (phi* - phi) with phi* = prior + mult * statistic; both
 * optima come from the statistics present at entry.  `nodes` is a bit set: 1 = the table, 2 = the
 * weights (K <= 64 contiguous columns: prior_r, Nk (null: the prior), alpha_r, elog_r); what a node
 * that is not named owns is neither read nor written.
 *   kind 0: Dirichlet rows in the addressing of vmp_lda_dirichlet (element (r, c) at r * row_stride +
 *     c * col_stride; cols <= 1024, rows <= 65536, rows * cols <= 2^21): par = alpha, mom = <log>,
 *     stat = the counts (null: the prior); prior_b, cnt, per_element are not used.
 *   kind 1: Gamma pairs in the layout of vmp_pmm_update (cols = 2, rows <= 65536): prior = a0,
 *     prior_b = b0, stat = S, cnt = N_k (per_element 0: rows = D K walked as (D, K), element e reads
 *     cnt[e % K]) or M (per_element 1); a <- a + scale (a0 + mult S - a), b likewise.
 *   scale == 1 does not read the old parameters (they may be NaN) and, with mult == 1, leaves the
 *   parameters and moments of vmp_lda_dirichlet / vmp_pmm_update bit for bit; scale == 0 leaves the
 *   parameters as they are and forms moments and bound again.
 *   bound[0] = <log p> - <log q> of the table (0 for rows == 0), bound[1] that of the weights, each
 *   written only when its node is named.  No floating-point atomics: the workgroups leave partials in
 *   ws (vmp_mix_natural_step_workspace doubles, host only; its last word is the ticket, cleared on the
 *   stream ahead of the launch) and the one that finishes last adds them in index order; the bits of every output depend on the inputs and the shape only.
 *   mult <= 0, a NaN mult or scale, a null required pointer, a negative size, nodes outside 1..3:
 *   VMP_ERR_INVALID, nothing is launched.  K > 64 or a shape beyond the limits above:
 *   VMP_ERR_UNSUPPORTED. */
int32_t vmp_mix_natural_step_workspace(int32_t kind, int64_t rows, int64_t cols, int32_t K,
                                       int64_t *workspace_doubles);
int32_t vmp_mix_natural_step(vmp_ctx *ctx, int32_t kind, int32_t nodes, int64_t rows, int64_t cols,
                             int64_t row_stride, int64_t col_stride, const double *prior,
                             const double *prior_b, const double *stat, const double *cnt,
                             int32_t per_element, double *par, double *mom, int32_t K,
                             const double *prior_r, const double *Nk, double *alpha_r,
                             double *elog_r, double mult, double scale, double *ws, double *bound);

/* Stochastic VI on the two diagonal-Gaussian-mixture blocks: the global half of a step in one launch
 * (details: bayespy_amd/csrc/vmp_dgmm_svi.hip, vmp_dgmm_svi_dev.h).  `nodes` is a bit set: 1 = mu,
 * 2 = tau, 4 = the mixing weights.  Tables in the layout of vmp_dgmm_update: priors, S1, S2 (D x K),
 * par and mom (D K, 2) with mu = ((m, lambda), (<mu>, <mu^2>)) and tau = ((a, b), (<tau>, <log tau>));
 * cnt = N_k (K, per_element 0) or the count of the element M (D x K, per_element 1, the block with
 * missing observations).  S1, S2 and cnt are given together or all null (phi* is the prior).
 * Element e = d K + k moves in the natural parameters, both nodes from the state at entry:
 *   mu:  lambda* = beta0 + mult <tau> cnt, (lambda m)* = beta0 m0 + mult <tau> S1
 *   tau: a* = a0 + mult cnt / 2, b* = b0 + mult (S2 - 2 <mu> S1 + <mu^2> cnt) / 2
 *   phi <- phi + scale (phi* - phi)
 * and the weights (K <= 64 contiguous columns: prior_r, Nk (null: the prior), alpha_r, elog_r) as in
 * vmp_mix_natural_step.  A thread owns element e of both tables and reads whatever it needs of both
 * before it stores; the weights row is one more workgroup.  What a node that is not named owns is not
 * written (its moments are read where the named node needs them: <tau> by mu, <mu> and <mu^2> by
 * tau), nor is its bound slot.
 *   scale == 1 does not read the old parameters (they may be NaN) and, with mult == 1, leaves par, mom
 *   and the bound term of vmp_dgmm_update (per_element 1: of vmp_dgmm_update_masked) bit for bit.
 *   bound[0] = <log p> - <log q> of mu, bound[1] of tau, bound[2] of the weights, each written only
 *   when its node is named.  No floating-point atomics: a thread leaves the terms of its element in ws
 *   (vmp_dgmm_natural_step_workspace doubles, host only; its last word is the ticket, cleared on the
 *   stream ahead of the launch) and the workgroup that finishes last adds them in the order of
 *   vmp_dgmm_update; the grid depends on (D, K, nodes) and the bits of every output on the inputs
 *   and the shape only.
 *   D or K < 1, nodes outside 1..7, per_element outside 0..1, mult <= 0, a NaN mult or scale, a null
 *   required pointer, statistics given in part: VMP_ERR_INVALID; D or K above vmp_dgmm_limits:
 *   VMP_ERR_UNSUPPORTED.  Nothing is launched or written after a refusal. */
int32_t vmp_dgmm_natural_step_workspace(int32_t D, int32_t K, int64_t *workspace_doubles);
int32_t vmp_dgmm_natural_step(vmp_ctx *ctx, int32_t D, int32_t K, int32_t nodes, const double *m0,
                              const double *beta0, const double *a0, const double *b0,
                              const double *S1, const double *S2, const double *cnt,
                              int32_t per_element, double *mu_par, double *mu_mom, double *tau_par,
                              double *tau_mom, const double *prior_r, const double *Nk,
                              double *alpha_r, double *elog_r, double mult, double scale, double *ws,
                              double *bound);

/* Measurement knob: overrides a launch parameter the library otherwise takes from its
 * environment variable / default ("xpass_nt", "xpass_wgs_per_cu", "xpass_occ",
 * "plate_stream", ...); process-wide, for A/B harnesses (tools/xpass_lab.hip). */
int32_t vmp_tune_set(const char *key, int32_t value);

/* Elapsed milliseconds of the most recent vmp_pca_xpass / vmp_pca_pass on this context,
 * measured with HIP events on the stream the pass kernel was launched on (blocks until done);
 * enabled by vmp_ctx_set_timing(ctx, 1). */
int32_t vmp_ctx_set_timing(vmp_ctx *ctx, int32_t enabled);
int32_t vmp_pca_last_pass_ms(vmp_ctx *ctx, double *ms_pass, double *ms_reduce);

/* Durations of the (up to 64, up to `cap`) most recent timed plate passes (PCA or GMM) in issue
 * order, then forget them: one HIP event triple per pass, so a measurement loop reads them
 * after its timed region instead of blocking inside every iteration. */
int32_t vmp_pass_times_ms(vmp_ctx *ctx, double *ms_pass, double *ms_reduce, int32_t cap,
                          int32_t *count);

#ifdef __cplusplus
}
#endif
#endif /* VMP_HIP_H */
