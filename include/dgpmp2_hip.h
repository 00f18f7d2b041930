/* dgpmp2_hip.h -- C-ABI of the MI355X-native inner Gauss-Newton solver for dGPMP2.
 *
 * The reference (mhmukadam/dgpmp2) has NO FFI: its boundary for this path is a Python API,
 *   PlanLayer.forward(thb,startb,goalb,imb,sdfb,qc_inv_trajb,obscov_inv_trajb,eps_trajb)
 *       -> (dthetab, err, err_ext)                         diff_gpmp2/gpmp2/plan_layer.py:87-99
 *   DiffGPMP2Planner.step(...) / .forward(...)              diff_gpmp2/gpmp2/diff_gpmp2_planner.py:176-211 / :92-174
 *   PlanLayer.error_batch / error_ext_batch / gp_error / obs_error / start_goal_error
 *                                                           plan_layer.py:273-345, :374-388
 * Each entry point below names the reference function it replaces.  The host-side mirror of the
 * Python classes (same names, arguments, return tuples) lives in dgpmp2_amd/gpmp2/ and calls these
 * through ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - every data pointer is a BORROWED DEVICE pointer (torch tensor.data_ptr()), contiguous row-major
 *    with exactly the torch shapes quoted; element type is the handle's io_dtype (all tensors alike).
 *  - all arithmetic inside the kernels is IEEE binary64 (the reference is fp64-only).
 *  - calls are asynchronous on the HIP stream passed as `stream` (a hipStream_t cast to void*;
 *    NULL = the null stream).  Nothing is allocated, freed or synchronised inside a call.
 *  - return value: DGP_OK or a negative DGP_E* code; never throws.  dgp_last_error() gives the text
 *    of the calling thread's last failure.
 *  - a handle is immutable after dgp_create() => the same handle may be used from several threads
 *    and streams concurrently (unlike the reference PlanLayer, which mutates factor state per call).
 */
#ifndef DGPMP2_HIP_H
#define DGPMP2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGP_ABI_VERSION 7

/* status codes */
#define DGP_OK              0
#define DGP_EINVAL         -1   /* bad argument (NULL pointer, size out of range, bad enum)            */
#define DGP_EUNSUPPORTED   -2   /* valid request outside what the kernels implement (e.g. nlinks != 1) */
#define DGP_EHIP           -3   /* HIP runtime error (launch failure, no device)                       */

/* io_dtype */
#define DGP_F32 0
#define DGP_F64 1
#define DGP_U8  2   /* images only: dgp_sdf_2d (input), dgp_obstacle_maps (output) */

/* flags */
#define DGP_FLAG_NONHOLONOMIC 1u   /* planner_params['non_holonomic'] (plan_layer.py:32), needs dof == 3 */
#define DGP_FLAG_VEL_LIMITS   2u   /* planner_params['use_vel_limits'] (plan_layer.py:34)                 */

/* GP covariance input modes (plan_layer.py:90-91; diff_gpmp2_planner.py:247-290) */
#define DGP_QC_STATIC   0   /* qc_inv == NULL: gp_params['Q_c_inv'] for every factor (diff_gpmp2_planner.py:41-46)  */
#define DGP_QC_PERSTATE 1   /* qc_inv (B, n-1, dof, dof): Q^-1 built as in gp_factor.py:65-73                       */
#define DGP_QC_QFULL    2   /* qc_inv (B, n-1, d, d) is Q^-1 itself ('q_full', plan_layer.py:90)                    */
#define DGP_QC_SCALAR   3   /* qc_inv (B, n-1): one scalar s_k per GP factor, Q_c^-1 = s_k * DgpConfig.Q_c_inv (diagonal) --      */
                            /* 'diag_identity' (diff_gpmp2_planner.py:255-258: q_k^2 I with Q_c_inv = I); dgp_gn_step[_errors] and their backward (g_qc_inv: the (B,n-1,dof,dof) gradient of the blocks s_k I), n <= 256 */

/* Constructor arguments of PlanLayer / DiffGPMP2Planner that the math depends on
 * (plan_layer.py:14-81).  All lengths in the reference's units. */
typedef struct DgpConfig {
  uint32_t struct_size;      /* = sizeof(DgpConfig), ABI guard                                           */
  int32_t  num_states;       /* n = planner_params['total_time_step'] + 1          (plan_layer.py:30);   */
                             /* 2 <= n <= 1024 (dof 2) / 640 (dof 3): up to 256 states the unrolled       */
                             /* kernels, beyond that the loop kernels of csrc/gn_long.h (LDS-bounded)     */
  int32_t  dof;              /* planner_params['dof']: 2 (point robot) or 3 (x,y,theta); d = 2*dof       */
  int32_t  nlinks;           /* robot_model.nlinks; only 1 is implemented                                */
  int32_t  io_dtype;         /* DGP_F32 or DGP_F64                                                       */
  uint32_t flags;            /* DGP_FLAG_*                                                               */
  double   total_time_sec;   /* planner_params['total_time_sec']; dt = total_time_sec/(n-1) (:31)        */
  double   x_lims[2];        /* env_params['x_lims']                                                     */
  double   y_lims[2];        /* env_params['y_lims']                                                     */
  double   K_s, K_g;         /* gp_params['K_s'], ['K_g']: prior sigma, weight 1/K^2 (:64-65)            */
  double   reg;              /* optim_params['reg']: delta added to the diagonal (:96,:219)              */
  double   sphere_radius;    /* robot_model.get_sphere_radii()  (obstacle_cost.py:30)                    */
  double   Q_c_inv[9];       /* gp_params['Q_c_inv'] (dof x dof, row-major): static GP weight and the    */
                             /* FIXED weight of err_ext (plan_layer.py:70-73,80)                         */
  double   cost_sigma;       /* obs_params['cost_sigma']: static / fixed obstacle weight 1/sigma^2 (:74) */
  double   epsilon_dist;     /* obs_params['epsilon_dist']: static epsilon                               */
  double   K_d;              /* gp_params['K_d'] (non-holonomic factor sigma)                            */
  double   K_v, v_x, v_y;    /* gp_params['K_v'], ['v_x'], ['v_y'] (velocity-limit factor)               */
} DgpConfig;

typedef struct DgpHandle DgpHandle;

/* Signed-distance field argument: sdfb (B,1,H',W') of PlanLayer.forward (only sdfb[:,0] is read,
 * obstacle_cost.py:35).  batch_stride is in ELEMENTS between consecutive samples' grids; 0 means one
 * grid shared by the whole batch (an expand()ed tensor). */
/* Memory layout of a grid (DgpSdf::layout).  ROWMAJOR is the reference's tensor.  TILED4: the same H' x W' values stored as 4 x 4 tiles,
 * element (y, x) at offset ((y / 4) * ceil(W' / 4) + x / 4) * 16 + (y % 4) * 4 + (x % 4) of a grid of ceil(H'/4) * ceil(W'/4) * 16 elements (cells past
 * the last row / column are padding, never read): the 2 x 2 footprint of a bilinear lookup then lies in ONE 64-byte (fp32) tile in 9 cases of 16 instead of
 * in two rows 4 W' bytes apart -- what dgp_sdf_2d(..., out_layout) writes directly for per-sample grids (DESIGN.md section 3 "SDF"). */
#define DGP_SDF_ROWMAJOR 0
#define DGP_SDF_TILED4   1

/* How the backward entry points deliver dL/d(sdf) (DgpSdf::grad_mode; the `g_sdf` argument is the destination):
 *   DGP_GSDF_DENSE     g_sdf = grid(s) of the handle's io_dtype in the layout given by g_sdf_batch_stride / g_sdf_copies, accumulated with atomics
 *                      (the caller zeroes them) -- the reference's dense sdf.grad;
 *   DGP_GSDF_DENSE_F64 the same with grids of DOUBLES whatever io_dtype: the partial copies of a shared grid, summed (and cast) by the caller -- the
 *                      accumulation over thousands of trajectories no longer depends on the order of fp32 atomics;
 *   DGP_GSDF_SPARSE    no grid at all: g_sdf = (passes, B, n, 4) tap VALUES (io_dtype) and grad_indices = the (4, passes*B*n*4) int64 COO indices
 *                      (b, 0, y, x) of a sparse tensor of sdfb's shape (torch.sparse_coo_tensor; explicit zeros and duplicates included).  A TILED grid
 *                      (layout DGP_SDF_TILED4, tensor (B,1,H'/4,W'/4,4,4)): SIX index rows (b, 0, y / 4, x / 4, y % 4, x % 4), a (6, nnz) array.  passes = 1 (dgp_gn_step_backward, dgp_eval_errors_backward), 2 (dgp_gn_step_errors_backward with an
 *                      unweighted-error cotangent: the taps at th + dtheta, then those at th) or max_iters (dgp_gn_solve_backward, whose caller
 *                      ZERO-FILLS both arrays: passes a trajectory did not run stay untouched).  No atomics, no O(B H' W') zero fill: the dense
 *                      gradient of B per-sample grids is 1 GiB of zeros at B = 4096, 256 x 256 around 4 MB of taps.  num_states <= 256.  */
#define DGP_GSDF_DENSE     0
#define DGP_GSDF_DENSE_F64 1
#define DGP_GSDF_SPARSE    2

typedef struct DgpSdf {
  const void* data;
  int32_t     rows;          /* H' */
  int32_t     cols;          /* W' >= 2; res = (x_lims[1]-x_lims[0])/W'  (obstacle_cost.py:34); a single-column grid
                                is rejected with DGP_EUNSUPPORTED: the taps are fetched as column pairs */
  int64_t     batch_stride;
  int32_t     layout;        /* DGP_SDF_*: layout of `data` (and of a dense g_sdf)                                                  */
  int32_t     grad_mode;     /* DGP_GSDF_*: backward entry points only                                                              */
  int64_t*    grad_indices;  /* DGP_GSDF_SPARSE: the (4, nnz) -- tiled grids: (6, nnz) -- int64 index array, else ignored              */
} DgpSdf;

/* Per-call covariance inputs = the three trailing arguments of PlanLayer.forward. */
typedef struct DgpCovs {
  int32_t     qc_mode;       /* DGP_QC_*                                                                 */
  const void* qc_inv;        /* see DGP_QC_*; NULL iff DGP_QC_STATIC                                     */
  const void* obs_w;         /* obscov_inv_trajb (B,n,1,1) or NULL = static 1/cost_sigma^2               */
  const void* eps;           /* eps_trajb (B,n,1,1) or NULL = static epsilon_dist                        */
} DgpCovs;

int         dgp_abi_version(void);
const char* dgp_last_error(void);

/* PlanLayer.__init__ (plan_layer.py:14-81).  Host-only; validates cfg, precomputes constants. */
int  dgp_create(const DgpConfig* cfg, DgpHandle** out);
void dgp_destroy(DgpHandle* h);

/* M of plan_layer.py:43-45 (rows of the dense system; the normaliser of err) for this handle. */
int  dgp_num_factor_rows(const DgpHandle* h);

/* Launch shape the library will use for a batch of `batch` trajectories: lanes per trajectory and consecutive states per
 * lane (reporting / tuning aid; the environment variable DGP_FORCE_SHAPE="LPT,C" read by dgp_create pins it).  num_states > 256:
 * (64, ceil(num_states / 64)) -- one trajectory per wavefront, the rows of a lane walked in a loop. */
int  dgp_launch_shape(const DgpHandle* h, int32_t batch, int32_t* lanes_per_trajectory, int32_t* states_per_lane);

/* Kernel variant dgp_gn_step / dgp_gn_solve launch for a batch of `batch` trajectories WITH STATIC covariances (covs == NULL):
 * 1 = block elimination with the constant GP blocks as scalar operands, 3 / 4 = interior rows eliminated through the Woodbury identity
 * on the constant GP block (Q_c_inv = c I, no velocity-limit factors, a launch shape with four states per lane; gn_woodbury.h --
 * 3 when num_states fills the shape exactly, 4 otherwise),
 * 0 = the general kernels (non-diagonal Q_c_inv).  Per-state covariance tensors select their own kernels per call.  Reporting
 * only (bench.py names the kernel whose instruction counts it quotes); DGP_NO_WOODBURY=1 at dgp_create keeps variant 1. */
int  dgp_step_kernel_variant(const DgpHandle* h, int32_t batch);

/* One batched Gauss-Newton step == PlanLayer.forward (plan_layer.py:87-99):
 * factor evaluation (gp_factor.py:100-110, prior_factor.py:15-18, obstacle_factor.py:35-40 ->
 * obstacle_cost.py:29-38 -> sdf_utils.py:38-107, custom_factors/), assembly of the block-tridiagonal
 * A^T K A + delta I and A^T K b (plan_layer.py:152-220) and the solve (plan_layer.py:226-228), plus
 * err (error_batch, :273-308) and err_ext (error_ext_batch, :310-345) at the INPUT trajectory.
 *   th (B,n,d)  start,goal (B,1,d)  ->  dtheta (B,n,d)  err (B,1,1)  err_ext (B,1,1)
 *   info (B) int32, optional: 0 ok, 1 = a non-positive pivot was met (system not SPD; the reference
 *   raises from torch.cholesky there).  err / err_ext may be NULL. */
int dgp_gn_step(const DgpHandle* h, int32_t batch,
                const void* th, const void* start, const void* goal,
                const DgpSdf* sdf, const DgpCovs* covs,
                void* dtheta, void* err, void* err_ext, int32_t* info, void* stream);

/* Fused Gauss-Newton loop == DiffGPMP2Planner.forward's inner `while True` (diff_gpmp2_planner.py:122-156)
 * for every trajectory of the batch at once, the trajectory staying in registers across iterations.
 * Per trajectory: repeat {dtheta,err,err_ext = step(th); th += dtheta; j++} until
 * ||dtheta||_F < tol_delta or j >= max_iters (utils/planner_utils.py:3-16; the last dtheta IS applied).
 *   th_out (B,n,d); iters (B) int32; err_hist, errext_hist (B,max_iters), entries at or past iters[b] untouched;
 *   err_final (B): error_batch at th_out (diff_gpmp2_planner.py:145,162).  Optional outputs may be NULL.
 *   info (B) int32, optional: the OR of dgp_gn_step's flag over the iterates trajectory b ITSELF stepped from, th_k for k < iters[b] (th_0 = th_init):
 *   1 = one of those systems was not SPD (the reference raises from torch.cholesky in that iteration).  The system at th_out is never part of it, and the
 *   flag of a trajectory does not depend on which trajectories share its batch or on how many iterations they run.  Once a trajectory is flagged its
 *   dtheta is not meaningful: it keeps iterating to max_iters (or until a step norm below tol_delta turns up) and its th_out is to be discarded. */
int dgp_gn_solve(const DgpHandle* h, int32_t batch,
                 const void* th_init, const void* start, const void* goal,
                 const DgpSdf* sdf, const DgpCovs* covs,
                 int32_t max_iters, double tol_delta,
                 void* th_out, int32_t* iters, void* err_hist, void* errext_hist, void* err_final,
                 int32_t* info, void* stream);

/* Factor evaluation only == PlanLayer.error_batch / error_ext_batch (plan_layer.py:273-345) and the
 * unweighted errors of DiffGPMP2Planner.unweighted_errors_batch (diff_gpmp2_planner.py:229-237 ->
 * plan_layer.py:374-388).  Any output may be NULL.  err, err_ext, unw_sg, unw_gp, unw_obs: (B).
 * `sdf` (or sdf->data) may be NULL when err, err_ext and unw_obs are all NULL: PlanLayer.gp_error(thb) and
 * start_goal_error(thb) (plan_layer.py:374-377, :384-388) take no grid, and then none is read. */
int dgp_eval_errors(const DgpHandle* h, int32_t batch,
                    const void* th, const void* start, const void* goal,
                    const DgpSdf* sdf, const DgpCovs* covs,
                    void* err, void* err_ext, void* unw_sg, void* unw_gp, void* unw_obs, void* stream);

/* Backward of dgp_gn_step (the reference gets it from torch autograd over plan_layer.py:152-234;
 * consumers: learning/train_planner.py:366-374, examples/diff_gpmp2_2d_example.py:77).
 * Given the forward inputs, the forward output dtheta (B,n,d), g_dtheta = dL/d(dtheta) (B,n,d) and
 * g_err_ext = dL/d(err_ext) (B) (either cotangent may be NULL = 0; dtheta may be NULL iff g_dtheta is),
 * re-assembles the system, solves the adjoint system Lambda lambda = g_dtheta and writes dL/d{th,start,goal}
 * (same shapes), dL/d(qc_inv) (shape of the qc_mode), dL/d(obs_w), dL/d(eps) (B,n), and ACCUMULATES dL/d(sdf)
 * into g_sdf with atomics (layout given by g_sdf_batch_stride; the caller zeroes it).  NULL outputs are skipped.
 * g_sdf_copies: 1, or (shared grid, g_sdf_batch_stride == 0, only) the number of PARTIAL grids laid out back to back
 * in g_sdf: a wavefront accumulates into copy (xcc_id % g_sdf_copies) and the caller sums the copies afterwards.  With
 * g_sdf_copies >= 8 (gfx950 has at most 8 XCDs, so no two XCDs share a copy) the accumulation uses XCD-local L2 atomics
 * instead of device-scope ones (the per-XCD L2s are not coherent with each other; every copy is then only ever touched
 * by ONE L2 during the kernel); with 2..7 copies the atomics stay device-scope and the copies only spread contention. */
int dgp_gn_step_backward(const DgpHandle* h, int32_t batch,
                         const void* th, const void* start, const void* goal,
                         const DgpSdf* sdf, const DgpCovs* covs,
                         const void* dtheta, const void* g_dtheta, const void* g_err_ext,
                         void* g_th, void* g_start, void* g_goal,
                         void* g_sdf, int64_t g_sdf_batch_stride, int32_t g_sdf_copies,
                         void* g_qc_inv, void* g_obs_w, void* g_eps, void* stream);

/* The partial copies of a shared grid's gradient (g_sdf_copies above) -> the gradient: out[e] = scale * sum_c partial[c * elems + e], e < elems = H' W',
 * one launch at memory speed; partial_dtype DGP_F32 / DGP_F64 (DGP_GSDF_DENSE_F64), out_dtype DGP_F32 / DGP_F64.  `scale`: 1, or 1 / B for a caller whose
 * autograd will sum B equal shares of an expand()ed grid.  (torch.sum over the copies costs 45 us for 16 x 256 x 256 doubles on MI355X; this 3.) */
int dgp_sum_partial_grids(const void* partial, int32_t partial_dtype, int32_t copies, int64_t elems, double scale,
                          void* out, int32_t out_dtype, void* stream);

/* Backward of dgp_eval_errors == torch autograd through PlanLayer.error_ext_batch (plan_layer.py:310-345) and the unweighted errors
 * gp_error / obs_error / start_goal_error (:374-388), which the reference's training loss differentiates
 * (learning/train_planner.py:327,342 -> one_step_loss :75-120 -> final_loss.backward() :366-374).
 * Cotangents g_err_ext, g_unw_sg, g_unw_gp, g_unw_obs: (B), any may be NULL (= 0).  Writes dL/d{th,start,goal} (same shapes as the
 * inputs), dL/d(eps) (B,n; only with covs->eps, the current epsilons of plan_layer.py:94,329) and ACCUMULATES dL/d(sdf) into g_sdf
 * (layout and partial copies exactly as in dgp_gn_step_backward; the caller zeroes it).  NULL outputs are skipped.  err (error_batch)
 * runs under no_grad in the reference (:275) and has no cotangent; none of these errors depends on qc_inv / obs_w (fixed or unit
 * weights), so covs->qc_inv and covs->obs_w are ignored.  `sdf` (or sdf->data) may be NULL when g_err_ext, g_unw_obs and g_sdf are. */
int dgp_eval_errors_backward(const DgpHandle* h, int32_t batch,
                             const void* th, const void* start, const void* goal,
                             const DgpSdf* sdf, const DgpCovs* covs,
                             const void* g_err_ext, const void* g_unw_sg, const void* g_unw_gp, const void* g_unw_obs,
                             void* g_th, void* g_start, void* g_goal,
                             void* g_sdf, int64_t g_sdf_batch_stride, int32_t g_sdf_copies,
                             void* g_eps, void* stream);

/* ---- round 4: what the reference's callers do around the step, as single calls ------------------------------------------------ */

/* dgp_gn_solve with the trajectory history the backward pass needs: th_hist (max_iters, B, n, d) in fp64 WHATEVER the handle's io_dtype
 * (dtheta_k = th_{k+1} - th_k is formed from it), row (k, b) = th_k of trajectory b for k < iters[b]; rows at or past iters[b] are not
 * written.  iters must be given with th_hist.  th_hist == NULL: exactly dgp_gn_solve.  num_states <= 256.
 * info (B): as dgp_gn_solve's -- the OR of the step's SPD flag over the rows (k, b), k < iters[b], of th_hist, i.e. over the iterates trajectory b itself
 * stepped from; th_out and the other trajectories of the batch have no part in it. */
int dgp_gn_solve_traced(const DgpHandle* h, int32_t batch,
                        const void* th_init, const void* start, const void* goal,
                        const DgpSdf* sdf, const DgpCovs* covs,
                        int32_t max_iters, double tol_delta,
                        void* th_out, int32_t* iters, void* err_hist, void* errext_hist, void* err_final,
                        int32_t* info, double* th_hist, void* stream);

/* Backward of the whole Gauss-Newton loop == torch autograd through DiffGPMP2Planner.forward, which keeps the graph across its
 * iterations (diff_gpmp2_planner.py:122-156; consumer examples/diff_gpmp2_2d_example.py:77): given dgp_gn_solve_traced's th_hist,
 * th_out, iters and the cotangent g_th_out (B,n,d) of the final trajectory, ONE launch walks th_{k+1} = th_k + dtheta(th_k) backwards
 * per trajectory (adjoint solve + per-factor chain rule per iteration, the running cotangent in registers) and writes dL/d th_init
 * (B,n,d), dL/d start, dL/d goal (B,1,d) and ACCUMULATES dL/d sdf (layout / partial copies as in dgp_gn_step_backward; the caller
 * zeroes it).  Static covariances (what forward() runs without learn modules; any Q_c_inv since round 6 -- a non-diagonal one runs the general chain kernels), num_states <= 256;
 * DGP_EUNSUPPORTED otherwise -- chain dgp_gn_step_backward then.  The per-iteration errors have no cotangent: forward() returns them
 * as python floats (:138-141). */
int dgp_gn_solve_backward(const DgpHandle* h, int32_t batch,
                          const void* start, const void* goal, const DgpSdf* sdf,
                          int32_t max_iters, const double* th_hist, const void* th_out, const int32_t* iters,
                          const void* g_th_out,
                          void* g_th_init, void* g_start, void* g_goal,
                          void* g_sdf, int64_t g_sdf_batch_stride, int32_t g_sdf_copies, void* stream);

/* One iteration of the reference's training loop (learning/train_planner.py:311-327): dgp_gn_step, then the unweighted errors of
 * DiffGPMP2Planner.unweighted_errors_batch at th + dtheta (the sum formed in io_dtype, as torch forms th_curr_b + dthetab), no th + dtheta
 * tensor in between.  unw_* (B), any may be NULL (all NULL: dgp_gn_step).  ONE launch (the step kernels with an errors epilogue) for row-major
 * grids and num_states <= 128 -- dof = 2: every covariance representation; dof = 3: everything but the general family (q_full tensors, a non-diagonal
 * Q_c_inv: measured slower in one launch than in two, profiles/r06_d6_general_twin.txt); otherwise two stream-ordered launches. */
int dgp_gn_step_errors(const DgpHandle* h, int32_t batch,
                       const void* th, const void* start, const void* goal,
                       const DgpSdf* sdf, const DgpCovs* covs,
                       void* dtheta, void* err, void* err_ext, int32_t* info,
                       void* unw_sg, void* unw_gp, void* unw_obs, void* stream);

/* Backward of dgp_gn_step_errors: cotangents of dtheta, err_ext and of the three unweighted errors at th + dtheta in, every gradient
 * of dgp_gn_step_backward out (same conventions; g_sdf accumulated).  dof = 2, num_states <= 256: ONE launch -- the errors' backward at th + dtheta
 * runs as a prologue of the step's backward kernel and hands dL/d(th + dtheta) over inside the launch (lane-private LDS), `workspace` may be NULL.
 * dof = 3 and longer trajectories: two stream-ordered launches, the first leaves dL/d(th + dtheta) in `workspace` ((B,n,d) elements of io_dtype,
 * caller-provided: nothing is allocated inside a call).  No unweighted-error cotangent: exactly dgp_gn_step_backward (workspace may be NULL). */
int dgp_gn_step_errors_backward(const DgpHandle* h, int32_t batch,
                                const void* th, const void* start, const void* goal,
                                const DgpSdf* sdf, const DgpCovs* covs,
                                const void* dtheta, const void* g_dtheta, const void* g_err_ext,
                                const void* g_unw_sg, const void* g_unw_gp, const void* g_unw_obs,
                                void* g_th, void* g_start, void* g_goal,
                                void* g_sdf, int64_t g_sdf_batch_stride, int32_t g_sdf_copies,
                                void* g_qc_inv, void* g_obs_w, void* g_eps, void* workspace, void* stream);

/* DiffGPMP2Planner.get_covariances for a single-link robot in the modes whose tensors are plain squares of the learn module's output (diff_gpmp2_planner.py:247-290,
 * 'diag_identity' and 'fix_dynamics', with or without learned epsilons) as ONE small launch each way -- the reference spends some twenty tiny torch kernels on the
 * slices, outer products, broadcasts and their backward, which cost as much as the solver once a training iteration is replayed from a HIP graph.
 * raw (B, width): the module's output vector out[:, 0, :], column blocks [0, n_gp) one scalar q_k per GP factor (n_gp = n - 1: 'diag_identity'; 0: 'fix_dynamics'),
 * [n_gp, n_gp + n) the raw obstacle weights o_i, [n_gp + n, n_gp + 2 n) the raw epsilons e_i (learn_eps != 0).  Outputs, every one optional, dense, io dtype of `dtype`:
 *   sq_scalars (B, n_gp) = q_k^2 (what DGP_QC_SCALAR takes), sq_qc_inv (B, n_gp, dof, dof) = q_k^2 I (the tensor the reference returns), sq_obs_w (B, n) = o_i^2,
 *   sq_eps (B, n) = e_i^2 -- the squares formed in the I/O type, as torch's v * v. */
int dgp_square_covariances(const void* raw, int32_t dtype, int32_t batch, int32_t width, int32_t n_gp, int32_t num_states, int32_t learn_eps, int32_t dof,
                           void* sq_scalars, void* sq_qc_inv, void* sq_obs_w, void* sq_eps, void* stream);
/* Its backward: g_raw (B, width) = 2 raw * [trace of g_qc_inv's dof x dof blocks (the gradient dgp_gn_step_backward writes under DGP_QC_SCALAR) | g_obs_w | g_eps],
 * zero in columns the mode does not consume; any gradient input may be NULL (= 0). */
int dgp_square_covariances_backward(const void* raw, int32_t dtype, int32_t batch, int32_t width, int32_t n_gp, int32_t num_states, int32_t learn_eps, int32_t dof,
                                    const void* g_qc_inv, const void* g_obs_w, const void* g_eps, void* g_raw, void* stream);

/* Signed distance fields of a batch of occupancy images on the GPU: utils/sdf_utils.py:6-21 (sdf_2d) for every image of the batch --
 *   im = image > 0.75 (free space), padded by `padlen` pixels of free space on every side (:13-15),
 *   sdf = (distance_transform_edt(im) - distance_transform_edt(1 - im)) * res (:16-20; scipy.ndimage underneath),
 * i.e. positive distances to the nearest obstacle pixel in free space, negative distances to the nearest free pixel inside obstacles.
 * image (batch, rows, cols) contiguous, image_dtype DGP_F32 / DGP_F64 / DGP_U8; sdf_out (batch, rows + 2 padlen, cols + 2 padlen),
 * out_dtype DGP_F32 / DGP_F64 (the reference returns float64); out_layout DGP_SDF_ROWMAJOR, or DGP_SDF_TILED4: batch grids of ceil(H'/4) * ceil(W'/4) * 16
 * elements in the tiled layout of DgpSdf::layout (what the GN kernels read with half the cache lines when every trajectory has its own grid; padding cells
 * of the last tile row / column are not written).  Bit-identical to scipy's result in float64 (squared distances are
 * integers), including its convention for an image with no pixel of the other kind (distances from the pixel at row -1, column 0).
 * workspace: device memory of at least dgp_sdf_2d_workspace_bytes(...) bytes, 4-byte aligned, owned by the call until the stream has
 * passed it.  Two stream-ordered launches (+ one memset of batch words); padded sides up to 8192, batch up to 65535. */
size_t dgp_sdf_2d_workspace_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t padlen);
int dgp_sdf_2d(const void* image, int32_t image_dtype, int32_t batch, int32_t rows, int32_t cols, int32_t padlen, double res,
               void* sdf_out, int32_t out_dtype, int32_t out_layout, void* workspace, size_t workspace_bytes, void* stream);

/* Validation metrics of a batch of planned trajectories in ONE launch: what the reference's validation loop computes per trajectory with some thirty small torch
 * kernels and a nonzero() (a device -> host synchronisation) -- learning/test_planner.py:299-334, datasets/test_dataset_sensitivity.py:175-206:
 *   smoothness_metrics / collision_metrics (utils/planner_utils.py:75-102), the raw GP and obstacle factor errors (gpfactor.get_error, gp_factor.py; obsfactor.get_error,
 *   obstacle_factor.py:35-40 -> obstacle_cost.py:29-38), the velocity-limit count (test_planner.py:310-322) and the MSELoss against the expert trajectory (:342-344).
 * th (B,n,d) and th_opt (B,n,d; optional) in the handle's io_dtype; sdf as for dgp_gn_step (row-major or DGP_SDF_TILED4, shared or per sample).
 * metric_eps: the epsilon of the METRICS obstacle factor, which the reference builds with eps = 0.0 and NOT with obs_params['epsilon_dist'] (test_planner.py:140,182-184):
 *   a state has a hinge error where dist <= metric_eps + sphere_radius, exactly where the step kernels give it one at that epsilon.  Negative values are allowed.
 * Outputs (either may be NULL, not both):
 *   metrics   (B, DGP_METRIC_COUNT) DOUBLES whatever io_dtype, columns DGP_METRIC_* below; needs num_states >= 3 (DGP_EINVAL otherwise: no interior state -- the reference
 *             raises on the max of an empty tensor there)
 *   obs_error (B, n) io_dtype: the raw hinge error of every state, obs_error[0][:, 0, 0] of the reference
 * The definitions are the reference's, quirks included (tests/golden/g9_metrics.npz pins them):
 *   AVG_VEL / AVG_ACC / AVG_JERK  means of the row 2-norms of traj[:, 2:], (traj[1:] - traj[:-1])[:, 2:] / total_time_step and the second differences [:, 2:] /
 *             total_time_step^2 over n, n - 1 and n - 2 rows: columns 2.. whatever dof (d = 6: theta, vx, vy, omega), divided by the STEP COUNT n - 1, not by dt
 *   GP_MSE    mean of e^2 over the (n - 1) d entries of e_i = x_{i+1} - Phi x_i  (torch.mean(torch.sum(gp_error ** 2, dim=-1)), gp_error (1, n-1, d, 1))
 *   IN_COLL, NUM_PENETRATING, AVG_PENETRATION, MAX_PENETRATION, COLL_INTENSITY  over the n - 2 INTERIOR states (the first and the last are dropped).  The reference
 *             calls collision_metrics with obs_error[0] of shape (n,1,1): nonzero() returns three columns and its `num_penetrating = numel / 2` is 1.5 x the number of
 *             penetrating states.  NUM_PENETRATING here is the plain count of interior states with a non-zero hinge error; COLL_INTENSITY = (1.5 count dt) / total_time_sec
 *             EQUALS the reference's value as called from test_planner.py:304 (the factor 1.5 included); IN_COLL = count > 0 as 0.0 / 1.0
 *   CONSTRAINT_VIOLATION  fraction of ALL n states with |th[2]| > v_x or |th[3]| > v_y (columns 2 and 3 whatever dof); 0 unless the handle has DGP_FLAG_VEL_LIMITS
 *   POS_MSE / VEL_MSE / TRAJ_MSE  MSELoss (mean) of th against th_opt over columns [0, dof), [dof, d) and all; 0 when th_opt is NULL
 * Arithmetic in fp64; the sums, maxima and counts of a trajectory are reduced inside its wavefront in a fixed order (no atomics): results are bit-identical from run to
 * run, for either grid layout and wherever the trajectory sits in the batch.  One launch, nothing allocated or synchronised: capturable in a HIP graph. */
#define DGP_METRIC_AVG_VEL               0
#define DGP_METRIC_AVG_ACC               1
#define DGP_METRIC_AVG_JERK              2
#define DGP_METRIC_GP_MSE                3
#define DGP_METRIC_IN_COLL               4
#define DGP_METRIC_NUM_PENETRATING       5
#define DGP_METRIC_AVG_PENETRATION       6
#define DGP_METRIC_MAX_PENETRATION       7
#define DGP_METRIC_COLL_INTENSITY        8
#define DGP_METRIC_CONSTRAINT_VIOLATION  9
#define DGP_METRIC_POS_MSE              10
#define DGP_METRIC_VEL_MSE              11
#define DGP_METRIC_TRAJ_MSE             12
#define DGP_METRIC_COUNT                13
int dgp_traj_metrics(const DgpHandle* h, int32_t batch, const void* th, const DgpSdf* sdf, double metric_eps, const void* th_opt,
                     double* metrics, void* obs_error, void* stream);

/* Planning problems sampled on the device, ONE launch: for every problem of the batch a feasible start / goal pair and the straight-line initial trajectory between
 * them -- what the reference's dataset generation does one point at a time in Python rejection loops:
 *   get_random_2d_confs / generate_start_goal (datasets/generate_optimal_paths_gpmp2.py:54-81, :120-162) over Env2D.is_feasible (env/env_2d.py:86-90), i.e.
 *   get_signed_obstacle_distance (:119-175) > eps, and straight_line_trajb (utils/planner_utils.py:47-56).
 * dof == 2 handles only (the reference samples for ndims == 2 only): DGP_EINVAL otherwise, as for a NULL params / sdf, max_draws < 1 or a margin that leaves no box.
 * sdf as for dgp_traj_metrics (row-major or DGP_SDF_TILED4, shared or one grid per sample).  env_index (B) int32 device array or NULL: the grid problem b is sampled
 * in (several problems per environment without copies of the grids; every entry must name an existing grid); NULL: grid b (per-sample grids) / the shared grid.
 * diagonal (B) int32 device array or NULL: 0..3 = the corner-to-corner problem of :134-145 (0: (x_min + inset, y_min + inset) -> (x_max - inset, y_max - inset), 1: the
 * reverse, 2: (x_max - inset, y_min + inset) -> (x_min + inset, y_max - inset), 3: its reverse), replaced by a random problem when either corner is infeasible
 * (:147-148; info bit 3); any other value (-1): a random problem.
 * Feasibility of a point: dist(x, y) > clearance, dist = Env2D.get_signed_obstacle_distance in fp64 in the reference's operation order -- pixel coordinates
 * orig + x / res, floor, the four indices clamped to the grid, the bilinear weights formed from the clamped indices as the reference forms them (on the last row /
 * column both taps coincide and the weights cancel), MAX_D = x_max - x_min for a point outside the (closed) limits: the lookup of the step and metrics kernels.
 * Randomness is counter-based -- Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (problem lo, problem hi, k, stream), problem = first_problem + b,
 * stream 0 for start and 1 for goal candidates, k the draw index; the four output words give candidate k:
 *   u0 = ((w0 * 2^32 | w1) >> 11) * 2^-53, u1 = ((w2 * 2^32 | w3) >> 11) * 2^-53, x = lbx + u0 (ubx - lbx), y = lby + u1 (uby - lby),
 *   (lbx, lby) = (x_min + margin, y_min + margin), (ubx, uby) = (x_max - margin, y_max - margin)                                                 (:58-61)
 * so a problem is a pure function of (seed, first_problem + b) and its grid: independent of batch size, position in the batch, launch shape and grid layout.
 * The accepted start is the lowest k whose candidate is feasible (:63-67); the accepted goal is the lowest k whose candidate is feasible and either at distance
 * sqrt(dx^2 + dy^2) >= min_dist_frac * ||(ubx, uby) - (lbx, lby)|| from the start or preceded by MORE than near_tries feasible-but-near goal candidates (:69-80: with
 * near_tries = 15 the 17th such candidate is accepted).  Both loops stop after max_draws candidates (the reference loops for ever): the outputs then hold the last
 * candidate drawn (k = max_draws - 1), the goal loop still runs after a capped start loop, and every output is written.
 * Outputs, io_dtype, computed in fp64 and rounded once on store: start, goal (B,1,4) = [x, y, 0, 0]; th_init (B,n,4), rows i = 0 .. N = n - 1:
 *   positions s*(N-i)*1.0/N*1.0 + g*i*1.0/N*1.0, velocities (g - s)/total_time_sec*1.0 (planner_utils.py:49-55, in that operation order).
 * draws (B,2) int32 or NULL: the draw indices of the accepted start and goal (-1, -1 for a diagonal problem).  info (B) int32 or NULL: bit 0 the start loop hit
 * max_draws, bit 1 the goal loop did, bit 2 the goal was accepted by the near-tries rule, bit 3 the diagonal was replaced by a random problem.
 * One launch, no atomics, nothing allocated or synchronised: capturable in a HIP graph. */
typedef struct DgpSampleParams {
  double   clearance;      /* a point is feasible where dist(x, y) > clearance; the reference passes sphere_radius + epsilon_dist + 0.1 (generate_optimal_paths_gpmp2.py:124) */
  double   margin;         /* sampling box = the handle's limits shrunk by margin on every side (0.5, :58-61) */
  double   min_dist_frac;  /* goal wanted at least this fraction of the box diagonal away (0.6, :77) */
  int32_t  near_tries;     /* a feasible but too-near goal is accepted once more than this many have been seen (15, :77-80) */
  int32_t  max_draws;      /* bound on the draws of the start loop and of the goal loop; the reference loops for ever */
  double   corner_inset;   /* 0.2, :134-145 */
} DgpSampleParams;
int dgp_sample_problems(const DgpHandle* h, int32_t batch, const DgpSdf* sdf, const int32_t* env_index,
                        const DgpSampleParams* p, uint64_t seed, uint64_t first_problem, const int32_t* diagonal,
                        void* start, void* goal, void* th_init, int32_t* draws, int32_t* info, void* stream);

/* Obstacle maps generated on the device, ONE launch: the occupancy images of a batch of environments -- what the reference makes with one Python rejection loop per
 * obstacle that copies and repaints the whole map for every candidate:
 *   generate_rect_obstacle_map / generate_wall_obstacle_map (datasets/obst_generator.py:179-221, :226-268) over random_rect / random_wall (:130-146), the checks
 *   _obstacle_collision_check (:45-50, :89-94) and _point_collision_check (:52-64, :96-108) and the slices of _add_to_map (:72-77, :115-126) and _add_point_to_map
 *   (:66-69), with the parameters of get_tarpit / get_forest / get_multi_obs / get_passage (datasets/generate_2d_dataset.py:29-75).
 * The rule is the reference's, quirks included (tests/golden/g11_obstacles.npz pins it).  Rows are axis 0 (y), columns axis 1 (x).  Obstacles are placed one after
 * another; candidate k of an obstacle is valid iff, after adding it to a copy of the map, no cell exceeds 1 -- in the obstacle check (a rectangle grown by pad_obs on
 * every side, a wall as it is) and, where keep-out points are given, for the obstacle without padding together with each point's patch.  A rectangle (w, h, cx, cy)
 * paints rows [cy - ceil(h/2), cy + ceil(h/2)) x columns [cx - ceil(w/2), cx + ceil(w/2)); a wall (w, gw, cx, gy) paints rows [0, gy - ceil(gw/2)) and
 * [gy + ceil(gw/2), rows) x columns [cx - ceil(w/2), cx + ceil(w/2)): two boxes; the patch of a point (x, y) is rows [ceil(y) - pad_pt, ceil(y) + pad_pt) x columns
 * [ceil(x) - pad_pt, ceil(x) + pad_pt).  Every range is a NumPy slice: a negative bound has the axis length added, both bounds are then clamped to [0, N], and the
 * slice is empty where start >= stop.  A padded box that sticks out over the low edge is therefore EMPTY and its check vacuous, as in the reference.  Once the map holds
 * a cell above 1 (two placed boxes overlap, or a placed box lies on a patch) no candidate is valid any more.
 * Randomness is counter-based -- Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (env lo, env hi, k, stream), env = first_env + b.  An inclusive
 * integer range [a, b] is drawn from a word w as a + ((uint64)w * (b - a + 1) >> 32).  Stream i holds the candidates of obstacle i, k the draw index:
 *   rectangle: w0 -> w in [w_min, w_max], w1 -> h in [h_min, h_max], w2 -> cx in [start_x + ceil(w/2), end_x - ceil(w/2)], w3 -> cy in [start_y + ceil(h/2),
 *              end_y - ceil(h/2)]                                                                                                    (random_rect, :130-139)
 *   wall:      w0 -> w in [w_min, w_max], w1 -> gw in [h_min, h_max], w2 -> cx in [start_x + ceil(w/2), cols - ceil(w/2)], w3 -> gy in [start_y + ceil(gw/2),
 *              rows - ceil(gw/2)]   (random_wall, :141-146, start_y its gap_y; the reference bounds both by the side of its square maps)
 * and the accepted candidate is the lowest valid k.  Stream 0xffffffff, k = 0: w0 gives the obstacle count n_lo + ((uint64)w0 * (n_hi - n_lo) >> 32) of the half-open
 * range [n_lo, n_hi) (np.random.randint(5, 8)), w1 the generator ((uint64)w1 * num_params >> 32) of the environment where several are passed (mixed_clutter).  An
 * environment is a pure function of (seed, first_env + b), the parameters and its keep-out points: independent of batch size, position in the batch and launch shape.
 * Each obstacle's loop stops after max_draws candidates (the reference loops for ever): the last candidate, k = max_draws - 1, is then placed.
 * params: num_params (1 .. DGP_OBST_MAX_GENERATORS) generators.  start_pts / goal_pts: (batch, num_pts, 2) float64 device arrays of pixel coordinates (x, y) as
 * generate_2d_dataset.py:186-192 forms them, or NULL; num_pts <= DGP_OBST_MAX_POINTS per list.
 * Outputs: image (batch, rows, cols) of image_dtype DGP_U8 / DGP_F32 / DGP_F64, the reference's 1 - count (floating types; below 0 where boxes overlap) or 1 where free
 *   and 0 otherwise (DGP_U8, what dgp_sdf_2d takes); boxes (batch, DGP_OBST_MAX_BOXES, 4) int32 [r0, r1, c0, c1], the slices as painted (clamped; empty where
 *   r0 >= r1 or c0 >= c1), zeros past num_boxes; num_boxes (batch) int32; draws (batch, DGP_OBST_MAX_BOXES) int32, the accepted k of every obstacle, -1 past the last;
 *   info (batch) int32: bit 0 an obstacle's loop hit max_draws, bit 1 a cell of the finished map is covered more than once (the reference's outer `while True`
 *   never returns then), bit 2 a negative slice bound was met by a keep-out patch or by the painted or padded box of an accepted candidate.  All but image may be NULL.
 * DGP_EINVAL, nothing launched: a NULL handle, image or params; batch < 1; num_params or num_pts out of range; an obstacle count range that is empty or allows more
 * than DGP_OBST_MAX_BOXES boxes (a wall is two); max_draws < 1; a size range that is empty, negative or leaves no centre for its largest obstacle (the reference's
 * randint raises there); NaN paddings; sides or coordinates beyond 2^20.
 * One launch, no atomics, nothing allocated or synchronised: capturable in a HIP graph. */
#define DGP_OBST_RECT            0
#define DGP_OBST_WALL            1
#define DGP_OBST_MAX_BOXES      64
#define DGP_OBST_MAX_POINTS     32
#define DGP_OBST_MAX_GENERATORS  4
typedef struct DgpObstacleParams {
  int32_t  kind;             /* DGP_OBST_RECT / DGP_OBST_WALL */
  int32_t  n_lo, n_hi;       /* obstacle count in [n_lo, n_hi) */
  int32_t  w_min, w_max;     /* widths (columns) */
  int32_t  h_min, h_max;     /* rectangle: heights (rows); wall: gap widths gw_min, gw_max */
  int32_t  start_x, start_y; /* lower ends of the centre ranges; wall: start_y is gap_y */
  int32_t  end_x, end_y;     /* rectangle: upper ends of the centre ranges; wall: not read (cols, rows) */
  int32_t  max_draws;        /* bound on the candidates of one obstacle; the reference loops for ever */
  double   patch_size_obs;   /* rectangle: pad_obs = ceil(patch_size_obs / 2) cells between obstacles (:75-76); wall: no padding (not a NaN all the same) */
  double   patch_size;       /* pad_pt = ceil(patch_size / 2): half side of a keep-out patch (:67-68) */
} DgpObstacleParams;
int dgp_obstacle_maps(const DgpHandle* h, int32_t batch, int32_t rows, int32_t cols, const DgpObstacleParams* params, int32_t num_params, uint64_t seed,
                      uint64_t first_env, const double* start_pts, const double* goal_pts, int32_t num_pts, void* image, int32_t image_dtype,
                      int32_t* boxes, int32_t* num_boxes, int32_t* draws, int32_t* info, void* stream);

/* Collision-free initial trajectories on the device, ONE launch: for every problem of the batch a trajectory of n states from the start to the goal that stays in
 * free space -- the role of the reference's --rrt_star_init (datasets/generate_optimal_paths_gpmp2.py:95-110, :156-159; generate_2d_dataset.py:225-226): an OMPL
 * RRT* run of 4 seconds per problem (init_planner.plan(start_conf, goal_conf, 4.0)), interpolate(num_states) and path_to_traj_avg_vel (utils/planner_utils.py:60-71).
 * RRT* is randomised and OMPL is not part of this build, so the PATH below has no counterpart in the reference and no fixture from it; what has one is the validity
 * rule -- RRTStar.isStateValid -> Env2D.is_feasible(state, sphere_radius + epsilon_dist) (diff_gpmp2/ompl_rrtstar.py:18, :48-50) -- and the velocities of
 * path_to_traj_avg_vel.  The rule stated here is exact: tests/paths_oracle.py restates it and the kernel is held against that bit for bit.  The path is a
 * grid path; dgp_shortcut_paths (below) turns it into a short any-angle polyline, the part of OMPL's simplifySolution that is built.  No smoothing.
 * dof == 2 handles only; x_lims, y_lims, n = num_states and total_time_sec come from the handle.  sdf: row-major grids of the handle's io_dtype, shared
 * (batch_stride 0) or one per sample, sides up to 2^12; DGP_SDF_TILED4 is refused with DGP_EINVAL (not implemented here: pass the row-major grid).  env_index as for
 * dgp_sample_problems.  With res = (x_max - x_min) / W, orig_x = 0 - x_min / res, orig_y = 0 - y_min / res and the pixel coordinates px = orig_x + x / res,
 * py = orig_y - y / res of the lookup:
 * Cells.  The point of cell (r, c) is the world point whose pixel coordinates are exactly (c, r): x = (c - orig_x) * res, y = (orig_y - r) * res; the bilinear lookup
 *   returns sdf[r][c] there.  The cell of a point: c = clamp(floor(px + 0.5), 0, W - 1), r = clamp(floor(py + 0.5), 0, H - 1).  A cell is free where its stored
 *   distance, converted to double, is > clearance.
 * Moves.  8 neighbours; an axis move costs 5, a diagonal move 7; a diagonal move is allowed only if both cells that share its corner are free (no corner cutting).
 *   uint32 arithmetic, INF = 0xffffffff, INF + cost = INF.
 * Distance field D (the goal's cost-to-go).  D = INF everywhere, D[goal cell] = 0 if that cell is free.  The CLOSURE of a row sets every free cell c to
 *   min_k (D[r][k] + 5 |c - k|) over the cells k of its maximal run of free cells.  A DOWN PASS visits r = 0 .. H-1 in order: for r >= 1 each free cell takes the
 *   minimum of itself and the allowed moves from row r-1 (final for this pass), then row r is closed (row 0 is only closed).  An UP PASS is the mirror image,
 *   r = H-1 .. 0 from row r+1.  A SWEEP is a down pass followed by an up pass; the loop ends after the first sweep that changed no cell, or after max_sweeps sweeps.
 *   A field that ended by the first condition is a fixed point of every edge relaxation: THE 5-7 shortest-path field, whatever order a kernel relaxes in.
 *   `field` (B,H,W) holds D at return, blocked cells INF.
 * Trace.  L cells are visited, starting at the start cell: while D[cur] > 0 (and fewer than H W cells were visited), step to the first neighbour, in the order
 *   (dr, dc) = (0,+1), (-1,0), (0,-1), (+1,0), (-1,+1), (-1,-1), (+1,-1), (+1,+1), that is inside the grid, free, allowed as a diagonal move and has
 *   D[nb] + cost == D[cur]; the trace ends where there is none.  path_cells (B, path_cap): r * W + c of the first path_cap cells, -1 behind them; num_cells (B): L.
 * Trajectory.  Vertices V_0 = the start point itself, V_1 .. V_L the points of the traced cells, V_{L+1} = the goal point itself.  fp64, FMA contraction off:
 *   l_j = sqrt(dx*dx + dy*dy) of segment j = V_j V_{j+1}, s_0 = 0, s_{j+1} = s_j + l_j summed serially, S = s_{L+1} -> length (B).  Row i (0 .. N = n - 1):
 *   t = S * i / N (the product first); j the lowest index with s_{j+1} >= t (the last segment if there is none); f = l_j > 0 ? (t - s_j) / l_j : 0; position
 *   V_j + f * (V_{j+1} - V_j).  Row N is the goal point itself, not interpolated; with S == 0 every row is the start point.  Velocities (goal - start) /
 *   total_time_sec on every row (path_to_traj_avg_vel).  th_init (B,n,4) io_dtype, every value rounded once on store.
 * info (B): bit 0 the start cell is not free; bit 1 the goal cell is not free; bit 2 D[start cell] = INF in a converged field (unreachable; set along with bit 0
 *   or 1 where the field of such a problem converged); bit 3 max_sweeps sweeps were run and the last still changed a cell; bit 4 L > path_cap.  With any of bits
 *   0-3 set th_init is the straight line of dgp_sample_problems (same formula and operation order), num_cells 0, path_cells all -1 and length the straight
 *   distance sqrt(dx*dx + dy*dy); bit 4 only truncates path_cells.  Every output is always written.  A problem is a pure function of its grid, start, goal and
 *   params: independent of batch size, position in the batch and launch shape.
 * `field` is workspace AND output and is required; path_cells, num_cells, length and info may each be NULL.
 * DGP_EINVAL, nothing launched: a NULL handle, params, sdf, start, goal, th_init or field; dof != 2; batch < 1; max_sweeps outside 1 .. 4096; path_cap < 0; a NaN
 * clearance; a tiled grid; H or W beyond 2^12.
 * One launch, no atomics, nothing allocated or synchronised: capturable in a HIP graph. */
typedef struct DgpPathParams {
  double  clearance;   /* a cell is free where its stored distance, converted to double, is > clearance; reference: sphere_radius + epsilon_dist (ompl_rrtstar.py:18) */
  int32_t max_sweeps;  /* bound on the sweeps of the distance field, 1 .. 4096 */
  int32_t path_cap;    /* second dimension of path_cells (>= 0) */
} DgpPathParams;
int dgp_init_paths(const DgpHandle* h, int32_t batch, const DgpSdf* sdf, const int32_t* env_index, const DgpPathParams* p,
                   const void* start, const void* goal,            /* (B,1,4) io_dtype */
                   void* th_init,                                  /* (B,n,4) io_dtype */
                   uint32_t* field,                                /* (B,H,W): workspace AND output, required */
                   int32_t* path_cells, int32_t* num_cells, double* length, int32_t* info,   /* each may be NULL */
                   void* stream);

/* Line-of-sight shortcutting of the grid paths of dgp_init_paths, ONE launch: the step RRTStar.plan makes between its tree path and interpolate(num_states),
 * self.ss.simplifySolution() (diff_gpmp2/ompl_rrtstar.py:36-41) -- the trajectory the reference's Gauss-Newton receives is a short any-angle polyline.  Here one
 * greedy pass of string pulling over the vertices of the traced path; a segment is usable where OMPL's discrete motion check finds every check point valid by
 * RRTStar.isStateValid -> Env2D.is_feasible.  The rule is exact: tests/shortcut_oracle.py restates it and the kernel is held against that bit for bit.  OMPL's
 * randomised shortcutting, smoothing and B-splines stay out.
 * dof == 2 handles only; grids, env_index, res, orig_x, orig_y as for dgp_init_paths.  Everything below is fp64 whatever io_dtype, FMA contraction off, operations
 * in the order written.
 * Vertices.  V_0 .. V_{L+1} are those of dgp_init_paths' "Trajectory" paragraph: V_0 the start point itself, V_1 .. V_L the points of the traced cells
 *   path_cells[b][0 .. L-1], L = num_cells[b], x = (c - orig_x) * res, y = (orig_y - r) * res with r = cell / W, c = cell % W, V_{L+1} the goal point itself.
 * Feasible point.  feasible(x, y) is Env2D.is_feasible(point, clearance) (env/env_2d.py:86-90, :119-175): the bilinear distance is > clearance.  The distance is
 *   that of dgp_sample_problems bit for bit (tests/problems_oracle.signed_distance): clamped taps, the weights from the clamped indices, MAX_D = x_max - x_min for a
 *   point outside the limits (closed on both sides), a NaN coordinate counting as outside.
 * Visible segment.  OMPL's discrete motion check in the max-norm (no square root decides anything discrete): dx = Qx - Px, dy = Qy - Py,
 *   m = fmax(fabs(dx), fabs(dy)) / check_step;  M = 1 if !(m > 1), else (int)ceil(m);  the check points are (Px + f * dx, Py + f * dy), f = (double)k / (double)M,
 *   k = 0 .. M.  visible(P, Q) holds iff all M + 1 check points are feasible.  A segment with m > 2^20 is not visible (the bound of every loop over check points;
 *   with check_step >= res / 16 and sides up to 2^12 no segment between points inside the limits comes near it).
 * Greedy string pulling, one pass.  a = 0, index 0 is kept.  While a < L + 1: hi = min(L + 1, a + lookahead); j* is the largest j in [a + 2, hi] with
 *   visible(V_a, V_j); if there is none, j* = a + 1, and that segment is kept whether or not it is visible -- if it is not, info bit 3 is set.  Keep j*, a = j*.
 *   The kept indices 0 = k_0 < ... < k_{m-1} = L + 1 are the result.  visible is a pure predicate and "the largest j" is well defined: the result does not depend
 *   on the order a kernel tests candidates or check points in.
 * Trajectory.  The kept vertices go through the resampling rule of dgp_init_paths word for word: l_j, the serial arc lengths s_j and S over the kept vertices;
 *   t = S * i / N, the lowest segment with s_{j+1} >= t, f = l_j > 0 ? (t - s_j) / l_j : 0; row N is the goal itself, S == 0 makes every row the start;
 *   velocities (goal - start) / total_time_sec on every row; every value rounded once to io_dtype.
 * Outputs.  th (B,n,4) io_dtype, in-out: the rows of a simplified problem are rewritten.  vertex_index (B, vertex_cap): the kept indices, -1 behind them.
 *   num_vertices (B): m.  length (B): the new S.  info (B): bit 0 no path to simplify (num_cells <= 0: dgp_init_paths fell back); bit 1 the input was truncated
 *   (num_cells > path_cap); bit 2 m > vertex_cap -- only vertex_index is truncated (so with vertex_cap == 0 it is set for every simplified problem, as bit 4 of
 *   dgp_init_paths is with path_cap == 0); bit 3 at least one kept segment is not visible.  With bit 0 or 1 set th[b] is left untouched, num_vertices is 0,
 *   vertex_index all -1 and length -1.0.  vertex_index, num_vertices, length and info may each be NULL.  A problem is a pure function of its grid, points, cells
 *   and params: independent of batch size and position in the batch.
 * What is guaranteed.  Every check point of a kept, visible segment is feasible.  The grid holds a distance transform, which changes by at most |dx| + |dy| between
 *   two points, and so does its bilinear interpolant (a convex combination of four such values, whose weights move the value by at most the tap differences).
 *   Consecutive check points are at most check_step apart in each coordinate, so any point of the segment lies within check_step / 2 of a check point in each
 *   coordinate: its distance is above clearance - (check_step / 2 + check_step / 2).  With info bit 3 clear the whole polyline therefore has distance
 *   > clearance - check_step.  The new length is <= the old one up to rounding: every kept segment replaces a run of the old polyline between the same two vertices
 *   (triangle inequality).
 * DGP_EINVAL, nothing launched: a NULL handle, params, sdf or grid, start, goal, path_cells, num_cells or th; dof != 2; batch < 1; a tiled or unknown layout, sides
 * outside 1 .. 2^12, a negative batch stride; a NaN clearance; a check_step that is not finite or is < res / 16; path_cap outside 1 .. 2^18; vertex_cap < 0;
 * lookahead < 1 (values above 2^30 count as 2^30); vertex_index non-NULL with vertex_cap == 0.
 * One launch, no atomics, nothing allocated or synchronised: capturable in a HIP graph. */
typedef struct DgpShortcutParams {
  double  clearance;   /* a point is feasible where its bilinear distance is > clearance; reference: sphere_radius + epsilon_dist (ompl_rrtstar.py:18) */
  double  check_step;  /* spacing of the check points of a segment in the max-norm, finite and >= res / 16 */
  int32_t path_cap;    /* second dimension of path_cells, 1 .. 2^18 */
  int32_t vertex_cap;  /* second dimension of vertex_index (>= 0) */
  int32_t lookahead;   /* the farthest vertex tried from vertex a is a + lookahead (>= 1) */
  int32_t reserved;    /* not read */
} DgpShortcutParams;   /* 32 bytes */
int dgp_shortcut_paths(const DgpHandle* h, int32_t batch, const DgpSdf* sdf, const int32_t* env_index, const DgpShortcutParams* p,
                       const void* start, const void* goal,                        /* (B,1,4) io_dtype */
                       const int32_t* path_cells, const int32_t* num_cells,        /* (B,path_cap), (B): what dgp_init_paths wrote */
                       void* th,                                                   /* (B,n,4) io_dtype, in-out */
                       int32_t* vertex_index, int32_t* num_vertices, double* length, int32_t* info,   /* each may be NULL */
                       void* stream);

/* GP-interpolated dense trajectories and the collision check BETWEEN support states, ONE launch.  The reference names the capability and never builds it:
 * gpmp2_planner.py:29-41 reads planner_params['total_check_step'] / ['use_gp_inter'], derives check_inter and sizes num_obs_factors for it, and no code interpolates.
 * The rule is GPMP2's GP interpolation: the posterior mean of the constant-velocity prior at time tau inside an interval, Lambda(tau) theta_i + Psi(tau) theta_{i+1},
 *   Psi = Q_tau Phi(Delta - tau)^T Q_Delta^-1,  Lambda = Phi(tau) - Psi Phi(Delta),  Phi, Q, Q^-1 those of gp/gp_factor.py:31-53.
 * Q_c cancels: the rule holds for every covariance mode, the learned ones included.  The heading column of the dof 3 robot is interpolated like any other column (the
 * reference's GP factor does no angle wrapping either).
 * Symbols.  Delta = total_time_sec / (n - 1) (the handle's dt); K = num_inter >= 0 interpolated states per interval; the dense trajectory has N_d = (n - 1)(K + 1) + 1
 *   states; dense index m belongs to interval i = m / (K + 1) at offset j = m % (K + 1), time i Delta + j Delta / (K + 1).
 * Copies.  j == 0 is a copy of support state i (the last dense state, i = n - 1, included): bit for bit, NaN and -0.0 included, no arithmetic touches it.
 * j >= 1.  fp64 whatever io_dtype, FMA contraction off, every operation in the order written, left to right inside a pair of parentheses:
 *   s  = (double)j / (double)(K + 1),  s2 = s * s,  s3 = s2 * s
 *   a0 = (1 - 3 s2) + 2 s3          a1 = Delta * ((s - 2 s2) + s3)      a2 = 3 s2 - 2 s3      a3 = Delta * (s3 - s2)
 *   b2 = (6 * (s - s2)) / Delta     b0 = -b2                            b1 = (1 - 4 s) + 3 s2  b3 = 3 s2 - 2 s
 *   and per dof component, x0, v0 columns c, dof + c of state i and x1, v1 those of state i + 1 (converted to double):
 *   pos = ((a0 x0 + a1 v0) + a2 x1) + a3 v1          vel = ((b0 x0 + b1 v0) + b2 x1) + b3 v1
 *   i.e. pos = (1 - 3s^2 + 2s^3) x0 + Delta (s - 2s^2 + s^3) v0 + (3s^2 - 2s^3) x1 + Delta (s^3 - s^2) v1,
 *        vel = -6 (s - s^2) / Delta x0 + (1 - 4s + 3s^2) v0 + 6 (s - s^2) / Delta x1 + (3s^2 - 2s) v1.
 *   Stored values are rounded once to io_dtype.
 * Obstacle lookup.  Every dense state is looked up at its first two columns by the function of the step and metrics kernels (obstacle_cost.py:29-38), with eps given per
 *   call: a hinge cost where dist <= eps + sphere_radius, exactly where a support state at that position has one.  For DGP_F32 the lookup takes the UNROUNDED fp64
 *   interpolated position (a copied state: its stored value).
 * th (B,n,d) io_dtype.  sdf as for dgp_traj_metrics (row-major or DGP_SDF_TILED4, shared or one grid per sample); may be NULL when dense_cost and summary are both NULL.
 * Outputs (each may be NULL, not all three):
 *   th_dense   (B, N_d, d) io_dtype
 *   dense_cost (B, N_d) io_dtype: the raw hinge cost of every dense state; at K = 0 it is obs_error of dgp_traj_metrics
 *   summary    (B, DGP_DENSE_COUNT) DOUBLES, over the dense states 1 .. N_d - 2 (collision_metrics' convention for support states: the first and the last are left
 *              out); needs N_d >= 3:
 *     IN_COLL 0 / 1;  NUM_COLLIDING count of cost != 0 (a NaN counts);  AVG_PENETRATION mean cost;  MAX_PENETRATION the largest cost, a NaN wins (torch.max);
 *     FIRST_COLLIDING smallest dense index with cost != 0, -1 if none;  WORST_INDEX dense index of the maximum, the smallest on ties (and of the first NaN if any).
 * DGP_EINVAL, nothing launched: a NULL handle or th; batch < 1; num_inter outside 0 .. 1023; all outputs NULL; dense_cost or summary without sdf; summary with N_d < 3.
 * Every num_states and dof a handle accepts is accepted.  The sums, maxima, counts and indices of a trajectory are reduced inside its wavefront in a fixed order (no
 * atomics): bit-identical from run to run, for either grid layout and wherever the trajectory sits in the batch.  One launch, nothing allocated or synchronised:
 * capturable in a HIP graph. */
#define DGP_DENSE_IN_COLL          0
#define DGP_DENSE_NUM_COLLIDING    1
#define DGP_DENSE_AVG_PENETRATION  2
#define DGP_DENSE_MAX_PENETRATION  3
#define DGP_DENSE_FIRST_COLLIDING  4
#define DGP_DENSE_WORST_INDEX      5
#define DGP_DENSE_COUNT            6
int dgp_gp_interpolate(const DgpHandle* h, int32_t batch, const void* th, int32_t num_inter, const DgpSdf* sdf, double eps,
                       void* th_dense, void* dense_cost, double* summary, void* stream);

/* The loss of one training iteration and its gradient on the device: the reference's one_step_loss (learning/train_planner.py:75-120, called at :328 as
 * one_step_loss(dthetab, th_opt_b - th_curr_b, ...)) -- eight index_select, four cat, two einsum, five mean and the scalar arithmetic around them, forward and
 * backward -- as two stream-ordered launches forward and one launch backward.  No handle: the loss needs only dtype (DGP_F32 / DGP_F64, the type of every `void*`
 * array below), B = batch, n = num_states and dof (2 or 3), d = 2 dof.
 * Columns.  Positions are columns [0, dof), velocities [dof, d).  For dof 2 these are exactly the reference's columns 0, 1 / 2, 3; the reference hard-codes those
 *   four columns whatever dof is (at dof 3 it would take theta and v_x as "velocity" and ignore v_y and omega; its training loop only ever runs dof 2).
 * Arithmetic.  fp64 whatever dtype, FMA contraction off, every operation in the order written, left to right inside a pair of parentheses.
 * Per-element miss.  m = (double)update - ((double)target - (double)target_sub); with target_sub == NULL, m = (double)update - (double)target.  The three-array
 *   form folds the reference's subtraction in: update = dtheta, target = th_opt, target_sub = th_curr.
 * Per trajectory b.  pos_b = sum_i sum_{c < dof} m^2,  vel_b = sum_i sum_{dof <= c < d} m^2;  gp_b, sg_b, obs_b = unw_gp[b], unw_sg[b], unw_obs[b] converted to
 *   double (0 for a NULL array).  per_traj row b holds (pos_b, vel_b, gp_b, sg_b, obs_b).  The two sums are formed inside the trajectory's wavefront in a fixed
 *   order that depends on n alone: a row has the same bits wherever the trajectory sits in the batch and whatever the batch size is.
 * Batch.  POS = (sum_b pos_b) / ((double)B * (double)n), VEL likewise;  GP = (sum_b gp_b) / (double)B, SG and OBS likewise (fixed-order sums of per_traj, one workgroup);
 *   EXT = (GP + SG) + ext_obs_lambda * OBS;  TOTAL = (POS + vel_loss_lambda * VEL) + ext_loss_weight * EXT;  COV = 0.
 * terms holds them at DGP_LOSS_*: one_step_loss's return order (:120).
 * Backward, g = *g_total (1.0 for NULL):
 *   c_ext = ext_loss_weight * g;  k_pos = (2.0 * g) / ((double)B * (double)n);  k_vel = (2.0 * (vel_loss_lambda * g)) / ((double)B * (double)n);
 *   g_update = m * k (k = k_pos for a position column, k_vel for a velocity column);  g_target = -(m * k);  g_target_sub = m * k;
 *   g_unw_gp = g_unw_sg = c_ext / (double)B;  g_unw_obs = (ext_obs_lambda * c_ext) / (double)B.
 *   Every stored value is rounded once to dtype; NULL outputs are skipped (g_target_sub may be asked for without target_sub: m is then update - target).
 * Pointers need only be aligned to their element type: 16-byte vector accesses where every (B,n,d) pointer of the call allows them, element accesses otherwise,
 * the same bits either way.
 * DGP_EINVAL, nothing launched: dtype not DGP_F32 / DGP_F64; batch < 1; num_states < 1; dof not 2 or 3; a NULL update, target, w, terms or per_traj; a NaN weight;
 * backward with every output NULL.  No atomics: bit-identical from run to run.  Nothing allocated or synchronised: capturable in a HIP graph.
 * dgp_time_next_launch times the first of the two forward launches. */
#define DGP_LOSS_TOTAL 0   /* one_step_loss's return order, train_planner.py:120 */
#define DGP_LOSS_POS   1
#define DGP_LOSS_VEL   2
#define DGP_LOSS_COV   3   /* always 0: the reference's covariance regulariser is commented out (:113-116) */
#define DGP_LOSS_GP    4
#define DGP_LOSS_SG    5
#define DGP_LOSS_OBS   6
#define DGP_LOSS_EXT   7
#define DGP_LOSS_COUNT 8
#define DGP_LOSS_PER_TRAJ 5   /* per_traj columns: pos, vel, gp, sg, obs */
typedef struct DgpLossWeights { double vel_loss_lambda, ext_obs_lambda, ext_loss_weight; } DgpLossWeights;

int dgp_step_loss(int32_t dtype, int32_t batch, int32_t num_states, int32_t dof,
                  const void* update, const void* target, const void* target_sub,       /* (B,n,d) io dtype; target_sub may be NULL */
                  const void* unw_sg, const void* unw_gp, const void* unw_obs,         /* (B) io dtype; each may be NULL (= 0) */
                  const DgpLossWeights* w,
                  double* terms,        /* (DGP_LOSS_COUNT) doubles */
                  double* per_traj,     /* (B, DGP_LOSS_PER_TRAJ) doubles: output AND workspace, required */
                  void* stream);
int dgp_step_loss_backward(int32_t dtype, int32_t batch, int32_t num_states, int32_t dof,
                  const void* update, const void* target, const void* target_sub,
                  const DgpLossWeights* w, const double* g_total,                      /* device scalar; NULL = 1.0 */
                  void* g_update, void* g_target, void* g_target_sub,                  /* (B,n,d) io dtype; each may be NULL */
                  void* g_unw_sg, void* g_unw_gp, void* g_unw_obs,                     /* (B) io dtype; each may be NULL */
                  void* stream);

/* The reference's bilinear_interpolate (utils/sdf_utils.py:38-107) at arbitrary points of a batch, its gradient, and the per-row collision summary behind
 * check_solved (learning/train_initializer.py:81-88).  No handle: the reference function takes res, x_lims and y_lims explicitly (check_solved passes a cell size
 * taken from im_size, not from the padded width).  dtype (DGP_F32 / DGP_F64) is the type of every `void*` array below; B = batch, S = num_points.
 * points  (B,S,>=2): x, y are the first two elements of a row; point_stride is the row pitch in elements (>= 2), the batch pitch is S * point_stride: a (B,n,d)
 *   trajectory tensor is looked up at its positions with point_stride = d, without a copy.
 * sdf     rows >= 1, cols >= 2 (a single column: DGP_EUNSUPPORTED), batch_stride (0 = one grid for every row), layout ROWMAJOR / TILED4.
 * Arithmetic.  fp64 whatever dtype, FMA contraction off, every operation in the order written, left to right inside a pair of parentheses; `u / res` is the IEEE
 *   quotient for finite u, the sign of a zero kept (a non-finite u gives NaN).  Every stored value is rounded once to dtype.
 * Forward (sdf_utils.py:57-94; the in-limits rule of :96-106 is a no-op on torch >= 1.2 and MAX_D is never produced):
 *   ox = 0 - x_lims[0] / res,  oy = 0 - y_lims[0] / res;   px = ox + x / res,  py = oy - y / res
 *   x1 = floor(px), x2 = x1 + 1, y1 = floor(py), y2 = y1 + 1 as integers, THEN each clamped to [0, cols - 1] / [0, rows - 1].  floor(px) is saturated to +-1e9 before
 *   the conversion and a NaN lands on an in-range index (the step kernels' index computation): for |px| >= 1e9 the index saturates -- after the clamp the same taps
 *   as the exact integer would give, while the reference's own int64 cast is undefined there.
 *   a, b, c, e = grid[y1][x1], grid[y1][x2], grid[y2][x1], grid[y2][x2]  (the reference's dx1y1, dx2y1, dx1y2, dx2y2), converted to double
 *   wja = (double)y2 - py,  wjb = py - (double)y1,  wjc = (double)x2 - px,  wjd = px - (double)x1      (clamped integers against unclamped px, py)
 *   wa = wjc * wja,  wb = wjd * wja,  wc = wjc * wjb,  wd = wjd * wjb
 *   d  = ((wa * a + wb * b) + wc * c) + wd * e
 *   J0 = (-1.0 * (wja * (b - a) + wjb * (e - c))) / res        J1 = (wjc * (c - a) + wjd * (e - b)) / res
 * Outputs (each may be NULL, not all three): d_obs (B,S) and J (B,S,2) of dtype; summary (B, DGP_LOOKUP_COUNT) DOUBLES over the S points of a row, from the fp64 d
 *   before rounding:  SOLVED 1.0 iff no point has d <= clearance (check_solved's test: a NaN does not block);  NUM_BLOCKED the count of d <= clearance;
 *   FIRST_BLOCKED the smallest such index, -1.0 if none;  MIN_DIST the smallest d, a NaN wins (torch.min);  MIN_INDEX its index, the smallest among equals (of the
 *   first NaN if any).  clearance is read by the summary only and must be finite when summary is given.
 * Backward, cotangents g_d (B,S) and g_J (B,S,2) of dtype, either may be NULL (= 0), gd = g_d, g0 = g_J[0], g1 = g_J[1] converted to double:
 *   cr   = (((e - c) - b) + a) / res
 *   g_px = gd * (wja * (b - a) + wjb * (e - c)) + g1 * cr          g_points[0] =   g_px / res
 *   g_py = gd * (wjc * (c - a) + wjd * (e - b)) - g0 * cr          g_points[1] = -(g_py / res)
 *   t_a  = gd * (wjc * wja) + (g0 * wja - g1 * wjc) / res          t_b = gd * (wjd * wja) - (g0 * wja + g1 * wjd) / res
 *   t_c  = gd * (wjc * wjb) + (g0 * wjb + g1 * wjc) / res          t_e = gd * (wjd * wjb) + (g1 * wjd - g0 * wjb) / res
 *   g_points (B,S,2) dense, of dtype, WRITTEN.  g_sdf: t_a, t_b, t_c, t_e are ADDED to the cells of a, b, c, e with device-scope atomics (the caller zeroes it):
 *   grids in sdf->layout, g_sdf_batch_stride elements apart (0 = one grid).  sdf->grad_mode DGP_GSDF_DENSE: cells of dtype, every contribution rounded once to dtype,
 *   then added; DGP_GSDF_DENSE_F64: cells are doubles whatever dtype, contributions unrounded.  Clamped cells need no special case: coinciding taps receive both
 *   contributions.  Floor and clamp are piecewise constant: no gradient passes through them, as in the reference's autograd.  Either output may be NULL, not both.
 * Pointers need only be aligned to their element type: a point / J / g_points row moves as one 8-byte (fp32) or 16-byte (fp64) vector where point_stride == 2 and
 * the pointers of the call allow it, element by element otherwise, the same bits either way.
 * DGP_EINVAL, nothing launched: a bad dtype; batch or num_points < 1; NULL points, sdf, x_lims or y_lims; point_stride < 2; res not positive and finite; limits
 * with hi <= lo; all outputs NULL; a summary without a finite clearance; backward without a cotangent; g_sdf_copies < 1.  DGP_EUNSUPPORTED: cols < 2;
 * DGP_GSDF_SPARSE; g_sdf_copies > 1.  The forward uses no atomics: bit-identical from run to run.  Nothing allocated or synchronised: capturable in a HIP graph. */
#define DGP_LOOKUP_SOLVED        0
#define DGP_LOOKUP_NUM_BLOCKED   1
#define DGP_LOOKUP_FIRST_BLOCKED 2
#define DGP_LOOKUP_MIN_DIST      3
#define DGP_LOOKUP_MIN_INDEX     4
#define DGP_LOOKUP_COUNT         5
int dgp_sdf_lookup(int32_t dtype, int32_t batch, int32_t num_points,
                   const void* points, int64_t point_stride,
                   const DgpSdf* sdf, double res, const double x_lims[2], const double y_lims[2],
                   double clearance,                                                  /* summary only */
                   void* d_obs, void* J, double* summary, void* stream);
int dgp_sdf_lookup_backward(int32_t dtype, int32_t batch, int32_t num_points,
                   const void* points, int64_t point_stride,
                   const DgpSdf* sdf, double res, const double x_lims[2], const double y_lims[2],
                   const void* g_d, const void* g_J,                                  /* either may be NULL (= 0) */
                   void* g_points, void* g_sdf, int64_t g_sdf_batch_stride, int32_t g_sdf_copies,
                   void* stream);

/* Trajectory samples from the GP prior, ONE launch: num_samples trajectories per problem drawn from N(mu, Sigma), the initial trajectories of a multi-start.  No
 * counterpart in the reference, which gives Gauss-Newton one initial trajectory per problem.  Sigma^-1 = A^T K^-1 A is the matrix dgp_gn_step assembles from the start
 * prior, the n - 1 GP factors and the goal prior alone (obstacle, non-holonomic and velocity-limit rows left out, no reg), mu that system's solution; only the static
 * covariances of the handle enter (Q_c_inv, K_s, K_g -- no DgpCovs).  Every handle is accepted (every num_states, dof 2 and 3, both flags); the heading column of the
 * dof 3 robot is a column like any other (as for dgp_gp_interpolate).
 * Symbols.  d = 2 dof, n = num_states, dt the handle's (total_time_sec * 1.0 / (n - 1) * 1.0), t_k = (double)k * dt, t_end = t_(n-1); Phi(t) = [[I, t I], [0, I]];
 *   Q_c = (Q_c_inv)^-1, L_c its lower Cholesky factor; Q(t) = [[t^3/3 Q_c, t^2/2 Q_c], [t^2/2 Q_c, t Q_c]];
 *   P(t) = K_s^2 Phi(t) Phi(t)^T + Q(t): the covariance of the unconditioned chain at time t;  S = P(t_end) + K_g^2 I;  W(t) = P(t) Phi(t_end - t)^T S^-1.
 * Construction, per problem b and sample s, from standard normals z laid out (n + 1, d): row 0 is z_0, row k + 1 = [u_k | u'_k] (dof entries each, k = 0 .. n - 2),
 *   row n is z_g.
 *   1. chain:  x_0 = K_s z_0;  x_(k+1) = Phi(dt) x_k + w_k,  w_k = [cp L_c u_k | cv1 L_c u_k + cv2 L_c u'_k],  cp = dt^(3/2) / sqrt 3, cv1 = (sqrt 3 / 2) sqrt dt,
 *      cv2 = sqrt dt / 2  (Cov w_k = Q(dt));
 *   2. noisy goal observation:  y = x_(n-1) + K_g z_g;
 *   3. Matheron's rule:  xi_k = x_k - W(t_k) y  -- the chain conditioned on observing 0 at the goal: xi ~ N(0, Sigma) exactly;
 *   4. th[b, s, k] = m_k + scale * xi_k,  m = mean[b] (n, d) where given, else m_k = mu_k = Phi(t_k) start + W(t_k) (goal - Phi(t_end) start).
 *   mean may be any trajectory (the th_init of dgp_init_paths / dgp_shortcut_paths: samples around the grid path); scale >= 0 scales the spread, 0 returns m.
 * Arithmetic.  fp64 whatever io_dtype, FMA contraction off, every operation in the order written, left to right inside a pair of parentheses; a product of a matrix
 *   and a vector sums each row left to right, (M x)_i = (..(M_i0 x_0 + M_i1 x_1) + ..), a triangular one over its non-zero entries.  Stored values are rounded once.
 *   Host constants (double, passed by value):
 *     Cholesky of an N x N matrix A (lower triangle read), j = 0 .. N - 1:  s = A_jj, then s = s - G_jk G_jk for k = 0 .. j - 1;  G_jj = sqrt s  (s must be positive and
 *       finite);  for i > j:  r = A_ij, then r = r - G_ik G_jk for k < j;  G_ij = r / G_jj.
 *     Inverse of SPD A:  G as above;  V = G^-1:  V_jj = 1 / G_jj,  for i > j:  s = G_ij V_jj, then s = s + G_ik V_kj for k = j + 1 .. i - 1;  V_ij = (-s) / G_ii;
 *       (A^-1)_ij for j <= i:  s = V_ii V_ij, then s = s + V_ki V_kj for k = i + 1 .. N - 1;  mirrored.
 *     Q_c = inverse of Q_c_inv (which must be exactly symmetric), L_c = Cholesky of Q_c;  ks2 = K_s * K_s, kg2 = K_g * K_g;  sdt = sqrt dt, s3 = sqrt 3.0:
 *       cp = (dt * sdt) / s3,  cv1 = (s3 / 2) * sdt,  cv2 = sdt / 2;  t_end = (double)(n - 1) * dt.
 *     coefficients of P(t):  t2 = t * t, t3 = t2 * t;  i_pp = ks2 * (1 + t2), i_pv = ks2 * t, q_pp = t3 / 3, q_pv = t2 / 2, q_vv = t.
 *     S at t = t_end, e = 1 on the diagonal of a dof x dof block and 0 off it, q = Q_c[i][j]:  S_pp = (i_pp + kg2) * e + q_pp * q,  S_pv = S_vp^T = i_pv * e + q_pv * q,
 *       S_vv = (ks2 + kg2) * e + q_vv * q;  S^-1 by the inverse above (N = d).
 *   Per trajectory, c a dof component, z_k row k of the normals, lu_k = L_c z_k[0 : dof], lw_k = L_c z_k[dof : d]:
 *     velocity elements  ev_0 = K_s * z_0[dof + c],  ev_k = cv1 * lu_k[c] + cv2 * lw_k[c]  (k >= 1);        v = SCAN(ev)
 *     position elements  ep_0 = K_s * z_0[c],        ep_k = cp * lu_k[c] + dt * v_(k-1)[c]  (k >= 1);        p = SCAN(ep);      x_k = [p_k | v_k]
 *     SCAN, the inclusive prefix sum in this association order, a function of the index alone: inside each block of 64 consecutive indices starting at a multiple of
 *       64, for off = 1, 2, 4, 8, 16, 32 in turn and for all i of the block with i % 64 >= off at once, e_i <- e_(i - off) + e_i; then, block after block from the
 *       second on, e_i <- c + e_i for every i of the block, c the finished value of the last index of the block before.
 *     y[c] = p_(n-1)[c] + K_g * z_g[c],  y[dof + c] = v_(n-1)[c] + K_g * z_g[dof + c];  g = S^-1 y.
 *     W(t) g for a vector g, tau = t_end - t, the coefficients of P(t) as above:  hp = g[0 : dof],  hv[c] = tau * g[c] + g[dof + c];
 *       ap[c] = q_pp * hp[c] + q_pv * hv[c],  av[c] = q_pv * hp[c] + q_vv * hv[c];
 *       (W g)[c] = (i_pp * hp[c] + i_pv * hv[c]) + (Q_c ap)[c],   (W g)[dof + c] = (i_pv * hp[c] + ks2 * hv[c]) + (Q_c av)[c].
 *     mu_k (mean == NULL), sp / sv the position / velocity part of start:  r0[c] = goal[c] - (sp[c] + t_end * sv[c]),  r0[dof + c] = goal[dof + c] - sv[c];  gr = S^-1 r0;
 *       mu_k[c] = (sp[c] + t_k * sv[c]) + (W(t_k) gr)[c],   mu_k[dof + c] = sv[c] + (W(t_k) gr)[dof + c].
 *     th[b, s, k][j] = m_k[j] + scale * (x_k[j] - (W(t_k) g)[j]).
 *   Nothing here depends on the lanes per trajectory, the batch size or the position in the batch: th[b, s] is a pure function of (seed, first_problem + b, s), the
 *   handle and start / goal / mean[b] -- or of noise[b, s] in their place.
 * Noise.  noise (B, S, n + 1, d) DOUBLES, or NULL: generated -- Philox4x32-10 with the key of dgp_sample_problems (seed & 0xffffffff, seed >> 32) and counter
 *   (problem lo, problem hi, j, (0x50 << 24) | s), problem = first_problem + b; num_samples <= 2^24, and 0x50 in the top byte of the last counter word is a stream no
 *   other entry point uses.  Block j yields entries 2 j and 2 j + 1 of the trajectory's row-major (n + 1, d) array: u0, u1 from the four words as for
 *   dgp_sample_problems (53 bits, [0, 1)),  r = sqrt(-2.0 * log(1.0 - u0)),  a = 6.283185307179586 * u1,  entries r * cos(a) and r * sin(a), the fp64 library functions
 *   (a few ulp from the correctly rounded values: the generated normals are reproducible to 1e-13, not bit for bit, against another library; th from SUPPLIED noise is).
 *   noise_out (B, S, n + 1, d) doubles or NULL: the normals used (a copy of noise where that is given): feeding it back as noise reproduces th bit for bit.
 * info (B, S) int32 or NULL: bit 0 a stored position (the first two columns of a state) lies outside the handle's closed limits [x_min, x_max] x [y_min, y_max] (a NaN
 *   is outside) -- samples are neither clamped nor rejected; bit 1 a stored value is not finite.
 * start, goal (B,1,d) and mean (B,n,d) of io_dtype; th (B,S,n,d) io_dtype.  Pointers need only be aligned to their element type (th moves as 8- / 16-byte vectors where
 * its address allows, the same bits either way).
 * DGP_EINVAL, nothing launched: a NULL handle, start, goal or th; batch < 1; num_samples outside 1 .. 2^24, or batch * num_samples >= 2^31; scale negative or not
 * finite; Q_c_inv not symmetric positive definite.  One launch, no atomics, nothing allocated, copied or synchronised: capturable in a HIP graph. */
int dgp_prior_samples(const DgpHandle* h, int32_t batch, int32_t num_samples,
                      const void* start, const void* goal,      /* (B,1,d) io_dtype */
                      const void* mean,                         /* (B,n,d) io_dtype or NULL = mu */
                      double scale, uint64_t seed, uint64_t first_problem,
                      const double* noise,                      /* (B,S,n+1,d) doubles or NULL = generate */
                      void* th,                                 /* (B,S,n,d) io_dtype */
                      double* noise_out,                        /* (B,S,n+1,d) doubles or NULL */
                      int32_t* info,                            /* (B,S) or NULL */
                      void* stream);
/* What dgp_prior_samples launches for this handle (the function its dispatch itself reads): lanes per trajectory (16 / 32 / 64, from num_states) and the number of
 * 64-state blocks a wavefront walks (1: one pass; more: the block loop, two passes).  Either pointer may be NULL.  No effect on any result. */
int dgp_prior_launch_shape(const DgpHandle* h, int32_t* lanes_per_traj, int32_t* blocks);

/* Planar trajectories lifted to problems of the non-holonomic x-y-heading robot (PointRobotXYH, dof 3), ONE launch: th2 (B,n,4) -- a straight line of
 * dgp_sample_problems, a grid path of dgp_init_paths, its shortcut -- becomes start, goal (B,1,6) and th (B,n,6).  The reference can only build straight_line_trajb
 * with dof = 3 (utils/planner_utils.py:47-56): a heading linear in time and one constant velocity, which violates the non-holonomic factor
 * (custom_factors/nonholonomic_factor.py:20, vy cos(theta) - vx sin(theta)) at every state of any path that is not a straight line along both end headings.  Here the
 * heading follows the path's tangent, continuously (the running sum of the signed turns between consecutive tangents: never wrapped), blended into the end headings,
 * and the velocities are the path's own central differences; the reference's rule is DGP_HEADING_LINEAR with DGP_VEL_KEEP.
 * dof == 3 handles only.  Everything below is fp64 whatever io_dtype, FMA contraction off, every operation in the order written, left to right inside a pair of
 * parentheses; stored values are rounded once.  N = n - 1, Delta = total_time_sec / (double)N, PI = 3.141592653589793, TWO_PI = 6.283185307179586 (doubles),
 * wrap(a) = a - TWO_PI * rint(a / TWO_PI) (ties to even); (x_i, y_i) columns 0, 1 of row i of th2 converted to double.
 * Positions.  Columns 0, 1 of th are columns 0, 1 of th2 copied bit for bit (NaN and -0.0 included).
 * Tangents.  lo = max(i - 1, 0), hi = min(i + 1, N), t_i = (x_hi - x_lo, y_hi - y_lo).  Row i is degenerate where both components are zero or either is not finite.
 *   u_i is t_i after forward fill: a degenerate row takes the tangent of the nearest earlier non-degenerate row, leading degenerate rows that of the first
 *   non-degenerate row; with every row degenerate u_i = (1, 0).
 * Turns (DGP_HEADING_TANGENT).  turn_0 = atan2(u_0.y, u_0.x).  For i >= 1:  c = u_(i-1).x * u_i.y - u_(i-1).y * u_i.x, a zero of either sign counting as +0.0;
 *   d = u_(i-1).x * u_i.x + u_(i-1).y * u_i.y;  turn_i = atan2(c, d), the fp64 library function (a few ulp from the correctly rounded value).  A path that reverses
 *   on itself turns by +PI.  turns_in (B,n) doubles, where given, replace ALL n turns (no atan2 is evaluated; the tangents are still formed for the velocities and
 *   for info).  turns_out (B,n) receives the turns used: feeding it back as turns_in reproduces every output bit for bit.  With DGP_HEADING_LINEAR no turn is formed:
 *   turns_in is not read and turns_out is all +0.0.
 *   psi = SCAN(e) with e_0 = 0.0 and e_i = turn_i (i >= 1): psi_0 = 0, psi_i = turn_1 + ... + turn_i in the association order of dgp_prior_samples' SCAN, a function
 *   of n alone -- inside each block of 64 consecutive indices starting at a multiple of 64, for off = 1, 2, 4, 8, 16, 32 in turn and for all i of the block with
 *   i % 64 >= off at once, e_i <- e_(i - off) + e_i; then, block after block from the second on, e_i <- c + e_i for every i of the block, c the finished value of the
 *   last index of the block before.
 * End headings theta_s, theta_g, each end by its own mode.  DGP_END_SUPPLIED: start_heading[b] / goal_heading[b].  DGP_END_TANGENT (DGP_HEADING_TANGENT only):
 *   theta_s = turn_0 with e_s = 0, and e_g = 0, by definition.  DGP_END_RANDOM: ONE Philox4x32-10 block per problem, key (seed & 0xffffffff, seed >> 32), counter
 *   (problem lo, problem hi, 0, 2), problem = first_problem + b (stream 2 next to dgp_sample_problems' 0 and 1); u0, u1 from the four words as for
 *   dgp_sample_problems (53 bits, [0, 1));  theta_s = (-PI) + u0 * TWO_PI,  theta_g = (-PI) + u1 * TWO_PI.
 * Headings, DGP_HEADING_TANGENT.  e_s = wrap(theta_s - turn_0);  base = theta_s - e_s;  phi_i = base + psi_i;  e_g = wrap(theta_g - phi_N);
 *   ws_i = fmax(0, 1 - (double)i / (double)blend),  wg_i = fmax(0, 1 - (double)(N - i) / (double)blend);
 *   theta_i = (phi_i + ws_i * e_s) + wg_i * e_g, except that row 0 stores theta_s itself and row N stores phi_N + e_g: the representative of the goal heading nearest
 *   the path's own winding, which is what `goal` carries.
 * Headings, DGP_HEADING_LINEAR.  theta_i = theta_s * (double)(N - i) * 1.0 / (double)N * 1.0 + theta_g * (double)i * 1.0 / (double)N * 1.0: straight_line_trajb's
 *   expression and order.  No wrap.
 * Velocities.  DGP_VEL_KEEP: columns 3, 4 of th are columns 2, 3 of th2 copied bit for bit, and column 5 is (w_N - w_0) / total_time_sec * 1.0 on every row, with
 *   (w_0, w_N) = (theta_s, theta_g) under DGP_HEADING_LINEAR (the reference's avg_vel is formed from the configurations, not from the rows) and the stored
 *   (theta_0, theta_N) = (theta_s, phi_N + e_g) under DGP_HEADING_TANGENT.  LINEAR + KEEP on the planar straight line is straight_line_trajb with dof = 3 bit for bit.
 *   DGP_VEL_DIFF: den = (double)(hi - lo) * Delta;  vx_i = t_i.x / den, vy_i = t_i.y / den (the unfilled tangent);  omega_i = (theta_hi - theta_lo) / den, from the
 *   headings as doubles, before the store rounding.
 * start = [x_0, y_0, theta_0, 0, 0, 0] and goal = [x_N, y_N, theta_N, 0, 0, 0], the values row 0 and row N of th store.
 * info (B): bit 0 every tangent degenerate; bit 1 some row's tangent was degenerate (it was filled); bit 2 some |turn_i| > PI / 2.0, i >= 1 (of the turns used);
 *   bit 3 a non-finite position or supplied heading.  Bits 0-2 are clear under DGP_HEADING_LINEAR.
 * th2 (B,n,4), start, goal, th of io_dtype; start_heading, goal_heading (B), turns_in, turns_out (B,n) doubles.  Pointers need only be aligned to their element type
 * (rows move as 8- / 16-byte vectors where the addresses allow, the same bits either way).  Every output is always written; turns_out and info may be NULL.  A
 * trajectory's result is a pure function of its own inputs (and of (seed, first_problem + b) for random ends): independent of batch size, position in the batch and
 * launch shape.
 * DGP_EINVAL, nothing launched: a NULL handle, params, th2, start, goal or th; dof != 3; batch < 1; an unknown mode; DGP_END_TANGENT under DGP_HEADING_LINEAR;
 * DGP_END_SUPPLIED with its array NULL; blend outside 1 .. N.  One launch, no atomics, nothing allocated or synchronised: capturable in a HIP graph. */
#define DGP_HEADING_LINEAR   0   /* theta_i = ths*(N-i)*1.0/N*1.0 + thg*i*1.0/N*1.0, straight_line_trajb's expression and order */
#define DGP_HEADING_TANGENT  1
#define DGP_END_SUPPLIED 0       /* start_heading / goal_heading arrays */
#define DGP_END_TANGENT  1       /* the path's own end tangents (TANGENT heading mode only) */
#define DGP_END_RANDOM   2       /* Philox */
#define DGP_VEL_KEEP 0           /* vx, vy copied from th2; one constant omega on every row */
#define DGP_VEL_DIFF 1           /* finite differences of the stored positions and headings */
typedef struct DgpHeadingParams {
  int32_t  heading_mode, start_end, goal_end, velocity_mode;
  int32_t  blend;          /* rows over which an end's heading error is blended out, 1 .. N */
  int32_t  reserved;       /* not read */
  uint64_t seed, first_problem;   /* DGP_END_RANDOM */
} DgpHeadingParams;        /* 40 bytes */
int dgp_heading_lift(const DgpHandle* h /* dof 3 */, int32_t batch, const DgpHeadingParams* p,
                     const void* th2,                                           /* (B,n,4) io_dtype */
                     const double* start_heading, const double* goal_heading,   /* (B) or NULL */
                     const double* turns_in,                                    /* (B,n) or NULL */
                     void* start, void* goal, void* th,                         /* (B,1,6), (B,1,6), (B,n,6) io_dtype */
                     double* turns_out, int32_t* info,                          /* (B,n), (B); each may be NULL */
                     void* stream);

/* Multi-start selection, ONE launch: per problem, the dense collision check of each of its num_samples optimised trajectories, their total order, and the chosen
 * one gathered -- the back half of dgp_prior_samples -> dgp_gn_solve over the B S rows.  No counterpart in the reference, which optimises one trajectory per problem.
 * Inputs.  th: the optimised samples, io_dtype, (B,S,n,d) -- or (S,B,n,d) with sample_major, what S solve launches of B rows on per-problem grids leave behind;
 *   score (B,S) / (S,B) io_dtype or NULL (= all 0.0): smaller is better (err_final of dgp_gn_solve);  exclude (B,S) / (S,B) int32 or NULL: non-zero = unusable (info of
 *   dgp_gn_solve; bit 1 of dgp_prior_samples' info);  sdf as for dgp_gp_interpolate, batch_stride the distance between PROBLEMS' grids (0 = one shared grid), or
 *   NULL: no collision check;  env_index (B) int32 or NULL, as for dgp_sample_problems: problem b reads grid env_index[b] (NULL: grid b); needs sdf.
 * The dense check of a sample is dgp_gp_interpolate's, on the same N_d = (n - 1)(K + 1) + 1 dense states, K = num_inter: the same closed form and operation order, every
 *   dense state looked up at its unrounded fp64 position with epsilon eps, the same six numbers over dense states 1 .. N_d - 2, reduced by the same lanes in the same
 *   order.  sample_summary[b, s] is BIT FOR BIT what dgp_gp_interpolate(..., summary) returns for that trajectory on that grid, AVG_PENETRATION included.
 * Status bits of a sample (status (B,S), always problem-major like order and sample_summary):
 *   DGP_SEL_COLLIDING   NUM_COLLIDING != 0.  Never set without sdf.
 *   DGP_SEL_OUTSIDE     the position of ANY dense state 0 .. N_d - 1, the two end states included, lies outside the handle's closed [x_min, x_max] x [y_min, y_max]
 *                       (a NaN is outside): the rule of dgp_prior_samples' info bit 0 on the position the lookup takes.  Computed with or without sdf.
 *   DGP_SEL_NON_FINITE  one of the sample's n d stored values or its score is not finite, or MAX_PENETRATION is NaN.
 *   DGP_SEL_EXCLUDED    exclude != 0.
 * Tiers.  2: NON_FINITE or EXCLUDED.  0: not tier 2, not COLLIDING and not (require_inside and OUTSIDE).  1: the rest -- usable trajectories that collide or leave the map.
 * Total order.  Sample s precedes sample t iff, in turn: its tier is smaller; then, in tier 1 only, its MAX_PENETRATION is smaller (0 for every sample without sdf);
 *   then, in tiers 0 and 1, its score converted to double is smaller by `<` (-0.0 and 0.0 tie); then its index s is smaller.  Every key is an input or a bit-exact
 *   intermediate: the order is exact.  order[b] is that permutation of 0 .. S - 1, best first; best[b] = order[b][0].
 * th_best[b] (n,d) is a BIT COPY of the chosen trajectory: NaN payloads and -0.0 included, no arithmetic touches it (it moves as 16- / 8- / 4-byte words, whichever the
 *   addresses allow: pointers need only be aligned to their element type).
 * problem_summary (B, DGP_SELECT_COUNT) doubles: SOLVED 1.0 iff the chosen sample is of tier 0; NUM_ACCEPTED the number of tier-0 samples; BEST_INDEX; BEST_SCORE (as a
 *   double; 0.0 without score); BEST_MAX_PENETRATION (0.0 without sdf); BEST_STATUS the chosen sample's status bits.
 * Outputs: each may be NULL, not all six.  sample_summary needs sdf.
 * DGP_EINVAL, nothing launched: a NULL handle, th or p; a wrong struct_size; batch < 1; num_samples outside 1 .. 1024, or batch * num_samples >= 2^31; num_inter outside
 *   0 .. 1023; eps not finite; every output NULL; sample_summary or env_index without sdf (or without sdf->data); sdf given and N_d < 3.
 * Every num_states, both dof and both io_dtype a handle accepts are accepted (the heading of the dof 3 robot is a column like any other); row-major and DGP_SDF_TILED4
 * grids.  One workgroup per problem, the keys of its samples in LDS: one launch, no atomics, nothing allocated, copied or synchronised -- capturable in a HIP graph;
 * bit-identical from run to run, for either layout of th, either grid layout and wherever the problem sits in the batch. */
#define DGP_SEL_COLLIDING   1
#define DGP_SEL_OUTSIDE     2
#define DGP_SEL_NON_FINITE  4
#define DGP_SEL_EXCLUDED    8
#define DGP_SELECT_SOLVED               0
#define DGP_SELECT_NUM_ACCEPTED         1
#define DGP_SELECT_BEST_INDEX           2
#define DGP_SELECT_BEST_SCORE           3
#define DGP_SELECT_BEST_MAX_PENETRATION 4
#define DGP_SELECT_BEST_STATUS          5
#define DGP_SELECT_COUNT                6
typedef struct DgpSelectParams {
  uint32_t struct_size;     /* = sizeof(DgpSelectParams) */
  int32_t  num_inter;       /* K of the dense check, 0 .. 1023, as dgp_gp_interpolate */
  double   eps;             /* epsilon of the dense check's hinge, as dgp_gp_interpolate */
  int32_t  sample_major;    /* 0: th (B,S,n,d), score / exclude (B,S);  1: th (S,B,n,d), score / exclude (S,B) */
  int32_t  require_inside;  /* non-zero: DGP_SEL_OUTSIDE rejects a sample (tier 1) */
} DgpSelectParams;          /* 24 bytes */
int dgp_select_samples(const DgpHandle* h, int32_t batch, int32_t num_samples,
                       const void* th,             /* optimised samples, io_dtype */
                       const void* score,          /* io_dtype or NULL */
                       const int32_t* exclude,     /* int32 or NULL */
                       const DgpSdf* sdf,          /* or NULL: no collision check */
                       const int32_t* env_index,   /* (B) or NULL */
                       const DgpSelectParams* p,
                       void* th_best,              /* (B,n,d) io_dtype */
                       int32_t* best,              /* (B) */
                       int32_t* order,             /* (B,S) */
                       int32_t* status,            /* (B,S) */
                       double* sample_summary,     /* (B,S,DGP_DENSE_COUNT) */
                       double* problem_summary,    /* (B,DGP_SELECT_COUNT) */
                       void* stream);
/* What dgp_select_samples launches for num_samples samples checked with num_inter interpolated states (the function its dispatch itself reads): lanes per trajectory
 * (16 / 32 / 64, from N_d as for dgp_gp_interpolate), wavefronts of a problem's workgroup (up to 16) and the passes in which the workgroup walks the samples.  Any
 * pointer may be NULL.  No effect on any result. */
int dgp_select_launch_shape(const DgpHandle* h, int32_t num_samples, int32_t num_inter,
                            int32_t* lanes_per_traj, int32_t* waves_per_group, int32_t* passes);

/* Measurement aid (no counterpart in the reference): the NEXT kernel launched by the calling thread through any entry point
 * above records its own begin and end on the two HIP events (hipEvent_t, created with timing enabled, cast to void*), the way
 * hipExtLaunchKernelGGL does -- hipEventElapsedTime(start, stop) is then that kernel's execution time, the quantity
 * rocprofv3 --kernel-trace reports, with no marker packets between back-to-back launches.  One-shot: consumed by that launch.
 * Passing NULL for either event cancels a pending request. */
int dgp_time_next_launch(void* start_event, void* stop_event);
/* Events for dgp_time_next_launch, created and read through the HIP runtime this library is linked against (hipEvent_t as void*);
 * dgp_event_elapsed_ms needs both events completed (synchronise the stream first). */
int  dgp_event_create(void** out_event);
void dgp_event_destroy(void* event);
int  dgp_event_elapsed_ms(void* start_event, void* stop_event, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* DGPMP2_HIP_H */
