/* hpe.h — C ABI of libhpe.so, the MI355X (gfx950) head-pose regression hot path.
 *
 * The reference (Maaz77/Head-Pose-Estimation-Model) has no native code and no FFI: its boundary is
 * the Python/Keras API at the call sites below.  This ABI is what that Keras layer
 * bottoms out in once TF's CPU kernels are replaced; the Python host package
 * (head-pose-estimation-model_amd/hpe) binds it with ctypes and keeps the reference's surface.
 *
 *   hpe_program_create / _destroy   replaces keras.Model construction + compile
 *                                   (Model-96/train_96.py:65-110, Model-88/train_88.py:66-253,
 *                                    Model-88/attention_model.py:16-169): a compiled "row program"
 *                                    (per-position op list over a tile of rows kept in LDS)
 *   hpe_forward                     replaces model.predict (Model-96/test.py:34) and the forward of
 *                                   model.evaluate (train_96.py:186-187)
 *   hpe_train_step                  replaces one step of model.fit (train_96.py:175-183,
 *                                   train_88.py:355-363): forward + MSE + backward, per-workgroup
 *                                   gradient partials into the workspace
 *   hpe_reduce                      sums the per-workgroup partials into one flat gradient
 *                                   (the buffer RCCL all-reduces across ranks)
 *   hpe_optim_step                  replaces optimizer.apply_gradients of Keras' legacy SGD / Adam /
 *                                   Adamax (train_96.py:99-103, train_88.py:323) + the L2 penalty
 *                                   gradient of kernel_/bias_regularizer (train_96.py:78-79,90-91)
 *
 * Conventions: every buffer is a caller-owned DEVICE pointer (fp32 unless noted); every call is
 * stream-ordered on the hipStream_t passed as `stream` (0 = null stream) and never synchronises,
 * allocates or frees (graph-capturable).  Return value 0 = OK; otherwise hpe_last_error() (thread
 * local) holds the message.  Handles are not thread-safe; one per device.
 */
#ifndef HPE_H
#define HPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hpe_program hpe_program;

/* Error codes */
#define HPE_OK 0
#define HPE_EINVAL 1   /* bad argument / shape (the Python layer raises ValueError) */
#define HPE_ERUNTIME 2 /* HIP runtime failure (RuntimeError) */

/* Optimizer kinds (Keras legacy optimizers) */
#define HPE_OPT_SGD 0
#define HPE_OPT_ADAM 1
#define HPE_OPT_ADAMAX 2

/* Create a program from the int32 word stream produced by hpe/compiler.py (layout documented in
 * csrc/hpe_prog.h).  Copies the words to device memory owned by the handle. */
int hpe_program_create(const int32_t *words, int64_t n_words, hpe_program **out);
int hpe_program_destroy(hpe_program *prog);

/* Number of workgroups a launch over n_rows rows uses, and the workspace bytes hpe_train_step
 * needs for it: grid x (n_params + 4) floats of per-workgroup partials. */
int hpe_launch_grid(const hpe_program *prog, int64_t n_rows);
size_t hpe_workspace_size(const hpe_program *prog, int64_t n_rows);

/* Forward over n_images images of P positions each (rows = n_images * P, channels-last rows of
 * C_in floats).  image_index (int32, may be NULL) gathers images: row r reads image
 * image_index[r / P].  y: n_images * P * C_out floats, channel order yaw, pitch, roll. */
int hpe_forward(const hpe_program *prog, const float *params, const float *params_t,
                const float *x, int64_t n_images, int32_t P, const int32_t *image_index,
                float *y, void *stream);

/* One training (or, with a program compiled for evaluation, loss-only) pass.  y_true: per-image
 * labels [n_images_total][C_out] indexed like x.  image_offset: global index of this rank's first
 * image (dropout hash).  inv_count: 1 / (global rows * C_out), the MSE normaliser.  workspace:
 * hpe_workspace_size() bytes; receives per-workgroup partial gradients and [sum e^2, sum |e|]. */
int hpe_train_step(const hpe_program *prog, const float *params, const float *params_t,
                   const float *x, const float *y_true, int64_t n_images, int32_t P,
                   const int32_t *image_index, int64_t image_offset, float inv_count,
                   uint64_t dropout_seed, void *workspace, void *stream);

/* hpe_train_step with the caller's bound on max |x| over the rows the launch reads (0 = unknown).
 * The fused kernels compute the GEMMs on an fp16 split whose data side holds |x| < 64 and hand a launch
 * whose split overflowed to an exact-fp32 twin launched behind it; with x_bound in (0, 64) the twin
 * cannot be needed and is not launched (fit bounds its resident dataset once per call). */
int hpe_train_step_bounded(const hpe_program *prog, const float *params, const float *params_t,
                           const float *x, const float *y_true, int64_t n_images, int32_t P,
                           const int32_t *image_index, int64_t image_offset, float inv_count,
                           uint64_t dropout_seed, float x_bound, void *workspace, void *stream);

/* grad[i] = sum over workgroups of workspace partials, i < n_params + 4 (fixed order). */
int hpe_reduce(const hpe_program *prog, int64_t n_rows, const void *workspace, float *grad,
               void *stream);

/* Keras legacy optimizer step on the flat parameter vector:
 *   g = grad[i] * grad_scale + 2 * l2[i] * w[i]
 *   SGD:    w -= lr g
 *   Adam:   m += (g - m)(1-b1); v += (g^2 - v)(1-b2); w -= alpha m / (sqrt(v) + eps),
 *           alpha = lr sqrt(1-b2^t) / (1-b1^t)
 *   Adamax: m += (g - m)(1-b1); v = max(b2 v, |g|); w -= lr/(1-b1^t) m / (v + eps)
 * t = iter (1-based).  tpos[i] >= 0 mirrors the new w[i] into params_t[tpos[i]] (the transposed
 * copy the backward GEMMs read).  grad holds n + 4 floats (the step's [sum e^2, sum |e|] follow
 * the gradient).  stats receives [grad[n], grad[n+1], reg_0 .. reg_{grid-1}] where reg_b is block
 * b's share of sum l2[i] w[i]^2 on the pre-update weights (the Keras regularisation loss). */
int hpe_optim_step(int32_t kind, float lr, float beta_1, float beta_2, float epsilon, int64_t iter,
                   float grad_scale, float *params, float *params_t, float *m, float *v,
                   const float *grad, const float *l2, const int32_t *tpos, int64_t n,
                   float *stats, void *stream);
/* Blocks hpe_optim_step launches (stats holds 2 + this many floats). */
int hpe_optim_grid(int64_t n);

/* hpe_reduce followed by hpe_optim_step in ONE launch, for a single rank (no all-reduce between
 * them): grad receives exactly what hpe_reduce writes (bit-identical: same summation order), the
 * parameters / moments / stats exactly what hpe_optim_step then writes.  n must equal the program's
 * trained-parameter count.  Used by the per-step fit path at small launch grids (P = 1 batches). */
int hpe_reduce_optim_step(const hpe_program *prog, int64_t n_rows, const void *workspace, float *grad,
                          int32_t kind, float lr, float beta_1, float beta_2, float epsilon, int64_t iter,
                          float grad_scale, float *params, float *params_t, float *m, float *v,
                          const float *l2, const int32_t *tpos, int64_t n, float *stats, void *stream);

/* One epoch of model.fit's per-step path for a single rank, the step loop in C (replaces the
 * Python step loop of Keras fit, train_96.py:175-183, for programs the whole-epoch kernel does not
 * take: P > 1 maps, batches above its limit, every graph the fused kernels do not cover).  For
 * s = 0 .. ceil(n / batch) - 1 with rows perm[s*batch .. min(n, (s+1)*batch)): hpe_train_step_bounded
 * (dropout seed seed_base + iter0 + 1 + s, inv_count = (float)(1.0 / (rows * P * 3)), x_bound), then
 * hpe_reduce_optim_step when hpe_launch_grid <= 16, else hpe_reduce + hpe_optim_step, with iteration
 * iter0 + 1 + s and stats + s * stats_stride — the launches fit issues from Python, bit-identical.
 * Each stats row receives hpe_optim_step's [sse, sae, reg_0 .. reg_{grid-1}]: stats_stride must be
 * >= 2 + hpe_optim_grid(n_train) (HPE_EINVAL otherwise), stats holds ceil(n / batch) rows. */
int hpe_fit_steps(const hpe_program *prog, float *params, float *params_t, float *m, float *v,
                  const float *l2, const int32_t *tpos, int64_t n_train, const float *x,
                  const float *y_true, const int32_t *perm, int64_t n, int32_t batch, int32_t P,
                  float x_bound, int32_t kind, float lr, float beta_1, float beta_2, float epsilon,
                  uint64_t seed_base, int64_t iter0, void *workspace, float *grad, float *stats,
                  int32_t stats_stride, void *stream);

/* One epoch of a DATA-PARALLEL rank's fit with the step loop in C (replaces the Python step loop of
 * hpe/model.py's distributed fit; the reference's loop: train_96.py:175-183).  Per step s over rows
 * perm[b0 .. b0 + nb) of the global batch (b0 = s * batch): this rank's share [r0, r1) with
 * r0 = b0 + nb * rank / world, r1 = b0 + nb * (rank + 1) / world; hpe_train_step_bounded on it
 * (img_off = r0 - b0, inv_count = (float)(1.0 / (nb * P * 3)): the GLOBAL count) + hpe_reduce into
 * grad (n_train + 4 floats; zeroed when the share is empty), then allreduce(grad, n_train + 4,
 * stream, user) — the caller's sum over ranks, e.g. an RCCL all-reduce on that stream; non-zero
 * aborts with HPE_ERUNTIME — then hpe_optim_step with iteration iter0 + 1 + s into
 * stats + s * stats_stride (stats_stride >= 2 + hpe_optim_grid(n_train)).  Bit-identical to the
 * per-step launches issued one by one.  steps_done (may be NULL) receives the number of steps whose
 * optimizer update was issued, also when the epoch stops early on an error (the caller advances its
 * iteration count by it). */
typedef int (*hpe_allreduce_fn)(float *buf, int64_t n, void *stream, void *user);
int hpe_fit_steps_dp(const hpe_program *prog, float *params, float *params_t, float *m, float *v,
                     const float *l2, const int32_t *tpos, int64_t n_train, const float *x,
                     const float *y_true, const int32_t *perm, int64_t n, int32_t batch, int32_t P,
                     float x_bound, int32_t kind, float lr, float beta_1, float beta_2, float epsilon,
                     uint64_t seed_base, int64_t iter0, void *workspace, float *grad, float *stats,
                     int32_t stats_stride, int32_t rank, int32_t world, hpe_allreduce_fn allreduce,
                     void *user, int64_t *steps_done, void *stream);

/* Native RCCL all-reduce for hpe_fit_steps_dp on GPU ranks (csrc/hpe_rccl.hip; librccl opened at
 * run time): replaces the caller's per-step hook (e.g. a torch.distributed callback, one
 * interpreter re-entry per step) by an RCCL sum enqueued on the step's own stream.  Rank 0 calls
 * hpe_rccl_unique_id, the caller broadcasts the HPE_RCCL_ID_BYTES bytes to every rank, each rank
 * calls hpe_rccl_comm_init on its current device; then hpe_fit_steps_dp(..., allreduce =
 * hpe_rccl_allreduce, user = the communicator, ...).  hpe_rccl_available: 1 when librccl loads. */
#define HPE_RCCL_ID_BYTES 128
int hpe_rccl_available(void);
int hpe_rccl_unique_id(void *id_out);
int hpe_rccl_comm_init(const void *id, int32_t nranks, int32_t rank, void **comm_out);
int hpe_rccl_comm_destroy(void *comm);
int hpe_rccl_allreduce(float *buf, int64_t n, void *stream, void *comm);

/* ---------------------------------------------------------------------------------------------
 * One whole epoch of model.fit in ONE launch (csrc/hpe_fit.hip) — replaces the per-step loop of
 * Keras fit (train_96.py:175-183, train_88.py:355-363) for the reference's own regime: 1x1 maps
 * (P = 1), the 2-layer create_model family (programs of kind mlp2 compiled for training), one rank.
 * Equivalent to, for s = 0 .. ceil(n / batch) - 1 with rows perm[s*batch .. min(n, (s+1)*batch)):
 *   hpe_train_step (dropout_seed = seed_base + iter0 + 1 + s, inv_count = 1 / (rows * 3)),
 *   hpe_reduce, hpe_optim_step(kind, lr, beta_1, beta_2, epsilon, iter0 + 1 + s, 1.0)
 * with alpha[s] the optimizer step size hpe_optim_step derives for that iteration (lr for SGD,
 * lr sqrt(1-b2^t)/(1-b1^t) for Adam, lr/(1-b1^t) for Adamax; device array of ceil(n / batch)).
 * params / params_t / m / v are updated in place; stats[s * stats_stride + ...] receives the
 * step's [sum e^2, sum |e|, reg_0 .. reg_{G-1}] (G = ceil(F / 32) workgroups; the regularisation
 * loss on the pre-update weights is the sum of the reg_g).  exact != 0 runs exact-fp32 MFMA GEMMs.
 * workspace: hpe_fit_workspace_size bytes; after the launch its int word [1] holds flags
 * (1: a split accumulator was non-finite — rerun the epoch with exact = 1 from the saved state;
 * 2: the per-step workgroup exchange timed out — the workgroups may have stopped at different
 * steps, so restore params / m / v and run the epoch per step).  hpe_fit_supported: 1 if program
 * + batch qualify: F <= 1024 (G <= 32), batch <= 512, the exchange table G * batch * 3 floats
 * within 9,216 (batch <= 256) or 25,600 (batch 257..512), and all G workgroups co-resident (one
 * per CU, G <= CUs / 8); 0 otherwise (and without a device).  Env HPE_FIT_FORCE_TIMEOUT=1 (tests)
 * raises flag 2 at the first exchange. */
int hpe_fit_supported(const hpe_program *prog, int32_t batch);
size_t hpe_fit_workspace_size(const hpe_program *prog, int32_t batch);
int hpe_fit_epoch(const hpe_program *prog, float *params, float *params_t, float *m, float *v,
                  const float *l2, const int32_t *tpos, const float *x, const float *y_true,
                  const int32_t *perm, int64_t n, int32_t batch, int32_t kind, float lr, float beta_1,
                  float beta_2, float epsilon, const float *alpha, uint64_t seed_base, int64_t iter0,
                  float *stats, int32_t stats_stride, int32_t exact, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Several independent trainings ("trials") in ONE epoch launch.  hpe_fit_epoch uses one workgroup
 * per 32 hidden units in the blocks with blockIdx % 8 == 0 of an 8 G grid; the other seven eighths
 * of that grid carry further trials here, each a closed group of workgroups running the same
 * per-trial arithmetic as hpe_fit_epoch (bit-identical results).  Nothing crosses trials: each has
 * its own parameters, optimizer state, permutation, seeds, stats and workspace (with its own flags
 * word [1], as above).  hpe_fit_trial holds hpe_fit_epoch's arguments of one trial.
 *
 * hpe_fit_multi_plan (host arithmetic only, no device call): deals trials with groups[i] = G_i
 * workgroups to the 8 lanes blockIdx % 8 by decreasing G (ties in input order), each to the first
 * lane of least load that still fits it (eight trials go one per lane), a lane holding at most
 * lane_cap workgroups; trial i's workgroup c is block 8 (first_c[i] + c) + lane[i].
 * Returns the number of trials placed: the longest prefix of the input that fits one launch (the
 * rest, lane = first_c = -1, is for a later launch); 0 if some G_i is < 1 or > lane_cap.
 * hpe_fit_multi_lane_cap: lane_cap of the current device for prog's kernel (occupancy x CUs / 8:
 * the whole grid of 8 max(lane load) workgroups is resident at once).  hpe_fit_multi_instance: an
 * id of prog's kernel instance (input width 88 / 96, activation class tanh / softsign / other), -1
 * if hpe_fit_epoch_multi cannot run it; all trials of one launch must share it.
 * hpe_fit_multi_supported: 1 if every trial passes hpe_fit_supported for its batch, none is a
 * residual stack, all share one instance and the plan places all of them.
 * hpe_fit_epoch_multi: one launch for all trials (HPE_EINVAL if !hpe_fit_multi_supported); zeroes
 * every trial's workspace first.  table: hpe_fit_multi_table_size(n_trials) bytes of device memory,
 * written here through the stream (the call waits for that copy; the table must stay untouched
 * until the launch has finished).  With n_trials == 1 the call is hpe_fit_epoch of that trial: the
 * same launch (the trial's arguments by value on its 8 G grid), so the table, still required, is
 * neither written nor waited for.  hpe_fit_epoch is that one-trial case with its arguments spread
 * out. */
typedef struct hpe_fit_trial {
  const hpe_program *prog;
  float *params, *params_t, *m, *v;
  const float *l2;
  const int32_t *tpos;
  const float *x, *y_true;
  const int32_t *perm;
  int64_t n;
  int32_t batch, kind;
  float lr, beta_1, beta_2, epsilon;
  const float *alpha;
  uint64_t seed_base;
  int64_t iter0;
  float *stats;
  int32_t stats_stride;
  void *workspace;
} hpe_fit_trial;
int hpe_fit_multi_plan(const int32_t *groups, int32_t n_trials, int32_t lane_cap, int32_t *lane,
                       int32_t *first_c);
int hpe_fit_multi_lane_cap(const hpe_program *prog);
int hpe_fit_multi_instance(const hpe_program *prog);
size_t hpe_fit_multi_table_size(int32_t n_trials);
int hpe_fit_multi_supported(const hpe_fit_trial *trials, int32_t n_trials);
int hpe_fit_epoch_multi(const hpe_fit_trial *trials, int32_t n_trials, int32_t exact, void *table,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * Several residual stacks (programs of kind res: create_model_complex and the stacks like it,
 * csrc/hpe_res.hip) in ONE epoch launch.  hpe_fit_epoch trains such a program with one workgroup for
 * the whole epoch; here block b of a grid of n_trials workgroups trains trials[b], with the same
 * arithmetic (bit-identical results).  A trial is one workgroup that talks to no other, so there is
 * no placement plan and no residency cap: blocks beyond what the card holds at once simply wait for
 * a CU.  Nothing crosses trials: each has its own program (dropout rates, layer table), parameters,
 * optimizer state and kind, L2 vector, permutation, step sizes, seeds, stats rows ([sum e^2,
 * sum |e|, regularisation loss] per step, stats_stride >= 3) and workspace, whose flags word [1] is
 * always 0 after the launch (every GEMM is exact fp32 and no workgroup waits for another).  There is
 * no `exact` argument for the same reason.  The existing entry points keep refusing these programs:
 * hpe_fit_multi_instance returns -1, hpe_fit_multi_lane_cap 0, hpe_fit_epoch_multi HPE_EINVAL.
 *
 * hpe_res_fit_multi_instance: an id of prog's kernel instance (input width 88 / 96, number of
 * residual blocks, with / without the bottleneck, compiled-in softsign / relu against run-time
 * activations), -1 if prog is NULL or not a supported residual-stack training program; all trials of
 * one launch must share it.  hpe_res_fit_multi_instance_words: the same id from the word stream
 * hpe_program_create takes (-1 if it is not a well-formed one).  Both are host arithmetic only and
 * need no device.
 * hpe_res_fit_multi_table_size: bytes of device memory for the launch's argument table (0 if
 * n_trials < 1).
 * hpe_res_fit_epoch_multi: checks every trial before any device call (hpe_fit_epoch's argument
 * checks, kind res, stats_stride >= 3, one shared instance; otherwise HPE_EINVAL with a message that
 * names the trial), zeroes each trial's workspace, writes the table through the stream (the call
 * waits for that copy; the table must stay untouched until the launch has finished) and makes one
 * launch of n_trials workgroups.  With n_trials == 1 the call is hpe_fit_epoch of that trial: the
 * same launch on a grid of one with the arguments passed by value; the table, still required, is
 * neither written nor waited for. */
int hpe_res_fit_multi_instance(const hpe_program *prog);
int hpe_res_fit_multi_instance_words(const int32_t *words, int64_t n_words);
size_t hpe_res_fit_multi_table_size(int32_t n_trials);
int hpe_res_fit_epoch_multi(const hpe_fit_trial *trials, int32_t n_trials, void *table, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BlazeFace backbone — replaces the TF call on the fused BlazeFace+regressor
 * graph, `self.model.predict(...)` at BlazePoser/blazeFaceDetectorH5.py:272, for a whole batch.
 * words: the plan hpe/blazeface.py builds from the unified model's model_config (csrc/hpe_prog.h
 * BFH_* / BFO_*); params: the plan's flat fp32 parameter vector (device).
 * images: (n_images, 128, 128, 3) NHWC fp32 in [-1, 1] (the detector's preprocessed input).
 * outs: six device pointers (host array), in the unified model's output order:
 *   [0] classificators_1 (n,512,1)  [1] classificators_2 (n,384,1)
 *   [2] regressors_1 (n,512,16)     [3] regressors_2 (n,384,16)
 *   [4] re_lu_10 tap (n,16,16,88)   [5] re_lu_15 tap (n,8,8,96)
 * The two pose regressors of the unified model (`model` on re_lu_10, `model_10` on re_lu_15) run
 * on the taps through hpe_forward (programs compiled with P = 256 and P = 64).
 * workspace: hpe_blazeface_workspace_size(h, n_images) bytes of device memory. */
typedef struct hpe_blazeface hpe_blazeface;
int hpe_blazeface_create(const int32_t *words, int64_t n_words, hpe_blazeface **out);
int hpe_blazeface_destroy(hpe_blazeface *h);
size_t hpe_blazeface_workspace_size(const hpe_blazeface *h, int64_t n_images);
int hpe_blazeface_forward(const hpe_blazeface *h, const float *params, const float *images,
                          int64_t n_images, float *const *outs, void *workspace, void *stream);

/* Detector post-processing of the unified graph for a batch of frames,
 * replacing blazeFaceDetector.filterDetections / extractDetections / filterWithNonMaxSupression
 * (BlazePoser/blazeFaceDetectorH5.py:284-357) per frame:
 *   keep logit > score_logit_threshold (fp32; the reference's log(t/(1-t))), score = sigmoid (fp32),
 *   decode boxes / 6 keypoints against the 896 SSD anchors in fp64, greedy NMS with
 *   tf.image.non_max_suppression semantics (IoU in fp32, suppress iff IoU > iou_threshold, at most
 *   max_faces kept), and gather each kept detection's pose from its 16x16 / 8x8 regressor cell.
 *   The IoU, the score order and the greedy pass are defined once, in csrc/hpe_boxes.h, for this
 *   function, hpe_merge_rois and hpe_track.
 * Inputs (device): cls0 (n,512), cls1 (n,384), loc0 (n,512,16), loc1 (n,384,16), pose0 (n,16,16,3),
 * pose1 (n,8,8,3).  Outputs (device, per frame max_faces slots, the first count[i] valid, in NMS
 * selection order): det_index int32, scores f32, boxes f64 [x1,y1,x2,y2], keypoints f64 [6][2],
 * poses f32 [yaw, pitch, roll]. */
int hpe_detect(const float *cls0, const float *cls1, const float *loc0, const float *loc1,
               const float *pose0, const float *pose1, int64_t n_images, float score_logit_threshold,
               float iou_threshold, int32_t max_faces, int32_t *count, int32_t *det_index, float *scores,
               double *boxes, double *keypoints, float *poses, void *stream);

/* Feature-dataset extraction (the *_features_88|96_<t>_<k>.npz files of
 * FeatureMaps-Datasets/, whose extractor is outside the reference, JoinModels.py:114 taps re_lu_10 /
 * re_lu_15): for the first k kept detections of each frame (hpe_detect outputs), the regressor input
 * that detection's pose was computed from, following the pose gather at blazeFaceDetectorH5.py:342-353
 * — d < 512: tap0 (n,16,16,c0) cell d/2; else tap1 (n,8,8,c1) cell (d-512)/6.  Outputs (device):
 * feat0 (n,k,c0), feat1 (n,k,c1) (the other tap's row zero), src (n,k) int32 0 / 1 / -1 (empty). */
int hpe_gather_features(const int32_t *count, const int32_t *det_index, int64_t n_images, int32_t max_faces,
                        int32_t k, const float *tap0, int32_t c0, const float *tap1, int32_t c1, float *feat0,
                        float *feat1, int32_t *src, void *stream);

/* Raw camera frames -> network input (csrc/hpe_preproc.hip), replacing prepareInputForInference
 * (BlazePoser/blazeFaceDetectorH5.py:247-269: cv2.COLOR_BGR2RGB, / 255.0, tf.image.resize(method=
 * 'bicubic') to the model input, (x - 0.5) / 0.5) for a whole batch in one launch.
 * frames: n device images of in_h x in_w x 3 bytes, rows row_stride_bytes apart (>= 3 * in_w), frames
 * in_h * row_stride_bytes apart.  The crop rectangle (crop_x0, crop_y0, crop_w, crop_h), which must lie
 * inside the frame, is what gets resized (the webcam loop's centre crop, :394-399).  bgr != 0 reverses
 * the channel order.  out: (n, out_h, out_w, 3) fp32 RGB in [-1, 1] up to the bicubic overshoot —
 * the `images` argument of hpe_blazeface_forward.
 * Arithmetic: TF 2.x ResizeBicubic with half_pixel_centers (Keys cubic A = -0.5 through a 1/1024
 * weight table, taps clamped to the crop, clamped taps dropped and the rest renormalised), every
 * fp32 operation rounded on its own (no FMA contraction), tap value (float)((double)byte / 255.0);
 * tests/bicubic_ref.py restates it bit for bit.  n * out_h * out_w must fit int32; n == 0 is a no-op. */
int hpe_preprocess(const uint8_t *frames, int64_t n, int32_t in_h, int32_t in_w, int64_t row_stride_bytes,
                   int32_t crop_x0, int32_t crop_y0, int32_t crop_w, int32_t crop_h, int32_t bgr,
                   float *out, int32_t out_h, int32_t out_w, void *stream);

/* hpe_preprocess per region of interest: many rectangles per frame, each with its own frame, and
 * rectangles that reach outside the frame (a second look at each face, frames placed on a larger
 * canvas, batches whose frames need different crops).
 * rois: device table (m, 5) int32, row r = (frame, x0, y0, w, h) in frame pixels.  Output r is exactly
 * what hpe_preprocess produces for a whole h x w canvas whose pixel (y, x) is frames[frame, y0 + y,
 * x0 + x] where that lies inside the frame and the bytes (pad_b0, pad_b1, pad_b2), in the frame's own
 * channel order, elsewhere: the taps clamp to the canvas, not to the frame.  So an ROI inside the
 * frame equals hpe_preprocess with that crop, and an ROI reaching outside equals hpe_preprocess on a
 * host-padded copy, bit for bit.
 * The table is on the device, so its rows are checked there: a row is valid iff 0 <= frame < n_frames,
 * 1 <= w, h <= 2^24 and |x0|, |y0| <= 2^24 (every coordinate sum then fits int32).  An invalid row
 * reads no frame memory; its output is the constant (lut[pad_c] - 0.5f) / 0.5f per channel, after the
 * bgr swap.  Checked on the host (HPE_EINVAL): negative n_frames or m, non-positive sizes, a stride
 * below 3 * in_w, pad bytes outside 0..255, m * out_h * out_w beyond int32, null pointers when m > 0
 * (`frames` may be null when n_frames == 0: no row is valid then).  m == 0 is a no-op.
 * out: (m, out_h, out_w, 3) fp32. */
int hpe_preprocess_rois(const uint8_t *frames, int64_t n_frames, int32_t in_h, int32_t in_w,
                        int64_t row_stride_bytes, const int32_t *rois, int64_t m, int32_t pad_b0,
                        int32_t pad_b1, int32_t pad_b2, int32_t bgr, float *out, int32_t out_h, int32_t out_w,
                        void *stream);

/* hpe_preprocess / hpe_preprocess_rois reading decoded NV12 video frames (what a hardware or software
 * decoder and most cameras deliver) instead of packed BGR: the colour conversion happens per tap
 * inside the gather, and everything after it is the BGR path with bgr = 1, so the output equals, bit
 * for bit, hpe_preprocess(_rois) of the frame converted to BGR bytes by the rule below.
 * Frame layout: y: n luma planes of in_h x in_w bytes, rows y_row_stride apart, frames y_frame_stride
 * apart (bytes); uv: n chroma planes of in_h / 2 rows of in_w bytes (in_w / 2 interleaved U, V pairs),
 * rows uv_row_stride apart, frames uv_frame_stride apart.  The planes may be separate allocations with
 * their own pitch; the packed (3 in_h / 2, in_w) layout is uv = y + in_h * pitch.  in_h and in_w must
 * be even.  The chroma of pixel (y, x) is the pair uv[y >> 1][x >> 1] (the nearest sample, shared by
 * the four pixels of a 2 x 2 block; no chroma interpolation).  No byte outside [row start, row start
 * + in_w) of either plane is read.
 * Conversion, int32, OpenCV's fixed-point form with a shift of 20 (limited range in, full range out):
 *   yy = max(Y - 16, 0) * CY,  u = U - 128,  v = V - 128
 *   R = sat8((yy + CVR * v           + (1 << 19)) >> 20)
 *   G = sat8((yy + CVG * v + CUG * u + (1 << 19)) >> 20)
 *   B = sat8((yy + CUB * u           + (1 << 19)) >> 20)
 * with >> an arithmetic shift (a floor for negative sums) and sat8 a clamp to 0..255; the sums stay
 * below 2^31 for every (Y, U, V).  matrix picks the coefficients (CY, CVR, CVG, CUG, CUB):
 *   0, BT.601: 1220542, 1673527, -852492, -409993, 2116026 (the constants of OpenCV's
 *              COLOR_YUV2BGR_NV12)
 *   1, BT.709: 1220945, 1879825, -558796, -223607, 2215014 (round(c * 2^20) of the exact BT.709
 *              limited-range matrix)
 * tests/nv12_ref.py restates the rule.  out is RGB, as from hpe_preprocess with bgr = 1.
 * Checked on the host (HPE_EINVAL) before any device call: a negative n, non-positive or odd in_h /
 * in_w, non-positive crop or output sizes, a crop outside the frame, row strides below in_w, negative
 * frame strides, matrix outside 0..1, counts and strides that overflow, null pointers when n > 0.
 * n == 0 is a no-op. */
int hpe_preprocess_nv12(const uint8_t *y, const uint8_t *uv, int64_t n, int32_t in_h, int32_t in_w,
                        int64_t y_row_stride, int64_t y_frame_stride, int64_t uv_row_stride,
                        int64_t uv_frame_stride, int32_t matrix, int32_t crop_x0, int32_t crop_y0,
                        int32_t crop_w, int32_t crop_h, float *out, int32_t out_h, int32_t out_w, void *stream);

/* hpe_preprocess_rois on NV12 frames (described as for hpe_preprocess_nv12): the table, the validity
 * rule, the frame-or-pad decision per tap and the invalid row's output are those of
 * hpe_preprocess_rois with bgr = 1.  The pad bytes are given as B, G, R and used as they are, not
 * converted.  Also checked on the host: pad bytes outside 0..255, a negative m, m * out_h * out_w
 * beyond int32, null pointers when m > 0 (`y` and `uv` may be null when n_frames == 0).  m == 0 is a
 * no-op. */
int hpe_preprocess_rois_nv12(const uint8_t *y, const uint8_t *uv, int64_t n_frames, int32_t in_h, int32_t in_w,
                             int64_t y_row_stride, int64_t y_frame_stride, int64_t uv_row_stride,
                             int64_t uv_frame_stride, const int32_t *rois, int64_t m, int32_t pad_b,
                             int32_t pad_g, int32_t pad_r, int32_t matrix, float *out, int32_t out_h,
                             int32_t out_w, void *stream);

/* hpe_detect's outputs -> the ROI table of a second detector pass (an enlarged square around every
 * face), on the device.  count (n_images), boxes (n_images, max_faces, 4) as hpe_detect wrote them,
 * normalised to the source rectangle (src_x0, src_y0, src_w, src_h) of the first pass in frame pixels.
 * For frame i and detection j < count[i], in float64 with every operation rounded on its own:
 *   px1 = src_x0 + x1 * src_w (likewise py1, px2, py2), cx = 0.5 * (px1 + px2), cy = 0.5 * (py1 + py2),
 *   side = scale * max(px2 - px1, py2 - py1), S = clamp(ceil(side), 1, 2^24),
 *   rx = floor(cx - 0.5 * S), ry = floor(cy - 0.5 * S), each clamped to +-2^24;
 * the row is (i, rx, ry, S, S), or the invalid row (-1, 0, 0, 0, 0) if cx, cy or side is not finite.
 * Rows are compacted frame-major in NMS order (offsets are a prefix sum over count, so the order is
 * deterministic); n_rois[0] receives their number and the rows past it, up to n_images * max_faces,
 * are (-1, 0, 0, 0, 0).  rois: (n_images * max_faces, 5) int32 — the table of hpe_preprocess_rois. */
int hpe_face_rois(const int32_t *count, const double *boxes, int64_t n_images, int32_t max_faces,
                  int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h, double scale, int32_t *rois,
                  int32_t *n_rois, void *stream);

/* Tiled detection's merge (csrc/hpe_merge.hip): the detections hpe_detect made on the ROI images of a
 * frame-major table (hpe_preprocess_rois' `rois`, rows_per_frame = R rows per frame: rows f*R ..
 * f*R+R-1 belong to frame f, e.g. the whole look and its tiles) brought back into the coordinates of
 * one destination rectangle (dst_x0, dst_y0, dst_w, dst_h) in frame pixels, and the duplicates that
 * overlapping rows produce removed by one NMS per frame.  One workgroup per frame.
 * Inputs (device): count (n_frames*R), scores / boxes / keypoints / poses with M = max_faces_in slots per
 * ROI image, as the detector post-processing wrote them.
 * Candidates of frame f: (r, j) with r < R and j < min(max(count[f*R+r], 0), M), where row f*R+r passes
 * the validity rule of hpe_preprocess_rois and its frame field is f; any other row contributes nothing,
 * so (-1, 0, 0, 0, 0) is a legal filler.
 * Remap, for row (f, rx, ry, rw, rh), in float64 with every operation rounded on its own and the ints
 * converted exactly:
 *   X = ((rx + x * rw) - dst_x0) / dst_w,  Y = ((ry + y * rh) - dst_y0) / dst_h
 * for the two box corners and the six keypoints.  A candidate is dropped if a remapped box coordinate
 * is not finite or its score is NaN.  Order: score descending, then r*M + j ascending.  NMS: that of
 * the detector post-processing, the same code (csrc/hpe_boxes.h: greedy, IoU in fp32 on the fp32 casts
 * of the remapped boxes, corner order agnostic, zero area gives IoU 0, suppress iff IoU >
 * iou_threshold), at most max_faces_out kept.
 * Outputs (device, per frame max_faces_out slots, the first count_out[f] valid, in selection order; the
 * slots past it are not written): src_out int32 = r*M + j, scores_out / poses_out bit copies, boxes_out
 * f64 [x1,y1,x2,y2] and keypoints_out f64 [6][2] remapped.
 * Checked on the host (HPE_EINVAL): negative n_frames, non-positive rows_per_frame, max_faces_in,
 * max_faces_out, dst_w or dst_h; |dst_x0|, |dst_y0|, dst_w or dst_h above 2^24; rows_per_frame *
 * max_faces_in above HPE_MERGE_MAX_CAND (the workgroup's LDS: 64-bit sort keys, fp32 boxes and flags,
 * 112 KB of the 160 KB at the cap); n_frames beyond int32; null pointers when n_frames > 0.
 * n_frames == 0 is a no-op. */
#define HPE_MERGE_MAX_CAND 4096
int hpe_merge_rois(const int32_t *rois, int64_t n_frames, int32_t rows_per_frame, const int32_t *count,
                   const float *scores, const double *boxes, const double *keypoints, const float *poses,
                   int32_t max_faces_in, int32_t dst_x0, int32_t dst_y0, int32_t dst_w, int32_t dst_h,
                   float iou_threshold, int32_t max_faces_out, int32_t *count_out, int32_t *src_out,
                   float *scores_out, double *boxes_out, double *keypoints_out, float *poses_out,
                   void *stream);

/* Faces tracked across video frames and their box, keypoints and pose smoothed (csrc/hpe_track.hip):
 * association by IoU and, per track, the webcam loop's 19 EMA filters (blazeFaceDetectorH5.py:16-35,
 * :383-425: 4 box coordinates, 12 keypoint coordinates, 3 angles), which the reference indexes by a
 * face's position in the frame's result list.  One workgroup per stream; no host read.
 * Inputs (device): the detections of S = n_streams independent videos of T = n_frames consecutive
 * frames each, stream-major (frame t of stream s is image g = s*T + t), M = max_faces slots per image
 * as hpe_detect or hpe_merge_rois wrote them: count (S*T), boxes (S*T, M, 4) f64, keypoints
 * (S*T, M, 6, 2) f64, poses (S*T, M, 3) f32.  Scores are not an input: the slot order within a frame
 * (the NMS order) is the order the tracker takes the detections in.
 * State (device, caller-owned, carried from call to call), K = max_tracks slots per stream:
 *   state_i (S, 1 + 2K) int32, row s = [next_id, id_0 .. id_{K-1}, miss_0 .. miss_{K-1}]; an id below 0
 *           is a free slot
 *   state_d (S, K, HPE_TRACK_STATE_D) f64, per slot the smoothed box (4), keypoints (12) and pose (3),
 *           then the slot's last matched raw box (4)
 * hpe_track_reset writes next_id 0, every id -1, every miss 0 and every double 0.0.
 * Per stream, for t = 0 .. T-1 in order: c = min(max(count[g], 0), M); every live track (id >= 0)
 * starts the frame unmatched; for j = 0 .. c-1 in order, with m the detection's 19 values in float64
 * (the pose floats convert exactly):
 *   invalid  a box coordinate that is not finite: matches nothing, spawns nothing; track_out -1 and
 *            the outputs are bit copies of the inputs
 *   match    among the live tracks not yet matched in this frame, u = IoU of the detection's box and
 *            the track's last raw box, both cast to fp32, by the detector's formula (box_iou of
 *            csrc/hpe_boxes.h: corner order agnostic, zero area gives 0); a track qualifies iff
 *            u > match_iou; the largest u wins, on a tie the lowest slot.  A negative match_iou lets a
 *            zero overlap match: with one face that is the reference's position-only filter
 *   update   on a match, each of the 19 values: state = alpha * m + (1.0 - alpha) * state in float64,
 *            three separately rounded operations, 1.0 - alpha computed once (EMAFilter.update)
 *   spawn    when nothing matches, the lowest free slot if there is one: id = next_id, next_id =
 *            (next_id + 1) & 0x7fffffff, state = m (the first measurement passes through)
 *   neither  no match and no free slot: track_out -1, outputs bit copies of the inputs
 *   after a match or a spawn the slot is matched, its miss is 0 and its last raw box is the detection's
 *   outputs  track_out (S*T, M) int32 the id; boxes_out, keypoints_out the slot's smoothed doubles;
 *            poses_out (float) of the smoothed pose
 * After the frame's detections every live unmatched track gets miss += 1 and is freed (id = -1) if
 * miss > max_missed: reusable from the next frame on, never within the same frame.  A missed track's
 * values are held, not extrapolated.  Output slots at or past c are not written, and no coasting
 * tracks are emitted: the output has exactly the frame's detections.
 * The outputs must not overlap the inputs or the state.  Nothing in the state is used as an index, so
 * a corrupt state cannot cause an out-of-bounds access.
 * Checked on the host (HPE_EINVAL, before any device call): negative n_streams or n_frames, max_faces
 * < 1, max_tracks outside 1 .. HPE_TRACK_MAX_TRACKS, max_missed < 0, alpha outside (0, 1], a NaN
 * match_iou, n_streams * n_frames beyond int32, null pointers when n_streams * n_frames > 0 (for
 * hpe_track_reset: n_streams negative or beyond int32, max_tracks, null pointers when n_streams > 0).  n_streams * n_frames == 0 is a no-op that leaves the state
 * untouched. */
#define HPE_TRACK_MAX_TRACKS 64
#define HPE_TRACK_STATE_D 23   /* doubles per track slot */
int hpe_track_reset(int64_t n_streams, int32_t max_tracks, int32_t *state_i, double *state_d, void *stream);
int hpe_track(int64_t n_streams, int32_t n_frames, int32_t max_faces, const int32_t *count,
              const double *boxes, const double *keypoints, const float *poses, double alpha, float match_iou,
              int32_t max_missed, int32_t max_tracks, int32_t *state_i, double *state_d, int32_t *track_out,
              double *boxes_out, double *keypoints_out, float *poses_out, void *stream);

/* Detections and pose axes drawn into video frames on the device (csrc/hpe_draw.hip): the last stage of
 * the reference's webcam loop, drawDetections (blazeFaceDetectorH5.py:175-219 with drawAxis_simo :64-77
 * and EulerToMatrix :40-62).  Two stages: hpe_pose_prims turns detections into a table of integer
 * primitives (float64 rules), hpe_draw / hpe_draw_nv12 rasterise any such table (pure integer).
 *
 * The primitive table: device memory (n_frames, P, HPE_DRAW_PRIM_WORDS) int32, row = (kind, x0, y0, x1,
 * y1, size, colour, 0) in frame pixels; n_prims (n_frames) int32, of which min(max(n_prims[f], 0), P)
 * leading rows of frame f are live.  Coverage of the pixel at integer (x, y), all in integers:
 *   kind 1  rectangle outline: xa = min(x0, x1), xb = max(x0, x1), likewise ya, yb; th = size, h0 = th / 2,
 *           h1 = (th - 1) / 2; covered iff inside [xa - h0, xb + h0] x [ya - h0, yb + h0] and not inside
 *           the hole [xa + h1 + 1, xb - h1 - 1] x [ya + h1 + 1, yb - h1 - 1] (empty when its bounds cross)
 *   kind 2  filled disk of radius r = size >= 0 about (x0, y0): (x - x0)^2 + (y - y0)^2 <= r^2
 *   kind 3  thick segment P0 = (x0, y0) .. P1 = (x1, y1), th = size: d = P1 - P0, L2 = d.d, v = p - P0,
 *           t = v.d;  t <= 0: 4 |v|^2 <= th^2;  t >= L2: 4 |p - P1|^2 <= th^2;  else 4 (vx dy - vy dx)^2
 *           <= th^2 L2 in int64: the pixel centres within th / 2 of the segment; zero length is a dot
 * A row is valid iff its kind is 1, 2 or 3, every coordinate has |c| <= HPE_DRAW_MAX_DIM, 1 <= size <=
 * HPE_DRAW_MAX_SIZE (0 <= size for kind 2) and 0 <= colour < n_colours; any other row draws nothing, so
 * a row of zeros is the legal filler.  With these bounds the largest term, 4 cross^2, is below 2^61.
 * Nothing read from the table is used as an index before it is checked.  A pixel takes the colour of
 * the highest-indexed valid live row that covers it (later rows paint over earlier ones); a pixel no
 * row covers is not written at all.
 * colours: device (n_colours, 4) uint8, byte 3 ignored.
 * hpe_draw: frames of h x w pixels of 3 bytes, rows row_stride and frames frame_stride bytes apart;
 * bytes 0..2 of the colour go to the pixel's three bytes (BGR or RGB is the caller's affair).
 * hpe_draw_nv12: the plane layout of hpe_preprocess_nv12.  Byte 0 goes to the luma of every covered
 * pixel; for each chroma pair uv[y >> 1][x >> 1], bytes 1 and 2 of the highest-indexed winning row over
 * the block's four pixels are written as (U, V) if any of the four is covered, so thin lines keep
 * their colour.  No colour conversion: the caller supplies (Y, U, V) bytes.
 * No byte outside [row start, row start + 3 w) of a frame row (+ w for the NV12 planes) is written.
 * Checked on the host (HPE_EINVAL, before any device call): negative n_frames or P, h or w outside 1 ..
 * HPE_DRAW_MAX_DIM (or odd, NV12), row strides below the row's bytes, negative frame strides, n_colours
 * outside 1..256, n_frames beyond int32, n_frames * P * HPE_DRAW_PRIM_WORDS or a frame's last byte offset
 * beyond int64, null pointers when there is work.  n_frames == 0 or P == 0 is a no-op.
 *
 * hpe_pose_prims: count (n_images), boxes (n_images, max_faces, 4) f64 [x1,y1,x2,y2], keypoints
 * (n_images, max_faces, 6, 2) f64, poses (n_images, max_faces, 3) f32 (yaw, pitch, roll), as hpe_detect,
 * hpe_merge_rois or hpe_track wrote them, normalised to the source rectangle (src_x0, src_y0, src_w,
 * src_h) in frame pixels as for hpe_face_rois -> prims (n_images, P = max_faces * HPE_DRAW_FACE_PRIMS,
 * 8) and n_prims[i] = 11 c, c = min(max(count[i], 0), max_faces).  Detection j owns rows 11 j .. 11 j +
 * 10: box, keypoints 0..5, axis X, axis Y, axis Z, with the colour indices 0, 1, 2 / 3 / 4, then one
 * reserved row that is written as zeros (ten primitives in a stride of 11).  A kind-0 row is always
 * written as eight zeros.  Rows at or past 11 c are not written.  In float64, every operation rounded on its own, floats converted exactly:
 *   pix(v, s, o) = o + (int) clamp(trunc(s * v), -2^30, 2^30), then clamped to +-HPE_DRAW_MAX_DIM
 *   box      x1 = pix(bx1, src_w, src_x0), y1 = pix(by1, src_h, src_y0), likewise x2, y2 (the reference's
 *            (img_width * box[0]).astype(int), truncation toward zero): row (1, x1, y1, x2, y2, box_th, 0, 0)
 *   keypoint (kx, ky) = (pix(., src_w, src_x0), pix(., src_h, src_y0)): row (2, kx, ky, kx, ky, kp_radius, 1, 0)
 *   axes     tdx = (x1 + x2) / 2.0, tdy = (y1 + y2) / 2.0, cx = trunc(tdx), cy = trunc(tdy),
 *            size = trunc(min(x2 - x1, y2 - y1) / 2.0) (negative for flipped corners, used as it is);
 *            r = (-roll) / 180 * pi, y = (-yaw) / 180 * pi, p = (-pitch) / 180 * pi (pi the nearest double);
 *            m00 = cy cr, m10 = (sp sy) cr + cp sr, m01 = -(cy sr), m11 = -((sp sy) sr) + cp cr, m02 = sy,
 *            m12 = -(sp cy);  X ends at (trunc(m00 size + tdx), trunc(-(m10 size) + tdy)), Y at
 *            (trunc(-(m01 size) + tdx), trunc(m11 size + tdy)), Z at (trunc(m02 size + tdx),
 *            trunc(-(m12 size) + tdy)), each clamped to +-HPE_DRAW_MAX_DIM: rows (3, cx, cy, ex, ey,
 *            axis_th_*, 2 | 3 | 4, 0)
 * A box_th of 0, a negative kp_radius or an axis_th_* of 0 writes kind 0 for those rows.  A non-finite
 * box coordinate makes all 11 rows kind 0, a non-finite keypoint coordinate its own row, a non-finite
 * angle the three axis rows.
 * Two facts about this rule.  (1) The closed form is Rx Ry Rz of EulerToMatrix(-roll, -yaw, -pitch) with
 * the exact zero and one terms dropped; its entries differ from np.matmul's by a rounding for about half
 * of random poses (CPU, 20,000 random poses and boxes on a 1920 x 1080 frame: 9,574 poses differ in some
 * entry, zero truncated endpoints differ).  (2) The device's float64 sin / cos may differ from the
 * host's by an ulp, so an endpoint whose untruncated value lies within that distance of an integer can
 * land one pixel away: parity with the reference holds for the integer table except for such values.
 * Parity with OpenCV's own line, circle and rectangle rasterisation is unpinned: the coverage rules
 * above are this project's.
 * Out of scope: the text the reference puts on the frame (score, Yaw / Pitch / Roll, FPS; it needs
 * OpenCV's Hershey font data), anti-aliasing, alpha blending, and the unused draw_axis method (:142-172).
 * Checked on the host (HPE_EINVAL): negative n_images, max_faces < 1, src_w or src_h outside 1 .. 2^24,
 * |src_x0| or |src_y0| above 2^24, thicknesses outside 0 .. HPE_DRAW_MAX_SIZE, kp_radius outside -1 ..
 * HPE_DRAW_MAX_SIZE, n_images * max_faces * 11 beyond int32, null pointers when n_images > 0.
 * n_images == 0 is a no-op. */
#define HPE_DRAW_PRIM_WORDS 8
#define HPE_DRAW_FACE_PRIMS 11
#define HPE_DRAW_MAX_DIM 8192
#define HPE_DRAW_MAX_SIZE 64
int hpe_draw(uint8_t *frames, int64_t n_frames, int32_t h, int32_t w, int64_t row_stride, int64_t frame_stride,
             const int32_t *prims, const int32_t *n_prims, int32_t P, const uint8_t *colours, int32_t n_colours,
             void *stream);
int hpe_draw_nv12(uint8_t *y, uint8_t *uv, int64_t n_frames, int32_t h, int32_t w, int64_t y_row_stride,
                  int64_t y_frame_stride, int64_t uv_row_stride, int64_t uv_frame_stride, const int32_t *prims,
                  const int32_t *n_prims, int32_t P, const uint8_t *colours, int32_t n_colours, void *stream);
int hpe_pose_prims(const int32_t *count, const double *boxes, const double *keypoints, const float *poses,
                   int64_t n_images, int32_t max_faces, int32_t src_x0, int32_t src_y0, int32_t src_w,
                   int32_t src_h, int32_t box_th, int32_t kp_radius, int32_t axis_th_x, int32_t axis_th_y,
                   int32_t axis_th_z, int32_t *prims, int32_t *n_prims, void *stream);

const char *hpe_last_error(void);

/* Build stamp: "src=<sha256/16 of the library's sources> git=<commit>[-dirty]" (csrc/Makefile).  The
 * Python binding recomputes the source hash from the tree it runs in and refuses a library built
 * from other sources, so a run's kernels are provably the checkout's. */
const char *hpe_build_id(void);

/* Dominant-kernel timing (bench.py's roofline): hpe_kernel_timing(capacity) turns timing on for
 * the next `capacity` program launches (0 turns it off): hpe_forward / hpe_train_step record a HIP
 * event pair on their stream around the launch's dominant kernel only (the fp16-split kernel, not
 * its early-exit exact twin, nor hpe_reduce).  hpe_kernel_times waits for the recorded pairs and
 * writes their elapsed milliseconds to ms[0 .. n); returns n (<= max): the leading run of pairs
 * whose launch has finished recording (a launch another host thread has not returned from yet
 * ends the run). */
int hpe_kernel_timing(int32_t capacity);
int hpe_kernel_times(float *ms, int32_t max);

/* Diagnostics (race screens; synchronises the device, so not for the hot path): out[0] = the
 * program's last launch epoch, out[1 .. 16] its guard ring (word e % 16 holds e when launch e's
 * fp16-split kernel flagged a non-finite value and its exact-fp32 twin recomputed the step),
 * out[17 .. 32] reserved per ring slot for which check fired (no current kernel writes them: 0). */
int hpe_guard_peek(const hpe_program *prog, int32_t *out);

/* Precision of the regressor GEMMs (process-wide; returns the previous setting).  Default 0: the
 * fused kernels run their fp32 GEMMs as three fp16 MFMAs per product (hi/lo split, fp32
 * accumulate, ~2^-22 relative per product; csrc/hpe_common.h mfma3), and a launch whose split
 * overflows fp16 (|value| >= 65504) is recomputed by the exact-fp32 kernel automatically.
 * 1: exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) only.  The environment variable HPE_EXACT_FP32=1
 * sets the initial value. */
int hpe_set_exact_fp32(int on);

/* Diagnostics: out[i] = the fused regressor kernels' layer-1 activation `act` (ACT_* of
 * csrc/hpe_prog.h) of z[i], as they evaluate it (csrc/hpe_dev.h act1_f).  fast = 1: the fp16-split
 * kernels' form (tanh: fast_tanh5, absolute error <= 2^-22); fast = 0: the exact-fp32 kernels'
 * (tanh: tanhf).  Device pointers, n floats; asynchronous on `stream`. */
int hpe_act_probe(int32_t act, int32_t fast, const float *z, float *out, int64_t n, void *stream);

/* Diagnostics: the DPP row-broadcast operand of the fused regressor kernel (csrc/hpe_dev.h
 * fmac_bcast / mul_bcast) as one 64-lane wave evaluates it.  t, x, acc: 64 floats each; out: [2][16][64]
 * floats, out[0][N][lane] = fma(t[(lane & ~15) + N], x[lane], acc[lane]) and out[1][N][lane] =
 * t[(lane & ~15) + N] * x[lane].  Device pointers; asynchronous on `stream`. */
int hpe_bcast_probe(const float *t, const float *x, const float *acc, float *out, void *stream);

/* Attention heads on H x W > 1 feature maps: the two stages that are not
 * row-local.  Replace the TF kernels behind GlobalAveragePooling2D -> Dense -> Dense -> Multiply
 * (Model-88/attention_model.py:34-38, :78-82) and behind MultiHeadAttention's softmax(QK^T)V over
 * the H*W tokens of each image (attention_model.py:52-55).
 *
 * hpe_se_gate: x, xg [n_images * P][C] rows; w1 [C][U] (+ b1 [U], may be NULL), w2 [U][C]
 * (+ b2 [C]); act1 / act2 activation codes of csrc/hpe_prog.h (ACT_*).  xg = x * s[image].
 * hpe_mha: per row, in = [pass-through C | q H*D (pre-scaled by 1/sqrt(D)) | k H*D | v H*D]
 * (stride ld_in floats); out = [pass-through C | o H*D] (stride ld_out).  1 <= D <= 64. */
int hpe_se_gate(const float *x, float *xg, int64_t n_images, int32_t P, int32_t C, const float *w1,
                const float *b1, int32_t U, int32_t act1, const float *w2, const float *b2,
                int32_t act2, void *stream);
/* y[i][c] = mean over the P rows of image i of x (a terminal GlobalAveragePooling2D), C <= 256. */
int hpe_seg_mean(const float *x, float *y, int64_t n_images, int32_t P, int32_t C, void *stream);
int hpe_mha(const float *in, int32_t ld_in, int32_t C, float *out, int32_t ld_out,
            int64_t n_images, int32_t P, int32_t H, int32_t D, void *stream);
/* hpe_mha_xg: the same attention with the pass-through columns read from their own rows: qkv =
 * [q H*D (pre-scaled) | k H*D | v H*D] (stride ld_qkv), xg [n_images * P][C] contiguous; out =
 * [xg | o H*D] (stride ld_out).  The projection that feeds it then computes only q | k | v (no
 * identity block for xg: 2 * C * C fewer FLOPs and C fewer stored floats per row). */
int hpe_mha_xg(const float *qkv, int32_t ld_qkv, const float *xg, int32_t C, float *out, int32_t ld_out,
               int64_t n_images, int32_t P, int32_t H, int32_t D, void *stream);

/* hpe_attn_tail: the row-local tail of se_transformer_regr_head after the attention core
 * (Model-88/attention_model.py:56-72: residual Add of the attention output, LayerNorm, feed-forward
 * Dense -> Dense, residual Add, LayerNorm, 1x1 conv hidden -> 1x1 conv 3) in one kernel: reads xg
 * [n_rows][ld_xg >= C] and the attention output o [n_rows][ld_o >= H*D] (hpe_mha_xg with C = 0),
 * writes y [n_rows][3].  desc: 20 host int32 words (C, H*D, ff_dim, hidden, activations, the two
 * LayerNorm epsilons as float bits, the parameter buffer's size and vector offsets); w: the device
 * parameter buffer hpe/spatial.py:_attn_tail prepares (weights in MFMA operand order, padded
 * vectors; the layout is written out at the top of csrc/hpe_tail.hip).
 * hpe_attn_tail_supported(desc), host only: 1 when a kernel is compiled for these widths (C in
 * {84, 88, 92, 96}; H*D a multiple of 4 in 1, 2, 4 or 8 blocks of 16; (ff_dim, hidden) in (4, 8),
 * (4, 4) or (2, 8) blocks of 16) and every other word is in range: the three activation codes in
 * 0..9, both epsilons finite and positive, the buffer size a multiple of 4 floats that holds the
 * weight tiles and the nine padded vectors and fits the 160 KB LDS, each vector offset a multiple
 * of 4, at or after the end of the weight tiles, its padded vector inside the buffer.
 * hpe_attn_tail returns HPE_EINVAL for a descriptor that hpe_attn_tail_supported refuses, for a
 * null argument and for strides below the widths or not multiples of 4 (also when n_rows = 0). */
int hpe_attn_tail_supported(const int32_t *desc);
int hpe_attn_tail(const float *xg, int32_t ld_xg, const float *o, int32_t ld_o, int64_t n_rows,
                  const int32_t *desc, const float *w, float *y, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HPE_H */
