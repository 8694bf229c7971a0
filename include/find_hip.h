/* find_hip.h -- C ABI of libfind_hip.so: the MI355X (gfx950) hot path of FIND.
 *
 * The reference (OllieBoyne/FIND) is pure Python; its "FFI" for this path is the PyTorch / PyTorch3D
 * operator surface.  Each entry point below names the reference call site(s) it replaces
 * (paths relative to the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - All pointers are DEVICE pointers owned by the caller (PyTorch-allocated); the library allocates no device
 *     memory.  Scratch is passed in as `ws` + `ws_bytes`; query sizes with *_ws_bytes().  The only persistent
 *     state is the opaque per-device context of find_ctx_create (internal HIP streams / events of the MLP entry
 *     points, per-kernel launch attributes, tuning knobs): nothing is process-global.
 *   - All tensors are contiguous row-major fp32 unless stated; indices are int32 or int64 as stated.
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and performs no device synchronisation.
 *   - Return value: 0 on success, negative FIND_E* code otherwise; find_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI.
 *   - Threading: a context is used by one thread at a time (the thread that owns the autograd graph); one
 *     context per device and process under data parallelism.  Entry points without a context are re-entrant.
 */
#ifndef FIND_HIP_H
#define FIND_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIND_ABI_VERSION 3

#define FIND_OK 0
#define FIND_EINVAL (-1)   /* bad argument / unsupported configuration */
#define FIND_EWORKSPACE (-2) /* workspace too small */
#define FIND_ELAUNCH (-3)  /* HIP launch or runtime error */

#define FIND_MAX_LAYERS 8

int find_abi_version(void);
const char* find_last_error(void);
/* Name of the code-object architecture the library was built for ("gfx950"). */
const char* find_build_arch(void);

/* ------------------------------------------------------------------------------------------------
 * Context: per-device state of the MLP entry points -- the internal side streams and the event pool
 * that find_mlp_fwd / find_mlp_bwd fork work onto (always joined back into the caller's stream before the call
 * returns, also on an error return), the device's CU count and LDS size, per-kernel launch attributes and the
 * tuning knobs.  The reference has no counterpart (its operators keep their state inside PyTorch / PyTorch3D).
 * find_ctx_create makes `device` current for the calling thread while it builds the context and restores the
 * previous device.  A context must be destroyed only after the work launched through it has completed.
 * ---------------------------------------------------------------------------------------------- */
typedef struct find_ctx find_ctx;
int find_ctx_create(int device, find_ctx** out);
int find_ctx_destroy(find_ctx* ctx);
/* Which of the context's four side streams share a hardware queue with `caller_stream` or with each other (HIP maps streams
 * onto GPU_MAX_HW_QUEUES queues in creation order; two streams on one queue run in order).  groups[0] = 0 is the caller's stream,
 * groups[1 + k] side stream k; equal numbers = same queue.  Synchronises the streams it probes (~0.3 ms per probe). */
int find_ctx_stream_groups(find_ctx* ctx, void* caller_stream, int32_t* groups /* [5] */);
/* A second stream for the CALLER's own concurrent work (find_amd.model_with_loss: the Chamfer term beside the texture term's MLP pass, the
 * GT render beside the predicted one) that fits the context's stream layout: *index = the first of the n candidate streams that runs beside
 * `caller_stream` AND shares the hardware queue of side stream `role` (0 = Q, 1 = T1, 2 = T2, 3 = R), -1 if none does.  With four hardware
 * queues a fifth stream always shares one with somebody, and its work runs in order behind whatever that stream was given first: on T1's
 * queue the Chamfer backward waited ~0.2 ms behind the texture pass's weight gradients; Q is idle until the main pass's backward.
 * Binds the side streams first if that has not happened yet; synchronises the streams it probes. */
int find_ctx_stream_beside(find_ctx* ctx, void* caller_stream, void* const* candidates, int32_t n, int32_t role, int32_t* index);
/* Knobs (see the list at find_ctx_set below); find_ctx_get reads the current value, plus the read-only
 * "num_cus", "lds_bytes", "device", "events_per_call_max" (largest event count one MLP call has used so far). */
int find_ctx_set(find_ctx* ctx, const char* key, int64_t value);
int find_ctx_get(const find_ctx* ctx, const char* key, int64_t* value);

/* ------------------------------------------------------------------------------------------------
 * MLP: Fourier positional encoding + trunk + displacement head + colour head.
 * Replaces NeuralDisplacementField.forward  (src/model/model.py:393-453)
 *      and FourierFeatureTransform.forward  (src/utils/fourier_feature_transform.py:28-55),
 * plus their autograd backward (reached from src/train/trainer.py:121).
 *
 * Weight pointers use the reference state_dict tensors directly:
 *   trunk_w[i] = base.{2i}.weight   (width, in_i) ; in_0 = in_dim + 2*pe_size (or in_dim), else width
 *   disp_w[0]  = mlp_disp.0.weight  (width, width + lat_disp)  ... disp_w[n_disp] = final (3, width)
 *   col_w[0]   = mlp_col.0.weight   (width, width + lat_col)   ... col_w[n_col]   = final (3, width)
 * Only width == 256 and in_dim == 3 are supported (the reference's fixed setting, model.py:207).
 * ---------------------------------------------------------------------------------------------- */
typedef struct find_mlp_params {
	int32_t width;      /* hidden width (256) */
	int32_t in_dim;     /* 3 */
	int32_t pe_size;    /* Fourier mapping size (256); 0 = positional encoding disabled */
	int32_t n_trunk;    /* number of trunk Linear layers (depth + 1) */
	int32_t n_disp;     /* hidden Linear layers in the displacement head (dispdepth); final 3-wide layer is extra */
	int32_t n_col;      /* hidden Linear layers in the colour head (coldepth) */
	int32_t lat_disp;   /* latent columns appended to the disp-head input ([shapevec, posevec]) */
	int32_t lat_col;    /* latent columns appended to the col-head input (texvec) */
	const float* B;     /* (in_dim, pe_size) Fourier matrix (_B; not in the state_dict) */
	const float* trunk_w[FIND_MAX_LAYERS];
	const float* trunk_b[FIND_MAX_LAYERS];
	const float* disp_w[FIND_MAX_LAYERS];
	const float* disp_b[FIND_MAX_LAYERS];
	const float* col_w[FIND_MAX_LAYERS];
	const float* col_b[FIND_MAX_LAYERS];
	const float* avg_col; /* (3) added to the colour output when non-NULL (use_avg_colour, model.py:446-447) */
	int32_t precision;    /* arithmetic of the 256 -> 256 layers, per call (two models in one process may differ):
	                       *   0 = the context's "mlp_f16" knob;
	                       *   1 = fp32 MFMA (v_mfma_f32_32x32x2_f32), the reference's arithmetic;
	                       *   2 = fp16 MFMA operands (rounded to 11 bits) with fp32 accumulation: opt-in, BASELINE.json configs[4], no reference
	                       *       counterpart, ~1e-3 relative per layer;
	                       *   3 = bf16x3: every fp32 operand split EXACTLY into three bf16 pieces, the six products of relative size >= 2^-18
	                       *       on the bf16 matrix pipe, fp32 accumulation -- what is left out is <= 2^-26 of a product (a quarter of one fp32
	                       *       rounding), so results are as close to the float64 product as mode 1's (tests/test_gpu_mlp_bf16x3.py) at
	                       *       6/16 of its matrix-pipe time; the default of the Python surface (find_amd.functional.set_mlp_precision).
	                       *       Launches of >= "gemm6_min_units" 32-row units (gemm7_kernel / dw6_kernel) and the fused layer chains of small calls
	                       *       (fused6_kernel); what lies in between, the grouped weight gradients of small calls and the Fourier layer's run
	                       *       mode 1's kernels */
} find_mlp_params;

/* Gradient outputs, same shapes as the corresponding weights; every buffer given is OVERWRITTEN.
 * Which buffers may be NULL (what autograd's needs_input_grad asks for on the FIND path):
 *   - a head whose upstream gradient (d_disp / d_col) is NULL contributes nothing: its weight-gradient and latent-gradient pointers may be
 *     NULL (nothing is written); given, they receive exact zeros;
 *   - ALL weight-gradient pointers NULL = frozen network (requires_grad False on every weight; stage 3 of src/train/train.py:217-224 steps
 *     Adam(latent_params) only): the call stops at the heads' first layers and writes lat_disp / lat_col alone;
 *   - anything in between is refused (FIND_EINVAL). */
typedef struct find_mlp_grads {
	float* trunk_w[FIND_MAX_LAYERS];
	float* trunk_b[FIND_MAX_LAYERS];
	float* disp_w[FIND_MAX_LAYERS];
	float* disp_b[FIND_MAX_LAYERS];
	float* col_w[FIND_MAX_LAYERS];
	float* col_b[FIND_MAX_LAYERS];
	float* lat_disp; /* (n_feet, lat_disp) or NULL */
	float* lat_col;  /* (n_feet, lat_col) or NULL */
} find_mlp_grads;

/* Bytes of workspace find_mlp_fwd needs.  `pos_batch` is 1 (positions shared by every foot: the template,
 * model.py:404-406 / pytorch3d_tools.py:7-16) or n_feet.  With save_for_bwd the same buffer must be passed,
 * untouched, to find_mlp_bwd. */
int64_t find_mlp_ws_bytes(const find_mlp_params* p, int64_t pos_batch, int64_t n_feet, int64_t n_pts, int save_for_bwd);

/* pos (pos_batch, n_pts, 3); lat_disp (n_feet, lat_disp) or NULL; lat_col (n_feet, lat_col) or NULL (NULL when params say the head takes no
 * latents -- or when the call does not evaluate that head: disp / col NULL here, d_disp / d_col NULL in find_mlp_bwd);
 * out: disp (n_feet, n_pts, 3) = 0.1*tanh(.), col (n_feet, n_pts, 3) = 0.5*(1+tanh(.)) [+avg_col]. */
int find_mlp_fwd(find_ctx* ctx, const find_mlp_params* p, const float* pos, int64_t pos_batch, int64_t n_feet, int64_t n_pts,
				 const float* lat_disp, const float* lat_col, float* disp, float* col,
				 void* ws, int64_t ws_bytes, int save_for_bwd, void* stream);

/* Backward of find_mlp_fwd.  d_disp, d_col: (n_feet, n_pts, 3) upstream gradients (either may be NULL = zero).
 * `ws` is the forward workspace (save_for_bwd=1); `scratch` is extra space of find_mlp_bwd_scratch_bytes(). */
int64_t find_mlp_bwd_scratch_bytes(const find_mlp_params* p, int64_t pos_batch, int64_t n_feet, int64_t n_pts);
int find_mlp_bwd(find_ctx* ctx, const find_mlp_params* p, const float* pos, int64_t pos_batch, int64_t n_feet, int64_t n_pts,
				 const float* lat_disp, const float* lat_col, const float* d_disp, const float* d_col,
				 const void* ws, int64_t ws_bytes, void* scratch, int64_t scratch_bytes,
				 const find_mlp_grads* grads, void* stream);

/* Make `stream` wait for weight-gradient work a find_mlp_bwd left running under the "defer_join" knob.  Returns 1 if there was any,
 * 0 if not, a negative code on error. */
int find_ctx_join(find_ctx* ctx, void* stream);

/* One hidden layer  y = relu(x @ w^T + b)  with x (n_feet*n_pts, 256), w (256,256), b (256): the dominant kernel
 * of the path (nn.Linear + nn.ReLU pairs built at src/model/model.py:255-257, 353-356, 362-365).  Exposed so the
 * kernel can be timed and checked in isolation; find_mlp_fwd launches the same kernel.  w must be 16-byte aligned. */
int find_linear_relu_fwd(find_ctx* ctx, const float* x, const float* w, const float* b, int64_t n_feet, int64_t n_pts, float* y, void* stream);

/* Weight gradient of one 256 -> 256 layer:  dw[n][k] = sum_rows dz[row][n] * x[row][k]  (256 x 256, row-major) and, when db is not
 * NULL, db[n] = sum_rows dz[row][n], over rows = (foot, point) as above -- what autograd computes for the `weight` / `bias` of an
 * nn.Linear (src/model/model.py:255-257, 353-356, 362-365) from the layer's input x and the gradient dz of its output.  Exposed, like
 * find_linear_relu_fwd, so that the kernel (dw2_kernel; dw3_kernel in the fp16 mode) can be timed and checked in isolation;
 * find_mlp_bwd launches the same kernels.  `scratch` holds the partial tiles (find_linear_wgrad_scratch_bytes). */
int64_t find_linear_wgrad_scratch_bytes(int64_t n_feet);
int find_linear_wgrad(find_ctx* ctx, const float* dz, const float* x, int64_t n_feet, int64_t n_pts, float* dw, float* db,
					  void* scratch, int64_t scratch_bytes, void* stream);

/* Tuning knobs of a context (no reference counterpart).  Results do not depend on any knob except "mlp_f16" (the precision, below) and the
 * summation order of "reduce_exclusive" = 2 and "footsum_fold".
 *   "gemm4_min_units" launches with at least this many 32-row x 128-column units use the W-resident kernel on column halves (default 1024)
 *   "gemm4_small"     ... and launches of at least this many 32-row units use it on column quarters (default 64; 0 = never);
 *                     anything smaller, and the two-segment trunk-output gradient, runs on the LDS-DMA ring kernel (gemm3)
 *   "dw2_min_cps"     weight-gradient kernels: shortest row run (16-row chunks) per workgroup
 *   "bwd_streams"     0 = backward on the caller's stream only, 1 = weight gradients on the context's side streams (default)
 *   "fwd_streams"     1 = the forward runs the colour head on a side stream beside the displacement head (default), 0 = one stream
 *   "reduce_stream"   1 = slab reduces of the large head layers on their own stream, two alternating slab sets; default 0 (behind their
 *                     weight-gradient launch: measured 0.6 - 0.9 % faster since the weight gradients use no LDS)
 *   "bind_streams"    1 (default) = the first call that forks picks the four side streams among a dozen candidates by probing which
 *                     hardware queue each one shares (see find_ctx_stream_groups); 0 = keep them as created
 *   "defer_join"      1 = the NEXT find_mlp_bwd, if it is a small per-foot call (the fused-chain path: the texture pass of a train_3d step),
 *                     returns with its weight-gradient kernels still running on the context's side streams; its latent gradients are
 *                     complete on the caller's stream.  The weight-gradient buffers, `scratch` and `ws` of that call must stay untouched
 *                     until find_ctx_join() -- or the end of a later find_mlp_bwd on this context -- has made the reader's stream wait.
 *                     The knob resets itself with the call.  Ignored under stream capture and for the large-call paths.
 *   "mlp_f16"         default precision for calls whose find_mlp_params.precision is 0, and the precision of find_linear_relu_fwd /
 *                     find_linear_wgrad: 1 = the K = 256 Linear layers (forward, dX and dW) run on the fp16 matrix pipe: operands rounded to
 *                     fp16, fp32 accumulation, fp32 tensors (gemm5_kernel, dw3_kernel; BASELINE.json configs[4]).  Default 0: this knob DOES
 *                     change results (~1e-3 relative per layer); the Python surface is find_amd.functional.set_mlp_precision
 *                     2 = bf16x3 (find_mlp_params.precision 3: fp32-faithful, gemm7_kernel / dw6_kernel)
 *   "gemm5_min_units" in fp16 mode, launches of fewer 32-row units than this stay on the fp32 kernels (default 1024)
 *   "act16"           in fp16 mode only: 1 (default) = the heads' hidden activations and their gradients are STORED as fp16 inside the
 *                     call's workspace / scratch when a template is shared by more than one foot and the heads have >= "gemm5_min_units"
 *                     units (the matrix pipe rounds these values to fp16 anyway; BASELINE.json configs[4] is bound by their bytes); 0 = fp32
 *                     storage.  (A find_mlp_bwd follows what the find_mlp_fwd of its workspace did, also if a knob was turned in between.)
 *   "bcast_fold"      1 (default) = with a template shared by several feet, the output relu(P[v] + bias[foot]) of a head's broadcast first layer is
 *                     not stored: the second layer's forward GEMM, the ReLU mask of its dX GEMM and the x operand of its weight gradient form it
 *                     from the V x 256 product P and the bias rows (bf16x3: gemm7_kernel / dw6v_kernel; fp16 mode inside "act16": gemm5_kernel /
 *                     dw3_h16v_kernel).  Bit-identical to 0 (bias_relu_bcast_kernel materialises it).  The backward follows its forward's note
 *   "footsum_fold"    1 (default; bf16x3, needs "bcast_fold") = the dX GEMM that produces that layer's gradient forms the two sums the backward reads
 *                     of it -- over the feet, and per foot over the rows -- in its epilogue and stores no gradient tensor (gemm7_kernel<.., FSUM>);
 *                     0 = footsum_kernel over the stored tensor.  Same sums in another order (~2e-7 of a gradient's largest entry), deterministic
 *   "gemm6_min_units" the same threshold for the bf16x3 kernels (default 1024)
 *   "fused_max_units" calls of at most this many 32-row units (0..1024, default 512) run whole layer chains -- the trunk, trunk + heads of a
 *                     per-foot pass, their dX chains -- in one launch of fused_chain_kernel, and the weight gradients of a chain as one grouped
 *                     launch + one grouped reduce; 0 = one launch per layer at every size
 *   "fused6"          bf16x3 calls run their chains on fused6_kernel (weights pre-split by split_w_kernel into the call's workspace; default 1);
 *                     0 = fused_chain_kernel (fp32 MFMA), as the other precisions
 *   "dw_lds_free"     kernel of the 256 x 256 weight gradients: 1 = dw4_kernel (operands straight from global memory, no LDS, <= 256
 *                     registers; default), 0 = dw2_kernel (LDS-DMA ring, the whole register file of its SIMDs claimed)
 *   "lds_exclusive"   1 = the LDS-DMA ring kernels reserve their CU's whole LDS: round 1's containment of that fault, which turned out
 *                     to be about registers; default 0
 *   "reduce_exclusive" the stress test's hook for that fault (tests/test_gpu_mlp.py): 1 = the slab-reduce kernels reserve their CU's whole LDS;
 *                     2 = they use no LDS and are slow, so that they stay resident beside later weight-gradient kernels; default 0
 *   "ablate"          switches that leave results unchanged (the tests compare them): 16 no s_setprio in gemm4 (gemm7 always sets its wave priorities), 32 every column block in
 *                     the Fourier layer's weight gradient, 128 fused chains always on 32-row tiles.  Any other bit is refused here.
 * The Python binding applies FIND_TUNING="key=value,..." from the environment to every context it creates. */

/* Process-wide switches of the rasteriser and of find_chamfer_fwd's neighbour search, all with unchanged results (tests/test_gpu_render.py,
 * tests/test_gpu_geom.py compare them): 8 no early exit of finished pixels / tiles, 16 tile lists left in face order (no depth-slab sort),
 * 256 a list pool of 512 entries per image (tiles without room scan the faces themselves); Chamfer: 512 all pairs at every size, 1024 the
 * uniform grid from 64 points per cloud on, 16384 the balanced tiles from 64 points per cloud on (up to 8192), 32768 never the tiles
 * (geom.hip; tests/test_gpu_chamfer_tiles.py); 2048 / 4096 the band / the candidate-list rasteriser at every image size (default: the
 * band kernel from 384^2 pixels on, csrc/render_band.h -- the two agree in everything but the last bits of the alpha products); 8192
 * find_point_face_fwd, find_winding_fwd and find_ray_fwd never split a mesh's faces over several workgroups (surface.hip, winding.hip,
 * raycast.hip; tests/test_gpu_surface.py, tests/test_gpu_inside.py, tests/test_gpu_rays.py); the field 0x70000, when
 * k = (bits >> 16) & 7 is not 0: find_chamfer_surface_bwd cuts every foot into 1 << (k - 1) slices, whatever its size rule says
 * (tests/test_gpu_surface_chamfer_bwd.py).  Any other bit is refused (FIND_EINVAL). */
int find_render_switches(int64_t bits);
/* ------------------------------------------------------------------------------------------------
 * Latent-table lookup.  Replaces LatentVector.__getitem__ with a tensor of indices (src/model/model.py:131-152;
 * call sites src/model/model.py:360-372 get_meshes_from_batch) and the index_put its autograd runs backward.
 * table (n_rows, dim) fp32; idx (n_idx) int64, negative values count from the end; an out-of-range index yields a
 * NaN row (no host synchronisation here).  The backward owns every table element by one thread and sums the
 * matching rows in index order: deterministic with duplicates, untouched rows come out zero.
 * ---------------------------------------------------------------------------------------------- */
int find_latent_gather_fwd(const float* table, int64_t n_rows, int64_t dim, const int64_t* idx, int64_t n_idx, float* out, void* stream);
int find_latent_gather_bwd(const float* d_out, const int64_t* idx, int64_t n_idx, int64_t n_rows, int64_t dim, float* d_table, void* stream);
/* The same for up to 8 tables in one launch each way -- trainer.sample_latent_vectors (src/train/trainer.py:29-46) looks up the shape,
 * pose, texture and registration rows of a batch, one LatentVector.__getitem__ each.  tables / idx / outs (and n_rows, dims) are HOST
 * arrays of n_tables entries; every lookup has n_idx indices.  Backward: d_outs[t] may be NULL (no gradient arrived: d_tables[t] = 0). */
int find_latent_gather_many_fwd(int64_t n_tables, const float* const* tables, const int64_t* n_rows, const int64_t* dims,
								const int64_t* const* idx, int64_t n_idx, float* const* outs, void* stream);
int find_latent_gather_many_bwd(int64_t n_tables, const float* const* d_outs, const int64_t* n_rows, const int64_t* dims,
								const int64_t* const* idx, int64_t n_idx, float* const* d_tables, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Loss weighting: scaled[i] = *terms[i] * weights[i], *total = sum_i scaled[i] in term order (ModelWithLoss.forward,
 * src/model/model.py:1157-1163: losses[k] = raw * opts.weight_k, loss = sum).  terms: HOST array of 1 <= n <= 16 device scalars; weights:
 * host floats; scaled (n) and total: device.  Backward: d_terms[i] = weights[i] * (*g_total + g_scaled[i]); either upstream may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int find_weighted_terms_fwd(int64_t n, const float* const* terms, const float* weights, float* scaled, float* total, void* stream);
int find_weighted_terms_bwd(int64_t n, const float* weights, const float* g_total, const float* g_scaled, float* d_terms, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Contrastive pose loss.  Replaces ContrastiveLoss.forward / crit (src/model/losses.py:305-333; call site ModelWithLoss.forward,
 * src/model/model.py:1042-1049): for P drawn pairs (a, b) -- pairs (P, 2) int32, drawn on the host --
 *   y = <codes[a], codes[b]>, d2 = ||vecs[a] - vecs[b]||^2, L = y d2 + (1 - y) max(margin - d2, 0)^2, *loss_out = sum_p L_p / P.
 * vecs (N, K) fp32, codes (N, C) fp32; N >= 2, 1 <= P <= N(N-1).  One workgroup; the per-pair terms are formed in double and summed in
 * pair order (deterministic, no atomics), the loss rounded to fp32 once.  coef_ws (P floats) receives dL_p/d(d2) / P for the backward.
 * Backward: d_vecs (N, K) is overwritten with *d_loss * dloss/dvecs (d_loss: device scalar), every element owned by one thread that
 * walks the pairs in order; d = 0 gives a zero gradient.  A pair index outside [0, N) yields NaN (loss, coef, every gradient entry).
 * ---------------------------------------------------------------------------------------------- */
int find_contrastive_fwd(const float* vecs, int64_t N, int64_t K, const float* codes, int64_t C, const int32_t* pairs, int64_t P, float margin,
						 float* loss_out, float* coef_ws, void* stream);
int find_contrastive_bwd(const float* vecs, int64_t N, int64_t K, const int32_t* pairs, int64_t P, const float* coef_ws, const float* d_loss,
						 float* d_vecs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2-D part loss.  Replaces everything RestylePerceptualLoss.forward(mode='cluster', pred_logit=...) does after the encoder
 * (src/model/losses.py:251-302; call site src/model/model.py:1129-1147).
 * find_part_labels: gt_logits (B, C, h, w) fp32 NCHW -> labels (B, H, W) int32 = argmax_c of the bilinear resample to (H, W) with
 *   F.interpolate's defaults (align_corners=False: src = (dst + 0.5) * in / out - 0.5, clamped at 0), lowest index on ties (a NaN counts
 *   as the maximum, as torch.argmax); the resampled tensor is never stored.
 * find_part_ce_fwd: logits (P, C) fp32 channel-last (a feature render, P = B*H*W pixels), labels (P) int32, mask (P) fp32:
 *   z_0 = 100 where mask == 0, else 0 (the rendered channel 0 is never read);  z_c = logits_c, c >= 1;
 *   ce = logsumexp_c z - z_label;  ce_out (P) = ce * mask;  *loss_out = sum_p ce_out / P.
 *   Per-pixel arithmetic is fp32 with the maximum subtracted; the sum over pixels is double in a fixed order -- one partial per
 *   workgroup in partial_ws (cdiv(P, 64) doubles), then one workgroup adds the partials -- so two runs agree bit for bit (no atomics).
 * find_part_ce_bwd: d_logits (P, C) and d_mask (P) are overwritten (plain stores, every element; channel 0 gets zeros):
 *   d_logits_c = *d_loss / P * mask * (softmax(z)_c - [c == label]),  d_mask = *d_loss / P * ce   (ce recomputed: ce_out holds ce * mask).
 * A label outside [0, C) gives NaN (ce_out, the loss, that pixel's d_logits and d_mask): nothing is read through it.
 * form: FIND_PART_AUTO picks FIND_PART_STAGED (a tile of 64 .. 256 pixels through LDS, 16-byte global loads and stores, odd row pitch)
 *   when a 64-pixel tile fits 40 KiB and the pointers are 16-byte aligned, else FIND_PART_DIRECT (a lane walks its pixel's C floats in
 *   global memory); the other two values force a form (tools/part_loss_cost.py measures both) and FIND_PART_STAGED refuses what does not fit.
 * ---------------------------------------------------------------------------------------------- */
#define FIND_PART_AUTO 0
#define FIND_PART_DIRECT 1
#define FIND_PART_STAGED 2
int find_part_labels(const float* gt_logits, int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W, int32_t* labels, void* stream);
int find_part_ce_fwd(const float* logits, const int32_t* labels, const float* mask, int64_t P, int64_t C, float* loss_out, float* ce_out,
					 double* partial_ws, int64_t form, void* stream);
int find_part_ce_bwd(const float* logits, const int32_t* labels, const float* mask, int64_t P, int64_t C, const float* d_loss, float* d_logits,
					 float* d_mask, int64_t form, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Surface normals (normals.hip): vertex normals, the normal-map stage behind the feature render, a cosine loss between two maps.
 * No float atomics anywhere: two calls agree bit for bit.
 * find_vertex_normals_fwd: PyTorch3D's verts_normals_padded.  verts (N, V, 3); faces (faces_batch, F, 3) int32, faces_batch 1 (shared) or
 *   N (per mesh, rows of -1 pad the shorter ones); vf_off (faces_batch, V + 1) and vf_items (faces_batch, 3 F) int32: the corners
 *   (item = face * 3 + corner) at every vertex, ascending per vertex -- a CSR table, the caller's (functional.MeshTopology holds one for a
 *   shared topology).  normals_out (N, V, 3) = s / max(|s|, 1e-6), s = the sum of (v1 - v0) x (v2 - v0) over the vertex's corners in the
 *   table's order; (0, 0, 0) for a vertex of no face.  A face with an index outside [0, V) contributes nothing.
 * find_vertex_normals_bwd: d_verts (N, V, 3) overwritten (every element) from d_normals (N, V, 3): through the normalisation
 *   ((g - n (n . g)) / |s|; g / 1e-6 where |s| <= 1e-6), then through the cross products by the same gather.  d_raw_ws: N * V * 3 floats.
 * find_normal_map_fwd: raw (n_images, H, W, 3), a blended map of world-space normals -> out = (raw / |raw|) @ R[image % n_views]
 *   (R (n_views, 3, 3) row-major, p_view = p_world @ R; image = mesh * n_views + view); world != 0 skips the rotation (R may be NULL);
 *   0 where |raw| <= 1e-6.   find_normal_map_bwd: d_raw (overwritten) from d_out; 0 where |raw| <= 1e-6.
 * find_normal_loss_fwd: pred, target (P, 3), not necessarily unit; weight (P):  c_i = p^_i . t^_i (0 where |p_i| <= 1e-6 or |t_i| <= 1e-6),
 *   *loss_out = sum_i w_i (1 - c_i) / max(sum_i w_i, 1e-12).  fp32 per pixel; both sums in double, one pair of partials per workgroup of
 *   1024 pixels, added by one workgroup in a fixed order.  16-byte loads and stores when pred, target, weight (and d_pred) are 16-byte aligned.
 *   ws: find_normal_loss_ws_bytes(P) bytes, 8-byte aligned; the backward reads sum_i w_i from it, so it lives until then.
 * find_normal_loss_bwd: d_pred_i = -*d_loss * w_i / max(sum w, 1e-12) * (t^_i - c_i p^_i) / |p_i|  (overwritten, every element; 0 where c_i
 *   was forced to 0).  target and weight receive no gradient.
 * ---------------------------------------------------------------------------------------------- */
int find_vertex_normals_fwd(const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* vf_off, const int32_t* vf_items, int64_t N,
							int64_t V, int64_t F, float* normals_out, void* stream);
int find_vertex_normals_bwd(const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* vf_off, const int32_t* vf_items, int64_t N,
							int64_t V, int64_t F, const float* d_normals, float* d_raw_ws, float* d_verts, void* stream);
int find_normal_map_fwd(const float* raw, const float* R, int64_t n_images, int64_t n_views, int64_t H, int64_t W, int world, float* out, void* stream);
int find_normal_map_bwd(const float* raw, const float* R, const float* d_out, int64_t n_images, int64_t n_views, int64_t H, int64_t W, int world,
						float* d_raw, void* stream);
int64_t find_normal_loss_ws_bytes(int64_t P);
int find_normal_loss_fwd(const float* pred, const float* target, const float* weight, int64_t P, float* loss_out, void* ws, int64_t ws_bytes, void* stream);
int find_normal_loss_bwd(const float* pred, const float* target, const float* weight, int64_t P, const float* d_loss, const void* ws, float* d_pred,
						 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exact point-to-surface distance (surface.hip; not in the reference -- PyTorch3D's point_mesh_face_distance is the nearest relative).
 * points (N, P, 3) with per-mesh counts p_len (N) int32 (NULL = all P); verts (N, V, 3); faces (faces_batch, F, 3) int32, faces_batch 1
 * (shared) or N (per mesh, rows of -1 pad the shorter ones), as find_face_areas.  P = 0 and F = 0 are allowed.
 * find_point_face_fwd: for every valid point the nearest CLOSED triangle of its mesh: dist2 (N, P) the squared distance, idx (N, P) int32
 *   the face, bary (N, P, 3) the barycentrics of the closest point c = sum_i bary_i v_i, with dist2 = |p - c|^2 of those very weights.
 *   A -1 row, a face with an index outside [0, V) and a face whose float32 (b - a) x (c - a) is exactly zero (products rounded one by one)
 *   are never candidates; among equal distances the smallest face index wins.  Rows at or past p_len[n], and every row of a mesh without a
 *   candidate, get dist2 0, idx -1, bary 0.  Brute force over all faces with a bounding-sphere cull, no float atomics: bit-identical on
 *   repeat.  ws: find_point_face_ws_bytes(N, P) bytes, 8-byte aligned, free again when the call's work is done.
 * find_point_face_bwd: from g (N, P), the gradient of dist2:  d_points (N, P, 3) = 2 g (p - c), overwritten, every row (0 where idx is -1);
 *   d_verts[n, faces[idx, i]] += -2 g bary_i (p - c) with float atomics: d_verts (N, V, 3) must be zero-initialised.  The barycentrics count
 *   as constants (c minimises the distance over the triangle), which is the exact gradient almost everywhere.  Either output may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_point_face_ws_bytes(int64_t n_meshes, int64_t n_points);
int find_point_face_fwd(const float* points, const int32_t* p_len, const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes,
						int64_t n_points, int64_t n_verts, int64_t n_faces, float* dist2, int32_t* idx, float* bary, void* ws, int64_t ws_bytes, void* stream);
int find_point_face_bwd(const float* points, const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* idx, const float* bary,
						const float* g, int64_t n_meshes, int64_t n_points, int64_t n_verts, int64_t n_faces, float* d_points, float* d_verts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Similarity registration  X = ((v + disp) * S) @ R(euler 'XYZ') + t.
 * Replaces euler_angles_to_matrix + Transform3d().scale().rotate().translate().transform_points
 * in NeuralDisplacementField.get_meshes (src/model/model.py:481-491).
 * reg (n_feet, 9) = [t(3), euler(3), S(3)]; verts (verts_batch in {1, n_feet}, n_pts, 3).
 * ---------------------------------------------------------------------------------------------- */
int find_register_fwd(const float* verts, int64_t verts_batch, const float* disp, const float* reg,
					  int64_t n_feet, int64_t n_pts, float* out, void* stream);
/* d_out (n_feet,n_pts,3) -> d_disp (n_feet,n_pts,3), d_reg (n_feet,9).  ws: find_register_bwd_ws_bytes(). */
int64_t find_register_bwd_ws_bytes(int64_t n_feet, int64_t n_pts);
int find_register_bwd(const float* verts, int64_t verts_batch, const float* disp, const float* reg,
					  const float* d_out, int64_t n_feet, int64_t n_pts, float* d_disp, float* d_reg,
					  void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Linear PCA foot model: offsets[n,v,c] = sum_b coefs[v,b,c] * shapevec[n,b]   (PCAModel.get_meshes, src/model/model.py:581;
 * the registration that follows is find_register_fwd with disp = offsets, model.py:584-594).
 * coefs (V, B, 3) fp32 in the state_dict layout of pca_coefs; shapevec (n_feet, B); offsets (n_feet, V, 3).  1 <= B <= 4000,
 * 1 <= V < 2^29, 1 <= n_feet <= 2^20.  coefs is read once per call for all feet.
 * ---------------------------------------------------------------------------------------------- */
int find_pca_fwd(const float* coefs, int64_t V, int64_t B, const float* shapevec, int64_t n_feet, float* offsets, void* stream);
/* d_offsets (n_feet, V, 3) -> d_shapevec[n,b] = sum_{v,c} d_offsets[n,v,c] * coefs[v,b,c]  (n_feet, B); pca_coefs is frozen
 * (requires_grad=False, model.py:648) and gets no gradient.  ws: find_pca_bwd_ws_bytes() (-1 for bad sizes): one partial row per vertex
 * tile, added in tile order by a second kernel -- no atomics, bit-identical from run to run. */
int64_t find_pca_bwd_ws_bytes(int64_t n_feet, int64_t V, int64_t B);
int find_pca_bwd(const float* coefs, int64_t V, int64_t B, const float* d_offsets, int64_t n_feet, float* d_shapevec, void* ws, int64_t ws_bytes,
				 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Skinned foot model (src/model/model.py:726-727, SUPRModel.get_meshes: self.supr_model(poses, betas, trans)): SMPL-family linear blend
 * skinning with quaternion pose correctives, as STAR / SUPR publish it.  Per foot n and joint j, th = pose[n, 3j:3j+3], a = |th|:
 *   R_j = exp([th]x) (Rodrigues);  q_j = ((sin(a/2) / a) th, cos(a/2) - 1);  c = [betas | q_0.. (P = 4J) or q_1.. (P = 4(J-1))]
 *   v_posed = v_template + sum_k dirs[:, k] c_k;  Jn = J0 + JS . betas  (the joint regressor folded through the shape directions)
 *   G_0 = [R_0 | Jn_0], G_j = G_parent(j) o [R_j | Jn_j - Jn_parent(j)];  A_j = [G_j.R | G_j.t - G_j.R Jn_j]
 *   out[n, v] = sum_j weights[v, j] (A_j.R v_posed + A_j.t) + trans[n]
 * The angle is |th| itself, not STAR's |th + 1e-8|; power series below a = 1, so values and derivatives are exact at th = 0.
 * v_template (V, 3); dirs (V, B+P, 3), shape directions first (the layout of pca_coefs); J0 (J, 3); JS (J, B, 3); weights (V, J);
 * parent (J) int32, parent[j] < j, anything else (as the root's -1) read as "no parent"; pose (n_feet, 3J); betas (n_feet, B);
 * trans (n_feet, 3); out (n_feet, V, 3); joints NULL or (n_feet, J, 3), the posed joints G_j.t.
 * 1 <= J <= 128, P = 4J or 4(J-1), 3(B+P) padded + J within 9216 floats, B + P + 12J <= 3072, 1 <= V < 2^29, 1 <= n_feet <= 2^20.
 * dirs and weights are read once per call for all feet.  ws: find_skin_fwd_ws_bytes / find_skin_bwd_ws_bytes (-1 for bad sizes).
 * find_skin_bwd: d_out (n_feet, V, 3) -> d_pose, d_betas, d_trans (shaped as their inputs); the model gets no gradient.  Sums over the
 * vertices go tile by tile in a fixed order: no atomics, bit-identical from run to run, and a foot's rows do not depend on n_feet.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_skin_fwd_ws_bytes(int64_t n_feet, int64_t V, int64_t J, int64_t B, int64_t P);
int find_skin_fwd(const float* v_template, const float* dirs, const float* J0, const float* JS, const float* weights, const int32_t* parent, int64_t V,
				  int64_t J, int64_t B, int64_t P, const float* pose, const float* betas, const float* trans, int64_t n_feet, float* out, float* joints,
				  void* ws, int64_t ws_bytes, void* stream);
int64_t find_skin_bwd_ws_bytes(int64_t n_feet, int64_t V, int64_t J, int64_t B, int64_t P);
int find_skin_bwd(const float* v_template, const float* dirs, const float* J0, const float* JS, const float* weights, const int32_t* parent, int64_t V,
				  int64_t J, int64_t B, int64_t P, const float* pose, const float* betas, const float* d_out, int64_t n_feet, float* d_pose,
				  float* d_betas, float* d_trans, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Surface sampling gather.  Replaces the gather/lerp half of pytorch3d.ops.sample_points_from_meshes
 * (call sites src/model/losses.py:39-41,63,67; src/eval/eval_3d.py:149-150); the random draws
 * (face index, u, v) are INPUTS so CPU and GPU runs see identical samples.
 * verts (n_meshes, n_verts, 3); faces (n_faces, 3) int32 shared topology when faces_batch == 1, else
 * (n_meshes, n_faces, 3); face_idx (n_meshes, n_samples) int32; uv (n_meshes, n_samples, 2).
 * out (n_meshes, n_samples, 3) = w0*v0 + w1*v1 + w2*v2,  (w0,w1,w2) = (1-sqrt(u), sqrt(u)(1-v), sqrt(u)v).
 * `attr` (optional, same layout as verts, n_attr channels=3) is sampled into attr_out with the same weights.
 * A corner whose vertex index lies outside [0, n_verts) -- the -1 rows that pad a ragged batch's faces, when a given draw names one --
 * adds nothing, forward and backward, and nothing is read through it.
 * ---------------------------------------------------------------------------------------------- */
int find_sample_points_fwd(const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* face_idx,
						   const float* uv, int64_t n_meshes, int64_t n_verts, int64_t n_faces, int64_t n_samples,
						   float* out, const float* attr, float* attr_out, void* stream);
/* d_out (n_meshes,n_samples,3) scattered to d_verts (n_meshes,n_verts,3), which must be zero-initialised. */
int find_sample_points_bwd(const int32_t* faces, int64_t faces_batch, const int32_t* face_idx, const float* uv,
						   const float* d_out, int64_t n_meshes, int64_t n_verts, int64_t n_faces, int64_t n_samples,
						   float* d_verts, void* stream);
/* Face areas 0.5*|(v1-v0)x(v2-v0)| (n_meshes, n_faces): the multinomial weights of the sampler. */
int find_face_areas(const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts,
					int64_t n_faces, float* areas, void* stream);
/* The whole of sample_points_from_meshes with the face choice on the device (same call sites): faces ~ multinomial(area) with
 * replacement -- a block per mesh builds the running sum of the face areas (ws: find_sample_surface_ws_bytes), a thread per sample
 * searches it with its uniform draw -- then the gather above.  rnd (n_meshes, n_samples, 3) uniform in [0,1): [face draw, u, v];
 * only the DRAWS are inputs (torch's device generator, exactly where PyTorch3D would draw).  Outputs: face_idx (n_meshes, n_samples)
 * int32 and uv (n_meshes, n_samples, 2) -- what find_sample_points_bwd / find_uv_sample need --, out and optionally attr_out as
 * above.  Faces of zero area (and the -1 padding of ragged batches) are never chosen; a mesh of total area 0 yields face 0. */
int64_t find_sample_surface_ws_bytes(int64_t n_meshes, int64_t n_faces);
int find_sample_surface_fwd(const float* verts, const int32_t* faces, int64_t faces_batch, const float* rnd, int64_t n_meshes,
							int64_t n_verts, int64_t n_faces, int64_t n_samples, int32_t* face_idx, float* uv, float* out,
							const float* attr, float* attr_out, void* ws, int64_t ws_bytes, void* stream);
/* The same for a mesh whose running area sum is already in `ws`: left there by an earlier find_sample_surface_fwd on the SAME verts /
 * faces (a GT scan is sampled twice per training step and does not change between steps: losses.py:39,63).  Only the search + gather run. */
int find_sample_surface_again(const float* verts, const int32_t* faces, int64_t faces_batch, const float* rnd, int64_t n_meshes,
							  int64_t n_verts, int64_t n_faces, int64_t n_samples, int32_t* face_idx, float* uv, float* out,
							  const float* attr, float* attr_out, const void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Chamfer nearest neighbour (K=1, squared L2, brute force).
 * Replaces pytorch3d.ops.knn_points inside pytorch3d.loss.chamfer_distance
 * (call sites src/model/losses.py:77,85,88; src/eval/eval_3d.py:151,159).
 * x (n, p1_max, 3) with per-cloud lengths x_len (n) int32 (NULL = all p1_max); same for y.
 * Outputs for every valid x_i: dist (n,p1_max) = min_j |x_i-y_j|^2, idx (n,p1_max) int32 = argmin_j
 * (lowest j on ties); padding rows get dist 0 / idx -1.
 * ---------------------------------------------------------------------------------------------- */
int find_nn_fwd(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, int64_t n,
				int64_t p1_max, int64_t p2_max, float* dist, int32_t* idx, void* stream);
/* Chamfer gradient for one direction: for valid i, g = 2*w[n,i]*(x_i - y_idx);  d_x[n,i] += g ; d_y[n,idx] -= g.
 * w (n,p1_max) is the upstream gradient of dist.  d_x / d_y must be zero-initialised (or hold the other
 * direction's contribution); either may be NULL. */
int find_nn_bwd(const float* x, const int32_t* x_len, const float* y, const int32_t* idx, const float* w, int64_t n,
				int64_t p1_max, int64_t p2_max, float* d_x, float* d_y, void* stream);
/* pytorch3d.loss.chamfer_distance with its defaults as ONE loss (the reference never uses anything else: losses.py:77,85,88;
 * eval_3d.py:151,159): both nearest-neighbour directions in one launch, then
 *   loss = ( sum_n sum_i min_j|x_i-y_j|^2 / max(x_len[n],1)  +  sum_n sum_j min_i|x_i-y_j|^2 / max(y_len[n],1) ) / n
 * as a 1-element device scalar (deterministic reduction).  ws (find_chamfer_ws_bytes) keeps the neighbours for the backward and must
 * be passed to it untouched.  find_chamfer_bwd: g_loss = device scalar, the upstream gradient; d_x (n,p1_max,3) / d_y (n,p2_max,3)
 * must be zero-initialised, either may be NULL; contributions are added with float atomics (as PyTorch3D's knn backward). */
int64_t find_chamfer_ws_bytes(int64_t n, int64_t p1_max, int64_t p2_max);
int find_chamfer_fwd(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, int64_t n, int64_t p1_max,
					 int64_t p2_max, float* loss, void* ws, int64_t ws_bytes, void* stream);
int find_chamfer_bwd(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, int64_t n, int64_t p1_max,
					 int64_t p2_max, const float* g_loss, const void* ws, int64_t ws_bytes, float* d_x, float* d_y, void* stream);
/* find_chamfer_bwd and find_sample_points_bwd in one, for x = the samples find_sample_surface_fwd drew on a mesh (x (n,p1,3), all valid;
 * face_idx, uv: what that call returned) and a y that takes no gradient: d_verts (n,n_verts,3) is OVERWRITTEN with the loss's gradient
 * with respect to the mesh's vertices -- no zero-initialisation, no d_x in memory, no global float atomic: a workgroup sums d_x of a
 * range of one foot's samples and then an image of that foot's d_verts in LDS and stores the image; several workgroups per foot write a
 * slab each into ws, summed in a fixed order.  chamfer_ws: find_chamfer_fwd's workspace, untouched.
 * find_chamfer_surface_bwd_ws_bytes < 0: the image (n_verts * 12 bytes) and a range's d_x do not fit one workgroup's LDS, or bad
 * sizes -- use the two calls above. */
int64_t find_chamfer_surface_bwd_ws_bytes(int64_t n, int64_t n_verts, int64_t n_samples);
int find_chamfer_surface_bwd(const float* x, const float* y, const int32_t* y_len, int64_t n, int64_t p1, int64_t p2_max,
							 const float* g_loss, const void* chamfer_ws, int64_t chamfer_ws_bytes, const int32_t* faces,
							 int64_t faces_batch, const int32_t* face_idx, const float* uv, int64_t n_verts, int64_t n_faces,
							 float* d_verts, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Masked colour error of TextureLossGTSpace (src/model/losses.py:43-57): mask = any(target < 1) per point, loss = mean over all
 * n_pts * 3 elements of mask * (pred - target)^2 -- F.mse_loss(reduction='none') * mask, .mean() -- as a 1-element device scalar.
 * pred, target (n_pts, 3).  The backward overwrites d_pred (n_pts, 3) with g_loss * dloss/dpred (g_loss: device scalar).
 * ---------------------------------------------------------------------------------------------- */
int find_masked_mse_fwd(const float* pred, const float* target, int64_t n_pts, float* loss, void* stream);
int find_masked_mse_bwd(const float* pred, const float* target, int64_t n_pts, const float* g_loss, float* d_pred, void* stream);
/* Image losses in one pass each way: loss = mean over n_pix x channels of (a * a_mask - b * b_mask)^2, masks per pixel or NULL (= 1).
 * Replaces nn.MSELoss on image * mask.unsqueeze(-1) products (pixel loss, src/model/model.py:1101-1105: images compared inside their
 * silhouettes) and on the two masks (silhouette loss, model.py:1107-1108 / losses.py:122-128: channels = 1, no masks).  ws: find_image_mse_ws_bytes().
 * Backward: gradients w.r.t. a (d_a, same shape) and a_mask (d_a_mask, per pixel), either may be NULL; b / b_mask are the GT side. */
int64_t find_image_mse_ws_bytes(void);
int find_image_mse_fwd(const float* a, const float* a_mask, const float* b, const float* b_mask, int64_t n_pix, int64_t channels, float* loss,
					   void* ws, int64_t ws_bytes, void* stream);
int find_image_mse_bwd(const float* a, const float* a_mask, const float* b, const float* b_mask, int64_t n_pix, int64_t channels,
					   const float* g_loss, float* d_a, float* d_a_mask, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2-D evaluation sums in one pass (src/eval/eval_2d.py:92-121 with the metrics of src/eval/eval_metrics.py:4-40).  Per image i, with
 *   p~ = 1 where hide[i,p] else pred,   m~ = 0 where hide[i,p] else pred_mask    (the in-place edit of eval_2d.py:92-94, not written back)
 *   sums[i][FIND_IMAGE_METRIC_SQ]        = sum_p,c (g - p~)^2                         MSE, PSNR_A
 *   sums[i][FIND_IMAGE_METRIC_SQ_EACH]   = sum_p,c (g [gm>0] - p~ [m~>0])^2           PSNR_B (each image inside its own silhouette)
 *   sums[i][FIND_IMAGE_METRIC_SQ_COMMON] = sum_p,c [gm>0 and m~>0] (g - p~)^2         PSNR_C (inside both)
 *   sums[i][FIND_IMAGE_METRIC_INTER]     = sum_p gm m~                                IOU intersection
 *   sums[i][FIND_IMAGE_METRIC_UNION]     = sum_p max(gm, m~)                          IOU union
 *   sums[i][FIND_IMAGE_METRIC_WSQ]       = sum_p,c w (g - p~)^2                       MSE_masked
 *   sums[i][FIND_IMAGE_METRIC_W]         = sum_p w                                    MSE_masked denominator (times channels)
 * pred, gt (n_img, n_pix, channels) fp32; pred_mask, gt_mask, weight (n_img, n_pix) fp32 or NULL (= 1); hide (n_img, n_pix) bytes (0 / non-zero:
 * the renderer's bool mask_out_masks) or NULL (= nothing hidden).  sums (n_img, 7) fp64.  ws: find_image_metrics_ws_bytes(n_img, n_pix)
 * (-1 for bad sizes).  Terms are formed in fp32, at most 4 pixels of them added in fp32, everything after that in fp64; the block split
 * depends on (n_img, n_pix) only and every reduction runs in a fixed order: bit-identical from run to run.
 * ---------------------------------------------------------------------------------------------- */
#define FIND_IMAGE_METRIC_SQ 0
#define FIND_IMAGE_METRIC_SQ_EACH 1
#define FIND_IMAGE_METRIC_SQ_COMMON 2
#define FIND_IMAGE_METRIC_INTER 3
#define FIND_IMAGE_METRIC_UNION 4
#define FIND_IMAGE_METRIC_WSQ 5
#define FIND_IMAGE_METRIC_W 6
#define FIND_IMAGE_METRIC_COUNT 7
int64_t find_image_metrics_ws_bytes(int64_t n_img, int64_t n_pix);
int find_image_metrics(const float* pred, const float* gt, const float* pred_mask, const float* gt_mask, const uint8_t* hide, const float* weight,
					   int64_t n_img, int64_t n_pix, int64_t channels, double* sums, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh smoothness: mesh_edge_loss(target 0) and mesh_laplacian_smoothing('cot').
 * Replaces pytorch3d.loss.mesh_edge_loss / mesh_laplacian_smoothing (call site src/model/losses.py:95-97).
 * Topology is shared by every mesh in the batch (one template) and static, so the host builds two CSR tables once:
 *   vf_off (n_verts+1), vf_items (3*n_faces): for every vertex the incident corners, item = face*3 + corner;
 *   nbr_off (n_verts+1), nbr_idx (2*n_edges): for every vertex its neighbours over the unique undirected edges.
 * faces (n_faces,3) int32; verts (n_meshes,n_verts,3).  All kernels are deterministic gathers (no float atomics).
 * Outputs: loss_edge, loss_lap: 1-element device scalars (batch means, as PyTorch3D).
 * ws: find_smooth_ws_bytes();  the forward leaves what the backward needs in ws.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_smooth_ws_bytes(int64_t n_meshes, int64_t n_verts, int64_t n_faces);
int find_smooth_fwd(const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_items,
					const int32_t* nbr_off, const int32_t* nbr_idx, int64_t n_meshes, int64_t n_verts, int64_t n_faces,
					int64_t n_edges, float* loss_edge, float* loss_lap, void* ws, int64_t ws_bytes, void* stream);
/* d_verts (n_meshes,n_verts,3) OVERWRITTEN with g_edge*dLedge/dV + g_lap*dLlap/dV; g_* are device scalars. */
int find_smooth_bwd(const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_items,
					const int32_t* nbr_off, const int32_t* nbr_idx, int64_t n_meshes, int64_t n_verts, int64_t n_faces,
					int64_t n_edges, const float* g_edge, const float* g_lap, void* ws, int64_t ws_bytes, float* d_verts,
					void* stream);
/* MeshSmoothnessLoss as one scalar (src/model/losses.py:93-99: 0.1 * laplacian + 10 * edge): loss = w_edge * loss_edge + w_lap * loss_lap
 * written by the same three kernels; the backward takes the upstream gradient of that scalar (device pointer) and the two weights. */
int find_smooth_loss_fwd(const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_items,
						 const int32_t* nbr_off, const int32_t* nbr_idx, int64_t n_meshes, int64_t n_verts, int64_t n_faces,
						 int64_t n_edges, float w_edge, float w_lap, float* loss, void* ws, int64_t ws_bytes, void* stream);
int find_smooth_loss_bwd(const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_items,
						 const int32_t* nbr_off, const int32_t* nbr_idx, int64_t n_meshes, int64_t n_verts, int64_t n_faces,
						 int64_t n_edges, float w_edge, float w_lap, const float* g_loss, void* ws, int64_t ws_bytes,
						 float* d_verts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Differentiable mesh render: world->view->NDC transform, rasterisation, fused shading.
 * Replaces FootRenderer.forward / rasterize (src/model/renderer.py:208-245, 247-383), i.e. PyTorch3D's
 * FoVPerspectiveCameras + rasterize_meshes (naive and binned) + SoftSilhouetteShader + SoftPhongShader +
 * softmax_rgb_blend (in-repo mirror src/model/renderer.py:23-72), and their backward.
 *
 * Image index = mesh*n_views + view (renderer.py:271-277).  verts (n_meshes, n_verts, 3) world space;
 * faces (n_faces,3) int32 shared when faces_batch==1 else (n_meshes,n_faces,3); R (n_views,3,3), T (n_views,3)
 * in PyTorch3D row-vector convention (p_view = p_world @ R + T).
 * ---------------------------------------------------------------------------------------------- */
typedef struct find_render_params {
	int32_t image_h, image_w;
	float fov_deg;        /* 60 */
	float znear, zfar;    /* 0.02, 100 (renderer.py:274; PyTorch3D default zfar) */
	float sil_blur_radius;/* log(1/1e-4 - 1) * 1e-4 (renderer.py:127) */
	float sil_sigma;      /* 1e-4 (renderer.py:124) */
	int16_t sil_faces_per_pixel; /* 100 (renderer.py:128); the soft mask uses the K nearest-in-depth faces (1 .. 32767) */
	int16_t clip_faces;   /* 0: a face that straddles the z-clip plane is rasterised whole and counted in find_render_flags' out2[0];
	                       * 1: it is clipped as PyTorch3D's clip.py does (cull_to_frustum=False): one vertex behind the plane -> a quad
	                       * split into two triangles, two behind -> one triangle; pix_to_face, the barycentrics (find_render_frags)
	                       * and the shading refer to the original face, zbuf and the silhouette distances to the clipped triangle.
	                       * Every image then has 2 x n_faces face slots (the second triangles of split quads after every face), so
	                       * the workspace grows (find_render_ws_bytes), and n_faces must stay below 2^23.  No host synchronisation
	                       * either way: both modes can be captured in a HIP graph.
	                       * (The flag takes the upper half of what was an int32 K: the struct keeps its size and layout, and a
	                       * caller that still writes K as an int32 gets clip_faces = 0 on this little-endian target.) */
	float rgb_sigma, rgb_gamma;  /* 1e-4, 1e-4 BlendParams defaults */
	float background[3];  /* (1,1,1) renderer.py:109,118 */
	float light_pos[3];   /* (0,0,100) renderer.py:114 */
	float ambient, diffuse, specular, shininess; /* 0.5, 0.3, 0.2, 64 (PyTorch3D PointLights/Materials defaults) */
	float z_clip;         /* znear/2 (renderer.py:231-234) */
} find_render_params;

int64_t find_render_ws_bytes(const find_render_params* rp, int64_t n_meshes, int64_t n_views, int64_t n_verts,
							 int64_t n_faces);
/* Outputs (any may be NULL to skip): mask (n_meshes,n_views,H,W) soft silhouette; image (n_meshes,n_views,H,W,3)
 * Phong RGB; pix_to_face (n_meshes,n_views,H,W) int32 nearest face (K=1, blur 0) packed id mesh*n_faces+f or -1;
 * zbuf (n_meshes,n_views,H,W) depth of that face (-1 where empty).  vert_colors (n_meshes,n_verts,3) needed for image. */
int find_render_fwd(const find_render_params* rp, const float* verts, const int32_t* faces, int64_t faces_batch,
					const float* vert_colors, const float* R, const float* T, int64_t n_meshes, int64_t n_views,
					int64_t n_verts, int64_t n_faces, float* mask, float* image, int32_t* pix_to_face, float* zbuf,
					void* ws, int64_t ws_bytes, void* stream);
/* d_mask / d_image upstream grads (either NULL); `mask` is the forward's soft silhouette (required with d_mask; the kernel reads the
 * alpha product the forward saved in ws beside it -- 1 - mask is zero wherever the mask has rounded to 1).
 * d_verts (n_meshes,n_verts,3) and d_vert_colors (same, may be NULL) are OVERWRITTEN.  ws must be the forward workspace,
 * untouched since find_render_fwd (it holds the projected faces and the nearest-fragment buffers). */
int find_render_bwd(const find_render_params* rp, const float* verts, const int32_t* faces, int64_t faces_batch,
					const float* vert_colors, const float* R, const float* T, int64_t n_meshes, int64_t n_views,
					int64_t n_verts, int64_t n_faces, const float* mask, const float* d_mask, const float* d_image,
					float* d_verts, float* d_vert_colors, void* ws, int64_t ws_bytes, void* stream);
/* Diagnostics of the last forward that used `ws` (synchronises the stream): out2[0] = faces straddling the z-clip
 * plane that were rasterised whole (clip_faces = 0; PyTorch3D would clip them -- none exists on FIND's camera set-up; always 0
 * with clip_faces = 1),
 * out2[1] = pixels left UNRESOLVED by the K-nearest rule: a pixel with more silhouette candidates than
 * sil_faces_per_pixel keeps the K nearest in depth (ties to the earlier face, as PyTorch3D's per-pixel K-buffer);
 * only a pixel with more than 4096 candidates is not resolved -- all of its candidates stay blended. */
int find_render_flags(const void* ws, int32_t* out2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Keypoint splats (FootRenderer(..., keypoints=...), src/model/renderer.py:139-142, 365-376): PyTorch3D's PointsRasterizer with
 * PointsRasterizationSettings(radius, points_per_pixel) and the renderer's FoVPerspectiveCameras, fused with PointsRenderer +
 * AlphaCompositor (no background), forward only.  Image index = cloud*n_views + view: cloud n is drawn in each of the n_views views.
 * A point with view-space z < 0 is skipped; it covers a pixel if d^2 < radius^2 in NDC (strict); each pixel keeps the
 * points_per_pixel points of smallest z (equal z: lower point index) and composites them front to back with w = 1 - d^2 / radius^2.
 * points, features (n_clouds,P,3); R (n_views,3,3), T (n_views,3) as find_render_fwd.  Outputs (any may be NULL, not all):
 * image (n_clouds*n_views,H,W,3), 0 where no point lands; idx (…,H,W,K) int32 point index within the cloud, zbuf (view-space z) and
 * dists (d^2) (…,H,W,K), -1 in empty slots.  1 <= points_per_pixel <= 32, radius > 0.  No workspace, no host synchronisation, no
 * atomics: repeated calls are bit-identical.
 * ---------------------------------------------------------------------------------------------- */
typedef struct find_points_params {
	int32_t image_h, image_w;
	float fov_deg;           /* 60, as find_render_params */
	float radius;            /* 0.03 NDC units (renderer.py:140) */
	int32_t points_per_pixel;/* 10 (renderer.py:140) */
} find_points_params;

int find_points_render(const find_points_params* pp, const float* points, const float* features, const float* R, const float* T,
					   int64_t n_clouds, int64_t n_views, int64_t P, float* image, int32_t* idx, float* zbuf, float* dists, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Video frames of a render (src/vis/mesh_turntable.py:60-61: (255 * image).astype(np.uint8), then cv2.rotate(..., ROTATE_180)).
 * img (n,h,w,c) fp32 -> out (n,h,w,c) bytes: out = (uint8) min(max(255.f * x, 0.f), 255.f), i.e. truncation toward zero, NaN -> 0;
 * with rot180 != 0 pixel (y, x) of image i goes to (h-1-y, w-1-x), channels in order.  1 <= c <= 16, n*h*w*c <= 2^40; img and out must
 * not overlap.  One pass, no workspace, no host synchronisation; 16-byte loads and packed 32-bit stores when h*w (n*h*w without rot180)
 * is a multiple of 4, c is 1 or 3 and img / out are 16- / 4-byte aligned, a pixel per thread otherwise.
 * ---------------------------------------------------------------------------------------------- */
int find_frames_u8(const float* img, int64_t n, int64_t h, int64_t w, int64_t c, int rot180, uint8_t* out, void* stream);


/* ------------------------------------------------------------------------------------------------
 * UV textures.  Replaces pytorch3d TexturesUV.sample_textures as the reference uses it for GT scans
 * (src/data/dataset.py:263-271 builds TexturesUV(img, faces_uvs, verts_uvs); losses.py:39-43 samples GT surface colours;
 * renderer.py:329-346 renders GT images): colour at a surface point = bilinear read of the vertically flipped map at the
 * barycentric mix of the face's three UV vertices (grid_sample align_corners=True, padding_mode='border').
 * maps (n_maps,H,W,3); verts_uvs (n_maps,Vt,2); faces_uvs (1|n_maps, F, 3) int32; face_idx / bary (n_rows,P[,3]) with
 * n_rows a multiple of n_maps (rows of one map consecutive: feet x views); face_idx < 0 -> zeros.
 * find_render_frags copies out the nearest-fragment buffers (local face id, barycentrics) of the forward that used `ws`.
 * ---------------------------------------------------------------------------------------------- */
int find_uv_sample(const float* maps, int64_t n_maps, int64_t map_h, int64_t map_w, const float* verts_uvs, int64_t n_uv_verts,
				   const int32_t* faces_uvs, int64_t faces_batch, int64_t n_faces, const int32_t* face_idx, const float* bary,
				   int64_t n_rows, int64_t n_points, float* out, void* stream);
int find_render_frags(const find_render_params* rp, int64_t n_meshes, int64_t n_views, int64_t n_verts, int64_t n_faces, const void* ws,
					  int32_t* face_local, float* bary, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Baking into UV maps (bake.hip): the writing half of the UV textures above.  Not in the reference (it only ever reads scan textures).
 * Texel (i, j) of an H x W map has its centre at (u, v) = (j / (W - 1), 1 - i / (H - 1)), row 0 the top of the image: the points
 * find_uv_sample reads without interpolation.  2 <= H, W <= 4096.
 * find_uv_raster: verts_uvs (n_uv_verts, 2), faces_uvs (n_faces, 3) int32 -> face (H, W) int32, the SMALLEST face index whose closed UV
 *   triangle (either orientation) contains the texel's centre, -1 where none does, and bary (H, W, 3): the three edge functions of that face
 *   at the centre over its signed area, in fp32 without contraction, recomputed from the winning face (0 where face is -1).  A face with an
 *   index outside [0, n_uv_verts) or with a signed area that is 0 or NaN in fp32 covers nothing; UVs outside [0, 1] are legal and do not
 *   wrap.  n_faces = 0 writes -1 / 0 everywhere (verts_uvs / faces_uvs may then be NULL).  A wave per face walks the face's clamped bounding
 *   box in 8 x 8 tiles (boxes of many tiles are shared by 16 waves) and takes the minimum into `face` itself with integer atomics, which
 *   is independent of their order: repeated calls are bit-identical; a texel per lane then writes -1 / bary.
 * find_uv_dilate_map: face (H, W) as above -> src (H, W) int32, the flat index i * W + j of the texel to copy: a covered texel (face >= 0)
 *   its own, an uncovered one that of the covered texel within Chebyshev distance `pad` with the smallest di^2 + dj^2 (ties: the smallest
 *   flat index), -1 if there is none.  0 <= pad <= 16.  The gutter that keeps find_uv_sample's bilinear reads off the background.
 * Neither uses a workspace or synchronises with the host.
 * ---------------------------------------------------------------------------------------------- */
int find_uv_raster(const float* verts_uvs, int64_t n_uv_verts, const int32_t* faces_uvs, int64_t n_faces, int64_t map_h, int64_t map_w,
				   int32_t* face, float* bary, void* stream);
int find_uv_dilate_map(const int32_t* face, int64_t map_h, int64_t map_w, int64_t pad, int32_t* src, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-vertex feature render (FootRenderer.forward(..., return_features=True, features=...), src/model/renderer.py:293-299).
 * Replaces FeatureShader.forward (renderer.py:74-105) on fragments['sil']: [P3D-recall] TexturesVertex(features).sample_textures
 * (interpolate_face_attributes with the clipped, perspective-correct barycentrics of the K = sil_faces_per_pixel, blurred pass) and
 * softmax_blend (renderer.py:23-72) with its DEFAULT znear = 1, zfar = 100 -- not the camera's znear --, sigma = rgb_sigma, gamma =
 * rgb_gamma and a background of C zeros.  features (n_meshes,n_verts,C) fp32; out (n_meshes,n_views,H,W,C), 0 where no fragment.
 * `ws` must come from a find_render_fwd WITH a mask (its K nearest silhouette candidates per pixel and its tile lists are read) of the same
 * geometry, untouched since; a workspace without one is refused (FIND_EINVAL), as are clip_faces = 1 and n_channels < 1.  `fws`
 * (find_render_features_ws_bytes) carries per-pixel state from the forward to the backward.  No host synchronisation; the forward uses
 * no atomics (repeated calls are bit-identical).
 * find_render_features_bwd: d_out (like out) upstream gradient; `out` the forward's output.  d_verts (n_meshes,n_verts,3) is ADDED TO
 * (find_render_bwd overwrites it: call that first when the mask or image has a gradient too), d_features (n_meshes,n_verts,C) is
 * OVERWRITTEN, summed over the views; either may be NULL, not both.  It reuses the projection gradient buffer of `ws`.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_render_features_ws_bytes(const find_render_params* rp, int64_t n_meshes, int64_t n_views, int64_t n_channels);
int find_render_features_fwd(const find_render_params* rp, const float* verts, const int32_t* faces, int64_t faces_batch, const float* R,
							 const float* T, int64_t n_meshes, int64_t n_views, int64_t n_verts, int64_t n_faces, const float* features,
							 int64_t n_channels, float* out, const void* ws, int64_t ws_bytes, void* fws, int64_t fws_bytes, void* stream);
int find_render_features_bwd(const find_render_params* rp, const float* verts, const int32_t* faces, int64_t faces_batch, const float* R,
							 const float* T, int64_t n_meshes, int64_t n_views, int64_t n_verts, int64_t n_faces, const float* features,
							 int64_t n_channels, const float* out, const float* d_out, float* d_verts, float* d_features, void* ws,
							 int64_t ws_bytes, void* fws, int64_t fws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth (depth.hip): the backward of find_render_fwd's zbuf -- view-space z of the nearest face, -1 on the background -- and a masked,
 * robust loss between two depth maps.  Not in the reference (PyTorch3D's fragments.zbuf carries this gradient).
 * find_depth_bwd: d_verts (n_meshes, n_verts, 3) is OVERWRITTEN from d_depth (n_meshes, n_views, H, W).  pix_to_face is what
 *   find_render_fwd handed out: the packed id image * n_faces + f, or -1; verts, faces, faces_batch, R, T as there (faces shared, or per
 *   mesh with rows of -1 padding).  Self-contained: no render workspace is read.  Per pixel with a face, with p_k = v_k @ R[view] + T[view]
 *   the face's corners in view space, d = (x_ndc / s, y_ndc / s, 1) the pixel's ray (s = 1 / tan(fov / 2), x_ndc = 1 - (2 xi + 1) / W,
 *   y_ndc = 1 - (2 yi + 1) / H), n = (p1 - p0) x (p2 - p0):
 *     z = (n . p0) / (n . d),  X = z d,  b_k = ((p_{k+1} - X) x (p_{k+2} - X)) . n / (n . n),
 *     d p_k = g b_k n / (n . d),  d v_k += d p_k @ R[view]^T.
 *   The triangles split mode (clip_faces = 1) cuts lie in their face's plane and pix_to_face names the face: the same formula holds there.
 *   A pixel with -1, a face index outside [0, n_faces), a vertex index outside [0, n_verts) or n . d == 0 adds nothing and nothing is read
 *   through such an index.  The sum over pixels uses float atomics: two runs may differ in the last bits.
 * find_depth_loss_fwd: pred, target (n_img, n_pix); weight (n_img, n_pix) or NULL (= 1).  r = pred - target; a pixel is valid where
 *   pred > 0, target > 0 and (trunc <= 0 or |r| <= trunc); w_i = weight_i on valid pixels, 0 elsewhere;
 *   rho = |r| (FIND_DEPTH_L1), r^2 (FIND_DEPTH_L2), r^2 / (2 delta) for |r| <= delta and |r| - delta / 2 beyond (FIND_DEPTH_HUBER, delta > 0);
 *   *loss_out = sum_i w_i rho(r_i) / max(sum_i w_i, 1e-12).  fp32 per pixel; both sums in double, one pair of partials per workgroup of 1024
 *   pixels of ONE image, added by one workgroup in a fixed order (no atomics: bit-identical on repeat).  per_image (n_img, 2) fp64 or NULL:
 *   [sum w rho, sum w] of every image.  16-byte loads and stores where the pointers and the image's first pixel are 16-byte aligned.
 *   ws: find_depth_loss_ws_bytes(n_img, n_pix) bytes (-1 for bad sizes), 8-byte aligned; the backward reads sum w from it.
 * find_depth_loss_bwd: d_pred_i = *d_loss w_i rho'(r_i) / max(sum w, 1e-12), overwritten, every element (sign(0) = 0).  target and weight
 *   receive no gradient.
 * ---------------------------------------------------------------------------------------------- */
enum { FIND_DEPTH_L1 = 0, FIND_DEPTH_L2 = 1, FIND_DEPTH_HUBER = 2 };
int find_depth_bwd(const find_render_params* rp, const float* verts, const int32_t* faces, int64_t faces_batch, const float* R, const float* T,
				   int64_t n_meshes, int64_t n_views, int64_t n_verts, int64_t n_faces, const int32_t* pix_to_face, const float* d_depth,
				   float* d_verts, void* stream);
int64_t find_depth_loss_ws_bytes(int64_t n_img, int64_t n_pix);
int find_depth_loss_fwd(const float* pred, const float* target, const float* weight, int64_t n_img, int64_t n_pix, int kind, float delta, float trunc,
						float* loss_out, double* per_image, void* ws, int64_t ws_bytes, void* stream);
int find_depth_loss_bwd(const float* pred, const float* target, const float* weight, int64_t n_img, int64_t n_pix, int kind, float delta, float trunc,
						const float* d_loss, const void* ws, float* d_pred, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SSIM (ssim.hip): structural similarity (Wang et al. 2004) of two image batches, the definition of pytorch-msssim / 3DGS with
 * data_range = L.  Not in the reference.  x, y (n_img, H, W, C) channel-last, C in 1 .. 4; xm, ym (n_img, H, W) or NULL (= 1);
 * a = x * xm, b = y * ym.  Window: separable Gaussian, 11 taps, sigma 1.5, normalised in double, fp32 constants.  Per pixel and channel,
 * with the window means m1 = E[a], m2 = E[b], s11 = E[a^2], s22 = E[b^2], s12 = E[ab], C1 = (0.01 L)^2, C2 = (0.03 L)^2:
 *     ssim = (2 m1 m2 + C1)(2 (s12 - m1 m2) + C2) / ((m1^2 + m2^2 + C1)((s11 - m1^2) + (s22 - m2^2) + C2)).
 * valid == 0 ("same"): the window is zero-padded at the border and an image's value is the mean over its H W C values; valid != 0: the mean
 *   over the (H - 10)(W - 10) C values whose window lies inside the image (H, W >= 11).  Nothing outside the image is read.
 * find_ssim_ws_bytes: want_grad == 0: the bytes of `ws` (a double per 16 x 16 tile); want_grad != 0: the bytes of `dmaps`
 *   (n_img H W 3 C floats).  -1 for bad sizes (non-positive, C > 4, more than 65535 images, H or W above 32768).
 * find_ssim_fwd: *mean_out = the mean over images of the per-image values; per_image (n_img) fp64 or NULL.  Moments and sums in double, a
 *   partial per tile, added in a fixed order: no atomics, bit-identical on repeat.  dmaps or NULL: what the backward needs, (n_img, C, 3, H, W)
 *   fp32: d ssim / d (m1, s11, s12) of every pixel scaled by 1 / (n_img * values per image), 0 where a pixel does not count; all of it is written.
 * find_ssim_bwd: g: one fp32 on the device, d loss / d mean.  d_x (as x) and d_xm (as xm; needs xm), either may be NULL, are OVERWRITTEN,
 *   every element: with d a(q) = sum_p w(p - q) [A1(p) + 2 a(q) A2(p) + b(q) A3(p)],  d_x = xm d a g,  d_xm = sum_c x_c d a_c g.  One launch, no
 *   atomics.  y and ym receive no gradient.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_ssim_ws_bytes(int64_t n_img, int64_t H, int64_t W, int64_t C, int want_grad);
int find_ssim_fwd(const float* x, const float* xm, const float* y, const float* ym, int64_t n_img, int64_t H, int64_t W, int64_t C, float L, int valid,
				  float* mean_out, double* per_image, float* dmaps, void* ws, int64_t ws_bytes, void* stream);
int find_ssim_bwd(const float* x, const float* xm, const float* y, const float* ym, int64_t n_img, int64_t H, int64_t W, int64_t C, float L, int valid,
				  const float* g, const float* dmaps, float* d_x, float* d_xm, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Foot measurements (measure.hip): sections of meshes by planes and extents along directions.  Not in the reference.
 * verts (N, V, 3); faces (faces_batch, F, 3) int32, faces_batch 1 (shared) or N (per mesh, rows of -1 pad the shorter ones), as
 * find_point_face_fwd; planes (planes_batch, P, 4) rows (nx, ny, nz, d), planes_batch 1 or N, 1 <= P <= 64.  The normal is taken as
 * given (the caller normalises it).  The rule, per mesh and plane:
 *   s = fmaf(nz, z, fmaf(ny, y, nx * x)) - d per vertex, "above" iff s >= 0; a face crosses iff its three vertices are not all on one side,
 *   and then exactly two of its edges cross; on a crossing edge, lo the vertex below and hi the one above, t = s_lo / (s_lo - s_hi) (the
 *   denominator is < 0) and p = fmaf(t, hi - lo, lo); the face contributes |p1 - p2|.  A face with a -1, an index outside [0, V) or a
 *   repeated vertex contributes nothing.  So a closed mesh gives closed loops, an edge lying in the plane is counted once (by the face on
 *   its lower side), a face lying in the plane contributes nothing, and a plane touching the mesh at one vertex gives crossing faces of
 *   length 0.
 * find_plane_sections_fwd: perimeter (N, P) fp32 the summed lengths, count (N, P) int32 the crossing faces.  One pass over the faces serves
 *   all planes; fp32 per face, the sums in double: a partial per workgroup of 256 faces and plane, added by a second kernel in workgroup
 *   order.  No float atomics: bit-identical on repeat, and a mesh's row does not depend on the rest of the batch.
 *   ws: find_plane_sections_ws_bytes(N, F, P, 0) bytes, 8-byte aligned, free again when the call's work is done.
 * find_plane_sections_bwd: from g (N, P): d_verts (N, V, 3) OVERWRITTEN, every element, the plain chain rule through p, t and s.  The face
 *   pass writes the nine corner gradients of every face (summed over the planes in plane order; zeros for a face that crosses none), a
 *   second kernel adds them per vertex through vf_off (faces_batch, V + 1) / vf_items (faces_batch, 3 F), the corner table of
 *   find_vertex_normals_fwd, in the table's order.  d_offset (planes_batch, P) or NULL: the gradient of the offsets d, through a double
 *   partial per workgroup, added in workgroup order and -- planes_batch 1 -- over the meshes in mesh order.  A segment of length 0 gives
 *   a zero gradient.  The plane NORMALS receive no gradient.  ws: find_plane_sections_ws_bytes(N, F, P, 1) bytes (N F 9 floats and the
 *   partials), 8-byte aligned.
 * find_plane_sections_ws_bytes: -1 for bad sizes (N, F < 1, P outside 1 .. 64, N >= 65536, F >= 2^24, N F >= 2^32).
 * find_extents_fwd: dirs (D, 3) fp32 on the device, 1 <= D <= 8; v_len (N) int32 or NULL (= V).  lo, hi (N, D): min and max of
 *   fmaf(dz, z, fmaf(dy, y, dx * x)) over the first v_len[n] vertices, arg_lo, arg_hi (N, D) int32 where they are taken: among equal
 *   values the smallest index.  v_len[n] == 0: 0, 0, -1, -1.  Rows at or past v_len[n] are never read.  A workgroup per mesh.
 * find_extents_bwd: d_verts (N, V, 3) is ADDED INTO (zero-initialise it): g_lo[n, d] dir_d at arg_lo[n, d] and g_hi[n, d] dir_d at
 *   arg_hi[n, d], a thread per mesh in the order lo_0, hi_0, lo_1, ...; g_lo or g_hi may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_plane_sections_ws_bytes(int64_t N, int64_t F, int64_t P, int backward);
int find_plane_sections_fwd(const float* verts, const int32_t* faces, int64_t faces_batch, const float* planes, int64_t planes_batch, int64_t N,
							int64_t V, int64_t F, int64_t P, float* perimeter, int32_t* count, void* ws, int64_t ws_bytes, void* stream);
int find_plane_sections_bwd(const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* vf_off, const int32_t* vf_items,
							const float* planes, int64_t planes_batch, int64_t N, int64_t V, int64_t F, int64_t P, const float* g, float* d_verts,
							float* d_offset, void* ws, int64_t ws_bytes, void* stream);
int find_extents_fwd(const float* verts, const int32_t* v_len, const float* dirs, int64_t N, int64_t V, int64_t D, float* lo, float* hi,
					 int32_t* arg_lo, int32_t* arg_hi, void* stream);
int find_extents_bwd(const float* g_lo, const float* g_hi, const int32_t* arg_lo, const int32_t* arg_hi, const float* dirs, int64_t N,
					 int64_t V, int64_t D, float* d_verts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tape girths (girth.hip): the perimeter of the convex hull of a plane section.  Not in the reference.  verts, faces, planes as above; the
 * points of (mesh, plane) are the crossing points of the section rule above, two per crossing face: edge 0 joins the face's lone vertex L
 * (corner k) to corner k + 1, edge 1 to corner k + 2; id = 2 face + edge.  The two faces of a mesh edge give the same bits.
 *   The hull is taken in the plane's 2-D coordinates (x, y) = (p . e1, p . e2), each fmaf(e_z, p_z, fmaf(e_y, p_y, e_x * p_x)) in fp32, with
 *   a the coordinate axis of the smallest |n_k| (lowest index on ties), e1 = normalize(n x a), e2 = n x e1.  Corners are strict: points
 *   identical in (x, y) count once, owned by the smallest id; of points collinear with a hull edge only its end points are corners.  The
 *   orientation predicate is evaluated in double on the fp32 coordinates.  The corners run counter-clockwise (seen against e1 x e2 = n) from
 *   the point of the smallest (x, y, id).
 * find_section_hull_fwd: girth (N, P) fp32 the sum of the 3-D distances |p_i - p_i+1| around the loop, each fp32, summed in double in a
 *   fixed order; two distinct points give 2 |p1 - p2|, one or none 0.  count (N, P) int32 the crossing faces (as find_plane_sections_fwd),
 *   n_hull (N, P) int32 the corners, status (N, P) int32: bit 1 more than max_points crossing faces, bit 2 the walk did not close within
 *   one step per point; a status != 0 gives girth 0 and n_hull 0.  hull_ids (N, P, 2 max_points) int32: the first n_hull entries are the
 *   corners' ids in order, the rest is not written.  hull_points (N, P, max_hull, 3) or NULL (max_hull 0): the corners' points in order,
 *   zeros past n_hull, truncated at max_hull (<= 2 max_points).  One workgroup per (mesh, plane) compacts its crossing faces in face order and
 *   walks the hull, on chip up to 2048 points and from the workspace beyond.  No atomics: bit-identical on repeat, and a mesh's row does not
 *   depend on the rest of the batch.  ws: find_section_hull_ws_bytes(N, F, P, max_points, 0) bytes, 8-byte aligned.
 * find_section_hull_bwd: from g (N, P), n_hull and hull_ids: d_verts (N, V, 3) OVERWRITTEN, every element; d_planes (planes_batch, P, 4) or
 *   NULL, all four components (ds / dn = v, ds / dd = -1; the normal is not renormalised), for planes_batch 1 summed over the meshes in
 *   mesh order.  A corner p between a and b receives g ((p - a) / |p - a| + (p - b) / |p - b|), a zero distance masked; the sums into a
 *   vertex run in plane order, then corner order.  ws: find_section_hull_ws_bytes(N, F, P, max_points, 1) bytes.
 * find_section_hull_ws_bytes: -1 for bad sizes (as find_plane_sections_ws_bytes, and max_points outside 1 .. F).
 * ---------------------------------------------------------------------------------------------- */
int64_t find_section_hull_ws_bytes(int64_t N, int64_t F, int64_t P, int64_t max_points, int backward);
int find_section_hull_fwd(const float* verts, const int32_t* faces, int64_t faces_batch, const float* planes, int64_t planes_batch, int64_t N,
						  int64_t V, int64_t F, int64_t P, int64_t max_points, int64_t max_hull, float* girth, int32_t* count, int32_t* n_hull,
						  int32_t* status, int32_t* hull_ids, float* hull_points, void* ws, int64_t ws_bytes, void* stream);
int find_section_hull_bwd(const float* verts, const int32_t* faces, int64_t faces_batch, const float* planes, int64_t planes_batch, int64_t N,
						  int64_t V, int64_t F, int64_t P, int64_t max_points, const float* g, const int32_t* n_hull, const int32_t* hull_ids,
						  float* d_verts, float* d_planes, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rigid and similarity alignment of point clouds (align.hip).  Not in the reference; stands in for
 * pytorch3d.ops.corresponding_points_alignment and iterative_closest_point.  Row vectors: x' = s (x @ R) + t, R (n, 3, 3) row-major.
 * No allocation, no host synchronisation and no float atomics in either call; every sum is taken in double in a fixed order (256 pairs per
 * workgroup: lanes by butterfly, waves in wave order, workgroups in workgroup order), so two runs agree bit for bit and a cloud's row does
 * not depend on the rest of the batch.  status (n) int32: 0, or the sum of FIND_ALIGN_MAX_ITERATIONS (1) and FIND_ALIGN_DEGENERATE (2).
 * find_align_fit: Umeyama / Kabsch on the pairs (x[n, i], y[n, i]), i < len[n] (len NULL: p_max), of weight w[n, i] (w NULL: 1; a weight
 *   that is not > 0 and finite counts as 0, and such a pair is never read).  The minimiser of sum w |s (x @ R) + t - y|^2: the centred
 *   cross-covariance H = sum w (x - mu_x)^T (y - mu_y) = U D V^T (3 x 3 SVD by one-sided Jacobi rotations in double), R = U diag(1, 1, e) V^T
 *   with e = det(U) det(V) -- e = 1 if allow_reflection --, s = trace(D diag(1, 1, e)) / sum w |x - mu_x|^2 if estimate_scale, else 1,
 *   t = mu_y - s mu_x R.  R, t, s are rounded to fp32 once, at the end.  Fewer than 3 pairs of positive weight, or an H whose second singular
 *   value is <= 1e-12 of its first (rank < 2; with estimate_scale also an x without spread): identity, t = 0, s = 1, status 2; never NaN.
 *   Precision: the moments are taken about the cloud's first pair (x[n, 0], y[n, 0]) as pivots, in double, so the covariance loses
 *   |mu - pivot|^2 / sigma^2 * 2^-53 relative, whatever the cloud's distance from the origin.
 *   ws: find_align_ws_bytes(n, p_max) bytes, 8-byte aligned (-1 for bad sizes: n, p_max < 1, n >= 65536, p_max >= 2^24, n p_max >= 2^31).
 * find_icp_run: trimmed ICP from x (n, p1_max, 3) / x_len to y (n, p2_max, 3) / y_len, the whole loop enqueued on `stream` by one call.
 *   From init_R (n, 3, 3), init_t (n, 3), init_s (n) -- all three or all NULL (identity) --, max_iterations + 1 rounds of:
 *     apply    xt = fmaf(s, fmaf(x2, R[2][j], fmaf(x1, R[1][j], x0 * R[0][j])), t[j]) in fp32 (rows past x_len: zeros);
 *     match    find_nn_fwd(xt, y): dist = d2, idx (lowest index on ties; padding rows as find_nn_fwd leaves them: 0 / -1);
 *     select   (trim > 0) tau = the exact k-th smallest d2 among the cloud's m = x_len valid queries, k = m - floor(trim m), by a radix
 *              select over the floats' bit patterns; a pair is USED iff d2 <= tau (ties at tau all count) and d2 <= max_dist^2
 *              (fp32 product; max_dist = INFINITY: no limit).  trim == 0: tau = +inf;
 *     solve    rmse = sqrt(sum d2 / count) over the used pairs (0 without any) -- the rmse of the transform the match used.  A cloud
 *              whose |rmse_prev - rmse| <= rel_tol rmse_prev has converged: its transform is left alone from then on (the later rounds
 *              still match it: wasted but harmless, there is no host round trip to skip them).  Otherwise, except in the last round,
 *              the fit above over (x[i], y[idx[i]]) of the used pairs replaces the transform: every round solves for the ABSOLUTE
 *              transform from the original x, so once the correspondences stop changing, transform and rmse repeat bit for bit.
 *              A degenerate fit leaves the transform, freezes the cloud the same way and sets status bit 2.
 *   So the returned xt, dist, idx, tau, used and rmse belong to the returned R, t, s.  iterations (n): the updates applied; status: 0 converged,
 *   1 stopped at max_iterations without, 2 degenerate.  used (n) int32: the pairs of the last round's sums.  Reflections are never allowed.
 *   ws: find_icp_ws_bytes(n, p1_max, p2_max) bytes, 8-byte aligned.  0 <= max_iterations <= 10000, rel_tol >= 0, 0 <= trim < 1, max_dist > 0.
 * ---------------------------------------------------------------------------------------------- */
#define FIND_ALIGN_MAX_ITERATIONS 1
#define FIND_ALIGN_DEGENERATE 2
int64_t find_align_ws_bytes(int64_t n, int64_t p_max);
int find_align_fit(const float* x, const float* y, const int32_t* len, const float* w, int64_t n, int64_t p_max, int estimate_scale,
				   int allow_reflection, float* R, float* t, float* s, int32_t* status, void* ws, int64_t ws_bytes, void* stream);
int64_t find_icp_ws_bytes(int64_t n, int64_t p1_max, int64_t p2_max);
int find_icp_run(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, int64_t n, int64_t p1_max, int64_t p2_max,
				 const float* init_R, const float* init_t, const float* init_s, int64_t max_iterations, double rel_tol, int estimate_scale,
				 double trim, float max_dist, float* R, float* t, float* s, float* rmse, int32_t* iterations, int32_t* status, float* xt,
				 float* dist, int32_t* idx, float* tau, int32_t* used, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The as-rigid-as-possible energy (arap.hip; Sorkine & Alexa 2007).  Not in the reference.  n deformed meshes verts (n, v, 3) against ONE rest
 * mesh rest (v, 3), over a vertex -> neighbour CSR nbr_off (v + 1) / nbr_idx (n_nbr) with a weight nbr_w (n_nbr) >= 0 per entry (symmetric:
 * w_ij = w_ji) and w_sum = the sum of all n_nbr weights (0: a mesh without edges, every result 0).  With e_q = rest_i - rest_j, e_p = verts_i - verts_j:
 *   S_i = sum_j w_ij e_q e_p^T = U D V^T (3 x 3 SVD by one-sided Jacobi rotations in double),  R_i = V diag(1, 1, det(V U^T)) U^T,
 *   energy[n] = (1 / w_sum) sum_i sum_j w_ij |e_p - R_i e_q|^2,   cell[n, i] = the i-th inner sum / w_sum,
 *   d_verts[n, i] = g[n] (2 / w_sum) sum_j w_ij [2 e_p - (R_i + R_j) e_q]   (the rotations held fixed: exact, they minimise the energy).
 * A cell without a unique rotation -- no neighbours, D_1 = 0, or D_2 <= 1e-12 D_1 -- takes R_i = I and is counted in degenerate[n]; never NaN.
 * find_arap_fwd writes R (n, v, 3, 3) in DOUBLE, row-major, for find_arap_bwd, which reads it and does not refit.  An entry of nbr_idx outside
 * [0, v) is skipped.  All arithmetic in double; no allocation, no host synchronisation, no atomics; every sum in a fixed order (the lanes of a
 * vertex by butterfly -- 4 in the forward, 8 in the backward --, 64 vertices per forward workgroup, workgroups in a strided fixed order), so two runs agree bit for bit and a mesh's values do
 * not depend on the rest of the batch.  Valence is not bounded.
 *   ws: find_arap_ws_bytes(n, v) bytes, 8-byte aligned (-1 for bad sizes: n, v < 1, n >= 65536, v >= 2^24, n v >= 2^31); only the forward needs it.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_arap_ws_bytes(int64_t n, int64_t v);
int find_arap_fwd(const float* verts, const float* rest, const int32_t* nbr_off, const int32_t* nbr_idx, const float* nbr_w, int64_t n, int64_t v,
				  int64_t n_nbr, double w_sum, double* R, float* cell, float* energy, int32_t* degenerate, void* ws, int64_t ws_bytes, void* stream);
int find_arap_bwd(const float* verts, const float* rest, const int32_t* nbr_off, const int32_t* nbr_idx, const float* nbr_w, int64_t n, int64_t v,
				  int64_t n_nbr, double w_sum, const double* R, const float* g, float* d_verts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Generalised winding numbers (winding.hip; Jacobson et al. 2013).  Not in the reference.  points (N, P, 3) with per-mesh counts p_len (N)
 * int32 (NULL = all P); verts (N, V, 3); faces (faces_batch, F, 3) int32, faces_batch 1 (shared) or N (per mesh, rows of -1 pad the shorter
 * ones), as find_point_face_fwd.  P = 0 and F = 0 are allowed.
 * find_winding_fwd: w (N, P) = sum over the faces of mesh n of Omega / 4 pi, with A = a - p, B = b - p, C = c - p formed in float32,
 *   det = A . (B x C) (every product rounded on its own), den = |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|, Omega = 2 atan2f(det, den).
 *   Exactly 0, never NaN: a -1 row, a face with an index outside [0, V), a face with a corner at the query, a face with det == 0.  Rows at
 *   or past p_len[n], and a mesh without such a face, get 0.  No gradient.  The sum is in double, without atomics, in an order that depends
 *   on F alone: faces in runs of 128 in face order, eight runs to a chunk of 1024 faces, the chunks in order (csrc/winding_math.h:
 *   ordered_sum).  Two runs agree bit for bit; a row does not depend on N, P or its position, nor on whether the chunks went to workgroups
 *   of their own (they do when ceil(P / 128) N < 2048 and 2 <= ceil(F / 1024) <= 64; never under bit 8192 of find_render_switches).
 *   ws: find_winding_ws_bytes(N, P, F) bytes, 8-byte aligned (-1 for bad sizes: N >= 65536, P, F >= 2^30), free again when the call's work
 *   is done.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_winding_ws_bytes(int64_t n_meshes, int64_t n_points, int64_t n_faces);
int find_winding_fwd(const float* points, const int32_t* p_len, const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes,
					 int64_t n_points, int64_t n_verts, int64_t n_faces, float* w, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ray casting (raycast.hip; the watertight test of Woop, Benthin & Wald 2013).  Not in the reference.  origins, dirs (N, R, 3) with per-mesh
 * counts r_len (N) int32 (NULL = all R); skip (N, R) int32 (NULL = none): a face the ray never hits (the face its origin lies on); verts,
 * faces, faces_batch as find_winding_fwd.  R = 0 and F = 0 are allowed.  d need not be normalised: t is in units of |d|.
 * The pair test, every product and sum rounded on its own in the order of csrc/raycast_math.h (which tests/rays_ref.py restates):
 *   per ray   kz = argmax |d| (the first of equals), kx, ky the next two axes in cyclic order, swapped if d[kz] < 0;
 *             e1 = axis(kx) - (d[kx] / d[kz]) axis(kz), e2 = axis(ky) - (d[ky] / d[kz]) axis(kz), dd = d . d
 *   per corner P = p - o, x = (P0 e1_0 + P1 e1_1) + P2 e1_2, y likewise with e2: the same bits in every face that uses the vertex
 *   per pair  U = cx by - cy bx, V = ax cy - ay cx, W = bx ay - by ax, det = (U + V) + W; inside: all three >= 0 or all three <= 0, det != 0;
 *             t = ((U za + V zb) + W zc) / (det dd) with z = P . d; barycentrics (U, V, W) / det; a hit: t_min < t <= t_max, t finite.
 *   Never a hit: a -1 row, a face with an index outside [0, V), a face with a corner at the origin (P == 0), the ray's skip face, a ray with a
 *   non-finite component or d == 0.  Among equal t the smallest face index wins.  A computed sign is right or zero, and a zero is inside:
 *   a ray through a shared edge or a vertex of a closed mesh hits; there is no double-precision fallback.
 * find_ray_fwd, any_hit = 0: t (N, R), idx (N, R) int32, bary (N, R, 3); a miss, and a row at or past r_len, gives +inf, -1, 0 0 0.  hit may
 *   be NULL.  any_hit = 1: hit (N, R) uint8 alone, equal to isfinite(t) of the other call; t, idx, bary may be NULL.  Every row is written.
 *   Results are 64-bit keys (t bits << 32 | face) merged by integer minimum, no float atomics: two runs agree bit for bit, and a row does not
 *   depend on N, R, its position, nor on whether the face range was split over workgroups (it is, in up to 16 pieces of at least 1024 faces,
 *   while ceil(R / 128) N pieces < 1024; never under bit 8192 of find_render_switches).  t_min >= 0 is required.
 *   ws: find_ray_ws_bytes(N, R, F) bytes, 8-byte aligned (-1 for bad sizes: N >= 65536, R, F >= 2^30), free again when the call's work is done.
 * find_ray_bwd: with n = (b - a) x (c - a), g = n . d, w the stored barycentrics: d_origins = -d_t n / g, d_dirs = -d_t t n / g, both
 *   (N, R, 3), OVERWRITTEN in every row (0 for a miss); d_verts (N, V, 3) += d_t w_i n / g at the hit face's corners, with float atomics into a
 *   buffer the CALLER ZEROED (the contract of find_point_face_bwd).  The face and the barycentrics are constants.  Any of the three may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int64_t find_ray_ws_bytes(int64_t n_meshes, int64_t n_rays, int64_t n_faces);
int find_ray_fwd(const float* origins, const float* dirs, const int32_t* r_len, const int32_t* skip, const float* verts, const int32_t* faces,
				 int64_t faces_batch, int64_t n_meshes, int64_t n_rays, int64_t n_verts, int64_t n_faces, float t_min, float t_max, int any_hit,
				 float* t, int32_t* idx, float* bary, uint8_t* hit, void* ws, int64_t ws_bytes, void* stream);
int find_ray_bwd(const float* origins, const float* dirs, const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* idx,
				 const float* bary, const float* t, const float* d_t, int64_t n_meshes, int64_t n_rays, int64_t n_verts, int64_t n_faces,
				 float* d_origins, float* d_dirs, float* d_verts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A bounding-volume hierarchy for ray queries (bvh.hip, csrc/bvh_math.h).  Not in the reference.  verts, faces, faces_batch as find_ray_fwd.
 * The structure is opaque: find_bvh_bytes(N, F) bytes (-1 for bad sizes: N >= 65536, F >= 2^30, a negative size), 256-byte aligned, a
 * function of N and F alone.  Per mesh it holds the faces' order (int32) and one box per node of an implicit, complete 4-ary tree over
 * leaves of FIND_BVH_LEAF faces in that order, the leaf count padded to a power of 4 with empty boxes; child and parent indices are computed,
 * and every face index taken from it is range-checked, so a call on a stale or overwritten structure gives wrong answers and never a fault.
 * A face is INVALID -- never hit, in no box -- if it is a -1 row, has an index outside [0, V), or a non-finite corner (find_ray_fwd leaves
 * the last to the pair test); validity is decided from verts and faces at every call, not stored.
 * find_bvh_keys: keys (N, F) uint64, morton << 32 | face: the 30-bit Morton code of the face's centroid on the box of the mesh's valid
 *   centroids (an axis without extent: 0); an invalid face has the high word 0x7fffffff, so every key is below 2^63 and a signed 64-bit sort
 *   orders the rows as an unsigned one does.  The head of the structure is its scratch.  No atomics.
 * The CALLER sorts each row of keys ascending (any correct 64-bit sort: the keys of a row are distinct); the library does not sort.
 * find_bvh_build: stores the order of the sorted keys and forms every box from verts, bottom-up, without atomics.
 * find_bvh_refit: forms every box again from other verts (same faces, same sizes) with the stored order: no keys, no sort.  The order decides
 *   only which faces share a box: results after a refit are exact however far the vertices moved.
 * find_ray_bvh_fwd: find_ray_fwd's arguments, outputs, workspace (find_ray_ws_bytes) and rules, with the structure: a lane walks the tree
 *   per ray and runs find_ray_fwd's pair test, on the same operands, on the faces of the leaves it reaches; a box is skipped only when no
 *   pair in it can be accepted (bvh_math.h derives the margin), an equal t on a smaller face still wins, and the result does not depend on
 *   the order of the walk: t, idx, bary and hit equal find_ray_fwd's bit for bit, except that a face with a non-finite corner is never hit.
 *   any_hit = 1 stops a ray at its first accepted pair.  No atomics; the face range is never split.  bvh may be NULL when F = 0.
 * ---------------------------------------------------------------------------------------------- */
#define FIND_BVH_LEAF 4
#define FIND_BVH_ARITY 4
int64_t find_bvh_bytes(int64_t n_meshes, int64_t n_faces);
int find_bvh_keys(const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts, int64_t n_faces, uint64_t* keys,
				  void* bvh, int64_t bvh_bytes, void* stream);
int find_bvh_build(const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts, int64_t n_faces,
				   const uint64_t* sorted_keys, void* bvh, int64_t bvh_bytes, void* stream);
int find_bvh_refit(const float* verts, const int32_t* faces, int64_t faces_batch, int64_t n_meshes, int64_t n_verts, int64_t n_faces, void* bvh,
				   int64_t bvh_bytes, void* stream);
int find_ray_bvh_fwd(const float* origins, const float* dirs, const int32_t* r_len, const int32_t* skip, const float* verts, const int32_t* faces,
					 int64_t faces_batch, int64_t n_meshes, int64_t n_rays, int64_t n_verts, int64_t n_faces, float t_min, float t_max, int any_hit,
					 float* t, int32_t* idx, float* bary, uint8_t* hit, const void* bvh, int64_t bvh_bytes, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Iso-surface extraction by surface nets (surface_nets.hip; Gibson 1998).  Not in the reference.  values (N, nx, ny, nz) float32, sample
 * (i, j, k) at flat index (i ny + j) nz + k, every axis 2 .. 1024 samples, one `iso` per call.
 *   Sides: a sample is inside iff value < iso, compared exactly, and the value is finite (value == iso, NaN, +-inf: outside).
 *   Cells: cell (i, j, k) covers samples i..i+1, j..j+1, k..k+1, flat index (i (ny-1) + j) (nz-1) + k; corner c = 4 di + 2 dj + dk; the 12
 *     edges (a, b), a < b, join corners that differ in one bit, in lexicographic order; a cell is active iff its corners are not all on one side.
 *   Vertex: on a crossing edge t = (iso - v_a) / (v_b - v_a) in float32 (0.5 if not finite), p = corner_a + t (corner_b - corner_a);
 *     g = (i, j, k) + (sum of p in edge order) / n, n the number of crossing edges: GRID coordinates (the caller forms
 *     origin + (g + 0.5) spacing).  Vertices are numbered in flat cell order.
 *   Faces: lattice edges in flat sample order, per sample +x, +y, +z.  The edge along ax from sample s emits a quad iff its ends differ in
 *     side and 1 <= s_u <= n_u - 2, 1 <= s_w <= n_w - 2 for u = (ax+1) % 3, w = (ax+2) % 3: the vertices of the cells s + du e_u + dw e_w,
 *     (du, dw) = (-1,-1), (0,-1), (0,0), (-1,0), reversed if s is not inside; triangles (q0, q1, q2), (q0, q2, q3).  Normals point outside.
 *   status (N) int32: 1 an active cell in the outermost cell layer (the mesh is open there); 2 / 4 vertex / face capacity exceeded; 8 a
 *     non-finite sample.  Closed away from the grid boundary; 2-manifold only where no lattice face has four sign changes.
 * find_surface_nets_count writes n_verts, n_faces (N) int64 and status (bits 1 and 8), and leaves the per-block counts (blocks of
 *   FIND_SURFACE_NETS_BLOCK samples / cells) and their exclusive scans in ws.
 * find_surface_nets_emit, with the SAME ws and the counts of the count call: g (N, vcap, 3) float32, faces (N, fcap, 3) int32, the
 *   cell -> vertex map (N, cells) int32 (-1: no vertex) at the START of ws, and bits 2 / 4 of status.  Rows at or past a mesh's count: 0 (g),
 *   -1 (faces).  Nothing at or past vcap / fcap is written; on overflow the counts stay the true ones and that mesh's rows are unspecified.
 * find_surface_nets_bwd: grad_values (N, nx, ny, nz) and grad_iso (N) float32 from grad_g (N, vcap, 3) = d L / d g and the map: one gather
 *   per sample; d = v_b - v_a, dt/dv_a = (iso - v_b) / d^2, dt/dv_b = -(iso - v_a) / d^2, dt/diso = 1 / d, n constant; grad_iso is summed
 *   in double in a fixed order.  Vertices at or past vcap have no gradient.
 * No atomics anywhere; two runs agree bit for bit; a mesh's output depends on its own grid alone.  ws: find_surface_nets_ws_bytes /
 *   find_surface_nets_bwd_ws_bytes(N, nx, ny, nz) bytes, 8-byte aligned (-1 for bad sizes: N >= 65536, an axis outside 2 .. 1024).
 * ---------------------------------------------------------------------------------------------- */
#define FIND_SURFACE_NETS_BLOCK 256
int64_t find_surface_nets_ws_bytes(int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz);
int64_t find_surface_nets_bwd_ws_bytes(int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz);
int find_surface_nets_count(const float* values, float iso, int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz, int64_t* n_verts, int64_t* n_faces,
							int32_t* status, void* ws, int64_t ws_bytes, void* stream);
int find_surface_nets_emit(const float* values, float iso, int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz, const int64_t* n_verts,
						   const int64_t* n_faces, int64_t vcap, int64_t fcap, float* g, int32_t* faces, int32_t* status, void* ws, int64_t ws_bytes,
						   void* stream);
int find_surface_nets_bwd(const float* values, float iso, int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz, const int32_t* cellmap,
						  const float* grad_g, int64_t vcap, float* grad_values, float* grad_iso, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused multi-tensor optimiser steps. Replace torch.optim.Adam / torch.optim.SGD(momentum=0.9)
 * as constructed by the reference (src/train/train.py:161-168) and stepped once per batch
 * (src/train/trainer.py:121-123).  `param`, `grad`, moment arrays: HOST arrays of n_tensors DEVICE pointers (fp32,
 * contiguous); `numel`: host array.  Dense updates, torch's single-tensor arithmetic operation for operation;
 * amsgrad / maximize / foreach-only options are not provided.
 * find_adam_step, find_sgd_step: hyper-parameters are doubles, as torch's Python floats are, and each is rounded to fp32 once, where
 * torch rounds it: 1 - beta1, 1 - beta2, 1 - dampening and lr / bias_correction1 are formed in double first.  A tensor with numel == 0
 * is accepted and skipped: its pointers (param, grad, moments) may be NULL, as the data_ptr() of a 0-element device tensor is.  For every
 * other tensor a NULL pointer is refused.  All tensors and hyper-parameters are checked before the first launch: a call that returns an
 * error has updated nothing.
 * find_adam_step: `step` is the 1-based count INCLUDING this update (torch's state['step'] after it).
 * find_sgd_step: `first_step` != 0 initialises the momentum buffers to the gradient (torch clones it, dampening ignored).
 * ---------------------------------------------------------------------------------------------- */
int find_adam_step(int64_t n_tensors, float* const* param, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
				   const int64_t* numel, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void* stream);
 /* find_adam_step_dev: the same update with the step count on the DEVICE -- `step_dev` points to one fp32 holding the 1-based count
 * including this update (the caller increments it on `stream` first), and the bias corrections are formed on the device in fp32, as
 * torch.optim.Adam(capturable=True) does: nothing step-dependent is baked into the launch, so the call can be captured in a HIP graph
 * and replayed (find_amd/graph.py).  This entry point still takes fp32 hyper-parameters and forms 1 - beta in fp32, refuses a NULL pointer
 * whatever the tensor's numel, and checks the tensors launch by launch (48 at a time). */
int find_adam_step_dev(int64_t n_tensors, float* const* param, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
					   const int64_t* numel, float lr, float beta1, float beta2, float eps, float weight_decay, const float* step_dev, void* stream);
int find_sgd_step(int64_t n_tensors, float* const* param, const float* const* grad, float* const* momentum_buf, const int64_t* numel,
				  double lr, double momentum, double dampening, double weight_decay, int nesterov, int first_step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FIND_HIP_H */
