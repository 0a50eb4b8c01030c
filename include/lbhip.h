/*
 * lbhip.h - C ABI of liblbhip.so: the MI355X (gfx950) rollout engine that sits behind
 * LagrangeBench's case_setup / models.GNS / evaluate.rollout Python API.
 *
 * The reference (tumaer/lagrangebench) is pure Python/JAX and has no FFI of its own; each
 * entry point below replaces the reference function named in its comment (paths relative to
 * the reference repo root).  A maintainer binds them with ctypes - see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer suffixed _dev is DEVICE memory owned by the caller (e.g. a torch tensor);
 *     the library owns only its opaque handles and internal scratch.
 *   - all work is enqueued on the hipStream_t given to lb_engine_create(); only the calls
 *     documented as "host-synchronous" block.
 *   - return value: 0 = LB_OK, < 0 = error (lb_strerror()).  Neighbor-list overflow is NOT an
 *     error: like the reference (evaluate/rollout.py:134-151) it is a flag the driver polls.
 *   - positions/targets are fp64 (the reference's default dtype, defaults.py:22); network
 *     inputs/outputs are fp32 (runner.py:71-72).  Indices are int32.
 *   - B independent trajectories ("batch", the reference's vmap axis rollout.py:226-228) of
 *     N particles each are processed as one disjoint graph of B*N nodes.
 */
#ifndef LBHIP_H
#define LBHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LB_OK 0
#define LB_ERR_ARG (-1)         /* bad argument / unsupported configuration            */
#define LB_ERR_HIP (-2)         /* a HIP runtime call failed (message via lb_strerror) */
#define LB_ERR_STATE (-3)       /* call order violated (e.g. update before allocate)   */
#define LB_ERR_DENSITY (-4)     /* a cell stencil / row exceeds the LDS tile bounds    */
#define LB_ERR_UNSUPPORTED (-5) /* valid in the reference, not built yet               */

#define LB_FORCE_NONE 0
#define LB_FORCE_PIECEWISE 1 /* f = pos[axis] > split ? f_hi : f_lo (RPF body force, DAM gravity) */
#define LB_FORCE_BUFFER 2    /* caller supplies (B,N,dim) fp64 every step via lb_set_force()       */

typedef struct lb_engine lb_engine;
typedef struct lb_gns lb_gns;

/* What case_builder(box, metadata, input_seq_length, cfg_neighbors, cfg_model, noise_std,
 * external_force_fn, dtype) closes over: case_setup/case.py:62-140.  Normalisation stats are the
 * OUTPUT of get_dataset_stats (data/utils.py:9-45), i.e. noise already folded into std. */
typedef struct lb_case_desc {
  int32_t dim;          /* 2 or 3 */
  int32_t n_particles;  /* N per trajectory (metadata["num_particles_max"]) */
  int32_t batch;        /* B trajectories advanced together */
  int32_t isl;          /* input_seq_length (>= 2) */
  int32_t periodic;     /* any(metadata["periodic_boundary_conditions"]) - case.py:104-108 */
  int32_t has_bound;    /* "bound" node feature: not any(pbc) - features.py:87-103 */
  int32_t has_vel_mag;  /* cfg_model.magnitude_features - features.py:80-85 */
  int32_t force_kind;   /* LB_FORCE_* : external_force_fn - features.py:105-107 */
  int32_t force_axis;
  int32_t geometry_f32; /* dtype of case_builder (case.py:169): 0 float64 (default), 1 float32 - buffers stay fp64, every
                         * value is float-representable and every arithmetic result is rounded to float */
  double box[3];
  double r_cutoff;      /* metadata["default_connectivity_radius"] */
  double capacity_multiplier; /* cfg_neighbors.multiplier */
  double vel_mean[3], vel_std[3], acc_mean[3], acc_std[3];
  double bound_lo[3], bound_hi[3]; /* metadata["bounds"] */
  double force_split;
  double force_lo[3], force_hi[3];
} lb_case_desc;

/* GNS hyper-parameters: models/gns.py:36-63 (runner.py:205-216). */
typedef struct lb_gns_desc {
  int32_t latent_size;        /* 128 (GNS-10-128); any multiple of 16 up to 128 (GNS-5-64) runs zero-padded */
  int32_t blocks_per_step;    /* num_mlp_layers >= 1 (models/utils.py:100-115); 2 = the fused kernels, other depths
                               * run one Linear per launch (csrc/lb_gns_generic.hip) */
  int32_t num_mp_steps;
  int32_t embedding_size;     /* particle_type_embedding_size (16) */
  int32_t num_particle_types; /* NodeType.SIZE = 9; <= 1 disables the embedding */
  int32_t node_in;            /* feature width WITHOUT the embedding: K*dim [+K] [+2dim] [+dim] */
  int32_t edge_in;            /* dim + 1 */
  int32_t out_dim;            /* particle_dimension */
} lb_gns_desc;

const char* lb_strerror(int code);
const char* lb_last_error(void);
int lb_version(void);

/* ---- engine / state ------------------------------------------------------------------ */

/* case_builder(...) - case_setup/case.py:62.  stream = hipStream_t (NULL = default stream). */
int lb_engine_create(const lb_case_desc* desc, void* hip_stream, lb_engine** out);
void lb_engine_destroy(lb_engine* eng);

/* sample[1] of the reference's (pos, particle_type) tuple: (B,N) int32.
 * Padded trajectories (data/data.py:183-197, case_setup/case.py:180-190: variable particle counts, the `matscipy` backend):
 * a particle of type -1 (NodeType.PAD_VALUE) is NOT THERE for the neighbor search - it is binned into no cell, is never a
 * sender or a receiver, has no self-edge, and counts towards no cell occupancy, edge count or capacity.  It is kinematic
 * (lb_integrate / lb_rollout write its target position, 0 in a padded dataset), its node rows are computed (finite,
 * deterministic, read by no edge) and it is outside the training loss, whose denominator is the non-kinematic real
 * particles of its trajectory.  Pads may sit anywhere in a trajectory and their number may differ between trajectories.
 * Also counts the live particles per trajectory (asynchronous, on the engine's stream).  With no particle of type -1
 * every call computes what it did before this was added, bit for bit. */
int lb_set_particle_type(lb_engine* eng, const int32_t* ptype_dev);

/* LB_FORCE_BUFFER only: (B,N,dim) fp64 = vmap(external_force_fn)(most_recent_position). */
int lb_set_force(lb_engine* eng, const double* force_dev);

/* Load the position window sample[0][:, t0:t0+isl] from a (B,N,T,dim) fp64 trajectory
 * (the layout H5Dataset.get_trajectory returns, data/data.py:199-225) into the engine's SoA
 * ring, and reset the step counter to `step` (normally 0).  rollout.py:113. */
int lb_load_window(lb_engine* eng, const double* traj_dev, int32_t T, int32_t t0, int32_t step);

/* The input of one training step from a device-resident dataset, in ONE launch with no host arithmetic and no
 * host-to-device copy (csrc/lb_train_input.hip).  It replaces, for training samples, H5Dataset.get_window + numpy_collate
 * (data/data.py:227-257), add_gns_noise with its random walk (train/strats.py:12-83) and the noise and target part of
 * _preprocess / _compute_target (case_setup/case.py:142-178).
 *   pos_dev    [n_traj][seq_len][N][dim] positions in the file's dtype: float, or double when pos_is_f64 (the order of the
 *              H5 `position` arrays; a trajectory with fewer than N particles padded with zeros),
 *   ptype_dev  [n_traj][N] particle types (-1 on the pads),
 *   traj_host, t0_host, slot_host: B entries each, HOST memory, passed to the kernel by value (B <= LB_TRAIN_BATCH_MAX):
 *              sample b of the batch is frames [t0, t0 + T) of trajectory traj[b]; slot[b] is its number in the GLOBAL
 *              batch (data parallel: rank * local batch + b).
 * Per particle: the T frames are gathered and converted to fp64 exactly (to float first on a dtype=float32 engine,
 * case.py:169).  With noise_std != 0, N(0, 1) draws from Philox4x32-10 keyed by `seed`, counter (step, slot, particle,
 * draw / 4), Box-Muller in fp64 on u = (x + 0.5) * 2^-32 (cos then sin of each pair) are scaled by noise_std / sqrt(isl - 1)
 * and summed twice along the isl - 1 velocity slots; frame 0 gets no noise, every frame after isl - 1 the noise of frame
 * isl - 1, particles of type 1, 2 or -1 none; the noise is applied with the case's shift in fp64 on the box as given
 * (result rounded to float on a float32 engine).  With noise_std == 0 the frames are the data, unshifted, as on the host.
 * A slot's draws depend on (seed, step, slot, particle, velocity slot, component) only - not on B, on the sample's place
 * in the batch or on the rank.
 * Outputs, all device memory: traj_out (B,N,T,dim) fp64, the tensor lb_load_window takes; ptype_out (B,N) for
 * lb_set_particle_type; the targets of frames isl-2+unroll_steps ... isl+unroll_steps of traj_out, (B,N,dim) fp64 each:
 * normalised acceleration and velocity and the raw position, in float arithmetic on a float32 engine (operation for
 * operation what _compute_target does); want_normals_dev: null, or (B,N,isl-1,dim) fp64 receiving the raw draws (tests).
 * Asynchronous on the engine's stream; changes no engine state. */
#define LB_TRAIN_BATCH_MAX 128
int lb_train_batch(lb_engine* eng, const void* pos_dev, int32_t pos_is_f64, const int32_t* ptype_dev, int32_t n_traj,
                   int32_t seq_len, const int32_t* traj_host, const int32_t* t0_host, const int32_t* slot_host,
                   uint64_t seed, int64_t step, double noise_std, int32_t T, int32_t unroll_steps, double* traj_out_dev,
                   int32_t* ptype_out_dev, double* target_acc_dev, double* target_vel_dev, double* target_pos_dev,
                   double* want_normals_dev);

/* Copy the current window back out as (B,N,isl,dim) fp64 (oldest frame first). */
int lb_read_window(lb_engine* eng, double* win_out_dev);

/* ---- neighbor list: jax_sph.jax_md.partition.neighbor_list (3rd party) ----------------
 * constructed case.py:120-130; used .allocate case.py:184-186, .update case.py:188-190. */

/* neighbor_fn.allocate(most_recent_position): HOST-SYNCHRONOUS sizing.  Builds the list for the
 * current window's newest frame, then freezes cell_capacity = int(max cell occupancy * mult)
 * and E_cap = int(max_b occupancy_b * mult) (clamped like jax-md).  Outputs may be NULL. */
int lb_nl_allocate(lb_engine* eng, int32_t* cell_capacity_out, int32_t* e_cap_out,
                   int32_t* occupancy_out /* [B] host */);

/* Pin the frozen capacities explicitly (e.g. to mirror a reference NeighborList). */
int lb_nl_set_capacity(lb_engine* eng, int32_t cell_capacity, int32_t e_cap);

/* neighbors.update(most_recent_position): asynchronous rebuild with the frozen capacities.
 * Sets the per-trajectory did_buffer_overflow flags (read them with lb_nl_read_flags). */
int lb_nl_update(lb_engine* eng);

/* did_buffer_overflow per trajectory -> (B,) int32 device buffer (async copy). */
int lb_nl_read_flags(lb_engine* eng, int32_t* overflow_out_dev);

/* NeighborList.idx in the reference's format: (B, 2, E_cap) int32, row 0 receivers, row 1
 * senders, trajectory-local ids, padding = N (features.py:110).  Edge ORDER is the engine's
 * canonical one - sorted by (receiver, sender) - not jax-md's slot order.  n_edges_out_dev
 * (B,) int32 gets the real edge counts (may be NULL). */
int lb_nl_read_idx(lb_engine* eng, int32_t* idx_out_dev, int32_t* n_edges_out_dev);

/* ---- features: feature_transform - case_setup/features.py:47-126 ---------------------- */

/* Node features as fp64 in reference column order:
 *   vel_hist (B,N,K*dim) time-major; vel_mag (B,N,K) or NULL; bound (B,N,2*dim) or NULL;
 *   force (B,N,dim) or NULL. */
int lb_node_features(lb_engine* eng, double* vel_hist_out_dev, double* vel_mag_out_dev,
                     double* bound_out_dev, double* force_out_dev);

/* Edge features of the CURRENT list in lb_nl_read_idx order: rel_disp (B,E_cap,dim) and
 * rel_dist (B,E_cap,1) fp64.  Padded rows hold what the reference's clamped gather produces
 * (disp(pos[N-1], pos[N-1]) = 0). */
int lb_edge_features(lb_engine* eng, double* rel_disp_out_dev, double* rel_dist_out_dev);

/* ---- model: GNS - models/gns.py:35-171 ------------------------------------------------ */

/* Weights are fp32 HOST arrays in haiku layout (Linear w is (in,out) row-major), concatenated in
 * module creation order:
 *   [embed (types,emb)] then for each MLP in order enc_node, enc_edge, (proc_k_edge, proc_k_node)
 *   for k < num_mp_steps, decoder:  w0, b0, w1, b1, [ln_scale, ln_offset]  (decoder: no LN).
 * n_floats is the total length (checked). */
int lb_gns_create(lb_engine* eng, const lb_gns_desc* desc, const float* weights_host,
                  int64_t n_floats, lb_gns** out);
void lb_gns_destroy(lb_gns* gns);

/* model.apply(params, state, (features, particle_type)) -> {"acc": (B,N,dim) fp32}
 * (rollout.py:59) on the engine's current window and neighbor list. */
int lb_gns_forward(lb_engine* eng, lb_gns* gns, float* acc_out_dev);

/* 1 (default): jraph.segment_sum is fused into the edge-MLP epilogue (segmented wavefront scan,
 * no message round trip through HBM); 0: messages are written out and reduced by the stand-alone
 * segment_sum kernel (lb_segment_sum's kernel).  Both are deterministic and atomic-free. */
int lb_set_fused_aggregation(lb_engine* eng, int32_t on);

/* Debug/parity taps: node latents after the encoder and after each MP step
 * ((num_mp_steps+1), B*N, latent) fp32, or NULL. */
int lb_gns_set_tap(lb_gns* gns, float* node_latents_out_dev);

/* ---- integrator + driver -------------------------------------------------------------- */

/* _forward_eval minus the model call - rollout.py:61-73 with case.integrate (case.py:230-259):
 * next = shift(p[-1], disp(p[-1], p[-2]) + acc_mean + acc*acc_std); kinematic particles
 * (utils.py:28-35) take target (B,N,dim) fp64 instead; the window advances by one frame and
 * the step counter increments.  If pred_out_dev != NULL the new frame is also written to
 * pred_out_dev[b][step][:][:] of a (B,pred_T,N,dim) buffer (rollout.py:165-167). */
int lb_integrate(lb_engine* eng, const float* acc_dev, const double* target_dev,
                 double* pred_out_dev, int32_t pred_T);

/* case.integrate(normalized_in, position_sequence) alone - case.py:230-259 - stateless:
 * mode 0 "acc": shift(p[-1], disp(p[-1],p[-2]) + acc_mean + pred*acc_std);
 * mode 1 "vel": shift(p[-1], vel_mean + pred*vel_std).  ("pos" is the identity: host side.)
 * pred (B,N,dim) fp32; pos_seq (B,N,T,dim) fp64 (last two frames used); out (B,N,dim) fp64. */
int lb_case_integrate(lb_engine* eng, int32_t mode, const float* pred_dev, const double* pos_seq_dev,
                      int32_t T, double* next_out_dev);

/* _eval_batched_rollout's step loop - rollout.py:125-169 - fully on the device:
 * for step in [0, n_steps): nl_update -> features -> GNS -> integrate -> store prediction.
 * traj_dev (B,N,T,dim) fp64 supplies the initial window (frames [0,isl)) and the kinematic
 * targets (frame isl+step, clamped to T-1 as JAX clamps the gather, rollout.py:159).
 * HOST-SYNCHRONOUS at the end.  On neighbor overflow it re-allocates (allocate_eval semantics,
 * rollout.py:139-151) and resumes from the overflowed step; *n_realloc_out counts that. */
int lb_rollout(lb_engine* eng, lb_gns* gns, const double* traj_dev, int32_t T, int32_t n_steps,
               double* pred_out_dev, int32_t* n_realloc_out);

/* ---- SEGNN (models/segnn.py:403-610) ---------------------------------------------------------- */

/* ---- training step ----------------------------------------------------
 * trainer.py:35-89: loss = _mse (weighted squared error of the normalised accelerations, summed over dim, masked
 * to the non-kinematic particles, divided by their number), value_and_grad vmapped over the batch with the
 * gradients SUMMED and the loss averaged, optax.adamw.  Forward (with saved activations), loss, backward and the
 * optimiser step run on the device (csrc/lb_train.hip: rocBLAS sgemm for the dense contractions, hand-written HIP
 * kernels for everything else); the graph, features and targets are the engine's (case.preprocess first). */
typedef struct lb_gns_train lb_gns_train;
/* weights_host: the flat blob of GNS.flatten (same layout as lb_gns_create); latent <= 128 (narrower: zero-padded on the device),
 * two to eight Linears per MLP (num_mlp_layers, models/utils.py:100-115; round 6). */
int lb_gns_train_create(lb_engine* eng, const lb_gns_desc* desc, const float* weights_host, int64_t n_floats,
                        lb_gns_train** out);
void lb_gns_train_destroy(lb_gns_train* t);
/* jax.value_and_grad(_mse) summed over the batch, on the engine's current window + neighbor list.
 * target_dev (B*N, dim) fp32 normalised accelerations; gradients ACCUMULATE (lb_gns_train_zero_grad);
 * *loss_out = mean of the per-trajectory losses; pred_out_dev (optional) receives the (B*N, dim) predictions. */
int lb_gns_train_loss_grad(lb_gns_train* t, const float* target_dev, float loss_weight, double* loss_out,
                           float* pred_out_dev);
int lb_gns_train_zero_grad(lb_gns_train* t);
/* optax.adamw(learning_rate, b1, b2, eps, weight_decay) on every parameter (trainer.py:183-193). */
int lb_adamw_step(lb_gns_train* t, float lr, float b1, float b2, float eps, float weight_decay);
/* which: 0 weights, 1 gradients, 2 / 3 first / second AdamW moment; flat blob in GNS.flatten order.
 * write: step >= 0 also restores the optimiser's step counter (bias correction). */
int lb_gns_train_read(lb_gns_train* t, int32_t which, float* out_host, int64_t n_floats);
int lb_gns_train_write(lb_gns_train* t, int32_t which, const float* in_host, int64_t n_floats, int64_t step);
/* optax's `count`: AdamW steps taken so far (the bias-correction exponent of the NEXT step is count + 1); what a
 * checkpoint has to store to resume bit-identically (utils.py:61-91 pickles it inside opt_state). */
int64_t lb_gns_train_step_count(lb_gns_train* t);
/* Data-parallel training (one process per GPU, the batch split over the ranks).
 * lb_gns_train_device_blob: the DEVICE pointer of blob `which` (0 weights, 1 gradients, 2 / 3 AdamW moments) and its
 * float count in the device layout (latent padded to 128: >= the n_floats of read / write; the padding is zero and stays
 * zero).  Every rank has the same layout, so this is what a collective gathers - no host copy, no re-ordering.  The
 * engine's stream is synchronised before the call returns; the pointer lives as long as the handle.
 * lb_adamw_step_gathered: gathered_dev = `world` rows of that many floats, row r = rank r's gradient blob (world 1 ... 16;
 * for world > 1 it must not overlap the handle's own gradient blob).  ONE kernel sums the rows per parameter in rank
 * order, g = ((row0 + row1) + row2) + ... in fp32 with plain adds, multiplies by grad_scale (1: the reference's
 * "gradients summed over the batch"), stores g as the handle's gradient blob and applies lb_adamw_step's arithmetic to
 * weights and moments; the step counter advances once.  No atomics, a fixed order: ranks that start from the same
 * weights and get the same rows end with the same bits.  world 1 with the handle's own gradients, grad_scale 1 gives
 * the bits of lb_adamw_step. */
int lb_gns_train_device_blob(lb_gns_train* t, int32_t which, float** dev_out, int64_t* n_floats_out);
int lb_adamw_step_gathered(lb_gns_train* t, const float* gathered_dev, int32_t world, float grad_scale, float lr,
                           float b1, float b2, float eps, float weight_decay);
/* Arithmetic of the training step (round 5 / 6).  Default: every tall-skinny product (Y = XW, dX = dY W^T, dW += X^T dY) runs
 * as three fp16 MFMA passes over hi / lo splits of fp32 operands, fp32 accumulate; the operands of the first two are put into
 * fp16's range by exact power-of-two scales per row block / matrix, dY of the third per row chunk.  Its X operand (saved
 * activations) carries ONE power-of-two scale per call site (initially 1) under a range GUARD: when a chunk's largest scaled
 * |X| leaves [2^-8, 2^15) the step's gradients are NOT added, lb_gns_train_loss_grad re-centres the scales of the call sites
 * that fired and repeats the step (a call site that fires again switches to per-chunk scales: one more pass over its X).
 * Error per product term <= 2^-22 of the operand chunks' scales; gradients vs float64 autograd <= 1e-4 per leaf
 * (tests/test_train.py).  LB_TRAIN_MATH=f32 in the environment at handle creation selects the exact-fp32 MFMA kernels
 * throughout (1.7x slower).  This returns how many steps were repeated so far. */
int32_t lb_gns_train_math_fallbacks(lb_gns_train* t);
/* Training steps repeated with a radix sort of the senders: the sender-sorted view of a step is built by transposing the
 * receiver rows, which needs every edge's transpose; a list with an edge in one direction only (a pair within one rounding
 * of the cutoff: the periodic displacement is not exactly antisymmetric) sends the step to the sort.  Gradients are the
 * same either way. */
int32_t lb_gns_train_sort_fallbacks(lb_gns_train* t);

/* The step split at d loss / d pred, for a loss the CALLER computes.  trainer.py:63-89 takes
 * value_and_grad of _mse only; these two are the halves of that step around any loss: forward with saved activations, then
 * the hand-written backward from the caller's d loss / d pred.  t: a GNS, SEGNN, EGNN or Linear training handle.
 * lb_train_forward: on the engine's current window + neighbor list; pred_out_dev receives (B*N, dim) fp32 - the normalised
 * accelerations (GNS, SEGNN, Linear) or the positions x^L (EGNN) - with the bits lb_*_train_loss_grad reports.  The handle's
 * forward is then LIVE until the next call on the handle other than lb_gns_train_zero_grad.
 * lb_train_backward: needs a live forward (else LB_ERR_STATE) and ends it.  dpred_dev (B*N, dim) fp32 is copied into the
 * handle (rows of pad particles zeroed); the gradients ACCUMULATE into the gradient blob exactly as in lb_*_train_loss_grad.
 * If the step's guard fires, the repeated attempt re-runs the forward (same weights, same window: the same activations)
 * and starts from the saved copy.  dpos_out_dev: null, or (B, N, isl, dim) fp64 that receives (overwritten) d loss / d window
 * through the feature builder (velocity history and magnitudes, wall distances, edge displacements and distances; the
 * external force counts as constant, the neighbor list as fixed) - GNS only, LB_ERR_UNSUPPORTED for SEGNN / EGNN / Linear handles. */
int lb_train_forward(lb_gns_train* t, float* pred_out_dev);
int lb_train_backward(lb_gns_train* t, const float* dpred_dev, double* dpos_out_dev);
/* The arithmetic of the handle's products from the next forward on: exact != 0 selects the exact-fp32 kernels (what
 * LB_TRAIN_MATH=f32 selects at creation), 0 the handle's default (EGNN and Linear handles are always exact).  A live forward stays
 * live: lb_train_forward in one arithmetic may be followed by lb_train_backward in the other.  Why: a ReLU unit within the
 * forward's rounding of zero takes either side of its kink, which moves its particle's gradient by per cent, and the f16x2
 * forward has about ten times as many of them as the exact one.  autograd.DeviceModule therefore runs the forward of a GNS
 * in exact arithmetic, and the backward too where the window's gradient (a per-particle quantity) is asked for. */
int lb_train_exact_math(lb_gns_train* t, int32_t exact);

/* Push-forward from device weights.
 * Re-make every packed image of `g` from the CURRENT weights of training handle `t`, on the device.
 * g and t: same engine, same lb_gns_desc (else LB_ERR_ARG).  Afterwards g is what lb_gns_create would
 * have made from lb_gns_train_read(t, 0): the same image bytes, dec_unscale, and f16x2 / rms decision
 * (the rms is an fp64 sum in another fixed order than lb_gns_create's: the decision can differ only for a
 * matrix whose rms lies within rounding of 2^-7).
 * Runs on the engine's stream; may read back a few scalars, never the weights. */
int lb_gns_train_sync_model(lb_gns_train* t, lb_gns* g);
/* Test support: the packed device blob of a model (every image, in packing order), for byte comparison. */
int64_t lb_gns_image_bytes(lb_gns* g);
int lb_gns_image_read(lb_gns* g, void* out_host, int64_t n_bytes);
/* Test support, NO HIP call: stage the images of (desc, weights_host) with the host packers of lb_gns_create, stage them
 * again by replaying the recorded job table of lb_gns_train_sync_model on the host - through the element function the
 * device kernel uses, from the training handle's 128-padded layout of the weights - and return the number of differing
 * bytes (a differing dec_unscale counts 4, an rms further apart than summation order explains 8); < 0: an error code.
 * node_in_kq: 0 = the node input's row padding as lb_gns_create derives it from the description (units of 8 columns),
 * else 4, 8, 12 or 16 to widen it.  *n_bytes_out (optional): bytes compared. */
int64_t lb_gns_pack_selftest(const lb_gns_desc* desc, int32_t node_in_kq, const float* weights_host, int64_t n_floats,
                             int64_t* n_bytes_out);

typedef struct lb_segnn lb_segnn;

/* SEGNN hyper-parameters (runner.py:217-237; configs: scalar_units 64 -> hidden irreps
 * 32x0e+32x1o through weight_balanced_irreps, segnn.py:365-400). */
typedef struct lb_segnn_desc {
  int32_t hidden;           /* multiplicity n of every irrep of the hidden irreps n x (0e + 1o + ..) (weight_balanced_irreps) */
  int32_t blocks_per_step;  /* num_mlp_layers (2) */
  int32_t num_mp_steps;
  int32_t homogeneous;      /* homogeneous_particles: 1 = no one-hot particle-type scalars */
  int32_t n_vels;           /* input_seq_length - 1 */
  int32_t velocity_avg;     /* velocity_aggregate: 1 "avg", 0 "last" */
  int32_t lmax_hidden;      /* 0 .. 2 (segnn.py:482-484) */
  int32_t lmax_attributes;  /* 0 .. 2: attributes = spherical harmonics up to this order (segnn.py:481) */
  int32_t norm;             /* segnn_norm: 0 None, 1 "instance", 2 "batch" (segnn.py:303,346-351) */
  float norm_eps;           /* eps of e3nn's BatchNorm; <= 0: 1e-5 */
} lb_segnn_desc;

/* SEGNN(...) + params.  Two weight layouts.
 * (1) hidden == 32, lmax_hidden == lmax_attributes == 1, norm == 0 (every shipped config; the fused kernels):
 *   weights_host: one (ws, wv, b) triple per O3TensorProduct in call order
 * (embedding_nodes; per layer message tp_0.. then update tp_0..; readout_0..; output):
 *   ws (K, Ms) weights of the 0e outputs (gated blocks: Ms = 2*hidden, activated scalars first,
 *   then the gates), wv (K, Mv) weights of the 1o outputs, b (Ms).  K indexes the tensor-product
 *   channels operand by operand, scalar-derived channels first, then vector-derived
 *   (oracle/segnn_oracle.py:tp_inputs); the 1/sqrt(K) of e3nn's Linear is applied here.
 * (2) anything else with lmax <= 2 (csrc/lb_segnn_gen.hip): per O3TensorProduct in the same call order, per output irrep
 *   l = 0, 1, 2: W_l (K_l, mul_l) with the rows in e3nn's regrouped order (x chunk major, attribute l minor), then b (the
 *   scalar outputs) if the output has 0e; then, with norm, per layer [messages: weight, bias - "batch" only], nodes:
 *   weight (one per channel of every hidden irrep), bias (one per hidden scalar) (e3nn BatchNorm, training-mode statistics
 *   as the reference calls it). */
int lb_segnn_create(lb_engine* eng, const lb_segnn_desc* desc, const float* weights_host,
                    int64_t n_floats, lb_segnn** out);

/* The same training step for SEGNN (round 5; reference: train/trainer.py:35-89 is model-agnostic, models/segnn.py:44-362,
 * 595-610 is the network).  The handle type is lb_gns_train (round 3's name for "a training handle"): lb_gns_train_zero_grad,
 * lb_adamw_step, lb_gns_train_read / _write (flat blob in SEGNN.flatten order = lb_segnn_create's), lb_gns_train_step_count
 * and lb_gns_train_destroy work on it unchanged; lb_gns_train_loss_grad dispatches to lb_segnn_train_loss_grad.
 * hidden <= 32, lmax 1, norm None (the shipped configs); gradients bit-reproducible. */
int lb_segnn_train_create(lb_engine* eng, const lb_segnn_desc* desc, const float* weights_host, int64_t n_floats,
                          lb_gns_train** out);
int lb_segnn_train_loss_grad(lb_gns_train* t, const float* target_dev, float loss_weight, double* loss_out,
                             float* pred_out_dev);
void lb_segnn_destroy(lb_segnn* segnn);

/* SEGNN.__call__ -> {"acc": (B,N,dim) fp32} (segnn.py:595-610) on the current window + list. */
int lb_segnn_forward(lb_engine* eng, lb_segnn* segnn, float* acc_out_dev);

/* ---- EGNN (models/egnn.py:209-400) --------------------------------------------------------------
 * Construction by runner.py:246-268: hidden_size = latent_dim, dt = metadata dt * write_every, n_vels = isl - 1,
 * residual = 1, homogeneous_particles left at its default 1, attention / normalize / tanh 0, act_fn silu.  Runs in fp32
 * throughout (runner.py:71-72), positions included; sums in a fixed order (bit-reproducible). */
typedef struct lb_egnn lb_egnn;
typedef struct lb_egnn_desc {
  int32_t hidden;        /* hidden_size: a multiple of 16, <= 128 */
  int32_t num_mp_steps;  /* >= 1 */
  int32_t n_vels;        /* input_seq_length - 1 (1 .. 9) */
  int32_t homogeneous;   /* homogeneous_particles: 1 = no one-hot of the 9 particle types in the node input */
  int32_t residual;      /* h' = h + node_mlp(..) */
  int32_t normalize;     /* coord_diff /= sqrt(radial) + 1e-8 */
  int32_t tanh_pos;      /* tanh on the position net's output */
} lb_egnn_desc;

/* EGNN(...) + params.  weights_host, with H = hidden, I = n_vels (+ 9 when !homogeneous), A = 1 when the engine has an
 * external force (node attribute |force|) else 0; every matrix (fan_in, fan_out) row-major:
 *   scalar_emb w (I, H), b (H)
 *   per layer n (module names egnn/~/layer_{n}/~/...):
 *     mlp_xav/~/linear_0   w (2H + 2, H), b (H)   rows [h_sender | h_receiver | radial | rel_dist]
 *     mlp_xav/~/linear_1   w (H, H), b (H)
 *     mlp_xav_1/~/linear_0 w (2H + A, H), b (H)   rows [h | aggregated messages | |force|]
 *     mlp_xav_1/~/linear_1 w (H, H), b (H)
 *     linear_xav   w (H, H), b (H);  linear_xav_1 w (H, 1)     position net
 *     linear_xav_2 w (H, H), b (H);  linear_xav_3 w (H, 1)     velocity net
 * n_floats must match exactly. */
int lb_egnn_create(lb_engine* eng, const lb_egnn_desc* desc, const float* weights_host, int64_t n_floats,
                   lb_egnn** out);
void lb_egnn_destroy(lb_egnn* egnn);
/* EGNN.__call__ -> {"pos"} on the current window + list: (B,N,dim) fp64 holding the fp32 positions (fp64 so that
 * rollout.py's window keeps its dtype, as the reference's promotion does).  The position update sums over senders: an
 * edge held in one direction only (a pair within one rounding of the cutoff) is summed at its sender as the reference's
 * segment_sum does.  Host-synchronous. */
int lb_egnn_forward(lb_engine* eng, lb_egnn* egnn, double* pos_out_dev);
/* Debug/parity taps: h after the embedding and after every layer ((L+1), B*N, hidden) fp32 and the positions at the same
 * points ((L+1), B*N, dim) fp32; NULL = off. */
int lb_egnn_set_tap(lb_egnn* egnn, float* h_out_dev, float* pos_out_dev);
/* lb_rollout for an EGNN: the whole step loop on the device (the predicted positions are the new frame). */
int lb_egnn_rollout(lb_engine* eng, lb_egnn* egnn, const double* traj_dev, int32_t T, int32_t n_steps,
                    double* pred_out_dev, int32_t* n_realloc_out);

/* The training step for EGNN (reference: train/trainer.py:35-89 with EGNN's three outputs, models/egnn.py:361-369).  The
 * handle type is lb_gns_train: lb_gns_train_zero_grad, lb_adamw_step, lb_gns_train_read / _write (flat blob in EGNN.flatten
 * order = lb_egnn_create's), lb_gns_train_step_count and lb_gns_train_destroy work on it unchanged; lb_gns_train_loss_grad
 * on it returns LB_ERR_ARG (the loss needs three targets).  desc->normalize = 1 is refused (LB_ERR_ARG): every radius graph
 * here holds self-edges, and d/d radial of coord_diff / (sqrt(radial) + 1e-8) at radial = 0 is 0 * inf, so the
 * reference's own gradient is NaN for num_mp_steps >= 2.  num_mp_steps <= 40.  Exact fp32 arithmetic, sums in a fixed
 * order: gradients bit-reproducible. */
int lb_egnn_train_create(lb_engine* eng, const lb_egnn_desc* desc, const float* weights_host, int64_t n_floats,
                         lb_gns_train** out);
/* value_and_grad of _mse on the engine's CURRENT window / neighbor list: predictions pos = the network's fp32 positions,
 * vel = displacement(pos, newest input position), acc = vel - the normalised last velocity feature (all fp32); loss =
 * sum over the outputs of w_k |pred_k - target_k|^2 (fp64 residuals), summed over dim, masked to the non-kinematic
 * particles, / their number; mean over the batch, gradients summed and ACCUMULATED (lb_gns_train_zero_grad).  Targets: device
 * (B*N, dim) fp64, the case's {pos, vel, acc}; a target may be NULL when its weight is 0.  pred_pos_out_dev (B*N, dim) fp32
 * or NULL: the prediction, bit-identical to lb_egnn_forward's.  Host-synchronous. */
int lb_egnn_train_loss_grad(lb_gns_train* t, const double* tgt_pos, const double* tgt_vel, const double* tgt_acc,
                            float w_pos, float w_vel, float w_acc, double* loss_out, float* pred_pos_out_dev);
/* The inference model of an EGNN training handle: a view of its device weights, so lb_egnn_forward / lb_egnn_rollout on it
 * run on the CURRENT weights (bit-identical to a model created from lb_gns_train_read(t, 0)).  BORROWED: owned by t,
 * valid until lb_gns_train_destroy(t); never pass it to lb_egnn_destroy. */
int lb_egnn_train_model(lb_gns_train* t, lb_egnn** out);

/* ---- PaiNN (models/painn.py:372-510) -----------------------------------------------------------
 * Construction by runner.py:270-284: hidden_size = latent_dim, output_size 1, n_vels = isl - 1, gaussian_rbf(20,
 * 1.5 r_c, trainable) and cosine_cutoff(1.5 r_c) with the PHYSICAL radius (the network's norms are in units of r_c),
 * homogeneous_particles left at its default 1, activation silu.  The output is the normalised acceleration, integrated
 * like GNS's.  Runs in fp32 throughout (runner.py:71-72); sums in a fixed order (bit-reproducible).  The case must
 * carry the velocity magnitudes (magnitude_features), the model's scalars. */
typedef struct lb_painn lb_painn;
typedef struct lb_painn_desc {
  int32_t hidden;               /* hidden_size: a multiple of 16, <= 128 */
  int32_t num_mp_steps;         /* >= 1 */
  int32_t n_vels;               /* input_seq_length - 1 (1 .. 9) */
  int32_t homogeneous;          /* homogeneous_particles: 1 = no one-hot of the 9 particle types in the scalars */
  int32_t shared_filters;       /* one 3H filter block for all layers */
  int32_t shared_interactions;  /* one set of layer weights (layer_0) for all layers */
  int32_t n_rbf;                /* Gaussian radial basis functions (1 .. 64) */
  int32_t has_cutoff;           /* 1: cosine_cutoff(cutoff); 0: cutoff_fn None (the filters are scaled by the norm) */
  float cutoff;                 /* cosine cutoff radius in the units of rel_disp's norm */
} lb_painn_desc;

/* PaiNN(...) + params.  weights_host, with H = hidden, Hh = H / 2, R = n_rbf, S = n_vels (+ 9 when !homogeneous),
 * C = n_vels (+ 1 with an external force) (+ 2 with boundary features) vector channels in the order [v_0 .. v_{K-1} |
 * force | bound_lo | bound_hi], F = 1 if shared_filters else num_mp_steps, P = 1 if shared_interactions else
 * num_mp_steps; every matrix (fan_in, fan_out) row-major (Haiku names painn/~/...):
 *   scalar_embedding w (S, H), b (H);  vector_embedding w (C, H)
 *   filter_net w (R, F 3H), b (F 3H)                    layer n takes columns [3H n, 3H (n + 1)) as [ds | dv1 | dv2]
 *   per parameter set p < P (layer_{p}/~/...):
 *     linear_xav   w (H, H), b (H);  linear_xav_1 w (H, 3H), b (3H)     interaction block
 *     linear_xav_2 w (2H, H), b (H); linear_xav_3 w (H, 3H), b (3H)     mixing block, rows [s | |v_r|]
 *     vector_mixing_block w (H, 2H)                                      columns [v_l | v_r]
 *   readout_block_0/~/:   vector_mix_net w (H, H); linear_xav w (H + Hh, H), b (H); linear_xav_1 w (H, H), b (H)
 *   readout_block_out/~/: vector_mix_net w (Hh, 2); linear_xav w (Hh + 1, Hh), b (Hh); linear_xav_1 w (Hh, 2), b (2)
 *   ~/widths (R), ~/offset (R)                          the radial basis (parameters, or state when not trainable)
 * n_floats must match exactly. */
int lb_painn_create(lb_engine* eng, const lb_painn_desc* desc, const float* weights_host, int64_t n_floats,
                    lb_painn** out);
void lb_painn_destroy(lb_painn* painn);
/* PaiNN.__call__ -> {"acc": (B,N,dim) fp32} on the current window + list.  The messages are summed over senders, edges
 * held in one direction only included.  Host-synchronous. */
int lb_painn_forward(lb_engine* eng, lb_painn* painn, float* acc_out_dev);
/* Debug/parity taps: s after the embedding and after every layer ((L+1), B*N, hidden) fp32 and v at the same points
 * ((L+1), B*N, dim, hidden) fp32; NULL = off. */
int lb_painn_set_tap(lb_painn* painn, float* s_out_dev, float* v_out_dev);
/* lb_rollout for a PaiNN: the whole step loop on the device, the acceleration integrated as GNS's. */
int lb_painn_rollout(lb_engine* eng, lb_painn* painn, const double* traj_dev, int32_t T, int32_t n_steps,
                     double* pred_out_dev, int32_t* n_realloc_out);

/* The training step for PaiNN (reference: train/trainer.py:35-89 on PaiNN.__call__).  The handle type is lb_gns_train:
 * lb_gns_train_loss_grad (one "acc" target, the masked _mse), lb_train_forward / lb_train_backward (weights only: a
 * non-null dpos_out_dev is LB_ERR_UNSUPPORTED), lb_gns_train_zero_grad, lb_adamw_step(_gathered), lb_gns_train_read /
 * _write (flat blob in PaiNN.flatten order = lb_painn_create's, n_floats exact), lb_gns_train_step_count,
 * lb_gns_train_device_blob and lb_gns_train_destroy work on it unchanged; lb_egnn_train_loss_grad on it is LB_ERR_ARG.
 * The forward is lb_painn_forward's, bit for bit; the backward gives the gradients of every weight, in exact fp32 with
 * sums in a fixed order (bit-reproducible).  rbf_trainable = 1: ~/widths and ~/offset (the last 2 n_rbf floats) are
 * parameters, as with gaussian_rbf(trainable=True); 0: they are state - their gradient stays 0 and neither optimiser step
 * touches them, so lb_gns_train_read returns the bits that were written.  Built for 64 <= hidden <= 128 and
 * num_mp_steps <= 32 (LB_ERR_UNSUPPORTED otherwise). */
int lb_painn_train_create(lb_engine* eng, const lb_painn_desc* desc, const float* weights_host, int64_t n_floats,
                          int32_t rbf_trainable, lb_gns_train** out);
/* The inference model of a PaiNN training handle: a view of its device weights, so lb_painn_forward / lb_painn_rollout on
 * it run on the CURRENT weights (bit-identical to a model created from lb_gns_train_read(t, 0)).  BORROWED: owned by t,
 * valid until lb_gns_train_destroy(t); never pass it to lb_painn_destroy. */
int lb_painn_train_model(lb_gns_train* t, lb_painn** out);

/* ---- Linear (models/linear.py:13-42) ------------------------------------------------------------
 * The baseline of the reference's own end-to-end test: acc_i = x_i W + b with x_i = [vel_hist | vel_mag | bound | force |
 * float(particle_type_i)], each block present when the case has it - the engine's node features followed by the raw type
 * id as a VALUE (no one-hot).  The output is the normalised acceleration, integrated like GNS's.  fp32 (runner.py:71-72),
 * sums in a fixed order (bit-reproducible; a particle's result does not depend on the batch). */
typedef struct lb_linear lb_linear;
typedef struct lb_linear_desc {
  int32_t n_in;     /* node features of the engine + 1 (the type column): <= 64 */
  int32_t out_dim;  /* dim */
} lb_linear_desc;

/* Linear(dim_out) + params (Haiku names linear/~/linear).  weights_host: w (n_in, out_dim) row-major, then b (out_dim);
 * n_floats must match exactly.  desc is checked against the engine (LB_ERR_ARG); n_in > 64 is LB_ERR_UNSUPPORTED. */
int lb_linear_create(lb_engine* eng, const lb_linear_desc* desc, const float* weights_host, int64_t n_floats,
                     lb_linear** out);
void lb_linear_destroy(lb_linear* linear);
/* Linear.__call__ -> {"acc": (B,N,dim) fp32} on the current window.  The model reads no edges: a neighbor list need not
 * exist.  If the engine's last list build overflowed, every step kernel is a no-op until a re-allocation: nothing is written
 * and the call returns LB_ERR_STATE.  Host-synchronous. */
int lb_linear_forward(lb_engine* eng, lb_linear* linear, float* acc_out_dev);
/* lb_rollout for a Linear: the whole step loop on the device (features, model, integrator).  No step builds the neighbor
 * list - the positions equal those of the generic loop, which builds one per step, bit for bit - so *n_realloc_out is 0;
 * like lb_rollout it leaves an allocated list behind (an engine without one, or with an overflowed one, allocates once
 * before the loop; the latter is counted as one re-allocation). */
int lb_linear_rollout(lb_engine* eng, lb_linear* linear, const double* traj_dev, int32_t T, int32_t n_steps,
                      double* pred_out_dev, int32_t* n_realloc_out);
/* The training step for Linear.  The handle type is lb_gns_train: lb_gns_train_loss_grad (one "acc" target, like SEGNN),
 * lb_train_forward / lb_train_backward (no gradient with respect to the window: LB_ERR_UNSUPPORTED), lb_gns_train_zero_grad,
 * lb_adamw_step(_gathered), lb_gns_train_read / _write / _device_blob (flat blob in lb_linear_create's order, no padding),
 * lb_gns_train_step_count and lb_gns_train_destroy work on it.  The prediction is lb_linear_forward's bit for bit; dW = X^T dY
 * and db = sum dY in exact fp32, chunks of rows summed in ascending order: gradients bit-reproducible. */
int lb_linear_train_create(lb_engine* eng, const lb_linear_desc* desc, const float* weights_host, int64_t n_floats,
                           lb_gns_train** out);
/* The inference model of a Linear training handle: a view of its device weights, so lb_linear_forward / lb_linear_rollout
 * on it run on the CURRENT weights.  BORROWED: owned by t, valid until lb_gns_train_destroy(t); never pass it to
 * lb_linear_destroy.  The view has node rows of its own: a forward or rollout on it between lb_train_forward and
 * lb_train_backward leaves the handle's saved activations alone (the ENGINE's window is the caller's to restore). */
int lb_linear_train_model(lb_gns_train* t, lb_linear** out);

/* ---- a training handle that is only optimiser state ----------------------
 * For a model the CALLER evaluates and differentiates (models.TorchModel: a torch.nn.Module on the engine's features and
 * graph ops): w / g / m / v blobs of exactly n_floats floats, initialised from weights_host / 0 / 0 / 0 - no padding, nothing
 * frozen, step counter 0.  lb_gns_train_zero_grad, lb_adamw_step, lb_adamw_step_gathered, lb_gns_train_read / _write /
 * _device_blob, lb_gns_train_step_count and lb_gns_train_destroy work on it unchanged (the caller's autograd accumulates into
 * the gradient blob through lb_gns_train_device_blob).  lb_gns_train_loss_grad, lb_segnn_train_loss_grad,
 * lb_egnn_train_loss_grad, lb_train_forward, lb_train_backward and lb_gns_train_sync_model return LB_ERR_UNSUPPORTED with a
 * message that names the blob handle: there is no model in it. */
int lb_blob_train_create(lb_engine* eng, const float* weights_host, int64_t n_floats, lb_gns_train** out);

/* Arithmetic of the GNS GEMMs.  Default (LB_MATH unset) = mode 1: every fp32 operand is carried as an fp16
 * hi/lo pair on the fp16 MFMA (fp32-class accuracy, ~5x fewer matrix-pipe cycles than the fp32 MFMA) WITH a
 * range guard: operands >= 2^15 (sampled), operand ROWS whose values all sit below 2^-11 (tested on every tile of the
 * batch edge / node kernels and of the small-graph kernels), and non-finite accelerations raise
 * flags; lb_gns_forward / lb_rollout then redo the flagged forward / rollout step in mode 0 and return to mode 1
 * (round 4: not sticky; after LB_GUARD_MAX_FALLBACKS = 3 flagged steps the rest of that rollout runs in mode 0).
 * set_mode: -1 query, 0 exact fp32 MFMA, 1 guarded f16x2, 2 f16x2 without the switch (tests), 3 guarded with
 * every k-group of every tile tested (LB_GUARD=full).  flags_out: guard bits raised and not yet consumed
 * (1 large, 2 tiny, 4 non-finite).  The reference computes the model in fp32 (runner.py:71-72). */
int lb_math_mode(lb_engine* eng, int32_t set_mode, int32_t* mode_out, int32_t* flags_out);

/* Steps (or stand-alone forwards) the range guard has redone in exact fp32 since the engine was created. */
int32_t lb_math_fallbacks(lb_engine* eng);

/* What the per-tile guard covers (mode 1): LARGE / NaN - the sampled probe (first tile of every wave) on every GEMM operand,
 * plus the decoder's output test on every row; TINY rows - the edge latents and the hidden layer of k_edge16v, every operand
 * of the M-split kernels, the hidden layer of k_node16s.  NOT row-tested: the first operand [node latents | aggregated
 * messages] of k_node16s (its rows are LayerNorm outputs, |x| = O(1), plus sums of them).  A flagged step is redone in fp32
 * and the steps before it are kept; with LB_GUARD=sampled (probe only) the rollout restarts from step 0 instead.
 *
 * Test hook: the NEXT lb_rollout behaves as if the guard had raised `flags` (LB_MATH_* bits: 1 large, 2 tiny, 4 non-finite)
 * at rollout step `step` (one-shot; step < 0 disarms).  Lets a test drive the redo-one-step-in-fp32 / resume-in-f16x2
 * path on healthy weights and compare the result with the oracle.  No reference counterpart. */
int lb_debug_inject_guard(lb_engine* eng, int32_t flags, int32_t step);

/* ---- test hooks of the training step's gradient reductions -----------------
 * TEST ONLY: no product code calls them.  They run the launchers of csrc/lb_train.hip - the host code that decides a
 * kernel's grid, row chunks and partial-sum slots - on arrays the caller supplies, so that a test compares each producer
 * kernel and the ordered reduce with a float64 reference without restating that geometry.  Both change no state of a
 * model-backed handle: the plan query takes no handle, and lb_train_probe accepts a blob handle (lb_blob_train_create)
 * only and is LB_ERR_ARG on every other one.
 *
 * lb_train_probe_plan: host only.  What the weight-gradient launcher does with `rows` rows and K columns of X in
 * arithmetic `math` (0 exact fp32, 1 f16x2): out[0] = G workgroups, out[1] = chunk (rows per workgroup), out[2] = 1 if
 * k_dw_part_h runs, else out[3] = NA and out[4] = DEPTH of k_dw_part<NA, DEPTH>.  The launcher itself chooses through
 * the same function. */
int lb_train_probe_plan(int64_t rows, int32_t K, int32_t math, int64_t* out5);

#define LB_PROBE_DW 0          /* dW[K x 128] += X^T dY, db[nb] += column sums of dY (k_dw_part / k_dw_part_h)             */
#define LB_PROBE_DW_NARROW 1   /* dW[K x M] += X^T dY, M <= 4, K <= 128 (k_dw_narrow)                                       */
#define LB_PROBE_COLSUM 2      /* out[M] += column sums of x (rows x M, row stride ldx) (k_colsum_part)                     */
#define LB_PROBE_LN_BWD 3      /* LayerNorm backward with its parameter gradients (k_ln_bwd2)                               */
#define LB_PROBE_REDUCE 4      /* the ordered reduce alone, on partials the caller wrote (k_part_reduce)                    */
#define LB_PROBE_EMBED_GRAD 5  /* gembed[ntypes x emb] += per-type row sums of x[:, col0 : col0 + emb] (k_embed_grad)       */
/* One call of lb_train_probe.  Pointers are DEVICE pointers; a field an op does not name is ignored.  dst0 / dst1 /
 * dst_b are float offsets into the handle's GRADIENT blob (lb_gns_train_device_blob, which = 1), -1 = none; the op's whole
 * destination must lie inside the blob.
 *   DW           x (rows x K, row stride ldx), dy (rows x 128), rows, K, ldx, dst0 = dW, dst1 = db or -1, nb (columns of db),
 *                tmax (largest |dy| per 16-row tile, ceil(rows / 16) floats) or NULL, dy_b / dst_b = the second product of a
 *                paired launch or NULL / -1, math (0 exact fp32, 1 f16x2), xexp (the site's X exponent, |xexp| <= 126), xdyn
 *   DW_NARROW    x, ldx, K, dy (rows x M, row stride ldy), M, rows, dst0
 *   COLSUM       x (rows x M, row stride ldx), M, rows, dst0
 *   LN_BWD       z, b1, scale (128 floats each, zero beyond d), dy, dz (out, rows x 128), rows, d, gth / idx (the gathered
 *                term dy[r] + gth[idx[r]]) or NULL, dst0 = d scale, dst1 = d offset
 *   REDUCE       x = G partials (G * stride floats; copied to float offset part_off of the partial buffer), G, stride, n0, n1,
 *                off1, ld0, dst0, dst1 (the descriptor of csrc/lb_train.hip: lb_red_ent), skip (nonzero: the guard word is
 *                raised before the launch, which then adds nothing)
 *   EMBED_GRAD   x (rows x ldx), col0, emb, idx = particle types (rows), ntypes, rows, dst0, skip
 * Out: guard = the step's guard word after the call (bit 1 / 2: k_dw_part_h saw |X| above / below its fp16 window; the
 * reduce then added nothing), slot = the site's slot (the bit pattern of the largest raw |X| when the guard fired). */
typedef struct lb_train_probe_args {
  const float *x, *dy, *dy_b, *tmax, *z, *b1, *scale, *gth;
  float* dz;
  const int32_t* idx;
  int64_t rows, dst0, dst1, dst_b, part_off, stride;
  int32_t K, ldx, M, ldy, nb, math, xexp, xdyn, d, G, n0, n1, off1, ld0, skip, col0, emb, ntypes;
  int32_t guard, slot;
} lb_train_probe_args;
/* Runs launcher `op` and the ordered reduce on the handle's stream and waits for them.  The partial buffer, descriptor
 * table and guard words come from the handle's arena and grow to what the call needs; the arithmetic, the site's X
 * exponent and its per-chunk switch hold for this call only.  LB_ERR_ARG with a reason in lb_last_error: a null
 * pointer, K > 384, an odd K with ldx <= K, a paired launch outside f16x2 (math 0 or K < 32), a destination outside
 * the blob, a handle that is not a blob handle.  The arguments are checked before the handle is looked at. */
int lb_train_probe(lb_gns_train* t, int32_t op, lb_train_probe_args* args);

/* Debug/parity tap: hidden node state after the embedding and after each layer,
 * ((num_mp_steps+1), B*N, lb_segnn_row_floats) fp32 rows, or NULL.  Layout (1): 128 floats [s(32) | vx(32) | vy(32) | vz(32)];
 * layout (2): e3nn's own layout (n scalars, n x 3, n x 5), padded to a multiple of 4 floats. */
int lb_segnn_set_tap(lb_segnn* segnn, float* hidden_out_dev);
int32_t lb_segnn_row_floats(lb_segnn* segnn);

/* lb_rollout with SEGNN as the model. */
int lb_segnn_rollout(lb_engine* eng, lb_segnn* segnn, const double* traj_dev, int32_t T,
                     int32_t n_steps, double* pred_out_dev, int32_t* n_realloc_out);

/* MetricsComputer.mse / .mae per step - evaluate/metrics.py:139-147: mean over (N,dim) of
 * disp(pred,target)^2 (|.|) with the case's displacement.  Both rollouts are (B,T,N,dim) fp64,
 * the layout metrics_computer receives (rollout.py:171-176).  Outputs (B,n_steps) fp64,
 * either may be NULL. */
int lb_metrics(lb_engine* eng, const double* pred_dev, int32_t pred_T, const double* target_dev,
               int32_t target_T, int32_t n_steps, double* mse_out_dev, double* mae_out_dev);

/* MetricsComputer "e_kin" - evaluate/metrics.py:98-125,157-160: kinetic energy of strided frames of
 * one rollout (B,T,N,dim) fp64: out[b][k] = dx^dim * sum((disp(x[1+k*stride], x[k*stride]) / dt)^2),
 * k < n_out = ceil((T-1)/stride) (= len(x[1::stride])).  out (B,n_out) fp64. */
int lb_ekin(lb_engine* eng, const double* rollout_dev, int32_t T, int32_t stride, double dt, double dx,
            double* out_dev, int32_t n_out);

/* MetricsComputer "sinkhorn" - evaluate/metrics.py:127-136,162-176,198-213: Sinkhorn divergence
 * between the predicted and the target particle cloud of every stride-th frame,
 * out[b][k] = S_eps(pred[b, k*stride], target[b, k*stride]), k < n_out = ceil(T/stride) with
 * T = min(pred_T, target_T) frames compared.  Cost = squared case displacement rounded to float32,
 * uniform weights, eps = 0.05 * mean(C_xy) shared by the xy / xx / yy problems, convergence
 * `threshold` (the reference passes 1e-4) on the L1 marginal error checked every 10 iterations
 * (ott-jax 0.4.6 sinkhorn_divergence, restated in oracle/sinkhorn_oracle.py).  Rollouts (B,T,N,dim)
 * fp64; out (B,n_out) fp64 on the device; iters_out_host (optional, HOST, B*n_out*3 int32) receives
 * the iteration counts of the three solves.  Host-synchronous (the stopping rule is data dependent). */
int lb_sinkhorn(lb_engine* eng, const double* pred_dev, int32_t pred_T, const double* target_dev,
                int32_t target_T, int32_t stride, double threshold, double* out_dev, int32_t n_out,
                int32_t* iters_out_host);

/* MetricsComputer(ot_backend="pot") - evaluate/metrics.py:178-196: POT's sinkhorn2(a, b, M, reg, numItermax,
 * stopThr) (the reference passes reg=0.1, numItermax=500, stopThr=1e-05) on the xy / xx / yy float32 cost
 * matrices with uniform weights, out[b][k] = clip(xy - 0.5 * (xx + yy), 0) evaluated in float32 like the reference
 * (each sinkhorn2 value is rounded to float32 first).  POT is an optional dependency of the reference; its
 * Sinkhorn-Knopp iteration is restated in oracle/sinkhorn_pot_oracle.py.  Same frame selection / shapes as
 * lb_sinkhorn.  info_out_host (optional, HOST, B*n_out*6 int32): iterations of the three solves, then how each
 * loop ended (0 numItermax reached, 1 err < stopThr, 2 numerical stop: previous scalings kept). */
int lb_sinkhorn_pot(lb_engine* eng, const double* pred_dev, int32_t pred_T, const double* target_dev,
                    int32_t target_T, int32_t stride, double reg, int32_t num_iter_max, double stop_thr,
                    double* out_dev, int32_t n_out, int32_t* info_out_host);

/* ---- measurement hooks (bench.py) ------------------------------------------------------ */

/* Enable per-kernel-class HIP-event timing on the engine stream.  Classes: see lb_timer_name. */
int lb_timers_enable(lb_engine* eng, int32_t on);
int lb_timers_reset(lb_engine* eng);
int32_t lb_timer_count(void);
const char* lb_timer_name(int32_t cls);
/* Accumulated milliseconds and launch count of one class (host-synchronous). */
int lb_timer_get(lb_engine* eng, int32_t cls, double* ms_out, int64_t* launches_out);

/* Current totals: real edges over all trajectories, E_cap, cell capacity (host-synchronous). */
int lb_stats(lb_engine* eng, int64_t* n_edges_total, int32_t* e_cap, int32_t* cell_capacity);

/* Edge accounting for measurements: every neighbor-list build (allocate or update, each rollout step is one) adds its real
 * edge count (all B trajectories, before clamping to the capacity) to a device-side sum.  sum_edges / n_builds = the MEAN
 * E of the steps run since the last reset - what a per-launch byte or flop count averaged over a rollout must use
 * (SURVEY 8d "use real E"; a rollout's E drifts).  first_edges / last_edges: the first build after the reset and the
 * latest one.  reset != 0 zeroes the sums after reading.  Host-synchronous.  No reference counterpart. */
int lb_edge_accounting(lb_engine* eng, int64_t* sum_edges, int64_t* n_builds, int64_t* first_edges, int64_t* last_edges,
                       int32_t reset);

/* Which kernels a GNS forward of this engine runs on at its CURRENT size / arithmetic mode, as
 * "edge=<kernel>;node=<kernel>" (NUL-terminated, truncated to cap): the network kernels are picked by graph size
 * (M-split kernels for one small trajectory, wave-per-tile kernels for batches) - bench.py names the kernel its
 * roofline line is about with this.  No reference counterpart (measurement aid). */
int lb_kernel_names(lb_engine* eng, char* out, int32_t cap);

/* What the most recent neighbor-list build (lb_nl_allocate, lb_nl_update, a rollout step outside a replayed graph) launched,
 * as "key=value;" pairs (NUL-terminated, truncated to cap), read from host bookkeeping only:
 *   build     k_nl_small | k_nl_mid (the whole build in one launch) | multi
 *   cells     none | strided | cells_small | cells_traj | cells_mid | sort (the counting sort)
 *   search    none | k_nl | k_nlw | k_nlc: the sweep that writes edges;  f32, dim: the template instance of the search or
 *             single-launch kernel;  cell_list, dense: 0 | 1
 *   cand      staged candidates of k_nl (128 .. 1024 one wave, 2048 four waves; 0 for the other kernels)
 *   count, count_cand   the same for the counting sweep of an allocation (it may run another kernel than the fill)
 *   mode      none | rows (one sweep into per-node rows) | count+fill (two sweeps)
 *   finish    none | compact_scan | rows_small | scan+finish, "+compact" appended when k_nl_compact follows
 *   reentry   none, or the kernel an allocation counted with before it hit the stencil limit and ran again dense
 * An allocation reports its whole call.  No reference counterpart (test aid). */
int lb_nl_route(lb_engine* eng, char* out, int32_t cap);

/* Stand-alone jraph.segment_sum(messages, receivers, N) on the CURRENT list (gns.py:117-119):
 * msg (E_total,D) fp32 in engine edge order -> out (B*N,D) fp32.  Used by tests and by the
 * aggregation-roofline leg of bench.py. */
int lb_segment_sum(lb_engine* eng, const float* msg_dev, float* out_dev, int32_t D);

/* ---- graph primitives for a network written outside the library --------
 * x[senders], x[receivers] and jraph.segment_sum(msg, receivers | senders, N) on the engine's CURRENT list, each other's
 * adjoints (the backward of one is the other).  role: 0 receivers, 1 senders.  All tensors fp32 (bfloat16: the _t entries
 * further down), row-major, on the engine's
 * device, in the PADDED layout of lb_nl_read_idx: edge slot (b, j), j < n_edges[b], is the j-th edge of trajectory b in
 * canonical (receiver, sender) order.  C >= 1 columns, no upper limit; 16-byte accesses when C % 4 == 0 and both pointers
 * are 16-byte aligned.  Asynchronous on the engine's stream, except the first call after a list build, which reads the
 * list's status back (and, for the sender sum, builds the sender-ordered view: per sender its edges in ascending slot
 * order, by transposing the receiver rows, or by a stable radix sort when an edge has no transpose).  LB_ERR_STATE
 * without a list or with an overflowed one.
 * lb_graph_gather: real slots get a copy of the node row, pad slots (j >= n_edges[b]) +0.0.
 * lb_graph_segment_sum: out[b, i, :] = the fp32 sum of the real slots whose role index is i, taken one term after the other
 * in ASCENDING SLOT ORDER starting from the first term - bit for bit a float32 loop; pad slots are never read (they may
 * hold NaN); a node with no such edge gets +0.0.  No float atomics: two calls give the same bits. */
int lb_graph_gather(lb_engine* eng, int32_t role, const float* x_dev /*(B*N,C)*/, float* out_dev /*(B*E_cap,C)*/, int32_t C);
int lb_graph_segment_sum(lb_engine* eng, int32_t role, const float* msg_dev /*(B*E_cap,C)*/, float* out_dev /*(B*N,C)*/,
                         int32_t C);
/* ---- graph ops for attention and pooling layers ------------------------
 * The rules of the segment sum hold for all of them: fp32, the padded layout, role 0 receivers / 1 senders (the cached sender
 * view), pad slots never read (they may hold NaN), every pad slot of an edge-shaped output +0.0, no float atomics, two calls
 * give the same bits, int64 addresses.  LB_ERR_ARG on a null pointer, a role other than 0 / 1, or C, H, D < 1; LB_ERR_STATE as
 * above.  "Slot order" is ascending slot j within the trajectory, over the real slots whose role index is the node.
 * degree: out[b, i] = the number of those slots (int32).
 * segment_max: out[b, i, c] starts from the node's first slot; each further slot in slot order replaces it only if it is
 *   strictly greater (ties keep the earlier slot, -0.0 then +0.0 stays -0.0); a NaN wins and stays.  segment_min: strictly
 *   smaller.  A node without a slot gets +0.0 (not -/+inf).  win[b, i, c] (int32) is the slot j that won, -1 for such a node.
 * segment_max_backward (max and min): d_msg[slot, c] = d_out[node, c] where the slot is win[node, c], +0.0 in every other
 *   slot, pads included; every slot is written.
 * segment_softmax: per node and column m = the maximum as above, e_j = expf(x_j - m) (the accurate expf), s = e of the first
 *   slot + e of each further slot in slot order, y_j = e_j / s.
 * segment_softmax_backward: d_x_j = y_j (d_y_j - sum_k d_y_k y_k), the sum in slot order from its first term.
 * attend: out[b, i, h, :] = sum_j alpha[j, h] values[j, h, :] with alpha = e / s exactly as segment_softmax computes it from
 *   logits (B*E_cap, H); each product is rounded to fp32, the sum starts from the first product and adds in slot order, without
 *   FMA contraction - bit for bit segment_sum(segment_softmax(logits)[..., None] * values).  m, s (B*N, H): the maximum and the
 *   sum used (0 and 1 for a node without a slot), for the backward.
 * attend_backward: d_values[j, h, :] = alpha[j, h] d_out[node, h, :] (one multiplication: the composition's bits);
 *   d_logits[j, h] = alpha[j, h] (t[j, h] - sum_k alpha[k, h] t[k, h]), t[j, h] = sum_d d_out[node, h, d] values[j, h, d] with d
 *   ascending in one lane, the sum over k in slot order.  alpha is recomputed from logits, m and s: the forward's bits. */
int lb_graph_degree(lb_engine* eng, int32_t role, int32_t* out_dev /*(B*N)*/);
int lb_graph_segment_max(lb_engine* eng, int32_t role, const float* msg_dev /*(B*E_cap,C)*/, float* out_dev /*(B*N,C)*/,
                         int32_t* win_dev /*(B*N,C)*/, int32_t C);
int lb_graph_segment_min(lb_engine* eng, int32_t role, const float* msg_dev /*(B*E_cap,C)*/, float* out_dev /*(B*N,C)*/,
                         int32_t* win_dev /*(B*N,C)*/, int32_t C);
int lb_graph_segment_max_backward(lb_engine* eng, int32_t role, const float* d_out_dev /*(B*N,C)*/,
                                  const int32_t* win_dev /*(B*N,C)*/, float* d_msg_dev /*(B*E_cap,C)*/, int32_t C);
int lb_graph_segment_softmax(lb_engine* eng, int32_t role, const float* logits_dev /*(B*E_cap,C)*/,
                             float* out_dev /*(B*E_cap,C)*/, int32_t C);
int lb_graph_segment_softmax_backward(lb_engine* eng, int32_t role, const float* y_dev /*(B*E_cap,C)*/,
                                      const float* d_y_dev /*(B*E_cap,C)*/, float* d_x_dev /*(B*E_cap,C)*/, int32_t C);
int lb_graph_attend(lb_engine* eng, int32_t role, const float* logits_dev /*(B*E_cap,H)*/,
                    const float* values_dev /*(B*E_cap,H*D)*/, float* out_dev /*(B*N,H*D)*/, float* m_dev /*(B*N,H)*/,
                    float* s_dev /*(B*N,H)*/, int32_t H, int32_t D);
int lb_graph_attend_backward(lb_engine* eng, int32_t role, const float* logits_dev, const float* values_dev, const float* m_dev,
                             const float* s_dev, const float* d_out_dev /*(B*N,H*D)*/, float* d_logits_dev /*(B*E_cap,H)*/,
                             float* d_values_dev /*(B*E_cap,H*D)*/, int32_t H, int32_t D);
/* ---- the same ops on float32 OR bfloat16 tensors ("bfloat16") ----------
 * Each entry has the arguments of its fp32 entry above, with void* data pointers and the element type of every data tensor of
 * the call: dtype LB_DTYPE_F32 or LB_DTYPE_BF16 (anything else is LB_ERR_ARG).  win stays int32, m and s of attend stay fp32.
 * The fp32 entries above ARE these with LB_DTYPE_F32.  The contract of LB_DTYPE_BF16, for every op and every backward:
 *
 *     bf16 op  ==  round_to_bf16( fp32 op( upcast(inputs) ) )      bit for bit
 *
 * upcast is the exact bf16 -> fp32 widening; the fp32 op is the arithmetic stated above, unchanged - the same order of adds,
 * the same m, expf, s, division and roundings of products; round_to_bf16 is ONE round-to-nearest-even per stored element
 * (a NaN stays a NaN, payload unspecified; beyond the bf16 range -> +-inf; bf16 subnormals are kept; -0.0 stays -0.0 where
 * the fp32 op keeps it).  So: gather is a bit copy; segment_sum adds the upcast terms in fp32 from the first term in ascending
 * slot order and rounds once - no partial sum is ever held in bf16; segment_max / _min return one of the inputs and
 * the backward copies d_out into the winning slot; segment_softmax stores y = round(e / s), and its backward works on the
 * stored (rounded) y; attend forms alpha in fp32 from the upcast logits, rounds each alpha v to fp32, adds in slot order and
 * rounds once - it does NOT round alpha to bf16 as the composition segment_sum(segment_softmax(l) v) does, and is the more
 * accurate of the two; attend_backward recomputes alpha from m, s and the upcast logits, d_values = round(alpha d_out),
 * d_logits = round(alpha (t - sum alpha t)) with t held in fp32 (a buffer of the engine's).  Pad slots are never read and every
 * pad slot of an edge-shaped output is +0.0 (bf16 bits 0x0000).  16-byte accesses (8 bf16) when C % 8 == 0 and the pointers
 * are 16-byte aligned, single elements otherwise; attend: 16 bytes when D % 8 == 0, 8 bytes when D % 4 == 0. */
#define LB_DTYPE_F32 0
#define LB_DTYPE_BF16 1
int lb_graph_gather_t(lb_engine* eng, int32_t role, const void* x_dev, void* out_dev, int32_t C, int32_t dtype);
int lb_graph_segment_sum_t(lb_engine* eng, int32_t role, const void* msg_dev, void* out_dev, int32_t C, int32_t dtype);
int lb_graph_segment_max_t(lb_engine* eng, int32_t role, const void* msg_dev, void* out_dev, int32_t* win_dev, int32_t C,
                           int32_t dtype);
int lb_graph_segment_min_t(lb_engine* eng, int32_t role, const void* msg_dev, void* out_dev, int32_t* win_dev, int32_t C,
                           int32_t dtype);
int lb_graph_segment_max_backward_t(lb_engine* eng, int32_t role, const void* d_out_dev, const int32_t* win_dev,
                                    void* d_msg_dev, int32_t C, int32_t dtype);
int lb_graph_segment_softmax_t(lb_engine* eng, int32_t role, const void* logits_dev, void* out_dev, int32_t C, int32_t dtype);
int lb_graph_segment_softmax_backward_t(lb_engine* eng, int32_t role, const void* y_dev, const void* d_y_dev, void* d_x_dev,
                                        int32_t C, int32_t dtype);
int lb_graph_attend_t(lb_engine* eng, int32_t role, const void* logits_dev, const void* values_dev, void* out_dev,
                      float* m_dev, float* s_dev, int32_t H, int32_t D, int32_t dtype);
int lb_graph_attend_backward_t(lb_engine* eng, int32_t role, const void* logits_dev, const void* values_dev,
                               const float* m_dev, const float* s_dev, const void* d_out_dev, void* d_logits_dev,
                               void* d_values_dev, int32_t H, int32_t D, int32_t dtype);
/* ---- edge messages: filter x neighbour without edge-shaped intermediates -----
 * The rules above hold: the padded layout, role 0 receivers / 1 senders, pad slots never read (they may hold NaN), every pad
 * slot of an edge-shaped output +0.0, no float atomics, two calls give the same bits, int64 addresses; dtype LB_DTYPE_F32 or
 * LB_DTYPE_BF16 for every data tensor of the call (there are no fp32-only twins).  other(role) is the opposite role; a slot's
 * two nodes are its entries of the engine's compact sender and receiver lists.  Node tensors are (B*N, K, C), K >= 1 rows of C
 * per node; w and the edge-shaped outputs are (B*E_cap, C).  16-byte accesses when C % 4 == 0 (bf16: C % 8 == 0) and the
 * pointers are 16-byte aligned: a unit never crosses a k boundary.  LB_ERR_ARG on a null pointer, a role other than 0 / 1, a
 * dtype other than the two, K < 1 or C < 1; LB_ERR_STATE without a list or with an overflowed one.
 * conv: out[i, k, c] = the sum over the real slots j whose `role` index is i, in ascending slot order (the CSR row for
 *   receivers, the sender view for senders), of fl32(x[other(role) index of j, k, c] * w[j, c]): each product rounded to fp32,
 *   the first product starts the sum, one fp32 add per further one, no FMA contraction; +0.0 for a node without a slot.  With
 *   fp32 tensors bit for bit segment_sum(gather(x, other(role)) * w[:, None, :], role).  Its adjoints: d_x = conv(d_out, w,
 *   other(role)); d_w = pair_mul(other(role), x, d_out) with the K of the call.  Only role 1 builds (or reuses) the sender view.
 * pair_mul: out[j, c] = fl32(a[a_role index of j, 0, c] * b[other(a_role) index of j, 0, c]) + ... over k = 0 .. K-1 ascending,
 *   the first product starts the sum; +0.0 in the pad slots.  K = 1 is the plain product.  Adjoints at K = 1 and a_role 1:
 *   d_a = conv(b, d, 1), d_b = conv(a, d, 0).
 * pair_add: out[j, c] = fl32(a[a_role index of j, c] + b[other(a_role) index of j, c]), a and b (B*N, C); +0.0 in the pad
 *   slots.  Adjoints: the segment sums of d over the two roles.
 * LB_DTYPE_BF16: round_to_bf16(the fp32 op(upcast inputs)), one rounding per stored element.  A product of two bf16 values is
 *   exact in fp32 (8 + 8 significant bits), so conv sums exact products in fp32 and rounds once - it is NOT the composition of
 *   the bf16 ops, which rounds each product to bf16 before it adds; pair_mul's k-sum likewise.  pair_mul at K = 1 and pair_add
 *   equal bf16 arithmetic on the gathered rows. */
int lb_graph_conv(lb_engine* eng, int32_t role, const void* x_dev /*(B*N,K,C)*/, const void* w_dev /*(B*E_cap,C)*/,
                  void* out_dev /*(B*N,K,C)*/, int32_t K, int32_t C, int32_t dtype);
int lb_graph_pair_mul(lb_engine* eng, int32_t a_role, const void* a_dev /*(B*N,K,C)*/, const void* b_dev /*(B*N,K,C)*/,
                      void* out_dev /*(B*E_cap,C)*/, int32_t K, int32_t C, int32_t dtype);
int lb_graph_pair_add(lb_engine* eng, int32_t a_role, const void* a_dev /*(B*N,C)*/, const void* b_dev /*(B*N,C)*/,
                      void* out_dev /*(B*E_cap,C)*/, int32_t C, int32_t dtype);
/* ---- equivariant vector messages: scalar <-> vector channels through a per-edge vector -----
 * The rules of the edge messages hold (layout, roles, pads never read, +0.0 in the pad slots of edge-shaped outputs, no float
 * atomics, two calls the same bits, dtype for every data tensor).  u (B*E_cap, K) is any per-edge vector - rel_disp, or spherical
 * harmonics up to l = 2 -, 1 <= K <= 9, read with scalar loads; x (B*N, C), v (B*N, K, C), w (B*E_cap, C).  o(j) is the
 * other(role) node of slot j, n(j) its `role` node.  Every product is one fp32 multiplication, every add one fp32 add, no FMA
 * contraction.  LB_ERR_ARG on a null pointer, a role other than 0 / 1, a dtype other than the two, K < 1, K > 9 or C < 1.
 * conv_vec: out[i, k, c] = the sum over the real slots j with n(j) = i, ascending, of fl32(fl32(x[o(j), c] * w[j, c]) * u[j, k]);
 *   the first term starts the sum, +0.0 for a node without a slot.  With fp32 tensors bit for bit
 *   segment_sum((gather(x, other(role)) * w)[:, None, :] * u[:, :, None], role).
 * conv_dot: t[j, c] = fl32(v[o(j), 0, c] * u[j, 0]) + fl32(v[o(j), 1, c] * u[j, 1]) + ... (k ascending, the first product starts
 *   the sum); out[i, c] = the sum over the real slots j with n(j) = i, ascending, of fl32(w[j, c] * t[j, c]).  With fp32 tensors
 *   bit for bit segment_sum(w * t, role) with t added k by k from gather(v, other(role))[:, k] * u[:, k:k+1].
 * Adjoints: d_x of conv_vec over role = conv_dot(d_out, w, u, other(role)); d_v of conv_dot over role = conv_vec(d_out, w, u,
 *   other(role)) - the same kernels, the same bits.
 * conv_vec_edge_grad: the gradients to w and u of both ops from a scalar-side node tensor S (B*N, C), read at the slot's s_role
 *   node, and a vector-side one V (B*N, K, C), read at its other node - conv_vec over role: S = x, s_role = other(role), V =
 *   d_out; conv_dot over role: S = d_out, s_role = role, V = v:
 *     d_w[j, c] = fl32(S[c] * t[j, c]), t formed from V and u as in conv_dot;
 *     d_u[j, k] = sum over c of fl32(fl32(S[c] * w[j, c]) * V[k, c]) in a FIXED order: the columns in consecutive blocks of
 *       LB_GRAPH_DU_BLOCK (the last may be short), inside a block c ascending and the first product starts the sum, then the
 *       block sums added in ascending block order from the first one.  The order does not depend on C's divisibility, the
 *       pointers' alignment or the dtype; a numpy loop reproduces it.
 *   Either of d_w_dev (B*E_cap, C) and d_u_dev (B*E_cap, K) may be null: that gradient is not computed (both null: LB_ERR_ARG).
 * LB_DTYPE_BF16: round_to_bf16(the fp32 op(upcast inputs)), one rounding per stored element, d_u included; no partial result is
 *   held in bf16, so neither op is the composition of the bf16 ops. */
#define LB_GRAPH_DU_BLOCK 16
int lb_graph_conv_vec(lb_engine* eng, int32_t role, const void* x_dev /*(B*N,C)*/, const void* w_dev /*(B*E_cap,C)*/,
                      const void* u_dev /*(B*E_cap,K)*/, void* out_dev /*(B*N,K,C)*/, int32_t K, int32_t C, int32_t dtype);
int lb_graph_conv_dot(lb_engine* eng, int32_t role, const void* v_dev /*(B*N,K,C)*/, const void* w_dev /*(B*E_cap,C)*/,
                      const void* u_dev /*(B*E_cap,K)*/, void* out_dev /*(B*N,C)*/, int32_t K, int32_t C, int32_t dtype);
int lb_graph_conv_vec_edge_grad(lb_engine* eng, int32_t s_role, const void* s_dev /*(B*N,C)*/, const void* v_dev /*(B*N,K,C)*/,
                                const void* w_dev /*(B*E_cap,C)*/, const void* u_dev /*(B*E_cap,K)*/,
                                void* d_w_dev /*(B*E_cap,C) or NULL*/, void* d_u_dev /*(B*E_cap,K) or NULL*/, int32_t K, int32_t C,
                                int32_t dtype);
/* ---- filter_conv: conv with its one-Linear filter formed in registers -----
 * The rules of the edge messages hold (layout, roles, pads never read - the pad slots of f may hold NaN -, +0.0 in the pad slots of
 * edge-shaped outputs, no float atomics, two calls the same bits, dtype for every data tensor, weight included).  x (B*N, K, C),
 * f (B*E_cap, R) any per-edge basis, weight (R, C) shared by the batch, 1 <= R <= LB_GRAPH_MAX_R.  o(j) is the other(role) node
 * of slot j, n(j) its `role` node.  Every product is one fp32 multiplication, every add one fp32 add, no FMA contraction.
 * The filter, never stored: wf[j, c] = fl32(f[j, 0] * weight[0, c]) + fl32(f[j, 1] * weight[1, c]) + ..., r ascending, the first
 *   product starts the sum.
 * filter_conv: out[i, k, c] = the sum over the real slots j with n(j) = i, ascending, of fl32(x[o(j), k, c] * wf[j, c]); the first
 *   term starts the sum, +0.0 for a node without a slot: with fp32 tensors bit for bit lb_graph_conv on wf.  Its adjoint:
 *   d_x = filter_conv(d_out, f, weight, other(role)).
 * filter_conv_grad (role: the forward's), from g[j, c] = fl32(x[o(j), 0, c] * d[n(j), 0, c]) + fl32(x[o(j), 1, c] * d[n(j), 1, c])
 *   + ... (k ascending, the first product starts the sum: conv's d_w), never stored:
 *     d_f[j, r] = the sum over c of fl32(weight[r, c] * g[j, c]) in the order of LB_GRAPH_DU_BLOCK (blocks of consecutive columns,
 *       c ascending inside a block from its first product, the block sums added in ascending order from the first one); +0.0 in
 *       the pad slots;
 *     d_weight[r, c] = the sum over every real slot of every trajectory of fl32(f[j, r] * g[j, c]) in a two-level order: the flat
 *       padded slots b * E_cap + j in consecutive chunks of LB_GRAPH_FILTER_CHUNK; per chunk a partial sum that starts at +0.0
 *       and takes the terms of the chunk's real slots in ascending order (a chunk of pads keeps +0.0); the total starts at +0.0
 *       and takes the partials in ascending chunk order.  A numpy loop reproduces it.
 *   Either of d_f_dev (B*E_cap, R) and d_weight_dev (R, C) may be null: that gradient is not computed (both null: LB_ERR_ARG).
 *   With d_weight_dev the caller gives partials_dev, fp32 scratch of at least lb_graph_filter_partials(eng, R, C) =
 *   ceil(B*E_cap / LB_GRAPH_FILTER_CHUNK) * R * C elements (partials_len: what it holds); nothing else is allocated, and nothing of
 *   E_cap x C elements exists.  One launch for d_f, two for d_weight (the partials, the ordered finish).
 * LB_DTYPE_BF16: every output, d_f and d_weight included, is round_to_bf16(the fp32 result on the widened inputs), one rounding
 *   per stored element; wf and g stay fp32.
 * LB_ERR_ARG on a null required pointer, a role other than 0 / 1, a dtype other than the two, K < 1, R < 1, R > LB_GRAPH_MAX_R,
 *   C < 1 or partials too short; LB_ERR_STATE without a list or with an overflowed one. */
#define LB_GRAPH_MAX_R 32
#define LB_GRAPH_FILTER_CHUNK 256
int lb_graph_filter_conv(lb_engine* eng, int32_t role, const void* x_dev /*(B*N,K,C)*/, const void* f_dev /*(B*E_cap,R)*/,
                         const void* weight_dev /*(R,C)*/, void* out_dev /*(B*N,K,C)*/, int32_t K, int32_t R, int32_t C,
                         int32_t dtype);
int lb_graph_filter_conv_grad(lb_engine* eng, int32_t role, const void* x_dev /*(B*N,K,C)*/, const void* d_dev /*(B*N,K,C)*/,
                              const void* f_dev /*(B*E_cap,R)*/, const void* weight_dev /*(R,C)*/,
                              void* d_f_dev /*(B*E_cap,R) or NULL*/, void* d_weight_dev /*(R,C) or NULL*/,
                              float* partials_dev /*NULL without d_weight*/, int64_t partials_len, int32_t K, int32_t R, int32_t C,
                              int32_t dtype);
/* elements of the fp32 partials of lb_graph_filter_conv_grad on the engine's current E_cap; 0 without a list or on bad sizes */
int64_t lb_graph_filter_partials(lb_engine* eng, int32_t R, int32_t C);
/* ---- the multi-aggregator: sum, mean, max, min, std and var of one message in one launch -----
 * The rules of the graph ops hold (layout, roles, pads never read, +0.0 in the pad slots of edge-shaped outputs, no float atomics,
 * two calls the same bits, dtype for every data tensor).  msg (B*E_cap, C) -> out (B*N, A, C): plane a holds the op whose code
 * LB_AGG_* stands in nibble a of `ops`, from the low end; a 0 nibble ends the list, A is the number of codes before it.  Per
 * node i and column c, with the real slots j1 < ... < jd of `role` in ascending slot order and d the degree:
 *   sum:  x_j1 + x_j2 + ... - the first term starts the sum, one fp32 add per further slot: the bits of lb_graph_segment_sum;
 *   mean: m = fl32(sum / max(d, 1)), one correctly rounded division;
 *   max, min: the first slot, replaced only by a strictly greater / smaller one (ties keep the earlier slot, a NaN wins and
 *         stays): the bits and the winning slots of lb_graph_segment_max / _min;
 *   var:  fl32(q / max(d, 1)), centred and two-pass: t_j = fl32(x_j - m), q = the ordered fp32 sum of fl32(t_j t_j), the first
 *         term starting it - never E[x^2] - m^2;
 *   std:  sqrt_rn(fl32(var + eps)), eps inside the root.
 * A node without slots gets +0.0 in every plane, std included.  Every step is one correctly rounded IEEE operation (no FMA
 * contraction), so a numpy float32 loop reproduces the planes bit for bit.
 * Side outputs for the backward, required only when an op that needs them is in `ops` (else they may be NULL and are not
 * touched): win (B*N, 2, C) int32 - the winning slot within the trajectory of the max, then of the min, -1 for a node without
 * slots - with max or min; stats (B*N, 2, C) fp32 - m, then std (+0.0 when std is not in `ops`) - with std or var.
 * Backward: d_msg (B*E_cap, C), +0.0 in the pad slots; for a real slot j of node n the PRESENT terms in this fixed order,
 * whatever the order of `ops`, the first present one starting the sum: g_sum; fl32(g_mean / d); g_max if j is the max winner
 * of (n, c); g_min likewise; fl32(fl32(g_std t_j) / fl32(d std)); fl32(fl32(fl32(2 g_var) t_j) / d) - t_j recomputed from msg
 * and the saved m.  A real slot with no present term gets +0.0.  msg_dev and stats_dev are required with std or var, win_dev
 * with max or min.
 * LB_DTYPE_BF16: out and d_msg are round_to_bf16(the fp32 result on the widened inputs), one rounding per stored element; stats
 * stay fp32, so the mean inside var and in the backward is the fp32 mean, not its rounded copy.
 * LB_ERR_ARG on a null handle, a null required pointer, a role other than 0 / 1, a dtype other than the two, C < 1, an `ops`
 * word that is empty, repeats a code, holds a code above LB_AGG_VAR or a code after the end, or eps <= 0 with std (forward);
 * LB_ERR_STATE without a list or with an overflowed one. */
#define LB_AGG_SUM 1
#define LB_AGG_MEAN 2
#define LB_AGG_MAX 3
#define LB_AGG_MIN 4
#define LB_AGG_STD 5
#define LB_AGG_VAR 6
int lb_graph_aggregate(lb_engine* eng, int32_t role, const void* msg_dev /*(B*E_cap,C)*/, void* out_dev /*(B*N,A,C)*/,
                       int32_t* win_dev /*(B*N,2,C) or NULL*/, float* stats_dev /*(B*N,2,C) or NULL*/, int32_t C, int32_t ops,
                       float eps, int32_t dtype);
int lb_graph_aggregate_backward(lb_engine* eng, int32_t role, const void* d_out_dev /*(B*N,A,C)*/,
                                const void* msg_dev /*(B*E_cap,C) or NULL*/, const int32_t* win_dev /*(B*N,2,C) or NULL*/,
                                const float* stats_dev /*(B*N,2,C) or NULL*/, void* d_msg_dev /*(B*E_cap,C)*/, int32_t C,
                                int32_t ops, int32_t dtype);
/* ---- edge pairs: an edge beside its transpose -----
 * The rules of the graph ops hold (the padded layout, pads never read, +0.0 in the pad slots of edge-shaped outputs, no atomics,
 * two calls the same bits, int64 addresses).
 * reverse: out (B*E_cap) int32.  For the real slot j of (receiver r, sender s) the slot, within its trajectory, of the edge
 *   (receiver s, sender r) of the same trajectory; a self-edge maps to itself; -1 where the list holds no such edge (the periodic
 *   displacement is antisymmetric only up to one rounding, so a pair at the cutoff can be an edge in one direction only) and -1
 *   in every pad slot.  So out[out[j]] == j wherever out[j] >= 0.  The engine builds the map at its first use after a list
 *   build - one edge-parallel launch that bisects the sender's CSR row (a row holds a sender at most once), nothing read back,
 *   independent of the sender view - keeps it in its arena and copies it out here.
 * edge_pair_t: msg, out (B*E_cap, C), out != msg; p(j) = reverse[j]:
 *   LB_GRAPH_PAIR_SWAP     out[j, c] = msg[p(j), c], a bit copy;
 *   LB_GRAPH_PAIR_SYM      out[j, c] = fl32(msg[j, c] + msg[p(j), c]);
 *   LB_GRAPH_PAIR_ANTISYM  out[j, c] = fl32(msg[j, c] - msg[p(j), c]);
 *   a slot without a partner (p(j) = -1) gets +0.0 in every mode - an edge without its transpose takes no part, so the result is
 *   an exactly symmetric / antisymmetric edge field on every list -, and so does every pad slot.  A self-edge: fl32(m + m), and
 *   +0.0 for a finite m under ANTISYM.  Each mode is its own adjoint (ANTISYM: d_msg = ANTISYM(d_out), the two signs cancel), so
 *   the backward is the same call on the cotangent.  LB_DTYPE_BF16: round_to_bf16(the fp32 op(upcast inputs)), rounded once;
 *   SWAP copies the 16 bits.  16-byte accesses when C % 4 == 0 (bf16: C % 8 == 0) and both pointers are 16-byte aligned.
 * LB_ERR_ARG on a null pointer, a mode or dtype other than those named, C < 1, out == msg; LB_ERR_STATE without a list or with an
 *   overflowed one. */
#define LB_GRAPH_PAIR_SWAP 0
#define LB_GRAPH_PAIR_SYM 1
#define LB_GRAPH_PAIR_ANTISYM 2
int lb_graph_reverse(lb_engine* eng, int32_t* out_dev /*(B*E_cap)*/);
int lb_graph_edge_pair_t(lb_engine* eng, int32_t mode, const void* msg_dev /*(B*E_cap,C)*/, void* out_dev /*(B*E_cap,C)*/,
                         int32_t C, int32_t dtype);
/* d loss / d window from the cotangents of the features a TorchModel module receives (graph.differentiable_features), on the
 * engine's CURRENT window and list: the transpose of the feature builder.  Every input may be NULL (= zero).  fp32 inputs in the
 * layouts of TorchModel's feature dict; the edge-shaped ones in the padded slot layout of lb_nl_read_idx, whose pad slots are
 * never read (they may hold NaN).  vel_hist: g / std to the later frame of each velocity, -g / std to the earlier (the periodic
 * displacement has derivative 1); vel_mag: the same path with g = d_vel_mag vn / |vn| (0 where |vn| = 0); bound: +-d / r_c on
 * the newest frame where the feature lies strictly inside (-1, 1); per edge h = (d_rel_disp + d_rel_dist rel_disp / rel_dist) /
 * r_c (second term 0 where rel_dist = 0), +h to the receiver's newest frame, -h to the sender's (the cached sender view); the
 * external force is a constant of the positions; d_abs_pos is added term by term; rows of pad particles are 0.  Forward values:
 * rel_disp / rel_dist from the engine's fp32 edge features, the node values recomputed from the fp64 window and rounded to
 * fp32.  Every sum in fp64 over terms formed from the fp32 inputs, in a fixed order - frames ascending (velocities, then
 * d_abs_pos); on the newest frame the walls, the receiver row in ascending slot order, the sent edges in ascending sender-view
 * order - without atomics: two calls give the same bits, and a call with every input NULL writes +0.0 everywhere.
 * LB_ERR_UNSUPPORTED on an engine with float32 geometry; LB_ERR_STATE as for the other graph ops. */
int lb_graph_features_backward(lb_engine* eng,
    const float* d_abs_pos,   /* (B*N, isl, dim)            identity                                    */
    const float* d_vel_hist,  /* (B*N, (isl-1)*dim)                                                     */
    const float* d_vel_mag,   /* (B*N, isl-1)      LB_ERR_ARG if non-null and the engine has no vel_mag */
    const float* d_bound,     /* (B*N, 2*dim)      LB_ERR_ARG if non-null and the engine has no bound   */
    const float* d_rel_disp,  /* (B*E_cap, dim)    padded slot layout of lb_nl_read_idx                 */
    const float* d_rel_dist,  /* (B*E_cap, 1)                                                           */
    double* d_window_out);    /* (B*N, isl, dim) fp64, overwritten                                      */
/* Test support / diagnostics, like lb_gns_train_sort_fallbacks: sender views built by the radix sort since the engine was
 * created (a list with an edge in one direction only).  Nothing in the package depends on it. */
int32_t lb_graph_sender_sorts(lb_engine* eng);

#ifdef __cplusplus
}
#endif
#endif /* LBHIP_H */
