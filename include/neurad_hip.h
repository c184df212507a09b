/*
 * neurad_hip.h -- C ABI of libneurad_hip.so: NeuRAD's volumetric ray-marching hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary for the path named by BASELINE.json:north_star.  Every entry point
 * replaces one reference interface (cited as file:line relative to the neurad-studio tree); the
 * reference-side binding (ctypes) a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - All data pointers are DEVICE pointers (HBM) unless the comment says "host".  Buffers are owned by
 *    the caller (PyTorch allocates them); the library never allocates, frees or retains device memory.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Every call only enqueues
 *    kernels on that stream; nothing synchronises the device.
 *  - Return value: 0 = NRHIP_OK, otherwise an NRHIP_ERR_* code; nrhip_last_error() returns a
 *    thread-local human-readable message for the last failing call on this thread.
 *  - Floating point is fp32 end to end (the parity target is the reference's implementation="torch"
 *    path).  Hash tables may be stored as fp32 (param_dtype 0) or fp16 (param_dtype 1, BASELINE config 5).
 *  - Hash tables handed to a lookup (nrhip_hashgrid_fwd, nrhip_encode_fwd, nrhip_proposal_density_fwd) must be 16-byte
 *    aligned: entries are fetched with vector loads of up to 16 bytes.  An fp32 table with 1 feature per level must have
 *    log2_table_size >= 2 there (its corners are read as aligned 4-entry blocks).  Both are checked on the host:
 *    NRHIP_ERR_INVALID_ARG for the alignment, NRHIP_ERR_UNSUPPORTED for the size.
 *  - Row-major, innermost dimension last.  R = rays, S = samples per ray, N = R*S, L = levels,
 *    F = features per level, T = 2^log2_table_size entries per level.
 */
#ifndef NEURAD_HIP_H_
#define NEURAD_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRHIP_OK 0
#define NRHIP_ERR_INVALID_ARG 1  /* bad size / NULL pointer / unsupported configuration */
#define NRHIP_ERR_UNSUPPORTED 2  /* configuration outside what the kernels are instantiated for */
#define NRHIP_ERR_LAUNCH 3       /* hipLaunchKernel / hipGetLastError failure */

#define NRHIP_MAX_LEVELS 32
#define NRHIP_MAX_LAYERS 8

/* ---- descriptors (plain C structs, passed by pointer from host memory) ------------------------- */

/* Multi-resolution hash grid == HashEncoding(implementation="torch")
 * (nerfstudio/field_components/encodings.py:326-384).  scalings[l] = floor(min_res * g^l) is computed
 * by the host exactly as encodings.py:348-350 does, so the device never re-derives it.           */
typedef struct {
  int32_t num_levels;       /* L  */
  int32_t n_features;       /* F in {1,2,4,8} */
  int32_t log2_table_size;  /* T = 1 << log2_table_size (per level) */
  int32_t param_dtype;      /* 0 = fp32 table, 1 = fp16 table */
  float scalings[NRHIP_MAX_LEVELS];
} nrhip_grid;

/* MLP == MLP.pytorch_fwd (nerfstudio/field_components/mlp.py:142-178): Linear(+bias)+ReLU ... Linear.
 * weight[k] is nn.Linear.weight of layer k ([out_k][in_k] row-major), bias[k] may be NULL.         */
typedef struct {
  int32_t in_dim;
  int32_t hidden_dim;
  int32_t out_dim;
  int32_t num_layers;       /* number of Linear layers (>= 1) */
  const float* weight[NRHIP_MAX_LAYERS];
  const float* bias[NRHIP_MAX_LAYERS];
} nrhip_mlp;

/* A ray batch == the per-ray part of RayBundle/Frustums (nerfstudio/cameras/rays.py:33-59,251-357).
 * Samples are described by per-ray origin/direction and per-sample [start,end]; the materialised
 * [R,S,3] broadcast views of rays.py:336-355 are never built.                                       */
typedef struct {
  int64_t n_rays;           /* R */
  int32_t n_samples;        /* S */
  const float* origins;     /* [R,3] */
  const float* directions;  /* [R,3] */
  const float* pixel_area;  /* [R]   */
  const float* starts;      /* [R,S] euclidean bin starts */
  const float* ends;        /* [R,S] euclidean bin ends   */
  int32_t sample_stride;    /* row stride (floats) of starts/ends; 0 = S.  With bin EDGES e[R,S+1] pass
                               starts = e, ends = e + 1, sample_stride = S + 1 (no copies).            */
  const int32_t* order;     /* optional [R] permutation (NULL = batch order): the ORDER in which the fused kernels
                               (nrhip_field_fwd*, nrhip_render_fwd*) walk the rays -- a cache-locality hint from
                               nrhip_ray_order; every output stays indexed by the ray's own position in the batch,
                               results do not depend on it.  Other entry points ignore it.                      */
} nrhip_rays;

/* NeuRADField (nerfstudio/fields/neurad_field.py:78-152), static scene part.
 *   geo:  L*F -> hidden -> 1 + geo_feat_dim   (neurad_field.py:98-106)
 *   feat: geo_feat_dim + 16 (SH deg 4) -> hidden ... -> geo_feat_dim  (neurad_field.py:109-117)
 * The fused field kernels (nrhip_field_fwd*, nrhip_render_fwd*) are instantiated for the (L, F, hidden width) listed in
 * csrc/render_variants.h (static scene: its Static rows; with actors: its Actors / Overrides rows); anything else is
 * NRHIP_ERR_UNSUPPORTED.  Every encoding-wide tensor is dense [*, L*F]: geo.weight[0] [H, L*F], save_enc, the override
 * rows.   */
typedef struct {
  nrhip_grid grid;
  const void* table;        /* [L*T, F] level-major rows (encodings.py:382-384) */
  float static_scale;       /* ScaledSceneContraction scale (neurad_encoding.py:99) */
  nrhip_mlp geo;
  nrhip_mlp feat;
  int32_t use_sdf;          /* 1: ALPHA = sigmoid(-sdf*beta) ; 0: DENSITY = exp(geo_out) */
  float beta;               /* |beta| + beta_min already applied (model_components/utils.py:38-41) */
  /* Optional, inference only (both NULL = off): the table re-laid out by nrhip_eval_layout_build and its description
   * from nrhip_eval_layout_plan (HOST array [L][4]).  nrhip_render_fwd* then reads the coarse levels from their shadow
   * copies; outputs are bit-identical to the plain table's.  A cache of the caller: rebuild after a parameter change. */
  const void* eval_table;
  const uint32_t* eval_layout;
} nrhip_field;

/* NeuRADProposalField (nerfstudio/fields/neurad_field.py:182-216): grid -> Linear(L*F,1,no bias) -> exp */
typedef struct {
  nrhip_grid grid;
  const void* table;
  float static_scale;
  const float* decoder_weight; /* [L*F] */
} nrhip_proposal;

/* ---- library ---------------------------------------------------------------------------------- */
const char* nrhip_last_error(void);
int nrhip_version(void);
/* number of CUs / XCDs of the current device (host out-pointers) */
int nrhip_device_info(int32_t* n_cus, int32_t* n_xcds, int64_t* hbm_bytes);
/* The library's A/B switches (NRHIP_* environment variables, csrc/common.h: struct Tuning) are read once, when the library is
 * loaded; a process that changes one afterwards calls this to have them read again.  Every switch selects between two
 * implementations of the same result. */
int nrhip_tuning_reload(void);

/* ---- eval-time layout of the coarse levels (csrc/eval_layout.hip) ----------------------------------------------
 * Levels whose lattice (0 .. ceil(scalings[l]))^3, padded to 2^s per axis, fits the table size are copied into a shadow
 * region indexed ix | iy << s | iz << 2s (8 corners in 4 cache lines, neighbours share lines); the others keep the
 * reference hash (encodings.py:419-444).  plan: layout [L][4] = {mulY, mulZ, mask, row0} per level and the eval table's
 * row count (host outputs, no GPU needed); build: fills eval_table [rows, F] (table's dtype) from the table.        */
int nrhip_eval_layout_plan(const nrhip_grid* g, uint32_t* layout /*host [L*4]*/, int64_t* rows /*host*/);
int nrhip_eval_layout_build(const nrhip_grid* g, const void* table, const uint32_t* layout /*host*/, void* eval_table,
                            void* stream);

/* ---- H1: hash grid (replaces HashEncoding.pytorch_fwd, encodings.py:425-466; tcnn.Encoding
 *          {otype:"HashGrid"} call sites encodings.py:362-373,468-471) --------------------------- */
int nrhip_hashgrid_fwd(const nrhip_grid* g, const void* table, const float* x /*[N,3] in [0,1]*/, int64_t n,
                       float* out /*[N,L*F]*/, void* stream);
/* grad_table [L*T,F] fp32 is ACCUMULATED into (caller zeroes it): autograd of encodings.py:446-464 */
int nrhip_hashgrid_bwd(const nrhip_grid* g, const float* x, const float* grad_out /*[N,L*F]*/, int64_t n,
                       float* grad_table, void* stream);

/* dL/dx of the lookup (fp32 table): only actor-hit samples need it */
int nrhip_hashgrid_bwd_input(const nrhip_grid* g, const void* table, const float* x, const float* grad_out, int64_t n,
                             float* grad_x /*[N,3]*/, void* stream);

/* Several grids of one shape in one launch -- the per-actor grids of NeuRADHashEncoding (the reference loops over
 * actor ids, `_get_actor_features_slow`, neurad_encoding.py:270-295).  tables / grad_tables: DEVICE arrays of n_grids
 * pointers to [L*T,F] fp32 tables; grid_id [N] int32 selects the grid of each sample.  grad_tables are ACCUMULATED
 * into; a sample whose grid_id is outside [0, n_grids) or whose grad_tables entry is NULL sends nothing (ABI 511; the
 * forward and _bwd_input need valid ids). */
int nrhip_hashgrid_multi_fwd(const nrhip_grid* g, const void* const* tables, int32_t n_grids, const int32_t* grid_id,
                             const float* x /*[N,3]*/, int64_t n, float* out /*[N,L*F]*/, void* stream);
int nrhip_hashgrid_multi_bwd(const nrhip_grid* g, int32_t n_grids, const int32_t* grid_id, const float* x,
                             const float* grad_out, int64_t n, float* const* grad_tables, void* stream);
/* The same table gradients WITHOUT memory-side atomics (ABI 511): the radix partition of nrhip_encode_bwd_binned over
 * (slot, level, slice) -- the gradients of the n_slots grids that have samples form ONE block [n_slots][L*T][F] (fp32, or
 * fp16 for fp16-storage grids: block_dtype 1, at most 2^23 samples), EVERY element of which is written (no zero-fill by
 * the caller).  slot_of [n_grids] int32 DEVICE: the grid's position in the block, < 0 = no gradient wanted (its samples
 * send nothing, like samples with grid_id outside [0, n_grids)).  Same sums as nrhip_hashgrid_multi_bwd up to the order of
 * the fp32 additions (this one is bit-reproducible).  _workspace gives 0 bytes when the shape cannot be partitioned
 * (n_slots x T / slice length > 2048 columns per level): use the atomic entry point then. */
int nrhip_hashgrid_multi_bwd_binned_workspace(const nrhip_grid* g, int32_t n_slots, int64_t n, int64_t* bytes /*host*/);
int nrhip_hashgrid_multi_bwd_binned(const nrhip_grid* g, int32_t n_grids, const int32_t* grid_id, const int32_t* slot_of,
                                    int32_t n_slots, const float* x /*[N,3]*/, const float* grad_out /*[N,L*F]*/, int64_t n,
                                    void* grad_block, int32_t block_dtype, void* workspace, int64_t workspace_bytes,
                                    void* stream);
int nrhip_hashgrid_multi_bwd_input(const nrhip_grid* g, const void* const* tables, int32_t n_grids,
                                   const int32_t* grid_id, const float* x, const float* grad_out, int64_t n,
                                   float* grad_x /*[N,3]*/, void* stream);

/* ---- H2+H3+H1+H4: NeuRADHashEncoding static path (neurad_encoding.py:164-169,265-268,297-304;
 *      cameras/rays.py:109-124; spatial_distortions.py:103-141) --------------------------------- */
int nrhip_encode_fwd(const nrhip_grid* g, const void* table, float static_scale, const nrhip_rays* rays,
                     float* out /*[N,L*F]*/, void* stream);
int nrhip_encode_bwd(const nrhip_grid* g, float static_scale, const nrhip_rays* rays,
                     const float* grad_out /*[N,L*F]*/, float* grad_table, void* stream);
/* dL/d(origins) [R,3] and dL/d(directions) [R,3] (both WRITTEN) of the same path given grad_out [N,L*F] = dL/d(rescaled
 * features): what autograd hands a camera optimizer that moves the rays (cameras/camera_optimizers.py:173-182,
 * apply_to_raybundle; the `*-scaleopt` methods, configs/method_configs.py:438-447) -- mean = o + d t (cameras/rays.py:119,
 * t constant: bins are detached, ray_samplers.py:363-364) -> contraction of mean AND std (spatial_distortions.py:126-141)
 * -> trilinear offsets (encodings.py:425-464) and the std-dependent rescale (neurad_encoding.py:297-304).  No atomics. */
int nrhip_encode_bwd_rays(const nrhip_grid* g, const void* table, float static_scale, const nrhip_rays* rays,
                          const float* grad_out /*[N,L*F]*/, float* grad_origins, float* grad_directions, void* stream);
/* Same result without memory-side atomics (every table entry gets one owning workgroup; see
 * csrc/encode_bwd_binned.hip).  Needs scratch: ask _workspace for the size (0 = this grid can not be binned, use
 * nrhip_encode_bwd), hand in a 16-byte aligned device buffer of at least that many bytes.  overwrite = 0: grad_table
 * is ACCUMULATED into, as above; overwrite = 1: every element of grad_table is WRITTEN (no zero-fill needed before,
 * and the pass over the table is a store instead of a read-modify-write). */
/* grad_table of the _binned entry points is ALWAYS fp32 [L*T,F]; g->param_dtype keeps its meaning (the TABLE's storage type)
 * and is not looked at (the partition never reads the table).  (ABI 500 read it as the gradient's type; 510 does not: a caller
 * that passes the descriptor of its fp16-storage table together with an fp32 grad_table gets fp32 again.)
 * nrhip_encode_bwd_binned_f16 writes the gradient as fp16 [L*T,F] instead -- the dtype autograd wants for an fp16-storage
 * table, without an fp32 image and a cast pass: every element is WRITTEN (overwrite semantics), at most 2^23 samples (one
 * round), NRHIP_ERR_UNSUPPORTED otherwise. */
int nrhip_encode_bwd_binned_workspace(const nrhip_grid* g, int64_t n_samples, int64_t* bytes);
/* The same scratch size serves the two other table gradients below (it depends on the grid and the sample count
 * only): nrhip_hashgrid_bwd_binned == nrhip_hashgrid_bwd, nrhip_proposal_density_bwd_binned ==
 * nrhip_proposal_density_bwd, without memory-side atomics. */
int nrhip_hashgrid_bwd_binned(const nrhip_grid* g, const float* x, const float* grad_out /*[N,L*F]*/, int64_t n,
                              float* grad_table, int32_t overwrite, void* workspace, int64_t workspace_bytes,
                              void* stream);
int nrhip_encode_bwd_binned(const nrhip_grid* g, float static_scale, const nrhip_rays* rays,
                            const float* grad_out /*[N,L*F]*/, float* grad_table, int32_t overwrite, void* workspace,
                            int64_t workspace_bytes, void* stream);
int nrhip_encode_bwd_binned_f16(const nrhip_grid* g, float static_scale, const nrhip_rays* rays,
                                const float* grad_out /*[N,L*F]*/, void* grad_table_fp16, void* workspace,
                                int64_t workspace_bytes, void* stream);

/* ---- F3: SHEncoding(levels=4) (encodings.py:797-805 -> utils/math.py:31-94) -------------------- */
int nrhip_sh4_fwd(const float* dirs /*[N,3]*/, int64_t n, float* out /*[N,16]*/, void* stream);

/* ---- F2: MLP (mlp.py:142-183; tcnn.Network call sites mlp.py:102-113,180-183) ------------------
 * hidden (optional, may be NULL): [N, (num_layers-1)*hidden_dim] post-ReLU activations, saved for bwd */
int nrhip_mlp_fwd(const nrhip_mlp* m, const float* x /*[N,in]*/, int64_t n, float* y /*[N,out]*/,
                  float* hidden, void* stream);
/* Backward.  grad_x may be NULL.  grad_weight[k] ([out_k][in_k]) and grad_bias[k] (may be NULL) are
 * ACCUMULATED into.  workspace: at least N*(num_layers-1)*hidden_dim floats (dZ of the hidden layers); with the
 * nrhip_mlp_bwd_workspace() amount NeuRAD's own MLP shapes get their weight gradients from the same pass as the
 * data gradient (no second read of the activations, no atomics). */
int nrhip_mlp_bwd_workspace(const nrhip_mlp* m, int64_t n, int64_t* floats);
int nrhip_mlp_bwd(const nrhip_mlp* m, const float* x, const float* hidden, const float* grad_y, int64_t n,
                  float* grad_x, float* const* grad_weight /*host array*/, float* const* grad_bias /*host array*/,
                  float* workspace, int64_t workspace_floats, void* stream);
/* Backward of NeuRADField's feature head, feature = geo[:, 1:] + mlp_feature([geo[:, 1:] | sh]) (neurad_field.py:146-152),
 * in one pass: the feature MLP's weight / bias gradients as nrhip_mlp_bwd forms them (x [N,48] = (embedding | sh), hidden,
 * workspace as there, sized by nrhip_mlp_bwd_workspace), and -- instead of grad_x -- the geometry MLP's complete output
 * gradient grad_geo [N,33]: column 0 = grad_geo0[n] (the sdf / density logit's gradient), columns 1..32 = grad_feature +
 * the embedding columns of grad_x (the residual connection).  The sh columns' gradient has no consumer and is not formed.
 * Covers the feature head's shapes 48 -> {32,64} -> {32,64} -> 32; pointers 16-byte aligned. */
int nrhip_field_feature_bwd(const nrhip_mlp* m, const float* x, const float* hidden, const float* grad_feature /*[N,32]*/,
                            const float* grad_geo0 /*[N]*/, int64_t n, float* grad_geo /*[N,33]*/,
                            float* const* grad_weight, float* const* grad_bias, float* workspace, int64_t workspace_floats,
                            void* stream);

/* ---- F1+F4: NeuRADField.forward, per-sample outputs (neurad_field.py:128-152) ------------------
 * feature [R,S,C], sdf_or_raw [R,S] (sdf when use_sdf else the pre-exp geo output), alpha_or_density [R,S] */
int nrhip_field_fwd(const nrhip_field* f, const nrhip_rays* rays, float* feature, float* sdf, float* alpha,
                    void* stream);
/* Training forward: the same kernel, additionally storing what nrhip_mlp_bwd / nrhip_encode_bwd* need, in their
 * layouts (N = R*S, H = hidden width, all 16-byte aligned):  save_enc [N,L*F] rescaled grid features (geometry MLP
 * input), save_geo_hidden [N,H], save_feat_in [N,48] = geometry embedding | SH(direction) (feature MLP input),
 * save_feat_hidden [N,2H] = layer 0 | layer 1.  Replaces encode_fwd + 2x mlp_fwd + sh4 + concat of the operator path. */
int nrhip_field_fwd_train(const nrhip_field* f, const nrhip_rays* rays, float* feature, float* sdf, float* alpha,
                          float* save_enc, float* save_geo_hidden, float* save_feat_in, float* save_feat_hidden,
                          void* stream);
/* The same with ROW OVERRIDES -- the training forward of a scene with dynamic actors (neurad_encoding.py:150-187): a
 * sample with ovr_row[i] = p >= 0 (i = ray * S + sample) takes its encoding row from ovr_rows [P,L*F] (the actor grid's
 * rescaled features, zero-padded, computed by the differentiable actor branch for the few samples inside a box) and the
 * view direction of its SH inputs from ovr_dirs [P,3] (box frame, neurad_encoding.py:203-208) instead of the static
 * lookup and the ray direction; ovr_row[i] = -1: the static scene.  save_enc then holds the overriding rows, so the
 * backward's d/d enc of those samples is the gradient of ovr_rows.  fp32 and fp16 static tables. */
int nrhip_field_fwd_train_ovr(const nrhip_field* f, const nrhip_rays* rays, const int32_t* ovr_row, const float* ovr_rows,
                              const float* ovr_dirs, float* feature, float* sdf, float* alpha, float* save_enc,
                              float* save_geo_hidden, float* save_feat_in, float* save_feat_hidden, void* stream);

/* ---- C1: nerfacc 0.5.2 dense-mode (call sites models/neurad.py:716-723,734; renderers.py:88,345) */
int nrhip_render_weight_from_alpha(const float* alphas /*[R,S]*/, int64_t r, int32_t s, float* weights,
                                   float* trans, void* stream);
int nrhip_render_weight_from_alpha_bwd(const float* alphas, const float* grad_w, const float* grad_t, int64_t r,
                                       int32_t s, float* grad_alphas, void* stream);
int nrhip_render_weight_from_density(const float* t_starts, const float* t_ends, const float* sigmas, int64_t r,
                                     int32_t s, float* weights, float* trans, float* alphas, void* stream);
int nrhip_render_weight_from_density_bwd(const float* t_starts, const float* t_ends, const float* sigmas,
                                         const float* grad_w, int64_t r, int32_t s, float* grad_sigmas,
                                         void* stream);
/* values may be NULL (accumulation only, C=1) */
int nrhip_accumulate_along_rays(const float* weights /*[R,S]*/, const float* values /*[R,S,C]*/, int64_t r,
                                int32_t s, int32_t c, float* out /*[R,C]*/, void* stream);
/* its autograd (values given): grad_weights [R,S] = sum_c g[r,c] v[r,s,c], grad_values [R,S,C] = w[r,s] g[r,c];
 * either output may be NULL */
int nrhip_accumulate_along_rays_bwd(const float* weights, const float* values, const float* g_out /*[R,C]*/, int64_t r,
                                    int32_t s, int32_t c, float* grad_weights, float* grad_values, void* stream);

/* ---- C4 / §8(f) row 2: lidar carving.  is_close [R,S] (uint8) = NeuRADModel._compute_is_close_to_lidar
 * (models/neurad.py:677-700): lidar sample whose midpoint lies within carving_epsilon of the measured return, or -- no
 * return -- anywhere closer than non_return_lidar_distance; with `weights` also the proposal carving term of
 * models/neurad.py:399-408 per ray, loss_per_ray [R] = sum_s (w * (is_lidar & ~close))^2, and its gradient
 * grad_weights [R,S] = 2 w (is_lidar & ~close).  is_lidar / did_return (may be NULL = all returned) are uint8 [R];
 * any of the three outputs may be NULL.                                                                             */
int nrhip_lidar_carving(const float* starts, const float* ends, int32_t sample_stride /*0 = S*/, const float* weights,
                        const uint8_t* is_lidar, const uint8_t* did_return, const float* distance /*[R]*/,
                        float carving_epsilon, float non_return_lidar_distance, int64_t r, int32_t s, uint8_t* is_close,
                        float* loss_per_ray, float* grad_weights, void* stream);

/* ---- C3: appearance embedding (models/neurad.py:423-441): out[r,:] = E[idx_lo[r]] * (1 - frac[r]) + E[idx_hi[r]] * frac[r]
 * (idx_hi == frac == NULL: the plain lookup of use_temporal_appearance = False).  E [n_embed, dim], indices int64.
 * bwd ACCUMULATES the table gradient into grad_weight [n_embed, dim] (caller zeroes): nn.Embedding's backward.     */
int nrhip_embedding_lerp_fwd(const float* weight, const int64_t* idx_lo, const int64_t* idx_hi, const float* frac,
                             int64_t r, int32_t n_embed, int32_t dim, float* out /*[R,dim]*/, void* stream);
int nrhip_embedding_lerp_bwd(const float* g_out /*[R,dim]*/, const int64_t* idx_lo, const int64_t* idx_hi,
                             const float* frac, int64_t r, int32_t n_embed, int32_t dim, float* grad_weight,
                             void* stream);

/* ---- C2: get_nff_outputs compositing (models/neurad.py:377-395,727-734) ------------------------
 * weights [R,S] come from C1; the residual 1-acc goes on the last (sky) sample; depth drops it.     */
int nrhip_composite_fwd(const float* weights, const float* features /*[R,S,C]*/, const float* starts,
                        const float* ends, int64_t r, int32_t s, int32_t c, float* out_features /*[R,C]*/,
                        float* out_depth /*[R]*/, float* out_acc /*[R]*/, void* stream);
int nrhip_composite_bwd(const float* weights, const float* features, const float* starts, const float* ends,
                        const float* g_features, const float* g_depth, const float* g_acc, int64_t r, int32_t s,
                        int32_t c, float* grad_weights /*[R,S]*/, float* grad_features /*[R,S,C]*/, void* stream);

/* ---- F1+C1+C2 fused: the headline kernel -- hash lookup + MLPs + compositing per ray -----------
 * (NeuRADModel.get_nff_outputs minus sampling, models/neurad.py:373-395).  Optional per-sample
 * outputs (may be NULL): weights [R,S] (pre sky residual, as returned by C1).
 * The MLPs' product sums are fp32 sums: formed from fp16 pairs on the matrix cores (x = fp16(x) + fp16(x - fp16(x)), fp32
 * accumulation; inputs that do not fit a pair take the fp32 MFMA tile by tile), 1e-7 from the fp32 MFMA's, which the
 * environment variable NRHIP_MLP_PAIRS=0 selects everywhere.                                        */
int nrhip_render_fwd(const nrhip_field* f, const nrhip_rays* rays, float* out_features /*[R,C]*/,
                     float* out_depth /*[R]*/, float* out_acc /*[R]*/, float* out_weights /*[R,S] or NULL*/,
                     void* stream);
/* The same with options.  early_stop_eps > 0 (eval only; 0 = exact): a ray stops marching once the transmittance
 * entering a 16-sample tile has fallen below it -- the samples behind that tile carry less than early_stop_eps of
 * weight in total and are skipped (wave-uniform test; weights of skipped samples are written as 0). */
int nrhip_render_fwd_ex(const nrhip_field* f, const nrhip_rays* rays, float* out_features, float* out_depth,
                        float* out_acc, float* out_weights, float early_stop_eps, void* stream);

/* ---- ray generation on the device (the step before the path) -------------------------------------
 * Sensor tables are device arrays indexed by camera / lidar; one call turns R (sensor index, pixel | point) pairs into
 * the per-ray part of a RayBundle.  Outputs: origins [R,3], directions [R,3] (unit), pixel_area [R], times [R]. */
typedef struct {
  const float* camera_to_worlds;     /* [C,3,4] row major (Cameras.camera_to_worlds) */
  const float* fx; const float* fy;  /* [C] */
  const float* cx; const float* cy;  /* [C] */
  const float* times;                /* [C] or NULL */
  int32_t rolling_shutter;           /* 0 none; 1 rows (PandaSet, top to bottom); 2 columns; 3 columns reversed
                                        (metadata["rs_direction"], cameras.py:941-953) */
  const float* rolling_shutter_time; /* [C] metadata["rolling_shutter_time"]   (NULL when rolling_shutter == 0) */
  const float* time_to_center_pixel; /* [C] metadata["time_to_center_pixel"] */
  const float* velocities;           /* [C,3] metadata["velocities"] */
  const float* shutter_extent;       /* [C] image height (mode 1) or width (modes 2, 3) as float */
} nrhip_camera_table;
/* == Cameras._generate_rays_from_coords (cameras.py:560-968) for PERSPECTIVE cameras without lens distortion (the
 * caller checks camera_type / distortion_params and keeps the reference's generator for anything else).  coords [R,2]
 * = (y, x) pixel-centre coordinates as in Cameras.get_image_coords.  directions_norm [R] = the pre-normalisation norm
 * (metadata["directions_norm"]).  times may be NULL when the table has no times. */
int nrhip_camera_rays(const nrhip_camera_table* cams, const int64_t* camera_indices /*[R]*/, const float* coords /*[R,2]*/,
                      int64_t n_rays, float* origins, float* directions, float* pixel_area, float* directions_norm,
                      float* times, void* stream);

/* The lens of the cameras of one call (ABI 517).  All cameras share the type; a Cameras object of mixed types is the
 * caller's to refuse (the reference's own loop, cameras.py:792-800, fills the rays of one type only). */
typedef struct {
  int32_t camera_type;      /* CameraType value (cameras.py:43-55): 1 PERSPECTIVE, 2 FISHEYE; others NRHIP_ERR_UNSUPPORTED */
  const float* distortion;  /* [C,6] k1 k2 k3 k4 p1 p2 (Cameras.distortion_params), or NULL: no undistortion */
} nrhip_camera_lens;
/* nrhip_camera_rays for PERSPECTIVE or FISHEYE cameras with OpenCV lens distortion: each of the pixel and its +1 x / +1 y
 * neighbours is undistorted by the reference's Newton solve (camera_utils.py:655-758: ten iterations from the distorted
 * point, step 0 where |denominator| <= 1e-3; an all-zero row comes back bit for bit), then turned into a direction --
 * (u, -v, -1), or for FISHEYE (u sin t / t, -v sin t / t, -cos t) with t = |(u, v)| clipped to [0, pi]
 * (cameras.py:800-815).  Everything after that is nrhip_camera_rays: PERSPECTIVE with distortion NULL gives its bits.
 * Mirrored from the reference: a FISHEYE ray exactly at the principal point (t = 0) is NaN in directions, directions_norm
 * and pixel_area, and the rays one pixel to its left / above it are NaN in pixel_area. */
int nrhip_camera_rays_lens(const nrhip_camera_table* cams, const nrhip_camera_lens* lens,
                           const int64_t* camera_indices /*[R]*/, const float* coords /*[R,2]*/, int64_t n_rays,
                           float* origins, float* directions, float* pixel_area, float* directions_norm, float* times,
                           void* stream);

typedef struct {
  const float* lidar_to_worlds;             /* [Ln,3,4] */
  const float* times;                       /* [Ln] or NULL */
  const float* velocities;                  /* [Ln,3] metadata["velocities"] or NULL */
  const float* horizontal_beam_divergence;  /* [Ln] */
  const float* vertical_beam_divergence;    /* [Ln] */
  int32_t assume_ego_compensated;           /* Lidars.assume_ego_compensated */
  float valid_lidar_distance_threshold;     /* did_return = distance < threshold (lidars.py:447) */
} nrhip_lidar_table;
/* == Lidars._generate_rays_from_points (lidars.py:399-460).  points [R,point_dim]: xyz in the lidar frame, intensity,
 * time offset within the sweep (point_dim >= 5 for the motion / time terms).  distance [R] = range of the point
 * (metadata["directions_norm"]), did_return [R] uint8. */
int nrhip_lidar_rays(const nrhip_lidar_table* lidars, const int64_t* lidar_indices /*[R]*/, const float* points,
                     int32_t point_dim, int64_t n_rays, float* origins, float* directions, float* pixel_area,
                     float* distance, uint8_t* did_return, float* times, void* stream);

/* == ScaledPatchSampler.collate_image_dataset_batch (data/pixel_samplers.py:618-742) on a device-resident image batch
 * images [n_images, height, width, channels] (image_dtype 0 = fp32, 1 = uint8; may be NULL together with patches):
 * patch centres -> ray_indices [P * patch_size^2, 3] int64 = (image_idx[c] (or c when image_idx is NULL), y, x), the
 * ground-truth patches [P, K, K, channels] with K = patch_size * patch_scale, and (optional, may be NULL) coords
 * [P * patch_size^2, 2] = (y + 0.5, x + 0.5), the image_coords[y, x] row RayGenerator.forward feeds to
 * nrhip_camera_rays (model_components/ray_generators.py:41-55).  Exactly one of
 *   uniforms [P,3] fp32  -- the torch.rand((P,3)) draws of PixelSampler.sample_method (:100-103); centre =
 *                           (u * float(n_images, H-K+1, W-K+1)).long() + (0, K/2, K/2)  (:722-726), and
 *   centers  [P,3] int64 -- (image, y, x) given directly (the sampling-weights branch, :728-742, clips them itself)
 * is non-NULL.  Integer results are bit-identical to the reference's; patches are copies.  Image reads are clamped into
 * the image (a centre closer than K/2 to the border would raise in the reference). */
int nrhip_patch_sample(const float* uniforms, const int64_t* centers, int64_t n_patches, int32_t n_images, int32_t height,
                       int32_t width, int32_t channels, int32_t patch_size, int32_t patch_scale, const int64_t* image_idx,
                       const void* images, int32_t image_dtype, int64_t* ray_indices, float* coords, void* patches,
                       void* stream);

/* == LidarPointSampler.collate_image_dataset_batch (data/pixel_samplers.py:538-583) on packed point clouds
 * lidar [sum(points_per_lidar), point_dim] fp32 (lidar_packed_collate, image_lidar_datamanager.py:60-74).  The caller
 * hands over torch's own draws -- shuffle [n_lidars] int64 = torch.randperm (:540) and draws [n_lidars, rays_per_lidar]
 * fp64 = torch.rand(..., dtype=float64) (:552), rays_per_lidar = ceil(n_rays / n_lidars) (:542).  Output row r < n_rays
 * belongs to scan l = shuffle[r / rays_per_lidar] and is its point p = floor(draws[l, r % rays_per_lidar] *
 * points_per_lidar[l]): indices [n_rays,2] = (lidar_idx[l] (or l when NULL), p), points [n_rays, point_dim] = the
 * gathered rows -- exactly what LidarRayGenerator / nrhip_lidar_rays consume.  n_lidars <= 2048. */
int nrhip_lidar_point_sample(const int64_t* shuffle, const double* draws, const int64_t* points_per_lidar,
                             const int64_t* lidar_idx, const float* lidar, int32_t n_lidars, int32_t rays_per_lidar,
                             int32_t point_dim, int64_t n_rays, int64_t* indices, float* points, void* stream);

/* ---- optimizer step of a hash table == torch.optim.Adam / AdamW on one fp32 tensor
 * (engine/optimizers.py:168-181; hashgrids group: lr 1e-2, eps 1e-15, configs/method_configs.py:423-426).  In place on
 * param / exp_avg / exp_avg_sq [n], 16-byte aligned; step = 1 for the first update; weight_decay is decoupled (AdamW),
 * 0 = plain Adam; grad_scale multiplies the gradient first (1 = off).  Hyper-parameters are doubles: torch derives 1 - beta,
 * lr / (1 - beta1^t) ... from Python floats and rounds once (1.f - 0.999f would be 1.3e-5 off).  Rows with grad = exp_avg = exp_avg_sq = 0 are
 * skipped: their update is exactly zero. */
int nrhip_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step, double lr,
                    double beta1, double beta2, double eps, double weight_decay, double grad_scale, void* stream);

/* The same update for MANY tensors in one launch per 24 tensors (the per-actor grids: 66 launches -> 3 on a 32-actor
 * scene), with two extras per tensor: grad_dtype 1 = the gradient is fp16 (what autograd hands an fp16-storage table),
 * converted in registers; image_fp16 != NULL = `param` is the fp32 MASTER copy of an fp16-storage table and the rounded
 * new value is written to image_fp16 in the same pass (no .float() / copy_ passes over the table).  step is per tensor
 * (a table no ray touched keeps its count: optim.py skips it, as torch.optim.Adam skips parameters without a gradient). */
typedef struct nrhip_adam_tensor {
  float* param;        /* [n] fp32: the tensor the update runs on                    */
  const void* grad;    /* [n] fp32 or fp16 (grad_dtype)                               */
  float* exp_avg;      /* [n] fp32                                                    */
  float* exp_avg_sq;   /* [n] fp32                                                    */
  void* image_fp16;    /* [n] fp16 or NULL                                            */
  int64_t n;
  int64_t step;        /* >= 1, this tensor's step count AFTER the increment          */
  int32_t grad_dtype;  /* 0 fp32, 1 fp16                                              */
  int32_t reserved;
} nrhip_adam_tensor;
int nrhip_adam_step_many(const nrhip_adam_tensor* tensors /* HOST array */, int32_t n_tensors, double lr, double beta1,
                         double beta2, double eps, double weight_decay, double grad_scale, void* stream);

/* The device-controlled form of the same update: torch.amp.GradScaler's optimizer protocol (engine/trainer.py:550-576 steps
 * every optimizer through GradScaler.step; optimizers with `_step_supports_amp_scaling` get the scale and the found-inf flag
 * as DEVICE scalars, torch/amp/grad_scaler.py) and the form a captured step (HIP graph) replays.
 *   step       DEVICE fp32 scalar per tensor (torch's capturable=True state layout), advanced by the launch itself;
 *   found_inf  DEVICE fp32 scalar or NULL: != 0 -> NOTHING is touched (parameters, moments, images, step counts);
 *   grad_scale DEVICE fp32 scalar or NULL: GradScaler's scale S, gradients are divided by it inside the update (no unscale
 *              pass over the table gradients); host_grad_scale multiplies on top (1 = off);
 *   lr_dev     DEVICE fp32 scalar or NULL: overrides lr (a scheduler fills it between graph replays);
 *   workspace  DEVICE, nrhip_adam_step_many_workspace(n_tensors) bytes: the per-tensor arguments a one-thread-per-tensor
 *              kernel derives (in double, rounded once -- the host form's arithmetic) for the streaming kernel.
 * No host read anywhere; every argument of a replay is behind a pointer. */
typedef struct nrhip_adam_tensor_dev {
  float* param;
  const void* grad;
  float* exp_avg;
  float* exp_avg_sq;
  void* image_fp16;
  int64_t n;
  float* step;         /* DEVICE fp32 scalar: the count BEFORE this update                */
  int32_t grad_dtype;  /* 0 fp32, 1 fp16                                                  */
  int32_t reserved;
} nrhip_adam_tensor_dev;
int nrhip_adam_step_many_workspace(int32_t n_tensors, int64_t* bytes);
int nrhip_adam_step_many_dev(const nrhip_adam_tensor_dev* tensors /* HOST array */, int32_t n_tensors, double lr,
                             const float* lr_dev, double beta1, double beta2, double eps, double weight_decay,
                             double host_grad_scale, const float* grad_scale, const float* found_inf, void* workspace,
                             void* stream);

/* GradScaler's inf check over gradients, READ-ONLY (ABI 511).  torch.amp.GradScaler.step runs `_check_inf_per_device` on an
 * optimizer that consumes the scale itself (engine/optimizers.py:168-181 steps every group through it): torch's
 * `_amp_foreach_non_finite_check_and_unscale_` with a scale of 1, which reads and re-writes every element.  This entry point
 * only reads: *found_inf (DEVICE fp32 scalar) is set to 1 when any element of any tensor is +-inf or NaN and is left alone
 * otherwise (the caller zeroes it; several calls may accumulate into one flag).  dtype 0 = fp32, 1 = fp16. */
typedef struct nrhip_check_tensor {
  const void* data;  /* [n], 16-byte aligned */
  int64_t n;
  int32_t dtype;
  int32_t reserved;
} nrhip_check_tensor;
int nrhip_nonfinite_check_many(const nrhip_check_tensor* tensors /* HOST array */, int32_t n_tensors, float* found_inf,
                               void* stream);

/* Processing order for cache locality (fills nrhip_rays.order): a permutation that groups rays looking at the same
 * region -- counting sort by the Morton code of the contracted position (ScaledSceneContraction, static_scale as in
 * nrhip_field) of the point origin + direction * t_ref, t_ref = a representative sample distance (the sampler's
 * median).  The reference has no counterpart: its rays arrive in data-loader order (camera patches + random lidar
 * points, data/datamanagers/image_lidar_datamanager.py:150-169).  order [R] int32 device buffer. */
int nrhip_ray_order(const float* origins /*[R,3]*/, const float* directions /*[R,3]*/, int64_t n_rays, float t_ref,
                    float static_scale, int32_t key_bits /* per axis: 0 = default (4), 3..5 */, int32_t* order,
                    void* stream);

/* The same permutation property (a counting sort by the same key; the order inside a bucket is unspecified in both) over
 * many workgroups, for eval chunks of tens of thousands of rays where the single-workgroup pass (~2 us per 1024 rays) would
 * cost more than the ordered kernels return.  workspace: (n_rays + 8^key_bits) uint32, see _workspace. */
int nrhip_ray_order_workspace(int64_t n_rays, int32_t key_bits, int64_t* bytes /*host*/);
int nrhip_ray_order_large(const float* origins, const float* directions, int64_t n_rays, float t_ref, float static_scale,
                          int32_t key_bits, void* workspace, int64_t workspace_bytes, int32_t* order, void* stream);

/* ---- S2: NeuRADProposalField.get_density (neurad_field.py:208-213) ----------------------------- */
/* level_features (may be NULL): LEVEL-MAJOR [L, R*S] rescaled per-level features, saved for the decoder gradient;
 * when requested (training) the lookups run level-partitioned over the XCDs (csrc/hashgrid.hip) */
int nrhip_proposal_density_fwd(const nrhip_proposal* p, const nrhip_rays* rays, float* density /*[R,S]*/,
                               float* level_features, void* stream);
/* grad_table / grad_decoder are accumulated into */
int nrhip_proposal_density_bwd(const nrhip_proposal* p, const nrhip_rays* rays, const float* density,
                               const float* grad_density, float* grad_table, float* grad_decoder, void* stream);
/* level_features: what the forward saved, or NULL (the interpolated features are then recomputed) */
int nrhip_proposal_density_bwd_binned(const nrhip_proposal* p, const nrhip_rays* rays, const float* density,
                                      const float* level_features, const float* grad_density, float* grad_table,
                                      float* grad_decoder, int32_t overwrite /*grad_table only*/, void* workspace,
                                      int64_t workspace_bytes, void* stream);

/* ---- S3: RaySamples.get_weights (cameras/rays.py:188-210) -------------------------------------- */
int nrhip_weights_from_density(const float* deltas, const float* densities, int64_t r, int32_t s, float* weights,
                               void* stream);
int nrhip_weights_from_density_bwd(const float* deltas, const float* densities, const float* grad_w, int64_t r,
                                   int32_t s, float* grad_densities, void* stream);

/* ---- S1: PowerSampler / SpacedSampler (ray_samplers.py:80-132,838-852; utils/math.py:541-579) ---
 * t_rand [R,S+1] = injected stratified jitter (training) or NULL (eval).  Outputs are bin EDGES.
 * last_edge > 0: the last euclidean edge is set to it -- the model's sky stretch (models/neurad.py:451-455) when
 * the PowerSampler bins go straight to the field; <= 0: off.                                          */
int nrhip_power_sampler(const float* nears /*[R]*/, const float* fars /*[R]*/, int64_t r, int32_t s, float lam,
                        float scaling, const float* t_rand, float last_edge, float* spacing_bins /*[R,S+1]*/,
                        float* euclid_bins /*[R,S+1]*/, void* stream);
/* nrhip_power_sampler + nrhip_ray_order in ONE launch (same arguments, same results as the two calls): workgroup 0 runs the
 * single-workgroup ordering pass while the others fill bins, so that the processing order of an eval chunk costs no launch
 * of its own in front of the render kernel. */
int nrhip_power_sampler_ordered(const float* nears, const float* fars, int64_t r, int32_t s, float lam, float scaling,
                                const float* t_rand, float last_edge, float* spacing_bins, float* euclid_bins,
                                const float* origins /*[R,3]*/, const float* directions /*[R,3]*/, float t_ref,
                                float static_scale, int32_t key_bits, int32_t* order /*[R]*/, void* stream);

/* ---- S4: PDFSampler (ray_samplers.py:280-376), include_original=False -------------------------
 * rand: NULL (eval) or [R] (single_jitter) / [R,S_new+1] (rand_stride = 1 / S_new+1)               */
int nrhip_pdf_sample(const float* weights /*[R,S_prev]*/, const float* spacing_bins /*[R,S_prev+1]*/,
                     const float* nears, const float* fars, int64_t r, int32_t s_prev, int32_t s_new, float lam,
                     float scaling, float histogram_padding, const float* rand, int32_t rand_stride,
                     float* new_spacing_bins /*[R,S_new+1]*/, float* new_euclid_bins /*[R,S_new+1]*/,
                     void* stream);

/* ---- H5: dynamic actors (NeuRADHashEncoding._split_static_vs_actors / _get_actor_indices /
 *      _get_actor_features_slow, field_components/neurad_encoding.py:189-295; DynamicActors.get_boxes2world,
 *      model_components/dynamic_actors.py:251-268; interpolate_trajectories_6d, utils/poses.py:90-150).
 *      Torch-path semantics: one 3-D hash grid per actor; when boxes overlap the highest actor index wins
 *      (the CPU index_put order of neurad_encoding.py:184-185); eval mode (no random flip).              */
typedef struct {
  int32_t n_actors;              /* A */
  int32_t n_times;               /* Tn */
  const float* timestamps;       /* [Tn]      unique_timestamps */
  const float* positions;        /* [Tn,A,3]  actor_positions */
  const float* rotations_6d;     /* [Tn,A,6]  actor_rotations_6d */
  const uint8_t* present;        /* [Tn,A]    actor_present_at_time */
  const float* bounds;           /* [A,3]     actor_sizes/2 + actor_padding (dynamic_actors.py:106-107) */
  nrhip_grid grid;               /* geometry shared by all actor grids (ActorSettings) */
  const void* const* tables;     /* DEVICE array of A table pointers, indexed by actor_to_id[actor] */
  float actor_scale;             /* actor contraction scale, 10 m (neurad_encoding.py:52,100) */
  int32_t max_candidates;        /* K: row length of the per-ray candidate lists below; 0 = NRHIP_DEFAULT_ACTOR_CANDIDATES.
                                    With K = n_actors no ray can overflow (the reference has no limit,
                                    neurad_encoding.py:225-263) and the lists cost R*K*52 bytes of HBM.          */
} nrhip_actors;

#define NRHIP_DEFAULT_ACTOR_CANDIDATES 8
#define NRHIP_MAX_SAMPLE_CONTAINMENTS 8 /* boxes that can contain ONE sample and still all receive gradients */
/* Per ray: interpolate every actor's pose at the ray's time, cull by distance to the ray's first->last sample line,
 * and compact the survivors: cand_count [R] int32, cand_actor [R,K] int32, cand_w2b [R,K,12] (3x4 world->box),
 * K = actors->max_candidates.  overflow (device int32, caller zeroes; may be NULL) is set if a ray has more than K. */
int nrhip_actor_prepare(const nrhip_actors* a, const nrhip_rays* rays, const float* times /*[R]*/,
                        int32_t* cand_count, int32_t* cand_actor, float* cand_w2b, int32_t* overflow, void* stream);
/* The same with the EVAL-time actor edit of DynamicActors.edit_boxes2world (model_components/dynamic_actors.py:181-249,
 * applied by get_boxes2world when the module is not training, :261-265; set by the viewer sliders :58-104 and by the
 * actor-shift FID evaluation, pipelines/ad_pipeline.py:476-480): after the pose interpolation the boxes of `index` (-1:
 * all; clamped to the last actor) are moved by (lateral, longitudinal, height) in their own frame and yawed by `rotation`
 * (radians, pre-multiplied: the translation stays).  Everything downstream -- line cull, in-box test, box-frame positions
 * and directions -- sees the edited pose.  As in the reference nothing happens unless lateral, longitudinal or rotation is
 * non-zero (a height-only edit is ignored, :182-187).  edit = NULL: nrhip_actor_prepare.                                    */
typedef struct {
  float lateral, longitudinal, height, rotation;
  int32_t index;
} nrhip_actor_edit;
int nrhip_actor_prepare_edited(const nrhip_actors* a, const nrhip_rays* rays, const float* times /*[R]*/,
                               const nrhip_actor_edit* edit, int32_t* cand_count, int32_t* cand_actor, float* cand_w2b,
                               int32_t* overflow, void* stream);
/* Field features: for every sample inside an actor box, OVERWRITE its feature row [out_dim] with the actor grid's
 * rescaled features zero-padded to out_dim, and write the per-sample direction (box frame, renormalised) -- ray
 * direction elsewhere.  hit [N] int32 = index of the actor whose grid was used, -1 elsewhere.                                         */
int nrhip_actor_encode(const nrhip_actors* a, const nrhip_rays* rays, const int32_t* cand_count,
                       const int32_t* cand_actor, const float* cand_w2b, int32_t out_dim, float* features /*[N,out_dim]*/,
                       float* directions /*[N,3]*/, int32_t* hit /*[N] actor index or -1*/,
                       const float* ray_flip /*[R] +-1 (training x-flip, neurad_encoding.py:212-219) or NULL*/,
                       void* stream);
/* All containments: hits [N, NRHIP_MAX_SAMPLE_CONTAINMENTS] = the actors whose boxes contain the sample, compacted in
 * ascending actor order and padded with -1 (the last non-negative entry is the one nrhip_actor_encode used; if more
 * boxes than that overlap at one point, the lowest indices drop out).  The reference's index_put backward
 * gives EVERY duplicate (ray, sample) row the upstream gradient, so training needs the whole list.            */
int nrhip_actor_hits(const nrhip_actors* a, const nrhip_rays* rays, const int32_t* cand_count,
                     const int32_t* cand_actor, const float* cand_w2b, int32_t* hits /*[N,8]*/, void* stream);
/* Proposal density: density = exp(decoder . padded actor features) for samples inside an actor box
 * (fields/neurad_field.py:208-213 with the actor branch of neurad_encoding.py:170-185).                      */
int nrhip_actor_density(const nrhip_actors* a, const nrhip_rays* rays, const int32_t* cand_count,
                        const int32_t* cand_actor, const float* cand_w2b, const float* decoder_weight, int32_t n_dec,
                        float* density /*[R,S] overwritten where hit*/, int32_t* hit /*actor index or -1*/, const float* ray_flip,
                        void* stream);

/* Training path of the in-box samples: box-frame, contracted position of P (sample, actor) pairs -- the chain
 * interpolate_trajectories_6d (utils/poses.py:90-150) -> rotation_6d_to_matrix (cameras/camera_utils.py:422-443) ->
 * pose inverse (utils/poses.py:42-55) -> transform_points_pairwise (cameras/lidars.py:550-564) -> training x-flip
 * (neurad_encoding.py:212-219) -> ScaledSceneContraction(inf) (spatial_distortions.py:103-141) -- and its backward into
 * the trajectory parameters (what autograd does for `require_actor_grad`, neurad_encoding.py:174-176).
 * sample_idx [P] int64 = flat sample index ray*S + s; actor_idx [P] int32; x01 [P,3] in [0,1]^3, cstd [P].
 * bwd ACCUMULATES into grad_positions [Tn,A,3] and grad_rotations_6d [Tn,A,6] (caller zeroes).                    */
int nrhip_actor_pair_positions_fwd(const nrhip_actors* a, const nrhip_rays* rays, const float* times,
                                   const int64_t* sample_idx, const int32_t* actor_idx, const float* ray_flip /*[R] or NULL*/,
                                   int64_t n_pairs, float* x01, float* cstd, void* stream);
int nrhip_actor_pair_positions_bwd(const nrhip_actors* a, const nrhip_rays* rays, const float* times,
                                   const int64_t* sample_idx, const int32_t* actor_idx, const float* ray_flip,
                                   int64_t n_pairs, const float* grad_x01, const float* grad_cstd,
                                   float* grad_positions, float* grad_rotations_6d, void* stream);
/* The same backward, additionally ACCUMULATING dL/d(origins) [R,3] and dL/d(directions) [R,3] of the pairs' rays (caller
 * zeroes or pre-fills): the in-box samples' share of the pose gradient of a camera optimizer that moves the rays
 * (cameras/camera_optimizers.py:173-182; `require_actor_grad`, neurad_encoding.py:174-176 keeps positions.mean in the graph). */
int nrhip_actor_pair_positions_bwd_rays(const nrhip_actors* a, const nrhip_rays* rays, const float* times,
                                        const int64_t* sample_idx, const int32_t* actor_idx, const float* ray_flip,
                                        int64_t n_pairs, const float* grad_x01, const float* grad_cstd,
                                        float* grad_positions, float* grad_rotations_6d, float* grad_origins,
                                        float* grad_directions, void* stream);

/* The (sample, actor) pairs of a hits table [N, NRHIP_MAX_SAMPLE_CONTAINMENTS] in (sample, slot) order -- what
 * `(hits >= 0).nonzero()` + a gather produce in the reference's style of indexing (neurad_encoding.py:221-263 returns such index
 * lists from torch.nonzero), as two streaming passes.  count: block_offsets [ceil(N / 1024)] u32 (scratch, exclusive prefix
 * on return) and *total (DEVICE int64) = number of pairs; the caller reads total, allocates sample_idx int64 [P] / actor_idx
 * int32 [P], and calls write with the same block_offsets and total (device pointers). */
int nrhip_actor_pairs_count(const int32_t* hits, int64_t n_samples, uint32_t* block_offsets, int64_t* total, void* stream);
int nrhip_actor_pairs_write(const int32_t* hits, int64_t n_samples, const uint32_t* block_offsets, const int64_t* total,
                            int64_t* sample_idx, int32_t* actor_idx, void* stream);

/* Proposal density of the in-box samples in TRAINING (fields/neurad_field.py:208-213 over neurad_encoding.py:150-187,
 * index_put order :184-185): rows [P, row_dim] = rescaled actor features of the P (sample, actor) pairs, decoder_weight
 * [row_dim], sample_idx [P] int64 flat sample index, winner [P] u8 (the pair whose actor the forward uses: the highest index
 * containing the sample; exactly one per hit sample).
 * fwd: density [N] IN/OUT -- the winners' trunc_exp(rows . w) overwrite the static density of their samples; logit [P] out.
 * bwd: grad_density [N] IN/OUT = the caller's copy of grad_out, zeroed here at the hit samples; grad_rows [P, row_dim] out
 *      (winners: through trunc_exp's backward exp(clamp(logit, +-15)), field_components/activations.py:37-41; shadowed pairs:
 *      grad_out * merged density * w, the duplicate-index gradient of the reference's index_put); grad_decoder [row_dim]
 *      ACCUMULATES (caller zeroes) and comes from the winners only.                                                        */
int nrhip_actor_density_splice_fwd(const float* rows, int32_t row_dim, const float* decoder_weight, const int64_t* sample_idx,
                                   const uint8_t* winner, int64_t n_pairs, float* density, float* logit, void* stream);
int nrhip_actor_density_splice_bwd(const float* rows, int32_t row_dim, const float* decoder_weight, const int64_t* sample_idx,
                                   const uint8_t* winner, const float* logit, const float* density_out, const float* grad_out,
                                   int64_t n_pairs, float* grad_density, float* grad_rows, float* grad_decoder, void* stream);

/* F1+C1+C2 with dynamic actors in ONE kernel (eval): nrhip_render_fwd_ex where a sample inside an actor's box reads
 * that actor's grid at its box-frame position and uses the box-frame view direction -- NeuRADHashEncoding.forward
 * (field_components/neurad_encoding.py:150-187, 203-208) + NeuRADField.forward (fields/neurad_field.py:128-152) +
 * compositing (models/neurad.py:373-395).  cand_*: the per-ray candidate lists of nrhip_actor_prepare (row length
 * a->max_candidates).  NRHIP_ERR_UNSUPPORTED unless both grids share one storage type (fp32 or fp16), the actor grid has the static grid's
 * features per level and at most its number of levels (the reference's defaults: static 8x4, actors 4x4).
 * Three launches, no host round trip: a device-side split of the processing order into rays without / with candidate
 * actors, the plain static kernel over the first slice, the actor-aware instantiation over the second.
 * workspace: device scratch of (n_rays + 4) int32.                                                                  */
int nrhip_render_fwd_actors(const nrhip_field* f, const nrhip_actors* a, const nrhip_rays* rays,
                            const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                            float* out_features, float* out_depth, float* out_acc, float* out_weights /*or NULL*/,
                            float early_stop_eps, int32_t* workspace, void* stream);

/* ---- S6: occupancy-grid ray march (VolumetricSampler.forward -> nerfacc OccGridEstimator.sampling,
 *      model_components/ray_samplers.py:483-566).  nerfacc is un-vendored and nothing in neurad-studio instantiates
 *      VolumetricSampler: the marching rule is this library's own statement (csrc/occgrid.hip header), parity
 *      unpinned.  Two passes: offsets == NULL -> per-ray counts; then, with the exclusive prefix sum of the counts as
 *      offsets, the packed (ray_indices, t_starts, t_ends) are written.
 *      max_candidates (>= 1): the number of candidate intervals a ray may have, counted BEFORE the occupancy test --
 *      candidates k = 0 .. max_candidates - 1 of the tiling are looked at, kept or not, and the march of the ray ends
 *      there; a ray emits at most that many samples.  The same in all three march entry points.                */
typedef struct {
  float aabb[6];            /* min xyz, max xyz */
  int32_t resolution;       /* res^3 cells, one level; cell index = (ix*res + iy)*res + iz */
  const uint8_t* binaries;  /* [res,res,res] occupancy */
} nrhip_occgrid;
int nrhip_occgrid_march(const nrhip_occgrid* grid, const float* origins, const float* directions,
                        const float* t_min /*[R] or NULL*/, const float* t_max /*[R] or NULL*/,
                        const float* t_rand /*[R] stratified offset in [0,1) or NULL*/, int64_t r,
                        float render_step_size, float near_plane, float far_plane, float cone_angle,
                        int32_t max_candidates, int32_t* counts /*[R], counting pass*/,
                        const int64_t* offsets /*[R], write pass*/, int64_t* ray_indices, float* t_starts,
                        float* t_ends, void* stream);
/* Multi-level grid: level l is the level-0 box scaled by 2^l about its centre (the caller passes every box, nested and in
 * that order).  The march clips the ray to the outermost box; a candidate's level is the first whose box contains its
 * midpoint, and it is kept iff that level's cell (same floor-and-clamp rule) is set.  Same two passes and outputs as
 * nrhip_occgrid_march; with levels == 1 the outputs are those of nrhip_occgrid_march bit for bit.                      */
#define NRHIP_OCCGRID_MAX_LEVELS 8
typedef struct {
  int32_t levels, resolution;                 /* res^3 cells per level, cell index = (ix*res + iy)*res + iz */
  float aabbs[NRHIP_OCCGRID_MAX_LEVELS][6];   /* per level: min xyz, max xyz */
  uint8_t* binaries;                          /* [levels,res,res,res] occupancy (written by the update entry points) */
} nrhip_occgrid_levels;
int nrhip_occgrid_march_levels(const nrhip_occgrid_levels* grid, const float* origins, const float* directions,
                               const float* t_min /*[R] or NULL*/, const float* t_max /*[R] or NULL*/,
                               const float* t_rand /*[R] or NULL*/, int64_t r, float render_step_size, float near_plane,
                               float far_plane, float cone_angle, int32_t max_candidates, int32_t* counts,
                               const int64_t* offsets, int64_t* ray_indices, float* t_starts, float* t_ends,
                               void* stream);
/* The box-aware march (ABI 518), for scenes with dynamic actors.  The grid is a time-independent world-space grid built
 * from static densities: the cells inside an actor's box at a ray's time are empty to it, and the plain march drops exactly
 * the intervals the actors live in.  Here the candidate intervals are those of nrhip_occgrid_march_levels (same clipping,
 * stepping, cone_angle and t_rand), and one is kept iff its level's cell is set (that entry point's test, unchanged) OR its
 * sample position -- the mean the field evaluates, t_start + (t_end - t_start) / 2 along the ray -- lies strictly inside
 * the box of one of the ray's candidate actors: cand_count [R], cand_actor [R,K], cand_w2b [R,K,12] as nrhip_actor_prepare
 * writes them at the ray's time (K = actors->max_candidates; one list per RAY -- prepare them from any two distinct points
 * of the ray's line, nothing here is sized by the sample count).  Position and in-box test are the device functions the
 * field kernels call, so march and field agree on every sample bit for bit.  Of `actors` only n_actors, bounds and
 * max_candidates are read.  Same two passes and outputs; with every cand_count zero the outputs are those of
 * nrhip_occgrid_march_levels bit for bit.                                                                             */
int nrhip_occgrid_march_levels_actors(const nrhip_occgrid_levels* grid, const nrhip_actors* actors,
                                      const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                                      const float* origins, const float* directions, const float* t_min /*[R] or NULL*/,
                                      const float* t_max /*[R] or NULL*/, const float* t_rand /*[R] or NULL*/, int64_t r,
                                      float render_step_size, float near_plane, float far_plane, float cone_angle,
                                      int32_t max_candidates, int32_t* counts, const int64_t* offsets,
                                      int64_t* ray_indices, float* t_starts, float* t_ends, void* stream);
/* ---- occupancy-grid maintenance (modelled on nerfacc 0.5 OccGridEstimator._update / mark_invisible_cells; the rule is
 *      stated in csrc/occgrid_update.h and restated in tests/occgrid_update_restatement.py -- parity with nerfacc itself is
 *      unpinned, like the march).  occs fp32 [levels*res^3]; occs < 0 marks an invisible cell.  No entry point allocates,
 *      synchronises with the host or sizes anything by data; results are bitwise reproducible.
 *      workspace: device scratch of nrhip_occgrid_update_workspace bytes, ZERO-FILLED once by the caller and then owned by
 *      the grid (the entry points keep the parts they rely on zeroed).                                               */
int nrhip_occgrid_update_workspace(int32_t levels, int32_t resolution, int64_t* bytes);
/* Candidate cells and their jittered positions.  warmup != 0: every visible cell of every level, capacity res^3 per level.
 * warmup == 0: per level the visible ones of the n draws cell_draws int64 [levels,n], then its occupied cells in ascending
 * order (more than n: n draws with replacement through sel_draws fp32 [levels,n] in [0,1)), capacity 2 n per level.
 * jitter fp32 [levels,capacity,3] in [0,1).  Outputs: cell_ids int32 [levels,capacity] (-1 behind the level's count),
 * counts int32 [levels], positions fp32 [levels*capacity,3].  capacity == 0 is a no-op that reads no pointer.          */
int nrhip_occgrid_update_candidates(const nrhip_occgrid_levels* grid, const float* occs, int32_t warmup, int32_t n,
                                    const int64_t* cell_draws, const float* sel_draws, const float* jitter,
                                    int32_t* cell_ids, int32_t* counts, float* positions, void* workspace,
                                    int64_t workspace_bytes, void* stream);
/* occ_values fp32 [levels*capacity]: what was evaluated at the positions.  occs[c] = max(occs[c] * ema_decay, max of the
 * cell's candidates) on touched cells; then binaries = occs > min(mean of the visible occs, occ_thre).                */
int nrhip_occgrid_update_apply(const nrhip_occgrid_levels* grid, float* occs, int64_t capacity, const int32_t* cell_ids,
                               const int32_t* counts, const float* occ_values, float ema_decay, float occ_thre,
                               void* workspace, int64_t workspace_bytes, void* stream);
/* K fp32 [n_k,3,3] with n_k == n_cams or 1, c2w fp32 [n_cams,3,4] (OpenCV convention).  Visible cells: occs = 0;
 * invisible ones: occs = -1 and their binary cleared.                                                               */
int nrhip_occgrid_mark_invisible(const nrhip_occgrid_levels* grid, const float* K, int32_t n_k, const float* c2w,
                                 int32_t n_cams, int32_t width, int32_t height, float near_plane, float* occs,
                                 void* stream);
/* nerfacc render_visibility_from_alpha, packed: segments [R+1] delimit each ray's samples */
int nrhip_packed_visibility_from_alpha(const float* alphas, const int64_t* segments, int64_t r, float early_stop_eps,
                                       float alpha_thre, uint8_t* mask, void* stream);

/* ---- C1 packed: compositing of the march's packed samples (nerfacc's packed render_weight_from_alpha /
 *      render_weight_from_density / accumulate_along_rays, renderers.py:83-90,126-135,343-347,402-409) and their fusion.
 *      segments int64 [R+1]: ray r owns the samples [segments[r], segments[r+1]) of the [M]-shaped arrays -- the fourth
 *      output of the march's Python wrapper, or nrhip_packed_segments of ray_indices.  One wavefront walks one ray in
 *      chunks of 64 with a carried prefix, the arithmetic of the dense kernels; no atomics (bitwise reproducible), no
 *      allocation, no host synchronisation (graph-capturable).  r == 0 is a no-op that reads no pointer; a batch without
 *      samples (every segment empty) reads no sample pointer and still zeroes the per-ray outputs.  Parity with nerfacc
 *      itself is unpinned (un-vendored); what is pinned is listed in DESIGN.md.                                      */
/* segments[q] = number of i with ray_indices[i] < q, q in [0, R].  PRECONDITION: ray_indices [M] is non-decreasing with
 * values in [0, R) -- what the march and nerfacc both guarantee; it is not checked.                                  */
int nrhip_packed_segments(const int64_t* ray_indices, int64_t m, int64_t r, int64_t* segments, void* stream);
/* alpha_i = 1 - exp(-sigma_i (t_end_i - t_start_i)), T_i = exp(-sum_{j<i, same ray} sigma_j delta_j), w_i = T_i alpha_i;
 * trans / alphas may be NULL.  Backward: gradient w.r.t. sigmas from grad_w.                                          */
int nrhip_packed_weight_from_density(const float* t_starts, const float* t_ends, const float* sigmas,
                                     const int64_t* segments, int64_t r, float* weights, float* trans /*or NULL*/,
                                     float* alphas /*or NULL*/, void* stream);
int nrhip_packed_weight_from_density_bwd(const float* t_starts, const float* t_ends, const float* sigmas,
                                         const int64_t* segments, const float* grad_w, int64_t r, float* grad_sigmas,
                                         void* stream);
/* T_i = prod_{j<i, same ray} (1 - alpha_j), w_i = T_i alpha_i; trans may be NULL */
int nrhip_packed_weight_from_alpha(const float* alphas, const int64_t* segments, int64_t r, float* weights,
                                   float* trans /*or NULL*/, void* stream);
int nrhip_packed_weight_from_alpha_bwd(const float* alphas, const int64_t* segments, const float* grad_w,
                                       const float* grad_t /*may be NULL*/, int64_t r, float* grad_alphas, void* stream);
/* out[r,c] = sum over ray r's samples of weights[i] values[i,c]  (values NULL: c must be 1, a plain sum of the weights).
 * Every row of out is written, zeros for an empty segment: the caller does not pre-zero it.  C % 4 == 0 with 16-byte
 * aligned rows reads values in 16-byte pieces (C = 32: 8 lanes a sample, C = 48: 4 lanes x 3), any other C >= 1 takes
 * a generic path.                                                                                                     */
int nrhip_packed_accumulate(const float* weights, const float* values /*[M,C] or NULL*/, const int64_t* segments,
                            int64_t r, int32_t c, float* out /*[R,C]*/, void* stream);
int nrhip_packed_accumulate_bwd(const float* weights, const float* values, const float* g_out /*[R,C]*/,
                                const int64_t* segments, int64_t r, int32_t c, float* grad_weights /*[M], may be NULL*/,
                                float* grad_values /*[M,C], may be NULL*/, void* stream);
/* fused: weights (mode 1: from sigmas, mode 0: from alphas), sum w f, sum w (t_start + t_end) / 2 (render_depth_simple:
 * no normalisation) and sum w in one pass over a ray's segment; no sky-residual sample.  The backward recomputes the
 * transmittance and runs the sums over the later samples as a suffix scan; g_weights is the upstream gradient of
 * out_weights.                                                                                                        */
int nrhip_packed_composite_fwd(const float* t_starts, const float* t_ends, const float* sigmas_or_alphas,
                               const float* features /*[M,C]*/, const int64_t* segments, int64_t r, int32_t c,
                               int32_t mode, float* out_features /*[R,C]*/, float* out_depth /*[R,1]*/,
                               float* out_accumulation /*[R,1]*/, float* out_weights /*[M], may be NULL*/, void* stream);
int nrhip_packed_composite_bwd(const float* t_starts, const float* t_ends, const float* sigmas_or_alphas,
                               const float* features, const int64_t* segments, const float* g_features /*[R,C]*/,
                               const float* g_depth /*[R], may be NULL*/, const float* g_accumulation /*[R], may be NULL*/,
                               const float* g_weights /*[M], may be NULL*/, int64_t r, int32_t c, int32_t mode,
                               float* grad_sigmas_or_alphas /*[M], may be NULL*/, float* grad_features /*[M,C], may be NULL*/,
                               void* stream);

/* ---- F1+C1 packed, fused: nrhip_render_fwd_ex for the march's packed samples -- the field evaluated on every sample and
 *      composited as nrhip_packed_composite_fwd does (no sky-residual sample, depth = sum w (t_start + t_end) / 2 over all
 *      samples, an empty segment writes zeros to its three output rows: the caller does not pre-zero), in ONE kernel:
 *      one wavefront per ray in tiles of 16 samples, origins / directions / pixel area read PER RAY (no per-sample copy
 *      exists on this path), no per-sample feature ever written.  Static scene, inference; instantiated for every
 *      `Composite, Static` row of csrc/render_variants.h with fp32 or fp16-pair products (NRHIP_MLP_PAIRS as for
 *      nrhip_render_fwd_ex), fp32 and fp16 tables.  early_stop_eps as nrhip_render_fwd_ex (tile-granular; weights of the
 *      skipped samples are written as 0; 0 = exact).  n_rays == 0 is a no-op that reads no pointer; n_samples == 0 reads
 *      no sample pointer and no segment and still zeroes the per-ray outputs; n_samples >= 2^31 is NRHIP_ERR_UNSUPPORTED.
 *      No allocation, no host synchronisation (graph-capturable).  PRECONDITION (not checked): segments is
 *      non-decreasing from 0 to n_samples.                                                                              */
typedef struct {
  int64_t n_rays;            /* R */
  int64_t n_samples;         /* M = segments[R]; < 2^31 */
  const float* origins;      /* [R,3] */
  const float* directions;   /* [R,3] */
  const float* pixel_area;   /* [R]   */
  const float* t_starts;     /* [M]   */
  const float* t_ends;       /* [M]   */
  const int64_t* segments;   /* [R+1], as nrhip_packed_segments / the march produce */
  const int32_t* order;      /* optional [R]: processing order (see nrhip_rays.order) */
} nrhip_packed_rays;
int nrhip_render_fwd_packed(const nrhip_field* f, const nrhip_packed_rays* rays, float* out_features /*[R,32]*/,
                            float* out_depth /*[R]*/, float* out_acc /*[R]*/, float* out_weights /*[M] or NULL*/,
                            float early_stop_eps, void* stream);

/* nrhip_render_fwd_packed for a scene with dynamic actors (ABI 518): the packed counterpart of nrhip_render_fwd_actors.
 * cand_*: one candidate list per RAY (nrhip_actor_prepare on two distinct points of the ray's line; row length
 * a->max_candidates).  Three launches, no host round trip: the device-side split of the processing order into rays without
 * / with candidates, nrhip_render_fwd_packed's kernel over the first slice, the actor-aware packed kernel (every
 * `Composite, Actors, F32` row of csrc/render_variants.h, fp32 and fp16 tables) over the second.  Compositing, early_stop_eps,
 * order, n_rays == 0 and n_samples == 0 as nrhip_render_fwd_packed; overlapping boxes: the highest actor index wins; the
 * grid restrictions of nrhip_render_fwd_actors apply.  With every cand_count zero the outputs are those of
 * nrhip_render_fwd_packed bit for bit.  workspace: device scratch of (n_rays + 4) int32.                                */
int nrhip_render_fwd_packed_actors(const nrhip_field* f, const nrhip_actors* a, const nrhip_packed_rays* rays,
                                   const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                                   float* out_features /*[R,32]*/, float* out_depth /*[R]*/, float* out_acc /*[R]*/,
                                   float* out_weights /*[M] or NULL*/, float early_stop_eps, int32_t* workspace,
                                   void* stream);

/* ---- training on packed samples: the packed counterparts of nrhip_field_fwd_train, nrhip_sdf_render_fwd / _bwd and
 *      nrhip_encode_bwd_binned.  No atomics, no allocation, no host synchronisation (graph-capturable).                  */
/* nrhip_field_fwd_train on the march's packed samples: the same per-sample kernel (every `PerSample, Static, F32` row of
 * csrc/render_variants.h, fp32 and fp16 tables), ray constants read per ray, every per-sample row stored at the PACKED
 * sample index.  geo_out [M] = the geometry MLP's first output (sdf / raw density), head [M] = sigmoid(-geo_out beta) with
 * the descriptor's beta, or exp(geo_out).  rays->order is honoured.  n_rays == 0 and n_samples == 0 are no-ops that read
 * no pointer; n_samples >= 2^31 is NRHIP_ERR_UNSUPPORTED; the save buffers must be 16-byte aligned.                      */
int nrhip_field_fwd_train_packed(const nrhip_field* f, const nrhip_packed_rays* rays, float* feature /*[M,32]*/,
                                 float* geo_out /*[M]*/, float* head /*[M]*/, float* save_enc /*[M,L*F]*/,
                                 float* save_geo_hidden /*[M,H]*/, float* save_feat_in /*[M,48]*/,
                                 float* save_feat_hidden /*[M,2H]*/, void* stream);
/* The same with ROW OVERRIDES (ABI 519): nrhip_field_fwd_train_ovr on packed samples -- the training forward of a scene with
 * dynamic actors on the march's output.  ovr_row [M] int32 is indexed by the PACKED sample index (-1: the static scene);
 * ovr_rows [P, L*F] (16-byte aligned) and ovr_dirs [P, 3] as for the dense kernel: a sample with ovr_row >= 0 takes its
 * encoding row and the view direction of its SH inputs from the caller, save_enc holds the overriding row, and no static
 * gather is done for it.  The five `PerSample, Overrides, F32` rows of csrc/render_variants.h, fp32 and fp16 static tables.
 * order, n_rays == 0, n_samples == 0, n_samples >= 2^31 and the alignment of the save buffers as above.                  */
int nrhip_field_fwd_train_packed_ovr(const nrhip_field* f, const nrhip_packed_rays* rays, const int32_t* ovr_row /*[M]*/,
                                     const float* ovr_rows, const float* ovr_dirs, float* feature /*[M,32]*/,
                                     float* geo_out /*[M]*/, float* head /*[M]*/, float* save_enc /*[M,L*F]*/,
                                     float* save_geo_hidden /*[M,H]*/, float* save_feat_in /*[M,48]*/,
                                     float* save_feat_hidden /*[M,2H]*/, void* stream);
/* Actor geometry of packed samples (ABI 519), from one candidate list per RAY (nrhip_actor_prepare on the ray's line, or the
 * box-aware march's own lists): ray_of [M] int64 (the march's ray_indices, clamped into [0, n_rays)) names each sample's ray;
 * rays->segments and rays->order are not read.  hits [M, NRHIP_MAX_SAMPLE_CONTAINMENTS] as nrhip_actor_hits writes them,
 * hit [M] the winning actor (highest index) or -1 and directions [M,3] (may be NULL) the winner's box-frame, renormalised
 * direction with the training x-flip (ray_flip [R] +-1 or NULL) -- the ray direction outside every box -- as
 * nrhip_actor_encode.  No feature rows are written.  Position and containment are the dense kernels' own device functions:
 * uniform segments give their bits.  A sample of a ray without candidates reads its ray index, the candidate count and the
 * ray direction only.  n_rays == 0 and n_samples == 0 are no-ops that read no pointer.                                   */
int nrhip_actor_find_packed(const nrhip_actors* a, const nrhip_packed_rays* rays, const int64_t* ray_of,
                            const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                            int32_t* hits /*[M,8]*/, int32_t* hit /*[M]*/, float* directions /*[M,3] or NULL*/,
                            const float* ray_flip, void* stream);
/* nrhip_actor_pair_positions_fwd / _bwd on packed samples (ABI 519): sample_idx [P] int64 is a PACKED sample index (clamped
 * into [0, M)), its ray comes from ray_of [M]; times and ray_flip stay per ray ([R]).  The same kernel bodies as the dense
 * pair; the backward ACCUMULATES (atomics) into grad_positions / grad_rotations_6d.  The rays' gradient is the entry point
 * nrhip_actor_pair_positions_bwd_rays_packed below.                                                                        */
int nrhip_actor_pair_positions_fwd_packed(const nrhip_actors* a, const nrhip_packed_rays* rays, const int64_t* ray_of,
                                          const float* times, const int64_t* sample_idx, const int32_t* actor_idx,
                                          const float* ray_flip /*[R] or NULL*/, int64_t n_pairs, float* x01, float* cstd,
                                          void* stream);
int nrhip_actor_pair_positions_bwd_packed(const nrhip_actors* a, const nrhip_packed_rays* rays, const int64_t* ray_of,
                                          const float* times, const int64_t* sample_idx, const int32_t* actor_idx,
                                          const float* ray_flip, int64_t n_pairs, const float* grad_x01,
                                          const float* grad_cstd, float* grad_positions, float* grad_rotations_6d,
                                          void* stream);
/* dL/d(origins), dL/d(directions) [R,3] of the in-box samples of PACKED rays: the ray share of
 * nrhip_actor_pair_positions_bwd_rays, on the pairs of nrhip_actor_pair_positions_fwd_packed (additive to ABI 520).  A pair
 * hands its ray -gt for the origin and -gt * t_mid for the direction, gt = dL/d(interpolated translation), exactly what the
 * dense kernel adds; the trajectory gradients stay with _bwd_packed.  This entry WRITES the two outputs (no caller zeroing),
 * without atomics and without a workspace, an allocation or a host synchronisation (graph-capturable): bit-reproducible.
 * PRECONDITION: sample_idx [P] is a packed sample index and NON-DECREASING -- what nrhip_actor_pairs_write produces ((sample,
 * slot) order; several actors may share a sample).  With samples in ray order the pairs of ray r are then one range of the
 * list; values are clamped into [0, M) when read (a clamped non-decreasing list is non-decreasing), segment bounds into
 * [0, M], and a list that breaks the precondition gives wrong sums but no read outside the arrays.  rays->segments is
 * required; there is no ray_of, the group knows its ray.
 * A group of lanes_per_ray lanes (16 / 32 / 64) owns a ray: two searches of the pair list for the range of its segment,
 * lane `sub` adds the pairs sub, sub + G, ... of the range in that order, xor butterfly, lane 0 writes.  A ray's rows depend
 * on its own pairs and on G only; a ray without samples or without pairs gets exact zeros.  lanes_per_ray = 0: chosen on the
 * host from the shapes alone, by the dense rule on the mean pair count n_pairs / n_rays (> 32 -> 64, > 16 -> 32, else 16;
 * a ray far above the mean only makes its own group loop longer).
 * n_rays == 0 is a no-op that reads no pointer; n_pairs == 0 zeroes both outputs without a launch; n_pairs > 0 on a batch
 * without samples is NRHIP_ERR_INVALID_ARG, n_samples >= 2^31 NRHIP_ERR_UNSUPPORTED.                                      */
int nrhip_actor_pair_positions_bwd_rays_packed(const nrhip_actors* a, const nrhip_packed_rays* rays, const float* times,
                                               const int64_t* sample_idx, const int32_t* actor_idx,
                                               const float* ray_flip /*[R] or NULL*/, int64_t n_pairs,
                                               const float* grad_x01, const float* grad_cstd,
                                               int32_t lanes_per_ray /*0 = choose*/, float* grad_origins /*[R,3]*/,
                                               float* grad_directions /*[R,3]*/, void* stream);
/* head + packed compositing.  beta: DEVICE pointer to the raw parameter, alpha = sigmoid(-geo_out (|beta| + beta_min));
 * beta == NULL: the density head, alpha = 1 - exp(-trunc_exp(geo_out) (t_end - t_start)).  Compositing as
 * nrhip_packed_composite_fwd (no sky residual, depth over all samples, zeros for an empty segment).  alpha [M] is what the
 * backward starts from.  Backward: each of g_features / g_depth / g_accumulation / g_weights may be NULL (g_features
 * NULL: grad_features is not written -- it is zero); grad_beta [1] = sign(beta) x the fixed-order sum of one partial per
 * wavefront (workspace: nrhip_sdf_render_packed_bwd_workspace(r) floats), bitwise reproducible; the density head leaves
 * grad_beta alone.  r == 0 is a no-op that reads no pointer (the backward zeroes grad_beta).                           */
int nrhip_sdf_render_packed_fwd(const float* geo_out /*[M]*/, const float* beta /*device [1] or NULL*/, float beta_min,
                                const float* features /*[M,C]*/, const float* t_starts, const float* t_ends,
                                const int64_t* segments, int64_t r, int32_t c, float* alpha /*[M]*/, float* weights /*[M]*/,
                                float* out_features /*[R,C]*/, float* out_depth /*[R]*/, float* out_accumulation /*[R]*/,
                                void* stream);
int nrhip_sdf_render_packed_bwd_workspace(int64_t r, int64_t* floats);
int nrhip_sdf_render_packed_bwd(const float* geo_out, const float* beta, float beta_min, const float* alpha,
                                const float* features, const float* t_starts, const float* t_ends, const int64_t* segments,
                                const float* g_features /*[R,C]*/, const float* g_depth /*[R]*/,
                                const float* g_accumulation /*[R]*/, const float* g_weights /*[M]*/, int64_t r, int32_t c,
                                float* grad_features /*[M,C]*/, float* grad_geo_out /*[M]*/, float* grad_beta /*[1]*/,
                                float* workspace, void* stream);
/* nrhip_encode_bwd_binned / _f16 for packed samples: ray_of [M] (the march's ray_indices, values in [0, n_rays)) names
 * each sample's ray; grad_out [M, L*F].  Workspace: nrhip_encode_bwd_binned_workspace(g, n_samples); `overwrite` and the
 * fp16 one-round rule as for the dense pair.  rays->segments and rays->order are not read.                             */
int nrhip_encode_bwd_binned_packed(const nrhip_grid* g, float static_scale, const nrhip_packed_rays* rays,
                                   const int64_t* ray_of, const float* grad_out, float* grad_table, int32_t overwrite,
                                   void* workspace, int64_t workspace_bytes, void* stream);
int nrhip_encode_bwd_binned_packed_f16(const nrhip_grid* g, float static_scale, const nrhip_packed_rays* rays,
                                       const int64_t* ray_of, const float* grad_out, void* grad_table_fp16, void* workspace,
                                       int64_t workspace_bytes, void* stream);
/* nrhip_encode_bwd_rays for packed samples: dL/d(origins), dL/d(directions) [R,3] of the static encoding path from
 * grad_out [M, L*F] = dL/d(rescaled features) at the packed sample index -- what a camera optimizer receives when the model
 * samples through the occupancy grid.  Each sample's arithmetic is nrhip_encode_bwd_rays' (one shared body); a group of
 * lanes_per_ray lanes (16 / 32 / 64; 0: chosen from the mean count M / R by the dense rule, > 32 -> 64, > 16 -> 32, else 16)
 * owns ray r, strides over the samples [segments[r], segments[r+1]), merges by xor-butterfly and WRITES both rows: no
 * atomics, no workspace, bit-reproducible; a ray's rows depend on its own samples and the group size only.  A ray without
 * samples gets zeros; rows of grad_out that are exactly zero skip their gathers.  fp32 and fp16-storage tables, every
 * n_features.  n_rays == 0 is a no-op that reads no pointer; n_samples == 0 zeroes both outputs without a launch;
 * n_samples >= 2^31 is NRHIP_ERR_UNSUPPORTED.  Sample indices are clamped into [0, M).  rays->order is not read.
 * No allocation, no host synchronisation (graph-capturable).                                                            */
int nrhip_encode_bwd_rays_packed(const nrhip_grid* g, const void* table, float static_scale, const nrhip_packed_rays* rays,
                                 const float* grad_out /*[M, L*F]*/, int32_t lanes_per_ray /*0 = choose*/,
                                 float* grad_origins /*[R,3]*/, float* grad_directions /*[R,3]*/, void* stream);

/* ---- S5+M1 fused: ProposalNetworkSampler as driven by NeuRADModel._get_ray_samples
 *      (ray_samplers.py:623-666, models/neurad.py:443-459).  One wave marches one ray through
 *      power bins -> (density -> weights -> pdf resample) x n_rounds, entirely on chip.
 *      props[i] is the field evaluated in round i (the caller reproduces the late-binding quirk of
 *      models/neurad.py:248 by passing the same field twice).
 *      Outputs: final bins [R,S_final+1] (spacing + euclid, NOT sky-stretched -- M1's stretch is applied
 *      by the host mirror) and per-round weights / bins for the proposal losses.                     */
typedef struct {
  int32_t n_rounds;                 /* <= 2 */
  int32_t n_samples[3];             /* e.g. {128, 64, 32} */
  float lam, scaling;               /* PowerSampler(lambda_, scaling) */
  float histogram_padding;          /* 0.01 */
  float sky_distance;               /* fars are clamped to this (neurad.py:445-446) */
} nrhip_sampler_cfg;
int nrhip_proposal_sampler_fwd(const nrhip_sampler_cfg* cfg, const nrhip_proposal* props /*host array[n_rounds]*/,
                               const float* origins, const float* directions, const float* pixel_area,
                               const float* nears, const float* fars, int64_t r,
                               float* const* round_weights /*host array[n_rounds] of [R,S_i]*/,
                               float* const* round_spacing /*host array[n_rounds+1] of [R,S_i+1]*/,
                               float* const* round_euclid  /*host array[n_rounds+1] of [R,S_i+1]*/,
                               void* stream);
/* The same for a scene with dynamic actors: a proposal sample inside an actor's box takes its density from that actor's
 * grid of the proposal field (fields/neurad_field.py:208-213 over neurad_encoding.py:150-187).  actors[i] = the actor
 * grids of props[i] (host array[n_rounds]; all rounds share the actor set: bounds, max_candidates); cand_* = the per-ray
 * candidate lists of nrhip_actor_prepare -- they depend on the ray's line only, so one call on any two samples of the
 * ray serves every round and the field.  NRHIP_ERR_UNSUPPORTED unless the actor grids have 1 feature per level, fp32
 * tables and at most the static grid's levels (the reference's proposal defaults).                                  */
int nrhip_proposal_sampler_fwd_actors(const nrhip_sampler_cfg* cfg, const nrhip_proposal* props,
                                      const nrhip_actors* actors /*host array[n_rounds]*/, const int32_t* cand_count,
                                      const int32_t* cand_actor, const float* cand_w2b, const float* origins,
                                      const float* directions, const float* pixel_area, const float* nears,
                                      const float* fars, int64_t r, float* const* round_weights,
                                      float* const* round_spacing, float* const* round_euclid, void* stream);

/* ---- losses on the sampler outputs (model_components/losses.py) ---------------
 * One wavefront per ray; spacing-space bin edges c [R,S+1] in [0,1], weights [R,S].
 * zipnerf_interlevel_loss (losses.py:645-705), ONE proposal level per call: c/w = the fine (field) histogram
 * (detached in the reference), cp/wp = the proposal level, pulse_width = 0.03 / 0.003 for level 0 / 1.
 * loss_per_ray [R] = sum_s relu(w_s - wp)^2 / (wp + 1e-5); grad_wp [R,n_prop] (may be NULL) = d loss_per_ray / d wp.
 * The reference's value is the mean over rays, summed over levels. */
int nrhip_interlevel_loss(const float* c, const float* w, int32_t n_fine, const float* cp, const float* wp,
                          int32_t n_prop, float pulse_width, int64_t r, float* loss_per_ray, float* grad_wp,
                          void* stream);
/* distortion_loss / lossfun_distortion (losses.py:137-156): loss_per_ray [R], grad_w [R,S] (may be NULL) */
int nrhip_distortion_loss(const float* c, const float* w, int32_t n_samples, int64_t r, float* loss_per_ray,
                          float* grad_w, void* stream);

/* ---- the two per-sample loss terms on PACKED (occupancy-marched) samples (csrc/losses.hip): the distortion loss and the
 *      lidar carving term for [M]-shaped arrays with segments int64 [R+1] as nrhip_packed_segments / the march make them,
 *      ray r owning the samples [segments[r], segments[r+1]) -- no padding of [M] to [R, max_n], any number of samples per
 *      ray.  Both follow the packed compositing kernels' contract: one wavefront walks one ray's segment in chunks of 64
 *      with a carried prefix; no atomics, no LDS, no allocation, no host synchronisation (graph-capturable); every element
 *      has one writer, so the same inputs give the same bits; an empty segment writes 0 to its ray's row of the per-ray
 *      outputs (the caller does not pre-zero); no row past M or R is written.  r == 0 is a no-op that reads no pointer;
 *      m == 0 reads no sample pointer (they may be NULL) and still writes the per-ray outputs as zeros; m >= 2^31 is
 *      NRHIP_ERR_UNSUPPORTED; a negative count or a NULL required pointer is NRHIP_ERR_INVALID_ARG.  Segments are clamped
 *      into [0, m], so broken ones read inside the arrays.
 *
 * nrhip_packed_distortion_loss -- THE CONTRACT.  For a ray with samples i = 0..n-1 in segment order, fp32 interval ends
 * s_i, e_i (in whatever metric the caller chose: the march's Euclidean t, or t mapped through a monotone spacing function)
 * and fp32 weights w_i, everything computed in float64 from the fp32 inputs:
 *   m_i = (s_i + e_i) / 2, delta_i = e_i - s_i                       (both exact in float64)
 *   A_i = sum_{j<i} w_j, B_i = sum_{j<i} w_j m_j;  W, Bt = the same sums over the whole ray
 *   loss   = fp32( 2 sum_i w_i (m_i A_i - B_i) + (1/3) sum_i w_i^2 delta_i )
 *   grad_k = fp32( 2 [ m_k (A_k - (W - A_k - w_k)) - (B_k - (Bt - B_k - w_k m_k)) ] + (2/3) w_k delta_k )
 * PRECONDITION, unchecked like the sortedness of ray_indices: the midpoints are non-decreasing within a ray (the march
 * guarantees it, a monotone spacing map keeps it).  Then this is the reference's
 *   sum_i sum_j w_i w_j |m_i - m_j| + sum_i w_i^2 delta_i / 3
 * -- lossfun_distortion (losses.py:137-148) for contiguous edges, nerfstudio_distortion_loss (losses.py:159-200) for
 * separate starts and ends -- in O(n) instead of O(n^2), and its derivative w.r.t. the weights.  Equal midpoints,
 * zero-width intervals and zero weights are no special case.  No gradient goes to the interval ends (the dense node
 * detaches them too).  grad_w needs the ray's totals before any per-sample value: a ray of more than 64 samples is walked
 * twice (the second walk repeats the first one's scans bit for bit), a shorter one once.
 * Float64 on purpose: the prefix form cancels (m_i A_i - B_i) where the O(n^2) form adds non-negative terms; in fp32 that
 * would cost digits exactly on the peaked weight distributions this loss produces.
 * ERROR BOUNDS against the exact value of the formulas above on the fp32 inputs (u = 2^-53, S = sum_i |w_i|,
 * X = max_i |m_i|, interval ends >= 0 so that delta_i <= 2 m_i):
 *   |loss - exact|     <= 2^-24 |exact|   + c (n + 2) u X S^2
 *   |grad_k - exact_k| <= 2^-24 |exact_k| + c (n + 2) u X S         with c = NRHIP_PACKED_DISTORTION_C = 16.
 * The first term is the one rounding to fp32.  The second is a first-order count of the roundings (units: u X S^2 for
 * the loss, u X S for the gradient):
 *   - a sum of up to n float64 terms taken in ANY association (wave scan + carry) is within (n - 1) u sum|terms|, so A_i
 *     and W carry (n - 1) [x X once multiplied by m], B_i and Bt (with the rounding of each product w_j m_j) n;
 *   - loss: per sample |w_i| times { (n - 1) + n from A_i, B_i; 1 for the product m_i A_i; 2 for the difference (at most
 *     2 X S); 2 for the product with w_i (same size) } = 2n + 4; summed over i: (2n + 4) S; the sum of the n terms, each at
 *     most 2 |w_i| X S: 2 (n - 1) S; times the exact factor 2: (8n + 4) X S^2.  The width term, three roundings per sample
 *     and the sum, on at most (2/3) X S^2: (2/3)(n + 2); the last addition, on at most (14/3) X S^2: 5.  Together
 *     8.67n + 10.4 < 9 (n + 2);
 *   - grad_k: A_k enters twice and W once, 3 (n - 1), plus three subtractions with results of at most S: 3; times m_k,
 *     one more rounding: 3n + 1.  B_k twice and Bt once, 3n, the product w_k m_k, 1, and three subtractions: 3n + 4.  The
 *     difference of the two brackets, at most 2 X S: 2; times the exact 2: 2 (6n + 7) = 12n + 14.  The width term, three
 *     roundings on at most (4/3) X S: 4; the last addition, on at most (16/3) X S: 6.  Together 12n + 24 <= 15 (n + 2);
 *   - the slack of both, and one more unit, cover the roundings of a float64 reference that evaluates the O(n^2) form with
 *     exactly rounded sums (at most 3 u on each product): c = 16.                                                      */
#define NRHIP_PACKED_DISTORTION_C 16
int nrhip_packed_distortion_loss(const float* s_starts, const float* s_ends, const float* weights,
                                 const int64_t* segments, int64_t r, int64_t m, float* loss_per_ray /*[R]*/,
                                 float* grad_w /*[M] or NULL*/, void* stream);
/* nrhip_lidar_carving on packed samples.  is_lidar uint8 [R], did_return uint8 [R] or NULL = all returned, distance [R].
 * The mask is computed exactly as the dense kernel computes it and matches the reference bit for bit:
 *   mid = (t_start + t_end) * 0.5f in fp32;  close = lidar && (returned ? fabsf(dist - mid) < eps : mid < non_return),
 * both comparisons strict.  With wf_i = (lidar && !close_i) ? w_i : 0:
 *   is_close [M] = close_i,  loss_per_ray [R] = fp32(sum_i (double)wf_i^2),  grad_weights [M] = 2 wf_i  (exact in fp32).
 * |loss - exact| <= 2^-24 |exact| + n 2^-53 sum_i wf_i^2: the squares are exact in float64, their sum is taken in
 * float64 in some association, then rounded to fp32 once.  A camera ray (is_lidar == 0) reads no sample and gets mask 0,
 * loss 0 and gradient 0.  Any of the three outputs may be NULL (at least one is needed); weights may be NULL when only
 * the mask is asked for.                                                                                              */
int nrhip_packed_lidar_carving(const float* t_starts, const float* t_ends, const float* weights /*[M] or NULL*/,
                               const int64_t* segments, const uint8_t* is_lidar, const uint8_t* did_return,
                               const float* distance, float carving_epsilon, float non_return_lidar_distance, int64_t r,
                               int64_t m, uint8_t* is_close /*[M] or NULL*/, float* loss_per_ray /*[R] or NULL*/,
                               float* grad_weights /*[M] or NULL*/, void* stream);

/* ---- lidar scan evaluation (csrc/lidar_eval.hip): the chamfer distance of NeuRADModel.get_image_metrics_and_images
 *      (models/neurad.py:614-618; utils/math.py:745-798, there 2 ceil(N / 1000) torch.cdist blocks) ------------------------
 * A point set is fp32 [n, stride]: the first three floats of a row are xyz, the row stride (floats) is >= 3, so
 * points[:, :3] of an [N,5] scan and homogeneous [N,4] points go in without a copy; valid is uint8 [n] or NULL (all valid).
 *
 * nrhip_nearest_sq_dist: out[i] = min over the valid targets j of |q_i - t_j|^2, as three rounded fp32 subtractions, then
 * fma(dz, dz, fma(dy, dy, dx * dx)), the minimum by fminf -- never |a|^2 + |b|^2 - 2ab.  Against the exact value of the
 * fp32 inputs |out_i - ref_i| <= 6 * 2^-24 * ref_i.  A valid query without a valid target gets +inf; an invalid query gets
 * 0 (written); a valid target with a NaN coordinate is ignored by every query; a valid query with a NaN coordinate gets
 * +inf; neither touches any other row.  n == 0 or m == 0 reads nothing of the empty set.
 * Brute force: one lane holds Q queries in registers, the targets stream through LDS in tiles of NRHIP_NEAREST_TILE; when
 * the queries alone cannot fill the chip the target range is split over `split` workgroups whose partial minima meet in an
 * unsigned atomic min on the float's bits.  plan: 0 = chosen from n and m alone (nrhip_nearest_plan, host logic), else
 * Q | split << 8 with Q in {1, 2, 4}, split in [1, 64].  Every plan, and every order of the targets, gives the same bits.
 * Counts >= 2^31 are NRHIP_ERR_UNSUPPORTED.                                                                            */
#define NRHIP_NEAREST_TILE 1024
int nrhip_nearest_sq_dist(const float* query, int32_t stride_q, const uint8_t* query_valid, int64_t n, const float* target,
                          int32_t stride_t, const uint8_t* target_valid, int64_t m, int32_t plan, float* out, void* stream);
int nrhip_nearest_plan(int64_t n, int64_t m, int32_t* q /*host*/, int32_t* split /*host*/);
/* chamfer_distance (utils/math.py:745-798): result [1] (device) = (S2T + T2S) / (normalize_with_target ? #valid targets : 1),
 * S2T = sum over the valid sources of their nearest squared distance to the valid targets, T2S the other way round.  Both
 * sums are accumulated in float64 in a fixed order (per-workgroup partials, then one fixed-order pass) and the result is
 * rounded to fp32 once: bitwise reproducible, no float atomics, no host read.  Empty sets follow IEEE arithmetic: a side
 * without valid points contributes 0 and leaves the other side's points at +inf; 0 / 0 is NaN.  source_sq_dist [n] /
 * target_sq_dist [m] (either may be NULL) receive the per-point values of nrhip_nearest_sq_dist.  workspace: device scratch
 * of nrhip_chamfer_workspace bytes (host logic), 16-byte aligned.                                                       */
int nrhip_chamfer_workspace(int64_t n, int64_t m, int64_t* bytes /*host*/);
int nrhip_chamfer_distance(const float* source, int32_t stride_s, const uint8_t* source_valid, int64_t n,
                           const float* target, int32_t stride_t, const uint8_t* target_valid, int64_t m,
                           int32_t normalize_with_target, int32_t plan, float* result, float* source_sq_dist,
                           float* target_sq_dist, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- median (quantile) depth (csrc/median_depth.hip): DepthRenderer(method="median"), model_components/renderers.py:353-397,
 *      for dense samples and -- what the reference does not have (renderers.py:390-391 raises) -- for packed ones ------------
 * THE CONTRACT.  For a ray with samples 0..n-1, fp32 weights w_i, a threshold q and midpoints mid_i = (start_i + end_i) / 2
 * (fp32: one rounded add, then one multiplication by 0.5):
 *   1. c_i = float32(sum_{j<=i} w_j): the sum taken in float64 in sample order and rounded to fp32 ONCE per i.  This is
 *      what torch.cumsum gives on the CPU (fp32 accumulated in float64); it is not the sequential fp32 sum, and not the
 *      fp32 parallel scan torch runs on a GPU.
 *   2. k = the first i with !(c_i < q); none: k = n - 1 (the reference's searchsorted returns n and is clamped).
 *   3. depth = mid_k, index = k.
 * The kernels take the float64 prefix sums from a wave-level scan: for weights whose float64 partial sums are exact (e.g.
 * multiples of 2^-24 below 2) every order of the additions gives the same c_i, and that is what the tests pin bit for bit;
 * otherwise a c_i may differ from the sequential float64 sum by the last float64 bit before its rounding to fp32.
 * What follows from the three rules, each on purpose:
 *   - an exact tie c_i == q crosses at i (searchsorted's side="left");
 *   - a +inf weight crosses where it stands;
 *   - a NaN weight behind the crossing is never looked at;
 *   - c_k itself NaN (a NaN weight at or before the crossing): depth = NaN, index = k, the sample of the first NaN sum -- a
 *     NaN is kept.  DEVIATION from the reference: its binary search treats NaN as "less than" and lands on a sample that
 *     depends on where the NaN sits (the last one even for a ray that crossed at sample 0); that is not reproduced;
 *   - negative weights make c non-monotone: the linear rule above still defines the result (the reference's is undefined);
 *   - packed only: a ray without samples gets depth 0 and index -1, what accumulate_along_rays gives such a ray.
 * Interfaces.  weights / starts / ends: fp32 [R,S] contiguous, S >= 1 (dense), or [M] with segments int64 [R+1] as
 * nrhip_packed_segments makes them (packed; M < 2^31; segments are clamped into [0, M], so broken ones read inside the
 * arrays).  thresholds: k HOST floats, 1 <= k <= NRHIP_MEDIAN_MAX_THRESHOLDS, read during the call and handed to the
 * kernel by value; each must be finite (else NRHIP_ERR_INVALID_ARG).  One pass over a ray serves all k.  out_depth fp32
 * [R,k]; out_index int32 [R,k] or NULL.  r == 0 is a no-op that reads no device pointer; m == 0 reads no sample pointer.
 * One wavefront per ray in chunks of 64 samples with a float64 carry, left as soon as every threshold has crossed; starts /
 * ends are read at the crossing sample only.  No LDS, no atomics, no allocation, no host read: the same inputs give the
 * same bits.  No gradient: the result is piecewise constant in the weights.                                            */
#define NRHIP_MEDIAN_MAX_THRESHOLDS 8
int nrhip_median_depth(const float* weights, const float* starts, const float* ends, int64_t r, int32_t s,
                       const float* thresholds /*host [k]*/, int32_t k, float* out_depth /*[R,k]*/,
                       int32_t* out_index /*[R,k] or NULL*/, void* stream);
int nrhip_median_depth_packed(const float* weights, const float* t_starts, const float* t_ends, const int64_t* segments,
                              int64_t r, int64_t m, const float* thresholds /*host [k]*/, int32_t k,
                              float* out_depth /*[R,k]*/, int32_t* out_index /*[R,k] or NULL*/, void* stream);

/* ---- surface normals from the geometry head (csrc/normals.hip; additive to ABI 520) -----------------------------------
 * Definition.  For a sample with gaussian mean x = o + d (t0 + t1) / 2 (cameras/rays.py:109-124, M = 1):
 *   geo  = the first output of the geometry MLP at x: the SDF, or the pre-exp logit when use_sdf = 0 (what nrhip_field_fwd
 *          returns as sdf_or_raw);
 *   g    = d geo / d x, through the rescale weights (neurad_encoding.py:297-304), the trilinear offsets
 *          (encodings.py:425-464) and the scene contraction of mean AND std (spatial_distortions.py:126-141): the chain of
 *          nrhip_encode_bwd_rays, whose origin gradient on [N,1] rays g is.  Subgradients are torch's: ReLU'(0) = 0,
 *          clamp_min passes at equality, an inf-norm tie is split evenly over the tied axes, floor / ceil carry none;
 *   n    = g / max(|g|_2, 1e-12) for an SDF (use_sdf = 1): it points towards free space; -g / max(|g|_2, 1e-12) in density
 *          mode (fields/base_field.py:80-101).  A zero gradient gives a zero normal.
 * Outputs, each optional (NULL skips the store; all NULL is NRHIP_ERR_INVALID_ARG): geo [N], gradient [N,3], normals
 * [N,3], N = R * S at row ray * S + sample (dense) or N = M at the packed sample index.  With weights non-NULL ([R, S]
 * with row stride weight_stride floats, 0 = S; packed: [M]) ray_normals [R,3] = sum_s w_s n_s, NOT normalised;
 * ray_normals without weights is NRHIP_ERR_INVALID_ARG (unless the batch has no samples).  A sample with w == 0 adds nothing to its ray, not even a NaN, and
 * when no per-sample output is asked for it is skipped entirely (no gathers; its interval may hold anything).  The order of
 * the additions is fixed by the ray's own samples and the group width G alone (G lanes per ray, lane i adds the samples i,
 * i + G, ... in that order, then an xor butterfly; G = the power of two >= S, at most 64; packed: S = ceil(M / R)), so a
 * ray's row does not depend on its place in the batch; a ray or segment without samples gets zeros.
 * rays: sample_stride is honoured (bin edges: starts = e, ends = e + 1, stride S + 1); order is a locality hint (the ray
 * the group at a position works on), results do not depend on it.  Host-side checks: NULL descriptors; R == 0 is a no-op
 * that reads no device pointer; S == 0 / M == 0 reads no sample pointer and zeroes ray_normals; samples without rays are
 * NRHIP_ERR_INVALID_ARG, M >= 2^31 is NRHIP_ERR_UNSUPPORTED.  Packed segments are clamped into [0, M).
 * Shapes: the (L, F, hidden width) of every `PerSample, Static, F32` row of csrc/render_variants.h with a two-layer
 * geometry MLP L*F -> H -> out with biases (only row 0 of the last layer is read), fp32 and fp16 tables; anything
 * else is NRHIP_ERR_UNSUPPORTED (compose nrhip_encode_fwd, nrhip_mlp_fwd, nrhip_mlp_bwd and nrhip_encode_bwd_rays
 * instead).  The static scene only: nrhip_field_normals_actors (below) rotates an in-box sample's gradient to the world.
 * Numerics.  One thread per sample; products are fp32 VALU fma chains (no MFMA, no fp16 pairs).  Position, cells, offsets
 * and the encoding row are nrhip_field_fwd's bits.  geo sums the same products as nrhip_field_fwd's sdf_or_raw from the
 * same encoding bits in another order (fma chains here, the matrix cores there): the two agree within
 * 2 (L F + H + 2) 2^-24 A_geo,  A_geo = |b1| + sum_j |w1_j| (|b0_j| + sum_k |W0_jk| |enc_k|), not to the bit.
 * Error bound against the float64 chain on the fp32 primal (cells, offsets, masks as the reference's fp32 forward):
 *   |g - g_ref| <= 2^-24 |g_ref| + NRHIP_NORMALS_C(L, F, H) 2^-24 A      per element,
 * A = the same chain with every product and difference in absolute value, run on |W0|^T (|w1| mask) and |table|.  The
 * constant is a first-order count of the roundings on the longest path of this formulation, not fitted to any output:
 *   H          d geo / d enc_k: an fma chain over the H neurons;
 *   F + 15     one level's sum over its features of (d geo / d enc) x (lerp derivative or rescaled value): 9 for the value
 *              (3 complements, 3 x (mul, fma)), 3 for the rescale weight (product, v_rcp_f32), the two products;
 *   L + 5      the level sum of those with scal_l w (and 2 scal_l w for the std term);
 *   24         the contraction's backward (k, dk, d/dm of the std factor with cbrtf, the inf-norm share) and / scale;
 *   196        the forward's std: sample and contraction take their cube roots from v_log_f32 / v_exp_f32 (<= 2^-19 relative
 *              each; one in std, one squared in the contracted std: 3 x 32 units on s), which the clamped rescale weight
 *              ~ 1 / s carries once and its derivative ~ 1 / s^2 twice (192), plus their own roundings (4).
 * geo obeys the same form with A_geo.  A ReLU mask is a discrete choice: a sample with a hidden pre-activation inside its
 * own rounding error may take the other branch, which the bound does not cover (nor a rescale clamp within 2^-19 of 1).
 * The unit normal then differs per component by at most 2 |bound|_2 / |g| + 2^-22 (first order in the normalisation).
 * No gradient flows through any output.  No atomics, no allocation, no host synchronisation: graph-capturable, and the same
 * inputs give the same bits.                                                                                            */
#define NRHIP_NORMALS_C(L, F, H) ((H) + (L) + (F) + 240)
int nrhip_field_normals(const nrhip_field* f, const nrhip_rays* rays, const float* weights /*[R,weight_stride] or NULL*/,
                        int32_t weight_stride, float* geo /*[N] or NULL*/, float* gradient /*[N,3] or NULL*/,
                        float* normals /*[N,3] or NULL*/, float* ray_normals /*[R,3] or NULL*/, void* stream);
int nrhip_field_normals_packed(const nrhip_field* f, const nrhip_packed_rays* rays, const float* weights /*[M] or NULL*/,
                               float* geo /*[M] or NULL*/, float* gradient /*[M,3] or NULL*/,
                               float* normals /*[M,3] or NULL*/, float* ray_normals /*[R,3] or NULL*/, void* stream);

/* ---- surface normals in a scene with dynamic actors (csrc/normals.hip; additive) -----------------------------------------
 * The same quantity where the scene has actors.  cand_count [R], cand_actor [R,K], cand_w2b [R,K,12] are one candidate list
 * per RAY, K = actors->max_candidates: what nrhip_actor_prepare / nrhip_actor_prepare_edited write (for packed samples: on
 * the ray's line).  ray_flip [R] = +-1 (the training x flip) or NULL.
 * Definition.  A sample whose gaussian mean x lies in no box: g = d geo / d x exactly as nrhip_field_normals defines it, and
 * geo / gradient / normals have that kernel's bits.  A sample inside a box takes its encoding row from the actor's grid
 * (neurad_encoding.py:173-187), so geo is the geometry MLP on the row nrhip_actor_encode writes, and the chain is
 *   p = W x + t (the ray's world2box row of that actor, after the eval-time edit if one was prepared), p.x *= f,
 *   ScaledSceneContraction(inf) of (p, std) with the ACTOR scale (std is the sample's own, not transformed),
 *   the actor's La x F grid with its own scalings and rescale weights, zero columns from La * F on, the same MLP;
 *   g_world = W^T diag(f, 1, 1) g_box,   g_box = d geo / d p through offsets, rescale weights and the contraction of mean
 *   and std, with the subgradients above.  The static table is not gathered for such a sample.
 * Winner only.  Where several boxes contain a sample the forward uses the highest actor index (nrhip_actor_encode), and the
 * normal is the derivative of that value: the winner's chain.  (The reference's autograd also hands gradient to the
 * overwritten duplicates, an artefact of index_put's backward and not a derivative of the output; this deviates on purpose.)
 * Outputs: geo, gradient, normals, ray_normals as nrhip_field_normals (order of additions, G, zero-weight skipping, S == 0 /
 * M == 0 / R == 0 included), and two more, optional and per sample: hit [N] int32 = the winning actor or -1, bit for bit
 * nrhip_actor_encode's; box_position [N,3] = the fp32 box-frame position after the flip at which the kernel differentiated,
 * left untouched where hit < 0.  Asking for either makes every sample evaluated, as a per-sample output does.
 * Host-side checks, in this order: field as nrhip_field_normals (NULL: INVALID_ARG; shape: UNSUPPORTED); every output NULL
 * (hit and box_position included): INVALID_ARG; NULL actors descriptor, one of its arrays or a candidate pointer:
 * INVALID_ARG; an actor grid with another F or storage type than the static grid, or more levels: UNSUPPORTED; then the
 * rays: R == 0 is a no-op that reads no device pointer.
 * Shapes: the (L, F, hidden width) of every `Composite, Actors, F32` row of csrc/render_variants.h, fp32 and fp16 tables.
 * Error bound for an in-box sample, against the float64 chain on the fp32 primal -- the kernel's own box_position and hit
 * and the fp32 cand_w2b row:
 *   |g - g_ref| <= 2^-24 |g_ref| + NRHIP_NORMALS_ACTORS_C(La, F, H) 2^-24 A,     A = |W|^T A_box,
 * A_box the absolute-value chain of nrhip_field_normals on the actor grid.  The constant is NRHIP_NORMALS_C's count with the
 * actor grid's La levels, plus 1 for the flip and 5 for a row of the W^T product (3 products, 2 sums).                     */
#define NRHIP_NORMALS_ACTORS_C(La, F, H) (NRHIP_NORMALS_C(La, F, H) + 6)
int nrhip_field_normals_actors(const nrhip_field* f, const nrhip_actors* actors, const nrhip_rays* rays,
                               const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                               const float* ray_flip /*[R] or NULL*/, const float* weights /*[R,weight_stride] or NULL*/,
                               int32_t weight_stride, float* geo, float* gradient, float* normals, float* ray_normals,
                               int32_t* hit /*[N] or NULL*/, float* box_position /*[N,3] or NULL*/, void* stream);
int nrhip_field_normals_packed_actors(const nrhip_field* f, const nrhip_actors* actors, const nrhip_packed_rays* rays,
                                      const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                                      const float* ray_flip /*[R] or NULL*/, const float* weights /*[M] or NULL*/,
                                      float* geo, float* gradient, float* normals, float* ray_normals,
                                      int32_t* hit /*[M] or NULL*/, float* box_position /*[M,3] or NULL*/, void* stream);

/* ---- camera image evaluation (csrc/image_eval.hip): PSNR and SSIM of NeuRADModel.get_image_metrics_and_images
 *      (models/neurad.py:265-266,585-586: torchmetrics' PeakSignalNoiseRatio(data_range=1.0) and
 *      structural_similarity_index_measure(preds, target) with its defaults) -----------------------------------------------
 * a, b: fp32 [h, w, c] channel-last, contiguous, h, w >= 11, c in {1, 3}.  out [2] (device) = psnr, ssim.
 * psnr = 10 log10(psnr_range^2 / mean((a - b)^2)): the fp32 difference, squared and summed in float64 in a fixed order, the
 * logarithm in float64, rounded to fp32 once; +inf for identical images.
 * ssim = the mean over every 11 x 11 window that lies inside the image ((h - 10)(w - 10) per channel) of
 *   s = (2 mu_a mu_b + c1)(2 s_ab + c2) / ((mu_a^2 + mu_b^2 + c1)(s_a^2 + s_b^2 + c2)),
 * the moments under the separable Gaussian window (11 taps, sigma 1.5, normalised), c1 = (0.01 R)^2, c2 = (0.03 R)^2 with
 * R = max(max a - min a, max b - min b) over both whole images (taken on the device: no host read).  torchmetrics' reflect
 * pad followed by its crop leaves exactly these windows.  The moments are accumulated on values shifted by a per-tile pivot
 * (tiles of NRHIP_SSIM_TILE windows per edge), so s_a^2 = sum g a'^2 - (sum g a')^2 cancels at the size of the local
 * contrast; s is summed in float64 in a fixed order and the mean is rounded once.  ssim_map: [h - 10, w - 10, c] receives s
 * per window, or NULL.  A NaN anywhere makes both results NaN.  Two constant images (R = 0) give ssim = NaN (0 / 0, as in
 * the reference).  Same inputs, same bits; no atomics, no host read, no allocation.  workspace: device scratch of
 * nrhip_image_metrics_workspace bytes (host logic), 16-byte aligned.                                                        */
#define NRHIP_SSIM_TILE 32
#define NRHIP_IMAGE_STAT_ITEMS 4096 /* elements per workgroup (and per float64 partial) of the squared-error pass */
int nrhip_image_metrics_workspace(int32_t h, int32_t w, int32_t c, int64_t* bytes /*host*/);
int nrhip_image_metrics(const float* a, const float* b, int32_t h, int32_t w, int32_t c, float psnr_range, float* ssim_map,
                        void* workspace, int64_t workspace_bytes, float* out, void* stream);
/* PSNR alone over n >= 1 flat elements (the training step's metric): out [1] (device).  workspace: device scratch of
 * 8 * ceil(n / NRHIP_IMAGE_STAT_ITEMS) bytes, 8-byte aligned.                                                           */
int nrhip_image_psnr(const float* a, const float* b, int64_t n, float psnr_range, void* workspace, float* out, void* stream);

/* ---- camera pose correction (csrc/pose_opt.hip): CameraOptimizer.apply_to_raybundle with mode "SO3xR3"
 *      (cameras/camera_optimizers.py:139-182, cameras/lie_groups.py:24-58) and its gradient ------------------------------
 * pose: fp32 [n_cameras, 6] (translation first, then the so(3) tangent vector: the order of the reference's code);
 * weights: fp32 [6] or NULL (= ones); camera_indices: int64 [r]; origins, directions and the outputs: fp32 [r, 3].
 * Forward, per ray of camera c, in fp32 in the reference's operation order (no contraction):
 *   a = fl32(pose[c] * weights), w = a[3:6], nrms = x^2 + y^2 + z^2, theta = sqrt(max(nrms, 1e-4f)), inv = 1 / theta,
 *   f1 = inv sin(theta), f2 = inv inv (1 - cos(theta)), R = f1 K + f2 K^2 + I with K v = w x v,
 *   out_origins = origins + a[0:3], out_directions = R directions.
 * Clamp rule: below nrms = 1e-4f the factors are those of theta = sqrt(1e-4f), constants; at and above it the gradient
 * passes through them (torch.clamp).  Backward and forward decide on the same fp32 nrms.
 * Backward: the twelve terms of a ray are grad_origins[0..2] and grad_directions[i] directions[j]; R enters linearly, so
 * their per-camera sums determine grad_pose exactly.  Each term is formed in double (exact), scaled by 2^(B - e_c), rounded
 * to the nearest int64 and added with a 64-bit integer atomic: 2^(e_c) is the smallest power of two above the camera's largest
 * finite |term| (a per-camera integer max first), B = 62 - ceil(log2 max(r, 2)), so |q| <= 2^B and r of them cannot overflow.
 * One lane per camera then evaluates the chain through the exponential map in double from the fp32 parameters, multiplies by
 * weights and rounds to fp32 once into the dense grad_pose [n_cameras, 6].  Bound, per camera c (n_c rays, largest |term|
 * m_c) and component k against exact arithmetic: |g - g_exact| <= 2^-22 |g_exact| + 16 n_c 2^-B m_c |weights_k|.
 * Properties: no float atomics, no host read, no allocation, capturable in a graph; the same inputs give the same bits, ANY
 * permutation of the rays gives the same bits, and gradients scaled by a power of two give the result scaled by it exactly
 * (short of fp32 under- / overflow of the result).  Cameras without a ray get exact zeros.
 * NaN rule: a ray with a non-finite gradient or direction (or a |term| above FLT_MAX) takes no part in the sums and sets its
 * camera's flag; that camera's row of grad_pose is NaN in all six components, every other row is unaffected.
 * Precondition: 0 <= camera_indices < n_cameras.  A ray that violates it is neither read from pose nor written to the
 * workspace: it comes out of the forward unchanged, contributes nothing to grad_pose, and its input gradients are the output
 * gradients.  workspace: device scratch of nrhip_pose_apply_bwd_workspace bytes (host logic; n_cameras rows of 16 64-bit
 * words: 12 sums, the max cell, the flag, 2 spare), 8-byte aligned; the first pass clears it.  grad_in_origins (= grad_origins)
 * and grad_in_directions (= R^T grad_directions): fp32 [r, 3] or NULL; with both NULL that kernel is skipped.
 * r = 0 or n_cameras = 0: success, nothing is launched and nothing written.                                             */
int nrhip_pose_apply(const float* pose, const float* weights, int32_t n_cameras, const int64_t* camera_indices,
                     const float* origins, const float* directions, int64_t r, float* out_origins, float* out_directions,
                     void* stream);
int nrhip_pose_apply_bwd_workspace(int64_t r, int32_t n_cameras, int64_t* bytes /*host*/);
int nrhip_pose_apply_bwd(const float* pose, const float* weights, int32_t n_cameras, const int64_t* camera_indices,
                         const float* directions, const float* grad_origins, const float* grad_directions, int64_t r,
                         void* workspace, float* grad_pose, float* grad_in_origins, float* grad_in_directions, void* stream);

/* ---- the training step's glue as kernels (csrc/train_fused.hip) ---------------------------------------------------
 * What the reference spreads over dozens of elementwise torch ops per step between the field / sampler kernels.
 * `edges` is a bin-edge tensor e[R, >= S+1] with row stride edge_stride (floats): sample s of a ray spans
 * [e[s], e[s+1]] -- the [R,S,1] starts / ends / deltas views of cameras/rays.py:313-357 are never materialised.   */

/* RaySamples.get_weights (cameras/rays.py:188-210) + render_depth_simple of the round (models/neurad.py:396,727-734):
 * weights [R,S] = nan_to_num((1 - exp(-delta*dens)) * exp(-exclusive_cumsum(delta*dens))), depth [R] (may be NULL)
 * = sum_s weights * (e[s] + e[s+1]) / 2.                                                                            */
int nrhip_prop_weights_fwd(const float* edges, int32_t edge_stride, const float* densities /*[R,S]*/, int64_t r,
                           int32_t s, float* weights, float* depth, void* stream);
/* its autograd: grad_densities [R,S] from grad_weights [R,S] and / or grad_depth [R] (either may be NULL) */
int nrhip_prop_weights_bwd(const float* edges, int32_t edge_stride, const float* densities, const float* grad_weights,
                           const float* grad_depth, int64_t r, int32_t s, float* grad_densities, void* stream);

/* SigmoidDensity (model_components/utils.py:21-41; `beta` = DEVICE pointer to the raw learnable parameter, the kernel
 * applies |beta| + beta_min) -> nerfacc.render_weight_from_alpha -> accumulation -> sky residual on the last sample ->
 * features over all S samples, depth over the first S-1 (models/neurad.py:377-395).  alpha [R,S] (saved for the
 * backward), weights_ns [R,S-1] = the weights of the non-sky samples (`weights[..., :-1, :]` of models/neurad.py:388),
 * out_features rows of out_stride floats (>= C: room for the appearance embedding beside them), depth / acc [R].   */
int nrhip_sdf_render_fwd(const float* sdf /*[R,S]*/, const float* beta, float beta_min, const float* features /*[R,S,C]*/,
                         const float* edges, int32_t edge_stride, int64_t r, int32_t s, int32_t c, float* alpha,
                         float* weights_ns, float* out_features, int32_t out_stride, float* out_depth, float* out_acc,
                         void* stream);
/* floats of scratch nrhip_sdf_render_bwd needs (host out-pointer) */
int nrhip_sdf_render_bwd_workspace(int64_t r, int64_t* floats);
/* backward of the above: g_features rows of g_stride floats, g_depth / g_acc [R] and g_weights_ns [R,S-1] may be NULL;
 * -> grad_features [R,S,C], grad_sdf [R,S], grad_beta [1] (w.r.t. the raw parameter, sign(beta) applied; summed in a
 * fixed order: reproducible)                                                                                          */
int nrhip_sdf_render_bwd(const float* sdf, const float* beta, float beta_min, const float* alpha, const float* features,
                         const float* edges, int32_t edge_stride, const float* g_features, int32_t g_stride,
                         const float* g_depth, const float* g_acc, const float* g_weights_ns, int64_t r, int32_t s,
                         int32_t c, float* grad_features, float* grad_sdf, float* grad_beta, float* workspace,
                         void* stream);

/* NeuRADModel._get_appearance_embedding (models/neurad.py:423-441) with the slot arithmetic in the kernel:
 * t = times / duration * n_per_sensor, lo = clamp(floor(t)), hi = clamp(lo + 1), out = E[lo + sensor*n] (1 - (t - lo))
 * + E[hi + sensor*n] (t - lo); temporal = 0 (or times NULL): out = E[sensor].  sensor_idx may be NULL (= 0).  Rows of
 * `out` are out_stride floats apart.  Indices are clamped into the table.                                            */
int nrhip_appearance_fwd(const float* weight /*[E,D]*/, const int64_t* sensor_idx /*[R]*/, const float* times /*[R]*/,
                         float duration, int32_t n_per_sensor, int32_t temporal, int64_t r, int32_t n_embed, int32_t dim,
                         float* out, int32_t out_stride, void* stream);
/* gradient to the embedding table [E,D] (written, not accumulated) */
int nrhip_appearance_bwd(const float* g_out, int32_t g_stride, const int64_t* sensor_idx, const float* times,
                         float duration, int32_t n_per_sensor, int32_t temporal, int64_t r, int32_t n_embed, int32_t dim,
                         float* grad_weight, void* stream);

/* rows [n_out] (in order; the first n_out set positions) of a uint8 ray mask [R] + inverse [R] (slot of the row or -1)
 * + count [1] (all may be NULL): what `x[mask]` needs a nonzero + a device->host read for (models/neurad.py:478,485). */
int nrhip_mask_compact(const uint8_t* mask, int64_t r, int64_t* rows, int64_t n_out, int32_t* inverse, int32_t* count,
                       void* stream);

/* The lidar terms of NeuRADModel.get_metrics_dict (models/neurad.py:485-521) over the n lidar rays of a batch:
 * depths: HOST array of n_levels DEVICE pointers [R] (level 0 = the field's depth, 1.. = prop_depth_i), read at
 * lidar_rows [n].  metrics [2 + n_levels] = depth_loss (mean over the rays below the `quantile` of the per-ray error,
 * torch.quantile's linear interpolation), intensity_loss (same rays & returned), ray_drop_loss (BCE with logits, target
 * = no return), depth_loss_0, ...  unit_grads [(n_levels + 2), n] and scratch (nrhip_lidar_losses_workspace floats) carry
 * what the backward needs.  A per-ray pass + one single-workgroup pass; the quantile is a radix select, nothing is sorted. */
int nrhip_lidar_losses_workspace(int64_t n, int64_t* floats /*host*/);
int nrhip_lidar_losses(const float* const* depths, int32_t n_levels, const int64_t* lidar_rows, const float* distance,
                       const uint8_t* did_return, const float* intensity, const float* intensity_target,
                       const float* ray_drop_logits, int64_t n, float non_return_distance, float non_return_mult,
                       float quantile, float* metrics, float* unit_grads, float* scratch, void* stream);
/* d metrics / d predictions x upstream [2 + n_levels] (device) scattered to the batch: grad_depths = HOST array of
 * n_levels DEVICE pointers [R] (0 for camera rays; entries may be NULL), grad_intensity / grad_logits [n] (may be NULL);
 * unit_grads / scratch / did_return as given to (and filled by) nrhip_lidar_losses, inverse [R] from nrhip_mask_compact */
int nrhip_lidar_losses_bwd(const float* unit_grads, const float* scratch, const uint8_t* did_return, const int32_t* inverse,
                           const float* upstream, int32_t n_levels, int64_t r, int64_t n, float* const* grad_depths,
                           float* grad_intensity, float* grad_logits, void* stream);

/* ---- the level-sparse gradient exchange (opt-in; the reference's DDP all-reduce, pipelines/base_pipeline.py:304-307,
 *      sends every level of a hash table densely).  grad [n_levels * rows_per_level, f] fp32, 16-byte aligned.
 * count  : block_counts [n_levels, ceil(rows_per_level / NRHIP_GRAD_ROWS_PER_BLOCK)] = non-zero rows per block, turned into their
 *          exclusive prefix per level before the call returns; level_counts [n_levels] int64 = non-zero rows per level.
 * compact: the levels `levels[i]` (i < n_list_levels <= 32) as ordered lists: entries [sum caps[<i], + caps[i]) of rows (int32,
 *          level-local, ascending; the CALLER pre-fills -1: padding up to the capacity agreed between the ranks) and of vals
 *          [., f] = grad * scale.  block_offsets = count's block_counts.
 * apply  : mode 0: grad[level, row] = 0; mode 1: grad[level, row] += vals -- for the entries with row >= 0 of a list laid out
 *          the same way.  The rows of one list are distinct: no atomics, and lists applied in a fixed order give every rank
 *          bit-identical sums.                                                                                              */
#define NRHIP_GRAD_ROWS_PER_BLOCK 256 /* blocks per level = ceil(rows_per_level / 256) */
int nrhip_grad_rows_count(const float* grad, int32_t n_levels, int64_t rows_per_level, int32_t f, uint32_t* block_counts,
                          int64_t* level_counts, void* stream);
int nrhip_grad_rows_compact(const float* grad, int32_t n_levels, int64_t rows_per_level, int32_t f,
                            const uint32_t* block_offsets, const int32_t* levels /*host*/, const int64_t* caps /*host*/,
                            int32_t n_list_levels, float scale, int32_t* rows, float* vals, void* stream);
int nrhip_grad_rows_apply(float* grad, int32_t n_levels, int64_t rows_per_level, int32_t f, const int32_t* levels /*host*/,
                          const int64_t* caps /*host*/, int32_t n_list_levels, const int32_t* rows, const float* vals,
                          int32_t mode, void* stream);

/* ---- (f)-1: RGB CNN decoder (models/neurad.py:198-216,359-366; model_components/cnns.py:20-46) on fp16 operands with
 *          fp32 accumulation -- the arithmetic of the reference's mixed-precision trainer.  Activations are NHWC fp16:
 *          [B, H, W, 32].                                                                                              */
/* torch Conv2d weight [32][32][7][7] fp32 -> the kernel's fragment order, 49*2*64*16 bytes.  mode 0: forward (replaces
 * the four BasicBlocks' Conv2d.forward, cnns.py:38-44); mode 1: the same convolution's input gradient (flipped taps,
 * channels swapped), i.e. nrhip_conv7x7 on a packed mode-1 weight IS conv2d_backward w.r.t. the input.               */
int nrhip_conv7x7_pack(const float* weight, int32_t mode, void* wfrag, void* stream);
/* the same for up to 8 convolutions in one launch: weights = HOST array of n device pointers; wfrag [n][2][49*2*64*16 bytes]
 * receives mode 0 and mode 1 of every weight (the decoder packs once per step).                                       */
int nrhip_conv7x7_pack_many(const float* const* weights, int32_t n, void* wfrag, void* stream);
/* workgroups per image for an h x w image (a workgroup covers 4*rows_per_wave rows x 32 columns): stats_partial below is
 * [b * tiles, 64] floats.                                                                                             */
int nrhip_conv7x7_tiles(int32_t h, int32_t w, int32_t rows_per_wave, int32_t* tiles);
/* out = conv7x7(in, padding 3) + bias (bias may be NULL).  stats_partial (optional): per workgroup the sum and the sum
 * of squares of the ROUNDED outputs per channel (BatchNorm2d's batch statistics, cnns.py:40,43, in a fixed order).
 * rows_per_wave in {1, 2, 4}.                                                                                          */
int nrhip_conv7x7(const void* in, const void* wfrag, const float* bias, void* out, float* stats_partial, int32_t b,
                  int32_t h, int32_t w, int32_t rows_per_wave, void* stream);
/* Weight and bias gradient of the same convolution (conv2d_backward w.r.t. weight / bias): x = the convolution's input,
 * grad_out = the gradient of its output, both NHWC fp16.  grad_weight [32][32][7][7] and grad_bias [32] (optional) are fp32
 * and ACCUMULATED into.  workspace: nrhip_conv7x7_wgrad_workspace floats (per-workgroup partial sums, reduced in a fixed
 * order: bit-reproducible).                                                                                            */
int nrhip_conv7x7_wgrad_workspace(int32_t b, int32_t h, int32_t w, int64_t* floats);
int nrhip_conv7x7_wgrad(const void* x, const void* grad_out, float* workspace, float* grad_weight, float* grad_bias,
                        const float* grad_scale, int32_t b, int32_t h, int32_t w, void* stream);

/* The decoder's other layers.  All reductions over pixels go through per-workgroup partial sums in `workspace` that are
 * added in a fixed order; gradients of parameters are ACCUMULATED into (caller zeroes), fp32, in torch's layouts.
 * grad_scale (optional, every backward entry point): device {S, 1/S} from nrhip_dec_grad_scale.  The fp16 gradient
 * tensors inside the decoder carry the factor S -- the per-call equivalent of the loss scale the reference's
 * mixed-precision trainer applies (engine/trainer.py:189,553), without which gradients of order 1e-7 fall into fp16's
 * subnormals -- and every fp32 result (parameter gradients, grad_features) is multiplied by 1/S.                       */
/* scale [3 floats: S, 1/S, scratch]: S = the power of two that brings max |grad| into [0.5, 1)                        */
int nrhip_dec_grad_scale(const float* grad, int64_t n, float* scale, void* stream);
/* BatchNorm2d, training mode (cnns.py:40,43; functional.batch_norm): batch statistics from nrhip_conv7x7's stats_partial
 * [n_partial, 64]; coef [4][32] = scale, shift, mean, rstd; running_mean / running_var (both or neither) are updated as
 * torch does (momentum, unbiased variance).                                                                            */
int nrhip_dec_bn_finalize(const float* stats_partial, int32_t n_partial, int64_t count, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                          float* coef, void* stream);
/* out = relu(c * scale + shift [+ skip]) with the reference's fp16 roundings (BasicBlock.forward, cnns.py:31,38-44)   */
int nrhip_dec_bn_act(const void* c, const float* coef, const void* skip, void* out, int64_t n_pixels, void* stream);
/* backward of the above w.r.t. c (and gamma, beta): grad_c = batch_norm_backward(grad_out * (act > 0)), act = the
 * forward's output.  workspace: nrhip_dec_bn_bwd_workspace floats.                                                     */
int nrhip_dec_bn_bwd_workspace(int64_t n_pixels, int64_t* floats);
int nrhip_dec_bn_bwd(const void* grad_out, const void* act, const void* c, const float* gamma, const float* coef,
                     float* workspace, float* grad_gamma, float* grad_beta, const float* grad_scale, void* grad_c,
                     int64_t n_pixels, void* stream);
/* out = a + grad_out * (act > 0): a residual block's input gradient (convolution path + skip path)                    */
int nrhip_dec_add_masked(const void* a, const void* grad_out, const void* act, void* out, int64_t n_pixels, void* stream);
/* Conv2d(cin, 32, 1) + ReLU on the rendered feature rows (models/neurad.py:201-203, 361-364): features [n, cin] fp32 ->
 * h [n, 32] fp16; and its backward (grad_features [n, cin] fp32 is written, not accumulated).                          */
int nrhip_dec_conv1x1_in_fwd(const float* features, const float* weight /*[32,cin]*/, const float* bias, void* out,
                             int64_t n, int32_t cin, void* stream);
int nrhip_dec_conv1x1_in_bwd_workspace(int64_t n, int32_t cin, int64_t* floats);
int nrhip_dec_conv1x1_in_bwd(const float* features, const void* h, const void* grad_h, const float* weight,
                             float* workspace, float* grad_features, float* grad_weight, float* grad_bias,
                             const float* grad_scale, int64_t n, int32_t cin, void* stream);
/* ConvTranspose2d(32, 32, kernel_size = stride = 3) (models/neurad.py:206-211): [b,h,w,32] -> [b,3h,3w,32] as nine
 * [pixels,32] x [32,32] products on the matrix cores.  pack: weight [32 in][32 out][3][3] fp32 -> wup, 2*9*2*64*16 bytes
 * (forward and input-gradient fragment orders).                                                                        */
int nrhip_dec_upsample_pack(const float* weight, void* wup, void* stream);
int nrhip_dec_upsample_fwd(const void* h, const void* wup, const float* bias, void* out, int32_t b, int32_t hh, int32_t w,
                           void* stream);
int nrhip_dec_upsample_bwd_workspace(int32_t b, int32_t hh, int32_t w, int64_t* floats);
int nrhip_dec_upsample_bwd(const void* h, const void* grad_out, const void* wup, float* workspace, void* grad_h,
                           float* grad_weight, float* grad_bias, const float* grad_scale, int32_t b, int32_t hh, int32_t w,
                           void* stream);
/* Conv2d(32, 3, 1) + Sigmoid (models/neurad.py:214-215): rgb [n_pixels, 3] fp32, and its backward                    */
int nrhip_dec_rgb_fwd(const void* h, const float* weight /*[3,32]*/, const float* bias, float* rgb, int64_t n_pixels,
                      void* stream);
int nrhip_dec_rgb_bwd_workspace(int64_t n_pixels, int64_t* floats);
int nrhip_dec_rgb_bwd(const void* h, const float* rgb, const float* grad_rgb, const float* weight, float* workspace,
                      void* grad_h, float* grad_weight, float* grad_bias, const float* grad_scale, int64_t n_pixels,
                      void* stream);

/* The whole decoder behind one entry point per direction (what a binding needs; the per-layer entry points above are its
 * parts and stay callable).  Parameters in torch's layouts, fp32; features [n_patches * patch_h * patch_w, cin] fp32 in
 * patch order (models/neurad.py:361-362); rgb [n_patches, 3 patch_h, 3 patch_w, 3] fp32.  conv_w/conv_b/bn_*[2k + j] =
 * convolution j (0: first, 1: second) of BasicBlock k (0, 1 before the upsampling, 2, 3 after).                        */
typedef struct {
  int32_t n_patches, patch_h, patch_w, cin;
  int32_t training; /* BatchNorm2d: 1 = batch statistics (running statistics are updated), 0 = running statistics      */
  const float* conv_in_w; /* [32, cin] */
  const float* conv_in_b;
  const float* conv_w[8]; /* [32, 32, 7, 7] */
  const float* conv_b[8];
  const float* bn_gamma[8];
  const float* bn_beta[8];
  float* bn_running_mean[8];
  float* bn_running_var[8];
  float bn_eps[8];
  float bn_momentum[8];
  const float* up_w; /* [32 in, 32 out, 3, 3] */
  const float* up_b;
  const float* out_w; /* [3, 32] */
  const float* out_b;
} nrhip_rgb_decoder;
/* bytes of `saved` (activations kept for the backward) and `workspace` (scratch), floats of grad_params                */
int nrhip_rgb_decoder_sizes(const nrhip_rgb_decoder* d, int64_t* saved_bytes, int64_t* workspace_bytes,
                            int64_t* grad_param_floats);
int nrhip_rgb_decoder_fwd(const nrhip_rgb_decoder* d, const float* features, void* saved, void* workspace, float* rgb,
                          void* stream);
/* grad_params (written, not accumulated): conv_in (w, b), then per convolution i = 0..7 (w, b, gamma, beta), up (w, b),
 * out (w, b).  training == 0: BatchNorm normalised with its running statistics in the forward, its backward is then the
 * affine map gamma * rstd * g (round 4).                                                                               */
int nrhip_rgb_decoder_bwd(const nrhip_rgb_decoder* d, const float* features, const void* saved, const float* rgb,
                          const float* grad_rgb, void* workspace, float* grad_features, float* grad_params, void* stream);

/* ---- VGG-19 perceptual loss (model_components/losses.py:582-625): the network up to relu5_1 on cat([rgb, image]), L1 on
 *          the five relu{i}_1 features, a gradient into the rendered half.  Activations and gradients are NHWC fp16,
 *          accumulation is fp32.  Channel counts are 3, 64, 128, 256 or 512; the 3-channel (image) side is STORED with
 *          NRHIP_VGG_IMAGE_CHANNELS channels, the rest zero.
 *
 * Working scale.  A fp16 gradient tensor comes with a device `state` of two floats {amax, S}: stored = S * true with S a
 * power of two, amax = the largest stored magnitude, kept by an unsigned atomic max on the float's bits (the caller zeroes
 * the state before the producer runs).  A consumer multiplies by the power of two p that brings amax into [0.5, 1) in its
 * epilogue -- exact -- and writes S_out = S_in * p.  A non-finite value makes amax, p and everything after it NaN.  There
 * is no host read.                                                                                                      */
#define NRHIP_VGG_IMAGE_CHANNELS 16
#define NRHIP_L1_ITEMS 2048 /* elements per workgroup of the L1 kernels */
/* torch Conv2d weight [cout][cin][3][3] fp32 -> fragment order, nrhip_conv3x3_pack_bytes bytes.  mode 0: forward;
 * mode 1: the same convolution's input gradient (taps flipped, channels swapped): nrhip_conv3x3(cin = cout, cout = cin)
 * on a mode-1 pack IS conv2d_backward w.r.t. the input.                                                                 */
int nrhip_conv3x3_pack_bytes(int32_t cout, int32_t cin, int32_t mode, int64_t* bytes);
int nrhip_conv3x3_pack(const float* weight, int32_t cout, int32_t cin, int32_t mode, void* wfrag, void* stream);
/* Host logic: the launch plan of a convolution over n_pixels = b * h * w pixels.  A wave owns 32 * pixel_blocks pixels x
 * 32 * channel_blocks output channels; plan 0 chooses pixel_blocks from n_pixels and cout alone, 1 or 2 forces it.
 * Every plan gives the same bits.                                                                                      */
int nrhip_conv3x3_plan(int64_t n_pixels, int32_t cin, int32_t cout, int32_t plan, int32_t* pixel_blocks,
                       int32_t* channel_blocks, int64_t* waves);
/* out [b,h,w,cout] = fp16(conv3x3(in [b,h,w,cin], pad 1) * p + bias), then ReLU if `relu`, then zero where mask <= 0
 * (mask: fp16, out's shape; the ReLU mask of the layer's stored input in the backward).  bias, mask, in_state, out_state
 * may be NULL; p = 1 without in_state; with out_state the kernel tracks amax and writes S_out.                         */
int nrhip_conv3x3(const void* in, const void* wfrag, const float* bias, const void* mask, const float* in_state,
                  float* out_state, void* out, int32_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t relu,
                  int32_t plan, void* stream);
/* max_pool2d(2, 2), floor mode, on [b,h,w,c] fp16 (c a multiple of 8) -> [b,h/2,w/2,c].  The backward recomputes the
 * first maximum of every window in row-major order from `in` (no index tensor) and writes ALL of grad_in: zero off the
 * maximum and in a dropped odd row / column.                                                                            */
int nrhip_maxpool2_fwd(const void* in, void* out, int64_t b, int32_t h, int32_t w, int32_t c, void* stream);
int nrhip_maxpool2_bwd(const void* in, const void* grad_out, const float* in_state, float* out_state, void* grad_in,
                       int64_t b, int32_t h, int32_t w, int32_t c, void* stream);
/* out [1] = (accum ? *accum : 0) + weight * mean |fx - fy| over n fp16 elements: float64 per-workgroup partials
 * (NRHIP_L1_ITEMS elements each) in `workspace`, added in a fixed order, one rounding to fp32.  Bit-reproducible.         */
int nrhip_l1_feature_workspace(int64_t n, int64_t* bytes);
int nrhip_l1_feature_fwd(const void* fx, const void* fy, int64_t n, float weight, const float* accum, void* workspace,
                         int64_t workspace_bytes, float* out, void* stream);
/* grad_fx = S * (weight * grad_loss[0] / n * sign(fx - fy) (* [fx > 0] if mask_fx) + above / S_above), sign(0) = 0, as
 * fp16.  Without `above` S brings the constant into [0.5, 1) and the value is rounded once from float64; with `above`
 * (a gradient tensor of the same shape and its state) both are brought to a common power of two and added in fp32.      */
int nrhip_l1_feature_bwd(const void* fx, const void* fy, int64_t n, float weight, const float* grad_loss, int32_t mask_fx,
                         const void* above, const float* above_state, float* out_state, void* grad_fx, void* stream);
/* cat([x, y]) of two fp32 [n_pixels, 3] images -> fp16 [2 * n_pixels, NRHIP_VGG_IMAGE_CHANNELS]                         */
int nrhip_vgg_stage_images(const float* x, const float* y, int64_t n_pixels, void* out, void* stream);
/* grad [n_pixels, 3] fp32 = grad16 [n_pixels, NRHIP_VGG_IMAGE_CHANNELS] / S (state = {amax, S} of grad16)               */
int nrhip_vgg_image_grad(const void* grad16, const float* state, int64_t n_pixels, float* grad, void* stream);

/* ---- LPIPS (torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True), models/neurad.py:267,587):
 *          AlexNet features of cat([a, b]) tapped after each ReLU, unit-normalised per pixel, a weighted squared difference
 *          per tap, the pixel mean.  Forward only.  Activations are NHWC fp16, accumulation is fp32; the image is STORED with
 *          NRHIP_LPIPS_IMAGE_CHANNELS channels, the last zero.                                                              */
#define NRHIP_LPIPS_IMAGE_CHANNELS 4
#define NRHIP_LPIPS_MIN_SIZE 31      /* below it AlexNet's second pool is empty */
#define NRHIP_LPIPS_HEAD_PIXELS 32   /* pixels per workgroup (and per float64 partial) of the head */
#define NRHIP_LPIPS_EPS_INSIDE 0     /* n(f) = f / sqrt(eps + sum f^2)   (torchmetrics, eps = 1e-8)  */
#define NRHIP_LPIPS_EPS_OUTSIDE 1    /* n(f) = f / (sqrt(sum f^2) + eps) (the lpips package, 1e-10) */
/* cat([a, b]) of two fp32 [n_pixels, 3] images in [0, 1] -> fp16 [2 * n_pixels, NRHIP_LPIPS_IMAGE_CHANNELS] holding
 * (2 v - 1 - shift[c]) / scale[c], evaluated in float64 and rounded to fp32, then to fp16.  *flag (the caller zeroes it) is
 * set to 1 when any value is outside [0, 1] or not finite; the call does not read it.                                      */
int nrhip_lpips_stage_images(const float* a, const float* b, int64_t n_pixels, const float* shift, const float* scale,
                             void* out, int32_t* flag, void* stream);
/* One implicit-GEMM convolution, for exactly AlexNet's five layers (cin -> cout, ksize, stride, pad): 3 -> 64, 11, 4, 2;
 * 64 -> 192, 5, 1, 2; 192 -> 384, 384 -> 256 and 256 -> 256, 3, 1, 1.  Anything else is NRHIP_ERR_UNSUPPORTED.
 * Host logic: the plan over n_pixels OUTPUT pixels.  A wave owns 32 * pixel_blocks pixels x 32 * channel_blocks channels;
 * plan 0 chooses pixel_blocks from n_pixels and cout, 1 or 2 forces it.  Every plan gives the same bits.                   */
int nrhip_conv2d_plan(int64_t n_pixels, int32_t cin, int32_t cout, int32_t ksize, int32_t stride, int32_t pad, int32_t plan,
                      int32_t* pixel_blocks, int32_t* channel_blocks, int64_t* waves);
/* torch Conv2d weight [cout][cin][ksize][ksize] fp32 -> fragment order, nrhip_conv2d_pack_bytes bytes; reduction indices
 * that are padding (the image's 4th channel, the 12th tap of an 11-tap row) hold zeros.                                    */
int nrhip_conv2d_pack_bytes(int32_t cout, int32_t cin, int32_t ksize, int64_t* bytes);
int nrhip_conv2d_pack(const float* weight, int32_t cout, int32_t cin, int32_t ksize, void* wfrag, void* stream);
/* out [b, ho, wo, cout] = fp16(conv(in [b, h, w, cin]) + bias), then ReLU if `relu`; ho = (h + 2 pad - ksize) / stride + 1.
 * bias may be NULL.  The image layer needs h, w >= NRHIP_LPIPS_MIN_SIZE.                                                    */
int nrhip_conv2d(const void* in, const void* wfrag, const float* bias, void* out, int32_t b, int32_t h, int32_t w, int32_t cin,
                 int32_t cout, int32_t ksize, int32_t stride, int32_t pad, int32_t relu, int32_t plan, void* stream);
/* max_pool2d(3, 2), floor mode, no padding, on [b,h,w,c] fp16 (h, w >= 3, c a multiple of 8) -> [b,(h-3)/2+1,(w-3)/2+1,c]   */
int nrhip_maxpool3s2_fwd(const void* in, void* out, int64_t b, int32_t h, int32_t w, int32_t c, void* stream);
/* One tap's term.  feat [2 b, n_pixels, c] fp16 (the first b images against the second b), lin [c] fp32:
 * out[i] = (accumulate ? out[i] : 0) + mean_pixels sum_c lin[c] (n(fa)_c - n(fb)_c)^2, n as eps_mode says; fp32 per pixel,
 * float64 per-workgroup partials in `workspace` added in a fixed order, one rounding to fp32.  Bit-reproducible.           */
int nrhip_lpips_head_workspace(int64_t b, int64_t n_pixels, int64_t* bytes);
int nrhip_lpips_head(const void* feat, const float* lin, int64_t b, int64_t n_pixels, int32_t c, float eps, int32_t eps_mode,
                     int32_t accumulate, void* workspace, int64_t workspace_bytes, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEURAD_HIP_H_ */
