// Library plumbing: thread-local error string, argument validation, device info.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "common.h"

namespace nrhip {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return NRHIP_ERR_LAUNCH;
  }
  return NRHIP_OK;
}

static Tuning read_tuning() {
  Tuning t;
  auto env = [](const char* name) { return getenv(name); };
  auto is = [&](const char* name, char c) {
    const char* e = env(name);
    return e && e[0] == c;
  };
  t.bin_round_log2 = 23;
  if (const char* e = env("NRHIP_BIN_ROUND_LOG2")) {
    const int x = atoi(e);
    if (x >= 15 && x <= 24) t.bin_round_log2 = x;
  }
  t.bin_pairs = is("NRHIP_BIN_PAIRS", 'a') ? 1 : is("NRHIP_BIN_PAIRS", 'n') ? 0 : -1;
  t.bin_transpose = !is("NRHIP_BIN_TRANSPOSE", '0');
  t.bin_stats = env("NRHIP_BIN_STATS") != nullptr;
  t.multi_bwd_runs = !is("NRHIP_MULTI_BWD_RUNS", '0');
  t.pair_bwd_runs = !is("NRHIP_PAIR_BWD_RUNS", '0');
  t.mlp_generic = env("NRHIP_MLP_GENERIC") != nullptr;
  t.mlp_split_wgrad = env("NRHIP_MLP_SPLIT_WGRAD") != nullptr;
  t.mlp_split_bf16 = env("NRHIP_MLP_SPLIT_BF16") != nullptr;
  t.mlp_pairs = env("NRHIP_MLP_PAIRS") ? (is("NRHIP_MLP_PAIRS", '1') ? 1 : 0) : -1;
  t.mlp_pairs_train = is("NRHIP_MLP_PAIRS_TRAIN", '1');
  t.sampler_actor_inline = is("NRHIP_SAMPLER_ACTOR_INLINE", '1');
  t.sdf_render_pair = is("NRHIP_SDF_RENDER_PAIR", '1');
  return t;
}

static Tuning g_tuning = read_tuning();  // at library load

const Tuning& tuning() { return g_tuning; }

int validate_grid(const nrhip_grid* g) {
  NR_REQUIRE(g, NRHIP_ERR_INVALID_ARG, "grid descriptor is NULL");
  NR_REQUIRE(g->num_levels >= 1 && g->num_levels <= NRHIP_MAX_LEVELS, NRHIP_ERR_INVALID_ARG,
             "num_levels %d outside [1,%d]", g->num_levels, NRHIP_MAX_LEVELS);
  NR_REQUIRE(g->n_features == 1 || g->n_features == 2 || g->n_features == 4 || g->n_features == 8,
             NRHIP_ERR_UNSUPPORTED, "features_per_level %d not in {1,2,4,8}", g->n_features);
  NR_REQUIRE(g->log2_table_size >= 1 && g->log2_table_size <= 26 &&
                 (int64_t)g->num_levels << g->log2_table_size <= (int64_t)1 << 31,
             NRHIP_ERR_INVALID_ARG, "log2_table_size %d unsupported (L*T must fit 2^31 rows)", g->log2_table_size);
  NR_REQUIRE(((int64_t)g->num_levels << g->log2_table_size) * g->n_features * 4 <= (int64_t)1 << 32,
             NRHIP_ERR_UNSUPPORTED, "hash table larger than 4 GiB is not supported (32-bit byte offsets)");
  NR_REQUIRE(g->param_dtype == 0 || g->param_dtype == 1, NRHIP_ERR_INVALID_ARG, "param_dtype %d not in {0,1}",
             g->param_dtype);
  return NRHIP_OK;
}

int validate_rays(const nrhip_rays* r) {
  NR_REQUIRE(r, NRHIP_ERR_INVALID_ARG, "rays descriptor is NULL");
  NR_REQUIRE(r->n_rays >= 0 && r->n_samples >= 0, NRHIP_ERR_INVALID_ARG, "negative ray/sample count");
  NR_REQUIRE(r->sample_stride == 0 || r->sample_stride >= r->n_samples, NRHIP_ERR_INVALID_ARG, "sample_stride < n_samples");
  if (r->n_rays == 0 || r->n_samples == 0) return NRHIP_OK;
  NR_REQUIRE(r->origins && r->directions && r->pixel_area && r->starts && r->ends, NRHIP_ERR_INVALID_ARG,
             "rays descriptor has a NULL pointer");
  return NRHIP_OK;
}

int validate_packed_rays(const char* who, const nrhip_packed_rays* r, bool need_segments) {
  NR_REQUIRE(r, NRHIP_ERR_INVALID_ARG, "%s: rays descriptor is NULL", who);
  NR_REQUIRE(r->n_rays >= 0 && r->n_samples >= 0, NRHIP_ERR_INVALID_ARG, "%s: negative ray/sample count", who);
  NR_REQUIRE(r->n_samples < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "%s: M >= 2^31", who);
  if (r->n_rays == 0 || r->n_samples == 0) return NRHIP_OK;
  NR_REQUIRE(r->origins && r->directions && r->pixel_area && r->t_starts && r->t_ends && (r->segments || !need_segments),
             NRHIP_ERR_INVALID_ARG, "%s: rays descriptor has a NULL pointer", who);
  return NRHIP_OK;
}

int validate_points(const char* who, const float* points, int32_t stride, int64_t n) {
  NR_REQUIRE(n >= 0, NRHIP_ERR_INVALID_ARG, "%s: negative count", who);
  NR_REQUIRE(stride >= 3, NRHIP_ERR_INVALID_ARG, "%s: row stride %d < 3 floats", who, stride);
  NR_REQUIRE(n < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "%s: count >= 2^31", who);
  NR_REQUIRE(points || n == 0, NRHIP_ERR_INVALID_ARG, "%s: NULL pointer with %lld points", who, (long long)n);
  return NRHIP_OK;
}

}  // namespace nrhip

extern "C" const char* nrhip_last_error(void) { return nrhip::g_err; }
// 200: nrhip_rays.order, render_fwd_ex, ray_order.  300: nrhip_field grew eval_table / eval_layout (trailing), the training
// glue of train_fused.hip, nrhip_field_fwd_train_ovr, nrhip_eval_layout_*.
// 510: nrhip_encode_bwd_binned / nrhip_hashgrid_bwd_binned write fp32 gradients whatever g->param_dtype says (the fp16 form
// is nrhip_encode_bwd_binned_f16); nrhip_adam_step_many_dev (+ _workspace), nrhip_tuning_reload.
// 511: nrhip_nonfinite_check_many.
// 512: packed compositing: nrhip_packed_segments, nrhip_packed_weight_from_density / _alpha (+ _bwd),
// nrhip_packed_accumulate (+ _bwd), nrhip_packed_composite_fwd / _bwd.
// 513: occupancy-grid maintenance: nrhip_occgrid_march_levels, nrhip_occgrid_update_workspace / _candidates / _apply,
//      nrhip_occgrid_mark_invisible
// 514: nrhip_render_fwd_packed (+ nrhip_packed_rays): the fused render kernel on packed samples
// 515: training on packed samples: nrhip_field_fwd_train_packed, nrhip_sdf_render_packed_fwd / _bwd / _bwd_workspace,
//      nrhip_encode_bwd_binned_packed / _f16
// 516: nrhip_encode_bwd_rays_packed: ray gradients through packed samples
// 517: nrhip_camera_rays_lens (+ nrhip_camera_lens): FISHEYE and lens-distorted cameras
// 518: nrhip_occgrid_march_levels_actors, nrhip_render_fwd_packed_actors: the occupancy route with dynamic actors (eval)
// 519: training on packed samples of a scene with dynamic actors: nrhip_field_fwd_train_packed_ovr, nrhip_actor_find_packed,
//      nrhip_actor_pair_positions_fwd_packed / _bwd_packed
// 520: lidar scan evaluation: nrhip_nearest_sq_dist (+ nrhip_nearest_plan), nrhip_chamfer_distance (+ _workspace)
//      additive, same number: the VGG perceptual loss -- nrhip_conv3x3 (+ _pack, _pack_bytes, _plan), nrhip_maxpool2_fwd /
//      _bwd, nrhip_l1_feature_fwd / _bwd (+ _workspace), nrhip_vgg_stage_images, nrhip_vgg_image_grad
//      additive, same number: camera image evaluation -- nrhip_image_metrics (+ _workspace), nrhip_image_psnr
//      additive, same number: camera pose correction -- nrhip_pose_apply, nrhip_pose_apply_bwd (+ _workspace)
//      additive, same number: median depth -- nrhip_median_depth, nrhip_median_depth_packed
//      additive, same number: surface normals -- nrhip_field_normals, nrhip_field_normals_packed
extern "C" int nrhip_version(void) { return 520; }

extern "C" int nrhip_tuning_reload(void) {
  nrhip::g_tuning = nrhip::read_tuning();
  return NRHIP_OK;
}

extern "C" int nrhip_device_info(int32_t* n_cus, int32_t* n_xcds, int64_t* hbm_bytes) {
  int dev = 0;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) {
    nrhip::set_error("device_info: no HIP device");
    return NRHIP_ERR_LAUNCH;
  }
  if (n_cus) *n_cus = p.multiProcessorCount;
  if (n_xcds) *n_xcds = 8;
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  return NRHIP_OK;
}
