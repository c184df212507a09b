// ray generation on the device -- the step immediately before the hot path.
//
//   nrhip_camera_rays      == Cameras._generate_rays_from_coords for PERSPECTIVE cameras without lens distortion, incl. the
//                             rolling-shutter correction of origins and times (nerfstudio/cameras/cameras.py:560-968);
//   nrhip_camera_rays_lens == the same for PERSPECTIVE or FISHEYE cameras with OpenCV lens distortion k1 k2 k3 k4 p1 p2
//                             (camera_utils.py:655-758).  All cameras of a call share the type and the kernel is compiled
//                             per type, so a wave never diverges on it;
//   nrhip_lidar_rays       == Lidars._generate_rays_from_points (nerfstudio/cameras/lidars.py:399-460).
//
// The reference runs ~40 torch ops per batch for each (index_select of the per-sensor tables, stacks, masked selects,
// norms) and, with distortion, ten Newton iterations of ~60 ops each over a [3,R,2] stack.  Here one thread produces one
// ray: the sensor row is a handful of broadcast loads (rays of a 32x32 patch share one camera; lidar points of a scan
// share one lidar), the Newton solve of the pixel and its two neighbours stays in registers, outputs go out as whole
// [R,3] / [R,1] rows.
//
// What is mirrored, and how that was established.  A ray's direction feeds floor() in every hash-grid level downstream, so
// the perspective and lidar kernels reproduce the BITS of the reference's fp32 CPU run (tests/golden/raygen.npz, made by
// oracle/make_golden_raygen.py): origins, times, directions, norms and lidar pixel areas on every ray of the fixture,
// camera pixel areas to 2 ulp (bit-equal on 99 % of rays; the rest is the order torch's sum takes over a 3-element inner
// dimension).  Every product, sum and quotient is rounded on its own (-ffp-contract=off; the divide and sqrtf are the
// correctly rounded ones), in the order torch applies them, with ONE exception found by comparing candidate roundings with
// that fixture: torch.linalg.vector_norm's CPU kernel accumulates the squares as an FMA chain (norm3 below).  The
// separately rounded form sat 1-2 ulp off on ~6 % of camera and ~12 % of lidar rays.  tests/raygen_refs.py restates the
// kernels in numpy float32 and is pinned to the fixture (tests/test_raygen_refs_host.py); tests/test_gpu_raygen_exact.py
// holds the kernels to it bit for bit.  The reference's GPU-side vector_norm has not been compared: nobody has measured
// how it rounds.  The lens kernel shares finish_camera_ray, but its sinf / cosf are bounded against a float64 run instead.
//
// Mirrored, not repaired: a FISHEYE ray exactly at the principal point has theta = 0, where the reference's
// (u * sin theta) / theta is 0 * 0 / 0 = NaN (cameras.py:809-814).  Its direction and directions_norm are NaN, and so is
// the pixel area of that ray and of the rays one pixel to its left and one pixel above it, whose neighbour it is.  The
// lens kernel evaluates the same expressions and returns the same NaNs.
#include "common.h"

namespace nrhip {

constexpr float kNormEps = 8.8817841970012523e-16f;  // camera_utils._EPS = 4 * finfo(float64).eps, cast to fp32

struct Vec3 {
  float x, y, z;
};

__device__ __forceinline__ Vec3 rotate(const float* __restrict__ m /*3x4 row major*/, float a, float b, float c) {
#pragma clang fp contract(off)
  // torch.sum(d[..., None, :] * R, dim=-1): three separately rounded products, summed left to right
  Vec3 o;
  o.x = (a * m[0] + b * m[1]) + c * m[2];
  o.y = (a * m[4] + b * m[5]) + c * m[6];
  o.z = (a * m[8] + b * m[9]) + c * m[10];
  return o;
}

// torch.maximum(torch.linalg.vector_norm(v, dim=-1), _EPS) (camera_utils.py:596-608, cameras and lidars alike).  The sum
// of squares is the single-rounded FMA chain of vector_norm's CPU kernel, established from the CPU-made fixture (see the
// header); the explicit fmaf is the wanted contraction under contract(off).  A NaN norm stays NaN, as torch.maximum keeps
// it: fmaxf would return the epsilon, and a lidar point with a NaN coordinate would come out as a return at distance 9e-16.
__device__ __forceinline__ float norm3(Vec3 v) {
#pragma clang fp contract(off)
  const float n = sqrtf(fmaf(v.z, v.z, fmaf(v.y, v.y, v.x * v.x)));
  return n < kNormEps ? kNormEps : n;
}

struct CameraTable {
  const float* c2w;    // [C,3,4]
  const float* fx;     // [C]
  const float* fy;
  const float* cx;
  const float* cy;
  const float* times;  // [C] or NULL
  // rolling shutter (all three or none): cameras.py:937-960
  const float* rs_time;         // [C] rolling_shutter_time
  const float* time_to_center;  // [C]
  const float* velocities;      // [C,3]
  const float* extent;          // [C] image height (vertical shutter) or width (horizontal)
  int rs_mode;                  // 0 none, 1 vertical (rows), 2 horizontal (cols), 3 horizontal reversed
};

// From the camera-frame directions of a pixel (d0) and of its +1 x / +1 y neighbours (d1, d2) to the ray: rotation into
// the world, normalisation, pixel area, rolling-shutter origin and time (cameras.py:900-960).
__device__ __forceinline__ void finish_camera_ray(const CameraTable& t, int64_t c, int64_t i, float x, float y, Vec3 d0,
                                                  Vec3 d1, Vec3 d2, float* __restrict__ origins,
                                                  float* __restrict__ directions, float* __restrict__ pixel_area,
                                                  float* __restrict__ dir_norm, float* __restrict__ times) {
#pragma clang fp contract(off)
  const float* m = t.c2w + 12 * c;
  d0 = rotate(m, d0.x, d0.y, d0.z), d1 = rotate(m, d1.x, d1.y, d1.z), d2 = rotate(m, d2.x, d2.y, d2.z);
  const float n0 = norm3(d0), n1 = norm3(d1), n2 = norm3(d2);
  d0.x /= n0, d0.y /= n0, d0.z /= n0;
  d1.x /= n1, d1.y /= n1, d1.z /= n1;
  d2.x /= n2, d2.y /= n2, d2.z /= n2;
  const float ax = d0.x - d1.x, ay = d0.y - d1.y, az = d0.z - d1.z;
  const float bx = d0.x - d2.x, by = d0.y - d2.y, bz = d0.z - d2.z;
  // torch.sqrt(torch.sum(a ** 2, dim=-1)): separately rounded, left to right -- not vector_norm, and not its FMA chain
  const float dx = sqrtf((ax * ax + ay * ay) + az * az), dy = sqrtf((bx * bx + by * by) + bz * bz);
  float ox = m[3], oy = m[7], oz = m[11];
  float tm = t.times ? t.times[c] : 0.f;
  if (t.rs_mode) {
    const float pos = t.rs_mode == 1 ? y : x;
    float off = (pos / t.extent[c] - 0.5f) * t.rs_time[c] + t.time_to_center[c];
    if (t.rs_mode == 3) off = -off;
    ox = ox + t.velocities[3 * c] * off, oy = oy + t.velocities[3 * c + 1] * off, oz = oz + t.velocities[3 * c + 2] * off;
    tm = tm + off;
  }
  origins[3 * i] = ox, origins[3 * i + 1] = oy, origins[3 * i + 2] = oz;
  directions[3 * i] = d0.x, directions[3 * i + 1] = d0.y, directions[3 * i + 2] = d0.z;
  pixel_area[i] = dx * dy;
  dir_norm[i] = n0;
  if (times) times[i] = tm;
}

__global__ __launch_bounds__(256) void camera_rays_kernel(CameraTable t, const int64_t* __restrict__ cam_idx,
                                                          const float* __restrict__ coords, int64_t n,
                                                          float* __restrict__ origins, float* __restrict__ directions,
                                                          float* __restrict__ pixel_area, float* __restrict__ dir_norm,
                                                          float* __restrict__ times) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cam_idx[i];
  const float y = coords[2 * i], x = coords[2 * i + 1];
  const float fx = t.fx[c], fy = t.fy[c], cx = t.cx[c], cy = t.cy[c];
  // image-plane coordinates and the two neighbours one pixel away (cameras.py:631-633), OpenCV -> OpenGL (:668)
  const float u0 = (x - cx) / fx, u1 = ((x - cx) + 1.f) / fx;
  const float v0 = -((y - cy) / fy), v1 = -(((y - cy) + 1.f) / fy);
  finish_camera_ray(t, c, i, x, y, {u0, v0, -1.f}, {u1, v0, -1.f}, {u0, v1, -1.f}, origins, directions, pixel_area,
                    dir_norm, times);
}

// ---- lens distortion and the fisheye model ----------------------------------------------------------------------------
constexpr int kPerspective = 1, kFisheye = 2;  // CameraType values (cameras.py:43-55)

// radial_and_tangential_undistort (camera_utils.py:721-758) of one point: Newton's method from the distorted point, exactly
// ten iterations, residual and Jacobian with the expression trees of _compute_residual_and_jacobian (:655-717) -- Python's
// precedence spelled out, every product and sum rounded on its own.  With all six coefficients zero the residual is 0 and
// the step -0: the point comes back bit for bit.
__device__ __forceinline__ void undistort(const float* __restrict__ k, float& px, float& py) {
#pragma clang fp contract(off)
  const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3], p1 = k[4], p2 = k[5];
  const float xd = px, yd = py;
  float x = xd, y = yd;
  for (int it = 0; it < 10; ++it) {
    const float r = x * x + y * y;
    const float d = 1.f + r * (k1 + r * (k2 + r * (k3 + r * k4)));
    const float fx = ((d * x + ((2.f * p1) * x) * y) + p2 * (r + (2.f * x) * x)) - xd;
    const float fy = ((d * y + ((2.f * p2) * x) * y) + p1 * (r + (2.f * y) * y)) - yd;
    const float d_r = k1 + r * (2.f * k2 + r * (3.f * k3 + (r * 4.f) * k4));
    const float d_x = (2.f * x) * d_r, d_y = (2.f * y) * d_r;
    const float fx_x = ((d + d_x * x) + (2.f * p1) * y) + (6.f * p2) * x;
    const float fx_y = (d_y * x + (2.f * p1) * x) + (2.f * p2) * y;
    const float fy_x = (d_x * y + (2.f * p2) * y) + (2.f * p1) * x;
    const float fy_y = ((d + d_y * y) + (2.f * p2) * x) + (6.f * p1) * y;
    const float den = fy_x * fx_y - fx_x * fy_y;
    const float x_num = fx * fy_y - fy * fx_y, y_num = fy * fx_x - fx * fy_x;
    const bool ok = fabsf(den) > 1e-3f;
    x = x + (ok ? x_num / den : 0.f);
    y = y + (ok ? y_num / den : 0.f);
  }
  px = x, py = y;
}

// image-plane point (OpenCV, undistorted) -> direction in the camera frame (OpenGL: v negated, cameras.py:667)
template <int kType>
__device__ __forceinline__ Vec3 camera_direction(float u, float v) {
#pragma clang fp contract(off)
  v = -v;
  if (kType == kPerspective) return {u, v, -1.f};
  // FISHEYE (cameras.py:800-815).  sinf / cosf, not the fast intrinsics: the direction feeds floor() downstream
  float theta = sqrtf(u * u + v * v);
  theta = theta < 0.f ? 0.f : (theta > 3.14159274101257324f ? 3.14159274101257324f : theta);  // torch.clip keeps a NaN
  const float s = sinf(theta);
  return {(u * s) / theta, (v * s) / theta, -cosf(theta)};
}

template <int kType>
__global__ __launch_bounds__(256) void camera_rays_lens_kernel(CameraTable t, const float* __restrict__ distortion,
                                                               const int64_t* __restrict__ cam_idx,
                                                               const float* __restrict__ coords, int64_t n,
                                                               float* __restrict__ origins, float* __restrict__ directions,
                                                               float* __restrict__ pixel_area, float* __restrict__ dir_norm,
                                                               float* __restrict__ times) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cam_idx[i];
  const float y = coords[2 * i], x = coords[2 * i + 1];
  const float fx = t.fx[c], fy = t.fy[c], cx = t.cx[c], cy = t.cy[c];
  // the pixel, its +1 x and its +1 y neighbour on the image plane (cameras.py:631-635)
  float u[3] = {(x - cx) / fx, ((x - cx) + 1.f) / fx, (x - cx) / fx};
  float v[3] = {(y - cy) / fy, (y - cy) / fy, ((y - cy) + 1.f) / fy};
  if (distortion) {
    const float* k = distortion + 6 * c;
    // an all-zero row passes through the solve unchanged: skipped (rays of a patch share the camera, the branch is uniform)
    if (k[0] != 0.f || k[1] != 0.f || k[2] != 0.f || k[3] != 0.f || k[4] != 0.f || k[5] != 0.f)
      for (int j = 0; j < 3; ++j) undistort(k, u[j], v[j]);
  }
  finish_camera_ray(t, c, i, x, y, camera_direction<kType>(u[0], v[0]), camera_direction<kType>(u[1], v[1]),
                    camera_direction<kType>(u[2], v[2]), origins, directions, pixel_area, dir_norm, times);
}

struct LidarTable {
  const float* l2w;         // [Ln,3,4]
  const float* times;       // [Ln] or NULL
  const float* velocities;  // [Ln,3] or NULL
  const float* hdiv;        // [Ln] horizontal beam divergence
  const float* vdiv;        // [Ln]
  int ego_compensated;
  float valid_distance;
};

__global__ __launch_bounds__(256) void lidar_rays_kernel(LidarTable t, const int64_t* __restrict__ lidar_idx,
                                                         const float* __restrict__ points, int point_dim, int64_t n,
                                                         float* __restrict__ origins, float* __restrict__ directions,
                                                         float* __restrict__ pixel_area, float* __restrict__ distance,
                                                         uint8_t* __restrict__ did_return, float* __restrict__ times) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t l = lidar_idx[i];
  const float* p = points + (int64_t)point_dim * i;
  const float* m = t.l2w + 12 * l;
  // transform_points_pairwise (lidars.py:550-564): bmm then + translation
  Vec3 w = rotate(m, p[0], p[1], p[2]);
  w.x = w.x + m[3], w.y = w.y + m[7], w.z = w.z + m[11];
  float ox = m[3], oy = m[7], oz = m[11];
  const float dt = point_dim >= 5 ? p[4] : 0.f;
  if (point_dim >= 5 && t.velocities) {  // motion of the sensor during the sweep (lidars.py:420-426)
    const float vx = dt * t.velocities[3 * l], vy = dt * t.velocities[3 * l + 1], vz = dt * t.velocities[3 * l + 2];
    ox = ox + vx, oy = oy + vy, oz = oz + vz;
    if (!t.ego_compensated) w.x = w.x + vx, w.y = w.y + vy, w.z = w.z + vz;
  }
  Vec3 d{w.x - ox, w.y - oy, w.z - oz};
  const float dist = norm3(d);
  origins[3 * i] = ox, origins[3 * i + 1] = oy, origins[3 * i + 2] = oz;
  directions[3 * i] = d.x / dist, directions[3 * i + 1] = d.y / dist, directions[3 * i + 2] = d.z / dist;
  pixel_area[i] = t.hdiv[l] * t.vdiv[l];
  distance[i] = dist;
  did_return[i] = dist < t.valid_distance ? 1 : 0;
  if (times) times[i] = (t.times ? t.times[l] : 0.f) + dt;
}

// ---- ScaledPatchSampler (data/pixel_samplers.py:618-742): patch centres -> ray indices + ground-truth RGB patches ------
// One workgroup per patch.  The centre is either handed over (the sampling-weights branch draws it with
// torch.multinomial and clips it, :728-742) or derived from the three uniform draws of PixelSampler.sample_method
// (:100-103): (u * float(dim)).long() over (n_images, H - K + 1, W - K + 1), then + K/2 on the pixel axes (:722-726).
// Integer work downstream of that one fp32 product; the image gather is a row-wise copy, K*C contiguous elements per row.
template <typename Pix>
__global__ __launch_bounds__(256) void patch_sample_kernel(const float* __restrict__ uniforms,
                                                           const int64_t* __restrict__ centers, int n_images, int H, int W,
                                                           int C, int Kf, int sc, const int64_t* __restrict__ image_idx,
                                                           const Pix* __restrict__ images, int64_t* __restrict__ ray_indices,
                                                           float* __restrict__ coords, Pix* __restrict__ patches) {
#pragma clang fp contract(off)
  const int64_t p = blockIdx.x;
  const int K = Kf * sc, half = K / 2;
  int64_t c, cy, cx;
  if (centers) {
    c = centers[3 * p], cy = centers[3 * p + 1], cx = centers[3 * p + 2];
  } else {
    c = (int64_t)(uniforms[3 * p] * (float)n_images);
    cy = (int64_t)(uniforms[3 * p + 1] * (float)(H - K + 1)) + half;
    cx = (int64_t)(uniforms[3 * p + 2] * (float)(W - K + 1)) + half;
  }
  const int64_t y0 = cy - half, x0 = cx - half;  // offsets = arange(-(K//2), K//2 + K%2)  (:703)
  const int64_t global_c = image_idx ? image_idx[min(max(c, (int64_t)0), (int64_t)n_images - 1)] : c;
  for (int r = threadIdx.x; r < Kf * Kf; r += 256) {  // ray_indices = rgb_indices[:, sc//2::sc, sc//2::sc]  (:709-712)
    const int64_t y = y0 + sc / 2 + (r / Kf) * sc, x = x0 + sc / 2 + (r % Kf) * sc;
    int64_t* o = ray_indices + 3 * (p * Kf * Kf + r);
    o[0] = global_c, o[1] = y, o[2] = x;
    if (coords) {  // RayGenerator.forward's image_coords[y, x] = pixel centres (ray_generators.py:49, cameras.py:get_image_coords)
      coords[2 * (p * Kf * Kf + r)] = (float)y + 0.5f;
      coords[2 * (p * Kf * Kf + r) + 1] = (float)x + 0.5f;
    }
  }
  if (!patches) return;
  // reads are clamped into the image: a centre the caller placed too close to the border must not fault (the reference's
  // advanced indexing would raise / wrap there)
  const int64_t cc = min(max(c, (int64_t)0), (int64_t)n_images - 1);
  const int row_len = K * C;
  Pix* dst = patches + p * (int64_t)K * row_len;
  for (int e = threadIdx.x; e < K * row_len; e += 256) {
    const int r = e / row_len, q = e - r * row_len;
    const int64_t y = min(max(y0 + r, (int64_t)0), (int64_t)H - 1);
    const int64_t x = min(max(x0 + q / C, (int64_t)0), (int64_t)W - 1);
    dst[e] = images[((cc * H + y) * W + x) * C + q % C];
  }
}

// ---- LidarPointSampler.collate_image_dataset_batch (data/pixel_samplers.py:538-583), packed point clouds ----------------
// Output row r belongs to scan l = shuffle[r / rays_per_lidar] and takes its point floor(draw[l, r % rays_per_lidar] *
// points_per_lidar[l]) (fp64 product, as torch computes it): one thread per row copies the point and writes the
// (lidar_idx[l], point) index pair.  The exclusive prefix sum of the scan sizes (:549-551) is rebuilt per workgroup in LDS.
constexpr int kMaxScans = 2048;

__global__ __launch_bounds__(256) void lidar_point_sample_kernel(const int64_t* __restrict__ shuffle,
                                                                 const double* __restrict__ draws,
                                                                 const int64_t* __restrict__ points_per_lidar,
                                                                 const int64_t* __restrict__ lidar_idx,
                                                                 const float* __restrict__ lidar, int n_lidars,
                                                                 int rays_per_lidar, int D, int64_t n_rays,
                                                                 int64_t* __restrict__ indices, float* __restrict__ points) {
#pragma clang fp contract(off)
  __shared__ int64_t first_point[kMaxScans];
  if (threadIdx.x < 64) {  // one wave: chunked serial scan, n_lidars is tens to hundreds
    int64_t run = 0;
    for (int base = 0; base < n_lidars; base += 64) {
      const int i = base + threadIdx.x;
      int64_t v = i < n_lidars ? points_per_lidar[i] : 0, incl = v;
      for (int d = 1; d < 64; d <<= 1) {
        const int64_t up = __shfl_up(incl, d, 64);
        if ((int)threadIdx.x >= d) incl += up;
      }
      if (i < n_lidars) first_point[i] = run + incl - v;
      run += __shfl(incl, 63, 64);
    }
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  const int64_t l = shuffle[r / rays_per_lidar];
  const int64_t k = r % rays_per_lidar;
  const int64_t p = (int64_t)floor(draws[l * rays_per_lidar + k] * (double)points_per_lidar[l]);
  indices[2 * r] = lidar_idx ? lidar_idx[l] : l;
  indices[2 * r + 1] = p;
  const float* src = lidar + (first_point[l] + p) * D;
  for (int d = 0; d < D; ++d) points[r * D + d] = src[d];
}

}  // namespace nrhip

using namespace nrhip;

// the checks both camera entry points make before a launch; 0 or the error code
static int check_camera_args(const char* who, const nrhip_camera_table* cams, const int64_t* camera_indices,
                             const float* coords, float* origins, float* directions, float* pixel_area,
                             float* directions_norm, float* times) {
  NR_REQUIRE(cams->camera_to_worlds && cams->fx && cams->fy && cams->cx && cams->cy && camera_indices && coords && origins &&
                 directions && pixel_area && directions_norm,
             NRHIP_ERR_INVALID_ARG, "%s: NULL pointer", who);
  NR_REQUIRE(cams->rolling_shutter >= 0 && cams->rolling_shutter <= 3, NRHIP_ERR_INVALID_ARG, "%s: rolling_shutter mode", who);
  NR_REQUIRE(cams->rolling_shutter == 0 || (cams->rolling_shutter_time && cams->time_to_center_pixel && cams->velocities &&
                                            cams->shutter_extent && cams->times && times),
             NRHIP_ERR_INVALID_ARG, "%s: rolling shutter needs duration, time_to_center_pixel, velocities, extent, times", who);
  return NRHIP_OK;
}

static CameraTable camera_table(const nrhip_camera_table* cams) {
  return {cams->camera_to_worlds, cams->fx, cams->fy, cams->cx, cams->cy, cams->times, cams->rolling_shutter_time,
          cams->time_to_center_pixel, cams->velocities, cams->shutter_extent, cams->rolling_shutter};
}

extern "C" int nrhip_camera_rays(const nrhip_camera_table* cams, const int64_t* camera_indices, const float* coords,
                                 int64_t n_rays, float* origins, float* directions, float* pixel_area,
                                 float* directions_norm, float* times, void* stream) {
  NR_REQUIRE(cams && n_rays >= 0, NRHIP_ERR_INVALID_ARG, "camera_rays: bad argument");
  if (n_rays == 0) return NRHIP_OK;
  if (int rc = check_camera_args("camera_rays", cams, camera_indices, coords, origins, directions, pixel_area,
                                 directions_norm, times))
    return rc;
  camera_rays_kernel<<<grid_for(n_rays, 256), 256, 0, (hipStream_t)stream>>>(
      camera_table(cams), camera_indices, coords, n_rays, origins, directions, pixel_area, directions_norm, times);
  return check_launch("camera_rays");
}

extern "C" int nrhip_camera_rays_lens(const nrhip_camera_table* cams, const nrhip_camera_lens* lens,
                                      const int64_t* camera_indices, const float* coords, int64_t n_rays, float* origins,
                                      float* directions, float* pixel_area, float* directions_norm, float* times,
                                      void* stream) {
  NR_REQUIRE(cams && lens, NRHIP_ERR_INVALID_ARG, "camera_rays_lens: NULL camera table or lens");
  NR_REQUIRE(n_rays >= 0, NRHIP_ERR_INVALID_ARG, "camera_rays_lens: negative n_rays");
  NR_REQUIRE(lens->camera_type == kPerspective || lens->camera_type == kFisheye, NRHIP_ERR_UNSUPPORTED,
             "camera_rays_lens: camera type %d (1 PERSPECTIVE and 2 FISHEYE are covered)", (int)lens->camera_type);
  if (n_rays == 0) return NRHIP_OK;
  if (int rc = check_camera_args("camera_rays_lens", cams, camera_indices, coords, origins, directions, pixel_area,
                                 directions_norm, times))
    return rc;
  const auto kernel = lens->camera_type == kFisheye ? camera_rays_lens_kernel<kFisheye> : camera_rays_lens_kernel<kPerspective>;
  kernel<<<grid_for(n_rays, 256), 256, 0, (hipStream_t)stream>>>(camera_table(cams), lens->distortion, camera_indices, coords,
                                                                 n_rays, origins, directions, pixel_area, directions_norm,
                                                                 times);
  return check_launch("camera_rays_lens");
}

extern "C" int nrhip_lidar_rays(const nrhip_lidar_table* lidars, const int64_t* lidar_indices, const float* points,
                                int32_t point_dim, int64_t n_rays, float* origins, float* directions, float* pixel_area,
                                float* distance, uint8_t* did_return, float* times, void* stream) {
  NR_REQUIRE(lidars && n_rays >= 0 && point_dim >= 3, NRHIP_ERR_INVALID_ARG, "lidar_rays: bad argument");
  if (n_rays == 0) return NRHIP_OK;
  NR_REQUIRE(lidars->lidar_to_worlds && lidars->horizontal_beam_divergence && lidars->vertical_beam_divergence &&
                 lidar_indices && points && origins && directions && pixel_area && distance && did_return,
             NRHIP_ERR_INVALID_ARG, "lidar_rays: NULL pointer");
  LidarTable t{lidars->lidar_to_worlds, lidars->times, lidars->velocities, lidars->horizontal_beam_divergence,
               lidars->vertical_beam_divergence, lidars->assume_ego_compensated, lidars->valid_lidar_distance_threshold};
  lidar_rays_kernel<<<grid_for(n_rays, 256), 256, 0, (hipStream_t)stream>>>(t, lidar_indices, points, point_dim, n_rays,
                                                                           origins, directions, pixel_area, distance,
                                                                           did_return, times);
  return check_launch("lidar_rays");
}

extern "C" int nrhip_patch_sample(const float* uniforms, const int64_t* centers, int64_t n_patches, int32_t n_images,
                                  int32_t height, int32_t width, int32_t channels, int32_t patch_size, int32_t patch_scale,
                                  const int64_t* image_idx, const void* images, int32_t image_dtype, int64_t* ray_indices,
                                  float* coords, void* patches, void* stream) {
  NR_REQUIRE(n_patches >= 0 && n_images > 0 && channels > 0 && patch_size > 0 && patch_scale > 0, NRHIP_ERR_INVALID_ARG,
             "patch_sample: bad argument");
  const int64_t K = (int64_t)patch_size * patch_scale;
  NR_REQUIRE(K <= height && K <= width, NRHIP_ERR_INVALID_ARG, "patch_sample: the rgb patch (patch_size * patch_scale) exceeds the image");
  NR_REQUIRE(image_dtype == 0 || image_dtype == 1, NRHIP_ERR_UNSUPPORTED, "patch_sample: image_dtype 0 (fp32) or 1 (uint8)");
  if (n_patches == 0) return NRHIP_OK;
  NR_REQUIRE((uniforms != nullptr) != (centers != nullptr), NRHIP_ERR_INVALID_ARG,
             "patch_sample: exactly one of uniforms / centers");
  NR_REQUIRE(ray_indices && (!patches || images), NRHIP_ERR_INVALID_ARG, "patch_sample: NULL pointer");
  NR_REQUIRE(n_patches <= 0x7fffffff, NRHIP_ERR_INVALID_ARG, "patch_sample: too many patches for one launch");
  if (image_dtype == 0)
    patch_sample_kernel<float><<<(int)n_patches, 256, 0, (hipStream_t)stream>>>(
        uniforms, centers, n_images, height, width, channels, patch_size, patch_scale, image_idx, (const float*)images,
        ray_indices, coords, (float*)patches);
  else
    patch_sample_kernel<uint8_t><<<(int)n_patches, 256, 0, (hipStream_t)stream>>>(
        uniforms, centers, n_images, height, width, channels, patch_size, patch_scale, image_idx, (const uint8_t*)images,
        ray_indices, coords, (uint8_t*)patches);
  return check_launch("patch_sample");
}

extern "C" int nrhip_lidar_point_sample(const int64_t* shuffle, const double* draws, const int64_t* points_per_lidar,
                                        const int64_t* lidar_idx, const float* lidar, int32_t n_lidars,
                                        int32_t rays_per_lidar, int32_t point_dim, int64_t n_rays, int64_t* indices,
                                        float* points, void* stream) {
  NR_REQUIRE(n_rays >= 0 && n_lidars > 0 && rays_per_lidar > 0 && point_dim > 0, NRHIP_ERR_INVALID_ARG,
             "lidar_point_sample: bad argument");
  NR_REQUIRE(n_lidars <= kMaxScans, NRHIP_ERR_UNSUPPORTED, "lidar_point_sample: at most 2048 scans per batch");
  NR_REQUIRE(n_rays <= (int64_t)n_lidars * rays_per_lidar, NRHIP_ERR_INVALID_ARG,
             "lidar_point_sample: n_rays exceeds n_lidars * rays_per_lidar draws");
  if (n_rays == 0) return NRHIP_OK;
  NR_REQUIRE(shuffle && draws && points_per_lidar && lidar && indices && points, NRHIP_ERR_INVALID_ARG,
             "lidar_point_sample: NULL pointer");
  lidar_point_sample_kernel<<<grid_for(n_rays, 256), 256, 0, (hipStream_t)stream>>>(
      shuffle, draws, points_per_lidar, lidar_idx, lidar, n_lidars, rays_per_lidar, point_dim, n_rays, indices, points);
  return check_launch("lidar_point_sample");
}
