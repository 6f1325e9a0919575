// Generalisation training: the batch of one item made on the device from the device-resident DTU training set
// (surf_amd/datasets/dtu_resident.py; the reference decodes five PNGs, two mask PNGs, four PFMs and a PLY on the host for every
// item and uploads a 25.9 MB dictionary at 480 x 640: datasets/dtu.py:85-471).  The cache holds what the files hold after the
// nearest-neighbour pick - uint8 texels and masks, fp32 depths, unscaled - and these two kernels write the fp32 entries of the
// dictionary from it.
//
//  * train_views_kernel: the per-view planes of one item in one launch.  blockIdx.y < n_views: imgs[v] (3, H, W) fp32 from the
//    uint8 (H, W, 3) image in slot v, an HWC -> CHW transposition with imgs = (float)texel * (1 / 256) (exact: a power of two).
//    blockIdx.y = n_views + j, j in {0, 1} (the reference view and the supervised source view): mask_out[j] = (float)mask,
//    depth_out[j] = scaled(depth), pseudo_out[j] = scaled(pseudo depth) with
//        scaled(d) = (float)((double)d * scale)         (one fp64 product, one round-to-nearest conversion)
//    which is how the reader's `fp32 array * np.float64 scalar` followed by the cast to fp32 rounds.  One thread per four
//    consecutive pixels of a plane (flat index: no assumption on W): 12 bytes = three dwords read, one 16-byte store per plane;
//    the H W % 4 pixels of the last group go one at a time.  Image and mask pointers are 4-byte aligned (SURF_E_ARG otherwise);
//    the 16-byte accesses are written on packed types, so a plane that starts off a 16-byte boundary (H W % 4 != 0) is fine.
//    The image pointers travel in a by-value argument struct, SURF_MAX_VIEWS of them.
//  * train_rays_kernel: the ray block, one thread per ray, the n_masked = n_rays - n_rays / 4 pixels drawn inside the reference
//    mask first (choose_pixels' order).  Ray t < n_masked: i = pick[t], flat = inside[i] (the row-major list of pixels with
//    mask > 0.5), x = flat % w, y = flat / w; otherwise x = free_x[t - n_masked], y = free_y[t - n_masked].  px = (float)x,
//    py = (float)y (exact below 2^24).  The library is compiled with -ffp-contract=off; every line below is one fp32 operation
//    per operator, evaluated left to right as parenthesised - the sequence of finetune_rays.hip (Ki = the reference view's
//    inverse(K)[:3,:3] row-major, computed on the host in fp32; c = its c2w[:3,:4] row-major):
//        dx = (Ki[0]*px + Ki[1]*py) + Ki[2]          dy, dz likewise with Ki[3..5], Ki[6..8]     (the homogeneous 1: x * 1 = x)
//        n  = sqrt((dx*dx + dy*dy) + dz*dz)          (IEEE fp32 square root)
//        dx = dx / n;  dy = dy / n;  dz = dz / n      (IEEE fp32 division)
//        rays_d[0] = (c[0]*dx + c[1]*dy) + c[2]*dz    rays_d[1], rays_d[2] likewise with c[4..6], c[8..10]
//        rays_o    = (c[3], c[7], c[11])
//        color = image[y][x][0..2] * (1 / 256), depth = scaled(depth[y][x]), pseudo_depth = scaled(pseudo[y][x]),
//        mask = (float)mask[y][x]
//    A pixel outside the image (a free pixel, or an inside-list entry outside [0, h w)) keeps its coordinates and rays and
//    yields zeros for color / depth / pseudo_depth / mask, as finetune_rays.hip does; a pick outside [0, n_inside) has no pixel:
//    every output of that ray is zero.  tests/test_train_resident_gpu.py mirrors exactly this sequence in numpy fp32.
// Bandwidth-trivial: 7.4 MB written per item at 5 x 480 x 640, 512 rays.  What it buys is the 25.9 MB upload and the 0.4 s of
// host decoding that no longer happen every step, not its own speed.  No LDS, 256-thread blocks for the planes, 64 for the rays.
#include <math.h>

#include "common.h"

namespace {

struct TrainViewsArgs {
  const uint8_t* image[SURF_MAX_VIEWS];
  const uint8_t* mask[2];
  const float* depth[2];
  const float* pseudo[2];
};

struct __attribute__((packed, aligned(4))) U3u { uint32_t a, b, c; };       // 12 / 16 bytes at a 4-byte aligned address
struct __attribute__((packed, aligned(4))) F4u { float x, y, z, w; };

__device__ __forceinline__ float scaled(float d, double scale) { return (float)((double)d * scale); }

__global__ __launch_bounds__(256) void train_views_kernel(TrainViewsArgs a, int n_views, int64_t hw, double scale,
                                                          float* __restrict__ imgs, float* __restrict__ mask_out,
                                                          float* __restrict__ depth_out, float* __restrict__ pseudo_out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // group of four pixels
  const int64_t p0 = g * 4;
  if (p0 >= hw) return;
  const bool full = p0 + 4 <= hw;
  const int job = blockIdx.y;
  const float inv256 = 0.00390625f;
  if (job < n_views) {
    const uint8_t* __restrict__ src = a.image[job];
    float* __restrict__ dst = imgs + (int64_t)job * 3 * hw;
    if (full) {
      const U3u t = *reinterpret_cast<const U3u*>(src + p0 * 3);          // bytes 3 p + c of pixels p0 .. p0 + 3
      const uint32_t b[12] = {t.a & 255u, (t.a >> 8) & 255u, (t.a >> 16) & 255u, t.a >> 24, t.b & 255u, (t.b >> 8) & 255u,
                              (t.b >> 16) & 255u, t.b >> 24, t.c & 255u, (t.c >> 8) & 255u, (t.c >> 16) & 255u, t.c >> 24};
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<F4u*>(dst + c * hw + p0) = F4u{(float)b[c] * inv256, (float)b[3 + c] * inv256, (float)b[6 + c] * inv256,
                                                         (float)b[9 + c] * inv256};
    } else {
      for (int64_t p = p0; p < hw; ++p)
        for (int c = 0; c < 3; ++c) dst[c * hw + p] = (float)src[p * 3 + c] * inv256;
    }
    return;
  }
  const int j = job - n_views;                                             // 0: the reference view, 1: the source view
  const uint8_t* __restrict__ m = a.mask[j];
  const float* __restrict__ d = a.depth[j];
  const float* __restrict__ q = a.pseudo[j];
  const int64_t o = (int64_t)j * hw + p0;
  if (full) {
    const uint32_t mb = *reinterpret_cast<const uint32_t*>(m + p0);
    const F4u dv = *reinterpret_cast<const F4u*>(d + p0);
    const F4u qv = *reinterpret_cast<const F4u*>(q + p0);
    *reinterpret_cast<F4u*>(mask_out + o) = F4u{(float)(mb & 255u), (float)((mb >> 8) & 255u), (float)((mb >> 16) & 255u),
                                                (float)(mb >> 24)};
    *reinterpret_cast<F4u*>(depth_out + o) = F4u{scaled(dv.x, scale), scaled(dv.y, scale), scaled(dv.z, scale), scaled(dv.w, scale)};
    *reinterpret_cast<F4u*>(pseudo_out + o) = F4u{scaled(qv.x, scale), scaled(qv.y, scale), scaled(qv.z, scale), scaled(qv.w, scale)};
  } else {
    for (int64_t p = p0; p < hw; ++p) {
      mask_out[(int64_t)j * hw + p] = (float)m[p];
      depth_out[(int64_t)j * hw + p] = scaled(d[p], scale);
      pseudo_out[(int64_t)j * hw + p] = scaled(q[p], scale);
    }
  }
}

struct TrainRaysCam {
  float kinv[9];
  float c2w[12];
};

__global__ __launch_bounds__(64) void train_rays_kernel(const int32_t* __restrict__ pick, const int32_t* __restrict__ free_x,
                                                        const int32_t* __restrict__ free_y, int n_rays, int n_masked,
                                                        const int32_t* __restrict__ inside, int64_t n_inside, TrainRaysCam cam,
                                                        const uint8_t* __restrict__ image, const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ depth, const float* __restrict__ pseudo,
                                                        double scale, int h, int w, float* __restrict__ pixels_x,
                                                        float* __restrict__ pixels_y, float* __restrict__ rays_o,
                                                        float* __restrict__ rays_d, float* __restrict__ color,
                                                        float* __restrict__ depth_out, float* __restrict__ pseudo_out,
                                                        float* __restrict__ mask_out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rays) return;
  int64_t x, y;
  bool have = true;                                                         // the ray has a pixel at all
  if (t < n_masked) {
    const int64_t i = pick[t];
    have = i >= 0 && i < n_inside;
    const int64_t flat = have ? (int64_t)inside[i] : 0;
    const bool in_list = flat >= 0;                                         // a negative entry: off the image, truncating division
    x = in_list ? flat % w : -1;
    y = in_list ? flat / w : -1;
  } else {
    x = free_x[t - n_masked];
    y = free_y[t - n_masked];
  }
  const float px = (float)x, py = (float)y;
  float dx = (cam.kinv[0] * px + cam.kinv[1] * py) + cam.kinv[2];
  float dy = (cam.kinv[3] * px + cam.kinv[4] * py) + cam.kinv[5];
  float dz = (cam.kinv[6] * px + cam.kinv[7] * py) + cam.kinv[8];
  const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz);
  dx = dx / nrm;
  dy = dy / nrm;
  dz = dz / nrm;
  pixels_x[t] = have ? px : 0.0f;
  pixels_y[t] = have ? py : 0.0f;
  rays_d[t * 3 + 0] = have ? (cam.c2w[0] * dx + cam.c2w[1] * dy) + cam.c2w[2] * dz : 0.0f;
  rays_d[t * 3 + 1] = have ? (cam.c2w[4] * dx + cam.c2w[5] * dy) + cam.c2w[6] * dz : 0.0f;
  rays_d[t * 3 + 2] = have ? (cam.c2w[8] * dx + cam.c2w[9] * dy) + cam.c2w[10] * dz : 0.0f;
  rays_o[t * 3 + 0] = have ? cam.c2w[3] : 0.0f;
  rays_o[t * 3 + 1] = have ? cam.c2w[7] : 0.0f;
  rays_o[t * 3 + 2] = have ? cam.c2w[11] : 0.0f;
  const bool in_image = have && x >= 0 && x < w && y >= 0 && y < h;
  const int64_t at = in_image ? y * w + x : 0;
  const float inv256 = 0.00390625f;
  color[t * 3 + 0] = in_image ? (float)image[at * 3 + 0] * inv256 : 0.0f;
  color[t * 3 + 1] = in_image ? (float)image[at * 3 + 1] * inv256 : 0.0f;
  color[t * 3 + 2] = in_image ? (float)image[at * 3 + 2] * inv256 : 0.0f;
  depth_out[t] = in_image ? scaled(depth[at], scale) : 0.0f;
  pseudo_out[t] = in_image ? scaled(pseudo[at], scale) : 0.0f;
  mask_out[t] = in_image ? (float)mask[at] : 0.0f;
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace

extern "C" int surf_train_views(const uint8_t* const* h_images, int n_views, int h, int w, const uint8_t* const* h_masks,
                                const float* const* h_depths, const float* const* h_pseudos, double scale, float* imgs,
                                float* mask_out, float* depth_out, float* pseudo_out, void* stream) {
  if (!h_images || !h_masks || !h_depths || !h_pseudos || !imgs || !mask_out || !depth_out || !pseudo_out || n_views <= 0 ||
      h <= 0 || w <= 0)
    return SURF_E_ARG;
  if (n_views > SURF_MAX_VIEWS || h > (1 << 20) || w > (1 << 20) || (int64_t)h * w >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  TrainViewsArgs a = {};
  for (int v = 0; v < n_views; ++v) {
    if (!h_images[v] || !aligned4(h_images[v])) return SURF_E_ARG;
    a.image[v] = h_images[v];
  }
  for (int j = 0; j < 2; ++j) {
    if (!h_masks[j] || !h_depths[j] || !h_pseudos[j] || !aligned4(h_masks[j]) || !aligned4(h_depths[j]) || !aligned4(h_pseudos[j]))
      return SURF_E_ARG;
    a.mask[j] = h_masks[j];
    a.depth[j] = h_depths[j];
    a.pseudo[j] = h_pseudos[j];
  }
  if (!aligned4(imgs) || !aligned4(mask_out) || !aligned4(depth_out) || !aligned4(pseudo_out)) return SURF_E_ARG;
  const int64_t hw = (int64_t)h * w;
  const unsigned blocks = (unsigned)(((hw + 3) / 4 + 255) / 256);
  hipLaunchKernelGGL(train_views_kernel, dim3(blocks, (unsigned)n_views + 2), dim3(256), 0, (hipStream_t)stream, a, n_views, hw,
                     scale, imgs, mask_out, depth_out, pseudo_out);
  return surf_check_launch();
}

extern "C" int surf_train_rays(const int32_t* pick, const int32_t* free_x, const int32_t* free_y, int n_rays, const int32_t* inside,
                               int64_t n_inside, const float* h_kinv, const float* h_c2w, const uint8_t* image, const uint8_t* mask,
                               const float* depth, const float* pseudo, double scale, int h, int w, float* pixels_x,
                               float* pixels_y, float* rays_o, float* rays_d, float* color, float* depth_out, float* pseudo_out,
                               float* mask_out, void* stream) {
  if (!inside || !h_kinv || !h_c2w || !image || !mask || !depth || !pseudo || !pixels_x || !pixels_y || !rays_o || !rays_d || !color ||
      !depth_out || !pseudo_out || !mask_out || n_rays <= 0 || n_inside <= 0 || h <= 0 || w <= 0)
    return SURF_E_ARG;
  const int n_free = n_rays / 4, n_masked = n_rays - n_free;
  if (!pick || (n_free > 0 && (!free_x || !free_y))) return SURF_E_ARG;
  if (n_rays > (1 << 24) || h > (1 << 20) || w > (1 << 20) || (int64_t)h * w >= ((int64_t)1 << 31) || n_inside > (int64_t)h * w)
    return SURF_E_LIMIT;
  TrainRaysCam cam;
  for (int i = 0; i < 9; ++i) cam.kinv[i] = h_kinv[i];
  for (int i = 0; i < 12; ++i) cam.c2w[i] = h_c2w[i];
  hipLaunchKernelGGL(train_rays_kernel, dim3((unsigned)((n_rays + 63) / 64)), dim3(64), 0, (hipStream_t)stream, pick, free_x, free_y,
                     n_rays, n_masked, inside, n_inside, cam, image, mask, depth, pseudo, scale, h, w, pixels_x, pixels_y, rays_o,
                     rays_d, color, depth_out, pseudo_out, mask_out);
  return surf_check_launch();
}
