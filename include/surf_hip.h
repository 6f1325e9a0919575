/*
 * surf_hip.h -- C ABI of the MI355X (gfx950) kernels behind the SuRF volume-rendering hot path.
 *
 * The reference (prstrive/SuRF) has no FFI: its "operator API" is the Python class
 * models/surf.py:15 `SuRF(nn.Module)`.  These entry points are what a binding for that path
 * would call instead of the PyTorch ops listed beside each one (file:line into the reference).
 * INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every `d_` / unprefixed data pointer is a DEVICE pointer owned by the caller; the library
 *     never allocates, frees or synchronises.  `h_` pointers are small HOST arrays read at launch.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).
 *   - return value: 0 ok, <0 invalid argument (SURF_E_*), >0 a hipError_t from the launch.
 *   - all floating point is fp32; index tables are int32 (the reference's int64 tables are
 *     converted by the host wrapper), -1 = empty voxel.
 *
 * Layouts
 *   - dense volumes (matching logits, index tables): [x][y][z], z fastest (volume.py:99-132).
 *   - sparse feature volumes: rows of 8 floats = 7 channels + 1 pad (surf.py:119 `out_feats[:,1:]`).
 *   - image / feature maps: NHWC with 4 floats per texel ("texel4"): (nv, H, W, 4).
 *   - per-sample arrays are ray-major: index = ray * S + sample.
 */
#ifndef SURF_HIP_H
#define SURF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SURF_MAX_VIEWS 8
#define SURF_MAX_STAGES 4
#define SURF_MAX_SAMPLES 256

#define SURF_E_ARG (-1)      /* null pointer / bad size */
#define SURF_E_LIMIT (-2)    /* exceeds SURF_MAX_* */

/* ABI version, bumped whenever a signature below changes.  Defined here once: surf_abi_version() returns it and the
 * host binding (surf_amd/_lib.py, which reads it from this line) refuses a library that reports a different number. */
#define SURF_ABI_VERSION 41
int surf_abi_version(void);

/* Repack NCHW fp32 (n, C<=4, H, W) into texel4 NHWC (n, H, W, 4), zero padding channels >= C. */
int surf_pack_texel4(const float* src, int n, int C, int H, int W, float* dst, void* stream);

/*
 * Ray set-up: z-sampling guided by the matching volume + section mid-points + voxel mask.
 * Replaces ImplicitSurface.render's sampling block (implicit_surface.py:268-311),
 * the head of render_core (implicit_surface.py:72-86) and lookup_volume (projector.py:392-420).
 *   rays_o, rays_d (R,3); near, far (R)
 *   mvol        dense matching volume (Dm^3)
 *   lin_depth   device copy of torch.linspace(0,1,n_depth); lin_samples: the n_stage linspaces
 *               torch.linspace(0,1,n_samples[s]) concatenated (S floats)
 *   h_n_samples[n_stage], h_sample_ranges[n_stage]   (confs/surf.conf:118-119)
 *   jitter      NULL (render.perturb = 0) or device (R, n_stage): the per-ray, per-stage `torch.rand([R,1]) - 0.5`
 *               draws of render.perturb > 0 (implicit_surface.py:274-277, 304-306)
 *   tables[n_stage] (fine -> coarse, as surf.py:159 passes them), h_dims[n_stage]
 * outputs (any of z_vals may be NULL): z_vals, mid_z, dists (R,S); pts (R*S,3); vmask (R*S) uint8
 */
int surf_ray_setup(const float* rays_o, const float* rays_d, const float* near, const float* far, int n_rays,
                   const float* mvol, int Dm, const float* lin_depth, int n_depth, const float* lin_samples,
                   const int* h_n_samples, const float* h_sample_ranges, int n_stage, const float* jitter,
                   float sample_dist, const int32_t* const* h_tables, const int* h_dims, int n_vol,
                   float* z_vals, float* mid_z, float* dists, float* pts, uint8_t* vmask, void* stream);

/*
 * Size in floats of the packed SDF-MLP weight buffer, and the packer.
 * Replaces the weight_norm re-parameterisation + layer loop of SDFNetworkSparse
 * (sdf_network.py:28-121) for the shipped architecture (d_hidden 128, 6 hidden layers,
 * skip_in [3], multires 4, 28 feature channels, scale 1).  `h_W[l]`/`h_b[l]` are HOST pointers to
 * the EFFECTIVE (weight-normed) row-major matrices lin0..lin6 and biases.
 */
int64_t surf_sdf_packed_floats(void);
int surf_sdf_pack_weights(const float* const* h_W, const float* const* h_b, float* h_packed);

/* Bytes of scratch the SDF kernel needs for a launch of n points (gradient variant only). */
int64_t surf_sdf_scratch_bytes(int64_t n_points);

/*
 * SDF MLP forward (+ analytic gradient) at n points with sparse trilinear feature gather.
 * Replaces lookup_sparse_volume/grid_sample_3d_sparse (projector.py:217-390),
 * SDFNetworkSparse.forward/sdf (sdf_network.py:95-124) and the first-order part of
 * SDFNetworkSparse.gradient (sdf_network.py:129-141).
 *   pts (.,3); mask (.) uint8 or NULL (NULL = all points active)
 *   idx: NULL -> points 0..n-1 are evaluated; else the n point indices to evaluate (e.g. surf_compact of the mask):
 *        inputs are gathered and outputs scattered through idx, so wavefront tiles hold active points only
 *   h_vols[n_vol]: (N_s,8) rows; h_tables[n_vol]: (D_s^3) int32; fine -> coarse
 *   packed: device copy of surf_sdf_pack_weights output
 *   sdf (n); grad (n,3) or NULL (forward only); scratch: >= surf_sdf_scratch_bytes(n) or NULL if grad NULL
 * Points with mask 0 are not written.
 */
int surf_sdf_mlp(const float* pts, const uint8_t* mask, const int32_t* idx, int64_t n, const float* const* h_vols,
                 const int32_t* const* h_tables, const int* h_dims, int n_vol, const float* packed,
                 float* sdf, float* grad, void* scratch, void* stream);

/*
 * The same evaluation on the 16-bit matrix pipes with fp32 accumulation (surf_amd/csrc/sdf_mlp_split.hip).  Arguments
 * as surf_sdf_mlp; `packed` is the output of the matching surf_sdf_pack_weights_* (…_packed_bytes() bytes, device copy),
 * `scratch` >= …_scratch_bytes(n): the launch's round counter (256 bytes; the gradient kernel deals its rounds of 128 samples
 * to the workgroups on demand), then the per-wavefront slots of the exponent slices and the feature Jacobian.  Contents need
 * not be preserved between launches: the entry points zero the counter on the launch stream themselves.  Counter and slots
 * belong to ONE gradient launch at a time: two gradient launches that may run concurrently (different streams) need two buffers.
 *   bf16x3: every fp32 operand is split exactly into three bf16 pieces and six partial products are accumulated
 *           (dropped terms <= 2^-23 per product): fp32-equivalent results.  The packed image is opaque: the kernel works in
 *           units of the softplus exponent (biases and input columns x 100 log2 e, lin6's row 0 x ln 2 / 100, hidden matrices
 *           as they are), so an image is only meaningful to the kernel of the same library build.
 *   f16x2:  two fp16 pieces per operand, three partial products (the product of the two second pieces is dropped).  The
 *           second piece is the fp16 of the fp32 residual v - fp16(v), at the operand's own scale: weights (and the reverse
 *           sweep's deltas) are stored x 2^8 as a whole, activations unscaled.  Operand error <= 2^-22 relative while the
 *           second piece is a normal fp16 number, <= 2^-25 absolute (2^-33 for the x 2^8 operands) below that; activations
 *           must stay below 65504 in magnitude, weights below 65504 / 2^8.  The fast path.
 */
int64_t surf_sdf_bf16_packed_bytes(void);
int64_t surf_sdf_bf16_scratch_bytes(int64_t n_points);
int surf_sdf_pack_weights_bf16(const float* const* h_W, const float* const* h_b, unsigned char* h_packed);
int surf_sdf_mlp_bf16x3(const float* pts, const uint8_t* mask, const int32_t* idx, int64_t n, const float* const* h_vols,
                        const int32_t* const* h_tables, const int* h_dims, int n_vol, const void* packed, float* sdf,
                        float* grad, void* scratch, void* stream);
int64_t surf_sdf_f16_packed_bytes(void);
int64_t surf_sdf_f16_scratch_bytes(int64_t n_points);
int surf_sdf_pack_weights_f16(const float* const* h_W, const float* const* h_b, unsigned char* h_packed);
int surf_sdf_mlp_f16x2(const float* pts, const uint8_t* mask, const int32_t* idx, int64_t n, const float* const* h_vols,
                       const int32_t* const* h_tables, const int* h_dims, int n_vol, const void* packed, float* sdf,
                       float* grad, void* scratch, void* stream);

/* Both split kernels with the number of `idx` entries read from DEVICE memory (d_n[0] <= n_capacity = entries allocated for idx):
 * the launch that follows surf_compact needs no host round trip for the count ("replaced by device-side counters").
 * Grid and scratch are sized by the capacity; rows beyond d_n[0] are not touched. */
int surf_sdf_mlp_bf16x3_dn(const float* pts, const int32_t* idx, int64_t n_capacity, const int32_t* d_n, const float* const* h_vols,
                           const int32_t* const* h_tables, const int* h_dims, int n_vol, const void* packed, float* sdf,
                           float* grad, void* scratch, void* stream);
int surf_sdf_mlp_f16x2_dn(const float* pts, const int32_t* idx, int64_t n_capacity, const int32_t* d_n, const float* const* h_vols,
                          const int32_t* const* h_tables, const int* h_dims, int n_vol, const void* packed, float* sdf,
                          float* grad, void* scratch, void* stream);

/* The SDF on a lattice WITHOUT point tensors (extract_geometry, models/modules/implicit_surface.py:337-351, replaces its
 * meshgrid + cat of points): out[(ix ny + iy) nz + iz] = sign * sdf(ax[ix], ay[iy], az[iz]) by the forward-only split kernels;
 * ax / ay / az: device arrays of nx / ny / nz coordinates (torch.linspace's values, :338-340), sign = -1 gives marching cubes'
 * input u directly (:350).  nx ny nz < 2^31 per call (the caller walks slabs of x). */
int surf_sdf_lattice_bf16x3(const float* ax, const float* ay, const float* az, int nx, int ny, int nz, const float* const* h_vols,
                            const int32_t* const* h_tables, const int* h_dims, int n_vol, const void* packed, float* out,
                            float sign, void* stream);
int surf_sdf_lattice_f16x2(const float* ax, const float* ay, const float* az, int nx, int ny, int nz, const float* const* h_vols,
                           const int32_t* const* h_tables, const int* h_dims, int n_vol, const void* packed, float* out,
                           float sign, void* stream);

/* The same on the bricks of the narrow band (surf_band_*): out[j * 512 + (lx << 6 | ly << 3 | lz)] = sign * sdf(ax[x], ay[y], az[z])
 * at lattice point (x, y, z) = 8 (bx, by, bz) + (lx, ly, lz) of brick bricks[j] = (bx nbp + by) nbp + bz, nbp = ceil(res / 8), for
 * the points with x, y, z < res (the others are not written).  ax / ay / az: res values each (the dense lattice's axes, so
 * the values are bit-equal to surf_sdf_lattice_*'s).  n_bricks * 512 < 2^31 per call. */
int surf_sdf_bricks_bf16x3(const float* ax, const float* ay, const float* az, int res, const int32_t* bricks, int64_t n_bricks,
                           const float* const* h_vols, const int32_t* const* h_tables, const int* h_dims, int n_vol, const void* packed,
                           float* out, float sign, void* stream);
int surf_sdf_bricks_f16x2(const float* ax, const float* ay, const float* az, int res, const int32_t* bricks, int64_t n_bricks,
                          const float* const* h_vols, const int32_t* const* h_tables, const int* h_dims, int n_vol, const void* packed,
                          float* out, float sign, void* stream);

/*
 * Second-order term of the SDF network (training): grad (n,3) (optional) and smooth (n,3) = H.1, the row sums of the
 * Hessian of the SDF wrt the point.  Replaces the two chained torch.autograd.grad calls of SDFNetworkSparse.gradient
 * (models/modules/sdf_network.py:129-152; `smooth` feeds smooth_error, implicit_surface.py:172) by their closed form
 * in plain fp32.  idx (optional): compacted list of the n point indices to evaluate; other rows are left untouched.
 * surf_sdf_smooth_pack_weights takes the same host matrices as surf_sdf_pack_weights.
 */
int64_t surf_sdf_smooth_packed_floats(void);
int surf_sdf_smooth_pack_weights(const float* const* h_W, const float* const* h_b, float* h_packed);
int surf_sdf_smooth(const float* pts, const int32_t* idx, int64_t n, const float* const* h_vols,
                    const int32_t* const* h_tables, const int* h_dims, int n_vol, const float* packed, float* grad,
                    float* smooth, void* stream);

/*
 * Backward of the multi-view feature-consistency term (mfc_loss, losses/loss.py:43-45) w.r.t. the SDF: the patches depend
 * on the network only through the surface point p = o + d z0 (normal and feature maps are detached, implicit_surface.py:
 * 224-235), so d ncc / d z0 is the forward-mode tangent of (surface_patch_warp2 -> compute_LNCC2) along the ray.
 *   surf_patch_warp_tangent  surf_patch_warp's outputs plus their derivatives along dirs (R,3) = d pts / d z0
 *   surf_lncc_jvp            ncc (optional) and d ncc / d z0 (n_rays) from patches and tangents
 *   surf_crossing_backward   d_sdf (R,S) += g_z0 dz0/d sdf at the two samples bracketing the first sign change
 *                            (implicit_surface.py:181-220; nothing where there is no crossing or z0 left [0, *zmax])
 */
int surf_patch_warp_tangent(const float* pts, const float* dirs, const float* grads, int n_rays, const float* const* h_maps_t4,
                            int nv, int H, int W, const float* h_intrs, const float* h_kinv_ref, const float* h_c2w,
                            int patch_size, float* ref_out, float* src_out, float* ref_tan, float* src_tan, void* stream);
int surf_lncc_jvp(const float* ref, const float* src, const float* ref_tan, const float* src_tan, int64_t n_rays, int n_src,
                  int patch_elems, int channels, float* ncc, float* dncc, void* stream);
int surf_crossing_backward(const float* sdf, const uint8_t* vmask, const float* mid_z, int n_rays, int S, const float* zmax,
                           const float* g_z0, float* d_sdf, void* stream);

/*
 * Tall-skinny reduction for the weight / bias gradients of the backward kernels:
 *   out (M, N + with_sum) = (accumulate ? out : 0) + A[:, :M]^T [ X[:, :N] | 1 ]      A (rows, ldA), X (rows, ldX) row-major
 * M <= 128, N + with_sum <= 160.  workspace: surf_colgram_workspace_floats(rows, M, N) device floats.  Deterministic
 * (slab partials + a second pass, no atomics).
 */
int64_t surf_colgram_workspace_floats(int64_t rows, int M, int N);
int surf_colgram(const float* A, int ldA, int M, const float* X, int ldX, int N, int64_t rows, int with_sum, int accumulate,
                 float* workspace, float* out, void* stream);
/* The same with a precision policy: 0 = fp32-equivalent (surf_colgram: fp32 FMAs for rows < 4096, otherwise the matrix cores with an
 * exact three-way bf16 operand split and fp32 accumulation), 1 = operands rounded to ONE bf16 piece, fp32 accumulation (the
 * weight-gradient reductions of `train.precision = bf16`, BASELINE configs[3]). */
int surf_colgram_p(const float* A, int ldA, int M, const float* X, int ldX, int N, int64_t rows, int with_sum, int accumulate,
                   int precision, float* workspace, float* out, void* stream);

/*
 * Backward of the blending network w.r.t. its parameters for an upstream gradient of the per-sample colour (gcolor, indexed
 * like pts): the autograd of BlendingNetwork.forward (blending_network.py:69-118) under loss.backward() in closed form.
 * rows (n, nv-1, surf_blend_backward_row_floats()): per (sample, view) the INPUT vector and the pre-activation ADJOINT of
 * each of the 11 linear layers (column layout in blend_bwd.hip); dW = adj^T in, db = sum adj.  ds (n): per-sample d/d s.
 * color (n,3), optional: the recomputed forward colour.  raw_weights: DEVICE copy of the raw parameter buffer
 * (surf_blend_raw_floats(), state_dict order).  h_gfeats_t4 (may be NULL): four texel4 maps like h_feats_t4 that ACCUMULATE
 * the gradient of the sampled feature channels (generalisation training: the FPN's share of the colour loss).
 */
int surf_blend_backward_row_floats(void);
int surf_blend_backward(const float* pts, const int32_t* idx, int64_t n, const float* gcolor, const float* const* h_feats_t4,
                        const int* h_feat_hw, const float* imgs_t4, int nv, const float* h_intrs, const float* h_w2c,
                        const float* h_c2w, const float* raw_weights, float* rows, float* ds, float* color,
                        float* const* h_gfeats_t4, void* stream);

/*
 * Local normalised cross-correlation of the surface patches: out (n_rays) = mean of the two smallest per-view values of
 * mean_c clamp(1 - cov^2 / (var_ref var_src + 1e-5), 0, 2).  Replaces compute_LNCC2 (models/losses/ncc.py:7-51), the
 * multi-view feature-consistency term of Loss.forward (losses/loss.py:43-45).  ref (1, n_rays, P, C), src (n_src, n_rays, P, C)
 * as written by surf_patch_warp; n_src >= 2.
 */
int surf_lncc(const float* ref, const float* src, int64_t n_rays, int n_src, int patch_elems, int channels, float* out,
              void* stream);

/*
 * Backward of surf_lncc: the autograd of compute_LNCC2 (models/losses/ncc.py:7-51) under loss.backward() (runner.py:163).
 * g_out (n_rays): upstream gradient of the per-ray value; g_ref (1, n_rays, P, C) and g_src (n_src, n_rays, P, C): gradients
 * of the two patch stacks (fully written: zero for the views outside the two smallest of a ray).
 */
int surf_lncc_backward(const float* ref, const float* src, const float* g_out, int64_t n_rays, int n_src, int patch_elems,
                       int channels, float* g_ref, float* g_src, void* stream);

/*
 * Per-pixel terms of the photometric loss of one depth map (training).  Replaces compute_ptloss + SSIM
 * (models/losses/photometric_loss.py:54-125, :6-33): the other nv-1 views are warped into view ref_idx through `depth` (H,W)
 * (bilinear, zeros, align_corners=True) into `warp` (nv-1,H,W,4: rgb + validity); terms (H,W,8) =
 * [l1 m, grad_x mx, grad_y my, ssim m | m, mx, my, m], every loss value being the SUM of its topk smallest source views
 * and m / mx / my the reference mask and its products with the right / lower neighbour.  The loss is
 * sum(col0)/(sum(col4)+1e-8) + sum(col1)/(sum(col5)+1e-8) + sum(col2)/(sum(col6)+1e-8) + sum(col3)/(sum(col7)+1e-8)
 * (col7 repeats col4 so that the four quotients are one vector division).
 * imgs_t4 (nv,H,W,4) texel4; h_intrs / h_c2w / h_w2c: host (nv,4,4) intrinsics, camera-to-world and their inverses.
 */
int surf_ptloss_terms(const float* imgs_t4, int nv, int H, int W, const float* depth, const float* mask, int ref_idx, int topk,
                      const float* h_intrs, const float* h_c2w, const float* h_w2c, float* warp, float* terms, void* stream);

/*
 * Backward of the SDF network for upstream gradients of the SDF value (ybar, n) and of its spatial gradient (gbar, n x 3):
 * gbar . grad is the forward-mode tangent of the SDF along gbar, so one reverse sweep over a (value, tangent) forward sweep
 * replaces the reference's double backward (sdf_network.py:129-141 under loss.backward(), runner.py:163).  The kernel writes
 * per-sample buffers - in_v / in_d (7, n, 160): every layer's inputs and their tangents; tb / tdb (6, n, 128): the adjoints
 * of lin0..lin5's pre-activations and of their tangents - from which dW_l = tb_l^T in_v_l + tdb_l^T in_d_l, db_l = sum tb_l
 * (lin6 row 0: sum ybar in_v_6 + in_d_6), and accumulates the gradient of the sparse feature rows into h_dvols[s] (N_s, 8)
 * with float atomics (caller zero-fills; NULL = skip).  packed: surf_sdf_smooth_pack_weights' image.
 */
int surf_sdf_backward(const float* pts, const float* ybar, const float* gbar, int64_t n, const float* const* h_vols,
                      const int32_t* const* h_tables, const int* h_dims, int n_vol, float* const* h_dvols, const float* packed,
                      float* in_v, float* in_d, float* tb, float* tdb, void* stream);

/* Backward of the smooth (H.1) loss term through the SDF network (the autograd of sdf_network.py:143-150 under loss.backward(),
 * losses/loss.py:40): for sbar (n,3) = d loss / d smooth, the gradients of sum_n sbar_n . (H_n 1) = the mixed second directional
 * derivative of the SDF along (1,1,1) and sbar_n - one reverse sweep over a forward sweep with four streams (value, tangent
 * along 1, tangent along sbar, mixed).  Per-sample buffers like surf_sdf_backward's with the four streams stacked per layer:
 * in (7, 4, n, 160), ab (6, 4, n, 128); dW_l = ab[l]^T in[l] over the 4 n rows, db_l = column sums of ab[l][0]; lin6: dW row 0 =
 * column sums of in[6][3].  h_dvols: the sparse feature rows' gradients (N_s, 8), accumulated (may be NULL). */
int surf_sdf_smooth_backward(const float* pts, const float* sbar, int64_t n, const float* const* h_vols,
                             const int32_t* const* h_tables, const int* h_dims, int n_vol, float* const* h_dvols,
                             const float* packed, float* in, float* ab, void* stream);

/*
 * Multi-view feature fetch + blending MLP.
 * Replaces lookup_feature/compute_angle (projector.py:485-556) and BlendingNetwork.forward
 * (blending_network.py:69-118).
 *   h_feats[n_level]: texel4 maps (nv,H_i,W_i,4) fine -> coarse, h_hw[2*n_level] their sizes
 *   imgs: texel4 (nv,H,W,4) rgb
 *   h_intrs (nv,4,4), h_w2c (nv,4,4) = inverse(c2w), h_c2w (nv,4,4): HOST row-major
 *   blend_w: device copy of surf_blend_pack_weights output
 *   color (n,3); n_valid (n) uint8 = number of source views the point projects into
 * Only the shipped colour network (d_feature 16 = 4 pyramid levels x 4 channels) is supported.
 */
int surf_blend_raw_floats(void);     /* floats of the concatenated state_dict tensors, order below   */
int surf_blend_packed_floats(void);  /* floats of the MFMA-ordered buffer the kernel reads            */
/* h_raw: HOST concatenation of color_network.{s, ray_dir_fc.0.weight, ray_dir_fc.0.bias, ray_dir_fc.2.*,
 * base_fc.0.*, base_fc.2.*, vis_fc.0.*, vis_fc.2.*, vis_fc2.0.*, vis_fc2.2.*, rgb_fc.0.*, rgb_fc.2.*,
 * rgb_fc.4.*} (weight then bias, row-major), i.e. blending_network.py:34-64 in declaration order. */
int surf_blend_pack_weights(const float* h_raw, float* h_packed);
int surf_blend(const float* pts, const uint8_t* mask, const int32_t* idx, int64_t n, const float* const* h_feats, const int* h_hw,
               int n_level, const float* imgs, int nv, const float* h_intrs, const float* h_w2c,
               const float* h_c2w, const float* blend_w, float* color, uint8_t* n_valid, void* stream);

/*
 * The same blending MLP on the 16-bit MFMA pipes (blend_split.hip): every fp32 operand split into 16-bit pieces, fp32
 * accumulation.  precision: SURF_BLEND_BF16X3 (exact three-way bf16 split, six products: fp32-equivalent) or
 * SURF_BLEND_F16X2 (two fp16 pieces, 22-bit operands, three products).  `blend_w` is the device copy of
 * surf_blend_pack_weights_split's output for the same precision (the kernel's LDS image); other arguments as surf_blend.
 */
#define SURF_BLEND_BF16X3 1
#define SURF_BLEND_F16X2 2
#define SURF_BLEND_F32 3      /* the same LDS-resident kernel on v_mfma_f32_32x32x2_f32, no operand split */
int64_t surf_blend_split_packed_bytes(int precision);
int surf_blend_pack_weights_split(const float* h_raw, unsigned char* h_packed, int precision);
/* Bytes of device scratch a launch over n points with nv views needs (the launch's tile counter, then per-wavefront staging of
 * the per-view inputs of the second pass; stays in L2 / Infinity Cache).  Contents need not be preserved between launches: the
 * entry points zero the counter on the launch stream themselves.  One buffer serves one launch at a time. */
int64_t surf_blend_split_scratch_bytes(int64_t n_points, int nv);
int surf_blend_split(const float* pts, const uint8_t* mask, const int32_t* idx, int64_t n, const float* const* h_feats,
                     const int* h_hw, int n_level, const float* imgs, int nv, const float* h_intrs, const float* h_w2c,
                     const float* h_c2w, const void* blend_w, int precision, float* color, uint8_t* n_valid, void* scratch,
                     void* stream);
/* ... with the number of idx entries read from device memory, as surf_sdf_mlp_bf16x3_dn. */
int surf_blend_split_dn(const float* pts, const int32_t* idx, int64_t n_capacity, const int32_t* d_n, const float* const* h_feats,
                        const int* h_hw, int n_level, const float* imgs, int nv, const float* h_intrs, const float* h_w2c,
                        const float* h_c2w, const void* blend_w, int precision, float* color, uint8_t* n_valid, void* scratch,
                        void* stream);

/*
 * NeuS SDF -> alpha compositing, zero-crossing depth and per-ray reductions.
 * Replaces render_core's tail (implicit_surface.py:126-166,181-216) and validate's normal sum (:380-382).
 *   per-sample inputs (R,S): sdf, grad(3), color(3), n_valid, mid_z, dists, pts(3), vmask
 *   h_rot_ref: inverse(c2w[0][:3,:3]) row-major (9 floats, HOST)
 * outputs (R rows each; any may be NULL): color(3), render_depth, sdf_depth, normal(3) (camera frame),
 *   normal_val(3) = sum_k grad*w*inside (world frame, for validate), valid_mask u8, mid_inside u8,
 *   weights (R,S), inside (R,S), eik (R,2) = per-ray [sum relax*(|g|-1)^2, sum relax],
 *   z_sdf0 (R) = the zero crossing's ray parameter before the validity factor and the cosine (feeds surf_surface_points)
 */
int surf_composite(const float* sdf, const float* grad, const float* color, const uint8_t* n_valid,
                   const float* mid_z, const float* dists, const float* pts, const uint8_t* vmask,
                   const float* rays_d, int n_rays, int S, float inv_s, float cos_anneal_ratio,
                   const float* h_rot_ref, float* out_color, float* out_depth, float* out_sdf_depth,
                   float* out_normal, float* out_normal_val, uint8_t* out_valid, uint8_t* out_mid_inside,
                   float* out_weights, float* out_inside, float* out_eik, float* out_z_sdf0, void* stream);
/*
 * Backward of surf_composite for the outputs the training loss differentiates (colour_fine, render_depth, the eikonal
 * sums): the autograd of render_core's tail (implicit_surface.py:126-166) in closed form.  g_color (R,3), g_depth (R, may
 * be NULL): upstream gradients; eik_scale = dL/d gradient_error / (sum relax + 1e-5).  Outputs: d_sdf (R,S), d_grad (R,S,3),
 * d_color (R,S,3), d_inv_s (R) per-ray partial sums.  First kernel of the training row's backward side.
 */
int surf_composite_backward(const float* sdf, const float* grad, const float* color, const float* mid_z, const float* dists,
                            const float* pts, const uint8_t* vmask, const float* rays_d, int n_rays, int S, float inv_s,
                            float cos_anneal_ratio, const float* h_rot_ref, const float* g_color, const float* g_depth,
                            float eik_scale, float* d_sdf, float* d_grad, float* d_color, float* d_inv_s, void* stream);
/* The same with the upstream gradient of gradient_error left ON THE DEVICE: eik_upstream (1 float, may be NULL = 1) multiplies
 * eik_scale inside the kernel, so a caller holding dL/d gradient_error as a device scalar (autograd) passes
 * eik_scale = 1 / (sum relax + 1e-5) and never reads the scalar back (a synchronising read at the head of the backward sweep). */
int surf_composite_backward_s(const float* sdf, const float* grad, const float* color, const float* mid_z, const float* dists,
                              const float* pts, const uint8_t* vmask, const float* rays_d, int n_rays, int S, float inv_s,
                              float cos_anneal_ratio, const float* h_rot_ref, const float* g_color, const float* g_depth,
                              float eik_scale, const float* eik_upstream, float* d_sdf, float* d_grad, float* d_color,
                              float* d_inv_s, void* stream);


/* =====================================================================================================
 * Volume build (surf.py:80-131).  Voxel coordinates are int32 triples; voxel_size = 2/(D-1), origin -1.
 * ===================================================================================================== */

/*
 * Children + depth-band test.  Replaces Volume.up_sample (volume.py:35-52) and the test of
 * Volume.depth_filtering (volume.py:134-165).  Child o of parent p has coordinate 2*parent + pos_list[o]
 * (order of volume.py:42).  flags[8 p + o] = 1 iff |warped depth - voxel depth| < depth_range in > 1 views.
 *   parents (n_parents,3) on the D/2 lattice; D = child lattice side; depths (nv,H,W) previous-stage maps
 */
int surf_upsample_filter(const int32_t* parents, int64_t n_parents, int D, const float* depths, int nv, int H, int W,
                         const float* h_intrs, const float* h_w2c, float depth_range, uint8_t* flags, void* stream);

/*
 * Homography warp + softmax mean/variance cost volume.  Replaces Volume.back_proj_multiscale
 * (volume.py:54-97).  Voxel i = site i of the full D^3 lattice (parents == idx == NULL, n == D^3, x slowest,
 * volume.py:21-33) or child (idx[i] & 7) of parent (idx[i] >> 3).
 *   h_feats[4]: texel4 pyramids COARSE -> fine (the reference's `features` order), h_hw[8] their (H,W);
 *   levels stage..3 are summed; h_agg: agg_mlp as [0.weight(8x4) | 0.bias(8) | 2.weight(8) | 2.bias(1)] (HOST)
 * outputs: coords (n,3), feat (n,8) = [mean | var], keep (n) = (#views in frustum > 1)
 */
int surf_costvol(const int32_t* parents, const int32_t* idx, int64_t n, int D, const float* const* h_feats,
                 const int* h_hw, int stage, int nv, const float* h_intrs, const float* h_w2c, const float* h_agg,
                 int32_t* coords, float* feat, uint8_t* keep, void* stream);

/* Stable stream compaction: idx_out = ascending indices i with flags[i] != 0, *total = their number
 * (device int).  Replaces the boolean-mask indexing of volume.py:165-166 / surf.py:104-108.
 * workspace: surf_compact_workspace_ints(n) int32; idx_out must hold up to n entries. */
int64_t surf_compact_workspace_ints(int64_t n);
int surf_compact(const uint8_t* flags, int64_t n, int32_t* workspace, int32_t* idx_out, int32_t* total, void* stream);
/* The same compaction of an (n_rays, n_samples) ray-major flag array, emitted in the traversal order
 * (ray / G, s / B, ray % G, s % B) with G = rays_per_block, B = samples_per_block: a 32-entry tile of the list then holds a
 * few consecutive samples of a few neighbouring rays.  The last ray block may hold fewer than G rays.  idx_out still holds
 * flat ray-major indices ray * n_samples + s: a permutation of surf_compact's list (G = 1, B = n_samples: the same list);
 * *total is their number (device int).  Same workspace (of n = n_rays * n_samples) and the same three launches.
 * G and B must be powers of two and B must divide n_samples (SURF_E_ARG); n + G * n_samples < 2^31 (SURF_E_LIMIT). */
int surf_compact_blocked(const uint8_t* flags, int64_t n_rays, int64_t n_samples, int rays_per_block, int samples_per_block,
                         int32_t* workspace, int32_t* idx_out, int32_t* total, void* stream);

/* dst[i, off:off+row_words] = src[idx[i] >> idx_shift, :]  (rows of 32-bit words; idx_shift 3 = row of the parent) */
int surf_gather_rows(const void* src, const int32_t* idx, int64_t n, int row_words, int idx_shift, int dst_stride_words,
                     int dst_offset_words, void* dst, void* stream);
/* out[i] = a[b[i]] */
int surf_compose_index(const int32_t* a, const int32_t* b, int64_t n, int32_t* out, void* stream);

/*
 * Dense matching volume + index table.  Replaces Volume.sparse2dense and Volume.get_index
 * (volume.py:99-121, 123-132): dense = x2 trilinear upsample (align_corners=False) of prev (D/2)^3, or zeros
 * if prev == NULL; dense[coords[i]] = rows[i*row_stride]; table = -1 then table[coords[i]] = i.
 */
int surf_densify(const int32_t* coords, const float* rows, int row_stride, int64_t n, int D, const float* prev,
                 float* dense, int32_t* table, void* stream);

/*
 * Matching field: per-view softmax-expected depth.  Replaces MatchingField.forward / depth_render
 * (matching_field.py:73-141, 18-71, perturb False).
 *   h_kinv (nv,3,3) = inverse(intrs)[:, :3, :3]; h_c2w (nv,4,4); h_rinv (nv,3,3) = inverse(c2w[:, :3, :3]);
 *   h_near_fars (nv,2) -- HOST.  lin_x/lin_y/lin_n: device copies of torch.linspace(0,W-1,w), (0,H-1,h), (0,1,n).
 *   pre_depths (nv,H,W) or NULL (stage 0); ratio_cur/ratio_prev = range_ratios[stage], [stage-1]
 * jitter (optional, device, (nv, h*w, 2)): the train-mode `torch.rand([batch, 1]) - 0.5` of every ray and band
 * (matching_field.py:33-35; zeros for the views rendered without it, :129-133)
 * outputs: depth_lr (nv,h,w) and depth_full (nv,H,W) = bilinear upsample (align_corners=False);
 * stats (nv,h,w,4) or NULL: per ray (max logit, softmax denominator, expected z, 0) for surf_matching_depth_backward
 */
int surf_matching_depth(const float* mvol, int D, int nv, const float* h_kinv, const float* h_c2w, const float* h_rinv,
                        const float* h_near_fars, int H, int W, int h, int w, const float* lin_x, const float* lin_y,
                        const float* lin_n, int n, const float* pre_depths, float ratio_cur, float ratio_prev,
                        const float* jitter, float* depth_lr, float* depth_full, float* stats, void* stream);

/* =====================================================================================================
 * Sparse 3D U-Net pieces (reg_network.py:38-88 over torchsparse 2.1.0 -- third party, PARITY UNPINNED).
 * Kernel (27, C_in, C_out), offsets enumerated x fastest / z slowest; rows of C floats, C in {8,16,32,64}.
 * ===================================================================================================== */

/*
 * One sparse convolution with fused BatchNorm(eval) + ReLU (+ skip add after the ReLU, reg_network.py:79-83).
 *   mode 0 submanifold (stride 1): out site c gathers input sites c + o            (in_table on the same lattice)
 *   mode 1 down (k3, stride 2):    out site q gathers input sites 2q + o          (in_table on the fine lattice)
 *   mode 2 up (transposed, s2):    out site c gathers input sites q with 2q + o = c (in_table on the coarse lattice)
 *   bn_scale = gamma / sqrt(running_var + eps), bn_shift = beta - running_mean * bn_scale (device, C_out), or both NULL
 */
int surf_spconv(const float* in, int cin, const int32_t* in_table, int D_in, const int32_t* out_coords, int64_t n_out,
                int mode, const float* weight, int cout, const float* bn_scale, const float* bn_shift, const float* skip,
                float* out, void* stream);
/* bf16 ROW STORAGE of the sparse U-Net under the bf16 training policy (round 6; conf key train_precision = bf16).  Activations
 * keep their fp32 rows (BatchNorm statistics, skip sums, the backward's streaming reads) and get a bf16 SHADOW (n, C) uint16 that
 * the gather side of the next convolution reads instead: surf_bn_relu_apply16 / surf_bn_relu_backward16 = the fp32 entry points
 * below with the shadow of their output written in the same pass (out16 / dx16 may be NULL), surf_rows_to_bf16 for rows that come
 * from elsewhere, surf_spconv_rows16 = surf_spconv (no BN epilogue) for the (16, 8) channel pair - the one where halving the row
 * bytes pays - gathering from the shadow; fp32 weights, accumulation and output.  Never used by inference. */
int surf_spconv_rows16(const uint16_t* in16, int cin, const int32_t* in_table, int D_in, const int32_t* out_coords, int64_t n_out,
                       int mode, const float* weight, int cout, float* out, void* stream);
int surf_rows_to_bf16(const float* x, int64_t n_floats, uint16_t* out16, void* stream);
int surf_bn_relu_apply16(const float* x, int64_t n, int channels, const float* scale, const float* shift, const float* skip,
                         float* out, uint16_t* out16, void* stream);
int surf_bn_relu_backward16(const float* x, const float* dy, int64_t n, int channels, const float* scale, const float* shift,
                            const float* mean, const float* invstd, int train, void* workspace, float* dgamma, float* dbeta,
                            float* dx, uint16_t* dx16, void* stream);
/*
 * The same convolution on the matrix cores for the wide layers (C_in, C_out in {16, 32, 64}): per-offset gather-GEMM,
 * fp32 operands split exactly into three bf16 pieces (fp32-equivalent results).  surf_spconv_packed_bytes returns 0 for a
 * channel pair without such a kernel (use surf_spconv); surf_spconv_pack_weights (a device kernel on `stream`) turns the
 * (27, C_in, C_out) kernel into the split operand image `packed` once per model.
 */
int64_t surf_spconv_packed_bytes(int cin, int cout);
int surf_spconv_pack_weights(const float* weight, int cin, int cout, void* packed, void* stream);
/* bf16_operands != 0 (training under train_precision = bf16, BASELINE configs[3]): both operands rounded to bf16 - the first
 * piece of the same image, the first piece of the gathered rows - one product per k-step with fp32 accumulation instead of
 * the six of the exact split. */
int surf_spconv_mfma(const float* in, int cin, const int32_t* in_table, int D_in, const int32_t* out_coords, int64_t n_out,
                     int mode, const void* packed, int cout, const float* bn_scale, const float* bn_shift,
                     const float* skip, float* out, int bf16_operands, void* stream);

/*
 * BatchNorm with BATCH statistics over the voxel rows x (n, C) (train mode of spnn.BatchNorm, reg_network.py:14-15,28-29;
 * C in {8, 16, 32, 64}): scale = gamma / sqrt(var + eps), shift = beta - mean scale (device, C floats each), fp64 reduction;
 * running_mean / running_var (may both be NULL) are updated in place as torch.nn.BatchNorm1d does (momentum, unbiased
 * variance); batch_stats (may be NULL): mean | 1/sqrt(var + eps) (2C floats), what the backward needs.  surf_bn_relu_apply: out = relu(x scale + shift) (+ skip).  workspace: surf_bn_workspace_bytes(C) device bytes.
 */
int64_t surf_bn_workspace_bytes(int channels);
int surf_bn_train_affine(const float* x, int64_t n, int channels, const float* gamma, const float* beta, float eps,
                         float momentum, float* running_mean, float* running_var, float* scale, float* shift, float* batch_stats,
                         void* workspace, void* stream);
int surf_bn_relu_apply(const float* x, int64_t n, int channels, const float* scale, const float* shift, const float* skip,
                       float* out, void* stream);
/* Backward of y = relu(x scale + shift) (+ skip; the skip's gradient is dy itself) with scale = gamma invstd, shift = beta -
 * mean scale: x the raw convolution output, scale / shift the forward's affine, mean / invstd (C each) the statistics behind it.
 * train != 0: batch statistics (dx = scale (zbar - mean(zbar) - xhat mean(zbar xhat))); 0: running statistics (dx = scale zbar).
 * Outputs dgamma, dbeta (C), dx (n, C).  workspace: surf_bn_workspace_bytes(C). */
int surf_bn_relu_backward(const float* x, const float* dy, int64_t n, int channels, const float* scale, const float* shift,
                          const float* mean, const float* invstd, int train, void* workspace, float* dgamma, float* dbeta,
                          float* dx, void* stream);
/* InstanceNorm + ReLU (+ skip) backward of an FPN layer (models/modules/feature_network.py: nn.InstanceNorm2d, no affine
 * parameters) for all N views in three launches: x, dy, dx (N, hw, C) NHWC; stats (N, C, 2) = mean | rstd as surf_inorm_relu
 * wrote them; workspace: surf_inorm_backward_workspace_bytes(N, C) device bytes.  (= surf_bn_relu_backward per view with
 * scale = rstd, shift = -mean rstd, which is what the FPN backward called N times per layer until round 5.) */
int64_t surf_inorm_backward_workspace_bytes(int N, int channels);
int surf_inorm_relu_backward(const float* x, const float* dy, int N, int64_t hw, int channels, const float* stats, void* workspace,
                             float* dx, void* stream);

/* ---- backward of the volume build (train mode; the autograd of surf.py:80-131 under loss.backward(), runner.py:163) ----
 * surf_matching_depth_backward: same geometry arguments as surf_matching_depth; g_full (nv,H,W) = d loss / d depth maps
 * of the two views that carry gradient, view0 and view1 (the reference view and src_idx, matching_field.py:129-133; view1 < 0
 * or == view0: one view); the other views' maps are ignored; g_lr (nv,h,w) scratch; dmvol (D,D,D) ACCUMULATED.
 * The bands are constants (pre_depths are detached, matching_field.py:104).  stats: what surf_matching_depth wrote for the
 * same arguments (same jitter), or NULL - then the softmax statistics are recomputed by a first walk over the samples.
 * surf_densify_backward: g_rows[i * row_stride] += g_dense[coords[i]]; g_prev (D/2)^3 (may be NULL) accumulates the
 * background's share through the transposed x2 trilinear upsample (sites of the index table pass nothing).
 * surf_scatter_rows_add: backward of surf_gather_rows (float rows, atomics).
 * surf_costvol_backward: for the kept voxels `coords` (n,3) of a stage and g (n,8) = [d mean | d var], accumulates the
 * gradients of the summed feature levels into h_gfeats[l] (texel4 maps like h_feats[l], l >= stage) and of agg_mlp
 * (w1 | b1 | w2 | b2, 49 floats, device) into g_agg.  workspace: surf_costvol_backward_workspace_floats(n, nv, H, W) device
 * floats, (H, W) = the finest feature level (the kernel sorts its (view, voxel) adds by image tile: 9 floats per pair - 1.1 to
 * 1.5 GB of transient memory at the finest DTU stage, ~6 M voxels x 5 views); an upper bound for every pyramid.
 * surf_costvol_backward_workspace_floats_for(n, nv, h_hw): the exact need for the pyramid h_hw (4 x (H, W), coarse to fine, as
 * passed to surf_costvol_backward): 4,096 floats when the tile-sorted form will not run (irregular pyramid such as the
 * Tanks&Temples shape, more than 16,384 (view, tile) buckets) and the direct scatter is used instead. */
int surf_matching_depth_backward(const float* mvol, int D, int nv, const float* h_kinv, const float* h_c2w, const float* h_rinv,
                                 const float* h_near_fars, int H, int W, int h, int w, const float* lin_x, const float* lin_y,
                                 const float* lin_n, int n, const float* pre_depths, float ratio_cur, float ratio_prev,
                                 const float* jitter, const float* g_full, int view0, int view1, float* g_lr, float* dmvol,
                                 const float* stats, void* stream);
int surf_densify_backward(const int32_t* coords, int64_t n, int D, const int32_t* table, const float* g_dense, int row_stride,
                          float* g_rows, float* g_prev, void* stream);
int surf_scatter_rows_add(const float* g_dst, const int32_t* idx, int64_t n, int row_words, int idx_shift, int dst_stride_words,
                          int dst_offset_words, float* g_src, void* stream);
int64_t surf_costvol_backward_workspace_floats(int64_t n, int nv, int H, int W);
int64_t surf_costvol_backward_workspace_floats_for(int64_t n, int nv, const int* h_hw);
int surf_costvol_backward(const int32_t* coords, const float* g, int64_t n, int D, const float* const* h_feats,
                          float* const* h_gfeats, const int* h_hw, int stage, int nv, const float* h_intrs, const float* h_w2c,
                          const float* h_agg, float* workspace, float* g_agg, void* stream);

/* Weight gradient of the FPN's 3x3 convolutions (train mode; the autograd of feature_network.py:6-25,57-75):
 * out[ky][kx][cb][cs] = sum_(n,ys,xs) big[n][ys S + ky - 1][xs S + kx - 1][cb] small[n][ys][xs][cs], zero padding, NHWC maps,
 * big (N, Hs S, Ws S, cb), small (N, Hs, Ws, cs).  Conv2d: big = layer input, small = d output -> [ky][kx][ci][co];
 * ConvTranspose2d (S = 2): big = d output, small = layer input -> [ky][kx][co][ci].  Input gradients run on the forward
 * kernels: stride 1 -> surf_conv3x3 with the flipped, transposed kernel; stride 2 -> surf_deconv3x3_s2; deconv -> stride-2
 * surf_conv3x3.  InstanceNorm + ReLU backward = surf_inorm_relu_backward, one call for all views. */
int64_t surf_conv3x3_wgrad_workspace_floats(int N, int Hs, int Ws, int cb, int cs);
int surf_conv3x3_wgrad(const float* big, const float* small, int N, int Hs, int Ws, int cb, int cs, int stride,
                       float* workspace, float* out, void* stream);
/* With a precision argument (as surf_conv3x3_p): pairs with max(cb, cs) >= 16 run on the matrix cores - a GEMM over the pixel
 * index with both operands read transposed, per-row-group partial sums in the workspace, summed in a fixed order. */
int surf_conv3x3_wgrad_p(const float* big, const float* small, int N, int Hs, int Ws, int cb, int cs, int stride,
                         float* workspace, float* out, int precision, void* stream);

/* Backward of surf_ptloss_terms w.r.t. the depth map (train mode; the autograd of losses/photometric_loss.py:54-125):
 * warp = the forward's warped images; coef (device, 4 floats) = upstream / (M_t + 1e-8) for the l1, gx, gy and ssim terms;
 * g_warp (ns,H,W,4) scratch (zeroed here); g_depth (H,W) written.  Only the topk sources selected by the forward receive
 * gradient (torch.topk's backward); validity masks and the SSIM mask pool are constants. */
int surf_ptloss_backward(const float* imgs_t4, int nv, int H, int W, const float* depth, const float* mask, int ref_idx, int topk,
                         const float* h_intrs, const float* h_c2w, const float* h_w2c, const float* warp, const float* coef,
                         float* g_warp, float* g_depth, void* stream);




/*
 * Weight gradient of surf_spconv (no BN): dW (27, C_in, C_out) += sum_i x[neighbour_k(i)] (x) dy[i]  (float atomics; the caller
 * zero-fills).  The INPUT gradient is surf_spconv itself on the swapped lattices: submanifold with mirrored offsets
 * (slice 26 - k), stride-2 down <-> transposed up, kernel slices transposed (surf_amd.ops.spconv_backward).
 */
int surf_spconv_wgrad(const float* x, int cin, const int32_t* in_table, int D_in, const int32_t* out_coords, int64_t n_out,
                      int mode, const float* dy, int cout, float* dW, void* stream);
/* The same weight gradient on the matrix cores (per offset the GEMM X_k^T dY over the sites: 64-site tiles, the 27 offsets dealt
 * over the four wavefronts, dy split once per tile; exact three-way bf16 split, six products: fp32-equivalent) for the channel
 * pairs where it beats the per-voxel kernels - surf_spconv_wgrad_mfma_supported returns 1 for those ((8,16), (16,32), (32,16),
 * (32,32)), 0 otherwise. */
int surf_spconv_wgrad_mfma_supported(int cin, int cout);
int surf_spconv_wgrad_mfma(const float* x, int cin, const int32_t* in_table, int D_in, const int32_t* out_coords, int64_t n_out,
                           int mode, const float* dy, int cout, float* dW, void* stream);

/* bbox (device int32[6]) = [min x, min y, min z, max x, max y, max z] of coords (n,3) */
int surf_coords_bbox(const int32_t* coords, int64_t n, int32_t* bbox, void* stream);
/* Output sites of a k3/s2 conv, marks[(D/2+1)^3] |= 1 (marks zeroed by the caller).  torchsparse 2.1 is absent, which of its
 * down-sampling rules the authors' checkpoint was trained with is unknown, so both are offered:
 *   SURF_DOWN_DILATE  q is an output site when 2q lies in the 3^3 window of an input voxel and inside the inputs'
 *                     bounding box (device int32[6] from surf_coords_bbox: no host round trip)        [default]
 *   SURF_DOWN_FLOOR   q = floor(c / 2) for every input voxel c (bbox unused, may be NULL) */
#define SURF_DOWN_DILATE 0
#define SURF_DOWN_FLOOR 1
int surf_mark_down_sites(const int32_t* coords, int64_t n, int D, const int32_t* bbox, uint8_t* marks, int rule, void* stream);
/* keys (ascending lattice site numbers, e.g. from surf_compact) -> coords (n,3) and table[key] = rank */
int surf_sites_from_keys(const int32_t* keys, int64_t n, int D, int32_t* coords, int32_t* table, void* stream);
/* table[coords[i]] = i (table pre-filled with -1 by the caller) */
int surf_table_from_coords(const int32_t* coords, int64_t n, int D, int32_t* table, void* stream);
/* out = in @ W^T for rows of 8 floats (out_lin, reg_network.py:67,86) */
int surf_row_linear8(const float* in, const float* weight, int64_t n, float* out, void* stream);

/* =====================================================================================================
 * FPN (feature_network.py:126-178).  Activations NHWC fp32, channels a multiple of 4 (the RGB input is the
 * texel4 image); weights repacked by the host to [ky][kx][c_in][c_out].
 * ===================================================================================================== */

/* 3x3 convolution, padding 1, stride 1 or 2, no bias (feature_network.py:15,151).  out (N, H/stride, W/stride, cout). */
int surf_conv3x3(const float* in, const float* weight, int N, int H, int W, int cin, int cout, int stride, float* out,
                 void* stream);
/* ConvTranspose2d(3x3, stride 2, padding 1, output_padding 1), no bias (feature_network.py:66,155).  out (N,2H,2W,cout). */
int surf_deconv3x3_s2(const float* in, const float* weight, int N, int H, int W, int cin, int cout, float* out, void* stream);
/* The same two with a precision argument.  Layers with cin >= 16 run on the matrix cores (csrc/fpn_mfma.hip, round 6):
 * precision 0 = fp32-equivalent (both operands split exactly into three bf16 pieces, six products, fp32 accumulate: what
 * surf_conv3x3 / surf_deconv3x3_s2 call), 1 = operands rounded to bf16, one product (the bf16 training policy, conf key
 * train_precision; never used by inference).  cin < 16: the fp32 VALU kernels whatever the precision.  weight: fp32
 * [ky][kx][cin][cout] as above - split on the fly, there is no packed weight image. */
int surf_conv3x3_p(const float* in, const float* weight, int N, int H, int W, int cin, int cout, int stride, float* out,
                   int precision, void* stream);
int surf_deconv3x3_s2_p(const float* in, const float* weight, int N, int H, int W, int cin, int cout, float* out, int precision,
                        void* stream);
/* In place: x = relu(InstanceNorm2d(x)) (+ skip)  (feature_network.py:16-17,21-24; skip add :170).
 * workspace: surf_inorm_workspace_doubles(N,H,W,C) doubles; stats (N,C,2) receives mean and 1/sqrt(var+1e-5).
 * C must be a multiple of 4 that divides 256 (4, 8, 16, 32, 64: the channel counts surf_conv3x3 / surf_deconv3x3_s2 are
 * instantiated for; since round 5 the statistics pass assigns 256 / C pixels to a workgroup row); any other C is SURF_E_ARG.
 * surf_inorm_relu_backward: C in {8, 16, 32, 64}. */
int64_t surf_inorm_workspace_doubles(int N, int H, int W, int C);
int surf_inorm_relu(float* x, int N, int H, int W, int C, const float* skip, double* workspace, float* stats, void* stream);
/* The same into `out` (N,H,W,C), x left as it is: a recording (train-mode) forward keeps the raw convolution output for
 * surf_inorm_relu_backward and needs no copy of it. */
int surf_inorm_relu_out(const float* x, int N, int H, int W, int C, const float* skip, double* workspace, float* stats,
                        float* out, void* stream);

/*
 * Surface patches for the LNCC loss (training outputs ref_gray_val / sampled_gray_val).  Replaces render_core's tail
 * (implicit_surface.py:217-245), surface_patch_warp2 (projector.py:560-627) and patch_homography (:630-645).
 *   surf_upsample_bilinear_t4  F.interpolate(bilinear, align_corners=False) of a texel4 map (n,h,w,4) -> (n,H,W,4)
 *   surf_surface_points        pts = rays_o + rays_d * z with z = z_sdf0 zeroed outside [0, max(z_vals)] (:217-220);
 *                              workspace: one device uint32
 *   surf_patch_warp            maps: the three finest FPN levels as texel4 (nv,H,W,4) at FULL resolution (levels 1, 2
 *                              upsampled); h_intrs / h_c2w (nv,4,4) HOST; h_kinv_ref = inverse(intrs)[0][:3,:3] (9 floats);
 *                              grads = raw SDF gradients at pts; ref_out (1,R,p*p,12), src_out (nv-1,R,p*p,12)
 */
int surf_upsample_bilinear_t4(const float* src, int n, int h, int w, int H, int W, float* dst, void* stream);
int surf_surface_points(const float* rays_o, const float* rays_d, const float* z_sdf0, int n_rays, const float* z_vals,
                        int64_t n_z, unsigned* workspace, float* pts, void* stream);
int surf_patch_warp(const float* pts, const float* grads, int n_rays, const float* const* h_maps, int nv, int H, int W,
                    const float* h_intrs, const float* h_kinv_ref, const float* h_c2w, int patch_size, float* ref_out,
                    float* src_out, void* stream);

/* =====================================================================================================
 * Small fused helpers of the training step (csrc/train_small.hip): chains of tiny torch ops as single launches.
 * ===================================================================================================== */

/* lookup_volume(pts, mask_volumes, 'nearest').any(-1) (models/modules/implicit_surface.py:175; the mask volume of a level is
 * 1 exactly where its index table is >= 0, volume.py:112-130): out[i] = 1 when the voxel nearest to pts[i] (grid_sample
 * 'nearest', align_corners=False: round-half-even of ((p + 1) D - 1) / 2, zeros outside) is occupied on ANY level.
 * pts (n,3) device; h_tables / h_dims: HOST arrays of `levels` device index tables (D^3 int32) and their D; out (n) bytes. */
int surf_occupied_any(const float* pts, int64_t n, const int32_t* const* h_tables, const int* h_dims, int levels, uint8_t* out,
                      void* stream);

/* sum(|pred - target| mask) / (sum(mask) + 1e-8) over n elements: the masked L1 of the depth terms of models/losses/loss.py
 * (:71-93).  mask_kind 0: mask = n floats; 1: n bytes (torch.bool); 2: mask = target > 0 (`mask` unused).  Sums in fp64, in a
 * fixed order.  workspace: surf_masked_l1_workspace_bytes() device bytes; counter: one device uint32 that is 0 on entry (the
 * kernel leaves it 0: allocate and clear it once per stream); out2[0] = the loss, out2[1] = 1 / (sum(mask) + 1e-8).
 * The backward: g_pred[i] = upstream[0] out2[1] sgn(pred - target) mask  (upstream: a device scalar). */
int64_t surf_masked_l1_workspace_bytes(void);
int surf_masked_l1(const float* pred, const float* target, const void* mask, int mask_kind, int64_t n, void* workspace,
                   unsigned* counter, float* out2, void* stream);
int surf_masked_l1_backward(const float* pred, const float* target, const void* mask, int mask_kind, int64_t n, const float* out2,
                            const float* upstream, float* g_pred, void* stream);

/* Backward of the weight-norm re-parameterisation W = g v / |v|_row (models/modules/sdf_network.py:88-89, nn.utils.weight_norm)
 * of `layers` (<= 8) linear layers in one launch: dg = <dW, v>_row / |v|, dv = (g / |v|) (dW - (dg / |v|) v).
 * HOST arrays of device pointers: v, dW, dv (rows[l] x cols[l]), g, dg (rows[l]). */
int surf_weight_norm_backward(int layers, const float* const* h_v, const float* const* h_g, const float* const* h_dW,
                              const int* h_rows, const int* h_cols, float* const* h_dv, float* const* h_dg, void* stream);

/*
 * Marching cubes on a (nx, ny, nz) fp32 lattice u[x][y][z] (z fastest).  Replaces mcubes.marching_cubes(u, isovalue)
 * (PyMCubes 0.1.4, called at models/modules/implicit_surface.py:353): classic 256-case table, `u <= isovalue` inside
 * test, one vertex per sign-changing lattice edge by linear interpolation in double precision, lattice-index units.
 * Call sequence (the host sizes the outputs between the steps):
 *   surf_mc_classify  -> flags (nx*ny*nz bytes): bits 0-2 sign change along x/y/z from the point, bits 3-5 triangles of
 *                        the cell whose origin it is
 *   surf_compact(flags) -> active (ascending lattice indices of the non-zero flags)
 *   surf_mc_count     -> workspace (surf_mc_workspace_ints(n_active) int32), totals[0] = vertices, totals[1] = triangles
 *   surf_mc_emit      -> vertices (totals[0], 3) double, triangles (totals[1], 3) int32 vertex ids; vbase: scratch of
 *                        nx*ny*nz int32 (first vertex id of every active point)
 * Vertex order: (owner lattice point, axis); triangle order: cell (x outermost) then table order.
 */
int surf_mc_classify(const float* u, int nx, int ny, int nz, double isovalue, uint8_t* flags, void* stream);
int64_t surf_mc_workspace_ints(int64_t n_active);
int surf_mc_count(const uint8_t* flags, const int32_t* active, int64_t n_active, int32_t* workspace, int32_t* totals, void* stream);
int surf_mc_emit(const float* u, int nx, int ny, int nz, double isovalue, const uint8_t* flags, const int32_t* active,
                 int64_t n_active, const int32_t* workspace, int32_t* vbase, double* vertices, int32_t* triangles, void* stream);

/*
 * Narrow-band marching cubes (extract_geometry with render.mesh_extraction = band): the mesh of surf_mc_* on a res^3
 * lattice, the same arrays in the same order, from the SDF evaluated only in bricks of 8^3 cells near the surface.
 * Brick b owns lattice points 8b .. 8b+7 per axis and the cells whose origins those are; nbp = ceil(res / 8) bricks per axis
 * in the table (surf_band_table_size(res) = nbp^3 entries), brick ids (bx nbp + by) nbp + bz.  State on the device:
 *   table (nbp^3 int32, -1 = not evaluated) -> slot; bricks (slot -> id); vals (slots * 512 fp32, u = -sdf, local point
 *   lx << 6 | ly << 3 | lz); is_cell (nbp^3 bytes: the brick's cells are meshed; the other evaluated bricks are halo)
 * Call sequence (the host sizes buffers and runs the growth loop with ONE read of the two counts per pass):
 *   surf_band_screen   coarse lattice uc ((nbc+1)^3, nbc = ceil((res-1)/8), at lattice indices 0, 8, .., and res-1; cax/cay/caz
 *                      its axis values) -> mark[id] = 1 for the bricks whose corners change sign (u <= isovalue) or whose
 *                      min |u - isovalue| <= margin * (brick diagonal) / 2
 *   loop: surf_band_promote  marked bricks that are no cell bricks yet become ones (they stay marked); they and their forward
 *                      neighbours not in the table get need[id] = 1
 *         surf_compact(mark) -> new cell bricks, surf_compact(need) -> bricks to evaluate; stop when no new cell brick
 *         surf_band_assign  table slots for the bricks to evaluate (clears need) -> evaluate (surf_sdf_bricks_* or
 *                      surf_band_points + surf_sdf_mlp)
 *         surf_band_clear(new cell bricks, mark); surf_band_grow: every sign-changing edge of their cells marks the bricks of
 *                      the cells incident to it
 *   surf_band_classify -> flags (slots * 512 bytes) as surf_mc_classify's, for edges / cells of cell bricks only
 *   surf_compact(flags) -> pos; surf_band_keys -> int64 lattice keys (x res + y) res + z; sort them ascending;
 *   surf_band_rank     sorted keys -> pos (band positions); surf_mc_count(flags, pos) -> workspace, totals
 *   surf_band_emit     -> vertices / triangles as surf_mc_emit; vbase: slots * 512 int32 scratch
 * Vertex order: (owner lattice point, axis); triangle order: cell then table order - surf_mc_emit's.  res <= SURF_BAND_MAX_RES.
 */
#define SURF_BAND_MAX_RES 8192
int64_t surf_band_table_size(int res);
int surf_band_screen(const float* uc, const float* cax, const float* cay, const float* caz, int res, double isovalue, double margin,
                     uint8_t* mark, void* stream);
int surf_band_promote(uint8_t* mark, uint8_t* is_cell, const int32_t* table, uint8_t* need, int res, void* stream);
int surf_band_assign(const int32_t* ids, int64_t m, int32_t slot0, int32_t* table, int32_t* bricks, uint8_t* need, void* stream);
int surf_band_clear(const int32_t* ids, int64_t m, uint8_t* mark, void* stream);
int surf_band_grow(const float* vals, const int32_t* table, const uint8_t* is_cell, const int32_t* ids, int64_t m, int res,
                   double isovalue, uint8_t* mark, void* stream);
int surf_band_points(const float* ax, const float* ay, const float* az, const int32_t* bricks, int64_t m, int res, float* pts,
                     void* stream);
int surf_band_classify(const float* vals, const int32_t* table, const uint8_t* is_cell, const int32_t* bricks, int64_t n_slots,
                       int res, double isovalue, uint8_t* flags, void* stream);
int surf_band_keys(const int32_t* pos, int64_t m, const int32_t* bricks, int res, int64_t* keys, void* stream);
int surf_band_rank(const int64_t* keys, int64_t m, const int32_t* table, int res, int32_t* pos, void* stream);
int surf_band_emit(const float* vals, const int32_t* table, int res, double isovalue, const uint8_t* flags, const int64_t* keys,
                   const int32_t* pos, int64_t m, const int32_t* workspace, int32_t* vbase, double* vertices, int32_t* triangles,
                   void* stream);

/*
 * First-hit face ids of a triangle mesh from one pinhole view, by z-buffer rasterisation (mesh cleaning of the
 * evaluation: the faces some mask-pixel ray hits first; utils/clean_mesh.py:37-108 uses trimesh + pyembree for it).
 *   vertices (nv,3) fp32, faces (nf,3) int32 on the device; h_K (9) and h_w2c (12) HOST row-major; (h, w) the image the
 *   intrinsics refer to, (Hup, Wup) the sample lattice torch.linspace(0, w-1, Wup) x torch.linspace(0, h-1, Hup)
 *   zbuf (Hup*Wup) uint64 pre-filled with ~0: on return (depth bits << 32 | face id) of the nearest covering face
 * Rules: coverage is inclusive (a sample on an edge or a vertex belongs to every face that has it; faces of either winding are
 * drawn; a sample on or next to an edge that two faces share is covered by at least one of them); the nearest
 * perspective-correct depth wins, the smaller face id on an exact tie of the fp32 depth; near rule: a face with any vertex at
 * camera depth <= 1e-6 is not drawn at all (no near clipping); a face with a non-finite vertex or of zero screen area is
 * ignored.  Face indices are not checked against the vertex array.  SURF_E_ARG (nothing written) for a null pointer,
 * n_faces <= 0 or any of h, w, Hup, Wup < 2.
 */
int surf_raster_first_hit(const float* vertices, const int32_t* faces, int64_t n_faces, const float* h_K, const float* h_w2c,
                          int h, int w, int Hup, int Wup, unsigned long long* zbuf, void* stream);

/*
 * DTU Chamfer evaluation on the device (surf_amd/evaluation/dtu_eval.py, device="gpu"; dtu_eval.hip).  fp64 throughout, in
 * numpy's operation order; every output equals the numpy / scikit-learn evaluator's bit for bit.
 *   surf_dtu_sample_count / _write: sample_mesh_points' lattice samples of every triangle.  vertices (nv,3) fp64, triangles
 *     (n_tri,3) int64; counts (n_tri) int64 samples per triangle; out + 3*offsets[t] receives triangle t's samples, offsets
 *     the exclusive scan of counts (the caller places the vertices in front).
 *   surf_dtu_cell_keys: key (cx*ny + cy)*nz + cz of the cell floor((p - lo) / cell) of every point, clamped to the grid
 *     (nx, ny, nz <= 2^21; the thinning grid uses 2^21 on every axis, i.e. (cx << 42) | (cy << 21) | cz).
 *   surf_dtu_thin_round: one round of the parallel greedy thinning (downsample_points).  The n samples in cell order:
 *     sorted_points (n,3), sorted_index (n) their position in the shuffled order (ascending inside a cell), sorted_cell (n)
 *     their cell's position in cell_keys (n_cells distinct keys, ascending), cell_start (n_cells+1).  state (n, by shuffled
 *     position) 0 undecided / 1 kept / 2 removed, updated in place; *undecided is zeroed, then counts the samples still
 *     undecided.  Neighbours: (dx*dx + dy*dy) + dz*dz <= thresh*thresh.
 *   surf_dtu_nearest: out[q] = distance from queries[q] to the nearest of the reference points if < max_dist, else +inf.
 *     sorted_ref (r,3) in cell order of the dense (nx, ny, nz) grid of `cell` at lo, cell_start (nx*ny*nz + 1).
 */
int surf_dtu_sample_count(const double* vertices, const int64_t* triangles, int64_t n_tri, double thresh, int64_t* counts,
                          void* stream);
int surf_dtu_sample_write(const double* vertices, const int64_t* triangles, int64_t n_tri, double thresh, const int64_t* offsets,
                          double* out, void* stream);
int surf_dtu_cell_keys(const double* points, int64_t n, double lo_x, double lo_y, double lo_z, double cell, int64_t nx, int64_t ny,
                       int64_t nz, int64_t* keys, void* stream);
int surf_dtu_thin_round(const double* sorted_points, const int32_t* sorted_index, const int32_t* sorted_cell, const int64_t* cell_keys,
                        const int32_t* cell_start, int64_t n, int64_t n_cells, double thresh, int32_t* state, int32_t* undecided,
                        void* stream);
int surf_dtu_nearest(const double* queries, int64_t m, const double* sorted_ref, const int32_t* cell_start, double lo_x, double lo_y,
                     double lo_z, double cell, int64_t nx, int64_t ny, int64_t nz, double max_dist, double* out, void* stream);

/*
 * Mesh cleaning on the device (surf_amd/evaluation/clean_mesh.py, backend="device"; mesh_clean.hip).  Every stage returns what
 * the host stage returns.  These entry points were ADDED under SURF_ABI_VERSION 41 without a bump: the rule above is about
 * signatures that change, none did, and a library that lacks one of them is refused by name (surf_amd/_lib.py lib()).
 * Faces are (n,3) int32, masks uint8 (0 = unset), flags / keep arrays uint8, all on the device.  n_faces or n_vertices >= 2^31,
 * or a component table beyond 2^31 slots, is SURF_E_LIMIT.
 *   surf_clean_dilate: out = binary dilation of masks (n_views,h,w) with the disk dx*dx + dy*dy <= radius^2, outside unset.
 *   surf_clean_hull_count: n_seen[v] = number of views that see vertex v: in front of the camera, inside the image, and on a
 *     set texel of the view's mask under the four-texel bilinear footprint.  vertices (n,3) fp32; cams (n_views,21) fp32 on
 *     the DEVICE: K row-major (9) then inverse(c2w)[:3,:4] row-major (12).  The fp32 operation order is fixed and written out
 *     in mesh_clean.hip's header comment.
 *   surf_clean_face_keep: keep[f] = n_seen > min_nb_visible for the three vertices of f.
 *   surf_clean_mark_visible: seen[face] = 1 for every sample of surf_raster_first_hit's zbuf (Hup = h*upscale, Wup = w*upscale)
 *     that holds a hit and whose texel (i / upscale, j / upscale) of mask (h,w) is set; seen (n_faces) is not cleared.
 *   surf_clean_components: keep[f] = f shares an undirected edge with a face AND its edge-connected component has >= min_len
 *     faces (trimesh.graph.connected_components on face_adjacency; an edge of k faces joins all k).  Lock-free union-find over
 *     an edge hash table.  Work arrays, contents ignored: keys (slots) uint64, owner (slots) int32, shared (slots) uint8,
 *     edge_slot (3 n_faces) uint32, parent / size (n_faces) int32, has_nb (n_faces) uint8; slots = surf_clean_components_slots
 *     (n_faces) (< 0: SURF_E_*).  On return parent[f] is the smallest face id of f's component, size[parent[f]] its face count.
 *   surf_clean_mark_used: used[v] = 1 for the vertices of the faces with keep != 0 (used is not cleared).
 *   surf_clean_compact_faces: out[face_scan[f] - 1] = vertex_scan[faces[f]] - 1 for the kept faces (vertex_scan NULL: the ids
 *     unchanged); the scans are INCLUSIVE int64 prefix sums of keep and used.
 *   surf_clean_compact_rows: out[scan[i] - 1] = src[i] for rows of three elem_bytes (4 or 8) elements with flags[i] != 0.
 */
int surf_clean_dilate(const uint8_t* masks, int n_views, int h, int w, int radius, uint8_t* out, void* stream);
int surf_clean_hull_count(const float* vertices, int64_t n_vertices, const uint8_t* masks, const float* cams, int n_views, int h,
                          int w, int32_t* n_seen, void* stream);
int surf_clean_face_keep(const int32_t* n_seen, const int32_t* faces, int64_t n_faces, int min_nb_visible, uint8_t* keep,
                         void* stream);
int surf_clean_mark_visible(const unsigned long long* zbuf, int Hup, int Wup, const uint8_t* mask, int h, int w, int upscale,
                            int64_t n_faces, uint8_t* seen, void* stream);
int64_t surf_clean_components_slots(int64_t n_faces);
int surf_clean_components(const int32_t* faces, int64_t n_faces, int64_t min_len, unsigned long long* keys, int32_t* owner,
                          uint8_t* shared, int64_t slots, uint32_t* edge_slot, int32_t* parent, uint8_t* has_nb, int32_t* size,
                          uint8_t* keep, void* stream);
int surf_clean_mark_used(const int32_t* faces, const uint8_t* keep, int64_t n_faces, int64_t n_vertices, uint8_t* used,
                         void* stream);
int surf_clean_compact_faces(const int32_t* faces, const uint8_t* keep, const int64_t* face_scan, const int64_t* vertex_scan,
                             int64_t n_faces, int64_t n_vertices, int32_t* out, void* stream);
int surf_clean_compact_rows(const void* src, int elem_bytes, const uint8_t* flags, const int64_t* scan, int64_t n, void* out,
                            void* stream);

/*
 * The DTU evaluation protocol's mesh cleaner on the device (surf_amd/evaluation/clean_dtu.py, backend="device"; dtu_clean.hip).
 * Every stage returns what the host stage returns.  Added under SURF_ABI_VERSION 41 without a bump, like the entry points above.
 * Compaction by vertex flag goes through surf_clean_compact_rows / surf_clean_compact_faces; the frustum stage through
 * surf_raster_first_hit, surf_clean_mark_visible and surf_clean_components.
 *   surf_dtu_clean_dilate: out = maximum of masks (n_views,h,w) uint8 over a footprint of k rows (k odd, <= 64: SURF_E_LIMIT
 *     beyond) given as half_widths (k) int32 on the DEVICE: row i covers columns [-half_widths[i], half_widths[i]] of image row
 *     y + i - k/2 (negative: empty row).  Pixels outside the image do not contribute.
 *   surf_dtu_clean_points_in_masks: count[v] = number of views whose padded mask is set at the rounded projection of vertex v.
 *     vertices (n,3) float64; dilated (n_views,h,w) uint8, set where > 128; proj (n_views,12) fp32 on the DEVICE: the first
 *     three rows of K4 @ E, row-major.  The one-pixel ring of ones around the mask is arithmetic.  The float64 operation order
 *     is fixed and written out in dtu_clean.hip's header comment.
 *   surf_dtu_clean_keep: vertex_keep[v] = count[v] > minimal_vis; face_keep[f] = the three vertices of f are kept (an index
 *     outside [0, n_vertices) drops the face).  n_faces may be 0 (faces / face_keep then unused).
 */
int surf_dtu_clean_dilate(const uint8_t* masks, int n_views, int h, int w, const int32_t* half_widths, int k, uint8_t* out,
                          void* stream);
int surf_dtu_clean_points_in_masks(const double* vertices, int64_t n_vertices, const uint8_t* dilated, const float* proj,
                                   int n_views, int h, int w, int32_t* count, void* stream);
int surf_dtu_clean_keep(const int32_t* count, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int minimal_vis,
                        uint8_t* vertex_keep, uint8_t* face_keep, void* stream);

/*
 * Per-scene fine-tuning: the ray batch of one view made on the device (surf_amd/datasets/dtu_finetune.py after .to(device);
 * finetune_rays.hip).  Added under SURF_ABI_VERSION 41 without a bump, like the mesh-cleaning entry points above: nothing
 * existing changes signature, and a library that lacks them is refused by name.
 *   surf_finetune_rays: one ray per pixel coordinate of ONE view.  px / py (n_rays) on the device, fp32 (coords_int32 == 0) or
 *     int32 (!= 0; converted to fp32, exact); kinv (9) = inverse(K)[:3,:3] and c2w (12) = c2w[:3,:4], row-major fp32 on the
 *     DEVICE; image (h,w,3) and depth (h,w) fp32 on the device.  rays_o / rays_d / color (n_rays,3), pseudo_depth (n_rays) or
 *     NULL (then depth may be NULL too).  color and pseudo_depth are copies of the texel at (long(py), long(px)) (truncation);
 *     a pixel outside the image yields zeros.  The fp32 operation order of the directions is fixed and written out in
 *     finetune_rays.hip's header comment.
 *   surf_finetune_gather_pts: out[i] = pts[idx[i]], rows of three fp32; idx (n) int32; an index outside [0, n_pts) yields zeros.
 */
int surf_finetune_rays(const void* px, const void* py, int coords_int32, int64_t n_rays, const float* kinv, const float* c2w,
                       const float* image, const float* depth, int h, int w, float* rays_o, float* rays_d, float* color,
                       float* pseudo_depth, void* stream);
int surf_finetune_gather_pts(const float* pts, int64_t n_pts, const int32_t* idx, int64_t n, float* out, void* stream);

/*
 * Generalisation training: the batch of one item written on the device from the device-resident DTU training set
 * (surf_amd/datasets/dtu_resident.py; train_batch.hip).  Added under SURF_ABI_VERSION 41 without a bump, like the entry points
 * above.  The cache holds uint8 texels (h,w,3), uint8 0/1 masks (h,w) and UNSCALED fp32 depth maps (h,w) on the device;
 * scaled(d) = (float)((double)d * scale), the rounding of the host reader's `fp32 array * float64 scalar` cast back to fp32.
 *   surf_train_views: h_images: HOST array of n_views (<= SURF_MAX_VIEWS) device pointers, one image per view slot (a pointer may
 *     repeat); h_masks / h_depths / h_pseudos: HOST arrays of two device pointers each, the maps of the reference view and of the
 *     supervised source view (the two may be the same view).  Image and mask pointers 4-byte aligned.  Outputs: imgs
 *     (n_views,3,h,w) = texel / 256; mask_out (2,h,w) = (float)mask; depth_out / pseudo_out (2,h,w) = scaled(map).  Any h, w.
 *   surf_train_rays: n_rays rays of the reference view, the n_rays - n_rays / 4 pixels inside its mask first: ray t takes pixel
 *     inside[pick[t]] (inside: n_inside row-major flat indices y w + x on the device, n_inside <= h w; pick: int32 on the device),
 *     the last n_rays / 4 rays the pixels (free_x[i], free_y[i]) (int32 on the device; may be NULL when n_rays < 4).  h_kinv (9) =
 *     inverse(K)[:3,:3] and h_c2w (12) = c2w[:3,:4] of the reference camera, row-major fp32 on the HOST.  Outputs: pixels_x,
 *     pixels_y (n_rays) = the coordinates as fp32; rays_o, rays_d, color (n_rays,3); depth_out, pseudo_out, mask_out (n_rays).
 *     color = texel / 256, depth_out / pseudo_out = scaled(map texel), mask_out = (float)mask texel.  A pixel outside the image
 *     keeps its coordinates and rays and yields zeros for the four gathered entries; a pick outside [0, n_inside) yields zeros
 *     in every output.  The fp32 operation order of the directions is surf_finetune_rays' and is restated in train_batch.hip's
 *     header comment.  n_rays <= 2^24.
 */
int surf_train_views(const uint8_t* const* h_images, int n_views, int h, int w, const uint8_t* const* h_masks,
                     const float* const* h_depths, const float* const* h_pseudos, double scale, float* imgs, float* mask_out,
                     float* depth_out, float* pseudo_out, void* stream);
int surf_train_rays(const int32_t* pick, const int32_t* free_x, const int32_t* free_y, int n_rays, const int32_t* inside,
                    int64_t n_inside, const float* h_kinv, const float* h_c2w, const uint8_t* image, const uint8_t* mask,
                    const float* depth, const float* pseudo, double scale, int h, int w, float* pixels_x, float* pixels_y,
                    float* rays_o, float* rays_d, float* color, float* depth_out, float* pseudo_out, float* mask_out, void* stream);

/*
 * Per-vertex mesh attributes (ImplicitSurface.vertex_attributes; vertex_attrs.hip): the stages around the SDF gradient and blend
 * kernels, which run unchanged over a mesh's vertex list.  Added under SURF_ABI_VERSION 41 without a bump, like the entry
 * points above.  n >= 2^31 is SURF_E_LIMIT.
 *   surf_vertex_points: vertices (n,3) on the device, float64 (is_f64 != 0; converted by round-to-nearest-even, as
 *     torch.Tensor.float()) or fp32 (copied) -> pts (n,3) fp32 and idx (n) int32 = 0 .. n-1, the index list surf_sdf_mlp* and
 *     surf_blend* take.
 *   surf_vertex_finish: grad (n,3), color (n,3) fp32 and n_valid (n) uint8 -> normals (n,3) fp32 = grad / |grad| ((0,0,0) where
 *     |grad| is zero or not finite) and colors (n,3) uint8 = trunc(clamp(color * 256, 0, 255)), (128,128,128) where n_valid is 0.
 *     The fp32 operation order is fixed and written out in vertex_attrs.hip's header comment.
 */
int surf_vertex_points(const void* vertices, int is_f64, int64_t n, float* pts, int32_t* idx, void* stream);
int surf_vertex_finish(const float* grad, const float* color, const uint8_t* n_valid, int64_t n, float* normals, uint8_t* colors,
                       void* stream);

/*
 * Depth-map fusion (surf_amd/fusion.py; fuse.hip): truncated-signed-distance integration of the depth maps rendered for many
 * reference views into one world-frame lattice, and the mesh taken from it.  Added under SURF_ABI_VERSION 41 without a bump, like
 * the entry points above.  State: tsdf, weight (nx,ny,nz) fp32, z contiguous (the layout surf_mc_* read), color (nx,ny,nz,3) fp32 or
 * NULL; the lattice points are (ax[i], ay[j], az[k]) (device arrays of nx / ny / nz coordinates, any spacing).  More lattice points
 * than 2^31 - 1 blocks of 256, nx > 65535, ny nz >= 2^31, or a depth map of 2^31 / 3 pixels or more, is SURF_E_LIMIT.
 *   surf_fuse_integrate: updates the state in place with n_views (<= SURF_FUSE_MAX_VIEWS: SURF_E_LIMIT beyond) depth views in ONE
 *     launch, in the order given.  HOST arrays: h_P (n_views,12) fp32, row-major 3x4 world -> (x z, y z, z) with z in world units
 *     and x, y in depth-map pixel indices; h_depths / h_images: n_views device pointers to the depth maps (H,W) fp32 and the images
 *     (H,W,3) fp32 (h_images is read only when color != NULL); h_hw (n_views,2) = (H, W); h_dscale (n_views): depth units -> world
 *     units.  trunc > 0: the truncation distance in world units.  A point's update by one view is a running mean with weight 1 per
 *     observation of min((d - z) / trunc, 1), skipped where the point is behind the camera, projects (rounded to the nearest pixel)
 *     outside the map, meets no measurement (d <= 0, NaN, inf) or lies further than trunc behind it.  The fp32 operation order is
 *     fixed and written out in fuse.hip's header comment.
 *   surf_fuse_lattice: u (n) = -tsdf where weight > 0, NaN elsewhere: marching cubes' input (surf_mc_classify_observed).
 *   surf_fuse_vertex_colors: out (n_vertices,3) uint8 = the colour lattice interpolated along the lattice edge each vertex lies on;
 *     vertices (n_vertices,3) float64 in lattice-index units (surf_mc_emit's), quantised like surf_vertex_finish's colours.  The
 *     operation order is written out in fuse.hip's header comment.
 *   surf_mc_classify_observed (mcubes.hip): surf_mc_classify for a lattice with unobserved (non-finite) points.  An edge bit is
 *     set only where both end points are finite, a cell's triangle count only where its eight corners are; surf_mc_count and
 *     surf_mc_emit run unchanged on these flags.  (surf_mc_classify reads a NaN as "outside": observed free space, which is
 *     "inside", would be closed by a sheet wherever it borders unobserved points - frustum sides, dropped pixels.)  Vertices on an
 *     edge none of whose cells is fully observed are emitted but referenced by no triangle.
 */
#define SURF_FUSE_MAX_VIEWS 16
int surf_fuse_integrate(float* tsdf, float* weight, float* color, const float* ax, const float* ay, const float* az, int nx, int ny,
                        int nz, const float* h_P, const float* const* h_depths, const float* const* h_images, const int* h_hw,
                        const float* h_dscale, int n_views, float trunc, void* stream);
int surf_mc_classify_observed(const float* u, int nx, int ny, int nz, double isovalue, uint8_t* flags, void* stream);
int surf_fuse_lattice(const float* tsdf, const float* weight, int64_t n, float* u, void* stream);
int surf_fuse_vertex_colors(const double* vertices, int64_t n_vertices, const float* color, int nx, int ny, int nz, uint8_t* out,
                            void* stream);

/*
 * Brick-sparse depth-map fusion (surf_amd/fusion.py FusionVolume(sparse=True); fuse_sparse.hip): the state of surf_fuse_* kept only
 * in the 8^3-point bricks that can carry a triangle, so that lattices of 2^31 points and more can be fused and meshed.  Added under
 * SURF_ABI_VERSION 41 without a bump, like the entry points above.  The lattice (nx,ny,nz) is embedded in the cube of side
 * res = max(nx,ny,nz) (2 <= res, res <= SURF_BAND_MAX_RES: SURF_E_LIMIT beyond) and uses the band layout above: table
 * (surf_band_table_size(res) int32, -1 = not allocated), bricks (slot -> id, ascending ids), state tsdf / weight (n_slots * 512)
 * and color (n_slots * 512, 3) fp32, brick-major.  The axes must be strictly increasing.  n_slots * 512 >= 2^31 is SURF_E_LIMIT.
 * Call sequence:
 *   surf_fuse_mark_bricks      once per view, ALL views before the first integration: mark[id] = 1 for every brick that can hold a
 *                              point the view updates with less than the truncation distance, or a lattice neighbour of one.
 *                              HOST h_lift (12) fp32 = M^-1 (row-major) then -M^-1 t of the view's P = [M | t], formed in float64
 *                              and rounded once.  The rule and its fp32 operation order: fuse_sparse.hip's header comment.
 *   surf_compact(mark) -> ids; surf_band_assign(ids, m, 0, table, bricks, mark)
 *   surf_fuse_integrate_bricks surf_fuse_integrate over every point of the listed bricks, the same per-point arithmetic: the state
 *                              equals the dense lattice's there, bit for bit.  Points past the upper faces are never updated.
 *   surf_fuse_lattice          on the flat state -> vals (u = -tsdf where weight > 0, NaN elsewhere)
 *   surf_band_classify_observed  surf_mc_classify_observed's flags for every band point, values read through the table (a missing
 *                              brick reads NaN); then surf_compact / surf_band_keys / sort / surf_band_rank / surf_mc_count /
 *                              surf_band_emit with res as above.  For an isovalue in (-1, 1) the mesh is the dense one, array for array.
 *   surf_fuse_vertex_colors_bricks  surf_fuse_vertex_colors with the colour reads going through the table.
 */
int surf_fuse_mark_bricks(const float* depth, int H, int W, float dscale, const float* h_lift, const float* ax, const float* ay,
                          const float* az, int nx, int ny, int nz, float trunc, uint8_t* mark, void* stream);
int surf_fuse_integrate_bricks(float* tsdf, float* weight, float* color, const int32_t* bricks, int64_t n_slots, const float* ax,
                               const float* ay, const float* az, int nx, int ny, int nz, const float* h_P,
                               const float* const* h_depths, const float* const* h_images, const int* h_hw, const float* h_dscale,
                               int n_views, float trunc, void* stream);
int surf_band_classify_observed(const float* vals, const int32_t* table, const int32_t* bricks, int64_t n_slots, int nx, int ny,
                                int nz, double isovalue, uint8_t* flags, void* stream);
int surf_fuse_vertex_colors_bricks(const double* vertices, int64_t n_vertices, const float* color, const int32_t* table, int nx,
                                   int ny, int nz, uint8_t* out, void* stream);

/*
 * Ray casting of the fused state (surf_amd/fusion.py FusionVolume.ray_cast; ray_cast.hip): per pixel of an (H,W) image of any camera
 * the first front-to-inside crossing of tsdf = level along the pixel's ray, found by a cell-by-cell walk of the lattice over the cells
 * whose eight corners are observed (weight > 0; in the brick layout a corner of an unallocated brick is unobserved) and refined by a
 * fixed number of evaluations of the cell's trilinear interpolant.  Added under SURF_ABI_VERSION 41 without a bump, like the entry
 * points above.  The lattice must be uniform; the rule and its fp32 operation order are written out in ray_cast.hip's header comment,
 * and the two entry points return equal arrays on a dense and a brick-sparse state of the same views.
 *   HOST h_lift (12) fp32, in lattice-index units: M^-1 / voxel (row-major), then (-M^-1 t - lo) / voxel of the camera P = [M | t]
 *     (world -> (x z, y z, z)) and the lattice world = lo + voxel * index, formed in float64 and rounded once.
 *   z_min >= 0: rays start at z-depth z_min.  level = -isovalue in (-1, 1).
 *   depth (H,W): z-depth in world units of the crossing, 0 where there is none.  normal (H,W,3) or NULL: the normalised gradient of the
 *     interpolant there, world frame, pointing into free space; 0 where there is no hit.  out_color (H,W,3): the colour state
 *     interpolated in the same cell; given exactly when color is (SURF_E_ARG otherwise).  Every pixel is written.
 *   H W == 0 succeeds without a launch.  SURF_E_LIMIT: the limits of surf_fuse_integrate (surf_fuse_ray_cast) or of
 *     surf_fuse_integrate_bricks (surf_fuse_ray_cast_bricks), an axis, H or W above 2^24, H W >= 2^31.
 */
int surf_fuse_ray_cast(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz, const float* h_lift,
                       int H, int W, float z_min, float level, float* depth, float* normal, float* out_color, void* stream);
int surf_fuse_ray_cast_bricks(const float* tsdf, const float* weight, const float* color, const int32_t* table, int64_t n_slots,
                              int nx, int ny, int nz, const float* h_lift, int H, int W, float z_min, float level, float* depth,
                              float* normal, float* out_color, void* stream);

/*
 * Multi-view geometric consistency of depth maps (surf_amd/fusion.py filter_views; depth_filter.hip): which pixels of a reference
 * depth map do enough other views agree with?  A pixel is lifted with its depth, projected into a source view, the source's depth
 * is read there (bilinear over four MEASURED taps), the source point is projected back, and the source agrees when the round trip
 * ends within px_thresh pixels of the pixel and within rel_thresh (relative) of its depth.  Added under SURF_ABI_VERSION 41
 * without a bump, like the entry points above.  A depth that is 0, negative, NaN or inf is no measurement, as in surf_fuse_*.
 *   surf_depth_consistency: ONE launch tests the reference map depth_r (H,W) fp32 (dscale_r: depth units -> world units) against
 *     n_sources (<= SURF_FUSE_MAX_VIEWS: SURF_E_LIMIT beyond) source maps, in the order given, one thread per reference pixel.
 *     HOST arrays: h_T (n_sources,24) fp32 = per source A_rs (3x3 row-major), b_rs (3), A_sr (3x3), b_sr (3) with
 *     A_rs = M_s M_r^-1, b_rs = t_s - A_rs t_r for P = [M | t] (formed in float64, rounded once: fusion.pair_transforms);
 *     h_depths: n_sources device pointers to the source maps (Hs,Ws) fp32; h_hw (n_sources,2) = (Hs, Ws); h_dscale (n_sources).
 *     px2 = px_thresh^2 (fp32), rel_thresh: the two thresholds.  count (H,W) int32 and zsum (H,W) fp32 are READ AND WRITTEN: at a
 *     measured pixel count grows by one and zsum by the back-projected depth per agreeing source, so more than 16 sources are
 *     further launches with identical results; pixels the launch does not change are not written.  tile_w: the pixels one
 *     wavefront covers, 64 = 64 consecutive pixels of the flat row-major index, 16 = a 16 x 4 tile, 8 = an 8 x 8 tile (a choice of
 *     speed only: the results are the same; other values are SURF_E_ARG).  A map of 2^31 pixels or more, a map side above 2^24
 *     (its largest index is no exact float) or more than 65535 rows of 8-pixel tiles is SURF_E_LIMIT.
 *   surf_depth_consistency_finish: n pixels -> out_depth (n) fp32 and keep (n) uint8.  keep = measured and count >= min_consistent;
 *     out_depth = 0 where not kept, depth_r unchanged where kept, or with average != 0 the mean over the reference and its
 *     agreeing sources ((zsum + d) / (count + 1)) / dscale_r.
 * The fp32 operation order of both is fixed and written out in depth_filter.hip's header comment.
 */
int surf_depth_consistency(const float* depth_r, int H, int W, float dscale_r, const float* h_T, const float* const* h_depths,
                           const int* h_hw, const float* h_dscale, int n_sources, float px2, float rel_thresh, int32_t* count,
                           float* zsum, int tile_w, void* stream);
int surf_depth_consistency_finish(const float* depth_r, float dscale_r, const int32_t* count, const float* zsum, int64_t n,
                                  int min_consistent, int average, float* out_depth, uint8_t* keep, void* stream);

/*
 * Fused point clouds (surf_amd/fusion.py fuse_points; point_cloud.hip): the depth maps of many views merged into one cloud with one
 * point per surface sample.  Views are visited in index order; a pixel that is measured, not yet used and agreed with by at least
 * min_consistent sources (the rule of surf_depth_consistency) is emitted, and the pixel it lands on in every agreeing source is
 * marked used, so that it is not emitted again.  Added under SURF_ABI_VERSION 41 without a bump, like the entry points above.
 * used maps are (H,W) uint8, 0 or 1.  Per view the caller runs surf_points_candidates, surf_depth_consistency (+ _finish) on the
 * candidates, surf_points_mark per chunk of sources, and surf_points_lift on the ordered list of kept pixels, all on one stream.
 * Empty work (no pixels, no sources, no kept pixels) returns 0 at once: no zero-sized grid is launched.  A map of 2^31 pixels or
 * more or a map side above 2^24 is SURF_E_LIMIT, as for surf_depth_consistency.
 *   surf_points_candidates: out (n) = 0 where used != 0, depth elsewhere: a used pixel is no measurement as a reference.
 *   surf_points_mark: ONE launch re-runs the rule at the pixels of the reference map cand_r (H,W) with keep != 0 against n_sources
 *     (<= SURF_FUSE_MAX_VIEWS: SURF_E_LIMIT beyond) sources - h_T, h_depths, h_hw, h_dscale, px2, rel_thresh as for
 *     surf_depth_consistency - and stores 1 at h_used[s][rintf(sy), rintf(sx)] (HOST array of n_sources device pointers to the
 *     sources' used maps (Hs,Ws)) for every agreeing source s; (sx, sy) is the pixel's projection into s, inside the map by the
 *     rule.  No h_used[s] may be the reference's own map.
 *   surf_points_lift: kept (n_kept) int64 = the flat row-major indices of the kept pixels, ascending.  Per kept pixel k:
 *     z = average ? (zsum + d) / (count + 1) : d with d = cand_r * dscale_r; points (n_kept,3) fp32 = Minv (x z, y z, z) + c with
 *     HOST h_lift (12) fp32 = Minv = M^-1 (3x3 row-major) then c = -M^-1 t for P = [M | t] (formed in float64, rounded once);
 *     colors (n_kept,3) uint8 = image (H,W,3) fp32 at the pixel, quantised like surf_fuse_vertex_colors (image NULL: colors is
 *     not written); origin (n_kept,2) int32 = (view, flat pixel index).  An index outside the map writes nothing.
 * The fp32 operation order is fixed and written out in point_cloud.hip's header comment.
 */
int surf_points_candidates(const float* depth, const uint8_t* used, int64_t n, float* out, void* stream);
int surf_points_mark(const float* cand_r, int H, int W, float dscale_r, const uint8_t* keep, const float* h_T,
                     const float* const* h_depths, uint8_t* const* h_used, const int* h_hw, const float* h_dscale, int n_sources,
                     float px2, float rel_thresh, void* stream);
int surf_points_lift(const float* cand_r, int H, int W, float dscale_r, const int32_t* count, const float* zsum, int average,
                     const int64_t* kept, int64_t n_kept, const float* h_lift, const float* image, int view, float* points,
                     uint8_t* colors, int32_t* origin, void* stream);

/*
 * Tanks and Temples / ETH3D F-score evaluation on the device (surf_amd/evaluation/fscore.py, device="gpu"; fscore.hip).  fp64
 * throughout, in the host path's operation order: the transform, the crop, the voxel means and the nearest distances / indices
 * equal the numpy / scikit-learn path's arrays.  Added under SURF_ABI_VERSION 41 without a bump, like the entry points above.
 * Points are (n,3) fp64 on the device; n >= 2^31 (int32 point indices) or a grid of more than 2^21 cells along an axis is
 * SURF_E_LIMIT, never a wrapped index.
 *   surf_fscore_transform: out = R p + t with HOST h_T (16) fp64, a row-major 4x4 whose last row is not read:
 *     out[k] = ((R[k,0]*x + R[k,1]*y) + R[k,2]*z) + t[k].  out must not overlap points.
 *   surf_fscore_crop: keep (n) uint8 = axis_min <= p[axis] <= axis_max and p inside polygon (n_polygon >= 3 vertices, (n_polygon,2)
 *     fp64 on the DEVICE: the coordinates (u, v) along the two other axes in increasing order) by the crossing number over the
 *     edges (i, j = i - 1): ((v_i > v) != (v_j > v)) and u < (u_j - u_i) * (v - v_i) / (v_j - v_i) + u_i.
 *   surf_fscore_voxel_keys: keys[i] = (cx << 42) | (cy << 21) | cz of the cell floor((p - origin) / voxel), origin = h_lo - voxel/2,
 *     with HOST h_lo (3), h_hi (3) the per-axis minimum and maximum of the points (Open3D's voxel_down_sample grid); a box that
 *     needs more than 2^21 cells along an axis is SURF_E_LIMIT.
 *   surf_fscore_voxel_mean: out (n_voxels,3) = per voxel the sum of its members, added one after the other in the order given,
 *     divided by their number.  order (n) int64 = the points' indices sorted by key (a STABLE sort: input order inside a voxel),
 *     segment_start (n_voxels+1) int64 = the first position of every voxel in order.  A voxel may hold any number of points.
 *   surf_fscore_nearest: surf_dtu_nearest that also reports WHICH point: sorted_index (r) int32 = the index in the caller's order of
 *     every row of sorted_ref; index (m) int64 = that of the nearest reference point, -1 where out is +inf.  Equal squared
 *     distances go to the smaller index.
 *   surf_fscore_icp_sums / _cov: the two reductions of one point-to-point ICP step over the pairs (source[i], target[index[i]]),
 *     index[i] in [0, n_target) (any other value: no pair).  _sums: out (8) = [pairs, sum of source (3), sum of target (3), sum of
 *     dist*dist]; _cov: out (9) row-major H[r][c] = sum (source[r] - cs[r]) * (target[c] - ct[c]) with HOST h_centroids (6) =
 *     cs then ct.  partials: device scratch of SURF_FSCORE_ICP_SLOTS * 9 fp64.  Workgroup w of min(ceil(n / 256),
 *     SURF_FSCORE_ICP_SLOTS) writes its sums to slot w, then one workgroup adds the slots in slot order: no float atomics, the same
 *     bits on every run.
 */
#define SURF_FSCORE_ICP_SLOTS 1024
int surf_fscore_transform(const double* points, int64_t n, const double* h_T, double* out, void* stream);
int surf_fscore_crop(const double* points, int64_t n, int axis, double axis_min, double axis_max, const double* polygon, int n_polygon,
                     uint8_t* keep, void* stream);
int surf_fscore_voxel_keys(const double* points, int64_t n, const double* h_lo, const double* h_hi, double voxel, int64_t* keys,
                           void* stream);
int surf_fscore_voxel_mean(const double* points, int64_t n, const int64_t* order, const int64_t* segment_start, int64_t n_voxels,
                           double* out, void* stream);
int surf_fscore_nearest(const double* queries, int64_t m, const double* sorted_ref, const int32_t* sorted_index,
                        const int32_t* cell_start, double lo_x, double lo_y, double lo_z, double cell, int64_t nx, int64_t ny, int64_t nz,
                        double max_dist, double* out, int64_t* index, void* stream);
int surf_fscore_icp_sums(const double* source, const double* target, int64_t n_target, const int64_t* index, const double* dist,
                         int64_t n, double* partials, double* out, void* stream);
int surf_fscore_icp_cov(const double* source, const double* target, int64_t n_target, const int64_t* index, int64_t n,
                        const double* h_centroids, double* partials, double* out, void* stream);

/*
 * Mesh simplification by vertex clustering with quadric placement (surf_amd/mesh_simplify.py, backend="device";
 * mesh_simplify.hip).  Added under SURF_ABI_VERSION 41 without a bump, like the entry points above.  The device path returns the
 * host path's arrays: both follow the rule below, fp64 with separate multiplies and adds (-ffp-contract=off), every sum of more
 * than two terms parenthesised from the left.
 *
 * THE RULE.  vertices (n,3) fp32, faces (m,3) int32, optional normals (n,3) fp32 and colors (n,3) uint8, cell > 0 (fp64).
 *   1. cell of a vertex: i[a] = floor(double(v[a]) / cell); the lattice is anchored at the world origin.  key = ((ix + 2^20) << 42)
 *      | ((iy + 2^20) << 21) | (iz + 2^20).  A non-finite coordinate or an index outside [-2^20, 2^20) is SURF_E_LIMIT.
 *      centre[a] = (double(i[a]) + 0.5) * cell.
 *   2. per face (p = double(v[faces[f]])): e1 = p1 - p0, e2 = p2 - p0, c = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x),
 *      L = sqrt((cx*cx + cy*cy) + cz*cz).  A face with L == 0, a non-finite L or a repeated index contributes nothing.  Otherwise
 *      nrm = c / L, w = (L / 2) / (cell*cell), and for each corner k with the centre of ITS vertex's cell: q = (p0 - centre) / cell,
 *      d = (nx*qx + ny*qy) + nz*qz, g = w * nrm, and the cell receives  A00 += gx*nx  A01 += gx*ny  A02 += gx*nz  A11 += gy*ny
 *      A12 += gy*nz  A22 += gz*nz  b[a] += (w*d) * nrm[a].  A face inside one cell is added three times.
 *   3. per vertex, referenced or not, to its cell: count += 1, u[a] += (double(v[a]) - centre[a]) / cell, colour sums (integers),
 *      normal sums (fp64 of the fp32 values).
 *   4. accumulation: SEQUENTIAL, the order is part of the rule (the int64 fixed-point alternative was not taken).  Inside a cell the
 *      face terms are added in (face index, corner) order and the vertex terms in vertex-index order, each sum starting from +0:
 *      the caller sorts the corners / the vertices by cell with a STABLE sort and one thread walks a cell's two segments, as
 *      surf_fscore_voxel_mean does.  np.add.at walks the same order on the host.  No float atomics.
 *   5. representative: t = (A00 + A11) + A22, mean[a] = u[a] / double(count), s = 2^-20 * t.  If not t > 0: x = mean.  Otherwise
 *      (A + s I) x = b + s mean by LDL^T without pivoting (the matrix is symmetric positive definite, pivots >= s), written out:
 *        m00 = A00 + s   m11 = A11 + s   m22 = A22 + s   r[a] = b[a] + s * mean[a]
 *        l10 = A01 / m00          l20 = A02 / m00
 *        d1  = m11 - l10 * A01    u21 = A12 - l20 * A01    l21 = u21 / d1    d2 = (m22 - l20 * A02) - l21 * u21
 *        y1  = r1 - l10 * r0      y2  = (r2 - l20 * r0) - l21 * y1
 *        x2  = y2 / d2            x1  = y1 / d1 - l21 * x2                   x0 = (r0 / m00 - l10 * x1) - l20 * x2
 *      then x[a] = min(max(x[a], -0.5), 0.5) and position[a] = float(centre[a] + x[a] * cell).
 *   6. colour = (2 sum + count) / (2 count) in integers (rounded to nearest, halves up).  normal = float(S[a] / len) with
 *      len = sqrt((Sx*Sx + Sy*Sy) + Sz*Sz), or (0,0,0) when len is 0 or not finite.
 *   7. faces: every index is replaced by its vertex's cell.  A face with fewer than three distinct cells is dropped.  Of the faces
 *      with the same set of three cells, in any orientation, the one of lowest input index is kept.  Kept faces stay in input order
 *      with their own orientation.
 *   8. output vertices: the cells that a kept face references, numbered in ascending key.  vertex_map (n) int32 = the output index
 *      of every input vertex's cell, or -1.
 *
 * Entry points, in the order surf_amd.ops.simplify_mesh calls them (sorts, scans and searches between them are the caller's):
 *   surf_simplify_keys: keys (n) int64 of rule 1.  A vertex that breaks rule 1's limit gets key 0 and sets flag[0] = 1 (int32 on the
 *     device, zeroed by the caller): a launch cannot return it, so the CALLER reads the flag before it goes on and reports
 *     SURF_E_LIMIT.  !(cell > 0), or a cell whose square is 0 or not finite, is SURF_E_ARG.
 *   surf_simplify_segments: from sorted_keys / order (n) int64 (the keys' stable ascending sort and its permutation) and rank (n)
 *     int64 (rank[j] = number of distinct keys among sorted_keys[0..j], minus 1): vertex_cell[order[j]] = rank[j] (n) int32 and
 *     segment_start (n_cells + 1) int64, the first position of every cell in order, segment_start[n_cells] = n.
 *   surf_simplify_face_cells: face_cells (m,3) int32 = vertex_cell[faces]; a face with an index outside [0, n) gets (0,0,0) (it is
 *     dropped by rule 7 and skipped by rule 2) and sets flag[0] = 1.
 *   surf_simplify_faces: rule 7.  keep (m) uint8.  owner (slots) int32 and face_slot (m) uint32 are scratch; slots is the smallest
 *     power of two >= max(1024, 2 m) (SURF_E_ARG otherwise).  One table slot per set of cells (open addressing, linear probing; a
 *     slot is claimed by atomicCAS with a face id and compared through that face's cells), one atomicMin of the face id per face.
 *   surf_simplify_mark_used: used (n_cells) uint8, zeroed by the caller, = 1 for the cells of the kept faces.
 *   surf_simplify_cells: rules 2-6, one thread per cell; a used cell c writes row cell_scan[c] - 1 of out_vertices (fp32),
 *     out_normals (fp32, with normals) and out_colors (uint8, with colors).  corner_order (3 m) int64 = the stable ascending sort
 *     permutation of face_cells read as a flat array, corner_start (n_cells + 1) int64 the first position of every cell in it;
 *     vertex_order / vertex_start = order / segment_start above; cell_scan (n_cells) int64 = the INCLUSIVE scan of used.
 *   surf_simplify_compact: out_faces (kept faces, 3) int32 with row face_scan[f] - 1 = cell_scan[face_cells[f]] - 1 for the kept
 *     faces (face_scan the INCLUSIVE scan of keep), and vertex_map (n) int32 of rule 8.
 * n == 0 or m == 0 returns 0 at once where there is nothing to do; n, m >= 2^31 / 3 is SURF_E_LIMIT.
 */
int surf_simplify_keys(const float* vertices, int64_t n, double cell, int64_t* keys, int32_t* flag, void* stream);
int surf_simplify_segments(const int64_t* sorted_keys, const int64_t* order, const int64_t* rank, int64_t n, int64_t n_cells,
                           int32_t* vertex_cell, int64_t* segment_start, void* stream);
int surf_simplify_face_cells(const int32_t* faces, int64_t m, const int32_t* vertex_cell, int64_t n, int32_t* face_cells,
                             int32_t* flag, void* stream);
int surf_simplify_faces(const int32_t* face_cells, int64_t m, int32_t* owner, int64_t slots, uint32_t* face_slot, uint8_t* keep,
                        void* stream);
int surf_simplify_mark_used(const int32_t* face_cells, const uint8_t* keep, int64_t m, int64_t n_cells, uint8_t* used,
                            void* stream);
int surf_simplify_cells(const float* vertices, const float* normals, const uint8_t* colors, int64_t n, const int32_t* faces,
                        int64_t m, double cell, const int64_t* sorted_keys, const int64_t* vertex_order,
                        const int64_t* vertex_start, const int64_t* corner_order, const int64_t* corner_start, int64_t n_cells,
                        const uint8_t* used, const int64_t* cell_scan, float* out_vertices, float* out_normals,
                        uint8_t* out_colors, void* stream);
int surf_simplify_compact(const int32_t* face_cells, const uint8_t* keep, const int64_t* face_scan, int64_t m,
                          const int32_t* vertex_cell, int64_t n, const uint8_t* used, const int64_t* cell_scan, int64_t n_cells,
                          int32_t* out_faces, int32_t* vertex_map, void* stream);

/*
 * Point-cloud clean-up: the k nearest neighbours of every point of a cloud WITHIN the cloud, the outlier statistic and normals
 * taken from them (surf_amd/point_filter.py, backend="device"; point_knn.hip).  Added under SURF_ABI_VERSION 41 without a bump,
 * like the entry points above.  The device path returns the host path's arrays: both follow the rule below.  fp32 with separate
 * multiplies and adds (-ffp-contract=off) in the stated order unless fp64 is named.  Open3D's remove_statistical_outlier /
 * remove_radius_outlier / estimate_normals and PCL's StatisticalOutlierRemoval do the same jobs; the rule is RESTATED here, not
 * pinned against either library.
 *
 * THE RULE.  P (n,3) fp32, n <= 2^31 - 1; 1 <= k <= SURF_POINTS_KNN_MAX_K; max_dist finite and > 0.
 *   1. neighbours.  md2 = max_dist * max_dist (fp32, formed once on the host).  For a query i and a candidate j != i:
 *      dx = P[j].x - P[i].x (dy, dz alike), d2 = (dx*dx + dy*dy) + dz*dz; j is admitted iff d2 <= md2.  A duplicate of P[i] at another
 *      index is an ordinary neighbour at d2 = 0: only the index i itself is excluded.  A point with a non-finite coordinate is
 *      nobody's neighbour and has no neighbours.  The list of i is the first k admitted candidates in ascending (d2, j) order (equal
 *      d2: the smaller index first); count[i] is its length, 0 .. k.  The cell size of the search structure is not part of the rule.
 *   2. statistic.  dist_m = sqrtf(d2_m); sum = ((dist_0 + dist_1) + ...) in list order; stat[i] = sum / (float)k if count[i] == k,
 *      +inf otherwise (a STARVED point).
 *   3. statistical rule.  Over the finite stat values, in fp64: N = their number, S = their sum, Q = the sum of their squares;
 *      mu = S / N, sd = sqrt(max(Q / N - mu * mu, 0)), thr = mu + std_ratio * sd, keep[i] = (double)stat[i] <= thr.  Starved points
 *      are dropped; with N == 0 nothing is kept.  surf_points_stat_sums forms N, S, Q by fixed-slot partial sums (below): the same
 *      bits on every run, no float atomics.  The ORDER of that sum is the device's own: the host path adds the same numbers with
 *      np.sum, so its thr may differ in the last bits (a mask differs only where a stat lies within ~1e-15 relative of thr).
 *   4. radius rule.  keep[i] = count[i] == k, with k = the least number of neighbours and max_dist = the radius.
 *   5. normals.  For a point with count >= 2: e_m = P[j_m] - P[i] (fp32, per component), then in fp64, sequentially in list order
 *      from +0: S1[a] += e[a], S2[ab] += e[a] * e[b] for ab = 00 01 02 11 12 22.  The point itself contributes e = 0: m = count + 1,
 *      M[a] = S1[a] / m, C[ab] = S2[ab] / m - M[a] * M[b].  The normal is the unit eigenvector of C's smallest eigenvalue by
 *      SURF_POINTS_NORMAL_SWEEPS cyclic Jacobi sweeps over (p,q) = (0,1), (0,2), (1,2), V = I at the start, r the third index:
 *        if C[pq] != 0:  theta = (C[qq] - C[pp]) / (2 * C[pq]);  t = 1 / (|theta| + sqrt(theta*theta + 1)), negated if theta < 0;
 *                        c = 1 / sqrt(t*t + 1);  s = t * c;  h = t * C[pq];  C[pp] -= h;  C[qq] += h;  C[pq] = 0;
 *                        (C[rp], C[rq]) = (c*C[rp] - s*C[rq], s*C[rp] + c*C[rq]);  the same for (V[ip], V[iq]), i = 0, 1, 2.
 *      Column g of V with the smallest C[gg] (ties: the lowest g), divided by sqrt((x*x + y*y) + z*z), is n.
 *      Orientation, with the fp64 centre c of the point's view (view[i] in [0, n_views)): d = (n.x*(c.x - P.x) + n.y*(c.y - P.y)) +
 *      n.z*(c.z - P.z); n is negated if d < 0.  If d == 0, or without centres, n is negated iff its component of largest magnitude
 *      (ties: the lowest axis) is negative.  n is rounded to fp32 once.  count < 2, or a result that is not finite: (0,0,0).
 *
 * Entry points, in the order surf_amd.ops calls them (the sort of the keys, bincount and cumsum between them are the caller's):
 *   surf_points_knn_keys: keys (n) int64 = ((cx * ny) + cy) * nz + cz with c[a] = floor(((double)P[a] - lo[a]) / cell) clamped to the
 *     grid, or nx*ny*nz for a point with a non-finite coordinate (it sorts behind the table and is never visited).
 *     nx*ny*nz <= SURF_POINTS_KNN_MAX_CELLS (SURF_E_LIMIT beyond).
 *   surf_points_knn: the lists.  sorted_points (n,3) = P in ascending key order, sorted_index (n) int32 = the caller's index of every
 *     row of it, cell_start (nx*ny*nz + 1) int32 = the first row of every cell (cell_start[nx*ny*nz] = the number of finite points).
 *     index (n,k) int32 padded with -1, d2 (n,k) fp32 padded with +inf, count (n) int32; every row is written.  One thread per
 *     query in cell order; shells of cells around the query's own are walked until no unvisited point can enter the list (an equal
 *     d2 with a smaller index included: the test is strict) or the shell's reach exceeds max_dist.  The k-slot list lives in LDS
 *     (8 B per slot: d2's bits above the index, so that one integer comparison is the (d2, j) order).
 *   surf_points_knn_reduce: the same search without writing the lists: stat (n) fp32, count (n) int32 and, if normal is given,
 *     normal (n,3) fp32 by rule 5; points (n,3) = P in the caller's order (read for e_m).  view (n) int32 and centres (n_views,3)
 *     fp64 on the DEVICE are given together or not at all (SURF_E_ARG otherwise); a view index outside [0, n_views) is oriented
 *     as if there were no centres.
 *   surf_points_stat_sums: out (3) fp64 = [N, S, Q] of rule 3.  partials: device scratch of SURF_POINTS_STAT_SLOTS * 3 fp64.
 *     Workgroup w of min(ceil(n / 256), SURF_POINTS_STAT_SLOTS) adds its points (thread by thread in index order, then a fixed tree)
 *     into slot w; one workgroup adds the slots in slot order.
 * k outside [1, SURF_POINTS_KNN_MAX_K], a max_dist that is not finite and > 0 (or whose square is 0 or not finite), !(cell > 0) are
 * SURF_E_ARG; n >= 2^31 is SURF_E_LIMIT; n == 0 returns 0 at once.
 */
#define SURF_POINTS_KNN_MAX_K 32
#define SURF_POINTS_KNN_MAX_CELLS (1 << 26)
#define SURF_POINTS_NORMAL_SWEEPS 8
#define SURF_POINTS_STAT_SLOTS 1024
int surf_points_knn_keys(const float* points, int64_t n, double lo_x, double lo_y, double lo_z, double cell, int64_t nx, int64_t ny,
                         int64_t nz, int64_t* keys, void* stream);
int surf_points_knn(const float* sorted_points, const int32_t* sorted_index, const int32_t* cell_start, int64_t n, double lo_x,
                    double lo_y, double lo_z, double cell, int64_t nx, int64_t ny, int64_t nz, int k, float max_dist, int32_t* index,
                    float* d2, int32_t* count, void* stream);
int surf_points_knn_reduce(const float* points, const float* sorted_points, const int32_t* sorted_index, const int32_t* cell_start,
                           int64_t n, double lo_x, double lo_y, double lo_z, double cell, int64_t nx, int64_t ny, int64_t nz, int k,
                           float max_dist, const int32_t* view, const double* centres, int n_views, float* stat, int32_t* count,
                           float* normal, void* stream);
int surf_points_stat_sums(const float* stat, int64_t n, double* partials, double* out, void* stream);

/*
 * Point-set surface: a signed distance on the lattice nodes near an ORIENTED point cloud, from which the fusion path's marching
 * cubes, vertex colours, ray casting and simplification take a mesh (surf_amd/point_surface.py, backend="device";
 * point_surface.hip).  Added under SURF_ABI_VERSION 41 without a bump, like the entry points above.  The field is Kolluri's
 * implicit moving-least-squares surface, f(x) = sum_i w_i(x) n_i . (x - p_i) / sum_i w_i(x), with the compact weight
 * w = (1 - |x - p|^2 / R^2)^4: one gather pass, no global solve, only + - * / and comparisons, so the device path returns the host
 * path's arrays.  fp32 with separate multiplies and adds (-ffp-contract=off) in the stated order unless fp64 is named.
 *
 * THE RULE.  P (n,3) fp32 world points, N (n,3) fp32 normals pointing into free space (used as given, not renormalised), optional
 * colours (n,3) uint8, n <= 2^31 - 1.  A uniform lattice in the fusion conventions: fp32 axis arrays ax (nx), ay (ny), az (nz) that
 * follow lo + voxel * i (lo, voxel fp64: fusion.uniform_lattice) and the band layout above: res = max(nx,ny,nz) <= SURF_BAND_MAX_RES,
 * nbp = ceil(res / 8), brick ids (bx nbp + by) nbp + bz, state brick-major, slot * 512 + (lx << 6 | ly << 3 | lz).  A support radius R
 * (fp32, world units, R and R * R finite and > 0) and min_points >= 1.
 *   reach (fp64, lattice steps) comes from the caller and is the same number in every call:
 *        reach = (R / voxel) * (1 + 1e-5) + 4 * ulp32(A) / voxel,   A = the largest |axis value|,
 *      where ulp32(A) is the spacing of fp32 at A.  It bounds |i - u| of every admitted (node i, point at lattice coordinate u) pair
 *      per axis: an axis value lies within 2 ulp32(A) of lo + voxel * i (uniform_lattice's tolerance), the fp32 rounding of dx and of
 *      d2 moves the admission boundary by less than 1e-6 R, and the fp64 rounding of u is below 1e-12.  ring = ceil(reach / 8) is
 *      the number of bricks the support reaches across; 1 <= ring <= SURF_CLOUD_MAX_RING (SURF_E_LIMIT beyond: R just under 32 voxels).
 *   1. taking part.  A point takes part iff its three coordinates and its three normal components are finite and the normal is not
 *      (0,0,0) (estimate_normals returns that for a starved point) - and rule 2 keeps it.
 *   2. brick of a point.  Per axis u = ((double)p - lo) / voxel and b = floor(u / 8) (the division by 8 is exact), in fp64; b may be
 *      negative or >= the bricks of the axis, ceil(n_axis / 8): a point beyond the lattice still reaches nodes inside it.  A point
 *      with b < -ring or b >= ceil(n_axis / 8) + ring on any axis takes no part (by the bound above it is admitted at no node).
 *   3. order.  A node's sums run over the points taking part in ascending (bx, by, bz, caller index) order: the order of the
 *      composite keys below, which the lattice defines and no tunable cell does.  The keys are unique, so any sort gives it.
 *   4. per node x = (ax[i], ay[j], az[k]) and point, in fp32:  dx = x - p.x (dy, dz alike);  d2 = (dx*dx + dy*dy) + dz*dz;  the point is
 *      ADMITTED iff d2 < R2, with R2 = R * R and inv = 1 / R2 formed once;  t = 1 - d2 * inv;  t2 = t * t;  w = t2 * t2;
 *      g = (dx*nx + dy*ny) + dz*nz;  then count += 1, sw += w, sf += w * g and per channel sc += w * c with c = (colour + 0.5) / 256
 *      (exact in fp32; the inverse of fusion.quantise_colors_host).  The sums are sequential fp32 from +0.  (A pair that is not
 *      admitted may add +0 instead: that leaves such a sum as it is.)
 *   5. node state, in fusion's conventions.  Observed iff count >= min_points and sw > 0:  tsdf = fmin(fmax((sf / sw) / R, -1), 1),
 *      weight = (float)count, color = sc / sw per channel.  Not observed, or past the upper faces of the lattice (i >= nx ...):
 *      tsdf = weight = color = 0.  tsdf is positive on the normals' side, as in front of a measured surface; u = -tsdf through
 *      surf_fuse_lattice.
 *   6. allocation.  Per axis a point can be admitted at the nodes i0 = ceil(u - reach) .. i1 = floor(u + reach) only (fp64, then
 *      integers), clamped to [0, n_axis - 1]; a point with an empty interval on some axis allocates nothing.  Allocated are the
 *      bricks (i0 >> 3 .. i1 >> 3) per axis, a box of bricks per point: a superset of the bricks that hold a node with count >= 1,
 *      and for R = 3 voxels about 5 bricks per point where the blanket (2 ring + 1)^3 neighbourhood has 27.  The mesh does not
 *      depend on the allocation: a node outside it is unobserved, as a node with count 0 is.
 *
 * Entry points, in the order surf_amd.ops calls them (the sort and the gathers between them are the caller's):
 *   surf_cloud_brick_keys: keys (n) int64 = (key << 31) | index, key = ((bx + ring) * ey + (by + ring)) * ez + (bz + ring) over the
 *     extended brick grid e_axis = ceil(n_axis / 8) + 2 ring, or key = ex * ey * ez for a point that takes no part: those sort
 *     behind every brick, as the tail of surf_points_knn_keys does.
 *   surf_cloud_mark_bricks: rule 6 over sorted_points (m,3), the points taking part in key order; mark (nbp^3 bytes) gets a 1 at
 *     every allocated brick.  surf_compact and surf_band_assign turn the marks into the table and the brick list.
 *   surf_cloud_field_bricks: rules 3-5 at the 512 nodes of every listed brick; every value of tsdf, weight (n_bricks * 512) and,
 *     given together with sorted_colors or not at all (SURF_E_ARG otherwise), color (n_bricks * 512, 3) is written.  sorted_keys
 *     (m), sorted_points, sorted_normals (m,3) fp32 and sorted_colors (m,3) uint8: the points taking part in ascending key order.
 *     One workgroup per brick; the candidates of a brick are the points of the (2 ring + 1)^3 bricks around it, found as
 *     (2 ring + 1)^2 runs of the sorted keys by binary search (no start table) and staged through LDS in key order; a candidate
 *     whose rule-6 box misses the brick is dropped while staging - it is admitted at none of its nodes.  staged (n_bricks) int32, or
 *     null: the candidates of every brick that were not dropped (a brick evaluates 512 x staged pairs).
 * n == 0 (keys), m == 0 (mark) and n_bricks == 0 (field) return 0 without a launch; m == 0 with bricks writes zero state.
 * !(voxel > 0), a reach that is not finite and > 0, min_points < 1, an R that is not finite and > 0 (or whose square is 0 or not
 * finite) are SURF_E_ARG; res > SURF_BAND_MAX_RES, ring > SURF_CLOUD_MAX_RING, n or m >= 2^31, n_bricks * 512 >= 2^31 are SURF_E_LIMIT.
 */
#define SURF_CLOUD_MAX_RING 4
int surf_cloud_brick_keys(const float* points, const float* normals, int64_t n, double lo_x, double lo_y, double lo_z, double voxel,
                          int64_t nx, int64_t ny, int64_t nz, double reach, int64_t* keys, void* stream);
int surf_cloud_mark_bricks(const float* sorted_points, int64_t m, double lo_x, double lo_y, double lo_z, double voxel, int64_t nx,
                           int64_t ny, int64_t nz, double reach, uint8_t* mark, void* stream);
int surf_cloud_field_bricks(const int64_t* sorted_keys, const float* sorted_points, const float* sorted_normals,
                            const uint8_t* sorted_colors, int64_t m, const int32_t* bricks, int64_t n_bricks, const float* ax,
                            const float* ay, const float* az, int64_t nx, int64_t ny, int64_t nz, double lo_x, double lo_y,
                            double lo_z, double voxel, double reach, float radius, int min_points, float* tsdf, float* weight,
                            float* color, int32_t* staged, void* stream);

/*
 * Mesh smoothing: Laplacian and Taubin lambda|mu steps with uniform (umbrella) weights on a triangle mesh
 * (surf_amd/mesh_smooth.py, backend="device"; mesh_smooth.hip).  Added under SURF_ABI_VERSION 41 without a bump, like the entry
 * points above.  The device path returns the host path's arrays: both follow the rule below, fp64 with separate multiplies and
 * adds (-ffp-contract=off), positions rounded to fp32 after every step.  Faces, colours, vertex count and order never change.
 *
 * THE RULE.  vertices (n,3) fp32, all finite; faces (m,3) int32 with indices in [0, n); iterations >= 0; 0 < lam <= 1; mu absent
 * or finite with mu < -lam; pin_boundary; max_move absent or finite and > 0; normals not wanted, wanted, or wanted and aligned
 * with given normals (n,3) fp32.
 *   1. edges.  A face (a,b,c) has the undirected edges {a,b}, {b,c}, {c,a}, in that order.  An edge with equal ends is dropped, and
 *      so is an edge that an earlier edge of the SAME face equals, so that a face counts once at each of its edges.  i and j are
 *      neighbours iff at least one face has the edge {i,j}; N(i) lists the neighbours of i once each in ascending index order and
 *      d_i is its length (0 for a vertex without an edge: an ISOLATED vertex).  uses({i,j}) is the number of faces, a face listed
 *      twice counted twice, that have the edge.  i is a BOUNDARY vertex iff uses({i,j}) == 1 for some j; edges of two, three or
 *      more faces are interior.
 *   2. one step with factor s (fp64).  x'_i = x_i to the bit if d_i == 0, or if pin_boundary and i is a boundary vertex.  Otherwise
 *      per axis:  S = +0;  for j in N(i) ascending: S = S + (double)x_j;  m = S / (double)d_i;
 *      x'_i = (float)((double)x_i + s * (m - (double)x_i)).  A step reads only the positions before it (Jacobi, two buffers).
 *   3. schedule.  Without mu: `iterations` steps with s = lam (Laplacian).  With mu: `iterations` pairs, a step with s = lam and
 *      then a step with s = mu (Taubin).
 *   4. displacement cap, once after the last step, with M = max_move and x0 the input position:  d[a] = (double)x[a] -
 *      (double)x0[a];  q = (d0*d0 + d1*d1) + d2*d2.  If q > M*M the vertex is CAPPED:  r = M / sqrt(q),
 *      x[a] = (float)((double)x0[a] + d[a] * r).  The movement of a vertex is q of its final fp32 position (formed again after a
 *      cap); moved_max = sqrt(max q), moved_rms = sqrt(Q / (double)n) with Q the sum of all q by the 256-ary sequential tree: the
 *      values are cut into runs of 256 consecutive ones (the last may be shorter), every run is added from +0 in index order, and
 *      the run sums are summed in the same way until one value is left.
 *   5. normals, from the final positions.  Per face F = e1 x e2 in fp64 with e1 = p1 - p0, e2 = p2 - p0:
 *      F = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x).  Per vertex S[a] = the sum of F[a] over every corner of every
 *      face that names it, in (face, corner) order from +0 (a face that names it twice is added twice);  L2 = (Sx*Sx + Sy*Sy) + Sz*Sz;
 *      normal[a] = (float)(S[a] / sqrt(L2)), or (0,0,0) if L2 == 0 or L2 is not finite.  With given normals g:
 *      t = ((double)nx*(double)gx + (double)ny*(double)gy) + (double)nz*(double)gz of the fp32 normal, and the normal is negated
 *      iff t < 0: the orientation of whatever made g survives.
 *
 * Entry points, in the order surf_amd.ops.smooth_mesh calls them (sorts, scans and searches between them are the caller's).
 * Positions travel between the steps as (n,4) fp32 rows of 16 bytes, (x, y, z, unused), so that a neighbour is one load.
 *   surf_smooth_edge_keys: keys (6 m) int64.  Slot k of face f writes (lo << 32 | hi) to keys[6 f + 2 k] and (hi << 32 | lo) to
 *     keys[6 f + 2 k + 1]: one directed key per end.  A dropped edge (rule 1) and every edge of a face with an index outside [0, n)
 *     write SURF_SMOOTH_NO_KEY, which sorts behind every key; such a face also sets flag[0] = 1 (int32, zeroed by the caller),
 *     which the CALLER reads before it goes on.
 *   surf_smooth_adjacency: from sorted_keys (6 m) ascending and head_scan (6 m) int64, the INCLUSIVE scan of "differs from the key
 *     before it" (head_scan[0] = 1): neighbours[head_scan[j] - 1] = low word of the first key of every run of equal keys (nnz =
 *     the number of runs below SURF_SMOOTH_NO_KEY), which lists N(i) row after row; boundary (n) uint8, zeroed by the caller, gets
 *     a 1 at the high word of every run of length one.  row_start (n + 1) int32, the first entry of every row, is the caller's
 *     (a search of v << 32 in sorted_keys, looked up in head_scan).
 *   surf_smooth_step: rule 2, positions_out = step(positions_in) with factor s; one vertex per lane.  A vertex of more than
 *     SURF_SMOOTH_WAVE_DEGREE neighbours is summed by its whole wavefront, 64 gathers at a time, in the same order.
 *   surf_smooth_cap: rule 4 from positions (n,4) and vertices0 (n,3): out_vertices (n,3) fp32, moved2 (n) fp64 = q of the final
 *     position, capped (n) uint8.  max_move <= 0 means no cap.
 *   surf_smooth_sum256: out (ceil(count / 256)) fp64 = the run sums of rule 4 of values (count) fp64; the caller repeats it until
 *     one value is left.
 *   surf_smooth_normals: rule 5.  corner_order (3 m) int64 = the stable ascending sort permutation of faces read as a flat array,
 *     corner_start (n + 1) int64 the first position of every vertex in it; face_normals (m,3) fp64 is scratch; given_normals (n,3)
 *     fp32 or null.
 * n == 0 or m == 0 returns 0 at once where there is nothing to do.  n or m > SURF_SMOOTH_MAX_ITEMS is SURF_E_LIMIT (6 m directed
 * edges are counted in int32).  A null pointer, nnz outside [0, 6 m], a factor or max_move that is not finite are SURF_E_ARG.
 */
#define SURF_SMOOTH_MAX_ITEMS 357913941         /* (2^31 - 1) / 6 */
#define SURF_SMOOTH_NO_KEY 0x7fffffffffffffffLL
#define SURF_SMOOTH_WAVE_DEGREE 32
int surf_smooth_edge_keys(const int32_t* faces, int64_t m, int64_t n, int64_t* keys, int32_t* flag, void* stream);
int surf_smooth_adjacency(const int64_t* sorted_keys, const int64_t* head_scan, int64_t m, int64_t n, int64_t nnz,
                          int32_t* neighbours, uint8_t* boundary, void* stream);
int surf_smooth_step(const float* positions_in, float* positions_out, int64_t n, const int32_t* row_start,
                     const int32_t* neighbours, int64_t nnz, const uint8_t* boundary, int pin_boundary, double s, void* stream);
int surf_smooth_cap(const float* positions, const float* vertices0, int64_t n, double max_move, float* out_vertices,
                    double* moved2, uint8_t* capped, void* stream);
int surf_smooth_sum256(const double* values, int64_t count, double* out, void* stream);
int surf_smooth_normals(const float* vertices, int64_t n, const int32_t* faces, int64_t m, const int64_t* corner_order,
                        const int64_t* corner_start, const float* given_normals, double* face_normals, float* normals,
                        void* stream);

/*
 * Mesh deviation: the exact distance from a point to a triangle mesh, and from it the two-sided vertex-sampled deviation between
 * two meshes (surf_amd/mesh_distance.py, backend="device"; mesh_distance.hip).  Added under SURF_ABI_VERSION 41 without a bump,
 * like the entry points above.  The device path returns the host path's arrays: both follow the rule below.
 *
 * THE RULE.  vertices (n,3) fp32, all finite; faces (m,3) int32 with indices in [0, n); points (k,3) fp32, all finite; max_dist
 * finite and > 0.  All arithmetic is fp64 on the exactly converted fp32 values, multiplies and adds separate (-ffp-contract=off);
 * dot(u,v) = (u0*v0 + u1*v1) + u2*v2; vector expressions are taken per axis.
 *   PAIR VALUE q(p, face) with a, b, c the face's corners in order (the region scheme of Ericson, Real-Time Collision Detection,
 *   5.1.5):
 *     ab=b-a  ac=c-a  ap=p-a   d1=dot(ab,ap) d2=dot(ac,ap)
 *     bp=p-b                   d3=dot(ab,bp) d4=dot(ac,bp)
 *     cp=p-c                   d5=dot(ab,cp) d6=dot(ac,cp)
 *     vc=d1*d4-d3*d2   vb=d5*d2-d1*d6   va=d3*d6-d5*d4   e1=d4-d3   e2=d5-d6
 *     the first test that holds, in this order, names the REGION:
 *      0: d1<=0 && d2<=0                        c* = a
 *      1: d3>=0 && d4<=d3                       c* = b
 *      2: vc<=0 && d1>=0 && d3<=0 && d1>d3      c* = a + ab*(d1/(d1-d3))
 *      3: d6>=0 && d5<=d6                       c* = c
 *      4: vb<=0 && d2>=0 && d6<=0               c* = a + ac*(d2/(d2-d6))
 *      5: va<=0 && e1>=0 && e2>=0               c* = b + (c-b)*(e1/(e1+e2))
 *      6: otherwise   den=1/((va+vb)+vc)        c* = (a + ab*(vb*den)) + ac*(vc*den)
 *     e = p - c*;  q = dot(e,e)
 *   Only the quotient of the region taken is part of the value.  Degenerate faces take part through the same tests.  d1 > d3 in
 *   test 2 is there for them: d1 - d3 is |ab|^2, and without it a face with a == b would answer 0/0 for every point that is not
 *   nearest to a; with it such a face is the segment a-c (tests 3 and 4).  a == c, b == c, a == b == c and collinear corners never
 *   reach a vanishing divisor.  A pair whose q is NaN is ignored.
 *   PER QUERY.  Q = the least non-NaN q over ALL faces; face = the smallest face index that attains it; closest = that pair's c*
 *   (fp64); distance = sqrt(Q).  If distance < max_dist does not hold (no face at all, for one): distance +inf, face -1, closest
 *   (+inf, +inf, +inf).  The value is a minimum over all faces: it does not depend on how the faces are searched.
 *   DEVIATION of mesh A against mesh B.  "forward" queries the vertices of A that at least one face of A names, in index order,
 *   against B; "backward" is the same with A and B exchanged.  Per direction: count (queries), beyond (queries answered +inf), and
 *   over the rest max, mean = S1 / found and rms = sqrt(S2 / found), where S1 and S2 are the sums of distance and of
 *   distance * distance in query order by the 256-ary sequential tree of the smoothing rule 4 (surf_smooth_sum256; a `beyond`
 *   query contributes +0).  Nothing found: max, mean and rms are absent.  hausdorff = the larger of the two max, absent if either
 *   is.  The default max_dist is the diagonal of the joint bounding box of all vertices of both meshes.
 *
 * THE SEARCH is a dense cell table over the bounding box of the vertices the faces name, nx * ny * nz cells of size `cell` from
 * (lo_x, lo_y, lo_z); a coordinate x lies in cell floor((x - lo) / cell) of its axis, clamped to the table.  Every face is
 * listed in every cell that its axis-aligned box overlaps: a (cell, face) PAIR.  A query walks shells of cells around its own
 * cell, as surf_fscore_nearest does: after shells 0 .. k-1 every unlisted face lies more than R = (k - 1) * cell * (1 - 1e-6)
 * away (its nearest point is inside its box, hence in an unvisited cell), and the walk stops once Q < R * R STRICTLY (a face at
 * exactly R could still tie with a smaller index) or R >= max_dist.  A query outside the table starts at the first shell that
 * touches it and answers +inf at once if that shell is beyond ceil(max_dist / (cell * (1 - 1e-6))) + 1.
 *   Why the margin also covers the rounding of q: the dots of a pair are sums of products of differences of size at most
 *   L + d (L the face's extent, d the distance), so the computed q is off by a few 2^-53 (L + d)^2, while R * R stands 2e-6 R * R
 *   below the true bound.  For d near R >= cell that needs 2^-53 (L / cell + 1)^2 << 2e-6, i.e. L / cell far below 1e5.  The
 *   caller keeps no more than SURF_MESHDIST_MAX_AXIS_CELLS cells along an axis, so L / cell < 1.8 * 4096.
 *   PAIR BUDGET (surf_amd.ops.point_to_mesh): the cell starts at about four cells per face by volume and grows by 1.25 until the
 *   pairs number at most max(SURF_MESHDIST_PAIRS_PER_FACE * m, 2^16).  A pair costs a 48-byte record and a sort entry, and every
 *   further listing of a face is one more evaluation by the queries that pass it, so the budget bounds the table at 8 x 60 bytes
 *   per face and the repeats at a small factor; 2^16 lets a small mesh keep fine cells.  A tuning choice, not measured against
 *   others (the meshes measured came to 2.4 to 4.0 pairs per face without a growth).
 *
 * Entry points, in the order surf_amd.ops.point_to_mesh calls them (scans, sorts and gathers between them are the caller's).
 *   surf_meshdist_pairs_count: records (m,12) fp32 = (a, b, c, the face index as int32 bits, 0, 0): 48 bytes, three 16-byte
 *     loads; counts (m) int64 = the cells the face's box overlaps.  A face with an index outside [0, n) gets a zero record and
 *     count 0 (the caller has refused such faces before).
 *   surf_meshdist_pairs_emit: from records and starts (m) int64, the EXCLUSIVE scan of counts with `pairs` their total:
 *     pair_cell[starts[f] + i] int64 = (x * ny + y) * nz + z of the i-th cell of face f, pair_face[...] int32 = f.  No order is
 *     promised within a cell, and none is needed.  One lane per face: a face that spans the table is written by one lane.
 *   surf_meshdist_query: the hot kernel, one lane per query.  cell_records (pairs,12) fp32 = the records in cell order, cell_start
 *     (nx ny nz + 1) int32 the first record of every cell.  order (k) int64 = a permutation of the queries (the caller sorts them
 *     by cell, so that the 64 lanes of a wavefront walk the same cells and read the same records); lane t serves query order[t]
 *     and writes ITS rows: distance (k) fp64, face (k) int64, closest (k,3) fp64.  No sqrt and no division outside the region
 *     taken inside the walk; every loop is bounded by the shell limit and the clipped table range.
 * k == 0 or m == 0 returns 0 at once.  Null pointers, a cell or max_dist that is not finite and > 0, a lo that is not finite, a
 * table dimension < 1 and pairs < 0 are SURF_E_ARG; n, m, k or pairs > 2^31 - 1, a dimension > SURF_MESHDIST_MAX_AXIS_CELLS and
 * nx ny nz > SURF_MESHDIST_MAX_CELLS are SURF_E_LIMIT; all reported before any launch.
 * Measured on an MI355X (scripts/time_mesh_distance.py, profiles/mesh_distance.txt), a 589 k-face mesh against its 10-pair Taubin
 * smoothing, 299 k queries a direction: pairs 1.9 ms, sort 0.9 ms, query 1.3 ms; 2.4 pairs per face, 240 pairs evaluated per query.
 */
#define SURF_MESHDIST_MAX_AXIS_CELLS 4096
#define SURF_MESHDIST_MAX_CELLS 67108864        /* 2^26 */
#define SURF_MESHDIST_PAIRS_PER_FACE 8
int surf_meshdist_pairs_count(const float* vertices, int64_t n, const int32_t* faces, int64_t m, double lo_x, double lo_y,
                              double lo_z, double cell, int64_t nx, int64_t ny, int64_t nz, float* records, int64_t* counts,
                              void* stream);
int surf_meshdist_pairs_emit(const float* records, int64_t m, double lo_x, double lo_y, double lo_z, double cell, int64_t nx,
                             int64_t ny, int64_t nz, const int64_t* starts, int64_t pairs, int64_t* pair_cell, int32_t* pair_face,
                             void* stream);
int surf_meshdist_query(const float* points, const int64_t* order, int64_t k, const float* cell_records, int64_t pairs,
                        const int32_t* cell_start, double lo_x, double lo_y, double lo_z, double cell, int64_t nx, int64_t ny,
                        int64_t nz, double max_dist, double* distance, int64_t* face, double* closest, void* stream);

/*
 * Feature-preserving mesh denoising: two-stage bilateral normal filtering (surf_amd/mesh_denoise.py, backend="device";
 * mesh_denoise.hip).  Stage one filters the face normals (the local iterative scheme of Zheng, Fu, Au, Tai 2011, "Bilateral normal
 * filtering for mesh denoising"), stage two moves the vertices to fit them (Sun, Rosin, Martin, Langbein 2007, "Fast and effective
 * feature-preserving mesh denoising").  Added under SURF_ABI_VERSION 41 without a bump, like the entry points above.  The device
 * path returns the host path's arrays: both follow the rule below, fp64 on fp32 data with separate multiplies and adds
 * (-ffp-contract=off), one operation per operator in the written order, and no function beyond + - * / sqrt, which round
 * correctly in numpy and on gfx950.  Faces, colours, vertex count and order never change.  "Smoothing rule k" is rule k of the
 * surf_smooth_* group above.
 *
 * THE RULE.  vertices (n,3) fp32, all finite; faces (m,3) int32 with indices in [0, n); 0 <= normal_iterations, vertex_iterations
 * <= 10000; sigma_r finite and > 0; sigma_s absent, or finite and > 0; pin_boundary; max_move absent or finite and > 0; normals
 * not wanted, wanted, or wanted and aligned with given normals (n,3) fp32.  dot-like sums are (t0 + t1) + t2.
 *   1. face record, from the INPUT positions p0, p1, p2 of the face's corners in order.  F = e1 x e2 by smoothing rule 5's formula
 *      and L2 = (Fx*Fx + Fy*Fy) + Fz*Fz.  The face is DEGENERATE iff L2 == 0 or L2 is not finite, and its record is all zeros.
 *      Otherwise L = sqrt(L2), normal[a] = (float)(F[a] / L), area = (float)(0.5 * L), centroid[a] = (float)((((double)p0[a] +
 *      (double)p1[a]) + (double)p2[a]) / 3.0).  The normal of a face that is not degenerate has a component of at least 0.57 and
 *      stays of unit length through rule 4, so the zero normal marks exactly the degenerate faces.
 *   2. sigma_s when absent: the mean side length.  The side from a to b has d[a] = (double)b[a] - (double)a[a], q = (d0*d0 + d1*d1)
 *      + d2*d2 and length sqrt(q); the 3 m lengths of the sides (p0p1, p1p2, p2p0) in (face, side) order are summed by the 256-ary
 *      sequential tree of smoothing rule 4 and the sum is divided by (double)(3 m).  A result that is not finite or not > 0 is
 *      refused.
 *   3. face neighbours.  N(f) lists the faces that share at least one vertex with f, each once, f itself included, in this order:
 *      for slot k = 0, 1, 2 of f, the corners that name vertex f[k] in (face, corner) order (corner_order / corner_start of
 *      surf_smooth_normals); the face g of such a corner is taken unless g names one of f[0..k-1] (it was taken there), or the
 *      corner is not g's first that names f[k] (g names the vertex twice), or f[k] equals an earlier slot of f (the slot was
 *      walked).  Degenerate faces are members like any other: their area gives them weight 0.
 *   4. one normal iteration (Jacobi: it reads only the normals before it; areas and centroids never change), with
 *      is = 1.0 / (9.0 * sigma_s * sigma_s) and ir = 1.0 / (9.0 * sigma_r * sigma_r) in fp64.  A degenerate face keeps its zero
 *      normal.  For any other f:  S = +0;  for g in N(f) in order:  d[a] = (double)c_g[a] - (double)c_f[a] of the centroids,
 *      ds2 = (d0*d0 + d1*d1) + d2*d2, us = 1.0 - ds2 * is;  e[a] = (double)n_g[a] - (double)n_f[a] of the normals, dn2 likewise,
 *      ur = 1.0 - dn2 * ir;  if us <= 0 or ur <= 0 the term is skipped, otherwise
 *      w = ((double)area_g * ((us*us)*(us*us))) * ((ur*ur)*(ur*ur)) and S[a] = S[a] + w * (double)n_g[a].
 *      L2 = (Sx*Sx + Sy*Sy) + Sz*Sz;  n'_f[a] = (float)(S[a] / sqrt(L2)), or n_f unchanged if L2 == 0 or L2 is not finite.
 *      The weight is the compact (1 - r^2/R^2)^4 of the point-set surface with support R = 3 sigma: no exp.
 *   5. one vertex iteration (Jacobi on fp32 positions), with n_g the normal of face g after the last normal iteration.  k_i is the
 *      number of corners that name i and whose face is not degenerate.  x'_i = x_i to the bit if k_i == 0, or if pin_boundary and
 *      i is a boundary vertex of smoothing rule 1.  Otherwise T = +0 and for every such corner in (face, corner) order, with
 *      xa, xb, xc the CURRENT positions of the corners of its face g in the face's order:
 *      c[a] = (((double)xa[a] + (double)xb[a]) + (double)xc[a]) / 3.0 (not rounded to fp32),
 *      d = ((c0 - x0)*n0 + (c1 - x1)*n1) + (c2 - x2)*n2 with x = (double)x_i and n = (double)n_g,  T[a] = T[a] + n[a] * d;
 *      x'_i[a] = (float)((double)x_i[a] + T[a] / (double)k_i).  A face that names i twice is added twice.
 *   6. displacement cap, movement statistics and normals: smoothing rules 4 and 5 verbatim, through surf_smooth_cap,
 *      surf_smooth_sum256 and surf_smooth_normals; the boundary flags are surf_smooth_adjacency's.
 * Fixed points: a mesh whose faces around every moving vertex lie in one plane has d == 0 in rule 5 wherever c - x lies in that
 * plane to the bit (a lattice cube, a planar grid), and a neighbourhood of equal normals returns that normal from rule 4 when the
 * normalisation is exact; the tests pin both on a cube and on a planar grid.
 *
 * Entry points, in the order surf_amd.ops.denoise_mesh calls them (sorts, scans and searches between them are the caller's).
 * Face records travel as (m,8) fp32 rows of 32 bytes, (nx, ny, nz, area, cx, cy, cz, unused): two 16-byte loads, the first of
 * which is all a normal iteration writes; positions travel as (n,4) fp32 rows as in smoothing.
 *   surf_denoise_face_records: rule 1 into records (m,8), and when side_lengths is not null rule 2's (m,3) fp64 lengths.  A face
 *     with an index outside [0, n) gets a zero record and zero lengths (the caller has refused such faces before).
 *   surf_denoise_neighbour_count: counts (m) int64 = the length of N(f).  corner_order (3 m) int64, corner_start (n + 1) int64 as
 *     for surf_smooth_normals.  The caller scans them: face_row_start (m + 1) int32 with the total last, which it READS first:
 *   surf_denoise_neighbour_emit: face_neighbours (total) int32 = N(f) row after row.  total > 2^31 - 1 is SURF_E_LIMIT, here and in
 *     the caller, before anything is written.
 *   surf_denoise_normal_step: rule 4, the first 16 bytes of every row of records_out from records_in (both hold the same areas
 *     and centroids).  One face per lane; a row of more than SURF_DENOISE_WAVE_ROW neighbours is summed by the face's whole
 *     wavefront, 64 gathers at a time, in the same order.
 *   surf_denoise_vertex_step: rule 5, positions_out from positions_in and the normals of records.  One vertex per lane; a vertex
 *     of more than SURF_DENOISE_WAVE_ROW corners is summed by its whole wavefront in the same way.
 * n == 0 or m == 0 returns 0 at once.  n or m > SURF_SMOOTH_MAX_ITEMS and total > 2^31 - 1 are SURF_E_LIMIT; a null pointer, a
 * negative size, in == out and an is or ir that is not finite and >= 0 are SURF_E_ARG; all reported before any launch.
 */
#define SURF_DENOISE_WAVE_ROW 48
int surf_denoise_face_records(const float* vertices, int64_t n, const int32_t* faces, int64_t m, float* records,
                              double* side_lengths, void* stream);
int surf_denoise_neighbour_count(const int32_t* faces, int64_t m, int64_t n, const int64_t* corner_order,
                                 const int64_t* corner_start, int64_t* counts, void* stream);
int surf_denoise_neighbour_emit(const int32_t* faces, int64_t m, int64_t n, const int64_t* corner_order,
                                const int64_t* corner_start, const int32_t* face_row_start, int64_t total,
                                int32_t* face_neighbours, void* stream);
int surf_denoise_normal_step(const float* records_in, float* records_out, int64_t m, const int32_t* face_row_start,
                             const int32_t* face_neighbours, int64_t total, double inv_s, double inv_r, void* stream);
int surf_denoise_vertex_step(const float* positions_in, float* positions_out, int64_t n, const int32_t* faces, int64_t m,
                             const float* records, const int64_t* corner_order, const int64_t* corner_start,
                             const uint8_t* boundary, int pin_boundary, void* stream);

/*
 * Textured meshes: the source photographs baked into one atlas image (surf_amd/mesh_texture.py, backend="device";
 * mesh_texture.hip).  Added under SURF_ABI_VERSION 41 without a bump, like the entry points above.  The device path returns the
 * host path's arrays: both follow the rule below in fp32 with separate multiplies and adds (-ffp-contract=off), one operation per
 * operator in the written order, and no function beyond + - * / sqrtf floorf fabsf, which round correctly in numpy and on gfx950
 * (the camera centre alone is formed in float64 by the caller and rounded once).  Positions, faces and vertex order are never
 * touched.  Dot-like sums are (t0 + t1) + t2.
 *
 * THE RULE.  vertices (n,3) fp32, faces (m,3) int32, T = texels_per_edge an integer in [4, 64], K views in order.
 *   1. atlas layout, arithmetic only.  Faces 2k and 2k+1 share cell k, T+1 texels wide and T tall, at column k % cols and row
 *      k / cols of the atlas, with ncell = ceil(m / 2), cols = ceil(sqrt(ncell)), rows = ceil(ncell / cols); the atlas is
 *      (Ha, Wa) = (rows T, cols (T+1)) texels, row 0 first.  Texel (X, Y): i = X % (T+1), j = Y % T, k = (Y / T) cols + X / (T+1).
 *      Face A = 2k owns the texels with i + j <= T-1, face B = 2k+1 those with i + j >= T.  A's corners 0, 1, 2 sit at the centres
 *      of texels (i, j) = (0, 0), (T-2, 0), (0, T-2), B's at (T, T-1), (2, T-1), (T, 1): the bilinear footprint of every point of a
 *      triangle lies in texels of its own face, so there is no dilation pass.  A texel whose face index is >= m belongs to no face.
 *      uv (3m, 2) fp32, one row per face corner: u = (x + 0.5) / Wa, v = 1 - (y + 0.5) / Ha of the corner's texel (x, y) of the
 *      atlas, formed in float64 and rounded once (v points up, as an OBJ file has it).
 *   2. texel to point.  den = (float)(T-2).  A: beta = (float)i / den, gamma = (float)j / den.  B: beta = (float)(T-i) / den,
 *      gamma = (float)(T-1-j) / den.  The guard texels beyond the hypotenuse keep their extrapolated barycentrics (beta + gamma
 *      > 1).  With a, b, c the face's corners: e1 = b - a, e2 = c - a, p = (a + beta * e1) + gamma * e2 per axis,
 *      n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), nn = (nx*nx + ny*ny) + nz*nz.  The face is NEVER SEEN, and
 *      no view is looked at, if an index is outside [0, n), a coordinate of a corner is not finite, or nn is not in (0, FLT_MAX].
 *      Otherwise ln = sqrtf(nn).
 *   3. one view: P (12) = world -> (x z, y z, z) in pixel indices of its image, image (H, W, 3) fp32 and the mesh's own depth map
 *      D (H, W) fp32 from that camera (0 = nothing hit), H, W >= 2, centre (3) = -M^-1 t of P = [M | t].
 *        cx = ((P0*px + P1*py) + P2*pz) + P3, cy with P4..P7, z with P8..P11;  skip unless z > z_min
 *        x = cx / z, y = cy / z;  skip unless 0 <= x <= W-1 and 0 <= y <= H-1              (float compares: a NaN fails)
 *        d = centre - p per axis, nd = (nx*dx + ny*dy) + nz*dz, dd = (dx*dx + dy*dy) + dz*dz
 *        cos = nd / (ln * sqrtf(dd)), cos = fabsf(cos) when two_sided;  skip unless cos >= min_cos
 *        x0 = min((int)floorf(x), W-2), y0 = min((int)floorf(y), H-2), u = x - (float)x0, v = y - (float)y0    (u = 1 on the
 *        last column); the four pixels (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1) must ALL have D > 0, z <= D + depth_tol and
 *        D <= z + depth_tol, else skip: silhouettes take colour from neither side.  (The second half keeps a texel of a front
 *        surface from blending in the pixels beside it that show a surface far behind it.)
 *        colour per channel = lerp(lerp(c00, c01, u), lerp(c10, c11, u), v) with lerp(a, b, s) = (1 - s) * a + s * b
 *        w = cos, then w = w * cos power-1 times (power an integer in [1, 16]: no powf)
 *   4. all views, in the order 0..K-1:  sum_c = sum_c + w * colour_c per channel, sum_w = sum_w + w, count = count + 1, all
 *      starting from 0.  The accumulators live in memory between launches of at most SURF_FUSE_MAX_VIEWS views, so the result
 *      does not depend on how the views are cut into launches.
 *   5. finish.  A texel of no face gets `fill`.  One with sum_w > 0 gets sum_c / sum_w per channel.  Any other texel of a face
 *      whose indices are inside [0, n) gets, when vertex colours (n,3) uint8 are given, the mix of its corners' colours
 *      C = (float)colour / 255.0f:  s = beta + gamma;  if s > 1: beta = beta / s, gamma = gamma / s;  alpha = (1 - beta) - gamma;
 *      value = (alpha * Ca + beta * Cb) + gamma * Cc.  Every texel left gets `fill`.  Then q = value * 256,
 *      q = fmin(fmax(q, 0), 255), (uint8)q - surf_fuse_vertex_colors' quantisation.
 *
 * Entry points, in the order surf_amd.ops.bake_texture calls them.  The depth maps come from surf_raster_first_hit with K = I,
 * w2c = P, h = Hup = H, w = Wup = W: the upper 32 bits of its keys.
 *   surf_texture_pack_view: record (H, W, 4) fp32 = (r, g, b, D) per pixel from image (H, W, 3) and depth (H, W): a bilinear tap
 *     is one 16-byte load that carries colour and depth.
 *   surf_texture_bake: rules 1-4 for n_views >= 0 views, one texel per lane.  sums (Ha Wa, 4) fp32 = (sum_r, sum_g, sum_b, sum_w),
 *     count (Ha Wa) int32 or null.  first != 0: the accumulators start from 0 whatever the arrays hold, and every entry is
 *     written; first == 0: they continue from the arrays.  h_P (n_views,12), h_centre (n_views,3), h_hw (n_views,2) = (H, W) and
 *     h_records (n_views) device pointers are HOST arrays.  No atomics: a texel has one owner.
 *   surf_texture_finish: rule 5, atlas (Ha, Wa, 3) uint8; vertex_colors (n,3) uint8 or null.  Every texel is written.
 * A null pointer, n < 0, m < 1, T outside [4, 64], cols or rows < 1, rows cols < ceil(m / 2), n_views < 0, power outside
 * [1, 16], H or W < 2 and a depth_tol, min_cos or z_min that is NaN are SURF_E_ARG.  n_views > SURF_FUSE_MAX_VIEWS, n or
 * m > 2^31 - 1, an atlas of 2^31 texels or more and a view of 2^31 / 4 pixels or more are SURF_E_LIMIT.  All are reported before
 * any launch; what does not depend on a view's (H, W) or record pointer, before a host array is read.
 */
int surf_texture_pack_view(const float* image, const float* depth, int H, int W, float* record, void* stream);
int surf_texture_bake(const float* vertices, int64_t n, const int32_t* faces, int64_t m, int T, int cols, int rows,
                      const float* h_P, const float* h_centre, const float* const* h_records, const int* h_hw, int n_views,
                      float z_min, float depth_tol, float min_cos, int power, int two_sided, int first, float* sums,
                      int32_t* count, void* stream);
int surf_texture_finish(const float* sums, int64_t n, const int32_t* faces, int64_t m, int T, int cols, int rows,
                        const uint8_t* vertex_colors, float fill, uint8_t* atlas, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SURF_HIP_H */
