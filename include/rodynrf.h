/* rodynrf.h -- C ABI of the MI355X-native RoDynRF ray-batch hot path (librodynrf.so).
 *
 * The reference (facebookresearch/robust-dynrf) is pure Python: it has no FFI.  Its boundary for
 * this path is the Python call surface of three objects:
 *
 *   TensorVMSplit.forward / TensorVMSplit_TimeEmbedding.forward   models/tensorBase.py:704-850
 *   renderer.sampleXYZ                                            renderer.py:147-170
 *   renderer.raw2outputs                                          renderer.py:173-315
 *   TensorVMSplit_TimeEmbedding.get_forward_backward_scene_flow   models/tensoRF.py:446-462
 *   ray generation (ids2pixel .. ndc_rays_blender2)               train.py:96-103, 1062-1077
 *
 * Each entry point below replaces one of those calls (cited per function).  The host-side mirror
 * (robust-dynrf_amd/ *.py) binds them with ctypes and re-exposes the reference signatures.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; all tensors fp32, row major;
 *     masks are uint8; indices int32/int64 as stated.
 *   - return 0 on success, a negative code on failure; rdrf_last_error() gives the message
 *     (thread local). No entry point throws, allocates device memory, or synchronises: outputs and
 *     the workspace are caller-allocated, work is enqueued on `stream`.
 *   - VM factors are CHANNEL-LAST: the reference's (1,C,H,W) plane tensors with the component
 *     axis contiguous and explicit h/w strides (RdrfVM); line i is [L_i][C_i].  plane 0/1/2 =
 *     XY/XZ/YZ, line 0/1/2 = Z/Y/X (matMode/vecMode, models/tensorBase.py:326-327).  The host
 *     mirror stores every plane as [H][W][C] (plane 0 [y][x][C], planes 1,2 [z][x|y][C]): the two
 *     bilinear columns of a tap are then adjacent in memory, which the scatter exploits (one L2
 *     atomic request for both); any other h/w strides are accepted.
 *   - gradients are ACCUMULATED (+=) into the caller's (zero-initialised) buffers.
 */
#ifndef RODYNRF_H
#define RODYNRF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: RdrfStaticParams / RdrfDynamicParams grew the trailing packed_fwd / packed_bwd pointers (round 2);
 * 3: sorted scatter workspace + fused render entry points (round 3);
 * 4: rdrf_set_scatter_mode replaces the RDRF_SCATTER / RDRF_RENDER environment switches -- no entry point reads the
 *    caller's environment any more; rdrf_render_chunks_fwd (round 4).  A binding built against another version must refuse to load: the structs
 *    are passed by pointer and read to their full length.
 * 5: rdrf_saved_row_bytes and RDRF_SCATTER_SORTED_PLAIN (added in round 5 under version 4: a stale version-4 library then failed
 *    on the missing symbol instead of on the version check); rdrf_render_chunks_fwd coalesces the chunks that fit the
 *    caller's workspace into one launch sequence (same results, round 6).
 * 6: iteration scalars may live on the DEVICE, so that a whole training iteration can be captured in one HIP graph and
 *    replayed while they change (train.py draws the white-background coin and ramps loss weights every iteration):
 *    rdrf_composite_fwd / _bwd take `white_dev` (a device float, 0 or 1, that overrides add_white_bg when non-NULL) and
 *    RdrfLossTerm grew the trailing `coef_dev` (a device float that multiplies `coef` when non-NULL);
 *    rdrf_rows_scatter_add. */
#define RDRF_ABI_VERSION 6

typedef void* rdrf_stream_t; /* hipStream_t */

enum { RDRF_RAY_NDC = 0, RDRF_RAY_CONTRACT = 1, RDRF_RAY_OTHER = 2 };
enum { RDRF_ACT_RELU = 0, RDRF_ACT_SOFTPLUS = 1 };
enum { RDRF_HEAD_MLP_FEA = 0, RDRF_HEAD_MLP_FEA_TIMEEMBEDDING = 1 };
enum { RDRF_SCATTER_RAY = 0, RDRF_SCATTER_SORTED = 1, RDRF_SCATTER_AUTO = 2, RDRF_SCATTER_SORTED_PLAIN = 3 };

/* One vector-matrix factor set (3 planes + 3 lines).  Components are always contiguous (channel
 * stride 1); the texel strides are explicit so that the planes containing the ray-marching axis can
 * be stored with that axis fastest: element (c,h,w) of plane i lives at h*sH[i] + w*sW[i] + c. */
typedef struct {
  float* plane[3]; /* logical (C,H,W) */
  float* line[3];  /* [L][C]    */
  int C[3];        /* components per plane/line pair: {16,4,4} or {48,12,12} */
  int H[3], W[3];  /* plane i: H = grid[matMode[i][1]], W = grid[matMode[i][0]] */
  int L[3];        /* line i:  L = grid[vecMode[i]] */
  int sH[3], sW[3]; /* float strides of one step in h / w */
} RdrfVM;

/* Scalars the path reads from the field object (models/tensorBase.py:282-339, get_kwargs). */
typedef struct {
  float aabb[6];        /* min xyz, max xyz */
  float distance_scale; /* 25 */
  float weight_thres;   /* rayMarch_weight_thres, 1e-4 */
  float density_shift;  /* softplus shift */
  int act;              /* RDRF_ACT_* (fea2denseAct) */
  int ray_type;         /* RDRF_RAY_* */
  int static_head;      /* RDRF_HEAD_* (static field only) */
} RdrfFieldCfg;

/* Static TensorVMSplit parameters (state_dict names in comments). Used for values AND, with the
 * same struct filled with gradient buffers, for gradients. */
typedef struct {
  RdrfVM density, app;  /* density_plane/line.{0,1,2}, app_plane/line.{0,1,2} */
  float* basis;         /* basis_mat.weight (27,72) */
  float *w1, *b1;       /* renderModule.mlp.0 (128,138) | (128,135) */
  float *w2, *b2;       /* renderModule.mlp.2 (128,128) */
  float *w3, *b3;       /* renderModule.mlp.4 (3,128) | renderModule.mlp_view.0 (3,131) */
  /* optional (NULL = the entry point packs into its workspace, as before): images written by rdrf_static_pack
   * for THESE weights.  The caller owns their validity: re-pack after every change of w1..b3 / basis. */
  const float* packed_fwd;
  const float* packed_bwd;
} RdrfStaticParams;

/* Dynamic TensorVMSplit_TimeEmbedding parameters. */
typedef struct {
  RdrfVM density, blending, app;
  float* basis;                 /* basis_mat.weight (27,216) */
  float *rw1, *rb1;             /* renderModule.mlp.0 (128,107) */
  float *rw2, *rb2;             /* renderModule.mlp.2 (128,128) */
  float *rwv, *rbv;             /* renderModule.mlp_view.0 (3,131) */
  float *l1w, *l1b;             /* layer1 (64,17) */
  float *l2w, *l2b;             /* layer2 (30,64) */
  float *l3w, *l3b;             /* layer3 (64,93) */
  float *l4w, *l4b;             /* layer4 (64,64) */
  float *l5w, *l5b;             /* layer5 (3,64) */
  float *dw1, *db1, *dw2, *db2; /* density_layer1 (64,152), density_layer2 (1,64) */
  float *bw1, *bb1, *bw2, *bb2; /* blending_layer1/2 */
  float *sfw[4], *sfb[4];       /* scene_flow_mlp.{0,2,4,6}: (64,36)(64,64)(64,64)(6,64) */
  const float* packed_fwd;      /* optional images of rdrf_dynamic_pack (see RdrfStaticParams) */
  const float* packed_bwd;
} RdrfDynamicParams;

int rdrf_abi_version(void);
const char* rdrf_last_error(void);

/* Bytes of workspace a forward/backward call of either field needs for N rays x S samples. */
size_t rdrf_workspace_bytes(int N, int S);
/* The forward calls alone (inference: rdrf_*_fwd with saved == NULL, rdrf_render_*) need only this much of it
 * (weight pack area, compaction list, warped coordinates: ~16 B per sample + 4 MB instead of ~6 KB per sample). */
size_t rdrf_forward_workspace_bytes(int N, int S);
/* Training mode: a forward call given a `saved` buffer of this size (kind 0 = static field,
 * 1 = dynamic field, 2 = scene flow) stores the activations its backward needs; the matching
 * *_bwd call must receive the same buffer untouched.  saved == NULL => inference, nothing kept. */
size_t rdrf_saved_bytes(int kind, int N, int S);
/* Rows are saved only where a backward can read them.  `flags` of the *_ex entry points (0 = as the plain ones):
 *   RDRF_SAVE_NO_APP  the colours of this call are values only -- no gradient will arrive for rgb.  The density phase saves
 *                     as usual, the appearance phase runs the inference kernels and writes no rows; the appearance block is
 *                     the last one of the buffer, so a buffer of this kind is a prefix of the full layout.  The matching
 *                     *_bwd call tells the two kinds apart by `saved_bytes` (the size the forward was given) and refuses
 *                     (-1, nothing launched) a non-NULL g_rgb for a buffer without appearance rows.  Kind 2 ignores it. */
#define RDRF_SAVE_NO_APP 1
size_t rdrf_saved_bytes_ex(int kind, int N, int S, int flags);
/* Bytes per sample of the activation rows inside that buffer (a measurement aid, bench.py `saved_bytes_per_sample`):
 * phase 0 = dynamic field, density phase (every sample); 1 = dynamic field, appearance phase (per sample that passes the
 * weight > 1e-4 mask, models/tensorBase.py:773-790); 2 = static field, appearance phase (per masked sample); 3 = scene flow. */
size_t rdrf_saved_row_bytes(int phase);

/* ---- ray generation: train.py:96-103 + dataLoader/ray_utils.py:53-140 + camera.py:8-15 -------
 * ids[N] int64 flat ray ids over (T,H,W); poses9[T][9] 6-D rotation + translation; focal scalar.
 * rays[N][6]; if ndc != 0 the NDC warp with near = `near` is applied (ndc_rays_blender2). */
int rdrf_generate_rays(const int64_t* ids, const float* poses9, const float* focal, int N, int T,
                       int H, int W, int ndc, float near, float* rays, rdrf_stream_t stream);
/* grad_rays[N][6] -> grad_poses9[T][9] (+=), grad_focal[1] (+=) */
int rdrf_generate_rays_bwd(const int64_t* ids, const float* poses9, const float* focal, int N,
                           int T, int H, int W, int ndc, float near, const float* grad_rays,
                           float* grad_poses9, float* grad_focal, rdrf_stream_t stream);

/* The flow-displaced rays of train.py:1433-1460, 1530-1557, 1968-1990, 2033-2050: uv[N][2] (may be NULL)
 * replaces the pixel centre of the ray id by (column + 0.5 + flow_x, row + 0.5 + flow_y); the camera is
 * frame id / (H W) + view_shift clamped to [0, T-1] (allposes_refine_f / allposes_refine_b). uv carries no
 * gradient (the flow is data). */
int rdrf_generate_rays_uv(const int64_t* ids, const float* uv, int view_shift, const float* poses9,
                          const float* focal, int N, int T, int H, int W, int ndc, float near, float* rays,
                          rdrf_stream_t stream);
int rdrf_generate_rays_uv_bwd(const int64_t* ids, const float* uv, int view_shift, const float* poses9,
                              const float* focal, int N, int T, int H, int W, int ndc, float near,
                              const float* grad_rays, float* grad_poses9, float* grad_focal,
                              rdrf_stream_t stream);

/* ---- renderer.sampleXYZ (renderer.py:147-170) ------------------------------------------------
 * NDC: models/tensorBase.py:487-499. jitter[S] (uniform [0,1), shared by all rays) or NULL. */
int rdrf_sample_ndc(const float* rays, int N, int S, float near, float far, const float* jitter,
                    const float aabb_host[6], float* xyz, float* z, uint8_t* valid,
                    rdrf_stream_t stream);
/* contract: models/tensorBase.py:524-559. jitter_inner[S-S/2+1], jitter_outer[S/2+1] or NULL. */
int rdrf_sample_contract(const float* rays, int N, int S, float near, float far,
                         const float* jitter_inner, const float* jitter_outer, float* xyz,
                         float* z, uint8_t* valid, rdrf_stream_t stream);
/* grad_xyz[N][S][3] -> grad_rays[N][6] (+=). z[N][S] are the sample depths the sampler returned. */
int rdrf_sample_bwd(const float* rays, const float* z, int N, int S, int ray_type,
                    const float* grad_xyz, float* grad_rays, rdrf_stream_t stream);

/* world: models/tensorBase.py:501-522, the sampler of every ray_type but ndc / contract (RDRF_RAY_OTHER).  The rays march
 * through the box aabb_host (lo[3], hi[3]) in world space: t_min = the entry depth max_k min((hi_k - o_k) / vec_k,
 * (lo_k - o_k) / vec_k), vec = d with 1e-6 for 0, clamped to [near, far]; z[n][j] = t_min[n] + step * (j + u[n]) with the
 * field's stepSize and jitter_per_ray u[N] (uniform [0,1), one per ray) or NULL; xyz = o + d z; valid = inside the box. */
int rdrf_sample_world(const float* rays, int N, int S, float near, float far, float step,
                      const float* jitter_per_ray, const float aabb_host[6], float* xyz, float* z,
                      uint8_t* valid, rdrf_stream_t stream);
/* grad_xyz[N][S][3], grad_z[N][S] (either may be NULL) -> grad_rays[N][6] (+=).  Unlike rdrf_sample_bwd's, these z depend
 * on the ray: beside grad_xyz . d(o + d z) at fixed z, (sum_j grad_xyz . d + sum_j grad_z) flows through t_min -- nowhere
 * where the clamp is active, else into axis k and face f of the selected quotient: d/do_k = -1 / vec_k, d/dd_k =
 * -t_min / vec_k (0 where d_k == 0).  The selection is recomputed from rays, aabb_host, near and far. */
int rdrf_sample_world_bwd(const float* rays, const float* z, int N, int S, float near, float far,
                          const float aabb_host[6], const float* grad_xyz, const float* grad_z,
                          float* grad_rays, rdrf_stream_t stream);

/* ---- TensorVMSplit.forward (models/tensorBase.py:704-850, models/tensoRF.py:118-196) ---------
 * outputs: rgb[N][S][3], sigma[N][S], weight[N][S], dists[N][S] (= dists*distance_scale).
 * rgb may be NULL (rdrf_static_fwd and rdrf_dynamic_fwd): the caller does not consume the colours -- passes B-D of the
 * trainer discard them (train.py:1166-1246, 1433-1625) -- and the appearance phase (gather, basis, RGB head) is not run;
 * every other output is unchanged.  A later backward of such a call must not carry a gradient for rgb. */
int rdrf_static_fwd(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* rays,
                    const float* ts, const float* xyz, const float* z, const uint8_t* valid, int N,
                    int S, float* rgb, float* sigma, float* weight, float* dists, void* saved,
                    size_t saved_bytes, void* ws, size_t ws_bytes, rdrf_stream_t stream);
/* the same with a flags word (RDRF_SAVE_*: see rdrf_saved_bytes_ex); `saved_bytes` is rdrf_saved_bytes_ex of the same flags */
int rdrf_static_fwd_ex(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* rays,
                       const float* ts, const float* xyz, const float* z, const uint8_t* valid, int N,
                       int S, float* rgb, float* sigma, float* weight, float* dists, void* saved,
                       size_t saved_bytes, void* ws, size_t ws_bytes, rdrf_stream_t stream, int flags);
/* g_* are gradients wrt the four outputs (any may be NULL = zero). G receives parameter
 * gradients (+=); g_xyz[N][S][3], g_z[N][S], g_rays[N][6] (+=, each may be NULL). */
int rdrf_static_bwd(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* rays,
                    const float* ts, const float* xyz, const float* z, const uint8_t* valid, int N,
                    int S, const float* g_rgb, const float* g_sigma, const float* g_weight,
                    const float* g_dists, const RdrfStaticParams* G, float* g_xyz, float* g_z,
                    float* g_rays, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                    rdrf_stream_t stream);

/* ---- TensorVMSplit_TimeEmbedding.forward (models/tensorBase.py:704-850,
 *      models/tensoRF.py:521-811) -- adds blending[N][S], xyz_prime[N][S][3]. */
int rdrf_dynamic_fwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* rays,
                     const float* ts, const float* xyz, const float* z, const uint8_t* valid,
                     int N, int S, float* blending, float* weight, float* xyz_prime, float* rgb,
                     float* sigma, float* dists, void* saved, size_t saved_bytes, void* ws,
                     size_t ws_bytes, rdrf_stream_t stream);
int rdrf_dynamic_fwd_ex(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* rays,
                        const float* ts, const float* xyz, const float* z, const uint8_t* valid,
                        int N, int S, float* blending, float* weight, float* xyz_prime, float* rgb,
                        float* sigma, float* dists, void* saved, size_t saved_bytes, void* ws,
                        size_t ws_bytes, rdrf_stream_t stream, int flags);
int rdrf_dynamic_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* rays,
                     const float* ts, const float* xyz, const float* z, const uint8_t* valid,
                     int N, int S, const float* g_blending, const float* g_weight,
                     const float* g_xyz_prime, const float* g_rgb, const float* g_sigma,
                     const float* g_dists, const RdrfDynamicParams* G, float* g_xyz, float* g_z,
                     float* g_rays, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                     rdrf_stream_t stream);

/* ---- compute_densityfeature / compute_appfeature / compute_blendingfeature / warp_coordinate -----
 * The per-point building blocks TensorBase.forward calls (models/tensoRF.py:118-196 static;
 * :521-541 warp_coordinate, :543-629 compute_blendingfeature, :646-732 compute_densityfeature,
 * :734-811 compute_appfeature dynamic), on a batch of M independent points.  They run the SAME
 * kernels as rdrf_*_fwd/bwd in a point geometry (32 points per wave tile, time per point).
 *   xn[M][3]     NORMALISED coordinates ([-1,1] inside the aabb; outside is zero padded, as grid_sample)
 *   density[M]   raw density feature (static: sum of the 24 VM products; dynamic: density_layer2 output)
 *   blending[M]  raw blending feature (before the sigmoid)
 *   app[M][27]   basis_mat output
 * Any output pointer may be NULL (not computed).  saved: NULL for inference, else a buffer of
 * rdrf_features_saved_bytes(dynamic, M) bytes that the matching *_bwd call needs.
 * dynamic: x is xn when x_is_normalized != 0 (compute_*), else UN-normalised coordinates
 * (warp_coordinate); t[M] is the time of every point; xyz_prime[M][3] = un-normalised warped point.
 * bwd: g_* gradients wrt the outputs (NULL = zero); parameter gradients accumulate (+=) into G;
 * g_x[M][3] (+=, may be NULL) is the gradient wrt the coordinates as they were passed in. */
size_t rdrf_features_saved_bytes(int dynamic, int M);
size_t rdrf_features_workspace_bytes(int M);
size_t rdrf_features_bwd_workspace_bytes(int M);
int rdrf_static_features_fwd(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* xn, int M,
                             float* density, float* app, void* saved, size_t saved_bytes, void* ws,
                             size_t ws_bytes, rdrf_stream_t stream);
int rdrf_static_features_bwd(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* xn, int M,
                             const float* g_density, const float* g_app, const RdrfStaticParams* G,
                             float* g_xn, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                             rdrf_stream_t stream);
int rdrf_dynamic_features_fwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* x,
                              const float* t, int M, int x_is_normalized, float* density, float* blending,
                              float* app, float* xyz_prime, void* saved, size_t saved_bytes, void* ws,
                              size_t ws_bytes, rdrf_stream_t stream);
int rdrf_dynamic_features_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* x,
                              const float* t, int M, int x_is_normalized, const float* g_density,
                              const float* g_blending, const float* g_app, const float* g_xyz_prime,
                              const RdrfDynamicParams* G, float* g_x, void* saved, size_t saved_bytes,
                              void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- get_forward_backward_scene_flow (models/tensoRF.py:446-462) -----------------------------
 * pts[N][S][3] un-normalised, ts[N] -> sf_f[N][S][3], sf_b[N][S][3]. */
int rdrf_scene_flow_fwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* pts,
                        const float* ts, int N, int S, float* sf_f, float* sf_b, void* saved,
                        size_t saved_bytes, void* ws, size_t ws_bytes, rdrf_stream_t stream);
int rdrf_scene_flow_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* pts,
                        const float* ts, int N, int S, const float* g_sf_f, const float* g_sf_b,
                        const RdrfDynamicParams* G, float* g_pts, void* saved, size_t saved_bytes,
                        void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- renderer.raw2outputs (renderer.py:173-315) ----------------------------------------------
 * add_white_bg: the caller draws the train-time coin (renderer.py:269).  white_dev (nullable): the same coin as a DEVICE
 * float (0.0f or 1.0f) read when the kernel runs -- it overrides add_white_bg, so a launch captured in a HIP graph follows
 * the coin of each replay.  out13: pointers to the 13
 * outputs in the reference's order: rgb_map_full[N][3], depth_map_full[N], acc_map_full[N],
 * weights_full[N][S], rgb_map_s, depth_map_s, acc_map_s, weights_s, rgb_map_d, depth_map_d,
 * acc_map_d, weights_d, dynamicness_map[N]. */
int rdrf_composite_fwd(const float* rgb_s, const float* sigma_s, const float* rgb_d,
                       const float* sigma_d, const float* dists, const float* blending,
                       const float* z, const float* rays, int N, int S, int ray_type,
                       int add_white_bg, const float* white_dev, float* const out13[13], rdrf_stream_t stream);
/* g_out13: gradients wrt the 13 outputs (entries may be NULL). g_in8: gradient buffers (+=) for
 * rgb_s, sigma_s, rgb_d, sigma_d, dists, blending, z, rays (entries may be NULL). */
int rdrf_composite_bwd(const float* rgb_s, const float* sigma_s, const float* rgb_d,
                       const float* sigma_d, const float* dists, const float* blending,
                       const float* z, const float* rays, int N, int S, int ray_type,
                       int add_white_bg, const float* white_dev, const float* const g_out13[13],
                       float* const g_in8[8], rdrf_stream_t stream);

/* ---- induced optical flow / disparity of the rendered 3-D point (renderer.py:1334-1392
 * render_3d_point + induce_flow; NDC2world :1266, world2NDC :1276, contract2world :1286).
 * P = sum_s w p + (1 - sum_s w) * far(rays); world = NDC2world(P) | contract2world(P); projected
 * with the neighbour pose c2w[N][3][4] and focal; flow = pixel - pts_2d, disp = 1 + 2/z_cam.
 * focal: DEVICE pointer to one float (it is a trained scalar). H, W: image size.
 * render_single_3d_point / induce_flow_single (renderer.py:1301, :1381) are the S = 1, w = 1 case.
 * bwd: gradient buffers accumulate (+=); g_rays, g_c2w[N][12], g_focal[1] may be NULL. */
int rdrf_induce_flow_fwd(int H, int W, const float* focal, const float* c2w, const float* weights,
                         const float* pts, const float* pts_2d, const float* rays, int N, int S,
                         int ray_type, float* flow, float* disp, rdrf_stream_t stream);
int rdrf_induce_flow_bwd(int H, int W, const float* focal, const float* c2w, const float* weights,
                         const float* pts, const float* rays, int N, int S, int ray_type,
                         const float* g_flow, const float* g_disp, float* g_weights, float* g_pts,
                         float* g_rays, float* g_c2w, float* g_focal, rdrf_stream_t stream);

/* ---- adjoint of a row gather rows[n] = table[idx[n]] (the camera matrices of the neighbour frames,
 * `allposes_refine[view +- 1]`, train.py:1895-1948, live when the poses are optimised): g_table[idx[n]][c] += g_rows[n][c].
 * idx [N] int64 in [0, R); g_rows [N][C]; g_table [R][C] accumulates (+=). */
int rdrf_rows_scatter_add(const int64_t* idx, const float* g_rows, int N, int R, int C, float* g_table,
                          rdrf_stream_t stream);

/* ---- distortion loss (train.py:1299-1312, 1685-1716, 1840-1856 call flatten_eff_distloss of the
 * un-vendored torch_efficient_distloss with ray_id = tile(arange(N), S), i.e. N rays x S points).
 * Published formulation (DVGO v2 / mip-NeRF 360), m ascending along a ray:
 *   loss_ray[n] = sum_i 2 w_i (m_i sum_{j<i} w_j - sum_{j<i} w_j m_j) + (1/3) sum_i interval w_i^2
 * (= sum_ij w_i w_j |m_i - m_j| + ...); the caller sums loss_ray and divides by N.
 * bwd: g_w[n][i] += g_ray[n] * (2 (m_i (P_i - Q_i) + (QM_i - PM_i)) + (2/3) interval w_i) with
 * P/PM exclusive prefix and Q/QM exclusive suffix sums of w and w m.  m gets no gradient (the
 * reference passes it detached / it is not trained).  interval_pt (per point, may be NULL) overrides
 * the scalar interval.  PARITY UNPINNED against the library itself (absent here): checked against an
 * O(S^2) evaluation of the double sum. */
int rdrf_distloss_fwd(const float* w, const float* m, float interval, const float* interval_pt,
                      int N, int S, float* loss_ray, rdrf_stream_t stream);
int rdrf_distloss_bwd(const float* w, const float* m, float interval, const float* interval_pt,
                      int N, int S, const float* g_ray, float* g_w, rdrf_stream_t stream);

/* ---- total-variation regulariser of the factor tensors (utils.py:157-181 TVLoss, applied to every
 * plane / line by models/tensoRF.py:100-116, 418-444 each iteration of configs/Nvidia.txt).
 * One launch handles up to RDRF_TV_MAX logical (1,C,H,W) views with arbitrary element strides
 * (channel-last storage included).  sums[t] = { sum (x[h+1]-x[h])^2 , sum (x[w+1]-x[w])^2 }; the
 * caller forms TVLoss_weight * 2 * (h_tv/count_h + w_tv/count_w) / batch exactly as the reference
 * does (a line has count_w = 0, so the reference's VALUE is 0/0 = NaN while its gradient is finite;
 * that is reproduced by doing this scalar arithmetic on the host side of the ABI, in torch).
 * bwd: g_x[t] (same strides as x[t]) += g_sums[t][0] * d h_tv/dx + g_sums[t][1] * d w_tv/dx, the
 * second term skipped when W == 1 (its coefficient is 2/0 there). g_sums is a DEVICE array. */
#define RDRF_TV_MAX 16
typedef struct {
  const float* x;
  float* g;            /* gradient buffer (bwd only) */
  int C, H, W;
  long long sC, sH, sW;  /* element strides of the (1,C,H,W) view */
} RdrfTensor4;
int rdrf_tv_fwd(const RdrfTensor4* t, int n, float* sums /* [n][2], overwritten */, rdrf_stream_t stream);
int rdrf_tv_bwd(const RdrfTensor4* t, int n, const float* g_sums /* [n][2] */, rdrf_stream_t stream);
/* The gradient of the TV terms in one pass, for any number of tensors: t[i].g (+=) receives
 * coef_host[i][0] * d(h_tv)/dx + coef_host[i][1] * d(w_tv)/dx (the W term is skipped when W == 1).  The caller
 * folds TVLoss_weight * 2 / (count * batch), the 1e-2 / 1e-3 plane / line factors of TV_loss_* and the
 * config's TV weight into the HOST coefficients: no forward sums, no scalar arithmetic on the device. */
int rdrf_tv_grad(const RdrfTensor4* t, int n, const float* coef_host /* [n][2] */, rdrf_stream_t stream);

/* ---- Adam over a flat parameter range (torch.optim.Adam as train.py:924-934 builds it: betas
 * (0.9, 0.99), eps 1e-8, no weight decay / amsgrad; the learning-rate decay of train.py:2608-2612 is the
 * caller's: it passes the current rates).  p, g, m, v: n floats each, 16-byte aligned, n % 4 == 0.
 * Elements [0, split) step with lr0 (the VM factors), [split, n) with lr1 (the networks).  step >= 1 is
 * the 1-based iteration for the bias corrections; grad_scale multiplies g first (1 / world size when the
 * data-parallel exchange summed the per-rank gradients). */
int rdrf_adam_step(float* p, const float* g, float* m, float* v, size_t n, size_t split, float lr0,
                   float lr1, float beta1, float beta2, float eps, int step, float grad_scale,
                   rdrf_stream_t stream);

/* ---- upsample_volume_grid (models/tensoRF.py:199-232, 814-850): bilinear, align_corners=True, of up to
 * RDRF_TV_MAX (1,C,H,W) views with arbitrary element strides (src[i] -> dst[i], C % 4 == 0) in one launch;
 * lines are the W == 1 case. */
int rdrf_upsample_bilinear(const RdrfTensor4* src, const RdrfTensor4* dst, int n, rdrf_stream_t stream);

/* ---- density_L1 / blending_L1 (models/tensoRF.py:80-98, 378-416): sum over the X x Y x Z grid of
 * |feature2density(sum_c plane x line)| without materialising any volume (the reference builds a
 * [1,24,X,Y,Z] tensor).  fwd: sum_out[0] = the sum (the caller divides by X*Y*Z).  bwd: g_mean[0] (device)
 * = d loss / d mean; plane / line gradients accumulate (+=) into gvm. {16,4,4}-component sets only. */
int rdrf_dense_l1_fwd(const RdrfVM* vm, int act, float density_shift, float* sum_out, rdrf_stream_t stream);
int rdrf_dense_l1_bwd(const RdrfVM* vm, const RdrfVM* gvm, int act, float density_shift, const float* g_mean,
                      rdrf_stream_t stream);

/* ---- packed weight images.  Every field entry point first re-lays its MLP weights out for the MFMA kernels
 * (a ~6 us launch, ~40 of them per training iteration).  The weights of a field do not change between the passes
 * of one iteration or the chunks of a render, so a caller may pack once and hand the image in through
 * packed_fwd / packed_bwd of the parameter struct.  image: rdrf_pack_floats() floats, 16-byte aligned.
 * backward = 0: the image of *_fwd / *_features_fwd / scene_flow_fwd / render_fwd; 1: of the *_bwd entry points.
 * The factor tensors (planes / lines) are NOT part of the image. */
size_t rdrf_pack_floats(void);
int rdrf_static_pack(const RdrfStaticParams* P, int static_head, int backward, float* image, rdrf_stream_t stream);
int rdrf_dynamic_pack(const RdrfDynamicParams* P, int backward, float* image, rdrf_stream_t stream);

/* ---- the per-ray / per-sample loss terms of one iteration, reduced in one launch (+ a finishing launch)
 * and differentiated in one launch.  Replaces the elementwise chains of train.py:1323-1331 (photometric),
 * :1341-1365 (dynamicness mask), :1392-1410 (induced flow, masked means), :1421, 1627 (scene flow, weighted by
 * the sample weights in this path), :1522-1524, 1619-1621 (induced disparity), :1828-1832 (static photometric,
 * background-masked), :2293-2299 (disparity smoothness).
 *   term = coef [* *coef_dev] * sum_rows w[row] * sum_cols rho(x + ysign * y) / Z
 *   rho = r^2 | |r| | r ;  Z = rows * cols (NORM_MEAN)  or  sum_rows w + 1e-8 (NORM_WEIGHT, a masked mean)
 * x, y: [rows][cols] contiguous (y nullable); w: [rows] (nullable = 1).  gx / gy (backward only, nullable):
 * d loss / d x, d loss / d y, WRITTEN (not accumulated).
 * fwd: partial = rdrf_loss_terms_workspace_floats(n) floats of scratch; out = 1 + 2 n floats:
 *      out[0] = sum of the terms, out[1 + k] = coef_k / Z_k, out[1 + n + k] = value of term k.
 * bwd: out as written by fwd; g_loss[0] (device) = d L / d out[0].  Deterministic (no float atomics). */
enum { RDRF_LOSS_SQUARE = 0, RDRF_LOSS_ABS = 1, RDRF_LOSS_IDENTITY = 2 };
enum { RDRF_LOSS_NORM_MEAN = 0, RDRF_LOSS_NORM_WEIGHT = 1 };
#define RDRF_MAX_LOSS_TERMS 32
typedef struct {
  const float* x;
  const float* y;
  const float* w;
  float* gx;
  float* gy;
  long long rows;
  int cols;
  int kind;   /* RDRF_LOSS_* */
  int norm;   /* RDRF_LOSS_NORM_* */
  float ysign;
  float coef;
  const float* coef_dev; /* nullable: DEVICE float multiplied into coef when the finishing kernel runs (loss weights that
                            change every iteration -- train.py:1299-1312 distortion ramp, Temp_static :1034-1036 -- inside
                            a captured HIP graph) */
} RdrfLossTerm;
size_t rdrf_loss_terms_workspace_floats(int n);
int rdrf_loss_terms_fwd(const RdrfLossTerm* terms, int n, float* partial, float* out, rdrf_stream_t stream);
/* The same in two stages, for data-parallel runs that want the single-process normalisers (the reference's
 * masked means divide by the mask sum of the WHOLE batch, train.py:1391-1394): stats[2k], stats[2k+1] = this rank's
 * (sum_rows w rho, sum_rows w) of term k; the caller sums `stats` over the ranks (all-reduce) and passes both to finish,
 * which normalises a masked mean by (sum over ranks of sum w) / world + 1e-8, so that the MEAN over ranks of the per-rank
 * losses / gradients is exactly the single-process value.  rdrf_loss_terms_fwd == stats + finish(local, local, 1). */
int rdrf_loss_terms_stats(const RdrfLossTerm* terms, int n, float* partial, float* stats, rdrf_stream_t stream);
int rdrf_loss_terms_finish(const RdrfLossTerm* terms, int n, const float* stats_local, const float* stats_global, int world,
                           float* out, rdrf_stream_t stream);
int rdrf_loss_terms_bwd(const RdrfLossTerm* terms, int n, const float* out, const float* g_loss,
                        rdrf_stream_t stream);

/* ---- per-frame median-normalised monocular depth loss: train.py:797-807 compute_depth_loss summed over the
 * frames of the batch and divided by the number of rays used (train.py:1636-1664 dynamic, 2097-2121 static):
 *   for each frame k with more than one (unmasked) ray:  t = median(p), s = mean|p - t|, u = (p - t) / (s + 1e-10),
 *   likewise v from gt;  L_k = sum (u - v)^2;      loss = coef * sum_k L_k / sum_k n_k.
 * The reference loops over the frames on the host (one sync each); here one workgroup per frame selects its
 * rays (in ray order), bitonic-sorts them in LDS for the median (torch.median: the lower middle element) and
 * writes the loss AND its gradient wrt pred in the same pass: g_raw[j] = d(sum_k L_k)/d pred[j], with the
 * median's gradient spread evenly over the elements equal to it (ATen's evenly_distribute_backward).
 * pred, gt [N]; frame [N] int64 in [0, T); mask [N] uint8 or NULL (NULL: every ray is used).
 * out[0] = loss, out[1] = coef / sum_k n_k (the factor g_raw is to be multiplied with), out[2] = sum_k n_k.
 * ws: rdrf_frame_depth_loss_workspace_bytes(N, T).  N <= 32768 (the gathered batch of a data-parallel run included). */
size_t rdrf_frame_depth_loss_workspace_bytes(int N, int T);
int rdrf_frame_depth_loss_fwd(const float* pred, const float* gt, const int64_t* frame, const uint8_t* mask,
                              int N, int T, float coef, float* out, float* g_raw, void* ws, size_t ws_bytes,
                              rdrf_stream_t stream);
/* g_pred[j] = g_loss[0] * out[1] * gscale * g_raw[j]   (gscale: world size when the batch was gathered over a
 * data-parallel group whose exchange averages the per-rank gradients; 1 otherwise) */
int rdrf_frame_depth_loss_bwd(const float* g_raw, const float* out, const float* g_loss, int N, float gscale, float* g_pred,
                              rdrf_stream_t stream);

/* ---- no-grad render of a ray chunk (renderer.py:740-812 loop body): sample -> static -> dynamic -> composite;
 * writes rgb_map_full[N][3], depth_map_full[N]; scratch for the per-sample tensors comes out of ws
 * (rdrf_render_workspace_bytes).
 *   rdrf_render_fused_fwd     ONE cooperative launch: persistent workgroups walk the sampler, both density phases, both
 *                             appearance phases and the compositor, separated by grid-wide barriers (the LDS is re-filled
 *                             with each phase's weight image).  Same device code as the per-phase kernels: identical bits.
 *   rdrf_render_sequence_fwd  the per-phase kernels as a launch sequence (11 stream operations).
 *   rdrf_render_fwd           the launch sequence (measured faster at every size on MI355X: 274 vs 378 us per 512-ray
 *                             chunk, equal on whole frames; csrc/rdrf_render.hip). */
size_t rdrf_render_workspace_bytes(int N, int S);
int rdrf_render_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s,
                    const RdrfDynamicParams* PD, const RdrfFieldCfg* cfg_d, const float* rays,
                    const float* ts, int N, int S, float near, float far, float* rgb_map,
                    float* depth_map, void* ws, size_t ws_bytes, rdrf_stream_t stream);
int rdrf_render_fused_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s,
                          const RdrfDynamicParams* PD, const RdrfFieldCfg* cfg_d, const float* rays,
                          const float* ts, int N, int S, float near, float far, float* rgb_map,
                          float* depth_map, void* ws, size_t ws_bytes, rdrf_stream_t stream);
int rdrf_render_sequence_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s,
                             const RdrfDynamicParams* PD, const RdrfFieldCfg* cfg_d, const float* rays,
                             const float* ts, int N, int S, float near, float far, float* rgb_map,
                             float* depth_map, void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- the eval chunk loop of renderer.py:740-812 (chunk = 512 rays, renderer.py:732) as one native call: the launch
 * sequences of the chunks are issued round-robin on `nstreams` caller streams (0: all on main_stream), which first wait for
 * main_stream and which main_stream finally waits for.  Both parameter structs must carry packed_fwd; ws: nstreams slices of
 * rdrf_render_workspace_bytes(chunk, S) (rdrf_render_chunks_workspace_bytes).  Same bits as rdrf_render_fwd per chunk. */
size_t rdrf_render_chunks_workspace_bytes(int chunk, int S, int nstreams);
int rdrf_render_chunks_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                           const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, int chunk,
                           float near, float far, float* rgb_map, float* depth_map, void* ws, size_t ws_bytes,
                           rdrf_stream_t main_stream, const rdrf_stream_t* streams, int nstreams);

/* ---- decomposed maps of the no-grad render (the eval loop keeps seven maps per frame, renderer.py:745-826) ------------
 * One nullable DEVICE pointer per per-ray output of raw2outputs (renderer.py:173-315; the three per-sample weight planes
 * are not offered).  NULL = not wanted: that output goes to the workspace, as with the entry points above.  The same
 * workspace sizes apply (rdrf_render_workspace_bytes, rdrf_render_chunks_workspace_bytes), and every requested map has
 * the bits the corresponding output of rdrf_composite_fwd has after the fields' forward. */
typedef struct RdrfRenderMaps {
  float* rgb;        /* rgb_map_full[N][3] */
  float* depth;      /* depth_map_full[N] */
  float* acc;        /* acc_map_full[N] */
  float* rgb_s;      /* rgb_map_s[N][3] */
  float* depth_s;    /* depth_map_s[N] */
  float* acc_s;      /* acc_map_s[N] */
  float* rgb_d;      /* rgb_map_d[N][3] */
  float* depth_d;    /* depth_map_d[N] */
  float* acc_d;      /* acc_map_d[N] */
  float* blending;   /* dynamicness_map[N] */
} RdrfRenderMaps;
/* mode: the launch form of rdrf_render_fwd (AUTO), rdrf_render_sequence_fwd (SEQUENCE) or rdrf_render_fused_fwd (FUSED);
 * a barrier time-out of the fused form sets every requested map of the affected rays to NaN. */
enum { RDRF_RENDER_AUTO = 0, RDRF_RENDER_SEQUENCE = 1, RDRF_RENDER_FUSED = 2 };
int rdrf_render_maps_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                         const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near, float far,
                         int mode, const RdrfRenderMaps* maps, void* ws, size_t ws_bytes, rdrf_stream_t stream);
/* the chunk loop of rdrf_render_chunks_fwd (same streams, same coalescing) with every non-NULL map offset per chunk */
int rdrf_render_chunks_maps_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, int chunk,
                                float near, float far, const RdrfRenderMaps* maps, void* ws, size_t ws_bytes,
                                rdrf_stream_t main_stream, const rdrf_stream_t* streams, int nstreams);

/* ---- the no-grad render of world-space rays (cfg->ray_type == RDRF_RAY_OTHER: sampler rdrf_sample_world, no far-plane
 * depth term) -- the one entry point of the whole family for this ray type, because its sampler needs the field's `step`
 * and RdrfFieldCfg carries none; the entry points above refuse RDRF_RAY_OTHER.  chunk <= 0: rdrf_render_maps_fwd with
 * `mode` on main_stream (streams / nstreams are not read).  chunk > 0: rdrf_render_chunks_maps_fwd (the launch sequence;
 * `mode` is not read).  Same workspace sizes, same bits in every map as rdrf_composite_fwd after the fields' forward. */
int rdrf_render_world_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                          const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, int chunk, float near,
                          float far, float step, int mode, const RdrfRenderMaps* maps, void* ws, size_t ws_bytes,
                          rdrf_stream_t main_stream, const rdrf_stream_t* streams, int nstreams);

/* ---- motion maps of the no-grad render (the per-frame `render` of renderer.py:319-657 keeps, beside the maps above, four
 * induced optical-flow maps and the warp displacement of every frame) --------------------------------------------------
 * One nullable DEVICE pointer per map; NULL = not wanted, not computed (the scene-flow MLP runs only if flow_f or flow_b
 * is wanted).  Every map is reduced in a fixed order that depends on S alone: the same bits run after run, for any
 * chunking of the image, for any subset of requested maps, in every render mode and in the deterministic build. */
typedef struct RdrfMotionMaps {
  float* flow_f;     /* [N][2] induced flow to the next frame through scene_flow_f   (renderer.py:493-503) */
  float* flow_b;     /* [N][2] ... to the previous frame through scene_flow_b        (:504-514) */
  float* flow_s_f;   /* [N][2] static field, camera motion only, next frame          (:516-526) */
  float* flow_s_b;   /* [N][2] ... previous frame                                    (:527-537) */
  float* delta_xyz;  /* [N][3] sum_s weights_d (xyz_prime - xyz), raw               (:460, :610) */
} RdrfMotionMaps;
typedef struct RdrfMotionCams {
  int H, W;
  const float* focal;     /* DEVICE, one float (as rdrf_induce_flow_fwd) */
  const float* c2w_f;     /* DEVICE [3][4]: pose of the next frame, one for all rays */
  const float* c2w_b;     /* DEVICE [3][4]: pose of the previous frame */
  int64_t first_pixel;    /* ray k is flat pixel first_pixel + k of the H x W image: pts_2d = (p % W, p / W % H), the
                             reference's integer meshgrid (renderer.py:372-375) */
} RdrfMotionCams;
/* rdrf_render_maps_fwd (same `mode`, same bits in every requested RdrfRenderMaps entry; `maps` may be NULL), then the
 * motion kernel on the same workspace and stream.  A barrier time-out of the fused form sets the motion maps to NaN as
 * well.  ws: rdrf_render_motion_workspace_bytes(N, S) (>= rdrf_render_workspace_bytes(N, S)). */
size_t rdrf_render_motion_workspace_bytes(int N, int S);
int rdrf_render_motion_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                           const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near, float far,
                           int mode, const RdrfRenderMaps* maps, const RdrfMotionCams* cams, const RdrfMotionMaps* motion,
                           void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- flow_viz.flow_to_image with its defaults (flow_viz.py:107-136: no clip, RGB; the Middlebury colour wheel) --------
 * flow [H][W][2] fp32 -> rgb [H][W][3] uint8, both on the DEVICE; the flow is not modified.  +-inf entries count as 0,
 * a NaN entry makes the radius maximum NaN and with it every pixel white, as in numpy.  numpy's precision sequence: fp32
 * up to the wheel position, fp64 for the colour mix.  ws: rdrf_flow_to_image_workspace_bytes(H, W). */
size_t rdrf_flow_to_image_workspace_bytes(int H, int W);
int rdrf_flow_to_image(const float* flow, int H, int W, uint8_t* rgb, void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- point tracks: the scene-flow field chained across frames (no-grad) ----------------------------------------------
 * M seed points p0[M][3] (un-normalised field coordinates, as rdrf_scene_flow_fwd takes them) at times t0[M] in [-1,1]
 * are followed n_fwd frames forward and n_bwd frames backward, K = n_bwd + 1 + n_fwd slots per point, slot n_bwd = the seed:
 *     forward   p_{k+1} = p_k + scene_flow_f(p_k, t_k),  t_{k+1} = t_k + dt
 *     backward  p_{k-1} = p_k + scene_flow_b(p_k, t_k),  t_{k-1} = t_k - dt       (dt = 2 / (T - 1) for a T-frame video)
 * fp32, no contraction; cfg_d->ray_type contract clamps every sum to [-2 + 1e-6, 2 - 1e-6] (train.py:1377-1378); ndc or
 * contract only.  A step's scene flow has rdrf_scene_flow_fwd's bits for that point and time, so a track equals the chain of
 * single calls bit for bit, and does not depend on M or on which other points share the call.
 * cams (nullable): camera k of slot k.  pix = render_single_3d_point's pixel coordinates of p_k in camera k
 * (renderer.py:1299-1325; contract: render_3d_point's contract2world leg, :1351-1366); disp = its second output, (z_ndc + 1) / 2
 * for ndc, z_ndc for contract.  One nullable DEVICE pointer per output; pix / disp need `cams`.
 * ws: rdrf_track_ws_bytes(M, K) (the pack area; not read when PD->packed_fwd is given).  M == 0 is a no-op. */
typedef struct RdrfTrackCams {
  int H, W;
  int K;                  /* number of cameras: must equal n_bwd + 1 + n_fwd */
  const float* focal;     /* DEVICE, one float (as rdrf_induce_flow_fwd) */
  const float* c2w;       /* DEVICE [K][3][4] */
} RdrfTrackCams;
typedef struct RdrfTracks {
  float* pts;    /* [M][K][3] */
  float* pix;    /* [M][K][2] */
  float* disp;   /* [M][K] */
} RdrfTracks;
size_t rdrf_track_ws_bytes(int M, int K);
int rdrf_track_points_fwd(const RdrfDynamicParams* PD, const RdrfFieldCfg* cfg_d, const float* p0, const float* t0, int M,
                          int n_fwd, int n_bwd, float dt, const RdrfTrackCams* cams, const RdrfTracks* out, void* ws,
                          size_t ws_bytes, rdrf_stream_t stream);
/* rdrf_render_maps_fwd (the launch sequence; same bits in every requested RdrfRenderMaps entry, `maps` may be NULL), then
 * seeds[N][3] = sum_s weights_d xyz + (1 - acc_d) far from the render's workspace: the first half of render_3d_point
 * (renderer.py:1333-1345, far point per ray type), the point a track of that pixel starts from.  ndc or contract.
 * ws: rdrf_render_motion_workspace_bytes(N, S). */
int rdrf_render_track_seeds_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near,
                                float far, const RdrfRenderMaps* maps, float* seeds, void* ws, size_t ws_bytes,
                                rdrf_stream_t stream);
/* Per-slot visibility of a track: vis[M][K], the transmittance T_full of raw2outputs (renderer.py:236-245) from camera k to
 * the point p = pts[i][k] (field coordinates, as rdrf_track_points_fwd writes them).  No-grad; ndc or contract only.
 *   time    t_k: t0[i] stepped by dt as rdrf_track_points_fwd steps it (one rounded sum per step), so it has the chain's bits.
 *   ray     world = NDC2world(p) (ndc) or contract2world(p) (contract), cam = R_k^T (world - c_k): the arithmetic of pix above.
 *           The slot's ray is camera k's ray through the slot's own fractional pixel pix[i][k]: origin c_k, direction
 *           R_k ((u - W/2) / f, -(v - H/2) / f, -1), for ndc followed by ndc_rays_blender with near = 1 -- rdrf_camera_rays'
 *           arithmetic at (u, v) in the place of a pixel centre.
 *   depth   z* = (clamp(p_z, -1, 1 - 1e-6) + 1) / 2 for ndc, -cam_z for contract: where the point lies on that ray in z_vals
 *           units.  The query depth is zq = z* - margin; `margin` is the caller's, in z_vals units.  A seed made by
 *           rdrf_render_track_seeds_fwd sits INSIDE the density that defines it, so its value at margin = 0 is well below 1:
 *           a caller that wants "is the surface seen" picks a margin of a few sample steps.
 *   samples the field's no-jitter sampler for the ray type with S samples and (near, far): z_s, valid_s,
 *           dists_s = (z_{s+1} - z_s) |d| cfg_d->distance_scale (the last 0); sigma_s, sigma_d and blending of a sample have
 *           the bits rdrf_static_fwd / rdrf_dynamic_fwd give it on that ray at time t_k (0 where not valid).
 *   vis     with F_s(d) = (1 - (1 - exp(-sigma_d d)) b) (1 - (1 - exp(-sigma_s d)) (1 - b)) + 1e-10 and j the last sample
 *           with z_j <= zq:   vis = prod_{s < j} F_s(dists_s) * F_j(min(zq - z_j, z_{j+1} - z_j) |d| distance_scale).
 *           At zq = z_j this is T_full[j] of raw2outputs, formed in rdrf_composite_fwd's scan order; between samples it is
 *           continuous (the piecewise-constant density the compositor assumes); zq <= z_0 gives exactly 1.0, zq beyond the
 *           last sample the full product; a point behind its camera (cam_z >= 0) gives 0.0; a NaN depth gives NaN.  vis
 *           never rises with zq, bit for bit: where rounding would let the scan's T_full[j + 1] exceed T_full[j] F_j by an
 *           ulp, the running minimum of T_full is taken.  Pixels outside the frame are computed like any other: clipping
 *           to the frame is the caller's.
 * Only the samples with valid_s and z_s < zq reach a density kernel (the list kernels of rdrf_render_masked_fwd); no
 * appearance phase runs.  The product is formed in a fixed order that depends on S and j alone: a slot's bits do not depend
 * on M, on the other slots of the call or on the run, in the deterministic build too.
 * cams: required, cams->K == n_bwd + 1 + n_fwd.  ws: rdrf_track_visibility_ws_bytes(M, K, S); M * K * S * 3 < 2^31.
 * No allocation, no synchronisation.  M == 0 is a no-op. */
size_t rdrf_track_visibility_ws_bytes(int M, int K, int S);
int rdrf_track_visibility_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                              const RdrfFieldCfg* cfg_d, const float* pts, const float* t0, int M, int n_fwd, int n_bwd,
                              float dt, const RdrfTrackCams* cams, int S, float near, float far, float margin, float* vis,
                              void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- surface hits: per ray the depth at which the opacity 1 - T_full reaches a level tau (no-grad) ---------------------
 * The depth maps above are expected depths, sum_s w_s z_s: a blend that lies between foreground and background at an
 * occlusion edge and inside a semi-transparent floater.  A hit is where the ray's transmittance falls to L = 1 - tau
 * (tau = 0.5: the median depth).  For one ray with samples z_0 < ... < z_{S-1}, dists_s = (z_{s+1} - z_s) |d| distance_scale
 * (the last 0; ndc, contract: |d| the norm of the ray's direction), sigma_s, sigma_d, blending b:
 *   factor  F_s(d) = (1 - (1 - exp(-sigma_d d)) b) (1 - (1 - exp(-sigma_s d)) (1 - b)) + 1e-10, the one of the visibility above
 *   T_s     T_full[s] of raw2outputs as rdrf_composite_fwd forms it (rounds of 64 samples, Hillis-Steele product scan, carry)
 *   m_s     min_{i <= s} T_i, the running minimum rdrf_track_visibility_fwd takes: it never rises with s, bit for bit
 *   level   L = 1 - tau, rounded once in fp32
 *   sample  j = the first s < S - 1 with m_{s+1} <= L.  (The last sample has no width and the factor 1 + 1e-10: it cannot be
 *           the first to cross and is not looked at.)  None: the ray is a MISS.
 *   depth   z_hit = min(z_j + t (z_{j+1} - z_j), z_{j+1}) with t = the smallest fp32 number in [0, 1] at which
 *           m_j F_j(t dists_j) <= L in the compositor's own fp32 arithmetic (t = 1 counts as crossed, the scan having said
 *           so; t = 0 where m_j <= L already, which happens at j = 0 or through the 1e-10).  It is found by a 64-section over
 *           the bit pattern of t, 5 rounds whatever the data; t is exact to one ulp of ITSELF, so the transmittance at z_hit
 *           equals L to rounding however steep the density.  F_j does not rise with d, so z_hit does not fall as tau rises.
 *   xyz     the sampler's own arithmetic for the ray type (rdrf_sample_ndc / rdrf_sample_contract) at depth z_hit in the place
 *           of a sample's z: field coordinates; for z_hit == z_s the bits of that sample's xyz
 *   owner   a_d b / (a_d b + a_s (1 - b)) with a = 1 - exp(-sigma dists_j) of the hit sample, 0 where the denominator is 0:
 *           the dynamic field's share -- 1 a moving surface, 0 the static scene
 *   miss    hit = 0, z = z_{S-1}, xyz = the last sample's point, owner = 0
 *   NaN     a NaN in sigma_s, sigma_d, blending or z of a sample at or before the one a level would cross in: hit = 0 and NaN
 *           in z, xyz and owner of that level; a NaN behind the crossing has no effect
 * taus[n_tau]: HOST array, 1 <= n_tau <= 8, each in (0, 1), strictly ascending; all are answered from one scan of the ray.
 * RdrfHits: DEVICE pointers, each nullable (not wanted: not written), level-major.
 * Bit for bit: z_j <= z_hit <= z_{j+1}; z_hit does not fall and hit does not rise as tau rises; a ray's outputs do not depend
 * on N, on the other rays or levels of the call, on the run or on the build (the deterministic library included): every
 * product is formed in an order that depends on S and j alone.  No allocation, no synchronisation; N == 0 is a no-op. */
typedef struct RdrfHits {
  float* z;        /* [n_tau][N] */
  uint8_t* hit;    /* [n_tau][N] 0 / 1 */
  float* xyz;      /* [n_tau][N][3] */
  float* owner;    /* [n_tau][N] */
} RdrfHits;
/* the kernel alone, on the caller's planes: rays [N][6], z, sigma_s, sigma_d, blending [N][S] (device); ray_type ndc or
 * contract (it selects |d| and the point's arithmetic); N * S * 3 < 2^31 */
int rdrf_hits_from_planes(const float* rays, const float* z, const float* sigma_s, const float* sigma_d, const float* blending,
                          int N, int S, int ray_type, float distance_scale, const float* taus, int n_tau, const RdrfHits* out,
                          rdrf_stream_t stream);
/* The hits of rendered rays: z and valid of the field's no-jitter sampler for (near, far), sigma_s, sigma_d and blending with
 * the bits rdrf_static_fwd / rdrf_dynamic_fwd give the samples at the rays' times, distance_scale = cfg_d's.
 *   maps != NULL  rdrf_render_maps_fwd as the launch sequence (same bits in every requested RdrfRenderMaps entry), then the
 *                 hits from the render's own planes
 *   maps == NULL  the density-only path: sampler, time branch, both list-driven density kernels of rdrf_render_masked_fwd on
 *                 every valid sample, the hits; no appearance phase
 * Both paths give the same bits in every RdrfHits output.  ndc or contract only (alpha masks and world-space rays are not
 * built here).  ws: rdrf_render_hits_ws_bytes(N, S); N * S * 3 < 2^31.  Every check comes before any device work. */
size_t rdrf_render_hits_ws_bytes(int N, int S);
int rdrf_render_hits_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                         const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near, float far,
                         const float* taus, int n_tau, const RdrfRenderMaps* maps, const RdrfHits* out, void* ws,
                         size_t ws_bytes, rdrf_stream_t stream);

/* ---- rays of arbitrary cameras (evaluation_path, renderer.py:1013-1030; evaluation, :702-716) -----------------------
 * c2w[B][3][4] camera-to-world matrices, focal[B] per camera.  Ray k is flat pixel first + k over (B, H, W):
 * get_ray_directions_blender (pixel centre + 0.5, centre (W/2, H/2), focal on both axes, dataLoader/ray_utils.py:93-110),
 * get_rays (:143-160, world rays, unnormalised directions) and, if ndc != 0, ndc_rays_blender with `near` (:197-218).
 * rays[N][6]; first + N <= B H W. */
int rdrf_camera_rays(const float* c2w, const float* focal, int B, int H, int W, int ndc, float near, int64_t first, int N,
                     float* rays, rdrf_stream_t stream);

/* ---- SSIM of two images (rgb_ssim, utils.py:98-151, with its defaults: 11-tap Gaussian, sigma 1.5, k1 = 0.01,
 * k2 = 0.03) ----------------------------------------------------------------------------------------------------------
 * img0, img1 [H][W][C] fp32, H, W >= 11.  The five moments and the map are accumulated in fp64 (the reference's
 * float64 filter upcasts); *mean_out (one DEVICE double) = the mean of the map; map_out (nullable) [H-10][W-10][C] fp32.
 * The mean is reduced in a fixed order: the same bits run after run.  ws: rdrf_ssim_workspace_bytes(H, W, C). */
size_t rdrf_ssim_workspace_bytes(int H, int W, int C);
int rdrf_ssim(const float* img0, const float* img1, int H, int W, int C, float max_val, double* mean_out, float* map_out,
              void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- batch assembly of a device-resident training set (train.py:1043-1060: `allrgbs[ray_idx]`, `alldisps[ray_idx]`,
 * `allflows_f[ray_idx]`, ... one index launch per tensor there) -----------------------------------------------------------
 * The per-pixel tables of T frames of H x W pixels, flat over (T, H, W); total = T H W, T >= 2.  Pixel centre, integer
 * pixel, frame and time are not stored: they are arithmetic on the index (ids2pixel, train.py:96-103). */
typedef struct RdrfSceneTables {
  int T, H, W;
  int rgb_u8;            /* 1: rgb is uint8 [total][3], converted as (float)x / 255.0f; 0: fp32 [total][3] */
  const void* rgb;
  const float* disp;     /* [total]; NULL: the batch's disp is zeros */
  const float* flow_f;   /* [total][2], pixels, 8-byte aligned */
  const float* flow_b;
  const uint8_t* masks;  /* [total]: bit 0 foreground mask, bit 1 forward flow mask, bit 2 backward flow mask; a scene
                            without a foreground mask leaves bit 0 clear (the batch's fg is zeros) */
} RdrfSceneTables;
/* Everything one iteration reads of its N rays; every pointer is required. */
typedef struct RdrfBatch {
  float* rgb;      /* [N][3] */
  float* disp;     /* [N] */
  float* fg;       /* [N] 0 / 1 */
  float* mask_f;   /* [N] 0 / 1 */
  float* mask_b;   /* [N] 0 / 1 */
  float* flow_f;   /* [N][2], 8-byte aligned (as flow_b, grid, px) */
  float* flow_b;   /* [N][2] */
  float* ts;       /* [N] (float)view * (float)(2.0 / (T - 1)) - 1.0f */
  float* ts_rand;  /* [N] the same of ids2: the second, independent sampler's times (train.py:1011-1012) */
  float* grid;     /* [N][2] pixel centre (col + 0.5, row + 0.5) */
  float* px;       /* [N][2] integer pixel (col, row): `allgrids` (train.py:983-988) */
  int64_t* view;   /* [N] frame index id / (H W) */
} RdrfBatch;
/* ONE launch writes every tensor of `out` for the flat pixel indices ids[N] (and ts_rand for ids2[N]).  Each fp32
 * operation is rounded on its own, in the order above: the values are bit-identical to gathers from fp32 tables built
 * with those expressions.  An index outside [0, total) is UNDEFINED (not checked: the indices live on the device and no
 * entry point synchronises).  N = 0 is a no-op that touches nothing. */
int rdrf_gather_batch(const RdrfSceneTables* tables, const int64_t* ids, const int64_t* ids2, int N, RdrfBatch* out,
                      rdrf_stream_t stream);

/* ---- process-wide choice of the density / blending scatter of the dynamic field's backward (models/tensoRF.py:646-811,
 * grid_sampler_2d_backward semantics either way): RDRF_SCATTER_RAY = ray tiles, RDRF_SCATTER_SORTED = samples grouped by
 * plane cell first (about 10x fewer memory-side atomic requests, a fixed grouping cost per launch), RDRF_SCATTER_AUTO
 * (default) = sorted from 300 k samples per launch.  The sorted density / blending passes form their plane sums in LDS
 * windows (k_scatter_tiled) wherever those fit beside two workgroups per CU; RDRF_SCATTER_SORTED_PLAIN forces the sorted
 * path WITHOUT the windows (every run tail goes to global memory: the form large grids fall back to), so that both forms
 * can be held to the same parity tests at any size.  Returns 0, or -1 for an unknown mode. */
int rdrf_set_scatter_mode(int mode);

/* ---- deterministic debugging build (librodynrf_det.so = the same sources with -DRDRF_DETERMINISTIC) ----------------
 * Every addition into a BOUND flat gradient buffer (scatter of the VM factors, line flushes, dW / bias sums, time
 * branch) goes to a 64-bit fixed-point shadow of that buffer (value * 2^40, integer atomics: order-independent) and
 * rdrf_det_finish adds the shadow into the fp32 gradients and clears it; the compaction lists of the appearance
 * phases are sorted, LDS line accumulators are bypassed.  Result: bit-identical parameter gradients run after run,
 * within fp32 rounding of the product build's.  rdrf_deterministic() = 1 in that build, 0 in the product build
 * (where bind / finish fail).  slot 0 = static field, 1 = dynamic field; shadow: n 64-bit words, zero-initialised. */
int rdrf_deterministic(void);
int rdrf_det_bind(int slot, float* grad_base, size_t n, void* shadow_i64, rdrf_stream_t stream);
int rdrf_det_finish(int slot, rdrf_stream_t stream);

/* ---- kernel self-tests (used by tests/ only): run the MFMA layer chain on a synthetic input
 * and return it for comparison with a numpy matmul. x[M][K] -> y[M][OUT] = relu(x W^T + b). */
int rdrf_selftest_mlp(const float* x, const float* w, const float* b, int M, int K, int OUT,
                      float* y, void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* Every MLP layer primitive on its own, with the template arguments of the product kernels and the product's pack code; the
 * raw accumulators are returned (no bias, no relu).  w[OUT][K] is a torch.nn.Linear weight.  Forward forms: x[M][K] ->
 * y[M][OUT] = x w^T.  Transposed forms (_T, the backward-data product): x[M][OUT] -> y[M][K] = x w.  Instantiated (K, OUT):
 *   F32        fp32 MFMA, pack mode 0            (64, 64) (128, 128) (72, 32)
 *   F32_T      fp32 MFMA, mode 2                 (64, 64) (32, 128)
 *   B3         bf16 x 3, mode 7                  (144, 64): the heads' first layer, three segments in one image; (64, 64)
 *   B3_T       bf16 x 3, mode 8                  (64, 64)
 *   B3_PAIR_T  two images, one input, mode 8     (160, 64): y = 96 columns of image A, 64 of B; (96, 64): 64 + 32
 *   B3S        split storage, mode 9, as chains  (112, 128): 16 | 32 | 8 slots (dynamic appearance); (160, 128): 16 | 64 (static)
 *   B3S_T      split storage, mode 10            (224, 32) (96, 32) (128, 128) (96, 128) (160, 128)
 * Any other (form, K, OUT) returns -1.  M = 0 is a no-op.  ws: 16-byte aligned scratch, 128 KiB suffice for every form. */
#define RDRF_ST_F32 0
#define RDRF_ST_F32_T 1
#define RDRF_ST_B3 2
#define RDRF_ST_B3_T 3
#define RDRF_ST_B3_PAIR_T 4
#define RDRF_ST_B3S 5
#define RDRF_ST_B3S_T 6
int rdrf_selftest_layer(int form, const float* x, const float* w, int M, int K, int OUT, float* y, void* ws, size_t ws_bytes,
                        rdrf_stream_t stream);

/* The dW products (k_dw3 behind its host planner) on rows the caller supplies, with the job lists of the backward entry points:
 * one plan per list.  A: dz rows [ntiles][A_stride][32], B: activation rows [ntiles][B_stride][32] (device, 16-byte aligned,
 * A_floats / B_floats long); a plan with two row regions (DYN, FEAT_DYN: the appearance rows, then the density-phase rows)
 * takes region 1 right behind the ntiles tiles of region 0, in both arrays.  count: nullable device sample count; the plans whose
 * entry point passes one (STATIC_*, DYN_APP, the appearance region of DYN) then walk ceil(count / 32) <= ntiles tiles.  flags:
 * the density phase's live heads and whether the small layers' gradients are formed by the backward-data kernel instead.
 * grads: RdrfStaticParams (STATIC_*, FEAT_STATIC) or RdrfDynamicParams of gradient pointers, added into.  Unknown plan: -1;
 * ntiles == 0 without a count the plan reads (STATIC_*, DYN_APP, DYN read it; the others ignore one): a no-op.
 * FEAT_DYN ignores RDRF_DW_SMALL_IN_KERNEL, as rdrf_dynamic_features_bwd always forms the small layers' gradients in k_dw3.
 * rdrf_selftest_dw_describe writes the plan's job list in resolved form to host memory (layout: csrc/rdrf_selftest.hip) and
 * returns the number of ints written; -3 when cap is too small. */
#define RDRF_DW_DENSITY 0
#define RDRF_DW_STATIC_FEA 1
#define RDRF_DW_STATIC_TE 2
#define RDRF_DW_DYN_APP 3
#define RDRF_DW_DYN 4
#define RDRF_DW_SCENE_FLOW 5
#define RDRF_DW_FEAT_STATIC 6
#define RDRF_DW_FEAT_DYN 7
#define RDRF_DW_LIVE_D 1
#define RDRF_DW_LIVE_B 2
#define RDRF_DW_SMALL_IN_KERNEL 4
#define RDRF_DW_WARP_IN_KERNEL 8 /* density phase: the warp MLP's layer3 / layer4 gradients are formed by the backward-data kernel */
int rdrf_selftest_dw(int plan, int flags, const float* A, size_t A_floats, const float* B, size_t B_floats, int ntiles,
                     const int* count, const void* grads, rdrf_stream_t stream);
int rdrf_selftest_dw_describe(int plan, int flags, int* out, int cap);
/* The kernel launches the host planner makes for a plan's job list at ntiles (>= 1) tiles, in resolved form (layout:
 * csrc/rdrf_selftest.hip): grid, LDS bytes, accumulator sets, the runs of consecutive rows, the staged blocks and every wave's
 * products.  Host code only: runs without a GPU.  Returns the number of ints written; -3 when cap is too small. */
int rdrf_selftest_dw_plan(int plan, int flags, int ntiles, int* out, int cap);
/* launch geometry of the scene-flow backward kernel that forms its weight gradients itself, for ntiles 32-sample tiles:
 * workgroups and waves per workgroup (a wave walks the tiles wg * waves + wave, + grid * waves, ...).  Host code only. */
int rdrf_selftest_sf_geometry(int ntiles, int* grid, int* waves);
/* the same for the warp MLP backward kernel of the flat training path */
int rdrf_selftest_warp_geometry(int ntiles, int* grid, int* waves);
/* The warp MLP backward of the flat training path alone (what rdrf_dynamic_bwd runs between the density scatter and the time
 * branch), on rows the caller supplies: act1 [T][576][32] saved density-phase rows (X0, T, H3, H4 are read), grows1 [T][544][32]
 * gradient rows (the d(X0) rows of the heads are read, the small-layer rows 0..2 written), T = ceil(N S / 32) flat tiles; dxw /
 * dxn [N S][3] coordinate gradients arriving from the appearance phase and the scatter; g_xyz_prime [N S][3] nullable.
 * Added into: g_xyz [N S][3] (nullable) and, of grads, warp layers 3, 4, 5 (weights and biases).  Written: dtout [N][32] for
 * the rays inside one tile, dtp [T][2][32] for the others (both must be pre-filled by a caller that compares them whole).
 * ws: 16-byte aligned scratch of rdrf_selftest_warp_bwd_workspace_bytes(N, S). */
size_t rdrf_selftest_warp_bwd_workspace_bytes(int N, int S);
int rdrf_selftest_warp_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, int N, int S, const float* act1,
                           size_t act1_floats, float* grows1, size_t grows1_floats, float* dxw, float* dxn,
                           const float* g_xyz_prime, const RdrfDynamicParams* grads, float* g_xyz, float* dtout, float* dtp,
                           void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* The radix sort of the sorted scatter as the product calls it: keys [n] (the low `bits` bits are sorted on) -> keys_out ascending
 * and stable, order[i] = original position of keys_out[i].  count (nullable, device): only the first min(n, n_mul * *count) entries
 * are sorted and written; the rest of keys_out / order is left alone.  temp: 256-byte aligned, rdrf_selftest_sort_temp_bytes(n, bits).
 * n = 0 is a no-op. */
size_t rdrf_selftest_sort_temp_bytes(unsigned n, int bits);
int rdrf_selftest_sort(const unsigned* keys, unsigned n, int bits, const int* count, unsigned n_mul, unsigned* keys_out,
                       unsigned* order, void* temp, size_t temp_bytes, rdrf_stream_t stream);

/* The segmented form (the product's: the three planes' keys are three segments): nseg independent stable sorts of seg_len consecutive
 * entries over the low `bits` bits, the bits above ride along; order = GLOBAL positions segment * L + index.  count (nullable,
 * device): segments are L = min(seg_len, *count) entries long and L apart; entries beyond nseg * L are left alone.  temp: 256-byte
 * aligned, rdrf_selftest_sort_seg_temp_bytes.  rdrf_selftest_sort_describe (host only) writes the plan: [0] values used, [1] passes,
 * [2] bits per digit, [3] tiles per segment, [4] entries per tile, [5] bytes carved from temp, [6] the temp-size formula, [7] launches
 * of such a sort, [8] launches of a sorted-scatter call (key kernel + sort); returns the values written, -1 / -3 on bad arguments. */
size_t rdrf_selftest_sort_seg_temp_bytes(int nseg, unsigned seg_len, int bits);
int rdrf_selftest_sort_seg(const unsigned* keys, int nseg, unsigned seg_len, int bits, const int* count, unsigned* keys_out,
                           unsigned* order, void* temp, size_t temp_bytes, rdrf_stream_t stream);
int rdrf_selftest_sort_describe(int nseg, unsigned seg_len, int bits, unsigned long long* out, int cap);

/* The gradient scatter (VM gather backward) on data the caller supplies, through the launch functions of the backward entry
 * points: kind = one of the four instantiations in use, mode = RDRF_SCATTER_RAY (ray / flat / list tiles), _SORTED (samples
 * grouped by plane cell: key generation, sort and counts, then the windowed passes where the launch policy takes them) or
 * _SORTED_PLAIN (the same without windows); the dynamic kinds have the sorted modes.  Layouts: rdrf_selftest_scatter_describe
 * (csrc/rdrf_selftest.hip).  -1 bad arguments, -2 a mode or tile form the kind does not have, -3 a buffer too small. */
#define RDRF_SCK_STATIC_DENSITY 0 /* k_scatter<4,1,3>:   row 0 broadcast, xyz + box, g_xyz */
#define RDRF_SCK_DYN_DENSITY 1    /* k_scatter<4,1,9>:   density and / or blending by set mask, ray or flat tiles, dxw added */
#define RDRF_SCK_STATIC_APP 2     /* k_scatter<12,3,9>:  list + device count, xyz + box, g_xyz */
#define RDRF_SCK_DYN_APP 3        /* k_scatter<12,3,27>: list + device count, xw, dxw written (ray) / added (sorted) */
typedef struct {
  RdrfVM vm[2], gvm[2];       /* factor values and gradient buffers (same sizes and strides); set 1: blending (DYN_DENSITY only) */
  int set_mask;               /* DYN_DENSITY: bit 0 density, bit 1 blending */
  int N, S, flat;             /* flat: the tiles are 32-sample tiles of the [N S] array (DYN_DENSITY) */
  const float* coords;        /* [N S][3]: xyz (static kinds) or normalised xw (dynamic kinds) */
  float box_lo[3], box_inv[3];
  const unsigned char* valid; /* [N S] */
  const int* list;            /* appearance kinds: sample ids + device count */
  const int* count;
  const float* rows;          /* ray modes: d(feature) rows [tiles][stride][32]; DYN_DENSITY sorted: the liveness rows are read */
  size_t rows_floats;
  const float* recs;          /* sorted modes: sample-major records [N S][rec_floats] */
  size_t recs_floats;
  float* dxw;                 /* [N S][3] */
  float* g_xyz;               /* [N S][3] */
  void* ws;                   /* sorted modes: 256-byte aligned, rdrf_selftest_scatter_workspace_bytes(N, S) */
  size_t ws_bytes;
  unsigned* keys_out;         /* sorted modes, nullable: [3 N S] keys as generated, [3 N S] sorted keys, [3 N S] order, [3] live entries per plane */
  unsigned* keys_sorted_out;
  unsigned* order_out;
  int* counts_out;
} RdrfScatterTest;
size_t rdrf_selftest_scatter_workspace_bytes(int N, int S);
int rdrf_selftest_scatter(int kind, int mode, const RdrfScatterTest* t, rdrf_stream_t stream);
/* host only: the kind's layouts / the launch decisions of the most recent scatter as ints; return the number written, -3 when cap
 * is too small.  grid: nullable {W, H} of the three level-0 planes, for the key layout. */
int rdrf_selftest_scatter_describe(int kind, const int* grid, int* out, int cap);
int rdrf_selftest_scatter_last(int* out, int cap);

/* The forward VM gather with shared taps on points the caller supplies, through the device functions of the forward kernels
 * unchanged (one wave per 32 points, lane = 32 h + s as there).  kind = RDRF_SCK_*: STATIC_DENSITY static_density_feature, one
 * float per point; STATIC_APP gather_level_app at level 0, 72 features; DYN_DENSITY gather_level_den at levels 0, 1, 2 as the
 * density / blending heads call it, 72 features; DYN_APP gather_level_app at levels 0, 1, 2, 216 features.  xn [M][3] normalised
 * coordinates (any float, non-finite included: every address is clamped).  out [nsets][M][features], the raw products in logical
 * order [level][plane][component], moved there from the lane layout by the index maps that lay out the first-layer weight columns.
 * vm: nsets (1 or 2) factor sets of the kind's component counts on one grid, axes of at least one texel.  M = 0 is a no-op.
 *
 * rdrf_selftest_encodings: fill_x0 / fill_x1 per half-wave on (xn [M][3], t [M]) -> x0_out [M][64] = [xn 3 | sin(2^k xn_d), d-major,
 * k = 0..9 | cos likewise | t], x1_out [M][16] = [sin(2^k t), k = 0..7 | cos likewise]: the column order of the heads' first layer. */
int rdrf_selftest_gather(int kind, const RdrfVM* vm, int nsets, const float* xn, int M, float* out, rdrf_stream_t stream);
int rdrf_selftest_encodings(const float* xn, const float* t, int M, float* x0_out, float* x1_out, rdrf_stream_t stream);

/* The per-field ray scan on arrays the caller supplies, through the kernels and the launch geometry of the entry points.
 * rdrf_selftest_ray_scan: sigma [N][S] -> dists -> alpha -> transmittance scan -> weight, the appearance-mask compaction and the zero
 * fill of the colours.  width 32: k_ray_scan (the dynamic field's flat density phase), width 64: k_static_scan (the per-ray half of
 * the static field's density kernel).  rays [N][6], z [N][S]; weight, dists [N][S]; list: the flat indices of the samples with
 * weight > weight_thres, appended from *counter on (the counter is ADDED to; ascending within a ray, rays in arrival order); rgb
 * (nullable) [N][S][3] is zeroed.
 * rdrf_selftest_ray_scan_bwd: the same scan backward.  width 32: k_ray_scan_bwd, raw [N][S][2] (the density head's output in slot
 * 0), out = gsig [N][S], the total d(sigma) of every sample.  width 64: k_static_density_bwd, raw [N][S], out = gf rows
 * [N][32 ceil(S / 32)], d(density feature) = d(sigma) act'(raw) at valid samples and 0 elsewhere (padding columns untouched).
 * sigma = valid ? act(raw) : 0 (act = RDRF_ACT_*).  g_weight, g_sigma, g_dists [N][S]: nullable cotangents; g_z [N][S], g_rays [N][6]:
 * nullable, ACCUMULATED into (g_rays columns 3..5, ndc / contract rays only).
 * Both: N = 0 is a no-op; S in 1 .. 4096; -1 on bad arguments. */
int rdrf_selftest_ray_scan(int width, const float* rays, const float* z, const float* sigma, int N, int S, int ray_type,
                           float distance_scale, float weight_thres, float* weight, float* dists, int* list, int* counter,
                           float* rgb, rdrf_stream_t stream);
int rdrf_selftest_ray_scan_bwd(int width, const float* rays, const float* z, const uint8_t* valid, const float* raw, int N, int S,
                               int act, float density_shift, float distance_scale, int ray_type, const float* g_weight,
                               const float* g_sigma, const float* g_dists, float* out, float* g_z, float* g_rays,
                               rdrf_stream_t stream);

/* The heads' backward of the dynamic field's density phase alone (what the backward entry points run between the ray scan
 * backward and the density / blending scatter), on rows the caller supplies, with the entry points' launch geometry.
 * mode RDRF_HEADS_FLAT: k_dyn_density_bwd<0, false, true> on the T = ceil(N S / 32) flat tiles of [N][S], as rdrf_dynamic_bwd runs
 * it.  raw [N S][2] the heads' raw outputs, valid [N S], g_sigma [N S] the TOTAL d(sigma) of every sample (the ray scan backward's
 * output), g_blending [N S] nullable d(blending); live_d: the density head receives a gradient.  dfs (nullable) [N S][144]: the
 * d(feature) results go there as sample-major records instead of into the d(feature) rows.  The gradients of the two heads' second
 * layers (dw2, db2, bw2, bb2 of grads) are ADDED into.
 * mode RDRF_HEADS_FEAT: k_dyn_density_bwd<0, true> on T = ceil(N / 32) tiles of N points (S is ignored), as
 * rdrf_dynamic_features_bwd runs it.  g_sigma, g_blending [N]: nullable gradients of the RAW head outputs; raw, valid and live_d
 * are not read, dfs must be NULL, grads is left alone.
 * Both: cfg gives act and density_shift; act1 [T][576][32] saved density-phase rows (the two heads' hidden rows are read), grows1
 * [T][544][32] gradient rows, pre-filled by a caller that compares them whole: a live head writes its dz and d(feature) rows, the
 * d(X0) rows and the small-layer dz rows 3 and 4 are always written.  ws: 16-byte aligned scratch of
 * rdrf_selftest_heads_bwd_workspace_bytes(N, S).  N = 0 is a no-op; -1 on bad arguments, -3 when rows, records or workspace are too
 * small.  rdrf_selftest_heads_describe (host only): the launch geometry at this shape and the row offsets the other describe
 * functions do not report, as ints (layout: csrc/rdrf_selftest.hip); returns the number written. */
#define RDRF_HEADS_FLAT 0
#define RDRF_HEADS_FEAT 1
size_t rdrf_selftest_heads_bwd_workspace_bytes(int N, int S);
int rdrf_selftest_heads_describe(int mode, int N, int S, int* out, int cap);
int rdrf_selftest_heads_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, int mode, int N, int S, const float* act1,
                            size_t act1_floats, const float* raw, const uint8_t* valid, const float* g_sigma,
                            const float* g_blending, int live_d, float* grows1, size_t grows1_floats, float* dfs, size_t dfs_floats,
                            const RdrfDynamicParams* grads, void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* The dynamic field's time branch alone, through the launchers of the entry points.  rdrf_selftest_time_branch: ts [N] -> tout
 * [N][32] = W2 relu(W1 [t, sin(2^f t), cos(2^f t), f = 0..7] + b1) + b2 in columns 0..29, zero in columns 30 and 31 (k_time_branch,
 * 8 rays per workgroup); zero64: nullable block of 64 ints, cleared on the way.  rdrf_selftest_time_branch_bwd: dtout [N][32] and the
 * nullable partial records dtp [ceil(N S / 32)][2][32] of the flat tiles (dtp_floats long) -> the gradients of time_layer1 /
 * time_layer2 (l1w, l1b, l2w, l2b of grads), ADDED into (k_time_branch_bwd, 32 rays per workgroup).  With dtp a ray that crosses a
 * tile edge takes its d(tout) from the records of its tiles and a ray inside one tile from dtout; without, every ray from dtout.
 * N = 0 is a no-op; -1 on bad arguments, -3 when dtp is too small. */
int rdrf_selftest_time_branch(const RdrfDynamicParams* P, const float* ts, int N, float* tout, int* zero64, rdrf_stream_t stream);
int rdrf_selftest_time_branch_bwd(const RdrfDynamicParams* P, const float* ts, int N, int S, const float* dtout, const float* dtp,
                                  size_t dtp_floats, const RdrfDynamicParams* grads, rdrf_stream_t stream);

/* The backward-data kernels of the appearance phase alone (what the backward entry points run in front of the appearance scatter
 * and the appearance dW products), on saved rows the caller supplies, with the entry points' launchers and launch geometry.
 * field RDRF_APP_DYN: P is a RdrfDynamicParams (k_dyn_app_bwd); RDRF_APP_STATIC_FEA / RDRF_APP_STATIC_TE: P is a RdrfStaticParams
 * with the MLP_Fea / MLP_Fea_TimeEmbedding head (k_static_app_bwd); cfg gives the box, ray_type (RDRF_RAY_*) and the head come from
 * the arguments.
 * mode RDRF_APP_ROWS / RDRF_APP_RECORDS: the ray path over the compacted samples list[0 .. *count) of [N][S] (list [N S] and count
 * in device memory; the list is checked against N S on the host first).  act3 [T][rows][32], T = ceil(N S / 32): the saved
 * appearance rows, of which H2, H1 and X0 (dynamic) or P (static) are read -- finite in all 32 lanes of every tile read; rays
 * [N][6]; g_rgb [N S][3] nullable (then every dz is 0).  Written: the rows DZV, DZ2, DZ1, DF and DA of the first ceil(count / 32)
 * tiles of grows3 [T][544][32]; dynamic: dxn [N S][3] of the listed samples, and with RDRF_APP_RECORDS the d(app features) as
 * sample-major records dfa [count][216] INSTEAD of the DA rows (dfa non-null exactly then; dfa_floats >= N S 216); static: the
 * view-direction gradient ADDED into g_rays [N][6] columns 3..5 (nullable).
 * mode RDRF_APP_FEAT: N points (S is ignored), g_feat [N][27]: DF and DA rows of ceil(N / 32) tiles; act3, list, count, rays,
 * g_rgb, dxn and g_rays are not read or written.
 * ws: 16-byte aligned scratch of rdrf_selftest_app_bwd_workspace_bytes(N, S).  N = 0 is a no-op; -1 on bad arguments, -3 when rows,
 * records or workspace are too small.  rdrf_selftest_app_describe (host only): the launch geometry at this shape and the rows of a
 * tile, as ints (layout: csrc/rdrf_selftest.hip; record offsets: rdrf_selftest_scatter_describe); returns the number written. */
#define RDRF_APP_DYN 0
#define RDRF_APP_STATIC_FEA 1
#define RDRF_APP_STATIC_TE 2
#define RDRF_APP_ROWS 0
#define RDRF_APP_RECORDS 1
#define RDRF_APP_FEAT 2
size_t rdrf_selftest_app_bwd_workspace_bytes(int N, int S);
int rdrf_selftest_app_describe(int field, int mode, int N, int S, int* out, int cap);
int rdrf_selftest_app_bwd(const void* P, const RdrfFieldCfg* cfg, int field, int mode, int ray_type, int N, int S, const float* act3,
                          size_t act3_floats, const int* list, const int* count, const float* rays, const float* g_rgb,
                          const float* g_feat, float* grows3, size_t grows3_floats, float* dfa, size_t dfa_floats, float* dxn,
                          float* g_rays, void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- alpha volumes and alpha-grid masks (models/tensorBase.py:42-79 AlphaGridMask, :565-702) ----------------------------
 * A mask is the occupancy grid of updateAlphaMask, bit-packed exactly as `save` (:465-469) stores it: the bool volume of
 * logical shape (G2, G1, G0, T) flattened in C order, eight entries per byte, first entry in the most significant bit
 * (np.packbits) -- the buffer IS the checkpoint's "alphaMask.mask" payload.  grid = {G0, G1, G2} (x, y, z), aabb = the
 * mask's own box (min xyz, max xyz). */
typedef struct RdrfAlphaMask {
  const uint8_t* bits;
  int grid[3];
  int T;
  float aabb[6];
} RdrfAlphaMask;

/* compute_alpha (:684-702) for M points x T times: alpha[M][T] = 1 - exp(-sigma length), sigma what the field's forward
 * gives a sample at that un-normalised position and time (dynamic: warp -> density features at the warped point ->
 * density head -> feature2density; static: density features -> feature2density), bit for bit.  params: RdrfStaticParams
 * (dynamic = 0) or RdrfDynamicParams (dynamic = 1).  mask: nullable; a point whose mask sample at a time is <= 0 gets
 * sigma 0 there.  sigma: nullable [M][T].  The static field needs no workspace. */
size_t rdrf_compute_alpha_workspace_bytes(int M, int T);
int rdrf_compute_alpha(const void* params, int dynamic, const RdrfFieldCfg* cfg, const float* xyz, int M,
                       const float* times, int T, float length, const RdrfAlphaMask* mask, float* alpha, float* sigma,
                       void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* the native part of updateAlphaMask (:592-629): alpha [G0][G1][G2][T] is clamped to [0, 1], max-pooled 3 x 3 x 3 over
 * space per time slice (stride 1, padding 1) and thresholded (>= thres is occupied).  bits: ceil(G0 G1 G2 T / 8) bytes in
 * the layout of RdrfAlphaMask.  stats (7 x int64, device): the occupied count, then the min and the max lattice index
 * (ix, iy, iz) over all times; with a count of 0 the six indices are meaningless. */
int rdrf_alpha_mask_build(const float* alpha, int G0, int G1, int G2, int T, float thres, uint8_t* bits, int64_t* stats,
                          rdrf_stream_t stream);

/* AlphaGridMask.sample_alpha (:56-73): normalise by the mask's aabb, slice round((t + 1) / 2 (T - 1)) (half-way cases to
 * even; clamped to the slices), trilinear, align_corners, zero padding.  t: one device value for all points
 * (t_per_point = 0) or one per point. */
int rdrf_alpha_mask_sample(const RdrfAlphaMask* mask, const float* xyz, const float* t, int t_per_point, int64_t n,
                           float* out, rdrf_stream_t stream);
/* ray_valid &= alpha_mask for xyz [N][S][3], ts [N]: valid[N][S] keeps its 1 where mask0's or (nullable) mask1's sample
 * is > 0 -- the static and the dynamic occupancy together, one launch. */
int rdrf_alpha_mask_valid(const RdrfAlphaMask* mask0, const RdrfAlphaMask* mask1, const float* xyz, const float* ts, int N,
                          int S, uint8_t* valid, rdrf_stream_t stream);

/* ---- isosurface meshes: marching tetrahedra over one time slice of a dense volume ------------------------------------------
 * vol is [G0][G1][G2][T] (the alpha volume of getDenseAlpha, used in place; T = 1: a plain 3-D volume) and slice t_index is
 * meshed at `level`: a sample is inside iff v >= level.  Every lattice cube is cut into the six Kuhn tetrahedra
 * v0, v0 + e_a, v0 + e_a + e_b, v0 + (1,1,1); a lattice edge (3 axis edges, 3 face diagonals, the body diagonal; owned by its
 * lower end) with exactly one end inside carries one vertex at p_lo + t (p_hi - p_lo), t = (level - v_lo) / (v_hi - v_lo), lo
 * the outside end, lattice positions aabb_min + idx / (G - 1) (aabb_max - aabb_min).  Vertices come in ascending (point, edge
 * kind) order, faces in ascending (cube, tetrahedron, triangle) order, counter-clockwise seen from the outside (flip: the
 * reverse); no atomics, the same bits from every build.  normals (nullable): -grad v by central differences (one-sided at the
 * boundary) at the two ends, interpolated with t and normalised.  Shapes with a side below 2, with 7 G0 G1 G2 >= 2^31 or with
 * 12 (G0-1)(G1-1)(G2-1) >= 2^31 are refused before any launch (rdrf_iso_ws_bytes returns 0 for them).
 * rdrf_iso_count writes the per-point edge flags and the vertex / triangle prefixes into ws and counts = {vertices, faces}
 * (device); the caller reads the two counts, allocates, and hands the same ws to rdrf_iso_emit.  aabb6: host, min xyz then
 * max xyz.  rdrf_iso_ws_bytes does not carry the *_workspace_bytes suffix for the reason given at rdrf_render_masked_ws_bytes. */
size_t rdrf_iso_ws_bytes(int G0, int G1, int G2);
int rdrf_iso_count(const float* vol, int G0, int G1, int G2, int T, int t_index, float level, void* ws, size_t ws_bytes,
                   int64_t* counts, rdrf_stream_t stream);
int rdrf_iso_emit(const float* vol, int G0, int G1, int G2, int T, int t_index, float level, const float* aabb6, int flip,
                  const void* ws, float* verts, float* normals, int* faces, int64_t nv, int64_t nf, rdrf_stream_t stream);

/* ---- masked render: the no-grad render of a ray chunk that skips what the alpha-grid masks leave empty ------------------
 * The maps are those of: sample -> valid_s = valid & (mask_s > 0), valid_d = valid & (mask_d > 0) (rdrf_alpha_mask_valid with
 * one mask) -> rdrf_static_fwd with valid_s, rdrf_dynamic_fwd with valid_d -> rdrf_composite_fwd, bit for bit in every map;
 * the density phase of a field runs on the samples its mask keeps only (a kept-sample list per field, device-side lengths,
 * no host sync).  mask_s / mask_d: each nullable (that field keeps every sample the sampler marks valid), not both.
 * step > 0 exactly for the world-space march (ray_type RDRF_RAY_OTHER, as rdrf_render_world_fwd); all three ray types are
 * served.  kept (nullable, device, [2]): the lengths of the static and the dynamic list.  The per-sample xyz_prime of a
 * dropped sample is not written, so there are no motion maps on this path.  N == 0 is a no-op.
 * rdrf_render_masked_ws_bytes is the end offset of the entry point's own carve (whole 256-byte blocks; it holds
 * rdrf_render_workspace_bytes(N, S) and grows with N and S).  It does not carry the *_workspace_bytes suffix: those names are
 * the closed set whose values tests/test_workspace_sizes_cpu.py holds to a table recorded from an earlier library. */
size_t rdrf_render_masked_ws_bytes(int N, int S);
int rdrf_render_masked_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                           const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near, float far,
                           float step, const RdrfAlphaMask* mask_s, const RdrfAlphaMask* mask_d, const RdrfRenderMaps* maps,
                           int64_t* kept, void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- point queries: a field evaluated at M points off the rays -------------------------------------------------------------
 * Point i gets what the field's forward gives a sample at xyz[i] with valid = 1 whose ray has the time ts[i] (ts[0] with
 * t_per_point = 0) and the normalised view direction viewdirs[i], bit for bit: sigma after the density activation, rgb,
 * and for the dynamic field blending (after the sigmoid) and xyz_prime (un-normalised).  rgb is computed for every point: there
 * is no weight threshold off the rays, no alpha-mask lookup and no aabb test -- the caller filters.  viewdirs are used as given,
 * not normalised.  params: RdrfStaticParams (dynamic = 0; ts may be NULL) or RdrfDynamicParams (dynamic = 1).  Every output is
 * nullable; rgb == NULL skips the appearance phase (viewdirs may then be NULL); blending and xyz_prime belong to the dynamic
 * field.  M == 0 is a no-op; M above RDRF_QUERY_POINTS_MAX is refused (the kernels index points with 32-bit ints): query in
 * chunks.  No allocation, no synchronisation, no read-back: the call can be captured into a graph.  The size function is the
 * end offset of the entry point's own carve; it does not carry the *_workspace_bytes suffix for the reason given at
 * rdrf_render_masked_ws_bytes. */
#define RDRF_QUERY_POINTS_MAX (1 << 24)
size_t rdrf_query_points_ws_bytes(int dynamic, int M, int t_per_point);
int rdrf_query_points(const void* params, int dynamic, const RdrfFieldCfg* cfg, const float* xyz, int M, const float* ts,
                      int t_per_point, const float* viewdirs, float* sigma, float* rgb, float* blending, float* xyz_prime,
                      void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- mesh simplification: vertex clustering of an indexed triangle mesh on the device ----------------------------------------
 * verts [V][3] and faces [F][3] (int vertex indices) are device arrays; origin, cell and n are host arrays: a lattice of
 * n[0] x n[1] x n[2] cells of size cell[] from origin[].  The cell of a vertex is, per axis,
 * c = clamp(floor((v - origin) / cell), 0, n - 1), formed in fp32 without contraction; a coordinate for which
 * (v - origin) / cell >= 0 is false (NaN among them) goes to cell 0.  The vertices of one cell form a cluster; clusters ascend
 * by key (c0 n[1] + c1) n[2] + c2, their members by original index.  A cluster's position is the mean of its members: fp64 sums
 * in member order, one fp64 division, one rounding to fp32.  normals (nullable): summed in fp64, scaled by the largest component
 * and normalised in fp64, rounded once; a zero sum stays zero.  colors (nullable, [V][3] bytes): per channel
 * floor((2 sum + k) / (2 k)), the mean rounded half up.  A face is mapped through the clusters and kept iff its three clusters
 * differ (a face with an index outside [0, V) is dropped); kept faces keep their order and their winding.  Duplicate faces are
 * not merged.  drop_unreferenced: only the clusters that a kept face references are emitted (renumbered in ascending key order);
 * 0: every cluster.  No atomics on global memory; the same bits from every build.
 * rdrf_simplify_count writes counts = {V', F'} (device) and, where remap is given, remap[v] = the output index of vertex v's
 * cluster (-1: dropped); the caller reads the two counts, allocates, and hands the same ws to rdrf_simplify_emit with the same
 * V and F.  V == 0 or F == 0: counts = {0, 0}, nothing else is written.  Refused before any launch (rdrf_simplify_ws_bytes
 * returns 0 for them): n below 1, n[0] n[1] n[2] >= 2^31, V or F >= 2^31 (the vertex indices are ints and the lane index
 * blockIdx.x * 256 + threadIdx.x of the kernels is 32-bit); by rdrf_simplify_count also a cell size that is not positive and
 * finite.  The size function does not carry the *_workspace_bytes suffix for the reason given at rdrf_render_masked_ws_bytes. */
size_t rdrf_simplify_ws_bytes(int64_t V, int64_t F, const int n[3]);
int rdrf_simplify_count(const float* verts, int64_t V, const int* faces, int64_t F, const float origin[3], const float cell[3],
                        const int n[3], int drop_unreferenced, void* ws, size_t ws_bytes, int64_t* counts, int* remap,
                        rdrf_stream_t stream);
int rdrf_simplify_emit(const float* verts, const float* normals, const unsigned char* colors, int64_t V, const int* faces,
                       int64_t F, const void* ws, float* verts_out, float* normals_out, unsigned char* colors_out, int* faces_out,
                       int64_t nv, int64_t nf, rdrf_stream_t stream);

/* ---- whole-scene volumes: both fields at M points x T times, composed as the renderer composes a sample ---------------------
 * xyz[M][3] are un-normalised points (each field normalises them with its own box), times[T] a DEVICE array, every output
 * [M][T] and nullable: a null output is not written and, where that saves work, not computed (sigma_s alone: the dynamic
 * field is not evaluated; no alpha and no owner: the static field only for sigma_s; a head nobody reads is skipped).  Per
 * point and time, in fp32, in this order:
 *   sigma_d, blending   the bits rdrf_query_points gives the point at that time (fill_x0, load_tout, warp_mlp, warp_point,
 *                       head_raw<false>, head_raw<true>, density_act; the sigmoid 1 / (1 + expf(-f)) of k_point_dyn): the warp
 *                       is evaluated once for both heads
 *   sigma_s             the bits rdrf_query_points gives the static field (static_density_feature, density_act)
 *   masks               mask_s / mask_d (each nullable): a field whose mask sample at the point and time is <= 0 gets sigma 0
 *                       there, as in rdrf_compute_alpha; blending is not masked
 *   a_d = 1 - expf(-sigma_d * length),  a_s = 1 - expf(-sigma_s * length)       (rdrf_compute_alpha's expression)
 *   w_d = a_d * b,  w_s = a_s * (1 - b)
 *   alpha = 1 - (1 - w_d) * (1 - w_s)    one minus the compositor's per-sample factor WITHOUT its + 1e-10; no contraction
 *   owner = w_d / (w_d + w_s), 0 where the sum is 0: the owner of rdrf_render_hits_fwd
 * A NaN in sigma_s, sigma_d or blending of an entry gives NaN in alpha and owner of that entry and nowhere else.  No aabb test:
 * a point outside a field's box gets what rdrf_query_points gives it.  An entry depends on its own point and time only, not on
 * M, T, the other points, the outputs asked for, the run or the build: no atomics, the deterministic library runs the same
 * code.  No allocation, no synchronisation, no read-back: the call can be captured into a graph.  M == 0 is a no-op.  Refused
 * before any device work: M < 0, T < 1, every output null, M * T >= 2^31, a workspace below rdrf_scene_alpha_ws_bytes(M, T)
 * (which does not carry the *_workspace_bytes suffix for the reason given at rdrf_render_masked_ws_bytes). */
size_t rdrf_scene_alpha_ws_bytes(int M, int T);
int rdrf_scene_alpha(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                     const RdrfFieldCfg* cfg_d, const float* xyz, int M, const float* times, int T, float length,
                     const RdrfAlphaMask* mask_s, const RdrfAlphaMask* mask_d, float* alpha, float* owner, float* sigma_s,
                     float* sigma_d, float* blending, void* ws, size_t ws_bytes, rdrf_stream_t stream);

/* ---- texture atlases: a mesh turned into a point batch, a point batch into an RGB8 image --------------------------------------
 * A per-face atlas of fixed layout for an indexed triangle mesh on the device, verts [nv][3] (in the field's coordinates) and
 * faces [F][3] (int vertex indices, which the caller has checked: the kernels index verts with them).  q = the side of a square
 * in texels (RDRF_BAKE_TEXELS_MIN to _MAX), the atlas Wt >= q texels wide, R = Wt / q squares to a row.  Square s = f >> 1 has
 * its origin at ((s % R) q, (s / R) q) and holds face 2s where i + j <= q - 1 and face 2s + 1 elsewhere, (i, j) the texel's
 * indices inside the square.  The layout needs q ceil(ceil(F / 2) / R) rows; Ht may be larger.  A texel's barycentric weights,
 * in fp32:  lower  w1 = i / (q - 2), w2 = j / (q - 2);  upper  w1 = (q - 1 - i) / (q - 3), w2 = (q - 1 - j) / (q - 3);
 * w0 = (1 - w1) - w2; its point is (w0 v0 + w1 v1) + w2 v2, every operation rounded once (no contraction).  These are the
 * weights of the texel's centre (i + 0.5, j + 0.5) against the local corners  lower (0.5, 0.5), (q - 1.5, 0.5), (0.5, q - 1.5)
 * / upper (q - 0.5, q - 0.5), (2.5, q - 0.5), (q - 0.5, 2.5), so the diagonals i + j = q - 1 and i + j = q lie just outside
 * their triangles (w0 < 0) and a bilinear fetch at a UV inside a face's triangle reads texels of that face only.  The upper
 * half of the last square of an odd F, the squares from ceil(F / 2) on, the columns from R q on and rows past the layout's
 * belong to no face: point 0, direction (0, 0, 1), face -1, colour `fill`.
 * view: a HOST array of three floats handed to every texel as given, or NULL: minus the unit normal of the texel's face,
 * n = (v1 - v0) x (v2 - v0), -n / sqrt(n . n) in fp32; a face whose n . n is 0 or not finite takes (0, 0, 1).
 * rdrf_bake_texels is the geometry stage alone, in image order: points and viewdirs [Ht][Wt][3], face [Ht][Wt] (nullable).
 * rdrf_bake_texture evaluates one field (params / dynamic / cfg as rdrf_query_points; t: a DEVICE float, read by the dynamic
 * field) and writes tex [Ht][Wt][3] bytes, round-half-even(clamp(rgb, 0, 1) 255) with rgb the bits rdrf_query_points gives the
 * texel's point and direction; rdrf_bake_scene_texture forms rgb = o rgb_d + (1 - o) rgb_s first (four roundings), o the
 * `owner` of rdrf_scene_alpha at the point and time with the given length and masks.  A NaN colour gives 0.  The texels are
 * evaluated in chunks of chunk_squares whole squares (chunk_squares q q <= RDRF_QUERY_POINTS_MAX); the workspace,
 * rdrf_bake_ws_bytes(scene, dynamic, q, chunk_squares) (0 for a refused q or chunk; named *_ws_bytes for the reason given at
 * rdrf_render_masked_ws_bytes), depends on the chunk and not on the atlas, and a texel does not depend on the chunking.
 * fill: a HOST array of three bytes.  Every byte of tex is written exactly once per call; F == 0 writes `fill` everywhere and
 * touches no field.  No atomics, the deterministic library runs the same code; no allocation, no synchronisation, no
 * read-back.  Refused before any device work: q outside its range, Wt < q, Ht below the layout's, Wt Ht >= 2^31, null
 * pointers, a chunk outside its range, a workspace below the size call's. */
#define RDRF_BAKE_TEXELS_MIN 4
#define RDRF_BAKE_TEXELS_MAX 64
int rdrf_bake_texels(const float* verts, const int* faces, int F, int q, int Wt, int Ht, const float* view, float* points,
                     float* viewdirs, int* face, rdrf_stream_t stream);
size_t rdrf_bake_ws_bytes(int scene, int dynamic, int q, int chunk_squares);
int rdrf_bake_texture(const void* params, int dynamic, const RdrfFieldCfg* cfg, const float* verts, const int* faces, int F, int q,
                      int Wt, int Ht, const float* view, const float* t, const unsigned char* fill, int chunk_squares,
                      unsigned char* tex, void* ws, size_t ws_bytes, rdrf_stream_t stream);
int rdrf_bake_scene_texture(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                            const RdrfFieldCfg* cfg_d, const float* verts, const int* faces, int F, int q, int Wt, int Ht,
                            const float* view, const float* t, float length, const RdrfAlphaMask* mask_s,
                            const RdrfAlphaMask* mask_d, const unsigned char* fill, int chunk_squares, unsigned char* tex, void* ws,
                            size_t ws_bytes, rdrf_stream_t stream);

/* timing hook: average device time (ms) of the dominant kernel launches recorded with HIP events
 * since the last reset; used by bench.py for the roofline figure. */
void rdrf_prof_reset(void);
int rdrf_prof_enable(int on);
int rdrf_prof_get(const char* kernel, double* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif
