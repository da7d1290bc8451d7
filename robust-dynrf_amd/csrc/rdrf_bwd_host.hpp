// rdrf_bwd_host.hpp -- host interface between the backward entry points (rdrf_bwd.hip) and the units that launch the
// kernels they define: the gradient scatter (rdrf_scatter.hip), the dW products (rdrf_dw.hip) and the backward-data kernels
// that form their weight gradients themselves (rdrf_bwd_fused.hip).  Without relocatable device code a kernel is launched
// from the unit that defines it, so these are plain functions, not kernel pointers.
#pragma once
#include "rdrf_host.hpp"

struct BwdArgs;   // rdrf_bwd_dev.hpp
struct DynG;

// backward workspace (carve_bwd, rdrf_bwd.hip)
struct BwdWs {
  float* dfs;            // sorted scatter (dynamic field)
  float* dfa;            // sorted appearance scatter: [N*S] records of DFA_FLOATS (capacity; count <= N*S entries are used)
  unsigned *keys_in, *keys_out, *order;
  int* counts;
  void* sort_tmp;
  size_t sort_tmp_bytes;
  float* pk;
  float* gf;       // static field: d(density feature) per sample, [N][ceil(S/32)*32]
  float* grows1;
  float* grows3;
  float* dxw;
  float* dxn;
  float* dtout;
  float* gsig;     // flat-tile density phase (BwdArgs::gsig, ::dtp)
  float* dtp;
};
// the sorted scatter's buffers over ns samples: keys in / out and sorted positions of the 3 planes, counters, radix-sort scratch
static inline void carve_sorted_scatter(BwdWs& b, WsCarver& c, size_t ns) {
  b.keys_in = c.take<unsigned>(3 * ns);
  b.keys_out = c.take<unsigned>(3 * ns);
  b.order = c.take<unsigned>(3 * ns);
  b.counts = c.take<int>(64);
  b.sort_tmp_bytes = rdrf_sort_seg_temp_bytes(3, (unsigned)ns, 32);
  b.sort_tmp = c.take<char>(b.sort_tmp_bytes);
}

// ------------------------------------------------------------------------------------------------
// gradient scatter (rdrf_scatter.hip)
// ------------------------------------------------------------------------------------------------
struct ScatterArgs {
  RdrfVM vm[2], gvm[2];
  int nsets;
  const float* rows;   // d(feature) rows: tile t, row r at rows + (t*stride + row0[set] + r)*32
  int flat;            // ray-tile mode: the tiles are 32-sample tiles of the flat [N * S] array, not (ray, tile) pairs
  int stride, row0[2];
  const float* xw;     // [idx][3] normalised coordinates, or nullptr -> normalise xyz
  const float* xyz;
  Box box;
  const int* list;     // compacted mode: sample ids (+ device count); nullptr -> ray tiles
  const int* count;
  const uint8_t* valid;
  int N, S;
  float* dxw;          // [idx][3] coordinate gradients (nullable)
  int dxw_accumulate;
  float* g_xyz;        // static field: g_xyz += dw * inv (nullable)
  int lds_bytes;       // dynamic LDS for the line accumulators (0: lines go to global memory)
  int lds_f64;         // the accumulators are doubles (ds_add_f64: 11 x the update rate of ds_add_f32) / floats
  int bcast;           // 1: every component's gradient is row 0 of the tile (static density: the
                       //    feature is the plain sum of the 24 products)
};
enum ScatterKernel {   // the instantiations of k_scatter<C0Q, C1Q, NQ> in use
  SCATTER_4_1_3,       // static density
  SCATTER_4_1_9,       // dynamic density + blending
  SCATTER_12_3_9,      // static appearance
  SCATTER_12_3_27      // dynamic appearance
};
void fill_scatter_common(ScatterArgs& sa, const BwdArgs& a);
int launch_scatter(const char* name, ScatterKernel kern, ScatterArgs& sa, long ntiles, hipStream_t stream);
int scatter_mode(size_t ns, hipStream_t stream);   // 0 ray, 1 sorted
int scatter_dyn_app_sorted(const BwdArgs& a, const BwdWs& b, const RdrfDynamicParams* P, const RdrfDynamicParams* G,
                           hipStream_t stream);
int scatter_dyn_density_sorted(const BwdArgs& a, const BwdWs& b, const RdrfDynamicParams* P, const RdrfDynamicParams* G,
                               int set_mask, hipStream_t stream);
int sorted_key_bits(const int W[3], const int H[3]);   // bits of the cell part of a sort key: cells of (W + 3) x (H + 3) + the drop code
int scatter_mode_swap(int mode);                       // sets the process-wide scatter mode, returns the previous one (self-tests)
// What the launch policy decided for the most recent scatter (host stores only; rdrf_selftest_scatter_last reads it): one entry
// per kernel launch of the last launch_scatter / scatter_dyn_*_sorted call.
struct ScatterLaunch {
  int elem_bytes;    // LDS line accumulators: 8 doubles, 4 floats, 0 none (global atomics)
  int threads, workgroups;
  int tiled;         // sorted passes: 1 k_scatter_tiled taken, 0 refused by the policy (k_scatter_sorted ran), -2 windows switched
                     // off (_SORTED_PLAIN, deterministic build), -1 not tried (appearance); ray tiles: -1
  int tw, slice_steps;
};
struct ScatterRecord {
  int form;          // 0 ray tiles (launch_scatter), 1 sorted passes
  int split;         // ray tiles: one launch per factor set
  int n;
  ScatterLaunch l[4];
};
const ScatterRecord& scatter_last_record();   // of the calling host thread

// ------------------------------------------------------------------------------------------------
// generic dW kernel: dW[out][col(e)] += sum_tiles sum_samples dz[out][s] * in[e][s]
// (rdrf_dw.hip)
// ------------------------------------------------------------------------------------------------
struct DwJob {
  const float* A;   // dz rows: tile t, row r at A + (t*A_stride + A_row0 + r)*32
  int A_stride, A_row0, nbo, out_dim, out_row0;
  const float* B;   // input rows
  int B_stride;
  int nblk;         // number of 32-row input blocks
  int blk_row0[8], blk_seg[8], blk_e0[8];
  int in_dim, ld;
  float* dW;
  float* db;        // bias gradient (nullable), indexed like the out rows
  const int* count; // device sample count (compacted phases) or nullptr
  int ntiles;
};
#define RDRF_MAX_DW_JOBS 12
struct DwJobs {
  DwJob j[RDRF_MAX_DW_JOBS];
  int n;
};
void dw_add(DwJobs& D, const float* A, int A_stride, int A_row0, int nbo, int out_dim, int out_row0, const float* B,
            int B_stride, int in_dim, int ld, float* dW, float* db, const int* count, int ntiles);
void dw_blk(DwJobs& D, int row0, int seg, int e0);
int dw_launch(DwJobs& D, hipStream_t stream, const char* name);
// the launches dw_launch would make, written as ints (rdrf_selftest_dw_plan); host code only, no HIP call
int dw_describe_launches(const DwJobs& D, int* out, int cap);

// the job lists of the backward entry points, one builder per list (rdrf_bwd.hip); rdrf_selftest_dw (rdrf_selftest.hip) runs
// the same lists on caller-supplied rows.  cnt / ntiles: the device sample count of a compacted phase, or the host tile count.
void add_density_phase_dw(DwJobs& D, const float* grows1, const float* act1, const RdrfDynamicParams* G, int T1,
                          bool live_d = true, bool live_b = true, bool small_in_kernel = false, bool warp_in_kernel = false);
void add_static_app_dw(DwJobs& D, const float* grows3, const float* act3, const RdrfStaticParams* G, bool fea, const int* cnt,
                       int ntiles);
void add_dyn_app_dw(DwJobs& D, const float* grows3, const float* act3, const RdrfDynamicParams* G, const int* cnt, int ntiles);
void add_scene_flow_dw(DwJobs& D, const float* grows, const float* act, const RdrfDynamicParams* G, int T);
void add_feat_static_dw(DwJobs& D, const float* grows3, const float* act3, const RdrfStaticParams* G, int Np);
void add_feat_dyn_app_dw(DwJobs& D, const float* grows3, const float* act3, const RdrfDynamicParams* G, int Np);
// The warp MLP backward of the flat training path alone, on rows the caller supplies (rdrf_selftest_warp_bwd): the kernel(s)
// rdrf_dynamic_bwd launches under `dyn_warp_bwd`, followed on the two-kernel path by the k_dw3 products of layer3 / layer4.
// pk: PACK_AREA_FLOATS floats for the weight images; valid: N * S bytes of scratch.
int warp_bwd_on_rows(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, int N, int S, const float* act1, float* grows1,
                     float* dxw, float* dxn, const float* g_xyz_prime, const RdrfDynamicParams* G, float* g_xyz, float* dtout,
                     float* dtp, float* pk, uint8_t* valid, hipStream_t stream);

// The heads' backward of the density phase alone, on rows the caller supplies (rdrf_selftest_heads_bwd): k_dyn_density_bwd<0>
// as rdrf_dynamic_bwd launches it on the flat tiles of [N][S] (feat == 0: raw, valid, gsig, nullable g_blending and dfs; live_d:
// the density head gets a gradient) or as rdrf_dynamic_features_bwd does on the N = ceil(M / 32) pseudo rays of S = 32 points
// (feat == 1: nullable g_sigma / g_blending of the raw outputs).  The small layers' gradients are added into G (flat tiles only).
// pk: PACK_AREA_FLOATS floats for the weight images.  heads_bwd_units: the units the launch geometry (geo_for_units) is sized for.
long heads_bwd_units(int N, int S, int flat);
int heads_bwd_on_rows(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, int feat, int N, int S, int M, const float* act1,
                      const float* raw, const uint8_t* valid, const float* gsig, const float* g_sigma, const float* g_blending,
                      int live_d, float* grows1, float* dfs, const RdrfDynamicParams* G, float* pk, hipStream_t stream);
// k_time_branch_bwd with the entry points' geometry (32 rays per workgroup of 128 threads); dtp nullable; G: l1w, l1b, l2w, l2b
struct DynW;
int launch_time_branch_bwd(const float* ts, const DynW& w, int N, const float* dtout, const float* dtp, int S,
                           const RdrfDynamicParams* G, hipStream_t stream);

// The backward-data kernels of the appearance phase (k_dyn_app_bwd, k_static_app_bwd: rdrf_bwd.hip) with the entry points' geometry,
// geo_for_units of app_bwd_units: the tiles of [N][S] on the ray path, the N pseudo rays of feature mode.  APP_RECORDS (dynamic
// only): d(app features) go to a.dfa as sample-major records; head: RDRF_HEAD_* of the static field (feature mode runs the
// MLP_Fea instantiation for either).  The four backward entry points launch them; app_bwd_on_rows does on caller-supplied rows
// (rdrf_selftest_app_bwd): dynamic != 0: P is a RdrfDynamicParams, else a RdrfStaticParams with cfg->static_head; ray path: act3
// [tiles][K3_ROWS | S3_ROWS][32], list [N S] and the device count of the compacted samples, rays [N][6], nullable g_rgb [N S][3],
// dxn [N S][3] (dynamic), nullable g_rays [N][6] (static, added into); feature mode: N = ceil(M / 32), S = 32, g_feat [M][27].
// grows3 [tiles][K3G_ROWS][32]; pk: PACK_AREA_FLOATS floats for the weight image.
enum AppBwdForm { APP_ROWS, APP_RECORDS, APP_FEAT };
struct StaticW;
struct StaticG;
struct DynG;
long app_bwd_units(int N, int S, int feat);
int launch_dyn_app_bwd(const char* name, AppBwdForm form, const BwdArgs& a, const DynW& w, const DynG& gw, hipStream_t stream);
int launch_static_app_bwd(const char* name, int head, AppBwdForm form, const BwdArgs& a, const StaticW& w, const StaticG& gw,
                          hipStream_t stream);
int app_bwd_on_rows(const void* P, const RdrfFieldCfg* cfg, int dynamic, AppBwdForm form, int N, int S, int M, const float* act3,
                    const int* list, const int* count, const float* rays, const float* g_rgb, const float* g_feat, float* grows3,
                    float* dfa, float* dxn, float* g_rays, float* pk, hipStream_t stream);

// The ray scan backward alone on arrays the caller supplies (rdrf_selftest_ray_scan_bwd), launched as the entry points launch
// it: width 32 k_ray_scan_bwd (raw [N][S][2], out = gsig [N][S]), width 64 k_static_density_bwd (raw [N][S], out = gf rows
// [N][32 ceil(S / 32)]).  Cotangents and g_z / g_rays nullable.
int ray_scan_bwd_on_arrays(int width, const float* rays, const float* z, const uint8_t* valid, const float* raw, int N, int S,
                           int act, float density_shift, float distance_scale, int ray_type, const float* g_weight,
                           const float* g_sigma, const float* g_dists, float* out, float* g_z, float* g_rays, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// backward-data kernels with the weight gradients formed in the kernel (rdrf_bwd_fused.hip)
// ------------------------------------------------------------------------------------------------
void fused_dw_geometry(long tiles, int* grid, int* waves);   // for `tiles` 32-sample tiles: workgroups, waves per workgroup
// k_scene_flow_bwd_dw<g_pts != nullptr>: pkimg = the backward weight images, saved = the forward's activation rows, G: sfw / sfb
int launch_scene_flow_fused(int N, int S, const Box& box, const float* pkimg, const float* saved, const float* g_sf_f,
                            const float* g_sf_b, const RdrfDynamicParams* G, float* g_pts, long tiles, hipStream_t stream);
// k_dyn_warp_bwd_dw<a.g_xyz != nullptr>: G = where the gradients of layer3 / layer4 go (layer5: gw)
int launch_warp_fused(const BwdArgs& a, const DynG& gw, const RdrfDynamicParams* G, long tiles, hipStream_t stream);
