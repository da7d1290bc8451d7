// rdrf_render_host.hpp -- the host side of the no-grad render, one copy of each step for the four units that run it
// (rdrf_render.hip, rdrf_render_masked.hip, rdrf_motion.hip, rdrf_track.hip) and the per-slot visibility (rdrf_track_vis.hip):
//   RenderCall     what every entry point of the family is called with; each builds it once
//   RenderBufs     the workspace carve of a render; the runner hands it back, and the kernels that run after a render
//                  (motion maps, track seeds) read it
//   render_check_* the argument checks; render_sample, render_fields: the sampler dispatch and the fields' launch set-up
//   render_run     the render itself, as a launch sequence or as the one cooperative launch
// (all defined in rdrf_render.hip).  And the host helpers of the forward entry points (rdrf_fwd.hip) that the field set-up uses.
#pragma once
#include "rdrf_host.hpp"

struct FieldArgs;   // rdrf_kernels.hpp
// the field-independent part of a forward launch's arguments (everything else zeroed)
void fill_common(FieldArgs& a, const RdrfFieldCfg* cfg, const float* rays, const float* ts, const float* xyz, const float* z,
                 const uint8_t* valid, int N, int S);
// pack area, counter, tout, xw and list out of a rdrf_forward_workspace_bytes(N, S) slice; with `saved`, the training buffers
int ws_carve_fwd(FieldArgs& a, void* ws, size_t ws_bytes, int N, int S, void* saved, size_t saved_bytes, int dynamic);
int fwd_dynq();   // FieldArgs::dynq of the forward launches
// The per-ray scans over stored sigmas with their production launch geometry, each in the unit that defines its kernel:
// k_ray_scan (rdrf_fwd.hip; 32 wide, 16 rays per workgroup) and k_static_scan (rdrf_render_masked.hip; 64 wide, 4 rays per
// workgroup).  They read a.rays, z, sigma, N, S, ray_type, distance_scale, weight_thres and write a.weight, dists, list, counter
// (added to) and rgb (zero fill; nullable).  The entry points launch them; rdrf_selftest_ray_scan does on caller-owned arrays.
int launch_ray_scan(const FieldArgs& a, hipStream_t stream);
int launch_static_scan(const FieldArgs& a, hipStream_t stream);
// k_time_branch (rdrf_fwd.hip) over N rays or points, 8 per workgroup of 256 threads: ts [N] -> tout [N][32]; zero64: the counter
// block of the density phase that follows, cleared on the way (nullable).  The training and feature-mode forward launch it;
// rdrf_selftest_time_branch does on caller-owned arrays.
struct DynW;
int launch_time_branch(const float* ts, const DynW& w, int N, float* tout, int* zero64, hipStream_t stream);

struct RenderCall {
  const RdrfStaticParams* PS;
  const RdrfFieldCfg* cfg_s;
  const RdrfDynamicParams* PD;
  const RdrfFieldCfg* cfg_d;
  const float *rays, *ts;
  int N, S;
  float near, far;
  float step;        // > 0: the world-space march (RDRF_RAY_OTHER); 0 for ndc / contract
  float* want[13];   // the caller's output buffers in the compositor's slot order (NULL: the output goes to the workspace)
  void* ws;          // the caller's scratch
  size_t ws_bytes;
};
// RdrfRenderMaps -> the compositor's 13 output slots (NULL: not requested)
void maps_to_slots(float* out[13], const RdrfRenderMaps* m);
// the legacy entry points: rgb and depth only, which carves the workspace exactly as before the maps existed
int want_rgb_depth(float* want[13], float* rgb_map, float* depth_map, const char* who);

struct RenderBufs {
  float *xyz, *z, *rgb_s, *sigma_s, *weight_s, *dists_s, *rgb_d, *sigma_d, *weight_d, *dists_d, *blending, *xyz_prime;
  uint8_t* valid;
  float* out[13];
  void *fws_s, *fws_d;
  unsigned* barrier;
};
int carve_render(RenderBufs& b, void* ws, size_t ws_bytes, int N, int S, float* const want[13]);

// The checks of the shared prefix in two halves, `who` the message prefix ("render", "render_masked").  A unit puts its own
// checks between them, where a caller has always met them: the render its workspace size, the masked render its masks.
//   render_check_args  : no null pointer, N, S > 0; `step` > 0 exactly for the world-space march (`step_rule`: the unit's
//                        wording of that rule); N * S * 3 < 2^31
//   render_check_fields: the component counts and the one grid the kernels are built for
int render_check_args(const RenderCall& c, const char* who, const char* step_rule);
int render_check_fields(const RenderCall& c, const char* who);

// xyz, z, valid of every sample by the sampler of cfg_d->ray_type
int render_sample(const RenderCall& c, const RenderBufs& b, rdrf_stream_t stream);
// Both fields' launch arguments over the carve (`valid_s`, `valid_d`: the plane each field reads), their forward workspaces,
// weight pointers and packed images (packed on `stream` where the caller brought none)
struct StaticW;
struct DynW;
int render_fields(const RenderCall& c, const RenderBufs& b, const uint8_t* valid_s, const uint8_t* valid_d, FieldArgs& as,
                  FieldArgs& ad, StaticW& wst, DynW& wdy, hipStream_t stream);

// The render: checks, carve (handed back in `b`), launches.  mode: RDRF_RENDER_FUSED is the cooperative launch, the two
// others the launch sequence; an unknown one is refused under the prefix `who`.
int render_run(const RenderCall& c, int mode, const char* who, RenderBufs& b, rdrf_stream_t stream);

// The list-driven density phase (kernels and launchers: rdrf_render_masked.hip): a field's density kernel runs on the listed
// samples [N * S flat indices] and on no other.  The device counters of a call are one block of 64 ints, a counter per
// 64-byte line: the two list lengths and the two appearance-list lengths.
//   launch_list_time_branch    : the dynamic field's time branch of every ray; clears the counter block on its way
//   launch_static_density_list : sigma of the listed samples (as.xyz, as.sigma; length ctr[CTR_KEPT_S]); `kept` (nullable)
//                                receives both list lengths
//   launch_dyn_density_list    : sigma, blending, xyz_prime, xw of the listed samples (ad.ts, ad.tout, ad.pk; length *count);
//                                the grid is sized for ad.N * ad.S entries
constexpr int CTR_KEPT_S = 0, CTR_KEPT_D = 16, CTR_APP_S = 32, CTR_APP_D = 48;
int launch_list_time_branch(const float* ts, const DynW& wdy, int N, float* tout, int* ctr, hipStream_t stream);
int launch_static_density_list(const FieldArgs& as, const StaticW& wst, const int* list_s, const int* ctr, long long* kept,
                               hipStream_t stream);
int launch_dyn_density_list(const FieldArgs& ad, const DynW& wdy, const int* list_d, const int* count, hipStream_t stream);

// The density-only run (defined in rdrf_track_vis.hip; also the maps == NULL path of rdrf_render_hits_fwd, rdrf_hits.hip):
// sampler of c.rays, time branch, ONE list of the samples with valid (and, with `zq` [N], z < zq of their ray), both
// list-driven density kernels.  Afterwards sigma_s, sigma_d and blending of a listed sample have forward()'s bits and those
// of every other sample are zero.  No appearance phase.
struct DensityBufs {
  float *xyz, *z;
  uint8_t* valid;
  float *sigma_s, *sigma_d, *blending, *xyz_prime, *xw, *tout;
  int *list, *ctr;
  float* pk;   // the dynamic field's weight image, packed here when the caller brings none
};
void carve_density_only(DensityBufs& b, WsCarver& c, size_t N, size_t S);
int density_only_run(const RenderCall& c, const DensityBufs& b, const float* zq, rdrf_stream_t stream);
