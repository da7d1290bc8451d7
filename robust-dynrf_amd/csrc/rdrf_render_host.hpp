// rdrf_render_host.hpp -- the workspace layout of the no-grad render (rdrf_render.hip), shared with the masked render
// (rdrf_render_masked.hip): both cut their buffers with one carve.  And the host helpers of the forward entry points
// (rdrf_fwd.hip) that the render units set their field launches up with.
#pragma once
#include "rdrf_host.hpp"

struct FieldArgs;   // rdrf_kernels.hpp
// the field-independent part of a forward launch's arguments (everything else zeroed)
void fill_common(FieldArgs& a, const RdrfFieldCfg* cfg, const float* rays, const float* ts, const float* xyz, const float* z,
                 const uint8_t* valid, int N, int S);
// pack area, counter, tout, xw and list out of a rdrf_forward_workspace_bytes(N, S) slice; with `saved`, the training buffers
int ws_carve_fwd(FieldArgs& a, void* ws, size_t ws_bytes, int N, int S, void* saved, size_t saved_bytes, int dynamic);
int fwd_dynq();   // FieldArgs::dynq of the forward launches

struct RenderBufs {
  float *xyz, *z, *rgb_s, *sigma_s, *weight_s, *dists_s, *rgb_d, *sigma_d, *weight_d, *dists_d, *blending, *xyz_prime;
  uint8_t* valid;
  float* out[13];
  void *fws_s, *fws_d;
  unsigned* barrier;
};
// RdrfRenderMaps -> the compositor's 13 output slots (NULL: not requested)
void maps_to_slots(float* out[13], const RdrfRenderMaps* m);
// want[13]: the caller's output buffers (NULL: the output goes to the workspace)
int carve_render(RenderBufs& b, void* ws, size_t ws_bytes, int N, int S, float* const want[13]);
// where a render with these `maps` left what the kernels that run after it read (rdrf_motion.hip, rdrf_track.hip): the
// carve of the render itself
int render_motion_views(const RdrfRenderMaps* maps, void* ws, size_t ws_bytes, int N, int S, const float** xyz,
                        const float** xyz_prime, const float** weights_s, const float** weights_d, const unsigned** barrier,
                        void** fws_d);
