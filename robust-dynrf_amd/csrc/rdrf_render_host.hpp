// rdrf_render_host.hpp -- the workspace layout of the no-grad render (rdrf_render.hip), shared with the masked render
// (rdrf_render_masked.hip): both cut their buffers with one carve.
#pragma once
#include "rdrf_host.hpp"

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
