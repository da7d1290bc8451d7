// rdrf_motion.hip -- motion maps of the no-grad evaluation render (the reference's renderer.py:319-657 `render`):
//   k_motion_maps   : the four induced optical-flow maps (dynamic forward / backward through the scene-flow MLP, :487-514;
//                     static forward / backward through camera motion alone, :516-537) and the warp-displacement map
//                     sum_s weights_d (xyz_prime - xyz) (:460, :610) from what the render left in its workspace
//   k_flow_to_image : flow_viz.flow_to_image (flow_viz.py:107-136, defaults) -- the Middlebury colour wheel
#include "rdrf_misc_dev.hpp"
#include "rdrf_render_host.hpp"

// ------------------------------------------------------------------------------------------------
// k_motion_maps: one wave per ray, 32-sample tiles (sample s of the tile in lanes s and s + 32: the layout of mfma_seg).
//
// Per sample the 36 -> 64 -> 64 -> 64 -> 6 scene-flow MLP is k_scene_flow's: fill_sf_x and sf_mlp (rdrf_fwd_dev.hpp) on the
// same packed image -- an MFMA column depends on its own sample only, so the per-sample values have k_scene_flow's
// bits -- and nothing per sample is written: lane s keeps the running sums of the samples s, s + 32,
// s + 64, ... of its ray, in that order; after the last tile the 32 lane sums are added by a fixed xor tree (16, 8, 4, 2,
// 1).  The order depends on S alone -- not on N, on where a chunk starts, on which maps are requested or on timing --
// and no atomic is involved: the maps are bit-identical run after run, chunked or not, in either library build.
// A tile whose 32 weights_d are all exactly 0 skips the MLP: 0 * (p + sf) = 0 * p for every finite sf.
// Then lanes 0..3 each run one per-ray tail (flow_ray_fwd, shared with k_induce_flow) and lane 4 writes delta_xyz.
// ------------------------------------------------------------------------------------------------
struct MotionArgs {
  const float *xyz, *xyz_prime, *w_s, *w_d;   // the render's workspace: [N][S][3], [N][S][3], [N][S], [N][S]
  const float *rays, *ts;
  const float *focal, *c2w_f, *c2w_b;
  const unsigned* barrier;                    // fused render: barrier[1] != 0 after a time-out (NaN maps); else nullptr
  float *flow_f, *flow_b, *flow_s_f, *flow_s_b, *delta;
  long long first_pixel;
  int N, S, H, W, ray_type;
  Box box;
};

RDRF_D float half_sum32(float v) {   // over the 32 lanes of a half wave, fixed pairing
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <bool MLP>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_motion_maps(MotionArgs a, const float* __restrict__ pkg,
                                                                  const float* __restrict__ sfb6) {
  __shared__ __attribute__((aligned(16))) float lds[MLP ? pk::SF_SIZE : 4];
  if constexpr (MLP) lds_fill(lds, pkg + pk::REG_SF, pk::SF_SIZE);
  const float* pkw = lds;
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int S = a.S;
  const bool failed = a.barrier != nullptr && a.barrier[1] != 0u;
  for (int n = blockIdx.x * nwaves + wave; n < a.N; n += gridDim.x * nwaves) {
    const float t = a.ts[n];
    float Af[3] = {0.f, 0.f, 0.f}, Ab[3] = {0.f, 0.f, 0.f}, As[3] = {0.f, 0.f, 0.f}, D[3] = {0.f, 0.f, 0.f};
    float sum_d = 0.f, sum_s = 0.f;
    for (int j0 = 0; j0 < S; j0 += 32) {
      const int j = j0 + s;
      const bool act = j < S;
      const size_t idx = (size_t)n * S + (act ? j : 0);   // 64-bit: idx * 3 is formed below
      const float wd = act ? a.w_d[idx] : 0.f, ws = act ? a.w_s[idx] : 0.f;
      float p[3], q[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[c] = a.xyz[idx * 3 + c];
        q[c] = act ? a.xyz_prime[idx * 3 + c] : p[c];
      }
      float sf[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if constexpr (MLP) {
        if (__any(wd != 0.f)) {   // (wave-uniform)
          float X[20];
          fill_sf_x(X, norm_c(p[0], a.box.lo[0], a.box.inv[0]), norm_c(p[1], a.box.lo[1], a.box.inv[1]),
                    norm_c(p[2], a.box.lo[2], a.box.inv[2]), t, h);
          sf_mlp(sf, X, pkw, sfb6, nullptr, s, h, lane);
        }
      }
      if (!act) { p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; q[0] = 0.f; q[1] = 0.f; q[2] = 0.f; }
      sum_d += wd;
      sum_s += ws;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if constexpr (MLP) {
          Af[c] += wd * (p[c] + sf[c]);
          Ab[c] += wd * (p[c] + sf[3 + c]);
        }
        As[c] += ws * p[c];
        D[c] += wd * (q[c] - p[c]);
      }
    }
    sum_d = half_sum32(sum_d);
    sum_s = half_sum32(sum_s);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (MLP) { Af[c] = half_sum32(Af[c]); Ab[c] = half_sum32(Ab[c]); }
      As[c] = half_sum32(As[c]);
      D[c] = half_sum32(D[c]);
    }
    const float nan = __int_as_float(0x7fc00000);
    if (lane < 4) {   // 0: flow_f, 1: flow_b, 2: flow_s_f, 3: flow_s_b
      float* out = lane == 0 ? a.flow_f : (lane == 1 ? a.flow_b : (lane == 2 ? a.flow_s_f : a.flow_s_b));
      if (out != nullptr) {
        const bool dyn = lane < 2;
        float ps[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) ps[c] = dyn ? (lane == 0 ? Af[c] : Ab[c]) : As[c];
        const float* c2w = (lane & 1) ? a.c2w_b : a.c2w_f;
        FlowRay r;
        float u, v, disp;
        flow_ray_fwd(r, a.rays + (size_t)n * 6, c2w, dyn ? sum_d : sum_s, ps, a.H, a.W, a.focal[0], a.ray_type, u, v, disp);
        // pts_2d of the reference's integer meshgrid (renderer.py:372-375)
        const long long pix = a.first_pixel + n;
        const float px = (float)(pix % a.W), py = (float)((pix / a.W) % a.H);
        out[(size_t)n * 2 + 0] = failed ? nan : u - px;
        out[(size_t)n * 2 + 1] = failed ? nan : v - py;
      }
    } else if (lane == 4 && a.delta != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.delta[(size_t)n * 3 + c] = failed ? nan : D[c];
    }
  }
}

extern "C" size_t rdrf_render_motion_workspace_bytes(int N, int S) { return rdrf_render_workspace_bytes(N, S); }

extern "C" int rdrf_render_motion_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                      const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near,
                                      float far, int mode, const RdrfRenderMaps* maps, const RdrfMotionCams* cams,
                                      const RdrfMotionMaps* motion, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;
  RDRF_CHECK(cams && motion, -1, "render_motion: cameras and motion maps are required");
  RDRF_CHECK(cams->H > 0 && cams->W > 0 && cams->focal && cams->c2w_f && cams->c2w_b && cams->first_pixel >= 0, -1,
             "render_motion: bad cameras (H, W > 0; focal, c2w_f, c2w_b device pointers; first_pixel >= 0)");
  RDRF_CHECK(cfg_d && (cfg_d->ray_type == RDRF_RAY_NDC || cfg_d->ray_type == RDRF_RAY_CONTRACT), -1,
             "render_motion: ray_type must be ndc or contract (renderer.py:1335-1351)");
  // the render itself: same launches, same bits (the workspace carve does not depend on the motion request)
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, 0.f, {}, ws, ws_bytes};
  maps_to_slots(c.want, maps);
  RenderBufs b;
  RDRF_TRY(render_run(c, mode, "render_maps", b, stream_));
  if (!motion->flow_f && !motion->flow_b && !motion->flow_s_f && !motion->flow_s_b && !motion->delta_xyz) return 0;
  MotionArgs a;
  memset(&a, 0, sizeof(a));
  a.xyz = b.xyz; a.xyz_prime = b.xyz_prime; a.w_s = b.out[7]; a.w_d = b.out[11];
  a.barrier = mode == RDRF_RENDER_FUSED ? b.barrier : nullptr;   // only the cooperative launch has a barrier (and clears it)
  a.rays = rays; a.ts = ts;
  a.focal = cams->focal; a.c2w_f = cams->c2w_f; a.c2w_b = cams->c2w_b;
  a.flow_f = motion->flow_f; a.flow_b = motion->flow_b; a.flow_s_f = motion->flow_s_f; a.flow_s_b = motion->flow_s_b;
  a.delta = motion->delta_xyz;
  a.first_pixel = cams->first_pixel;
  a.N = N; a.S = S; a.H = cams->H; a.W = cams->W; a.ray_type = cfg_d->ray_type;
  a.box = make_box(cfg_d);
  const bool mlp = motion->flow_f != nullptr || motion->flow_b != nullptr;
  const float* pkg = PD->packed_fwd;
  if (pkg == nullptr) {   // the image the dynamic field's forward packed into its workspace on this stream
    FieldArgs fa;
    memset(&fa, 0, sizeof(fa));
    RDRF_TRY(ws_carve_fwd(fa, b.fws_d, rdrf_forward_workspace_bytes(N, S), N, S, nullptr, 0, 1));
    pkg = fa.pk;
  }
  int ncu = 0;
  RDRF_TRY(current_cu_count(&ncu));
  // persistent workgroups (the MLP form fills 45 KB of LDS once per workgroup): two per CU, or fewer for few rays
  long g = ((long)N + RDRF_MAXW - 1) / RDRF_MAXW;
  const long cap = (long)ncu * (mlp ? 2 : 8);
  g = g < 1 ? 1 : (g > cap ? cap : g);
  if (mlp) RDRF_LAUNCH("motion_maps", k_motion_maps<true>, dim3((unsigned)g), dim3(64 * RDRF_MAXW), stream, a, pkg,
                      (const float*)PD->sfb[3]);
  else RDRF_LAUNCH("motion_maps", k_motion_maps<false>, dim3((unsigned)g), dim3(64 * RDRF_MAXW), stream, a, pkg,
                      (const float*)PD->sfb[3]);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// flow_to_image (flow_viz.py:107-136 with its defaults: no clip, RGB) in numpy's precision sequence: fp32 up to fk
// (radius, division by rad_max + 1e-5, arctan2 / pi, (a + 1) / 2 * 54), fp64 from f = fk - k0 on (numpy promotes
// float32 - int32 to float64; the colour wheel is a float64 array).  arctan2 is evaluated in fp64 and rounded to fp32:
// the correctly rounded fp32 value.
//   stage 1  k_flow_radmax : per workgroup max of the radius over its pixels (+-inf entries -> 0 first; a NaN radius
//                            makes the max NaN, as np.max does)
//   stage 2  k_flow_colors : every workgroup folds the partial maxima (a max is the same in any order; NaN is sticky),
//                            then colours its pixels
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int kFlowThreads = 256, kFlowMaxBlocks = 1024;
__constant__ int kWheelLen[6] = {15, 6, 4, 11, 13, 6};   // RY, YG, GC, CB, BM, MR
}

RDRF_D float nanmax(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : fmaxf(a, b); }
RDRF_D float block_nanmax(float v, float* red) {
  for (int off = 32; off >= 1; off >>= 1) v = nanmax(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = red[0];
  for (int i = 1; i < kFlowThreads / 64; ++i) m = nanmax(m, red[i]);
  __syncthreads();
  return m;
}
RDRF_D float deinf(float x) { return (x == INFINITY || x == -INFINITY) ? 0.f : x; }

__global__ __launch_bounds__(kFlowThreads) void k_flow_radmax(const float* __restrict__ flow, long long npix,
                                                              float* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ float red[kFlowThreads / 64];
  float m = 0.f;   // rad >= 0
  for (long long i = (long long)blockIdx.x * kFlowThreads + threadIdx.x; i < npix; i += (long long)gridDim.x * kFlowThreads) {
    const float u = deinf(flow[i * 2 + 0]), v = deinf(flow[i * 2 + 1]);
    m = nanmax(m, sqrtf(u * u + v * v));
  }
  m = block_nanmax(m, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// colour-wheel entry k (0..54), channel c, as make_colorwheel builds it (flow_viz.py:23-68): six segments of lengths
// 15, 6, 4, 11, 13, 6, each a ramp floor(255 i / len) up or down on one channel
RDRF_D double wheel(int k, int c) {
  int seg = 0, i = k;
  while (seg < 5 && i >= kWheelLen[seg]) { i -= kWheelLen[seg]; ++seg; }
  const double ramp = floor(255.0 * (double)i / (double)kWheelLen[seg]);
  // segment: RY (R 255, G up), YG (R down, G 255), GC (G 255, B up), CB (G down, B 255), BM (B 255, R up), MR (B down, R 255)
  const int full = seg == 0 ? 0 : (seg == 1 || seg == 2 ? 1 : (seg == 3 || seg == 4 ? 2 : 0));
  const int var = seg == 0 ? 1 : (seg == 1 ? 0 : (seg == 2 ? 2 : (seg == 3 ? 1 : (seg == 4 ? 0 : 2))));
  const bool down = (seg & 1) != 0;
  if (c == full) return 255.0;
  if (c == var) return down ? 255.0 - ramp : ramp;
  return 0.0;
}

__global__ __launch_bounds__(kFlowThreads) void k_flow_colors(const float* __restrict__ flow, long long npix,
                                                              const float* __restrict__ partial, int npartial,
                                                              uint8_t* __restrict__ rgb) {
#pragma clang fp contract(off)
  __shared__ float red[kFlowThreads / 64];
  __shared__ double s_wheel[55 * 3];
  for (int e = threadIdx.x; e < 55 * 3; e += kFlowThreads) s_wheel[e] = wheel(e / 3, e % 3);
  float m = 0.f;
  for (int i = threadIdx.x; i < npartial; i += kFlowThreads) m = nanmax(m, partial[i]);
  const float rad_max = block_nanmax(m, red);   // (its barriers also publish s_wheel)
  const float denom = rad_max + 1e-5f;
  const float pi32 = 3.14159265358979323846f;
  for (long long i = (long long)blockIdx.x * kFlowThreads + threadIdx.x; i < npix; i += (long long)gridDim.x * kFlowThreads) {
    float u = deinf(flow[i * 2 + 0]) / denom, v = deinf(flow[i * 2 + 1]) / denom;
    u = deinf(u); v = deinf(v);
    if (u != u) u = 0.f;
    if (v != v) v = 0.f;
    const float rad = sqrtf(u * u + v * v);
    const float ang = (float)atan2((double)(-v), (double)(-u)) / pi32;
    const float fk = (ang + 1.0f) / 2.0f * 54.0f;
    const int k0 = (int)floorf(fk);
    int k1 = k0 + 1;
    if (k1 == 55) k1 = 0;
    const double f = (double)fk - (double)k0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double col0 = s_wheel[k0 * 3 + c] / 255.0, col1 = s_wheel[k1 * 3 + c] / 255.0;
      double col = (1.0 - f) * col0 + f * col1;
      if (rad <= 1.0f) col = 1.0 - (double)rad * (1.0 - col);
      else col = col * 0.75;   // out of range
      rgb[i * 3 + c] = (uint8_t)(int)floor(255.0 * col);
    }
  }
}

static int flow_blocks(long long npix) {
  const long long b = (npix + kFlowThreads - 1) / kFlowThreads;
  return (int)(b < 1 ? 1 : (b > kFlowMaxBlocks ? kFlowMaxBlocks : b));
}

extern "C" size_t rdrf_flow_to_image_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 256;
  return (size_t)flow_blocks((long long)H * W) * sizeof(float) + 256;
}

extern "C" int rdrf_flow_to_image(const float* flow, int H, int W, uint8_t* rgb, void* ws, size_t ws_bytes,
                                  rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(flow && rgb && ws && H > 0 && W > 0, -1, "flow_to_image: bad arguments");
  RDRF_CHECK(ws_bytes >= rdrf_flow_to_image_workspace_bytes(H, W), -3, "flow_to_image: workspace too small");
  const long long npix = (long long)H * W;
  const int nb = flow_blocks(npix);
  RDRF_LAUNCH("flow_radmax", k_flow_radmax, dim3(nb), dim3(kFlowThreads), stream, flow, npix, (float*)ws);
  RDRF_LAUNCH("flow_colors", k_flow_colors, dim3(nb), dim3(kFlowThreads), stream, flow, npix, (const float*)ws, nb, rgb);
  return 0;
}
