// rdrf_track.hip -- point tracks: a surface point followed through the video by chaining the scene-flow MLP
// (models/tensoRF.py:506-519 get_forward_backward_scene_flow_point_single, applied frame after frame).
//   k_track_points : M seed points x (n_bwd + 1 + n_fwd) frames.  p_{k+1} = p_k + sf_f(p_k, t_k), t_{k+1} = t_k + dt forward,
//                    p_{k-1} = p_k + sf_b(p_k, t_k), t_{k-1} = t_k - dt backward; contract scenes clamp the sum to
//                    [-2 + 1e-6, 2 - 1e-6] (train.py:1377-1378).  Each p_k is optionally projected into camera k with
//                    render_single_3d_point's arithmetic (renderer.py:1299-1325; contract: render_3d_point's contract2world leg).
//   k_track_seeds  : the first half of render_3d_point (renderer.py:1333-1345) on what a render left in its workspace:
//                    sum_s weights_d xyz + (1 - acc_d) far, the point a track of a pixel starts from.
#include "rdrf_misc_dev.hpp"
#include "rdrf_render_host.hpp"

// ------------------------------------------------------------------------------------------------
// k_track_points: persistent workgroups with the scene-flow image (pk::REG_SF, 45 KB) in LDS; a wave owns a 32-point tile
// (point s of the tile in lanes s and s + 32: the layout of mfma_seg) and runs the whole chain of its tile with the points
// in registers -- the forward steps, then, from the reloaded seed, the backward steps.  Per step the 36 -> 64 -> 64 -> 64 -> 6
// MLP is k_scene_flow's: fill_sf_x and sf_mlp (rdrf_fwd_dev.hpp) on the same image; an MFMA column depends on its own
// point only, so a point gets k_scene_flow's bits whatever shares its tile.  sf_mlp leaves the six outputs in both
// half-waves, both add them to their copy of the point, and the lower half writes the slot.  Nothing in the step loop
// writes LDS.  A lane past M holds the point 0 at time 0 (finite MFMA operands) and writes nothing.
// ------------------------------------------------------------------------------------------------
struct TrackArgs {
  const float *p0, *t0;       // [M][3], [M]
  const float *c2w, *focal;   // [K][3][4], one float; nullptr: no projection
  float *pts, *pix, *disp;    // [M][K][3], [M][K][2], [M][K]; each nullable
  int M, K, n_fwd, n_bwd, H, W, ray_type;
  float dt;
  Box box;
};

RDRF_D void track_step(float (&p)[3], float& t, const float (&sf)[6], int dir, float dt, int ray_type) {
#pragma clang fp contract(off)
  const float lo = (float)(-2.0 + 1e-6), hi = (float)(2.0 - 1e-6);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float q = p[c] + (dir == 0 ? sf[c] : sf[3 + c]);
    if (ray_type == RDRF_RAY_CONTRACT) q = fminf(fmaxf(q, lo), hi);
    p[c] = q;
  }
  t = dir == 0 ? t + dt : t - dt;
}

// slot k of point i: the point itself and its projection into camera k (a weight-1, one-sample "ray" through flow_ray_fwd:
// acc = 1 and a zero ray, which is how render_single_3d_point runs on the induce-flow kernel)
RDRF_D void track_emit(const TrackArgs& a, size_t i, int k, const float (&p)[3]) {
#pragma clang fp contract(off)
  const size_t o = i * (size_t)a.K + (size_t)k;
  if (a.pts != nullptr) {
    a.pts[o * 3 + 0] = p[0]; a.pts[o * 3 + 1] = p[1]; a.pts[o * 3 + 2] = p[2];
  }
  if (a.pix != nullptr || a.disp != nullptr) {
    const float zero_ray[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    FlowRay r;
    float u, v, d;
    flow_ray_fwd(r, zero_ray, a.c2w + (size_t)k * 12, 1.0f, p, a.H, a.W, a.focal[0], a.ray_type, u, v, d);
    if (a.pix != nullptr) { a.pix[o * 2 + 0] = u; a.pix[o * 2 + 1] = v; }
    // ndc: render_single_3d_point's (z_ndc + 1) / 2; contract: render_3d_point's z_ndc
    if (a.disp != nullptr) a.disp[o] = a.ray_type == RDRF_RAY_NDC ? (d + 1.0f) / 2.0f : d;
  }
}

__global__ __launch_bounds__(64 * RDRF_MAXW) void k_track_points(TrackArgs a, const float* __restrict__ pkg,
                                                                   const float* __restrict__ sfb6) {
  __shared__ __attribute__((aligned(16))) float lds[pk::SF_SIZE];
  lds_fill(lds, pkg + pk::REG_SF, pk::SF_SIZE);
  const float* pkw = lds;
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int ntiles = (a.M + 31) >> 5;
  for (int q = wave, tile; (tile = blockIdx.x + q * gridDim.x) < ntiles; q += nwaves) {
    const int li = tile * 32 + s;
    const bool act = li < a.M;
    const size_t i = act ? (size_t)li : 0;
    for (int dir = 0; dir < 2; ++dir) {   // 0: forward chain, 1: backward chain, each from the seed
      const int nstep = dir == 0 ? a.n_fwd : a.n_bwd;
      float p[3] = {0.f, 0.f, 0.f}, t = 0.f;
      if (act) {
        p[0] = a.p0[i * 3 + 0]; p[1] = a.p0[i * 3 + 1]; p[2] = a.p0[i * 3 + 2];
        t = a.t0[i];
      }
      if (dir == 0 && act && h == 0) track_emit(a, i, a.n_bwd, p);
      for (int k = 1; k <= nstep; ++k) {
        // compiler barrier (as k_alpha_dyn): nothing below writes LDS, so without it the weight reads of every layer are
        // invariant in k and get hoisted out of the loop into registers the kernel does not have
        asm volatile("" ::: "memory");
        float sf[6];
        {
          float X[20];
          fill_sf_x(X, norm_c(p[0], a.box.lo[0], a.box.inv[0]), norm_c(p[1], a.box.lo[1], a.box.inv[1]),
                    norm_c(p[2], a.box.lo[2], a.box.inv[2]), t, h);
          sf_mlp(sf, X, pkw, sfb6, nullptr, s, h, lane);
        }
        track_step(p, t, sf, dir, a.dt, a.ray_type);
        if (!act) { p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; t = 0.f; }
        if (act && h == 0) track_emit(a, i, dir == 0 ? a.n_bwd + k : a.n_bwd - k, p);
      }
    }
  }
}

// workspace: the pack area, read only when the caller supplies no packed image (nothing is kept per point or step)
static void carve_track(float*& pk, WsCarver& c) { pk = c.take<float>(PACK_AREA_FLOATS); }

extern "C" size_t rdrf_track_ws_bytes(int M, int K) {
  (void)M; (void)K;
  float* pk;
  WsCarver c;
  carve_track(pk, c);
  return c.off;
}

extern "C" int rdrf_track_points_fwd(const RdrfDynamicParams* PD, const RdrfFieldCfg* cfg_d, const float* p0, const float* t0,
                                     int M, int n_fwd, int n_bwd, float dt, const RdrfTrackCams* cams, const RdrfTracks* out,
                                     void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(PD && cfg_d && out && M >= 0, -1, "track_points: bad arguments");
  RDRF_CHECK(n_fwd >= 0 && n_bwd >= 0, -1, "track_points: n_fwd and n_bwd are step counts >= 0 (got %d, %d)", n_fwd, n_bwd);
  RDRF_CHECK(cfg_d->ray_type == RDRF_RAY_NDC || cfg_d->ray_type == RDRF_RAY_CONTRACT, -1,
             "track_points: ray_type must be ndc or contract (renderer.py:1335-1351)");
  const long long K = (long long)n_bwd + 1 + n_fwd;
  RDRF_CHECK(K * 3 < (long long)INT32_MAX, -1, "track_points: too many steps");
  if (cams != nullptr) {
    RDRF_CHECK(cams->K == (int)K, -1, "track_points: %d cameras for n_bwd + 1 + n_fwd = %lld slots", cams->K, K);
    RDRF_CHECK(cams->H > 0 && cams->W > 0 && cams->focal && cams->c2w, -1,
               "track_points: bad cameras (H, W > 0; focal, c2w device pointers)");
  }
  RDRF_CHECK(cams != nullptr || (out->pix == nullptr && out->disp == nullptr), -1,
             "track_points: pix / disp need the cameras");
  if (M == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(p0 && t0, -1, "track_points: no seed points / times");
  if (!out->pts && !out->pix && !out->disp) return 0;
  TrackArgs a;
  memset(&a, 0, sizeof(a));
  a.p0 = p0; a.t0 = t0;
  a.pts = out->pts; a.pix = out->pix; a.disp = out->disp;
  if (cams != nullptr && (out->pix || out->disp)) { a.c2w = cams->c2w; a.focal = cams->focal; a.H = cams->H; a.W = cams->W; }
  a.M = M; a.K = (int)K; a.n_fwd = n_fwd; a.n_bwd = n_bwd; a.ray_type = cfg_d->ray_type;
  a.dt = dt;
  a.box = make_box(cfg_d);
  const float* pkg = nullptr;
  if (PD->packed_fwd == nullptr) {
    RDRF_CHECK(ws != nullptr, -3, "track_points: no workspace");
    WsCarver c(ws, ws_bytes);
    float* pkbuf;
    carve_track(pkbuf, c);
    RDRF_CHECK(c.ok(), -3, "track_points: workspace too small: need %zu have %zu", c.off, ws_bytes);
    RDRF_TRY(pack_image(pkg, PD->packed_fwd, pkbuf, stream, dyn_pack_jobs_fwd, PD));
  } else {
    pkg = PD->packed_fwd;
  }
  const Geo g = geo_for_units(((long)M + 31) / 32);   // the persistent geometry of the field kernels
  RDRF_LAUNCH("track_points", k_track_points, dim3(g.grid), dim3(g.block), stream, a, pkg, (const float*)PD->sfb[3]);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// k_track_seeds: a wave per ray; the sums in k_induce_flow's order (lane-strided, then the xor tree of wave_sum), the far
// point by flow_ray_seed -- so the seed is the very P that render_3d_point projects for these weights and points.
// ------------------------------------------------------------------------------------------------
constexpr int kSeedWaves = 4;
__global__ __launch_bounds__(64 * kSeedWaves) void k_track_seeds(const float* __restrict__ weights, const float* __restrict__ pts,
                                                                  const float* __restrict__ rays, int N, int S, int ray_type,
                                                                  float* __restrict__ seeds) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * kSeedWaves + (threadIdx.x >> 6);
  if (n >= N) return;   // (wave-uniform)
  float acc = 0.f, ps[3] = {0.f, 0.f, 0.f};
  for (int s = lane; s < S; s += 64) {
    const float w = weights[(size_t)n * S + s];
    const float* p = pts + ((size_t)n * S + s) * 3;
    acc += w; ps[0] += w * p[0]; ps[1] += w * p[1]; ps[2] += w * p[2];
  }
  acc = wave_sum(acc); ps[0] = wave_sum(ps[0]); ps[1] = wave_sum(ps[1]); ps[2] = wave_sum(ps[2]);
  if (lane == 0) {
    FlowRay r;
    flow_ray_seed(r, rays + (size_t)n * 6, acc, ps, ray_type);
    seeds[(size_t)n * 3 + 0] = r.P[0]; seeds[(size_t)n * 3 + 1] = r.P[1]; seeds[(size_t)n * 3 + 2] = r.P[2];
  }
}

extern "C" int rdrf_render_track_seeds_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                           const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S,
                                           float near, float far, const RdrfRenderMaps* maps, float* seeds, void* ws,
                                           size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;
  RDRF_CHECK(seeds != nullptr, -1, "render_track_seeds: no seed buffer");
  RDRF_CHECK(cfg_d && (cfg_d->ray_type == RDRF_RAY_NDC || cfg_d->ray_type == RDRF_RAY_CONTRACT), -1,
             "render_track_seeds: ray_type must be ndc or contract (renderer.py:1335-1351)");
  // the render itself: the launch sequence, same bits in every requested map (the workspace carve does not depend on `seeds`)
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, 0.f, {}, ws, ws_bytes};
  maps_to_slots(c.want, maps);
  RenderBufs b;
  RDRF_TRY(render_run(c, RDRF_RENDER_AUTO, "render_maps", b, stream_));
  RDRF_LAUNCH("track_seeds", k_track_seeds, dim3((N + kSeedWaves - 1) / kSeedWaves), dim3(64 * kSeedWaves), stream,
              (const float*)b.out[11], (const float*)b.xyz, rays, N, S, cfg_d->ray_type, seeds);
  return 0;
}
