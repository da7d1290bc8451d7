// rdrf_point.hip -- per-point queries of a field: what TensorBase.forward (models/tensorBase.py:704-850) gives a sample at
// a position, a time and a view direction, without a ray around it.  valid = 1, no alpha-mask lookup, no aabb test, no weight
// threshold: every point gets its sigma (after density_act), its colour and, for the dynamic field, blending and xyz_prime.
//
//   k_point_time_branch : time_branch_body over 1 row (one time for all points) or M rows (a time per point)
//   k_point_dyn         : the density phase of the dynamic field, modelled on k_alpha_dyn -- 32-point tiles from the
//                         workgroup's queue, per point fill_x0 / fill_x1, load_tout, warp_mlp, warp_point, head_raw<false>
//                         and head_raw<true> (rdrf_fwd_dev.hpp) -- with a time per point instead of a T-loop and both heads.
//                         Writes sigma, blending, xyz_prime and the warped normalised point xw for the appearance kernel
//   k_point_static      : a lane per point, static_density_feature + density_act as k_alpha_static
//   k_point_prep        : the point-shaped ray batch the appearance bodies read: S = 1, N = M, rays[n] = (0, viewdir_n), an
//                         identity list, the device counter = M and, with one shared time, the per-point time row
//   k_point_static_app / k_point_dyn_app : static_app_body / dyn_app_body on that batch (ray_type RDRF_RAY_OTHER, so ray_norm
//                         hands the view directions on as given; no saved rows).  The per-sample lines exist once, in the bodies.
//
// An MFMA column depends on its own sample only, so a point's outputs do not depend on what shares its tile, and they are
// the bits the ray-batch forward gives the same sample.  No atomics on global memory: the deterministic build runs the same
// path.  The call allocates nothing, does not synchronise and reads nothing back.
#include "rdrf_fwd_dev.hpp"
#include "rdrf_render_host.hpp"

// The shared bodies and time_branch_body index with int: idx * 3 (xyz, xw, rgb), n * 6 + 5 (rays) and n * 32 + 31 (tout, the
// largest) must stay below 2^31, which holds up to M = 2^26 - 1.  The limit is a quarter of that; the workspace offsets are
// size_t.  include/rodynrf.h: RDRF_QUERY_POINTS_MAX.
static_assert((long long)RDRF_QUERY_POINTS_MAX * 32 + 31 < (1ll << 31), "time_branch_body forms n * 32 + o in int");

struct PointArgs {
  const float* xyz;    // [M][3] un-normalised
  const float* ts;     // [M] or [1]
  const float* pk;     // packed forward image
  const float* tout;   // [M][32] or [1][32]
  float *sigma, *blending, *xyz_prime;   // each nullable
  float* xw;           // [M][3] or nullptr (no appearance phase follows)
  int M, t_per_point;
  float density_shift;
  int act, dynq;
  Box box;
};

__global__ __launch_bounds__(256) void k_point_time_branch(const float* __restrict__ ts, DynW w, int N, float* __restrict__ tout) {
  __shared__ float s_h[8 * 64];
  time_branch_body(ts, w, N, tout, s_h, grid_ctx());
}

__global__ __launch_bounds__(64 * RDRF_MAXW) void k_point_dyn(PointArgs a, DynW w) {
  __shared__ __attribute__((aligned(16))) float lds[pk::K1_SIZE];
  __shared__ int s_next;
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  if (threadIdx.x == 0) s_next = nwaves;
  lds_fill(lds, a.pk + pk::REG_K1, pk::K1_SIZE);
  const float* pkw = lds;
  const int ntiles = (a.M + 31) >> 5;
  const bool dynq = (a.dynq & 1) != 0;
  for (int k = wave, tile; (tile = blockIdx.x + k * gridDim.x) < ntiles; k = tile_queue_next(&s_next, k, nwaves, dynq)) {
    const int i = tile * 32 + s;
    const bool act = i < a.M;
    const int idx = act ? i : 0;
    const int ti = a.t_per_point ? idx : 0;
    const float t = a.ts[ti];
    const float px[3] = {a.xyz[(size_t)idx * 3 + 0], a.xyz[(size_t)idx * 3 + 1], a.xyz[(size_t)idx * 3 + 2]};
    float xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xn[c] = norm_c(px[c], a.box.lo[c], a.box.inv[c]);
    float X0[32], X1[8], T[16];
    fill_x0(X0, xn[0], xn[1], xn[2], t, h);
    fill_x1(X1, t, h);
    load_tout(T, a.tout, (size_t)ti, h);
    float d[3], xw[3];
    warp_mlp(d, X0, T, pkw, w.l5b, nullptr, s, h, lane);
    warp_point(xw, xn, d, a.box);
    if (act && h == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (a.xyz_prime != nullptr) a.xyz_prime[(size_t)idx * 3 + c] = px[c] + d[c];
        if (a.xw != nullptr) a.xw[(size_t)idx * 3 + c] = xw[c];
      }
    }
    const float fd = head_raw<false>(w, xw, act, X0, X1, pkw, nullptr, s, h, lane);
    const float fb = head_raw<true>(w, xw, act, X0, X1, pkw, nullptr, s, h, lane);
    if (act && h == 0) {
      if (a.sigma != nullptr) a.sigma[idx] = density_act(fd, a.act, a.density_shift);
      if (a.blending != nullptr) a.blending[idx] = sigmoidf_(fb);
    }
  }
}

__global__ __launch_bounds__(256) void k_point_static(PointArgs a, StaticW w) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.M; i += gridDim.x * blockDim.x) {
    const float x0 = norm_c(a.xyz[(size_t)i * 3 + 0], a.box.lo[0], a.box.inv[0]);
    const float x1 = norm_c(a.xyz[(size_t)i * 3 + 1], a.box.lo[1], a.box.inv[1]);
    const float x2 = norm_c(a.xyz[(size_t)i * 3 + 2], a.box.lo[2], a.box.inv[2]);
    a.sigma[i] = density_act(static_density_feature(w.density, x0, x1, x2), a.act, a.density_shift);
  }
}

// ts_row: nullptr, or the [M] row that carries the one shared time to every point (dyn_app_body reads a.ts[n])
__global__ __launch_bounds__(256) void k_point_prep(const float* __restrict__ viewdirs, const float* __restrict__ ts, int M,
                                                    float* __restrict__ rays, int* __restrict__ list, float* __restrict__ ts_row,
                                                    int* __restrict__ counter) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter = M;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
    float* r = rays + (size_t)i * 6;
    r[0] = 0.f; r[1] = 0.f; r[2] = 0.f;
    r[3] = viewdirs[(size_t)i * 3 + 0]; r[4] = viewdirs[(size_t)i * 3 + 1]; r[5] = viewdirs[(size_t)i * 3 + 2];
    list[i] = i;
    if (ts_row != nullptr) ts_row[i] = ts[0];
  }
}

template <int HEAD>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_point_static_app(FieldArgs a, StaticW w) {
  static_app_body<HEAD, false, false>(a, w, nullptr, grid_ctx());
}
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_point_dyn_app(FieldArgs a, DynW w) {
  dyn_app_body<false, false>(a, w, nullptr, grid_ctx());
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct PointWs {
  float* pk;
  int* counter;
  float* rays;     // [M][6]
  int* list;       // [M]
  float* tout;     // dynamic: [M][32] with a time per point, else [1][32]
  float* xw;       // dynamic: [M][3]
  float* ts_row;   // dynamic, one shared time: [M]
};
// one layout for the size call and the launch
static void carve_point(PointWs& p, WsCarver& c, int dynamic, int M, int t_per_point) {
  const size_t m = M > 0 ? (size_t)M : 0;
  memset(&p, 0, sizeof(p));
  p.pk = c.take<float>(PACK_AREA_FLOATS);
  p.counter = c.take<int>(64);
  p.rays = c.take<float>(m * 6);
  p.list = c.take<int>(m);
  if (dynamic) {
    p.tout = c.take<float>((t_per_point ? m : 1) * 32);
    p.xw = c.take<float>(m * 3);
    if (!t_per_point) p.ts_row = c.take<float>(m);
  }
}

extern "C" size_t rdrf_query_points_ws_bytes(int dynamic, int M, int t_per_point) {
  PointWs p;
  WsCarver c;
  carve_point(p, c, dynamic, M, t_per_point);
  return c.off;
}

extern "C" int rdrf_query_points(const void* params, int dynamic, const RdrfFieldCfg* cfg, const float* xyz, int M,
                                 const float* ts, int t_per_point, const float* viewdirs, float* sigma, float* rgb,
                                 float* blending, float* xyz_prime, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0) return 0;   // empty batch: a no-op, as rdrf_compute_alpha
  RDRF_CHECK(params && cfg && xyz && M > 0, -1, "query_points: bad arguments");
  RDRF_CHECK(M <= RDRF_QUERY_POINTS_MAX, -1,
             "query_points: M = %d is above RDRF_QUERY_POINTS_MAX = %d (32-bit point indices): query in smaller chunks", M,
             RDRF_QUERY_POINTS_MAX);
  RDRF_CHECK(rgb == nullptr || viewdirs != nullptr, -1, "query_points: rgb needs viewdirs");
  RDRF_CHECK(!dynamic || ts != nullptr, -1, "query_points: the dynamic field needs ts");
  RDRF_CHECK(dynamic || (blending == nullptr && xyz_prime == nullptr), -1,
             "query_points: blending and xyz_prime are outputs of the dynamic field");
  if (!sigma && !rgb && !blending && !xyz_prime) return 0;   // nothing asked for
  RDRF_CHECK(ws != nullptr, -3, "query_points: no workspace");
  WsCarver c(ws, ws_bytes);
  PointWs p;
  carve_point(p, c, dynamic, M, t_per_point);
  RDRF_CHECK(c.ok(), -3, "query_points: workspace too small: need %zu have %zu", c.off, ws_bytes);

  PointArgs a;
  memset(&a, 0, sizeof(a));
  a.xyz = xyz; a.ts = ts; a.M = M; a.t_per_point = t_per_point ? 1 : 0;
  a.sigma = sigma; a.blending = blending; a.xyz_prime = xyz_prime;
  a.density_shift = cfg->density_shift; a.act = cfg->act;
  a.box = make_box(cfg);
  // the point-shaped ray batch of the appearance bodies: S = 1, N = M, view directions used as given
  FieldArgs f;
  fill_common(f, cfg, p.rays, nullptr, xyz, nullptr, nullptr, M, 1);
  f.ray_type = RDRF_RAY_OTHER;
  f.rgb = rgb; f.list = p.list; f.counter = p.counter; f.xw = p.xw;
  f.dynq = fwd_dynq();
  const long pblocks = ((long)M + 255) / 256;
  const dim3 pgrid((unsigned)(pblocks > 4096 ? 4096 : pblocks));
  const Geo g = geo_for_units(((long)M + 31) / 32);   // the persistent geometry of the field kernels

  if (!dynamic) {
    const RdrfStaticParams* P = (const RdrfStaticParams*)params;
    RDRF_CHECK(vm_ok(P->density, 16, 4) && vm_ok(P->app, 48, 12), -1,
               "query_points: only density comps {16,4,4} / app comps {48,12,12}, the planes and lines of a set spanning one grid, are built");
    StaticW w;
    fill_static_w(w, P);
    if (sigma != nullptr) RDRF_LAUNCH("point_static", k_point_static, pgrid, dim3(256), stream, a, w);
    if (rgb == nullptr) return 0;   // no appearance phase
    RDRF_TRY(pack_image(f.pk, P->packed_fwd, p.pk, stream, static_pack_jobs_fwd, P, cfg->static_head));
    RDRF_LAUNCH("point_prep", k_point_prep, pgrid, dim3(256), stream, viewdirs, ts, M, p.rays, p.list, (float*)nullptr, p.counter);
    if (cfg->static_head == RDRF_HEAD_MLP_FEA)
      RDRF_LAUNCH("point_static_app", k_point_static_app<RDRF_HEAD_MLP_FEA>, dim3(g.grid), dim3(g.block), stream, f, w);
    else
      RDRF_LAUNCH("point_static_app", k_point_static_app<RDRF_HEAD_MLP_FEA_TIMEEMBEDDING>, dim3(g.grid), dim3(g.block), stream, f, w);
    return 0;
  }
  const RdrfDynamicParams* P = (const RdrfDynamicParams*)params;
  RDRF_CHECK(vm_ok(P->density, 16, 4) && vm_ok(P->blending, 16, 4) && vm_ok(P->app, 48, 12) && vm_same_grid(P->density, P->blending), -1,
             "query_points: only density comps {16,4,4} / app comps {48,12,12}, the planes and lines of a set spanning one grid, are built");
  DynW w;
  fill_dyn_w(w, P);
  RDRF_TRY(pack_image(f.pk, P->packed_fwd, p.pk, stream, dyn_pack_jobs_fwd, P));
  a.pk = f.pk; a.tout = p.tout; a.dynq = 1;
  a.xw = rgb != nullptr ? p.xw : nullptr;
  const int rows = t_per_point ? M : 1;
  RDRF_LAUNCH("time_branch", k_point_time_branch, dim3((rows + 7) / 8), dim3(256), stream, ts, w, rows, p.tout);
  RDRF_LAUNCH("point_dyn", k_point_dyn, dim3(g.grid), dim3(g.block), stream, a, w);
  if (rgb == nullptr) return 0;   // no appearance phase
  RDRF_LAUNCH("point_prep", k_point_prep, pgrid, dim3(256), stream, viewdirs, ts, M, p.rays, p.list, p.ts_row, p.counter);
  f.ts = t_per_point ? ts : p.ts_row;
  RDRF_LAUNCH("point_dyn_app", k_point_dyn_app, dim3(g.grid), dim3(g.block), stream, f, w);
  return 0;
}
