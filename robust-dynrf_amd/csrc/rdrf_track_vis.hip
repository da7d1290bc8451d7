// rdrf_track_vis.hip -- per-slot visibility of a point track: the transmittance T_full of raw2outputs (renderer.py:236-245)
// from camera k to the point p = pts[i][k] of slot k, along the ray of camera k through the point's own pixel.
//
// Meaning (include/rodynrf.h has the contract): the slot's ray is sampled by the field's no-jitter sampler, both fields'
// sigma and the blending are those forward() gives the samples of that ray at the slot's time, and with the compositor's
//     F_s(d) = (1 - (1 - exp(-sigma_d d)) b) (1 - (1 - exp(-sigma_s d)) (1 - b)) + 1e-10
//     vis = prod_{s < j} F_s(dists_s) * F_j(min(zq - z_j, z_{j+1} - z_j) |d| distance_scale),  j = the last sample with z_j <= zq
// where zq = z* - margin is the query depth.  The launch sequence:
//
//   k_track_vis_rays : a lane per slot: the slot's time (t0 stepped by dt as k_track_points steps it), the projection of p
//                      into camera k (flow_ray_fwd: the bits of the track's own pixels), the camera's ray through that pixel
//                      (camera_ray: k_camera_rays' arithmetic), z* and zq, the behind-camera flag
//   sampler          : rdrf_sample_ndc / rdrf_sample_contract on the MK rays
//   time branch      : launch_list_time_branch (clears the list counter on its way)
//   k_track_vis_keep : one pass over the [MK * S] samples: the flat index of every sample with valid && z < zq appended to
//                      ONE list (both fields keep the same samples: one append per workgroup), zeros in sigma_s, sigma_d and
//                      blending of every other sample
//   k_static_density_list, k_dyn_density_list (rdrf_render_masked.hip) on that list: a listed sample gets forward()'s bits;
//                      no sample behind the point reaches a density kernel and no appearance phase runs
//   k_track_vis_scan : a wave per slot, see there
//
// The list's order depends on the arrival of the workgroups; a sample's values depend on that sample alone and a slot's product
// on its own samples in a fixed order, so no result depends on it and the deterministic build runs the same path.
#include "rdrf_misc_dev.hpp"
#include "rdrf_render_host.hpp"

struct VisRayArgs {
  const float *pts, *t0;      // [M][K][3], [M]
  const float *c2w, *focal;   // [K][3][4], one float
  int MK, K, n_bwd, H, W, ray_type;
  float dt, margin;
  float *rays, *ts, *zq;      // [MK][6], [MK], [MK]
  uint8_t* behind;            // [MK]
};

__global__ __launch_bounds__(256) void k_track_vis_rays(VisRayArgs a) {
#pragma clang fp contract(off)
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.MK) return;
  const int i = o / a.K, k = o - i * a.K;
  // the slot's time: the chain of k_track_points (track_step), one rounded sum per step
  float t = a.t0[i];
  for (int q = a.n_bwd; q < k; ++q) t = t + a.dt;
  for (int q = a.n_bwd; q > k; --q) t = t - a.dt;
  const float p[3] = {a.pts[(size_t)o * 3 + 0], a.pts[(size_t)o * 3 + 1], a.pts[(size_t)o * 3 + 2]};
  const float* M = a.c2w + (size_t)k * 12;
  const float f = a.focal[0];
  // projection into camera k as track_emit does it: a weight-1, one-sample "ray" through flow_ray_fwd
  const float zero_ray[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  FlowRay r;
  float u, v, d;
  flow_ray_fwd(r, zero_ray, M, 1.0f, p, a.H, a.W, f, a.ray_type, u, v, d);
  float ray[6];
  camera_ray(M, f, u, v, a.H, a.W, a.ray_type == RDRF_RAY_NDC ? 1 : 0, 1.0f, ray);
  // depth of the point on that ray, in z_vals units.  ndc: the ray runs from z_ndc = -1 to 1 over [0, 1]; contract: the
  // camera's direction has z = -1, so the depth is the distance along the optical axis
  const float zs = a.ray_type == RDRF_RAY_NDC ? (r.c + 1.0f) / 2.0f : -r.cam[2];
  const bool behind = r.cam[2] >= 0.0f;
  float zq = zs - a.margin;
  if (behind) zq = -INFINITY;   // nothing of this ray is listed (its pixel is the mirror image's: meaningless samples)
  for (int c = 0; c < 6; ++c) a.rays[(size_t)o * 6 + c] = ray[c];
  a.ts[o] = t;
  a.zq[o] = zq;
  a.behind[o] = behind ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// k_track_vis_keep: k_keep's shape (rdrf_render_masked.hip) with the point's depth in the place of the masks -- a workgroup
// owns 2048 consecutive samples and appends once.  A NaN zq keeps nothing; without zq (the density-only surface hits,
// rdrf_hits.hip) every valid sample is kept.
// ------------------------------------------------------------------------------------------------
constexpr int VIS_KEEP_ROUNDS = 8;

struct VisKeepArgs {
  const float* z;         // [MK * S]
  const uint8_t* valid;   // [MK * S] of the sampler
  const float* zq;        // [MK]; nullptr: no depth test
  int ns, S;
  int *list, *count;
  float *sigma_s, *sigma_d, *blending;
};

__global__ __launch_bounds__(256) void k_track_vis_keep(VisKeepArgs a) {
  __shared__ int s_cnt[16];
  const int i0 = blockIdx.x * (256 * VIS_KEEP_ROUNDS) + threadIdx.x;
  unsigned kb = 0;   // bit r: the thread's sample of round r is kept
  int cnt = 0;       // wave-uniform
#pragma unroll 1
  for (int r = 0; r < VIS_KEEP_ROUNDS; ++r) {
    const int i = i0 + r * 256;
    const bool act = i < a.ns;
    const bool keep = act && a.valid[i] != 0 && (a.zq == nullptr || a.z[i] < a.zq[i / a.S]);
    if (act && !keep) {
      a.sigma_s[i] = 0.0f;
      a.sigma_d[i] = 0.0f;
      a.blending[i] = 0.0f;
    }
    kb |= (keep ? 1u : 0u) << r;
    cnt += __popcll(__ballot(keep));
  }
  int base = block_append_base(a.count, cnt, s_cnt, threadIdx.x, blockDim.x);
#pragma unroll 1
  for (int r = 0; r < VIS_KEEP_ROUNDS; ++r) {
    const int i = i0 + r * 256;
    const bool m = ((kb >> r) & 1u) != 0;
    const unsigned long long bal = __ballot(m);
    if (m) a.list[base + ballot_rank(bal)] = i;
    base += __popcll(bal);
  }
}

// ------------------------------------------------------------------------------------------------
// k_track_vis_scan: a wave per slot (a workgroup of VIS_SCAN_WAVES waves walks the slots with the stride of the grid, at most
// VIS_SCAN_MAX_BLOCKS workgroups).  The order of the product, which depends on S and j alone:
//   1. j = (number of samples with z_s <= zq) - 1 (the sampler's z ascend along a ray); j < 0: vis = 1.0.
//   2. The samples go through the wave in rounds of 64, sample s of a round in lane s - j0, as in the compositor
//      (composite_body): factor F_s(dists_s) by alpha_of and tfull_factor, inclusive product scan over the round
//      (scan_mul64: Hillis-Steele, lane l multiplies in lane l - d for d = 1, 2, 4 .. 32), T = carry * (scan of lane - 1, 1.0
//      in lane 0), carry *= scan of lane 63.  The rounds stop with the one that holds j.
//   3. Lane j - j0 of that round holds T_j = the compositor's T_full[j] for these sigmas, bit for bit, and T_{j+1} = carry *
//      (its own scan value).  Two scans associate their products differently, so T_{j+1} can come out an ulp ABOVE T_j F_j where
//      the density is next to nothing; a visibility must not rise with depth, so the lane takes the running minimum
//      m_s = min_{i <= s} T_i (a min scan of the same shape, carried from round to round) and writes
//          vis = max(m_j * F_j(min(zq - z_j, z_{j+1} - z_j) |d| distance_scale), m_{j+1})
//      (no lower end for the last sample, whose interval has width 0, as its dists).  m_j F_j <= m_j as F <= 1, so vis is
//      non-increasing in zq within an interval and across intervals.  For zq = z_j the partial factor is exactly 1.0 and
//      vis = m_j, which is T_full[j] wherever the scan's T did not rise.
// A slot behind its camera gets 0.0, a NaN query depth NaN.
// ------------------------------------------------------------------------------------------------
constexpr int VIS_SCAN_WAVES = 4;
constexpr int VIS_SCAN_MAX_BLOCKS = 2048;

struct VisScanArgs {
  const float *rays, *z, *zq;
  const uint8_t* behind;
  const float *sigma_s, *sigma_d, *blending;
  int MK, S, ray_type;
  float distance_scale;
  float* vis;   // [MK]
};

__global__ __launch_bounds__(64 * VIS_SCAN_WAVES) void k_track_vis_scan(VisScanArgs a) {
  const int lane = threadIdx.x & 63;
  const int S = a.S;
  for (int n = blockIdx.x * VIS_SCAN_WAVES + (threadIdx.x >> 6); n < a.MK; n += gridDim.x * VIS_SCAN_WAVES) {   // (wave-uniform)
    const float zq = a.zq[n];
    if (a.behind[n] != 0 || zq != zq) {
      if (lane == 0) a.vis[n] = a.behind[n] != 0 ? 0.0f : zq;
      continue;
    }
    int cnt = 0;
    for (int j0 = 0; j0 < S; j0 += 64) {
      const int s = j0 + lane;
      cnt += __popcll(__ballot(s < S && a.z[(size_t)n * S + (s < S ? s : 0)] <= zq));
    }
    const int j = cnt - 1;
    if (j < 0) {
      if (lane == 0) a.vis[n] = 1.0f;
      continue;
    }
    float vx, vy, vz;
    const float nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
    float cf = 1.0f, mc = 1.0f;   // carries: the product and the smallest T of the rounds before
    for (int j0 = 0; j0 <= j; j0 += 64) {
      const int s = j0 + lane;
      const RaySample q = ray_sample(a.z, a.sigma_s, a.sigma_d, a.blending, n, S, s, nrm, a.distance_scale);
      float Tf, Tn, mn;   // T_s (T_{j+1} in the lanes behind j), T_{s+1}, m_s
      tfull_min_round(s <= j ? q.pf : 1.0f, lane, cf, mc, Tf, Tn, mn);
      if (s == j) {
        const float dq = fminf(zq - q.zs, q.width) * nrm * a.distance_scale;
        const float pq = tfull_factor(alpha_of(q.sg_d, dq), alpha_of(q.sg_s, dq), q.b);
        const float v = mn * pq;
        a.vis[n] = j + 1 < S ? fmaxf(v, fminf(mn, Tn)) : v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
void carve_density_only(DensityBufs& b, WsCarver& c, size_t N, size_t S) {
  const size_t ns = N * S;
  b.xyz = c.take<float>(ns * 3);
  b.z = c.take<float>(ns);
  b.valid = c.take<uint8_t>(ns);
  b.sigma_s = c.take<float>(ns);
  b.sigma_d = c.take<float>(ns);
  b.blending = c.take<float>(ns);
  b.xyz_prime = c.take<float>(ns * 3);
  b.xw = c.take<float>(ns * 3);
  b.tout = c.take<float>(N * 32);
  b.list = c.take<int>(ns);
  b.ctr = c.take<int>(64);
  b.pk = c.take<float>(PACK_AREA_FLOATS);
}

int density_only_run(const RenderCall& call, const DensityBufs& b, const float* zq, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int N = call.N, S = call.S, ns = N * S;
  RenderBufs rb;
  memset(&rb, 0, sizeof(rb));
  rb.xyz = b.xyz; rb.z = b.z; rb.valid = b.valid;
  RDRF_TRY(render_sample(call, rb, stream_));

  // the fields' launch arguments: the static list kernel reads xyz and writes sigma; the dynamic one also reads the rays'
  // times and time branches and its weight image, and writes blending, xyz_prime and xw of the listed samples
  FieldArgs as, ad;
  StaticW wst;
  DynW wdy;
  fill_common(as, call.cfg_s, call.rays, call.ts, b.xyz, b.z, b.valid, N, S);
  as.sigma = b.sigma_s;
  fill_common(ad, call.cfg_d, call.rays, call.ts, b.xyz, b.z, b.valid, N, S);
  ad.sigma = b.sigma_d; ad.blending = b.blending; ad.xyz_prime = b.xyz_prime; ad.xw = b.xw; ad.tout = b.tout;
  ad.dynq = fwd_dynq();
  fill_static_w(wst, call.PS);
  fill_dyn_w(wdy, call.PD);
  RDRF_TRY(pack_image(ad.pk, call.PD->packed_fwd, b.pk, stream, dyn_pack_jobs_fwd, call.PD));

  RDRF_TRY(launch_list_time_branch(call.ts, wdy, N, b.tout, b.ctr, stream));   // clears the counter block
  VisKeepArgs k;
  memset(&k, 0, sizeof(k));
  k.z = b.z; k.valid = b.valid; k.zq = zq; k.ns = ns; k.S = S;
  k.list = b.list; k.count = b.ctr + CTR_KEPT_S;
  k.sigma_s = b.sigma_s; k.sigma_d = b.sigma_d; k.blending = b.blending;
  RDRF_LAUNCH("track_vis_keep", k_track_vis_keep, dim3((ns + 256 * VIS_KEEP_ROUNDS - 1) / (256 * VIS_KEEP_ROUNDS)), dim3(256),
              stream, k);
  // one list, one length (at CTR_KEPT_S) for both fields
  RDRF_TRY(launch_static_density_list(as, wst, b.list, b.ctr, nullptr, stream));
  RDRF_TRY(launch_dyn_density_list(ad, wdy, b.list, b.ctr + CTR_KEPT_S, stream));
  return 0;
}

struct VisBufs {
  float *rays, *ts, *zq;
  uint8_t* behind;
  DensityBufs d;
};
static void carve_track_vis(VisBufs& b, WsCarver& c, size_t MK, size_t S) {
  b.rays = c.take<float>(MK * 6);
  b.ts = c.take<float>(MK);
  b.zq = c.take<float>(MK);
  b.behind = c.take<uint8_t>(MK);
  carve_density_only(b.d, c, MK, S);
}

extern "C" size_t rdrf_track_visibility_ws_bytes(int M, int K, int S) {
  VisBufs b;
  WsCarver c;
  carve_track_vis(b, c, (size_t)(M < 0 ? 0 : M) * (size_t)(K < 0 ? 0 : K), (size_t)(S < 0 ? 0 : S));
  return c.off;
}

extern "C" int rdrf_track_visibility_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                         const RdrfFieldCfg* cfg_d, const float* pts, const float* t0, int M, int n_fwd,
                                         int n_bwd, float dt, const RdrfTrackCams* cams, int S, float near, float far,
                                         float margin, float* vis, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(PS && cfg_s && PD && cfg_d && M >= 0 && S > 0, -1, "track_visibility: bad arguments");
  RDRF_CHECK(n_fwd >= 0 && n_bwd >= 0, -1, "track_visibility: n_fwd and n_bwd are step counts >= 0 (got %d, %d)", n_fwd, n_bwd);
  RDRF_CHECK((cfg_d->ray_type == RDRF_RAY_NDC || cfg_d->ray_type == RDRF_RAY_CONTRACT) && cfg_s->ray_type == cfg_d->ray_type, -1,
             "track_visibility: ray_type must be ndc or contract, the same for both fields (renderer.py:1335-1351)");
  const long long K = (long long)n_bwd + 1 + n_fwd;
  RDRF_CHECK(cams != nullptr && cams->K == (int)K && K < (long long)INT32_MAX, -1,
             "track_visibility: one camera per slot: n_bwd + 1 + n_fwd = %lld slots, %d cameras", K, cams ? cams->K : 0);
  RDRF_CHECK(cams->H > 0 && cams->W > 0 && cams->focal && cams->c2w, -1,
             "track_visibility: bad cameras (H, W > 0; focal, c2w device pointers)");
  if (M == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(pts && t0 && vis && ws, -1, "track_visibility: no points / times / output / workspace");
  RDRF_CHECK((size_t)M * (size_t)K * (size_t)S * 3 < (size_t)INT32_MAX, -1,
             "track_visibility: M * K * S * 3 must stay below 2^31 (32-bit sample indices): call in chunks of points");
  const int MK = (int)((long long)M * K);
  VisBufs b;
  WsCarver c(ws, ws_bytes);
  carve_track_vis(b, c, (size_t)MK, (size_t)S);
  RDRF_CHECK(c.ok(), -3, "track_visibility: workspace too small: need %zu have %zu", c.off, ws_bytes);
  RenderCall call = {PS, cfg_s, PD, cfg_d, b.rays, b.ts, MK, S, near, far, 0.f, {}, ws, ws_bytes};
  RDRF_TRY(render_check_fields(call, "track_visibility"));

  VisRayArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.pts = pts; ra.t0 = t0; ra.c2w = cams->c2w; ra.focal = cams->focal;
  ra.MK = MK; ra.K = (int)K; ra.n_bwd = n_bwd; ra.H = cams->H; ra.W = cams->W; ra.ray_type = cfg_d->ray_type;
  ra.dt = dt; ra.margin = margin;
  ra.rays = b.rays; ra.ts = b.ts; ra.zq = b.zq; ra.behind = b.behind;
  RDRF_LAUNCH("track_vis_rays", k_track_vis_rays, dim3((MK + 255) / 256), dim3(256), stream, ra);

  // sampler, time branch, keep pass (valid && z < zq) and both list-driven density kernels
  RDRF_TRY(density_only_run(call, b.d, b.zq, stream_));

  VisScanArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.rays = b.rays; sa.z = b.d.z; sa.zq = b.zq; sa.behind = b.behind;
  sa.sigma_s = b.d.sigma_s; sa.sigma_d = b.d.sigma_d; sa.blending = b.d.blending;
  sa.MK = MK; sa.S = S; sa.ray_type = cfg_d->ray_type;
  sa.distance_scale = cfg_d->distance_scale;   // the compositor reads the dynamic field's dists
  sa.vis = vis;
  const int blocks = (MK + VIS_SCAN_WAVES - 1) / VIS_SCAN_WAVES;
  RDRF_LAUNCH("track_vis_scan", k_track_vis_scan, dim3(blocks > VIS_SCAN_MAX_BLOCKS ? VIS_SCAN_MAX_BLOCKS : blocks),
              dim3(64 * VIS_SCAN_WAVES), stream, sa);
  return 0;
}
