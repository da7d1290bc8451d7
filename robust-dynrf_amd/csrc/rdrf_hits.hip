// rdrf_hits.hip -- surface hits: per ray the depth at which the compositor's transmittance falls to a given level, the point
// there and the dynamic field's share of the sample it lies in (include/rodynrf.h has the contract).
//
// With the compositor's factor F_s(d) = (1 - (1 - exp(-sigma_d d)) b) (1 - (1 - exp(-sigma_s d)) (1 - b)) + 1e-10, T_s =
// T_full[s] as rdrf_composite_fwd forms it and m_s = min_{i <= s} T_i, the hit sample of the level L = 1 - tau is the first
// j with m_{j+1} <= L, and the hit depth lies in [z_j, z_{j+1}] where m_j F_j(d) = L: the inverse of k_track_vis_scan
// (rdrf_track_vis.hip), which evaluates the same T(z) at a given depth.  The running minimum is what makes "the first j" and
// the order of the levels well defined: two scans associate their products differently, so T_{s+1} can come out an ulp above
// T_s where there is next to no density, and m never rises.
//
// Launch sequences of rdrf_render_hits_fwd:
//   maps != NULL : render_run (the launch sequence of rdrf_render_maps_fwd, same bits in every map), then k_render_hits on the
//                  render's own z, sigma_s, sigma_d and blending planes
//   maps == NULL : density_only_run without a depth test (sampler, time branch, k_track_vis_keep over every valid sample,
//                  k_static_density_list, k_dyn_density_list), then k_render_hits; no appearance phase
// A listed sample has forward()'s bits and every other sample zeros, as forward() gives them, so both paths hand the kernel
// the same planes.  rdrf_hits_from_planes is the kernel alone.
#include "rdrf_misc_dev.hpp"
#include "rdrf_render_host.hpp"

// ------------------------------------------------------------------------------------------------
// k_render_hits: a wave per ray (a workgroup of HITS_WAVES waves walks the rays with the stride of the grid, at most
// HITS_MAX_BLOCKS workgroups), the samples in rounds of 64 as in k_track_vis_scan: ray_sample and tfull_min_round
// (rdrf_misc_dev.hpp) give lane s - j0 the factor F_s(dists_s), T_s, T_{s+1} and m_s, and m_{s+1} = min(m_s, T_{s+1}).
//   crossing  per level, in ascending tau (descending L): a ballot of m_{s+1} <= L over the lanes with s + 1 < S; the first
//             set lane owns the hit.  The last sample has no width (its dists is 0, its factor 1 + 1e-10), so in exact
//             arithmetic it is never the first to cross; it is not a candidate, and a level that only it could cross through
//             the scan's rounding is a miss.  No lane set: the level and all after it wait for the next round.  The rounds
//             stop once the last level has crossed.
//   solver    the owner's m_j, sigmas, b, dists_j and z go to the whole wave (readlane), and the wave finds the SMALLEST fp32
//             fraction t in (0, 1] with  m_j * F_j(t dists_j) <= L  (fp32, the compositor's own alpha_of / tfull_factor) by a
//             64-section over t's bit pattern: positive floats order as their bits, [0, bits(1.0f)] holds fewer than 2^30
//             patterns, so HITS_SOLVE_ROUNDS = 5 rounds of 64 trial points (steps 2^24, 2^18, 2^12, 2^6, 1), a ballot each,
//             end at one pattern.  The count is fixed and depends on nothing in the data; t = 1 is taken as crossed (the scan
//             said so), so t never leaves [0, 1].  m_j <= L already (j = 0 or the 1e-10): t = 0.  Searching the bit pattern
//             and not a uniform grid keeps t's RELATIVE error at one ulp, which is what bounds the residual at a wall, where
//             the crossing lies at a tiny fraction of the interval.  The answer is a function of (m_j, the sample, L) alone,
//             and, the predicate being non-increasing in t and in L, non-decreasing in tau.
//   outputs   z_hit = min(z_j + t (z_{j+1} - z_j), z_{j+1}), the point by ray_point (the samplers' arithmetic: z_hit = z_s
//             gives xyz_s's bits), owner = a_d b / (a_d b + a_s (1 - b)) of the whole sample (0 where the sum is 0).
//   miss      no crossing within the ray: hit = 0, z = z_{S-1}, the last sample's point, owner = 0.
//   NaN       a NaN factor (sigma, blending or z) in lane f: levels that cross in a lane before f are answered as usual,
//             every other level gets hit = 0 and NaN in z, xyz and owner, and the ray is done.
// Every product is formed in an order that depends on S and j alone; nothing is accumulated across rays or levels.
//
// Traffic: the kernel reads the z, sigma_s, sigma_d and blending planes once (z twice per lane, the neighbour from cache)
// and no dists plane -- it re-forms dists from z and |d| as the fields do -- so a ray that runs to its end costs
// 4 planes * 4 bytes * S = 16 S bytes of reads (20 S with a stored dists plane, the five planes the compositor reads),
// plus 24 bytes of the ray and 21 bytes of output per level.  The arithmetic per round is the compositor's for one of its
// three products, and a solve is 5 evaluations of one factor on the wave: the kernel is bound by those plane reads
// (profiles/hits_speed.txt: 0.06 ms for a 135 x 240 frame at S = 270).
// ------------------------------------------------------------------------------------------------
constexpr int HITS_WAVES = 4;
constexpr int HITS_MAX_BLOCKS = 2048;
constexpr int HITS_SOLVE_ROUNDS = 5;
constexpr int HITS_MAX_TAU = 8;

struct HitsArgs {
  const float *rays, *z, *sigma_s, *sigma_d, *blending;   // [N][6], [N][S] x 4
  int N, S, ray_type, n_tau;
  float distance_scale;
  float L[HITS_MAX_TAU];   // 1 - tau, descending
  float* oz;               // [n_tau][N]      each nullable
  uint8_t* ohit;           // [n_tau][N]
  float* oxyz;             // [n_tau][N][3]
  float* oowner;           // [n_tau][N]
};

RDRF_D void hits_write(const HitsArgs& a, int k, int n, float zh, int hit, const float* ray, float owner, bool nan) {
  const size_t o = (size_t)k * a.N + n;
  if (a.oz) a.oz[o] = zh;
  if (a.ohit) a.ohit[o] = (uint8_t)hit;
  if (a.oowner) a.oowner[o] = owner;
  if (a.oxyz) {
    float p[3];
    ray_point(ray, zh, a.ray_type == RDRF_RAY_CONTRACT ? 1 : 0, p);
    for (int c = 0; c < 3; ++c) a.oxyz[o * 3 + c] = nan ? zh : p[c];
  }
}

// the dynamic field's share of a sample: a_d b / (a_d b + a_s (1 - b)), 0 where the denominator is 0
RDRF_D float hits_owner(float sg_d, float sg_s, float b, float ds) {
#pragma clang fp contract(off)
  const float num = alpha_of(sg_d, ds) * b;
  const float den = num + alpha_of(sg_s, ds) * (1.0f - b);
  return den == 0.0f ? 0.0f : num / den;
}

__global__ __launch_bounds__(64 * HITS_WAVES) void k_render_hits(HitsArgs a) {
  const int lane = threadIdx.x & 63;
  const int S = a.S, nt = a.n_tau;
  for (int n = blockIdx.x * HITS_WAVES + (threadIdx.x >> 6); n < a.N; n += gridDim.x * HITS_WAVES) {   // (wave-uniform)
    float vx, vy, vz;
    const float nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
    const float* ray = a.rays + (size_t)n * 6;
    float cf = 1.0f, mc = 1.0f;   // carries: the product and the smallest T of the rounds before
    int next = 0;                 // the first level that has not crossed (wave-uniform)
    for (int j0 = 0; j0 < S && next < nt; j0 += 64) {
      const int s = j0 + lane;
      const bool act = s < S;
      const RaySample q = ray_sample(a.z, a.sigma_s, a.sigma_d, a.blending, n, S, s, nrm, a.distance_scale);
      float Tf, Tn, mn;   // T_s, T_{s+1}, m_s
      tfull_min_round(act ? q.pf : 1.0f, lane, cf, mc, Tf, Tn, mn);
      const float m1 = fminf(mn, Tn);   // m_{s+1}
      const unsigned long long nanb = __ballot(act && !(q.pf == q.pf));
      const int fnan = nanb ? __ffsll((long long)nanb) - 1 : 64;
      const bool cand = act && s + 1 < S && lane < fnan;
      while (next < nt) {
        const float L = a.L[next];
        const unsigned long long bal = __ballot(cand && m1 <= L);
        if (!bal) break;
        const int f = __ffsll((long long)bal) - 1;   // the owning lane (wave-uniform)
        const float mj = __shfl(mn, f, 64), sg_d = __shfl(q.sg_d, f, 64), sg_s = __shfl(q.sg_s, f, 64);
        const float b = __shfl(q.b, f, 64), ds = __shfl(q.ds, f, 64);
        float t = 0.0f;
        if (!(mj <= L)) {
          constexpr unsigned TOP = 0x3F800000u;   // bits of 1.0f
          unsigned u0 = 0;   // invariant: not crossed at u0 (t = 0: m_j > L), crossed at u0 + 64 * step
#pragma unroll
          for (int r = 0; r < HITS_SOLVE_ROUNDS; ++r) {
            const unsigned step = 1u << (6 * (HITS_SOLVE_ROUNDS - 1 - r));
            const unsigned ut = u0 + (unsigned)(lane + 1) * step;
            bool crossed = ut >= TOP;
            if (!crossed) {
              const float d = __uint_as_float(ut) * ds;
              crossed = mj * tfull_factor(alpha_of(sg_d, d), alpha_of(sg_s, d), b) <= L;
            }
            const unsigned long long cb = __ballot(crossed);   // never empty: lane 63 sits on the point known to have crossed
            u0 += (unsigned)(cb ? __ffsll((long long)cb) - 1 : 63) * step;
          }
          t = __uint_as_float(u0 + 1 < TOP ? u0 + 1 : TOP);
        }
        if (lane == f) {
#pragma clang fp contract(off)
          const float zh = fminf(q.zs + t * q.width, q.zn);
          hits_write(a, next, n, zh, 1, ray, hits_owner(sg_d, sg_s, b, ds), false);
        }
        ++next;
      }
      if (nanb != 0 && next < nt) {   // a NaN in front of every crossing that is left
        const float qnan = __uint_as_float(0x7FC00000u);
        for (int k = next + lane; k < nt; k += 64) hits_write(a, k, n, qnan, 0, ray, qnan, true);
        next = nt;
      }
    }
    // misses: the levels the ray never reached
    for (int k = next + lane; k < nt; k += 64) {
      const float zl = a.z[(size_t)n * S + (S - 1)];
      hits_write(a, k, n, zl, 0, ray, 0.0f, false);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int hits_check_taus(const float* taus, int n_tau, const RdrfHits* out, const char* who) {
  RDRF_CHECK(out != nullptr, -1, "%s: no RdrfHits", who);
  RDRF_CHECK(taus != nullptr && n_tau >= 1 && n_tau <= HITS_MAX_TAU, -1, "%s: 1 to %d opacity levels per call (got %d)", who,
             HITS_MAX_TAU, n_tau);
  for (int k = 0; k < n_tau; ++k) {
    RDRF_CHECK(taus[k] > 0.0f && taus[k] < 1.0f, -1, "%s: tau[%d] = %g is not in (0, 1)", who, k, (double)taus[k]);
    RDRF_CHECK(k == 0 || taus[k] > taus[k - 1], -1, "%s: the levels must ascend strictly (tau[%d] = %g after %g)", who, k,
               (double)taus[k], (double)taus[k - 1]);
  }
  return 0;
}

static int launch_hits(const float* rays, const float* z, const float* sigma_s, const float* sigma_d, const float* blending,
                       int N, int S, int ray_type, float distance_scale, const float* taus, int n_tau, const RdrfHits* out,
                       hipStream_t stream) {
  if (!out->z && !out->hit && !out->xyz && !out->owner) return 0;
  HitsArgs a;
  memset(&a, 0, sizeof(a));
  a.rays = rays; a.z = z; a.sigma_s = sigma_s; a.sigma_d = sigma_d; a.blending = blending;
  a.N = N; a.S = S; a.ray_type = ray_type; a.n_tau = n_tau;
  a.distance_scale = distance_scale;
  for (int k = 0; k < n_tau; ++k) a.L[k] = 1.0f - taus[k];   // rounded once
  a.oz = out->z; a.ohit = out->hit; a.oxyz = out->xyz; a.oowner = out->owner;
  const int blocks = (N + HITS_WAVES - 1) / HITS_WAVES;
  RDRF_LAUNCH("render_hits", k_render_hits, dim3(blocks > HITS_MAX_BLOCKS ? HITS_MAX_BLOCKS : blocks), dim3(64 * HITS_WAVES),
              stream, a);
  return 0;
}

extern "C" int rdrf_hits_from_planes(const float* rays, const float* z, const float* sigma_s, const float* sigma_d,
                                     const float* blending, int N, int S, int ray_type, float distance_scale, const float* taus,
                                     int n_tau, const RdrfHits* out, rdrf_stream_t stream) {
  RDRF_CHECK(N >= 0 && S > 0, -1, "hits_from_planes: bad arguments (N %d, S %d)", N, S);
  RDRF_CHECK(ray_type == RDRF_RAY_NDC || ray_type == RDRF_RAY_CONTRACT, -1,
             "hits_from_planes: ray_type must be ndc or contract (the point of a hit is the sampler's, and world-space rays have "
             "no sampler without the field's step)");
  RDRF_TRY(hits_check_taus(taus, n_tau, out, "hits_from_planes"));
  if (N == 0) return 0;
  RDRF_CHECK(rays && z && sigma_s && sigma_d && blending, -1, "hits_from_planes: no rays / planes");
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX && (size_t)N * 6 < (size_t)INT32_MAX, -1,
             "hits_from_planes: N * S * 3 and N * 6 must stay below 2^31: call in chunks of rays");
  return launch_hits(rays, z, sigma_s, sigma_d, blending, N, S, ray_type, distance_scale, taus, n_tau, out, (hipStream_t)stream);
}

extern "C" size_t rdrf_render_hits_ws_bytes(int N, int S) {
  DensityBufs b;
  WsCarver c;
  carve_density_only(b, c, (size_t)(N < 0 ? 0 : N), (size_t)(S < 0 ? 0 : S));
  const size_t render = rdrf_render_workspace_bytes(N < 0 ? 0 : N, S < 0 ? 0 : S);
  return c.off > render ? c.off : render;
}

extern "C" int rdrf_render_hits_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                    const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near,
                                    float far, const float* taus, int n_tau, const RdrfRenderMaps* maps, const RdrfHits* out,
                                    void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(PS && cfg_s && PD && cfg_d && N >= 0 && S > 0, -1, "render_hits: bad arguments");
  RDRF_CHECK((cfg_d->ray_type == RDRF_RAY_NDC || cfg_d->ray_type == RDRF_RAY_CONTRACT) && cfg_s->ray_type == cfg_d->ray_type, -1,
             "render_hits: ray_type must be ndc or contract, the same for both fields (world-space rays are not built here)");
  RDRF_TRY(hits_check_taus(taus, n_tau, out, "render_hits"));
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, 0.f, {}, ws, ws_bytes};
  RDRF_TRY(render_check_args(c, "render_hits", "ray_type ndc / contract only"));
  RDRF_TRY(render_check_fields(c, "render_hits"));
  RDRF_CHECK(ws != nullptr && ws_bytes >= rdrf_render_hits_ws_bytes(N, S), -3, "render_hits: workspace too small: need %zu have %zu",
             rdrf_render_hits_ws_bytes(N, S), ws_bytes);
  if (maps != nullptr) {
    // the render itself: the launch sequence, same bits in every requested map (the carve does not depend on `out`)
    maps_to_slots(c.want, maps);
    RenderBufs b;
    RDRF_TRY(render_run(c, RDRF_RENDER_AUTO, "render_hits", b, stream_));
    return launch_hits(rays, b.z, b.sigma_s, b.sigma_d, b.blending, N, S, cfg_d->ray_type, cfg_d->distance_scale, taus, n_tau, out,
                       stream);
  }
  DensityBufs b;
  WsCarver wc(ws, ws_bytes);
  carve_density_only(b, wc, (size_t)N, (size_t)S);
  RDRF_TRY(density_only_run(c, b, nullptr, stream_));
  return launch_hits(rays, b.z, b.sigma_s, b.sigma_d, b.blending, N, S, cfg_d->ray_type, cfg_d->distance_scale, taus, n_tau, out,
                     stream);   // the compositor reads the dynamic field's dists: its distance_scale
}
