// rdrf_render_masked.hip -- the no-grad render of a ray chunk with alpha-grid masks: the density phase of either field
// runs on the samples its mask keeps and on no other.
//
// Meaning (what the launch sequence below reproduces bit for bit): sample -> valid_s = valid & (mask_s > 0),
// valid_d = valid & (mask_d > 0) (rdrf_alpha_mask_valid) -> static forward with valid_s, dynamic forward with valid_d ->
// compositor.  The dense density kernels evaluate a dropped sample in full and then force its sigma to 0; here
//
//   k_keep               : one pass over the [N * S] samples: both masks at (xyz, ts[ray]), the two valid planes, the flat
//                          index of every kept sample appended to list_s / list_d (one append per workgroup and list), and
//                          zeros where the later phases read a dropped sample (sigma of both fields, blending)
//   k_static_density_list: a lane per listed sample, static_density_feature -> sigma
//   k_static_scan        : the per-ray half of static_density_body (wave per ray; zero_rgb_round<64>, weight_round<64>,
//                          append_masked<64>) over all N * S sigmas: weight, dists, app-mask compaction, zero fill of the
//                          colours
//   k_dyn_density_list   : 32-entry tiles of list_d through the per-sample functions dyn_density_body calls (load_tout,
//                          warp_mlp, warp_point, head_raw; FLAT form: time and tout through the sample's ray).  An MFMA
//                          column depends on its own sample only, so a listed sample gets the bits k_dyn_density_flat
//                          gives it
// (the shared functions: rdrf_fwd_dev.hpp)
//   k_masked_ray_scan    : ray_scan_body, unchanged
//   appearance kernels, compositor: the bodies / the entry point of the unmasked render
//
// The tile counts come from the device-side list lengths; the grids are sized for the worst case (no host sync).  A list's
// order depends on the arrival of the workgroups; a sample's values depend on that sample alone, so no result depends on it
// and the deterministic build runs the same path.
#include "rdrf_fwd_dev.hpp"
#include "rdrf_mask_dev.hpp"
#include "rdrf_render_host.hpp"

// the four device counters of a call (CTR_*: rdrf_render_host.hpp), one 256-byte block cleared by the time-branch launch

constexpr int KEEP_ROUNDS = 8;   // samples per thread of k_keep: a workgroup owns 2048 consecutive samples, appends once per list

struct KeepArgs {
  const float* xyz;       // [N * S][3]
  const float* ts;        // [N]
  const uint8_t* valid;   // [N * S] of the sampler
  int ns, S;
  MaskDev ms, md;         // bits == nullptr: the field keeps every valid sample
  uint8_t *valid_s, *valid_d;
  int *list_s, *list_d;
  int* ctr;               // CTR_KEPT_S / CTR_KEPT_D
  float *sigma_s, *sigma_d, *blending;
};

__global__ __launch_bounds__(256) void k_keep(KeepArgs a) {
  __shared__ int s_cnt[16];
  const int i0 = blockIdx.x * (256 * KEEP_ROUNDS) + threadIdx.x;
  unsigned ks = 0, kd = 0;   // bit r: the thread's sample of round r is kept
  int cnt_s = 0, cnt_d = 0;  // wave-uniform
#pragma unroll 1
  for (int r = 0; r < KEEP_ROUNDS; ++r) {
    const int i = i0 + r * 256;
    const bool act = i < a.ns;
    bool keep_s = false, keep_d = false;
    if (act && a.valid[i] != 0) {
      keep_s = keep_d = true;
      if (a.ms.bits != nullptr || a.md.bits != nullptr) {
        const float x = a.xyz[(size_t)i * 3 + 0], y = a.xyz[(size_t)i * 3 + 1], z = a.xyz[(size_t)i * 3 + 2];
        const float tt = a.ts[i / a.S];
        if (a.ms.bits != nullptr) keep_s = mask_sample(a.ms, x, y, z, mask_slice(a.ms, tt)) > 0.0f;
        if (a.md.bits != nullptr) keep_d = mask_sample(a.md, x, y, z, mask_slice(a.md, tt)) > 0.0f;
      }
    }
    if (act) {
      a.valid_s[i] = keep_s ? 1 : 0;
      a.valid_d[i] = keep_d ? 1 : 0;
      if (!keep_s) a.sigma_s[i] = 0.0f;
      if (!keep_d) {
        a.sigma_d[i] = 0.0f;
        a.blending[i] = 0.0f;
      }
    }
    ks |= (keep_s ? 1u : 0u) << r;
    kd |= (keep_d ? 1u : 0u) << r;
    cnt_s += __popcll(__ballot(keep_s));
    cnt_d += __popcll(__ballot(keep_d));
  }
  int base_s = block_append_base(a.ctr + CTR_KEPT_S, cnt_s, s_cnt, threadIdx.x, blockDim.x);
  int base_d = block_append_base(a.ctr + CTR_KEPT_D, cnt_d, s_cnt, threadIdx.x, blockDim.x);
#pragma unroll 1
  for (int r = 0; r < KEEP_ROUNDS; ++r) {
    const int i = i0 + r * 256;
    const bool m_s = ((ks >> r) & 1u) != 0, m_d = ((kd >> r) & 1u) != 0;
    const unsigned long long bs = __ballot(m_s), bd = __ballot(m_d);
    if (m_s) a.list_s[base_s + ballot_rank(bs)] = i;
    if (m_d) a.list_d[base_d + ballot_rank(bd)] = i;
    base_s += __popcll(bs);
    base_d += __popcll(bd);
  }
}

// the static field's sigma of the listed samples: a lane per entry, static_density_feature as in static_density_body.  Also hands the two
// list lengths to the caller (`kept`, nullable)
__global__ __launch_bounds__(256) void k_static_density_list(FieldArgs a, StaticW w, const int* __restrict__ klist,
                                                             const int* __restrict__ ctr, long long* __restrict__ kept) {
  if (kept != nullptr && blockIdx.x == 0 && threadIdx.x < 2) kept[threadIdx.x] = ctr[threadIdx.x == 0 ? CTR_KEPT_S : CTR_KEPT_D];
  const int count = ctr[CTR_KEPT_S];
  for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < count; li += gridDim.x * blockDim.x) {
    const int idx = klist[li];
    const float f = static_density_feature(w.density, norm_c(a.xyz[idx * 3 + 0], a.box.lo[0], a.box.inv[0]),
                                           norm_c(a.xyz[idx * 3 + 1], a.box.lo[1], a.box.inv[1]),
                                           norm_c(a.xyz[idx * 3 + 2], a.box.lo[2], a.box.inv[2]));
    a.sigma[idx] = density_act(f, a.act, a.density_shift);
  }
}

// the per-ray half of static_density_body over stored sigmas: a wave per ray, 64 samples per round -- its weight_round<64>
// (ray_scan_body scans 32 wide: other roundings), so weight, dists and the app mask come out as the dense kernel's
__global__ __launch_bounds__(256) void k_static_scan(FieldArgs a) {
  __shared__ int s_cnt[16];
  const int lane = threadIdx.x & 63;
  const int wave_ = threadIdx.x >> 6, nwaves_ = blockDim.x >> 6;
  for (int nb = blockIdx.x * nwaves_; nb < a.N; nb += gridDim.x * nwaves_) {   // uniform over the workgroup (block_append_base syncs)
    const bool ray = nb + wave_ < a.N;
    const int n = ray ? nb + wave_ : 0;
    float vx, vy, vz;
    const float nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
    float carry = 1.0f;
    int cnt = 0;
    for (int j0 = 0; j0 < a.S; j0 += 64) {
      const int j = j0 + lane;
      const bool act = ray && j < a.S;
      const int idx = n * a.S + (act ? j : 0);
      if (ray && a.rgb != nullptr) zero_rgb_round<64>(a.rgb, n, a.S, j0, lane);   // (nullable, as in static_density_body)
      const float sigma = act ? a.sigma[idx] : 0.0f;
      float ds;
      const float wt = weight_round<64>(a, sigma, act, idx, j, lane, nrm, carry, ds);
      if (act) {
        a.weight[idx] = wt;
        a.dists[idx] = ds;
      }
      cnt += __popcll(__ballot(act && wt > a.weight_thres));
    }
    const int base = block_append_base(a.counter, cnt, s_cnt, threadIdx.x, blockDim.x);
    if (cnt) append_masked<64>(a, base, n, ray, lane);
  }
}

// 32-entry tiles of the kept list from the workgroup's queue: per tile the inference path of dyn_density_body<., ., ., FLAT>
// (the same per-sample functions in the same order, no saved rows), every entry a valid sample
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_dyn_density_list(FieldArgs a, DynW w, const int* __restrict__ klist,
                                                                    const int* __restrict__ kcount) {
  __shared__ __attribute__((aligned(16))) float lds[pk::K1_SIZE];
  __shared__ int s_next;
  const int count = *kcount;
  const int ntiles = (count + 31) >> 5;
  if ((int)blockIdx.x >= ntiles) return;   // (uniform over the workgroup) nothing of the list is this workgroup's: no LDS fill
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  if (threadIdx.x == 0) s_next = nwaves;
  lds_fill(lds, a.pk + pk::REG_K1, pk::K1_SIZE);
  const float* pkw = lds;
  const bool dynq = (a.dynq & 1) != 0;
  for (int k = wave, tile; (tile = blockIdx.x + k * gridDim.x) < ntiles; k = tile_queue_next(&s_next, k, nwaves, dynq)) {
    const int li = tile * 32 + s;
    const bool act = li < count;
    const int idx = act ? klist[li] : 0;
    const int ti = idx / a.S;
    const float t = a.ts[ti];
    float T[16];
    float X1[8];
    load_tout(T, a.tout, (size_t)ti, h);
    fill_x1(X1, t, h);
    const float px[3] = {a.xyz[idx * 3 + 0], a.xyz[idx * 3 + 1], a.xyz[idx * 3 + 2]};
    float xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xn[c] = norm_c(px[c], a.box.lo[c], a.box.inv[c]);
    float X0[32];
    fill_x0(X0, xn[0], xn[1], xn[2], t, h);
    float d[3], xw[3];
    warp_mlp(d, X0, T, pkw, w.l5b, nullptr, s, h, lane);
    warp_point(xw, xn, d, a.box);
    if (act && h == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.xyz_prime[(size_t)idx * 3 + c] = px[c] + d[c];
#pragma unroll
      for (int c = 0; c < 3; ++c) a.xw[(size_t)idx * 3 + c] = xw[c];
    }
    const float fd = head_raw<false>(w, xw, act, X0, X1, pkw, nullptr, s, h, lane);
    const float fb = head_raw<true>(w, xw, act, X0, X1, pkw, nullptr, s, h, lane);
    if (act && h == 0) {
      a.sigma[idx] = density_act(fd, a.act, a.density_shift);
      a.blending[idx] = sigmoidf_(fb);
    }
  }
}

// the phases after the density kernels: the bodies of the unmasked render in kernels of this unit
__global__ __launch_bounds__(256) void k_masked_time_branch(const float* __restrict__ ts, DynW w, int N, float* __restrict__ tout,
                                                            int* __restrict__ zero64) {
  __shared__ float s_h[8 * 64];
  if (blockIdx.x == 0 && threadIdx.x < 64) zero64[threadIdx.x] = 0;   // the call's four counters
  time_branch_body(ts, w, N, tout, s_h, grid_ctx());
}
__global__ __launch_bounds__(512) void k_masked_ray_scan(FieldArgs a) { ray_scan_body(a); }   // 16 rays per workgroup
template <int HEAD>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_masked_static_app(FieldArgs a, StaticW w) {
  static_app_body<HEAD, false, false>(a, w, nullptr, grid_ctx());
}
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_masked_dyn_app(FieldArgs a, DynW w) {
  dyn_app_body<false, false>(a, w, nullptr, grid_ctx());
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// the launchers of the list-driven density phase (rdrf_render_host.hpp): the masked render below and the per-slot visibility
// of a point track (rdrf_track_vis.hip) issue them
int launch_list_time_branch(const float* ts, const DynW& wdy, int N, float* tout, int* ctr, hipStream_t stream) {
  RDRF_LAUNCH("time_branch", k_masked_time_branch, dim3((N + 7) / 8), dim3(256), stream, ts, wdy, N, tout, ctr);
  return 0;
}
int launch_static_density_list(const FieldArgs& as, const StaticW& wst, const int* list_s, const int* ctr, long long* kept,
                               hipStream_t stream) {
  const int blocks = (as.N * as.S + 255) / 256;
  RDRF_LAUNCH("static_density_list", k_static_density_list, dim3(blocks > 4096 ? 4096 : blocks), dim3(256), stream, as, wst,
              list_s, ctr, kept);
  return 0;
}
int launch_static_scan(const FieldArgs& as, hipStream_t stream) {
  RDRF_LAUNCH("static_scan", k_static_scan, dim3((as.N + 3) / 4), dim3(256), stream, as);   // 4 rays per workgroup: one list append
  return 0;
}
int launch_dyn_density_list(const FieldArgs& ad, const DynW& wdy, const int* list_d, const int* count, hipStream_t stream) {
  const Geo g3 = geo_for_tiles(ad.N, ad.S);
  RDRF_LAUNCH("dyn_density_list", k_dyn_density_list, dim3(g3.grid), dim3(g3.block), stream, ad, wdy, list_d, count);
  return 0;
}

struct MaskedBufs {
  void* render;   // the unmasked render's workspace (carve_render)
  size_t render_bytes;
  uint8_t *valid_s, *valid_d;
  int *list_s, *list_d;
  int* ctr;
};
static void carve_masked(MaskedBufs& b, WsCarver& c, int N, int S) {
  const size_t ns = (size_t)N * S;
  b.render_bytes = rdrf_render_workspace_bytes(N, S);
  b.render = c.take<char>(b.render_bytes);
  b.valid_s = c.take<uint8_t>(ns);
  b.valid_d = c.take<uint8_t>(ns);
  b.list_s = c.take<int>(ns);
  b.list_d = c.take<int>(ns);
  b.ctr = c.take<int>(64);
}
extern "C" size_t rdrf_render_masked_ws_bytes(int N, int S) {
  MaskedBufs b;
  WsCarver c;
  carve_masked(b, c, N < 0 ? 0 : N, S < 0 ? 0 : S);
  return c.off;
}

extern "C" int rdrf_render_masked_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                      const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near,
                                      float far, float step, const RdrfAlphaMask* mask_s, const RdrfAlphaMask* mask_d,
                                      const RdrfRenderMaps* maps, int64_t* kept, void* ws, size_t ws_bytes,
                                      rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RenderCall call = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, step, {}, ws, ws_bytes};
  maps_to_slots(call.want, maps);
  RDRF_CHECK(ws != nullptr, -1, "render_masked: bad arguments");
  RDRF_TRY(render_check_args(call, "render_masked", "step > 0 exactly for the world-space march"));
  const bool has_s = mask_s != nullptr && mask_s->bits != nullptr, has_d = mask_d != nullptr && mask_d->bits != nullptr;
  RDRF_CHECK(has_s || has_d, -1, "render_masked: at least one of the two masks must be given");
  RDRF_CHECK(mask_ok(mask_s) && mask_ok(mask_d), -1, "render_masked: the masks' grids and slice counts must be positive");
  RDRF_TRY(render_check_fields(call, "render_masked"));
  MaskedBufs m;
  WsCarver c(ws, ws_bytes);
  carve_masked(m, c, N, S);
  RDRF_CHECK(c.ok(), -3, "render_masked: workspace too small: need %zu have %zu", c.off, ws_bytes);
  RenderBufs b;
  RDRF_TRY(carve_render(b, m.render, m.render_bytes, N, S, call.want));
  const int ns = N * S;

  // each field reads its own mask's valid plane and counts its appearance list in this call's counter block
  FieldArgs as, ad;
  StaticW wst;
  DynW wdy;
  RDRF_TRY(render_fields(call, b, m.valid_s, m.valid_d, as, ad, wst, wdy, stream));
  as.counter = m.ctr + CTR_APP_S;
  as.dynq = fwd_dynq();
  ad.counter = m.ctr + CTR_APP_D;
  ad.dynq = fwd_dynq();

  RDRF_TRY(render_sample(call, b, stream));
  // the time branch of every ray (a masked-out ray costs 17 -> 64 -> 30 once); clears the four counters on its way
  RDRF_TRY(launch_list_time_branch(ts, wdy, N, ad.tout, m.ctr, stream));

  KeepArgs k;
  memset(&k, 0, sizeof(k));
  k.xyz = b.xyz; k.ts = ts; k.valid = b.valid; k.ns = ns; k.S = S;
  k.ms = make_mask(mask_s); k.md = make_mask(mask_d);
  k.valid_s = m.valid_s; k.valid_d = m.valid_d; k.list_s = m.list_s; k.list_d = m.list_d; k.ctr = m.ctr;
  k.sigma_s = b.sigma_s; k.sigma_d = b.sigma_d; k.blending = b.blending;
  RDRF_LAUNCH("mask_keep", k_keep, dim3((ns + 256 * KEEP_ROUNDS - 1) / (256 * KEEP_ROUNDS)), dim3(256), stream, k);

  RDRF_TRY(launch_static_density_list(as, wst, m.list_s, m.ctr, (long long*)kept, stream));
  RDRF_TRY(launch_static_scan(as, stream));
  const Geo g3 = geo_for_tiles(N, S);
  RDRF_TRY(launch_dyn_density_list(ad, wdy, m.list_d, m.ctr + CTR_KEPT_D, stream));
  RDRF_LAUNCH("ray_scan", k_masked_ray_scan, dim3((N + 15) / 16), dim3(512), stream, ad);
  if (cfg_s->static_head == RDRF_HEAD_MLP_FEA)
    RDRF_LAUNCH("static_app", k_masked_static_app<RDRF_HEAD_MLP_FEA>, dim3(g3.grid), dim3(g3.block), stream, as, wst);
  else
    RDRF_LAUNCH("static_app", k_masked_static_app<RDRF_HEAD_MLP_FEA_TIMEEMBEDDING>, dim3(g3.grid), dim3(g3.block), stream, as, wst);
  RDRF_LAUNCH("dyn_app", k_masked_dyn_app, dim3(g3.grid), dim3(g3.block), stream, ad, wdy);
  return rdrf_composite_fwd(b.rgb_s, b.sigma_s, b.rgb_d, b.sigma_d, b.dists_d, b.blending, b.z, rays, N, S, cfg_d->ray_type, 0,
                            nullptr, b.out, stream);
}
