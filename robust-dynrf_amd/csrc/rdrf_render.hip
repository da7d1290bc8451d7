// rdrf_render.hip -- no-grad render of a ray chunk in one launch sequence (the loop body of
// the reference's renderer.py:740-812: sampleXYZ -> static -> dynamic -> raw2outputs), and the host steps the render
// units share (rdrf_render_host.hpp).
#include "rdrf_misc_dev.hpp"
#include "rdrf_render_host.hpp"

// ------------------------------------------------------------------------------------------------
// FUSED render: sample -> static + dynamic density phases -> static + dynamic appearance phases -> compositor in ONE
// cooperative launch (/root/reference/renderer.py:740-812 loop body).  The persistent workgroups (one per CU, 8
// waves) walk the phases of the per-phase kernels -- the same device bodies (rdrf_fwd_dev.hpp, rdrf_misc_dev.hpp),
// so the results are those of the launch sequence bit for bit -- separated by grid-wide barriers; the LDS is
// re-filled with the weight image of each MLP phase (121 / 159 / 153 KB: they cannot be resident together).  What
// it buys is the launch sequence itself: 11 stream operations -> 2, which is what a 512-ray chunk (the reference's
// eval chunk, renderer.py:732) spends most of its time on; the per-sample intermediates stay in the L2 / MALL.
// ------------------------------------------------------------------------------------------------
struct RenderFusedArgs {
  FieldArgs as, ad;      // static / dynamic field (outputs + workspaces in the caller's scratch)
  StaticW ws;
  DynW wd;
  CompArgs comp;
  float near, far;
  float step;            // world-space march (RDRF_RAY_OTHER): the field's stepSize
  unsigned* barrier;     // zero at launch
};

// grid-wide barrier of the cooperative launch (all workgroups are resident): a monotonically increasing arrival
// counter; agent-scope fences publish this workgroup's writes (other XCDs have their own L2) and invalidate stale
// lines before the next phase reads what other workgroups wrote.  A bounded spin: a lost workgroup cannot hang the GPU;
// a barrier that times out raises the error word bar[1], every workgroup then leaves at its next barrier and the
// compositor phase is replaced by NaN outputs -- a stalled launch gives a loudly wrong image, never a plausible one.
// Returns false when the launch has failed.
RDRF_D bool grid_barrier(unsigned* bar, unsigned nblk, unsigned& epoch) {
  __syncthreads();
  epoch += 1;
  __shared__ unsigned failed_s;
  if (threadIdx.x == 0) {
    __threadfence();
    atomicAdd(bar, 1u);
    const unsigned target = epoch * nblk;
    unsigned spins = 0;
    while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(4);
      if (++spins > (1u << 26) || __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
        atomicExch(bar + 1, 1u);
        break;
      }
    }
    __threadfence();
    failed_s = __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return failed_s == 0u;
}

template <int HEAD>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_render_fused(RenderFusedArgs r) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GridCtx gc = grid_ctx();
  unsigned epoch = 0;
  const int N = r.as.N, S = r.as.S;
  // ---- phase 0: sample points, per-ray time branch, clear the per-sample rgb (0 off the appearance masks) and the
  // compaction counters
  if (r.ad.ray_type == RDRF_RAY_NDC)
    sample_ndc_body(r.as.rays, N, S, r.near, r.far, nullptr, r.ad.box, (float*)r.as.xyz, (float*)r.as.z, (uint8_t*)r.as.valid, gc);
  else if (r.ad.ray_type == RDRF_RAY_CONTRACT)
    sample_contract_body(r.as.rays, N, S, r.near, r.far, nullptr, nullptr, (float*)r.as.xyz, (float*)r.as.z,
                         (uint8_t*)r.as.valid, gc);
  else
    sample_world_body(r.as.rays, N, S, r.near, r.far, r.step, nullptr, r.ad.box, (float*)r.as.xyz, (float*)r.as.z,
                      (uint8_t*)r.as.valid, gc);
  time_branch_body<true>(r.ad.ts, r.wd, N, r.ad.tout, lds, gc);
  {
    const size_t n3 = (size_t)N * S * 3;
    for (size_t i = (size_t)gc.bid * gc.nthr + gc.tid; i < n3; i += (size_t)gc.nblk * gc.nthr) {
      r.as.rgb[i] = 0.f;
      r.ad.rgb[i] = 0.f;
    }
    if (gc.bid == 0 && gc.tid == 0) { *r.as.counter = 0; *r.ad.counter = 0; }
  }
  bool ok = grid_barrier(r.barrier, gc.nblk, epoch);
  // ---- phase 1: density of both fields (weights, compaction of the appearance masks)
  static_density_body<false, true>(r.as, r.ws, gc);
  dyn_density_body<false, false, true>(r.ad, r.wd, lds, gc);
  ok = grid_barrier(r.barrier, gc.nblk, epoch) && ok;
  // ---- phase 2: appearance of both fields over the compacted lists
  static_app_body<HEAD, false, false, true>(r.as, r.ws, lds, gc);
  __syncthreads();
  dyn_app_body<false, false, true>(r.ad, r.wd, lds, gc);
  ok = grid_barrier(r.barrier, gc.nblk, epoch) && ok;
  // ---- phase 3: raw2outputs per ray
  if (ok) {
    composite_body(r.comp, gc);
  } else {   // a barrier timed out: the phases ran on partial data -- poison this workgroup's share of every per-ray
    // output (the caller's maps and the workspace's alike; the per-sample weight planes 3, 7, 11 are no maps)
    const float nan = __int_as_float(0x7fc00000);
    for (int i = gc.bid * gc.nthr + gc.tid; i < N; i += gc.nblk * gc.nthr) {
#pragma unroll
      for (int m = 0; m < 13; ++m) {
        if (m == 3 || m == 7 || m == 11) continue;
        const int w = (m % 4 == 0 && m < 12) ? 3 : 1;
        for (int c = 0; c < w; ++c) r.comp.out[m][i * w + c] = nan;
      }
    }
  }
}

extern "C" size_t rdrf_render_workspace_bytes(int N, int S) {
  const size_t ns = (size_t)N * S;
  // xyz, xyz_prime, rgb_s, rgb_d (3 floats) + 12 scalar planes + valid + 13 outputs + both fields' workspaces
  return ns * 4 * (3 * 4 + 12) + ns + (size_t)N * 4 * 16 + 2 * rdrf_forward_workspace_bytes(N, S) + (1 << 14);
}

// the per-ray outputs among the compositor's 13 (out13 order of rdrf_composite_fwd) and their widths; the three per-sample
// weight planes (3, 7, 11) always stay in the workspace
static const int kMapSlot[10] = {0, 1, 2, 4, 5, 6, 8, 9, 10, 12};
static inline int map_width(int slot) { return (slot % 4 == 0 && slot < 12) ? 3 : 1; }
void maps_to_slots(float* out[13], const RdrfRenderMaps* m) {
  for (int i = 0; i < 13; ++i) out[i] = nullptr;
  if (!m) return;
  float* const p[10] = {m->rgb, m->depth, m->acc, m->rgb_s, m->depth_s, m->acc_s, m->rgb_d, m->depth_d, m->acc_d, m->blending};
  for (int i = 0; i < 10; ++i) out[kMapSlot[i]] = p[i];
}

int want_rgb_depth(float* want[13], float* rgb_map, float* depth_map, const char* who) {
  RDRF_CHECK(rgb_map && depth_map, -1, "%s: bad arguments", who);
  maps_to_slots(want, nullptr);
  want[0] = rgb_map;
  want[1] = depth_map;
  return 0;
}

int carve_render(RenderBufs& b, void* ws, size_t ws_bytes, int N, int S, float* const want[13]) {
  WsCarver c(ws, ws_bytes);
  const size_t ns = (size_t)N * S;
  b.xyz = c.take<float>(ns * 3);
  b.z = c.take<float>(ns);
  b.valid = c.take<uint8_t>(ns);
  b.rgb_s = c.take<float>(ns * 3);
  b.sigma_s = c.take<float>(ns);
  b.weight_s = c.take<float>(ns);
  b.dists_s = c.take<float>(ns);
  b.rgb_d = c.take<float>(ns * 3);
  b.sigma_d = c.take<float>(ns);
  b.weight_d = c.take<float>(ns);
  b.dists_d = c.take<float>(ns);
  b.blending = c.take<float>(ns);
  b.xyz_prime = c.take<float>(ns * 3);
  const size_t osz[13] = {(size_t)N * 3, (size_t)N, (size_t)N, ns, (size_t)N * 3, (size_t)N, (size_t)N, ns, (size_t)N * 3,
                          (size_t)N, (size_t)N, ns, (size_t)N};
  for (int i = 0; i < 13; ++i) b.out[i] = want[i] ? want[i] : c.take<float>(osz[i]);
  b.barrier = c.take<unsigned>(64);
  b.fws_s = c.take<char>(rdrf_forward_workspace_bytes(N, S));
  b.fws_d = c.take<char>(rdrf_forward_workspace_bytes(N, S));
  RDRF_CHECK(c.ok(), -3, "render: workspace too small: need %zu have %zu", c.off, ws_bytes);
  return 0;
}

int render_check_args(const RenderCall& c, const char* who, const char* step_rule) {
  RDRF_CHECK(c.PS && c.PD && c.cfg_s && c.cfg_d && c.rays && c.ts && c.N > 0 && c.S > 0, -1, "%s: bad arguments", who);
  const int ray_type = c.cfg_d->ray_type;
  RDRF_CHECK((ray_type == RDRF_RAY_NDC || ray_type == RDRF_RAY_CONTRACT) == !(c.step > 0.0f), -1, "%s: %s (ray_type %d, step %g)",
             who, step_rule, ray_type, (double)c.step);
  RDRF_CHECK((size_t)c.N * c.S * 3 < (size_t)INT32_MAX, -1, "%s: N * S * 3 must stay below 2^31: render in chunks", who);
  return 0;
}
int render_check_fields(const RenderCall& c, const char* who) {
  const RdrfStaticParams* PS = c.PS;
  const RdrfDynamicParams* PD = c.PD;
  RDRF_CHECK(vm_ok(PS->density, 16, 4) && vm_ok(PS->app, 48, 12) && vm_ok(PD->density, 16, 4) && vm_ok(PD->blending, 16, 4) &&
             vm_ok(PD->app, 48, 12) && vm_same_grid(PD->density, PD->blending), -1,
             "%s: only density comps {16,4,4} / app comps {48,12,12} of one grid are built", who);
  return 0;
}
// the checks of this unit's runners and the carve behind them
static int render_begin(const RenderCall& c, RenderBufs& b) {
  // `step` > 0 comes from rdrf_render_world_fwd alone: the world march needs it, the other two samplers have no use for it
  RDRF_TRY(render_check_args(c, "render", "ray_type ndc / contract through rdrf_render_*_fwd, any other through "
                                          "rdrf_render_world_fwd with step > 0"));
  RDRF_CHECK(c.ws_bytes >= rdrf_render_workspace_bytes(c.N, c.S), -3, "render: workspace too small");
  RDRF_TRY(render_check_fields(c, "render"));
  return carve_render(b, c.ws, c.ws_bytes, c.N, c.S, c.want);
}

int render_sample(const RenderCall& c, const RenderBufs& b, rdrf_stream_t stream) {
  const RdrfFieldCfg* cfg = c.cfg_d;
  if (cfg->ray_type == RDRF_RAY_NDC)
    return rdrf_sample_ndc(c.rays, c.N, c.S, c.near, c.far, nullptr, cfg->aabb, b.xyz, b.z, b.valid, stream);
  if (cfg->ray_type == RDRF_RAY_CONTRACT)
    return rdrf_sample_contract(c.rays, c.N, c.S, c.near, c.far, nullptr, nullptr, b.xyz, b.z, b.valid, stream);
  return rdrf_sample_world(c.rays, c.N, c.S, c.near, c.far, c.step, nullptr, cfg->aabb, b.xyz, b.z, b.valid, stream);
}

int render_fields(const RenderCall& c, const RenderBufs& b, const uint8_t* valid_s, const uint8_t* valid_d, FieldArgs& as,
                  FieldArgs& ad, StaticW& wst, DynW& wdy, hipStream_t stream) {
  const int N = c.N, S = c.S;
  const size_t fwb = rdrf_forward_workspace_bytes(N, S);
  fill_common(as, c.cfg_s, c.rays, c.ts, b.xyz, b.z, valid_s, N, S);
  as.rgb = b.rgb_s; as.sigma = b.sigma_s; as.weight = b.weight_s; as.dists = b.dists_s;
  RDRF_TRY(ws_carve_fwd(as, b.fws_s, fwb, N, S, nullptr, 0, 0));
  fill_common(ad, c.cfg_d, c.rays, c.ts, b.xyz, b.z, valid_d, N, S);
  ad.rgb = b.rgb_d; ad.sigma = b.sigma_d; ad.weight = b.weight_d; ad.dists = b.dists_d;
  ad.blending = b.blending; ad.xyz_prime = b.xyz_prime;
  RDRF_TRY(ws_carve_fwd(ad, b.fws_d, fwb, N, S, nullptr, 0, 1));
  fill_static_w(wst, c.PS);
  fill_dyn_w(wdy, c.PD);
  RDRF_TRY(pack_image(as.pk, c.PS->packed_fwd, (float*)as.pk, stream, static_pack_jobs_fwd, c.PS, c.cfg_s->static_head));
  RDRF_TRY(pack_image(ad.pk, c.PD->packed_fwd, (float*)ad.pk, stream, dyn_pack_jobs_fwd, c.PD));
  return 0;
}

/* one cooperative launch (see k_render_fused) */
static int render_fused(const RenderCall& c, RenderBufs& b, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_TRY(render_begin(c, b));
  const int N = c.N, S = c.S;
  RenderFusedArgs r;
  memset(&r, 0, sizeof(r));
  RDRF_TRY(render_fields(c, b, b.valid, b.valid, r.as, r.ad, r.ws, r.wd, stream));
  r.comp.rgb_s = b.rgb_s; r.comp.sigma_s = b.sigma_s; r.comp.rgb_d = b.rgb_d; r.comp.sigma_d = b.sigma_d;
  r.comp.dists = b.dists_d; r.comp.blending = b.blending; r.comp.z = b.z; r.comp.rays = c.rays;
  r.comp.N = N; r.comp.S = S; r.comp.ray_type = c.cfg_d->ray_type; r.comp.add_white_bg = 0; r.comp.white_dev = nullptr;
  for (int i = 0; i < 13; ++i) r.comp.out[i] = b.out[i];
  r.near = c.near; r.far = c.far; r.step = c.step; r.barrier = b.barrier;
  RDRF_FILL(b.barrier, 0, 256, stream);
  // one workgroup per CU at most (its LDS holds a whole weight image); fewer when the chunk has fewer units of work
  const long tiles = ((long)N * S + 31) / 32;
  const long units = tiles > N ? tiles : N;
  int ncu = 0;
  RDRF_TRY(current_cu_count(&ncu));
  long g = (units + RDRF_MAXW - 1) / RDRF_MAXW;
  g = g < 1 ? 1 : (g > ncu ? ncu : g);
  const size_t lds_bytes = (size_t)(pk::S3_SIZE > pk::K3_SIZE ? (pk::S3_SIZE > pk::K1_SIZE ? pk::S3_SIZE : pk::K1_SIZE)
                                                            : (pk::K3_SIZE > pk::K1_SIZE ? pk::K3_SIZE : pk::K1_SIZE)) * 4;
  const void* kern = c.cfg_s->static_head == RDRF_HEAD_MLP_FEA ? (const void*)k_render_fused<RDRF_HEAD_MLP_FEA>
                                                            : (const void*)k_render_fused<RDRF_HEAD_MLP_FEA_TIMEEMBEDDING>;
  RDRF_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  void* kargs[] = {(void*)&r};
  rdrf_prof_begin("render_fused", stream);
  hipError_t e = hipLaunchCooperativeKernel(kern, dim3((unsigned)g), dim3(64 * RDRF_MAXW), kargs, (unsigned)lds_bytes, stream);
  rdrf_prof_end("render_fused", stream);
  RDRF_CHECK(e == hipSuccess, -5, "render_fused: cooperative launch failed: %s", hipGetErrorString(e));
  return 0;
}

/* launch sequence of the per-phase kernels (whole frames: every kernel fills the chip, nothing to gain from fusion) */
static int render_sequence(const RenderCall& c, RenderBufs& b, rdrf_stream_t stream) {
  RDRF_TRY(render_begin(c, b));
  RDRF_TRY(render_sample(c, b, stream));
  // (a side stream for the static density phase under the dynamic field's density kernel does not overlap: the MLP kernels
  // hold all 512 VGPRs of every SIMD, so no other wave becomes resident; measured)
  const int N = c.N, S = c.S;
  const size_t fwb = rdrf_forward_workspace_bytes(N, S);
  RDRF_TRY(rdrf_static_fwd(c.PS, c.cfg_s, c.rays, c.ts, b.xyz, b.z, b.valid, N, S, b.rgb_s, b.sigma_s, b.weight_s, b.dists_s,
                           nullptr, 0, b.fws_s, fwb, stream));
  RDRF_TRY(rdrf_dynamic_fwd(c.PD, c.cfg_d, c.rays, c.ts, b.xyz, b.z, b.valid, N, S, b.blending, b.weight_d, b.xyz_prime,
                            b.rgb_d, b.sigma_d, b.dists_d, nullptr, 0, b.fws_d, fwb, stream));
  return rdrf_composite_fwd(b.rgb_s, b.sigma_s, b.rgb_d, b.sigma_d, b.dists_d, b.blending, b.z, c.rays, N, S,
                            c.cfg_d->ray_type, 0, nullptr, b.out, stream);
}

int render_run(const RenderCall& c, int mode, const char* who, RenderBufs& b, rdrf_stream_t stream) {
  RDRF_CHECK(mode == RDRF_RENDER_AUTO || mode == RDRF_RENDER_SEQUENCE || mode == RDRF_RENDER_FUSED, -1, "%s: unknown mode %d",
             who, mode);
  return mode == RDRF_RENDER_FUSED ? render_fused(c, b, stream) : render_sequence(c, b, stream);
}

extern "C" int rdrf_render_fused_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                     const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near,
                                     float far, float* rgb_map, float* depth_map, void* ws, size_t ws_bytes,
                                     rdrf_stream_t stream) {
  if (N == 0) return 0;
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, 0.f, {}, ws, ws_bytes};
  RDRF_TRY(want_rgb_depth(c.want, rgb_map, depth_map, "render"));
  RenderBufs b;
  return render_fused(c, b, stream);
}
extern "C" int rdrf_render_sequence_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                           const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near,
                           float far, float* rgb_map, float* depth_map, void* ws, size_t ws_bytes, rdrf_stream_t stream) {
  if (N == 0) return 0;
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, 0.f, {}, ws, ws_bytes};
  RDRF_TRY(want_rgb_depth(c.want, rgb_map, depth_map, "render"));
  RenderBufs b;
  return render_sequence(c, b, stream);
}

// Measured on MI355X (tools/render_bench.py, Balloon1 stage-0 shape, 240 x 135 frame): whole frame 7.7 ms either way (the
// kernels ARE the frame time: their HIP-event sum is 7.9 ms); 512-ray chunks 274 us per chunk as a launch sequence -- the
// seven kernels run back to back, their event times add up to 282 us -- against 378 us for the single cooperative launch
// (static density at 2 waves per SIMD instead of 6, three serial LDS fills, barrier round trips).  What makes small chunks
// slow is not the launch sequence but the wave-per-ray density phase: 512 rays = 512 busy waves of 2048.  The launch
// sequence is what rdrf_render_fwd runs at every size; rdrf_render_fused_fwd is the explicit entry point of the single launch.
extern "C" int rdrf_render_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s,
                               const RdrfDynamicParams* PD, const RdrfFieldCfg* cfg_d, const float* rays,
                               const float* ts, int N, int S, float near, float far, float* rgb_map,
                               float* depth_map, void* ws, size_t ws_bytes, rdrf_stream_t stream) {
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  return rdrf_render_sequence_fwd(PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, rgb_map, depth_map, ws, ws_bytes, stream);
}

// The decomposed maps (renderer.py:745-826 keeps rgb / depth of the full, static and dynamic renders and the blending map
// of every frame): the same launches, the caller's buffers replace the workspace slices of the requested outputs.
extern "C" int rdrf_render_maps_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                    const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, float near,
                                    float far, int mode, const RdrfRenderMaps* maps, void* ws, size_t ws_bytes,
                                    rdrf_stream_t stream) {
  if (N == 0) return 0;
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, 0.f, {}, ws, ws_bytes};
  maps_to_slots(c.want, maps);
  RenderBufs b;
  return render_run(c, mode, "render_maps", b, stream);
}

// ------------------------------------------------------------------------------------------------
// The reference's eval loop (renderer.py:740-812: `for chunk_idx in range(N_rays_all // chunk + ...)`, chunk = 512,
// renderer.py:732) as ONE native call: the chunks' launch sequences are issued round-robin on `nstreams` caller streams.
// Why native: issued from Python, one chunk costs ~250 us of host time (struct marshalling + 10 launches) against
// ~190 us of GPU time -- the loop is host-bound; from here a chunk costs its launches.  Why streams: one 512-ray chunk
// fills 64-110 of the 256 CUs (the MLP kernels hold one workgroup per CU: 121-159 KB of LDS), the chunks are
// independent, so several run side by side.  Both packed weight images must be supplied (packed_fwd: they are shared,
// read-only, by every stream); `ws` is cut into one slice of rdrf_render_workspace_bytes(chunk, S) per stream.
// Ordering: every stream first waits for `main_stream` (inputs, weights), `main_stream` finally waits for every stream.
// ------------------------------------------------------------------------------------------------
extern "C" size_t rdrf_render_chunks_workspace_bytes(int chunk, int S, int nstreams) {
  return (size_t)(nstreams < 1 ? 1 : nstreams) * ((rdrf_render_workspace_bytes(chunk, S) + 255) & ~(size_t)255);
}
// the call for the n rays from r0 on, with the scratch it may use
static RenderCall rays_of(const RenderCall& c, int r0, int n, void* ws, size_t ws_bytes) {
  RenderCall p = c;
  p.rays = c.rays + (size_t)r0 * 6;
  p.ts = c.ts + r0;
  p.N = n;
  for (int i = 0; i < 13; ++i) p.want[i] = c.want[i] ? c.want[i] + (size_t)r0 * map_width(i) : nullptr;
  p.ws = ws;
  p.ws_bytes = ws_bytes;
  return p;
}
static int render_chunks(const RenderCall& c, int chunk, rdrf_stream_t main_stream_, const rdrf_stream_t* streams,
                         int nstreams) {
  const int N = c.N, S = c.S;
  void* const ws = c.ws;
  const size_t ws_bytes = c.ws_bytes;
  if (N == 0) return 0;
  RDRF_CHECK(c.PS && c.PD && c.cfg_s && c.cfg_d && c.rays && c.ts && ws && chunk > 0 && S > 0, -1,
             "render_chunks: bad arguments");
  RDRF_CHECK(c.PS->packed_fwd != nullptr && c.PD->packed_fwd != nullptr, -1,
             "render_chunks: both packed weight images are required (rdrf_static_pack / rdrf_dynamic_pack)");
  RDRF_CHECK(nstreams >= 0 && nstreams <= 16 && (nstreams == 0 || streams != nullptr), -1, "render_chunks: 0..16 streams");
  hipStream_t main_stream = (hipStream_t)main_stream_;
#ifdef RDRF_DETERMINISTIC
  // the deterministic build sorts every compaction list through ONE process-wide scratch (rdrf_sort_ints_inplace): chunks
  // on different streams would race on it (and it may be re-allocated under them), so this build runs the loop in order
  // on the caller's stream -- same bits, no concurrency
  nstreams = 0;
#endif
  const int ns = nstreams < 1 ? 1 : nstreams;
  const size_t slice = (rdrf_render_workspace_bytes(chunk < N ? chunk : N, S) + 255) & ~(size_t)255;
  RDRF_CHECK(ws_bytes >= slice * ns, -3, "render_chunks: workspace too small: need %zu have %zu", slice * ns, ws_bytes);
  {
    // Chunk coalescing (round 6).  The workspace the caller sized for `nstreams` concurrent chunks holds ONE launch sequence
    // over that many chunks' rays just as well, and a ray's result does not depend on which other rays share its launch
    // (per-ray scans, per-sample MFMA columns: tests/test_gpu_forward.py compares chunked and whole-batch renders bit for
    // bit).  A group of g chunks pays the fixed costs of a launch sequence once -- ten launches, two 121-159 KB LDS weight
    // images per CU and MLP kernel -- instead of g times: the frame time of the 512-ray loop was the SUM of its chunks'
    // isolated kernel times (profiles/r05_render_chunk512_kernel_stats.csv), streams or not.
    // (the 32-bit sample index bound first: behind it (g + 1) * chunk is an int)
    int g = 1;
    while (g < 256 && (long)g * chunk < N && (size_t)(g + 1) * chunk * S * 3 < (size_t)INT32_MAX &&
           rdrf_render_workspace_bytes((int)((long)(g + 1) * chunk), S) <= ws_bytes)
      ++g;
    if (g > 1) {
      const int super = g * chunk;
      for (int c0 = 0; c0 < N; c0 += super) {
        RenderBufs b;
        RDRF_TRY(render_sequence(rays_of(c, c0, N - c0 < super ? N - c0 : super, ws, ws_bytes), b, main_stream_));
      }
      return 0;
    }
  }
  hipEvent_t ev_start = nullptr, ev_done[16];
  if (nstreams >= 1) {
    RDRF_HIP(hipEventCreateWithFlags(&ev_start, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev_start, main_stream);
    for (int k = 0; k < nstreams && e == hipSuccess; ++k) e = hipStreamWaitEvent((hipStream_t)streams[k], ev_start, 0);
    if (e != hipSuccess) {   // nothing was issued on the side streams yet: release the event and report
      (void)hipEventDestroy(ev_start);
      RDRF_CHECK(false, -5, "render_chunks: fork onto the side streams failed: %s", hipGetErrorString(e));
    }
  }
  int rc = 0, k = 0;
  for (int c0 = 0; c0 < N && rc == 0; c0 += chunk, ++k) {
    const int n = N - c0 < chunk ? N - c0 : chunk;
    const int si = k % ns;
    rdrf_stream_t st = nstreams >= 1 ? streams[si] : main_stream_;
    RenderBufs b;
    rc = render_sequence(rays_of(c, c0, n, (char*)ws + slice * si, slice), b, st);
  }
  if (nstreams >= 1) {   // join (also on error: the streams must not run past the caller's buffers unobserved)
    for (int q = 0; q < nstreams; ++q) {
      if (hipEventCreateWithFlags(&ev_done[q], hipEventDisableTiming) != hipSuccess) { rc = rc ? rc : -5; continue; }
      (void)hipEventRecord(ev_done[q], (hipStream_t)streams[q]);
      (void)hipStreamWaitEvent(main_stream, ev_done[q], 0);
      (void)hipEventDestroy(ev_done[q]);   // released when the recorded work completes
    }
    (void)hipEventDestroy(ev_start);
  }
  return rc;
}
extern "C" int rdrf_render_chunks_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                      const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, int chunk,
                                      float near, float far, float* rgb_map, float* depth_map, void* ws, size_t ws_bytes,
                                      rdrf_stream_t main_stream, const rdrf_stream_t* streams, int nstreams) {
  if (N == 0) return 0;
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, 0.f, {}, ws, ws_bytes};
  RDRF_TRY(want_rgb_depth(c.want, rgb_map, depth_map, "render_chunks"));
  return render_chunks(c, chunk, main_stream, streams, nstreams);
}
extern "C" int rdrf_render_chunks_maps_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                           const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S,
                                           int chunk, float near, float far, const RdrfRenderMaps* maps, void* ws,
                                           size_t ws_bytes, rdrf_stream_t main_stream, const rdrf_stream_t* streams,
                                           int nstreams) {
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, 0.f, {}, ws, ws_bytes};
  maps_to_slots(c.want, maps);
  return render_chunks(c, chunk, main_stream, streams, nstreams);
}

// World-space rays (RDRF_RAY_OTHER): the family above behind one entry point that carries the sampler's `step`.
extern "C" int rdrf_render_world_fwd(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                     const RdrfFieldCfg* cfg_d, const float* rays, const float* ts, int N, int S, int chunk,
                                     float near, float far, float step, int mode, const RdrfRenderMaps* maps, void* ws,
                                     size_t ws_bytes, rdrf_stream_t main_stream, const rdrf_stream_t* streams, int nstreams) {
  if (N == 0) return 0;
  RDRF_CHECK(step > 0.0f, -1, "render_world: step must be positive (the field's stepSize)");
  RenderCall c = {PS, cfg_s, PD, cfg_d, rays, ts, N, S, near, far, step, {}, ws, ws_bytes};
  maps_to_slots(c.want, maps);
  if (chunk > 0) return render_chunks(c, chunk, main_stream, streams, nstreams);
  RenderBufs b;
  return render_run(c, mode, "render_world", b, main_stream);
}
