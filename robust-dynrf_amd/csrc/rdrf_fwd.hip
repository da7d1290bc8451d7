// rdrf_fwd.hip -- forward kernels of the two fields (TensorBase.forward,
// /root/reference/models/tensorBase.py:704-850) for gfx950.
//
//   static  field: k_static_density (wave per ray: VM gather -> sigma -> wave scan -> weight ->
//                  app-mask compaction) ; k_static_app (32-sample MFMA tiles over the compacted
//                  list: VM gather -> basis -> PE -> 138|135->128->128->3 MLP -> sigmoid)
//   dynamic field: k_time_branch (per ray 17->64->30), k_dyn_density (wave per ray, 32-sample
//                  tiles: warp MLP -> 3-stride VM gathers at the warped point -> density and
//                  blending MLPs -> scan -> weight/compaction), k_dyn_app (MFMA tiles over the
//                  compacted list: 216-feature gather -> basis -> 107->128->128->(131)->3)
//   scene flow   : k_scene_flow (36->64->64->64->6, models/tensoRF.py:446-462)
#include "rdrf_fwd_dev.hpp"
#include "rdrf_render_host.hpp"

// ------------------------------------------------------------------------------------------------
// per-phase kernels: thin wrappers over the bodies of rdrf_fwd_dev.hpp
// ------------------------------------------------------------------------------------------------
template <bool FEAT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_static_density(FieldArgs a, StaticW w) { static_density_body<FEAT>(a, w, grid_ctx()); }

template <int HEAD, bool FEAT, bool SAVE = true>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_static_app(FieldArgs a, StaticW w) {
  static_app_body<HEAD, FEAT, SAVE>(a, w, nullptr, grid_ctx());
}

template <bool FEAT, bool SAVE = true>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_dyn_density(FieldArgs a, DynW w) {
  dyn_density_body<FEAT, SAVE>(a, w, nullptr, grid_ctx());
}

template <bool FEAT, bool SAVE = true>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_dyn_app(FieldArgs a, DynW w) {
  dyn_app_body<FEAT, SAVE>(a, w, nullptr, grid_ctx());
}

// `zero64`: 64 ints cleared on the way (the append counter of the density phase that follows on the same stream)
__global__ __launch_bounds__(256) void k_time_branch(const float* __restrict__ ts, DynW w, int N,
                                                     float* __restrict__ tout, int* __restrict__ zero64) {
  __shared__ float s_h[8 * 64];
  if (zero64 != nullptr && blockIdx.x == 0 && threadIdx.x < 64) zero64[threadIdx.x] = 0;
  time_branch_body(ts, w, N, tout, s_h, grid_ctx());
}

// the density phase of the dynamic field at tile granularity + the per-ray scan (rdrf_fwd_dev.hpp); SAVE: training
template <bool SAVE>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_dyn_density_flat(FieldArgs a, DynW w) {
  dyn_density_body<false, SAVE, false, true>(a, w, nullptr, grid_ctx());
}
__global__ __launch_bounds__(512) void k_ray_scan(FieldArgs a) { ray_scan_body(a); }   // 16 rays per workgroup

// ------------------------------------------------------------------------------------------------
// scene flow MLP over all N*S samples (models/tensoRF.py:446-462)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_scene_flow(const float* __restrict__ pts,
                                                   const float* __restrict__ ts, int N, int S,
                                                   Box box, const float* __restrict__ pkg, DynW w,
                                                   float* __restrict__ sf_f,
                                                   float* __restrict__ sf_b,
                                                   float* __restrict__ act_rows, int dynq) {
  __shared__ __attribute__((aligned(16))) float lds[pk::SF_SIZE];
  __shared__ int s_next;
  if (threadIdx.x == 0) s_next = blockDim.x >> 6;
  lds_fill(lds, pkg + pk::REG_SF, pk::SF_SIZE);
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const float* pkw = lds;
  const int total = N * S;
  const int ntiles = (total + 31) >> 5;
  for (int k = wave, tile; (tile = blockIdx.x + k * gridDim.x) < ntiles; k = tile_queue_next(&s_next, k, nwaves, dynq != 0)) {
    const int li = tile * 32 + s;
    const bool act = li < total;
    const int idx = act ? li : 0;
    const float t = ts[idx / S];
    const float xn0 = norm_c(pts[(size_t)idx * 3 + 0], box.lo[0], box.inv[0]);
    const float xn1 = norm_c(pts[(size_t)idx * 3 + 1], box.lo[1], box.inv[1]);
    const float xn2 = norm_c(pts[(size_t)idx * 3 + 2], box.lo[2], box.inv[2]);
    float X[20];
    fill_sf_x(X, xn0, xn1, xn2, t, h);
    float* svb = act_rows ? act_rows + (size_t)tile * sv::SF_ROWS * 32 : nullptr;
    save_rows<20>(svb, sv::SF_X, X, s, h);
    float sf[6];
    sf_mlp(sf, X, pkw, w.sfb6, svb, s, h, lane);
    if (act && h == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sf_f[(size_t)idx * 3 + c] = sf[c];
#pragma unroll
      for (int c = 0; c < 3; ++c) sf_b[(size_t)idx * 3 + c] = sf[3 + c];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
void fill_common(FieldArgs& a, const RdrfFieldCfg* cfg, const float* rays, const float* ts,
                        const float* xyz, const float* z, const uint8_t* valid, int N, int S) {
  memset(&a, 0, sizeof(a));
  a.rays = rays; a.ts = ts; a.xyz = xyz; a.z = z; a.valid = valid;
  a.N = N; a.S = S;
  a.box = make_box(cfg);
  a.distance_scale = cfg->distance_scale;
  a.weight_thres = cfg->weight_thres;
  a.density_shift = cfg->density_shift;
  a.act = cfg->act;
  a.ray_type = cfg->ray_type;
  a.static_head = cfg->static_head;
}

void dyn_pack_jobs_fwd(PackJobs& J, const RdrfDynamicParams* P) {
  using namespace pk;
  J.n = 0;
  const int k1 = REG_K1, k3 = REG_K3, sf = REG_SF;
  pack_add(J, P->l3w, 93, 64, 93, SEG_WARP3_X0, 0, 2, 32, k1 + K1_W3_X0);
  pack_add(J, P->l3w, 93, 64, 93, SEG_WARP3_T, 0, 2, 16, k1 + K1_W3_T);
  pack_add(J, P->l4w, 64, 64, 64, SEG_IDENT, 0, 2, 32, k1 + K1_W4);
  pack_add(J, P->l5w, 64, 3, 64, SEG_IDENT, 1, 3, 32, k1 + K1_W5);
#ifdef RDRF_HEADS_F32
  pack_add(J, P->dw1, 152, 64, 72, SEG_IDENT, 0, 2, 36, k1 + K1_DEN1_F);
  pack_add(J, P->dw1, 152, 64, 152, SEG_DEN1_X0, 0, 2, 32, k1 + K1_DEN1_X0);
  pack_add(J, P->dw1, 152, 64, 152, SEG_DEN1_X1, 0, 2, 8, k1 + K1_DEN1_X1);
  pack_add(J, P->bw1, 152, 64, 72, SEG_IDENT, 0, 2, 36, k1 + K1_BLE1_F);
  pack_add(J, P->bw1, 152, 64, 152, SEG_DEN1_X0, 0, 2, 32, k1 + K1_BLE1_X0);
  pack_add(J, P->bw1, 152, 64, 152, SEG_DEN1_X1, 0, 2, 8, k1 + K1_BLE1_X1);
#else
  for (int head = 0; head < 2; ++head) {   // bf16 x 3 image [F 36 | X0 32 | X1 0..3] + the fp32 tail X1 4..7 (pk::K1_DEN1)
    const float* w1 = head == 0 ? P->dw1 : P->bw1;
    const int img = k1 + (head == 0 ? K1_DEN1 : K1_BLE1), tail = k1 + (head == 0 ? K1_DEN1_X1T : K1_BLE1_X1T);
    pack_add_b3(J, w1, 152, 64, 72, SEG_IDENT, 2, 36, 0, 0, K1_HEAD_KK, img);
    pack_add_b3(J, w1, 152, 64, 152, SEG_DEN1_X0, 2, 32, 0, 36, K1_HEAD_KK, img);
    pack_add_b3(J, w1, 152, 64, 152, SEG_DEN1_X1, 2, 4, 0, 68, K1_HEAD_KK, img);
    pack_add_from(J, w1, 152, 64, 152, SEG_DEN1_X1, 2, 4, 4, tail);
  }
#endif
  pack_add(J, P->dw2, 64, 1, 64, SEG_IDENT, 1, 1, 32, k1 + K1_DEN2);
  pack_add(J, P->bw2, 64, 1, 64, SEG_IDENT, 1, 1, 32, k1 + K1_BLE2);
  pack_add(J, P->l3b, 0, 64, 0, 0, 3, 0, 32, k1 + K1_B3);
  pack_add(J, P->l4b, 0, 64, 0, 0, 3, 0, 32, k1 + K1_B4);
  pack_add(J, P->db1, 0, 64, 0, 0, 3, 0, 32, k1 + K1_BD1);
  pack_add(J, P->bb1, 0, 64, 0, 0, 3, 0, 32, k1 + K1_BB1);
  pack_add(J, P->basis, 216, 27, 216, SEG_IDENT, 0, 1, 108, k3 + K3_BASIS);
#ifdef RDRF_APP_F32   // A/B builds: the hidden layers on the fp32 matrix pipe, as up to round 5
  pack_add(J, P->rw1, 107, 128, 107, SEG_RGB1_F, 0, 4, 16, k3 + K3_RGB1_F);
  pack_add(J, P->rw1, 107, 128, 107, SEG_RGB1_X0, 0, 4, 32, k3 + K3_RGB1_X0);
  pack_add(J, P->rw1, 107, 128, 107, SEG_RGB1_X1, 0, 4, 8, k3 + K3_RGB1_X1);
  pack_add(J, P->rw2, 128, 128, 128, SEG_IDENT, 0, 4, 64, k3 + K3_RGB2);
#else                 // bf16 x 3 with split storage (same image offsets and sizes; lo pieces behind the images)
  pack_add_b3s(J, P->rw1, 107, 128, 107, SEG_RGB1_F, 4, 16, 0, 0, 16, k3 + K3_RGB1_F, REG_K3_LO + K3_LO_RGB1_F);
  pack_add_b3s(J, P->rw1, 107, 128, 107, SEG_RGB1_X0, 4, 32, 0, 0, 32, k3 + K3_RGB1_X0, REG_K3_LO + K3_LO_RGB1_X0);
  pack_add_b3s(J, P->rw1, 107, 128, 107, SEG_RGB1_X1, 4, 8, 0, 0, 8, k3 + K3_RGB1_X1, REG_K3_LO + K3_LO_RGB1_X1);
  pack_add_b3s(J, P->rw2, 128, 128, 128, SEG_IDENT, 4, 64, 0, 0, 64, k3 + K3_RGB2, REG_K3_LO + K3_LO_RGB2);
#endif
  pack_add(J, P->rwv, 131, 3, 128, SEG_IDENT, 1, 3, 64, k3 + K3_RGBV);
  pack_add(J, P->rb1, 0, 128, 0, 0, 3, 0, 64, k3 + K3_B1);
  pack_add(J, P->rb2, 0, 128, 0, 0, 3, 0, 64, k3 + K3_B2);
  pack_add(J, P->sfw[0], 36, 64, 36, SEG_SF_X, 0, 2, 20, sf + SF_W0);
  pack_add(J, P->sfw[1], 64, 64, 64, SEG_IDENT, 0, 2, 32, sf + SF_W2);
  pack_add(J, P->sfw[2], 64, 64, 64, SEG_IDENT, 0, 2, 32, sf + SF_W4);
  pack_add(J, P->sfw[3], 64, 6, 64, SEG_IDENT, 1, 6, 32, sf + SF_W6);
  pack_add(J, P->sfb[0], 0, 64, 0, 0, 3, 0, 32, sf + SF_B0);
  pack_add(J, P->sfb[1], 0, 64, 0, 0, 3, 0, 32, sf + SF_B2);
  pack_add(J, P->sfb[2], 0, 64, 0, 0, 3, 0, 32, sf + SF_B4);
}

void static_pack_jobs_fwd(PackJobs& J, const RdrfStaticParams* P, int head) {
  using namespace pk;
  J.n = 0;
  const bool fea = head == RDRF_HEAD_MLP_FEA;
  const int in1 = fea ? 138 : 135;
  pack_add(J, P->basis, 72, 27, 72, SEG_IDENT, 0, 1, 36, REG_S3 + S3_BASIS);
#ifdef RDRF_APP_F32   // A/B builds: the hidden layers on the fp32 matrix pipe, as up to round 5
  pack_add(J, P->w1, in1, 128, in1, fea ? SEG_STAT1_F_FEA : SEG_STAT1_F_TE, 0, 4, 16, REG_S3 + S3_W1_F);
  pack_add(J, P->w1, in1, 128, in1, fea ? SEG_STAT1_P_FEA : SEG_STAT1_P_TE, 0, 4, 64, REG_S3 + S3_W1_P);
  pack_add(J, P->w2, 128, 128, 128, SEG_IDENT, 0, 4, 64, REG_S3 + S3_W2);
#else                 // bf16 x 3 with split storage: hi + mid pieces in the image (same offsets and sizes), lo pieces streamed
  pack_add_b3s(J, P->w1, in1, 128, in1, fea ? SEG_STAT1_F_FEA : SEG_STAT1_F_TE, 4, 16, 0, 0, 16, REG_S3 + S3_W1_F, REG_S3_LO + S3_LO_W1_F);
  pack_add_b3s(J, P->w1, in1, 128, in1, fea ? SEG_STAT1_P_FEA : SEG_STAT1_P_TE, 4, 64, 0, 0, 64, REG_S3 + S3_W1_P, REG_S3_LO + S3_LO_W1_P);
  pack_add_b3s(J, P->w2, 128, 128, 128, SEG_IDENT, 4, 64, 0, 0, 64, REG_S3 + S3_W2, REG_S3_LO + S3_LO_W2);
#endif
  pack_add(J, P->w3, fea ? 128 : 131, 3, 128, SEG_IDENT, 1, 3, 64, REG_S3 + S3_W3);
  pack_add(J, P->b1, 0, 128, 0, 0, 3, 0, 64, REG_S3 + S3_B1);
  pack_add(J, P->b2, 0, 128, 0, 0, 3, 0, 64, REG_S3 + S3_B2);
}

void fill_static_w(StaticW& w, const RdrfStaticParams* P) {
  w.density = P->density; w.app = P->app;
  w.b1 = P->b1; w.b2 = P->b2; w.b3 = P->b3; w.w3 = P->w3;
}
void fill_dyn_w(DynW& w, const RdrfDynamicParams* P) {
  w.density = P->density; w.blending = P->blending; w.app = P->app;
  w.l1w = P->l1w; w.l1b = P->l1b; w.l2w = P->l2w; w.l2b = P->l2b;
  w.l3b = P->l3b; w.l4b = P->l4b; w.l5b = P->l5b;
  w.db1 = P->db1; w.db2 = P->db2; w.bb1 = P->bb1; w.bb2 = P->bb2;
  w.rb1 = P->rb1; w.rb2 = P->rb2; w.rbv = P->rbv; w.rwv = P->rwv;
  w.sfb0 = P->sfb[0]; w.sfb2 = P->sfb[1]; w.sfb4 = P->sfb[2]; w.sfb6 = P->sfb[3];
}

// forward calls (either field, scene flow): pack area + counter + tout + xw + list -- what an inference-only caller needs.
// The render workspaces are cut in slices of this size (rdrf_render.hip), so it keeps its closed form.
extern "C" size_t rdrf_forward_workspace_bytes(int N, int S) {
  const size_t ns = (size_t)N * S;
  return (size_t)PACK_AREA_FLOATS * 4 + 256 + (size_t)N * 32 * 4 + ns * 3 * 4 + ns * 4 + (1 << 12);
}

static int ws_carve_fwd_ex(FieldArgs& a, void* ws, size_t ws_bytes, int N, int S, void* saved,
                           size_t saved_bytes, int dynamic, int flags) {
  WsCarver c(ws, ws_bytes);
  size_t ns = (size_t)N * S;
  a.pk = c.take<float>(PACK_AREA_FLOATS);
  a.counter = c.take<int>(64);
  a.tout = c.take<float>((size_t)N * 32);
  a.xw = c.take<float>(ns * 3);
  a.list = c.take<int>(ns);
  RDRF_CHECK(c.ok(), -3, "workspace too small: need %zu have %zu", c.off, ws_bytes);
  if (saved != nullptr) {  // training mode: the backward re-uses these instead of recomputing
    SavedPtrs sp;
    RDRF_CHECK(carve_saved(sp, saved, saved_bytes, dynamic, N, S, flags), -3,
               "saved buffer too small: need %zu have %zu", saved_bytes_field(dynamic, N, S, flags),
               saved_bytes);
    a.counter = &sp.hdr->count;
    a.list = sp.list;
    a.xw = sp.xw;
    a.tout = sp.tout;
    a.raw = sp.raw;
    a.act1 = sp.act1;
    a.act3 = sp.act3;   // nullptr with RDRF_SAVE_NO_APP
  }
  return 0;
}

int ws_carve_fwd(FieldArgs& a, void* ws, size_t ws_bytes, int N, int S, void* saved,
                 size_t saved_bytes, int dynamic) {
  return ws_carve_fwd_ex(a, ws, ws_bytes, N, S, saved, saved_bytes, dynamic, 0);
}

extern "C" size_t rdrf_saved_bytes_ex(int kind, int N, int S, int flags) {
  if (kind == 2) return ((size_t)N * S + 31) / 32 * sv::SF_ROWS * 32 * 4 + 256;
  return saved_bytes_field(kind == 1, N, S, flags);
}
extern "C" size_t rdrf_saved_bytes(int kind, int N, int S) { return rdrf_saved_bytes_ex(kind, N, S, 0); }

extern "C" size_t rdrf_saved_row_bytes(int phase) {
  return (size_t)4 * (phase == 0 ? sv::K1_ROWS : phase == 1 ? sv::K3_ROWS : phase == 2 ? sv::S3_ROWS : sv::SF_ROWS);
}

// FieldArgs::dynq of the forward launches: bit 0 = per-workgroup tile queue (+1-2 % on the compacted-tile MLP kernels)
int fwd_dynq() { return 1; }

extern "C" int rdrf_static_fwd_ex(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* rays,
                                  const float* ts, const float* xyz, const float* z,
                                  const uint8_t* valid, int N, int S, float* rgb, float* sigma,
                                  float* weight, float* dists, void* saved, size_t saved_bytes,
                                  void* ws, size_t ws_bytes, rdrf_stream_t stream_, int flags) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && N > 0 && S > 0, -1, "static_fwd: bad arguments");
  RDRF_CHECK((flags & ~RDRF_SAVE_NO_APP) == 0, -1, "static_fwd: unknown flags 0x%x", flags);
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "static_fwd: N * S * 3 must stay below 2^31 (32-bit sample indices): render / train in smaller chunks");
  RDRF_CHECK(vm_ok(P->density, 16, 4) && vm_ok(P->app, 48, 12), -1,
             "static_fwd: only density comps {16,4,4} / app comps {48,12,12}, the planes and lines of a set spanning one grid, are built");
  FieldArgs a;
  fill_common(a, cfg, rays, ts, xyz, z, valid, N, S);
  a.rgb = rgb; a.sigma = sigma; a.weight = weight; a.dists = dists;
  RDRF_TRY(ws_carve_fwd_ex(a, ws, ws_bytes, N, S, saved, saved_bytes, 0, flags));
  // rows are saved only where a backward can read them: no buffer, or one without appearance rows (RDRF_SAVE_NO_APP: the
  // colours are values only) -> the inference instantiation of the appearance kernel
  const bool save_app = saved != nullptr && !(flags & RDRF_SAVE_NO_APP);
  StaticW w;
  fill_static_w(w, P);
  RDRF_TRY(pack_image(a.pk, P->packed_fwd, (float*)a.pk, stream, static_pack_jobs_fwd, P, cfg->static_head));
  RDRF_FILL(a.counter, 0, 256, stream);   // (the colours are zero-filled by k_static_density)
#ifdef RDRF_DETERMINISTIC
  RDRF_FILL(a.list, 0x7f, (size_t)N * S * sizeof(int), stream);
#endif
  RDRF_LAUNCH("static_density", k_static_density<false>, dim3((N + 3) / 4), dim3(256), stream, a, w);   // 4 rays per workgroup: one list append
  if (rgb == nullptr) return 0;   // the caller does not consume the colours: the appearance phase is not run
#ifdef RDRF_DETERMINISTIC
  RDRF_TRY(rdrf_sort_ints_inplace(a.list, (unsigned)((size_t)N * S), stream));   // append order depends on wave timing
#endif
  const Geo g = geo_for_tiles(N, S);
  const bool fea = cfg->static_head == RDRF_HEAD_MLP_FEA;
  a.dynq = fwd_dynq();
  if (save_app) {
    if (fea) RDRF_LAUNCH("static_app", (k_static_app<RDRF_HEAD_MLP_FEA, false, true>), dim3(g.grid), dim3(g.block), stream, a, w);
    else RDRF_LAUNCH("static_app", (k_static_app<RDRF_HEAD_MLP_FEA_TIMEEMBEDDING, false, true>), dim3(g.grid), dim3(g.block), stream, a, w);
  } else {
    if (fea) RDRF_LAUNCH("static_app", (k_static_app<RDRF_HEAD_MLP_FEA, false, false>), dim3(g.grid), dim3(g.block), stream, a, w);
    else RDRF_LAUNCH("static_app", (k_static_app<RDRF_HEAD_MLP_FEA_TIMEEMBEDDING, false, false>), dim3(g.grid), dim3(g.block), stream, a, w);
  }
  return 0;
}

extern "C" int rdrf_static_fwd(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* rays,
                               const float* ts, const float* xyz, const float* z,
                               const uint8_t* valid, int N, int S, float* rgb, float* sigma,
                               float* weight, float* dists, void* saved, size_t saved_bytes,
                               void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  return rdrf_static_fwd_ex(P, cfg, rays, ts, xyz, z, valid, N, S, rgb, sigma, weight, dists, saved, saved_bytes, ws, ws_bytes,
                            stream_, 0);
}

// the per-ray scan of the flat density phase (rdrf_render_host.hpp): rdrf_dynamic_fwd_ex below and rdrf_selftest_ray_scan
int launch_ray_scan(const FieldArgs& a, hipStream_t stream) {
  RDRF_LAUNCH("ray_scan", k_ray_scan, dim3((a.N + 15) / 16), dim3(512), stream, a);
  return 0;
}

// the time branch of N rays or points, 8 per workgroup (rdrf_render_host.hpp): the two entry points below and
// rdrf_selftest_time_branch; zero64: nullable counter block, cleared on the way
int launch_time_branch(const float* ts, const DynW& w, int N, float* tout, int* zero64, hipStream_t stream) {
  RDRF_LAUNCH("time_branch", k_time_branch, dim3((N + 7) / 8), dim3(256), stream, ts, w, N, tout, zero64);
  return 0;
}

extern "C" int rdrf_dynamic_fwd_ex(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg,
                                   const float* rays, const float* ts, const float* xyz,
                                   const float* z, const uint8_t* valid, int N, int S,
                                   float* blending, float* weight, float* xyz_prime, float* rgb,
                                   float* sigma, float* dists, void* saved, size_t saved_bytes,
                                   void* ws, size_t ws_bytes, rdrf_stream_t stream_, int flags) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && N > 0 && S > 0, -1, "dynamic_fwd: bad arguments");
  RDRF_CHECK((flags & ~RDRF_SAVE_NO_APP) == 0, -1, "dynamic_fwd: unknown flags 0x%x", flags);
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "dynamic_fwd: N * S * 3 must stay below 2^31 (32-bit sample indices): render / train in smaller chunks");
  RDRF_CHECK(vm_ok(P->density, 16, 4) && vm_ok(P->blending, 16, 4) && vm_ok(P->app, 48, 12) && vm_same_grid(P->density, P->blending), -1,
             "dynamic_fwd: only density comps {16,4,4} / app comps {48,12,12}, the planes and lines of a set spanning one grid, are built");
  FieldArgs a;
  fill_common(a, cfg, rays, ts, xyz, z, valid, N, S);
  a.rgb = rgb; a.sigma = sigma; a.weight = weight; a.dists = dists;
  a.blending = blending; a.xyz_prime = xyz_prime;
  a.dynq = fwd_dynq();
  RDRF_TRY(ws_carve_fwd_ex(a, ws, ws_bytes, N, S, saved, saved_bytes, 1, flags));
  DynW w;
  fill_dyn_w(w, P);
  RDRF_TRY(pack_image(a.pk, P->packed_fwd, (float*)a.pk, stream, dyn_pack_jobs_fwd, P));
  // the density phase runs at tile granularity (k_dyn_density_flat + k_ray_scan): no tile is padded to the end of its ray,
  // and a 512-ray eval chunk fills the chip.  In training the saved rows are addressed by flat tile, and the backward
  // (rdrf_dynamic_bwd) reads them the same way: both sides take the switch from rdrf_flat_density()
  const bool flat = rdrf_flat_density();
  if (!flat && rgb != nullptr) RDRF_FILL(rgb, 0, (size_t)N * S * 3 * sizeof(float), stream);   // flat: k_ray_scan
  RDRF_TRY(launch_time_branch(ts, w, N, a.tout, a.counter, stream));
  const Geo g1 = geo_for_units(N), g3 = geo_for_tiles(N, S);
#ifdef RDRF_DETERMINISTIC
  RDRF_FILL(a.list, 0x7f, (size_t)N * S * sizeof(int), stream);
#endif
  if (flat) {
    if (saved != nullptr) RDRF_LAUNCH("dyn_density", k_dyn_density_flat<true>, dim3(g3.grid), dim3(g3.block), stream, a, w);
    else RDRF_LAUNCH("dyn_density", k_dyn_density_flat<false>, dim3(g3.grid), dim3(g3.block), stream, a, w);
    RDRF_TRY(launch_ray_scan(a, stream));
  } else if (saved != nullptr) RDRF_LAUNCH("dyn_density", (k_dyn_density<false, true>), dim3(g1.grid), dim3(g1.block), stream, a, w);
  else RDRF_LAUNCH("dyn_density", (k_dyn_density<false, false>), dim3(g1.grid), dim3(g1.block), stream, a, w);
#ifdef RDRF_DETERMINISTIC
  RDRF_TRY(rdrf_sort_ints_inplace(a.list, (unsigned)((size_t)N * S), stream));
#endif
  if (rgb == nullptr) return 0;   // the caller does not consume the colours: the appearance phase is not run
  // RDRF_SAVE_NO_APP: the density phase above saved as usual (list, xw, tout, raw, K1 rows, count); the colours are values
  // only, so the appearance phase is the inference instantiation and writes no K3 rows (see rdrf_static_fwd_ex)
  if (saved != nullptr && !(flags & RDRF_SAVE_NO_APP)) RDRF_LAUNCH("dyn_app", (k_dyn_app<false, true>), dim3(g3.grid), dim3(g3.block), stream, a, w);
  else RDRF_LAUNCH("dyn_app", (k_dyn_app<false, false>), dim3(g3.grid), dim3(g3.block), stream, a, w);
  return 0;
}

extern "C" int rdrf_dynamic_fwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg,
                                const float* rays, const float* ts, const float* xyz,
                                const float* z, const uint8_t* valid, int N, int S,
                                float* blending, float* weight, float* xyz_prime, float* rgb,
                                float* sigma, float* dists, void* saved, size_t saved_bytes,
                                void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  return rdrf_dynamic_fwd_ex(P, cfg, rays, ts, xyz, z, valid, N, S, blending, weight, xyz_prime, rgb, sigma, dists, saved,
                             saved_bytes, ws, ws_bytes, stream_, 0);
}

// ------------------------------------------------------------------------------------------------
// feature mode: compute_densityfeature / compute_appfeature / compute_blendingfeature /
// warp_coordinate on a batch of M independent points (models/tensoRF.py:118-196, 521-811).  The same
// kernels in pseudo-ray geometry: N = ceil(M/32) rays of 32 samples, time per point.
// ------------------------------------------------------------------------------------------------
extern "C" size_t rdrf_features_saved_bytes(int dynamic, int M) { return saved_bytes_feat(dynamic, M); }
extern "C" size_t rdrf_features_workspace_bytes(int M) {
  const int Np = (M + 31) / 32;
  return rdrf_workspace_bytes(Np, 32) + (size_t)Np * 32 * (32 * 4 + 27 * 4 + 8) + (1 << 14);
}

static int feat_carve_fwd(FieldArgs& a, void* ws, size_t ws_bytes, int M, void* saved, size_t saved_bytes,
                          int dynamic) {
  WsCarver c(ws, ws_bytes);
  const size_t mp = ((size_t)M + 31) / 32 * 32;
  a.pk = c.take<float>(PACK_AREA_FLOATS);
  a.tout = c.take<float>(mp * 32);
  a.xw = c.take<float>(mp * 3);
  RDRF_CHECK(c.ok(), -3, "features: workspace too small: need %zu have %zu", c.off, ws_bytes);
  if (saved != nullptr) {
    SavedPtrs sp;
    RDRF_CHECK(carve_saved_feat(sp, saved, saved_bytes, dynamic, M), -3,
               "features: saved buffer too small: need %zu have %zu", saved_bytes_feat(dynamic, M), saved_bytes);
    a.xw = sp.xw; a.tout = sp.tout; a.raw = sp.raw; a.act1 = sp.act1; a.act3 = sp.act3;
  }
  return 0;
}

extern "C" int rdrf_static_features_fwd(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* xn,
                                        int M, float* density, float* app, void* saved, size_t saved_bytes,
                                        void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && xn && M > 0 && (density || app), -1, "static_features_fwd: bad arguments");
  RDRF_CHECK(vm_ok(P->density, 16, 4) && vm_ok(P->app, 48, 12), -1,
             "static_features_fwd: only density comps {16,4,4} / app comps {48,12,12}, the planes and lines of a set spanning one grid, are built");
  const int Np = (M + 31) / 32;
  FieldArgs a;
  fill_common(a, cfg, nullptr, nullptr, xn, nullptr, nullptr, Np, 32);
  a.M = M; a.in_norm = 1; a.sigma = density; a.feat = app;
  RDRF_TRY(feat_carve_fwd(a, ws, ws_bytes, M, saved, saved_bytes, 0));
  StaticW w;
  fill_static_w(w, P);
  if (density != nullptr)
    RDRF_LAUNCH("feat_static_density", k_static_density<true>, dim3(Np), dim3(64), stream, a, w);
  if (app != nullptr) {
    RDRF_TRY(pack_image(a.pk, P->packed_fwd, (float*)a.pk, stream, static_pack_jobs_fwd, P, cfg->static_head));
    const Geo g = geo_for_units(Np);
    RDRF_LAUNCH("feat_static_app", (k_static_app<RDRF_HEAD_MLP_FEA, true>), dim3(g.grid), dim3(g.block), stream,
                a, w);
  }
  return 0;
}

extern "C" int rdrf_dynamic_features_fwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* x,
                                         const float* t, int M, int x_is_normalized, float* density,
                                         float* blending, float* app, float* xyz_prime, void* saved,
                                         size_t saved_bytes, void* ws, size_t ws_bytes,
                                         rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && x && t && M > 0 && (density || blending || app || xyz_prime), -1,
             "dynamic_features_fwd: bad arguments");
  RDRF_CHECK(vm_ok(P->density, 16, 4) && vm_ok(P->blending, 16, 4) && vm_ok(P->app, 48, 12) && vm_same_grid(P->density, P->blending), -1,
             "dynamic_features_fwd: only density comps {16,4,4} / app comps {48,12,12}, the planes and lines of a set spanning one grid, are built");
  const int Np = (M + 31) / 32;
  FieldArgs a;
  fill_common(a, cfg, nullptr, t, x, nullptr, nullptr, Np, 32);
  a.M = M; a.in_norm = x_is_normalized ? 1 : 0;
  a.sigma = density; a.blending = blending; a.feat = app; a.xyz_prime = xyz_prime;
  RDRF_TRY(feat_carve_fwd(a, ws, ws_bytes, M, saved, saved_bytes, 1));
  DynW w;
  fill_dyn_w(w, P);
  RDRF_TRY(pack_image(a.pk, P->packed_fwd, (float*)a.pk, stream, dyn_pack_jobs_fwd, P));
  RDRF_TRY(launch_time_branch(t, w, M, a.tout, nullptr, stream));
  const Geo g = geo_for_units(Np);
  RDRF_LAUNCH("feat_dyn_density", k_dyn_density<true>, dim3(g.grid), dim3(g.block), stream, a, w);
  if (app != nullptr) RDRF_LAUNCH("feat_dyn_app", k_dyn_app<true>, dim3(g.grid), dim3(g.block), stream, a, w);
  return 0;
}

extern "C" int rdrf_scene_flow_fwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg,
                                   const float* pts, const float* ts, int N, int S, float* sf_f,
                                   float* sf_b, void* saved, size_t saved_bytes, void* ws,
                                   size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && N > 0 && S > 0, -1, "scene_flow_fwd: bad arguments");
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "scene_flow_fwd: N * S * 3 must stay below 2^31 (32-bit sample indices): render / train in smaller chunks");
  FieldArgs a;
  memset(&a, 0, sizeof(a));
  RDRF_CHECK(saved == nullptr || saved_bytes >= rdrf_saved_bytes(2, N, S), -3,
             "scene_flow_fwd: saved buffer too small");
  RDRF_TRY(ws_carve_fwd(a, ws, ws_bytes, N, S, nullptr, 0, 1));
  DynW w;
  fill_dyn_w(w, P);
  RDRF_TRY(pack_image(a.pk, P->packed_fwd, (float*)a.pk, stream, dyn_pack_jobs_fwd, P));
  const Geo g = geo_for_tiles(N, S);
  RDRF_LAUNCH("scene_flow", k_scene_flow, dim3(g.grid), dim3(g.block), stream, pts, ts, N, S,
              make_box(cfg), a.pk, w, sf_f, sf_b, (float*)saved, fwd_dynq());
  return 0;
}
