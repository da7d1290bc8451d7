// rdrf_scene_alpha.hip -- the whole scene on points: both fields evaluated at M points x T times and composed the way the
// renderer composes a sample (rdrf_composite_fwd / rdrf_render_hits_fwd: the factor (1 - a_d b)(1 - a_s (1 - b)) and the
// `owner` of a hit), without a ray around it.  include/rodynrf.h, rdrf_scene_alpha, has the definition and its order.
//
//   k_scene_time_branch : time_branch_body over the T times
//   k_scene_static      : a lane per point, static_density_feature + density_act as k_alpha_static / k_point_static.  The static
//                         sigma does not depend on the time: it goes into the workspace ([M], before the mask) for the tile
//                         kernel, and -- where the caller asks for sigma_s -- masked per time into that output
//   k_scene_alpha       : k_alpha_dyn with both heads -- flat 32-point tiles from the workgroup's queue, K1 image in LDS,
//                         [xn, PE10(xn)] once per point, a T-loop behind the compiler barrier; per (point, time) ONE warp_mlp /
//                         warp_point for head_raw<false> and head_raw<true>, then, where only the two raw head outputs are live,
//                         the two mask lookups, density_act, the sigmoid of k_point_dyn, the static sigma from the workspace and
//                         the composition.  <DEN, BLE>: a head nobody reads is not evaluated
//
// Why a pre-pass and not the static field inside the tile kernel: the tile kernel is an MFMA kernel with two lanes per point
// (halves h = 0 / 1 of a column) at 8 waves per CU; a lane-per-point gather runs there at half the lanes and a quarter of the
// occupancy, and its plane / line pointers would be live across the layers of a kernel that has no registers to spare
// (k_alpha_dyn: 219 VGPRs with one head).  As a pre-pass it costs 4 bytes written and 4 read per point, once for all T.
//
// An MFMA column depends on its own sample only, so an entry depends on its own point and time alone.  No atomics on global
// memory: the deterministic build runs the same code.  The call allocates nothing, does not synchronise, reads nothing back.
#include "rdrf_misc_dev.hpp"
#include "rdrf_mask_dev.hpp"

struct SceneAlphaArgs {
  const float* xyz;      // [M][3] un-normalised
  const float* times;    // [T]
  const float* pk;       // packed forward image (dynamic)
  const float* tout;     // [T][32] time-branch outputs
  const float* sig_s;    // [M] static sigma before the mask (k_scene_static), or nullptr: neither alpha nor owner is asked for
  float *alpha, *owner, *sigma_d, *blending;   // [M][T], each nullable
  long long M;
  int T;
  float length, density_shift;
  int act, dynq;
  Box box;               // the dynamic field's
  MaskDev mask_s, mask_d;
};

struct SceneStaticArgs {
  const float* xyz;
  const float* times;
  float* sig_ws;         // [M] or nullptr
  float* sigma_s;        // [M][T] or nullptr
  long long M;
  int T;
  float density_shift;
  int act;
  Box box;               // the static field's
  MaskDev mask;
};

// alpha and owner of one entry from the two fields' opacities and the blending.  No contraction: the order below is the one
// include/rodynrf.h states and tests/_scene_prim.py counts its bound from.
RDRF_D void scene_compose(float a_d, float a_s, float b, float& alpha, float& owner) {
#pragma clang fp contract(off)
  const float w_d = a_d * b;
  const float nb = 1.0f - b;
  const float w_s = a_s * nb;
  const float u = 1.0f - w_d;
  const float v = 1.0f - w_s;
  const float uv = u * v;
  alpha = 1.0f - uv;
  const float den = w_d + w_s;
  owner = den == 0.0f ? 0.0f : w_d / den;
}

__global__ __launch_bounds__(256) void k_scene_time_branch(const float* __restrict__ ts, DynW w, int N, float* __restrict__ tout) {
  __shared__ float s_h[8 * 64];
  time_branch_body(ts, w, N, tout, s_h, grid_ctx());
}

__global__ __launch_bounds__(256) void k_scene_static(SceneStaticArgs a, StaticW w) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.M; i += (long long)gridDim.x * blockDim.x) {
    const size_t idx = (size_t)i;
    const float px = a.xyz[idx * 3 + 0], py = a.xyz[idx * 3 + 1], pz = a.xyz[idx * 3 + 2];
    const float x0 = norm_c(px, a.box.lo[0], a.box.inv[0]);
    const float x1 = norm_c(py, a.box.lo[1], a.box.inv[1]);
    const float x2 = norm_c(pz, a.box.lo[2], a.box.inv[2]);
    const float sig = density_act(static_density_feature(w.density, x0, x1, x2), a.act, a.density_shift);
    if (a.sig_ws != nullptr) a.sig_ws[idx] = sig;
    if (a.sigma_s == nullptr) continue;
    for (int kt = 0; kt < a.T; ++kt) {
      bool vld = true;
      if (a.mask.bits != nullptr) vld = mask_sample(a.mask, px, py, pz, mask_slice(a.mask, a.times[kt])) > 0.0f;
      a.sigma_s[idx * a.T + kt] = vld ? sig : 0.0f;
    }
  }
}

template <bool DEN, bool BLE>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_scene_alpha(SceneAlphaArgs a, DynW w) {
  __shared__ __attribute__((aligned(16))) float lds[pk::K1_SIZE];
  __shared__ int s_next;
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  if (threadIdx.x == 0) s_next = nwaves;
  lds_fill(lds, a.pk + pk::REG_K1, pk::K1_SIZE);
  const float* pkw = lds;
  const long long ntiles = (a.M + 31) >> 5;
  const bool dynq = (a.dynq & 1) != 0;
  for (int k = wave; (long long)blockIdx.x + (long long)k * gridDim.x < ntiles; k = tile_queue_next(&s_next, k, nwaves, dynq)) {
    const long long tile = (long long)blockIdx.x + (long long)k * gridDim.x;
    const long long i = tile * 32 + s;
    const bool act = i < a.M;
    const unsigned idx = act ? (unsigned)i : 0u;   // (M is an int)
    float X0[32];
    {
      const float* p = a.xyz + (size_t)idx * 3;
      fill_x0(X0, norm_c(p[0], a.box.lo[0], a.box.inv[0]), norm_c(p[1], a.box.lo[1], a.box.inv[1]),
              norm_c(p[2], a.box.lo[2], a.box.inv[2]), 0.f, h);
    }   // [xn, PE10(xn)]: once per point; slot 3 of the lower half is the time
    for (int kt = 0; kt < a.T; ++kt) {
      // compiler barrier, as in k_alpha_dyn: nothing below writes LDS, so without it the weight reads of every layer are
      // invariant in kt and get hoisted out of the loop into registers the kernel does not have
      asm volatile("" ::: "memory");
      const float t = a.times[kt];
      if (h == 0) X0[3] = t;
      float T[16];
      load_tout(T, a.tout, (size_t)kt, h);
      float d[3];
      warp_mlp(d, X0, T, pkw, w.l5b, nullptr, s, h, lane);   // once for both heads
      // (the point is read again here and at the mask lookups, as in k_alpha_dyn: six registers less across the layers)
      const float* pp = a.xyz + (size_t)idx * 3;
      asm volatile("" : "+v"(pp));
      const float xn[3] = {norm_c(pp[0], a.box.lo[0], a.box.inv[0]), norm_c(pp[1], a.box.lo[1], a.box.inv[1]),
                           norm_c(pp[2], a.box.lo[2], a.box.inv[2])};
      float xw[3];
      warp_point(xw, xn, d, a.box);
      float X1[8];
      fill_x1(X1, t, h);
      float fd = 0.f, fb = 0.f;
      if constexpr (DEN) fd = head_raw<false>(w, xw, act, X0, X1, pkw, nullptr, s, h, lane);
      // X0 and X1 are made opaque between the heads: both first layers split the same [X0, X1] slots into bf16 pieces
      // (mfma_seg_b3), hipcc keeps the first head's pieces for the second, and the kernel spills 33 registers (128 B of scratch
      // per lane).  The second head splits again (the VALU work k_alpha_dyn spends per head); same values, same bits.  The
      // statements sit between the two calls, not inside a step of mfma_seg_b3 (its no-asm rule).
      if constexpr (DEN && BLE) {
#pragma unroll
        for (int q = 0; q < 32; ++q) asm volatile("" : "+v"(X0[q]));
#pragma unroll
        for (int q = 0; q < 8; ++q) asm volatile("" : "+v"(X1[q]));
      }
      if constexpr (BLE) fb = head_raw<true>(w, xw, act, X0, X1, pkw, nullptr, s, h, lane);
      if (act && h == 0) {
        // only fd and fb are live here: the masks, the activations and the composition cost no register of the layers
        const float* p = a.xyz + (size_t)idx * 3;
        asm volatile("" : "+v"(p));
        const size_t o = (size_t)idx * a.T + kt;
        float sg_d = 0.f, b = 0.f;
        if constexpr (DEN) {
          bool vld = true;
          if (a.mask_d.bits != nullptr) vld = mask_sample(a.mask_d, p[0], p[1], p[2], mask_slice(a.mask_d, t)) > 0.0f;
          sg_d = vld ? density_act(fd, a.act, a.density_shift) : 0.0f;
          if (a.sigma_d != nullptr) a.sigma_d[o] = sg_d;
        }
        if constexpr (BLE) {
          b = sigmoidf_(fb);
          if (a.blending != nullptr) a.blending[o] = b;
        }
        if constexpr (DEN && BLE) {
          if (a.sig_s != nullptr) {
            bool vld = true;
            if (a.mask_s.bits != nullptr) vld = mask_sample(a.mask_s, p[0], p[1], p[2], mask_slice(a.mask_s, t)) > 0.0f;
            const float sg_s = vld ? a.sig_s[idx] : 0.0f;
            float al, ow;
            scene_compose(alpha_of(sg_d, a.length), alpha_of(sg_s, a.length), b, al, ow);
            if (a.alpha != nullptr) a.alpha[o] = al;
            if (a.owner != nullptr) a.owner[o] = ow;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct SceneAlphaWs {
  float* pk;
  float* tout;    // [T][32]
  float* sig_s;   // [M]
};
// one layout for the size call and the launch
static void carve_scene_alpha(SceneAlphaWs& p, WsCarver& c, int M, int T) {
  p.pk = c.take<float>(PACK_AREA_FLOATS);
  p.tout = c.take<float>((size_t)(T > 0 ? T : 0) * 32);
  p.sig_s = c.take<float>(M > 0 ? (size_t)M : 0);
}

extern "C" size_t rdrf_scene_alpha_ws_bytes(int M, int T) {
  SceneAlphaWs p;
  WsCarver c;
  carve_scene_alpha(p, c, M, T);
  return c.off;
}

extern "C" int rdrf_scene_alpha(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                const RdrfFieldCfg* cfg_d, const float* xyz, int M, const float* times, int T, float length,
                                const RdrfAlphaMask* mask_s, const RdrfAlphaMask* mask_d, float* alpha, float* owner,
                                float* sigma_s, float* sigma_d, float* blending, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0) return 0;   // empty batch: a no-op, as rdrf_compute_alpha (the data pointers of empty tensors are null)
  RDRF_CHECK(M > 0 && T >= 1, -1, "scene_alpha: M = %d points and T = %d times: M must not be negative, T must be at least 1", M, T);
  RDRF_CHECK(PS && cfg_s && PD && cfg_d && xyz && times, -1, "scene_alpha: bad arguments");
  RDRF_CHECK(alpha || owner || sigma_s || sigma_d || blending, -1, "scene_alpha: every output is null");
  RDRF_CHECK((long long)M * T < (1ll << 31), -1, "scene_alpha: M * T = %lld entries per output, the limit is 2^31 - 1: call in chunks",
             (long long)M * T);
  RDRF_CHECK(mask_ok(mask_s) && mask_ok(mask_d), -1, "scene_alpha: the masks' grids and slice counts must be positive");
  RDRF_CHECK(vm_ok(PS->density, 16, 4) && vm_ok(PD->density, 16, 4) && vm_ok(PD->blending, 16, 4) && vm_same_grid(PD->density, PD->blending),
             -1, "scene_alpha: only density / blending comps {16,4,4}, the planes and lines of a set spanning one grid, are built");
  RDRF_CHECK(ws != nullptr, -3, "scene_alpha: no workspace");
  WsCarver c(ws, ws_bytes);
  SceneAlphaWs p;
  carve_scene_alpha(p, c, M, T);
  RDRF_CHECK(c.ok(), -3, "scene_alpha: workspace too small: need %zu have %zu", c.off, ws_bytes);

  const bool compose = alpha != nullptr || owner != nullptr;
  const bool den = compose || sigma_d != nullptr, ble = compose || blending != nullptr;
  if (compose || sigma_s != nullptr) {
    SceneStaticArgs a;
    memset(&a, 0, sizeof(a));
    a.xyz = xyz; a.times = times; a.M = M; a.T = T;
    a.sig_ws = compose ? p.sig_s : nullptr;
    a.sigma_s = sigma_s;
    a.density_shift = cfg_s->density_shift; a.act = cfg_s->act;
    a.box = make_box(cfg_s);
    a.mask = make_mask(mask_s);
    StaticW w;
    fill_static_w(w, PS);
    const long blocks = ((long)M + 255) / 256;
    RDRF_LAUNCH("scene_static", k_scene_static, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), stream, a, w);
  }
  if (!den && !ble) return 0;   // sigma_s alone: the dynamic field is not touched

  SceneAlphaArgs a;
  memset(&a, 0, sizeof(a));
  a.xyz = xyz; a.times = times; a.M = M; a.T = T; a.length = length;
  a.alpha = alpha; a.owner = owner; a.sigma_d = sigma_d; a.blending = blending;
  a.sig_s = compose ? p.sig_s : nullptr;
  a.density_shift = cfg_d->density_shift; a.act = cfg_d->act;
  a.box = make_box(cfg_d);
  a.mask_s = make_mask(mask_s);
  a.mask_d = make_mask(mask_d);
  DynW w;
  fill_dyn_w(w, PD);
  RDRF_TRY(pack_image(a.pk, PD->packed_fwd, p.pk, stream, dyn_pack_jobs_fwd, PD));
  a.tout = p.tout;
  a.dynq = 1;
  RDRF_LAUNCH("time_branch", k_scene_time_branch, dim3((T + 7) / 8), dim3(256), stream, times, w, T, p.tout);
  const Geo g = geo_for_units(((long)M + 31) / 32);   // the persistent geometry of the field kernels
  if (den && ble) RDRF_LAUNCH("scene_alpha", (k_scene_alpha<true, true>), dim3(g.grid), dim3(g.block), stream, a, w);
  else if (den) RDRF_LAUNCH("scene_alpha", (k_scene_alpha<true, false>), dim3(g.grid), dim3(g.block), stream, a, w);
  else RDRF_LAUNCH("scene_alpha", (k_scene_alpha<false, true>), dim3(g.grid), dim3(g.block), stream, a, w);
  return 0;
}
