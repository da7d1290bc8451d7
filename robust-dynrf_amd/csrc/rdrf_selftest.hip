// rdrf_selftest.hip -- every MLP layer primitive of rdrf_common.hpp, stand-alone, with the template arguments the product
// kernels use and the product's own pack code (tests/test_gpu_mlp_primitives.py compares the results with float64).
//
// One wave per 32-row tile, as k_selftest (end of the file: a layer with bias and relu): the wave's workgroup copies the packed
// image into LDS, lane (h, s) loads its half of row s in the canonical layout, the primitive runs on ZERO accumulators and
// the raw accumulators are stored: no bias, no relu, so the result is linear in x and w.  Rows past M read as zero and are not stored.
//   forward forms     x[M][K]   , w[OUT][K]  ->  y[M][OUT] = x w^T
//   transposed forms  x[M][OUT] , w[OUT][K]  ->  y[M][K]   = x w      (the backward-data product of the same layer)
//
// rdrf_selftest_dw (end of the file, host code only): the dW job lists of the backward entry points (the builders of
// rdrf_bwd.hip) planned and launched by dw_launch on rows the caller supplies; reference: tests/_dw_prim.py.
//
// rdrf_selftest_sort / rdrf_selftest_scatter (host code only): the radix sort as sorted_scatter_prepare calls it, and the
// gradient scatter through the product's own launch functions (launch_scatter, scatter_dyn_*_sorted of rdrf_scatter.hip) on
// data the caller supplies; reference: tests/_scatter_prim.py.
//
// rdrf_selftest_gather / rdrf_selftest_encodings: the forward VM gather and the positional encodings through the device functions
// of the forward kernels; reference: tests/_gather_prim.py.
//
// rdrf_selftest_ray_scan / rdrf_selftest_ray_scan_bwd (host code only): the per-field ray scan, forward and backward at both
// widths, through the entry points' launchers on arrays the caller supplies; reference: tests/_scan_prim.py.
//
// rdrf_selftest_heads_bwd / rdrf_selftest_time_branch / rdrf_selftest_time_branch_bwd (host code only): the heads' backward tile
// (k_dyn_density_bwd<0> on flat tiles and in feature mode) and the time branch through the entry points' launchers;
// reference: tests/_heads_prim.py.
//
// rdrf_selftest_app_bwd (host code only): the backward-data kernels of the appearance phase (k_dyn_app_bwd, k_static_app_bwd) on
// saved rows the caller supplies, through the entry points' launchers; reference: tests/_app_prim.py.
#include <vector>

#include "rdrf_fwd_dev.hpp"
#include "rdrf_bwd_dev.hpp"
#include "rdrf_bwd_host.hpp"
#include "rdrf_render_host.hpp"
#include "rdrf_sort_dev.hpp"

namespace {

template <int KK>
RDRF_D void st_load(float (&in)[KK], const float* __restrict__ x, int row, int M, int ld, int c0, int h) {
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) in[kk] = row < M ? x[(size_t)row * ld + c0 + elem_of(kk, h)] : 0.f;
}
template <int NBO>
RDRF_D void st_store(const f32x16 (&acc)[NBO], float* __restrict__ y, int row, int M, int ld, int c0, int h) {
  if (row < M)
#pragma unroll
    for (int nb = 0; nb < NBO; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) y[(size_t)row * ld + c0 + nb * 32 + elem_of(r, h)] = acc[nb][r];
}

// mfma_seg<NBO, KK>: 2 KK inputs -> 32 NBO outputs (pack mode 0, or mode 2 for a transposed layer)
template <int NBO, int KK>
__global__ __launch_bounds__(64) void k_st_f32(const float* __restrict__ x, const float* __restrict__ pkw, int M,
                                               float* __restrict__ y) {
  constexpr int IMG = NBO * KK * 64;
  __shared__ __attribute__((aligned(16))) float lds[IMG];
  lds_fill(lds, pkw, IMG);
  const int lane = threadIdx.x & 63, h = lane >> 5, row = blockIdx.x * 32 + (lane & 31);
  float in[KK];
  st_load<KK>(in, x, row, M, 2 * KK, 0, h);
  f32x16 acc[NBO];
  acc_bias<NBO>(acc, nullptr, h);
  mfma_seg<NBO, KK>(acc, in, lds, lane);
  st_store<NBO>(acc, y, row, M, 32 * NBO, 0, h);
}

// mfma_seg_b3<NBO, KK> (pack mode 7, or mode 8 for a transposed layer)
template <int NBO, int KK>
__global__ __launch_bounds__(64) void k_st_b3(const float* __restrict__ x, const float* __restrict__ pkw, int M,
                                              float* __restrict__ y) {
  constexpr int IMG = NBO * KK * 96;
  __shared__ __attribute__((aligned(16))) float lds[IMG];
  lds_fill(lds, pkw, IMG);
  const int lane = threadIdx.x & 63, h = lane >> 5, row = blockIdx.x * 32 + (lane & 31);
  float in[KK];
  st_load<KK>(in, x, row, M, 2 * KK, 0, h);
  f32x16 acc[NBO];
  acc_bias<NBO>(acc, nullptr, h);
  mfma_seg_b3<NBO, KK>(acc, in, lds, lane);
  st_store<NBO>(acc, y, row, M, 32 * NBO, 0, h);
}

// mfma_seg_b3_pair<NA, NB, KK>: two images (A, then B), one input; y = A's 32 NA columns, then B's 32 NB
template <int NA, int NB, int KK>
__global__ __launch_bounds__(64) void k_st_b3_pair(const float* __restrict__ x, const float* __restrict__ pkw, int M,
                                                   float* __restrict__ y) {
  constexpr int IMG_A = NA * KK * 96, IMG = (NA + NB) * KK * 96;
  __shared__ __attribute__((aligned(16))) float lds[IMG];
  lds_fill(lds, pkw, IMG);
  const int lane = threadIdx.x & 63, h = lane >> 5, row = blockIdx.x * 32 + (lane & 31);
  float in[KK];
  st_load<KK>(in, x, row, M, 2 * KK, 0, h);
  f32x16 accA[NA], accB[NB];
  acc_bias<NA>(accA, nullptr, h);
  acc_bias<NB>(accB, nullptr, h);
  mfma_seg_b3_pair<NA, NB, KK>(accA, accB, in, lds, lds + IMG_A, lane);
  st_store<NA>(accA, y, row, M, 32 * (NA + NB), 0, h);
  st_store<NB>(accB, y, row, M, 32 * (NA + NB), 32 * NA, h);
}

// the segment chains of the appearance kernels' first layer (four output blocks): mfma_seg_b3s<4, KA, KB> -> <4, KB, KC> ->
// <4, KC, 64> (k_dyn_app; its last segment requests step 0 of the NEXT layer, here: of the chain's own first image), or
// <4, KA, KB> -> <4, KB, 0> with KC = 0 (k_static_app).  hi + mid images in LDS, the lo stream in global memory behind them.
template <int KA, int KB, int KC>
__global__ __launch_bounds__(64) void k_st_b3s_chain(const float* __restrict__ x, const float* __restrict__ pkw, int M,
                                                     float* __restrict__ y) {
  constexpr int KT = KA + KB + KC, IMG = 4 * KT * 64;
  constexpr int LO_A = 0, LO_B = 4 * KA * 32, LO_C = LO_B + 4 * KB * 32;
  __shared__ __attribute__((aligned(16))) float lds[IMG];
  lds_fill(lds, pkw, IMG);
  const int lane = threadIdx.x & 63, h = lane >> 5, row = blockIdx.x * 32 + (lane & 31);
  float A[KA], B[KB];
  st_load<KA>(A, x, row, M, 2 * KT, 0, h);
  st_load<KB>(B, x, row, M, 2 * KT, 2 * KA, h);
  f32x16 acc[4];
  acc_bias<4>(acc, nullptr, h);
  const B3sLo st = b3s_lo_stream(pkw + IMG, lane);
  u32x4 lo[4];
  b3s_lo_load<4>(lo, st, LO_A, KA / 8, 0);
  if constexpr (KC > 0) {
    float Cc[KC > 0 ? KC : 8];
    st_load<KC>(Cc, x, row, M, 2 * KT, 2 * (KA + KB), h);
    mfma_seg_b3s<4, KA, KB>(acc, A, lds, st, LO_A, LO_B, lo, lane);
    mfma_seg_b3s<4, KB, KC>(acc, B, lds + 4 * KA * 64, st, LO_B, LO_C, lo, lane);
    mfma_seg_b3s<4, KC, 64>(acc, Cc, lds + 4 * (KA + KB) * 64, st, LO_C, LO_A, lo, lane);
  } else {
    mfma_seg_b3s<4, KA, KB>(acc, A, lds, st, LO_A, LO_B, lo, lane);
    mfma_seg_b3s<4, KB, 0>(acc, B, lds + 4 * KA * 64, st, LO_B, 0, lo, lane);
  }
  st_store<4>(acc, y, row, M, 128, 0, h);
}

// mfma_seg_b3s<NBI, KK, 0> as app_bwd_seg (rdrf_bwd.hip) calls it: the lo pieces of step 0 are requested right before
template <int NBI, int KK>
__global__ __launch_bounds__(64) void k_st_b3s_t(const float* __restrict__ x, const float* __restrict__ pkw, int M,
                                                 float* __restrict__ y) {
  constexpr int IMG = NBI * KK * 64;
  __shared__ __attribute__((aligned(16))) float lds[IMG];
  lds_fill(lds, pkw, IMG);
  const int lane = threadIdx.x & 63, h = lane >> 5, row = blockIdx.x * 32 + (lane & 31);
  float dz[KK];
  st_load<KK>(dz, x, row, M, 2 * KK, 0, h);
  f32x16 acc[NBI];
  acc_bias<NBI>(acc, nullptr, h);
  const B3sLo st = b3s_lo_stream(pkw + IMG, lane);
  u32x4 lo[NBI];
  b3s_lo_load<NBI>(lo, st, 0, KK / 8, 0);
  mfma_seg_b3s<NBI, KK, 0>(acc, dz, lds, st, 0, 0, lo, lane);
  st_store<NBI>(acc, y, row, M, 32 * NBI, 0, h);
}

}  // namespace

#define ST_RUN(floats, kernel)                                                                                       \
  do {                                                                                                               \
    RDRF_CHECK(ws_bytes >= (size_t)(floats) * sizeof(float), -3, "selftest_layer: workspace too small (%zu < %zu)",  \
               ws_bytes, (size_t)(floats) * sizeof(float));                                                          \
    int rc_ = pack_launch(J, (float*)ws, stream);                                                                    \
    if (rc_) return rc_;                                                                                             \
    RDRF_LAUNCH("selftest_layer", kernel, dim3((M + 31) / 32), dim3(64), stream, x, (const float*)ws, M, y);         \
    return 0;                                                                                                        \
  } while (0)

extern "C" int rdrf_selftest_layer(int form, const float* x, const float* w, int M, int K, int OUT, float* y, void* ws,
                                   size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(form >= RDRF_ST_F32 && form <= RDRF_ST_B3S_T, -1, "selftest_layer: unknown form %d", form);
  if (M == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(x && w && y && ws && M > 0, -1, "selftest_layer: bad arguments");
  RDRF_CHECK(((size_t)ws & 15) == 0, -1, "selftest_layer: the workspace must be 16-byte aligned");
  PackJobs J;
  J.n = 0;
  switch (form) {
    case RDRF_ST_F32:   // mfma_seg<NBO, KK>, pack mode 0: K = 2 KK, OUT = 32 NBO
      if (K == 64 && OUT == 64) { pack_add(J, w, 64, 64, 64, SEG_IDENT, 0, 2, 32, 0); ST_RUN(2 * 32 * 64, (k_st_f32<2, 32>)); }
      if (K == 128 && OUT == 128) { pack_add(J, w, 128, 128, 128, SEG_IDENT, 0, 4, 64, 0); ST_RUN(4 * 64 * 64, (k_st_f32<4, 64>)); }
      if (K == 72 && OUT == 32) { pack_add(J, w, 72, 32, 72, SEG_IDENT, 0, 1, 36, 0); ST_RUN(1 * 36 * 64, (k_st_f32<1, 36>)); }
      break;
    case RDRF_ST_F32_T:   // mfma_seg<NBI, KK>, pack mode 2: OUT = 2 KK, K = 32 NBI
      if (K == 64 && OUT == 64) { pack_add(J, w, 64, 64, 64, SEG_IDENT, 2, 2, 32, 0); ST_RUN(2 * 32 * 64, (k_st_f32<2, 32>)); }
      if (K == 32 && OUT == 128) { pack_add(J, w, 32, 128, 32, SEG_IDENT, 2, 1, 64, 0); ST_RUN(1 * 64 * 64, (k_st_f32<1, 64>)); }
      break;
    case RDRF_ST_B3:   // mfma_seg_b3<NBO, KK>, pack mode 7
      if (K == 2 * pk::K1_HEAD_KK && OUT == 64) {   // the heads' first layer: one image from three segments (36 | 32 | 4 slots)
        pack_add_b3(J, w, K, 64, 72, SEG_IDENT, 2, 36, 0, 0, pk::K1_HEAD_KK, 0);
        pack_add_b3(J, w + 72, K, 64, 64, SEG_IDENT, 2, 32, 0, 36, pk::K1_HEAD_KK, 0);
        pack_add_b3(J, w + 136, K, 64, 8, SEG_IDENT, 2, 4, 0, 68, pk::K1_HEAD_KK, 0);
        ST_RUN(2 * pk::K1_HEAD_KK * 96, (k_st_b3<2, pk::K1_HEAD_KK>));
      }
      if (K == 64 && OUT == 64) { pack_add_b3(J, w, 64, 64, 64, SEG_IDENT, 2, 32, 0, 0, 32, 0); ST_RUN(2 * 32 * 96, (k_st_b3<2, 32>)); }
      break;
    case RDRF_ST_B3_T:   // mfma_seg_b3<NBI, KK>, pack mode 8
      if (K == 64 && OUT == 64) { pack_add(J, w, 64, 64, 64, SEG_IDENT, 8, 2, 32, 0); ST_RUN(2 * 32 * 96, (k_st_b3<2, 32>)); }
      break;
    case RDRF_ST_B3_PAIR_T:   // mfma_seg_b3_pair<NA, NB, 32>, pack mode 8: image A = input columns 0 .. 32 NA - 1, B = the rest
      if (K == 160 && OUT == 64) {
        pack_add(J, w, 160, 64, 96, SEG_IDENT, 8, 3, 32, 0);
        pack_add(J, w + 96, 160, 64, 64, SEG_IDENT, 8, 2, 32, 3 * 32 * 96);
        ST_RUN(5 * 32 * 96, (k_st_b3_pair<3, 2, 32>));
      }
      if (K == 96 && OUT == 64) {
        pack_add(J, w, 96, 64, 64, SEG_IDENT, 8, 2, 32, 0);
        pack_add(J, w + 64, 96, 64, 32, SEG_IDENT, 8, 1, 32, 2 * 32 * 96);
        ST_RUN(3 * 32 * 96, (k_st_b3_pair<2, 1, 32>));
      }
      break;
    case RDRF_ST_B3S:   // mfma_seg_b3s chains, pack mode 9: one job per segment, lo images behind the hi + mid images
      if (K == 112 && OUT == 128) {   // k_dyn_app: 16 | 32 | 8 slots
        constexpr int IMG = 4 * 56 * 64;
        pack_add_b3s(J, w, 112, 128, 32, SEG_IDENT, 4, 16, 0, 0, 16, 0, IMG);
        pack_add_b3s(J, w + 32, 112, 128, 64, SEG_IDENT, 4, 32, 0, 0, 32, 4 * 16 * 64, IMG + 4 * 16 * 32);
        pack_add_b3s(J, w + 96, 112, 128, 16, SEG_IDENT, 4, 8, 0, 0, 8, 4 * 48 * 64, IMG + 4 * 48 * 32);
        ST_RUN(IMG + 4 * 56 * 32, (k_st_b3s_chain<16, 32, 8>));
      }
      if (K == 160 && OUT == 128) {   // k_static_app: 16 | 64 slots
        constexpr int IMG = 4 * 80 * 64;
        pack_add_b3s(J, w, 160, 128, 32, SEG_IDENT, 4, 16, 0, 0, 16, 0, IMG);
        pack_add_b3s(J, w + 32, 160, 128, 128, SEG_IDENT, 4, 64, 0, 0, 64, 4 * 16 * 64, IMG + 4 * 16 * 32);
        ST_RUN(IMG + 4 * 80 * 32, (k_st_b3s_chain<16, 64, 0>));
      }
      break;
    case RDRF_ST_B3S_T: {   // mfma_seg_b3s<NBI, KK, 0>, pack mode 10: OUT = 2 KK, K = 32 NBI
      const int nbi = K / 32, kk = OUT / 2;
      const bool known = K % 32 == 0 && ((OUT == 32 && (nbi == 7 || nbi == 3)) || (OUT == 128 && (nbi == 4 || nbi == 3 || nbi == 5)));
      if (!known) break;
      const int img = nbi * kk * 64;
      if (OUT == 128 && nbi != 4) {   // the first layers' images: one block (features), then the rest, as rdrf_bwd.hip packs them
        pack_add_b3s_t(J, w, K, OUT, 32, SEG_IDENT, 1, kk, 0, img);
        pack_add_b3s_t(J, w + 32, K, OUT, K - 32, SEG_IDENT, nbi - 1, kk, kk * 64, img + kk * 32);
      } else {
        pack_add_b3s_t(J, w, K, OUT, K, SEG_IDENT, nbi, kk, 0, img);
      }
      if (OUT == 32 && nbi == 7) ST_RUN(img + nbi * kk * 32, (k_st_b3s_t<7, 16>));
      if (OUT == 32 && nbi == 3) ST_RUN(img + nbi * kk * 32, (k_st_b3s_t<3, 16>));
      if (OUT == 128 && nbi == 4) ST_RUN(img + nbi * kk * 32, (k_st_b3s_t<4, 64>));
      if (OUT == 128 && nbi == 3) ST_RUN(img + nbi * kk * 32, (k_st_b3s_t<3, 64>));
      if (OUT == 128 && nbi == 5) ST_RUN(img + nbi * kk * 32, (k_st_b3s_t<5, 64>));
      break;
    }
  }
  rdrf_set_error("selftest_layer: form %d is not instantiated for K = %d, OUT = %d", form, K, OUT);
  return -1;
}

// ------------------------------------------------------------------------------------------------
// rdrf_selftest_dw: the product's dW job lists on caller-supplied rows.  A plan is one DwJobs list as an entry point of
// rdrf_bwd.hip hands it to dw_launch.  Its jobs fall into one or two row regions (a region = one dz array and one activation
// array with their strides: what dw_launch plans together); region g + 1 starts where region g ends, ntiles tiles on.
// ------------------------------------------------------------------------------------------------
namespace {

struct DwPlanInfo {
  int dynamic;                          // the gradient struct is RdrfDynamicParams / RdrfStaticParams
  int region[RDRF_MAX_DW_JOBS];         // region of each job
  int nregions;
};

int dw_plan_jobs(int plan, int flags, const float* A, const float* B, size_t ntiles, const int* count, const void* G, DwJobs& D,
                 DwPlanInfo& I) {
  const RdrfStaticParams* Gs = (const RdrfStaticParams*)G;
  const RdrfDynamicParams* Gd = (const RdrfDynamicParams*)G;
  const bool live_d = (flags & RDRF_DW_LIVE_D) != 0, live_b = (flags & RDRF_DW_LIVE_B) != 0, small = (flags & RDRF_DW_SMALL_IN_KERNEL) != 0,
             warp = (flags & RDRF_DW_WARP_IN_KERNEL) != 0;
  const int T = (int)ntiles, Tc = count ? 0 : T;   // a compacted phase passes (count, 0) in the product
  D.n = 0;
  I.dynamic = 1;
  int n0 = -1;   // first job of the second region
  const float *A1 = nullptr, *B1 = nullptr;
  auto second = [&]() {
    n0 = D.n;
    A1 = A + ntiles * (size_t)D.j[0].A_stride * 32;
    B1 = B + ntiles * (size_t)D.j[0].B_stride * 32;
  };
  switch (plan) {
    case RDRF_DW_DENSITY: add_density_phase_dw(D, A, B, Gd, T, live_d, live_b, small, warp); break;
    case RDRF_DW_STATIC_FEA: I.dynamic = 0; add_static_app_dw(D, A, B, Gs, true, count, Tc); break;
    case RDRF_DW_STATIC_TE: I.dynamic = 0; add_static_app_dw(D, A, B, Gs, false, count, Tc); break;
    case RDRF_DW_DYN_APP: add_dyn_app_dw(D, A, B, Gd, count, Tc); break;
    case RDRF_DW_DYN:   // rdrf_dynamic_bwd: appearance + density phase in one list
      add_dyn_app_dw(D, A, B, Gd, count, Tc);
      second();
      add_density_phase_dw(D, A1, B1, Gd, T, live_d, live_b, small, warp);
      break;
    case RDRF_DW_SCENE_FLOW: add_scene_flow_dw(D, A, B, Gd, T); break;
    case RDRF_DW_FEAT_STATIC: I.dynamic = 0; add_feat_static_dw(D, A, B, Gs, T); break;
    case RDRF_DW_FEAT_DYN:   // rdrf_dynamic_features_bwd
      add_feat_dyn_app_dw(D, A, B, Gd, T);
      second();
      add_density_phase_dw(D, A1, B1, Gd, T, live_d, live_b);
      break;
    default: rdrf_set_error("selftest_dw: unknown plan %d", plan); return -1;
  }
  I.nregions = n0 < 0 ? 1 : 2;
  for (int j = 0; j < D.n; ++j) I.region[j] = (n0 >= 0 && j >= n0) ? 1 : 0;
  return 0;
}

}  // namespace

extern "C" int rdrf_selftest_dw(int plan, int flags, const float* A, size_t A_floats, const float* B, size_t B_floats, int ntiles,
                                const int* count, const void* grads, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DwJobs D;
  DwPlanInfo I;
  RDRF_CHECK(plan >= RDRF_DW_DENSITY && plan <= RDRF_DW_FEAT_DYN, -1, "selftest_dw: unknown plan %d", plan);
  RDRF_CHECK(ntiles >= 0, -1, "selftest_dw: bad arguments (ntiles < 0)");
  const bool takes_count = plan >= RDRF_DW_STATIC_FEA && plan <= RDRF_DW_DYN;   // the plans with a compacted phase
  if (!takes_count) count = nullptr;                                           // the others never read it
  if (ntiles == 0 && count == nullptr) return 0;   // no tile: a no-op
  RDRF_CHECK(A && B && grads, -1, "selftest_dw: bad arguments (null rows or gradient struct)");
  RDRF_CHECK((((uintptr_t)A | (uintptr_t)B) & 15) == 0, -1, "selftest_dw: the rows must be 16-byte aligned");
  int rc = dw_plan_jobs(plan, flags, A, B, (size_t)ntiles, count, grads, D, I);
  if (rc) return rc;
  size_t needA = 0, needB = 0;
  for (int g = 0, j = 0; g < I.nregions; ++g) {
    while (j < D.n && I.region[j] != g) ++j;
    needA += (size_t)ntiles * D.j[j].A_stride * 32;
    needB += (size_t)ntiles * D.j[j].B_stride * 32;
  }
  RDRF_CHECK(A_floats >= needA && B_floats >= needB, -3, "selftest_dw: rows too small (A %zu < %zu or B %zu < %zu floats)", A_floats,
             needA, B_floats, needB);
  bool uses_count = false;
  for (int j = 0; j < D.n; ++j) uses_count |= D.j[j].count != nullptr;
  if (uses_count) {   // the kernel walks ceil(count / 32) tiles: they must lie inside the rows
    int c = -1;
    RDRF_HIP(hipMemcpyAsync(&c, count, sizeof(int), hipMemcpyDeviceToHost, stream));
    RDRF_HIP(hipStreamSynchronize(stream));
    RDRF_CHECK(c >= 0 && ((size_t)c + 31) / 32 <= (size_t)ntiles, -1, "selftest_dw: count %d does not fit %d tiles", c, ntiles);
  }
  return dw_launch(D, stream, "selftest_dw");
}

// The job list of a plan in resolved form (host memory, ints), so that a reference needs no knowledge of the row layouts or the
// segment maps:  [0] ints used, [1] regions, [2] jobs, [3] 1 = RdrfDynamicParams / 0 = RdrfStaticParams;
// per region: A_stride, B_stride, 1 if its jobs take the device count;
// per job: region, A_row0, nbo, out_dim, out_row0, in_dim, ld, byte offset of the dW pointer in the gradient struct, of the db
// pointer (-1: none), number of input blocks; per block: row0 and the 32 columns seg_imap(seg, e0 + li, in_dim) (-1: none).
extern "C" int rdrf_selftest_dw_describe(int plan, int flags, int* out, int cap) {
  constexpr size_t NSLOT = (sizeof(RdrfDynamicParams) > sizeof(RdrfStaticParams) ? sizeof(RdrfDynamicParams) : sizeof(RdrfStaticParams)) / 8;
  uintptr_t slots[NSLOT];   // a gradient struct whose pointer fields hold their own byte offset + 8
  for (size_t i = 0; i < NSLOT; ++i) slots[i] = (i + 1) * 8;
  alignas(16) static const float rowsA[4] = {0.f}, rowsB[4] = {0.f};   // addresses only: never read
  static const int cnt = 0;
  DwJobs D;
  DwPlanInfo I;
  int rc = dw_plan_jobs(plan, flags, rowsA, rowsB, 1, &cnt, slots, D, I);
  if (rc) return rc;
  int need = 4 + 3 * I.nregions;
  for (int j = 0; j < D.n; ++j) need += 10 + 33 * D.j[j].nblk;
  RDRF_CHECK(out != nullptr && cap >= need, -3, "selftest_dw_describe: description buffer too small (%d < %d ints)", out ? cap : 0, need);
  int n = 0;
  out[n++] = need; out[n++] = I.nregions; out[n++] = D.n; out[n++] = I.dynamic;
  for (int g = 0, j = 0; g < I.nregions; ++g) {
    while (j < D.n && I.region[j] != g) ++j;
    out[n++] = D.j[j].A_stride; out[n++] = D.j[j].B_stride; out[n++] = D.j[j].count != nullptr ? 1 : 0;
  }
  for (int j = 0; j < D.n; ++j) {
    const DwJob& J = D.j[j];
    out[n++] = I.region[j]; out[n++] = J.A_row0; out[n++] = J.nbo; out[n++] = J.out_dim; out[n++] = J.out_row0;
    out[n++] = J.in_dim; out[n++] = J.ld;
    out[n++] = (int)((uintptr_t)J.dW - 8);
    out[n++] = J.db != nullptr ? (int)((uintptr_t)J.db - 8) : -1;
    out[n++] = J.nblk;
    for (int k = 0; k < J.nblk; ++k) {
      out[n++] = J.blk_row0[k];
      for (int li = 0; li < 32; ++li) out[n++] = seg_imap(J.blk_seg[k], J.blk_e0[k] + li, J.in_dim);
    }
  }
  return n;
}

// The launches dw_launch makes for a plan at ntiles tiles (host memory, ints; host code only, no HIP call):
// [0] ints used, [1] launches; per launch: workgroups, dynamic LDS bytes, accumulator sets of the k_dw3 instantiation, staged
// blocks, runs; per run: source (0 dz rows, 1 activation rows), first row, first staged block; per staged block: source, first
// row; per wave (12): its number of products, and per product the staged block indices of its dz and its input block, then the
// job, the out block and the input block of the job that it forms.  The plans with a compacted phase are planned with a device
// count, as their entry points pass one.
extern "C" int rdrf_selftest_dw_plan(int plan, int flags, int ntiles, int* out, int cap) {
  constexpr size_t NSLOT = (sizeof(RdrfDynamicParams) > sizeof(RdrfStaticParams) ? sizeof(RdrfDynamicParams) : sizeof(RdrfStaticParams)) / 8;
  uintptr_t slots[NSLOT];   // as in rdrf_selftest_dw_describe: only "is there a bias" is read of the gradient struct
  for (size_t i = 0; i < NSLOT; ++i) slots[i] = (i + 1) * 8;
  alignas(16) static const float rowsA[4] = {0.f}, rowsB[4] = {0.f};   // addresses only: never read
  static const int cnt = 0;
  RDRF_CHECK(ntiles >= 1 && ntiles <= (1 << 20), -1, "selftest_dw_plan: bad arguments (ntiles = %d)", ntiles);
  DwJobs D;
  DwPlanInfo I;
  int rc = dw_plan_jobs(plan, flags, rowsA, rowsB, 0, &cnt, slots, D, I);   // (both regions at the same address: they differ in stride)
  if (rc) return rc;
  for (int j = 0; j < D.n; ++j)
    if (D.j[j].count == nullptr) D.j[j].ntiles = ntiles;
  return dw_describe_launches(D, out, cap);
}

extern "C" int rdrf_selftest_sf_geometry(int ntiles, int* grid, int* waves) {
  RDRF_CHECK(ntiles >= 0 && grid && waves, -1, "selftest_sf_geometry: bad arguments");
  fused_dw_geometry(ntiles, grid, waves);
  return 0;
}

extern "C" int rdrf_selftest_warp_geometry(int ntiles, int* grid, int* waves) {
  RDRF_CHECK(ntiles >= 0 && grid && waves, -1, "selftest_warp_geometry: bad arguments");
  fused_dw_geometry(ntiles, grid, waves);
  return 0;
}

static void carve_warp_bwd(float*& pk, uint8_t*& valid, WsCarver& c, int N, int S) {
  pk = c.take<float>(PACK_AREA_FLOATS);
  valid = c.take<uint8_t>((size_t)N * S);
}
extern "C" size_t rdrf_selftest_warp_bwd_workspace_bytes(int N, int S) {
  float* pk;
  uint8_t* valid;
  WsCarver c;
  carve_warp_bwd(pk, valid, c, N, S);
  return c.off;
}
extern "C" int rdrf_selftest_warp_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, int N, int S, const float* act1,
                                      size_t act1_floats, float* grows1, size_t grows1_floats, float* dxw, float* dxn,
                                      const float* g_xyz_prime, const RdrfDynamicParams* grads, float* g_xyz, float* dtout,
                                      float* dtp, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(P && cfg && grads && act1 && grows1 && dxw && dxn && dtout && dtp && ws && N > 0 && S > 0 && S <= 4096, -1,
             "selftest_warp_bwd: bad arguments");
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "selftest_warp_bwd: N * S * 3 must stay below 2^31");
  RDRF_CHECK((((uintptr_t)act1 | (uintptr_t)grows1 | (uintptr_t)ws) & 15) == 0, -1, "selftest_warp_bwd: rows and workspace must be 16-byte aligned");
  const size_t tiles = ((size_t)N * S + 31) / 32;
  RDRF_CHECK(act1_floats >= tiles * sv::K1_ROWS * 32 && grows1_floats >= tiles * sv::K1G_ROWS * 32, -3,
             "selftest_warp_bwd: rows too small for %zu tiles", tiles);
  WsCarver c(ws, ws_bytes);
  float* pk;
  uint8_t* valid;
  carve_warp_bwd(pk, valid, c, N, S);
  RDRF_CHECK(c.ok(), -3, "selftest_warp_bwd: workspace too small");
  return warp_bwd_on_rows(P, cfg, N, S, act1, grows1, dxw, dxn, g_xyz_prime, grads, g_xyz, dtout, dtp, pk, valid, stream);
}

// ------------------------------------------------------------------------------------------------
// rdrf_selftest_sort: rdrf_sort_positions on caller-owned arrays
// ------------------------------------------------------------------------------------------------
extern "C" size_t rdrf_selftest_sort_temp_bytes(unsigned n, int bits) { return rdrf_sort_temp_bytes(n, bits); }

extern "C" int rdrf_selftest_sort(const unsigned* keys, unsigned n, int bits, const int* count, unsigned n_mul, unsigned* keys_out,
                                  unsigned* order, void* temp, size_t temp_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(bits >= 1 && bits <= 32, -1, "selftest_sort: bits must be 1 .. 32 (got %d)", bits);
  if (n == 0) return 0;   // nothing to sort: a no-op
  RDRF_CHECK(keys && keys_out && order, -1, "selftest_sort: bad arguments (null keys, keys_out or order)");
  RDRF_CHECK(count == nullptr || n_mul >= 1, -1, "selftest_sort: a device count needs n_mul >= 1");
  RDRF_CHECK(temp != nullptr && (((uintptr_t)temp) & 255) == 0, -1, "selftest_sort: the temporary storage must be 256-byte aligned");
  if (count) {   // n_mul * count is formed in 32 bits on the device
    int c = -1;
    RDRF_HIP(hipMemcpyAsync(&c, count, sizeof(int), hipMemcpyDeviceToHost, stream));
    RDRF_HIP(hipStreamSynchronize(stream));
    RDRF_CHECK(c >= 0 && (unsigned long long)c * n_mul <= 0xffffffffull, -1, "selftest_sort: device count %d out of range", c);
  }
  return rdrf_sort_positions(keys, keys_out, order, n, bits, temp, temp_bytes, stream, count, count ? n_mul : 0u);
}

// rdrf_selftest_sort_seg: rdrf_sort_positions_seg on caller-owned arrays (nseg segments of seg_len entries, or of *count with a
// device count; the sort builds its own first histograms here, as rdrf_selftest_sort does)
extern "C" size_t rdrf_selftest_sort_seg_temp_bytes(int nseg, unsigned seg_len, int bits) {
  return rdrf_sort_seg_temp_bytes(nseg, seg_len, bits);
}

extern "C" int rdrf_selftest_sort_seg(const unsigned* keys, int nseg, unsigned seg_len, int bits, const int* count, unsigned* keys_out,
                                      unsigned* order, void* temp, size_t temp_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(bits >= 1 && bits <= 32, -1, "selftest_sort_seg: bits must be 1 .. 32 (got %d)", bits);
  RDRF_CHECK(nseg >= 1 && (unsigned long long)nseg * seg_len <= 0xffffffffull, -1, "selftest_sort_seg: bad segments (%d x %u)", nseg, seg_len);
  if (seg_len == 0) return 0;   // nothing to sort: a no-op
  RDRF_CHECK(keys && keys_out && order, -1, "selftest_sort_seg: bad arguments (null keys, keys_out or order)");
  RDRF_CHECK(temp != nullptr && (((uintptr_t)temp) & 255) == 0, -1, "selftest_sort_seg: the temporary storage must be 256-byte aligned");
  if (count) {
    int c = -1;
    RDRF_HIP(hipMemcpyAsync(&c, count, sizeof(int), hipMemcpyDeviceToHost, stream));
    RDRF_HIP(hipStreamSynchronize(stream));
    RDRF_CHECK(c >= 0, -1, "selftest_sort_seg: device count %d out of range", c);
  }
  return rdrf_sort_positions_seg(keys, keys_out, order, nseg, seg_len, bits, temp, temp_bytes, stream, count, nullptr);
}

// The sort's plan in resolved form (host only): [0] values used, [1] passes, [2] bits per digit, [3] tiles per segment, [4] entries
// per tile, [5] bytes the sort carves out of its temporary storage, [6] rdrf_selftest_sort_seg_temp_bytes, [7] launches of a sort
// that builds its own first histograms, [8] launches of a sorted-scatter call (key kernel + sort, first histograms by the key kernel)
extern "C" int rdrf_selftest_sort_describe(int nseg, unsigned seg_len, int bits, unsigned long long* out, int cap) {
  RDRF_CHECK(bits >= 1 && bits <= 32 && nseg >= 1, -1, "selftest_sort_describe: bad arguments (bits %d, segments %d)", bits, nseg);
  RDRF_CHECK(out != nullptr && cap >= 9, -3, "selftest_sort_describe: room for 9 values needed");
  int passes, db;
  rdrf_sort_plan(bits, &passes, &db);
  out[0] = 9; out[1] = (unsigned long long)passes; out[2] = (unsigned long long)db;
  out[3] = ((unsigned long long)seg_len + RS_TILE - 1) / RS_TILE; out[4] = RS_TILE;
  out[5] = rdrf_sort_carved_bytes(nseg, seg_len); out[6] = rdrf_sort_seg_temp_bytes(nseg, seg_len, bits);
  out[7] = 3ull * passes; out[8] = 3ull * passes;   // (key kernel + (3 passes - the first histogram))
  return 9;
}

// ------------------------------------------------------------------------------------------------
// rdrf_selftest_scatter: the four instantiations of the scatter in use, with the arguments their backward entry points give
// them (rdrf_bwd.hip), through launch_scatter (ray tiles) or scatter_dyn_*_sorted (key generation, sort and counts, sorted /
// tiled passes).
// ------------------------------------------------------------------------------------------------
namespace {

struct ScatterKindInfo {
  int c0q, c1q, nlv;       // quads of an XY / XZ-YZ texel, stride levels
  int nsets;               // factor sets a launch can carry
  int stride, row0[2];     // ray tiles: rows per tile, first d(feature) row of each set
  int bcast;
  int rec_floats, set_floats;   // sorted: floats per record / per set inside it (0: the kind has no sorted form)
  int live_row[2];         // sorted key generation: the two rows whose zero marks a dead sample (-1: none)
  int list, xw;            // compacted list + device count; normalised coordinates (else xyz + box)
  int dxw_ray, dxw_sorted; // coordinate gradients: 0 none, 1 written, 2 added
  int g_xyz, flat;         // g_xyz += dw * inv; the tiles may be flat 32-sample tiles
  ScatterKernel kern;
};

bool scatter_kind_info(int kind, ScatterKindInfo& k) {
  switch (kind) {
    case RDRF_SCK_STATIC_DENSITY:
      k = ScatterKindInfo{4, 1, 1, 1, 1, {0, -1}, 1, 0, 0, {-1, -1}, 0, 0, 0, 0, 1, 0, SCATTER_4_1_3};
      return true;
    case RDRF_SCK_DYN_DENSITY:
      k = ScatterKindInfo{4, 1, 3, 2, sv::K1G_ROWS, {sv::K1G_DFD, sv::K1G_DFB}, 0, DFS_FLOATS, DFS_FLOATS / 2,
                          {sv::K1G_SM + 3, sv::K1G_SM + 4}, 0, 1, 2, 2, 0, 1, SCATTER_4_1_9};
      return true;
    case RDRF_SCK_STATIC_APP:
      k = ScatterKindInfo{12, 3, 1, 1, sv::K3G_ROWS, {sv::K3G_DA, -1}, 0, 0, 0, {-1, -1}, 1, 0, 0, 0, 1, 0, SCATTER_12_3_9};
      return true;
    case RDRF_SCK_DYN_APP:
      k = ScatterKindInfo{12, 3, 3, 1, sv::K3G_ROWS, {sv::K3G_DA, -1}, 0, DFA_FLOATS, DFA_FLOATS, {-1, -1}, 1, 1, 1, 2, 0, 0,
                          SCATTER_12_3_27};
      return true;
  }
  return false;
}

bool scatter_vm_ok(const RdrfVM& v, const RdrfVM& g, int c0, int c1) {
  if (!vm_ok(v, c0, c1)) return false;
  for (int i = 0; i < 3; ++i) {
    if (v.W[i] < 2 || v.H[i] < 2 || v.L[i] < 2 || !v.plane[i] || !v.line[i] || !g.plane[i] || !g.line[i]) return false;
    if (g.C[i] != v.C[i] || g.W[i] != v.W[i] || g.H[i] != v.H[i] || g.L[i] != v.L[i] || g.sH[i] != v.sH[i] || g.sW[i] != v.sW[i])
      return false;
    const bool w_fast = v.sW[i] == v.C[i] && v.sH[i] == v.W[i] * v.C[i], h_fast = v.sH[i] == v.C[i] && v.sW[i] == v.H[i] * v.C[i];
    if (!w_fast && !h_fast) return false;   // the two storage orders of a plane: the arrays hold H W C floats
    if ((((uintptr_t)v.plane[i] | (uintptr_t)v.line[i] | (uintptr_t)g.plane[i] | (uintptr_t)g.line[i]) & 15) != 0) return false;
  }
  return true;
}

}  // namespace

extern "C" size_t rdrf_selftest_scatter_workspace_bytes(int N, int S) {   // of the sorted forms (carve_sorted_scatter)
  BwdWs b;
  WsCarver c;
  carve_sorted_scatter(b, c, (size_t)(N > 0 ? N : 0) * (size_t)(S > 0 ? S : 0));
  return c.off;
}

extern "C" int rdrf_selftest_scatter(int kind, int mode, const RdrfScatterTest* t, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ScatterKindInfo k;
  RDRF_CHECK(scatter_kind_info(kind, k), -1, "selftest_scatter: unknown kind %d", kind);
  RDRF_CHECK(mode == RDRF_SCATTER_RAY || mode == RDRF_SCATTER_SORTED || mode == RDRF_SCATTER_SORTED_PLAIN, -1,
             "selftest_scatter: mode must be RDRF_SCATTER_RAY, _SORTED or _SORTED_PLAIN (got %d)", mode);
  const bool sorted = mode != RDRF_SCATTER_RAY;
  RDRF_CHECK(!sorted || k.rec_floats > 0, -2, "selftest_scatter: kind %d has no sorted form", kind);
  RDRF_CHECK(t != nullptr, -1, "selftest_scatter: bad arguments (null description)");
  if (t->N == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(t->N > 0 && t->S > 0 && t->S <= 4096 && (size_t)t->N * t->S * 3 < (size_t)INT32_MAX / 4, -1,
             "selftest_scatter: bad batch shape %d x %d", t->N, t->S);
  const int N = t->N, S = t->S;
  const size_t ns = (size_t)N * S;
  const int flat = t->flat != 0;
  RDRF_CHECK(!flat || k.flat, -2, "selftest_scatter: kind %d has no flat tiles", kind);
  // the sorted density / blending passes address the liveness rows the way the process-wide density phase does
  RDRF_CHECK(!(sorted && kind == RDRF_SCK_DYN_DENSITY) || flat == (rdrf_flat_density() ? 1 : 0), -2,
             "selftest_scatter: the sorted density scatter of this build runs on %s tiles", rdrf_flat_density() ? "flat" : "ray");
  const int set_mask = k.nsets == 2 ? t->set_mask : 1;
  RDRF_CHECK(set_mask >= 1 && set_mask <= 3, -1, "selftest_scatter: set mask must be 1, 2 or 3 (got %d)", t->set_mask);
  for (int set = 0; set < k.nsets; ++set)
    RDRF_CHECK(scatter_vm_ok(t->vm[set], t->gvm[set], 16 * k.c0q / 4, 4 * k.c1q), -1,
               "selftest_scatter: factor set %d: component counts, one grid, W-fastest or H-fastest planes matching the gradient "
               "buffers, 16-byte aligned", set);
  RDRF_CHECK(k.nsets == 1 || vm_same_grid(t->vm[0], t->vm[1]), -1, "selftest_scatter: the two factor sets differ in size");
  RDRF_CHECK(t->coords != nullptr, -1, "selftest_scatter: bad arguments (null coordinates)");
  RDRF_CHECK(k.list || t->valid != nullptr, -1, "selftest_scatter: bad arguments (null valid)");
  RDRF_CHECK(!k.list || (t->list != nullptr && t->count != nullptr), -1, "selftest_scatter: kind %d takes a list and a device count", kind);
  RDRF_CHECK(!(sorted ? k.dxw_sorted : k.dxw_ray) || t->dxw != nullptr, -1, "selftest_scatter: bad arguments (null dxw)");
  RDRF_CHECK(!k.g_xyz || t->g_xyz != nullptr, -1, "selftest_scatter: bad arguments (null g_xyz)");
  const size_t tpr = ((size_t)S + 31) / 32, t3 = (ns + 31) / 32, ntiles = k.list || flat ? t3 : (size_t)N * tpr;
  const bool needs_rows = !sorted || k.live_row[0] >= 0;
  if (needs_rows) {
    RDRF_CHECK(t->rows != nullptr && ((uintptr_t)t->rows & 15) == 0, -1, "selftest_scatter: the rows must be 16-byte aligned");
    RDRF_CHECK(t->rows_floats >= ntiles * (size_t)k.stride * 32, -3, "selftest_scatter: rows too small (%zu < %zu floats)",
               t->rows_floats, ntiles * (size_t)k.stride * 32);
  }
  if (sorted) {
    RDRF_CHECK(t->recs != nullptr && ((uintptr_t)t->recs & 15) == 0, -1, "selftest_scatter: the records must be 16-byte aligned");
    RDRF_CHECK(t->recs_floats >= ns * (size_t)k.rec_floats, -3, "selftest_scatter: records too small (%zu < %zu floats)",
               t->recs_floats, ns * (size_t)k.rec_floats);
    RDRF_CHECK(t->ws != nullptr && ((uintptr_t)t->ws & 255) == 0, -1, "selftest_scatter: the workspace must be 256-byte aligned");
    RDRF_CHECK(t->ws_bytes >= rdrf_selftest_scatter_workspace_bytes(N, S), -3, "selftest_scatter: workspace too small (%zu < %zu)",
               t->ws_bytes, rdrf_selftest_scatter_workspace_bytes(N, S));
  }
  if (k.list) {   // the kernels index the batch with the list entries: they must lie inside it
    int c = -1;
    RDRF_HIP(hipMemcpyAsync(&c, t->count, sizeof(int), hipMemcpyDeviceToHost, stream));
    RDRF_HIP(hipStreamSynchronize(stream));
    RDRF_CHECK(c >= 0 && (size_t)c <= ns, -1, "selftest_scatter: count %d does not fit %zu samples", c, ns);
    std::vector<int> host((size_t)c);
    if (c > 0) {
      RDRF_HIP(hipMemcpyAsync(host.data(), t->list, (size_t)c * sizeof(int), hipMemcpyDeviceToHost, stream));
      RDRF_HIP(hipStreamSynchronize(stream));
    }
    for (int i = 0; i < c; ++i)
      RDRF_CHECK(host[i] >= 0 && (size_t)host[i] < ns, -1, "selftest_scatter: list[%d] = %d is outside the batch", i, host[i]);
  }
  if (!sorted) {
    ScatterArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.valid = t->valid; sa.N = N; sa.S = S;
    if (k.xw) sa.xw = t->coords;
    else {
      sa.xyz = t->coords;
      for (int i = 0; i < 3; ++i) { sa.box.lo[i] = t->box_lo[i]; sa.box.inv[i] = t->box_inv[i]; sa.box.hi[i] = t->box_lo[i] + 2.0f / t->box_inv[i]; }
    }
    sa.nsets = 0;   // live sets only, as rdrf_dynamic_bwd fills them
    for (int set = 0; set < k.nsets; ++set)
      if ((set_mask >> set) & 1) { sa.vm[sa.nsets] = t->vm[set]; sa.gvm[sa.nsets] = t->gvm[set]; sa.row0[sa.nsets] = k.row0[set]; ++sa.nsets; }
    sa.rows = t->rows; sa.stride = k.stride; sa.bcast = k.bcast; sa.flat = flat;
    if (k.list) { sa.list = t->list; sa.count = t->count; }
    if (k.dxw_ray) { sa.dxw = t->dxw; sa.dxw_accumulate = k.dxw_ray == 2; }
    if (k.g_xyz) sa.g_xyz = t->g_xyz;
    return launch_scatter("selftest_scatter", k.kern, sa, (long)ntiles, stream);
  }
  WsCarver c(t->ws, t->ws_bytes);
  BwdWs b;
  memset(&b, 0, sizeof(b));
  carve_sorted_scatter(b, c, ns);
  RDRF_CHECK(c.ok(), -3, "selftest_scatter: workspace too small");
  b.dxw = t->dxw;
  b.grows1 = const_cast<float*>(t->rows);
  b.dfs = b.dfa = const_cast<float*>(t->recs);
  BwdArgs a;
  memset(&a, 0, sizeof(a));
  a.N = N; a.S = S; a.valid = t->valid;
  a.sp.xw = const_cast<float*>(t->coords);
  a.sp.list = const_cast<int*>(t->list);
  a.sp.hdr = reinterpret_cast<SavedHdr*>(const_cast<int*>(t->count));   // only &hdr->count is formed: SavedHdr begins with it
  static_assert(offsetof(SavedHdr, count) == 0, "the device count is the first member of SavedHdr");
  RdrfDynamicParams P, G;
  memset(&P, 0, sizeof(P));
  memset(&G, 0, sizeof(G));
  if (kind == RDRF_SCK_DYN_DENSITY) { P.density = t->vm[0]; P.blending = t->vm[1]; G.density = t->gvm[0]; G.blending = t->gvm[1]; }
  else { P.app = t->vm[0]; G.app = t->gvm[0]; }
  const int old = scatter_mode_swap(mode);   // launch_scatter_tiled reads the process-wide mode (_SORTED_PLAIN: no windows)
  const int rc = kind == RDRF_SCK_DYN_DENSITY ? scatter_dyn_density_sorted(a, b, &P, &G, set_mask, stream)
                                              : scatter_dyn_app_sorted(a, b, &P, &G, stream);
  scatter_mode_swap(old);
  if (rc) return rc;
  if (t->keys_out) RDRF_HIP(hipMemcpyAsync(t->keys_out, b.keys_in, 3 * ns * 4, hipMemcpyDeviceToDevice, stream));   // (the sort leaves them intact)
  if (t->keys_sorted_out) RDRF_HIP(hipMemcpyAsync(t->keys_sorted_out, b.keys_out, 3 * ns * 4, hipMemcpyDeviceToDevice, stream));
  if (t->order_out) RDRF_HIP(hipMemcpyAsync(t->order_out, b.order, 3 * ns * 4, hipMemcpyDeviceToDevice, stream));
  if (t->counts_out) RDRF_HIP(hipMemcpyAsync(t->counts_out, b.counts, 3 * sizeof(int), hipMemcpyDeviceToDevice, stream));
  return 0;
}

// A kind's layouts in resolved form (host memory, ints), so that a reference needs none of the sv:: constants:
// [0] ints used, [1] C0Q, [2] C1Q, [3] stride levels, [4] factor sets, [5] rows per tile, [6] [7] first d(feature) row of set 0 / 1
// (-1: no such set), [8] 1 = every component's gradient is row 0, [9] floats per record (0: no sorted form), [10] floats per set
// inside a record, [11] [12] the rows the key kernel reads for liveness (-1: none), [13] takes list + count, [14] coordinates are
// normalised (xw) / xyz + box, [15] [16] coordinate gradients of the ray / sorted form (0 none, 1 written, 2 added),
// [17] g_xyz += dw * inv, [18] flat tiles allowed, [19] bits of the cell part of a key and [20..22] key row length W + 3 per plane
// (0 without `grid`), [23] quads; per quad: row relative to the set's first row, level, plane, first component, float offset inside
// the set's part of a record (-1: none).  grid: nullable {W, H} x 3 of the level-0 planes.
extern "C" int rdrf_selftest_scatter_describe(int kind, const int* grid, int* out, int cap) {
  ScatterKindInfo k;
  RDRF_CHECK(scatter_kind_info(kind, k), -1, "selftest_scatter_describe: unknown kind %d", kind);
  const int qpl = k.c0q + 2 * k.c1q, nq = k.nlv * qpl, need = 24 + 5 * nq;
  RDRF_CHECK(out != nullptr && cap >= need, -3, "selftest_scatter_describe: description buffer too small (%d < %d ints)", out ? cap : 0, need);
  int n = 0;
  out[n++] = need; out[n++] = k.c0q; out[n++] = k.c1q; out[n++] = k.nlv; out[n++] = k.nsets; out[n++] = k.stride;
  out[n++] = k.row0[0]; out[n++] = k.row0[1]; out[n++] = k.bcast; out[n++] = k.rec_floats; out[n++] = k.set_floats;
  out[n++] = k.live_row[0]; out[n++] = k.live_row[1]; out[n++] = k.list; out[n++] = k.xw; out[n++] = k.dxw_ray; out[n++] = k.dxw_sorted;
  out[n++] = k.g_xyz; out[n++] = k.flat;
  if (grid) {
    const int W[3] = {grid[0], grid[2], grid[4]}, H[3] = {grid[1], grid[3], grid[5]};
    out[n++] = sorted_key_bits(W, H);
    for (int p = 0; p < 3; ++p) out[n++] = W[p] + 3;
  } else {
    for (int i = 0; i < 4; ++i) out[n++] = 0;
  }
  out[n++] = nq;
  for (int g = 0; g < nq; ++g) {
    const int lv = g / qpl, w = g - lv * qpl;
    const int pi = w < k.c0q ? 0 : (w < k.c0q + k.c1q ? 1 : 2), q = w - (pi == 0 ? 0 : (pi == 1 ? k.c0q : k.c0q + k.c1q));
    out[n++] = k.bcast ? 0 : 4 * g; out[n++] = lv; out[n++] = pi; out[n++] = 4 * q;
    out[n++] = k.rec_floats == DFS_FLOATS ? dfs_off(g) : (k.rec_floats == DFA_FLOATS ? dfa_off(g) : -1);
  }
  return n;
}

// the launch decisions of the most recent scatter: [0] ints used, [1] form (0 ray tiles, 1 sorted passes), [2] 1 = one launch per
// factor set, [3] launches; per launch: accumulator element bytes (8 / 4 / 0), threads, workgroups, tiled (1 taken, 0 refused,
// -2 switched off,
// -1 not tried), window width, wave steps per slice
extern "C" int rdrf_selftest_scatter_last(int* out, int cap) {
  const ScatterRecord& r = scatter_last_record();
  const int need = 4 + 6 * r.n;
  RDRF_CHECK(out != nullptr && cap >= need, -3, "selftest_scatter_last: buffer too small (%d < %d ints)", out ? cap : 0, need);
  int n = 0;
  out[n++] = need; out[n++] = r.form; out[n++] = r.split; out[n++] = r.n;
  for (int i = 0; i < r.n; ++i) {
    out[n++] = r.l[i].elem_bytes; out[n++] = r.l[i].threads; out[n++] = r.l[i].workgroups; out[n++] = r.l[i].tiled;
    out[n++] = r.l[i].tw; out[n++] = r.l[i].slice_steps;
  }
  return n;
}

// ------------------------------------------------------------------------------------------------
// rdrf_selftest_gather / rdrf_selftest_encodings: the forward VM gather (shared taps) and the positional encodings as the forward
// kernels call them, on points the caller supplies; reference: tests/_gather_prim.py.  One wave per 32 points, lane = 32 h + s
// holds half h of point s in the canonical layout; a lane past M evaluates point 0 and stores nothing.  The raw registers go
// out in LOGICAL column order through the index maps the pack jobs of rdrf_fwd.hip lay the first-layer weights out with
// (seg_imap o elem_of): slot kk of half h is column seg_imap(seg, elem_of(kk, h), in_dim), so a gather order that disagrees with
// the weight columns shows up as a permuted row.
// ------------------------------------------------------------------------------------------------
namespace {

template <int NK>
RDRF_D void gt_store(const float (&v)[NK], float* __restrict__ out, int row, int ld, int seg, int kk0, int in_dim, int col0, int h) {
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
    const int col = seg_imap(seg, elem_of(kk0 + kk, h), in_dim);
    if (col >= 0) out[(size_t)row * ld + (col - col0)] = v[kk];
  }
}

template <int KIND>
__global__ __launch_bounds__(64) void k_st_gather(const RdrfVM vm, const float* __restrict__ xn, int M, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, h = lane >> 5, row = blockIdx.x * 32 + (lane & 31);
  const bool act = row < M;
  const int idx = act ? row : 0;
  const float x0 = xn[(size_t)idx * 3 + 0], x1 = xn[(size_t)idx * 3 + 1], x2 = xn[(size_t)idx * 3 + 2];
  if constexpr (KIND == RDRF_SCK_STATIC_DENSITY) {   // static_density_body / k_alpha_static / k_point_static
    const float f = static_density_feature(vm, x0, x1, x2);
    if (act && h == 0) out[row] = f;
  } else if constexpr (KIND == RDRF_SCK_STATIC_APP) {   // static_app_body: basis columns SEG_IDENT of 72
    float G[36];
    gather_level_app<0>(vm, point_taps(vm, x0, x1, x2, 0), h, G);
    if (act) gt_store<36>(G, out, row, 72, SEG_IDENT, 0, 72, 0, h);
  } else if constexpr (KIND == RDRF_SCK_DYN_DENSITY) {   // head_raw: first-layer columns SEG_IDENT of 72
    float Fv[36];
    gather_level_den<0>(vm, point_taps(vm, x0, x1, x2, 0), h, Fv);
    gather_level_den<12>(vm, point_taps(vm, x0, x1, x2, 1), h, Fv);
    gather_level_den<24>(vm, point_taps(vm, x0, x1, x2, 2), h, Fv);
    if (act) gt_store<36>(Fv, out, row, 72, SEG_IDENT, 0, 72, 0, h);
  } else {   // dyn_app_body: level by level, basis columns SEG_IDENT of 216 at slots 36 lv ..
    {
      float A[36];
      gather_level_app<0>(vm, point_taps(vm, x0, x1, x2, 0), h, A);
      if (act) gt_store<36>(A, out, row, 216, SEG_IDENT, 0, 216, 0, h);
    }
    {
      float A[36];
      gather_level_app<0>(vm, point_taps(vm, x0, x1, x2, 1), h, A);
      if (act) gt_store<36>(A, out, row, 216, SEG_IDENT, 36, 216, 0, h);
    }
    {
      float A[36];
      gather_level_app<0>(vm, point_taps(vm, x0, x1, x2, 2), h, A);
      if (act) gt_store<36>(A, out, row, 216, SEG_IDENT, 72, 216, 0, h);
    }
  }
}

// X0 -> [xn 3 | sin 30 | cos 30 | t] = columns 72 .. 135 of the heads' first layer, X1 -> [sin 8 | cos 8] = columns 136 .. 151
__global__ __launch_bounds__(64) void k_st_encodings(const float* __restrict__ xn, const float* __restrict__ t, int M,
                                                     float* __restrict__ x0_out, float* __restrict__ x1_out) {
  const int lane = threadIdx.x & 63, h = lane >> 5, row = blockIdx.x * 32 + (lane & 31);
  const bool act = row < M;
  const int idx = act ? row : 0;
  const float tt = t[idx];
  float X0[32], X1[8];
  fill_x0(X0, xn[(size_t)idx * 3 + 0], xn[(size_t)idx * 3 + 1], xn[(size_t)idx * 3 + 2], tt, h);
  fill_x1(X1, tt, h);
  if (act) {
    gt_store<32>(X0, x0_out, row, 64, SEG_DEN1_X0, 0, 152, 72, h);
    gt_store<8>(X1, x1_out, row, 16, SEG_DEN1_X1, 0, 152, 136, h);
  }
}

// every address of the gather is a clamped tap index times a stride: inside the arrays for any axis of at least one texel
bool gather_vm_ok(const RdrfVM& v, int c0, int c1) {
  if (!vm_ok(v, c0, c1)) return false;
  for (int i = 0; i < 3; ++i) {
    if (v.W[i] < 1 || v.H[i] < 1 || v.L[i] < 1 || !v.plane[i] || !v.line[i]) return false;
    const bool w_fast = v.sW[i] == v.C[i] && v.sH[i] == v.W[i] * v.C[i], h_fast = v.sH[i] == v.C[i] && v.sW[i] == v.H[i] * v.C[i];
    if (!w_fast && !h_fast) return false;   // the two storage orders of a plane: the arrays hold H W C floats
    if ((((uintptr_t)v.plane[i] | (uintptr_t)v.line[i]) & 15) != 0) return false;
  }
  return true;
}

}  // namespace

extern "C" int rdrf_selftest_gather(int kind, const RdrfVM* vm, int nsets, const float* xn, int M, float* out, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(kind >= RDRF_SCK_STATIC_DENSITY && kind <= RDRF_SCK_DYN_APP, -1, "selftest_gather: unknown kind %d", kind);
  RDRF_CHECK(nsets >= 1 && nsets <= 2, -1, "selftest_gather: one or two factor sets (got %d)", nsets);
  if (M == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(vm && xn && out && M > 0 && M <= (1 << 24), -1, "selftest_gather: bad arguments");
  const bool app = kind == RDRF_SCK_STATIC_APP || kind == RDRF_SCK_DYN_APP;
  const int nf = kind == RDRF_SCK_STATIC_DENSITY ? 1 : (kind == RDRF_SCK_DYN_APP ? 216 : 72);
  for (int set = 0; set < nsets; ++set)
    RDRF_CHECK(gather_vm_ok(vm[set], app ? 48 : 16, app ? 12 : 4), -1,
               "selftest_gather: factor set %d: component counts, one grid of at least one texel per axis, W-fastest or H-fastest "
               "planes, 16-byte aligned", set);
  const dim3 grid((M + 31) / 32), block(64);
  for (int set = 0; set < nsets; ++set) {
    float* o = out + (size_t)set * M * nf;
    switch (kind) {
      case RDRF_SCK_STATIC_DENSITY: RDRF_LAUNCH("selftest_gather", k_st_gather<RDRF_SCK_STATIC_DENSITY>, grid, block, stream, vm[set], xn, M, o); break;
      case RDRF_SCK_STATIC_APP: RDRF_LAUNCH("selftest_gather", k_st_gather<RDRF_SCK_STATIC_APP>, grid, block, stream, vm[set], xn, M, o); break;
      case RDRF_SCK_DYN_DENSITY: RDRF_LAUNCH("selftest_gather", k_st_gather<RDRF_SCK_DYN_DENSITY>, grid, block, stream, vm[set], xn, M, o); break;
      default: RDRF_LAUNCH("selftest_gather", k_st_gather<RDRF_SCK_DYN_APP>, grid, block, stream, vm[set], xn, M, o); break;
    }
  }
  return 0;
}

extern "C" int rdrf_selftest_encodings(const float* xn, const float* t, int M, float* x0_out, float* x1_out, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(xn && t && x0_out && x1_out && M > 0 && M <= (1 << 24), -1, "selftest_encodings: bad arguments");
  RDRF_LAUNCH("selftest_encodings", k_st_encodings, dim3((M + 31) / 32), dim3(64), stream, xn, t, M, x0_out, x1_out);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// rdrf_selftest_ray_scan / rdrf_selftest_ray_scan_bwd (host code only): the per-field ray scan on caller-owned arrays, through the
// launchers of the entry points (rdrf_render_host.hpp, rdrf_bwd_host.hpp); reference: tests/_scan_prim.py
// ------------------------------------------------------------------------------------------------
extern "C" int rdrf_selftest_ray_scan(int width, const float* rays, const float* z, const float* sigma, int N, int S, int ray_type,
                                      float distance_scale, float weight_thres, float* weight, float* dists, int* list,
                                      int* counter, float* rgb, rdrf_stream_t stream_) {
  RDRF_CHECK(width == 32 || width == 64, -1, "selftest_ray_scan: width is 32 (k_ray_scan) or 64 (k_static_scan), got %d", width);
  if (N == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(rays && z && sigma && weight && dists && list && counter && N > 0, -1, "selftest_ray_scan: bad arguments");
  RDRF_CHECK(S >= 1 && S <= 4096, -1, "selftest_ray_scan: S in 1 .. 4096 (got %d)", S);
  RDRF_CHECK(ray_type >= RDRF_RAY_NDC && ray_type <= RDRF_RAY_OTHER, -1, "selftest_ray_scan: unknown ray type %d", ray_type);
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "selftest_ray_scan: N * S * 3 must stay below 2^31");
  FieldArgs a;
  memset(&a, 0, sizeof(a));
  a.rays = rays; a.z = z; a.N = N; a.S = S;
  a.distance_scale = distance_scale; a.weight_thres = weight_thres; a.ray_type = ray_type;
  a.sigma = const_cast<float*>(sigma); a.weight = weight; a.dists = dists; a.rgb = rgb;
  a.list = list; a.counter = counter;
  return width == 32 ? launch_ray_scan(a, (hipStream_t)stream_) : launch_static_scan(a, (hipStream_t)stream_);
}

extern "C" int rdrf_selftest_ray_scan_bwd(int width, const float* rays, const float* z, const uint8_t* valid, const float* raw, int N,
                                          int S, int act, float density_shift, float distance_scale, int ray_type,
                                          const float* g_weight, const float* g_sigma, const float* g_dists, float* out, float* g_z,
                                          float* g_rays, rdrf_stream_t stream_) {
  RDRF_CHECK(width == 32 || width == 64, -1, "selftest_ray_scan_bwd: width is 32 (k_ray_scan_bwd) or 64 (k_static_density_bwd), got %d",
             width);
  if (N == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(rays && z && valid && raw && out && N > 0, -1, "selftest_ray_scan_bwd: bad arguments");
  RDRF_CHECK(S >= 1 && S <= 4096, -1, "selftest_ray_scan_bwd: S in 1 .. 4096, the carry slots of the kernels (got %d)", S);
  RDRF_CHECK(act == RDRF_ACT_RELU || act == RDRF_ACT_SOFTPLUS, -1, "selftest_ray_scan_bwd: unknown activation %d", act);
  RDRF_CHECK(ray_type >= RDRF_RAY_NDC && ray_type <= RDRF_RAY_OTHER, -1, "selftest_ray_scan_bwd: unknown ray type %d", ray_type);
  RDRF_CHECK((size_t)N * (S + 31) * 3 < (size_t)INT32_MAX, -1, "selftest_ray_scan_bwd: N * S * 3 must stay below 2^31");
  return ray_scan_bwd_on_arrays(width, rays, z, valid, raw, N, S, act, density_shift, distance_scale, ray_type, g_weight, g_sigma,
                                g_dists, out, g_z, g_rays, (hipStream_t)stream_);
}

// ------------------------------------------------------------------------------------------------
// rdrf_selftest_heads_bwd / rdrf_selftest_time_branch / rdrf_selftest_time_branch_bwd (host code only): the heads' backward tile of
// the dynamic field's density phase and the time branch, forward and backward, on rows and arrays the caller supplies, through
// the launchers of the entry points (rdrf_bwd_host.hpp, rdrf_render_host.hpp); reference: tests/_heads_prim.py
// ------------------------------------------------------------------------------------------------
static void carve_heads_bwd(float*& pk, WsCarver& c) { pk = c.take<float>(PACK_AREA_FLOATS); }
extern "C" size_t rdrf_selftest_heads_bwd_workspace_bytes(int N, int S) {   // the weight images only: the same at every shape
  (void)N; (void)S;
  float* pk;
  WsCarver c;
  carve_heads_bwd(pk, c);
  return c.off;
}

// [0] ints used, [1] workgroups and [2] waves per workgroup of the launch (a wave walks the tiles wg * waves + wave, + grid * waves,
// ...), [3] tiles, [4] saved rows per tile, [5] gradient rows per tile, [6] first d(X0) row, [7] first small-layer dz row (the
// heads write rows + 3 and + 4), [8] floats per sample-major record.  The other rows: rdrf_selftest_dw_describe (dz, saved
// activations) and rdrf_selftest_scatter_describe (d(feature) rows, record offsets).
extern "C" int rdrf_selftest_heads_describe(int mode, int N, int S, int* out, int cap) {
  RDRF_CHECK(mode == RDRF_HEADS_FLAT || mode == RDRF_HEADS_FEAT, -1, "selftest_heads_describe: unknown mode %d", mode);
  RDRF_CHECK(N >= 0 && (mode == RDRF_HEADS_FEAT || S >= 1), -1, "selftest_heads_describe: bad shape %d x %d", N, S);
  RDRF_CHECK(out != nullptr && cap >= 9, -3, "selftest_heads_describe: description buffer too small (%d < 9 ints)", out ? cap : 0);
  const long units = mode == RDRF_HEADS_FEAT ? heads_bwd_units((N + 31) / 32, 32, 0) : heads_bwd_units(N, S, 1);
  const Geo g = geo_for_units(units);
  int n = 0;
  out[n++] = 9; out[n++] = g.grid; out[n++] = g.block / 64; out[n++] = (int)units; out[n++] = sv::K1_ROWS; out[n++] = sv::K1G_ROWS;
  out[n++] = sv::K1G_DX0; out[n++] = sv::K1G_SM; out[n++] = DFS_FLOATS;
  return n;
}

extern "C" int rdrf_selftest_heads_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, int mode, int N, int S, const float* act1,
                                       size_t act1_floats, const float* raw, const uint8_t* valid, const float* g_sigma,
                                       const float* g_blending, int live_d, float* grows1, size_t grows1_floats, float* dfs,
                                       size_t dfs_floats, const RdrfDynamicParams* grads, void* ws, size_t ws_bytes,
                                       rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(mode == RDRF_HEADS_FLAT || mode == RDRF_HEADS_FEAT, -1, "selftest_heads_bwd: unknown mode %d", mode);
  if (N == 0) return 0;   // empty batch: a no-op
  const bool feat = mode == RDRF_HEADS_FEAT;
  RDRF_CHECK(P && cfg && grads && act1 && grows1 && ws && N > 0, -1, "selftest_heads_bwd: bad arguments");
  RDRF_CHECK(cfg->act == RDRF_ACT_RELU || cfg->act == RDRF_ACT_SOFTPLUS, -1, "selftest_heads_bwd: unknown activation %d", cfg->act);
  if (feat) {
    RDRF_CHECK(dfs == nullptr, -1, "selftest_heads_bwd: feature mode writes no sample-major records");
    RDRF_CHECK(N <= (1 << 24), -1, "selftest_heads_bwd: at most 2^24 points (got %d)", N);
  } else {
    RDRF_CHECK(S >= 1 && S <= 4096, -1, "selftest_heads_bwd: S in 1 .. 4096 (got %d)", S);
    RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "selftest_heads_bwd: N * S * 3 must stay below 2^31");
    RDRF_CHECK(raw && valid && g_sigma, -1, "selftest_heads_bwd: flat tiles take raw, valid and the total d(sigma)");
    RDRF_CHECK(grads->dw2 && grads->db2 && grads->bw2 && grads->bb2, -1, "selftest_heads_bwd: null small-layer gradient");
  }
  RDRF_CHECK((((uintptr_t)act1 | (uintptr_t)grows1 | (uintptr_t)ws | (uintptr_t)dfs) & 15) == 0, -1,
             "selftest_heads_bwd: rows, records and workspace must be 16-byte aligned");
  const size_t ns = feat ? (size_t)N : (size_t)N * S, tiles = (ns + 31) / 32;
  RDRF_CHECK(act1_floats >= tiles * sv::K1_ROWS * 32 && grows1_floats >= tiles * sv::K1G_ROWS * 32, -3,
             "selftest_heads_bwd: rows too small for %zu tiles", tiles);
  RDRF_CHECK(dfs == nullptr || dfs_floats >= ns * DFS_FLOATS, -3, "selftest_heads_bwd: records too small (%zu < %zu floats)", dfs_floats,
             ns * DFS_FLOATS);
  WsCarver c(ws, ws_bytes);
  float* pk;
  carve_heads_bwd(pk, c);
  RDRF_CHECK(c.ok(), -3, "selftest_heads_bwd: workspace too small");
  return heads_bwd_on_rows(P, cfg, feat ? 1 : 0, feat ? (int)tiles : N, feat ? 32 : S, feat ? N : 0, act1, raw, valid,
                           feat ? nullptr : g_sigma, feat ? g_sigma : nullptr, g_blending, live_d != 0, grows1, dfs, grads, pk, stream);
}

extern "C" int rdrf_selftest_time_branch(const RdrfDynamicParams* P, const float* ts, int N, float* tout, int* zero64,
                                         rdrf_stream_t stream_) {
  if (N == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(P && ts && tout && N > 0 && N <= (1 << 24), -1, "selftest_time_branch: bad arguments");
  RDRF_CHECK(P->l1w && P->l1b && P->l2w && P->l2b, -1, "selftest_time_branch: null time-branch weights");
  DynW w;
  fill_dyn_w(w, P);
  return launch_time_branch(ts, w, N, tout, zero64, (hipStream_t)stream_);
}

extern "C" int rdrf_selftest_time_branch_bwd(const RdrfDynamicParams* P, const float* ts, int N, int S, const float* dtout,
                                             const float* dtp, size_t dtp_floats, const RdrfDynamicParams* grads,
                                             rdrf_stream_t stream_) {
  if (N == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(P && ts && dtout && grads && N > 0 && S >= 1 && S <= 4096, -1, "selftest_time_branch_bwd: bad arguments");
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "selftest_time_branch_bwd: N * S * 3 must stay below 2^31");
  RDRF_CHECK(P->l1w && P->l1b && P->l2w && P->l2b, -1, "selftest_time_branch_bwd: null time-branch weights");
  RDRF_CHECK(grads->l1w && grads->l1b && grads->l2w && grads->l2b, -1, "selftest_time_branch_bwd: null time-branch gradient");
  const size_t tiles = ((size_t)N * S + 31) / 32;
  RDRF_CHECK(dtp == nullptr || dtp_floats >= tiles * 64, -3, "selftest_time_branch_bwd: partial records too small (%zu < %zu floats)",
             dtp_floats, tiles * 64);
  DynW w;
  fill_dyn_w(w, P);
  return launch_time_branch_bwd(ts, w, N, dtout, dtp, S, grads, (hipStream_t)stream_);
}

// ------------------------------------------------------------------------------------------------
// rdrf_selftest_app_bwd (host code only): the backward-data kernels of the appearance phase on saved rows, a compaction list and
// cotangents the caller supplies, through the launchers of the entry points (rdrf_bwd_host.hpp); reference: tests/_app_prim.py
// ------------------------------------------------------------------------------------------------
static void carve_app_bwd(float*& pk, WsCarver& c) { pk = c.take<float>(PACK_AREA_FLOATS); }
extern "C" size_t rdrf_selftest_app_bwd_workspace_bytes(int N, int S) {   // the weight image only: the same at every shape
  (void)N; (void)S;
  float* pk;
  WsCarver c;
  carve_app_bwd(pk, c);
  return c.off;
}
static bool app_field_ok(int field) { return field == RDRF_APP_DYN || field == RDRF_APP_STATIC_FEA || field == RDRF_APP_STATIC_TE; }
static bool app_mode_ok(int mode) { return mode == RDRF_APP_ROWS || mode == RDRF_APP_RECORDS || mode == RDRF_APP_FEAT; }

// [0] ints used, [1] workgroups and [2] waves per workgroup of the launch (the waves of workgroup b take the tiles b, b + grid,
// ... from the workgroup's queue: the first `waves` of them one each, then whoever is done first), [3] tiles the launch is sized
// for (the kernel walks ceil(count / 32) of them), [4] saved rows per tile, [5] gradient rows per tile, [6] .. [10] first row of
// DZV, DZ2, DZ1, DF, DA, [11] .. [13] first of the saved rows the ray path reads: H2, H1, and X0 (dynamic) or P (static), [14]
// floats per sample-major record (0: the field writes none), [15] DA rows the field writes.  The offset of every feature quad in
// a record, and the level / plane / component behind every DA row: rdrf_selftest_scatter_describe (RDRF_SCK_DYN_APP / STATIC_APP).
extern "C" int rdrf_selftest_app_describe(int field, int mode, int N, int S, int* out, int cap) {
  RDRF_CHECK(app_field_ok(field), -1, "selftest_app_describe: unknown field %d", field);
  RDRF_CHECK(app_mode_ok(mode), -1, "selftest_app_describe: unknown mode %d", mode);
  RDRF_CHECK(N >= 0 && (mode == RDRF_APP_FEAT || S >= 1), -1, "selftest_app_describe: bad shape %d x %d", N, S);
  RDRF_CHECK(out != nullptr && cap >= 16, -3, "selftest_app_describe: description buffer too small (%d < 16 ints)", out ? cap : 0);
  const bool dyn = field == RDRF_APP_DYN;
  const long units = mode == RDRF_APP_FEAT ? app_bwd_units((N + 31) / 32, 32, 1) : app_bwd_units(N, S, 0);
  const Geo g = geo_for_units(units);
  int n = 0;
  out[n++] = 16; out[n++] = g.grid; out[n++] = g.block / 64; out[n++] = (int)units;
  out[n++] = dyn ? sv::K3_ROWS : sv::S3_ROWS; out[n++] = sv::K3G_ROWS;
  out[n++] = sv::K3G_DZV; out[n++] = sv::K3G_DZ2; out[n++] = sv::K3G_DZ1; out[n++] = sv::K3G_DF; out[n++] = sv::K3G_DA;
  out[n++] = dyn ? sv::K3_H2 : sv::S3_H2; out[n++] = dyn ? sv::K3_H1 : sv::S3_H1; out[n++] = dyn ? sv::K3_X0 : sv::S3_P;
  out[n++] = dyn ? DFA_FLOATS : 0; out[n++] = dyn ? 112 : 48;
  return n;
}

extern "C" int rdrf_selftest_app_bwd(const void* P, const RdrfFieldCfg* cfg, int field, int mode, int ray_type, int N, int S,
                                     const float* act3, size_t act3_floats, const int* list, const int* count, const float* rays,
                                     const float* g_rgb, const float* g_feat, float* grows3, size_t grows3_floats, float* dfa,
                                     size_t dfa_floats, float* dxn, float* g_rays, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(app_field_ok(field), -1, "selftest_app_bwd: unknown field %d", field);
  RDRF_CHECK(app_mode_ok(mode), -1, "selftest_app_bwd: unknown mode %d", mode);
  RDRF_CHECK(mode != RDRF_APP_RECORDS || field == RDRF_APP_DYN, -1, "selftest_app_bwd: only the dynamic field writes sample-major records");
  RDRF_CHECK((mode == RDRF_APP_RECORDS) == (dfa != nullptr), -1, "selftest_app_bwd: records go with RDRF_APP_RECORDS and nothing else");
  if (N == 0) return 0;   // empty batch: a no-op
  const bool feat = mode == RDRF_APP_FEAT, dyn = field == RDRF_APP_DYN;
  RDRF_CHECK(P && cfg && grows3 && ws && N > 0, -1, "selftest_app_bwd: bad arguments");
  RDRF_CHECK(ray_type == RDRF_RAY_NDC || ray_type == RDRF_RAY_CONTRACT || ray_type == RDRF_RAY_OTHER, -1,
             "selftest_app_bwd: unknown ray type %d", ray_type);
  if (feat) {
    RDRF_CHECK(g_feat != nullptr, -1, "selftest_app_bwd: feature mode takes g_feat");
    RDRF_CHECK(N <= (1 << 24), -1, "selftest_app_bwd: at most 2^24 points (got %d)", N);
  } else {
    RDRF_CHECK(S >= 1 && S <= 4096, -1, "selftest_app_bwd: S in 1 .. 4096 (got %d)", S);
    RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "selftest_app_bwd: N * S * 3 must stay below 2^31");
    RDRF_CHECK(act3 && list && count && rays, -1, "selftest_app_bwd: the ray path takes saved rows, the list, its count and rays");
    RDRF_CHECK(!dyn || dxn != nullptr, -1, "selftest_app_bwd: the dynamic field writes dxn");
  }
  RDRF_CHECK((((uintptr_t)act3 | (uintptr_t)grows3 | (uintptr_t)ws | (uintptr_t)dfa) & 15) == 0, -1,
             "selftest_app_bwd: rows, records and workspace must be 16-byte aligned");
  const size_t ns = feat ? (size_t)N : (size_t)N * S, tiles = (ns + 31) / 32;
  RDRF_CHECK((feat || act3_floats >= tiles * (dyn ? sv::K3_ROWS : sv::S3_ROWS) * 32) && grows3_floats >= tiles * sv::K3G_ROWS * 32, -3,
             "selftest_app_bwd: rows too small for %zu tiles", tiles);
  RDRF_CHECK(dfa == nullptr || dfa_floats >= ns * DFA_FLOATS, -3, "selftest_app_bwd: records too small (%zu < %zu floats)", dfa_floats,
             ns * DFA_FLOATS);
  WsCarver c(ws, ws_bytes);
  float* pk;
  carve_app_bwd(pk, c);
  RDRF_CHECK(c.ok(), -3, "selftest_app_bwd: workspace too small");
  if (!feat) {   // the kernels index g_rgb, dxn, rays and the records by what the list holds: looked at before anything is launched
    std::vector<int> hl(ns);
    int hc = 0;
    RDRF_HIP(hipMemcpyAsync(&hc, count, sizeof(int), hipMemcpyDeviceToHost, stream));
    RDRF_HIP(hipMemcpyAsync(hl.data(), list, ns * sizeof(int), hipMemcpyDeviceToHost, stream));
    RDRF_HIP(hipStreamSynchronize(stream));
    RDRF_CHECK(hc >= 0 && (size_t)hc <= ns, -1, "selftest_app_bwd: count %d outside 0 .. %zu", hc, ns);
    for (int i = 0; i < hc; ++i)
      RDRF_CHECK(hl[i] >= 0 && (size_t)hl[i] < ns, -1, "selftest_app_bwd: list[%d] = %d outside 0 .. %zu", i, hl[i], ns - 1);
  }
  RdrfFieldCfg cf = *cfg;
  cf.ray_type = ray_type;
  cf.static_head = field == RDRF_APP_STATIC_TE ? RDRF_HEAD_MLP_FEA_TIMEEMBEDDING : RDRF_HEAD_MLP_FEA;
  const AppBwdForm form = feat ? APP_FEAT : (mode == RDRF_APP_RECORDS ? APP_RECORDS : APP_ROWS);
  return app_bwd_on_rows(P, &cf, dyn ? 1 : 0, form, feat ? (int)tiles : N, feat ? 32 : S, feat ? N : 0, act3, list, count, rays,
                         feat ? nullptr : g_rgb, feat ? g_feat : nullptr, grows3, dfa, dxn, feat ? nullptr : g_rays, pk, stream);
}

// ------------------------------------------------------------------------------------------------
// rdrf_selftest_mlp: y[M][64] = relu(x[M][64] W^T + b) through pack + LDS + mfma_seg, one tile per wave -- a whole fp32
// layer with its bias and relu (tests/test_gpu_forward.py)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_selftest(const float* __restrict__ x,
                                                 const float* __restrict__ pkw, int M,
                                                 float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float lds[2 * 32 * 64 + 64];
  lds_fill(lds, pkw, 2 * 32 * 64 + 64);
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int row = blockIdx.x * 32 + s;
  float in[32];
#pragma unroll
  for (int kk = 0; kk < 32; ++kk) in[kk] = row < M ? x[(size_t)row * 64 + elem_of(kk, h)] : 0.f;
  f32x16 acc[2];
  acc_bias<2>(acc, lds + 2 * 32 * 64, h);
  mfma_seg<2, 32>(acc, in, lds, lane);
  float out[32];
  acc_relu<2>(out, acc);
  if (row < M)
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) y[(size_t)row * 64 + elem_of(kk, h)] = out[kk];
}

extern "C" int rdrf_selftest_mlp(const float* x, const float* w, const float* b, int M, int K,
                                 int OUT, float* y, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(x && w && b && y && M > 0, -1, "selftest_mlp: bad arguments");
  RDRF_CHECK(K == 64 && OUT == 64, -1, "selftest_mlp: the self-test layer is 64 -> 64");
  RDRF_CHECK(ws_bytes >= (2 * 32 * 64 + 64) * sizeof(float), -3, "selftest_mlp: workspace too small");
  PackJobs J;
  J.n = 0;
  pack_add(J, w, 64, 64, 64, SEG_IDENT, 0, 2, 32, 0);
  pack_add(J, b, 0, 64, 0, 0, 3, 0, 32, 2 * 32 * 64);
  int rc = pack_launch(J, (float*)ws, stream);
  if (rc) return rc;
  RDRF_LAUNCH("selftest", k_selftest, dim3((M + 31) / 32), dim3(64), stream, x, (const float*)ws, M, y);
  return 0;
}
