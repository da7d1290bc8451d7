// rdrf_selftest.hip -- every MLP layer primitive of rdrf_common.hpp, stand-alone, with the template arguments the product
// kernels use and the product's own pack code (tests/test_gpu_mlp_primitives.py compares the results with float64).
//
// One wave per 32-row tile, as k_selftest (rdrf_render.hip): the wave's workgroup copies the packed image into LDS, lane
// (h, s) loads its half of row s in the canonical layout, the primitive runs on ZERO accumulators and the raw accumulators
// are stored: no bias, no relu, so the result is linear in x and w.  Rows past M read as zero and are not stored.
//   forward forms     x[M][K]   , w[OUT][K]  ->  y[M][OUT] = x w^T
//   transposed forms  x[M][OUT] , w[OUT][K]  ->  y[M][K]   = x w      (the backward-data product of the same layer)
//
// rdrf_selftest_dw (end of the file, host code only): the dW job lists of the backward entry points (the builders of
// rdrf_bwd.hip) planned and launched by dw_launch on rows the caller supplies; reference: tests/_dw_prim.py.
#include "rdrf_kernels.hpp"
#include "rdrf_bwd_host.hpp"

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

extern "C" int rdrf_selftest_sf_geometry(int ntiles, int* grid, int* waves) {
  RDRF_CHECK(ntiles >= 0 && grid && waves, -1, "selftest_sf_geometry: bad arguments");
  scene_flow_fused_geometry(ntiles, grid, waves);
  return 0;
}

extern "C" int rdrf_selftest_warp_geometry(int ntiles, int* grid, int* waves) {
  RDRF_CHECK(ntiles >= 0 && grid && waves, -1, "selftest_warp_geometry: bad arguments");
  warp_fused_geometry(ntiles, grid, waves);
  return 0;
}

extern "C" size_t rdrf_selftest_warp_bwd_workspace_bytes(int N, int S) {
  return warp_bwd_on_rows_pack_floats() * 4 + (((size_t)N * S + 255) & ~(size_t)255) + 512;
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
  RDRF_CHECK(ws_bytes >= rdrf_selftest_warp_bwd_workspace_bytes(N, S), -3, "selftest_warp_bwd: workspace too small");
  WsCarver c(ws, ws_bytes);
  float* pk = c.take<float>(warp_bwd_on_rows_pack_floats());
  uint8_t* valid = c.take<uint8_t>((size_t)N * S);
  return warp_bwd_on_rows(P, cfg, N, S, act1, grows1, dxw, dxn, g_xyz_prime, grads, g_xyz, dtout, dtp, pk, valid, stream);
}
