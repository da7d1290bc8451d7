// rdrf_selftest.hip -- every MLP layer primitive of rdrf_common.hpp, stand-alone, with the template arguments the product
// kernels use and the product's own pack code (tests/test_gpu_mlp_primitives.py compares the results with float64).
//
// One wave per 32-row tile, as k_selftest (rdrf_render.hip): the wave's workgroup copies the packed image into LDS, lane
// (h, s) loads its half of row s in the canonical layout, the primitive runs on ZERO accumulators and the raw accumulators
// are stored: no bias, no relu, so the result is linear in x and w.  Rows past M read as zero and are not stored.
//   forward forms     x[M][K]   , w[OUT][K]  ->  y[M][OUT] = x w^T
//   transposed forms  x[M][OUT] , w[OUT][K]  ->  y[M][K]   = x w      (the backward-data product of the same layer)
#include "rdrf_host.hpp"

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
