// rdrf_fwd_dev.hpp -- device bodies of the forward field kernels (TensorBase.forward, /root/reference/models/
// tensorBase.py:704-850), shared by the per-phase kernels of rdrf_fwd.hip and the single-launch fused render of
// rdrf_render.hip.  A body sees its position in the launch through GridCtx (workgroup id / count, thread id / count)
// and gets its LDS weight image as a pointer, so the same code runs as its own kernel or as one phase of a larger one.
// The evaluation of ONE sample -- load_tout, warp_mlp, warp_point, head_raw, static_density_feature, fill_sf_x + sf_mlp -- and
// of one round of a ray -- weight_round, append_masked, zero_rgb_round -- are functions of their own: the kernels that
// need the forward's bits off the training path (rdrf_alpha.hip, rdrf_render_masked.hip, rdrf_motion.hip, rdrf_track.hip)
// call them too.
#pragma once
#include "rdrf_kernels.hpp"

struct GridCtx {
  int bid, nblk, tid, nthr;
};
RDRF_D GridCtx grid_ctx() { return GridCtx{(int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, (int)blockDim.x}; }
// a body that IS the kernel (FUSED = false) reads the launch geometry from the hardware registers, exactly as the
// kernels did before they were split into bodies (same code generation); as a phase of the fused render it reads gc
#define GC_BID (FUSED ? gc.bid : (int)blockIdx.x)
#define GC_NBLK (FUSED ? gc.nblk : (int)gridDim.x)
#define GC_TID (FUSED ? gc.tid : (int)threadIdx.x)
#define GC_NTHR (FUSED ? gc.nthr : (int)blockDim.x)

// rank of the calling lane among the set lanes below it in a ballot
RDRF_D unsigned ballot_rank(unsigned long long bal) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}

// App-mask compaction (models/tensorBase.py:773-790): the masked samples are appended to one list through one counter -- an
// atomic with return on ONE address for the whole chip (~3.6 ns each, serialised at the memory side: 65 k appends of a
// 32 400-ray frame are 0.23 ms during which every appending wave waits).  So the density kernels count first, append once
// per workgroup (here) or per ray (dyn_density_body), and write their entries in a second sweep over the stored weights.
// cnt is wave-uniform; returns the wave's base in the list.  All threads of the workgroup must call it.
RDRF_D int block_append_base(int* counter, int cnt, int* s_cnt, int tid, int nthr) {   // cnt: wave-uniform; returns the wave's base
  const int wave = tid >> 6, nwaves = nthr >> 6;
  __syncthreads();   // s_cnt may still be read by the previous use
  if ((tid & 63) == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < nwaves; ++w) {
      const int c = s_cnt[w];
      s_cnt[w] = tot;
      tot += c;
    }
    const int b = tot ? atomicAdd(counter, tot) : 0;
    for (int w = 0; w < nwaves; ++w) s_cnt[w] += b;
  }
  __syncthreads();
  return s_cnt[wave];
}

// The static field's density feature at a normalised point (models/tensoRF.py:118-154): quads 0..3 plane XY, 4 plane XZ,
// 5 plane YZ; one set of axis taps for all six (shared-tap gather).  The order of the sums is part of the result's bits.
RDRF_D float static_density_feature(const RdrfVM& density, float x0, float x1, float x2) {
  float f = 0.0f;
  const PointTaps pt = point_taps(density, x0, x1, x2, 0);
  const PlaneTaps xy = plane_taps(density, 0, pt.x, pt.y, pt.z, 0);
  float sp = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 v = taps_quad(xy, 4 * q);
    sp += v.x + v.y + v.z + v.w;
  }
  f += sp;
  const f32x4 v1 = taps_quad(plane_taps(density, 1, pt.x, pt.z, pt.y, 0), 0);
  f += v1.x + v1.y + v1.z + v1.w;
  const f32x4 v2 = taps_quad(plane_taps(density, 2, pt.y, pt.z, pt.x, 0), 0);
  f += v2.x + v2.y + v2.z + v2.w;
  return f;
}

// One transmittance round of a ray (models/tensorBase.py:755-772): W consecutive samples in the lanes l = 0 .. W - 1 of a
// W-lane group, sample j of the ray at idx.  z -> dists -> alpha -> product scan -> weight; `carry` is the transmittance
// behind the rounds before this one.  A 32-wide and a 64-wide scan multiply in different orders (other roundings), so a
// field's every path scans at that field's width.  Returns the weight.
template <int W>
RDRF_D float weight_round(const FieldArgs& a, float sigma, bool act, int idx, int j, int l, float nrm, float& carry, float& ds) {
  const float zj = act ? a.z[idx] : 0.f;
  const float zn = (j + 1 < a.S) ? a.z[idx + 1] : zj;
  ds = ((j + 1 < a.S) ? (zn - zj) : 0.0f) * nrm * a.distance_scale;
  const float alpha = 1.0f - expf(-sigma * ds);
  const float p = act ? one_minus_alpha_eps(alpha) : 1.0f;
  const float incl = W == 64 ? scan_mul64(p, l) : scan_mul32(p, l);
  float excl = __shfl_up(incl, 1, W);
  if (l == 0) excl = 1.0f;
  const float T = carry * excl;
  const float wt = alpha * T;
  carry *= __shfl(incl, W - 1, W);
  return wt;
}

// The second sweep of the app-mask compaction: ray n's entries go to a.list from `base` on, read back from the weights the
// lane stored in its rounds (same lane, program order).  `on`: the lane takes part (its ray exists; the writing half).
template <int W>
RDRF_D void append_masked(const FieldArgs& a, int base, int n, bool on, int l) {
  for (int j0 = 0; j0 < a.S; j0 += W) {
    const int j = j0 + l;
    const bool act = on && j < a.S;
    const int idx = n * a.S + (act ? j : 0);
    const bool m = act && a.weight[idx] > a.weight_thres;   // the lane's own store above
    const unsigned long long bal = __ballot(m);
    if (m) a.list[base + ballot_rank(bal)] = idx;
    base += __popcll(bal);
  }
}

// The appearance phase writes the masked samples only: zero the colours of the round [j0, j0 + W) of ray n (coalesced)
template <int W>
RDRF_D void zero_rgb_round(float* rgb, int n, int S, int j0, int l) {
  float* r = rgb + ((size_t)n * S + j0) * 3 + l;
  const int lim = (S - j0 < W ? S - j0 : W) * 3;
  if (l < lim) r[0] = 0.f;
  if (l + W < lim) r[W] = 0.f;
  if (l + 2 * W < lim) r[2 * W] = 0.f;
}

template <bool FEAT, bool FUSED = false>
RDRF_D void static_density_body(const FieldArgs a, const StaticW w, const GridCtx gc) {
  __shared__ int s_cnt[16];
  const int lane = GC_TID & 63;
  const int wave_ = GC_TID >> 6, nwaves_ = GC_NTHR >> 6;
  for (int nb = GC_BID * nwaves_; nb < a.N; nb += GC_NBLK * nwaves_) {   // uniform over the workgroup (block_append_base syncs)
  const bool ray = nb + wave_ < a.N;
  const int n = ray ? nb + wave_ : 0;
  float vx, vy, vz;
  float nrm = 1.0f;
  if constexpr (!FEAT) nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
  float carry = 1.0f;
  int cnt = 0;   // app-masked samples of the ray (wave-uniform)
  for (int j0 = 0; j0 < a.S; j0 += 64) {
    const int j = j0 + lane;
    const bool act = ray && j < a.S && (!FEAT || n * a.S + j < a.M);
    const int idx = n * a.S + (act ? j : 0);
    const bool vld = act && (FEAT || a.valid[idx] != 0);
    if constexpr (!FEAT) {
      if (ray && a.rgb != nullptr) zero_rgb_round<64>(a.rgb, n, a.S, j0, lane);
    }
    float f = 0.0f;
    if (vld) {
      float x0, x1, x2;
      if (FEAT && a.in_norm) {
        x0 = a.xyz[idx * 3 + 0]; x1 = a.xyz[idx * 3 + 1]; x2 = a.xyz[idx * 3 + 2];
      } else {
        x0 = norm_c(a.xyz[idx * 3 + 0], a.box.lo[0], a.box.inv[0]);
        x1 = norm_c(a.xyz[idx * 3 + 1], a.box.lo[1], a.box.inv[1]);
        x2 = norm_c(a.xyz[idx * 3 + 2], a.box.lo[2], a.box.inv[2]);
      }
      f = static_density_feature(w.density, x0, x1, x2);
    }
    if (a.raw != nullptr && act) a.raw[idx] = f;
    if constexpr (FEAT) {  // compute_densityfeature: the raw feature (models/tensoRF.py:118-154)
      if (act && a.sigma != nullptr) a.sigma[idx] = f;
    } else {
      const float sigma = vld ? density_act(f, a.act, a.density_shift) : 0.0f;
      float ds;
      const float wt = weight_round<64>(a, sigma, act, idx, j, lane, nrm, carry, ds);
      if (act) {
        a.sigma[idx] = sigma;
        a.weight[idx] = wt;
        a.dists[idx] = ds;
      }
      cnt += __popcll(__ballot(act && wt > a.weight_thres));
    }
  }
  if constexpr (!FEAT) {
    const int base = block_append_base(a.counter, cnt, s_cnt, GC_TID, GC_NTHR);
    if (cnt) append_masked<64>(a, base, n, ray, lane);
  }
  }  // ray loop
}

template <int HEAD, bool FEAT, bool SAVE = true, bool FUSED = false>
RDRF_D void static_app_body(const FieldArgs a, const StaticW w, float* lds_fused, const GridCtx gc) {
  float* lds;
  if constexpr (FUSED) lds = lds_fused;
  else {   // the standalone kernel owns its image as a named LDS array (constant addresses in every ds_read)
    __shared__ __attribute__((aligned(16))) float lds_own[pk::S3_SIZE];
    lds = lds_own;
  }
  __shared__ int s_next;
  if (GC_TID == 0) s_next = GC_NTHR >> 6;
  lds_fill(lds, a.pk + pk::REG_S3, pk::S3_SIZE);
  const int lane = GC_TID & 63, h = lane >> 5, s = lane & 31;
  const int wave = GC_TID >> 6, nwaves = GC_NTHR >> 6;
  const int count = FEAT ? a.M : *a.counter;
  const int ntiles = (count + 31) >> 5;
  const float* pkw = lds;
  const bool dynq = !FUSED && (a.dynq & 1) != 0;
  for (int k = wave, tile; (tile = GC_BID + k * GC_NBLK) < ntiles; k = tile_queue_next(&s_next, k, nwaves, dynq)) {
    const int li = tile * 32 + s;
    const bool act = li < count;
    const int idx = act ? (FEAT ? li : a.list[li]) : 0;
    const int n = idx / a.S;
    float* svb = (SAVE && a.act3) ? a.act3 + (size_t)tile * sv::S3_ROWS * 32 : nullptr;
    float vx = 0.f, vy = 0.f, vz = 0.f;
    if constexpr (!FEAT) ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
    float x0, x1, x2;
    if (FEAT && a.in_norm) {
      x0 = a.xyz[idx * 3 + 0]; x1 = a.xyz[idx * 3 + 1]; x2 = a.xyz[idx * 3 + 2];
    } else {
      x0 = norm_c(a.xyz[idx * 3 + 0], a.box.lo[0], a.box.inv[0]);
      x1 = norm_c(a.xyz[idx * 3 + 1], a.box.lo[1], a.box.inv[1]);
      x2 = norm_c(a.xyz[idx * 3 + 2], a.box.lo[2], a.box.inv[2]);
    }
    float G[36];
    gather_level_app<0>(w.app, point_taps(w.app, x0, x1, x2, 0), h, G);
    if (!act) {
#pragma unroll
      for (int i = 0; i < 36; ++i) G[i] = 0.f;
    }
    f32x16 accF[1];
    acc_bias<1>(accF, nullptr, h);
    mfma_seg<1, 36>(accF, G, pkw + pk::S3_BASIS, lane);
    float F[16];
    acc_copy<1>(F, accF);
    if constexpr (FEAT) {  // compute_appfeature: basis_mat output (models/tensoRF.py:156-196)
      save_rows<36>(svb, sv::S3_G, G, s, h);
      if (act) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
          if (elem_of(kk, h) < 27) a.feat[(size_t)idx * 27 + elem_of(kk, h)] = F[kk];
      }
      continue;
    }
    float P[64];
    {
      float fmax_ = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) fmax_ = fmaxf(fmax_, fabsf(F[r]));
      if (__builtin_expect(__any(!(fmax_ * 2.0f <= RDRF_PE_FAST_MAX)), 0)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float s1, c1, s2, c2;
          sincosf(F[r], &s1, &c1);
          sincosf(F[r] * 2.0f, &s2, &c2);
          P[4 * r + 0] = s1; P[4 * r + 1] = c1; P[4 * r + 2] = s2; P[4 * r + 3] = c2;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float s1, c1, s2, c2;
          sincos_sel<true>(F[r], s1, c1);
          sincos_double(s1, c1, s2, c2);   // (sin 2F, cos 2F): rdrf_common.hpp
          P[4 * r + 0] = s1; P[4 * r + 1] = c1; P[4 * r + 2] = s2; P[4 * r + 3] = c2;
        }
      }
    }
    if (HEAD == RDRF_HEAD_MLP_FEA) {  // viewdirs ride in the pad slots 27..29 of the feature block
      if (h == 0) F[15] = vx;
      else { F[12] = vy; F[13] = vz; }
    }
    if (svb != nullptr && h == 0) {
      svb[(size_t)(sv::S3_VD + 0) * 32 + s] = vx; svb[(size_t)(sv::S3_VD + 1) * 32 + s] = vy;
      svb[(size_t)(sv::S3_VD + 2) * 32 + s] = vz;
    }
    save_rows<36>(svb, sv::S3_G, G, s, h);
    save_rows<16>(svb, sv::S3_F, F, s, h);
    save_rows<64>(svb, sv::S3_P, P, s, h);
    f32x16 acc[4];
    acc_bias<4>(acc, pkw + pk::S3_B1, h);
    float H1[64];
#ifdef RDRF_APP_F32
    mfma_seg<4, 16>(acc, F, pkw + pk::S3_W1_F, lane);
    mfma_seg<4, 64>(acc, P, pkw + pk::S3_W1_P, lane);
    acc_relu<4>(H1, acc);
    save_rows<64>(svb, sv::S3_H1, H1, s, h);
    acc_bias<4>(acc, pkw + pk::S3_B2, h);
    mfma_seg<4, 64>(acc, H1, pkw + pk::S3_W2, lane);
#else
    {  // the two hidden layers on the bf16 matrix pipe (fp32-grade bf16 x 3, lo pieces streamed from the pack buffer)
      const B3sLo st = b3s_lo_stream(a.pk + pk::REG_S3_LO, lane);
      u32x4 lo[4];
      b3s_lo_load<4>(lo, st, pk::S3_LO_W1_F, 2, 0);
      mfma_seg_b3s<4, 16, 64>(acc, F, pkw + pk::S3_W1_F, st, pk::S3_LO_W1_F, pk::S3_LO_W1_P, lo, lane);
      mfma_seg_b3s<4, 64, 64>(acc, P, pkw + pk::S3_W1_P, st, pk::S3_LO_W1_P, pk::S3_LO_W2, lo, lane);
      acc_relu<4>(H1, acc);
      save_rows<64>(svb, sv::S3_H1, H1, s, h);
      acc_bias<4>(acc, pkw + pk::S3_B2, h);
      mfma_seg_b3s<4, 64, 0>(acc, H1, pkw + pk::S3_W2, st, pk::S3_LO_W2, 0, lo, lane);
    }
#endif
    acc_relu<4>(H1, acc);
    save_rows<64>(svb, sv::S3_H2, H1, s, h);
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float v = dot_small<64>(H1, pkw + pk::S3_W3 + o * 128, h) + w.b3[o];
      if (HEAD == RDRF_HEAD_MLP_FEA_TIMEEMBEDDING)
        v += w.w3[o * 131 + 128] * vx + w.w3[o * 131 + 129] * vy + w.w3[o * 131 + 130] * vz;
      if (act && h == 0) a.rgb[(size_t)idx * 3 + o] = sigmoidf_(v);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// One sample of the dynamic field's density phase, in the lane layout of mfma_seg (sample s of a 32-sample tile in the
// lanes s and s + 32, half h).  pkw: the pk::REG_K1 image in LDS.  svb: the tile's block of saved rows, or nullptr
// (save_rows on a null base is a no-op: the inference callers pass nullptr and the stores fold away).  An MFMA column
// depends on its own sample only, so every caller gets the same bits for a sample whatever shares its tile.
// ------------------------------------------------------------------------------------------------
// row `row` of the time-branch outputs [.][32] in the slot order of SEG_WARP3_T (`row`: int or size_t, as the caller indexes)
template <typename I>
RDRF_D void load_tout(float (&T)[16], const float* tout, I row, int h) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 v = ld4(tout + row * 32 + 8 * q + 4 * h);
    T[q * 4 + 0] = v.x; T[q * 4 + 1] = v.y; T[q * 4 + 2] = v.z; T[q * 4 + 3] = v.w;
  }
}

// warp MLP: [xn, PE10(xn), tout] -> 64 -> 64 -> 3  (models/tensoRF.py:521-541).  The callers off the training path
// (k_alpha_dyn, k_dyn_density_list); dyn_density_body holds the same lines in place, see there.
RDRF_D void warp_mlp(float (&d)[3], const float (&X0)[32], const float (&T)[16], const float* pkw, const float* l5b,
                     float* svb, int s, int h, int lane) {
  f32x16 acc[2];
  acc_bias<2>(acc, pkw + pk::K1_B3, h);
  mfma_seg<2, 32>(acc, X0, pkw + pk::K1_W3_X0, lane);
  mfma_seg<2, 16>(acc, T, pkw + pk::K1_W3_T, lane);
  float H3[32];
  acc_relu<2>(H3, acc);
  save_rows<32>(svb, sv::K1_H3, H3, s, h);
  acc_bias<2>(acc, pkw + pk::K1_B4, h);
  mfma_seg<2, 32>(acc, H3, pkw + pk::K1_W4, lane);
  acc_relu<2>(H3, acc);
  save_rows<32>(svb, sv::K1_H4, H3, s, h);
#pragma unroll
  for (int o = 0; o < 3; ++o) d[o] = dot_small<32>(H3, pkw + pk::K1_W5 + o * 64, h) + l5b[o];
}

// the warped point in normalised coordinates: the un-normalised round trip of xn (models/tensoRF.py:647-649)
RDRF_D void warp_point(float (&xw)[3], const float (&xn)[3], const float (&d)[3], const Box& box) {
#pragma unroll
  for (int c = 0; c < 3; ++c) xw[c] = norm_c(unnorm_c(xn[c], box.lo[c], box.inv[c]) + d[c], box.lo[c], box.inv[c]);
}

// density (BLEND = false) or blending head at the warped point: 3-stride VM features (72) + X0 + X1 -> 64 -> 1, the raw
// output.  vld = false zeroes the column's features.
template <bool BLEND>
RDRF_D float head_raw(const DynW& w, const float (&xw)[3], bool vld, const float (&X0)[32], const float (&X1)[8],
                      const float* __restrict__ pkw, float* svb, int s, int h, int lane) {
  const RdrfVM& set = BLEND ? w.blending : w.density;
  float Fv[36];
  gather_level_den<0>(set, point_taps(set, xw[0], xw[1], xw[2], 0), h, Fv);
  gather_level_den<12>(set, point_taps(set, xw[0], xw[1], xw[2], 1), h, Fv);
  gather_level_den<24>(set, point_taps(set, xw[0], xw[1], xw[2], 2), h, Fv);
  if (!vld) {
#pragma unroll
    for (int i = 0; i < 36; ++i) Fv[i] = 0.f;
  }
  f32x16 acc[2];
  acc_bias<2>(acc, pkw + (BLEND ? pk::K1_BB1 : pk::K1_BD1), h);
#ifdef RDRF_HEADS_F32
  mfma_seg<2, 36>(acc, Fv, pkw + (BLEND ? pk::K1_BLE1_F : pk::K1_DEN1_F), lane);
  mfma_seg<2, 32>(acc, X0, pkw + (BLEND ? pk::K1_BLE1_X0 : pk::K1_DEN1_X0), lane);
  mfma_seg<2, 8>(acc, X1, pkw + (BLEND ? pk::K1_BLE1_X1 : pk::K1_DEN1_X1), lane);
#else
  {  // the first layer (152 -> 64) on the bf16 matrix pipe: [features 36 | X0 32 | X1 0..3] as nine K = 16 steps of
     // mfma_seg_b3, X1[4..7] as an fp32 segment (pk::K1_DEN1)
    float U[pk::K1_HEAD_KK];
#pragma unroll
    for (int i = 0; i < 36; ++i) U[i] = Fv[i];
#pragma unroll
    for (int i = 0; i < 32; ++i) U[36 + i] = X0[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) U[68 + i] = X1[i];
    mfma_seg_b3<2, pk::K1_HEAD_KK>(acc, U, pkw + (BLEND ? pk::K1_BLE1 : pk::K1_DEN1), lane);
    const float V[4] = {X1[4], X1[5], X1[6], X1[7]};
    mfma_seg<2, 4>(acc, V, pkw + (BLEND ? pk::K1_BLE1_X1T : pk::K1_DEN1_X1T), lane);
  }
#endif
  float Hd[32];
  acc_relu<2>(Hd, acc);
  save_rows<36>(svb, BLEND ? sv::K1_FB : sv::K1_FD, Fv, s, h);
  save_rows<32>(svb, BLEND ? sv::K1_HB : sv::K1_HD, Hd, s, h);
  return dot_small<32>(Hd, pkw + (BLEND ? pk::K1_BLE2 : pk::K1_DEN2), h) + (BLEND ? w.bb2 : w.db2)[0];
}

// FLAT: the unit of work is a 32-sample tile of the flattened [N * S] sample array instead of a ray, so no tile is padded
// to the ray's end (S = 115: 3.6 tiles per ray instead of 4; S = 13: 0.41 instead of 1) and a 512-ray eval chunk is 1840
// tiles for the 2048 resident waves instead of 512 rays.  The tiles come from the workgroup's queue (tile_queue_next).  The
// per-ray constants (time, tout, PE8(t)) are fetched per lane through the sample's ray index; sigma and blending (and in
// training the raw head outputs and the saved rows of tile `n`) are written per sample, and the transmittance scan /
// app-mask compaction run afterwards in ray_scan_body (same arithmetic in the same order: results are bit-identical to the
// wave-per-ray form).  The backward kernels address the saved rows by flat tile as well (k_dyn_density_bwd<., ., true>).
template <bool FEAT, bool SAVE = true, bool FUSED = false, bool FLAT = false>
RDRF_D void dyn_density_body(const FieldArgs a, const DynW w, float* lds_fused, const GridCtx gc) {
  static_assert(!FLAT || (!FEAT && !FUSED), "the flat-tile form is a ray-path kernel of its own");
  float* lds;
  if constexpr (FUSED) lds = lds_fused;
  else {   // the standalone kernel owns its image as a named LDS array (constant addresses in every ds_read)
    __shared__ __attribute__((aligned(16))) float lds_own[pk::K1_SIZE];
    lds = lds_own;
  }
  const int lane = GC_TID & 63, h = lane >> 5, s = lane & 31;
  const int wave = GC_TID >> 6, nwaves = GC_NTHR >> 6;
  __shared__ int s_next;   // FLAT: the workgroup's tile queue
  if (FLAT && GC_TID == 0) s_next = nwaves;
  lds_fill(lds, a.pk + pk::REG_K1, pk::K1_SIZE);
  const float* pkw = lds;
  const int nunits = FLAT ? (int)(((long)a.N * a.S + 31) >> 5) : a.N;
  const bool dynq = FLAT && (a.dynq & 1) != 0;
  int k = wave;   // FLAT: queue position of the wave's current tile (tile = block + k * blocks)
  for (int n = FLAT ? GC_BID + k * GC_NBLK : GC_BID * nwaves + wave; n < nunits;
       n = FLAT ? GC_BID + (k = tile_queue_next(&s_next, k, nwaves, dynq)) * GC_NBLK : n + GC_NBLK * nwaves) {
  float t = 0.f, nrm = 1.0f;
  float T[16];
  float X1[8];
  if constexpr (!FEAT && !FLAT) {   // time is per ray: tout / PE8(t) are per-ray constants
    t = a.ts[n];
    float vx, vy, vz;
    nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
    load_tout(T, a.tout, n, h);
    fill_x1(X1, t, h);
  }
  float carry = 1.0f;
  int nmask = 0;   // app-masked samples of the ray (wave-uniform)
  for (int j0 = 0; j0 < (FLAT ? 32 : a.S); j0 += 32) {
    const int j = j0 + s;
    bool act;
    int idx;
    if constexpr (FLAT) {   // n = tile of the flattened sample array
      const long i = (long)n * 32 + s;
      act = i < (long)a.N * a.S;
      idx = act ? (int)i : 0;
    } else {
      act = j < a.S && (!FEAT || n * a.S + j < a.M);
      idx = n * a.S + (act ? j : 0);
    }
    const bool vld = act && (FEAT || a.valid[idx] != 0);
    if constexpr (FEAT || FLAT) {  // time is per point (FEAT) / looked up through the sample's ray (FLAT)
      const int ti = FLAT ? idx / a.S : idx;
      t = a.ts[ti];
      load_tout(T, a.tout, (size_t)ti, h);
      fill_x1(X1, t, h);
    }
    // the per-ray time-branch outputs are re-read per tile (L1 hits) instead of living in 16 registers across the tiles: the
    // training instantiation loses its 29 spilled registers (104 B of scratch per lane): kernel -6 % / -7 % (stage 0 / final,
    // profiles/r06_ab_t_reload.txt).  Same loads, same bits.
    if constexpr (!FEAT && !FLAT) {
      int nn = n;
      asm volatile("" : "+v"(nn));
      load_tout(T, a.tout, nn, h);
    }
    const float px[3] = {a.xyz[idx * 3 + 0], a.xyz[idx * 3 + 1], a.xyz[idx * 3 + 2]};
    const bool raw_in = FEAT && a.in_norm;   // compute_*: the caller hands normalised coordinates
    float xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xn[c] = raw_in ? px[c] : norm_c(px[c], a.box.lo[c], a.box.inv[c]);
    float X0[32];
    fill_x0(X0, xn[0], xn[1], xn[2], t, h);
    float* svb = (SAVE && a.act1) ? a.act1 + (FLAT ? (size_t)n : (size_t)n * ((a.S + 31) >> 5) + (j0 >> 5)) * sv::K1_ROWS * 32 : nullptr;
    save_rows<32>(svb, sv::K1_X0, X0, s, h);
    save_rows<8>(svb, sv::K1_X1, X1, s, h);
    save_rows<16>(svb, sv::K1_T, T, s, h);
    float d[3], xw[3];
    // warp_mlp, written out: called as a function here, the compiler orders the bf16 MFMAs of the heads below differently and
    // k_dyn_density<false, false> falls under the WAR distance tests/test_mfma_hazards_cpu.py holds it to (9 < 11).  Keep the
    // two in step: tests/test_gpu_alpha.py and tests/test_gpu_masked_render.py compare their bits.
    {
      f32x16 acc[2];
      acc_bias<2>(acc, pkw + pk::K1_B3, h);
      mfma_seg<2, 32>(acc, X0, pkw + pk::K1_W3_X0, lane);
      mfma_seg<2, 16>(acc, T, pkw + pk::K1_W3_T, lane);
      float H3[32];
      acc_relu<2>(H3, acc);
      save_rows<32>(svb, sv::K1_H3, H3, s, h);
      acc_bias<2>(acc, pkw + pk::K1_B4, h);
      mfma_seg<2, 32>(acc, H3, pkw + pk::K1_W4, lane);
      acc_relu<2>(H3, acc);
      save_rows<32>(svb, sv::K1_H4, H3, s, h);
      d[0] = dot_small<32>(H3, pkw + pk::K1_W5 + 0 * 64, h) + w.l5b[0];
      d[1] = dot_small<32>(H3, pkw + pk::K1_W5 + 1 * 64, h) + w.l5b[1];
      d[2] = dot_small<32>(H3, pkw + pk::K1_W5 + 2 * 64, h) + w.l5b[2];
    }
    warp_point(xw, xn, d, a.box);
    if (act && h == 0) {
      if (!FEAT || a.xyz_prime != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          a.xyz_prime[(size_t)idx * 3 + c] = (raw_in ? unnorm_c(xn[c], a.box.lo[c], a.box.inv[c]) : px[c]) + d[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) a.xw[(size_t)idx * 3 + c] = xw[c];
    }
    const float fd = head_raw<false>(w, xw, vld, X0, X1, pkw, svb, s, h, lane);
    const float fb = head_raw<true>(w, xw, vld, X0, X1, pkw, svb, s, h, lane);
    if constexpr (FEAT) {  // compute_densityfeature / compute_blendingfeature: the raw head outputs
      if (act && h == 0) {
        if (a.sigma != nullptr) a.sigma[idx] = fd;
        if (a.blending != nullptr) a.blending[idx] = fb;
        if (a.raw != nullptr) { a.raw[(size_t)idx * 2] = fd; a.raw[(size_t)idx * 2 + 1] = fb; }
      }
    } else if constexpr (FLAT) {   // the scan and the compaction follow in ray_scan_body
      if (act && h == 0) {
        a.sigma[idx] = vld ? density_act(fd, a.act, a.density_shift) : 0.0f;
        a.blending[idx] = vld ? sigmoidf_(fb) : 0.0f;
        if (SAVE && a.raw != nullptr) { a.raw[(size_t)idx * 2] = fd; a.raw[(size_t)idx * 2 + 1] = fb; }
      }
    } else {
    const float sigma = vld ? density_act(fd, a.act, a.density_shift) : 0.0f;
    const float blend = vld ? sigmoidf_(fb) : 0.0f;
    float ds;
    const float wt = weight_round<32>(a, sigma, act, idx, j, s, nrm, carry, ds);
    const bool m = act && h == 0 && wt > a.weight_thres;
    if (act && h == 0) {
      a.sigma[idx] = sigma;
      a.weight[idx] = wt;
      a.dists[idx] = ds;
      a.blending[idx] = blend;
      if (SAVE && a.raw != nullptr) { a.raw[(size_t)idx * 2] = fd; a.raw[(size_t)idx * 2 + 1] = fb; }
    }
    nmask += __popcll(__ballot(m));
    }
  }
  if constexpr (!FEAT && !FLAT) {
    // app-mask compaction (models/tensorBase.py:773-790), ONE append per ray: every append is an atomic with return on the
    // same address for the whole chip (~3.6 ns each, serialised at the memory side), so the ray's tiles count first and
    // the entries are written in a second sweep over the weights just stored (append_masked)
    if (nmask) {
      int base = 0;
      if (lane == 0) base = atomicAdd(a.counter, nmask);
      base = __shfl(base, 0, 64);
      append_masked<32>(a, base, n, h == 0, s);
    }
  }
  }  // ray loop
}

// The per-ray half of the density phase for the flat-tile form: sigma -> alpha -> transmittance scan -> weight, dists, the
// app-mask compaction (models/tensorBase.py:773-790) and the zero fill of the colours the appearance phase will not write.
// A half-wave per ray (two rays per wave), 32 samples per round with the carry across rounds -- weight_round<32>, the round
// of the wave-per-ray dyn_density_body, so weight / dists / the mask come out bit-identical.
// The compaction appends ONCE per workgroup (block_append_base).
RDRF_D void ray_scan_body(const FieldArgs a) {
  __shared__ int s_cnt[16];
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int n_ = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 2 + h;
  const bool ray = n_ < a.N;
  const int n = ray ? n_ : 0;
  float vx, vy, vz;
  const float nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
  float carry = 1.0f;
  int cnt = 0;
  for (int j0 = 0; j0 < a.S; j0 += 32) {
    const int j = j0 + s;
    const bool act = ray && j < a.S;
    const int idx = n * a.S + (act ? j : 0);
    const float sigma = act ? a.sigma[idx] : 0.0f;
    float ds;
    const float wt = weight_round<32>(a, sigma, act, idx, j, s, nrm, carry, ds);
    if (act) {
      a.weight[idx] = wt;
      a.dists[idx] = ds;
    }
    if (ray && a.rgb != nullptr) zero_rgb_round<32>(a.rgb, n, a.S, j0, s);
    cnt += __popcll(__ballot(act && wt > a.weight_thres));
  }
  const int base = block_append_base(a.counter, cnt, s_cnt, threadIdx.x, blockDim.x);
  if (cnt) append_masked<32>(a, base, n, ray, s);
}

template <bool FEAT, bool SAVE = true, bool FUSED = false>
RDRF_D void dyn_app_body(const FieldArgs a, const DynW w, float* lds_fused, const GridCtx gc) {
  float* lds;
  if constexpr (FUSED) lds = lds_fused;
  else {   // the standalone kernel owns its image as a named LDS array (constant addresses in every ds_read)
    __shared__ __attribute__((aligned(16))) float lds_own[pk::K3_SIZE];
    lds = lds_own;
  }
  __shared__ int s_next;
  if (GC_TID == 0) s_next = GC_NTHR >> 6;
  lds_fill(lds, a.pk + pk::REG_K3, pk::K3_SIZE);
  const int lane = GC_TID & 63, h = lane >> 5, s = lane & 31;
  const int wave = GC_TID >> 6, nwaves = GC_NTHR >> 6;
  const int count = FEAT ? a.M : *a.counter;
  const int ntiles = (count + 31) >> 5;
  const float* pkw = lds;
  const bool dynq = !FUSED && (a.dynq & 1) != 0;   // tile queue of the workgroup (tile_queue_next)
  for (int k = wave, tile; (tile = GC_BID + k * GC_NBLK) < ntiles; k = tile_queue_next(&s_next, k, nwaves, dynq)) {
    const int li = tile * 32 + s;
    const bool act = li < count;
    const int idx = act ? (FEAT ? li : a.list[li]) : 0;
    const int n = idx / a.S;
    const float t = FEAT ? 0.f : a.ts[n];
    float* svb = (SAVE && a.act3) ? a.act3 + (size_t)tile * sv::K3_ROWS * 32 : nullptr;
    float vx = 0.f, vy = 0.f, vz = 0.f;
    float xn0 = 0.f, xn1 = 0.f, xn2 = 0.f;
    if constexpr (!FEAT) {
      ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
      xn0 = norm_c(a.xyz[idx * 3 + 0], a.box.lo[0], a.box.inv[0]);
      xn1 = norm_c(a.xyz[idx * 3 + 1], a.box.lo[1], a.box.inv[1]);
      xn2 = norm_c(a.xyz[idx * 3 + 2], a.box.lo[2], a.box.inv[2]);
    }
    const float xw0 = a.xw[(size_t)idx * 3 + 0], xw1 = a.xw[(size_t)idx * 3 + 1], xw2 = a.xw[(size_t)idx * 3 + 2];
    float F[16];
    {
      // level by level: gather a level's 36 features (two load batches), feed them to the basis product, store their
      // rows -- the 108 gathered values never coexist, which leaves the registers for 36 loads in flight
      f32x16 accF[1];
      acc_bias<1>(accF, nullptr, h);
      {
        float A[36];
        gather_level_app<0>(w.app, point_taps(w.app, xw0, xw1, xw2, 0), h, A);
        if (!act) {
#pragma unroll
          for (int i = 0; i < 36; ++i) A[i] = 0.f;
        }
        mfma_seg<1, 36>(accF, A, pkw + pk::K3_BASIS, lane);
        save_rows<36>(svb, sv::K3_A, A, s, h);
      }
      {
        float A[36];
        gather_level_app<0>(w.app, point_taps(w.app, xw0, xw1, xw2, 1), h, A);
        if (!act) {
#pragma unroll
          for (int i = 0; i < 36; ++i) A[i] = 0.f;
        }
        mfma_seg<1, 36>(accF, A, pkw + pk::K3_BASIS + 9 * 256, lane);
        save_rows<36>(svb, sv::K3_A + 72, A, s, h);
      }
      {
        float A[36];
        gather_level_app<0>(w.app, point_taps(w.app, xw0, xw1, xw2, 2), h, A);
        if (!act) {
#pragma unroll
          for (int i = 0; i < 36; ++i) A[i] = 0.f;
        }
        mfma_seg<1, 36>(accF, A, pkw + pk::K3_BASIS + 18 * 256, lane);
        save_rows<36>(svb, sv::K3_A + 144, A, s, h);
      }
      acc_copy<1>(F, accF);
    }
    if constexpr (FEAT) {  // compute_appfeature: basis_mat output (models/tensoRF.py:734-811)
      if (act) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
          if (elem_of(kk, h) < 27) a.feat[(size_t)idx * 27 + elem_of(kk, h)] = F[kk];
      }
      continue;
    }
    float X0[32], X1[8];
    fill_x0(X0, xn0, xn1, xn2, t, h);
    fill_x1(X1, t, h);
    if (svb != nullptr && h == 0) {
      svb[(size_t)(sv::K3_VD + 0) * 32 + s] = vx; svb[(size_t)(sv::K3_VD + 1) * 32 + s] = vy;
      svb[(size_t)(sv::K3_VD + 2) * 32 + s] = vz;
    }
    save_rows<16>(svb, sv::K3_F, F, s, h);
    save_rows<32>(svb, sv::K3_X0, X0, s, h);
    save_rows<8>(svb, sv::K3_X1, X1, s, h);
    f32x16 acc[4];
    acc_bias<4>(acc, pkw + pk::K3_B1, h);
    float H1[64];
#ifdef RDRF_APP_F32
    mfma_seg<4, 16>(acc, F, pkw + pk::K3_RGB1_F, lane);
    mfma_seg<4, 32>(acc, X0, pkw + pk::K3_RGB1_X0, lane);
    mfma_seg<4, 8>(acc, X1, pkw + pk::K3_RGB1_X1, lane);
    acc_relu<4>(H1, acc);
    save_rows<64>(svb, sv::K3_H1, H1, s, h);
    acc_bias<4>(acc, pkw + pk::K3_B2, h);
    mfma_seg<4, 64>(acc, H1, pkw + pk::K3_RGB2, lane);
#else
    {  // the two hidden layers on the bf16 matrix pipe (fp32-grade bf16 x 3, lo pieces streamed from the pack buffer)
      const B3sLo st = b3s_lo_stream(a.pk + pk::REG_K3_LO, lane);
      u32x4 lo[4];
      b3s_lo_load<4>(lo, st, pk::K3_LO_RGB1_F, 2, 0);
      mfma_seg_b3s<4, 16, 32>(acc, F, pkw + pk::K3_RGB1_F, st, pk::K3_LO_RGB1_F, pk::K3_LO_RGB1_X0, lo, lane);
      mfma_seg_b3s<4, 32, 8>(acc, X0, pkw + pk::K3_RGB1_X0, st, pk::K3_LO_RGB1_X0, pk::K3_LO_RGB1_X1, lo, lane);
      mfma_seg_b3s<4, 8, 64>(acc, X1, pkw + pk::K3_RGB1_X1, st, pk::K3_LO_RGB1_X1, pk::K3_LO_RGB2, lo, lane);
      acc_relu<4>(H1, acc);
      save_rows<64>(svb, sv::K3_H1, H1, s, h);
      acc_bias<4>(acc, pkw + pk::K3_B2, h);
      mfma_seg_b3s<4, 64, 0>(acc, H1, pkw + pk::K3_RGB2, st, pk::K3_LO_RGB2, 0, lo, lane);
    }
#endif
    acc_relu<4>(H1, acc);
    save_rows<64>(svb, sv::K3_H2, H1, s, h);
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float v = dot_small<64>(H1, pkw + pk::K3_RGBV + o * 128, h) + w.rbv[o];
      v += w.rwv[o * 131 + 128] * vx + w.rwv[o * 131 + 129] * vy + w.rwv[o * 131 + 130] * vz;
      if (act && h == 0) a.rgb[(size_t)idx * 3 + o] = sigmoidf_(v);
    }
  }
}

// time branch of the dynamic field for the rays [0, N): 32 lanes per ray (lane o: hidden neurons o and o + 32, then
// output o); s_h: [threads / 32][64] floats of LDS.  Every thread of the block must call (barriers inside).
template <bool FUSED = false>
RDRF_D void time_branch_body(const float* __restrict__ ts, const DynW w, int N, float* __restrict__ tout, float* s_h,
                             const GridCtx gc) {
  const int rpb = GC_NTHR >> 5;
  const int r = GC_TID >> 5, o = GC_TID & 31;
  for (int base = GC_BID * rpb; base < N; base += GC_NBLK * rpb) {
    const int n = base + r;
    const bool act = n < N;
    const float t = act ? ts[n] : 0.f;
    float tin[17];
    tin[0] = t;
#pragma unroll
    for (int f = 0; f < 8; ++f) sincosf(ldexpf(t, f), &tin[1 + f], &tin[9 + f]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = o + 32 * j;
      float hk = w.l1b[k];
#pragma unroll
      for (int i = 0; i < 17; ++i) hk = fmaf(w.l1w[k * 17 + i], tin[i], hk);
      s_h[r * 64 + k] = fmaxf(hk, 0.0f);
    }
    __syncthreads();
    float out = 0.f;
    if (o < 30) {
      out = w.l2b[o];
      for (int k = 0; k < 64; ++k) out = fmaf(w.l2w[o * 64 + k], s_h[r * 64 + k], out);   // k ascending, as before
    }
    if (act) tout[n * 32 + o] = out;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// scene-flow MLP (models/tensoRF.py:446-462) of one sample in the lane layout of mfma_seg: shared by k_scene_flow
// (rdrf_fwd.hip), the evaluation render's k_motion_maps (rdrf_motion.hip) and k_track_points (rdrf_track.hip).
// fill_sf_x: the input [xn3, PE4(xn), t, PE4(t)] in the slot order of SEG_SF_X
// ------------------------------------------------------------------------------------------------
RDRF_D void fill_sf_x(float (&X)[20], float xn0, float xn1, float xn2, float t, int h) {
#pragma unroll
  for (int o = 0; o < 5; ++o) {
    if (o == 0 && h == 0) {
      X[0] = xn0; X[1] = xn1; X[2] = xn2; X[3] = t;
    } else {
      const int k = 2 * o + h - 1;
      // (exact sin / cos for every octave here: the scene-flow losses are L1 terms, and with the doubled-angle form of
      // rdrf_common.hpp sincos_double one sign flip of a ~0 flow component moved the nvidia_late reference-trainer
      // comparison by 8e-4 of a gradient's max -- the kernel is 0.15 ms of the step, the 60 VALU instructions stay)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int pr = 2 * k + p;
        float sv = 0.f, cv = 0.f;
        if (pr < 16) {
          const int d = pr >> 2, f = pr & 3;
          const float x = pr < 12 ? (d == 0 ? xn0 : (d == 1 ? xn1 : xn2)) : t;
          const float a_ = ldexpf(x, f);
          if (__builtin_expect(!(fabsf(a_) <= RDRF_PE_FAST_MAX), 0)) sincosf(a_, &sv, &cv);
          else sincos_sel<true>(a_, sv, cv);
        }
        X[o * 4 + 2 * p] = sv;
        X[o * 4 + 2 * p + 1] = cv;
      }
    }
  }
}

// 36 -> 64 -> 64 -> 64 -> 6 on X = fill_sf_x(...): sf[0..2] forward, sf[3..5] backward flow, in both half-waves.  pkw: the
// pk::REG_SF image in LDS; b6: the last layer's bias; svb: the tile's saved rows or nullptr (save_rows is then a no-op)
RDRF_D void sf_mlp(float (&sf)[6], const float (&X)[20], const float* pkw, const float* b6, float* svb, int s, int h,
                   int lane) {
  f32x16 acc[2];
  acc_bias<2>(acc, pkw + pk::SF_B0, h);
  mfma_seg<2, 20>(acc, X, pkw + pk::SF_W0, lane);
  float H[32];
  acc_relu<2>(H, acc);
  save_rows<32>(svb, sv::SF_H0, H, s, h);
  acc_bias<2>(acc, pkw + pk::SF_B2, h);
  mfma_seg<2, 32>(acc, H, pkw + pk::SF_W2, lane);
  acc_relu<2>(H, acc);
  save_rows<32>(svb, sv::SF_H2, H, s, h);
  acc_bias<2>(acc, pkw + pk::SF_B4, h);
  mfma_seg<2, 32>(acc, H, pkw + pk::SF_W4, lane);
  acc_relu<2>(H, acc);
  save_rows<32>(svb, sv::SF_H4, H, s, h);
#pragma unroll
  for (int o = 0; o < 6; ++o) sf[o] = dot_small<32>(H, pkw + pk::SF_W6 + o * 64, h) + b6[o];
}
