// rdrf_bwd.hip -- backward of the two fields and of the scene-flow MLP for gfx950: the backward-DATA kernels and every
// backward entry point (ray path, feature mode, scene flow), the backward pack jobs and the workspace carving.  The entry points
// choose between the two-kernel forms here and the kernels that form the weight gradients themselves (rdrf_bwd_fused.hip).
//
// Structure per phase (appearance / density / scene flow):
//   1. the training-mode forward saved the per-tile activations as [tile][row][32 samples]
//      (rdrf_kernels.hpp, namespace sv);
//   2. a backward-DATA kernel (k_*_bwd, here) walks the same tiles with the TRANSPOSED weight packs
//      resident in LDS: d_in = W^T dz runs on the fp32 MFMA in the same canonical register layout
//      as the forward (dz of one layer is the B operand of the next), applies the relu masks from
//      the saved rows, back-propagates the positional encodings and writes every dz, and the
//      d(feature) of the VM gathers, as rows (or sample-major records for the sorted scatter);
//   3. the scatter kernels (rdrf_scatter.hip) run the VM gather backward from those rows: atomic scatter
//      into the channel-last planes / lines + coordinate gradients (per-quad device functions: rdrf_bwd_dev.hpp);
//   4. k_dw3 (rdrf_dw.hip) forms dW = sum_samples dz (x) in on the MFMA from the dz rows and the saved rows.
// The entry points call 3, 4 and the fused kernels through the host interface of rdrf_bwd_host.hpp.  The ray-generation backward is in
// rdrf_misc.hip beside its forward, the deterministic build's bind / finish in rdrf_det.hip.
// The kernels here are the launch geometry, the tile queues, the loops, the LDS and the sums; the per-sample and per-tile steps --
// the ray scan backward at both widths, the heads' and the warp MLP's tile, the shared steps of the two appearance kernels, the
// positional-encoding backwards -- are the device functions of rdrf_bwd_mlp_dev.hpp, one copy each, which the fused kernels of
// rdrf_bwd_fused.hip call too.  Three steps are written out in place because hipcc punishes the function (comments at the sites): the
// appearance output layer (spills), the load of the heads' K1G_DX0 rows in front of the warp's layer 3 (MFMA hazard distance) and
// the 64-wide ray scan of k_static_density_bwd (time).
// References: autograd of /root/reference/models/tensorBase.py:704-850, models/tensoRF.py:118-196,
// 446-462, 521-811 (grid_sample backward per SURVEY.md Appendix A).
#include "rdrf_bwd_mlp_dev.hpp"
#include "rdrf_bwd_host.hpp"

RDRF_DET_UNIT(bwd)

// ------------------------------------------------------------------------------------------------
// appearance phase backward-data (dynamic: MLP_Fea_late_view; static: MLP_Fea | TimeEmbedding)
// ------------------------------------------------------------------------------------------------
// REC: d(app features) go out as sample-major records for the sorted scatter (a.dfa) instead of DA rows
template <bool FEAT, bool REC = false>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_dyn_app_bwd(BwdArgs a, DynW w, DynG gw) {
  __shared__ int s_next;
  if (threadIdx.x == 0) s_next = blockDim.x >> 6;   // (before the barrier of lds_fill)
  __shared__ __attribute__((aligned(16))) float lds[pkb::K3_SIZE];
  lds_fill(lds, a.pk + pkb::REG_K3, pkb::K3_SIZE);
  const float* basisT = lds + pkb::K3_BASIST;
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int count = FEAT ? a.M : a.sp.hdr->count;
  const int ntiles = (count + 31) >> 5;
  for (int k = wave, tile; (tile = blockIdx.x + k * gridDim.x) < ntiles; k = tile_queue_next(&s_next, k, nwaves, a.dynq != 0)) {
    const AppTile t = app_tile<FEAT>(a, tile, s, count);
    const float* svb = a.sp.act3 + (size_t)tile * sv::K3_ROWS * 32;
    float* gb = a.grows3 + (size_t)tile * sv::K3G_ROWS * 32;
    if constexpr (FEAT) {
      app_feat_only<7>(a, gb, t, basisT, pkb::REG_K3_LO, pkb::K3_LO_BASIST, s, h, lane);
      continue;
    }
    float vx, vy, vz;
    ray_norm(a.rays, t.n, a.ray_type, vx, vy, vz);
    // ---- output layer: v = Wv [H2, vd] + b ; rgb = sigmoid(v).  Written out here and in k_static_app_bwd: as a function
    // shared by the two (whole, or the dzv loop alone, H2 loaded inside or passed in) hipcc spills 39 to 56 registers in all
    // four ray-path instantiations of the appearance kernels, which hold 223 to 236 without it
    float H2[64];
    load_rows<64>(svb, sv::K3_H2, H2, s, h);
    float dzv[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float v = dot_small<64>(H2, lds + pkb::K3_RGBV + o * 128, h) + w.rbv[o];
      v += w.rwv[o * 131 + 128] * vx + w.rwv[o * 131 + 129] * vy + w.rwv[o * 131 + 130] * vz;
      const float r = sigmoidf_(v);
      const float g = (t.act && a.g_rgb) ? a.g_rgb[(size_t)t.idx * 3 + o] : 0.f;
      dzv[o] = g * r * (1.0f - r);
      if (h == 0) gb[(size_t)(sv::K3G_DZV + o) * 32 + s] = dzv[o];
    }
    float dz2[64];
    small_layer_bwd<64, 3>(dz2, H2, lds + pkb::K3_RGBV, h, dzv);
    save_rows<64>(gb, sv::K3G_DZ2, dz2, s, h);
    float dz1[64];
    app_l2_bwd(dz1, dz2, a, svb, gb, sv::K3_H1, lds + pkb::K3_RGB2T, pkb::REG_K3_LO, pkb::K3_LO_RGB2T, s, h, lane);
    // ---- layer 1 backward: feature block and X0 block (t / PE(t) carry no gradient)
    float dF[16], dX0[32];
    {
#ifdef RDRF_APP_F32
      f32x16 acc[1];
      acc_zero<1>(acc);
      mfma_seg<1, 64>(acc, dz1, lds + pkb::K3_RGB1T_F, lane);
      acc_copy<1>(dF, acc);
      f32x16 acc2[2];
      acc_zero<2>(acc2);
      mfma_seg<2, 64>(acc2, dz1, lds + pkb::K3_RGB1T_X0, lane);
      acc_copy<2>(dX0, acc2);
#else   // the F block and the two X0 blocks are one three-block image: one split of dz1
      f32x16 acc[3];
      acc_zero<3>(acc);
      app_bwd_seg<3, 64>(acc, dz1, lds + pkb::K3_RGB1T_F, a.pk, pkb::REG_K3_LO, pkb::K3_LO_RGB1T, lane);
#pragma unroll
      for (int i = 0; i < 16; ++i) dF[i] = acc[0][i];
#pragma unroll
      for (int i = 0; i < 32; ++i) dX0[i] = acc[1 + (i >> 4)][i & 15];
#endif
    }
    save_rows<16>(gb, sv::K3G_DF, dF, s, h);
    float dn0 = 0.f, dn1 = 0.f, dn2 = 0.f;
    {
      float X0[32];
      load_rows<32>(svb, sv::K3_X0, X0, s, h);
      x0_bwd(X0, dX0, h, dn0, dn1, dn2);
    }
    dn0 += __shfl_xor(dn0, 32, 64); dn1 += __shfl_xor(dn1, 32, 64); dn2 += __shfl_xor(dn2, 32, 64);
    // ---- basis backward: d(app features) rows for the scatter kernel
    {
      float dA[112];
      app_basis_bwd<7>(dA, dF, basisT, a.pk, pkb::REG_K3_LO, pkb::K3_LO_BASIST, lane);
      if constexpr (REC) {
        // sample-major record for the sorted scatter: this lane half holds the feature quads Q = 2 m + h (slots
        // 4m..4m+3) of compacted sample li; one 16-byte store per quad, the two halves write adjacent quads
        if (t.act) {
          // quad 2 m + 1 sits 4 floats after quad 2 m in the record, except for the (XZ quad 2 | YZ quad 0) pair of
          // every level: one base pointer per half + immediate offsets
          float* rec = a.dfa + (size_t)t.li * DFA_FLOATS + 4 * h;
          float* recx = a.dfa + (size_t)t.li * DFA_FLOATS + (h ? dfa_off(15) - dfa_off(14) : 0);
#pragma unroll
          for (int m = 0; m < 27; ++m) {
            static_assert(dfa_off(1) == dfa_off(0) + 4 && dfa_off(13) == dfa_off(12) + 4 && dfa_off(17) == dfa_off(16) + 4, "record layout");
            float* dst = (m % 9 == 7 ? recx : rec) + dfa_off(2 * m);
            *reinterpret_cast<f32x4*>(dst) = f32x4{dA[4 * m], dA[4 * m + 1], dA[4 * m + 2], dA[4 * m + 3]};
          }
        }
      } else {
        save_rows<112>(gb, sv::K3G_DA, dA, s, h);
      }
    }
    if (t.act && h == 0) {
      a.dxn_app[(size_t)t.idx * 3 + 0] = dn0; a.dxn_app[(size_t)t.idx * 3 + 1] = dn1;
      a.dxn_app[(size_t)t.idx * 3 + 2] = dn2;
    }
  }
}

template <int HEAD, bool FEAT>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_static_app_bwd(BwdArgs a, StaticW w, StaticG gw) {
  __shared__ int s_next;
  if (threadIdx.x == 0) s_next = blockDim.x >> 6;   // (before the barrier of lds_fill)
  __shared__ __attribute__((aligned(16))) float lds[pkb::S3_SIZE];
  lds_fill(lds, a.pk + pkb::REG_S3, pkb::S3_SIZE);
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int count = FEAT ? a.M : a.sp.hdr->count;
  const int ntiles = (count + 31) >> 5;
  for (int k = wave, tile; (tile = blockIdx.x + k * gridDim.x) < ntiles; k = tile_queue_next(&s_next, k, nwaves, a.dynq != 0)) {
    const AppTile t = app_tile<FEAT>(a, tile, s, count);
    const float* svb = a.sp.act3 + (size_t)tile * sv::S3_ROWS * 32;
    float* gb = a.grows3 + (size_t)tile * sv::K3G_ROWS * 32;
    if constexpr (FEAT) {
      app_feat_only<3>(a, gb, t, lds + pkb::S3_BASIST, pkb::REG_S3_LO, pkb::S3_LO_BASIST, s, h, lane);
      continue;
    }
    float vx, vy, vz;
    ray_norm(a.rays, t.n, a.ray_type, vx, vy, vz);
    // ---- output layer (in place: see k_dyn_app_bwd)
    float H2[64];
    load_rows<64>(svb, sv::S3_H2, H2, s, h);
    float dzv[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float v = dot_small<64>(H2, lds + pkb::S3_W3 + o * 128, h) + w.b3[o];
      if (HEAD == RDRF_HEAD_MLP_FEA_TIMEEMBEDDING)
        v += w.w3[o * 131 + 128] * vx + w.w3[o * 131 + 129] * vy + w.w3[o * 131 + 130] * vz;
      const float r = sigmoidf_(v);
      const float g = (t.act && a.g_rgb) ? a.g_rgb[(size_t)t.idx * 3 + o] : 0.f;
      dzv[o] = g * r * (1.0f - r);
      if (h == 0) gb[(size_t)(sv::K3G_DZV + o) * 32 + s] = dzv[o];
    }
    float dz2[64];
    small_layer_bwd<64, 3>(dz2, H2, lds + pkb::S3_W3, h, dzv);
    save_rows<64>(gb, sv::K3G_DZ2, dz2, s, h);
    float dz1[64];
    app_l2_bwd(dz1, dz2, a, svb, gb, sv::S3_H1, lds + pkb::S3_W2T, pkb::REG_S3_LO, pkb::S3_LO_W2T, s, h, lane);
    float dF[16];
    {
#ifdef RDRF_APP_F32
      f32x16 acc[1];
      acc_zero<1>(acc);
      mfma_seg<1, 64>(acc, dz1, lds + pkb::S3_W1T_F, lane);
      acc_copy<1>(dF, acc);
      f32x16 accp[4];
      acc_zero<4>(accp);
      mfma_seg<4, 64>(accp, dz1, lds + pkb::S3_W1T_P, lane);
#else   // the F block and the four PE blocks are one five-block image: one split of dz1
      f32x16 acc5[5];
      acc_zero<5>(acc5);
      app_bwd_seg<5, 64>(acc5, dz1, lds + pkb::S3_W1T_F, a.pk, pkb::REG_S3_LO, pkb::S3_LO_W1T, lane);
#pragma unroll
      for (int i = 0; i < 16; ++i) dF[i] = acc5[0][i];
      f32x16 (&accp)[4] = *reinterpret_cast<f32x16 (*)[4]>(&acc5[1]);
#endif
      float P[64];
      load_rows<64>(svb, sv::S3_P, P, s, h);
      // PE2 backward: P[4r..4r+3] = (sin f, cos f, sin 2f, cos 2f) of feature slot r
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d0 = accp[r >> 2][(r & 3) * 4 + 0], d1 = accp[r >> 2][(r & 3) * 4 + 1];
        const float d2 = accp[r >> 2][(r & 3) * 4 + 2], d3 = accp[r >> 2][(r & 3) * 4 + 3];
        dF[r] += d0 * P[4 * r + 1] - d1 * P[4 * r + 0] + 2.0f * (d2 * P[4 * r + 3] - d3 * P[4 * r + 2]);
      }
    }
    // the view-direction slots (27..29) of the feature block are not features: they carry
    // d(loss)/d(viewdir); viewdir = d/|d|  =>  g_d = (g_v - (g_v.v) v) / |d|
    {
      const int n = t.n;
      const bool act = t.act;
      float gv0 = 0.f, gv1 = 0.f, gv2 = 0.f;
      if (HEAD == RDRF_HEAD_MLP_FEA) {
        if (h == 0) { gv0 = dF[15]; dF[15] = 0.f; }
        else { gv1 = dF[12]; gv2 = dF[13]; dF[12] = 0.f; dF[13] = 0.f; }
        gv0 += __shfl_xor(gv0, 32, 64); gv1 += __shfl_xor(gv1, 32, 64); gv2 += __shfl_xor(gv2, 32, 64);
      } else {
#pragma unroll
        for (int o = 0; o < 3; ++o) {
          gv0 += w.w3[o * 131 + 128] * dzv[o]; gv1 += w.w3[o * 131 + 129] * dzv[o];
          gv2 += w.w3[o * 131 + 130] * dzv[o];
        }
      }
      if (a.g_rays && act && h == 0 && a.ray_type != RDRF_RAY_OTHER) {
        const float rx = a.rays[(size_t)n * 6 + 3], ry = a.rays[(size_t)n * 6 + 4], rz = a.rays[(size_t)n * 6 + 5];
        const float nr = sqrtf(rx * rx + ry * ry + rz * rz);
        const float dotv = gv0 * vx + gv1 * vy + gv2 * vz;
        atomicAdd(a.g_rays + (size_t)n * 6 + 3, (gv0 - dotv * vx) / nr);
        atomicAdd(a.g_rays + (size_t)n * 6 + 4, (gv1 - dotv * vy) / nr);
        atomicAdd(a.g_rays + (size_t)n * 6 + 5, (gv2 - dotv * vz) / nr);
      } else if (a.g_rays && act && h == 0) {
        atomicAdd(a.g_rays + (size_t)n * 6 + 3, gv0);
        atomicAdd(a.g_rays + (size_t)n * 6 + 4, gv1);
        atomicAdd(a.g_rays + (size_t)n * 6 + 5, gv2);
      }
    }
    save_rows<16>(gb, sv::K3G_DF, dF, s, h);
    float dG[48];
    app_basis_bwd<3>(dG, dF, lds + pkb::S3_BASIST, a.pk, pkb::REG_S3_LO, pkb::S3_LO_BASIST, lane);
    save_rows<48>(gb, sv::K3G_DA, dG, s, h);
  }
}

// static field, density phase backward: wave per ray, lane per sample.  This is the ray scan backward of rdrf_bwd_mlp_dev.hpp
// (scan_sample, tile_carries, suffix_g_alpha, dist_grads) 64 wide, written out in place: built from those functions the kernel
// gave the same bits with the same 37 registers, and took 0.0185 ms against 0.0176 ms at the bench's final stage (ten
// alternating runs each: new 0.0183 .. 0.0188, parent 0.0174 .. 0.0178), 0.0109 against 0.0107 ms at stage 0.
__global__ __launch_bounds__(64) void k_static_density_bwd(BwdArgs a, StaticW w, float* __restrict__ gf_rows) {
  __shared__ float carr[64];   // transmittance carries at each 64-sample step (S <= 4096)
  const int lane = threadIdx.x;
  const int n = blockIdx.x;
  if (n >= a.N) return;
  float vx, vy, vz;
  const float nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
  if (a.g_weight) {
    float carry = 1.0f;
    for (int j0 = 0; j0 < a.S; j0 += 64) {
      if (lane == 0) carr[j0 >> 6] = carry;
      const int j = j0 + lane;
      const bool act = j < a.S;
      const int idx = n * a.S + (act ? j : 0);
      const bool vld = act && a.valid[idx] != 0;
      const float sigma = vld ? density_act(a.sp.raw[idx], a.act, a.density_shift) : 0.f;
      const float zj = act ? a.z[idx] : 0.f;
      const float zn = (j + 1 < a.S) ? a.z[idx + 1] : zj;
      const float ds = ((j + 1 < a.S) ? (zn - zj) : 0.0f) * nrm * a.distance_scale;
      const float alpha = 1.0f - expf(-sigma * ds);
      const float p = act ? one_minus_alpha_eps(alpha) : 1.0f;
      carry *= __shfl(scan_mul64(p, lane), 63, 64);
    }
  }
  __syncthreads();
  float sufcarry = 0.f, g_nrm = 0.f;
  const int ntile = (a.S + 63) >> 6;
  for (int tl = ntile - 1; tl >= 0; --tl) {
    const int j0 = tl << 6;
    const int j = j0 + lane;
    const bool act = j < a.S;
    const int idx = n * a.S + (act ? j : 0);
    const bool vld = act && a.valid[idx] != 0;
    const float f = a.sp.raw[idx];
    const float sigma = vld ? density_act(f, a.act, a.density_shift) : 0.f;
    const float zj = act ? a.z[idx] : 0.f;
    const float zn = (j + 1 < a.S) ? a.z[idx + 1] : zj;
    const float ds = ((j + 1 < a.S) ? (zn - zj) : 0.0f) * nrm * a.distance_scale;
    const float alpha = 1.0f - expf(-sigma * ds);
    const float p = act ? one_minus_alpha_eps(alpha) : 1.0f;
    float g_alpha = 0.f;
    if (a.g_weight) {
      const float incl = scan_mul64(p, lane);
      float excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = 1.0f;
      const float T = carr[tl] * excl;
      const float gwv = act ? a.g_weight[idx] : 0.f;
      float rinc = gwv * alpha * T;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_down(rinc, d, 64);
        if (lane + d < 64) rinc += o;
      }
      float rex = __shfl_down(rinc, 1, 64);
      if (lane == 63) rex = 0.f;
      g_alpha = gwv * T - (sufcarry + rex) / p;
      sufcarry += __shfl(rinc, 0, 64);
    }
    float g_sigma = (act && a.g_sigma) ? a.g_sigma[idx] : 0.f;
    g_sigma += g_alpha * ds * (1.0f - alpha);
    if ((a.g_rays || a.g_z) && act) {  // dists = dz * |d| * scale: d(loss)/d|d| and d(loss)/dz
      const float g_ds = (a.g_dists ? a.g_dists[idx] : 0.f) + g_alpha * sigma * (1.0f - alpha);
      if (a.g_rays) g_nrm += g_ds * ((j + 1 < a.S) ? (zn - zj) : 0.0f) * a.distance_scale;
      if (a.g_z && j + 1 < a.S) {
        const float gz = g_ds * nrm * a.distance_scale;
        atomicAdd(a.g_z + idx, -gz);
        atomicAdd(a.g_z + idx + 1, gz);
      }
    }
    const float gf = vld ? g_sigma * act_grad(f, a.act, a.density_shift) : 0.f;
    // d(loss)/d(density feature) per sample; the VM gather backward (scatter + coordinate gradients)
    // runs in k_scatter with LDS line accumulators (bcast mode: the feature is the plain sum of the
    // 24 products, so every component has this same gradient)
    if (act) gf_rows[(size_t)n * (((a.S + 31) >> 5) << 5) + j] = gf;
  }
  if (a.g_rays && a.ray_type != RDRF_RAY_OTHER) {
    g_nrm = wave_sum(g_nrm);
    if (lane < 3) atomicAdd(a.g_rays + (size_t)n * 6 + 3 + lane, g_nrm * (lane == 0 ? vx : (lane == 1 ? vy : vz)));
  }
}

// ------------------------------------------------------------------------------------------------
// dynamic field, density / blending / warp backward-data: wave per ray, 32-sample tiles, in two
// phases around the scatter kernel:
//   PHASE 0 (heads): weight/sigma/blending backward, density + blending head backward ->
//                    d(feature) rows for k_scatter, d(X0) partial rows, dz rows        (dyn_heads_bwd_tile)
//   PHASE 1 (warp) : coordinate gradients (appearance + density + blending scatter) ->
//                    warp MLP backward, positional-encoding backward, g_xyz, d(tout)  (dyn_warp_bwd_tile)
// ------------------------------------------------------------------------------------------------

// The scan half of the heads' backward on the flat-tile path (rdrf_flat_density): per ray, the transmittance carries at
// the tile starts (pre-pass) and the reverse suffix sweep of d(weight) -> d(alpha); per sample the total
// g_sigma = the caller's g_sigma + g_alpha ds (1 - alpha) (BwdArgs::gsig), the g_z updates, and the ray norm's share of
// g_rays.  A half-wave per ray (two rays per wave, as ray_scan_body).  It runs the functions the wave-per-ray
// k_dyn_density_bwd<0> runs, at the same width, so g_sigma comes out bit-identical.
__global__ __launch_bounds__(512) void k_ray_scan_bwd(BwdArgs a) {
  __shared__ float carr[16][128];   // per half-wave: transmittance at the tile starts (S <= 4096)
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int hw = (threadIdx.x >> 6) * 2 + h;
  const int n_ = blockIdx.x * 16 + hw;
  const bool ray = n_ < a.N;
  const int n = ray ? n_ : 0;
  const int tpr = (a.S + 31) >> 5;
  float vx, vy, vz;
  const float nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
  if (a.g_weight) tile_carries<32>(a, carr[hw], 2, n, ray, s == 0, s, nrm);
  float sufcarry = 0.f, g_nrm = 0.f;
  for (int tli = tpr - 1; tli >= 0; --tli) {  // LAST tile first: direct suffix sums
    const int j = (tli << 5) + s;
    const bool act = ray && j < a.S;
    const int idx = n * a.S + (act ? j : 0);
    const bool vld = act && a.valid[idx] != 0;
    const float g_sigma = scan_bwd_step<32>(a, a.sp.raw[(size_t)idx * 2], carr[hw] + tli, act, vld, act, idx, j, s, nrm, sufcarry, g_nrm);
    if (act) a.gsig[idx] = g_sigma;
  }
  if (a.g_rays && a.ray_type != RDRF_RAY_OTHER) {   // the half-wave owns its ray: one update per component
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) g_nrm += __shfl_xor(g_nrm, d, 64);
    if (ray && s < 3) atomicAdd(a.g_rays + (size_t)n * 6 + 3 + s, g_nrm * (s == 0 ? vx : (s == 1 ? vy : vz)));
  }
}

// FLAT (training, rdrf_flat_density): the unit of work is a 32-sample tile of the flat [N * S] array, the saved rows and the
// gradient rows are those of tile `n`; phase 0 reads the total d(sigma) per sample from k_ray_scan_bwd, phase 1 reduces
// d(tout) per ray over the tile's lanes (segmented by the lane's ray) and writes it directly for a ray that lies inside
// the tile, or as one of the tile's two partial records (first / last ray) that k_time_branch_bwd sums in a fixed order.
template <int PHASE, bool FEAT, bool FLAT = false>
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_dyn_density_bwd(BwdArgs a, DynW w, DynG gw) {
  static_assert(!(FLAT && FEAT), "feature mode keeps its pseudo-ray geometry (S = 32: a ray is a tile)");
  __shared__ __attribute__((aligned(16))) float lds[PHASE == 0 ? pkb::K1H_SIZE : pkb::K1W_SIZE];
  __shared__ float carr[8][128];  // per-wave transmittance carries at tile starts (S <= 4096)
  lds_fill(lds, a.pk + (PHASE == 0 ? pkb::REG_K1H : pkb::REG_K1W), PHASE == 0 ? pkb::K1H_SIZE : pkb::K1W_SIZE);
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int tpr = (a.S + 31) >> 5;
  // small-layer weight gradients of this wave (ray path): lane (s, h) holds input element elem_of(s, h) of up to three
  // output rows (PHASE 0: density / blending layer2; PHASE 1: the three rows of layer5) + the rows' bias sums per lane
  float sw[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f};
  const int nunits = FLAT ? (a.N * a.S + 31) >> 5 : a.N;
  for (int n = blockIdx.x * nwaves + wave; n < nunits; n += gridDim.x * nwaves) {
    float vx = 0.f, vy = 0.f, vz = 0.f;
    float nrm = 1.0f;
    if constexpr (!FEAT && !FLAT) nrm = ray_norm(a.rays, n, a.ray_type, vx, vy, vz);
    if (!FEAT && !FLAT && PHASE == 0 && a.g_weight) tile_carries<32>(a, carr[wave], 2, n, true, lane == 0, s, nrm);
    float sufcarry = 0.f, g_nrm = 0.f;
    float dTacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) dTacc[i] = 0.f;
    for (int tli = FLAT ? 0 : tpr - 1; tli >= 0; --tli) {  // LAST tile first: direct suffix sums
      const int j0 = tli << 5;
      const int j = j0 + s;
      const bool act = FLAT ? n * 32 + s < a.N * a.S : j < a.S && (!FEAT || n * a.S + j < a.M);
      const int idx = FLAT ? (act ? n * 32 + s : 0) : n * a.S + (act ? j : 0);
      const bool vld = act && (FEAT || a.valid[idx] != 0);
      const size_t tl = FLAT ? (size_t)n : (size_t)n * tpr + tli;
      const float* svb = a.sp.act1 + tl * sv::K1_ROWS * 32;
      float* gb = a.grows1 + tl * sv::K1G_ROWS * 32;
      if constexpr (PHASE == 0) dyn_heads_bwd_tile<FEAT, FLAT>(a, lds, svb, gb, act, vld, idx, j, s, h, lane, nrm, carr[wave] + tli, sufcarry, g_nrm, sw, sb);
      else dyn_warp_bwd_tile<FEAT>(a, lds, svb, gb, act, idx, s, h, lane, dTacc, sw, sb);
    }
    if (PHASE == 1 && !FEAT && FLAT) {
      const DtoutSeg g = dtout_segments(a, n, s);
      float* dst = g.inside ? a.dtout + (size_t)g.nl * 32 : a.dtp + ((size_t)n * 2 + (s == 0 ? 0 : 1)) * 32;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = dTacc[i];
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) {
          const float o = __shfl_down(v, d, 32);
          if (s + d <= g.end) v += o;
        }
        if (g.head) dst[elem_of(i, h)] = v;
      }
    }
    if (PHASE == 1 && !FEAT && !FLAT) {  // per-ray d(tout): sum over the samples (lanes of each half)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = dTacc[i];
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if (s == 0) a.dtout[(size_t)n * 32 + elem_of(i, h)] = v;
      }
    }
    if (!FEAT && !FLAT && PHASE == 0 && a.g_rays && a.ray_type != RDRF_RAY_OTHER) {
      g_nrm = wave_sum(g_nrm);
      if (lane < 3) atomicAdd(a.g_rays + (size_t)n * 6 + 3 + lane, g_nrm * (lane == 0 ? vx : (lane == 1 ? vy : vz)));
    }
  }
  if (!FEAT && a.small_dw) {
    // small-layer gradients: sum the workgroup's waves in LDS, then one atomic per entry and workgroup
    __shared__ float red[8][3][65];
    __syncthreads();   // (also: every wave is done with `carr`)
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      red[wave][o][lane] = sw[o];
      const float bs = wave_sum(h == 0 ? sb[o] : 0.f);   // both halves hold the same samples
      if (lane == 0) red[wave][o][64] = bs;
    }
    __syncthreads();
    if (wave == 0) {
      const bool live_d = a.g_sigma != nullptr || a.g_weight != nullptr, live_b = a.g_blending != nullptr;
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        float v = 0.f, bv = 0.f;
        for (int wv = 0; wv < nwaves; ++wv) { v += red[wv][o][lane]; bv += red[wv][o][64]; }
        float* gwt = PHASE == 1 ? gw.l5w + o * 64 : (o == 0 ? gw.dw2 : gw.bw2);
        float* gbs = PHASE == 1 ? gw.l5b + o : (o == 0 ? gw.db2 : gw.bb2);
        const bool on = PHASE == 1 ? true : (o == 0 ? live_d : (o == 1 ? live_b : false));
        if (on) {
          grad_add(gwt + elem_of(s, h), v);
          if (lane == 0) grad_add(gbs, bv);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// time branch backward: [t, PE8(t)] -> 64 -> relu -> 30.  32 rays per 128-thread block, 4 lanes per
// ray (16 hidden neurons each); parameter gradients are reduced inside the block through LDS, then
// one atomic per entry.  (128 rays per block / thread per ray used 32 CUs: 56 us per launch.)
// ------------------------------------------------------------------------------------------------
#define TB_RPB 32
// d(tout) of ray n, element o.  dtp == nullptr: dtout holds it.  Flat-tile path (k_dyn_density_bwd<1, false, true>): a ray
// inside one tile was written to dtout; a ray that crosses tile edges is the sum of its tiles' partial records, in tile
// order: [t0][last ray] (or [t0][first ray] if the ray starts the tile), then [t][first ray] for the following tiles.
RDRF_D float dtout_of_ray(const float* __restrict__ dtout, const float* __restrict__ dtp, int S, int n, int o) {
  const int b = n * S, t0 = b >> 5, t1 = (b + S - 1) >> 5;
  if (dtp == nullptr || t0 == t1) return dtout[(size_t)n * 32 + o];
  float v = dtp[((size_t)t0 * 2 + ((b & 31) == 0 ? 0 : 1)) * 32 + o];
  for (int t = t0 + 1; t <= t1; ++t) v += dtp[(size_t)t * 64 + o];
  return v;
}

__global__ __launch_bounds__(128) void k_time_branch_bwd(const float* __restrict__ ts, DynW w, int N,
                                                         const float* __restrict__ dtout,
                                                         const float* __restrict__ dtp, int S,
                                                         float* __restrict__ g_l1w,
                                                         float* __restrict__ g_l1b,
                                                         float* __restrict__ g_l2w,
                                                         float* __restrict__ g_l2b) {
  __shared__ float s_tin[TB_RPB][17];
  __shared__ float s_h[TB_RPB][65];
  __shared__ float s_dz1[TB_RPB][65];
  __shared__ float s_dz2[TB_RPB][31];
  const int tid = threadIdx.x;
  const int r = tid >> 2, q = tid & 3;
  const int n = blockIdx.x * TB_RPB + r;
  const bool act = n < N;
  float tin[17];
  const float t = act ? ts[n] : 0.f;
  tin[0] = t;
#pragma unroll
  for (int f = 0; f < 8; ++f) sincosf(ldexpf(t, f), &tin[1 + f], &tin[9 + f]);
  if (q == 0)
    for (int i = 0; i < 17; ++i) s_tin[r][i] = tin[i];
  for (int o = q; o < 30; o += 4) s_dz2[r][o] = act ? dtout_of_ray(dtout, dtp, S, n, o) : 0.f;
  __syncthreads();
  for (int k = 16 * q; k < 16 * q + 16; ++k) {
    float hk = w.l1b[k];
#pragma unroll
    for (int i = 0; i < 17; ++i) hk = fmaf(w.l1w[k * 17 + i], tin[i], hk);
    float dh = 0.f;
    for (int o = 0; o < 30; ++o) dh = fmaf(w.l2w[o * 64 + k], s_dz2[r][o], dh);
    s_h[r][k] = fmaxf(hk, 0.f);
    s_dz1[r][k] = hk > 0.f ? dh : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < 30 * 64; e += 128) {
    const int o = e / 64, k = e - o * 64;
    float a = 0.f;
    for (int rr = 0; rr < TB_RPB; ++rr) a = fmaf(s_dz2[rr][o], s_h[rr][k], a);
    grad_add(g_l2w + e, a);
  }
  for (int e = tid; e < 64 * 17; e += 128) {
    const int k = e / 17, i = e - k * 17;
    float a = 0.f;
    for (int rr = 0; rr < TB_RPB; ++rr) a = fmaf(s_dz1[rr][k], s_tin[rr][i], a);
    grad_add(g_l1w + e, a);
  }
  if (tid < 30) {
    float a = 0.f;
    for (int rr = 0; rr < TB_RPB; ++rr) a += s_dz2[rr][tid];
    grad_add(g_l2b + tid, a);
  }
  if (tid < 64) {
    float a = 0.f;
    for (int rr = 0; rr < TB_RPB; ++rr) a += s_dz1[rr][tid];
    grad_add(g_l1b + tid, a);
  }
}

// ------------------------------------------------------------------------------------------------
// scene flow backward-data
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_scene_flow_bwd(int N, int S, Box box,
                                                        const float* __restrict__ pkg,
                                                        const float* __restrict__ act_rows,
                                                        float* __restrict__ grows,
                                                        const float* __restrict__ g_f,
                                                        const float* __restrict__ g_b,
                                                        float* __restrict__ g_sfb6,
                                                        float* __restrict__ g_pts) {
  __shared__ __attribute__((aligned(16))) float lds[pkb::SF_SIZE];
  lds_fill(lds, pkg + pkb::REG_SF, pkb::SF_SIZE);
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int total = N * S;
  const int ntiles = (total + 31) >> 5;
  for (int tile = blockIdx.x * nwaves + wave; tile < ntiles; tile += gridDim.x * nwaves) {
    const int li = tile * 32 + s;
    const bool act = li < total;
    const int idx = act ? li : 0;
    const float* svb = act_rows + (size_t)tile * sv::SF_ROWS * 32;
    float* gb = grows + (size_t)tile * sv::SFG_ROWS * 32;
    float dz6[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) {
      const float* gsrc = o < 3 ? g_f : g_b;
      dz6[o] = (act && gsrc) ? gsrc[(size_t)idx * 3 + (o % 3)] : 0.f;
      if (h == 0) gb[(size_t)(sv::SFG_DZ6 + o) * 32 + s] = dz6[o];
    }
    float dz[32], Hh[32];
    load_rows<32>(svb, sv::SF_H4, Hh, s, h);
    small_layer_bwd<32, 6>(dz, Hh, lds + pkb::SF_W6, h, dz6);
    save_rows<32>(gb, sv::SFG_DZ4, dz, s, h);
    f32x16 acc[2];
    acc_zero<2>(acc);
    mfma_seg<2, 32>(acc, dz, lds + pkb::SF_W4T, lane);
    load_rows<32>(svb, sv::SF_H2, Hh, s, h);
    relu_gate<32>(dz, Hh, acc);
    save_rows<32>(gb, sv::SFG_DZ2, dz, s, h);
    acc_zero<2>(acc);
    mfma_seg<2, 32>(acc, dz, lds + pkb::SF_W2T, lane);
    load_rows<32>(svb, sv::SF_H0, Hh, s, h);
    relu_gate<32>(dz, Hh, acc);
    save_rows<32>(gb, sv::SFG_DZ0, dz, s, h);
    if (g_pts) {
      acc_zero<2>(acc);
      mfma_seg<2, 32>(acc, dz, lds + pkb::SF_W0T, lane);
      float X[20], dX[20];
      load_rows<20>(svb, sv::SF_X, X, s, h);
#pragma unroll
      for (int kk = 0; kk < 20; ++kk) dX[kk] = acc[kk >> 4][kk & 15];
      float d0 = 0.f, d1 = 0.f, d2 = 0.f;
      sf_x_bwd(X, dX, h, d0, d1, d2);
      d0 += __shfl_xor(d0, 32, 64); d1 += __shfl_xor(d1, 32, 64); d2 += __shfl_xor(d2, 32, 64);
      if (act && h == 0) {
        g_pts[(size_t)idx * 3 + 0] += d0 * box.inv[0];
        g_pts[(size_t)idx * 3 + 1] += d1 * box.inv[1];
        g_pts[(size_t)idx * 3 + 2] += d2 * box.inv[2];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
void dyn_pack_jobs_bwd(PackJobs& J, const RdrfDynamicParams* P) {
  using namespace pkb;
  J.n = 0;
  const int kh = REG_K1H, kw = REG_K1W, k3 = REG_K3, sf = REG_SF;
  pack_add(J, P->l5w, 64, 3, 64, SEG_IDENT, 1, 3, 32, kw + K1W_W5);
#ifdef RDRF_HEADS_BWD_F32
  const int wm = 2, hm = 2;
#else
  const int wm = 8, hm = 8;   // bf16 x 3 transposed fragments
#endif
  pack_add(J, P->l4w, 64, 64, 64, SEG_IDENT, wm, 2, 32, kw + K1W_W4T);
  pack_add(J, P->l3w, 93, 64, 93, SEG_WARP3_X0, wm, 2, 32, kw + K1W_W3T_X0);
  pack_add(J, P->l3w, 93, 64, 93, SEG_WARP3_T, wm, 1, 32, kw + K1W_W3T_T);
  pack_add(J, P->dw2, 64, 1, 64, SEG_IDENT, 1, 1, 32, kh + K1H_DEN2);
  pack_add(J, P->bw2, 64, 1, 64, SEG_IDENT, 1, 1, 32, kh + K1H_BLE2);
  pack_add(J, P->dw1, 152, 64, 72, SEG_IDENT, hm, 3, 32, kh + K1H_DEN1T_F);
  pack_add(J, P->dw1, 152, 64, 152, SEG_DEN1_X0, hm, 2, 32, kh + K1H_DEN1T_X0);
  pack_add(J, P->bw1, 152, 64, 72, SEG_IDENT, hm, 3, 32, kh + K1H_BLE1T_F);
  pack_add(J, P->bw1, 152, 64, 152, SEG_DEN1_X0, hm, 2, 32, kh + K1H_BLE1T_X0);
  pack_add(J, P->rwv, 131, 3, 128, SEG_IDENT, 1, 3, 64, k3 + K3_RGBV);
#ifdef RDRF_APP_F32   // A/B builds: the appearance phases' backward-data products on the fp32 matrix pipe
  pack_add(J, P->rw2, 128, 128, 128, SEG_IDENT, 2, 4, 64, k3 + K3_RGB2T);
  pack_add(J, P->rw1, 107, 128, 107, SEG_RGB1_F, 2, 1, 64, k3 + K3_RGB1T_F);
  pack_add(J, P->rw1, 107, 128, 107, SEG_RGB1_X0, 2, 2, 64, k3 + K3_RGB1T_X0);
  pack_add(J, P->basis, 216, 27, 216, SEG_IDENT, 2, 7, 16, k3 + K3_BASIST);
#else                 // bf16 x 3 with split storage (same image offsets and sizes)
  pack_add_b3s_t(J, P->rw2, 128, 128, 128, SEG_IDENT, 4, 64, k3 + K3_RGB2T, REG_K3_LO + K3_LO_RGB2T);
  pack_add_b3s_t(J, P->rw1, 107, 128, 107, SEG_RGB1_F, 1, 64, k3 + K3_RGB1T_F, REG_K3_LO + K3_LO_RGB1T);
  pack_add_b3s_t(J, P->rw1, 107, 128, 107, SEG_RGB1_X0, 2, 64, k3 + K3_RGB1T_X0, REG_K3_LO + K3_LO_RGB1T + 64 * 32);
  pack_add_b3s_t(J, P->basis, 216, 27, 216, SEG_IDENT, 7, 16, k3 + K3_BASIST, REG_K3_LO + K3_LO_BASIST);
#endif
  pack_add(J, P->sfw[3], 64, 6, 64, SEG_IDENT, 1, 6, 32, sf + SF_W6);
  pack_add(J, P->sfw[2], 64, 64, 64, SEG_IDENT, 2, 2, 32, sf + SF_W4T);
  pack_add(J, P->sfw[1], 64, 64, 64, SEG_IDENT, 2, 2, 32, sf + SF_W2T);
  pack_add(J, P->sfw[0], 36, 64, 36, SEG_SF_X, 2, 2, 32, sf + SF_W0T);
}

void static_pack_jobs_bwd(PackJobs& J, const RdrfStaticParams* P, int head) {
  using namespace pkb;
  J.n = 0;
  const bool fea = head == RDRF_HEAD_MLP_FEA;
  const int in1 = fea ? 138 : 135;
  pack_add(J, P->w3, fea ? 128 : 131, 3, 128, SEG_IDENT, 1, 3, 64, REG_S3 + S3_W3);
#ifdef RDRF_APP_F32
  pack_add(J, P->w2, 128, 128, 128, SEG_IDENT, 2, 4, 64, REG_S3 + S3_W2T);
  pack_add(J, P->w1, in1, 128, in1, fea ? SEG_STAT1_F_FEA : SEG_STAT1_F_TE, 2, 1, 64, REG_S3 + S3_W1T_F);
  pack_add(J, P->w1, in1, 128, in1, fea ? SEG_STAT1_P_FEA : SEG_STAT1_P_TE, 2, 4, 64, REG_S3 + S3_W1T_P);
  pack_add(J, P->basis, 72, 27, 72, SEG_IDENT, 2, 3, 16, REG_S3 + S3_BASIST);
#else
  pack_add_b3s_t(J, P->w2, 128, 128, 128, SEG_IDENT, 4, 64, REG_S3 + S3_W2T, REG_S3_LO + S3_LO_W2T);
  pack_add_b3s_t(J, P->w1, in1, 128, in1, fea ? SEG_STAT1_F_FEA : SEG_STAT1_F_TE, 1, 64, REG_S3 + S3_W1T_F, REG_S3_LO + S3_LO_W1T);
  pack_add_b3s_t(J, P->w1, in1, 128, in1, fea ? SEG_STAT1_P_FEA : SEG_STAT1_P_TE, 4, 64, REG_S3 + S3_W1T_P, REG_S3_LO + S3_LO_W1T + 64 * 32);
  pack_add_b3s_t(J, P->basis, 72, 27, 72, SEG_IDENT, 3, 16, REG_S3 + S3_BASIST, REG_S3_LO + S3_LO_BASIST);
#endif
}

static_assert(pkb::REG_K3_LO + pkb::K3_LO_SIZE <= PACK_AREA_FLOATS && pkb::REG_S3_LO + pkb::S3_LO_SIZE <= PACK_AREA_FLOATS,
              "the backward images and their streamed lo pieces fit the pack area");

static void fill_bwd_common(BwdArgs& a, const RdrfFieldCfg* cfg, const float* rays, const float* ts,
                            const float* xyz, const float* z, const uint8_t* valid, int N, int S) {
  memset(&a, 0, sizeof(a));
  a.rays = rays; a.ts = ts; a.xyz = xyz; a.z = z; a.valid = valid; a.N = N; a.S = S;
  a.box = make_box(cfg);
  a.distance_scale = cfg->distance_scale; a.weight_thres = cfg->weight_thres;
  a.density_shift = cfg->density_shift; a.act = cfg->act; a.ray_type = cfg->ray_type;
  a.static_head = cfg->static_head;
  a.dynq = 1;   // per-workgroup tile queue (tile_queue_next)
}

static void fill_static_g(StaticG& g, const RdrfStaticParams* G) {
  g.density = G->density; g.app = G->app; g.b3 = G->b3; g.w3 = G->w3;
}
static void fill_dyn_g(DynG& g, const RdrfDynamicParams* G) {
  g.density = G->density; g.blending = G->blending; g.app = G->app;
  g.rbv = G->rbv; g.rwv = G->rwv; g.l5b = G->l5b; g.db2 = G->db2; g.bb2 = G->bb2;
  g.l5w = G->l5w; g.dw2 = G->dw2; g.bw2 = G->bw2;
}

// the two ray scan backward kernels with their launch geometry: the entry points below and ray_scan_bwd_on_arrays
static int launch_static_density_bwd(const BwdArgs& a, const StaticW& w, float* gf, hipStream_t stream) {
  RDRF_LAUNCH("static_density_bwd", k_static_density_bwd, dim3(a.N), dim3(64), stream, a, w, gf);   // a wave per ray
  return 0;
}
static int launch_ray_scan_bwd(const BwdArgs& a, hipStream_t stream) {
  RDRF_LAUNCH("ray_scan_bwd", k_ray_scan_bwd, dim3((a.N + 15) / 16), dim3(512), stream, a);   // 16 rays per workgroup
  return 0;
}
// The heads' kernel of the dynamic field's density phase (k_dyn_density_bwd<0>) with its launch geometry: the persistent one
// over the flat 32-sample tiles of the [N * S] array (training), the rays (wave per ray) or the a.N pseudo rays of feature
// mode.  The entry points below and heads_bwd_on_rows.
enum HeadsForm { HEADS_RAY, HEADS_FLAT, HEADS_FEAT };
long heads_bwd_units(int N, int S, int flat) { return flat ? ((long)N * S + 31) / 32 : (long)N; }
static int launch_heads_bwd(const char* name, HeadsForm form, const BwdArgs& a, const DynW& w, const DynG& gw, hipStream_t stream) {
  const Geo g = geo_for_units(heads_bwd_units(a.N, a.S, form == HEADS_FLAT));
  if (form == HEADS_FLAT) RDRF_LAUNCH(name, (k_dyn_density_bwd<0, false, true>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  else if (form == HEADS_FEAT) RDRF_LAUNCH(name, (k_dyn_density_bwd<0, true>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  else RDRF_LAUNCH(name, (k_dyn_density_bwd<0, false>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  return 0;
}
// k_time_branch_bwd over N rays (feature mode: points), TB_RPB rays per workgroup; dtp: the flat tiles' partial records or nullptr
int launch_time_branch_bwd(const float* ts, const DynW& w, int N, const float* dtout, const float* dtp, int S,
                           const RdrfDynamicParams* G, hipStream_t stream) {
  RDRF_LAUNCH("time_branch_bwd", k_time_branch_bwd, dim3((N + TB_RPB - 1) / TB_RPB), dim3(128), stream, ts, w, N, dtout, dtp, S,
              G->l1w, G->l1b, G->l2w, G->l2b);
  return 0;
}
// The backward-data kernels of the appearance phase with their launch geometry: persistent over the compacted 32-sample tiles of
// the [N * S] array (ray path; APP_RECORDS: the dynamic field's d(app features) as sample-major records in a.dfa) or over the a.N
// pseudo rays of feature mode.  The entry points below and app_bwd_on_rows.
long app_bwd_units(int N, int S, int feat) { return feat ? (long)N : ((long)N * S + 31) / 32; }
int launch_dyn_app_bwd(const char* name, AppBwdForm form, const BwdArgs& a, const DynW& w, const DynG& gw, hipStream_t stream) {
  const Geo g = geo_for_units(app_bwd_units(a.N, a.S, form == APP_FEAT));
  if (form == APP_RECORDS) RDRF_LAUNCH(name, (k_dyn_app_bwd<false, true>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  else if (form == APP_FEAT) RDRF_LAUNCH(name, k_dyn_app_bwd<true>, dim3(g.grid), dim3(g.block), stream, a, w, gw);
  else RDRF_LAUNCH(name, (k_dyn_app_bwd<false, false>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  return 0;
}
// feature mode runs the MLP_Fea instantiation for either head: only the basis backward is left of the kernel
int launch_static_app_bwd(const char* name, int head, AppBwdForm form, const BwdArgs& a, const StaticW& w, const StaticG& gw,
                          hipStream_t stream) {
  const Geo g = geo_for_units(app_bwd_units(a.N, a.S, form == APP_FEAT));
  if (form == APP_FEAT)
    RDRF_LAUNCH(name, (k_static_app_bwd<RDRF_HEAD_MLP_FEA, true>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  else if (head == RDRF_HEAD_MLP_FEA)
    RDRF_LAUNCH(name, (k_static_app_bwd<RDRF_HEAD_MLP_FEA, false>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  else
    RDRF_LAUNCH(name, (k_static_app_bwd<RDRF_HEAD_MLP_FEA_TIMEEMBEDDING, false>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  return 0;
}

// `valid` of a feature-mode batch: 1 for the M points, 0 for the padding of the last 32-point tile
static int pad_valid_tiles(uint8_t* valid, int M, size_t mp, hipStream_t stream) {
  RDRF_FILL(valid, 0, mp, stream);
  RDRF_FILL(valid, 1, (size_t)M, stream);
  return 0;
}

// ScatterArgs (after fill_scatter_common) of one appearance factor set: the DA rows of the appearance phase
static void scatter_app_set(ScatterArgs& sa, const RdrfVM& vm, const RdrfVM& gvm, const float* grows3) {
  sa.vm[0] = vm; sa.gvm[0] = gvm; sa.nsets = 1;
  sa.rows = grows3; sa.stride = sv::K3G_ROWS; sa.row0[0] = sv::K3G_DA;
}
// ... and of the density / blending sets.  A head without an upstream gradient (passes B-D of the trainer carry none for the
// blending head before the late mask terms) has d(features) == 0 and wrote no rows (k_dyn_density_bwd<0>): its factor set is
// left out of the launch instead of being walked with zeros
static void scatter_head_sets(ScatterArgs& sa, const BwdArgs& a, const RdrfDynamicParams* P, const RdrfDynamicParams* G,
                              bool has_d, bool has_b, float* dxw) {
  sa.nsets = 0;
  if (has_d) { sa.vm[sa.nsets] = P->density; sa.gvm[sa.nsets] = G->density; sa.row0[sa.nsets] = sv::K1G_DFD; ++sa.nsets; }
  if (has_b) { sa.vm[sa.nsets] = P->blending; sa.gvm[sa.nsets] = G->blending; sa.row0[sa.nsets] = sv::K1G_DFB; ++sa.nsets; }
  sa.rows = a.grows1; sa.stride = sv::K1G_ROWS;
  sa.xw = a.sp.xw;
  sa.dxw = dxw; sa.dxw_accumulate = 1;
}

// backward workspace of either field.  dynamic: dz rows of both phases, coordinate-gradient buffers, d(tout); the sorted
// scatter's sample-major d(feature) records and sort buffers; the flat-tile density phase's total d(sigma) per sample and
// the d(tout) partial records of the tiles
static void carve_bwd(BwdWs& b, WsCarver& c, int N, int S, int dynamic) {
  size_t ns = (size_t)N * S, t1 = (size_t)N * ((S + 31) / 32), t3 = (ns + 31) / 32;
  b.pk = c.take<float>(PACK_AREA_FLOATS);
  b.grows3 = c.take<float>(t3 * sv::K3G_ROWS * 32);
  b.grows1 = dynamic ? c.take<float>(t1 * sv::K1G_ROWS * 32) : nullptr;
  b.dxw = dynamic ? c.take<float>(ns * 3) : nullptr;
  b.dxn = dynamic ? c.take<float>(ns * 3) : nullptr;
  b.dtout = dynamic ? c.take<float>((size_t)N * 32) : nullptr;
  b.gf = dynamic ? nullptr : c.take<float>(t1 * 32);
  b.dfs = nullptr;
  b.dfa = nullptr;
  b.gsig = b.dtp = nullptr;
  if (dynamic) {
    b.dfs = c.take<float>(ns * DFS_FLOATS);
    b.dfa = c.take<float>(ns * DFA_FLOATS);
    carve_sorted_scatter(b, c, ns);
    b.gsig = c.take<float>(ns);
    b.dtp = c.take<float>(t3 * 64);
  }
}
static int carve_bwd(BwdWs& b, void* ws, size_t ws_bytes, int N, int S, int dynamic) {
  WsCarver c(ws, ws_bytes);
  carve_bwd(b, c, N, S, dynamic);
  RDRF_CHECK(c.ok(), -3, "backward workspace too small: need %zu have %zu", c.off, ws_bytes);
  return 0;
}
// scene flow backward: the two-kernel path (k_scene_flow_bwd + dw_sf) carries its dz rows through the workspace
static void carve_sf_bwd(float*& pk, float*& grows, WsCarver& c, size_t tiles, bool fused) {
  pk = c.take<float>(PACK_AREA_FLOATS);
  grows = fused ? nullptr : c.take<float>(tiles * sv::SFG_ROWS * 32);
}

// One workspace serves every call of a training step: the largest of the three backward carves and the forward size.  The
// dynamic carve decides at every shape -- it has the pack area and the appearance rows of the static one and t1 * K1G_ROWS
// * 32 floats of density rows against t1 * 32, more appearance rows than the scene flow has rows at all (K3G_ROWS >
// SFG_ROWS), and 28 N S bytes of coordinate and sigma buffers against the forward's 16 N S -- the others are kept in the
// maximum so that this stays true by construction.
extern "C" size_t rdrf_workspace_bytes(int N, int S) {
  BwdWs b;
  float *pk, *grows;
  WsCarver st, dy, sf;
  carve_bwd(b, st, N, S, 0);
  carve_bwd(b, dy, N, S, 1);
  carve_sf_bwd(pk, grows, sf, ((size_t)N * S + 31) / 32, false);
  size_t m = rdrf_forward_workspace_bytes(N, S);
  m = st.off > m ? st.off : m;
  m = dy.off > m ? dy.off : m;
  return sf.off > m ? sf.off : m;
}

// dW jobs of the dynamic field's density phase (warp MLP, density / blending heads)
void add_density_phase_dw(DwJobs& D, const float* grows1, const float* act1, const RdrfDynamicParams* G, int T1, bool live_d,
                          bool live_b, bool small_in_kernel, bool warp_in_kernel) {
  // warp_in_kernel: the fused warp kernel (rdrf_bwd_fused.hip) formed the gradients of layer3 and layer4 (and wrote no DZ3 / DZ4 rows)
  if (!warp_in_kernel) {
  // layer3: [X0 | tout]
  dw_add(D, grows1, sv::K1G_ROWS, sv::K1G_DZ3, 2, 64, 0, act1, sv::K1_ROWS, 93, 93, G->l3w, G->l3b, nullptr, T1);
  dw_blk(D, sv::K1_X0, SEG_WARP3_X0, 0);
  dw_blk(D, sv::K1_X0 + 32, SEG_WARP3_X0, 32);
  dw_blk(D, sv::K1_T, SEG_WARP3_T, 0);
  dw_add(D, grows1, sv::K1G_ROWS, sv::K1G_DZ4, 2, 64, 0, act1, sv::K1_ROWS, 64, 64, G->l4w, G->l4b, nullptr, T1);
  dw_blk(D, sv::K1_H3, SEG_IDENT, 0);
  dw_blk(D, sv::K1_H3 + 32, SEG_IDENT, 32);
  }
  // small layers share one dz block: rows 0..2 -> layer5, row 3 -> density_layer2, row 4 -> blending_layer2.
  // On the ray path k_dyn_density_bwd forms these gradients itself (reduce_scatter32): as MFMA products they were 6 of
  // the 40 per tile, 27 of 32 rows empty, and the 12 waves of the dW kernel take 34 products in 3 rounds instead of 4
  if (!small_in_kernel) {
  dw_add(D, grows1, sv::K1G_ROWS, sv::K1G_SM, 1, 3, 0, act1, sv::K1_ROWS, 64, 64, G->l5w, G->l5b, nullptr, T1);
  dw_blk(D, sv::K1_H4, SEG_IDENT, 0);
  dw_blk(D, sv::K1_H4 + 32, SEG_IDENT, 32);
  if (live_d) {
    dw_add(D, grows1, sv::K1G_ROWS, sv::K1G_SM, 1, 1, 3, act1, sv::K1_ROWS, 64, 64, G->dw2, G->db2, nullptr, T1);
    dw_blk(D, sv::K1_HD, SEG_IDENT, 0);
    dw_blk(D, sv::K1_HD + 32, SEG_IDENT, 32);
  }
  if (live_b) {
    dw_add(D, grows1, sv::K1G_ROWS, sv::K1G_SM, 1, 1, 4, act1, sv::K1_ROWS, 64, 64, G->bw2, G->bb2, nullptr, T1);
    dw_blk(D, sv::K1_HB, SEG_IDENT, 0);
    dw_blk(D, sv::K1_HB + 32, SEG_IDENT, 32);
  }
  }
  for (int head = 0; head < 2; ++head) {
    if (!(head ? live_b : live_d)) continue;   // dead head: its dz rows were not written (k_dyn_density_bwd<0>)
    dw_add(D, grows1, sv::K1G_ROWS, head ? sv::K1G_DZB : sv::K1G_DZD, 2, 64, 0, act1, sv::K1_ROWS, 152, 152,
           head ? G->bw1 : G->dw1, head ? G->bb1 : G->db1, nullptr, T1);
    const int f0 = head ? sv::K1_FB : sv::K1_FD;
    dw_blk(D, f0, SEG_IDENT72, 0);
    dw_blk(D, f0 + 32, SEG_IDENT72, 32);
    dw_blk(D, f0 + 64, SEG_IDENT72, 64);
    dw_blk(D, sv::K1_X0, SEG_DEN1_X0, 0);
    dw_blk(D, sv::K1_X0 + 32, SEG_DEN1_X0, 32);
    dw_blk(D, sv::K1_X1, SEG_DEN1_X1, 0);
  }
}
// The warp MLP backward of the flat training path: the fused kernel behind launch_warp_fused (rdrf_bwd_fused.hip) forms the
// gradients of layer3 / layer4 itself (it needs the 3-row layer's sums in the kernel as well: small_dw).  RDRF_WARP_FUSED=0 (tools build): k_dyn_density_bwd<1, false, true> + their
// products in k_dw3, its A/B partner.  The wave-per-ray and feature-mode paths keep the two kernels.
static bool warp_fused_path(bool flat, bool small_dw) {
  static const int fused = RDRF_ENV("RDRF_WARP_FUSED") ? atoi(RDRF_ENV("RDRF_WARP_FUSED")) : 1;
  return flat && small_dw && fused != 0;
}
// static appearance phase (compacted: device count), MLP_Fea (fea) or MLP_Fea_TimeEmbedding head
void add_static_app_dw(DwJobs& D, const float* grows3, const float* act3, const RdrfStaticParams* G, bool fea, const int* cnt,
                       int ntiles) {
  const int in1 = fea ? 138 : 135;
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DZV, 1, 3, 0, act3, sv::S3_ROWS, 128,
         fea ? 128 : 131, G->w3, G->b3, cnt, ntiles);
  for (int i = 0; i < 4; ++i) dw_blk(D, sv::S3_H2 + 32 * i, SEG_IDENT, 32 * i);
  if (!fea) dw_blk(D, sv::S3_VD, SEG_VIEW3, 0);
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DF, 1, 27, 0, act3, sv::S3_ROWS, 72, 72, G->basis,
         nullptr, cnt, ntiles);
  for (int i = 0; i < 3; ++i) dw_blk(D, sv::S3_G + 32 * i, SEG_IDENT, 32 * i);
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DZ2, 4, 128, 0, act3, sv::S3_ROWS, 128, 128, G->w2,
         G->b2, cnt, ntiles);
  for (int i = 0; i < 4; ++i) dw_blk(D, sv::S3_H1 + 32 * i, SEG_IDENT, 32 * i);
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DZ1, 4, 128, 0, act3, sv::S3_ROWS, in1, in1, G->w1,
         G->b1, cnt, ntiles);
  dw_blk(D, sv::S3_F, fea ? SEG_STAT1_F_FEA : SEG_STAT1_F_TE, 0);
  for (int i = 0; i < 4; ++i) dw_blk(D, sv::S3_P + 32 * i, fea ? SEG_STAT1_P_FEA : SEG_STAT1_P_TE, 32 * i);
}
// dynamic appearance phase (compacted: device count)
void add_dyn_app_dw(DwJobs& D, const float* grows3, const float* act3, const RdrfDynamicParams* G, const int* cnt, int ntiles) {
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DZV, 1, 3, 0, act3, sv::K3_ROWS, 128, 131, G->rwv,
         G->rbv, cnt, ntiles);
  for (int i = 0; i < 4; ++i) dw_blk(D, sv::K3_H2 + 32 * i, SEG_IDENT, 32 * i);
  dw_blk(D, sv::K3_VD, SEG_VIEW3, 0);
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DF, 1, 27, 0, act3, sv::K3_ROWS, 216, 216, G->basis,
         nullptr, cnt, ntiles);
  for (int i = 0; i < 7; ++i) dw_blk(D, sv::K3_A + 32 * i, SEG_IDENT, 32 * i);
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DZ2, 4, 128, 0, act3, sv::K3_ROWS, 128, 128, G->rw2,
         G->rb2, cnt, ntiles);
  for (int i = 0; i < 4; ++i) dw_blk(D, sv::K3_H1 + 32 * i, SEG_IDENT, 32 * i);
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DZ1, 4, 128, 0, act3, sv::K3_ROWS, 107, 107, G->rw1,
         G->rb1, cnt, ntiles);
  dw_blk(D, sv::K3_F, SEG_RGB1_F, 0);
  dw_blk(D, sv::K3_X0, SEG_RGB1_X0, 0);
  dw_blk(D, sv::K3_X0 + 32, SEG_RGB1_X0, 32);
  dw_blk(D, sv::K3_X1, SEG_RGB1_X1, 0);
}
// scene flow MLP
void add_scene_flow_dw(DwJobs& D, const float* grows, const float* act, const RdrfDynamicParams* G, int T) {
  dw_add(D, grows, sv::SFG_ROWS, sv::SFG_DZ6, 1, 6, 0, act, sv::SF_ROWS, 64, 64, G->sfw[3], G->sfb[3],
         nullptr, T);
  dw_blk(D, sv::SF_H4, SEG_IDENT, 0);
  dw_blk(D, sv::SF_H4 + 32, SEG_IDENT, 32);
  dw_add(D, grows, sv::SFG_ROWS, sv::SFG_DZ4, 2, 64, 0, act, sv::SF_ROWS, 64, 64, G->sfw[2], G->sfb[2],
         nullptr, T);
  dw_blk(D, sv::SF_H2, SEG_IDENT, 0);
  dw_blk(D, sv::SF_H2 + 32, SEG_IDENT, 32);
  dw_add(D, grows, sv::SFG_ROWS, sv::SFG_DZ2, 2, 64, 0, act, sv::SF_ROWS, 64, 64, G->sfw[1], G->sfb[1],
         nullptr, T);
  dw_blk(D, sv::SF_H0, SEG_IDENT, 0);
  dw_blk(D, sv::SF_H0 + 32, SEG_IDENT, 32);
  dw_add(D, grows, sv::SFG_ROWS, sv::SFG_DZ0, 2, 64, 0, act, sv::SF_ROWS, 36, 36, G->sfw[0], G->sfb[0],
         nullptr, T);
  dw_blk(D, sv::SF_X, SEG_SF_X, 0);
  dw_blk(D, sv::SF_X + 32, SEG_SF_X, 32);
}
// feature mode: the basis matrix of the static / the dynamic appearance features (Np tiles of 32 points)
void add_feat_static_dw(DwJobs& D, const float* grows3, const float* act3, const RdrfStaticParams* G, int Np) {
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DF, 1, 27, 0, act3, sv::S3_ROWS, 72, 72, G->basis, nullptr,
         nullptr, Np);
  for (int i = 0; i < 3; ++i) dw_blk(D, sv::S3_G + 32 * i, SEG_IDENT, 32 * i);
}
void add_feat_dyn_app_dw(DwJobs& D, const float* grows3, const float* act3, const RdrfDynamicParams* G, int Np) {
  dw_add(D, grows3, sv::K3G_ROWS, sv::K3G_DF, 1, 27, 0, act3, sv::K3_ROWS, 216, 216, G->basis, nullptr,
         nullptr, Np);
  for (int i = 0; i < 7; ++i) dw_blk(D, sv::K3_A + 32 * i, SEG_IDENT, 32 * i);
}

extern "C" int rdrf_static_bwd(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* rays,
                               const float* ts, const float* xyz, const float* z,
                               const uint8_t* valid, int N, int S, const float* g_rgb,
                               const float* g_sigma, const float* g_weight, const float* g_dists,
                               const RdrfStaticParams* G, float* g_xyz, float* g_z, float* g_rays,
                               void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                               rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && G && saved && N > 0 && S > 0 && S <= 4096, -1, "static_bwd: bad arguments (S <= 4096)");
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "static_bwd: N * S * 3 must stay below 2^31 (32-bit sample indices)");
  // z_vals never depends on a trainable quantity in the reference (linspace + jitter)
  BwdArgs a;
  fill_bwd_common(a, cfg, rays, ts, xyz, z, valid, N, S);
  a.g_rgb = g_rgb; a.g_sigma = g_sigma; a.g_weight = g_weight; a.g_xyz = g_xyz;
  a.g_rays = g_rays; a.g_dists = g_dists; a.g_z = g_z;
  // a buffer the forward filled under RDRF_SAVE_NO_APP has no appearance rows (a prefix of the full layout): told apart by its
  // size, on the host, before anything is launched
  const int saved_kind = carve_saved_bwd(a.sp, saved, saved_bytes, 0, N, S);
  RDRF_CHECK(saved_kind >= 0, -3, "static_bwd: saved buffer too small");
  RDRF_CHECK(saved_kind == 1 || g_rgb == nullptr, -1,
             "static_bwd: the forward saved no appearance rows (RDRF_SAVE_NO_APP): no gradient can flow through rgb");
  BwdWs b;
  RDRF_TRY(carve_bwd(b, ws, ws_bytes, N, S, 0));
  a.grows3 = b.grows3;
  StaticW w;
  fill_static_w(w, P);
  StaticG gw;
  fill_static_g(gw, G);
  RDRF_TRY(pack_image(a.pk, P->packed_bwd, b.pk, stream, static_pack_jobs_bwd, P, cfg->static_head));
  const size_t t3 = ((size_t)N * S + 31) / 32;
  if (g_rgb != nullptr) {
    RDRF_TRY(launch_static_app_bwd("static_app_bwd", cfg->static_head, APP_ROWS, a, w, gw, stream));
    const int* cnt = &a.sp.hdr->count;
    ScatterArgs sa;
    fill_scatter_common(sa, a);
    scatter_app_set(sa, P->app, G->app, b.grows3);
    sa.list = a.sp.list; sa.count = cnt;
    sa.g_xyz = g_xyz;
    RDRF_TRY(launch_scatter("scatter_static_app", SCATTER_12_3_9, sa, (long)t3, stream));
    DwJobs D;
    D.n = 0;
    add_static_app_dw(D, b.grows3, a.sp.act3, G, cfg->static_head == RDRF_HEAD_MLP_FEA, cnt, 0);
    RDRF_TRY(dw_launch(D, stream, "dw_static"));
  }
  if (g_sigma != nullptr || g_weight != nullptr || ((g_rays != nullptr || g_z != nullptr) && g_dists != nullptr)) {
    RDRF_TRY(launch_static_density_bwd(a, w, b.gf, stream));
    if (g_sigma != nullptr || g_weight != nullptr) {
      ScatterArgs sa;
      fill_scatter_common(sa, a);
      sa.vm[0] = P->density; sa.gvm[0] = G->density; sa.nsets = 1;
      sa.rows = b.gf; sa.stride = 1; sa.row0[0] = 0; sa.bcast = 1;
      sa.g_xyz = g_xyz;
      RDRF_TRY(launch_scatter("scatter_static_density", SCATTER_4_1_3, sa, (long)N * ((S + 31) / 32), stream));
    }
  }
  return 0;
}

extern "C" int rdrf_dynamic_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg,
                                const float* rays, const float* ts, const float* xyz,
                                const float* z, const uint8_t* valid, int N, int S,
                                const float* g_blending, const float* g_weight,
                                const float* g_xyz_prime, const float* g_rgb, const float* g_sigma,
                                const float* g_dists, const RdrfDynamicParams* G, float* g_xyz,
                                float* g_z, float* g_rays, void* saved, size_t saved_bytes, void* ws,
                                size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && G && saved && N > 0 && S > 0 && S <= 4096, -1, "dynamic_bwd: bad arguments (S <= 4096)");
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "dynamic_bwd: N * S * 3 must stay below 2^31 (32-bit sample indices)");
  BwdArgs a;
  fill_bwd_common(a, cfg, rays, ts, xyz, z, valid, N, S);
  a.g_rgb = g_rgb; a.g_sigma = g_sigma; a.g_weight = g_weight; a.g_blending = g_blending;
  a.g_xyz_prime = g_xyz_prime; a.g_xyz = g_xyz; a.g_rays = g_rays; a.g_dists = g_dists; a.g_z = g_z;
  a.small_dw = 1;
  // a buffer the forward filled under RDRF_SAVE_NO_APP has no appearance rows (a prefix of the full layout): told apart by its
  // size, on the host, before anything is launched
  const int saved_kind = carve_saved_bwd(a.sp, saved, saved_bytes, 1, N, S);
  RDRF_CHECK(saved_kind >= 0, -3, "dynamic_bwd: saved buffer too small");
  RDRF_CHECK(saved_kind == 1 || g_rgb == nullptr, -1,
             "dynamic_bwd: the forward saved no appearance rows (RDRF_SAVE_NO_APP): no gradient can flow through rgb");
  BwdWs b;
  RDRF_TRY(carve_bwd(b, ws, ws_bytes, N, S, 1));
  a.grows1 = b.grows1; a.grows3 = b.grows3; a.dxw_app = b.dxw; a.dxn_app = b.dxn;
  a.dtout = b.dtout;
  // the density phase on flat 32-sample tiles (the forward wrote its saved rows that way: rdrf_dynamic_fwd)
  const bool flat = rdrf_flat_density();
  a.gsig = b.gsig; a.dtp = b.dtp;
  DynW w;
  fill_dyn_w(w, P);
  DynG gw;
  fill_dyn_g(gw, G);
  RDRF_TRY(pack_image(a.pk, P->packed_bwd, b.pk, stream, dyn_pack_jobs_bwd, P));
  const size_t ns = (size_t)N * S, t3 = (ns + 31) / 32, t1 = flat ? t3 : (size_t)N * ((S + 31) / 32);   // density-phase tiles
  RDRF_FILL(b.dxw, 0, ns * 3 * 4, stream);
  RDRF_FILL(b.dxn, 0, ns * 3 * 4, stream);
  const int* cnt = &a.sp.hdr->count;
  DwJobs D;
  D.n = 0;
  if (g_rgb != nullptr) {
    const int smode_app = scatter_mode(ns, stream);
    a.dfa = smode_app != 0 ? b.dfa : nullptr;   // sorted: k_dyn_app_bwd writes sample-major records instead of DA rows
    RDRF_TRY(launch_dyn_app_bwd("dyn_app_bwd", smode_app != 0 ? APP_RECORDS : APP_ROWS, a, w, gw, stream));
    if (smode_app != 0) {
      rdrf_prof_begin("scatter_dyn_app", stream);
      const int rc = scatter_dyn_app_sorted(a, b, P, G, stream);
      rdrf_prof_end("scatter_dyn_app", stream);
      if (rc) return rc;
    } else {
      ScatterArgs sa;
      fill_scatter_common(sa, a);
      scatter_app_set(sa, P->app, G->app, b.grows3);
      sa.xw = a.sp.xw; sa.list = a.sp.list; sa.count = cnt;
      sa.dxw = b.dxw; sa.dxw_accumulate = 0;
      RDRF_TRY(launch_scatter("scatter_dyn_app", SCATTER_12_3_27, sa, (long)t3, stream));
    }
    add_dyn_app_dw(D, b.grows3, a.sp.act3, G, cnt, 0);
  }
  {
    const Geo g = geo_for_units(flat ? (long)t1 : (long)N);
    const int smode = scatter_mode(ns, stream);
    a.dfs = smode != 0 ? b.dfs : nullptr;
    if (flat) RDRF_TRY(launch_ray_scan_bwd(a, stream));
    RDRF_TRY(launch_heads_bwd("dyn_heads_bwd", flat ? HEADS_FLAT : HEADS_RAY, a, w, gw, stream));
    const bool has_d = g_sigma != nullptr || g_weight != nullptr, has_b = g_blending != nullptr;
    if (smode != 0) {
      if (has_d || has_b) {
        rdrf_prof_begin("scatter_dyn_density", stream);
        const int rc = scatter_dyn_density_sorted(a, b, P, G, (has_d ? 1 : 0) | (has_b ? 2 : 0), stream);
        rdrf_prof_end("scatter_dyn_density", stream);
        if (rc) return rc;
      }
    } else if (has_d || has_b) {
      ScatterArgs sa;
      fill_scatter_common(sa, a);
      scatter_head_sets(sa, a, P, G, has_d, has_b, b.dxw);
      sa.flat = flat ? 1 : 0;
      RDRF_TRY(launch_scatter("scatter_dyn_density", SCATTER_4_1_9, sa, (long)t1, stream));
    }
    const bool warp_fused = warp_fused_path(flat, a.small_dw != 0);
    if (warp_fused) RDRF_TRY(launch_warp_fused(a, gw, G, (long)t1, stream));
    else if (flat) RDRF_LAUNCH("dyn_warp_bwd", (k_dyn_density_bwd<1, false, true>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
    else RDRF_LAUNCH("dyn_warp_bwd", (k_dyn_density_bwd<1, false>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
    RDRF_TRY(launch_time_branch_bwd(ts, w, N, b.dtout, flat ? (const float*)b.dtp : nullptr, S, G, stream));
    add_density_phase_dw(D, b.grows1, a.sp.act1, G, (int)t1, has_d, has_b, a.small_dw != 0, warp_fused);
  }
  return dw_launch(D, stream, "dw_dyn");
}

// ------------------------------------------------------------------------------------------------
// feature mode backward (compute_* / warp_coordinate): gradients of the raw features wrt every
// parameter they depend on and wrt the input coordinates; pseudo-ray geometry (rdrf_fwd.hip)
// ------------------------------------------------------------------------------------------------
struct FeatWs {
  float *pk, *grows3, *grows1, *dxw, *dxn, *dtout, *gpad, *xpad;
  uint8_t* valid;
};
static void carve_feat_bwd(FeatWs& b, WsCarver& c, int M, int dynamic) {
  const size_t t = ((size_t)M + 31) / 32, mp = t * 32;
  b.pk = c.take<float>(PACK_AREA_FLOATS);
  b.grows3 = c.take<float>(t * sv::K3G_ROWS * 32);
  b.grows1 = dynamic ? c.take<float>(t * sv::K1G_ROWS * 32) : nullptr;
  b.dxw = dynamic ? c.take<float>(mp * 3) : nullptr;
  b.dxn = dynamic ? c.take<float>(mp * 3) : nullptr;
  b.dtout = dynamic ? c.take<float>(mp * 32) : nullptr;
  b.gpad = dynamic ? nullptr : c.take<float>(mp);
  b.xpad = dynamic ? nullptr : c.take<float>(mp * 3);
  b.valid = c.take<uint8_t>(mp);
}
static int carve_feat_bwd(FeatWs& b, void* ws, size_t ws_bytes, int M, int dynamic) {
  WsCarver c(ws, ws_bytes);
  carve_feat_bwd(b, c, M, dynamic);
  RDRF_CHECK(c.ok(), -3, "features backward: workspace too small: need %zu have %zu", c.off, ws_bytes);
  return 0;
}
extern "C" size_t rdrf_features_bwd_workspace_bytes(int M) {   // of either field: the dynamic carve is the larger one
  FeatWs b;
  WsCarver st, dy;
  carve_feat_bwd(b, st, M, 0);
  carve_feat_bwd(b, dy, M, 1);
  return st.off > dy.off ? st.off : dy.off;
}

extern "C" int rdrf_static_features_bwd(const RdrfStaticParams* P, const RdrfFieldCfg* cfg, const float* xn,
                                        int M, const float* g_density, const float* g_app,
                                        const RdrfStaticParams* G, float* g_xn, void* saved, size_t saved_bytes,
                                        void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && G && xn && M > 0 && (g_density || g_app), -1, "static_features_bwd: bad arguments");
  RDRF_CHECK(g_app == nullptr || saved != nullptr, -1, "static_features_bwd: the appearance features need the "
             "saved buffer of their forward call");
  const int Np = (M + 31) / 32;
  const size_t mp = (size_t)Np * 32;
  FeatWs b;
  RDRF_TRY(carve_feat_bwd(b, ws, ws_bytes, M, 0));
  BwdArgs a;
  fill_bwd_common(a, cfg, nullptr, nullptr, xn, nullptr, b.valid, Np, 32);
  a.M = M; a.in_norm = 1; a.g_feat = g_app; a.pk = b.pk; a.grows3 = b.grows3;
  if (saved != nullptr)
    RDRF_CHECK(carve_saved_feat(a.sp, saved, saved_bytes, 0, M), -3, "static_features_bwd: saved buffer too small");
  RDRF_TRY(pad_valid_tiles(b.valid, M, mp, stream));
  RDRF_FILL(b.xpad, 0, mp * 3 * 4, stream);
  RDRF_HIP(hipMemcpyAsync(b.xpad, xn, (size_t)M * 3 * 4, hipMemcpyDeviceToDevice, stream));
  ScatterArgs sa0;
  fill_scatter_common(sa0, a);
  sa0.xw = b.xpad;                       // already normalised
  sa0.box.inv[0] = sa0.box.inv[1] = sa0.box.inv[2] = 1.0f;   // g_xn is the gradient wrt the normalised input
  sa0.g_xyz = g_xn;
  if (g_density != nullptr) {            // the feature is the plain sum of the 24 products: broadcast rows
    RDRF_FILL(b.gpad, 0, mp * 4, stream);
    RDRF_HIP(hipMemcpyAsync(b.gpad, g_density, (size_t)M * 4, hipMemcpyDeviceToDevice, stream));
    ScatterArgs sa = sa0;
    sa.vm[0] = P->density; sa.gvm[0] = G->density; sa.nsets = 1;
    sa.rows = b.gpad; sa.stride = 1; sa.row0[0] = 0; sa.bcast = 1;
    RDRF_TRY(launch_scatter("feat_scatter_static_density", SCATTER_4_1_3, sa, (long)Np, stream));
  }
  if (g_app != nullptr) {
    StaticW w;
    fill_static_w(w, P);
    StaticG gw;
    fill_static_g(gw, G);
    RDRF_TRY(pack_image(a.pk, P->packed_bwd, b.pk, stream, static_pack_jobs_bwd, P, cfg->static_head));
    RDRF_TRY(launch_static_app_bwd("feat_static_app_bwd", cfg->static_head, APP_FEAT, a, w, gw, stream));
    ScatterArgs sa = sa0;
    scatter_app_set(sa, P->app, G->app, b.grows3);
    RDRF_TRY(launch_scatter("feat_scatter_static_app", SCATTER_12_3_9, sa, (long)Np, stream));
    DwJobs D;
    D.n = 0;
    add_feat_static_dw(D, b.grows3, a.sp.act3, G, Np);
    RDRF_TRY(dw_launch(D, stream, "feat_dw_static"));
  }
  return 0;
}

extern "C" int rdrf_dynamic_features_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, const float* x,
                                         const float* t, int M, int x_is_normalized, const float* g_density,
                                         const float* g_blending, const float* g_app, const float* g_xyz_prime,
                                         const RdrfDynamicParams* G, float* g_x, void* saved, size_t saved_bytes,
                                         void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && G && x && t && saved && M > 0 && (g_density || g_blending || g_app || g_xyz_prime), -1,
             "dynamic_features_bwd: bad arguments");
  const int Np = (M + 31) / 32;
  const size_t mp = (size_t)Np * 32;
  FeatWs b;
  RDRF_TRY(carve_feat_bwd(b, ws, ws_bytes, M, 1));
  BwdArgs a;
  fill_bwd_common(a, cfg, nullptr, t, x, nullptr, b.valid, Np, 32);
  a.M = M; a.in_norm = x_is_normalized ? 1 : 0;
  a.g_sigma = g_density; a.g_blending = g_blending; a.g_feat = g_app; a.g_xyz_prime = g_xyz_prime; a.g_xyz = g_x;
  RDRF_CHECK(carve_saved_feat(a.sp, saved, saved_bytes, 1, M), -3, "dynamic_features_bwd: saved buffer too small");
  a.grows1 = b.grows1; a.grows3 = b.grows3; a.dxw_app = b.dxw; a.dxn_app = b.dxn; a.dtout = b.dtout;
  DynW w;
  fill_dyn_w(w, P);
  DynG gw;
  fill_dyn_g(gw, G);
  RDRF_TRY(pack_image(a.pk, P->packed_bwd, b.pk, stream, dyn_pack_jobs_bwd, P));
  RDRF_TRY(pad_valid_tiles(b.valid, M, mp, stream));
  RDRF_FILL(b.dxw, 0, mp * 3 * 4, stream);
  RDRF_FILL(b.dxn, 0, mp * 3 * 4, stream);
  const Geo g = geo_for_units(Np);
  DwJobs D;
  D.n = 0;
  if (g_app != nullptr) {
    RDRF_TRY(launch_dyn_app_bwd("feat_dyn_app_bwd", APP_FEAT, a, w, gw, stream));
    ScatterArgs sa;
    fill_scatter_common(sa, a);
    scatter_app_set(sa, P->app, G->app, b.grows3);
    sa.xw = a.sp.xw;
    sa.dxw = b.dxw; sa.dxw_accumulate = 0;
    RDRF_TRY(launch_scatter("feat_scatter_dyn_app", SCATTER_12_3_27, sa, (long)Np, stream));
    add_feat_dyn_app_dw(D, b.grows3, a.sp.act3, G, Np);
  }
  RDRF_TRY(launch_heads_bwd("feat_dyn_heads_bwd", HEADS_FEAT, a, w, gw, stream));
  if (g_density != nullptr || g_blending != nullptr) {
    ScatterArgs sa;
    fill_scatter_common(sa, a);
    scatter_head_sets(sa, a, P, G, g_density != nullptr, g_blending != nullptr, b.dxw);
    RDRF_TRY(launch_scatter("feat_scatter_dyn_density", SCATTER_4_1_9, sa, (long)Np, stream));
  }
  RDRF_LAUNCH("feat_dyn_warp_bwd", (k_dyn_density_bwd<1, true>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  RDRF_TRY(launch_time_branch_bwd(t, w, M, b.dtout, nullptr, 32, G, stream));
  add_density_phase_dw(D, b.grows1, a.sp.act1, G, Np, g_density != nullptr, g_blending != nullptr);
  return dw_launch(D, stream, "feat_dw_dyn");
}

extern "C" int rdrf_scene_flow_bwd(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg,
                                   const float* pts, const float* ts, int N, int S,
                                   const float* g_sf_f, const float* g_sf_b,
                                   const RdrfDynamicParams* G, float* g_pts, void* saved,
                                   size_t saved_bytes, void* ws, size_t ws_bytes,
                                   rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(P && cfg && G && saved && N > 0 && S > 0, -1, "scene_flow_bwd: bad arguments");
  RDRF_CHECK((size_t)N * S * 3 < (size_t)INT32_MAX, -1, "scene_flow_bwd: N * S * 3 must stay below 2^31 (32-bit sample indices)");
  const size_t tiles = ((size_t)N * S + 31) / 32;
  RDRF_CHECK(saved_bytes >= tiles * sv::SF_ROWS * 32 * 4, -3, "scene_flow_bwd: saved buffer too small");
  // the fused kernel (launch_scene_flow_fused, rdrf_bwd_fused.hip) forms the weight gradients itself: no dz rows, no dw_sf launch.  RDRF_SF_FUSED=0 (tools build):
  // k_scene_flow_bwd + k_dw3, its A/B partner
  static const int fused = RDRF_ENV("RDRF_SF_FUSED") ? atoi(RDRF_ENV("RDRF_SF_FUSED")) : 1;
  WsCarver c(ws, ws_bytes);
  float *pkbuf, *grows;
  carve_sf_bwd(pkbuf, grows, c, tiles, fused != 0);
  RDRF_CHECK(c.ok(), -3, "scene_flow_bwd: workspace too small: need %zu have %zu", c.off, ws_bytes);
  const float* pkimg;
  RDRF_TRY(pack_image(pkimg, P->packed_bwd, pkbuf, stream, dyn_pack_jobs_bwd, P));
  if (fused)
    return launch_scene_flow_fused(N, S, make_box(cfg), pkimg, (const float*)saved, g_sf_f, g_sf_b, G, g_pts, (long)tiles, stream);
  const Geo g = geo_for_units((long)tiles);
  RDRF_LAUNCH("scene_flow_bwd", k_scene_flow_bwd, dim3(g.grid), dim3(g.block), stream, N, S,
              make_box(cfg), pkimg, (const float*)saved, grows, g_sf_f, g_sf_b, G->sfb[3], g_pts);
  DwJobs D;
  D.n = 0;
  add_scene_flow_dw(D, grows, (const float*)saved, G, (int)tiles);
  return dw_launch(D, stream, "dw_sf");
}

// ------------------------------------------------------------------------------------------------
// caller-managed packed weight images (include/rodynrf.h)
// ------------------------------------------------------------------------------------------------
extern "C" size_t rdrf_pack_floats(void) { return PACK_AREA_FLOATS; }
extern "C" int rdrf_static_pack(const RdrfStaticParams* P, int static_head, int backward, float* image,
                                rdrf_stream_t stream_) {
  RDRF_CHECK(P && image && (((uintptr_t)image) & 15) == 0, -1, "static_pack: bad arguments");
  PackJobs J;
  if (backward) static_pack_jobs_bwd(J, P, static_head); else static_pack_jobs_fwd(J, P, static_head);
  return pack_launch(J, image, (hipStream_t)stream_);
}
extern "C" int rdrf_dynamic_pack(const RdrfDynamicParams* P, int backward, float* image, rdrf_stream_t stream_) {
  RDRF_CHECK(P && image && (((uintptr_t)image) & 15) == 0, -1, "dynamic_pack: bad arguments");
  PackJobs J;
  if (backward) dyn_pack_jobs_bwd(J, P); else dyn_pack_jobs_fwd(J, P);
  return pack_launch(J, image, (hipStream_t)stream_);
}

// ------------------------------------------------------------------------------------------------
// the warp MLP backward alone on caller-supplied rows (rdrf_bwd_host.hpp; rdrf_selftest_warp_bwd)
// ------------------------------------------------------------------------------------------------
int warp_bwd_on_rows(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, int N, int S, const float* act1, float* grows1,
                     float* dxw, float* dxn, const float* g_xyz_prime, const RdrfDynamicParams* G, float* g_xyz, float* dtout,
                     float* dtp, float* pk, uint8_t* valid, hipStream_t stream) {
  BwdArgs a;
  fill_bwd_common(a, cfg, nullptr, nullptr, nullptr, nullptr, valid, N, S);
  a.g_xyz_prime = g_xyz_prime; a.g_xyz = g_xyz;
  a.small_dw = 1;
  a.sp.act1 = const_cast<float*>(act1);
  a.grows1 = grows1; a.dxw_app = dxw; a.dxn_app = dxn; a.dtout = dtout; a.dtp = dtp;
  DynW w;
  fill_dyn_w(w, P);
  DynG gw;
  memset(&gw, 0, sizeof(gw));
  gw.l5b = G->l5b; gw.l5w = G->l5w;
  RDRF_TRY(pack_image(a.pk, P->packed_bwd, pk, stream, dyn_pack_jobs_bwd, P));
  const size_t ns = (size_t)N * S, t1 = (ns + 31) / 32;
  RDRF_FILL(valid, 1, ns, stream);
  if (warp_fused_path(true, true)) return launch_warp_fused(a, gw, G, (long)t1, stream);
  const Geo g = geo_for_units((long)t1);
  RDRF_LAUNCH("dyn_warp_bwd", (k_dyn_density_bwd<1, false, true>), dim3(g.grid), dim3(g.block), stream, a, w, gw);
  DwJobs D;
  D.n = 0;
  add_density_phase_dw(D, grows1, act1, G, (int)t1, false, false, true, false);
  return dw_launch(D, stream, "dw_warp");
}

// ------------------------------------------------------------------------------------------------
// the heads' backward alone on caller-supplied rows (rdrf_bwd_host.hpp; rdrf_selftest_heads_bwd)
// ------------------------------------------------------------------------------------------------
int heads_bwd_on_rows(const RdrfDynamicParams* P, const RdrfFieldCfg* cfg, int feat, int N, int S, int M, const float* act1,
                      const float* raw, const uint8_t* valid, const float* gsig, const float* g_sigma, const float* g_blending,
                      int live_d, float* grows1, float* dfs, const RdrfDynamicParams* G, float* pk, hipStream_t stream) {
  BwdArgs a;
  fill_bwd_common(a, cfg, nullptr, nullptr, nullptr, nullptr, valid, N, S);
  a.small_dw = 1;
  a.sp.act1 = const_cast<float*>(act1);
  a.sp.raw = const_cast<float*>(raw);
  a.grows1 = grows1;
  a.g_blending = g_blending;
  if (feat) {
    a.M = M; a.g_sigma = g_sigma;
  } else {
    a.gsig = const_cast<float*>(gsig); a.dfs = dfs;
    a.g_sigma = live_d ? gsig : nullptr;   // never read on flat tiles: the kernel takes the head's liveness from it
  }
  DynW w;
  fill_dyn_w(w, P);
  DynG gw;
  memset(&gw, 0, sizeof(gw));
  gw.dw2 = G->dw2; gw.db2 = G->db2; gw.bw2 = G->bw2; gw.bb2 = G->bb2;
  RDRF_TRY(pack_image(a.pk, P->packed_bwd, pk, stream, dyn_pack_jobs_bwd, P));
  return launch_heads_bwd(feat ? "feat_dyn_heads_bwd" : "dyn_heads_bwd", feat ? HEADS_FEAT : HEADS_FLAT, a, w, gw, stream);
}

// ------------------------------------------------------------------------------------------------
// the appearance backward-data kernels alone on caller-supplied rows (rdrf_bwd_host.hpp; rdrf_selftest_app_bwd)
// ------------------------------------------------------------------------------------------------
int app_bwd_on_rows(const void* P, const RdrfFieldCfg* cfg, int dynamic, AppBwdForm form, int N, int S, int M, const float* act3,
                    const int* list, const int* count, const float* rays, const float* g_rgb, const float* g_feat, float* grows3,
                    float* dfa, float* dxn, float* g_rays, float* pk, hipStream_t stream) {
  BwdArgs a;
  fill_bwd_common(a, cfg, rays, nullptr, nullptr, nullptr, nullptr, N, S);
  static_assert(offsetof(SavedHdr, count) == 0, "the device count stands for the saved buffer's header");
  a.sp.hdr = reinterpret_cast<SavedHdr*>(const_cast<int*>(count));
  a.sp.list = const_cast<int*>(list);
  a.sp.act3 = const_cast<float*>(act3);
  a.g_rgb = g_rgb; a.g_feat = g_feat; a.g_rays = g_rays;
  a.grows3 = grows3; a.dfa = dfa; a.dxn_app = dxn;
  if (form == APP_FEAT) { a.M = M; a.in_norm = 1; }
  if (dynamic) {
    const RdrfDynamicParams* PD = static_cast<const RdrfDynamicParams*>(P);
    DynW w;
    fill_dyn_w(w, PD);
    DynG gw;
    memset(&gw, 0, sizeof(gw));
    RDRF_TRY(pack_image(a.pk, PD->packed_bwd, pk, stream, dyn_pack_jobs_bwd, PD));
    return launch_dyn_app_bwd(form == APP_FEAT ? "feat_dyn_app_bwd" : "dyn_app_bwd", form, a, w, gw, stream);
  }
  const RdrfStaticParams* PS = static_cast<const RdrfStaticParams*>(P);
  StaticW w;
  fill_static_w(w, PS);
  StaticG gw;
  memset(&gw, 0, sizeof(gw));
  RDRF_TRY(pack_image(a.pk, PS->packed_bwd, pk, stream, static_pack_jobs_bwd, PS, cfg->static_head));
  return launch_static_app_bwd(form == APP_FEAT ? "feat_static_app_bwd" : "static_app_bwd", cfg->static_head, form, a, w, gw, stream);
}

// ------------------------------------------------------------------------------------------------
// the ray scan backward alone on caller-owned arrays (rdrf_bwd_host.hpp; rdrf_selftest_ray_scan_bwd)
// ------------------------------------------------------------------------------------------------
int ray_scan_bwd_on_arrays(int width, const float* rays, const float* z, const uint8_t* valid, const float* raw, int N, int S,
                           int act, float density_shift, float distance_scale, int ray_type, const float* g_weight,
                           const float* g_sigma, const float* g_dists, float* out, float* g_z, float* g_rays, hipStream_t stream) {
  BwdArgs a;
  memset(&a, 0, sizeof(a));
  a.rays = rays; a.z = z; a.valid = valid; a.N = N; a.S = S;
  a.distance_scale = distance_scale; a.density_shift = density_shift; a.act = act; a.ray_type = ray_type;
  a.g_weight = g_weight; a.g_sigma = g_sigma; a.g_dists = g_dists; a.g_z = g_z; a.g_rays = g_rays;
  a.sp.raw = const_cast<float*>(raw);
  if (width == 32) {
    a.gsig = out;
    return launch_ray_scan_bwd(a, stream);
  }
  StaticW w;
  memset(&w, 0, sizeof(w));   // k_static_density_bwd reads no weight
  return launch_static_density_bwd(a, w, out, stream);
}
