// rdrf_bwd_mlp_dev.hpp -- the per-sample and per-tile steps of the backward-DATA kernels (rdrf_bwd.hip, rdrf_bwd_fused.hip),
// each written once: the ray scan backward (scan_sample, tile_carries, suffix_g_alpha, dist_grads, scan_bwd_step), the
// positional-encoding backwards with their branch-free twins side by side, the heads' and the warp
// MLP's per-tile steps of the dynamic field's density phase, and the steps the two appearance kernels share.  The kernels
// keep their launch geometry, tile queues, loops, LDS, sums and stores; a kernel that must give the bits of a partner
// calls the partner's functions on the same values.  Every function is force-inlined: hipcc contracts a function's
// products after inlining, within the caller.
#pragma once
#include "rdrf_bwd_dev.hpp"

RDRF_D float act_grad(float f, int act, float shift) {
  return act == RDRF_ACT_RELU ? (f > 0.0f ? 1.0f : 0.0f) : sigmoidf_(f + shift);
}

// the ReLU gate of one backward layer: dz = W^T dz_next where the saved activation is positive
template <int KK>
RDRF_D void relu_gate(float (&dz)[KK], const float (&H)[KK], const f32x16 (&acc)[KK / 16]) {
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) dz[kk] = H[kk] > 0.f ? acc[kk >> 4][kk & 15] : 0.f;
}

// a 32-float weight row of an LDS image as eight 16-byte reads up front (element-wise reads were 32 x {ds_read_b32, lgkmcnt(0)})
RDRF_D void lds_row32(float (&r)[32], const float* __restrict__ row) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
    r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
  }
}

// ------------------------------------------------------------------------------------------------
// positional-encoding backwards; each branchy function is followed by its branch-free twin (one basic block: head of
// rdrf_bwd_fused.hip), which must give its bits
// ------------------------------------------------------------------------------------------------
// d(X0)/d(xn): X0 = [xn, t | (sin q, cos q) pairs], q_j = xn[j/10] * 2^(j%10); returns this lane
// half's partial (combine with __shfl_xor 32)
// (no contraction in here: left to hipcc, which products of `a cv - b sv` fuse depends on the kernel around the call, and
// the fused warp kernel, through x0_bwd_flat, has to give the bits of k_dyn_density_bwd<1>)
RDRF_D void x0_bwd(const float (&X0)[32], const float (&dX0)[32], int h, float& d0, float& d1,
                   float& d2) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    if (o == 0 && h == 0) {
      d0 += dX0[0]; d1 += dX0[1]; d2 += dX0[2];
    } else {
      const int k = 2 * o + h - 1;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int j = 2 * k + p;
        const int d = j / 10, f = j - d * 10;
        const float sv = X0[o * 4 + 2 * p], cv = X0[o * 4 + 2 * p + 1];
        const float dq = ldexpf(dX0[o * 4 + 2 * p] * cv - dX0[o * 4 + 2 * p + 1] * sv, f);
        // (selects: d differs between the lane halves, and a branchy update makes d0..2 a scratch array indexed per lane)
        d0 += d == 0 ? dq : 0.f; d1 += d == 1 ? dq : 0.f; d2 += d == 2 ? dq : 0.f;
      }
    }
  }
}
// x0_bwd without the branch on the lane half, as sf_x_bwd_flat (no contraction: see x0_bwd)
RDRF_D void x0_bwd_flat(const float (&X0)[32], const float (&dX0)[32], int h, float& d0, float& d1, float& d2) {
#pragma clang fp contract(off)
  d0 += h == 0 ? dX0[0] : 0.f; d1 += h == 0 ? dX0[1] : 0.f; d2 += h == 0 ? dX0[2] : 0.f;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const int k = 2 * o + h - 1;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int j = 2 * k + p;
      const int d = j >= 0 ? j / 10 : -1, f = j >= 0 ? j - d * 10 : 0;
      const float sv = X0[o * 4 + 2 * p], cv = X0[o * 4 + 2 * p + 1];
      const float dq = ldexpf(dX0[o * 4 + 2 * p] * cv - dX0[o * 4 + 2 * p + 1] * sv, f);
      d0 += d == 0 ? dq : 0.f; d1 += d == 1 ? dq : 0.f; d2 += d == 2 ? dq : 0.f;
    }
  }
}

// the scene-flow MLP's input: X = [x | (sin, cos) pairs of 4 frequencies per axis]
RDRF_D void sf_x_bwd(const float (&X)[20], const float (&dX)[20], int h, float& d0, float& d1,
                     float& d2) {
#pragma unroll
  for (int o = 0; o < 5; ++o) {
    if (o == 0 && h == 0) {
      d0 += dX[0]; d1 += dX[1]; d2 += dX[2];
    } else {
      const int k = 2 * o + h - 1;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int pr = 2 * k + p;
        if (pr < 12) {
          const int d = pr >> 2, f = pr & 3;
          const float dq = ldexpf(dX[o * 4 + 2 * p] * X[o * 4 + 2 * p + 1] -
                                  dX[o * 4 + 2 * p + 1] * X[o * 4 + 2 * p], f);
          d0 += d == 0 ? dq : 0.f; d1 += d == 1 ? dq : 0.f; d2 += d == 2 ? dq : 0.f;   // selects, see x0_bwd
        }
      }
    }
  }
}
// sf_x_bwd without a branch: every lane runs the pair path of every octet -- where sf_x_bwd skips it (h == 0 in octet 0:
// pair -2 / -1; pairs 12 ..) nothing is selected and 0.f is added -- and the lanes h == 0 add dX[0..2] first, as there.
// The same values in the same order, plus additions of 0.f.
RDRF_D void sf_x_bwd_flat(const float (&X)[20], const float (&dX)[20], int h, float& d0, float& d1, float& d2) {
  d0 += h == 0 ? dX[0] : 0.f; d1 += h == 0 ? dX[1] : 0.f; d2 += h == 0 ? dX[2] : 0.f;
#pragma unroll
  for (int o = 0; o < 5; ++o) {
    const int k = 2 * o + h - 1;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int pr = 2 * k + p;
      const int d = (pr >= 0 && pr < 12) ? pr >> 2 : -1, f = pr & 3;
      const float dq = ldexpf(dX[o * 4 + 2 * p] * X[o * 4 + 2 * p + 1] - dX[o * 4 + 2 * p + 1] * X[o * 4 + 2 * p], f);
      d0 += d == 0 ? dq : 0.f; d1 += d == 1 ? dq : 0.f; d2 += d == 2 ? dq : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// d(weight)/d(alpha) along a ray.  weight_k = alpha_k T_k, T_k = prod_{j<k} p_j, p = 1-alpha+1e-10
//   dL/dalpha_k = gw_k T_k - (sum_{m>k} gw_m w_m) / p_k
// W consecutive samples of a ray sit in the lanes l = 0 .. W - 1 of a W-lane group (W = 32: the dynamic field, a wave or a
// half-wave per ray; W = 64: the static field, a wave per ray, whose kernel holds these lines in place -- see
// k_static_density_bwd).  The suffix sum is formed directly by walking the ray LAST
// tile first (the transmittance at each tile start comes from a forward pre-pass, tile_carries); total - prefix would cancel
// catastrophically when p -> 1e-10.  A 32-wide and a 64-wide scan sum in different orders: a field scans at its own width.
// ------------------------------------------------------------------------------------------------
struct ScanSample {
  float sigma, dz, ds, alpha, p;   // dz = z[j + 1] - z[j] (0 behind the last sample), ds = dz |d| scale
};
// sample j of a ray at idx; raw: the density head's raw output there
RDRF_D ScanSample scan_sample(const BwdArgs& a, float raw, bool act, bool vld, int idx, int j, float nrm) {
  ScanSample q;
  q.sigma = vld ? density_act(raw, a.act, a.density_shift) : 0.f;
  const float zj = act ? a.z[idx] : 0.f;
  const float zn = (j + 1 < a.S) ? a.z[idx + 1] : zj;
  q.dz = (j + 1 < a.S) ? (zn - zj) : 0.0f;
  q.ds = q.dz * nrm * a.distance_scale;
  q.alpha = 1.0f - expf(-q.sigma * q.ds);
  q.p = act ? one_minus_alpha_eps(q.alpha) : 1.0f;
  return q;
}
template <int W>
RDRF_D float scan_mul(float p, int l) {
  return W == 64 ? scan_mul64(p, l) : scan_mul32(p, l);
}
// pre-pass: the transmittance at each tile start of ray n -> carr[tile] (written by the lanes with `wr`); raw_stride: floats
// per sample of a.sp.raw; on: the group's ray exists
template <int W>
RDRF_D void tile_carries(const BwdArgs& a, float* carr, int raw_stride, int n, bool on, bool wr, int l, float nrm) {
  float carry = 1.0f;
  for (int j0 = 0; j0 < a.S; j0 += W) {
    if (wr) carr[j0 >> (W == 64 ? 6 : 5)] = carry;
    const int j = j0 + l;
    const bool act = on && j < a.S;
    const int idx = n * a.S + (act ? j : 0);
    const bool vld = act && a.valid[idx] != 0;
    const ScanSample q = scan_sample(a, a.sp.raw[(size_t)idx * raw_stride], act, vld, idx, j, nrm);
    carry *= __shfl(scan_mul<W>(q.p, l), W - 1, W);
  }
}
// one tile of the reverse sweep: d(weight) gwv -> d(alpha); T_start: the transmittance at the tile's start, sufcarry: the
// sum of gw_m w_m over the tiles behind this one
template <int W>
RDRF_D float suffix_g_alpha(float p, float alpha, float gwv, float T_start, int l, float& sufcarry) {
  const float incl = scan_mul<W>(p, l);
  float excl = __shfl_up(incl, 1, W);
  if (l == 0) excl = 1.0f;
  const float T = T_start * excl;
  float rinc = gwv * alpha * T;
#pragma unroll
  for (int d = 1; d < W; d <<= 1) {
    const float o = __shfl_down(rinc, d, W);
    if (l + d < W) rinc += o;
  }
  float rex = __shfl_down(rinc, 1, W);
  if (l == W - 1) rex = 0.f;
  const float g_alpha = gwv * T - (sufcarry + rex) / p;
  sufcarry += __shfl(rinc, 0, W);
  return g_alpha;
}
// dists = dz * |d| * scale: d(loss)/d|d| (summed into g_nrm) and d(loss)/dz (g_z), in the lanes with `on`
RDRF_D void dist_grads(const BwdArgs& a, const ScanSample& q, int idx, int j, float nrm, float g_alpha, bool on, float& g_nrm) {
  if ((a.g_rays || a.g_z) && on) {
    const float g_ds = (a.g_dists ? a.g_dists[idx] : 0.f) + g_alpha * q.sigma * (1.0f - q.alpha);
    if (a.g_rays) g_nrm += g_ds * q.dz * a.distance_scale;
    if (a.g_z && j + 1 < a.S) {
      const float gz = g_ds * nrm * a.distance_scale;
      atomicAdd(a.g_z + idx, -gz);
      atomicAdd(a.g_z + idx + 1, gz);
    }
  }
}
// one sample of the reverse sweep: returns the total d(sigma) = the caller's g_sigma + g_alpha ds (1 - alpha); T_start points
// at the tile's carry (read only under g_weight); on_dist: dist_grads' lane predicate (act, in one lane per sample)
template <int W>
RDRF_D float scan_bwd_step(const BwdArgs& a, float raw, const float* T_start, bool act, bool vld, bool on_dist, int idx, int j,
                           int l, float nrm, float& sufcarry, float& g_nrm) {
  const ScanSample q = scan_sample(a, raw, act, vld, idx, j, nrm);
  float g_alpha = 0.f;
  if (a.g_weight) g_alpha = suffix_g_alpha<W>(q.p, q.alpha, act ? a.g_weight[idx] : 0.f, *T_start, l, sufcarry);
  float g_sigma = (act && a.g_sigma) ? a.g_sigma[idx] : 0.f;
  g_sigma += g_alpha * q.ds * (1.0f - q.alpha);
  dist_grads(a, q, idx, j, nrm, g_alpha, on_dist, g_nrm);
  return g_sigma;
}

// ------------------------------------------------------------------------------------------------
// dynamic field, density phase: the heads' tile (phase 0 of k_dyn_density_bwd)
// ------------------------------------------------------------------------------------------------
// gradients of the raw head outputs from the total d(sigma) and the caller's d(blending)
RDRF_D void head_out_grads(const BwdArgs& a, int idx, bool vld, float g_sigma, float& g_fd, float& g_fb) {
  const float fd = a.sp.raw[(size_t)idx * 2], fb = a.sp.raw[(size_t)idx * 2 + 1];
  g_fd = vld ? g_sigma * act_grad(fd, a.act, a.density_shift) : 0.f;
  const float bl = sigmoidf_(fb);
  g_fb = (vld && a.g_blending) ? a.g_blending[idx] * bl * (1.0f - bl) : 0.f;
}

// weight/sigma/blending backward, density + blending head backward -> d(feature) rows (or records) for the scatter, d(X0)
// partial rows, dz rows; sw / sb: the wave's layer2 weight / bias sums of the two heads.  T_start, sufcarry, g_nrm: the
// wave-per-ray scan (scan_bwd_step<32>), not used in feature mode or on flat tiles
template <bool FEAT, bool FLAT>
RDRF_D void dyn_heads_bwd_tile(const BwdArgs& a, const float* lds, const float* svb, float* gb, bool act, bool vld, int idx, int j,
                               int s, int h, int lane, float nrm, const float* T_start, float& sufcarry, float& g_nrm,
                               float (&sw)[3], float (&sb)[3]) {
  float g_fd, g_fb;
  if constexpr (FEAT) {  // the gradients of the raw head outputs arrive directly
    g_fd = (act && a.g_sigma) ? a.g_sigma[idx] : 0.f;
    g_fb = (act && a.g_blending) ? a.g_blending[idx] : 0.f;
  } else if constexpr (FLAT) {   // the scan half ran in k_ray_scan_bwd
    head_out_grads(a, idx, vld, act ? a.gsig[idx] : 0.f, g_fd, g_fb);
  } else {
    const float g_sigma = scan_bwd_step<32>(a, a.sp.raw[(size_t)idx * 2], T_start, act, vld, act && h == 0, idx, j, s, nrm, sufcarry, g_nrm);
    head_out_grads(a, idx, vld, g_sigma, g_fd, g_fb);
  }
  f32x16 accX[2];  // d(X0) of the density and blending heads
  acc_zero<2>(accX);
  // head liveness (wave-uniform): a head whose output no loss reaches is not differentiated -- the reference's
  // autograd never visits that subgraph either (passes B-D of the trainer: no term depends on the blending head
  // before the late mask terms) -- so its 160 MFMAs per tile, its dz / d(feature) rows, its scatter set and its
  // dW products (host side) all drop out
  const bool live_d = FEAT ? a.g_sigma != nullptr : (a.g_sigma != nullptr || a.g_weight != nullptr);
  const bool live_b = a.g_blending != nullptr;
#pragma unroll
  for (int head = 0; head < 2; ++head) {
    if (!(head == 0 ? live_d : live_b)) continue;
    const float gfh = head == 0 ? g_fd : g_fb;
    float Hh[32], dzh[32];
    load_rows<32>(svb, head == 0 ? sv::K1_HD : sv::K1_HB, Hh, s, h);
    float w2r[32];
    lds_row32(w2r, lds + (head == 0 ? pkb::K1H_DEN2 : pkb::K1H_BLE2) + h * 32);
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) dzh[kk] = Hh[kk] > 0.f ? w2r[kk] * gfh : 0.f;
    save_rows<32>(gb, head == 0 ? sv::K1G_DZD : sv::K1G_DZB, dzh, s, h);
    if (!FEAT && a.small_dw) {   // d(layer2 weight) = sum over the samples of g * (layer2 input = the saved activation)
      float pw[32];
#pragma unroll
      for (int kk = 0; kk < 32; ++kk) pw[kk] = gfh * Hh[kk];
      sw[head] += reduce_scatter32(pw, s);
      sb[head] += gfh;
    }
    f32x16 accF[3];
    acc_zero<3>(accF);
#ifdef RDRF_HEADS_BWD_F32
    mfma_seg<3, 32>(accF, dzh, lds + (head == 0 ? pkb::K1H_DEN1T_F : pkb::K1H_BLE1T_F), lane);
    mfma_seg<2, 32>(accX, dzh, lds + (head == 0 ? pkb::K1H_DEN1T_X0 : pkb::K1H_BLE1T_X0), lane);
#else
    mfma_seg_b3_pair<3, 2, 32>(accF, accX, dzh, lds + (head == 0 ? pkb::K1H_DEN1T_F : pkb::K1H_BLE1T_F),
                               lds + (head == 0 ? pkb::K1H_DEN1T_X0 : pkb::K1H_BLE1T_X0), lane);
#endif
    float dFh[48];
    acc_copy<3>(dFh, accF);
    if (!FEAT && a.dfs != nullptr) {
      // sample-major record for the sorted scatter: this lane half holds the feature quads Q = 2 m + h
      // (slots 4m..4m+3), Q = 6 level + {0..3: XY quad, 4: XZ, 5: YZ}; one 16-byte store per quad
      if (act) {
        float* rec = a.dfs + (size_t)idx * DFS_FLOATS + head * 72;
#pragma unroll
        for (int m = 0; m < 9; ++m) {
          const int off = h ? dfs_off(2 * m + 1) : dfs_off(2 * m);
          *reinterpret_cast<f32x4*>(rec + off) = f32x4{dFh[4 * m], dFh[4 * m + 1], dFh[4 * m + 2], dFh[4 * m + 3]};
        }
      }
    } else {
      save_rows<48>(gb, head == 0 ? sv::K1G_DFD : sv::K1G_DFB, dFh, s, h);
    }
  }
  float dXh[32];
  acc_copy<2>(dXh, accX);
  save_rows<32>(gb, sv::K1G_DX0, dXh, s, h);
  if (h == 0) {
    gb[(size_t)(sv::K1G_SM + 3) * 32 + s] = g_fd;
    gb[(size_t)(sv::K1G_SM + 4) * 32 + s] = g_fb;
  }
}

// ------------------------------------------------------------------------------------------------
// dynamic field, density phase: the warp MLP's tile (phase 1 of k_dyn_density_bwd; k_dyn_warp_bwd_dw runs the same steps)
// ------------------------------------------------------------------------------------------------
// coordinate gradients arriving at the warp: appearance phase + density/blending scatter (already summed);
// xw = normalize(unnormalize(xn) + delta), xyz_prime = xyz + delta.  dd = d(delta): the dz of layer5, stored as the small-layer
// dz rows 0..2 (rows 3, 4 were written by the heads)
struct WarpIn {
  float dw0, dw1, dw2, dn0, dn1, dn2, dd0, dd1, dd2, gp0, gp1, gp2;
};
RDRF_D WarpIn warp_coord_grads(const BwdArgs& a, float* gb, bool act, int idx, int s, int h) {
  WarpIn g;
  g.dw0 = act ? a.dxw_app[(size_t)idx * 3 + 0] : 0.f; g.dw1 = act ? a.dxw_app[(size_t)idx * 3 + 1] : 0.f;
  g.dw2 = act ? a.dxw_app[(size_t)idx * 3 + 2] : 0.f;
  g.dn0 = act ? a.dxn_app[(size_t)idx * 3 + 0] : 0.f; g.dn1 = act ? a.dxn_app[(size_t)idx * 3 + 1] : 0.f;
  g.dn2 = act ? a.dxn_app[(size_t)idx * 3 + 2] : 0.f;
  g.dd0 = g.dw0 * a.box.inv[0]; g.dd1 = g.dw1 * a.box.inv[1]; g.dd2 = g.dw2 * a.box.inv[2];
  g.gp0 = 0.f; g.gp1 = 0.f; g.gp2 = 0.f;
  if (act && a.g_xyz_prime) {
    g.gp0 = a.g_xyz_prime[(size_t)idx * 3 + 0]; g.gp1 = a.g_xyz_prime[(size_t)idx * 3 + 1];
    g.gp2 = a.g_xyz_prime[(size_t)idx * 3 + 2];
  }
  g.dd0 += g.gp0; g.dd1 += g.gp1; g.dd2 += g.gp2;
  if (!act) { g.dd0 = g.dd1 = g.dd2 = 0.f; }
  if (h == 0) {
    gb[(size_t)(sv::K1G_SM + 0) * 32 + s] = g.dd0; gb[(size_t)(sv::K1G_SM + 1) * 32 + s] = g.dd1;
    gb[(size_t)(sv::K1G_SM + 2) * 32 + s] = g.dd2;
  }
  return g;
}
// layer5 on the VALU: dz4 = relu'(H4) W5^T dd; small: also d(layer5 weight), three output rows against the 64 saved inputs
// (sw: lane (s, h) holds input element elem_of(s, h) of the three rows; sb: the rows' bias sums per lane)
RDRF_D void warp_layer5_bwd(float (&dz4)[32], const float* lds, const float* svb, const WarpIn& g, bool small, int s, int h,
                            float (&sw)[3], float (&sb)[3]) {
  float H4[32];
  load_rows<32>(svb, sv::K1_H4, H4, s, h);
  const float* w5 = lds + pkb::K1W_W5 + h * 32;
  float wa[32], wb[32], wc[32];
  lds_row32(wa, w5);
  lds_row32(wb, w5 + 64);
  lds_row32(wc, w5 + 128);
#pragma unroll
  for (int kk = 0; kk < 32; ++kk) {
    const float d = wa[kk] * g.dd0 + wb[kk] * g.dd1 + wc[kk] * g.dd2;
    dz4[kk] = H4[kk] > 0.f ? d : 0.f;
  }
  if (small) {
    sb[0] += g.dd0; sb[1] += g.dd1; sb[2] += g.dd2;
#pragma unroll 1
    for (int o = 0; o < 3; ++o) {   // one row at a time: the three butterflies unrolled together spill
      const float dd = o == 0 ? g.dd0 : (o == 1 ? g.dd1 : g.dd2);
      float pw[32];
#pragma unroll
      for (int kk = 0; kk < 32; ++kk) pw[kk] = dd * H4[kk];
      const float r = reduce_scatter32(pw, s);
      sw[0] += o == 0 ? r : 0.f; sw[1] += o == 1 ? r : 0.f; sw[2] += o == 2 ? r : 0.f;
    }
  }
}
// layer4 backward: the data product of dz4 (the caller gates it with H3: relu_gate)
RDRF_D void warp_layer4_bwd(f32x16 (&acc)[2], const float (&dz4)[32], const float* lds, int lane) {
  acc_zero<2>(acc);
#ifdef RDRF_HEADS_BWD_F32
  mfma_seg<2, 32>(acc, dz4, lds + pkb::K1W_W4T, lane);
#else
  mfma_seg_b3<2, 32>(acc, dz4, lds + pkb::K1W_W4T, lane);
#endif
}
// layer3 backward: accX (the caller has set it to the heads' d(X0), from their K1G_DX0 rows) += d(X0) of the warp, accT = d(tout)
// of the sample.  The callers load those rows themselves: with the load in here, or in a function of its own, the bf16 MFMAs of
// k_dyn_density_bwd<1> see a VALU write of an operand 0 instructions behind them instead of 3 (RAW distance 11 instead of 14).
RDRF_D void warp_layer3_bwd(f32x16 (&accX)[2], f32x16 (&accT)[1], const float (&dz3)[32], const float* lds, int lane) {
  acc_zero<1>(accT);
#ifdef RDRF_HEADS_BWD_F32
  mfma_seg<2, 32>(accX, dz3, lds + pkb::K1W_W3T_X0, lane);
  mfma_seg<1, 32>(accT, dz3, lds + pkb::K1W_W3T_T, lane);
#else
  mfma_seg_b3_pair<2, 1, 32>(accX, accT, dz3, lds + pkb::K1W_W3T_X0, lds + pkb::K1W_W3T_T, lane);
#endif
}
// positional encoding backward -> d(xn), plus the identity path xw <- xn, into g.dn; FLATPE: the branch-free encoder
template <bool FLATPE>
RDRF_D void warp_x0_bwd(WarpIn& g, const f32x16 (&accX)[2], const float* svb, int s, int h) {
  float X0[32], dX0[32];
  load_rows<32>(svb, sv::K1_X0, X0, s, h);
  acc_copy<2>(dX0, accX);
  float e0 = 0.f, e1 = 0.f, e2 = 0.f;
  if constexpr (FLATPE) x0_bwd_flat(X0, dX0, h, e0, e1, e2);
  else x0_bwd(X0, dX0, h, e0, e1, e2);
  e0 += __shfl_xor(e0, 32, 64); e1 += __shfl_xor(e1, 32, 64); e2 += __shfl_xor(e2, 32, 64);
  g.dn0 += e0 + g.dw0; g.dn1 += e1 + g.dw1; g.dn2 += e2 + g.dw2;
}
// d(tout) of a flat tile's rays: segmented suffix sums over the lanes of each half (keys: the lane's ray, contiguous); the
// first lane of a segment (head) ends up with the segment's sum, which belongs in dtout if the ray lies inside the tile and
// else in one of the tile's two partial records (first / last ray) that k_time_branch_bwd sums in a fixed order
struct DtoutSeg {
  int nl, rb, re, end;   // the lane's ray; its first / last sample relative to the tile; the last lane of its segment
  bool head, inside;
};
RDRF_D DtoutSeg dtout_segments(const BwdArgs& a, int n, int s) {
  DtoutSeg g;
  const int i0 = n * 32 + s;
  g.nl = i0 / a.S;
  g.rb = g.nl * a.S - n * 32; g.re = g.rb + a.S - 1;
  g.end = g.re < 31 ? g.re : 31;
  g.head = i0 < a.N * a.S && (s == 0 || g.rb == s);
  g.inside = g.rb >= 0 && g.re <= 31;
  return g;
}

// The warp tile of k_dyn_density_bwd<1>: coordinate gradients -> warp MLP backward, positional-encoding backward, g_xyz;
// d(tout) of the sample is added to dTacc (the kernel reduces it per ray)
template <bool FEAT>
RDRF_D void dyn_warp_bwd_tile(const BwdArgs& a, const float* lds, const float* svb, float* gb, bool act, int idx, int s, int h,
                              int lane, float (&dTacc)[16], float (&sw)[3], float (&sb)[3]) {
  WarpIn g = warp_coord_grads(a, gb, act, idx, s, h);
  // ---- warp MLP backward: layer5 (VALU) -> layer4 -> layer3
  float dz4[32];
  warp_layer5_bwd(dz4, lds, svb, g, !FEAT && a.small_dw, s, h, sw, sb);
  save_rows<32>(gb, sv::K1G_DZ4, dz4, s, h);
  float dz3[32];
  {
    f32x16 acc[2];
    warp_layer4_bwd(acc, dz4, lds, lane);
    float H3[32];
    load_rows<32>(svb, sv::K1_H3, H3, s, h);
    relu_gate<32>(dz3, H3, acc);
  }
  save_rows<32>(gb, sv::K1G_DZ3, dz3, s, h);
  f32x16 accX[2], accT[1];  // d(X0): heads (from rows) + warp layer 3
  {
    float dXh[32];
    load_rows<32>(gb, sv::K1G_DX0, dXh, s, h);
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) accX[kk >> 4][kk & 15] = dXh[kk];
  }
  warp_layer3_bwd(accX, accT, dz3, lds, lane);
#pragma unroll
  for (int i = 0; i < 16; ++i) dTacc[i] += accT[0][i];
  warp_x0_bwd<false>(g, accX, svb, s, h);
  if (act && h == 0 && a.g_xyz) {
    if (FEAT && a.in_norm) {   // compute_*: gradient wrt the NORMALISED input coordinates
      a.g_xyz[(size_t)idx * 3 + 0] += g.dn0; a.g_xyz[(size_t)idx * 3 + 1] += g.dn1;
      a.g_xyz[(size_t)idx * 3 + 2] += g.dn2;
    } else {
      a.g_xyz[(size_t)idx * 3 + 0] += g.dn0 * a.box.inv[0] + g.gp0;
      a.g_xyz[(size_t)idx * 3 + 1] += g.dn1 * a.box.inv[1] + g.gp1;
      a.g_xyz[(size_t)idx * 3 + 2] += g.dn2 * a.box.inv[2] + g.gp2;
    }
  }
  if constexpr (FEAT) {  // time is per point: d(tout) of this sample, no reduction over the tile
    if (act) {
#pragma unroll
      for (int i = 0; i < 16; ++i) a.dtout[(size_t)idx * 32 + elem_of(i, h)] = dTacc[i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dTacc[i] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// appearance phase (dynamic: MLP_Fea_late_view; static: MLP_Fea | TimeEmbedding): the steps the two kernels share
// ------------------------------------------------------------------------------------------------
// FEAT: the features ARE the basis output: d(features) arrive in g_feat, only the basis backward runs
template <bool FEAT>
RDRF_D void feat_dF(float (&dF)[16], const float* g_feat, int idx, bool act, int h) {
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int e = elem_of(kk, h);
    dF[kk] = (act && e < 27) ? g_feat[(size_t)idx * 27 + e] : 0.f;
  }
}

// one backward-data layer of the appearance phases: NBI input blocks from one dz vector, fp32 pipe (A/B builds) or split-storage
// bf16 x 3 (the lo pieces of step 0 are requested here: callers place the call so that row loads / VALU work follow the request)
template <int NBI, int KK>
RDRF_D void app_bwd_seg(f32x16 (&acc)[NBI], const float (&dz)[KK], const float* __restrict__ whm, const float* __restrict__ pk,
                        int lo_reg, int lo_off, int lane) {
#ifdef RDRF_APP_F32
  mfma_seg<NBI, KK>(acc, dz, whm, lane);
#else
  const B3sLo st = b3s_lo_stream(pk + lo_reg, lane);
  u32x4 lo[NBI];
  b3s_lo_load<NBI>(lo, st, lo_off, KK / 8, 0);
  mfma_seg_b3s<NBI, KK, 0>(acc, dz, whm, st, lo_off, 0, lo, lane);
#endif
}

// a tile's lane: compacted sample li of the app-mask list (feature mode: point li), its flat sample idx and ray n
struct AppTile {
  int li, idx, n;
  bool act;
};
template <bool FEAT>
RDRF_D AppTile app_tile(const BwdArgs& a, int tile, int s, int count) {
  AppTile t;
  t.li = tile * 32 + s;
  t.act = t.li < count;
  t.idx = t.act ? (FEAT ? t.li : a.sp.list[t.li]) : 0;
  t.n = t.idx / a.S;
  return t;
}
// basis backward: d(app features) of the NB blocks of the VM gather from dF
template <int NB>
RDRF_D void app_basis_bwd(float (&dA)[16 * NB], const float (&dF)[16], const float* basisT, const float* pk, int lo_reg, int lo_off,
                          int lane) {
  f32x16 acc[NB];
  acc_zero<NB>(acc);
  app_bwd_seg<NB, 16>(acc, dF, basisT, pk, lo_reg, lo_off, lane);
  acc_copy<NB>(dA, acc);
}
// the features-only tile
template <int NB>
RDRF_D void app_feat_only(const BwdArgs& a, float* gb, const AppTile& t, const float* basisT, int lo_reg, int lo_off, int s, int h,
                          int lane) {
  float dF[16];
  feat_dF<true>(dF, a.g_feat, t.idx, t.act, h);
  save_rows<16>(gb, sv::K3G_DF, dF, s, h);
  float dA[16 * NB];
  app_basis_bwd<NB>(dA, dF, basisT, a.pk, lo_reg, lo_off, lane);
  save_rows<16 * NB>(gb, sv::K3G_DA, dA, s, h);
}
// layer 2 backward: dH1 = W2^T dz2, gated by the saved H1 -> dz1 (also written as rows)
RDRF_D void app_l2_bwd(float (&dz1)[64], const float (&dz2)[64], const BwdArgs& a, const float* svb, float* gb, int row_h1,
                       const float* w2t, int lo_reg, int lo_off, int s, int h, int lane) {
  f32x16 acc[4];
  acc_zero<4>(acc);
  app_bwd_seg<4, 64>(acc, dz2, w2t, a.pk, lo_reg, lo_off, lane);
  float H1[64];
  load_rows<64>(svb, row_h1, H1, s, h);
  relu_gate<64>(dz1, H1, acc);
  save_rows<64>(gb, sv::K3G_DZ1, dz1, s, h);
}
