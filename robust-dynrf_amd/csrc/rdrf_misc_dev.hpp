// rdrf_misc_dev.hpp -- device bodies of the sampler (renderer.sampleXYZ, /root/reference/renderer.py:147-170, models/
// tensorBase.py:487-559) and of the compositor (raw2outputs, renderer.py:173-315), shared by their own kernels in
// rdrf_misc.hip and by the single-launch fused render of rdrf_render.hip.
#pragma once
#include "rdrf_fwd_dev.hpp"

// ATen's CPU linspace (aten/src/ATen/native/cpu/RangeFactoriesKernel.cpp), fp32, as the shipped torch
// binaries compute it: step = (end - start) / (steps - 1); element i is start + step * i in the first
// half and end - step * (steps - i - 1) in the second, and GCC contracts each multiply-add into ONE
// fused operation (checked bit-for-bit against torch.linspace over many (start, end, steps),
// tests/test_oracle_golden.py::test_linspace_formula).  The `valid` byte mask depends on these bits.
RDRF_D float linspace_at(float start, float end, int steps, int i) {
#pragma clang fp contract(off)
  if (steps <= 1) return start;
  const float step = (end - start) / (float)(steps - 1);
  if (i < steps / 2) return __builtin_fmaf(step, (float)i, start);
  return __builtin_fmaf(-step, (float)(steps - i - 1), end);
}

// The point of a ray at depth t in field coordinates, as the ndc and the contract sampler place a sample: o + d t, and for
// contract scenes the L-inf contraction of it.  One copy for the two sampler bodies below and for the surface hits
// (k_render_hits, rdrf_hits.hip), whose point at a sample's own depth so has that sample's bits.
RDRF_D void ray_point(const float* __restrict__ r, float t, int contract, float (&p)[3]) {
#pragma clang fp contract(off)
  float nrm = 0.f;
  for (int k = 0; k < 3; ++k) {
    const float m = r[3 + k] * t;
    p[k] = r[k] + m;
    nrm = fmaxf(nrm, fabsf(p[k]));
  }
  if (contract && nrm > 1.0f) {
    const float sc = 2.0f - 1.0f / nrm;
    for (int k = 0; k < 3; ++k) p[k] = sc * (p[k] / nrm);
  }
}

RDRF_D void sample_ndc_body(const float* __restrict__ rays, int N, int S, float near, float far,
                            const float* __restrict__ jitter, Box box, float* __restrict__ xyz,
                            float* __restrict__ z, uint8_t* __restrict__ valid, const GridCtx gc) {
#pragma clang fp contract(off)
  for (long i = (long)gc.bid * gc.nthr + gc.tid; i < (long)N * S; i += (long)gc.nblk * gc.nthr) {
  const int n = (int)(i / S), j = (int)(i - (long)n * S);
  float t = linspace_at(near, far, S, j);
  if (jitter) {
    const float c = (float)(((double)far - (double)near) / (double)S);
    const float jj = jitter[j] * c;
    t = t + jj;
  }
  float p[3];
  ray_point(rays + (size_t)n * 6, t, 0, p);
  bool out = false;
  for (int k = 0; k < 3; ++k) {
    xyz[i * 3 + k] = p[k];
    out = out || (box.lo[k] > p[k]) || (p[k] > box.hi[k]);
  }
  z[i] = t;
  valid[i] = out ? 0 : 1;
  }
}

RDRF_D void sample_contract_body(const float* __restrict__ rays, int N, int S, float near,
                                 float far, const float* __restrict__ jin,
                                 const float* __restrict__ jout, float* __restrict__ xyz,
                                 float* __restrict__ z, uint8_t* __restrict__ valid, const GridCtx gc) {
#pragma clang fp contract(off)
  for (long i = (long)gc.bid * gc.nthr + gc.tid; i < (long)N * S; i += (long)gc.nblk * gc.nthr) {
  const int n = (int)(i / S), j = (int)(i - (long)n * S);
  const int inner = S - S / 2, outer = S / 2;
  float t;
  if (j < inner) {
    float a = linspace_at(near, 2.0f, inner + 1, j);
    float b = linspace_at(near, 2.0f, inner + 1, j + 1);
    if (jin) {
      const float c = (float)((2.0 - (double)near) / (double)inner);
      a = a + jin[j] * c;
      if (j + 1 < inner) b = b + jin[j + 1] * c;
    }
    t = (b + a) * 0.5f;
  } else {
    const int k = j - inner;  // flipped: rng'[k] = rng[outer-k]
    float r0 = (float)(outer - k), r1 = (float)(outer - k - 1);
    if (jout) {
      if (outer - k < outer) r0 = r0 + jout[outer - k];
      r1 = r1 + jout[outer - k - 1];
    }
    const float mid = (r1 + r0) * 0.5f;
    const float c2 = (float)(1.0 / 2.0 - 1.0 / (double)far);
    const float inv_far = (float)(1.0 / (double)far);
    const float den = inv_far + (c2 * mid) / (float)outer;
    t = 1.0f / den;
  }
  float p[3];
  ray_point(rays + (size_t)n * 6, t, 1, p);
  for (int k = 0; k < 3; ++k) xyz[i * 3 + k] = p[k];
  z[i] = t;
  valid[i] = 1;
  }
}

// World-space march (TensorBase.sample_ray, models/tensorBase.py:501-522: every ray_type but ndc / contract): the entry depth
// of the ray into the box, clamped to [near, far], then S samples a fixed `step` apart.  raw: the depth before the clamp;
// axis / upper: which slab bound gave it (the backward differentiates that one quotient).  fp32 in the reference's operation
// order, correctly rounded quotients.
RDRF_D float world_tmin(const float* __restrict__ r, const Box& box, float near, float far, float& raw, int& axis,
                        bool& upper) {
#pragma clang fp contract(off)
  raw = 0.f; axis = 0; upper = false;
  for (int k = 0; k < 3; ++k) {
    const float vec = r[3 + k] == 0.0f ? 1e-6f : r[3 + k];
    const float ra = __fdiv_rn(box.hi[k] - r[k], vec);
    const float rb = __fdiv_rn(box.lo[k] - r[k], vec);
    const bool up = ra < rb;
    const float m = up ? ra : rb;
    if (k == 0 || m > raw) { raw = m; axis = k; upper = up; }
  }
  return fminf(fmaxf(raw, near), far);
}

// jitter: one value per ray [N] (the reference's rand_like(rng[:, [0]])) or NULL
RDRF_D void sample_world_body(const float* __restrict__ rays, int N, int S, float near, float far, float step,
                              const float* __restrict__ jitter, Box box, float* __restrict__ xyz,
                              float* __restrict__ z, uint8_t* __restrict__ valid, const GridCtx gc) {
#pragma clang fp contract(off)
  for (long i = (long)gc.bid * gc.nthr + gc.tid; i < (long)N * S; i += (long)gc.nblk * gc.nthr) {
  const int n = (int)(i / S), j = (int)(i - (long)n * S);
  const float* r = rays + (size_t)n * 6;
  float raw; int axis; bool upper;
  const float t_min = world_tmin(r, box, near, far, raw, axis, upper);
  float rng = (float)j;
  if (jitter) rng = rng + jitter[n];
  const float off = step * rng;
  const float t = t_min + off;
  bool out = false;
  for (int k = 0; k < 3; ++k) {
    const float m = r[3 + k] * t;
    const float p = r[k] + m;
    xyz[i * 3 + k] = p;
    out = out || (box.lo[k] > p) || (p > box.hi[k]);
  }
  z[i] = t;
  valid[i] = out ? 0 : 1;
  }
}

// ------------------------------------------------------------------------------------------------
// the ray of camera c2w [3][4] through the pixel coordinates (i, j) (a pixel centre is column + 0.5, row + 0.5):
// get_ray_directions_blender, get_rays and, with `ndc`, ndc_rays_blender with `near` (dataLoader/ray_utils.py:93-110,
// :143-160, :197-218).  One copy for k_camera_rays (rdrf_eval.hip) and the slot rays of k_track_vis_rays
// (rdrf_track_vis.hip).  r: origin, direction.
// ------------------------------------------------------------------------------------------------
RDRF_D void camera_ray(const float* __restrict__ M, float focal, float i, float j, int H, int W, int ndc, float near,
                       float (&r)[6]) {
#pragma clang fp contract(off)
  // get_ray_directions_blender: centre (W / 2, H / 2), [focal, focal]
  const float cx = (float)((double)W / 2), cy = (float)((double)H / 2);
  const float dir[3] = {(i - cx) / focal, -(j - cy) / focal, -1.0f};
  // get_rays: rays_d = directions @ c2w[:3, :3].T, rays_o = c2w[:3, 3]
  float d[3], o[3];
  for (int q = 0; q < 3; ++q) {
    d[q] = dir[0] * M[q * 4 + 0] + dir[1] * M[q * 4 + 1] + dir[2] * M[q * 4 + 2];
    o[q] = M[q * 4 + 3];
  }
  if (ndc) {  // ndc_rays_blender
    const float t = -(near + o[2]) / d[2];
    o[0] = o[0] + t * d[0]; o[1] = o[1] + t * d[1]; o[2] = o[2] + t * d[2];
    const float kw = -1.0f / ((float)W / (2.0f * focal)), kh = -1.0f / ((float)H / (2.0f * focal));
    const float o0 = kw * o[0] / o[2];
    const float o1 = kh * o[1] / o[2];
    const float o2 = 1.0f + 2.0f * near / o[2];
    const float d0 = kw * (d[0] / d[2] - o[0] / o[2]);
    const float d1 = kh * (d[1] / d[2] - o[1] / o[2]);
    const float d2 = -2.0f * near / o[2];
    o[0] = o0; o[1] = o1; o[2] = o2; d[0] = d0; d[1] = d1; d[2] = d2;
  }
  r[0] = o[0]; r[1] = o[1]; r[2] = o[2]; r[3] = d[0]; r[4] = d[1]; r[5] = d[2];
}

// ------------------------------------------------------------------------------------------------
// compositor (raw2outputs)
// ------------------------------------------------------------------------------------------------
struct CompArgs {
  const float *rgb_s, *sigma_s, *rgb_d, *sigma_d, *dists, *blending, *z, *rays;
  int N, S, ray_type, add_white_bg;
  const float* white_dev;   // nullable: the coin as a device float (overrides add_white_bg; HIP-graph replays)
  float* out[13];
};

RDRF_D float alpha_of(float sigma, float dist) { return 1.0f - expf(-sigma * dist); }
RDRF_D float tfull_factor(float ad, float as, float b) {
#pragma clang fp contract(off)
  const float u = 1.0f - ad * b;
  const float v = 1.0f - as * (1.0f - b);
  return u * v + 1e-10f;
}

// ------------------------------------------------------------------------------------------------
// One round of 64 samples of the T_full scan with its running minimum, for the kernels that walk a ray's transmittance after
// the compositor (k_track_vis_scan, rdrf_track_vis.hip; k_render_hits, rdrf_hits.hip).  Sample s of the round sits in lane
// s - j0.  ray_sample: the sample's planes and its dists as the fields form them, (z_{s+1} - z_s) |d| distance_scale, 0 for
// the last; pf = F_s(dists_s).  tfull_min_round: with pf the lane's factor (1.0 where the caller wants none), Tf = T_s as
// composite_body forms T_full[s] (scan_mul64, carry cf), Tn = T_{s+1}, mn = m_s = min_{i <= s} T_i (a min scan of the same
// Hillis-Steele shape, carry mc); cf and mc move on to the next round.
// ------------------------------------------------------------------------------------------------
struct RaySample {
  float zs, zn, width, b, sg_d, sg_s, ds, pf;
};
RDRF_D RaySample ray_sample(const float* __restrict__ z, const float* __restrict__ sigma_s, const float* __restrict__ sigma_d,
                            const float* __restrict__ blending, int n, int S, int s, float nrm, float distance_scale) {
  RaySample q;
  const bool act = s < S;
  const size_t idx = (size_t)n * S + (act ? s : 0);
  q.zs = z[idx];
  q.zn = (act && s + 1 < S) ? z[idx + 1] : q.zs;
  q.width = (s + 1 < S) ? (q.zn - q.zs) : 0.0f;
  q.b = blending[idx]; q.sg_d = sigma_d[idx]; q.sg_s = sigma_s[idx];
  q.ds = q.width * nrm * distance_scale;
  q.pf = tfull_factor(alpha_of(q.sg_d, q.ds), alpha_of(q.sg_s, q.ds), q.b);
  return q;
}
RDRF_D void tfull_min_round(float pf, int lane, float& cf, float& mc, float& Tf, float& Tn, float& mn) {
  const float ifl = scan_mul64(pf, lane);
  float ef = __shfl_up(ifl, 1, 64);
  if (lane == 0) ef = 1.0f;
  Tf = cf * ef;
  Tn = cf * ifl;
  cf *= __shfl(ifl, 63, 64);
  mn = Tf;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float o = __shfl_up(mn, d, 64);
    if (lane >= d) mn = fminf(mn, o);
  }
  mn = fminf(mn, mc);
  mc = __shfl(mn, 63, 64);
}

RDRF_D void composite_body(const CompArgs a, const GridCtx gc) {
  const int lane = gc.tid & 63;
  const int wave_ = gc.tid >> 6, nwaves_ = gc.nthr >> 6;
  for (int n = gc.bid * nwaves_ + wave_; n < a.N; n += gc.nblk * nwaves_) {
  const int S = a.S;
  float cd = 1.f, cs = 1.f, cf = 1.f;  // scan carries
  float sum_wd = 0.f;
  float rs[3] = {0, 0, 0}, rf[3] = {0, 0, 0};
  float acc_s = 0.f, acc_f = 0.f, dep_s = 0.f, dep_f = 0.f, dyn = 0.f;
  float* w_full = a.out[3];
  float* w_s = a.out[7];
  float* w_d = a.out[11];
  for (int j0 = 0; j0 < S; j0 += 64) {
    const int j = j0 + lane;
    const bool act = j < S;
    const size_t idx = (size_t)n * S + (act ? j : 0);
    const float di = a.dists[idx], b = a.blending[idx], zz = a.z[idx];
    const float ad = act ? alpha_of(a.sigma_d[idx], di) : 0.f;
    const float as = act ? alpha_of(a.sigma_s[idx], di) : 0.f;
    const float pd = act ? one_minus_alpha_eps(ad) : 1.f;
    const float ps = act ? one_minus_alpha_eps(as) : 1.f;
    const float pf = act ? tfull_factor(ad, as, b) : 1.f;
    const float id = scan_mul64(pd, lane), is = scan_mul64(ps, lane), ifl = scan_mul64(pf, lane);
    float ed = __shfl_up(id, 1, 64), es = __shfl_up(is, 1, 64), ef = __shfl_up(ifl, 1, 64);
    if (lane == 0) { ed = 1.f; es = 1.f; ef = 1.f; }
    const float Td = cd * ed, Ts = cs * es, Tf = cf * ef;
    cd *= __shfl(id, 63, 64);
    cs *= __shfl(is, 63, 64);
    cf *= __shfl(ifl, 63, 64);
    if (act) {
      const float wd = ad * Td, ws = as * Ts;
      const float wf = (ad * b + as * (1.0f - b)) * Tf;
      const float fd = Tf * ad * b, fs = Tf * as * (1.0f - b);
      sum_wd += wd;
      w_d[idx] = wd;  // raw; normalised in pass 2
      w_s[idx] = ws;
      w_full[idx] = wf;
      for (int c = 0; c < 3; ++c) {
        const float cs_ = a.rgb_s[idx * 3 + c], cd_ = a.rgb_d[idx * 3 + c];
        rs[c] += ws * cs_;
        rf[c] += fd * cd_ + fs * cs_;
      }
      acc_s += ws; acc_f += wf;
      dep_s += ws * zz; dep_f += wf * zz;
      dyn += wf * b;
    }
  }
  sum_wd = wave_sum(sum_wd);
  const float denom = sum_wd + 1e-10f;
  float rd[3] = {0, 0, 0}, acc_d = 0.f, dep_d = 0.f;
  for (int j0 = 0; j0 < S; j0 += 64) {
    const int j = j0 + lane;
    if (j < S) {
      const size_t idx = (size_t)n * S + j;
      const float wd = w_d[idx] / denom;
      w_d[idx] = wd;
      for (int c = 0; c < 3; ++c) rd[c] += wd * a.rgb_d[idx * 3 + c];
      acc_d += wd;
      dep_d += wd * a.z[idx];
    }
  }
  for (int c = 0; c < 3; ++c) { rs[c] = wave_sum(rs[c]); rf[c] = wave_sum(rf[c]); rd[c] = wave_sum(rd[c]); }
  acc_s = wave_sum(acc_s); acc_f = wave_sum(acc_f); acc_d = wave_sum(acc_d);
  dep_s = wave_sum(dep_s); dep_f = wave_sum(dep_f); dep_d = wave_sum(dep_d);
  dyn = wave_sum(dyn);
  if (lane == 0) {
    const float rl = fmaxf(1.0f - acc_f, 0.0f);
    if (a.white_dev ? (a.white_dev[0] != 0.f) : (a.add_white_bg != 0)) {
      for (int c = 0; c < 3; ++c) { rd[c] += 1.0f - acc_d; rs[c] += 1.0f - acc_s; rf[c] += rl; }
    }
    if (a.ray_type == RDRF_RAY_NDC) {
      const float far = a.rays[(size_t)n * 6 + 2] + a.rays[(size_t)n * 6 + 5];
      dep_d += (1.0f - acc_d) * far; dep_s += (1.0f - acc_s) * far; dep_f += rl * far;
    } else if (a.ray_type == RDRF_RAY_CONTRACT) {
      dep_d += (1.0f - acc_d) * 256.0f; dep_s += (1.0f - acc_s) * 256.0f; dep_f += rl * 256.0f;
    }
    for (int c = 0; c < 3; ++c) {
      a.out[0][(size_t)n * 3 + c] = fminf(fmaxf(rf[c], 0.f), 1.f);
      a.out[4][(size_t)n * 3 + c] = fminf(fmaxf(rs[c], 0.f), 1.f);
      a.out[8][(size_t)n * 3 + c] = fminf(fmaxf(rd[c], 0.f), 1.f);
    }
    a.out[1][n] = dep_f; a.out[2][n] = acc_f;
    a.out[5][n] = dep_s; a.out[6][n] = acc_s;
    a.out[9][n] = dep_d; a.out[10][n] = acc_d;
    a.out[12][n] = dyn + rl * 0.0f;
  }
  }  // ray loop
}

// ------------------------------------------------------------------------------------------------
// per-ray tail of render_3d_point + induce_flow (renderer.py:1328-1392): far-point fill, NDC2world / contract2world,
// projection into the neighbour camera.  Shared by k_induce_flow / k_induce_flow_bwd (rdrf_misc.hip) and k_motion_maps
// (rdrf_motion.hip).
// ------------------------------------------------------------------------------------------------
struct FlowRay {
  float far[3], P[3], world[3], q[3], cam[3];
  float acc, c, pz;            // NDC: clamped P.z and 2/(c-1)
  float fn, fs; int fk;        // contract far point: norm, scale g(n), arg-max component (fk<0: inside)
  float wn, wsc; int wk;       // contract2world: norm, scale s(m), arg-max (wk<0: identity)
};
RDRF_D int argmax_abs3(const float (&v)[3], float& n) {
  int k = 0;
  n = fabsf(v[0]);
  if (fabsf(v[1]) > n) { n = fabsf(v[1]); k = 1; }
  if (fabsf(v[2]) > n) { n = fabsf(v[2]); k = 2; }
  return k;
}
// first half (renderer.py:1333-1345): P = ps + (1 - acc) far, the far point per ray type; also the seed of a point track
// (k_track_seeds, rdrf_track.hip)
RDRF_D void flow_ray_seed(FlowRay& r, const float* ray, float acc, const float (&ps)[3], int ray_type) {
#pragma clang fp contract(off)
  r.acc = acc;
  if (ray_type == RDRF_RAY_NDC) {
    for (int i = 0; i < 3; ++i) r.far[i] = ray[i] + ray[3 + i];
    r.fk = -1;
  } else {
    float f0[3];
    for (int i = 0; i < 3; ++i) f0[i] = ray[i] + ray[3 + i] * 256.0f;
    const int k = argmax_abs3(f0, r.fn);
    if (r.fn > 1.0f) {
      r.fk = k;
      r.fs = (2.0f - 1.0f / r.fn);
      for (int i = 0; i < 3; ++i) r.far[i] = r.fs * (f0[i] / r.fn);
    } else {
      r.fk = -1;
      for (int i = 0; i < 3; ++i) r.far[i] = f0[i];
    }
  }
  for (int i = 0; i < 3; ++i) r.P[i] = ps[i] + (1.0f - acc) * r.far[i];
}
RDRF_D void flow_ray_fwd(FlowRay& r, const float* ray, const float* c2w, float acc, const float (&ps)[3],
                         int H, int W, float f, int ray_type, float& u, float& v, float& disp) {
#pragma clang fp contract(off)
  flow_ray_seed(r, ray, acc, ps, ray_type);
  if (ray_type == RDRF_RAY_NDC) {
    r.c = fminf(fmaxf(r.P[2], -1.0f), 1.0f - 1e-6f);
    r.pz = 2.0f / (r.c - 1.0f);
    r.world[0] = -r.P[0] * r.pz * (float)W / 2.0f / f;
    r.world[1] = -r.P[1] * r.pz * (float)H / 2.0f / f;
    r.world[2] = r.pz;
    r.wk = -1;
  } else {
    const int k = argmax_abs3(r.P, r.wn);
    if (r.wn > 1.0f) {
      r.wk = k;
      r.wsc = -1.0f / (r.wn - 2.0f);
      for (int i = 0; i < 3; ++i) r.world[i] = r.P[i] / r.wn * r.wsc;
    } else {
      r.wk = -1;
      for (int i = 0; i < 3; ++i) r.world[i] = r.P[i];
    }
  }
  for (int j = 0; j < 3; ++j) r.q[j] = r.world[j] - c2w[j * 4 + 3];
  for (int i = 0; i < 3; ++i)   // cam_i = sum_j q_j R[j][i]  (w2c = R^T)
    r.cam[i] = r.q[0] * c2w[0 * 4 + i] + r.q[1] * c2w[1 * 4 + i] + r.q[2] * c2w[2 * 4 + i];
  u = r.cam[0] / (-r.cam[2]) * f + (float)W * 0.5f;
  v = -r.cam[1] / (-r.cam[2]) * f + (float)H * 0.5f;
  disp = 1.0f + 2.0f / r.cam[2];
}
