// rdrf_mask_dev.hpp -- the packed occupancy grid of an alpha mask on the device and AlphaGridMask.sample_alpha on it
// (models/tensorBase.py:42-79), shared by the alpha-mask family (rdrf_alpha.hip) and the masked render
// (rdrf_render_masked.hip): both evaluate one and the same function.
#pragma once
#include "rdrf_host.hpp"

// ------------------------------------------------------------------------------------------------
// the packed occupancy grid on the device: bit f = ((iz G1 + iy) G0 + ix) T + k of the buffer, most significant bit of
// a byte first (np.packbits)
// ------------------------------------------------------------------------------------------------
struct MaskDev {
  const uint8_t* bits;   // nullptr: no mask
  int G0, G1, G2, T;
  float lo[3], inv[3];
};

static inline MaskDev make_mask(const RdrfAlphaMask* m) {
  MaskDev d;
  memset(&d, 0, sizeof(d));
  if (m == nullptr || m->bits == nullptr) return d;
  d.bits = m->bits;
  d.G0 = m->grid[0]; d.G1 = m->grid[1]; d.G2 = m->grid[2]; d.T = m->T;
  for (int i = 0; i < 3; ++i) {
    d.lo[i] = m->aabb[i];
    d.inv[i] = (1.0f / (m->aabb[3 + i] - m->aabb[i])) * 2.0f;   // AlphaGridMask.invgridSize (:49)
  }
  return d;
}
static inline bool mask_ok(const RdrfAlphaMask* m) {
  return m == nullptr || m->bits == nullptr || (m->grid[0] > 0 && m->grid[1] > 0 && m->grid[2] > 0 && m->T > 0);
}

RDRF_D int mask_slice(const MaskDev& m, float t) {   // round((t + 1) / 2 (T - 1)), half-way cases to even (torch.round)
#pragma clang fp contract(off)
  const float a = t + 1.0f;
  const float b = a / 2.0f;
  const float c = b * (float)(m.T - 1);
  const int k = (int)rintf(c);
  return k < 0 ? 0 : (k > m.T - 1 ? m.T - 1 : k);   // (one_hot raises beyond the slices; the nearest slice is taken)
}

RDRF_D float mask_bit(const MaskDev& m, int ix, int iy, int iz, int k) {
  if (ix < 0 || iy < 0 || iz < 0 || ix >= m.G0 || iy >= m.G1 || iz >= m.G2) return 0.0f;   // zero padding
  const size_t f = (((size_t)iz * m.G1 + iy) * m.G0 + ix) * m.T + k;
  return (float)((m.bits[f >> 3] >> (7 - (int)(f & 7))) & 1);
}

// F.grid_sample of the (1, T, G2, G1, G0) volume, trilinear, align_corners=True, zero padding, slice k: ATen's
// grid_sampler_3d expressions and corner order
RDRF_D float mask_sample(const MaskDev& m, float x, float y, float z, int k) {
#pragma clang fp contract(off)
  const float gx = norm_c(x, m.lo[0], m.inv[0]), gy = norm_c(y, m.lo[1], m.inv[1]), gz = norm_c(z, m.lo[2], m.inv[2]);
  const float fx = ((gx + 1.0f) / 2.0f) * (float)(m.G0 - 1);
  const float fy = ((gy + 1.0f) / 2.0f) * (float)(m.G1 - 1);
  const float fz = ((gz + 1.0f) / 2.0f) * (float)(m.G2 - 1);
  // (a coordinate far outside -- or NaN -- has no tap inside the volume)
  if (!(fx > -1.0f && fx < (float)m.G0 && fy > -1.0f && fy < (float)m.G1 && fz > -1.0f && fz < (float)m.G2)) return 0.0f;
  const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
  const int x0 = (int)x0f, y0 = (int)y0f, z0 = (int)z0f;
  const float wx1 = fx - x0f, wy1 = fy - y0f, wz1 = fz - z0f;
  const float wx0 = (x0f + 1.0f) - fx, wy0 = (y0f + 1.0f) - fy, wz0 = (z0f + 1.0f) - fz;
  float v = 0.0f;
  v += mask_bit(m, x0, y0, z0, k) * (wx0 * wy0 * wz0);
  v += mask_bit(m, x0 + 1, y0, z0, k) * (wx1 * wy0 * wz0);
  v += mask_bit(m, x0, y0 + 1, z0, k) * (wx0 * wy1 * wz0);
  v += mask_bit(m, x0 + 1, y0 + 1, z0, k) * (wx1 * wy1 * wz0);
  v += mask_bit(m, x0, y0, z0 + 1, k) * (wx0 * wy0 * wz1);
  v += mask_bit(m, x0 + 1, y0, z0 + 1, k) * (wx1 * wy0 * wz1);
  v += mask_bit(m, x0, y0 + 1, z0 + 1, k) * (wx0 * wy1 * wz1);
  v += mask_bit(m, x0 + 1, y0 + 1, z0 + 1, k) * (wx1 * wy1 * wz1);
  return v;
}
