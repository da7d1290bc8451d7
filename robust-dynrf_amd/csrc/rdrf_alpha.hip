// rdrf_alpha.hip -- the alpha-mask family of TensorBase (the reference's models/tensorBase.py): a field evaluated off
// the rays, on a lattice, and the occupancy grid made from it.
//
//   k_alpha_dyn / k_alpha_static : compute_alpha (:684-702) for M points x T times.  sigma is the density phase of the
//                  field's forward on the same point and time -- the per-sample functions dyn_density_body /
//                  static_density_body call (rdrf_fwd_dev.hpp: load_tout, warp_mlp, warp_point, head_raw<false>;
//                  static_density_feature) on the same packed image, an MFMA column depending on its own sample
//                  only -- then alpha = 1 - exp(-sigma length).  A point's coordinate encoding is formed
//                  once and reused by the T times.
//   k_alpha_mask_build  : the native part of updateAlphaMask (:592-629): clamp, 3x3x3 max pool per time slice, threshold,
//                  bit packing in the order `save` (:465-469) flattens the volume, occupied count and lattice box
//   k_alpha_mask_sample : AlphaGridMask.sample_alpha (:56-73) straight from the packed bits, and the AND of (value > 0)
//                  into the `valid` bytes of a ray batch for up to two masks
#include "rdrf_fwd_dev.hpp"
#include "rdrf_mask_dev.hpp"

// ------------------------------------------------------------------------------------------------
// compute_alpha
// ------------------------------------------------------------------------------------------------
struct AlphaArgs {
  const float* xyz;     // [M][3] un-normalised
  const float* times;   // [T]
  const float* pk;      // packed forward image (dynamic)
  const float* tout;    // [T][32] time-branch outputs (dynamic)
  float* alpha;         // [M][T]
  float* sigma;         // [M][T] or nullptr
  long long M;
  int T;
  float length, density_shift;
  int act, dynq;
  Box box;
  MaskDev mask;
};

__global__ __launch_bounds__(256) void k_alpha_time_branch(const float* __restrict__ ts, DynW w, int N, float* __restrict__ tout) {
  __shared__ float s_h[8 * 64];
  time_branch_body(ts, w, N, tout, s_h, grid_ctx());
}

// flat 32-point tiles from the workgroup's queue, as k_dyn_density_flat; per tile the T times in turn
__global__ __launch_bounds__(64 * RDRF_MAXW) void k_alpha_dyn(AlphaArgs a, DynW w) {
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
      // compiler barrier: nothing below writes LDS, so without it the weight reads of every layer are invariant in kt and
      // get hoisted out of the loop into registers the kernel does not have
      asm volatile("" ::: "memory");
      const float t = a.times[kt];
      if (h == 0) X0[3] = t;
      float T[16];
      load_tout(T, a.tout, (size_t)kt, h);
      float d[3];
      warp_mlp(d, X0, T, pkw, w.l5b, nullptr, s, h, lane);
      // (the point is read again here and at the mask lookup: six registers less across the layers; same loads, same bits)
      const float* pp = a.xyz + (size_t)idx * 3;
      asm volatile("" : "+v"(pp));
      const float xn[3] = {norm_c(pp[0], a.box.lo[0], a.box.inv[0]), norm_c(pp[1], a.box.lo[1], a.box.inv[1]),
                           norm_c(pp[2], a.box.lo[2], a.box.inv[2])};
      float xw[3];
      warp_point(xw, xn, d, a.box);
      float X1[8];
      fill_x1(X1, t, h);
      const float fd = head_raw<false>(w, xw, act, X0, X1, pkw, nullptr, s, h, lane);
      if (act && h == 0) {
        // the mask is looked up here, where only fd is live: a masked point's column was computed and is dropped (no
        // column of an MFMA reads another's), which costs less than holding the lookup's registers across the layers
        bool vld = true;
        if (a.mask.bits != nullptr) {
          const float* p = a.xyz + (size_t)idx * 3;
          asm volatile("" : "+v"(p));
          vld = mask_sample(a.mask, p[0], p[1], p[2], mask_slice(a.mask, t)) > 0.0f;
        }
        const float sigma = vld ? density_act(fd, a.act, a.density_shift) : 0.0f;
        a.alpha[(size_t)idx * a.T + kt] = 1.0f - expf(-sigma * a.length);
        if (a.sigma != nullptr) a.sigma[(size_t)idx * a.T + kt] = sigma;
      }
    }
  }
}

// the static field: a lane per point, static_density_feature as in static_density_body; sigma does not depend on the time (the mask does)
__global__ __launch_bounds__(256) void k_alpha_static(AlphaArgs a, StaticW w) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.M; i += (long long)gridDim.x * blockDim.x) {
    const size_t idx = (size_t)i;
    const float px = a.xyz[idx * 3 + 0], py = a.xyz[idx * 3 + 1], pz = a.xyz[idx * 3 + 2];
    const float x0 = norm_c(px, a.box.lo[0], a.box.inv[0]);
    const float x1 = norm_c(py, a.box.lo[1], a.box.inv[1]);
    const float x2 = norm_c(pz, a.box.lo[2], a.box.inv[2]);
    const float f = static_density_feature(w.density, x0, x1, x2);
    const float sig = density_act(f, a.act, a.density_shift);
    for (int kt = 0; kt < a.T; ++kt) {
      bool vld = true;
      if (a.mask.bits != nullptr) vld = mask_sample(a.mask, px, py, pz, mask_slice(a.mask, a.times[kt])) > 0.0f;
      const float sigma = vld ? sig : 0.0f;
      a.alpha[(size_t)idx * a.T + kt] = 1.0f - expf(-sigma * a.length);
      if (a.sigma != nullptr) a.sigma[idx * a.T + kt] = sigma;
    }
  }
}

// workspace of the dynamic field's alpha: the pack area and the time branch of the T times (nothing is kept per point)
static void carve_alpha(float*& pk, float*& tout, WsCarver& c, int T) {
  pk = c.take<float>(PACK_AREA_FLOATS);
  tout = c.take<float>((size_t)(T > 0 ? T : 0) * 32);
}
extern "C" size_t rdrf_compute_alpha_workspace_bytes(int M, int T) {
  (void)M;
  float *pk, *tout;
  WsCarver c;
  carve_alpha(pk, tout, c, T);
  return c.off;
}

extern "C" int rdrf_compute_alpha(const void* params, int dynamic, const RdrfFieldCfg* cfg, const float* xyz, int M,
                                  const float* times, int T, float length, const RdrfAlphaMask* mask, float* alpha,
                                  float* sigma, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (M == 0 || T == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(params && cfg && xyz && times && alpha && M > 0 && T > 0, -1, "compute_alpha: bad arguments");
  RDRF_CHECK(mask_ok(mask), -1, "compute_alpha: the mask's grid and slice count must be positive");
  AlphaArgs a;
  memset(&a, 0, sizeof(a));
  a.xyz = xyz; a.times = times; a.alpha = alpha; a.sigma = sigma;
  a.M = M; a.T = T; a.length = length;
  a.density_shift = cfg->density_shift; a.act = cfg->act;
  a.box = make_box(cfg);
  a.mask = make_mask(mask);
  if (!dynamic) {
    const RdrfStaticParams* P = (const RdrfStaticParams*)params;
    RDRF_CHECK(vm_ok(P->density, 16, 4), -1,
               "compute_alpha: only density comps {16,4,4}, the planes and lines of a set spanning one grid, are built");
    StaticW w;
    fill_static_w(w, P);
    const long blocks = ((long)M + 255) / 256;
    RDRF_LAUNCH("alpha_static", k_alpha_static, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), stream, a, w);
    return 0;
  }
  const RdrfDynamicParams* P = (const RdrfDynamicParams*)params;
  RDRF_CHECK(vm_ok(P->density, 16, 4), -1,
             "compute_alpha: only density comps {16,4,4}, the planes and lines of a set spanning one grid, are built");
  RDRF_CHECK(ws != nullptr, -3, "compute_alpha: no workspace");
  WsCarver c(ws, ws_bytes);
  float *pkbuf, *tout;
  carve_alpha(pkbuf, tout, c, T);
  RDRF_CHECK(c.ok(), -3, "compute_alpha: workspace too small: need %zu have %zu", c.off, ws_bytes);
  DynW w;
  fill_dyn_w(w, P);
  RDRF_TRY(pack_image(a.pk, P->packed_fwd, pkbuf, stream, dyn_pack_jobs_fwd, P));
  a.tout = tout;
  a.dynq = 1;
  RDRF_LAUNCH("time_branch", k_alpha_time_branch, dim3((T + 7) / 8), dim3(256), stream, times, w, T, tout);
  const Geo g = geo_for_units(((long)M + 31) / 32);   // the persistent geometry of the field kernels
  RDRF_LAUNCH("alpha_dyn", k_alpha_dyn, dim3(g.grid), dim3(g.block), stream, a, w);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// updateAlphaMask: alpha [G0][G1][G2][T] -> packed occupancy (G2, G1, G0, T), count, lattice box
// A thread forms one output byte: eight consecutive bits of the flattened (iz, iy, ix, k) order.  The statistics are
// reduced over the wave by shuffles, over the workgroup in LDS, and one lane per workgroup adds them to the totals.
// stats: [0] occupied count, [1..3] min ix, iy, iz, [4..6] max ix, iy, iz (unsigned 64-bit)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_alpha_mask_build(const float* __restrict__ alpha, int G0, int G1, int G2, int T, float thres,
                                                          uint8_t* __restrict__ bits, unsigned long long* __restrict__ stats) {
  __shared__ unsigned s_red[4][7];
  const size_t total = (size_t)G0 * G1 * G2 * T;
  const size_t nbytes = (total + 7) >> 3;
  unsigned cnt = 0, mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbytes; b += (size_t)gridDim.x * blockDim.x) {
    unsigned byte = 0;
    for (int j = 0; j < 8; ++j) {
      const size_t f = b * 8 + j;
      if (f >= total) break;   // the tail bits of the last byte stay 0 (np.packbits pads with zeros)
      const int k = (int)(f % T);
      size_t r = f / T;
      const int c[3] = {(int)(r % G0), (int)((r / G0) % G1), (int)(r / ((size_t)G0 * G1))};   // ix, iy, iz
      float m = -1.0f;   // (below every clamped value: the padding of max_pool3d never wins)
      for (int dx = -1; dx <= 1; ++dx) {
        const int x = c[0] + dx;
        if (x < 0 || x >= G0) continue;
        for (int dy = -1; dy <= 1; ++dy) {
          const int y = c[1] + dy;
          if (y < 0 || y >= G1) continue;
          for (int dz = -1; dz <= 1; ++dz) {
            const int z = c[2] + dz;
            if (z < 0 || z >= G2) continue;
            const float v = alpha[(((size_t)x * G1 + y) * G2 + z) * T + k];
            const float cl = fminf(fmaxf(v, 0.0f), 1.0f);
            m = (cl > m || cl != cl) ? cl : m;   // a NaN propagates, as in max_pool3d
          }
        }
      }
      if (m >= thres) {
        byte |= 0x80u >> j;
        ++cnt;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          mn[d] = min(mn[d], (unsigned)c[d]);
          mx[d] = max(mx[d], (unsigned)c[d]);
        }
      }
    }
    bits[b] = (uint8_t)byte;
  }
  unsigned v[7] = {cnt, mn[0], mn[1], mn[2], mx[0], mx[1], mx[2]};
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    v[0] += __shfl_xor(v[0], off, 64);
#pragma unroll
    for (int d = 1; d < 4; ++d) v[d] = min(v[d], (unsigned)__shfl_xor(v[d], off, 64));
#pragma unroll
    for (int d = 4; d < 7; ++d) v[d] = max(v[d], (unsigned)__shfl_xor(v[d], off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int d = 0; d < 7; ++d) s_red[threadIdx.x >> 6][d] = v[d];
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int d = threadIdx.x;
    unsigned r = s_red[0][d];
    for (int w = 1; w < 4; ++w) r = d == 0 ? r + s_red[w][d] : (d < 4 ? min(r, s_red[w][d]) : max(r, s_red[w][d]));
    if (s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0] != 0u) {   // a workgroup without an occupied voxel adds nothing
      if (d == 0) atomicAdd(&stats[0], (unsigned long long)r);
      else if (d < 4) atomicMin(&stats[d], (unsigned long long)r);
      else atomicMax(&stats[d], (unsigned long long)r);
    }
  }
}

extern "C" int rdrf_alpha_mask_build(const float* alpha, int G0, int G1, int G2, int T, float thres, uint8_t* bits,
                                     int64_t* stats, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(alpha && bits && stats && G0 > 0 && G1 > 0 && G2 > 0 && T > 0, -1, "alpha_mask_build: bad arguments");
  const size_t nbytes = ((size_t)G0 * G1 * G2 * T + 7) >> 3;
  RDRF_FILL(stats, 0, 7 * sizeof(int64_t), stream);
  RDRF_FILL(stats + 1, 0x7f, 3 * sizeof(int64_t), stream);   // the minima start above every lattice index
  const size_t blocks = (nbytes + 255) / 256;
  RDRF_LAUNCH("alpha_mask_build", k_alpha_mask_build, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), stream, alpha,
              G0, G1, G2, T, thres, bits, (unsigned long long*)stats);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// sample_alpha / ray_valid &= alpha_mask
// ------------------------------------------------------------------------------------------------
// out != nullptr: out[i] = sample of m0 at point i, time t[i * t_stride]
// valid != nullptr: valid[i] &= (m0 > 0) | (m1 > 0) at point i of ray i / S, time t[i / S]
__global__ __launch_bounds__(256) void k_alpha_mask_sample(MaskDev m0, MaskDev m1, const float* __restrict__ xyz,
                                                           const float* __restrict__ t, int t_stride, long long n, int S,
                                                           float* __restrict__ out, uint8_t* __restrict__ valid) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float x = xyz[(size_t)i * 3 + 0], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
    if (out != nullptr) {
      const float tt = t[(size_t)i * t_stride];
      out[i] = mask_sample(m0, x, y, z, mask_slice(m0, tt));
    } else {
      if (valid[i] == 0) continue;
      const float tt = t[i / S];
      bool keep = mask_sample(m0, x, y, z, mask_slice(m0, tt)) > 0.0f;
      if (!keep && m1.bits != nullptr) keep = mask_sample(m1, x, y, z, mask_slice(m1, tt)) > 0.0f;
      if (!keep) valid[i] = 0;
    }
  }
}

extern "C" int rdrf_alpha_mask_sample(const RdrfAlphaMask* mask, const float* xyz, const float* t, int t_per_point, int64_t n,
                                      float* out, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(mask && mask->bits && xyz && t && out && n > 0, -1, "alpha_mask_sample: bad arguments");
  RDRF_CHECK(mask_ok(mask), -1, "alpha_mask_sample: the mask's grid and slice count must be positive");
  const MaskDev m0 = make_mask(mask), m1 = make_mask(nullptr);
  const int64_t blocks = (n + 255) / 256;
  RDRF_LAUNCH("alpha_mask_sample", k_alpha_mask_sample, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), stream, m0, m1,
              xyz, t, t_per_point ? 1 : 0, (long long)n, 1, out, (uint8_t*)nullptr);
  return 0;
}

extern "C" int rdrf_alpha_mask_valid(const RdrfAlphaMask* mask0, const RdrfAlphaMask* mask1, const float* xyz, const float* ts,
                                     int N, int S, uint8_t* valid, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0 || S == 0) return 0;   // empty batch: a no-op
  RDRF_CHECK(mask0 && mask0->bits && xyz && ts && valid && N > 0 && S > 0, -1, "alpha_mask_valid: bad arguments");
  RDRF_CHECK(mask_ok(mask0) && mask_ok(mask1), -1, "alpha_mask_valid: the masks' grids and slice counts must be positive");
  const MaskDev m0 = make_mask(mask0), m1 = make_mask(mask1);
  const long long n = (long long)N * S;
  const long long blocks = (n + 255) / 256;
  RDRF_LAUNCH("alpha_mask_valid", k_alpha_mask_sample, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), stream, m0, m1,
              xyz, ts, 0, n, S, (float*)nullptr, valid);
  return 0;
}
