// rdrf_scatter.hip -- VM gather backward as kernels of their own: the feature-gradient rows (or sample-major records) that
// the backward-data kernels of rdrf_bwd.hip wrote are scattered into the factor planes / lines, and the coordinate
// gradients are formed.  Three forms share the per-quad device functions of rdrf_bwd_dev.hpp: the ray-tile kernel
// (k_scatter), the sorted kernels (k_sort_keys + k_scatter_sorted: samples grouped by plane cell first)
// and the sorted kernel with LDS plane windows (k_scatter_tiled); the launch policy of each is here too.
// Host interface: rdrf_bwd_host.hpp.
#include "rdrf_bwd_dev.hpp"
#include "rdrf_bwd_host.hpp"
#include "rdrf_sort_dev.hpp"

RDRF_DET_UNIT(scatter)

// ------------------------------------------------------------------------------------------------
// generic scatter kernel: VM gather backward of one or two factor sets from feature-gradient rows.
// No MFMA state and no weight image -> ~100 VGPRs, several workgroups per CU: the dependent
// shuffle-scan / atomic latency chains of different waves overlap (inside the fused MLP kernels,
// at 2 waves/SIMD, they were 85 % of the backward-data time).
// ------------------------------------------------------------------------------------------------
#ifndef SC_LINES_MAX_BYTES
/* LDS line-gradient accumulators per workgroup, sized per launch (dynamic LDS): up to 80 KB keeps two
   256-thread workgroups per CU; up to 152 KB runs one 512-thread workgroup per CU, still faster than
   sending the line gradients to global atomics (final stage appearance: 3.9 -> 2.6 ms) */
#define SC_LINES_MAX_BYTES (152 * 1024)
#endif
// (ScatterArgs: rdrf_bwd_host.hpp)

template <int C0Q, int C1Q, int NQ>
__global__ __launch_bounds__(512, 3) void k_scatter(ScatterArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lacc[];
  const int nl0 = lines_floats(a.vm[0]), nl1 = a.nsets > 1 ? lines_floats(a.vm[1]) : 0;
  const bool use_lacc = a.lds_bytes > 0;   // host: (nl0 + nl1) elements of 8 (lds_f64) or 4 bytes if they fit SC_LINES_MAX_BYTES, else 0
  if (use_lacc)
    for (int i = threadIdx.x; i < (nl0 + nl1) * (a.lds_f64 ? 2 : 1); i += blockDim.x) lacc[i] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int tpr = (a.S + 31) >> 5;
  const int count = a.list ? *a.count : 0;
  const int ntiles = a.list ? ((count + 31) >> 5) : (a.flat ? (a.N * a.S + 31) >> 5 : a.N * tpr);
  for (int t = blockIdx.x * nwaves + wave; t < ntiles; t += gridDim.x * nwaves) {
    int idx;
    bool live;
    if (a.list) {
      const int li = t * 32 + s;
      live = li < count;
      idx = live ? a.list[li] : 0;
    } else if (a.flat) {
      const int i = t * 32 + s;
      const bool act = i < a.N * a.S;
      idx = act ? i : 0;
      live = act && a.valid[idx] != 0;
    } else {
      const int n = t / tpr, j = (t - n * tpr) * 32 + s;
      const bool act = j < a.S;
      idx = n * a.S + (act ? j : 0);
      live = act && a.valid[idx] != 0;
    }
    float x0, x1, x2;
    if (a.xw) {
      x0 = a.xw[(size_t)idx * 3 + 0]; x1 = a.xw[(size_t)idx * 3 + 1]; x2 = a.xw[(size_t)idx * 3 + 2];
    } else {
      x0 = norm_c(a.xyz[(size_t)idx * 3 + 0], a.box.lo[0], a.box.inv[0]);
      x1 = norm_c(a.xyz[(size_t)idx * 3 + 1], a.box.lo[1], a.box.inv[1]);
      x2 = norm_c(a.xyz[(size_t)idx * 3 + 2], a.box.lo[2], a.box.inv[2]);
    }
    // coordinates / liveness of the samples this lane handles in the (quad, 16-sample) mapping of
    // the XY iterations: sample 16 j + (lane & 15), j = 0, 1 (lanes 0..31 hold samples 0..31)
    const float xa0 = __shfl(x0, lane & 15, 64), xa1 = __shfl(x1, lane & 15, 64), xa2 = __shfl(x2, lane & 15, 64);
    const float xb0 = __shfl(x0, 16 + (lane & 15), 64), xb1 = __shfl(x1, 16 + (lane & 15), 64),
                xb2 = __shfl(x2, 16 + (lane & 15), 64);
    const bool livea = __shfl((int)live, lane & 15, 64) != 0, liveb = __shfl((int)live, 16 + (lane & 15), 64) != 0;
    float dw0 = 0.f, dw1 = 0.f, dw2 = 0.f;
    for (int set = 0; set < a.nsets; ++set) {
      const float* rb = a.rows + ((size_t)t * a.stride + a.row0[set]) * 32;
      const LdsLines ll = make_lds_lines(use_lacc ? lacc : nullptr, set ? nl0 : 0, a.lds_f64, a.vm[set]);
      // Per level: the XY plane's C0Q quads go four at a time over 16-sample sub-tiles
      // (gather_xy4_bwd: a texel's four quads in one instruction = one 64-byte request); then the
      // XZ / YZ quads, either column-split over the half-waves (ZSPLIT: density / blending, one
      // quad per wave iteration, two bilinear columns = one request) or one quad per half-wave.
      constexpr bool ZSPLIT = C0Q <= 4;
      constexpr int QPL = C0Q + 2 * C1Q, NLV = (2 * NQ) / QPL;
      static_assert(C0Q % 4 == 0 && NLV * QPL == 2 * NQ, "quad layout");
      const int q = lane >> 4, s16 = lane & 15;
#pragma unroll 1
      for (int lv = 0; lv < NLV; ++lv) {
#pragma unroll 1
        for (int it = 0; it < C0Q / 2; ++it) {
          const int grp = it >> 1, j = it & 1;
          const int g = lv * QPL + 4 * grp + q;
          const int sidx = 16 * j + s16;
          const float* rq = rb + (a.bcast ? (size_t)0 : (size_t)(4 * g) * 32) + sidx;
          const int rs = a.bcast ? 0 : 32;
          const f32x4 dq = {rq[0], rq[rs], rq[2 * rs], rq[3 * rs]};
          gather_xy4_bwd<C0Q, C1Q>(a.vm[set], a.gvm[set], lv, 4 * grp + q, j ? xb0 : xa0, j ? xb1 : xa1,
                                   j ? xb2 : xa2, dq, j ? liveb : livea, lane < 32 && q == j, dw0, dw1, dw2, ll);
        }
        if constexpr (ZSPLIT) {
#pragma unroll 1
          for (int zq = 0; zq < 2 * C1Q; ++zq) {
            const int g = lv * QPL + C0Q + zq;
            const float* rq = rb + (a.bcast ? (size_t)0 : (size_t)(4 * g) * 32) + s;
            const int rs = a.bcast ? 0 : 32;
            const f32x4 dq = {rq[0], rq[rs], rq[2 * rs], rq[3 * rs]};
            gather_zquad_bwd<C0Q, C1Q>(a.vm[set], a.gvm[set], g, h, x0, x1, x2, dq, live, s, dw0, dw1, dw2, ll);
          }
        } else {
#pragma unroll 1
          for (int zp = 0; zp < C1Q; ++zp) {
            const int g = lv * QPL + C0Q + 2 * zp + h;
            const float* rq = rb + (a.bcast ? (size_t)0 : (size_t)(4 * g) * 32) + s;
            const int rs = a.bcast ? 0 : 32;
            const f32x4 dq = {rq[0], rq[rs], rq[2 * rs], rq[3 * rs]};
            gather_quad_bwd<C0Q, C1Q, 1>(a.vm[set], a.gvm[set], g, x0, x1, x2, dq, live, s, dw0, dw1, dw2, ll);
          }
        }
      }
    }
    dw0 += __shfl_xor(dw0, 32, 64); dw1 += __shfl_xor(dw1, 32, 64); dw2 += __shfl_xor(dw2, 32, 64);
    if (live && h == 0) {
      if (a.dxw) {
        float* d = a.dxw + (size_t)idx * 3;
        if (a.dxw_accumulate) { d[0] += dw0; d[1] += dw1; d[2] += dw2; }
        else { d[0] = dw0; d[1] = dw1; d[2] = dw2; }
      }
      if (a.g_xyz) {
        a.g_xyz[(size_t)idx * 3 + 0] += dw0 * a.box.inv[0];
        a.g_xyz[(size_t)idx * 3 + 1] += dw1 * a.box.inv[1];
        a.g_xyz[(size_t)idx * 3 + 2] += dw2 * a.box.inv[2];
      }
    }
  }
  if (use_lacc) {
    __syncthreads();
    flush_lds_lines(lacc, a.lds_f64, 0, a.vm[0], a.gvm[0]);
    if (a.nsets > 1) flush_lds_lines(lacc, a.lds_f64, nl0, a.vm[1], a.gvm[1]);
  }
}

// ------------------------------------------------------------------------------------------------
// SORTED scatter of the density / blending gradients (dynamic field, ray path).
//
// With the reference initialiser the warp MLP moves the warped point by about a texel between consecutive samples of
// a ray, so the ray-tile scatter above finds runs of 1-2 samples and pays ~13 M memory-side atomic requests per launch
//  for gradient planes of a few MB.  Here the live samples are first grouped by the plane CELL they fall
// into (one stable radix sort of (plane | level-0 cell) keys per plane segment, rdrf_sort.hip), and each
// plane is scattered in that order by the SAME per-quad device functions: consecutive lanes now hold samples of the
// same or the neighbouring cell (~20-40 samples per level-0 cell at the benchmark shapes), so the in-register run
// reduction collapses them and a run of lanes issues one request per tap.  Per plane: XY = 16 samples x 4 quads per
// wave step (gather_xy4_bwd), XZ / YZ = 32 samples, the half-waves taking the two bilinear columns (gather_zquad_bwd).
// d(features) come from the sample-major records the heads kernel writes (BwdArgs::dfs); coordinate gradients are
// accumulated into dxw by the three launches in turn (a sample is owned by one lane per launch: no atomics).
// ------------------------------------------------------------------------------------------------
struct SortKeyArgs {
  const float* xw;
  const uint8_t* valid;
  const float* grows1;   // K1G_SM rows 3 / 4 hold g_fd / g_fb: a sample with both zero scatters nothing
  const int* list;       // appearance: the compacted sample ids (entry li of the key arrays = compacted sample li) ...
  const int* count;      // ... and their device count; nullptr: every sample of the batch, liveness from valid / grows1
  int N, S;
  int W[3], H[3];        // level-0 plane sizes
  int kb;                // bits of the cell part of the key
  unsigned* keys;        // [3][N*S]; compact: [3][*count]
  int* counts;           // [3] live entries per plane
  int flat;              // the density-phase rows are addressed by flat 32-sample tile (rdrf_flat_density)
  int compact;           // list mode: the key arrays hold the *count compacted entries of each plane back to back (stride *count
                         // instead of N*S), so that the sort and the key generation touch live entries only (round 6)
  // tables of the sort's first pass (rdrf_sort_dev.hpp): per tile of RS_TILE entries and plane, the histogram of the keys'
  // lowest digit (nbins bins) and the number of dropped keys
  unsigned* hist;
  unsigned* drops;
  unsigned tps;
  int nbins;
};

RDRF_D int cell_axis(float c, int L, bool& any) {
  // level-0 tap index clamped to [-2, L]; `any`: some stride level has an in-range tap on this axis
  const Tap1 t0 = tap1d(c, L), t1 = tap1d(c, (L + 1) >> 1), t2 = tap1d(c, (L + 3) >> 2);
  any = t0.ok0 || t0.ok1 || t1.ok0 || t1.ok1 || t2.ok0 || t2.ok1;
  return min(max(t0.i0, -2), L) + 2;
}

// A workgroup owns tiles of RS_TILE entries -- the tiles of the sort (a plane's keys are one segment of it) -- and writes,
// besides the keys, what the sort's first pass needs of each tile: per plane the histogram of the lowest digit and the
// number of dropped keys.  Plain stores into the tile's own table entries: the first pass starts at its scan, whose extra
// workgroup per plane turns the drop counts into counts[plane] = entries - dropped (a per-wave atomic counter here
// serialised 66 k same-address atomics: 240 us; a search of the sorted keys was a launch of its own).
constexpr int SK_THREADS = 1024;
__global__ __launch_bounds__(SK_THREADS) void k_sort_keys(SortKeyArgs a) {
  __shared__ unsigned h[3 * RS_BINS];
  __shared__ unsigned dr[3];
  const int NS = a.N * a.S, tpr = (a.S + 31) >> 5;
  const int count = a.list ? min(*a.count, NS) : 0;
  const int nent = (a.list && a.compact) ? count : NS;   // entries per plane = the stride of the key arrays
  const unsigned ntile = nent > 0 ? rs_tiles((unsigned)nent) : 0u, mask = (unsigned)a.nbins - 1u;
  const int lane = threadIdx.x & 63;
  for (unsigned t = blockIdx.x; t < ntile; t += gridDim.x) {
    for (int i = threadIdx.x; i < 3 * RS_BINS; i += SK_THREADS) h[i] = 0u;
    if (threadIdx.x < 3) dr[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RS_TILE / SK_THREADS; ++k) {
      const int e = (int)(t * RS_TILE) + k * SK_THREADS + (int)threadIdx.x;
      const bool have = e < nent;
      bool live = false;
      float x0 = 0.f, x1 = 0.f, x2 = 0.f;
      if (have) {
        if (a.list) {
          live = e < count;
          const int idx = live ? a.list[e] : 0;
          x0 = a.xw[(size_t)idx * 3 + 0]; x1 = a.xw[(size_t)idx * 3 + 1]; x2 = a.xw[(size_t)idx * 3 + 2];
        } else {
          const int idx = e;
          const int n = idx / a.S, j = idx - n * a.S;
          const float* sm = a.grows1 + ((size_t)(a.flat ? idx >> 5 : n * tpr + (j >> 5)) * sv::K1G_ROWS + sv::K1G_SM) * 32 +
                            (a.flat ? idx & 31 : j & 31);
          live = a.valid[idx] != 0 && (sm[3 * 32] != 0.f || sm[4 * 32] != 0.f);
          x0 = a.xw[(size_t)idx * 3 + 0]; x1 = a.xw[(size_t)idx * 3 + 1]; x2 = a.xw[(size_t)idx * 3 + 2];
        }
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const float cx = p == 2 ? x1 : x0, cy = p == 0 ? x1 : x2;
        bool ax, ay;
        const int ix = cell_axis(cx, a.W[p], ax), iy = cell_axis(cy, a.H[p], ay);
        const bool in = live && ax && ay;
        const unsigned cell = in ? (unsigned)(iy * (a.W[p] + 3) + ix) : ((1u << a.kb) - 1u);
        if (have) {
          a.keys[(size_t)p * nent + e] = ((unsigned)p << a.kb) | cell;
          atomicAdd(&h[p * RS_BINS + (cell & mask)], 1u);
        }
        const unsigned long long dropped = __ballot(have && !in);
        if (lane == 0 && dropped) atomicAdd(&dr[p], (unsigned)__popcll(dropped));
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * a.nbins; i += SK_THREADS) {
      const int p = i / a.nbins, d = i - p * a.nbins;
      a.hist[rs_hist_at(p, a.nbins, (unsigned)d, a.tps, t)] = h[p * RS_BINS + d];
    }
    if (threadIdx.x < 3) a.drops[rs_drops_at((int)threadIdx.x, a.tps, t)] = dr[threadIdx.x];
    __syncthreads();   // (the next tile zeroes the tables)
  }
}

struct SortedScatterArgs {
  RdrfVM vm[2], gvm[2];
  int set_mask;            // bit k: set k has a gradient
  const unsigned* order;   // [NS] sorted positions of THIS plane (value = plane * NS + entry index)
  const int* count;        // live entries of this plane
  unsigned base;           // plane * NS
  const int* seg;          // compact key arrays: `order` is the base of the whole array, this plane's positions start at
                           // PLANE * *seg and carry that base (nullptr: order / base as given)
  const float* dfs;        // records: entry e at dfs + e * rec_floats (+ set * floats per set)
  int rec_floats;
  const int* list;         // appearance: entry e is compacted sample e, its sample id is list[e]; nullptr: entry = sample id
  const float* xw;
  float* dxw;              // += coordinate gradients
  int lds_bytes, lds_f64;  // line accumulator of this pass in LDS: bytes (0: global atomics), doubles / floats
  int line_direct;         // no run reduction in front of the LDS line updates (see LdsLines::direct)
  // k_scatter_tiled: the sorted keys of this plane (a slice's window is anchored at its first key), bits of the cell part
  // of a key, key-space row length W + 3, window width in cells, wave steps per slice, windows allocated (factor sets)
  const unsigned* keys;
  int kb, Wk, tw, slice_steps, tile_sets;
};

// C0Q / C1Q: quads of an XY / XZ-YZ texel: <4, 1> density and blending ({16,4,4} components, two sets per record),
// <12, 3> appearance ({48,12,12}, one set, entries = the compacted list)
template <int PLANE, int C0Q, int C1Q>
__global__ __launch_bounds__(512, 3) void k_scatter_sorted(SortedScatterArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lacc[];
  // pass PLANE touches line PLANE only (the partner of its plane): one line per factor set in the accumulator
  const int nl0 = (a.set_mask & 1) ? a.vm[0].L[PLANE] * lds_stride(a.vm[0].C[PLANE]) : 0;   // (no accumulator for a factor set
  const int nl1 = (a.set_mask & 2) ? a.vm[1].L[PLANE] * lds_stride(a.vm[1].C[PLANE]) : 0;   //  without a gradient in this launch)
  const bool use_lacc = a.lds_bytes > 0;
  if (use_lacc)
    for (int i = threadIdx.x; i < (nl0 + nl1) * (a.lds_f64 ? 2 : 1); i += blockDim.x) lacc[i] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31, q = lane >> 4, s16 = lane & 15;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int count = *a.count;
  const unsigned obase = a.seg ? (unsigned)PLANE * (unsigned)*a.seg : a.base;   // compact key arrays (SortKeyArgs::compact)
  const unsigned* order = a.seg ? a.order + obase : a.order;
  constexpr int SPT = PLANE == 0 ? 16 : 32;   // samples per wave step
  // record of one set: [XY level 0 | 1 | 2 (XYF floats each)] [XZ: 3 x ZF] [YZ: 3 x ZF]
  constexpr int XYF = 4 * C0Q, ZF = 4 * C1Q, SETF = 3 * XYF + 6 * ZF, QPL = C0Q + 2 * C1Q;
  const int ntiles = (count + SPT - 1) / SPT;
  for (int t = blockIdx.x * nwaves + wave; t < ntiles; t += gridDim.x * nwaves) {
    const int pos = t * SPT + (PLANE == 0 ? s16 : s);
    const bool live = pos < count;
    const int ent = live ? (int)(order[pos] - obase) : 0;
    const int idx = a.list ? a.list[ent] : ent;
    const float x0 = a.xw[(size_t)idx * 3 + 0], x1 = a.xw[(size_t)idx * 3 + 1], x2 = a.xw[(size_t)idx * 3 + 2];
    float dw0 = 0.f, dw1 = 0.f, dw2 = 0.f;
#pragma unroll 1
    for (int set = 0; set < 2; ++set) {
      if (!((a.set_mask >> set) & 1)) continue;
      const int first = set ? nl0 : 0;
      const LdsLines ll = LdsLines{use_lacc ? lacc : nullptr, {first, first, first}, a.lds_f64, a.line_direct};
      const float* rec = a.dfs + (size_t)ent * a.rec_floats + set * SETF;
#pragma unroll 1
      for (int lv = 0; lv < 3; ++lv) {
        if constexpr (PLANE == 0) {
#pragma unroll 1
          for (int grp = 0; grp < C0Q / 4; ++grp) {
            const f32x4 dq = live ? ld4(rec + lv * XYF + grp * 16 + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
            gather_xy4_bwd<C0Q, C1Q>(a.vm[set], a.gvm[set], lv, 4 * grp + q, x0, x1, x2, dq, live, q == 0, dw0, dw1, dw2, ll);
          }
        } else {
#pragma unroll 1
          for (int zq = 0; zq < C1Q; ++zq) {
            const f32x4 dq = live ? ld4(rec + 3 * XYF + (PLANE - 1) * 3 * ZF + lv * ZF + 4 * zq) : f32x4{0.f, 0.f, 0.f, 0.f};
            gather_zquad_bwd<C0Q, C1Q>(a.vm[set], a.gvm[set], lv * QPL + C0Q + (PLANE - 1) * C1Q + zq, h, x0, x1, x2, dq, live, s,
                                       dw0, dw1, dw2, ll);
          }
        }
      }
    }
    if constexpr (PLANE != 0) {   // both halves computed half of every coordinate gradient
      dw0 += __shfl_xor(dw0, 32, 64); dw1 += __shfl_xor(dw1, 32, 64); dw2 += __shfl_xor(dw2, 32, 64);
    }
    if (live && (PLANE == 0 ? q == 0 : h == 0)) {
      float* d = a.dxw + (size_t)idx * 3;
      d[0] += dw0; d[1] += dw1; d[2] += dw2;
    }
  }
  if (use_lacc) {
    __syncthreads();
    if (a.set_mask & 1) flush_lds_line(lacc, a.lds_f64, 0, a.vm[0].L[PLANE], a.vm[0].C[PLANE], a.gvm[0].line[PLANE]);
    if (a.set_mask & 2) flush_lds_line(lacc, a.lds_f64, nl0, a.vm[1].L[PLANE], a.vm[1].C[PLANE], a.gvm[1].line[PLANE]);
  }
}

// ------------------------------------------------------------------------------------------------
// TILED sorted scatter.  After the LDS line accumulators became doubles (ds_add_f64), what was left of the sorted passes
// was their memory-side plane atomics: 1.08 of 1.85 ms per step for the density / blending scatter (ablation builds,
// profiles/r05_scatter_ablation.txt) although the sort had already cut the REQUESTS tenfold -- every run tail still pays a
// round trip to the memory side, and vmcnt is one in-order counter, so the next gathers wait behind it.  Neighbouring
// plane cells are neighbours in the sorted array, so a SLICE of consecutive sorted entries (slice_steps wave steps of
// one workgroup) touches a window of ~(tw + 1) x 2 texels per stride level, anchored at the slice's first cell: the
// window lives in LDS as doubles, the run tails add into it with ds_add_f64, and the workgroup flushes it with one
// coalesced sweep (64-byte texels = one request per 16 lanes).  Slices have equal size (static stride over the workgroups:
// the load is balanced by construction; windows by CELL ranges with a dynamic queue were 2 x slower than the untiled
// kernel, the ray density per cell varies too much).  Everything per entry (taps, run reduction, cross-run merge,
// coordinate gradients, line updates) is the code of k_scatter_sorted; only the destination of a plane sum differs
// (plane_add4), and a tap outside the window (the slice ran into the next key row, a sparse region, a clamped key)
// still goes to global memory, so the result is the same sum in a different order.
// ------------------------------------------------------------------------------------------------
RDRF_HD int tile_texels(int tw) { return (tw + 1) * 2 + (tw / 2 + 3) * 3 + (tw / 4 + 3) * 3; }

template <int PLANE, int C0Q, int C1Q>
__global__ __launch_bounds__(512, 4) void k_scatter_tiled(SortedScatterArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lacc[];   // doubles: [line set 0 | line set 1 | tile set 0 | tile set 1]
  __shared__ int s_geo[24];
  constexpr int CT = PLANE == 0 ? 4 * C0Q : 4 * C1Q;   // components per texel of this plane
  // (a factor set without a gradient in this launch gets no accumulator)
  const int nl0 = (a.set_mask & 1) ? a.vm[0].L[PLANE] * lds_stride(a.vm[0].C[PLANE]) : 0;
  const int nl1 = (a.set_mask & 2) ? a.vm[1].L[PLANE] * lds_stride(a.vm[1].C[PLANE]) : 0;
  const int tile_elems = tile_texels(a.tw) * CT;
  for (int i = threadIdx.x; i < (nl0 + nl1 + a.tile_sets * tile_elems) * 2; i += blockDim.x) lacc[i] = 0.f;
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31, q = lane >> 4, s16 = lane & 15;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int count = *a.count;
  constexpr int SPT = PLANE == 0 ? 16 : 32;
  constexpr int XYF = 4 * C0Q, ZF = 4 * C1Q, SETF = 3 * XYF + 6 * ZF, QPL = C0Q + 2 * C1Q;
  const int W = a.vm[0].W[PLANE], H = a.vm[0].H[PLANE];
  const unsigned cmask = (1u << a.kb) - 1u;
  const int E = a.slice_steps * SPT;   // entries per slice
  for (int sl = blockIdx.x; (long)sl * E < count; sl += gridDim.x) {
    __syncthreads();   // (first pass: the zero fill; later: the previous slice's flush has read s_geo)
    const int e_lo = sl * E, e_hi = min(e_lo + E, count);
    if (threadIdx.x == 0) {   // the slice's windows, one per stride level (PlaneTile), anchored at its first (= smallest) cell
      const int cell = (int)(a.keys[e_lo] & cmask), r = cell / a.Wk, kx = cell - r * a.Wk;
      const int ix_lo = kx - 2, ix_hi = min(kx + a.tw, a.Wk) - 3, iy = r - 2;
      int off = 0;
      for (int lv = 0; lv < 3; ++lv) {
        const int st = 1 << lv, Ws = (W + st - 1) >> lv, Hs = (H + st - 1) >> lv;
        int x0, x1, y0, y1;
        if (lv == 0) {
          x0 = max(ix_lo, 0); x1 = min(ix_hi + 1, Ws - 1); y0 = max(iy, 0); y1 = min(iy + 1, Hs - 1);
        } else {   // f_lv = f_0 (Ws - 1) / (W - 1): the taps of f_0 in [i, j + 1) are floor(i rho) .. floor((j + 1) rho) + 1
          const float rx = W > 1 ? (float)(Ws - 1) / (float)(W - 1) : 0.f, ry = H > 1 ? (float)(Hs - 1) / (float)(H - 1) : 0.f;
          x0 = max((int)floorf((float)ix_lo * rx), 0); x1 = min((int)floorf((float)(ix_hi + 1) * rx) + 1, Ws - 1);
          y0 = max((int)floorf((float)iy * ry), 0); y1 = min((int)floorf((float)(iy + 1) * ry) + 1, Hs - 1);
        }
        const int nxcap = lv == 0 ? a.tw + 1 : (a.tw >> lv) + 3, nycap = lv == 0 ? 2 : 3;
        const int nx = min(max(x1 - x0 + 1, 0), nxcap), ny = min(max(y1 - y0 + 1, 0), nycap);
        s_geo[lv * 8 + 0] = x0; s_geo[lv * 8 + 1] = y0; s_geo[lv * 8 + 2] = nx; s_geo[lv * 8 + 3] = ny; s_geo[lv * 8 + 4] = off;
        off += nx * ny * CT;
      }
    }
    __syncthreads();
    for (int t = wave; t * SPT < e_hi - e_lo; t += nwaves) {
      const int pos = e_lo + t * SPT + (PLANE == 0 ? s16 : s);
      const bool live = pos < e_hi;
      const int ent = live ? (int)(a.order[pos] - a.base) : 0;
      const int idx = a.list ? a.list[ent] : ent;
      const float x0 = a.xw[(size_t)idx * 3 + 0], x1 = a.xw[(size_t)idx * 3 + 1], x2 = a.xw[(size_t)idx * 3 + 2];
      float dw0 = 0.f, dw1 = 0.f, dw2 = 0.f;
#pragma unroll 1
      for (int set = 0; set < 2; ++set) {
        if (!((a.set_mask >> set) & 1)) continue;
        const int first = set ? nl0 : 0;
        const LdsLines ll = LdsLines{lacc, {first, first, first}, 1, a.line_direct};
        const int tslot = set == 1 && (a.set_mask & 1) ? 1 : 0;   // windows are allocated for the live sets only
        const PlaneTile T = PlaneTile{lacc + 2 * (nl0 + nl1 + tslot * tile_elems), s_geo, CT};
        const float* rec = a.dfs + (size_t)ent * a.rec_floats + set * SETF;
#pragma unroll 1
        for (int lv = 0; lv < 3; ++lv) {
          if constexpr (PLANE == 0) {
#pragma unroll 1
            for (int grp = 0; grp < C0Q / 4; ++grp) {
              const f32x4 dq = live ? ld4(rec + lv * XYF + grp * 16 + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
              gather_xy4_bwd<C0Q, C1Q, true>(a.vm[set], a.gvm[set], lv, 4 * grp + q, x0, x1, x2, dq, live, q == 0, dw0, dw1, dw2, ll, T);
            }
          } else {
#pragma unroll 1
            for (int zq = 0; zq < C1Q; ++zq) {
              const f32x4 dq = live ? ld4(rec + 3 * XYF + (PLANE - 1) * 3 * ZF + lv * ZF + 4 * zq) : f32x4{0.f, 0.f, 0.f, 0.f};
              gather_zquad_bwd<C0Q, C1Q, true>(a.vm[set], a.gvm[set], lv * QPL + C0Q + (PLANE - 1) * C1Q + zq, h, x0, x1, x2, dq, live, s,
                                               dw0, dw1, dw2, ll, T);
            }
          }
        }
      }
      if constexpr (PLANE != 0) {
        dw0 += __shfl_xor(dw0, 32, 64); dw1 += __shfl_xor(dw1, 32, 64); dw2 += __shfl_xor(dw2, 32, 64);
      }
      if (live && (PLANE == 0 ? q == 0 : h == 0)) {
        float* d = a.dxw + (size_t)idx * 3;
        d[0] += dw0; d[1] += dw1; d[2] += dw2;
      }
    }
    __syncthreads();
    // flush the windows: component fastest, so 16 consecutive lanes cover one 64-byte texel (one request); the slots are
    // left zeroed for the next chunk
#pragma unroll 1
    for (int set = 0; set < 2; ++set) {
      if (!((a.set_mask >> set) & 1)) continue;
      double* tile = reinterpret_cast<double*>(lacc) + nl0 + nl1 + (set == 1 && (a.set_mask & 1) ? 1 : 0) * tile_elems;
      float* GP = a.gvm[set].plane[PLANE];
      const int sH = a.vm[set].sH[PLANE], sW = a.vm[set].sW[PLANE];
      for (int lv = 0; lv < 3; ++lv) {
        const int gx0 = s_geo[lv * 8 + 0], gy0 = s_geo[lv * 8 + 1], nx = s_geo[lv * 8 + 2], ny = s_geo[lv * 8 + 3], off = s_geo[lv * 8 + 4];
        const int n = nx * ny * CT;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
          const double v = tile[off + i];
          if (v != 0.0) {
            tile[off + i] = 0.0;
            const int t = i / CT, cc = i - t * CT, ty = t / nx, tx = t - ty * nx;
            grad_add(GP + (size_t)(((gy0 + ty) << lv) * sH + ((gx0 + tx) << lv) * sW) + cc, (float)v);
          }
        }
      }
    }
  }
  __syncthreads();
  if (a.set_mask & 1) flush_lds_line(lacc, 1, 0, a.vm[0].L[PLANE], a.vm[0].C[PLANE], a.gvm[0].line[PLANE]);
  if (a.set_mask & 2) flush_lds_line(lacc, 1, nl0, a.vm[1].L[PLANE], a.vm[1].C[PLANE], a.gvm[1].line[PLANE]);
}

// the launch decisions of the most recent scatter of the calling host thread (ScatterRecord, rdrf_bwd_host.hpp): thread_local,
// so that backward passes running on several host threads do not write one struct
static thread_local ScatterRecord g_last_scatter;
const ScatterRecord& scatter_last_record() { return g_last_scatter; }
static void record_begin(int form) {
  memset(&g_last_scatter, 0, sizeof(g_last_scatter));
  g_last_scatter.form = form;
}
static void record_launch(int elem_bytes, int threads, long workgroups, int tiled, int tw, int slice_steps) {
  if (g_last_scatter.n >= 4) return;
  g_last_scatter.l[g_last_scatter.n++] = ScatterLaunch{elem_bytes, threads, (int)workgroups, tiled, tw, slice_steps};
}

void fill_scatter_common(ScatterArgs& sa, const BwdArgs& a) {
  memset(&sa, 0, sizeof(sa));
  sa.xyz = a.xyz; sa.box = a.box; sa.valid = a.valid; sa.N = a.N; sa.S = a.S;
}
static int lines_floats_host(const RdrfVM& vm) {
  int n = 0;
  for (int i = 0; i < 3; ++i) n += vm.L[i] * (vm.C[i] + 4);   // lds_stride(C) = C + 4
  return n;
}
// LDS line accumulators when both factor sets' lines fit SC_LINES_MAX_BYTES; launches with that much
// dynamic LDS (the attribute call is needed above 64 KB and is idempotent)
template <typename K>
static int launch_scatter_k(const char* name, K kern, ScatterArgs& sa, long ntiles, hipStream_t stream) {
  const long n0 = lines_floats_host(sa.vm[0]), n1 = sa.nsets > 1 ? lines_floats_host(sa.vm[1]) : 0;
  // element type of the accumulators: doubles when they fit (ds_add_f64 retires 11 x the updates of ds_add_f32, see
  // LdsLines), also at the price of one launch per factor set; floats for lines too long for that; else global atomics
  int esz = 0;
  bool split = false;
  for (int e = 8; e >= 4 && !esz; e -= 4) {
    if (e * (n0 + n1) <= SC_LINES_MAX_BYTES) esz = e;
    else if (sa.nsets == 2 && e * n0 <= SC_LINES_MAX_BYTES && e * n1 <= SC_LINES_MAX_BYTES) { esz = e; split = true; }
  }
#ifdef RDRF_DETERMINISTIC
  esz = 0;   // the LDS accumulators add in wave-arrival order: the line gradients go straight to the fixed-point shadow
  split = false;
#endif
  if (split) {
    // the two factor sets do not fit the LDS together but each does alone: one launch per set
    ScatterArgs s0 = sa, s1 = sa;
    s0.nsets = 1;
    s1.nsets = 1;
    s1.vm[0] = sa.vm[1]; s1.gvm[0] = sa.gvm[1]; s1.row0[0] = sa.row0[1];
    s1.dxw_accumulate = 1;
    g_last_scatter.split = 1;
    int rc = launch_scatter_k(name, kern, s0, ntiles, stream);
    return rc ? rc : launch_scatter_k(name, kern, s1, ntiles, stream);
  }
  sa.lds_bytes = (int)(esz * (n0 + n1));
  sa.lds_f64 = esz == 8;
  if (sa.lds_bytes > 48 * 1024)
    RDRF_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SC_LINES_MAX_BYTES));
  // workgroups per CU that the accumulators leave room for (160 KB of LDS): one big workgroup, or two / three of 256
  // threads; the grid never exceeds what is resident at once (the tile loop is a static stride: a workgroup that starts
  // after the others have finished would run its share alone)
  const int per_cu = sa.lds_bytes > 80 * 1024 ? 1 : (sa.lds_bytes > 53 * 1024 ? 2 : 3);
  const int threads = per_cu == 1 ? 512 : 256;
  const int wpb = threads / 64;
  long g = (ntiles + wpb - 1) / wpb;
  const long cap = 256 * per_cu;
  g = g < 1 ? 1 : (g > cap ? cap : g);
  record_launch(esz, threads, g, -1, 0, 0);
  rdrf_prof_begin(name, stream);
  hipLaunchKernelGGL(kern, dim3((unsigned)g), dim3(threads), (size_t)sa.lds_bytes, stream, sa);
  rdrf_prof_end(name, stream);
  RDRF_HIP(hipGetLastError());
  return 0;
}
int launch_scatter(const char* name, ScatterKernel kern, ScatterArgs& sa, long ntiles, hipStream_t stream) {
  record_begin(0);
  switch (kern) {
    case SCATTER_4_1_3: return launch_scatter_k(name, k_scatter<4, 1, 3>, sa, ntiles, stream);
    case SCATTER_4_1_9: return launch_scatter_k(name, k_scatter<4, 1, 9>, sa, ntiles, stream);
    case SCATTER_12_3_9: return launch_scatter_k(name, k_scatter<12, 3, 9>, sa, ntiles, stream);
    case SCATTER_12_3_27: return launch_scatter_k(name, k_scatter<12, 3, 27>, sa, ntiles, stream);
  }
  rdrf_set_error("launch_scatter: unknown kernel %d", (int)kern);
  return -1;
}

// rdrf_set_scatter_mode(RDRF_SCATTER_AUTO (default) | _RAY | _SORTED): how the density / blending gradients of the dynamic
// field's ray path reach the factor planes -- the ray-tile kernel (k_scatter), or samples grouped by plane cell first
// (k_scatter_sorted: ~10x fewer memory-side atomic requests).  Measured on MI355X at the Balloon1 stage-0 shape (DESIGN.md
// 9): the grouping is a fixed cost per launch, the saving grows with the batch.  Kept selectable: sorted is the only path
// whose request count does not depend on the warp field's smoothness, and the parity tests run both at every size.
static int g_scatter_mode = RDRF_SCATTER_AUTO;
extern "C" int rdrf_set_scatter_mode(int mode) {
  RDRF_CHECK(mode == RDRF_SCATTER_AUTO || mode == RDRF_SCATTER_RAY || mode == RDRF_SCATTER_SORTED || mode == RDRF_SCATTER_SORTED_PLAIN, -1,
             "rdrf_set_scatter_mode: mode must be RDRF_SCATTER_AUTO, _RAY, _SORTED or _SORTED_PLAIN");
  g_scatter_mode = mode;
  return 0;
}
int scatter_mode_swap(int mode) {
  const int old = g_scatter_mode;
  g_scatter_mode = mode;
  return old;
}
int scatter_mode(size_t ns, hipStream_t stream) {   // 0 ray, 1 sorted
  int m = g_scatter_mode;
  // auto: with the hand-written radix sort (72 us for 1.4 M keys; rocPRIM took 150) the sorted path wins from the
  // Balloon1 stage-0 pass (4096 x 115 = 471 k samples: 12.57 vs 12.72 ms/step, interleaved A/B on one box) upwards, and
  // sends a tenth of the atomic requests; below ~300 k samples the fixed cost of its seven extra launches dominates
  // A launch sequence that is being CAPTURED into a HIP graph pays no per-launch host cost at replay, so the grouping wins at
  // every size there: at the S = 13 stages of Nvidia_no_poses.txt / DAVIS.txt (53 k - 106 k samples per pass into a 17 x 19 x 11 /
  // 16^3 grid: every plane fits one LDS window) the captured iteration runs 5.44 -> 5.11 / 9.31 -> 8.93 ms
  // (profiles/r06_graph_scatter_ab.txt).
  if (m == RDRF_SCATTER_AUTO) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) return 1;
    return ns >= (size_t)300000 ? 1 : 0;
  }
  return (m == RDRF_SCATTER_SORTED || m == RDRF_SCATTER_SORTED_PLAIN) ? 1 : 0;
}

template <int PLANE, int C0Q, int C1Q>
static int launch_scatter_sorted(SortedScatterArgs& sa, long max_samples, hipStream_t stream, int tiled_state = -1) {
  // pass PLANE accumulates line PLANE only: L x (C + 4) elements per factor set, doubles when they fit (see LdsLines)
  const long n = ((sa.set_mask & 1) ? (long)sa.vm[0].L[PLANE] * (sa.vm[0].C[PLANE] + 4) : 0) +
                 ((sa.set_mask & 2) ? (long)sa.vm[1].L[PLANE] * (sa.vm[1].C[PLANE] + 4) : 0);
  const int esz = 8 * n <= SC_LINES_MAX_BYTES ? 8 : (4 * n <= SC_LINES_MAX_BYTES ? 4 : 0);
  sa.lds_bytes = (int)(esz * n);
  sa.lds_f64 = esz == 8;
  sa.line_direct = sa.lds_f64;   // measured: -0.1 ms / step on top of the double accumulators (profiles/r05_ab_lds_f64.txt)
#ifdef RDRF_DETERMINISTIC
  sa.lds_bytes = 0;
#endif
  if (sa.lds_bytes > 48 * 1024)
    RDRF_HIP(hipFuncSetAttribute((const void*)k_scatter_sorted<PLANE, C0Q, C1Q>, hipFuncAttributeMaxDynamicSharedMemorySize, SC_LINES_MAX_BYTES));
  // 512 threads x 2 workgroups per CU = 4 waves per SIMD (the kernels need <= 116 VGPRs): 12.16 -> 11.98 ms / step against
  // 256 x 3 (profiles/r05_ab_sorted_occupancy.txt); one workgroup per CU when the accumulators take more than half the LDS
  const int per_cu = sa.lds_bytes > 80 * 1024 ? 1 : 2;
  const int threads = 512;
  const int wpb = threads / 64;
  const long ntiles = (max_samples + (PLANE == 0 ? 15 : 31)) / (PLANE == 0 ? 16 : 32);
  long g = (ntiles + wpb - 1) / wpb;
  const long cap = 256 * per_cu;
  g = g < 1 ? 1 : (g > cap ? cap : g);
  static const char* names[3] = {"scatter_sorted_xy", "scatter_sorted_xz", "scatter_sorted_yz"};
  record_launch(sa.lds_bytes > 0 ? esz : 0, threads, g, tiled_state, 0, 0);
  rdrf_prof_begin(names[PLANE], stream);
  hipLaunchKernelGGL((k_scatter_sorted<PLANE, C0Q, C1Q>), dim3((unsigned)g), dim3(threads), (size_t)sa.lds_bytes, stream, sa);
  rdrf_prof_end(names[PLANE], stream);
  RDRF_HIP(hipGetLastError());
  return 0;
}

// the tiled form of pass PLANE (k_scatter_tiled) when its line accumulators and plane windows fit the LDS as doubles;
// returns 1 if it was launched, 0 if the caller should take k_scatter_sorted, < 0 on error
template <int PLANE, int C0Q, int C1Q>
static int launch_scatter_tiled(SortedScatterArgs& sa, const unsigned* keys_sorted, int kb, long max_samples, hipStream_t stream) {
#ifdef RDRF_DETERMINISTIC
  return 0;   // LDS sums form in wave-arrival order
#endif
  if (g_scatter_mode == RDRF_SCATTER_SORTED_PLAIN) return 0;
  static_assert(C0Q == 4, "windows hold the 16- / 4-component texels of the density / blending sets");
  constexpr int CT = PLANE == 0 ? 4 * C0Q : 4 * C1Q;
  const int tw = 32;
  const long n0 = (sa.set_mask & 1) ? (long)sa.vm[0].L[PLANE] * (sa.vm[0].C[PLANE] + 4) : 0;
  const long n1 = (sa.set_mask & 2) ? (long)sa.vm[1].L[PLANE] * (sa.vm[1].C[PLANE] + 4) : 0;
  const long n = n0 + n1;
  sa.tile_sets = sa.set_mask == 3 ? 2 : 1;
  const long bytes = 8L * (n + (long)sa.tile_sets * tile_texels(tw) * CT);
  // only where two 512-thread workgroups per CU still fit (at the final grids the z lines of two factor sets alone take
  // 70 KB: one workgroup per CU lost more than the windows gained, 3.46 -> 3.97 ms) and for the 16- / 4-component texels
  // of the density / blending sets (the 48-component appearance windows gained nothing: 0.71 -> 0.71 ms)
  // two workgroups per CU: each needs its dynamic bytes + the kernel's static LDS (s_geo: 96 B), rounded to the 512-byte
  // allocation granule (at exactly 80 KB of dynamic LDS the second workgroup did not fit)
  const long per_wg = ((bytes + 96 + 511) / 512) * 512;
  // where both factor sets together leave no room for two workgroups per CU the caller falls back: one tiled launch per set
  // was measured and LOSES to the untiled two-set kernel (final stage, scatter_dyn_density 3.08 -> 3.24 ms / step,
  // profiles/r05_ab_tiled_scatter.txt: every entry's taps and run structure are formed twice)
  if (per_wg > 80 * 1024) return 0;
  sa.lds_bytes = (int)bytes; sa.lds_f64 = 1;
  sa.line_direct = 1;
  sa.keys = keys_sorted; sa.kb = kb; sa.tw = tw;
  sa.slice_steps = 16;   // 2 steps for each of the 8 waves (16: 1.51, 32: 1.55, 64: 1.68 ms / step)
  sa.Wk = sa.vm[0].W[PLANE] + 3;
  if (sa.lds_bytes > 48 * 1024)
    RDRF_HIP(hipFuncSetAttribute((const void*)k_scatter_tiled<PLANE, C0Q, C1Q>, hipFuncAttributeMaxDynamicSharedMemorySize, SC_LINES_MAX_BYTES));
  const int per_cu = 2;   // 512-thread workgroups, 4 waves per SIMD (__launch_bounds__(512, 4): HIP counts waves per SIMD)
  const long nslices = (max_samples + (long)sa.slice_steps * (PLANE == 0 ? 16 : 32) - 1) / ((long)sa.slice_steps * (PLANE == 0 ? 16 : 32));
  long g = nslices < 256L * per_cu ? nslices : 256L * per_cu;
  g = g < 1 ? 1 : g;
  static const char* names[3] = {"scatter_tiled_xy", "scatter_tiled_xz", "scatter_tiled_yz"};
  record_launch(8, 512, g, 1, tw, sa.slice_steps);
  rdrf_prof_begin(names[PLANE], stream);
  hipLaunchKernelGGL((k_scatter_tiled<PLANE, C0Q, C1Q>), dim3((unsigned)g), dim3(512), (size_t)sa.lds_bytes, stream, sa);
  rdrf_prof_end(names[PLANE], stream);
  RDRF_HIP(hipGetLastError());
  return 1;
}

int sorted_key_bits(const int W[3], const int H[3]) {
  long maxcells = 0;
  for (int p = 0; p < 3; ++p) {
    const long c = (long)(W[p] + 3) * (H[p] + 3);
    maxcells = c > maxcells ? c : maxcells;
  }
  int kb = 1;
  while (((1L << kb) - 1) < maxcells) ++kb;
  return kb;
}

// keys of the entries (all samples, or the compacted list), stable sort by (plane | cell), live counts per plane
static int sorted_scatter_prepare(SortKeyArgs& ka, const RdrfVM& vm, const BwdArgs& a, const BwdWs& b, hipStream_t stream) {
  const size_t ns = (size_t)a.N * a.S;
  ka.xw = a.sp.xw; ka.valid = a.valid; ka.N = a.N; ka.S = a.S;
  for (int p = 0; p < 3; ++p) { ka.W[p] = vm.W[p]; ka.H[p] = vm.H[p]; }
  const int kb = sorted_key_bits(ka.W, ka.H);
  RDRF_CHECK(kb <= 29, -1, "sorted scatter: plane too large for 32-bit keys");
  ka.kb = kb; ka.keys = b.keys_in; ka.counts = b.counts;
  // the keys of plane p are segment p of the key arrays and carry p above their kb cell bits: three independent sorts
  // over kb bits give what one sort over kb + 2 bits gave.  The key kernel owns the sort's tiles and builds its first
  // histograms and the drop counts behind counts[]
  RsTables T;
  int rc = rdrf_sort_tables(3, (unsigned)ns, kb, b.sort_tmp, b.sort_tmp_bytes, &T, &ka.nbins);
  if (rc) return rc;
  ka.hist = T.hist; ka.drops = T.drops; ka.tps = T.tps;
  rdrf_prof_begin("scatter_sort", stream);
  rdrf_prof_begin("sort_keys", stream);
  hipLaunchKernelGGL(k_sort_keys, dim3(T.tps), dim3(SK_THREADS), 0, stream, ka);
  rdrf_prof_end("sort_keys", stream);
  // compact: the sort covers the 3 x *count live-list entries only (launches sized for 3 N S; the appearance list holds
  // 35-60 % of the samples)
  rc = rdrf_sort_positions_seg(b.keys_in, b.keys_out, b.order, 3, (unsigned)ns, kb, b.sort_tmp, b.sort_tmp_bytes, stream,
                               ka.compact ? ka.count : nullptr, b.counts);
  rdrf_prof_end("scatter_sort", stream);
  if (rc) return rc;
  RDRF_HIP(hipGetLastError());
  return 0;
}

// appearance scatter of the dynamic field's ray path with the compacted samples grouped by plane cell: the same
// per-quad device functions as the ray-tile kernel (k_scatter<12, 3, 27>), whose 18 M memory-side atomic requests per
// launch (runs of 1-2 samples along a ray) were the largest share of the step's requests
int scatter_dyn_app_sorted(const BwdArgs& a, const BwdWs& b, const RdrfDynamicParams* P, const RdrfDynamicParams* G,
                           hipStream_t stream) {
  const size_t ns = (size_t)a.N * a.S;
  record_begin(1);
  SortKeyArgs ka;
  memset(&ka, 0, sizeof(ka));
  ka.list = a.sp.list; ka.count = &a.sp.hdr->count;
  ka.compact = 1;
  int rc = sorted_scatter_prepare(ka, P->app, a, b, stream);
  if (rc) return rc;
  SortedScatterArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.vm[0] = P->app; sa.gvm[0] = G->app;
  sa.set_mask = 1; sa.dfs = b.dfa; sa.rec_floats = DFA_FLOATS; sa.list = a.sp.list; sa.xw = a.sp.xw; sa.dxw = b.dxw;
  for (int p = 0; p < 3; ++p) {
    sa.order = b.order + (size_t)p * ns; sa.count = b.counts + p; sa.base = (unsigned)(p * ns);
    if (ka.compact) { sa.order = b.order; sa.seg = ka.count; }   // device-side segment starts (k_scatter_sorted)
    // (no windows here: for the 48-component texels they gained nothing, 0.713 -> 0.695 ms, profiles/r05_ab_tiled_scatter.txt)
    rc = p == 0 ? launch_scatter_sorted<0, 12, 3>(sa, (long)ns, stream)
                : (p == 1 ? launch_scatter_sorted<1, 12, 3>(sa, (long)ns, stream) : launch_scatter_sorted<2, 12, 3>(sa, (long)ns, stream));
    if (rc) return rc;
  }
  return 0;
}

// density / blending scatter of the dynamic field's ray path, samples grouped by plane cell (see k_scatter_sorted)
int scatter_dyn_density_sorted(const BwdArgs& a, const BwdWs& b, const RdrfDynamicParams* P, const RdrfDynamicParams* G,
                               int set_mask, hipStream_t stream) {
  const size_t ns = (size_t)a.N * a.S;
  for (int p = 0; p < 3; ++p)
    RDRF_CHECK(P->blending.W[p] == P->density.W[p] && P->blending.H[p] == P->density.H[p], -1,
               "sorted scatter: density and blending planes differ in size");
  record_begin(1);
  SortKeyArgs ka;
  memset(&ka, 0, sizeof(ka));
  ka.grows1 = b.grows1;
  ka.flat = rdrf_flat_density() ? 1 : 0;
  int rc = sorted_scatter_prepare(ka, P->density, a, b, stream);
  if (rc) return rc;
  SortedScatterArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.vm[0] = P->density; sa.gvm[0] = G->density; sa.vm[1] = P->blending; sa.gvm[1] = G->blending;
  sa.set_mask = set_mask; sa.dfs = b.dfs; sa.rec_floats = DFS_FLOATS; sa.xw = a.sp.xw; sa.dxw = b.dxw;
  // what a pass that runs k_scatter_sorted records: 0 = the launch policy refused the windows, -2 = windows switched off
  // (RDRF_SCATTER_SORTED_PLAIN, the deterministic build)
#ifdef RDRF_DETERMINISTIC
  const int why = -2;
#else
  const int why = g_scatter_mode == RDRF_SCATTER_SORTED_PLAIN ? -2 : 0;
#endif
  for (int p = 0; p < 3; ++p) {
    sa.order = b.order + (size_t)p * ns; sa.count = b.counts + p; sa.base = (unsigned)(p * ns);
    const unsigned* ks = b.keys_out + (size_t)p * ns;
    rc = p == 0 ? launch_scatter_tiled<0, 4, 1>(sa, ks, ka.kb, (long)ns, stream)
                : (p == 1 ? launch_scatter_tiled<1, 4, 1>(sa, ks, ka.kb, (long)ns, stream)
                          : launch_scatter_tiled<2, 4, 1>(sa, ks, ka.kb, (long)ns, stream));
    if (rc < 0) return rc;
    if (rc == 1) continue;
    rc = p == 0 ? launch_scatter_sorted<0, 4, 1>(sa, (long)ns, stream, why)
                : (p == 1 ? launch_scatter_sorted<1, 4, 1>(sa, (long)ns, stream, why) : launch_scatter_sorted<2, 4, 1>(sa, (long)ns, stream, why));
    if (rc) return rc;
  }
  return 0;
}
