// rdrf_bwd_dev.hpp -- device-side pieces shared by the backward-data kernels (rdrf_bwd.hip, rdrf_bwd_fused.hip) and the
// gradient-scatter kernels (rdrf_scatter.hip): the backward LDS images, the argument block of the backward kernels, the
// small-layer / reduce-scatter helpers of the backward-data kernels, the sample-major d(feature) records, and the VM gather
// backward per quad (run reduction in DPP, LDS line accumulators, plane windows).
#pragma once
#include "rdrf_kernels.hpp"

// ------------------------------------------------------------------------------------------------
// backward LDS images (transposed packs + small layers), float offsets inside each region
// ------------------------------------------------------------------------------------------------
namespace pkb {
// dynamic density phase, heads kernel image
constexpr int K1H_DEN2 = 0;                           // small 1 x [2][32]
constexpr int K1H_BLE2 = K1H_DEN2 + 64;
#ifdef RDRF_HEADS_BWD_F32   // A/B builds: the transposed first layers of the heads on the fp32 matrix pipe
constexpr int K1H_DEN1T_F = K1H_BLE2 + 64;            // NBI 3 x KK 32
constexpr int K1H_DEN1T_X0 = K1H_DEN1T_F + 3 * 32 * 64;
constexpr int K1H_BLE1T_F = K1H_DEN1T_X0 + 2 * 32 * 64;
constexpr int K1H_BLE1T_X0 = K1H_BLE1T_F + 3 * 32 * 64;
constexpr int K1H_SIZE = K1H_BLE1T_X0 + 2 * 32 * 64;
#else                       // bf16 x 3 fragments (mfma_seg_b3_pair): 96 dwords per block and slot
constexpr int K1H_DEN1T_F = K1H_BLE2 + 64;            // NBI 3 x KK 32
constexpr int K1H_DEN1T_X0 = K1H_DEN1T_F + 3 * 32 * 96;
constexpr int K1H_BLE1T_F = K1H_DEN1T_X0 + 2 * 32 * 96;
constexpr int K1H_BLE1T_X0 = K1H_BLE1T_F + 3 * 32 * 96;
constexpr int K1H_SIZE = K1H_BLE1T_X0 + 2 * 32 * 96;
#endif
// dynamic density phase, warp kernel image
constexpr int K1W_W5 = 0;                             // small 3 x [2][32]
#ifdef RDRF_HEADS_BWD_F32
constexpr int K1W_W4T = K1W_W5 + 3 * 64;              // NBI 2 x KK 32
constexpr int K1W_W3T_X0 = K1W_W4T + 2 * 32 * 64;     // NBI 2
constexpr int K1W_W3T_T = K1W_W3T_X0 + 2 * 32 * 64;   // NBI 1
constexpr int K1W_SIZE = K1W_W3T_T + 1 * 32 * 64;
#else                       // bf16 x 3 fragments
constexpr int K1W_W4T = K1W_W5 + 3 * 64;              // NBI 2 x KK 32
constexpr int K1W_W3T_X0 = K1W_W4T + 2 * 32 * 96;     // NBI 2
constexpr int K1W_W3T_T = K1W_W3T_X0 + 2 * 32 * 96;   // NBI 1
constexpr int K1W_SIZE = K1W_W3T_T + 1 * 32 * 96;
#endif
// dynamic appearance phase
constexpr int K3_RGBV = 0;                        // small 3 x [2][64]
constexpr int K3_RGB2T = K3_RGBV + 3 * 128;       // NBI 4 x KK 64
constexpr int K3_RGB1T_F = K3_RGB2T + 4 * 64 * 64;   // NBI 1
constexpr int K3_RGB1T_X0 = K3_RGB1T_F + 1 * 64 * 64;  // NBI 2
constexpr int K3_BASIST = K3_RGB1T_X0 + 2 * 64 * 64;  // NBI 7 x KK 16
constexpr int K3_SIZE = K3_BASIST + 7 * 16 * 64;
// static appearance phase
constexpr int S3_W3 = 0;                          // small 3 x [2][64]
constexpr int S3_W2T = S3_W3 + 3 * 128;           // NBI 4 x 64
constexpr int S3_W1T_F = S3_W2T + 4 * 64 * 64;    // NBI 1
constexpr int S3_W1T_P = S3_W1T_F + 1 * 64 * 64;  // NBI 4
constexpr int S3_BASIST = S3_W1T_P + 4 * 64 * 64; // NBI 3 x KK 16
constexpr int S3_SIZE = S3_BASIST + 3 * 16 * 64;
// scene flow
constexpr int SF_W6 = 0;                          // small 6 x [2][32]
constexpr int SF_W4T = SF_W6 + 6 * 64;
constexpr int SF_W2T = SF_W4T + 2 * 32 * 64;
constexpr int SF_W0T = SF_W2T + 2 * 32 * 64;      // NBI 2 (40 -> 64)
constexpr int SF_SIZE = SF_W0T + 2 * 32 * 64;
constexpr int REG_K1H = 0, REG_K1W = REG_K1H + K1H_SIZE, REG_K3 = REG_K1W + K1W_SIZE,
              REG_SF = REG_K3 + K3_SIZE, REG_DYN_END = REG_SF + SF_SIZE;
constexpr int REG_S3 = 0, REG_STAT_END = S3_SIZE;
// lo pieces of the appearance backward kernels' bf16 x 3 layers with split storage (mfma_seg_b3s): streamed, never in LDS
constexpr int K3_LO_RGB2T = 0;                                // 4 x 64 slots
constexpr int K3_LO_RGB1T = K3_LO_RGB2T + 4 * 64 * 32;        // (1 + 2) x 64: the F block, then the two X0 blocks
constexpr int K3_LO_BASIST = K3_LO_RGB1T + 3 * 64 * 32;       // 7 x 16
constexpr int K3_LO_SIZE = K3_LO_BASIST + 7 * 16 * 32;
constexpr int S3_LO_W2T = 0;                                  // 4 x 64
constexpr int S3_LO_W1T = S3_LO_W2T + 4 * 64 * 32;            // (1 + 4) x 64: the F block, then the four PE blocks
constexpr int S3_LO_BASIST = S3_LO_W1T + 5 * 64 * 32;         // 3 x 16
constexpr int S3_LO_SIZE = S3_LO_BASIST + 3 * 16 * 32;
constexpr int REG_K3_LO = REG_DYN_END, REG_S3_LO = REG_STAT_END;
static_assert(K3_RGB1T_X0 == K3_RGB1T_F + 64 * 64 && S3_W1T_P == S3_W1T_F + 64 * 64, "layer-1 blocks form one image");
static_assert(K1H_SIZE * 4 <= 160 * 1024 && K3_SIZE * 4 <= 160 * 1024 && S3_SIZE * 4 <= 160 * 1024,
              "backward weight images must fit the LDS");
}  // namespace pkb

// ------------------------------------------------------------------------------------------------
// argument block of the backward kernels
// ------------------------------------------------------------------------------------------------

// sample-major d(feature) record of the sorted scatter: per factor set 72 floats ordered
// [XY: level 0 (16) | level 1 (16) | level 2 (16)] [XZ: 3 x 4] [YZ: 3 x 4]  (each XY level block is one 64-byte line)
#define DFS_FLOATS 144
RDRF_HD constexpr int dfs_off(int Q) {   // feature quad Q = 6 level + w  (w < 4: XY quad w, 4: XZ, 5: YZ)
  return (Q % 6) < 4 ? (Q / 6) * 16 + 4 * (Q % 6) : ((Q % 6) == 4 ? 48 + 4 * (Q / 6) : 60 + 4 * (Q / 6));
}

// sample-major d(feature) record of the SORTED APPEARANCE scatter: 216 floats per compacted sample, ordered
// [XY: level 0 (48) | level 1 (48) | level 2 (48)] [XZ: 3 x 12] [YZ: 3 x 12]  (an XY level block = three 64-byte lines)
#define DFA_FLOATS 216
RDRF_HD constexpr int dfa_off(int Q) {   // feature quad Q = 18 level + w  (w < 12: XY quad w, 12..14: XZ, 15..17: YZ)
  return (Q % 18) < 12 ? (Q / 18) * 48 + 4 * (Q % 18)
                       : ((Q % 18) < 15 ? 144 + 12 * (Q / 18) + 4 * ((Q % 18) - 12) : 180 + 12 * (Q / 18) + 4 * ((Q % 18) - 15));
}

struct BwdArgs {
  const float* rays;
  const float* ts;
  const float* xyz;
  const float* z;
  const uint8_t* valid;
  int N, S;
  Box box;
  float distance_scale, weight_thres, density_shift;
  int act, ray_type, static_head;
  // upstream gradients (nullable)
  const float *g_rgb, *g_sigma, *g_weight, *g_dists, *g_blending, *g_xyz_prime;
  // saved by the forward
  SavedPtrs sp;
  // packed weights (global) and gradient rows (workspace)
  const float* pk;
  float* grows1;   // density-phase dz rows
  float* grows3;   // appearance-phase dz rows
  float* dxw_app;  // [N*S*3] coordinate grads arriving from the appearance phase
  float* dxn_app;  // [N*S*3]
  float* dtout;    // [N*32]
  float* gsig;     // flat-tile path: total d(sigma) per sample, [N*S] (k_ray_scan_bwd)
  float* dtp;      // flat-tile path: d(tout) partial sums of the rays that cross a tile edge, [tiles][2][32] (k_time_branch_bwd sums them)
  float* dfs;      // sorted scatter: d(features) of the density / blending heads SAMPLE-major, [N*S][2][72] in the
                   // order [XY quads of level 0, 1, 2 | XZ quads | YZ quads] (nullptr: row layout for the ray-tile scatter)
  float* dfa;      // sorted appearance scatter: d(app features) per COMPACTED sample, [count][216] (dfa_off); nullptr: rows
  // outputs
  float* g_xyz;
  float* g_rays;   // [N][6] (+=): through dists (ray norm) and the static head's view directions
  float* g_z;      // [N][S] (+=): through dists = (z[j+1] - z[j]) |d| scale (nullable; no reference loss
                   // reaches it, kept for autograd completeness: models/tensorBase.py:726-731)
  // feature mode (template parameter FEAT; see FieldArgs): M points, g_sigma / g_blending carry the
  // gradients of the RAW density / blending features, g_feat [M][27] of the appearance features
  int M, in_norm;
  const float* g_feat;
  int small_dw;   // ray path: k_dyn_density_bwd forms the weight gradients of layer5 / density_layer2 / blending_layer2
  int dynq;       // 1: the compacted-tile kernels draw their tiles from the workgroup's queue (tile_queue_next)
};

struct StaticG {
  RdrfVM density, app;
  float *b3, *w3;
};
struct DynG {
  RdrfVM density, blending, app;
  float *rbv, *rwv, *l5b, *db2, *bb2;
  float *l5w, *dw2, *bw2;   // small layers of the density phase: weight gradients formed in k_dyn_density_bwd (ray path)
};

// pieces shared by the backward-data kernels (rdrf_bwd.hip) and their fused-dW forms (rdrf_bwd_fused.hip), whose flush targets
// SfGrads / WarpGrads are
struct SfGrads {
  float* w[4];   // sfw[0..3]
  float* b[4];   // sfb[0..3]
};
struct WarpGrads {
  float *l3w, *l3b, *l4w, *l4b;
};

// backward of a small output layer kept on the VALU (NO <= 6 outputs): dz[kk] = relu'(H[kk]) * sum_o W[o][kk] dzo[o]
// for this lane half's KK inputs.  ws = [NO][2][KK] in LDS, read as 16-byte quads (element-wise `lds[...]` reads
// compiled to one ds_read_b32 + lgkmcnt(0) wait per weight).
template <int KK, int NO>
RDRF_D void small_layer_bwd(float (&dz)[KK], const float (&H)[KK], const float* __restrict__ ws, int h,
                            const float (&dzo)[NO]) {
#pragma unroll
  for (int q = 0; q < KK / 4; ++q) {
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(ws + o * 2 * KK + h * KK + 4 * q);
      d.x = fmaf(wv.x, dzo[o], d.x); d.y = fmaf(wv.y, dzo[o], d.y);
      d.z = fmaf(wv.z, dzo[o], d.z); d.w = fmaf(wv.w, dzo[o], d.w);
    }
    dz[4 * q + 0] = H[4 * q + 0] > 0.f ? d.x : 0.f; dz[4 * q + 1] = H[4 * q + 1] > 0.f ? d.y : 0.f;
    dz[4 * q + 2] = H[4 * q + 2] > 0.f ? d.z : 0.f; dz[4 * q + 3] = H[4 * q + 3] > 0.f ? d.w : 0.f;
  }
}

template <int NB>
RDRF_D void acc_zero(f32x16 (&acc)[NB]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
}

// Reduce-scatter over the 32 lanes of a half-wave: on return lane s holds the sum over the half's 32 lanes of p[s]
// (five butterfly stages: 31 lane exchanges + 31 adds).  Used for the weight gradients of the 3- and 1-row layers of the
// density phase (layer5, density / blending layer2): dW[e] = sum over the tile's samples of dz(sample) * in_e(sample),
// with dz a per-lane scalar and in_e the 32 slots the lane already holds -- as MFMA products of the dW kernel these were 6 of
// the 40 per tile, each 27/32 empty.  ALL lanes of the wave must call.
RDRF_D float reduce_scatter32(const float (&p)[32], int s) {
  const bool b4 = s & 16, b3 = s & 8, b2 = s & 4, b1 = s & 2, b0 = s & 1;
  float q[16], r[8], t[4], u[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) q[i] = (b4 ? p[i + 16] : p[i]) + __shfl_xor(b4 ? p[i] : p[i + 16], 16, 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = (b3 ? q[i + 8] : q[i]) + __shfl_xor(b3 ? q[i] : q[i + 8], 8, 64);
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = (b2 ? r[i + 4] : r[i]) + __shfl_xor(b2 ? r[i] : r[i + 4], 4, 64);
#pragma unroll
  for (int i = 0; i < 2; ++i) u[i] = (b1 ? t[i + 2] : t[i]) + __shfl_xor(b1 ? t[i] : t[i + 2], 2, 64);
  return (b0 ? u[1] : u[0]) + __shfl_xor(b0 ? u[0] : u[1], 1, 64);
}

// ------------------------------------------------------------------------------------------------
// VM gather backward for one quad: scatter into plane / line (atomics) + coordinate gradients
// ------------------------------------------------------------------------------------------------
// DPP lane movement (VALU rate, no LDS crossbar).  ctrl: quad_perm 0x00-0xFF, row_shr:n 0x110+n,
// wave_shr:1 0x138, row_bcast:15 0x142.  Lanes without a valid source read 0.
// bound_ctrl:1 makes lanes without a valid source read 0 WITHOUT a `v_mov dst, 0` preload, and lets
// LLVM's DPP combiner fold the move into the consuming v_add / v_cndmask (one VALU op per step).
template <int CTRL, int ROW_MASK = 0xF>
RDRF_D float dppf(float v) {
  if constexpr (ROW_MASK == 0xF)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
  else  // masked rows keep `old`: pass the lane's own value so that no zero has to be materialised
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK = 0xF>
RDRF_D int dppi(int v) {
  if constexpr (ROW_MASK == 0xF)
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
  else
    return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xF, false);
}

// fp32 atomics on MI355X: the L2 retires ~20 G atomic REQUESTS/s, where a request is one
// (instruction, <=64-byte line) pair -- not one lane (tools/ubench/atomics.hip: one component per
// lane per instruction 20 G updates/s; 4 adjacent lanes covering a 16-byte quad 83 G/s; 16 lanes on
// a 64-byte texel 322 G/s).  So a quad is never sent as 4 instructions x 1 component: each group of
// 4 adjacent lanes transposes its 4x4 (lane x component) block with two rounds of quad_perm
// exchanges (8 v_cndmask_dpp), so that instruction k carries, in lanes 4t..4t+3, components 0..3 of
// lane 4t+k's quad: one request per live quad.  `off` = float offset from `base` (uniform over the
// 4-lane group; 0xffffffff = nothing to add).  Must be called by ALL lanes of the wave.
template <int K>
RDRF_D void atomic_quad_k(float* base, unsigned off, float val, int c) {
  constexpr int QP = K * 0x55;  // quad_perm:[K,K,K,K]
  const unsigned o = (unsigned)dppi<QP>((int)off);
  if (__ballot(o != 0xffffffffu) == 0ull) return;
  if (o != 0xffffffffu) grad_add(base + (size_t)o + c, val);
}
RDRF_D void atomic_add4(float* p_base, size_t p_off, f32x4 v, bool ok) {
  if (__ballot(ok) == 0ull) return;
  const int lane = threadIdx.x, c = lane & 3;
  const bool a = lane & 1, b = lane & 2;
  // round 1: 2x2 blocks between lanes i and i^1   (quad_perm [1,0,3,2] = 0xB1)
  // (DPP moves are convergent: issue them for ALL lanes, select afterwards)
  const float px = dppf<0xB1>(v.x), py = dppf<0xB1>(v.y), pz = dppf<0xB1>(v.z), pw = dppf<0xB1>(v.w);
  const float n0 = a ? py : v.x, n1 = a ? v.y : px, n2 = a ? pw : v.z, n3 = a ? v.w : pz;
  // round 2: between lanes i and i^2               (quad_perm [2,3,0,1] = 0x4E)
  const float q0 = dppf<0x4E>(n0), q1 = dppf<0x4E>(n1), q2 = dppf<0x4E>(n2), q3 = dppf<0x4E>(n3);
  const float t0 = b ? q2 : n0, t1 = b ? q3 : n1, t2 = b ? n2 : q0, t3 = b ? n3 : q1;
  const unsigned off = ok ? (unsigned)p_off : 0xffffffffu;
  atomic_quad_k<0>(p_base, off, t0, c);
  atomic_quad_k<1>(p_base, off, t1, c);
  atomic_quad_k<2>(p_base, off, t2, c);
  atomic_quad_k<3>(p_base, off, t3, c);
}
RDRF_D float dot4(f32x4 a, f32x4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// Segmented run reduction over the 32 lanes of a half-wave: lanes are consecutive samples of one
// ray, so equal keys (same texel / line entry) form CONTIGUOUS runs.  After the inclusive segmented
// scan the last lane of each run holds the run's sum and is the only one that issues the atomic:
// fp32 L2 atomics sustain only ~10-20 G/s on MI355X and serialise on hot addresses, so combining
// in registers first is worth ~5 DPP steps per value.
struct Run {
  int start;   // first lane (0..31) of the maximal contiguous equal-key stretch this lane is in
  bool tail;   // this lane is the last of its run
};
RDRF_D Run run_of(int key, int s) {
  const int prev = dppi<0x138>(key);  // wave_shr:1
  const bool head = (s == 0) || (prev != key);
  const unsigned long long b = __ballot(head);
  const unsigned m = (unsigned)(b >> (32 * ((threadIdx.x & 63) >> 5)));
  Run r;
  r.start = 31 - __clz((int)(m & (0xffffffffu >> (31 - s))));
  r.tail = (s == 31) || ((m >> (s + 1)) & 1u);
  return r;
}
// inclusive segmented scan over the 32 lanes of a half-wave, entirely in DPP: four row_shr steps
// inside each 16-lane row, then lane 15's row total is added to the lanes of the next row whose
// run started at or before lane 15 (row_bcast:15, written to rows 1 and 3 only).
RDRF_D f32x4 run_scan4(f32x4 v, int start, int s) {
  const int sr = s & 15;
#define RDRF_SCAN_STEP(D)                                                                   \
  {                                                                                         \
    const float ox = dppf<0x110 + D>(v.x), oy = dppf<0x110 + D>(v.y);                       \
    const float oz = dppf<0x110 + D>(v.z), ow = dppf<0x110 + D>(v.w);                       \
    const bool take = sr >= D && s - D >= start;                                            \
    const float tx_ = v.x + ox, ty_ = v.y + oy, tz_ = v.z + oz, tw_ = v.w + ow;             \
    v.x = take ? tx_ : v.x; v.y = take ? ty_ : v.y; v.z = take ? tz_ : v.z; v.w = take ? tw_ : v.w; \
  }
  RDRF_SCAN_STEP(1)
  RDRF_SCAN_STEP(2)
  RDRF_SCAN_STEP(4)
  RDRF_SCAN_STEP(8)
#undef RDRF_SCAN_STEP
  {
    const float ox = dppf<0x142, 0xA>(v.x), oy = dppf<0x142, 0xA>(v.y);
    const float oz = dppf<0x142, 0xA>(v.z), ow = dppf<0x142, 0xA>(v.w);
    const bool take = s >= 16 && start <= 15;
    const float tx_ = v.x + ox, ty_ = v.y + oy, tz_ = v.z + oz, tw_ = v.w + ow;
    v.x = take ? tx_ : v.x; v.y = take ? ty_ : v.y; v.z = take ? tz_ : v.z; v.w = take ? tw_ : v.w;
  }
  return v;
}
RDRF_D bool nz4(f32x4 v) { return v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f; }

// MODE 0: every lane is an independent sample (compacted appearance tiles): plain atomics.
// MODE 1: lanes of a half-wave walk one ray in order: run-reduce first.  ALL lanes of the wave
//         must call (shuffles); `live` = this lane really has a gradient to scatter.
// Line gradients are tiny tensors hammered by every sample (the z line has no runs along a ray), so
// when they fit they are accumulated in LDS (ds_add_f32) by the whole workgroup and flushed to
// global memory once per block: `ll` = LDS accumulator of this factor set or nullptr.
struct LdsLines {
  float* base;   // LDS accumulator (nullptr: scatter straight to global memory); holds doubles when f64 != 0
  int off[3];    // ELEMENT offset of line 0/1/2 inside it
  int f64;       // element type of the accumulator: 1 = double (ds_add_f64), 0 = float (ds_add_f32)
  int direct;    // 1: every live lane adds its own line taps (no run reduction): the sorted passes, where the line index of
                 //    consecutive entries is random and a ds_add_f64 costs less than the DPP scan that would precede it
};
// Element type.  ds_add_f32 is the slowest LDS atomic of gfx950 by an order of magnitude (tools/micro/lds_atomic_rate.hip,
// the access pattern below, 24 waves per CU): 193 cycles per 64-lane instruction = 0.33 lane-updates per clock and CU,
// against 17.9 cycles for ds_add_f64 (3.6 / clk), 10.9 for ds_add_u64, 9.1 for ds_add_u32 and 11.6 for a plain
// ds_write_b32.  So the accumulators are DOUBLES whenever they fit (twice the LDS, 11 x the update rate, and the line
// sums of ~1e5 terms are formed in fp64 before their one conversion to fp32 at the flush); fp32 accumulators remain for
// lines too long for that (final-stage appearance lines in the ray-tile kernel).
// LDS accumulator layout: entry l of a line with C components starts at element l*(C+4): with the natural
// stride (16 floats for C=16) every entry maps to the same two banks and a z-line update (32 distinct
// entries per half-wave) serialises ~16-fold; stride 20 (and 52 for C=48) walks all eight 4-bank
// sets.  Updates use the same quad transposition as the global atomics (4 adjacent lanes = 4
// adjacent banks).
RDRF_D int lds_stride(int C) { return C + 4; }
template <int K>
RDRF_D void lds_quad_k(float* base, int f64, int addr, float val, int c) {
  constexpr int QP = K * 0x55;
  const int ad = dppi<QP>(addr);
  if (__ballot(ad >= 0) == 0ull) return;
  if (ad >= 0) {
    if (f64) __hip_atomic_fetch_add(reinterpret_cast<double*>(base) + ad + c, (double)val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else atomicAdd(base + ad + c, val);
  }
}
// all lanes of the wave must call; `addr` = ELEMENT offset of the lane's quad inside the accumulator `ll`
RDRF_D void lds_add4(const LdsLines& ll, int addr, f32x4 v, bool ok) {
  if (__ballot(ok) == 0ull) return;
  const int lane = threadIdx.x, c = lane & 3;
  const bool a = lane & 1, b = lane & 2;
  // (DPP moves are convergent: issue them for ALL lanes, select afterwards)
  const float px = dppf<0xB1>(v.x), py = dppf<0xB1>(v.y), pz = dppf<0xB1>(v.z), pw = dppf<0xB1>(v.w);
  const float n0 = a ? py : v.x, n1 = a ? v.y : px, n2 = a ? pw : v.z, n3 = a ? v.w : pz;
  const float q0 = dppf<0x4E>(n0), q1 = dppf<0x4E>(n1), q2 = dppf<0x4E>(n2), q3 = dppf<0x4E>(n3);
  const float t0 = b ? q2 : n0, t1 = b ? q3 : n1, t2 = b ? n2 : q0, t3 = b ? n3 : q1;
  const int ad = ok ? addr : -1;
  lds_quad_k<0>(ll.base, ll.f64, ad, t0, c);
  lds_quad_k<1>(ll.base, ll.f64, ad, t1, c);
  lds_quad_k<2>(ll.base, ll.f64, ad, t2, c);
  lds_quad_k<3>(ll.base, ll.f64, ad, t3, c);
}
RDRF_D int lines_floats(const RdrfVM& vm) {
  return vm.L[0] * lds_stride(vm.C[0]) + vm.L[1] * lds_stride(vm.C[1]) + vm.L[2] * lds_stride(vm.C[2]);
}
// all three lines of a factor set, starting at element `first` of the accumulator (ray-tile kernel)
RDRF_D LdsLines make_lds_lines(float* base, int first, int f64, const RdrfVM& vm) {
  LdsLines l;
  l.base = base;
  l.f64 = f64;
  l.direct = 0;
  l.off[0] = first;
  l.off[1] = first + vm.L[0] * lds_stride(vm.C[0]);
  l.off[2] = l.off[1] + vm.L[1] * lds_stride(vm.C[1]);
  return l;
}
// flush `n_entries` x C components of one line (accumulator elements first ..) into its global gradient
RDRF_D void flush_lds_line(const float* acc, int f64, int first, int L, int C, float* __restrict__ gline) {
  const int st = lds_stride(C), n = L * C;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int l = i / C, c = i - l * C;
    const float v = f64 ? (float)reinterpret_cast<const double*>(acc)[first + l * st + c] : acc[first + l * st + c];
    if (v != 0.f) grad_add(gline + i, v);
  }
}
RDRF_D void flush_lds_lines(const float* acc, int f64, int first, const RdrfVM& vm, const RdrfVM& gvm) {
  for (int li = 0; li < 3; ++li) {
    flush_lds_line(acc, f64, first, vm.L[li], vm.C[li], gvm.line[li]);
    first += vm.L[li] * lds_stride(vm.C[li]);
  }
}

// LDS tile of one factor set's gradient PLANE for the chunk of plane cells a workgroup of the tiled sorted scatter is
// working on (k_scatter_tiled): per stride level a small window [y0, y0 + ny) x [x0, x0 + nx) of that level's sub-grid,
// `C` doubles per texel.  A tap inside the window is a ds_add_f64 (18 cycles per 64-lane instruction); a tap outside it
// (entries whose key was clamped, float rounding at a window edge) takes the global atomic as before -- the window only
// decides WHERE a sum is formed, never whether.  geo (LDS, written once per chunk): [lv][0..4] = x0, y0, nx, ny, element
// offset of the level's window inside `base`.
struct PlaneTile {
  float* base;      // LDS, holds doubles (nullptr: no tile)
  const int* geo;   // LDS
  int C;
};
RDRF_D void lds_add4_f64(float* base, int addr, f32x4 v, bool ok) {
  LdsLines l;
  l.base = base; l.f64 = 1; l.direct = 0; l.off[0] = l.off[1] = l.off[2] = 0;
  lds_add4(l, addr, v, ok);
}
template <bool TILED>
RDRF_D void plane_add4(const PlaneTile& T, int lv, int ixs, int iys, int qo, float* GP, size_t goff, f32x4 v, bool ok) {
  if constexpr (!TILED) {
    atomic_add4(GP, goff, v, ok);
  } else {
    // the window of this level: five wave-uniform ints, moved to scalar registers (a VGPR copy per tap would wait for the
    // LDS atomics in front of it: lgkmcnt is in-order)
    const int* g = T.geo + lv * 8;
    const int gx0 = __builtin_amdgcn_readfirstlane(g[0]), gy0 = __builtin_amdgcn_readfirstlane(g[1]);
    const int gnx = __builtin_amdgcn_readfirstlane(g[2]), gny = __builtin_amdgcn_readfirstlane(g[3]);
    const int gof = __builtin_amdgcn_readfirstlane(g[4]);
    const int dx = ixs - gx0, dy = iys - gy0;
    const bool in = ok && (unsigned)dx < (unsigned)gnx && (unsigned)dy < (unsigned)gny;
    lds_add4_f64(T.base, gof + (dy * gnx + dx) * T.C + qo, v, in);
    atomic_add4(GP, goff, v, ok && !in);
  }
}

template <int C0Q, int C1Q, int MODE>
RDRF_D void gather_quad_bwd(const RdrfVM& vm, const RdrfVM& gvm, int g, float x0, float x1,
                            float x2, f32x4 dq, bool live, int s, float& dx0, float& dx1,
                            float& dx2, const LdsLines ll = LdsLines{nullptr, {0, 0, 0}, 0, 0}) {
  QuadSel<C0Q, C1Q> sl = quad_sel<C0Q, C1Q>(g);
  const int pi = sl.pi;
  const float cx = pi == 2 ? x1 : x0;
  const float cy = pi == 0 ? x1 : x2;
  const float cl = pi == 0 ? x2 : (pi == 1 ? x1 : x0);
  const float* P = pi == 0 ? vm.plane[0] : (pi == 1 ? vm.plane[1] : vm.plane[2]);
  const float* Lp = pi == 0 ? vm.line[0] : (pi == 1 ? vm.line[1] : vm.line[2]);
  float* GP = pi == 0 ? gvm.plane[0] : (pi == 1 ? gvm.plane[1] : gvm.plane[2]);
  float* GL = pi == 0 ? gvm.line[0] : (pi == 1 ? gvm.line[1] : gvm.line[2]);
  const int H = pi == 0 ? vm.H[0] : (pi == 1 ? vm.H[1] : vm.H[2]);
  const int W = pi == 0 ? vm.W[0] : (pi == 1 ? vm.W[1] : vm.W[2]);
  const int L = pi == 0 ? vm.L[0] : (pi == 1 ? vm.L[1] : vm.L[2]);
  const int sH = pi == 0 ? vm.sH[0] : (pi == 1 ? vm.sH[1] : vm.sH[2]);
  const int sW = pi == 0 ? vm.sW[0] : (pi == 1 ? vm.sW[1] : vm.sW[2]);
  const int lv = sl.level, st = 1 << lv;
  const int Ws = (W + st - 1) >> lv, Hs = (H + st - 1) >> lv, Ls = (L + st - 1) >> lv;
  Tap1 tx = tap1d(cx, Ws), ty = tap1d(cy, Hs), tl = tap1d(cl, Ls);
  const int C = sl.C, qo = 4 * sl.q;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const size_t o00 = (size_t)((ty.i0 << lv) * sH + (tx.i0 << lv) * sW) + qo;
  const size_t o01 = (size_t)((ty.i0 << lv) * sH + ((tx.i0 + 1) << lv) * sW) + qo;
  const size_t o10 = (size_t)(((ty.i0 + 1) << lv) * sH + (tx.i0 << lv) * sW) + qo;
  const size_t o11 = (size_t)(((ty.i0 + 1) << lv) * sH + ((tx.i0 + 1) << lv) * sW) + qo;
  const bool k00 = live && ty.ok0 && tx.ok0, k01 = live && ty.ok0 && tx.ok1,
             k10 = live && ty.ok1 && tx.ok0, k11 = live && ty.ok1 && tx.ok1;
  const bool m0 = live && tl.ok0, m1 = live && tl.ok1;
  // unconditional loads from clamped addresses (no per-tap branch + wait); out-of-range taps are
  // zeroed afterwards, exactly like zero padding
  const int x0c = min(max(tx.i0, 0), Ws - 1) << lv, x1c = min(max(tx.i0 + 1, 0), Ws - 1) << lv;
  const int y0c = min(max(ty.i0, 0), Hs - 1) << lv, y1c = min(max(ty.i0 + 1, 0), Hs - 1) << lv;
  const int l0c = min(max(tl.i0, 0), Ls - 1) << lv, l1c = min(max(tl.i0 + 1, 0), Ls - 1) << lv;
  f32x4 v00 = ld4(P + (size_t)(y0c * sH + x0c * sW) + qo), v01 = ld4(P + (size_t)(y0c * sH + x1c * sW) + qo);
  f32x4 v10 = ld4(P + (size_t)(y1c * sH + x0c * sW) + qo), v11 = ld4(P + (size_t)(y1c * sH + x1c * sW) + qo);
  const size_t l0 = (size_t)(tl.i0 << lv) * C + qo, l1 = (size_t)((tl.i0 + 1) << lv) * C + qo;
  f32x4 a0 = ld4(Lp + (size_t)l0c * C + qo), a1 = ld4(Lp + (size_t)l1c * C + qo);
  if (!k00) v00 = zero;
  if (!k01) v01 = zero;
  if (!k10) v10 = zero;
  if (!k11) v11 = zero;
  if (!m0) a0 = zero;
  if (!m1) a1 = zero;
  const f32x4 pv = v00 * (tx.w0 * ty.w0) + v01 * (tx.w1 * ty.w0) + v10 * (tx.w0 * ty.w1) +
                   v11 * (tx.w1 * ty.w1);
  const f32x4 lvv = a0 * tl.w0 + a1 * tl.w1;
  const f32x4 dp = live ? dq * lvv : zero;  // grad wrt the interpolated plane quad
  const f32x4 dl = live ? dq * pv : zero;   // grad wrt the interpolated line quad
  // coordinate gradients (grid_sampler_2d_backward: piecewise-linear in the fractional part), before the
  // atomics: see gather_xy4_bwd
  const float gcx = 0.5f * (float)(Ws - 1) * dot4(dp, (v01 - v00) * ty.w0 + (v11 - v10) * ty.w1);
  const float gcy = 0.5f * (float)(Hs - 1) * dot4(dp, (v10 - v00) * tx.w0 + (v11 - v01) * tx.w1);
  const float gcl = 0.5f * (float)(Ls - 1) * dot4(dl, a1 - a0);
  if (MODE == 0) {
    atomic_add4(GP, o00, dp * (tx.w0 * ty.w0), k00);
    atomic_add4(GP, o01, dp * (tx.w1 * ty.w0), k01);
    atomic_add4(GP, o10, dp * (tx.w0 * ty.w1), k10);
    atomic_add4(GP, o11, dp * (tx.w1 * ty.w1), k11);
    atomic_add4(GL, l0, dl * tl.w0, m0);
    atomic_add4(GL, l1, dl * tl.w1, m1);
  } else {
    // the quad / plane selection is uniform over a half-wave, so the (iy, ix) pair keys the run.
    // Keys are purely geometric (a dead sample inside a run contributes zeros, it must not split
    // the run); the run's last lane issues the atomics whatever its own liveness.
    const bool g00 = ty.ok0 && tx.ok0, g01 = ty.ok0 && tx.ok1, g10 = ty.ok1 && tx.ok0,
               g11 = ty.ok1 && tx.ok1;
    const int pkey = ((ty.i0 + 4) << 16) | ((tx.i0 + 4) & 0xffff);
    const Run pr = run_of(pkey, s);
    f32x4 r00 = run_scan4(k00 ? dp * (tx.w0 * ty.w0) : zero, pr.start, s);
    f32x4 r01 = run_scan4(k01 ? dp * (tx.w1 * ty.w0) : zero, pr.start, s);
    const f32x4 r10 = run_scan4(k10 ? dp * (tx.w0 * ty.w1) : zero, pr.start, s);
    const f32x4 r11 = run_scan4(k11 ? dp * (tx.w1 * ty.w1) : zero, pr.start, s);
    // cross-run merge: consecutive runs of a ray almost always differ by ONE texel in x or in y and
    // then share two of their four bilinear taps (same memory locations).  The later run absorbs the
    // earlier run's sums for the shared taps and the earlier run skips those two atomics: ~2 requests
    // per run instead of 4.  Directions (this run relative to the previous one), tap bits 00=1 01=2
    // 10=4 11=8 (first digit = row):   +y: prev.10->00, prev.11->01     -y: prev.00->10, prev.01->11
    //                                  +x: prev.01->00, prev.11->10     -x: prev.00->01, prev.10->11
    // All lanes act on the RAW scanned sums simultaneously, so a tap that a run has itself received
    // must not be forwarded again (multi-hop): the taps moved across a boundary are
    // skip(direction out) & ~receive(direction in of the earlier run).
    auto recv_mask = [](int d) { return d == 65536 ? 3 : (d == -65536 ? 12 : (d == 1 ? 5 : (d == -1 ? 10 : 0))); };
    auto skip_mask = [](int d) { return d == 65536 ? 12 : (d == -65536 ? 3 : (d == 1 ? 10 : (d == -1 ? 5 : 0))); };
    int skip_out = 0;
    {
      const int pl = pr.start > 0 ? pr.start - 1 : 0;           // tail lane of the previous run
      const int pk = __shfl(pkey, pl, 32);
      const int din = pr.start > 0 ? pkey - pk : 0;             // direction INTO this run
      const int pdin = __shfl(din, pl, 32);                     // direction into the previous run
      const int min_ = skip_mask(din) & ~recv_mask(pdin);       // prev-run taps moved into this run
      const int nk = dppi<0x130>(pkey);                         // wave_shl:1 -> key of lane s+1
      const int dout = s < 31 ? nk - pkey : 0;
      skip_out = skip_mask(dout) & ~recv_mask(din);             // own taps the next run takes over
      if (pi == 0) {
        (void)min_;
        const f32x4 hA = dout == 65536 ? ((skip_out & 4) ? r10 : zero) : (dout == -65536 ? ((skip_out & 1) ? r00 : zero)
                       : (dout == 1 ? ((skip_out & 2) ? r01 : zero) : ((skip_out & 1) ? r00 : zero)));
        const f32x4 hB = dout == 65536 ? ((skip_out & 8) ? r11 : zero) : (dout == -65536 ? ((skip_out & 2) ? r01 : zero)
                       : (dout == 1 ? ((skip_out & 8) ? r11 : zero) : ((skip_out & 4) ? r10 : zero)));
        f32x4 pA, pB;
        pA.x = __shfl(hA.x, pl, 32); pA.y = __shfl(hA.y, pl, 32); pA.z = __shfl(hA.z, pl, 32); pA.w = __shfl(hA.w, pl, 32);
        pB.x = __shfl(hB.x, pl, 32); pB.y = __shfl(hB.y, pl, 32); pB.z = __shfl(hB.z, pl, 32); pB.w = __shfl(hB.w, pl, 32);
        f32x4 a00 = zero, a01 = zero, a10 = zero, a11 = zero;
        if (din == 65536) { a00 = pA; a01 = pB; }
        else if (din == -65536) { a10 = pA; a11 = pB; }
        else if (din == 1) { a00 = pA; a10 = pB; }
        else if (din == -1) { a01 = pA; a11 = pB; }
        r00 = r00 + a00; r01 = r01 + a01;
        f32x4 t10 = r10 + a10, t11 = r11 + a11;
        // (r10 / r11 are const above: rebuild the outputs)
        atomic_add4(GP, o00, r00, pr.tail && g00 && nz4(r00) && !(skip_out & 1));
        atomic_add4(GP, o01, r01, pr.tail && g01 && nz4(r01) && !(skip_out & 2));
        atomic_add4(GP, o10, t10, pr.tail && g10 && nz4(t10) && !(skip_out & 4));
        atomic_add4(GP, o11, t11, pr.tail && g11 && nz4(t11) && !(skip_out & 8));
      } else {
        // XZ / YZ (the non-split path of the appearance / static scatter): +y chains only
        const float ux = __shfl(r10.x, pl, 32), uy = __shfl(r10.y, pl, 32), uz = __shfl(r10.z, pl, 32),
                    uw = __shfl(r10.w, pl, 32);
        const float vx_ = __shfl(r11.x, pl, 32), vy_ = __shfl(r11.y, pl, 32), vz_ = __shfl(r11.z, pl, 32),
                    vw_ = __shfl(r11.w, pl, 32);
        if (din == 65536) {
          r00.x += ux; r00.y += uy; r00.z += uz; r00.w += uw;
          r01.x += vx_; r01.y += vy_; r01.z += vz_; r01.w += vw_;
        }
        const bool up_ok = dout != 65536;
        atomic_add4(GP, o00, r00, pr.tail && g00 && nz4(r00));
        atomic_add4(GP, o01, r01, pr.tail && g01 && nz4(r01));
        atomic_add4(GP, o10, r10, pr.tail && up_ok && g10 && nz4(r10));
        atomic_add4(GP, o11, r11, pr.tail && up_ok && g11 && nz4(r11));
      }
    }
    f32x4 r;
    const Run lr = run_of(tl.i0 + 4, s);
    const bool LL = ll.base != nullptr;
    const int lo_ = pi == 0 ? ll.off[0] : (pi == 1 ? ll.off[1] : ll.off[2]);
    const int lst = lds_stride(C);
    r = run_scan4(m0 ? dl * tl.w0 : zero, lr.start, s);
    {
      const bool okl = lr.tail && tl.ok0 && nz4(r);
      if (LL) lds_add4(ll, lo_ + (tl.i0 << lv) * lst + qo, r, okl); else atomic_add4(GL, l0, r, okl);
    }
    r = run_scan4(m1 ? dl * tl.w1 : zero, lr.start, s);
    {
      const bool okl = lr.tail && tl.ok1 && nz4(r);
      if (LL) lds_add4(ll, lo_ + ((tl.i0 + 1) << lv) * lst + qo, r, okl); else atomic_add4(GL, l1, r, okl);
    }
  }
  // plane 0 = (x, y | z), 1 = (x, z | y), 2 = (y, z | x).  Selects, not branches: pi differs between the lane
  // halves of the appearance scatter, and the branchy form made the compiler keep dx0..2 in a scratch array
  // indexed per lane (scratch load + vmcnt(0) + store per update, draining the atomics in flight).
  dx0 += pi == 2 ? gcl : gcx;
  dx1 += pi == 0 ? gcy : (pi == 1 ? gcl : gcx);
  dx2 += pi == 0 ? gcl : gcy;
}

// XY quads, four at a time: the wave works on 16 samples (sub-tile j of the 32-sample tile) and the
// four quads 4*grp .. 4*grp+3 of the XY plane at one level: lane = (q = lane>>4, s16 = lane&15).
// Run structure and tail positions are identical in the four 16-lane rows (same samples), so in each
// atomic instruction the four rows carry the four quads of the SAME texel: 64 contiguous bytes
// (16 components), which the L2 coalescer turns into one request -- the (quad | quad) half-wave
// pairing of gather_quad_bwd needed two.  A 16-lane run-scan is four row_shr steps.
// xs/live: coordinates and liveness of THIS lane's sample (sub-tile j); q_is_owner: this lane also
// owns that sample in the (half, sample) mapping of the caller's dx accumulators.
RDRF_D Run run_of16(int key, int s16) {
  const int prev = dppi<0x111>(key);  // row_shr:1 (lane 0 of a row reads 0)
  const bool head = (s16 == 0) || (prev != key);
  const unsigned long long b = __ballot(head);
  const unsigned m = (unsigned)(b >> (16 * ((threadIdx.x & 63) >> 4))) & 0xffffu;
  Run r;
  r.start = 31 - __clz((int)(m & (0xffffu >> (15 - s16))));
  r.tail = (s16 == 15) || ((m >> (s16 + 1)) & 1u);
  return r;
}
RDRF_D f32x4 run_scan4_16(f32x4 v, int start, int s16) {
#define RDRF_SCAN_STEP(D)                                                                   \
  {                                                                                         \
    const float ox = dppf<0x110 + D>(v.x), oy = dppf<0x110 + D>(v.y);                       \
    const float oz = dppf<0x110 + D>(v.z), ow = dppf<0x110 + D>(v.w);                       \
    const bool take = s16 >= D && s16 - D >= start;                                         \
    const float tx_ = v.x + ox, ty_ = v.y + oy, tz_ = v.z + oz, tw_ = v.w + ow;             \
    v.x = take ? tx_ : v.x; v.y = take ? ty_ : v.y; v.z = take ? tz_ : v.z; v.w = take ? tw_ : v.w; \
  }
  RDRF_SCAN_STEP(1)
  RDRF_SCAN_STEP(2)
  RDRF_SCAN_STEP(4)
  RDRF_SCAN_STEP(8)
#undef RDRF_SCAN_STEP
  return v;
}
RDRF_D f32x4 shfl4_row(f32x4 v, int src_lane) {
  f32x4 r;
  r.x = __shfl(v.x, src_lane, 64); r.y = __shfl(v.y, src_lane, 64);
  r.z = __shfl(v.z, src_lane, 64); r.w = __shfl(v.w, src_lane, 64);
  return r;
}
template <int C0Q, int C1Q, bool TILED = false>
RDRF_D void gather_xy4_bwd(const RdrfVM& vm, const RdrfVM& gvm, int lv, int q4, float x0, float x1, float x2,
                           f32x4 dq, bool live, bool q_is_owner, float& dx0, float& dx1, float& dx2,
                           const LdsLines ll, const PlaneTile T = PlaneTile{nullptr, nullptr, 0}) {
  const int lane = threadIdx.x & 63, s16 = lane & 15, rowbase = lane & ~15;
  const float* P = vm.plane[0];
  const float* Lp = vm.line[0];
  float* GP = gvm.plane[0];
  float* GL = gvm.line[0];
  const int H = vm.H[0], W = vm.W[0], L = vm.L[0], sH = vm.sH[0], sW = vm.sW[0];
  const int st = 1 << lv;
  const int Ws = (W + st - 1) >> lv, Hs = (H + st - 1) >> lv, Ls = (L + st - 1) >> lv;
  Tap1 tx = tap1d(x0, Ws), ty = tap1d(x1, Hs), tl = tap1d(x2, Ls);
  constexpr int C = 4 * C0Q;
  const int qo = 4 * q4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const size_t o00 = (size_t)((ty.i0 << lv) * sH + (tx.i0 << lv) * sW) + qo;
  const size_t o01 = (size_t)((ty.i0 << lv) * sH + ((tx.i0 + 1) << lv) * sW) + qo;
  const size_t o10 = (size_t)(((ty.i0 + 1) << lv) * sH + (tx.i0 << lv) * sW) + qo;
  const size_t o11 = (size_t)(((ty.i0 + 1) << lv) * sH + ((tx.i0 + 1) << lv) * sW) + qo;
  const bool g00 = ty.ok0 && tx.ok0, g01 = ty.ok0 && tx.ok1, g10 = ty.ok1 && tx.ok0, g11 = ty.ok1 && tx.ok1;
  const bool k00 = live && g00, k01 = live && g01, k10 = live && g10, k11 = live && g11;
  const bool m0 = live && tl.ok0, m1 = live && tl.ok1;
  const int x0c = min(max(tx.i0, 0), Ws - 1) << lv, x1c = min(max(tx.i0 + 1, 0), Ws - 1) << lv;
  const int y0c = min(max(ty.i0, 0), Hs - 1) << lv, y1c = min(max(ty.i0 + 1, 0), Hs - 1) << lv;
  const int l0c = min(max(tl.i0, 0), Ls - 1) << lv, l1c = min(max(tl.i0 + 1, 0), Ls - 1) << lv;
  f32x4 v00 = ld4(P + (size_t)(y0c * sH + x0c * sW) + qo), v01 = ld4(P + (size_t)(y0c * sH + x1c * sW) + qo);
  f32x4 v10 = ld4(P + (size_t)(y1c * sH + x0c * sW) + qo), v11 = ld4(P + (size_t)(y1c * sH + x1c * sW) + qo);
  f32x4 a0 = ld4(Lp + (size_t)l0c * C + qo), a1 = ld4(Lp + (size_t)l1c * C + qo);
  if (!k00) v00 = zero;
  if (!k01) v01 = zero;
  if (!k10) v10 = zero;
  if (!k11) v11 = zero;
  if (!m0) a0 = zero;
  if (!m1) a1 = zero;
  const f32x4 pv = v00 * (tx.w0 * ty.w0) + v01 * (tx.w1 * ty.w0) + v10 * (tx.w0 * ty.w1) +
                   v11 * (tx.w1 * ty.w1);
  const f32x4 lvv = a0 * tl.w0 + a1 * tl.w1;
  const f32x4 dp = live ? dq * lvv : zero;
  const f32x4 dl = live ? dq * pv : zero;
  // coordinate gradients FIRST: they are the last consumers of the gathered taps.  Computed after the atomics
  // (as the formulas read), the wait for the taps sat behind 16 conditional atomics -- vmcnt is one in-order
  // counter on gfx9, and with conditional issues the compiler must assume the smallest count -- so every
  // iteration waited for all of its own atomics to be acknowledged by the memory side.
  float gcx = 0.5f * (float)(Ws - 1) * dot4(dp, (v01 - v00) * ty.w0 + (v11 - v10) * ty.w1);
  float gcy = 0.5f * (float)(Hs - 1) * dot4(dp, (v10 - v00) * tx.w0 + (v11 - v01) * tx.w1);
  float gcl = 0.5f * (float)(Ls - 1) * dot4(dl, a1 - a0);
  // sum over the four quads (rows) of this sample, then hand it to the lane that owns the sample
  gcx += __shfl_xor(gcx, 16, 64); gcy += __shfl_xor(gcy, 16, 64); gcl += __shfl_xor(gcl, 16, 64);
  gcx += __shfl_xor(gcx, 32, 64); gcy += __shfl_xor(gcy, 32, 64); gcl += __shfl_xor(gcl, 32, 64);
  const int pkey = ((ty.i0 + 4) << 16) | ((tx.i0 + 4) & 0xffff);
  const Run pr = run_of16(pkey, s16);
  f32x4 r00 = run_scan4_16(k00 ? dp * (tx.w0 * ty.w0) : zero, pr.start, s16);
  f32x4 r01 = run_scan4_16(k01 ? dp * (tx.w1 * ty.w0) : zero, pr.start, s16);
  f32x4 r10 = run_scan4_16(k10 ? dp * (tx.w0 * ty.w1) : zero, pr.start, s16);
  f32x4 r11 = run_scan4_16(k11 ? dp * (tx.w1 * ty.w1) : zero, pr.start, s16);
  {  // cross-run merge of shared taps, all four directions (see gather_quad_bwd)
    auto recv_mask = [](int d) { return d == 65536 ? 3 : (d == -65536 ? 12 : (d == 1 ? 5 : (d == -1 ? 10 : 0))); };
    auto skip_mask = [](int d) { return d == 65536 ? 12 : (d == -65536 ? 3 : (d == 1 ? 10 : (d == -1 ? 5 : 0))); };
    const int pl = rowbase | (pr.start > 0 ? pr.start - 1 : 0);
    const int pk = __shfl(pkey, pl, 64);
    const int din = pr.start > 0 ? pkey - pk : 0;
    const int pdin = __shfl(din, pl, 64);
    const int min_ = skip_mask(din) & ~recv_mask(pdin);
    const int nk = dppi<0x101>(pkey);                        // row_shl:1 -> key of lane s16+1
    const int dout = s16 < 15 ? nk - pkey : 0;
    const int skip_out = skip_mask(dout) & ~recv_mask(din);
    // the EARLIER run prepares the two taps it hands over (its direction out = the later run's
    // direction in), so the later run pulls two quads instead of four
    (void)min_;
    const f32x4 hA = dout == 65536 ? ((skip_out & 4) ? r10 : zero) : (dout == -65536 ? ((skip_out & 1) ? r00 : zero)
                   : (dout == 1 ? ((skip_out & 2) ? r01 : zero) : ((skip_out & 1) ? r00 : zero)));
    const f32x4 hB = dout == 65536 ? ((skip_out & 8) ? r11 : zero) : (dout == -65536 ? ((skip_out & 2) ? r01 : zero)
                   : (dout == 1 ? ((skip_out & 8) ? r11 : zero) : ((skip_out & 4) ? r10 : zero)));
    const f32x4 pA = shfl4_row(hA, pl), pB = shfl4_row(hB, pl);
    if (din == 65536) { r00 = r00 + pA; r01 = r01 + pB; }
    else if (din == -65536) { r10 = r10 + pA; r11 = r11 + pB; }
    else if (din == 1) { r00 = r00 + pA; r10 = r10 + pB; }
    else if (din == -1) { r01 = r01 + pA; r11 = r11 + pB; }
    plane_add4<TILED>(T, lv, tx.i0, ty.i0, qo, GP, o00, r00, pr.tail && g00 && nz4(r00) && !(skip_out & 1));
    plane_add4<TILED>(T, lv, tx.i0 + 1, ty.i0, qo, GP, o01, r01, pr.tail && g01 && nz4(r01) && !(skip_out & 2));
    plane_add4<TILED>(T, lv, tx.i0, ty.i0 + 1, qo, GP, o10, r10, pr.tail && g10 && nz4(r10) && !(skip_out & 4));
    plane_add4<TILED>(T, lv, tx.i0 + 1, ty.i0 + 1, qo, GP, o11, r11, pr.tail && g11 && nz4(r11) && !(skip_out & 8));
  }
  {
    const Run lr = run_of16(tl.i0 + 4, s16);
    const bool LL = ll.base != nullptr;
    const int lst = lds_stride(C);
    if (LL && ll.direct) {
      const f32x4 r0 = m0 ? dl * tl.w0 : zero, r1 = m1 ? dl * tl.w1 : zero;
      lds_add4(ll, ll.off[0] + (tl.i0 << lv) * lst + qo, r0, m0 && nz4(r0));
      lds_add4(ll, ll.off[0] + ((tl.i0 + 1) << lv) * lst + qo, r1, m1 && nz4(r1));
    } else {
    f32x4 r = run_scan4_16(m0 ? dl * tl.w0 : zero, lr.start, s16);
    bool okl = lr.tail && tl.ok0 && nz4(r);
    if (LL) lds_add4(ll, ll.off[0] + (tl.i0 << lv) * lst + qo, r, okl); else atomic_add4(GL, (size_t)(tl.i0 << lv) * C + qo, r, okl);
    r = run_scan4_16(m1 ? dl * tl.w1 : zero, lr.start, s16);
    okl = lr.tail && tl.ok1 && nz4(r);
    if (LL) lds_add4(ll, ll.off[0] + ((tl.i0 + 1) << lv) * lst + qo, r, okl); else atomic_add4(GL, (size_t)((tl.i0 + 1) << lv) * C + qo, r, okl);
    }
  }
  if (q_is_owner) { dx0 += gcx; dx1 += gcy; dx2 += gcl; }
}

// XZ / YZ quads of the ray-tile scatter, column-split: BOTH half-waves work on the same quad g of the
// same 32 samples; half h owns the bilinear column ix + h (its lower and upper row taps) and the line
// tap h.  The run structure is identical in the two halves, so in every atomic instruction the lanes
// of half 0 carry texel (iy, ix) and the same lanes of half 1 carry texel (iy, ix + 1): with x-fastest
// plane storage these are 16 bytes apart and the L2 coalescer (which merges same-line lanes across
// the whole wave, tools/ubench/atomics.hip kernels G/H) makes ONE request of them -- half the atomic
// requests of the XZ / YZ planes, which were ~1/3 of the density scatter's time.
// Coordinate gradients are computed by both halves and halved (x*0.5 + x*0.5 is exact).
template <int C0Q, int C1Q, bool TILED = false>
RDRF_D void gather_zquad_bwd(const RdrfVM& vm, const RdrfVM& gvm, int g, int h, float x0, float x1, float x2,
                             f32x4 dq, bool live, int s, float& dx0, float& dx1, float& dx2,
                             const LdsLines ll, const PlaneTile T = PlaneTile{nullptr, nullptr, 0}) {
  QuadSel<C0Q, C1Q> sl = quad_sel<C0Q, C1Q>(g);
  const int pi = sl.pi;   // 1 or 2 (wave-uniform)
  const float cx = pi == 2 ? x1 : x0;
  const float cy = x2;
  const float cl = pi == 1 ? x1 : x0;
  const float* P = pi == 1 ? vm.plane[1] : vm.plane[2];
  const float* Lp = pi == 1 ? vm.line[1] : vm.line[2];
  float* GP = pi == 1 ? gvm.plane[1] : gvm.plane[2];
  float* GL = pi == 1 ? gvm.line[1] : gvm.line[2];
  const int H = pi == 1 ? vm.H[1] : vm.H[2], W = pi == 1 ? vm.W[1] : vm.W[2], L = pi == 1 ? vm.L[1] : vm.L[2];
  const int sH = pi == 1 ? vm.sH[1] : vm.sH[2], sW = pi == 1 ? vm.sW[1] : vm.sW[2];
  const int lv = sl.level, st = 1 << lv;
  const int Ws = (W + st - 1) >> lv, Hs = (H + st - 1) >> lv, Ls = (L + st - 1) >> lv;
  Tap1 tx = tap1d(cx, Ws), ty = tap1d(cy, Hs), tl = tap1d(cl, Ls);
  const int C = sl.C, qo = 4 * sl.q;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int x0c = min(max(tx.i0, 0), Ws - 1) << lv, x1c = min(max(tx.i0 + 1, 0), Ws - 1) << lv;
  const int y0c = min(max(ty.i0, 0), Hs - 1) << lv, y1c = min(max(ty.i0 + 1, 0), Hs - 1) << lv;
  const int l0c = min(max(tl.i0, 0), Ls - 1) << lv, l1c = min(max(tl.i0 + 1, 0), Ls - 1) << lv;
  f32x4 v00 = ld4(P + (size_t)(y0c * sH + x0c * sW) + qo), v01 = ld4(P + (size_t)(y0c * sH + x1c * sW) + qo);
  f32x4 v10 = ld4(P + (size_t)(y1c * sH + x0c * sW) + qo), v11 = ld4(P + (size_t)(y1c * sH + x1c * sW) + qo);
  f32x4 a0 = ld4(Lp + (size_t)l0c * C + qo), a1 = ld4(Lp + (size_t)l1c * C + qo);
  if (!(live && ty.ok0 && tx.ok0)) v00 = zero;
  if (!(live && ty.ok0 && tx.ok1)) v01 = zero;
  if (!(live && ty.ok1 && tx.ok0)) v10 = zero;
  if (!(live && ty.ok1 && tx.ok1)) v11 = zero;
  if (!(live && tl.ok0)) a0 = zero;
  if (!(live && tl.ok1)) a1 = zero;
  const f32x4 pv = v00 * (tx.w0 * ty.w0) + v01 * (tx.w1 * ty.w0) + v10 * (tx.w0 * ty.w1) +
                   v11 * (tx.w1 * ty.w1);
  const f32x4 lvv = a0 * tl.w0 + a1 * tl.w1;
  const f32x4 dp = live ? dq * lvv : zero;
  const f32x4 dl = live ? dq * pv : zero;
  // (coordinate gradients before the atomics: see gather_xy4_bwd)
  const float gcx = 0.25f * (float)(Ws - 1) * dot4(dp, (v01 - v00) * ty.w0 + (v11 - v10) * ty.w1);
  const float gcy = 0.25f * (float)(Hs - 1) * dot4(dp, (v10 - v00) * tx.w0 + (v11 - v01) * tx.w1);
  const float gcl = 0.25f * (float)(Ls - 1) * dot4(dl, a1 - a0);
  // this half's column
  const float wxc = h ? tx.w1 : tx.w0;
  const bool okc = h ? tx.ok1 : tx.ok0;
  const int ixc = tx.i0 + h;
  const bool g0 = ty.ok0 && okc, g1 = ty.ok1 && okc;
  const size_t o0 = (size_t)((ty.i0 << lv) * sH + (ixc << lv) * sW) + qo;
  const size_t o1 = (size_t)(((ty.i0 + 1) << lv) * sH + (ixc << lv) * sW) + qo;
  const int pkey = ((ty.i0 + 4) << 16) | ((tx.i0 + 4) & 0xffff);   // same key in both halves
  const Run pr = run_of(pkey, s);
  f32x4 r0 = run_scan4((live && g0) ? dp * (wxc * ty.w0) : zero, pr.start, s);
  const f32x4 r1 = run_scan4((live && g1) ? dp * (wxc * ty.w1) : zero, pr.start, s);
  // cross-run merge along the row axis (see gather_quad_bwd)
  const int pl = pr.start > 0 ? pr.start - 1 : 0;
  const int pk = __shfl(pkey, pl, 32);
  const bool chain_prev = pr.start > 0 && pk == pkey - (1 << 16);
  const float ux = __shfl(r1.x, pl, 32), uy = __shfl(r1.y, pl, 32), uz = __shfl(r1.z, pl, 32),
              uw = __shfl(r1.w, pl, 32);
  if (chain_prev) { r0.x += ux; r0.y += uy; r0.z += uz; r0.w += uw; }
  const int nk = dppi<0x130>(pkey);
  const bool up_ok = !(s < 31 && nk == pkey + (1 << 16));
  plane_add4<TILED>(T, lv, ixc, ty.i0, qo, GP, o0, r0, pr.tail && g0 && nz4(r0));
  plane_add4<TILED>(T, lv, ixc, ty.i0 + 1, qo, GP, o1, r1, pr.tail && up_ok && g1 && nz4(r1));
  // line tap h
  if (ll.base && ll.direct) {
    const bool okl = live && (h ? tl.ok1 : tl.ok0);
    const f32x4 r = okl ? dl * (h ? tl.w1 : tl.w0) : zero;
    lds_add4(ll, (pi == 1 ? ll.off[1] : ll.off[2]) + ((tl.i0 + h) << lv) * lds_stride(C) + qo, r, okl && nz4(r));
  } else {
    const Run lr = run_of(tl.i0 + 4, s);
    const bool okl = h ? tl.ok1 : tl.ok0;
    const f32x4 r = run_scan4((live && okl) ? dl * (h ? tl.w1 : tl.w0) : zero, lr.start, s);
    const bool doit = lr.tail && okl && nz4(r);
    const int li = tl.i0 + h;
    if (ll.base) lds_add4(ll, (pi == 1 ? ll.off[1] : ll.off[2]) + (li << lv) * lds_stride(C) + qo, r, doit);
    else atomic_add4(GL, (size_t)(li << lv) * C + qo, r, doit);
  }
  dx0 += pi == 1 ? gcx : gcl;   // plane 1 = (x, z | y), 2 = (y, z | x)
  dx1 += pi == 1 ? gcl : gcx;
  dx2 += gcy;
}
