// rdrf_bwd_fused.hip -- the backward-data kernels that form their layers' weight gradients themselves, for gfx950:
// k_scene_flow_bwd_dw (scene-flow MLP) and k_dyn_warp_bwd_dw (warp MLP of the dynamic field on flat tiles), the device code
// only they use, and the host functions that launch them (rdrf_bwd_host.hpp).  Their two-kernel partners -- k_scene_flow_bwd /
// k_dyn_density_bwd<1> followed by k_dw3 -- and the entry points that choose between the two forms are in rdrf_bwd.hip.  The data
// steps a kernel here shares with its partner (warp_coord_grads, warp_layer5_bwd, warp_layer4_bwd, warp_layer3_bwd, warp_x0_bwd,
// dtout_segments, relu_gate, the *_bwd_flat encoders beside their branchy twins) are the partner's functions, rdrf_bwd_mlp_dev.hpp;
// the kernels here keep their own stores (buffer stores, where the partner has plain ones: the one-basic-block rule below).
// The family's design.  A backward-data kernel writes each layer's dz as rows only for k_dw3 to read them back, together with
// the activation rows the data kernel had just loaded.  Here the wave that owns a 32-sample tile keeps going: the data gradient
// runs the calls of the partner kernel on the same values (its outputs keep their bits), and after each 64-row layer the wave
// writes the layer's dz into its OWN 8 KB LDS stage in the saved-row layout [row][32 samples] (dzs_write), reads it back as the A
// operand of the fp32 MFMA -- lane (li, h): row li of a 32-row block, samples 16 h .. 16 h + 15, as k_dw3 reads its stage -- and
// multiplies it with the layer's input rows, read in the same form from the saved rows (row16_load: 64 contiguous bytes of a row,
// L2 hits: the data path of the same pass loads those rows too) (dzs_layer).  The 32 x 32 products accumulate in registers of the
// wave for the whole launch -- 160 to 192 accumulators, hence FUSED_WAVES = 4 waves per workgroup (512 registers per lane) -- with
// no workgroup barrier in the tile loop and no round of tiles that could be partly empty.  At the end the waves of a workgroup add
// their accumulators through the then dead LDS in wave order (a fixed order: the deterministic build stays bit-reproducible) and
// the workgroup flushes once through grad_add, columns mapped as dw_launch maps them (fused_flush_tile, fused_flush_bias).  Layers
// with a handful of outputs stay off the matrix pipe (most rows of their 32 x 32 products would be empty); their sums ride along
// in the cross-wave sum and each kernel flushes them itself.
// What the code generator needs -- hipcc's allocation for these kernels swings between no spill and 100 to 140 spilled registers
// on changes that look neutral in the source:
//   - From the first stage write on, a tile's pass is ONE basic block: what depends on a pointer being there is a template
//     argument, partial updates of global memory are buffer accesses whose offset is out of range in the lanes that do not take
//     part (tile_add3), the positional-encoding backward has no branch on the lane half (*_bwd_flat).  With a branch in the pass,
//     hipcc sinks every product -- pure arithmetic that only the next pass reads -- behind the branch to the end of the pass and
//     keeps the operands of all of them alive until there.
//   - The stage addresses are four lane offsets per direction plus constants (DzsPos): given dzs_pos per slot, hipcc keeps one
//     address register per slot (32) alive across the tile loop.
//   - A scheduling fence follows the products of each dz block (dzs_layer; the 6-output layer of the scene-flow kernel has its
//     own): left free, hipcc gathers the LDS reads of every block in front of the first product and spills.
// Row contract (head of rdrf_dw.hip): a lane past N * S stages dz = 0 behind finite activations (0 x finite = 0); tiles past
// ceil(N * S / 32) are never read; every stage row that is read was written by the same wave for the same tile.
#include "rdrf_bwd_mlp_dev.hpp"
#include "rdrf_bwd_host.hpp"

RDRF_DET_UNIT(bwd_fused)

// ------------------------------------------------------------------------------------------------
// a wave's private 64-row dz stage
// ------------------------------------------------------------------------------------------------
constexpr int FUSED_WAVES = 4;       // waves per workgroup, a tile per wave and pass
constexpr int DZS_FLOATS = 64 * 32;  // one layer's dz: 64 rows x 32 samples
// float offset of 16-byte chunk `chunk` (4 samples) of stage row `row`: the chunk index is XORed with bits of the row so
// that the 16 lanes of a ds_read_b128 group (consecutive rows, one chunk) cover all 64 banks
RDRF_D int dzs_pos(int row, int chunk) { return row * 32 + ((chunk ^ ((row >> 1) & 7)) << 2); }
RDRF_D void dzs_wave_sync() {   // LDS traffic of ONE wave: in order in hardware; this orders it for the compiler
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  __builtin_amdgcn_sched_barrier(0);
}
// Lane (s, h) writes slot kk to row elem_of(kk, h) = 8 (kk >> 2) + 4 h + (kk & 3), whose swizzle term ((row >> 1) & 7) is
// (h << 1) ^ C with C = 4 ((kk >> 2) & 1) + ((kk & 3) >> 1): FOUR lane offsets (DzsPos::w) + a constant per slot, and the reads of
// row 32 a + li are four more (DzsPos::r) + 1024 a.
struct DzsPos {
  int w[4], r[4];
};
RDRF_D DzsPos dzs_lane_pos(int s, int h) {
  DzsPos p;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    p.w[c] = h * 128 + ((((s >> 2) ^ (h << 1)) ^ ((c >> 1) * 4 + (c & 1))) << 2) + (s & 3);
    p.r[c] = dzs_pos(s, 4 * h + c);
  }
  return p;
}
RDRF_D void dzs_write(float* __restrict__ st, const float (&v)[32], const DzsPos& p) {
#pragma unroll
  for (int kk = 0; kk < 32; ++kk) st[p.w[(((kk >> 2) & 1) << 1) | ((kk & 3) >> 1)] + (8 * (kk >> 2) + (kk & 3)) * 32] = v[kk];
}
RDRF_D void dzs_read(f32x4 (&o)[4], const float* __restrict__ st, int blk, const DzsPos& p) {
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = *(const f32x4*)(st + p.r[q] + 1024 * blk);
}
// the 16 samples of lane half h of a saved row, in the form dzs_read gives
RDRF_D void row16_load(f32x4 (&o)[4], const float* __restrict__ tile_base, int row, int h) {
  const float* p = tile_base + (size_t)row * 32 + 16 * h;
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = *(const f32x4*)(p + 4 * q);
}
RDRF_D float row16_sum(const f32x4 (&a)[4]) {
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) t += a[q].x + a[q].y + a[q].z + a[q].w;
  return t;
}
RDRF_D void dzs_prod(f32x16& acc, const f32x4 (&a)[4], const f32x4 (&b)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[q].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[q].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[q].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[q].w, acc, 0, 0, 0);
  }
}
// the products of one staged layer: NA dz blocks (stage rows 32 a + li of lane (li, h)) x the NB = 2 or 3 input blocks b0 | b1
// [| b2, not read when NB == 2] -> accW[P0 + NB a + k], bias sums -> bsum[A0 + a]; the head comment's fence per dz block
template <int NA, int NB, int P0, int A0, int NPROD, int NDZ>
RDRF_D void dzs_layer(f32x16 (&accW)[NPROD], float (&bsum)[NDZ], const float* __restrict__ st, const DzsPos& p, const f32x4 (&b0)[4],
                      const f32x4 (&b1)[4], const f32x4 (&b2)[4]) {
  static_assert((NB == 2 || NB == 3) && P0 + NB * NA <= NPROD && A0 + NA <= NDZ, "products past the accumulators");
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    f32x4 av[4];
    dzs_read(av, st, a, p);
    bsum[A0 + a] += row16_sum(av);
    dzs_prod(accW[P0 + NB * a], av, b0);
    dzs_prod(accW[P0 + NB * a + 1], av, b1);
    if constexpr (NB == 3) dzs_prod(accW[P0 + NB * a + 2], av, b2);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ------------------------------------------------------------------------------------------------
// cross-wave sum and flush
// ------------------------------------------------------------------------------------------------
// red, over the kernel's LDS (weight image and stages, dead by then): NPROD product tiles of 1024 floats [rr][lane], then 64
// floats per dz block (bias sums) and per small-layer sum.  The sum itself is written out in each kernel: as a function shared
// by the two, hipcc vectorises it differently and renumbers the registers of the whole kernel with it (the bf16 MFMAs of the
// warp kernel then see a VALU write of an operand 6 instructions behind them instead of 10).
constexpr int fused_red_floats(int nprod, int ndz, int nsm) { return nprod * 1024 + (ndz + nsm) * 64; }
// flush of one product tile by the workgroup.  tile[rr * 64 + 32 hh + c]: C row (rr & 3) + 8 (rr >> 2) + 4 hh (out neuron of the dz
// block) -> row orow0 + that of dW; column c = li (element e0 + c of input segment `seg`) -> seg_imap's of dW's ld columns, or none
RDRF_D void fused_flush_tile(const float* tile, float* dW, int orow0, int ld, int seg, int e0) {
  for (int e = threadIdx.x; e < 1024; e += blockDim.x) {
    const int rr = e >> 6, hh = (e >> 5) & 1, c = e & 31;
    const int col = seg_imap(seg, e0 + c, ld);
    const int orow = orow0 + (rr & 3) + 8 * (rr >> 2) + 4 * hh;
    if (col >= 0) grad_add(dW + (size_t)orow * ld + col, tile[e]);
  }
}
// flush of one dz block's bias sums (the two lane halves hold the two halves of a tile's samples) -> db[0 .. 31]
RDRF_D void fused_flush_bias(const float* sums, float* db) {
  if (threadIdx.x < 32) grad_add(db + (int)threadIdx.x, sums[threadIdx.x] + sums[32 + threadIdx.x]);
}
// g[s][0..2] += v in the lanes with `on`, g = the tile's 32 x 3 floats: the tile's 384 bytes as a buffer, every other lane out
// of range (no branch: see the head comment)
RDRF_D void tile_add3(float* g, bool on, int s, float v0, float v1, float v2) {
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)g, 0, 384, 0x00020000);
  const int off = on ? s * 12 : 1 << 20;
  const float p0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, off, 0, 0));
  const float p1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, off, 4, 0));
  const float p2 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, off, 8, 0));
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, p0 + v0), rp, off, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, p1 + v1), rp, off, 4, 0);
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, p2 + v2), rp, off, 8, 0);
}
// launch geometry: whole workgroups of FUSED_WAVES waves, a wave per tile, at most a workgroup per CU
void fused_dw_geometry(long tiles, int* grid, int* waves) {
  const long blocks = (tiles + FUSED_WAVES - 1) / FUSED_WAVES;
  *grid = (int)(blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks));
  *waves = FUSED_WAVES;
}

// ------------------------------------------------------------------------------------------------
// scene flow, the partner of k_scene_flow_bwd + dw_sf (224 dz rows per tile written and read back): 12 products of the three
// 64-row layers in 192 accumulators; g_pts keeps its bits.  The 6-output layer as two 32 x 32 products would have 26 of 32 rows
// empty (2048 MFMA cycles per tile): instead the lane that holds row li of the H4 blocks for the 16 samples of its half reads the
// six dz6 rows of those samples as LDS broadcasts and keeps 12 sums (192 FMAs per tile).  One basic block: PTS is a template
// argument, both lane halves store the dz6 rows.
// ------------------------------------------------------------------------------------------------
namespace sfd {
constexpr int ST_DZ6 = DZS_FLOATS, ST_SIZE = DZS_FLOATS + 8 * 32;   // a wave's stage: one layer's dz + the dz6 rows
constexpr int NPROD = 12, NDZ = 6;                                  // MFMA products / their dz blocks (dz4 x 2 | dz2 x 2 | dz0 x 2)
constexpr int NSM = 18;                                             // 6-output layer: 6 x 2 weight sums, 6 bias sums per lane
constexpr int LDS = pkb::SF_SIZE + FUSED_WAVES * ST_SIZE;
static_assert(fused_red_floats(NPROD, NDZ, NSM) <= LDS && LDS * 4 <= 160 * 1024, "the cross-wave sum reuses the kernel's LDS");
}  // namespace sfd
template <bool PTS>   // PTS: the caller takes the point gradient (g_pts); without it the first layer's data product is skipped
__global__ __launch_bounds__(64 * FUSED_WAVES) void k_scene_flow_bwd_dw(int N, int S, Box box,
                                                        const float* __restrict__ pkg,
                                                        const float* __restrict__ act_rows,
                                                        const float* __restrict__ g_f,
                                                        const float* __restrict__ g_b,
                                                        SfGrads G,
                                                        float* __restrict__ g_pts) {
  __shared__ __attribute__((aligned(16))) float lds[sfd::LDS];
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
  float* st = lds + pkb::SF_SIZE + wave * sfd::ST_SIZE;
  lds_fill(lds, pkg + pkb::REG_SF, pkb::SF_SIZE);
  const int total = N * S;
  const int ntiles = (total + 31) >> 5;
  const DzsPos pos = dzs_lane_pos(s, h);
  f32x16 accW[sfd::NPROD];
  float bsum[sfd::NDZ], sm[sfd::NSM];   // sm: dW of sfw[3], [o][input block] for input li of the block; then db of sfb[3]
  acc_zero<sfd::NPROD>(accW);
#pragma unroll
  for (int a = 0; a < sfd::NDZ; ++a) bsum[a] = 0.f;
#pragma unroll
  for (int a = 0; a < sfd::NSM; ++a) sm[a] = 0.f;
  for (int tile = blockIdx.x * nwaves + wave; tile < ntiles; tile += gridDim.x * nwaves) {
    const int li = tile * 32 + s;
    const bool act = li < total;
    const int idx = act ? li : 0;
    const float* svb = act_rows + (size_t)tile * sv::SF_ROWS * 32;
    float dz6[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) {
      const float* gsrc = o < 3 ? g_f : g_b;
      dz6[o] = (act && gsrc) ? gsrc[(size_t)idx * 3 + (o % 3)] : 0.f;
    }
    float dz[32], Hh[32];
    f32x4 b0[4], b1[4];
    load_rows<32>(svb, sv::SF_H4, Hh, s, h);
    row16_load(b0, svb, sv::SF_H4 + s, h);
    row16_load(b1, svb, sv::SF_H4 + 32 + s, h);
    small_layer_bwd<32, 6>(dz, Hh, lds + pkb::SF_W6, h, dz6);
    dzs_wave_sync();   // the previous tile's reads of the stage are done
#pragma unroll
    for (int o = 0; o < 6; ++o) st[sfd::ST_DZ6 + o * 32 + s] = dz6[o];   // (both halves, the same value; read as broadcasts)
    dzs_write(st, dz, pos);
    dzs_wave_sync();
#pragma unroll
    for (int o = 0; o < 6; ++o) {   // sfw[3]: dz6 x H4
      f32x4 d[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) d[q] = *(const f32x4*)(st + sfd::ST_DZ6 + o * 32 + 16 * h + 4 * q);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sm[2 * o] = fmaf(d[q].x, b0[q].x, sm[2 * o]); sm[2 * o + 1] = fmaf(d[q].x, b1[q].x, sm[2 * o + 1]);
        sm[2 * o] = fmaf(d[q].y, b0[q].y, sm[2 * o]); sm[2 * o + 1] = fmaf(d[q].y, b1[q].y, sm[2 * o + 1]);
        sm[2 * o] = fmaf(d[q].z, b0[q].z, sm[2 * o]); sm[2 * o + 1] = fmaf(d[q].z, b1[q].z, sm[2 * o + 1]);
        sm[2 * o] = fmaf(d[q].w, b0[q].w, sm[2 * o]); sm[2 * o + 1] = fmaf(d[q].w, b1[q].w, sm[2 * o + 1]);
      }
      sm[12 + o] += row16_sum(d);
      __builtin_amdgcn_sched_barrier(0);
    }
    row16_load(b0, svb, sv::SF_H2 + s, h);
    row16_load(b1, svb, sv::SF_H2 + 32 + s, h);
    f32x16 acc[2];
    acc_zero<2>(acc);
    mfma_seg<2, 32>(acc, dz, lds + pkb::SF_W4T, lane);
    load_rows<32>(svb, sv::SF_H2, Hh, s, h);
    dzs_layer<2, 2, 0, 0>(accW, bsum, st, pos, b0, b1, b1);   // sfw[2]: dz4 x H2
    relu_gate<32>(dz, Hh, acc);
    dzs_wave_sync();
    dzs_write(st, dz, pos);
    dzs_wave_sync();
    row16_load(b0, svb, sv::SF_H0 + s, h);
    row16_load(b1, svb, sv::SF_H0 + 32 + s, h);
    acc_zero<2>(acc);
    mfma_seg<2, 32>(acc, dz, lds + pkb::SF_W2T, lane);
    load_rows<32>(svb, sv::SF_H0, Hh, s, h);
    dzs_layer<2, 2, 4, 2>(accW, bsum, st, pos, b0, b1, b1);   // sfw[1]: dz2 x H0
    relu_gate<32>(dz, Hh, acc);
    dzs_wave_sync();
    dzs_write(st, dz, pos);
    dzs_wave_sync();
    row16_load(b0, svb, sv::SF_X + s, h);
    row16_load(b1, svb, sv::SF_X + 32 + s, h);
    if constexpr (PTS) {
      acc_zero<2>(acc);
      mfma_seg<2, 32>(acc, dz, lds + pkb::SF_W0T, lane);
    }
    dzs_layer<2, 2, 8, 4>(accW, bsum, st, pos, b0, b1, b1);   // sfw[0]: dz0 x X
    if constexpr (PTS) {
      float X[20], dX[20];
      load_rows<20>(svb, sv::SF_X, X, s, h);
#pragma unroll
      for (int kk = 0; kk < 20; ++kk) dX[kk] = acc[kk >> 4][kk & 15];
      float d0 = 0.f, d1 = 0.f, d2 = 0.f;
      sf_x_bwd_flat(X, dX, h, d0, d1, d2);
      d0 += __shfl_xor(d0, 32, 64); d1 += __shfl_xor(d1, 32, 64); d2 += __shfl_xor(d2, 32, 64);
      tile_add3(g_pts + (size_t)tile * 96, act && h == 0, s, d0 * box.inv[0], d1 * box.inv[1], d2 * box.inv[2]);
    }
  }
  // cross-wave sum in wave order (layout: fused_red_floats), then one flush per workgroup
  float* red = lds;
  for (int w = 0; w < nwaves; ++w) {
    __syncthreads();   // (the first: every wave is done with the image and its stage)
    if (wave == w) {
#pragma unroll
      for (int p = 0; p < sfd::NPROD; ++p)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          float* r = red + p * 1024 + rr * 64 + lane;
          *r = w == 0 ? accW[p][rr] : *r + accW[p][rr];
        }
#pragma unroll
      for (int a = 0; a < sfd::NDZ; ++a) {
        float* r = red + sfd::NPROD * 1024 + a * 64 + lane;
        *r = w == 0 ? bsum[a] : *r + bsum[a];
      }
#pragma unroll
      for (int a = 0; a < sfd::NSM; ++a) {
        float* r = red + sfd::NPROD * 1024 + (sfd::NDZ + a) * 64 + lane;
        *r = w == 0 ? sm[a] : *r + sm[a];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < sfd::NPROD; ++p) {
    // product p: layer, dz block of the layer, input block of the layer (the order of the dzs_layer calls above)
    const int layer = 2 - (p >> 2), bo = (p & 3) >> 1, k = p & 1;
    fused_flush_tile(red + p * 1024, G.w[layer], bo * 32, layer == 0 ? 36 : 64, layer == 0 ? SEG_SF_X : SEG_IDENT, 32 * k);
  }
#pragma unroll
  for (int a = 0; a < sfd::NDZ; ++a) fused_flush_bias(red + sfd::NPROD * 1024 + a * 64, G.b[2 - (a >> 1)] + (a & 1) * 32);
  // the 6-output layer: the two lane halves hold the two halves of a tile's samples; every lane li holds the same bias sums
  for (int e = threadIdx.x; e < 12 * 32 + 6; e += blockDim.x) {
    const int a = e < 12 * 32 ? e >> 5 : 12 + (e - 12 * 32), c = e < 12 * 32 ? e & 31 : 0;
    const float* r = red + sfd::NPROD * 1024 + (sfd::NDZ + a) * 64 + c;
    if (a < 12) grad_add(G.w[3] + (a >> 1) * 64 + (a & 1) * 32 + c, r[0] + r[32]);
    else grad_add(G.b[3] + (a - 12), r[0] + r[32]);
  }
}

// ------------------------------------------------------------------------------------------------
// warp MLP on flat tiles, the partner of k_dyn_density_bwd<1, false, true> + the layer3 / layer4 products of k_dw3 (128 dz rows
// per tile): the wave stages dz4, then dz3, and multiplies them with H3 (2 x 2 products) and with X0 | T (2 x 3); of those rows
// only T is not loaded by the data path of the same pass.  10 products in 160 accumulators; the sums of the 3-row layer (sw / sb
// of k_dyn_density_bwd) ride along in the cross-wave sum.  The data gradient runs the partner's calls on the same values: g_xyz,
// d(tout) and K1G_SM keep their bits.  One basic block: x0_bwd_flat, g_xyz through tile_add3, d(tout) as buffer stores.
// ------------------------------------------------------------------------------------------------
namespace wpd {
constexpr int NPROD = 10, NDZ = 4, NSM = 6;            // products (dz4 x H3: 4 | dz3 x [X0 | T]: 6), dz blocks, sw[3] + sb[3]
constexpr int LDS = pkb::K1W_SIZE + FUSED_WAVES * DZS_FLOATS;
static_assert(pkb::K1W_SIZE % 4 == 0 && fused_red_floats(NPROD, NDZ, NSM) <= LDS && LDS * 4 <= 160 * 1024,
              "the stages are 16-byte aligned; the cross-wave sum reuses the kernel's LDS");
}  // namespace wpd
template <bool GX>   // GX: the caller takes g_xyz
__global__ __launch_bounds__(64 * FUSED_WAVES) void k_dyn_warp_bwd_dw(BwdArgs a, DynG gw, WarpGrads G) {
  __shared__ __attribute__((aligned(16))) float lds[wpd::LDS];
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
  float* st = lds + pkb::K1W_SIZE + wave * DZS_FLOATS;
  lds_fill(lds, a.pk + pkb::REG_K1W, pkb::K1W_SIZE);
  const int total = a.N * a.S;
  const int ntiles = (total + 31) >> 5;
  const DzsPos pos = dzs_lane_pos(s, h);
  f32x16 accW[wpd::NPROD];
  float bsum[wpd::NDZ];
  float sw[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f};
  acc_zero<wpd::NPROD>(accW);
#pragma unroll
  for (int i = 0; i < wpd::NDZ; ++i) bsum[i] = 0.f;
  for (int n = blockIdx.x * nwaves + wave; n < ntiles; n += gridDim.x * nwaves) {
    const bool act = n * 32 + s < total;
    const int idx = act ? n * 32 + s : 0;
    const float* svb = a.sp.act1 + (size_t)n * sv::K1_ROWS * 32;
    float* gb = a.grows1 + (size_t)n * sv::K1G_ROWS * 32;
    WarpIn g = warp_coord_grads(a, gb, act, idx, s, h);
    float dz4[32];
    warp_layer5_bwd(dz4, lds, svb, g, true, s, h, sw, sb);
    // ---- one basic block from here to the end of the pass
    f32x4 b0[4], b1[4], b2[4];
    dzs_wave_sync();   // the previous tile's reads of the stage are done
    dzs_write(st, dz4, pos);
    dzs_wave_sync();
    row16_load(b0, svb, sv::K1_H3 + s, h);
    row16_load(b1, svb, sv::K1_H3 + 32 + s, h);
    float dz3[32];
    {
      f32x16 acc[2];
      warp_layer4_bwd(acc, dz4, lds, lane);
      float H3[32];
      load_rows<32>(svb, sv::K1_H3, H3, s, h);
      dzs_layer<2, 2, 0, 0>(accW, bsum, st, pos, b0, b1, b1);   // layer4: dz4 x H3
      relu_gate<32>(dz3, H3, acc);
    }
    dzs_wave_sync();
    dzs_write(st, dz3, pos);
    dzs_wave_sync();
    row16_load(b0, svb, sv::K1_X0 + s, h);
    row16_load(b1, svb, sv::K1_X0 + 32 + s, h);
    row16_load(b2, svb, sv::K1_T + s, h);
    f32x16 accX[2], accT[1];
    {
      float dXh[32];
      load_rows<32>(gb, sv::K1G_DX0, dXh, s, h);
#pragma unroll
      for (int kk = 0; kk < 32; ++kk) accX[kk >> 4][kk & 15] = dXh[kk];
    }
    warp_layer3_bwd(accX, accT, dz3, lds, lane);
    dzs_layer<2, 3, 4, 2>(accW, bsum, st, pos, b0, b1, b2);   // layer3: dz3 x [X0 | T]
    warp_x0_bwd<true>(g, accX, svb, s, h);
    if constexpr (GX)
      tile_add3(a.g_xyz + (size_t)n * 96, act && h == 0, s, g.dn0 * a.box.inv[0] + g.gp0, g.dn1 * a.box.inv[1] + g.gp1, g.dn2 * a.box.inv[2] + g.gp2);
    {
      // d(tout) of the tile's rays, as k_dyn_density_bwd<1, false, true> (dtout_segments); the first lane of a segment stores -- to
      // dtout (ray inside the tile: a buffer over the tile's rays) or to one of the tile's two partial records in dtp (a buffer
      // over the tile's 256 bytes); the other lanes and the other buffer: out of range
      const DtoutSeg sg = dtout_segments(a, n, s);
      const int nl0 = (n * 32) / a.S;
      const int nrays = a.N - nl0 < 32 ? a.N - nl0 : 32;
      const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc((void*)(a.dtout + (size_t)nl0 * 32), 0, nrays * 128, 0x00020000);
      const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)(a.dtp + (size_t)n * 64), 0, 256, 0x00020000);
      const int offt = (sg.head && sg.inside) ? (sg.nl - nl0) * 128 + h * 16 : 1 << 20;
      const int offq = (sg.head && !sg.inside) ? (s == 0 ? 0 : 128) + h * 16 : 1 << 20;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = 0.f + accT[0][i];   // (dTacc of the other kernel: 0.f + the tile's product)
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) {
          const float o = __shfl_down(v, d, 32);
          v += s + d <= sg.end ? o : 0.f;
        }
        const int eo = (8 * (i >> 2) + (i & 3)) * 4;   // elem_of(i, h) = 8 (i >> 2) + 4 h + (i & 3)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rt, offt, eo, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rq, offq, eo, 0);
      }
    }
  }
  // cross-wave sum in wave order (layout: fused_red_floats), then one flush per workgroup
  float sm[wpd::NSM];
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    sm[o] = sw[o];
    sm[3 + o] = wave_sum(h == 0 ? sb[o] : 0.f);   // both halves hold the same samples
  }
  float* red = lds;
  for (int w = 0; w < nwaves; ++w) {
    __syncthreads();   // (the first: every wave is done with the image and its stage)
    if (wave == w) {
#pragma unroll
      for (int p = 0; p < wpd::NPROD; ++p)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          float* r = red + p * 1024 + rr * 64 + lane;
          *r = w == 0 ? accW[p][rr] : *r + accW[p][rr];
        }
#pragma unroll
      for (int i = 0; i < wpd::NDZ; ++i) {
        float* r = red + wpd::NPROD * 1024 + i * 64 + lane;
        *r = w == 0 ? bsum[i] : *r + bsum[i];
      }
#pragma unroll
      for (int i = 0; i < wpd::NSM; ++i) {
        float* r = red + wpd::NPROD * 1024 + (wpd::NDZ + i) * 64 + lane;
        *r = w == 0 ? sm[i] : *r + sm[i];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < wpd::NPROD; ++p) {
    // product p: layer4 (p < 4): dz block p >> 1, input block p & 1; layer3: dz block (p - 4) / 3, input block (p - 4) % 3
    const bool l4 = p < 4;
    const int bo = l4 ? p >> 1 : (p - 4) / 3, k = l4 ? p & 1 : (p - 4) % 3;
    fused_flush_tile(red + p * 1024, l4 ? G.l4w : G.l3w, bo * 32, l4 ? 64 : 93, l4 ? SEG_IDENT : (k < 2 ? SEG_WARP3_X0 : SEG_WARP3_T),
                     k < 2 ? 32 * k : 0);
  }
#pragma unroll
  for (int i = 0; i < wpd::NDZ; ++i) fused_flush_bias(red + wpd::NPROD * 1024 + i * 64, (i < 2 ? G.l4b : G.l3b) + (i & 1) * 32);
  // the 3-row layer: lane (s, h) of every wave holds input element elem_of(s, h) of the three rows; every lane the rows' bias sums
  for (int e = threadIdx.x; e < 3 * 64 + 3; e += blockDim.x) {
    const float* r = red + wpd::NPROD * 1024 + wpd::NDZ * 64;
    if (e < 192) grad_add(gw.l5w + (e >> 6) * 64 + elem_of(e & 31, (e >> 5) & 1), r[e]);
    else grad_add(gw.l5b + (e - 192), r[(3 + e - 192) * 64]);
  }
}

// host side (rdrf_bwd_host.hpp)
int launch_scene_flow_fused(int N, int S, const Box& box, const float* pkimg, const float* saved, const float* g_sf_f,
                            const float* g_sf_b, const RdrfDynamicParams* G, float* g_pts, long tiles, hipStream_t stream) {
  int grid, waves;
  fused_dw_geometry(tiles, &grid, &waves);
  SfGrads sg;
  for (int i = 0; i < 4; ++i) { sg.w[i] = G->sfw[i]; sg.b[i] = G->sfb[i]; }
  if (g_pts != nullptr)
    RDRF_LAUNCH("scene_flow_bwd", k_scene_flow_bwd_dw<true>, dim3(grid), dim3(64 * waves), stream, N, S, box, pkimg, saved, g_sf_f, g_sf_b, sg, g_pts);
  else
    RDRF_LAUNCH("scene_flow_bwd", k_scene_flow_bwd_dw<false>, dim3(grid), dim3(64 * waves), stream, N, S, box, pkimg, saved, g_sf_f, g_sf_b, sg, g_pts);
  return 0;
}
int launch_warp_fused(const BwdArgs& a, const DynG& gw, const RdrfDynamicParams* G, long tiles, hipStream_t stream) {
  int grid, waves;
  fused_dw_geometry(tiles, &grid, &waves);
  WarpGrads wg;
  wg.l3w = G->l3w; wg.l3b = G->l3b; wg.l4w = G->l4w; wg.l4b = G->l4b;
  if (a.g_xyz != nullptr) RDRF_LAUNCH("dyn_warp_bwd", k_dyn_warp_bwd_dw<true>, dim3(grid), dim3(64 * waves), stream, a, gw, wg);
  else RDRF_LAUNCH("dyn_warp_bwd", k_dyn_warp_bwd_dw<false>, dim3(grid), dim3(64 * waves), stream, a, gw, wg);
  return 0;
}
