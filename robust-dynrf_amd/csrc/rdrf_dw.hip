// rdrf_dw.hip -- weight gradients of every MLP layer of the backward passes: dW = sum_samples dz (x) in on the fp32 MFMA.
// The backward-data kernels (rdrf_bwd.hip) wrote every dz as rows of 32 samples and the forward saved the layer inputs
// in the same layout ([tile][row][32 samples], rdrf_kernels.hpp namespace sv): a lane reads 64 contiguous bytes of a row
// (16 samples) straight into its operand registers, so nothing is transposed.  The entry points describe their products
// as jobs (dw_add / dw_blk); dw_launch plans them into launches of k_dw3.
// Host interface: rdrf_bwd_host.hpp.
//
// ROW CONTRACT.  k_dw3 multiplies whole 32-sample tiles: it knows no sample mask.  In every sample slot of every tile it walks,
// of every 32-row block that is an operand of a product -- the slots past `count` in the last compacted tile, the slots past S
// of a ragged ray tile, the slots of invalid samples -- the dz entry is ZERO and the activation entry is FINITE (0 x NaN and
// 0 x inf are NaN in the matrix unit, and one NaN poisons a whole gradient row).  This is a REQUIREMENT ON THE PRODUCERS of the
// rows, not on the allocators: the saved-row buffers and the workspace arrive uninitialised (torch.empty, reused across calls
// of other shapes) and nobody clears them.  So the backward-data kernels (rdrf_bwd.hip) have to store every dz row a job names
// with all 32 lanes of the tile's wave, a lane without a live sample storing 0, and the forward kernels (rdrf_fwd_dev.hpp)
// every activation row likewise, a lane without a sample storing a finite value.  tests/test_gpu_poisoned_scratch.py holds them
// to it: it runs every entry point on buffers pre-filled with NaN bytes.  The kernel's side is checked on its own by
// tests/test_gpu_dw_primitives.py through rdrf_selftest_dw (rdrf_selftest.hip: the product's job lists on rows a test
// supplies): 3e38 behind a zero dz changes no bit.  Tiles past ceil(count / 32) are not read.  Rows of a dz block past a job's
// out_dim are multiplied and their products dropped at the write-out (rows of the product are independent): they need not hold
// anything.  Rows that are operands of no product are, as a rule, NOT READ at all: a plan addresses up to DW2_MAX_SEG runs of
// consecutive rows, which covers every list of the flat training path (one dz run; [X0, X1], [FD], [FB]) without a filler.  Only
// a list with more runs than that (the two-kernel warp lists with both heads live: two dz runs, three activation runs) has its
// smallest hole staged as a bridge block, which no product reads (dw_plan; tests/test_dw_plan_cpu.py counts them).
#include <algorithm>
#include <vector>

#include "rdrf_kernels.hpp"
#include "rdrf_bwd_host.hpp"

RDRF_DET_UNIT(dw)

// ------------------------------------------------------------------------------------------------
// dW jobs (DwJob, DwJobs: rdrf_bwd_host.hpp)
// ------------------------------------------------------------------------------------------------
void dw_add(DwJobs& D, const float* A, int A_stride, int A_row0, int nbo, int out_dim,
            int out_row0, const float* B, int B_stride, int in_dim, int ld, float* dW,
            float* db, const int* count, int ntiles) {
  DwJob& j = D.j[D.n];
  memset(&j, 0, sizeof(j));
  j.A = A; j.A_stride = A_stride; j.A_row0 = A_row0; j.nbo = nbo; j.out_dim = out_dim;
  j.out_row0 = out_row0; j.B = B; j.B_stride = B_stride; j.nblk = 0; j.in_dim = in_dim; j.ld = ld;
  j.dW = dW; j.db = db; j.count = count; j.ntiles = ntiles;
  D.n++;
}
void dw_blk(DwJobs& D, int row0, int seg, int e0) {
  DwJob& j = D.j[D.n - 1];
  j.blk_row0[j.nblk] = row0; j.blk_seg[j.nblk] = seg; j.blk_e0[j.nblk] = e0;
  j.nblk++;
}
// ------------------------------------------------------------------------------------------------
// cooperative dW plan (Dw2Plan; the names keep the spelling of the first kernel that ran it).  ONE 12-wave workgroup owns a
// tile: it stages every unique 32-row block of the tile in LDS once (27 blocks for the density phase, 30 for the appearance
// phases -- a density-phase tile would be requested 55 blocks at a time if every product fetched its own operands), then its
// waves form all (dz block) x (input block) products of all the jobs from that stage -- up to DW2_MAX_PROD products per wave,
// accumulators resident for the whole launch.  The rows of the next step are in flight while the MFMAs of the current one run.
// The heads' first-layer products that are left of the density phase on the flat training path are far smaller: 8 or 13 blocks
// and 12 or 24 products.
// ------------------------------------------------------------------------------------------------
#define DW2_MAX_BLK 30
#define DW2_MAX_PROD 4
#define DW2_WAVES 12
#define DW2_MAX_SEG 4
struct Dw2Prod {     // 32-bit fields: scalar loads (see blk_meta)
  int a, b;          // staged block indices of the dz block / the input block
  int job, bo, k;    // write-out: job, out-block of the job, in-block index of the job
  int bias;          // this product also accumulates the bias gradient of its out-block
};
struct Dw2Plan {
  const float* A;    // dz rows: tile t, row r at A + (t*A_stride + r)*32
  const float* B;    // activation rows
  int A_stride, B_stride;
  int nblk;
  int blk_meta[DW2_MAX_BLK];        // (src << 16) | row0, src 0 = A, 1 = B.  32-bit on purpose: the block index is
                                    // wave-uniform, so these are SCALAR loads (lgkmcnt); byte / short fields
                                    // compile to vector loads whose vmcnt(0) waits drain the data loads in flight
  // the staged blocks, sorted by (source, first row), form at most DW2_MAX_SEG runs of consecutive rows: a run
  // is ONE contiguous byte range per tile, so a slot's address needs no per-block metadata (see k_dw3).  Four runs are one
  // dz run and the three activation runs [X0, X1], [FD], [FB] of the density phase, or any other split; dw_plan bridges
  // holes only where a list has more
  int nseg;
  int seg_blk0[DW2_MAX_SEG];          // first staged block of the run (runs past nseg: past every block)
  int seg_src[DW2_MAX_SEG];           // 0 = A, 1 = B
  int seg_row0[DW2_MAX_SEG];          // first row of the run inside a tile
  int nprod[DW2_WAVES];
  Dw2Prod prod[DW2_WAVES][DW2_MAX_PROD];
  const int* count;
  int ntiles;
  DwJob job[RDRF_MAX_DW_JOBS];
};

// ------------------------------------------------------------------------------------------------
// k_dw3 (round 6): the plan above on HALF stages with LDS-DMA.  A stage is 16 samples x all rows (64 bytes of
// every row, 54-60 KB), there are two of them, and `buffer_load_dwordx4 ... lds` moves a half stage straight from HBM into the
// buffer that is not being read: step s = barrier; issue the DMA of step s + 1; the products of step s (8 MFMAs each, K = 16
// samples).  One barrier per half stage, no staging registers, no LDS write instructions.  Its predecessor k_dw2 (removed)
// staged a whole tile (32 samples x all rows, 108-120 KB of the 160 KB LDS) through registers: barrier, ten ds_write_b128 per
// thread, barrier, the products -- the matrix pipes waited during the write pass and both barriers (3 x (64 MFMA + 4 VALU cycles)
// accounted for 0.66 of its wave cycles), and nothing could be double-buffered.
// Measured (profiles/r06_ab_dw3_*.txt): dw launches 2.02 -> 1.91 ms/step at stage 0, 4.40 -> 4.10 at the final stage.  Ablations:
// MFMAs + barriers alone 1.05 ms (dw_dyn, stage 0), DMA + barriers alone 1.29 -- the memory side binds, and NOT through its
// latency: a ring of 80 block slots that keeps two half stages in flight (counted vmcnt, raw s_barrier) left the DMA-only time
// at 1.30 ms and made the kernel slower (1.56).  Nor through the 64-byte half rows: the same bytes fetched as full 128-byte
// rows (wrong arithmetic, timing only: profiles/r06_ab_dw3_fullrow_timing.txt) take 1.18 instead of 1.25 ms
// DMA-only and 1.43 instead of 1.47 ms in the whole kernel.  What is left is the per-step bubble of a 12-wave workgroup:
// vmcnt(0) -> barrier -> ~5 DMA issues per wave, during which this CU has nothing in flight (~0.5 of each 2.7 us step).
// Two workgroups per CU (profiles/r15_ab_dw_runs.txt): where a plan is small enough (k_dw3<2>, at most 80 KB of LDS) a second
// co-resident workgroup issues into that bubble: stage 0 step 8.630 -> 8.571 ms on top of the runs (8.756 -> 8.630: no bridge blocks).
//   LDS image of a block (32 rows x 16 samples = 2 KB): float4 position p = row * 4 + (chunk ^ ((row >> 2) & 3)); a DMA
//   instruction fills 1 KB in lane order (base + lane * 16 -- the hardware's layout), so the swizzle sits on the SOURCE
//   address of lane l (row = 16 sub + (l >> 2), chunk = (l & 3) ^ ((row >> 2) & 3)) and on the read (cdna guide, rule 21);
//   the 16 lanes of a ds_read_b128 group then cover all 64 banks.
// ------------------------------------------------------------------------------------------------
// NACC: accumulator sets of a wave (products it can carry).  The 2-set form is for plans whose waves hold at most two products (the
// heads' first layers of the flat training path): 32 accumulator registers fewer, so that two workgroups share a CU (dw_plan).
template <int NACC>
__global__ __launch_bounds__(64 * DW2_WAVES) void k_dw3(Dw2Plan P) {
  extern __shared__ __attribute__((aligned(16))) f32x4 dw3_stage[];   // 2 buffers x nblk x 128 float4
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, li = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntiles = P.count ? ((*P.count + 31) >> 5) : P.ntiles;
  static_assert((DW2_WAVES & 1) == 0, "a wave's pieces share their parity");
  const int npieces = 2 * P.nblk;   // 1 KB pieces (16 rows x 64 B) of a half stage
  constexpr int NPW = (2 * DW2_MAX_BLK + DW2_WAVES - 1) / DW2_WAVES;   // pieces per wave: 5
  // A wave's pieces (wave, wave + 12, ...) are the same blocks in every step, so the run of each is chosen ONCE, here, by a
  // chain of wave-uniform selects over the run boundaries: piece i of tile t lies at pbase[i] + t * pstep[i] + block * 4 KB.
  // Scalar registers only; the issue loop below adds a multiply and an add per piece and no load of any kind.
  const float* pbase[NPW];
  unsigned pstep[NPW];   // floats per tile of the piece's source
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    const int blk = (wave + DW2_WAVES * i) >> 1;
    int src = P.seg_src[0], row0 = P.seg_row0[0], b0 = 0;
#pragma unroll
    for (int q = 1; q < DW2_MAX_SEG; ++q) {
      const bool in = blk >= P.seg_blk0[q];
      src = in ? P.seg_src[q] : src; row0 = in ? P.seg_row0[q] : row0; b0 = in ? P.seg_blk0[q] : b0;
    }
    pbase[i] = (src ? P.B : P.A) + (ptrdiff_t)row0 * 32 - (ptrdiff_t)b0 * 1024;
    pstep[i] = (unsigned)(src ? P.B_stride : P.A_stride) * 32u;
  }
  // the lane's source offset inside a piece (bytes): row (l >> 2) of the piece's 16, chunk swizzled by the row
  // (a wave's pieces wave, wave + 12, ... all have the parity of the wave: one offset register)
  const int prow_ = 16 * (wave & 1) + (lane >> 2);
  const unsigned voff = (unsigned)(prow_ * 128 + (((lane & 3) ^ ((prow_ >> 2) & 3)) << 4));
  const int hbuf = P.nblk * 128;   // float4 per buffer
  auto dma = [&](int t, int hf, int buf) {
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      const int pc = wave + DW2_WAVES * i;   // wave-uniform
      if (pc < npieces) {
        const int blk = pc >> 1;
        const float* g = pbase[i] + (size_t)t * pstep[i];
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)g, 0, 0x7fffffff, 0x00020000);
        __attribute__((address_space(3))) void* dst = (__attribute__((address_space(3))) void*)(dw3_stage + buf * hbuf + pc * 64);
        const unsigned soff = (unsigned)(blk * 4096 + hf * 64);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst, 16, voff, soff, 0, 0);
      }
    }
  };
  int rpos[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) rpos[q] = li * 4 + ((2 * h + q) ^ ((li >> 2) & 3));
  const int np = P.nprod[wave];
  int pa[NACC], pb[NACC];   // staged block offsets (float4) of each product, bias flag in bit 30 of pa (scalars)
#pragma unroll
  for (int p = 0; p < NACC; ++p) {
    pa[p] = __builtin_amdgcn_readfirstlane(P.prod[wave][p].a * 128 | (P.prod[wave][p].bias << 30));
    pb[p] = __builtin_amdgcn_readfirstlane(P.prod[wave][p].b * 128);
  }
  f32x16 acc[NACC];
  float bsum[NACC];
#pragma unroll
  for (int p = 0; p < NACC; ++p) {
    bsum[p] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
  }
  int t = blockIdx.x, hf = 0, buf = 0;
  if (t < ntiles) dma(t, 0, 0);
  while (t < ntiles) {
    // this wave's DMA pieces of the current half stage have landed; behind the barrier everybody's have, and everybody is
    // done reading the other buffer (the products of the previous step)
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0) (expcnt / lgkmcnt untouched)
    __syncthreads();
    int tn = t, hn = hf ^ 1;
    if (hf) tn = t + gridDim.x;
    if (tn < ntiles) dma(tn, hn, buf ^ 1);   // lands while the MFMAs below run
    __builtin_amdgcn_sched_barrier(0);       // (issued BEFORE the products: hipcc is free to sink it below them otherwise)
    const f32x4* stage = dw3_stage + buf * hbuf;
#pragma unroll
    for (int p = 0; p < NACC; ++p) {
      if (p < np) {
        int oa = pa[p] & 0xffffff, ob = pb[p];
        // (opaque to the optimiser: with loop-invariant offsets it hoists the LDS read addresses of the four products out of
        // the tile loop and spills them -- reloads whose vmcnt(0) drain the DMA in flight)
        asm volatile("" : "+s"(oa), "+s"(ob));
        const f32x4* sa = stage + oa;
        const f32x4* sb = stage + ob;
        f32x4 av4[2], bv4[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) { av4[q] = sa[rpos[q]]; bv4[q] = sb[rpos[q]]; }
        if (pa[p] >> 30) {
#pragma unroll
          for (int q = 0; q < 2; ++q) bsum[p] += av4[q].x + av4[q].y + av4[q].z + av4[q].w;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av4[q].x, bv4[q].x, acc[p], 0, 0, 0);
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av4[q].y, bv4[q].y, acc[p], 0, 0, 0);
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av4[q].z, bv4[q].z, acc[p], 0, 0, 0);
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av4[q].w, bv4[q].w, acc[p], 0, 0, 0);
        }
      }
    }
    t = tn; hf = hn; buf ^= 1;
  }
#pragma unroll
  for (int p = 0; p < NACC; ++p) {
    if (p < np) {
      const Dw2Prod pr = P.prod[wave][p];
      const DwJob& J = P.job[pr.job];
      const int col = seg_imap(J.blk_seg[pr.k], J.blk_e0[pr.k] + li, J.in_dim);
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int orow = pr.bo * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * h - J.out_row0;
        if (col >= 0 && orow >= 0 && orow < J.out_dim) grad_add(J.dW + (size_t)orow * J.ld + col, acc[p][rr]);
      }
      if (pr.bias && J.db != nullptr) {
        const float b = bsum[p] + __shfl_xor(bsum[p], 32, 64);
        const int orow = pr.bo * 32 + li - J.out_row0;
        if (h == 0 && orow >= 0 && orow < J.out_dim) grad_add(J.db + orow, b);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// planning (host code only, no HIP call: rdrf_selftest_dw_plan runs it on a machine without a GPU)
// ------------------------------------------------------------------------------------------------
struct DwLaunch {
  Dw2Plan P;
  int grid, lds;   // workgroups, dynamic LDS bytes
  int nacc;        // accumulator sets of the instantiation: 2 or DW2_MAX_PROD
};
#define DW2_LDS_PER_CU (160 * 1024)
// Workgroups of k_dw3<2> that share a CU as far as registers go: tools/kernel_resources.py shows the instantiation at 6 or more
// waves per SIMD without spill or scratch, and a 12-wave workgroup is 3 waves per SIMD.  k_dw3<4> (5 waves per SIMD): one.
#define DW2_WG_PER_CU_2ACC 2

// close a plan: stage order, runs, launch shape
static int dw_close_plan(Dw2Plan& P, std::vector<DwLaunch>& out) {
  int tot = 0, most = 0;
  for (int w = 0; w < DW2_WAVES; ++w) { tot += P.nprod[w]; most = P.nprod[w] > most ? P.nprod[w] : most; }
  if (tot == 0) return 0;
  auto count_runs = [&](const int* meta, int n) {
    int runs = 0;
    for (int i = 0; i < n; ++i) runs += i == 0 || meta[i] != meta[i - 1] + 32;   // (a change of source is no + 32 either)
    return runs;
  };
  // stage order = (source, first row) order.  Only operand blocks are staged; where that leaves more runs of consecutive rows than
  // the kernel addresses, the hole with the fewest blocks is filled with bridge blocks (staged, read by no product) until it does
  for (;;) {
    int meta[DW2_MAX_BLK];
    for (int i = 0; i < P.nblk; ++i) meta[i] = P.blk_meta[i];
    std::sort(meta, meta + P.nblk);
    if (count_runs(meta, P.nblk) <= DW2_MAX_SEG) break;
    int best = -1, best_n = 1 << 30;
    for (int i = 1; i < P.nblk; ++i) {
      if ((meta[i] >> 16) != (meta[i - 1] >> 16)) continue;
      const int n = ((meta[i] & 0xffff) - (meta[i - 1] & 0xffff)) / 32 - 1;
      if (n > 0 && n < best_n) { best = i; best_n = n; }
    }
    RDRF_CHECK(best >= 0 && P.nblk + best_n <= DW2_MAX_BLK, -2,
               "dw: the staged rows form more than %d contiguous runs and %d staged blocks are not enough to bridge them", DW2_MAX_SEG,
               DW2_MAX_BLK);
    for (int r = (meta[best - 1] & 0xffff) + 32; r < (meta[best] & 0xffff); r += 32) P.blk_meta[P.nblk++] = (meta[best] & ~0xffff) | r;
  }
  {
    int order[DW2_MAX_BLK], rank[DW2_MAX_BLK], meta[DW2_MAX_BLK];
    for (int i = 0; i < P.nblk; ++i) order[i] = i;
    std::sort(order, order + P.nblk, [&](int x, int y) { return P.blk_meta[x] < P.blk_meta[y]; });
    for (int i = 0; i < P.nblk; ++i) { rank[order[i]] = i; meta[i] = P.blk_meta[order[i]]; }
    for (int i = 0; i < P.nblk; ++i) P.blk_meta[i] = meta[i];
    for (int w = 0; w < DW2_WAVES; ++w)
      for (int k = 0; k < P.nprod[w]; ++k) { P.prod[w][k].a = rank[P.prod[w][k].a]; P.prod[w][k].b = rank[P.prod[w][k].b]; }
    P.nseg = 0;
    for (int i = 0; i < P.nblk; ++i) {
      if (i == 0 || meta[i] != meta[i - 1] + 32) {
        RDRF_CHECK(P.nseg < DW2_MAX_SEG, -2, "dw: the staged rows form more than %d contiguous runs", DW2_MAX_SEG);
        P.seg_blk0[P.nseg] = i; P.seg_src[P.nseg] = meta[i] >> 16; P.seg_row0[P.nseg] = meta[i] & 0xffff;
        ++P.nseg;
      }
    }
    for (int q = P.nseg; q < DW2_MAX_SEG; ++q) P.seg_blk0[q] = 1 << 20;   // never selected
  }
  DwLaunch L;
  L.lds = P.nblk * 4096;   // two half stages of nblk x 2 KB
  L.nacc = most <= 2 ? 2 : DW2_MAX_PROD;
  int per_cu = DW2_LDS_PER_CU / L.lds;
  if (per_cu > (L.nacc == 2 ? DW2_WG_PER_CU_2ACC : 1)) per_cu = L.nacc == 2 ? DW2_WG_PER_CU_2ACC : 1;
  L.grid = 256 * per_cu;
  if (P.count == nullptr && P.ntiles < L.grid) L.grid = P.ntiles < 1 ? 1 : P.ntiles;
  L.P = P;
  out.push_back(L);
  return 0;
}

// one plan per group of jobs that walk the same rows (same dz array, same activation array, same tile
// space); a group whose products or blocks exceed one plan is cut into several launches
static int dw_plan(const DwJobs& D, std::vector<DwLaunch>& out) {
  bool done[RDRF_MAX_DW_JOBS] = {false};
  for (int g0 = 0; g0 < D.n; ++g0) {
    if (done[g0]) continue;
    const DwJob& R = D.j[g0];
    Dw2Plan P;
    auto reset = [&]() {
      memset(&P, 0, sizeof(P));
      P.A = R.A; P.B = R.B; P.A_stride = R.A_stride; P.B_stride = R.B_stride;
      P.count = R.count; P.ntiles = R.ntiles;
      for (int i = 0; i < D.n; ++i) P.job[i] = D.j[i];
    };
    auto find_blk = [&](int src, int row) {
      for (int i = 0; i < P.nblk; ++i)
        if (P.blk_meta[i] == ((src << 16) | row)) return i;
      return -1;
    };
    reset();
    int nprods = 0;
    for (int ji = g0; ji < D.n; ++ji) {
      const DwJob& J = D.j[ji];
      if (done[ji] || J.A != R.A || J.B != R.B || J.A_stride != R.A_stride || J.B_stride != R.B_stride ||
          J.count != R.count || J.ntiles != R.ntiles)
        continue;
      done[ji] = true;
      for (int bo = 0; bo < J.nbo; ++bo)
        for (int k = 0; k < J.nblk; ++k) {
          int need = (find_blk(0, J.A_row0 + 32 * bo) < 0) + (find_blk(1, J.blk_row0[k]) < 0);
          if (nprods == DW2_WAVES * DW2_MAX_PROD || P.nblk + need > DW2_MAX_BLK) {
            int rc = dw_close_plan(P, out);
            if (rc) return rc;
            reset();
            nprods = 0;
          }
          int a = find_blk(0, J.A_row0 + 32 * bo);
          if (a < 0) { a = P.nblk++; P.blk_meta[a] = J.A_row0 + 32 * bo; }
          int b = find_blk(1, J.blk_row0[k]);
          if (b < 0) { b = P.nblk++; P.blk_meta[b] = (1 << 16) | J.blk_row0[k]; }
          const int w = nprods % DW2_WAVES;   // round robin: consecutive products of a job share their dz block
          Dw2Prod& pr = P.prod[w][P.nprod[w]++];
          pr.a = a; pr.b = b; pr.job = ji; pr.bo = bo; pr.k = k;
          pr.bias = (k == 0 && J.db != nullptr) ? 1 : 0;
          ++nprods;
        }
    }
    int rc = dw_close_plan(P, out);
    if (rc) return rc;
  }
  return 0;
}

// the launches dw_launch would make for these jobs, as ints (layout: rdrf_selftest_dw_plan, rdrf_selftest.hip)
int dw_describe_launches(const DwJobs& D, int* out, int cap) {
  std::vector<DwLaunch> Ls;
  int rc = dw_plan(D, Ls);
  if (rc) return rc;
  int need = 2;
  for (const DwLaunch& L : Ls) {
    need += 5 + 3 * L.P.nseg + 2 * L.P.nblk + DW2_WAVES;
    for (int w = 0; w < DW2_WAVES; ++w) need += 5 * L.P.nprod[w];
  }
  RDRF_CHECK(out != nullptr && cap >= need, -3, "selftest_dw_plan: description buffer too small (%d < %d ints)", out ? cap : 0, need);
  int n = 0;
  out[n++] = need; out[n++] = (int)Ls.size();
  for (const DwLaunch& L : Ls) {
    const Dw2Plan& P = L.P;
    out[n++] = L.grid; out[n++] = L.lds; out[n++] = L.nacc; out[n++] = P.nblk; out[n++] = P.nseg;
    for (int q = 0; q < P.nseg; ++q) { out[n++] = P.seg_src[q]; out[n++] = P.seg_row0[q]; out[n++] = P.seg_blk0[q]; }
    for (int i = 0; i < P.nblk; ++i) { out[n++] = P.blk_meta[i] >> 16; out[n++] = P.blk_meta[i] & 0xffff; }
    for (int w = 0; w < DW2_WAVES; ++w) {
      out[n++] = P.nprod[w];
      for (int k = 0; k < P.nprod[w]; ++k) {
        const Dw2Prod& pr = P.prod[w][k];
        out[n++] = pr.a; out[n++] = pr.b; out[n++] = pr.job; out[n++] = pr.bo; out[n++] = pr.k;
      }
    }
  }
  return n;
}

template <int NACC>
static int dw_launch_one(const DwLaunch& L, hipStream_t stream, const char* name) {
  // (per instantiation: the attribute belongs to the function)
  if (L.lds > 48 * 1024)
    RDRF_HIP(hipFuncSetAttribute((const void*)k_dw3<NACC>, hipFuncAttributeMaxDynamicSharedMemorySize, DW2_MAX_BLK * 4096));
  rdrf_prof_begin(name, stream);
  hipLaunchKernelGGL(k_dw3<NACC>, dim3(L.grid), dim3(64 * DW2_WAVES), (size_t)L.lds, stream, L.P);
  rdrf_prof_end(name, stream);
  RDRF_HIP(hipGetLastError());
  return 0;
}

// plans the jobs (dw_plan) and launches exactly what the planning describes, in its order
int dw_launch(DwJobs& D, hipStream_t stream, const char* name) {
  std::vector<DwLaunch> Ls;
  int rc = dw_plan(D, Ls);
  if (rc) return rc;
  for (const DwLaunch& L : Ls) {
    rc = L.nacc == 2 ? dw_launch_one<2>(L, stream, name) : dw_launch_one<DW2_MAX_PROD>(L, stream, name);
    if (rc) return rc;
  }
  return 0;
}
