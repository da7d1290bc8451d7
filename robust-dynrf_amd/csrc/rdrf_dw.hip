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
// out_dim are multiplied and their products dropped at the write-out (rows of the product are independent), and the blocks
// dw_launch stages only to bridge a hole in the row ranges (a pruned head) are operands of no product: neither needs to hold
// anything.
#include <algorithm>

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
// ------------------------------------------------------------------------------------------------
#define DW2_MAX_BLK 30
#define DW2_MAX_PROD 4
#define DW2_WAVES 12
#define DW2_MAX_SEG 2
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
  // is ONE contiguous byte range per tile, so a slot's address needs no per-block metadata (see k_dw3)
  int nseg;
  int seg_blk0[DW2_MAX_SEG];          // first staged block of the run
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
//   LDS image of a block (32 rows x 16 samples = 2 KB): float4 position p = row * 4 + (chunk ^ ((row >> 2) & 3)); a DMA
//   instruction fills 1 KB in lane order (base + lane * 16 -- the hardware's layout), so the swizzle sits on the SOURCE
//   address of lane l (row = 16 sub + (l >> 2), chunk = (l & 3) ^ ((row >> 2) & 3)) and on the read (cdna guide, rule 21);
//   the 16 lanes of a ds_read_b128 group then cover all 64 banks.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * DW2_WAVES) void k_dw3(Dw2Plan P) {
  extern __shared__ __attribute__((aligned(16))) f32x4 dw3_stage[];   // 2 buffers x nblk x 128 float4
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, li = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntiles = P.count ? ((*P.count + 31) >> 5) : P.ntiles;
  static_assert(DW2_MAX_SEG == 2 && (DW2_WAVES & 1) == 0, "segment select below; a wave's pieces share their parity");
  const int sb1 = P.nseg > 1 ? P.seg_blk0[1] : 1 << 20;
  const int s1 = P.nseg > 1 ? 1 : 0;
  const float* seg0a = (P.seg_src[0] ? P.B : P.A) + (size_t)P.seg_row0[0] * 32;
  const float* seg0b = (P.seg_src[s1] ? P.B : P.A) + (size_t)P.seg_row0[s1] * 32 - (size_t)P.seg_blk0[s1] * 1024;
  const size_t st0 = (size_t)(P.seg_src[0] ? P.B_stride : P.A_stride) * 32,
               st1 = (size_t)(P.seg_src[s1] ? P.B_stride : P.A_stride) * 32;
  const int npieces = 2 * P.nblk;   // 1 KB pieces (16 rows x 64 B) of a half stage
  constexpr int NPW = (2 * DW2_MAX_BLK + DW2_WAVES - 1) / DW2_WAVES;   // pieces per wave: 5
  // the lane's source offset inside a piece (bytes): row (l >> 2) of the piece's 16, chunk swizzled by the row
  // (a wave's pieces wave, wave + 12, ... all have the parity of the wave: one offset register)
  const int prow_ = 16 * (wave & 1) + (lane >> 2);
  const unsigned voff = (unsigned)(prow_ * 128 + (((lane & 3) ^ ((prow_ >> 2) & 3)) << 4));
  const int hbuf = P.nblk * 128;   // float4 per buffer
  auto dma = [&](int t, int hf, int buf) {
    const float* g0 = seg0a + (size_t)t * st0;
    const float* g1 = seg0b + (size_t)t * st1;
    const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc((void*)g0, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc((void*)g1, 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      const int pc = wave + DW2_WAVES * i;   // wave-uniform
      if (pc < npieces) {
        const int blk = pc >> 1;
        __attribute__((address_space(3))) void* dst = (__attribute__((address_space(3))) void*)(dw3_stage + buf * hbuf + pc * 64);
        const unsigned soff = (unsigned)(blk * 4096 + hf * 64);
        if (blk < sb1) __builtin_amdgcn_raw_ptr_buffer_load_lds(r0, dst, 16, voff, soff, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(r1, dst, 16, voff, soff, 0, 0);
      }
    }
  };
  int rpos[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) rpos[q] = li * 4 + ((2 * h + q) ^ ((li >> 2) & 3));
  const int np = P.nprod[wave];
  int pa[DW2_MAX_PROD], pb[DW2_MAX_PROD];   // staged block offsets (float4) of each product, bias flag in bit 30 of pa (scalars)
#pragma unroll
  for (int p = 0; p < DW2_MAX_PROD; ++p) {
    pa[p] = __builtin_amdgcn_readfirstlane(P.prod[wave][p].a * 128 | (P.prod[wave][p].bias << 30));
    pb[p] = __builtin_amdgcn_readfirstlane(P.prod[wave][p].b * 128);
  }
  f32x16 acc[DW2_MAX_PROD];
  float bsum[DW2_MAX_PROD];
#pragma unroll
  for (int p = 0; p < DW2_MAX_PROD; ++p) {
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
    for (int p = 0; p < DW2_MAX_PROD; ++p) {
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
  for (int p = 0; p < DW2_MAX_PROD; ++p) {
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

// one plan per group of jobs that walk the same rows (same dz array, same activation array, same tile
// space); a group whose products or blocks exceed one plan is cut into several launches
int dw_launch(DwJobs& D, hipStream_t stream, const char* name) {
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
    auto flush = [&]() -> int {
      int tot = 0;
      for (int w = 0; w < DW2_WAVES; ++w) tot += P.nprod[w];
      if (tot == 0) return 0;
      {  // one contiguous run per source: a pruned head leaves a hole in the row ranges (its dz / activation rows are
         // not part of any product); the hole's blocks are staged unused so that the two-run addressing holds
        for (int src = 0; src < 2; ++src) {
          int lo = 1 << 30, hi = -1;
          for (int i = 0; i < P.nblk; ++i)
            if ((P.blk_meta[i] >> 16) == src) { const int r = P.blk_meta[i] & 0xffff; lo = r < lo ? r : lo; hi = r > hi ? r : hi; }
          for (int r = lo; r < hi; r += 32)
            if (find_blk(src, r) < 0) {
              RDRF_CHECK(P.nblk < DW2_MAX_BLK, -2, "dw: %d staged blocks are not enough to bridge the row ranges of this plan", DW2_MAX_BLK);
              P.blk_meta[P.nblk++] = (src << 16) | r;
            }
        }
      }
      {  // stage order = (source, first row) order; runs of consecutive rows become segments
        int order[DW2_MAX_BLK], rank[DW2_MAX_BLK], meta[DW2_MAX_BLK];
        for (int i = 0; i < P.nblk; ++i) order[i] = i;
        std::sort(order, order + P.nblk, [&](int x, int y) { return P.blk_meta[x] < P.blk_meta[y]; });
        for (int i = 0; i < P.nblk; ++i) { rank[order[i]] = i; meta[i] = P.blk_meta[order[i]]; }
        for (int i = 0; i < P.nblk; ++i) P.blk_meta[i] = meta[i];
        for (int w = 0; w < DW2_WAVES; ++w)
          for (int k = 0; k < P.nprod[w]; ++k) { P.prod[w][k].a = rank[P.prod[w][k].a]; P.prod[w][k].b = rank[P.prod[w][k].b]; }
        P.nseg = 0;
        for (int i = 0; i < P.nblk; ++i) {
          if (i == 0 || (meta[i] >> 16) != (meta[i - 1] >> 16) || (meta[i] & 0xffff) != (meta[i - 1] & 0xffff) + 32) {
            RDRF_CHECK(P.nseg < DW2_MAX_SEG, -2, "dw: the staged rows form more than %d contiguous runs", DW2_MAX_SEG);
            P.seg_blk0[P.nseg] = i; P.seg_src[P.nseg] = meta[i] >> 16; P.seg_row0[P.nseg] = meta[i] & 0xffff;
            ++P.nseg;
          }
        }
      }
      const size_t lds = (size_t)P.nblk * 4096;   // two half stages of nblk x 2 KB
      int grid = 256;
      if (P.count == nullptr && P.ntiles < grid) grid = P.ntiles < 1 ? 1 : P.ntiles;
      if (lds > 48 * 1024)
        RDRF_HIP(hipFuncSetAttribute((const void*)k_dw3, hipFuncAttributeMaxDynamicSharedMemorySize, DW2_MAX_BLK * 4096));
      rdrf_prof_begin(name, stream);
      hipLaunchKernelGGL(k_dw3, dim3(grid), dim3(64 * DW2_WAVES), lds, stream, P);
      rdrf_prof_end(name, stream);
      RDRF_HIP(hipGetLastError());
      return 0;
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
            int rc = flush();
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
    int rc = flush();
    if (rc) return rc;
  }
  return 0;
}
