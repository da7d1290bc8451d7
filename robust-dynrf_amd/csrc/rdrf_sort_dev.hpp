// rdrf_sort_dev.hpp -- what the segmented radix sort (rdrf_sort.hip) and a kernel that builds the first pass's tile
// histograms for it (k_sort_keys, rdrf_scatter.hip) must agree on: the tile size, the pass / digit plan and the layout of
// the histogram and drop-count tables.
#pragma once
#include <cstddef>

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_TILE = 2048;                  // entries per workgroup (8192 -> 2048: sort -11 % at stage 0, -12 % at the final stage, profiles/r06_ab_sort_tile.txt)
constexpr int RS_PER_WAVE = RS_TILE / RS_WAVES;
constexpr int RS_ROUNDS = RS_PER_WAVE / 64;    // 64-entry rounds per wave
constexpr int RS_MAX_DIGIT_BITS = 9;
constexpr int RS_BINS = 1 << RS_MAX_DIGIT_BITS;

// LSD passes over `bits` bits: the fewest passes of <= RS_MAX_DIGIT_BITS, digits as even as they come (the last may be short)
inline int radix_plan(int bits, int& passes, int& digit_bits) {
  if (bits < 1) bits = 1;
  passes = (bits + RS_MAX_DIGIT_BITS - 1) / RS_MAX_DIGIT_BITS;
  digit_bits = (bits + passes - 1) / passes;
  return passes;
}

// tiles of a segment of seg_len entries (a tile never spans two segments)
inline __host__ __device__ unsigned rs_tiles(unsigned seg_len) { return (seg_len + RS_TILE - 1) / RS_TILE; }

// Tables of one pass.  tps = tiles per segment the launch was sized for (the host-side maximum; with a device-side
// segment length only the first rs_tiles(length) entries of a row are written and read).
//   hist   [segment][digit][tile]   a tile's count of the digit; the row-wise exclusive scan orders equal digits by tile
//   drops  [segment][tile]          entries of the tile that the key kernel dropped (first pass of the sorted scatter)
inline __host__ __device__ size_t rs_hist_at(int seg, int nbins, unsigned digit, unsigned tps, unsigned tile) {
  return ((size_t)seg * nbins + digit) * tps + tile;
}
inline __host__ __device__ size_t rs_drops_at(int seg, unsigned tps, unsigned tile) { return (size_t)seg * tps + tile; }

// where the tables of a sort over (nseg, seg_len) lie inside its temporary storage (rdrf_sort_carve): the key kernel
// writes the first pass's hist / drops there before rdrf_sort_positions_seg runs
struct RsTables {
  unsigned* hist;     // [nseg][RS_BINS rows at most][tps]
  unsigned* totals;   // [nseg][nbins]
  unsigned* drops;    // [nseg][tps]
  unsigned tps;
};
