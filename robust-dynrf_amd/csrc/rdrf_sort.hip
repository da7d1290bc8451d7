// rdrf_sort.hip -- device-wide stable key sort for the sorted scatter (rdrf_scatter.hip), hand-written for gfx950.
//
// The keys are (plane | level-0 cell) codes of every live sample: 15-19 significant cell bits, a few million entries, the
// value of an entry is its position in the key array.  The sort is SEGMENTED: nseg independent stable sorts of seg_len
// consecutive entries each, over the low `bits` bits, inside the same launches (the sorted scatter lays the three planes'
// keys out back to back, so the plane bits above the cell bits need no sorting: rdrf_sort_positions_seg with nseg = 3,
// bits = kb).  rdrf_sort_positions / rdrf_sort_ints_inplace are the one-segment case.  An LSD radix sort over digits of
// <= 9 bits (two passes for up to 18 bits); a tile of 2048 entries never spans two segments; one pass =
//   k_radix_hist     a workgroup owns a tile; digit histogram of the tile in LDS, written [segment][digit][tile]
//                    (rdrf_sort_dev.hpp) so that a row-wise exclusive scan orders equal digits by tile.  The sorted
//                    scatter's key kernel writes the FIRST pass's histograms itself (and the tiles' dropped-key counts):
//                    that pass then starts at the scan
//   k_radix_scan     one workgroup per (segment, digit): exclusive scan of its row + the digit's total; with the key
//                    kernel's drop counts, one more workgroup per segment: counts[segment] = length - dropped
//   k_radix_scatter  the same tiles again: exclusive scan of the segment's digit totals in LDS, then a STABLE rank of
//                    every entry among the equal digits of its tile -- waves own contiguous quarters of the tile, a wave
//                    walks its quarter 64 entries at a time, equal digits inside a 64-entry round are ranked with nine
//                    ballots (the peers of a lane = the lanes whose digit agrees in every bit), per-(wave, digit) running
//                    offsets live in LDS.  The rank places key and value at the entry's TILE-LOCAL sorted slot in LDS;
//                    after a barrier thread i takes slot i and stores it to (global base of its digit) + (i - first slot
//                    of the digit), so consecutive lanes inside a digit's run store to consecutive addresses.
// No atomics with return values, no data-dependent loops, no workgroup waits on another.  Equal keys keep ascending position
// order (the deterministic build and the run reduction of the scatter rely on it).
#include <cstring>
#include <hip/hip_runtime.h>

#include "rdrf_host.hpp"
#include "rdrf_sort_dev.hpp"

namespace {
struct RadixArgs {
  const unsigned* keys_in;
  const unsigned* vals_in;   // nullptr: the value of an entry is its position
  unsigned* keys_out;
  unsigned* vals_out;        // nullptr: values are not wanted (key-only sort)
  unsigned* hist;            // [nseg][nbins][tps]
  unsigned* totals;          // [nseg][nbins]
  const unsigned* drops;     // [nseg][tps] dropped keys per tile (the key kernel's) ...
  int* counts;               // ... -> counts[segment] = length - dropped, by k_radix_scan (nullptr: no such workgroup)
  unsigned seg_len;          // entries per segment = the segment stride (the host-side maximum)
  unsigned tps;              // tiles per segment the launches are sized for
  int nseg, shift, nbins;
  const int* len_dev;        // device-side count: segments are min(seg_len, len_mul * *len_dev) entries long AND that far
  unsigned len_mul;          // apart (nullptr: seg_len).  Tiles beyond the device-side length find nothing to do
};
__device__ __forceinline__ unsigned radix_len(const RadixArgs& a) {
  if (a.len_dev == nullptr) return a.seg_len;
  const unsigned m = (unsigned)*a.len_dev * a.len_mul;
  return m < a.seg_len ? m : a.seg_len;
}

// (from the second pass on; the first one too where no key kernel has built its histograms)
__global__ __launch_bounds__(RS_THREADS) void k_radix_hist(RadixArgs a) {
  __shared__ unsigned h[RS_BINS];
  const unsigned len = radix_len(a), tile = blockIdx.x, t0 = tile * (unsigned)RS_TILE;
  const int seg = blockIdx.y;
  if (t0 >= len) return;   // (uniform: the whole tile lies beyond the device-side length; the scan reads no such tile)
  for (int i = threadIdx.x; i < a.nbins; i += RS_THREADS) h[i] = 0u;
  __syncthreads();
  const unsigned mask = (unsigned)a.nbins - 1u;
  const unsigned cnt = len - t0 < (unsigned)RS_TILE ? len - t0 : (unsigned)RS_TILE;
  const unsigned* k = a.keys_in + (size_t)seg * len + t0;
  for (unsigned i = threadIdx.x; i < cnt; i += RS_THREADS) atomicAdd(&h[(k[i] >> a.shift) & mask], 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < a.nbins; i += RS_THREADS) a.hist[rs_hist_at(seg, a.nbins, (unsigned)i, a.tps, tile)] = h[i];
}

// workgroup-wide exclusive scan of one value per thread (256 threads); returns the exclusive prefix, *total = the sum
__device__ __forceinline__ unsigned block_exscan(unsigned v, unsigned* wsum, unsigned* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  unsigned off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < RS_WAVES; ++w) {
    const unsigned s = wsum[w];
    if (w < wave) off += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return off + inc - v;
}

// grid (nbins [+ 1], nseg)
__global__ __launch_bounds__(RS_THREADS) void k_radix_scan(RadixArgs a) {
  __shared__ unsigned wsum[RS_WAVES];
  const unsigned len = radix_len(a), nt = rs_tiles(len);
  const int seg = blockIdx.y;
  if ((int)blockIdx.x == a.nbins) {   // the extra workgroup of a segment: live entries = length - the tiles' dropped keys
    const unsigned* dr = a.drops + rs_drops_at(seg, a.tps, 0);
    unsigned v = 0, tot;
    for (unsigned i = threadIdx.x; i < nt; i += RS_THREADS) v += dr[i];
    block_exscan(v, wsum, &tot);
    if (threadIdx.x == 0) a.counts[seg] = (int)(len - tot);
    return;
  }
  unsigned* row = a.hist + rs_hist_at(seg, a.nbins, blockIdx.x, a.tps, 0);
  unsigned carry = 0;
  for (unsigned i0 = 0; i0 < nt; i0 += RS_THREADS) {
    const unsigned i = i0 + threadIdx.x;
    const unsigned v = i < nt ? row[i] : 0u;
    unsigned tot;
    const unsigned ex = block_exscan(v, wsum, &tot);
    if (i < nt) row[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) a.totals[(size_t)seg * a.nbins + blockIdx.x] = carry;
}

// grid (tps, nseg)
__global__ __launch_bounds__(RS_THREADS) void k_radix_scatter(RadixArgs a) {
  __shared__ unsigned offs[RS_WAVES][RS_BINS];   // running tile-local slot of (wave, digit)
  __shared__ unsigned gd[RS_BINS];               // global base of the digit for this tile - the digit's first tile-local slot
  __shared__ unsigned wsum[RS_WAVES];
  __shared__ unsigned sk[RS_TILE], sv[RS_TILE];  // the tile in sorted order: keys, values
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned mask = (unsigned)a.nbins - 1u;
  const unsigned len = radix_len(a), tile = blockIdx.x, t0 = tile * (unsigned)RS_TILE;
  const int seg = blockIdx.y;
  if (t0 >= len) return;   // (uniform: the whole tile lies beyond the device-side length)
  const unsigned cnt = len - t0 < (unsigned)RS_TILE ? len - t0 : (unsigned)RS_TILE;
  const unsigned sbase = (unsigned)seg * len;    // global position of the segment's first entry (nseg * seg_len fits 32 bits)
  for (int i = threadIdx.x; i < RS_WAVES * RS_BINS; i += RS_THREADS) (&offs[0][0])[i] = 0u;
  __syncthreads();
  // ---- per-wave digit counts of the wave's quarter (keys and values stay in registers for the second sweep)
  const unsigned wl = (unsigned)wave * RS_PER_WAVE;
  unsigned key[RS_ROUNDS], val[RS_ROUNDS];
#pragma unroll
  for (int r = 0; r < RS_ROUNDS; ++r) {
    const unsigned i = wl + (unsigned)r * 64 + lane;
    const size_t p = (size_t)sbase + t0 + i;
    key[r] = i < cnt ? a.keys_in[p] : 0xffffffffu;
    val[r] = (i < cnt && a.vals_in) ? a.vals_in[p] : (unsigned)p;
    if (i < cnt) atomicAdd(&offs[wave][(key[r] >> a.shift) & mask], 1u);
  }
  __syncthreads();
  // ---- counts -> slots: the tile-exclusive scan of the digit counts + the counts of the lower waves; the digit's global
  // base = exclusive scan of the segment's totals + this tile's entry of the digit's row scan
  {
    unsigned carry_t = 0, carry_g = 0;
    for (int d0 = 0; d0 < a.nbins; d0 += RS_THREADS) {
      const int d = d0 + threadIdx.x;
      const bool in = d < a.nbins;
      unsigned c[RS_WAVES], ct = 0;
#pragma unroll
      for (int w = 0; w < RS_WAVES; ++w) { c[w] = in ? offs[w][d] : 0u; ct += c[w]; }
      const unsigned g = in ? a.totals[(size_t)seg * a.nbins + d] : 0u;
      unsigned tt, tg;
      const unsigned et = block_exscan(ct, wsum, &tt);
      const unsigned eg = block_exscan(g, wsum, &tg);
      if (in) {
        const unsigned first = carry_t + et;
        unsigned run = first;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) { offs[w][d] = run; run += c[w]; }
        gd[d] = sbase + carry_g + eg + a.hist[rs_hist_at(seg, a.nbins, (unsigned)d, a.tps, tile)] - first;
      }
      carry_t += tt;
      carry_g += tg;
    }
  }
  __syncthreads();
  // ---- stable rank inside each 64-entry round -> the entry's slot in the sorted tile
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll   // (key[] is a register array: a rolled loop would index it dynamically, i.e. through scratch)
  for (int r = 0; r < RS_ROUNDS; ++r) {
    const bool act = wl + (unsigned)r * 64 + lane < cnt;
    const unsigned d = (key[r] >> a.shift) & mask;
    unsigned long long peers = __ballot(act);
#pragma unroll
    for (int b = 0; b < RS_MAX_DIGIT_BITS; ++b) {
      const unsigned long long m = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? m : ~m;
    }
    if (act) {
      const unsigned base = offs[wave][d];
      const unsigned slot = base + (unsigned)__popcll(peers & lt);
      sk[slot] = key[r];
      sv[slot] = val[r];
      if ((peers >> lane) >> 1 == 0ull) offs[wave][d] = base + (unsigned)__popcll(peers);   // highest peer: next round's base
    }
  }
  __syncthreads();
  // ---- slot i -> global: a digit's run of slots goes to consecutive addresses
  for (unsigned i = threadIdx.x; i < cnt; i += RS_THREADS) {
    const unsigned k = sk[i];
    const unsigned o = gd[(k >> a.shift) & mask] + i;
    if (o - sbase >= len) continue;   // (cannot happen with tables built from these keys; a store never leaves the segment)
    a.keys_out[o] = k;
    if (a.vals_out) a.vals_out[o] = sv[i];
  }
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// the temporary storage of a sort over (nseg, seg_len): two key-sized arrays, then the tables
void rs_carve(int nseg, unsigned seg_len, void* temp, size_t temp_bytes, unsigned*& tk, unsigned*& tv, RsTables& t, size_t* used) {
  WsCarver c(temp, temp_bytes);
  const size_t n = (size_t)nseg * seg_len;
  t.tps = rs_tiles(seg_len) ? rs_tiles(seg_len) : 1u;
  tk = c.take<unsigned>(n);
  tv = c.take<unsigned>(n);
  t.hist = c.take<unsigned>((size_t)nseg * RS_BINS * t.tps);
  t.totals = c.take<unsigned>((size_t)nseg * RS_BINS);
  t.drops = c.take<unsigned>((size_t)nseg * t.tps);
  *used = c.off;
}
}  // namespace

size_t rdrf_sort_seg_temp_bytes(int nseg, unsigned seg_len, int bits) {
  (void)bits;   // the tables are sized for the widest digit
  if (nseg < 1) nseg = 1;
  const size_t tps = rs_tiles(seg_len) ? rs_tiles(seg_len) : 1u;
  return 2 * al256((size_t)nseg * seg_len * 4) + al256((size_t)nseg * RS_BINS * tps * 4) + al256((size_t)nseg * RS_BINS * 4) +
         al256((size_t)nseg * tps * 4) + 1024;
}

size_t rdrf_sort_temp_bytes(unsigned n, int bits) { return rdrf_sort_seg_temp_bytes(1, n, bits); }

size_t rdrf_sort_carved_bytes(int nseg, unsigned seg_len) {
  unsigned *tk, *tv;
  RsTables t;
  size_t used;
  rs_carve(nseg < 1 ? 1 : nseg, seg_len, nullptr, 0, tk, tv, t, &used);
  return used;
}

void rdrf_sort_plan(int bits, int* passes, int* digit_bits) { radix_plan(bits, *passes, *digit_bits); }

static int seg_args_ok(int nseg, unsigned seg_len, int bits, void* temp, size_t temp_bytes) {
  RDRF_CHECK(nseg >= 1 && (unsigned long long)nseg * seg_len <= 0xffffffffull, -1, "sort: %d segments of %u entries do not fit 32-bit positions",
             nseg, seg_len);
  RDRF_CHECK(temp != nullptr && temp_bytes >= rdrf_sort_seg_temp_bytes(nseg, seg_len, bits), -3,
             "sort: temporary storage too small (%zu < %zu)", temp_bytes, rdrf_sort_seg_temp_bytes(nseg, seg_len, bits));
  return 0;
}

// where a key kernel writes the first pass's tile histograms and drop counts, and that pass's bin count
int rdrf_sort_tables(int nseg, unsigned seg_len, int bits, void* temp, size_t temp_bytes, RsTables* t, int* nbins) {
  int rc = seg_args_ok(nseg, seg_len, bits, temp, temp_bytes);
  if (rc) return rc;
  unsigned *tk, *tv;
  size_t used;
  rs_carve(nseg, seg_len, temp, temp_bytes, tk, tv, *t, &used);
  RDRF_CHECK(used <= temp_bytes, -3, "sort: temporary storage too small");
  int passes, db;
  radix_plan(bits, passes, db);
  *nbins = 1 << db;
  return 0;
}

// counts != nullptr: the caller's key kernel has written the first pass's hist / drops (rdrf_sort_tables)
static int radix_sort(const unsigned* keys_in, unsigned* keys_out, unsigned* vals_out, int nseg, unsigned seg_len, int bits, void* temp,
                      size_t temp_bytes, hipStream_t stream, const int* len_dev, unsigned len_mul, int* counts) {
  if (seg_len == 0) return 0;
  int rc = seg_args_ok(nseg, seg_len, bits, temp, temp_bytes);
  if (rc) return rc;
  int passes, db;
  if (bits < 1) bits = 1;
  radix_plan(bits, passes, db);
  unsigned *tk, *tv;
  RsTables t;
  size_t used;
  rs_carve(nseg, seg_len, temp, temp_bytes, tk, tv, t, &used);
  RDRF_CHECK(used <= temp_bytes, -3, "sort: temporary storage too small");
  const unsigned* kin = keys_in;
  const unsigned* vin = nullptr;
  for (int p = 0; p < passes; ++p) {
    const bool to_out = ((passes - 1 - p) & 1) == 0;   // the last pass lands in the caller's arrays
    const bool prebuilt = p == 0 && counts != nullptr;
    RadixArgs a;
    a.keys_in = kin; a.vals_in = vin;
    a.keys_out = to_out ? keys_out : tk;
    a.vals_out = vals_out ? (to_out ? vals_out : tv) : nullptr;
    a.hist = t.hist; a.totals = t.totals; a.drops = t.drops; a.counts = prebuilt ? counts : nullptr;
    a.seg_len = seg_len; a.tps = t.tps; a.nseg = nseg; a.len_dev = len_dev; a.len_mul = len_mul;
    a.shift = p * db;
    a.nbins = 1 << (bits - p * db < db ? bits - p * db : db);   // the last digit may be short: bits above `bits` are never sorted on
    const dim3 tiles(t.tps, (unsigned)nseg);
    rdrf_prof_begin("sort", stream);
    if (!prebuilt) hipLaunchKernelGGL(k_radix_hist, tiles, dim3(RS_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_radix_scan, dim3((unsigned)a.nbins + (prebuilt ? 1u : 0u), (unsigned)nseg), dim3(RS_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_radix_scatter, tiles, dim3(RS_THREADS), 0, stream, a);
    rdrf_prof_end("sort", stream);
    RDRF_HIP(hipGetLastError());
    kin = a.keys_out;
    vin = a.vals_out;
  }
  return 0;
}

// keys_in [n] -> keys_out [n] ascending (stable), vals_out[i] = original position of keys_out[i]
// n_dev (optional): the first n_mul * *n_dev entries only (a count that lives on the device)
int rdrf_sort_positions(const unsigned* keys_in, unsigned* keys_out, unsigned* vals_out, unsigned n, int bits, void* temp,
                        size_t temp_bytes, hipStream_t stream, const int* n_dev, unsigned n_mul) {
  RDRF_CHECK(keys_in && keys_out && vals_out, -1, "sort: null argument");
  return radix_sort(keys_in, keys_out, vals_out, 1, n, bits, temp, temp_bytes, stream, n_dev, n_mul, nullptr);
}

// nseg independent stable sorts over the low `bits` bits (the bits above ride along): segment s is entries
// [s * L, (s + 1) * L) of keys_in and of the outputs, L = seg_len, or min(seg_len, *seg_len_dev) with a device-side count
// (the compacted appearance list); vals_out = GLOBAL positions s * L + index.  counts (optional): see rdrf_sort_tables
int rdrf_sort_positions_seg(const unsigned* keys_in, unsigned* keys_out, unsigned* vals_out, int nseg, unsigned seg_len, int bits,
                            void* temp, size_t temp_bytes, hipStream_t stream, const int* seg_len_dev, int* counts) {
  RDRF_CHECK(keys_in && keys_out && vals_out, -1, "sort: null argument");
  return radix_sort(keys_in, keys_out, vals_out, nseg, seg_len, bits, temp, temp_bytes, stream, seg_len_dev, 1u, counts);
}

// deterministic build: ascending in-place sort of an int list (the app-mask compaction lists, whose append order depends on
// wave timing).  Scratch is a lazily grown device allocation owned by this debugging build.
int rdrf_sort_ints_inplace(int* data, unsigned n, hipStream_t stream) {
  static void* scratch = nullptr;
  static size_t scratch_bytes = 0;
  if (n == 0) return 0;
  const size_t need = rdrf_sort_temp_bytes(n, 32);
  const size_t total = need + (((size_t)n * 4 + 255) & ~(size_t)255) + 512;
  if (total > scratch_bytes) {
    if (scratch) RDRF_HIP(hipFree(scratch));
    RDRF_HIP(hipMalloc(&scratch, total));
    scratch_bytes = total;
  }
  unsigned* out = (unsigned*)scratch;
  void* tmp = (char*)scratch + (((size_t)n * 4 + 255) & ~(size_t)255);
  int rc = radix_sort((const unsigned*)data, out, nullptr, 1, n, 32, tmp, need, stream, nullptr, 0u, nullptr);
  if (rc) return rc;
  RDRF_HIP(hipMemcpyAsync(data, out, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
  return 0;
}
