// rdrf_simplify.hip -- mesh simplification by vertex clustering (Rossignac-Borrel) of an indexed triangle mesh that lives on the
// device: a sort, a segmented reduction and two stream compactions, in fixed orders, without atomics on global memory.
//
// Conventions ("Mesh simplification"; tests/_simplify_prim.py restates them):
//   cell of a vertex   per axis c = clamp(floor((v - origin) / cell), 0, n - 1) in fp32 without contraction; a coordinate for
//                      which (v - origin) / cell >= 0 is false (NaN among them) goes to 0.  key = (c0 n1 + c1) n2 + c2
//   cluster            the vertices of one key.  Clusters ascend by key, their members by original index (the stable sort)
//   representative     fp64 sums over the members in that order, divided by the count in fp64, rounded once to fp32
//   face               mapped through the cluster ids; kept iff the three differ; kept faces keep their order and their winding
//
//   k_simp_keys     a lane per vertex: its key
//   (rdrf_sort_positions: keys -> sorted keys + the original index of every sorted position)
//   k_simp_heads    a lane per sorted position: head flag (the key differs from its predecessor's), scanned over the workgroup
//   k_simp_scan     exclusive scan of 256-entry chunks of a sum table, chunk totals to the next table (three levels reach 2^32;
//                   no pass adds the levels back: prefix(i) = local[i] + s0[i >> 8] + s1[i >> 16] + s2[i >> 24])
//   k_simp_assign   a lane per sorted position: cluster id = inclusive head count - 1 -> cluster[original index]; a head
//                   stores the cluster's first sorted position; the referenced marks are initialised
//   k_simp_fcount   a lane per face: kept flag, scanned; a kept face marks its three clusters (plain stores of the value 1)
//   k_simp_used     a lane per cluster: its mark, scanned -> the cluster's output index
//   k_simp_remap    a lane per vertex: the output index of its cluster, -1 where the cluster was dropped
//   k_simp_verts    a lane per cluster: walks its members in order (one lane whatever the cluster's size: the order of the
//                   additions is the member order) and writes position, normal, colour at the cluster's output index
//   k_simp_faces    a lane per face: a kept face at its prefix, its indices the output indices of its clusters
#include "rdrf_host.hpp"

#include <cmath>
#include <stdint.h>

constexpr int SIMP_BLOCK = 256;
// V and F below 2^31: a vertex index is an int of `faces` and `remap` (-1 marks a dropped vertex), and both counts go through
// the unsigned lane index blockIdx.x * 256 + threadIdx.x, which must not wrap in the last workgroup (n <= 2^32 - 256)
constexpr int64_t SIMP_MAX_COUNT = 2147483647ll;

struct SimpScan {
  uint8_t* local;   // [n]  exclusive prefix of the 0 / 1 flags inside the entry's 256-entry block
  unsigned* s[3];   // [ceil(n / 256^(l + 1))]  exclusive prefix of the level's chunks inside the next level's chunk
};

struct SimpWs {
  unsigned* keys;      // [V]      key of vertex v
  unsigned* skeys;     // [V]      keys ascending
  unsigned* order;     // [V]      original index of sorted position i
  int* cluster;        // [V]      cluster of vertex v (before any cluster is dropped)
  unsigned* start;     // [V + 1]  first sorted position of cluster c; start[clusters] = V
  uint8_t* used;       // [V]      cluster c is emitted
  long long* nc;       // [1]      clusters
  SimpScan H, U, K;    // heads over sorted positions, emitted clusters over clusters, kept faces over faces
  void* sort_temp;
  size_t sort_bytes;
};

__device__ __forceinline__ unsigned simp_prefix(const SimpScan& t, unsigned i) {
  return (unsigned)t.local[i] + t.s[0][i >> 8] + t.s[1][i >> 16] + t.s[2][i >> 24];
}

// exclusive scan of one count per thread over the workgroup; total = the workgroup's sum
__device__ __forceinline__ unsigned simp_block_exscan(unsigned x, unsigned* s_wave, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned y = __shfl_up(inc, off, 64);
    if (lane >= off) inc += y;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  unsigned base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < SIMP_BLOCK / 64; ++w) {
    const unsigned t = s_wave[w];
    if (w < wave) base += t;
    total += t;
  }
  return base + inc - x;
}

// the flag of entry i of a level-0 scan: local prefix + the block's total
__device__ __forceinline__ void simp_scan_flag(const SimpScan& t, unsigned i, bool act, unsigned flag, unsigned* s_wave) {
  unsigned total;
  const unsigned ex = simp_block_exscan(flag, s_wave, total);
  if (act) t.local[i] = (uint8_t)ex;
  if (threadIdx.x == 0) t.s[0][blockIdx.x] = total;
}

struct SimpLattice {
  float origin[3], cell[3];
  int n[3];
};

__device__ __forceinline__ unsigned simp_cell(float v, float origin, float cell, int n) {
#pragma clang fp contract(off)
  const float t = (v - origin) / cell;
  if (!(t >= 0.0f)) return 0u;
  const float f = floorf(t);
  if (f >= (float)n) return (unsigned)(n - 1);   // (float)n <= 2^31, so below it the conversion cannot overflow
  const int c = (int)f;
  return (unsigned)(c < n - 1 ? c : n - 1);
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_keys(const float* __restrict__ verts, unsigned V, SimpLattice g,
                                                          unsigned* __restrict__ keys) {
  const unsigned v = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (v >= V) return;
  const float* p = verts + (size_t)v * 3;
  const unsigned c0 = simp_cell(p[0], g.origin[0], g.cell[0], g.n[0]);
  const unsigned c1 = simp_cell(p[1], g.origin[1], g.cell[1], g.n[1]);
  const unsigned c2 = simp_cell(p[2], g.origin[2], g.cell[2], g.n[2]);
  keys[v] = (c0 * (unsigned)g.n[1] + c1) * (unsigned)g.n[2] + c2;
}

__device__ __forceinline__ bool simp_head(const unsigned* __restrict__ skeys, unsigned i) {
  return i == 0u || skeys[i] != skeys[i - 1u];
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_heads(SimpWs ws, unsigned V) {
  __shared__ unsigned s_wave[SIMP_BLOCK / 64];
  const unsigned i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const bool act = i < V;
  simp_scan_flag(ws.H, i, act, act && simp_head(ws.skeys, i) ? 1u : 0u, s_wave);
}

// in place: a[i] becomes the exclusive prefix inside its 256-entry chunk; chunk totals go to `next`; total_out (top level, one
// chunk): the sum of everything
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_scan(unsigned* __restrict__ a, unsigned n, unsigned* __restrict__ next,
                                                          long long* __restrict__ total_out) {
  __shared__ unsigned s_wave[SIMP_BLOCK / 64];
  const unsigned i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const unsigned x = i < n ? a[i] : 0u;
  unsigned total;
  const unsigned ex = simp_block_exscan(x, s_wave, total);
  if (i < n) a[i] = ex;
  if (threadIdx.x == 0) {
    if (next != nullptr) next[blockIdx.x] = total;
    if (total_out != nullptr) *total_out = (long long)total;
  }
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_assign(SimpWs ws, unsigned V, int drop) {
  const unsigned i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (i >= V) return;
  const bool head = simp_head(ws.skeys, i);
  const unsigned c = simp_prefix(ws.H, i) + (head ? 1u : 0u) - 1u;
  const unsigned v = ws.order[i];
  if (v < V) ws.cluster[v] = (int)c;   // (the sort's values are the positions 0 .. V - 1)
  if (head) ws.start[c] = i;
  if (i == V - 1u) ws.start[c + 1u] = V;
  ws.used[i] = drop ? (uint8_t)0 : (uint8_t)1;   // entry i of the marks, not this position's cluster
}

// the clusters of face f; false where an index lies outside [0, V) or two of the three agree
__device__ __forceinline__ bool simp_face(const int* __restrict__ faces, const int* __restrict__ cluster, unsigned f, unsigned V,
                                          int idx[3], int c[3]) {
  const int* p = faces + (size_t)f * 3;
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    idx[d] = p[d];
    ok = ok && idx[d] >= 0 && (unsigned)idx[d] < V;
  }
  if (!ok) return false;
#pragma unroll
  for (int d = 0; d < 3; ++d) c[d] = cluster[idx[d]];
  return c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_fcount(const int* __restrict__ faces, unsigned F, unsigned V, SimpWs ws, int drop) {
  __shared__ unsigned s_wave[SIMP_BLOCK / 64];
  const unsigned f = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const bool act = f < F;
  int idx[3], c[3];
  const bool keep = act && simp_face(faces, ws.cluster, f, V, idx, c);
  if (keep && drop) {
    // several lanes may store the same value to the same byte: the only race of the unit
#pragma unroll
    for (int d = 0; d < 3; ++d) ws.used[c[d]] = (uint8_t)1;
  }
  simp_scan_flag(ws.K, f, act, keep ? 1u : 0u, s_wave);
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_used(SimpWs ws, unsigned V) {
  __shared__ unsigned s_wave[SIMP_BLOCK / 64];
  const unsigned c = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  const bool act = c < V;
  const bool cl = act && (long long)c < *ws.nc;
  simp_scan_flag(ws.U, c, act, cl && ws.used[c] != 0 ? 1u : 0u, s_wave);
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_remap(SimpWs ws, unsigned V, int* __restrict__ remap) {
  const unsigned v = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (v >= V) return;
  const unsigned c = (unsigned)ws.cluster[v];
  remap[v] = ws.used[c] != 0 ? (int)simp_prefix(ws.U, c) : -1;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_verts(const float* __restrict__ verts, const float* __restrict__ normals,
                                                           const unsigned char* __restrict__ colors, unsigned V, SimpWs ws,
                                                           float* __restrict__ verts_out, float* __restrict__ normals_out,
                                                           unsigned char* __restrict__ colors_out, long long nv) {
  const unsigned c = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (c >= V || (long long)c >= *ws.nc || ws.used[c] == 0) return;
  const long long o = (long long)simp_prefix(ws.U, c);
  if (o >= nv) return;
  const unsigned b = ws.start[c], e = ws.start[c + 1u];
  const bool has_n = normals != nullptr && normals_out != nullptr, has_c = colors != nullptr && colors_out != nullptr;
  double sp[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0};
  unsigned long long sc[3] = {0ull, 0ull, 0ull};
  for (unsigned i = b; i < e && i < V; ++i) {
    const size_t v = (size_t)ws.order[i] * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) sp[d] += (double)verts[v + d];
    if (has_n) {
#pragma unroll
      for (int d = 0; d < 3; ++d) sn[d] += (double)normals[v + d];
    }
    if (has_c) {
#pragma unroll
      for (int d = 0; d < 3; ++d) sc[d] += (unsigned long long)colors[v + d];
    }
  }
  const unsigned long long k = (unsigned long long)(e - b);
  const double kd = (double)k;
#pragma unroll
  for (int d = 0; d < 3; ++d) verts_out[(size_t)o * 3 + d] = (float)(sp[d] / kd);
  if (has_n) {
    // scaled by the largest component first, so that the squares neither overflow nor vanish; a zero vector stays zero
    const double big = fmax(fabs(sn[0]), fmax(fabs(sn[1]), fabs(sn[2])));
    if (big > 0.0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) sn[d] /= big;
      const double len = sqrt(sn[0] * sn[0] + sn[1] * sn[1] + sn[2] * sn[2]);
#pragma unroll
      for (int d = 0; d < 3; ++d) sn[d] /= len;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) normals_out[(size_t)o * 3 + d] = (float)sn[d];
  }
  if (has_c) {
#pragma unroll
    for (int d = 0; d < 3; ++d) colors_out[(size_t)o * 3 + d] = (unsigned char)((2ull * sc[d] + k) / (2ull * k));   // the mean, half up
  }
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_faces(const int* __restrict__ faces, unsigned F, unsigned V, SimpWs ws,
                                                           int* __restrict__ faces_out, long long nf) {
  const unsigned f = blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (f >= F) return;
  int idx[3], c[3];
  if (!simp_face(faces, ws.cluster, f, V, idx, c)) return;
  const long long o = (long long)simp_prefix(ws.K, f);
  if (o >= nf) return;
#pragma unroll
  for (int d = 0; d < 3; ++d) faces_out[(size_t)o * 3 + d] = (int)simp_prefix(ws.U, (unsigned)c[d]);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static inline unsigned simp_chunks(unsigned n) { return (n + SIMP_BLOCK - 1) / SIMP_BLOCK; }

static void carve_scan(SimpScan& t, WsCarver& c, size_t n) {
  t.local = c.take<uint8_t>(n);
  size_t m = n;
  for (int l = 0; l < 3; ++l) {
    m = (m + SIMP_BLOCK - 1) / SIMP_BLOCK;
    t.s[l] = c.take<unsigned>(m ? m : 1);
  }
}

// (the layout depends on V and F only: the sort's temporary storage is sized for the widest key)
static void carve_simp(SimpWs& w, WsCarver& c, size_t V, size_t F) {
  w.keys = c.take<unsigned>(V);
  w.skeys = c.take<unsigned>(V);
  w.order = c.take<unsigned>(V);
  w.cluster = c.take<int>(V);
  w.start = c.take<unsigned>(V + 1);
  w.used = c.take<uint8_t>(V);
  w.nc = c.take<long long>(1);
  carve_scan(w.H, c, V);
  carve_scan(w.U, c, V);
  carve_scan(w.K, c, F);
  w.sort_bytes = (rdrf_sort_temp_bytes((unsigned)V, 32) + 255) & ~(size_t)255;
  w.sort_temp = c.take<char>(w.sort_bytes);
}

static int simp_counts_refused(const char* what, int64_t V, int64_t F) {
  RDRF_CHECK(V >= 0 && F >= 0, -1, "%s: negative counts (%lld vertices, %lld faces)", what, (long long)V, (long long)F);
  RDRF_CHECK(V <= SIMP_MAX_COUNT, -1, "%s: %lld vertices, the vertex indices are 32-bit ints (at most %lld)", what, (long long)V,
             (long long)SIMP_MAX_COUNT);
  RDRF_CHECK(F <= SIMP_MAX_COUNT, -1, "%s: %lld faces, the face prefixes are 32-bit (at most %lld)", what, (long long)F,
             (long long)SIMP_MAX_COUNT);
  return 0;
}

// the lattice's limits; bits = ceil(log2(cells))
static int simp_lattice_refused(const char* what, const int n[3], int* bits) {
  RDRF_CHECK(n != nullptr, -1, "%s: no lattice", what);
  RDRF_CHECK(n[0] >= 1 && n[1] >= 1 && n[2] >= 1, -1, "%s: every side of the lattice must have at least 1 cell, not %d x %d x %d", what,
             n[0], n[1], n[2]);
  const double cells = (double)n[0] * n[1] * n[2];
  RDRF_CHECK(cells < 2147483648.0, -1, "%s: %d x %d x %d has %.0f cells, the keys are below 2^31", what, n[0], n[1], n[2], cells);
  int b = 0;
  while (((uint64_t)1 << b) < (uint64_t)cells) ++b;
  if (bits) *bits = b;
  return 0;
}

extern "C" size_t rdrf_simplify_ws_bytes(int64_t V, int64_t F, const int n[3]) {
  if (simp_counts_refused("simplify_ws_bytes", V, F) || simp_lattice_refused("simplify_ws_bytes", n, nullptr)) return 0;
  SimpWs w;
  WsCarver c;
  carve_simp(w, c, (size_t)V, (size_t)F);
  return c.off;
}

// top of a three-level scan over n entries whose level-0 kernel has written t.local and t.s[0]
static int simp_scan_levels(const SimpScan& t, unsigned n, long long* total_out, hipStream_t stream) {
  const unsigned n0 = simp_chunks(n), n1 = simp_chunks(n0), n2 = simp_chunks(n1);   // n2 <= 256: one chunk at the top
  RDRF_LAUNCH("simplify_scan", k_simp_scan, dim3(n1), dim3(SIMP_BLOCK), stream, t.s[0], n0, t.s[1], (long long*)nullptr);
  RDRF_LAUNCH("simplify_scan", k_simp_scan, dim3(n2), dim3(SIMP_BLOCK), stream, t.s[1], n1, t.s[2], (long long*)nullptr);
  RDRF_LAUNCH("simplify_scan", k_simp_scan, dim3(1), dim3(SIMP_BLOCK), stream, t.s[2], n2, (unsigned*)nullptr, total_out);
  return 0;
}

extern "C" int rdrf_simplify_count(const float* verts, int64_t V, const int* faces, int64_t F, const float origin[3], const float cell[3],
                                   const int n[3], int drop_unreferenced, void* ws, size_t ws_bytes, int64_t* counts, int* remap,
                                   rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int bits = 0;
  RDRF_TRY(simp_counts_refused("simplify_count", V, F));
  RDRF_TRY(simp_lattice_refused("simplify_count", n, &bits));
  RDRF_CHECK(origin != nullptr && cell != nullptr, -1, "simplify_count: no lattice origin or cell size");
  SimpLattice g;
  for (int d = 0; d < 3; ++d) {
    RDRF_CHECK(cell[d] > 0.0f && std::isfinite(cell[d]), -1, "simplify_count: cell sizes must be positive and finite, not %g %g %g",
               (double)cell[0], (double)cell[1], (double)cell[2]);
    RDRF_CHECK(std::isfinite(origin[d]), -1, "simplify_count: the origin must be finite, not %g %g %g", (double)origin[0], (double)origin[1],
               (double)origin[2]);
    g.origin[d] = origin[d];
    g.cell[d] = cell[d];
    g.n[d] = n[d];
  }
  RDRF_CHECK(counts != nullptr, -1, "simplify_count: bad arguments");
  if (V == 0 || F == 0) {   // nothing is kept: the counts only
    RDRF_FILL(counts, 0, 2 * sizeof(int64_t), stream);
    return 0;
  }
  RDRF_CHECK(verts != nullptr && faces != nullptr, -1, "simplify_count: bad arguments");
  RDRF_CHECK(ws != nullptr, -3, "simplify_count: no workspace");
  SimpWs w;
  WsCarver c(ws, ws_bytes);
  carve_simp(w, c, (size_t)V, (size_t)F);
  RDRF_CHECK(c.ok(), -3, "simplify_count: workspace too small: need %zu have %zu", c.off, ws_bytes);
  const unsigned v = (unsigned)V, f = (unsigned)F;
  const int drop = drop_unreferenced ? 1 : 0;
  const dim3 block(SIMP_BLOCK), gv(simp_chunks(v)), gf(simp_chunks(f));
  RDRF_LAUNCH("simplify_keys", k_simp_keys, gv, block, stream, verts, v, g, w.keys);
  RDRF_TRY(rdrf_sort_positions(w.keys, w.skeys, w.order, v, bits, w.sort_temp, w.sort_bytes, stream));
  RDRF_LAUNCH("simplify_heads", k_simp_heads, gv, block, stream, w, v);
  RDRF_TRY(simp_scan_levels(w.H, v, w.nc, stream));
  RDRF_LAUNCH("simplify_assign", k_simp_assign, gv, block, stream, w, v, drop);
  RDRF_LAUNCH("simplify_fcount", k_simp_fcount, gf, block, stream, faces, f, v, w, drop);
  RDRF_TRY(simp_scan_levels(w.K, f, (long long*)(counts + 1), stream));
  RDRF_LAUNCH("simplify_used", k_simp_used, gv, block, stream, w, v);
  RDRF_TRY(simp_scan_levels(w.U, v, (long long*)counts, stream));
  if (remap != nullptr) RDRF_LAUNCH("simplify_remap", k_simp_remap, gv, block, stream, w, v, remap);
  return 0;
}

extern "C" int rdrf_simplify_emit(const float* verts, const float* normals, const unsigned char* colors, int64_t V, const int* faces,
                                  int64_t F, const void* ws, float* verts_out, float* normals_out, unsigned char* colors_out,
                                  int* faces_out, int64_t nv, int64_t nf, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_TRY(simp_counts_refused("simplify_emit", V, F));
  RDRF_CHECK(nv >= 0 && nf >= 0 && nv <= V && nf <= F, -1, "simplify_emit: %lld vertices and %lld faces out of %lld and %lld",
             (long long)nv, (long long)nf, (long long)V, (long long)F);
  if (nv == 0 && nf == 0) return 0;
  RDRF_CHECK(verts != nullptr && faces != nullptr && (verts_out != nullptr || nv == 0) && (faces_out != nullptr || nf == 0), -1,
             "simplify_emit: bad arguments");
  RDRF_CHECK((normals != nullptr) == (normals_out != nullptr) && (colors != nullptr) == (colors_out != nullptr), -1,
             "simplify_emit: normals and colours need both their input and their output");
  RDRF_CHECK(ws != nullptr, -3, "simplify_emit: no workspace");
  SimpWs w;
  WsCarver c((void*)ws, ~(size_t)0);   // (the workspace is the one rdrf_simplify_count carved and checked)
  carve_simp(w, c, (size_t)V, (size_t)F);
  const unsigned v = (unsigned)V, f = (unsigned)F;
  const dim3 block(SIMP_BLOCK);
  if (nv > 0)
    RDRF_LAUNCH("simplify_verts", k_simp_verts, dim3(simp_chunks(v)), block, stream, verts, normals, colors, v, w, verts_out, normals_out,
                colors_out, (long long)nv);
  if (nf > 0) RDRF_LAUNCH("simplify_faces", k_simp_faces, dim3(simp_chunks(f)), block, stream, faces, f, v, w, faces_out, (long long)nf);
  return 0;
}
