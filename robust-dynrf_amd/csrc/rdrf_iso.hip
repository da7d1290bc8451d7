// rdrf_iso.hip -- isosurface meshes of a dense volume [G0][G1][G2][T] (the alpha volume of getDenseAlpha, one time slice):
// marching tetrahedra on the Kuhn split of the lattice cubes, as an indexed mesh in a fixed order, without atomics.
//
// Conventions ("Isosurface meshes"; tests/_iso_prim.py restates them):
//   point p = (i G1 + j) G2 + k; corner code c = 4 dx + 2 dy + dz of a cube corner; a lattice edge belongs to its lower end
//   and has kind c(upper - lower) - 1 (0 z, 1 y, 2 yz, 3 x, 4 xz, 5 xy, 6 xyz); a sample is inside iff v >= level.
//   tetrahedron q of a cube: corners 0, bit(a), bit(a) | bit(b), 7 with (a, b, c) the q-th permutation of the axes in
//   lexicographic order and bit(axis) = 4 >> axis.
//
//   k_iso_count  a lane per point (k fastest, so the eight corner reads of a wave are eight coalesced rows): the crossed flags
//                of the point's seven edges + its inside bit, the triangle count of the cube it is the lower corner of, and
//                the exclusive scan of both counts over the workgroup's 256 points (packed: vertices low, triangles high)
//   k_iso_scan   exclusive scan of 256-entry chunks of a sum table, chunk totals to the next table; three levels reach
//                2^32 points.  No pass adds the levels back: a point's prefix is local + s0[p >> 8] + s1[p >> 16] + s2[p >> 24]
//   k_iso_verts  a lane per point: the vertices of its crossed edges at prefix + rank; positions, optional normals
//   k_iso_faces  a lane per cube: its triangles at the cube's triangle prefix, tetrahedron by tetrahedron; a vertex index is
//                prefix[owner] + popcount(flags[owner] & lower kinds), looked up for the cubes the surface passes through only
#include "rdrf_host.hpp"

#include <stdint.h>

constexpr int ISO_BLOCK = 256;
typedef unsigned long long iso_u64;

struct IsoGrid {
  int G0, G1, G2, T, t_index;
  unsigned n;   // lattice points
};

struct IsoWs {
  uint8_t* flags;     // [n]   bits 0..6 crossed edge kinds, bit 7 the point is inside
  ushort2* local;     // [n]   exclusive (vertex, triangle) prefix inside the point's 256-point block
  iso_u64* s[3];      // [ceil(n / 256^(l + 1))]  exclusive packed prefix of the level's chunks inside the next level's chunk
};

__device__ __forceinline__ float iso_sample(const float* __restrict__ vol, const IsoGrid& g, unsigned p) {
  return vol[(size_t)p * (size_t)g.T + (size_t)g.t_index];
}

__device__ __forceinline__ unsigned iso_corner(const IsoGrid& g, unsigned p, unsigned code) {
  return p + ((code >> 2) & 1u) * (unsigned)(g.G1 * g.G2) + ((code >> 1) & 1u) * (unsigned)g.G2 + (code & 1u);
}

// corner codes of tetrahedron q, three bits each, corner 0 lowest
__device__ __forceinline__ unsigned iso_tet_codes(int q) {
  const int a = q >> 1;
  const int b = (q & 1) ? (a == 2 ? 1 : 2) : (a == 0 ? 1 : 0);
  const unsigned c1 = 4u >> a, c2 = c1 | (4u >> b);
  return (c1 << 3) | (c2 << 6) | (7u << 9);
}
// the inside bits of the tetrahedron's corners 0..3 from the cube's eight
__device__ __forceinline__ unsigned iso_tet_mask(unsigned m, unsigned codes) {
  return (m & 1u) | (((m >> ((codes >> 3) & 7u)) & 1u) << 1) | (((m >> ((codes >> 6) & 7u)) & 1u) << 2) | (((m >> 7) & 1u) << 3);
}

// exclusive scan of a packed pair of counts over the workgroup; total = the workgroup's sum
__device__ __forceinline__ iso_u64 iso_block_exscan(iso_u64 x, iso_u64* s_wave, iso_u64& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  iso_u64 inc = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const iso_u64 y = __shfl_up(inc, off, 64);
    if (lane >= off) inc += y;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  iso_u64 base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < ISO_BLOCK / 64; ++w) {
    const iso_u64 t = s_wave[w];
    if (w < wave) base += t;
    total += t;
  }
  return base + inc - x;
}

__global__ __launch_bounds__(ISO_BLOCK) void k_iso_count(const float* __restrict__ vol, IsoGrid g, float level, IsoWs ws) {
  __shared__ iso_u64 s_wave[ISO_BLOCK / 64];
  const unsigned p = blockIdx.x * ISO_BLOCK + threadIdx.x;
  const bool act = p < g.n;
  unsigned vc = 0, tc = 0, flags = 0;
  if (act) {
    const unsigned k = p % (unsigned)g.G2, r = p / (unsigned)g.G2;
    const unsigned j = r % (unsigned)g.G1, i = r / (unsigned)g.G1;
    const bool e[3] = {i + 1 < (unsigned)g.G0, j + 1 < (unsigned)g.G1, k + 1 < (unsigned)g.G2};
    const bool in0 = iso_sample(vol, g, p) >= level;
    unsigned m = in0 ? 1u : 0u;
#pragma unroll
    for (unsigned c = 1; c < 8; ++c) {
      const bool exists = (!(c & 4) || e[0]) && (!(c & 2) || e[1]) && (!(c & 1) || e[2]);
      // an edge whose upper end lies outside the volume does not exist: its end counts as the point itself
      const bool in = exists ? iso_sample(vol, g, iso_corner(g, p, c)) >= level : in0;
      m |= (in ? 1u : 0u) << c;
    }
    const unsigned crossed = ((m >> 1) ^ (in0 ? 0x7fu : 0u)) & 0x7fu;
    flags = crossed | (in0 ? 0x80u : 0u);
    vc = __popc(crossed);
    if (e[0] && e[1] && e[2]) {
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int ni = __popc(iso_tet_mask(m, iso_tet_codes(q)));
        tc += (ni == 0 || ni == 4) ? 0u : (ni == 2 ? 2u : 1u);
      }
    }
  }
  iso_u64 total;
  const iso_u64 ex = iso_block_exscan((iso_u64)vc | ((iso_u64)tc << 32), s_wave, total);
  if (act) {
    ws.flags[p] = (uint8_t)flags;
    ws.local[p] = make_ushort2((unsigned short)(ex & 0xffffu), (unsigned short)((ex >> 32) & 0xffffu));
  }
  if (threadIdx.x == 0) ws.s[0][blockIdx.x] = total;
}

// in place: a[i] becomes the exclusive prefix inside its 256-entry chunk; chunk totals go to `next`; counts (top level, one
// chunk): {vertices, triangles}
__global__ __launch_bounds__(ISO_BLOCK) void k_iso_scan(iso_u64* __restrict__ a, unsigned n, iso_u64* __restrict__ next,
                                                        int64_t* __restrict__ counts) {
  __shared__ iso_u64 s_wave[ISO_BLOCK / 64];
  const unsigned i = blockIdx.x * ISO_BLOCK + threadIdx.x;
  const iso_u64 x = i < n ? a[i] : 0ull;
  iso_u64 total;
  const iso_u64 ex = iso_block_exscan(x, s_wave, total);
  if (i < n) a[i] = ex;
  if (threadIdx.x == 0) {
    if (next != nullptr) next[blockIdx.x] = total;
    if (counts != nullptr) {
      counts[0] = (int64_t)(total & 0xffffffffull);
      counts[1] = (int64_t)(total >> 32);
    }
  }
}

// packed (vertex, triangle) prefix of point p
__device__ __forceinline__ iso_u64 iso_prefix(const IsoWs& ws, unsigned p) {
  const ushort2 l = ws.local[p];
  return ws.s[0][p >> 8] + ws.s[1][p >> 16] + ws.s[2][p >> 24] + ((iso_u64)l.x | ((iso_u64)l.y << 32));
}

// the index of the vertex on the edge of `kind` that point `owner` owns
__device__ __forceinline__ int iso_vertex_id(const IsoWs& ws, unsigned owner, unsigned kind) {
  return (int)(unsigned)(iso_prefix(ws, owner) & 0xffffffffull) + __popc((unsigned)ws.flags[owner] & ((1u << kind) - 1u));
}

struct IsoBox {
  float lo[3], ext[3], h[3];   // aabb min, aabb max - min, lattice spacing
  float den[3];                // G - 1
};

__device__ __forceinline__ float iso_pos(const IsoBox& b, int d, unsigned idx) {
  return b.lo[d] + ((float)idx / b.den[d]) * b.ext[d];
}

// -grad v at lattice point (i, j, k): central differences, one-sided at the volume boundary
__device__ __forceinline__ void iso_neg_gradient(const float* __restrict__ vol, const IsoGrid& g, const IsoBox& b, unsigned p,
                                                 const unsigned idx[3], float out[3]) {
  const unsigned stride[3] = {(unsigned)(g.G1 * g.G2), (unsigned)g.G2, 1u};
  const unsigned top[3] = {(unsigned)g.G0 - 1u, (unsigned)g.G1 - 1u, (unsigned)g.G2 - 1u};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const bool has_lo = idx[d] > 0, has_hi = idx[d] < top[d];
    const float v_lo = iso_sample(vol, g, has_lo ? p - stride[d] : p);
    const float v_hi = iso_sample(vol, g, has_hi ? p + stride[d] : p);
    const float span = (has_lo && has_hi) ? 2.0f * b.h[d] : b.h[d];
    out[d] = (v_lo - v_hi) / span;
  }
}

__global__ __launch_bounds__(ISO_BLOCK) void k_iso_verts(const float* __restrict__ vol, IsoGrid g, float level, IsoBox box, IsoWs ws,
                                                         float* __restrict__ verts, float* __restrict__ normals, long long nv) {
  const unsigned p = blockIdx.x * ISO_BLOCK + threadIdx.x;
  if (p >= g.n) return;
  const unsigned f = ws.flags[p];
  const unsigned crossed = f & 0x7fu;
  if (crossed == 0u) return;
  const bool in0 = (f & 0x80u) != 0u;
  const unsigned k = p % (unsigned)g.G2, r = p / (unsigned)g.G2;
  const unsigned i0[3] = {r / (unsigned)g.G1, r % (unsigned)g.G1, k};
  const float v0 = iso_sample(vol, g, p);
  long long vi = (long long)(unsigned)(iso_prefix(ws, p) & 0xffffffffull);
  float g0[3] = {0.f, 0.f, 0.f};
  if (normals != nullptr) iso_neg_gradient(vol, g, box, p, i0, g0);
  const float x0[3] = {iso_pos(box, 0, i0[0]), iso_pos(box, 1, i0[1]), iso_pos(box, 2, i0[2])};
  for (unsigned kind = 0; kind < 7; ++kind) {
    if (!((crossed >> kind) & 1u)) continue;
    const unsigned c = kind + 1;
    const unsigned q = iso_corner(g, p, c);
    const unsigned i1[3] = {i0[0] + ((c >> 2) & 1u), i0[1] + ((c >> 1) & 1u), i0[2] + (c & 1u)};
    const float v1 = iso_sample(vol, g, q);
    // lo = the outside end, hi = the inside end: v_lo < level <= v_hi
    const float v_lo = in0 ? v1 : v0, v_hi = in0 ? v0 : v1;
    const float t = (level - v_lo) / (v_hi - v_lo);
    if (vi < nv) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float x1 = i1[d] != i0[d] ? iso_pos(box, d, i1[d]) : x0[d];
        const float p_lo = in0 ? x1 : x0[d], p_hi = in0 ? x0[d] : x1;
        verts[(size_t)vi * 3 + d] = p_lo + t * (p_hi - p_lo);
      }
      if (normals != nullptr) {
        float g1[3];
        iso_neg_gradient(vol, g, box, q, i1, g1);
        float n[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float g_lo = in0 ? g1[d] : g0[d], g_hi = in0 ? g0[d] : g1[d];
          n[d] = (1.0f - t) * g_lo + t * g_hi;
        }
        // scaled by the largest component first, so that the squares neither overflow nor vanish; a zero vector stays zero
        const float big = fmaxf(fabsf(n[0]), fmaxf(fabsf(n[1]), fabsf(n[2])));
        if (big > 0.0f) {
#pragma unroll
          for (int d = 0; d < 3; ++d) n[d] /= big;
          const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
          for (int d = 0; d < 3; ++d) n[d] /= len;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) normals[(size_t)vi * 3 + d] = n[d];
      }
    }
    ++vi;
  }
}

// Triangles of a tetrahedron with local corners 0..3, e(p, q) the vertex on the edge between corners p and q:
//   one corner u apart from the others w1 < w2 < w3:      e(u,w1) e(u,w2) e(u,w3)
//   two inside p < q, two outside r < s:                  e(p,r) e(p,s) e(q,s)  and  e(p,r) e(q,s) e(q,r)
// Where (b - a) x (c - a) of that order would point at the inside corners the last two entries swap.  For a tetrahedron of an
// even axis permutation those are the inside masks of ISO_SWAP (u alone inside: odd u; u alone outside: even u; of the pairs
// {0,2}, {1,3}, {2,3}); a tetrahedron of an odd permutation is the mirror image, so there the bit is inverted.
// tests/_iso_prim.py decides every winding from the geometry instead, and the GPU tests compare the faces one by one.
constexpr unsigned ISO_SWAP = 0x4d24u;   // bit s: inside mask s of corners 0..3 needs the swap (even permutation)
constexpr unsigned ISO_ODD = 0x26u;      // bit q: tetrahedron q has an odd axis permutation

__device__ __forceinline__ int iso_edge_vertex(const IsoWs& ws, const IsoGrid& g, unsigned p, unsigned codes, unsigned a, unsigned b) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  const unsigned c_lo = (codes >> (3u * lo)) & 7u, c_hi = (codes >> (3u * hi)) & 7u;
  return iso_vertex_id(ws, iso_corner(g, p, c_lo), (c_hi ^ c_lo) - 1u);
}

__device__ __forceinline__ void iso_write_face(int* __restrict__ faces, long long ti, long long nf, int a, int b, int c, bool swap) {
  if (ti < nf) {
    faces[(size_t)ti * 3 + 0] = a;
    faces[(size_t)ti * 3 + 1] = swap ? c : b;
    faces[(size_t)ti * 3 + 2] = swap ? b : c;
  }
}

__global__ __launch_bounds__(ISO_BLOCK) void k_iso_faces(IsoGrid g, int flip, IsoWs ws, int* __restrict__ faces, long long nf) {
  const unsigned p = blockIdx.x * ISO_BLOCK + threadIdx.x;
  if (p >= g.n) return;
  const unsigned k = p % (unsigned)g.G2, r = p / (unsigned)g.G2;
  const unsigned j = r % (unsigned)g.G1, i = r / (unsigned)g.G1;
  if (!(i + 1 < (unsigned)g.G0 && j + 1 < (unsigned)g.G1 && k + 1 < (unsigned)g.G2)) return;   // not the lower corner of a cube
  const unsigned f = ws.flags[p];
  const unsigned in0 = f >> 7;
  // every edge of a cube's lower corner exists, so its flags give the eight inside bits
  const unsigned m = in0 | ((((f & 0x7fu) ^ (in0 ? 0x7fu : 0u)) & 0x7fu) << 1);
  if (m == 0u || m == 0xffu) return;
  long long ti = (long long)(iso_prefix(ws, p) >> 32);
  for (int q = 0; q < 6; ++q) {
    const unsigned codes = iso_tet_codes(q);
    const unsigned s = iso_tet_mask(m, codes);
    const int ni = __popc(s);
    if (ni == 0 || ni == 4) continue;
    const bool swap = ((((ISO_SWAP >> s) ^ (ISO_ODD >> q)) & 1u) != 0u) != (flip != 0);
    if (ni != 2) {
      const unsigned u = (unsigned)__ffs((int)(ni == 1 ? s : (~s & 15u))) - 1u;
      const unsigned w1 = u == 0u ? 1u : 0u, w2 = u <= 1u ? 2u : 1u, w3 = u <= 2u ? 3u : 2u;
      iso_write_face(faces, ti, nf, iso_edge_vertex(ws, g, p, codes, u, w1), iso_edge_vertex(ws, g, p, codes, u, w2),
                     iso_edge_vertex(ws, g, p, codes, u, w3), swap);
      ++ti;
    } else {
      const unsigned o = ~s & 15u;
      const unsigned a = (unsigned)__ffs((int)s) - 1u, b = 31u - (unsigned)__clz((int)s);
      const unsigned c = (unsigned)__ffs((int)o) - 1u, d = 31u - (unsigned)__clz((int)o);
      const int e_ac = iso_edge_vertex(ws, g, p, codes, a, c), e_bd = iso_edge_vertex(ws, g, p, codes, b, d);
      iso_write_face(faces, ti, nf, e_ac, iso_edge_vertex(ws, g, p, codes, a, d), e_bd, swap);
      iso_write_face(faces, ti + 1, nf, e_ac, e_bd, iso_edge_vertex(ws, g, p, codes, b, c), swap);
      ti += 2;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static inline unsigned iso_chunks(unsigned n) { return (n + ISO_BLOCK - 1) / ISO_BLOCK; }

static void carve_iso(IsoWs& w, WsCarver& c, size_t n) {
  w.flags = c.take<uint8_t>(n);
  w.local = c.take<ushort2>(n);
  size_t m = n;
  for (int l = 0; l < 3; ++l) {
    m = (m + ISO_BLOCK - 1) / ISO_BLOCK;
    w.s[l] = c.take<iso_u64>(m);
  }
}

// the limits of the 32-bit vertex and triangle numbering; 0 when the shape is served
static int iso_shape_refused(const char* what, int G0, int G1, int G2) {
  RDRF_CHECK(G0 >= 2 && G1 >= 2 && G2 >= 2, -1, "%s: every side of the lattice must have at least 2 samples, not %d x %d x %d", what,
             G0, G1, G2);
  const double points = (double)G0 * G1 * G2, cubes = (double)(G0 - 1) * (G1 - 1) * (G2 - 1);
  RDRF_CHECK(7.0 * points < 2147483648.0, -1, "%s: %d x %d x %d has 7 x %.0f possible vertices, the indices are 32-bit", what, G0,
             G1, G2, points);
  RDRF_CHECK(12.0 * cubes < 2147483648.0, -1, "%s: %d x %d x %d has 12 x %.0f possible triangles, the indices are 32-bit", what, G0,
             G1, G2, cubes);
  return 0;
}

extern "C" size_t rdrf_iso_ws_bytes(int G0, int G1, int G2) {
  if (iso_shape_refused("iso_ws_bytes", G0, G1, G2)) return 0;
  IsoWs w;
  WsCarver c;
  carve_iso(w, c, (size_t)G0 * G1 * G2);
  return c.off;
}

static int iso_setup(const char* what, int G0, int G1, int G2, int T, int t_index, void* ws, size_t ws_bytes, IsoGrid& g, IsoWs& w) {
  RDRF_TRY(iso_shape_refused(what, G0, G1, G2));
  RDRF_CHECK(T >= 1 && t_index >= 0 && t_index < T, -1, "%s: time slice %d of %d", what, t_index, T);
  RDRF_CHECK(ws != nullptr, -3, "%s: no workspace", what);
  g.G0 = G0; g.G1 = G1; g.G2 = G2; g.T = T; g.t_index = t_index;
  g.n = (unsigned)((size_t)G0 * G1 * G2);
  WsCarver c(ws, ws_bytes);
  carve_iso(w, c, g.n);
  RDRF_CHECK(c.ok(), -3, "%s: workspace too small: need %zu have %zu", what, c.off, ws_bytes);
  return 0;
}

extern "C" int rdrf_iso_count(const float* vol, int G0, int G1, int G2, int T, int t_index, float level, void* ws, size_t ws_bytes,
                              int64_t* counts, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  IsoGrid g;
  IsoWs w;
  RDRF_TRY(iso_setup("iso_count", G0, G1, G2, T, t_index, ws, ws_bytes, g, w));
  RDRF_CHECK(vol && counts, -1, "iso_count: bad arguments");
  const unsigned n0 = iso_chunks(g.n), n1 = iso_chunks(n0), n2 = iso_chunks(n1);   // n2 <= 256: one chunk at the top
  RDRF_LAUNCH("iso_count", k_iso_count, dim3(n0), dim3(ISO_BLOCK), stream, vol, g, level, w);
  RDRF_LAUNCH("iso_scan", k_iso_scan, dim3(n1), dim3(ISO_BLOCK), stream, w.s[0], n0, w.s[1], (int64_t*)nullptr);
  RDRF_LAUNCH("iso_scan", k_iso_scan, dim3(n2), dim3(ISO_BLOCK), stream, w.s[1], n1, w.s[2], (int64_t*)nullptr);
  RDRF_LAUNCH("iso_scan", k_iso_scan, dim3(1), dim3(ISO_BLOCK), stream, w.s[2], n2, (iso_u64*)nullptr, counts);
  return 0;
}

extern "C" int rdrf_iso_emit(const float* vol, int G0, int G1, int G2, int T, int t_index, float level, const float* aabb6, int flip,
                             const void* ws, float* verts, float* normals, int* faces, int64_t nv, int64_t nf,
                             rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  IsoGrid g;
  IsoWs w;
  // (the workspace is the one rdrf_iso_count carved and checked)
  RDRF_TRY(iso_setup("iso_emit", G0, G1, G2, T, t_index, (void*)ws, ~(size_t)0, g, w));
  RDRF_CHECK(vol && aabb6 && nv >= 0 && nf >= 0 && (verts || nv == 0) && (faces || nf == 0), -1, "iso_emit: bad arguments");
  IsoBox box;
  const int G[3] = {G0, G1, G2};
  for (int d = 0; d < 3; ++d) {
    box.lo[d] = aabb6[d];
    box.ext[d] = aabb6[3 + d] - aabb6[d];
    box.den[d] = (float)(G[d] - 1);
    box.h[d] = box.ext[d] / box.den[d];
  }
  const unsigned n0 = iso_chunks(g.n);
  if (nv > 0)
    RDRF_LAUNCH("iso_verts", k_iso_verts, dim3(n0), dim3(ISO_BLOCK), stream, vol, g, level, box, w, verts, normals, (long long)nv);
  if (nf > 0) RDRF_LAUNCH("iso_faces", k_iso_faces, dim3(n0), dim3(ISO_BLOCK), stream, g, flip, w, faces, (long long)nf);
  return 0;
}
