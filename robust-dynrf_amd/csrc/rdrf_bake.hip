// rdrf_bake.hip -- texture atlases for indexed triangle meshes: the stage that turns a mesh into a point batch (one point per
// texel, on the face that owns the texel) and a point batch into an RGB8 image.  The field evaluation between the two is
// rdrf_query_points (and, for the scene, rdrf_scene_alpha) on chunks of whole squares; no per-sample code lives here.
//
// The atlas (include/rodynrf.h, rdrf_bake_texels, states it; tests/_bake_prim.py restates it in float64): squares of q x q
// texels, R = Wt / q to a row, square s = f >> 1 at (s % R, s / R) q holding face 2s below its anti-diagonal (i + j <= q - 1)
// and face 2s + 1 above it.  A texel's barycentric weights are those of its centre against the face's local corners, so the
// two diagonals i + j = q - 1 and i + j = q lie just outside their triangles and are filled by the same formula with a
// negative w0: a bilinear fetch inside a triangle reads its own face's texels only, without a dilation pass.
//
//   k_bake_texels : a lane per texel -- of the squares [s0, s1) in chunk order ((s - s0) q^2 + j q + i: the batch the field
//                   kernels read), or of the whole atlas in image order (y Wt + x: the public geometry stage).  Writes the
//                   point w0 v0 + w1 v1 + w2 v2, the view direction (one shared vector as given, or minus the unit face normal)
//                   and the face id; a texel no face owns gets the point 0, the direction (0, 0, 1) and face -1
//   k_bake_pack   : a lane per texel of the chunk: rgb (scene: o rgb_d + (1 - o) rgb_s first) -> round-half-even(clamp(., 0, 1)
//                   255) at tex[y][x], `fill` where no face owns the texel; in image order it writes `fill` into what no chunk
//                   covers (squares from ceil(F / 2) on, the columns right of R q, rows below the layout's).  Together the
//                   launches of a call write every byte of the atlas exactly once.
//
// Every product and sum below is a single fp32 operation (no contraction): the texel points are what a numpy float32
// evaluation in the same order gives, and the scene's colours are the bits of the torch expression in mesh.scene_vertex_colors.
// No atomics on global memory: the deterministic build runs the same code.  The calls allocate nothing, do not synchronise
// and read nothing back.
#include "rdrf_host.hpp"

#include <stdint.h>

static_assert((long long)RDRF_BAKE_TEXELS_MAX * RDRF_BAKE_TEXELS_MAX <= RDRF_QUERY_POINTS_MAX, "a chunk holds at least one square");

struct BakeAtlas {
  int F, q, Wt, Ht, R;
};

struct BakeTexelArgs {
  BakeAtlas at;
  const float* verts;   // [nv][3]
  const int* faces;     // [F][3]
  int s0;               // chunk order: the first square
  int image;            // 1: image order over Wt x Ht
  long long n;          // lanes
  int normal;           // 1: minus the unit face normal, 0: `view`
  float view[3];
  float* points;        // [n][3]
  float* viewdirs;      // [n][3]
  int* face;            // [n] or nullptr
};

struct BakePackArgs {
  BakeAtlas at;
  int s0, image;
  long long n;
  const float* rgb;     // [n][3]: the field's colours (scene: the dynamic field's)
  const float* rgb_s;   // scene: [n][3], else nullptr
  const float* owner;   // scene: [n]
  unsigned char fill[3];
  unsigned char* tex;   // [Ht][Wt][3]
};

// the face of texel (i, j) of square s; -1: none (the upper half of the last square of an odd F, squares from ceil(F / 2) on)
RDRF_D int bake_face(int F, int q, int s, int i, int j, bool& upper) {
  upper = i + j > q - 1;
  const int f = 2 * s + (upper ? 1 : 0);
  return f < F ? f : -1;
}

// lane k -> square and local texel; false: the lane has no square (image order: the right margin, rows below the layout's)
RDRF_D bool bake_locate(const BakeAtlas& at, int image, int s0, long long k, int& s, int& i, int& j) {
  if (image) {
    const int x = (int)(k % at.Wt), y = (int)(k / at.Wt);
    if (x >= at.R * at.q) return false;
    s = (y / at.q) * at.R + x / at.q;
    i = x % at.q;
    j = y % at.q;
    return true;
  }
  const int qq = at.q * at.q;
  const int r = (int)(k % qq);
  s = s0 + (int)(k / qq);
  i = r % at.q;
  j = r / at.q;
  return true;
}

// the texel's point and, with `normal`, its face's view direction.  Plain operators under contract(off): one rounding each, in
// the order tests/_bake_prim.py counts its bounds from
RDRF_D void bake_texel(const float* v0, const float* v1, const float* v2, int q, int i, int j, bool upper, bool normal, float* p,
                       float* d) {
#pragma clang fp contract(off)
  const float w1 = upper ? (float)(q - 1 - i) / (float)(q - 3) : (float)i / (float)(q - 2);
  const float w2 = upper ? (float)(q - 1 - j) / (float)(q - 3) : (float)j / (float)(q - 2);
  const float w0 = (1.0f - w1) - w2;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a0 = w0 * v0[c], a1 = w1 * v1[c], a2 = w2 * v2[c];
    const float a01 = a0 + a1;
    p[c] = a01 + a2;
  }
  if (!normal) return;
  // n = (v1 - v0) x (v2 - v0), the orientation of mesh.face_vertex_normals; the direction looks at the face: -n / |n|
  float e1[3], e2[3], n[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e1[c] = v1[c] - v0[c];
    e2[c] = v2[c] - v0[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
    const float l = e1[c1] * e2[c2], r = e1[c2] * e2[c1];
    n[c] = l - r;
  }
  const float xx = n[0] * n[0], yy = n[1] * n[1], zz = n[2] * n[2];
  const float xy = xx + yy;
  const float n2 = xy + zz;
  if (n2 > 0.0f && n2 <= 3.402823466e+38f) {   // false for 0, NaN and an overflow: the face keeps (0, 0, 1)
    const float len = sqrtf(n2);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = -(n[c] / len);
  }
}

__global__ __launch_bounds__(256) void k_bake_texels(BakeTexelArgs a) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < a.n; k += (long long)gridDim.x * blockDim.x) {
    int s = 0, i = 0, j = 0, f = -1;
    bool upper = false;
    if (bake_locate(a.at, a.image, a.s0, k, s, i, j)) f = bake_face(a.at.F, a.at.q, s, i, j, upper);
    float p[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 1.f};
    if (f >= 0) {
      const int* fv = a.faces + (size_t)f * 3;
      bake_texel(a.verts + (size_t)fv[0] * 3, a.verts + (size_t)fv[1] * 3, a.verts + (size_t)fv[2] * 3, a.at.q, i, j, upper,
                 a.normal != 0, p, d);
      if (!a.normal) {
        d[0] = a.view[0]; d[1] = a.view[1]; d[2] = a.view[2];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a.points[(size_t)k * 3 + c] = p[c];
      a.viewdirs[(size_t)k * 3 + c] = d[c];
    }
    if (a.face != nullptr) a.face[k] = f;
  }
}

// round-half-even(clamp(x, 0, 1) * 255) as torch.round(x.clamp(0, 1) * 255).to(uint8); a NaN gives 0
RDRF_D unsigned char bake_quantise(float x) {
  const float c = fminf(fmaxf(x, 0.0f), 1.0f);
  return (unsigned char)(int)rintf(c * 255.0f);
}

// o * rgb_d + (1 - o) * rgb_s as torch evaluates it: four roundings, no contraction
RDRF_D float bake_blend(float o, float rgb_d, float rgb_s) {
#pragma clang fp contract(off)
  const float a = o * rgb_d;
  const float no = 1.0f - o;
  const float b = no * rgb_s;
  return a + b;
}

__global__ __launch_bounds__(256) void k_bake_pack(BakePackArgs a) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < a.n; k += (long long)gridDim.x * blockDim.x) {
    int s = 0, i = 0, j = 0;
    const bool located = bake_locate(a.at, a.image, a.s0, k, s, i, j);
    size_t o;
    int f = -1;
    if (a.image) {
      if (located && 2 * s < a.at.F) continue;   // a square of some chunk: its launch writes it
      o = (size_t)k * 3;
    } else {
      bool upper;
      f = bake_face(a.at.F, a.at.q, s, i, j, upper);
      const int x = (s % a.at.R) * a.at.q + i, y = (s / a.at.R) * a.at.q + j;
      o = ((size_t)y * a.at.Wt + x) * 3;
    }
    unsigned char out[3] = {a.fill[0], a.fill[1], a.fill[2]};
    if (f >= 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = a.rgb[(size_t)k * 3 + c];
        if (a.rgb_s != nullptr) v = bake_blend(a.owner[k], v, a.rgb_s[(size_t)k * 3 + c]);
        out[c] = bake_quantise(v);
      }
    }
    a.tex[o + 0] = out[0]; a.tex[o + 1] = out[1]; a.tex[o + 2] = out[2];
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static inline dim3 bake_grid(long long n) {
  const long long blocks = (n + 255) / 256;
  return dim3((unsigned)(blocks > 8192 ? 8192 : (blocks > 0 ? blocks : 1)));
}

// the layout of F faces in an atlas Wt x Ht with q x q squares; Ht may exceed the layout's q * ceil(ceil(F / 2) / R)
static int bake_atlas(BakeAtlas& at, const char* who, int F, int q, int Wt, int Ht) {
  RDRF_CHECK(F >= 0, -1, "%s: F = %d faces", who, F);
  RDRF_CHECK(q >= RDRF_BAKE_TEXELS_MIN && q <= RDRF_BAKE_TEXELS_MAX, -1, "%s: %d texels per square side, built for %d to %d", who, q,
             RDRF_BAKE_TEXELS_MIN, RDRF_BAKE_TEXELS_MAX);
  RDRF_CHECK(Wt >= q, -1, "%s: an atlas %d texels wide holds no square of %d", who, Wt, q);
  at.F = F; at.q = q; at.Wt = Wt; at.Ht = Ht; at.R = Wt / q;
  const long long nsq = ((long long)F + 1) / 2, rows = (nsq + at.R - 1) / at.R;
  RDRF_CHECK(Ht >= 0 && (long long)Ht >= rows * q, -1, "%s: %d faces in squares of %d need %lld rows of an atlas %d wide, not %d", who, F, q,
             rows * q, Wt, Ht);
  RDRF_CHECK((long long)Wt * Ht < (1ll << 31), -1, "%s: an atlas of %d x %d texels, the limit is 2^31 - 1", who, Wt, Ht);
  return 0;
}

static void bake_view(BakeTexelArgs& a, const float* view) {
  a.normal = view == nullptr ? 1 : 0;
  for (int c = 0; c < 3; ++c) a.view[c] = view != nullptr ? view[c] : 0.f;
}

extern "C" int rdrf_bake_texels(const float* verts, const int* faces, int F, int q, int Wt, int Ht, const float* view, float* points,
                                float* viewdirs, int* face, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BakeTexelArgs a;
  memset(&a, 0, sizeof(a));
  RDRF_TRY(bake_atlas(a.at, "bake_texels", F, q, Wt, Ht));
  a.n = (long long)Wt * Ht;
  if (a.n == 0) return 0;
  RDRF_CHECK(points && viewdirs && (F == 0 || (verts && faces)), -1, "bake_texels: bad arguments");
  a.verts = verts; a.faces = faces; a.image = 1;
  bake_view(a, view);
  a.points = points; a.viewdirs = viewdirs; a.face = face;
  RDRF_LAUNCH("bake_texels", k_bake_texels, bake_grid(a.n), dim3(256), stream, a);
  return 0;
}

struct BakeWs {
  float* points;     // [M][3]
  float* viewdirs;   // [M][3]
  float* rgb;        // [M][3]
  float* rgb_s;      // scene: [M][3]
  float* owner;      // scene: [M]
  char* sub;         // the workspace of the field calls, one after the other on the stream
  size_t sub_bytes;
};
// one layout for the size call and the launch; M = the points of one chunk
static void carve_bake(BakeWs& p, WsCarver& c, int scene, int dynamic, int M) {
  const size_t m = M > 0 ? (size_t)M : 0;
  memset(&p, 0, sizeof(p));
  p.points = c.take<float>(m * 3);
  p.viewdirs = c.take<float>(m * 3);
  p.rgb = c.take<float>(m * 3);
  if (scene) {
    p.rgb_s = c.take<float>(m * 3);
    p.owner = c.take<float>(m);
    p.sub_bytes = rdrf_scene_alpha_ws_bytes(M, 1);
    for (int dyn = 0; dyn < 2; ++dyn) {
      const size_t b = rdrf_query_points_ws_bytes(dyn, M, 0);
      if (b > p.sub_bytes) p.sub_bytes = b;
    }
  } else {
    p.sub_bytes = rdrf_query_points_ws_bytes(dynamic, M, 0);
  }
  p.sub = c.take<char>(p.sub_bytes);
}

static bool bake_chunk_ok(int q, int chunk_squares) {
  return q >= RDRF_BAKE_TEXELS_MIN && q <= RDRF_BAKE_TEXELS_MAX && chunk_squares >= 1 &&
         (long long)chunk_squares * q * q <= RDRF_QUERY_POINTS_MAX;
}

extern "C" size_t rdrf_bake_ws_bytes(int scene, int dynamic, int q, int chunk_squares) {
  if (!bake_chunk_ok(q, chunk_squares)) return 0;   // refused by the bake, by name
  BakeWs p;
  WsCarver c;
  carve_bake(p, c, scene, dynamic, chunk_squares * q * q);
  return c.off;
}

struct BakeCall {
  const char* who;
  const void* P;                  // the field's parameters (scene: the dynamic field's)
  int dynamic;
  const RdrfFieldCfg* cfg;
  const RdrfStaticParams* PS;     // scene: the static field, else nullptr
  const RdrfFieldCfg* cfg_s;
  float length;
  const RdrfAlphaMask *mask_s, *mask_d;
  const float *verts, *view, *t;
  const int* faces;
  int F, q, Wt, Ht, chunk_squares;
  const unsigned char* fill;
  unsigned char* tex;
  void* ws;
  size_t ws_bytes;
  hipStream_t stream;
};

// the launch sequence of both bakes: fill what no square covers, then per chunk of whole squares texels -> colours -> pack
static int bake_run(const BakeCall& b) {
  const bool scene = b.PS != nullptr;
  BakeAtlas at;
  RDRF_TRY(bake_atlas(at, b.who, b.F, b.q, b.Wt, b.Ht));
  const long long texels = (long long)b.Wt * b.Ht;
  if (texels == 0) return 0;
  RDRF_CHECK(b.tex && b.fill, -1, "%s: no atlas or no fill colour", b.who);
  BakePackArgs k;
  memset(&k, 0, sizeof(k));
  k.at = at; k.tex = b.tex;
  for (int c = 0; c < 3; ++c) k.fill[c] = b.fill[c];
  {
    BakePackArgs m = k;
    m.image = 1; m.n = texels;
    RDRF_LAUNCH("bake_fill", k_bake_pack, bake_grid(m.n), dim3(256), b.stream, m);
  }
  if (b.F == 0) return 0;   // an empty mesh: the atlas is filled, no field is touched
  RDRF_CHECK(b.P && b.cfg && b.verts && b.faces && (!scene || b.cfg_s), -1, "%s: bad arguments", b.who);
  RDRF_CHECK(!b.dynamic || b.t != nullptr, -1, "%s: the dynamic field needs the time t", b.who);
  RDRF_CHECK(bake_chunk_ok(b.q, b.chunk_squares), -1, "%s: chunks of %d squares of %d x %d texels, a chunk holds 1 square to %d points",
             b.who, b.chunk_squares, b.q, b.q, RDRF_QUERY_POINTS_MAX);
  RDRF_CHECK(b.ws != nullptr, -3, "%s: no workspace", b.who);
  const int qq = b.q * b.q;
  WsCarver c(b.ws, b.ws_bytes);
  BakeWs p;
  carve_bake(p, c, scene, b.dynamic, b.chunk_squares * qq);
  RDRF_CHECK(c.ok(), -3, "%s: workspace too small: need %zu have %zu", b.who, c.off, b.ws_bytes);

  BakeTexelArgs g;
  memset(&g, 0, sizeof(g));
  g.at = at; g.verts = b.verts; g.faces = b.faces;
  bake_view(g, b.view);
  g.points = p.points; g.viewdirs = p.viewdirs;
  k.rgb = p.rgb; k.rgb_s = p.rgb_s; k.owner = p.owner;
  const int nsq = (b.F + 1) / 2;
  for (int s0 = 0; s0 < nsq; s0 += b.chunk_squares) {
    const int ns = nsq - s0 < b.chunk_squares ? nsq - s0 : b.chunk_squares;
    const int M = ns * qq;
    g.s0 = k.s0 = s0;
    g.n = k.n = M;
    RDRF_LAUNCH("bake_texels", k_bake_texels, bake_grid(M), dim3(256), b.stream, g);
    if (scene) {
      RDRF_TRY(rdrf_scene_alpha(b.PS, b.cfg_s, (const RdrfDynamicParams*)b.P, b.cfg, p.points, M, b.t, 1, b.length, b.mask_s, b.mask_d,
                                nullptr, p.owner, nullptr, nullptr, nullptr, p.sub, p.sub_bytes, b.stream));
      RDRF_TRY(rdrf_query_points(b.PS, 0, b.cfg_s, p.points, M, nullptr, 0, p.viewdirs, nullptr, p.rgb_s, nullptr, nullptr, p.sub,
                                 p.sub_bytes, b.stream));
    }
    RDRF_TRY(rdrf_query_points(b.P, b.dynamic, b.cfg, p.points, M, b.t, 0, p.viewdirs, nullptr, p.rgb, nullptr, nullptr, p.sub,
                               p.sub_bytes, b.stream));
    RDRF_LAUNCH("bake_pack", k_bake_pack, bake_grid(M), dim3(256), b.stream, k);
  }
  return 0;
}

extern "C" int rdrf_bake_texture(const void* params, int dynamic, const RdrfFieldCfg* cfg, const float* verts, const int* faces, int F,
                                 int q, int Wt, int Ht, const float* view, const float* t, const unsigned char* fill, int chunk_squares,
                                 unsigned char* tex, void* ws, size_t ws_bytes, rdrf_stream_t stream) {
  BakeCall b;
  memset(&b, 0, sizeof(b));
  b.who = "bake_texture";
  b.P = params; b.dynamic = dynamic ? 1 : 0; b.cfg = cfg;
  b.verts = verts; b.faces = faces; b.F = F; b.q = q; b.Wt = Wt; b.Ht = Ht; b.view = view; b.t = t; b.fill = fill;
  b.chunk_squares = chunk_squares; b.tex = tex; b.ws = ws; b.ws_bytes = ws_bytes; b.stream = (hipStream_t)stream;
  return bake_run(b);
}

extern "C" int rdrf_bake_scene_texture(const RdrfStaticParams* PS, const RdrfFieldCfg* cfg_s, const RdrfDynamicParams* PD,
                                       const RdrfFieldCfg* cfg_d, const float* verts, const int* faces, int F, int q, int Wt, int Ht,
                                       const float* view, const float* t, float length, const RdrfAlphaMask* mask_s,
                                       const RdrfAlphaMask* mask_d, const unsigned char* fill, int chunk_squares, unsigned char* tex,
                                       void* ws, size_t ws_bytes, rdrf_stream_t stream) {
  RDRF_CHECK(PS != nullptr || (long long)Wt * Ht == 0, -1, "bake_scene_texture: no static field");
  BakeCall b;
  memset(&b, 0, sizeof(b));
  b.who = "bake_scene_texture";
  b.P = PD; b.dynamic = 1; b.cfg = cfg_d; b.PS = PS; b.cfg_s = cfg_s; b.length = length; b.mask_s = mask_s; b.mask_d = mask_d;
  b.verts = verts; b.faces = faces; b.F = F; b.q = q; b.Wt = Wt; b.Ht = Ht; b.view = view; b.t = t; b.fill = fill;
  b.chunk_squares = chunk_squares; b.tex = tex; b.ws = ws; b.ws_bytes = ws_bytes; b.stream = (hipStream_t)stream;
  return bake_run(b);
}
