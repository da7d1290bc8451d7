// rdrf_scene.hip -- batch assembly of a training set that lives on the device (train.py:1043-1060: the
// iteration's `allrgbs[ray_idx]`, `alldisps[ray_idx]`, `allflows_f[ray_idx]`, ... -- a dozen index launches there).
//   one launch, one thread per ray: every per-ray tensor of the iteration is written from the ray's flat pixel index.
//   colours may be stored as uint8 (converted as float(x) / 255.0f), the three masks as bits of one byte; pixel centre,
//   integer pixel, frame and time are arithmetic on the index (ids2pixel, train.py:96-103) in the operation order of
//   the fp32 tables a loader would gather them from: (float)col + 0.5f, (float)view * (float)(2.0 / (T - 1)) - 1.0f,
//   each operation rounded on its own (no contraction).
#include "rdrf_host.hpp"

namespace {
struct GatherArgs {
  RdrfSceneTables t;
  RdrfBatch o;
  const int64_t *ids, *ids2;
  int64_t hw;      // H * W
  float dt;        // (float)(2.0 / (T - 1))
  int rgb_word;    // the uint8 colour table starts on a 4-byte boundary: a pixel may be read as one 32-bit word
  int N;
};
}  // namespace

__global__ __launch_bounds__(256) void k_gather_batch(GatherArgs a) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.N) return;
  const int64_t id = a.ids[k];
  const int W = a.t.W, H = a.t.H;
  // ---- colours
  float r, g, b;
  if (a.t.rgb_u8) {
    const uint8_t* p = (const uint8_t*)a.t.rgb;
    const int64_t e = 3 * id;
    const int sh = (int)(e & 3);
    // the three bytes lie inside the aligned word at e - sh when sh <= 1; with sh == 0 the word's fourth byte is the next
    // pixel's, which the table's last pixel does not have
    if (a.rgb_word && (sh == 1 || (sh == 0 && id + 1 < (int64_t)a.t.T * a.hw))) {
      const uint32_t w = *(const uint32_t*)(p + (e - sh)) >> (8 * sh);
      r = (float)(w & 255u); g = (float)((w >> 8) & 255u); b = (float)((w >> 16) & 255u);
    } else {
      r = (float)p[e]; g = (float)p[e + 1]; b = (float)p[e + 2];
    }
    r = r / 255.0f; g = g / 255.0f; b = b / 255.0f;
  } else {
    const float* p = (const float*)a.t.rgb + 3 * id;
    r = p[0]; g = p[1]; b = p[2];
  }
  float* orgb = a.o.rgb + (size_t)k * 3;
  orgb[0] = r; orgb[1] = g; orgb[2] = b;
  // ---- per-pixel scalars and the packed masks
  a.o.disp[k] = a.t.disp ? a.t.disp[id] : 0.0f;
  const unsigned m = a.t.masks[id];
  a.o.fg[k] = (float)(m & 1u);
  a.o.mask_f[k] = (float)((m >> 1) & 1u);
  a.o.mask_b[k] = (float)((m >> 2) & 1u);
  ((float2*)a.o.flow_f)[k] = ((const float2*)a.t.flow_f)[id];
  ((float2*)a.o.flow_b)[k] = ((const float2*)a.t.flow_b)[id];
  // ---- what the index alone decides
  const int64_t view = id / a.hw;
  const float col = (float)(int)(id % W), row = (float)(int)((id / W) % H);
  a.o.view[k] = view;
  a.o.ts[k] = (float)view * a.dt - 1.0f;
  a.o.ts_rand[k] = (float)(a.ids2[k] / a.hw) * a.dt - 1.0f;
  ((float2*)a.o.grid)[k] = make_float2(col + 0.5f, row + 0.5f);
  ((float2*)a.o.px)[k] = make_float2(col, row);
}

extern "C" int rdrf_gather_batch(const RdrfSceneTables* tables, const int64_t* ids, const int64_t* ids2, int N,
                                 RdrfBatch* out, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, the outputs are not touched
  RDRF_CHECK(tables && out && ids && ids2 && N > 0, -1, "gather_batch: bad arguments");
  const RdrfSceneTables& t = *tables;
  RDRF_CHECK(t.T >= 2 && t.H > 0 && t.W > 0, -1, "gather_batch: T = %d (>= 2: the time axis is 2 / (T - 1) wide), H = %d, W = %d",
             t.T, t.H, t.W);
  RDRF_CHECK(t.rgb && t.flow_f && t.flow_b && t.masks, -1, "gather_batch: the colour, flow and mask tables are required");
  const RdrfBatch& o = *out;
  RDRF_CHECK(o.rgb && o.disp && o.fg && o.mask_f && o.mask_b && o.flow_f && o.flow_b && o.ts && o.ts_rand && o.grid && o.px &&
                 o.view, -1, "gather_batch: every output of RdrfBatch is required");
  const uintptr_t al8 = (uintptr_t)t.flow_f | (uintptr_t)t.flow_b | (uintptr_t)o.flow_f | (uintptr_t)o.flow_b |
                        (uintptr_t)o.grid | (uintptr_t)o.px;
  RDRF_CHECK((al8 & 7) == 0, -1, "gather_batch: the [.][2] tables and outputs must be 8-byte aligned");
  GatherArgs a;
  a.t = t;
  a.o = o;
  a.ids = ids;
  a.ids2 = ids2;
  a.hw = (int64_t)t.H * t.W;
  a.dt = (float)(2.0 / (double)(t.T - 1));
  a.rgb_word = ((uintptr_t)t.rgb & 3) == 0;
  a.N = N;
  RDRF_LAUNCH("gather_batch", k_gather_batch, dim3((N + 255) / 256), dim3(256), stream, a);
  return 0;
}
