// rdrf_host.hpp -- host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rdrf_common.hpp"

void rdrf_set_error(const char* fmt, ...);

// Environment switches.  The product library never reads the caller's environment: a C-ABI call's behaviour depends on its
// arguments (and on explicit rdrf_set_* calls) only.  `make tools` builds librodynrf_tools.so with -DRDRF_TOOLS, where
// RDRF_ENV is getenv and three switches select the earlier, independent implementation of a phase for the GPU tests that
// compare the two:
//   RDRF_FLAT=0        wave-per-ray density kernels                              (tests/test_gpu_flat_density.py)
//   RDRF_SF_FUSED=0    k_scene_flow_bwd + dw_sf                                  (tests/test_gpu_scene_flow_fused.py)
//   RDRF_WARP_FUSED=0  k_dyn_density_bwd<1, false, true> + its k_dw3 launches    (tests/test_gpu_warp_dw_fused.py)
// The A/B switches and RDRF_ABL_* ablation blocks of the decided experiments (profiles/LABBOOK.md) were
// removed; commit ea23fff is the last tree that has them.  tests/test_abi_cpu.py holds the list to these three.
#ifdef RDRF_TOOLS
#include <stdlib.h>
#define RDRF_ENV(name) getenv(name)
#else
#define RDRF_ENV(name) ((const char*)nullptr)
#endif

// The dynamic field's density phase on flat 32-sample tiles of the [N * S] sample array (k_dyn_density_flat + k_ray_scan
// forward; k_ray_scan_bwd + k_dyn_density_bwd<., ., true> backward) instead of a wave per ray.  Read once per process, so the
// forward and the backward of a step agree on the saved-row addressing.  RDRF_FLAT=0 (tools build): wave per ray.
inline bool rdrf_flat_density() {
  static const bool flat = !(RDRF_ENV("RDRF_FLAT") != nullptr && atoi(RDRF_ENV("RDRF_FLAT")) == 0);
  return flat;
}

#define RDRF_CHECK(cond, code, ...)  \
  do {                               \
    if (!(cond)) {                   \
      rdrf_set_error(__VA_ARGS__);   \
      return (code);                 \
    }                                \
  } while (0)

#define RDRF_HIP(expr)                                                             \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      rdrf_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return -5;                                                                   \
    }                                                                              \
  } while (0)

// a launch helper's return code, passed on
#define RDRF_TRY(expr)        \
  do {                        \
    int rc_try_ = (expr);     \
    if (rc_try_) return rc_try_; \
  } while (0)

// byte fill as a kernel launch (rdrf_pack.hip): the launch sequences use it instead of hipMemsetAsync, whose memset nodes do
// not replay reliably inside a captured HIP graph
int rdrf_fill_async(void* p, int byte_value, size_t bytes, hipStream_t stream);
#define RDRF_FILL(p, v, bytes, stream)                          \
  do {                                                          \
    int rc_fill_ = rdrf_fill_async((p), (v), (bytes), (stream)); \
    if (rc_fill_) return rc_fill_;                              \
  } while (0)

// optional per-kernel timing with HIP events on the launch stream (bench.py roofline figure)
void rdrf_prof_begin(const char* name, hipStream_t s);
void rdrf_prof_end(const char* name, hipStream_t s);

#define RDRF_LAUNCH(name, kernel, grid, block, stream, ...)            \
  do {                                                                 \
    rdrf_prof_begin(name, stream);                                     \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);   \
    rdrf_prof_end(name, stream);                                       \
    RDRF_HIP(hipGetLastError());                                       \
  } while (0)

static inline Box make_box(const RdrfFieldCfg* cfg) {
  Box b;
  for (int i = 0; i < 3; ++i) {
    b.lo[i] = cfg->aabb[i];
    b.hi[i] = cfg->aabb[3 + i];
    b.inv[i] = 2.0f / (cfg->aabb[3 + i] - cfg->aabb[i]);  // models/tensorBase.py:377
  }
  return b;
}

// workspace carving (all offsets 256-byte aligned).  A layout is written once, as a function of a carver: the entry point
// carves the caller's buffer with it, and the *_workspace_bytes function runs it on a carver without a buffer (measuring
// mode: take() returns nullptr and only advances `off`) and returns the end offset.
struct WsCarver {
  char* base;
  size_t off, cap;
  WsCarver(void* p, size_t c) : base((char*)p), off(0), cap(c) {}
  WsCarver() : base(nullptr), off(0), cap(~(size_t)0) {}   // measuring mode
  template <typename T>
  T* take(size_t n) {
    size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
    T* r = base ? (T*)(base + off) : nullptr;
    off += bytes;
    return r;
  }
  bool ok() const { return off <= cap; }
};

// persistent launch geometry: one workgroup per CU (its LDS holds the kernel's weight image),
// up to 8 waves per workgroup, each wave walking its own rays / tiles.
struct Geo {
  int grid, block;
};
static inline Geo geo_for_units(long units) {
  Geo g;
  const int ncu = 256;
  int waves = (int)((units + ncu - 1) / ncu);
  waves = waves < 1 ? 1 : (waves > RDRF_MAXW ? RDRF_MAXW : waves);
  g.block = waves * 64;
  // one tile per wave: small launches (a 512-ray eval chunk = 1840 tiles) take proportionally fewer CUs -- every workgroup
  // pays the 121-159 KB LDS fill of its weight image once per launch, and independent launches on other streams find free
  // CUs (rdrf_render_chunks_fwd)
  long blocks = (units + waves - 1) / waves;
  g.grid = (int)(blocks < 1 ? 1 : (blocks > ncu ? ncu : blocks));
  return g;
}
static inline Geo geo_for_tiles(int N, int S) { return geo_for_units(((long)N * S + 31) / 32); }
// the CU count of the CURRENT device (a process may drive several), for the launches that size themselves by it
static inline int current_cu_count(int* ncu) {
  int dev = 0;
  RDRF_HIP(hipGetDevice(&dev));
  RDRF_HIP(hipDeviceGetAttribute(ncu, hipDeviceAttributeMultiprocessorCount, dev));
  if (*ncu <= 0) *ncu = 256;
  return 0;
}

// component counts + the three planes / lines span ONE grid (plane XY <-> line Z, XZ <-> Y, YZ <-> X): the forward
// kernels compute one tap per grid axis and share it between the planes (rdrf_common.hpp, shared-tap gather)
static inline bool vm_one_grid(const RdrfVM& v) {
  return v.W[0] == v.W[1] && v.W[0] == v.L[2] && v.H[0] == v.W[2] && v.H[0] == v.L[1] && v.H[1] == v.H[2] && v.H[1] == v.L[0];
}
static inline bool vm_same_grid(const RdrfVM& a, const RdrfVM& b) {
  return a.W[0] == b.W[0] && a.H[0] == b.H[0] && a.L[0] == b.L[0];
}
static inline bool vm_ok(const RdrfVM& v, int c0, int c1) {
  return v.C[0] == c0 && v.C[1] == c1 && v.C[2] == c1 && vm_one_grid(v);
}

// device-wide stable key sort (rdrf_sort.hip)
size_t rdrf_sort_temp_bytes(unsigned n, int bits);
int rdrf_sort_positions(const unsigned* keys_in, unsigned* keys_out, unsigned* vals_out, unsigned n, int bits, void* temp,
                        size_t temp_bytes, hipStream_t stream, const int* n_dev = nullptr, unsigned n_mul = 0);
// the segmented form: nseg independent sorts of seg_len entries (device-side length: *seg_len_dev) over the low `bits` bits,
// values = global positions.  counts != nullptr: a key kernel has written the first pass's tile histograms and drop counts
// into the tables rdrf_sort_tables names (layout: rdrf_sort_dev.hpp); the sort then starts at the scan, which also writes
// counts[segment] = length - dropped
struct RsTables;
size_t rdrf_sort_seg_temp_bytes(int nseg, unsigned seg_len, int bits);
size_t rdrf_sort_carved_bytes(int nseg, unsigned seg_len);   // what the sort carves out of its temporary storage
void rdrf_sort_plan(int bits, int* passes, int* digit_bits);
int rdrf_sort_tables(int nseg, unsigned seg_len, int bits, void* temp, size_t temp_bytes, RsTables* t, int* nbins);
int rdrf_sort_positions_seg(const unsigned* keys_in, unsigned* keys_out, unsigned* vals_out, int nseg, unsigned seg_len, int bits,
                            void* temp, size_t temp_bytes, hipStream_t stream, const int* seg_len_dev = nullptr, int* counts = nullptr);

int rdrf_sort_ints_inplace(int* data, unsigned n, hipStream_t stream);   // deterministic build only

// pack-job builders (rdrf_pack.hip)
void pack_add(PackJobs& J, const float* src, int ld, int out_dim, int in_dim, int seg, int mode,
              int nb, int kk, int dst);
void pack_add_b3(PackJobs& J, const float* src, int ld, int out_dim, int in_dim, int seg, int nb, int kk, int seg_kk0, int kk_off,
                 int kk_tot, int dst);
void pack_add_b3s(PackJobs& J, const float* src, int ld, int out_dim, int in_dim, int seg, int nb, int kk, int seg_kk0, int kk_off,
                  int kk_tot, int dst, int dst_lo);
void pack_add_b3s_t(PackJobs& J, const float* src, int ld, int out_dim, int in_dim, int seg, int nbi, int kk, int dst, int dst_lo);
void pack_add_from(PackJobs& J, const float* src, int ld, int out_dim, int in_dim, int seg, int nb, int kk, int seg_kk0, int dst);
int pack_launch(const PackJobs& J, float* dst, hipStream_t stream);

#define PACK_AREA_FLOATS (1 << 20) /* 4 MiB: forward + transposed packs of either field */

// the job lists of the four weight images (forward: rdrf_fwd.hip, backward: rdrf_bwd.hip) and the kernels' weight-pointer
// structs (rdrf_kernels.hpp; filled in rdrf_fwd.hip)
struct StaticW;
struct DynW;
void static_pack_jobs_fwd(PackJobs& J, const RdrfStaticParams* P, int head);
void dyn_pack_jobs_fwd(PackJobs& J, const RdrfDynamicParams* P);
void static_pack_jobs_bwd(PackJobs& J, const RdrfStaticParams* P, int head);
void dyn_pack_jobs_bwd(PackJobs& J, const RdrfDynamicParams* P);
void fill_static_w(StaticW& w, const RdrfStaticParams* P);
void fill_dyn_w(DynW& w, const RdrfDynamicParams* P);

// The weight image an entry point reads: `packed`, the caller-packed one (rdrf_static_pack / rdrf_dynamic_pack), or the jobs
// of build(J, args...) packed into `area` now.
template <typename... A>
static inline int pack_image(const float*& pk, const float* packed, float* area, hipStream_t stream,
                             void (*build)(PackJobs&, A...), A... args) {
  pk = packed != nullptr ? packed : area;
  if (packed != nullptr) return 0;
  PackJobs J;
  build(J, args...);
  return pack_launch(J, area, stream);
}
