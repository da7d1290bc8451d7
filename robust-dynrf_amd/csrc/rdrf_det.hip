// rdrf_det.hip -- deterministic build (-DRDRF_DETERMINISTIC -> librodynrf_det.so): bind a field's flat gradient buffer to
// its fixed-point shadow in EVERY unit whose kernels call grad_add (rdrf_common.hpp: g_det is one copy per unit), and fold
// the shadow back into the fp32 gradients.  In the product build the entry points report that they are not available.
#include "rdrf_host.hpp"

#ifdef RDRF_DETERMINISTIC
// the units that invoke RDRF_DET_UNIT (rdrf_common.hpp): every unit with a grad_add in a kernel has to be in this list
typedef int (*DetBind)(int slot, const DetMap* m, hipStream_t stream);
int det_bind_bwd(int, const DetMap*, hipStream_t);
int det_bind_bwd_fused(int, const DetMap*, hipStream_t);
int det_bind_scatter(int, const DetMap*, hipStream_t);
int det_bind_dw(int, const DetMap*, hipStream_t);
int det_bind_optim(int, const DetMap*, hipStream_t);
static const DetBind g_det_binders[] = {det_bind_bwd, det_bind_bwd_fused, det_bind_scatter, det_bind_dw, det_bind_optim};
static DetMap g_det_host[2];   // what the slots are bound to; the binders copy from here, so it outlives the call

__global__ void k_det_finish(float* __restrict__ g, unsigned long long* __restrict__ shadow, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const long long v = (long long)shadow[i];
    if (v != 0) {
      g[i] += (float)((double)v * (1.0 / (double)RDRF_DET_SCALE));
      shadow[i] = 0ull;
    }
  }
}
#endif

extern "C" int rdrf_deterministic(void) {
#ifdef RDRF_DETERMINISTIC
  return 1;
#else
  return 0;
#endif
}

extern "C" int rdrf_det_bind(int slot, float* grad_base, size_t n, void* shadow_i64, rdrf_stream_t stream_) {
#ifdef RDRF_DETERMINISTIC
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(slot == 0 || slot == 1, -1, "det_bind: slot 0 (static field) or 1 (dynamic field)");
  g_det_host[slot].base = grad_base;
  g_det_host[slot].n = n;
  g_det_host[slot].shadow = (unsigned long long*)shadow_i64;
  for (DetBind bind : g_det_binders) {
    int rc = bind(slot, &g_det_host[slot], stream);
    if (rc) return rc;
  }
  return 0;
#else
  (void)slot; (void)grad_base; (void)n; (void)shadow_i64; (void)stream_;
  rdrf_set_error("det_bind: this library is the product build (fp32 atomics); load librodynrf_det.so (RDRF_DETERMINISTIC=1)");
  return -1;
#endif
}

extern "C" int rdrf_det_finish(int slot, rdrf_stream_t stream_) {
#ifdef RDRF_DETERMINISTIC
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK((slot == 0 || slot == 1) && g_det_host[slot].shadow != nullptr, -1, "det_finish: slot %d is not bound", slot);
  const size_t n = g_det_host[slot].n;
  RDRF_LAUNCH("det_finish", k_det_finish, dim3((unsigned)((n + 1023) / 1024 > 4096 ? 4096 : (n + 1023) / 1024)), dim3(256), stream,
              (float*)g_det_host[slot].base, g_det_host[slot].shadow, n);
  return 0;
#else
  (void)slot; (void)stream_;
  rdrf_set_error("det_finish: product build");
  return -1;
#endif
}
