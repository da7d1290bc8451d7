// rdrf_eval.hip -- what the evaluation loops need beside the renderer:
//   camera rays : rays of arbitrary c2w cameras (/root/reference/renderer.py:702-716 `evaluation`, :1013-1030
//                 `evaluation_path`; dataLoader/ray_utils.py:93-110 get_ray_directions_blender, :143-160 get_rays,
//                 :197-218 ndc_rays_blender)
//   SSIM        : utils.py:98-151 rgb_ssim (reported beside PSNR by `evaluation`, renderer.py:869-883), in fp64
#include "rdrf_misc_dev.hpp"

// ------------------------------------------------------------------------------------------------
// camera rays: ray k = flat pixel first + k over (B, H, W)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_camera_rays(const float* __restrict__ c2w, const float* __restrict__ focal_p, int H,
                                                     int W, int ndc, float near, int64_t first, int N,
                                                     float* __restrict__ rays) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const int64_t id = first + k;
  const int col = (int)(id % W), row = (int)((id / W) % H);
  const int64_t b = id / ((int64_t)W * H);
  float r[6];
  camera_ray(c2w + b * 12, focal_p[b], (float)col + 0.5f, (float)row + 0.5f, H, W, ndc, near, r);   // pixel centre: meshgrid + 0.5
  float* out = rays + (size_t)k * 6;
  for (int q = 0; q < 6; ++q) out[q] = r[q];
}

extern "C" int rdrf_camera_rays(const float* c2w, const float* focal, int B, int H, int W, int ndc, float near, int64_t first,
                                int N, float* rays, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) return 0;   // empty batch: a no-op, like torch ops on empty tensors (their data pointers are null)
  RDRF_CHECK(c2w && focal && rays && B > 0 && H > 0 && W > 0 && N > 0 && first >= 0, -1, "camera_rays: bad arguments");
  RDRF_CHECK(first + N <= (int64_t)B * H * W, -1, "camera_rays: pixels %lld..%lld lie beyond the %d cameras' %d x %d frames",
             (long long)first, (long long)(first + N - 1), B, H, W);
  RDRF_LAUNCH("camera_rays", k_camera_rays, dim3((N + 255) / 256), dim3(256), stream, c2w, focal, H, W, ndc, near, first, N,
              rays);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// SSIM (rgb_ssim): per channel, the `valid` separable 11-tap Gaussian of x, y, x^2, y^2, x y; variances clipped at 0,
// the covariance clamped to sign * min(sqrt(s00 s11), |s01|); map = (2 mu01 + c1)(2 s01 + c2) / ((mu00 + mu11 + c1)(s00 +
// s11 + c2)); mean over the map.  The reference's float64 filter makes its convolutions float64: here every moment and
// the map are fp64 as well (E[x^2] - mu^2 next to c2 = 9e-4 wants it).
// One workgroup per (16 x 32 output tile, channel): the input tile with its 10-pixel halo is staged in LDS, the horizontal
// pass leaves 26 x 32 rows of the five moments in LDS, the vertical pass forms the map.  The mean: one partial per
// workgroup, each reduced in a fixed order, then one workgroup sums the partials in a fixed order (same bits every run).
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int kTaps = 11, kHalo = kTaps - 1;
constexpr int kTH = 16, kTW = 32;                        // output tile
constexpr int kIH = kTH + kHalo, kIW = kTW + kHalo;      // input tile (26 x 42)
constexpr int kThreads = 256;
struct SsimArgs {
  const float *x, *y;
  int H, W, C, Ho, Wo;
  double g[kTaps];
  double c1, c2;
  float* map;     // nullable
  double* partial;
};
}  // namespace

RDRF_D double block_sum_fixed(double v, double* red) {
  // wave tree (fixed pairing), then the waves' sums in index order by thread 0
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / 64; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(kThreads) void k_ssim_tile(SsimArgs a) {
  __shared__ float sx[kIH][kIW + 1], sy[kIH][kIW + 1];
  __shared__ double hm[5][kIH][kTW];
  __shared__ double red[kThreads / 64];
  const int tid = threadIdx.x, c = blockIdx.z;
  const int oy0 = blockIdx.y * kTH, ox0 = blockIdx.x * kTW;
  for (int p = tid; p < kIH * kIW; p += kThreads) {
    const int r = p / kIW, q = p % kIW, yy = oy0 + r, xx = ox0 + q;
    float u = 0.f, v = 0.f;   // zeros past the image edge feed only outputs past the valid map
    if (yy < a.H && xx < a.W) {
      const size_t e = ((size_t)yy * a.W + xx) * a.C + c;
      u = a.x[e];
      v = a.y[e];
    }
    sx[r][q] = u;
    sy[r][q] = v;
  }
  __syncthreads();
  for (int p = tid; p < kIH * kTW; p += kThreads) {
    const int r = p / kTW, q = p % kTW;
    double m0 = 0.0, m1 = 0.0, m00 = 0.0, m11 = 0.0, m01 = 0.0;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const double u = (double)sx[r][q + k], v = (double)sy[r][q + k], g = a.g[k];
      m0 += g * u; m1 += g * v; m00 += g * (u * u); m11 += g * (v * v); m01 += g * (u * v);
    }
    hm[0][r][q] = m0; hm[1][r][q] = m1; hm[2][r][q] = m00; hm[3][r][q] = m11; hm[4][r][q] = m01;
  }
  __syncthreads();
  double acc = 0.0;
  for (int p = tid; p < kTH * kTW; p += kThreads) {
    const int r = p / kTW, q = p % kTW, oy = oy0 + r, ox = ox0 + q;
    if (oy >= a.Ho || ox >= a.Wo) continue;
    double mu0 = 0.0, mu1 = 0.0, e00 = 0.0, e11 = 0.0, e01 = 0.0;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const double g = a.g[k];
      mu0 += g * hm[0][r + k][q]; mu1 += g * hm[1][r + k][q];
      e00 += g * hm[2][r + k][q]; e11 += g * hm[3][r + k][q]; e01 += g * hm[4][r + k][q];
    }
    const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
    const double s00 = fmax(0.0, e00 - mu00), s11 = fmax(0.0, e11 - mu11);
    double s01 = e01 - mu01;
    const double sg = s01 > 0.0 ? 1.0 : (s01 < 0.0 ? -1.0 : 0.0);
    s01 = sg * fmin(sqrt(s00 * s11), fabs(s01));
    const double v = ((2.0 * mu01 + a.c1) * (2.0 * s01 + a.c2)) / ((mu00 + mu11 + a.c1) * (s00 + s11 + a.c2));
    if (a.map) a.map[((size_t)oy * a.Wo + ox) * a.C + c] = (float)v;
    acc += v;
  }
  const double s = block_sum_fixed(acc, red);
  if (tid == 0) a.partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void k_ssim_finish(const double* __restrict__ partial, int n, double count,
                                                          double* __restrict__ mean_out) {
  __shared__ double red[kThreads / 64];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) v += partial[i];
  const double s = block_sum_fixed(v, red);
  if (threadIdx.x == 0) mean_out[0] = s / count;
}

static void ssim_grid(int H, int W, int C, dim3& grid) {
  const int Ho = H - kHalo, Wo = W - kHalo;
  grid = dim3((unsigned)((Wo + kTW - 1) / kTW), (unsigned)((Ho + kTH - 1) / kTH), (unsigned)C);
}

extern "C" size_t rdrf_ssim_workspace_bytes(int H, int W, int C) {
  if (H < kTaps || W < kTaps || C < 1) return 256;
  dim3 g;
  ssim_grid(H, W, C, g);
  return (size_t)g.x * g.y * g.z * sizeof(double) + 256;
}

extern "C" int rdrf_ssim(const float* img0, const float* img1, int H, int W, int C, float max_val, double* mean_out,
                         float* map_out, void* ws, size_t ws_bytes, rdrf_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RDRF_CHECK(img0 && img1 && mean_out && ws && C >= 1 && C <= 65535, -1, "ssim: bad arguments");
  RDRF_CHECK(H >= kTaps && W >= kTaps, -1, "ssim: the image (%d x %d) must be at least %d x %d (valid 11-tap filter)", H, W,
             kTaps, kTaps);
  RDRF_CHECK(ws_bytes >= rdrf_ssim_workspace_bytes(H, W, C), -3, "ssim: workspace too small");
  SsimArgs a;
  a.x = img0; a.y = img1; a.H = H; a.W = W; a.C = C; a.Ho = H - kHalo; a.Wo = W - kHalo;
  // the filter of rgb_ssim: exp(-0.5 ((i - hw + shift) / sigma)^2), normalised to sum 1
  const int hw = kTaps / 2;
  const double shift = (2 * hw - kTaps + 1) / 2.0, sigma = 1.5;
  double sum = 0.0;
  for (int i = 0; i < kTaps; ++i) {
    const double f = (i - hw + shift) / sigma;
    a.g[i] = exp(-0.5 * (f * f));
    sum += a.g[i];
  }
  for (int i = 0; i < kTaps; ++i) a.g[i] /= sum;
  a.c1 = (0.01 * (double)max_val) * (0.01 * (double)max_val);
  a.c2 = (0.03 * (double)max_val) * (0.03 * (double)max_val);
  a.map = map_out;
  a.partial = (double*)ws;
  dim3 grid;
  ssim_grid(H, W, C, grid);
  RDRF_LAUNCH("ssim", k_ssim_tile, grid, dim3(kThreads), stream, a);
  const int n = (int)(grid.x * grid.y * grid.z);
  RDRF_LAUNCH("ssim_finish", k_ssim_finish, dim3(1), dim3(kThreads), stream, (const double*)a.partial, n,
              (double)a.Ho * a.Wo * C, mean_out);
  return 0;
}
