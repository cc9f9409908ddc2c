// Time grids of the few-step samplers that are uniform in a function of the mean schedule (not in the reference).
// NoiseSchedule_polynomial_fixedend pins every sub-pixel to gamma(0) = gamma_min, gamma(1) = gamma_max:
//   gamma_i(t) = gamma_min + R P_i(t) / S_i,  P_i(t) = c^2 t + b c t^2 + (b^2 + 2 a c) t^3 / 3 + a b t^4 / 2 + a^2 t^5 / 5,
// S_i = P_i(1) (poly_scale of vdm_loss.hip), so the mean over a batch's sub-pixels is again a quintic without a constant
// term: gamma_bar(t) = gamma_min + R sum_k m_k t^k, m the mean of the five ratios (c^2, b c, (b^2 + 2 a c) / 3, a b / 2,
// a^2 / 5) / S.  gamma_bar' is a mean of squares (a t^2 + b t + c)^2 / S with c >= 1e-3, so gamma_bar is strictly
// increasing and gamma_bar(t) = target has one root in [0, 1].
//   schedule_moments : the five ratios' means per sample, [B, 5]
//   schedule_invert  : the batch mean of those rows and one root per target
#include "common.h"

namespace {

constexpr int D = 3072;
constexpr int EPT = D / 256;   // elements per thread

// S = int_0^1 (a t^2 + b t + c)^2 dt.  The monomial form (poly_scale) is a quadratic form in (a, b, c) through the 3 x 3
// Hilbert matrix, condition 524: near its null direction (a, b, c) ~ (6, -6, 1) the fp32 terms cancel and S loses up to
// 1e-5 of its value -- on the very elements whose ratios are largest, which alone costs the mean 8e-7.  In the shifted
// Legendre basis q = u0 + u1 (2 t - 1) + u2 (6 t^2 - 6 t + 1) the same integral is a sum of squares,
// S = u0^2 + u1^2 / 3 + u2^2 / 5, whose only cancellation is inside u0 and enters S through 2 u0 du <= 2 sqrt(S) du:
// the square root of that condition.  Measured in fp32 on the host over the test's input families: 5.8e-8 against 8.3e-7.
__device__ __forceinline__ float legendre_scale(float a, float b, float c) {
  const float u0 = c + 0.5f * b + a * (1.f / 3.f), u1 = 0.5f * (a + b), u2 = a * (1.f / 6.f);
  return u0 * u0 + u1 * u1 * (1.f / 3.f) + u2 * u2 * 0.2f;
}

// One block per sample.  Thread t takes elements t, t + 256, ... of its sample in that order, a wave sums its lanes by
// the xor butterfly, wave 0's first five lanes add the four waves' sums in wave order: one fixed order, no atomics.
__global__ __launch_bounds__(256) void schedule_moments_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                               const float* __restrict__ c, float* __restrict__ m) {
  __shared__ float red[4][5];
  const size_t base = (size_t)blockIdx.x * D;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const size_t i = base + (size_t)e * 256 + threadIdx.x;
    const float av = a[i], bv = b[i], cv = c[i];
    const float r = 1.f / legendre_scale(av, bv, cv);
    acc[0] += cv * cv * r;
    acc[1] += bv * cv * r;
    acc[2] += (bv * bv + 2.f * av * cv) * (1.f / 3.f) * r;
    acc[3] += av * bv * 0.5f * r;
    acc[4] += av * av * 0.2f * r;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] = wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    m[(size_t)blockIdx.x * 5 + k] = (((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) * (1.f / (float)D);
  }
}

// One thread per target.  Every thread forms the batch mean of the moments itself, in double, in the order b = 0 .. B - 1
// (5 B loads of one cache line or a few: cheaper than a launch of its own), then halves the bracket [0, 1] on the quintic
// in double 48 times: 2^-48, far below the fp32 spacing of any t in (0, 1].  The midpoint is rounded to fp32 once.
__global__ __launch_bounds__(64) void schedule_invert_kernel(const float* __restrict__ m, int B,
                                                             const double* __restrict__ targets, int M, double gmin,
                                                             double gmax, float* __restrict__ t_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= M) return;
  const double target = targets[i];
  if (!(target < gmax)) { t_out[i] = 1.f; return; }       // (a NaN target lands here too: an end, not a loop on NaN)
  if (target <= gmin) { t_out[i] = 0.f; return; }
  double mm[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int bb = 0; bb < B; ++bb) {
#pragma unroll
    for (int k = 0; k < 5; ++k) mm[k] += (double)m[(size_t)bb * 5 + k];
  }
  const double R = (gmax - gmin) / (double)B;              // (the mean's 1 / B folded into the range)
  double lo = 0.0, hi = 1.0;
  for (int it = 0; it < 48; ++it) {
    const double t = 0.5 * (lo + hi);
    const double g = gmin + R * (t * (mm[0] + t * (mm[1] + t * (mm[2] + t * (mm[3] + t * mm[4])))));
    if (g < target) lo = t; else hi = t;
  }
  t_out[i] = (float)(0.5 * (lo + hi));
}

}  // namespace

MULAN_API int mulan_schedule_moments(const float* a, const float* b, const float* c, int B, int d, float* m_out,
                                     hipStream_t stream) {
  if (!a || !b || !c || !m_out || B < 1 || d != D) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(schedule_moments_kernel, dim3((unsigned)B), dim3(256), 0, stream, a, b, c, m_out);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_schedule_invert(const float* m, int B, const double* targets, int M, double gamma_min,
                                    double gamma_max, float* t_out, hipStream_t stream) {
  if (!m || !targets || !t_out || B < 1 || M < 1 || !(gamma_min < gamma_max)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(schedule_invert_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, stream, m, B, targets, M,
                     gamma_min, gamma_max, t_out);
  MULAN_CHECK_LAUNCH();
}
