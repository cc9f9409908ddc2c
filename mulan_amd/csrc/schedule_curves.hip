// The learned noise schedule on a time grid, per embedding (the data behind the reference's noise_schedule_per_embedding
// and its heat-map / histogram views, ldm/notebook_utils.py:554-667): for E embeddings with coefficients a, b, c
// [E, 3072] and T times, in one launch,
//   gamma_out [E, T, 3072]    gamma_i(t) = gamma_min + R P_i(t) / S_i (the form of vdm_loss.hip and schedule_grid.hip)
//   stats_out [E, T, 8]       over the 3072 sub-pixels: mean, population standard deviation, min, max, the three channel
//                             means (sub-pixel i is channel i % 3), the mean of sigma^2 = sigmoid(gamma)
//   hist_out  [E, T, bins]    counts of min(bins - 1, (int)((gamma - gamma_min) * (bins / R)))
// each optional, so the summaries can be had without the curves ever being written.
//
// Values.  With z = 2 t - 1 and q(t) = a t^2 + b t + c = al z^2 + be z + ga (al = a / 4, be = (a + b) / 2,
// ga = a / 4 + b / 2 + c), P(t) = int_0^t q^2 = (G(z) - G(-1)) / 2 for the quintic G(z) = al^2 z^5 / 5 + al be z^4 / 2 +
// (be^2 + 2 al ga) z^3 / 3 + be ga z^2 + ga^2 z, and z = -1 is a root of G(z) - G(-1): dividing it out leaves
//   gamma_i(t) = gamma_min + R t Q_i(z),   Q_i(z) = e0 + z (e1 + z (e2 + z (e3 + z e4))),
// five ratios e_k = d_k / S per sub-pixel (d_4 = g_5, d_k = g_{k+1} - d_{k+1}, g_k the coefficients of G) and Horner in
// the centred time.  It is the same polynomial as the monomials in t of vdm_loss.hip, in a basis in which it is well
// conditioned: in the direction (a, b, c) ~ (6, -6, 1) the monomial ratios are (5, -30, 80, -90, 36) and sum to 1, a
// cancellation that costs fp32 4e-4 of gamma however S is formed, while the e_k are (1, 0.25, -0.25, -2.25, 2.25).  The
// factor t makes t = 0 give gamma_min bit for bit; a = b = 0 gives e = (1, 0, 0, 0, 0) exactly.  The ratios are formed
// once per sub-pixel and block, in double, and rounded to fp32 once (S as the sum of squares of schedule_grid.hip,
// legendre_scale; one reciprocal per sub-pixel), so the error that is left is the fp32 Horner's.  A time costs five fmaf
// and two products per sub-pixel.
//
// Geometry.  A block of 256 threads takes one embedding and a chunk of consecutive times.  Thread `tid` owns the twelve
// sub-pixels 1024 j + 4 tid + q (j < 3, q < 4): three 16-byte loads of each of a, b, c, and per time three 16-byte
// stores -- a wave stores 1 KiB contiguous per instruction; the 60 ratios stay in registers.
// The chunk is chosen by the launch: the largest of 16, 8, 4, 2, 1 times that still gives 1024 blocks (four per CU, what
// 128 VGPRs admit), else 1 -- E = 2, T = 128 is 256 blocks of one time each, E = 3840, T = 128 is 30720 blocks of 16.
// Blocks of one embedding are neighbours in x, so a, b, c (36 KiB) are fetched once per XCD and then served by its L2.
//
// Reductions.  Sums are taken of x = gamma - gamma_min = R p, not of gamma, so equal values (t = 0: x = 0) give exactly
// mean = min = max = gamma_min and deviation 0.  Per thread in the order j, q; lanes by the xor butterfly; the four waves
// in wave order by thread 0: one fixed order, no floating-point atomics.  The deviation is a second block reduction of
// (x - mean_x)^2 over the values still in registers.  The histogram is counted with integer LDS atomics (integer adds
// commute).  bins / R is formed once, in fp32, by the host entry point and passed to the kernel.
//
// LDS hand-over between times, two barriers per time (A after the partial sums and the counts, B after the partial
// deviations; B only with stats_out): everything is kept once per parity of the time's index in the block, so what time n
// leaves for thread 0 (or, the counts, for thread k) to read after its last barrier is next written at time n + 2, behind
// barrier A of time n + 1, which the reader passes after reading.  A thread zeroes the bin it has just read.
#include "common.h"

namespace {

constexpr int D = 3072;
constexpr int NT = 256;
constexpr int VPT = D / (NT * 4);      // 16-byte vectors per thread and array
constexpr int MAX_BINS = 256;
constexpr int MAX_CHUNK = 16;
constexpr int FULL_GRID = 1024;        // blocks: four per CU
constexpr int TUNE_CHUNK = 30;         // mulan_set_tuning(30, n), n in 1..16: n times per block whatever the grid size

// S = int_0^1 (a t^2 + b t + c)^2 dt in the shifted Legendre basis: schedule_grid.hip, legendre_scale
__device__ __forceinline__ double legendre_scale(double a, double b, double c) {
  const double u0 = c + 0.5 * b + a * (1.0 / 3.0), u1 = 0.5 * (a + b), u2 = a * (1.0 / 6.0);
  return u0 * u0 + u1 * u1 * (1.0 / 3.0) + u2 * u2 * 0.2;
}

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

__global__ __launch_bounds__(NT) void schedule_curves_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ c, const float* __restrict__ t,
                                                             int E, int T, int chunk, float gmin, float R,
                                                             float bin_scale, int bins, float* __restrict__ gamma_out,
                                                             float* __restrict__ stats_out, int* __restrict__ hist_out) {
  __shared__ float red[2][4][7];       // per wave: sum x, min, max, sum sigmoid, three channel sums of x
  __shared__ float red2[2][4];         // per wave: sum (x - mean_x)^2
  __shared__ int hist[2][MAX_BINS];
  const int tid = threadIdx.x, wave = tid >> 6;
  const bool first_lane = (tid & 63) == 0;
  const int rot = tid % 3;             // sub-pixel 1024 j + 4 tid + q is channel (j + q + rot) % 3
  const int t_begin = blockIdx.x * chunk, t_end = min(T, t_begin + chunk);
  if (hist_out) {
    hist[0][tid] = 0;
    hist[1][tid] = 0;
    __syncthreads();
  }
  int par = 0;
  for (int e = blockIdx.y; e < E; e += gridDim.y) {
    float r[5][VPT * 4];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const size_t i = (size_t)e * D + (size_t)(j * NT + tid) * 4;
      const f32x4 av = ld_stream4(a + i), bv = ld_stream4(b + i), cv = ld_stream4(c + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double aq = av[q], bq = bv[q], cq = cv[q];
        const double inv_s = 1.0 / legendre_scale(aq, bq, cq);
        const double al = 0.25 * aq, be = 0.5 * (aq + bq), ga = al + 0.5 * bq + cq;
        const double d4 = al * al * 0.2, d3 = al * be * 0.5 - d4, d2 = (be * be + 2.0 * al * ga) * (1.0 / 3.0) - d3,
                     d1 = be * ga - d2, d0 = ga * ga - d1;
        r[0][j * 4 + q] = (float)(d0 * inv_s);
        r[1][j * 4 + q] = (float)(d1 * inv_s);
        r[2][j * 4 + q] = (float)(d2 * inv_s);
        r[3][j * 4 + q] = (float)(d3 * inv_s);
        r[4][j * 4 + q] = (float)(d4 * inv_s);
      }
    }
    for (int ti = t_begin; ti < t_end; ++ti, par ^= 1) {
      const float tv = t[ti], z = fmaf(2.f, tv, -1.f);
      const size_t row = (size_t)e * T + ti;
      float x[VPT * 4];
      float sum = 0.f, lo = INFINITY, hi = -INFINITY, sig = 0.f, cs[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        f32x4 g;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = j * 4 + q;
          const float p = tv * fmaf(z, fmaf(z, fmaf(z, fmaf(z, r[4][k], r[3][k]), r[2][k]), r[1][k]), r[0][k]);
          x[k] = R * p;
          g[q] = fmaf(R, p, gmin);
          if (stats_out) {
            sum += x[k];
            cs[(j + q) % 3] += x[k];
            lo = fminf(lo, g[q]);
            hi = fmaxf(hi, g[q]);
            sig += sigmoid_f(g[q]);
          }
          if (hist_out) {
            const int bin = (int)((g[q] - gmin) * bin_scale);
            atomicAdd(&hist[par][max(0, min(bins - 1, bin))], 1);
          }
        }
        if (gamma_out) *reinterpret_cast<f32x4*>(gamma_out + row * D + (size_t)(j * NT + tid) * 4) = g;
      }
      if (stats_out) {
        // this thread's slot k = (j + q) % 3 holds channel (k + rot) % 3
        const float ch0 = rot == 0 ? cs[0] : rot == 1 ? cs[2] : cs[1];
        const float ch1 = rot == 0 ? cs[1] : rot == 1 ? cs[0] : cs[2];
        const float ch2 = rot == 0 ? cs[2] : rot == 1 ? cs[1] : cs[0];
        const float w[7] = {wave_sum(sum), wave_min(lo), wave_max(hi), wave_sum(sig),
                            wave_sum(ch0), wave_sum(ch1), wave_sum(ch2)};
        if (first_lane) {
#pragma unroll
          for (int k = 0; k < 7; ++k) red[par][wave][k] = w[k];
        }
      }
      if (stats_out || hist_out) __syncthreads();                                   // barrier A
      if (stats_out) {
        const float mean_x = (((red[par][0][0] + red[par][1][0]) + red[par][2][0]) + red[par][3][0]) / (float)D;
        float dev = 0.f;
#pragma unroll
        for (int k = 0; k < VPT * 4; ++k) dev += (x[k] - mean_x) * (x[k] - mean_x);
        dev = wave_sum(dev);
        if (first_lane) red2[par][wave] = dev;
        __syncthreads();                                                            // barrier B
        if (tid == 0) {
          float s[7];
#pragma unroll
          for (int k = 0; k < 7; ++k) {
            const float v0 = red[par][0][k], v1 = red[par][1][k], v2 = red[par][2][k], v3 = red[par][3][k];
            s[k] = k == 1 ? fminf(fminf(v0, v1), fminf(v2, v3)) : k == 2 ? fmaxf(fmaxf(v0, v1), fmaxf(v2, v3))
                                                                          : ((v0 + v1) + v2) + v3;
          }
          const float var = (((red2[par][0] + red2[par][1]) + red2[par][2]) + red2[par][3]) / (float)D;
          const f32x4 o0 = {gmin + mean_x, sqrtf(var), s[1], s[2]};
          const f32x4 o1 = {gmin + s[4] / (float)(D / 3), gmin + s[5] / (float)(D / 3), gmin + s[6] / (float)(D / 3),
                            s[3] / (float)D};
          *reinterpret_cast<f32x4*>(stats_out + row * 8) = o0;
          *reinterpret_cast<f32x4*>(stats_out + row * 8 + 4) = o1;
        }
      }
      if (hist_out && tid < bins) {
        hist_out[row * bins + tid] = hist[par][tid];
        hist[par][tid] = 0;
      }
    }
  }
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

MULAN_API int mulan_schedule_curves(const float* a, const float* b, const float* c, int E, int d, const float* t, int T,
                                    float gamma_min, float gamma_max, float* gamma_out, float* stats_out, int* hist_out,
                                    int bins, hipStream_t stream) {
  if (!a || !b || !c || !t || (!gamma_out && !stats_out && !hist_out) || d != D || E < 1 || T < 1 ||
      (hist_out && (bins < 1 || bins > MAX_BINS)) || !(gamma_min < gamma_max))
    return (int)hipErrorInvalidValue;
  if (misaligned(a) || misaligned(b) || misaligned(c) || misaligned(gamma_out) || misaligned(stats_out))
    return (int)hipErrorInvalidValue;
  int chunk = g_mulan_tune[TUNE_CHUNK];
  if (chunk < 1 || chunk > MAX_CHUNK) {
    chunk = MAX_CHUNK;
    while (chunk > 1 && (long long)E * ((T + chunk - 1) / chunk) < FULL_GRID) chunk >>= 1;
  }
  while ((T + chunk - 1) / chunk > 65535) chunk <<= 1;      // (grid.x; the kernel's chunk is a loop bound, any size runs)
  const float R = gamma_max - gamma_min;
  const float bin_scale = hist_out ? (float)bins / R : 0.f;
  hipLaunchKernelGGL(schedule_curves_kernel, dim3((unsigned)((T + chunk - 1) / chunk), (unsigned)min(E, 65535)), dim3(NT),
                     0, stream, a, b, c, t, E, T, chunk, gamma_min, R, bin_scale, hist_out ? bins : 0, gamma_out,
                     stats_out, hist_out);
  MULAN_CHECK_LAUNCH();
}
