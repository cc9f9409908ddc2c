// Ancestral sampler steps: the elementwise part of VDM.sample / conditional_sample and
// VDM.generate_x of the reference (ldm/model_mulan_velocity.py:281-368, ldm/model_mulan_epsilon.py:377-460,
// ldm/model_vdm.py:182-227).  The 1000 U-Net evaluations in between are the forward kernels of the train path.
#include "common.h"

namespace {

// z_s = sqrt(a/b) (z_t - sigma_t c eps_hat) + sqrt((1-a) c) eps,   a = sigmoid(-g_s), b = sigmoid(-g_t),
// c = -expm1(g_s - g_t), sigma_t = sqrt(sigmoid(g_t)), alpha_t = sqrt(sigmoid(-g_t));
// mode 0 (velocity): eps_hat = net alpha_t + sigma_t z_t;  mode 1 (epsilon): eps_hat = net;
// mode 2 (plain VDM, reparam_type 'input'): eps_hat = (z_t - alpha_t net) / sigma_t.
// gamma is per element (g_per_sample = 0, [n]) or per sample (g_per_sample = d: [n / d], the plain VDM).
__global__ void ancestral_step_kernel(const float* __restrict__ zt, const float* __restrict__ net,
                                      const float* __restrict__ gt, const float* __restrict__ gs,
                                      const float* __restrict__ eps, float* __restrict__ zs, size_t n, int mode,
                                      int g_per_sample) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t gi = g_per_sample ? i / (size_t)g_per_sample : i;
    const float g_t = gt[gi], g_s = gs[gi];
    const float a = sigmoid_f(-g_s), b = sigmoid_f(-g_t), c = -expm1f(g_s - g_t);
    const float sigma_t = sqrtf(sigmoid_f(g_t));
    const float z = zt[i];
    float eh = net[i];
    if (mode == 0) eh = eh * sqrtf(b) + sigma_t * z;
    if (mode == 2) eh = (z - sqrtf(b) * eh) / sigma_t;
    zs[i] = sqrtf(a / b) * (z - sigma_t * c * eh) + sqrtf(sigmoid_f(g_s) * c) * eps[i];   // 1 - a = sigmoid(g_s), without the cancellation
  }
}

// x = argmax_j of the 256-bin decoder logits of EncDec.decode (ldm/model_vdm.py:282-296) at
// z_0 / sqrt(1 - sigmoid(g_0)):  logits_j = -0.5 ((z - v_j) exp(-0.5 g_0))^2,  v_j = 2 (j + 0.5) / 256 - 1
// (first maximum wins, like jnp.argmax)
// sample != 0: jax.random.categorical(logits) instead of the argmax (sample_softmax = True), drawn by the Gumbel-max
// trick with Philox noise: counter (offset + 64 i + j / 4) so every (element, bin) has its own draw
__global__ void decode_argmax_kernel(const float* __restrict__ z0, const float* __restrict__ g0,
                                     unsigned char* __restrict__ out, size_t n, int g_per_sample, int sample,
                                     unsigned long long seed, unsigned long long offset) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float g = g0[g_per_sample ? i / (size_t)g_per_sample : i];
    const float z = z0[i] / sqrtf(1.f - sigmoid_f(g));
    const float inv_stdev = expf(-0.5f * g);
    float best = -INFINITY;
    int arg = 0;
    for (int j4 = 0; j4 < 64; ++j4) {
      float gum[4] = {0.f, 0.f, 0.f, 0.f};
      if (sample) {
        const Philox4 r = philox4x32_10(seed, offset + (unsigned long long)i * 64ull + j4, 0ull);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)   // (2^24 - 1) + 0.5 is a tie that rounds to 2^24: u = 1.0f, whose Gumbel is +inf
          gum[e] = -logf(-logf(fminf(((float)(w[e] >> 8) + 0.5f) * 5.9604644775390625e-08f, 0.99999994f)));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j4 * 4 + e;
        const float v = 2.f * (((float)j + 0.5f) / 256.f) - 1.f;
        const float d = (z - v) * inv_stdev;
        const float l = -0.5f * d * d + gum[e];
        if (l > best) { best = l; arg = j; }
      }
    }
    out[i] = (unsigned char)arg;
  }
}

// EncDec.decode (ldm/model_vdm.py:282-296) as a table: out[i, j] = log_softmax_j(-0.5 ((z_i - v_j) exp(-0.5 g_i))^2), the 256
// decoder log-probabilities of every sub-pixel.  One wave per element (4 bins per lane, one 1 KB row written per wave);
// the train / eval path never materialises this table (mulan_qsample_fwd evaluates the bin of x in registers): this
// entry point backs the reference's module-level EncDec.decode / EncDec.__call__.
__global__ __launch_bounds__(256) void decode_logprobs_kernel(const float* __restrict__ z, const float* __restrict__ g0,
                                                              float* __restrict__ out, size_t n, int g_per_sample) {
  const int lane = threadIdx.x & 63;
  for (size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (size_t)gridDim.x * 4) {
    const float g = g0[g_per_sample ? i / (size_t)g_per_sample : i];
    const float zi = z[i], istd = expf(-0.5f * g);
    float l[4], mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = 2.f * (((float)(lane * 4 + e) + 0.5f) / 256.f) - 1.f;
      const float u = (zi - v) * istd;
      l[e] = -0.5f * u * u;
      mx = fmaxf(mx, l[e]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float se = expf(l[0] - mx) + expf(l[1] - mx) + expf(l[2] - mx) + expf(l[3] - mx);
    se = wave_sum(se);
    // (l - mx) first: both are O(1e4 .. 1e6), their difference is exact; adding log(se) to mx would round it away
    const float ls = logf(se);
    float4 o4 = make_float4((l[0] - mx) - ls, (l[1] - mx) - ls, (l[2] - mx) - ls, (l[3] - mx) - ls);
    *reinterpret_cast<float4*>(out + i * 256 + lane * 4) = o4;
  }
}

// out[r] = mean of x[r, 0:cols]  (VDM._get_score_model_gt, ldm/model_mulan_velocity.py:141-146); one wave per row
__global__ __launch_bounds__(256) void rowmean_kernel(const float* __restrict__ x, float* __restrict__ out, int rows,
                                                      int cols) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += x[(size_t)row * cols + c];
  s = wave_sum(s);
  if (lane == 0) out[row] = s / (float)cols;
}

int grid_for(size_t n) { return (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256); }

}  // namespace

MULAN_API int mulan_ancestral_step(const float* zt, const float* net, const float* gt, const float* gs, const float* eps,
                                   float* zs, size_t n, int mode, int g_per_sample, hipStream_t stream) {
  if (n == 0 || mode < 0 || mode > 2 || g_per_sample < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ancestral_step_kernel, dim3(grid_for(n)), dim3(256), 0, stream, zt, net, gt, gs, eps, zs, n, mode,
                     g_per_sample);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_decode_argmax(const float* z0, const float* g0, unsigned char* out, size_t n, int g_per_sample,
                                  hipStream_t stream) {
  if (n == 0 || g_per_sample < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(decode_argmax_kernel, dim3(grid_for(n)), dim3(256), 0, stream, z0, g0, out, n, g_per_sample, 0, 0ull,
                     0ull);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_decode_logprobs(const float* z, const float* g0, float* out, size_t n, int g_per_sample,
                                    hipStream_t stream) {
  if (n == 0 || g_per_sample < 0 || !z || !g0 || !out) return (int)hipErrorInvalidValue;
  const size_t blocks = (n + 3) / 4;
  hipLaunchKernelGGL(decode_logprobs_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, stream, z, g0,
                     out, n, g_per_sample);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_decode_sample(const float* z0, const float* g0, unsigned char* out, size_t n, int g_per_sample,
                                  unsigned long long seed, unsigned long long offset, hipStream_t stream) {
  if (n == 0 || g_per_sample < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(decode_argmax_kernel, dim3(grid_for(n)), dim3(256), 0, stream, z0, g0, out, n, g_per_sample, 1, seed,
                     offset);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_rowmean(const float* x, float* out, int rows, int cols, hipStream_t stream) {
  if (rows <= 0 || cols <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rowmean_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, out, rows, cols);
  MULAN_CHECK_LAUNCH();
}

// ---- deterministic few-step samplers: DDIM (eta = 0) and DPM-Solver++(2M) per element --------------------------------
// MuLAN's forward process is diagonal, so lambda_i = -gamma_i / 2 is a change of variable per sub-pixel and the
// DPM-Solver++ step holds coordinate by coordinate with the step size h = (g_t - g_s) / 2 of that coordinate:
//   x_hat = alpha_t z_t - sigma_t net (mode 0, velocity) | (z_t - sigma_t net) / alpha_t (mode 1, eps) | net (mode 2)
//   D = x_hat (first order), or with the previous step's (g_p, x_p): w = h / (2 h_p), D = (1 + w) x_hat - w x_p
//   z_s = (sigma_s / sigma_t) z_t - alpha_s expm1(-h) D
// An element whose h_p is not a finite positive number takes the first-order D (the history of a first step, a NaN
// sentinel written by a replayed stepper, a pixel whose schedule did not move): one code path for both orders, so a
// first-order step is the same bits whichever way it was asked for.  At g_s == g_t, sigma_s / sigma_t = 1 and
// expm1(0) = 0: z_s == z_t exactly.
namespace {

__device__ __forceinline__ float fast_step_elem(float z, float nt, float g_t, float g_s, float g_p, float x_p, int mode,
                                                bool second, float* xh_out) {
  const float st2 = sigmoid_f(g_t), ss2 = sigmoid_f(g_s);
  const float alpha_t = sqrtf(sigmoid_f(-g_t)), sigma_t = sqrtf(st2), alpha_s = sqrtf(sigmoid_f(-g_s));
  float xh = nt;
  if (mode == 0) xh = alpha_t * z - sigma_t * nt;
  if (mode == 1) xh = (z - sigma_t * nt) / alpha_t;
  *xh_out = xh;
  const float h = 0.5f * (g_t - g_s);
  float d = xh;
  if (second) {
    const float hp = 0.5f * (g_p - g_t);
    if (hp > 0.f && hp < INFINITY) {
      const float w = h / (2.f * hp);
      d = (1.f + w) * xh - w * x_p;
    }
  }
  return sqrtf(ss2 / st2) * z - alpha_s * expm1f(-h) * d;
}

template <bool VEC>
__global__ __launch_bounds__(256) void fast_sampler_step_kernel(const float* __restrict__ zt, const float* __restrict__ net,
                                                                const float* __restrict__ gt, const float* __restrict__ gs,
                                                                const float* __restrict__ gprev,
                                                                const float* __restrict__ xprev, float* __restrict__ zs,
                                                                float* __restrict__ x0, size_t n, int mode,
                                                                int g_per_sample) {
  const bool second = gprev != nullptr;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (VEC) {
    // n % 4 == 0, every pointer 16-byte aligned, g_per_sample % 4 == 0: the four lanes of a float4 share one gamma
    // per sample, or read a float4 of gamma per element
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n / 4; q += stride) {
      const size_t i = q * 4;
      const float4 z4 = reinterpret_cast<const float4*>(zt)[q], n4 = reinterpret_cast<const float4*>(net)[q];
      float4 gt4, gs4, gp4 = make_float4(0.f, 0.f, 0.f, 0.f), xp4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g_per_sample) {
        const size_t gi = i / (size_t)g_per_sample;
        gt4 = make_float4(gt[gi], gt[gi], gt[gi], gt[gi]);
        gs4 = make_float4(gs[gi], gs[gi], gs[gi], gs[gi]);
        if (second) gp4 = make_float4(gprev[gi], gprev[gi], gprev[gi], gprev[gi]);
      } else {
        gt4 = reinterpret_cast<const float4*>(gt)[q];
        gs4 = reinterpret_cast<const float4*>(gs)[q];
        if (second) gp4 = reinterpret_cast<const float4*>(gprev)[q];
      }
      if (second) xp4 = reinterpret_cast<const float4*>(xprev)[q];
      float4 o, x;
      o.x = fast_step_elem(z4.x, n4.x, gt4.x, gs4.x, gp4.x, xp4.x, mode, second, &x.x);
      o.y = fast_step_elem(z4.y, n4.y, gt4.y, gs4.y, gp4.y, xp4.y, mode, second, &x.y);
      o.z = fast_step_elem(z4.z, n4.z, gt4.z, gs4.z, gp4.z, xp4.z, mode, second, &x.z);
      o.w = fast_step_elem(z4.w, n4.w, gt4.w, gs4.w, gp4.w, xp4.w, mode, second, &x.w);
      reinterpret_cast<float4*>(zs)[q] = o;
      if (x0) reinterpret_cast<float4*>(x0)[q] = x;
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const size_t gi = g_per_sample ? i / (size_t)g_per_sample : i;
      float x;
      zs[i] = fast_step_elem(zt[i], net[i], gt[gi], gs[gi], second ? gprev[gi] : 0.f, second ? xprev[i] : 0.f, mode,
                             second, &x);
      if (x0) x0[i] = x;
    }
  }
}

// memory-bound: one round of at most 2048 blocks (8 per CU), grid-stride beyond
int grid_capped(size_t work) { return (int)((work + 255) / 256 > 2048 ? 2048 : (work + 255) / 256); }

bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

MULAN_API int mulan_fast_sampler_step(const float* zt, const float* net, const float* gt, const float* gs,
                                      const float* gprev, const float* xprev, float* zs, float* x0, size_t n, int mode,
                                      int g_per_sample, hipStream_t stream) {
  if (n == 0 || mode < 0 || mode > 2 || g_per_sample < 0 || !zt || !net || !gt || !gs || !zs ||
      (gprev == nullptr) != (xprev == nullptr) || (g_per_sample && n % (size_t)g_per_sample))
    return (int)hipErrorInvalidValue;
  const bool vec = n % 4 == 0 && (g_per_sample % 4) == 0 && aligned16(zt) && aligned16(net) && aligned16(zs) &&
                   aligned16(x0) && aligned16(xprev) && (g_per_sample || (aligned16(gt) && aligned16(gs) && aligned16(gprev)));
  if (vec)
    hipLaunchKernelGGL(fast_sampler_step_kernel<true>, dim3(grid_capped(n / 4)), dim3(256), 0, stream, zt, net, gt, gs,
                       gprev, xprev, zs, x0, n, mode, g_per_sample);
  else
    hipLaunchKernelGGL(fast_sampler_step_kernel<false>, dim3(grid_capped(n)), dim3(256), 0, stream, zt, net, gt, gs, gprev,
                       xprev, zs, x0, n, mode, g_per_sample);
  MULAN_CHECK_LAUNCH();
}

// ---- stochastic few-step samplers: DDIM with eta in [0, 1] and SDE-DPM-Solver++(2M) per element ---------------------
// The step above with fresh noise xi ~ N(0, 1) per element, read from a buffer (the kernel draws nothing).  With
// h = (g_t - g_s) / 2, c = -expm1(g_s - g_t) = 1 - e^(-2h), x_hat and D as in fast_step_elem:
//   k_z = (sigma_s / sigma_t) sqrt(1 - eta^2 c)
//   k_x = -alpha_s expm1(u),  u = -h + log1p(-eta^2 c) / 2     (= alpha_s (1 - e^(-h) sqrt(1 - eta^2 c)))
//   k_n = eta sigma_s sqrt(c)
//   z_s = k_z z_t + k_x D + k_n xi
// Known answers (tests/test_gpu_stochastic_sampler.py holds the kernel to each):
//   eta = 0: k_z = sigma_s / sigma_t, k_x = -alpha_s expm1(-h), k_n = 0: mulan_fast_sampler_step, i.e. DDIM at first
//     order and DPM-Solver++(2M) at second.
//   eta = 1, first order: k_z = (sigma_s / sigma_t) e^(-h), k_x = alpha_s c, k_n = sigma_s sqrt(c) = sqrt(sigmoid(g_s) c):
//     the ancestral posterior step of ancestral_step_kernel, which is also the first-order SDE-DPM-Solver++ step.
//   eta = 1, second order: SDE-DPM-Solver++(2M) in its midpoint form,
//     z_s = (sigma_s / sigma_t) e^(-h) z_t + alpha_s (1 - e^(-2h)) D + sigma_s sqrt(1 - e^(-2h)) xi.
//   g_s == g_t: c = 0, so k_z = 1, k_x = 0, k_n = 0 and z_s == z_t bit for bit, for every eta, both orders, any finite xi.
// Second order with 0 < eta < 1 interpolates the two coefficient sets; it is no named method.
// 1 - eta^2 c is formed as (1 - eta^2) + eta^2 e^(g_s - g_t): two non-negative terms, so a long step (c -> 1) loses
// nothing to cancellation, and at g_s == g_t the sum rounds to exactly 1 (the error of 1 - eta^2 is below half an ulp
// of 1), so k_z is sqrt(x / x) * sqrt(1) = 1 and not a product that rounds away from it.
namespace {

__device__ __forceinline__ float stochastic_step_elem(float z, float nt, float g_t, float g_s, float g_p, float x_p,
                                                      float xi, float eta, int mode, bool second, float* xh_out) {
  const float st2 = sigmoid_f(g_t), ss2 = sigmoid_f(g_s);
  const float alpha_t = sqrtf(sigmoid_f(-g_t)), sigma_t = sqrtf(st2), alpha_s = sqrtf(sigmoid_f(-g_s));
  float xh = nt;
  if (mode == 0) xh = alpha_t * z - sigma_t * nt;
  if (mode == 1) xh = (z - sigma_t * nt) / alpha_t;
  *xh_out = xh;
  const float h = 0.5f * (g_t - g_s);
  float d = xh;
  if (second) {
    const float hp = 0.5f * (g_p - g_t);
    if (hp > 0.f && hp < INFINITY) {
      const float w = h / (2.f * hp);
      d = (1.f + w) * xh - w * x_p;
    }
  }
  const float e2 = eta * eta;
  const float c = -expm1f(g_s - g_t), q = e2 * c;
  const float om = fmaf(e2, expf(g_s - g_t), 1.f - e2);          // 1 - eta^2 c
  const float u = -h + 0.5f * (q < 0.5f ? log1pf(-q) : logf(om));
  const float k_z = sqrtf(ss2 / st2) * sqrtf(om);
  const float k_x = -alpha_s * expm1f(u);
  const float k_n = eta * sqrtf(ss2) * sqrtf(c);
  return k_z * z + k_x * d + k_n * xi;
}

// one thread per float4 (VEC) or per element, the grid covers n exactly: no grid-stride loop, no cap
template <bool VEC>
__global__ __launch_bounds__(256) void stochastic_sampler_step_kernel(
    const float* __restrict__ zt, const float* __restrict__ net, const float* __restrict__ gt,
    const float* __restrict__ gs, const float* __restrict__ gprev, const float* __restrict__ xprev,
    const float* __restrict__ xi, float eta, float* __restrict__ zs, float* __restrict__ x0, size_t n, int mode,
    int g_per_sample) {
  const bool second = gprev != nullptr;
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    // n % 4 == 0, every pointer 16-byte aligned, g_per_sample % 4 == 0 (as fast_sampler_step_kernel)
    if (q >= n / 4) return;
    const size_t i = q * 4;
    const float4 z4 = reinterpret_cast<const float4*>(zt)[q], n4 = reinterpret_cast<const float4*>(net)[q];
    const float4 e4 = reinterpret_cast<const float4*>(xi)[q];
    float4 gt4, gs4, gp4 = make_float4(0.f, 0.f, 0.f, 0.f), xp4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g_per_sample) {
      const size_t gi = i / (size_t)g_per_sample;
      gt4 = make_float4(gt[gi], gt[gi], gt[gi], gt[gi]);
      gs4 = make_float4(gs[gi], gs[gi], gs[gi], gs[gi]);
      if (second) gp4 = make_float4(gprev[gi], gprev[gi], gprev[gi], gprev[gi]);
    } else {
      gt4 = reinterpret_cast<const float4*>(gt)[q];
      gs4 = reinterpret_cast<const float4*>(gs)[q];
      if (second) gp4 = reinterpret_cast<const float4*>(gprev)[q];
    }
    if (second) xp4 = reinterpret_cast<const float4*>(xprev)[q];
    float4 o, x;
    o.x = stochastic_step_elem(z4.x, n4.x, gt4.x, gs4.x, gp4.x, xp4.x, e4.x, eta, mode, second, &x.x);
    o.y = stochastic_step_elem(z4.y, n4.y, gt4.y, gs4.y, gp4.y, xp4.y, e4.y, eta, mode, second, &x.y);
    o.z = stochastic_step_elem(z4.z, n4.z, gt4.z, gs4.z, gp4.z, xp4.z, e4.z, eta, mode, second, &x.z);
    o.w = stochastic_step_elem(z4.w, n4.w, gt4.w, gs4.w, gp4.w, xp4.w, e4.w, eta, mode, second, &x.w);
    reinterpret_cast<float4*>(zs)[q] = o;
    if (x0) reinterpret_cast<float4*>(x0)[q] = x;
  } else {
    if (q >= n) return;
    const size_t gi = g_per_sample ? q / (size_t)g_per_sample : q;
    float x;
    zs[q] = stochastic_step_elem(zt[q], net[q], gt[gi], gs[gi], second ? gprev[gi] : 0.f, second ? xprev[q] : 0.f, xi[q],
                                 eta, mode, second, &x);
    if (x0) x0[q] = x;
  }
}

}  // namespace

MULAN_API int mulan_stochastic_sampler_step(const float* zt, const float* net, const float* gt, const float* gs,
                                            const float* gprev, const float* xprev, const float* xi, float eta,
                                            float* zs, float* x0, size_t n, int mode, int g_per_sample,
                                            hipStream_t stream) {
  if (n == 0 || mode < 0 || mode > 2 || g_per_sample < 0 || !zt || !net || !gt || !gs || !zs || !xi ||
      (gprev == nullptr) != (xprev == nullptr) || (g_per_sample && n % (size_t)g_per_sample) || !(eta >= 0.f && eta <= 1.f))
    return (int)hipErrorInvalidValue;
  const bool vec = n % 4 == 0 && (g_per_sample % 4) == 0 && aligned16(zt) && aligned16(net) && aligned16(zs) &&
                   aligned16(x0) && aligned16(xprev) && aligned16(xi) &&
                   (g_per_sample || (aligned16(gt) && aligned16(gs) && aligned16(gprev)));
  // every thread owns one float4 (or one element): the grid is the exact cover, refused where it does not fit a launch
  const size_t nb = ((vec ? n / 4 : n) + 255) / 256;
  if (nb > 0x7fffffffull) return (int)hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(stochastic_sampler_step_kernel<true>, dim3((unsigned)nb), dim3(256), 0, stream, zt, net, gt, gs,
                       gprev, xprev, xi, eta, zs, x0, n, mode, g_per_sample);
  else
    hipLaunchKernelGGL(stochastic_sampler_step_kernel<false>, dim3((unsigned)nb), dim3(256), 0, stream, zt, net, gt, gs,
                       gprev, xprev, xi, eta, zs, x0, n, mode, g_per_sample);
  MULAN_CHECK_LAUNCH();
}

// ---- inpainting: the known sub-pixels of a sampler state, and the forward transition q(z_t | z_s) --------------------
// MuLAN's forward process is diagonal, so q(z_t | x) of a known sub-pixel is a closed form per element with its own
// gamma: the replacement method overwrites the known elements of the state after every step with
//   alpha(g) x + sigma(g) xi,   alpha = sqrt(sigmoid(-g)), sigma = sqrt(sigmoid(g)),
// and leaves the others as they are (a select, not a blend: what x and xi hold at an unknown element never reaches
// out).  xi comes from a buffer (the kernel draws nothing); NULL reads as zeros through the same expression, so a zero
// xi and a NULL xi give the same bits, and a known element is then exactly the fp32 product alpha x.
// The forward jump s -> t (g_t >= g_s) is the transition whose Bayes inverse ancestral_step_kernel is:
//   z_t = sqrt(sigmoid(-g_t) / sigmoid(-g_s)) z_s + sqrt(sigmoid(g_t) c) xi,   c = -expm1(g_s - g_t)
// (sigma^2_{t|s} = sigma_t^2 c).  At g_t == g_s the ratio is x / x = 1 and c = 0: z_t == z_s for any finite xi, down to
// the sign of a zero: a noise term that is zero is left out, since -0 + 0 would round to +0.
// Both may run in place (out == z, zt == zs): every thread reads its own elements before it writes them.
namespace {

__device__ __forceinline__ float inpaint_mix_elem(float z, float x, unsigned m, float g, float xi) {
  const float p = sqrtf(sigmoid_f(-g)) * x;
  const float v = fmaf(sqrtf(sigmoid_f(g)), xi, p);
  return m ? v : z;
}

__device__ __forceinline__ float forward_jump_elem(float z, float g_s, float g_t, float xi) {
  const float as2 = sigmoid_f(-g_s), at2 = sigmoid_f(-g_t), c = -expm1f(g_s - g_t);
  const float zr = sqrtf(at2 / as2) * z, nz = sqrtf(sigmoid_f(g_t) * c) * xi;
  return nz == 0.f ? zr : zr + nz;
}

// one thread per float4 (VEC: n % 4 == 0, the float pointers 16-byte and the mask 4-byte aligned, g_per_sample % 4 == 0,
// so a float4 has one 4-byte word of mask) or per element; the grid covers n exactly
template <bool VEC>
__global__ __launch_bounds__(256) void inpaint_mix_kernel(const float* z, const float* __restrict__ x,
                                                          const unsigned char* __restrict__ mask,
                                                          const float* __restrict__ g, const float* __restrict__ xi,
                                                          float* out, size_t n, int g_per_sample) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    if (q >= n / 4) return;
    const float4 z4 = reinterpret_cast<const float4*>(z)[q], x4 = reinterpret_cast<const float4*>(x)[q];
    const float4 e4 = xi ? reinterpret_cast<const float4*>(xi)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    const unsigned m4 = reinterpret_cast<const unsigned*>(mask)[q];
    float4 g4;
    if (g_per_sample) {
      const float gv = g[(q * 4) / (size_t)g_per_sample];
      g4 = make_float4(gv, gv, gv, gv);
    } else {
      g4 = reinterpret_cast<const float4*>(g)[q];
    }
    float4 o;
    o.x = inpaint_mix_elem(z4.x, x4.x, m4 & 0xffu, g4.x, e4.x);
    o.y = inpaint_mix_elem(z4.y, x4.y, m4 & 0xff00u, g4.y, e4.y);
    o.z = inpaint_mix_elem(z4.z, x4.z, m4 & 0xff0000u, g4.z, e4.z);
    o.w = inpaint_mix_elem(z4.w, x4.w, m4 & 0xff000000u, g4.w, e4.w);
    reinterpret_cast<float4*>(out)[q] = o;
  } else {
    if (q >= n) return;
    const size_t gi = g_per_sample ? q / (size_t)g_per_sample : q;
    out[q] = inpaint_mix_elem(z[q], x[q], mask[q], g[gi], xi ? xi[q] : 0.f);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void forward_jump_kernel(const float* zs, const float* __restrict__ gs,
                                                           const float* __restrict__ gt, const float* __restrict__ xi,
                                                           float* zt, size_t n, int g_per_sample) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    if (q >= n / 4) return;
    const float4 z4 = reinterpret_cast<const float4*>(zs)[q], e4 = reinterpret_cast<const float4*>(xi)[q];
    float4 gs4, gt4;
    if (g_per_sample) {
      const size_t gi = (q * 4) / (size_t)g_per_sample;
      gs4 = make_float4(gs[gi], gs[gi], gs[gi], gs[gi]);
      gt4 = make_float4(gt[gi], gt[gi], gt[gi], gt[gi]);
    } else {
      gs4 = reinterpret_cast<const float4*>(gs)[q];
      gt4 = reinterpret_cast<const float4*>(gt)[q];
    }
    float4 o;
    o.x = forward_jump_elem(z4.x, gs4.x, gt4.x, e4.x);
    o.y = forward_jump_elem(z4.y, gs4.y, gt4.y, e4.y);
    o.z = forward_jump_elem(z4.z, gs4.z, gt4.z, e4.z);
    o.w = forward_jump_elem(z4.w, gs4.w, gt4.w, e4.w);
    reinterpret_cast<float4*>(zt)[q] = o;
  } else {
    if (q >= n) return;
    const size_t gi = g_per_sample ? q / (size_t)g_per_sample : q;
    zt[q] = forward_jump_elem(zs[q], gs[gi], gt[gi], xi[q]);
  }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

MULAN_API int mulan_inpaint_mix(const float* z, const float* x, const unsigned char* mask, const float* g,
                                const float* xi, float* out, size_t n, int g_per_sample, hipStream_t stream) {
  if (n == 0 || g_per_sample < 0 || !z || !x || !mask || !g || !out || (g_per_sample && n % (size_t)g_per_sample))
    return (int)hipErrorInvalidValue;
  const bool vec = n % 4 == 0 && (g_per_sample % 4) == 0 && aligned16(z) && aligned16(x) && aligned16(xi) &&
                   aligned16(out) && aligned4(mask) && (g_per_sample || aligned16(g));
  // every thread owns one float4 (or one element): the grid is the exact cover, refused where it does not fit a launch
  const size_t nb = ((vec ? n / 4 : n) + 255) / 256;
  if (nb > 0x7fffffffull) return (int)hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(inpaint_mix_kernel<true>, dim3((unsigned)nb), dim3(256), 0, stream, z, x, mask, g, xi, out, n,
                       g_per_sample);
  else
    hipLaunchKernelGGL(inpaint_mix_kernel<false>, dim3((unsigned)nb), dim3(256), 0, stream, z, x, mask, g, xi, out, n,
                       g_per_sample);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_forward_jump(const float* zs, const float* gs, const float* gt, const float* xi, float* zt, size_t n,
                                 int g_per_sample, hipStream_t stream) {
  if (n == 0 || g_per_sample < 0 || !zs || !gs || !gt || !xi || !zt || (g_per_sample && n % (size_t)g_per_sample))
    return (int)hipErrorInvalidValue;
  const bool vec = n % 4 == 0 && (g_per_sample % 4) == 0 && aligned16(zs) && aligned16(xi) && aligned16(zt) &&
                   (g_per_sample || (aligned16(gs) && aligned16(gt)));
  const size_t nb = ((vec ? n / 4 : n) + 255) / 256;
  if (nb > 0x7fffffffull) return (int)hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(forward_jump_kernel<true>, dim3((unsigned)nb), dim3(256), 0, stream, zs, gs, gt, xi, zt, n,
                       g_per_sample);
  else
    hipLaunchKernelGGL(forward_jump_kernel<false>, dim3((unsigned)nb), dim3(256), 0, stream, zs, gs, gt, xi, zt, n,
                       g_per_sample);
  MULAN_CHECK_LAUNCH();
}
