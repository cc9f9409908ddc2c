// The variational bound taken apart: for B rows of the loss heads (x, gamma_0, gamma_1, gamma_t, the diffusion weight,
// eps_0, eps, z_t and the network output, as mulan_qsample_fwd and mulan_diffloss_fwd read them), the per-element terms
//   d_i     = 1/2 w_i r_i^2, r = eps - eps_hat                        (mode 2)
//           = 1/2 (1 - sigma_i^2) w_i r_i^2, r = v* - v_hat           (modes 0, 1; mode 1 rebuilds v_hat from z_t and eps_hat)
//   rho_i   = -log softmax_j(-1/2 u_j^2)[x_i] over the non-zero bin window (loss_terms.h)
//   kappa_i = 1/2 ((1 - v1) f^2 + v1 - log v1 - 1)
// (the arithmetic of qsample_fwd_kernel and diffloss_kernel<false> in vdm_loss.hip, restated) are reduced in both
// directions without ever being written as [B, 3072] arrays:
//   rows_out [B, 8]        per row: sum d, sum d per channel (sub-pixel i is channel i % 3) x3, sum rho, sum kappa,
//                          sum r^2, and the mean of the factor that multiplies 1/2 r^2 (w, or (1 - sigma^2) w)
//   cols_out [G, 3, 3072]  per group of R consecutive rows (B = G R): the mean over its rows of d_i, rho_i, kappa_i
// each optional.
//
// Geometry.  Grid (G, ceil(R / CHUNK)), 256 threads; CHUNK = 8 rows is a compile-time constant.  Block (g, c) walks the
// rows g R + c CHUNK ... of its chunk in ascending order.  Thread `tid` owns the twelve sub-pixels 1024 j + 4 tid + q
// (j < 3, q < 4) of every row -- three 16-byte loads per fp32 array and row, one 4-byte load of x -- which is channel
// (j + q + tid) % 3.  Its 3 x 12 column partials stay in registers and go to workspace [G, chunks, 3, 3072] once; the
// second kernel (grid (G, 9) x 256 threads x one float4: exactly [G, 3, 3072]) folds the chunks and divides by R.  Both
// grids cover their work exactly.
//
// Summation orders (one each, no floating-point atomics; nothing depends on the device or on B):
//   a row sum   per thread over its twelve sub-pixels in the order j, q; the 64 lanes of a wave by the xor butterfly
//               (offsets 32, 16, ... 1); the four waves as ((w0 + w1) + w2) + w3.  The channel sums likewise, each
//               thread's three slots rotated to channels first.  Column 7 is that sum / 3072.
//   a column    within a chunk (0 + row_0) + row_1 + ... in ascending row order; the chunks as (c_0 + c_1) + c_2 + ...
//               in ascending chunk order; then one division by R.
//
// gfx950 (hipcc -O3): 176 VGPRs, no scratch, 256 B of LDS for the main kernel (the unrolled twelve sub-pixels with their
// bin loops, beside the 36 column partials); 14 VGPRs for the fold.
//
// LDS hand-over between rows, one barrier per row: the four waves' partials are kept once per parity of the row's index
// in the chunk, so what row n leaves for threads 0..7 to read after its barrier is next written at row n + 2, behind the
// barrier of row n + 1, which the readers pass after reading.
#include "common.h"
#include "loss_terms.h"

namespace {

constexpr int D = 3072;
constexpr int NT = 256;
constexpr int VPT = D / (NT * 4);      // 16-byte vectors per thread, array and row
constexpr int EPT = VPT * 4;
constexpr int CHUNK = 8;               // rows per block
constexpr int FOLD_BLOCKS = 3 * D / (NT * 4);

struct BpArgs {
  int mode;                                      // 0 velocity, 1 velocity-from-epsilon, 2 epsilon
  const unsigned char* x;                        // [B, D]
  const float* g0; const float* g1; const float* gt; const float* w; int per_elem;   // [B, D], or [B] per row
  const float* eps0; const float* eps; const float* zt; const float* net;            // [B, D]
  float* rows;                                   // [B, 8] or null
  float* ws;                                     // [G, chunks, 3, D] or null
  int R, chunks;
};

__device__ __forceinline__ f32x4 ld_gamma(const float* p, size_t o, size_t b, int per_elem) {
  if (per_elem) return ld_stream4(p + o);
  const float v = p[b];
  return f32x4{v, v, v, v};
}

__global__ __launch_bounds__(NT) void bound_profile_kernel(BpArgs p) {
  __shared__ float red[2][4][8];
  const int tid = threadIdx.x, wave = tid >> 6;
  const bool first_lane = (tid & 63) == 0;
  const int rot = tid % 3;             // sub-pixel 1024 j + 4 tid + q is channel (j + q + rot) % 3
  const int g = blockIdx.x, c = blockIdx.y;
  const int r_begin = c * CHUNK, r_end = min(p.R, r_begin + CHUNK);
  float acc[3][EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) acc[0][k] = acc[1][k] = acc[2][k] = 0.f;
  int par = 0;
  for (int r = r_begin; r < r_end; ++r, par ^= 1) {
    const size_t b = (size_t)g * p.R + r;
    float s_d = 0.f, cs[3] = {0.f, 0.f, 0.f}, s_rho = 0.f, s_kap = 0.f, s_r2 = 0.f, s_fac = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const size_t o = b * D + (size_t)(j * NT + tid) * 4;
      const uint32_t xw = *reinterpret_cast<const uint32_t*>(p.x + o);
      const f32x4 g0v = ld_gamma(p.g0, o, b, p.per_elem), g1v = ld_gamma(p.g1, o, b, p.per_elem),
                  gtv = ld_gamma(p.gt, o, b, p.per_elem), wv = ld_gamma(p.w, o, b, p.per_elem);
      const f32x4 e0v = ld_stream4(p.eps0 + o), epv = ld_stream4(p.eps + o), ntv = ld_stream4(p.net + o);
      f32x4 ztv = {0.f, 0.f, 0.f, 0.f};
      if (p.mode == 1) ztv = ld_stream4(p.zt + o);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = j * 4 + q;
        const int xv = (int)((xw >> (8 * q)) & 255u);
        const float f = encode_u8((unsigned char)xv);
        // reconstruction: -log softmax_j(-0.5 ((z - v_j) e^{-g0/2})^2)[x]   (qsample_fwd_kernel)
        const float g0 = g0v[q];
        const float z0 = f + expf(0.5f * g0) * e0v[q];
        const float istd = expf(-0.5f * g0);
        int jlo, jhi;
        bin_window(z0, istd, jlo, jhi);
        float mx = -INFINITY;
        for (int m = jlo; m <= jhi; ++m) {
          const float u = (z0 - bin_val(m)) * istd;
          mx = fmaxf(mx, -0.5f * u * u);
        }
        float se = 0.f;
        for (int m = jlo; m <= jhi; ++m) {
          const float u = (z0 - bin_val(m)) * istd;
          se += expf(-0.5f * u * u - mx);
        }
        const float ux = (z0 - bin_val(xv)) * istd;
        const float rho = -((-0.5f * ux * ux - mx) - logf(se));
        // latent KL
        const float v1 = sigmoid_f(g1v[q]);
        const float kap = 0.5f * ((1.f - v1) * f * f + v1 - logf(v1) - 1.f);
        // diffusion term   (diffloss_kernel<false>)
        const float gt = gtv[q], gp = wv[q], eps = epv[q], net = ntv[q];
        float res, fac;
        if (p.mode == 2) {
          res = eps - net;
          fac = gp;
        } else {
          const float s = sigmoid_f(gt), al = sqrtf(1.f - s), sg = sqrtf(s);
          const float vstar = al * eps - sg * f;
          float vhat = net;
          if (p.mode == 1) {
            const float eg2 = expf(0.5f * gt);
            const float sq = sqrtf(1.f + expf(gt));
            vhat = -eg2 * ztv[q] + sq * net;
          }
          res = vstar - vhat;
          fac = (1.f - s) * gp;
        }
        const float d = 0.5f * fac * res * res;
        s_d += d;
        cs[(j + q) % 3] += d;
        s_rho += rho;
        s_kap += kap;
        s_r2 += res * res;
        s_fac += fac;
        acc[0][k] += d;
        acc[1][k] += rho;
        acc[2][k] += kap;
      }
    }
    if (p.rows) {
      // this thread's slot k = (j + q) % 3 holds channel (k + rot) % 3
      const float ch0 = rot == 0 ? cs[0] : rot == 1 ? cs[2] : cs[1];
      const float ch1 = rot == 0 ? cs[1] : rot == 1 ? cs[0] : cs[2];
      const float ch2 = rot == 0 ? cs[2] : rot == 1 ? cs[1] : cs[0];
      const float w8[8] = {wave_sum(s_d), wave_sum(ch0), wave_sum(ch1), wave_sum(ch2),
                           wave_sum(s_rho), wave_sum(s_kap), wave_sum(s_r2), wave_sum(s_fac)};
      if (first_lane) {
#pragma unroll
        for (int k = 0; k < 8; ++k) red[par][wave][k] = w8[k];
      }
      __syncthreads();
      if (tid < 8) {
        const float s = ((red[par][0][tid] + red[par][1][tid]) + red[par][2][tid]) + red[par][3][tid];
        p.rows[b * 8 + tid] = tid == 7 ? s / (float)D : s;
      }
    }
  }
  if (p.ws) {
    float* out = p.ws + ((size_t)g * p.chunks + c) * 3 * D;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const f32x4 v = {acc[t][j * 4], acc[t][j * 4 + 1], acc[t][j * 4 + 2], acc[t][j * 4 + 3]};
        *reinterpret_cast<f32x4*>(out + (size_t)t * D + (size_t)(j * NT + tid) * 4) = v;
      }
  }
}

// cols[g] = ((ws[g][0] + ws[g][1]) + ...) / R: block (g, y) folds the 256 float4 at y * 256 of the 3 * D / 4 of group g
__global__ __launch_bounds__(NT) void bound_profile_fold_kernel(const float* __restrict__ ws, float* __restrict__ cols,
                                                                int chunks, int R) {
  const size_t e = ((size_t)blockIdx.y * NT + threadIdx.x) * 4;
  const float* in = ws + (size_t)blockIdx.x * chunks * 3 * D + e;
  f32x4 s = ld_stream4(in);
  for (int c = 1; c < chunks; ++c) s += ld_stream4(in + (size_t)c * 3 * D);
  *reinterpret_cast<f32x4*>(cols + (size_t)blockIdx.x * 3 * D + e) = s / (float)R;
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

MULAN_API size_t mulan_bound_profile_workspace(int B, int rows_per_group) {
  if (B <= 0 || rows_per_group <= 0 || B % rows_per_group != 0) return 0;
  const size_t chunks = ((size_t)rows_per_group + CHUNK - 1) / CHUNK;
  return (size_t)(B / rows_per_group) * chunks * 3 * D * sizeof(float);
}

MULAN_API int mulan_bound_profile(int mode, const unsigned char* x, const float* g0, const float* g1, const float* gt,
                                  const float* w, int per_element_gamma, const float* eps0, const float* eps,
                                  const float* zt, const float* net, float* rows_out, float* cols_out, float* workspace,
                                  int B, int d, int rows_per_group, hipStream_t stream) {
  const int R = rows_per_group;
  if (d != D || B <= 0 || R <= 0 || B % R != 0 || mode < 0 || mode > 2) return (int)hipErrorInvalidValue;
  if (!x || !g0 || !g1 || !gt || !w || !eps0 || !eps || !net || (mode == 1 && !zt)) return (int)hipErrorInvalidValue;
  if ((!rows_out && !cols_out) || (cols_out && !workspace)) return (int)hipErrorInvalidValue;
  const int chunks = (R + CHUNK - 1) / CHUNK;
  if (chunks > 65535) return (int)hipErrorInvalidValue;            // (grid.y)
  if (misaligned(x, 4) || misaligned(eps0, 16) || misaligned(eps, 16) || misaligned(zt, 16) || misaligned(net, 16) ||
      misaligned(cols_out, 16) || misaligned(workspace, 16))
    return (int)hipErrorInvalidValue;
  if (per_element_gamma && (misaligned(g0, 16) || misaligned(g1, 16) || misaligned(gt, 16) || misaligned(w, 16)))
    return (int)hipErrorInvalidValue;
  const int G = B / R;
  BpArgs a{mode, x, g0, g1, gt, w, per_element_gamma ? 1 : 0, eps0, eps, zt, net, rows_out,
           cols_out ? workspace : nullptr, R, chunks};
  hipLaunchKernelGGL(bound_profile_kernel, dim3((unsigned)G, (unsigned)chunks), dim3(NT), 0, stream, a);
  if (cols_out)
    hipLaunchKernelGGL(bound_profile_fold_kernel, dim3((unsigned)G, FOLD_BLOCKS), dim3(NT), 0, stream, workspace, cols_out,
                       chunks, R);
  MULAN_CHECK_LAUNCH();
}
