// Exact t-SNE in two dimensions for N <= 16384 points: the dense affinities P [N, N] of the inputs and one gradient-descent
// iteration on the map Y [N, 2], as sklearn.manifold.TSNE(method='exact') computes them, without a point leaving the chip.
//
// Affinities (mulan_tsne_affinities), three launches:
//   distances   d_ij = sum_d (x_id - x_jd)^2 from the differences (never |a|^2 + |b|^2 - 2ab: near-duplicate rows would
//               cancel), a 64 x 64 tile per block of 256 threads, 4 x 4 per thread, the feature axis staged through LDS
//               16 columns at a time and summed in ascending d; written into P
//   rows        one block per row i: the row sits in LDS (4 N bytes, 64 KB at the cap) less its minimum over j != i, and
//               beta_i is searched so that the entropy H_i(beta) = ln(sum_j p_j) + beta sum_j d_j p_j / sum_j p_j of
//               p_j = exp(-beta d_j) equals ln(perplexity): sklearn's bracketing (beta starts at 1 and doubles or halves
//               while a side is open, then midpoints), with no tolerance and no early exit -- BISECTIONS midpoint steps
//               after the bracket closes, MAX_STEPS steps in all -- so beta ends where the fp32 H crosses the target.
//               Every thread sums its j = tid, tid + 256, ... in that order, a wave folds by the xor tree, thread 0 adds
//               the four waves in order.  The row becomes P_{j|i} = p_j / sum_j p_j, P_{i|i} = 0.
//   symmetrise  P <- (P + P^T) / (2 N) in place, a 32 x 32 tile against its mirror image per block
// Gradient (mulan_tsne_gradient), two launches: a wave per row streams the row of P (16-byte loads when N is a multiple
// of 4) against Y held in LDS (8 N bytes, 128 KB at the cap) with w_ij = 1 / (1 + |y_i - y_j|^2), w_ii = 0, and leaves
//   a_i = sum_j P_ij w_ij (y_i - y_j)   r_i = sum_j w_ij^2 (y_i - y_j)   z_i = sum_j w_ij
//   k_i = sum_{P_ij > 0} P_ij (ln P_ij - ln w_ij), s_i = sum_j P_ij      (only in the instantiation with kl)
// in the workspace (k and s in fp64: their terms cancel to a hundredth of their size); the fold launch takes Z = sum_i z_i in fp64 (thread t of 256 its contiguous slice of the rows in
// index order, then the 256 partial sums in order), writes grad_i = 4 (exaggeration a_i - r_i / Z) and, block 0,
// kl = sum_i k_i + ln Z sum_i s_i.  Update (mulan_tsne_update) is sklearn's _gradient_descent body per element.
// No atomics, one order per sum: the same call returns the same bits.  The gradient is VALU and bandwidth work -- 30
// flops per 4 bytes of P -- so there is no matrix instruction in this file; DESIGN.md section 3.12 has the measurement.
#include "common.h"

namespace {

constexpr int MIN_N = 4, MAX_N = 16384;
constexpr int NT = 256;
constexpr int TD = 64, DK = 16, TDS = TD + 4;    // distance tile, feature columns per stage, LDS row stride (16-byte rows)
constexpr int MAX_STEPS = 100, BISECTIONS = 64;
constexpr int TS = 32;                           // symmetrise tile
constexpr int GRAD_BLOCKS = 512;                 // two blocks per CU of the MI355X: a constant of the library

__global__ __launch_bounds__(NT) void tsne_distance_kernel(const float* __restrict__ x, int N, int D, float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) float si[DK * TDS];        // [k][row of the i tile]
  __shared__ __attribute__((aligned(16))) float sj[DK * TDS];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * TD, j0 = blockIdx.x * TD;
  const int lr = tid >> 2, lk = (tid & 3) * 4;                        // this thread stages row lr, columns lk .. lk + 3
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int k0 = 0; k0 < D; k0 += DK) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = k0 + lk + e;
      const int ri = i0 + lr, rj = j0 + lr;
      si[(lk + e) * TDS + lr] = (ri < N && k < D) ? x[(size_t)ri * D + k] : 0.f;
      sj[(lk + e) * TDS + lr] = (rj < N && k < D) ? x[(size_t)rj * D + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DK; ++k) {
      const f32x4 vi = *reinterpret_cast<const f32x4*>(si + k * TDS + ty * 4);
      const f32x4 vj = *reinterpret_cast<const f32x4*>(sj + k * TDS + tx * 4);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float diff = vi[a] - vj[b];
          acc[a][b] = fmaf(diff, diff, acc[a][b]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ty * 4 + a;
    if (i >= N) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + tx * 4 + b;
      if (j < N) P[(size_t)i * N + j] = acc[a][b];
    }
  }
}

// (sum of a, sum of b) over the block, every thread gets them: xor tree in the wave, the four waves in order
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = a;
    red[4 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  a = ((red[0] + red[1]) + red[2]) + red[3];
  b = ((red[4] + red[5]) + red[6]) + red[7];
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(NT) void tsne_row_kernel(float* __restrict__ P, int N, float target, float* __restrict__ beta_out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];        // [8] reduction cells, then the row [N]
  float* red = smem;
  float* d = smem + 8;
  const int tid = threadIdx.x, i = blockIdx.x;
  float* row = P + (size_t)i * N;
  float lo = INFINITY;
  for (int j = tid; j < N; j += NT) {
    const float v = row[j];
    d[j] = v;
    if (j != i) lo = fminf(lo, v);
  }
  lo = wave_min(lo);
  if ((tid & 63) == 0) red[tid >> 6] = lo;
  __syncthreads();
  lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  for (int j = tid; j < N; j += NT) d[j] = j == i ? 0.f : d[j] - lo;  // (each thread rewrites the cells it wrote)

  float beta = 1.f, bmin = -INFINITY, bmax = INFINITY;
  int bisections = 0;
  for (int step = 0; step < MAX_STEPS && bisections < BISECTIONS; ++step) {
    float sp = 0.f, sdp = 0.f;
    for (int j = tid; j < N; j += NT) {
      const float dj = d[j];
      const float p = j == i ? 0.f : expf(-dj * beta);
      sp += p;
      sdp = fmaf(dj, p, sdp);
    }
    block_sum2(sp, sdp, red);                                         // sp >= 1: the row minimum gives p = 1
    const float H = logf(sp) + beta * sdp / sp;
    if (H - target > 0.f) {
      bmin = beta;
      if (bmax == INFINITY) beta *= 2.f;
      else { beta = (beta + bmax) * 0.5f; ++bisections; }
    } else {
      bmax = beta;
      if (bmin == -INFINITY) beta *= 0.5f;
      else { beta = (beta + bmin) * 0.5f; ++bisections; }
    }
  }
  float sp = 0.f, unused = 0.f;
  for (int j = tid; j < N; j += NT) sp += j == i ? 0.f : expf(-d[j] * beta);
  block_sum2(sp, unused, red);
  for (int j = tid; j < N; j += NT) row[j] = j == i ? 0.f : expf(-d[j] * beta) / sp;
  if (beta_out && tid == 0) beta_out[i] = beta;
}

__global__ __launch_bounds__(NT) void tsne_symmetrise_kernel(float* __restrict__ P, int N) {
  if (blockIdx.x < blockIdx.y) return;                                // the tile below the diagonal belongs to its mirror
  __shared__ float sa[TS][TS + 1];
  __shared__ float sb[TS][TS + 1];
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  const int i0 = blockIdx.y * TS, j0 = blockIdx.x * TS;
  const bool diag = i0 == j0;
  for (int r = r0; r < TS; r += NT / TS) {
    sa[r][c] = (i0 + r < N && j0 + c < N) ? P[(size_t)(i0 + r) * N + j0 + c] : 0.f;
    sb[r][c] = (j0 + r < N && i0 + c < N) ? P[(size_t)(j0 + r) * N + i0 + c] : 0.f;
  }
  __syncthreads();
  const float two_n = 2.f * (float)N;
  for (int r = r0; r < TS; r += NT / TS) {
    if (i0 + r < N && j0 + c < N) P[(size_t)(i0 + r) * N + j0 + c] = (sa[r][c] + sb[c][r]) / two_n;
    if (!diag && j0 + r < N && i0 + c < N) P[(size_t)(j0 + r) * N + i0 + c] = (sb[r][c] + sa[c][r]) / two_n;
  }
}

// the workspace: fp64 k [N], s [N], then fp32 ax, ay, rx, ry, z [N] each
constexpr size_t WS_BYTES_PER_POINT = 2 * sizeof(double) + 5 * sizeof(float);
__host__ __device__ __forceinline__ float* ws_floats(double* ws, int N) { return reinterpret_cast<float*>(ws + 2 * (size_t)N); }
__host__ __device__ __forceinline__ const float* ws_floats(const double* ws, int N) {
  return reinterpret_cast<const float*>(ws + 2 * (size_t)N);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct RowSums {
  float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, z = 0.f;
  double k = 0.0, s = 0.0;
};

template <bool KL>
__device__ __forceinline__ void pair_term(RowSums& t, float p, float yix, float yiy, float yjx, float yjy, bool self) {
  const float dx = yix - yjx, dy = yiy - yjy;
  const float q = 1.f + fmaf(dx, dx, dy * dy);
  const float w = self ? 0.f : 1.f / q;
  const float pw = p * w, w2 = w * w;
  t.ax = fmaf(pw, dx, t.ax);
  t.ay = fmaf(pw, dy, t.ay);
  t.rx = fmaf(w2, dx, t.rx);
  t.ry = fmaf(w2, dy, t.ry);
  t.z += w;
  if constexpr (KL) {
    const double ddx = (double)yix - (double)yjx, ddy = (double)yiy - (double)yjy;
    t.s += (double)p;
    if (p > 0.f) t.k = fma((double)p, log((double)p * (1.0 + fma(ddx, ddx, ddy * ddy))), t.k);
  }
}

template <bool KL, bool VEC>
__global__ __launch_bounds__(NT) void tsne_gradient_rows_kernel(const float* __restrict__ P, const float* __restrict__ Y,
                                                                int N, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float sY[];          // [N][2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < 2 * N; e += NT) sY[e] = Y[e];
  __syncthreads();
  for (int i = blockIdx.x * (NT / 64) + wave; i < N; i += gridDim.x * (NT / 64)) {
    const float yix = sY[2 * i], yiy = sY[2 * i + 1];
    const float* row = P + (size_t)i * N;
    RowSums t;
    if constexpr (VEC) {                                              // N is a multiple of 4: every row starts on 16 bytes
#pragma unroll 2
      for (int j = lane * 4; j < N; j += 256) {
        const f32x4 p = ld_stream4(row + j);
        const f32x4 y01 = *reinterpret_cast<const f32x4*>(sY + 2 * j);
        const f32x4 y23 = *reinterpret_cast<const f32x4*>(sY + 2 * j + 4);
        pair_term<KL>(t, p[0], yix, yiy, y01[0], y01[1], j == i);
        pair_term<KL>(t, p[1], yix, yiy, y01[2], y01[3], j + 1 == i);
        pair_term<KL>(t, p[2], yix, yiy, y23[0], y23[1], j + 2 == i);
        pair_term<KL>(t, p[3], yix, yiy, y23[2], y23[3], j + 3 == i);
      }
    } else {
#pragma unroll 4
      for (int j = lane; j < N; j += 64) pair_term<KL>(t, row[j], yix, yiy, sY[2 * j], sY[2 * j + 1], j == i);
    }
    t.ax = wave_sum(t.ax);
    t.ay = wave_sum(t.ay);
    t.rx = wave_sum(t.rx);
    t.ry = wave_sum(t.ry);
    t.z = wave_sum(t.z);
    if constexpr (KL) {
      t.k = wave_sum_f64(t.k);
      t.s = wave_sum_f64(t.s);
    }
    if (lane == 0) {
      float* f = ws_floats(ws, N);
      f[i] = t.ax;
      f[N + i] = t.ay;
      f[2 * N + i] = t.rx;
      f[3 * N + i] = t.ry;
      f[4 * N + i] = t.z;
      if constexpr (KL) {
        ws[i] = t.k;
        ws[N + i] = t.s;
      }
    }
  }
}

// the sum of v[0 .. N) in fp64: thread t adds its contiguous slice in index order, thread 0 the 256 slices in order
template <typename T>
__device__ __forceinline__ double ordered_sum(const T* __restrict__ v, int N, double* part) {
  const int per = (N + NT - 1) / NT, lo = threadIdx.x * per;
  const int hi = lo + per < N ? lo + per : N;
  double s = 0.0;
  for (int i = lo; i < hi; ++i) s += (double)v[i];
  __syncthreads();                                                    // the last call's readers are done with `part`
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < NT; ++k) t += part[k];
    part[NT] = t;
  }
  __syncthreads();
  return part[NT];
}

template <bool KL>
__global__ __launch_bounds__(NT) void tsne_gradient_fold_kernel(const double* __restrict__ ws, int N, float exaggeration,
                                                                float* __restrict__ grad, double* __restrict__ kl) {
  __shared__ double part[NT + 1];
  const float* f = ws_floats(ws, N);
  const double Z = ordered_sum(f + 4 * (size_t)N, N, part);
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i < N) {
    const double e = (double)exaggeration;
    grad[2 * i] = (float)(4.0 * (e * (double)f[i] - (double)f[2 * (size_t)N + i] / Z));
    grad[2 * i + 1] = (float)(4.0 * (e * (double)f[(size_t)N + i] - (double)f[3 * (size_t)N + i] / Z));
  }
  if constexpr (KL) {
    if (blockIdx.x == 0) {                                            // (uniform over the block: the barriers are safe)
      const double K = ordered_sum(ws, N, part);
      const double S = ordered_sum(ws + N, N, part);
      if (threadIdx.x == 0) *kl = K + log(Z) * S;
    }
  }
}

__global__ __launch_bounds__(NT) void tsne_update_kernel(const float* __restrict__ grad, float* __restrict__ Y,
                                                         float* __restrict__ U, float* __restrict__ G, int n,
                                                         float momentum, float lr) {
  const int e = blockIdx.x * NT + threadIdx.x;
  if (e >= n) return;
  const float g = grad[e], u = U[e];
  float gain = G[e];
  gain = u * g < 0.f ? gain + 0.2f : gain * 0.8f;
  gain = fmaxf(gain, 0.01f);
  const float un = momentum * u - lr * (gain * g);
  G[e] = gain;
  U[e] = un;
  Y[e] += un;
}

bool n_ok(int N) { return MIN_N <= N && N <= MAX_N; }

template <typename K>
hipError_t allow_lds(K kernel, int bytes, bool& done) {
  if (done) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done = true;
  return e;
}

template <bool KL, bool VEC>
hipError_t launch_rows(const float* P, const float* Y, int N, double* ws, hipStream_t stream) {
  static bool configured = false;
  hipError_t e = allow_lds(tsne_gradient_rows_kernel<KL, VEC>, MAX_N * 2 * (int)sizeof(float), configured);
  if (e != hipSuccess) return e;
  const int want = (N + NT / 64 - 1) / (NT / 64);
  const int blocks = want < GRAD_BLOCKS ? want : GRAD_BLOCKS;
  hipLaunchKernelGGL((tsne_gradient_rows_kernel<KL, VEC>), dim3((unsigned)blocks), dim3(NT), (size_t)N * 2 * sizeof(float),
                     stream, P, Y, N, ws);
  return hipSuccess;
}

}  // namespace

MULAN_API size_t mulan_tsne_workspace(int N) {
  return n_ok(N) ? WS_BYTES_PER_POINT * N : 0;
}

MULAN_API int mulan_tsne_affinities(const float* x, int N, int D, float perplexity, int symmetrise, float* P, float* beta,
                                    hipStream_t stream) {
  if (!x || !P || !n_ok(N) || D < 1 || (symmetrise != 0 && symmetrise != 1)) return (int)hipErrorInvalidValue;
  if (!(perplexity >= 1.f && perplexity < (float)(N - 1))) return (int)hipErrorInvalidValue;       // (refuses NaN too)
  if (((uintptr_t)x & 3) || ((uintptr_t)P & 15) || ((uintptr_t)beta & 3)) return (int)hipErrorInvalidValue;
  static bool configured = false;
  hipError_t e = allow_lds(tsne_row_kernel, (MAX_N + 8) * (int)sizeof(float), configured);
  if (e != hipSuccess) return (int)e;
  const unsigned tiles = (unsigned)((N + TD - 1) / TD);
  hipLaunchKernelGGL(tsne_distance_kernel, dim3(tiles, tiles), dim3(NT), 0, stream, x, N, D, P);
  hipLaunchKernelGGL(tsne_row_kernel, dim3((unsigned)N), dim3(NT), (size_t)(N + 8) * sizeof(float), stream, P, N,
                     logf(perplexity), beta);
  if (symmetrise) {
    const unsigned st = (unsigned)((N + TS - 1) / TS);
    hipLaunchKernelGGL(tsne_symmetrise_kernel, dim3(st, st), dim3(NT), 0, stream, P, N);
  }
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_tsne_gradient(const float* P, const float* Y, int N, float exaggeration, float* grad, double* kl,
                                  void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!P || !Y || !grad || !n_ok(N) || !workspace || workspace_bytes < mulan_tsne_workspace(N))
    return (int)hipErrorInvalidValue;
  if (!(exaggeration > 0.f) || exaggeration == INFINITY) return (int)hipErrorInvalidValue;
  if (((uintptr_t)P & 15) || ((uintptr_t)Y & 15) || ((uintptr_t)grad & 3) || ((uintptr_t)kl & 7) || ((uintptr_t)workspace & 15))
    return (int)hipErrorInvalidValue;
  double* ws = static_cast<double*>(workspace);
  const bool vec = (N & 3) == 0;
  hipError_t e;
  if (kl) e = vec ? launch_rows<true, true>(P, Y, N, ws, stream) : launch_rows<true, false>(P, Y, N, ws, stream);
  else e = vec ? launch_rows<false, true>(P, Y, N, ws, stream) : launch_rows<false, false>(P, Y, N, ws, stream);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((N + NT - 1) / NT));
  if (kl) hipLaunchKernelGGL(tsne_gradient_fold_kernel<true>, grid, dim3(NT), 0, stream, ws, N, exaggeration, grad, kl);
  else hipLaunchKernelGGL(tsne_gradient_fold_kernel<false>, grid, dim3(NT), 0, stream, ws, N, exaggeration, grad, kl);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_tsne_update(const float* grad, float* Y, float* U, float* G, int N, float momentum, float lr,
                                hipStream_t stream) {
  if (!grad || !Y || !U || !G || !n_ok(N)) return (int)hipErrorInvalidValue;
  if (!(momentum >= 0.f && momentum < 1.f) || !(lr > 0.f) || lr == INFINITY) return (int)hipErrorInvalidValue;
  if (((uintptr_t)grad & 3) || ((uintptr_t)Y & 3) || ((uintptr_t)U & 3) || ((uintptr_t)G & 3)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)((2 * N + NT - 1) / NT)), dim3(NT), 0, stream, grad, Y, U, G, 2 * N,
                     momentum, lr);
  MULAN_CHECK_LAUNCH();
}
