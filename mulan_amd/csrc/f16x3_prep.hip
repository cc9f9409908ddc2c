// Operand preparation for the f16x3 kernels (see conv3x3_f16x3.hip for the arithmetic): the per-row maxima that give the
// power-of-two operand scales, and the scaled, split and tiled weights of the 3x3 convolutions -- per tensor, or for all
// parameter leaves of a step at once.
#include "common.h"
#include "f16x3_common.h"

namespace {

using namespace f16x3;

// out[r][c] = fp32 bits of the maximum |x| over part c of row r (16 parts per row; non-negative floats order like
// their bit patterns, so integer max works); no atomics, no zero-fill pass
__global__ __launch_bounds__(256) void absmax_rows_kernel(const float* __restrict__ x, unsigned* __restrict__ out,
                                                          size_t row_len4) {
  __shared__ unsigned red[4];
  const f32x4* row = reinterpret_cast<const f32x4*>(x) + (size_t)blockIdx.x * row_len4;
  unsigned m = 0;
  const size_t stride = (size_t)kMaxParts * 256;
  size_t i = (size_t)blockIdx.y * 256 + threadIdx.x;
  for (; i + 3 * stride < row_len4; i += 4 * stride) {
    const f32x4 a = row[i], b = row[i + stride], c = row[i + 2 * stride], d = row[i + 3 * stride];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      m = max(m, __float_as_uint(a[e]) & 0x7fffffffu);
      m = max(m, __float_as_uint(b[e]) & 0x7fffffffu);
      m = max(m, __float_as_uint(c[e]) & 0x7fffffffu);
      m = max(m, __float_as_uint(d[e]) & 0x7fffffffu);
    }
  }
  for (; i < row_len4; i += stride) {
    const f32x4 a = row[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) m = max(m, __float_as_uint(a[e]) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[(size_t)blockIdx.x * kMaxParts + blockIdx.y] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// c = a + b with the maxima of c as above: the sum autograd would form for a tensor with two consumers (the U-Net skip
// connections) and the maxima pass of the convolution that takes c as its dy, in one pass over the data
// colpart (optional, [rows][kMaxParts][ncols]): the column sums of c's rows seen as [row_len / ncols, ncols] matrices,
// one partial per block -- the bias gradient of the convolution that receives c as its output gradient is the column
// sum of these rows * 16 small vectors instead of a second pass over c.  (ncols / 4) divides 256: a thread's float4s
// all belong to one column quad.
__global__ __launch_bounds__(256) void add_absmax_rows_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              float* __restrict__ c, unsigned* __restrict__ out,
                                                              size_t row_len4, float* __restrict__ colpart, int ncols) {
  __shared__ unsigned red[4];
  __shared__ f32x4 cred[256];
  f32x4 cs = {0.f, 0.f, 0.f, 0.f};
  const size_t base = (size_t)blockIdx.x * row_len4;
  const f32x4* ra = reinterpret_cast<const f32x4*>(a) + base;
  const f32x4* rb = reinterpret_cast<const f32x4*>(b) + base;
  f32x4* rc = reinterpret_cast<f32x4*>(c) + base;
  unsigned m = 0;
  const size_t stride = (size_t)kMaxParts * 256;
  for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < row_len4; i += stride) {
    const f32x4 v = ra[i] + rb[i];
    rc[i] = v;
    cs += v;
#pragma unroll
    for (int e = 0; e < 4; ++e) m = max(m, __float_as_uint(v[e]) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  if (colpart) cred[threadIdx.x] = cs;
  __syncthreads();
  if (threadIdx.x == 0) out[(size_t)blockIdx.x * kMaxParts + blockIdx.y] = max(max(red[0], red[1]), max(red[2], red[3]));
  if (colpart) {     // threads t, t + q, t + 2 q, ... (q = ncols / 4 column quads) hold the same columns: fixed order
    const int q = ncols >> 2;
    if ((int)threadIdx.x < q) {
      f32x4 t = cred[threadIdx.x];
      for (int j = threadIdx.x + q; j < 256; j += q) t += cred[j];
      reinterpret_cast<f32x4*>(colpart)[((size_t)blockIdx.x * kMaxParts + blockIdx.y) * q + threadIdx.x] = t;
    }
  }
}

// wp[t][cc][o][plane][k] = split2( s_w * Wl[t][cc*16 + k][o] ),  Wl = w (flip = 0) or the tap-flipped,
// channel-transposed weights of the input-gradient convolution (flip = 1: Wl[t][k][o] = w[8-t][o][k]).
__global__ void conv3x3_pack_f16x3_kernel(const float* __restrict__ w, _Float16* __restrict__ wp,
                                          const unsigned* __restrict__ wmax, int C, int N, int flip) {
  const int Kin = flip ? N : C, Nout = flip ? C : N;
  const size_t total = (size_t)9 * Kin * Nout;
  float sw, inv_w;
  scale_of(row_max16(wmax, 0), sw, inv_w);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % 16);
    size_t r = i / 16;
    const int o = (int)(r % Nout); r /= Nout;
    const int cc = (int)(r % (Kin / 16));
    const int t = (int)(r / (Kin / 16));
    const int kin = cc * 16 + k;
    const float v = flip ? w[((size_t)(8 - t) * C + o) * N + kin] : w[((size_t)t * C + kin) * N + o];
    _Float16 h, l;
    split2(v * sw, h, l);
    _Float16* dst = wp + (((size_t)(t * (Kin / 16) + cc) * Nout + o) * 2) * 16 + k;
    dst[0] = h; dst[16] = l;
  }
}

// ---- once-per-step weight preparation for every eligible parameter leaf at a time (two launches instead of two
// per layer and direction): maxima of all leaves, then both packed operands (forward and gradient) of all leaves.
// Leaf record (8 x int64): [0] element offset in the flat parameter buffer, [1] kind (0: 3x3 conv [3,3,C,N],
// 1: dense [C,N]), [2] C, [3] N, [4] byte offset of the forward operand in the packed buffer or -1, [5] of the
// gradient operand (tap-flipped / transposed) or -1, [6] number of elements.
__global__ __launch_bounds__(256) void param_maxima_kernel(const float* __restrict__ flat, const long long* __restrict__ leaves,
                                                           unsigned* __restrict__ out) {
  __shared__ unsigned red[4];
  const long long* L = leaves + (size_t)blockIdx.x * 8;
  const f32x4* row = reinterpret_cast<const f32x4*>(flat + L[0]);
  const size_t len4 = (size_t)L[6] / 4;
  unsigned m = 0;
  for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < len4; i += (size_t)kMaxParts * 256) {
    const f32x4 a = row[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) m = max(m, __float_as_uint(a[e]) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[(size_t)blockIdx.x * kMaxParts + blockIdx.y] = max(max(red[0], red[1]), max(red[2], red[3]));
}

__global__ __launch_bounds__(256) void param_pack_kernel(const float* __restrict__ flat, const long long* __restrict__ leaves,
                                                         const unsigned* __restrict__ maxima, unsigned char* __restrict__ packed) {
  const long long* L = leaves + (size_t)blockIdx.x * 8;
  const int dir = blockIdx.y;                       // 0: forward operand, 1: gradient operand
  const long long dst_off = L[4 + dir];
  if (dst_off < 0) return;
  const float* w = flat + L[0];
  const int kind = (int)L[1], C = (int)L[2], N = (int)L[3];
  _Float16* wp = reinterpret_cast<_Float16*>(packed + dst_off);
  float sw, inv_w;
  scale_of(row_max16(maxima, blockIdx.x), sw, inv_w);
  const int taps = kind == 0 ? 9 : 1;
  const int Kin = dir ? N : C, Nout = dir ? C : N;
  const size_t total = (size_t)taps * Kin * Nout;
  for (size_t i = (size_t)blockIdx.z * 256 + threadIdx.x; i < total; i += (size_t)gridDim.z * 256) {
    const int k = (int)(i % 16);
    size_t r = i / 16;
    const int o = (int)(r % Nout); r /= Nout;
    const int cc = (int)(r % (Kin / 16));
    const int t = (int)(r / (Kin / 16));
    const int kin = cc * 16 + k;
    // forward: Wl[t][kin][o] = w[t][kin][o]; gradient: Wl[t][kin][o] = w[taps-1-t][o][kin]   (w is [taps][C][N])
    const float v = dir ? w[((size_t)(taps - 1 - t) * C + o) * N + kin] : w[((size_t)t * C + kin) * N + o];
    _Float16 h, l;
    split2(v * sw, h, l);
    _Float16* dst = wp + (((size_t)(t * (Kin / 16) + cc) * Nout + o) * 2) * 16 + k;
    dst[0] = h; dst[16] = l;
  }
}

}  // namespace

// out[r][0..15] = fp32 bit patterns of 16 partial maxima of |x[r, 0:row_len]| (row_len % 4 == 0, x 16-byte aligned);
// the maximum of a row's 16 entries is the per-image maximum that feeds the power-of-two operand scales of the f16x3
// kernels.  (The fused GroupNorm kernel writes the same format for its output as a by-product.)
MULAN_API int mulan_absmax_rows(const float* x, unsigned* out, int rows, size_t row_len, hipStream_t stream) {
  if (rows <= 0 || row_len == 0 || row_len % 4 != 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(absmax_rows_kernel, dim3(rows, kMaxParts), dim3(256), 0, stream, x, out, row_len / 4);
  MULAN_CHECK_LAUNCH();
}

// c = a + b (rows x row_len, c may alias a or b) and out = mulan_absmax_rows(c): gradient accumulation of a tensor with
// two consumers fused with the maxima pass of the layer behind it
MULAN_API int mulan_add_absmax_rows(const float* a, const float* b, float* c, unsigned* out, int rows, size_t row_len,
                                    hipStream_t stream) {
  if (rows <= 0 || row_len == 0 || row_len % 4 != 0 || !a || !b || !c || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(add_absmax_rows_kernel, dim3(rows, kMaxParts), dim3(256), 0, stream, a, b, c, out, row_len / 4,
                     static_cast<float*>(nullptr), 0);
  MULAN_CHECK_LAUNCH();
}

// The same with the column sums of c as a by-product: every row is a [row_len / ncols, ncols] matrix (pixels x channels);
// colpart [rows][16][ncols] receives 16 partial column sums per row (the sum of all rows * 16 vectors is the column sum of
// c: the bias gradient of the layer whose output gradient c is, without a second pass over c).  ncols % 4 == 0,
// 256 % (ncols / 4) == 0, row_len % ncols == 0.
MULAN_API int mulan_add_absmax_rows_colsum(const float* a, const float* b, float* c, unsigned* out, float* colpart,
                                           int rows, size_t row_len, int ncols, hipStream_t stream) {
  if (rows <= 0 || row_len == 0 || row_len % 4 != 0 || !a || !b || !c || !out || !colpart || ncols <= 0 || ncols % 4 != 0 ||
      256 % (ncols / 4) != 0 || row_len % ncols != 0)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(add_absmax_rows_kernel, dim3(rows, kMaxParts), dim3(256), 0, stream, a, b, c, out, row_len / 4,
                     colpart, ncols);
  MULAN_CHECK_LAUNCH();
}

MULAN_API size_t mulan_conv3x3_pack_f16x3_bytes(int C, int N) { return (size_t)9 * C * N * 2 * 2; }

// Packs (and scales, splits) the weights for mulan_conv3x3_fwd_f16x3; wmax[16] = mulan_absmax_rows(w, 1 row).
MULAN_API int mulan_conv3x3_pack_f16x3(const float* w, void* wp, const unsigned* wmax, int C, int N, int flip,
                                       hipStream_t stream) {
  const int Kin = flip ? N : C;
  if (Kin % 16 != 0 || C <= 0 || N <= 0 || !wmax) return (int)hipErrorInvalidValue;
  const size_t total = (size_t)9 * C * N;
  const int blocks = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
  hipLaunchKernelGGL(conv3x3_pack_f16x3_kernel, dim3(blocks), dim3(256), 0, stream, w, static_cast<_Float16*>(wp), wmax,
                     C, N, flip);
  MULAN_CHECK_LAUNCH();
}

// Maxima of n parameter leaves in one launch (leaf records: see param_maxima_kernel); out is [n][16].
MULAN_API int mulan_param_maxima(const float* flat, const long long* leaves, int n, unsigned* out, hipStream_t stream) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(param_maxima_kernel, dim3(n, kMaxParts), dim3(256), 0, stream, flat, leaves, out);
  MULAN_CHECK_LAUNCH();
}

// Both packed f16x3 operands (forward: mulan_conv3x3_pack_f16x3 flip = 0 / mulan_linear_pack_f16x3 transpose = 0;
// gradient: flip = 1 / transpose = 1) of n parameter leaves in one launch, into `packed` at the records' offsets.
MULAN_API int mulan_param_pack_f16x3(const float* flat, const long long* leaves, int n, const unsigned* maxima,
                                     void* packed, hipStream_t stream) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(param_pack_kernel, dim3(n, 2, 16), dim3(256), 0, stream, flat, leaves, maxima,
                     static_cast<unsigned char*>(packed));
  MULAN_CHECK_LAUNCH();
}

