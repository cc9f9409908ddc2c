// Spatial spectra of 32 x 32 x 3 images: per image and plane the orthonormal 2-D DCT-II Y = D X D^T on the fp32 matrix
// cores, and what is read off it without the coefficients having to leave the chip:
//   coef   [N, 32, 32, P]  Y[u][v] (u the vertical frequency, v the horizontal one)
//   radial [N, 45, P]      the sum of Y^2 over the coefficients of radial bin r = floor(sqrt(u^2 + v^2) + 1/2), in integers
//                          the r with r^2 - r < u^2 + v^2 <= r^2 + r (bin 0 is the DC term alone, the last bin is 44)
//   sum1, sum2 [32, 32, P] fp64 sums of Y and Y^2 over the N images (added to what is there with `accumulate`)
// P = 3 planes (the channels), or 1 with `gray` (0.2125 R + 0.7154 G + 0.0721 B, the weights of skimage's rgb2gray and so
// of the reference's notebook_utils.dct2).  The input is uint8, read as scale v + offset, or fp32 taken as is; channels
// innermost.  D[u][y] = c_u cos(pi (2 y + 1) u / 64), c_0 = sqrt(1 / 32), c_u = 1 / 4: scipy.fft.dctn(norm='ortho').
//
// Tables.  D and the bins' member lists are compile-time constants (SpecTables, built by constexpr code below): the 128
// values cos(pi k / 64) from a Taylor series in double, good to 1e-16 and then rounded to fp32 (c_u = 1/4 is exact), and
// per bin the LDS offsets of its members in (u, v) order, padded with the offset of a cell that holds 0.
//
// Geometry.  A block of 192 threads takes one image at a time, grid-striding over N; wave p owns plane p.
//   load      uint8: the image's 3072 bytes are one 16-byte load per thread; fp32: four.  The next image's loads are
//             issued before this image's arithmetic.
//   scatter   every thread converts its values and writes them to the planes' tiles in LDS, [32][33] floats each
//             (gray: then the three tiles are mixed into tile 0, each pixel by one thread)
//   T = D X   16 v_mfma_f32_32x32x2_f32: lane l supplies D[l & 31][k] and X[k][l & 31], k = 2 kk + (l >> 5); T goes back
//             to the wave's tile, accumulator register e to row mfma32_row(e, l), column l & 31
//   Y = T D^T 16 more: lane l supplies T[l & 31][k] and D[l & 31][k]
//   sums      lane l keeps sum1 and sum2 of its 16 coefficients in fp64 registers across the grid stride; at the end they
//             go to workspace [blocks][2][32][32][P]
//   radial    Y goes to the tile; lane r < 45 adds the squares of bin r's members in table order (every lane the same
//             number of loads: the padding reads the zero cell)
//   coef      the block writes the image's coefficients from the tiles, 16 bytes per thread and store
// A second launch folds the workspace: 16 threads per output element each add every 16th block's partial in block order,
// thread 0 of them adds the 16 results in order onto the previous contents (accumulate) or onto 0.  The number of blocks
// is min(N, 1024) (four blocks per CU of the MI355X: what 137 - 151 VGPRs admit) unless the caller names one: a constant of the library, not of the device.  One fixed order per sum, no
// atomics, the same bits on every run; coef and radial do not depend on the number of blocks at all.
//
// Cost.  2 x 16 MFMAs of 64 cycles per plane: 50 000 images are 2 10^10 flops, 0.13 ms of the fp32 matrix peak, beside
// 0.04 ms to read their 150 MB; DESIGN.md section 3.11 has the measurement.
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int S = 32;                    // image side
constexpr int TS = S + 1;                // tile row stride in floats
constexpr int ZERO_CELL = S * TS;        // offset of the cell that holds 0 (behind the tile's last row)
constexpr int TILE = ZERO_CELL + 8;      // floats per tile
constexpr int NB = 45;                   // radial bins
constexpr int NT = 192;
constexpr int IMG = S * S * 3;
constexpr int MAX_BLOCKS = 1024;         // blocks the library launches at most when it chooses
constexpr int LIMIT_BLOCKS = 4096;       // ... and the most a caller may ask for
constexpr int FOLD_WAYS = 16;
constexpr float GRAY_R = 0.2125f, GRAY_G = 0.7154f, GRAY_B = 0.0721f;

constexpr int bin_of(int s) {            // the r with r^2 - r < s <= r^2 + r; 0 for s = 0
  int r = 0;
  while (r * r + r < s) ++r;
  return r;
}
constexpr int max_bin_size() {
  int count[NB] = {};
  int m = 0;
  for (int u = 0; u < S; ++u)
    for (int v = 0; v < S; ++v) {
      const int n = ++count[bin_of(u * u + v * v)];
      m = n > m ? n : m;
    }
  return m;
}
constexpr int MAXB = (max_bin_size() + 7) / 8 * 8;     // members per bin, padded to whole 16-byte reads
static_assert(bin_of(2 * (S - 1) * (S - 1)) == NB - 1, "the last bin");

// cos(pi k / 64), k in 0..127, folded to [0, pi / 2] and summed as a Taylor series (terms below 1e-20 after 14)
constexpr double cos_pi_64(int k) {
  k %= 128;
  if (k > 64) k = 128 - k;
  double sign = 1.0;
  if (k > 32) {
    k = 64 - k;
    sign = -1.0;
  }
  if (k == 32) return 0.0;
  const double x = 3.14159265358979323846264338327950288 * k / 64.0, x2 = x * x;
  double term = 1.0, sum = 1.0;
  for (int i = 1; i <= 16; ++i) {
    term *= -x2 / ((2 * i - 1) * (2 * i));
    sum += term;
  }
  return sign * sum;
}

struct SpecTables {
  float d[S * S];                        // D[u][y]
  unsigned short member[NB * MAXB];      // tile offsets u * TS + v of bin r's members in (u, v) order, then ZERO_CELL
};
constexpr SpecTables make_tables() {
  SpecTables t{};
  for (int u = 0; u < S; ++u)
    for (int y = 0; y < S; ++y)
      t.d[u * S + y] = u == 0 ? (float)0.17677669529663688110 : (float)(0.25 * cos_pi_64((2 * y + 1) * u));
  int count[NB] = {};
  for (int i = 0; i < NB * MAXB; ++i) t.member[i] = (unsigned short)ZERO_CELL;
  for (int u = 0; u < S; ++u)
    for (int v = 0; v < S; ++v) {
      const int r = bin_of(u * u + v * v);
      t.member[r * MAXB + count[r]++] = (unsigned short)(u * TS + v);
    }
  return t;
}
__constant__ SpecTables kTab = make_tables();

struct SpecArgs {
  const void* x;
  float scale, offset;
  int N, P;
  float* coef;
  float* radial;
  double* ws;                            // [blocks][2][S][S][P] or null
};

template <bool U8> struct Fetch;
template <> struct Fetch<true> {
  i32x4 v;
  __device__ __forceinline__ void load(const void* x, int n, int tid) {
    v = *reinterpret_cast<const i32x4*>(static_cast<const unsigned char*>(x) + (size_t)n * IMG + tid * 16);
  }
};
template <> struct Fetch<false> {
  f32x4 v[4];
  __device__ __forceinline__ void load(const void* x, int n, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = ld_stream4(static_cast<const float*>(x) + (size_t)n * IMG + (size_t)(i * NT + tid) * 4);
  }
};

// flat sub-pixel f of an image -> its cell in the three tiles
__device__ __forceinline__ int cell_of(int f) {
  const int pix = f / 3, ch = f - 3 * pix;
  return ch * TILE + (pix >> 5) * TS + (pix & 31);
}

template <bool U8, bool GRAY>
__global__ __launch_bounds__(NT) void spectrum_kernel(SpecArgs p) {
  __shared__ float sD[S * TS];
  __shared__ float tiles[3 * TILE];
  __shared__ __attribute__((aligned(16))) unsigned short sMember[NB * MAXB];
  constexpr int P = GRAY ? 1 : 3;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;

  for (int i = tid; i < S * S; i += NT) sD[(i >> 5) * TS + (i & 31)] = kTab.d[i];
  for (int i = tid; i < NB * MAXB; i += NT) sMember[i] = kTab.member[i];
  if (tid < 3) tiles[tid * TILE + ZERO_CELL] = 0.f;

  double s1[16], s2[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) s1[e] = s2[e] = 0.0;

  Fetch<U8> cur;
  int n = blockIdx.x;
  if (n < p.N) cur.load(p.x, n, tid);
  __syncthreads();
  float* tile = tiles + wave * TILE;
  const bool active = wave < P;

  for (; n < p.N; n += gridDim.x) {
    // scatter
    if constexpr (U8) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned b = ((unsigned)cur.v[j >> 2] >> (8 * (j & 3))) & 0xffu;
        tiles[cell_of(tid * 16 + j)] = fmaf(p.scale, (float)b, p.offset);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) tiles[cell_of((i * NT + tid) * 4 + j)] = cur.v[i][j];
    }
    if (n + (int)gridDim.x < p.N) cur.load(p.x, n + gridDim.x, tid);
    __syncthreads();
    if constexpr (GRAY) {
      for (int i = tid; i < S * S; i += NT) {
        const int c = (i >> 5) * TS + (i & 31);
        tiles[c] = fmaf(GRAY_B, tiles[2 * TILE + c], fmaf(GRAY_G, tiles[TILE + c], GRAY_R * tiles[c]));
      }
      __syncthreads();
    }

    f32x16 acc;
    if (active) {                                             // T = D X
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const int k = 2 * kk + half;
        acc = mfma32(sD[col * TS + k], tile[k * TS + col], acc);
      }
    }
    __syncthreads();                                          // every lane has read X
    if (active) {
#pragma unroll
      for (int e = 0; e < 16; ++e) tile[mfma32_row(e, lane) * TS + col] = acc[e];
    }
    __syncthreads();
    if (active) {                                             // Y = T D^T
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const int k = 2 * kk + half;
        acc = mfma32(tile[col * TS + k], sD[col * TS + k], acc);
      }
      if (p.ws) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const double y = (double)acc[e];
          s1[e] += y;
          s2[e] = fma(y, y, s2[e]);
        }
      }
    }
    __syncthreads();                                          // every lane has read T
    if (active && (p.radial || p.coef)) {
#pragma unroll
      for (int e = 0; e < 16; ++e) tile[mfma32_row(e, lane) * TS + col] = acc[e];
    }
    __syncthreads();
    if (active && p.radial && lane < NB) {
      const i32x4* mine = reinterpret_cast<const i32x4*>(sMember + lane * MAXB);
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < MAXB / 8; ++i) {
        const i32x4 m = mine[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float y = tile[((unsigned)m[j >> 1] >> (16 * (j & 1))) & 0xffffu];
          sum = fmaf(y, y, sum);
        }
      }
      p.radial[((size_t)n * NB + lane) * P + wave] = sum;
    }
    if (p.coef) {
      float* out = p.coef + (size_t)n * (S * S * P);
      for (int i = tid; i < S * S * P / 4; i += NT) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int f = 4 * i + j;
          o[j] = GRAY ? tiles[(f >> 5) * TS + (f & 31)] : tiles[cell_of(f)];
        }
        *reinterpret_cast<f32x4*>(out + 4 * i) = o;
      }
    }
    __syncthreads();                                          // the tiles are free for the next image
  }

  if (p.ws && active) {
    double* w = p.ws + (size_t)blockIdx.x * (2 * S * S * P);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = (mfma32_row(e, lane) * S + col) * P + wave;
      w[i] = s1[e];
      w[S * S * P + i] = s2[e];
    }
  }
}

// Output element i of [2][S * S * P] (sum1, then sum2): FOLD_WAYS threads add the blocks b = way, way + FOLD_WAYS, ...
// in order, way 0 adds the partial sums in order.
__global__ __launch_bounds__(256) void spectrum_fold_kernel(const double* __restrict__ ws, int blocks, int P,
                                                            double* __restrict__ sum1, double* __restrict__ sum2,
                                                            int accumulate) {
  __shared__ double part[FOLD_WAYS][16];
  const int j = threadIdx.x & 15, way = threadIdx.x >> 4;
  const int per = S * S * P;
  const int i = blockIdx.x * 16 + j;                          // 2 per is a multiple of 16
  double s = 0.0;
#pragma unroll 8
  for (int b = way; b < blocks; b += FOLD_WAYS) s += ws[(size_t)b * (2 * per) + i];
  part[way][j] = s;
  __syncthreads();
  if (way == 0) {
    double* out = i < per ? sum1 : sum2;
    const int o = i < per ? i : i - per;
    if (out) {
      double t = accumulate ? out[o] : 0.0;
#pragma unroll
      for (int k = 0; k < FOLD_WAYS; ++k) t += part[k][j];
      out[o] = t;
    }
  }
}

// blocks = 0: the library's choice
int blocks_for(int N, int blocks) {
  const int b = blocks ? blocks : MAX_BLOCKS;
  return N < b ? N : b;
}

}  // namespace

MULAN_API size_t mulan_spectrum_workspace(int N, int gray, int blocks) {
  if (N < 1 || blocks < 0 || LIMIT_BLOCKS < blocks) return 0;
  return (size_t)blocks_for(N, blocks) * 2 * S * S * (gray ? 1 : 3) * sizeof(double);
}

MULAN_API int mulan_spectrum(const void* x, int dtype, float scale, float offset, int N, int gray, float* coef,
                             float* radial, double* sum1, double* sum2, int accumulate, int blocks,
                             void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!x || N < 1 || (dtype != 0 && dtype != 1) || (gray != 0 && gray != 1) || (accumulate != 0 && accumulate != 1) ||
      blocks < 0 || LIMIT_BLOCKS < blocks)
    return (int)hipErrorInvalidValue;
  const bool sums = sum1 || sum2;
  if ((!coef && !radial && !sums) || (accumulate && !sums)) return (int)hipErrorInvalidValue;
  if (sums && (!workspace || workspace_bytes < mulan_spectrum_workspace(N, gray, blocks))) return (int)hipErrorInvalidValue;
  if (((uintptr_t)x & 15) || ((uintptr_t)coef & 15) || ((uintptr_t)radial & 3) || ((uintptr_t)sum1 & 7) ||
      ((uintptr_t)sum2 & 7) || (sums && ((uintptr_t)workspace & 7)))
    return (int)hipErrorInvalidValue;
  const int P = gray ? 1 : 3, nblocks = blocks_for(N, blocks);
  SpecArgs a{x, scale, offset, N, P, coef, radial, sums ? static_cast<double*>(workspace) : nullptr};
  const dim3 grid((unsigned)nblocks), block(NT);
  if (dtype == 0) {
    if (gray) hipLaunchKernelGGL((spectrum_kernel<true, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((spectrum_kernel<true, false>), grid, block, 0, stream, a);
  } else {
    if (gray) hipLaunchKernelGGL((spectrum_kernel<false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((spectrum_kernel<false, false>), grid, block, 0, stream, a);
  }
  if (sums)
    hipLaunchKernelGGL(spectrum_fold_kernel, dim3((unsigned)(2 * S * S * P / 16)), dim3(256), 0, stream, a.ws, nblocks, P,
                       sum1, sum2, accumulate);
  MULAN_CHECK_LAUNCH();
}
