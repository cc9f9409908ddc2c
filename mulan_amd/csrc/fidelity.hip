// Image fidelity of M pairs of 32 x 32 x 3 uint8 images, channels innermost: pair m is (a[ia ? ia[m] : m], b[ib ? ib[m] : m]).
//   sse        [M, 3]          the sum over the 1024 pixels of (a - b)^2 per channel, in integers (at most 1024 255^2 < 2^31)
//   sse_masked [M, 3]          the same over the pixels whose mask byte is not 0 (mask [M, 32, 32], or one [32, 32] for all)
//   ssim_map   [M, 22, 22, P]  the SSIM of Wang et al. (2004) per window: the normalised 11 x 11 Gaussian of sigma 1.5,
//                              w_k ~ exp(-k^2 / 4.5), applied separably; biased moments; C1 = (0.01 255)^2, C2 = (0.03 255)^2;
//                              only the 22 x 22 windows that lie inside the image, so no boundary rule enters
//   ssim       [M, P]          the mean of the 484 windows
// P = 3 planes (the channels), or 1 with `gray`: the luma 0.2125 R + 0.7154 G + 0.0721 B in fp32, not rounded (the
// constants of spectrum.hip).  sse stays per channel with gray.
//
// Numerics.  sigma^2 = E[x^2] - mu^2 cancels, so the five filtered maps (x, y, x^2, y^2, x y) are taken of x - 128 and
// y - 128 (for uint8 planes the squares and the product are then exact in fp32, at most 2^14), and 128 is put back into mu
// afterwards; the variances do not depend on the shift.  Every filter sum is one fmaf chain in tap order 0..10 that
// starts from the rounded product of tap 0; tests/fidelity_oracle.py restates the same chains in numpy.
//
// Geometry.  A block of 192 threads takes one pair at a time, grid-striding over M; the next pair's bytes are loaded into
// registers (one 16-byte load per image and thread) before this pair's arithmetic.
//   stage   the 3072 bytes of each image go to LDS as they are, rows padded to 100 bytes (25 dwords: threads that walk
//           down a column hit 32 different banks); the mask to rows of 36 bytes.  gray: the block mixes the two luma
//           tiles, [32][33] floats, less 128.
//   rows    thread (plane p = wave, row y, half h) reads the 21 pixels x = 11 h .. 11 h + 20 of its row of a and b, adds
//           the squared differences of its 16 pixels (x < 16 for h = 0, x >= 16 for h = 1) and filters the five maps
//           horizontally for the 11 window columns j = 11 h .. 11 h + 10: H[p][map][y][j], row stride 23 floats.
//           The integer sums are folded over the wave by shuffles (exact in any order).
//   columns thread (p, half h2, column j < 22; one half-wave per (p, h2)) reads H's rows 11 h2 .. 11 h2 + 20 of its column,
//           filters vertically for the windows i = 11 h2 .. 11 h2 + 10, forms their SSIM and adds the 11 values in i order
//   mean    thread p adds the 44 partial sums of plane p in (h2, j) order and divides by 484
//   map     the 484 P values go through LDS (over H) and leave in 16-byte stores
// One fixed order per sum and no atomics: the same arguments give the same bits on every run, and an output does not
// depend on which other outputs are asked for.  A pair whose index lies outside [0, Na) or [0, Nb) is not read: its
// sse and sse_masked are -1, its ssim and ssim_map NaN.
//
// Cost.  2 x 605 fmaf per thread for the filters, 0.2 M per pair beside its 6 KB: 50 000 pairs are 2 10^10 flops, 0.13 ms
// of the fp32 vector peak, beside 0.05 ms to read their 300 MB.  LDS is 51 KB per block; the registers (two waves per SIMD) admit two blocks per CU.  DESIGN.md
// section 3.13 has the measurement (0.71 ms).
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int S = 32;                    // image side
constexpr int W = 22;                    // windows per side
constexpr int TAPS = 11;
constexpr int SPAN = 21;                 // pixels under 11 neighbouring windows
constexpr int NT = 192;
constexpr int IMG = S * S * 3;
constexpr int ROW_B = 100;               // bytes per image row in LDS
constexpr int MROW_B = 36;               // bytes per mask row in LDS
constexpr int HS = 23;                   // floats per row of a filtered map
constexpr int HMAP = S * HS;
constexpr int HPLANE = 5 * HMAP;
constexpr int LS = S + 1;                // floats per row of a luma tile
constexpr int MAX_BLOCKS = 512;          // two blocks per CU of the MI355X (what the registers admit): a constant of the
                                         // library, not of the device
constexpr float GRAY_R = 0.2125f, GRAY_G = 0.7154f, GRAY_B = 0.0721f;
constexpr float CENTRE = 128.f;
constexpr float C1 = 6.5025f, C2 = 58.5225f;

// e^-x for 0 <= x < 6 as 1 / (the Taylor series of e^x): all terms positive, below 1e-20 after 60
constexpr double exp_neg(double x) {
  double term = 1.0, sum = 1.0;
  for (int i = 1; i <= 60; ++i) {
    term *= x / i;
    sum += term;
  }
  return 1.0 / sum;
}
struct Taps {
  float w[TAPS];
};
constexpr Taps make_taps() {
  double e[TAPS] = {}, s = 0.0;
  for (int k = 0; k < TAPS; ++k) {
    const double d = k - 5;
    e[k] = exp_neg(d * d / 4.5);
    s += e[k];
  }
  Taps t{};
  for (int k = 0; k < TAPS; ++k) t.w[k] = (float)(e[k] / s);
  return t;
}
__constant__ Taps kTaps = make_taps();   // read through the scalar cache into SGPRs, once per block

struct FidArgs {
  const unsigned char* a;
  const unsigned char* b;
  int Na, Nb;
  const int* ia;
  const int* ib;
  int M;
  const unsigned char* mask;
  int mask_per_pair;
  int* sse;
  int* sse_masked;
  float* ssim;
  float* ssim_map;
};

constexpr int MASK_PER_THREAD = (S * S + NT - 1) / NT;

// one pair's bytes in registers; `ok` is the same in every thread of the block
struct Fetch {
  i32x4 va, vb;
  unsigned char vm[MASK_PER_THREAD];
  bool ok;
  __device__ __forceinline__ void load(const FidArgs& p, int m, int tid) {
    const int i = p.ia ? p.ia[m] : m, j = p.ib ? p.ib[m] : m;
    ok = (unsigned)i < (unsigned)p.Na && (unsigned)j < (unsigned)p.Nb;
    if (!ok) return;
    va = *reinterpret_cast<const i32x4*>(p.a + (size_t)i * IMG + tid * 16);
    vb = *reinterpret_cast<const i32x4*>(p.b + (size_t)j * IMG + tid * 16);
    if (p.mask) {
      const unsigned char* mk = p.mask + (p.mask_per_pair ? (size_t)m * (S * S) : 0);
#pragma unroll
      for (int q = 0; q < MASK_PER_THREAD; ++q) {
        const int f = q * NT + tid;
        vm[q] = f < S * S ? mk[f] : 0;
      }
    }
  }
};

// Pixel k of the 21 under 11 neighbouring windows enters the sums out[j] = sum_t w[t] v[j + t] of the windows j = k - t it
// lies under.  Called for k = 0..20 in order, every out[j] is the rounded product of tap 0, then fmaf in tap order.
__device__ __forceinline__ void tap_in(float (&out)[TAPS], int k, float v) {
#pragma unroll
  for (int j = 0; j < TAPS; ++j) {
    const int tap = k - j;
    if (tap == 0) out[j] = kTaps.w[0] * v;
    else if (0 < tap && tap < TAPS) out[j] = fmaf(kTaps.w[tap], v, out[j]);
  }
}

// the SSIM of one window from the filtered maps of the centred planes
__device__ __forceinline__ float ssim_of(float mx, float my, float exx, float eyy, float exy) {
  const float sxx = fmaf(-mx, mx, exx), syy = fmaf(-my, my, eyy), sxy = fmaf(-mx, my, exy);
  const float ux = mx + CENTRE, uy = my + CENTRE;
  const float n1 = fmaf(2.f * ux, uy, C1), n2 = fmaf(2.f, sxy, C2);
  const float d1 = fmaf(ux, ux, fmaf(uy, uy, C1)), d2 = (sxx + syy) + C2;
  return (n1 * n2) / (d1 * d2);
}

template <bool GRAY>
__global__ __launch_bounds__(NT, 2) void fidelity_kernel(FidArgs p) {
  constexpr int P = GRAY ? 1 : 3;
  __shared__ __attribute__((aligned(16))) unsigned char sImg[2][S * ROW_B];
  __shared__ __attribute__((aligned(16))) unsigned char sMask[S * MROW_B];
  __shared__ __attribute__((aligned(16))) float sH[P * HPLANE];
  __shared__ float sLuma[GRAY ? 2 * S * LS : 1];
  __shared__ float sPart[P * 2 * W];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool want_ssim = p.ssim || p.ssim_map;
  const float nan = __int_as_float(0x7fc00000);

  Fetch cur;
  cur.ok = false;
  int m = blockIdx.x;
  if (m < p.M) cur.load(p, m, tid);

  for (; m < p.M; m += gridDim.x) {
    const bool ok = cur.ok;
    if (ok) {                                                   // stage
      const int dst = (tid / 6) * ROW_B + (tid % 6) * 16;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        *reinterpret_cast<int*>(sImg[0] + dst + 4 * q) = cur.va[q];
        *reinterpret_cast<int*>(sImg[1] + dst + 4 * q) = cur.vb[q];
      }
      if (p.mask) {
#pragma unroll
        for (int q = 0; q < MASK_PER_THREAD; ++q) {
          const int f = q * NT + tid;
          if (f < S * S) sMask[(f >> 5) * MROW_B + (f & 31)] = cur.vm[q];
        }
      }
    }
    if (m + (int)gridDim.x < p.M) cur.load(p, m + gridDim.x, tid);
    if (!ok) {                                                  // an index out of range: nothing of the pair is read
      if (tid < 3) {
        if (p.sse) p.sse[(size_t)m * 3 + tid] = -1;
        if (p.sse_masked) p.sse_masked[(size_t)m * 3 + tid] = -1;
      }
      if (tid < P && p.ssim) p.ssim[(size_t)m * P + tid] = nan;
      if (p.ssim_map)
        for (int i = tid; i < W * W * P; i += NT) p.ssim_map[(size_t)m * (W * W * P) + i] = nan;
      continue;
    }
    __syncthreads();
    if constexpr (GRAY) {
      if (want_ssim) {
        for (int i = tid; i < 2 * S * S; i += NT) {
          const int img = i >> 10, row = (i >> 5) & 31, col = i & 31;
          const unsigned char* px = sImg[img] + row * ROW_B + 3 * col;
          const float luma = fmaf(GRAY_B, (float)px[2], fmaf(GRAY_G, (float)px[1], GRAY_R * (float)px[0]));
          sLuma[img * (S * LS) + row * LS + col] = luma - CENTRE;
        }
      }
      __syncthreads();
    }

    {                                                           // rows
      const int y = lane & 31, h = lane >> 5, x0 = TAPS * h;
      const unsigned char* ra = sImg[0] + y * ROW_B + 3 * x0 + wave;
      const unsigned char* rb = sImg[1] + y * ROW_B + 3 * x0 + wave;
      const bool filter = want_ssim && wave < P;
      if (p.sse || p.sse_masked) {
        int sse = 0, ssem = 0;
#pragma unroll
        for (int k = 0; k < SPAN; ++k) {
          const bool mine = h ? k >= 5 : k < 16;
          const int d = (int)ra[3 * k] - (int)rb[3 * k], sq = mine ? d * d : 0;
          sse += sq;
          if (p.mask) ssem += sMask[y * MROW_B + x0 + k] ? sq : 0;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          sse += __shfl_xor(sse, off);
          ssem += __shfl_xor(ssem, off);
        }
        if (lane == 0) {
          if (p.sse) p.sse[(size_t)m * 3 + wave] = sse;
          if (p.sse_masked) p.sse_masked[(size_t)m * 3 + wave] = ssem;
        }
      }
      float o[5][TAPS];
      if (filter) {
#pragma unroll
        for (int k = 0; k < SPAN; ++k) {
          float fa, fb;
          if constexpr (GRAY) {
            fa = sLuma[y * LS + x0 + k];
            fb = sLuma[S * LS + y * LS + x0 + k];
          } else {
            fa = (float)((int)ra[3 * k] - 128);
            fb = (float)((int)rb[3 * k] - 128);
          }
          tap_in(o[0], k, fa);
          tap_in(o[1], k, fb);
          tap_in(o[2], k, fa * fa);
          tap_in(o[3], k, fb * fb);
          tap_in(o[4], k, fa * fb);
        }
      }
      if (filter) {
        float* hrow = sH + wave * HPLANE + y * HS + x0;
#pragma unroll
        for (int map = 0; map < 5; ++map)
#pragma unroll
          for (int j = 0; j < TAPS; ++j) hrow[map * HMAP + j] = o[map][j];
      }
    }
    __syncthreads();

    if (want_ssim) {                                            // columns
      const int half = tid >> 5, j = tid & 31, pp = half >> 1, h2 = half & 1;
      const bool active = j < W && pp < P;
      float sv[TAPS];
      if (active) {
        const float* col = sH + pp * HPLANE + (TAPS * h2) * HS + j;
        float o[5][TAPS];
#pragma unroll
        for (int k = 0; k < SPAN; ++k)
#pragma unroll
          for (int map = 0; map < 5; ++map) tap_in(o[map], k, col[map * HMAP + k * HS]);
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < TAPS; ++i) {
          sv[i] = ssim_of(o[0][i], o[1][i], o[2][i], o[3][i], o[4][i]);
          acc = i == 0 ? sv[0] : acc + sv[i];
        }
        sPart[pp * (2 * W) + h2 * W + j] = acc;
      }
      if (p.ssim_map) {
        __syncthreads();                                        // every thread has read H
        if (active) {
#pragma unroll
          for (int i = 0; i < TAPS; ++i) sH[((TAPS * h2 + i) * W + j) * P + pp] = sv[i];
        }
        __syncthreads();
        float* out = p.ssim_map + (size_t)m * (W * W * P);
        for (int i = tid; i < W * W * P / 4; i += NT)
          *reinterpret_cast<f32x4*>(out + 4 * i) = *reinterpret_cast<const f32x4*>(sH + 4 * i);
      }
      __syncthreads();
      if (p.ssim && tid < P) {                                  // mean
        float s = sPart[tid * (2 * W)];
        for (int i = 1; i < 2 * W; ++i) s += sPart[tid * (2 * W) + i];
        p.ssim[(size_t)m * P + tid] = s / (float)(W * W);
      }
    }
  }
}

}  // namespace

MULAN_API int mulan_image_fidelity(const unsigned char* a, int Na, const unsigned char* b, int Nb, const int* ia,
                                   const int* ib, int M, int gray, const unsigned char* mask, int mask_per_pair,
                                   int* sse, int* sse_masked, float* ssim, float* ssim_map, hipStream_t stream) {
  if (M < 1 || Na < 1 || Nb < 1 || !a || !b || (!ia && M > Na) || (!ib && M > Nb)) return (int)hipErrorInvalidValue;
  if (!sse && !sse_masked && !ssim && !ssim_map) return (int)hipErrorInvalidValue;
  if ((sse_masked != nullptr) != (mask != nullptr)) return (int)hipErrorInvalidValue;
  if ((gray != 0 && gray != 1) || (mask_per_pair != 0 && mask_per_pair != 1)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)ssim_map & 15) || ((uintptr_t)ia & 3) ||
      ((uintptr_t)ib & 3) || ((uintptr_t)sse & 3) || ((uintptr_t)sse_masked & 3) || ((uintptr_t)ssim & 3))
    return (int)hipErrorInvalidValue;
  FidArgs p{a, b, Na, Nb, ia, ib, M, mask, mask_per_pair, sse, sse_masked, ssim, ssim_map};
  const dim3 grid((unsigned)(M < MAX_BLOCKS ? M : MAX_BLOCKS)), block(NT);
  if (gray) hipLaunchKernelGGL(fidelity_kernel<true>, grid, block, 0, stream, p);
  else hipLaunchKernelGGL(fidelity_kernel<false>, grid, block, 0, stream, p);
  MULAN_CHECK_LAUNCH();
}
