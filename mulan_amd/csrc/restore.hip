// Restoration with the few-step samplers (not in the reference): range / null-space projection of the data prediction
// onto a linear measurement (DDNM, Wang et al. 2022) for the operators whose pseudo-inverse is replication.
// A degradation partitions the H x W x C sub-pixels of an image (HWC) into equal groups and A takes each group's mean:
//   sr:f       f x f average pooling per channel     group of (h, w, c) = (h / f, w / f, c)   n_g = f^2     y [B, H/f, W/f, C]
//   gray       channel mean                          (f = 1, gray)        (h, w)              n_g = C       y [B, H, W, 1]
//   sr:f+gray  both                                                       (h / f, w / f)      n_g = C f^2   y [B, H/f, W/f, 1]
// A+ replicates, so A A+ = I and the projection of a prediction x_hat onto {x : A x = y} is, per element i of group g,
//   x_hat'_i = x_hat_i + (y_g - mean_{j in g} x_hat_j).
// It lives in data space, where no schedule appears: x_hat is formed from (z_t, net, gamma_t) by the expressions of
// fast_step_elem (sampler.hip) per element, whatever gammas the members of a group have.
//
// Mapping.  A row band of f image rows is f W C contiguous floats and holds whole groups, G = (W / f) (gray ? 1 : C) of
// them: one block of 256 threads per (image, band).  The block (1) forms x_hat of its band with coalesced loads and
// parks it in LDS, (2) reduces the groups from LDS, (3) adds each element's group correction and stores the band
// coalesced.  z, net and gamma are read once and x_hat' written once, which is all the traffic the operation needs; the
// strided walk over a group's members touches LDS only.  A group is reduced by a team of L = 2^k lanes, L the largest
// power of two <= min(n_g, 64): lane l of the team adds members l, l + L, l + 2L, ... in that order (member m of a group is
// its m-th sub-pixel in row-major order of (row, column, channel)) and the L partial sums meet in a xor-shuffle tree
// inside the team.  So groups of 3 .. 16 take 2 .. 16 lanes each and many groups share a wave, and from n_g = 64 on a
// whole wave serves one group.  The order depends on (f, gray, C) alone -- no atomics, no dependence on the grid -- so
// two runs give the same bits, and mulan_restore_measure, which runs the same reduction on the same LDS image, returns
// the very means the projection subtracts: projecting x onto its own measurement adds (y_g - mean_g) = 0.
// Every lane of a wave runs the same number of rounds (a team past the last group adds zeros), so the shuffles are
// never executed under a partial mask.
// The band in LDS limits f W C to 16384 - G floats (64 KiB with the G corrections behind it); a 32 x 32 x 3 image at
// f = 16 takes 6 KiB.
// `gray` alone (f = 1) has groups of C consecutive floats that no row boundary cuts, so an image row of W C floats
// (96 at 32 x 32 x 3) would leave most of a block idle: the launch then treats 2^k rows as one (H / 2^k rows of 2^k W
// pixels, the same groups in the same order in memory and in y), the largest 2^k that divides H and keeps a band
// within 1024 floats.
#include "common.h"

namespace {

struct RestoreGeom {
  int H, W, C, f, gray;
  int band;        // f W C: the elements of a row band
  int G;           // groups per band
  int n_g;         // members per group
  int L;           // lanes per team
  int Cy;          // channels of y: gray ? 1 : C
};

// sum of group g's members from the band in LDS, complete in every lane of the team (lanes [tid & ~(L-1), +L))
__device__ __forceinline__ float restore_group_sum(const float* band, const RestoreGeom& q, int g, bool live, int lane) {
  const int cg = q.gray ? q.C : 1, run = q.f * cg;
  const int wo = g / q.Cy, c0 = q.gray ? 0 : g - wo * q.Cy;
  float acc = 0.f;
  if (live) {
    for (int m = lane; m < q.n_g; m += q.L) {
      const int dy = m / run, r = m - dy * run;       // r = dx cg + cc: f cg consecutive floats when gray
      const int dx = r / cg, cc = r - dx * cg;
      acc += band[(dy * q.W + wo * q.f + dx) * q.C + c0 + cc];
    }
  }
  for (int o = q.L >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

// group of element e of the band
__device__ __forceinline__ int restore_group_of(const RestoreGeom& q, int e) {
  const int pix = e / q.C, c = e - pix * q.C;
  const int wo = (pix % q.W) / q.f;
  return q.gray ? wo : wo * q.C + c;
}

// x_hat as fast_step_elem (sampler.hip) forms it, bit for bit.  The step kernels round each product on its own: modes 0
// and 1 share sigma_t net there, so the compiler keeps the multiplications apart from the subtraction.  Here the lone
// expression would contract into an fma and x_hat would differ from their x0 output in the last bit, so contraction is
// switched off for this function.
__device__ __forceinline__ float restore_xhat(float zt, float nt, float g_t, int mode) {
#pragma clang fp contract(off)
  const float alpha_t = sqrtf(sigmoid_f(-g_t)), sigma_t = sqrtf(sigmoid_f(g_t));
  float xh = nt;
  if (mode == 0) xh = alpha_t * zt - sigma_t * nt;
  if (mode == 1) xh = (zt - sigma_t * nt) / alpha_t;
  return xh;
}

// PROJECT: band = x_hat(z, net, gamma), out = x_hat + (y - mean); else band = x, y_out = mean
template <bool PROJECT>
__global__ __launch_bounds__(256) void restore_kernel(const float* z, const float* net, const float* __restrict__ gt,
                                                      const float* __restrict__ y, float* out, RestoreGeom q, int mode,
                                                      int g_per_sample) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* band = lds;                 // [q.band]
  float* corr = lds + q.band;        // [q.G]: y_g - mean_g
  const int bands = q.H / q.f;
  const size_t blk = blockIdx.x;
  const size_t b = blk / (size_t)bands;
  const size_t base = blk * (size_t)q.band;          // (b, band) is band number blk of the batch
  const int tid = threadIdx.x;

  for (int e = tid; e < q.band; e += 256) {
    const size_t i = base + e;
    if (PROJECT) {
      const float g_t = gt[g_per_sample ? b : i], zt = z[i], nt = net[i];
      band[e] = restore_xhat(zt, nt, g_t, mode);
    } else {
      band[e] = z[i];
    }
  }
  __syncthreads();

  const int teams = 256 / q.L, team = tid / q.L, lane = tid & (q.L - 1);
  const float n = (float)q.n_g;
  for (int g0 = 0; g0 < q.G; g0 += teams) {           // the same trip count in every thread
    const int g = g0 + team;
    const bool live = g < q.G;
    const float mean = restore_group_sum(band, q, live ? g : 0, live, lane) / n;
    if (live && lane == 0) {
      const size_t yi = blk * (size_t)q.G + g;        // y [B, H / f, W / f, Cy]: band blk holds G consecutive values
      if (PROJECT) corr[g] = y[yi] - mean;
      else out[yi] = mean;
    }
  }
  if (!PROJECT) return;
  __syncthreads();

  for (int e = tid; e < q.band; e += 256) out[base + e] = band[e] + corr[restore_group_of(q, e)];
}

// -> hipSuccess and the geometry, or hipErrorInvalidValue
int restore_geometry(int B, int H, int W, int C, int f, int gray, RestoreGeom* q, size_t* blocks, size_t* lds_bytes) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return (int)hipErrorInvalidValue;
  gray = gray != 0;
  const bool listed = f == 2 || f == 4 || f == 8 || f == 16 || (f == 1 && gray);     // f = 1: `gray` alone
  if (!listed || H % f || W % f) return (int)hipErrorInvalidValue;
  if (f == 1)                                          // pixels are the groups: fold rows into wider ones (see above)
    while (H % 2 == 0 && (size_t)2 * W * C <= 1024) H /= 2, W *= 2;
  const size_t band = (size_t)f * W * C, G = (size_t)(W / f) * (gray ? 1 : C);
  if (band + G > 16384) return (int)hipErrorInvalidValue;                               // 64 KiB of LDS
  const size_t nb = (size_t)B * (H / f);
  if (nb > 0xffffffull) return (int)hipErrorInvalidValue;         // 256 nb threads must stay below 2^32
  const int n_g = f * f * (gray ? C : 1);
  int L = 1;
  while (L * 2 <= n_g && L < 64) L *= 2;
  *q = RestoreGeom{H, W, C, f, gray, (int)band, (int)G, n_g, L, gray ? 1 : C};
  *blocks = nb;
  *lds_bytes = (band + G) * sizeof(float);
  return (int)hipSuccess;
}

}  // namespace

MULAN_API int mulan_restore_project(const float* z, const float* net, const float* g_t, const float* y, float* xh_out,
                                    int B, int H, int W, int C, int f, int gray, int mode, int g_per_sample,
                                    hipStream_t stream) {
  if (!z || !net || !g_t || !y || !xh_out || mode < 0 || mode > 2) return (int)hipErrorInvalidValue;
  RestoreGeom q;
  size_t nb, lds;
  if (restore_geometry(B, H, W, C, f, gray, &q, &nb, &lds) != (int)hipSuccess) return (int)hipErrorInvalidValue;
  if (g_per_sample != 0 && (long long)g_per_sample != (long long)H * W * C) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(restore_kernel<true>, dim3((unsigned)nb), dim3(256), lds, stream, z, net, g_t, y, xh_out, q, mode,
                     g_per_sample);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_restore_measure(const float* x, float* y_out, int B, int H, int W, int C, int f, int gray,
                                    hipStream_t stream) {
  if (!x || !y_out) return (int)hipErrorInvalidValue;
  RestoreGeom q;
  size_t nb, lds;
  if (restore_geometry(B, H, W, C, f, gray, &q, &nb, &lds) != (int)hipSuccess) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(restore_kernel<false>, dim3((unsigned)nb), dim3(256), lds, stream, x, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, y_out, q, 2, 0);
  MULAN_CHECK_LAUNCH();
}
