// Device helpers shared by the loss-head kernels (vdm_loss.hip) and the bound profile (bound_profile.hip): the 8-bit
// encoding, the decoder's bin values and the window of bins whose softmax term is not exactly zero.
#pragma once
#include "common.h"

__device__ __forceinline__ float encode_u8(unsigned char x) { return 2.f * (((float)x + 0.5f) / 256.f) - 1.f; }
__device__ __forceinline__ float bin_val(int j) { return 2.f * (((float)j + 0.5f) / 256.f) - 1.f; }

// The bins whose softmax term exp(-0.5 u_j^2 - mx) is not exactly 0.0f in fp32, u_j = (z0 - bin_val(j)) istd: with the
// reference's gamma_0 = -13.3 the bins are 6 standard deviations apart and 5-7 of the 256 terms are non-zero.  expf
// returns 0 below -104.7; every bin with -0.5 u_j^2 - mx > -106 is inside [jlo, jhi] (one bin and 1e-4 of slack for the
// rounding of this estimate), as is the nearest bin (the maximum), so the sums over the window in ascending j are, bit
// for bit, the sums over all 256 bins: the skipped terms add +0.0f.  Wide noise, infinities and NaN give the full range.
__device__ __forceinline__ void bin_window(float z0, float istd, int& jlo, int& jhi) {
  const float pos = (z0 + 1.f) * 128.f - 0.5f;                 // z0 in bin units: bin_val(j) = (j + 0.5) / 128 - 1
  const float s = istd * (1.f / 128.f);                        // u_j = (pos - j) s
  const float dstar = fabsf(pos - fminf(fmaxf(rintf(pos), 0.f), 255.f));     // distance to the nearest bin
  const float R = sqrtf(212.f / (s * s) + dstar * dstar) * 1.0001f + 1.5f;
  jlo = (int)fmaxf(0.f, fminf(255.f, floorf(pos - R)));
  jhi = (int)fminf(255.f, fmaxf(0.f, ceilf(pos + R)));
  if (!(R < 1e6f) || !(fabsf(pos) < 1e6f)) { jlo = 0; jhi = 255; }
}
