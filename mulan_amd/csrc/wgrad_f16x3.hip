// Weight gradients in the f16x3 arithmetic (see conv3x3_f16x3.hip): of the 3x3 convolutions (from fp32 tensors, or from
// the split planes the forward / input-gradient kernels hand on), of every per-pixel dense layer, and the attention
// core's batched x^T dy.  Kernels first, then one shape check and one launcher for the plane-fed family, then the
// entry points.
#include "common.h"
#include "f16x3_common.h"

namespace {

using namespace f16x3;

// ------------------------------------------------------------------------------------------------ wgrad
// dW[t][ci][co] = sum_pixels x[p + shift_t][ci] * dy[p][co] with the same 3-pass split.  The contraction index is
// the pixel, while both tensors are stored channel-contiguous, so the operands are fetched with the transposing LDS
// read ds_read_b64_tr_b16 (a 4 k x 16 channel block per 16-lane group, delivered k-major): a tap shift is then a
// whole-row address offset and every read stays 8-byte aligned.  LDS rows are 64 B (32 channels of one split plane),
// which makes the two 16-lane groups of a half-wave cover all 64 banks exactly once.
constexpr int WG_T = 64, WG_ROWS = 2;
constexpr int XPIX = (WG_ROWS + 2) * kPW;                 // 136 halo-patch pixels
constexpr int X_HALF = XPIX * 64, X_PLANE = 2 * X_HALF;   // bytes
constexpr int DPIX = WG_ROWS * kW;                        // 64
constexpr int D_HALF = DPIX * 64, D_PLANE = 2 * D_HALF;
constexpr int WG_SMEM = 2 * X_PLANE + 2 * D_PLANE;        // 34816 + 16384 = 51200

struct WgradArgsH {
  const float* x; const float* dy; float* slab;
  const unsigned* xmax; const unsigned* dymax;    // [B] per-image maxima (the kernel takes the tensor maximum)
  int B, H, C, N, S;
};

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f16x8 tr_read8h(const unsigned char* base) {
  // two 4-k blocks (k .. k+3 and k+4 .. k+7) -> the 8 k values of this lane's MFMA operand
  typedef __attribute__((address_space(3))) s16x4* lds_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base + 4 * 64));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(f16x8, v);
}

__global__ __launch_bounds__(256) void conv3x3_wgrad_f16x3_kernel(WgradArgsH p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* xs = smem;
  unsigned char* ds = smem + 2 * X_PLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wci = wave >> 1, wco = wave & 1;
  const int C = p.C, N = p.N;
  const int c0 = blockIdx.y * WG_T, n0 = blockIdx.z * WG_T;
  const int pairs_per_img = p.H / WG_ROWS;
  const int total_pairs = p.B * pairs_per_img;
  const int per_split = (total_pairs + p.S - 1) / p.S;
  const int pair_begin = blockIdx.x * per_split;
  const int pair_end = min(total_pairs, pair_begin + per_split);

  // tensor maxima -> scales
  float sx, inv_x, sg, inv_g;
  {
    unsigned mx = 0, mg = 0;
    for (int i = tid; i < p.B * kMaxParts; i += 256) { mx = max(mx, p.xmax[i]); mg = max(mg, p.dymax[i]); }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
      mg = max(mg, (unsigned)__shfl_xor((int)mg, o, 64));
    }
    unsigned* red = reinterpret_cast<unsigned*>(smem);
    if (lane == 0) { red[wave] = mx; red[4 + wave] = mg; }
    __syncthreads();
    mx = max(max(red[0], red[1]), max(red[2], red[3]));
    mg = max(max(red[4], red[5]), max(red[6], red[7]));
    __syncthreads();
    scale_of(mx, sx, inv_x);
    scale_of(mg, sg, inv_g);
    balance_pow2(inv_x, inv_g);
  }

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  constexpr int XV = (XPIX * 16 + 255) / 256;   // 9 float4 slots / thread
  constexpr int DV = (DPIX * 16) / 256;         // 4
  f32x4 xreg[XV], dreg[DV];
  int xoff[XV], doff[DV], xdst[XV], ddst[DV];
  unsigned xstat = 0, xtop = 0, xbot = 0, dstat = 0, xmask = 0;
#pragma unroll
  for (int i = 0; i < XV; ++i) {
    const int slot = tid + i * 256;
    const int q = slot & 15, pix = slot >> 4;
    const int prow = pix / kPW, pcol = pix - prow * kPW;
    const int ww = pcol - 1, c = c0 + q * 4;
    const bool inb = slot < XPIX * 16;
    const bool ok = inb && ww >= 0 && ww < kW && c < C;
    xoff[i] = ((prow - 1) * kW + ww) * C + c;
    xdst[i] = inb ? (q >> 3) * X_HALF + pix * 64 + (q & 7) * 8 : -1;
    xstat |= (ok ? 1u : 0u) << i;
    xtop |= (prow == 0 ? 1u : 0u) << i;
    xbot |= (prow == WG_ROWS + 1 ? 1u : 0u) << i;
  }
#pragma unroll
  for (int i = 0; i < DV; ++i) {
    const int slot = tid + i * 256;
    const int q = slot & 15, pix = slot >> 4;
    const int n = n0 + q * 4;
    doff[i] = pix * N + n;
    ddst[i] = (q >> 3) * D_HALF + pix * 64 + (q & 7) * 8;
    dstat |= (n < N ? 1u : 0u) << i;
  }
  auto gload = [&](int pr) {
    const int b = pr / pairs_per_img, h0 = (pr - b * pairs_per_img) * WG_ROWS;
    const float* xrow = p.x + ((size_t)b * p.H + h0) * kW * C;
    const float* dyb = p.dy + ((size_t)b * p.H + h0) * kW * N;
    xmask = xstat & ~(h0 == 0 ? xtop : 0u) & ~(h0 + WG_ROWS >= p.H ? xbot : 0u);
#pragma unroll
    for (int i = 0; i < XV; ++i) xreg[i] = *reinterpret_cast<const f32x4*>(((xmask >> i) & 1u) ? xrow + xoff[i] : p.x);
#pragma unroll
    for (int i = 0; i < DV; ++i) dreg[i] = *reinterpret_cast<const f32x4*>(((dstat >> i) & 1u) ? dyb + doff[i] : p.dy);
  };
  auto split_store = [&](unsigned char* base, int plane_stride, int dst, f32x4 v, float s) {
    f16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      _Float16 h, l;
      split2(v[e] * s, h, l);
      hi[e] = h; lo[e] = l;
    }
    *reinterpret_cast<f16x4*>(base + dst) = hi;
    *reinterpret_cast<f16x4*>(base + plane_stride + dst) = lo;
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      if (xdst[i] < 0) continue;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      split_store(xs, X_PLANE, xdst[i], ((xmask >> i) & 1u) ? xreg[i] : z, sx);
    }
#pragma unroll
    for (int i = 0; i < DV; ++i) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      split_store(ds, D_PLANE, ddst[i], ((dstat >> i) & 1u) ? dreg[i] : z, sg);
    }
  };

  const int grp_q = (lane & 15) >> 2, grp_p = lane & 3, cb16 = ((lane >> 4) & 1) * 16;
  const int lane_off = (8 * lh + grp_q) * 64 + (cb16 + 4 * grp_p) * 2;
  const unsigned char* xa = xs + wci * X_HALF + lane_off;
  const unsigned char* db = ds + wco * D_HALF + lane_off;

  if (pair_begin < pair_end) {
    gload(pair_begin);
    lstore();
  }
  __syncthreads();
  for (int pr = pair_begin; pr < pair_end; ++pr) {
    const bool has_next = pr + 1 < pair_end;
    if (has_next) gload(pr + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
    for (int ks = 0; ks < DPIX / 16; ++ks) {
      const int rr = ks >> 1, w0 = (ks & 1) * 16;
      f16x8 bfr[2];
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) bfr[pl] = tr_read8h(db + pl * D_PLANE + (rr * kW + w0) * 64);
      f16x8 af[2][2];
      const unsigned char* xk = xa + (rr * kPW + w0) * 64;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) af[0][pl] = tr_read8h(xk + pl * X_PLANE);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (t + 1 < 9) {
          const int kh = (t + 1) / 3, kw = (t + 1) % 3;
#pragma unroll
          for (int pl = 0; pl < 2; ++pl) af[(t + 1) & 1][pl] = tr_read8h(xk + pl * X_PLANE + (kh * kPW + kw) * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t & 1][1], bfr[0], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t & 1][0], bfr[1], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t & 1][0], bfr[0], acc[t], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (has_next) {
      lstore();
      __syncthreads();
    }
  }

  float* slab = p.slab + (size_t)blockIdx.x * 9 * C * N;
  const int n = n0 + wco * 32 + li;
  if (n < N) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = c0 + wci * 32 + mfma32_row(r, lane);
        if (c < C) slab[((size_t)t * C + c) * N + n] = (acc[t][r] * inv_x) * inv_g;
      }
  }
}

// ---- plane-fed, row-split weight-gradient kernel.
// Inputs are the split planes that the forward / input-gradient convolutions write as a by-product
// ([B][C/16][H*W][plane][16] fp16, scaled per image), so staging is a plain copy: the fp32 -> 2 x fp16 split is done
// once per tensor instead of once per consuming block, and nothing competes with the MFMAs for the VALU.  The
// accumulators live in the units of the image being multiplied (s_x[b] s_dy[b]): when the pixel range crosses into the
// next image they are multiplied by the exact power of two between the two images' scales (in place, on the accumulator
// registers).
// A block owns a 128 ci x 128 co tile over a range of row pairs (2 image rows): of one kernel row kh (3 taps) in the 3x3
// kernel, of the single tap in the dense one -- a fraction of the LDS traffic per MFMA of the 9-tap kernel above, and no
// vertical halo.
// Three row pairs are in flight: pair p is multiplied out of LDS buffer (p & 1), pair p + 1 sits in registers and is
// copied into the other buffer, pair p + 2 is being fetched (a whole iteration of latency budget); one barrier / pair.
constexpr int WG3_T = 128;
constexpr int X3PIX = WG_ROWS * kPW;                          // 68 pixels: 2 rows x (32 + 2 halo columns)
constexpr int X3_HALF = X3PIX * 64 + 64, X3_PLANE = 4 * X3_HALF + 32;   // +64: the 4 halves of a pixel start 16 banks
constexpr int D3_HALF = DPIX * 64 + 64, D3_PLANE = 4 * D3_HALF + 32;    // apart; +32: plane 1 sits 8 banks further
constexpr int WG3_BUF = 2 * X3_PLANE + 2 * D3_PLANE;          // 35392 + 33344 = 68736
constexpr int WG3_SMEM = 2 * WG3_BUF;                         // 137472

struct WgradArgsP {
  const unsigned char* xs; const unsigned char* dys;   // split planes of x [B][C/16][HW][2][16], dy [B][N/16][HW][2][16]
  const unsigned* xmax; const unsigned* dymax;         // [B] per-image maxima the planes were scaled with
  float* slab;
  int B, H, C, N, S;
  unsigned long long* stamps;                          // dev-only (mulan_set_debug_buffer)
  // XF32 instantiation (one-tap kernel only): x arrives in fp32 as the virtual concat [x1 | x2] ([B][HW][C1], [B][HW][C - C1])
  // and is split while it is staged; xmax holds the maxima of the concat (elementwise max of the two tensors' maxima)
  const float* x1f; const float* x2f; int C1;
  const unsigned* xmax2;                               // (XF32) maxima of x2: the concat's are the elementwise max of xmax, xmax2
};

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));


__device__ __forceinline__ int clamped_exp(unsigned maxbits) {
  const int e = (int)((maxbits >> 23) & 255u);
  return e < 14 ? 14 : (e > 254 ? 254 : e);
}


// The four-wave block, one tap: a wave owns 64 ci x 64 co on v_mfma_f32_32x32x16_f16.  A 1x1 "convolution", i.e. the
// weight gradient x^T dy of a per-pixel dense layer (nin_shortcut, the attention projections and the attention core's
// batched products) from the planes its forward kernel handed on: only the centre tap of the LDS image (the haloed x
// row layout is the one the eight-wave 3x3 kernel below shares; the halo columns are staged and never read).
// XF32: the x operand is read in fp32 and split in the staging path instead of arriving as planes.  The
// dense weight gradient is memory bound (48 MFMAs per wave and row pair against 68 KB of operands), so the split
// arithmetic is free there, and the layer's forward kernel no longer has to write the planes of its input (134 MB per
// nin_shortcut at E = 128: 27 us of a 83 us launch, profiles/r03_linear_probe.log).  Same values as the planes the
// forward kernel used to hand on (split2 of x * s with the concat's per-image scale): bit-identical dw.
template <bool XF32 = false>
__global__ __launch_bounds__(256) void conv3x3_wgrad_f16x3_planes_kernel(WgradArgsP p) {
  constexpr int NQ = 4;                          // stages per row pair: 4 k steps
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wci = wave >> 1, wco = wave & 1;
  const int C = p.C, N = p.N;
  const int ntn = N / WG3_T;
  const int c0 = (blockIdx.z / ntn) * WG3_T, n0 = (blockIdx.z % ntn) * WG3_T;
  const int nchc = C / 16, nchn = N / 16;
  const int pairs_per_img = p.H / WG_ROWS;
  const int total_pairs = p.B * pairs_per_img;
  auto xmax_of = [&](int b) {
    unsigned m = row_max16(p.xmax, b);
    if constexpr (XF32) { if (p.xmax2) m = max(m, row_max16(p.xmax2, b)); }
    return m;
  };
  const int pair_begin = (int)((long long)blockIdx.x * total_pairs / p.S);
  const int pair_end = (int)((long long)(blockIdx.x + 1) * total_pairs / p.S);

  f32x16 acc[2][2];         // [ci tile][co tile]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // staging units of 16 bytes (8 channels of one plane of one pixel): unit e = tid + 256 i,
  //   e & 3 -> (plane, channel half),  e >> 2 = chunk * pixels + pixel   (consecutive lanes: consecutive 64-B records)
  constexpr int XV = (X3PIX * 32 + 255) / 256;  // 9 (2176 units)
  constexpr int DV = (DPIX * 32) / 256;         // 8 (2048 units)
  i32x4 xreg[XV], dreg[DV];
  const int hw = p.H * kW;                       // pixels per image: a chunk of the planes is [hw][plane][16]
  const __amdgpu_buffer_rsrc_t xs_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.xs), 0, p.B * nchc * hw * 64, kBufWord3);
  const __amdgpu_buffer_rsrc_t ds_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.dys), 0, p.B * nchn * hw * 64, kBufWord3);
  const int u = tid & 3, upl = u >> 1, uh = u & 1;
  // fp32 x: float4 unit t = tid + 256 i (i < 8): pixel t >> 5 of the pair's 64, channel quad t & 31 of the 128-ci tile
  const bool x_first = c0 < p.C1;
  const int ldxf = x_first ? p.C1 : C - p.C1, cxf = x_first ? c0 : c0 - p.C1;
  const __amdgpu_buffer_rsrc_t xf_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(x_first ? p.x1f : p.x2f), 0, XF32 ? (int)((size_t)p.B * 1024 * ldxf * 4) : 0, kBufWord3);
  int b_stage = -1;
  float sx_stage = 0.f;
  auto gload_x1 = [&](int pr, int i) {
    const int b = pr / pairs_per_img, h0 = (pr - b * pairs_per_img) * WG_ROWS;
    if constexpr (XF32) {
      if (i < 8) {
        const int t = tid + 256 * i;
        const int pix = t >> 5, q = t & 31;
        const unsigned off = (unsigned)((((b * 1024 + h0 * kW + pix) * ldxf) + cxf + q * 4) * 4);
        xreg[i] = __builtin_amdgcn_raw_buffer_load_b128(xf_rsrc, off, 0, 0);
      }
      return;
    }
    const int t = (tid >> 2) + 64 * i;
    const int cc = t / X3PIX, pix = t - cc * X3PIX;
    const int prow = pix / kPW, pcol = pix - prow * kPW;
    const int hh = h0 + prow;
    const bool ok = t < 8 * X3PIX && pcol >= 1 && pcol <= kW && hh >= 0 && hh < p.H;
    const unsigned off = (unsigned)((((b * nchc + (c0 >> 4) + cc) * hw + hh * kW + pcol - 1) * 2 + upl) * 32 + uh * 16);
    xreg[i] = __builtin_amdgcn_raw_buffer_load_b128(xs_rsrc, ok ? off : 0xffffffffu, 0, 0);
  };
  auto gload_d1 = [&](int pr, int i) {
    const int b = pr / pairs_per_img, h0 = (pr - b * pairs_per_img) * WG_ROWS;
    const int t = (tid >> 2) + 64 * i;
    const int cc = t >> 6, pix = t & 63;
    const unsigned off = (unsigned)((((b * nchn + (n0 >> 4) + cc) * hw + h0 * kW + pix) * 2 + upl) * 32 + uh * 16);
    dreg[i] = __builtin_amdgcn_raw_buffer_load_b128(ds_rsrc, off, 0, 0);
  };
  // branch free (the loop body must stay one basic block): the 128 units past the x tile land in a dummy area
  // (XF32) the scale of the image the staged pair belongs to; set_stage_scale(pr) before the pair's first store
  auto set_stage_scale = [&](int pr) {
    if constexpr (XF32) {
      const int b = pr / pairs_per_img;
      if (b != b_stage) {
        float inv;
        scale_of(xmax_of(b), sx_stage, inv);
        b_stage = b;
      }
    }
  };
  auto store_x = [&](unsigned char* buf, int i) {
    if constexpr (XF32) {
      if (i < 8) {
        const int t = tid + 256 * i;
        const int pix = t >> 5, q = t & 31;
        const int cc = q >> 2, pixl = (pix >> 5) * kPW + (pix & 31) + 1;       // interior pixel of the haloed row layout
        const f32x4 v = __builtin_bit_cast(f32x4, xreg[i]);
        f16x4 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          _Float16 h, l;
          split2(v[e] * sx_stage, h, l);
          hi[e] = h; lo[e] = l;
        }
        unsigned char* d = buf + (cc >> 1) * X3_HALF + pixl * 64 + (cc & 1) * 32 + (q & 3) * 8;
        *reinterpret_cast<f16x4*>(d) = hi;
        *reinterpret_cast<f16x4*>(d + X3_PLANE) = lo;
      }
      return;
    }
    const int t = (tid >> 2) + 64 * i;
    const int cc = t / X3PIX, pix = t - cc * X3PIX;
    const int dst = upl * X3_PLANE + (cc >> 1) * X3_HALF + pix * 64 + (cc & 1) * 32 + uh * 16;
    *reinterpret_cast<i32x4*>(t < 8 * X3PIX ? buf + dst : smem + 2 * WG3_BUF) = xreg[i];
  };
  auto store_d = [&](unsigned char* buf, int i) {
    const int t = (tid >> 2) + 64 * i;
    const int cc = t >> 6, pix = t & 63;
    const int dst = 2 * X3_PLANE + upl * D3_PLANE + (cc >> 1) * D3_HALF + pix * 64 + (cc & 1) * 32 + uh * 16;
    *reinterpret_cast<i32x4*>(buf + dst) = dreg[i];
  };

  // lane part of every transposing read: row q of the 4-k block, columns 4p..4p+3 of this group's 16 channels,
  // k half = lh  (MFMA operand element j <-> k = 8 lh + j)
  const int grp_q = (lane & 15) >> 2, grp_p = lane & 3, cb16 = ((lane >> 4) & 1) * 16;
  const int lane_off = (8 * lh + grp_q) * 64 + (cb16 + 4 * grp_p) * 2;
  const int xa_off = (wci * 2) * X3_HALF + lane_off;
  const int db_off = 2 * X3_PLANE + (wco * 2) * D3_HALF + lane_off;

  const bool stamp = p.stamps && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0;
  if (stamp) { p.stamps[0] = __builtin_amdgcn_s_memtime(); p.stamps[30] = __builtin_amdgcn_s_memrealtime(); }
  const int last = pair_end - 1;
  int b_acc = pair_begin < pair_end ? pair_begin / pairs_per_img : 0;   // image whose scales the accumulators carry
  if (pair_begin < pair_end) {
    const int p1 = min(pair_begin + 1, last);
#pragma unroll
    for (int i = 0; i < XV; ++i) gload_x1(pair_begin, i);
#pragma unroll
    for (int i = 0; i < DV; ++i) gload_d1(pair_begin, i);
    set_stage_scale(pair_begin);
#pragma unroll
    for (int i = 0; i < XV; ++i) store_x(smem, i);
#pragma unroll
    for (int i = 0; i < DV; ++i) store_d(smem, i);
#pragma unroll
    for (int i = 0; i < XV; ++i) gload_x1(p1, i);
#pragma unroll
    for (int i = 0; i < DV; ++i) gload_d1(p1, i);
  }
  __syncthreads();
  if (stamp) p.stamps[1] = __builtin_amdgcn_s_memtime();
  for (int pr = pair_begin; pr < pair_end; ++pr) {
    if (stamp && pr - pair_begin < 20) p.stamps[2 + pr - pair_begin] = __builtin_amdgcn_s_memtime();
    const int cur = (pr - pair_begin) & 1;
    const unsigned char* bc = smem + cur * WG3_BUF;
    unsigned char* bn = smem + (cur ^ 1) * WG3_BUF;
    const int pr2 = min(pr + 2, last);                 // past the end: a harmless re-read of the last pair
    set_stage_scale(min(pr + 1, last));                // (XF32) the pair in the staging registers is pair pr + 1
    const int b_now = pr / pairs_per_img;
    if (b_now != b_acc) {                              // crossed into the next image: move the accumulators to its units
      const int d = (clamped_exp(xmax_of(b_acc)) - clamped_exp(xmax_of(b_now))) +
                    (clamped_exp(row_max16(p.dymax, b_acc)) - clamped_exp(row_max16(p.dymax, b_now)));
      // acc *= 2^d in place on the accumulator registers (kept in the "a" class so that the register allocation of
      // the main loop is not disturbed by this rare path); four registers per block so the moves interleave.
      // Neighbouring images mostly share their exponents: nothing to do then.
      if (d != 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; r += 4) {
            float t0, t1, t2, t3;
            asm volatile(
                "v_accvgpr_read_b32 %4, %0\n\tv_accvgpr_read_b32 %5, %1\n\t"
                "v_accvgpr_read_b32 %6, %2\n\tv_accvgpr_read_b32 %7, %3\n\ts_nop 0\n\t"
                "v_ldexp_f32 %4, %4, %8\n\tv_ldexp_f32 %5, %5, %8\n\tv_ldexp_f32 %6, %6, %8\n\tv_ldexp_f32 %7, %7, %8\n\t"
                "s_nop 1\n\t"
                "v_accvgpr_write_b32 %0, %4\n\tv_accvgpr_write_b32 %1, %5\n\t"
                "v_accvgpr_write_b32 %2, %6\n\tv_accvgpr_write_b32 %3, %7"
                : "+a"(acc[i][j][r]), "+a"(acc[i][j][r + 1]), "+a"(acc[i][j][r + 2]), "+a"(acc[i][j][r + 3]),
                  "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                : "v"(d));
          }
      }
      b_acc = b_now;
    }
    const unsigned char* xa = bc + xa_off;
    const unsigned char* db = bc + db_off;
    f16x8 af[2][2][2], bfr[2][2][2];                   // [buffer][tile][plane]
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) bfr[0][j][pl] = tr_read8h(db + pl * D3_PLANE + j * D3_HALF);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) af[0][i][pl] = tr_read8h(xa + pl * X3_PLANE + i * X3_HALF + 64);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {                     // stage q = k step: 16 pixels of row rr = q >> 1
      const int ks = q;
      if (q + 1 < NQ) {                                // next stage's x fragments (centre tap: + 1 past the halo column)
        const int rr = (q + 1) >> 1, w0 = ((q + 1) & 1) * 16;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
            af[(q + 1) & 1][i][pl] = tr_read8h(xa + pl * X3_PLANE + i * X3_HALF + (rr * kPW + w0 + 1) * 64);
      }
      if (ks + 1 < 4) {                                // next k step's dy fragments
        const int rr = (ks + 1) >> 1, w0 = ((ks + 1) & 1) * 16;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
            bfr[(ks + 1) & 1][j][pl] = tr_read8h(db + pl * D3_PLANE + j * D3_HALF + (rr * kW + w0) * 64);
      }
      // staging, each register refilled at once with the same unit of pair p + 2: units q, q + 4, (q + 8)
#pragma unroll
      for (int uu = q; uu < XV; uu += 4) { store_x(bn, uu); gload_x1(pr2, uu); }
#pragma unroll
      for (int uu = q; uu < DV; uu += 4) { store_d(bn, uu); gload_d1(pr2, uu); }
#pragma unroll
      for (int term = 0; term < 3; ++term) {
        constexpr int PA[3] = {1, 0, 0};
        constexpr int PB[3] = {0, 1, 0};
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[q & 1][i][PA[term]], bfr[ks & 1][j][PB[term]],
                                                               acc[i][j], 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 12; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  }

  if (stamp) p.stamps[22] = __builtin_amdgcn_s_memtime();
  float sdummy, inv_x, inv_g;
  scale_of(xmax_of(b_acc), sdummy, inv_x);
  scale_of(row_max16(p.dymax, b_acc), sdummy, inv_g);
  float* slab = p.slab + (size_t)blockIdx.x * C * N;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wco * 64 + j * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = c0 + wci * 64 + i * 32 + mfma32_row(r, lane);
        slab[(size_t)c * N + n] = (acc[i][j][r] * inv_x) * inv_g;
      }
    }
  if (stamp) { p.stamps[23] = __builtin_amdgcn_s_memtime(); p.stamps[31] = __builtin_amdgcn_s_memrealtime(); }
}

// ---- the 3x3 plane-fed weight gradient: a block of EIGHT waves (round 6).
// A block owns one kernel row kh (3 taps) of a 128 ci x 128 co tile over a range of row pairs, in the LDS image and with
// the staging scheme described above (pair p multiplied, p + 1 in registers, p + 2 in flight); a wave owns 32 ci x 64 co
// x 3 taps (96 accumulators, <= 256 registers), so TWO waves share every SIMD and one's MFMAs fill the slots the other
// loses after each barrier and on every fragment wait (a four-wave block of 64 ci x 64 co waves issued 144 MFMAs per row
// pair in 5.76 k cycles where 4.6 k would be back to back, profiles/r03_wgrad_block_timeline.log).
// The halo columns of the x rows (always zero) are written once in the prologue instead of being staged with every
// pair: 2048 + 2048 sixteen-byte units per pair = 4 + 4 per thread, no partial slots.
// Grid: one dimension, decoded so that the blocks of one pixel range (3 kh x tiles) run on one XCD (block L runs on
// XCD L % 8) for ANY split count -- the launcher can use 255 of the 256 CUs (S = 85 at one tile) instead of 240: the
// planes come from HBM once and from L2 twice.
constexpr int W8_THREADS = 512;

__device__ __forceinline__ void w8_decode(int L, int S, int tiles, int& s, int& kh, int& tile) {
  const int nslot = 3 * tiles, full = S & ~7;
  int slot;
  if (L < full * nslot) {
    const int g = L / (8 * nslot), rem = L - g * 8 * nslot;
    slot = rem >> 3;
    s = g * 8 + (rem & 7);
  } else {
    const int l2 = L - full * nslot, G = S - full;
    slot = l2 / G;
    s = full + (l2 - slot * G);
  }
  tile = slot / 3;
  kh = slot - tile * 3;
}

// ---- the kernel, on v_mfma_f32_16x16x32_f16.
// A first form of this block on v_mfma_f32_32x32x16_f16 ran the train step at 76.4 ms; a timing probe with every MFMA
// replaced by two 16x16x32 on the same fragments ran it 4.5 ms shorter (72.9 ms): under the chip's power limit the 16x16
// shape holds a 12-15 % higher clock for the same matrix work (MI355X_MICROARCH.md, clock note 7), and the energy it does
// not draw is there for the kernels on the other stream.  K = 32 of one MFMA is one whole image row of 32 pixels: a row
// pair is 2 k steps x 3 taps = 6 stages of 24 MFMAs per wave (wave = 32 ci x 64 co x 3 taps = 2 x 4 tiles of 16 x 16,
// 96 accumulators).
// Transposing reads for this operand shape put the four 16-lane groups of a wave on pixels 8 g .. 8 g + 7 of the SAME 16
// channels: with 64-byte pixel records, groups g and g + 1 of a 32-lane bank group would hit the same banks (8 pixels =
// 512 bytes).  The two 16-channel halves of a record therefore swap places on pixel columns with bit 3 set
// (swizzle by the column inside the padded row, applied by the staging stores and by every fragment address): conflict free
// for every tap shift.
// One barrier per row pair, placed BEFORE the last stage: every LDS read of the pair has completed by then, so the last
// stage prefetches the first fragments of the next pair from the other buffer and no wave starts a pair by waiting for
// LDS (the 32x32 form stalled there, both waves of a SIMD at once).
__device__ __forceinline__ f16x8 tr_read8h2(const unsigned char* lo_addr, const unsigned char* hi_addr) {
  typedef __attribute__((address_space(3))) s16x4* lds_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(lo_addr));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(hi_addr));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(f16x8, v);
}

__global__ __launch_bounds__(W8_THREADS) void conv3x3_wgrad_f16x3_w16_kernel(WgradArgsP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wci = wave >> 1, wco = wave & 1;
  const int C = p.C, N = p.N;
  const int ntn = N / WG3_T;
  int bs, kh, tile;
  w8_decode(blockIdx.x, p.S, (C / WG3_T) * ntn, bs, kh, tile);
  const int c0 = (tile / ntn) * WG3_T, n0 = (tile % ntn) * WG3_T;
  const int nchc = C / 16, nchn = N / 16;
  const int pairs_per_img = p.H / WG_ROWS;
  const int total_pairs = p.B * pairs_per_img;
  const int pair_begin = (int)((long long)bs * total_pairs / p.S);
  const int pair_end = (int)((long long)(bs + 1) * total_pairs / p.S);

  f32x4 acc[3][2][4];   // [kw][ci tile][co tile]
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Staging.  Unit i (0..3) of a thread: 16 bytes = 8 channels of one plane of one pixel;
  //   tid & 3 -> (plane, channel half), chunk = (tid >> 8) + 2 i, pixel = (tid >> 2) & 63 of the pair's 64.
  // A wave's 16 pixels lie in ONE image row (wrow), so everything that changes from pair to pair is wave-uniform:
  // the row's byte offset goes into the scalar offset of the buffer load, the lane part is a constant, and a row
  // outside the image is one OR of bit 31 into that constant (>= num_records: the load returns zeros).  A load
  // costs its own issue slot and two scalar adds -- the first form of this block spent ~15 instructions per load on
  // per-lane address arithmetic, clustered in one MFMA gap: ~600 of 5650 cycles per row pair (profiles/r06_w8_ablation.log).
  // The LDS destination carries the swizzle.
  i32x4 xreg[4], dreg[4];
  const __amdgpu_buffer_rsrc_t xs_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.xs), 0, 0x80000000, kBufWord3);
  const __amdgpu_buffer_rsrc_t ds_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.dys), 0, 0x80000000, kBufWord3);
  const int u = tid & 3, upl = u >> 1, uh = u & 1;
  const int spix = (tid >> 2) & 63, scol = spix & 31, scc = (tid >> 8) & 1;
  const int wrow = (wave & 3) >> 1;
  const unsigned chunk_b = (unsigned)(p.H * kW * 64);   // bytes of one 16-channel chunk of one image: [H * W][plane][16]
  const unsigned vlane = (unsigned)scc * chunk_b + (unsigned)((scol * 2 + upl) * 32 + uh * 16);
  const int xdst0 = upl * X3_PLANE + (wrow * kPW + scol + 1) * 64 + (scc ^ (((scol + 1) >> 3) & 1)) * 32 + uh * 16;
  const int ddst0 = 2 * X3_PLANE + upl * D3_PLANE + spix * 64 + (scc ^ ((scol >> 3) & 1)) * 32 + uh * 16;
  const unsigned xtile = (unsigned)(c0 >> 4) * chunk_b, dtile = (unsigned)(n0 >> 4) * chunk_b;
  // fetch pointer (the pair whose loads are being issued): image fb, pair fr inside it; scalar offsets and lane word
  int fb = 0, fr = 0;
  unsigned sx = 0, sd = 0, vx = vlane;
  auto set_fetch = [&](int b, int r) {
    fb = b; fr = r;
    const int hx = r * WG_ROWS + kh - 1 + wrow;                        // image row of this wave's x units
    sx = (unsigned)(b * nchc) * chunk_b + xtile + (unsigned)(hx * (kW * 64));
    sd = (unsigned)(b * nchn) * chunk_b + dtile + (unsigned)((r * WG_ROWS + wrow) * (kW * 64));
    vx = vlane | ((unsigned)hx >= (unsigned)p.H ? 0x80000000u : 0u);
  };
  auto gload_x1 = [&](int i) {
    xreg[i] = __builtin_amdgcn_raw_buffer_load_b128(xs_rsrc, vx, sx + (unsigned)i * 2u * chunk_b, 0);
  };
  auto gload_d1 = [&](int i) {
    dreg[i] = __builtin_amdgcn_raw_buffer_load_b128(ds_rsrc, vlane, sd + (unsigned)i * 2u * chunk_b, 0);
  };
  auto store_x = [&](unsigned char* buf, int i) { *reinterpret_cast<i32x4*>(buf + xdst0 + i * X3_HALF) = xreg[i]; };
  auto store_d = [&](unsigned char* buf, int i) { *reinterpret_cast<i32x4*>(buf + ddst0 + i * D3_HALF) = dreg[i]; };

  // fragment addressing: lane = (k group g = lane >> 4: pixels 8 g .. 8 g + 7; q, pq: the 4 pixels x 4 channel quads a
  // 16-lane group presents to the transposing read).  Padded column of the pixel a lane addresses in read s (0: pixels
  // .. + 3, 1: .. + 7) of tap kw: pc = kw + 8 g + q + 4 s; its swizzle bit (pc >> 3) & 1 = (g + carry) & 1 with
  // carry = (kw + q + 4 s) >> 3 -- three distinct lane patterns: no carry (every s = 0 read, kw = 0, all of dy),
  // (kw = 1, s = 1), (kw = 2, s = 1).
  const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;
  const int lane_px = (8 * g + q) * 64 + pq * 8;
  const int par0 = g & 1, par1 = (g + ((1 + q + 4) >> 3)) & 1, par2 = (g + ((2 + q + 4) >> 3)) & 1;
  // x: [variant: 0 no carry, 1 (kw 1, s 1), 2 (kw 2, s 1)][ci tile]
  int xoff[3][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    xoff[0][ti] = wci * X3_HALF + lane_px + (ti ^ par0) * 32;
    xoff[1][ti] = wci * X3_HALF + lane_px + (ti ^ par1) * 32;
    xoff[2][ti] = wci * X3_HALF + lane_px + (ti ^ par2) * 32;
  }
  int doff[2];   // [co sub-tile inside a 32-channel record]
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) doff[tj] = 2 * X3_PLANE + (wco * 2) * D3_HALF + lane_px + (tj ^ par0) * 32;

  f16x8 af[2][2][2], bfr[2][4][2];                     // [buffer][ci tile][plane], [buffer][co tile][plane]
  auto read_a = [&](const unsigned char* buf, int slot, int rr, int kw) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        const int o = pl * X3_PLANE + (rr * kPW + kw) * 64;
        af[slot][ti][pl] = tr_read8h2(buf + xoff[0][ti] + o, buf + xoff[kw][ti] + o + 4 * 64);
      }
  };
  auto read_b = [&](const unsigned char* buf, int slot, int rr) {
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        const unsigned char* a = buf + doff[tj & 1] + pl * D3_PLANE + (tj >> 1) * D3_HALF + rr * kW * 64;
        bfr[slot][tj][pl] = tr_read8h2(a, a + 4 * 64);
      }
  };

  const bool stamp = p.stamps && blockIdx.x == 0 && threadIdx.x == 0;
  if (stamp) { p.stamps[0] = __builtin_amdgcn_s_memtime(); p.stamps[30] = __builtin_amdgcn_s_memrealtime(); }
  if (tid < 256) {   // the zero halo columns (pixel columns 0 and 33) of both rows, planes, halves and buffers
    const int rec = tid >> 2;
    const int zb = rec >> 5, zpl = (rec >> 4) & 1, zh = (rec >> 2) & 3, zr = (rec >> 1) & 1, zc = (rec & 1) * (kPW - 1);
    const i32x4 z = {0, 0, 0, 0};
    *reinterpret_cast<i32x4*>(smem + zb * WG3_BUF + zpl * X3_PLANE + zh * X3_HALF + (zr * kPW + zc) * 64 + (tid & 3) * 16) = z;
  }
  const int last = pair_end - 1;
  int b_acc = pair_begin < pair_end ? pair_begin / pairs_per_img : 0;
  auto advance_fetch = [&]() {                         // to the next pair of this block's range; stays on the last one
    if (fb * pairs_per_img + fr < last) {
      int r = fr + 1, b = fb;
      if (r == pairs_per_img) { r = 0; ++b; }
      set_fetch(b, r);
    }
  };
  if (pair_begin < pair_end) {
    set_fetch(b_acc, pair_begin - b_acc * pairs_per_img);
#pragma unroll
    for (int i = 0; i < 4; ++i) gload_x1(i);
#pragma unroll
    for (int i = 0; i < 4; ++i) gload_d1(i);
#pragma unroll
    for (int i = 0; i < 4; ++i) store_x(smem, i);
#pragma unroll
    for (int i = 0; i < 4; ++i) store_d(smem, i);
    advance_fetch();
#pragma unroll
    for (int i = 0; i < 4; ++i) gload_x1(i);
#pragma unroll
    for (int i = 0; i < 4; ++i) gload_d1(i);
  }
  __syncthreads();
  read_b(smem, 0, 0);
  read_a(smem, 0, 0, 0);
  if (stamp) p.stamps[1] = __builtin_amdgcn_s_memtime();
  int b_now = b_acc, r_now = pair_begin - b_acc * pairs_per_img;
  for (int pr = pair_begin; pr < pair_end; ++pr) {
    if (stamp && pr - pair_begin < 20) p.stamps[2 + pr - pair_begin] = __builtin_amdgcn_s_memtime();
    const int cur = (pr - pair_begin) & 1;
    const unsigned char* bc = smem + cur * WG3_BUF;
    unsigned char* bn = smem + (cur ^ 1) * WG3_BUF;
    advance_fetch();                                   // -> pair pr + 2 (the registers hold pr + 1)
    if (b_now != b_acc) {                              // next image: move the accumulators to its units (exact powers of two)
      const int d = (clamped_exp(row_max16(p.xmax, b_acc)) - clamped_exp(row_max16(p.xmax, b_now))) +
                    (clamped_exp(row_max16(p.dymax, b_acc)) - clamped_exp(row_max16(p.dymax, b_now)));
      if (d != 0) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[t][i][j][r] = ldexpf(acc[t][i][j][r], d);
      }
      b_acc = b_now;
    }
    if (++r_now == pairs_per_img) { r_now = 0; ++b_now; }
#pragma unroll
    for (int st = 0; st < 6; ++st) {                   // st = rr * 3 + kw: image row rr of the pair (one k step), tap kw
      const int rr = st / 3, kw = st - rr * 3;
      if (st == 5) __syncthreads();                    // every LDS read of this pair is done: the other buffer is complete
      if (st < 5) read_a(bc, (st + 1) & 1, (st + 1) / 3, (st + 1) % 3);
      else read_a(bn, 0, 0, 0);                        // first fragments of the next pair
      if (st == 1) read_b(bc, 1, 1);
      if (st == 5) read_b(bn, 0, 0);
      if (st < 4) { store_x(bn, st); gload_x1(st); store_d(bn, st); gload_d1(st); }
#pragma unroll
      for (int term = 0; term < 3; ++term) {
        constexpr int PA[3] = {1, 0, 0};
        constexpr int PB[3] = {0, 1, 0};
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < 4; ++tj)
            acc[kw][ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[st & 1][ti][PA[term]], bfr[rr][tj][PB[term]],
                                                                     acc[kw][ti][tj], 0, 0, 0);
      }
      // the stage as a pipeline: one transposing read behind each of the first 8 (24: the stages that also fetch the
      // eight dy fragments) MFMAs, the two LDS stores and the two global loads of the stage spread behind later ones
#pragma unroll
      for (int gq = 0; gq < 24; ++gq) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (gq < 8 || st == 1 || st == 5) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        if (st < 4 && (gq == 9 || gq == 13)) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        if (st < 4 && (gq == 11 || gq == 15)) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  if (stamp) p.stamps[22] = __builtin_amdgcn_s_memtime();
  float sdummy, inv_x, inv_g;
  scale_of(row_max16(p.xmax, b_acc), sdummy, inv_x);
  scale_of(row_max16(p.dymax, b_acc), sdummy, inv_g);
  balance_pow2(inv_x, inv_g);
  float* slab = p.slab + (size_t)bs * 9 * C * N;
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) {
        const int n = n0 + wco * 64 + tj * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = c0 + wci * 32 + ti * 16 + 4 * g + r;
          slab[((size_t)(kh * 3 + kw) * C + c) * N + n] = (acc[kw][ti][tj][r] * inv_x) * inv_g;
        }
      }
  if (stamp) { p.stamps[23] = __builtin_amdgcn_s_memtime(); p.stamps[31] = __builtin_amdgcn_s_memrealtime(); }
}

// split count of the eight-wave kernel: any S works (w8_decode keeps a pixel range's blocks on one XCD), so a launch
// that owns the chip takes 255-256 CUs.  share_chip = 1 (an ARGUMENT of the entry point: the caller says that the launch
// shares the chip with another stream's kernels -- the train step's weight-gradient stream): 120 blocks for the one- and
// two-tile shapes, so that the other stream keeps half of the CUs and both run side by side (a block owns its CU); four
// tiles and more keep the whole chip (measured: E = 256 is slower with fewer).  tune[1] > 0: explicit target (dev only).
int wgrad_splits_w8(int B, int H, int C, int N, int share_chip) {
  const int tiles = (C / WG3_T) * (N / WG3_T);
  const int pairs = B * (H / WG_ROWS);
  int target = share_chip == 1 && tiles <= 2 ? 120 : 256;
  if (g_mulan_tune[1] > 0) target = g_mulan_tune[1];
  int S = target / (3 * tiles);
  if (S < 1) S = 1;
  if (S > pairs) S = pairs;
  return S;
}

__global__ void slab_reduce_h_kernel(const float* __restrict__ slab, float* __restrict__ out, int S, int E,
                                     int accumulate) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float s = 0.f;
  int i = 0;
  for (; i + 20 <= S; i += 20) {         // (S = 40 / 80 in the train step: 20 loads in flight, summed in index order)
    float v[20];
#pragma unroll
    for (int u = 0; u < 20; ++u) v[u] = slab[(size_t)(i + u) * E + e];
#pragma unroll
    for (int u = 0; u < 20; ++u) s += v[u];
  }
  for (; i + 8 <= S; i += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = slab[(size_t)(i + u) * E + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; i < S; ++i) s += slab[(size_t)i * E + e];
  out[e] = accumulate ? out[e] + s : s;
}

int wgrad_splits_h(int B, int H, int C, int N) {
  const int tiles = ((C + WG_T - 1) / WG_T) * ((N + WG_T - 1) / WG_T);
  const int pairs = B * (H / WG_ROWS);
  const int target = g_mulan_tune[1] > 0 ? g_mulan_tune[1] : 256;
  int S = target / tiles;
  if (S < 1) S = 1;
  if (S > pairs) S = pairs;
  while (S > 1 && pairs / S < 4) --S;
  return S;
}

}  // namespace

MULAN_API size_t mulan_conv3x3_wgrad_f16x3_workspace(int B, int H, int W, int C, int N) {
  if (W != kW || H % WG_ROWS != 0) return 0;
  return (size_t)wgrad_splits_h(B, H, C, N) * 9 * C * N * sizeof(float);
}

// dw[3,3,C,N] (+)= sum x (x) dy with the 3-pass fp16 split; xmax / dymax are the per-image maxima [B] of x and dy.
MULAN_API int mulan_conv3x3_wgrad_f16x3(const float* x, const unsigned* xmax, const float* dy, const unsigned* dymax,
                                        float* dw, float* workspace, int B, int H, int W, int C, int N, int accumulate,
                                        hipStream_t stream) {
  if (W != kW || H % WG_ROWS != 0 || B <= 0 || C % 4 != 0 || N % 4 != 0 || !xmax || !dymax)
    return (int)hipErrorInvalidValue;
  static bool configured = false;
  if (!configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_wgrad_f16x3_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, WG_SMEM);
    if (e != hipSuccess) return (int)e;
    configured = true;
  }
  const int S = wgrad_splits_h(B, H, C, N);
  const WgradArgsH a{.x = x, .dy = dy, .slab = workspace, .xmax = xmax, .dymax = dymax, .B = B, .H = H, .C = C, .N = N,
                     .S = S};
  dim3 grid(S, (C + WG_T - 1) / WG_T, (N + WG_T - 1) / WG_T);
  hipLaunchKernelGGL(conv3x3_wgrad_f16x3_kernel, grid, dim3(256), WG_SMEM, stream, a);
  const int E = 9 * C * N;
  hipLaunchKernelGGL(slab_reduce_h_kernel, dim3((E + 255) / 256), dim3(256), 0, stream, workspace, dw, S, E, accumulate);
  MULAN_CHECK_LAUNCH();
}

// ---- the plane-fed family: the 3x3 weight gradient, the dense one (from planes or from fp32 x) and the batched x^T dy.
// The grid every plane-fed kernel needs: 32 pixels wide, whole row pairs, whole 128 x 128 tiles.  The workspace functions
// answer 0 off this grid.
static bool wgrad_planes_grid_ok(int H, int W, int C, int N) {
  return W == kW && H % WG_ROWS == 0 && C % WG3_T == 0 && N % WG3_T == 0;
}

// What every plane-fed launch takes: the grid above, at least one image, both operands (x: planes, or the fp32 x1 of
// _x32) with the maxima they are scaled with, and tensors below 2 GiB (the kernels form 32-bit byte offsets).  What
// else an entry point requires stands in the entry point.
static bool wgrad_planes_shape_ok(const void* x, const unsigned* xmax, const void* dys, const unsigned* dymax, int B,
                                  int H, int W, int C, int N) {
  return wgrad_planes_grid_ok(H, W, C, N) && B > 0 && x && dys && xmax && dymax &&
         (size_t)B * H * W * (C > N ? C : N) * 4 < 0x80000000ull;
}

// One launch of a plane-fed kernel (all take WG3_SMEM + 64 bytes of dynamic LDS, allowed once per instantiation), then
// dw (+)= the sum of its a.S slabs of `taps` x C x N -- unless dw is NULL: the caller had the kernel write its result
// directly.  Returns the error of hipFuncSetAttribute if there is one, else 0: the caller ends with MULAN_CHECK_LAUNCH.
template <void (*KERNEL)(WgradArgsP)>
static int launch_wgrad_planes(const WgradArgsP& a, dim3 grid, int threads, int taps, float* dw, int accumulate,
                               hipStream_t stream) {
  static bool configured = false;
  if (!configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       WG3_SMEM + 64);
    if (e != hipSuccess) return (int)e;
    configured = true;
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(threads), WG3_SMEM + 64, stream, a);
  if (dw) {
    const int E = taps * a.C * a.N;
    hipLaunchKernelGGL(slab_reduce_h_kernel, dim3((E + 255) / 256), dim3(256), 0, stream, a.slab, dw, a.S, E, accumulate);
  }
  return 0;
}

MULAN_API size_t mulan_conv3x3_wgrad_f16x3_planes_workspace(int B, int H, int W, int C, int N, int share_chip) {
  if (!wgrad_planes_grid_ok(H, W, C, N)) return 0;
  return (size_t)wgrad_splits_w8(B, H, C, N, share_chip) * 9 * C * N * sizeof(float);
}

// dw[3,3,C,N] (+)= sum x (x) dy from the split planes written by mulan_conv3x3_fwd_f16x3 (xs: of the forward input,
// dys: of the output gradient, written by the input-gradient convolution); needs C % 128 == 0 and N % 128 == 0.
MULAN_API int mulan_conv3x3_wgrad_f16x3_planes(const void* xs, const unsigned* xmax, const void* dys,
                                               const unsigned* dymax, float* dw, float* workspace, int B, int H, int W,
                                               int C, int N, int accumulate, int share_chip, hipStream_t stream) {
  if (!wgrad_planes_shape_ok(xs, xmax, dys, dymax, B, H, W, C, N)) return (int)hipErrorInvalidValue;
  const int S = wgrad_splits_w8(B, H, C, N, share_chip);
  const WgradArgsP a{.xs = static_cast<const unsigned char*>(xs), .dys = static_cast<const unsigned char*>(dys),
                     .xmax = xmax, .dymax = dymax, .slab = workspace, .B = B, .H = H, .C = C, .N = N, .S = S,
                     .stamps = g_mulan_debug_buffer};
  if (const int rc = launch_wgrad_planes<conv3x3_wgrad_f16x3_w16_kernel>(a, dim3(3 * S * (C / WG3_T) * (N / WG3_T)),
                                                                      W8_THREADS, 9, dw, accumulate, stream))
    return rc;
  MULAN_CHECK_LAUNCH();
}

// ---- weight gradient of a per-pixel dense layer from split planes: dw[C, N] (+)= x^T dy, x planes [B][C/16][HW][2][16]
// (handed on by mulan_linear_f16x3), dy planes [B][N/16][HW][2][16] (handed on by the convolution that consumed the same
// dy); xmax / dymax are the per-image maxima the planes were scaled with.  Needs C % 128 == 0, N % 128 == 0.
static int linear_wgrad_splits(int B, int H, int C, int N, int share_chip) {
  const int tiles = (C / WG3_T) * (N / WG3_T);
  const int pairs = B * (H / WG_ROWS);
  const int target = share_chip == 1 ? 160 : 240;     // (shared chip, see wgrad_splits_w8: scan 64 ... 240)
  int S = target / tiles;
  if (S < 1) S = 1;
  if (S > pairs) S = pairs;
  return S;
}

MULAN_API size_t mulan_linear_wgrad_f16x3_planes_workspace(int B, int H, int W, int C, int N, int share_chip) {
  if (!wgrad_planes_grid_ok(H, W, C, N)) return 0;
  return (size_t)linear_wgrad_splits(B, H, C, N, share_chip) * C * N * sizeof(float);
}

MULAN_API int mulan_linear_wgrad_f16x3_planes(const void* xs, const unsigned* xmax, const void* dys,
                                              const unsigned* dymax, float* dw, float* workspace, int B, int H, int W,
                                              int C, int N, int accumulate, int share_chip, hipStream_t stream) {
  if (!wgrad_planes_shape_ok(xs, xmax, dys, dymax, B, H, W, C, N)) return (int)hipErrorInvalidValue;
  const int S = linear_wgrad_splits(B, H, C, N, share_chip);
  const WgradArgsP a{.xs = static_cast<const unsigned char*>(xs), .dys = static_cast<const unsigned char*>(dys),
                     .xmax = xmax, .dymax = dymax, .slab = workspace, .B = B, .H = H, .C = C, .N = N, .S = S,
                     .stamps = g_mulan_debug_buffer};
  if (const int rc = launch_wgrad_planes<conv3x3_wgrad_f16x3_planes_kernel<false>>(
      a, dim3(S, 1, (C / WG3_T) * (N / WG3_T)), 256, 1, dw, accumulate, stream))
    return rc;
  MULAN_CHECK_LAUNCH();
}

// The same weight gradient with x in fp32 (round 3): dw[C1 + C2, N] (+)= [x1 | x2]^T dy, x1 [B, H*W, C1] and x2 [B, H*W, C2]
// (x2 / C2 may be NULL / 0) read as they are and split while staged, dy as the planes the convolution that consumed the
// same dy handed on.  xmax, xmax2 [B][16]: the maxima of x1 and of x2 (the kernel takes their elementwise max: the maxima
// of the concat), i.e. the scale the layer's forward pass used: results equal mulan_linear_wgrad_f16x3_planes on the planes that pass would have
// written, bit for bit -- which the forward kernel therefore need not write.  C1 and C2 multiples of 128.
MULAN_API size_t mulan_linear_wgrad_f16x3_x32_workspace(int B, int H, int W, int C, int N, int share_chip) {
  return mulan_linear_wgrad_f16x3_planes_workspace(B, H, W, C, N, share_chip);
}

MULAN_API int mulan_linear_wgrad_f16x3_x32(const float* x1, const float* x2, int C1, int C2, const unsigned* xmax,
                                           const unsigned* xmax2, const void* dys, const unsigned* dymax, float* dw, float* workspace, int B,
                                           int H, int W, int N, int accumulate, int share_chip, hipStream_t stream) {
  const int C = C1 + C2;
  if (H != 32 || C1 <= 0 || C1 % WG3_T != 0 || C2 < 0 || C2 % WG3_T != 0 || (C2 > 0 && (!x2 || !xmax2)) ||
      !wgrad_planes_shape_ok(x1, xmax, dys, dymax, B, H, W, C, N))
    return (int)hipErrorInvalidValue;
  const int S = linear_wgrad_splits(B, H, C, N, share_chip);
  const WgradArgsP a{.dys = static_cast<const unsigned char*>(dys), .xmax = xmax, .dymax = dymax, .slab = workspace,
                     .B = B, .H = H, .C = C, .N = N, .S = S, .stamps = g_mulan_debug_buffer, .x1f = x1, .x2f = x2, .C1 = C1,
                     .xmax2 = C2 > 0 ? xmax2 : nullptr};
  if (const int rc = launch_wgrad_planes<conv3x3_wgrad_f16x3_planes_kernel<true>>(
      a, dim3(S, 1, (C / WG3_T) * (N / WG3_T)), 256, 1, dw, accumulate, stream))
    return rc;
  MULAN_CHECK_LAUNCH();
}

// out[b] = x[b]^T @ dy[b] per image:  [C, N] = sum over the H * 32 rows of image b of x[row, :]^T dy[row, :], both
// operands as split planes (the by-products of mulan_linear_f16x3 / _batched) scaled with xmax[b] / dymax[b].  The
// attention core's dV = P^T dO and dK = dS^T Q (autodiff of ldm/model_vdm.py:775-796) on the dense weight-gradient
// kernel with one slab per image and no slab reduction.
MULAN_API int mulan_bmm_tn_f16x3_planes(const void* xs, const unsigned* xmax, const void* dys, const unsigned* dymax,
                                        float* out, int B, int H, int W, int C, int N, hipStream_t stream) {
  if (!wgrad_planes_shape_ok(xs, xmax, dys, dymax, B, H, W, C, N) || !out) return (int)hipErrorInvalidValue;
  const WgradArgsP a{.xs = static_cast<const unsigned char*>(xs), .dys = static_cast<const unsigned char*>(dys),
                     .xmax = xmax, .dymax = dymax, .slab = out, .B = B, .H = H, .C = C, .N = N, .S = B,
                     .stamps = g_mulan_debug_buffer};
  if (const int rc = launch_wgrad_planes<conv3x3_wgrad_f16x3_planes_kernel<false>>(
      a, dim3(B, 1, (C / WG3_T) * (N / WG3_T)), 256, 1, nullptr, 0, stream))
    return rc;
  MULAN_CHECK_LAUNCH();
}
