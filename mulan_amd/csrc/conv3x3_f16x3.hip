// 3x3 convolution with fp32-equivalent products on the fp16 matrix cores ("f16x3").
//
// An fp32 operand v, scaled by a power of two s so that max|v s| lies in [2^13, 2^14), splits into two fp16 pieces
//     v s = h + l,   h = fp16(v s),  l = fp16(v s - h)          (11 + 11 mantissa bits + the two rounding signs:
// |v s - h - l| <= 2^-24 |v s| as long as l is a normal fp16 number, and <= 2^-25 absolute below that: fp16 subnormals
// are honoured by the matrix cores, tools/f16_probe.hip), and
//     a * b  ~=  a_h b_h + a_h b_l + a_l b_h                    (the dropped a_l b_l is <= 2^-24 |a b|)
// is accumulated in fp32 by three v_mfma_f32_32x32x16_f16 per 16-deep k step: 5.3x fewer matrix-pipe cycles than
// v_mfma_f32_32x32x2_f32 at the same measured error against fp64 (tools/f16_probe.hip, tests/test_gpu_f16x3.py), and
// half the cycles of the 6-pass split into three bf16 pieces that the project used before.  The power-of-two scales
// are exact and are divided out of the fp32 accumulators in the epilogue.  Activations / output gradients carry one scale per
// image (every image is normalised on its own, so images of very different magnitude in one batch keep full
// precision); weights carry one scale per tensor; the weight-gradient kernel, which sums over images, uses the
// per-tensor maxima.  The reference asks XLA for float32 matmul precision (ldm/main.py:39); this is that contract.
//
// Forward / input-gradient tiling: a block covers 8 image rows x 128 couts of one image, with the halo patch of its rows
// in LDS and one stage per (16-channel chunk, tap); the weights are pre-split by mulan_conv3x3_pack_f16x3 into tiles
// [tap][chunk][cout][plane][16 k] that a wave's MFMA operand reads directly.  Two kernels share it: the 32x32x16
// one-block-per-CU kernel below and the 16x16x32 two-blocks-per-CU kernel of conv3x3_f16x3_v3.hip (the default where
// C % 32 == 0).
#include "common.h"
#include "f16x3_common.h"

namespace {

using namespace f16x3;

// ---- the 8-row 32x32x16 kernel: block = 8 image rows x 128 couts, wave = 4 rows x 64 couts (4 x 2 MFMA tiles, 128
// accumulator registers, one wave per SIMD).  The weight fragments are read straight from the packed global tensor
// (L2/L1 resident, two stages ahead, no LDS copy and no per-stage barrier); only the activation patch goes through
// LDS, double buffered, with one barrier per 16-channel chunk.  With three passes per product a block of 4 rows and
// 2 x 2 MFMA tiles that also staged its weights in LDS was LDS-bandwidth bound; this tiling halves the LDS traffic
// per MFMA.
constexpr int TR2 = 8;
constexpr int PATCH2_B = (TR2 + 2) * kPW * PIXB;     // 27200
constexpr int SMEM2_B = 2 * PATCH2_B + 64;           // 54464 (+ dummy store target)

__global__ __launch_bounds__(256) void conv3x3_f16x3_v2_kernel(ConvArgsH p) {
  constexpr int MT = 4, NT = 2;
  constexpr int PV = 6;                          // float4 patch slots per thread (1360 slots)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_per_img = p.H / TR2;
  const int b = blockIdx.x / tiles_per_img;
  const int h0 = (blockIdx.x % tiles_per_img) * TR2;
  const int n0 = blockIdx.y * BN;
  const int C = p.C, N = p.N;
  const int nchunks = C / CK;
  float sx, inv_x, sw, inv_w;
  scale_of(row_max16(p.xmax, b), sx, inv_x);
  scale_of(row_max16(p.wmax, 0), sw, inv_w);
  balance_pow2(inv_x, inv_w);

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // Global operands go through buffer descriptors: per-stage offsets are formed on the scalar unit (soffset) instead
  // of 64-bit vector address arithmetic, and halo / out-of-image slots simply read zeros (offset 2^31 is out of range).
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.x), 0, (int)((size_t)p.B * p.H * kW * C * 4), kBufWord3);
  const __amdgpu_buffer_rsrc_t wp_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(p.wp), 0, 9 * C * N * 4, kBufWord3);
  unsigned poff[PV];
  int pdst[PV];
  unsigned pemit[PV];
#pragma unroll
  for (int s = 0; s < PV; ++s) {
    const int slot = tid + s * 256;
    const int q = slot & 3, pix = slot >> 2;
    const int prow = pix / kPW, pcol = pix - prow * kPW;
    const int hh = h0 + prow - 1, ww = pcol - 1;
    const bool inb = slot < (TR2 + 2) * kPW * 4;
    const bool ok = inb && hh >= 0 && hh < p.H && ww >= 0 && ww < kW;
    poff[s] = ok ? (unsigned)((((b * p.H + hh) * kW + ww) * C + q * 4) * 4) : 0x80000000u;
    pdst[s] = inb ? pix * PIXB + q * 8 : -1;
    // byte offset of this slot's hi quad inside (image b, chunk 0) of the plane tensor; interior pixels only
    const bool interior = inb && prow >= 1 && prow <= TR2 && ww >= 0 && ww < kW;
    pemit[s] = interior ? (unsigned)(((hh * kW + ww) * 2) * 32 + q * 8) : 0xffffffffu;
  }
  // plane output window of this block: image b (nothing for the other cout blocks, or when not requested);
  // chunk_b: bytes of one 16-channel chunk of one image, [H * W][plane][16] fp16
  const unsigned chunk_b = (unsigned)(p.H * kW * 64);
  const __amdgpu_buffer_rsrc_t xs_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      p.xs + (size_t)b * nchunks * chunk_b, 0, (p.xs && blockIdx.y == 0) ? (int)(nchunks * chunk_b) : 0, kBufWord3);
  i32x4 preg[PV];
  auto gload_patch = [&](int cc) {
#pragma unroll
    for (int s = 0; s < PV; ++s) preg[s] = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, poff[s], cc * CK * 4, 0);
  };
  // branch free (the loop body must stay one basic block so that this work can be scheduled between the MFMAs;
  // even a uniform condition in here makes the compiler branch): slots beyond the patch land in a dummy area behind
  // the two patches.  (During the last chunk the "next" patch is a harmless re-load of the current one: same data,
  // stored into the idle buffer and re-emitted to the same place.)
  auto store_slot = [&](unsigned char* pb, int s, int cc) {
    const f32x4 v = __builtin_bit_cast(f32x4, preg[s]);
    f16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      _Float16 h, l;
      split2(v[e] * sx, h, l);
      hi[e] = h; lo[e] = l;
    }
    unsigned char* d = pdst[s] >= 0 ? pb + pdst[s] : smem + 2 * PATCH2_B;
    *reinterpret_cast<f16x4*>(d) = hi;
    *reinterpret_cast<f16x4*>(d + 32) = lo;
    // the same two quads go to the plane tensor (consumed by the weight-gradient kernel)
    const unsigned eo = pemit[s] != 0xffffffffu ? pemit[s] + (unsigned)cc * chunk_b : 0xffffffffu;
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(i32x2, hi), xs_rsrc, eo, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(i32x2, lo), xs_rsrc, eo == 0xffffffffu ? eo : eo + 32, 0, 0);
  };
  auto store_patch = [&](unsigned char* pb, int cc) {
#pragma unroll
    for (int s = 0; s < PV; ++s) store_slot(pb, s, cc);
  };
  // weight fragments: packed [tap][chunk][cout][plane][16 k] fp16; this lane's 8 k of cout (n0 + wn*64 + nt*32 + li)
  const unsigned bvoff = (unsigned)((n0 + wn * 64 + li) * 64 + lh * 16);
  auto gload_b = [&](f16x8 (&bs)[NT][2], int cc, int tap) {
    const int so = (tap * nchunks + cc) * N * 64;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
        bs[nt][pl] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wp_rsrc, bvoff + nt * 2048 + pl * 32, so, 0));
  };
  auto read_a = [&](f16x8 (&af)[MT][2], const unsigned char* pb, int tap) {
    const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int prow = wm * MT + mt + kh, pcol = li + kw;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
        af[mt][pl] = *reinterpret_cast<const f16x8*>(pb + (prow * kPW + pcol) * PIXB + pl * 32 + lh * 16);
    }
  };

  const bool stamp = p.stamps && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
  if (stamp) { p.stamps[0] = __builtin_amdgcn_s_memtime(); p.stamps[30] = __builtin_amdgcn_s_memrealtime(); }
  // dev-only timeline: [64 + 2 blk] = start, [65 + 2 blk] = end of every block in 100 MHz ticks (tools/kbench.py timeline)
  const unsigned tl_blk = blockIdx.y * gridDim.x + blockIdx.x;
  const bool tl = p.stamps && threadIdx.x == 0 && tl_blk < 1024;
  if (tl) p.stamps[64 + 2 * tl_blk] = __builtin_amdgcn_s_memrealtime();
  f16x8 bq[3][NT][2];
  f16x8 afc[MT][2], afn[MT][2];
  gload_patch(0);
  gload_b(bq[0], 0, 0);
  gload_b(bq[1], 0, 1);                            // nchunks * 9 >= 9 stages
  store_patch(smem, 0);
  __syncthreads();
  read_a(afc, smem, 0);
  if (stamp) p.stamps[1] = __builtin_amdgcn_s_memtime();

  for (int cc = 0; cc < nchunks; ++cc) {
    if (stamp && cc < 20) p.stamps[2 + cc] = __builtin_amdgcn_s_memtime();
    const unsigned char* pcur = smem + (cc & 1) * PATCH2_B;
    unsigned char* pnxt = smem + ((cc + 1) & 1) * PATCH2_B;
    const bool more = cc + 1 < nchunks;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap == 8) __syncthreads();               // next chunk's patch (stored at taps 2..7) is complete
      read_a(afn, tap < 8 ? pcur : pnxt, tap < 8 ? tap + 1 : 0);
      {                                            // past the last tile: a harmless reload of the last chunk
        const int t2 = tap + 2 >= 9 ? tap + 2 - 9 : tap + 2;
        const int c2 = tap + 2 >= 9 ? cc + 1 : cc;
        gload_b(bq[(tap + 2) % 3], c2 < nchunks ? c2 : nchunks - 1, t2);
      }
      if (tap == 0) gload_patch(more ? cc + 1 : cc);
      // the next patch is split and stored one float4 slot per stage (taps 2..7), inside the MFMA shadow
      if (tap >= 2 && tap < 2 + PV) store_slot(pnxt, tap - 2, more ? cc + 1 : cc);
#pragma unroll
      for (int term = 0; term < 3; ++term) {
        constexpr int PA[3] = {1, 0, 0};
        constexpr int PB[3] = {0, 1, 0};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afc[mt][PA[term]], bq[tap % 3][nt][PB[term]], acc[mt][nt],
                                                                 0, 0, 0);
      }
      // issue order inside the stage: one MFMA at a time, with the next stage's LDS reads / global loads and the
      // VALU + LDS-write work of the patch slot spread over the MFMA shadows
#pragma unroll
      for (int g = 0; g < 24; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (g < 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        else if (g < 18) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        if (g >= 12) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) afc[mt][pl] = afn[mt][pl];
    }
  }

  if (stamp) p.stamps[22] = __builtin_amdgcn_s_memtime();
  // epilogue: per image row, transposed through LDS so every lane moves float4s; scales divided out here
  const float* __restrict__ res = p.res;
  const float* __restrict__ cbp = p.cbias;
  float* __restrict__ yout = p.y;
  constexpr int TS = 64 + 4;
  float* stage = reinterpret_cast<float*>(smem) + wave * 32 * TS;
  const int c4 = lane & 15, prl = lane >> 4;
  const int nb = n0 + wn * 64 + c4 * 4;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (p.bias) bias4 = *reinterpret_cast<const f32x4*>(p.bias + nb);
  if (p.cbias_mode == 1) {
    const f32x4 c = *reinterpret_cast<const f32x4*>(cbp + (size_t)b * N + nb);
    bias4[0] += c[0]; bias4[1] += c[1]; bias4[2] += c[2]; bias4[3] += c[3];
  }
  // (issuing the residual / per-pixel bias loads of all four rows up front, or of row mt + 1 before row mt is stored,
  // were both measured slower: with a residual the launch moves 285 MB and the epilogue is bound by the memory
  // system's throughput, not by load latency; staggering the blocks' start does not help either)
  unsigned omax = 0;
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[mfma32_row(r, lane) * TS + nt * 32 + li] = (acc[mt][nt][r] * inv_x) * inv_w;
    const size_t rowbase = (((size_t)b * p.H + h0 + wm * MT + mt) * kW) * N + nb;
    f32x4 add[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) add[it] = bias4;
    if (p.cbias_mode == 2) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cbp + rowbase + (size_t)(it * 4 + prl) * N);
        add[it][0] += c[0]; add[it][1] += c[1]; add[it][2] += c[2]; add[it][3] += c[3];
      }
    }
    if (res) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(res + rowbase + (size_t)(it * 4 + prl) * N);
        add[it][0] += c[0]; add[it][1] += c[1]; add[it][2] += c[2]; add[it][3] += c[3];
      }
    }
    // the staging tile is private to this wave: only wave-level ordering is needed
    __builtin_amdgcn_s_waitcnt(0xc07f);            // lgkmcnt(0): this wave's ds_writes have landed
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(stage + (it * 4 + prl) * TS + c4 * 4);
      const f32x4 o = {a[0] + add[it][0], a[1] + add[it][1], a[2] + add[it][2], a[3] + add[it][3]};
      *reinterpret_cast<f32x4*>(yout + rowbase + (size_t)(it * 4 + prl) * N) = o;
#pragma unroll
      for (int e = 0; e < 4; ++e) omax = max(omax, __float_as_uint(o[e]) & 0x7fffffffu);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }
  if (p.ymax) {   // this block is partial maximum number (row tile, cout block) of image b; unused entries zeroed
    const int part = (h0 / TR2) * gridDim.y + blockIdx.y, nparts = tiles_per_img * gridDim.y;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) omax = max(omax, (unsigned)__shfl_xor((int)omax, o, 64));
    __syncthreads();
    unsigned* ured = reinterpret_cast<unsigned*>(smem);
    if (lane == 0) ured[wave] = omax;
    __syncthreads();
    if (tid == 0) p.ymax[b * 16 + part] = max(max(ured[0], ured[1]), max(ured[2], ured[3]));
    if (part == 0 && tid >= nparts && tid < 16) p.ymax[b * 16 + tid] = 0u;
  }
  if (stamp) { p.stamps[23] = __builtin_amdgcn_s_memtime(); p.stamps[31] = __builtin_amdgcn_s_memrealtime(); }
  if (tl) p.stamps[65 + 2 * tl_blk] = __builtin_amdgcn_s_memrealtime();
}

}  // namespace

// Eligibility: W == 32, H % 8 == 0, C % 16 == 0, N % 128 == 0 (the ResBlock convolutions); everything else goes
// through mulan_conv3x3_fwd.  xmax = mulan_absmax_rows(x, B rows); wp / wmax from mulan_conv3x3_pack_f16x3.
MULAN_API size_t mulan_conv3x3_planes_bytes(int B, int H, int W, int C) { return (size_t)B * H * W * C * 4; }

// The shape every forward entry point takes: 32 pixels wide, whole 8-row tiles, whole blocks of 128 couts.  below_2gib:
// the launch addresses the input (or its planes) with 32-bit byte offsets; with_ymax: it writes the [B][16] maxima array,
// one slot per block of an image.  What else an entry point requires (its grid of C, pointers, the GroupNorm and
// statistics rules) stands in the entry point.
static bool conv_fwd_shape_ok(int B, int H, int W, int C, int N, bool below_2gib, bool with_ymax) {
  if (W != kW || H % TR2 != 0 || B <= 0 || C <= 0 || N <= 0 || N % BN != 0) return false;
  if (below_2gib && (size_t)B * H * W * C * 4 >= 0x80000000ull) return false;
  return !(with_ymax && (H / TR2) * (N / BN) > kMaxParts);
}

// xs (optional, mulan_conv3x3_planes_bytes): receives the split planes of x, the input format of
// mulan_conv3x3_wgrad_f16x3_planes.
// _alone: the same launch with the caller's word that no other stream's kernels share the chip (alone != 0: a forward
// pass, an evaluator, the ODE likelihood's vector-Jacobian product): small launches may then run as k-split blocks
// (conv3x3_f16x3_v3.hip, KS).  mulan_conv3x3_fwd_f16x3 = alone 0.
static int conv3x3_fwd_f16x3_impl(const float* x, const unsigned* xmax, const void* wp, const unsigned* wmax,
                                  const float* bias, const float* cbias, int cbias_mode, const float* res, float* y,
                                  void* xs, unsigned* ymax, int alone, int B, int H, int W, int C, int N,
                                  hipStream_t stream) {
  if (!conv_fwd_shape_ok(B, H, W, C, N, xs != nullptr, ymax != nullptr) || C % CK != 0 || !xmax || !wmax)
    return (int)hipErrorInvalidValue;
  const ConvArgsH a{.x = x, .xmax = xmax, .wp = static_cast<const unsigned char*>(wp), .wmax = wmax, .bias = bias,
                    .cbias = cbias, .res = res, .y = y, .B = B, .H = H, .C = C, .N = N,
                    .cbias_mode = cbias ? cbias_mode : 0, .stamps = g_mulan_debug_buffer,
                    .xs = static_cast<unsigned char*>(xs), .ymax = ymax, .alone = alone};
  // default: the 16x16x32 / two-blocks-per-CU kernel (conv3x3_f16x3_v3.hip); otherwise (C % 32 != 0, a tensor of 2 GiB,
  // or tune[3] = 2, the dev A/B switch -- any non-zero value acts alike) the 32x32x16 one-block-per-CU kernel above
  if (g_mulan_tune[3] == 0 && mulan_conv3x3_f16x3_v3_eligible(H, C, N) && (size_t)B * H * W * C * 4 < 0x80000000ull)
    return mulan_launch_conv3x3_f16x3_v3(a, stream);
  static bool configured2 = false;
  if (!configured2) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_f16x3_v2_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_B);
    if (e != hipSuccess) return (int)e;
    configured2 = true;
  }
  hipLaunchKernelGGL(conv3x3_f16x3_v2_kernel, dim3(B * (H / TR2), N / BN), dim3(256), SMEM2_B, stream, a);
  MULAN_CHECK_LAUNCH();
}

MULAN_API int mulan_conv3x3_fwd_f16x3(const float* x, const unsigned* xmax, const void* wp, const unsigned* wmax,
                                      const float* bias, const float* cbias, int cbias_mode, const float* res,
                                      float* y, void* xs, unsigned* ymax, int B, int H, int W, int C, int N,
                                      hipStream_t stream) {
  return conv3x3_fwd_f16x3_impl(x, xmax, wp, wmax, bias, cbias, cbias_mode, res, y, xs, ymax, 0, B, H, W, C, N, stream);
}
MULAN_API int mulan_conv3x3_fwd_f16x3_alone(const float* x, const unsigned* xmax, const void* wp, const unsigned* wmax,
                                            const float* bias, const float* cbias, int cbias_mode, const float* res,
                                            float* y, void* xs, unsigned* ymax, int alone, int B, int H, int W, int C,
                                            int N, hipStream_t stream) {
  return conv3x3_fwd_f16x3_impl(x, xmax, wp, wmax, bias, cbias, cbias_mode, res, y, xs, ymax, alone, B, H, W, C, N,
                                stream);
}

// The forward convolution fed with the split planes of its input (mulan_groupnorm_fwd_planes writes them; xmax is the
// [B][16] array that kernel filled with the bound the planes are scaled with).  Same epilogue and by-products as
// mulan_conv3x3_fwd_f16x3, minus the plane output -- the input already is one, for the weight-gradient kernel too.
// Needs the shapes of the two-blocks-per-CU kernel: H % 8 == 0, C % 32 == 0, N % 128 == 0.
// _stats: ystats (optional) receives the partial sums of y and y^2 per (image, row tile of this launch, channel quad),
// [B][H / mulan_conv3x3_f16x3_tile_rows(B, H, N, ymax != NULL)][N / 4][2] -- what mulan_groupnorm_fwd_stream forms the
// statistics of the NEXT GroupNorm from (norm2 behind conv1, the next block's norm1 behind conv2: model_vdm.py:622-644).
// alone != 0: the caller has no other stream's kernels on the chip during this launch (a forward pass, an evaluator):
// launches of at most 256 blocks then run as k-split blocks of eight waves (conv3x3_f16x3_v3.hip, KS).
MULAN_API int mulan_conv3x3_fwd_f16x3_planes_in_stats(const void* xplanes, const unsigned* xmax, const void* wp,
                                                      const unsigned* wmax, const float* bias, const float* cbias,
                                                      int cbias_mode, const float* res, float* y, unsigned* ymax,
                                                      float* ystats, int alone, int B, int H, int W, int C, int N,
                                                      hipStream_t stream) {
  if (!conv_fwd_shape_ok(B, H, W, C, N, true, ymax != nullptr) || !mulan_conv3x3_f16x3_v3_eligible(H, C, N) || !xplanes ||
      !xmax || !wmax)
    return (int)hipErrorInvalidValue;
  const ConvArgsH a{.xmax = xmax, .wp = static_cast<const unsigned char*>(wp), .wmax = wmax, .bias = bias, .cbias = cbias,
                    .res = res, .y = y, .B = B, .H = H, .C = C, .N = N, .cbias_mode = cbias ? cbias_mode : 0,
                    .stamps = g_mulan_debug_buffer, .ymax = ymax, .xplanes = static_cast<const unsigned char*>(xplanes),
                    .ystats = ystats, .alone = alone};
  return mulan_launch_conv3x3_f16x3_v3(a, stream);
}

MULAN_API int mulan_conv3x3_fwd_f16x3_planes_in(const void* xplanes, const unsigned* xmax, const void* wp,
                                                const unsigned* wmax, const float* bias, const float* cbias,
                                                int cbias_mode, const float* res, float* y, unsigned* ymax, int B, int H,
                                                int W, int C, int N, hipStream_t stream) {
  return mulan_conv3x3_fwd_f16x3_planes_in_stats(xplanes, xmax, wp, wmax, bias, cbias, cbias_mode, res, y, ymax, nullptr, 0,
                                                 B, H, W, C, N, stream);
}

// y = conv3x3(act(GroupNorm([x1 | x2]))) + bias + cbias + res with the normalisation done inside the convolution's patch
// fill (ResnetBlock norm1 + swish -> conv1, norm2 + swish -> conv2 where no dropout is drawn: ldm/model_vdm.py:622-656 in
// the evaluators and the sampler): x1 (, x2: equal widths) are the fp32 inputs of the GroupNorm.
//  * xstats1 == NULL: mean / rstd / bound are what mulan_groupnorm_stats left; the result is, bit for bit, that of
//    mulan_groupnorm_fwd_planes + mulan_conv3x3_fwd_f16x3_planes_in.
//  * xstats1 (, xstats2) given: the partial sums the convolutions that PRODUCED x1 (, x2) left through their `ystats`
//    ([B][xstats_tiles][C1 / 4][2]: sum and sum of squares per image, row tile and channel quad; xstats_tiles = H / the
//    producer's tile rows, mulan_conv3x3_f16x3_tile_rows): every block forms mean / rstd
//    and the bound itself -- no pass over x in front of the convolution at all -- and mean / rstd / bound are OUTPUTS (for
//    a later backward pass).  Same formulas, another summation order: statistics agree to fp32 rounding.
//  * ystats (optional, [B][H / mulan_conv3x3_f16x3_tile_rows(B, H, N, ymax != NULL)][N / 4][2]): this launch's partial
//    sums of y for the next GroupNorm.
// The normalised tensor is not written unless yplanes_out (optional, mulan_conv3x3_planes_bytes(B, 32, 32, C1 + C2)
// bytes) asks for it as the weight-gradient kernel's operand.
MULAN_API int mulan_conv3x3_fwd_f16x3_gn_in(const float* x1, const float* x2, int C1, int C2, const float* gamma,
                                            const float* beta, float* mean, float* rstd, int G, int act, float eps,
                                            unsigned* bound, const float* xstats1, const float* xstats2, int xstats_tiles,
                                            const void* wp, const unsigned* wmax, const float* bias, const float* cbias,
                                            int cbias_mode, const float* res, float* y, unsigned* ymax, float* ystats,
                                            void* yplanes_out, int B, int H, int W, int N, hipStream_t stream) {
  const int C = C1 + (x2 ? C2 : 0);
  if (!conv_fwd_shape_ok(B, H, W, C, N, true, ymax != nullptr) || !mulan_conv3x3_f16x3_v3_eligible(H, C, N) || G <= 0 ||
      !x1 || !gamma || !beta || !mean || !rstd || !bound || !wmax || (x2 && C2 != C1) || C % G != 0 || (C / G) % 4 != 0 ||
      C > 512 || (xstats1 && x2 && !xstats2) || (ystats && yplanes_out) ||
      (xstats1 && xstats_tiles != H / 8 && xstats_tiles != H / 4 && xstats_tiles != H / 2))
    return (int)hipErrorInvalidValue;
  // alone = 1: forward-only paths (and the forward pass of a train step)
  const ConvArgsH a{.x = x1, .xmax = bound, .wp = static_cast<const unsigned char*>(wp), .wmax = wmax, .bias = bias,
                    .cbias = cbias, .res = res, .y = y, .B = B, .H = H, .C = C, .N = N,
                    .cbias_mode = cbias ? cbias_mode : 0, .stamps = g_mulan_debug_buffer,
                    .xs = static_cast<unsigned char*>(yplanes_out), .ymax = ymax, .x2 = x2, .gn_mean = mean,
                    .gn_rstd = rstd, .gn_gamma = gamma, .gn_beta = beta, .gn_act = act, .gn_groups = G, .ystats = ystats,
                    .xstats = xstats1, .xstats2 = xstats2, .gn_mean_out = xstats1 ? mean : nullptr,
                    .gn_rstd_out = xstats1 ? rstd : nullptr, .xmax_out = xstats1 ? bound : nullptr, .gn_eps = eps,
                    .xstats_tiles = xstats_tiles, .alone = 1};
  return mulan_launch_conv3x3_f16x3_v3(a, stream);
}

// Image rows per block (8, 4 or 2) of the two-blocks-per-CU convolution kernel for a launch of B images with N output
// channels: the tallest tile that still gives the launch two blocks per CU.  `ystats` of mulan_conv3x3_fwd_f16x3_gn_in
// holds H / rows row tiles per image ([B][H / rows][N / 4][2]): the caller sizes it with this function and hands the count
// on as `xstats_tiles`.  with_ymax: the launch also writes the maxima array (16 partials per image limit the tile count).
MULAN_API int mulan_conv3x3_f16x3_tile_rows(int B, int H, int N, int with_ymax) {
  if (B <= 0 || H % 8 != 0 || N <= 0 || N % BN != 0) return 8;
  return mulan_conv3x3_f16x3_v3_tile_rows(B, H, N, with_ymax != 0);
}
