// Exact first and second moments of a set of uint8 rows on the int8 matrix cores: for x [N, D] and c = x - 128 as int8,
//   sum[j] = sum_i c[i, j]          gram[j, k] = sum_i c[i, j] c[i, k]
// as int64, the Gram product X^T X whose contraction index is the SAMPLE, the strided index of memory.
//
// Arithmetic.  Bytes are recentred to int8 (x - 128 is x ^ 0x80 on the bit pattern).  |c c| <= 2^14, so the int32
// accumulators of v_mfma_i32_32x32x32_i8 are exact for at most 131 071 rows; a block hands its int32 tile over to 64-bit
// sums after FLUSH_ROWS = 65 536 rows at the latest (2^30 per entry, 2^23 per column sum).  Every intermediate is an
// integer: nothing below depends on the tile schedule, the number of slices or the device, and there are no atomics.
//
// Geometry.  Only the T (T + 1) / 2 tiles of 128 x 128 columns with tile_j <= tile_k are computed (T = ceil(D / 128)); 256
// threads, wave w owns the 64 x 64 quadrant (w >> 1, w & 1) as 2 x 2 accumulators of 32 x 32.  The N rows are cut into
// chunks of C = 64 samples and the chunks into `splits` contiguous slices (slice s: chunks [s n / S, (s + 1) n / S), which
// may be empty).  Block b of a 1-D grid is tile b % tiles of slice b / tiles: neighbouring blocks walk the same rows at the
// same pace, so a chunk of x is fetched from HBM once per wave of co-resident blocks and found in L2 / the Infinity Cache
// by the others.  A block's int64 tile goes to workspace [slice][tile][128][128], the column sums (taken by the diagonal
// tiles, v_dot4_i32_i8 against ones) to workspace [slice][D]; the fold launch adds the slices in 64 bits and writes
// gram[j][k] and, from the same total, its mirror gram[k][j].
//
// Fill.  An MFMA operand wants, per lane, 16 consecutive k-bytes of one output index; here k is the sample and the
// output index the column, so every operand is the transpose of what memory holds.  Both operands of a product come
// from the same chunk, so any order of the samples inside a 16-byte piece will do as long as both use it.
//   fetch     a thread owns 4 columns x 16 samples of a panel: 16 dwords from 16 consecutive rows.  The 32 lanes of a
//             half-wave run along a row (one 128-byte segment per row and load); waves 0, 1 fill the tile_j panel, waves
//             2, 3 the tile_k panel, and a diagonal tile stages one panel only.  A row past N or a column past D is
//             zero-filled by index, never read, AFTER the recentring: a zero c adds nothing to gram or sum.  The fetch of
//             chunk c + 1 is issued before the MFMAs of chunk c.
//   transpose four 4 x 4 byte transposes in registers, two v_perm_b32 stages of four each: per column 16 samples in
//             four dwords.
//   store     one ds_write_b128 per column into the [column][sample] image: column q = 4 g + c lies at g GS + c RS with
//             RS = 64 (the chunk, unpadded) and GS = 4 RS + 16 = 272.  The 8 consecutive lanes one LDS cycle of a 16-byte
//             store serves are 8 groups g at one c: 17 g 16-byte slots apart, 8 different slots of the 8 (32 banks).
//   read      lane l reads column l & 31 of a 32-column block, bytes 32 kk + 16 (l >> 5) ... + 15 (ds_read_b128).  Its 16
//             lanes per LDS cycle are four whole groups g (0, 3, 5, 6 or 1, 2, 4, 7 of the block, in either half-wave) at
//             c = 0..3: slots 17 g + 4 c mod 16 = g + 4 c mod 16, 16 different slots of the 16 (64 banks).
// LDS: 2 panels x 32 groups x 272 B = 17 408 B (the column-sum hand-over reuses the first 2 KB).
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256;
constexpr int TILE = 128;               // columns per tile side
constexpr int KC = 64;                  // C: samples per chunk
constexpr int RS = KC;                  // bytes per column of the LDS image
constexpr int GS = 4 * RS + 16;         // bytes per group of 4 columns
constexpr int PANEL_BYTES = (TILE / 4) * GS;
constexpr int TILE_ELEMS = TILE * TILE;
constexpr int FLUSH_ROWS = 65536;       // rows after which the int32 accumulators are handed over to the 64-bit sums
constexpr int FLUSH_CHUNKS = FLUSH_ROWS / KC;
constexpr int MIN_D = 64, MAX_D = 4096;
constexpr int MAX_N = 1 << 24;
constexpr int MAX_SPLITS = 4096;
constexpr int AUTO_BLOCKS = 1024;       // blocks the library aims for when it chooses the slices (a constant, not the device's)
constexpr int AUTO_MAX_SPLITS = 64;
constexpr int FOLD_SUB = 32;            // the fold launch works on 32 x 32 pieces of a tile
static_assert((long long)FLUSH_ROWS * 128 * 128 <= 0x7fffffffll, "an int32 accumulator holds FLUSH_ROWS products of at most 2^14");
static_assert(FLUSH_ROWS % KC == 0 && GS % 16 == 0 && (GS / 16) % 2 == 1, "chunks per hand-over; odd slot stride of a group");
static_assert(4 * TILE * 4 <= PANEL_BYTES, "the column-sum hand-over fits the first panel");

struct MomentsArgs {
  const unsigned char* x;
  int N, D, splits, T, tiles, chunks;
  long long* ws_tiles;                  // [splits][tiles][128][128]
  long long* ws_sum;                    // [splits][D]
};

// byte offset of column q of a panel in the LDS image
__device__ __forceinline__ int col_off(int q) { return (q >> 2) * GS + (q & 3) * RS; }

// t[c] = byte c of d[0..3]: a 4 x 4 byte transpose.  Which of d[0..3] lands in which byte of t[c] is the same for every c.
__device__ __forceinline__ void transpose4(const int* d, int* t) {
  const int lo01 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400), hi01 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602);
  const int lo23 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400), hi23 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602);
  t[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100);
  t[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302);
  t[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100);
  t[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302);
}

// 16 rows from `row` on, 4 columns at `col`: recentred, zero outside the array
__device__ __forceinline__ void fetch_unit(const unsigned char* x, int row, int N, size_t D, int col, bool col_ok, int* d) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int v = 0;
    if (col_ok && row + r < N) v = *reinterpret_cast<const int*>(x + (size_t)(row + r) * D + col) ^ (int)0x80808080;
    d[r] = v;
  }
}

__global__ __launch_bounds__(NT, 2) void set_moments_u8_kernel(MomentsArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * PANEL_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int t = blockIdx.x % p.tiles;
  const int tile = t, s = blockIdx.x / p.tiles;
  int tj = 0;
  while (t >= p.T - tj) {
    t -= p.T - tj;
    ++tj;
  }
  const int tk = tj + t;
  const bool diag = tj == tk;
  const int c_begin = (int)((long long)s * p.chunks / p.splits), c_end = (int)((long long)(s + 1) * p.chunks / p.splits);
  const size_t D = (size_t)p.D;

  unsigned char* sA = smem;
  unsigned char* sB = diag ? smem : smem + PANEL_BYTES;

  // fill: panel tid >> 7, group of 4 columns tid & 31, 16 samples from 16 ((tid >> 5) & 3) on
  const int fpanel = tid >> 7, fg = tid & 31, fq = (tid >> 5) & 3;
  const bool filler = fpanel == 0 || !diag;
  const int fcol = (fpanel ? tk : tj) * TILE + 4 * fg;
  const bool fcol_ok = filler && fcol < p.D;
  unsigned char* fdst = smem + fpanel * PANEL_BYTES + fg * GS + fq * 16;
  const bool summer = diag && fpanel == 0;
  // fragments: column lane & 31 of a 32-column block, bytes 16 (lane >> 5) ... of a 32-byte k-step
  const int frow = lane & 31, fk = (lane >> 5) * 16;

  i32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0;
  int csum[4] = {0, 0, 0, 0};

  long long* wt = p.ws_tiles + ((size_t)s * p.tiles + tile) * TILE_ELEMS;
  long long* wsum = p.ws_sum + (size_t)s * D + (size_t)tj * TILE;

  // hand-over of the int32 accumulators to the block's 64-bit tile and column sums; all threads call it together
  auto flush = [&](bool add) {
    // accumulator register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
    long long* w = wt;
    asm volatile("" : "+v"(w));                               // the 64 addresses are made here, not kept across the K-loop
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        long long* dst0 = w + (wm * 64 + m * 32 + 4 * (lane >> 5)) * TILE + wn * 64 + n * 32 + (lane & 31);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          long long* dst = dst0 + ((e & 3) + 8 * (e >> 2)) * TILE;
          const long long v = (long long)acc[m][n][e];
          *dst = add ? *dst + v : v;
          acc[m][n][e] = 0;
        }
        __builtin_amdgcn_sched_barrier(0);                    // one accumulator at a time: the hand-over is rare, registers are not
      }
    if (diag) {                                               // block-uniform
      int* sS = reinterpret_cast<int*>(smem);                 // [4][TILE]; the K-loop left the image behind a barrier
      if (summer) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          sS[fq * TILE + 4 * fg + c] = csum[c];
          csum[c] = 0;
        }
      }
      __syncthreads();
      if (tid < TILE && tj * TILE + tid < p.D) {
        const long long v = (long long)sS[tid] + sS[TILE + tid] + sS[2 * TILE + tid] + sS[3 * TILE + tid];
        wsum[tid] = add ? wsum[tid] + v : v;
      }
      __syncthreads();
    }
  };

  int d[16];
  if (c_begin < c_end) fetch_unit(p.x, c_begin * KC + fq * 16, p.N, D, fcol, fcol_ok, d);
  bool wrote = false;
  int since = 0;
  for (int c = c_begin; c < c_end; ++c) {
    if (filler) {
      int tr[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) transpose4(d + 4 * q, tr[q]);
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const i32x4 v = {tr[0][cc], tr[1][cc], tr[2][cc], tr[3][cc]};
        *reinterpret_cast<i32x4*>(fdst + cc * RS) = v;
        if (summer) {
#pragma unroll
          for (int q = 0; q < 4; ++q) csum[cc] = __builtin_amdgcn_sdot4(v[q], 0x01010101, csum[cc], false);
        }
      }
    }
    __syncthreads();
    if (c + 1 < c_end) fetch_unit(p.x, (c + 1) * KC + fq * 16, p.N, D, fcol, fcol_ok, d);
#pragma unroll
    for (int kk = 0; kk < KC / 32; ++kk) {
      i32x4 fa[2], fb[2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
        fa[m] = *reinterpret_cast<const i32x4*>(sA + col_off(wm * 64 + m * 32 + frow) + kk * 32 + fk);
#pragma unroll
      for (int n = 0; n < 2; ++n)
        fb[n] = *reinterpret_cast<const i32x4*>(sB + col_off(wn * 64 + n * 32 + frow) + kk * 32 + fk);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
    __syncthreads();
    if (++since == FLUSH_CHUNKS && c + 1 < c_end) {
      flush(wrote);
      wrote = true;
      since = 0;
    }
  }
  flush(wrote);                                               // an empty slice writes zeros
}

// Blocks [0, 16 tiles): one 32 x 32 piece of a tile: the slices' totals go to gram[j][k] and, through LDS so that both
// stores run along rows, to the mirror gram[k][j].  The blocks after them add the slices' column sums, 256 columns each.
__global__ __launch_bounds__(NT) void set_moments_u8_fold_kernel(MomentsArgs p, long long* __restrict__ sum,
                                                                 long long* __restrict__ gram, int accumulate) {
  __shared__ long long piece[FOLD_SUB][FOLD_SUB + 1];
  const int tid = threadIdx.x;
  constexpr int PIECES = (TILE / FOLD_SUB) * (TILE / FOLD_SUB);
  const size_t D = (size_t)p.D;
  if ((int)blockIdx.x >= p.tiles * PIECES) {
    const int col = ((int)blockIdx.x - p.tiles * PIECES) * NT + tid;
    if (col < p.D) {
      long long v = accumulate ? sum[col] : 0;
      for (int s = 0; s < p.splits; ++s) v += p.ws_sum[(size_t)s * D + col];
      sum[col] = v;
    }
    return;
  }
  const int tile = blockIdx.x / PIECES, sub = blockIdx.x % PIECES;
  const int sj = sub / (TILE / FOLD_SUB), sk = sub % (TILE / FOLD_SUB);
  int t = tile, tj = 0;
  while (t >= p.T - tj) {
    t -= p.T - tj;
    ++tj;
  }
  const int tk = tj + t;
  const int j0 = tj * TILE + sj * FOLD_SUB, k0 = tk * TILE + sk * FOLD_SUB;
  for (int e = tid; e < FOLD_SUB * FOLD_SUB; e += NT) {
    const int jj = e / FOLD_SUB, kk = e % FOLD_SUB;
    const long long* src = p.ws_tiles + (size_t)tile * TILE_ELEMS + (sj * FOLD_SUB + jj) * TILE + sk * FOLD_SUB + kk;
    long long v = 0;
    for (int s = 0; s < p.splits; ++s) v += src[(size_t)s * p.tiles * TILE_ELEMS];
    piece[jj][kk] = v;
    if (j0 + jj < p.D && k0 + kk < p.D) {
      long long* dst = gram + (size_t)(j0 + jj) * D + k0 + kk;
      *dst = accumulate ? *dst + v : v;
    }
  }
  if (tj == tk) return;                                       // a diagonal tile holds both triangles itself
  __syncthreads();
  for (int e = tid; e < FOLD_SUB * FOLD_SUB; e += NT) {
    const int kk = e / FOLD_SUB, jj = e % FOLD_SUB;
    if (j0 + jj < p.D && k0 + kk < p.D) {
      long long* dst = gram + (size_t)(k0 + kk) * D + j0 + jj;
      *dst = accumulate ? *dst + piece[jj][kk] : piece[jj][kk];
    }
  }
}

bool shape_ok(int N, int D, int splits) {
  return N >= 1 && N <= MAX_N && D >= MIN_D && D <= MAX_D && D % 64 == 0 && splits >= 0 && splits <= MAX_SPLITS;
}

int tiles_of(int D) {
  const int T = (D + TILE - 1) / TILE;
  return T * (T + 1) / 2;
}

// the library's choice: enough slices for AUTO_BLOCKS blocks, no more than chunks
int auto_splits(int N, int D) {
  const int tiles = tiles_of(D), chunks = (N + KC - 1) / KC;
  int s = (AUTO_BLOCKS + tiles - 1) / tiles;
  if (s > AUTO_MAX_SPLITS) s = AUTO_MAX_SPLITS;
  if (s > chunks) s = chunks;
  return s < 1 ? 1 : s;
}

}  // namespace

MULAN_API size_t mulan_set_moments_u8_workspace(int N, int D, int splits) {
  if (!shape_ok(N, D, splits)) return 0;
  const size_t S = (size_t)(splits ? splits : auto_splits(N, D));
  return S * ((size_t)tiles_of(D) * TILE_ELEMS + (size_t)D) * sizeof(long long);
}

MULAN_API int mulan_set_moments_u8(const unsigned char* x, int N, int D, int accumulate, int splits, long long* sum,
                                   long long* gram, void* workspace, hipStream_t stream) {
  if (!x || !sum || !gram || !workspace) return (int)hipErrorInvalidValue;
  if (!shape_ok(N, D, splits) || (accumulate != 0 && accumulate != 1)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)x & 15) || ((uintptr_t)sum & 7) || ((uintptr_t)gram & 7) || ((uintptr_t)workspace & 7))
    return (int)hipErrorInvalidValue;
  const int S = splits ? splits : auto_splits(N, D);
  const int T = (D + TILE - 1) / TILE, tiles = tiles_of(D);
  if ((long long)tiles * S > 0x7fffffffll) return (int)hipErrorInvalidValue;
  long long* ws = static_cast<long long*>(workspace);
  MomentsArgs a{x, N, D, S, T, tiles, (N + KC - 1) / KC, ws, ws + (size_t)S * tiles * TILE_ELEMS};
  constexpr int PIECES = (TILE / FOLD_SUB) * (TILE / FOLD_SUB);
  hipLaunchKernelGGL(set_moments_u8_kernel, dim3((unsigned)(tiles * S)), dim3(NT), 0, stream, a);
  hipLaunchKernelGGL(set_moments_u8_fold_kernel, dim3((unsigned)(tiles * PIECES + (D + NT - 1) / NT)), dim3(NT), 0, stream,
                     a, sum, gram, accumulate);
  MULAN_CHECK_LAUNCH();
}
