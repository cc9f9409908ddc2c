// Exact k nearest neighbours between two sets of uint8 rows on the int8 matrix cores: for every row i of q [Q, D] the k
// smallest squared Euclidean distances to the rows j of r [N, D], with their indices, as integers.
//
// Arithmetic.  Bytes are recentred to int8 (x - 128 is x ^ 0x80 on the bit pattern; distances do not change), and
//   d2(i, j) = |a_i|^2 + |b_j|^2 - 2 a_i . b_j
// with a . b from v_mfma_i32_32x32x32_i8 (int32 accumulation) and the norms from v_dot4_i32_i8, also int32.  Every
// intermediate is an exact integer: |a . b| <= D 128^2 = 2^28 and d2 <= D 255^2 < 2^31 at D <= 16384, the most accepted.
//
// Order.  A candidate is the 64-bit key (d2 << 32) | global index (global index = j + idx_base >= 0), so "smaller distance,
// then smaller index" is one signed comparison and no two candidates compare equal; the empty slot is the largest key,
// (INT32_MAX, -1).  The k smallest keys of a set are then one list whatever order they were met in: nothing below depends
// on the tile schedule, the number of slices or the device, and there are no atomics.
//
// Geometry.  Tile T = 128 queries x U = 128 references, K-chunk C = 64 bytes, 256 threads: wave w owns the 64 x 64
// quadrant (w >> 1, w & 1) as 2 x 2 accumulators of 32 x 32.  Block b of a 1-D grid is query tile b % qtiles of slice
// b / qtiles; the reference tiles are cut into `splits` contiguous slices (slice s: tiles [s n / S, (s + 1) n / S), which
// may be empty).  Neighbouring blocks are neighbouring query tiles of one slice, walking the same reference tiles in the
// same order at the same pace, so a reference tile is fetched from HBM once per wave of co-resident blocks and found in
// L2 / the Infinity Cache by the others.
//   K-loop    each thread fetches two 16-byte pieces of the query chunk and two of the reference chunk into registers
//             (guarded: a row past Q or N is zero-filled, never read), flips the sign bits, adds the pieces' squared norms
//             to its partial sums and stores them to LDS rows of 80 bytes; the fetch of chunk c + 1 is issued before the
//             MFMAs of chunk c.  Lane l reads row l & 31, bytes 32 kk + 16 (l >> 5) ... + 15 of both operands for k-step
//             kk: the same k order on both sides, so the product does not depend on the order inside a lane.
//   epilogue  the four lanes of a row add their norm partials (xor 1, 2); d2 goes to a [128][130] int32 LDS tile that
//             overlays the staging buffers (stride 130: the scan below and this store are both at most 2-way conflicted).
//   scan      thread t owns row t >> 1 and the columns of parity t & 1, and keeps a sorted list of k keys in LDS.  A
//             column past N, and the pair excluded by self_offset, are skipped BY INDEX; a key enters the list by
//             insertion only if it is below the list's last.  In radius mode the same loop ORs d2 <= radius2[j].
//   end       the odd thread's list is inserted into the even thread's, which goes to workspace [slice][Q][k]; the
//             coverage bit to workspace bytes [slice][Q].
// The fold launch (one thread per query) copies the previous lists to slot `splits` of the workspace when accumulate is
// set, then writes output slot t = the smallest key of all slots that is above output slot t - 1: the merged list, and
// the OR of the coverage bytes (with the previous one when accumulate is set).
//
// LDS: 66 560 B tile + 1 536 B norms and radii + 256 k x 8 B lists (10 KB at k = 5: two blocks per CU; 32 KB at k = 16).
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef long long knn_key;

constexpr int NT = 256;
constexpr int TQ = 128;                 // T: queries per tile
constexpr int TR = 128;                 // U: references per tile
constexpr int KC = 64;                  // C: bytes of D per K-chunk
constexpr int ROWB = KC + 16;           // bytes per staged row
constexpr int D2S = TR + 2;             // words per row of the d2 tile
constexpr int STAGE_BYTES = (TQ + TR) * ROWB;
constexpr int TILE_BYTES = TQ * D2S * 4;
constexpr int FIXED_BYTES = TILE_BYTES + (TQ + 2 * TR) * 4;
constexpr int MAX_K = 16;
constexpr int MAX_D = 16384;
constexpr int MAX_SPLITS = 4096;
constexpr int AUTO_BLOCKS = 4096;       // blocks the library aims for when it chooses the slices (a constant, not the device's)
constexpr int AUTO_MAX_SPLITS = 64;
constexpr knn_key EMPTY = (knn_key)(((unsigned long long)0x7fffffffu << 32) | 0xffffffffu);
static_assert(STAGE_BYTES <= TILE_BYTES, "the d2 tile overlays the staging buffers");
static_assert(FIXED_BYTES + NT * MAX_K * 8 <= 160 * 1024, "LDS");

struct KnnArgs {
  const unsigned char* q; const unsigned char* r;
  int Q, N, D, k, idx_base, self_offset, splits, qtiles, rtiles;
  const int* radius2;                   // [N] or null
  knn_key* ws_keys;                       // [splits + 1][Q][k]
  unsigned char* ws_cov;                // [splits][Q]
};

__device__ __forceinline__ knn_key make_key(int d2, int gidx) {
  return (knn_key)(((unsigned long long)(unsigned)d2 << 32) | (unsigned)gidx);
}

// sorted insertion of a key that is below L[k - 1]
__device__ __forceinline__ void list_insert(knn_key* L, int k, knn_key key) {
  int p = k - 1;
  while (p > 0 && L[p - 1] > key) {
    L[p] = L[p - 1];
    --p;
  }
  L[p] = key;
}

__device__ __forceinline__ i32x4 fetch16(const unsigned char* base, int row, int rows, size_t D, int off) {
  i32x4 v = {0, 0, 0, 0};
  if (row < rows) v = *reinterpret_cast<const i32x4*>(base + (size_t)row * D + off);
  return v ^ (int)0x80808080;
}

__device__ __forceinline__ int norm16(i32x4 v, int acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_sdot4(v[j], v[j], acc, false);
  return acc;
}

__global__ __launch_bounds__(NT) void knn_u8_kernel(KnnArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sA = smem;                                   // [TQ][ROWB]   } during the K-loop
  unsigned char* sB = smem + TQ * ROWB;                       // [TR][ROWB]   }
  int* sD2 = reinterpret_cast<int*>(smem);                    // [TQ][D2S]    after it
  int* sNA = reinterpret_cast<int*>(smem + TILE_BYTES);       // [TQ]
  int* sNB = sNA + TQ;                                        // [TR]
  int* sRad = sNB + TR;                                       // [TR]
  knn_key* lists = reinterpret_cast<knn_key*>(smem + FIXED_BYTES);  // [NT][k]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int qt = blockIdx.x % p.qtiles, s = blockIdx.x / p.qtiles;
  const int q0 = qt * TQ;
  const int t_begin = (int)((long long)s * p.rtiles / p.splits), t_end = (int)((long long)(s + 1) * p.rtiles / p.splits);
  const int k = p.k;
  const size_t D = (size_t)p.D;
  const int chunks = p.D / KC;

  knn_key* mine = lists + tid * k;
  for (int j = 0; j < k; ++j) mine[j] = EMPTY;
  knn_key last = EMPTY;
  bool cov = false;

  // staging: piece tid + 256 i is bytes 16 (piece & 3) ... of row piece >> 2
  const int srow0 = tid >> 2, srow1 = srow0 + 64, spart = (tid & 3) * 16;
  // fragments: row lane & 31 of a 32-row block, bytes 16 (lane >> 5) ... of a 32-byte k-step
  const int frow = lane & 31, fk = (lane >> 5) * 16;
  // scan
  const int row = tid >> 1, par = tid & 1;
  const int gi = q0 + row;
  const long long self_idx = p.self_offset >= 0 ? (long long)gi + p.self_offset : -1;

  for (int t = t_begin; t < t_end; ++t) {
    const int r0 = t * TR;
    const bool first = t == t_begin;
    i32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][n][e] = 0;
    int na0 = 0, na1 = 0, nb0 = 0, nb1 = 0;
    i32x4 a0 = fetch16(p.q, q0 + srow0, p.Q, D, spart), a1 = fetch16(p.q, q0 + srow1, p.Q, D, spart);
    i32x4 b0 = fetch16(p.r, r0 + srow0, p.N, D, spart), b1 = fetch16(p.r, r0 + srow1, p.N, D, spart);
    if (p.radius2 && tid < TR) sRad[tid] = r0 + tid < p.N ? p.radius2[r0 + tid] : 0;
    for (int c = 0; c < chunks; ++c) {
      *reinterpret_cast<i32x4*>(sA + srow0 * ROWB + spart) = a0;
      *reinterpret_cast<i32x4*>(sA + srow1 * ROWB + spart) = a1;
      *reinterpret_cast<i32x4*>(sB + srow0 * ROWB + spart) = b0;
      *reinterpret_cast<i32x4*>(sB + srow1 * ROWB + spart) = b1;
      if (first) {
        na0 = norm16(a0, na0);
        na1 = norm16(a1, na1);
      }
      nb0 = norm16(b0, nb0);
      nb1 = norm16(b1, nb1);
      __syncthreads();
      if (c + 1 < chunks) {
        const int off = (c + 1) * KC + spart;
        a0 = fetch16(p.q, q0 + srow0, p.Q, D, off);
        a1 = fetch16(p.q, q0 + srow1, p.Q, D, off);
        b0 = fetch16(p.r, r0 + srow0, p.N, D, off);
        b1 = fetch16(p.r, r0 + srow1, p.N, D, off);
      }
#pragma unroll
      for (int kk = 0; kk < KC / 32; ++kk) {
        i32x4 fa[2], fb[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
          fa[m] = *reinterpret_cast<const i32x4*>(sA + (wm * 64 + m * 32 + frow) * ROWB + kk * 32 + fk);
#pragma unroll
        for (int n = 0; n < 2; ++n)
          fb[n] = *reinterpret_cast<const i32x4*>(sB + (wn * 64 + n * 32 + frow) * ROWB + kk * 32 + fk);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
      }
      __syncthreads();
    }
    // norms: the four threads of a row (tid & 3) are neighbouring lanes
    na0 += __shfl_xor(na0, 1, 64); na0 += __shfl_xor(na0, 2, 64);
    na1 += __shfl_xor(na1, 1, 64); na1 += __shfl_xor(na1, 2, 64);
    nb0 += __shfl_xor(nb0, 1, 64); nb0 += __shfl_xor(nb0, 2, 64);
    nb1 += __shfl_xor(nb1, 1, 64); nb1 += __shfl_xor(nb1, 2, 64);
    if ((tid & 3) == 0) {
      if (first) {
        sNA[srow0] = na0;
        sNA[srow1] = na1;
      }
      sNB[srow0] = nb0;
      sNB[srow1] = nb1;
    }
    __syncthreads();
    // d2 tile; accumulator register e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int col = wn * 64 + n * 32 + (lane & 31);
        const int nb = sNB[col];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int rw = wm * 64 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
          sD2[rw * D2S + col] = sNA[rw] + nb - 2 * acc[m][n][e];
        }
      }
    __syncthreads();
    if (gi < p.Q) {
      const int* drow = sD2 + row * D2S;
      const int cols = min(TR, p.N - r0);                     // the tile's padding is excluded by index
      int last_d = (int)(last >> 32);
#pragma unroll 4
      for (int col = par; col < cols; col += 2) {
        const int d2 = drow[col];
        const int gidx = r0 + col + p.idx_base;
        if ((long long)gidx == self_idx) continue;
        if (p.radius2) cov = cov || d2 <= sRad[col];
        if (d2 <= last_d) {
          const knn_key key = make_key(d2, gidx);
          if (key < last) {
            list_insert(mine, k, key);
            last = mine[k - 1];
            last_d = (int)(last >> 32);
          }
        }
      }
    }
    __syncthreads();
  }

  // the two lists of a row: the odd thread's keys into the even thread's list
  const bool cov_other = __shfl_xor((int)cov, 1, 64) != 0;
  __syncthreads();
  if (gi < p.Q && par == 0) {
    const knn_key* other = mine + k;
    for (int j = 0; j < k; ++j) {
      const knn_key key = other[j];
      if (key < mine[k - 1]) list_insert(mine, k, key);
    }
    knn_key* out = p.ws_keys + ((size_t)s * p.Q + gi) * k;
    for (int j = 0; j < k; ++j) out[j] = mine[j];
    p.ws_cov[(size_t)s * p.Q + gi] = (cov || cov_other) ? 1 : 0;
  }
}

// One thread per query: the k smallest keys of the slices' lists (and of the previous lists, moved to slot `splits`
// first), by taking k times the smallest key above the last one taken.
__global__ __launch_bounds__(NT) void knn_u8_fold_kernel(knn_key* __restrict__ ws_keys, const unsigned char* __restrict__ ws_cov,
                                                         int* __restrict__ dist2, int* __restrict__ idx,
                                                         unsigned char* __restrict__ covered, int Q, int k, int splits,
                                                         int accumulate) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= Q) return;
  int sources = splits;
  if (accumulate) {
    knn_key* prev = ws_keys + ((size_t)splits * Q + i) * k;
    for (int j = 0; j < k; ++j) prev[j] = make_key(dist2[(size_t)i * k + j], idx[(size_t)i * k + j]);
    sources = splits + 1;
  }
  knn_key taken = -1;                                           // below every key: d2 >= 0
  for (int t = 0; t < k; ++t) {
    knn_key best = EMPTY;
    for (int s = 0; s < sources; ++s) {
      const knn_key* L = ws_keys + ((size_t)s * Q + i) * k;
      for (int j = 0; j < k; ++j) {
        const knn_key key = L[j];
        if (key > taken) {                                    // sorted: the first one above is this list's smallest
          best = key < best ? key : best;
          break;
        }
      }
    }
    dist2[(size_t)i * k + t] = (int)(best >> 32);
    idx[(size_t)i * k + t] = (int)(unsigned)(best & 0xffffffffll);
    taken = best;
  }
  if (covered) {
    int c = accumulate ? (covered[i] != 0) : 0;
    for (int s = 0; s < splits; ++s) c |= ws_cov[(size_t)s * Q + i];
    covered[i] = c ? 1 : 0;
  }
}

int auto_splits(int Q) {
  const int qtiles = (Q + TQ - 1) / TQ;
  const int s = (AUTO_BLOCKS + qtiles - 1) / qtiles;
  return s < 1 ? 1 : s > AUTO_MAX_SPLITS ? AUTO_MAX_SPLITS : s;
}

size_t keys_bytes(int Q, int k, int splits) { return ((size_t)splits + 1) * (size_t)Q * k * sizeof(knn_key); }

}  // namespace

MULAN_API size_t mulan_knn_u8_workspace(int Q, int k, int splits) {
  if (Q <= 0 || k < 1 || k > MAX_K || splits < 0 || splits > MAX_SPLITS) return 0;
  const int S = splits ? splits : auto_splits(Q);
  return keys_bytes(Q, k, S) + (size_t)S * Q;
}

MULAN_API int mulan_knn_u8(const unsigned char* q, const unsigned char* r, int Q, int N, int D, int k, int idx_base,
                           int self_offset, int accumulate, int splits, const int* radius2, unsigned char* covered,
                           int* dist2, int* idx, void* workspace, hipStream_t stream) {
  if (!q || !r || !dist2 || !idx || !workspace) return (int)hipErrorInvalidValue;
  if (Q <= 0 || N <= 0 || D < KC || D > MAX_D || D % KC != 0 || k < 1 || k > MAX_K) return (int)hipErrorInvalidValue;
  if (splits < 0 || splits > MAX_SPLITS || (accumulate != 0 && accumulate != 1)) return (int)hipErrorInvalidValue;
  if (idx_base < 0 || (long long)idx_base + N > 0x7fffffffll || self_offset < -1) return (int)hipErrorInvalidValue;
  if ((radius2 == nullptr) != (covered == nullptr)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)q & 15) || ((uintptr_t)r & 15) || ((uintptr_t)workspace & 7) || ((uintptr_t)dist2 & 3) ||
      ((uintptr_t)idx & 3) || ((uintptr_t)radius2 & 3))
    return (int)hipErrorInvalidValue;
  const int qtiles = (Q + TQ - 1) / TQ, rtiles = (N + TR - 1) / TR;
  int S = splits;
  if (S == 0) {                                               // no more slices than reference tiles; the workspace is
    S = auto_splits(Q);                                       // sized for auto_splits(Q), the larger of the two
    if (S > rtiles) S = rtiles;
  }
  if ((long long)qtiles * S > 0x7fffffffll) return (int)hipErrorInvalidValue;
  KnnArgs a{q, r, Q, N, D, k, idx_base, self_offset, S, qtiles, rtiles, radius2,
            static_cast<knn_key*>(workspace), static_cast<unsigned char*>(workspace) + keys_bytes(Q, k, S)};
  const int smem = FIXED_BYTES + NT * k * (int)sizeof(knn_key);
  static bool configured = false;
  if (!configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_u8_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, FIXED_BYTES + NT * MAX_K * 8);
    if (e != hipSuccess) return (int)e;
    configured = true;
  }
  hipLaunchKernelGGL(knn_u8_kernel, dim3((unsigned)(qtiles * S)), dim3(NT), smem, stream, a);
  hipLaunchKernelGGL(knn_u8_fold_kernel, dim3((unsigned)((Q + NT - 1) / NT)), dim3(NT), 0, stream, a.ws_keys, a.ws_cov,
                     dist2, idx, covered, Q, k, S, accumulate);
  MULAN_CHECK_LAUNCH();
}
