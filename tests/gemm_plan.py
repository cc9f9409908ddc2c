"""Host restatement of mulan_gemm's launch plan (mulan_amd/csrc/gemm.hip): which of the three tiles a call lands on, and
in how many k splits.  A port of plan_ksplit, ksplit_big_tile and the tile choice at the end of mulan_gemm, line for line,
so that a test can say which kernel a shape reaches.  tests/test_gemm_plan.py holds it against the built library
(mulan_gemm_workspace) and against the text of gemm.hip; tests/test_gpu_gemm.py asserts with it that each of its cases
runs on the kernel it was written for."""

T128, T128x32, T64 = "128x128", "128x32", "64x64"

# the direct path's tile choice: 128 x 128 when M >= BIG_MIN_M && N >= BIG_MIN_N && tiles128 >= BIG_MIN_TILES,
# else 128 x 32 when N <= THIN_MAX_N, else 64 x 64
BIG_MIN_M = 128
BIG_MIN_N = 128
BIG_MIN_TILES = 256
THIN_MAX_N = 32


def ksplit_big_tile(M, N, K):
    return K >= 4096 and M % 128 == 0 and N % 128 == 0


def plan_ksplit(M, N, K, batch):
    """(splits, kchunk) of gemm.hip's plan_ksplit; (1, K) when the product is not split"""
    if batch != 1:
        return 1, K
    big = ksplit_big_tile(M, N, K)
    tiles = (M // 128) * (N // 128) if big else ((M + 63) // 64) * ((N + 63) // 64)
    if K >= 4096:
        if tiles >= 256:
            return 1, K
        s = (256 if big else 512) // tiles
        s = min(s, K // 512)
    else:
        if K < 256:
            return 1, K
        if tiles > 8:
            if tiles >= 128 or K < 1024:
                return 1, K
            s = (768 + tiles - 1) // tiles
            s = min(s, K // 256)
        else:
            s = K // 64
    if s < 2:
        return 1, K
    kc = ((K + s - 1) // s + 15) // 16 * 16
    return (K + kc - 1) // kc, kc


def direct_tile(M, N, batch):
    tiles128 = ((M + 127) // 128) * ((N + 127) // 128) * batch
    if M >= BIG_MIN_M and N >= BIG_MIN_N and tiles128 >= BIG_MIN_TILES:
        return T128
    if N <= THIN_MAX_N:
        return T128x32
    return T64


def plan(M, N, K, batch, workspace_given):
    """(tile, splits, kchunk) of the kernel that mulan_gemm(M, N, K, batch, workspace) launches"""
    if workspace_given:
        s, kc = plan_ksplit(M, N, K, batch)
        if s > 1:
            return (T128 if ksplit_big_tile(M, N, K) else T64), s, kc
    return direct_tile(M, N, batch), 1, K


def workspace_bytes(M, N, K, batch):
    s, _ = plan_ksplit(M, N, K, batch)
    return s * M * N * 4 if s > 1 else 0


def vec(a_ptr, b_ptr, M, N, K, lda, ldb, transA, transB, strideA, strideB):
    """mulan_gemm's gate between the float4 loaders and the scalar ones"""
    contig_a = M if transA else K
    contig_b = K if transB else N
    return (a_ptr % 16 == 0 and b_ptr % 16 == 0 and lda % 4 == 0 and ldb % 4 == 0 and contig_a % 4 == 0
            and contig_b % 4 == 0 and strideA % 4 == 0 and strideB % 4 == 0)
