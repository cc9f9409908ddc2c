"""Host model (numpy, no GPU) of the "f16x3" scheme of the per-pixel dense kernels, written from include/mulan_hip.h and
the comments of mulan_amd/csrc/f16x3_common.h: an fp32 operand is multiplied by a power of two taken from the maximum of
its tensor (per image for activations), and the product is held as two fp16 pieces h + l.

    scale_of(maxbits)       s = 2^(140 - e), inv = 1 / s, e = biased exponent of the maximum clamped to [14, 254]
    split2(vs)              h = f16(vs), l = f16(vs - f32(h)), both round to nearest even
    row_max16(x)            fp32 bits of max |x| per image
    pack_linear(w, t)       packed weight operand, fp16 [K/16][N][plane][16]
    planes_of(x1, x2, r)    split planes of [x1 | x2], fp16 [B][K/16][rows][plane][16], one scale per image
    dense_ref(...)          float64 result on the fp32-rounded inputs, and the magnitude sum |x||w| + |bias| + |res|

The index maps of the two layouts are functions of their own (pack_index, plane_index) so that a test can hold them to
being bijections, and unpack_linear / unplane invert the layouts for the tests that bound h + l against the operand."""
import numpy as np


def bits_of(v):
    """fp32 bit pattern(s) of v as uint32"""
    return np.asarray(v, np.float32).view(np.uint32)


def scale_of(maxbits):
    """(s, inv) as np.float32: s = 2^(140 - e) with e the biased exponent of the maximum, clamped to [14, 254], so that
    max * s lies in [2^13, 2^14) for every normal maximum inside the clamp; inv = 1 / s = 2^(e - 140)"""
    e = (int(maxbits) >> 23) & 255
    e = min(max(e, 14), 254)
    return np.float32(2.0 ** (140 - e)), np.float32(2.0 ** (e - 140))


def split2(vs):
    """vs (float32, already scaled) -> (h, l), both np.float16: h = RNE(vs), l = RNE(vs - h) with the difference formed
    in float32"""
    vs = np.asarray(vs, np.float32)
    h = vs.astype(np.float16)
    l = (vs - h.astype(np.float32)).astype(np.float16)
    return h, l


def row_max16(x):
    """x [B, ...] -> uint32 [B]: fp32 bits of max |x[b]|"""
    x = np.asarray(x, np.float32)
    return bits_of(np.abs(x).reshape(x.shape[0], -1).max(axis=1))


def pack_index(K, N):
    """int64 [K, N, 2]: position (in fp16 elements) of piece `plane` of Wl[kin][o] in the packed operand
    [K/16][N][plane][16]"""
    kin, o, pl = np.arange(K)[:, None, None], np.arange(N)[None, :, None], np.arange(2)[None, None, :]
    return (((kin // 16) * N + o) * 2 + pl) * 16 + kin % 16


def plane_index(B, K, rows):
    """int64 [B, rows, K, 2]: position (in fp16 elements) of piece `plane` of x[b][r][k] in the plane tensor
    [B][K/16][rows][plane][16]"""
    b, r = np.arange(B)[:, None, None, None], np.arange(rows)[None, :, None, None]
    k, pl = np.arange(K)[None, None, :, None], np.arange(2)[None, None, None, :]
    return ((((b * (K // 16) + k // 16) * rows + r) * 2) + pl) * 16 + k % 16


def pack_linear(w, transpose):
    """w float32 [K, N], or [N, K] with transpose (the operand is then its transpose) -> (packed fp16 [K * N * 2],
    maxbits): the pieces of s_w * Wl, s_w from the maximum of the whole tensor"""
    w = np.asarray(w, np.float32)
    wl = w.T if transpose else w
    K, N = wl.shape
    assert K % 16 == 0
    maxbits = int(bits_of(np.abs(w).max()))
    s, _ = scale_of(maxbits)
    h, l = split2(wl * s)
    idx = pack_index(K, N)
    out = np.empty(K * N * 2, np.float16)
    out[idx[..., 0]] = h
    out[idx[..., 1]] = l
    return out, maxbits


def unpack_linear(packed, K, N):
    """packed fp16 [K * N * 2] -> (h, l) as [K, N] arrays in the orientation of Wl"""
    idx = pack_index(K, N)
    packed = np.asarray(packed).reshape(-1)
    return packed[idx[..., 0]], packed[idx[..., 1]]


def planes_of(x1, x2, rows_per_img):
    """x1 [M, K1], x2 [M, K2] or None (float32) -> fp16 [B * K * rows * 2]: the planes of [x1 | x2], image b scaled
    with the larger of the maxima of x1[b] and x2[b]"""
    x1 = np.asarray(x1, np.float32)
    x = x1 if x2 is None else np.concatenate([x1, np.asarray(x2, np.float32)], axis=-1)
    M, K = x.shape
    assert M % rows_per_img == 0 and K % 16 == 0
    B = M // rows_per_img
    x = x.reshape(B, rows_per_img, K)
    vs = scaled(x)
    h, l = split2(vs)
    idx = plane_index(B, K, rows_per_img)
    out = np.empty(B * K * rows_per_img * 2, np.float16)
    out[idx[..., 0]] = h
    out[idx[..., 1]] = l
    return out


def scaled(x):
    """x float32 [B, rows, K] -> x * s_b in float32, s_b from the maximum of image b (the concat's maximum is the larger
    of its halves' maxima)"""
    x = np.asarray(x, np.float32)
    s = np.array([scale_of(m)[0] for m in row_max16(x)], np.float32)
    return x * s.reshape(-1, *([1] * (x.ndim - 1)))


def unplane(planes, B, K, rows):
    """fp16 [B * K * rows * 2] -> (h, l) as [B, rows, K] arrays"""
    idx = plane_index(B, K, rows)
    planes = np.asarray(planes).reshape(-1)
    return planes[idx[..., 0]], planes[idx[..., 1]]


def split_bound(vs):
    """the reconstruction bound of split2 for |vs| < 2^14 (derived in tests/test_f16x3_oracle.py)"""
    return 2.0 ** -22 * np.abs(np.asarray(vs, np.float64)) + 2.0 ** -25


def f32(a):
    """round to fp32, return as float64"""
    return np.asarray(a).astype(np.float32).astype(np.float64)


def dense_ref(x1, x2, w, bias=None, res=None):
    """float64 [x1 | x2] @ w + bias + res on the fp32-rounded inputs, and mag = |x| @ |w| + |bias| + |res|.
    x* are [..., K*]; w is [K, N], or [B, K, N] against x [B, rows, K] (one operand per image)."""
    x = f32(x1) if x2 is None else np.concatenate([f32(x1), f32(x2)], axis=-1)
    w = f32(w)
    ref = np.matmul(x, w)
    mag = np.matmul(np.abs(x), np.abs(w))
    for t in (bias, res):
        if t is not None:
            ref = ref + f32(t)
            mag = mag + np.abs(f32(t))
    return ref, mag
