"""Host model (numpy, no GPU) of the "f16x3" scheme of the per-pixel dense kernels, written from include/mulan_hip.h and
the comments of mulan_amd/csrc/f16x3_common.h: an fp32 operand is multiplied by a power of two taken from the maximum of
its tensor (per image for activations), and the product is held as two fp16 pieces h + l.

    scale_of(maxbits)       s = 2^(140 - e), inv = 1 / s, e = biased exponent of the maximum clamped to [14, 254]
    split2(vs)              h = f16(vs), l = f16(vs - f32(h)), both round to nearest even
    row_max16(x)            fp32 bits of max |x| per image
    pack_linear(w, t)       packed weight operand, fp16 [K/16][N][plane][16]
    planes_of(x1, x2, r)    split planes of [x1 | x2], fp16 [B][K/16][rows][plane][16], one scale per image
    dense_ref(...)          float64 result on the fp32-rounded inputs, and the magnitude sum |x||w| + |bias| + |res|

The 3x3 convolutions (conv3x3_f16x3*.hip, f16x3_prep.hip, wgrad_f16x3.hip) use the same scheme; their counterparts stand
at the end of this file:

    conv_pack_index(C, N)   position of piece `plane` of Wl[t][kin][o] in the packed operand [9][C/16][N][plane][16]
    pack_conv(w, flip)      packed 3x3 weights; flip = 1: Wl[t][k][o] = w[8 - t][o][k], the input-gradient operand
    conv_planes(x)          split planes of an image tensor: planes_of with rows = H * W, the layout is the same
    conv_ref / dgrad_ref / wgrad_ref    float64 results on the fp32-rounded inputs with their magnitude sums, any H
    model_conv / model_dgrad / model_wgrad    the three-product sum of the scaled pieces with an exact accumulator
    conv_floor(x, w)        the absolute floor of the split under the scale clamp

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


# ---------------------------------------------------------------------------------------------- the 3x3 convolutions
def conv_pack_index(C, N):
    """int64 [9, C, N, 2]: position (in fp16 elements) of piece `plane` of Wl[t][kin][o] in the packed operand
    [9][C/16][N][plane][16]; C input and N output channels OF Wl (with flip = 1 those of w swapped)"""
    t = np.arange(9)[:, None, None, None]
    return t * (C * N * 2) + pack_index(C, N)[None]


def flip_conv(w):
    """w [3, 3, C, N] -> the operand of the input-gradient convolution [3, 3, N, C]: wT[t][n][c] = w[8 - t][c][n]"""
    w = np.asarray(w)
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))


def pack_conv(w, flip):
    """w float32 [3, 3, C, N] -> (packed fp16 [9 * C * N * 2], maxbits): the pieces of s_w * Wl in [9][Kin/16][Nout][2][16],
    Wl = w (flip = 0) or Wl[t][k][o] = w[8 - t][o][k] (flip = 1), s_w from the maximum of the whole tensor"""
    w = np.asarray(w, np.float32)
    _, _, C, N = w.shape
    w9 = w.reshape(9, C, N)
    wl = w9[::-1].transpose(0, 2, 1) if flip else w9
    Kin, Nout = wl.shape[1:]
    assert Kin % 16 == 0
    maxbits = int(bits_of(np.abs(w).max()))
    s, _ = scale_of(maxbits)
    h, l = split2(wl * s)
    idx = conv_pack_index(Kin, Nout)
    out = np.empty(9 * C * N * 2, np.float16)
    out[idx[..., 0]] = h
    out[idx[..., 1]] = l
    return out, maxbits


def unpack_conv(packed, C, N):
    """packed fp16 [9 * C * N * 2] -> (h, l) as [9, C, N] arrays in the orientation of Wl (C, N: those of Wl)"""
    idx = conv_pack_index(C, N)
    packed = np.asarray(packed).reshape(-1)
    return packed[idx[..., 0]], packed[idx[..., 1]]


def conv_planes(x):
    """x float32 [B, H, W, C] -> fp16 [B * C * H * W * 2]: the planes [B][C/16][H * W][plane][16] an f16x3 convolution
    hands on.  The layout is that of the dense kernels with rows = H * W (plane_index), one scale per image."""
    x = np.asarray(x, np.float32)
    B, H, W, C = x.shape
    return planes_of(x.reshape(B * H * W, C), None, H * W)


def conv64(x, w):
    """float64 SAME 3x3 convolution, x [B, H, W, C], w [3, 3, C, N]: the nine shifted products of
    oracle.mulan_np.conv3x3 (which takes any height, but sums them with einsum: ten times the host time), written as
    matrix products; tests/test_f16x3_conv_oracle.py holds the two equal"""
    B, H, W, C = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    y = np.zeros((B * H * W, w.shape[3]))
    for kh in range(3):
        for kw in range(3):
            y += np.ascontiguousarray(xp[:, kh:kh + H, kw:kw + W]).reshape(-1, C) @ w[kh, kw]
    return y.reshape(B, H, W, -1)


def wgrad64(x, dy):
    """float64 dw[kh, kw, c, n] = sum over images and pixels of x[b, h + kh - 1, w + kw - 1, c] dy[b, h, w, n]"""
    B, H, W, C = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    d = dy.reshape(B * H * W, -1)
    dw = np.empty((3, 3, C, d.shape[1]))
    for kh in range(3):
        for kw in range(3):
            dw[kh, kw] = np.ascontiguousarray(xp[:, kh:kh + H, kw:kw + W]).reshape(-1, C).T @ d
    return dw


def _adds(B, H, W, N, bias, cbias, res):
    """the epilogue's addends broadcast to [B, H, W, N] (cbias [B, N] per sample or [B, H, W, N] per pixel), float64"""
    out = []
    for t in (bias, cbias, res):
        if t is not None:
            t = f32(t)
            if t.ndim == 2:
                t = t[:, None, None, :]
            out.append(np.broadcast_to(t, (B, H, W, N)))
    return out


def conv_ref(x, w, bias=None, cbias=None, res=None):
    """float64 conv(x, w) + bias + cbias + res on the fp32-rounded inputs, and mag = conv(|x|, |w|) + |bias| + |cbias| +
    |res|; x [B, H, W, C] with any H, w [3, 3, C, N]"""
    x, w = f32(x), f32(w)
    ref, mag = conv64(x, w), conv64(np.abs(x), np.abs(w))
    for t in _adds(*ref.shape, bias, cbias, res):
        ref = ref + t
        mag = mag + np.abs(t)
    return ref, mag


def dgrad_ref(dy, w):
    """float64 dx = conv(dy, wT), wT[t][n][c] = w[8 - t][c][n], and mag = |dy| * |wT|; dy [B, H, W, N], w [3, 3, C, N]"""
    return conv_ref(dy, flip_conv(w))


def wgrad_ref(x, dy):
    """float64 dw [3, 3, C, N] and mag = |x|^T |dy| per tap, on the fp32-rounded inputs"""
    x, dy = f32(x), f32(dy)
    return wgrad64(x, dy), wgrad64(np.abs(x), np.abs(dy))


def _pieces(v, s):
    """(h, l) of v * s as float64; s broadcasts against v (float32 each)"""
    h, l = split2(np.asarray(v, np.float32) * s)
    return h.astype(np.float64), l.astype(np.float64)


def _image_scales(x):
    """x [B, ...] -> float32 [B, 1, 1, 1]: the scale of every image"""
    return np.array([scale_of(m)[0] for m in row_max16(x)], np.float32).reshape(-1, 1, 1, 1)


def model_conv(x, w, bias=None, cbias=None, res=None):
    """what the forward kernel gives with an exact accumulator: a_h b_h + a_h b_l + a_l b_h of the pieces of x * s_x[b]
    and w * s_w, summed in float64 and divided by s_x[b] s_w, plus the addends"""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    sx = _image_scales(x)
    sw = scale_of(int(bits_of(np.abs(w).max())))[0]
    ah, al = _pieces(x, sx)
    bh, bl = _pieces(w, sw)
    y = (conv64(ah, bh) + conv64(ah, bl) + conv64(al, bh)) / sx.astype(np.float64) / np.float64(sw)
    for t in _adds(*y.shape, bias, cbias, res):
        y = y + t
    return y


def model_dgrad(dy, w):
    """the input-gradient kernel with an exact accumulator: model_conv on the flipped operand (same maximum, same scale)"""
    return model_conv(dy, flip_conv(w))


def model_wgrad(x, dy, per_image):
    """the weight-gradient kernels with an exact accumulator.  per_image: the plane-fed kernel multiplies the planes, which
    carry one scale per image; otherwise (the nine-tap kernel) both tensors are split with the scale of their tensor-wide
    maximum"""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    B = x.shape[0]
    if per_image:
        sx, sg = _image_scales(x), _image_scales(dy)
    else:
        sx = np.full((B, 1, 1, 1), scale_of(int(row_max16(x).max()))[0], np.float32)
        sg = np.full((B, 1, 1, 1), scale_of(int(row_max16(dy).max()))[0], np.float32)
    ah, al = _pieces(x, sx)
    bh, bl = _pieces(dy, sg)
    dw = 0.0
    for b in range(B):
        i = slice(b, b + 1)
        part = wgrad64(ah[i], bh[i]) + wgrad64(ah[i], bl[i]) + wgrad64(al[i], bh[i])
        dw = dw + part / np.float64(sx[b, 0, 0, 0]) / np.float64(sg[b, 0, 0, 0])
    return dw


def clamped(x):
    """bool [B]: images whose maximum lies below the scale clamp (biased exponent < 14: zero, subnormal, below 2^-113)"""
    return ((row_max16(x) >> 23) & 255) < 14


def conv_floor(x, w):
    """float64 [B, H, W, N]: the absolute floor of the split for conv(x, w).  Under the clamp s_x stays at 2^126 however small
    the image is, x * s_x falls below 2^13 and the pieces end at the fp16 subnormal spacing: |x s_x - h - l| <= 2^-25
    absolute (split_bound), i.e. 2^-25 / s_x in the units of x; the same holds for w with s_w.  A product x w is then off
    by at most (2^-25 / s_x) |w| + |x| (2^-25 / s_w), and the floor is that sum over the products of an output element
    (border pixels have fewer)."""
    x, w = f32(x), f32(w)
    sx = _image_scales(x).astype(np.float64)
    sw = np.float64(scale_of(int(bits_of(np.abs(w).max())))[0])
    return 2.0 ** -25 / sx * conv64(np.ones_like(x), np.abs(w)) + 2.0 ** -25 / sw * conv64(np.abs(x), np.ones_like(w))
