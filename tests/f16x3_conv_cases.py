"""The non-integer input sets of tests/test_gpu_conv_f16x3.py, by name.  One generator serves the GPU tests and the CPU
test that holds the host model of the kernels (tests/f16x3_oracle.py: model_conv, model_dgrad, model_wgrad) to the very
bars the GPU tests assert (tests/test_f16x3_conv_oracle.py), so the two cannot drift apart.

Every set is a dict of float32 arrays: x [B, H, 32, C], w [3, 3, C, N], dy [B, H, 32, N] (the image tensor of the input
gradient, with the per-image maxima of x), g [B, H, 32, N] and xg [B, H, 32, C] (unremarkable partners for the weight
gradients: dw from (x, g) and from (xg, dy)), bias [N], cbias [B, N], res [B, H, 32, N]."""
import math

import numpy as np

BAR = 3e-6          # of the magnitude sum, per element: the figure of test_f16x3_accuracy_matches_fp32_kernel
MODEL_SHARE = 0.5   # the exact-accumulator model must stay within this share of a bar; the rest is the fp32 accumulator's

SMALL = (1.0, 2.0 ** -120, 2.0 ** -132, 0.0)      # normal; below the clamp (e < 14); fp32 subnormal; all zero
BIG = (1.0, 2.0 ** 120, 2.0 ** -120, 1e-3)        # one image near the top of fp32

CASES = {
    #            B  H   C    N    image magnitudes             w factor   partner factor
    "gauss_h24": (3, 24, 128, 128, (1.0, 1e-4, 300.0), 1.0, 1.0),
    "gauss_h32": (2, 32, 128, 128, (1.0, 3e-3), 1.0, 1.0),
    "clamp_small": (4, 8, 128, 128, SMALL, 1.0, 1.0),
    # 2^120 times a sum of 1152 products: the weights and the partners are scaled down so that every result stays finite
    "clamp_big": (4, 8, 128, 128, BIG, 2.0 ** -8, 2.0 ** -20),
}


def _images(rng, B, H, ch, mags, heavy):
    t = rng.standard_normal((B, H, 32, ch))
    if heavy:
        t = t * np.exp(rng.standard_normal(t.shape))
    t = t / np.abs(t).reshape(B, -1).max(axis=1).reshape(B, 1, 1, 1)          # maximum 1 per image ...
    return (t * np.asarray(mags, np.float64).reshape(B, 1, 1, 1)).astype(np.float32)   # ... then exactly the magnitude


def conv_case(name):
    B, H, C, N, mags, wf, pf = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    heavy = name.startswith("gauss")
    w = rng.standard_normal((3, 3, C, N))
    if heavy:
        w = w * np.exp(rng.standard_normal(w.shape))
    w = (w / math.sqrt(9 * C) * wf).astype(np.float32)
    m = np.asarray(mags, np.float64).reshape(B, 1, 1, 1)
    return dict(B=B, H=H, C=C, N=N, w=w,
                x=_images(rng, B, H, C, mags, heavy), dy=_images(rng, B, H, N, mags, heavy),
                g=(rng.standard_normal((B, H, 32, N)) * pf).astype(np.float32),
                xg=(rng.standard_normal((B, H, 32, C)) * pf).astype(np.float32),
                bias=(rng.standard_normal(N) * wf).astype(np.float32),
                cbias=(rng.standard_normal((B, N)) * wf).astype(np.float32),
                res=(rng.standard_normal((B, H, 32, N)) * np.where(m == 0, 1.0, m) * wf).astype(np.float32))


def image_bar(fo, x, w, mag):
    """the bar of one forward / input-gradient launch, [B, H, W, N]: BAR * mag, plus the absolute floor of the split
    (fo.conv_floor) for the images under the scale clamp"""
    return BAR * mag + fo.conv_floor(x, w) * fo.clamped(x).reshape(-1, 1, 1, 1)
