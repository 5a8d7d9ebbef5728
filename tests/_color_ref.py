"""Test infrastructure: numpy restatement of the colour part of the reference's clip_augmentation
(datasets/video_transforms.py:248-363, :491-500) on the spatially sampled T x 3 x S x S float32 clip, with the draws
passed in.  Pinned against the executed reference by tests/golden/make_color_golden.py -> tests/golden/clip_color.npz.

Rounding: torch multiplies a float32 tensor by a Python float in float32 with the scalar rounded to float32 first, and
blend() forms 1 - alpha in float64 before that rounding; every product and sum is rounded on its own; the gray sum
associates left to right.  The only step that cannot be mirrored is the contrast stage's frame mean: torch's float32
summation order depends on its vector width and thread count.  ``mean`` selects how it is formed here:
  "f64"   the correctly rounded float64 sum (math.fsum) divided by the count in float64, rounded to float32 once --
          what csrc/input.hip's clip_gray_mean_kernel computes up to the rounding of its own float64 partial sums;
  "f32"   numpy's float32 pairwise mean (one more plausible order, for the spread).
"""
import math

import numpy as np

BRIGHTNESS, CONTRAST, SATURATION = 1, 2, 3
ORDERS = [(a, b, c) for a in (1, 2, 3) for b in (1, 2, 3) for c in (1, 2, 3) if len({a, b, c}) == 3]
_F = np.float32


def gray(x):
    """:262-266 on T x 3 x S x S -> T x S x S; channel indices as written (the function assumes BGR)."""
    return (_F(0.299) * x[:, 2] + _F(0.587) * x[:, 1]) + _F(0.114) * x[:, 0]


def frame_means(g, mean="f64"):
    """T x S x S gray -> T float32 means (the mean over three equal channels is the mean over the pixels)."""
    if mean == "f32":
        return g.reshape(g.shape[0], -1).mean(axis=1, dtype=np.float32)
    n = g[0].size
    return np.array([np.float64(math.fsum(f.ravel().astype(np.float64).tolist())) / np.float64(n) for f in g]
                    ).astype(np.float32)


def blend(x, other, alpha):
    """:248: images1 * alpha + images2 * (1 - alpha)."""
    return x * _F(alpha) + other * _F(1 - alpha)


def color_ref(x, stages, use_gray, mean="f64"):
    """x: T x 3 x S x S float32 (spatially sampled, TCHW); stages: ((code, alpha), ...) in application order."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    for code, alpha in stages:
        if code == BRIGHTNESS:
            x = blend(x, np.zeros_like(x), alpha)
        elif code == CONTRAST:
            m = frame_means(gray(x), mean)
            x = blend(x, m[:, None, None, None], alpha)
        elif code == SATURATION:
            x = blend(x, gray(x)[:, None], alpha)
        else:
            raise ValueError(code)
    if use_gray:
        x = np.repeat(gray(x)[:, None], 3, axis=1)
    assert x.dtype == np.float32
    return x


def clip_color_ref(frames_u8, spatial, crop, stages, use_gray, mean="f64"):
    """uint8 T x H x W x 3 frames -> 3 x T x S x S float32: oracle.input_ref's spatial sampling, then the stages."""
    from oracle import input_ref
    nh, nw, yo, xo, flip = spatial
    y = input_ref.clip_augmentation_ref(frames_u8, (nh, nw), yo, xo, flip, crop)          # C T S S
    y = color_ref(y.transpose(1, 0, 2, 3), stages, use_gray, mean)
    return np.ascontiguousarray(y.transpose(1, 0, 2, 3))
