"""Golden vectors for colour jitter / grayscale in the clip augmentation, produced by EXECUTING the reference's
datasets/video_transforms.clip_augmentation (it imports only math/numpy/torch) with colorjitter / use_grayscale on.

    python tests/golden/make_color_golden.py        # needs /root/reference; writes tests/golden/clip_color.npz

np.random is seeded per case; the draws the reference makes are recovered by replaying the same generator calls in
the same order: size (:52), y / x offsets (:121-125), flip (:158), then the jitter gate (:493), the permutation (:297),
one alpha per stage in application order (:320,339,359) and the grayscale gate (:499).

Per case c<i>: _params (int64), _codes (stage codes in application order, 0 = none), _alphas (float64), _out (whole
output, crop 64) or _sample (strided, crop 112; with _sum, the order-free checksum of every output word, where no
contrast stage makes the output depend on torch's summation order), and
  _spread  the largest difference between the reference's own outputs at 1, 2 and 8 torch threads,
  _dev     the largest difference between the stored output and tests/_color_ref.py with a float64 frame mean,
  _maxabs  the largest magnitude of the output
-- what tests/test_color_*.py derive the tolerance of the contrast cases from.  The stored output is the 8-thread run.
All sizes are at or above the 64 x 64 outputs from which oracle/input_ref.py's bilinear association is bit-identical to
torch's CPU kernel -- at 2 threads and more: with ONE thread torch's bilinear kernel itself takes another association
(up to 4.8e-7 away, with the colour flags off as well), so _spread holds that too, also for the cases without a
contrast stage; _spread_mt (2 against 8 threads) is the part that comes from the summation order of the frame mean, and
is 0 wherever there is no contrast stage.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import input_ref                                                     # noqa: E402
from tests import _color_ref as CR                                               # noqa: E402

spec = importlib.util.spec_from_file_location("ref_video_transforms", "/root/reference/datasets/video_transforms.py")
vt = importlib.util.module_from_spec(spec)
spec.loader.exec_module(vt)

L, P, N, V = (128, 171, 128, 160, 112, -1), (171, 128, 128, 160, 112, -1), (128, 171, 128, 128, 112, -1), \
    (128, 171, 128, 128, 112, 4)
SL, SP = (72, 96, 64, 80, 64, -1), (96, 72, 64, 80, 64, -1)
CASES = [  # seed, T, (H, W, min_scale, max_scale, crop, spatial_idx), colorjitter, use_grayscale
    (1, 4, L, True, True),       # contrast, saturation, brightness; grayscale after the jitter
    (2, 4, P, True, True),       # portrait: brightness, contrast, saturation
    (3, 4, N, True, True),       # no resize: brightness, saturation, contrast
    (4, 4, L, True, True),       # saturation, brightness, contrast; grayscale
    (5, 4, P, True, True),       # portrait: saturation, contrast, brightness; grayscale
    (11, 4, L, True, True),      # contrast, brightness, saturation; grayscale
    (6, 4, L, True, True),       # the jitter gate says no (u < 0.2), no grayscale: the plain spatial output
    (12, 4, L, True, True),      # gate no, grayscale
    (5, 4, L, False, True),      # grayscale alone (colorjitter off: no gate draw)
    (12, 4, V, True, True),      # test-time view (centre crop + flip): contrast, saturation, brightness; grayscale
    (9, 2, SL, True, True),      # small, whole: brightness, contrast, saturation; grayscale
    (18, 2, SL, True, True),     # small, whole: gate no, grayscale
    (10, 2, SL, True, False),    # small, whole: colorjitter alone: brightness, saturation, contrast
    (4, 2, SP, True, True),      # small portrait, whole: saturation, brightness, contrast; grayscale
]


def replay(seed, H, W, lo, hi, crop, sidx, cj, gs):
    np.random.seed(seed)
    size = int(round(np.random.uniform(lo, hi)))
    nh, nw = input_ref.resized_shape(H, W, size)
    if sidx == -1:
        yo = int(np.random.randint(0, nh - crop)) if nh > crop else 0
        xo = int(np.random.randint(0, nw - crop)) if nw > crop else 0
        flip = bool(np.random.uniform() < 0.5)
    else:
        yo, xo = input_ref.uniform_crop_offsets(nh, nw, crop, {0: 0, 1: 1, 2: 2, 3: 0, 4: 1, 5: 2}[sidx])
        flip = sidx in (3, 4, 5)
        if flip:
            np.random.uniform()
    gate, stages, gray, ugray = -1.0, [], False, -1.0
    if cj:
        gate = np.random.uniform()
        if gate >= 0.2:
            order = np.random.permutation(np.arange(3))
            for i in range(3):
                stages.append((int(order[i]) + 1, 1.0 + np.random.uniform(-0.4, 0.4)))
    if gs:
        ugray = np.random.uniform()
        gray = bool(ugray >= 0.8)
    return (nh, nw, yo, xo, flip), stages, gray, gate, ugray


out = {}
seen_orders = set()
for i, (seed, T, (H, W, lo, hi, crop, sidx), cj, gs) in enumerate(CASES):
    frames = np.random.RandomState(seed).randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)   # a frozen stream
    runs = []
    for nt in (1, 2, 8):
        torch.set_num_threads(nt)
        np.random.seed(seed)
        runs.append(vt.clip_augmentation(torch.from_numpy(frames), spatial_idx=sidx, min_scale=lo, max_scale=hi,
                                         crop_size=crop, colorjitter=cj, use_grayscale=gs).contiguous().numpy())
    y = runs[2]
    spread = max(float(np.abs(a - b).max()) for a in runs for b in runs)
    spread_mt = float(np.abs(runs[1] - runs[2]).max())
    spatial, stages, gray, gate, ugray = replay(seed, H, W, lo, hi, crop, sidx, cj, gs)
    ref = CR.clip_color_ref(frames, spatial, crop, stages, gray, mean="f64")
    dev = float(np.abs(ref.astype(np.float64) - y).max())
    contrast = any(c == CR.CONTRAST for c, _ in stages)
    if not contrast:
        assert spread_mt == 0.0 and np.array_equal(ref, y), (i, spread_mt, dev)
    if stages:
        seen_orders.add(tuple(c for c, _ in stages))
    k = f"c{i}"
    nh, nw, yo, xo, flip = spatial
    out[k + "_params"] = np.array([lo, hi, crop, sidx, nh, nw, yo, xo, int(flip), seed, T, H, W, int(cj), int(gs),
                                   int(gray)], dtype=np.int64)
    out[k + "_codes"] = np.array([c for c, _ in stages] + [0] * (3 - len(stages)), dtype=np.int64)
    out[k + "_alphas"] = np.array([a for _, a in stages] + [0.0] * (3 - len(stages)), dtype=np.float64)
    out[k + "_spread"] = np.array([spread])
    out[k + "_spread_mt"] = np.array([spread_mt])
    out[k + "_dev"] = np.array([dev])
    out[k + "_maxabs"] = np.array([float(np.abs(y).max())])
    if crop <= 64:
        out[k + "_out"] = y
    else:
        out[k + "_sample"] = y[:, ::3, ::7, ::5].copy()
        if not contrast:
            out[k + "_sum"] = np.array([np.ascontiguousarray(y).view(np.uint32).astype(np.uint64).sum()])
    print(k, "seed", seed, tuple(y.shape), spatial, "gate %.3f" % gate, [(c, round(a, 4)) for c, a in stages],
          "gray-u %.3f" % ugray, gray, "| threads spread", spread, "(2 vs 8:", spread_mt, ")", "restatement dev", dev,
          "bit-equal" if np.array_equal(ref, y) else "")
assert len(seen_orders) == 6, seen_orders
path = os.path.join(HERE, "clip_color.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
