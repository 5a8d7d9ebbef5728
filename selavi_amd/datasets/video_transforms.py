"""clip_augmentation on the GPU (mirrors /root/reference/datasets/video_transforms.py:420-510).

The reference normalises, permutes, resizes (bilinear), crops and flips one clip at a time on the CPU, creating four
intermediate tensors.  Here the random draws are made on the host with the SAME np.random calls in the SAME order
(:52 size, :121-125 crop offsets, :158 flip), and one kernel (csrc/input.hip: slv_clip_augment) reads the uint8
frames once and writes the float32 C x T x S x S clip -- for a whole batch per launch.

Colour jitter and grayscale (:273-363, :491-500) ride on the same kernel (slv_clip_augment_color): their draws are made
by sample_color_params, again with the reference's generator calls, and ClipAugmenter is the per-batch callable that
draws for every clip what the reference's worker would draw for it.

clip_sample_augmentation_batch is the same step for callers that hold whole decoded videos: a B x T table of frame
indices (datasets/decoder.py: frame_indices) goes up with the descriptors and slv_clip_sample_augment[_color] reads
those frames straight from the videos, so temporal_sampling's gathered copy is never made.
"""
import math

import numpy as np
import torch

from .._lib import C, ptr, stream

MEAN = [0.45, 0.45, 0.45]                  # video_transforms.py:13-14
STD = [0.225, 0.225, 0.225]
_MEAN = np.array(MEAN, dtype=np.float32)
_STD = np.array(STD, dtype=np.float32)


def _resized_shape(height, width, size):
    """video_transforms.py:52-67."""
    if (width <= height and width == size) or (height <= width and height == size):
        return height, width
    if width < height:
        return int(math.floor((float(height) / width) * size)), size
    return size, int(math.floor((float(width) / height) * size))


def sample_spatial_params(height, width, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224):
    """The host half of spatial_sampling (:420-459): draws (resized H, resized W, y offset, x offset, flip)
    with the reference's generator calls."""
    assert spatial_idx in [-1, 0, 1, 2, 3, 4, 5]
    size = int(round(np.random.uniform(min_scale, max_scale)))
    nh, nw = _resized_shape(height, width, size)
    if nh < crop_size or nw < crop_size:
        raise ValueError(f"crop {crop_size} does not fit the resized frame {nh}x{nw}")
    if spatial_idx == -1:
        y_off = x_off = 0
        if not (nh == crop_size and nw == crop_size):                       # random_crop :115-125
            if nh > crop_size:
                y_off = int(np.random.randint(0, nh - crop_size))
            if nw > crop_size:
                x_off = int(np.random.randint(0, nw - crop_size))
        flip = bool(np.random.uniform() < 0.5)                               # horizontal_flip :158
        return nh, nw, y_off, x_off, flip
    idx = {0: 0, 1: 1, 2: 2, 3: 0, 4: 1, 5: 2}[spatial_idx]                  # uniform_crop :186-201
    y_off = int(math.ceil((nh - crop_size) / 2))
    x_off = int(math.ceil((nw - crop_size) / 2))
    if nh > nw:
        y_off = 0 if idx == 0 else (nh - crop_size if idx == 2 else y_off)
    else:
        x_off = 0 if idx == 0 else (nw - crop_size if idx == 2 else x_off)
    flip = spatial_idx in (3, 4, 5)
    if flip:
        np.random.uniform()                                                  # horizontal_flip(1, ...) still draws
    return nh, nw, y_off, x_off, flip


BRIGHTNESS, CONTRAST, SATURATION = 1, 2, 3       # stage codes of slv_clip_augment_color (0: none)
_JITTER = (BRIGHTNESS, CONTRAST, SATURATION)     # color_jitter's list order (:288-294)


class ColorParams:
    """The colour draws of one clip: ``stages`` = ((code, alpha), ...) in application order (empty: the jitter gate
    said no, or colorjitter is off), ``gray``: grayscale applied after them."""
    __slots__ = ("stages", "gray")

    def __init__(self, stages=(), gray=False):
        self.stages, self.gray = tuple((int(c), float(a)) for c, a in stages), bool(gray)

    def __eq__(self, other):
        return isinstance(other, ColorParams) and (self.stages, self.gray) == (other.stages, other.gray)

    def __repr__(self):
        return f"ColorParams(stages={self.stages}, gray={self.gray})"


def sample_color_params(colorjitter=False, use_grayscale=False, var=0.4):
    """The host half of the colour part of clip_augmentation (:491-500), called after sample_spatial_params for the
    same clip: the gate draw, color_jitter's permutation (:297) and one alpha per stage in application order
    (:320,339,359), then the grayscale gate.  With both flags off it draws nothing."""
    stages, gray = [], False
    if colorjitter:
        if np.random.uniform() >= 0.2:
            order = np.random.permutation(np.arange(3))
            for idx in range(3):
                stages.append((_JITTER[order[idx]], 1.0 + np.random.uniform(-var, var)))
    if use_grayscale:
        gray = bool(np.random.uniform() >= 0.8)
    return ColorParams(stages, gray)


def _color_desc(color):
    """B x 12 32-bit words: stage codes x 3, grayscale flag, float32 alpha x 3, float32 (1 - alpha) x 3, 2 unused.
    torch multiplies a float32 tensor by a Python float in float32, so alpha and the float64 difference 1 - alpha
    (blend, :248) are rounded to float32 separately."""
    words = np.zeros((len(color), 12), dtype=np.int32)
    fl = words.view(np.float32)
    for b, cp in enumerate(color):
        if cp is None:
            continue
        if len(cp.stages) > 3:
            raise ValueError("at most three colour stages per clip")
        for i, (code, alpha) in enumerate(cp.stages):
            words[b, i] = code
            fl[b, 4 + i] = np.float32(alpha)
            fl[b, 7 + i] = np.float32(1 - alpha)
        words[b, 3] = int(cp.gray)
    return words


def clip_augmentation_batch(clips, params, crop_size, out=None, color=None):
    """clips: list of uint8 device tensors T x H x W x 3 (same T; H, W may differ per clip), or one B x T x H x W x 3
    tensor.  params: per clip (resized H, resized W, y offset, x offset, flip).  color: None, or per clip a ColorParams
    (None for a clip without colour work).  -> B x 3 x T x S x S float32."""
    if torch.is_tensor(clips):
        assert clips.dtype == torch.uint8 and clips.dim() == 5 and clips.shape[-1] == 3 and clips.is_cuda
        B, T, H, W = clips.shape[:4]
        buf = clips.contiguous()
        shapes = [(H, W)] * B
        offs = [b * T * H * W * 3 for b in range(B)]
    else:
        B = len(clips)
        T = clips[0].shape[0]
        shapes, offs, o = [], [], 0
        for c in clips:
            assert c.dtype == torch.uint8 and c.dim() == 4 and c.shape[-1] == 3 and c.shape[0] == T and c.is_cuda
            shapes.append((c.shape[1], c.shape[2]))
            offs.append(o)
            o += c.numel()
        buf = torch.cat([c.reshape(-1) for c in clips])
    desc = np.zeros((B, 8), dtype=np.int64)
    for b, ((H, W), (nh, nw, yo, xo, flip)) in enumerate(zip(shapes, params)):
        if not (0 <= yo and yo + crop_size <= nh and 0 <= xo and xo + crop_size <= nw):
            raise ValueError("crop window outside the resized frame")
        desc[b] = (offs[b], H, W, nh, nw, yo, xo, int(flip))
    if color is not None and len(color) != B:
        raise ValueError("one colour-parameter object (or None) per clip")
    words = None if color is None else _color_desc(color)
    # one upload: the spatial descriptors, then (colour path) the colour words behind them
    host = desc.view(np.uint8).reshape(-1) if words is None else \
        np.concatenate([desc.view(np.uint8).reshape(-1), words.view(np.uint8).reshape(-1)])
    dev = torch.from_numpy(host).to(buf.device, non_blocking=False)
    if out is None:
        out = torch.empty((B, 3, T, crop_size, crop_size), dtype=torch.float32, device=buf.device)
    assert out.shape == (B, 3, T, crop_size, crop_size) and out.dtype == torch.float32
    if words is None:
        C.slv_clip_augment(ptr(buf), ptr(dev), ptr(out), B, T, crop_size, _MEAN.ctypes.data, _STD.ctypes.data, stream())
        return out
    ws = None
    if (words[:, :3] == CONTRAST).any():
        ws = torch.empty((B, T), dtype=torch.float32, device=buf.device)
    C.slv_clip_augment_color(ptr(buf), ptr(dev), ptr(dev) + desc.nbytes, words.ctypes.data, ptr(ws), ptr(out), B, T,
                             crop_size, _MEAN.ctypes.data, _STD.ctypes.data, stream())
    return out


def _video_layout(videos):
    """-> (base pointer, device, per video (byte offset from the base, N, H, W)).
    A list of tensors is addressed in place: the offsets are the distances of the tensors' data pointers from the first
    one's (the device address space is flat), so no packed copy of the videos is made.  ``(buf, offsets, shapes)``: one
    flat uint8 device buffer, the byte offset of each video in it and its (N, H, W)."""
    if isinstance(videos, tuple):
        buf, offs, shapes = videos
        assert torch.is_tensor(buf) and buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_cuda
        if len(offs) != len(shapes):
            raise ValueError("one offset and one (N, H, W) per video")
        lay = []
        for o, (N, H, W) in zip(offs, shapes):
            if o < 0 or N <= 0 or o + N * H * W * 3 > buf.numel():
                raise ValueError("a video lies outside the frame buffer")
            lay.append((int(o), int(N), int(H), int(W)))
        return ptr(buf), buf.device, lay
    videos = list(videos)
    lay = []
    for v in videos:
        assert v.dtype == torch.uint8 and v.dim() == 4 and v.shape[-1] == 3 and v.is_cuda and v.shape[0] > 0
        assert v.device == videos[0].device
        lay.append((ptr(v) - ptr(videos[0]), v.shape[0], v.shape[1], v.shape[2]))
    return ptr(videos[0]), videos[0].device, lay


def clip_sample_augmentation_batch(videos, frame_idx, params, crop_size, out=None, color=None, video_of=None):
    """temporal_sampling + clip_augmentation in one launch chain, from whole decoded videos.

    videos: list of uint8 device tensors N_i x H_i x W_i x 3, or ``(buf, offsets, shapes)`` (see _video_layout).
    frame_idx: B x T integers (array, tensor or rows), the frames of each output clip inside ITS video.
    video_of: per output clip the index of its video (default: clip b is cut from video b); several clips may name one
    video.  params / color / out: as in clip_augmentation_batch, per output clip.  -> B x 3 x T x S x S float32, equal
    bit for bit to clip_augmentation_batch on the gathered clips."""
    base, device, lay = _video_layout(videos)
    if not torch.is_tensor(frame_idx) and len(frame_idx) and torch.is_tensor(frame_idx[0]):
        frame_idx = torch.stack(list(frame_idx))
    fidx = np.ascontiguousarray(frame_idx.cpu().numpy() if torch.is_tensor(frame_idx) else np.asarray(frame_idx))
    if fidx.ndim != 2 or fidx.dtype.kind not in "iu":
        raise ValueError("frame_idx: B x T integers")
    B, T = fidx.shape
    video_of = list(range(B)) if video_of is None else [int(v) for v in video_of]
    if len(video_of) != B or len(params) != B or any(not 0 <= v < len(lay) for v in video_of):
        raise ValueError("one video index and one spatial parameter set per output clip")
    n_frames = np.array([lay[v][1] for v in video_of], dtype=np.int64)
    if (fidx < 0).any() or (fidx >= n_frames[:, None]).any():
        raise ValueError("frame index outside the video")
    fidx = fidx.astype(np.int32)
    desc = np.zeros((B, 8), dtype=np.int64)
    for b, (v, (nh, nw, yo, xo, flip)) in enumerate(zip(video_of, params)):
        if not (0 <= yo and yo + crop_size <= nh and 0 <= xo and xo + crop_size <= nw):
            raise ValueError("crop window outside the resized frame")
        off, _, H, W = lay[v]
        desc[b] = (off, H, W, nh, nw, yo, xo, int(flip))
    if color is not None and len(color) != B:
        raise ValueError("one colour-parameter object (or None) per clip")
    words = None if color is None else _color_desc(color)
    # one upload: the spatial descriptors, the frame table, then (colour path) the colour words
    parts = [desc.view(np.uint8).reshape(-1), fidx.view(np.uint8).reshape(-1)]
    if words is not None:
        parts.append(words.view(np.uint8).reshape(-1))
    dev = torch.from_numpy(np.concatenate(parts)).to(device, non_blocking=False)
    d_fidx = ptr(dev) + desc.nbytes
    if out is None:
        out = torch.empty((B, 3, T, crop_size, crop_size), dtype=torch.float32, device=device)
    assert out.shape == (B, 3, T, crop_size, crop_size) and out.dtype == torch.float32 and out.is_cuda
    if words is None:
        C.slv_clip_sample_augment(base, ptr(dev), d_fidx, fidx.ctypes.data, n_frames.ctypes.data, ptr(out), B, T,
                                  crop_size, _MEAN.ctypes.data, _STD.ctypes.data, stream())
        return out
    ws = None
    if (words[:, :3] == CONTRAST).any():
        ws = torch.empty((B, T), dtype=torch.float32, device=device)
    C.slv_clip_sample_augment_color(base, ptr(dev), d_fidx, fidx.ctypes.data, n_frames.ctypes.data,
                                    d_fidx + fidx.nbytes, words.ctypes.data, ptr(ws), ptr(out), B, T, crop_size,
                                    _MEAN.ctypes.data, _STD.ctypes.data, stream())
    return out


class ClipAugmenter:
    """clip_augmentation (:462-504) for a batch on the device, with the reference's keyword names.  Called on a
    B x T x H x W x 3 uint8 device tensor or a list of T x H x W x 3 ones; ``spatial_idx`` in the call (an int or one
    per clip) overrides the constructor's for the test-time views.  Per clip, in clip order, it draws exactly what the
    reference's worker draws for that clip: the spatial draws, then the colour draws.  use_gaussian is accepted and
    unused, like in the reference (no draw, no effect).  -> B x 3 x T x S x S float32."""

    def __init__(self, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224, colorjitter=False,
                 use_grayscale=False, use_gaussian=False):
        self.spatial_idx, self.min_scale, self.max_scale, self.crop_size = spatial_idx, min_scale, max_scale, crop_size
        self.colorjitter, self.use_grayscale, self.use_gaussian = bool(colorjitter), bool(use_grayscale), use_gaussian

    def sample(self, shapes, spatial_idx=None):
        """shapes: (H, W) per clip -> (spatial params per clip, ColorParams per clip or None when both flags are off)."""
        sidx = self.spatial_idx if spatial_idx is None else spatial_idx
        if isinstance(sidx, (int, np.integer)):
            sidx = [int(sidx)] * len(shapes)
        sidx = [int(i) for i in sidx]
        if len(sidx) != len(shapes):
            raise ValueError("one spatial_idx per clip")
        with_color = self.colorjitter or self.use_grayscale
        params, color = [], []
        for (H, W), si in zip(shapes, sidx):
            params.append(sample_spatial_params(H, W, si, self.min_scale, self.max_scale, self.crop_size))
            if with_color:
                color.append(sample_color_params(self.colorjitter, self.use_grayscale))
        return params, (color if with_color else None)

    def __call__(self, clips, spatial_idx=None, out=None):
        if torch.is_tensor(clips):
            shapes = [(clips.shape[2], clips.shape[3])] * clips.shape[0]
        else:
            shapes = [(c.shape[1], c.shape[2]) for c in clips]
        params, color = self.sample(shapes, spatial_idx)
        return clip_augmentation_batch(clips, params, self.crop_size, out=out, color=color)


def clip_augmentation(frames, spatial_idx=-1, min_scale=256, max_scale=320, crop_size=224, colorjitter=False,
                      use_grayscale=False, use_gaussian=False):
    """One clip, the reference's signature (:462-471): frames T x H x W x 3 uint8 (device) -> 3 x T x S x S float32."""
    if colorjitter or use_grayscale or use_gaussian:
        raise NotImplementedError("the single-clip entry point covers the spatial part only: use ClipAugmenter("
                                  "..., colorjitter=, use_grayscale=, use_gaussian=) for colour jitter / grayscale")
    prm = sample_spatial_params(frames.shape[1], frames.shape[2], spatial_idx, min_scale, max_scale, crop_size)
    return clip_augmentation_batch([frames], [prm], crop_size)[0]
