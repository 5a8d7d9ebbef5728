"""The temporal half of the reference's datasets/decoder.py (:21-69, :392) without the decoding: where a clip starts in a
decoded video and which frames it takes.

Demuxing and decoding are out of scope; a caller holds whole decoded videos.  ``get_start_end_idx`` draws the clip
window with Python's ``random.uniform`` like the reference; ``frame_indices`` is the index row ``temporal_sampling``
gathers with -- the same ``torch.linspace`` / clamp / ``.long()`` on the CPU, so the indices are the reference's by
construction.  On the device the row feeds slv_clip_sample_augment (video_transforms.clip_sample_augmentation_batch),
which reads those frames straight from the video; ``temporal_sampling`` is the stand-alone gather.
"""
import random

import torch


def clip_size(num_frames, sampling_rate, fps, target_fps):
    """Frames of the source video a clip spans (decoder.py:392)."""
    return num_frames * sampling_rate * fps / target_fps


def get_start_end_idx(video_size, clip_size, clip_idx, num_clips):
    """(start_idx, end_idx) of a clip of ``clip_size`` frames in a video of ``video_size`` frames (decoder.py:41-69).
    clip_idx -1: one ``random.uniform(0, delta)`` draw; otherwise clip ``clip_idx`` of ``num_clips`` evenly spaced ones
    (no draw).  start_idx is a float in the random case."""
    delta = max(video_size - clip_size, 0)
    start_idx = random.uniform(0, delta) if clip_idx == -1 else int(delta * clip_idx / num_clips)
    return start_idx, start_idx + clip_size - 1


def frame_indices(n_frames, start_idx, end_idx, num_samples):
    """int64 [num_samples]: the frames temporal_sampling takes from a video of ``n_frames`` frames (decoder.py:35-36)."""
    index = torch.linspace(start_idx, end_idx, num_samples)
    return torch.clamp(index, 0, n_frames - 1).long()


def temporal_sampling(frames, start_idx, end_idx, num_samples):
    """``num_samples`` equally spaced frames of ``frames`` (N x ...) between start_idx and end_idx (decoder.py:21-38)."""
    index = frame_indices(frames.shape[0], start_idx, end_idx, num_samples)
    return torch.index_select(frames, 0, index.to(frames.device))
