"""From decoded videos to the tensors the model eats, for a whole batch: the part of the reference's
AVideoDataset.__getitem__ (datasets/AVideoDataset.py:355-454) and decoder.decode (datasets/decoder.py:300-398) that runs
after demuxing and decoding.

Per sample the reference picks a clip window, takes ``num_frames`` frames from it, augments them, and cuts the audio
window at the clip's start; under ``dual_data`` it does so twice and concatenates, in test mode the item's index names
one of ``num_ensemble_views x num_spatial_crops`` deterministic views.  DecodedAVBatcher makes the same random draws on
the host, per sample and per clip in the order the reference's worker makes them --

  1. the clip window: ``random.uniform(0, delta)`` (decoder.get_start_end_idx; train / val mode with temp_jitter),
  2. the audio draws of get_spec: the temporal jitter, then the volume (np.random),
  3. the spatial draws (video_transforms.sample_spatial_params),
  4. the colour draws (video_transforms.sample_color_params)

-- and then runs ONE video launch chain (slv_clip_sample_augment[_color]: the frames are read straight from the whole
videos through a frame table, every clip is written to its place in the output) and ONE audio launch (slv_logfbank).

The reference's decoder has two branches.  Where the container tells the stream's duration it decodes only the clip
window (pyav_decode, decoder.py:243-254) and the audio starts at that window's ``start_idx / fps`` (:275).  Where it
does not, the whole video is decoded and ``start_idx`` is never assigned before :275 reads it, so the audio of that
branch is undefined.  The batcher follows the selective-decoding branch: the decoded window is the clip window, i.e.
the window is drawn once, on the whole video's frame count, the frames are
``decoder.frame_indices(n_frames, start_idx, end_idx, num_frames)`` of the whole video, and the audio window starts at
``start_idx / fps``.

One expression is not that branch's: the span of a clip is ``decoder.clip_size``, the association of decoder.py:392
(``num_frames * sampling_rate * fps / target_fps``), where pyav_decode's own window (:247) writes
``sampling_rate * num_frames / target_fps * fps``.  For a fractional fps the two can differ by one float64 ulp, and with
them ``delta``, a drawn ``start_idx`` and the audio start; tests/golden/decoder_sampling.npz pins the :392 form.

A clip that starts less than 0.5 s into its video can, under ``use_temporal_jittering``, get an audio window that starts
before the recording.  The reference slices ``wav[negative:to]`` there, gets an empty signal and drops the sample as bad
audio, so it defines no output to mirror.  The batcher keeps the policy of audio_utils.get_spec / window: ValueError, for
the whole batch, before anything is launched -- a caller that trains with temporal jitter catches it and redraws.
"""
import numpy as np
import torch

from . import audio_utils, decoder
from .video_transforms import clip_sample_augmentation_batch, sample_color_params, sample_spatial_params


class Plan:
    """The draws and tables of one batch, one entry per output CLIP (a dual_data sample has two, back to back):
    ``video_of`` index of the clip's video, ``start_idx`` / ``end_idx`` the window, ``fidx`` n_clips x T int32 frame
    table, ``params`` spatial parameters, ``color`` ColorParams per clip or None (both flags off), ``audio_start`` first
    sample of the audio window and ``volume`` factor per clip (None: no audio / no volume jitter), ``crop_size``."""
    __slots__ = ("video_of", "start_idx", "end_idx", "fidx", "params", "color", "audio_start", "volume", "crop_size")

    def __init__(self, crop_size):
        self.video_of, self.start_idx, self.end_idx, self.fidx, self.params = [], [], [], None, []
        self.color, self.audio_start, self.volume, self.crop_size = None, None, None, crop_size


class DecodedAVBatcher:
    """AVideoDataset's sampling and augmentation on decoded videos, with the keyword names of AVideoDataset.__init__
    that matter after decoding.  ``train_jitter_scles`` None: the reference's rule (:213-217).  ``use_gaussian`` is
    accepted and unused, like in the reference.  ``aud_spec_type`` 1: 40 mel bands, otherwise 257.

    ``batcher(videos, fps, wavs=None, spatial_temporal_idx=None, video_of=None) -> (frames, audio or None)``
      videos   list of uint8 device tensors N_i x H_i x W_i x 3 (whole decoded videos), or the (buf, offsets, shapes)
               form of video_transforms.clip_sample_augmentation_batch
      fps      frames per second of each video
      wavs     with decode_audio: per video a 1-D int16 device tensor (or one R x n tensor)
      video_of per SAMPLE the index of its video (default: sample i is video i); a video named by several samples is
               resident once -- the test views of one video
      spatial_temporal_idx   test mode: per sample the item's index among the num_ensemble_views x num_spatial_crops
               views of its video (AVideoDataset.py:370-380)
      frames   n_samples x 3 x T x S x S float32 (dual_data: x 6 x, the reference's torch.cat(dim=0) of the sample's two
               clips); audio n_samples x 1 x nfilt x frames (dual_data: x 2 x)

    Raises ValueError before any launch when an audio window does not fit its recording (a recording shorter than
    num_sec, or -- see the module docstring -- a negative temporal jitter at the very start of a video).

    ``plan(...)`` returns the draws and tables without touching the device.  ``calls`` / ``clips`` count the batches and
    output clips cut so far."""

    def __init__(self, mode='train', num_frames=30, sample_rate=1, train_crop_size=112, test_crop_size=112,
                 num_spatial_crops=3, num_ensemble_views=10, colorjitter=False, use_grayscale=False, use_gaussian=False,
                 dual_data=False, temp_jitter=True, center_crop=False, target_fps=30, decode_audio=True, num_sec=1,
                 aud_sample_rate=48000, aud_spec_type=1, use_volume_jittering=False, use_temporal_jittering=False,
                 z_normalize=False, train_jitter_scles=None):
        if mode not in ("train", "val", "test"):
            raise ValueError(f"Split '{mode}' not supported")
        self.mode, self.num_frames, self.sample_rate = mode, int(num_frames), sample_rate
        self.train_crop_size, self.test_crop_size = train_crop_size, test_crop_size
        if train_jitter_scles is None:
            train_jitter_scles = (128, 160) if train_crop_size in (112, 128) else (256, 320)
        self.train_jitter_scles = tuple(train_jitter_scles)
        self.num_spatial_crops, self.num_ensemble_views = num_spatial_crops, num_ensemble_views
        self.colorjitter, self.use_grayscale, self.use_gaussian = bool(colorjitter), bool(use_grayscale), use_gaussian
        self.dual_data, self.temp_jitter, self.center_crop = bool(dual_data), bool(temp_jitter), bool(center_crop)
        self.target_fps, self.decode_audio = int(target_fps), bool(decode_audio)
        self.num_sec, self.aud_sample_rate, self.aud_spec_type = int(num_sec), aud_sample_rate, aud_spec_type
        self.use_volume_jittering = bool(use_volume_jittering)
        self.use_temporal_jittering = bool(use_temporal_jittering)
        self.z_normalize = bool(z_normalize)
        self.calls = self.clips = 0

    @property
    def clips_per_sample(self):
        return 2 if self.mode in ("train", "val") and self.dual_data else 1

    def _sample_setup(self, st_idx):
        """(temporal index, spatial index, min scale, max scale, crop) of one sample (AVideoDataset.py:358-383)."""
        if self.mode in ("train", "val"):
            if self.center_crop:
                return -1, 1, self.train_crop_size, self.train_crop_size, self.train_crop_size
            return -1, -1, self.train_jitter_scles[0], self.train_jitter_scles[1], self.train_crop_size
        if st_idx is None:
            raise ValueError("test mode: spatial_temporal_idx names the view of every sample")
        st_idx = int(st_idx)
        if not 0 <= st_idx < self.num_ensemble_views * self.num_spatial_crops:
            raise ValueError("spatial_temporal_idx outside num_ensemble_views x num_spatial_crops")
        c = self.test_crop_size
        return st_idx // self.num_spatial_crops, st_idx % self.num_spatial_crops, c, c, c

    def plan(self, shapes, fps, n_audio_samples=None, spatial_temporal_idx=None, video_of=None):
        """shapes: (N, H, W) per video; n_audio_samples: per video the length of its recording (decode_audio)."""
        n_samples = len(shapes) if video_of is None else len(video_of)
        video_of = list(range(n_samples)) if video_of is None else [int(v) for v in video_of]
        if any(not 0 <= v < len(shapes) for v in video_of) or len(fps) != len(shapes):
            raise ValueError("video_of names a video that is not there, or fps is not one per video")
        if spatial_temporal_idx is None:
            spatial_temporal_idx = [None] * n_samples
        if len(spatial_temporal_idx) != n_samples:
            raise ValueError("one spatial_temporal_idx per sample")
        if self.decode_audio and (n_audio_samples is None or len(n_audio_samples) != len(shapes)):
            raise ValueError("decode_audio: one recording per video")
        with_color = self.colorjitter or self.use_grayscale
        plan, rows = None, []
        for v, st in zip(video_of, spatial_temporal_idx):
            N, H, W = shapes[v]
            t_idx, s_idx, lo, hi, crop = self._sample_setup(st)
            if plan is None:
                plan = Plan(crop)
                plan.color = [] if with_color else None
                plan.audio_start = [] if self.decode_audio else None
                plan.volume = [] if self.decode_audio and self.use_volume_jittering else None
            for _ in range(self.clips_per_sample):
                size = decoder.clip_size(self.num_frames, self.sample_rate, float(fps[v]), self.target_fps)
                start, end = decoder.get_start_end_idx(N, size, t_idx if self.temp_jitter else 500,
                                                       self.num_ensemble_views if self.temp_jitter else 1000)
                if self.decode_audio:                                   # decoder.py:275 -> audio_utils.py:25-43
                    plan.audio_start.append(audio_utils.window(n_audio_samples[v], start / float(fps[v]), self.num_sec,
                                                               self.aud_sample_rate, self.use_temporal_jittering))
                    if self.use_volume_jittering:
                        plan.volume.append(np.random.uniform(0.9, 1.1))
                plan.params.append(sample_spatial_params(H, W, s_idx, lo, hi, crop))
                if with_color:
                    plan.color.append(sample_color_params(self.colorjitter, self.use_grayscale))
                plan.video_of.append(v)
                plan.start_idx.append(start)
                plan.end_idx.append(end)
                rows.append(decoder.frame_indices(N, start, end, self.num_frames))
        if plan is None:
            raise ValueError("an empty batch")
        plan.fidx = torch.stack(rows).numpy().astype(np.int32)
        return plan

    def __call__(self, videos, fps, wavs=None, spatial_temporal_idx=None, video_of=None):
        if isinstance(videos, tuple):
            shapes = [tuple(int(x) for x in s) for s in videos[2]]
        else:
            shapes = [tuple(v.shape[:3]) for v in videos]
        n_audio = None
        if self.decode_audio:
            if wavs is None:
                raise ValueError("decode_audio=True: pass the recordings")
            n_audio = [wavs.shape[1]] * wavs.shape[0] if torch.is_tensor(wavs) else [w.numel() for w in wavs]
        plan = self.plan(shapes, fps, n_audio, spatial_temporal_idx, video_of)
        n_clips, k, S, T = len(plan.video_of), self.clips_per_sample, plan.crop_size, self.num_frames
        device = videos[0].device
        # a dual_data sample's two clips are rows 2i, 2i + 1 of the kernel's output: the same memory as i x 6 x T x S x S
        frames = torch.empty((n_clips // k, 3 * k, T, S, S), dtype=torch.float32, device=device)
        clip_sample_augmentation_batch(videos, plan.fidx, plan.params, S, out=frames.view(n_clips, 3, T, S, S),
                                       color=plan.color, video_of=plan.video_of)
        audio = None
        if self.decode_audio:
            if torch.is_tensor(wavs):
                wav = wavs
            elif len({w.numel() for w in wavs}) == 1:
                wav = torch.stack([w.reshape(-1) for w in wavs])
            else:                                # ragged recordings: zero-padded rows (a window never reaches the padding)
                wav = torch.zeros((len(wavs), max(n_audio)), dtype=torch.int16, device=device)
                for i, w in enumerate(wavs):
                    wav[i, :w.numel()] = w.reshape(-1)
            spec = audio_utils.get_spec_batch(wav, plan.audio_start, self.num_sec, self.aud_sample_rate,
                                              self.aud_spec_type, plan.volume, self.z_normalize, rows=plan.video_of,
                                              lengths=n_audio)
            audio = spec.view(n_clips // k, k, spec.shape[2], spec.shape[3])
        self.calls += 1
        self.clips += n_clips
        return frames, audio
