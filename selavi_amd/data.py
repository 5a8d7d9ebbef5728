"""Synthetic stand-in for the reference's AVideoDataset output contract
(datasets/AVideoDataset.py:355-454): ``dataset[i] -> (frames[3,T,H,W], spec[1,F,T'], label, index, vid_idx)``.
Deterministic per index (counter-based), generated on the host; used by tests, smoke and bench."""
import torch


class SyntheticAVDataset(torch.utils.data.Dataset):
    def __init__(self, n=3328, T=8, S=112, F=40, Tp=100, n_classes=28, seed=31, device=None):
        self.n, self.T, self.S, self.F, self.Tp, self.seed = n, T, S, F, Tp, seed
        g = torch.Generator().manual_seed(seed)
        self._labels = torch.randint(0, n_classes, (n,), generator=g).tolist()
        self.valid_indices = list(range(n))
        self.n_classes = n_classes
        self.device = device

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + int(i))
        lab = self._labels[i]
        # class-dependent mean so that clusters are learnable, unit variance like the normalised real data
        video = torch.randn(3, self.T, self.S, self.S, generator=g) + 0.25 * ((lab % 7) - 3)
        audio = torch.randn(1, self.F, self.Tp, generator=g) + 0.25 * ((lab % 5) - 2)
        return video, audio, lab, i, i


class SyntheticRetrievalDataset(torch.utils.data.Dataset):
    """Stand-in for the retrieval datasets of the reference (AVideoDataset with decode_audio=False,
    src/retrieval_utils.py:104-145): ``dataset[i] -> (frames[3,T,S,S], label, clip_idx, vid_idx)`` for clip ``clip_idx``
    of video ``vid_idx = i // clips_per_video``.  A clip is a class pattern (the same for every dataset built with the same
    ``n_classes``, so a train and a test set share it) plus a pattern of its video plus noise of its own: clips of one video
    look alike, videos of one class less so.  Deterministic per index."""

    def __init__(self, n_videos=64, clips_per_video=2, T=16, S=112, n_classes=8, seed=31):
        self.n_videos, self.clips_per_video, self.T, self.S = n_videos, clips_per_video, T, S
        self.n_classes, self.seed = n_classes, seed
        g = torch.Generator().manual_seed(seed)
        self._labels = torch.randint(0, n_classes, (n_videos,), generator=g).tolist()

    def __len__(self):
        return self.n_videos * self.clips_per_video

    def _pattern(self, key, scale):
        g = torch.Generator().manual_seed(key)
        coarse = torch.randn(3, max(self.T // 4, 1), max(self.S // 16, 1), max(self.S // 16, 1), generator=g)
        return scale * torch.nn.functional.interpolate(coarse[None], size=(self.T, self.S, self.S), mode="nearest")[0]

    def __getitem__(self, i):
        vid, clip = divmod(int(i), self.clips_per_video)
        lab = self._labels[vid]
        g = torch.Generator().manual_seed((self.seed * 1000003 + int(i)) * 7 + 1)
        video = (self._pattern(9176 + lab, 1.0) + self._pattern((self.seed * 1000003 + vid) * 7 + 2, 0.5)
                 + 0.5 * torch.randn(3, self.T, self.S, self.S, generator=g))
        return video, lab, clip, vid


class SyntheticFramesDataset(SyntheticRetrievalDataset):
    """The same clips as decoded frames: ``dataset[i] -> (frames[T,H,W,3] uint8, label, clip_idx, vid_idx)``, what a
    video decoder hands to clip_augmentation (datasets/video_transforms.py).  The float clip is generated at
    max(H, W) square, cut to H x W, de-normalised with the pipeline's mean / std and rounded to bytes."""

    def __init__(self, H, W, **kw):
        super().__init__(S=max(H, W), **kw)
        self.H, self.W = H, W

    def __getitem__(self, i):
        video, lab, clip, vid = super().__getitem__(i)
        frames = ((video[:, :, :self.H, :self.W] * 0.225 + 0.45) * 255.0).round().clamp(0, 255).to(torch.uint8)
        return frames.permute(1, 2, 3, 0).contiguous(), lab, clip, vid


class SyntheticVideoDataset(SyntheticRetrievalDataset):
    """Whole decoded videos, what a decoder hands over before any temporal sampling: item ``i`` is sample
    ``i % clips_per_video`` of video ``vid_idx = i // clips_per_video`` (the reference's AVideoDataset lists every video
    num_clips times, AVideoDataset.py:296-306) -> ``(video[N,H,W,3] uint8, fps, label, spatial_temporal_idx, vid_idx)``,
    with ``with_audio`` -> ``(video, wav int16 [n], fps, label, spatial_temporal_idx, vid_idx)``.  Lengths, frame sizes
    (landscape and portrait) and frame rates differ from video to video; the pixels are the class / video patterns of
    SyntheticRetrievalDataset, so the sets are learnable.  ``decoded_videos`` tells a driver to cut its clips with
    datasets.av_batcher.DecodedAVBatcher; ``collate`` keeps one copy of a video that several items of a batch name."""
    decoded_videos = True

    def __init__(self, n_videos=16, clips_per_video=1, min_frames=12, max_frames=40, S=40, n_classes=8, seed=31,
                 with_audio=False, aud_sample_rate=48000):
        super().__init__(n_videos=n_videos, clips_per_video=clips_per_video, T=max_frames, S=S * 3 // 2,
                         n_classes=n_classes, seed=seed)
        g = torch.Generator().manual_seed(seed + 77)
        self.n_frames = torch.randint(min_frames, max_frames + 1, (n_videos,), generator=g).tolist()
        self.fps = [(24.0, 25.0, 29.97, 30.0)[k] for k in torch.randint(0, 4, (n_videos,), generator=g).tolist()]
        sizes = ((S * 5 // 4, S * 3 // 2), (S * 3 // 2, S * 5 // 4), (S * 5 // 4, S * 5 // 4))
        self.sizes = [sizes[k] for k in torch.randint(0, 3, (n_videos,), generator=g).tolist()]
        self.with_audio, self.aud_sample_rate = with_audio, aud_sample_rate

    def video(self, vid):
        lab = self._labels[vid]
        N, (H, W) = self.n_frames[vid], self.sizes[vid]
        g = torch.Generator().manual_seed((self.seed * 1000003 + vid) * 7 + 3)
        x = (self._pattern(9176 + lab, 1.0) + self._pattern((self.seed * 1000003 + vid) * 7 + 2, 0.5))[:, :N, :H, :W]
        x = x + 0.5 * torch.randn(3, N, H, W, generator=g)
        return ((x * 0.225 + 0.45) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 3, 0).contiguous()

    def wav(self, vid):
        seconds = self.n_frames[vid] / self.fps[vid] + 1.5          # longer than the video by more than one window
        g = torch.Generator().manual_seed((self.seed * 1000003 + vid) * 7 + 4)
        return (torch.randn(int(seconds * self.aud_sample_rate), generator=g) * 3000).to(torch.int16)

    def __getitem__(self, i):
        vid, clip = divmod(int(i), self.clips_per_video)
        head = (self.video(vid), self.wav(vid)) if self.with_audio else (self.video(vid),)
        return head + (self.fps[vid], self._labels[vid], clip, vid)

    @staticmethod
    def collate(items):
        """-> (videos, [wavs,] fps, video_of, labels, spatial_temporal_idx, vid_idx): the first lists hold one entry per
        distinct video of the batch, ``video_of`` maps each item to its entry, the last three are int64 tensors."""
        slot, cols = {}, [[] for _ in range(len(items[0]) - 3)]
        video_of = []
        for it in items:
            vid = it[-1]
            if vid not in slot:
                slot[vid] = len(slot)
                for c, x in zip(cols, it[:-3]):
                    c.append(x)
            video_of.append(slot[vid])
        tail = [torch.tensor([it[k] for it in items], dtype=torch.int64) for k in (-3, -2, -1)]
        return (*cols, video_of, *tail)
