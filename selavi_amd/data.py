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
