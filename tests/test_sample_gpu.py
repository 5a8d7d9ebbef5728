"""Clips cut from whole decoded videos on the device (csrc/input.hip: slv_clip_sample_augment[_color],
video_transforms.clip_sample_augmentation_batch, datasets.av_batcher.DecodedAVBatcher, finetune_video on
``--dataset synthetic_video``) against the path that was there before: gather the clip, then clip_augmentation_batch /
ClipAugmenter / get_spec -- which tests/test_input_gpu.py and tests/test_color_gpu.py pin to the executed reference.
Same arithmetic, same reduction order: every comparison is bit for bit."""
import random

import numpy as np
import pytest
import torch

from oracle import input_ref
from selavi_amd import _lib
from selavi_amd.datasets import audio_utils, decoder
from selavi_amd.datasets import video_transforms as VT
from selavi_amd.datasets.av_batcher import DecodedAVBatcher

pytestmark = pytest.mark.gpu

T, S = 6, 64
SHAPES = [(23, 72, 96), (4, 96, 72), (40, 80, 80), (9, 72, 128), (17, 96, 128)]      # (frames, H, W): ragged


def _videos(seed=5, shapes=SHAPES):
    g = np.random.RandomState(seed)
    return [torch.from_numpy(g.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)).cuda() for n, h, w in shapes]


def _case():
    """Eleven output clips of five videos: several clips of one video, a video shorter than the clip (repeated and
    clamped indices), the two clips of a dual_data sample (video 2, neighbours), test views with and without flip."""
    video_of = [0, 1, 2, 2, 3, 0, 4, 4, 4, 1, 0]
    fidx = np.array([[0, 3, 7, 11, 15, 22],
                     [0, 0, 1, 2, 3, 3],                       # a 4-frame video: repeated indices
                     [5, 6, 7, 8, 9, 10],
                     [34, 35, 36, 37, 38, 39],
                     [8, 8, 8, 8, 8, 8],
                     [22, 18, 13, 9, 4, 0],                    # any order is a valid table
                     [2, 5, 8, 11, 14, 16],
                     [2, 5, 8, 11, 14, 16],                    # the same frames, another crop of the view
                     [2, 5, 8, 11, 14, 16],
                     [3, 3, 3, 3, 3, 3],
                     [1, 2, 3, 4, 5, 6]], dtype=np.int64)
    sidx = [-1, -1, -1, -1, -1, -1, 0, 1, 5, 4, -1]            # views 5 and 4 are flipped
    np.random.seed(17)
    params = []
    for v, si in zip(video_of, sidx):
        _, h, w = SHAPES[v]
        lo, hi = (S, S) if si >= 0 else (S, 80)
        params.append(VT.sample_spatial_params(h, w, si, lo, hi, S))
    assert params[8][4] and params[9][4] and not params[6][4]
    color = [None,
             VT.ColorParams([(VT.CONTRAST, 1.31), (VT.SATURATION, 0.72), (VT.BRIGHTNESS, 0.9)]),
             VT.ColorParams([(VT.SATURATION, 0.61), (VT.BRIGHTNESS, 1.39), (VT.CONTRAST, 0.8)], gray=True),
             VT.ColorParams([(VT.BRIGHTNESS, 1.2), (VT.CONTRAST, 0.65), (VT.SATURATION, 1.1)]),
             VT.ColorParams(gray=True),
             VT.ColorParams(),
             VT.ColorParams([(VT.CONTRAST, 0.7)]),
             VT.ColorParams([(VT.SATURATION, 1.25)]),
             VT.ColorParams([(VT.BRIGHTNESS, 0.8), (VT.SATURATION, 1.3), (VT.CONTRAST, 1.2)]),
             VT.ColorParams([(VT.CONTRAST, 1.4), (VT.BRIGHTNESS, 0.95)]),
             None]
    return video_of, fidx, params, color


def _gathered(videos, video_of, fidx):
    """Today's path: one index_select per clip."""
    return [torch.index_select(videos[v], 0, torch.as_tensor(row, device="cuda")) for v, row in zip(video_of, fidx)]


@pytest.mark.parametrize("with_color", [False, True])
def test_fused_path_equals_gather_then_augment_bit_for_bit(with_color):
    videos = _videos()
    video_of, fidx, params, color = _case()
    color = color if with_color else None
    want = VT.clip_augmentation_batch(_gathered(videos, video_of, fidx), params, S, color=color)
    got = VT.clip_sample_augmentation_batch(videos, fidx, params, S, color=color, video_of=video_of)
    assert got.shape == (11, 3, T, S, S) and got.dtype == torch.float32
    for b in range(11):
        assert torch.equal(got[b], want[b]), b
    assert not torch.equal(got[6], got[7])                     # two crops of one view
    # a second launch into a poisoned buffer: the same bits, every word written
    again = VT.clip_sample_augmentation_batch(videos, torch.from_numpy(fidx), params, S, color=color, video_of=video_of,
                                              out=torch.full_like(got, float("nan")))
    assert torch.equal(again, got)
    # one flat buffer plus offsets: the videos in another order, with a gap between them
    order, offs, o = [3, 0, 4, 2, 1], {}, 7
    for v in order:
        offs[v] = o
        o += videos[v].numel() + 5
    buf = torch.zeros(o, dtype=torch.uint8, device="cuda")
    for v in order:
        buf[offs[v]:offs[v] + videos[v].numel()] = videos[v].reshape(-1)
    flat = VT.clip_sample_augmentation_batch((buf, [offs[v] for v in range(5)], SHAPES), fidx, params, S, color=color,
                                             video_of=video_of)
    assert torch.equal(flat, got)
    # the default video_of: clip b from video b; against the oracle directly where no colour is involved
    one = VT.clip_sample_augmentation_batch(videos[:2], fidx[:2], params[:2], S)
    assert torch.equal(one, VT.clip_augmentation_batch(_gathered(videos, [0, 1], fidx[:2]), params[:2], S))
    nh, nw, yo, xo, fl = params[0]
    ref = input_ref.clip_augmentation_ref(videos[0].cpu().numpy()[fidx[0]], (nh, nw), yo, xo, fl, S)
    assert np.array_equal(one[0].cpu().numpy(), ref)


def test_old_entry_points_are_unchanged_by_the_frame_table_template():
    """slv_clip_augment / _color are now the null-table instantiation of the same kernels: a clip that already has T
    frames gives the bits of the identity table, and the oracle's."""
    videos = _videos(seed=9, shapes=[(T, 72, 96), (T, 96, 72)])
    np.random.seed(3)
    params = [VT.sample_spatial_params(72, 96, -1, S, 80, S), VT.sample_spatial_params(96, 72, 4, S, S, S)]
    color = [VT.ColorParams([(VT.SATURATION, 0.7), (VT.CONTRAST, 1.2)], gray=True), VT.ColorParams([(VT.CONTRAST, 0.9)])]
    ident = np.tile(np.arange(T), (2, 1))
    for col in (None, color):
        old = VT.clip_augmentation_batch(videos, params, S, color=col)
        assert torch.equal(old, VT.clip_sample_augmentation_batch(videos, ident, params, S, color=col))
    old = VT.clip_augmentation_batch(videos, params, S).cpu().numpy()
    for b, (v, (nh, nw, yo, xo, fl)) in enumerate(zip(videos, params)):
        assert np.array_equal(old[b], input_ref.clip_augmentation_ref(v.cpu().numpy(), (nh, nw), yo, xo, fl, S)), b


def test_a_bad_table_fails_on_the_host_and_nothing_is_written():
    videos = _videos()
    video_of, fidx, params, color = _case()
    bad = fidx.copy()
    bad[1, 2] = 4                                              # video 1 has frames 0..3
    with pytest.raises(ValueError, match="outside the video"):
        VT.clip_sample_augmentation_batch(videos, bad, params, S, video_of=video_of)
    with pytest.raises(ValueError):
        VT.clip_sample_augmentation_batch(videos, fidx, params, S, video_of=video_of[:-1])
    with pytest.raises(ValueError):
        VT.clip_sample_augmentation_batch((torch.zeros(100, dtype=torch.uint8, device="cuda"), [0], [(2, 8, 8)]),
                                          fidx[:1], params[:1], 8)
    # the C entry points themselves, with real device memory: an error code, and the output keeps its poison
    L = _lib.load()
    v = videos[1]
    desc = torch.tensor([[0, 96, 72, 96, 72, 0, 0, 0]], dtype=torch.int64, device="cuda")
    table = np.array([[0, 1, 2, 3, 4, 0]], dtype=np.int32)     # 4 is outside
    table_d = torch.from_numpy(table).cuda()
    nfr = np.array([4], dtype=np.int64)
    words = VT._color_desc([VT.ColorParams([(VT.CONTRAST, 1.1)])])
    words_d = torch.from_numpy(words).cuda()
    ws = torch.full((1, T), float("nan"), device="cuda")
    out = torch.full((1, 3, T, S, S), float("nan"), device="cuda")
    mean, std = VT._MEAN.ctypes.data, VT._STD.ctypes.data
    rc = L.slv_clip_sample_augment(v.data_ptr(), desc.data_ptr(), table_d.data_ptr(), table.ctypes.data,
                                   nfr.ctypes.data, out.data_ptr(), 1, T, S, mean, std, _lib.stream())
    assert rc != 0 and b"frame index outside the video" in L.slv_last_error()
    rc = L.slv_clip_sample_augment_color(v.data_ptr(), desc.data_ptr(), table_d.data_ptr(), table.ctypes.data,
                                         nfr.ctypes.data, words_d.data_ptr(), words.ctypes.data, ws.data_ptr(),
                                         out.data_ptr(), 1, T, S, mean, std, _lib.stream())
    assert rc != 0 and b"frame index outside the video" in L.slv_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all()


# ---- the batcher against the per-sample composition of the functions that were there before --------------------------------
FPS = [30.0, 29.97, 25.0, 23.976, 30.0]


def _wavs(seed=6):
    g = np.random.RandomState(seed)
    n = [48000 * 3, 48000 * 2 + 17, 48000 * 4, 48000 + 5000, 48000 * 2]          # ragged recordings
    return [torch.from_numpy((g.randn(k) * 3000).astype(np.int16)).cuda() for k in n]


def _per_sample(b, videos, wavs, video_of, st_idx):
    """What the reference's worker does for every sample, with the single-purpose functions: window, host-side gather
    (temporal_sampling), get_spec, ClipAugmenter -- in that order, clip by clip; then its two torch.cat."""
    V, A = [], []
    for s, v in enumerate(video_of):
        t_idx, s_idx, lo, hi, crop = b._sample_setup(None if st_idx is None else st_idx[s])
        aug = VT.ClipAugmenter(s_idx, lo, hi, crop, colorjitter=b.colorjitter, use_grayscale=b.use_grayscale)
        clips, specs = [], []
        for _ in range(b.clips_per_sample):
            size = decoder.clip_size(b.num_frames, b.sample_rate, FPS[v], b.target_fps)
            start, end = decoder.get_start_end_idx(videos[v].shape[0], size, t_idx, b.num_ensemble_views)
            clip = decoder.temporal_sampling(videos[v], start, end, b.num_frames)
            if wavs is not None:
                specs.append(audio_utils.get_spec(wavs[v], start / FPS[v], b.num_sec, b.aud_sample_rate, [],
                                                  b.aud_spec_type, b.use_volume_jittering, b.use_temporal_jittering,
                                                  b.z_normalize))
            clips.append(aug([clip])[0])
        V.append(torch.cat(clips, dim=0))
        if wavs is not None:
            A.append(torch.cat(specs, dim=0))
    return torch.stack(V), (torch.stack(A) if wavs is not None else None)


@pytest.mark.parametrize("dual", [False, True])
def test_batcher_train_mode_equals_the_per_sample_composition(dual):
    videos, wavs = _videos(), _wavs()
    b = DecodedAVBatcher(mode="train", num_frames=T, sample_rate=2, train_crop_size=S, train_jitter_scles=(S, 80),
                         colorjitter=True, use_grayscale=True, dual_data=dual, decode_audio=True,
                         use_volume_jittering=True, z_normalize=True)
    video_of = [0, 1, 2, 3, 4, 2]
    random.seed(11)
    np.random.seed(12)
    frames, audio = b(videos, FPS, wavs, video_of=video_of)
    state = random.getstate(), np.random.get_state()[1].tobytes()
    k = 2 if dual else 1
    assert frames.shape == (6, 3 * k, T, S, S) and audio.shape == (6, k, 40, 99)
    assert b.calls == 1 and b.clips == 6 * k
    random.seed(11)
    np.random.seed(12)
    want_v, want_a = _per_sample(b, videos, wavs, video_of, None)
    assert (random.getstate(), np.random.get_state()[1].tobytes()) == state
    assert torch.equal(frames, want_v)
    assert torch.equal(audio, want_a)
    if dual:                                                   # two different clips of the sample, not one twice
        assert not torch.equal(frames[2, :3], frames[2, 3:]) and not torch.equal(audio[2, 0], audio[2, 1])


def test_batcher_test_mode_equals_the_per_sample_composition_for_every_view():
    videos, wavs = _videos(), _wavs()
    views, crops = 3, 3
    b = DecodedAVBatcher(mode="test", num_frames=T, sample_rate=1, test_crop_size=S, num_spatial_crops=crops,
                         num_ensemble_views=views, colorjitter=False, decode_audio=True, aud_spec_type=1)
    video_of = [0] * 9 + [3] * 9 + [1] * 9                     # every (view, crop) of a landscape, a wide and a short video
    st_idx = list(range(9)) * 3
    random.seed(21)
    np.random.seed(22)
    frames, audio = b(videos, FPS, wavs, spatial_temporal_idx=st_idx, video_of=video_of)
    assert frames.shape == (27, 3, T, S, S) and audio.shape == (27, 1, 40, 99) and b.clips == 27
    random.seed(21)
    np.random.seed(22)
    want_v, want_a = _per_sample(b, videos, wavs, video_of, st_idx)
    for i in range(27):
        assert torch.equal(frames[i], want_v[i]), i
        assert torch.equal(audio[i], want_a[i]), i
    assert not torch.equal(frames[0], frames[1]) and not torch.equal(frames[0], frames[3])    # crops and views differ
    # video only, colour at test time (--test_time_cj), the flat-buffer form
    b2 = DecodedAVBatcher(mode="test", num_frames=T, test_crop_size=S, num_spatial_crops=crops, num_ensemble_views=views,
                          colorjitter=True, decode_audio=False)
    np.random.seed(23)
    f2, a2 = b2(videos, FPS, spatial_temporal_idx=st_idx, video_of=video_of)
    np.random.seed(23)
    w2, _ = _per_sample(b2, videos, None, video_of, st_idx)
    assert a2 is None and torch.equal(f2, w2)


def test_get_spec_batch_rows_share_a_recording_and_respect_true_lengths():
    wavs = _wavs()
    n = [w.numel() for w in wavs]
    wav = torch.zeros((5, max(n)), dtype=torch.int16, device="cuda")
    for i, w in enumerate(wavs):
        wav[i, :n[i]] = w
    rows, starts = [3, 0, 3, 1], [0, 48000, 5000, 17]
    got = audio_utils.get_spec_batch(wav, starts, rows=rows, lengths=n)
    for k, (r, s) in enumerate(zip(rows, starts)):
        assert torch.equal(got[k], audio_utils.get_spec_batch(wavs[r].reshape(1, -1), [s])[0]), k
    with pytest.raises(ValueError, match="outside the recording"):        # inside the padding of row 3, outside its samples
        audio_utils.get_spec_batch(wav, [5001], rows=[3], lengths=n)
    with pytest.raises(ValueError):
        audio_utils.get_spec_batch(wav, [0], rows=[5])
    with pytest.raises(ValueError):
        audio_utils.get_spec_batch(wav, [0] * 5, lengths=n)


def test_finetune_on_whole_videos_takes_the_batcher_path(tmp_path, capsys, monkeypatch):
    from selavi_amd import finetune_video as fv
    made, epochs = [], []
    real_build, real_train, real_aug = fv.build_batchers, fv.train, VT.clip_augmentation_batch

    def build_batchers(args):
        made.append(real_build(args))
        return made[-1]

    def train(*a, **k):
        epochs.append(real_train(*a, **k))
        return epochs[-1]

    def no_clip_path(*a, **k):
        raise AssertionError("a decoded-video run went through clip_augmentation_batch")

    monkeypatch.setattr(fv, "build_batchers", build_batchers)
    monkeypatch.setattr(fv, "train", train)
    monkeypatch.setattr(VT, "clip_augmentation_batch", no_clip_path)
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)
    # the README's fine-tuning example with the new dataset, a small clip and crop, two epochs, a handful of videos
    args = fv.parse_args(["--dataset", "synthetic_video", "--fold", "1", "--epochs", "2", "--clip_len", "4",
                          "--synthetic_crop", "32", "--batch_size", "8", "--train_clips_per_video", "2",
                          "--val_clips_per_video", "2", "--num_spatial_crops", "2", "--use_bn", "True",
                          "--use_l2_norm", "True", "--head_lr", "0.005", "--base_lr", "0.0005",
                          "--use_scheduler", "False", "--synthetic_videos", "16", "--output_dir", str(tmp_path)])
    acc1, acc5, _ = fv.run_folds(args)
    printed = capsys.readouterr().out
    print(printed[-600:])
    assert "Vid Acc@1" in printed and np.isfinite(acc1) and 0.0 <= acc1 <= 100.0
    assert (tmp_path / "checkpoints" / "checkpoint.pth").exists()
    losses = [e[1] for e in epochs]
    print("training loss per epoch:", losses)
    assert len(losses) == 2 and all(np.isfinite(l) for l in losses) and losses[1] < losses[0]
    (train_b, test_b), = made
    # 16 videos x 2 train clips in batches of 8, two epochs; 8 test videos x (2 views x 2 crops), two epochs
    assert train_b.calls == 2 * 4 and train_b.clips == 2 * 32
    assert test_b.calls == 2 * 4 and test_b.clips == 2 * 32
    assert train_b.mode == "train" and test_b.mode == "test" and test_b.num_ensemble_views == 2
