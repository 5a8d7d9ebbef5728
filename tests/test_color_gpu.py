"""Colour jitter / grayscale in the device clip augmentation (csrc/input.hip: slv_clip_augment_color,
video_transforms.ClipAugmenter, finetune_video on uint8 frames) against the restatement (tests/_color_ref.py) and the
outputs of the executed reference (tests/golden/clip_color.npz)."""
import numpy as np
import pytest
import torch

from selavi_amd import _lib
from selavi_amd.datasets import video_transforms as VT
from tests import _color_ref as CR
from tests.test_color_cpu import cases, compare_with_golden

pytestmark = pytest.mark.gpu


def _run(frames, spatial, crop, color):
    clips = [torch.from_numpy(f).cuda() for f in frames]
    return VT.clip_augmentation_batch(clips, spatial, crop, color=color).cpu().numpy()


def test_kernel_against_restatement_and_reference_outputs():
    """Bit-equal to the restatement where no contrast stage is present.  With one, the restatement is evaluated with
    the same float64 frame mean and must match to the last bit as well: the kernel's float64 sum (1024 strided partial
    sums and a tree) and the restatement's exactly rounded sum differ by a few float64 ulp, which survives the one
    rounding to float32 only if the mean lies within ~1e-13 relative of a float32 rounding boundary (odds about 1e-6
    per frame) -- not the case for any frame of this set, so no ulp allowance is made."""
    for k, d, frames, p in cases():
        y = _run([frames], [p["spatial"]], p["crop"], [VT.ColorParams(p["stages"], p["gray"])])[0]
        ref = CR.clip_color_ref(frames, p["spatial"], p["crop"], p["stages"], p["gray"], mean="f64")
        print(f"{k}: kernel vs restatement max abs diff {np.abs(y.astype(np.float64) - ref).max():.3g}")
        assert np.array_equal(y, ref), (k, np.abs(y - ref).max())
        compare_with_golden(y, d, k, p)


def _ragged():
    g = np.random.RandomState(8)
    shapes = ((72, 96), (96, 72), (80, 80), (72, 120), (72, 96), (90, 70), (72, 96))
    frames = [g.randint(0, 256, size=(3, h, w, 3)).astype(np.uint8) for h, w in shapes]
    np.random.seed(21)
    spatial = [VT.sample_spatial_params(h, w, -1, 64, 80, 64) for h, w in shapes]
    color = [None,                                                                         # no colour
             VT.ColorParams(),                                                             # the gate said no
             VT.ColorParams([(CR.CONTRAST, 1.31), (CR.SATURATION, 0.72), (CR.BRIGHTNESS, 0.9)]),
             VT.ColorParams([(CR.SATURATION, 0.61), (CR.BRIGHTNESS, 1.39), (CR.CONTRAST, 0.8)], gray=True),
             VT.ColorParams([(CR.BRIGHTNESS, 1.2), (CR.CONTRAST, 0.65), (CR.SATURATION, 1.1)]),
             VT.ColorParams(gray=True),                                                    # grayscale alone
             VT.ColorParams([(CR.SATURATION, 1.25)])]                                      # a single stage, no pass 1 of its own
    return frames, spatial, color


def test_ragged_batch_equals_the_one_clip_calls():
    frames, spatial, color = _ragged()
    y = _run(frames, spatial, 64, color)
    assert y.shape == (7, 3, 3, 64, 64)
    plain = _run(frames, spatial, 64, None)
    for b, (f, sp, cp) in enumerate(zip(frames, spatial, color)):
        one = _run([f], [sp], 64, [cp])[0]
        assert np.array_equal(y[b], one), b
        cp = cp or VT.ColorParams()
        assert np.array_equal(y[b], CR.clip_color_ref(f, sp, 64, cp.stages, cp.gray)), b
    for b in (0, 1):                                                                       # no colour work: today's kernel's bits
        assert np.array_equal(y[b], plain[b]), b
    for b in range(2, 7):
        assert not np.array_equal(y[b], plain[b]), b
    # a batch without any contrast stage takes pass 2 alone (no workspace is allocated or read)
    sub = [0, 1, 5, 6]
    z = _run([frames[b] for b in sub], [spatial[b] for b in sub], 64, [color[b] for b in sub])
    assert np.array_equal(z, y[sub])


def test_two_launches_are_bit_identical():
    frames, spatial, color = _ragged()
    clips = [torch.from_numpy(f).cuda() for f in frames]
    a = VT.clip_augmentation_batch(clips, spatial, 64, color=color)
    b = VT.clip_augmentation_batch(clips, spatial, 64, out=torch.full_like(a, float("nan")), color=color)
    assert torch.equal(a, b)


def test_clip_augmenter_reproduces_the_reference_under_the_same_seed():
    for k, d, frames, p in cases():
        aug = VT.ClipAugmenter(spatial_idx=p["sidx"], min_scale=p["lo"], max_scale=p["hi"], crop_size=p["crop"],
                               colorjitter=p["cj"], use_grayscale=p["gs"], use_gaussian=True)
        np.random.seed(p["seed"])
        y = aug([torch.from_numpy(frames).cuda()])
        assert y.shape == (1, 3, frames.shape[0], p["crop"], p["crop"]) and y.dtype == torch.float32
        compare_with_golden(y[0].cpu().numpy(), d, k, p)
    # a B x T x H x W x 3 tensor with per-clip test-time views
    g = np.random.RandomState(3)
    clips = g.randint(0, 256, size=(3, 2, 72, 96, 3)).astype(np.uint8)
    aug = VT.ClipAugmenter(1, 64, 64, 64, colorjitter=True)
    np.random.seed(4)
    y = aug(torch.from_numpy(clips).cuda(), spatial_idx=[0, 4, 2]).cpu().numpy()
    np.random.seed(4)
    for b, si in enumerate((0, 4, 2)):
        sp = VT.sample_spatial_params(72, 96, si, 64, 64, 64)
        cp = VT.sample_color_params(True, False)
        assert np.array_equal(y[b], CR.clip_color_ref(clips[b], sp, 64, cp.stages, cp.gray)), b


def test_bad_arguments_are_reported_not_crashed():
    frames, spatial, color = _ragged()
    clips = [torch.from_numpy(frames[2]).cuda()]
    with pytest.raises(_lib.SelaviHipError, match="unknown stage code"):
        VT.clip_augmentation_batch(clips, spatial[2:3], 64, color=[VT.ColorParams([(7, 1.1)])])
    with pytest.raises(_lib.SelaviHipError, match="more than one contrast"):
        VT.clip_augmentation_batch(clips, spatial[2:3], 64, color=[VT.ColorParams([(2, 1.1), (2, 0.9)])])
    with pytest.raises(ValueError):
        VT.clip_augmentation_batch(clips, spatial[2:3], 64, color=[None, None])
    # the C entry point itself: a contrast stage without the workspace, null pointers, sizes
    L = _lib.load()
    words = VT._color_desc([color[2]])
    words_d = torch.from_numpy(words).cuda()
    buf = clips[0].reshape(-1)
    desc = torch.zeros(8, dtype=torch.int64, device="cuda")
    out = torch.empty(1, 3, 3, 64, 64, device="cuda")
    mean, std = VT._MEAN.ctypes.data, VT._STD.ctypes.data
    rc = L.slv_clip_augment_color(buf.data_ptr(), desc.data_ptr(), words_d.data_ptr(), words.ctypes.data, None,
                                  out.data_ptr(), 1, 3, 64, mean, std, None)
    assert rc != 0 and b"workspace" in L.slv_last_error()
    rc = L.slv_clip_augment_color(buf.data_ptr(), desc.data_ptr(), words_d.data_ptr(), None, None, out.data_ptr(), 1, 3,
                                  64, mean, std, None)
    assert rc != 0 and b"null pointer" in L.slv_last_error()
    rc = L.slv_clip_augment_color(buf.data_ptr(), desc.data_ptr(), words_d.data_ptr(), words.ctypes.data, None,
                                  out.data_ptr(), 0, 3, 64, mean, std, None)
    assert rc != 0 and b"bad sizes" in L.slv_last_error()
    torch.cuda.synchronize()


def test_finetune_end_to_end_on_uint8_frames(tmp_path, capsys, monkeypatch):
    from selavi_amd import finetune_video as fv
    calls, logits = [], []
    real_clips, real_acc = fv.device_clips, fv.video_accuracy

    def device_clips(video, augment, spatial_idx=None):
        state = np.random.get_state()
        out = real_clips(video, augment, spatial_idx)
        calls.append((video.clone(), spatial_idx, state, out.clone()))
        return out

    def video_accuracy(outs, *a, **k):
        logits.append(outs.clone())
        return real_acc(outs, *a, **k)

    monkeypatch.setattr(fv, "device_clips", device_clips)
    monkeypatch.setattr(fv, "video_accuracy", video_accuracy)
    base = ["--dataset", "synthetic_uint8", "--synthetic_crop", "32", "--fold", "1",
            "--epochs", "1", "--clip_len", "4", "--batch_size", "8", "--synthetic_videos", "8",
            "--train_clips_per_video", "2", "--val_clips_per_video", "1", "--num_spatial_crops", "3",
            "--use_scheduler", "False", "--test_time_cj", "False"]
    first = {}
    for cj in ("True", "False"):
        torch.manual_seed(0)
        np.random.seed(0)
        calls.clear()
        acc1, _, _ = fv.run_folds(fv.parse_args(base + ["--colorjitter", cj, "--output_dir", str(tmp_path / cj)]))
        assert np.isfinite(acc1) and (tmp_path / cj / "checkpoints" / "checkpoint.pth").exists()
        assert len(calls) == 2 + 2                                   # 16 training clips, 12 test clips, batches of 8
        assert [c[1] for c in calls[:2]] == [None, None] and calls[2][1] == [0, 1, 2, 0, 1, 2, 0, 1]
        assert all(c[3].shape[1:] == (3, 4, 32, 32) and c[3].dtype == torch.float32 for c in calls)
        first[cj] = calls[0]
    frames, _, state, clip_off = first["False"]
    assert frames.dtype == torch.uint8 and frames.shape == (8, 4, 40, 48, 3) and torch.equal(frames, first["True"][0])
    assert not torch.equal(first["True"][3], clip_off)               # the jitter reached the trunk's input
    np.random.set_state(state)                                       # --colorjitter False: the plain spatial path
    prms = [VT.sample_spatial_params(40, 48, -1, 32, 40, 32) for _ in range(8)]
    assert torch.equal(VT.clip_augmentation_batch(frames.cuda(), prms, 32), clip_off)
    # evaluation does not depend on --colorjitter: either run's checkpoint gives the same bits under both settings
    for ck in ("True", "False"):
        got = {}
        for cj in ("True", "False"):
            calls.clear()
            logits.clear()
            a = fv.parse_args(base + ["--colorjitter", cj, "--output_dir", str(tmp_path / ck), "--resume", "1",
                                      "--test_only", "True"])
            acc1, acc5, _ = fv.main(a)
            got[cj] = (acc1, acc5, [c[3] for c in calls], logits[0])
        assert got["True"][:2] == got["False"][:2]
        assert all(torch.equal(x, y) for x, y in zip(got["True"][2], got["False"][2])) and len(got["True"][2]) == 2
        assert torch.equal(got["True"][3], got["False"][3])
    # a float dataset: the flag is not dropped in silence
    capsys.readouterr()
    fv._noted.clear()
    fv.run_folds(fv.parse_args([
        "--dataset", "synthetic", "--synthetic_crop", "32", "--fold", "1", "--epochs", "1", "--clip_len", "4",
        "--batch_size", "8", "--synthetic_videos", "8", "--train_clips_per_video", "1", "--val_clips_per_video", "1",
        "--num_spatial_crops", "1", "--use_scheduler", "False", "--colorjitter", "True", "--output_dir", ""]))
    assert "--colorjitter True has no effect" in capsys.readouterr().out
