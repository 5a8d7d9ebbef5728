"""Temporal sampling on the host: selavi_amd.datasets.decoder against what the executed reference produced
(tests/golden/make_decoder_golden.py), the order and count of DecodedAVBatcher's draws against a straight-line
restatement built from the package's single-purpose functions, and the C ABI of the two new entry points."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from selavi_amd import _lib
from selavi_amd.datasets import audio_utils, decoder
from selavi_amd.datasets import video_transforms as VT
from selavi_amd.datasets.av_batcher import DecodedAVBatcher

GOLD = os.path.join(os.path.dirname(__file__), "golden", "decoder_sampling.npz")


def golden_cases():
    d = np.load(GOLD)
    for i, row in enumerate(d["cases"]):
        seed, n, T, sr, fps, tfps, cidx, nclips = row
        yield i, d, int(seed), int(n), int(T), int(sr), float(fps), int(tfps), int(cidx), int(nclips)


def test_window_and_frame_indices_equal_the_executed_reference():
    kinds = set()
    for i, d, seed, n, T, sr, fps, tfps, cidx, nclips in golden_cases():
        random.seed(seed)
        size = decoder.clip_size(T, sr, fps, tfps)
        start, end = decoder.get_start_end_idx(n, size, cidx, nclips)
        idx = decoder.frame_indices(n, start, end, T)
        assert np.float64(size) == d["clip_size"][i], i
        assert np.float64(start) == d["start"][i] and np.float64(end) == d["end"][i], (i, start, end)
        assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), d[f"idx_{i}"]), i
        frames = torch.arange(n).reshape(n, 1)
        assert torch.equal(decoder.temporal_sampling(frames, start, end, T).reshape(-1), idx), i
        if cidx == -1:
            assert isinstance(start, float)
            random.seed(seed)                                             # exactly one draw, and only in the random case
            random.uniform(0, 1)
            after = random.getstate()
            random.seed(seed)
            decoder.get_start_end_idx(n, size, cidx, nclips)
            assert random.getstate() == after, i
        else:
            assert isinstance(start, int)
        kinds.add(("train" if cidx == -1 else f"of{nclips}", n < size, fps not in (30.0,)))
    # the issue's cases are all there: train draws, 1 / 10 / 1000 test clips, short videos, fractional rates
    assert {k[0] for k in kinds} == {"train", "of1", "of10", "of1000"}
    assert any(k[1] for k in kinds) and any(k[2] for k in kinds)


def _state():
    return random.getstate(), np.random.get_state()[1].tobytes(), np.random.get_state()[2]


SHAPES = [(57, 72, 96), (20, 96, 72), (140, 80, 80), (9, 72, 120)]
FPS = [30.0, 29.97, 25.0, 23.976]
NAUD = [48000 * 3, 48000 * 2 + 17, 48000 * 6, 48000 + 5000]
# for the jittered audio: audio_utils.window rejects a window that starts before the recording, which a clip at the very
# start of a video gets with a negative temporal jitter -- videos long enough that the seeded draws stay clear of it
LONG = [(257, 72, 96), (220, 96, 72), (340, 80, 80), (209, 72, 120)]
NAUD_LONG = [48000 * 10, 48000 * 9 + 17, 48000 * 15, 48000 * 10]


@pytest.mark.parametrize("audio", [None, "plain", "jitter"])
@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("mode", ["train", "train_dual", "train_center", "train_nojitter", "test"])
def test_batcher_draws_in_the_reference_order(mode, color, audio):
    T, crop = 8, 64
    jit = audio == "jitter"
    SHAPES, NAUD = (LONG, NAUD_LONG) if jit else (globals()["SHAPES"], globals()["NAUD"])
    kw = dict(num_frames=T, sample_rate=2, train_crop_size=crop, test_crop_size=crop, train_jitter_scles=(64, 80),
              num_spatial_crops=3, num_ensemble_views=4, colorjitter=color, use_grayscale=color, use_gaussian=True,
              decode_audio=bool(audio), use_volume_jittering=jit, use_temporal_jittering=jit, target_fps=30)
    b = DecodedAVBatcher(mode="test" if mode == "test" else "train", dual_data=mode == "train_dual",
                         center_crop=mode == "train_center", temp_jitter=mode != "train_nojitter", **kw)
    video_of = [0, 1, 2, 3, 0, 0] if mode == "test" else [0, 1, 2, 3]
    st_idx = [9, 5, 11, 7, 3, 4] if mode == "test" else None
    random.seed(3)
    np.random.seed(4)
    plan = b.plan(SHAPES, FPS, NAUD if audio else None, st_idx, video_of)
    after = _state()

    # the restatement: per sample, per clip, the package's single-purpose functions in the reference worker's order
    random.seed(3)
    np.random.seed(4)
    want = dict(video_of=[], start=[], fidx=[], params=[], color=[], audio_start=[], volume=[])
    for s, v in enumerate(video_of):
        N, H, W = SHAPES[v]
        if mode == "test":
            t_idx, s_idx, lo, hi = st_idx[s] // 3, st_idx[s] % 3, crop, crop
        elif mode == "train_center":
            t_idx, s_idx, lo, hi = -1, 1, crop, crop
        else:
            t_idx, s_idx, lo, hi = -1, -1, 64, 80
        for _ in range(2 if mode == "train_dual" else 1):
            size = T * 2 * FPS[v] / 30
            if mode == "train_nojitter":
                start, end = decoder.get_start_end_idx(N, size, 500, 1000)
            else:
                start, end = decoder.get_start_end_idx(N, size, t_idx, 4)
            if audio:
                want["audio_start"].append(audio_utils.window(NAUD[v], start / FPS[v], 1, 48000, jit))
                if jit:
                    want["volume"].append(np.random.uniform(0.9, 1.1))
            want["params"].append(VT.sample_spatial_params(H, W, s_idx, lo, hi, crop))
            if color:
                want["color"].append(VT.sample_color_params(True, True))
            want["video_of"].append(v)
            want["start"].append(start)
            want["fidx"].append(decoder.frame_indices(N, start, end, T).numpy())
    assert _state() == after                                   # the same number of draws from both generators
    assert plan.video_of == want["video_of"] and plan.start_idx == want["start"]
    assert plan.fidx.dtype == np.int32 and np.array_equal(plan.fidx, np.stack(want["fidx"]))
    assert plan.params == want["params"]
    assert plan.color == (want["color"] if color else None)
    assert plan.audio_start == (want["audio_start"] if audio else None)
    assert plan.volume == (want["volume"] if jit else None)
    assert plan.crop_size == crop and b.calls == 0 and b.clips == 0        # plan() launches and counts nothing
    for row, v in zip(plan.fidx, plan.video_of):
        assert row.min() >= 0 and row.max() < SHAPES[v][0]
    if mode == "train_dual":                                               # the two clips of sample 2: a window draw each
        assert plan.video_of[4:6] == [2, 2] and plan.start_idx[4] != plan.start_idx[5]
    if mode == "train_nojitter":                                           # 500 of 1000: the middle, no draw
        assert plan.start_idx == [int(max(SHAPES[v][0] - T * 2 * FPS[v] / 30, 0) * 500 / 1000) for v in video_of]
    if mode == "test":                                                     # views 3 and 4 of video 0: one window, two crops
        assert plan.start_idx[4] == plan.start_idx[5] and np.array_equal(plan.fidx[4], plan.fidx[5])
        assert plan.params[4] != plan.params[5]


def test_batcher_flags_off_draw_only_the_window_and_the_spatial_parameters():
    b = DecodedAVBatcher(mode="train", num_frames=4, train_crop_size=64, train_jitter_scles=(64, 80), decode_audio=True)
    random.seed(1)
    np.random.seed(2)
    plan = b.plan(SHAPES[:1], FPS[:1], NAUD[:1])
    after = _state()
    random.seed(1)
    np.random.seed(2)
    start, _ = decoder.get_start_end_idx(57, 4.0, -1, 10)
    prm = VT.sample_spatial_params(72, 96, -1, 64, 80, 64)
    assert _state() == after and plan.params == [prm] and plan.color is None and plan.volume is None
    assert plan.audio_start == [audio_utils.window(NAUD[0], start / 30.0)]
    with pytest.raises(ValueError):
        DecodedAVBatcher(mode="test", decode_audio=False).plan(SHAPES[:1], FPS[:1])         # no view index
    with pytest.raises(ValueError):
        DecodedAVBatcher(mode="test", decode_audio=False).plan(SHAPES[:1], FPS[:1], None, [30])
    with pytest.raises(ValueError):
        b.plan(SHAPES[:1], FPS[:1])                                                           # audio without recordings


# ---- the C ABI -------------------------------------------------------------------------------------------------------
NEW = {"slv_clip_sample_augment": ["frames_u8", "desc", "fidx", "fidx_host", "n_frames_host", "out", "B", "T", "S",
                                   "mean3", "std3", "stream"],
       "slv_clip_sample_augment_color": ["frames_u8", "desc", "fidx", "fidx_host", "n_frames_host", "color",
                                         "color_host", "frame_mean_ws", "out", "B", "T", "S", "mean3", "std3",
                                         "stream"]}
OLD = {"slv_clip_augment": ["frames_u8", "desc", "out", "B", "T", "S", "mean3", "std3", "stream"],
       "slv_clip_augment_color": ["frames_u8", "desc", "color", "color_host", "frame_mean_ws", "out", "B", "T", "S",
                                  "mean3", "std3", "stream"]}


def test_symbols_declared_and_exported():
    from selavi_amd import build
    build.build(verbose=False)
    decl = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIBPATH)
    for name, args in {**NEW, **OLD}.items():                  # the old pair keeps its signature
        ret, got = decl[name]
        assert ret == "int" and [a[1] for a in got] == args, name
        assert hasattr(lib, name), name


def test_entry_points_reject_a_bad_frame_table_on_the_host():
    """Nothing is launched: the pointers that would be device memory are never dereferenced on these paths (host
    buffers stand in for them), the stream is null, and the call returns before any launch."""
    from selavi_amd import build
    build.build(verbose=False)
    L = _lib.load()
    B, T, S = 2, 4, 8
    dummy = np.zeros(4096, dtype=np.uint8)                                 # stands in for every device pointer
    words = VT._color_desc([VT.ColorParams([(VT.CONTRAST, 1.1)]), None])
    n_frames = np.array([10, 3], dtype=np.int64)
    mean, std = VT._MEAN.ctypes.data, VT._STD.ctypes.data
    dp = dummy.ctypes.data

    def plain(fidx, nf=n_frames, B=B):
        return L.slv_clip_sample_augment(dp, dp, dp, fidx.ctypes.data if fidx is not None else None, nf.ctypes.data,
                                         dp, B, T, S, mean, std, None)

    def colour(fidx, nf=n_frames, w=words):
        return L.slv_clip_sample_augment_color(dp, dp, dp, fidx.ctypes.data, nf.ctypes.data, dp, w.ctypes.data, dp, dp,
                                               B, T, S, mean, std, None)

    good = np.array([[0, 3, 9, 9], [2, 2, 0, 1]], dtype=np.int32)
    for bad_at, val in (((0, 2), 10), ((1, 0), 3), ((1, 3), -1), ((0, 0), 2 ** 31 - 1)):
        fidx = good.copy()
        fidx[bad_at] = val
        for call in (plain, colour):
            rc = call(fidx)
            assert rc != 0 and b"frame index outside the video" in L.slv_last_error(), (bad_at, val)
    assert plain(good, np.array([10, 0], dtype=np.int64)) != 0 and b"without frames" in L.slv_last_error()
    assert plain(None) != 0 and b"null pointer" in L.slv_last_error()
    assert plain(good, B=0) != 0 and b"bad sizes" in L.slv_last_error()
    # the colour checks of slv_clip_augment_color hold for the table variant too (a good table, bad colour words)
    bad_words = words.copy()
    bad_words[0, 0] = 7
    assert colour(good, w=bad_words) != 0 and b"unknown stage code" in L.slv_last_error()
    rc = L.slv_clip_sample_augment_color(dp, dp, dp, good.ctypes.data, n_frames.ctypes.data, dp, words.ctypes.data, None,
                                         dp, B, T, S, mean, std, None)
    assert rc != 0 and b"workspace" in L.slv_last_error()
    assert b"slv_clip_sample_augment_color" in L.slv_last_error()          # the message names the entry point

