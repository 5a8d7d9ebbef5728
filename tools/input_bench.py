"""Throughput of the device input pipeline (slv_clip_augment, slv_clip_augment_color, slv_logfbank) at the cfg2 batch
shape.

    python tools/input_bench.py            # on the GPU box
    python tools/input_bench.py --sample [--out profiles/input_bench_sample.txt]
                                           # clips cut from whole videos: the fused path (slv_clip_sample_augment)
                                           # against index_select per clip + clip_augmentation_batch, in one process
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from selavi_amd.datasets import audio_utils, decoder, video_transforms  # noqa: E402
from selavi_amd.datasets.av_batcher import DecodedAVBatcher  # noqa: E402


def timeit(fn, reps=50):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    B, T, H, W, S = 16, 16, 128, 171, 112
    g = torch.Generator(device="cuda").manual_seed(0)
    clips = torch.randint(0, 256, (B, T, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    np.random.seed(0)
    prms = [video_transforms.sample_spatial_params(H, W, -1, 128, 160, S) for _ in range(B)]
    out = torch.empty((B, 3, T, S, S), device="cuda")
    ms = timeit(lambda: video_transforms.clip_augmentation_batch(clips, prms, S, out=out))
    src_bytes = sum(T * 3 * (S * H / nh) * (S * W / nw) for nh, nw, *_ in prms)      # source pixels under the crop
    byt = src_bytes + out.numel() * 4
    print(f"clip_augment  B={B} T={T} {H}x{W}->{S}: {ms * 1e3:8.1f} us  {B / ms * 1e3:10.0f} clips/s  "
          f"{byt / ms / 1e6:7.1f} GB/s (algorithmic: crop footprint read + clip written)")
    # the colour path: every clip jittered with contrast last (the longest pass 1: two stages in front of the frame mean),
    # and grayscale only (pass 2 alone)
    VT = video_transforms
    jit = [VT.ColorParams([(VT.SATURATION, 0.8 + 0.02 * b), (VT.BRIGHTNESS, 1.3 - 0.02 * b), (VT.CONTRAST, 0.7 + 0.03 * b)])
           for b in range(B)]
    for name, color, reads, what in (("contrast last", jit, 2, "crop footprint read twice + clip written"),
                                     ("grayscale only", [VT.ColorParams(gray=True)] * B, 1,
                                      "crop footprint read + clip written")):
        ms = timeit(lambda: VT.clip_augmentation_batch(clips, prms, S, out=out, color=color))
        byt = reads * src_bytes + out.numel() * 4
        print(f"clip_augment_color {name:14s} B={B} T={T} {H}x{W}->{S}: {ms * 1e3:8.1f} us  {B / ms * 1e3:10.0f} clips/s  "
              f"{byt / ms / 1e6:7.1f} GB/s (algorithmic: {what})")
    wav = (torch.randn(B, 48000 * 2, device="cuda", generator=g) * 3000).to(torch.int16)
    for t in (1, 2):
        ms = timeit(lambda: audio_utils.get_spec_batch(wav, [100] * B, aud_spec_type=t))
        flop = B * 99 * 513 * 960 * 4
        print(f"logfbank type {t} B={B}: {ms * 1e3:8.1f} us  {B / ms * 1e3:10.0f} clips/s  {flop / ms / 1e9:6.2f} TFLOP/s fp64 (direct DFT)")


def sample_leg(out_path, rounds=5, reps=20):
    """Whole videos -> clips at the cfg2 batch (16 clips x 16 frames, 128 x 171 -> 112), training and test time.  The two
    paths are timed alternately, ``rounds`` times ``reps`` calls each; the figure is the median round.  Each timed call
    includes its host work (descriptors, the one upload), as a training loop would pay it.  At 16 clips a round of 20
    calls is only 1-5 ms of work: read those legs by the spread of the rounds printed next to them."""
    VT = video_transforms
    B, T, H, W, S = 16, 16, 128, 171, 112
    g = torch.Generator(device="cuda").manual_seed(0)
    lengths = [150 + 10 * i for i in range(B)]                           # 5 - 10 s at 30 fps
    videos = [torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g) for n in lengths]
    fps = [30.0] * B
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def run(name, batcher, video_of, st_idx):
        import random
        random.seed(0)
        np.random.seed(0)
        plan = batcher.plan([(n, H, W) for n in lengths], fps, None, st_idx, video_of)
        n = len(plan.video_of)
        out_f = torch.empty((n, 3, T, S, S), device="cuda")
        out_g = torch.empty((n, 3, T, S, S), device="cuda")
        rows = [torch.from_numpy(r.astype(np.int64)).cuda() for r in plan.fidx]

        def fused():
            VT.clip_sample_augmentation_batch(videos, plan.fidx, plan.params, S, out=out_f, color=plan.color,
                                              video_of=plan.video_of)

        def gathered():
            clips = [torch.index_select(videos[v], 0, r) for v, r in zip(plan.video_of, rows)]
            VT.clip_augmentation_batch(clips, plan.params, S, out=out_g, color=plan.color)

        fused(), gathered()
        torch.cuda.synchronize()
        assert torch.equal(out_f, out_g), name                          # faster and different is not faster
        tf, tg = [], []
        for _ in range(rounds):
            tf.append(timeit(fused, reps))
            tg.append(timeit(gathered, reps))
        f, gth = float(np.median(tf)), float(np.median(tg))
        gather_bytes = n * T * H * W * 3
        say(f"{name}: {n} clips of {len(set(plan.video_of))} videos, T={T} {H}x{W}->{S}")
        say(f"  fused  (slv_clip_sample_augment)              {f * 1e3:9.1f} us   rounds {[round(x * 1e3, 1) for x in tf]}")
        say(f"  gather (index_select x {n} + cat + clip_augment) {gth * 1e3:9.1f} us   rounds {[round(x * 1e3, 1) for x in tg]}")
        say(f"  fused / gather = {f / gth:.3f}   ({gth / f:.2f}x)   gathered copy: {gather_bytes / 1e6:.1f} MB written by "
            f"index_select, read and written again by cat, read by the kernel; output {out_f.numel() * 4 / 1e6:.1f} MB; "
            f"outputs bit-equal")

    kw = dict(num_frames=T, sample_rate=1, train_crop_size=S, test_crop_size=S, decode_audio=False)
    say(f"# tools/input_bench.py --sample on {torch.cuda.get_device_name(0)}: median of {rounds} alternating rounds of "
        f"{reps} calls, device events, host work of each call included")
    run("train", DecodedAVBatcher(mode="train", **kw), None, None)
    run("train, colour jitter + grayscale", DecodedAVBatcher(mode="train", colorjitter=True, use_grayscale=True, **kw),
        None, None)
    run("train, dual_data", DecodedAVBatcher(mode="train", dual_data=True, **kw), None, None)
    views, crops = 10, 3
    run("test, 10 views x 3 crops of each video",
        DecodedAVBatcher(mode="test", num_ensemble_views=views, num_spatial_crops=crops, **kw),
        [v for v in range(B) for _ in range(views * crops)], list(range(views * crops)) * B)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", action="store_true", help="time clips cut from whole videos, fused against gathered")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "input_bench_sample.txt"))
    a = ap.parse_args()
    if a.sample:
        sample_leg(a.out)
    else:
        main()
