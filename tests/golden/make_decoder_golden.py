"""Golden vectors for the temporal sampling (selavi_amd/datasets/decoder.py), produced by EXECUTING the reference's
datasets/decoder.py: get_start_end_idx and temporal_sampling.

    python tests/golden/make_decoder_golden.py      # needs /root/reference; writes tests/golden/decoder_sampling.npz

The reference module imports torchvision.io and its audio_utils at the top and uses neither in the two functions;
where they do not import, empty stand-ins are put into sys.modules for the load.  ``random`` is seeded per case.
temporal_sampling is run on frames whose value is their own index, so its output IS the index row.

The file holds ``cases`` (float64, one row per case: seed, video_size, num_frames, sampling_rate, fps, target_fps,
clip_idx, num_clips), ``clip_size`` (float64, computed HERE with the expression of decoder.py:392 and handed to the
reference's get_start_end_idx), ``start`` / ``end`` (float64, as the reference returned them) and ``idx_<i>`` (int64, the
frames of case i, as the reference's temporal_sampling picked them).
"""
import importlib
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/datasets/decoder.py"

for name in ("torchvision", "torchvision.io", "audio_utils"):
    try:
        importlib.import_module(name)
    except Exception:
        stub = types.ModuleType(name)
        if name == "audio_utils":
            stub.load_audio = None
        sys.modules[name] = stub
        if name == "torchvision.io":
            sys.modules["torchvision"].io = stub
spec = importlib.util.spec_from_file_location("ref_decoder", REF)
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

CASES = []        # (seed, video_size, num_frames, sampling_rate, fps, target_fps, clip_idx, num_clips)
for seed, (n, T, sr, fps) in enumerate([(300, 30, 1, 30.0), (157, 32, 1, 30.0), (91, 8, 2, 30.0), (64, 16, 1, 30.0),
                                        (250, 32, 2, 30.0), (33, 32, 1, 30.0)]):
    CASES.append((seed + 1, n, T, sr, fps, 30, -1, 10))                          # train draws
for n, T in ((300, 30), (97, 8)):                                                # test views
    CASES += [(0, n, T, 1, 30.0, 30, 0, 1)]
    CASES += [(0, n, T, 1, 30.0, 30, k, 10) for k in range(10)]
    CASES += [(0, n, T, 1, 30.0, 30, k, 1000) for k in (0, 1, 499, 500, 999)]    # 500 of 1000: temp_jitter off
for seed, (n, T, sr) in enumerate([(20, 32, 1), (7, 8, 1), (15, 8, 2), (1, 4, 1), (30, 30, 1)]):
    CASES.append((seed + 11, n, T, sr, 30.0, 30, -1, 10))                        # shorter than (or as long as) the clip
    CASES.append((0, n, T, sr, 30.0, 30, 3, 10))
for seed, fps in enumerate((29.97, 23.976, 25.0, 59.94, 12.5, 30000 / 1001)):    # fractional fps / target_fps
    CASES.append((seed + 21, 211, 16, 2, fps, 30, -1, 10))
    CASES.append((0, 211, 16, 2, fps, 30, 7, 10))
    CASES.append((seed + 31, 40, 32, 1, fps, 30, -1, 10))

out = {"cases": np.array(CASES, dtype=np.float64)}
size, start, end = [], [], []
for i, (seed, n, T, sr, fps, tfps, cidx, nclips) in enumerate(CASES):
    random.seed(seed)
    cs = T * sr * fps / tfps                                                     # the expression of decoder.py:392
    s, e = ref.get_start_end_idx(n, cs, cidx, nclips)
    frames = torch.arange(n).reshape(n, 1)
    idx = ref.temporal_sampling(frames, s, e, T).reshape(-1).numpy().astype(np.int64)
    assert idx.shape == (T,) and idx.min() >= 0 and idx.max() < n
    size.append(cs), start.append(float(s)), end.append(float(e))
    out[f"idx_{i}"] = idx
    print(i, CASES[i], "clip_size", cs, "start", s, "end", e, idx.tolist())
out["clip_size"], out["start"], out["end"] = (np.array(a, dtype=np.float64) for a in (size, start, end))
path = os.path.join(HERE, "decoder_sampling.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
