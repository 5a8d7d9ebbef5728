"""Golden vectors for the retrieval evaluation, produced by EXECUTING the reference's src/retrieval_utils.py in the build
container (needs /root/reference and sklearn; never run on the GPU box):

  (a) average_features (norm_feats True and False) on seeded clip features with repeated, shuffled, sparse video ids;
  (b) retrieval on those averages: the printed recall values, every recal_acc and the neighbour lists.  The seed is the
      first one for which no float64 distance gap at a recall cutoff (k-th to (k+1)-th nearest) is below 1e-4 and no gap
      inside the 51 nearest is below 1e-6, so the label sets and the neighbour lists are well defined;
  (c) get_model(args) for pool_op max and avg on a checkpoint written from portable seeds (non-trivial BatchNorm running
      statistics, DataParallel ``module.`` names), applied to a seeded 2-clip, 16-frame 112x112 input.

Only data is stored: no reference source.

    python tests/golden/make_retrieval_golden.py        # writes tests/golden/retrieval.npz
"""
import contextlib
import io
import os
import re
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import install_torchvision_standin  # noqa: E402
from tests import _retrieval_ref as R  # noqa: E402

REF = "/root/reference"


def import_reference():
    install_torchvision_standin()
    ds = types.ModuleType("datasets")
    avd = types.ModuleType("datasets.AVideoDataset")

    class AVideoDataset:                       # decoding is not exercised: only the module's functions are called
        def __init__(self, *a, **k):
            raise RuntimeError("stub")
    avd.AVideoDataset = AVideoDataset
    ds.AVideoDataset = avd
    sys.modules["datasets"], sys.modules["datasets.AVideoDataset"] = ds, avd
    sys.path.insert(0, REF)
    from src import retrieval_utils as ref_ru   # /root/reference/src/retrieval_utils.py
    import model as ref_model                   # /root/reference/model.py
    from sklearn.neighbors import NearestNeighbors
    # the reference passes n_neighbors positionally, which scikit-learn >= 1.0 made keyword-only
    ref_ru.NearestNeighbors = lambda n_neighbors: NearestNeighbors(n_neighbors=n_neighbors)
    return ref_ru, ref_model


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def run_quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **k)
    return out, buf.getvalue()


def main():
    ref_ru, ref_model = import_reference()
    out = {}
    # (a) + (b)
    for seed in range(1, 200):
        tr = R.synth_clips(seed, 80)
        va = R.synth_clips(seed + 1000, 24)
        ok = True
        for norm in (True, False):
            a_tr, _, _ = R.average(*tr, norm)
            a_va, _, _ = R.average(*va, norm)
            ok &= R.min_gap(a_va, a_tr) >= 1e-4 and R.min_gap(a_va, a_tr, range(1, 51)) >= 1e-6
        if ok:
            break
    assert ok, "no seed below 200 separates the cutoffs"
    out["seed"] = np.array([seed])
    for norm in (True, False):
        tag = "norm" if norm else "raw"
        args = Args(norm_feats=norm)
        (f_tr, i_tr, l_tr), _ = run_quiet(ref_ru.average_features, args, *tr)
        (f_va, i_va, l_va), _ = run_quiet(ref_ru.average_features, args, *va)
        out[f"{tag}_train_feats"], out[f"{tag}_train_idx"], out[f"{tag}_train_labels"] = f_tr, np.array(i_tr), l_tr
        out[f"{tag}_val_feats"], out[f"{tag}_val_idx"], out[f"{tag}_val_labels"] = f_va, np.array(i_va), l_va
        assert R.min_gap(f_va, f_tr) >= 1e-4 and R.min_gap(f_va, f_tr, range(1, 51)) >= 1e-6
        rd, txt = run_quiet(ref_ru.retrieval, f_tr, l_tr, i_tr, f_va, l_va, i_va, task='v-v')
        lines = [ln for ln in re.split(r"[\r\n]", txt) if "Recall @" in ln]
        print("\n".join(lines))
        out[f"{tag}_recall"] = np.array([float(ln.split(":")[-1]) for ln in lines])
        out[f"{tag}_recal_acc"] = np.array([[rd[v]['recal_acc'][str(k)] for k in R.RECALL_AT] for v in i_va])
        out[f"{tag}_neighbors"] = np.stack([rd[v]['neighbors']['50'] for v in i_va]).astype(np.int64)
        for v in i_va:                          # the shorter lists are prefixes of the 50-list (well separated)
            for k in R.RECALL_AT:
                assert np.array_equal(rd[v]['neighbors'][str(k)], rd[v]['neighbors']['50'][:k])
    # (c)
    x = R.encoder_input()
    with tempfile.TemporaryDirectory() as d:
        ckpt = os.path.join(d, "ckpt.pth")
        m = ref_model.load_model(vid_base_arch='r2plus1d_18', aud_base_arch='resnet9', pretrained=False, num_classes=309,
                                 norm_feat=False, use_mlp=True, headcount=10)
        R.seeded_checkpoint(m, ckpt)
        for pool in ("max", "avg"):
            args = Args(vid_base_arch='r2plus1d_18', aud_base_arch='resnet9', pretrained=False, num_clusters=309,
                        use_mlp=True, headcount=10, weights_path=ckpt, pool_op=pool)
            enc, _ = run_quiet(ref_ru.get_model, args)
            with torch.no_grad():
                out[f"enc_{pool}"] = enc(x).numpy()
            print(pool, out[f"enc_{pool}"].shape, float(np.abs(out[f"enc_{pool}"]).mean()))
    np.savez_compressed(os.path.join(HERE, "retrieval.npz"), **out)
    print("seed", seed, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
