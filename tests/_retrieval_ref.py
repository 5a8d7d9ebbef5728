"""Numpy float64 restatement of the reference's retrieval evaluation (src/retrieval_utils.py: average_features, brute-force
NearestNeighbors, the recall bookkeeping of retrieval) and the seeded inputs of tests/golden/retrieval.npz.

tests/test_retrieval_cpu.py pins the restatement to the numbers the executed reference produced; the GPU tests then
judge the package against it."""
import zlib

import numpy as np
import torch

RECALL_AT = (1, 5, 10, 20, 50)


# ------------------------------------------------------------------ seeded inputs (shared with make_retrieval_golden.py)
def synth_clips(seed, n_videos, D=96, n_classes=12, max_clips=5, proto_seed=7):
    """Clip features of n_videos videos (1..max_clips clips each, rows shuffled), sparse video ids and labels.
    Train and val sets built with the same proto_seed share the class prototypes."""
    proto = np.random.RandomState(proto_seed).randn(n_classes, D)
    g = np.random.RandomState(seed)
    cls = g.randint(0, n_classes, size=n_videos)
    vpat = g.randn(n_videos, D)
    counts = g.randint(1, max_clips + 1, size=n_videos)
    vid = np.repeat(np.arange(n_videos), counts)
    g.shuffle(vid)
    scale = g.uniform(0.5, 2.0, size=(len(vid), 1))            # per-clip scale: normalisation matters
    feats = ((0.3 * proto[cls[vid]] + 0.8 * vpat[vid] + 0.4 * g.randn(len(vid), D)) * scale).astype(np.float32)
    return feats, (vid * 7 + 100 + seed).astype(np.int32), (cls[vid] * 3 + 1).astype(np.int32)


def fill_bn_stats_(model, seed=5):
    """Non-trivial BatchNorm running statistics, drawn per buffer name (portable across hosts)."""
    from oracle.model_ref import portable_fill_
    for name, b in sorted(model.named_buffers(), key=lambda kv: kv[0]):
        s = (zlib.crc32(name.encode()) + seed * 7919) & 0x7FFFFFFF
        if name.endswith("running_mean"):
            portable_fill_(b.data, s, scale=0.1, kind="normal")
        elif name.endswith("running_var"):
            portable_fill_(b.data, s, scale=0.25, kind="uniform")
            b.data.add_(1.0)
    return model


def seeded_checkpoint(model, path, epoch=3):
    """portable_init_(seed 31) weights + fill_bn_stats_, saved as the reference's checkpoint dict with DataParallel's
    ``module.`` prefix on every name."""
    from oracle.model_ref import portable_init_
    portable_init_(model, seed=31)
    fill_bn_stats_(model)
    sd = {"module." + k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    torch.save({"model": sd, "epoch": epoch}, path)


def encoder_input():
    from oracle.model_ref import portable_fill_
    return portable_fill_(torch.empty(2, 3, 16, 112, 112), 77, kind="normal")


# ------------------------------------------------------------------ restatement
def average(features, vid_indices, labels, norm):
    """-> (mean features float64 [V, D], video ids [V], labels [V]) with videos in the order of their first clip."""
    f = np.asarray(features, dtype=np.float64)
    if norm:
        f = f / np.sqrt((f ** 2).sum(1, keepdims=True))
    vid = np.asarray(vid_indices)
    _, first = np.unique(vid, return_index=True)
    order = np.sort(first)
    out = np.stack([f[vid == vid[i]].mean(0) for i in order])
    return out, vid[order], np.asarray(labels)[order]


def sq_distances(queries, bank):
    q, t = np.asarray(queries, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    return ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1) if q.shape[0] * t.shape[0] * q.shape[1] < 5e7 else \
        np.maximum((q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2.0 * q @ t.T, 0.0)


def knn(queries, bank, k):
    """-> (d2 [Q, k], idx [Q, k]) ascending, ties to the lower index."""
    d2 = sq_distances(queries, bank)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d2, idx, 1), idx


def min_gap(queries, bank, cutoffs=RECALL_AT):
    """Smallest gap, over all queries, between the Euclidean distances of the k-th and (k+1)-th nearest for k in
    ``cutoffs`` (RECALL_AT: the recall values and label sets are well defined; range(1, 51): so is every list's order)."""
    d = np.sqrt(np.sort(sq_distances(queries, bank), axis=1))
    return float(min((d[:, k] - d[:, k - 1]).min() for k in cutoffs))


def recall(train_labels, val_labels, idx):
    """-> (mean recall per threshold {k: float}, recal_acc [Q, 5])."""
    train_labels, val_labels = np.asarray(train_labels), np.asarray(val_labels)
    rec = {k: [] for k in RECALL_AT}
    acc = np.zeros((len(val_labels), len(RECALL_AT)))
    for i, lab in enumerate(val_labels):
        for j, k in enumerate(RECALL_AT):
            labs = set(train_labels[idx[i, :k]].tolist())
            rec[k].append(100 if lab in labs else 0)
            acc[i, j] = (1 if lab in labs else 0) / float(len(labs))
    return {k: float(np.mean(v)) for k, v in rec.items()}, acc


def recall_lines(task, means):
    return [f"{task}: Recall @ {k}: {np.float64(means[k])}" for k in RECALL_AT]

