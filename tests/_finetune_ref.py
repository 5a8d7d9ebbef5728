"""Float64 restatements and seeded inputs shared by the fine-tuning golden maker (tests/golden/make_finetune_golden.py)
and the tests (tests/test_finetune_cpu.py, tests/test_finetune_gpu.py)."""
import numpy as np
import torch

from oracle.model_ref import portable_fill_

B, T, S, K = 4, 4, 32, 11             # the model-parity case of finetune.npz
HEAD_LR, BASE_LR, MOMENTUM, WD = 0.01, 1e-4, 0.9, 0.005


def model_input():
    x = portable_fill_(torch.empty(B, 3, T, S, S), 71)
    target = torch.tensor([3, 0, 10, 3], dtype=torch.int64)
    return x, target


def seeded_classifier(k=K):
    w = portable_fill_(torch.empty(k, 512), 73, scale=0.05)
    b = portable_fill_(torch.empty(k), 74, scale=0.1)
    return w, b


def acc_case(n_videos=12, k=K, seed=5):
    """Seeded tie-free logits of clips with shuffled, repeated video ids; every clip of a video has its label."""
    g = np.random.RandomState(seed)
    counts = g.randint(1, 5, size=n_videos)
    vids = np.repeat(np.arange(n_videos) * 3 + 7, counts)
    g.shuffle(vids)
    labels = g.randint(0, k, size=n_videos)
    targets = labels[(vids - 7) // 3]
    logits = g.randn(len(vids), k).astype(np.float32)
    return logits, targets.astype(np.int64), vids.astype(np.int64)


def rank_counts(scores, targets, ks=(1, 5)):
    """#rows whose target ranks below k under #{j: z_j > z_t} + #{j < t: z_j == z_t} < k."""
    scores = np.asarray(scores, dtype=np.float64)
    out = []
    for k in ks:
        c = 0
        for z, t in zip(scores, targets):
            rank = int((z > z[t]).sum() + (z[:t] == z[t]).sum())
            c += rank < k
        out.append(c)
    return np.array(out, dtype=np.float64)


def video_means(outputs, targets, vids):
    """Per-video mean of the outputs in order of first appearance; the label of a video is that of its last clip."""
    order, rows = [], {}
    for i, v in enumerate(vids):
        if v not in rows:
            order.append(v)
            rows[v] = []
        rows[v].append(i)
    out = np.asarray(outputs, dtype=np.float64)
    means = np.stack([out[rows[v]].mean(0) for v in order])
    labels = np.array([targets[rows[v][-1]] for v in order])
    return means, labels


def video_accuracy(outputs, targets, vids, ks=(1, 5)):
    means, labels = video_means(outputs, targets, vids)
    return rank_counts(means, labels, ks) * 100.0 / len(labels)


def head_ref(x, W, b, gamma=None, beta=None, rmean=None, rvar=None, l2=False, train=False, mask=None, p=0.0,
             target=None, momentum=0.1, eps=1e-5):
    """Finetune_Model's head in float64 torch (autograd on): -> dict of logits, loss, u, new running stats."""
    x = x.double().detach().requires_grad_(True)
    W = W.double().detach().requires_grad_(True)
    b = b.double().detach().requires_grad_(True)
    out = {"x": x, "W": W, "b": b}
    u = torch.nn.functional.normalize(x, p=2, dim=1) if l2 else x
    v = u
    if gamma is not None:
        gamma = gamma.double().detach().requires_grad_(True)
        beta = beta.double().detach().requires_grad_(True)
        out["gamma"], out["beta"] = gamma, beta
        if train:
            mean = u.mean(0)
            var = u.var(0, unbiased=False)
            n = u.shape[0]
            out["rmean"] = (1 - momentum) * rmean.double() + momentum * mean.detach()
            out["rvar"] = (1 - momentum) * rvar.double() + momentum * var.detach() * n / (n - 1)
        else:
            mean, var = rmean.double(), rvar.double()
        v = (u - mean) / torch.sqrt(var + eps) * gamma + beta
    if train and p > 0:
        v = v * mask.double() / (1 - p)
    z = v @ W.t() + b
    out["logits"] = z
    if target is not None:
        out["loss"] = torch.nn.functional.cross_entropy(z, target.to(z.device))
    return out
