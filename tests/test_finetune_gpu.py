"""Fine-tuning on the MI355X (csrc/finetune.hip, nn.ClassifierHeadFunction, optim.SGD grouped / Adam,
selavi_amd.finetune_video) against float64 restatements (tests/_finetune_ref.py), torch's optimizers, the CPU oracle
trunk and the executed reference (tests/golden/finetune.npz)."""
import os

import numpy as np
import pytest
import torch

from tests import _finetune_ref as F

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "finetune.npz")
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _close(got, want, rtol, atol, what=""):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    assert err <= atol + rtol * scale, (what, err, scale)


# ------------------------------------------------------------------ 1. head forward + backward
def _head_case(B, K, l2, bn, drop, train, seed):
    from selavi_amd import nn as snn
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 512, generator=g) * 3
    W, b = torch.randn(K, 512, generator=g) * 0.05, torch.randn(K, generator=g) * 0.1
    R = torch.randn(B, K, generator=g)
    target = torch.randint(0, K, (B,), generator=g)
    mask = (torch.rand(B, 512, generator=g) > 0.7).float()
    hold = None
    if bn:
        hold = snn.BatchNorm1d(512)
        with torch.no_grad():
            hold.weight.copy_(1 + 0.3 * torch.randn(512, generator=g))
            hold.bias.copy_(0.2 * torch.randn(512, generator=g))
            hold.running_mean.copy_(0.05 * torch.randn(512, generator=g))
            hold.running_var.copy_(0.5 + torch.rand(512, generator=g))
    return x, W, b, R, target, mask, hold


@pytest.mark.parametrize("K", [7, 51, 101])
@pytest.mark.parametrize("B", [2, 33, 64, 65, 256])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("l2,bn,drop", [(l, b, d) for l in (0, 1) for b in (0, 1) for d in (0, 1)])
def test_head_forward_backward(B, K, l2, bn, drop, train):
    from selavi_amd import nn as snn
    p = 0.7
    x, W, b, R, target, mask, hold = _head_case(B, K, l2, bn, drop, train, seed=B * 1000 + K * 10 + l2 * 4 + bn * 2 + drop)
    ref = F.head_ref(x, W, b, *((hold.weight, hold.bias, hold.running_mean, hold.running_var) if bn else (None,) * 4),
                     l2=bool(l2), train=train, mask=mask if drop else None, p=p if drop else 0.0, target=target)
    (ref["loss"] * 0.5 + (ref["logits"] * R.double()).sum()).backward()
    if bn:
        hold = hold.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    Wg, bg = W.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    ga = hold.weight if bn else None
    be = hold.bias if bn else None
    if bn:
        ga.grad = be.grad = None
    spec = snn.ClassifierSpec(hold, bool(l2), p if drop else 0.0, train, mask=mask.to(DEV) if drop else None)
    logits, loss, correct = snn.ClassifierHeadFunction.apply(spec, xg, target.to(DEV), Wg, bg, ga, be)
    (loss * 0.5 + (logits * R.to(DEV)).sum()).backward()
    # fp32 against float64: at B = 2 train-mode BatchNorm normalises a difference of two rows (x_hat = +-1), which
    # amplifies the rounding of the rows
    _close(logits, ref["logits"], 1e-4, 1e-5, "logits")
    _close(loss, ref["loss"], 1e-4, 1e-6, "loss")
    want = F.rank_counts(logits.detach().cpu().numpy(), target.numpy())
    assert np.array_equal(correct.cpu().numpy(), want), (correct, want)
    _close(xg.grad, ref["x"].grad, 1e-3, 1e-6, "dfeat")
    _close(Wg.grad, ref["W"].grad, 1e-4, 1e-5, "dW")
    _close(bg.grad, ref["b"].grad, 1e-4, 1e-5, "db")
    if bn:
        _close(ga.grad, ref["gamma"].grad, 1e-3, 1e-5, "dgamma")
        _close(be.grad, ref["beta"].grad, 1e-4, 1e-5, "dbeta")
        if train:
            _close(hold.running_mean, ref["rmean"], 1e-5, 1e-6, "running_mean")
            _close(hold.running_var, ref["rvar"], 1e-5, 1e-6, "running_var")


def test_head_dropout_draws_the_library_philox(monkeypatch):
    """Without an injected mask the head draws keep masks from Philox on (seed, offset): the masks of slv_dropout_masks."""
    from selavi_amd import nn as snn
    from selavi_amd._lib import C, ptr, stream
    B, K, p = 40, 13, 0.7
    x, W, b, R, target, _, _ = _head_case(B, K, 1, 0, 1, True, seed=9)
    monkeypatch.setattr(snn, "_dropout_stream", lambda: (0x1234567887654321, 99))
    m = torch.empty(B, 512, device=DEV)
    C.slv_dropout_masks(0x1234567887654321, 99, p, ptr(m), m.numel(), 0, 0, stream())
    ref = F.head_ref(x, W, b, l2=True, train=True, mask=m.cpu(), p=p, target=target)
    ref["loss"].backward()
    xg = x.to(DEV).requires_grad_(True)
    spec = snn.ClassifierSpec(None, True, p, True)
    logits, loss, _ = snn.ClassifierHeadFunction.apply(spec, xg, target.to(DEV), W.to(DEV), b.to(DEV), None, None)
    loss.backward()
    _close(logits, ref["logits"], 1e-5, 1e-5, "logits")
    _close(xg.grad, ref["x"].grad, 1e-4, 1e-6, "dfeat")


# ------------------------------------------------------------------ 2. top-k kernel
@pytest.mark.parametrize("N,K,tied", [(1, 7, False), (300, 101, False), (257, 51, True), (64, 5, True), (1000, 3, True)])
def test_topk_correct(N, K, tied):
    from selavi_amd import ops
    g = torch.Generator().manual_seed(N + K)
    z = torch.randn(N, K, generator=g)
    if tied:
        z = torch.round(z * 2) / 2             # many ties
    t = torch.randint(0, K, (N,), generator=g)
    got = ops.topk_correct(z.to(DEV), t.to(DEV)).cpu().numpy()
    assert np.array_equal(got, F.rank_counts(z.numpy(), t.numpy())), got


# ------------------------------------------------------------------ 3. video accuracy
def test_video_accuracy_matches_reference(gold):
    from selavi_amd import utils
    lo, tg, vi = (torch.from_numpy(gold[k]).to(DEV) for k in ("acc_logits", "acc_targets", "acc_vids"))
    a1, a5 = utils.video_accuracy(lo, tg, vi, topk=(1, 5))
    np.testing.assert_allclose([a1.item(), a5.item()], gold["acc_video"], rtol=1e-6)
    c1, c5 = utils.accuracy(lo, tg, topk=(1, 5))
    np.testing.assert_allclose([c1.item(), c5.item()], gold["acc_clip"], rtol=1e-6)
    softmaxes, labels = {}, {}
    for j in range(lo.shape[0]):
        softmaxes.setdefault(int(vi[j]), []).append(lo[j])
        labels[int(vi[j])] = tg[j]
    d1, d5 = utils.aggregrate_video_accuracy(softmaxes, labels, topk=(1, 5))
    np.testing.assert_allclose([d1.item(), d5.item()], gold["acc_video"], rtol=1e-6)


# ------------------------------------------------------------------ 4. optimizers
def _tensors(n, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(int(s),) for s in torch.randint(1, 9000, (n,), generator=g)]
    shapes[3] = (64, 3, 7, 7)
    return [torch.randn(*s, generator=g) for s in shapes], [[torch.randn(*s, generator=g) for s in shapes]
                                                          for _ in range(3)]


def test_sgd_grouped_matches_torch():
    from selavi_amd import optim
    ps0, grads = _tensors(113, 1)
    mine = [p.clone().to(DEV).requires_grad_(True) for p in ps0]
    ref = [p.clone().to(DEV).requires_grad_(True) for p in ps0]
    hp = [(0.05 if i < 2 else 0.005, 0.005 if i % 3 else 0.0) for i in range(len(ps0))]
    o1 = optim.SGD([{'params': p, 'lr': lr, 'weight_decay': wd} for p, (lr, wd) in zip(mine, hp)], lr=0.05, momentum=0.9)
    o2 = torch.optim.SGD([{'params': p, 'lr': lr, 'weight_decay': wd} for p, (lr, wd) in zip(ref, hp)], lr=0.05,
                         momentum=0.9, foreach=False)
    for step in range(3):
        for a, r, gr in zip(mine, ref, grads[step]):
            a.grad, r.grad = gr.to(DEV), gr.to(DEV)
        o1.step()
        o2.step()
    for a, r in zip(mine, ref):
        torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)


def test_sgd_single_group_bits_unchanged():
    """One group (or groups that share their hyperparameters) keeps the per-group slv_sgd_step launches, bit for bit."""
    from selavi_amd import ops, optim
    ps0, grads = _tensors(60, 2)
    mine = [p.clone().to(DEV).requires_grad_(True) for p in ps0]
    old = [p.clone().to(DEV) for p in ps0]
    bufs = [torch.empty_like(p) for p in old]
    opt = optim.SGD([{'params': mine[:30]}, {'params': mine[30:]}], lr=0.01, momentum=0.9, weight_decay=1e-4)
    assert opt._uniform()
    for step in range(3):
        for a, gr in zip(mine, grads[step]):
            a.grad = gr.to(DEV)
        opt.step()
        for lo, hi in ((0, 30), (30, 60)):
            ops.sgd_step(old[lo:hi], [g.to(DEV) for g in grads[step][lo:hi]], bufs[lo:hi], 0.01, 0.9, 1e-4, step == 0)
    for a, o in zip(mine, old):
        assert torch.equal(a.detach(), o)


def test_adam_matches_torch():
    from selavi_amd import optim
    ps0, grads = _tensors(70, 3)
    mine = [p.clone().to(DEV).requires_grad_(True) for p in ps0]
    ref = [p.clone().to(DEV).requires_grad_(True) for p in ps0]
    hp = [(1e-3 if i < 2 else 1e-4, 0.005 if i % 2 else 0.0) for i in range(len(ps0))]
    o1 = optim.Adam([{'params': p, 'lr': lr, 'weight_decay': wd} for p, (lr, wd) in zip(mine, hp)], lr=1e-3)
    o2 = torch.optim.Adam([{'params': p, 'lr': lr, 'weight_decay': wd} for p, (lr, wd) in zip(ref, hp)], lr=1e-3,
                          foreach=False)
    for step in range(3):
        for i, (a, r, gr) in enumerate(zip(mine, ref, grads[step])):
            if step == 1 and i == 5:          # a tensor without a gradient this step keeps its own step count
                a.grad = r.grad = None
                continue
            a.grad, r.grad = gr.to(DEV), gr.to(DEV)
        o1.step()
        o2.step()
    for a, r in zip(mine, ref):
        torch.testing.assert_close(a.detach(), r.detach(), rtol=1e-6, atol=1e-7)
    assert float(o1.state[mine[5]]["step"]) == 2.0


# ------------------------------------------------------------------ 5. model parity with the reference
def _ft_model(K=F.K, use_bn=True, use_l2_norm=True, use_dropout=False, seed=37):
    from oracle.model_ref import portable_init_
    from selavi_amd import finetune_video as fv
    from selavi_amd import model as smodel
    av = smodel.load_model(use_mlp=True, num_classes=309, norm_feat=False, headcount=1)
    portable_init_(av, seed=seed)
    m = fv.Finetune_Model(av.video_network.base, 512, K, use_dropout=use_dropout, use_bn=use_bn,
                          use_l2_norm=use_l2_norm, dropout=0.7)
    w, b = F.seeded_classifier(K)
    with torch.no_grad():
        m.classifier.weight.copy_(w)
        m.classifier.bias.copy_(b)
    return m.to(DEV)


def test_finetune_model_matches_reference(gold):
    from selavi_amd import optim
    m = _ft_model()
    params = [{'params': p, 'lr': F.HEAD_LR, 'weight_decay': F.WD} for p in m.classifier.parameters()]
    params += [{'params': p, 'lr': F.BASE_LR, 'weight_decay': F.WD} for p in m.base.parameters()]
    opt = optim.SGD(params, lr=F.HEAD_LR, momentum=F.MOMENTUM, weight_decay=F.WD)
    assert not opt._uniform()
    x, target = F.model_input()
    x, target = x.to(DEV), target.to(DEV)
    m.train()
    for step in range(2):
        logits, loss, correct = m(x, target)
        if step == 0:
            np.testing.assert_allclose(logits.detach().cpu().numpy(), gold["train_logits_0"], rtol=1e-3, atol=1e-3)
            np.testing.assert_allclose(loss.item(), gold["train_loss_0"][0], rtol=1e-3)
            np.testing.assert_allclose((correct * 100.0 / x.shape[0]).cpu().numpy(), gold["train_acc_0"], rtol=1e-5)
        else:
            # the second train-mode forward is ill-conditioned (final_bn over 4 rows): the reference's own fp32 and
            # fp64 runs differ by 6 % in its logits, so only the loss is held, at test_model_gpu's step-2 tolerance
            np.testing.assert_allclose(loss.item(), gold["train_loss_1"][0], rtol=6e-2)
        opt.zero_grad()
        loss.backward()
        opt.step()
    sd = m.state_dict()
    assert sorted(sd.keys()) == list(gold["state_dict_keys"])
    np.testing.assert_allclose(sd["classifier.weight"].cpu().numpy(), gold["classifier_weight"], rtol=5e-2, atol=5e-3)
    np.testing.assert_allclose(sd["classifier.bias"].cpu().numpy(), gold["classifier_bias"], rtol=5e-2, atol=5e-3)
    for k in gold.files:
        if k.startswith("param:"):
            got = sd[k[6:]].reshape(-1)[:256].cpu().numpy()
            np.testing.assert_allclose(got, gold[k], rtol=5e-2, atol=5e-3, err_msg=k)
        elif k.startswith("buf:"):
            np.testing.assert_allclose(sd[k[4:]].cpu().numpy(), gold[k], rtol=5e-2, atol=5e-3, err_msg=k)
    assert torch.equal(sd["final_bn.weight"].cpu(), torch.ones(512))          # not optimised, as in the reference
    m.eval()
    with torch.no_grad():
        np.testing.assert_allclose(m(x).cpu().numpy(), gold["eval_logits"], rtol=6e-2, atol=5e-3)


# ------------------------------------------------------------------ 6. trunk + head at the fine-tune shape (128^2)
def test_trunk_and_head_at_128_match_oracle():
    from oracle import model_ref
    from oracle.model_ref import portable_fill_, portable_init_
    m = _ft_model(K=101, seed=41)
    ref_av = model_ref.load_model(use_mlp=True, num_classes=309, norm_feat=False, headcount=1)
    portable_init_(ref_av, seed=41)
    base = ref_av.video_network.base
    x = portable_fill_(torch.empty(2, 3, 4, 128, 128), 43)
    target = torch.tensor([5, 100])
    w, b = F.seeded_classifier(101)
    w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    base.train()
    feat = base(x).reshape(2, -1)
    u = torch.nn.functional.normalize(feat, dim=1)
    v = torch.nn.functional.batch_norm(u, torch.zeros(512), torch.ones(512), torch.ones(512), torch.zeros(512), True)
    z = v @ w.t() + b
    loss_ref = torch.nn.functional.cross_entropy(z, target)
    loss_ref.backward()
    m.train()
    logits, loss, _ = m(x.to(DEV), target.to(DEV))
    loss.backward()
    np.testing.assert_allclose(loss.item(), loss_ref.item(), rtol=1e-3)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), z.detach().numpy(), rtol=2e-3, atol=2e-3)
    _close(m.classifier.weight.grad, w.grad, 2e-3, 1e-5, "dW")
    ref_p = dict(base.named_parameters())
    for name, p in m.base.named_parameters():
        if name in ("stem.0.weight", "layer1.0.conv1.0.0.weight", "layer4.1.conv2.0.3.weight", "layer4.0.downsample.0.weight"):
            _close(p.grad, ref_p[name].grad, 2e-2, 1e-6, name)


# ------------------------------------------------------------------ 7. linear probe
def test_linear_probe_skips_trunk_backward():
    from selavi_amd import optim
    x, target = F.model_input()
    x, target = x.to(DEV), target.to(DEV)
    runs = {}
    for probe in (True, False):
        m = _ft_model(use_dropout=False)
        m.feature_extract = probe
        m.train()
        opt = optim.SGD([{'params': p, 'lr': 0.05, 'weight_decay': 0.005} for p in m.classifier.parameters()], lr=0.05,
                        momentum=0.9)
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        _, loss, _ = m(x, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        runs[probe] = (before, {k: v.detach().clone() for k, v in m.state_dict().items()},
                       [p.grad for p in m.base.parameters()])
    before, after, grads = runs[True]
    assert all(g is None for g in grads)
    for k in before:
        if k.startswith("base.") and ("running" in k):
            assert not torch.equal(before[k], after[k]), k
            assert torch.equal(after[k], runs[False][1][k]), k
        elif k.startswith("base.") and "num_batches" not in k:
            assert torch.equal(before[k], after[k]), k
    for k in ("classifier.weight", "classifier.bias", "final_bn.running_mean", "final_bn.running_var"):
        assert torch.equal(after[k], runs[False][1][k]), k


# ------------------------------------------------------------------ 8. end to end
def test_main_end_to_end(tmp_path, capsys, monkeypatch):
    from selavi_amd import finetune_video as fv
    torch.manual_seed(0)
    trained = []
    real_train, real_eval = fv.train, fv.evaluate
    evals = []
    monkeypatch.setattr(fv, "train", lambda *a, **k: trained.append(real_train(*a, **k)) or trained[-1])
    monkeypatch.setattr(fv, "evaluate", lambda *a, **k: evals.append(real_eval(*a, **k)) or evals[-1])
    argv = ["--dataset", "synthetic", "--fold", "1,2", "--epochs", "3", "--clip_len", "4", "--synthetic_crop", "32",
            "--batch_size", "8", "--synthetic_videos", "24", "--train_clips_per_video", "2", "--val_clips_per_video", "1",
            "--num_spatial_crops", "2", "--use_bn", "True", "--use_l2_norm", "True", "--use_dropout", "False",
            "--head_lr", "0.005", "--base_lr", "0.0005", "--use_scheduler", "False",
            "--output_dir", str(tmp_path)]
    acc1, acc5, epochs = fv.run_folds(fv.parse_args(argv))
    out = capsys.readouterr().out
    assert "2-Fold (synthetic)" in out and "Vid Acc@1" in out and "Video Acc@5" in out
    assert len(trained) == 6 and len(epochs) == 2
    for fold in range(2):
        ls = [t[1] for t in trained[3 * fold:3 * fold + 3]]
        assert all(np.isfinite(ls)), ls
        assert ls[2] < ls[0], ls
    for f in ("model_weights/model_0.pth", "checkpoints/checkpoint.pth", "checkpoints/ckpt_0.pth",
              "checkpoints/ckpt_1.pth", "checkpoints/ckpt_2.pth"):
        assert (tmp_path / f).exists(), f
    ck = torch.load(tmp_path / "checkpoints" / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "epoch", "args"} and ck["epoch"] == 3
    assert not any(k.startswith("module.") for k in ck["model"]) and "classifier.weight" in ck["model"]
    last_vid_acc = evals[-1][1]
    # --resume: continues at the saved epoch (fold 2's checkpoint)
    trained.clear()
    a = fv.parse_args(argv + ["--resume", "1", "--epochs", "4", "--fold", "2"])
    fv.main(a)
    assert [t[0] for t in trained] == [3]
    # --test_only: the last evaluation's video accuracy, from the checkpoint of the run before
    torch.save(ck, tmp_path / "checkpoints" / "checkpoint.pth")
    a = fv.parse_args(argv + ["--resume", "1", "--test_only", "True", "--fold", "2"])
    vid_acc1, _, ep = fv.main(a)
    assert ep == 3 and vid_acc1 == last_vid_acc
