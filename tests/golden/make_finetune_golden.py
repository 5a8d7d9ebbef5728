"""Golden vectors for fine-tuning, produced by EXECUTING the reference's finetune_video.py / utils.py /
src/warmup_scheduler.py in the build container (needs /root/reference; never run on the GPU box):

  (a) Finetune_Model (use_bn, use_l2_norm, no dropout, K = 11) on a portable-seeded r2plus1d_18 trunk
      (oracle.model_ref.portable_init_) and a portable-seeded classifier, B = 4, T = 4, S = 32: train-mode logits, loss
      and accuracy; parameters and BatchNorm running statistics after 2 SGD steps with the reference's per-tensor param
      groups; eval-mode logits afterwards;
  (b) accuracy / aggregrate_video_accuracy on seeded, tie-free logits with shuffled, repeated video ids;
  (c) the per-epoch learning rates of GradualWarmupScheduler + MultiStepLR for the default flags, for
      --lr_warmup_epochs 0 and for a multiplier-1 warm-up;
  (d) parse_args() defaults.

Only data is stored: no reference source.

    python tests/golden/make_finetune_golden.py        # writes tests/golden/finetune.npz
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import install_torchvision_standin  # noqa: E402
from oracle.model_ref import portable_init_  # noqa: E402
from tests import _finetune_ref as F  # noqa: E402

REF = "/root/reference"
SAMPLED = ["base.stem.0.weight", "base.layer1.0.conv1.0.0.weight", "base.layer4.1.conv2.0.3.weight",
           "base.layer4.1.conv2.1.weight"]
BUFFERS = ["final_bn.running_mean", "final_bn.running_var", "base.stem.1.running_mean", "base.layer4.1.conv2.1.running_var"]


def import_reference():
    install_torchvision_standin()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    ds = types.ModuleType("datasets")
    avd = types.ModuleType("datasets.AVideoDataset")

    class AVideoDataset:
        def __init__(self, *a, **k):
            raise RuntimeError("stub")
    avd.AVideoDataset = AVideoDataset
    ds.AVideoDataset = avd
    sys.modules["datasets"], sys.modules["datasets.AVideoDataset"] = ds, avd
    sys.path.insert(0, REF)
    import finetune_video as ref_ft            # /root/reference/finetune_video.py
    import utils as ref_utils                  # /root/reference/utils.py
    import model as ref_model
    from src.warmup_scheduler import GradualWarmupScheduler
    return ref_ft, ref_utils, ref_model, GradualWarmupScheduler


def view_falls_back_to_reshape():
    """utils.accuracy's ``correct[:k].view(-1)`` on a transposed tensor raises under torch >= 1.13 (it ran on the torch
    1.x the reference was written for): while the golden is made, a view that cannot alias falls back to a reshape."""
    orig = torch.Tensor.view

    def view(self, *shape):
        try:
            return orig(self, *shape)
        except RuntimeError:
            return self.reshape(*shape)
    torch.Tensor.view = view


def sample(t):
    return t.detach().reshape(-1)[:256].numpy().copy()


def lr_trace(Sched, warm, mult, epochs=12, milestones="6,10", gamma=0.05, lrs=(0.0025, 0.00025)):
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in lrs]
    opt = torch.optim.SGD([{'params': p, 'lr': lr} for p, lr in zip(ps, lrs)], lr=lrs[0], momentum=0.9)
    ms = [int(m) - warm for m in milestones.split(',')]
    if warm > 0:
        sch = Sched(opt, multiplier=mult, total_epoch=warm,
                    after_scheduler=torch.optim.lr_scheduler.MultiStepLR(opt, milestones=ms, gamma=gamma))
    else:
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=ms, gamma=gamma)
    out = []
    for _ in range(epochs):
        out.append([g['lr'] for g in opt.param_groups])
        opt.step()
        sch.step()
    return np.array(out)


def main():
    import warnings
    warnings.filterwarnings("ignore")
    ref_ft, ref_utils, ref_model, Sched = import_reference()
    view_falls_back_to_reshape()
    out = {}
    # (a)
    av = ref_model.load_model(vid_base_arch='r2plus1d_18', aud_base_arch='resnet9', pretrained=False, num_classes=309,
                              norm_feat=False, use_mlp=True, headcount=1)
    portable_init_(av, seed=37)
    m = ref_ft.Finetune_Model(av.video_network.base, 512, F.K, use_dropout=False, use_bn=True, use_l2_norm=True,
                              dropout=0.7)
    w, b = F.seeded_classifier()
    with torch.no_grad():
        m.classifier.weight.copy_(w)
        m.classifier.bias.copy_(b)
    params = [{'params': p, 'lr': F.HEAD_LR, 'weight_decay': F.WD} for p in m.classifier.parameters()]
    params += [{'params': p, 'lr': F.BASE_LR, 'weight_decay': F.WD} for p in m.base.parameters()]
    opt = torch.optim.SGD(params, lr=F.HEAD_LR, momentum=F.MOMENTUM, weight_decay=F.WD)
    x, target = F.model_input()
    crit = torch.nn.CrossEntropyLoss()
    m.train()
    for step in range(2):
        logits = m(x)
        loss = crit(logits, target)
        acc1, acc5 = ref_utils.accuracy(logits, target, topk=(1, 5))
        out[f"train_logits_{step}"] = logits.detach().numpy()
        out[f"train_loss_{step}"] = np.array([loss.item()])
        out[f"train_acc_{step}"] = np.array([acc1.item(), acc5.item()])
        opt.zero_grad()
        loss.backward()
        opt.step()
    sd = m.state_dict()
    out["classifier_weight"] = sd["classifier.weight"].numpy()
    out["classifier_bias"] = sd["classifier.bias"].numpy()
    for name in SAMPLED:
        out["param:" + name] = sample(sd[name])
    for name in BUFFERS:
        out["buf:" + name] = sd[name].numpy().copy()
    out["state_dict_keys"] = np.array(sorted(sd.keys()))
    m.eval()
    with torch.no_grad():
        out["eval_logits"] = m(x).numpy()
    # (b)
    logits, targets, vids = F.acc_case()
    lt = torch.from_numpy(logits)
    acc = ref_utils.accuracy(lt, torch.from_numpy(targets), topk=(1, 5))
    softmaxes, labels = {}, {}
    for j in range(len(vids)):
        softmaxes.setdefault(int(vids[j]), []).append(lt[j])
        labels[int(vids[j])] = torch.tensor(targets[j])
    vacc = ref_utils.aggregrate_video_accuracy(softmaxes, labels, topk=(1, 5))
    out["acc_logits"], out["acc_targets"], out["acc_vids"] = logits, targets, vids
    out["acc_clip"] = np.array([a.item() for a in acc])
    out["acc_video"] = np.array([a.item() for a in vacc])
    # (c)
    out["lr_default"] = lr_trace(Sched, 2, 8)
    out["lr_nowarmup"] = lr_trace(Sched, 0, 8)
    out["lr_mult1"] = lr_trace(Sched, 3, 1.0)
    # (d)
    argv = sys.argv
    sys.argv = ["finetune_video.py"]
    try:
        out["parse_args_defaults"] = np.array(json.dumps(vars(ref_ft.parse_args()), sort_keys=True))
    finally:
        sys.argv = argv
    np.savez_compressed(os.path.join(HERE, "finetune.npz"), **out)
    print({k: v.shape for k, v in out.items()})
    print("loss", out["train_loss_0"], out["train_loss_1"], "acc", out["acc_clip"], out["acc_video"])


if __name__ == "__main__":
    main()
