"""Fine-tuning pieces that need no GPU, against the executed reference (tests/golden/finetune.npz): the learning-rate
schedule, the command-line defaults, and the float64 restatement of the top-k rule and the video-level aggregation that
the GPU tests hold the kernels to."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _finetune_ref as F

GOLD = os.path.join(os.path.dirname(__file__), "golden", "finetune.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _trace(warm, mult, epochs=12, milestones="6,10", gamma=0.05, lrs=(0.0025, 0.00025)):
    from selavi_amd.warmup_scheduler import GradualWarmupScheduler
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in lrs]
    opt = torch.optim.SGD([{'params': p, 'lr': lr} for p, lr in zip(ps, lrs)], lr=lrs[0], momentum=0.9)
    ms = [int(m) - warm for m in milestones.split(',')]
    if warm > 0:
        sch = GradualWarmupScheduler(opt, multiplier=mult, total_epoch=warm,
                                     after_scheduler=torch.optim.lr_scheduler.MultiStepLR(opt, milestones=ms, gamma=gamma))
    else:
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=ms, gamma=gamma)
    out = []
    for _ in range(epochs):
        out.append([g['lr'] for g in opt.param_groups])
        opt.step()
        sch.step()
    return np.array(out)


@pytest.mark.parametrize("key,warm,mult", [("lr_default", 2, 8), ("lr_nowarmup", 0, 8), ("lr_mult1", 3, 1.0)])
def test_scheduler_matches_reference(gold, key, warm, mult):
    np.testing.assert_allclose(_trace(warm, mult), gold[key], rtol=1e-12, atol=0)


def test_build_scheduler_follows_flags(gold):
    from selavi_amd import finetune_video as fv
    args = fv.parse_args([])
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in range(2)]
    opt = torch.optim.SGD([{'params': ps[0], 'lr': args.head_lr}, {'params': ps[1], 'lr': args.base_lr}], lr=1.0)
    sch = fv.build_scheduler(args, opt)
    got = []
    for _ in range(args.epochs):
        got.append([g['lr'] for g in opt.param_groups])
        sch.step()
    np.testing.assert_allclose(np.array(got), gold["lr_default"], rtol=1e-12, atol=0)
    sd = sch.state_dict()
    assert "optimizer" not in sd and isinstance(sd["after_scheduler"], dict)


def test_parse_args_defaults(gold):
    from selavi_amd import finetune_video as fv
    ref = json.loads(str(gold["parse_args_defaults"]))
    got = vars(fv.parse_args([]))
    assert {k: got[k] for k in ref} == ref
    assert set(got) - set(ref) == {"synthetic_videos", "synthetic_crop"}


def test_rank_rule_and_video_aggregation_match_reference(gold):
    logits, targets, vids = gold["acc_logits"], gold["acc_targets"], gold["acc_vids"]
    clip = F.rank_counts(logits, targets) * 100.0 / len(targets)
    np.testing.assert_allclose(clip, gold["acc_clip"], rtol=1e-6)
    np.testing.assert_allclose(F.video_accuracy(logits, targets, vids), gold["acc_video"], rtol=1e-6)


def test_rank_rule_breaks_ties_towards_lower_index():
    z = np.array([[1.0, 2.0, 2.0, 0.0, 2.0, 2.0, 2.0, 2.0]])
    # target 1: no larger value, no tie below it -> rank 0; target 2: one tie below (index 1) -> rank 1
    assert list(F.rank_counts(z, [1], ks=(1,))) == [1]
    assert list(F.rank_counts(z, [2], ks=(1,))) == [0]
    # target 7: ties at 1, 2, 4, 5, 6 below it -> rank 5: outside the top 5
    assert list(F.rank_counts(z, [7], ks=(1, 5))) == [0, 0]
    assert list(F.rank_counts(z, [6], ks=(1, 5))) == [0, 1]


def test_state_dict_keys_match_reference(gold):
    from selavi_amd import finetune_video as fv
    from selavi_amd import model as smodel
    av = smodel.load_model(use_mlp=True, num_classes=309, norm_feat=False, headcount=1)
    m = fv.Finetune_Model(av.video_network.base, 512, F.K, use_bn=True, use_l2_norm=True)
    assert sorted(m.state_dict().keys()) == list(gold["state_dict_keys"])
    w = m.classifier.weight.detach()
    np.testing.assert_allclose((w @ w.t()).numpy(), np.eye(F.K), atol=1e-5)     # orthogonal rows
    assert float(m.classifier.bias.abs().max()) == 0.0
