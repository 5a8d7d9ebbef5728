"""Timings of fine-tuning on the device (selavi_amd.finetune_video, csrc/finetune.hip) at the reference's shape: batch 32,
32 frames, 128^2 crops (augtype 1), K = 101 (UCF101), use_bn + use_l2_norm + dropout 0.7, device events.

    python tools/finetune_bench.py [--out profiles/finetune_bench.json] [--steps 10] [--trace-steps 0]

* full fine-tune step (trunk forward + fused head + backward + grouped SGD over 113 per-tensor groups), clips/s;
* the same step's trunk forward + backward alone (the head replaced by a precomputed feature gradient);
* linear-probe step (--feature_extract: trunk forward under no_grad, classifier-only SGD), clips/s;
* head forward + backward alone, and its launch count (B <= 64: one launch each way);
* optimizer steps alone: grouped SGD and Adam over the 113 tensors;
* eval views/s (eval-mode trunk + head).
``--trace-steps N``: run N full steps only (for rocprofv3 --kernel-trace --stats) and write nothing.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selavi_amd import finetune_video as fv  # noqa: E402
from selavi_amd import model as smodel, nn as snn, optim  # noqa: E402

B, T, S, K = 32, 32, 128, 101


def _events(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def _model(probe=False):
    av = smodel.load_model(use_mlp=True, num_classes=309, norm_feat=False, headcount=10)
    m = fv.Finetune_Model(av.video_network.base, 512, K, use_dropout=True, use_bn=True, use_l2_norm=True, dropout=0.7)
    m = m.cuda().train()
    m.feature_extract = probe
    return m


def _args(optim_name="sgd", probe=False):
    a = fv.parse_args([])
    a.optim_name, a.feature_extract = optim_name, probe
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/finetune_bench.json")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args()
    torch.manual_seed(0)
    x = torch.randn(B, 3, T, S, S).cuda()            # (made on the host: the traced run holds library kernels only)
    target = torch.randint(0, K, (B,)).cuda()
    one = torch.ones(()).cuda()
    res = {"shape": {"B": B, "T": T, "S": S, "K": K}, "device": torch.cuda.get_device_name()}

    m = _model()
    opt = fv.build_optimizer(_args(), m)

    def step():
        _, loss, _ = m(x, target)
        m.zero_grad(set_to_none=True)
        loss.backward(one)
        opt.step()

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    if a.trace_steps:
        for _ in range(a.trace_steps):
            step()
        torch.cuda.synchronize()
        print(f"traced {a.trace_steps} fine-tune steps")
        return
    t_step = _events(step, a.steps)
    res["finetune_step_ms"] = t_step * 1e3
    res["finetune_clips_per_s"] = B / t_step

    dfeat = (torch.randn(B, 512) * 1e-3).cuda()

    def trunk():
        feat = m.base(x)
        feat.backward(dfeat)
    trunk()
    res["trunk_fwd_bwd_ms"] = _events(trunk, a.steps) * 1e3

    feat = m.base(x).detach()
    W, bb = m.classifier.weight, m.classifier.bias
    bn = m.final_bn

    def head():
        fr = feat.requires_grad_(True)
        spec = snn.ClassifierSpec(bn, True, 0.7, True)
        _, loss, _ = snn.ClassifierHeadFunction.apply(spec, fr, target, W, bb, bn.weight, bn.bias)
        loss.backward()
    head()
    res["head_fwd_bwd_ms"] = _events(head, 50) * 1e3
    res["head_launches"] = {"forward": 1, "backward": 1, "note": "B <= 64: one workgroup each way (slv_ft_head_fwd/bwd)"}

    n_t = sum(1 for g in opt.param_groups for _ in g["params"])
    res["optimizer_tensors"] = n_t
    res["sgd_grouped_ms"] = _events(lambda: opt.step(), 50) * 1e3
    res["sgd_grouped_launches"] = (n_t + 47) // 48
    aopt = fv.build_optimizer(_args("adam"), m)
    aopt.step()
    res["adam_ms"] = _events(lambda: aopt.step(), 50) * 1e3
    res["adam_launches"] = (n_t + 47) // 48
    res["head_plus_sgd_share_of_step"] = (res["head_fwd_bwd_ms"] + res["sgd_grouped_ms"]) / res["finetune_step_ms"]
    del aopt

    mp = _model(probe=True)
    popt = fv.build_optimizer(_args(probe=True), mp)

    def probe_step():
        _, loss, _ = mp(x, target)
        popt.zero_grad()
        loss.backward()
        popt.step()
    probe_step()
    t_probe = _events(probe_step, a.steps)
    res["linear_probe_step_ms"] = t_probe * 1e3
    res["linear_probe_clips_per_s"] = B / t_probe

    m.eval()

    def ev():
        with torch.no_grad():
            m(x, target)
    ev()
    t_ev = _events(ev, a.steps)
    res["eval_views_per_s"] = B / t_ev
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
