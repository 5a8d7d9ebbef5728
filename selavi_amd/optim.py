"""Fused multi-tensor SGD with the semantics of ``torch.optim.SGD(params, lr, momentum=0.9,
weight_decay=wd)`` as built by /root/reference/main.py:132-137 (no nesterov, no dampening;
first step buf = d).  One launch per 48 tensors instead of ~5 launches per tensor.

The fine-tuning script (finetune_video.py:150-173) builds one param group per tensor (head_lr / weight_decay for the
classifier, base_lr / wd_base for the trunk): when the groups' hyperparameters differ, SGD steps every tensor of every
group in one table with per-tensor lr / weight decay / momentum (slv_sgd_step_grouped), 48 tensors per launch.  Adam
(``--optim_name adam``) does the same with torch.optim.Adam's update."""
import math

import torch

from . import ops


def _live(groups):
    return [(g, p) for g in groups for p in g["params"] if p.grad is not None]


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    def _uniform(self):
        keys = {(g["lr"], g["momentum"], g["weight_decay"]) for g in self.param_groups}
        return len(keys) <= 1

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if not self._uniform():
            self._grouped_step()
            return loss
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            fresh, seasoned = [], []
            for p in ps:
                st = self.state[p]
                if "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                    fresh.append(p)
                else:
                    seasoned.append(p)
            for lst, first in ((fresh, True), (seasoned, False)):
                if lst:
                    ops.sgd_step([p.data for p in lst], [p.grad.contiguous() for p in lst],
                                 [self.state[p]["momentum_buffer"] for p in lst], group["lr"], group["momentum"],
                                 group["weight_decay"], first)
        return loss

    def _grouped_step(self):
        ps, gs, bufs, lrs, wds, mus, firsts = [], [], [], [], [], [], []
        for group, p in _live(self.param_groups):
            st = self.state[p]
            first = "momentum_buffer" not in st
            if first:
                st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
            ps.append(p.data)
            gs.append(p.grad.contiguous())
            bufs.append(st["momentum_buffer"])
            lrs.append(group["lr"])
            wds.append(group["weight_decay"])
            mus.append(group["momentum"])
            firsts.append(first)
        if ps:
            ops.sgd_step_grouped(ps, gs, bufs, lrs, wds, mus, firsts)


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight decay added to the gradient, not AdamW; no amsgrad) on one fused kernel: per-tensor
    step counts and bias corrections, lr and weight decay per group.  The state (``step`` as a CPU float tensor,
    ``exp_avg``, ``exp_avg_sq``) has torch's names, so optimizer state dicts carry over."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        launches = {}       # (beta1, beta2, eps) -> per-tensor lists: one table per key
        for group, p in _live(self.param_groups):
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            step = float(st["step"])
            beta1, beta2 = group["betas"]
            lst = launches.setdefault((beta1, beta2, group["eps"]), ([], [], [], [], [], [], []))
            lst[0].append(p.data)
            lst[1].append(p.grad.contiguous())
            lst[2].append(st["exp_avg"])
            lst[3].append(st["exp_avg_sq"])
            lst[4].append(group["lr"] / (1 - beta1 ** step))
            lst[5].append(math.sqrt(1 - beta2 ** step))
            lst[6].append(group["weight_decay"])
        for (beta1, beta2, eps), lst in launches.items():
            ops.adam_step(*lst, beta1, beta2, eps)
        return loss
