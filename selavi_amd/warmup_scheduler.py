"""Gradual learning-rate warm-up (Goyal et al., "Accurate, Large Minibatch SGD", 2017) in front of a second scheduler: the
schedule finetune_video.py builds (:199-222): a linear warm-up to ``multiplier`` x the base rates over ``total_epoch``
epochs, then a MultiStepLR whose milestones were shifted by the warm-up.

Per-epoch rates (``e`` = number of ``step()`` calls so far, ``base`` = each group's initial lr):
  e <= total_epoch:  base * ((multiplier - 1) * e / total_epoch + 1)   (multiplier 1: base * e / total_epoch)
  e >  total_epoch:  the after-scheduler, started from base * multiplier at e = total_epoch + 1 and stepped once per
                     epoch after that (so a shifted milestone m takes effect at e = total_epoch + 1 + m);
                     without one: base * multiplier.
"""
import torch


class GradualWarmupScheduler(torch.optim.lr_scheduler.LRScheduler):
    def __init__(self, optimizer, multiplier, total_epoch, after_scheduler=None):
        if multiplier < 1.0:
            raise ValueError('multiplier should be greater than or equal to 1.')
        self.multiplier = multiplier
        self.total_epoch = total_epoch
        self.after_scheduler = after_scheduler
        self.finished = False
        super().__init__(optimizer)

    def _warm_factor(self, e):
        if self.multiplier == 1.0:
            return float(e) / self.total_epoch
        return (self.multiplier - 1.0) * e / self.total_epoch + 1.0

    def get_lr(self):
        e = self.last_epoch
        if e <= self.total_epoch:
            return [base * self._warm_factor(e) for base in self.base_lrs]
        peak = [base * self.multiplier for base in self.base_lrs]
        if self.after_scheduler is not None and not self.finished:
            # hand over: the after-scheduler continues from the peak rates, one step per epoch from here on
            self.after_scheduler.base_lrs = list(peak)
            self.finished = True
        return peak

    def step(self, epoch=None):
        if epoch is not None:
            raise ValueError("GradualWarmupScheduler steps once per epoch (no explicit epoch)")
        if self.finished and self.after_scheduler is not None:
            self.after_scheduler.step()
            self.last_epoch += 1
            self._last_lr = self.after_scheduler.get_last_lr()
        else:
            super().step()

    def state_dict(self):
        sd = {k: v for k, v in self.__dict__.items() if k not in ("optimizer", "after_scheduler")}
        sd["after_scheduler"] = self.after_scheduler.state_dict() if self.after_scheduler is not None else None
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        after = sd.pop("after_scheduler", None)
        self.__dict__.update(sd)
        if after is not None and self.after_scheduler is not None:
            self.after_scheduler.load_state_dict(after)
