"""Mirror of the hot-path helpers of /root/reference/utils.py (get_loss :377-387,
warmup_batchnorm :389-418) on the HIP kernels."""
import time

import torch

from . import nn as snn


def get_loss(activations, targets, headcount=1):
    """utils.py:377-387: cross entropy (hc==1) or the mean over heads of per-head cross entropy.

    ``activations``: B x K tensor (hc==1) or the list of hc B x K tensors AVModel returns;
    ``targets``: int64 [B] or [B, hc].  One grouped softmax-CE kernel for all heads."""
    if headcount == 1:
        act = activations[0] if isinstance(activations, (list, tuple)) else activations
        return snn.GroupedCE.apply(act.unsqueeze(0), targets.reshape(-1, 1))
    stacked = getattr(activations, "stacked", None)
    if stacked is None:
        stacked = torch.stack(list(activations))
    return snn.GroupedCE.apply(stacked, targets)


def warmup_batchnorm(args, model, dataloader, batches=20, group=None):
    """utils.py:389-418: `batches` no-grad train-mode forwards to seed the BN running statistics.
    (The reference reads an undefined ``args.distributed`` at :412; here the barrier is taken
    whenever torch.distributed is initialised.)"""
    start = time.time()
    with torch.no_grad():
        model.train()
        for i, batch in enumerate(dataloader):
            video, audio = batch[0], batch[1]
            if i == batches:
                break
            _ = model(video.cuda(non_blocking=True), audio.cuda(non_blocking=True))
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.barrier(group=group) if group is not None else dist.barrier()
    return time.time() - start


def load_model_parameters(model, model_weights):
    """utils.py:264-274: copy a state dict into ``model`` by name -- a ``module.`` (DataParallel / DDP) prefix is dropped,
    names the model does not have are reported and skipped."""
    self_state = model.state_dict()
    for name, param in model_weights.items():
        if 'module.' in name:
            name = name.replace('module.', '')
        if name in self_state.keys():
            self_state[name].copy_(param)
        else:
            print("didnt load ", name)


# ------------------------------------------------------------------------------------------ fine-tuning (utils.py:191-374)
def save_checkpoint(args, epoch, model, optimizer, lr_scheduler, ckpt_freq=10):
    """utils.py:191-216: the reference's files and keys -- ``model_weights/model_{epoch}.pth`` every 10 epochs,
    ``checkpoints/checkpoint.pth`` always, ``checkpoints/ckpt_{epoch}.pth`` every ``ckpt_freq``; keys model (no
    ``module.`` prefix), optimizer, lr_scheduler (None without a scheduler, where the reference crashes), epoch
    (epoch + 1), args."""
    import os
    net = getattr(model, "module", model)
    checkpoint = {
        'model': net.state_dict(),
        'optimizer': optimizer.state_dict(),
        'lr_scheduler': lr_scheduler.state_dict() if lr_scheduler is not None else None,
        'epoch': epoch + 1,
        'args': args,
    }
    os.makedirs(os.path.join(args.output_dir, 'model_weights'), exist_ok=True)
    os.makedirs(os.path.join(args.output_dir, 'checkpoints'), exist_ok=True)
    if epoch % 10 == 0:
        torch.save(checkpoint, os.path.join(args.output_dir, 'model_weights', f'model_{epoch}.pth'))
    torch.save(checkpoint, os.path.join(args.output_dir, 'checkpoints', 'checkpoint.pth'))
    if epoch % ckpt_freq == 0:
        torch.save(checkpoint, os.path.join(args.output_dir, 'checkpoints', f'ckpt_{epoch}.pth'))
    print(f'Saving checkpoint to: {args.output_dir}', flush=True)
    print('Checkpoint saved', flush=True)


class AverageMeter(object):
    """utils.py:286-302: current value, sum, count and average."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def _percent(correct, n, topk):
    """[2] correct@1 / correct@5 counts -> the reference's list of [1]-shaped percentages (device tensors)."""
    idx = {1: 0, 5: 1}
    for k in topk:
        if k not in idx:
            raise ValueError(f"top-{k}: the rank kernel counts top-1 and top-5")
    pct = correct * (100.0 / n)
    return [pct[idx[k]:idx[k] + 1] for k in topk]


def accuracy(output, target, topk=(1,)):
    """utils.py:336-351 on the device: percentages of rows whose target is in the top k (k in {1, 5}), each a [1]
    tensor.  Ties go to the lower class index (ops.topk_correct), where torch.topk leaves the order unspecified."""
    from . import ops
    out = output.reshape(target.shape[0], -1).float()
    return _percent(ops.topk_correct(out, target), target.shape[0], topk)


def video_accuracy(outputs, targets, video_idx, topk=(1,)):
    """aggregrate_video_accuracy on device tensors: outputs [N, K] (raw logits, as the reference averages them), targets
    and video ids [N].  The outputs of each video are averaged in clip order (ops.segment_mean, videos in order of first
    appearance), the video's label is that of its last clip (the reference's ``labels[video_id] = label``), and the
    averages are ranked by the top-k kernel.  -> list of [1] percentages."""
    from . import ops
    means, _, _, _ = ops.segment_mean(outputs.float(), video_idx, normalize=False)
    vid = video_idx.to(device=outputs.device, dtype=torch.int64)
    uniq, inv = torch.unique(vid, return_inverse=True)
    rows = torch.arange(vid.shape[0], device=outputs.device)
    first = torch.full((uniq.shape[0],), vid.shape[0], dtype=torch.int64, device=outputs.device).scatter_reduce_(
        0, inv, rows, reduce="amin")
    last = torch.full((uniq.shape[0],), -1, dtype=torch.int64, device=outputs.device).scatter_reduce_(
        0, inv, rows, reduce="amax")
    labels = targets.to(device=outputs.device, dtype=torch.int64)[last[torch.argsort(first)]]
    return _percent(ops.topk_correct(means, labels), means.shape[0], topk)


def aggregrate_video_accuracy(softmaxes, labels, topk=(1,), aggregate="mean"):
    """utils.py:354-374: ``softmaxes`` {video_id: [outputs of its clips]}, ``labels`` {video_id: label} (the reference's
    dicts) -> list of [1] percentages.  The clips are laid out in dict order and go through video_accuracy."""
    assert aggregate == "mean"
    outs, vids, tgts = [], [], []
    for v, lst in softmaxes.items():
        for o in lst:
            outs.append(o.reshape(-1))
            vids.append(v)
            tgts.append(int(labels[v]))
    dev = outs[0].device
    return video_accuracy(torch.stack(outs), torch.tensor(tgts, device=dev), torch.tensor(vids, device=dev), topk)
