"""Fine-tuning the video trunk for action recognition on UCF101 / HMDB51 (mirror of /root/reference/finetune_video.py).

    python -m selavi_amd.finetune_video --dataset synthetic --fold 1,2 --epochs 3 --clip_len 4 --synthetic_crop 32 \
        --batch_size 8 --train_clips_per_video 2 --val_clips_per_video 1 --num_spatial_crops 2 --output_dir /tmp/ft

Same names, signatures, return values and checkpoint layout as the reference.  The classifier head with its loss and
accuracy epilogue is one autograd node over csrc/finetune.hip (nn.ClassifierHeadFunction) under the trunk's stage nodes;
the optimizer steps every per-tensor param group in one fused table (optim.SGD / optim.Adam).  Video decoding is out of
scope: ``main`` takes dataset objects yielding ``(video, target, _, video_idx)``; ``--dataset synthetic`` builds
data.SyntheticRetrievalDataset ones.  A dataset may hand out the video as augmented float32 ``3 x T x S x S`` clips, or
as decoded ``T x H x W x 3`` uint8 frames: those go through datasets.video_transforms.ClipAugmenter on the device
(resize / crop / flip, ``--colorjitter``, ``--test_time_cj``), set up the way the reference sets up AVideoDataset
(:176-207); a test set then carries the item's spatial-temporal index as the third item (AVideoDataset.py:370-380).
``--dataset synthetic_uint8`` builds synthetic sets of that kind.  A dataset that declares ``decoded_videos = True`` hands
out WHOLE decoded videos (data.SyntheticVideoDataset: ``--dataset synthetic_video``): its train clips and its
``val_clips_per_video x num_spatial_crops`` test views are cut on the device by datasets.av_batcher.DecodedAVBatcher,
set up like the reference's two AVideoDataset (:176-207), temporal sampling included.

Divergences from the reference (it crashes or wastes work there; nothing observable changes):
  - train / evaluate take what they need as arguments instead of reading a global ``args``;
  - ``lr_scheduler.step()`` is skipped when ``--use_scheduler False`` (the reference calls it on None);
  - the trunk's features are reshaped to [B, 512] instead of ``.squeeze()``d, so a last eval batch of one clip works;
  - ``--feature_extract True`` runs the trunk's train-mode forward under no_grad (BatchNorm running statistics update as
    in the reference) and skips the trunk backward whose gradients the reference computes and never uses;
  - no torch.nn.DataParallel: one GPU per process;
  - each step drops every gradient of the model (``model.zero_grad``), not only those of the optimised tensors: the
    gradients of final_bn, which the reference leaves out of the optimizer, do not pile up step after step (an extra
    accumulation launch per step that nothing reads).
"""
import datetime
import logging
import os
import sys
import time

import numpy as np
import torch
from torch import nn

from . import nn as snn
from . import ops, optim
from .datasets.av_batcher import DecodedAVBatcher
from .datasets.video_transforms import ClipAugmenter
from .model import load_model
from .utils import AverageMeter, load_model_parameters, save_checkpoint, video_accuracy
from .warmup_scheduler import GradualWarmupScheduler


class _StdoutHandler(logging.StreamHandler):
    """Writes to whatever sys.stdout is at the time of the record."""

    @property
    def stream(self):
        return sys.stdout

    @stream.setter
    def stream(self, value):
        pass


logger = logging.getLogger("selavi_amd.finetune_video")
if not logger.handlers:
    _h = _StdoutHandler()
    _h.setFormatter(logging.Formatter("%(levelname)s - %(asctime)s - %(message)s", "%x %X"))
    logger.addHandler(_h)
    logger.setLevel(logging.INFO)
    logger.propagate = False


# number of classes of each dataset
NUM_CLASSES = {
    'hmdb51': 51,
    'ucf101': 101,
    'synthetic': 11,
    'synthetic_uint8': 11,       # the synthetic sets as uint8 frames larger than the crop
    'synthetic_video': 11,       # the synthetic sets as whole decoded videos of differing lengths and sizes
}
SYNTHETIC = ('synthetic', 'synthetic_uint8', 'synthetic_video')


def get_video_dim(vid_base_arch='r2plus1d_18'):
    assert vid_base_arch == 'r2plus1d_18', "only r2plus1d_18 is on the hot path"
    return 512


class Finetune_Model(nn.Module):
    """finetune_video.py:44-92: the trunk plus [L2 norm] -> [BatchNorm1d] -> [Dropout] -> Linear.  Same attributes and
    state_dict keys (``base.*``, ``final_bn.*``, ``classifier.weight/bias``); the head runs as one autograd node.

    ``forward(x)`` returns the logits; ``forward(x, target)`` returns (logits, mean cross-entropy, [2] correct@1 / @5
    counts) from the same launch.  ``_dropout_mask`` (tests): a [B, 512] keep mask used instead of the Philox draw.
    ``feature_extract``: the trunk runs without autograd (the linear probe)."""

    def __init__(self, base_arch, num_ftrs=512, num_classes=101, use_dropout=False, use_bn=False, use_l2_norm=False,
                 dropout=0.9):
        super().__init__()
        self.base = base_arch
        self.use_bn = use_bn
        self.use_dropout = use_dropout
        self.use_l2_norm = use_l2_norm
        message = 'Classifier to %d classes;' % (num_classes)
        if use_dropout:
            message += ' + dropout %f' % dropout
        if use_l2_norm:
            message += ' + L2Norm'
        if use_bn:
            message += ' + final BN'
        print(message)
        if num_ftrs != 512:
            raise ValueError("the fused head takes 512-d trunk features")
        if self.use_bn:
            self.final_bn = snn.BatchNorm1d(num_ftrs)       # gamma 1, beta 0, eps 1e-5, momentum 0.1
        if self.use_dropout:
            self.dropout = nn.Dropout(dropout)              # holds p; the mask is drawn inside the head kernel
        self.classifier = nn.Linear(num_ftrs, num_classes)
        self._initialize_weights(self.classifier)
        self.feature_extract = False
        self._dropout_mask = None

    def _initialize_weights(self, module):
        for name, param in module.named_parameters():      # on the host, before the model moves to the GPU
            if 'bias' in name:
                nn.init.constant_(param, 0.0)
            elif 'weight' in name:
                nn.init.orthogonal_(param, 1)

    def features(self, x):
        if self.feature_extract and self.training:
            with torch.no_grad():
                feat = self.base(x)
        else:
            feat = self.base(x)
        return feat.reshape(feat.shape[0], -1)

    def forward(self, x, target=None):
        feat = self.features(x)
        bn = self.final_bn if self.use_bn else None
        p = self.dropout.p if (self.use_dropout and self.training) else 0.0
        spec = snn.ClassifierSpec(bn, self.use_l2_norm, p, self.training, mask=self._dropout_mask)
        return snn.ClassifierHeadFunction.apply(spec, feat.contiguous(), target, self.classifier.weight,
                                                self.classifier.bias, bn.weight if bn is not None else None,
                                                bn.bias if bn is not None else None)


def _crop_size(args):
    """finetune_video.py:183,198; ``--synthetic_crop`` shrinks it for the synthetic sets."""
    if args.dataset in SYNTHETIC and getattr(args, 'synthetic_crop', 0):
        return args.synthetic_crop
    return 128 if args.augtype == 1 else 224


def _jitter_scales(crop):
    """AVideoDataset.py:213-217."""
    if crop in (112, 128):
        return (128, 160)
    if crop == 224:
        return (256, 320)
    return (crop, crop * 5 // 4)  # a synthetic size the reference has no rule for: the 128 rule, in proportion


def build_augmenters(args):
    """The (train, test) ClipAugmenter for datasets that hand out uint8 frames, from the arguments the way the reference
    builds its two AVideoDataset (finetune_video.py:176-207, AVideoDataset.py:213-217,358-380): training draws scale,
    crop and flip (spatial_idx -1) with ``--colorjitter``; testing resizes the short side to the crop and takes view
    ``index % num_spatial_crops`` (given per clip in the call) with ``--test_time_cj``."""
    crop = _crop_size(args)
    scales = _jitter_scales(crop)
    train_aug = ClipAugmenter(spatial_idx=-1, min_scale=scales[0], max_scale=scales[1], crop_size=crop,
                              colorjitter=args.colorjitter)
    test_aug = ClipAugmenter(spatial_idx=1, min_scale=crop, max_scale=crop, crop_size=crop,
                             colorjitter=args.test_time_cj)
    return train_aug, test_aug


def build_batchers(args):
    """The (train, test) DecodedAVBatcher for datasets of whole decoded videos, with the keywords of the reference's two
    AVideoDataset (finetune_video.py:176-207)."""
    crop = _crop_size(args)
    train = DecodedAVBatcher(mode='train', num_frames=args.clip_len, sample_rate=args.steps_bet_clips,
                             train_crop_size=crop, train_jitter_scles=_jitter_scales(crop),
                             colorjitter=args.colorjitter, temp_jitter=True, center_crop=False, target_fps=30,
                             decode_audio=False)
    test = DecodedAVBatcher(mode='test', num_frames=args.clip_len, sample_rate=args.steps_bet_clips,
                            test_crop_size=crop, num_spatial_crops=args.num_spatial_crops,
                            num_ensemble_views=args.val_clips_per_video, colorjitter=args.test_time_cj,
                            temp_jitter=True, target_fps=30, decode_audio=False)
    return train, test


class DecodedVideoLoader:
    """A loader over a ``decoded_videos`` dataset (batches as its ``collate`` makes them) -> the batches train() and
    evaluate() take: ``(clips B x 3 x T x S x S float32 on the device, target, spatial_temporal_idx, video_idx)``.  The
    videos of a batch go to the device once each and the batcher cuts every item's clip from them."""

    def __init__(self, loader, batcher):
        self.loader, self.batcher, self.dataset = loader, batcher, loader.dataset

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        test = self.batcher.mode == 'test'
        for videos, fps, video_of, target, st_idx, video_idx in self.loader:
            videos = [v.cuda(non_blocking=True) for v in videos]
            clips, _ = self.batcher(videos, fps, spatial_temporal_idx=st_idx.tolist() if test else None,
                                    video_of=video_of)
            yield clips, target, st_idx, video_idx


def is_frames(video):
    """Decoded frames (B x T x H x W x 3 uint8) as opposed to augmented float clips (B x 3 x T x S x S)."""
    return video.dtype == torch.uint8 and video.dim() == 5 and video.shape[-1] == 3


def device_clips(video, augment, spatial_idx=None):
    """A batch as the loader hands it out -> B x 3 x T x S x S float32 on the device."""
    if not is_frames(video):
        return video.cuda(non_blocking=True)
    if augment is None:
        raise ValueError("the dataset hands out uint8 frames: train() / evaluate() need augment=ClipAugmenter(...)")
    return augment(video.cuda(non_blocking=True), spatial_idx=spatial_idx)


_noted = set()


def _note_colorjitter_without_frames():
    """Once per process: the flag is not dropped in silence."""
    if 'colorjitter' not in _noted:
        _noted.add('colorjitter')
        logger.info("--colorjitter True has no effect on this training set: it hands out float clips, and colour jitter "
                    "is part of the device clip augmentation of uint8 frames (see --dataset synthetic_uint8)")


def _synthetic_datasets(args):
    from .data import SyntheticFramesDataset, SyntheticRetrievalDataset, SyntheticVideoDataset
    S = _crop_size(args)
    fold = int(args.fold)
    if args.dataset == 'synthetic_video':
        # videos from a little shorter than a clip's span (clamped indices) to a few spans long
        lo, hi = max(args.clip_len * args.steps_bet_clips * 3 // 4, 2), args.clip_len * args.steps_bet_clips * 3
        train = SyntheticVideoDataset(n_videos=args.synthetic_videos, clips_per_video=args.train_clips_per_video,
                                      min_frames=lo, max_frames=hi, S=S, n_classes=NUM_CLASSES['synthetic'],
                                      seed=1000 + fold)
        test = SyntheticVideoDataset(n_videos=max(args.synthetic_videos // 2, 1),
                                     clips_per_video=args.num_spatial_crops * args.val_clips_per_video,
                                     min_frames=lo, max_frames=hi, S=S, n_classes=NUM_CLASSES['synthetic'],
                                     seed=2000 + fold)
        return train, test
    if args.dataset == 'synthetic_uint8':
        H, W = S * 5 // 4, S * 3 // 2                  # larger than the crop, landscape
        train = SyntheticFramesDataset(H, W, n_videos=args.synthetic_videos, clips_per_video=args.train_clips_per_video,
                                       T=args.clip_len, n_classes=NUM_CLASSES['synthetic'], seed=1000 + fold)
        test = SyntheticFramesDataset(H, W, n_videos=max(args.synthetic_videos // 2, 1),
                                      clips_per_video=args.num_spatial_crops * args.val_clips_per_video,
                                      T=args.clip_len, n_classes=NUM_CLASSES['synthetic'], seed=2000 + fold)
        return train, test
    train = SyntheticRetrievalDataset(n_videos=args.synthetic_videos, clips_per_video=args.train_clips_per_video,
                                      T=args.clip_len, S=S, n_classes=NUM_CLASSES['synthetic'], seed=1000 + fold)
    test = SyntheticRetrievalDataset(n_videos=max(args.synthetic_videos // 2, 1),
                                     clips_per_video=args.num_spatial_crops * args.val_clips_per_video,
                                     T=args.clip_len, S=S, n_classes=NUM_CLASSES['synthetic'], seed=2000 + fold)
    return train, test


def build_optimizer(args, model):
    """finetune_video.py:150-173 and :186-197: one param group per tensor -- the classifier at head_lr / weight_decay,
    then (unless feature_extract) the trunk at base_lr / wd_base.  final_bn is not optimised (it stays at 1 / 0)."""
    params = []
    for name, param in model.classifier.named_parameters():
        logger.info((name, param.shape))
        params.append({'params': param, 'lr': args.head_lr, 'weight_decay': args.weight_decay})
    if not args.feature_extract:
        for name, param in model.base.named_parameters():
            params.append({'params': param, 'lr': args.base_lr, 'weight_decay': args.wd_base})
    if args.optim_name == 'sgd':
        return optim.SGD(params, lr=args.head_lr, momentum=args.momentum, weight_decay=args.weight_decay)
    if args.optim_name == 'adam':
        return optim.Adam(params, lr=args.head_lr, weight_decay=args.weight_decay)
    raise ValueError(args.optim_name)


def build_scheduler(args, optimizer):
    """finetune_video.py:199-222."""
    if not args.use_scheduler:
        return None
    milestones = [int(lr) - args.lr_warmup_epochs for lr in args.lr_milestones.split(',')]
    if args.lr_warmup_epochs > 0:
        scheduler_step = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=milestones, gamma=args.lr_gamma)
        return GradualWarmupScheduler(optimizer, multiplier=8, total_epoch=args.lr_warmup_epochs,
                                      after_scheduler=scheduler_step)
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=milestones, gamma=args.lr_gamma)


def main(args, writer=None, dataset=None, dataset_test=None):
    """finetune_video.py:95-274 -> (best_vid_acc1, best_vid_acc5, best_epoch)."""
    logger.info("Loading model")
    model = load_model(vid_base_arch=args.vid_base_arch, aud_base_arch=args.aud_base_arch, pretrained=args.pretrained,
                       num_classes=args.num_clusters, norm_feat=False, use_mlp=args.use_mlp, headcount=args.headcount)
    weights = args.weights_path
    has_weights = (weights != 'None' and weights != '') if isinstance(weights, str) else weights is not None
    if not args.pretrained and has_weights:
        logger.info("Loading model weights")
        if os.path.exists(weights):
            ckpt_dict = torch.load(weights, map_location='cpu', weights_only=False)
            logger.info(f"Epoch checkpoint: {args.ckpt_epoch}")
            load_model_parameters(model, ckpt_dict["model"])
    logger.info("Loading model done")
    model = Finetune_Model(model.video_network.base, get_video_dim(vid_base_arch=args.vid_base_arch),
                           NUM_CLASSES[args.dataset], use_dropout=args.use_dropout, use_bn=args.use_bn,
                           use_l2_norm=args.use_l2_norm, dropout=0.7)
    model = model.cuda()
    model.feature_extract = bool(args.feature_extract)

    if dataset is None or dataset_test is None:
        if args.dataset not in SYNTHETIC:
            raise NotImplementedError("video decoding is out of scope: pass dataset= and dataset_test= "
                                      "(items (video, target, _, video_idx)) or use --dataset synthetic")
        dataset, dataset_test = _synthetic_datasets(args)
    logger.info("Creating data loaders")
    train_aug, test_aug = build_augmenters(args)
    decoded = getattr(dataset, 'decoded_videos', False), getattr(dataset_test, 'decoded_videos', False)
    data_loader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, sampler=None,
                                              num_workers=args.workers, pin_memory=True, drop_last=True, shuffle=True,
                                              collate_fn=dataset.collate if decoded[0] else None)
    data_loader_test = torch.utils.data.DataLoader(dataset_test, batch_size=args.batch_size, sampler=None,
                                                   num_workers=args.workers, pin_memory=True, drop_last=False,
                                                   collate_fn=dataset_test.collate if decoded[1] else None)
    if any(decoded):             # whole decoded videos: the batchers draw and apply temporal sampling and augmentation
        train_batcher, test_batcher = build_batchers(args)             # (--colorjitter / --test_time_cj included)
        if decoded[0]:
            data_loader, train_aug = DecodedVideoLoader(data_loader, train_batcher), None
        if decoded[1]:
            data_loader_test, test_aug = DecodedVideoLoader(data_loader_test, test_batcher), None
    nsc = args.num_spatial_crops

    optimizer = build_optimizer(args, model)
    lr_scheduler = build_scheduler(args, optimizer)

    if args.resume:
        ckpt_path = os.path.join(args.output_dir, 'checkpoints', 'checkpoint.pth')
        checkpoint = torch.load(ckpt_path, map_location='cpu', weights_only=False)
        model.load_state_dict(checkpoint['model'])
        optimizer.load_state_dict(checkpoint['optimizer'])
        if lr_scheduler is not None and checkpoint['lr_scheduler'] is not None:
            lr_scheduler.load_state_dict(checkpoint['lr_scheduler'])
        args.start_epoch = checkpoint['epoch']
        logger.info(f"Resuming from epoch: {args.start_epoch}")

    if args.test_only:
        _, vid_acc1, vid_acc5 = evaluate(model, data_loader_test, epoch=args.start_epoch, writer=writer, ds=args.dataset,
                                         augment=test_aug, num_spatial_crops=nsc)
        return vid_acc1, vid_acc5, args.start_epoch

    start_time = time.time()
    best_vid_acc_1, best_vid_acc_5, best_epoch = -1, -1, 0
    for epoch in range(args.start_epoch, args.epochs):
        logger.info(f'Start training epoch: {epoch}')
        train(model, optimizer, data_loader, epoch, writer=writer, ds=args.dataset, augment=train_aug)
        logger.info(f'Start evaluating epoch: {epoch}')
        if lr_scheduler is not None:
            lr_scheduler.step()
        _, vid_acc1, vid_acc5 = evaluate(model, data_loader_test, epoch=epoch, writer=writer, ds=args.dataset,
                                         augment=test_aug, num_spatial_crops=nsc)
        if vid_acc1 > best_vid_acc_1:
            best_vid_acc_1, best_vid_acc_5, best_epoch = vid_acc1, vid_acc5, epoch
        if args.output_dir:
            logger.info(f'Saving checkpoint to: {args.output_dir}')
            save_checkpoint(args, epoch, model, optimizer, lr_scheduler, ckpt_freq=1)
    total_time_str = str(datetime.timedelta(seconds=int(time.time() - start_time)))
    logger.info(f'Training time {total_time_str}')
    return best_vid_acc_1, best_vid_acc_5, best_epoch


def _lr_of(optimizer):
    return optimizer.param_groups[0]["lr"]


def train(model, optimizer, loader, epoch, writer=None, ds='hmdb51', log_every=50, augment=None):
    """finetune_video.py:277-350 -> (epoch, loss_avg, top1_avg, top5_avg).  The loss and correct counts of every step
    stay on the device; they are read back at the log lines and at the end of the epoch.  ``augment``: the training
    ClipAugmenter, for loaders that hand out uint8 frames."""
    model.train()
    batch_time, data_time = AverageMeter(), AverageMeter()
    losses, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter()
    pending = []                 # (loss [], correct [2], batch size) not yet read back

    def drain():
        if not pending:
            return
        vals = torch.stack([torch.cat([l.reshape(1), c]) for l, c, _ in pending]).cpu().numpy()
        for (_, _, n), (lv, c1, c5) in zip(pending, vals):
            losses.update(float(lv), n)
            top1.update(100.0 * float(c1) / n, n)
            top5.update(100.0 * float(c5) / n, n)
        pending.clear()

    one = None                   # d loss / d loss, made once: no fill launch inside the step
    end = time.perf_counter()
    for it, batch in enumerate(loader):
        data_time.update(time.perf_counter() - end)
        iteration = epoch * len(loader) + it
        video, target, _, _ = batch
        if augment is not None and augment.colorjitter and not is_frames(video):
            _note_colorjitter_without_frames()
        video, target = device_clips(video, augment), target.cuda(non_blocking=True)
        output, loss, correct = model(video, target)
        model.zero_grad(set_to_none=True)
        if one is None:
            one = torch.ones_like(loss)
        loss.backward(one)
        optimizer.step()
        pending.append((loss.detach(), correct, video.size(0)))
        batch_time.update(time.perf_counter() - end)
        end = time.perf_counter()
        if it % log_every == 0:
            drain()
            logger.info(
                "Epoch[{0}] - Iter: [{1}/{2}]\t"
                "Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t"
                "Data {data_time.val:.3f} ({data_time.avg:.3f})\t"
                "Loss {loss.val:.4f} ({loss.avg:.4f})\t"
                "Prec {top1.val:.3f} ({top1.avg:.3f})\t"
                "LR {lr}".format(epoch, it, len(loader), batch_time=batch_time, data_time=data_time, loss=losses,
                                 top1=top1, lr=_lr_of(optimizer)))
            if writer is not None:
                writer.add_scalar(f'{ds}/train/loss/iter', losses.val, iteration)
                writer.add_scalar(f'{ds}/train/clip_acc1/iter', top1.val, iteration)
    drain()
    return epoch, losses.avg, top1.avg, top5.avg


def evaluate(model, val_loader, epoch=0, writer=None, ds='hmdb51', augment=None, num_spatial_crops=3):
    """finetune_video.py:353-436 -> (loss_avg, vid_acc1, vid_acc5).  Logits, targets and video ids of the whole pass
    go into preallocated device buffers; the video-level accuracy is ops.segment_mean + the top-k kernel
    (utils.video_accuracy), read back once at the end of the pass.  ``augment``: the test ClipAugmenter, for loaders that
    hand out uint8 frames; the view of a clip is its spatial-temporal index (third item) % num_spatial_crops."""
    batch_time, losses, top1 = AverageMeter(), AverageMeter(), AverageMeter()
    model.eval()
    n = len(val_loader.dataset)
    K = model.classifier.weight.shape[0]
    dev = model.classifier.weight.device
    outs = torch.empty(n, K, dtype=torch.float32, device=dev)
    tgts = torch.empty(n, dtype=torch.int64, device=dev)
    vids = torch.empty(n, dtype=torch.int64, device=dev)
    stats = []                   # (loss [], correct [2], batch size) per batch
    row = 0
    with torch.no_grad():
        end = time.perf_counter()
        for batch_idx, batch in enumerate(val_loader):
            video, target, st_idx, video_idx = batch
            views = [int(i) % num_spatial_crops for i in st_idx] if is_frames(video) else None
            video = device_clips(video, augment, spatial_idx=views)
            target = target.cuda(non_blocking=True)
            b = video.size(0)
            output, loss, correct = model(video, target)
            outs[row:row + b].copy_(output)
            tgts[row:row + b].copy_(target)
            vids[row:row + b].copy_(video_idx, non_blocking=True)
            row += b
            stats.append((loss, correct, b))
            batch_time.update(time.perf_counter() - end)
            end = time.perf_counter()
    vals = torch.stack([torch.cat([l.reshape(1), c]) for l, c, _ in stats]).cpu().numpy()
    for (_, _, b), (lv, c1, _c5) in zip(stats, vals):
        losses.update(float(lv), b)
        top1.update(100.0 * float(c1) / b, b)
    video_acc1, video_acc5 = video_accuracy(outs[:row], tgts[:row], vids[:row], topk=(1, 5))
    video_acc1, video_acc5 = float(video_acc1.item()), float(video_acc5.item())
    logger.info("Test:\tTime {batch_time.avg:.3f}\tLoss {loss.avg:.4f}\tClipAcc@1 {top1.avg:.3f}\t"
                "VidAcc@1 {video_acc1:.3f}".format(batch_time=batch_time, loss=losses, top1=top1,
                                                   video_acc1=video_acc1))
    if writer is not None:
        writer.add_scalar(f'{ds}/val/vid_acc1/epoch', video_acc1, epoch)
        writer.add_scalar(f'{ds}/val/vid_acc5/epoch', video_acc5, epoch)
    return losses.avg, video_acc1, video_acc5


def parse_args(argv=None):
    """finetune_video.py:439-620: the reference's flags and defaults, plus ``synthetic`` as a dataset and the size of
    the synthetic sets (--synthetic_videos, --synthetic_crop); ``synthetic_uint8`` is the synthetic set handing out
    uint8 frames larger than the crop, so that the device clip augmentation runs; ``synthetic_video`` is the synthetic
    set handing out whole decoded videos, so that the device temporal sampling runs too."""
    def str2bool(v):
        v = v.lower()
        if v in ('yes', 'true', 't', '1'):
            return True
        elif v in ('no', 'false', 'f', '0'):
            return False
        raise ValueError('Boolean argument needs to be true or false. Instead, it is %s.' % v)

    import argparse
    parser = argparse.ArgumentParser(description='Finetuning')
    parser.register('type', 'bool', str2bool)
    add = parser.add_argument
    # DATA
    add('--dataset', default='ucf101', type=str,
        choices=['kinetics', 'vggsound', 'kinetics_sound', 'ave', 'ucf101', 'hmdb51', 'synthetic', 'synthetic_uint8',
                 'synthetic_video'])
    add('--root_dir', type=str, default='/path/to/dataset')
    add('--fold', default='1,2,3', type=str)
    add('--clip_len', default=32, type=int)
    add('--augtype', default=1, type=int)
    add('--colorjitter', default='True', type='bool')
    add('--steps_bet_clips', default=1, type=int)
    add('--num_data_samples', default=None, type=int)
    add('--train_clips_per_video', default=10, type=int)
    add('--val_clips_per_video', default=10, type=int)
    add('--num_spatial_crops', default=3, type=int)
    add('--test_time_cj', default='False', type='bool')
    add('--workers', default=0, type=int)
    add('--synthetic_videos', default=32, type=int, help='videos of the synthetic train set (test: half)')
    add('--synthetic_crop', default=0, type=int, help='frame size of the synthetic sets (0: the augtype crop)')
    # MODEL
    add('--weights_path', default='', type=str)
    add('--ckpt_epoch', default='0', type=str)
    add('--vid_base_arch', default='r2plus1d_18')
    add('--aud_base_arch', default='resnet9')
    add('--pretrained', default='False', type='bool')
    add('--use_mlp', default='True', type='bool')
    add('--mlptype', default=0, type=int)
    add('--headcount', default=10, type=int)
    add('--num_clusters', default=309, type=int)
    # FINETUNE
    add('--feature_extract', default='False', type='bool')
    add('--use_dropout', default='False', type='bool')
    add('--use_bn', default='False', type='bool')
    add('--use_l2_norm', default='False', type='bool')
    # TRAINING
    add('--batch_size', default=32, type=int)
    add('--epochs', default=12, type=int)
    add('--optim_name', default='sgd', type=str, choices=['sgd', 'adam'])
    add('--head_lr', default=0.0025, type=float)
    add('--base_lr', default=0.00025, type=float)
    add('--momentum', default=0.9, type=float)
    add('--weight_decay', default=0.005, type=float)
    add('--wd_base', default=5e-3, type=float)
    add('--use_scheduler', default='True', type='bool')
    add('--lr_warmup_epochs', default=2, type=int)
    add('--lr_milestones', default='6,10', type=str)
    add('--lr_gamma', default=0.05, type=float)
    # LOGGING
    add('--output_dir', default='.', type=str)
    # CHECKPOINTING
    add('--resume', default='', type=str)
    add('--start_epoch', default=0, type=int)
    add('--test_only', type='bool', default='False')
    return parser.parse_args(argv)


def run_folds(args, writer=None):
    """The reference's ``__main__`` (:623-650): main() once per --fold, then the fold averages."""
    args.dump_path = args.output_dir
    args.rank = 0
    logger.info(args)
    if args.output_dir:
        os.makedirs(args.output_dir, exist_ok=True)
    if args.clip_len > 32:
        args.num_sec = int(args.clip_len / 30)
    best_accs_1, best_accs_5, best_epochs = [], [], []
    folds = [int(fold) for fold in str(args.fold).split(',')]
    print(f"Evaluating on folds: {folds}")
    for fold in folds:
        args.fold = fold
        best_acc1, best_acc5, best_epoch = main(args, writer)
        best_accs_1.append(best_acc1)
        best_accs_5.append(best_acc5)
        best_epochs.append(best_epoch)
    avg_acc1, avg_acc5 = np.mean(best_accs_1), np.mean(best_accs_5)
    logger.info(f"{len(folds)}-Fold ({args.dataset}): ")
    logger.info(f"Vid Acc@1 {avg_acc1:.3f}, Video Acc@5 {avg_acc5:.3f}")
    return avg_acc1, avg_acc5, best_epochs


if __name__ == "__main__":
    run_folds(parse_args())
