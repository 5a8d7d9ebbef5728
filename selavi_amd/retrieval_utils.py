"""kNN video retrieval (mirror of /root/reference/src/retrieval_utils.py): Recall@{1,5,10,20,50} of test videos against
train videos, on features of the video trunk's layer 4 pooled 2x2x2 and flattened.

Same names, arguments and return structures as the reference.  What differs is where the work runs: the encoder is the
engine's eval forward with a pooled layer-4 tap (engine.video_stage_forward(layer4_pool=)), the per-video averaging is
slv_segment_mean, and the neighbour search is slv_gemm_nt + slv_knn_select (ops.knn) instead of sklearn on the host.
Features stay on the device between the steps: get_features returns device tensors, and average_features / retrieval
take numpy arrays or tensors.  save_pkl / use_cache_feats write and read the reference's pickle names and formats
(numpy arrays), so feature dumps move between the two implementations.
"""
import os
import pickle
import time

import numpy as np
import torch

from . import engine, ops
from . import nn as snn
from . import utils
from .data import SyntheticRetrievalDataset
from .model import load_model

RECALL_AT = (1, 5, 10, 20, 50)
FEATURE_PASSES = ("fp32", "fp32_folded", "fp32x2", "bf16")


def save_pickle(obj, name):
    with open(name, 'wb') as handle:
        print("Dumping data as pkl file", flush=True)
        pickle.dump(obj, handle, protocol=pickle.HIGHEST_PROTOCOL)


def load_pickle(pkl_path):
    if not os.path.exists(pkl_path):
        raise FileNotFoundError(pkl_path)
    print(f"Loading pickle file: {pkl_path}", flush=True)
    with open(pkl_path, 'rb') as handle:
        return pickle.load(handle)


def _feature_pass(args_value=None):
    """args.feature_pass / SELAVI_FEATURE_PASS as in sk_utils.cluster: "fp32" (default, the model's own eval arithmetic),
    "fp32_folded" / "fp32x2" (BatchNorm folded into the weights, three / two operand pieces), "bf16" (infer16)."""
    mode = args_value or os.environ.get("SELAVI_FEATURE_PASS", "fp32")
    if mode not in FEATURE_PASSES:
        raise ValueError(f"feature_pass {mode!r}: fp32 | fp32_folded | fp32x2 | bf16")
    return mode


class VideoRetrievalEncoder(torch.nn.Module):
    """What the reference's get_model builds for retrieval: Sequential(stem, layer1..4, {Max,Avg}Pool3d(2, 2), Flatten())
    of the video trunk, in eval mode.  forward(video [B,3,T,H,W]) -> fp32 [B, 512*(T/8)*(H/32)*(W/32)] (floor halvings)."""

    def __init__(self, model, pool_op='max', feature_pass=None):
        super().__init__()
        if pool_op not in ('max', 'avg'):
            raise ValueError("Only 'max' and 'avg' pool operations allowed")
        self.model = model.module if hasattr(model, "module") else model
        self.model.eval()
        self.pool_op = pool_op
        self.feature_pass = _feature_pass(feature_pass)
        self._folded = self._engine16 = None

    def begin_pass(self):
        """Re-derive folded / bf16 weights from the weights as they are now (get_features calls it once per pass)."""
        self._folded = self._engine16 = None

    @torch.no_grad()
    def forward(self, video):
        base = self.model.video_network.base
        x = video.contiguous()
        if self.feature_pass == "bf16":
            if self._engine16 is None:
                from . import infer16
                self._engine16 = infer16.Engine(self.model)
            return self._engine16.video_features(x, layer4_pool=self.pool_op)
        ectx = engine.Ctx(False, ops=snn._backend(base))
        if self.feature_pass in ("fp32_folded", "fp32x2") and ectx.ops is ops:
            if self._folded is None:
                from . import infer32
                self._folded = infer32.FoldedEval(pieces=3 if self.feature_pass == "fp32_folded" else 2)
            ectx.folded = self._folded
            feat, _ = engine.video_forward(ectx, base, x, layer4_pool=self.pool_op)
            return feat
        ectx.wimg = snn._weight_images(base, x, False, first=True)       # as the model's own eval forward does
        feat, _ = engine.video_forward(ectx, base, x, layer4_pool=self.pool_op)
        snn._weight_images(base, x, False, first=False, last_done=True)
        return feat


def get_model(args, get_video_encoder_only=True, logger=None):
    model = load_model(
        vid_base_arch=args.vid_base_arch,
        aud_base_arch=args.aud_base_arch,
        pretrained=args.pretrained,
        num_classes=args.num_clusters,
        norm_feat=False,
        use_mlp=args.use_mlp,
        headcount=args.headcount,
    )
    start = time.time()
    wp = args.weights_path
    if (wp != 'None' and wp != '') if isinstance(wp, str) else wp is not None:
        print("Loading model weights")
        if os.path.exists(wp):
            ckpt_dict = torch.load(wp, map_location="cpu")
            args.ckpt_epoch = ckpt_dict.get('epoch')
            print(f"Epoch checkpoint: {args.ckpt_epoch}", flush=True)
            utils.load_model_parameters(model, ckpt_dict["model"])
    print(f"Time to load model weights: {time.time() - start}")
    model.eval()
    model = model.cuda()
    if get_video_encoder_only:
        return VideoRetrievalEncoder(model, args.pool_op, getattr(args, "feature_pass", None))
    return model


def _datasets(args):
    if args.dataset != 'synthetic':
        raise NotImplementedError(
            f"dataset {args.dataset!r}: video decoding of the real datasets is out of scope of this build (SURVEY.md 2); "
            "pass dataset objects returning (video, label, clip_idx, vid_idx), or use --dataset synthetic")
    kw = dict(clips_per_video=args.train_clips_per_video, T=args.clip_len, S=112, n_classes=args.synthetic_classes)
    return (SyntheticRetrievalDataset(args.synthetic_videos, seed=args.synthetic_seed, **kw),
            SyntheticRetrievalDataset(args.synthetic_test_videos, seed=args.synthetic_seed + 1, **kw))


def init(args, get_video_encoder_only=True, logger=None, dataset=None, dataset_test=None):
    """-> (model, dataset, dataset_test).  Dataset objects passed in are used as they are."""
    if dataset is None or dataset_test is None:
        print("Loading training data")
        print("Loading validation data")
        made, made_test = _datasets(args)
        dataset = made if dataset is None else dataset
        dataset_test = made_test if dataset_test is None else dataset_test
    model = get_model(args, get_video_encoder_only=get_video_encoder_only, logger=logger)
    return model, dataset, dataset_test


def _pretext(args, mode, pretext):
    return pretext if pretext is not None else f"{args.vid_base_arch}_{args.dataset}_{args.train_clips_per_video}_{mode}"


def get_features(args, dataset, model, get_audio=False, logger=None, mode='train', print_freq=250, pretext=None):
    """-> (features fp32 [R, D], video indices int32 [R], labels int32 [R]), all on the device."""
    if get_audio:
        raise NotImplementedError("audio-feature extraction is out of scope of this build; retrieval() takes audio arrays")
    N = len(dataset)
    print(f"Size of DS: {N}")
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, num_workers=args.workers,
                                             pin_memory=True, drop_last=False)
    print(f"Size of Dataloader: {len(dataloader)}")
    dev = torch.device("cuda")
    if hasattr(model, "begin_pass"):
        model.begin_pass()
    feats, indices, labels = [], [], []
    with torch.no_grad():
        for batch_idx, batch in enumerate(dataloader):
            video, label, _, video_idx = batch
            feats.append(model(video.to(dev, non_blocking=True)))
            indices.append(video_idx.to(dev, non_blocking=True).to(torch.int32))
            labels.append(label.to(dev, non_blocking=True).to(torch.int32))
            if batch_idx % print_freq == 0:
                print(f'{batch_idx} / {len(dataloader)}', end='\r')
        print("Done collecting features")
    PS_v, indices, labels = torch.cat(feats), torch.cat(indices), torch.cat(labels)
    if args.save_pkl:
        pretext = _pretext(args, mode, pretext)
        os.makedirs(args.output_dir, exist_ok=True)
        save_pickle(PS_v.cpu().numpy(), os.path.join(args.output_dir, f"{pretext}_feats.pkl"))
        save_pickle(indices.cpu().numpy(), os.path.join(args.output_dir, f"{pretext}_indices.pkl"))
        save_pickle(labels.cpu().numpy(), os.path.join(args.output_dir, f"{pretext}_labels.pkl"))
    return PS_v, indices, labels


def load_or_get_features(args, dataset, model, get_audio=False, logger=None, mode='train', pretext=None):
    """The pickles of an earlier get_features (numpy arrays) when args.use_cache_feats and they load; else get_features."""
    pretext = _pretext(args, mode, pretext)
    if args.use_cache_feats:
        try:
            names = ["feats", "indices", "labels"] + (["feats_aud"] if get_audio else [])
            got = {n: load_pickle(os.path.join(args.output_dir, f"{pretext}_{n}.pkl")) for n in names}
            if get_audio:
                return got["feats"], got["feats_aud"], got["indices"], got["labels"]
            return got["feats"], got["indices"], got["labels"]
        except Exception:
            pass
    return get_features(args, dataset, model, get_audio=get_audio, logger=logger, mode=mode)


def _numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _device_f32(a, device=None):
    dev = device if device is not None else (a.device if isinstance(a, torch.Tensor) and a.is_cuda else torch.device("cuda"))
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=torch.float32).contiguous()


def average_features(args, features, vid_indices, labels, get_audio=False, aud_features=None, logger=None):
    """Mean feature per video (each clip L2-normalised first when args.norm_feats), videos in the order of their first clip.
    -> (features [V, D] on the device, list of V video indices, labels [V] numpy): the reference's structure."""
    feats = _device_f32(features)
    print(f"Total Number of features: {len(feats)}")
    vid_np = _numpy(vid_indices)
    avg, _, first, _ = ops.segment_mean(feats, torch.from_numpy(vid_np.astype(np.int64)).to(feats.device),
                                        normalize=args.norm_feats)
    first = first.cpu().numpy()
    avg_vid_indices = list(vid_np[first])
    avg_labels = _numpy(labels)[first]
    if get_audio and aud_features is not None:
        avg_a, _, _, _ = ops.segment_mean(_device_f32(aud_features, feats.device),
                                          torch.from_numpy(vid_np.astype(np.int64)).to(feats.device), normalize=args.norm_feats)
        return avg, avg_a, avg_vid_indices, avg_labels
    return avg, avg_vid_indices, avg_labels


def retrieval(train_features, train_labels, train_vid_indices, val_features, val_labels, val_vid_indices,
              train_aud_features=None, val_aud_features=None, task='v-v'):
    """Recall@{1,5,10,20,50} of every val video against the train bank (Euclidean, brute force).  Prints one line per
    threshold and returns {val video index: {'label', 'recal_acc': {k: share of the distinct neighbour labels that are the
    query's}, 'neighbors': {k: row positions in the train bank, nearest first}}}."""
    assert task in ['v-a', 'a-v', 'v-v', 'a-a']
    if task in ['v-a', 'a-v', 'a-a']:
        assert train_aud_features is not None
        assert val_aud_features is not None
    feat_val = val_aud_features if task in ('a-v', 'a-a') else val_features
    feat_train = train_aud_features if task in ('v-a', 'a-a') else train_features
    bank = _device_f32(feat_train)
    queries = _device_f32(feat_val, bank.device)
    kmax = max(RECALL_AT)
    if bank.shape[0] < kmax:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {kmax}, n_samples_fit = {bank.shape[0]}")
    _, idx = ops.knn(queries, bank, kmax)
    idx = idx.cpu().numpy().astype(np.int64)
    train_labels = _numpy(train_labels)
    val_labels = _numpy(val_labels)
    if isinstance(val_vid_indices, torch.Tensor):
        val_vid_indices = val_vid_indices.cpu().tolist()
    recall = {k: [] for k in RECALL_AT}
    retrieval_dict = {}
    for i in range(len(queries)):
        vid_idx, vid_label = val_vid_indices[i], val_labels[i]
        entry = retrieval_dict[vid_idx] = {'label': vid_label, 'recal_acc': {}, 'neighbors': {}}
        for k in RECALL_AT:
            neighbor_indices = idx[i, :k].copy()
            neighbor_labels = set(train_labels[neighbor_indices].tolist())
            recall[k].append(100 if vid_label in neighbor_labels else 0)
            entry['recal_acc'][str(k)] = (1 if vid_label in neighbor_labels else 0) / float(len(neighbor_labels))
            entry['neighbors'][str(k)] = neighbor_indices
    for k in RECALL_AT:
        print(f"{task}: Recall @ {k}: {np.mean(recall[k])}")
    return retrieval_dict


def parse_args(argv=None):
    def str2bool(v):
        v = v.lower()
        if v in ('yes', 'true', 't', '1'):
            return True
        elif v in ('no', 'false', 'f', '0'):
            return False
        raise ValueError(f'Boolean argument needs to be true or false. Instead, it is {v}.')

    import argparse
    parser = argparse.ArgumentParser(description='Video Retrieval')
    parser.register('type', 'bool', str2bool)
    # retrieval
    parser.add_argument('--use_cache_feats', default='False', type='bool', help='use cache features')
    parser.add_argument('--save_pkl', default='False', type='bool', help='save pickled feats')
    parser.add_argument('--avg_feats', default='True', type='bool', help='Average features of video')
    parser.add_argument('--norm_feats', default='True', type='bool', help='L2 normalize features of video')
    parser.add_argument('--pool_op', default='max', type=str, choices=['max', 'avg'],
                        help='Type of pooling operation: [max, avg]')
    parser.add_argument('--get_audio', default='False', type='bool', help='Get audio features')
    parser.add_argument('--feature_pass', default=None, choices=list(FEATURE_PASSES),
                        help='arithmetic of the feature pass (default: SELAVI_FEATURE_PASS, else fp32)')
    # dataset
    parser.add_argument('--dataset', default='hmdb51', type=str,
                        choices=['kinetics', 'vggsound', 'kinetics_sound', 'ave', 'ucf101', 'hmdb51', 'synthetic'],
                        help='name of dataset (synthetic: data.SyntheticRetrievalDataset; the others need dataset objects)')
    parser.add_argument("--root_dir", type=str, default="/path/to/dataset", help="root dir of dataset")
    parser.add_argument('--batch_size', default=96, type=int, help='Size of batch')
    parser.add_argument('--fold', default='1', type=str, help='name of dataset')
    parser.add_argument('--clip_len', default=32, type=int, help='number of frames per clip')
    parser.add_argument('--augtype', default=1, type=int, help='augmentation type (default: 1)')
    parser.add_argument('--steps_bet_clips', default=1, type=int, help='number of steps between clips in video')
    parser.add_argument('--train_clips_per_video', default=10, type=int,
                        help='maximum number of clips per video for training')
    parser.add_argument('--val_clips_per_video', default=10, type=int, help='maximum number of clips per video for testing')
    parser.add_argument('--workers', default=0, type=int, help='number of data loading workers')
    parser.add_argument('--synthetic_videos', default=64, type=int, help='synthetic: train videos')
    parser.add_argument('--synthetic_test_videos', default=16, type=int, help='synthetic: test videos')
    parser.add_argument('--synthetic_classes', default=8, type=int, help='synthetic: classes')
    parser.add_argument('--synthetic_seed', default=31, type=int, help='synthetic: seed')
    # model
    parser.add_argument('--weights_path', default='', type=str, help='Path to weights file')
    parser.add_argument('--vid_base_arch', default='r2plus1d_18', type=str, help='Video Base Arch for A-V model')
    parser.add_argument('--aud_base_arch', default='resnet9', help='Audio Base Arch for A-V model')
    parser.add_argument('--pretrained', type='bool', default='False', help="Use pre-trained models from the modelzoo")
    parser.add_argument('--use_mlp', default='True', type='bool', help='Use MLP projection head')
    parser.add_argument('--headcount', default=10, type=int, help='how many heads each modality has')
    parser.add_argument('--num_clusters', default=309, type=int, help="number of clusters")
    parser.add_argument('--output_dir', default='./retrieval_results', help='path where to save')
    return parser.parse_args(argv)
