"""kNN video retrieval (selavi_amd.retrieval_utils, csrc/retrieval.hip) against the executed reference
(tests/golden/retrieval.npz) and the float64 restatement of tests/_retrieval_ref.py (pinned by tests/test_retrieval_cpu.py)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _retrieval_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "retrieval.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _args(**kw):
    from selavi_amd import retrieval_utils as ru
    a = ru.parse_args([])
    a.__dict__.update(kw)
    return a


# ------------------------------------------------------------------ 1. pool kernels
@pytest.mark.parametrize("shape", [(2, 5, 7, 7, 7), (1, 3, 4, 6, 5), (3, 4, 2, 3, 2), (2, 512, 4, 7, 7)])
@pytest.mark.parametrize("op", ["max", "avg"])
def test_pool222_fp32_matches_torch(shape, op):
    from selavi_amd import ops
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    x = torch.randn(*shape, device="cuda", generator=g)
    x[0, 0, 0, 0, 0] = -0.0
    ref = (torch.nn.functional.max_pool3d if op == "max" else torch.nn.functional.avg_pool3d)(x, 2, 2).flatten(1)
    got = ops.pool222(x, op)
    if op == "max":
        assert torch.equal(got, ref)
    else:
        torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("N,T,H,W,C,Cp", [(2, 4, 7, 7, 512, 512), (3, 3, 5, 6, 20, 32), (1, 2, 2, 3, 45, 64)])
@pytest.mark.parametrize("op", ["max", "avg"])
def test_pool222_bf16_channels_last_matches_torch(N, T, H, W, C, Cp, op):
    from selavi_amd import ops
    g = torch.Generator(device="cuda").manual_seed(N * T + C)
    x = torch.randn(N, T, H, W, Cp, device="cuda", generator=g).to(torch.bfloat16)
    ncthw = x[..., :C].permute(0, 4, 1, 2, 3).float()
    ref = (torch.nn.functional.max_pool3d if op == "max" else torch.nn.functional.avg_pool3d)(ncthw, 2, 2).flatten(1)
    got = ops.pool222(x, op, channels=C)
    if op == "max":
        assert torch.equal(got, ref)
    else:
        torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-7)


def test_pool222_rejects_an_empty_pooled_extent():
    from selavi_amd import ops
    with pytest.raises(ValueError):
        ops.pool222(torch.zeros(2, 8, 1, 7, 7, device="cuda"), "max")       # an 8-frame clip at layer 4: T = 1
    with pytest.raises(ValueError):
        ops.pool222(torch.zeros(2, 1, 7, 1, 32, device="cuda", dtype=torch.bfloat16), "avg", channels=20)


# ------------------------------------------------------------------ 2. encoder features against the executed reference
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from selavi_amd.model import load_model
    path = str(tmp_path_factory.mktemp("ckpt") / "ckpt.pth")
    m = load_model(vid_base_arch='r2plus1d_18', aud_base_arch='resnet9', num_classes=309, norm_feat=False, use_mlp=True,
                   headcount=10)
    R.seeded_checkpoint(m, path)
    return path


# fp32: the bar of the full-model forward tests.  fp32_folded: the same three-piece exact operand split with BatchNorm
# folded into the weights (features ~1e-6 off the plain forward): the same bar.  bf16: bf16 weights and activations
# (8 significand bits) through 17 convs, fp32 accumulation: ~5e-3 of the feature scale measured on the pooled features of
# the SK pass (infer16.py); 3e-2 of the largest feature bounds it with margin.
@pytest.mark.parametrize("feature_pass,tol", [("fp32", 1e-3), ("fp32_folded", 1e-3), ("bf16", 3e-2)])
@pytest.mark.parametrize("pool", ["max", "avg"])
def test_encoder_features_match_reference(gold, ckpt, feature_pass, tol, pool):
    from selavi_amd import retrieval_utils as ru
    enc = ru.get_model(_args(weights_path=ckpt, pool_op=pool, feature_pass=feature_pass))
    got = enc(R.encoder_input().cuda()).cpu().numpy()
    ref = gold[f"enc_{pool}"]
    assert got.shape == ref.shape == (2, 512 * 1 * 3 * 3)
    assert np.abs(got - ref).max() <= tol * np.abs(ref).max()


# ------------------------------------------------------------------ 3. / 4. averaging and retrieval against the reference
def _synth(gold):
    seed = int(gold["seed"][0])
    return R.synth_clips(seed, 80), R.synth_clips(seed + 1000, 24)


@pytest.mark.parametrize("tag,norm", [("norm", True), ("raw", False)])
def test_average_features_matches_reference(gold, tag, norm):
    from selavi_amd import retrieval_utils as ru
    tr, va = _synth(gold)
    for part, (f, v, l) in (("train", tr), ("val", va)):
        src = (torch.from_numpy(f).cuda(), torch.from_numpy(v).cuda(), l) if part == "train" else (f, v, l)  # both input kinds
        avg, idx, lab = ru.average_features(_args(norm_feats=norm), *src)
        assert avg.is_cuda
        assert np.array_equal(np.array([int(i) for i in idx]), gold[f"{tag}_{part}_idx"])
        assert np.array_equal(lab, gold[f"{tag}_{part}_labels"])
        np.testing.assert_allclose(avg.cpu().numpy(), gold[f"{tag}_{part}_feats"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("tag", ["norm", "raw"])
def test_retrieval_matches_reference(gold, tag, capsys):
    from selavi_amd import retrieval_utils as ru
    g = lambda k: gold[f"{tag}_{k}"]
    capsys.readouterr()
    rd = ru.retrieval(torch.from_numpy(g("train_feats")).cuda(), g("train_labels"), list(g("train_idx")),
                      g("val_feats"), g("val_labels"), list(g("val_idx")))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "Recall @" in ln]
    assert lines == R.recall_lines("v-v", dict(zip(R.RECALL_AT, g("recall").tolist())))
    assert list(rd.keys()) == list(g("val_idx"))
    for i, v in enumerate(g("val_idx")):
        e = rd[v]
        assert e['label'] == g("val_labels")[i]
        assert [e['recal_acc'][str(k)] for k in R.RECALL_AT] == g("recal_acc")[i].tolist()
        for k in R.RECALL_AT:
            assert np.array_equal(e['neighbors'][str(k)], g("neighbors")[i, :k])


def test_retrieval_needs_fifty_train_videos():
    from selavi_amd import retrieval_utils as ru
    f = np.random.RandomState(0).randn(49, 8).astype(np.float32)
    with pytest.raises(ValueError):
        ru.retrieval(f, np.zeros(49), list(range(49)), f[:3], np.zeros(3), [0, 1, 2])


# ------------------------------------------------------------------ 5. knn
def _check_knn(q, t, d2, idx, k, gap=1e-5):
    """GPU (d2, idx) against float64 on the CPU: every returned d^2 is the float64 one of its index within `gap`, and a
    position may hold another index than the float64 ranking only where the two distances are within `gap`."""
    q64, t64 = q.double().cpu(), t.double().cpu()
    full = ((q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :] - 2.0 * q64 @ t64.T).clamp_min(0)
    ref_d2, ref_idx = torch.sort(full, dim=1, stable=True)
    ref_d2, ref_idx = ref_d2[:, :k], ref_idx[:, :k]
    idx = idx.long().cpu()
    at = torch.gather(full, 1, idx)
    assert (at - d2.double().cpu()).abs().max() <= gap
    assert (at - ref_d2).abs().max() <= gap
    swapped = idx != ref_idx
    assert bool(((at - ref_d2).abs() < gap)[swapped].all())
    assert all(len(set(r.tolist())) == k for r in idx)


def test_knn_at_the_ucf101_split1_shape():
    from selavi_amd import ops
    Q, N, D, k = 3783, 9537, 9216, 50
    g = torch.Generator(device="cuda").manual_seed(101)
    bank = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=1)
    queries = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=g), dim=1)
    queries[::7] = torch.nn.functional.normalize(bank[:Q:7] + 0.5 * queries[::7], dim=1)     # some with real neighbours
    d2, idx = ops.knn(queries, bank, k)
    sel = torch.linspace(0, Q - 1, 64).long()
    _check_knn(queries[sel], bank, d2[sel], idx[sel], k)


def test_knn_edge_cases():
    from selavi_amd import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    Q, N, D = 301, 777, 130                                    # no multiple of any tile
    bank = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=1)     # unit norm: d^2 <= 4
    bank[500] = bank[3]                                        # duplicate rows: the tie goes to the lower index
    bank[600] = bank[3]
    q = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=g), dim=1)
    q[5] = bank[3]
    d2, idx = ops.knn(q, bank, 64)
    _check_knn(q, bank, d2, idx, 64)
    assert idx[5, :3].tolist() == [3, 500, 600]
    assert d2[5, 0] == d2[5, 1] == d2[5, 2] and float(d2[5, 0]) <= 1e-5
    d2c, idxc = ops.knn(q, bank, 64, max_chunk_bytes=4 * N * 37)    # 9 chunks of <= 37 query rows
    assert torch.equal(d2c, d2) and torch.equal(idxc, idx)
    d1, i1 = ops.knn(q, bank, 1)
    assert torch.equal(i1[:, 0], idx[:, 0]) and torch.equal(d1[:, 0], d2[:, 0])
    with pytest.raises(ValueError):
        ops.knn(q, bank[:10], 11)
    with pytest.raises(ValueError):
        ops.knn(q, bank, 65)


def test_segment_mean_squared_norms():
    from selavi_amd import ops
    x = torch.randn(40, 33, device="cuda")
    vid = torch.tensor([3, 1, 3, 2] * 10, device="cuda")
    avg, ids, first, sq = ops.segment_mean(x, vid, normalize=False)
    assert ids.tolist() == [3, 1, 2] and first.tolist() == [0, 1, 3]
    torch.testing.assert_close(sq, (avg * avg).sum(1), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ 6. end to end
def test_video_retrieval_main_end_to_end(ckpt, tmp_path, capsys, monkeypatch):
    from selavi_amd import retrieval_utils as ru, video_retrieval
    from selavi_amd.data import SyntheticRetrievalDataset
    tr = SyntheticRetrievalDataset(n_videos=52, clips_per_video=2, T=16, S=112, n_classes=6, seed=3)
    te = SyntheticRetrievalDataset(n_videos=10, clips_per_video=2, T=16, S=112, n_classes=6, seed=4)
    args = _args(dataset="synthetic", weights_path=ckpt, clip_len=16, batch_size=16, train_clips_per_video=2,
                 save_pkl=True, output_dir=str(tmp_path))
    capsys.readouterr()
    rd = video_retrieval.main(args, dataset=tr, dataset_test=te)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "Recall @" in ln]
    assert len(lines) == 5
    # the restatement on the features the package extracted (the pickles it wrote)
    load = lambda m, n: ru.load_pickle(os.path.join(str(tmp_path), f"r2plus1d_18_synthetic_2_{m}_{n}.pkl"))
    f_tr, i_tr, l_tr = R.average(load("train", "feats"), load("train", "indices"), load("train", "labels"), True)
    f_va, i_va, l_va = R.average(load("test", "feats"), load("test", "indices"), load("test", "labels"), True)
    assert load("train", "feats").shape == (104, 4608) and load("train", "indices").dtype == np.int32
    _, idx = R.knn(f_va, f_tr, 50)
    means, acc = R.recall(l_tr, l_va, idx)
    assert list(rd.keys()) == [int(i) for i in i_va]
    d = np.sqrt(np.sort(R.sq_distances(f_va, f_tr), axis=1))
    for i, v in enumerate(i_va):
        if min(d[i, k] - d[i, k - 1] for k in R.RECALL_AT) < 1e-5:
            continue                                            # a near-tie at a cutoff: not decidable in fp32
        assert [rd[v]['recal_acc'][str(k)] for k in R.RECALL_AT] == acc[i].tolist()
        assert np.array_equal(rd[v]['neighbors']['5'], idx[i, :5])
    # from the cached features: no forward
    args.save_pkl, args.use_cache_feats = False, True

    def no_forward(self, video):
        raise AssertionError("forward with use_cache_feats")
    monkeypatch.setattr(ru.VideoRetrievalEncoder, "forward", no_forward)
    rd2 = video_retrieval.main(args, dataset=tr, dataset_test=te)
    assert [ln for ln in capsys.readouterr().out.splitlines() if "Recall @" in ln] == lines
    for v in rd:
        assert rd2[v]['recal_acc'] == rd[v]['recal_acc']
        assert all(np.array_equal(rd2[v]['neighbors'][k], rd[v]['neighbors'][k]) for k in rd[v]['neighbors'])


# ------------------------------------------------------------------ 7. load_model_parameters
def test_load_model_parameters_strips_module_prefix(capsys):
    from oracle.model_ref import portable_init_
    from selavi_amd import utils
    from selavi_amd.model import load_model
    a = portable_init_(load_model(use_mlp=True, num_classes=28, headcount=2), seed=5)
    R.fill_bn_stats_(a)
    b = load_model(use_mlp=True, num_classes=28, headcount=2)
    sd = {"module." + k: v for k, v in a.state_dict().items()}
    sd["module.not_a_parameter"] = torch.zeros(1)
    capsys.readouterr()
    utils.load_model_parameters(b, sd)
    assert re.search(r"didnt load\s+not_a_parameter", capsys.readouterr().out)
    sb = b.state_dict()
    for k, v in a.state_dict().items():
        assert torch.equal(sb[k], v), k
