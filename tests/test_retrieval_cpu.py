"""The float64 restatement of the retrieval evaluation (tests/_retrieval_ref.py) against what the executed reference
produced (tests/golden/retrieval.npz, tests/golden/make_retrieval_golden.py): the GPU tests judge the package by it."""
import os

import numpy as np
import pytest

from tests import _retrieval_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "retrieval.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _inputs(gold):
    seed = int(gold["seed"][0])
    return R.synth_clips(seed, 80), R.synth_clips(seed + 1000, 24)


@pytest.mark.parametrize("tag,norm", [("norm", True), ("raw", False)])
def test_restated_average_matches_reference(gold, tag, norm):
    tr, va = _inputs(gold)
    for part, clips in (("train", tr), ("val", va)):
        f, idx, lab = R.average(*clips, norm)
        assert np.array_equal(idx, gold[f"{tag}_{part}_idx"])
        assert np.array_equal(lab, gold[f"{tag}_{part}_labels"])
        np.testing.assert_allclose(f, gold[f"{tag}_{part}_feats"], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("tag,norm", [("norm", True), ("raw", False)])
def test_restated_knn_and_recall_match_reference(gold, tag, norm):
    tr, va = _inputs(gold)
    f_tr, _, l_tr = R.average(*tr, norm)
    f_va, _, l_va = R.average(*va, norm)
    _, idx = R.knn(f_va, f_tr, 50)
    assert np.array_equal(idx, gold[f"{tag}_neighbors"])
    means, acc = R.recall(l_tr, l_va, idx)
    assert [means[k] for k in R.RECALL_AT] == gold[f"{tag}_recall"].tolist()
    assert np.array_equal(acc, gold[f"{tag}_recal_acc"])


def test_restated_knn_breaks_ties_to_the_lower_index():
    bank = np.array([[1.0, 0.0], [0.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    d2, idx = R.knn(np.zeros((1, 2)), bank, 4)
    assert idx.tolist() == [[1, 3, 0, 2]] and d2.tolist() == [[0.0, 0.0, 1.0, 1.0]]
