"""softmax + top-k on the host: ``softmax_topk_reference`` (the statement the topk.hip tests compare against) — its
tie rule on hand-made rows, agreement with ``torch.topk`` where the selected values are distinct, scores equal to
the fp64 softmax's entries, -inf classes at 0; ``decode_topk`` against ``decode_predictions``; ``predict_topk`` on
the CPU against ``predict``'s probabilities; ``batch_predict``'s worker labelling through ``predict_topk_batches``
(``HOPSX_INFER_TOPK=1``) with ``predict_batches`` made unusable, and its column-wise table against the row-wise one."""
import numpy as np
import pytest
import torch


def _ref(z, k, dtype=torch.float64):
    from hops_examples_amd.ops.functional import softmax_topk_reference

    return softmax_topk_reference(z, k, dtype=dtype)


def test_tie_rule_on_hand_made_rows():
    z = torch.tensor([[2.0] * 6,                           # all equal: classes in order
                      [5.0, 4.0, 3.0, 2.0, 1.0, 0.0],      # descending
                      [0.0, 1.0, 2.0, 3.0, 4.0, 5.0],      # ascending
                      [1.0, 7.0, 3.0, 3.0, 3.0, 0.0],      # a plateau of three straddling the 3rd place
                      [0.0, -0.0, -1.0, 0.0, -0.0, -2.0]])  # -0.0 == 0.0: still by class
    ids, scores = _ref(z, 3)
    assert ids.dtype == torch.int32 and scores.dtype == torch.float64
    assert ids.tolist() == [[0, 1, 2], [0, 1, 2], [5, 4, 3], [1, 2, 3], [0, 1, 3]]
    ids6, _ = _ref(z, 6)
    assert ids6[3].tolist() == [1, 2, 3, 4, 0, 5] and ids6[0].tolist() == list(range(6))
    # the same rows as bf16 (exact there) select the same classes
    assert _ref(z.to(torch.bfloat16), 3)[0].tolist() == ids.tolist()
    with pytest.raises(ValueError):
        _ref(z, 7)
    with pytest.raises(ValueError):
        _ref(z, 0)


def test_ids_match_torch_topk_where_values_are_distinct_and_scores_are_the_softmax_entries():
    g = torch.Generator().manual_seed(3)
    for B, C, k, std in ((4, 10, 1, 1.0), (7, 65, 8, 4.0), (5, 1000, 3, 16.0)):
        z = torch.randn(B, C, generator=g) * std
        ids, scores = _ref(z, k)
        tv, ti = torch.topk(z, k, dim=-1)
        distinct = (tv[:, 1:] != tv[:, :-1]).all() if k > 1 else True
        assert distinct  # (continuous draws: the comparison below is then well defined)
        assert torch.equal(ids.long(), ti)
        p = torch.softmax(z.double(), dim=-1)
        assert torch.equal(scores, p.gather(1, ids.long()))
        assert (scores[:, 1:] <= scores[:, :-1]).all()
        # the fp32 yardstick: same ids, scores from an fp32 softmax
        ids32, s32 = _ref(z, k, dtype=torch.float32)
        assert torch.equal(ids32, ids) and s32.dtype == torch.float32
        assert torch.equal(s32, torch.softmax(z, dim=-1).gather(1, ids.long()))


def test_minus_inf_classes_score_zero():
    z = torch.tensor([[0.5, float("-inf"), 1.5, float("-inf")], [float("-inf"), float("-inf"), float("-inf"), 2.0]])
    ids, scores = _ref(z, 4)
    assert ids.tolist() == [[2, 0, 1, 3], [3, 0, 1, 2]]
    assert scores[0, 2:].tolist() == [0.0, 0.0] and scores[1].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert abs(float(scores[0, :2].sum()) - 1.0) < 1e-15


def test_decode_topk_equals_decode_predictions():
    from hops_examples_amd import inference as I

    p = np.random.default_rng(0).dirichlet(np.ones(12), size=9)  # probability rows, no ties
    ids = np.argsort(-p, axis=1)[:, :3].astype(np.int32)
    scores = np.take_along_axis(p, ids.astype(np.int64), axis=1)
    labels = [f"name_{i}" for i in range(12)]
    assert I.decode_topk(ids, scores) == I.decode_predictions(p, top=3)
    assert I.decode_topk(ids, scores, labels) == I.decode_predictions(p, top=3, labels=labels)
    assert I.decode_topk(np.empty((0, 3), np.int32), np.empty((0, 3), np.float32)) == []


def test_predict_topk_cpu_agrees_with_predict():
    from hops_examples_amd import inference as I
    from hops_examples_amd.models.resnet import cifar_resnet

    torch.manual_seed(0)
    m = cifar_resnet(8, num_classes=5)
    imgs = np.random.default_rng(1).integers(0, 256, (11, 32, 32, 3), dtype=np.uint8)
    p = I.predict(m, imgs, batch_size=4, device="cpu")
    ids, scores = I.predict_topk(m, imgs, top=3, batch_size=4, device="cpu")
    assert ids.shape == (11, 3) and ids.dtype == np.int32 and scores.shape == (11, 3) and scores.dtype == np.float32
    np.testing.assert_array_equal(ids, np.argsort(-p, axis=1, kind="stable")[:, :3])
    np.testing.assert_array_equal(scores, np.take_along_axis(p, ids.astype(np.int64), axis=1))
    assert (scores[:, 1:] <= scores[:, :-1]).all()
    pr = I.Predictor(m, "cpu")
    pairs = list(pr.predict_topk_batches((imgs[i:i + 4] for i in range(0, 11, 4)), top=5))
    assert [a.shape for a, _ in pairs] == [(4, 5), (4, 5), (3, 5)] and pr.topk_replays == 0
    assert list(pr.predict_topk_batches(iter(()), top=3)) == []
    e_ids, e_scores = I.predict_topk(m, imgs[:0], top=3, device="cpu")
    assert e_ids.shape == (0, 3) and e_scores.shape == (0, 3)
    with pytest.raises(ValueError):
        I.predict_topk(m, imgs, top=3, device="cpu", frozen=True)
    with pytest.raises(ValueError):
        I.predict_topk(m, imgs, top=9, device="cpu")
    with pytest.raises(ValueError):
        I.predict_topk(m, imgs, top=6, device="cpu")  # more than the 5 classes


def _rowwise_frame(paths, probs, top, labels):
    """The table as the worker builds it from probabilities: one dict per image out of decode_predictions."""
    import pandas as pd

    from hops_examples_amd import inference as I

    rows = []
    for p, dec in zip(paths, I.decode_predictions(probs, top, labels)):
        r = {"image_path": str(p)}
        for k, (cid, lab, sc) in enumerate(dec, 1):
            r[f"top{k}_id"], r[f"top{k}_label"], r[f"top{k}_score"] = cid, lab, sc
        rows.append(r)
    return pd.DataFrame(rows)


@pytest.mark.parametrize("labels", [None, [f"name_{i}" for i in range(12)]], ids=["class_i", "labels"])
def test_label_frame_equals_the_row_wise_table(labels):
    from hops_examples_amd import inference as I

    p = np.random.default_rng(4).dirichlet(np.ones(12), size=9).astype(np.float32)
    paths = [f"/data/img_{i}.png" for i in range(9)]
    ids = np.argsort(-p, axis=1, kind="stable")[:, :3].astype(np.int32)
    scores = np.take_along_axis(p, ids.astype(np.int64), axis=1)
    got, want = I._label_frame(paths, ids, scores, labels), _rowwise_frame(paths, p, 3, labels)
    assert list(got.columns) == list(want.columns) and [str(t) for t in got.dtypes] == [str(t) for t in want.dtypes]
    assert got.equals(want)
    if labels:
        assert list(got.top1_label) == [labels[i] for i in ids[:, 0]]


def _png_paths(d, n=7):
    from PIL import Image

    rng = np.random.default_rng(0)
    paths = []
    for i in range(n):
        p = d / f"img_{i}.png"
        Image.fromarray(rng.integers(0, 255, (40, 48, 3), dtype=np.uint8)).save(p)
        paths.append(str(p))
    return paths


def _seeded_tiny_resnet():
    from hops_examples_amd.models.resnet import cifar_resnet

    torch.manual_seed(0)
    return cifar_resnet(8, num_classes=5)


@pytest.mark.parametrize("top,labels", [(3, None), (3, list("abcde")), (6, None)], ids=["top3", "top3-labels", "top6-of-5"])
def test_shard_worker_labels_through_topk_without_predict_batches(tmp_path, monkeypatch, top, labels):
    """With HOPSX_INFER_TOPK=1 the worker must not touch predict_batches (made to raise here), and writes the table
    the HOPSX_INFER_TOPK=0 worker writes: same columns and dtypes, same classes, scores within the 1e-4 of
    test_inference_gpu.py's graph-vs-eager bound.  top = 6 on a 5-class model: five column groups on both paths."""
    import pandas as pd

    from hops_examples_amd import inference as I

    paths = _png_paths(tmp_path)
    (tmp_path / "broken.png").write_bytes(b"not an image")
    paths.insert(2, str(tmp_path / "broken.png"))
    monkeypatch.setenv("HOPSX_INFER_TOPK", "0")
    n_old = I._shard_worker(_seeded_tiny_resnet, None, paths, 3, top, labels, str(tmp_path / "old.parquet"), 2)

    def unusable(self, batches):
        raise AssertionError("predict_batches called on the top-k labelling path")

    monkeypatch.setattr(I.Predictor, "predict_batches", unusable)
    monkeypatch.setenv("HOPSX_INFER_TOPK", "1")
    n_new = I._shard_worker(_seeded_tiny_resnet, None, paths, 3, top, labels, str(tmp_path / "new.parquet"), 2)
    old, new = pd.read_parquet(tmp_path / "old.parquet"), pd.read_parquet(tmp_path / "new.parquet")
    groups = min(top, 5)
    assert n_old == n_new == 7 and len(new.columns) == 1 + 3 * groups
    assert list(new.columns) == list(old.columns) and [str(t) for t in new.dtypes] == [str(t) for t in old.dtypes]
    assert list(new.image_path) == list(old.image_path) == [p for p in paths if "broken" not in p]
    for j in range(1, groups + 1):
        assert list(new[f"top{j}_id"]) == list(old[f"top{j}_id"])
        assert list(new[f"top{j}_label"]) == list(old[f"top{j}_label"])
        assert np.abs(new[f"top{j}_score"].to_numpy() - old[f"top{j}_score"].to_numpy()).max() <= 1e-4
    if labels:
        assert set(new.top1_label) <= set(labels)
    # (the public generator keeps refusing top > classes unless asked to clamp)
    pr = I.Predictor(_seeded_tiny_resnet(), "cpu")
    x = np.zeros((2, 32, 32, 3), np.uint8)
    assert [a.shape for a, _ in pr.predict_topk_batches([x], top=6, clamp=True)] == [(2, 5)]
