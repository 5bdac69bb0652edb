"""Predictor.predict_topk_batches on the GPU (forward + topk.hip in one hipGraph per batch shape, input slot and top;
results through pinned buffers, the next replay enqueued before this batch is yielded) against ``predict_batches`` on
the same predictor, and ``batch_predict`` labelling through it against the ``HOPSX_INFER_TOPK=0`` path.

The model, images and batch are test_inference_gpu.py's, and the 1e-4 is that test's graph-vs-eager bound on the
probabilities: a score is within 1e-4 of the probability of its class, and that class' probability is no more than 2e-4
below the j-th largest of the row (two probabilities 1e-4 off each may swap places)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model_and_images():
    from hops_examples_amd.models.resnet import cifar_resnet
    from hops_examples_amd.runtime.arena import ParamArena

    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    m = cifar_resnet(20).to(dev).eval()
    ParamArena.from_module(m, dev)
    imgs = np.random.default_rng(1).integers(0, 256, (70, 32, 32, 3), dtype=np.uint8)
    return m, dev, imgs


def _batches(imgs, n=16):
    return (imgs[i:i + n] for i in range(0, len(imgs), n))


def _check_against_probs(ids, scores, p, top):
    assert ids.dtype == np.int32 and scores.dtype == np.float32 and ids.shape == scores.shape == (len(p), top)
    assert (scores[:, 1:] <= scores[:, :-1]).all()
    at = np.take_along_axis(p, ids.astype(np.int64), axis=1)
    assert np.abs(scores - at).max() <= 1e-4
    best = -np.sort(-p, axis=1)[:, :top]
    assert (at >= best - 2e-4).all()
    assert all(len(set(r)) == top for r in ids.tolist())


def test_topk_batches_agree_with_predict_batches_and_keep_its_accounting():
    from hops_examples_amd import inference as I

    m, dev, imgs = _model_and_images()
    pr = I.Predictor(m, dev, graph=True)
    p = np.concatenate(list(pr.predict_batches(_batches(imgs))))
    replays, graphs = pr.replays, len(pr._graphs)
    assert (replays, graphs) == (5, 3)
    pairs = list(pr.predict_topk_batches(_batches(imgs), top=3))
    assert [a.shape for a, _ in pairs] == [(16, 3)] * 4 + [(6, 3)]
    ids, scores = np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs])
    _check_against_probs(ids, scores, p, 3)
    assert pr.topk_replays == 5 and len(pr._topk_graphs) == 3
    assert pr.replays == replays and len(pr._graphs) == graphs  # predict_batches' own cache and count: untouched
    # graph=False: eager kernels, the same classes
    e_ids, e_scores = I.predict_topk(m, imgs, top=3, batch_size=16, graph=False)
    np.testing.assert_array_equal(e_ids, ids)
    assert np.abs(e_scores - scores).max() <= 1e-4
    # a single batch, and an empty iterator
    one = list(pr.predict_topk_batches([imgs[:16]], top=3))
    assert len(one) == 1
    np.testing.assert_array_equal(one[0][0], ids[:16])
    np.testing.assert_array_equal(one[0][1], scores[:16])
    assert list(pr.predict_topk_batches(iter(()), top=3)) == []
    assert pr.topk_replays == 6 and len(pr._topk_graphs) == 3
    # another top: graphs of its own; top = 1 is the argmax
    ids1, scores1 = (np.concatenate(x) for x in zip(*pr.predict_topk_batches(_batches(imgs), top=1)))
    _check_against_probs(ids1, scores1, p, 1)
    with pytest.raises(ValueError):
        list(pr.predict_topk_batches(_batches(imgs), top=0))
    with pytest.raises(ValueError):
        list(pr.predict_topk_batches(_batches(imgs), top=11))  # more than the 10 classes (and than 8)


def test_replays_see_a_changed_classifier_bias():
    from hops_examples_amd import inference as I

    m, dev, imgs = _model_and_images()
    pr = I.Predictor(m, dev, graph=True)
    ids, _ = (np.concatenate(x) for x in zip(*pr.predict_topk_batches(_batches(imgs[:32]), top=3)))
    bias = [q for n, q in m.named_parameters() if n.endswith("bias") and q.numel() == 10][-1]
    loser = int(np.bincount(ids[:, 0], minlength=10).argmin())
    with torch.no_grad():
        bias[loser] += 100.0  # in place: the captured graphs read the live classifier parameters
    ids2, scores2 = (np.concatenate(x) for x in zip(*pr.predict_topk_batches(_batches(imgs[:32]), top=3)))
    assert pr.topk_replays == 4 and len(pr._topk_graphs) == 2  # replayed, not recaptured
    assert (ids2[:, 0] == loser).all() and (scores2[:, 0] > 0.99).all()


def test_batch_predict_labels_through_topk(project_root, monkeypatch):
    from PIL import Image

    from hops_examples_amd import inference as I

    d = project_root / "images"
    d.mkdir(parents=True)
    rng = np.random.default_rng(0)
    paths = []
    for i in range(7):
        p = d / f"img_{i}.png"
        Image.fromarray(rng.integers(0, 255, (40, 48, 3), dtype=np.uint8)).save(p)
        paths.append(str(p))

    def builder():  # (a local function travels to the worker process by value; seeded: both runs get the same weights)
        import torch

        from hops_examples_amd.models.resnet import cifar_resnet

        torch.manual_seed(0)
        return cifar_resnet(8, num_classes=5)

    monkeypatch.setenv("HOPSX_INFER_TOPK", "1")
    new = I.batch_predict(builder, paths, "Resources/labels_topk.parquet", batch_size=3, num_workers=1)
    monkeypatch.setenv("HOPSX_INFER_TOPK", "0")
    old = I.batch_predict(builder, paths, "Resources/labels_probs.parquet", batch_size=3, num_workers=1)
    assert list(new.columns) == list(old.columns) and len(new) == len(old) == 7
    assert [str(t) for t in new.dtypes] == [str(t) for t in old.dtypes]
    new, old = new.sort_values("image_path").reset_index(drop=True), old.sort_values("image_path").reset_index(drop=True)
    assert list(new.image_path) == list(old.image_path) == sorted(paths)
    assert list(new.top1_id) == list(old.top1_id) and list(new.top1_label) == list(old.top1_label)
    for j in (1, 2, 3):
        assert np.abs(new[f"top{j}_score"].to_numpy() - old[f"top{j}_score"].to_numpy()).max() <= 1e-4
    assert (new.top1_score >= new.top2_score).all() and (new.top2_score >= new.top3_score).all()
    # that the HOPSX_INFER_TOPK=1 run went through predict_topk_batches, not twice through the old path: the worker,
    # in this process on the GPU, with predict_batches made unusable, writes the same table (with label names)
    import pandas as pd

    def unusable(self, batches):
        raise AssertionError("predict_batches called on the top-k labelling path")

    monkeypatch.setattr(I.Predictor, "predict_batches", unusable)
    monkeypatch.setenv("HOPSX_INFER_TOPK", "1")
    out = project_root / "inproc.parquet"
    assert I._shard_worker(builder, None, sorted(paths), 3, 3, list("abcde"), str(out), 2) == 7
    mine = pd.read_parquet(out)
    assert list(mine.columns) == list(old.columns) and list(mine.image_path) == list(old.image_path)
    assert list(mine.top1_id) == list(old.top1_id)
    assert list(mine.top1_label) == ["abcde"[int(i[1:])] for i in old.top1_id]
    for j in (1, 2, 3):
        assert np.abs(mine[f"top{j}_score"].to_numpy() - old[f"top{j}_score"].to_numpy()).max() <= 1e-4
