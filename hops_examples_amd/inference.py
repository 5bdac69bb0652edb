"""Image inference: single-image prediction and sharded multi-GPU batch inference.

Reference: notebooks/ml/Inference/Inference_Hello_World.ipynb (ResNet50 -> save to the project ->
reload -> ``load_img(target_size=(224, 224))`` -> ``preprocess_input`` -> ``predict`` ->
``decode_predictions(top=3)``) and Batch_Inference_Imagenet_Spark.ipynb (``mapPartitions``
over image paths, 10k-image limit, ``repartition(num_executors * 3)``, Parquet output with
``image_path, top1_label … top3_label``).

MI355X design: instead of Spark executors, ``batch_predict`` shards the image list over one
worker process per GPU; each worker decodes JPEG/PNG on a thread pool (PIL releases the GIL) and
runs a :class:`Predictor`: uint8 NHWC batches are packed into pinned host memory and copied to the
device on a side stream while the previous batch computes (two device input buffers), the forward
+ softmax is replayed from a hipGraph captured once per (batch shape, input buffer) — bf16
ResNet-50 frozen (runtime/frozen.py: batch norm folded into the convs, residual + ReLU in the conv
epilogue; ``frozen=False``: batch norm in its own inference kernel) — and each worker writes its
shard as Parquet; the driver concatenates the shards.  The labels can come from ``predict_topk_batches``:
the graph ends in the softmax + top-k kernel (csrc/ops/topk.hip), only the ``[B, top]`` class ids and
scores cross to the host, and the next batch's replay is already enqueued while the host labels this
one.  That path is opt-in (``HOPSX_INFER_TOPK=1``, see ``infer_topk_default``); without it the whole
probability matrix crosses and ``decode_predictions`` sorts it on the host.
No pretrained ImageNet weights exist offline, so models are random-init unless a checkpoint
is loaded, and labels default to ``class_<i>`` (pass ``labels=`` for real names).
"""
from __future__ import annotations

import concurrent.futures as cf
from pathlib import Path

import numpy as np
import pandas as pd

from . import hdfs

HEIGHT = WIDTH = 224


def load_img(path, target_size=(HEIGHT, WIDTH)) -> np.ndarray:
    from PIL import Image

    img = Image.open(str(hdfs._resolve(path)) if not Path(str(path)).exists() else str(path)).convert("RGB")
    if target_size is not None:
        img = img.resize((target_size[1], target_size[0]), Image.BILINEAR)
    return np.asarray(img, dtype=np.uint8)


def img_to_array(img) -> np.ndarray:
    return np.asarray(img, dtype=np.float32)


def preprocess_input(x: np.ndarray) -> np.ndarray:
    """Keras ResNet50 'caffe' preprocessing: RGB->BGR and ImageNet mean subtraction."""
    x = np.asarray(x, dtype=np.float32)[..., ::-1]
    return x - np.array([103.939, 116.779, 123.68], dtype=np.float32)


def decode_predictions(preds, top: int = 3, labels: list[str] | None = None):
    """[(class_id, label, score)] per row, best first (Keras ``decode_predictions`` shape)."""
    preds = np.asarray(preds)
    out = []
    for row in preds:
        idx = np.argsort(-row)[:top]
        out.append([(f"n{i:08d}", labels[i] if labels else f"class_{i}", float(row[i])) for i in idx])
    return out


def decode_topk(ids, scores, labels: list[str] | None = None):
    """``decode_predictions`` rows, [(class_id, label, score)] best first, from the ``[B, top]`` class ids and scores
    that ``predict_topk`` / ``Predictor.predict_topk_batches`` return (the selection already happened on the device)."""
    ids, scores = np.asarray(ids), np.asarray(scores)
    return [[(f"n{i:08d}", labels[i] if labels else f"class_{i}", float(s)) for i, s in zip(ri.tolist(), rs.tolist())]
            for ri, rs in zip(ids, scores)]


def _predict_probs(model, x, device):
    import torch

    with torch.no_grad():
        t = torch.from_numpy(np.ascontiguousarray(x)).to(device, non_blocking=True)
        logits = model(t)
        return torch.softmax(logits.float(), dim=-1).cpu().numpy()


def _freeze_cpu(frozen):
    if frozen is True:
        raise ValueError("frozen=True: the frozen ResNet engine runs on a GPU")
    if frozen not in ("auto", False, None):
        raise ValueError(f"frozen: 'auto', True or False, got {frozen!r}")
    return None


def _freeze(model, frozen):
    """The frozen engine for ``model`` under the ``frozen`` argument of Predictor (see there), or None."""
    import os

    from .runtime.frozen import FrozenResNet

    if frozen is True:
        return FrozenResNet.freeze(model)  # (raises for an unsupported model)
    if frozen == "auto":
        if os.environ.get("HOPSX_INFER_FROZEN", "1") == "0" or not FrozenResNet.supported(model):
            return None
        return FrozenResNet.freeze(model)
    return _freeze_cpu(frozen)


class Predictor:
    """Streaming inference on one device.

    ``predict_batches(batches)`` yields softmax probabilities per batch.  On a GPU: batch i+1 is
    packed into a pinned host buffer and copied host->device on a side stream while batch i runs;
    the forward (+ softmax) of each (batch shape, input buffer) pair is captured into a hipGraph on
    first use and replayed afterwards (``graph=False``: eager kernels, same results).  On the CPU
    it is the eager forward.  ``predict_topk_batches(batches, top)`` yields the ``top`` class ids and scores per
    batch instead, selected on the device (see there).

    ``frozen``: run the hopsx ResNets through :class:`runtime.frozen.FrozenResNet` (BatchNorm folded into
    the convs, the residual added in the conv epilogue: one launch per conv + BN pair).  ``"auto"`` freezes
    when the model is supported (a CifarResNet / ResNet50 on a GPU) unless ``HOPSX_INFER_FROZEN=0``;
    ``True`` insists (an unsupported model is an error); ``False`` keeps ``model.eval()``'s own forward.
    ``Predictor.frozen`` is the engine or None; it is a snapshot of the model taken here (call its
    ``refresh()`` after changing the model)."""

    def __init__(self, model, device=None, graph: bool = True, frozen="auto"):
        import torch

        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu"))
        self.model = model.eval()
        self.cuda = self.device.type == "cuda"
        self.graph = graph and self.cuda
        self._graphs: dict = {}  # (shape, dtype, slot) -> (graph, static_in, static_out)
        self._bufs: dict = {}    # (shape, dtype) -> ([pinned x2], [device x2])
        self._copy = torch.cuda.Stream(self.device) if self.cuda else None
        self.replays = 0
        self._topk_graphs: dict = {}  # (shape, dtype, slot, top) -> (graph, int32 [2, b, top]): forward + softmax_topk
        self._topk_pins: dict = {}    # ((2, b, top), slot) -> the pinned buffer that result is copied into
        self.topk_replays = 0
        self.frozen = _freeze(self.model, frozen) if self.cuda else _freeze_cpu(frozen)

    def _buffers(self, shape, dtype):
        import torch

        key = (tuple(shape), dtype)
        if key not in self._bufs:
            tdt = torch.from_numpy(np.zeros(1, dtype)).dtype
            self._bufs[key] = ([torch.empty(shape, dtype=tdt).pin_memory() for _ in range(2)],
                               [torch.empty(shape, dtype=tdt, device=self.device) for _ in range(2)])
        return self._bufs[key]

    def _forward(self, t):
        import torch

        return torch.softmax((self.frozen or self.model)(t).float(), dim=-1)

    def _run(self, dev_in, key):
        import torch

        if not self.graph:
            return self._forward(dev_in)
        g = self._graphs.get(key)
        if g is None:
            from .runtime.capture import graph as capture

            self._forward(dev_in)  # warm-up: first-call allocations and kernel selection, outside capture
            torch.cuda.current_stream(self.device).synchronize()
            cg = torch.cuda.CUDAGraph()
            with capture(cg):
                out = self._forward(dev_in)
            g = self._graphs[key] = (cg, out)
        g[0].replay()
        self.replays += 1
        return g[1]

    def predict_batches(self, batches):
        import torch

        if not self.cuda:
            with torch.no_grad():
                for x in batches:
                    yield self._forward(torch.from_numpy(np.ascontiguousarray(x))).numpy()
            return
        cur = torch.cuda.current_stream(self.device)
        done = [None, None]  # per input slot: event after the last replay that read it

        def stage(x, k):
            """pack batch -> pinned[k], then H2D pinned[k] -> dev[k] on the copy stream once the replay
            that last read dev[k] (two batches ago) has finished."""
            pins, devs = self._buffers(x.shape, x.dtype)
            pins[k].numpy()[...] = x  # pinned[k]'s previous H2D finished before that batch's replay
            if done[k] is not None:
                self._copy.wait_event(done[k])
            with torch.cuda.stream(self._copy):
                devs[k].copy_(pins[k], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._copy)
            return devs[k], ev, (tuple(x.shape), x.dtype, k)

        it = iter(batches)
        nxt = next(it, None)
        staged = stage(np.ascontiguousarray(nxt), 0) if nxt is not None else None
        slot = 0
        with torch.no_grad():
            while staged is not None:
                dev_in, ev, key = staged
                cur.wait_event(ev)
                out = self._run(dev_in, key)
                done[slot] = torch.cuda.Event()
                done[slot].record(cur)
                nxt = next(it, None)
                slot ^= 1
                # the next batch's packing + H2D overlap this batch's forward
                staged = stage(np.ascontiguousarray(nxt), slot) if nxt is not None else None
                yield out.cpu().numpy()  # the output buffer is reused two batches later

    def _topk_eager(self, t, top, clamp=False):
        """int32 [2, b, top] of one device batch: [0] the class ids, [1] the bits of the fp32 scores — the forward,
        then topk.hip on its logits (no probability matrix, no PyTorch softmax).  One buffer: one copy to the host."""
        import torch

        from .ops import kernels as K

        z = (self.frozen or self.model)(t)
        if z.dtype not in (torch.float32, torch.bfloat16):
            z = z.float()
        if clamp:
            top = min(top, z.shape[-1])
        out = torch.empty(2, z.shape[0], top, dtype=torch.int32, device=z.device)
        K.softmax_topk(z.contiguous(), top, out[0], out[1].view(torch.float32))
        return out

    def _run_topk(self, dev_in, key, top, clamp):
        import torch

        if not self.graph:
            return self._topk_eager(dev_in, top, clamp)
        key = (*key, top, clamp)
        g = self._topk_graphs.get(key)
        if g is None:
            from .runtime.capture import graph as capture

            self._topk_eager(dev_in, top, clamp)  # warm-up, as _run
            torch.cuda.current_stream(self.device).synchronize()
            cg = torch.cuda.CUDAGraph()
            with capture(cg):
                out = self._topk_eager(dev_in, top, clamp)
            g = self._topk_graphs[key] = (cg, out)
        g[0].replay()
        self.topk_replays += 1
        return g[1]

    def predict_topk_batches(self, batches, top: int = 3, clamp: bool = False):
        """Yields ``(ids int32 [b, top], scores float32 [b, top])`` numpy pairs, one per batch, in order: the ``top``
        largest logits' classes, best first (the lower class first among equal logits), and their softmax
        probabilities.  1 <= top <= min(8, classes); ``clamp=True`` yields ``[b, classes]`` pairs from a model with
        fewer than ``top`` classes instead of raising (``decode_predictions`` returns that many entries too).

        On a GPU the selection runs on the device behind the forward (one hipGraph per (batch shape, input buffer,
        top), counted in ``topk_replays``; ``predict_batches``' graphs and ``replays`` are not touched), the two small
        results are copied into a pinned host buffer behind it, and batch i+1's replay is enqueued BEFORE the generator
        waits for batch i's results and yields them: the device runs the next batch while the consumer labels this
        one.  The input iterator is therefore read two batches ahead of the yielded one.  On the CPU it is the eager
        forward and a stable descending sort."""
        import torch

        top = int(top)
        if not 1 <= top <= 8:
            raise ValueError(f"predict_topk_batches: 1 <= top <= 8 expected, got {top}")
        if not self.cuda:
            with torch.no_grad():
                for x in batches:
                    z = self.model(torch.from_numpy(np.ascontiguousarray(x))).float()
                    if top > z.shape[-1] and not clamp:
                        raise ValueError(f"predict_topk_batches: top = {top} > {z.shape[-1]} classes")
                    order = torch.sort(z, dim=-1, descending=True, stable=True).indices[:, :top]
                    yield (order.to(torch.int32).numpy(), torch.softmax(z, dim=-1).gather(1, order).numpy())
            return
        cur = torch.cuda.current_stream(self.device)
        done = [None, None]  # per input slot: event after the last replay that read it (and its result copy)
        h2d = [None, None]   # per input slot: event after the last H2D copy out of its pinned buffer

        def stage(x, k):
            """pack batch -> pinned[k], then H2D pinned[k] -> dev[k] on the copy stream once the replay that last
            read dev[k] has finished.  Unlike predict_batches, this generator has not waited on anything that
            followed pinned[k]'s previous H2D when it gets here (that copy's batch is still pending, only the one
            before it has been yielded), so the host waits for that copy's own event before it overwrites the
            buffer; the copy ran a whole replay ago, so the wait returns at once."""
            pins, devs = self._buffers(x.shape, x.dtype)
            if h2d[k] is not None:
                h2d[k].synchronize()
            pins[k].numpy()[...] = x
            if done[k] is not None:
                self._copy.wait_event(done[k])
            with torch.cuda.stream(self._copy):
                devs[k].copy_(pins[k], non_blocking=True)
                ev = h2d[k] = torch.cuda.Event()
                ev.record(self._copy)
            return devs[k], ev, (tuple(x.shape), x.dtype, k)

        def fetch(out, k):
            """D2H of one batch's ids and scores into slot k's pinned buffer (free: that slot's previous batch was
            yielded, hence copied out, one iteration ago) behind the replay, and the event behind the copy."""
            pk = (tuple(out.shape), k)
            if pk not in self._topk_pins:
                self._topk_pins[pk] = torch.empty(out.shape, dtype=torch.int32).pin_memory()
            pin = self._topk_pins[pk]
            pin.copy_(out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cur)
            return ev, pin

        def result(p):
            # p[1] is the pinned int32 [2, b, top] copy of _topk_eager's buffer: [0] the ids, [1] the fp32 scores' BITS
            # (the kernel wrote floats through a float32 view of that half), hence the reinterpreting view, not a cast
            p[0].synchronize()
            return p[1][0].numpy().copy(), p[1][1].numpy().view(np.float32).copy()

        it = iter(batches)
        nxt = next(it, None)
        staged = stage(np.ascontiguousarray(nxt), 0) if nxt is not None else None
        slot = 0
        pending = None  # the batch whose replay and copy are enqueued and not yet yielded
        with torch.no_grad():
            while staged is not None:
                dev_in, ev, key = staged
                cur.wait_event(ev)
                out = self._run_topk(dev_in, key, top, clamp)
                mine = fetch(out, slot)
                done[slot] = mine[0]  # (one event serves both: the input slot is free once the results are out)
                nxt = next(it, None)
                slot ^= 1
                staged = stage(np.ascontiguousarray(nxt), slot) if nxt is not None else None
                if pending is not None:
                    yield result(pending)
                pending = mine
            if pending is not None:
                yield result(pending)


def predict(model, images: np.ndarray, batch_size: int = 64, device=None, graph: bool = True,
            frozen="auto") -> np.ndarray:
    """Softmax probabilities for uint8 NHWC ``images`` (the hopsx ResNets normalise on device).  ``frozen``: see
    :class:`Predictor`."""
    pr = Predictor(model, device, graph=graph, frozen=frozen)
    batches = (images[i:i + batch_size] for i in range(0, len(images), batch_size))
    return np.concatenate(list(pr.predict_batches(batches)))


def predict_topk(model, images: np.ndarray, top: int = 3, batch_size: int = 64, device=None, graph: bool = True,
                 frozen="auto"):
    """``(ids int32 [N, top], scores float32 [N, top])`` for uint8 NHWC ``images``: the ``top`` most probable classes
    per image, best first, and their softmax probabilities, selected on the device (``Predictor.predict_topk_batches``).
    ``frozen``: see :class:`Predictor`."""
    pr = Predictor(model, device, graph=graph, frozen=frozen)
    batches = (images[i:i + batch_size] for i in range(0, len(images), batch_size))
    out = list(pr.predict_topk_batches(batches, top))
    if not out:
        return np.empty((0, int(top)), np.int32), np.empty((0, int(top)), np.float32)
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def infer_topk_default() -> bool:
    """Whether ``batch_predict`` labels through ``predict_topk_batches``: ``HOPSX_INFER_TOPK=1``.  Opt-in: measured
    end to end against ``predict_batches`` + ``decode_predictions`` (tools/infer_topk_bench.py,
    profiles/r19_infer_topk.txt) it is faster for ResNet-50 at B=100 (8 %) and ResNet-20 at B=128 (2.3 x), and within
    1 % either way for ResNet-50 at B=8 (one run won every pair, the next lost every pair, a third was level); the default goes to it only
    once it wins everywhere."""
    import os

    return os.environ.get("HOPSX_INFER_TOPK", "0") == "1"


def _label_frame(paths, ids, scores, labels):
    """The label table of ``batch_predict`` from ``[N, top]`` ids and scores, built column by column."""
    cols = {"image_path": [str(p) for p in paths]}
    names = np.asarray(labels, dtype=object) if labels else None
    for j in range(ids.shape[1]):
        cid = ids[:, j]
        cols[f"top{j + 1}_id"] = np.char.mod("n%08d", cid).astype(object)
        cols[f"top{j + 1}_label"] = names[cid] if names is not None else np.char.mod("class_%d", cid).astype(object)
        cols[f"top{j + 1}_score"] = scores[:, j].astype(np.float64)
    return pd.DataFrame(cols)


def _shard_worker(model_builder, checkpoint, paths, batch_size, top, labels, out_path, threads, frozen="auto"):
    import torch

    from .runtime.arena import ParamArena

    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    model = model_builder()
    if checkpoint:
        from .model import load_torch

        sd = load_torch(checkpoint, device="cpu") if str(checkpoint).endswith(".pt") else None
        if isinstance(sd, dict):
            model.load_state_dict(sd)
    model = model.to(dev).eval()
    if dev.type == "cuda":
        ParamArena.from_module(model, dev)
    rows = []
    pool = cf.ThreadPoolExecutor(threads)

    def load(p):
        try:
            return p, load_img(p)
        except Exception:  # malformed images are skipped, as the reference does
            return p, None

    batches = [paths[i:i + batch_size] for i in range(0, len(paths), batch_size)]
    order: list = []  # paths of the batches handed to the predictor, in order

    def decoded():
        fut = pool.map(load, batches[0]) if batches else None
        for bi in range(len(batches)):
            loaded = [(p, a) for p, a in fut if a is not None]
            if bi + 1 < len(batches):
                fut = pool.map(load, batches[bi + 1])  # decode the next batch while this one runs
            if loaded:
                order.append([p for p, _ in loaded])
                yield np.stack([a for _, a in loaded])

    predictor = Predictor(model, dev, frozen=frozen)
    if infer_topk_default() and 1 <= top <= 8:
        # (clamp: a model with fewer than `top` classes gets that many column groups, as from decode_predictions)
        out = list(predictor.predict_topk_batches(decoded(), top, clamp=True))
        if out:
            df = _label_frame([p for b in order for p in b], np.concatenate([o[0] for o in out]),
                              np.concatenate([o[1] for o in out]), labels)
            df.attrs["graph_replays"] = predictor.topk_replays
        else:
            df = pd.DataFrame([])
        df.to_parquet(out_path, index=False)
        return len(df)
    for bi, probs in enumerate(predictor.predict_batches(decoded())):
        for p, dec in zip(order[bi], decode_predictions(probs, top, labels)):
            r = {"image_path": str(p)}
            for k, (cid, lab, sc) in enumerate(dec, 1):
                r[f"top{k}_id"], r[f"top{k}_label"], r[f"top{k}_score"] = cid, lab, sc
            rows.append(r)
    df = pd.DataFrame(rows)
    if rows:
        df.attrs["graph_replays"] = predictor.replays
    df.to_parquet(out_path, index=False)
    return len(df)


def batch_predict(model_builder, image_paths: list, output_path: str, batch_size: int = 100, top: int = 3,
                  labels: list[str] | None = None, num_workers: int | None = None, limit: int | None = None,
                  checkpoint: str | None = None, decode_threads: int = 8, timeout: float | None = None,
                  frozen="auto") -> pd.DataFrame:
    """Label ``image_paths`` with one worker process per GPU; writes ``output_path`` (Parquet dir).  ``frozen``:
    see :class:`Predictor`."""
    from .experiment import _runner as R

    paths = list(image_paths)[:limit] if limit else list(image_paths)
    ngpu = R.num_gpus()
    n = num_workers or max(1, ngpu)
    out = Path(hdfs._resolve(output_path))
    out.mkdir(parents=True, exist_ok=True)
    for f in out.glob("part-*.parquet"):
        f.unlink()
    shards = [paths[i::n] for i in range(n)]
    workers = []
    for i, sh in enumerate(shards):
        if not sh:
            continue
        w = R.spawn(_shard_worker, {"model_builder": model_builder, "checkpoint": checkpoint, "paths": sh,
                                    "batch_size": batch_size, "top": top, "labels": labels,
                                    "out_path": str(out / f"part-{i:05d}.parquet"), "threads": decode_threads,
                                    "frozen": frozen},
                    out / "_logs", log_name=f"worker_{i}_output.log", gpu=(i % ngpu) if ngpu else None)
        workers.append(w)
    for w in workers:
        R.collect(w, timeout)
    return read_labels(output_path)


def read_labels(output_path: str) -> pd.DataFrame:
    out = Path(hdfs._resolve(output_path))
    frames = [pd.read_parquet(f) for f in sorted(out.glob("part-*.parquet"))]
    return pd.concat(frames, ignore_index=True) if frames else pd.DataFrame()
