"""Benchmark harness for every BASELINE.json config (+ the reference's ResNet-50 benchmark notebook).

    python benchmarks/run.py <config> [--gpus N] [--steps K] [--warmup W] [--batch B] [--rehearse]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 benchmarks/run.py <config>

``--gpus N`` without a rank environment launches N ranks itself (parallel/launch.py; refuses when
fewer than N GPUs are visible unless ``--rehearse``).  ``cifar_resnet`` runs through
``experiment.collective_allreduce`` (BASELINE config 5): the workers are experiment workers
(chief_0_output.log / worker_<i>_output.log in Experiments/<id>/) and the chief's returned
record is the printed JSON line.

configs:
  mnist_launch_cpu   MNIST 2-layer CNN through experiment.launch on CPU (plumbing; images/s)
  mnist_mirrored     MNIST CNN (E3, 1.39M params) bf16, DP over RCCL (images/s)       == bench.py
  mnist_ps           the same model through experiment.parameter_server's sharded-PS engine (images/s)
  taxi               Chicago-taxi wide & deep trainer (steps/s)
  titanic            Titanic TD (Parquet) -> HBM ingest (GB/s) + 7.8k-param DNN (steps/s)
  titanic_ingest     GB-scale TD ingest alone (--rows; raw column GB/s per rank) + the 891k-row fixed cost
  cifar_resnet       CIFAR-10 ResNet-20/56, collective all-reduce (images/s)
  resnet50           ResNet-50 224x224, RMSprop(0.2), batch 8/GPU as benchmark.ipynb (images/s)

Every run prints one JSON line (rank 0) with the whole-job value; data are synthetic with the
real shapes, weights random-init.  Timing: warmup untimed, then K steps between a barrier +
device synchronize on both sides, max over ranks.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hops_examples_amd.parallel import dist as hdist  # noqa: E402


def timed(fn, n, dev):
    hdist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if hasattr(fn, "run_n"):
        fn.run_n(n)  # n steps, replayed steps_per_execution at a time
    else:
        for i in range(n):
            fn(i)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    hdist.barrier()
    return hdist.all_reduce_scalar(time.perf_counter() - t0, "max")


def _train_loop(model, opt, kind, xs, ys, steps, warmup, dev, world, forward_fn=None, box=None, mode=None,
                stats=None):
    from hops_examples_amd.parallel import ps as P
    from hops_examples_amd.runtime.step import TrainStep

    dp = P.make(model, opt, mode) if world > 1 else None
    if box is not None:
        box["dp"] = dp
    st = TrainStep(model, opt, kind, dp=dp, graph=dev.type == "cuda", forward_fn=forward_fn)
    nb = len(xs)
    box = {}

    def run(i):
        box["r"] = st(xs[i % nb], ys[i % nb])
        if "first" not in box:
            box["first"] = float(box["r"]["loss"].reshape(-1)[0])  # initial loss (learning check)

    # one GPU: the epoch stays resident in HBM and steps_per_execution steps replay as ONE graph, the
    # optimizer kernel's tail copying the next batch into the input buffers (TrainStep.run_resident,
    # as bench.py's flagship) — no per-step graph launch or input copy.  HOPSX_BENCH_RESIDENT=0: per step
    resident = (world == 1 and st.use_graph and forward_fn is None and torch.is_tensor(xs) and torch.is_tensor(ys)
                and os.environ.get("HOPSX_BENCH_RESIDENT", "1") != "0"
                # the in-kernel prefetch moves 16-B chunks: every batch slice a multiple of 16 bytes
                and all(t[0].numel() * t.element_size() % 16 == 0 for t in (xs, ys)))
    if resident:
        def run(i):
            box["r"] = st.step_resident(xs, ys)
            if "first" not in box:
                box["first"] = float(box["r"]["loss"].reshape(-1)[0])

        def run_n(n):
            box["r"] = st.run_resident(xs, ys, n)

        run.run_n = run_n
    # TrainStep runs `st.warmup` eager steps and captures the graph on the next one: warm up past the
    # capture, so the timed window holds replays only (whatever --warmup says)
    for i in range(max(warmup, st.warmup + 2 if st.use_graph else warmup)):
        run(i)
    if resident:
        st.prepare_resident(xs, ys, n=steps)  # capture the multi-step graphs untimed
    el = timed(run, steps, dev)
    if stats is not None:
        stats["initial_loss"] = box["first"]
    return el, float(box["r"]["loss"].reshape(-1)[0])


def _record(metric, value, unit, steps, warmup, el, world, cfg, extra=None) -> dict:
    rec = {"metric": metric, "value": round(value, 2), "unit": unit, "n_gpus": world, "steps": steps,
           "warmup": warmup, "ms_per_step": round(el / steps * 1e3, 4), "higher_is_better": True,
           "scaling": "weak", "dtype": "bf16", "data": "synthetic", "config": cfg}
    if extra:
        rec.update(extra)
    return rec


def _emit(rank, metric, value, unit, steps, warmup, el, world, cfg, extra=None):
    if rank != 0:
        return
    print(json.dumps(_record(metric, value, unit, steps, warmup, el, world, cfg, extra)), flush=True)


def cfg_mnist_mirrored(a, dev, rank, world, mode=None):
    from hops_examples_amd import optim
    from hops_examples_amd.models.mnist import MirroredMnistCNN
    from hops_examples_amd.runtime.arena import ALIGN, ParamArena

    B = a.batch or 32
    m = MirroredMnistCNN().to(dev)
    ParamArena.from_module(m, dev, pad_multiple=max(1, world) * ALIGN)
    opt = optim.Adadelta(m, lr=1.0)
    nb = max(8, -(-61440 // B))
    xs = torch.randint(0, 256, (nb, B, 28, 28, 1), dtype=torch.uint8, device=dev)
    ys = torch.randint(0, 10, (nb, B), device=dev)
    box = {}
    el, loss = _train_loop(m, opt, "sparse_ce", xs, ys, a.steps, a.warmup, dev, world, box=box, mode=mode)
    dp = box.get("dp")
    _emit(rank, "images/sec MNIST CNN (E3) DP" + (" parameter-server" if mode == "parameter_server" else ""),
          B * world * a.steps / el, "images/sec", a.steps, a.warmup, el, world,
          {"model": "MirroredMnistCNN 1,394,282 params", "per_gpu_batch": B, "parallelism": f"dp{world}",
           "engine": type(dp).__name__ if dp is not None else None},
          {"final_loss": round(loss, 4)})


def cfg_mnist_ps(a, dev, rank, world):
    """experiment.parameter_server's engine (parallel/ps.py ShardedPS: reduce-scatter of the gradient to the
    shard owners, owner-only optimizer update, bf16 all-gather of the weights) on the E3 model."""
    cfg_mnist_mirrored(a, dev, rank, world, mode="parameter_server")


def cfg_mnist_launch_cpu(a, dev, rank, world):
    from hops_examples_amd import experiment

    steps, B = a.steps, a.batch or 32

    def train():
        import time as _t

        import torch as _torch

        from hops_examples_amd import optim as _optim
        from hops_examples_amd.models.mnist import KerasMnistCNN
        from hops_examples_amd.runtime.arena import ParamArena as _PA
        from hops_examples_amd.runtime.step import TrainStep as _TS

        _torch.set_num_threads(max(1, (os.cpu_count() or 2) // 2))
        m = KerasMnistCNN()
        _PA.from_module(m)
        st = _TS(m, _optim.Adadelta(m, lr=1.0), "sparse_ce", graph=False)
        x = _torch.randint(0, 256, (B, 28, 28, 1), dtype=_torch.uint8)
        y = _torch.randint(0, 10, (B,))
        for _ in range(2):
            st(x, y)
        t0 = _t.perf_counter()
        for _ in range(steps):
            r = st(x, y)
        el = _t.perf_counter() - t0
        return {"images_per_sec": B * steps / el, "elapsed": el, "loss": float(r["loss"])}

    os.environ.setdefault("HOPSX_NUM_GPUS", "0")
    t0 = time.perf_counter()
    _, res = experiment.launch(train, name="mnist_launch_cpu")
    wall = time.perf_counter() - t0
    _emit(rank, "images/sec MNIST 2-layer CNN via experiment.launch on CPU", res["images_per_sec"], "images/sec",
          steps, 2, res["elapsed"], 1, {"model": "KerasMnistCNN 239,594 params", "per_gpu_batch": B,
                                        "parallelism": "cpu"},
          {"dtype": "fp32", "launch_wall_s": round(wall, 2)})


def cfg_taxi(a, dev, rank, world):
    from hops_examples_amd.models.widedeep import TRAIN_BATCH_SIZE, bench_taxi

    B = a.batch or TRAIN_BATCH_SIZE
    r = bench_taxi(dev, B, a.steps, a.warmup, timed, world, graph=dev.type == "cuda", from_transform=a.from_transform)
    _emit(rank, "steps/sec Chicago-taxi wide&deep", r["steps_per_sec"], "steps/sec", a.steps, a.warmup,
          r["ms_per_step"] * a.steps / 1e3, world, {"model": f"TaxiWideDeep {r['params']} params", "per_gpu_batch": B,
                                                     "parallelism": f"dp{world}"},
          {"examples_per_sec": r["examples_per_sec"], "final_loss": r["loss"], "data": r["data"],
           "transform_s": r.get("transform_s")})


def _titanic_td(rows: int, rank: int):
    """The featurestore tour's Titanic training dataset at ``rows`` synthetic passengers: rank 0
    builds the feature group and the Parquet TD (64k-row row groups) once, every rank opens it."""
    import numpy as np
    import pandas as pd

    import hsfs

    name = f"titanic_bench_v2_{rows}"
    fs = hsfs.connection().get_feature_store()
    if rank == 0:
        try:
            fs.get_training_dataset(name, 1)
        except Exception:  # noqa: BLE001 - first run: build it
            rng = np.random.default_rng(0)
            df = pd.DataFrame({"passenger_id": np.arange(rows), "pclass": rng.integers(1, 4, rows),
                               "sex": rng.integers(0, 2, rows), "fare": rng.gamma(2.0, 16.0, rows),
                               "age": rng.normal(30, 12, rows).clip(1, 80), "sibsp": rng.integers(0, 5, rows),
                               "parch": rng.integers(0, 4, rows)})
            df["survived"] = ((df.sex == 1) ^ (rng.random(rows) < 0.2)).astype(np.int64)
            fg = fs.create_feature_group(f"{name}_fg", 1, primary_key=["passenger_id"],
                                         statistics_config={"enabled": False})
            fg.save(df)
            td = fs.create_training_dataset(name, 1, data_format="parquet", label=["survived"],
                                            statistics_config={"enabled": True})
            td.save(fg.select(["pclass", "sex", "fare", "age", "sibsp", "parch", "survived"]))
    hdist.barrier()
    return fs.get_training_dataset(name, 1)


def titanic_record(rows: int, batch: int, steps: int, warmup: int) -> dict:
    """BASELINE config 4: the featurestore tour's Titanic training dataset (Parquet) -> a DNN, one
    rank per GPU.  Every rank streams ONLY its row groups of the TD into HBM
    (td.to_device(shard=(world, rank)): Arrow decode -> pinned staging -> side-stream H2D -> fp32
    convert on the GPU; reference: PetastormHelloWorld.ipynb:864-899 shard_count / cur_shard), then
    trains with the gradient all-reduce.  Returns the JSON record on rank 0."""
    from hops_examples_amd import optim
    from hops_examples_amd.models.zoo import titanic_dnn
    from hops_examples_amd.parallel import launch
    from hops_examples_amd.runtime.arena import ALIGN, ParamArena

    rank, _, world = hdist.init()
    dev = hdist.device()
    torch.manual_seed(1234 + rank)
    os.environ.setdefault("HOPSX_PROJECT_ROOT", os.path.join(os.environ.get("TMPDIR", "/tmp"), "hopsx_bench_project"))
    B = batch or 10
    td = _titanic_td(rows, rank)
    feats = ["pclass", "sex", "fare", "age", "sibsp", "parch"]
    td.to_device("survived", feature_names=feats, device=dev, shard=(world, rank) if world > 1 else None)  # warm
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    xd, yd = td.to_device("survived", feature_names=feats, device=dev, shard=(world, rank) if world > 1 else None)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    ingest = time.perf_counter() - t0
    local_rows = xd.shape[0]
    gbps = local_rows * 7 * 4 / ingest / 1e9
    # standardise the features with the training dataset's own statistics (computed when the TD was
    # written; TitanicTrainingDatasetPython.ipynb:113-129 cleans, the statistics scale): raw fare / age
    # saturate the sigmoid layer and the clipped cross-entropy stops learning
    st = {c["column"]: c for c in td.get_statistics()["columns"]}
    mu = torch.tensor([st[f]["mean"] for f in feats], device=dev, dtype=xd.dtype)
    sd = torch.tensor([max(st[f]["stdDev"], 1e-6) for f in feats], device=dev, dtype=xd.dtype)
    xd = (xd - mu) / sd
    m = titanic_dnn()
    m.build((6,))
    net = m.net.to(dev)
    ParamArena.from_module(net, dev, pad_multiple=max(1, world) * ALIGN)
    opt = optim.Adam(net, lr=1e-3, eps=1e-7)
    nb = local_rows // B
    xs = xd[: nb * B].view(nb, B, 6)
    ys = yd[: nb * B].view(nb, B, 1)
    box, lst = {}, {}
    # the maggy-ablation Titanic DNN ends in Dense(1, linear); the notebook compiles it with the
    # probability-form cross-entropy (maggy-ablation-titanic-example.ipynb:415-426), whose clip has no
    # gradient outside (0, 1) — read the linear output as a logit instead, so the benchmark trains
    el, loss = _train_loop(net, opt, "bce_logits", xs, ys, steps, warmup, dev, world, box=box, stats=lst)
    dp = box.get("dp")
    if steps + warmup >= 50 and not loss < lst["initial_loss"]:  # (a 2-step rehearsal proves nothing)
        raise SystemExit(f"[titanic] the model did not learn: loss {lst['initial_loss']:.4f} -> {loss:.4f}")
    extra = {"ingest_GBps_parquet_to_hbm_per_rank": round(gbps, 3),
             "ingest_raw_column_GBps_per_rank": round(getattr(td, "last_read_bytes", 0) / ingest / 1e9, 3),
             "rows_per_rank": int(local_rows),
             "shard_mode": getattr(td, "last_shard_mode", None), "final_loss": round(loss, 4),
             "initial_loss": round(lst["initial_loss"], 4), "normalised": "td statistics (mean / stdDev)",
             "loss": "sigmoid cross-entropy on the linear output",
             "dtype": "bf16" if dev.type == "cuda" else "fp32"}
    if dp is not None and hasattr(dp, "verify_replicas"):
        extra["replicas_identical"] = dp.verify_replicas()["identical"]
    ranks = launch.gather_rank_info(dev, {"rows": int(local_rows), "ingest_s": round(ingest, 4)})
    if dp is not None and hasattr(dp, "close"):
        dp.close()
    rec = _record("steps/sec Titanic TD -> DNN", steps / el, "steps/sec", steps, warmup, el, world,
                  {"model": f"titanic_dnn {m.count_params()} params", "per_gpu_batch": B, "global_batch": B * world,
                   "parallelism": f"dp{world}", "rows": rows, "launcher": "experiment.mirrored" if world > 1 else
                   "process", "allreduce": getattr(dp, "path", None), "ranks": ranks}, extra)
    hdist.shutdown()
    return rec if rank == 0 else {}


def _ingest_td(name: str, rows: int, rank: int, write_options: dict):
    """A Titanic-schema training dataset of ``rows`` synthetic passengers written straight from a
    frame (rank 0, once), as Parquet parts with the given write options."""
    import numpy as np
    import pandas as pd

    import hsfs

    fs = hsfs.connection().get_feature_store()
    if rank == 0:
        try:
            fs.get_training_dataset(name, 1)
        except Exception:  # noqa: BLE001 - first run: write it
            rng = np.random.default_rng(0)
            df = pd.DataFrame({"pclass": rng.integers(1, 4, rows), "sex": rng.integers(0, 2, rows),
                               "fare": rng.gamma(2.0, 16.0, rows), "age": rng.normal(30, 12, rows).clip(1, 80),
                               "sibsp": rng.integers(0, 5, rows), "parch": rng.integers(0, 4, rows)})
            df["survived"] = ((df.sex == 1) ^ (rng.random(rows) < 0.2)).astype(np.int64)
            td = fs.create_training_dataset(name, 1, data_format="parquet", label=["survived"],
                                            statistics_config={"enabled": False})
            td.save(df, write_options=write_options)
            del df
    hdist.barrier()
    return fs.get_training_dataset(name, 1)


def cfg_titanic_ingest(a, dev, rank, world):
    """BASELINE config 4's ingest at GB scale: a ``--rows`` Titanic-schema training dataset (PLAIN,
    uncompressed Parquet parts, 1M-row row groups) streamed into HBM by td.to_device — native decode
    into the pinned ring (csrc/io/parquet_core.h), side-stream H2D, GPU convert — best of 3 warm reads;
    plus the fixed cost of the 891k-row TD in the default layout (snappy + dictionary, 64k-row groups).
    Reference: PetastormHelloWorld.ipynb:864-899, training_datasets.ipynb:463-526."""
    os.environ.setdefault("HOPSX_PROJECT_ROOT", os.path.join(os.environ.get("TMPDIR", "/tmp"), "hopsx_bench_project"))
    feats = ["pclass", "sex", "fare", "age", "sibsp", "parch"]
    shard = (world, rank) if world > 1 else None

    def best_read(td, reps):
        ts, x = [], None
        for _ in range(reps):
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            x, y = td.to_device("survived", feature_names=feats, device=dev, shard=shard)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return min(ts), x, getattr(td, "last_read_bytes", 0)

    small = _ingest_td("titanic_ingest_891k", 891_000, rank, {})
    best_read(small, 1)  # warm: footers, staging ring, kernels
    t_small, xs, _ = best_read(small, 5)
    # the layouts: PLAIN uncompressed (the decoder's best case), snappy pages, snappy + dictionary pages
    # (pyarrow's defaults, as the reference's own telco-delta parts) — same rows, 1M-row groups
    layouts = {"plain": {"compression": None, "use_dictionary": False},
               "snappy": {"compression": "snappy", "use_dictionary": False},
               "snappy_dict": {"compression": "snappy", "use_dictionary": True}}
    pick = [l for l in (a.layout.split(",") if a.layout != "all" else layouts)]
    per = {}
    for lay in pick:
        opts = dict(layouts[lay], row_group_size=1 << 20, part_rows=4 << 20)
        suffix = "" if lay == "plain" else f"_{lay}"
        big = _ingest_td(f"titanic_ingest_{a.rows}{suffix}", a.rows, rank, opts)
        best_read(big, 1)
        t_big, xb, nbytes = best_read(big, 3)
        t_max = hdist.all_reduce_scalar(t_big, "max")
        per[lay] = {"GBps_per_rank": round(nbytes / t_big / 1e9, 3), "seconds_per_read": round(t_big, 4),
                    "job_GBps": round(nbytes * world / t_max / 1e9, 3), "raw_column_bytes_per_rank": int(nbytes),
                    "rows_per_rank": int(xb.shape[0])}
        del xb
    head = pick[0]
    if rank == 0:
        rec = _record("GB/s Titanic TD Parquet -> HBM ingest (raw column bytes, per rank)", per[head]["GBps_per_rank"],
                      "GB/s", 3, 1, per[head]["seconds_per_read"], world,
                      {"model": None, "rows": a.rows, "layout": f"{head} (value); all layouts in 'layouts'",
                       "row_group_rows": 1 << 20, "parallelism": f"dp{world}"},
                      {"layouts": per, "fixed_cost_891k_rows_ms": round(t_small * 1e3, 3),
                       "rows_891k_decoded": int(xs.shape[0]),
                       "decoder": "native" if os.environ.get("HOPSX_PARQUET_NATIVE", "1") == "1" else "arrow",
                       "decode_workers": int(os.environ.get("HOPSX_PARQUET_WORKERS", "0")) or None})
        print(json.dumps(rec), flush=True)


def cfg_titanic(a, dev, rank, world):
    rec = titanic_record(a.rows, a.batch, a.steps, a.warmup)
    if rank == 0:
        print(json.dumps(rec), flush=True)


def titanic_via_experiment(a) -> int:
    """BASELINE config 4 at N ranks: the training function runs under ``experiment.mirrored``."""
    from hops_examples_amd import experiment
    from hops_examples_amd.parallel import launch

    n = a.gpus
    if launch.visible_gpus() < n and not a.rehearse:
        print(f"[run] {n} workers requested but {launch.visible_gpus()} GPU(s) visible; refusing", file=sys.stderr)
        return 2
    if launch.visible_gpus() < n:
        os.environ.setdefault("HOPSX_DIST_BACKEND", "gloo")  # rehearsal: ranks share a device / the CPU
    os.environ.setdefault("HOPSX_PROJECT_ROOT", os.path.join(os.environ.get("TMPDIR", "/tmp"), "hopsx_bench_project"))
    rows, batch, steps, warmup = a.rows, a.batch, a.steps, a.warmup

    def train():
        sys.path.insert(0, ROOT)
        return titanic_record(rows, batch, steps, warmup)

    exp_dir, res = experiment.mirrored(train, name="titanic_td_bench", num_workers=n, metric_key="value")
    res = dict(res)
    res["experiment_dir"] = exp_dir
    print(json.dumps(res), flush=True)
    return 0


def cifar_resnet_record(depth: int, batch: int, steps: int, warmup: int) -> dict:
    """One rank of the CIFAR-10 ResNet benchmark (runs inside an experiment worker or a rank
    process; the process group is initialised here).  Returns the JSON record on rank 0, {} else."""
    from hops_examples_amd import optim
    from hops_examples_amd.models.resnet import cifar_resnet
    from hops_examples_amd.parallel import launch
    from hops_examples_amd.runtime.arena import ALIGN, ParamArena

    rank, _, world = hdist.init()
    dev = hdist.device()
    torch.manual_seed(1234 + rank)
    B = batch or 128
    m = cifar_resnet(depth).to(dev)
    ParamArena.from_module(m, dev, pad_multiple=max(1, world) * ALIGN)
    opt = optim.SGD(m, lr=0.1, momentum=0.9, weight_decay=1e-4)
    nb = 16
    xs = torch.randint(0, 256, (nb, B, 32, 32, 3), dtype=torch.uint8, device=dev)
    ys = torch.randint(0, 10, (nb, B), device=dev)
    box = {}
    el, loss = _train_loop(m, opt, "sparse_ce", xs, ys, steps, warmup, dev, world, box=box)
    dp = box.get("dp")
    extra = {"final_loss": round(loss, 4)}
    if dp is not None and hasattr(dp, "verify_replicas"):
        extra["replicas_identical"] = dp.verify_replicas()["identical"]
    ranks = launch.gather_rank_info(dev)
    if dp is not None and hasattr(dp, "close"):
        dp.close()
    rec = _record(f"images/sec CIFAR-10 ResNet-{depth} collective all-reduce", B * world * steps / el, "images/sec",
                  steps, warmup, el, world, {"model": f"ResNet-{depth}", "per_gpu_batch": B, "global_batch": B * world,
                                             "parallelism": f"dp{world}", "launcher": "experiment.collective_allreduce",
                                             "allreduce": getattr(dp, "path", None), "ranks": ranks},
                  dict(extra, dtype="bf16" if dev.type == "cuda" else "fp32"))
    hdist.shutdown()
    return rec if rank == 0 else {}


def cfg_cifar_resnet(a, dev, rank, world):
    rec = cifar_resnet_record(a.depth, a.batch, a.steps, a.warmup)
    if rank == 0:
        print(json.dumps(rec), flush=True)


def cifar_via_experiment(a) -> int:
    """BASELINE config 5 as the reference names it: the training function runs under
    ``experiment.collective_allreduce`` (one worker process per GPU, RCCL / P2P over xGMI)."""
    from hops_examples_amd import experiment
    from hops_examples_amd.parallel import launch

    n = a.gpus
    if launch.visible_gpus() < n and not a.rehearse:
        print(f"[run] {n} workers requested but {launch.visible_gpus()} GPU(s) visible; refusing", file=sys.stderr)
        return 2
    if launch.visible_gpus() < n:
        os.environ.setdefault("HOPSX_DIST_BACKEND", "gloo")  # rehearsal: ranks share a device / the CPU
    depth, batch, steps, warmup = a.depth, a.batch, a.steps, a.warmup

    def train():
        sys.path.insert(0, ROOT)
        return cifar_resnet_record(depth, batch, steps, warmup)

    exp_dir, res = experiment.collective_allreduce(train, name=f"cifar_resnet{depth}_bench", num_workers=n,
                                                   metric_key="value")
    res = dict(res)
    res["experiment_dir"] = exp_dir
    print(json.dumps(res), flush=True)
    return 0


def cfg_resnet50(a, dev, rank, world):
    from hops_examples_amd import optim
    from hops_examples_amd.models.resnet import resnet50
    from hops_examples_amd.runtime.arena import ALIGN, ParamArena

    B = a.batch or 8
    m = resnet50().to(dev)
    ParamArena.from_module(m, dev, pad_multiple=max(1, world) * ALIGN)
    opt = optim.RMSprop(m, lr=0.2)
    nb = 4
    xs = torch.randint(0, 256, (nb, B, 224, 224, 3), dtype=torch.uint8, device=dev)
    ys = torch.randint(0, 1000, (nb, B), device=dev)
    box = {}
    el, loss = _train_loop(m, opt, "sparse_ce", xs, ys, a.steps, a.warmup, dev, world, box=box)
    dp = box.get("dp")
    extra = {"final_loss": round(loss, 4)}
    if dp is not None:
        extra.update(allreduce=dp.path, buckets=len(getattr(dp, "buckets", [])),
                     grad_hbm_bytes_per_param=getattr(dp, "grad_hbm_bytes_per_param", None))
    _emit(rank, "images/sec ResNet-50 224x224 (benchmark.ipynb)", B * world * a.steps / el, "images/sec", a.steps,
          a.warmup, el, world, {"model": "ResNet-50 25,557,032 params", "per_gpu_batch": B,
                                "parallelism": f"dp{world}"}, extra)


CONFIGS = {"mnist_launch_cpu": cfg_mnist_launch_cpu, "mnist_mirrored": cfg_mnist_mirrored, "mnist_ps": cfg_mnist_ps,
           "taxi": cfg_taxi,
           "titanic": cfg_titanic, "titanic_ingest": cfg_titanic_ingest, "cifar_resnet": cfg_cifar_resnet, "resnet50": cfg_resnet50}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--rows", type=int, default=891 * 1000)
    ap.add_argument("--layout", default="plain", help="titanic_ingest: plain,snappy,snappy_dict or all")
    ap.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    ap.add_argument("--rehearse", action="store_true", help="allow more ranks than GPUs (shared devices, gloo)")
    ap.add_argument("--from-transform", action="store_true",
                    help="taxi: train on the TFX Transform stage's output (raw trips analyzed + transformed on the GPU)")
    ap.add_argument("--inline", action="store_true",
                    help="cifar_resnet on one GPU in this process (no experiment worker: profilers see the kernels)")
    a = ap.parse_args()
    from hops_examples_amd.parallel import launch

    if not launch.is_rank_process():
        if a.config == "cifar_resnet" and not (a.inline and a.gpus == 1):
            sys.exit(cifar_via_experiment(a))
        if a.config == "titanic" and a.gpus > 1:
            sys.exit(titanic_via_experiment(a))
        if a.gpus > 1:
            sys.exit(launch.launch(a.gpus, [os.path.abspath(__file__)] + sys.argv[1:], rehearse=a.rehearse))
    rank, _, world = hdist.init()
    dev = hdist.device()
    torch.manual_seed(1234 + rank)
    CONFIGS[a.config](a, dev, rank, world)
    # the ordered teardown bench.py ends with (a no-op after a config that shut down itself): a rank that left
    # its process group to interpreter teardown could abort there ("terminate called without an active exception")
    hdist.shutdown()
    launch.rank_exit(0)  # a finished rank of the self-launch skips interpreter teardown (see launch.rank_exit)


if __name__ == "__main__":
    main()
