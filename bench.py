#!/usr/bin/env python3
"""Headline benchmark: MNIST CNN (experiment.mirrored model) training throughput.

BASELINE.json metric "images/sec MNIST CNN + steps/sec Chicago-taxi DNN at 1/2/4/8 MI355X",
config 2 "MNIST CNN experiment.mirrored bf16 on 8xMI355X (RCCL gradient all-reduce)".

Model   : the MirroredStrategy MNIST CNN of the reference
          (notebooks/ml/Distributed_Training/mirrored_strategy/mirroredstrategy_mnist_example.ipynb:189-207;
          Conv32 k2 -> Conv64 k2 -> MaxPool2 -> Dropout .01 -> Dense128 -> Dense10, 1,394,282 params,
          Adadelta(1.0), categorical cross-entropy), random init.
Data    : synthetic uint8 28x28 images + labels resident in HBM (no dataset download possible).
Scaling : weak — per-GPU batch fixed (reference: 32 x num_replicas_in_sync, :128-131).
Step    : full training step inside the timed region — forward, fused loss, backward,
          gradient exchange (world > 1), fused Adadelta update.  hipGraph replay, 32 consecutive
          steps per graph (Keras steps_per_execution: every step still trains on its own batch,
          the last kernel of each step prefetches the next one).
World>1 : one process per GPU.  On one node the gradient exchange is the P2P xGMI path
          (parallel/oneshot.py): ONE kernel per step reduce-scatters the gradient over the
          peers' IPC-mapped buffers, runs Adadelta on this rank's 1/N slice and all-gathers the
          new weights, inside the step's hipGraph.  If any rank fails the P2P self-test, every
          rank uses RCCL all-reduce instead; config.allreduce says which path ran.  After the
          timed region the fp32 weights are checked bit-identical across ranks.

A plain run sets up, warms up, times --steps steps and prints one JSON line.  --full also measures the
Chicago-taxi wide&deep trainer (steps/sec, "chicago_taxi" in the JSON line) unless --no-taxi.
--dump-outputs DIR writes what the last timed step returned (loss, correct, count) and the fp32 weights it
left as DIR/<name>.npy (float32, rank 0); the seeds are fixed, so the same arguments give the same inputs.

Launch: python bench.py [--gpus N --steps K --warmup W --full --dump-outputs DIR].  With N > 1 and no rank environment the
script launches its own N ranks (parallel/launch.py: one process per GPU, torchrun's env contract;
refuses when fewer than N GPUs are visible unless --rehearse, which shares devices / uses the CPU
with gloo); under torch.distributed.run it is one of the ranks.  n_gpus is the size of the process
group the ranks actually formed, and config.ranks lists the device each rank drove.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    # default: the launcher's world size (torchrun without --gpus); an explicit --gpus must match it
    ap.add_argument("--gpus", type=int, default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch-per-gpu", type=int, default=int(os.environ.get("HOPSX_BENCH_BATCH", "32")))
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also measure the Chicago-taxi wide&deep trainer (a run of its own after the headline one)")
    ap.add_argument("--no-taxi", action="store_true", help="with --full: skip the taxi trainer all the same")
    ap.add_argument("--taxi-batch", type=int, default=40)  # TFX taxi trainer batch
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned and the weights it left as DIR/<name>.npy")
    ap.add_argument("--rehearse", action="store_true",
                    help="allow more ranks than GPUs (ranks share devices, gloo process group)")
    return ap.parse_args()


def timed(step_fn, n, sync_dev):
    from hops_examples_amd.parallel import dist as hdist

    cuda = sync_dev.type == "cuda"
    hdist.barrier()
    if cuda:
        torch.cuda.synchronize(sync_dev)
    t0 = time.perf_counter()
    if hasattr(step_fn, "run_n"):
        step_fn.run_n(n)  # n steps, replayed steps_per_execution at a time
    else:
        for i in range(n):
            step_fn(i)
    if cuda:
        torch.cuda.synchronize(sync_dev)
    hdist.barrier()
    el = time.perf_counter() - t0
    return hdist.all_reduce_scalar(el, "max")


def dump_outputs(path, result, model):
    """What a caller of the timed path holds after its last step, one float32 ``<name>.npy`` each: the
    step's returned loss / correct / count and every parameter as that step's update left it (fp32
    master weights, ``param.<name>``; 1.39 M values, 5.6 MB in all)."""
    import numpy as np

    os.makedirs(path, exist_ok=True)

    def f32(v):
        v = v.detach().float().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        return np.ascontiguousarray(v, dtype=np.float32)

    arrays = {k: f32(result[k]) for k in ("loss", "correct", "count") if result.get(k) is not None}
    arrays.update({f"param.{n}": f32(p) for n, p in model.named_parameters()})
    for name, arr in arrays.items():
        np.save(os.path.join(path, name + ".npy"), arr)


def main():
    a = parse()
    from hops_examples_amd.parallel import launch

    explicit = a.gpus is not None
    if not explicit:
        a.gpus = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus > 1 and not launch.is_rank_process():
        # the launcher: spawns the N ranks and never touches the GPU itself
        sys.exit(launch.launch(a.gpus, [os.path.abspath(__file__)] + sys.argv[1:], rehearse=a.rehearse))
    from hops_examples_amd.parallel import dist as hdist

    rank, local_rank, world = hdist.init()
    if world != a.gpus and explicit:
        if rank == 0:
            print(f"[bench] --gpus {a.gpus} but the process group has {world} ranks", file=sys.stderr)
        sys.exit(2)
    dev = hdist.device()
    torch.manual_seed(1234 + rank)

    from hops_examples_amd import optim
    from hops_examples_amd.models.mnist import MirroredMnistCNN, param_count
    from hops_examples_amd.runtime.arena import ParamArena

    B = a.batch_per_gpu
    model = MirroredMnistCNN().to(dev)
    nparams = param_count(model)
    ParamArena.from_module(model, dev)
    opt = optim.Adadelta(model, lr=1.0)
    from hops_examples_amd.runtime.persist import PersistentMnistStep
    from hops_examples_amd.runtime.step import make_step

    # the framework's step factory (runtime/step.py make_step): the persistent whole-step kernel (fwd, loss,
    # bwd, Adadelta of 32 steps in ONE launch; with N ranks, one per GPU, the replicas exchange inside
    # the launch over xGMI after a collective selftest) whenever it applies, else TrainStep + DataParallel
    # with 32 steps per replayed graph (Keras steps_per_execution; HOPSX_STEPS_PER_EXEC overrides)
    step = make_step(model, opt, "sparse_ce", dp="auto", batch=B, graph=not a.no_graph and dev.type == "cuda",
                     steps_per_execution=32)
    dp = getattr(step, "dp", None) if step.kind == "trainstep" else None
    persist_note = step.note

    # an MNIST-sized synthetic epoch (>= 60k images) resident in HBM, so the random
    # labels are not memorised within the timed window
    nb = max(8, -(-61440 // B))
    xs = torch.randint(0, 256, (nb, B, 28, 28, 1), dtype=torch.uint8, device=dev)
    ys = torch.randint(0, 10, (nb, B), dtype=torch.int64, device=dev)
    out = {}

    def run(i):
        # cycles through the resident epoch; in the replayed graph the optimizer kernel's tail
        # copies the next batch into the step's input buffers (no copy launch per step)
        out["r"] = step.step_resident(xs, ys)

    def run_n(n):
        out["r"] = step.run_resident(xs, ys, n)

    run.run_n = run_n
    # TrainStep runs `warmup` eager steps and captures its graph on the next one: warm up past the capture
    # (as benchmarks/run.py does), so the timed window holds replays only whatever --warmup says.  A
    # 2-rank rehearsal with --warmup 2 otherwise timed the one-step graph's capture: 13.3 ms/step over 5
    # steps vs 0.17 ms/step after 10 warm-up steps (profiles/r5_rehearsal_2rank_trace.txt)
    nwarm = a.warmup
    if step.kind == "trainstep" and getattr(step, "use_graph", False):
        nwarm = max(nwarm, step.warmup + 2)
    for i in range(nwarm):
        run(i)
    step.prepare_resident(xs, ys, n=a.steps)  # capture the steps_per_execution (+ remainder) graphs untimed
    el = timed(run, a.steps, dev)
    if isinstance(step, PersistentMnistStep):
        # the persistent engine's sticky hand-off error word (outside the timed region), agreed on by every
        # rank: a run whose in-launch exchange failed is not a measurement — the ranks fall back together to
        # the multi-kernel DP engine and time that instead (the JSON says so in persistent_note)
        if os.environ.get("HOPSX_BENCH_FAKE_PERSIST_ERR"):  # (exercises this fallback: tests/test_bench_gpu.py)
            step.err.fill_(int(os.environ["HOPSX_BENCH_FAKE_PERSIST_ERR"]))
        err = int(step.err[0].item()) & 0xFFFFFFFF
        errs = [err]
        if world > 1:
            import torch.distributed as dist

            errs = [None] * world
            dist.all_gather_object(errs, err)
        if any(errs):
            try:
                step.check()
            except Exception as e:  # (the rank's own error text, for the note)
                persist_note = f"persistent run failed ({str(e)[:160]}); timed on TrainStep instead"
            else:
                persist_note = f"a peer's persistent run failed (error words {errs}); timed on TrainStep instead"
            if world > 1:
                step.close()
            os.environ["HOPSX_PERSIST"] = "0"
            step = make_step(model, opt, "sparse_ce", dp="auto", batch=B, graph=not a.no_graph and dev.type == "cuda",
                             steps_per_execution=32)
            dp = getattr(step, "dp", None)
            for i in range(max(a.warmup, step.warmup + 2)):
                run(i)
            step.prepare_resident(xs, ys, n=a.steps)
            el = timed(run, a.steps, dev)
    loss = float(out["r"]["loss"].item())
    ms = el / a.steps * 1e3
    ips = B * world * a.steps / el
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, out["r"], model)  # (the data-parallel replicas are checked identical below)
    replicas = None
    dp_path = dp.path if dp is not None else None
    ranks = None
    if isinstance(step, PersistentMnistStep) and world > 1:
        replicas = step.verify_replicas()
        dp_path = "persistent in-kernel xGMI exchange"
        ranks = launch.gather_rank_info(dev, {"persistent_dp": True})
        step.close()
    if dp is not None:
        replicas = dp.verify_replicas()  # outside the timed region
        ranks = launch.gather_rank_info(dev, {"p2p_world": dp.p2p_world})
        dp.close()  # collective; raises if a P2P collective failed during the run

    taxi = None
    if a.full and not a.no_taxi:
        try:
            from hops_examples_amd.models.widedeep import bench_taxi

            taxi = None if dev.type != "cuda" else bench_taxi(dev, a.taxi_batch, max(200, a.steps // 2), max(5, a.warmup // 2), timed, world,
                              graph=not a.no_graph)
        except Exception as e:  # keep the headline metric even if the secondary one fails
            taxi = {"error": repr(e)[:300]}

    if rank == 0:
        rec = {
            "metric": "images/sec MNIST CNN + steps/sec Chicago-taxi DNN at 1/2/4/8 MI355X",
            "value": round(ips, 1),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(ms, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if dev.type == "cuda" else "fp32",
            "data": "synthetic (a 60k-image uint8 28x28 epoch + labels resident in HBM, next batch prefetched "
                    "by the optimizer kernel), random-init weights",
            "config": {
                "model": f"MNIST CNN (experiment.mirrored model, {nparams} params), Adadelta(1.0)",
                "global_batch": B * world,
                "per_gpu_batch": B,
                "seq_len": None,
                "parallelism": f"dp{world}",
                "engine": type(step).__name__,
                "hipgraph": step.use_graph,
                "steps_per_execution": step.steps_per_execution if getattr(step, "_gU", True) is not None else 1,
                "allreduce": dp_path,
                "wire_bytes_per_param": None if dp is None else dp.wire_bytes_per_param,
                "persistent_note": persist_note,
                "ranks": ranks,
                "warmup_steps_run": nwarm,
            },
            "replicas_identical": None if replicas is None else replicas["identical"],
            "final_loss": round(loss, 4),
            "chicago_taxi": taxi,
        }
        print(json.dumps(rec), flush=True)
    hdist.shutdown()
    from hops_examples_amd.parallel import launch

    launch.rank_exit(0)  # a finished rank of the self-launch skips interpreter teardown (see launch.rank_exit)


if __name__ == "__main__":
    main()
