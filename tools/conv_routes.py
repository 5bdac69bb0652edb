"""Which kernels the conv launchers run, case by case: the record a change to the launchers' routing is held to.

    python tools/conv_routes.py [--only GROUP]       (GPU) every launcher once over table() on CPU-seeded operands:
                                                     one line per (case, launcher) with the return code and the
                                                     SHA-256 of the output bytes
    python tools/conv_routes.py --join LOG TRACE.csv the kernels (name with template arguments, grid) of a
                                                     `rocprofv3 --kernel-trace --output-format csv` run of the
                                                     above behind each of its lines
    python tools/conv_routes.py --diff A B           two joined files: return codes, kernel lists and, for launches
                                                     without a split-K ticket kernel (fp32 atomics in arrival
                                                     order), output hashes must be equal; then the counts per engine

The run launches a one-element fp64 fill before every launcher call; the join cuts the trace there, so every other
kernel between two marks belongs to that call (operands are made on the CPU and copied, hashes are taken on the
CPU: neither launches a kernel).  Run it per setting: default, HOPSX_DETERMINISTIC=1, HOPSX_DISABLE=gg."""
import argparse
import csv
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# (B, H, C, CO, k, stride, pad); square images
R50 = [(224, 8, 64, 7, 2)]  # the stem on its 8-channel padded input; bench_wgrad.LAYERS follow in table()
R20 = [(32, 8, 16, 3, 1), (32, 16, 16, 3, 1), (32, 16, 32, 3, 2), (32, 16, 32, 1, 2), (16, 32, 32, 3, 1),
       (16, 32, 64, 3, 2), (16, 32, 64, 1, 2), (8, 64, 64, 3, 1)]
MNIST = [(28, 1, 32, 2), (27, 32, 64, 2), (28, 1, 32, 4), (25, 32, 64, 4)]  # E3 (2x2), E1 (4x4): unpadded
FROZEN = [(1, 5, 16, 16, 3, 1), (1, 5, 32, 32, 3, 1), (1, 5, 256, 64, 1, 1), (2, 5, 64, 40, 1, 1), (1, 63, 64, 64, 3, 1),
          (1, 44, 64, 256, 1, 1), (2, 7, 512, 512, 3, 1)]  # tests/test_frozen_resnet_gpu.py CASES
SPLITK = [(8, 7, 512, 512, 3, 1), (2, 7, 512, 512, 3, 1), (8, 14, 256, 256, 3, 2)]  # tests/test_conv_splitk_gpu.py SHAPES
# the geometries of tests/test_conv_routes_gpu.py that the groups above do not have: the direct input-layer kernel,
# dgrad's parity-class GEMMs, its 1x1 strided scatter (with HOPSX_DISABLE=dgrad_par; else parity), its dense 1x1,
# a BN-statistics forward on gemm_core.h's engine
ROUTES = [(1, 6, 1, 32, 3, 1), (1, 44, 256, 16, 3, 2), (1, 88, 256, 64, 1, 2), (1, 44, 256, 64, 1, 1), (1, 5, 64, 64, 3, 1)]
LAUNCHERS = ("fwd", "fwd_colsum", "fwd_f32", "fwd_res", "fwd_bnstats", "dgrad", "dgrad_y", "dgrad_addend", "dgrad_colsum",
             "dgrad_bn")
MARK = "FillFunctor<double>"


def table():
    from bench_wgrad import LAYERS

    t = []
    for B in (8, 64):
        t += [(f"r50_b{B}", B, H, C, CO, k, s, k // 2, 0) for (H, C, CO, k, s) in R50 + [l[:5] for l in LAYERS]]
    t += [("r20_b128", 128, H, C, CO, k, s, k // 2, 0) for (H, C, CO, k, s) in R20]
    t += [("mnist_b32", 32, H, C, CO, k, 1, 0, 0) for (H, C, CO, k) in MNIST]
    t += [("frozen", B, H, C, CO, k, s, k // 2, 0) for (B, H, C, CO, k, s) in FROZEN]
    t += [("splitk", B, H, C, CO, k, s, k // 2, 0) for (B, H, C, CO, k, s) in SPLITK]
    t += [("routes", B, H, C, CO, k, s, k // 2, 0) for (B, H, C, CO, k, s) in ROUTES]
    t += [("x_off8", 1, 63, 64, 64, 3, 1, 1, 4)]  # x four bf16 elements (8 bytes) into its buffer
    return t


def run(only=None):
    import torch

    from hops_examples_amd.ops import kernels as K

    dev, bf = torch.device("cuda", 0), torch.bfloat16
    mark = torch.empty(1, device=dev, dtype=torch.float64)  # (empty: zeros would be a first, unpaired mark)
    # every operand is a window of one pool of CPU-seeded normal values (windows start at multiples of 8 elements)
    gen = torch.Generator().manual_seed(20)
    pool = torch.randn(1 << 26, generator=gen).to(bf).to(dev)
    fpool = torch.randn(1 << 12, generator=gen).to(dev)
    fpos = (torch.randn(1 << 10, generator=gen).abs() + 0.5).to(dev)

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]

    for (tag, B, H, C, CO, k, s, pad, xoff) in table():
        if only and tag != only:
            continue
        name = f"{tag}:{B}x{H}x{H}x{C}->{CO} k{k} s{s} p{pad}" + (f" x+{2 * xoff}B" if xoff else "")
        at = [8 * sum(map(ord, name))]

        def rnd(*sh):
            n = 1
            for v in sh:
                n *= v
            at[0] = (at[0] * 3 + 4096) % ((1 << 26) - n) // 8 * 8
            return pool[at[0]:at[0] + n].view(*sh)

        geom = K.conv_geom((B, H, H, C), (CO, k, k, C), (s, s), (pad, pad), (1, 1))
        OH, OW = geom[4], geom[5]
        xbuf = rnd(B * H * H * C + 8)
        x = xbuf[xoff:xoff + B * H * H * C].view(B, H, H, C)
        w = rnd(CO, k, k, C)
        dy, y, res = rnd(B, OH, OW, CO), rnd(B, OH, OW, CO), rnd(B, OH, OW, CO)
        add, z = rnd(B, H, H, C), rnd(B, H, H, C)
        bias, mean, rstd = fpool[:CO], fpool[2048:2048 + C], fpos[:C]
        acc_n = K.BN_NREP * 2 * C + 12 * 32  # kernels.bn_acc's layout
        calls = {
            "fwd": lambda: K.conv2d_fwd(x, w, geom, bias=bias, act=1),
            "fwd_colsum": lambda: K.conv2d_fwd(x, w, geom, bias=bias, act=1, colsum=torch.zeros(CO, device=dev)),
            "fwd_f32": lambda: K.conv2d_fwd(x, w, geom, bias=bias, act=1,
                                            out=torch.empty(B, OH, OW, CO, device=dev, dtype=torch.float32)),
            "fwd_res": lambda: K.conv2d_fwd_res(x, w, geom, bias=bias, act=1, residual=res),
            "fwd_bnstats": lambda: K.conv2d_fwd_bnstats(x, w, geom),
            "dgrad": lambda: K.conv2d_dgrad(dy, w, geom),
            "dgrad_y": lambda: K.conv2d_dgrad(dy, w, geom, y=y, act=1),
            "dgrad_addend": lambda: K.conv2d_dgrad(dy, w, geom, addend=add),
            "dgrad_colsum": lambda: K.conv2d_dgrad(dy, w, geom, yprev=x, act_prev=1, colsum=torch.zeros(C, device=dev)),
            "dgrad_bn": lambda: K.conv2d_dgrad_bn(dy, w, geom, (z, mean, rstd, x, 1, torch.zeros(acc_n, device=dev)),
                                                  addend=add),
        }
        for ln in LAUNCHERS:
            mark.fill_(1.0)
            try:
                out = calls[ln]()
                rc = "0" if torch.is_tensor(out) else "-2"  # (the wrappers turn the -2 refusal into None / False)
            except (RuntimeError, ValueError) as e:
                m = re.search(r"-?\d+", str(e))
                out, rc = None, (m.group(0) if m else "error") + f" ({str(e)[:60]})"
            torch.cuda.synchronize()
            print(f"CASE {name} | {ln} | rc {rc} | sha {sha(out) if torch.is_tensor(out) else '-'}", flush=True)
            if ln == "fwd_bnstats":
                K.bn_acc(dev, CO).zero_()  # (back at rest for the next case of this width)


def join(log, trace):
    rows = list(csv.DictReader(open(trace)))
    order = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"  # (one stream: the launch order)
    rows.sort(key=lambda r: int(r[order]))
    gcols = [c for c in rows[0] if c.startswith("Grid_Size")]
    groups, cur = [], None
    for r in rows:
        if MARK in r["Kernel_Name"]:
            cur = []
            groups.append(cur)
        elif cur is not None and "FillFunctor" not in r["Kernel_Name"]:  # (the zeroed accumulators and column sums)
            cur.append(f"{r['Kernel_Name']} grid {'x'.join(r[c] for c in gcols)}")
    cases = [ln.rstrip("\n") for ln in open(log) if ln.startswith("CASE ")]
    if len(cases) != len(groups):
        sys.exit(f"{len(cases)} CASE lines, {len(groups)} marks in the trace")
    for c, g in zip(cases, groups):
        print(c)
        for kname in g:
            print("    " + kname)


def engine(kernels):
    if not kernels:
        return "refused"
    s = " ".join(kernels)
    for pat, name in (("dgrad_par_fill_k", "gg_par"), ("EpiDgradPar", "gg_par"), ("EpiDgradScatter", "gg_scatter"),
                      ("EpiAtomicTicket", "splitk"), ("GgDgradA", "gg_gather"), ("GgWeightT", "gg_dense"),
                      ("gg_kernel", "gg"), ("conv_direct_fwd_k", "direct"),
                      ("_mfma_k", "mfma")):
        if pat in s:
            return name
    return "gemm"


def parse(path):
    out, cur = [], None
    for ln in open(path):
        if ln.startswith("CASE "):
            case, launcher, rc, h = [p.strip() for p in ln[5:].split("|")]
            cur = {"key": f"{case} | {launcher}", "rc": rc, "sha": h, "kernels": []}
            out.append(cur)
        elif ln.startswith("    ") and cur is not None:
            cur["kernels"].append(ln.strip())
    return out


def diff(a, b):
    A, B = parse(a), parse(b)
    bad = 0
    if [r["key"] for r in A] != [r["key"] for r in B]:
        sys.exit("the two files list different cases")
    counts, loose = {}, 0
    for ra, rb in zip(A, B):
        e = engine(ra["kernels"])
        kind = ra["key"].split("|")[1].strip()
        counts.setdefault(kind, {}).setdefault(e, 0)
        counts[kind][e] += 1
        atomic = any("EpiAtomicTicket" in kn for kn in ra["kernels"] + rb["kernels"])
        loose += atomic
        what = [n for n, same in (("rc", ra["rc"] == rb["rc"]), ("kernels", ra["kernels"] == rb["kernels"]),
                                  ("sha", atomic or ra["sha"] == rb["sha"])) if not same]
        if what:
            bad += 1
            print(f"DIFFERENT {'/'.join(what)}: {ra['key']}\n  A rc {ra['rc']} sha {ra['sha']} {ra['kernels']}\n"
                  f"  B rc {rb['rc']} sha {rb['sha']} {rb['kernels']}")
    print(f"{len(A)} launches: {len(A) - bad} with equal return code, kernel list (name, grid) and output hash, "
          f"{bad} different; {loose} split-K launches compared without the hash")
    for kind in LAUNCHERS:
        print(f"  {kind:<13}" + "  ".join(f"{e} {n}" for e, n in sorted(counts.get(kind, {}).items())))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--join", nargs=2, metavar=("LOG", "TRACE_CSV"))
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("--only", help="run one group of the table (r50_b8, r50_b64, r20_b128, mnist_b32, frozen, splitk, "
                    "routes, x_off8)")
    a = ap.parse_args()
    if a.join:
        join(*a.join)
    elif a.diff:
        diff(*a.diff)
    else:
        run(a.only)
