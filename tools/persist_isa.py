"""Static instruction table of the position workgroups' local compute in the persistent flagship step
(csrc/ops/mnist_persist.hip): compiles the file to gfx950 assembly with the build's flags (no GPU needed), cuts
the step loop of position_wg at its s_barriers and prints, per compute segment, the VALU / LDS / s_waitcnt / MFMA
instruction counts and how many of the waits are a full `lgkmcnt(0)` — for mnist_persist_k<false> and <true>.
One wave per SIMD runs this code, so every wait placed right behind its LDS read exposes the read's latency:
the s_waitcnt column is what "keep the LDS reads in flight" lowers.

usage: python tools/persist_isa.py [--src FILE] [--keep-asm OUT.s] [--resources]"""
import argparse
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kernel_asm import compile_asm  # noqa: E402  (the one compile command line)

# the MFMA-carrying segments of one step, in program order (DP: the replica-order fc1 weight gradient follows)
NAMES = ["conv2 + bias/relu/pool/dropout epilogue", "fc1 partial product", "fc1 dgrad + pool backward",
         "conv2 weight gradient", "publish C part 1 + conv2 dgrad + fc1 wgrad + col2im + conv1 wgrad",
         "fc1 wgrad over the replicas + fc1 Adadelta (DP)"]


def instructions(body):
    for line in body.split("\n"):
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            yield t


def count(seg):
    c = dict(valu=0, pk=0, acc=0, lds=0, wait=0, wait0=0, mfma=0)
    for t in seg:
        op = t.split()[0]
        if "mfma" in op:
            c["mfma"] += 1
        elif op.startswith("v_accvgpr"):
            c["acc"] += 1
        elif op.startswith("v_pk_"):
            c["pk"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op == "s_waitcnt":
            c["wait"] += 1
            c["wait0"] += "lgkmcnt(0)" in t
    return c


def segments(asm, kernel):
    """[(name, counts)] of the compute segments of position_wg's step loop in `kernel` (a mangled-name
    substring).  The loop opens at the opaque zero (`v_mov_b32 vN, 0` inside an asm statement)."""
    m = re.search(r"^(_Z\w*" + re.escape(kernel) + r"\w*):", asm, re.M)
    if not m:
        sys.exit(f"no kernel matching {kernel}")
    body = asm[m.end():asm.find(".Lfunc_end", m.end())]
    top = re.search(r";;#ASMSTART\s*\n\s*v_mov_b32 v\d+, 0\s*\n\s*;;#ASMEND", body)
    if not top:
        sys.exit("step loop marker (the opaque zero) not found")
    segs, cur = [], []
    for t in instructions(body[top.end():]):
        if t.split()[0] == "s_barrier":
            segs.append(cur)
            cur = []
        else:
            cur.append(t)
    cs = [count(s) for s in segs]
    first = next(i for i, c in enumerate(cs) if c["mfma"])
    out = [("conv1", cs[first - 1])]
    names = iter(NAMES)
    for c in cs[first:]:
        if c["mfma"]:
            n = next(names, None)
            if n is None:
                break
            out.append((n, c))
    return out


def table(asm, kernel, title):
    print(f"== {title}")
    print(f"  {'segment':<68}{'VALU':>6}{'+pk':>5}{'+acc':>5}{'LDS':>6}{'waitcnt':>9}{'lgkm(0)':>9}{'MFMA':>6}")
    tot = dict(valu=0, pk=0, acc=0, lds=0, wait=0, wait0=0, mfma=0)
    for n, c in segments(asm, kernel):
        if n.endswith("(DP)"):
            print(f"  {n:<68}{c['valu']:>6}{c['pk']:>5}{c['acc']:>5}{c['lds']:>6}{c['wait']:>9}{c['wait0']:>9}{c['mfma']:>6}")
            continue
        for k in tot:
            tot[k] += c[k]
        print(f"  {n:<68}{c['valu']:>6}{c['pk']:>5}{c['acc']:>5}{c['lds']:>6}{c['wait']:>9}{c['wait0']:>9}{c['mfma']:>6}")
    n = "the six segments"
    print(f"  {n:<68}{tot['valu']:>6}{tot['pk']:>5}{tot['acc']:>5}{tot['lds']:>6}{tot['wait']:>9}{tot['wait0']:>9}{tot['mfma']:>6}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "csrc", "ops", "mnist_persist.hip"))
    ap.add_argument("--keep-asm", default=None, help="write the assembly here")
    ap.add_argument("--resources", action="store_true", help="also print the compiler's resource-usage remarks")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        out = a.keep_asm or os.path.join(d, "mnist_persist.s")
        log = compile_asm(a.src, out, a.resources)
        asm = open(out).read()
    table(asm, "mnist_persist_kILb0E", "mnist_persist_k<false>")
    table(asm, "mnist_persist_kILb1E", "mnist_persist_k<true>")
    if a.resources:
        for ln in log.splitlines():
            mm = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill)(.*?)\s*\[-R", ln)
            if mm and "mnist_persist_k" in (mm.group(2) if mm.group(1) == "Function Name" else "mnist_persist_k"):
                print(("" if mm.group(1) == "Function Name" else "    ") + mm.group(1) + mm.group(2))


if __name__ == "__main__":
    main()
