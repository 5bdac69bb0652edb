"""Static instruction table of the position workgroups' local compute in the persistent flagship step
(csrc/ops/mnist_persist.hip): compiles the file to gfx950 assembly with the build's flags (no GPU needed), cuts
the step loop of position_wg at its s_barriers and wave-level ordering points and prints, per compute segment, the
VALU / LDS / s_waitcnt / MFMA instruction counts, how many of the waits are a full `lgkmcnt(0)`, and which of the two
stands in front of the segment (`barrier`) — for mnist_persist_k<false> and <true>, once per path of
HOPSX_PERSIST_WLOCAL (the default and 0: compiled with -DHOPSX_PERSIST_WLOCAL_FIXED, so that each text holds one path).
One wave per SIMD runs this code, so every wait placed right behind its LDS read exposes the read's latency:
the s_waitcnt column is what "keep the LDS reads in flight" lowers.

usage: python tools/persist_isa.py [--src FILE] [--keep-asm OUT.s] [--resources]"""
import argparse
import concurrent.futures as cf
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
# segments without MFMAs behind a wave-level ordering point, in program order.  The read-back of A stood in a
# segment of its own before too (not a row, not in the total); that of C's part 1 was part of the row after it
WAVE_NAMES = ["publish A: the wave's read-back + stores (not in the total)", "publish C part 1: the wave's read-back + stores"]


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
    # A segment lies between two ordering points: an s_barrier ("wg") or the wave-level ordering point that stands
    # for one where producer and consumer are the same wave (wave_lds_order: an `s_waitcnt lgkmcnt(0)` inside an asm
    # statement, "wave").  Rows: conv1 (the segment in front of the first MFMA), every segment with MFMAs, and every
    # segment without MFMAs that a wave-level point opens (a wave's read-back of its own staged block), in program order
    segs, cur, kind, in_asm = [], [], "wg", False
    for line in body[top.end():].split("\n"):
        if "#ASMSTART" in line or "#ASMEND" in line:
            in_asm = "#ASMSTART" in line
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        cut = "wg" if t.split()[0] == "s_barrier" else "wave" if in_asm and t == "s_waitcnt lgkmcnt(0)" else None
        if cut is None:
            cur.append(t)
        else:
            segs.append((kind, count(cur)))
            cur, kind = [], cut
    first = next(i for i, (k, c) in enumerate(segs) if c["mfma"])
    out = [("conv1", segs[first - 1])]
    names, wnames = iter(NAMES), iter(WAVE_NAMES)
    for k, c in segs[first:]:
        n = next(names, None) if c["mfma"] else next(wnames, None) if k == "wave" else ""
        if n is None and c["mfma"]:
            break
        if n:
            out.append((n, (k, c)))
    return [(n, dict(c, barrier=k)) for n, (k, c) in out]


def table(asm, kernel, title):
    print(f"== {title}")
    # barrier: what stands in front of the segment: wg an s_barrier, wave the wave-level ordering point
    print(f"  {'segment':<68}{'VALU':>6}{'+pk':>5}{'+acc':>5}{'LDS':>6}{'waitcnt':>9}{'lgkm(0)':>9}{'MFMA':>6}  barrier")
    tot = dict(valu=0, pk=0, acc=0, lds=0, wait=0, wait0=0, mfma=0)
    for n, c in segments(asm, kernel):
        row = (f"  {n:<68}{c['valu']:>6}{c['pk']:>5}{c['acc']:>5}{c['lds']:>6}{c['wait']:>9}{c['wait0']:>9}{c['mfma']:>6}"
               f"  {c['barrier']}")
        print(row)
        if n.endswith("(DP)") or n.endswith("(not in the total)"):
            continue
        for k in tot:
            tot[k] += c[k]
    n = "total"
    print(f"  {n:<68}{tot['valu']:>6}{tot['pk']:>5}{tot['acc']:>5}{tot['lds']:>6}{tot['wait']:>9}{tot['wait0']:>9}{tot['mfma']:>6}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "csrc", "ops", "mnist_persist.hip"))
    ap.add_argument("--keep-asm", default=None, help="write the assembly here")
    ap.add_argument("--resources", action="store_true", help="also print the compiler's resource-usage remarks")
    a = ap.parse_args()
    # one compile per path of HOPSX_PERSIST_WLOCAL (fixed at compile time: one arm of every branch on it in the text),
    # and the build's own text (the knob read at run time) for the resources
    paths = {"7": "HOPSX_PERSIST_WLOCAL=7 (the default)", "0": "HOPSX_PERSIST_WLOCAL=0"}
    with tempfile.TemporaryDirectory() as d, cf.ThreadPoolExecutor(max_workers=3) as ex:
        jobs = {v: ex.submit(compile_asm, a.src, os.path.join(d, f"wl{v}.s"), False, [f"-DHOPSX_PERSIST_WLOCAL_FIXED={v}"])
                for v in paths}
        out = a.keep_asm or os.path.join(d, "mnist_persist.s")
        log = ex.submit(compile_asm, a.src, out, True).result() if a.resources or a.keep_asm else ""
        for v, title in paths.items():
            jobs[v].result()
            asm = open(os.path.join(d, f"wl{v}.s")).read()
            table(asm, "mnist_persist_kILb0E", f"mnist_persist_k<false>, {title}")
            table(asm, "mnist_persist_kILb1E", f"mnist_persist_k<true>, {title}")
    if a.resources:
        for ln in log.splitlines():
            mm = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill)(.*?)\s*\[-R", ln)
            if mm and "mnist_persist_k" in (mm.group(2) if mm.group(1) == "Function Name" else "mnist_persist_k"):
                print(("" if mm.group(1) == "Function Name" else "    ") + mm.group(1) + mm.group(2))


if __name__ == "__main__":
    main()
