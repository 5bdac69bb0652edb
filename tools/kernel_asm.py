"""Per-kernel assembly comparison of the working tree against a base revision (no GPU needed): compiles each
.hip file to gfx950 assembly with the build's flags, once from the working tree and once from `git archive REV
csrc/ops` unpacked into a temporary directory, cuts both texts per kernel symbol (`_Z...:` to `.Lfunc_end`),
drops comments and .loc / .file lines, and prints `identical` or `DIFFERENT (n lines)` per kernel with the first
differing lines.  Exits non-zero on any difference.  It compares texts; it looks for no particular instruction.
A refactor that only moves definitions must leave every kernel identical.

`--normalize`, for a change that ADDS template instantiations or a trailing template flag to a kernel:
  * function-local labels `.LBB<n>_<m>` carry the number of the function within its file, which moves when
    instantiations are added before it: they are compared as `.LBB_<m>`;
  * a kernel of the base that is missing from the working tree is paired with the tree's kernel of the same
    template whose arguments are the base's plus one trailing `false` (a new flag, off); the pair is compared
    as one kernel and named `A == B`.  Whatever else differs (a longer argument list: kernarg size, offsets of
    the hidden arguments) is still reported line by line.

usage: python tools/kernel_asm.py [--base REV] [--show N] [--normalize] [FILE.hip ...]"""
import argparse
import concurrent.futures as cf
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = os.path.join("csrc", "ops")
DEFAULT = ["mnist_persist.hip", "mnist_eval.hip", "taxi_step.hip", "taxi_eval.hip"]


def compile_asm(src, out, resources=False, defines=()):
    """`src` to gfx950 assembly at `out` with the build's flags; returns the compiler's output (the
    resource-usage remarks with `resources`).  The one place the command line is spelled."""
    from hops_examples_amd import _build

    cmd = [_build.HIPCC, *_build.HIP_FLAGS, *defines, *_build._py_includes(), f"-I{os.path.dirname(src)}",
           "--cuda-device-only", "-S", src, "-o", out]
    if resources:
        cmd.append("-Rpass-analysis=kernel-resource-usage")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit("compile failed:\n" + " ".join(cmd) + "\n" + r.stdout)
    return r.stdout


def kernels(asm):
    """{kernel symbol: [instruction and directive lines]} of the `.amdhsa_kernel` symbols of an assembly text."""
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        m = re.search(r"^" + re.escape(name) + r":", asm, re.M)
        body = asm[m.end():asm.find(".Lfunc_end", m.end())]
        lines = []
        for ln in body.split("\n"):
            t = ln.split(";")[0].strip()
            if t and not t.startswith((".loc", ".file")):
                lines.append(t)
        out[name] = lines
    return out


def demangled(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    short = [re.sub(r"\((?!anonymous namespace).*", "", s) for s in r.stdout.split("\n")]
    return dict(zip(names, short)) if r.returncode == 0 and len(short) >= len(names) else {n: n for n in names}


def unlabel(lines):
    return [re.sub(r"\.LBB\d+_", ".LBB_", ln) for ln in lines]


def pair_trailing_flag(base, tree):
    """Renames tree kernels `k<args, false>` to the base symbol `k<args>` that the tree no longer has; returns
    {base symbol: tree symbol} of the pairs made."""
    gone = [s for s in base if s not in tree]
    new = [s for s in tree if s not in base]
    full = lambda names: dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE,
                                                        text=True).stdout.split("\n")))
    dg, dn = full(gone), full(new)
    tmpl = lambda d: re.match(r"(.*?<)(.*)(>\(.*)", d)  # (head<, template args, >(parameters...)
    by_args = {}
    for s in new:
        m = tmpl(dn.get(s, ""))
        if m and m.group(2).endswith(", false"):
            by_args[m.group(1) + m.group(2)[:-len(", false")]] = s
    pairs = {}
    for s in gone:
        m = tmpl(dg.get(s, ""))
        t = by_args.get(m.group(1) + m.group(2)) if m else None
        if t is not None:
            pairs[s] = t
            tree[s] = [ln.replace(t, s) for ln in tree.pop(t)]
    return pairs


def base_tree(rev, into):
    """`rev`'s csrc/ops unpacked under `into`; returns the directory."""
    r = subprocess.run(["git", "-C", ROOT, "archive", rev, OPS.replace(os.sep, "/")], stdout=subprocess.PIPE)
    if r.returncode != 0:
        sys.exit(f"git archive {rev} failed")
    tarfile.open(fileobj=io.BytesIO(r.stdout)).extractall(into)
    return os.path.join(into, OPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*", default=DEFAULT, help="file names under csrc/ops")
    ap.add_argument("--base", default="HEAD", help="revision to compare the working tree against")
    ap.add_argument("--show", type=int, default=6, help="differing lines printed per kernel")
    ap.add_argument("--normalize", action="store_true", help="ignore label numbering, pair kernels that gained a "
                    "trailing template flag (see above)")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        base = base_tree(a.base, d)
        jobs = {}
        with cf.ThreadPoolExecutor(max_workers=min(8, 2 * len(a.files))) as ex:
            for f in a.files:
                f = os.path.basename(f)
                for side, srcdir in (("base", base), ("tree", os.path.join(ROOT, OPS))):
                    out = os.path.join(d, f"{side}_{f}.s")
                    jobs[f, side] = (ex.submit(compile_asm, os.path.join(srcdir, f), out), out)
        for f in dict.fromkeys(os.path.basename(f) for f in a.files):
            texts = {}
            for side in ("base", "tree"):
                fut, out = jobs[f, side]
                fut.result()
                texts[side] = kernels(open(out).read())
            pairs = pair_trailing_flag(texts["base"], texts["tree"]) if a.normalize else {}
            names = demangled(sorted(set(texts["base"]) | set(texts["tree"])))
            print(f"== {f}  ({a.base} -> working tree)" + (f"  [normalized; {len(pairs)} kernels paired with their "
                                                            "<..., false> successor]" if a.normalize else ""))
            for sym, nice in names.items():
                b, t = texts["base"].get(sym), texts["tree"].get(sym)
                if a.normalize and b is not None and t is not None:
                    b, t = unlabel(b), unlabel(t)
                if b is None or t is None:
                    bad += 1
                    print(f"  {nice:<64} only in the {'working tree' if b is None else 'base'}")
                elif b == t:
                    print(f"  {nice:<64} identical ({len(t)} lines)")
                else:
                    bad += 1
                    diff = [ln for ln in difflib.unified_diff(b, t, "base", "tree", lineterm="", n=0)
                            if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
                    print(f"  {nice:<64} DIFFERENT ({len(diff)} lines)")
                    for ln in diff[:a.show]:
                        print("      " + ln)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
