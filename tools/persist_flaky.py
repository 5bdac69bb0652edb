"""How often do five persistent flagship steps leave other bits than the parent's golden file?  Repeats the run of
tools/persist_bits.py N times per knob setting and instantiation (one process, loopback 2), alternating the two dropout
cases, and counts the runs whose per-tensor digests differ from tests/golden/persist_parent_conv_bits.json.

A build whose schedule keeps every float operation's operands and order differs in 0 of N.  The count is the tool
for a build that does NOT: the bit-equality tests of the persistent step compare single runs, so a run-to-run
difference shows there as a sporadic failure of whichever case happened to hit it
(profiles/r18_persist_head_chain.txt: the build of commit 8c11b67 differed in 1 of 80 runs).

usage (GPU): python tools/persist_flaky.py [--plan 1 2 2] [--runs 40] ["GATE_A=0,HEAD_CHAIN=0" ...]
             (a setting is a comma-separated list of HOPSX_PERSIST_ knobs without the prefix; none: the defaults)

--plan: the five steps cut into these launches instead of the golden file's 3 + 2.  The state written back between
launches is exact, so the digests are the golden file's for every plan of five steps; the count of distinct digest
sets per line is printed with it (1 when no run differs)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import persist_bits  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("settings", nargs="*", default=[""])
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--plan", type=int, nargs="+", default=list(persist_bits.LAUNCHES), help="steps per launch, 5 in all")
    a = ap.parse_args()
    from hops_examples_amd.runtime import persist

    with open(persist_bits.GOLDEN_TENSORS) as f:
        golden = json.load(f)["digests"]
    cases = list(persist_bits.CASES)
    assert sum(a.plan) == sum(persist_bits.LAUNCHES), "the golden digests are those of five steps"
    persist_bits.LAUNCHES = tuple(a.plan)
    for s in a.settings or [""]:
        knobs = dict(kv.split("=", 1) for kv in s.split(",") if kv)
        for k, v in knobs.items():
            os.environ["HOPSX_PERSIST_" + k] = v
        persist._ext().mnist_persist_reload_knobs()  # the host wrapper caches the knobs otherwise
        for wn, lb in persist_bits.WORLDS.items():
            bad, sets = [], set()
            for r in range(a.runs):
                case = cases[r % len(cases)]
                d = persist_bits.digests(persist_bits.CASES[case], loopback=lb, per_tensor=True)
                nb = sum(d[k] != golden[wn][case][k] for k in d)
                sets.add((case, tuple(sorted(d.items()))))
                if nb:
                    bad.append((r, case, nb))
            print(f"[{s or 'defaults'}] {wn}: {len(bad)} of {a.runs} runs differ from the golden file {bad[:6]}"
                  f" (plan {'+'.join(map(str, a.plan))}, {len(sets)} distinct digest sets over {len(cases)} cases)", flush=True)
        for k in knobs:
            os.environ.pop("HOPSX_PERSIST_" + k, None)
    persist._ext().mnist_persist_reload_knobs()


if __name__ == "__main__":
    main()
