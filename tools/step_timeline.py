"""Timeline of the training step from one `rocprofv3 --kernel-trace --output-format csv` run of
`bench.py --steps 200`: per kernel of the step its duration, the gap from its end to the next kernel's
start, and the step period (fused start to fused start) -- medians over the steady-state steps with
min and max. Shows whether time between kernels sits in gaps or inside the durations.

  python tools/step_timeline.py <dir or *kernel_trace.csv> [--skip 20] [--label NAME]
"""
import argparse
import csv
import glob
import os
import statistics
import sys

# the step's kernels in launch order (name prefixes of the demangled names)
STEP = ("k_fused_train_grid", "k_grid_bwd_lds", "k_adam")


def short(name):
    """`void tcnn_amd::k_adam<...>(...)` or `_ZN8tcnn_amd6k_adamE...` (long names stay mangled) -> `k_adam`"""
    if name.startswith("_ZN"):  # nested name: <length><component> ..., the last component is the function
        i, last = 3, name
        while i < len(name) and name[i].isdigit():
            j = i
            while name[j].isdigit():
                j += 1
            n = int(name[i:j])
            last, i = name[j:j + n], j + n
        return last
    n = name.split("(")[0].split("<")[0].split()
    n = n[-1] if n else name
    n = n.split("::")[-1]
    return n[:-3] if n.endswith(".kd") else n


def load(path):
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            sys.exit(f"no *kernel_trace.csv under {path}")
        path = found[0]
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    return path, rows


def steps_of(rows):
    """the runs fused, grid backward, Adam with no other dispatch between them: [(start, end) x 3]"""
    out = []
    i = 0
    while i + len(STEP) <= len(rows):
        if all(rows[i + k][2] == STEP[k] for k in range(len(STEP))):
            out.append([rows[i + k][:2] for k in range(len(STEP))])
            i += len(STEP)
        else:
            i += 1
    return out


def stat(v):
    return f"median {statistics.median(v) / 1e3:7.2f}  min {min(v) / 1e3:7.2f}  max {max(v) / 1e3:7.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip", type=int, default=20, help="leading steps left out (warm-up)")
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    path, rows = load(a.trace)
    st = steps_of(rows)[a.skip:]
    if len(st) < 2:
        sys.exit(f"{path}: {len(st)} steady-state steps found")
    print(f"# {a.label or path}: {len(st)} steps (us)")
    for k, name in enumerate(STEP):
        print(f"{name:20s} duration  {stat([s[k][1] - s[k][0] for s in st])}")
        if k + 1 < len(STEP):
            print(f"{'  -> ' + STEP[k + 1]:20s} gap       {stat([s[k + 1][0] - s[k][1] for s in st])}")
    # the step-to-step figures only between steps that follow each other directly (no foreign kernel
    # of more than the step's own between them would go unnoticed: its time shows in the gap's max)
    nxt = list(zip(st[:-1], st[1:]))
    print(f"{'  -> next step':20s} gap       {stat([b[0][0] - a_[-1][1] for a_, b in nxt])}")
    print(f"{'step period':20s}           {stat([b[0][0] - a_[0][0] for a_, b in nxt])}")
    print(f"{'sum of durations':20s}           {stat([sum(e - s for s, e in x) for x in st])}")


if __name__ == "__main__":
    main()
