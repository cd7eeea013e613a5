"""tools/kt_dispatch.py KT_DIR KERNEL_REGEX OUT.csv — the per-dispatch durations of a kernel family
from a rocprofv3 --kernel-trace run (tools/profile.sh's kt pass): one row per dispatch in start
order — launch index within the family, kernel (its k_* name and template arguments), microseconds.
The counterpart of prof_summary.py --csv, which keeps the per-dispatch counters."""
import csv
import glob
import os
import re
import sys


def main():
    d, pat, out = sys.argv[1], re.compile(sys.argv[2]), sys.argv[3]
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if pat.search(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    with open(out, "w", newline="") as g:
        w = csv.writer(g)
        w.writerow(["launch", "kernel", "us"])
        for i, r in enumerate(rows):
            m = re.search(r"(k_\w+(<[^>]*>)?)", r["Kernel_Name"])
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            w.writerow([i, m.group(1) if m else r["Kernel_Name"][:60], f"{us:.1f}"])
    total = sum((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows) / 1e6
    print(f"wrote {out}: {len(rows)} dispatches, {total:.3f} ms")


if __name__ == "__main__":
    main()
