"""Per-level medians of the search and recheck kernels over every quantize in a rocprofv3 kernel trace
(quantizes split at each mean_sums launch, levels at each search launch).

    python tools/level_medians.py TRACE.csv [TRACE.csv ...]

One line per trace: the search kernels' median us by level, then the rechecks' (every recheck
kernel between two searches summed), then the median of the quantizes' search totals.
"""
import csv
import statistics
import sys


def quantizes(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out, cur = [], None
    for r in rows:
        n = r["Kernel_Name"]
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "mean_sums" in n:
            cur = []
            out.append(cur)
        elif cur is None:
            continue
        elif "assign_" in n:
            cur.append([d, 0.0])
        elif "recheck" in n and cur:
            cur[-1][1] += d
    return out


def main():
    for path in sys.argv[1:]:
        q = quantizes(path)
        nlev = statistics.mode(len(x) for x in q)
        q = [x for x in q if len(x) == nlev]
        s = [statistics.median(x[i][0] for x in q) for i in range(nlev)]
        r = [statistics.median(x[i][1] for x in q) for i in range(nlev)]
        tot = statistics.median(sum(v[0] + v[1] for v in x) for x in q)
        print("%s: %d quantizes\n  search  %s\n  recheck %s\n  search + recheck per quantize %.1f us" %
              (path, len(q), " ".join("%6.1f" % v for v in s), " ".join("%6.1f" % v for v in r), tot))


if __name__ == "__main__":
    main()
