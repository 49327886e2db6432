"""Start / run / gap listing of one bench step's dispatches, and their counts by kind, from a rocprofv3 kernel trace; in front
of it one line per traced step (span, busy, idle), so that a step with a hiccup of the host can be told from the others.
Usage: python tools/step_timeline.py <kernel_trace.csv> [step]     (step: 1 = the last complete one, the default; 2 = the one before ...)"""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
back = int(sys.argv[2]) if len(sys.argv) > 2 else 1
ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows), key=lambda e: e[0])
# steps start at k_partition
starts = [i for i, e in enumerate(ev) if "k_partition" in e[2]]
if len(starts) < back + 1:
    sys.exit("not that many steps")
for s in range(len(starts) - 1):
    st = ev[starts[s]:starts[s + 1]]
    span, busy = ev[starts[s + 1]][0] - st[0][0], sum(e[1] - e[0] for e in st)
    print("traced step %d: span %.3f ms, busy %.3f ms, idle %.3f ms, %d dispatches" % (s, span / 1e6, busy / 1e6, (span - busy) / 1e6, len(st)))
a, b = starts[-1 - back], starts[-back]
step = ev[a:b]
t0 = step[0][0]
busy = sum(e[1] - e[0] for e in step)
span = ev[b][0] - t0
print("step span %.3f ms, busy %.3f ms, idle %.3f ms, %d dispatches" % (span / 1e6, busy / 1e6, (span - busy) / 1e6, len(step)))
kinds = {}
for i, (s, e, name) in enumerate(step):
    nxt = step[i + 1][0] if i + 1 < len(step) else ev[b][0]
    short = name.split("(")[0]
    print("%8.1f us  + %6.1f run  %6.1f gap  %s" % ((s - t0) / 1e3, (e - s) / 1e3, (nxt - e) / 1e3, short))
    kind = ("copy" if "copyBuffer" in name else "runtime fill" if "fillBuffer" in name
            else "fill kernel (k_fill / k_fill2)" if "k_fill" in name else "other kernels")
    kinds[kind] = kinds.get(kind, 0) + 1
print("dispatches by kind:", ", ".join("%s %d" % kv for kv in sorted(kinds.items())))
