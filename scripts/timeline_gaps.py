"""From a rocprofv3 kernel trace (+ memory-copy trace) of the headline: the gaps between consecutive sketch
sweeps (the matrix sweep's launches, or the grouped kernel's in a library without it), what runs inside them and whether
merges / reranks overlap a sweep.  Where the trace holds launches of the matrix sweep's two-block form, the window is the
last long call's.  usage: timeline_gaps.py <dir>"""
import csv, glob, re, sys, statistics

path = sys.argv[1]
ev = []
for f in glob.glob(path + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        n = re.sub(r"szg::\(anonymous namespace\)::", "", r["Kernel_Name"])
        n = re.sub(r"\(.*", "", n).replace("void ", "")
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n[:60], "q" + r.get("Queue_Id", "")))
for f in glob.glob(path + "/**/*memory_copy_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy " + r.get("Direction", ""), "dma"))
ev.sort()
sw = [e for e in ev if e[2].startswith("scan_mx_kernel")]  # the matrix sketch sweep, where the library has it
if not sw:
    sw = [e for e in ev if e[2].startswith("scan_kernel<8") and ", 4, 2, true" in e[2]]
if not sw:
    sw = [e for e in ev if e[2].startswith("scan_kernel<8")]
print("sweeps:", len(sw), "name:", sw[0][2] if sw else None)
# the two-block form: launches of a long call -- wide launches of 32 queries, or shared launches of up to 64 (the same
# name: their argument types, cut off above, tell them apart); the collect flag may follow the block count
wide = [e for e in sw if re.search(r"scan_mx_kernel<.*, 2(, false)?>$", e[2])]
if wide:
    # the LAST long call (the timed one; the settling loop's 64-query calls keep one block): its run of wide sweeps --
    # more than a millisecond apart is another call -- with the one-block sweeps of its first and last batches
    run = [wide[-1]]
    for e in reversed(wide[:-1]):
        if run[0][0] - e[1] > 1000000:
            break
        run.insert(0, e)
    sw = [e for e in sw if run[0][0] - 1000000 <= e[0] and e[1] <= run[-1][1] + 1000000]
    print("the last long call: %d sweeps, %d of them of the two-block form" % (len(sw), len(run)))
    wd = [(e - s_) / 1e3 for s_, e, _, _ in run]
    print("two-block sweep us: median %.1f min %.1f max %.1f" % (statistics.median(wd), min(wd), max(wd)))
else:
    sw = sw[len(sw) // 4:]  # the timed region's (warm-up launches come first)
durs = [(e - s) / 1e3 for s, e, _, _ in sw]
print("sweep us: median %.1f min %.1f max %.1f" % (statistics.median(durs), min(durs), max(durs)))
gaps = []
for a, b in zip(sw, sw[1:]):
    gaps.append((b[0] - a[1]) / 1e3)
print("gap us: median %.1f mean %.1f min %.1f max %.1f (n=%d)" % (statistics.median(gaps), statistics.mean(gaps), min(gaps), max(gaps), len(gaps)))
gs = sorted(gaps)
print("gap percentiles 10/25/50/75/90: " + " ".join("%.1f" % gs[int(len(gs) * p)] for p in (0.1, 0.25, 0.5, 0.75, 0.9)))
# overlap of tails with sweeps
ov = {}
for s, e, n, q in ev:
    if n.startswith("scan_kernel") or n.startswith("scan_mx_kernel"):
        continue
    if s < sw[0][0] or e > sw[-1][1]:
        continue
    o = 0
    for a, b, _, _ in sw:
        lo, hi = max(s, a), min(e, b)
        if hi > lo:
            o += hi - lo
    d = ov.setdefault(n, [0, 0.0, 0.0])
    d[0] += 1
    d[1] += (e - s) / 1e3
    d[2] += o / 1e3
print("%-52s %6s %10s %10s" % ("inside the timed window", "calls", "total us", "of it beside a sweep"))
for n, (c, t, o) in sorted(ov.items(), key=lambda x: -x[1][1]):
    print("%-52s %6d %10.1f %10.1f" % (n, c, t, o))
# one window in full
i0 = ev.index(sw[4]) if len(sw) > 8 else 0
t0 = ev[i0][0]
print("--- a window of the timeline (us from its first sweep) ---")
for s, e, n, q in ev[i0:i0 + 40]:
    print("%9.1f  +%7.1f  %-5s %s" % ((s - t0) / 1e3, (e - s) / 1e3, q, n))
