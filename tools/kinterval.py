"""Start-to-next-start interval per kernel from a rocprofv3 --kernel-trace database: for every launch of the steady-state training step
(the most frequent launch count between two k_adam launches, as tools/ktimeline.py) the time from its start to the start of the launch
behind it — the launch's duration plus the boundary that follows it, so a kernel whose stores now drain inside it instead of at its end
shows the net of both.  Means over all such steps; the step that follows a graph boundary is left out of k_adam's mean.
usage: python tools/kinterval.py <results.db>"""
import sqlite3
import statistics
import sys

c = sqlite3.connect(sys.argv[1])
rows = c.execute("select name, start, end from kernels order by start").fetchall()
is_adam = lambda n: n.startswith("k_adam") or n.startswith("void k_adam")
ends = [i for i, r in enumerate(rows) if is_adam(r[0])]
steps = [(ends[i] + 1, ends[i + 1] + 1) for i in range(len(ends) - 1)]
lens = {}
for a, b in steps:
    if b - a > 1:
        lens[b - a] = lens.get(b - a, 0) + 1
L = max(lens, key=lens.get)
steps = [(a, b) for a, b in steps if b - a == L and b < len(rows)]
iv = [[] for _ in range(L)]
du = [[] for _ in range(L)]
for a, b in steps:
    for k in range(L):
        nxt = rows[a + k + 1]
        if k == L - 1 and (b + L > len(rows) or not is_adam(rows[b + L - 1][0])):
            continue                                 # k_adam in front of a graph boundary (the next step is not a plain replayed one)
        iv[k].append(nxt[1] - rows[a + k][1])
        du[k].append(rows[a + k][2] - rows[a + k][1])
print(f"# {len(steps)} steps of {L} launches; mean over the steps, us")
print(f"{'#':>2s} {'kernel':52s} {'n':>5s} {'interval':>9s} {'duration':>9s} {'boundary':>9s}")
tot = 0.0
for k in range(L):
    name = rows[steps[0][0] + k][0]
    i, d = statistics.mean(iv[k]) / 1e3, statistics.mean(du[k]) / 1e3
    tot += i
    print(f"{k:2d} {name[:52]:52s} {len(iv[k]):5d} {i:9.3f} {d:9.3f} {i - d:9.3f}")
print(f"# sum of intervals {tot:.3f} us")
