"""Per-step figures of the head of the headline's sweep run from a rocprofv3 kernel trace (profiles/sweep_head.txt):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python bench.py --steps 20
    python scripts/sweep_head_trace.py DIR/run_kernel_trace.csv

A step is a run of at least 40 fp64 sweep kernels in a row; the kernels between two such runs are the step's head (and the read-back
of the previous step's stop row).  Figures over the second half of the steps (the first half is bench.py's warm-up): the duration of
every kernel that is not a sweep, the idle time between neighbouring kernels of the head, the sweeps by their position in the step."""
import csv
import sys
import numpy as np

rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(sys.argv[1])))
is_sweep = lambda name: 'spmm_sell_kernel<double' in name
short = lambda name: name.split('(')[0][-44:]
runs = []
for i, r in enumerate(rows):
    if is_sweep(r[2]):
        if runs and i == runs[-1][-1] + 1:
            runs[-1].append(i)
        else:
            runs.append([i])
runs = [r for r in runs if len(r) >= 40]
timed = runs[len(runs) // 2:]
print('steps: %d (figures over the last %d), sweeps per step: %s' % (len(runs), len(timed), sorted({len(r) for r in runs})))
fmt = lambda v: 'median %6.2f us  min %6.2f  max %6.2f  (n = %d)' % (np.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3, len(v))
durations, gaps = {}, {}
for r in timed:
    j = r[0] - 1
    while j >= 0 and not is_sweep(rows[j][2]):
        j -= 1
    if j < 0:
        continue
    chain = list(range(j, r[0] + 1))                 # last sweep of the previous step, the kernels between, sweep 0
    for h in chain[1:-1]:
        durations.setdefault(short(rows[h][2]), []).append(rows[h][1] - rows[h][0])
    for a, b in zip(chain, chain[1:]):
        gaps.setdefault((short(rows[a][2]), short(rows[b][2])), []).append(rows[b][0] - rows[a][1])
print('kernels between the last sweep of a step and sweep 0 of the next:')
for name, v in durations.items():
    print('  %-44s x %.1f per step   %s' % (name, len(v) / len(timed), fmt(v)))
print('idle between neighbours:')
for (a, b), v in gaps.items():
    print('  %-44s -> %-44s %s' % (a, b, fmt(v)))
d = np.array([[rows[i][1] - rows[i][0] for i in r[:min(len(x) for x in timed)]] for r in timed]) / 1e3
print('sweep duration by position in the step (median, us): sweep 0 %.2f, 1 %.2f, 2 %.2f, 3 .. last-1 %.2f, last %.2f; all %.2f, mean %.3f'
      % (np.median(d[:, 0]), np.median(d[:, 1]), np.median(d[:, 2]), np.median(d[:, 3:-1]), np.median(d[:, -1]), np.median(d), d.mean()))
g = np.array([rows[b][0] - rows[a][1] for r in timed for a, b in zip(r, r[1:])]) / 1e3
print('idle between two sweeps of a step: median %.2f us, p99 %.1f, sum per step %.0f (the tracer stalls a replayed graph about once per step)'
      % (np.median(g), np.quantile(g, 0.99), g.sum() / len(timed)))
