#!/usr/bin/env python3
"""Per-kernel durations from a rocprofv3 database, grouped by kernel and grid: the step behind
profiles/ste_kernel_stats.csv.

    rocprofv3 --kernel-trace --stats -d OUT -o ste -- python tools/ste_bench.py --reps 5
    python tools/ste_kernel_stats.py OUT/ste_results.db > profiles/ste_kernel_stats.csv

Register counts are left out: the profiler's `vgpr_count` is not in the compiler's units
(hipcc -Rpass-analysis=kernel-resource-usage is the source for those).
"""
import csv
import sqlite3
import sys


def main(db):
    c = sqlite3.connect(db)
    rows = c.execute(
        'select name, grid_x, grid_y, count(*), avg(duration), min(duration), max(duration), '
        'max(scratch_size), max(lds_size) from kernels group by name, grid_x, grid_y '
        'order by min(id)')
    w = csv.writer(sys.stdout, lineterminator='\n')
    w.writerow(['kernel', 'grid_x', 'grid_y', 'calls', 'avg_us', 'min_us', 'max_us', 'scratch',
                'lds'])
    for r in rows:
        name = r[0].replace('ipa::(anonymous namespace)::', '').replace('(SteArgs)', '')
        w.writerow([name, r[1], r[2], r[3]] + ['%.1f' % (x / 1000.0) for x in r[4:7]] +
                   [r[7], r[8]])


if __name__ == '__main__':
    main(sys.argv[1])
