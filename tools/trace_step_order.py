#!/usr/bin/env python3
"""The schedule of ONE training step as the hardware queues saw it: for the last whole step of a rocprofv3 kernel trace (kernel_trace.csv of a
short bench.py run, either schedule), the ordered list of kernel names per hardware queue and a digest of each list.  Two builds enqueue the same
schedule when they print the same SET of per-queue digests (the queue numbers themselves may differ between runs) -- the last line is a digest
of that set.  Reads a CSV, touches no GPU.

    python3 tools/trace_step_order.py OUT/*/*_kernel_trace.csv [--names]       # --names: every kernel name, not only the digests"""
import csv
import hashlib
import re
import sys
from collections import defaultdict


def short(n):
    n = re.sub(r'\(anonymous namespace\)::', '', n)
    return re.sub(r'^void ', '', n)


def step_queues(path):
    """{queue: [kernel names in dispatch order]} of the last whole step: from the end of the previous step's third Adadelta launch (enhancer,
    ASR, D: the D update is a step's last kernel) to the end of this step's, as tools/trace_sequence.py finds it."""
    rows = list(csv.DictReader(open(path)))
    qkey = 'Queue_Id' if 'Queue_Id' in rows[0] else 'Stream_Id'
    order = 'Dispatch_Id' if 'Dispatch_Id' in rows[0] else 'Start_Timestamp'
    ends = sorted(int(r['End_Timestamp']) for r in rows if 'adadelta' in r['Kernel_Name'])
    if len(ends) < 4:
        sys.exit('%s: fewer than two steps in the trace (%d Adadelta launches)' % (path, len(ends)))
    t0, t1 = ends[-4], ends[-1]
    queues = defaultdict(list)
    for r in sorted(rows, key=lambda r: int(r[order])):
        if int(r['Start_Timestamp']) >= t0 and int(r['End_Timestamp']) <= t1:
            queues[r[qkey]].append(short(r['Kernel_Name']))
    return queues, (t1 - t0) / 1e6


def main(path, names=False):
    queues, ms = step_queues(path)
    digests = sorted((hashlib.sha256('\n'.join(seq).encode()).hexdigest()[:16], len(seq), q) for q, seq in queues.items())
    print('last whole step: %.2f ms, %d kernels on %d queues' % (ms, sum(d[1] for d in digests), len(digests)))
    for dg, n, q in sorted(digests, key=lambda d: -d[1]):
        print('queue %-4s %6d kernels  %s' % (q, n, dg))
        if names:
            for k in queues[q]:
                print('    ' + k)
    print('schedule digest %s' % hashlib.sha256(' '.join('%s:%d' % d[:2] for d in digests).encode()).hexdigest()[:16])


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--names']
    main(args[0], names='--names' in sys.argv[1:])
