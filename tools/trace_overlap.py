#!/usr/bin/env python3
"""Persistent kernels of a rocprofv3 kernel trace (conv_wino_kernel, gdn_resident_kernel, thin_mfma_kernel), every launch
labelled by whether a range-coder kernel (range_encode* / range_decode*) was running on another queue when it STARTED, and by how
much of its duration one was.  Launches are grouped by (kernel, grid, main queue or not, place in the step): a step issues the
same launches in the same order on its main queue (the busiest one), so launch i of N of a kernel over S traced steps is launch
i % (N / S) of a step, and places whose shortest launches agree within 4 % are one shape.  (On the side queues the order of two
launches can differ from step to step: a place whose launches differ by more than x3 is reported as `mixed` and left out of
the sums.)  Per group: launches and mean duration not overlapped / overlapped at the start, and the excess
= sum over the overlapped launches of (duration - mean of the not overlapped ones).  Then each kernel's time per step and
its longest launch.
usage: trace_overlap.py <kernel_trace.csv> <steps traced, warm-up included> [csv_out]"""
import bisect
import collections
import csv
import re
import sys

PERSISTENT = ('conv_wino_kernel', 'gdn_resident_kernel', 'thin_mfma_kernel')


def short(n):
    n = re.sub(r'\(.*', '', n).replace('void ', '').replace('aivc::', '')
    return n[:48]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    steps = int(sys.argv[2])
    coders = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in rows
                    if 'range_encode' in r['Kernel_Name'] or 'range_decode' in r['Kernel_Name'])
    c_start = [c[0] for c in coders]
    longest = max((e - s for s, e in coders), default=0)

    def coder_time(s, e):
        """-> (a coder was running at s, ns of [s, e) during which at least one was)"""
        lo = bisect.bisect_left(c_start, s - longest)
        hi = bisect.bisect_left(c_start, e)
        at_start, spans = False, []
        for cs, ce in coders[lo:hi]:
            if ce <= s:
                continue
            at_start |= cs <= s
            spans.append((max(cs, s), min(ce, e)))
        covered, end = 0, s
        for a, b in sorted(spans):
            if b > end:
                covered += b - max(a, end)
                end = b
        return at_start, covered

    qmain = collections.Counter(r['Queue_Id'] for r in rows).most_common(1)[0][0]
    per_kernel = collections.defaultdict(list)
    rows_of = collections.defaultdict(list)
    for r in rows:
        if any(p in r['Kernel_Name'] for p in PERSISTENT):
            grid = int(r.get('Grid_Size_X', r.get('Grid_Size', 0)) or 0) // int(r.get('Workgroup_Size_X', 1) or 1)
            span = (int(r['Start_Timestamp']), int(r['End_Timestamp']))
            per_kernel[(short(r['Kernel_Name']), grid, 'main' if r['Queue_Id'] == qmain else 'side')].append(span)
            rows_of[short(r['Kernel_Name'])].append(span[1] - span[0])
    lines = ['kernel,grid,queue,shape_ms,launches_per_step,clear_n,clear_mean_ms,overlapped_n,overlapped_mean_ms,ratio,excess_ms_per_step,coder_share_of_overlapped']
    total_excess = collections.Counter()
    mixed = collections.Counter()
    for (name, grid, queue), ls in sorted(per_kernel.items()):
        ls.sort()
        per_step = len(ls) // steps if len(ls) % steps == 0 else len(ls)
        places = collections.defaultdict(list)
        for i, (s, e) in enumerate(ls):
            places[i % per_step].append((s, e))
        for pl in [pl for pl, v in places.items() if max(e - s for s, e in v) > 3 * min(e - s for s, e in v)]:
            mixed[name] += sum(e - s for s, e in places.pop(pl))
        # places of one shape: shortest launches within 4 %
        shapes = []
        for pl, v in sorted(places.items(), key=lambda kv: min(e - s for s, e in kv[1])):
            t = min(e - s for s, e in v)
            if shapes and t <= shapes[-1][0] * 1.04:
                shapes[-1][1].extend(v)
                shapes[-1][2] += 1
            else:
                shapes.append([t, list(v), 1])
        for t, v, n_places in shapes:
            clear, over, share = [], [], 0.0
            for s, e in v:
                at_start, covered = coder_time(s, e)
                (over if at_start else clear).append(e - s)
                if at_start:
                    share += covered / (e - s)
            cm = sum(clear) / len(clear) if clear else float('nan')
            om = sum(over) / len(over) if over else float('nan')
            excess = sum(d - cm for d in over) / steps / 1e6 if clear and over else 0.0
            total_excess[name] += excess
            lines.append('"%s",%d,%s,%.3f,%d,%d,%.3f,%d,%.3f,%.3f,%.2f,%.2f' % (name, grid, queue, t / 1e6, n_places, len(clear), cm / 1e6, len(over), om / 1e6,
                                                                          om / cm if clear and over else float('nan'), excess, share / len(over) if over else 0.0))
    print('\n'.join(lines))
    for k, v in total_excess.items():
        print('excess per step at launches that started beside a coder: %-48s %8.2f ms   (mixed places left out: %.2f ms per step)' % (k, v, mixed[k] / steps / 1e6))
    for k, v in sorted(rows_of.items()):
        print('kernel row: %-48s %4d launches per step, %8.2f ms per step, longest %.3f ms' % (k, len(v) // steps, sum(v) / steps / 1e6, max(v) / 1e6))
    print('coder kernels: %d, busy %.1f ms per step' % (len(coders), sum(e - s for s, e in coders) / steps / 1e6))
    if len(sys.argv) > 3:
        open(sys.argv[3], 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
