"""python tools/cross_encoder_prof_summary.py <rocprofv3 results .db>

Kernel summary of one CrossEncoder.predict batch from a rocprofv3 --kernel-trace database written by
`tools/cross_encoder_bench.py --profile-batch B` (two predict calls of B pairs each): the kernels of the SECOND call, i.e.
those after the first qst_cls_head_fwd launch up to and including the second."""
import collections
import sqlite3
import sys

db = sys.argv[1]
c = sqlite3.connect(db)
rows = c.execute("select name, start, end from kernels order by start").fetchall()
heads = [i for i, r in enumerate(rows) if "cls_head" in r[0]]
batch = rows[heads[-2] + 1:heads[-1] + 1]
agg = collections.defaultdict(lambda: [0, 0])
for name, s, e in batch:
    agg[name][0] += 1
    agg[name][1] += e - s
busy = sum(v[1] for v in agg.values())
first = next(i for i, r in enumerate(batch) if "position_ids" in r[0])        # the encoder's first launch
span = batch[-1][2] - batch[first][1]
print(f"one predict() batch: {len(batch)} launches, kernel time {busy / 1e3:.1f} us, encoder start to head end {span / 1e3:.1f} us")
print(f"{'calls':>6} {'total us':>10} {'avg us':>9} {'share':>6}  kernel")
for name, (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    print(f"{n:6d} {t / 1e3:10.1f} {t / 1e3 / n:9.2f} {100 * t / busy:5.1f}%  {name[:110]}")
