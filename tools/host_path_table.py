"""Table of an A/B of tools/time_host_layer.py: python tools/host_path_table.py DIR, where DIR holds parent_<i>.txt and
branch_<i>.txt, one file per fresh process ('name us' lines), run in alternation with the order swapped every round
(profiles/binding_refactor_host_path.txt).  + / -: the branch's median lies above / below all of the parent's runs."""
import glob
import statistics
import sys


def runs(pattern):
    out = {}
    for path in sorted(glob.glob(pattern)):
        for line in open(path):
            if not line.startswith("#"):
                name, us = line.rsplit(" ", 1)
                out.setdefault(name, []).append(float(us))
    return out


parent, branch = runs(sys.argv[1] + "/parent_*.txt"), runs(sys.argv[1] + "/branch_*.txt")
print(f"{'case':38s}runs   parent min / median / max | branch min / median / max   branch - parent (medians)")
outside, deltas = [], []
for name, p in parent.items():
    b = branch[name]
    mp, mb = statistics.median(p), statistics.median(b)
    mark = "+" if mb > max(p) else "-" if mb < min(p) else " "
    if mark != " ":
        outside.append(f"{name} {mb - mp:+.2f}")
    deltas.append(mb - mp)
    print(f"{name:38s}{len(p):3d}   {min(p):6.2f} {mp:6.2f} {max(p):6.2f} | {min(b):6.2f} {mb:6.2f} {max(b):6.2f} {mark} {mb - mp:+.2f}")
print(f"{len(parent)} cases; branch median outside the parent's range: {len(outside)} ({'; '.join(outside) or 'none'}); "
      f"branch median - parent median: median {statistics.median(deltas):+.3f} us, largest {max(deltas):+.2f}, smallest {min(deltas):+.2f}")
