"""Generates tests/golden/rms_sentinels.json: rows on which a wrongly ordered RMSNorm sum of squares changes the quantizer's bytes.

    python tests/golden/make_rms_sentinels.py [-jN] [K ...]

CPU only; uses nothing but numpy and the oracle.  For every K of tests/rms_order_cases.py: SPLITS it walks the seeded row stream of
that K (rms_order_cases.seeded_rows: an LCG, no numpy random stream) in batches, computes rvar in the oracle's order and in every
wrong order of rms_order_cases.ORDERS, and keeps for every (integer_round, wrong order) the first PER_CASE rows whose oracle bytes
differ between the two.  The cheap screen is bf16(fp32(x w rvar)) of any element; only the survivors go through the oracle.  An order
whose rvar never differed from the oracle's in the rows walked is recorded as vacuous for that K after 4096 rows with equal bits
(tests/test_rms_sentinels_cpu.py repeats that proof).  At the K of the decode tests a row is taken only if a weight that is one-hot
at the flip column carries the flip into the product (rms_order_cases.one_hot_output_differs).  Per sentinel: K, integer_round, the
row's number in the stream and the CRC-32 of its bits, the wrong order it detects, and the first reordered column whose element code
flips.  Split, norm weight and reorder index are functions of K (rms_order_cases.SPLITS, norm_weight, reorder_index), so every
sentinel of one K fits one launch.

Run time on the machine that produced the committed file (eight cores, -j7): two minutes in all, and six CPU-minutes summed over
the K ("seconds" per K in the file itself).  K = 4224 walks the most rows, 237 000: padding to whole waves moves rvar in one row
of a hundred there.
"""
import json
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import rms_order_cases as c  # noqa: E402

PER_CASE = 2
BATCH_ELEMS = 1 << 22
MAX_ROWS = {128: 40_000_000}        # give up (loudly) beyond this many rows of the stream; default below
VACUOUS_ROWS = 4096


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def search(k, log=print):
    split, w, idx = c.SPLITS[k], c.norm_weight(k), c.reorder_index(k)
    found = {(ir, name): [] for ir in (True, False) for name in c.ORDERS}
    differed = {name: 0 for name in c.ORDERS}
    batch = max(BATCH_ELEMS // k, 16)
    limit = MAX_ROWS.get(k, 4_000_000_000 // k)
    first = 0
    t0 = time.time()
    vacuous = []
    while first < limit:
        names = [n for n in c.ORDERS if n not in vacuous and any(len(found[(ir, n)]) < PER_CASE for ir in (True, False))]
        if not names:
            break
        x = c.seeded_rows(k, first, batch)
        right, wrong = c.rvars(x, names)
        for name in names:
            rows = np.flatnonzero(bits(wrong[name]) != bits(right))
            differed[name] += len(rows)
            if not len(rows):
                continue
            a = c.normalised_bits(x[rows], w, idx, right[rows])
            b = c.normalised_bits(x[rows], w, idx, wrong[name][rows])
            for r in rows[np.any(a != b, axis=1)]:
                for ir in (True, False):
                    if len(found[(ir, name)]) < PER_CASE:
                        col = c.flip_column(x[r], k, ir, wrong[name][r:r + 1])
                        if col >= 0 and (k not in c.DECODE_KS or c.one_hot_output_differs(x[r], k, ir, wrong[name][r:r + 1], col)):
                            found[(ir, name)].append(dict(K=k, integer_round=ir, row=int(first + r), order=name, column=col,
                                                              crc32=zlib.crc32(x[r].tobytes())))
        first += batch
        if first >= VACUOUS_ROWS:
            for name in names:
                if differed[name] == 0 and name not in vacuous:
                    vacuous.append(name)
        log(f"K={k}: {first} rows, {time.time() - t0:.0f} s, missing "
            f"{[(n, ir) for (ir, n), v in found.items() if len(v) < PER_CASE and n not in vacuous]}")
    missing = [(n, ir) for (ir, n), v in found.items() if len(v) < PER_CASE and n not in vacuous]
    if missing:
        raise SystemExit(f"K={k}: no {PER_CASE} sentinels for {missing} in {first} rows")
    sentinels = [s for (ir, n), v in sorted(found.items(), key=lambda kv: (not kv[0][0], c.ORDERS.index(kv[0][1]))) for s in v
                 if n not in vacuous]
    return sentinels, vacuous, first, time.time() - t0


def main(ks, jobs=1):
    out = c.load_fixture() if os.path.exists(c.FIXTURE) else dict(eps=c.EPS, per_case=PER_CASE, sentinels=[], vacuous={}, searched={})
    from multiprocessing import Pool
    with Pool(jobs) as pool:
        results = pool.imap(search, ks)
        for k in ks:
            merge(out, k, *next(results))


def merge(out, k, sentinels, vacuous, walked, secs):
    out["sentinels"] = sorted([s for s in out["sentinels"] if s["K"] != k] + sentinels, key=lambda s: s["K"])
    out["vacuous"][str(k)] = vacuous
    out["searched"][str(k)] = dict(rows=walked, seconds=round(secs))
    with open(c.FIXTURE, "w") as f:
        f.write("{\n")
        f.write(f' "eps": {out["eps"]}, "per_case": {out["per_case"]},\n')
        f.write(' "vacuous": ' + json.dumps(out["vacuous"]) + ",\n")
        f.write(' "searched": ' + json.dumps(out["searched"]) + ",\n")
        f.write(' "sentinels": [\n  ' + ",\n  ".join(json.dumps(s) for s in out["sentinels"]) + "\n ]\n}\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    jobs = [int(a[2:]) for a in args if a.startswith("-j")]
    main([int(a) for a in args if not a.startswith("-j")] or sorted(c.SPLITS, reverse=True), jobs[0] if jobs else 1)
