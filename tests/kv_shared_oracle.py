"""Hand-built page tables in which groups of sequences share real pages, host images of caches over them, and the group tensors of
mm_paged_decode_shared (include/micromix_hip.h) -- for tests/test_kv_shared_gpu.py and test_kv_shared_cpu.py.  Plain numpy.

layout     groups (shared count, tails) -> page table + group tables.  The members of a group list the same ceil(shared / P) leading
           pages; a member's own tokens go on from there -- first into what is left of the last common page (the tokens a fork in the
           middle of a page leaves there: physically the same rows for every member that reaches them), then onto pages of its own.
image      a poisoned host cache (NaN codes / parameters everywhere) in which exactly the rows some sequence holds carry the given K / V
reference  the fp64 oracle of tests/kv_oracle.py over the dequantized image (fp8 through tests/kv_fp8_oracle.py)
The sequence numbers of the members are a random permutation, so group_members is never the identity.
"""
from __future__ import annotations

import numpy as np

import kv_exact_cases as kc
import kv_fp8_oracle as fo
import kv_oracle as ko

HD = 128
KINDS = ("int4", "bf16", "fp8_e4m3")
SHARED_COUNTS = (0, 1, 31, 32, 33, 127, 128, 129)      # the tile (32) and four-wave round (128) edges
TAILS = (0, 1, 33, 130)


def group_sizes(g):
    per = 16 // g
    return (1, per, per + 1, 2 * per + 1)


def layout(P, groups, seed, spare=3, shuffle=True):
    """groups: [(shared, [tail of each member])] -> dict.  Page 0 belongs to nobody (the kernels address it for invalid tokens)."""
    rng = np.random.default_rng(seed)
    B = sum(len(t) for _, t in groups)
    ids = rng.permutation(B) if shuffle else np.arange(B)
    lens, pages, shared_len = [0] * B, [None] * B, [0] * B
    members, gptr, next_page, owner = [], [0], 1, {}
    for gi, (shared, tails) in enumerate(groups):
        common = list(range(next_page, next_page + -(-shared // P)))
        next_page += len(common)
        for p in common:
            owner[p] = ("group", gi)
        for tail in tails:
            b = int(ids[len(members)])
            members.append(b)
            lens[b], shared_len[b] = shared + tail, shared
            own = -(-(shared + tail) // P) - len(common)
            pages[b] = common + list(range(next_page, next_page + own))
            for p in pages[b][len(common):]:
                owner[p] = ("seq", b)
            next_page += own
        gptr.append(len(members))
    max_pages = next_page + spare
    remap = np.concatenate([[0], 1 + rng.permutation(max_pages - 1)]).astype(np.int64)     # shuffled physical pages, 0 stays free
    pages = [[int(remap[p]) for p in pg] for pg in pages]
    owner = {int(remap[p]): o for p, o in owner.items()}
    npg = [len(p) for p in pages]
    valid = np.zeros((max_pages, P), dtype=bool)            # rows some sequence holds
    pos = np.zeros((max_pages, P), dtype=np.int64)          # ... and their position in it (the same for every holder)
    for b in range(B):
        for t in range(lens[b]):
            valid[pages[b][t // P], t % P] = True
            pos[pages[b][t // P], t % P] = t
    return dict(P=P, B=B, lens=lens, pages=pages, max_pages=max_pages, valid=valid, pos=pos, owner=owner, groups=groups,
                kv_indptr=kc.indptr_of(npg), kv_indices=np.array(sum(pages, []), dtype=np.int32),
                last_page_len=np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32),
                group_indptr=np.array(gptr + [B] * (B + 1 - len(gptr)), dtype=np.int32),
                group_members=np.array(members, dtype=np.int32), shared_len=np.array(shared_len, dtype=np.int32),
                max_shared=max(shared_len + [0]), max_suffix=max([n - s for n, s in zip(lens, shared_len)] + [0]))


def table(lay):
    return lay["kv_indptr"], lay["kv_indices"], lay["last_page_len"]


def group_tables(lay):
    return lay["group_indptr"], lay["group_members"], lay["shared_len"]


def poisoned(kind, max_pages, L, Hkv, P):
    if kind == "fp8_e4m3":                                   # 0x7F is e4m3fn's NaN
        return (np.full((max_pages, L, 2, Hkv, P, HD), 0x7F, dtype=np.uint8),
                np.full((max_pages, L, 2, Hkv, P, 2), 0x7E00, dtype=np.uint16).view(np.float16))
    return kc.empty_host_cache(kind, max_pages, L, Hkv, P, True)


def image(kind, lay, L, layer, Kp, Vp):
    """Kp, Vp float32 [max_pages, P, Hkv, 128] holding bf16 values: the physical rows.  -> (data, param) of a cache that is NaN
    everywhere except the rows of `layer` that lay['valid'] marks"""
    Hkv = Kp.shape[2]
    data, param = poisoned(kind, lay["max_pages"], L, Hkv, lay["P"])
    pg, sl = np.nonzero(lay["valid"])
    for which, src in ((0, Kp), (1, Vp)):
        rows = src[pg, sl]                                  # [n, Hkv, 128]
        if kind == "bf16":
            data[pg, layer, which, :, sl] = kc.bf16_bits(rows)
        elif kind == "int4":
            codes, s, z = ko.quantize_row(rows)
            data[pg, layer, which, :, sl] = ko.pack_codes(codes)
            param[pg, layer, which, :, sl, 0] = s
            param[pg, layer, which, :, sl, 1] = z
        else:
            codes, e = fo.quantize_row(kc.bf16_bits(rows))
            data[pg, layer, which, :, sl] = codes
            param[pg, layer, which, :, sl] = fo.param_pair(e)
    return data, param


def reference(kind, q_bits, data, param, tbl, layer, sm_scale=None):
    """fp64 attention of every sequence over all of its tokens, from the image as the cache holds it"""
    if kind == "fp8_e4m3":
        data, param = fo.dequantize(data, param), None
    return ko.attention(q_bits, data, param, *tbl, layer, sm_scale)


def gaussian_rows(lay, Hkv, seed, scale_k=1.0, scale_v=0.5):
    rng = np.random.default_rng(seed)
    shape = (lay["max_pages"], lay["P"], Hkv, HD)
    return kc.to_bf16(rng.standard_normal(shape).astype(np.float32) * scale_k), kc.to_bf16(rng.standard_normal(shape).astype(np.float32) * scale_v)


def random_groups(g, seed, rounds=2):
    """every group size of group_sizes(g) `rounds` times, the shared counts of SHARED_COUNTS dealt over them in a seeded order, the tails
    of TAILS dealt over the members so that they differ within a slab; plus an empty sequence (a group of one that shares nothing)"""
    rng = np.random.default_rng(seed)
    counts = list(rng.permutation(SHARED_COUNTS))
    groups, k = [], int(rng.integers(0, 4))
    for r in range(rounds):
        for size in group_sizes(g):
            tails = [TAILS[(k + m) % 4] for m in range(size)]
            k += 1
            groups.append((int(counts[len(groups) % len(counts)]), tails))
    groups.append((0, [0]))
    return groups


# ---- exact answers: tests/kv_exact_cases.py's needle over shared pages -----------------------------------------------------------------
def needle_rows(lay, Hkv):
    """K of a row is the +-1 code of its position (kv_exact_cases.codebook); V names the row: v_grid(who, position, head), who = the
    group's number for a common page and 8 + the sequence's number (mod 16) for a page of its own"""
    mp, P = lay["max_pages"], lay["P"]
    Kp, Vp = np.zeros((mp, P, Hkv, HD), np.float32), np.zeros((mp, P, Hkv, HD), np.float32)
    heads = np.arange(Hkv)
    for p, (what, n) in lay["owner"].items():
        who = n if what == "group" else 8 + n
        Kp[p] = np.stack([kc.codebook(h)[lay["pos"][p]] for h in range(Hkv)], 1)
        Vp[p] = kc.v_grid(who, lay["pos"][p][:, None], heads[None, :])
    return Kp, Vp


def needle_queries(lay, g, Hkv, Vp):
    """(q float32 [B, Hq, 128], expect float64 [B, Hq, 128], targets [B, Hq]): member m's head hq names entry (m + hq) of the seam
    positions of its sequence -- the first and last shared token, the first and last token of its own tail, the token before the last
    shared one -- so the heads of a member name different tokens and the members of a slab different ones"""
    Hq, P, B = g * Hkv, lay["P"], lay["B"]
    kc.needle_margin_nats(Hkv, max(lay["lens"]))
    q, expect = np.zeros((B, Hq, HD), np.float32), np.zeros((B, Hq, HD))
    targets = np.full((B, Hq), -1, dtype=np.int64)
    for m, b in enumerate(lay["group_members"]):
        n, s = lay["lens"][b], int(lay["shared_len"][b])
        if n == 0:
            continue
        cand = sorted({t for t in (0, s - 1, s, n - 1, s - 2, s + 1) if 0 <= t < n})
        for hq in range(Hq):
            t, h = cand[(m + hq) % len(cand)], hq // g
            targets[b, hq] = t
            q[b, hq] = 8.0 * kc.codebook(h)[t]
            expect[b, hq] = Vp[lay["pages"][b][t // P], t % P, h]
    return q, expect, targets
