"""numpy oracle of greedy draft verification (include/micromix_hip.h, mm_argmax_rows / mm_verify_greedy).

argmax_rows(bits)        the order rule written out on the uint16 bits of bf16 values
verify(...)              the walk, `result` and the move table, sequence by sequence, node by node
seq_lens(...)            len_b from kv_indptr / last_page_len / page_size, as the attention kernels derive it

Nothing here shares code with the kernels."""
import numpy as np

STRIDE = 66


def rank(bits):
    """an integer that grows with the value under the rule: any NaN above +inf, +0 == -0, otherwise the order of the reals"""
    bits = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    mag, negative = bits & 0x7FFF, (bits >> 15) == 1
    r = np.where(negative, -mag, mag)                     # sign-magnitude -> a signed integer; both zeros give 0
    return np.where(mag > 0x7F80, 1 << 20, r)             # exponent all ones and a mantissa: a NaN, whatever its sign


def argmax_rows(bits):
    """bits: uint16 [rows, vocab] -> int64 [rows], the LOWEST index among each row's largest ranks"""
    r = rank(bits)
    best = r.max(axis=1, keepdims=True)
    return np.array([int(np.flatnonzero(row)[0]) for row in (r == best)], dtype=np.int64)


def seq_lens(kv_indptr, last_page_len, page_size):
    out = []
    for b in range(len(last_page_len)):
        pages = int(kv_indptr[b + 1]) - int(kv_indptr[b])
        out.append((pages - 1) * page_size + min(max(int(last_page_len[b]), 0), page_size) if pages > 0 else 0)
    return out


def parent_of(word, i):
    """the highest set bit of `word` below bit i, -1 without one; bits at i and above are ignored"""
    for j in range(i - 1, -1, -1):
        if int(word) >> j & 1:
            return j
    return -1


def verify(target_tok, draft_tok, root_tok, words, qo_indptr, kv_indptr, last_page_len, page_size):
    """words: one int per row (any sign: taken modulo 2^64) or None for chains.  Returns (result [B, 66], move_src [T], move_dst [T]),
    int32, every element defined."""
    T, B = len(target_tok), len(root_tok)
    result = np.full((B, STRIDE), -1, dtype=np.int32)
    src, dst = np.full((T,), -1, dtype=np.int32), np.full((T,), -1, dtype=np.int32)
    lens = seq_lens(kv_indptr, last_page_len, page_size)
    for b in range(B):
        q0, q1 = int(qo_indptr[b]), int(qo_indptr[b + 1])
        n = q1 - q0
        if n > 64 or int(root_tok[b]) < 0:                # a prompt chunk keeps all
            result[b, 0] = n
            result[b, 1] = int(target_tok[q1 - 1]) if n else -1
            continue
        base = lens[b] - n
        parents = [i - 1 if words is None else parent_of(int(words[q0 + i]) & (1 << 64) - 1, i) for i in range(n)]
        cur, want, path = -1, int(root_tok[b]), []
        while True:
            nxt = [i for i in range(n) if parents[i] == cur and int(draft_tok[q0 + i]) == want]
            if not nxt:
                break
            cur = nxt[0]
            path.append(cur)
            want = int(target_tok[q0 + cur])
        result[b, 0], result[b, 1] = len(path), want
        result[b, 2:2 + len(path)] = path
        for i, p in enumerate(path):
            src[q0 + i], dst[q0 + i] = base + p, base + i
    return result, src, dst


def paths_of(result, counts):
    """what PagedKVCache.commit makes of a result: the path, every token for a sequence that kept all, None where nothing was announced"""
    out = []
    for row, n in zip(np.asarray(result).tolist(), counts):
        k = row[0]
        out.append(None if not n else list(range(k)) if k and row[2] < 0 else row[2:2 + k])
    return out
