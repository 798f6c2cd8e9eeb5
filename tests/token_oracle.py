"""The two rules of include/micromix_tokens.h over Python lists: mm_token_step (commit a verified step into the token history, with
stop conditions) and mm_ngram_draft (draft the next chain by prompt lookup).  Written from the header, not from the package's CPU
path: the search here goes from the longest n-gram down and takes the latest place it occurs, the package's walks the end positions."""

RUNNING, STOPPED, LENGTH = 0, 1, 2
STRIDE = 66


def clamp(x, lo, hi):
    return max(lo, min(hi, x))


def token_step(tokens, total_len, finished, result, target_tok, qo_indptr, root_tok, max_total, stop_tok=None, kv_status=0):
    """tokens: a list of rows (lists of ld_tok ints), changed in place like total_len and finished; result: rows of STRIDE ints.
    Returns emitted, or None when the call is a no-op (kv_status != 0)."""
    if kv_status:
        return None
    T, emitted = len(target_tok), []
    for b, row in enumerate(result):
        ld = len(tokens[b])
        q0, q1 = clamp(qo_indptr[b], 0, T), clamp(qo_indptr[b + 1], 0, T)
        n, k, N = q1 - q0, row[0], total_len[b]
        alone = finished[b] != RUNNING or n == 0 or n > 64 or root_tok[b] < 0 or k == 0
        alone = alone or not 0 <= k <= n or N < 0 or any(not 0 <= i < n for i in row[2:2 + k])      # not a row verify_greedy writes
        if alone:
            emitted.append(0)
            continue
        g = [target_tok[q0 + i] for i in row[2:2 + k]]
        limit = min(max_total[b], ld)
        cap = max(0, limit - N)
        c = min(k, cap)
        stops = [t for t in (stop_tok[b] if stop_tok is not None else []) if t >= 0]
        j = next((i for i in range(c) if g[i] in stops), None)
        if j is not None:
            m, finished[b] = j + 1, STOPPED
        else:
            m = c
            if N + m >= limit:
                finished[b] = LENGTH
        for i in range(m):
            tokens[b][N + i] = g[i]
        total_len[b] = N + m
        emitted.append(m)
    return emitted


def find_match(h, min_n, max_n):
    """(m, e) of the match of history h, or (0, None): the longest n-gram first, and its latest end position e <= N - 2"""
    N = len(h)
    for m in range(min(max_n, N - 1), min_n - 1, -1):
        suffix = h[N - m:]
        for e in range(N - 2, m - 2, -1):
            if h[e - m + 1:e + 1] == suffix:
                return m, e
    return 0, None


def ngram_draft(tokens, total_len, next_indptr, T, min_n, max_n):
    """tokens: a list of rows, whose slack is written in place.  Returns a dict of the six outputs; entries nothing writes are None"""
    B = len(tokens)
    out = dict(draft_tok=[None] * T, root_tok=[None] * B, cand_tok=[None] * T, match_len=[None] * B, row_seq=[None] * T,
               row_total_len=[None] * T)
    for b in range(B):
        ld = len(tokens[b])
        N = clamp(total_len[b], 0, ld)
        h = tokens[b][:N]
        m, e = find_match(h, min_n, max_n) if N >= 2 else (0, None)
        last = h[N - 1] if N else 0
        out["root_tok"][b] = h[N - 1] if N else -1
        out["match_len"][b] = m
        t0, t1 = clamp(next_indptr[b], 0, T), clamp(next_indptr[b + 1], 0, T)
        n = t1 - t0
        if n < 1 or n > 64:
            continue
        if m:
            p = N - 1 - e
            d = [h[e + 1 + (i % p)] for i in range(n - 1)]
        else:
            d = [last] * (n - 1)
        nodes = [last] + d
        for i in range(n):
            out["draft_tok"][t0 + i] = nodes[i]
            out["cand_tok"][t0 + i] = nodes[i + 1] if i + 1 < n else -1
            out["row_seq"][t0 + i] = b
            out["row_total_len"][t0 + i] = min(N + i, ld)
        for i, tok in enumerate(d):
            if N + i < ld:
                tokens[b][N + i] = tok
    return out


def rollout(f, prompt, max_total, ld, stops):
    """the plain greedy generation h[i + 1] = f[h[i]] from a prompt, cut behind its first stop token or at min(max_total, ld): what any
    sequence of token_step calls has to leave in the history, whatever was drafted.  Returns (history, finished)"""
    h, limit = list(prompt), min(max_total, ld)
    while len(h) < limit:
        h.append(f[h[-1]])
        if h[-1] in stops:
            return h, STOPPED
    return h, LENGTH


def chain_verify(target_tok, draft_tok, root_tok, qo_indptr):
    """mm_verify_greedy's result rows for chain drafts (include/micromix_hip.h): the walk from root_tok[b] along the nodes in order"""
    T, rows = len(target_tok), []
    for b, root in enumerate(root_tok):
        q0, q1 = clamp(qo_indptr[b], 0, T), clamp(qo_indptr[b + 1], 0, T)
        n = q1 - q0
        if n > 64 or root < 0:
            rows.append([n, target_tok[q1 - 1] if n else -1] + [-1] * 64)
            continue
        want, path = root, []
        for i in range(n):
            if draft_tok[q0 + i] != want:
                break
            path.append(i)
            want = target_tok[q0 + i]
        rows.append([len(path), want] + path + [-1] * (64 - len(path)))
    return rows


# ---- the loop of the tests: a deterministic "model" with short cycles, five requests ------------------------------------------------------
VOCAB, LOOP_LD, LOOP_STEPS = 96, 160, 8
LOOP_NODES = [6, 4, 6, 2, 5]


def model_table():
    """f: the token picked after token x.  Tokens 0 .. 59 lie on cycles of length 3, 4, 5, 6, 12 and 30, tokens 60 .. 95 on tails that
    run into token 0's cycle: every history becomes periodic, so the lookup hits, and the tails make drafts that miss"""
    f, at = [0] * VOCAB, 0
    for length in (3, 4, 5, 6, 12, 30):
        for i in range(length):
            f[at + i] = at + (i + 1) % length
        at += length
    assert at == 60
    for x in range(60, VOCAB):
        f[x] = x + 1 if x + 1 < VOCAB else 0
    return f


def loop_requests(variant):
    """(prompts, max_total, stop rows) of the five sequences; variant 1 rewrites every prompt, limit and stop set"""
    f = model_table()

    def run(start, n):
        h = [start]
        while len(h) < n:
            h.append(f[h[-1]])
        return h

    if variant == 0:
        prompts = [run(0, 7), run(3, 9), [70, 71, 5] + run(7, 11), run(12, 3), run(88, 4)]
        return prompts, [150, 40, 31, 1000, 60], [[-1, -1], [5, -1], [-1, -1], [-1, 17], [1, 2]]
    prompts = [run(18, 40), [9, 9, 9], run(30, 33), run(12, 14), run(60, 2)]
    return prompts, [64, 4, 160, 3, 120], [[-1, 25], [-1, -1], [59, 44], [-1, -1], [-1, 0]]


def loop_expected(variant):
    """per sequence (history, finished) of the plain rollout"""
    f = model_table()
    prompts, max_total, stops = loop_requests(variant)
    return [rollout(f, p, mt, LOOP_LD, [t for t in st if t >= 0]) for p, mt, st in zip(prompts, max_total, stops)]
