"""The rule of mm_kv_step (include/micromix_kvstep.h) over Python lists: besides a twin PagedKVCache that runs accept + extend on the
host, the only source of expected values of tests/test_kv_step_cpu.py and tests/test_kv_step_gpu.py."""

HEADER_INTS = 4
OK, BAD_STATE, BAD_KEEP, BAD_NEXT, TOO_LONG, SEQ_PAGES, BAD_SUM, OUT_OF_PAGES, INDICES_CAPACITY = range(9)
NAMES = ("MM_KV_STEP_OK", "MM_KV_STEP_BAD_STATE", "MM_KV_STEP_BAD_KEEP", "MM_KV_STEP_BAD_NEXT", "MM_KV_STEP_TOO_LONG", "MM_KV_STEP_SEQ_PAGES",
         "MM_KV_STEP_BAD_SUM", "MM_KV_STEP_OUT_OF_PAGES", "MM_KV_STEP_INDICES_CAPACITY")


def ceil_div(x, P):
    return -(-x // P)


class State:
    """the state buffer, unpacked: status, steps_done, failed_step, seq_len, announced, pages (a list per sequence), free (the stack, top last)"""

    def __init__(self, seq_len, announced, pages, free, max_pages, pages_per_seq):
        self.status = self.steps_done = self.failed_step = 0
        self.seq_len, self.announced = list(seq_len), list(announced)
        self.pages, self.free = [list(p) for p in pages], list(free)
        self.max_pages, self.pages_per_seq = max_pages, pages_per_seq

    def ints(self):
        return HEADER_INTS + 3 * len(self.seq_len) + self.max_pages + len(self.seq_len) * self.pages_per_seq

    def pack(self):
        """the buffer as a list, 0 in the entries that mean nothing"""
        out = [self.status, self.steps_done, len(self.free), self.failed_step] + self.seq_len + self.announced + [len(p) for p in self.pages]
        out += self.free + [0] * (self.max_pages - len(self.free))
        for p in self.pages:
            out += p + [0] * (self.pages_per_seq - len(p))
        return out

    @classmethod
    def unpack(cls, flat, batch, max_pages, pages_per_seq):
        H, B = HEADER_INTS, batch
        lens, ann, num = flat[H:H + B], flat[H + B:H + 2 * B], flat[H + 2 * B:H + 3 * B]
        free = flat[H + 3 * B:H + 3 * B + flat[2]]
        at = H + 3 * B + max_pages
        st = cls(lens, ann, [flat[at + b * pages_per_seq:at + b * pages_per_seq + num[b]] for b in range(B)], free, max_pages, pages_per_seq)
        st.status, st.steps_done, st.failed_step = flat[0], flat[1], flat[3]
        return st


def step(st, P, max_seq_len, keep, next_new, num_next_tokens, capacity, depths=None):
    """one step on `st`, in place; returns the tables (kv_indptr, kv_indices, last_page_len, append_indptr, token_pos), or None when the
    step did nothing: a sticky status, or a condition met now (st.status, st.failed_step say which)"""
    if st.status:
        return None
    B = len(st.seq_len)
    keep = list(st.announced) if keep is None else list(keep)
    met = []
    for b in range(B):
        sl, an, np_ = st.seq_len[b], st.announced[b], len(st.pages[b])
        if sl < 0 or an < 0 or an > sl or np_ > st.pages_per_seq or np_ != ceil_div(sl, P):
            met.append(BAD_STATE)
        elif not 0 <= keep[b] <= an:
            met.append(BAD_KEEP)
        elif next_new[b] < 0:
            met.append(BAD_NEXT)
        elif sl - an + keep[b] + next_new[b] > max_seq_len:
            met.append(TOO_LONG)
        elif ceil_div(sl - an + keep[b] + next_new[b], P) > st.pages_per_seq:
            met.append(SEQ_PAGES)
    status = min(met) if met else OK
    if not status:
        kept = [st.seq_len[b] - st.announced[b] + keep[b] for b in range(B)]
        pushes = sum(len(st.pages[b]) - ceil_div(kept[b], P) for b in range(B))
        pops = sum(ceil_div(kept[b] + next_new[b], P) - ceil_div(kept[b], P) for b in range(B))
        if len(st.free) + pushes > st.max_pages:
            status = BAD_STATE
        elif sum(next_new) != num_next_tokens:
            status = BAD_SUM
        elif pops > len(st.free) + pushes:
            status = OUT_OF_PAGES
        elif sum(ceil_div(kept[b] + next_new[b], P) for b in range(B)) > capacity:
            status = INDICES_CAPACITY
    if status:
        st.status, st.failed_step = status, st.steps_done
        return None
    for b in range(B):                                      # 1: shorten, b ascending; the highest list entry is pushed first
        st.seq_len[b] = kept[b]
        while len(st.pages[b]) > ceil_div(kept[b], P):
            st.free.append(st.pages[b].pop())
    for b in range(B):                                      # 2: after all are shortened, pages in pop order
        while len(st.pages[b]) < ceil_div(st.seq_len[b] + next_new[b], P):
            st.pages[b].append(st.free.pop())
        st.seq_len[b] += next_new[b]
        st.announced[b] = next_new[b]
    st.steps_done += 1
    kv_indptr, kv_indices, last, app, pos = [0], [], [], [0], []
    for b in range(B):
        kv_indices += st.pages[b]
        kv_indptr.append(len(kv_indices))
        last.append(st.seq_len[b] - (len(st.pages[b]) - 1) * P if st.seq_len[b] else 0)
        for i in range(next_new[b]):
            pos.append(st.seq_len[b] - next_new[b] + (depths[app[-1] + i] if depths is not None else i))
        app.append(app[-1] + next_new[b])
    return kv_indptr, kv_indices, last, app, pos


def from_cache(cache, max_seq_len):
    """the State of a host-current PagedKVCache"""
    pps = ceil_div(max_seq_len, cache.page_size)
    announced = cache._announced[0] if cache._announced is not None else [0] * cache.batch
    return State(cache._seq_lens, announced, cache._pages, cache._free, cache.max_pages, pps)
