"""The rule of mm_uniform_rows (include/micromix_random.h) over Python integers: Philox4x32-10 and the layout of its words into streams.
Written from the header and from Random123's description of the generator, not from the package's CPU path: the key schedule is laid
out first and a round is a function of a tuple here; the package bumps the key as it goes and walks the rows."""

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = (1 << 32) - 1
MAX_N, MAX_ROWS = 16, 1 << 24


def _round(counter, key):
    c0, c1, c2, c3 = counter
    p0, p1 = M0 * c0, M1 * c2
    return ((p1 >> 32) ^ c1 ^ key[0], p1 & MASK, (p0 >> 32) ^ c3 ^ key[1], p0 & MASK)


def philox4x32_10(counter, key):
    """the four output words of Philox4x32 with ten rounds: counter a 4-tuple, key a 2-tuple of 32-bit integers"""
    assert len(counter) == 4 and len(key) == 2 and all(0 <= x <= MASK for x in (*counter, *key))
    schedule = [((key[0] + i * W0) & MASK, (key[1] + i * W1) & MASK) for i in range(10)]
    c = tuple(counter)
    for k in schedule:
        c = _round(c, k)
    return c


def words(seed, pos, sub, domain, n):
    """the n 32-bit words of one row: block j = i // 4 has counter (pos, sub, j, domain), key = the seed's halves"""
    seed, out = seed % (1 << 64), []
    for j in range(-(-n // 4)):
        out += philox4x32_10((pos % (1 << 32), sub % (1 << 32), j, domain), (seed & MASK, seed >> 32))
    return out[:n]


def uniform_rows(seed, pos, n=3, sub=None, row_seq=None, domain=0):
    """(u24, bits): two lists of n streams of len(pos) integers each; bits the 32-bit words, u24 = word >> 8, so that the fp32 number is
    u24 * 2^-24 exactly.  A row whose sequence is outside [0, len(seed)) holds zeros"""
    rows = len(pos)
    bits = [[0] * rows for _ in range(n)]
    for r in range(rows):
        s = r if row_seq is None else row_seq[r]
        if 0 <= s < len(seed):
            for i, w in enumerate(words(seed[s], pos[r], 0 if sub is None else sub[s], domain, n)):
                bits[i][r] = w
    return [[w >> 8 for w in stream] for stream in bits], bits


def as_int32(w):
    """a 32-bit word as the int32 that holds its pattern"""
    return w - (1 << 32) if w >> 31 else w
