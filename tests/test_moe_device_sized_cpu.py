"""CPU tests of the device-sized grouped launches (mm_moe_quantize / mm_moe_matmul, include/micromix_hip.h): their status codes, which
come without device work, and the placement rule of the packed scale tensors restated in numpy -- expert e's run of 128-row tiles
starts at tile offsets[e] // 128 + e: for every offsets case the runs are disjoint, lie inside n // 128 + E tiles, and each holds
exactly the expert's own scale tensor as oracle/mx_oracle.py lays it out."""
import numpy as np
import pytest

from micromix_amd import _lib
from oracle import mx_oracle as o


def test_device_sized_entries_status_codes_without_device_work():
    lib = _lib.load()
    z, p = None, 16                                           # p: a non-null, 16-byte aligned pointer that is never dereferenced here
    assert lib.mm_version() >= 640
    S, U, B, OK = _lib.MM_ERR_BAD_SPLIT, _lib.MM_ERR_UNSUPPORTED, _lib.MM_ERR_BAD_ARG, _lib.MM_OK
    X, W4 = _lib.MM_QUANT_MIXED, _lib.MM_QUANT_W4
    quant = lambda src=p, ros=p, off=p, tab=p, E=8, n=16, rows=8, K=256, split=(128, 0, 128), mode=X, o3=(p, p, p), sf3=(p, p, p): \
        lib.mm_moe_quantize(src, ros, off, tab, E, n, rows, K, *split, mode, *o3, *sf3, z)
    mat = lambda A=(p,) * 6, off=p, tab=p, E=8, n=16, max_rows=8, N=256, split=(128, 0, 128), wmode=_lib.MM_W_FP4, flags=0, D=p: \
        lib.mm_moe_matmul(*A, off, tab, E, n, max_rows, N, *split, wmode, flags, D, z)
    # E outside [1, 64]
    for E in (0, 65, 1000):
        assert quant(E=E) == U and mat(E=E) == U, E
    # negative sizes
    assert quant(E=-1) == B and quant(n=-1) == B and quant(rows=-1) == B and quant(K=-256) == B
    assert mat(E=-1) == B and mat(n=-1) == B and mat(max_rows=-1) == B and mat(N=-1) == B and mat(split=(-128, 0, 128)) == B
    # a bad split
    assert quant(split=(128, 0, 64)) == S and quant(split=(128, 128, 128)) == S and quant(K=0, split=(0, 0, 0)) == S
    assert mat(split=(128, 0, 64)) == S and mat(split=(100, 0, 0)) == S
    # modes and flags
    assert quant(mode=2) == B and mat(wmode=7) == B
    assert mat(flags=_lib.MM_OUT_F32) == U and mat(flags=_lib.MM_OUT_F32 | _lib.MM_ROUND_ONCE) == U
    # n = 0 (and no source rows, no features, nothing allowed per expert): MM_OK, whatever the pointers
    assert quant(src=z, ros=z, off=z, tab=z, n=0, o3=(z, z, z), sf3=(z, z, z)) == OK and quant(src=z, rows=0) == OK
    assert mat(A=(z,) * 6, off=z, tab=z, n=0, D=z) == OK and mat(N=0, D=z) == OK and mat(max_rows=0, D=z) == OK
    # null pointers (row_of_slot may be null: the rows are then the slots themselves -- not tried here, it would launch)
    assert quant(src=z) == B and quant(off=z) == B and quant(tab=z) == B
    assert quant(o3=(z, p, p)) == B and quant(o3=(p, p, z)) == B and quant(sf3=(z, p, p)) == B and quant(sf3=(p, p, z)) == B
    assert mat(off=z) == B and mat(tab=z) == B and mat(D=z) == B
    for i in (0, 2, 3, 5):                                    # the N and O segments exist in this split, S does not
        A = [p] * 6
        A[i] = z
        assert mat(A=tuple(A)) == B, i
    # misaligned: bf16 rows and packed rows move as 16-byte pieces, scales as dwords, the table holds 8-byte addresses
    assert quant(src=8) == B and quant(o3=(8, p, p)) == B and quant(o3=(p, p, 24)) == B and quant(sf3=(2, p, p)) == B and quant(tab=12) == B
    assert mat(tab=12) == B and mat(D=17) == B
    # the supported() query answers without a device
    assert lib.mm_moe_matmul_supported(8, 256, 128, 0, 128, _lib.MM_W_FP4) == 1 and lib.mm_moe_matmul_supported(300, 4096, 0, 0, 14336, _lib.MM_W_MATCH) == 1
    assert lib.mm_moe_matmul_supported(0, 256, 128, 0, 128, _lib.MM_W_FP4) == 0 and lib.mm_moe_matmul_supported(8, 256, 100, 0, 128, _lib.MM_W_FP4) == 0
    assert lib.mm_moe_sf_bytes(300, 8, 256) == (300 // 128 + 8) * 128 * 8 and lib.mm_moe_sf_bytes(8, 64, 128) == 64 * 128 * 4


# ---- the scale-tile rule --------------------------------------------------------------------------------------------------------------
def first_tile(offsets, e):
    """the rule of include/micromix_hip.h: a function of offsets[e] alone"""
    return int(offsets[e]) // 128 + e


def allocated_tiles(n, E, kseg=128):
    """the allocation of a packed scale tensor in 128-row tiles, from the library's own size function (a tile: 128 rows x kseg / 32 bytes)"""
    nbytes, tile_bytes = int(_lib.load().mm_moe_sf_bytes(n, E, kseg)), 128 * kseg // 32
    assert nbytes % tile_bytes == 0
    return nbytes // tile_bytes


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])


def offsets_cases():
    rng = np.random.default_rng(7)
    cases = {
        "all rows in one expert": [0, 0, 0, 700, 0, 0, 0, 0],
        "all rows in the last expert": [0] * 7 + [129],
        "all experts empty but one row": [0, 0, 1, 0, 0, 0, 0, 0],
        "every M one below 128": [127] * 8,
        "every M at 128": [128] * 8,
        "every M one above 128": [129] * 8,
        "127 128 129 mixed": [127, 128, 129, 0, 129, 128, 127, 1],
        "E = 64, n = 8": [1 if e in (3, 9, 17, 26, 31, 40, 57, 63) else 0 for e in range(64)],
        "E = 64, n = 8 in two experts": [0] * 62 + [7, 1],
        "one expert": [300],
        "no rows": [0] * 8,
    }
    for i in range(12):
        E = int(rng.choice([1, 3, 8, 16, 64]))
        cases[f"random {i} (E = {E})"] = (rng.integers(0, 400, E) * (rng.random(E) < 0.7)).astype(np.int64).tolist()
    return cases


@pytest.mark.parametrize("name,counts", list(offsets_cases().items()))
def test_scale_tile_runs_are_disjoint_bounded_and_hold_each_experts_own_tensor(name, counts):
    off = offsets_of(counts)
    E, n = len(counts), int(off[-1])
    total = allocated_tiles(n, E)                             # the allocation: tiles per segment, as the library sizes it
    assert total == n // 128 + E
    owner = np.full(total, -1)
    for e in range(E):
        M = int(off[e + 1] - off[e])
        lo, tiles = first_tile(off, e), (M + 127) // 128
        assert 0 <= lo and lo + tiles <= total, (name, e)
        assert (owner[lo:lo + tiles] == -1).all(), f"{name}: expert {e}'s run overlaps expert {owner[lo:lo + tiles].max()}'s"
        owner[lo:lo + tiles] = e
    # every expert's scale bytes, written where the rule puts (slot s, block j), are the expert's own SF tensor at the run's first byte
    for kseg in (128, 384):
        tile_bytes = 128 * kseg // 32
        assert o.sf_size_x(127, kseg) == tile_bytes and allocated_tiles(n, E, kseg) == total            # one tile of the oracle's layout
        buf = np.full(total * tile_bytes, -1, dtype=np.int64)
        j = np.arange(kseg // 32)[None, :]
        for e in range(E):
            M = int(off[e + 1] - off[e])
            if M == 0:
                continue
            r = np.arange(M)[:, None]                          # the row inside the expert's own [M, kseg] matrix
            # as the kernel addresses it: the tile of (run, r // 128), then the oracle's offset of row r % 128 in one tile
            at = (first_tile(off, e) + r // 128) * tile_bytes + o.sf_offset(r % 128, j, kseg)
            assert (buf[at] == -1).all(), f"{name}: expert {e} writes a byte twice or over another expert's"
            buf[at] = e * 10 ** 6 + (r * (kseg // 32) + j)     # which (expert, row, block) the byte belongs to
            own = buf[first_tile(off, e) * tile_bytes:][: ((M + 127) // 128) * tile_bytes]
            valid = o.sf_valid_offsets(M, kseg)
            assert np.array_equal(own[valid], (e * 10 ** 6 + (r * (kseg // 32) + j)).reshape(-1)), f"{name}: expert {e}'s run is not its own SF tensor"
            rest = np.ones(len(own), dtype=bool)
            rest[valid] = False
            assert (own[rest] == -1).all()
        assert (buf[np.repeat(owner == -1, tile_bytes)] == -1).all()       # tiles no expert owns hold nothing


def test_scale_tile_rule_needs_its_e_term_and_reaches_its_bound():
    """64 experts of one row: every run is a tile of its own although n // 128 = 0 -- the `+ e` keeps them apart -- and the last run
    ends exactly at the bound n // 128 + E; 128 rows each: expert e's tile is 2 e, every second tile stays unowned"""
    off = offsets_of([1] * 64)
    assert [first_tile(off, e) for e in range(64)] == list(range(64)) and allocated_tiles(int(off[-1]), 64) == 64
    off = offsets_of([128] * 8)
    assert [first_tile(off, e) for e in range(8)] == [2 * e for e in range(8)] and first_tile(off, 7) + 1 <= allocated_tiles(int(off[-1]), 8)
