"""The device radix sort of csrc/kh_lattice.hip (SortPairs64: SortHistKernel, SortScanKernel, SortScatterKernel), called by
itself through kh_sort_pairs64, against the definition of a stable sort on the two bit fields of the key - bit for bit.

The sizes are boundaries of the code, not of the workload: the tile of 4096 pairs a block owns, the quarter of 1024 pairs a
wave owns (a tile that ends inside a quarter; waves without a pair), the 64 pairs a wave takes at a time, and the 256 columns
SortScanKernel scans per round (more than 256 tiles = more than 256*4096 pairs need its carry between rounds).  The bit
fields decide the number of 8-bit passes (odd: the result is in the second buffer) and the partial mask of a field's last
pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE, QUARTER, SCAN = 4096, 1024, 256

SIZES = [(str(n), n) for n in (1, 63, 64, 65, QUARTER - 1, QUARTER, QUARTER + 1, TILE - 1, TILE, TILE + 1)] + [
    ("3*4096+1024+1", 3 * TILE + QUARTER + 1),      # several tiles, the last one ends one pair into its second quarter
    ("256*4096", SCAN * TILE),                      # the last size with one round of the scan
    ("256*4096+1", SCAN * TILE + 1),                # 257 tiles: the scan's second round holds one column
    ("600*4096+777", 600 * TILE + 777),             # three rounds, the last one partial
]
FIELDS = [(1, 1),      # one pass per half, one-bit masks
          (8, 8),      # two full passes: the result is back in the first buffer
          (9, 1),      # three passes: the result is in the second buffer; the second pass has shift 8 and a one-bit mask
          (13, 20),    # the workload's fields: 2 + 3 passes, shifts 8 and 32 + 8, 32 + 16, masks of 5 and 4 bits
          (16, 16),    # four full passes
          (31, 31)]    # eight passes, every shift, 7-bit last masks
# the three sizes every field and every distribution runs at: below one tile, a partial last tile, the scan's carry
SMALL, MID, BIG = ("1025", QUARTER + 1), SIZES[10], SIZES[12]
DISTRIBUTIONS = ["uniform", "all_equal", "two_keys", "ascending", "descending", "bits_outside"]


def field_mask(lo_bits, hi_bits):
    return np.uint64(((1 << lo_bits) - 1) | (((1 << hi_bits) - 1) << 32))


def make_keys(rng, n, lo_bits, hi_bits, dist):
    def draw(k):
        lo = rng.integers(0, 1 << lo_bits, k, dtype=np.uint64)
        hi = rng.integers(0, 1 << hi_bits, k, dtype=np.uint64)
        return (hi << np.uint64(32)) | lo
    if dist == "uniform":
        return draw(n)
    if dist == "all_equal":    # one digit owns every cursor of every pass: the order of the payload is the input's
        return np.full(n, draw(1)[0], np.uint64)
    if dist == "two_keys":
        two = np.array([field_mask(lo_bits, hi_bits), np.uint64(0)])   # they differ in every pass
        return two[rng.integers(0, 2, n)]
    if dist == "ascending":
        return np.sort(draw(n))
    if dist == "descending":   # (equal keys occur, so the reverse of the input is NOT the answer)
        return np.sort(draw((n + 1) // 2))[::-1][np.arange(n) // 2].copy()
    if dist == "bits_outside":
        junk = rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
        return draw(n) | (junk & ~field_mask(lo_bits, hi_bits))
    raise ValueError(dist)


def check_sort(api, n, lo_bits, hi_bits, dist, seed):
    rng = np.random.default_rng(seed)
    keys = make_keys(rng, n, lo_bits, hi_bits, dist)
    vals = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)   # arbitrary payload, negatives and repeats
    assert keys.dtype == np.uint64 and keys.shape == (n,)
    keys_in, vals_in = keys.copy(), vals.copy()
    got_k, got_v = api.sort_pairs64(keys, vals, lo_bits, hi_bits)
    assert np.array_equal(keys, keys_in) and np.array_equal(vals, vals_in)      # the inputs are left alone
    m = keys & field_mask(lo_bits, hi_bits)
    order = np.argsort(m, kind="stable")
    assert np.array_equal(np.sort(got_v), np.sort(vals)), "the payload is not a permutation of the input's"
    assert np.array_equal(got_k, keys[order])
    assert np.array_equal(got_v, vals[order])


@pytest.mark.parametrize("size", SIZES, ids=[s[0] for s in SIZES])
@pytest.mark.parametrize("which", ["workload_field", "other_field"])
def test_every_size(api, size, which):
    """Every size with the workload's (13, 20) and with one of the other fields (they take turns)."""
    k = [s[0] for s in SIZES].index(size[0])
    others = [f for f in FIELDS if f != (13, 20)]
    lo_bits, hi_bits = (13, 20) if which == "workload_field" else others[k % len(others)]
    check_sort(api, size[1], lo_bits, hi_bits, "uniform", 1000 + k)


@pytest.mark.parametrize("size", [SMALL, MID, BIG], ids=[s[0] for s in (SMALL, MID, BIG)])
@pytest.mark.parametrize("field", FIELDS, ids=["%d,%d" % f for f in FIELDS])
def test_every_bit_field(api, field, size):
    check_sort(api, size[1], field[0], field[1], "uniform", 2000 + 37 * field[0] + field[1])


# every distribution at the three sizes with the workload's field, and below the largest size with (9, 1) too: a last-pass
# mask that is too wide shows only where bits outside the field are set
DIST_CASES = [(d, f, s) for d in DISTRIBUTIONS for f, sizes in (((13, 20), (SMALL, MID, BIG)), ((9, 1), (SMALL, MID))) for s in sizes]


@pytest.mark.parametrize("dist,field,size", DIST_CASES, ids=["%s-%d,%d-%s" % (d, f[0], f[1], s[0]) for d, f, s in DIST_CASES])
def test_every_key_distribution(api, dist, field, size):
    check_sort(api, size[1], field[0], field[1], dist, 3000 + DISTRIBUTIONS.index(dist))


def test_a_field_of_no_bits_takes_no_part(api):
    """lo_bits = 0 or hi_bits = 0: the order is the other field's alone; both 0: the input comes back as it is."""
    for lo_bits, hi_bits in ((0, 7), (11, 0), (0, 0)):
        rng = np.random.default_rng(41)
        n = MID[1]
        keys = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        vals = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
        got_k, got_v = api.sort_pairs64(keys, vals, lo_bits, hi_bits)
        order = np.argsort(keys & field_mask(lo_bits, hi_bits), kind="stable")
        assert np.array_equal(got_k, keys[order]) and np.array_equal(got_v, vals[order])


def test_no_pairs(api):
    k, v = api.sort_pairs64(np.zeros(0, np.uint64), np.zeros(0, np.int32), 13, 20)
    assert k.shape == (0,) and v.shape == (0,) and k.dtype == np.uint64 and v.dtype == np.int32
    lib, capi = api.lib(), api.capi
    assert lib.kh_sort_pairs64(0, None, None, 13, 20, None, None) == 0
    ko, vo = np.full(4, 7, np.uint64), np.full(4, -7, np.int32)        # n == 0 writes nothing
    assert lib.kh_sort_pairs64(0, ko.ctypes.data_as(capi.c_uint64_p), vo.ctypes.data_as(capi.c_int32_p), 13, 20,
                               ko.ctypes.data_as(capi.c_uint64_p), vo.ctypes.data_as(capi.c_int32_p)) == 0
    assert (ko == 7).all() and (vo == -7).all()


@pytest.mark.parametrize("n,lo_bits,hi_bits", [(-1, 13, 20), (2 ** 31, 13, 20), (2 ** 40, 13, 20), (4, -1, 20), (4, 32, 20),
                                               (4, 13, -1), (4, 13, 32), (4, 64, 64)])
def test_argument_errors(api, n, lo_bits, hi_bits):
    """Refused before any array is touched (the arrays hold 4 pairs whatever n says), and the outputs stay as they were."""
    lib, capi = api.lib(), api.capi
    k, v = np.arange(4, dtype=np.uint64), np.arange(4, dtype=np.int32)
    ko, vo = np.full(4, 7, np.uint64), np.full(4, -7, np.int32)
    rc = lib.kh_sort_pairs64(n, k.ctypes.data_as(capi.c_uint64_p), v.ctypes.data_as(capi.c_int32_p), lo_bits, hi_bits,
                             ko.ctypes.data_as(capi.c_uint64_p), vo.ctypes.data_as(capi.c_int32_p))
    assert rc == -1, rc     # KH_EINVAL
    assert b"argument check failed" in lib.kh_last_error()
    assert (ko == 7).all() and (vo == -7).all()
    with pytest.raises(api.KhError):
        api.check(rc)


def test_missing_arrays_are_an_argument_error(api):
    lib, capi = api.lib(), api.capi
    k, v = np.arange(4, dtype=np.uint64), np.arange(4, dtype=np.int32)
    kp, vp = k.ctypes.data_as(capi.c_uint64_p), v.ctypes.data_as(capi.c_int32_p)
    for args in ((None, vp, kp, vp), (kp, None, kp, vp), (kp, vp, None, vp), (kp, vp, kp, None)):
        assert lib.kh_sort_pairs64(4, args[0], args[1], 13, 20, args[2], args[3]) == -1
    with pytest.raises(api.KhError):
        api.sort_pairs64(k, v[:3], 13, 20)
