"""Host side of the PCG64 jump-table tests (csrc/pcg64_jump_tab.hpp): the count lists, NumPy's own states and advances, and the number of
32-bit draws NumPy's shuffle has used when its chain crosses a cut (what a cut launch of the sampler reset starts from)."""
import numpy as np

M128 = (1 << 128) - 1
PCG_MULT = 0x2360ED051FC65DA44385DF649FCCF645
BITS, LEVELS = 6, 6

# composed counts: the ends of one, two and three digits, the count range of the cut launches (2^18), the ends of 31 and 32 bits ...
COUNTS_EDGE = [0, 1, 63, 64, 65, 4095, 4096, 2 ** 18 - 1, 2 ** 18, 2 ** 31 - 1, 2 ** 32 - 1]


def digits_to_count(digits):
    return sum(d << (BITS * lv) for lv, d in enumerate(digits))


# ... and a dozen with at least one zero digit between two non-zero ones (a skipped level): digits from level 0 up
COUNTS_SKIPPED = [digits_to_count(d) for d in (
    (1, 0, 1), (63, 0, 63), (5, 0, 0, 9), (17, 0, 33, 0, 2), (0, 7, 0, 7), (63, 0, 0, 0, 0, 3), (1, 0, 0, 0, 0, 1), (0, 0, 12, 0, 40),
    (44, 21, 0, 3), (9, 0, 63, 0, 63, 0), (0, 1, 0, 0, 15), (31, 0, 31, 0, 31, 2))]
COUNTS = COUNTS_EDGE + COUNTS_SKIPPED
assert len(COUNTS_SKIPPED) == 12 and all(0 <= q < 2 ** 32 for q in COUNTS)


def has_skipped_level(q):
    d = [(q >> (BITS * lv)) & 63 for lv in range(LEVELS)]
    nz = [lv for lv in range(LEVELS) if d[lv]]
    return len(nz) >= 2 and any(d[lv] == 0 for lv in range(nz[0], nz[-1]))


assert all(has_skipped_level(q) for q in COUNTS_SKIPPED)


def pcg_state(seed):
    """(state, inc) of np.random.PCG64(seed) as Python ints."""
    s = np.random.PCG64(seed).state["state"]
    return int(s["state"]), int(s["inc"])


def advanced(seed, k):
    """NumPy's state k steps behind PCG64(seed)'s."""
    bg = np.random.PCG64(seed)
    bg.advance(int(k))
    return int(bg.state["state"]["state"])


def draws_at_cuts(seed, n, cuts):
    """32-bit draws np.random.default_rng(seed).shuffle(list of n) has used when step i = cut - 1 is next, for every cut < n: Generator.shuffle
    of a list runs i = n-1 .. 1 with j = random_interval(i), masked rejection on next_uint32, which hands out the low half of a 64-bit
    output, then the buffered high half.  (Checked against the shuffle itself by the caller's tests: the device continues from these.)"""
    raw = np.random.PCG64(seed).random_raw(2 * n + 4096)
    d32 = np.empty(2 * raw.size, dtype=np.uint32)
    d32[0::2] = (raw & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    d32[1::2] = (raw >> np.uint64(32)).astype(np.uint32)
    d32 = d32.tolist()
    out, c = {}, 0
    for i in range(n - 1, 0, -1):
        if i + 1 in cuts:
            out[i + 1] = c
        mask = (1 << i.bit_length()) - 1
        while True:
            v = d32[c] & mask
            c += 1
            if v <= i:
                break
    return out
