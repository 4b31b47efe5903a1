// Jump tables of the PCG64 LCG: the affine map of k steps is  state' = A^k * state + S_k * inc  with S_k = 1 + A + ... + A^(k-1),
// and A^k, S_k are constants of the multiplier alone -- the same in every chain of every launch.  pcg_jump (pcg64_dev.hpp) finds them by
// square-and-multiply over the bits of k, two to four 128-bit multiplies per bit; where a chain of the sampler reset starts (one jump per
// lane to its first draw, behind the draws the launches before it used) that was the chain's whole start-up time.  Here they are tables,
// filled at build time by a constexpr generator on unsigned __int128:
//   lane table   k = 1 .. 128: lane l of G wavefront g owns output 64 g + l + 1 of a block; k = 128 is the block-to-block jump
//   count table  a 32-bit count q in six digits of six bits: one row (A^(d * 64^level), S_(d * 64^level)) per level and non-zero digit d,
//                so a jump by q is one row application per non-zero digit (at most six; three for a count below 2^18).  12 KB.
// The header is plain C++ as well (tools/pcg_jump_tab_dump.cpp prints the tables on the host, tests/test_pcg_jump_tab.py holds every row
// against NumPy's PCG64.advance); the device arrays exist under hipcc only.
#pragma once
#include <stdint.h>

namespace offsim {

typedef unsigned __int128 pcg_u128;

struct PcgJumpRow {  // A^k and S_k as 64-bit halves (32 bytes: two 16-byte loads)
    uint64_t a_lo, a_hi, s_lo, s_hi;
};

#define OFFSIM_PCG_LANE_ROWS 128
#define OFFSIM_PCG_COUNT_BITS 6
#define OFFSIM_PCG_COUNT_LEVELS 6                                        /* 6 x 6 = 36 bits >= 32 */
#define OFFSIM_PCG_COUNT_DIGITS ((1 << OFFSIM_PCG_COUNT_BITS) - 1)       /* non-zero digits of a level */
#define OFFSIM_PCG_COUNT_ROWS (OFFSIM_PCG_COUNT_LEVELS * OFFSIM_PCG_COUNT_DIGITS)

template <int N>
struct PcgJumpTab {
    PcgJumpRow row[N];
};

constexpr pcg_u128 pcg_tab_mult() { return ((pcg_u128)0x2360ED051FC65DA4ull << 64) | (pcg_u128)0x4385DF649FCCF645ull; }
constexpr PcgJumpRow pcg_tab_row(pcg_u128 a, pcg_u128 s) {
    return PcgJumpRow{(uint64_t)a, (uint64_t)(a >> 64), (uint64_t)s, (uint64_t)(s >> 64)};
}

// row k - 1 = (A^k, S_k):  S_k = S_(k-1) * A + 1
constexpr PcgJumpTab<OFFSIM_PCG_LANE_ROWS> pcg_make_lane_tab() {
    PcgJumpTab<OFFSIM_PCG_LANE_ROWS> t{};
    pcg_u128 a = 1, s = 0;
    for (int k = 1; k <= OFFSIM_PCG_LANE_ROWS; k++) {
        s = s * pcg_tab_mult() + 1;
        a = a * pcg_tab_mult();
        t.row[k - 1] = pcg_tab_row(a, s);
    }
    return t;
}

// row level * 63 + d - 1 = the jump by d * 64^level.  Jumps compose as  A^(m+n) = A^m * A^n,  S_(m+n) = S_m * A^n + S_n : a level's rows
// are its base jump (64^level steps) composed d times, and the next level's base is one composition more.
constexpr PcgJumpTab<OFFSIM_PCG_COUNT_ROWS> pcg_make_count_tab() {
    PcgJumpTab<OFFSIM_PCG_COUNT_ROWS> t{};
    pcg_u128 base_a = pcg_tab_mult(), base_s = 1;
    for (int lv = 0; lv < OFFSIM_PCG_COUNT_LEVELS; lv++) {
        pcg_u128 a = 1, s = 0;
        for (int d = 1; d <= OFFSIM_PCG_COUNT_DIGITS; d++) {
            s = s * base_a + base_s;
            a = a * base_a;
            t.row[lv * OFFSIM_PCG_COUNT_DIGITS + d - 1] = pcg_tab_row(a, s);
        }
        base_s = s * base_a + base_s;
        base_a = a * base_a;
    }
    return t;
}

static_assert(sizeof(PcgJumpTab<OFFSIM_PCG_COUNT_ROWS>) <= 64 * 1024, "the count table stays small enough for the scalar cache's neighbourhood");

#ifdef __HIPCC__
static __device__ constexpr PcgJumpTab<OFFSIM_PCG_LANE_ROWS> g_pcg_lane_tab = pcg_make_lane_tab();
static __device__ constexpr PcgJumpTab<OFFSIM_PCG_COUNT_ROWS> g_pcg_count_tab = pcg_make_count_tab();
#endif

}  // namespace offsim
