// pcg_jump_tab_dump -- prints the PCG64 jump tables of csrc/pcg64_jump_tab.hpp as the host compiler's constexpr evaluation fills them
// (the header is plain C++; the device arrays are the same initialisers).  One row per line:
//     lane  <k>          <A^k hi> <A^k lo> <S_k hi> <S_k lo>
//     count <level> <d>  <A^m hi> <A^m lo> <S_m hi> <S_m lo>      m = d * 64^level
// build:  c++ -std=c++17 -I rl-offline-simulation_amd/csrc tools/pcg_jump_tab_dump.cpp -o pcg_jump_tab_dump
// tests/test_pcg_jump_tab.py holds every row against numpy.random.PCG64.advance.
#include <stdio.h>

#include "pcg64_jump_tab.hpp"

using namespace offsim;

static constexpr PcgJumpTab<OFFSIM_PCG_LANE_ROWS> lane_tab = pcg_make_lane_tab();
static constexpr PcgJumpTab<OFFSIM_PCG_COUNT_ROWS> count_tab = pcg_make_count_tab();

static void row(const PcgJumpRow &w) {
    printf("%016llx %016llx %016llx %016llx\n", (unsigned long long)w.a_hi, (unsigned long long)w.a_lo, (unsigned long long)w.s_hi,
           (unsigned long long)w.s_lo);
}

int main(void) {
    printf("bits %d levels %d\n", OFFSIM_PCG_COUNT_BITS, OFFSIM_PCG_COUNT_LEVELS);
    for (int k = 1; k <= OFFSIM_PCG_LANE_ROWS; k++) {
        printf("lane %d ", k);
        row(lane_tab.row[k - 1]);
    }
    for (int lv = 0; lv < OFFSIM_PCG_COUNT_LEVELS; lv++)
        for (int d = 1; d <= OFFSIM_PCG_COUNT_DIGITS; d++) {
            printf("count %d %d ", lv, d);
            row(count_tab.row[lv * OFFSIM_PCG_COUNT_DIGITS + d - 1]);
        }
    return 0;
}
