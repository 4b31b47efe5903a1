// The rollout's draw-stream row: ro.rng[4 * r .. 4 * r + 3], four 64-bit words per rollout (include/offsim.h, offsim_rollouts.rng_kind).
//   OFFSIM_STREAM_PCG64   (state.hi, state.lo, inc.hi, inc.lo): NumPy's PCG64 before the next draw's step -- draw k (k = 0, 1, ..) is the
//                         output of the state k + 1 steps on, and a call that consumed n draws leaves the state n steps on;
//   OFFSIM_STREAM_PHILOX  (seed, draws consumed so far, 0, 0): draw k is Philox draw (count + k), a call adds n to the count.
// Either kind reads as base = (word 0, word 1), inc = (word 2, word 3): base.hi / base.lo are Philox's seed / count.  The kind is a runtime
// value here; a kernel that has it as a template parameter passes the constant.  (I: the caller's own index type -- the address arithmetic
// stays what it was when every kernel wrote these lines out.)
#pragma once
#include "offsim.h"
#include "pcg64_dev.hpp"

#define WAVE 64  // lanes of a wavefront

namespace offsim {

template <typename I>
__device__ __forceinline__ U128 stream_row_base(const uint64_t *rng, I r) { return u128(rng[4 * r + 0], rng[4 * r + 1]); }
template <typename I>
__device__ __forceinline__ U128 stream_row_inc(const uint64_t *rng, I r) { return u128(rng[4 * r + 2], rng[4 * r + 3]); }

// ONE lane: the row of a call that started at (base, inc) and consumed `consumed` draws.  No draw, no store.
template <typename I>
__device__ __forceinline__ void stream_row_commit(uint64_t *rng, I r, int kind, U128 base, U128 inc, uint64_t consumed) {
    if (consumed && kind == OFFSIM_STREAM_PHILOX) {
        rng[4 * r + 1] = base.lo + consumed;
    } else if (consumed) {
        const U128 nb = pcg_apply(pcg_jump(inc, consumed), base);
        rng[4 * r + 0] = nb.hi;
        rng[4 * r + 1] = nb.lo;
    }
}

// A whole wavefront: the 65-entry PCG64 jump table of a stream with increment inc -- the identity at 0, the jump by lane + 1 draws at
// lane + 1 (which is also returned: applied to `base` it is the state behind draw `lane`).
__device__ __forceinline__ Jump jump_table_fill(Jump *table, U128 inc) {
    const int lane = threadIdx.x & (WAVE - 1);
    const Jump mine = pcg_jump(inc, (uint64_t)lane + 1);
    table[lane + 1] = mine;
    if (lane == 0) {
        Jump id;
        id.mult = u128(0, 1);
        id.plus = u128(0, 0);
        table[0] = id;
    }
    return mine;
}

}  // namespace offsim
