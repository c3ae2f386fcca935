// When a point of the fused vote is already "unlabelled" whatever its outstanding views say (no HIP beyond the qualifiers: tests
// compile this header for the host).
//
// segment_point (f3d_fuse.hip; voting.py:120-135) labels a point "unlabelled" when it has no votes, when its winner has none, or when
// winner < cmin[total], cmin[t] being the number of c in 0..t with (double)c / (double)t < threshold.  Mid-way through the views a point
// has  b  votes in the fullest bin that can win,  s  counted votes in all (every code but "no sample") and  R  views whose vote is not
// in its bins yet.  A completion adds r' <= R counted votes (the others sample nothing), a <= r' of them to the winner at most.
// cmin[t] does not decrease with t and grows by at most one per step (the division is monotone in both arguments), so
// cmin[s + r'] - (b + r') does not increase with r': the completion hardest to keep unlabelled sends all R votes to the leader.
// tests/test_fuse_decide_cpu.py checks this rule against the enumeration of every completion, for soundness and for tightness.
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#define __device__
#endif

#define F3D_DECIDE_MAX_TOTAL 255         // the table's last total (f3d_codebook::cmin has 256 entries)

// true: every completion of (b, s, R) ends "unlabelled".  cmin: the call's threshold table, entries 0 .. F3D_DECIDE_MAX_TOTAL.
__host__ __device__ inline bool f3d_decided_unlabelled(unsigned b, unsigned s, unsigned R, const uint16_t* cmin) {
    const unsigned t = s + R, w = b + R;
    if (t == 0u || w == 0u) return true;                                 // no vote can arrive, or none a winner could hold
    if (t > (unsigned)F3D_DECIDE_MAX_TOTAL) return false;                // beyond the table: the division itself decides, at the end
    return w < (unsigned)cmin[t];
}
