// floating_exact.h -- the long fixed-point accumulator in which floating_exact.hip sums the RB_FORCES / RB_TORQUES rows of a floating
// body exactly, so that the total does not depend on the order of the rows or on how they are split among ranks (DESIGN.md
// "Floating bodies").
//
// A float is an integer multiple of 2^-149 (subnormals included) below 2^128 in magnitude, so the sum of a body's rows of one
// component is N 2^-149 with an integer N.  N is held as FLOAT_LIMBS limbs of 32 bits, N = sum l_k 2^(32 k); canonical form:
// 0 <= l_k < 2^32 for k < 9, l_9 = floor(N / 2^288), signed.  2^32 rows keep |l_9| < 2^21.  Behind the limbs three counts: the
// NaN rows, the +Inf rows, the -Inf rows, which never enter the limbs.  On the wire (include/sphx.h, SPHX_FLOATING_LIMBS) every
// slot is a double with an integer value: canonical arrays of up to 1024 ranks add up exactly in any order.
#pragma once
#include "floating.h"

#define FLOAT_LIMBS      10
#define FLOAT_SLOTS      SPHX_FLOATING_LIMBS        // limbs, then the counts of NaN, +Inf and -Inf rows
#define FLOAT_LIMB_WAVES 4                          // one LDS accumulator per wave of floating_limbs_kernel's block
static_assert(FLOAT_SLOTS == FLOAT_LIMBS + 3, "the accumulator format of include/sphx.h");
static_assert(FLOAT_BLOCK == 64*FLOAT_LIMB_WAVES, "one accumulator per wave");
static_assert(6*FLOAT_LIMBS <= 64, "floating_limbs_finish_kernel gives every limb of a body a lane of one wave");

// per-block sums as the blocks leave them: signed 64-bit, not canonical (a limb has taken at most one term below 2^32 per row)
struct FloatingExactDev {
	long long part[SPHX_MAX_BODIES][FLOAT_MAX_BLOCKS][6][FLOAT_SLOTS];
};
static_assert(sizeof(FloatingExactDev) == FLOAT_EXACT_BYTES, "sphx_floating_setup allocates the limbs by this size");
