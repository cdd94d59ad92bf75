// The bounded multiplicative gain exp(m tanh(a)) and sech^2(a), shared by the behaviour modulator (dwn_modulator.hip) and the
// retinotopic readout gain (dwn_spatial.hip).  Device code only.
#pragma once
#include "dwn_common.h"

// tanh(a) = sign(a) (1 - e) / (1 + e), e = exp(-2 |a|).  Only its ABSOLUTE error counts (it enters log(gain) scaled by m), so the
// hardware exponential is enough here: the relative error of exp(x) through v_exp_f32 is about 2 eps (1 + |x|), eps = 2^-24, and
// |x| e^-|x| <= 1/e bounds what that does to e; with the sum, the difference and the quotient (correctly rounded here; the budget
// of tests/modulator_reference.py allows a 1-ulp reciprocal and a product) the error of tanh stays below 7 eps.  tanh(0) = 0 exactly (e = 1), so gain(0) = 1 exactly.  The gain's own exponent is at most m in size:
// the same exponential costs 2 eps (1 + m) there.  (The library's tanhf + expf measured 26.0 us against 24.3 us at the production geometry.)
__device__ __forceinline__ float mod_gain(float a, float m) {
    const float e = __expf(-2.f * fabsf(a));
    const float t = __fdividef(1.f - e, 1.f + e);
    return __expf(m * copysignf(t, a));
}
// sech^2(a) = 4 e / (1 + e)^2: here the RELATIVE error counts for every |a| (e = exp(-80) at |a| = 40), so e comes from expf
__device__ __forceinline__ float mod_sech2(float a) {
    const float e = expf(-2.f * fabsf(a));
    const float d = 1.f + e;
    return (4.f * e) / (d * d);
}
