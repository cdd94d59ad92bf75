// Philox4x32-10: one word of the block of counter (c0, c1, c2, c3) under key (k0, k1).  Shared by the noise stimulus (dwn_stim.hip,
// DESIGN.md 12q) and the start block of the population modes (dwn_modes.hip, 12u); tests/rf_reference.py restates it.
#pragma once
#include "dwn_common.h"

__device__ __forceinline__ unsigned philox_word(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, int word) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return word == 0 ? c0 : word == 1 ? c1 : word == 2 ? c2 : c3;
}
