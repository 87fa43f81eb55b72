// The permutation walk shared by every permutation-invariant loss (csrc/loss.hip: si-sdr, l1, mse; csrc/mrstft_loss.hip: the
// multi-resolution STFT loss).
#pragma once
#include "common.h"

#define PIT_MAXS 6

// The reference's walk over the permutations (src/loss.py:73-86): itertools.permutations(range(S)) order, strict '<' from
// lmin = 1e9, the sum over j of m[perm[j]][j] taken in fp32 in the order j = 0 .. S-1.  m is the S x S pair matrix (row =
// estimated speaker); best[j] = estimated speaker matched with target j.  One thread.
__device__ inline void pit_best_permutation(const float* m, int S, int* best) {
    int cur[PIT_MAXS];
    for (int k = 0; k < S; ++k) cur[k] = best[k] = k;
    float lmin = 1e9f;
    for (;;) {
        float l = 0.f;
        for (int j = 0; j < S; ++j) l += m[cur[j] * S + j];
        if (lmin > l) {
            lmin = l;
            for (int k = 0; k < S; ++k) best[k] = cur[k];
        }
        // next permutation in lexicographic order (the order of itertools.permutations(range(S)))
        int k = S - 2;
        while (k >= 0 && cur[k] > cur[k + 1]) --k;
        if (k < 0) break;
        int l2 = S - 1;
        while (cur[l2] < cur[k]) --l2;
        int t = cur[k]; cur[k] = cur[l2]; cur[l2] = t;
        for (int a = k + 1, b = S - 1; a < b; ++a, --b) { t = cur[a]; cur[a] = cur[b]; cur[b] = t; }
    }
}
