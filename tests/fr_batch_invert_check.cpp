// Host-only check of fr_batch_invert (csrc/prover_steps.h): the one Montgomery batch inversion behind the grand products of
// every prover and the SHPLONK Lagrange basis.  No device is touched.
#include <cstdio>
#include <vector>
#include "prover_steps.h"

static int fails = 0;
#define EXPECT(cond)                                           \
    do {                                                       \
        if (!(cond)) {                                         \
            printf("FAILED line %d: %s\n", __LINE__, #cond);   \
            fails++;                                           \
        }                                                      \
    } while (0)

// a deterministic non-zero element: (i + 2)^(i + 1) * 7^(2^5)
static Fr elem(uint32_t i) { return fe_mul(fe_pow_u64(fr_from_u64(i + 2), i + 1), fe_pow_u64(fr_from_u64(7), 32)); }

int main() {
    const Fr one = Fr::one(), minus_one = fe_neg(one);  // r - 1
    const Fr guard = fr_from_u64(0xC0FFEE);
    for (uint32_t count : {0u, 1u, 2u, 257u}) {
        std::vector<Fr> v(count), inv(count + 2, guard);  // one guard element on either side of the scratch
        for (uint32_t i = 0; i < count; i++) v[i] = elem(i);
        if (count >= 1) v[0] = one;
        if (count >= 2) v[count - 1] = minus_one;
        EXPECT(fr_batch_invert(v.data(), inv.data() + 1, count));
        for (uint32_t i = 0; i < count; i++) {
            EXPECT(inv[1 + i] == fe_inv_fast(v[i]));
            EXPECT(fe_mul(inv[1 + i], v[i]) == one);
        }
        EXPECT(inv[0] == guard && inv[count + 1] == guard);
        // a zero at the first, a middle and the last index: refused, nothing written outside the scratch — nor, inside it, past
        // the zero's own slot
        for (uint32_t z : {0u, count / 2, count ? count - 1 : 0u}) {
            if (z >= count) continue;
            std::vector<Fr> w(v), out(count + 2, guard);
            w[z] = Fr::zero();
            EXPECT(!fr_batch_invert(w.data(), out.data() + 1, count));
            EXPECT(out[0] == guard && out[count + 1] == guard);
            for (uint32_t i = z + 1; i < count; i++) EXPECT(out[1 + i] == guard);
        }
    }
    printf("fr_batch_invert: %d failures\n", fails);
    return fails ? 1 : 0;
}
