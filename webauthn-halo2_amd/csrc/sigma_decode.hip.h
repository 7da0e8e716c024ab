// sigma_decode.hip.h — a permutation argument's sigma value back into the cell it names.  Shared by the witness check (sigma as
// cell indices for the copy constraints) and the key audit (is every sigma value a label, is sigma a bijection).
//
// sigma(c, r) = delta^c' w^r'.  v^n = delta^(c' n) names the column among the shape's, and r' is the discrete logarithm of
// v delta^-c' in the group of order 2^k, bit by bit (Pohlig-Hellman: bit i is set iff (u_i)^(2^(k-1-i)) != 1, then
// u_{i+1} = u_i w^-(2^i)).
#pragma once
#include <vector>

#include "hostutil.h"

namespace zk {

inline Fr sigma_delta() {  // 7^(2^28): the generator of the permutation argument's cosets
    Fr d = fr_from_u64(7);
    for (int i = 0; i < 28; i++) d = fe_sqr(d);
    return d;
}

// the decoder's constants: delta^c | delta^(c n) | delta^-c (n_perm each) | w^-(2^i) (k)
inline std::vector<Fr> sigma_decode_consts(uint32_t k, uint32_t n_perm) {
    std::vector<Fr> consts((size_t)3 * n_perm + k);
    const Fr delta = sigma_delta(), delta_n = fe_pow_u64(delta, (uint64_t)1 << k), delta_inv = fe_inv_fast(delta);
    Fr d = Fr::one(), dn = Fr::one(), di = Fr::one();
    for (uint32_t p = 0; p < n_perm; p++) {
        consts[p] = d;
        consts[n_perm + p] = dn;
        consts[2 * n_perm + p] = di;
        d = fe_mul(d, delta);
        dn = fe_mul(dn, delta_n);
        di = fe_mul(di, delta_inv);
    }
    Fr wi = fe_inv_fast(fr_omega(k));
    for (uint32_t i = 0; i < k; i++) {
        consts[3 * n_perm + i] = wi;
        wi = fe_sqr(wi);
    }
    return consts;
}

// v = delta^cc w^rr with cc < n_perm, rr < 2^k: true and (cc, rr); false for a value that is no such label
__device__ __forceinline__ bool sigma_decode_label(const Fr& v, const Fr* __restrict__ consts, uint32_t n_perm, uint32_t k, uint32_t* cc_out,
                                                   uint32_t* rr_out) {
    Fr t = v;
    for (uint32_t i = 0; i < k; i++) t = fe_sqr(t);
    uint32_t cc = n_perm;
    for (uint32_t x = 0; x < n_perm && cc == n_perm; x++)
        if (t == fe_load(consts + n_perm + x)) cc = x;
    if (cc == n_perm) return false;
    const Fr one = Fr::one();
    Fr u = fe_mul(v, fe_load(consts + 2 * n_perm + cc));
    uint32_t rr = 0;
    for (uint32_t i = 0; i < k; i++) {
        Fr e = u;
        for (uint32_t s = i + 1; s < k; s++) e = fe_sqr(e);
        if (e != one) {
            rr |= 1u << i;
            u = fe_mul(u, fe_load(consts + 3 * n_perm + i));
        }
    }
    if (u != one) return false;
    *cc_out = cc;
    *rr_out = rr;
    return true;
}

}  // namespace zk
