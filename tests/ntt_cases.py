"""Inputs and references of the Fr NTT matrix (tests/test_ntt_cases.py pins them on the CPU, tests/test_gpu_ntt_plans.py holds the
device against them).  Vectors are (n, 4) uint64 arrays of stored words: Montgomery residues, canonical (< r).

Two independent references: the oracle's restatement of best_fft (cops.ntt, any primitive root) with the EvaluationDomain
wrappers of zkoracle.fastprover around it, and, for an impulse, the closed form — the transform of c e_j under the root w is
c, c w^j, c w^2j, ..: a run of powers that shares nothing with any butterfly code, the oracle's included."""
import numpy as np

from zkoracle import cops, fastprover as FP
from zkoracle.field import R, inv, omega

R_LIMBS = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
R_MINUS_1 = np.array([((R - 1) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def below_r(a):
    """Row-wise a < r over (n, 4) little-endian limbs."""
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (a[:, i] < R_LIMBS[i])
        eq &= a[:, i] == R_LIMBS[i]
    return lt


def canonical_random(rng, n):
    """n rows uniform in [0, r) as stored words.  r < 2^254: rows are drawn from 254 bits and those that come out >= r are
    drawn again (about a quarter) — replaced, not masked, so that words in [2^252, r) and both top bits occur."""
    a = np.frombuffer(rng.bytes(n * 32), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    bad = np.flatnonzero(~below_r(a))
    while bad.size:
        b = np.frombuffer(rng.bytes(bad.size * 32), dtype=np.uint64).reshape(bad.size, 4).copy()
        b[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        a[bad] = b
        bad = bad[~below_r(b)]
    return a


# ---- structured vectors: the largest stored word where the lazy bounds of the butterflies are largest ----

def all_max(n):
    return np.tile(R_MINUS_1, (n, 1))


def alternating_max(n):
    a = all_max(n)
    a[1::2] = 0
    return a


def period3_max(n, m):
    """r - 1 on i % 3 == m only: lines up with the period-3 factors of the coset transforms."""
    a = np.zeros((n, 4), dtype=np.uint64)
    a[m::3] = R_MINUS_1
    return a


STRUCTURED = ("all", "alt", "mod3")  # the three patterns of stored r - 1 the matrix runs


def structured(n, name):
    return all_max(n) if name == "all" else alternating_max(n) if name == "alt" else period3_max(n, 1)


def impulse(n, j, c):
    a = np.zeros((n, 4), dtype=np.uint64)
    a[j] = cops.fr_mont([c])[0]
    return a


def impulse_response(n, j, c, w):
    """Transform of c e_j under the root w, by its definition: out[i] = c w^(i j)."""
    return cops.fr_powers(pow(w, j, R), n, c)


# ---- the plan's first radix (csrc/ntt_plan.h, pinned by tests/ntt_plan_check.cpp): where the impulses are put ----

def default_first_radix_log2(log_n):
    max_r = 8 if log_n <= 16 else 9 if log_n <= 18 else 10 if log_n <= 20 else 7
    passes = -(-log_n // max_r)
    return -(-log_n // passes) if passes else 0


def impulse_positions(log_n):
    """0, 1, N/R, N/R + 1, N/2, N - 1 with R the first pass's radix under the default plan: the first and second element of the
    first two rows of the first pass's R x N/R view, the middle and the end."""
    n = 1 << log_n
    col = n >> default_first_radix_log2(log_n)
    return sorted({j for j in (0, 1, col, col + 1, n // 2, n - 1) if j < n})


# ---- resident-form references: zkoracle.fastprover's EvaluationDomain wrappers ----

def lagrange_to_coeff(v, k):
    return FP.lagrange_to_coeff(np.ascontiguousarray(v), k)


def coeff_to_lagrange(c, k):
    return cops.ntt(c, omega(k), k, FP.NT_FFT)


def coeff_to_extended(c, ext_k):
    """Any input length up to 2^ext_k (zero-extended)."""
    assert 0 < c.shape[0] <= 1 << ext_k
    return FP.coeff_to_extended(np.ascontiguousarray(c), ext_k)


def extended_to_coeff(e, ext_k):
    return FP.extended_to_coeff(np.ascontiguousarray(e), ext_k)


def omega_inv(log_n):
    return inv(omega(log_n), R)


def mont1(x):
    return cops.fr_mont([x])[0]
