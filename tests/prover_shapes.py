"""Circuit shapes shared by the prover and verifier tests (tests/test_gpu_prover.py, tests/test_gpu_verify_shapes.py,
tests/test_verify_host.py, tests/shape_sweep.py): (A, L, F, k, lookup_bits[, idle]) of the shapes that take different branches of
the prover, a seeded random draw of small shapes, and the full-size bench_ecdsa.config rows."""
import random

SHAPES = {
    "k19like": (1, 1, 1, 7, 6),
    "k17like": (4, 1, 1, 7, 5),
    "k18like": (2, 1, 1, 6, 4),
    "wide": (3, 2, 2, 8, 6),
    "idle": (5, 2, 2, 7, 5, 2),  # two trailing gate columns never enabled (the k <= 13 bench rows)
    # k >= 10: the SRS window tables exist, so commitments go through the column-batched MSM passes (and the
    # batched transforms / grand products / divisions) that the full-size proofs use
    "k10batched": (3, 2, 1, 10, 8),
    "k10single": (1, 1, 1, 10, 9),
    # more than 32 terms in every group of the quotient's y-combination (36 gate terms, 49 l_0 terms, 49 active-row terms) — but
    # quotient_log_slices(9, 36) = 4: quotient_sliced_kernel with 16 lanes per row, and no lane holds more than 3 gate terms, 4 l_0
    # terms, 2 l_last terms and 4 active-row terms.  The 32-term fold of quotient.hip's lazy sums is NOT reached here (nor by any
    # other shape of this file: tests/test_quotient_cases.py counts them); tests/test_gpu_quotient_device.py reaches it
    "manycols": (36, 12, 2, 7, 5),
    # more than 40 polynomials in one rotation set over >= 256 rows: the multi-open's linear combinations go through the
    # argument-list kernel (lincomb_terms), the quotient through the lanes-per-row kernel (16 lanes per row: at most 3 gate
    # terms, 4 l_0 terms, 2 l_last terms and 4 active-row terms per lane)
    "manycols_k8": (44, 6, 2, 8, 6),
}


# the seed of the draw tests/test_gpu_prover.py proves; the verifier tests take the head of the same draw
DRAW_SEED = 0x5EED0305


def random_shapes(count, seed):
    """Circuit shapes drawn at random (fixed seed): small enough for the plain-Python oracle, spread over everything the
    engine branches on — one or many gate columns, 1 ... 8 lookups, idle gate columns, 6 <= k <= 9, 1 ... 3 constants columns."""
    pr = random.Random(seed)
    shapes = []
    while len(shapes) < count:
        k = pr.choice([6, 7, 7, 8, 8, 9])
        A = pr.choice([1, 2, 3, 5, 9, 17, 33, 45]) if k <= 8 else pr.choice([1, 2, 4, 9])
        L = 1 if A == 1 else pr.choice([1, 2, 3, 8 if A >= 9 else 2])
        F = pr.choice([1, 1, 2, 3])
        lb = pr.randrange(3, k)            # lookup table of 2^lb rows inside the usable rows
        idle = pr.choice([0, 0, 1, 2]) if A >= 3 else 0
        if 2 * idle > A:   # more never-enabled selectors than used ones would pair up in columns of their own: not modelled
            idle = A // 2
        shapes.append((A, L, F, k, lb, idle))
    return shapes


# the remaining rows of halo2-circuits/src/configs/bench_ecdsa.config with the proof sizes the
# reference published for them (halo2-circuits/src/results/ecdsa_bench.csv:3,5-10)
# The k <= 13 rows are published 1 / 2 / 3 evaluations short of the full column shape: the only halo2
# mechanism that removes single elements is selector compression dropping the fixed column of a never-enabled
# selector, i.e. the circuit leaves its last 1 / 2 / 3 gate columns idle (last tuple entry).
BENCH_ROWS = [
    (18, 2, 1, 1, 17, 1344, 0),
    (16, 8, 2, 1, 15, 3552, 0),
    (15, 17, 3, 1, 14, 6560, 0),
    (14, 34, 6, 1, 13, 12704, 0),
    (13, 68, 12, 1, 12, 24960, 1),
    (12, 139, 24, 2, 11, 50496, 2),
    (11, 291, 53, 4, 10, 106496, 3),
    (20, 1, 1, 1, 19, 960, 0),  # not reference rows: above BASELINE's k=19 (same single-column shape); k=21 is
    (21, 1, 1, 1, 20, 960, 0),  # the size of the stress config and takes the 15-bit-window MSM path
]
