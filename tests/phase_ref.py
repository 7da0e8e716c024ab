"""The provers between the commitments as functions of explicit inputs (tests/test_phase_ref.py,
tests/test_gpu_phase_ops.py): steps 2 to 4 of zkoracle.prover.create_proof lifted out of its transcript flow, so that a test
can hand them any beta, gamma, advice columns and coefficient lists — what a host on the phase-level ABI (zk_lookup_permute,
zk_lookup_product, zk_permutation_product, zk_poly_lincomb, zk_random_poly) is free to do.  Plain Python integers, canonical,
lists over the rows; every inversion is field.batch_inv, whose 0 -> 0 rule is halo2's batch_invert.

Only the rows a device entry point promises are returned: a', s' over rows 0 .. usable - 1, every z over rows 0 .. usable
(usable = n - 7).  Nothing here reads an input row >= usable.

The *_fast functions are the same maps over (n, 4) Montgomery arrays with zkoracle.fastprover's numpy + C primitives, for
the sizes the integer code is too slow at; tests/test_phase_ref.py holds the two against each other."""
from zkoracle import hashes
from zkoracle.field import DELTA, R, batch_inv, omega


def lookup_input(shape, fixed, advice, l):
    """The input expression of lookup l: its lookup advice column, or q_lookup * a_0 for the one-column shape."""
    if shape.single:
        return [q * a % R for q, a in zip(fixed[shape.fx_qlookup], advice[0])]
    return list(advice[shape.n_gate + l])


def permuted_pair(inp, tab, usable):
    """lookup::prover::permute_expression_pair without the blinding draws -> (a', s') over the usable rows.
    ValueError: an input is not in the table (halo2's ConstraintSystemFailure)."""
    a = sorted(inp[:usable])
    left = {}
    for t in tab[:usable]:
        left[t] = left.get(t, 0) + 1
    s = [0] * usable
    repeated = []
    for row, v in enumerate(a):
        if row == 0 or v != a[row - 1]:
            s[row] = v
            if left.get(v, 0) <= 0:
                raise ValueError("lookup input not in table (ConstraintSystemFailure)")
            left[v] -= 1
        else:
            repeated.append(row)
    for t in sorted(left):
        for _ in range(left[t]):
            s[repeated.pop()] = t
    assert not repeated
    return a, s


def _column(shape, fixed, advice, col):
    return fixed[col[1]] if col[0] == "fixed" else advice[col[1]]


def permutation_products(shape, fixed, sigma, advice, beta, gamma):
    """permutation::prover commit: every chunk's z over rows 0 .. usable; chunk c starts from chunk c - 1's value at row usable."""
    usable, w = shape.usable_rows, omega(shape.k)
    wp = [1] * usable
    for i in range(1, usable):
        wp[i] = wp[i - 1] * w % R
    zs = []
    last_z, d0 = 1, 1
    for ci in range(shape.n_chunks):
        lo = ci * shape.chunk_len
        cols = shape.perm_cols[lo:lo + shape.chunk_len]
        den = [1] * usable
        for off, col in enumerate(cols):
            v, s = _column(shape, fixed, advice, col), sigma[lo + off]
            den = [d * ((beta * s[i] + gamma + v[i]) % R) % R for i, d in enumerate(den)]
        frac = batch_inv(den, R)
        for col in cols:
            v = _column(shape, fixed, advice, col)
            frac = [f * ((d0 * wp[i] % R * beta + gamma + v[i]) % R) % R for i, f in enumerate(frac)]
            d0 = d0 * DELTA % R
        z = [last_z]
        for i in range(usable):
            z.append(z[i] * frac[i] % R)
        last_z = z[usable]
        zs.append(z)
    return zs


def lookup_products(shape, fixed, advice, permuted_input, permuted_table, beta, gamma):
    """lookup::prover commit_product: zL of every lookup over rows 0 .. usable."""
    usable = shape.usable_rows
    tab = fixed[shape.fx_table]
    zs = []
    for l in range(shape.n_lookups):
        inp, ap, sp = lookup_input(shape, fixed, advice, l), permuted_input[l], permuted_table[l]
        den = [(beta + ap[i]) % R * ((gamma + sp[i]) % R) % R for i in range(usable)]
        frac = batch_inv(den, R)
        z = [1]
        for i in range(usable):
            z.append(z[i] * frac[i] % R * ((inp[i] + beta) % R) % R * ((tab[i] + gamma) % R) % R)
        zs.append(z)
    return zs


def lincomb(ins, coeffs, sub_low=()):
    """sum_j coeffs[j] * ins[j] - (sub_low[0] + sub_low[1] X + ..): of the low coefficients only those the vectors have."""
    n = len(ins[0])
    out = [0] * n
    for v, c in zip(ins, coeffs):
        assert len(v) == n
        out = [(o + c * x) % R for o, x in zip(out, v)]
    for i, s in enumerate(sub_low[:n]):
        out[i] = (out[i] - s) % R
    return out


def chacha_fr(key, first_block, count):
    """Fr::random of ChaCha20 blocks first_block .. first_block + count - 1 under `key`: from_u512 of the 64 keystream bytes
    (what hashes.ChaCha20Rng.fr draws, at any position of the 64-bit block counter)."""
    return [int.from_bytes(hashes.chacha20_block(key, (first_block + i) & ((1 << 64) - 1)), "little") % R for i in range(count)]


# ---- the same over (n, 4) Montgomery arrays (zkoracle.fastprover's primitives) ----------------------------------------------

def permuted_pair_fast(inp, tab, usable):
    """-> (a', s') as (usable, 4) Montgomery arrays."""
    from zkoracle import fastprover as FP

    a, s = FP.permute_expression_pair(inp, tab, usable, [0] * (inp.shape[0] - usable), [0] * (inp.shape[0] - usable))
    return a[:usable], s[:usable]


def permutation_products_fast(shape, fixed, sigma, advice, beta, gamma):
    """fixed / sigma / advice: lists of (n, 4) Montgomery arrays -> every chunk's z, (usable + 1, 4) Montgomery arrays."""
    from zkoracle import cops, fastprover as FP

    usable = shape.usable_rows
    wp = cops.fr_powers(omega(shape.k), shape.n)[:usable]
    zs = []
    last_z, d0 = 1, 1
    for ci in range(shape.n_chunks):
        lo = ci * shape.chunk_len
        cols = shape.perm_cols[lo:lo + shape.chunk_len]
        vals = [(fixed[c[1]] if c[0] == "fixed" else advice[c[1]])[:usable] for c in cols]
        den = None
        for off, v in enumerate(vals):
            t = FP.lin(sigma[lo + off][:usable], beta, v, 1, gamma)
            den = t if den is None else FP.mul(den, t)
        frac = FP.batch_inv(den)
        for v in vals:
            frac = FP.mul(frac, FP.lin(wp, d0 * beta % R, v, 1, gamma))
            d0 = d0 * DELTA % R
        z = FP.running_product(_extend(frac), last_z)
        last_z = FP.to_int(z[usable])
        zs.append(z)
    return zs


def lookup_products_fast(shape, fixed, advice, permuted_input, permuted_table, beta, gamma):
    from zkoracle import fastprover as FP

    usable = shape.usable_rows
    tab = fixed[shape.fx_table][:usable]
    zs = []
    for l in range(shape.n_lookups):
        inp = FP.mul(fixed[shape.fx_qlookup][:usable], advice[0][:usable]) if shape.single else advice[shape.n_gate + l][:usable]
        den = FP.mul(FP.lin(permuted_input[l][:usable], 1, k=beta), FP.lin(permuted_table[l][:usable], 1, k=gamma))
        frac = FP.batch_inv(den)
        frac = FP.mul(frac, FP.lin(inp, 1, k=beta))
        frac = FP.mul(frac, FP.lin(tab, 1, k=gamma))
        zs.append(FP.running_product(_extend(frac), 1))
    return zs


def _extend(frac):
    """one more row, so that running_product's z has rows 0 .. len(frac)"""
    import numpy as np

    return np.ascontiguousarray(np.concatenate([frac, np.zeros((1, 4), dtype=np.uint64)]))
