"""The phase-level forms with public inputs and N circuits as functions of explicit inputs (tests/test_phase_public_ref.py,
tests/test_gpu_phase_public.py): step 3 (the permutation grand products, the instance column among their columns) and step 6 (the
ONE quotient over N circuits) of tests/halo2_ref.py `create_proof`, restated a second time outside its transcript flow so that a
test can hand them any beta, gamma, y, columns and instance lists - what a host on zk_permutation_product_public and
zk_quotient_multi is free to do.  The same arrangement as tests/phase_ref.py for the forms without the column; the column itself,
the permutation columns and the transforms are that reference's own (halo2_ref.instance_column, the shape of
halo2_ref.public_shape, zkoracle.prover's transforms).  Plain Python integers, canonical.

Only the rows the device entry points promise are returned for z: rows 0 .. usable (usable = n - 7)."""
from zkoracle.field import DELTA, R, ZETA, batch_inv, inv, omega
from zkoracle.plonk import BLINDING_FACTORS, selector_value
from zkoracle.prover import coeff_to_extended, extended_to_coeff, lagrange_to_coeff

from halo2_ref import instance_column, quotient_terms


def _column(fixed, advice, inst, col):
    return fixed[col[1]] if col[0] == "fixed" else inst if col[0] == "instance" else advice[col[1]]


def permutation_products_public(sh, fixed, sigma, advice, instances, beta, gamma):
    """permutation::prover commit of one circuit with the public inputs `instances` (a list; the shape's column holds them in rows
    0 .. m - 1 and zero behind): every chunk's z over rows 0 .. usable, chunk c starting from chunk c - 1's value at row usable."""
    usable, w = sh.usable_rows, omega(sh.k)
    inst = instance_column(sh, instances)
    wp = [1] * usable
    for i in range(1, usable):
        wp[i] = wp[i - 1] * w % R
    zs, last_z, d0 = [], 1, 1
    for ci in range(sh.n_chunks):
        lo = ci * sh.chunk_len
        cols = sh.perm_cols[lo:lo + sh.chunk_len]
        den = [1] * usable
        for off, col in enumerate(cols):
            v, s = _column(fixed, advice, inst, col), sigma[lo + off]
            den = [d * ((beta * s[i] + gamma + v[i]) % R) % R for i, d in enumerate(den)]
        frac = batch_inv(den, R)
        for col in cols:
            v = _column(fixed, advice, inst, col)
            frac = [f * ((d0 * wp[i] % R * beta + gamma + v[i]) % R) % R for i, f in enumerate(frac)]
            d0 = d0 * DELTA % R
        z = [last_z]
        for i in range(usable):
            z.append(z[i] * frac[i] % R)
        last_z = z[usable]
        zs.append(z)
    return zs


def extended(sh, values):
    """A Lagrange column (n values) on the extended coset: lagrange_to_coeff, then coeff_to_extended."""
    return coeff_to_extended(lagrange_to_coeff(list(values), sh.k), sh.k, sh.ext_k)


def quotient_multi(sh, fixed, sigma, circuits, beta, gamma, y, divide=True):
    """Evaluator::evaluate_h over N = len(circuits) circuits into ONE h on the extended coset (divided by X^n - 1 when `divide`):
    the y-Horner chain runs through circuit 0's expressions, then circuit 1's, ...  circuits[c] = dict(adv=[..], z=[..], ap=[..],
    sp=[..], zl=[..], instances=[..]): Lagrange columns of n rows as the host holds them (blinded rows included) and circuit c's
    public inputs (ignored on a shape without the column)."""
    n, k, bf = sh.n, sh.k, BLINDING_FACTORS
    ext_k, NE = sh.ext_k, 1 << sh.ext_k
    step = 1 << (ext_k - k)
    ext = lambda v: extended(sh, v)
    fix_e = [ext(c) for c in fixed]
    sig_e = [ext(c) for c in sigma]
    P = []
    for d in circuits:
        P.append(dict(inst_e=ext(instance_column(sh, d["instances"])) if getattr(sh, "n_inst", 0) else None,
                      adv_e=[ext(c) for c in d["adv"]], z_e=[ext(c) for c in d["z"]], la_e=[ext(c) for c in d["ap"]],
                      ls_e=[ext(c) for c in d["sp"]], lz_e=[ext(c) for c in d["zl"]]))
    unit = lambda rows: [1 if i in rows else 0 for i in range(n)]
    l0_e = ext(unit({0}))
    llast_e = ext(unit({n - bf - 1}))
    lblind_e = ext(unit(set(range(n - bf, n))))
    wext = omega(ext_k)
    xs = [ZETA] * NE
    for i in range(1, NE):
        xs[i] = xs[i - 1] * wext % R
    rot = lambda vec, i, r: vec[(i + r * step) % NE]
    hvals = [0] * NE
    for i in range(NE):
        acc = 0
        l0, ll, lb = l0_e[i], llast_e[i], lblind_e[i]
        active = (1 - ll - lb) % R
        for d in P:
            exprs = []
            adv_e, z_e, inst_e = d["adv_e"], d["z_e"], d["inst_e"]
            col_e = lambda col: fix_e[col[1]] if col[0] == "fixed" else inst_e if col[0] == "instance" else adv_e[col[1]]
            for j in range(sh.n_gate):
                a, b, c, d4 = (rot(adv_e[j], i, r) for r in range(4))
                col, form = sh.gate_sel[j]
                exprs.append(selector_value(form, fix_e[col][i]) * (a + b * c - d4))
            exprs.append(l0 * (1 - z_e[0][i]))
            zl = z_e[-1][i]
            exprs.append(ll * (zl * zl - zl))
            for ci in range(1, sh.n_chunks):
                exprs.append(l0 * (z_e[ci][i] - rot(z_e[ci - 1], i, sh.last_rot)))
            for ci in range(sh.n_chunks):
                cols = sh.perm_cols[ci * sh.chunk_len:(ci + 1) * sh.chunk_len]
                left = rot(z_e[ci], i, 1)
                for off, col in enumerate(cols):
                    left = left * ((col_e(col)[i] + beta * sig_e[ci * sh.chunk_len + off][i] + gamma) % R) % R
                right = z_e[ci][i]
                cur = beta * xs[i] % R * pow(DELTA, ci * sh.chunk_len, R) % R
                for col in cols:
                    right = right * ((col_e(col)[i] + cur + gamma) % R) % R
                    cur = cur * DELTA % R
                exprs.append(active * (left - right))
            for l in range(sh.n_lookups):
                zc, zn = d["lz_e"][l][i], rot(d["lz_e"][l], i, 1)
                ap, apm, sp = d["la_e"][l][i], rot(d["la_e"][l], i, -1), d["ls_e"][l][i]
                inp = fix_e[sh.fx_qlookup][i] * adv_e[0][i] % R if sh.single else adv_e[sh.n_gate + l][i]
                tab = fix_e[sh.fx_table][i]
                exprs.append(l0 * (1 - zc))
                exprs.append(ll * (zc * zc - zc))
                exprs.append(active * ((zn * ((ap + beta) % R) % R * ((sp + gamma) % R) - zc * ((inp + beta) % R) % R * ((tab + gamma) % R)) % R))
                exprs.append(l0 * (ap - sp))
                exprs.append(active * ((ap - sp) % R) % R * (ap - apm))
            assert len(exprs) == quotient_terms(sh)
            for e in exprs:
                acc = (acc * y + e) % R
        hvals[i] = acc
    if divide:
        tinv = [inv((pow(xs[i], n, R) - 1) % R, R) for i in range(step)]
        hvals = [hv * tinv[i % step] % R for i, hv in enumerate(hvals)]
    return hvals


def h_pieces(sh, hvals):
    """extended_to_coeff of a divided quotient -> its n_h pieces of n coefficients; the coefficients above them (returned second) are
    zero exactly when the columns satisfy the circuit."""
    h_coeff = extended_to_coeff(list(hvals), sh.ext_k)
    n = sh.n
    return [h_coeff[i * n:(i + 1) * n] for i in range(sh.n_h)], h_coeff[n * sh.n_h:]
