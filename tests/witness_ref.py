"""Plain-Python reference of zk_witness_check (include/zkmi355.h): what MockProver::verify reports for the circuit family of
this engine.  Gates and lookups by direct evaluation; copies by inverting the ORACLE's sigma values
(zkoracle.prover.build_sigma) through a dictionary {delta^c w^r -> (c, r)}.  Shares no code with the engine.

A failure is a tuple (kind, index, row, other_index, other_row); `check` returns them in ascending order — the order of the
engine's list."""
from zkoracle import plonk, prover
from zkoracle.field import R, omega

GATE, GATE_BLINDED, LOOKUP, COPY = 1, 2, 3, 4
DELTA = pow(7, 1 << 28, R)  # the permutation argument's coset generator (halo2curves bn256::Fr::DELTA)


def shape_of(t):
    """plonk.Shape of a prover_shapes tuple (A, L, F, k, lookup_bits[, idle])."""
    A, L, F, k, lb, idle = (tuple(t) + (0,))[:6]
    return plonk.Shape(k, A, L, F, lb, idle)


def effective_selector(shape, fixed, j, r):
    """Gate j's selector on row r after compress_selectors: q, q (2 - q) or q (1 - q) (plonk.Shape.gate_sel)."""
    col, form = shape.gate_sel[j]
    q = fixed[col][r] % R
    return q if form == 0 else q * ((2 if form == 1 else 1) - q) % R


def gate_failure(shape, fixed, advice, j, r):
    """The failure of gate column j on row r, or None."""
    if effective_selector(shape, fixed, j, r) == 0:
        return None
    if r + 3 >= shape.usable_rows:
        return (GATE_BLINDED, j, r, 0, 0)
    a = advice[j]
    return (GATE, j, r, 0, 0) if (a[r] + a[r + 1] * a[r + 2] - a[r + 3]) % R else None


def gate_failures_around(shape, fixed, advice, j, row):
    """The failures among the (at most four) gate windows of column j that contain `row`."""
    out = [gate_failure(shape, fixed, advice, j, r) for r in range(max(0, row - 3), row + 1)]
    return sorted(f for f in out if f)


def lookup_failures_at(shape, fixed, advice, j, r):
    """The lookup failures that read advice cell (j, r)."""
    T = 1 << shape.lookup_bits
    if r >= shape.usable_rows:
        return []
    if shape.single:
        return [(LOOKUP, 0, r, 0, 0)] if fixed[shape.fx_qlookup][r] * advice[0][r] % R >= T else []
    return [(LOOKUP, j - shape.n_gate, r, 0, 0)] if j >= shape.n_gate and advice[j][r] % R >= T else []


def label_table(shape):
    n, w = shape.n, omega(shape.k)
    inv = {}
    for c in range(len(shape.perm_cols)):
        v = pow(DELTA, c, R)
        for r in range(n):
            inv[v] = (c, r)
            v = v * w % R
    return inv


def cell_value(shape, fixed, advice, c, r):
    kind, i = shape.perm_cols[c]
    return (fixed[i][r] if kind == "fixed" else advice[i][r]) % R


def check(shape, fixed, copies, advice, sigma=None):
    usable, T = shape.usable_rows, 1 << shape.lookup_bits
    out = []
    for j in range(shape.n_gate):
        for r in range(shape.n):
            f = gate_failure(shape, fixed, advice, j, r)
            if f:
                out.append(f)
    for l in range(shape.n_lookups):
        for r in range(usable):
            v = fixed[shape.fx_qlookup][r] * advice[0][r] % R if shape.single else advice[shape.n_gate + l][r] % R
            if v >= T:
                out.append((LOOKUP, l, r, 0, 0))
    sigma = prover.build_sigma(shape, copies) if sigma is None else sigma
    inv = label_table(shape)
    for c in range(len(shape.perm_cols)):
        for r in range(usable):
            c2, r2 = inv[sigma[c][r]]
            if (c2, r2) != (c, r) and cell_value(shape, fixed, advice, c, r) != cell_value(shape, fixed, advice, c2, r2):
                out.append((COPY, c, r, c2, r2))
    return sorted(out)


def counts(failures):
    c = [len(failures), 0, 0, 0, 0]
    for f in failures:
        c[f[0]] += 1
    return c
