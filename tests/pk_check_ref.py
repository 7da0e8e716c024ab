"""Plain reference of zk_pk_check (include/zkmi355.h) as a function of a key IMAGE (the zk_pk_write / ProvingKey::write layout):
the image is parsed with zkoracle.serde's restatement of the format, every part is recomputed from its source part as it stands
in the image with zkoracle.fastprover (lagrange_to_coeff, coeff_to_extended, Committer) and the label table delta^c w^r, and the
findings come back in the ABI's order and numbering.  Shares no code with the engine.

    check(shape, image, fmt)            -> (flags, [(part, column, index, count)])
    offset_of(shape, fmt, part, column, index) -> byte offset of that element in the image (what a test overwrites)

Comparison is on the Montgomery images, byte for byte: a non-reduced element (an unchecked file) never equals a recomputed one;
where it is a SOURCE it enters the recomputation as the field element it is an alias of."""
import numpy as np

from zkoracle import cops, fastprover as fp, serde
from zkoracle.field import R, omega
from zkoracle.vkrepr import halo2_fixed_order

(FIXED_COMMIT, SIGMA_COMMIT, FIXED_POLY, SIGMA_POLY, FIXED_COSET, SIGMA_COSET, L_COSET, SIGMA_LABEL, SIGMA_MAP) = range(1, 10)
FIXED_VAL, SIGMA_VAL = "fixed values", "sigma values"  # offset_of only: the audit has no finding "of" a value, values are sources
CHECK_COMMITMENTS, CHECK_POLYS, CHECK_COSETS, CHECK_SIGMA, CHECK_ALL, CHECK_REPR = 1, 2, 4, 8, 15, 16
DELTA = pow(7, 1 << 28, R)  # the permutation argument's coset generator (halo2curves bn256::Fr::DELTA)


def _g1_size(fmt):
    return 32 if fmt == serde.PROCESSED else 64


def vk_len(shape, fmt):
    n_sel = shape.n_gate + (1 if shape.single else 0)
    return 8 + (shape.n_fix + len(shape.perm_cols)) * _g1_size(fmt) + n_sel * (shape.n // 8)


def _layout(shape, fmt):
    """Byte offsets of the image's sections: {name: offset of the section's first polynomial header}, total length."""
    n, N, m, F = shape.n, 4 * shape.n, len(shape.perm_cols), shape.n_fix
    pos = vk_len(shape, fmt)
    at = {"l": pos}
    pos += 3 * (4 + 32 * N)
    for name, cnt, ln in (("fixed_val", F, n), ("fixed_poly", F, n), ("fixed_coset", F, N), ("sigma_val", m, n), ("sigma_poly", m, n),
                          ("sigma_coset", m, N)):
        at[name] = pos + 4  # (the slice's count)
        pos += 4 + cnt * (4 + 32 * ln)
    return at, pos


_SECTION = {FIXED_VAL: ("fixed_val", 1), FIXED_POLY: ("fixed_poly", 1), FIXED_COSET: ("fixed_coset", 4), SIGMA_VAL: ("sigma_val", 1),
            SIGMA_POLY: ("sigma_poly", 1), SIGMA_COSET: ("sigma_coset", 4), SIGMA_LABEL: ("sigma_val", 1), SIGMA_MAP: ("sigma_val", 1)}


def offset_of(shape, fmt, part, column, index=0):
    """Byte offset of element `index` of `column` of `part` in a key image of `shape` in `fmt`.  Fixed columns are numbered in
    the engine's (query) order — the file lists them in halo2's; FIXED_COMMIT / SIGMA_COMMIT: the commitment (index ignored);
    SIGMA_LABEL / SIGMA_MAP: the sigma VALUE (what both are findings about); FIXED_VAL / SIGMA_VAL: the values."""
    at, _ = _layout(shape, fmt)
    fpos = {i: p for p, i in enumerate(halo2_fixed_order(shape))}
    if part == FIXED_COMMIT:
        return 8 + fpos[column] * _g1_size(fmt)
    if part == SIGMA_COMMIT:
        return 8 + (shape.n_fix + column) * _g1_size(fmt)
    if part == L_COSET:
        return at["l"] + column * (4 + 32 * 4 * shape.n) + 4 + 32 * index
    name, mult = _SECTION[part]
    ln = mult * shape.n
    pos = fpos[column] if name.startswith("fixed") else column
    return at[name] + pos * (4 + 32 * ln) + 4 + 32 * index


def _vec(b, pos, ln, fmt):
    assert int.from_bytes(b[pos:pos + 4], "big") == ln
    a = np.frombuffer(b, dtype=np.uint64, count=4 * ln, offset=pos + 4).reshape(ln, 4).copy()
    return cops.to_mont_arr(a) if fmt == serde.PROCESSED else a


def parse(shape, image, fmt):
    """-> dict: fixed_commit / perm_commit (points, query order), l (3 arrays), fixed_val / _poly / _coset, sigma_val / _poly / _coset
    (lists of (len, 4) Montgomery-image arrays, fixed columns in query order)."""
    b = bytes(image)
    at, total = _layout(shape, fmt)
    assert len(b) == total
    n, N, F, m = shape.n, 4 * shape.n, shape.n_fix, len(shape.perm_cols)
    out = {}
    out["fixed_commit"], out["perm_commit"], _ = serde.vk_parse(shape, b[:vk_len(shape, fmt)], fmt)
    out["l"] = [_vec(b, at["l"] + i * (4 + 32 * N), N, fmt) for i in range(3)]
    order = halo2_fixed_order(shape)
    for name, cnt, ln in (("fixed_val", F, n), ("fixed_poly", F, n), ("fixed_coset", F, N), ("sigma_val", m, n), ("sigma_poly", m, n),
                          ("sigma_coset", m, N)):
        assert int.from_bytes(b[at[name] - 4:at[name]], "big") == cnt
        cols = [_vec(b, at[name] + p * (4 + 32 * ln), ln, fmt) for p in range(cnt)]
        if name.startswith("fixed"):
            byq = [None] * cnt
            for p, i in enumerate(order):
                byq[i] = cols[p]
            cols = byq
        out[name] = cols
    return out


def _reduced(a):
    """The same field elements with every image below r (the element a non-reduced image is an alias of)."""
    top = a[:, 3] >= np.uint64(R >> 192)
    if not top.any():
        return a
    a = a.copy()
    for i in np.nonzero(top)[0]:
        v = int.from_bytes(a[i].tobytes(), "little") % R
        a[i] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64)
    return a


def _diff(made, kept):
    """(count, lowest index) of the rows in which two (len, 4) arrays differ."""
    ne = np.nonzero((made != kept).any(axis=1))[0]
    return (int(ne.size), int(ne[0])) if ne.size else (0, 0)


def label_table(shape):
    """{Montgomery image of delta^c w^r (as bytes): (c, r)} over the shape's cells."""
    n, m = shape.n, len(shape.perm_cols)
    w = cops.fr_powers(omega(shape.k), n)
    table = {}
    for c in range(m):
        col = fp.lin(w, pow(DELTA, c, R))
        raw = col.tobytes()
        for r in range(n):
            table[raw[32 * r:32 * r + 32]] = (c, r)
    return table


def check(shape, image, fmt, committer=None):
    """The audit of a key image under the SRS of `committer` (default: the seed-0 setup, zkoracle.fastprover.Committer(k))."""
    # the oracle sizes its thread pools by the machine's processor count; the vectors here are small and a process may be
    # allowed far fewer processors than the machine has, so at most 8 threads for the duration of a check
    saved = fp.NT, fp.NT_FFT, fp.NT_MSM
    fp.NT, fp.NT_FFT, fp.NT_MSM = (min(v, 8) for v in saved)
    try:
        return _check(shape, image, fmt, committer)
    finally:
        fp.NT, fp.NT_FFT, fp.NT_MSM = saved


def _check(shape, image, fmt, committer):
    key = parse(shape, image, fmt)
    cm = committer or fp.Committer(shape.k)
    n, k, m, usable = shape.n, shape.k, len(shape.perm_cols), shape.usable_rows
    found = []
    for part, vals, kept in ((FIXED_COMMIT, key["fixed_val"], key["fixed_commit"]), (SIGMA_COMMIT, key["sigma_val"], key["perm_commit"])):
        for col, v in enumerate(vals):
            if cm.lagrange(_reduced(v)) != kept[col]:
                found.append((part, col, 0, 1))
    for part, src, kept in ((FIXED_POLY, key["fixed_val"], key["fixed_poly"]), (SIGMA_POLY, key["sigma_val"], key["sigma_poly"])):
        for col, v in enumerate(src):
            cnt, low = _diff(fp.lagrange_to_coeff(_reduced(v), k), kept[col])
            if cnt:
                found.append((part, col, low, cnt))
    for part, src, kept in ((FIXED_COSET, key["fixed_poly"], key["fixed_coset"]), (SIGMA_COSET, key["sigma_poly"], key["sigma_coset"])):
        for col, c in enumerate(src):
            cnt, low = _diff(fp.coeff_to_extended(_reduced(c), shape.ext_k), kept[col])
            if cnt:
                found.append((part, col, low, cnt))
    for which, rows in enumerate(([0], [usable], range(usable))):  # l_0, l_last, l_active = 1 on the usable rows
        v = np.zeros((n, 4), dtype=np.uint64)
        v[list(rows)] = fp.m1(1)
        cnt, low = _diff(fp.coeff_to_extended(fp.lagrange_to_coeff(v, k), shape.ext_k), key["l"][which])
        if cnt:
            found.append((L_COSET, which, low, cnt))
    table = label_table(shape)
    named = np.zeros((m, n), dtype=bool)
    bad = [[] for _ in range(m)]
    for c in range(m):
        raw = key["sigma_val"][c].tobytes()
        for r in range(n):
            t = table.get(raw[32 * r:32 * r + 32])
            ok = t is not None and (t[1] < usable if r < usable else t == (c, r))
            if ok:
                named[t] = True
            else:
                bad[c].append(r)
    for c in range(m):
        if bad[c]:
            found.append((SIGMA_LABEL, c, bad[c][0], len(bad[c])))
    for c in range(m):
        miss = np.nonzero(~named[c])[0]
        if miss.size:
            found.append((SIGMA_MAP, c, int(miss[0]), int(miss.size)))
    flags = CHECK_ALL | CHECK_REPR  # (a key read from an image carries the computed transcript_repr)
    for part, *_ in found:
        flags &= ~(CHECK_COMMITMENTS if part <= SIGMA_COMMIT else CHECK_POLYS if part <= SIGMA_POLY else CHECK_COSETS if part <= L_COSET
                   else CHECK_SIGMA)
    return flags, found
