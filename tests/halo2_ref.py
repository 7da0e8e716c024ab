"""halo2's `create_proof(params, pk, &[c_0 .. c_{N-1}], &[inst_0 .. inst_{N-1}], rng, transcript)` and `verify_proof(.., instances:
&[&[&[Fr]]], ..)` under KZG (`QUERY_INSTANCE = false`) for N >= 1 circuits of one key, with or without ONE instance column,
restated in plain Python over zkoracle primitives [RECALLED: halo2_proofs plonk/{keygen,prover,verifier}.rs, plonk/permutation - no
reference bytes pin it: the reference circuit has one circuit per proof and no public inputs].  The reference of zk_prove_public,
zk_prove_multi, zk_prove_multi_public and the zk_verify* forms (csrc/prover.hip, csrc/prover_lockstep.h, csrc/verifier.h,
csrc/vkrepr.h).  tests/test_halo2_ref.py and tests/test_multi_ref.py tie it to the pinned oracle where they overlap (a shape
without the column: key and proof byte for byte; N = 1: proof byte for byte), to recorded digests of its proofs
(tests/golden/ref_proof_sha256.json) and check that its own verifier accepts and rejects what it should.  The oracle's own keygen,
prover and rendering know neither N nor an instance column and stay untouched.

The rule, c = 0 .. N - 1 in the caller's order, T = terms of one circuit's y-combination, bf = BLINDING_FACTORS:
  shape       the circuit makes the instance column after the chips' columns and enables equality on it: the LAST permutation
              column, [constants.., gate advice.., lookup advice.., instance], queried at rotation 0.  cs.degree(), the blinding
              factors and the chunk length do not change; n_chunks = ceil(#perm columns / chunk_len) may grow by one.
  vk digest   the pinned rendering with num_instance_columns: 1, instance_queries: [(Column { index: 0, column_type: Instance },
              Rotation(0))] and the instance column at the end of permutation: Argument { columns: [..] }
  transcript  transcript_repr; for c: every value of circuit c's list as common_scalar (absorbed, not written; neither N nor the
              lengths are hashed; ALL circuits' instances come before any advice commitment: halo2's loop over `instances` at the
              top of create_proof and verify_proof); for c: advice commitments; theta; for c, per lookup: a', s'; beta, gamma; for
              c: z of every chunk; for c: zL of every lookup; ONE random-polynomial commitment; y; the h pieces; x; evaluations -
              for c: advice in query order; fixed, once; random; sigma, once; for c: per chunk z(x), z(wx) and (not the last
              chunk) z(w^last x); for c, per lookup: zL(x), zL(wx), a'(x), a'(w^-1 x), s'(x) - then the multi-open
  RNG         one stream: for c: (bf + 1) rows per advice column, then n_adv blinds; for c, per lookup: (bf + 1) rows for a',
              (bf + 1) for s', 2 blinds; for c, per chunk: bf rows, 1 blind; for c, per lookup: bf rows, 1 blind; n draws for
              the random polynomial, 1 blind; n_h blinds.  The instance columns draw nothing.
  instances   circuit c's m_c values fill rows 0 .. m_c - 1 of a Lagrange column, the rest is zero; the column is neither blinded
              nor committed, not evaluated into the proof and not opened.  It enters c's permutation grand product as its column's
              values and c's quotient terms as that column's extended coset.  m_c > n - 7 is halo2's InstanceTooLarge; on a shape
              without the column every m_c > 0 is.
  quotient    the y-Horner chain runs on across circuits (term j of circuit c has weight y^(N T - 1 - (c T + j)))
  multi-open  queries: for c: advice queries, per chunk z@0, z@1, then z@last for chunks n_chunks - 2 .. 0, per lookup zL@0, a'@0,
              s'@0, a'@-1, zL@1; then fixed, sigma (over the shape's permutation columns, the instance column's included), h,
              random.  GWC groups by rotation in order of first appearance, SHPLONK by rotation set.
  verifier    absorbs the same values; inst_c(x) = sum_i v_i l_i(x), l_i(x) = w^i (x^n - 1) / (n (x - w^i)), is that column's
              evaluation in circuit c's permutation terms of the expected h(x).

Both kinds of key are taken: a zkoracle.prover.ProvingKey, whose plonk.Shape has no n_inst, and the keys of keygen below.
Commitments are made with the known trusted-setup secret, as the oracle's; the verifier's pairing is the equivalent check with
tau and costs O(1) in n.  Everything is canonical Python ints."""
import copy
import hashlib

from zkoracle import curve as C
from zkoracle import vkrepr
from zkoracle.field import DELTA, R, ZETA, batch_inv, inv, omega
from zkoracle.plonk import (BLINDING_FACTORS, Shape, VerifyingKey, eval_poly, lagrange_evals_at, lagrange_interpolate, make_transcript,
                            msm_points, selector_value, vanishing_eval)
from zkoracle.prover import (Committer, ProvingKey, build_sigma, coeff_to_extended, commit_coeff, extended_to_coeff, kate_division,
                             lagrange_to_coeff, permute_expression_pair)
from zkoracle.srs import TAU

INSTANCE = ("instance", 0)


class InstanceTooLarge(ValueError):
    pass


def public_shape(k, A, L, F, lookup_bits, idle=0, n_inst=1):
    """The oracle's Shape with the instance column as the last permutation column (n_inst = 0: the oracle's Shape itself)."""
    sh = Shape(k, A, L, F, lookup_bits, idle)
    sh.n_inst = n_inst
    assert n_inst in (0, 1)
    if n_inst:
        sh.perm_cols = sh.perm_cols + [INSTANCE]
        sh.n_chunks = (len(sh.perm_cols) + sh.chunk_len - 1) // sh.chunk_len
    return sh


def pinned_debug(sh, fixed_commitments, permutation_commitments):
    """format!("{:?}", vk.pinned()): the oracle's rendering of the shape without the column, with the three changes of the rule."""
    if not sh.n_inst:
        return vkrepr.pinned_debug(sh, fixed_commitments, permutation_commitments)
    base = copy.copy(sh)
    base.perm_cols = sh.perm_cols[:-1]
    s = vkrepr.pinned_debug(base, fixed_commitments, permutation_commitments)
    col = "Column { index: 0, column_type: Instance }"
    for old, new in (("num_instance_columns: 0", "num_instance_columns: 1"),
                     ("instance_queries: []", "instance_queries: [(%s, Rotation(0))]" % col),
                     ("] }, lookups: [", ", %s] }, lookups: [" % col)):
        assert s.count(old) == 1
        s = s.replace(old, new)
    return s


def transcript_repr(sh, fixed_commitments, permutation_commitments):
    s = pinned_debug(sh, fixed_commitments, permutation_commitments).encode()
    h = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
    h.update(len(s).to_bytes(8, "little"))
    h.update(s)
    return int.from_bytes(h.digest(), "little") % R


def keygen(sh, fixed, copies):
    """keygen_vk + keygen_pk over the shape's permutation columns (the instance column included): copies may name it."""
    cm = Committer(sh.k)
    sigma = build_sigma(sh, copies)
    fc = [cm.lagrange(col) for col in fixed]
    pc = [cm.lagrange(col) for col in sigma]
    return ProvingKey(sh, fixed, sigma, VerifyingKey(sh, fc, pc, transcript_repr(sh, fc, pc)))


def instance_column(sh, instances):
    holds = sh.usable_rows if getattr(sh, "n_inst", 0) else 0
    if len(instances) > holds:
        raise InstanceTooLarge("%d instance values, the column holds %d" % (len(instances), holds))
    if any(not 0 <= v < R for v in instances):
        raise ValueError("instance value not below the modulus")
    return list(instances) + [0] * (sh.n - len(instances))


def instance_eval(sh, instances, x):
    """inst(x) = sum_i v_i l_i(x), l_i(x) = w^i (x^n - 1) / (n (x - w^i)), with one batch inversion."""
    if not instances:
        return 0
    w = omega(sh.k)
    wi = [1] * len(instances)
    for i in range(1, len(wi)):
        wi[i] = wi[i - 1] * w % R
    if any((x - p) % R == 0 for p in wi):
        raise ValueError("x on the domain")
    dinv = batch_inv([(x - p) % R for p in wi], R)
    c = (pow(x, sh.n, R) - 1) * inv(sh.n, R) % R
    return sum(v * p % R * d for v, p, d in zip(instances, wi, dinv)) % R * c % R


def quotient_terms(sh):
    return sh.n_gate + 2 + (sh.n_chunks - 1) + sh.n_chunks + 5 * sh.n_lookups


def query_list(sh, N):
    """[(key, rotation)] of the multi-open; keys of a circuit's own polynomials carry the circuit index."""
    q = []
    for c in range(N):
        q += [(("adv", c, col), r) for col, r in sh.advice_queries]
        for ci in range(sh.n_chunks):
            q += [(("z", c, ci), 0), (("z", c, ci), 1)]
        for ci in reversed(range(sh.n_chunks - 1)):
            q.append((("z", c, ci), sh.last_rot))
        for l in range(sh.n_lookups):
            q += [(("lz", c, l), 0), (("la", c, l), 0), (("ls", c, l), 0), (("la", c, l), -1), (("lz", c, l), 1)]
    q += [(("fix", col), r) for col, r in sh.fixed_queries]
    q += [(("sigma", i), 0) for i in range(len(sh.perm_cols))]
    q += [(("h",), 0), (("rand",), 0)]
    return q


def gwc_sets(queries):
    sets = []
    for key, r in queries:
        for s in sets:
            if s[0] == r:
                s[1].append(key)
                break
        else:
            sets.append((r, [key]))
    return sets


def shplonk_sets(queries):
    com_rots = {}
    for key, r in queries:  # (dicts keep the order of first appearance)
        com_rots.setdefault(key, set()).add(r)
    rsets = {}
    for key, rots in com_rots.items():
        rsets.setdefault(frozenset(rots), []).append(key)
    return list(rsets.items())


def create_proof(pk, advices, instances, rng, kind="evm", scheme=None):
    """The proof bytes of N = len(advices) circuits under `pk` with instances[c] the public inputs of circuit c (None: N empty
    lists); rng.fr() = one Fr::random.  A list the column cannot hold raises InstanceTooLarge."""
    scheme = scheme or ("gwc" if kind == "evm" else "shplonk")
    sh = pk.shape
    N = len(advices)
    instances = [[]] * N if instances is None else instances
    assert len(instances) == N, "one instance list per circuit"
    n, k, bf = sh.n, sh.k, BLINDING_FACTORS
    w = omega(k)
    cm = Committer(k)
    insts = [instance_column(sh, vals) for vals in instances]  # per circuit: the column, rows m_c .. n - 1 zero
    tr = make_transcript(kind)
    tr.common_scalar(pk.vk.transcript_repr)
    for vals in instances:  # all circuits' instances, before any commitment
        for v in vals:
            tr.common_scalar(v)
    fixed = pk.fixed

    # -- 1. advice
    advs = []
    for advice in advices:
        adv = [list(col) for col in advice]
        for col in adv:
            for r in range(sh.usable_rows, n):
                col[r] = rng.fr()
        for _ in adv:
            rng.fr()
        advs.append(adv)
    for adv in advs:
        for col in adv:
            tr.write_point(cm.lagrange(col))
    tr.squeeze()  # theta

    # -- 2. lookups
    lks = []
    for adv in advs:
        lk = []
        for l in range(sh.n_lookups):
            inp = [fixed[sh.fx_qlookup][i] * adv[0][i] % R for i in range(n)] if sh.single else adv[sh.n_gate + l][:]
            tab = fixed[sh.fx_table][:]
            ap, sp = permute_expression_pair(inp, tab, sh.usable_rows, rng)
            rng.fr()
            rng.fr()
            lk.append(dict(inp=inp, tab=tab, ap=ap, sp=sp))
        lks.append(lk)
    for lk in lks:
        for d in lk:
            tr.write_point(cm.lagrange(d["ap"]))
            tr.write_point(cm.lagrange(d["sp"]))
    beta = tr.squeeze()
    gamma = tr.squeeze()

    # -- 3. permutation grand products of every circuit: the instance column is a column like the others
    wp = [1] * n
    for i in range(1, n):
        wp[i] = wp[i - 1] * w % R
    zss = []
    for adv, inst in zip(advs, insts):
        col_values = lambda col: fixed[col[1]] if col[0] == "fixed" else inst if col[0] == "instance" else adv[col[1]]
        zs, last_z, d0 = [], 1, 1
        for ci in range(sh.n_chunks):
            cols = sh.perm_cols[ci * sh.chunk_len:(ci + 1) * sh.chunk_len]
            sig = pk.sigma[ci * sh.chunk_len:(ci + 1) * sh.chunk_len]
            den = [1] * n
            for col, s in zip(cols, sig):
                v = col_values(col)
                den = [d * ((beta * s[i] + gamma + v[i]) % R) % R for i, d in enumerate(den)]
            frac = batch_inv(den, R)
            for col in cols:
                v = col_values(col)
                frac = [f * ((d0 * wp[i] % R * beta + gamma + v[i]) % R) % R for i, f in enumerate(frac)]
                d0 = d0 * DELTA % R
            z = [last_z]
            for row in range(1, n):
                z.append(z[row - 1] * frac[row - 1] % R)
            for r in range(n - bf, n):
                z[r] = rng.fr()
            last_z = z[n - (bf + 1)]
            rng.fr()
            zs.append(z)
        zss.append(zs)
    for zs in zss:
        for z in zs:
            tr.write_point(cm.lagrange(z))

    # -- 4. lookup grand products of every circuit
    for lk in lks:
        for d in lk:
            den = [(beta + d["ap"][i]) % R * ((gamma + d["sp"][i]) % R) % R for i in range(n)]
            frac = batch_inv(den, R)
            frac = [frac[i] * ((d["inp"][i] + beta) % R) % R * ((d["tab"][i] + gamma) % R) % R for i in range(n)]
            z = [1]
            for i in range(n - bf - 1):
                z.append(z[-1] * frac[i] % R)
            d["z"] = z[:n - bf] + [rng.fr() for _ in range(bf)]
            rng.fr()
    for lk in lks:
        for d in lk:
            tr.write_point(cm.lagrange(d["z"]))

    # -- 5. ONE random polynomial
    random_poly = [rng.fr() for _ in range(n)]
    rng.fr()
    tr.write_point(commit_coeff(random_poly))
    y = tr.squeeze()

    # -- 6. ONE quotient: the Horner chain runs on across the circuits; the instance column through lagrange_to_coeff and
    #       coeff_to_extended, as an advice column
    ext_k, NE = sh.ext_k, 1 << sh.ext_k
    step = 1 << (ext_k - k)
    coeff = lambda v: lagrange_to_coeff(v, k)
    ext = lambda c: coeff_to_extended(c, k, ext_k)
    fix_c = [coeff(c) for c in fixed]
    sig_c = [coeff(c) for c in pk.sigma]
    fix_e = [ext(c) for c in fix_c]
    sig_e = [ext(c) for c in sig_c]
    P = []  # per circuit: coefficient and coset forms
    for adv, zs, lk, inst in zip(advs, zss, lks, insts):
        d = dict(inst_e=ext(coeff(inst)) if getattr(sh, "n_inst", 0) else None,
                 adv_c=[coeff(c) for c in adv], z_c=[coeff(z) for z in zs],
                 la_c=[coeff(x["ap"]) for x in lk], ls_c=[coeff(x["sp"]) for x in lk], lz_c=[coeff(x["z"]) for x in lk])
        for name in ("adv", "z", "la", "ls", "lz"):
            d[name + "_e"] = [ext(c) for c in d[name + "_c"]]
        P.append(d)
    unit = lambda rows: [1 if i in rows else 0 for i in range(n)]
    l0_e = ext(coeff(unit({0})))
    llast_e = ext(coeff(unit({n - bf - 1})))
    lblind_e = ext(coeff(unit(set(range(n - bf, n)))))
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
            adv_e, z_e = d["adv_e"], d["z_e"]
            inst_e = d["inst_e"]
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
            for e in exprs:
                acc = (acc * y + e) % R
        hvals[i] = acc
    tinv = [inv((pow(xs[i], n, R) - 1) % R, R) for i in range(step)]
    hvals = [hv * tinv[i % step] % R for i, hv in enumerate(hvals)]
    h_coeff = extended_to_coeff(hvals, ext_k)
    assert all(c == 0 for c in h_coeff[n * sh.n_h:]), "quotient degree too high: constraints not satisfied"
    h_pieces = [h_coeff[i * n:(i + 1) * n] for i in range(sh.n_h)]
    for _ in h_pieces:
        rng.fr()
    for hp in h_pieces:
        tr.write_point(commit_coeff(hp))
    x = tr.squeeze()

    # -- 7. evaluations: nothing of the instance columns
    xr = lambda r: x * pow(w, r, R) % R
    xn = pow(x, n, R)
    h_comb = [0] * n
    for hp in reversed(h_pieces):
        h_comb = [(hc * xn + p) % R for hc, p in zip(h_comb, hp)]
    polys = {("h",): h_comb, ("rand",): random_poly}
    for j, c in enumerate(fix_c):
        polys[("fix", j)] = c
    for j, c in enumerate(sig_c):
        polys[("sigma", j)] = c
    for ci_, d in enumerate(P):
        for name in ("adv", "z", "la", "ls", "lz"):
            for j, c in enumerate(d[name + "_c"]):
                polys[(name, ci_, j)] = c
    evals = {}

    def ev(key, r, write=True):
        e = eval_poly(polys[key], xr(r))
        evals[(key, r)] = e
        if write:
            tr.write_scalar(e)

    for c in range(N):
        for col, r in sh.advice_queries:
            ev(("adv", c, col), r)
    for col, r in sh.fixed_queries:
        ev(("fix", col), r)
    ev(("rand",), 0)
    for i in range(len(sig_c)):
        ev(("sigma", i), 0)
    for c in range(N):
        for ci in range(sh.n_chunks):
            ev(("z", c, ci), 0)
            ev(("z", c, ci), 1)
            if ci != sh.n_chunks - 1:
                ev(("z", c, ci), sh.last_rot)
    for c in range(N):
        for l in range(sh.n_lookups):
            ev(("lz", c, l), 0)
            ev(("lz", c, l), 1)
            ev(("la", c, l), 0)
            ev(("la", c, l), -1)
            ev(("ls", c, l), 0)
    ev(("h",), 0, write=False)

    # -- 8. ONE multi-open
    queries = query_list(sh, N)
    if scheme == "gwc":
        v = tr.squeeze()
        for r, keys in gwc_sets(queries):
            pb = [0] * n
            eb = 0
            pv = 1
            for key in keys:
                pb = [(a + pv * b) % R for a, b in zip(pb, polys[key])]
                eb = (eb + pv * evals[(key, r)]) % R
                pv = pv * v % R
            pb[0] = (pb[0] - eb) % R
            tr.write_point(commit_coeff(kate_division(pb, xr(r))))
        return tr.finalize()
    rsets = shplonk_sets(queries)
    all_rots = sorted({r for _, r in queries}, key=xr)
    yc = tr.squeeze()
    v = tr.squeeze()
    low = {}
    hx = [0] * n
    pv = 1
    for rots, keys in rsets:
        rl = sorted(rots, key=xr)
        pts = [xr(r) for r in rl]
        nx = [0] * n
        py = 1
        for key in keys:
            low[key] = lagrange_interpolate(pts, [evals[(key, r)] for r in rl])
            num = polys[key][:]
            for t, c in enumerate(low[key]):
                num[t] = (num[t] - c) % R
            nx = [(a + py * b) % R for a, b in zip(nx, num)]
            py = py * yc % R
        for z in pts:
            nx = kate_division(nx, z)
        nx += [0] * (n - len(nx))
        hx = [(a + pv * b) % R for a, b in zip(hx, nx)]
        pv = pv * v % R
    tr.write_point(commit_coeff(hx))
    u = tr.squeeze()
    lx = [0] * n
    pv = 1
    z_diffs = []
    for rots, keys in rsets:
        zi = vanishing_eval([xr(r) for r in all_rots if r not in rots], u)
        z_diffs.append(zi)
        inner = [0] * n
        py = 1
        for key in keys:
            p = polys[key][:]
            p[0] = (p[0] - eval_poly(low[key], u)) % R
            inner = [(a + py * b) % R for a, b in zip(inner, p)]
            py = py * yc % R
        lx = [(a + pv * zi % R * b) % R for a, b in zip(lx, inner)]
        pv = pv * v % R
    zt = vanishing_eval([xr(r) for r in all_rots], u)
    lx = [(a - zt * b) % R for a, b in zip(lx, hx)]
    assert eval_poly(lx, u) == 0
    z0inv = inv(z_diffs[0], R)
    tr.write_point(commit_coeff([c * z0inv % R for c in kate_division(lx, u)]))
    return tr.finalize()


def verify(vk, proof, instances, kind="evm", scheme=None):
    """True iff `proof` verifies as ONE proof over N = len(instances) circuits of `vk` with instances[c] the public inputs of circuit
    c ([[]] * N: none); the pairing is the equivalent check with tau.  A list the column cannot hold raises InstanceTooLarge
    (halo2's error, not a verdict)."""
    scheme = scheme or ("gwc" if kind == "evm" else "shplonk")
    sh = vk.shape
    N = len(instances)
    for vals in instances:
        instance_column(sh, vals)
    tr = make_transcript(kind, bytes(proof))
    try:
        tr.common_scalar(vk.transcript_repr)
        for vals in instances:
            for v in vals:
                tr.common_scalar(v)
        pts = {}
        for c in range(N):
            for j in range(sh.n_adv):
                pts[("adv", c, j)] = tr.read_point()
        tr.squeeze()  # theta
        for c in range(N):
            for l in range(sh.n_lookups):
                pts[("la", c, l)] = tr.read_point()
                pts[("ls", c, l)] = tr.read_point()
        beta = tr.squeeze()
        gamma = tr.squeeze()
        for c in range(N):
            for ci in range(sh.n_chunks):
                pts[("z", c, ci)] = tr.read_point()
        for c in range(N):
            for l in range(sh.n_lookups):
                pts[("lz", c, l)] = tr.read_point()
        pts[("rand",)] = tr.read_point()
        y = tr.squeeze()
        h_pts = [tr.read_point() for _ in range(sh.n_h)]
        x = tr.squeeze()
        evals = {}
        for c in range(N):
            for col, r in sh.advice_queries:
                evals[(("adv", c, col), r)] = tr.read_scalar()
        for col, r in sh.fixed_queries:
            evals[(("fix", col), r)] = tr.read_scalar()
        evals[(("rand",), 0)] = tr.read_scalar()
        for i in range(len(sh.perm_cols)):
            evals[(("sigma", i), 0)] = tr.read_scalar()
        for c in range(N):
            for ci in range(sh.n_chunks):
                evals[(("z", c, ci), 0)] = tr.read_scalar()
                evals[(("z", c, ci), 1)] = tr.read_scalar()
                if ci != sh.n_chunks - 1:
                    evals[(("z", c, ci), sh.last_rot)] = tr.read_scalar()
        for c in range(N):
            for l in range(sh.n_lookups):
                for key, r in ((("lz", c, l), 0), (("lz", c, l), 1), (("la", c, l), 0), (("la", c, l), -1), (("ls", c, l), 0)):
                    evals[(key, r)] = tr.read_scalar()

        # the expected h(x): the y-Horner of the N x T expressions
        l0, l_last, l_blind, xn = lagrange_evals_at(sh, x)
        active = (1 - l_last - l_blind) % R
        fix = lambda col: evals[(("fix", col), 0)]
        acc = 0
        for c in range(N):
            adv = lambda col, r: evals[(("adv", c, col), r)]
            inst_x = instance_eval(sh, list(instances[c]), x)
            col_eval = lambda col: fix(col[1]) if col[0] == "fixed" else inst_x if col[0] == "instance" else adv(col[1], 0)
            z = lambda ci, r: evals[(("z", c, ci), r)]
            exprs = []
            for j in range(sh.n_gate):
                col, form = sh.gate_sel[j]
                exprs.append(selector_value(form, fix(col)) * (adv(j, 0) + adv(j, 1) * adv(j, 2) - adv(j, 3)))
            exprs.append(l0 * (1 - z(0, 0)))
            zl = z(sh.n_chunks - 1, 0)
            exprs.append(l_last * (zl * zl - zl))
            for ci in range(1, sh.n_chunks):
                exprs.append(l0 * (z(ci, 0) - z(ci - 1, sh.last_rot)))
            for ci in range(sh.n_chunks):
                cols = sh.perm_cols[ci * sh.chunk_len:(ci + 1) * sh.chunk_len]
                left, right = z(ci, 1), z(ci, 0)
                cur = beta * x % R * pow(DELTA, ci * sh.chunk_len, R) % R
                for off, col in enumerate(cols):
                    left = left * ((col_eval(col) + beta * evals[(("sigma", ci * sh.chunk_len + off), 0)] + gamma) % R) % R
                    right = right * ((col_eval(col) + cur + gamma) % R) % R
                    cur = cur * DELTA % R
                exprs.append(active * (left - right))
            for l in range(sh.n_lookups):
                zc, zn = evals[(("lz", c, l), 0)], evals[(("lz", c, l), 1)]
                ap, apm, sp = evals[(("la", c, l), 0)], evals[(("la", c, l), -1)], evals[(("ls", c, l), 0)]
                inp = fix(sh.fx_qlookup) * adv(0, 0) % R if sh.single else adv(sh.n_gate + l, 0)
                tab = fix(sh.fx_table)
                exprs.append(l0 * (1 - zc))
                exprs.append(l_last * (zc * zc - zc))
                exprs.append(active * ((zn * ((ap + beta) % R) % R * ((sp + gamma) % R) - zc * ((inp + beta) % R) % R * ((tab + gamma) % R)) % R))
                exprs.append(l0 * (ap - sp))
                exprs.append(active * ((ap - sp) % R) % R * (ap - apm))
            assert len(exprs) == quotient_terms(sh)
            for e in exprs:
                acc = (acc * y + e) % R
        evals[(("h",), 0)] = acc * inv((xn - 1) % R, R) % R

        for j, p in enumerate(vk.fixed_commitments):
            pts[("fix", j)] = p
        for j, p in enumerate(vk.permutation_commitments):
            pts[("sigma", j)] = p
        pts[("h",)] = msm_points([(pow(xn, i, R), h) for i, h in enumerate(h_pts)])
        w = omega(sh.k)
        pt_of = lambda r: x * pow(w, r, R) % R
        queries = query_list(sh, N)
        if scheme == "gwc":
            v = tr.squeeze()
            sets = gwc_sets(queries)
            ws = [tr.read_point() for _ in sets]
            u = tr.squeeze()
            left, right = [], []
            eval_multi = 0
            pu = 1
            for (r, keys), wi in zip(sets, ws):
                pv, eb = 1, 0
                for key in keys:
                    right.append((pu * pv, pts[key]))
                    eb = (eb + pv * evals[(key, r)]) % R
                    pv = pv * v % R
                eval_multi = (eval_multi + pu * eb) % R
                right.append((pu * pt_of(r), wi))
                left.append((pu, wi))
                pu = pu * u % R
            right.append((-eval_multi, C.G1_GEN))
            lhs, rhs = msm_points(left), msm_points(right)
            ok = rhs == (C.mul(lhs, TAU) if lhs is not None else None)
        else:
            rsets = shplonk_sets(queries)
            all_rots = sorted({r for _, r in queries}, key=pt_of)
            yc = tr.squeeze()
            v = tr.squeeze()
            h1 = tr.read_point()
            u = tr.squeeze()
            h2 = tr.read_point()
            terms = []
            r_outer = 0
            z0 = z0_diff_inv = 0
            pv = 1
            for i, (rots, keys) in enumerate(rsets):
                rl = sorted(rots, key=pt_of)
                ps = [pt_of(r) for r in rl]
                zd = vanishing_eval([pt_of(r) for r in all_rots if r not in rots], u)
                if i == 0:
                    z0 = vanishing_eval(ps, u)
                    z0_diff_inv = inv(zd, R)
                    zd = 1
                else:
                    zd = zd * z0_diff_inv % R
                py, r_inner = 1, 0
                for key in keys:
                    rx = lagrange_interpolate(ps, [evals[(key, r)] for r in rl])
                    r_inner = (r_inner + py * eval_poly(rx, u)) % R
                    terms.append((py * pv % R * zd, pts[key]))
                    py = py * yc % R
                r_outer = (r_outer + pv * r_inner % R * zd) % R
                pv = pv * v % R
            terms += [(-r_outer, C.G1_GEN), (-z0, h1), (u, h2)]
            ok = msm_points(terms) == C.mul(h2, TAU)
        return bool(ok and tr.done())
    except ValueError:
        return False


def proof_offsets(sh, N, kind, scheme=None):
    """The proof length by formula (points before the evaluations, the evaluations, the opening proof) and the byte offsets of the
    places the tests tamper with, by name: the LAST z commitment (the new chunk's where the column starts one), the LAST sigma
    evaluation (the instance column's), and - N >= 2 - places of circuit 1 and of what the circuits share."""
    scheme = scheme or ("gwc" if kind == "evm" else "shplonk")
    ps = 64 if kind == "evm" else 32
    per_pts = sh.n_adv + 3 * sh.n_lookups + sh.n_chunks
    n_pts = N * per_pts + 1 + sh.n_h
    ev0 = n_pts * ps
    n_aq = len(sh.advice_queries)
    n_ev = N * (n_aq + 3 * sh.n_chunks - 1 + 5 * sh.n_lookups) + sh.n_fix + 1 + len(sh.perm_cols)
    z0 = N * n_aq + sh.n_fix + 1 + len(sh.perm_cols)  # evaluations before the first z's
    lk0 = z0 + N * (3 * sh.n_chunks - 1)
    n_open = 2 if scheme == "shplonk" else sh.gwc_sets()
    return {
        "advice commitment of circuit 1": sh.n_adv * ps + 3,
        "last z commitment": (N * (sh.n_adv + 2 * sh.n_lookups + sh.n_chunks) - 1) * ps + 3,
        "h piece": (N * per_pts + 1) * ps + 5,
        "shared fixed evaluation": ev0 + 32 * (N * n_aq) + 7,
        "last sigma evaluation": ev0 + 32 * (z0 - 1) + 7,
        "circuit-1 lookup evaluation": ev0 + 32 * (lk0 + 5 * sh.n_lookups) + 9,
        "last opening": ev0 + 32 * n_ev + (n_open - 1) * ps + 11,
        "length": ev0 + 32 * n_ev + n_open * ps,
        "per circuit": per_pts * ps + 32 * (n_aq + 3 * sh.n_chunks - 1 + 5 * sh.n_lookups),
    }


def proof_size(sh, N, kind, scheme=None):
    return proof_offsets(sh, N, kind, scheme)["length"]
