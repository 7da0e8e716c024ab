"""One proof over N circuits of one key WITH public inputs, restated in plain Python: halo2's `create_proof(params, pk, &[c_0 ..
c_{N-1}], &[inst_0 .. inst_{N-1}], rng, transcript)` and `verify_proof(.., instances: &[&[&[Fr]]], ..)` with one instance column
per circuit [RECALLED: halo2_proofs plonk/prover.rs, plonk/verifier.rs - no reference bytes pin it].  The reference of
zk_prove_multi_public / zk_verify_multi_public (csrc/prover_lockstep.h, csrc/verifier.h).  It is tests/multi_ref.py's flow with
tests/public_ref.py's column in it; tests/test_multi_public_ref.py ties it to both (N = 1: public_ref.create_proof byte for byte; a
shape without the column: multi_ref.create_proof_multi byte for byte) and checks what its own verifier accepts and rejects.

The rule is multi_ref's (transcript order, ONE RNG stream, the y-Horner chain across circuits, the multi-open) with:
  transcript   transcript_repr; for c = 0 .. N - 1: every value of circuit c's list as common_scalar (absorbed, not written; neither N
               nor the lengths are hashed); then everything else in multi_ref's order.  ALL circuits' instances come before any
               advice commitment: halo2's loop over `instances` at the top of create_proof and verify_proof.
  RNG          the instance columns draw nothing.
  permutation  circuit c's grand product reads c's column (rows 0 .. m_c - 1 its values, zero behind them).
  quotient     circuit c's terms read c's column on the extended coset.
  verifier     circuit c's permutation terms of the expected h(x) use inst_c(x) (public_ref.instance_eval).
Nothing of the columns is committed, evaluated into the proof or opened: the query list is multi_ref.query_list over the shape's
permutation columns, which include the instance column's sigma.  Everything is canonical Python ints."""
from zkoracle import curve as C
from zkoracle.field import DELTA, R, ZETA, batch_inv, inv, omega
from zkoracle.plonk import (BLINDING_FACTORS, eval_poly, lagrange_evals_at, lagrange_interpolate, make_transcript, msm_points,
                            selector_value, vanishing_eval)
from zkoracle.prover import (Committer, coeff_to_extended, commit_coeff, extended_to_coeff, kate_division, lagrange_to_coeff,
                             permute_expression_pair)
from zkoracle.srs import TAU

from multi_ref import gwc_sets, query_list, quotient_terms, shplonk_sets  # (the query list and its grouping are multi_ref's own)
from public_ref import instance_column, instance_eval


def create_proof_multi(pk, advices, instances, rng, kind="evm", scheme=None):
    """The proof bytes of N = len(advices) circuits under `pk` (public_ref.keygen) with instances[c] the public inputs of circuit c;
    rng.fr() = one Fr::random.  A list the column cannot hold raises public_ref.InstanceTooLarge."""
    scheme = scheme or ("gwc" if kind == "evm" else "shplonk")
    sh = pk.shape
    N = len(advices)
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

    # -- 3. permutation grand products of every circuit
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

    # -- 6. ONE quotient: the Horner chain runs on across the circuits
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

    # -- 7. evaluations
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


def verify_multi(vk, proof, instances, kind="evm", scheme=None):
    """True iff `proof` verifies as ONE proof over N = len(instances) circuits of `vk` with instances[c] the public inputs of circuit
    c; the pairing is the equivalent check with tau.  A list the column cannot hold raises InstanceTooLarge (halo2's error, not a
    verdict)."""
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
            inst_x = instance_eval(sh, list(instances[c]), x) if getattr(sh, "n_inst", 0) else 0
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
