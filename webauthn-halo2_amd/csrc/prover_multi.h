// prover_multi.h — create_proof for N circuits under ONE key in ONE proof on one context (zk_prove_multi).
// Included by prover.hip after prover_batch.h; not a translation unit of its own.
//
// Why: halo2's create_proof takes `circuits: &[ConcreteCircuit]`.  N circuits under one key share one transcript, one set of
// challenges, one random polynomial, one quotient and one multi-open: what is paid per circuit is its own columns (advice,
// a', s', z, zL), what is paid once is the random polynomial, the h pieces, the fixed / sigma evaluations and the opening proof
// — 5 N + 7 commitments instead of 12 N at the one-column k = 19 shape with SHPLONK, 11 N + 10 instead of 21 N at the four-column
// k = 17 shape with GWC, one inverse coset transform of h instead of N, and one pairing for the verifier.
//
// The rule [RECALLED] (halo2_proofs plonk/prover.rs `create_proof`, plonk/verifier.rs `verify_proof`; restated in plain Python
// by tests/multi_ref.py, against which the bytes are compared).  c = 0 .. N - 1 in the caller's order, T = quotient_terms(..),
// bf = BLINDING_FACTORS:
//   transcript   transcript_repr (N is not hashed); for c: circuit c's advice commitments; theta; for c, per lookup: a', s';
//                beta, gamma; for c: z of every chunk; for c: zL of every lookup; ONE random-polynomial commitment; y; the h
//                pieces; x; the evaluations — for c: advice in query order; fixed (once); random; sigma (once); for c: per chunk
//                z(x), z(wx) and, but for the last chunk, z(w^last x); for c, per lookup: zL(x), zL(wx), a'(x), a'(w^-1 x), s'(x) —
//                then the multi-open
//   RNG          ONE ChaCha20 stream: for c: (bf + 1) rows per advice column, then n_adv blinds; for c, per lookup: (bf + 1) rows
//                for a', (bf + 1) for s', 2 blinds; for c, per chunk: bf rows, 1 blind; for c, per lookup: bf rows, 1 blind; n draws
//                for the random polynomial, 1 blind; n_h blinds.  N = 1: Prover::run's order
//   quotient     the y-Horner chain runs on across the circuits: term j of circuit c has weight y^(N T - 1 - (c T + j)), so
//                h = sum_c y^(T (N - 1 - c)) h_c with h_c what quotient_row makes of circuit c's columns.  The division by X^n - 1
//                is linear and is applied per pass; the number of h pieces is that of one circuit
//   multi-open   for c: circuit c's advice queries, permutation opens (per chunk z@0, z@1; then z@last for chunks n_chunks - 2 .. 0),
//                lookup opens (per lookup zL@0, a'@0, s'@0, a'@-1, zL@1); after all circuits: fixed, sigma, h, random.  GWC groups
//                this list by rotation in order of first appearance, SHPLONK by rotation set: Prover::gwc_stage1 / shplonk_stage1/2
//                as they stand, on the longer list
//
// With public inputs (zk_prove_multi_public; restated by tests/multi_public_ref.py) the rule gains: behind transcript_repr, for c:
// every value of circuit c's instance list as common_scalar (absorbed, not written; neither N nor the lengths are hashed) — ALL
// circuits' instances before any advice commitment, halo2's loop over `instances` at the top of create_proof.  The columns draw
// nothing; circuit c's grand product reads c's column and quotient pass c its coset forms; nothing of them is committed or opened.
//
// The schedule is BatchRun's: circuit c works in the key's member record c - 1 (zk_pk_rec::members, shared with zk_prove_batch),
// the same commitment of all circuits goes through merged MSM passes, the transforms are batched, all lookups share one set of
// permutation launches, all grand products one scan, all opened values one evaluation launch.  What differs: every point goes to
// the ONE transcript, every draw comes from the ONE stream (circuit 0's prover holds both), the quotient is N passes into circuit
// 0's h_ext — circuit 0 the plain kernel, circuits 1 .. N - 1 the accumulating one (quotient.hip), each with its own powers of y —
// followed by one inverse transform, and the multi-open runs once, from circuit 0's workspace.
//
// Memory: one workspace per circuit (the lock-step batch's: ~1.4 GiB each at k = 19), allocated on first use and kept.

struct MultiRun {
    zk_ctx* c;
    zk_pk_rec* pk0;
    const Layout& lay;
    hipStream_t st;
    uint32_t n, N, B;  // rows; extended rows; circuits
    std::vector<Prover*> P;  // P[0] holds the proof's transcript and RNG; P[q > 0] are workspaces (their own transcripts are scratch)
    Transcript* tr;
    BatchBufs& bb;
    uint32_t pass_cap;  // columns per MSM pass
    int rc = ZK_OK;

    MultiRun(const MultiRun&) = delete;  // (cq is bound to this object)
    MultiRun(zk_ctx* c_, zk_pk_rec* pk_, std::vector<Prover*>& provers, uint32_t cap)
        : c(c_), pk0(pk_), lay(pk_->lay), st(c_->stream), n(pk_->lay.n), N(4 * pk_->lay.n), B((uint32_t)provers.size()), P(provers),
          tr(provers[0]->tr), bb(*pk_->bb), pass_cap(cap) {
        for (Prover* p : P) {
            p->rows = &P[0]->own_rows;  // one row stager for all circuits: one upload + one launch per phase
            p->batch_member = true;
        }
    }

    bool ok() {
        if (rc == ZK_OK)
            for (Prover* p : P)
                if (p->rc != ZK_OK) {
                    rc = p->rc;
                    break;
                }
        return rc == ZK_OK;
    }
    void fail(int code) {
        if (rc == ZK_OK) rc = code;
    }

    // ---- merged commitments (prover_steps.h): every point goes to the one transcript, in the order the columns were given
    using CQ = Commits<MultiRun>;
    CQ cq{*this};
    using Fifo = CQ::Fifo;
    using Batcher = CQ::Batcher;
    using Col = CommitCol;
    void rows_flush() { P[0]->rows_flush(); }
    Batcher batcher(Fifo& f, int basis) { return Batcher{&f, basis, pass_cap, false, {}}; }
    void add(Batcher& b, const Fr* poly) { cq.add(b, poly, tr); }
    void transforms(const std::vector<Prover::Forms>& cols) {
        if (!ok()) return;
        P[0]->transforms(cols);  // (flushes the shared row stager first)
    }
    std::vector<Fr> draw(uint32_t count) { return P[0]->draw(count); }  // the ONE stream

    // ------------------------------------------------------------------ run ---
    int run(const Fr* const* advice /* B x n_adv, circuit-major */, int scheme) {
        using Forms = Prover::Forms;
        using Q = Prover::Q;
        const uint32_t bf = BLINDING_FACTORS, usable = lay.usable;
        // transcript_repr is hashed once: circuit 0's begin() writes it to the proof's transcript, the others' to their scratch.
        // The instance lists (zk_prove_multi_public) are absorbed HERE, once: all circuits' values in circuit order behind
        // transcript_repr and before any advice commitment (halo2's loop over `instances` at the top of create_proof); no begin()
        // absorbs its own, so the scratch transcripts never see a list and nothing is hashed twice
        for (Prover* p : P) {
            p->absorb_instance = false;
            if (p->begin()) return p->rc;
        }
        for (Prover* p : P)
            if (p->instance)
                for (const Fr& v : *p->instance) tr->common_scalar(v);  // (neither N nor the lengths are hashed)
        const bool c3 = P[0]->cosets3;  // (one key, one context, one option: every begin() took the same decision)
        if (c3 && (rc = pk_ensure_cosets3(c, pk0))) return rc;
        if (int r = instance_columns(c, st, pk0, P)) return r;

        // -- 1. advice of every circuit
        const bool many = advice_staged(lay);
        for (uint32_t q = 0; q < B; q++) {
            zk_pk_rec* pk = P[q]->pk;
            const Fr* const* adv = advice + (size_t)q * lay.n_adv;
            if (many)
                if (int r = advice_columns_staged(c, st, pk, adv)) return r;
            for (uint32_t j = 0; j < lay.n_adv; j++) {
                if (!many)
                    if (int r = advice_column(c, st, pk, adv, j)) return r;
                P[q]->set_rows(pk->adv_val[j], usable, draw(bf + 1));
            }
            draw(lay.n_adv);  // advice blinds (unused by KZG, still drawn)
        }
        if (many && aud_sync(c, st) != hipSuccess) return ZK_EHIP;  // the argument staging is reused below
        const bool pipe = lay.n_adv == 1 && lay.n_lookups == 1 && B <= pass_cap;
        Fifo af{{0}, {}, nullptr};
        if (pipe) {
            std::vector<Col> cols;
            for (uint32_t q = 0; q < B; q++) cols.push_back(Col{P[q]->pk->adv_val[0], tr});
            cq.begin(af, cols, ZK_BASIS_LAGRANGE);
        } else {
            Fifo f{{0, 1, 2}, {}, nullptr};
            std::vector<Col> cols;
            std::vector<Forms> fm;
            with_instances(P, fm);  // (with the first pass's transforms)
            auto go = [&]() {
                cq.begin(f, cols, ZK_BASIS_LAGRANGE);
                transforms(fm);
                cols.clear();
                fm.clear();
            };
            for (uint32_t q = 0; q < B && ok(); q++)
                for (uint32_t j = 0; j < lay.n_adv && ok(); j++) {
                    zk_pk_rec* pk = P[q]->pk;
                    cols.push_back(Col{pk->adv_val[j], tr});
                    fm.push_back(Forms{pk->adv_val[j], pk->adv_poly[j], pk->adv_coset[j]});
                    if (cols.size() == pass_cap) go();
                }
            if (!cols.empty()) go();
            cq.drain(f);
        }
        if (!ok()) return rc;

        // -- 2. lookups of every circuit: one set of permutation launches; ONE theta, after the last circuit's advice
        bool theta_done = false;
        auto squeeze_theta = [&]() {
            if (!theta_done) {
                if (pipe) cq.drain(af);
                tr->squeeze();
                theta_done = true;
            }
        };
        Fifo lf{pipe ? std::vector<int>{1, 2} : std::vector<int>{0, 1, 2}, {}, squeeze_theta};
        Batcher lb = batcher(lf, ZK_BASIS_LAGRANGE);
        std::vector<Forms> due;
        if (!pipe) squeeze_theta();
        {
            std::vector<LkItem> items;
            for (uint32_t q = 0; q < B; q++)
                for (uint32_t l = 0; l < lay.n_lookups; l++) {
                    zk_pk_rec* pk = P[q]->pk;
                    items.push_back(LkItem{pk, pk->adv_val.data(), l, pk->lk_ap[l], pk->lk_sp[l]});
                }
            if (int r = lookup_permute(c, st, lay, items, bb.lks)) return r;
        }
        for (uint32_t q = 0; q < B && ok(); q++) {
            zk_pk_rec* pk = P[q]->pk;
            for (uint32_t l = 0; l < lay.n_lookups && ok(); l++) {
                P[q]->set_rows(pk->lk_ap[l], usable, draw(bf + 1));
                P[q]->set_rows(pk->lk_sp[l], usable, draw(bf + 1));
                draw(2);
                add(lb, pk->lk_ap[l]);
                add(lb, pk->lk_sp[l]);
                due.push_back(Forms{pk->lk_ap[l], pk->lk_ap_poly[l], pk->lk_ap_coset[l]});
                due.push_back(Forms{pk->lk_sp[l], pk->lk_sp_poly[l], pk->lk_sp_coset[l]});
                if (lb.pend.empty()) {
                    transforms(due);
                    due.clear();
                }
            }
        }
        cq.flush(lb);
        if (pipe) {
            for (uint32_t q = 0; q < B; q++) due.push_back(Forms{P[q]->pk->adv_val[0], P[q]->pk->adv_poly[0], P[q]->pk->adv_coset[0]});
            with_instances(P, due);
        }
        transforms(due);
        due.clear();
        {
            // one check for all lookups of all circuits: the call fails as a whole, nothing has been written for the lookups yet
            bool bad = false;
            if (int r = lookup_permute_failed(c, st, bb.lks, &bad)) return r;
            if (bad) {
                ctx_msm_drain(c);
                return ZK_EWITNESS;
            }
        }
        squeeze_theta();
        cq.drain(lf);
        if (!ok()) return rc;
        const Fr beta = tr->squeeze();
        const Fr gamma = tr->squeeze();

        // -- 5 (early). the ONE random polynomial: its n draws come after the grand products' draws of every circuit
        const uint32_t nprod = lay.n_chunks + lay.n_lookups;
        Fifo rf{{0}, {}, nullptr};
        {
            const uint64_t skip = (uint64_t)B * nprod * (bf + 1);
            ChaChaKey key;
            memcpy(key.w, P[0]->rng.key, 32);
            P[0]->A({}, {pk0->random_poly}, "random polynomial");
            launch_chacha_fr(key, P[0]->rng.block + skip, pk0->random_poly, n, st);
            cq.begin(rf, {Col{pk0->random_poly, tr}}, ZK_BASIS_MONOMIAL);
        }

        // -- 3. grand products of every circuit: numerators / denominators per circuit, then ALL scans in one batch
        Fifo zf{{1, 2}, {}, nullptr};
        Batcher zb = batcher(zf, ZK_BASIS_LAGRANGE);
        std::vector<Forms> zdue;
        {
            std::vector<Fr*> zs;
            std::vector<GpGroup> groups;
            const bool many_chunks = lay.n_chunks > BATCH_ARGS_MIN, many_lookups = lay.n_lookups > BATCH_ARGS_MIN;
            if ((many_chunks || many_lookups) && aud_sync(c, st) != hipSuccess) return ZK_EHIP;  // the argument staging may still be in use
            for (uint32_t q = 0; q < B; q++) {
                zk_pk_rec* pk = P[q]->pk;
                if (int r = perm_numden_enqueue(c, st, pk, pk->adv_val.data(), P[q]->tw, beta, gamma, true)) return r;
                if (many_chunks && many_lookups && aud_sync(c, st) != hipSuccess) return ZK_EHIP;  // the staging is rewritten below
                if (int r = lk_numden_enqueue(c, st, pk, pk->adv_val.data(), pk->lk_ap.data(), pk->lk_sp.data(), beta, gamma, lay.n_chunks, true, false))
                    return r;
                zs.insert(zs.end(), pk->z_val.begin(), pk->z_val.end());
                zs.insert(zs.end(), pk->lk_z.begin(), pk->lk_z.end());
            }
            // (a circuit's first product starts a new chain)
            for (uint32_t q = 0; q < B; q++) groups.push_back(GpGroup{P[q]->pk, zs.data() + (size_t)q * nprod, nprod, lay.n_chunks});
            if (int r = grand_products(c, st, lay, groups, GpScratch{bb.d_gp_items, bb.gp_scal, bb.gp_host})) return r;
            // blinding rows and commitments in the rule's order: the permutation products of every circuit, then the lookup products
            for (uint32_t part = 0; part < 2; part++)
                for (uint32_t q = 0; q < B && ok(); q++) {
                    zk_pk_rec* pk = P[q]->pk;
                    const uint32_t p0 = part ? lay.n_chunks : 0, p1 = part ? nprod : lay.n_chunks;
                    for (uint32_t p = p0; p < p1 && ok(); p++) {
                        Fr* z = zs[q * nprod + p];
                        P[q]->set_rows(z, n - bf, draw(bf));
                        draw(1);
                        add(zb, z);
                        if (p < lay.n_chunks) zdue.push_back(Forms{pk->z_val[p], pk->z_poly[p], pk->z_coset[p]});
                        else zdue.push_back(Forms{pk->lk_z[p - lay.n_chunks], pk->lk_z_poly[p - lay.n_chunks], pk->lk_z_coset[p - lay.n_chunks]});
                        if (zb.pend.empty()) {
                            transforms(zdue);
                            zdue.clear();
                        }
                    }
                }
        }
        cq.flush(zb);
        transforms(zdue);
        zdue.clear();
        cq.drain(zf);
        if (!ok()) return rc;

        // -- 5. the random polynomial's commitment (its draws happen here in stream order)
        P[0]->rng.block += n;
        draw(1);
        cq.drain(rf);
        if (!ok()) return rc;
        const Fr y = tr->squeeze();

        // -- 6. the quotient: N passes into circuit 0's h_ext (the y-Horner chain runs on across the circuits: pass q carries
        // y^(T (N - 1 - q)); circuit 0 stores, the others accumulate), ONE inverse transform, ONE set of h pieces
        {
            const uint32_t T = quotient_terms(lay.n_gate, lay.n_chunks, lay.n_lookups);
            const Fr yT = fr_pow(y, T);
            std::vector<Fr> scale(B);
            scale[B - 1] = Fr::one();
            for (uint32_t q = B - 1; q-- > 0;) scale[q] = fe_mul(scale[q + 1], yT);
            for (uint32_t q = 0; q < B; q++)
                if (int r = quotient_pass_of_workspace(c, st, P[q]->pk, c3, beta, gamma, y, pk0->h_ext, scale[q], q > 0)) return r;
            if (int r = c3 ? ctx_intt_cosets3(c, pk0->h_ext, lay.k) : ctx_ntt(c, pk0->h_ext, N, pk0->h_ext, lay.ext_k, true, true, N)) return r;
        }
        draw(lay.n_h);  // h-piece blinds
        {
            Fifo hf{{0, 1, 2}, {}, nullptr};
            Batcher hb = batcher(hf, ZK_BASIS_MONOMIAL);
            for (uint32_t i = 0; i < lay.n_h && ok(); i++) add(hb, pk0->h_ext + (size_t)i * n);
            cq.flush(hb);
            cq.drain(hf);
        }
        if (!ok()) return rc;
        const Fr x = tr->squeeze();

        // -- 7. evaluations: every opened value in ONE launch — the circuits' own, and ONCE the fixed, sigma, random and h
        // polynomials — in transcript order, then h(x) (not written)
        P[0]->combine_h(x);
        std::vector<Q> ev;
        std::vector<size_t> i_adv(B), i_z(B), i_lk(B);
        size_t i_fix, i_rand, i_sig, n_written;
        for (uint32_t q = 0; q < B; q++) {
            i_adv[q] = ev.size();
            for (auto& aq : lay.advice_queries) ev.push_back(Q{P[q]->pk->adv_poly[aq.first], aq.second, Fr::zero()});
        }
        i_fix = ev.size();
        for (uint32_t f = 0; f < lay.n_fix; f++) ev.push_back(Q{pk0->fixed_poly[f], 0, Fr::zero()});
        i_rand = ev.size();
        ev.push_back(Q{pk0->random_poly, 0, Fr::zero()});
        i_sig = ev.size();
        for (uint32_t p = 0; p < lay.perm_cols.size(); p++) ev.push_back(Q{pk0->sigma_poly[p], 0, Fr::zero()});
        for (uint32_t q = 0; q < B; q++) {
            i_z[q] = ev.size();
            for (uint32_t ci = 0; ci < lay.n_chunks; ci++) {
                ev.push_back(Q{P[q]->pk->z_poly[ci], 0, Fr::zero()});
                ev.push_back(Q{P[q]->pk->z_poly[ci], 1, Fr::zero()});
                if (ci != lay.n_chunks - 1) ev.push_back(Q{P[q]->pk->z_poly[ci], lay.last_rot, Fr::zero()});
            }
        }
        for (uint32_t q = 0; q < B; q++) {
            i_lk[q] = ev.size();
            for (uint32_t l = 0; l < lay.n_lookups; l++) {
                zk_pk_rec* pk = P[q]->pk;
                ev.push_back(Q{pk->lk_z_poly[l], 0, Fr::zero()});
                ev.push_back(Q{pk->lk_z_poly[l], 1, Fr::zero()});
                ev.push_back(Q{pk->lk_ap_poly[l], 0, Fr::zero()});
                ev.push_back(Q{pk->lk_ap_poly[l], -1, Fr::zero()});
                ev.push_back(Q{pk->lk_sp_poly[l], 0, Fr::zero()});
            }
        }
        n_written = ev.size();
        ev.push_back(Q{pk0->h_comb, 0, Fr::zero()});
        if (ev.size() > (size_t)bb.cap * pk0->max_evals) return ZK_ESTATE;  // (the shared buffers hold cap x one proof's openings)
        for (size_t i = 0; i < ev.size(); i++) {
            bb.h_evargs[i].poly = ev[i].poly;
            bb.h_evargs[i].x = P[0]->xrot(x, ev[i].rot);
        }
        if (int r = evaluate_enqueue(c, st, EvalBufs{bb.h_evargs, bb.d_evargs, bb.ev_scratch, bb.ev_out, bb.tail_host}, (uint32_t)ev.size(), n)) return r;
        for (size_t i = 0; i < ev.size(); i++) ev[i].eval = bb.tail_host[i];
        for (size_t i = 0; i < n_written; i++) tr->write_scalar(ev[i].eval);
        if (!ok()) return rc;

        // the query list of the multi-open: per circuit what Prover::queries_from_evals lists for one, then the shared tail
        std::vector<Q> queries;
        for (uint32_t q = 0; q < B; q++) {
            for (size_t i = 0; i < lay.advice_queries.size(); i++) queries.push_back(ev[i_adv[q] + i]);
            std::vector<Q> lastq(lay.n_chunks);
            size_t pos = i_z[q];
            for (uint32_t ci = 0; ci < lay.n_chunks; ci++) {
                queries.push_back(ev[pos++]);
                queries.push_back(ev[pos++]);
                if (ci != lay.n_chunks - 1) lastq[ci] = ev[pos++];
            }
            for (int ci = (int)lay.n_chunks - 2; ci >= 0; ci--) queries.push_back(lastq[ci]);
            pos = i_lk[q];
            for (uint32_t l = 0; l < lay.n_lookups; l++, pos += 5) {
                queries.push_back(ev[pos]);      // zL @ x
                queries.push_back(ev[pos + 2]);  // a' @ x
                queries.push_back(ev[pos + 4]);  // s' @ x
                queries.push_back(ev[pos + 3]);  // a' @ w^-1 x
                queries.push_back(ev[pos + 1]);  // zL @ w x
            }
        }
        for (size_t i = i_fix; i < i_rand; i++) queries.push_back(ev[i]);
        for (size_t i = i_sig; i < i_z[0]; i++) queries.push_back(ev[i]);
        queries.push_back(ev[n_written]);  // h
        queries.push_back(ev[i_rand]);     // random polynomial

        // -- 8. ONE multi-open over the concatenated list, from circuit 0's workspace (its stages as they stand; the commitments
        // between them through this driver's queue)
        pk0->lc_used = 0;
        Prover& p0 = *P[0];
        if (scheme == ZK_SCHEME_GWC) {
            std::vector<const Fr*> wit;
            if (int r = p0.gwc_stage1(queries, x, wit)) return r;
            Fifo wf{{0, 1, 2}, {}, nullptr};
            Batcher wb = batcher(wf, ZK_BASIS_MONOMIAL);
            for (const Fr* w : wit) add(wb, w);
            cq.flush(wb);
            cq.drain(wf);
            return ok() ? ZK_OK : rc;
        }
        Prover::Shplonk S;
        Fifo of{{0}, {}, nullptr};
        if (int r = p0.shplonk_stage1(queries, x, S)) return r;
        cq.begin(of, {Col{S.hx, tr}}, ZK_BASIS_MONOMIAL);
        cq.drain(of);
        if (!ok()) return rc;
        const Fr* last = nullptr;
        if (int r = p0.shplonk_stage2(S, &last)) return r;
        cq.begin(of, {Col{last, tr}}, ZK_BASIS_MONOMIAL);
        cq.drain(of);
        return ok() ? ZK_OK : rc;
    }
};
