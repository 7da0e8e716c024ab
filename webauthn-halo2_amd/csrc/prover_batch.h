// prover_batch.h — create_proof for B independent proofs of ONE key in lock-step on one context (zk_prove_batch).
// Included by prover.hip after `struct Prover`; not a translation unit of its own.
//
// Why: a proof alone is a chain of ~150 launches, most of them small (sort heads, reduction tails, scans, staging); several
// independent pipelines overlap those chains, but each still pays them per proof.  The B proofs of a batch — the reference's
// concurrent requests (proving-server/src/main.rs:457-472), the 256 jobs of BASELINE configs[3] — run the same phase at the
// same time, so the same commitment of all of them goes through ONE MSM pass (one sort head, one accumulation launch over
// B x columns, one reduction tail), the same transform through ONE launch per NTT pass (blockIdx.y), all lookups through
// one set of permutation launches, all grand products through one scan, all openings through one evaluation launch.  What
// stays per proof is chip-filling anyway (quotient, linear combinations, Kate divisions) or host work (transcripts, RNG).
//
// Public inputs (zk_prove_batch_public): every proof has its own validated instance list, absorbed by its own begin() into its own
// transcript; the B instance columns are written by ONE staged upload and ONE launch (instance_columns below) and transformed with
// the lanes' first advice forms.
//
// Every proof keeps its own transcript, its own ChaCha20 stream and its own workspace (zk_pk_rec::members); the bytes of
// proof j are those of zk_prove with the same key, advice and seed (tests/test_gpu_prove_batch.py).  The steps themselves are
// the single prover's (prover_steps.h): this driver holds the schedule of a batch — the per-proof steps looped, the shared ones
// given every proof's workspace at once — and the phase order is Prover::run's.

// the instance columns of every lane of a batch or multi run (a key with the column): ONE staged upload and ONE launch, where the
// lone prover has its memset + copy; every lane's list is its prover's (none: the empty column)
inline int instance_columns(zk_ctx* c, hipStream_t st, zk_pk_rec* pk0, const std::vector<Prover*>& P) {
    if (!pk0->inst_val) return ZK_OK;
    static const std::vector<Fr> none;
    std::vector<zk_pk_rec*> ws;
    std::vector<const std::vector<Fr>*> lists;
    for (Prover* p : P) {
        ws.push_back(p->pk);
        lists.push_back(p->instance ? p->instance : &none);
    }
    return pk_instance_upload_lanes(c, st, pk0, ws, lists);
}
// the columns' coefficient and coset forms ride with the lanes' first advice forms (Prover::with_instance's place)
inline void with_instances(const std::vector<Prover*>& P, std::vector<Prover::Forms>& fm) {
    for (Prover* p : P) p->with_instance(fm);
}

struct BatchRun {
    zk_ctx* c;
    zk_pk_rec* pk0;
    const Layout& lay;
    hipStream_t st;
    uint32_t n, N, B;
    std::vector<Prover*> P;
    BatchBufs& bb;
    uint32_t pass_cap;  // columns per MSM pass
    int rc = ZK_OK;

    BatchRun(const BatchRun&) = delete;  // (cq is bound to this object)
    BatchRun(zk_ctx* c_, zk_pk_rec* pk_, std::vector<Prover*>& provers, uint32_t cap)
        : c(c_), pk0(pk_), lay(pk_->lay), st(c_->stream), n(pk_->lay.n), N(4 * pk_->lay.n), B((uint32_t)provers.size()), P(provers),
          bb(*pk_->bb), pass_cap(cap) {
        for (Prover* p : P) {
            p->rows = &P[0]->own_rows;  // one row stager for all proofs: one upload + one launch per phase
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

    // ---- merged commitments: columns of several proofs in one MSM pass; every point goes to its owner's transcript, in the
    // order the columns were given (per proof that is the transcript's order).  Passes of four or more columns are always split
    // over two lanes (Commits::Batcher: never `loaded`)
    using CQ = Commits<BatchRun>;
    CQ cq{*this};
    using Fifo = CQ::Fifo;
    using Batcher = CQ::Batcher;
    using Col = CommitCol;
    void rows_flush() { P[0]->rows_flush(); }  // (the one row stager of all proofs)
    Batcher batcher(Fifo& f, int basis) { return Batcher{&f, basis, pass_cap, false, {}}; }
    void add(Batcher& b, const Fr* poly, uint32_t owner) { cq.add(b, poly, P[owner]->tr); }
    void transforms(const std::vector<Prover::Forms>& cols) {
        if (!ok()) return;
        P[0]->transforms(cols);  // (flushes the shared row stager first)
    }

    // ------------------------------------------------------------------ run ---
    int run(const Fr* const* advice /* B x n_adv, proof-major */, int scheme) {
        using Forms = Prover::Forms;
        const uint32_t bf = BLINDING_FACTORS, usable = lay.usable;
        for (Prover* p : P)
            if (p->begin()) return p->rc;
        // the three-coset route (poly.hip): every proof's begin() took the same decision; the members read the key's coset-major
        // copies through their own records
        const bool c3 = P[0]->cosets3;
        if (c3 && (rc = pk_ensure_cosets3(c, pk0))) return rc;
        if (int r = instance_columns(c, st, pk0, P)) return r;

        // -- 1. advice
        const bool many = advice_staged(lay);
        for (uint32_t q = 0; q < B; q++) {
            zk_pk_rec* pk = P[q]->pk;
            const Fr* const* adv = advice + (size_t)q * lay.n_adv;
            // (many columns: every proof stages into its own workspace's argument block)
            if (many)
                if (int r = advice_columns_staged(c, st, pk, adv)) return r;
            for (uint32_t j = 0; j < lay.n_adv; j++) {
                if (!many)
                    if (int r = advice_column(c, st, pk, adv, j)) return r;
                P[q]->set_rows(pk->adv_val[j], usable, P[q]->draw(bf + 1));
            }
            P[q]->draw(lay.n_adv);  // advice blinds (unused by KZG, still drawn)
        }
        if (many && aud_sync(c, st) != hipSuccess) return ZK_EHIP;  // the argument staging is reused below
        // one advice column and one lookup per proof (k = 19): the advice pass of all proofs stays in flight on lane 0
        // while the lookup columns are made and committed; otherwise plain order, as Prover::run
        const bool pipe = lay.n_adv == 1 && lay.n_lookups == 1 && B <= pass_cap;
        Fifo af{{0}, {}, nullptr};
        if (pipe) {
            std::vector<Col> cols;
            for (uint32_t q = 0; q < B; q++) cols.push_back(Col{P[q]->pk->adv_val[0], P[q]->tr});
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
                    cols.push_back(Col{pk->adv_val[j], P[q]->tr});
                    fm.push_back(Forms{pk->adv_val[j], pk->adv_poly[j], pk->adv_coset[j]});
                    if (cols.size() == pass_cap) go();
                }
            if (!cols.empty()) go();
            cq.drain(f);
        }
        if (!ok()) return rc;

        // -- 2. lookups: permuted input / table of every lookup of every proof in one set of launches
        std::vector<Fr> theta(B, Fr::zero());
        bool theta_done = false;
        auto squeeze_theta = [&]() {
            if (!theta_done) {
                if (pipe) cq.drain(af);
                for (uint32_t q = 0; q < B; q++) theta[q] = P[q]->tr->squeeze();
                theta_done = true;
            }
        };
        // (no a' / s' commitment reaches a transcript before the proof's advice commitments and theta)
        Fifo lf{pipe ? std::vector<int>{1, 2} : std::vector<int>{0, 1, 2}, {}, squeeze_theta};
        Batcher lb = batcher(lf, ZK_BASIS_LAGRANGE);
        std::vector<Forms> due;
        if (!pipe) squeeze_theta();  // the advice commitments are all written: theta precedes the first a'
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
                P[q]->set_rows(pk->lk_ap[l], usable, P[q]->draw(bf + 1));
                P[q]->set_rows(pk->lk_sp[l], usable, P[q]->draw(bf + 1));
                P[q]->draw(2);
                add(lb, pk->lk_ap[l], q);
                add(lb, pk->lk_sp[l], q);
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
            // one check for all lookups of all proofs (the flag accumulates): an input outside the table is halo2's
            // ConstraintSystemFailure; nothing has been written for the lookups yet.  The batch fails as a whole.
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
        std::vector<Fr> beta(B), gamma(B);
        for (uint32_t q = 0; q < B; q++) {
            beta[q] = P[q]->tr->squeeze();
            gamma[q] = P[q]->tr->squeeze();
        }

        // -- 5 (early). the random polynomials: no challenge needed; their n draws come after the grand products' draws
        Fifo rf{{0}, {}, nullptr};
        {
            const uint64_t skip = (uint64_t)lay.n_chunks * (bf + 1) + (uint64_t)lay.n_lookups * (bf + 1);
            std::vector<Col> cols;
            for (uint32_t q = 0; q < B; q++) {
                ChaChaKey key;
                memcpy(key.w, P[q]->rng.key, 32);
                P[q]->A({}, {P[q]->pk->random_poly}, "random polynomial");
                launch_chacha_fr(key, P[q]->rng.block + skip, P[q]->pk->random_poly, n, st);
                cols.push_back(Col{P[q]->pk->random_poly, P[q]->tr});
            }
            // (more proofs than a pass takes: the surplus random polynomials are committed after the grand products)
            if (B <= pass_cap) cq.begin(rf, cols, ZK_BASIS_MONOMIAL);
        }

        // -- 3. grand products of every proof: numerators / denominators per proof, then ALL scans in one batch
        Fifo zf{{1, 2}, {}, nullptr};
        Batcher zb = batcher(zf, ZK_BASIS_LAGRANGE);
        std::vector<Forms> zdue;
        const uint32_t nprod = lay.n_chunks + lay.n_lookups;
        {
            std::vector<Fr*> zs;
            std::vector<GpGroup> groups;
            const bool many_chunks = lay.n_chunks > BATCH_ARGS_MIN, many_lookups = lay.n_lookups > BATCH_ARGS_MIN;
            if ((many_chunks || many_lookups) && aud_sync(c, st) != hipSuccess) return ZK_EHIP;  // the argument staging may still be in use
            for (uint32_t q = 0; q < B; q++) {
                zk_pk_rec* pk = P[q]->pk;
                if (int r = perm_numden_enqueue(c, st, pk, pk->adv_val.data(), P[q]->tw, beta[q], gamma[q], true)) return r;
                if (many_chunks && many_lookups && aud_sync(c, st) != hipSuccess) return ZK_EHIP;  // the staging is rewritten below
                if (int r = lk_numden_enqueue(c, st, pk, pk->adv_val.data(), pk->lk_ap.data(), pk->lk_sp.data(), beta[q], gamma[q], lay.n_chunks, true,
                                              false))
                    return r;
                zs.insert(zs.end(), pk->z_val.begin(), pk->z_val.end());
                zs.insert(zs.end(), pk->lk_z.begin(), pk->lk_z.end());
            }
            // (a proof's first product starts a new chain)
            for (uint32_t q = 0; q < B; q++) groups.push_back(GpGroup{P[q]->pk, zs.data() + (size_t)q * nprod, nprod, lay.n_chunks});
            if (int r = grand_products(c, st, lay, groups, GpScratch{bb.d_gp_items, bb.gp_scal, bb.gp_host})) return r;
            // blinding rows and commitments, per proof in halo2's order (chunks, then lookups)
            for (uint32_t q = 0; q < B && ok(); q++) {
                zk_pk_rec* pk = P[q]->pk;
                for (uint32_t p = 0; p < nprod && ok(); p++) {
                    Fr* z = zs[q * nprod + p];
                    P[q]->set_rows(z, n - bf, P[q]->draw(bf));
                    P[q]->draw(1);
                    add(zb, z, q);
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

        // -- 5. the random polynomials' commitments (their draws happen here in stream order)
        for (uint32_t q = 0; q < B; q++) {
            P[q]->rng.block += n;
            P[q]->draw(1);
        }
        if (B <= pass_cap) {
            cq.drain(rf);
        } else {
            Fifo f{{0, 1, 2}, {}, nullptr};
            Batcher rb = batcher(f, ZK_BASIS_MONOMIAL);
            for (uint32_t q = 0; q < B; q++) add(rb, P[q]->pk->random_poly, q);
            cq.flush(rb);
            cq.drain(f);
        }
        if (!ok()) return rc;
        std::vector<Fr> y(B);
        for (uint32_t q = 0; q < B; q++) y[q] = P[q]->tr->squeeze();

        // -- 6. quotients: one launch per proof (each fills the chip), then the inverse coset transforms of all in batches
        for (uint32_t q = 0; q < B; q++) {
            if (int r = quotient_of_workspace(c, st, P[q]->pk, c3, beta[q], gamma[q], y[q])) return r;
        }
        if (c3) {
            for (uint32_t q = 0; q < B; q++)
                if (int r = ctx_intt_cosets3(c, P[q]->pk->h_ext, lay.k)) return r;
        } else {
            const uint32_t b2 = ctx_ntt_max_batch(lay.ext_k);
            const Fr* src[NTT_MAX_BATCH];
            Fr* dst[NTT_MAX_BATCH];
            for (uint32_t q0 = 0; q0 < B; q0 += b2) {
                const uint32_t cnt = std::min(b2, B - q0);
                for (uint32_t i = 0; i < cnt; i++) src[i] = dst[i] = P[q0 + i]->pk->h_ext;
                if (int r = ctx_ntt_batch(c, src, N, dst, cnt, lay.ext_k, true, true, N)) return r;
            }
        }
        {
            // the h pieces of every proof: contiguous n-coefficient slices of its quotient
            Fifo hf{{0, 1, 2}, {}, nullptr};
            Batcher hb = batcher(hf, ZK_BASIS_MONOMIAL);
            for (uint32_t q = 0; q < B && ok(); q++) {
                P[q]->draw(lay.n_h);  // h-piece blinds
                for (uint32_t i = 0; i < lay.n_h && ok(); i++) add(hb, P[q]->pk->h_ext + (size_t)i * n, q);
            }
            cq.flush(hb);
            cq.drain(hf);
        }
        if (!ok()) return rc;
        std::vector<Fr> x(B);
        for (uint32_t q = 0; q < B; q++) x[q] = P[q]->tr->squeeze();

        // -- 7. evaluations: every opened value of every proof in ONE launch
        std::vector<std::vector<Prover::Q>> ev(B);
        std::vector<Prover::EvIdx> ix(B);
        std::vector<std::vector<Prover::Q>> queries(B);
        {
            size_t total = 0;
            for (uint32_t q = 0; q < B; q++) {
                P[q]->combine_h(x[q]);
                P[q]->build_evals(ev[q], ix[q]);
                if (ev[q].size() > pk0->max_evals) return ZK_ESTATE;
                for (size_t i = 0; i < ev[q].size(); i++) {
                    bb.h_evargs[total + i].poly = ev[q][i].poly;
                    bb.h_evargs[total + i].x = P[q]->xrot(x[q], ev[q][i].rot);
                }
                total += ev[q].size();
            }
            if (int r = evaluate_enqueue(c, st, EvalBufs{bb.h_evargs, bb.d_evargs, bb.ev_scratch, bb.ev_out, bb.tail_host}, (uint32_t)total, n)) return r;
            size_t pos = 0;
            for (uint32_t q = 0; q < B; q++) {
                for (size_t i = 0; i < ev[q].size(); i++) ev[q][i].eval = bb.tail_host[pos + i];
                pos += ev[q].size();
                for (size_t i = 0; i < ix[q].n_written; i++) P[q]->tr->write_scalar(ev[q][i].eval);
                queries[q] = P[q]->queries_from_evals(ev[q], ix[q]);
                P[q]->pk->lc_used = 0;
            }
        }
        if (!ok()) return rc;

        // -- 8. multi-open: the stages of every proof, the commitments between them merged
        if (scheme == ZK_SCHEME_GWC) {
            Fifo wf{{0, 1, 2}, {}, nullptr};
            Batcher wb = batcher(wf, ZK_BASIS_MONOMIAL);
            for (uint32_t q = 0; q < B && ok(); q++) {
                std::vector<const Fr*> wit;
                if (int r = P[q]->gwc_stage1(queries[q], x[q], wit)) return r;
                for (const Fr* w : wit) add(wb, w, q);
            }
            cq.flush(wb);
            cq.drain(wf);
            return ok() ? ZK_OK : rc;
        }
        std::vector<Prover::Shplonk> S(B);
        Fifo of{{0, 1, 2}, {}, nullptr};
        {
            Batcher ob = batcher(of, ZK_BASIS_MONOMIAL);
            for (uint32_t q = 0; q < B && ok(); q++) {
                if (int r = P[q]->shplonk_stage1(queries[q], x[q], S[q])) return r;
                add(ob, S[q].hx, q);
            }
            cq.flush(ob);
            cq.drain(of);
        }
        if (!ok()) return rc;
        {
            Batcher ob = batcher(of, ZK_BASIS_MONOMIAL);
            for (uint32_t q = 0; q < B && ok(); q++) {
                const Fr* last = nullptr;
                if (int r = P[q]->shplonk_stage2(S[q], &last)) return r;
                add(ob, last, q);
            }
            cq.flush(ob);
            cq.drain(of);
        }
        return ok() ? ZK_OK : rc;
    }
};
