// prover_lockstep.h — create_proof, the ONE driver: B lanes of ONE key in lock-step on one context.  One lane is zk_prove /
// zk_prove_public; several are B independent proofs (zk_prove_batch) or ONE proof over B circuits (zk_prove_multi).  One schedule;
// the lane count and the mode are fixed at construction.  Included by prover.hip after `struct Prover`; not a translation unit of
// its own.
//
// Why lock-step: a proof alone is a chain of ~150 launches, most of them small (sort heads, reduction tails, scans, staging); several
// independent pipelines overlap those chains, but each still pays them per proof.  The B proofs of a batch — the reference's
// concurrent requests (proving-server/src/main.rs:457-472), the 256 jobs of BASELINE configs[3] — run the same phase at the
// same time, so the same commitment of all of them goes through ONE MSM pass (one sort head, one accumulation launch over
// B x columns, one reduction tail), the same transform through ONE launch per NTT pass (blockIdx.y), all lookups through
// one set of permutation launches, all grand products through one scan, all opened values through one evaluation launch.  What
// stays per lane is chip-filling anyway (quotient, linear combinations, Kate divisions) or host work (transcripts, RNG).
// The steps themselves are prover_steps.h's and Prover's (prover.hip): this driver holds the schedule — which step, in which order,
// on which MSM lane, when a lane is collected and when the host waits; the per-lane steps looped, the shared ones given every
// lane's workspace at once.  Lane 0 works in the key's own workspace, lane q > 0 in the key's member record q - 1
// (zk_pk_rec::members: ~1.4 GiB each at k = 19, allocated on first use and kept).
//
// B proofs: every proof keeps its own transcript, its own ChaCha20 stream and its own workspace; the bytes of proof j are those of
// zk_prove with the same key, advice and seed (tests/test_gpu_prove_batch.py).  With public inputs (zk_prove_batch_public) every
// proof has its own validated instance list, absorbed by its own begin() into its own transcript.
//
// One proof over B circuits: halo2's create_proof takes `circuits: &[ConcreteCircuit]`.  N circuits under one key share one
// transcript, one set of challenges, one random polynomial, one quotient and one multi-open: what is paid per circuit is its own
// columns (advice, a', s', z, zL), what is paid once is the random polynomial, the h pieces, the fixed / sigma evaluations and the
// opening proof — 5 N + 7 commitments instead of 12 N at the one-column k = 19 shape with SHPLONK, 11 N + 10 instead of 21 N at the
// four-column k = 17 shape with GWC, one inverse coset transform of h instead of N, and one pairing for the verifier.
//
// The rule [RECALLED] (halo2_proofs plonk/prover.rs `create_proof`, plonk/verifier.rs `verify_proof`; restated in plain Python
// by tests/halo2_ref.py, against which the bytes are compared).  c = 0 .. N - 1 in the caller's order, T = quotient_terms(..),
// bf = BLINDING_FACTORS:
//   transcript   transcript_repr (N is not hashed); for c: circuit c's advice commitments; theta; for c, per lookup: a', s';
//                beta, gamma; for c: z of every chunk; for c: zL of every lookup; ONE random-polynomial commitment; y; the h
//                pieces; x; the evaluations — for c: advice in query order; fixed (once); random; sigma (once); for c: per chunk
//                z(x), z(wx) and, but for the last chunk, z(w^last x); for c, per lookup: zL(x), zL(wx), a'(x), a'(w^-1 x), s'(x) —
//                then the multi-open
//   RNG          ONE ChaCha20 stream: for c: (bf + 1) rows per advice column, then n_adv blinds; for c, per lookup: (bf + 1) rows
//                for a', (bf + 1) for s', 2 blinds; for c, per chunk: bf rows, 1 blind; for c, per lookup: bf rows, 1 blind; n draws
//                for the random polynomial, 1 blind; n_h blinds
//   quotient     the y-Horner chain runs on across the circuits: term j of circuit c has weight y^(N T - 1 - (c T + j)), so
//                h = sum_c y^(T (N - 1 - c)) h_c with h_c what quotient_row makes of circuit c's columns.  The division by X^n - 1
//                is linear and is applied per pass; the number of h pieces is that of one circuit
//   multi-open   for c: circuit c's advice queries, permutation opens (per chunk z@0, z@1; then z@last for chunks n_chunks - 2 .. 0),
//                lookup opens (per lookup zL@0, a'@0, s'@0, a'@-1, zL@1); after all circuits: fixed, sigma, h, random.  GWC groups
//                this list by rotation in order of first appearance, SHPLONK by rotation set: Prover::gwc_stage1 / shplonk_stage1/2
//                as they stand, on the longer list (Prover::build_evals / queries_from_evals state both orders, for 1 and for N)
// This is the one statement of the order: a lone proof is N = 1.
// With public inputs (zk_prove_multi_public; restated by the same tests/halo2_ref.py) the rule gains: behind transcript_repr, for c:
// every value of circuit c's instance list as common_scalar (absorbed, not written; neither N nor the lengths are hashed) — ALL
// circuits' instances before any advice commitment, halo2's loop over `instances` at the top of create_proof.  The columns draw
// nothing; circuit c's grand product reads c's column and quotient pass c its coset forms; nothing of them is committed or opened.
//
// Where the modes differ, and nowhere else: WHO OWNS the transcript, the RNG stream and the challenges — each lane (B proofs), or
// lane 0 for all (one proof: P[q > 0] are workspaces, their own transcripts scratch, their streams never drawn from).  The
// schedule below is written over `proofs()` proofs of `lanes_end(p) - p` circuits each — B of one, or one of B — and reads the
// owner through tr_of / draw / squeeze; phases 1 - 3 loop over the lanes alike.  What only one mode has (the instances absorbed
// by the driver, the quotient accumulated over the circuits, the limit of the evaluation list, the lane of the SHPLONK
// commitments) is a branch on `one`, each with its reason.
//
// Where ONE lane differs from several — a lone proof has the context to itself, a member of a batch shares it — is a branch on
// `lone`, each with its reason: the shared buffers (LaneBufs), the instance upload, the side streams (Prover::batch_member, and
// with it the early advice transforms and the quotient), the split of wide passes, and two places where the host waits.  The
// pass width is the caller's (prove_one: the context's own; prove_lockstep: the lock-step rule).

// the buffers of the launches that all lanes share: one lane has the key's own, several the key's BatchBufs (sized for `cap`
// proofs; null on a key that has never seen a batch)
struct LaneBufs {
    LookupScratch lks;
    GpScratch gp;
    EvalBufs ev;
    size_t max_evals;  // what `ev` holds
    LaneBufs(const zk_pk_rec* pk, bool lone, bool one_proof) {
        if (lone) {
            lks = pk->lks;
            gp = GpScratch{pk->d_gp_items, pk->gp_scal, pk->gp_host};
            ev = EvalBufs{pk->h_evargs, pk->d_evargs, pk->ev_scratch, pk->ev_out, pk->tail_host};
            max_evals = pk->max_evals;
        } else {
            const BatchBufs& bb = *pk->bb;
            lks = bb.lks;
            gp = GpScratch{bb.d_gp_items, bb.gp_scal, bb.gp_host};
            ev = EvalBufs{bb.h_evargs, bb.d_evargs, bb.ev_scratch, bb.ev_out, bb.tail_host};
            // (cap x one proof's openings: B proofs share them, the one proof has them all)
            max_evals = one_proof ? (size_t)bb.cap * pk->max_evals : pk->max_evals;
        }
    }
};

struct LockstepRun {
    zk_ctx* c;
    zk_pk_rec* pk0;
    const Layout& lay;
    hipStream_t st;
    uint32_t n, N, B;  // rows; extended rows; lanes: the proofs, or the circuits of the one proof
    std::vector<Prover*> P;
    const bool one;   // ONE proof over the B circuits (P[0] holds its transcript and RNG); otherwise B proofs
    const bool lone;  // one lane: the lone proof
    LaneBufs bufs;
    uint32_t pass_cap;  // columns per MSM pass
    int rc = ZK_OK;

    LockstepRun(const LockstepRun&) = delete;  // (cq is bound to this object)
    LockstepRun(zk_ctx* c_, zk_pk_rec* pk_, const std::vector<Prover*>& provers, bool one_proof, uint32_t cap)
        : c(c_), pk0(pk_), lay(pk_->lay), st(c_->stream), n(pk_->lay.n), N(4 * pk_->lay.n), B((uint32_t)provers.size()), P(provers),
          one(one_proof), lone(provers.size() == 1), bufs(pk_, lone, one_proof), pass_cap(cap) {
        for (Prover* p : P) {
            p->rows = &P[0]->own_rows;  // one row stager for all lanes: one upload + one launch per phase
            p->batch_member = !lone;    // (a lone proof may take the side streams: Prover::begin)
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

    // ---- what the mode decides.  Proof p's lanes are p .. lanes_end(p) - 1 and its prover — transcript, RNG, multi-open — is P[p]
    uint32_t proofs() const { return one ? 1 : B; }
    uint32_t lanes_end(uint32_t p) const { return one ? B : p + 1; }
    Prover& owner(uint32_t q) { return *P[one ? 0 : q]; }
    Transcript* tr_of(uint32_t q) { return owner(q).tr; }                                // lane q's transcript, or the one
    std::vector<Fr> draw(uint32_t q, uint32_t count) { return owner(q).draw(count); }  // lane q's stream, or the one
    // a challenge for every lane: each proof's own, or the one squeezed once
    std::vector<Fr> squeeze() {
        std::vector<Fr> ch(B);
        for (uint32_t p = 0; p < proofs(); p++) {
            const Fr v = P[p]->tr->squeeze();
            for (uint32_t q = p; q < lanes_end(p); q++) ch[q] = v;
        }
        return ch;
    }

    // ---- commitments in flight over MSM lanes, collected — written to their transcripts — in the order they were begun: columns
    // of several lanes in one MSM pass; every point goes to its owner's transcript, in the order the columns were given (per
    // proof that is the transcript's order).  The staged blinding rows of the columns about to be read go up first
    struct Commits {
        LockstepRun& d;
        struct Pass {
            int lane;
            std::vector<Transcript*> to;
        };
        // a set of lanes used in turn; a one-lane queue is a commitment begun on a fixed lane and collected later (drain)
        struct Fifo {
            std::vector<int> lanes;
            std::deque<Pass> busy;
            // run before a pass of this queue is collected: what the transcripts must hold first (the lookup passes of a pipelined
            // proof may fill their lanes while the advice pass is still in flight on its own)
            std::function<void()> before_collect;
        };
        // gathers columns into passes of at most `cap`; flush() begins what is pending.  A pass of four or more columns goes as two
        // passes on two lanes — the first half's reduction tail runs under the second half's head — unless `loaded`: that pays only
        // while the tails have a stream of their own (a lone proof, two pipelines); under load — tails on the main stream — a second
        // pass is just a second head and tail (k = 17 EVM over four pipelines: 232.9 -> 236.9 proofs/s unsplit)
        struct Batcher {
            Fifo* f;
            int basis;
            uint32_t cap;
            bool loaded;
            std::vector<CommitCol> pend;
        };

        void begin(Fifo& f, const std::vector<CommitCol>& cols, int basis) {
            if (!d.ok() || cols.empty()) return;
            if (f.busy.size() == f.lanes.size()) {
                if (f.before_collect) f.before_collect();
                end_write(f.busy.front());
                f.busy.pop_front();
            }
            int lane = -1;
            for (int l : f.lanes) {
                bool used = false;
                for (const Pass& ps : f.busy) used = used || ps.lane == l;
                if (!used) lane = l;
            }
            d.rows_flush();
            if (!d.ok()) return;
            std::vector<const Fr*> polys;
            Pass ps{lane, {}};
            for (const CommitCol& cl : cols) {
                polys.push_back(cl.poly);
                ps.to.push_back(cl.to);
            }
            int r = ctx_msm_begin_batch(d.c, lane, polys.data(), (uint32_t)polys.size(), ctx_basis(d.c, basis), d.n);
            if (r) return d.fail(r);
            f.busy.push_back(ps);
        }
        // collects a pass: its commitments are written to their transcripts in the order the columns were given
        void end_write(const Pass& ps) {
            if (!d.ok()) return;
            G1Jac js[MSM_MAX_BATCH];
            int r = ctx_msm_end_batch(d.c, ps.lane, js);
            if (r) return d.fail(r);
            G1Affine af[MSM_MAX_BATCH];
            const uint32_t cnt = (uint32_t)ps.to.size();
            jac_batch_to_affine(js, cnt, af);
            for (uint32_t q = 0; q < cnt && d.ok(); q++)
                if (!ps.to[q]->write_point(af[q])) d.fail(ZK_EINVAL);  // identity: halo2 refuses to write it
        }
        void drain(Fifo& f) {
            if (f.before_collect && !f.busy.empty()) f.before_collect();
            while (!f.busy.empty()) {
                end_write(f.busy.front());
                f.busy.pop_front();
            }
        }
        void add(Batcher& b, const Fr* poly, Transcript* to) {
            b.pend.push_back(CommitCol{poly, to});
            if (b.pend.size() >= b.cap) flush(b);
        }
        void flush(Batcher& b) {
            if (b.pend.size() >= 4 && b.f->lanes.size() >= 2 && !b.loaded) {
                const size_t h = (b.pend.size() + 1) / 2;
                begin(*b.f, std::vector<CommitCol>(b.pend.begin(), b.pend.begin() + h), b.basis);
                begin(*b.f, std::vector<CommitCol>(b.pend.begin() + h, b.pend.end()), b.basis);
            } else {
                begin(*b.f, b.pend, b.basis);
            }
            b.pend.clear();
        }
    };
    Commits cq{*this};
    using Fifo = Commits::Fifo;
    using Batcher = Commits::Batcher;
    using Col = CommitCol;
    void rows_flush() { P[0]->rows_flush(); }  // (the one row stager of all lanes)
    // `lone`: wide passes stay whole in the regime the proof's begin() found (Prover::loaded: three or more contexts busy); the
    // passes of several lanes are always split over two lanes
    Batcher batcher(Fifo& f, int basis) { return Batcher{&f, basis, pass_cap, lone && P[0]->loaded, {}}; }
    void add(Batcher& b, const Fr* poly, uint32_t lane) { cq.add(b, poly, tr_of(lane)); }
    void transforms(const std::vector<Prover::Forms>& cols) {
        if (!ok()) return;
        P[0]->transforms(cols);  // (flushes the shared row stager first)
    }

    // the instance columns of every lane (a key with the column); every lane's list is its prover's (none: the empty column)
    int instance_columns() {
        if (!pk0->inst_val) return ZK_OK;
        static const std::vector<Fr> none;
        // `lone`: memset + copy into the key's own column; several lanes: ONE staged upload and ONE launch, whose staging is the
        // BatchBufs' — which a lone proof's key need not have
        if (lone) return pk_instance_upload(c, st, pk0, P[0]->instance ? *P[0]->instance : none);
        std::vector<zk_pk_rec*> ws;
        std::vector<const std::vector<Fr>*> lists;
        for (Prover* p : P) {
            ws.push_back(p->pk);
            lists.push_back(p->instance ? p->instance : &none);
        }
        return pk_instance_upload_lanes(c, st, pk0, ws, lists);
    }
    // the columns' coefficient and coset forms ride with the lanes' first advice forms: a column's values are uploaded on the main
    // stream before the first flush of blinding rows, which is what a transform on the side stream waits for
    void with_instances(std::vector<Prover::Forms>& fm) {
        for (Prover* p : P)
            if (p->pk->inst_val) fm.push_back(Prover::Forms{p->pk->inst_val, p->pk->inst_poly, p->pk->inst_coset});
    }

    // ------------------------------------------------------------------ run ---
    // Commitments are computed as early as their inputs exist (none of a', s', the random polynomial needs a challenge) and
    // collected in transcript order; RNG draws keep halo2's order (the random polynomial's block range is reserved up front).  The
    // coefficient and extended-coset forms the quotient needs are produced right behind each commitment's head: they need no
    // challenge, and they keep the main stream busy while the MSM tails (and the host's transcript work) would leave it idle.
    int run(const Fr* const* advice /* B x n_adv, lane-major */, int scheme) {
        using Forms = Prover::Forms;
        const uint32_t bf = BLINDING_FACTORS, usable = lay.usable, np = proofs();
        // transcript_repr is hashed once per proof: every lane's begin() writes it to its transcript — in the one-proof mode lane
        // 0's to the proof's, the others' to their scratch.  There the instance lists are absorbed HERE, once: all circuits' values
        // in circuit order behind transcript_repr and before any advice commitment (halo2's loop over `instances` at the top of
        // create_proof); no begin() absorbs its own, so the scratch transcripts never see a list and nothing is hashed twice
        for (Prover* p : P) {
            if (one) p->absorb_instance = false;
            if (p->begin()) return p->rc;
        }
        if (one)
            for (Prover* p : P)
                if (p->instance)
                    for (const Fr& v : *p->instance) P[0]->tr->common_scalar(v);  // (neither N nor the lengths are hashed)
        // the three-coset route (poly.hip): one key, one context, one option — every begin() took the same decision; lane 0's made
        // the key's coset-major copies, which the members read through their own records (pk_ensure_cosets3)
        const bool c3 = P[0]->cosets3;
        if (int r = instance_columns()) return r;

        // -- 1. advice of every lane
        // (many columns: one launch copies a lane's — every lane stages into its own workspace's argument block.  That staging is
        // reused by the later batched launches, each preceded by a stream-ordered upload, so the host must not overwrite it
        // before the upload has been consumed: `lone` waits right behind its staging, several lanes once behind the last lane's rows)
        const bool many = advice_staged(lay);
        for (uint32_t q = 0; q < B; q++) {
            zk_pk_rec* pk = P[q]->pk;
            const Fr* const* adv = advice + (size_t)q * lay.n_adv;
            if (many) {
                if (int r = advice_columns_staged(c, st, pk, adv)) return r;
                if (lone && aud_sync(c, st) != hipSuccess) return ZK_EHIP;
            }
            for (uint32_t j = 0; j < lay.n_adv; j++) {
                if (!many)
                    if (int r = advice_column(c, st, pk, adv, j)) return r;
                P[q]->set_rows(pk->adv_val[j], usable, draw(q, bf + 1));
            }
            draw(q, lay.n_adv);  // advice blinds (unused by KZG, still drawn)
        }
        if (many && !lone && aud_sync(c, st) != hipSuccess) return ZK_EHIP;
        // one advice column and one lookup per lane (k = 19): the advice pass of all lanes stays in flight on lane 0
        // while the lookup columns are made and committed; otherwise plain order
        const bool pipe = lay.n_adv == 1 && lay.n_lookups == 1 && B <= pass_cap;
        bool adv_transformed = false;
        Fifo af{{0}, {}, nullptr};
        if (pipe) {
            std::vector<Col> cols;
            for (uint32_t q = 0; q < B; q++) cols.push_back(Col{P[q]->pk->adv_val[0], tr_of(q)});
            cq.begin(af, cols, ZK_BASIS_LAGRANGE);
            if (P[0]->xform_side()) {  // a lone proof on the transform stream: the advice column's forms are made under its own MSM pass
                std::vector<Forms> fm;
                for (uint32_t q = 0; q < B; q++) fm.push_back(Forms{P[q]->pk->adv_val[0], P[q]->pk->adv_poly[0], P[q]->pk->adv_coset[0]});
                with_instances(fm);
                transforms(fm);
                adv_transformed = true;
            }
        } else {
            // several advice columns: whole batches of columns per MSM pass, up to MSM_LANES passes in flight, each followed by its
            // columns' transforms; collected in column order
            Fifo f{{0, 1, 2}, {}, nullptr};
            std::vector<Col> cols;
            std::vector<Forms> fm;
            bool first = true;
            auto go = [&]() {
                cq.begin(f, cols, ZK_BASIS_LAGRANGE);
                if (first) with_instances(fm);  // (with the first pass's transforms, behind its advice forms)
                first = false;
                transforms(fm);
                cols.clear();
                fm.clear();
            };
            for (uint32_t q = 0; q < B && ok(); q++)
                for (uint32_t j = 0; j < lay.n_adv && ok(); j++) {
                    zk_pk_rec* pk = P[q]->pk;
                    cols.push_back(Col{pk->adv_val[j], tr_of(q)});
                    fm.push_back(Forms{pk->adv_val[j], pk->adv_poly[j], pk->adv_coset[j]});
                    if (cols.size() == pass_cap) go();
                }
            if (!cols.empty()) go();
            cq.drain(f);
        }
        if (!ok()) return rc;

        // -- 2. lookups: permuted input / table of every lookup of every lane in one set of launches; theta after the last advice
        // commitment of its proof
        bool theta_done = false;
        auto squeeze_theta = [&]() {
            if (!theta_done) {
                if (pipe) cq.drain(af);
                squeeze();  // (single-expression lookups: theta-compression is the identity)
                theta_done = true;
            }
        };
        // a', s' of every lookup: batches of columns per MSM pass; their transforms (and, in the pipelined case, the advice
        // columns' where they have not gone out yet) follow the MSM heads so that they cover the tails
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
            if (int r = lookup_permute(c, st, lay, items, bufs.lks)) return r;
        }
        for (uint32_t q = 0; q < B && ok(); q++) {
            zk_pk_rec* pk = P[q]->pk;
            for (uint32_t l = 0; l < lay.n_lookups && ok(); l++) {
                P[q]->set_rows(pk->lk_ap[l], usable, draw(q, bf + 1));
                P[q]->set_rows(pk->lk_sp[l], usable, draw(q, bf + 1));
                draw(q, 2);
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
        if (pipe && !adv_transformed) {
            // (the advice columns' forms ahead of the lookups' in the one call, for every lane count)
            std::vector<Forms> fm;
            for (uint32_t q = 0; q < B; q++) fm.push_back(Forms{P[q]->pk->adv_val[0], P[q]->pk->adv_poly[0], P[q]->pk->adv_coset[0]});
            with_instances(fm);
            due.insert(due.begin(), fm.begin(), fm.end());
        }
        transforms(due);
        due.clear();
        {
            // one check for all lookups of all lanes (the flag accumulates): an input outside the table is halo2's
            // ConstraintSystemFailure; nothing has been written for the lookups yet.  The call fails as a whole.
            bool bad = false;
            if (int r = lookup_permute_failed(c, st, bufs.lks, &bad)) return r;
            if (bad) {
                ctx_msm_drain(c);
                return ZK_EWITNESS;
            }
        }
        squeeze_theta();
        cq.drain(lf);
        if (!ok()) return rc;
        const std::vector<Fr> beta = squeeze();  // (the transcripts of B proofs are independent: each still gives beta, then gamma)
        const std::vector<Fr> gamma = squeeze();

        // -- 5 (early). the random polynomial of every proof — B, or the ONE: no challenge needed; its n draws come after the
        // grand products' draws of all the proof's circuits, each proof's from its own key: that block range is reserved
        const uint32_t nprod = lay.n_chunks + lay.n_lookups;
        Fifo rf{{0}, {}, nullptr};
        // (more proofs than a pass takes: the random polynomials are committed after the grand products.  One proof: always early)
        const bool rand_early = np <= pass_cap;
        {
            const uint64_t skip = (uint64_t)(one ? B : 1) * nprod * (bf + 1);
            std::vector<Col> cols;
            for (uint32_t p = 0; p < np; p++) {
                ChaChaKey key;
                memcpy(key.w, P[p]->rng.key, 32);
                P[p]->A({}, {P[p]->pk->random_poly}, "random polynomial");
                launch_chacha_fr(key, P[p]->rng.block + skip, P[p]->pk->random_poly, n, st);
                cols.push_back(Col{P[p]->pk->random_poly, P[p]->tr});
            }
            if (rand_early) cq.begin(rf, cols, ZK_BASIS_MONOMIAL);
        }

        // -- 3. grand products of every lane: numerators / denominators per lane, then ALL scans in one batch; the z columns
        // (permutation chunks, lookups) are committed in batches on lanes 1 and 2, their transforms behind each batch's MSM head
        Fifo zf{{1, 2}, {}, nullptr};
        Batcher zb = batcher(zf, ZK_BASIS_LAGRANGE);
        std::vector<Forms> zdue;
        {
            std::vector<Fr*> zs;
            std::vector<GpGroup> groups;
            // The argument staging of the many-column shapes may still be in use: the host waits before it rewrites it.  Several
            // lanes, each with a staging of its own: once before the first lane's, and per lane between the two where both stage.
            // `lone`: as late as it may — before the chunks' only if they stage, before the lookups' if those do
            const bool many_chunks = lay.n_chunks > BATCH_ARGS_MIN, many_lookups = lay.n_lookups > BATCH_ARGS_MIN;
            if ((many_chunks || (many_lookups && !lone)) && aud_sync(c, st) != hipSuccess) return ZK_EHIP;
            for (uint32_t q = 0; q < B; q++) {
                zk_pk_rec* pk = P[q]->pk;
                if (int r = perm_numden_enqueue(c, st, pk, pk->adv_val.data(), P[q]->tw, beta[q], gamma[q], true)) return r;
                if (many_lookups && (many_chunks || lone) && aud_sync(c, st) != hipSuccess) return ZK_EHIP;
                if (int r = lk_numden_enqueue(c, st, pk, pk->adv_val.data(), pk->lk_ap.data(), pk->lk_sp.data(), beta[q], gamma[q], lay.n_chunks, true,
                                              false))
                    return r;
                zs.insert(zs.end(), pk->z_val.begin(), pk->z_val.end());
                zs.insert(zs.end(), pk->lk_z.begin(), pk->lk_z.end());
            }
            // (a lane's first product starts a new chain)
            for (uint32_t q = 0; q < B; q++) groups.push_back(GpGroup{P[q]->pk, zs.data() + (size_t)q * nprod, nprod, lay.n_chunks});
            if (int r = grand_products(c, st, lay, groups, bufs.gp)) return r;
            // blinding rows and commitments, per proof in halo2's order: the permutation products of every circuit of the proof, then
            // its lookup products — B proofs: per proof chunks, then lookups; one proof: part-major over the circuits.  This fixes
            // the RNG order, the transcript order and how zdue groups the transforms
            for (uint32_t p = 0; p < np; p++)
                for (uint32_t part = 0; part < 2; part++)
                    for (uint32_t q = p; q < lanes_end(p) && ok(); q++) {
                        zk_pk_rec* pk = P[q]->pk;
                        const uint32_t i0 = part ? lay.n_chunks : 0, i1 = part ? nprod : lay.n_chunks;
                        for (uint32_t i = i0; i < i1 && ok(); i++) {
                            Fr* z = zs[q * nprod + i];
                            P[q]->set_rows(z, n - bf, draw(q, bf));
                            draw(q, 1);
                            add(zb, z, q);
                            if (i < lay.n_chunks) zdue.push_back(Forms{pk->z_val[i], pk->z_poly[i], pk->z_coset[i]});
                            else zdue.push_back(Forms{pk->lk_z[i - lay.n_chunks], pk->lk_z_poly[i - lay.n_chunks], pk->lk_z_coset[i - lay.n_chunks]});
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

        // -- 5. the random polynomials' commitments (their draws happen here in stream order): once per proof
        for (uint32_t p = 0; p < np; p++) {
            P[p]->rng.block += n;
            P[p]->draw(1);
        }
        if (rand_early) {
            cq.drain(rf);
        } else {
            Fifo f{{0, 1, 2}, {}, nullptr};
            Batcher rb = batcher(f, ZK_BASIS_MONOMIAL);
            for (uint32_t p = 0; p < np; p++) add(rb, P[p]->pk->random_poly, p);
            cq.flush(rb);
            cq.drain(f);
        }
        if (!ok()) return rc;
        const std::vector<Fr> y = squeeze();

        // -- 6. quotients into every proof's h_ext (P[p]->pk), then their inverse coset transforms (every coefficient / coset
        // form was produced behind its commitment above)
        if (lone) {
            // Prover::quotient: the transforms on the side stream are joined first; one launch, one inverse transform
            if (int r = P[0]->quotient(beta[0], gamma[0], y[0])) return r;
        } else if (one) {
            // B passes into circuit 0's h_ext (the y-Horner chain runs on across the circuits: pass q carries y^(T (B - 1 - q));
            // circuit 0 stores, the others accumulate), then ONE inverse transform
            const uint32_t T = quotient_terms(lay.n_gate, lay.n_chunks, lay.n_lookups);
            const Fr yT = fr_pow(y[0], T);
            std::vector<Fr> scale(B);
            scale[B - 1] = Fr::one();
            for (uint32_t q = B - 1; q-- > 0;) scale[q] = fe_mul(scale[q + 1], yT);
            for (uint32_t q = 0; q < B; q++)
                if (int r = quotient_pass_of_workspace(c, st, P[q]->pk, c3, beta[q], gamma[q], y[q], pk0->h_ext, scale[q], q > 0)) return r;
            if (int r = c3 ? ctx_intt_cosets3(c, pk0->h_ext, lay.k) : ctx_ntt(c, pk0->h_ext, N, pk0->h_ext, lay.ext_k, true, true, N)) return r;
        } else {
            // one launch per proof (each fills the chip), then the inverse coset transforms of all in batches
            for (uint32_t q = 0; q < B; q++)
                if (int r = quotient_of_workspace(c, st, P[q]->pk, c3, beta[q], gamma[q], y[q])) return r;
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
        }
        {
            // the h pieces of every proof: contiguous n-coefficient slices of its quotient
            Fifo hf{{0, 1, 2}, {}, nullptr};
            Batcher hb = batcher(hf, ZK_BASIS_MONOMIAL);
            for (uint32_t p = 0; p < np && ok(); p++) {
                P[p]->draw(lay.n_h);  // h-piece blinds
                for (uint32_t i = 0; i < lay.n_h && ok(); i++) add(hb, P[p]->pk->h_ext + (size_t)i * n, p);
            }
            cq.flush(hb);
            cq.drain(hf);
        }
        if (!ok()) return rc;
        const std::vector<Fr> x = squeeze();
        HT("x squeezed");

        // -- 7. evaluations: every opened value of every proof in ONE launch, then written in transcript order.  A proof's list
        // is Prover::build_evals' over its circuits: B proofs, each its own; one proof, the concatenated one with fixed, sigma,
        // random and h ONCE
        std::vector<std::vector<Prover::Q>> ev(np), queries(np);
        std::vector<Prover::EvIdx> ix(np);
        {
            size_t total = 0;
            for (uint32_t p = 0; p < np; p++) {
                P[p]->combine_h(x[p]);
                std::vector<const zk_pk_rec*> circuits;
                for (uint32_t q = p; q < lanes_end(p); q++) circuits.push_back(P[q]->pk);
                P[p]->build_evals(circuits, ev[p], ix[p]);
                if (ev[p].size() > bufs.max_evals) return ZK_ESTATE;
                for (size_t i = 0; i < ev[p].size(); i++) {
                    bufs.ev.h_items[total + i].poly = ev[p][i].poly;
                    bufs.ev.h_items[total + i].x = P[p]->xrot(x[p], ev[p][i].rot);
                }
                total += ev[p].size();
            }
            if (int r = evaluate_enqueue(c, st, bufs.ev, (uint32_t)total, n)) return r;
            HT("evals on host");
            size_t pos = 0;
            for (uint32_t p = 0; p < np; p++) {
                for (size_t i = 0; i < ev[p].size(); i++) ev[p][i].eval = bufs.ev.host[pos + i];
                pos += ev[p].size();
                for (size_t i = 0; i < ix[p].n_written; i++) P[p]->tr->write_scalar(ev[p][i].eval);
                queries[p] = P[p]->queries_from_evals(ev[p], ix[p]);
                P[p]->pk->lc_used = 0;
            }
        }
        if (!ok()) return rc;
        HT("queries built");

        // -- 8. multi-open: the stages of every proof, from its prover's workspace, the commitments between them merged
        if (scheme == ZK_SCHEME_GWC) {
            // the witness polynomials need no challenge in between: all of them go through one MSM pass
            Fifo wf{{0, 1, 2}, {}, nullptr};
            Batcher wb = batcher(wf, ZK_BASIS_MONOMIAL);
            for (uint32_t p = 0; p < np && ok(); p++) {
                std::vector<const Fr*> wit;
                if (int r = P[p]->gwc_stage1(queries[p], x[p], wit)) return r;
                for (const Fr* w : wit) add(wb, w, p);
            }
            cq.flush(wb);
            cq.drain(wf);
            return ok() ? ZK_OK : rc;
        }
        std::vector<Prover::Shplonk> S(np);
        // (a queue takes the LAST of its free lanes: the single commitments of one proof — the lone one, or the one over B
        // circuits — stay on lane 0)
        Fifo of{np == 1 ? std::vector<int>{0} : std::vector<int>{0, 1, 2}, {}, nullptr};
        {
            Batcher ob = batcher(of, ZK_BASIS_MONOMIAL);
            for (uint32_t p = 0; p < np && ok(); p++) {
                if (int r = P[p]->shplonk_stage1(queries[p], x[p], S[p])) return r;
                add(ob, S[p].hx, p);
            }
            cq.flush(ob);
            cq.drain(of);
        }
        if (!ok()) return rc;
        {
            Batcher ob = batcher(of, ZK_BASIS_MONOMIAL);
            for (uint32_t p = 0; p < np && ok(); p++) {
                const Fr* last = nullptr;
                if (int r = P[p]->shplonk_stage2(S[p], &last)) return r;
                add(ob, last, p);
            }
            cq.flush(ob);
            cq.drain(of);
        }
        return ok() ? ZK_OK : rc;
    }
};
