// prover.hip — create_proof on the device-resident engine: a lane's state and its multi-open stages (Prover), the one driver of
// a proof alone, of several proofs and of one proof over several circuits (prover_lockstep.h) and their entry points.  Keygen and the
// key's workspace are prover_key.hip, the phase-level entry points prover_phases.hip; the steps they share are prover_steps.h — the
// driver holds the scheduling only: which step, in which order, on which lane, and when a lane is collected.
//
// Host orchestration (C++) of the kernels in msm.hip / ntt.hip / quotient.hip /
// prover_kernels.hip / poly.hip, mirroring halo2_proofs `plonk::create_proof` as the reference calls it:
//   create_proof  halo2-circuits/src/ecc/ecdsa_p256.rs:366-373 (EvmTranscript + ProverGWC)
//                 halo2-circuits/src/ecc/ecdsa_p256.rs:416-423 (Blake2bWrite + ProverSHPLONK)
// Phase structure, transcript order and RNG draw order: SURVEY.md §3.3 / App. A.3
// (the test oracle restates the same flow in Python; proofs are byte-compared against it).
// Polynomials never leave HBM: the host sees commitments (64 B), evaluations
// (32 B) and challenges only.  Randomness is a ChaCha20 stream (rand_chacha's
// ChaCha20Rng layout): one 64-byte block per Fr::random, drawn on the host for
// the handful of blinding rows and on the device for the n-coefficient random
// polynomial — the engine's kernels themselves consume no randomness.
#include <stdlib.h>

#include <algorithm>
#include <deque>
#include <functional>
#include <memory>
#include <unordered_map>
#include <vector>

#include "prover_steps.h"

using namespace zk;

#ifdef ZK_HOST_TRACE  // host-side stage stamps of the proof's last phases (experiments only: tools/ab_variants.sh ... "-DZK_HOST_TRACE")
#include <chrono>
#include <cstdio>
static std::chrono::steady_clock::time_point& ht_last() {
    static thread_local std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    return t;
}
#define HT(name)                                                                                                  \
    do {                                                                                                          \
        const auto ht_now = std::chrono::steady_clock::now();                                                     \
        fprintf(stderr, "HT %-24s +%7.1f us\n", name, std::chrono::duration<double, std::micro>(ht_now - ht_last()).count()); \
        ht_last() = ht_now;                                                                                       \
    } while (0)
#else
#define HT(name) do { } while (0)
#endif

// ==================================================================== prove ==

namespace {

Fr fr_pow(Fr a, uint64_t e) { return fe_pow_u64(a, e); }

// The Lagrange basis over `pts` as coefficient vectors: basis[j] = L_j(X) = prod_{i != j} (X - pts_i) / (pts_j - pts_i).  A
// rotation set's commitments share their points, so this is paid once per set — with ONE field inversion for all the
// denominators — and a commitment's interpolant is sum_j eval_j L_j (m^2 products): the same field elements
// halo2's lagrange_interpolate computes per commitment, hence the same bytes.
std::vector<std::vector<Fr>> lagrange_basis(const std::vector<Fr>& pts) {
    const size_t m = pts.size();
    std::vector<std::vector<Fr>> basis(m);
    std::vector<Fr> den(m, Fr::one()), inv(m);
    for (size_t j = 0; j < m; j++) {
        std::vector<Fr> num(1, Fr::one());
        for (size_t i = 0; i < m; i++) {
            if (i == j) continue;
            std::vector<Fr> nn(num.size() + 1, Fr::zero());
            for (size_t t = 0; t < num.size(); t++) {
                nn[t + 1] = fe_add(nn[t + 1], num[t]);
                nn[t] = fe_sub(nn[t], fe_mul(pts[i], num[t]));
            }
            num.swap(nn);
            den[j] = fe_mul(den[j], fe_sub(pts[j], pts[i]));
        }
        basis[j] = num;
    }
    fr_batch_invert(den.data(), inv.data(), (uint32_t)m);  // (distinct points: no denominator is zero)
    for (size_t j = 0; j < m; j++)
        for (Fr& cf : basis[j]) cf = fe_mul(cf, inv[j]);
    return basis;
}

Fr eval_small(const std::vector<Fr>& c, const Fr& x) {
    Fr acc = Fr::zero();
    for (size_t i = c.size(); i-- > 0;) acc = fe_add(fe_mul(acc, x), c[i]);
    return acc;
}

Fr vanishing_eval(const std::vector<Fr>& pts, const Fr& x) {
    Fr acc = Fr::one();
    for (const Fr& p : pts) acc = fe_mul(acc, fe_sub(x, p));
    return acc;
}

// One lane of a proof run (prover_lockstep.h): its transcript, RNG stream and row stager, what begin() decides for the proof
// (xside / cosets3 / loaded), the helpers over its workspace and the multi-open stages.  The schedule is the driver's.
struct Prover {
    zk_ctx* c;
    zk_pk_rec* pk;
    const Layout& lay;
    hipStream_t st;
    ChaCha20Rng rng;
    Transcript* tr;
    uint32_t n, N;
    const Fr *tw, *tw_ext;
    Fr omega, omega_inv;
    int rc = ZK_OK;
    // staged row writes: a ring of ROWS_BLOCKS blocks in the key's pinned / device staging; `rows` is this prover's own stager,
    // or — in a lock-step batch — the first prover's, so that the blinding rows of all proofs go up in one launch per phase
    struct RowStager {
        RowEntry *host = nullptr, *dev = nullptr;
        uint32_t block = 0, count = 0;
    };
    RowStager own_rows;
    RowStager* rows = &own_rows;
    // the instance column's values (zk_prove_public; a key with the column and no caller's values proves the empty column).  Absorbed
    // behind transcript_repr, never written; the column is neither blinded nor committed nor opened, and draws nothing
    const std::vector<Fr>* instance = nullptr;
    // begin() absorbs `instance` into this prover's transcript: a lone proof and every proof of a lock-step batch.  The driver of one
    // proof over several circuits (prover_lockstep.h, its one-proof mode) clears it and absorbs every circuit's list itself, once, on the one transcript
    bool absorb_instance = true;
    bool batch_member = false;  // one of the proofs of a lock-step batch (prover_lockstep.h): transforms stay on the main stream

    Prover(const Prover&) = delete;  // (`rows` may point into this object)
    Prover(zk_ctx* c_, zk_pk_rec* pk_, const uint8_t seed[32], Transcript* t)
        : c(c_), pk(pk_), lay(pk_->lay), st(c_->stream), rng(seed), tr(t), n(pk_->lay.n), N(4 * pk_->lay.n) {
        own_rows.host = pk_->rows_host;
        own_rows.dev = pk_->rows_dev;
    }

    bool ok() const { return rc == ZK_OK; }
    void fail(int code) {
        if (rc == ZK_OK) rc = code;
    }

    // ---- device helpers
    // Blinding rows are staged on the host and written by rows_flush() — one upload and one launch for all
    // the columns of a phase — before the first kernel that reads those columns (the driver's commitment queue and
    // transforms() flush; other readers call rows_flush() themselves).
    // ---- stream audit (audit.h, ZK_OPT_STREAM_AUDIT): every enqueue of this prover names the buffers it reads and writes
    void A(std::initializer_list<const void*> r, std::initializer_list<const void*> w, const char* site) {
        if (c->audit.on) c->audit.op(st, r, w, site);
    }
    void AV(const std::vector<const void*>& r, const std::vector<const void*>& w, const char* site) {
        if (c->audit.on) c->audit.op_v(st, r.data(), r.size(), w.data(), w.size(), site);
    }
    std::vector<const void*> aud_rows;  // the columns the staged blinding rows go to (audit only)
    void set_rows(Fr* col, uint32_t first, const std::vector<Fr>& vals) {
        if (!ok()) return;
        if (vals.size() > 8) return fail(ZK_ESTATE);
        if (rows->count == ROWS_CAP) rows_flush();
        if (c->audit.on) {
            if (rows->count == 0) c->audit.host_write(rows->host + (size_t)rows->block * ROWS_CAP, "blinding rows: the host fills a staging block");
            aud_rows.push_back(col);
        }
        RowEntry& e = rows->host[(size_t)rows->block * ROWS_CAP + rows->count++];
        memcpy(e.vals, vals.data(), vals.size() * sizeof(Fr));
        e.dst = col + first;
        e.count = (uint32_t)vals.size();
        e.pad_ = 0;
    }
    void rows_flush() {
        if (!ok() || rows->count == 0) return;
        RowEntry* h = rows->host + (size_t)rows->block * ROWS_CAP;
        RowEntry* d = rows->dev + (size_t)rows->block * ROWS_CAP;
        if (c->audit.on) {
            A({h}, {d}, "blinding rows: upload of the staging block");
            AV({d}, aud_rows, "blinding rows: scatter into the columns");
            aud_rows.clear();
        }
        if (hipMemcpyAsync(d, h, rows->count * sizeof(RowEntry), hipMemcpyHostToDevice, st) != hipSuccess) return fail(ZK_EHIP);
        launch_scatter_rows(d, rows->count, st);
        aud_record(c, c->ev_rows, st);  // what the transform stream waits for (transforms())
        rows->count = 0;
        if (++rows->block == ROWS_BLOCKS) {
            // the ring wraps: the oldest block's upload must have been consumed before it is overwritten
            if (aud_sync(c, st) != hipSuccess) return fail(ZK_EHIP);
            rows->block = 0;
        }
    }
    std::vector<Fr> draw(uint32_t count) {
        std::vector<Fr> v(count);
        for (auto& x : v) x = rng.next_fr();
        return v;
    }
    // Lagrange values -> coefficients -> extended coset for a set of columns, several columns per launch
    struct Forms {
        const Fr* val;
        Fr* poly;
        Fr* coset;
    };
    // The transforms of a LONE proof run on the context's transform stream, beside the MSM passes instead of between them (ctx.h
    // xform_stream): they wait for the last flush of blinding rows — every transformed column has such rows, written after the
    // kernels that made it — and the quotient waits for them (xform_join).
    // Auto: a lone context and columns of 2^18 rows or more (measured, tools/single_ab.py OPTS=8=1 / 8=2, same box: k = 19 12.10 ->
    // 11.47 ms, EVM 13.66 -> 13.03; k = 17 6.55 -> 6.67: there the transforms are too short to pay for the cross-stream events)
    // Decided ONCE per proof (begin()): a proof whose transforms changed streams half-way would have the two streams' NTTs
    // share the context's ping-pong scratch without an order between them (round 5's first form decided per call: under four
    // pipelines the count dips to one now and then, and 1 proof in ~ 1 500 came out wrong — tools/soak.py)
    bool xside = false;
    // a quotient of three pieces (deg h < 3n) is taken over three of the extended domain's four cosets (poly.hip "three cosets"):
    // the columns' coset forms are [3][n] coset-major, made by n-point transforms.  Decided once per proof (begin())
    bool cosets3 = false;
    // three or more contexts busy on the device (the regime in which reduction tails run on the main stream): decided once per
    // proof (begin()); a lone proof's multi-column commitments are then not split into two passes (LockstepRun::batcher)
    bool loaded = false;
    // (audit self-test, ZK_OPT_STREAM_AUDIT = 2: round 5's faulty form on purpose — the stream chosen per CALL, alternating, and no
    // join before a main-stream transform: the ledger must then refuse every proof whose transforms come in more than one call)
    bool fault_flip = false;
    bool xform_side() {
        if (c->audit_fault) return fault_flip = !fault_flip;
        return xside;
    }
    void xform_join() {
        if (!c->xform_pending) return;
        c->xform_pending = false;
        if (aud_wait(c, st, c->ev_xform) != hipSuccess) fail(ZK_EHIP);
    }
    void transforms(const std::vector<Forms>& cols) {
        rows_flush();
        if (!ok() || cols.empty()) return;
        const bool side = xform_side();
        const hipStream_t xs = side ? c->xform_stream : st;
        if (side && aud_wait(c, xs, c->ev_rows) != hipSuccess) return fail(ZK_EHIP);
        if (!side && !c->audit_fault) xform_join();  // (the two streams share the NTT's ping-pong scratch)
        transforms_on(cols, xs);
        if (side) {
            if (aud_record(c, c->ev_xform, xs) != hipSuccess) return fail(ZK_EHIP);
            c->xform_pending = true;
        }
    }
    void transforms_on(const std::vector<Forms>& cols, hipStream_t xs) {
        const uint32_t b1 = ctx_ntt_max_batch(lay.k), b2 = ctx_ntt_max_batch(lay.ext_k);
        const Fr* src[NTT_MAX_BATCH];
        Fr* dst[NTT_MAX_BATCH];
        for (size_t i0 = 0; i0 < cols.size() && ok(); i0 += b1) {
            const uint32_t cnt = (uint32_t)std::min<size_t>(b1, cols.size() - i0);
            for (uint32_t q = 0; q < cnt; q++) {
                src[q] = cols[i0 + q].val;
                dst[q] = cols[i0 + q].poly;
            }
            int r = ctx_ntt_batch(c, src, n, dst, cnt, lay.k, true, false, n, xs);
            if (r) fail(r);
        }
        if (cosets3) {
            // a quotient of three pieces: three n-point transforms per column into [3][n] coset-major values (poly.hip "three cosets")
            const uint32_t b3 = std::max(1u, b1 / 3);
            for (size_t i0 = 0; i0 < cols.size() && ok(); i0 += b3) {
                const uint32_t cnt = (uint32_t)std::min<size_t>(b3, cols.size() - i0);
                for (uint32_t q = 0; q < cnt; q++) {
                    src[q] = cols[i0 + q].poly;
                    dst[q] = cols[i0 + q].coset;
                }
                int r = ctx_ntt_cosets3(c, src, dst, cnt, lay.k, xs);
                if (r) fail(r);
            }
            return;
        }
        for (size_t i0 = 0; i0 < cols.size() && ok(); i0 += b2) {
            const uint32_t cnt = (uint32_t)std::min<size_t>(b2, cols.size() - i0);
            for (uint32_t q = 0; q < cnt; q++) {
                src[q] = cols[i0 + q].poly;
                dst[q] = cols[i0 + q].coset;
            }
            int r = ctx_ntt_batch(c, src, n, dst, cnt, lay.ext_k, false, true, N, xs);
            if (r) fail(r);
        }
    }
    // out = sum_j c_j * in_j (- sub0 on coefficient 0), any number of inputs: MAX_LC per launch
    void lincomb_many(Fr* out, const std::vector<Term>& terms, bool sub0, const Fr& sub0_val, bool accumulate_first = false,
                      const std::vector<Fr>* sub_low = nullptr) {
        if (c->audit.on) {
            std::vector<const void*> rd;
            for (auto& t : terms) rd.push_back(t.poly);
            if (accumulate_first) rd.push_back(out);
            AV(rd, {out}, "linear combination");
        }
        if (terms.size() > MAX_LC && !accumulate_first && n >= 256 && pk->lc_used + terms.size() <= pk->lc_cap) {
            // hundreds of inputs: one launch over an argument list in device memory.  The list's slots are not reused within a
            // proof (the copies are asynchronous; capacity: every opened polynomial twice, pk_alloc_workspace)
            LcTerm* h = pk->h_lc_terms + pk->lc_used;
            for (size_t j = 0; j < terms.size(); j++) h[j] = LcTerm{terms[j].poly, 0, terms[j].c};
            launch_lincomb_terms(h, pk->d_lc_terms + pk->lc_used, (uint32_t)terms.size(), out, n, sub0, sub0_val,
                                 sub_low ? sub_low->data() : nullptr, sub_low ? (uint32_t)sub_low->size() : 0u, st);
            pk->lc_used += (uint32_t)terms.size();
            return;
        }
        lincomb_enqueue(st, out, n, terms, accumulate_first, sub0 ? &sub0_val : nullptr, sub_low ? sub_low->data() : nullptr,
                        sub_low ? (uint32_t)sub_low->size() : 0u);
    }
    Fr xrot(const Fr& x, int r) const {
        Fr w = r >= 0 ? omega : omega_inv;
        return fe_mul(x, fr_pow(w, (uint64_t)(r >= 0 ? r : -r)));
    }

    // h(X) on the extended coset (one lane per row, quotient.hip), divided by X^n - 1, back to coefficients:
    // the first (degree - 1) * n coefficients of h_ext are the h pieces
    int quotient(const Fr& beta, const Fr& gamma, const Fr& y) {
        xform_join();  // every coset form is complete
        if (!ok()) return rc;
        if (int r = quotient_of_workspace(c, st, pk, cosets3, beta, gamma, y)) return r;
        if (cosets3) return ctx_intt_cosets3(c, pk->h_ext, lay.k);
        return ctx_ntt(c, pk->h_ext, N, pk->h_ext, lay.ext_k, true, true, N);
    }

    // an opening: polynomial, rotation of the point, value
    struct Q {
        const Fr* poly;
        int rot;
        Fr eval;
    };

    // ---- the opened values and the query order of a proof over one or more circuits of this key (`circuits`: this prover's own
    // workspace first; a lone proof and every proof of a lock-step batch have the one, prover_lockstep.h's one-proof mode B).
    // The verifier (verifier.h) reads both orders; they are stated here and nowhere else.
    // Every opened value in transcript order — for c: advice; fixed; random; sigma; for c: z; for c: lookups — then h(x) (not
    // written); where the groups start
    struct EvIdx {
        std::vector<size_t> i_adv, i_z, i_lk;  // per circuit
        size_t i_fix = 0, i_rand = 0, i_sig = 0, n_written = 0;
    };
    // the per-circuit parts: its advice queries; per chunk z(x), z(wx) and, but for the last chunk, z(w^last x); five openings per lookup
    void advice_evals(const zk_pk_rec* w, std::vector<Q>& ev) const {
        for (auto& aq : lay.advice_queries) ev.push_back(Q{w->adv_poly[aq.first], aq.second, Fr::zero()});
    }
    void z_evals(const zk_pk_rec* w, std::vector<Q>& ev) const {
        for (uint32_t ci = 0; ci < lay.n_chunks; ci++) {
            ev.push_back(Q{w->z_poly[ci], 0, Fr::zero()});
            ev.push_back(Q{w->z_poly[ci], 1, Fr::zero()});
            if (ci != lay.n_chunks - 1) ev.push_back(Q{w->z_poly[ci], lay.last_rot, Fr::zero()});
        }
    }
    void lookup_evals(const zk_pk_rec* w, std::vector<Q>& ev) const {
        for (uint32_t l = 0; l < lay.n_lookups; l++) {
            ev.push_back(Q{w->lk_z_poly[l], 0, Fr::zero()});
            ev.push_back(Q{w->lk_z_poly[l], 1, Fr::zero()});
            ev.push_back(Q{w->lk_ap_poly[l], 0, Fr::zero()});
            ev.push_back(Q{w->lk_ap_poly[l], -1, Fr::zero()});
            ev.push_back(Q{w->lk_sp_poly[l], 0, Fr::zero()});
        }
    }
    void build_evals(const std::vector<const zk_pk_rec*>& circuits, std::vector<Q>& ev, EvIdx& ix) const {
        for (const zk_pk_rec* w : circuits) {
            ix.i_adv.push_back(ev.size());
            advice_evals(w, ev);
        }
        // once, from this prover's workspace: fixed, random, sigma
        ix.i_fix = ev.size();
        for (uint32_t f = 0; f < lay.n_fix; f++) ev.push_back(Q{pk->fixed_poly[f], 0, Fr::zero()});
        ix.i_rand = ev.size();
        ev.push_back(Q{pk->random_poly, 0, Fr::zero()});
        ix.i_sig = ev.size();
        for (uint32_t p = 0; p < lay.perm_cols.size(); p++) ev.push_back(Q{pk->sigma_poly[p], 0, Fr::zero()});
        for (const zk_pk_rec* w : circuits) {
            ix.i_z.push_back(ev.size());
            z_evals(w, ev);
        }
        for (const zk_pk_rec* w : circuits) {
            ix.i_lk.push_back(ev.size());
            lookup_evals(w, ev);
        }
        ix.n_written = ev.size();
        ev.push_back(Q{pk->h_comb, 0, Fr::zero()});
    }
    // prover query order (== verifier's): for c: advice, perm z (x, wx per chunk; then `last` in reverse), lookups
    // (zL@x, a'@x, s'@x, a'@w^-1 x, zL@wx); then once fixed, sigma, h, random
    void circuit_queries(const std::vector<Q>& ev, size_t i_adv, size_t i_z, size_t i_lk, std::vector<Q>& queries) const {
        queries.insert(queries.end(), ev.begin() + i_adv, ev.begin() + i_adv + lay.advice_queries.size());
        std::vector<Q> lastq(lay.n_chunks);
        size_t pos = i_z;
        for (uint32_t ci = 0; ci < lay.n_chunks; ci++) {
            queries.push_back(ev[pos++]);
            queries.push_back(ev[pos++]);
            if (ci != lay.n_chunks - 1) lastq[ci] = ev[pos++];
        }
        for (int ci = (int)lay.n_chunks - 2; ci >= 0; ci--) queries.push_back(lastq[ci]);
        pos = i_lk;
        for (uint32_t l = 0; l < lay.n_lookups; l++, pos += 5) {
            queries.push_back(ev[pos]);      // zL @ x
            queries.push_back(ev[pos + 2]);  // a' @ x
            queries.push_back(ev[pos + 4]);  // s' @ x
            queries.push_back(ev[pos + 3]);  // a' @ w^-1 x
            queries.push_back(ev[pos + 1]);  // zL @ w x
        }
    }
    std::vector<Q> queries_from_evals(const std::vector<Q>& ev, const EvIdx& ix) const {
        std::vector<Q> queries;
        for (size_t ci = 0; ci < ix.i_adv.size(); ci++) circuit_queries(ev, ix.i_adv[ci], ix.i_z[ci], ix.i_lk[ci], queries);
        for (size_t i = ix.i_fix; i < ix.i_rand; i++) queries.push_back(ev[i]);
        for (size_t i = ix.i_sig; i < ix.i_z[0]; i++) queries.push_back(ev[i]);
        queries.push_back(ev[ix.n_written]);  // h
        queries.push_back(ev[ix.i_rand]);     // random poly
        return queries;
    }
    // h(X) = sum_i x^(n i) h_i(X) -> h_comb
    void combine_h(const Fr& x) {
        const Fr xn = fr_pow(x, n);
        LincombArgs a;
        memset(&a, 0, sizeof(a));
        a.out = pk->h_comb;
        a.n = n;
        a.count = lay.n_h;
        Fr p = Fr::one();
        for (uint32_t i = 0; i < lay.n_h; i++) {
            a.in[i] = pk->h_ext + (size_t)i * n;
            a.len[i] = n;
            a.c[i] = p;
            a.unit[i] = i == 0;
            p = fe_mul(p, xn);
        }
        A({pk->h_ext}, {pk->h_comb}, "h(X) from its pieces");
        launch_lincomb(a, st);
    }

    // ---------------------------------------------------------------- begin ---
    // the proof's once-only decisions, domain constants, and the transcript's first word
    int begin() {
        xside = !batch_member && (c->opt_xform_stream == 1 || (c->opt_xform_stream == 0 && lay.k >= 18 && ctx_activity_touch(c) <= 1));
        // the MSM passes of a lone proof on the context's MSM stream (ctx.h): same rule, same once-per-proof decision; measured
        // (tools/single_ab.py OPTS=9=1 / 9=2, four alternations on one box): 11.40-11.55 -> 11.29-11.38 ms, same bytes
        c->msm_side = !batch_member && (c->opt_msm_stream == 1 || (c->opt_msm_stream == 0 && xside && c->opt_xform_stream == 0));
        if ((xside || c->msm_side || c->audit_fault) && (rc = ctx_lone_streams(c))) return rc;
        c->stream_counts[2] += xside;  // zk_ctx_stream_info
        c->stream_counts[3] += c->msm_side;
        if ((rc = ctx_get_twiddles(c, lay.k, &tw)) || (rc = ctx_get_twiddles(c, lay.ext_k, &tw_ext))) return rc;
        // auto: columns of 2^16 rows or more (measured, tools/r6_cosets3_ab.sh: k = 18 / 17 / 16 - 1 / - 3 / - 3 %, k = 17 EVM over four
        // pipelines 196 -> 203 proofs/s; the many-column rows lose — three vectors per column fill the transforms' launches three
        // times as fast: k = 13 / 12 / 11 + 5 / + 5 / + 12 %)
        // (the members of a lock-step batch read the key's coset-major copies, made by lane 0's begin(): pk_ensure_cosets3)
        {
            const uint32_t above = c->opt_tail_main_above ? c->opt_tail_main_above : 2u;
            loaded = c->opt_tail_stream == 2 || (c->opt_tail_stream == 0 && (uint32_t)ctx_activity_touch(c) > above);
        }
        cosets3 = lay.n_h == 3 && 3 <= ctx_ntt_max_batch(lay.k) &&
                  (c->opt_quotient_domain == 2 || (c->opt_quotient_domain == 0 && lay.k >= 16));
        if (cosets3 && !pk->is_member && (rc = pk_ensure_cosets3(c, pk))) return rc;
        omega = fr_omega(lay.k);
        omega_inv = fe_inv_fast(omega);
        tr->common_scalar(pk->transcript_repr);
        if (instance && absorb_instance)
            for (const Fr& v : *instance) tr->common_scalar(v);  // (the count is not hashed)
        return ZK_OK;
    }
    // ---- multi-open, in stages: each stage ends with polynomials launched whose commitments the transcript needs next, so
    // that the driver (prover_lockstep.h) can put the same commitment of all its proofs into ONE MSM pass.

    // GWC (ProverGWC, halo2_proofs poly/kzg/multiopen/gwc): one witness polynomial per rotation.
    // Stage 1 (squeezes v): every set's (sum v^i p_i - sum v^i e_i) / (X - point), all in one batched division; the witness
    // polynomials — to be committed in this order, no challenge in between — are returned in `wit`.
    int gwc_stage1(const std::vector<Q>& queries, const Fr& x, std::vector<const Fr*>& wit) {
        const Fr v = tr->squeeze();
        std::vector<std::pair<int, std::vector<Q>>> sets;
        for (auto& qq : queries) {
            bool found = false;
            for (auto& s : sets)
                if (s.first == qq.rot) {
                    s.second.push_back(qq);
                    found = true;
                    break;
                }
            if (!found) sets.push_back({qq.rot, {qq}});
        }
        // Buffers: the h pieces (free once h(X) has been combined) and two temporaries — GWC has at most six rotation sets.
        Fr* wbuf[6] = {pk->h_ext, pk->h_ext + n, pk->h_ext + 2 * (size_t)n, pk->h_ext + 3 * (size_t)n, pk->t_num, pk->t_den};
        if (sets.size() > 6) return ZK_ESTATE;
        size_t set_idx = 0;
        Fr pts[6];
        for (auto& s : sets) {
            std::vector<Term> terms;
            Fr pv = Fr::one(), eb = Fr::zero();
            for (auto& qq : s.second) {
                terms.push_back(Term{qq.poly, pv});
                eb = fe_add(eb, fe_mul(pv, qq.eval));
                pv = fe_mul(pv, v);
            }
            lincomb_many(wbuf[set_idx], terms, true, eb);
            pts[set_idx] = xrot(x, s.first);
            set_idx++;
            if (!ok()) return rc;
        }
        if (c->audit.on) {
            std::vector<const void*> b(wbuf, wbuf + set_idx);
            AV(b, b, "GWC: division by (X - point)");
        }
        launch_kate_division_batch(wbuf, wbuf, pts, (uint32_t)set_idx, n, pk->kd_scratch, st);
        for (size_t i = 0; i < set_idx; i++) wit.push_back(wbuf[i]);
        return rc;
    }

    // SHPLONK (ProverSHPLONK, poly/kzg/multiopen/shplonk)
    struct CR {  // a polynomial with its rotations (sorted by point value) and evaluations
        const Fr* poly;
        std::vector<int> rots;
        std::vector<Fr> evals;
    };
    struct RotPt {
        int rot;
        Fr pt, canon;
    };
    struct RS {
        std::vector<int> rots;     // sorted by point value (BTreeSet<Fr>)
        std::vector<size_t> coms;  // indices into `com`
    };
    struct Shplonk {  // what stage 2 needs of stage 1
        std::vector<CR> com;
        std::vector<RotPt> rot_pts;
        std::vector<RS> rsets;
        std::vector<int> all_rots;
        std::vector<std::vector<Fr>> low;  // per commitment: its remainder polynomial (degree < |rotation set|)
        Fr yc, v;
        Fr* hx = nullptr;
    };
    static const RotPt& sh_rot_pt(const Shplonk& S, int r) {
        for (auto& e : S.rot_pts)
            if (e.rot == r) return e;
        return S.rot_pts[0];  // (every rotation of a query is in the list: shplonk_stage1 fills it first)
    }
    // Stage 1 (squeezes y, v): h(X) = sum_i v^i (sum_j y^j (P_ij - R_ij)) / Z_i is launched; its commitment comes next.
    int shplonk_stage1(const std::vector<Q>& queries, const Fr& x, Shplonk& S) {
        // group commitments by their set of rotations
        std::vector<CR>& com = S.com;
        {
            std::unordered_map<const Fr*, size_t> seen;  // wide circuits open hundreds of polynomials: no linear searches here
            seen.reserve(queries.size());
            for (auto& qq : queries) {
                auto it = seen.find(qq.poly);
                if (it == seen.end()) {
                    it = seen.emplace(qq.poly, com.size()).first;
                    com.push_back(CR{qq.poly, {}, {}});
                }
                com[it->second].rots.push_back(qq.rot);
                com[it->second].evals.push_back(qq.eval);
            }
        }
        // the points, once per distinct rotation: x w^rot and its canonical image (BTreeSet<Fr> orders by the integer value)
        for (auto& qq : queries) {
            bool have = false;
            for (auto& e : S.rot_pts) have = have || e.rot == qq.rot;
            if (!have) {
                const Fr pt = xrot(x, qq.rot);
                S.rot_pts.push_back(RotPt{qq.rot, pt, fe_from_mont(pt)});
            }
        }
        auto pt_less = [&](int ra, int rb) {
            const Fr &a = sh_rot_pt(S, ra).canon, &b = sh_rot_pt(S, rb).canon;
            for (int i = 7; i >= 0; i--)
                if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
            return false;
        };
        std::vector<RS>& rsets = S.rsets;
        std::vector<int>& all_rots = S.all_rots;
        for (size_t ci = 0; ci < com.size(); ci++) {
            CR& cr = com[ci];
            // sort this commitment's (rot, eval) pairs by point
            std::vector<size_t> order(cr.rots.size());
            for (size_t i = 0; i < order.size(); i++) order[i] = i;
            std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return pt_less(cr.rots[a], cr.rots[b]); });
            std::vector<int> r2;
            std::vector<Fr> e2;
            for (size_t i : order) {
                r2.push_back(cr.rots[i]);
                e2.push_back(cr.evals[i]);
            }
            cr.rots = r2;
            cr.evals = e2;
            for (int r : cr.rots)
                if (std::find(all_rots.begin(), all_rots.end(), r) == all_rots.end()) all_rots.push_back(r);
            size_t hit = rsets.size();
            for (size_t si = 0; si < rsets.size(); si++)
                if (rsets[si].rots == cr.rots) hit = si;  // (the last match, as before: sets are distinct, so the only one)
            if (hit == rsets.size()) rsets.push_back(RS{cr.rots, {}});
            rsets[hit].coms.push_back(ci);
        }
        std::sort(all_rots.begin(), all_rots.end(), pt_less);
        HT("grouped");
        S.yc = tr->squeeze();
        S.v = tr->squeeze();
        const Fr yc = S.yc, v = S.v;
        S.low.assign(com.size(), {});
        // h(X) = sum_i v^i * ( sum_j y^j (P_ij - R_ij) ) / Z_i.  Every rotation set has its own buffer (the h pieces
        // are free by now); step s divides, in ONE batched launch, every set that still has a point left by it.
        Fr* hx = pk->t_frac;  // h(X)
        S.hx = hx;
        Fr* sbuf[6] = {pk->h_ext, pk->h_ext + n, pk->h_ext + 2 * (size_t)n, pk->h_ext + 3 * (size_t)n, pk->t_num, pk->t_den};
        if (rsets.size() > 6) return ZK_ESTATE;
        std::vector<std::vector<Fr>> set_pts;
        size_t max_pts = 0;
        for (size_t si = 0; si < rsets.size(); si++) {
            auto& rs = rsets[si];
            std::vector<Fr> pts;
            for (int r : rs.rots) pts.push_back(sh_rot_pt(S, r).pt);
            const std::vector<std::vector<Fr>> basis = lagrange_basis(pts);
            std::vector<Term> terms;
            std::vector<Fr> rsum(pts.size(), Fr::zero());
            Fr py = Fr::one();
            for (size_t ci : rs.coms) {
                const CR& cr = com[ci];
                std::vector<Fr>& lo = S.low[ci];
                lo.assign(pts.size(), Fr::zero());
                for (size_t j = 0; j < pts.size(); j++)
                    for (size_t t = 0; t < pts.size(); t++) lo[t] = fe_add(lo[t], fe_mul(basis[j][t], cr.evals[j]));
                terms.push_back(Term{cr.poly, py});
                for (size_t t = 0; t < pts.size(); t++) rsum[t] = fe_add(rsum[t], fe_mul(py, lo[t]));
                py = fe_mul(py, yc);
            }
            // sum_j y^j P_j(X) minus sum_j y^j R_j(X) (degree < |set|: a few low coefficients, known on the host)
            if (pts.size() > 8) return ZK_ESTATE;
            lincomb_many(sbuf[si], terms, false, Fr::zero(), false, &rsum);
        HT("set lincomb launched");
            max_pts = std::max(max_pts, pts.size());
            set_pts.push_back(pts);
        }
        for (size_t step = 0; step < max_pts; step++) {
            Fr* bufs[6];
            Fr zs[6];
            uint32_t cnt = 0;
            for (size_t si = 0; si < rsets.size(); si++)
                if (step < set_pts[si].size()) {
                    bufs[cnt] = sbuf[si];
                    zs[cnt] = set_pts[si][step];
                    cnt++;
                }
            if (c->audit.on) {
                std::vector<const void*> b(bufs, bufs + cnt);
                AV(b, b, "SHPLONK: division step");
            }
            launch_kate_division_batch(bufs, bufs, zs, cnt, n, pk->kd_scratch, st);
        }
        {
            std::vector<Term> terms;
            Fr pv = Fr::one();
            for (size_t si = 0; si < rsets.size(); si++) {
                terms.push_back(Term{sbuf[si], pv});
                pv = fe_mul(pv, v);
            }
            lincomb_many(hx, terms, false, Fr::zero());
        HT("hx launched");
        }
        return rc;
    }
    // Stage 2 (h's commitment is in the transcript; squeezes u): the final quotient (L(X) / (X - u)) / z_0 is launched in
    // *out; its commitment ends the proof.
    int shplonk_stage2(Shplonk& S, const Fr** out) {
        const Fr u = tr->squeeze();
        HT("u squeezed");
        // L(X) = sum_i v^i z_i sum_j y^j (P_ij(X) - R_ij(u)) - Z_T(u) h(X)
        std::vector<Term> terms;
        Fr sub = Fr::zero();
        Fr pv = Fr::one();
        std::vector<Fr> z_diffs;
        for (auto& rs : S.rsets) {
            std::vector<Fr> diffs;
            for (int r : S.all_rots)
                if (std::find(rs.rots.begin(), rs.rots.end(), r) == rs.rots.end()) diffs.push_back(sh_rot_pt(S, r).pt);
            const Fr zi = vanishing_eval(diffs, u);
            z_diffs.push_back(zi);
            Fr py = Fr::one();
            for (size_t ci : rs.coms) {
                const Fr coef = fe_mul(fe_mul(pv, zi), py);
                terms.push_back(Term{S.com[ci].poly, coef});
                sub = fe_add(sub, fe_mul(coef, eval_small(S.low[ci], u)));
                py = fe_mul(py, S.yc);
            }
            pv = fe_mul(pv, S.v);
        }
        std::vector<Fr> all_pts;
        for (int r : S.all_rots) all_pts.push_back(sh_rot_pt(S, r).pt);
        const Fr zt = vanishing_eval(all_pts, u);
        terms.push_back(Term{S.hx, fe_neg(zt)});
        lincomb_many(pk->t_a, terms, true, sub);
        HT("L launched");
        A({pk->t_a}, {pk->t_b}, "SHPLONK: final division");
        launch_kate_division(pk->t_a, pk->t_b, n, u, pk->kd_scratch, st);
        A({pk->t_b}, {pk->t_b}, "SHPLONK: scale");
        launch_scale(pk->t_b, fe_inv_fast(z_diffs[0]), n, st);
        *out = pk->t_b;
        return rc;
    }
};

#include "prover_lockstep.h"

}  // namespace

// Leaves the context as every entry point expects to find it — no commitment in flight, the side streams drained and their
// flags cleared, the main stream idle — on EVERY way out of a whole-proof call, including an exception thrown inside the
// prover (std::bad_alloc from its vectors: ZK_API turns it into ZK_EINTERNAL after this destructor has run)
namespace {
struct ProveQuiesce {
    zk_ctx* c;
    explicit ProveQuiesce(zk_ctx* ctx) : c(ctx) { ctx_activity_hold(c, true); }
    ProveQuiesce(const ProveQuiesce&) = delete;
    ProveQuiesce& operator=(const ProveQuiesce&) = delete;
    void settle() {
        ctx_msm_drain(c);  // an early error may leave commitments in flight
        if (c->msm_side) {
            aud_sync(c, c->msm_stream);
            c->msm_side = false;
        }
        if (c->xform_pending) {  // (an early error before the quotient: transforms still in flight)
            aud_sync(c, c->xform_stream);
            c->xform_pending = false;
        }
        aud_sync(c, c->stream);
        ctx_activity_hold(c, false);
    }
    ~ProveQuiesce() { settle(); }
};
}  // namespace

// the bytes of one proof over n_circuits circuits (zk_prove: one).  Per circuit its own commitments — advice, (a', s', zL) per
// lookup, z per chunk — and evaluations (advice, z, lookups); once the random polynomial, the h pieces, the fixed / random / sigma
// evaluations and the opening proof: SHPLONK two points, GWC one per distinct rotation {0,1,2,3,-1} (+ `last` once there is a
// chunk link)
static int proof_size(zk_ctx* c, zk_pk pkh, size_t n_circuits, int transcript, int scheme, size_t* out) {
    std::lock_guard<std::mutex> g(c->mu);
    auto it = c->pks.find(pkh);
    if (it == c->pks.end()) return ZK_EINVAL;
    if (int r = resolve_scheme(transcript, &scheme)) return r;
    const Layout& lay = it->second->lay;
    size_t points = n_circuits * (lay.n_adv + 3 * lay.n_lookups + lay.n_chunks) + 1 + lay.n_h;
    points += scheme == ZK_SCHEME_SHPLONK ? 2 : 5 + (lay.n_chunks > 1 ? 1 : 0);
    const size_t evals = n_circuits * (lay.advice_queries.size() + 3 * lay.n_chunks - 1 + 5 * lay.n_lookups) + lay.n_fix + 1 + lay.perm_cols.size();
    *out = points * (transcript == ZK_TRANSCRIPT_EVM ? 64 : 32) + evals * 32;
    return ZK_OK;
}

ZK_API(zk_proof_size, (zk_ctx* c, zk_pk pkh, int transcript, int scheme, size_t* out), (c, pkh, transcript, scheme, out)) {
    if (!c || !out) return ZK_EINVAL;
    return proof_size(c, pkh, 1, transcript, scheme, out);
}

ZK_API(zk_proof_size_multi, (zk_ctx* c, zk_pk pkh, size_t n_circuits, int transcript, int scheme, size_t* out), (c, pkh, n_circuits, transcript, scheme, out)) {
    if (!c || !out || n_circuits == 0 || n_circuits > ZK_PROVE_MULTI_MAX) return ZK_EINVAL;
    return proof_size(c, pkh, n_circuits, transcript, scheme, out);
}

// ---- admission: the checks every whole-proof entry point makes, each in the order it always made them (which code comes back
// when two faults coincide is behaviour: prove_one has the instances first, the lock-step forms the key)
// key state and shape
static int admit_key(const zk_ctx* c, const zk_pk_rec* pk, size_t n_advice) {
    if (pk->srs_gen != c->srs_gen) return ZK_ESTATE;  // the SRS was replaced after this key was made: its vk is stale
    if (pk->verify_only) return ZK_ESTATE;  // a verifying-only key (zk_vk_read / zk_vk_from_parts) has no key polynomials
    if (n_advice != pk->lay.n_adv || c->srs_k != (int)pk->lay.k) return ZK_EINVAL;
    return ZK_OK;
}
// the `count` instance lists of a call (pk_instance_lists' rules); the forms without instances carry none and refuse a key WITH the
// column (halo2's InvalidInstances)
static int admit_instances(const Layout& lay, bool with_instances, size_t count, const uint64_t* const* instances_mont, const size_t* n_instances,
                           std::vector<std::vector<Fr>>* lists) {
    if (lay.n_inst && !with_instances) return ZK_EINVAL;
    return with_instances ? pk_instance_lists(lay, count, instances_mont, n_instances, lists) : ZK_OK;
}
// (transcript and scheme: resolve_scheme, pk.h)

// the advice handles of a call, as device pointers
static int resolve_advice(zk_ctx* c, const Layout& lay, const zk_poly* advice, size_t count, std::vector<const Fr*>* adv) {
    adv->resize(count);
    for (size_t j = 0; j < count; j++) {
        const PolyRec* r = ctx_poly(c, advice[j]);
        if (!r || r->n != lay.n) return ZK_EINVAL;
        (*adv)[j] = r->ptr;
    }
    return ZK_OK;
}

// the run of an admitted call (prover_lockstep.h) over its lanes' provers — one: a lone proof — under the stream audit's verdict
static int run_lanes(zk_ctx* c, zk_pk_rec* pk, const std::vector<Prover*>& P, bool one_proof, uint32_t pass_cap, const Fr* const* adv, int scheme) {
    const uint64_t aud0 = c->audit.violations;
    c->audit.base_of.clear();  // (allocations may have changed hands since the last proof)
    int rc;
    {
        LockstepRun run(c, pk, P, one_proof, pass_cap);
        ProveQuiesce quiesce(c);  // (made after the provers: it settles the streams while their host buffers are alive)
        rc = run.run(adv, scheme);
    }
    if ((rc = aud_verdict(c, aud0, rc))) return rc;
    if (hipGetLastError() != hipSuccess) return ZK_EHIP;
    return ZK_OK;
}

// create_proof for one circuit: the driver at one lane.  `with_instances`: zk_prove_public — the caller's instance values (none on a key without the
// column: zk_prove's bytes); otherwise zk_prove, which a key WITH the column refuses (halo2's InvalidInstances)
static int prove_one(zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, bool with_instances, const uint64_t* instance_mont,
                     size_t n_instance, const uint8_t rng_seed[32], int transcript, int scheme, uint8_t* proof_out, size_t proof_cap,
                     size_t* proof_len) {
    if (!c || !advice || !rng_seed || !proof_len) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    const Layout& lay = pk->lay;
    std::vector<std::vector<Fr>> lists;  // (the one list)
    if (int r = admit_instances(lay, with_instances, 1, &instance_mont, &n_instance, &lists)) return r;
    if (int r = admit_key(c, pk, n_advice)) return r;
    if (int r = resolve_scheme(transcript, &scheme)) return r;
    int rc = ctx_bind(c);
    if (rc) return rc;
    std::vector<const Fr*> adv;
    if ((rc = resolve_advice(c, lay, advice, n_advice, &adv))) return rc;
    EvmTranscript evm;
    Blake2bTranscript b2;
    Transcript* tr = transcript == ZK_TRANSCRIPT_EVM ? (Transcript*)&evm : (Transcript*)&b2;
    // the one lane: a prover on the key's own workspace, the pass width the context's own
    Prover p(c, pk, rng_seed, tr);
    if (lay.n_inst) p.instance = &lists[0];
    if ((rc = run_lanes(c, pk, {&p}, false, ctx_msm_max_batch(c), adv.data(), scheme))) return rc;
    *proof_len = tr->out.size();
    if (!proof_out || proof_cap < tr->out.size()) return proof_out ? ZK_EINVAL : ZK_OK;
    memcpy(proof_out, tr->out.data(), tr->out.size());
    return ZK_OK;
}

ZK_API(zk_prove, (zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, const uint8_t rng_seed[32], int transcript, int scheme, uint8_t* proof_out, size_t proof_cap, size_t* proof_len), (c, h, advice, n_advice, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len)) {
    return prove_one(c, h, advice, n_advice, false, nullptr, 0, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len);
}

// create_proof with the circuit's public inputs: one instance column, absorbed into the transcript and copy-constrained
ZK_API(zk_prove_public, (zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, const uint64_t* instance_mont, size_t n_instance, const uint8_t rng_seed[32], int transcript, int scheme, uint8_t* proof_out, size_t proof_cap, size_t* proof_len), (c, h, advice, n_advice, instance_mont, n_instance, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len)) {
    return prove_one(c, h, advice, n_advice, true, instance_mont, n_instance, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len);
}

// the one-list forms of the entry points below (batch == 1, n_circuits == 1): zk_prove_public with list 0
static int prove_one_of_lists(zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, const uint64_t* const* instances_mont,
                              const size_t* n_instances, const uint8_t rng_seed[32], int transcript, int scheme, uint8_t* proof_out, size_t proof_cap,
                              size_t* proof_len) {
    uint32_t cols = 0;
    if (int r = zk_pk_num_instance_columns(c, h, &cols)) return r;
    if (cols && !n_instances) return ZK_EINVAL;
    const size_t m = n_instances ? n_instances[0] : 0;
    return zk_prove_public(c, h, advice, n_advice, m && instances_mont ? instances_mont[0] : nullptr, m, rng_seed, transcript, scheme, proof_out,
                           proof_cap, proof_len);
}

// ---- the lock-step entry (prover_lockstep.h) for two or more lanes: what zk_prove_batch and zk_prove_multi do alike once a call is admitted.  Lane q —
// proof q, or circuit q of the one proof — gets a prover on the key's own workspace (q = 0) or on member q - 1, with the
// caller's transcript and seed for it and, on a key with the column, list q.  The callers keep what is their own: whose
// transcripts and seeds these are, and the copy of the output
struct LockstepLane {
    Transcript* tr;
    const uint8_t* seed;
};
static int prove_lockstep(zk_ctx* c, zk_pk_rec* pk, bool one_proof, const std::vector<LockstepLane>& lanes, const std::vector<std::vector<Fr>>& lists,
                          const zk_poly* advice, int scheme) {
    const Layout& lay = pk->lay;
    const uint32_t B = (uint32_t)lanes.size();
    // all grand products of the call are scanned by one 256-lane workgroup (gp_chain_kernel)
    if ((uint64_t)B * (lay.n_chunks + lay.n_lookups) > 256) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    std::vector<const Fr*> adv;
    if ((rc = resolve_advice(c, lay, advice, (size_t)B * lay.n_adv, &adv))) return rc;
    if ((rc = one_proof ? pk_ensure_multi(c, pk, B) : pk_ensure_batch(c, pk, B))) return rc;
    // columns per MSM pass: the same commitment of all lanes at once, two columns per lane where a phase has them (a', s';
    // z, zL) — ZK_OPT_BATCH_PASS_COLUMNS overrides; the lanes' workspaces grow to that on their next pass
    uint32_t cap = c->opt_batch_pass_cols ? c->opt_batch_pass_cols : std::max(std::min<uint32_t>(2 * B, 8u), ctx_msm_max_batch(c));
    cap = ctx_msm_pass_cap(c, cap);  // at most MSM_MAX_BATCH; one column per pass without window tables (k < 10) and on the swept sort (k >= 22)
    c->msm_min_cols = std::max(c->msm_min_cols, cap);
    std::vector<std::unique_ptr<Prover>> provers;
    std::vector<Prover*> P;
    for (uint32_t q = 0; q < B; q++) {
        provers.emplace_back(new Prover(c, q == 0 ? pk : pk->members[q - 1], lanes[q].seed, lanes[q].tr));
        if (lay.n_inst) provers.back()->instance = &lists[q];
        P.push_back(provers.back().get());
    }
    return run_lanes(c, pk, P, one_proof, cap, adv.data(), scheme);
}

// create_proof for `batch` independent proofs of one key in lock-step.  `with_instances`: zk_prove_batch_public —
// one list per proof; otherwise zk_prove_batch, which a key WITH the column refuses
static int prove_batch(zk_ctx* c, zk_pk h, size_t batch, const zk_poly* advice, size_t n_advice, bool with_instances,
                       const uint64_t* const* instances_mont, const size_t* n_instances, const uint8_t* rng_seeds, int transcript, int scheme,
                       uint8_t* proofs_out, size_t proof_stride, size_t* proof_len) {
    if (!c || !advice || !rng_seeds || !proof_len || batch == 0 || batch > ZK_PROVE_BATCH_MAX) return ZK_EINVAL;
    if (batch == 1) {
        if (!with_instances) return zk_prove(c, h, advice, n_advice, rng_seeds, transcript, scheme, proofs_out, proof_stride, proof_len);
        return prove_one_of_lists(c, h, advice, n_advice, instances_mont, n_instances, rng_seeds, transcript, scheme, proofs_out, proof_stride, proof_len);
    }
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    if (int r = admit_key(c, pk, n_advice)) return r;
    std::vector<std::vector<Fr>> lists;  // (proof q's own list, absorbed by its own begin())
    if (int r = admit_instances(pk->lay, with_instances, batch, instances_mont, n_instances, &lists)) return r;
    if (int r = resolve_scheme(transcript, &scheme)) return r;
    const uint32_t B = (uint32_t)batch;
    // every proof its own transcript and its own seed
    std::vector<std::unique_ptr<Transcript>> trs;
    std::vector<LockstepLane> lanes;
    for (uint32_t q = 0; q < B; q++) {
        trs.emplace_back(transcript == ZK_TRANSCRIPT_EVM ? (Transcript*)new EvmTranscript() : (Transcript*)new Blake2bTranscript());
        lanes.push_back(LockstepLane{trs.back().get(), rng_seeds + 32 * (size_t)q});
    }
    if (int r = prove_lockstep(c, pk, false, lanes, lists, advice, scheme)) return r;
    const size_t len = trs[0]->out.size();
    for (uint32_t q = 0; q < B; q++)
        if (trs[q]->out.size() != len) return ZK_EINTERNAL;  // (one shape, one length)
    *proof_len = len;
    if (!proofs_out) return ZK_OK;
    if (proof_stride < len) return ZK_EINVAL;
    for (uint32_t q = 0; q < B; q++) memcpy(proofs_out + (size_t)q * proof_stride, trs[q]->out.data(), len);
    return ZK_OK;
}

ZK_API(zk_prove_batch, (zk_ctx* c, zk_pk h, size_t batch, const zk_poly* advice, size_t n_advice, const uint8_t* rng_seeds, int transcript, int scheme, uint8_t* proofs_out, size_t proof_stride, size_t* proof_len), (c, h, batch, advice, n_advice, rng_seeds, transcript, scheme, proofs_out, proof_stride, proof_len)) {
    return prove_batch(c, h, batch, advice, n_advice, false, nullptr, nullptr, rng_seeds, transcript, scheme, proofs_out, proof_stride, proof_len);
}

// the lock-step batch with every proof's public inputs: proof j is zk_prove_public's with list j
ZK_API(zk_prove_batch_public, (zk_ctx* c, zk_pk h, size_t batch, const zk_poly* advice, size_t n_advice, const uint64_t* const* instances_mont, const size_t* n_instances, const uint8_t* rng_seeds, int transcript, int scheme, uint8_t* proofs_out, size_t proof_stride, size_t* proof_len), (c, h, batch, advice, n_advice, instances_mont, n_instances, rng_seeds, transcript, scheme, proofs_out, proof_stride, proof_len)) {
    return prove_batch(c, h, batch, advice, n_advice, true, instances_mont, n_instances, rng_seeds, transcript, scheme, proofs_out, proof_stride, proof_len);
}

// create_proof(&params, &pk, &[c_0 .. c_{N-1}], &[inst_0 .. inst_{N-1}], ..): ONE proof over n_circuits circuits of one key
// (prover_lockstep.h).  `with_instances`: zk_prove_multi_public — one list per circuit; otherwise zk_prove_multi
static int prove_multi(zk_ctx* c, zk_pk h, size_t n_circuits, const zk_poly* advice, size_t n_advice, bool with_instances,
                       const uint64_t* const* instances_mont, const size_t* n_instances, const uint8_t rng_seed[32], int transcript, int scheme,
                       uint8_t* proof_out, size_t proof_cap, size_t* proof_len) {
    if (!c || !advice || !rng_seed || !proof_len || n_circuits == 0 || n_circuits > ZK_PROVE_MULTI_MAX) return ZK_EINVAL;
    if (n_circuits == 1) {
        if (!with_instances) return zk_prove(c, h, advice, n_advice, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len);
        return prove_one_of_lists(c, h, advice, n_advice, instances_mont, n_instances, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len);
    }
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    if (int r = admit_key(c, pk, n_advice)) return r;
    std::vector<std::vector<Fr>> lists;  // (circuit q's column; the driver absorbs the lists, no begin() does)
    if (int r = admit_instances(pk->lay, with_instances, n_circuits, instances_mont, n_instances, &lists)) return r;
    if (int r = resolve_scheme(transcript, &scheme)) return r;
    // the proof's transcript and RNG are circuit 0's prover's; circuits 1 .. N - 1 are workspaces: their provers get a scratch
    // transcript (begin() hashes transcript_repr into it) and a stream that is never drawn from
    EvmTranscript evm;
    Blake2bTranscript b2;
    Transcript* tr = transcript == ZK_TRANSCRIPT_EVM ? (Transcript*)&evm : (Transcript*)&b2;
    std::vector<Blake2bTranscript> scratch(n_circuits - 1);
    std::vector<LockstepLane> lanes;
    for (size_t q = 0; q < n_circuits; q++) lanes.push_back(LockstepLane{q == 0 ? tr : &scratch[q - 1], rng_seed});
    if (int r = prove_lockstep(c, pk, true, lanes, lists, advice, scheme)) return r;
    *proof_len = tr->out.size();
    if (!proof_out || proof_cap < tr->out.size()) return proof_out ? ZK_EINVAL : ZK_OK;
    memcpy(proof_out, tr->out.data(), tr->out.size());
    return ZK_OK;
}

ZK_API(zk_prove_multi, (zk_ctx* c, zk_pk h, size_t n_circuits, const zk_poly* advice, size_t n_advice, const uint8_t rng_seed[32], int transcript, int scheme, uint8_t* proof_out, size_t proof_cap, size_t* proof_len), (c, h, n_circuits, advice, n_advice, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len)) {
    return prove_multi(c, h, n_circuits, advice, n_advice, false, nullptr, nullptr, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len);
}

// one proof over n_circuits circuits with every circuit's public inputs (the rule: prover_lockstep.h / DESIGN.md section 3)
ZK_API(zk_prove_multi_public, (zk_ctx* c, zk_pk h, size_t n_circuits, const zk_poly* advice, size_t n_advice, const uint64_t* const* instances_mont, const size_t* n_instances, const uint8_t rng_seed[32], int transcript, int scheme, uint8_t* proof_out, size_t proof_cap, size_t* proof_len), (c, h, n_circuits, advice, n_advice, instances_mont, n_instances, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len)) {
    return prove_multi(c, h, n_circuits, advice, n_advice, true, instances_mont, n_instances, rng_seed, transcript, scheme, proof_out, proof_cap, proof_len);
}
