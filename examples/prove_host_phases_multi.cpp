// prove_host_phases_multi — the RESIDENT integration of INTEGRATION.md §2 executed for ONE proof over N circuits of one key, with
// their public inputs where the key has the instance column: what prove_host_phases.cpp does for the reference's shape (one
// circuit, no instances), for `create_proof(&params, &pk, &[c_0 .. c_{N-1}], &[&[&inst_0] .. ], rng, &mut transcript)`.
//
// The HOST owns the transcript, the ChaCha20 stream and the blinding; the DEVICE does the arithmetic between them through the
// phase-level C ABI (include/zkmi355.h) alone.  Beside the calls prove_host_phases.cpp makes:
//     permutation argument   zk_permutation_product_public   (circuit c's instance column is its last permutation column)
//     vanishing argument     zk_quotient_multi               (ONE h: the y-Horner chain runs on across the circuits)
//     openings               zk_eval_batch                   (every opened value of all circuits in one call)
// The order of draws and transcript writes is the one include/zkmi355.h states for zk_prove_public, zk_prove_multi and
// zk_prove_multi_public: all circuits' instances are absorbed behind transcript_repr before any commitment; every
// phase's draws and commitments run c = 0 .. N - 1; there is one random polynomial, one quotient and one multi-open.  The bytes
// are those calls' own for the same key, advice, lists and seed (tests/test_gpu_host_phases_multi.py).
//
// usage: prove_host_phases_multi <srs.bin> <pk.bin> <advice.bin> <instances.bin> <proof.out> k num_advice num_lookup_advice
//                                num_fixed lookup_bits idle num_instance_columns N <transcript: blake2b|evm>
//                                <rng seed: 64 hex digits> [gwc|shplonk]
//   advice.bin      N x n_advice columns of n canonical 32-byte values, circuit-major
//   instances.bin   per circuit: u64 LE count m_c, then m_c canonical 32-byte values (every count 0 for a key without the column)
//   multi-open      the reference's pairings by default — GWC under the EVM transcript, SHPLONK under Blake2b
// Prints to stderr how many ABI calls the proof took.
#include "phase_host.h"

int main(int argc, char** argv) {
    prog = "prove_host_phases_multi";
    if (argc != 16 && argc != 17) {
        fprintf(stderr, "usage: %s srs.bin pk.bin advice.bin instances.bin proof.out k A L F lookup_bits idle n_instance_columns N blake2b|evm seedhex [gwc|shplonk]\n", argv[0]);
        return 2;
    }
    zk_circuit_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.k = (uint32_t)atoi(argv[6]);
    prm.num_advice = (uint32_t)atoi(argv[7]);
    prm.num_lookup_advice = (uint32_t)atoi(argv[8]);
    prm.num_fixed = (uint32_t)atoi(argv[9]);
    prm.lookup_bits = (uint32_t)atoi(argv[10]);
    prm.num_idle_gate_columns = (uint32_t)atoi(argv[11]);
    prm.num_instance_columns = (uint32_t)atoi(argv[12]);
    const uint32_t NC = (uint32_t)atoi(argv[13]);  // circuits
    const bool evm = strcmp(argv[14], "evm") == 0;
    const bool shplonk = argc == 17 ? strcmp(argv[16], "shplonk") == 0 : !evm;
    uint8_t seed[32];
    if (NC == 0 || NC > ZK_PROVE_MULTI_MAX || !parse_seed(argv[15], seed)) return 2;
    CHECK(zk_ctx_create(0, &ctx));
    {
        const std::vector<uint8_t> srs = slurp(argv[1]);
        CHECK(zk_srs_read(ctx, srs.data(), srs.size(), ZK_SERDE_RAW_BYTES));
    }
    zk_pk pk = 0;
    {
        const std::vector<uint8_t> key = slurp(argv[2]);
        CHECK(zk_pk_read(ctx, &prm, key.data(), key.size(), ZK_SERDE_RAW_BYTES, nullptr, &pk));
    }
    uint32_t shape[8], n_inst = 0;
    CHECK(zk_pk_shape(ctx, pk, shape));
    CHECK(zk_pk_num_instance_columns(ctx, pk, &n_inst));
    const uint32_t k = shape[0], n_adv = shape[2], n_fix = shape[3], n_perm = shape[4], n_chunks = shape[5], n_lookups = shape[6], n_h = shape[7];
    const size_t n = (size_t)1 << k, N = 4 * n;
    const uint32_t A = prm.num_advice;  // gate columns: queried at rotations 0 .. 3; lookup advice columns at 0
    const uint32_t bf = 6;              // blinding factors; rows n - 7 .. n - 1 of a column are the prover's
    const size_t usable = n - (bf + 1);
    const int last_rot = -(int)(bf + 1);
    Fr repr;
    {
        uint32_t counts[2];
        CHECK(zk_vk_export(ctx, pk, nullptr, nullptr, reinterpret_cast<uint64_t*>(repr.v), counts));
    }
    const Rotations xrot(k);
    // the public inputs of every circuit (Montgomery images)
    std::vector<std::vector<Fr>> inst(NC);
    {
        const std::vector<uint8_t> file = slurp(argv[4]);
        size_t pos = 0;
        for (uint32_t c = 0; c < NC; c++) {
            uint64_t m = 0;
            if (pos + 8 > file.size()) return 2;
            memcpy(&m, file.data() + pos, 8);
            pos += 8;
            if (m > usable || (m && !n_inst) || pos + 32 * m > file.size()) {
                fprintf(stderr, "%s: instance list %u does not fit the key (halo2: InvalidInstances / InstanceTooLarge)\n", prog, c);
                return 2;
            }
            for (uint64_t i = 0; i < m; i++, pos += 32) {
                Fr v;
                memcpy(v.v, file.data() + pos, 32);
                inst[c].push_back(fe_to_mont(v));
            }
        }
        if (pos != file.size()) return 2;
    }
    const size_t calls_before = abi_calls;  // what follows is the proof

    EvmTranscript evm_tr;
    Blake2bTranscript b2_tr;
    Transcript& tr = evm ? static_cast<Transcript&>(evm_tr) : static_cast<Transcript&>(b2_tr);
    ChaCha20Rng rng(seed);  // the host's RNG: ONE stream for the whole proof
    auto draw = [&](uint32_t count) {
        std::vector<Fr> v(count);
        for (Fr& x : v) x = rng.next_fr();
        return v;
    };
    auto blind = [&](zk_poly col, size_t first, uint32_t count) {  // rows [first, first + count) = fresh randomness
        const std::vector<Fr> v = draw(count);
        CHECK(zk_poly_upload_range(ctx, col, first, reinterpret_cast<const uint64_t*>(v.data()), count));
    };
    tr.common_scalar(repr);
    for (uint32_t c = 0; c < NC; c++)  // ALL circuits' instances before any commitment (neither N nor the lengths are hashed)
        for (const Fr& v : inst[c]) tr.common_scalar(v);

    // ---- 0. the instance columns: values in rows 0 .. m - 1, zero behind them; not blinded, not committed, drawing nothing
    std::vector<zk_poly> inst_val(NC, 0);
    if (n_inst) {
        std::vector<Fr> col(n);
        for (uint32_t c = 0; c < NC; c++) {
            std::fill(col.begin(), col.end(), Fr::zero());
            std::copy(inst[c].begin(), inst[c].end(), col.begin());
            inst_val[c] = alloc(n);
            CHECK(zk_poly_upload(ctx, inst_val[c], reinterpret_cast<const uint64_t*>(col.data()), n));
        }
    }

    // ---- 1. advice of every circuit, blinded on the host, shipped once; the commitments of all circuits, circuit by circuit
    std::vector<std::vector<zk_poly>> adv(NC, std::vector<zk_poly>(n_adv));
    {
        const std::vector<uint8_t> file = slurp(argv[3]);
        if (file.size() != (size_t)NC * n_adv * n * 32) {
            fprintf(stderr, "%s: %s does not hold %u x %u columns of %zu rows\n", prog, argv[3], NC, n_adv, n);
            return 2;
        }
        std::vector<Fr> col(n);
        std::vector<zk_poly> order;
        for (uint32_t c = 0; c < NC; c++) {
            for (uint32_t j = 0; j < n_adv; j++) {
                for (size_t r = 0; r < usable; r++) {
                    Fr v;
                    memcpy(v.v, file.data() + (((size_t)c * n_adv + j) * n + r) * 32, 32);
                    col[r] = fe_to_mont(v);
                }
                const std::vector<Fr> b = draw(bf + 1);
                for (uint32_t t = 0; t <= bf; t++) col[usable + t] = b[t];
                adv[c][j] = alloc(n);
                CHECK(zk_poly_upload(ctx, adv[c][j], reinterpret_cast<const uint64_t*>(col.data()), n));
                order.push_back(adv[c][j]);
            }
            draw(n_adv);  // circuit c's advice blinds
        }
        commit_write(tr, order, ZK_BASIS_LAGRANGE);
    }
    (void)tr.squeeze();  // theta: ONE, after the last circuit's advice

    // ---- 2. lookup argument of every circuit
    std::vector<std::vector<zk_poly>> ap(NC, std::vector<zk_poly>(n_lookups)), sp = ap, zl = ap;
    {
        std::vector<zk_poly> order;
        for (uint32_t c = 0; c < NC; c++) {
            for (uint32_t l = 0; l < n_lookups; l++) {
                ap[c][l] = alloc(n);
                sp[c][l] = alloc(n);
                zl[c][l] = alloc(n);
            }
            CHECK(zk_lookup_permute(ctx, pk, adv[c].data(), n_adv, ap[c].data(), sp[c].data(), n_lookups));
            for (uint32_t l = 0; l < n_lookups; l++) {
                blind(ap[c][l], usable, bf + 1);
                blind(sp[c][l], usable, bf + 1);
                draw(2);
                order.push_back(ap[c][l]);
                order.push_back(sp[c][l]);
            }
        }
        commit_write(tr, order, ZK_BASIS_LAGRANGE);
    }
    const Fr beta = tr.squeeze(), gamma = tr.squeeze();

    // ---- 3. grand products: the permutation products of every circuit (circuit c's reads c's instance column), then the lookup
    // products of every circuit — draws and commitments in that order
    std::vector<std::vector<zk_poly>> z(NC, std::vector<zk_poly>(n_chunks));
    {
        std::vector<zk_poly> order;
        for (uint32_t c = 0; c < NC; c++) {
            for (uint32_t ci = 0; ci < n_chunks; ci++) z[c][ci] = alloc(n);
            CHECK(zk_permutation_product_public(ctx, pk, adv[c].data(), n_adv, inst_val[c], limbs(beta), limbs(gamma), z[c].data(), n_chunks));
            for (uint32_t ci = 0; ci < n_chunks; ci++) {
                blind(z[c][ci], n - bf, bf);
                draw(1);
                order.push_back(z[c][ci]);
            }
        }
        for (uint32_t c = 0; c < NC; c++) {
            CHECK(zk_lookup_product(ctx, pk, adv[c].data(), n_adv, ap[c].data(), sp[c].data(), n_lookups, limbs(beta), limbs(gamma), zl[c].data()));
            for (uint32_t l = 0; l < n_lookups; l++) {
                blind(zl[c][l], n - bf, bf);
                draw(1);
                order.push_back(zl[c][l]);
            }
        }
        commit_write(tr, order, ZK_BASIS_LAGRANGE);
    }

    // ---- 4. vanishing argument: ONE random polynomial — n draws of the host's stream, expanded on the device
    zk_poly rnd = alloc(n);
    CHECK(zk_random_poly(ctx, rng.key, rng.block, rnd));
    rng.block += n;
    draw(1);
    commit_write(tr, {rnd}, ZK_BASIS_MONOMIAL);
    const Fr y = tr.squeeze();

    // ---- 5. coefficient and extended-coset forms of every circuit's columns (the instance column as an advice column), then ONE h
    auto to_poly = [&](zk_poly values) {
        zk_poly p = alloc(n);
        CHECK(zk_poly_copy(ctx, p, values));
        CHECK(zk_lagrange_to_coeff(ctx, p));
        return p;
    };
    auto to_ext = [&](zk_poly poly) {
        zk_poly e = alloc(N);
        CHECK(zk_coeff_to_extended(ctx, poly, e));
        return e;
    };
    std::vector<std::vector<zk_poly>> adv_p(NC), z_p(NC), ap_p(NC), sp_p(NC), zl_p(NC);
    std::vector<zk_poly> adv_e, z_e, lk_e, inst_e;  // circuit-major
    for (uint32_t c = 0; c < NC; c++) {
        for (uint32_t j = 0; j < n_adv; j++) {
            adv_p[c].push_back(to_poly(adv[c][j]));
            adv_e.push_back(to_ext(adv_p[c][j]));
        }
        for (uint32_t ci = 0; ci < n_chunks; ci++) {
            z_p[c].push_back(to_poly(z[c][ci]));
            z_e.push_back(to_ext(z_p[c][ci]));
        }
        for (uint32_t l = 0; l < n_lookups; l++) {
            ap_p[c].push_back(to_poly(ap[c][l]));
            sp_p[c].push_back(to_poly(sp[c][l]));
            zl_p[c].push_back(to_poly(zl[c][l]));
            lk_e.push_back(to_ext(ap_p[c][l]));
            lk_e.push_back(to_ext(sp_p[c][l]));
            lk_e.push_back(to_ext(zl_p[c][l]));
        }
        if (n_inst) inst_e.push_back(to_ext(to_poly(inst_val[c])));
    }
    zk_poly h_ext = alloc(N);
    CHECK(zk_quotient_multi(ctx, pk, NC, adv_e.data(), n_adv, n_inst ? inst_e.data() : nullptr, z_e.data(), n_chunks, lk_e.data(), n_lookups,
                            limbs(beta), limbs(gamma), limbs(y), 1, h_ext));
    CHECK(zk_extended_to_coeff(ctx, h_ext, (size_t)n_h * n));
    draw(n_h);  // the h pieces' blinds
    std::vector<zk_poly> h_piece(n_h);
    for (uint32_t i = 0; i < n_h; i++) {
        h_piece[i] = alloc(n);
        CHECK(zk_poly_copy_range(ctx, h_piece[i], 0, h_ext, (size_t)i * n, n));
    }
    commit_write(tr, h_piece, ZK_BASIS_MONOMIAL);
    const Fr x = tr.squeeze();

    // ---- 6. evaluations, in transcript order: for c: advice; fixed, once; random; sigma, once; for c: the permutation's; for c:
    // the lookups'; then h(x) (not written) — every value in ONE zk_eval_batch
    std::vector<zk_poly> fixed_p(n_fix), sigma_p(n_perm);
    for (uint32_t f = 0; f < n_fix; f++) CHECK(zk_pk_export_poly(ctx, pk, ZK_PK_FIXED_POLY, f, fixed_p[f] = alloc(n)));
    for (uint32_t p = 0; p < n_perm; p++) CHECK(zk_pk_export_poly(ctx, pk, ZK_PK_SIGMA_POLY, p, sigma_p[p] = alloc(n)));
    zk_poly h_comb = alloc(n);
    {
        std::vector<Fr> cf(n_h);
        const Fr xn = fe_pow_u64(x, n);
        Fr p = Fr::one();
        for (uint32_t i = 0; i < n_h; i++) {
            cf[i] = p;
            p = fe_mul(p, xn);
        }
        CHECK(zk_poly_lincomb(ctx, h_comb, h_piece.data(), reinterpret_cast<const uint64_t*>(cf.data()), n_h, nullptr, 0));
    }
    std::vector<Q> ev;
    std::vector<size_t> i_adv(NC), i_z(NC), i_lk(NC);
    for (uint32_t c = 0; c < NC; c++) {
        i_adv[c] = ev.size();
        for (uint32_t j = 0; j < A; j++)
            for (int r = 0; r < 4; r++) ev.push_back(Q{adv_p[c][j], r, Fr::zero()});
        for (uint32_t j = A; j < n_adv; j++) ev.push_back(Q{adv_p[c][j], 0, Fr::zero()});
    }
    const size_t n_adv_q = ev.size() / NC;
    const size_t i_fix = ev.size();
    for (uint32_t f = 0; f < n_fix; f++) ev.push_back(Q{fixed_p[f], 0, Fr::zero()});
    const size_t i_rand = ev.size();
    ev.push_back(Q{rnd, 0, Fr::zero()});
    const size_t i_sig = ev.size();
    for (uint32_t p = 0; p < n_perm; p++) ev.push_back(Q{sigma_p[p], 0, Fr::zero()});
    const size_t i_sig_end = ev.size();
    for (uint32_t c = 0; c < NC; c++) {
        i_z[c] = ev.size();
        for (uint32_t ci = 0; ci < n_chunks; ci++) {
            ev.push_back(Q{z_p[c][ci], 0, Fr::zero()});
            ev.push_back(Q{z_p[c][ci], 1, Fr::zero()});
            if (ci != n_chunks - 1) ev.push_back(Q{z_p[c][ci], last_rot, Fr::zero()});
        }
    }
    for (uint32_t c = 0; c < NC; c++) {
        i_lk[c] = ev.size();
        for (uint32_t l = 0; l < n_lookups; l++) {
            ev.push_back(Q{zl_p[c][l], 0, Fr::zero()});
            ev.push_back(Q{zl_p[c][l], 1, Fr::zero()});
            ev.push_back(Q{ap_p[c][l], 0, Fr::zero()});
            ev.push_back(Q{ap_p[c][l], -1, Fr::zero()});
            ev.push_back(Q{sp_p[c][l], 0, Fr::zero()});
        }
    }
    const size_t n_written = ev.size();
    ev.push_back(Q{h_comb, 0, Fr::zero()});
    {
        std::vector<zk_poly> polys(ev.size());
        std::vector<Fr> pts(ev.size()), vals(ev.size());
        for (size_t i = 0; i < ev.size(); i++) {
            polys[i] = ev[i].poly;
            pts[i] = xrot(x, ev[i].rot);
        }
        CHECK(zk_eval_batch(ctx, polys.data(), reinterpret_cast<const uint64_t*>(pts.data()), ev.size(), reinterpret_cast<uint64_t*>(vals.data())));
        for (size_t i = 0; i < ev.size(); i++) ev[i].eval = vals[i];
    }
    for (size_t i = 0; i < n_written; i++) tr.write_scalar(ev[i].eval);

    // ---- 7. ONE multi-open: for c: circuit c's advice queries, permutation opens, lookup opens; then fixed, sigma, h, random
    std::vector<Q> queries;
    for (uint32_t c = 0; c < NC; c++) {
        for (size_t i = 0; i < n_adv_q; i++) queries.push_back(ev[i_adv[c] + i]);
        std::vector<Q> lastq(n_chunks);
        size_t pos = i_z[c];
        for (uint32_t ci = 0; ci < n_chunks; ci++) {
            queries.push_back(ev[pos++]);
            queries.push_back(ev[pos++]);
            if (ci != n_chunks - 1) lastq[ci] = ev[pos++];
        }
        for (int ci = (int)n_chunks - 2; ci >= 0; ci--) queries.push_back(lastq[ci]);
        pos = i_lk[c];
        for (uint32_t l = 0; l < n_lookups; l++, pos += 5) {
            queries.push_back(ev[pos]);      // zL @ x
            queries.push_back(ev[pos + 2]);  // a' @ x
            queries.push_back(ev[pos + 4]);  // s' @ x
            queries.push_back(ev[pos + 3]);  // a' @ w^-1 x
            queries.push_back(ev[pos + 1]);  // zL @ w x
        }
    }
    for (size_t i = i_fix; i < i_rand; i++) queries.push_back(ev[i]);
    for (size_t i = i_sig; i < i_sig_end; i++) queries.push_back(ev[i]);
    queries.push_back(ev[n_written]);  // h
    queries.push_back(ev[i_rand]);     // the random polynomial
    multi_open(tr, queries, x, n, xrot, shplonk);

    FILE* out = fopen(argv[5], "wb");
    if (!out || fwrite(tr.out.data(), 1, tr.out.size(), out) != tr.out.size()) {
        fprintf(stderr, "%s: cannot write %s\n", prog, argv[5]);
        return 2;
    }
    fclose(out);
    printf("%s: %zu proof bytes over %u circuits\n", prog, tr.out.size(), NC);
    fprintf(stderr, "%s: %zu ABI calls for the proof\n", prog, abi_calls - calls_before);
    zk_pk_free(ctx, pk);
    zk_ctx_destroy(ctx);  // (frees every vector of the context)
    return 0;
}
