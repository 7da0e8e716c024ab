// quotient_device_check.hip — runs the eight instantiations of csrc/quotient.hip (quotient_kernel and quotient_sliced_kernel, whole
// extended domain or three cosets, storing or accumulating) on operand vectors read from a file and writes every output row, with
// the guards around `out`, to a file.  tests/quotient_cases.py makes the cases and their expected rows and documents both file
// formats; tests/test_gpu_quotient_device.py runs this once and compares.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I webauthn-halo2_amd/csrc tests/quotient_device_check.hip -o tests/quotient_device_check
// Nothing of the library is linked: quotient.hip is included, and only its two launchers are called — with any log_slices and
// cosets3, which the product never chooses freely (quotient_log_slices decides there).
//
// Per launch every vector of the data set lies in one arena, back to back, each with exactly as many rows as the launch (2^log_ext,
// or 3 * 2^(log_ext - 2) coset-major for three cosets; the coset points keep their 4n table, as in the product), then 256 rows of
// canary, `out`, and 256 rows of canary.  The QuotientArgs block is filled here from the data set's canonical challenges, the way
// pk_quotient_pass fills it: beta, gamma, delta times 32 in the Montgomery form, ypow[j] = 32 y^(T-1-j), delta_chunk[c] = 32
// delta^(c chunk_len), t_inv in the standard form (all one without the division).
//
// Standard output: quotient_log_slices(log_ext, n_gate) for log_ext 8 .. 26, n_gate 1 .. 352, one line "ls <log_ext> <352 digits>" each.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "quotient.hip"
#include "hostutil.h"
using namespace zk;

#define CHK(x)                                                                                      \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "quotient_device_check: HIP error '%s' at line %d: %s\n", hipGetErrorString(e_), __LINE__, #x); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)
#define REQUIRE(c, ...)                                        \
    do {                                                       \
        if (!(c)) {                                            \
            fprintf(stderr, "quotient_device_check: " __VA_ARGS__); \
            fprintf(stderr, "\n");                             \
            exit(2);                                           \
        }                                                      \
    } while (0)

constexpr uint32_t MAGIC_IN = 0x43514b5au, MAGIC_OUT = 0x52514b5au;  // "ZKQC", "ZKQR"
constexpr uint32_t GUARD_ROWS = 256, CANARY = 0xc0defaceu;

struct VecRec {
    uint32_t kind;            // 1: rows alternate e0, e1;  0: explicit
    uint32_t e[2][8];
    const uint32_t* data;     // explicit rows on the 4n coset
};

static Fr fr_of_canonical(const uint32_t* w) {
    Fr a;
    for (int i = 0; i < 8; i++) a.v[i] = w[i];
    return fe_to_mont(a);
}

// row `i` (4n coset) of a vector
static inline const uint32_t* row_of(const VecRec& v, uint32_t i) { return v.kind ? v.e[i & 1] : v.data + (size_t)i * 8; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    REQUIRE(f, "cannot open %s", argv[1]);
    fseek(f, 0, SEEK_END);
    const long fsize = ftell(f);
    fseek(f, 0, SEEK_SET);
    REQUIRE(fsize >= 8 && fsize % 4 == 0, "%s: bad length", argv[1]);
    std::vector<uint32_t> file((size_t)fsize / 4);
    REQUIRE(fread(file.data(), 4, file.size(), f) == file.size(), "%s: short read", argv[1]);
    fclose(f);
    REQUIRE(file[0] == MAGIC_IN && file[1] >= 1 && file[1] < 4096, "%s: bad header", argv[1]);
    const uint32_t n_sets = file[1];
    size_t pos = 2;
    auto take = [&](size_t words) {
        REQUIRE(pos + words <= file.size(), "%s is shorter than its records say", argv[1]);
        const uint32_t* p = file.data() + pos;
        pos += words;
        return p;
    };

    for (uint32_t le = 8; le <= 26; le++) {
        printf("ls %u ", le);
        for (uint32_t g = 1; g <= MAX_ADV; g++) printf("%u", quotient_log_slices(le, g));
        printf("\n");
    }

    FILE* g = fopen(argv[2], "wb");
    REQUIRE(g, "cannot create %s", argv[2]);
    uint32_t ohdr[2] = {MAGIC_OUT, 0};
    REQUIRE(fwrite(ohdr, 4, 2, g) == 2, "short write");

    QuotientArgs* h_q = new QuotientArgs;
    QuotientArgs* d_q;
    CHK(hipMalloc(&d_q, sizeof(QuotientArgs)));
    const Fr k32 = fr_from_u64(32);
    const Fr delta = fe_pow_u64(fr_from_u64(7), 1ull << 28);  // the permutation argument's coset generator
    uint32_t total_launches = 0;
    std::vector<uint32_t> host_arena, region;

    for (uint32_t si = 0; si < n_sets; si++) {
        const uint32_t* h = take(16);
        const uint32_t log_ext = h[0], n_gate = h[1], n_adv = h[2], n_fix = h[3], n_perm = h[4], n_chunks = h[5], chunk_len = h[6],
                       n_lookups = h[7], single = h[8], fx_table = h[10], fx_qlookup = h[11], has_inst = h[12], n_vec = h[13],
                       n_launches = h[14], n_explicit = h[15];
        const int32_t last_rot = (int32_t)h[9];
        // everything the kernels index with is checked here: no launch can leave its arena
        REQUIRE(log_ext >= 8 && log_ext <= 10, "data set %u: log_ext %u", si, log_ext);
        REQUIRE(n_gate >= 1 && n_gate <= n_adv && n_adv <= MAX_ADV && n_fix >= 1 && n_fix <= MAX_FIX && n_perm >= 1 && n_perm <= MAX_PERM,
                "data set %u: column counts", si);
        REQUIRE(n_chunks >= 1 && n_chunks <= MAX_CHUNKS && chunk_len >= 1 && (uint64_t)n_chunks * chunk_len >= n_perm &&
                    (uint64_t)(n_chunks - 1) * chunk_len < n_perm, "data set %u: chunks", si);
        REQUIRE(n_lookups >= 1 && n_lookups <= MAX_LOOKUPS && single <= 1 && has_inst <= 1 && fx_table < n_fix && fx_qlookup < n_fix,
                "data set %u: lookups", si);
        REQUIRE(single ? n_adv == n_gate : n_adv == n_gate + n_lookups, "data set %u: lookup columns", si);
        const uint32_t n_terms = quotient_terms(n_gate, n_chunks, n_lookups);
        REQUIRE(n_terms <= MAX_TERMS, "data set %u: %u terms", si, n_terms);
        const uint32_t want_vec = n_adv + n_fix + n_perm + n_chunks + 3 * n_lookups + has_inst + 5;
        REQUIRE(n_vec == want_vec && n_explicit <= n_vec && n_launches >= 1 && n_launches <= 256, "data set %u: vector count", si);
        const uint32_t N = 1u << log_ext, n = N >> 2;
        const uint32_t* fx_sel = take(n_gate);
        for (uint32_t j = 0; j < n_gate; j++)
            REQUIRE((fx_sel[j] & 0xffffffu) < n_fix && (fx_sel[j] >> 24) <= 2, "data set %u: selector of gate %u", si, j);
        const uint32_t* perm_src = take(n_perm);
        for (uint32_t p = 0; p < n_perm; p++) {
            const uint32_t type = perm_src[p] >> 24, idx = perm_src[p] & 0xffffffu;
            REQUIRE(type == 0 ? idx < n_adv : type == 1 ? idx < n_fix : (type == 2 && has_inst && idx == 0), "data set %u: permutation column %u", si, p);
        }
        const uint32_t* chal = take(7 * 8);
        std::vector<VecRec> vecs(n_vec);
        const uint32_t* recs = take((size_t)n_vec * 17);
        uint32_t seen_explicit = 0;
        for (uint32_t v = 0; v < n_vec; v++) {
            vecs[v].kind = recs[17 * v];
            REQUIRE(vecs[v].kind <= 1, "data set %u: vector %u kind", si, v);
            for (int e = 0; e < 2; e++)
                for (int w = 0; w < 8; w++) vecs[v].e[e][w] = recs[17 * v + 1 + 8 * e + w];
            vecs[v].data = nullptr;
            if (!vecs[v].kind) seen_explicit++;
        }
        REQUIRE(seen_explicit == n_explicit, "data set %u: explicit vectors", si);
        for (uint32_t v = 0; v < n_vec; v++)
            if (!vecs[v].kind) vecs[v].data = take((size_t)N * 8);
        const uint32_t* launches = take((size_t)n_launches * 4);

        // vector order: adv fix sigma z lk_z lk_a lk_s [inst] l0 l_last l_active xs prev
        const uint32_t o_adv = 0, o_fix = o_adv + n_adv, o_sigma = o_fix + n_fix, o_z = o_sigma + n_perm, o_lkz = o_z + n_chunks,
                       o_lka = o_lkz + n_lookups, o_lks = o_lka + n_lookups, o_inst = o_lks + n_lookups, o_l0 = o_inst + has_inst,
                       o_xs = o_l0 + 3, o_prev = o_xs + 1;
        const uint32_t n_plain = o_xs;  // vectors laid out with the launch's rows

        memset(h_q, 0, sizeof(*h_q));
        QuotientArgs& q = *h_q;
        q.log_ext = log_ext;
        q.n_gate = n_gate;
        q.n_adv = n_adv;
        q.n_chunks = n_chunks;
        q.chunk_len = chunk_len;
        q.n_perm = n_perm;
        q.n_lookups = n_lookups;
        q.single = single;
        q.last_rot = last_rot;
        q.fx_table = fx_table;
        q.fx_qlookup = fx_qlookup;
        for (uint32_t j = 0; j < n_gate; j++) q.fx_sel[j] = fx_sel[j];
        const Fr beta = fr_of_canonical(chal), gamma = fr_of_canonical(chal + 8), y = fr_of_canonical(chal + 16);
        q.beta = fe_mul(beta, k32);
        q.gamma = fe_mul(gamma, k32);
        q.delta = fe_mul(delta, k32);
        q.n_terms = n_terms;
        Fr yp = k32;
        for (uint32_t j = n_terms; j-- > 0;) {
            q.ypow[j] = yp;
            yp = fe_mul(yp, y);
        }
        const Fr dstep = fe_pow_u64(delta, chunk_len);
        Fr dc = k32;
        for (uint32_t c = 0; c < n_chunks; c++) {
            q.delta_chunk[c] = dc;
            dc = fe_mul(dc, dstep);
        }

        for (uint32_t c3 = 0; c3 < 2; c3++) {
            bool used = false;
            for (uint32_t l = 0; l < n_launches; l++) used |= launches[4 * l + 1] == c3;
            if (!used) continue;
            const uint32_t rows = c3 ? 3 * n : N;
            // arena: the plain vectors, the coset points (4n table), guard, out, guard
            const size_t xs_at = (size_t)n_plain * rows, guard_at = xs_at + N, out_at = guard_at + GUARD_ROWS,
                         arena_rows = out_at + rows + GUARD_ROWS;
            host_arena.assign(arena_rows * 8, 0);
            auto src_row = [&](uint32_t i) { return c3 ? 4 * (i % n) + i / n : i; };  // coset-major row j n + r is the point 4 r + j
            for (uint32_t v = 0; v < n_plain; v++)
                for (uint32_t i = 0; i < rows; i++) memcpy(&host_arena[((size_t)v * rows + i) * 8], row_of(vecs[v], src_row(i)), 32);
            for (uint32_t i = 0; i < N; i++) memcpy(&host_arena[(xs_at + i) * 8], row_of(vecs[o_xs], i), 32);
            Fr* d_arena;
            CHK(hipMalloc(&d_arena, arena_rows * 32));
            CHK(hipMemcpy(d_arena, host_arena.data(), arena_rows * 32, hipMemcpyHostToDevice));
            auto at = [&](uint32_t v) { return d_arena + (size_t)v * rows; };
            for (uint32_t j = 0; j < n_adv; j++) q.adv[j] = at(o_adv + j);
            for (uint32_t j = 0; j < n_fix; j++) q.fix[j] = at(o_fix + j);
            for (uint32_t p = 0; p < n_perm; p++) {
                const uint32_t type = perm_src[p] >> 24, idx = perm_src[p] & 0xffffffu;
                q.sigma[p] = at(o_sigma + p);
                q.perm_val[p] = type == 1 ? q.fix[idx] : type == 2 ? at(o_inst) : q.adv[idx];
            }
            for (uint32_t c = 0; c < n_chunks; c++) q.z[c] = at(o_z + c);
            for (uint32_t l = 0; l < n_lookups; l++) {
                q.lk_z[l] = at(o_lkz + l);
                q.lk_a[l] = at(o_lka + l);
                q.lk_s[l] = at(o_lks + l);
                q.lk_in[l] = single ? nullptr : q.adv[n_gate + l];
            }
            q.l0 = at(o_l0);
            q.l_last = at(o_l0 + 1);
            q.l_active = at(o_l0 + 2);
            q.xs = d_arena + xs_at;
            q.out = d_arena + out_at;

            const size_t region_rows = rows + 2 * GUARD_ROWS;
            for (uint32_t l = 0; l < n_launches; l++) {
                const uint32_t acc = launches[4 * l], lc3 = launches[4 * l + 1], divide = launches[4 * l + 2], log_slices = launches[4 * l + 3];
                if (lc3 != c3) continue;
                REQUIRE(acc <= 1 && divide <= 1 && log_slices <= 4 && (1u << log_slices) <= n_gate, "data set %u: launch %u", si, l);
                for (int j = 0; j < 4; j++) q.t_inv[j] = divide ? fr_of_canonical(chal + 24 + 8 * j) : Fr::one();
                q.divide = divide;
                // out: what an accumulating pass finds there; canary for a storing pass, so that a row never written shows
                region.assign(region_rows * 8, CANARY);
                if (acc)
                    for (uint32_t i = 0; i < rows; i++) memcpy(&region[((size_t)GUARD_ROWS + i) * 8], row_of(vecs[o_prev], src_row(i)), 32);
                CHK(hipMemcpy(d_arena + guard_at, region.data(), region_rows * 32, hipMemcpyHostToDevice));
                CHK(hipMemcpy(d_q, h_q, sizeof(QuotientArgs), hipMemcpyHostToDevice));
                if (acc) launch_quotient_acc_dev(d_q, log_ext, log_slices, 0, c3 != 0);
                else launch_quotient_dev(d_q, log_ext, log_slices, 0, c3 != 0);
                CHK(hipGetLastError());
                CHK(hipDeviceSynchronize());
                CHK(hipMemcpy(region.data(), d_arena + guard_at, region_rows * 32, hipMemcpyDeviceToHost));
                // (the records carry their data set and launch numbers: the 4n launches of a data set come before its three-coset ones)
                const uint32_t rh[4] = {si, l, rows, 0};
                REQUIRE(fwrite(rh, 4, 4, g) == 4 && fwrite(region.data(), 4, region.size(), g) == region.size(), "short write to %s", argv[2]);
                total_launches++;
            }
            CHK(hipFree(d_arena));
        }
    }
    REQUIRE(pos == file.size(), "%s: %zu trailing words", argv[1], file.size() - pos);
    ohdr[1] = total_launches;
    REQUIRE(fseek(g, 0, SEEK_SET) == 0 && fwrite(ohdr, 4, 2, g) == 2 && fclose(g) == 0, "short write to %s", argv[2]);
    CHK(hipFree(d_q));
    delete h_q;
    printf("quotient_device_check: %u data sets, %u launches\n", n_sets, total_launches);
    return 0;
}
