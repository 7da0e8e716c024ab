// msm_wide_device_check.hip — runs passes of the wide MSM path (csrc/msm_wide.hip.h behind msm_run / msm_collect) on small columns
// over workspaces and window tables of ANY stride, and writes out every buffer of every pass: the entry layout (ib, fb, bins)
// depends on the workspace's max_n and the table stride, not on the pass's length, so a workspace made for 2^21 points run over a
// few hundred scalars exercises the 2^21 layout.  tests/msm_wide_cases.py makes the cases, tests/msm_wide_model.py states what
// every buffer must hold and documents both file formats; tests/test_gpu_msm_wide_device.py runs this once and compares.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -DZK_MSM_POISON -I webauthn-halo2_amd/csrc tests/msm_wide_device_check.hip
//              -o tests/msm_wide_device_check
// Nothing of the library is linked: msm.hip is included.  ZK_MSM_POISON: msm_run_wide fills slots, parts and row / column sums
// with 0xA5 before every pass, so that an element read without having been written by THIS pass is a wrong value, and the sparse
// dumps below tell exactly which elements the pass wrote.
//
// Per geometry (c, S) one workspace msm_workspace_create(S, c, true, .., max_batch) and one window table of stride S (nwin * S
// points allocated, rows i < m of every window filled from a small table of stride m) are held at a time.  Every HIP call is
// checked: the first error ends the program with status 2 and nothing more is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <vector>

#include "msm.hip"
using namespace zk;

#define CHK(x)                                                                                                           \
    do {                                                                                                                 \
        hipError_t e_ = (x);                                                                                             \
        if (e_ != hipSuccess) {                                                                                          \
            fprintf(stderr, "msm_wide_device_check: HIP error '%s' at line %d: %s\n", hipGetErrorString(e_), __LINE__, #x); \
            exit(2);                                                                                                     \
        }                                                                                                                \
    } while (0)
#define REQUIRE(c, ...)                                             \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "msm_wide_device_check: " __VA_ARGS__); \
            fprintf(stderr, "\n");                                  \
            exit(2);                                                \
        }                                                           \
    } while (0)

constexpr uint32_t MAGIC_IN = 0x43574b5au, MAGIC_OUT = 0x52574b5au;  // "ZKWC", "ZKWR"
enum Tag : uint32_t { T_GEO, T_PASS, T_COUNTS, T_TOTALS, T_BSTART, T_PSTART, T_LANE_B, T_PBUCKET, T_ENTRIES, T_SUMS, T_RESULT, T_SLOTS, T_PARTS, T_RC, T_OTHER };

static FILE* g_out;
static uint32_t g_records;
static void record(uint32_t tag, uint32_t geo, uint32_t pass, uint32_t col, const uint32_t* data, size_t words) {
    REQUIRE(words < (1u << 30), "record too long");
    const uint32_t h[5] = {tag, geo, pass, col, (uint32_t)words};
    REQUIRE(fwrite(h, 4, 5, g_out) == 5 && (words == 0 || fwrite(data, 4, words, g_out) == words), "short write");
    g_records++;
}

static std::vector<uint32_t> download(const void* dev, size_t words) {
    std::vector<uint32_t> h(words);
    if (words) CHK(hipMemcpy(h.data(), dev, words * 4, hipMemcpyDeviceToHost));
    return h;
}

// the elements of dev[0 .. count) whose 144 bytes are not all poison, as (index, 36 words)
static std::vector<uint32_t> sparse_points(const G1X29S* dev, size_t count) {
    const std::vector<uint32_t> h = download(dev, count * 36);
    std::vector<uint32_t> out;
    for (size_t i = 0; i < count; i++) {
        bool poison = true;
        for (int k = 0; k < 36 && poison; k++) poison = h[i * 36 + k] == 0xA5A5A5A5u;
        if (poison) continue;
        out.push_back((uint32_t)i);
        out.insert(out.end(), h.begin() + i * 36, h.begin() + (i + 1) * 36);
    }
    return out;
}

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
    REQUIRE(fsize >= 12 && fsize % 4 == 0, "%s: bad length", argv[1]);
    std::vector<uint32_t> file((size_t)fsize / 4);
    REQUIRE(fread(file.data(), 4, file.size(), f) == file.size(), "%s: short read", argv[1]);
    fclose(f);
    REQUIRE(file[0] == MAGIC_IN && file[1] >= 1 && file[1] <= 16 && file[2] >= 1 && file[2] <= 16, "%s: bad header", argv[1]);
    const uint32_t n_bases = file[1], n_geos = file[2];
    size_t pos = 3;
    auto take = [&](size_t words) {
        REQUIRE(pos + words <= file.size(), "%s is shorter than its records say", argv[1]);
        const uint32_t* p = file.data() + pos;
        pos += words;
        return p;
    };
    static_assert(sizeof(G1Affine) == 64 && sizeof(Fr) == 32 && sizeof(G1Jac) == 96, "the file formats");

    g_out = fopen(argv[2], "wb");
    REQUIRE(g_out, "cannot create %s", argv[2]);
    uint32_t ohdr[2] = {MAGIC_OUT, 0};
    REQUIRE(fwrite(ohdr, 4, 2, g_out) == 2, "short write");

    hipStream_t st;
    CHK(hipStreamCreate(&st));
    std::vector<G1Affine*> d_bases(n_bases);
    std::vector<uint32_t> m_of(n_bases);
    for (uint32_t b = 0; b < n_bases; b++) {
        const uint32_t m = take(1)[0];
        REQUIRE(m >= 1024 && m <= (1u << 16), "basis %u: %u points", b, m);
        m_of[b] = m;
        const uint32_t* p = take((size_t)m * 16);
        CHK(hipMalloc(&d_bases[b], (size_t)m * sizeof(G1Affine)));
        CHK(hipMemcpy(d_bases[b], p, (size_t)m * sizeof(G1Affine), hipMemcpyHostToDevice));
    }
    uint32_t *d_word, *h_word;
    CHK(hipMalloc(&d_word, 4));
    CHK(hipHostMalloc(&h_word, 4));

    for (uint32_t gi = 0; gi < n_geos; gi++) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t* gh = take(4);
        const uint32_t c = gh[0], S = gh[1], max_batch = gh[2], n_passes = gh[3];
        REQUIRE(c >= 15 && c <= 17 && S >= 1024 && S <= (1u << 21) && (S & (S - 1)) == 0 && msm_wide_applies(c, S), "geometry %u: (%u, %u)", gi, c, S);
        REQUIRE(max_batch >= 1 && max_batch <= 3 && n_passes >= 1 && n_passes <= 256, "geometry %u: passes", gi);
        const uint32_t nwin = nwin_for(c), nb = 1u << (c - 1);
        hipError_t e;
        MsmWorkspace* ws = msm_workspace_create(S, c, true, &e, max_batch);
        CHK(e);
        REQUIRE(ws && ws->wide, "geometry %u: no wide workspace", gi);
        const MsmWsLayout L = msm_ws_layout(MSM_PLAN_WIDE, c, S, max_batch, sizeof(G1X29S), sizeof(G1X));
        uint64_t bytes = 0;
        for (uint32_t id = 0; id < WS_NBUF; id++) bytes += (uint64_t)L.buf[id].count * L.buf[id].elem;
        G1Affine* table;
        const size_t table_bytes = (size_t)nwin * S * sizeof(G1Affine);
        CHK(hipMalloc(&table, table_bytes));
        bytes += table_bytes;
        G1X* host_sums;
        CHK(hipHostMalloc(&host_sums, ((size_t)max_batch * WIDE_SUMS + 1) * sizeof(G1X)));
        Fr* d_cols;
        CHK(hipMalloc(&d_cols, (size_t)max_batch * S * sizeof(Fr)));
        bytes += (size_t)max_batch * S * sizeof(Fr);
        const MsmWorkspace::Wide& W = ws->w;
        const uint32_t gw[11] = {(uint32_t)bytes, (uint32_t)(bytes >> 32), W.geo.ib, W.geo.fb, W.geo.bins, W.rows, W.row_bits,
                                 W.lane_stride, W.slot_stride, W.part_stride, WL};
        uint32_t table_basis = 0xffffffffu;

        for (uint32_t pi = 0; pi < n_passes; pi++) {
            const uint32_t* ph = take(5);
            const uint32_t basis = ph[0], n = ph[1], batch = ph[2], ident = ph[3], t1_mode = ph[4];
            REQUIRE(basis < n_bases && n <= m_of[basis] && n <= S && batch >= 1 && batch <= max_batch && ident <= 2 && t1_mode <= 2,
                    "geometry %u pass %u: header", gi, pi);
            const uint32_t m = m_of[basis];
            if (basis != table_basis) {
                // rows i < m of every window, from a small table of stride m (internal form: (c, m) has the wide shape)
                REQUIRE(msm_table_is_internal(c, m) && m <= S, "geometry %u: basis %u has no wide table", gi, basis);
                G1Affine* small;
                CHK(hipMalloc(&small, (size_t)nwin * m * sizeof(G1Affine)));
                CHK(msm_build_table(d_bases[basis], m, c, small, st));
                for (uint32_t w = 0; w < nwin; w++)  // (a row at a time: the rows lie up to 128 MiB apart)
                    CHK(hipMemcpyAsync(table + (size_t)w * S, small + (size_t)w * m, (size_t)m * sizeof(G1Affine), hipMemcpyDeviceToDevice, st));
                CHK(hipStreamSynchronize(st));
                CHK(hipFree(small));
                table_basis = basis;
            }
            const uint32_t* sc = take((size_t)batch * n * 8);
            const Fr* cols[3] = {nullptr, nullptr, nullptr};
            for (uint32_t q = 0; q < batch; q++) {
                cols[q] = d_cols + (size_t)q * S;
                if (n) CHK(hipMemcpy(d_cols + (size_t)q * S, sc + (size_t)q * n * 8, (size_t)n * sizeof(Fr), hipMemcpyHostToDevice));
            }
            bool may = ident == 1;
            if (ident == 2) CHK(msm_bases_have_identity(d_bases[basis], m, st, d_word, h_word, &may));
            msm_ws_set_t1_mode(ws, t1_mode);
            const uint32_t par = W.par;  // the counter set this pass counts in
            MsmPassArgs a = {};
            a.columns = cols;
            a.batch = batch;
            a.n = n;
            a.table = table;
            a.table_stride = S;
            a.head = a.tail = st;
            a.bases_may_be_identity = may;
            a.host_sums = host_sums;
            MsmPass pass;
            CHK(msm_run(ws, a, &pass));
            CHK(hipStreamSynchronize(st));
            uint32_t listed = 0;
            if (pass.redo_word) memcpy(&listed, host_sums + (size_t)batch * WIDE_SUMS, 4);
            G1Jac res[3];
            bool redone = false;
            CHK(msm_collect(ws, pass, st, host_sums, res, &redone));
            CHK(hipDeviceSynchronize());
            const std::vector<uint32_t> counts = download(ws->counts, 4 * (MSM_MAX_BATCH + 1));
            const uint32_t pw[9] = {n, batch, may ? 1u : 0u, t1_mode, listed, redone ? 1u : 0u, counts[1], W.par, wcap_for(batch)};
            record(T_PASS, gi, pi, 0, pw, 9);
            for (uint32_t q = 0; q < batch; q++) {
                record(T_SUMS, gi, pi, q, (const uint32_t*)(host_sums + (size_t)q * WIDE_SUMS), WIDE_SUMS * 32);
                record(T_RESULT, gi, pi, q, (const uint32_t*)&res[q], 24);
                if (n == 0) continue;
                const uint32_t ents = counts[4 * q], nparts = counts[4 * q + 2], lanes = (ents + WL - 1) / WL;
                REQUIRE(ents <= (uint64_t)n * nwin && nparts <= W.part_stride, "geometry %u pass %u column %u: counts %u, %u", gi, pi, q, ents, nparts);
                record(T_COUNTS, gi, pi, q, &counts[4 * q], 3);
                record(T_TOTALS, gi, pi, q, download(W.tot[par] + (size_t)q * nb, nb).data(), nb);
                record(T_BSTART, gi, pi, q, download(W.bstart + (size_t)q * nb, nb).data(), nb);
                record(T_PSTART, gi, pi, q, download(W.pstart + (size_t)q * nb, nb).data(), nb);
                record(T_LANE_B, gi, pi, q, download(W.lane_b + (size_t)q * W.lane_stride, lanes).data(), lanes);
                record(T_PBUCKET, gi, pi, q, download(W.pbucket + (size_t)q * W.part_stride, nparts).data(), nparts);
                record(T_ENTRIES, gi, pi, q, download(ws->entries + (size_t)q * W.ent_stride, ents).data(), ents);
                const std::vector<uint32_t> s = sparse_points(ws->slot_pt + (size_t)q * W.slot_stride, (size_t)wide_lanes(nwin, n) + nb + 64);
                record(T_SLOTS, gi, pi, q, s.data(), s.size());
                const std::vector<uint32_t> p = sparse_points(W.part + (size_t)q * W.part_stride, nparts);
                record(T_PARTS, gi, pi, q, p.data(), p.size());
                const std::vector<uint32_t> r = sparse_points(W.rc + (size_t)q * (W.rows + 256), W.rows + 256);
                record(T_RC, gi, pi, q, r.data(), r.size());
            }
            // the set the NEXT pass counts in and the coarse append cursors: (kind << 28 | index, value) of every non-zero word
            std::vector<uint32_t> other;
            const std::vector<uint32_t> ot = download(W.tot[W.par], (size_t)max_batch * nb), oc = download(W.cur[W.par], (size_t)max_batch * nb);
            for (uint32_t i = 0; i < max_batch * nb; i++) {
                if (ot[i]) other.push_back(i), other.push_back(ot[i]);
                if (oc[i]) other.push_back((1u << 28) | i), other.push_back(oc[i]);
            }
            const std::vector<uint32_t> co = download(ws->coarse, (size_t)max_batch * ws->coarse_stride);
            for (uint32_t q = 0; q < max_batch; q++)
                for (uint32_t b = 0; b < WCB; b++) {
                    const uint32_t v = co[(size_t)q * ws->coarse_stride + WCUR0 + b * WCUR];
                    if (v) other.push_back((2u << 28) | (q * WCB + b)), other.push_back(v);
                }
            record(T_OTHER, gi, pi, 0, other.data(), other.size());
        }
        CHK(hipFree(d_cols));
        CHK(hipHostFree(host_sums));
        CHK(hipFree(table));
        msm_workspace_destroy(ws);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        uint32_t gw2[12];
        memcpy(gw2, gw, sizeof(gw));
        gw2[11] = (uint32_t)ms;
        record(T_GEO, gi, 0, 0, gw2, 12);
        printf("geometry (%u, 2^%u): %u passes, %.3f GB allocated, %.0f ms\n", c, (uint32_t)__builtin_ctz(S), n_passes, bytes / 1e9, ms);
    }
    REQUIRE(pos == file.size(), "%s: %zu trailing words", argv[1], file.size() - pos);
    for (uint32_t b = 0; b < n_bases; b++) CHK(hipFree(d_bases[b]));
    CHK(hipFree(d_word));
    CHK(hipHostFree(h_word));
    CHK(hipStreamDestroy(st));
    ohdr[1] = g_records;
    REQUIRE(fseek(g_out, 0, SEEK_SET) == 0 && fwrite(ohdr, 4, 2, g_out) == 2 && fclose(g_out) == 0, "short write to %s", argv[2]);
    printf("msm_wide_device_check: %u geometries, %u records\n", n_geos, g_records);
    return 0;
}
