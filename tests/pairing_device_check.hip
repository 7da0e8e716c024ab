// pairing_device_check.hip — runs csrc/pairing.h's tower, Frobenius map, line product, Miller loop, final exponentiation and
// whole check on the device over the cases of tests/pairing_device_cases.py, one case per lane, and writes the raw result words
// to a file.  tests/test_gpu_pairing_device.py writes the cases, runs this once as a child process and compares with the Python
// integers of tests/pairing_ref.py.  The per-case code is tests/pairing_check_ops.h; `--host` runs the same code over the same
// cases on the CPU and opens no device (tests/test_pairing_device_cases.py).
//
// Build (build.sh): hipcc <the library's FLAGS> -I webauthn-halo2_amd/csrc tests/pairing_device_check.hip -o tests/pairing_device_check
// Nothing of the library is linked.
//
//   pairing_device_check [--host] <cases.bin> <results.bin> <tables.bin>
//
// Case file (32-bit little-endian words): MAGIC_IN, n, REC_WORDS, n_tables; n records sorted by op; n words: the order of the
// second pass (a permutation of 0 .. n - 1); n_tables x 64 words: the raw images of g2 then s_g2 (all zero: the identity).  The
// tables are made here by pairing_table_make, as pairing.hip makes them, and uploaded; tables.bin gets their bytes: MAGIC_TAB,
// n_tables, words per table, 0, then the tables.
// Kernel shape: the product kernel's — __launch_bounds__(64), workgroups of one wave, lanes beyond n return before touching
// memory.  Pass 1 takes the cases in file order, so every wave is uniform in op; pass 2 takes them in the given order, which
// puts different ops into consecutive lanes: the __noinline__ products then run under partial exec masks.  Either way the result
// of case i lands at record i.  Result file: MAGIC_OUT, n, OUT_WORDS, passes (2; 1 under --host), then passes x n x OUT_WORDS
// words.  Word OUT_WORDS - 1 of a result is DONE | op: a lane that did not run leaves 0xffffffff.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pairing_check_ops.h"
using namespace pairingcheck;

#define CHK(x)                                                                                                               \
    do {                                                                                                                     \
        hipError_t e_ = (x);                                                                                                 \
        if (e_ != hipSuccess) {                                                                                              \
            fprintf(stderr, "pairing_device_check: HIP error '%s' at line %d: %s\n", hipGetErrorString(e_), __LINE__, #x);   \
            exit(2);                                                                                                         \
        }                                                                                                                    \
    } while (0)

constexpr uint32_t WG = 64;  // one wave

__global__ __launch_bounds__(WG) void run_kernel(const uint32_t* __restrict__ recs, const uint32_t* __restrict__ order, uint32_t n,
                                                 const PairingTable* __restrict__ tables, uint32_t* __restrict__ out) {
    const uint32_t j = blockIdx.x * WG + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = order[j];  // (a permutation of 0 .. n - 1: main checks it)
    run_case(recs + (size_t)i * REC_WORDS, tables, out + (size_t)i * OUT_WORDS);
}

static int fail(const char* why) {
    fprintf(stderr, "pairing_device_check: %s\n", why);
    return 2;
}

int main(int argc, char** argv) {
    const bool host = argc == 5 && strcmp(argv[1], "--host") == 0;
    if (!(argc == 4 || host)) return fail("usage: pairing_device_check [--host] cases.bin results.bin tables.bin");
    argv += host ? 1 : 0;
    FILE* f = fopen(argv[1], "rb");
    uint32_t head[4];
    if (!f || fread(head, 4, 4, f) != 4 || head[0] != MAGIC_IN || head[2] != REC_WORDS || head[1] == 0 || head[1] > (1u << 20) || head[3] == 0 ||
        head[3] > MAX_TABLES)
        return fail("cannot read the case file");
    const uint32_t n = head[1], n_tables = head[3];
    std::vector<uint32_t> recs((size_t)n * REC_WORDS), order(n), raw((size_t)n_tables * 64);
    if (fread(recs.data(), 4, recs.size(), f) != recs.size() || fread(order.data(), 4, n, f) != n || fread(raw.data(), 4, raw.size(), f) != raw.size())
        return fail("the case file is short");
    fclose(f);
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t j = 0; j < n; j++) {
        if (order[j] >= n || seen[order[j]]) return fail("the second pass's order is not a permutation");
        seen[order[j]] = 1;
        if (!record_in_bounds(recs.data() + (size_t)j * REC_WORDS, n_tables)) return fail("a record names a table or a step that is not there");
    }
    std::vector<PairingTable> tables(n_tables);
    for (uint32_t k = 0; k < n_tables; k++) {
        const uint8_t* p = (const uint8_t*)(raw.data() + (size_t)k * 64);
        pairing_table_make(g2_from_raw(p), g2_from_raw(p + 128), &tables[k]);
    }
    static_assert(sizeof(PairingTable) % 4 == 0, "a table is whole words");
    const uint32_t thead[4] = {MAGIC_TAB, n_tables, (uint32_t)(sizeof(PairingTable) / 4), 0};
    FILE* g = fopen(argv[3], "wb");
    if (!g || fwrite(thead, 4, 4, g) != 4 || fwrite((const void*)tables.data(), sizeof(PairingTable), n_tables, g) != n_tables || fclose(g))
        return fail("cannot write the table file");

    const uint32_t passes = host ? 1 : 2;
    const size_t out_words = (size_t)n * OUT_WORDS;
    std::vector<uint32_t> out(passes * out_words, 0xffffffffu);
    if (host) {
        for (uint32_t i = 0; i < n; i++) run_case(recs.data() + (size_t)i * REC_WORDS, tables.data(), out.data() + (size_t)i * OUT_WORDS);
    } else {
        uint32_t *d_recs = nullptr, *d_order = nullptr, *d_out = nullptr;
        PairingTable* d_tables = nullptr;
        std::vector<uint32_t> ident(n);
        for (uint32_t i = 0; i < n; i++) ident[i] = i;
        CHK(hipMalloc(&d_recs, recs.size() * 4));
        CHK(hipMalloc(&d_order, (size_t)n * 4));
        CHK(hipMalloc(&d_out, out_words * 4));
        CHK(hipMalloc(&d_tables, sizeof(PairingTable) * n_tables));
        CHK(hipMemcpy(d_recs, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
        CHK(hipMemcpy(d_tables, (const void*)tables.data(), sizeof(PairingTable) * n_tables, hipMemcpyHostToDevice));
        for (uint32_t pass = 0; pass < 2; pass++) {
            CHK(hipMemcpy(d_order, pass ? order.data() : ident.data(), (size_t)n * 4, hipMemcpyHostToDevice));
            CHK(hipMemset(d_out, 0xff, out_words * 4));
            hipLaunchKernelGGL(run_kernel, dim3((n + WG - 1) / WG), dim3(WG), 0, 0, d_recs, d_order, n, d_tables, d_out);
            CHK(hipGetLastError());
            CHK(hipDeviceSynchronize());
            CHK(hipMemcpy(out.data() + pass * out_words, d_out, out_words * 4, hipMemcpyDeviceToHost));
        }
        CHK(hipFree(d_recs));
        CHK(hipFree(d_order));
        CHK(hipFree(d_out));
        CHK(hipFree(d_tables));
    }
    const uint32_t ohead[4] = {MAGIC_OUT, n, OUT_WORDS, passes};
    g = fopen(argv[2], "wb");
    if (!g || fwrite(ohead, 4, 4, g) != 4 || fwrite(out.data(), 4, out.size(), g) != out.size() || fclose(g)) return fail("cannot write the result file");
    printf("pairing_device_check: %u cases, %u tables, %s\n", n, n_tables, host ? "on the host" : "grouped and interleaved passes of one-wave workgroups");
    return 0;
}
