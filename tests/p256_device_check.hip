// p256_device_check.hip — runs csrc/p256.hip.h's field, point and x-compare routines on the device over the cases of
// tests/p256_cases.py, one case per lane, and writes the raw result words to a file.  tests/test_gpu_p256_device.py writes the
// cases, runs this once as a child process and compares with Python integers.  The per-case code is tests/p256_check_ops.h, the
// same the CPU harness (tests/p256_host_check.cpp) runs.
//
// Build (build.sh): hipcc --offload-arch=gfx950 -O3 -std=c++17 -I webauthn-halo2_amd/csrc tests/p256_device_check.hip -o tests/p256_device_check
// Nothing of the library is linked.
//
//   p256_device_check <cases.bin> <results.bin>
//
// The records are sorted by (op, modulus), so the lanes of a wave mostly run the same routine.  The whole set is launched twice:
// in blocks of 64 and of 256 lanes, the last block ragged.  Result file: MAGIC_OUT, n, OUT_WORDS, 2, then the n x OUT_WORDS words
// of the 64-lane pass and those of the 256-lane pass.  Word OUT_WORDS - 1 of a result is DONE | op: a lane that did not run
// leaves 0xffffffff.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "p256_check_ops.h"
using namespace p256check;

#define CHK(x)                                                                                                            \
    do {                                                                                                                  \
        hipError_t e_ = (x);                                                                                              \
        if (e_ != hipSuccess) {                                                                                           \
            fprintf(stderr, "p256_device_check: HIP error '%s' at line %d: %s\n", hipGetErrorString(e_), __LINE__, #x);   \
            exit(2);                                                                                                      \
        }                                                                                                                 \
    } while (0)

__global__ void run_kernel(const uint32_t* recs, uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    run_case(recs + (size_t)i * REC_WORDS, out + (size_t)i * OUT_WORDS);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: p256_device_check cases.bin results.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    uint32_t head[4];
    if (!f || fread(head, 4, 4, f) != 4 || head[0] != MAGIC_IN || head[2] != REC_WORDS || head[1] == 0 || head[1] > (1u << 20)) {
        fprintf(stderr, "p256_device_check: cannot read the case file\n");
        return 2;
    }
    const uint32_t n = head[1];
    std::vector<uint32_t> recs((size_t)n * REC_WORDS);
    if (fread(recs.data(), 4, recs.size(), f) != recs.size()) {
        fprintf(stderr, "p256_device_check: the case file is short\n");
        return 2;
    }
    fclose(f);
    uint32_t *d_recs = nullptr, *d_out = nullptr;
    const size_t out_bytes = (size_t)n * OUT_WORDS * 4;
    CHK(hipMalloc(&d_recs, recs.size() * 4));
    CHK(hipMalloc(&d_out, out_bytes));
    CHK(hipMemcpy(d_recs, recs.data(), recs.size() * 4, hipMemcpyHostToDevice));
    std::vector<uint32_t> out((size_t)2 * n * OUT_WORDS);
    const uint32_t blocks[2] = {64, 256};
    for (int pass = 0; pass < 2; pass++) {
        CHK(hipMemset(d_out, 0xff, out_bytes));
        hipLaunchKernelGGL(run_kernel, dim3((n + blocks[pass] - 1) / blocks[pass]), dim3(blocks[pass]), 0, 0, d_recs, n, d_out);
        CHK(hipGetLastError());
        CHK(hipDeviceSynchronize());
        CHK(hipMemcpy(out.data() + (size_t)pass * n * OUT_WORDS, d_out, out_bytes, hipMemcpyDeviceToHost));
    }
    CHK(hipFree(d_recs));
    CHK(hipFree(d_out));
    const uint32_t ohead[4] = {MAGIC_OUT, n, OUT_WORDS, 2};
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(ohead, 4, 4, g) != 4 || fwrite(out.data(), 4, out.size(), g) != out.size() || fclose(g)) {
        fprintf(stderr, "p256_device_check: cannot write the result file\n");
        return 2;
    }
    printf("p256_device_check: %u cases, blocks of 64 and 256 lanes\n", n);
    return 0;
}
