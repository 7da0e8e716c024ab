// Host check of csrc/verifier.h for ONE proof over several circuits (zk_verify_multi's host half; tests/test_verify_multi_host.py
// builds and drives it): tests/verify_host_check.cpp's job reader, point decoding, host sums and pairing as they stand, with the
// proof layout taken for the circuit count given on the command line.
//
//   verify_multi_host_check <n_circuits> < job      one verdict per proof line of the job (format: tests/test_verify_host.py)
#include "pairing.h"
#include "verifier.h"

static uint32_t g_circuits = 1;
#define proof_layout(lay, evm, shplonk) proof_layout(lay, evm, shplonk, g_circuits)
#define main verify_host_check_main
#include "verify_host_check.cpp"
#undef main
#undef proof_layout

int main(int argc, char** argv) {
    if (argc < 2 || atoi(argv[1]) < 1) {
        fprintf(stderr, "usage: verify_multi_host_check <n_circuits> < job\n");
        return 2;
    }
    g_circuits = (uint32_t)atoi(argv[1]);
    return run_verify();
}
