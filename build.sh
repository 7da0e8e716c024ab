#!/bin/bash
# Builds webauthn-halo2_amd/libzkmi355.so for gfx950 (hipcc cross-compiles without a GPU).
set -e
cd "$(dirname "$0")/webauthn-halo2_amd"
OUT=libzkmi355.so
SRCS="csrc/ctx.hip csrc/streams.hip csrc/msm_lanes.hip csrc/srs.hip csrc/poly_abi.hip csrc/ntt.hip csrc/msm.hip csrc/poly.hip csrc/prover_kernels.hip csrc/quotient.hip csrc/prover.hip csrc/prover_key.hip csrc/prover_phases.hip csrc/serde.hip csrc/verify.hip csrc/g1_ntt.hip csrc/witness_check.hip csrc/pk_check.hip csrc/placement.hip csrc/es256.hip csrc/webauthn.hip csrc/webauthn_register.hip csrc/pairing.hip csrc/pairing_each.hip"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result"
mkdir -p build
objs=""
pids=""
for s in $SRCS; do
  o=build/$(basename $s .hip).o
  objs="$objs $o"
  if [ ! -f $o ] || [ $s -nt $o ] || [ -n "$(find csrc ../include -name '*.h' -newer $o)" ]; then
    hipcc $FLAGS -c $s -o $o &
    pids="$pids $!"
  fi
done
# the device harness of the field / curve headers (tests/field_device_check.hip, run by tests/test_gpu_field_device.py): one
# source, one binary per instruction form of the 29-bit product, plus one with the curve's squarings and fused product off
for v in "a0:-DZK_MUL29_ASM=0" "a1:-DZK_MUL29_ASM=1" "a2:-DZK_MUL29_ASM=2" "a2m:-DZK_MUL29_ASM=2 -DZK_MUL29_MASKRUN=1" \
         "a2p:-DZK_MUL29_ASM=2 -DZK_EC29_SQR=0 -DZK_EC29_FUSE=0"; do
  x=../tests/field_device_check_${v%%:*}
  if [ ! -f $x ] || [ ../tests/field_device_check.hip -nt $x ] || [ -n "$(find csrc -name '*.h' -newer $x)" ]; then
    hipcc $FLAGS ${v#*:} -Icsrc ../tests/field_device_check.hip -o $x &
    pids="$pids $!"
  fi
done
# the device harness of csrc/p256.hip.h (tests/p256_device_check.hip, run by tests/test_gpu_p256_device.py): the header has one
# portable form, so one binary
x=../tests/p256_device_check
if [ ! -f $x ] || [ ../tests/p256_device_check.hip -nt $x ] || [ ../tests/p256_check_ops.h -nt $x ] || [ csrc/p256.hip.h -nt $x ]; then
  hipcc $FLAGS -Icsrc ../tests/p256_device_check.hip -o $x &
  pids="$pids $!"
fi
# the device harness of csrc/pairing.h (tests/pairing_device_check.hip, run by tests/test_gpu_pairing_device.py, and on the CPU
# under --host by tests/test_pairing_device_cases.py): one binary, with the library's flags
x=../tests/pairing_device_check
if [ ! -f $x ] || [ ../tests/pairing_device_check.hip -nt $x ] || [ ../tests/pairing_check_ops.h -nt $x ] || [ -n "$(find csrc -name '*.h' -newer $x)" ]; then
  hipcc $FLAGS -Icsrc ../tests/pairing_device_check.hip -o $x &
  pids="$pids $!"
fi
# the device harness of csrc/quotient.hip (tests/quotient_device_check.hip, run by tests/test_gpu_quotient_device.py): the source
# includes quotient.hip itself, so one binary with the library's flags
x=../tests/quotient_device_check
if [ ! -f $x ] || [ ../tests/quotient_device_check.hip -nt $x ] || [ csrc/quotient.hip -nt $x ] || [ -n "$(find csrc ../include -name '*.h' -newer $x)" ]; then
  hipcc $FLAGS -Icsrc ../tests/quotient_device_check.hip -o $x &
  pids="$pids $!"
fi
# the device harness of the wide MSM path (tests/msm_wide_device_check.hip, run by tests/test_gpu_msm_wide_device.py): the source
# includes msm.hip itself; -DZK_MSM_POISON makes a slot, part or row / column sum that a pass reads without writing it a wrong value
x=../tests/msm_wide_device_check
if [ ! -f $x ] || [ ../tests/msm_wide_device_check.hip -nt $x ] || [ csrc/msm.hip -nt $x ] || [ -n "$(find csrc ../include -name '*.h' -newer $x)" ]; then
  hipcc $FLAGS -DZK_MSM_POISON -Icsrc ../tests/msm_wide_device_check.hip -o $x &
  pids="$pids $!"
fi
for p in $pids; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $objs
echo "built $(pwd)/$OUT"
echo "built $(cd ../tests && pwd)/field_device_check_{a0,a1,a2,a2m,a2p}"
echo "built $(cd ../tests && pwd)/p256_device_check"
echo "built $(cd ../tests && pwd)/pairing_device_check"
echo "built $(cd ../tests && pwd)/quotient_device_check"
echo "built $(cd ../tests && pwd)/msm_wide_device_check"
# the C++ host example of the same ABI (examples/prove_host.cpp): plain g++, linked against the library above
cd ..
g++ -O2 -std=c++17 -Wall -Iinclude examples/prove_host.cpp -Lwebauthn-halo2_amd -lzkmi355 -Wl,-rpath,'$ORIGIN/../webauthn-halo2_amd' -o examples/prove_host
echo "built $(pwd)/examples/prove_host"
# the phase-level host (examples/prove_host_phases.cpp): its host-side field / transcript code comes from the engine's host headers,
# which carry HIP's function attributes — hence hipcc; it links against the same library through the public ABI only
hipcc --offload-arch=gfx950 -O2 -std=c++17 -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result -x hip examples/prove_host_phases.cpp -Lwebauthn-halo2_amd -lzkmi355 -Wl,-rpath,'$ORIGIN/../webauthn-halo2_amd' -o examples/prove_host_phases
echo "built $(pwd)/examples/prove_host_phases"
# the phase-level host for N circuits and public inputs (examples/prove_host_phases_multi.cpp; examples/phase_host.h is shared by the two)
hipcc --offload-arch=gfx950 -O2 -std=c++17 -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result -x hip examples/prove_host_phases_multi.cpp -Lwebauthn-halo2_amd -lzkmi355 -Wl,-rpath,'$ORIGIN/../webauthn-halo2_amd' -o examples/prove_host_phases_multi
echo "built $(pwd)/examples/prove_host_phases_multi"
