// placement.hip — the device half of zk_stream_placement: the stamp-and-spin kernel and one probe over a list of streams.
// What the stamps mean, the constants and their derivation: placement.h.  A whole probe of the 40 pool streams on an idle
// MI355X takes 27 - 29 ms (docs/experiments.md "stream placement probe").
#include <hip/hip_runtime.h>

#include <chrono>

#include "placement.h"

namespace zk {

// ONE workgroup; lane 0 stamps the constant 100 MHz counter (s_memrealtime, the one clock_probe_kernel reads) at entry, waits
// until it has advanced by `ticks` and stamps it again.  The wait sleeps between reads (it needs no issue slots of the chip) and
// is bounded twice: by the counter, and by an iteration count that a spin of this length cannot reach (a counter that stood
// still would otherwise hold the queue for ever).
__global__ __launch_bounds__(64) void stamp_spin_kernel(uint64_t ticks, placement::Stamp* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const uint64_t t0 = wall_clock64();
    out->t0 = t0;
    uint64_t t1 = t0;
    for (uint32_t it = 0; it < (1u << 22) && t1 - t0 < ticks; it++) {
        __builtin_amdgcn_s_sleep(8);
        t1 = wall_clock64();
    }
    out->t1 = t1;
}

// classes of streams[0 .. n) of the current device.  `stamps`: pinned host memory for MAX_STREAMS stamps, the caller's.  Nothing
// else may be running on these streams.
placement::Classes placement_probe(const hipStream_t* streams, int n, placement::Stamp* stamps) {
    using namespace placement;
    if (n < 1 || n > MAX_STREAMS) return classify(0, [](int, const uint8_t*, Stamp*) { return -1; });
    // warm-up: the first launch of a kernel loads its code, the first use of a stream may set its queue up
    bool ok = true;
    for (int i = 0; i < n; i++) hipLaunchKernelGGL(stamp_spin_kernel, dim3(1), dim3(64), 0, streams[i], (uint64_t)0, stamps + i);
    ok = hipGetLastError() == hipSuccess;
    for (int i = 0; i < n; i++) ok = hipStreamSynchronize(streams[i]) == hipSuccess && ok;
    if (!ok) return classify(n, [](int, const uint8_t*, Stamp*) { return -1; });
    const uint64_t tp = t_pivot(n);
    const int64_t budget_ns = (int64_t)(enqueue_budget(n) * 1000 / TICKS_PER_US);
    return classify(n, [&](int pivot, const uint8_t* active, Stamp* st) -> int {
        memset(stamps, 0, MAX_STREAMS * sizeof(Stamp));
        const auto h0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(stamp_spin_kernel, dim3(1), dim3(64), 0, streams[pivot], tp, stamps + pivot);
        for (int i = 0; i < n; i++)
            if (active[i] && i != pivot) hipLaunchKernelGGL(stamp_spin_kernel, dim3(1), dim3(64), 0, streams[i], T_SHORT, stamps + i);
        const auto h1 = std::chrono::steady_clock::now();
        bool good = hipGetLastError() == hipSuccess;
        for (int i = 0; i < n; i++)
            if (active[i]) good = hipStreamSynchronize(streams[i]) == hipSuccess && good;
        if (!good) return -1;
        memcpy(st, stamps, (size_t)n * sizeof(Stamp));
        return std::chrono::duration_cast<std::chrono::nanoseconds>(h1 - h0).count() > budget_ns ? 1 : 0;
    });
}

}  // namespace zk
