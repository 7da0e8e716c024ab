// engine.h — internal declarations shared by the HIP translation units of
// libzkmi355.so (not part of the public C-ABI; that is include/zkmi355.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ec.hip.h"
#include "field.hip.h"
#include "msm_plan.h"  // MSM_MAX_BATCH, msm_auto_window, msm_auto_window_generic: the plan rules, host only

namespace zk {

// ---- NTT (ntt.hip) ---------------------------------------------------------
static constexpr uint32_t NTT_MAX_BATCH = 96;  // vectors transformed by one launch (grid.y): 32 columns x the three cosets of poly.hip "three cosets"
struct NttJob {
    const Fr* src;      // n_in elements (rest of the 2^log_n vector is zero)
    Fr* dst;            // 2^log_n elements (n_out stored)
    Fr* tmp;            // 2^log_n scratch per vector (required when more than one pass, or src == dst)
    // batch > 1: the same transform over srcs[b] -> dsts[b] (src / dst unused); tmp holds batch x 2^log_n
    uint32_t batch;
    const Fr* srcs[NTT_MAX_BATCH];
    Fr* dsts[NTT_MAX_BATCH];
    const Fr* tw;       // twiddle table in the NTT's internal form: w^i * 2^261 mod p, i < 2^log_n (launch_twiddles_internal)
    // optional: c * w^i in the STANDARD form (c = 1, or post[0] when tw_last_has_post): lets the last pass of a multi-pass
    // transform fold the final conversion (and a uniform output scaling) into its inter-pass twiddles (ntt.hip NTT_FOLD)
    const Fr* tw_last;
    uint32_t tw_last_has_post;
    uint32_t log_n;
    uint32_t inverse;   // use w^-1
    uint32_t n_in, n_out;
    uint32_t has_pre, has_post;
    Fr pre[3], post[3]; // period-3 scale factors by index (coset zeta powers, 1/N)
    // batch mode, optional per vector: element i of srcs[b] is multiplied by pre_tabs[b][i] (times 2^266 as plain words, like
    // `pre`) on the way in instead of pre[i % 3]: the twist of a transform over the coset (zeta w_4n^j) H (poly_abi.hip ctx_ntt_cosets3)
    const Fr* pre_tabs[NTT_MAX_BATCH];
    uint32_t max_log_r; // 0 = default
};
hipError_t ntt_run(const NttJob& job, hipStream_t st);
void launch_twiddles(Fr* tw, const Fr& w, uint32_t n, hipStream_t st);           // w^i, standard Montgomery form
void launch_twiddles_scaled(Fr* tw, const Fr& w, const Fr& scale, uint32_t n, hipStream_t st);  // scale * w^i, standard form
void launch_twiddles_internal(Fr* tw, const Fr& w, uint32_t n, hipStream_t st);  // w^i * 2^261 (plain words): ntt.hip's own form

// ---- the three-coset route of a quotient with three pieces (poly.hip "three cosets") ----
struct Coset3Consts {  // constants of the 3 x 3 solve, standard form
    Fr inv2, inv_2z, zi, inv_2z2;  // 1/2, 1/(2 z), z i, 1/(2 z^2) with z = zeta^n, i = w_4n^n
    Fr zinv[3];                    // zeta^-(m mod 3)
};
void launch_coset3_pre(const Fr* tw_ext, uint32_t n, uint32_t j, const Fr zp1024[3], Fr* tab, hipStream_t st);
void launch_coset3_relayout(const Fr* const* src, Fr* const* dst, uint32_t count, uint32_t n, hipStream_t st);
void launch_coset3_combine(Fr* h, const Fr* tw_ext, uint32_t n, const Coset3Consts& k, hipStream_t st);

// ---- SRS generation (poly.hip) and RawBytes validation of device points (serde.hip) ----
void launch_srs_lagrange_scalars(const Fr* tw, uint32_t n, const Fr& s, const Fr& c, Fr* out, hipStream_t st);
void launch_srs_fixed_base(const Fr* scalars, uint32_t n, const G1Affine* table, G1Affine* out, hipStream_t st);
hipError_t launch_g1_validate(const G1Affine* d, uint32_t n, uint32_t* d_err, hipStream_t st);  // *d_err |= 1: a coordinate not below p, a point off the curve

// ---- MSM (msm.hip) ---------------------------------------------------------
struct MsmWorkspace;  // opaque, sized for a maximum n and a maximum number of columns per launch, and made for one plan (msm_plan.h
// msm_ws_plan): `fixed` = the fixed-base mode over a resident table of max_n points, otherwise arbitrary bases
MsmWorkspace* msm_workspace_create(size_t max_n, uint32_t c, bool fixed, hipError_t* err, uint32_t max_batch = 1);
void msm_workspace_destroy(MsmWorkspace* ws);
size_t msm_ws_max_n(const MsmWorkspace* ws);
uint32_t msm_ws_max_batch(const MsmWorkspace* ws);
uint32_t msm_ws_window(const MsmWorkspace* ws);
void msm_ws_set_t1_mode(MsmWorkspace* ws, uint32_t mode);  // ZK_OPT_MSM_T1: 1 one lane per bucket, 0 / 2 parts + segmented tree (default)
// table[w * n + i] = 2^(c w) * bases[i] (affine), w < nwin_for(c); the wide path's tables (15 .. 17-bit windows: msm_table_is_internal)
// hold the points in the accumulation's internal form, x * 2^261: they are read by the fixed-base MSM only
hipError_t msm_build_table(const G1Affine* bases, uint32_t n, uint32_t c, G1Affine* table, hipStream_t st);
bool msm_table_is_internal(uint32_t c, size_t n);
// whether any of the n points is the identity (synchronises `st`; scratch: a device word, a pinned host word): if none, the unchecked loop
hipError_t msm_bases_have_identity(const G1Affine* bases, uint32_t n, hipStream_t st, uint32_t* d_word, uint32_t* h_word, bool* out);
// One pass: `batch` columns of n scalars over a window table (fixed-base mode: ONE pass, a bucket set and a result per column), or, batch = 1, over `bases`
struct MsmPassArgs {
    const Fr* const* columns;
    uint32_t batch;
    size_t n;
    const G1Affine *bases, *table;  // arbitrary bases, or table[w * table_stride + i] = 2^(c w) P_i
    uint32_t table_stride;
    hipStream_t head, tail;      // sort head + accumulation | the reduction tail, behind head_done (tail == head, or none: in order)
    hipEvent_t head_done;
    hipEvent_t* events;          // optional timing: [0, 1] around the accumulation, [2, 3] around the wide path's tail
    bool bases_may_be_identity;  // false: the unchecked accumulation loop
    G1X* host_sums;              // pinned, device-visible: the bit sums (XYZZ) arrive here once `tail` has drained
};
// What the pass was, for msm_collect (the wide path: fixed-base mode, 15 .. 17-bit windows, table indexes within 26 bits; 20 sums per column)
struct MsmPass {
    enum Plan : uint32_t { GENERIC, FIXED, WIDE } plan;  // arbitrary bases / the standard plan over window tables / the wide path
    uint32_t batch, sums_per_result, c;  // results (one per column; one over all windows for arbitrary bases), G1X each, window bits
    size_t n;
    bool redo_word;  // behind the sums: the lanes the wide path's unchecked accumulation (n > 0) wants redone with the checked loop
    const G1Affine* table;
};
hipError_t msm_run(MsmWorkspace* ws, const MsmPassArgs& a, MsmPass* pass);
// Once `tail` has drained: the results (Jacobian, Montgomery), Horner over the sums; a non-zero redo word (a degenerate basis only)
// first runs those lanes and the tail again on `tail` and waits for it (*redone)
hipError_t msm_collect(MsmWorkspace* ws, const MsmPass& pass, hipStream_t tail, G1X* host_sums, G1Jac* out, bool* redone);

// ---- host helpers (ctx.hip) --------------------------------------------------
G1Affine g1_jac_to_affine_host(const G1Jac& p);

}  // namespace zk
