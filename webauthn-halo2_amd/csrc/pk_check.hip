// pk_check.hip — zk_pk_check: is a resident proving key what zk_keygen would have made of its own values?
//
// A ProvingKey holds every column four times (commitment, values, coefficients, extended coset) next to l_0 / l_last / l_active
// and the permutation's sigma columns, and zk_pk_read ties none of these copies to each other.  The audit recomputes each part
// from its source part AS IT STANDS IN THE KEY, through the routines zk_keygen itself uses (the fixed-base MSM passes,
// ctx_ntt), and compares the Montgomery images byte for byte (everything the engine makes is fully reduced, so the image is
// unique): values -> commitment, values -> coefficients, coefficients -> extended coset, the closed forms of the three l
// cosets; then sigma itself: every value a label delta^c' w^r' of a cell of the shape, and every cell named by some value.
//
// Shape of the work: the recomputed vector lands in pk->h_ext (idle between proofs, as zk_pk_write borrows it) and ONE streaming
// pass compares it with the key's copy — 16 bytes per lane, a wave's verdicts as one ballot, and only a wave that saw a
// mismatch touches the (part, column) counter: count by atomicAdd, lowest index by atomicMin, both order-independent, so the
// same key gives the same report on every run.  Sigma: decode -> mark (one bit per cell, atomicOr) -> count the unmarked.
#include <string.h>

#include <algorithm>
#include <vector>

#include "lane_call.h"
#include "pk.h"
#include "sigma_decode.hip.h"

using namespace zk;

namespace {

struct PcSlot {  // one (part, column) of parts 3 .. 9
    unsigned long long count;
    uint32_t lowest, pad;
};

constexpr uint32_t PC_MAX_BLOCKS = 2048;  // of the grid-stride compare: 8192 waves, every CU full

__global__ __launch_bounds__(256) void pc_reset_kernel(PcSlot* __restrict__ slots, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    slots[i].count = 0;
    slots[i].lowest = 0xffffffffu;
    slots[i].pad = 0;
}

// a wave's verdicts (bit b: index first_index + b) -> the wave's running count and lowest index; then its share of the slot
__device__ __forceinline__ void pc_wave_tally(unsigned long long m, uint32_t first_index, uint32_t& cnt, uint32_t& low) {
    if (!m) return;
    cnt += (uint32_t)__popcll(m);
    const uint32_t at = first_index + (uint32_t)__ffsll((long long)m) - 1;
    low = at < low ? at : low;
}
__device__ __forceinline__ void pc_wave_commit(PcSlot* __restrict__ slot, uint32_t cnt, uint32_t low) {
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicAdd(&slot->count, (unsigned long long)cnt);
        atomicMin(&slot->lowest, low);
    }
}

// a[0 .. len) against b[0 .. len), 32-byte elements read as 2 len 16-byte halves (lane i: half i, fully coalesced); an element
// differs if either half does: lanes 2 e and 2 e + 1 of the ballot
__global__ __launch_bounds__(256) void pc_compare_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, uint32_t halves,
                                                         PcSlot* __restrict__ slot) {
    uint32_t cnt = 0, low = 0xffffffffu;
    for (uint32_t base = blockIdx.x * 256u; base < halves; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        bool ne = false;
        if (i < halves) {
            const uint4 x = a[i], y = b[i];
            ne = (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
        }
        unsigned long long m = __ballot(ne);
        m = (m | (m >> 1)) & 0x5555555555555555ull;  // bit 2 e: element e of this wave's 32
        if (m) {
            cnt += (uint32_t)__popcll(m);
            const uint32_t at = ((i & ~63u) + (uint32_t)__ffsll((long long)m) - 1) >> 1;
            low = at < low ? at : low;
        }
    }
    pc_wave_commit(slot, cnt, low);
}

// the Lagrange vectors of the l cosets as zk_keygen builds them: 0 = e_0, 1 = e_usable, 2 = rows < usable
__global__ __launch_bounds__(256) void pc_unit_kernel(Fr* __restrict__ out, uint32_t n, uint32_t usable, uint32_t which) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const bool on = which == 0 ? r == 0 : which == 1 ? r == usable : r < usable;
    fe_store(out + r, on ? Fr::one() : Fr::zero());
}

// sigma: blockIdx.y = permutation column.  A value is a LABEL finding unless it is (r < usable) the image of a label
// delta^c' w^r' with c' < n_perm, r' < usable, or (r >= usable) the cell's own label; a cell without a finding marks the cell it
// names, a cell with one names nobody.  "Is the image of" is byte for byte: the decoded label is rebuilt and compared, so a
// non-reduced alias of a label (an unchecked file) is no label.
__global__ __launch_bounds__(256) void pc_sigma_mark_kernel(const Fr* const* __restrict__ sigma, const Fr* __restrict__ tw,
                                                            const Fr* __restrict__ consts, uint32_t n_perm, uint32_t k, uint32_t usable,
                                                            unsigned long long* __restrict__ marks, PcSlot* __restrict__ label_slots) {
    const uint32_t c = blockIdx.y, n = 1u << k;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false, own = false, other = false;
    uint32_t cc = 0, rr = 0;
    if (r < n) {
        const Fr v = fe_load(sigma[c] + r);
        own = v == fe_mul(fe_load(consts + c), fe_load(tw + r));
        if (!own) {
            other = r < usable && sigma_decode_label(v, consts, n_perm, k, &cc, &rr) && rr < usable &&
                    v == fe_mul(fe_load(consts + cc), fe_load(tw + rr));
            bad = !other;
        }
    }
    // fixed points (most cells): the wave's 64 cells are 64 consecutive bits — one atomic per wave once a column has whole words
    const unsigned long long own_m = __ballot(own);
    const size_t cell0 = (size_t)c * n + (r & ~63u);
    if (n >= 64) {
        if ((threadIdx.x & 63) == 0 && own_m) atomicOr(marks + (cell0 >> 6), own_m);
    } else if (own) {
        const size_t cell = (size_t)c * n + r;
        atomicOr(marks + (cell >> 6), 1ull << (cell & 63));
    }
    if (other) {
        const size_t cell = (size_t)cc * n + rr;
        atomicOr(marks + (cell >> 6), 1ull << (cell & 63));
    }
    uint32_t cnt = 0, low = 0xffffffffu;
    pc_wave_tally(__ballot(bad), r & ~63u, cnt, low);
    pc_wave_commit(label_slots + c, cnt, low);
}

// cells no sigma value names: blockIdx.y = permutation column
__global__ __launch_bounds__(256) void pc_sigma_missed_kernel(const unsigned long long* __restrict__ marks, uint32_t n,
                                                              PcSlot* __restrict__ map_slots) {
    const uint32_t c = blockIdx.y;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool missed = false;
    if (r < n) {
        const size_t cell = (size_t)c * n + r;
        missed = !((marks[cell >> 6] >> (cell & 63)) & 1ull);
    }
    uint32_t cnt = 0, low = 0xffffffffu;
    pc_wave_tally(__ballot(missed), r & ~63u, cnt, low);
    pc_wave_commit(map_slots + c, cnt, low);
}

}  // namespace

// what a key keeps for its audits: made by the first zk_pk_check of the key, freed with it
struct PkCheckState {
    uint32_t n_slots = 0, base[10] = {0};       // base[part]: first slot of parts 3 .. 9
    PcSlot *d_slots = nullptr, *h_slots = nullptr;  // h_: pinned
    unsigned long long* d_marks = nullptr;      // one bit per cell, n_perm x n
    size_t mark_words = 0;
    Fr* d_consts = nullptr;                     // sigma_decode_consts
    const Fr** d_sigma = nullptr;               // the key's sigma value columns
};

void pc_destroy(PkCheckState* s) {
    if (!s) return;
    if (s->d_slots) hipFree(s->d_slots);
    if (s->h_slots) hipHostFree(s->h_slots);
    if (s->d_marks) hipFree(s->d_marks);
    if (s->d_consts) hipFree(s->d_consts);
    if (s->d_sigma) hipFree(s->d_sigma);
    delete s;
}

namespace {

// the state of a key's audits, all of it or nothing; the decoder's constants and the column pointers never change for a key
int pc_ensure_state(zk_ctx* c, zk_pk_rec* pk) {
    if (pk->pc) return ZK_OK;
    const Layout& lay = pk->lay;
    PkCheckState* s = new (std::nothrow) PkCheckState();
    if (!s) return ZK_ENOMEM;
    const uint32_t m = (uint32_t)lay.perm_cols.size(), F = lay.n_fix;
    const uint32_t per_part[10] = {0, 0, 0, F, m, F, m, 3, m, m};
    for (uint32_t p = ZK_PK_PART_FIXED_POLY; p <= ZK_PK_PART_SIGMA_MAP; p++) {
        s->base[p] = s->n_slots;
        s->n_slots += per_part[p];
    }
    s->mark_words = ((size_t)m * lay.n + 63) / 64;
    const std::vector<Fr> consts = sigma_decode_consts(lay.k, m);
    std::vector<const Fr*> sig(pk->sigma_val.begin(), pk->sigma_val.end());
    const bool ok = hipMalloc(&s->d_slots, (size_t)s->n_slots * sizeof(PcSlot)) == hipSuccess &&
                    hipHostMalloc(&s->h_slots, (size_t)s->n_slots * sizeof(PcSlot)) == hipSuccess &&
                    hipMalloc(&s->d_marks, s->mark_words * 8) == hipSuccess &&
                    hipMalloc(&s->d_consts, consts.size() * sizeof(Fr)) == hipSuccess &&
                    hipMalloc(&s->d_sigma, (size_t)m * sizeof(Fr*)) == hipSuccess &&
                    hipMemcpyAsync(s->d_consts, consts.data(), consts.size() * sizeof(Fr), hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                    hipMemcpyAsync(s->d_sigma, sig.data(), (size_t)m * sizeof(Fr*), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    const hipError_t e = aud_sync(c, c->stream);  // (`consts` and `sig` leave scope)
    if (!ok || e != hipSuccess) {
        (void)hipGetLastError();
        pc_destroy(s);
        return ok ? ZK_EHIP : ZK_ENOMEM;
    }
    pk->pc = s;
    return ZK_OK;
}

void pc_compare(zk_ctx* c, const Fr* made, const Fr* kept, size_t len, PcSlot* slot, const char* site) {
    const uint32_t halves = (uint32_t)(2 * len);
    const uint32_t blocks = std::min<uint32_t>((halves + 255) / 256, PC_MAX_BLOCKS);
    hipLaunchKernelGGL(pc_compare_kernel, dim3(blocks), dim3(256), 0, c->stream, reinterpret_cast<const uint4*>(made),
                       reinterpret_cast<const uint4*>(kept), halves, slot);
    c->audit.op(c->stream, {made, kept, slot}, {slot}, site);
}

// values -> coefficients and coefficients -> extended coset of one column, each against the key's copy
int pc_column_forms(zk_ctx* c, zk_pk_rec* pk, const Fr* val, const Fr* poly, const Fr* coset, PcSlot* poly_slot, PcSlot* coset_slot) {
    const Layout& lay = pk->lay;
    const size_t n = lay.n, N = 4 * n;
    int rc = ctx_ntt(c, val, n, pk->h_ext, lay.k, true, false, n);  // lagrange_to_coeff
    if (rc) return rc;
    pc_compare(c, pk->h_ext, poly, n, poly_slot, "key audit: coefficients");
    if ((rc = ctx_ntt(c, poly, n, pk->h_ext, lay.ext_k, false, true, N))) return rc;  // coeff_to_extended
    pc_compare(c, pk->h_ext, coset, N, coset_slot, "key audit: extended coset");
    return ZK_OK;
}

}  // namespace

ZK_API(zk_pk_check, (zk_ctx* c, zk_pk h, uint32_t* flags, zk_pk_finding* out, size_t cap, size_t* n_findings), (c, h, flags, out, cap, n_findings)) {
    if (!c || !flags || !n_findings || (cap && !out)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    const Layout& lay = pk->lay;
    if (pk->srs_gen != c->srs_gen || pk->verify_only) return ZK_ESTATE;  // (a verifying-only key holds no column to audit)
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    if (rc) return rc;
    if ((rc = pc_ensure_state(c, pk))) return rc;
    PkCheckState* s = pk->pc;
    hipStream_t st = c->stream;
    const uint32_t n = lay.n, F = lay.n_fix, m = (uint32_t)lay.perm_cols.size(), gx = (n + 255) / 256;
    const Fr* tw = nullptr;
    if ((rc = ctx_get_twiddles(c, lay.k, &tw))) return rc;

    hipLaunchKernelGGL(pc_reset_kernel, dim3((s->n_slots + 255) / 256), dim3(256), 0, st, s->d_slots, s->n_slots);
    c->audit.op(st, {}, {s->d_slots}, "key audit: counters cleared");
    HIPCHK(c, hipMemsetAsync(s->d_marks, 0, s->mark_words * 8, st));
    c->audit.op(st, {}, {s->d_marks}, "key audit: marks cleared");

    // ---- parts 1, 2: commit_lagrange of every value column, many columns per MSM pass (as zk_commit_batch shares them)
    std::vector<zk_pk_finding> found;
    {
        std::vector<const Fr*> cols(pk->fixed_val.begin(), pk->fixed_val.end());
        cols.insert(cols.end(), pk->sigma_val.begin(), pk->sigma_val.end());
        const uint32_t pass = ctx_msm_max_batch(c);
        G1Jac js[MSM_MAX_BATCH];
        for (size_t i0 = 0; i0 < cols.size(); i0 += pass) {
            const uint32_t cnt = (uint32_t)std::min<size_t>(pass, cols.size() - i0);
            if ((rc = ctx_msm_begin_batch(c, 0, cols.data() + i0, cnt, c->g_lagrange, n))) return rc;
            if ((rc = ctx_msm_end_batch(c, 0, js))) return rc;
            for (uint32_t q = 0; q < cnt; q++) {
                const size_t col = i0 + q;
                const G1Affine a = g1_jac_to_affine_host(js[q]);
                const G1Affine& kept = col < F ? pk->fixed_commit[col] : pk->perm_commit[col - F];
                if (memcmp(&a, &kept, sizeof(G1Affine)) != 0)
                    found.push_back(zk_pk_finding{col < F ? (uint32_t)ZK_PK_PART_FIXED_COMMIT : (uint32_t)ZK_PK_PART_SIGMA_COMMIT,
                                                  (uint32_t)(col < F ? col : col - F), 0, 0, 1});
            }
        }
    }
    // ---- parts 3 - 6: the polynomial forms of every column
    for (uint32_t f = 0; f < F; f++)
        if ((rc = pc_column_forms(c, pk, pk->fixed_val[f], pk->fixed_poly[f], pk->fixed_coset[f], s->d_slots + s->base[ZK_PK_PART_FIXED_POLY] + f,
                                  s->d_slots + s->base[ZK_PK_PART_FIXED_COSET] + f)))
            return rc;
    for (uint32_t p = 0; p < m; p++)
        if ((rc = pc_column_forms(c, pk, pk->sigma_val[p], pk->sigma_poly[p], pk->sigma_coset[p], s->d_slots + s->base[ZK_PK_PART_SIGMA_POLY] + p,
                                  s->d_slots + s->base[ZK_PK_PART_SIGMA_COSET] + p)))
            return rc;
    // ---- part 7: l_0, l_last, l_active from their closed forms (zk_keygen: Lagrange vector -> coefficients -> extended coset)
    {
        const Fr* kept[3] = {pk->l0_coset, pk->l_last_coset, pk->l_active_coset};
        for (uint32_t w = 0; w < 3; w++) {
            hipLaunchKernelGGL(pc_unit_kernel, dim3(gx), dim3(256), 0, st, pk->t_a, n, lay.usable, w);
            c->audit.op(st, {}, {pk->t_a}, "key audit: l vector");
            if ((rc = ctx_ntt(c, pk->t_a, n, pk->t_a, lay.k, true, false, n))) return rc;
            if ((rc = ctx_ntt(c, pk->t_a, n, pk->h_ext, lay.ext_k, false, true, 4 * (size_t)n))) return rc;
            pc_compare(c, pk->h_ext, kept[w], 4 * (size_t)n, s->d_slots + s->base[ZK_PK_PART_L_COSET] + w, "key audit: l coset");
        }
    }
    // ---- parts 8, 9: sigma's values are labels, and every cell is named
    {
        hipLaunchKernelGGL(pc_sigma_mark_kernel, dim3(gx, m), dim3(256), 0, st, s->d_sigma, tw, s->d_consts, m, lay.k, lay.usable, s->d_marks,
                           s->d_slots + s->base[ZK_PK_PART_SIGMA_LABEL]);
        if (c->audit.on) {
            std::vector<const void*> rd(pk->sigma_val.begin(), pk->sigma_val.end());
            rd.push_back(s->d_sigma);
            rd.push_back(s->d_consts);
            rd.push_back(s->d_marks);
            rd.push_back(s->d_slots);
            const void* wr[2] = {s->d_marks, s->d_slots};
            c->audit.op_v(st, rd.data(), rd.size(), wr, 2, "key audit: sigma decode + mark");
        }
        hipLaunchKernelGGL(pc_sigma_missed_kernel, dim3(gx, m), dim3(256), 0, st, s->d_marks, n, s->d_slots + s->base[ZK_PK_PART_SIGMA_MAP]);
        c->audit.op(st, {s->d_marks, s->d_slots}, {s->d_slots}, "key audit: unnamed cells");
    }
    HIPCHK(c, hipMemcpyAsync(s->h_slots, s->d_slots, (size_t)s->n_slots * sizeof(PcSlot), hipMemcpyDeviceToHost, st));
    c->audit.op(st, {s->d_slots}, {s->h_slots}, "key audit: counters -> host");
    HIPCHK(c, aud_sync(c, st));
    if (hipGetLastError() != hipSuccess) return ZK_EHIP;
    c->audit.host_read(s->h_slots, "key audit: counters read by the host");

    for (uint32_t part = ZK_PK_PART_FIXED_POLY; part <= ZK_PK_PART_SIGMA_MAP; part++) {
        const uint32_t cnt = (part == ZK_PK_PART_SIGMA_MAP ? s->n_slots : s->base[part + 1]) - s->base[part];
        for (uint32_t col = 0; col < cnt; col++) {
            const PcSlot& sl = s->h_slots[s->base[part] + col];
            if (sl.count) found.push_back(zk_pk_finding{part, col, sl.lowest, 0, (uint64_t)sl.count});
        }
    }
    if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    uint32_t fl = ZK_PK_CHECK_ALL;
    for (const zk_pk_finding& f : found) {
        if (f.part <= ZK_PK_PART_SIGMA_COMMIT) fl &= ~ZK_PK_CHECK_COMMITMENTS;
        else if (f.part <= ZK_PK_PART_SIGMA_POLY) fl &= ~ZK_PK_CHECK_POLYS;
        else if (f.part <= ZK_PK_PART_L_COSET) fl &= ~ZK_PK_CHECK_COSETS;
        else fl &= ~ZK_PK_CHECK_SIGMA;
    }
    const Fr repr = pk_standin_transcript_repr(pk);
    if (memcmp(&repr, &pk->transcript_repr, sizeof(Fr)) == 0) fl |= ZK_PK_CHECK_REPR;
    const size_t listed = std::min(cap, found.size());
    if (listed) memcpy(out, found.data(), listed * sizeof(zk_pk_finding));
    *flags = fl;
    *n_findings = found.size();
    return ZK_OK;
}
