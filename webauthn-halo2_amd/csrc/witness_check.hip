// witness_check.hip — zk_witness_check: MockProver::verify of resident advice columns against a resident key.
//
// What the reference's only circuit test does (halo2-circuits/src/ecc/ecdsa_p256.rs:209-248:
// `MockProver::run(K, &circuit, vec![]).verify()`), for the circuit family of this engine: every gate
// q (a + b c - d) on the rows its selector is enabled on, every lookup input against the range table, every cell of a
// permutation column against the cell sigma maps it to.  The fixed columns' values and sigma's are the key's own
// (zk_pk_rec::fixed_val / sigma_val); nothing of the prover's workspace is touched and no proof byte depends on a check.
//
// Shape of the work: one thread per row, one launch per kind (blockIdx.y = gate column / lookup / permutation column); a wave
// writes its 64 verdicts as one ballot word, so a call leaves one bit per (kind, index, row) in a bitmap whose bit order IS the
// order of the result list.  Counts are popcounts of that bitmap, the list is a prefix scan over it — the same bits give the
// same list on every run.  The copy check reads sigma as cell indices: the key holds sigma as field values (a key read from a
// file holds nothing else), so they are decoded once per key into one uint32 per cell (wc_sigma_decode_kernel) and kept.
#include <string.h>

#include <algorithm>
#include <vector>

#include "lane_call.h"
#include "pk.h"
#include "sigma_decode.hip.h"

using namespace zk;

namespace {

constexpr uint32_t WC_BLOCK_WORDS = 1024;  // bitmap words per block of the count / list kernels (256 lanes x 4 words)
constexpr uint32_t WC_KINDS = 4;           // bitmap segments, in the list's order: ZK_FAIL_GATE, _GATE_BLINDED, _LOOKUP, _COPY

// argument block of the row kernels (device memory: up to 352 columns do not fit the kernarg segment comfortably)
struct WcArgs {
    const Fr* perm_val[MAX_PERM];  // the values of permutation column c: a fixed column of the key, an advice column or the instance column
    const Fr* sigma[MAX_PERM];     // the key's sigma values (decode only)
    const Fr* gate_adv[MAX_ADV];
    const Fr* gate_sel[MAX_ADV];   // the fixed column gate j's selector lives in
    uint32_t gate_form[MAX_ADV];   // Layout::gate_sel's form: 0 = q, 1 = q (2 - q), 2 = q (1 - q)
    const Fr* lk_in[MAX_LOOKUPS];  // lookup advice column; the one-column shape: a_0
    const Fr* lk_q;                // the one-column shape: q_lookup (input = q_lookup * a_0); otherwise null
};

struct WcSegs {
    uint32_t start[WC_KINDS + 1];  // first bitmap word of each kind's segment (multiples of WC_BLOCK_WORDS)
    uint32_t W;                    // words per (kind, index): ceil(n / 64)
};

// a wave's verdicts -> its word of the bitmap (one plain 8-byte store per wave; rows >= n have no word when n < 64 x lanes)
__device__ __forceinline__ void wc_put(uint64_t* __restrict__ bits, uint32_t row, uint32_t W, bool verdict) {
    const unsigned long long m = __ballot(verdict);
    const uint32_t w = row >> 6;
    if ((threadIdx.x & 63) == 0 && w < W) bits[w] = m;
}

// gates: blockIdx.y = gate column.  The effective selector after compress_selectors is q, q (2 - q) or q (1 - q): as field
// elements the latter two vanish exactly for q in {0, 2} / {0, 1}
__global__ __launch_bounds__(256) void wc_gate_kernel(const WcArgs* __restrict__ args, uint32_t n, uint32_t usable, uint32_t W,
                                                      uint64_t* __restrict__ fail_bits, uint64_t* __restrict__ blind_bits) {
    const uint32_t j = blockIdx.y;
    const Fr* __restrict__ a = args->gate_adv[j];
    const Fr* __restrict__ q = args->gate_sel[j];
    const uint32_t form = args->gate_form[j];
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false, blind = false;
    if (r < n) {
        const Fr s = fe_load(q + r);
        bool on = !s.is_zero();
        if (on && form) on = s != (form == 1 ? fe_dbl(Fr::one()) : Fr::one());
        if (on) {
            if (r + 3 >= usable) {
                blind = true;  // the gate reads a row the prover overwrites: MockProver's ConstraintPoisoned
            } else {
                const Fr v = fe_sub(fe_add(fe_load(a + r), fe_mul(fe_load(a + r + 1), fe_load(a + r + 2))), fe_load(a + r + 3));
                fail = !v.is_zero();
            }
        }
    }
    wc_put(fail_bits + (size_t)j * W, r, W, fail);
    wc_put(blind_bits + (size_t)j * W, r, W, blind);
}

// lookups: blockIdx.y = lookup; the table rule is lk_in_table (prover.h), the one lk_hist_kernel raises ZK_EWITNESS by
__global__ __launch_bounds__(256) void wc_lookup_kernel(const WcArgs* __restrict__ args, uint32_t usable, uint32_t T, uint32_t W,
                                                        uint64_t* __restrict__ bits) {
    const uint32_t l = blockIdx.y;
    const Fr* __restrict__ inp = args->lk_in[l];
    const Fr* __restrict__ q = args->lk_q;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    if (r < usable) {
        Fr v = fe_load(inp + r);
        if (q) v = fe_mul(fe_load(q + r), v);
        fail = !lk_in_table(fe_from_mont(v), T);
    }
    wc_put(bits + (size_t)l * W, r, W, fail);
}

// copies: blockIdx.y = permutation column; a gather through the decoded sigma (c' << k | r')
__global__ __launch_bounds__(256) void wc_copy_kernel(const WcArgs* __restrict__ args, const uint32_t* __restrict__ map, uint32_t k,
                                                      uint32_t usable, uint32_t W, uint64_t* __restrict__ bits) {
    const uint32_t c = blockIdx.y, n = 1u << k;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    if (r < usable) {
        const uint32_t m = map[(size_t)c * n + r];
        if (m != ((c << k) | r)) fail = fe_load(args->perm_val[c] + r) != fe_load(args->perm_val[m >> k] + (m & (n - 1)));
    }
    wc_put(bits + (size_t)c * W, r, W, fail);
}

// sigma values -> cell indices, once per key.  sigma(c, r) = delta^c' w^r': most cells are fixed points (one product tells);
// the others go through the decoder the key audit shares (sigma_decode.hip.h).  A value that is no such label, or a usable cell
// mapped into the rows the prover blinds, raises *bad (every writer stores the same word).
// consts: sigma_decode_consts
__global__ __launch_bounds__(256) void wc_sigma_decode_kernel(const WcArgs* __restrict__ args, const Fr* __restrict__ tw,
                                                              const Fr* __restrict__ consts, uint32_t n_perm, uint32_t k, uint32_t usable,
                                                              uint32_t* __restrict__ map, uint32_t* __restrict__ bad) {
    const uint32_t c = blockIdx.y, n = 1u << k;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const Fr v = fe_load(args->sigma[c] + r);
    uint32_t m = (c << k) | r;
    if (v != fe_mul(fe_load(consts + c), fe_load(tw + r))) {
        uint32_t cc = 0, rr = 0;
        if (!sigma_decode_label(v, consts, n_perm, k, &cc, &rr) || (r < usable && rr >= usable)) *bad = 1u;
        else m = (cc << k) | rr;
    }
    map[(size_t)c * n + r] = m;
}

__device__ __forceinline__ uint32_t wc_block_scan(uint32_t* sh, uint32_t mine) {  // inclusive, 256 lanes
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    return sh[threadIdx.x];
}

// failures per block of WC_BLOCK_WORDS bitmap words (a block lies in one kind's segment)
__global__ __launch_bounds__(256) void wc_count_kernel(const uint64_t* __restrict__ bits, uint32_t* __restrict__ blk) {
    __shared__ uint32_t sh[256];
    const uint64_t* w = bits + (size_t)blockIdx.x * WC_BLOCK_WORDS + threadIdx.x * 4;
    const uint32_t mine = __popcll(w[0]) + __popcll(w[1]) + __popcll(w[2]) + __popcll(w[3]);
    const uint32_t inc = wc_block_scan(sh, mine);
    if (threadIdx.x == 255) blk[blockIdx.x] = inc;
}

// the list: failure number off[block] + (set bits before it in the block) goes to out[that number] while it is below cap
__global__ __launch_bounds__(256) void wc_list_kernel(const uint64_t* __restrict__ bits, const uint64_t* __restrict__ off, WcSegs segs,
                                                      const uint32_t* __restrict__ map, uint32_t k, uint64_t cap,
                                                      zk_witness_failure* __restrict__ out) {
    __shared__ uint32_t sh[256];
    const uint32_t w0 = blockIdx.x * WC_BLOCK_WORDS + threadIdx.x * 4;
    uint64_t wd[4];
    uint32_t mine = 0;
    for (int i = 0; i < 4; i++) {
        wd[i] = bits[w0 + i];
        mine += __popcll(wd[i]);
    }
    const uint32_t inc = wc_block_scan(sh, mine);
    uint64_t pos = off[blockIdx.x] + (inc - mine);
    if (!mine || pos >= cap) return;
    uint32_t s = 0;
    while (s + 1 < WC_KINDS && w0 >= segs.start[s + 1]) s++;
    const uint32_t n = 1u << k;
    for (int i = 0; i < 4; i++) {
        const uint32_t rel = w0 + i - segs.start[s];
        const uint32_t index = rel / segs.W, row0 = (rel % segs.W) * 64;
        uint64_t word = wd[i];
        while (word && pos < cap) {
            const uint32_t b = (uint32_t)__ffsll((long long)word) - 1;
            word &= word - 1;
            const uint32_t row = row0 + b;
            uint32_t oi = 0, orow = 0;
            if (s + 1 == ZK_FAIL_COPY) {
                const uint32_t m = map[(size_t)index * n + row];
                oi = m >> k;
                orow = m & (n - 1);
            }
            uint32_t* o = reinterpret_cast<uint32_t*>(out + pos);
            o[0] = s + 1;
            o[1] = index;
            o[2] = row;
            o[3] = oi;
            o[4] = orow;
            o[5] = 0;
            pos++;
        }
    }
}

}  // namespace

// what a key keeps for its checks: made by the first zk_witness_check of the key, freed with it
struct WitnessCheckState {
    uint32_t* sigma_map = nullptr;  // n_perm x n cells, c' << k | r'
    bool decoded = false, sigma_bad = false;
    WcSegs segs{};
    uint32_t nblocks = 0;
    uint64_t* bits = nullptr;       // segs.start[WC_KINDS] words; the padding behind each segment stays zero
    uint32_t *d_blk = nullptr, *h_blk = nullptr;  // failures per block (h_: pinned)
    uint64_t *d_off = nullptr, *h_off = nullptr;  // failures in front of each block
    WcArgs *d_args = nullptr, *h_args = nullptr;
    uint32_t* d_bad = nullptr;
    zk_witness_failure *d_out = nullptr, *h_out = nullptr;
    size_t out_cap = 0;
};

void wc_destroy(WitnessCheckState* s) {
    if (!s) return;
    if (s->sigma_map) hipFree(s->sigma_map);
    if (s->bits) hipFree(s->bits);
    if (s->d_blk) hipFree(s->d_blk);
    if (s->h_blk) hipHostFree(s->h_blk);
    if (s->d_off) hipFree(s->d_off);
    if (s->h_off) hipHostFree(s->h_off);
    if (s->d_args) hipFree(s->d_args);
    if (s->h_args) hipHostFree(s->h_args);
    if (s->d_bad) hipFree(s->d_bad);
    if (s->d_out) hipFree(s->d_out);
    if (s->h_out) hipHostFree(s->h_out);
    delete s;
}

namespace {

// the state of a key's checks, all of it or nothing: a failed allocation gives back what the attempt took
int wc_ensure_state(zk_ctx* c, zk_pk_rec* pk) {
    if (pk->wc) return ZK_OK;
    const Layout& lay = pk->lay;
    WitnessCheckState* s = new (std::nothrow) WitnessCheckState();
    if (!s) return ZK_ENOMEM;
    const uint32_t n_perm = (uint32_t)lay.perm_cols.size();
    const uint32_t W = (lay.n + 63) / 64;
    const uint32_t per_kind[WC_KINDS] = {lay.n_gate, lay.n_gate, lay.n_lookups, n_perm};
    uint64_t at = 0;
    for (uint32_t q = 0; q < WC_KINDS; q++) {
        s->segs.start[q] = (uint32_t)at;
        at += ((uint64_t)per_kind[q] * W + WC_BLOCK_WORDS - 1) / WC_BLOCK_WORDS * WC_BLOCK_WORDS;
    }
    if (at >> 31) {  // (word indices are 32-bit)
        delete s;
        return ZK_EINVAL;
    }
    s->segs.start[WC_KINDS] = (uint32_t)at;
    s->segs.W = W;
    s->nblocks = (uint32_t)(at / WC_BLOCK_WORDS);
    const bool ok = hipMalloc(&s->sigma_map, (size_t)n_perm * lay.n * 4) == hipSuccess && hipMalloc(&s->bits, at * 8) == hipSuccess &&
                    hipMalloc(&s->d_blk, (size_t)s->nblocks * 4) == hipSuccess && hipHostMalloc(&s->h_blk, (size_t)s->nblocks * 4) == hipSuccess &&
                    hipMalloc(&s->d_off, (size_t)s->nblocks * 8) == hipSuccess && hipHostMalloc(&s->h_off, (size_t)s->nblocks * 8) == hipSuccess &&
                    hipMalloc(&s->d_args, sizeof(WcArgs)) == hipSuccess && hipHostMalloc(&s->h_args, sizeof(WcArgs)) == hipSuccess &&
                    hipMalloc(&s->d_bad, 4) == hipSuccess && hipMemsetAsync(s->bits, 0, at * 8, c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        aud_sync(c, c->stream);
        wc_destroy(s);
        return ZK_ENOMEM;
    }
    c->audit.op(c->stream, {}, {s->bits}, "witness check: bitmap cleared");
    pk->wc = s;
    return ZK_OK;
}

// the argument block for this call's advice columns -> device (the pinned staging is free: every call ends synchronised)
int wc_upload_args(zk_ctx* c, zk_pk_rec* pk, const std::vector<const Fr*>& adv) {
    const Layout& lay = pk->lay;
    WitnessCheckState* s = pk->wc;
    c->audit.host_write(s->h_args, "witness check: the host fills the argument block");
    WcArgs& a = *s->h_args;
    memset(&a, 0, sizeof(a));
    for (size_t p = 0; p < lay.perm_cols.size(); p++) {
        const Col& col = lay.perm_cols[p];
        a.perm_val[p] = col.type == COL_FIXED ? pk->fixed_val[col.idx] : col.type == COL_INSTANCE ? pk->inst_val : adv[col.idx];
        a.sigma[p] = pk->sigma_val[p];
    }
    for (uint32_t j = 0; j < lay.n_gate; j++) {
        a.gate_adv[j] = adv[j];
        a.gate_sel[j] = pk->fixed_val[lay.gate_sel[j] & 0xffffffu];
        a.gate_form[j] = lay.gate_sel[j] >> 24;
    }
    for (uint32_t l = 0; l < lay.n_lookups; l++) a.lk_in[l] = lay.single ? adv[0] : adv[lay.n_gate + l];
    a.lk_q = lay.single ? pk->fixed_val[lay.fx_qlookup] : nullptr;
    HIPCHK(c, hipMemcpyAsync(s->d_args, s->h_args, sizeof(WcArgs), hipMemcpyHostToDevice, c->stream));
    c->audit.op(c->stream, {s->h_args}, {s->d_args}, "witness check: argument block");
    return ZK_OK;
}

// sigma as cell indices, on the first check of a key; ZK_EINVAL if the key's sigma values are not labels of its own cells
int wc_ensure_sigma(zk_ctx* c, zk_pk_rec* pk) {
    WitnessCheckState* s = pk->wc;
    if (s->decoded) return s->sigma_bad ? ZK_EINVAL : ZK_OK;
    const Layout& lay = pk->lay;
    const uint32_t n_perm = (uint32_t)lay.perm_cols.size(), k = lay.k;
    const Fr* tw = nullptr;
    int rc = ctx_get_twiddles(c, k, &tw);
    if (rc) return rc;
    const std::vector<Fr> consts = sigma_decode_consts(k, n_perm);
    Fr* d_consts = nullptr;
    if (hipMalloc(&d_consts, consts.size() * sizeof(Fr)) != hipSuccess) {
        (void)hipGetLastError();
        return ZK_ENOMEM;
    }
    hipStream_t st = c->stream;
    uint32_t* h_bad = reinterpret_cast<uint32_t*>(c->host_small);
    hipError_t e = hipMemcpyAsync(d_consts, consts.data(), consts.size() * sizeof(Fr), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_bad, 0, 4, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(wc_sigma_decode_kernel, dim3((lay.n + 255) / 256, n_perm), dim3(256), 0, st, s->d_args, tw, d_consts, n_perm, k,
                           lay.usable, s->sigma_map, s->d_bad);
        if (c->audit.on) {
            std::vector<const void*> rd(pk->sigma_val.begin(), pk->sigma_val.end());
            rd.push_back(s->d_args);
            rd.push_back(d_consts);
            const void* wr[2] = {s->sigma_map, s->d_bad};
            c->audit.op_v(st, rd.data(), rd.size(), wr, 2, "witness check: sigma values -> cells");
        }
        e = hipMemcpyAsync(h_bad, s->d_bad, 4, hipMemcpyDeviceToHost, st);
        c->audit.op(st, {s->d_bad}, {h_bad}, "witness check: decode verdict");
    }
    if (e == hipSuccess) e = aud_sync(c, st);  // (also: `consts` leaves scope)
    else aud_sync(c, st);
    hipFree(d_consts);
    c->audit.base_of.clear();  // (the freed block's address may come back as another buffer)
    HIPCHK(c, e);
    c->audit.host_read(h_bad, "witness check: decode verdict read by the host");
    s->decoded = true;
    s->sigma_bad = *h_bad != 0;
    return s->sigma_bad ? ZK_EINVAL : ZK_OK;
}

}  // namespace

// `with_instances`: zk_witness_check_public — the caller's instance values go into the workspace's instance column (idle between
// proofs), the last permutation column of the copy check; zk_witness_check carries none and refuses a key that has the column
static int witness_check_run(zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, zk_witness_failure* out, size_t cap,
                             uint64_t counts[5], bool with_instances, const uint64_t* instance_mont, size_t n_instance) {
    if (!c || !advice || !counts || (cap && !out)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    const Layout& lay = pk->lay;
    if (lay.n_inst && !with_instances) return ZK_EINVAL;
    std::vector<Fr> instance;
    if (with_instances)
        if (int r = pk_instance_values(lay, instance_mont, n_instance, &instance)) return r;
    if (pk->srs_gen != c->srs_gen || pk->verify_only) return ZK_ESTATE;  // (a verifying-only key holds no column values)
    if (n_advice != lay.n_adv) return ZK_EINVAL;
    std::vector<const Fr*> adv(n_advice);
    for (size_t j = 0; j < n_advice; j++) {
        const PolyRec* r = ctx_poly(c, advice[j]);
        if (!r || r->n != lay.n) return ZK_EINVAL;
        adv[j] = r->ptr;
    }
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    if (rc) return rc;
    if ((rc = wc_ensure_state(c, pk))) return rc;
    WitnessCheckState* s = pk->wc;
    if ((rc = wc_upload_args(c, pk, adv))) return rc;
    if ((rc = wc_ensure_sigma(c, pk))) return rc;
    if ((rc = pk_instance_upload(c, c->stream, pk, instance))) return rc;

    hipStream_t st = c->stream;
    const uint32_t n = lay.n, W = s->segs.W, gx = (n + 255) / 256, n_perm = (uint32_t)lay.perm_cols.size();
    uint64_t* const seg[WC_KINDS] = {s->bits + s->segs.start[0], s->bits + s->segs.start[1], s->bits + s->segs.start[2], s->bits + s->segs.start[3]};
    std::vector<const void*> rd(adv.begin(), adv.end());
    for (const Fr* f : pk->fixed_val) rd.push_back(f);
    if (pk->inst_val) rd.push_back(pk->inst_val);
    rd.push_back(s->d_args);
    rd.push_back(s->sigma_map);
    const void* wr[1] = {s->bits};
    hipLaunchKernelGGL(wc_gate_kernel, dim3(gx, lay.n_gate), dim3(256), 0, st, s->d_args, n, lay.usable, W, seg[0], seg[1]);
    c->audit.op_v(st, rd.data(), rd.size(), wr, 1, "witness check: gates");
    hipLaunchKernelGGL(wc_lookup_kernel, dim3(gx, lay.n_lookups), dim3(256), 0, st, s->d_args, lay.usable, 1u << lay.lookup_bits, W, seg[2]);
    c->audit.op_v(st, rd.data(), rd.size(), wr, 1, "witness check: lookups");
    hipLaunchKernelGGL(wc_copy_kernel, dim3(gx, n_perm), dim3(256), 0, st, s->d_args, s->sigma_map, lay.k, lay.usable, W, seg[3]);
    c->audit.op_v(st, rd.data(), rd.size(), wr, 1, "witness check: copies");
    hipLaunchKernelGGL(wc_count_kernel, dim3(s->nblocks), dim3(256), 0, st, s->bits, s->d_blk);
    c->audit.op(st, {s->bits}, {s->d_blk}, "witness check: counts");
    HIPCHK(c, hipMemcpyAsync(s->h_blk, s->d_blk, (size_t)s->nblocks * 4, hipMemcpyDeviceToHost, st));
    c->audit.op(st, {s->d_blk}, {s->h_blk}, "witness check: counts -> host");
    HIPCHK(c, aud_sync(c, st));
    if (hipGetLastError() != hipSuccess) return ZK_EHIP;
    c->audit.host_read(s->h_blk, "witness check: counts read by the host");

    uint64_t cnt[WC_KINDS + 1] = {0, 0, 0, 0, 0};
    uint32_t list_blocks = 0;  // blocks that hold one of the first `cap` failures
    for (uint32_t b = 0, q = 0; b < s->nblocks; b++) {
        while (b * WC_BLOCK_WORDS >= s->segs.start[q + 1]) q++;
        s->h_off[b] = cnt[0];
        if (cnt[0] < cap && s->h_blk[b]) list_blocks = b + 1;
        cnt[0] += s->h_blk[b];
        cnt[q + 1] += s->h_blk[b];
    }
    const size_t listed = (size_t)std::min<uint64_t>(cap, cnt[0]);
    if (listed) {
        if (s->out_cap < listed) {
            if (s->d_out) hipFree(s->d_out);
            if (s->h_out) hipHostFree(s->h_out);
            s->d_out = s->h_out = nullptr;
            s->out_cap = 0;
            c->audit.base_of.clear();
            if (hipMalloc(&s->d_out, listed * sizeof(zk_witness_failure)) != hipSuccess ||
                hipHostMalloc(&s->h_out, listed * sizeof(zk_witness_failure)) != hipSuccess) {
                (void)hipGetLastError();
                if (s->d_out) hipFree(s->d_out);
                s->d_out = nullptr;
                return ZK_ENOMEM;
            }
            s->out_cap = listed;
        }
        HIPCHK(c, hipMemcpyAsync(s->d_off, s->h_off, (size_t)list_blocks * 8, hipMemcpyHostToDevice, st));
        c->audit.op(st, {s->h_off}, {s->d_off}, "witness check: block offsets");
        hipLaunchKernelGGL(wc_list_kernel, dim3(list_blocks), dim3(256), 0, st, s->bits, s->d_off, s->segs, s->sigma_map, lay.k, (uint64_t)listed, s->d_out);
        c->audit.op(st, {s->bits, s->d_off, s->sigma_map}, {s->d_out}, "witness check: list");
        HIPCHK(c, hipMemcpyAsync(s->h_out, s->d_out, listed * sizeof(zk_witness_failure), hipMemcpyDeviceToHost, st));
        c->audit.op(st, {s->d_out}, {s->h_out}, "witness check: list -> host");
        HIPCHK(c, aud_sync(c, st));
        if (hipGetLastError() != hipSuccess) return ZK_EHIP;
        c->audit.host_read(s->h_out, "witness check: list read by the host");
    }
    if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    if (listed) memcpy(out, s->h_out, listed * sizeof(zk_witness_failure));
    memcpy(counts, cnt, sizeof(cnt));
    return ZK_OK;
}

ZK_API(zk_witness_check, (zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, zk_witness_failure* out, size_t cap, uint64_t counts[5]), (c, h, advice, n_advice, out, cap, counts)) {
    return witness_check_run(c, h, advice, n_advice, out, cap, counts, false, nullptr, 0);
}

// MockProver::run(k, &circuit, vec![instance]).verify(): the same check with the instance column's values
ZK_API(zk_witness_check_public, (zk_ctx* c, zk_pk h, const zk_poly* advice, size_t n_advice, zk_witness_failure* out, size_t cap, uint64_t counts[5], const uint64_t* instance_mont, size_t n_instance), (c, h, advice, n_advice, out, cap, counts, instance_mont, n_instance)) {
    return witness_check_run(c, h, advice, n_advice, out, cap, counts, true, instance_mont, n_instance);
}
