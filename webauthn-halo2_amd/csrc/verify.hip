// verify.hip — plonk::verify_proof on the resident engine: zk_verify / zk_verify_batch, and the verifying-only keys of
// zk_vk_read / zk_vk_from_parts.
//
// One batch of proofs of one key goes through four steps:
//   1. device: every proof point of the batch is decoded in one launch (verify_decode_kernel: 32-byte compressed points of
//      the Blake2b transcript, 64-byte big-endian x || y of the EVM one), with a flag per point — canonical, on the curve,
//      not the identity, the rules of the repository's pinned verifier;
//   2. host: one transcript per proof (verifier.h) — challenges, expected h(x), the GWC or SHPLONK opening — giving the
//      two term lists of the proof's KZG check e(A_j, [s]G2) = e(B_j, G2); a proof that fails here (length, a point, a
//      non-canonical scalar) has its verdict and leaves the batch.  Spread over at most 16 host threads;
//   3. device: all A_j, B_j in one launch (verify_msm_kernel: one wave per accumulator, lanes own terms and share one
//      doubling chain over the scalars' bits, then a tree sum through LDS);
//   4. fold: A = sum rho_j A_j, B = sum rho_j B_j with 128-bit rho_j drawn from a hash of the key's transcript_repr and
//      every proof's bytes (the same kernel over the accumulators), ONE host pairing (pairing.h); if it fails, the set is
//      halved and each half folded and paired again, down to single proofs, so every verdict is the proof's own.  Under
//      zk_verify_pairing_mode 2 a failing fold of two or more proofs is settled by ONE launch of the device pairing instead
//      (pairing.hip: every (A_j, B_j) of the set, one check per lane); auto is the host.
// zk_verify is the batch of one: the same path, without a fold.
// zk_evm_verifier / zk_evm_verifier_cost: the same rule emitted as a Yul program for one kind of proof (evm_codegen.h; host only).
// Public inputs: every proof (zk_verify_batch_public) or circuit (zk_verify_multi_public) has its instance list; step 2 absorbs them
// and needs inst(x) per list — on the host inside verifier.h, or (zk_verify_instance_eval_mode 2) every transcript runs to x, ONE
// launch of instance_eval_kernel evaluates every list of the call, and the term lists take those values.  zk_instance_eval is
// that kernel alone.  The fold weights then hash every proof's list beside its bytes.
#include <string.h>

#include <algorithm>
#include <thread>

#include "evm_codegen.h"
#include "lane_call.h"
#include "pairing.h"
#include "pk.h"
#include "verifier.h"
#include "vkrepr.h"

using zk::verifier::Term;

namespace {

// point i of the batch: bytes at off[i]; out = affine Montgomery ((0, 0) when refused), flag[i] = 1 if the point is one the
// verifier accepts.  The encodings are g1_codec.hip.h's; the rule that is this caller's own: a proof holds no identity
__global__ void verify_decode_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ off, uint32_t n, int evm,
                                     G1Affine* __restrict__ out, uint8_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* b = bytes + off[i];
    G1Affine r;
    const bool ok = evm ? g1_read_evm(b, &r) : g1_decompress(b, &r) == G1_POINT;
    fe_store(&out[i].x, r.x);
    fe_store(&out[i].y, r.y);
    flag[i] = ok ? 1 : 0;
}

struct VSeg {
    uint32_t first, count;
};

// out[s] = sum over the segment's terms of scalar * base.  One 64-lane wave per segment; lane l owns terms l, l + 64, ...
// and all lanes walk the scalars' top `nbits` bits together (acc = 2 acc + the lane's bases whose bit is set), then the 64
// partial sums are added pairwise through LDS.  Scalars are canonical integers; a base index below n0 reads t0, below n0 + n1
// t1, anything else t2[0] (g[0] of the SRS).  Zero scalars and identity bases (0, 0) contribute nothing.
__global__ __launch_bounds__(64) void verify_msm_kernel(const Fr* __restrict__ scal, const uint32_t* __restrict__ idx, const VSeg* __restrict__ segs,
                                                        const G1Affine* __restrict__ t0, uint32_t n0, const G1Affine* __restrict__ t1, uint32_t n1,
                                                        const G1Affine* __restrict__ t2, uint32_t nbits, G1X* __restrict__ out) {
    __shared__ G1X sh[64];
    const VSeg sg = segs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    G1X acc = G1X::identity();
    for (int bit = (int)nbits - 1; bit >= 0; bit--) {
        acc = g1x_dbl(acc);
        for (uint32_t t = lane; t < sg.count; t += 64) {
            const uint32_t j = sg.first + t;
            const uint32_t w = reinterpret_cast<const uint32_t*>(scal + j)[bit >> 5];
            if (!((w >> (bit & 31)) & 1)) continue;
            const uint32_t bi = idx[j];
            const G1Affine* bp = bi < n0 ? t0 + bi : bi < n0 + n1 ? t1 + (bi - n0) : t2;
            const G1Affine p = affine_load(bp);
            if (!affine_is_identity(p)) g1x_add_affine(acc, p.x, p.y);
        }
    }
    sh[lane] = acc;
    __syncthreads();
    for (uint32_t s = 32; s > 0; s >>= 1) {
        if (lane < s) {
            G1X a = sh[lane];
            g1x_add(a, sh[lane + s]);
            sh[lane] = a;
        }
        __syncthreads();
    }
    if (lane == 0) g1x_store(out + blockIdx.x, sh[0]);
}

// ---- inst(x) = sum_{i<m} v_i l_i(x), l_i(x) = w^i (x^n - 1) / (n (x - w^i)), for many (list, point) pairs in one launch ----
// Stage 1, grid (pairs, slices): a workgroup is one 64-lane wave and owns slice `blockIdx.y` of pair `blockIdx.x`: IE_SLICE values,
// taken in passes of IE_SPAN = IE_WG x IE_LANE.  In a pass lane l owns the IE_LANE contiguous indices from base + l IE_LANE: w^i starts
// at one power (square-and-multiply) and advances by one product per element; the denominators x - w^i are inverted by Montgomery's
// trick in groups of IE_GROUP that never leave the lane (IE_GROUP prefix products per lane, ONE field inversion per group, the powers
// walked back by w^-1 rather than kept).  A zero denominator sets the pair's flag and is replaced by one (the sum is then
// discarded).  The lanes' sums are added through LDS; the slice's sum and flag go to part / pflag.
// Stage 2, one wave per pair: adds the slices' sums, multiplies by (x^n - 1) / n and writes the value — zero with the flag set where
// x is one of the list's w^i.  Field addition is exact and every value is a canonical Montgomery image, so the order of the
// additions does not show in the bytes: they are verifier::instance_eval's.
// Registers against occupancy: the compiler reports 110 VGPRs and keeps the IE_GROUP prefix products in 272 bytes of scratch per
// lane (four waves per SIMD); a longer group would trade more of either for fewer inversions.  One wave per workgroup needs no more
// occupancy than that: the lists are short (9 values at the server's shape: a single lane works) or long enough to fill the chip
// with slices (2^19 values: 256 workgroups).  LDS: 64 x 32 B per
// workgroup, read and written as whole elements per lane (ds_*_b128 pairs): no bank concern at this size.
constexpr uint32_t IE_GROUP = 8, IE_LANE = 16, IE_WG = 64, IE_SPAN = IE_WG * IE_LANE, IE_SLICE = 2 * IE_SPAN;
struct IePair {
    uint32_t off, len;  // the list: vals[off .. off + len)
};

__device__ __forceinline__ Fr ie_pow(Fr a, uint32_t e) {
    Fr acc = Fr::one();
    while (e) {
        if (e & 1) acc = fe_mul(acc, a);
        a = fe_sqr(a);
        e >>= 1;
    }
    return acc;
}

__global__ __launch_bounds__(64) void instance_eval_kernel(const Fr* __restrict__ vals, const IePair* __restrict__ pairs, const Fr* __restrict__ xs,
                                                           Fr omega, Fr omega_inv, uint32_t slices_max, Fr* __restrict__ part,
                                                           uint8_t* __restrict__ pflag) {
    __shared__ Fr sh[IE_WG];
    __shared__ uint32_t shf[IE_WG];
    const uint32_t j = blockIdx.x, slice = blockIdx.y, lane = threadIdx.x;
    const IePair pr = pairs[j];
    const uint64_t first = (uint64_t)slice * IE_SLICE;
    if (first >= pr.len) return;  // (the whole workgroup: no barrier has been reached; stage 2 reads the list's own slices only)
    const uint32_t end = (uint32_t)(first + IE_SLICE < pr.len ? first + IE_SLICE : pr.len);
    const Fr x = fe_load(xs + j);
    const Fr one = Fr::one();
    Fr acc = Fr::zero();
    uint32_t bad = 0;
    for (uint32_t base = (uint32_t)first + lane * IE_LANE; base < end; base += IE_SPAN) {
        Fr w = ie_pow(omega, base);
        const uint32_t stop = end < base + IE_LANE ? end : base + IE_LANE;
        for (uint32_t g0 = base; g0 < stop; g0 += IE_GROUP) {
            const uint32_t cnt = stop - g0 < IE_GROUP ? stop - g0 : IE_GROUP;
            Fr pre[IE_GROUP];
            Fr run = one;
#pragma unroll
            for (uint32_t t = 0; t < IE_GROUP; t++)
                if (t < cnt) {
                    Fr d = fe_sub(x, w);
                    if (d.is_zero()) {
                        bad = 1;
                        d = one;
                    }
                    pre[t] = run;
                    run = fe_mul(run, d);
                    w = fe_mul(w, omega);
                }
            Fr inv = fe_inv(run);  // (never zero: the zero denominators were replaced)
            Fr wb = w;             // w^(g0 + cnt)
#pragma unroll
            for (uint32_t u = 0; u < IE_GROUP; u++) {
                const uint32_t t = IE_GROUP - 1 - u;
                if (t < cnt) {
                    wb = fe_mul(wb, omega_inv);
                    Fr d = fe_sub(x, wb);
                    if (d.is_zero()) d = one;
                    const Fr di = fe_mul(inv, pre[t]);
                    inv = fe_mul(inv, d);
                    acc = fe_add(acc, fe_mul(fe_load(vals + pr.off + g0 + t), fe_mul(wb, di)));
                }
            }
        }
    }
    sh[lane] = acc;
    shf[lane] = bad;
    __syncthreads();
    for (uint32_t s = IE_WG / 2; s > 0; s >>= 1) {
        if (lane < s) {
            sh[lane] = fe_add(sh[lane], sh[lane + s]);
            shf[lane] |= shf[lane + s];
        }
        __syncthreads();
    }
    if (lane == 0) {
        const size_t o = (size_t)j * slices_max + slice;
        fe_store(part + o, sh[0]);
        pflag[o] = (uint8_t)shf[0];
    }
}

__global__ __launch_bounds__(64) void instance_eval_finish_kernel(const IePair* __restrict__ pairs, const Fr* __restrict__ xs, const Fr* __restrict__ part,
                                                                  const uint8_t* __restrict__ pflag, uint32_t slices_max, uint32_t k, Fr n_inv,
                                                                  Fr* __restrict__ out, uint8_t* __restrict__ on_domain) {
    __shared__ Fr sh[IE_WG];
    __shared__ uint32_t shf[IE_WG];
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    const uint32_t ns = (pairs[j].len + IE_SLICE - 1) / IE_SLICE;  // <= slices_max
    Fr acc = Fr::zero();
    uint32_t bad = 0;
    for (uint32_t s = lane; s < ns; s += IE_WG) {
        const size_t o = (size_t)j * slices_max + s;
        acc = fe_add(acc, fe_load(part + o));
        bad |= pflag[o];
    }
    sh[lane] = acc;
    shf[lane] = bad;
    __syncthreads();
    for (uint32_t s = IE_WG / 2; s > 0; s >>= 1) {
        if (lane < s) {
            sh[lane] = fe_add(sh[lane], sh[lane + s]);
            shf[lane] |= shf[lane + s];
        }
        __syncthreads();
    }
    if (lane == 0) {
        Fr xn = fe_load(xs + j);
        for (uint32_t i = 0; i < k; i++) xn = fe_sqr(xn);
        const Fr c = fe_mul(fe_sub(xn, Fr::one()), n_inv);
        fe_store(out + j, shf[0] ? Fr::zero() : fe_mul(sh[0], c));
        on_domain[j] = (uint8_t)(shf[0] ? 1 : 0);
    }
}

// affine forms of XYZZ sums (one inversion for all of them)
std::vector<G1Affine> to_affine_batch(const std::vector<G1X>& v) {
    std::vector<Fq> den, pre;
    for (const G1X& p : v)
        if (!p.is_identity()) {
            den.push_back(p.zz);
            den.push_back(p.zzz);
        }
    pre.resize(den.size());
    Fq acc = Fq::one();
    for (size_t i = 0; i < den.size(); i++) {
        pre[i] = acc;
        acc = fe_mul(acc, den[i]);
    }
    Fq inv = fe_inv_fast(acc);
    std::vector<Fq> dinv(den.size());
    for (size_t i = den.size(); i-- > 0;) {
        dinv[i] = fe_mul(inv, pre[i]);
        inv = fe_mul(inv, den[i]);
    }
    std::vector<G1Affine> out(v.size());
    size_t k = 0;
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i].is_identity()) {
            out[i].x = Fq::zero();
            out[i].y = Fq::zero();
            continue;
        }
        out[i].x = fe_mul(v[i].x, dinv[k++]);
        out[i].y = fe_mul(v[i].y, dinv[k++]);
    }
    return out;
}

template <class Fn>
void parallel_for(size_t n, Fn fn) {
    const size_t T = std::min<size_t>(16, n / 4);  // at most 16 host threads, never the machine's core count
    if (T <= 1) {
        for (size_t i = 0; i < n; i++) fn(i);
        return;
    }
    std::vector<std::thread> th;
    for (size_t t = 1; t < T; t++)
        th.emplace_back([&, t]() {
            for (size_t i = t; i < n; i += T) fn(i);
        });
    for (size_t i = 0; i < n; i += T) fn(i);
    for (auto& x : th) x.join();
}

}  // namespace

// the context's verify workspace (grow-only buffers, sized by the largest batch seen)
struct VerifyWs {
    DevBuf bytes, off, pts, flag, scal, idx, seg, out, fold;
    // instance_eval_device: the call's distinct lists, the pairs, their points, the slices' sums and flags, the results
    DevBuf ie_vals, ie_pairs, ie_x, ie_part, ie_pflag, ie_out, ie_flag;
};

void verify_ws_destroy(VerifyWs* w) { delete w; }

// a key record holding the verifying key only: commitments (host and device), transcript_repr; no SRS-sized memory
int pk_make_verify_only(zk_ctx* c, const Layout& lay, const std::vector<G1Affine>& fixed, const std::vector<G1Affine>& perm,
                        const uint64_t transcript_repr[4], zk_pk* out) {
    if (fixed.size() != lay.n_fix || perm.size() != lay.perm_cols.size()) return ZK_EINVAL;
    Fr repr;
    if (transcript_repr) {
        memcpy(&repr, transcript_repr, 32);
        if (!repr.below_modulus()) return ZK_EINVAL;  // a Montgomery image is < r
    } else {
        repr = vkrepr::transcript_repr(lay, fixed, perm);
    }
    zk_pk_rec* pk = new (std::nothrow) zk_pk_rec();
    if (!pk) return ZK_ENOMEM;
    pk->lay = lay;
    pk->verify_only = true;
    pk->srs_gen = c->srs_gen;
    pk->fixed_commit = fixed;
    pk->perm_commit = perm;
    pk->transcript_repr = repr;
    const uint64_t h = c->next_handle++;
    c->pks[h] = pk;
    *out = h;
    return ZK_OK;
}

// the key's commitments on the device (fixed, then permutation), made on the first verify and kept with the key
static int pk_vk_bases(zk_ctx* c, zk_pk_rec* pk) {
    if (pk->d_vk_bases) return ZK_OK;
    const size_t n = pk->fixed_commit.size() + pk->perm_commit.size();
    G1Affine* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(G1Affine)) != hipSuccess) return ZK_ENOMEM;
    pk->dev.push_back(reinterpret_cast<Fr*>(d));  // freed with the key's other allocations (pk_destroy)
    std::vector<G1Affine> h(pk->fixed_commit);
    h.insert(h.end(), pk->perm_commit.begin(), pk->perm_commit.end());
    if (c->audit.on) c->audit.op(c->stream, {}, {d}, "verify: key commitments upload");
    HIPCHK(c, hipMemcpyAsync(d, h.data(), n * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));  // (h is pageable and goes out of scope)
    pk->d_vk_bases = d;
    return ZK_OK;
}

ZK_API(zk_vk_from_parts, (zk_ctx* c, const zk_circuit_params* params, const uint64_t* fixed_commitments, const uint64_t* perm_commitments, const uint64_t transcript_repr[4], zk_pk* out), (c, params, fixed_commitments, perm_commitments, transcript_repr, out)) {
    if (!c || !params || !fixed_commitments || !perm_commitments || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    Layout lay;
    if (params->num_advice > 1 && 2 * (uint64_t)params->num_idle_gate_columns > params->num_advice) return ZK_ELAYOUT;
    if (!lay.init(*params)) return ZK_EINVAL;
    std::vector<G1Affine> fixed(lay.n_fix), perm(lay.perm_cols.size());
    memcpy(fixed.data(), fixed_commitments, fixed.size() * sizeof(G1Affine));
    memcpy(perm.data(), perm_commitments, perm.size() * sizeof(G1Affine));
    for (const std::vector<G1Affine>* v : {&fixed, &perm})
        for (const G1Affine& p : *v)
            if (!g1_raw_is_valid(p)) return ZK_EINVAL;  // the caller's Montgomery images: the checked RawBytes rule
    return pk_make_verify_only(c, lay, fixed, perm, transcript_repr, out);
}

// the description of the program of zk_evm_verifier: the key's shape, commitments and transcript_repr, the resident SRS's G2 half
static int evm_description(zk_ctx* c, zk_pk h, size_t n_circuits, const size_t* n_instances, int scheme, zk::evmgen::Desc* d) {
    if (n_circuits == 0 || n_circuits > ZK_PROVE_MULTI_MAX) return ZK_EINVAL;
    if (int r = resolve_scheme(ZK_TRANSCRIPT_EVM, &scheme)) return r;
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    const zk_pk_rec* pk = it->second;
    const Layout& lay = pk->lay;
    d->n_instances.assign(n_circuits, 0);
    for (size_t i = 0; n_instances && i < n_circuits; i++) {
        if (n_instances[i] > lay.usable || (n_instances[i] && !lay.n_inst)) return ZK_EINVAL;  // halo2's InstanceTooLarge
        d->n_instances[i] = (uint32_t)n_instances[i];
    }
    if (!pk->verify_only && pk->srs_gen != c->srs_gen) return ZK_ESTATE;  // as zk_verify
    if (c->srs_k < 0 || !c->g2_valid) return ZK_ESTATE;
    d->params = zk_circuit_params{lay.k, lay.A, lay.L, lay.F, lay.lookup_bits, lay.idle, lay.n_inst};
    d->fixed = pk->fixed_commit;
    d->perm = pk->perm_commit;
    d->transcript_repr = pk->transcript_repr;
    d->g2 = g2_from_raw(c->g2_raw);
    d->s_g2 = g2_from_raw(c->s_g2_raw);
    d->n_circuits = (uint32_t)n_circuits;
    d->shplonk = scheme == ZK_SCHEME_SHPLONK;
    return ZK_OK;
}

ZK_API(zk_evm_verifier, (zk_ctx* c, zk_pk h, size_t n_circuits, const size_t* n_instances, int scheme, char* out, size_t cap, size_t* len), (c, h, n_circuits, n_instances, scheme, out, cap, len)) {
    if (!c || !len) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    zk::evmgen::Desc d;
    if (int r = evm_description(c, h, n_circuits, n_instances, scheme, &d)) return r;
    std::string text;
    if (!zk::evmgen::generate(d, &text, nullptr)) return ZK_EINVAL;
    *len = text.size();
    if (!out) return ZK_OK;
    if (cap < text.size()) return ZK_EINVAL;
    memcpy(out, text.data(), text.size());
    return ZK_OK;
}

ZK_API(zk_evm_verifier_cost, (zk_ctx* c, zk_pk h, size_t n_circuits, const size_t* n_instances, int scheme, zk_evm_cost* out), (c, h, n_circuits, n_instances, scheme, out)) {
    if (!c || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    zk::evmgen::Desc d;
    if (int r = evm_description(c, h, n_circuits, n_instances, scheme, &d)) return r;
    zk_evm_cost cost;
    if (!zk::evmgen::generate(d, nullptr, &cost)) return ZK_EINVAL;
    *out = cost;
    return ZK_OK;
}

namespace {

struct Job {
    zk_ctx* c;
    zk_pk_rec* pk;
    VerifyWs* w;
    G2A g2, s_g2;
    // per proof of the batch that reached the device sums: A_j (index 2 j), B_j (2 j + 1) of the accumulators
    std::vector<uint32_t> live;
    std::vector<G1Affine> acc;
    std::vector<Fr> rho;
};

// sum_{j in S} rho_j A_j and rho_j B_j on the device (64 terms per segment; the segments' sums are added here)
int fold(Job& J, const std::vector<uint32_t>& S, G1Affine* A, G1Affine* B) {
    zk_ctx* c = J.c;
    VerifyWs* w = J.w;
    std::vector<Fr> sc;
    std::vector<uint32_t> ix;
    std::vector<VSeg> sg;
    for (int side = 0; side < 2; side++)
        for (size_t lo = 0; lo < S.size(); lo += 64) {
            const size_t hi = std::min(S.size(), lo + 64);
            sg.push_back({(uint32_t)sc.size(), (uint32_t)(hi - lo)});
            for (size_t t = lo; t < hi; t++) {
                sc.push_back(fe_from_mont(J.rho[S[t]]));
                ix.push_back(2 * S[t] + side);
            }
        }
    int rc;
    if ((rc = w->scal.grow(c, sc.size() * sizeof(Fr))) || (rc = w->idx.grow(c, ix.size() * 4)) ||
        (rc = w->seg.grow(c, sg.size() * sizeof(VSeg))) || (rc = w->out.grow(c, sg.size() * sizeof(G1X))))
        return rc;
    if (c->audit.on) c->audit.op(c->stream, {}, {w->scal.p, w->idx.p, w->seg.p}, "verify: fold arguments upload");
    HIPCHK(c, hipMemcpyAsync(w->scal.p, sc.data(), sc.size() * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w->idx.p, ix.data(), ix.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w->seg.p, sg.data(), sg.size() * sizeof(VSeg), hipMemcpyHostToDevice, c->stream));
    if (c->audit.on) c->audit.op(c->stream, {w->scal.p, w->idx.p, w->seg.p, w->fold.p}, {w->out.p}, "verify: fold (verify_msm_kernel)");
    hipLaunchKernelGGL(verify_msm_kernel, dim3((uint32_t)sg.size()), dim3(64), 0, c->stream, (const Fr*)w->scal.p, (const uint32_t*)w->idx.p,
                       (const VSeg*)w->seg.p, (const G1Affine*)w->fold.p, (uint32_t)J.acc.size(), (const G1Affine*)nullptr, 0u,
                       (const G1Affine*)w->fold.p, 128u, (G1X*)w->out.p);
    HIPCHK(c, hipGetLastError());
    std::vector<G1X> res(sg.size());
    if (c->audit.on) c->audit.op(c->stream, {w->out.p}, {}, "verify: fold results download");
    HIPCHK(c, hipMemcpyAsync(res.data(), w->out.p, res.size() * sizeof(G1X), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));
    G1X sum[2] = {G1X::identity(), G1X::identity()};
    const size_t per_side = sg.size() / 2;
    for (size_t i = 0; i < sg.size(); i++) g1x_add(sum[i / per_side], res[i]);
    const std::vector<G1Affine> af = to_affine_batch({sum[0], sum[1]});
    *A = af[0];
    *B = af[1];
    return ZK_OK;
}

// exact verdicts for the proofs S (positions into J.live): one fold + pairing; on failure halves (host), or under
// ZK_VERIFY_PAIRING_DEVICE every proof of S in one launch of the device pairing (pairing.hip), whose verdicts are final
int settle(Job& J, const std::vector<uint32_t>& S, uint8_t* verdicts) {
    if (S.empty()) return ZK_OK;
    bool ok;
    J.c->verify_pairing_stats[0]++;
    if (S.size() == 1) {
        ok = pairing_check(J.acc[2 * S[0]], J.acc[2 * S[0] + 1], J.g2, J.s_g2);
    } else {
        G1Affine A, B;
        if (int rc = fold(J, S, &A, &B)) return rc;
        ok = pairing_check(A, B, J.g2, J.s_g2);
    }
    if (ok) {
        for (uint32_t s : S) verdicts[J.live[s]] = 1;
        return ZK_OK;
    }
    if (S.size() == 1) return ZK_OK;
    if (J.c->opt_verify_pairing == ZK_VERIFY_PAIRING_DEVICE) {
        std::vector<G1Affine> a(S.size()), b(S.size());
        for (size_t t = 0; t < S.size(); t++) {
            a[t] = J.acc[2 * S[t]];
            b[t] = J.acc[2 * S[t] + 1];
        }
        std::vector<uint8_t> reasons(S.size());
        if (int rc = pairing_check_resident(J.c, S.size(), a.data(), b.data(), reasons.data())) return rc;
        J.c->verify_pairing_stats[1] += S.size();
        for (size_t t = 0; t < S.size(); t++) verdicts[J.live[S[t]]] = reasons[t] == ZK_PAIRING_VALID ? 1 : 0;
        return ZK_OK;
    }
    const size_t h = S.size() / 2;
    if (int rc = settle(J, std::vector<uint32_t>(S.begin(), S.begin() + h), verdicts)) return rc;
    return settle(J, std::vector<uint32_t>(S.begin() + h, S.end()), verdicts);
}

// inst(x) of `count` (list, point) pairs on the device in one launch (+ the small second stage): lists[j] at xs[j] over the domain
// of 2^k rows, every lists[j].n <= 2^k.  The call's DISTINCT lists — by address and length — are uploaded once.  out / on_domain:
// host arrays of `count`.  Caller holds the context lock, device bound
int instance_eval_device(zk_ctx* c, uint32_t k, size_t count, const verifier::InstanceList* lists, const Fr* xs, Fr* out, uint8_t* on_domain) {
    if (!count) return ZK_OK;
    if (k > 26 || count > 0x7fffffffu) return ZK_EINVAL;
    if (!c->vws && !(c->vws = new (std::nothrow) VerifyWs())) return ZK_ENOMEM;
    VerifyWs* w = c->vws;
    std::vector<IePair> pairs(count);
    std::vector<Fr> vals;
    std::vector<std::pair<verifier::InstanceList, uint32_t>> seen;  // (a call has few distinct lists: one per proof or circuit)
    size_t longest = 0;
    for (size_t j = 0; j < count; j++) {
        const verifier::InstanceList& l = lists[j];
        if (l.n > ((size_t)1 << k) || (l.n && !l.vals)) return ZK_EINVAL;
        longest = std::max(longest, l.n);
        uint32_t off = 0;
        bool have = l.n == 0;
        for (size_t s = seen.size(); s-- > 0 && !have;)
            if (seen[s].first.vals == l.vals && seen[s].first.n == l.n) {
                off = seen[s].second;
                have = true;
            }
        if (!have) {
            if (vals.size() + l.n > 0xffffffffu) return ZK_EINVAL;
            off = (uint32_t)vals.size();
            vals.insert(vals.end(), l.vals, l.vals + l.n);
            seen.push_back({l, off});
        }
        pairs[j] = IePair{off, (uint32_t)l.n};
    }
    const uint32_t slices_max = (uint32_t)std::max<size_t>(1, (longest + IE_SLICE - 1) / IE_SLICE);  // <= 2^26 / IE_SLICE: a grid's y extent
    const size_t np = count * (size_t)slices_max;
    int rc;
    if ((rc = w->ie_vals.grow(c, std::max<size_t>(vals.size(), 1) * sizeof(Fr))) ||
        (rc = w->ie_pairs.grow(c, count * sizeof(IePair))) || (rc = w->ie_x.grow(c, count * sizeof(Fr))) ||
        (rc = w->ie_part.grow(c, np * sizeof(Fr))) || (rc = w->ie_pflag.grow(c, np)) ||
        (rc = w->ie_out.grow(c, count * sizeof(Fr))) || (rc = w->ie_flag.grow(c, count)))
        return rc;
    if (c->audit.on) c->audit.op(c->stream, {}, {w->ie_vals.p, w->ie_pairs.p, w->ie_x.p}, "instance evaluation: lists, pairs and points upload");
    if (!vals.empty()) HIPCHK(c, hipMemcpyAsync(w->ie_vals.p, vals.data(), vals.size() * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w->ie_pairs.p, pairs.data(), count * sizeof(IePair), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w->ie_x.p, xs, count * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    const Fr omega = fr_omega(k), omega_inv = fe_inv_fast(omega), n_inv = fe_inv_fast(fr_from_u64((uint64_t)1 << k));
    if (c->audit.on) c->audit.op(c->stream, {w->ie_vals.p, w->ie_pairs.p, w->ie_x.p}, {w->ie_part.p, w->ie_pflag.p}, "instance evaluation (instance_eval_kernel)");
    hipLaunchKernelGGL(instance_eval_kernel, dim3((uint32_t)count, slices_max), dim3(IE_WG), 0, c->stream, (const Fr*)w->ie_vals.p, (const IePair*)w->ie_pairs.p,
                       (const Fr*)w->ie_x.p, omega, omega_inv, slices_max, (Fr*)w->ie_part.p, (uint8_t*)w->ie_pflag.p);
    HIPCHK(c, hipGetLastError());
    if (c->audit.on)
        c->audit.op(c->stream, {w->ie_pairs.p, w->ie_x.p, w->ie_part.p, w->ie_pflag.p}, {w->ie_out.p, w->ie_flag.p}, "instance evaluation: second stage");
    hipLaunchKernelGGL(instance_eval_finish_kernel, dim3((uint32_t)count), dim3(IE_WG), 0, c->stream, (const IePair*)w->ie_pairs.p, (const Fr*)w->ie_x.p,
                       (const Fr*)w->ie_part.p, (const uint8_t*)w->ie_pflag.p, slices_max, k, n_inv, (Fr*)w->ie_out.p, (uint8_t*)w->ie_flag.p);
    HIPCHK(c, hipGetLastError());
    if (c->audit.on) c->audit.op(c->stream, {w->ie_out.p, w->ie_flag.p}, {}, "instance evaluation: results download");
    HIPCHK(c, hipMemcpyAsync(out, w->ie_out.p, count * sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(on_domain, w->ie_flag.p, count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, aud_sync(c, c->stream));  // (the host vectors above are pageable and go out of scope)
    return ZK_OK;
}

}  // namespace

// `batch` proofs of one key, each over `n_circuits` circuits (1: the proofs of zk_prove; more: those of zk_prove_multi — a longer
// proof read in the order verifier.h states, the same four steps)
// `with_instances`: the _public forms — batch x n_circuits instance lists, proof-major (zk_verify_public: one; zk_verify_batch_public:
// one per proof; zk_verify_multi_public: one per circuit; none on a key without the column); the other entry points carry none and
// refuse a key that has the column (halo2's InvalidInstances).  `may_device`: the form follows zk_verify_instance_eval_mode (the lone
// zk_verify_public does not: it evaluates inst(x) on the host as it always did)
static int verify_proofs(zk_ctx* c, zk_pk h, size_t batch, uint32_t n_circuits, int transcript, int scheme, const uint8_t* const* proofs,
                         const size_t* lens, uint8_t* verdicts, bool with_instances = false, const uint64_t* const* instances_mont = nullptr,
                         const size_t* n_instances = nullptr, bool may_device = false) {
    if (!c || !proofs || !lens || !verdicts || batch == 0 || batch > ZK_VERIFY_BATCH_MAX) return ZK_EINVAL;
    if (int r = resolve_scheme(transcript, &scheme)) return r;
    for (size_t j = 0; j < batch; j++)
        if (!proofs[j] && lens[j]) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    if (pk->lay.n_inst && !with_instances) return ZK_EINVAL;
    std::vector<std::vector<Fr>> instance;  // list j * n_circuits + c: proof j, circuit c (a list the caller passes several times: once)
    std::vector<uint32_t> same_as;
    if (with_instances)
        if (int r = pk_instance_lists(pk->lay, batch * n_circuits, instances_mont, n_instances, &instance, &same_as)) return r;
    // the lists as verifier.h takes them: per proof n_circuits of them on a key with the column, none otherwise
    const size_t per_proof = pk->lay.n_inst ? n_circuits : 0;
    std::vector<verifier::InstanceList> ilists(batch * per_proof);
    for (size_t i = 0; i < ilists.size(); i++) ilists[i] = verifier::InstanceList{instance[same_as[i]].data(), instance[same_as[i]].size()};
    // where inst(x) is evaluated: auto is the host (the device path has not been measured against it)
    const bool on_device = may_device && per_proof && c->opt_verify_inst_eval == 2;
    if (!pk->verify_only && pk->srs_gen != c->srs_gen) return ZK_ESTATE;  // a full key under a replaced SRS: its vk is stale
    if (c->srs_k < 0 || !c->g2_valid) return ZK_ESTATE;  // g[0], g2 and s_g2 come from the resident SRS
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    if (rc) return rc;
    if (!c->vws && !(c->vws = new (std::nothrow) VerifyWs())) return ZK_ENOMEM;
    VerifyWs* w = c->vws;
    if ((rc = pk_vk_bases(c, pk))) return rc;
    const Layout& lay = pk->lay;
    const verifier::ProofLayout pl = verifier::proof_layout(lay, transcript == ZK_TRANSCRIPT_EVM, scheme == ZK_SCHEME_SHPLONK, n_circuits);
    std::vector<uint8_t> v(batch, 0);
    Job J{c, pk, w, g2_from_raw(c->g2_raw), g2_from_raw(c->s_g2_raw), {}, {}, {}};

    // 1. decode every point of every proof of the right length
    std::vector<uint32_t> cand;
    for (size_t j = 0; j < batch; j++)
        if (lens[j] == pl.len) cand.push_back((uint32_t)j);
    if (!cand.empty()) {
        const size_t np = pl.n_points, nb = cand.size() * pl.len, npts = cand.size() * np;
        std::vector<uint8_t> bytes(nb);
        std::vector<uint32_t> off(npts);
        for (size_t t = 0; t < cand.size(); t++) {
            memcpy(bytes.data() + t * pl.len, proofs[cand[t]], pl.len);
            for (size_t i = 0; i < np; i++) off[t * np + i] = (uint32_t)(t * pl.len + pl.point_off[i]);
        }
        if ((rc = w->bytes.grow(c, nb)) || (rc = w->off.grow(c, npts * 4)) ||
            (rc = w->pts.grow(c, npts * sizeof(G1Affine))) || (rc = w->flag.grow(c, npts)))
            return rc;
        if (c->audit.on) c->audit.op(c->stream, {}, {w->bytes.p, w->off.p}, "verify: proof bytes upload");
        HIPCHK(c, hipMemcpyAsync(w->bytes.p, bytes.data(), nb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(w->off.p, off.data(), npts * 4, hipMemcpyHostToDevice, c->stream));
        if (c->audit.on) c->audit.op(c->stream, {w->bytes.p, w->off.p}, {w->pts.p, w->flag.p}, "verify: point decoding (verify_decode_kernel)");
        hipLaunchKernelGGL(verify_decode_kernel, dim3((uint32_t)((npts + 63) / 64)), dim3(64), 0, c->stream, (const uint8_t*)w->bytes.p,
                           (const uint32_t*)w->off.p, (uint32_t)npts, transcript == ZK_TRANSCRIPT_EVM ? 1 : 0, (G1Affine*)w->pts.p, (uint8_t*)w->flag.p);
        HIPCHK(c, hipGetLastError());
        std::vector<G1Affine> pts(npts);
        std::vector<uint8_t> flag(npts);
        if (c->audit.on) c->audit.op(c->stream, {w->pts.p, w->flag.p}, {}, "verify: decoded points download");
        HIPCHK(c, hipMemcpyAsync(pts.data(), w->pts.p, npts * sizeof(G1Affine), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(flag.data(), w->flag.p, npts, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, aud_sync(c, c->stream));

        // 2. transcripts and term lists, per proof on the host.  With inst(x) on the device: every proof's transcript runs to x
        // first, ONE launch evaluates every (list, x) pair of the batch, and the term lists take those values
        std::vector<verifier::Prepared> prep(cand.size());
        std::vector<uint8_t> good(cand.size(), 0);
        std::vector<Fr> ie_out(on_device ? cand.size() * per_proof : 0);
        std::vector<uint8_t> ie_flag(ie_out.size(), 0);
        if (on_device) {
            std::vector<Fr> xs(ie_out.size(), Fr::zero());
            std::vector<verifier::InstanceList> pl_lists(ie_out.size());
            parallel_for(cand.size(), [&](size_t t) {
                try {
                    for (size_t i = 0; i < per_proof; i++) pl_lists[t * per_proof + i] = ilists[cand[t] * per_proof + i];
                    for (size_t i = 0; i < np; i++)
                        if (!flag[t * np + i]) return;  // (rejected below; its pairs are evaluated at zero and never read)
                    const Fr x = verifier::challenge_x(lay, pk->transcript_repr, pl, pts.data() + t * np, ilists.data() + cand[t] * per_proof, per_proof);
                    for (size_t i = 0; i < per_proof; i++) xs[t * per_proof + i] = x;
                } catch (...) {
                    good[t] = 2;
                }
            });
            for (uint8_t g : good)
                if (g == 2) return ZK_ENOMEM;
            if ((rc = instance_eval_device(c, lay.k, ie_out.size(), pl_lists.data(), xs.data(), ie_out.data(), ie_flag.data()))) return rc;
        }
        parallel_for(cand.size(), [&](size_t t) {
            try {
                for (size_t i = 0; i < np; i++)
                    if (!flag[t * np + i]) return;
                verifier::InstanceEvals given{nullptr, nullptr};
                if (on_device) given = verifier::InstanceEvals{ie_out.data() + t * per_proof, ie_flag.data() + t * per_proof};
                good[t] = verifier::prepare_lists(lay, pk->transcript_repr, pl, proofs[cand[t]], pts.data() + t * np, &prep[t],
                                                  ilists.data() + cand[t] * per_proof, per_proof, on_device ? &given : nullptr)
                              ? 1
                              : 0;
            } catch (...) {
                good[t] = 2;  // (allocation failure)
            }
        });
        for (uint8_t g : good)
            if (g == 2) return ZK_ENOMEM;

        // 3. every A_j, B_j in one launch.  Bases: the batch's decoded points, then the key's commitments, then g[0]
        std::vector<Fr> sc;
        std::vector<uint32_t> ix;
        std::vector<VSeg> sg;
        const uint32_t n_key = pl.n_fix + pl.n_perm;
        for (size_t t = 0; t < cand.size(); t++) {
            if (!good[t]) continue;
            J.live.push_back(cand[t]);
            for (const std::vector<Term>* terms : {&prep[t].a, &prep[t].b}) {
                sg.push_back({(uint32_t)sc.size(), (uint32_t)terms->size()});
                for (const Term& x : *terms) {
                    sc.push_back(fe_from_mont(x.s));
                    const uint32_t b = x.base;
                    ix.push_back(b < pl.n_points ? (uint32_t)(t * np + b) : b < pl.base_g0() ? (uint32_t)(npts + b - pl.n_points) : (uint32_t)(npts + n_key));
                }
            }
        }
        if (!J.live.empty()) {
            if ((rc = w->scal.grow(c, sc.size() * sizeof(Fr))) || (rc = w->idx.grow(c, ix.size() * 4)) ||
                (rc = w->seg.grow(c, sg.size() * sizeof(VSeg))) || (rc = w->out.grow(c, sg.size() * sizeof(G1X))))
                return rc;
            if (c->audit.on) c->audit.op(c->stream, {}, {w->scal.p, w->idx.p, w->seg.p}, "verify: term lists upload");
            HIPCHK(c, hipMemcpyAsync(w->scal.p, sc.data(), sc.size() * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(w->idx.p, ix.data(), ix.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(w->seg.p, sg.data(), sg.size() * sizeof(VSeg), hipMemcpyHostToDevice, c->stream));
            if (c->audit.on)
                c->audit.op(c->stream, {w->scal.p, w->idx.p, w->seg.p, w->pts.p, pk->d_vk_bases, c->g}, {w->out.p}, "verify: accumulators (verify_msm_kernel)");
            hipLaunchKernelGGL(verify_msm_kernel, dim3((uint32_t)sg.size()), dim3(64), 0, c->stream, (const Fr*)w->scal.p, (const uint32_t*)w->idx.p,
                               (const VSeg*)w->seg.p, (const G1Affine*)w->pts.p, (uint32_t)npts, (const G1Affine*)pk->d_vk_bases, n_key,
                               (const G1Affine*)c->g, 256u, (G1X*)w->out.p);
            HIPCHK(c, hipGetLastError());
            std::vector<G1X> res(sg.size());
            if (c->audit.on) c->audit.op(c->stream, {w->out.p}, {}, "verify: accumulators download");
            HIPCHK(c, hipMemcpyAsync(res.data(), w->out.p, res.size() * sizeof(G1X), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, aud_sync(c, c->stream));
            J.acc = to_affine_batch(res);

            // 4. fold with rho_j from a hash of the key and every proof, one pairing, bisection on failure
            if (J.live.size() > 1) {
                Blake2b hs("zkmi355-vbatch-r");
                const Fr repr = fe_from_mont(pk->transcript_repr);
                hs.update((const uint8_t*)repr.v, 32);
                for (size_t j = 0; j < batch; j++) {
                    const uint64_t ln = lens[j];
                    hs.update((const uint8_t*)&ln, 8);
                    if (ln) hs.update(proofs[j], ln);
                    // the statement is the proof AND its public inputs: every list, length first, beside the proof's bytes (the forms
                    // without instances hash what they always hashed)
                    if (with_instances)
                        for (size_t i = 0; i < n_circuits; i++) {
                            const std::vector<Fr>& l = instance[same_as[j * n_circuits + i]];
                            const uint64_t m = l.size();
                            hs.update((const uint8_t*)&m, 8);
                            if (m) hs.update((const uint8_t*)l.data(), m * sizeof(Fr));
                        }
                }
                uint8_t seed[64];
                hs.finalize_copy(seed);
                J.rho.resize(J.live.size());
                for (size_t s = 0; s < J.live.size(); s++) {
                    Blake2b hr("zkmi355-vbatch-j");
                    hr.update(seed, 64);
                    const uint64_t sj = s;
                    hr.update((const uint8_t*)&sj, 8);
                    uint8_t d[64];
                    hr.finalize_copy(d);
                    Fr r = Fr::zero();
                    memcpy(r.v, d, 16);  // 128 bits
                    if (r.is_zero()) r.v[0] = 1;
                    J.rho[s] = fe_to_mont(r);
                }
                if ((rc = w->fold.grow(c, J.acc.size() * sizeof(G1Affine)))) return rc;
                if (c->audit.on) c->audit.op(c->stream, {}, {w->fold.p}, "verify: accumulators upload for the fold");
                HIPCHK(c, hipMemcpyAsync(w->fold.p, J.acc.data(), J.acc.size() * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
            }
            std::vector<uint32_t> S(J.live.size());
            for (uint32_t s = 0; s < S.size(); s++) S[s] = s;
            if ((rc = settle(J, S, v.data()))) return rc;
        }
    }
    memcpy(verdicts, v.data(), batch);
    return aud_verdict(c, aud0, ZK_OK);
}

ZK_API(zk_verify_batch, (zk_ctx* c, zk_pk h, size_t batch, int transcript, int scheme, const uint8_t* const* proofs, const size_t* lens, uint8_t* verdicts), (c, h, batch, transcript, scheme, proofs, lens, verdicts)) {
    return verify_proofs(c, h, batch, 1, transcript, scheme, proofs, lens, verdicts);
}

// verify_proof with n_circuits instance slices (all empty): one proof of zk_prove_multi.  A proof of another circuit count has
// another length: a verdict of 0, like every bad proof
ZK_API(zk_verify_multi, (zk_ctx* c, zk_pk h, size_t n_circuits, int transcript, int scheme, const uint8_t* proof, size_t len, int* ok), (c, h, n_circuits, transcript, scheme, proof, len, ok)) {
    if (!ok || n_circuits == 0 || n_circuits > ZK_PROVE_MULTI_MAX) return ZK_EINVAL;
    uint8_t v = 0;
    const int rc = verify_proofs(c, h, 1, (uint32_t)n_circuits, transcript, scheme, &proof, &len, &v);
    if (rc == ZK_OK) *ok = v;
    return rc;
}

// verify_proof with the circuit's public inputs: wrong values are a verdict, a list the column cannot hold an error
ZK_API(zk_verify_public, (zk_ctx* c, zk_pk h, int transcript, int scheme, const uint64_t* instance_mont, size_t n_instance, const uint8_t* proof, size_t len, int* ok), (c, h, transcript, scheme, instance_mont, n_instance, proof, len, ok)) {
    if (!ok) return ZK_EINVAL;
    uint8_t v = 0;
    const int rc = verify_proofs(c, h, 1, 1, transcript, scheme, &proof, &len, &v, true, &instance_mont, &n_instance);
    if (rc == ZK_OK) *ok = v;
    return rc;
}

// zk_verify_batch with one instance list per proof: verdict j is zk_verify_public's of (proof j, list j)
ZK_API(zk_verify_batch_public, (zk_ctx* c, zk_pk h, size_t batch, int transcript, int scheme, const uint64_t* const* instances_mont, const size_t* n_instances, const uint8_t* const* proofs, const size_t* lens, uint8_t* verdicts), (c, h, batch, transcript, scheme, instances_mont, n_instances, proofs, lens, verdicts)) {
    return verify_proofs(c, h, batch, 1, transcript, scheme, proofs, lens, verdicts, true, instances_mont, n_instances, true);
}

// zk_verify_multi with one instance list per circuit (the multi rule: the lists are absorbed in circuit order behind
// transcript_repr; circuit c's permutation terms use inst_c(x))
ZK_API(zk_verify_multi_public, (zk_ctx* c, zk_pk h, size_t n_circuits, int transcript, int scheme, const uint64_t* const* instances_mont, const size_t* n_instances, const uint8_t* proof, size_t len, int* ok), (c, h, n_circuits, transcript, scheme, instances_mont, n_instances, proof, len, ok)) {
    if (!ok || n_circuits == 0 || n_circuits > ZK_PROVE_MULTI_MAX) return ZK_EINVAL;
    uint8_t v = 0;
    const int rc = verify_proofs(c, h, 1, (uint32_t)n_circuits, transcript, scheme, &proof, &len, &v, true, instances_mont, n_instances, true);
    if (rc == ZK_OK) *ok = v;
    return rc;
}

ZK_API(zk_verify_instance_eval_mode, (zk_ctx* c, int mode), (c, mode)) {
    if (!c || mode < 0 || mode > 2) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->opt_verify_inst_eval = (uint32_t)mode;
    return ZK_OK;
}

// how settle() finds the verdicts of a set of two or more proofs whose fold fails; auto is the host (the device route has not
// been measured against it)
ZK_API(zk_verify_pairing_mode, (zk_ctx* c, int mode), (c, mode)) {
    if (!c || mode < ZK_VERIFY_PAIRING_AUTO || mode > ZK_VERIFY_PAIRING_DEVICE) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->opt_verify_pairing = (uint32_t)mode;
    return ZK_OK;
}

ZK_API(zk_verify_pairing_stats, (zk_ctx* c, uint64_t out[2]), (c, out)) {
    if (!c || !out) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    out[0] = c->verify_pairing_stats[0];
    out[1] = c->verify_pairing_stats[1];
    return ZK_OK;
}

// inst(x) of `count` (list, point) pairs on the device: no SRS, no key.  Outputs are untouched on error
ZK_API(zk_instance_eval, (zk_ctx* c, uint32_t k, size_t count, const uint64_t* const* instances_mont, const size_t* n_instances, const uint64_t* x_mont, uint64_t* out_mont, uint8_t* on_domain), (c, k, count, instances_mont, n_instances, x_mont, out_mont, on_domain)) {
    if (!c || k > 26 || (count && (!n_instances || !x_mont || !out_mont || !on_domain))) return ZK_EINVAL;
    if (!count) return ZK_OK;
    std::vector<verifier::InstanceList> lists(count);
    std::vector<Fr> xs(count);
    memcpy(xs.data(), x_mont, count * sizeof(Fr));
    for (size_t j = 0; j < count; j++) {
        const size_t m = n_instances[j];
        if (m > ((size_t)1 << k) || (m && (!instances_mont || !instances_mont[j]))) return ZK_EINVAL;
        lists[j] = verifier::InstanceList{m ? reinterpret_cast<const Fr*>(instances_mont[j]) : nullptr, m};
        if (!xs[j].below_modulus()) return ZK_EINVAL;
    }
    // every value a Montgomery image below the modulus; a list that several pairs share is looked at once
    for (size_t j = 0; j < count; j++) {
        bool seen = false;
        for (size_t i = 0; i < j && !seen; i++) seen = lists[i].vals == lists[j].vals && lists[i].n >= lists[j].n;
        if (seen) continue;
        for (size_t i = 0; i < lists[j].n; i++)
            if (!lists[j].vals[i].below_modulus()) return ZK_EINVAL;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    uint64_t aud0;
    int rc = call_enter(c, &aud0);
    if (rc) return rc;
    std::vector<Fr> out(count);
    std::vector<uint8_t> flags(count);
    if ((rc = instance_eval_device(c, k, count, lists.data(), xs.data(), out.data(), flags.data()))) return rc;
    if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    memcpy(out_mont, out.data(), count * sizeof(Fr));
    memcpy(on_domain, flags.data(), count);
    return ZK_OK;
}

ZK_API(zk_verify, (zk_ctx* c, zk_pk h, int transcript, int scheme, const uint8_t* proof, size_t len, int* ok), (c, h, transcript, scheme, proof, len, ok)) {
    if (!ok) return ZK_EINVAL;
    uint8_t v = 0;
    const int rc = zk_verify_batch(c, h, 1, transcript, scheme, &proof, &len, &v);
    if (rc == ZK_OK) *ok = v;
    return rc;
}
