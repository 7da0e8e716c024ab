// serde.hip — the reference's on-disk artefacts, read and written by the resident engine.
//
// The reference re-reads two files on EVERY request (halo2-circuits/src/ecc/ecdsa_p256.rs:338-343, 388-393) and
// writes them at :261-270 / in halo2-base `gen_srs`:
//   ./params/kzg_bn254_{k}.srs   ParamsKZG::write / read                       (SRS)
//   ./keys/proving_key.pk        ProvingKey::write / read, SerdeFormat::RawBytes
//   ./keys/verifying_key.vk      VerifyingKey::write / read, SerdeFormat::RawBytes
// so that artefacts interchange with the unchanged Rust host, the engine speaks the
// same byte layouts.  They live in halo2_proofs (PSE fork, not under /root/reference) and are restated here from
// the published code [RECALLED — poly/kzg/commitment.rs `write_custom`, plonk.rs `VerifyingKey::write`,
// `ProvingKey::write`, plonk/permutation.rs, poly.rs `Polynomial::write`, helpers.rs `SerdeFormat`]:
//
//   SerdeFormat      Processed: field elements canonical little-endian (`to_repr`), points compressed (x LE, sign of
//                    y in bit 7 of the last byte, identity = all zero — the encoding the Blake2b transcript also uses);
//                    RawBytes: the in-memory Montgomery limbs, little-endian (Fr 32 B, G1Affine x||y 64 B, G2Affine
//                    x.c0||x.c1||y.c0||y.c1 128 B), validated on read; RawBytesUnchecked: the same bytes, no validation.
//   ParamsKZG        u32 LE k | g[0..n) | g_lagrange[0..n) | g2 | s_g2          (Params::write = RawBytes)
//   Polynomial       u32 BE len | len field elements;   slice of polynomials: u32 BE count | polynomials
//   VerifyingKey     u32 BE k | u32 BE #fixed | fixed commitments | permutation commitments (one per permutation
//                    column, no count) | selectors: per selector 2^k bits packed LSB-first into 2^k / 8 bytes
//                    (transcript_repr is NOT in the file: the Rust host re-hashes the pinned vk after reading — here
//                    it is supplied by the caller, zk_vk_load / zk_pk_read / zk_pk_set_transcript_repr)
//   ProvingKey       vk | l0 | l_last | l_active_row (extended-coset polynomials) | fixed_values | fixed_polys |
//                    fixed_cosets | permutation.permutations | .polys | .cosets   (six polynomial slices)
// Selector order: halo2-lib creates one `q_enable` selector per gate column, then (single-column strategy) the complex
// `q_lookup` selector; selector compression turns every enabled one into its own fixed column (they are not mutually
// exclusive), never-enabled ones into the constant 0 — the fixed-column order constants, table, selectors that the
// reference's k=17 verifying key shows (proving-server/P256Verifier.yul:880-926).
// Nothing of this exists in the reference's tests as bytes, so the formats are parity-unpinned beyond the known answers
// they carry: s_g2 of the SRS (yul:1131-1134) and the k=17 vk commitments (yul:880-980), see tests/.
#include <string.h>

#include "pairing.h"
#include "pk.h"
#include "serde_host.h"
#include "vkrepr.h"

namespace {

// ------------------------------------------------------------ device side ---

// The four codec kernels: one element per thread, the rule itself in g1_codec.hip.h / field.hip.h (the host readers run the same
// functions).  A refused element sets *err; a file admits the identity
__global__ void g1_decompress_kernel(const uint8_t* __restrict__ in, G1Affine* __restrict__ out, uint32_t n, uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine r;
    if (g1_decompress(in + (size_t)i * 32, &r) == G1_REFUSED) atomicOr(err, 1u);
    fe_store(&out[i].x, r.x);
    fe_store(&out[i].y, r.y);
}

__global__ void g1_compress_kernel(const G1Affine* __restrict__ in, uint8_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g1_compress(affine_load(in + i), out + (size_t)i * 32);
}

__global__ void g1_validate_kernel(const G1Affine* __restrict__ in, uint32_t n, uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !g1_raw_is_valid(affine_load(in + i))) atomicOr(err, 1u);
}

__global__ void fr_validate_kernel(const Fr* __restrict__ in, size_t n, uint32_t* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !fe_load(in + i).below_modulus()) atomicOr(err, 1u);
}

__global__ void fr_from_mont_kernel(Fr* a, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fe_store(a + i, fe_from_mont(fe_load(a + i)));
}
__global__ void fr_to_mont_kernel(Fr* a, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fe_store(a + i, fe_to_mont(fe_load(a + i)));
}

// -------------------------------------------------------------- host side ---
// (the point codecs, f2_sqrt and the bounded In / Out: serde_host.h)
bool format_ok(int f) { return f == ZK_SERDE_PROCESSED || f == ZK_SERDE_RAW_BYTES || f == ZK_SERDE_RAW_BYTES_UNCHECKED; }

uint32_t blocks_for(size_t n, uint32_t t = 256) { return (uint32_t)((n + t - 1) / t); }

// The frame of a ParamsKZG image, read once for both SRS readers: K from the header, the length K and the format give, both
// G2 points validated.  In this order: which fault refuses an image with several is behaviour
struct SrsImage {
    uint32_t K;
    size_t N, gs;  // points per G1 section, bytes per point
    uint8_t g2[128], s_g2[128];
    const uint8_t* bytes;
    const uint8_t* points(int section, size_t first) const { return bytes + 4 + ((size_t)section * N + first) * gs; }  // 0: g, 1: g_lagrange
};
bool srs_image_open(const uint8_t* bytes, size_t len, int format, SrsImage* im) {
    if (len < 4) return false;
    im->bytes = bytes;
    im->K = (uint32_t)bytes[0] | ((uint32_t)bytes[1] << 8) | ((uint32_t)bytes[2] << 16) | ((uint32_t)bytes[3] << 24);
    if (im->K < 1 || im->K > 24) return false;
    im->N = (size_t)1 << im->K;
    im->gs = g1_size(format);
    if (len != 4 + 2 * im->N * im->gs + 2 * g2_size(format)) return false;
    const uint8_t* g2 = bytes + 4 + 2 * im->N * im->gs;
    return host_g2_read(g2, format, im->g2) && host_g2_read(g2 + g2_size(format), format, im->s_g2);
}

// `cnt` points of a G1 section at `src` into dst: uploaded and decompressed through `packed` (Processed), uploaded and validated in
// place (RawBytes), or uploaded only (unchecked).  A refused point sets *d_err.  Stream-ordered; nothing is waited for, so the
// caller's next run may reuse `packed`
hipError_t srs_points_to_device(zk_ctx* c, const uint8_t* src, size_t cnt, int format, uint8_t* packed, G1Affine* dst, uint32_t* d_err) {
    const bool processed = format == ZK_SERDE_PROCESSED;
    const hipError_t e = hipMemcpyAsync(processed ? (void*)packed : (void*)dst, src, cnt * g1_size(format), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return e;
    if (processed) hipLaunchKernelGGL(g1_decompress_kernel, dim3(blocks_for(cnt, 64)), dim3(64), 0, c->stream, packed, dst, (uint32_t)cnt, d_err);
    else if (format == ZK_SERDE_RAW_BYTES) hipLaunchKernelGGL(g1_validate_kernel, dim3(blocks_for(cnt, 64)), dim3(64), 0, c->stream, dst, (uint32_t)cnt, d_err);
    return hipGetLastError();
}

}  // namespace

namespace zk {
// RawBytes validation of n device points (zk_g_to_lagrange): *d_err |= 1 for a coordinate not below p or a point off the curve
hipError_t launch_g1_validate(const G1Affine* d, uint32_t n, uint32_t* d_err, hipStream_t st) {
    hipLaunchKernelGGL(g1_validate_kernel, dim3(blocks_for(n, 64)), dim3(64), 0, st, d, n, d_err);
    return hipGetLastError();
}
}  // namespace zk

// s_g2 = [s]G2 after zk_srs_setup (called from srs.hip with the secret)
void srs_set_g2_from_secret(zk_ctx* c, const Fr& s_mont) {
    const G2A g = g2_generator();
    g2_to_raw(g, c->g2_raw);
    g2_to_raw(g2_mul(g, s_mont), c->s_g2_raw);
    c->g2_valid = true;
}

// ================================================================== SRS =====

ZK_API(zk_srs_set_g2, (zk_ctx* c, const uint64_t g2[16], const uint64_t s_g2[16]), (c, g2, s_g2)) {
    if (!c || !g2 || !s_g2) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0) return ZK_ESTATE;
    uint8_t a[128], b[128];
    if (!host_g2_read((const uint8_t*)g2, ZK_SERDE_RAW_BYTES, a) || !host_g2_read((const uint8_t*)s_g2, ZK_SERDE_RAW_BYTES, b)) return ZK_EINVAL;
    memcpy(c->g2_raw, a, 128);
    memcpy(c->s_g2_raw, b, 128);
    c->g2_valid = true;
    c->pair_lines.reset();  // the device pairing's table of the previous pair
    return ZK_OK;
}

ZK_API(zk_srs_write, (zk_ctx* c, int format, uint8_t* out, size_t cap, size_t* len), (c, format, out, cap, len)) {
    if (!c || !len || !format_ok(format)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0 || !c->g2_valid) return ZK_ESTATE;  // after zk_srs_load the G2 half must be given: zk_srs_set_g2
    const size_t n = (size_t)1 << c->srs_k;
    const size_t gs = g1_size(format);
    const size_t total = 4 + 2 * n * gs + 2 * g2_size(format);
    *len = total;
    if (!out) return ZK_OK;
    if (cap < total) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    const uint32_t k = (uint32_t)c->srs_k;
    out[0] = (uint8_t)k;
    out[1] = (uint8_t)(k >> 8);
    out[2] = (uint8_t)(k >> 16);
    out[3] = (uint8_t)(k >> 24);
    uint8_t* p = out + 4;
    for (int b = 0; b < 2; b++) {
        const G1Affine* src = b ? c->g_lagrange : c->g;
        if (format == ZK_SERDE_PROCESSED) {
            uint8_t* tmp = nullptr;
            if (hipMalloc(&tmp, n * 32) != hipSuccess) return ZK_ENOMEM;
            hipLaunchKernelGGL(g1_compress_kernel, dim3(blocks_for(n)), dim3(256), 0, c->stream, src, tmp, (uint32_t)n);
            hipError_t e = hipMemcpyAsync(p, tmp, n * 32, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            hipFree(tmp);
            if (e != hipSuccess) {
                c->last_hip = (int)e;
                return ZK_EHIP;
            }
        } else {
            HIPCHK(c, hipMemcpy(p, src, n * 64, hipMemcpyDeviceToHost));
        }
        p += n * gs;
    }
    host_g2_write(c->g2_raw, format, p);
    host_g2_write(c->s_g2_raw, format, p + g2_size(format));
    return ZK_OK;
}

ZK_API(zk_srs_read, (zk_ctx* c, const uint8_t* bytes, size_t len, int format), (c, bytes, len, format)) {
    if (!c || !bytes || !format_ok(format)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    SrsImage im;
    if (!srs_image_open(bytes, len, format, &im)) return ZK_EINVAL;
    const uint32_t k = im.K;
    const size_t n = im.N;
    int rc = ctx_bind(c);
    if (rc) return rc;
    ctx_release_spares(c);  // the old SRS, its tables and the new bases are alive together below: parked vectors go first
    // decode and validate into fresh buffers: a malformed file leaves the resident SRS, its tables and the keys made under
    // it as they were (they are replaced only once every point has been accepted)
    G1Affine* fresh[2] = {nullptr, nullptr};
    uint32_t* d_err = nullptr;
    uint8_t* tmp = nullptr;  // one section's compressed points (Processed)
    auto drop = [&]() {
        hipFree(fresh[0]);
        hipFree(fresh[1]);
        hipFree(d_err);
        hipFree(tmp);
    };
    if (hipMalloc(&fresh[0], n * sizeof(G1Affine)) != hipSuccess || hipMalloc(&fresh[1], n * sizeof(G1Affine)) != hipSuccess ||
        hipMalloc(&d_err, 4) != hipSuccess || (format == ZK_SERDE_PROCESSED && hipMalloc(&tmp, n * 32) != hipSuccess)) {
        drop();
        return ZK_ENOMEM;
    }
    hipError_t e = hipMemsetAsync(d_err, 0, 4, c->stream);
    for (int b = 0; b < 2 && e == hipSuccess; b++) e = srs_points_to_device(c, im.points(b, 0), n, format, tmp, fresh[b], d_err);
    uint32_t herr = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        drop();
        c->last_hip = (int)e;
        return ZK_EHIP;
    }
    if (herr) {  // a point off the curve / a non-canonical coordinate: halo2's read fails the same way
        drop();
        return ZK_EINVAL;
    }
    hipFree(d_err);
    hipFree(tmp);
    srs_adopt(c, k, fresh[0], fresh[1]);
    if ((rc = srs_build_tables(c, k)) != ZK_OK) return rc;
    c->srs_k = (int)k;
    memcpy(c->g2_raw, im.g2, 128);
    memcpy(c->s_g2_raw, im.s_g2, 128);
    c->g2_valid = true;
    return ZK_OK;
}

// ParamsKZG::read_custom + downsize(k) without anything of the file's degree K on the device: the image is checked as
// zk_srs_read checks it (length, both G2 points, every point of both G1 sections unless the format is unchecked), streamed
// through a staging buffer of SRS_STAGE points; the first 2^k points of g are kept, g_lagrange is rebuilt from them.
ZK_API(zk_srs_read_downsize, (zk_ctx* c, const uint8_t* bytes, size_t len, int format, uint32_t k), (c, bytes, len, format, k)) {
    if (!c || !bytes || !format_ok(format)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    SrsImage im;
    if (!srs_image_open(bytes, len, format, &im)) return ZK_EINVAL;
    const size_t N = im.N;
    if (k < 1 || k > im.K) return ZK_EINVAL;  // halo2's downsize asserts k <= self.k
    int rc = ctx_bind(c);
    if (rc) return rc;
    ctx_release_spares(c);
    const size_t n = (size_t)1 << k;
    const size_t SRS_STAGE = (size_t)1 << 18;
    const size_t chunk = N < SRS_STAGE ? N : SRS_STAGE;
    G1Affine *g = nullptr, *gl = nullptr, *stage = nullptr;
    uint8_t* packed = nullptr;  // compressed points (Processed)
    uint32_t* d_err = (uint32_t*)c->small;
    auto drop = [&]() {
        hipFree(g);
        hipFree(gl);
        hipFree(stage);
        hipFree(packed);
    };
    if (hipMalloc(&g, n * sizeof(G1Affine)) != hipSuccess || hipMalloc(&gl, n * sizeof(G1Affine)) != hipSuccess ||
        hipMalloc(&stage, chunk * sizeof(G1Affine)) != hipSuccess ||
        (format == ZK_SERDE_PROCESSED && hipMalloc(&packed, chunk * 32) != hipSuccess)) {
        (void)hipGetLastError();
        drop();
        return ZK_ENOMEM;
    }
    hipError_t e = hipMemsetAsync(d_err, 0, 4, c->stream);
    // section 0 = g, 1 = g_lagrange; an unchecked image needs nothing beyond g[0 .. n)
    for (int b = 0; b < 2 && e == hipSuccess; b++) {
        const size_t end = format == ZK_SERDE_RAW_BYTES_UNCHECKED ? (b ? 0 : n) : N;
        for (size_t off = 0; off < end && e == hipSuccess; off += chunk) {
            const size_t cnt = end - off < chunk ? end - off : chunk;
            e = srs_points_to_device(c, im.points(b, off), cnt, format, packed, stage, d_err);
            if (e == hipSuccess && b == 0 && off < n) {
                const size_t keep = n - off < cnt ? n - off : cnt;
                e = hipMemcpyAsync(g + off, stage, keep * sizeof(G1Affine), hipMemcpyDeviceToDevice, c->stream);
            }
        }
    }
    uint32_t herr = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(stage);
    hipFree(packed);
    stage = nullptr;
    packed = nullptr;
    if (e != hipSuccess) {
        drop();
        c->last_hip = (int)e;
        return ZK_EHIP;
    }
    if (herr) {  // as zk_srs_read: a point off the curve / a non-canonical coordinate anywhere in the file
        drop();
        return ZK_EINVAL;
    }
    if ((rc = ctx_g1_to_lagrange(c, g, (uint32_t)k, gl)) != ZK_OK) {
        drop();
        return rc;
    }
    // the new SRS goes in whole or not at all: until srs_install succeeds the resident one, its G2 half and its keys stay
    if ((rc = srs_install(c, (uint32_t)k, g, gl)) != ZK_OK) return rc;
    memcpy(c->g2_raw, im.g2, 128);
    memcpy(c->s_g2_raw, im.s_g2, 128);
    c->g2_valid = true;
    return ZK_OK;
}

// =========================================================== vk / pk ========

namespace {

uint32_t n_selectors(const Layout& lay) { return lay.n_gate + (lay.single ? 1 : 0); }
// fixed column holding selector s (NO_SELECTOR: compressed away, all-false)
uint32_t selector_column(const Layout& lay, uint32_t s) { return s < lay.n_gate ? lay.fx_sel[s] : lay.fx_qlookup; }

size_t vk_size(const Layout& lay, int format) {
    return 8 + (lay.n_fix + lay.perm_cols.size()) * g1_size(format) + (size_t)n_selectors(lay) * (lay.n / 8);
}
size_t fr_size() { return 32; }
size_t poly_size(size_t len) { return 4 + len * fr_size(); }
size_t pk_size(const Layout& lay, int format) {
    const size_t n = lay.n, N = 4 * n, m = lay.perm_cols.size();
    return vk_size(lay, format) + 3 * poly_size(N) + 3 * 4 + lay.n_fix * (2 * poly_size(n) + poly_size(N)) + 3 * 4 +
           m * (2 * poly_size(n) + poly_size(N));
}

// selector bits of the resident key: the selector columns are 0/1-valued fixed columns
int selector_bits(zk_ctx* c, const zk_pk_rec* pk, std::vector<std::vector<uint8_t>>* out) {
    const Layout& lay = pk->lay;
    const uint32_t n = lay.n;
    std::vector<Fr> col(n);
    out->assign(n_selectors(lay), std::vector<uint8_t>(n / 8, 0));
    for (uint32_t s = 0; s < n_selectors(lay); s++) {
        const uint32_t f = selector_column(lay, s);
        if (f == NO_SELECTOR) continue;
        HIPCHK(c, hipMemcpy(col.data(), pk->fixed_val[f], (size_t)n * sizeof(Fr), hipMemcpyDeviceToHost));
        for (uint32_t r = 0; r < n; r++) {
            if (col[r].is_zero()) continue;
            if (col[r] != Fr::one()) return ZK_ESTATE;  // not a selector column
            (*out)[s][r >> 3] |= (uint8_t)(1u << (r & 7));
        }
    }
    return ZK_OK;
}

int write_vk(zk_ctx* c, const zk_pk_rec* pk, int format, Out& o) {
    const Layout& lay = pk->lay;
    if (uint8_t* p = o.take(4)) put_be32(p, lay.k);
    if (uint8_t* p = o.take(4)) put_be32(p, lay.n_fix);
    for (uint32_t i : vkrepr::halo2_fixed_order(lay))  // halo2's column order: the table column first (vkrepr.h)
        if (uint8_t* p = o.take(g1_size(format))) host_g1_write(pk->fixed_commit[i], format, p);
    for (const G1Affine& cm : pk->perm_commit)
        if (uint8_t* p = o.take(g1_size(format))) host_g1_write(cm, format, p);
    if (!o.real) {
        o.take((size_t)n_selectors(lay) * (lay.n / 8));
        return ZK_OK;
    }
    std::vector<std::vector<uint8_t>> bits;
    int rc = selector_bits(c, pk, &bits);
    if (rc) return rc;
    for (auto& b : bits)
        if (uint8_t* p = o.take(b.size())) memcpy(p, b.data(), b.size());
    return ZK_OK;
}

struct ParsedVk {
    std::vector<G1Affine> fixed, perm;
    std::vector<std::vector<uint8_t>> selectors;
};
int parse_vk(const Layout& lay, In& in, int format, ParsedVk* out) {
    const uint8_t* p = in.take(8);
    if (!p || get_be32(p) != lay.k || get_be32(p + 4) != lay.n_fix) return ZK_EINVAL;
    out->fixed.resize(lay.n_fix);
    out->perm.resize(lay.perm_cols.size());
    for (uint32_t i : vkrepr::halo2_fixed_order(lay)) {  // the file lists the fixed columns in halo2's column order
        const uint8_t* b = in.take(g1_size(format));
        if (!b || !host_g1_read(b, format, &out->fixed[i])) return ZK_EINVAL;
    }
    for (G1Affine& cm : out->perm) {
        const uint8_t* b = in.take(g1_size(format));
        if (!b || !host_g1_read(b, format, &cm)) return ZK_EINVAL;
    }
    out->selectors.assign(n_selectors(lay), std::vector<uint8_t>(lay.n / 8));
    for (auto& s : out->selectors) {
        const uint8_t* b = in.take(s.size());
        if (!b) return ZK_EINVAL;
        memcpy(s.data(), b, s.size());
    }
    return ZK_OK;
}

// one polynomial: u32 BE length, then the values (device -> bytes in `format`)
int write_poly(zk_ctx* c, const Fr* d, size_t len, int format, Out& o, Fr* d_tmp) {
    if (uint8_t* p = o.take(4)) put_be32(p, (uint32_t)len);
    uint8_t* p = o.take(len * fr_size());
    if (!p) return ZK_OK;
    if (format == ZK_SERDE_PROCESSED) {
        HIPCHK(c, hipMemcpyAsync(d_tmp, d, len * sizeof(Fr), hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(fr_from_mont_kernel, dim3(blocks_for(len)), dim3(256), 0, c->stream, d_tmp, len);
        d = d_tmp;
    }
    HIPCHK(c, hipMemcpyAsync(p, d, len * sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZK_OK;
}
int read_poly(zk_ctx* c, In& in, size_t len, int format, Fr* d, uint32_t* d_err) {
    const uint8_t* h = in.take(4);
    if (!h || get_be32(h) != len) return ZK_EINVAL;
    const uint8_t* p = in.take(len * fr_size());
    if (!p) return ZK_EINVAL;
    HIPCHK(c, hipMemcpyAsync(d, p, len * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    if (format != ZK_SERDE_RAW_BYTES_UNCHECKED)
        hipLaunchKernelGGL(fr_validate_kernel, dim3(blocks_for(len)), dim3(256), 0, c->stream, d, len, d_err);
    if (format == ZK_SERDE_PROCESSED) hipLaunchKernelGGL(fr_to_mont_kernel, dim3(blocks_for(len)), dim3(256), 0, c->stream, d, len);
    return ZK_OK;
}

}  // namespace

ZK_API(zk_vk_write, (zk_ctx* c, zk_pk h, int format, uint8_t* out, size_t cap, size_t* len), (c, h, format, out, cap, len)) {
    if (!c || !len || !format_ok(format)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    if (it->second->srs_gen != c->srs_gen || it->second->verify_only) return ZK_ESTATE;  // (no selector columns to write)
    *len = vk_size(it->second->lay, format);
    if (!out) return ZK_OK;
    if (cap < *len) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    Out o(out, cap);
    return write_vk(c, it->second, format, o);
}

// adopt the Rust host's VerifyingKey for a resident key: its commitments and selectors must be the key's own
// (ZK_EINVAL otherwise — a vk of another circuit or another SRS), and the host's transcript_repr replaces the stand-in
ZK_API(zk_vk_load, (zk_ctx* c, zk_pk h, const uint8_t* bytes, size_t len, int format, const uint64_t transcript_repr[4]), (c, h, bytes, len, format, transcript_repr)) {
    if (!c || !bytes || !format_ok(format)) return ZK_EINVAL;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        auto it = c->pks.find(h);
        if (it == c->pks.end()) return ZK_EINVAL;
        zk_pk_rec* pk = it->second;
        if (pk->srs_gen != c->srs_gen || pk->verify_only) return ZK_ESTATE;
        if (len != vk_size(pk->lay, format)) return ZK_EINVAL;
        In in{bytes, len};
        ParsedVk vk;
        int rc = parse_vk(pk->lay, in, format, &vk);
        if (rc) return rc;
        for (size_t i = 0; i < vk.fixed.size(); i++)
            if (memcmp(&vk.fixed[i], &pk->fixed_commit[i], sizeof(G1Affine)) != 0) return ZK_EINVAL;
        for (size_t i = 0; i < vk.perm.size(); i++)
            if (memcmp(&vk.perm[i], &pk->perm_commit[i], sizeof(G1Affine)) != 0) return ZK_EINVAL;
        if ((rc = ctx_bind(c))) return rc;
        std::vector<std::vector<uint8_t>> bits;
        if ((rc = selector_bits(c, pk, &bits))) return rc;
        if (bits != vk.selectors) return ZK_EINVAL;
    }
    return transcript_repr ? zk_pk_set_transcript_repr(c, h, transcript_repr) : ZK_OK;
}

// VerifyingKey::read: a verifying-only key from the zk_vk_write image of `params`' shape (its selector bits must be the
// layout's, as zk_pk_read demands); no SRS is needed
ZK_API(zk_vk_read, (zk_ctx* c, const zk_circuit_params* params, const uint8_t* bytes, size_t len, int format, const uint64_t transcript_repr[4], zk_pk* out), (c, params, bytes, len, format, transcript_repr, out)) {
    if (!c || !params || !bytes || !out || !format_ok(format)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    Layout lay;
    if (params->num_advice > 1 && 2 * (uint64_t)params->num_idle_gate_columns > params->num_advice) return ZK_ELAYOUT;
    if (!lay.init(*params)) return ZK_EINVAL;
    if (len != vk_size(lay, format)) return ZK_EINVAL;
    In in{bytes, len};
    ParsedVk vk;
    int rc = parse_vk(lay, in, format, &vk);
    if (rc) return rc;
    if (!layout_selectors_fit(lay, vk.selectors)) return ZK_ELAYOUT;
    return pk_make_verify_only(c, lay, vk.fixed, vk.perm, transcript_repr, out);
}

ZK_API(zk_pk_write, (zk_ctx* c, zk_pk h, int format, uint8_t* out, size_t cap, size_t* len), (c, h, format, out, cap, len)) {
    if (!c || !len || !format_ok(format)) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->pks.find(h);
    if (it == c->pks.end()) return ZK_EINVAL;
    zk_pk_rec* pk = it->second;
    if (pk->srs_gen != c->srs_gen || pk->verify_only) return ZK_ESTATE;
    const Layout& lay = pk->lay;
    *len = pk_size(lay, format);
    if (!out) return ZK_OK;
    if (cap < *len) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    const size_t n = lay.n, N = 4 * n;
    Out o(out, cap);
    if ((rc = write_vk(c, pk, format, o))) return rc;
    Fr* tmp = pk->h_ext;  // 4n elements of workspace, free between proofs
    if ((rc = write_poly(c, pk->l0_coset, N, format, o, tmp)) || (rc = write_poly(c, pk->l_last_coset, N, format, o, tmp)) ||
        (rc = write_poly(c, pk->l_active_coset, N, format, o, tmp)))
        return rc;
    // fixed columns in halo2's column order (table first), permutation columns as they are
    const std::vector<uint32_t> forder = vkrepr::halo2_fixed_order(lay);
    std::vector<uint32_t> sorder(lay.perm_cols.size());
    for (uint32_t i = 0; i < sorder.size(); i++) sorder[i] = i;
    auto slice = [&](const std::vector<Fr*>& v, const std::vector<uint32_t>& order, size_t len_each) -> int {
        if (uint8_t* p = o.take(4)) put_be32(p, (uint32_t)v.size());
        for (uint32_t i : order)
            if (int r = write_poly(c, v[i], len_each, format, o, tmp)) return r;
        return ZK_OK;
    };
    if ((rc = slice(pk->fixed_val, forder, n)) || (rc = slice(pk->fixed_poly, forder, n)) || (rc = slice(pk->fixed_coset, forder, N)) ||
        (rc = slice(pk->sigma_val, sorder, n)) || (rc = slice(pk->sigma_poly, sorder, n)) || (rc = slice(pk->sigma_coset, sorder, N)))
        return rc;
    return o.pos == *len && o.real ? ZK_OK : ZK_EINTERNAL;
}

ZK_API(zk_pk_read, (zk_ctx* c, const zk_circuit_params* params, const uint8_t* bytes, size_t len, int format, const uint64_t transcript_repr[4], zk_pk* out), (c, params, bytes, len, format, transcript_repr, out)) {
    if (!c || !params || !bytes || !out || !format_ok(format)) return ZK_EINVAL;
    uint64_t handle = 0;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        int rc = ctx_bind(c);
        if (rc) return rc;
        ctx_release_spares(c);
        Layout lay;
        if (params->num_advice > 1 && 2 * (uint64_t)params->num_idle_gate_columns > params->num_advice) return ZK_ELAYOUT;
        if (!lay.init(*params)) return ZK_EINVAL;
        if (c->srs_k != (int)lay.k) return ZK_ESTATE;
        if (len != pk_size(lay, format)) return ZK_EINVAL;
        const size_t n = lay.n, N = 4 * n, m = lay.perm_cols.size();
        In in{bytes, len};
        ParsedVk vk;
        if ((rc = parse_vk(lay, in, format, &vk))) return rc;
        zk_pk_rec* pk = new (std::nothrow) zk_pk_rec();
        if (!pk) return ZK_ENOMEM;
        pk->lay = lay;
        pk->srs_gen = c->srs_gen;
        pk->max_evals = (uint32_t)(lay.advice_queries.size() + lay.n_fix + lay.perm_cols.size() + 3 * lay.n_chunks + 5 * lay.n_lookups + 16);
        pk->fixed_commit = vk.fixed;
        pk->perm_commit = vk.perm;
        Dev d{c, pk};
        uint32_t* d_err = nullptr;
        auto fail = [&](int code) {
            hipStreamSynchronize(c->stream);
            hipFree(d_err);
            pk_destroy(pk);
            return code;
        };
        if (hipMalloc(&d_err, 4) != hipSuccess) return fail(ZK_ENOMEM);
        hipMemsetAsync(d_err, 0, 4, c->stream);
        pk->l0_coset = d.alloc(N);
        pk->l_last_coset = d.alloc(N);
        pk->l_active_coset = d.alloc(N);
        if (d.rc) return fail(d.rc);
        if ((rc = read_poly(c, in, N, format, pk->l0_coset, d_err)) || (rc = read_poly(c, in, N, format, pk->l_last_coset, d_err)) ||
            (rc = read_poly(c, in, N, format, pk->l_active_coset, d_err)))
            return fail(rc);
        // the file lists the fixed columns in halo2's column order (table first): column `pos` of a slice is the
        // engine's column order[pos]
        const std::vector<uint32_t> forder = vkrepr::halo2_fixed_order(lay);
        std::vector<uint32_t> sorder(m);
        for (uint32_t i = 0; i < m; i++) sorder[i] = i;
        auto slice = [&](std::vector<Fr*>& v, const std::vector<uint32_t>& order, size_t len_each) -> int {
            const uint8_t* hcount = in.take(4);
            if (!hcount || get_be32(hcount) != order.size()) return ZK_EINVAL;
            v.assign(order.size(), nullptr);
            for (uint32_t i : order) {
                Fr* p = d.alloc(len_each);
                if (d.rc) return d.rc;
                v[i] = p;
                if (int r = read_poly(c, in, len_each, format, p, d_err)) return r;
            }
            return ZK_OK;
        };
        if ((rc = slice(pk->fixed_val, forder, n)) || (rc = slice(pk->fixed_poly, forder, n)) || (rc = slice(pk->fixed_coset, forder, N)) ||
            (rc = slice(pk->sigma_val, sorder, n)) || (rc = slice(pk->sigma_poly, sorder, n)) || (rc = slice(pk->sigma_coset, sorder, N)))
            return fail(rc);
        if (in.pos != len) return fail(ZK_EINVAL);
        uint32_t herr = 0;
        if (hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            return fail(ZK_EHIP);
        if (herr) return fail(ZK_EINVAL);  // a field element >= r
        // the lookup path of this engine is specialised to halo2-lib's range table; the selector bits of the vk must be
        // the selector columns of the key
        {
            const uint32_t T = 1u << lay.lookup_bits;
            std::vector<Fr> tab(n);
            if (hipMemcpy(tab.data(), pk->fixed_val[lay.fx_table], n * sizeof(Fr), hipMemcpyDeviceToHost) != hipSuccess) return fail(ZK_EHIP);
            for (uint32_t r = 0; r < n; r++) {
                const Fr v = fe_from_mont(tab[r]);
                const uint32_t want = r < T ? r : 0;
                if (v.v[0] != want || v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) return fail(ZK_EINVAL);
            }
            std::vector<std::vector<uint8_t>> bits;
            if ((rc = selector_bits(c, pk, &bits))) return fail(rc == ZK_ESTATE ? ZK_EINVAL : rc);
            if (bits != vk.selectors) return fail(ZK_EINVAL);
            if (!layout_selectors_fit(lay, bits)) return fail(ZK_ELAYOUT);  // halo2 would have compressed these selectors differently
        }
        hipFree(d_err);
        d_err = nullptr;
        // the file's commitments must belong to the RESIDENT SRS: a key written under another SRS would be stamped with
        // this context's SRS generation and yield proofs that do not verify.  Spot check: the table column (never zero)
        // recommitted in both of its forms
        {
            G1Jac j1, j2;
            if ((rc = ctx_msm_device(c, pk->fixed_val[lay.fx_table], c->g_lagrange, n, &j1)) ||
                (rc = ctx_msm_device(c, pk->fixed_poly[lay.fx_table], c->g, n, &j2)))
                return fail(rc);
            const G1Affine a1 = g1_jac_to_affine_host(j1), a2 = g1_jac_to_affine_host(j2);
            if (memcmp(&a1, &pk->fixed_commit[lay.fx_table], sizeof(G1Affine)) != 0 || memcmp(&a2, &a1, sizeof(G1Affine)) != 0)
                return fail(ZK_EINVAL);
        }
        pk->transcript_repr = pk_standin_transcript_repr(pk);
        if ((rc = pk_alloc_workspace(c, pk))) return fail(rc);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail(ZK_EHIP);
        handle = c->next_handle++;
        c->pks[handle] = pk;
    }
    if (transcript_repr) {
        int rc = zk_pk_set_transcript_repr(c, handle, transcript_repr);
        if (rc) {
            zk_pk_free(c, handle);
            return rc;
        }
    }
    *out = handle;
    return ZK_OK;
}
