// g1_ntt.hip — the Lagrange basis of an SRS without its secret, and a randomized check of a resident SRS.
//
// halo2's `ParamsKZG::downsize(k)` truncates `g` to 2^k points and rebuilds `g_lagrange` with `g_to_lagrange`
// [RECALLED — poly/kzg/commitment.rs, arithmetic.rs `g_to_lagrange`]: an inverse FFT over G1 points, a scale by 1/n and a
// batch normalisation,
//     out[i] = [1/n] sum_j [w^-ij] g[j],   n = 2^k, w = the domain generator of k (fr_omega, the NTT's root).
// Here it is a radix-2 decimation-in-time transform over XYZZ points in global memory: a bit-reversing load, k stages of
// n / 2 butterflies (a, b) -> (a + [t] b, a - [t] b) and a normalisation to affine.  Each butterfly is one 254-bit scalar
// multiplication, so the stages are bound by Fq products (hundreds of point operations per butterfly against 512 B of
// traffic): plain passes over memory lose nothing to a tiled form.  Twiddles j = 0 are skipped, and 1/n rides on the last
// stage's multiplications.  The additions are g1x_add / g1x_dbl with their identity and doubling branches, so the result is
// exact for any input — the identity, repeated points, a + (-a) — not only for SRS-like ones.
//
// zk_srs_check multiplies nothing by the secret: it draws weights from a seed and tests, with two MSMs each, that g holds
// powers of the tau behind s_g2 (one pairing equation) and that g_lagrange is the Lagrange basis of g (an NTT of the weights).
//
// zk_srs_update is one ceremony contribution: g[i] -> [s^i] g[i] by one scalar multiplication per point, whose XYZZ result goes
// straight into the transform's scratch (the Lagrange basis has no pointwise update, so it is rebuilt by the same transform)
// and whose affine form is the new g[i].  The G2 step and the receipt are host code (srs_update.h).
#include <string.h>

#include "ctx.h"
#include "pairing.h"
#include "srs_update.h"

namespace {

__device__ __forceinline__ G1X g1x_of_affine(const G1Affine& p) {
    if (affine_is_identity(p)) return G1X::identity();
    G1X r;
    r.x = p.x;
    r.y = p.y;
    r.zz = Fq::one();
    r.zzz = Fq::one();
    return r;
}

__device__ __forceinline__ Fq fq_sel3(uint32_t d, const Fq& a, const Fq& b, const Fq& c) {
    Fq r;
#pragma unroll
    for (int q = 0; q < 8; q++) r.v[q] = d == 1 ? a.v[q] : d == 2 ? b.v[q] : c.v[q];
    return r;
}

// [s] p for a canonical s < 2^254: 2-bit windows from the top, the window's multiple of p ([1], [2] or [3]) picked by selects.
// Every lane of a wave runs the same 127 windows (two doublings and one addition each) whatever its own scalar is: with a
// bit at a time, a wave whose lanes hold different twiddles would run the addition of every bit that ANY lane has set.
__device__ G1X g1x_mul(const G1X& p, const Fr& s) {
    const G1X p2 = g1x_dbl(p);
    G1X p3 = p2;
    g1x_add(p3, p);
    G1X acc = G1X::identity();
#pragma unroll 1
    for (int w = 126; w >= 0; w--) {
        acc = g1x_dbl(g1x_dbl(acc));
        const uint32_t d = (s.v[w >> 4] >> ((w & 15) * 2)) & 3u;
        if (d) {
            G1X t;
            t.x = fq_sel3(d, p.x, p2.x, p3.x);
            t.y = fq_sel3(d, p.y, p2.y, p3.y);
            t.zz = fq_sel3(d, p.zz, p2.zz, p3.zz);
            t.zzz = fq_sel3(d, p.zzz, p2.zzz, p3.zzz);
            g1x_add(acc, t);
        }
    }
    return acc;
}

// a[i] = in[bitrev_k(i)] as XYZZ (the decimation-in-time order)
__global__ __launch_bounds__(256) void g1_ntt_load_kernel(const G1Affine* __restrict__ in, G1X* __restrict__ a, uint32_t log_n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (1u << log_n)) return;
    const uint32_t src = __brev(i) >> (32 - log_n);
    g1x_store(a + i, g1x_of_affine(affine_load(in + src)));
}

// stage s (half-size h = 2^s): butterfly t joins a[i0] and a[i1 = i0 + h], twiddle w_{2h}^-j = w^-(j n / 2h), j = t mod h.
// tw: w^e, e < n, standard Montgomery form (ctx_get_twiddles); w^-e = tw[n - e].  On the last stage both operands are also
// multiplied by 1/n (ninv: Montgomery, ninv_c: canonical)
__global__ __launch_bounds__(64) void g1_ntt_stage_kernel(G1X* __restrict__ a, const Fr* __restrict__ tw, uint32_t log_n, uint32_t s,
                                                          uint32_t last, Fr ninv, Fr ninv_c) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    const uint32_t n = 1u << log_n;
    if (t >= n / 2) return;
    const uint32_t h = 1u << s;
    const uint32_t j = t & (h - 1);
    const uint32_t i0 = ((t >> s) << (s + 1)) | j, i1 = i0 + h;
    G1X u = g1x_load(a + i0), v = g1x_load(a + i1);
    Fr sv = ninv_c;  // v's scalar
    if (j) {
        Fr w = fe_load(tw + (n - (j << (log_n - 1 - s))));
        if (last) w = fe_mul(w, ninv);
        sv = fe_from_mont(w);
    }
    // one call site of g1x_mul (q = 0: u, last stage only; q = 1: v, unless j = 0 on an inner stage)
#pragma unroll 1
    for (uint32_t q = last ? 0u : 1u; q < 2; q++) {
        if (q == 1 && !j && !last) break;
        G1X p = q ? v : u;
        p = g1x_mul(p, q ? sv : ninv_c);
        if (q) v = p;
        else u = p;
    }
    G1X x = u, y = u;
    g1x_add(x, v);
    v.y = fe_neg(v.y);  // -(X, Y, ZZ, ZZZ) = (X, -Y, ZZ, ZZZ); the identity (ZZ = 0) stays the identity
    g1x_add(y, v);
    g1x_store(a + i0, x);
    g1x_store(a + i1, y);
}

// XYZZ -> affine (x = X / ZZ, y = Y / ZZZ; the identity is (0, 0)), one inversion per point as srs_fixed_base_kernel does
__device__ __forceinline__ G1Affine g1x_to_affine(const G1X& p) {
    G1Affine r;
    if (p.is_identity()) {
        r.x = Fq::zero();
        r.y = Fq::zero();
    } else {
        const Fq t = fe_inv(p.zzz);    // 1/ZZZ
        const Fq u = fe_mul(p.zz, t);  // ZZ/ZZZ = 1/Z
        r.x = fe_mul(p.x, fe_sqr(u));
        r.y = fe_mul(p.y, t);
    }
    return r;
}
__global__ __launch_bounds__(64) void g1_ntt_affine_kernel(const G1X* __restrict__ a, G1Affine* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const G1Affine r = g1x_to_affine(g1x_load(a + i));
    fe_store(&out[i].x, r.x);
    fe_store(&out[i].y, r.y);
}

// The load of zk_srs_update: q = [s^i] g[i] (pw[i] = s^i, standard Montgomery form as launch_twiddles writes it), once per
// point for both of its uses — XYZZ into a[bitrev_k(i)], where the stage kernels expect the transform's input, and affine
// into out[i], the new monomial basis.  64-lane workgroups as the stage kernel, whose g1x_mul this is: the multiplication's
// live state (p, 2p, 3p, the accumulator and an addition's temporaries) decides the register count, and the inversion that
// follows starts from the product alone.
__global__ __launch_bounds__(64) void g1_update_kernel(const G1Affine* __restrict__ g, const Fr* __restrict__ pw, G1X* __restrict__ a,
                                                       G1Affine* __restrict__ out, uint32_t log_n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= (1u << log_n)) return;
    const G1X q = g1x_mul(g1x_of_affine(affine_load(g + i)), fe_from_mont(fe_load(pw + i)));
    g1x_store(a + (__brev(i) >> (32 - log_n)), q);
    const G1Affine r = g1x_to_affine(q);
    fe_store(&out[i].x, r.x);
    fe_store(&out[i].y, r.y);
}

bool host_affine_eq(const G1Affine& a, const G1Affine& b) { return a.x == b.x && a.y == b.y; }

}  // namespace

// The transform from its stage kernels on: a holds the n = 2^k inputs as XYZZ in bit-reversed order (g1_ntt_load_kernel's
// output, or g1_update_kernel's); d_out receives the affine result.  Returns with the stream drained.
static int g1_ntt_run(zk_ctx* c, G1X* a, uint32_t k, G1Affine* d_out) {
    const uint32_t n = 1u << k;
    const Fr* tw = nullptr;
    int rc = ctx_get_twiddles(c, k, &tw);
    if (rc) return rc;
    const Fr ninv = fe_inv(fr_from_u64(n));
    const Fr ninv_c = fe_from_mont(ninv);
    for (uint32_t s = 0; s < k; s++)
        hipLaunchKernelGGL(g1_ntt_stage_kernel, dim3((n / 2 + 63) / 64), dim3(64), 0, c->stream, a, tw, k, s, (uint32_t)(s + 1 == k),
                           ninv, ninv_c);
    hipLaunchKernelGGL(g1_ntt_affine_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, a, d_out, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = aud_sync(c, c->stream);
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        return ZK_EHIP;
    }
    return ZK_OK;
}

// halo2's g_to_lagrange between device buffers of 2^k affine points (in == out allowed); n XYZZ points of scratch for the call
int ctx_g1_to_lagrange(zk_ctx* c, const G1Affine* d_in, uint32_t k, G1Affine* d_out) {
    if (k < 1 || k > 24) return ZK_EINVAL;
    const uint32_t n = 1u << k;
    const Fr* tw = nullptr;
    int rc = ctx_get_twiddles(c, k, &tw);
    if (rc) return rc;
    G1X* a = nullptr;
    if (hipMalloc(&a, (size_t)n * sizeof(G1X)) != hipSuccess) {
        (void)hipGetLastError();
        return ZK_ENOMEM;
    }
    hipLaunchKernelGGL(g1_ntt_load_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_in, a, k);
    rc = g1_ntt_run(c, a, k, d_out);
    hipFree(a);
    return rc;
}

ZK_API(zk_g_to_lagrange, (zk_ctx* c, const uint64_t* g, uint32_t k, uint64_t* out), (c, g, k, out)) {
    if (!c || !g || !out || k < 1 || k > 24) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_bind(c);
    if (rc) return rc;
    const size_t n = (size_t)1 << k;
    G1Affine* d = nullptr;
    if (hipMalloc(&d, n * sizeof(G1Affine)) != hipSuccess) {
        (void)hipGetLastError();
        return ZK_ENOMEM;
    }
    uint32_t* d_err = (uint32_t*)c->small;
    uint32_t herr = 0;
    hipError_t e = hipMemcpyAsync(d, g, n * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, c->stream);
    if (e == hipSuccess) e = launch_g1_validate(d, (uint32_t)n, d_err, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = aud_sync(c, c->stream);
    if (e != hipSuccess) {
        hipFree(d);
        c->last_hip = (int)e;
        return ZK_EHIP;
    }
    if (herr) {  // a coordinate not below p, or a point off the curve ((0, 0) is the identity)
        hipFree(d);
        return ZK_EINVAL;
    }
    rc = ctx_g1_to_lagrange(c, d, k, d);
    if (rc == ZK_OK && (e = hipMemcpy(out, d, n * sizeof(G1Affine), hipMemcpyDeviceToHost)) != hipSuccess) {
        c->last_hip = (int)e;
        rc = ZK_EHIP;
    }
    hipFree(d);
    return rc;
}

ZK_API(zk_srs_downsize, (zk_ctx* c, uint32_t k), (c, k)) {
    if (!c) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0) return ZK_ESTATE;
    if (k < 1 || k > (uint32_t)c->srs_k) return ZK_EINVAL;
    int rc = ctx_bind(c);
    if (rc) return rc;
    ctx_release_spares(c);
    const size_t n = (size_t)1 << k;
    G1Affine *g = nullptr, *gl = nullptr;
    if (hipMalloc(&g, n * sizeof(G1Affine)) != hipSuccess || hipMalloc(&gl, n * sizeof(G1Affine)) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(g);
        return ZK_ENOMEM;
    }
    const hipError_t e = hipMemcpyAsync(g, c->g, n * sizeof(G1Affine), hipMemcpyDeviceToDevice, c->stream);
    rc = e == hipSuccess ? ctx_g1_to_lagrange(c, g, k, gl) : ZK_EHIP;
    if (e != hipSuccess) c->last_hip = (int)e;
    if (rc != ZK_OK) {
        hipFree(g);
        hipFree(gl);
        return rc;
    }
    return srs_install(c, k, g, gl);  // g2 / s_g2 stay; on failure the old SRS does too
}

// The randomized structure check.  rho_i = r^i and rho'_i = r'^i, r and r' the first two Fr draws of ChaCha20(seed): a wrong
// point survives a check only if r is a root of a nonzero polynomial of degree < n (probability below n / 2^253).
ZK_API(zk_srs_check, (zk_ctx* c, const uint8_t seed[32], uint32_t* flags), (c, seed, flags)) {
    if (!c || !seed || !flags) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0 || !c->g2_valid) return ZK_ESTATE;  // (after zk_srs_load: zk_srs_set_g2 first)
    int rc = ctx_bind(c);
    if (rc) return rc;
    const uint32_t k = (uint32_t)c->srs_k;
    const size_t n = (size_t)1 << k;
    ChaCha20Rng rng(seed);
    const Fr r0 = rng.next_fr(), r1 = rng.next_fr();
    Fr* d = nullptr;  // [rho | rho' | iNTT(rho')]
    if (hipMalloc(&d, 3 * n * sizeof(Fr)) != hipSuccess) {
        (void)hipGetLastError();
        return ZK_ENOMEM;
    }
    const G2A g2 = g2_from_raw(c->g2_raw), s_g2 = g2_from_raw(c->s_g2_raw);
    uint32_t f = 0;
    G1Jac A, B, L, M;
    // bit 0: A = sum rho_i g[i+1], B = sum rho_i g[i] (i < n - 1); g[i+1] = [tau] g[i] for all i makes A = [tau] B:
    // e(A, g2) = e(B, s_g2)
    launch_twiddles(d, r0, (uint32_t)n, c->stream);
    launch_twiddles(d + n, r1, (uint32_t)n, c->stream);
    rc = ctx_msm_device(c, d, c->g + 1, n - 1, &A);
    if (rc == ZK_OK) rc = ctx_msm_device(c, d, c->g, n - 1, &B);
    // bit 1: g_lagrange = M g with M_ij = w^-ij / n, so sum rho'_i g_lagrange[i] = sum_j (M^T rho')_j g[j] and M^T rho' = iNTT(rho')
    if (rc == ZK_OK) rc = ctx_ntt(c, d + n, n, d + 2 * n, k, true, false, n);
    if (rc == ZK_OK) rc = ctx_msm_device(c, d + n, c->g_lagrange, n, &L);
    if (rc == ZK_OK) rc = ctx_msm_device(c, d + 2 * n, c->g, n, &M);
    G1Affine g0;
    hipError_t e = hipSuccess;
    if (rc == ZK_OK && (e = hipMemcpy(&g0, c->g, sizeof(G1Affine), hipMemcpyDeviceToHost)) != hipSuccess) {
        c->last_hip = (int)e;
        rc = ZK_EHIP;
    }
    aud_sync(c, c->stream);
    hipFree(d);
    if (rc != ZK_OK) {
        ctx_msm_drain(c);
        return rc;
    }
    if (pairing_check(g1_jac_to_affine_host(B), g1_jac_to_affine_host(A), g2, s_g2)) f |= 1u;  // e(B, s_g2) == e(A, g2)
    if (host_affine_eq(g1_jac_to_affine_host(L), g1_jac_to_affine_host(M))) f |= 2u;
    // bit 2: g[0] = (1, 2) and g2 = the G2 generator, as in a ceremony's SRS and in ParamsKZG::setup
    G1Affine gen;
    gen.x = Fq::one();
    gen.y = fe_add(Fq::one(), Fq::one());
    uint8_t g2_gen[128];
    g2_to_raw(g2_generator(), g2_gen);
    if (host_affine_eq(g0, gen) && memcmp(c->g2_raw, g2_gen, 128) == 0) f |= 4u;
    *flags = f;
    return ZK_OK;
}

// One ceremony contribution.  Everything is built beside the resident SRS — the two new bases, the new s_g2, the receipt —
// and goes in through srs_install, so a failure at any point leaves the context as it was.  What depends on s: the host's
// `s` and the generator's state (cleared below on every path), the n powers on the device (zeroed on the stream before the
// buffer is freed), and the kernel argument of launch_twiddles, which lives in the runtime's argument buffer for the
// length of that launch, as zk_srs_setup's does.
ZK_API(zk_srs_update, (zk_ctx* c, const uint8_t seed[32], zk_srs_contribution* out), (c, seed, out)) {
    if (!c || !seed) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->srs_k < 0 || !c->g2_valid) return ZK_ESTATE;  // (after zk_srs_load: zk_srs_set_g2 first)
    int rc = ctx_bind(c);
    if (rc) return rc;
    const uint64_t aud0 = c->audit.violations;
    const uint32_t k = (uint32_t)c->srs_k;
    const size_t n = (size_t)1 << k;
    Fr s = srs_update_secret(seed);
    if (s.is_zero() || s == Fr::one()) {
        secure_zero(&s, sizeof(s));
        return ZK_EINVAL;
    }
    ctx_release_spares(c);
    G1Affine *g = nullptr, *gl = nullptr;
    Fr* pw = nullptr;
    G1X* a = nullptr;
    if (hipMalloc(&g, n * sizeof(G1Affine)) != hipSuccess || hipMalloc(&gl, n * sizeof(G1Affine)) != hipSuccess ||
        hipMalloc(&pw, n * sizeof(Fr)) != hipSuccess || hipMalloc(&a, n * sizeof(G1X)) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(g);
        hipFree(gl);
        hipFree(pw);
        secure_zero(&s, sizeof(s));
        return ZK_ENOMEM;
    }
    launch_twiddles(pw, s, (uint32_t)n, c->stream);
    hipLaunchKernelGGL(g1_update_kernel, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, c->stream, c->g, pw, a, g, k);
    hipError_t e = hipGetLastError();
    const hipError_t ez = hipMemsetAsync(pw, 0, n * sizeof(Fr), c->stream);  // the powers go before anything else can fail
    if (e == hipSuccess) e = ez;
    rc = e == hipSuccess ? g1_ntt_run(c, a, k, gl) : ZK_EHIP;
    if (e != hipSuccess) c->last_hip = (int)e;
    if (rc != ZK_OK) aud_sync(c, c->stream);  // (a successful transform has drained the stream itself)
    hipFree(a);
    hipFree(pw);  // zeroed by now
    G1Affine g1[2];  // g[1] before and after
    if (rc == ZK_OK && ((e = hipMemcpy(&g1[0], c->g + 1, sizeof(G1Affine), hipMemcpyDeviceToHost)) != hipSuccess ||
                        (e = hipMemcpy(&g1[1], g + 1, sizeof(G1Affine), hipMemcpyDeviceToHost)) != hipSuccess)) {
        c->last_hip = (int)e;
        rc = ZK_EHIP;
    }
    if (rc != ZK_OK) {
        hipFree(g);
        hipFree(gl);
        secure_zero(&s, sizeof(s));
        return rc;
    }
    uint8_t s_g2_new[128];
    srs_update_s_g2(c->s_g2_raw, s, s_g2_new);
    zk_srs_contribution rec;
    srs_contribution_make(g1[0], g1[1], s, &rec);
    secure_zero(&s, sizeof(s));
    if ((rc = srs_install(c, k, g, gl)) != ZK_OK) return rc;  // (the old SRS, its s_g2 and its keys stay; g and gl went with the new block)
    memcpy(c->s_g2_raw, s_g2_new, 128);
    if ((rc = aud_verdict(c, aud0, ZK_OK))) return rc;
    if (out) *out = rec;
    return ZK_OK;
}

ZK_API(zk_srs_contribution_check, (zk_ctx* c, const zk_srs_contribution* r, uint32_t* flags), (c, r, flags)) {
    if (!c || !r || !flags) return ZK_EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    uint32_t f = srs_contribution_flags(*r);
    if (c->srs_k >= 1) {
        int rc = ctx_bind(c);
        if (rc) return rc;
        G1Affine g1;
        HIPCHK(c, hipMemcpy(&g1, c->g + 1, sizeof(G1Affine), hipMemcpyDeviceToHost));
        if (host_affine_eq(g1, g1_from_words(r->after_g1))) f |= ZK_SRS_CONTRIB_RESIDENT;
    }
    *flags = f;
    return ZK_OK;
}
