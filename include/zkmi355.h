/*
 * zkmi355.h — C ABI of libzkmi355.so, the MI355X (gfx950) proving engine that
 * sits behind halo2_proofs::plonk::create_proof for the reference's
 * secp256r1-ECDSA circuit.
 *
 * Every entry point replaces a Rust routine of the (un-vendored) halo2_proofs /
 * halo2curves crates that the reference reaches from its three create_proof
 * call sites:
 *     halo2-circuits/src/ecc/ecdsa_p256.rs:366-373   (EvmTranscript + GWC, /prove_evm)
 *     halo2-circuits/src/ecc/ecdsa_p256.rs:416-423   (Blake2b + SHPLONK, /prove)
 *     halo2-circuits/src/ecc/ecdsa_p256.rs:555-562   (bench_secp256r1_ecdsa)
 * and from keygen at ecdsa_p256.rs:258-260.  The upstream routine replaced is
 * named on each declaration; INTEGRATION.md shows the Rust `extern "C"` shim.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every host buffer, the
 *     engine never keeps a host pointer past return;
 *   - memory images are those of the Rust types: Fr / Fq = 4 x u64 little-endian
 *     limbs in Montgomery form (R = 2^256); G1Affine = x || y (64 B), identity
 *     (0,0); G1 = Jacobian x || y || z (96 B), identity z = 0;
 *   - every function returns 0 on success or a negative ZK_E* code, never
 *     throws; outputs are untouched on error; no CPU fallback exists — a missing
 *     device is ZK_ENODEV;
 *   - a zk_ctx is bound to one HIP device and one stream and serialises its
 *     callers internally; use one context per worker thread / GPU;
 *   - the engine has no entropy source of its own: the seam and phase-level entry points are
 *     deterministic maps, and the one entry point that needs blinding values, zk_prove, expands the 32-byte seed the
 *     CALLER supplies with ChaCha20 (halo2's ChaCha20Rng stream and draw order) — the host draws that seed from its
 *     own RNG (the reference uses OsRng, ecdsa_p256.rs:362,412,550); a fixed or predictable seed forfeits zero-knowledge.
 */
#ifndef ZKMI355_H
#define ZKMI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_OK 0
#define ZK_EINVAL (-1)   /* bad size / argument / handle */
#define ZK_ENOMEM (-2)   /* device or host allocation failed */
#define ZK_EHIP (-3)     /* HIP runtime error (zk_last_hip_error) */
#define ZK_ENODEV (-4)   /* no usable gfx950 device */
#define ZK_ESTATE (-5)   /* missing prerequisite (SRS / key not loaded) */
#define ZK_EWITNESS (-6) /* witness violates the circuit (lookup input not in table): halo2's
                            Error::ConstraintSystemFailure */
#define ZK_EINTERNAL (-7) /* a C++ exception was stopped at the boundary (nothing is ever thrown across it), or — under ZK_OPT_STREAM_AUDIT — the
                            stream audit found an enqueue that is not ordered after the buffers it touches (zk_audit_report) */
#define ZK_ELAYOUT (-8)  /* zk_keygen / zk_pk_read: the selector columns do not fit the layout the key is built for — halo2's
                            compress_selectors would combine them differently (two used gate selectors that share no row, a used
                            selector that is never enabled, an "idle" one that is; or 2 * num_idle_gate_columns > num_advice:
                            the surplus never-enabled selectors would pair up in all-zero columns of their own): another vk
                            digest and other gates than the engine's closed form, so the key is refused rather than made to
                            prove something else */

typedef struct zk_ctx zk_ctx;
typedef uint64_t zk_poly; /* opaque device-resident vector of Fr; 0 is never valid */

#define ZK_BASIS_MONOMIAL 0 /* ParamsKZG::commit          (basis g)          */
#define ZK_BASIS_LAGRANGE 1 /* ParamsKZG::commit_lagrange (basis g_lagrange) */

/* ---- context ------------------------------------------------------------- */
int zk_device_count(void);
/* PCI address of a device ("0000:c1:00.0", cap >= 16): /sys/bus/pci/devices/<id>/{numa_node,local_cpulist} name its NUMA node —
 * an 8-GPU host binds each GPU's worker threads and staging buffers there (bench.py does) */
int zk_device_pci_bus_id(int device_id, char* out, size_t cap);
/* free and total device memory in bytes (hipMemGetInfo): a host sizes the number of resident proof pipelines by it (a k = 19
 * pipeline is ~ 5.3 GiB beside the first one's 6.4, docs in DESIGN.md section 2) */
int zk_device_mem_info(int device_id, size_t* free_bytes, size_t* total_bytes);
/* page-locked host memory for buffers handed to zk_poly_upload / zk_poly_upload_canonical (one DMA at the bus rate instead of a
 * staged copy out of pageable memory); NULL on failure */
void* zk_host_alloc(size_t bytes);
void zk_host_free(void* p);
int zk_ctx_create(int device_id, zk_ctx** out);
/* a further context on ctx's device that SHARES ctx's resident SRS (bases and window tables, read-only, as loaded at this
 * moment): one context per proof pipeline / host thread without a copy of the tables each.  Either context may later load
 * another SRS for itself; the shared memory is freed when its last user lets go (destroying `parent` first is fine). */
int zk_ctx_create_shared(zk_ctx* parent, zk_ctx** out);
void zk_ctx_destroy(zk_ctx* ctx);
const char* zk_strerror(int code);
int zk_last_hip_error(const zk_ctx* ctx); /* raw hipError_t of the last ZK_EHIP */
int zk_sync(zk_ctx* ctx);                 /* hipStreamSynchronize on the context stream */
/* tuning options (measurement tools, tests); value 0 restores the built-in choice.  The engine reads no
 * environment variables. */
#define ZK_OPT_MSM_WINDOW 1          /* signed window bits of the fixed-base MSM, 9..17; takes effect at the next SRS load */
#define ZK_OPT_MSM_BATCH 2           /* columns per fixed-base MSM pass, 1..256 (an SRS of 2^22 points or more runs one column per pass whatever is asked) */
#define ZK_OPT_NTT_MAX_RADIX_LOG2 3  /* largest radix of one NTT pass, as its log2: v = 1..11 (anything else is ZK_EINVAL).  Every value is
                                        honoured at every size the transforms accept (log_n <= 26), by every entry point that transforms
                                        (zk_ntt_bn254_fr, the zk_poly transforms, keygen, zk_prove, ...): a 2^log_n transform runs
                                        ceil(log_n / v) passes — 26 radix-2 passes at v = 1, log_n = 26 —, their radices as even as
                                        possible (the larger ones first: log_n = 22, v = 7 -> 2^6, 2^6, 2^5, 2^5), on the smallest LDS tile
                                        that holds 2^v: 2^9 elements for v <= 9, 2^10 for v = 10, 2^11 for v = 11; log_n <= v is ONE
                                        pass.  0 (default) plans by size: passes of at most 2^8 on the 2^9 tile up to log_n = 16
                                        (8 + 8), 2^9 on the 2^10 tile up to 18 (9 + 9), 2^10 on the 2^11 tile up to 20 (10 + 10), and at
                                        most 2^7 on the 2^9 tile above (21 = 7 + 7 + 7, 22 .. 26 four passes).  Same bytes whatever the
                                        value (tests/test_gpu_ntt_plans.py).  (A library built with another ZK_NTT_TILE_LOG than 9 keeps
                                        that one tile and clamps v to it.) */
#define ZK_OPT_GP_BATCH_INVERT 4     /* 1: grand products always take halo2's batch_invert form (the fallback path) */
#define ZK_OPT_MSM_TAIL_STREAM 5     /* where the MSM reduction tails run: 0 auto, 1 the context's side stream, 2 its main stream.
                                        Auto: the side stream while at most ZK_OPT_MSM_TAIL_MAIN_ABOVE contexts are ACTIVE on the
                                        device, the main stream beyond.  A context is active if it enqueued an MSM pass within the
                                        last 4 ms through ANY entry point (zk_prove, zk_commit, zk_commit_batch, zk_msm_srs,
                                        zk_msm_bn254, keygen): four host threads on the phase-level ABI are seen like four
                                        zk_prove calls.  The count is PROCESS-LOCAL — other processes on the same GPU are not seen:
                                        a host that runs several worker processes per device pins the regime with 1 / 2.
                                        Why it matters: the HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware
                                        queues (4 unless that environment variable of the HIP runtime says otherwise) and streams
                                        that share a queue run in order — with more than four streams busy some pipeline's kernels
                                        wait behind another's accumulation (DESIGN.md "Streams and hardware queues"; measured: 4
                                        pipelines 103.7 proofs/s on one stream each against 99.1 with a side stream each) */
#define ZK_OPT_MSM_TAIL_MAIN_ABOVE 6 /* the auto threshold above, 1..64; 0 restores the measured default (2, for the runtime's default
                                        of four hardware queues: two contexts x two streams fill them) */
#define ZK_OPT_BATCH_PASS_COLUMNS 7  /* zk_prove_batch: columns per MSM pass, 1..256; 0 = max(min(2 x batch, 8), the single prover's pass width).
                                         The lanes' MSM workspaces grow to that width on their next pass and KEEP it for the life of the context */
#define ZK_OPT_XFORM_STREAM 8        /* zk_prove: where a proof's column transforms (values -> coefficients -> extended coset) run:
                                        0 auto (beside the MSM passes on a stream of their own while this is the only active context
                                        of the process on the device — a lone proof —, in order on the main stream otherwise: see
                                        ZK_OPT_MSM_TAIL_STREAM on hardware queues), 1 always the side stream, 2 always the main stream */
#define ZK_OPT_MSM_STREAM 9          /* zk_prove: where a proof's MSM passes (sort head + accumulation) run: 0 auto (a stream of their own
                                        for a lone proof — with ZK_OPT_XFORM_STREAM's auto rule: main, tail, transform and MSM stream are
                                        the runtime's four hardware queues —, so that the glue kernels of the next phase do not queue
                                        behind an accumulation), 1 always that stream, 2 always the main stream */
#define ZK_OPT_MSM_T1 10             /* first kernel of the MSM reduction tail (the sum of a bucket's partial sums): 0 / 2 parts of <= 8 partial
                                        sums + a segmented tree (default), 1 one lane per bucket (a quarter fewer instructions, a dependent chain
                                        twice as long: measured equal under load, slower for a lone proof).  Same bytes either way */
#define ZK_OPT_STREAM_AUDIT 11       /* debug: 1 switches on the happens-before ledger of the context's streams (csrc/audit.h): every enqueue
                                        names the buffers it reads and writes, and one whose stream is not ordered after the buffer's last
                                        writer (or, for a write, its last readers) makes the entry point return ZK_EINTERNAL instead of ZK_OK —
                                        the class of bug that yields wrong proof bytes once in a thousand runs shows on the first run that takes
                                        the faulty path.  zk_audit_report tells what was found.  0 (default) switches it off; 2 = the
                                        audit's self-test: on, AND zk_prove takes a knowingly unordered path (its column transforms alternate
                                        between two streams per call without ordering their shared scratch — round 5's first form): every
                                        proof whose transforms come in more than one call must then return ZK_EINTERNAL */
#define ZK_OPT_STREAM_PRIORITY 12    /* experiment: dispatch priority of the context's MAIN stream — 0 normal (default), 1 high, 2 low
                                        (hipStreamCreateWithPriority).  Set it right after zk_ctx_create, before any other call: the stream
                                        is made again.  Pipelines of one device at DIFFERENT priorities do not share the chip evenly, so
                                        their chip-filling kernels stop ending together (docs/experiments.md) */
#define ZK_OPT_QUOTIENT_DOMAIN 13    /* zk_prove, circuits whose quotient has THREE pieces (two or more advice columns: deg h < 3n): h can be
                                        taken over three of the four cosets of halo2's extended domain — three n-point transforms per column
                                        instead of one 4n-point one, 3n quotient rows, a 3 x 3 solve per coefficient: the same pieces, the same
                                        proof bytes, a quarter of that work less.  0 (default) = auto: that route for columns of 2^16 rows or
                                        more (the proving server's k = 17 among them; the many-column rows below lose by it), 1 = always the
                                        whole extended domain (round 5's route), 2 = three cosets wherever h has three pieces.
                                        zk_prove_batch follows the same rule; the phase-level entry points (zk_coeff_to_extended, zk_quotient,
                                        zk_quotient_multi, zk_extended_to_coeff) always work on the whole domain in halo2's order */
#define ZK_OPT_ACTIVITY_HOLD 14      /* how a context inside zk_prove / zk_prove_batch counts for the automatic stream rules of the OTHER contexts
                                        of its device (ZK_OPT_MSM_TAIL_STREAM, ZK_OPT_XFORM_STREAM): 0 (default) active for the whole call — its
                                        quotient / evaluation / multi-open phases enqueue no MSM pass for longer than the 4 ms window under load,
                                        and the count dipped to two or three several times per proof; 1 = by its stamps alone (round 5's rule);
                                        2 = this context counts as active from now on, whatever entry points it uses, until the option is set
                                        to 0 or 1 — for the worker contexts of a host that drives the phase-level ABI (its calls between two MSM
                                        passes are invisible to the 4 ms window) */
int zk_ctx_set_option(zk_ctx* ctx, int option, int64_t value);

/* ---- fine-grained drop-in seam (host buffers in, host buffers out) --------
 * replaces halo2_proofs::arithmetic::best_multiexp(coeffs: &[Fr], bases: &[G1Affine]) -> G1 */
int zk_msm_bn254(zk_ctx* ctx, const uint64_t* scalars_mont /* n x 4 */,
                 const uint64_t* bases_affine_mont /* n x 8 */, size_t n,
                 uint64_t out_jacobian_mont[12]);
/* the same product over the RESIDENT SRS: replaces the body of ParamsKZG::commit (basis g: best_multiexp(&coeffs,
 * &self.g[..n])) / ParamsKZG::commit_lagrange (basis g_lagrange), where the Rust host knows by construction which
 * basis it multiplies against.  Only the n <= 2^k scalars are uploaded; the MSM runs on the window tables built at
 * zk_srs_setup / zk_srs_load / zk_srs_read.  (zk_msm_bn254 never guesses: it always uploads its bases.) */
int zk_msm_srs(zk_ctx* ctx, int basis /* ZK_BASIS_* */, const uint64_t* scalars_mont /* n x 4 */, size_t n,
               uint64_t out_jacobian_mont[12]);
/* replaces halo2_proofs::arithmetic::best_fft(a: &mut [Fr], omega: Fr, log_n: u32); in place,
 * natural order in and out */
int zk_ntt_bn254_fr(zk_ctx* ctx, uint64_t* a_mont /* 2^log_n x 4 */, const uint64_t omega_mont[4],
                    uint32_t log_n);

/* ---- SRS (ParamsKZG<Bn256>) ----------------------------------------------
 * replaces ParamsKZG::setup(k, ChaCha20Rng::from_seed(seed)) as run by halo2-base gen_srs(k)
 * (ecdsa_p256.rs:258,338,388): s = Fr::from_u512(first 64 keystream bytes);
 * g[i] = [s^i]G1, g_lagrange[i] = [L_i(s)]G1, both generated on the device. */
int zk_srs_setup(zk_ctx* ctx, uint32_t k, const uint8_t seed[32]);
/* adopt caller-supplied bases (the in-memory ParamsKZG of a Rust host: params.g / params.g_lagrange, n = 2^k points
 * each, affine Montgomery).  The arrays are copied; nothing is remembered about them.  Loading an SRS invalidates
 * every proving key made under the previous one (zk_prove / zk_vk_export return ZK_ESTATE for them). */
int zk_srs_load(zk_ctx* ctx, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange);
int zk_srs_export(zk_ctx* ctx, int basis, uint64_t* out_affine_mont /* n x 8 */, size_t first, size_t count);
int zk_srs_k(const zk_ctx* ctx); /* -1 if none */
/* how zk_commit runs over the resident SRS: signed window width and the number of windows (= bucket
 * additions per scalar; best_multiexp's `c` and `segments`, halo2_proofs arithmetic.rs [RECALLED]).
 * window_bits == 0: no window-multiple tables (k < 10).  For measurement (bench.py's ALU roofline). */
int zk_srs_msm_plan(const zk_ctx* ctx, uint32_t* window_bits, uint32_t* windows);

/* ---- the reference's files (SRS, proving key, verifying key) -------------------------------------------------
 * halo2_proofs `SerdeFormat` (helpers.rs): how field elements and points are laid out in a file.  The reference writes
 * and reads its keys with RawBytes (ecdsa_p256.rs:261-270, 339-343, 389-393); `Params::write` is RawBytes too. */
#define ZK_SERDE_PROCESSED 0           /* canonical little-endian field elements, compressed points */
#define ZK_SERDE_RAW_BYTES 1           /* in-memory Montgomery limbs, validated on read */
#define ZK_SERDE_RAW_BYTES_UNCHECKED 2 /* the same bytes, no validation on read */
/* replaces ParamsKZG::write_custom (halo2-base gen_srs writes ./params/kzg_bn254_{k}.srs): u32 LE k | g | g_lagrange | g2 |
 * s_g2.  out == NULL: only *len is set.  ZK_ESTATE after zk_srs_load until zk_srs_set_g2 supplies the G2 half. */
int zk_srs_write(zk_ctx* ctx, int format, uint8_t* out, size_t cap, size_t* len);
/* replaces ParamsKZG::read_custom (run by gen_srs on EVERY request in the reference, ecdsa_p256.rs:338,388): decodes
 * (decompresses / validates on the device), builds the window tables, keeps the SRS resident.  ZK_EINVAL on a
 * malformed file; the previously loaded SRS is gone in that case. */
int zk_srs_read(zk_ctx* ctx, const uint8_t* bytes, size_t len, int format);
/* G2 half of a ParamsKZG adopted with zk_srs_load (G2Affine memory images: x.c0 || x.c1 || y.c0 || y.c1, Montgomery) */
int zk_srs_set_g2(zk_ctx* ctx, const uint64_t g2[16], const uint64_t s_g2[16]);

/* ---- an SRS without its secret: downsize and check ------------------------------------------------------------------
 * replaces halo2's g_to_lagrange (arithmetic.rs [RECALLED]) on the caller's points: out[i] = [1/n] sum_j [w^-ij] g[j], n = 2^k,
 * 1 <= k <= 24, w the domain generator of k; affine Montgomery in and out, identity (0, 0).  Exact for any points (identity,
 * repeated and opposite points included); a coordinate not below p or a point off the curve is ZK_EINVAL. */
int zk_g_to_lagrange(zk_ctx* ctx, const uint64_t* g /* n x 8 */, uint32_t k, uint64_t* out /* n x 8 */);
/* replaces ParamsKZG::downsize(k): keeps the first 2^k points of g, rebuilds g_lagrange from them on the device (also for
 * k == zk_srs_k), keeps g2 / s_g2, builds the window tables.  The result is a NEW shared block: contexts made with
 * zk_ctx_create_shared before the call keep the old SRS and their keys; keys made here under the old SRS get ZK_ESTATE.
 * ZK_EINVAL: k < 1 or k > zk_srs_k; ZK_ESTATE: no SRS.  On any failure the resident SRS, its tables and its keys stay. */
int zk_srs_downsize(zk_ctx* ctx, uint32_t k);
/* ParamsKZG::read_custom + downsize(k) in one pass over the image, without building anything of the file's degree K: the
 * image is checked exactly as zk_srs_read checks it (an image zk_srs_read refuses is refused here too), streamed through a
 * fixed staging buffer, and only the degree-k SRS stays.  ZK_EINVAL also for k < 1 or k > K; otherwise zk_srs_read's rules. */
int zk_srs_read_downsize(zk_ctx* ctx, const uint8_t* bytes, size_t len, int format, uint32_t k);
/* randomized structure check of the resident SRS, weights drawn from ChaCha20(seed).  *flags gets one bit per check passed:
 *   ZK_SRS_CHECK_POWERS      g[i+1] = [tau] g[i] with s_g2 = [tau] g2 (two MSMs and one pairing equation)
 *   ZK_SRS_CHECK_LAGRANGE    g_lagrange is the Lagrange basis of g (an NTT and two MSMs)
 *   ZK_SRS_CHECK_GENERATORS  g[0] is the G1 generator (1, 2) and g2 the G2 generator
 * A failed check is a verdict (ZK_OK), not an error.  ZK_ESTATE: no SRS, or no G2 half (zk_srs_load without zk_srs_set_g2). */
#define ZK_SRS_CHECK_POWERS 1u
#define ZK_SRS_CHECK_LAGRANGE 2u
#define ZK_SRS_CHECK_GENERATORS 4u
int zk_srs_check(zk_ctx* ctx, const uint8_t seed[32], uint32_t* flags);

/* ---- one ceremony contribution to the resident SRS ------------------------------------------------------------------
 * The seed setup's secret is public and a ceremony file has to be trusted; zk_srs_update is the step that makes either
 * one's own: it multiplies a fresh secret s into the resident SRS and forgets it.  With tau the (unknown) secret so far,
 *   g[i] -> [s^i] g[i],  g_lagrange -> g_to_lagrange(g) (halo2's rule, one G1 transform on the device),  s_g2 -> [s] s_g2,
 * so the new secret is s tau: unknown as long as ONE contributor of the chain discarded theirs, even when the chain starts
 * at the seed-0 setup.  g2 stays.
 * s is the first Fr draw of ChaCha20Rng::from_seed(seed), zk_srs_setup's rule.  The engine has no entropy of its own: the
 * caller draws the 32 bytes from the operating system for this one call and discards them (as for zk_prove's seed) — who
 * keeps the seed keeps s.  The engine clears its own copies of s, on the host and on the device, before it returns.  The
 * call is deterministic: the same resident SRS and seed give the same bytes.
 * The result is a NEW shared block installed as zk_srs_downsize installs its own: window tables rebuilt, keys made under
 * the old SRS answer ZK_ESTATE, contexts made with zk_ctx_create_shared before the call keep the old SRS and their keys.
 * ZK_EINVAL: NULL ctx / seed, or a seed whose s is 0 or 1; ZK_ESTATE: no SRS, or no G2 half (zk_srs_load without
 * zk_srs_set_g2).  On any failure the resident SRS, its tables, s_g2 and its keys are what they were.
 * out (may be NULL; untouched on error) receives the receipt of the step. */
typedef struct {
    uint64_t before_g1[8]; /* g[1] of the SRS the step started from (affine Montgomery) */
    uint64_t after_g1[8];  /* g[1] after it = [s] before_g1 */
    uint64_t s_g1[8];      /* [s] G1 generator */
    uint64_t s_g2[16];     /* [s] G2 generator, zk_srs_set_g2's image */
} zk_srs_contribution;
int zk_srs_update(zk_ctx* ctx, const uint8_t seed[32], zk_srs_contribution* out);
/* checks a receipt on the host (three pairing equations); *flags gets one bit per check passed.  A bad receipt is a verdict
 * (ZK_OK with bits clear), never an error; ZK_EINVAL only for NULL arguments.  A receipt with a coordinate not below p, a
 * point off its curve (for s_g2: outside the order-r subgroup) or an identity point gets no bit but RESIDENT.
 * What a receipt is: a knowledge-of-exponent style proof, not a Schnorr proof — nobody can make the pair (s_g1, s_g2) with
 * SAME_SECRET without knowing s (the knowledge-of-exponent assumption), and LINKS ties that s to the step before_g1 ->
 * after_g1.  It is not bound to a contributor's name or to a transcript.  What it pins: a receipt with all four bits plus
 * zk_srs_check == 7 on the resulting SRS shows tau' = s tau — the check shows powers of ONE tau' that match s_g2 and the
 * Lagrange basis, and LINKS fixes g[1] = [tau'] G1 = [s] before_g1.  A chain is checked receipt by receipt, each before_g1
 * being the previous after_g1. */
#define ZK_SRS_CONTRIB_SAME_SECRET 1u /* e(s_g1, G2) == e(G1, s_g2): one s in both groups */
#define ZK_SRS_CONTRIB_LINKS       2u /* e(after_g1, G2) == e(before_g1, s_g2) */
#define ZK_SRS_CONTRIB_NONTRIVIAL  4u /* all points on their curves; s_g1 neither the identity nor the generator */
#define ZK_SRS_CONTRIB_RESIDENT    8u /* after_g1 is g[1] of the context's resident SRS (clear if it has none) */
int zk_srs_contribution_check(zk_ctx* ctx, const zk_srs_contribution* c, uint32_t* flags);
/* a chain of receipts in one launch on the device, one receipt per lane: flags[i] is what zk_srs_contribution_check gives for
 * c[i] (RESIDENT included; clear everywhere without a resident SRS, which the call does not need), plus CHAINED, which the host
 * adds.  Each lane tests its four points and walks its own s_g2 once through the Miller loop for both equations (csrc/pairing.h
 * contribution_check_lanes).  A bad receipt is a verdict, never an error.
 * ZK_EINVAL: NULL arguments, count == 0 or > ZK_SRS_CONTRIB_BATCH_MAX.  flags is untouched on every error. */
#define ZK_SRS_CONTRIB_CHAINED 16u /* i == 0, or before_g1 equals receipt i-1's after_g1 byte for byte */
#define ZK_SRS_CONTRIB_BATCH_MAX 4096
int zk_srs_contribution_check_batch(zk_ctx* ctx, size_t count, const zk_srs_contribution* c, uint32_t* flags /* count */);

/* ---- resident polynomials -------------------------------------------------- */
int zk_poly_alloc(zk_ctx* ctx, size_t n, zk_poly* out);
/* the handle dies; the memory is parked in the context (a few vectors, at most 2 GiB) for the next zk_poly_alloc of the same
 * length, because hipFree waits for the whole device — a host that allocates and frees around every request would otherwise
 * stall every other context of the GPU once per request */
int zk_poly_free(zk_ctx* ctx, zk_poly p);
/* Hand-over of a resident vector between two contexts of one device, no copy and no cross-context lock: the owner detaches
 * (its stream is drained first; the handle dies, a process-wide token is returned), the new owner attaches (new handle).  A
 * loader context with its own stream and host thread uploads the next request's columns while the proving context is inside
 * zk_prove.  A detached vector belongs to nobody until it is attached (ZK_EINVAL: unknown token, or another device). */
int zk_poly_detach(zk_ctx* ctx, zk_poly p, uint64_t* token);
int zk_poly_attach(zk_ctx* ctx, uint64_t token, zk_poly* out);
/* Frees a detached vector that will never be attached (the loader failed between staging and adoption, the target context
 * is gone): a token that is neither attached nor discarded keeps its device memory for the life of the process. */
int zk_poly_discard(uint64_t token);
int zk_poly_len(zk_ctx* ctx, zk_poly p, size_t* out);
int zk_poly_upload(zk_ctx* ctx, zk_poly p, const uint64_t* host_mont, size_t n);
int zk_poly_download(zk_ctx* ctx, zk_poly p, uint64_t* host_mont, size_t n);
int zk_poly_copy(zk_ctx* ctx, zk_poly dst, zk_poly src);
/* rows [first, first + count) from the host: the blinding rows a host appends to a column the device made (halo2's provers push
 * `blinding_factors` random rows onto a', s' and every z before committing), without shipping the column.  count == 0 is
 * allowed (nothing is written; first <= n still holds); first + count > n is ZK_EINVAL and the vector is unchanged */
int zk_poly_upload_range(zk_ctx* ctx, zk_poly p, size_t first, const uint64_t* host_mont, size_t count);
/* dst[dst_first ..] = src[src_first .. src_first + count) (the h pieces: n-coefficient slices of the quotient).  count == 0 is
 * allowed; a range that leaves either vector is ZK_EINVAL.  dst may be src when the two ranges are disjoint; overlapping ranges of
 * one vector (count > 0) are ZK_EINVAL — there is no memmove form.  On ZK_EINVAL nothing is written */
int zk_poly_copy_range(zk_ctx* ctx, zk_poly dst, size_t dst_first, zk_poly src, size_t src_first, size_t count);
/* out = sum_j coeffs[j] * in[j] - (sub_low[0] + sub_low[1] X + .. + sub_low[n_low - 1] X^(n_low - 1)), n_low <= 8 (0: nothing
 * subtracted; vectors shorter than n_low: only the coefficients they have, the first n, are subtracted); count >= 1 inputs, which
 * may repeat; all vectors of one length, out none of the inputs (ZK_EINVAL): the linear combinations of the multi-open provers — GWC's
 * sum_i v^i (p_i(X) - e_i) (n_low = 1), SHPLONK's sum_j y^j (P_j(X) - R_j(X)) with the remainders R_j of degree < |rotation set| —
 * and h(X) = sum_i x^(n i) h_i(X) */
int zk_poly_lincomb(zk_ctx* ctx, zk_poly out, const zk_poly* in, const uint64_t* coeffs_mont /* count x 4 */, size_t count,
                    const uint64_t* sub_low_mont /* n_low x 4 */, size_t n_low);

/* replaces ParamsKZG::commit / commit_lagrange (MSM against the resident SRS) + to_affine */
int zk_commit(zk_ctx* ctx, zk_poly p, int basis, uint64_t out_affine_mont[8]);
/* the same for `count` polynomials of one length: the columns share MSM passes (one bucket set per column, one
 * accumulation launch for several columns) — how create_proof commits its advice columns, (a', s'), grand
 * products and quotient pieces.  out: count x 8 limbs. */
int zk_commit_batch(zk_ctx* ctx, const zk_poly* polys, size_t count, int basis, uint64_t* out_affine_mont);
/* replaces EvaluationDomain::lagrange_to_coeff (in place: iNTT, x 1/n) */
int zk_lagrange_to_coeff(zk_ctx* ctx, zk_poly p);
/* replaces EvaluationDomain::coeff_to_lagrange (in place) */
int zk_coeff_to_lagrange(zk_ctx* ctx, zk_poly p);
/* replaces EvaluationDomain::coeff_to_extended: dst (2^ext_k) = NTT of zero-extended src scaled by zeta^i */
int zk_coeff_to_extended(zk_ctx* ctx, zk_poly src, zk_poly dst_ext);
/* replaces EvaluationDomain::extended_to_coeff: in place on a 2^ext_k vector; first n_out coefficients valid */
int zk_extended_to_coeff(zk_ctx* ctx, zk_poly ext, size_t n_out);
/* replaces arithmetic::eval_polynomial(poly, x) */
int zk_eval(zk_ctx* ctx, zk_poly p, const uint64_t x_mont[4], uint64_t out_mont[4]);
/* `count` >= 1 evaluations in one call: out_mont[4 i ..] = polys[i](points_mont[4 i ..]), each bit-identical to zk_eval of its pair.
 * It is the whole-proof provers' batched evaluation (one launch and one wait per 64 pairs; further pairs take further launches
 * inside the call), so a phase-driving host reads all opened values of a proof - of N circuits' columns - with one call instead of
 * one zk_eval and one wait each.  Handles may repeat (a polynomial opened at several rotations).  That launch takes ONE length:
 * every polynomial must have the same number of coefficients (ZK_EINVAL otherwise, as for count == 0, a bad handle or a NULL
 * argument); out_mont is written only when every pair has been evaluated. */
int zk_eval_batch(zk_ctx* ctx, const zk_poly* polys, const uint64_t* points_mont /* count x 4 */, size_t count,
                  uint64_t* out_mont /* count x 4 */);
/* replaces arithmetic::kate_division(p, z): q = (p - p(z)) / (X - z).  q has p's length (its top coefficient is 0: the
 * quotient is one coefficient shorter); q may be p (in place).  The multi-open provers (GWC / SHPLONK) divide with it. */
int zk_kate_division(zk_ctx* ctx, zk_poly p, const uint64_t z_mont[4], zk_poly q);

/* ---- keygen / create_proof ---------------------------------------------------
 * The config row that selects the column shape: reference CircuitParams
 * (halo2-circuits/src/ecc/ecdsa_p256.rs:44-55; rows in src/configs/bench_ecdsa.config). */
typedef struct {
    uint32_t k;                 /* "degree" */
    uint32_t num_advice;
    uint32_t num_lookup_advice;
    uint32_t num_fixed;
    uint32_t lookup_bits;
    uint32_t num_idle_gate_columns; /* trailing gate columns whose selector is never enabled (at most half of num_advice):
                                       halo2's selector compression puts the t-th such selector into the fixed column of
                                       gate t — no column of its own — and replaces the pair by q (2 - q) / q (1 - q) */
    uint32_t num_instance_columns;  /* 0, or 1: ONE instance column for the circuit's public inputs, made after the chips'
                                       columns and equality-enabled — the LAST permutation column, queried at rotation 0.  Zero
                                       (what aggregate-initialised and zero-filled callers get) is the reference's circuit.
                                       Anything above 1 is ZK_EINVAL.  See "public inputs" below */
} zk_circuit_params;
typedef uint64_t zk_pk; /* opaque: proving key + verifying key + prover workspace, device resident */

#define ZK_TRANSCRIPT_BLAKE2B 0 /* Blake2bWrite<_, G1Affine, Challenge255<_>>  (ecdsa_p256.rs:415) */
#define ZK_TRANSCRIPT_EVM 1     /* snark-verifier EvmTranscript (Keccak-256)   (ecdsa_p256.rs:365) */
#define ZK_SCHEME_DEFAULT 0     /* SHPLONK for Blake2b, GWC for EVM — the reference's pairings */
#define ZK_SCHEME_GWC 1         /* ProverGWC     (ecdsa_p256.rs:368) */
#define ZK_SCHEME_SHPLONK 2     /* ProverSHPLONK (ecdsa_p256.rs:418) */

/* replaces keygen_vk + keygen_pk (ecdsa_p256.rs:259-260) for a synthesized circuit: `fixed_canonical`
 * holds the fixed columns (n_fix x n x 4 limbs, canonical integers, column order: constants, range
 * table, selectors); `copies` the copy constraints as (perm_col_a, row_a, perm_col_b, row_b) with
 * permutation columns ordered [constants..., gate advice..., lookup advice..., instance (if the shape has one)] and
 * rows below the usable n - 7.  Needs the SRS of k. */
int zk_keygen(zk_ctx* ctx, const zk_circuit_params* params, const uint64_t* fixed_canonical /* n_fixed_columns x n x 4 */,
              size_t n_fixed_columns /* must equal the shape's fixed-column count: ZK_EINVAL otherwise */,
              const uint32_t* copies, size_t n_copies, zk_pk* out);
/* the vk digest every transcript starts with (halo2 `vk.transcript_repr`: Blake2b-512 of the pinned vk's Debug rendering,
 * reduced mod r): zk_keygen / zk_pk_read compute halo2's own value (csrc/vkrepr.h; pinned by the reference's k = 17 literal,
 * proving-server/P256Verifier.yul:34) for every shape, never-enabled gate columns included (bench_ecdsa.config rows k <= 13:
 * their combined selectors are rendered as compress_selectors builds them; no known answer exists for those rows).  A host
 * that knows better sets its value here (Montgomery image). */
int zk_pk_set_transcript_repr(zk_ctx* ctx, zk_pk pk, const uint64_t transcript_repr_mont[4]);
int zk_pk_free(zk_ctx* ctx, zk_pk pk);
/* the VerifyingKey half: commitments (affine Montgomery) and transcript_repr; counts = {n_fixed, n_perm} */
int zk_vk_export(zk_ctx* ctx, zk_pk pk, uint64_t* fixed_commitments, uint64_t* perm_commitments,
                 uint64_t transcript_repr[4], uint32_t counts[2]);
/* replaces VerifyingKey::write (ecdsa_p256.rs:266-270): u32 BE k | u32 BE #fixed | fixed commitments | permutation
 * commitments | selector bits.  out == NULL: only *len is set. */
int zk_vk_write(zk_ctx* ctx, zk_pk pk, int format, uint8_t* out, size_t cap, size_t* len);
/* adopts the Rust host's VerifyingKey (a VerifyingKey::write image) for a resident key: ZK_EINVAL unless its commitments
 * and selectors are the key's own; `transcript_repr` (may be NULL) is then what every transcript starts with. */
int zk_vk_load(zk_ctx* ctx, zk_pk pk, const uint8_t* vk_bytes, size_t len, int format, const uint64_t transcript_repr_mont[4]);
/* replaces ProvingKey::write (ecdsa_p256.rs:261-265): vk | l0 | l_last | l_active_row | fixed values / polys / cosets |
 * permutation values / polys / cosets (k=17: 336 MiB, k=19: 768 MiB in RawBytes).  out == NULL: only *len is set. */
int zk_pk_write(zk_ctx* ctx, zk_pk pk, int format, uint8_t* out, size_t cap, size_t* len);
/* replaces ProvingKey::read::<_, ECDSACircuit<Fr>> (ecdsa_p256.rs:339-343, 389-393 — on every request there, once
 * here): the key material comes from the file image, the column shape from `params` (what `ECDSACircuit::configure`
 * tells halo2), transcript_repr from the caller (NULL: computed as zk_keygen does).  Needs the SRS of params->k. */
int zk_pk_read(zk_ctx* ctx, const zk_circuit_params* params, const uint8_t* bytes, size_t len, int format,
               const uint64_t transcript_repr_mont[4], zk_pk* out);
/* the column shape of a key, for a host that drives the phases itself:
 * out = {k, extended k, #advice columns, #fixed columns, #permutation columns (the instance column included), #permutation
 * chunks, #lookups, #h pieces} */
int zk_pk_shape(zk_ctx* ctx, zk_pk pk, uint32_t out[8]);
/* instance columns of the key's shape: 0 or 1 */
int zk_pk_num_instance_columns(zk_ctx* ctx, zk_pk pk, uint32_t* out);
/* replaces plonk::evaluation::Evaluator::evaluate_h — and, with divide != 0, the EvaluationDomain::divide_by_vanishing_poly
 * that follows it in create_proof — for a Rust host that keeps halo2's own prover flow and off-loads phase by phase (the
 * [patch] route of INTEGRATION.md).  Every operand is a resident vector over the extended coset (2^(k+2) elements, as
 * zk_coeff_to_extended makes them): the advice columns, the permutation grand products z (one per chunk), and per lookup
 * the triple (permuted input a', permuted table s', product zL) — lookup_ext holds 3 * n_lookups handles in that order.
 * The fixed / sigma / l_0 / l_last / l_active cosets are the key's own.  beta, gamma, y: Montgomery images (theta does not
 * enter: every lookup of this circuit family is a single expression).  out_ext receives h on the extended coset
 * (zk_extended_to_coeff then gives the h pieces); it must not alias an input. */
int zk_quotient(zk_ctx* ctx, zk_pk pk, const zk_poly* advice_ext, size_t n_advice, const zk_poly* perm_z_ext, size_t n_chunks,
                const zk_poly* lookup_ext, size_t n_lookups, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t y[4],
                int divide, zk_poly out_ext);
/* zk_quotient for ONE proof over n_circuits circuits of the key (1 .. ZK_PROVE_MULTI_MAX), with their public inputs where the key has
 * the instance column: the h of zk_prove_public / zk_prove_multi / zk_prove_multi_public.  Every handle array is circuit-major,
 * circuit 0 first: advice_ext n_circuits x n_advice, perm_z_ext n_circuits x n_chunks, lookup_ext n_circuits x 3 n_lookups (per
 * lookup a', s', zL), instance_ext n_circuits - circuit c's instance polynomial on the extended coset.  The y-combination runs on
 * through the circuits in order into ONE h, h = sum_c y^(T (N - 1 - c)) h_c with T the terms of one circuit: circuit 0's pass stores,
 * every later pass adds its own terms (the accumulating pass of zk_prove_multi; no linear combination of N quotients is formed);
 * `divide` applies to every pass.  n_circuits == 1 on a key without the column gives zk_quotient's bytes.
 * The instance vector of a circuit is built with the calls above: zk_poly_alloc(n) and a zeroed host column with the Montgomery
 * values in rows 0 .. m - 1 through zk_poly_upload (or canonical integers through zk_poly_upload_canonical; zk_poly_upload_range
 * writes rows 0 .. m - 1 of a vector that is already zero) - that Lagrange vector is zk_permutation_product_public's `instance`;
 * a copy of it through zk_lagrange_to_coeff and zk_coeff_to_extended is the handle of instance_ext.  Nothing of it is blinded.
 * ZK_EINVAL: n_circuits outside 1 .. ZK_PROVE_MULTI_MAX, a count that is not the shape's, a handle that is not a 2^(k+2) vector,
 * out_ext among the inputs (checked before anything is launched), instance_ext != NULL for a key without the column or NULL for
 * a key with it (the whole-proof rule, halo2's InvalidInstances); ZK_ESTATE: a verifying-only key, or a key whose SRS was replaced.
 * zk_quotient itself keeps returning ZK_EINVAL on a key with the column. */
int zk_quotient_multi(zk_ctx* ctx, zk_pk pk, size_t n_circuits, const zk_poly* advice_ext /* n_circuits x n_advice */, size_t n_advice,
                      const zk_poly* instance_ext /* n_circuits, or NULL */, const zk_poly* perm_z_ext /* n_circuits x n_chunks */,
                      size_t n_chunks, const zk_poly* lookup_ext /* n_circuits x 3 n_lookups */, size_t n_lookups, const uint64_t beta[4],
                      const uint64_t gamma[4], const uint64_t y[4], int divide, zk_poly out_ext);
/* ---- the provers between the commitments, for a host that drives the phases itself (its transcript, its RNG, its blinding:
 * examples/prove_host_phases.cpp builds a whole proof from these and the calls above) ------------------------------------------
 * replaces plonk::lookup::prover's `permute_expression_pair` for every lookup of the key (halo2_proofs
 * plonk/lookup/prover.rs, reached from create_proof, ecdsa_p256.rs:366-373): from the advice columns (Lagrange values) the
 * permuted input a' and permuted table s' of each lookup, rows 0 .. n - 8 (the usable rows; the host writes the 7 rows behind
 * them — its blinding — with zk_poly_upload_range).  ZK_EWITNESS: an input is not in the table. */
int zk_lookup_permute(zk_ctx* ctx, zk_pk pk, const zk_poly* advice, size_t n_advice, zk_poly* permuted_input /* out, n_lookups */,
                      zk_poly* permuted_table /* out, n_lookups */, size_t n_lookups);
/* replaces lookup::prover `commit_product`: the grand product zL of every lookup (rows 0 .. n - 7; the host blinds the last 6) */
int zk_lookup_product(zk_ctx* ctx, zk_pk pk, const zk_poly* advice, size_t n_advice, const zk_poly* permuted_input,
                      const zk_poly* permuted_table, size_t n_lookups, const uint64_t beta[4], const uint64_t gamma[4],
                      zk_poly* z_out /* n_lookups */);
/* replaces plonk::permutation::prover `commit`: the grand products z of the permutation argument, one per chunk of columns
 * (zk_pk_shape), chunk c starting from chunk c - 1's value at the last usable row (rows 0 .. n - 7; the host blinds the rest) */
int zk_permutation_product(zk_ctx* ctx, zk_pk pk, const zk_poly* advice, size_t n_advice, const uint64_t beta[4],
                           const uint64_t gamma[4], zk_poly* z_out /* n_chunks */, size_t n_chunks);
/* the same for a key WITH the instance column (zk_circuit_params.num_instance_columns = 1): `instance` is a resident vector of n
 * rows, Lagrange values as Montgomery images - the public inputs in rows 0 .. m - 1, zero in every other row (how to build it:
 * zk_quotient_multi above) - and enters the product as the LAST permutation column, unblinded, as in zk_prove_public.  The chunks
 * and the start of chunk c from chunk c - 1 are zk_permutation_product's.  One call serves one circuit: a host proving N circuits
 * calls it once per circuit with that circuit's advice and instance vector.  For a key WITHOUT the column `instance` must be 0 and
 * the result is zk_permutation_product's, byte for byte.  ZK_EINVAL beyond zk_permutation_product's cases: no instance vector for a
 * key with the column, one for a key without (the whole-proof rule, halo2's InvalidInstances), a vector of another length, the
 * instance vector among z_out (checked before anything is launched).  zk_permutation_product itself keeps returning ZK_EINVAL on a
 * key with the column. */
int zk_permutation_product_public(zk_ctx* ctx, zk_pk pk, const zk_poly* advice, size_t n_advice, zk_poly instance, const uint64_t beta[4],
                                  const uint64_t gamma[4], zk_poly* z_out /* n_chunks */, size_t n_chunks);
/* a copy of one of the key's own polynomials (coefficient form, n coefficients) into the caller's vector: the fixed columns
 * (index in QUERY order: constants, lookup table, selector columns — the order of the fixed evaluations in a proof) and the
 * permutation polynomials sigma (permutation-column order) that create_proof evaluates at x and opens (`pk.fixed_polys`,
 * `pk.permutation.polys` of halo2's ProvingKey) */
#define ZK_PK_FIXED_POLY 0
#define ZK_PK_SIGMA_POLY 1
int zk_pk_export_poly(zk_ctx* ctx, zk_pk pk, int which, size_t index, zk_poly dst);
/* replaces the n `Fr::random(&mut rng)` draws of plonk::vanishing::prover `commit` (the random polynomial): coefficient i =
 * the Fr::random of ChaCha20 block first_block + i under `chacha_key` — what rand_chacha's ChaCha20Rng::from_seed(key) yields
 * for its draws first_block .. first_block + n - 1 when every draw is an Fr::random (as in create_proof).  The RNG stays the
 * host's: it hands over key and position and skips n draws; a host with another RNG uploads the column. */
int zk_random_poly(zk_ctx* ctx, const uint8_t chacha_key[32], uint64_t first_block, zk_poly out);
/* bytes zk_prove will write for this key / transcript / scheme (what `transcript.finalize().len()` is in
 * the reference, e.g. 960 at k=19 Blake2b, halo2-circuits/src/results/ecdsa_bench.csv:2) */
int zk_proof_size(zk_ctx* ctx, zk_pk pk, int transcript, int scheme, size_t* out);
/* replaces plonk::create_proof (ecdsa_p256.rs:366-373, 416-423, 555-562) for one circuit with no
 * instances (a key WITH an instance column: ZK_EINVAL, halo2's InvalidInstances - zk_prove_public).  `advice` are resident columns (Lagrange values, Montgomery, n rows each; the last 7 rows
 * are overwritten by blinding in a private copy).  Randomness: ChaCha20Rng::from_seed(rng_seed), one
 * 64-byte block per Fr::random in halo2's draw order.  Returns the proof bytes the transcript writer
 * would hold after `finalize()`.  proof_out == NULL: only *proof_len is set. */
int zk_prove(zk_ctx* ctx, zk_pk pk, const zk_poly* advice, size_t n_advice, const uint8_t rng_seed[32],
             int transcript, int scheme, uint8_t* proof_out, size_t proof_cap, size_t* proof_len);
/* ---- public inputs: create_proof / verify_proof with `instances = &[&[&values]]` for a key whose shape has the instance column
 * (zk_circuit_params.num_instance_columns = 1) [RECALLED: halo2 with KZG, QUERY_INSTANCE = false; no reference bytes pin it - the
 * reference circuit has no public inputs.  tests/halo2_ref.py restates the rule and the bytes are compared with it]:
 *   vk digest   num_instance_columns: 1, instance_queries: [(Column { index: 0, column_type: Instance }, Rotation(0))], and the
 *               column at the end of the permutation argument's columns
 *   transcript  transcript_repr; EVERY instance value as common_scalar, in order (absorbed, not written; the count is not hashed);
 *               the advice commitments and on as zk_prove
 *   column      the values fill rows 0 .. m - 1 of a Lagrange column, the rest is zero; it is neither blinded nor committed nor
 *               evaluated into the proof nor opened, and draws nothing from the RNG.  It enters the permutation grand product as
 *               its column's values and the quotient as that column's extended coset
 *   verifier    absorbs the same values and uses inst(x) = sum_i v_i l_i(x) as the column's evaluation in the permutation terms of
 *               the expected h(x); nothing else changes
 * [v] and [v, 0] are the same polynomial and different transcripts: neither proof verifies under the other list.  The proof grows
 * by the column's sigma evaluation and, where the column starts a permutation chunk of its own, by that chunk's z commitment and
 * evaluations (k = 19 one-column shape: 960 -> 992 bytes Blake2b; k = 17 server shape: 2720 -> 2912 bytes EVM + GWC).
 * n_instance == 0 is an empty column.  On a key WITHOUT the column n_instance must be 0 and the bytes are zk_prove's.
 * ZK_EINVAL beyond zk_prove's cases: a value that is not a Montgomery image below the modulus, n_instance > n - 7 (halo2's
 * InstanceTooLarge), values for a key without the column.  The workspace of a key with the column is three vectors larger (values,
 * coefficients, extended coset: 96 MiB at k = 19).
 * The batch and multi forms WITH instances are zk_prove_batch_public, zk_prove_multi_public, zk_verify_batch_public and
 * zk_verify_multi_public below.  zk_prove_batch, zk_prove_multi, zk_verify_batch, zk_verify_multi - and zk_prove, zk_verify,
 * zk_witness_check - carry none and return ZK_EINVAL on a key with the column.
 * The phase-level forms WITH instances are zk_permutation_product_public and zk_quotient_multi (examples/prove_host_phases_multi.cpp
 * builds these proofs from them); zk_permutation_product / zk_quotient carry none and return ZK_EINVAL on such a key.
 * OUT OF SCOPE: more than one instance column; batches of multi proofs.
 * Every other entry point (zk_lookup_permute, zk_lookup_product, the file and key functions, zk_pk_check) works on such a key. */
int zk_prove_public(zk_ctx* ctx, zk_pk pk, const zk_poly* advice, size_t n_advice,
                    const uint64_t* instance_mont /* n_instance x 4 */, size_t n_instance, const uint8_t rng_seed[32], int transcript,
                    int scheme, uint8_t* proof_out, size_t proof_cap, size_t* proof_len);
/* `batch` independent create_proof calls for ONE key in lock-step on this context: the reference's concurrent requests
 * (one Rocket worker thread per request, proving-server/src/main.rs:457-472, each inside create_proof, ecdsa_p256.rs:366-373 /
 * 416-423) advanced phase by phase together, so that the same commitment of all proofs shares one MSM pass, the same
 * transform one launch per NTT pass, and every proof's lookups / grand products / openings one set of launches.  Proof j
 * gets advice[j * n_advice .. (j + 1) * n_advice) and rng_seeds[32 j .. 32 j + 32) and is byte-identical to zk_prove with
 * the same key, advice and seed; the proofs have one length (*proof_len) and are written proof_stride bytes apart
 * (proofs_out == NULL: only *proof_len).  The first call with a larger batch allocates the further workspaces (kept with
 * the key: ~1.4 GiB each at k = 19).  ZK_EWITNESS means SOME proof's witness is off the table: the batch fails as a whole
 * (zk_prove tells which).  ZK_EINVAL: batch == 0, batch > ZK_PROVE_BATCH_MAX, batch x (#chunks + #lookups) > 256. */
#define ZK_PROVE_BATCH_MAX 64
int zk_prove_batch(zk_ctx* ctx, zk_pk pk, size_t batch, const zk_poly* advice /* batch x n_advice, proof-major */, size_t n_advice,
                   const uint8_t* rng_seeds /* batch x 32 */, int transcript, int scheme, uint8_t* proofs_out, size_t proof_stride,
                   size_t* proof_len);
/* replaces plonk::create_proof(&params, &pk, &[c_0 .. c_{N-1}], &[&[]; N], rng, &mut transcript): N circuits under ONE key in ONE
 * proof - one transcript, one set of challenges, one random polynomial, one quotient, one multi-open - as halo2 makes it for
 * `circuits: &[ConcreteCircuit]` [RECALLED; not pinned by reference bytes: tests/halo2_ref.py restates the rule and the bytes
 * are compared with it].  c = 0 .. N - 1 in the caller's order:
 *   transcript  transcript_repr (N is not hashed); for c: the advice commitments; theta; for c, per lookup: a', s'; beta, gamma;
 *               for c: z of every chunk; for c: zL of every lookup; ONE random-polynomial commitment; y; the h pieces (as many as
 *               for one circuit); x; evaluations - for c: advice; fixed, once; random; sigma, once; for c: the permutation's; for
 *               c: the lookups' - then the multi-open over, for c: circuit c's openings in zk_prove's order, then fixed, sigma, h,
 *               random
 *   RNG         ONE ChaCha20Rng::from_seed(rng_seed), drawn in the same nesting: every phase's draws for c = 0, 1, ..; then the
 *               random polynomial's n draws and its blind, then the h blinds
 *   quotient    the y-Horner chain runs on across the circuits: h = sum_c y^(T (N - 1 - c)) h_c, T = terms of one circuit
 * `advice` holds n_circuits x n_advice resident columns, circuit-major.  n_circuits == 1 gives zk_prove's bytes.  What is paid
 * per circuit is its own commitments (5 at the one-column k = 19 shape, 11 at the four-column k = 17 one); the random polynomial,
 * the h pieces, the opening proof, the inverse coset transform of h and the fixed / sigma evaluations are paid once per proof.
 * Circuit c > 0 works in the key's further workspaces (shared with zk_prove_batch, allocated on first use and kept: ~1.4 GiB
 * each at k = 19).  A verifier must expect the same N: zk_verify_multi here, `verify_proof` with N instance slices in halo2, a
 * verifier generated `with_num_proof(N)` in snark-verifier.
 * ZK_EINVAL: n_circuits == 0, n_circuits > ZK_PROVE_MULTI_MAX, n_circuits x (#chunks + #lookups) > 256, or zk_prove's own cases;
 * ZK_ESTATE as zk_prove; ZK_EWITNESS: SOME circuit's lookup input is off the table - the call fails as a whole, the outputs are
 * untouched (zk_witness_check tells which circuit).  proof_out == NULL: only *proof_len is set.  Follows zk_prove_batch's rules
 * for ZK_OPT_QUOTIENT_DOMAIN, ZK_OPT_BATCH_PASS_COLUMNS and the activity hold.  No instances (a key with an instance column:
 * ZK_EINVAL; zk_prove_public proves one circuit with them); no batches of such proofs. */
#define ZK_PROVE_MULTI_MAX 16
/* the length of a proof over n_circuits circuits.  On a key with an instance column it is the length of zk_prove_multi_public's proof:
 * the column is one more permutation column (its sigma evaluation once per proof; where it starts a chunk of its own, that chunk's z
 * commitment and evaluations once per circuit), and nothing else of it is in the proof - the count below takes the shape's
 * permutation columns and chunks, which include it. */
int zk_proof_size_multi(zk_ctx* ctx, zk_pk pk, size_t n_circuits, int transcript, int scheme, size_t* out);
int zk_prove_multi(zk_ctx* ctx, zk_pk pk, size_t n_circuits, const zk_poly* advice /* n_circuits x n_advice, circuit-major */,
                   size_t n_advice, const uint8_t rng_seed[32], int transcript, int scheme, uint8_t* proof_out, size_t proof_cap,
                   size_t* proof_len);
/* ---- the batch and multi forms with public inputs ----
 * Lists: instances_mont[j] holds n_instances[j] Montgomery values (x 4 words); the lists of one call may differ in length, 0
 * included, and instances_mont[j] may be NULL where n_instances[j] == 0.  Every list is validated by zk_prove_public's rules (a
 * Montgomery image below the modulus, at most n - 7 values); one bad list is ZK_EINVAL for the whole call.  On a key WITHOUT the
 * column every length must be 0, both arrays may be NULL, and the bytes are those of the form without _public.  Outputs are
 * untouched on error.  All other limits, errors and options are those of the forms without _public.
 *
 * zk_prove_batch_public: zk_prove_batch with list j for proof j; proof j is byte-identical to zk_prove_public with the same key,
 * advice, list and seed (every proof absorbs its own list into its own transcript).  batch == 1 is zk_prove_public.  The B
 * instance columns are written by ONE staged upload (a table of `batch` entries and the call's concatenated values: 16 bytes per
 * proof + 32 bytes per value, pinned and device, kept with the key's batch buffers and grown to the largest call) and ONE launch that
 * writes every row of every column; their coefficient and coset forms ride in the batched transforms of the first advice forms.
 *
 * zk_prove_multi_public: zk_prove_multi with list c for circuit c [RECALLED, as zk_prove_multi's rule: not pinned by reference
 * bytes; tests/halo2_ref.py restates it and the bytes are compared with it].  The rule is zk_prove_multi's with
 *   transcript   transcript_repr; for c = 0 .. N - 1: every value of circuit c's list (absorbed, not written; neither N nor the
 *                lengths are hashed); then everything else in zk_prove_multi's order.  ALL circuits' instances come before any advice
 *                commitment: halo2's loop over `instances` at the top of create_proof / verify_proof
 *   RNG          the instance columns draw nothing: zk_prove_multi's draw order
 *   permutation  circuit c's grand product reads c's column; quotient pass c reads c's extended coset (or three-coset copy)
 *   verifier     circuit c's permutation terms of the expected h(x) use inst_c(x)
 * n_circuits == 1 is zk_prove_public. */
int zk_prove_batch_public(zk_ctx* ctx, zk_pk pk, size_t batch, const zk_poly* advice /* batch x n_advice, proof-major */, size_t n_advice,
                          const uint64_t* const* instances_mont /* batch lists, each n_instances[j] x 4 */, const size_t* n_instances,
                          const uint8_t* rng_seeds /* batch x 32 */, int transcript, int scheme, uint8_t* proofs_out, size_t proof_stride,
                          size_t* proof_len);
int zk_prove_multi_public(zk_ctx* ctx, zk_pk pk, size_t n_circuits, const zk_poly* advice /* n_circuits x n_advice, circuit-major */,
                          size_t n_advice, const uint64_t* const* instances_mont /* n_circuits lists */, const size_t* n_instances,
                          const uint8_t rng_seed[32], int transcript, int scheme, uint8_t* proof_out, size_t proof_cap, size_t* proof_len);
/* upload canonical (non-Montgomery) integers and convert on the device */
int zk_poly_upload_canonical(zk_ctx* ctx, zk_poly p, const uint64_t* host_canonical, size_t n);

/* ---- MockProver::verify ------------------------------------------------------------------------------------------------
 * What a witness can violate, and where.  `usable` = n - 7 rows (n - blinding factors - 1) carry the circuit; the prover blinds
 * the rest. */
#define ZK_FAIL_GATE 1          /* index = gate column j, row = the row its selector is non-zero on */
#define ZK_FAIL_GATE_BLINDED 2  /* the same, but the gate reads a row the prover blinds (row + 3 >= usable rows):
                                   a failure whatever the values - MockProver's ConstraintPoisoned */
#define ZK_FAIL_LOOKUP 3        /* index = lookup, row = the row whose input is not in the table */
#define ZK_FAIL_COPY 4          /* index = permutation column (zk_keygen's order), row; other_* = the cell sigma maps it to */
typedef struct { uint32_t kind, index, row, other_index, other_row, reserved; } zk_witness_failure;
/* replaces MockProver::run(k, &circuit, vec![]).verify() (ecdsa_p256.rs:209-248) for a resident key and resident advice
 * columns (what zk_prove takes).  counts[kind] = number of failures of each kind (counts[0] = their sum); the first
 * min(cap, counts[0]) failures in ascending (kind, index, row) order are written to `out` (may be NULL with cap 0).
 * A violated circuit is a verdict (ZK_OK, counts[0] != 0), never an error.  Deterministic: same inputs, same output.
 *   gates    every gate column j, every row r whose selector AFTER compress_selectors (q, q (2 - q) or q (1 - q) over the key's
 *            fixed values) is non-zero: a[r] + a[r+1] a[r+2] - a[r+3] != 0 is a ZK_FAIL_GATE; r + 3 >= usable a ZK_FAIL_GATE_BLINDED
 *   lookups  every lookup, every row r < usable: the input (one-column shapes: q_lookup[r] a_0[r]) must be below 2^lookup_bits -
 *            the rule zk_prove returns ZK_EWITNESS by: counts[ZK_FAIL_LOOKUP] != 0 iff zk_prove refuses the witness
 *   copies   every permutation column c, row r < usable with sigma(c, r) = (c', r') != (c, r): different values are one
 *            ZK_FAIL_COPY at (c, r) - one per cell that differs from its sigma-image, so a corrupted cell of a pair is reported
 *            from both sides
 * Advice rows >= usable are never read; the inputs are not modified; nothing a proof is made of changes.  The first check of a
 * key decodes its sigma values into cell indices on the device (4 bytes per cell, kept with the key).
 * ZK_EINVAL: bad handle, n_advice != the shape's, a vector of another length, cap > 0 with out == NULL, or a key whose sigma
 * values are not labels of its own usable cells (a damaged file read with ZK_SERDE_RAW_BYTES_UNCHECKED); ZK_ESTATE: a
 * verifying-only key, or a key whose SRS was replaced. */
int zk_witness_check(zk_ctx* ctx, zk_pk pk, const zk_poly* advice, size_t n_advice, zk_witness_failure* out, size_t cap,
                     uint64_t counts[5]);
/* MockProver::run(k, &circuit, vec![instance]).verify(): zk_witness_check with the instance column's values (rows 0 ..
 * n_instance - 1, zero behind them; zk_prove_public's rules for them).  The instance column is the last permutation column: an
 * advice cell whose sigma-image is an instance cell with another value is a ZK_FAIL_COPY, reported from both sides.  The values
 * pass through the key's idle instance column; no proof byte depends on a check.  zk_witness_check itself returns ZK_EINVAL on
 * a key with the column. */
int zk_witness_check_public(zk_ctx* ctx, zk_pk pk, const zk_poly* advice, size_t n_advice, zk_witness_failure* out, size_t cap,
                            uint64_t counts[5], const uint64_t* instance_mont /* n_instance x 4 */, size_t n_instance);

/* ---- the key itself: is a resident proving key what keygen would have made of its own values? ---------------------------
 * A ProvingKey holds every column four times - commitment, values, coefficients, extended coset - next to l_0 / l_last /
 * l_active and the permutation's sigma columns; zk_pk_read checks lengths, element ranges, the range table and the selector
 * bits, and ties none of these copies to each other (halo2's ProvingKey::read validates elements only).  zk_pk_check does. */
#define ZK_PK_PART_FIXED_COMMIT 1  /* column f: commit_lagrange(fixed values f) under the RESIDENT SRS != the vk's commitment (index 0, count 1) */
#define ZK_PK_PART_SIGMA_COMMIT 2  /* the same for permutation column c */
#define ZK_PK_PART_FIXED_POLY   3  /* column f, index i: coefficient i != lagrange_to_coeff(fixed values f)[i] */
#define ZK_PK_PART_SIGMA_POLY   4
#define ZK_PK_PART_FIXED_COSET  5  /* column f, index i < 4n: coset value i != coeff_to_extended(fixed coefficients f)[i] */
#define ZK_PK_PART_SIGMA_COSET  6
#define ZK_PK_PART_L_COSET      7  /* column 0 / 1 / 2 = l_0 / l_last / l_active: != the closed form zk_keygen builds */
#define ZK_PK_PART_SIGMA_LABEL  8  /* column c, index r: the sigma value is not delta^c' w^r' of a cell with c' < #permutation columns and
                                      r' < usable (r < usable), or not the cell's own label (r >= usable) */
#define ZK_PK_PART_SIGMA_MAP    9  /* column c, index r: no cell's sigma value names cell (c, r) - sigma is not a bijection of the cells */
typedef struct { uint32_t part, column, index, reserved; uint64_t count; } zk_pk_finding;

#define ZK_PK_CHECK_COMMITMENTS 1u /* no finding of parts 1, 2 */
#define ZK_PK_CHECK_POLYS       2u /* none of 3, 4 */
#define ZK_PK_CHECK_COSETS      4u /* none of 5, 6, 7 */
#define ZK_PK_CHECK_SIGMA       8u /* none of 8, 9 */
#define ZK_PK_CHECK_ALL        15u
#define ZK_PK_CHECK_REPR       16u /* informational: transcript_repr is the value zk_keygen computes for these commitments and this shape
                                      (clear after a host override with another value - not a fault of the key) */
/* Each part is compared with what its SOURCE PART AS IT STANDS IN THE KEY yields - values -> commitment, values -> coefficients,
 * coefficients -> extended coset - through the routines zk_keygen itself uses, byte for byte on the Montgomery images
 * (everything the engine makes is fully reduced, so the image is unique; a non-reduced element of an unchecked file is a
 * mismatch).  One damaged element therefore has an exact signature: a damaged VALUE is 1 commitment finding plus count = n in
 * the column's POLY part (every coefficient of the inverse transform moves); a damaged COEFFICIENT is count = 1 in POLY and
 * count = 4n in COSET; a damaged COSET ELEMENT is count = 1 in COSET.  Sigma: a cell whose value has a LABEL finding names
 * nobody, so a value replaced by a non-label is LABEL 1 + MAP 1, one replaced by another cell's label is MAP 1 alone.
 * One finding per (part, column) that has any mismatch: its lowest `index` and its `count`, in ascending (part, column) order;
 * the first min(cap, *n_findings) are written (`out` may be NULL with cap 0), *n_findings is the total.  Fixed columns are
 * numbered in zk_vk_export's (query) order, permutation columns in zk_keygen's.  Same key, same output, on every run.  A
 * broken key is a verdict (ZK_OK, bits of *flags clear), never an error.  The key, every proof byte and what
 * zk_witness_check returns are unchanged by a check; its scratch is the key's idle quotient buffer, and what it allocates
 * on a key's first check (one bit per permutation cell, 16 bytes per (part, column)) is kept with the key.  Out of scope: the
 * lazily derived three-coset copies (made from the cosets checked here), the range table and the selector structure (zk_keygen
 * and zk_pk_read refuse violations).
 * ZK_EINVAL: bad handle, NULL flags / n_findings, cap > 0 with out == NULL; ZK_ESTATE: a verifying-only key, or a key whose
 * SRS was replaced. */
int zk_pk_check(zk_ctx* ctx, zk_pk pk, uint32_t* flags, zk_pk_finding* out, size_t cap, size_t* n_findings);

/* ---- verify_proof ---------------------------------------------------------------------------------------------------
 * plonk::verify_proof with the KZG pairing check (ecdsa_p256.rs:429-469: `verify` = Blake2b + SHPLONK, `verify_evm` = EVM +
 * GWC; no instances - zk_verify_public takes them).  The check is e(A, [s]G2) = e(B, G2) with g[0], g2 and s_g2 of the context's resident SRS: a proof
 * made under another SRS is rejected.  A bad proof is a verdict (ZK_OK, *ok = 0 / verdicts[j] = 0), never an error; the
 * error codes mean bad arguments (ZK_EINVAL), a full key whose SRS was replaced, or no SRS / no G2 half in the context
 * (ZK_ESTATE: zk_srs_load needs zk_srs_set_g2 first). */
/* replaces VerifyingKey::read::<_, ECDSACircuit<Fr>> (ecdsa_p256.rs:431-435): the zk_vk_write image of `params`' shape
 * gives a VERIFYING-ONLY key — commitments and transcript_repr, no SRS-sized memory, no prover workspace (zk_prove,
 * zk_prove_batch, zk_pk_write, zk_vk_write and the phase-level entry points return ZK_ESTATE for it; zk_pk_shape,
 * zk_vk_export, zk_verify and zk_pk_free work).  transcript_repr NULL: computed as zk_keygen does. */
int zk_vk_read(zk_ctx* ctx, const zk_circuit_params* params, const uint8_t* bytes, size_t len, int format,
               const uint64_t transcript_repr_mont[4], zk_pk* out);
/* the inverse of zk_vk_export: a verifying-only key from affine Montgomery commitments (n_fixed and n_perm of the shape,
 * fixed columns in zk_vk_export's order); a point off the curve is ZK_EINVAL */
int zk_vk_from_parts(zk_ctx* ctx, const zk_circuit_params* params, const uint64_t* fixed_commitments, const uint64_t* perm_commitments,
                     const uint64_t transcript_repr_mont[4], zk_pk* out);
/* one proof of `pk` (full or verifying-only): *ok = 1 if it verifies.  The batch of one below. */
int zk_verify(zk_ctx* ctx, zk_pk pk, int transcript, int scheme, const uint8_t* proof, size_t len, int* ok);
/* verify_proof with the public inputs of zk_prove_public (full or verifying-only key): the values are absorbed as the prover
 * absorbed them and inst(x) is computed on the host with one batch inversion.  Wrong values are a verdict (*ok = 0); a list the
 * column cannot hold (n_instance > n - 7, or any value for a key without the column) or a value not below the modulus is
 * ZK_EINVAL.  On a key without the column and n_instance == 0 it is zk_verify. */
int zk_verify_public(zk_ctx* ctx, zk_pk pk, int transcript, int scheme, const uint64_t* instance_mont /* n_instance x 4 */,
                     size_t n_instance, const uint8_t* proof, size_t len, int* ok);
/* `batch` proofs of one key: verdicts[j] = what zk_verify says of proof j.  Points are decoded and the per-proof sums
 * are made on the device, the proofs are folded with random 128-bit weights into one pairing, and a failing set is halved
 * until every verdict is exact.  ZK_EINVAL: batch == 0 or > ZK_VERIFY_BATCH_MAX. */
#define ZK_VERIFY_BATCH_MAX 1024
int zk_verify_batch(zk_ctx* ctx, zk_pk pk, size_t batch, int transcript, int scheme, const uint8_t* const* proofs, const size_t* lens,
                    uint8_t* verdicts);

/* one proof of zk_prove_multi over n_circuits circuits (verify_proof with n_circuits empty instance slices; a key with an instance
 * column: ZK_EINVAL): the proof is read in
 * zk_prove_multi's order, the expected h(x) is the y-Horner of the n_circuits x T expressions, one pairing.  A bad proof - one of
 * another circuit count included: it has another length - is a verdict (*ok = 0), never an error.  Full and verifying-only
 * keys.  n_circuits == 1 is zk_verify.  ZK_EINVAL: n_circuits == 0 or > ZK_PROVE_MULTI_MAX. */
int zk_verify_multi(zk_ctx* ctx, zk_pk pk, size_t n_circuits, int transcript, int scheme, const uint8_t* proof, size_t len, int* ok);

/* zk_verify_batch with list j for proof j (verdicts[j] = zk_verify_public's of proof j and list j) and zk_verify_multi with list c
 * for circuit c (n_circuits == 1 is zk_verify_public).  Lists as for the provers above; wrong values are a verdict, a list the
 * column cannot hold or a value not below the modulus is ZK_EINVAL for the whole call.  inst(x) is evaluated where
 * zk_verify_instance_eval_mode says (auto: the host; the device path runs every proof's transcript to x on the host, evaluates every
 * list of the call in one launch, and computes the rest of the term lists on the host).  The fold weights of the batch form are
 * drawn from a hash of the key, every proof's bytes AND every proof's list (length first), so that the whole statement is fixed
 * before the weights are; the bisection makes every verdict exact as before. */
int zk_verify_batch_public(zk_ctx* ctx, zk_pk pk, size_t batch, int transcript, int scheme, const uint64_t* const* instances_mont,
                           const size_t* n_instances, const uint8_t* const* proofs, const size_t* lens, uint8_t* verdicts);
int zk_verify_multi_public(zk_ctx* ctx, zk_pk pk, size_t n_circuits, int transcript, int scheme, const uint64_t* const* instances_mont,
                           const size_t* n_instances, const uint8_t* proof, size_t len, int* ok);

/* The EVM verifier of ONE kind of proof, as the text of a Yul program (the reference's /generate_evm_verifier; csrc/evm_codegen.h):
 * proofs of `pk` (full or verifying-only: the same bytes) over n_circuits circuits with n_instances[c] public inputs in circuit c
 * (NULL: none anywhere), made with the EVM transcript and `scheme` (ZK_SCHEME_DEFAULT is GWC), checked against the g2 / s_g2 of the
 * context's resident SRS.  The program takes the calldata [every instance, circuit-major, as a 32-byte big-endian word][the proof],
 * of one exact length, and reverts unless the proof verifies: it accepts exactly what zk_verify / zk_verify_public / zk_verify_multi /
 * zk_verify_multi_public accept for the same lists.  The text is a function of the arguments alone (no time stamp, no address).
 * out == NULL: only *len is set, like zk_vk_write; cap < *len: ZK_EINVAL with *len set.  ZK_EINVAL also: NULL ctx / len, n_circuits
 * == 0 or > ZK_PROVE_MULTI_MAX, a non-zero count on a key without the instance column, a count above n - 7, an unknown scheme, a
 * bad handle.  ZK_ESTATE as zk_verify (no SRS or no G2 half; a full key whose SRS was replaced).  `out` is untouched on every error.
 * Host work only: nothing is launched.  The text has not been compiled by solc nor run on an EVM by anyone: the suite runs it in
 * an interpreter of the Yul subset it uses. */
typedef struct {
    uint32_t calldata_bytes, memory_bytes, modexp, ecadd, ecmul, pairing, keccak_calls, keccak_bytes;
} zk_evm_cost;
int zk_evm_verifier(zk_ctx* ctx, zk_pk pk, size_t n_circuits, const size_t* n_instances /* n_circuits, NULL = none */, int scheme,
                    char* out, size_t cap, size_t* len);
/* what that program costs, counted where it is generated: calldata length, the top of the memory it touches, its calls of
 * precompiles 5 / 6 / 7 / 8 and its keccak256 calls with the bytes they hash.  Errors as zk_evm_verifier (out untouched). */
int zk_evm_verifier_cost(zk_ctx* ctx, zk_pk pk, size_t n_circuits, const size_t* n_instances, int scheme, zk_evm_cost* out);
/* where zk_verify_batch_public / zk_verify_multi_public evaluate inst(x): mode 0 auto, 1 on the host (verifier.h, one batch inversion
 * per list), 2 on the device (zk_instance_eval's kernel: one launch for every list of the call).  Same verdicts.  Auto is the host:
 * the two have NOT been measured against each other (tools/verify_public_rate.py is the tool).  zk_verify_public always evaluates
 * on the host.  A call of its own and not a ZK_OPT_* number: the option numbers of zk_ctx_set_option are a closed set
 * (tests/test_gpu_abi_errors.py pins it, the first undefined number included).  ZK_EINVAL: mode outside 0 .. 2. */
#define ZK_VERIFY_INSTANCE_EVAL_AUTO 0
#define ZK_VERIFY_INSTANCE_EVAL_HOST 1
#define ZK_VERIFY_INSTANCE_EVAL_DEVICE 2
int zk_verify_instance_eval_mode(zk_ctx* ctx, int mode);
/* inst(x) = sum_{i<m} v_i l_i(x), l_i(x) = w^i (x^n - 1) / (n (x - w^i)), n = 2^k, w the engine's primitive n-th root, for `count`
 * (list, point) pairs in one call on the device.  Needs no SRS and no key.  k <= 26, every m_j <= 2^k, values and points Montgomery
 * images below the modulus (else ZK_EINVAL).  on_domain[j] = 1 with out j zero exactly when x_j = w^i for some i < m_j (the case
 * in which the host verifier rejects); m_j = 0 gives zero; x_j^n = 1 with no such i gives zero with the flag clear.  Pairs that
 * name the same list (address and length) share one upload.  Outputs are untouched on error. */
int zk_instance_eval(zk_ctx* ctx, uint32_t k, size_t count, const uint64_t* const* instances_mont, const size_t* n_instances,
                     const uint64_t* x_mont /* count x 4 */, uint64_t* out_mont /* count x 4 */, uint8_t* on_domain /* count */);

/* ---- ES256 request check: secp256r1 (NIST P-256) ECDSA verification on the device ------------------------------------------
 * `count` signatures in one launch, one per lane.  A record is five fields of 32 LITTLE-endian bytes in the order pubkey_x,
 * pubkey_y, r, s, msghash (the proving server's request fields as the web client encodes them).  verdicts[i] = 1 for a valid
 * signature, else 0; reasons (may be NULL) names the FIRST failing test:
 *   ZK_ES256_RANGE      x >= p, y >= p, msghash >= n, r not in [1, n) or s not in [1, n)
 *   ZK_ES256_OFF_CURVE  y^2 != x^3 - 3 x + b ((0, 0) is off the curve)
 *   ZK_ES256_MISMATCH   u1 G + u2 Q (u1 = msghash / s, u2 = r / s mod n) is the identity, or its affine x mod n is not r
 * A bad signature is a verdict, never an error.  Needs no SRS and no key.  The first call on a context builds a 60 KiB table of
 * multiples of G on the device and keeps it with the context.  Public data only: the arithmetic is NOT constant time.
 * ZK_EINVAL: ctx, sigs or verdicts NULL, count == 0 or > ZK_ES256_BATCH_MAX.  Outputs are untouched on every error. */
#define ZK_ES256_VALID 0
#define ZK_ES256_RANGE 1
#define ZK_ES256_OFF_CURVE 2
#define ZK_ES256_MISMATCH 3
#define ZK_ES256_BATCH_MAX 16384
int zk_es256_verify(zk_ctx* ctx, size_t count, const uint8_t* sigs /* count x 160 */, uint8_t* verdicts /* count: 1 = valid */,
                    uint8_t* reasons /* count, may be NULL */);

/* ---- WebAuthn assertion check: the relying party's work on the device, ending in the ES256 check above ------------------------
 * `count` assertions (navigator.credentials.get with an ES256 credential) in two launches, one assertion per lane.  The call makes
 * msghash from the assertion itself - SHA-256(authenticatorData || SHA-256(clientDataJSON)) -, checks what a relying party must
 * check of both, parses the DER signature, assembles zk_es256_verify's 160-byte record and verifies it.  verdicts[i] = 1 for an
 * accepted assertion, else 0; reasons (may be NULL) names the FIRST failing test, in this order:
 *   ZK_WEBAUTHN_SIZE           authenticator_data_len > ZK_WEBAUTHN_AUTHDATA_MAX, client_data_json_len > ZK_WEBAUTHN_CLIENTDATA_MAX,
 *                              signature_len outside 8 .. 72, challenge_len outside 1 .. ZK_WEBAUTHN_CHALLENGE_MAX, origin_len >
 *                              ZK_WEBAUTHN_ORIGIN_MAX (decided on the host: such a request is not uploaded)
 *   ZK_WEBAUTHN_AUTHDATA       authenticatorData shorter than 37 bytes
 *   ZK_WEBAUTHN_RPID           its bytes 0 .. 31 are not rp_id_hash
 *   ZK_WEBAUTHN_FLAGS          (byte 32 & flags_required) != flags_required (UP = 0x01, UV = 0x04).  Bytes 33 .. 36, big-endian, are
 *                              the signature counter: returned in sign_counts, not judged
 *   ZK_WEBAUTHN_CLIENTDATA     the limited verification algorithm of WebAuthn Level 2: with
 *                                E = {"type":"webauthn.get","challenge":"<base64url of challenge, no padding>","origin":"<origin>","crossOrigin":
 *                              clientDataJSON must start with E, go on with `true` or `false`, then `,` or `}`, and end in `}`;
 *                              `true` passes only with allow_cross_origin.  No JSON is parsed: the same members in another order
 *                              are refused with this reason
 *   ZK_WEBAUTHN_SIGNATURE_DER  the signature is not the strict DER of ECDSA-Sig-Value (30 len 02 lr r 02 ls s: short-form lengths,
 *                              len exact, INTEGERs of 1 .. 33 bytes, non-negative, minimal, below 2^256, nothing after s)
 *   ZK_WEBAUTHN_RANGE, _OFF_CURVE, _MISMATCH   zk_es256_verify's, with the same values, over the assembled record
 * records (may be NULL): the 160-byte record of each assertion - pubkey_x, pubkey_y, r, s, msghash as 32 LITTLE-endian bytes each,
 * what the provers and zk_es256_verify take -, all zero for one refused before the curve (SIZE .. SIGNATURE_DER).  sign_counts (may
 * be NULL): the counter, 0 for SIZE and AUTHDATA.  A bad assertion is a verdict, never an error.  Needs no SRS and no key; shares
 * zk_es256_verify's table of G (built by the first call of either on a context).  Public data only: NOT constant time.
 * ZK_EINVAL: ctx, a or verdicts NULL, count == 0 or > ZK_WEBAUTHN_BATCH_MAX, a NULL pointer with a non-zero length.  Outputs are
 * untouched on every error. */
#define ZK_WEBAUTHN_VALID 0
#define ZK_WEBAUTHN_RANGE 1
#define ZK_WEBAUTHN_OFF_CURVE 2
#define ZK_WEBAUTHN_MISMATCH 3
#define ZK_WEBAUTHN_SIZE 4
#define ZK_WEBAUTHN_AUTHDATA 5
#define ZK_WEBAUTHN_RPID 6
#define ZK_WEBAUTHN_FLAGS 7
#define ZK_WEBAUTHN_CLIENTDATA 8
#define ZK_WEBAUTHN_SIGNATURE_DER 9
#define ZK_WEBAUTHN_BATCH_MAX ZK_ES256_BATCH_MAX
#define ZK_WEBAUTHN_AUTHDATA_MAX 1024
#define ZK_WEBAUTHN_CLIENTDATA_MAX 4096
#define ZK_WEBAUTHN_CHALLENGE_MAX 64
#define ZK_WEBAUTHN_ORIGIN_MAX 255
typedef struct zk_webauthn_assertion {
    const uint8_t* authenticator_data;
    size_t authenticator_data_len;
    const uint8_t* client_data_json;
    size_t client_data_json_len;
    const uint8_t* signature; /* DER */
    size_t signature_len;
    uint8_t pubkey_x[32], pubkey_y[32]; /* BIG-endian: COSE's -2 / -3 as they are */
    const uint8_t* challenge;           /* the raw bytes the server issued */
    size_t challenge_len;
    const char* origin;
    size_t origin_len;
    uint8_t rp_id_hash[32];
    uint8_t flags_required; /* e.g. 0x01, or 0x05 with user verification */
    uint8_t allow_cross_origin;
} zk_webauthn_assertion;
int zk_webauthn_verify(zk_ctx* ctx, size_t count, const zk_webauthn_assertion* a, uint8_t* verdicts /* count */,
                       uint8_t* reasons /* count, may be NULL */, uint8_t* records /* count x 160, may be NULL */,
                       uint32_t* sign_counts /* count, may be NULL */);

/* ---- WebAuthn registration check: where the key zk_webauthn_verify takes came from ------------------------------------------------
 * `count` registrations (navigator.credentials.create with an ES256 credential) in two launches, one per lane.  The call walks the
 * attestationObject (CBOR), checks authData and the attested credential data in it, takes the COSE key out, checks clientDataJSON
 * and, where the policy asks for it, the attestation statement; a packed self attestation is verified with the credential's own
 * key through zk_es256_verify's rule.  verdicts[i] = 1 for an accepted registration, else 0; reasons (may be NULL) names the FIRST
 * failing test, in this order (0 .. 9 are zk_webauthn_verify's values and meanings):
 *   ZK_WEBAUTHN_SIZE           attestation_object_len outside 1 .. ZK_WEBAUTHN_ATTOBJ_MAX, client_data_json_len >
 *                              ZK_WEBAUTHN_CLIENTDATA_MAX, challenge_len outside 1 .. ZK_WEBAUTHN_CHALLENGE_MAX, origin_len >
 *                              ZK_WEBAUTHN_ORIGIN_MAX (decided on the host: such a request is not uploaded)
 *   ZK_WEBAUTHN_CBOR           the object is not a definite-length map of exactly  "fmt" -> text, "attStmt" -> map, "authData" ->
 *                              byte string  in this order (CTAP2's canonical one) with nothing after it, or holds a data item that
 *                              is not well-formed under the strict rule: definite lengths only (additional information 28 .. 31
 *                              refused, `break` included), every head in its shortest form, a one-byte simple value >= 32, no
 *                              declared count of bytes, items or pairs above the bytes left.  Floats are taken as they are, text is
 *                              not checked for UTF-8
 *   ZK_WEBAUTHN_AUTHDATA, _RPID, _FLAGS   zk_webauthn_verify's rules over the authData bytes
 *   ZK_WEBAUTHN_CREDENTIAL     AT (0x40) clear; or aaguid (16 bytes), credentialIdLength (big-endian, 1 .. 1023), the id or the key
 *                              (one well-formed data item) run past the end of authData; or, behind the key, ED (0x80) clear and
 *                              authData goes on, ED set and what follows is not exactly one well-formed map
 *   ZK_WEBAUTHN_COSE_KEY       the key is not the 77 bytes  a5 01 02 03 26 20 01 21 58 20 <x> 22 58 20 <y>  (EC2, ES256, P-256 in
 *                              canonical form; compared as bytes: other algorithms, curves, member orders, extra members and
 *                              coordinates not of 32 bytes are refused)
 *   ZK_WEBAUTHN_CLIENTDATA     zk_webauthn_verify's rule with "type":"webauthn.create" in E
 *   ZK_WEBAUTHN_RANGE, _OFF_CURVE   the credential key: x, y below p and on the curve, whatever the statement
 *   ZK_WEBAUTHN_ATTESTATION    only under ZK_WEBAUTHN_ATT_NONE_OR_SELF: the statement is neither fmt "none" with an empty map nor
 *                              fmt "packed" with exactly {"alg": -7, "sig": bytes} in that order (self attestation, no x5c)
 *   ZK_WEBAUTHN_SIGNATURE_DER, then _RANGE / _MISMATCH   for a packed self statement under that policy: sig through the strict DER
 *                              parse, then zk_es256_verify's rule over  x, y, r, s, SHA-256(authData || SHA-256(clientDataJSON))
 * Under ZK_WEBAUTHN_ATT_IGNORE the statement only has to be well-formed and is not judged (attestation = _NOT_JUDGED for every
 * fmt): what a relying party that asked for conveyance "none" does.  Certificate chains (x5c) and every other format's own
 * verification are not done here.  out (may be NULL): the credential of each accepted registration, ALL ZERO for a refused one - a
 * refused registration never hands out a key.  A bad registration is a verdict, never an error.  Needs no SRS and no key; shares
 * zk_es256_verify's table of G.  Public data only: NOT constant time.
 * ZK_EINVAL: ctx, r or verdicts NULL, count == 0 or > ZK_WEBAUTHN_BATCH_MAX, a NULL pointer with a non-zero length, an
 * attestation_policy above 1.  Outputs are untouched on every error. */
#define ZK_WEBAUTHN_CBOR 10
#define ZK_WEBAUTHN_CREDENTIAL 11
#define ZK_WEBAUTHN_COSE_KEY 12
#define ZK_WEBAUTHN_ATTESTATION 13
#define ZK_WEBAUTHN_ATTOBJ_MAX 8192
#define ZK_WEBAUTHN_ATT_IGNORE 0
#define ZK_WEBAUTHN_ATT_NONE_OR_SELF 1
#define ZK_WEBAUTHN_ATTESTED_NONE 0
#define ZK_WEBAUTHN_ATTESTED_SELF 1 /* the signature was verified with the credential's key */
#define ZK_WEBAUTHN_ATTESTED_NOT_JUDGED 2
typedef struct zk_webauthn_registration {
    const uint8_t* attestation_object; /* CBOR, as the authenticator returned it */
    size_t attestation_object_len;
    const uint8_t* client_data_json;
    size_t client_data_json_len;
    const uint8_t* challenge; /* the raw bytes the server issued */
    size_t challenge_len;
    const char* origin;
    size_t origin_len;
    uint8_t rp_id_hash[32];
    uint8_t flags_required; /* e.g. 0x01, or 0x05 with user verification */
    uint8_t allow_cross_origin;
    uint8_t attestation_policy; /* ZK_WEBAUTHN_ATT_* */
} zk_webauthn_registration;
typedef struct zk_webauthn_credential {
    uint8_t pubkey_x[32], pubkey_y[32]; /* BIG-endian, what zk_webauthn_assertion takes */
    uint8_t aaguid[16];
    uint32_t auth_data_off, auth_data_len; /* within the caller's attestation_object */
    uint32_t credential_id_off, credential_id_len;
    uint32_t sign_count;
    uint8_t flags;       /* authData byte 32 */
    uint8_t attestation; /* ZK_WEBAUTHN_ATTESTED_* */
} zk_webauthn_credential;
int zk_webauthn_register(zk_ctx* ctx, size_t count, const zk_webauthn_registration* r, uint8_t* verdicts /* count */,
                         uint8_t* reasons /* count, may be NULL */, zk_webauthn_credential* out /* count, may be NULL */);

/* ---- KZG pairing checks on the device ----------------------------------------------------------------------------------
 * `count` checks e(a_i, s_g2) = e(b_i, g2) in one launch, one per lane, against ONE (g2, s_g2) pair: the caller's (16-word
 * Montgomery images as zk_srs_set_g2 takes them), or with both NULL the resident SRS's.  a_i, b_i are affine Montgomery points of
 * G1, (0, 0) the identity.  The walk through the Miller loop of the two G2 points is done once per pair on the host (the resident
 * pair's is kept with the SRS and dropped with it) and the lanes evaluate its lines at their points; the final exponentiation
 * uses no table.  verdicts[i] = 1 where the check holds; reasons (may be NULL) names the FIRST failing test:
 *   ZK_PAIRING_RANGE      a coordinate of a_i or b_i not below p
 *   ZK_PAIRING_OFF_CURVE  a_i or b_i neither on y^2 = x^3 + 3 nor the identity (0, 0)
 *   ZK_PAIRING_MISMATCH   e(a_i, s_g2) != e(b_i, g2)
 * A pair with the identity on the G1 side contributes 1: (O, O) holds, (O, b) and (a, O) do not.  A bad pair is a verdict, never
 * an error.  Needs no key; with its own G2 points it needs no SRS.
 * ZK_EINVAL: ctx, a, b or verdicts NULL, count == 0 or > ZK_PAIRING_BATCH_MAX, exactly one of g2 / s_g2 NULL, a given G2 point
 * with a coordinate not below p, off the twist, outside the order-r subgroup, or the identity.  ZK_ESTATE: both NULL and no SRS
 * or no G2 half resident.  Outputs are untouched on every error. */
#define ZK_PAIRING_VALID 0
#define ZK_PAIRING_RANGE 1
#define ZK_PAIRING_OFF_CURVE 2
#define ZK_PAIRING_MISMATCH 3
#define ZK_PAIRING_BATCH_MAX 4096
int zk_pairing_check_batch(zk_ctx* ctx, size_t count, const uint64_t* a /* count x 8 */, const uint64_t* b /* count x 8 */,
                           const uint64_t g2[16], const uint64_t s_g2[16], uint8_t* verdicts /* count: 1 = holds */,
                           uint8_t* reasons /* count, may be NULL */);
/* The same check with a G2 point PER ITEM: `count` checks e(a_i, q_i) = e(b_i, g2) in one launch, one per lane.  q_i are 16-word
 * images like g2's; g2 is the caller's, or with NULL the resident SRS's.  No walk of q_i can be prepared, so the lane tests its q_i
 * ([r] q_i in Jacobian coordinates) and walks it through the Miller loop itself, inverting nothing; g2's lines come from a
 * prepared table as above.  Reasons are zk_pairing_check_batch's in its order, the G1 tests first, then
 *   ZK_PAIRING_G2         q_i not a proper G2 point (range, off the twist, outside the subgroup, identity)
 * and ZK_PAIRING_MISMATCH last.  A bad item is a verdict, never an error.
 * ZK_EINVAL: ctx, a, b, q or verdicts NULL, count == 0 or > ZK_PAIRING_BATCH_MAX, a given g2 that is not a proper G2 point.
 * ZK_ESTATE: g2 NULL and no SRS or no G2 half resident.  Outputs are untouched on every error. */
#define ZK_PAIRING_G2 4            /* q_i not a proper G2 point (range, off the twist, outside the subgroup, identity) */
int zk_pairing_check_each(zk_ctx* ctx, size_t count, const uint64_t* a /* count x 8 */, const uint64_t* b /* count x 8 */,
                          const uint64_t* q /* count x 16 */, const uint64_t g2[16] /* NULL: the resident SRS's */,
                          uint8_t* verdicts /* count: 1 = holds */, uint8_t* reasons /* count, may be NULL */);
/* How zk_verify_batch / zk_verify_batch_public settle a set of two or more proofs whose folded check fails.  HOST: the set is
 * halved and each half folded and paired again (up to 2 B - 1 host pairings when every proof fails).  DEVICE: the first fold is
 * still one host check — an all-good batch costs what it always did —, and when it fails every proof of the set goes through one
 * launch of the device pairing, whose verdicts are final.  Sets of one (zk_verify, zk_verify_public, zk_verify_multi*) stay on the
 * host.  AUTO is the host.  Verdicts are the same in every mode.  ZK_EINVAL outside 0..2. */
#define ZK_VERIFY_PAIRING_AUTO 0
#define ZK_VERIFY_PAIRING_HOST 1
#define ZK_VERIFY_PAIRING_DEVICE 2
int zk_verify_pairing_mode(zk_ctx* ctx, int mode);
/* out[0]: host pairing checks, out[1]: device-checked pairs, of the zk_verify* calls of this context since zk_ctx_create */
int zk_verify_pairing_stats(zk_ctx* ctx, uint64_t out[2]);

/* ---- timing of the last call of each kind, measured with HIP events on the
 *      context stream (ms); used by bench.py for the roofline figures ---------- */
#define ZK_T_MSM 0
#define ZK_T_NTT 1
#define ZK_T_QUOTIENT 2
#define ZK_T_EVAL 3
#define ZK_T_MSM_ACCUM 4 /* the bucket-accumulation kernel of the last MSM alone */
#define ZK_T_MSM_COLUMNS 5 /* count only: scalar vectors (commitments) the accumulate launches served — a launch
                              serves several columns when commitments are batched */
#define ZK_T_MSM_TAIL_MAIN 6 /* count only: MSM passes whose reduction tail ran on the context's main stream (ZK_OPT_MSM_TAIL_STREAM) */
#define ZK_T_MSM_TAIL 7 /* the reduction tail (T1 .. T3) of the last MSM pass on the wide path, on whichever stream it ran */
#define ZK_T_COUNT 8
int zk_last_kernel_ms(zk_ctx* ctx, int which, float* out_ms);
/* accumulated HIP-event time and launch count since the last reset (ZK_T_MSM, ZK_T_MSM_ACCUM) */
/* ZK_OPT_STREAM_AUDIT: counts[0] = ordering checks made since the option was switched on, counts[1] = violations; msg (may be NULL)
 * receives the description of the first violation (empty if none) */
int zk_audit_report(zk_ctx* ctx, uint64_t counts[2], char* msg, size_t cap);
int zk_timer_reset(zk_ctx* ctx);
/* shader-clock probe: one wave spins for `millis` (1..2000) on a chain of dependent multiply-adds; out[0] = ticks of the shader-clock
 * counter (s_memtime), out[1] = ticks of the constant 100 MHz counter (s_memrealtime) over the same interval, out[2] = multiply-adds
 * issued, out[3] = scratch.  sclk = out[0] / out[1] x 100 MHz.  Called on a context of its own while other contexts prove, it
 * reads the clock the chip sustains UNDER that load (bench.py: roofline.valu_issue) */
int zk_clock_probe(zk_ctx* ctx, uint32_t millis, uint64_t out[4]);
int zk_timer_stats(zk_ctx* ctx, int which, double* total_ms, uint64_t* count);

/* ---- stream placement ------------------------------------------------------
 * The engine keeps, per device, a pool of 8 main and 32 side streams and hands a context its streams from it.  Which streams
 * share a hardware queue decides whether four pipelines (and the streams of a lone proof) run side by side or queue behind
 * each other (ZK_OPT_MSM_TAIL_STREAM above: 228 -> 190 proofs/s at k = 17 when main streams share queues).  The pool is made in
 * an order that gives the wanted placement under the HIP runtime's rule for a process that made no stream before - a host
 * that did (another GPU library, a tensor framework), another GPU_MAX_HW_QUEUES or another runtime release breaks the
 * assumption silently.  zk_stream_placement MEASURES the placement: a stamp-and-spin kernel per stream finds the classes of
 * streams that wait for each other (csrc/placement.h), about 30 ms on an idle device.  mode 0 reports; mode 1 also re-deals the
 * pool from what it measured when the report is not ZK_PLACEMENT_OK and exactly four classes were seen (further streams are
 * made when a class is short, 64 per device at most; no stream is ever destroyed).  With any other number of classes mode 1
 * changes nothing: CALIBRATED stays clear.
 * A host calls it once per device at start-up, BEFORE its first zk_ctx_create (it makes the pool itself), and logs the report.
 * The engine sees THIS PROCESS only: streams of other processes on the GPU take part in the hardware's scheduling unseen, and
 * work another process runs during the probe delays the probe's kernels and shows as an ambiguous round (UNRESOLVED).
 * Errors (out untouched): ZK_EINVAL (device, out == NULL, mode), ZK_ENODEV, ZK_EHIP, ZK_ESTATE: a context of this process is
 * active on the device (inside a whole-proof call, or enqueued an MSM pass within the last 4 ms) or, for mode 1, exists at all
 * on a pooled slot.  A bad placement is a verdict - ZK_OK with flags clear -, not an error. */
typedef struct {
    uint32_t n_queues;          /* classes among the pool's streams; 0 = unresolved */
    uint32_t flags;             /* ZK_PLACEMENT_* */
    uint8_t  main_queue[8];     /* class of slot i's main stream (classes are numbered in order of first appearance) */
    uint8_t  role_queue[8][3];  /* slot i's tail / transform / MSM stream */
    uint8_t  spare_queue[8];    /* the fourth side stream of slot i's block, unused */
    uint32_t rounds, streams;   /* rounds run, streams measured */
    float    probe_ms;          /* host time of the whole call */
} zk_placement;
#define ZK_PLACEMENT_MAINS_OK   1u  /* slots 0..3: four main streams on four classes (four pipelines) */
#define ZK_PLACEMENT_LONE_OK    2u  /* every slot: main, tail, transform, MSM stream on four classes (a lone proof) */
#define ZK_PLACEMENT_PAIR_OK    4u  /* slots 0, 1: both mains and both tails on four classes (two pipelines) */
#define ZK_PLACEMENT_LAYER1_OK  8u  /* slot 7 - i's main on slot i's class (the fifth context doubles up with the first) */
#define ZK_PLACEMENT_OK        15u
#define ZK_PLACEMENT_CALIBRATED 16u /* this call re-dealt the pool */
#define ZK_PLACEMENT_UNRESOLVED 32u
int zk_stream_placement(int device_id, int mode /* 0 probe, 1 probe + calibrate if not OK */, zk_placement* out);
/* the streams of one context: its slot in the pool (-1: beyond the eight slots, streams of its own), the class of its main, tail,
 * transform and MSM stream as the device's last zk_stream_placement measured them (255 = not measured yet), and four counts
 * since the context was made: MSM passes whose tail ran on the main stream / on the tail stream, proofs that took the transform
 * stream / the MSM stream */
typedef struct {
    int32_t  slot;
    uint8_t  queue[4];
    uint64_t counts[4];
} zk_ctx_streams;
int zk_ctx_stream_info(zk_ctx* ctx, zk_ctx_streams* out);

#ifdef __cplusplus
}
#endif
#endif /* ZKMI355_H */
