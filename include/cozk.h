/*
 * cozk.h -- C ABI of libcozk, the MI355X-native engine for the sumcheck + polynomial-commitment
 * hot path of ChainSafe/co-zkvms (co-jolt / co-noir-spartan workers).
 *
 * This is the drop-in boundary.  Every entry point names the reference interface
 * it replaces (paths relative to the reference repository root).  Conventions:
 *   - plain pointers and sizes only; no C++/torch types; every function returns an int status
 *     (COZK_OK = 0, negative = error; never unwinds across the boundary);
 *     cozk_last_error(ctx) returns the message of the last failure on that context.
 *   - field elements: BN254 Fr / Fq as 4 x u64 little-endian limbs in MONTGOMERY form (R = 2^256),
 *     i.e. the in-memory layout of arkworks `Fp256<MontBackend<_,4>>` (ark-ff 0.5).
 *   - G1 points cross the boundary affine: x[4], y[4] (Fq Montgomery, 64 B) + infinity flag.
 *   - one cozk_ctx per (party, GPU); a ctx owns one HIP stream and is NOT thread-safe -- mirror of
 *     the single-owner IoContext forks (mpc-core/src/protocols/rep3/network.rs:108-119).
 *   - handles (cozk_vec / cozk_bases / cozk_poly / cozk_layer / cozk_spliteq) are device resident;
 *     only round messages (3-8 field elements), commitments and opening proofs cross PCIe.
 */
#ifndef COZK_H
#define COZK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COZK_OK 0
#define COZK_ERR_INVALID_ARG (-1)
#define COZK_ERR_HIP (-2)
#define COZK_ERR_OOM (-3)
#define COZK_ERR_INTERNAL (-4)
#define COZK_ERR_NO_DEVICE (-5)

/* scalar kinds: the variants of jolt-core `MultilinearPolynomial` that
 * `VariableBaseMSM::batch_msm` dispatches on (call site co-jolt/src/poly/commitment/pst13.rs:319-323) */
#define COZK_SCALAR_FR 0  /* LargeScalars: Fr Montgomery, 32 B */
#define COZK_SCALAR_U8 1  /* U8Scalars  (also 0/1 flags) */
#define COZK_SCALAR_U16 2 /* U16Scalars */
#define COZK_SCALAR_U32 3 /* U32Scalars */
#define COZK_SCALAR_U64 4 /* U64Scalars */
#define COZK_SCALAR_I64 5 /* I64Scalars */

/* BindingOrder (jolt-core poly::multilinear_polynomial::BindingOrder; used
 * co-jolt/src/poly/dense_mlpoly.rs:310-459) */
#define COZK_LOW_TO_HIGH 0
#define COZK_HIGH_TO_LOW 1

/* share mode of a polynomial handle */
#define COZK_MODE_PLAIN 1 /* one field element per entry (plain prover / public polynomial) */
#define COZK_MODE_REP3 2  /* Rep3PrimeFieldShare {a, b}: mpc-types/src/protocols/rep3/arithmetic/types.rs:22-29 */

typedef struct cozk_ctx cozk_ctx;
typedef struct cozk_bases cozk_bases;
typedef struct cozk_vec cozk_vec;

/* ---------------------------------------------------------------- context ----------------- */
/* replaces `icicle_init()` (co-jolt/examples/rep3_jolt.rs:195) + IoContext creation */
int cozk_ctx_create(int device, cozk_ctx** out);
int cozk_ctx_destroy(cozk_ctx* ctx);
const char* cozk_last_error(cozk_ctx* ctx);
/* cozk_layer_prove_rounds keeps one single-workgroup kernel resident for the tail of a layer's sumcheck; while it
 * waits for the host's challenge, kernels of other streams that the driver mapped to the same hardware queue
 * cannot start.  That is harmless for independent provers, but provers that need EACH OTHER's round messages to
 * make progress (several parties of one protocol run driven from one process on one GPU) would then wait for each
 * other.  libcozk cannot see such dependencies, so the DEFAULT is automatic and safe: the resident kernel is used
 * only while the context is the one live context on its device in this process (one party per process -- the
 * reference's deployment); as soon as a second context exists, rounds are one launch each.  enable > 0 forces it on
 * (the host vouches that its contexts are independent), 0 off, < 0 restores the automatic default.  If the kernel's
 * watchdog fires anyway (a round callback slower than COZK_RESIDENT_TIMEOUT_S, default 10 s -- e.g. a peer that a
 * transport with a longer timeout is still waiting for), the remaining rounds of that call fall back to
 * per-round launches; the proof is unaffected. */
int cozk_ctx_set_resident_rounds(cozk_ctx* ctx, int enable);
int cozk_ctx_synchronize(cozk_ctx* ctx);
/* raw hipStream_t of the context (so a host can order its own work / events against it) */
int cozk_ctx_stream(cozk_ctx* ctx, void** out_stream);
int cozk_device_count(int* out);

/* ---------------------------------------------------------------- device vectors ---------- */
/* upload a scalar vector (kind = COZK_SCALAR_*); `host` holds n elements of that kind */
int cozk_vec_upload(cozk_ctx* ctx, const void* host, size_t n, int kind, cozk_vec** out);
/* An FR vector whose canonical values fit `kind` (COZK_SCALAR_U32 / COZK_SCALAR_U64) as a vector of that kind -- what
 * VariableBaseMSM::msm_field_elements does before it dispatches on the scalars' bit length (jolt-core msm; call site
 * co-jolt/src/poly/commitment/pst13.rs:286-294): the MSM then sorts 3 / 5 windows of a 4- / 8-byte scalar instead of 16 of a
 * 32-byte one.  COZK_ERR_INVALID_ARG (and no vector) if any value does not fit. */
int cozk_vec_narrow(cozk_ctx* ctx, const cozk_vec* fr, int kind, cozk_vec** out);
int cozk_vec_alloc(cozk_ctx* ctx, size_t n, int kind, cozk_vec** out);
int cozk_vec_download(cozk_ctx* ctx, const cozk_vec* v, void* host);
int cozk_vec_free(cozk_vec* v);
size_t cozk_vec_len(const cozk_vec* v);
/* raw device pointer (for zero-copy interop with the host's own device buffers, e.g. RCCL staging) */
void* cozk_vec_device_ptr(const cozk_vec* v);
/* SYNTHETIC TEST DATA ONLY (benchmarks, fixtures): element i draws from SplitMix64(seed + i * 0xD1342543DE82EF95):
 * FR = canonical value rejection-sampled below r, stored in Montgomery form; small kinds = low bits.  max_bits > 0
 * masks the value to that many bits (e.g. 1 for 0/1 flags).  SplitMix64 is not a PRF: nothing secret is ever drawn
 * from it -- shares and masks come from the keyed ChaCha12 PRF below. */
int cozk_vec_fill_random(cozk_ctx* ctx, cozk_vec* v, uint64_t seed, int max_bits);

/* Keyed PRF of the engine: PRF(key, j) = element j of the ChaCha12 stream keyed with the 32-byte `key` (one block per
 * element: counter = j, rejection-sampled below r; csrc/prf.hip.hpp).  Keys are what the reference's parties exchange as
 * 32-byte ChaCha seeds (mpc-types/src/protocols/rep3.rs:29,177; mpc-core/src/protocols/rep3/network.rs:190-211) and
 * come from the host's CryptoRng; (key, counter range) pairs must never be reused for different data. */
#define COZK_PRF_KEY_BYTES 32
/* out[i] = PRF(key, counter + i), Montgomery form (FR vector) */
int cozk_vec_fill_prf(cozk_ctx* ctx, cozk_vec* v, const uint8_t key[COZK_PRF_KEY_BYTES], uint64_t counter);
/* Rep3 sharing of a secret vector on the device -- the witness scatter (rep3::share_field_element,
 * mpc-core/src/protocols/rep3/arithmetic.rs:21-33; jolt/vm/../witness.rs generate_poly_shares_rep3):
 * t0[i] = PRF(key0, counter + i), t1[i] = PRF(key1, counter + i), t2 = v - t0 - t1; returns `party`'s (a, b) =
 * (t0, t2) / (t1, t0) / (t2, t1).  The dealer calls it once per party. */
int cozk_rep3_share_vec(cozk_ctx* ctx, const cozk_vec* v, const uint8_t key0[COZK_PRF_KEY_BYTES],
                        const uint8_t key1[COZK_PRF_KEY_BYTES], uint64_t counter, int party,
                        cozk_vec** out_a, cozk_vec** out_b);
/* The witness scatter device to device (jolt/vm/jolt/coordinator.rs:72-91; receive_witness_share in jolt/vm/.../witness.rs):
 * as cozk_rep3_share_vec, but the secret lives on the DEALER's context and the outputs are vectors of `party_ctx` (another
 * GPU, or the same one): generated on the dealer's device, moved by a peer copy over xGMI when the devices differ.
 * Returns after the copy has completed.  The outputs are blocks of party_ctx's allocator: the call drains party_ctx's
 * stream before the dealer's stream writes them, and -- like every call that takes a context -- must come from the
 * thread that owns party_ctx (a context and its allocator are single-owner). */
int cozk_rep3_scatter(cozk_ctx* dealer, const cozk_vec* v, const uint8_t key0[COZK_PRF_KEY_BYTES],
                      const uint8_t key1[COZK_PRF_KEY_BYTES], uint64_t counter, cozk_ctx* party_ctx, int party,
                      cozk_vec** out_a, cozk_vec** out_b);
/* element-wise out[i] = a[i] (op) b[i] on 32-byte field elements: the local arithmetic of
 * mpc-types/src/protocols/additive/ops.rs (AdditivePrimeFieldShare is repr(transparent) over F).
 * base_field = 0: Fr (scalar field, what shares live in); 1: Fq (G1 coordinate field). */
#define COZK_OP_ADD 0
#define COZK_OP_SUB 1
#define COZK_OP_MUL 2
int cozk_vec_binop(cozk_ctx* ctx, int op, int base_field, const cozk_vec* a, const cozk_vec* b,
                   cozk_vec* out);
/* v[i] *= s (Fr) in place */
int cozk_vec_scale(cozk_ctx* ctx, cozk_vec* v, const uint64_t s[4]);
/* v[i] += s (Fr) in place: share + public of the Shamir share type (mpc-types/src/protocols/shamir/arithmetic/ops.rs:41-61) */
int cozk_vec_add_scalar(cozk_ctx* ctx, cozk_vec* v, const uint64_t s[4]);

/* ---------------------------------------------------------------- Shamir shares ----------- */
/* A ShamirPrimeFieldShare is repr(transparent) over F (mpc-types/src/protocols/shamir/arithmetic/types.rs:10-30): party p's
 * share of a vector is ONE FR cozk_vec, its evaluation point is x = p + 1.  The local operators of
 * shamir/arithmetic/ops.rs need no entry points of their own: share +- share and share x share (element-wise; "result has
 * higher degree than the inputs", ops.rs:93-118) are cozk_vec_binop, share x public is cozk_vec_scale, negation is
 * cozk_vec_scale by -1, share + public is cozk_vec_add_scalar; a party's commitment of its share vector is cozk_msm_vec.
 * The element-wise product of two degree-t sharings has degree 2t and can only be opened (from 2t + 1 parties); a product
 * that is a degree-t sharing again, so that products chain, is cozk_shamir_mul_{deal, inproc, vec} below.  The reference has
 * no Shamir network, degree reduction or prover; the multiplication here is the classic one-round resharing (GRR / BGW),
 * restated in tests/shamir_mul_ref.py, and beside it the king variant with preprocessed double-random pairs
 * (cozk_shamir_rand_*, cozk_shamir_mul_king_*; tests/shamir_dn_ref.py).  co-noir-spartan by n Shamir parties is cozk_shamir_spartan_*
 * (behind the co-noir-spartan harness below).  The first Shamir prover is the dense batched grand
 * product at the end of this section: cozk_shamir_gp_prove_inproc (tests/shamir_gp_ref.py) with the resharing construct, and
 * cozk_shamir_gp_prep_inproc + cozk_shamir_gp_prove_king_inproc (tests/shamir_gp_king_ref.py) with the king's. */
#define COZK_SHAMIR_MAX_PARTIES 32
#define COZK_SHAMIR_MAX_DEGREE 15 /* of a dealt sharing: 2t + 1 <= 32 parties can still open a product */
/* share_field_elements (mpc-types/src/protocols/shamir.rs:58-77; `share` :190-207): out[p][i] = f_i(p + 1) with
 * f_i(x) = v[i] + sum_{c=1..degree} coef_c[i] x^c and coef_c[i] = PRF(keys[c-1], counter + i); keys = degree x 32 bytes,
 * out = num_parties handles.  One kernel writes all parties' vectors.  1 <= degree <= COZK_SHAMIR_MAX_DEGREE and
 * degree < num_parties <= COZK_SHAMIR_MAX_PARTIES; on any failure no output handle is left allocated: out[0..num_parties)
 * is NULL, except that out[] is not touched at all when num_parties itself is out of range (its length is then unknown). */
int cozk_shamir_share_vec(cozk_ctx* ctx, const cozk_vec* v, const uint8_t* keys, int degree, int num_parties,
                          uint64_t counter, cozk_vec** out);
/* the same evaluation with the caller's own coefficient vectors, coeffs[0] = the secret vector, coeffs[1..=degree] drawn
 * from the host's CryptoRng: evaluate_poly at x = 1..=num_parties (shamir.rs:166-175; test_shamir_poly :521-552) */
int cozk_shamir_eval_vec(cozk_ctx* ctx, const cozk_vec* const* coeffs, int degree, int num_parties, cozk_vec** out);
/* cozk_shamir_share_vec whose output p is a vector of party_ctxs[p] (the same or another GPU), as cozk_rep3_scatter does
 * for Rep3: every party's stream is drained before the dealer's stream writes, vectors on another device are generated
 * in the dealer's memory and moved by one peer copy each; returns after the copies have completed */
int cozk_shamir_scatter(cozk_ctx* dealer, const cozk_vec* v, const uint8_t* keys, int degree, int num_parties,
                        uint64_t counter, cozk_ctx* const* party_ctxs, cozk_vec** out);
/* lagrange_from_coeff (shamir.rs:273-291): out[i] = prod_{j != i} x_j / (x_j - x_i), k x 4 u64 Montgomery.  Pure host, no
 * context.  1 <= k <= COZK_SHAMIR_MAX_PARTIES; points distinct and in 1..COZK_SHAMIR_MAX_PARTIES (the reference would
 * panic on the inverse of zero). */
int cozk_shamir_lagrange(const uint32_t* points, size_t k, uint64_t* out);
/* combine_field_elements (shamir.rs:80-124): out[i] = sum_{j<=degree} lambda_j * shares[j][i], lambda =
 * lagrange(points[..=degree]); as in the reference only the first degree + 1 of the k shares are used.
 * 0 <= degree < k <= COZK_SHAMIR_MAX_PARTIES (a product of two degree-15 sharings opens with degree 30 from 31 shares);
 * k FR vectors of equal length; points as for cozk_shamir_lagrange. */
int cozk_shamir_combine_vec(cozk_ctx* ctx, const cozk_vec* const* shares, const uint32_t* points, size_t k, int degree,
                            cozk_vec** out);
/* combine_curve_point (shamir.rs:138-163; reconstruct_point :432-440) for the parties' commitments of their share
 * vectors: out = sum_{j<=degree} lambda_j * P_j; xy = k x 8 u64, infinity = k ints or NULL.  Host arithmetic (the code
 * behind cozk_g1_mul / cozk_g1_sum); ctx only receives the error message and may be NULL. */
int cozk_shamir_combine_points(cozk_ctx* ctx, const uint64_t* xy, const int* infinity, const uint32_t* points, size_t k,
                               int degree, uint64_t out_xy[8], int* out_infinity);

/* Shamir multiplication with degree reduction, one round of resharing.  Parties 0..2t (t = degree; the first 2t + 1
 * evaluation points, the convention of combine_field_elements) are the DEALERS: dealer p re-deals its local product
 *   h_{p -> q}[i] = a_p[i] b_p[i] + sum_{c=1..t} PRF(keys_p[c-1], counter + i) (q + 1)^c,   q = 0..n-1,
 * every party q receives h_{p -> q} from every dealer (its own slot stays local) and finishes with
 *   c_q[i] = sum_{p=0..2t} lambda_p h_{p -> q}[i],   lambda = lagrange(1..2t + 1):
 * c is a degree-t sharing of a b.  Traffic: a dealer sends (n - 1) x 32 B per element, one vector per peer.
 *
 * cozk_shamir_mul_deal is a dealer's first step: out[q] = h_{-> q}, num_parties handles in ctx, in ONE launch that folds the
 * product into the dealing kernel of cozk_shamir_share_vec (64 B read, n x 32 B written per element; the product vector is
 * never stored).  keys = this party's `degree` x 32 private bytes; counter discipline and argument rules as for
 * cozk_shamir_share_vec, and in addition 2 * degree + 1 <= num_parties, and a, b are FR vectors of one length.  On any failure
 * out[0..num_parties) is NULL (untouched when num_parties itself is out of range).
 * The finish needs no entry point of its own: with recv[p] = what dealer p sent, it is
 *   cozk_shamir_combine_vec(ctx, recv, points = {1, .., 2t + 1}, k = 2t + 1, degree = 2t, &c). */
int cozk_shamir_mul_deal(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* b, const uint8_t* keys, int degree,
                         int num_parties, uint64_t counter, cozk_vec** out);
/* the whole multiplication for num_parties parties driven from the one thread that owns their contexts (the same or
 * different GPUs), in the style of cozk_shamir_scatter: receive vectors come from each recipient's allocator, every party's
 * stream is drained before a dealer's stream writes another party's blocks (in place on the dealer's device, staged and
 * moved by one peer copy per recipient otherwise), the dealers' streams are synchronised, then each party's finish is
 * enqueued on its own stream.  a[p], b[p]: party p's share vectors, vectors of party_ctxs[p]; keys[p]: party p's
 * `degree` x 32 bytes; for p > 2 * degree none of the three is read and each may be NULL.  out[q] belongs to party_ctxs[q];
 * failure rules as for cozk_shamir_mul_deal, the error text is left with party_ctxs[0]. */
int cozk_shamir_mul_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* a, const cozk_vec* const* b,
                           const uint8_t* const* keys, int degree, int num_parties, uint64_t counter, cozk_vec** out);
/* cozk_shamir_mul_deal for one interleaved GKR layer (Rep3DenseInterleavedPolynomial's layout, L[j] = v[2j], R[j] = v[2j+1]):
 *   out[q][j] = v[2j] v[2j+1] + sum_{c=1..t} PRF(keys[c-1], counter + j) (q + 1)^c,   j < m,
 * for an FR vector v of even length 2m (0 included), in ONE launch of the dealing kernel: 64 B read, contiguous per lane, and
 * n x 32 B written per element; the product vector -- what cozk_layer_output_local would write and cozk_shamir_share_vec read
 * back -- is never stored.  Argument and failure rules as for cozk_shamir_mul_deal; an odd length is refused on the host. */
int cozk_shamir_mul_deal_pairs(cozk_ctx* ctx, const cozk_vec* v, const uint8_t* keys, int degree, int num_parties,
                               uint64_t counter, cozk_vec** out);
/* the whole multiplication of one tree level, out[q][j] = party q's share of v[2j] v[2j+1], for all parties driven from one
 * thread: cozk_shamir_mul_inproc with that source (one driver serves both).  v[p]: party p's share vector of the layer, a
 * vector of party_ctxs[p]; v[p] and keys[p] are not read for p > 2 * degree and may be NULL. */
int cozk_shamir_mul_pairs_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* v, const uint8_t* const* keys,
                                 int degree, int num_parties, uint64_t counter, cozk_vec** out);
/* one party per process over the context's ring (cozk_ring_init with num_parties ranks; this party = the context's rank):
 * a dealer deals, exchanges (cozk_ring_all_to_all) and finishes, a party > 2 * degree receives and finishes; all of it is
 * enqueued on the context's stream and nothing waits on the host.  A dealer needs a, b and keys; another party only a (for
 * the length).  Refused without a ring and when 2 * degree + 1 exceeds the ring's ranks. */
int cozk_shamir_mul_vec(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* b, const uint8_t* keys, int degree,
                        uint64_t counter, cozk_vec** out);

/* Shamir multiplication with a king and preprocessed double-random pairs (Damgard-Nielsen; semi-honest like the rest of the
 * Shamir seam; restated in tests/shamir_dn_ref.py, the reference has none of it).  Against the resharing above, the online step
 * moves 2t vectors into one party and n - 1 out of it instead of (2t + 1)(n - 1), in two rounds instead of one, and everything
 * that needs fresh randomness happens OFFLINE, before the factors exist.  t = degree, n = num_parties, with
 *   1 <= t, 2t <= COZK_SHAMIR_MAX_DEGREE (the degree-2t sharing goes through the dealing kernel too), 2t + 1 <= n <= 32.
 *
 * Offline.  Party p holds 3t + 1 private PRF keys: keys[0] gives its secret stream s_p[i] = PRF(keys[0], counter + i),
 * keys[1..t] the coefficients of a degree-t polynomial f_i, keys[t + 1..3t] those of a degree-2t polynomial g_i, with
 * f_i(0) = g_i(0) = s_p[i] and coefficient c of element i = PRF(key_c, counter + i) as in cozk_shamir_share_vec.  It deals
 * u_{p->q}[i] = f_i(q + 1) and w_{p->q}[i] = g_i(q + 1) to every q; party q then computes, for k = 0..n - t - 1,
 *   rt_q^k[i] = sum_{p=0..n-1} (p + 1)^k u_{p->q}[i]   and likewise r2t_q^k from the w
 * (the (n - t) x n Vandermonde matrix on the points 1..n).  Pair k is (rt^k, r2t^k): a degree-t and a degree-2t sharing of one
 * value that no t parties know.  One exchange yields n - t pairs.  (key, counter range) pairs must not be reused, and A PAIR
 * MUST NEVER BE USED TWICE: using it for two multiplications reveals the difference of the two products.  Both are the
 * caller's contract; there is no pool or bookkeeping object for pairs.
 *
 * cozk_shamir_rand_deal: this party's dealing, out_t[q] = u_{->q} and out_2t[q] = w_{->q}, two tables of num_parties handles
 * in ctx, in two launches of the dealing kernel (degree t, degree 2t) that both recompute the secret: it is never stored.
 * keys = (3 * degree + 1) x 32 bytes.  On any failure both tables are NULL in [0, num_parties) (untouched when num_parties
 * itself is out of range). */
int cozk_shamir_rand_deal(cozk_ctx* ctx, size_t n_elems, const uint8_t* keys, int degree, int num_parties, uint64_t counter,
                          cozk_vec** out_t, cozk_vec** out_2t);
/* the Vandermonde step on ONE set of received vectors: out[k][i] = sum_{j < num_parties} (j + 1)^k recv[j][i], k < count;
 * out = count handles in ctx.  One kernel reads every input once per tile of 8 outputs.  2 <= num_parties <= 32 FR vectors of
 * one length, 1 <= count <= num_parties - 1.  PRIVACY NEEDS count <= n - t where t parties may collude: the drivers below
 * call it once per degree with count = n - t; a larger count is arithmetic only.  As for cozk_shamir_combine_vec the inputs
 * need not be vectors of ctx (a transport may have filled them): they are read on ctx's stream, and ordering that read behind
 * whatever wrote a vector of another context is the caller's job.  On failure out[0..count) is NULL (untouched when count is
 * outside 1..32). */
int cozk_shamir_rand_extract(cozk_ctx* ctx, const cozk_vec* const* recv, int num_parties, int count, cozk_vec** out);
/* the whole preprocessing for num_parties parties driven from the one thread that owns their contexts (the same or different
 * GPUs), in the style of cozk_shamir_mul_inproc, one degree after the other: receive vectors from the recipients' allocators,
 * every party's stream drained before a dealer's stream writes another party's block (in place on the dealer's device, staged
 * and moved by one peer copy per recipient otherwise), the dealers' streams synchronised, then each party's extraction on its
 * own stream.  keys[p] = party p's (3 * degree + 1) x 32 bytes.  r_t[q * (n - t) + k] and r_2t[q * (n - t) + k] are party q's
 * halves of pair k, vectors of party_ctxs[q].  On failure both tables are NULL in [0, n (n - t)) (untouched when
 * 1 <= degree < num_parties <= 32 does not hold: their length is then unknown); the error text is left with party_ctxs[0]. */
int cozk_shamir_rand_inproc(cozk_ctx* const* party_ctxs, const uint8_t* const* keys, size_t n_elems, int degree,
                            int num_parties, uint64_t counter, cozk_vec** r_t, cozk_vec** r_2t);
/* one party per process over the context's ring (num_parties = its ranks, this party = the context's rank): deal, two
 * cozk_ring_all_to_all (one per degree; the own slot stays local), two extractions; all of it is enqueued on the context's
 * stream and nothing waits on the host.  r_t, r_2t: ranks - degree handles each; NULL on failure where that length is known
 * (a ring and 1 <= degree < ranks), untouched otherwise. */
int cozk_shamir_rand_vec(cozk_ctx* ctx, size_t n_elems, const uint8_t* keys, int degree, uint64_t counter, cozk_vec** r_t,
                         cozk_vec** r_2t);
/* Online, consuming ONE pair.  The SENDERS are parties 0..2t (the convention of combine_field_elements and of the dealers
 * above); `king` is any party 0..n - 1.
 *   1. sender p computes m_p[i] = a_p[i] b_p[i] + r2t_p[i] and (unless it is the king) sends it to the king;
 *   2. the king opens z = sum_{p<=2t} lambda_p m_p, lambda = lagrange(1..2t + 1) (cozk_shamir_combine_vec at degree 2t):
 *      z = a b + r is public;
 *   3. the king sends z to everyone, and party q's result is c_q = z - rt_q: a degree-t sharing of a b.
 * A party above 2t needs neither factors nor r2t (whether or not it is the king).
 *
 * cozk_shamir_mul_mask is step 1 in ONE launch, *out = a b + r_2t (96 B read, 32 B written per element; the product is never
 * stored): three FR vectors of one length; *out is NULL on failure. */
int cozk_shamir_mul_mask(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* b, const cozk_vec* r_2t, cozk_vec** out);
/* the whole online step with all parties in this process: the mask on each sender's own stream, written into the king's
 * memory (in place on the king's device, staged and peer-copied from another), the senders' streams synchronised, the combine
 * on the king's stream, z copied to the parties of other devices by that stream, which is then synchronised (parties of the
 * king's device read z in place), the subtraction on each party's own stream; the streams that read z in place are
 * synchronised before the king's pool takes it back.  a[p], b[p], r_2t[p] (p <= 2 * degree) and r_t[p] (every p) must be FR
 * vectors of party_ctxs[p] of one length; a[p], b[p], r_2t[p] are not read for p > 2 * degree and may be NULL.  out[q] belongs
 * to party_ctxs[q]; on failure out[0..num_parties) is NULL (untouched when num_parties is outside 1..32); the error text is
 * left with party_ctxs[0]. */
int cozk_shamir_mul_king_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* a, const cozk_vec* const* b,
                                const cozk_vec* const* r_t, const cozk_vec* const* r_2t, int degree, int num_parties, int king,
                                cozk_vec** out);
/* one party per process over the context's ring: two cozk_ring_all_to_all with empty slots -- the gather to the king, the
 * king's fan-out -- around the king's combine, then the subtraction; stream-ordered, no host wait.  Every party needs r_t (it
 * also gives the length); a party 0..2 * degree also a, b and r_2t; all must be vectors of ctx.  *out is NULL on failure. */
int cozk_shamir_mul_king_vec(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* b, const cozk_vec* r_t, const cozk_vec* r_2t,
                             int degree, int king, cozk_vec** out);
/* The king multiplication of one interleaved GKR layer (L[j] = v[2j], R[j] = v[2j+1]; a tree level of the king grand product
 * below), with the halves of the pair addressed by an ELEMENT OFFSET so that one preprocessed pair serves many levels and no
 * slice is copied.  Element off + j of a pair is used by product j; no element of a pair may be used twice.
 *
 * cozk_shamir_mul_mask_pairs: *out[j] = v[2j] v[2j+1] + r_2t[r_offset + j], len(v) / 2 elements in ONE launch (96 B read, 32 B
 * written per product; the product is never stored).  v is an even-length FR vector, r_2t an FR vector with
 * r_offset + len(v) / 2 <= len(r_2t).  *out is NULL on failure. */
int cozk_shamir_mul_mask_pairs(cozk_ctx* ctx, const cozk_vec* v, const cozk_vec* r_2t, size_t r_offset, cozk_vec** out);
/* the king's open and `count` parties' unmask in ONE launch: z[i] = sum_{p<=2t} lambda_p masked[p][i], lambda =
 * lagrange(1..2t + 1), t = degree, and out[q][i] = z[i] - r_t[q][r_offset + i] for q < count; z itself is stored only when
 * z_out is not NULL.  (2t + 1 + count) x 32 B read, count x 32 B written per element, every stored element canonical.
 * 1 <= degree <= COZK_SHAMIR_MAX_DEGREE (arithmetic only, as for cozk_shamir_combine_vec), 1 <= count <= 32; masked: 2t + 1 FR
 * vectors of one length n; r_t: count FR vectors with r_offset + n <= their lengths.  As for cozk_shamir_rand_extract the inputs
 * need not be vectors of ctx (they are read on ctx's stream, and ordering that read is the caller's job); out[0..count) and
 * *z_out are handles of ctx, NULL on failure (out untouched when count is outside 1..32). */
int cozk_shamir_king_finish(cozk_ctx* ctx, const cozk_vec* const* masked, int degree, const cozk_vec* const* r_t, size_t r_offset,
                            int count, cozk_vec** out, cozk_vec** z_out);
/* one tree level for all parties in this process: out[q][j] = party q's share of v[2j] v[2j+1], a degree-t sharing again.  As
 * cozk_shamir_mul_king_inproc: every stream drained, cozk_shamir_mul_mask_pairs' kernel on each sender's stream into the king's
 * blocks (staged and peer-copied from another device), the senders' streams synchronised; then ONE cozk_shamir_king_finish
 * launch on the king's stream serves every party of the king's device, writing into blocks of the recipients' allocators, and
 * that stream is synchronised before return.  A party on another device gets z by peer copy and subtracts at the offset on its
 * own stream.  v[p] (even length, one length) and r_2t[p] are read for p <= 2 * degree only and may be NULL above; r_t[p] for
 * every p; all halves have one length >= r_offset + len(v) / 2 and are vectors of party_ctxs[p].  1 <= t, 2t <=
 * COZK_SHAMIR_MAX_DEGREE, 2t + 1 <= n <= 32, 0 <= king < n.  On failure out[0..num_parties) is NULL (untouched when num_parties
 * is outside 1..32); the error text is left with party_ctxs[0]. */
int cozk_shamir_mul_king_pairs_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* v, const cozk_vec* const* r_t,
                                      const cozk_vec* const* r_2t, size_t r_offset, int degree, int num_parties, int king,
                                      cozk_vec** out);

/* The dense batched grand product (GKR; Rep3BatchedDenseGrandProduct, co-jolt/src/subprotocols/grand_product.rs) proved by n
 * Shamir parties, semi-honest, all driven from the one thread that owns their contexts and plays the coordinator
 * (csrc/host/shamir_gp.hpp; restated in tests/shamir_gp_ref.py; the reference has no Shamir prover).  Every sumcheck term
 * multiplies at most two secret factors (eq is public), so each party runs the COZK_MODE_PLAIN layer kernels on its share
 * vectors with the PUBLIC claim as prev_claim and holds a degree-2t sharing of the plain prover's message: THE PROOF IS
 * BYTE-IDENTICAL TO THE PLAIN PROVER'S PROOF OF THE SAME WITNESS, transcript order and layout those of the Rep3 coordinator.
 *   construct  layer[0] = leaves, layer[i+1] = cozk_shamir_mul_pairs_inproc(layer[i]), log2(per circuit) - 1 levels; level i
 *              uses the counter mul_counter + sum of the earlier levels' output lengths.
 *   masks      M = batch_size + 4 sum_layers rounds(layer) openings of degree 2t.  Opening a locally computed degree-2t
 *              sharing leaks more than its value unless it is re-randomised: ONE cozk_shamir_rand_inproc of M elements at
 *              rand_counter, pair 0 only, zero_p[m] = r2t_p^0[m] - rt_p^0[m] (a degree-2t sharing of zero).  As for
 *              cozk_shamir_mul_king_*, A PAIR MUST NEVER BE USED TWICE: (rand_keys, rand_counter .. rand_counter + M) must
 *              not be used again, by another proof or by a king multiplication -- the caller's contract, like
 *              (mul_keys, mul_counter .. + sum of the levels' lengths).
 *   openings   indexed m = 0, 1, .. in the order opened: the batch_size outputs (cozk_layer_claimed_outputs of the top layer),
 *              then layer by layer from the top, round by round, coefficients 0..3 of cozk_layer_round.  Sender p <= 2t sends
 *              local_p + zero_p[m]; the coordinator combines with lagrange(1..2t + 1).
 *   finals     L, R of cozk_layer_final_claims after the last bind: linear combinations of freshly dealt degree-t sharings,
 *              opened from parties 0..t with lagrange(1..t + 1), unmasked.
 * Parties above 2t receive their share of every level and send nothing.  leaves[p]: party p's FR share vector of the
 * interleaved leaves, a vector of party_ctxs[p], copied and never modified; mul_keys[p] = t x 32 bytes (both read for
 * p <= 2t only); rand_keys[p] = (3t + 1) x 32 bytes, every party.  Preconditions: batch_size > 0 divides the length, leaves
 * per circuit a power of two >= 2 (Rep3BatchedDenseGrandProduct::construct), 1 <= t, 2t <= COZK_SHAMIR_MAX_DEGREE,
 * 2t + 1 <= n <= 32; everything is refused on the host before any launch.  On failure *out is NULL and the error text is left
 * with party_ctxs[0].  verify != 0 replays the plain verifier on a fresh transcript with the same label. */
typedef struct cozk_shamir_gp cozk_shamir_gp;
typedef struct cozk_shamir_gp_result {
    int verified;          /* 1 accepted, 0 rejected, -1 verifier not run */
    int n_layers;
    uint64_t proof_len;
    uint64_t n_opened;     /* M */
    double t_construct_ms; /* host clock around the construction, every party's stream drained at both ends */
    double t_prove_ms;     /* the same around masks + openings + rounds; one thread drives the parties in turn: a SUM over parties */
} cozk_shamir_gp_result;
int cozk_shamir_gp_prove_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* leaves, size_t batch_size,
                                const uint8_t* const* mul_keys, const uint8_t* const* rand_keys, int degree, int num_parties,
                                uint64_t mul_counter, uint64_t rand_counter, const char* label, int verify,
                                cozk_shamir_gp** out);
int cozk_shamir_gp_free(cozk_shamir_gp* h);
int cozk_shamir_gp_get_result(const cozk_shamir_gp* h, cozk_shamir_gp_result* res);
/* How the rounds ran.  When the 2t + 1 senders' contexts are on one device, a layer's sumcheck is ONE layer group over the senders'
 * layers with ONE eq polynomial on sender 0's context: a cozk_layer_group_round per round and a cozk_layer_group_final with
 * k_final = t + 1 (group_*: calls made).  Otherwise, or with COZK_SHAMIR_GP_GROUP=0 in the environment (read on every call, for
 * A/B runs within one process), every sender runs cozk_layer_round on an eq of its own and every opener cozk_layer_bind +
 * cozk_layer_final_claims (single_rounds: per sender and round; single_finals: per opener and layer).  Proof, msgs and finals
 * are the same bytes either way. */
typedef struct cozk_shamir_gp_stats {
    uint64_t group_rounds, single_rounds, group_finals, single_finals;
} cozk_shamir_gp_stats;
int cozk_shamir_gp_get_stats(const cozk_shamir_gp* h, cozk_shamir_gp_stats* stats);
int cozk_shamir_gp_proof_bytes(const cozk_shamir_gp* h, uint8_t* out, size_t cap); /* cap >= proof_len bytes */
/* the final (claim, r): r = point_len x 4 u64 */
size_t cozk_shamir_gp_point_len(const cozk_shamir_gp* h);
int cozk_shamir_gp_final(const cozk_shamir_gp* h, uint64_t claim[4], uint64_t* r);
/* what went over the star, for tests and audits: msgs[m][p] = sender p's masked message of opening m, M x (2t + 1) elements;
 * finals[layer, top first][p][L, R] = opener p's final-claim shares, layers x (t + 1) x 2 elements.  *_len in elements;
 * out = len x 4 u64 Montgomery, cap in elements. */
size_t cozk_shamir_gp_msgs_len(const cozk_shamir_gp* h);
int cozk_shamir_gp_msgs(const cozk_shamir_gp* h, uint64_t* out, size_t cap);
size_t cozk_shamir_gp_finals_len(const cozk_shamir_gp* h);
int cozk_shamir_gp_finals(const cozk_shamir_gp* h, uint64_t* out, size_t cap);

/* The same proof with the KING construct and everything that needs fresh randomness moved OFFLINE, before the leaves exist.
 * cozk_shamir_gp_prep_inproc makes the preprocessing object of ONE proof of (n_leaves, batch_size) by (num_parties, degree):
 *   (A) the opening masks of cozk_shamir_gp_prove_inproc: M elements at rand_counter, pair 0 -- the same zero masks;
 *   (B) one dealing of n_leaves / 2 elements at rand_counter + M: pair 0 serves tree level 0 whole, pair 1 serves level
 *       i >= 1 at the element offset n_leaves / 2 - n_leaves / 2^i (the sum of the output lengths of levels 1..i - 1; the last
 *       level ends at n_leaves / 2 - 2 batch_size).  Only what is used is extracted: no pair for 2 leaves per circuit, one for
 *       4, two otherwise (fewer than n - t pairs of an exchange are still private), the degree-2t halves for parties 0..2t only.
 * (rand_keys, rand_counter .. rand_counter + M + n_leaves / 2) must never be used again: the caller's contract.  rand_keys[p] =
 * (3t + 1) x 32 bytes, every party.  The object holds vectors of party_ctxs: free it before those contexts are destroyed.
 * cozk_shamir_gp_prove_king_inproc consumes it: construct layer[i+1] = cozk_shamir_mul_king_pairs_inproc(layer[i], ..) at
 * those offsets; masks, openings, finals (unmasked: c_q = z - rt_q is a fresh uniformly random degree-t sharing), transcript
 * and proof are those of cozk_shamir_gp_prove_inproc, so THE PROOF IS THE PLAIN PROVER'S, BYTE FOR BYTE, and the handle is the
 * same cozk_shamir_gp with every getter above; t_construct_ms is the online construct alone (offline time lives in the prep's
 * result).  party_ctxs, the length of the leaves and batch_size must be those the prep was made for; the prep is marked used
 * before the first launch and a second proof with it is refused with COZK_ERR_INVALID_ARG.  Everything is refused on the host
 * before any launch; on failure *prep / *out is NULL and the error text is left with party_ctxs[0]. */
typedef struct cozk_shamir_gp_prep cozk_shamir_gp_prep;
typedef struct cozk_shamir_gp_prep_result {
    uint64_t n_openings; /* M */
    uint64_t pair_elems; /* elements per construct pair: n_leaves / 2, or 0 where no pair is needed */
    int pairs_held;      /* construct pairs still held: 0, 1 or 2; 0 once a proof has consumed them */
    int used;            /* 1 once a proof has started with it */
    double t_offline_ms; /* host clock around both dealings, every party's stream drained at both ends */
} cozk_shamir_gp_prep_result;
int cozk_shamir_gp_prep_inproc(cozk_ctx* const* party_ctxs, const uint8_t* const* rand_keys, size_t n_leaves, size_t batch_size,
                               int degree, int num_parties, uint64_t rand_counter, cozk_shamir_gp_prep** prep);
int cozk_shamir_gp_prep_free(cozk_shamir_gp_prep* prep);
int cozk_shamir_gp_prep_get_result(const cozk_shamir_gp_prep* prep, cozk_shamir_gp_prep_result* res);
int cozk_shamir_gp_prove_king_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* leaves, size_t batch_size,
                                     cozk_shamir_gp_prep* prep, int king, const char* label, int verify, cozk_shamir_gp** out);

/* The TOGGLED batched grand product (Rep3ToggledBatchedGrandProduct, co-jolt/src/subprotocols/sparse_grand_product.rs; the read /
 * write half of Lasso's memory checking) proved by the same n Shamir parties (csrc/host/shamir_gp.hpp; restated in
 * tests/shamir_tgp_ref.py).  flags: n_pairs public 0/1 U8 columns of N entries, vectors of party_ctxs[0]; fingerprints[p]: party
 * p's FR share vector of the 2 n_pairs x N fingerprints, a vector of party_ctxs[p], read for p <= 2t and never modified.  The
 * flags are public, so the toggle layer's output and round polynomial are affine in the fingerprint share: the PLAIN toggle calls
 * on a degree-t share, with the public claim as previous claim, give a degree-t sharing of the plain prover's values.
 *   construct  level 0 = the senders' toggle outputs (flag ? fingerprint : 1), adopted; above it the dense construct of
 *              cozk_shamir_gp_prove_inproc, with either multiplication.
 *   masks      batch B = 2 n_pairs, nv = ceil_log2(B), N = 2^d: the toggle layer has nv + d rounds, so M = M_dense(B N, B) +
 *              4 (nv + d), still ONE dealing at rand_counter, pair 0.
 *   rounds     the dense layers as they are; then the toggle layer as coordinate_prove_toggle_layer sees it (no r_layer, no claim
 *              fold): each sender's four coefficients are unipoly_from_evals(g0, claim - g0, g2, g3) of its toggle round, opened
 *              from senders 0..2t with the same zero masks, continuing the opening order.
 *   finals     the flag claim is public; the fingerprint claim is opened from parties 0..t, unmasked; the t + 1 pairs
 *              (flag, share) are appended to `finals`.
 * Transcript and proof are those of the Rep3 coordinator's toggled prover, THE PROOF IS THE PLAIN PROVER'S, BYTE FOR BYTE, and
 * verify != 0 replays the plain toggled verifier.  The handle is the same cozk_shamir_gp with every getter above (claim = the
 * toggle sumcheck's last claim, r = its point); n_layers counts the toggle layer; t_construct_ms includes the toggle outputs.
 * When the senders' contexts are on one device the toggle layer runs as ONE cozk_toggle_group on sender 0's context with one eq;
 * otherwise, or with COZK_SHAMIR_GP_GROUP=0, every sender gets the flags on its own context and a PLAIN cozk_toggle of its own.
 * cozk_shamir_tgp_prep_inproc (n_per = N) makes the king's preprocessing for this larger M, its pairs at rand_counter + M; it is
 * marked toggled: cozk_shamir_gp_prove_king_inproc refuses it and cozk_shamir_tgp_prove_king_inproc refuses a dense one.
 * Preconditions and failure behaviour are those of the dense provers. */
int cozk_shamir_tgp_prove_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* flags, size_t n_pairs,
                                 const cozk_vec* const* fingerprints, const uint8_t* const* mul_keys,
                                 const uint8_t* const* rand_keys, int degree, int num_parties, uint64_t mul_counter,
                                 uint64_t rand_counter, const char* label, int verify, cozk_shamir_gp** out);
int cozk_shamir_tgp_prep_inproc(cozk_ctx* const* party_ctxs, const uint8_t* const* rand_keys, size_t n_pairs, size_t n_per,
                                int degree, int num_parties, uint64_t rand_counter, cozk_shamir_gp_prep** prep);
int cozk_shamir_tgp_prove_king_inproc(cozk_ctx* const* party_ctxs, const cozk_vec* const* flags, size_t n_pairs,
                                      const cozk_vec* const* fingerprints, cozk_shamir_gp_prep* prep, int king,
                                      const char* label, int verify, cozk_shamir_gp** out);
/* the toggle layer's final claims of a toggled proof; COZK_ERR_INVALID_ARG on a dense proof's handle */
int cozk_shamir_gp_toggle_claims(const cozk_shamir_gp* h, uint64_t flag[4], uint64_t fingerprint[4]);
/* how the toggle layer's rounds ran: calls of cozk_toggle_group_round, and of cozk_toggle_round per sender and round */
typedef struct cozk_shamir_gp_toggle_stats {
    uint64_t toggle_group_rounds, toggle_single_rounds;
} cozk_shamir_gp_toggle_stats;
int cozk_shamir_gp_get_toggle_stats(const cozk_shamir_gp* h, cozk_shamir_gp_toggle_stats* stats);

/* ---------------------------------------------------------------- MSM seam ---------------- */
/* Upload SRS points (`ck.powers_of_g[i]`, co-jolt/src/poly/commitment/pst13.rs:286-287,461-462) once;
 * replaces the ICICLE `gpu_bases: Option<&[GpuBaseType]>` argument (pst13.rs:52-59,288,320).
 * xy = n x 8 u64 (x[4], y[4]); infinity = n bytes or NULL.  precompute != 0 additionally builds the
 * window table 2^(16w) * G_i (16 x n x 64 B of HBM) that merges all Pippenger windows into one
 * bucket set. */
int cozk_bases_upload(cozk_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, size_t n,
                      int precompute, cozk_bases** out);
/* bases[i] = scalars[i] * g on device -- `MultilinearPC::setup` building `powers_of_g`
 * (ark-poly-commit, invoked by PST13::setup co-jolt/src/poly/commitment/pst13.rs:49-62).
 * g_xy = affine generator (8 u64). */
int cozk_bases_from_scalars(cozk_ctx* ctx, const cozk_vec* scalars_fr, const uint64_t* g_xy,
                            int precompute, cozk_bases** out);
int cozk_bases_download(cozk_ctx* ctx, const cozk_bases* b, size_t offset, size_t n, uint64_t* xy,
                        uint8_t* infinity);
int cozk_bases_free(cozk_bases* b);
size_t cozk_bases_len(const cozk_bases* b);
/* G'[b] = G[2b] + G[2b+1]: folds the duplicated scalars `q[k][x >> 1]` of PST13 `open`
 * (pst13.rs:459) into a half-size MSM */
int cozk_bases_pair_sums(cozk_ctx* ctx, const cozk_bases* b, int precompute, cozk_bases** out);

/* `VariableBaseMSM::msm_field_elements(bases[offset..offset+n], _, scalars, _, _)`
 * (call sites pst13.rs:286-294,461-469; co-noir-spartan/co-spartan/src/worker.rs:801-804).
 * Host-scalar form (PCIe inclusive) and device-resident form. */
int cozk_msm(cozk_ctx* ctx, const cozk_bases* bases, size_t offset, const void* host_scalars,
             int kind, size_t n, uint64_t out_xy[8], int* out_infinity);
int cozk_msm_vec(cozk_ctx* ctx, const cozk_bases* bases, size_t offset, const cozk_vec* scalars,
                 uint64_t out_xy[8], int* out_infinity);
/* `VariableBaseMSM::batch_msm(bases[..n], _, polys)` (pst13.rs:319-323): k MSMs over one base
 * slice; out_xy = k x 8 u64, out_infinity = k ints. */
int cozk_batch_msm_vec(cozk_ctx* ctx, const cozk_bases* bases, size_t offset,
                       const cozk_vec* const* scalars, size_t k, uint64_t* out_xy,
                       int* out_infinity);

/* k MSMs with a different base slice per polynomial: poly i runs over bases[offsets[i] .. +lens[i])
 * (lens = NULL: each vector's full length).  One launch set for all `nv` MSMs of PST13 `open`
 * (pst13.rs:445-471), whose levels live concatenated in one bases handle. */
int cozk_batch_msm_slices(cozk_ctx* ctx, const cozk_bases* bases, const size_t* offsets,
                          const cozk_vec* const* scalars, const size_t* lens, size_t k,
                          uint64_t* out_xy, int* out_infinity);

/* G1 helpers used by the coordinator-side combine (`combine_commitment_shares`, pst13.rs:72-108;
 * `coordinate_prove`, :110-122): out = sum of k affine points */
int cozk_g1_sum(cozk_ctx* ctx, const uint64_t* xy, const int* infinity, size_t k,
                uint64_t out_xy[8], int* out_infinity);
/* out = s * P (host helper for `combine_commitments`, pst13.rs:333-348, and trapdoor checks) */
int cozk_g1_mul(cozk_ctx* ctx, const uint64_t xy[8], int infinity, const uint64_t s[4],
                uint64_t out_xy[8], int* out_infinity);

/* ---------------------------------------------------------------- polynomial seam ---------- */
typedef struct cozk_poly cozk_poly;       /* Rep3DensePolynomial (co-jolt/src/poly/dense_mlpoly.rs:23-32); PLAIN = DensePolynomial */
typedef struct cozk_layer cozk_layer;     /* Rep3DenseInterleavedPolynomial (co-jolt/src/poly/dense_interleaved_poly.rs:35-48) */
typedef struct cozk_spliteq cozk_spliteq; /* SplitEqPolynomial (jolt-core; used dense_interleaved_poly.rs:218-303) */

/* Rep3DensePolynomial::from_vec_shares(a, b) (dense_mlpoly.rs:77-84); b = NULL for MODE_PLAIN. Copies. */
int cozk_poly_create(cozk_ctx* ctx, int mode, const cozk_vec* a, const cozk_vec* b, cozk_poly** out);
/* split_poly: zero-copy chunk over the high variables (dense_mlpoly.rs:275-301) */
int cozk_poly_chunk(cozk_ctx* ctx, const cozk_poly* src, size_t offset, size_t len, cozk_poly** out);
int cozk_poly_free(cozk_poly* p);
size_t cozk_poly_len(const cozk_poly* p);
int cozk_poly_mode(const cozk_poly* p);
/* current (bound) coefficients -> host; a, b = len x 4 u64 */
int cozk_poly_download(cozk_ctx* ctx, const cozk_poly* p, uint64_t* a, uint64_t* b);
/* copy_share_a (dense_mlpoly.rs:103-110) as a zero-copy view: component 0 = a, 1 = b */
int cozk_poly_share_view(cozk_ctx* ctx, const cozk_poly* p, int component, cozk_vec** out);
/* PolynomialBinding::bind / bind_parallel (dense_mlpoly.rs:310-459) */
int cozk_poly_bind(cozk_ctx* ctx, cozk_poly* p, const uint64_t r[4], int order);
/* get_bound_coeff / final_sumcheck_claim (dense_mlpoly.rs:251-257,461-465) */
int cozk_poly_get_coeff(cozk_ctx* ctx, const cozk_poly* p, size_t index, uint64_t a[4], uint64_t b[4]);
/* EqPolynomial::evals(r) on device, big-endian (use: dense_mlpoly.rs:149-153,183-185) */
int cozk_eq_evals(cozk_ctx* ctx, const uint64_t* r, int nv, cozk_vec** out);
/* batch_evaluate / evaluate_at_chi (dense_mlpoly.rs:160-192): out[k] = additive share of poly_k . chi */
int cozk_poly_batch_evaluate_at_chi(cozk_ctx* ctx, const cozk_poly* const* polys, size_t k,
                                    const cozk_vec* chi, uint64_t* out);
/* dot_product_with_public (dense_mlpoly.rs:228-234) -> share (a, b) */
int cozk_poly_dot_product_with_public(cozk_ctx* ctx, const cozk_poly* p, const cozk_vec* pub,
                                      uint64_t a[4], uint64_t b[4]);
/* linear_combination (dense_mlpoly.rs:195-226; multilinear_polynomial.rs:196-296); PLAIN inputs in a
 * REP3 combination are public polynomials added via add_public for `party_id` */
int cozk_poly_linear_combination(cozk_ctx* ctx, const cozk_poly* const* polys, const uint64_t* coeffs,
                                 size_t k, int out_mode, int party_id, cozk_poly** out);
/* compute_leaves of the memory-checking instances (K11; co-jolt/src/jolt/vm/bytecode/worker.rs:57-100,
 * read_write_memory/worker.rs:207-300): leaf[i] = sum_k col_coeffs[k] * cols[k][i] (compact public columns: U8 /
 * U16 / U32 / U64 vectors, CompactPolynomial::field_mul) + sum_j poly_coeffs[j] * polys[j][i] (shared or public
 * Fr polynomials, mul_public) + constant (e.g. -tau).  In MODE_REP3 the public part enters through add_public
 * (party 0's a, party 1's b).  Writes n leaves at out_a / out_b[offset ..] (out_b NULL for MODE_PLAIN), so the leaves
 * of a batch land in one buffer that cozk_layer_create adopts. */
int cozk_fingerprint_leaves(cozk_ctx* ctx, const cozk_vec* const* cols, const uint64_t* col_coeffs, size_t n_cols,
                            const cozk_poly* const* polys, const uint64_t* poly_coeffs, size_t n_polys,
                            const uint64_t constant[4], int mode, int party_id, cozk_vec* out_a, cozk_vec* out_b,
                            size_t offset, size_t n);
/* compute_quadratic inner sums for the live openings of one round (opening_proof.rs:374-414):
 * out[2i] = eval_0, out[2i+1] = eval_2 (additive) */
int cozk_open_quadratic_evals(cozk_ctx* ctx, const cozk_poly* const* polys,
                              const cozk_poly* const* eqs, size_t k, uint64_t* out);
/* one round of prove_arbitrary_worker's evaluation loop (co-jolt/src/subprotocols/sumcheck.rs:189-215) for
 * the comb_funcs the reference uses: a product of m <= 4 polynomials, at most one of them REP3 (Spartan
 * inner / shift sumchecks r1cs/spartan/worker.rs:162-235; output check read_write_memory/worker.rs:149-164).
 * out[e] = additive evaluation at x = 0, 2, .., degree; HighToLow (sumcheck_evals, dense_mlpoly.rs:113-147) */
int cozk_prod_sumcheck_evals(cozk_ctx* ctx, const cozk_poly* const* polys, size_t m, int degree,
                             uint64_t* out);
/* co-noir-spartan: Rep3Sumcheck::first_sumcheck_prove_round evaluations at X = 0..3 of
 * sum_b eq * (za x zb) - into_additive(zc * eq), before the additive zero-mask
 * (co-noir-spartan/co-spartan/src/sumcheck.rs:171-280); fix_variables = cozk_poly_bind(.., LOW_TO_HIGH)
 * on the SoA components (mpc-core/src/protocols/rep3/poly.rs:56-62) */
int cozk_spartan_first_round(cozk_ctx* ctx, const cozk_poly* za, const cozk_poly* zb,
                             const cozk_poly* zc, const cozk_poly* pub, uint64_t out[16]);
/* Rep3Sumcheck::second_sumcheck_prove_round: Rep3 evaluations at X = 0..2 of
 * sum_b z * (alpha A + beta B + gamma C), before the Rep3 mask (sumcheck.rs:282-395) */
int cozk_spartan_second_round(cozk_ctx* ctx, const cozk_poly* z, const cozk_poly* a, const cozk_poly* b,
                              const cozk_poly* c, const uint64_t coef[12], uint64_t out_a[12],
                              uint64_t out_b[12]);
/* SpartanProverWorker::zero_round (co-spartan/src/worker.rs:153-182): (za, zb, zc) = (A, B, C) z on shares;
 * CSR rows: row_ptr (U32, nrows+1), col (U32, nnz), val_a/b/c (FR, nnz).
 * PRECONDITIONS (not checked): row_ptr is non-decreasing from 0 to nnz and every col[e] < z's length.  The kernels read
 * z[col[e]] as it stands, so a larger column is an out-of-bounds device read (the reference panics there). */
int cozk_sparse_matvec3(cozk_ctx* ctx, const cozk_vec* row_ptr, const cozk_vec* col,
                        const cozk_vec* val_a, const cozk_vec* val_b, const cozk_vec* val_c,
                        const cozk_poly* z, cozk_poly** out_za, cozk_poly** out_zb, cozk_poly** out_zc);
/* one fold of PST13 `open` (pst13.rs:445-459): q[b] = r[2b+1]-r[2b]; r'[b] = r[2b](1-p) + r[2b+1]p */
int cozk_pst_fold(cozk_ctx* ctx, const cozk_vec* r, const uint64_t p[4], cozk_vec* q, cozk_vec* r_next);

/* Rep3DenseInterleavedPolynomial::new (dense_interleaved_poly.rs:61-75); take_ownership != 0 adopts
 * the vectors' device buffers instead of copying (the vectors become empty views) */
int cozk_layer_create(cozk_ctx* ctx, int mode, const cozk_vec* a, const cozk_vec* b,
                      int take_ownership, cozk_layer** out);
int cozk_layer_free(cozk_layer* l);
size_t cozk_layer_len(const cozk_layer* l);
int cozk_layer_download(cozk_ctx* ctx, const cozk_layer* l, uint64_t* a, uint64_t* b);
int cozk_layer_clone(cozk_ctx* ctx, const cozk_layer* src, cozk_layer** out);
/* Rep3Bindable::bind (dense_interleaved_poly.rs:155-195) */
int cozk_layer_bind(cozk_ctx* ctx, cozk_layer* l, const uint64_t r[4]);
/* Rep3BatchedCubicSumcheckWorker::compute_cubic (dense_interleaved_poly.rs:210-365): 4 additive
 * coefficient shares (low -> high) of the round polynomial */
int cozk_layer_compute_cubic(cozk_ctx* ctx, const cozk_layer* l, const cozk_spliteq* eq,
                             const uint64_t prev_claim[4], uint64_t out_coeffs[16]);
/* one round of Rep3BatchedCubicSumcheckWorker::prove_sumcheck (co-jolt/src/subprotocols/sumcheck.rs:107-122) in
 * one call: Rep3Bindable::bind + SplitEqPolynomial::bind with the previous round's challenge r (NULL in the first
 * round), then compute_cubic; small layers run as a single launch */
int cozk_layer_round(cozk_ctx* ctx, cozk_layer* l, cozk_spliteq* eq, const uint64_t* r,
                     const uint64_t prev_claim[4], uint64_t out_coeffs[16]);
/* the whole round loop of prove_sumcheck (sumcheck.rs:96-131) for one layer, the host's transport as a callback:
 * per round cb(user, round, coeffs[4x4], r_out[4], next_claim_out[4]) sends the round polynomial's coefficient
 * shares and returns the challenge and this party's additive share of the next claim (0 = ok).  Large rounds
 * are one launch each; the tail of the layer (<= 2048 elements) runs in one resident kernel that trades sums and
 * challenges with the host through pinned memory.  out_r = num_rounds x 4; final_claims = L.a, L.b, R.a, R.b.
 * The call binds num_rounds times.  What its rounds would refuse half-way is asked before the first one -- eq must have at
 * least num_rounds unbound variables, and num_rounds binds must leave the layer at 2 elements -- so a refused call
 * (COZK_ERR_INVALID_ARG) has not called cb and leaves the layer and eq as they were. */
typedef int (*cozk_round_cb)(void* user, int round, const uint64_t coeffs[16], uint64_t r_out[4],
                             uint64_t next_claim_out[4]);
int cozk_layer_prove_rounds(cozk_ctx* ctx, cozk_layer* l, cozk_spliteq* eq, const uint64_t claim[4],
                            int num_rounds, cozk_round_cb cb, void* user, uint64_t* out_r,
                            uint64_t final_claims[16]);
/* the same loop for a worker sub-net (jolt/vm/instruction_lookups/worker.rs:593-597): the callback gets the raw sums
 * g(0), g(2), g(3) of its chunk -- the coordinator inserts g(1) = claim - g(0) -- and returns the challenge */
typedef int (*cozk_round_evals_cb)(void* user, int round, const uint64_t evals[12], uint64_t r_out[4]);
int cozk_layer_prove_rounds_evals(cozk_ctx* ctx, cozk_layer* l, cozk_spliteq* eq, int num_rounds,
                                  cozk_round_evals_cb cb, void* user, uint64_t* out_r,
                                  uint64_t final_claims[16]);
/* raw sums g(0), g(2), g(3) of compute_cubic (12 u64) for worker sub-nets: the coordinator inserts
 * claim - g(0) itself, as for the reference's primary sumcheck (instruction_lookups/worker.rs:593-597) */
int cozk_layer_compute_cubic_evals(cozk_ctx* ctx, const cozk_layer* l, const cozk_spliteq* eq,
                                   uint64_t out_evals[12]);
/* final_claims (dense_interleaved_poly.rs:367-372): out = L.a, L.b, R.a, R.b (b = 0 for PLAIN) */
int cozk_layer_final_claims(cozk_ctx* ctx, const cozk_layer* l, uint64_t out[16]);
/* Layer groups: one sumcheck round of SEVERAL layers that share the public eq polynomial, the challenge and the claim, as one
 * unit of work -- the senders of a Shamir prover (csrc/host/shamir_gp.hpp), each a party with a context of its own on one device.
 * A group refers to k layers, 1 <= k <= COZK_LAYER_GROUP_MAX, of one mode (all PLAIN or all REP3) and one current length >= 2,
 * pairwise distinct, each of a context on the DRIVER's device (the contexts may differ).  It does not own them: freeing the group
 * leaves them valid, and they must outlive it.  create drains every member context's stream once and sizes each member's other
 * ping-pong side, from that member's own pool, to 2 * ceil(len / 4) elements: later rounds allocate nothing.
 *   round  cozk_layer_round for every member at once: with r != NULL every member and the ONE eq `e` (a spliteq of the driver) are
 *          bound with r, then member m's four coefficient shares against that eq and the one public prev_claim go to
 *          out_coeffs + 16 m (k x 16 u64).  Members of <= 2048 elements run as ONE launch of k workgroups behind the eq fold;
 *          larger ones as their k launches back to back, one finishing kernel; either way ONE fetch.  Every launch goes on the
 *          driver's stream and the call returns with that stream drained, so between two group calls a member may be driven by
 *          the per-layer calls of its own context (and `e` by cozk_spliteq_bind) with the same results -- provided that context's
 *          stream is drained before the next group call (cozk_layer_round and cozk_layer_final_claims leave it so).
 *   final  for members 0 .. k_final - 1: the last bind with r (NULL: no bind, a layer that had no rounds) and the final claims,
 *          out_claims + 16 m laid out as cozk_layer_final_claims' (k_final x 16 u64); with r it binds `e` too, as
 *          cozk_layer_prove_rounds does behind its last round.  One launch, one fetch; members from k_final upwards are left
 *          untouched.
 * Refused on the host before any launch, with COZK_ERR_INVALID_ARG and the text left with the driver (*out is NULL): null
 * arguments, k out of range, mixed modes or lengths, a duplicate member, a member on another device, an `e` that is not the
 * driver's, a binding round on members that are down to their two claims or on a fully bound eq, k_final outside 0..k, a final on
 * members that the bind does not leave at two elements. */
#define COZK_LAYER_GROUP_MAX 32 /* = COZK_SHAMIR_MAX_PARTIES */
typedef struct cozk_layer_group cozk_layer_group;
int cozk_layer_group_create(cozk_ctx* driver, cozk_layer* const* layers, int k, cozk_layer_group** out);
int cozk_layer_group_round(cozk_layer_group* g, cozk_spliteq* e, const uint64_t* r, const uint64_t prev_claim[4],
                           uint64_t* out_coeffs /* k x 16 */);
int cozk_layer_group_final(cozk_layer_group* g, cozk_spliteq* e, const uint64_t* r, int k_final,
                           uint64_t* out_claims /* k_final x 16 */);
int cozk_layer_group_free(cozk_layer_group* g);
/* Spartan groups: one round of a co-noir-spartan sumcheck (co-noir-spartan/co-spartan/src/sumcheck.rs:171-395) for SEVERAL members
 * against ONE public polynomial, with one challenge, as one unit of work -- the senders of a Shamir prover
 * (csrc/host/shamir_spartan.hpp).  Every step of that prover is linear in the witness share or multiplies two secret factors, so a
 * party runs the PLAIN round on its shares.  A group has k members, 1 <= k <= COZK_LAYER_GROUP_MAX, of P PLAIN polynomials each
 * ("planes", planes[P m + j] = plane j of member m), all of one current length, a power of two >= 2, pairwise distinct, each of a
 * context on the DRIVER's device (the contexts may differ).
 *   COZK_SPARTAN_GROUP_FIRST   P = 3 (za, zb, zc), public = eq:  g_m(X) = sum_b pub(X) (za_m(X) zb_m(X) - zc_m(X)) at X = 0, 1, 2, 3:
 *                              cozk_spartan_first_round's out[] (LowToHigh pairs 2b, 2b + 1)
 *   COZK_SPARTAN_GROUP_SECOND  P = 1 (z), public = ONE vector lin = alpha A + beta B + gamma C, formed once in front of the rounds
 *                              (cozk_poly_linear_combination):  g_m(X) = sum_b pub(X) z_m(X) at X = 0, 1, 2: cozk_spartan_second_round's
 *                              out_a[].  The three matrix columns are not bound per round: A(rx,ry), B(rx,ry), C(rx,ry) are one public
 *                              evaluation at ry behind the rounds (cozk_poly_batch_evaluate_at_chi) -- the same field elements.
 * The group REFERS to the members' polynomials: it does not own them, freeing it leaves them valid, they must outlive it.  It OWNS the
 * public polynomial: create COPIES pub's current coefficients into ping-pong storage of the group's own (len and len / 2 elements from
 * the driver's pool); `pub` itself is only read, by create, and may be freed right after.  create drains the stream of every context
 * involved once and sizes both ping-pong sides of every plane for all binds to come, from the plane's own pool: later calls
 * allocate nothing.
 *   round  r == NULL (the first round): the sums of the members as they stand.  r != NULL: every plane and the group's public
 *          polynomial are bound with r (cozk_poly_bind(.., COZK_LOW_TO_HIGH)), then the sums are taken.  Member m's evaluations go to
 *          out_evals + 4 E m (E = 4 FIRST, 3 SECOND; k x E x 4 u64).  The bind is fused with the sums: ONE launch of gx x k workgroups
 *          and ONE finishing launch whatever k is, ONE fetch; members of <= 2048 elements run as ONE launch of k workgroups.  The bound
 *          public polynomial is written to the side of the group's ping-pong storage that no workgroup of the launch reads.
 *   final  the last bind with r (len == 2; r == NULL: no bind, everything is down to one element already) of members 0 .. k_final - 1
 *          and of the public polynomial; out = the P final values of member 0, .., of member k_final - 1, then the public polynomial's
 *          ((P k_final + 1) x 4 u64).  One launch, one fetch; members from k_final upwards are left untouched.
 *   len / pub_download  the current length, and the group's public polynomial as it stands (len x 4 u64).
 * Every launch goes on the driver's stream and every call returns with that stream drained; when a call returns every bound plane is
 * in the state cozk_poly_bind(.., COZK_LOW_TO_HIGH) on its own context would have left it in.
 * Refused on the host before any launch, with COZK_ERR_INVALID_ARG and the text left with the driver (*out is NULL), the members and
 * the public polynomial untouched: null arguments, an unknown kind, k out of range, a plane or a pub that is not PLAIN, unequal
 * lengths, a length that is not a power of two or is below 2, a duplicate plane, a member or a pub on another device, a round on
 * fully bound members or a binding round that would leave them so, k_final outside 0..k, a final that does not end at one element. */
#define COZK_SPARTAN_GROUP_FIRST 1
#define COZK_SPARTAN_GROUP_SECOND 2
typedef struct cozk_spartan_group cozk_spartan_group;
int cozk_spartan_group_create(cozk_ctx* driver, int kind, cozk_poly* const* planes /* k x P */, int k, const cozk_poly* pub,
                              cozk_spartan_group** out);
int cozk_spartan_group_round(cozk_spartan_group* g, const uint64_t* r, uint64_t* out_evals /* k x E x 4 */);
int cozk_spartan_group_final(cozk_spartan_group* g, const uint64_t* r, int k_final, uint64_t* out /* (P k_final + 1) x 4 */);
size_t cozk_spartan_group_len(const cozk_spartan_group* g);
int cozk_spartan_group_pub_download(cozk_spartan_group* g, uint64_t* out);
int cozk_spartan_group_free(cozk_spartan_group* g);
/* Outer groups: one round of co-jolt's Spartan OUTER cubic sumcheck (cozk_outer_round below) for SEVERAL members with one
 * challenge, as one unit of work -- the senders of a Shamir prover whose parties each hold a PLAIN cozk_outer over their shares of the
 * witness columns.  Az, Bz, Cz are affine in the columns and t(0), t(infinity) multiply exactly two of them, so a party runs the PLAIN
 * round on its shares.  A group has k members, 1 <= k <= COZK_LAYER_GROUP_MAX: PLAIN cozk_outer states made by cozk_outer_create from
 * the same system and the same tau, all in the same state (round, length, rows per step), pairwise distinct, each of a context on the
 * DRIVER's device (the contexts may differ).  The Gruen split-eq tables are public and identical: the group reads member 0's.  The
 * group REFERS to its members: it does not own them, freeing it leaves them valid, they must outlive it; create drains the stream
 * of every member's context once and allocates nothing on the device (a cozk_outer owns both ping-pong sides from its creation).
 *   round  r == NULL in the first round (and only there): the sums of the members as they stand, t(0) = 0 as in cozk_outer_round.
 *          r != NULL: every member is bound with r, then the sums are taken; with claims + 4 m as member m's share of the running claim
 *          (the hint), member m's four coefficients, low to high, go to out_coeffs + 16 m: what cozk_outer_round(ctx_m, member m, r,
 *          claims + 4 m, ..) writes.  The bind is fused with the sums in every storage regime (compact rows inside a step, the round
 *          whose output rows are whole steps, dense rows): ONE launch of gx x k workgroups and ONE finishing launch whatever k is, ONE
 *          fetch; members of <= 2048 (dense-equivalent) rows run as ONE launch of k workgroups.
 *   final  the last bind with r (length 2) of members 0 .. k_final - 1; out + 12 m = Az(r), Bz(r), Cz(r) of member m, what
 *          cozk_outer_final_evals writes.  One launch, one fetch; members from k_final upwards are left untouched.
 *   len    the members' current (dense-equivalent) length.
 * Every launch goes on the driver's stream and every call returns with that stream drained; when a call returns every member is in the
 * state cozk_outer_round / cozk_outer_final_evals on its own context would have left it in (cozk_outer_download shows it).
 * Refused on the host before any launch, with COZK_ERR_INVALID_ARG and the text left with the driver (*out is NULL), the members
 * untouched: null arguments, k out of range, a member that is not PLAIN, members whose state or tau differ, a duplicate member, a
 * member on another device, r == NULL after the first round or r != NULL in it, a round on fully bound members (or one whose bind
 * leaves them so), k_final outside 0..k, a final on members whose length is not 2.
 * Parity unpinned (the reference has no Shamir prover); restated in tests/ (tests/test_gpu_outer_group.py: twins driven by cozk_outer_round). */
typedef struct cozk_outer cozk_outer;
typedef struct cozk_outer_group cozk_outer_group;
int cozk_outer_group_create(cozk_ctx* driver, cozk_outer* const* members, int k, cozk_outer_group** out);
int cozk_outer_group_round(cozk_outer_group* g, const uint64_t* r /* NULL in round 0 */, const uint64_t* claims /* k x 4 */,
                           uint64_t* out_coeffs /* k x 16 */);
int cozk_outer_group_final(cozk_outer_group* g, const uint64_t r[4], int k_final, uint64_t* out /* k_final x 12 */);
size_t cozk_outer_group_len(const cozk_outer_group* g);
int cozk_outer_group_free(cozk_outer_group* g);
/* Shift groups: one round of a (share, public) product sumcheck of prove_arbitrary_worker's shape -- the Spartan worker's shift
 * sumcheck sum_t z_ry(t) eq_plus_one(rx_step, t) -- for k members of ONE PLAIN polynomial each against ONE public polynomial, binding
 * COZK_HIGH_TO_LOW (pairs i, i + len / 2).  Member m's evaluations at X = 0 and X = 2 go to out_evals + 8 m: what
 * cozk_prod_sumcheck_evals({z_m, pub}, 2, 2, ..) writes.  Members: 1 <= k <= COZK_LAYER_GROUP_MAX, all of one current length, a power of
 * two >= 2, pairwise distinct, each of a context on the DRIVER's device.  Ownership is the Spartan groups': the group REFERS to the
 * members and OWNS a copy of the public polynomial (len and len / 2 elements of ping-pong storage from the driver's pool; `pub` is only
 * read, by create).  create drains the stream of every context involved once and sizes what the binds write (side 0 of a member that is
 * still unbound; a bound member is bound in place, as cozk_poly_bind(.., COZK_HIGH_TO_LOW) binds it): later calls allocate nothing.
 *   round  r == NULL (the first round): the sums of the members as they stand.  r != NULL: every member and the group's public
 *          polynomial are bound with r, then the sums are taken.  The bind is fused with the sums (lane i < len / 4 reads i, i + len / 4,
 *          i + len / 2, i + 3 len / 4 and writes i, i + len / 4; only member row 0 stores the bound public polynomial, into the side
 *          no workgroup reads): ONE launch of gx x k workgroups and ONE finishing launch whatever k is, ONE fetch; members of <= 2048
 *          elements run as ONE launch of k workgroups.
 *   final  the last bind with r (len == 2; r == NULL: no bind, len == 1) of members 0 .. k_final - 1 and of the public polynomial; out =
 *          the k_final member values, then the public value ((k_final + 1) x 4 u64).  One launch, one fetch; members from k_final upwards
 *          are left untouched.
 *   len / pub_download  the current length, and the group's public polynomial as it stands (len x 4 u64).
 * Every launch goes on the driver's stream and every call returns with that stream drained; when a call returns every bound member is
 * in the state cozk_poly_bind(.., COZK_HIGH_TO_LOW) on its own context would have left it in.
 * Refused as for the Spartan groups (COZK_ERR_INVALID_ARG, text with the driver, *out NULL, nothing touched): null arguments, k out of
 * range, a member or a pub that is not PLAIN, unequal lengths, a length that is not a power of two or is below 2, a duplicate member,
 * a member or a pub on another device, a round on fully bound members or a binding round that would leave them so, k_final outside
 * 0..k, a final that does not end at one element.
 * Parity unpinned; restated in tests/ (tests/test_gpu_outer_group.py: twins driven by cozk_prod_sumcheck_evals and cozk_poly_bind). */
typedef struct cozk_shift_group cozk_shift_group;
int cozk_shift_group_create(cozk_ctx* driver, cozk_poly* const* members, int k, const cozk_poly* pub, cozk_shift_group** out);
int cozk_shift_group_round(cozk_shift_group* g, const uint64_t* r, uint64_t* out_evals /* k x 2 x 4 */);
int cozk_shift_group_final(cozk_shift_group* g, const uint64_t* r, int k_final, uint64_t* out /* (k_final + 1) x 4 */);
size_t cozk_shift_group_len(const cozk_shift_group* g);
int cozk_shift_group_pub_download(cozk_shift_group* g, uint64_t* out);
int cozk_shift_group_free(cozk_shift_group* g);
/* local half of layer_output -> mul_vec (dense_interleaved_poly.rs:122-141; local product
 * mpc-types/src/protocols/rep3/arithmetic/ops.rs:71-78): out[j] = L[j] x R[j] + mask_j, where
 * mask_j = PRF(key_self, counter + j) - PRF(key_prev, counter + j) when masked != 0 (key_self is shared with the
 * next party, key_prev with the previous one: the three masks sum to zero; keys may be NULL when masked == 0) */
int cozk_layer_output_local(cozk_ctx* ctx, const cozk_layer* l, int masked, const uint8_t* key_self,
                            const uint8_t* key_prev, uint64_t counter, cozk_vec** out);
/* rep3::arithmetic::mul_vec, local half, on SoA share vectors */
int cozk_rep3_mul_vec_local(cozk_ctx* ctx, int mode, const cozk_vec* xa, const cozk_vec* xb,
                            const cozk_vec* ya, const cozk_vec* yb, int masked, const uint8_t* key_self,
                            const uint8_t* key_prev, uint64_t counter, cozk_vec** out);
/* claimed_outputs (grand_product.rs:266-272): out = (len/2) x 4 u64 additive products */
int cozk_layer_claimed_outputs(cozk_ctx* ctx, const cozk_layer* l, uint64_t* out);

/* ---- toggled / sparse batched grand product (co-jolt/src/subprotocols/sparse_grand_product.rs; Lasso's read / write
 * memory checking of the instruction lookups, jolt/vm/instruction_lookups/worker.rs:763-859).
 * cozk_toggle = Rep3BatchedGrandProductToggleLayer (sparse_grand_product.rs:30-70): public 0/1 flags (one U8 column of N
 * entries per PAIR of circuits -- `flag_indices[batch_index / 2]`, :84) and shared fingerprints (2 * n_pairs circuits x N,
 * circuit-major).  The Rep3SparseInterleavedPolynomial layers above it (co-jolt/src/poly/sparse_interleaved_poly.rs) are
 * kept DENSE on the device -- a missing entry is a stored share of one -- i.e. they are ordinary cozk_layer objects:
 * cozk_toggle_layer_output gives the first of them, cozk_layer_output_local + the ring reshare the rest, and
 * cozk_layer_prove_rounds proves them; every party's round messages equal the reference's sparse computation. */
typedef struct cozk_toggle cozk_toggle;
/* Rep3BatchedGrandProductToggleLayer::new (:57-70); take_ownership != 0 adopts the fingerprint buffers */
int cozk_toggle_create(cozk_ctx* ctx, int mode, const cozk_vec* const* flags, size_t n_pairs, cozk_vec* fp_a,
                       cozk_vec* fp_b, int take_ownership, cozk_toggle** out);
int cozk_toggle_free(cozk_toggle* t);
size_t cozk_toggle_batch(const cozk_toggle* t); /* circuits = 2 * n_pairs */
size_t cozk_toggle_len(const cozk_toggle* t);   /* fingerprints per circuit */
/* layer_output (:76-97): entry b * N + i = flag ? fingerprint : promote_to_trivial_share(party_id, one) */
int cozk_toggle_layer_output(cozk_ctx* ctx, const cozk_toggle* t, int party_id, cozk_layer** out);
/* Rep3Bindable::bind (:153-290), incl. the coalesce step (:104-134) when one entry per circuit is left */
int cozk_toggle_bind(cozk_ctx* ctx, cozk_toggle* t, const uint64_t r[4]);
/* one round of prove_sumcheck over the toggle layer (compute_cubic, :311-823): bind layer + split-eq tables with the
 * previous challenge r (NULL in the first round), then this party's additive g(0), g(2), g(3) of
 * sum_x eq(x) (flag(x) fingerprint(x) + 1 - flag(x)).  The eq polynomial must be ctx's.  Every check comes before the bind: a call
 * refused with COZK_ERR_INVALID_ARG (a fully bound layer or eq polynomial, a bind that would leave no round to run) leaves both
 * as they were */
int cozk_toggle_round(cozk_ctx* ctx, cozk_toggle* t, cozk_spliteq* eq, const uint64_t* r, int party_id,
                      uint64_t out_evals[12]);
/* final_claims (:825-835): the bound flag (public) and the bound fingerprint share */
int cozk_toggle_final_claims(cozk_ctx* ctx, const cozk_toggle* t, uint64_t flag[4], uint64_t fp_a[4], uint64_t fp_b[4]);
/* current (bound) flags and fingerprints -> host; any output pointer may be NULL */
int cozk_toggle_download(cozk_ctx* ctx, const cozk_toggle* t, uint64_t* flags, uint64_t* fp_a, uint64_t* fp_b,
                         size_t* n_flags, size_t* n_fp);
/* Toggle groups: ONE PLAIN toggle layer with k fingerprint planes over ONE copy of the public flags, as one unit of work -- the
 * senders of a Shamir prover (csrc/host/shamir_gp.hpp).  The flags are public, so the layer's output flag ? fingerprint : 1 and
 * its round polynomial eq (flag fingerprint + 1 - flag) are affine in the fingerprints: a party that runs the PLAIN toggle calls
 * on its degree-t share holds a degree-t sharing of the plain prover's values, and everything but the fingerprint loads and the
 * products sum eq flag fingerprint_m is the same for every party.  A group holds one copy of the packed 0/1 flags and of the
 * bound flags and k fingerprint vectors of one shape, 1 <= k <= COZK_LAYER_GROUP_MAX, on the DRIVER's device; the ping-pong
 * storage of the bound planes and flags comes from the driver's pool, both sides at create: later calls allocate nothing.  The
 * rules for member contexts are those of the layer groups above: the vectors may belong to other contexts on the driver's device,
 * create drains each such context's stream once, every launch goes on the driver's stream and every call returns with that stream
 * drained.  take_ownership != 0 adopts the buffers of owned fingerprint vectors (they return to their own contexts' pools with
 * the group); otherwise the group REFERS to them: they are only read and must outlive it.  The flag columns are copied.
 *   layer_outputs  for every member m the dense interleaved layer of cozk_toggle_layer_output (PLAIN, one = 1) as an FR vector
 *                  of owners[m] (a context on the driver's device; storage from its pool), in ONE launch that reads each flag
 *                  byte once for all members.  Needs an unbound group.
 *   round          cozk_toggle_round (PLAIN) for every member at once: with r != NULL the k planes, the one flag array and the
 *                  ONE eq `e` (a spliteq of the driver) are bound with r -- planes and flags in one launch, including the switch
 *                  to the coalesced vectors, padded with ones (flags) and zeros (fingerprints) -- then member m's g(0), g(2),
 *                  g(3) go to out_evals + 12 m (k x 12 u64).  One round-sum launch for all members (a member-chunk grid
 *                  dimension bounds the accumulators per lane; the flag look, the compaction, the eq weights and sum eq flag are
 *                  done once per chunk), one closed-form sum over the eq tables, one finishing launch, ONE fetch.
 *   bind           the bind alone (the last one of a sumcheck); `e` is not touched.
 *   final_claims   of a fully bound group: the bound flag (public) and the bound fingerprints of members 0 .. k_final - 1
 *                  (k_final x 4 u64).  One launch, one fetch.
 * Refused on the host before any launch, with COZK_ERR_INVALID_ARG and the text left with the driver (*out / every out[] NULL):
 * null arguments, k out of range, a fingerprint vector that is not FR, of another length, a duplicate or on another device, flag
 * columns that are not U8 vectors of N entries on the driver's device, N not a power of two >= 2, owners on another device,
 * layer_outputs of a bound group, an `e` that is not the driver's or is fully bound, a round or a bind on a fully bound group, a
 * binding round whose bind leaves no round to run, final claims before the group is fully bound, k_final outside 0..k. */
typedef struct cozk_toggle_group cozk_toggle_group;
int cozk_toggle_group_create(cozk_ctx* driver, const cozk_vec* const* flags, size_t n_pairs, cozk_vec* const* fingerprints, int k,
                             int take_ownership, cozk_toggle_group** out);
int cozk_toggle_group_layer_outputs(cozk_toggle_group* g, cozk_ctx* const* owners, cozk_vec** out /* k */);
int cozk_toggle_group_round(cozk_toggle_group* g, cozk_spliteq* e, const uint64_t* r, uint64_t* out_evals /* k x 12 */);
int cozk_toggle_group_bind(cozk_toggle_group* g, const uint64_t r[4]);
int cozk_toggle_group_final_claims(cozk_toggle_group* g, uint64_t flag[4], uint64_t* fingerprints /* k_final x 4 */, int k_final);
int cozk_toggle_group_free(cozk_toggle_group* g);

/* ---- Sparse pair layers (co-jolt/src/poly/sparse_interleaved_poly.rs:28-737, Rep3SparseInterleavedPolynomial): the layers above
 * the toggle layer kept SPARSE on the device.  A dense interleaved layer of length n is n / 2 pairs (L_j, R_j) at entries 2j,
 * 2j + 1; a cozk_sparse_layer stores the pairs that are not (one, one): a sorted U32 array idx[count] of global pair indices and
 * the values L, R interleaved in that order (one FR array of 2 * count, two -- a, b -- for COZK_MODE_REP3), and the dense length n.
 * A missing pair is this party's trivial share of one in both entries.  n / 2 > 2^32 is refused.  Both structural maps merge
 * neighbours with equal idx >> 1 into one item at idx >> 1 (a head flag, a scan, one lane per merged group):
 *   bind          stored pairs 2k, 2k + 1 -> pair k: L' = lerp(L_2k, L_2k+1, r), R' likewise; a missing sibling is (one, one)
 *   layer_output  pair j -> entry j of the next layer, i.e. half j & 1 of that layer's pair j >> 1
 * The values are, entry by entry, those of the dense formulation restricted to the stored pairs; oracle/pysparse.py (SparseLayer,
 * sparse_layer_output, toggled_construct) is the yardstick.  Per-party SHARES of a Rep3 layer may differ from the dense path's and
 * the reference's: a pair (a, one) is multiplied here where the reference keeps it "ready" (:148-192), and the zero-sharing masks
 * sit at other counters (counter + position in the compact vector).  Only opened values are fixed: transcripts, messages and
 * proofs are byte for byte those of the dense path.
 * The dense formulation pads a ragged tail with zeros (dense_interleaved_poly.rs:155-195), a sparse layer reads a missing pair as
 * ones: bind, round and output are defined while n is a multiple of 4 (a binding round: of 8) -- every length of the toggled tree
 * down to the reference's coalesce point (one pair per circuit), where a prover hands over with cozk_sparse_layer_to_dense.
 * The party of a Rep3 layer is that of the toggle it came from or of the layer it is the output of; a layer from explicit lists
 * learns it from its first round or to_dense call (bind and output_local before that are refused).
 * Refused on the host before any launch, with COZK_ERR_INVALID_ARG and a text (*out NULL, the object usable): null arguments; an
 * idx that is not U32, not strictly increasing or with an index >= n / 2; value vectors of the wrong kind or length; n odd or below
 * 2; a round on an eq that is fully bound or not this context's; a bind that leaves fewer than one pair; a party other than the
 * layer's; a length that is not a multiple of 4 where one is needed. */
typedef struct cozk_sparse_layer cozk_sparse_layer;
/* Rep3SparseInterleavedPolynomial::new (:40-75) from explicit lists; take_ownership != 0 adopts the buffers of owned vectors */
int cozk_sparse_layer_create(cozk_ctx* ctx, int mode, size_t n, cozk_vec* idx, cozk_vec* a, cozk_vec* b, int take_ownership,
                             cozk_sparse_layer** out);
/* Rep3BatchedGrandProductToggleLayer::layer_output (sparse_grand_product.rs:76-97) of an unbound toggle: pair (i, i + 1) of
 * circuit b is stored iff flag[b / 2][i] | flag[b / 2][i + 1]; each entry is flag ? fingerprint : trivial share of one */
int cozk_toggle_sparse_output(cozk_ctx* ctx, const cozk_toggle* t, int party_id, cozk_sparse_layer** out);
int cozk_sparse_layer_free(cozk_sparse_layer* s);
size_t cozk_sparse_layer_len(const cozk_sparse_layer* s);   /* dense length n (:77-89 dense_len) */
size_t cozk_sparse_layer_count(const cozk_sparse_layer* s); /* stored pairs */
size_t cozk_sparse_layer_bytes(const cozk_sparse_layer* s); /* count * (64 * NC + 4), NC = 1 plain, 2 Rep3 */
/* stored pairs after a bind = stored pairs of the output layer: the merged groups G, the same for every party */
int cozk_sparse_layer_next_count(cozk_ctx* ctx, cozk_sparse_layer* s, size_t* out);
/* local half of layer_output (:135-196) as a compact FR vector of 2 * G additive products: L_j x R_j for a stored pair, the
 * additive trivial one (party 0 holds 1, the others 0) for the missing sibling, + PRF(key_self, c) - PRF(key_prev, c) at
 * c = counter + position when masked != 0, as cozk_layer_output_local does.  The caller advances its mask counter by 2 * G. */
int cozk_sparse_layer_output_local(cozk_ctx* ctx, cozk_sparse_layer* s, int masked, const uint8_t* key_self, const uint8_t* key_prev,
                                   uint64_t counter, cozk_vec** out);
/* the products of cozk_sparse_layer_output_local (va) and, for Rep3, what the ring reshare gave for them (vb) as the NEXT layer
 * (:135-196): dense length n / 2, idx = the group indices; take_ownership != 0 adopts the buffers of owned vectors */
int cozk_sparse_layer_from_output(cozk_ctx* ctx, cozk_sparse_layer* s, cozk_vec* va, cozk_vec* vb, int take_ownership,
                                  cozk_sparse_layer** out);
/* Rep3Bindable::bind (:198-380), LowToHigh; ping-pong storage from the context's pool */
int cozk_sparse_layer_bind(cozk_ctx* ctx, cozk_sparse_layer* s, const uint64_t r[4]);
/* one round of prove_sumcheck over the layer (compute_cubic, :415-715), the contract of cozk_toggle_round: bind layer and eq with
 * r when non-NULL, then this party's additive g(0), g(2), g(3) in delta form: the all-ones sums in closed form over the layer's
 * n / 4 quads + sum over the merged groups of eq_t(q) (L_t R_t - 1).  Every check comes before the two binds and before a layer
 * without a party takes party_id: a refused call leaves the layer and eq as they were.  With r, eq needs two unbound variables
 * (the bind takes one, the round the other). */
int cozk_sparse_layer_round(cozk_ctx* ctx, cozk_sparse_layer* s, cozk_spliteq* eq, const uint64_t* r, int party_id,
                            uint64_t out_evals[12]);
/* coalesce (:91-103): the dense interleaved layer (filled with trivial ones, then the stored pairs), an ordinary cozk_layer */
int cozk_sparse_layer_to_dense(cozk_ctx* ctx, const cozk_sparse_layer* s, int party_id, cozk_layer** out);
/* the lists -> host (:28-38 coeffs): idx count x u32, a / b 2 * count x 4 u64; any output pointer may be NULL */
int cozk_sparse_layer_download(cozk_ctx* ctx, const cozk_sparse_layer* s, uint32_t* idx, uint64_t* a, uint64_t* b);
/* per-context counters of the sparse layers (construct / prove_layer, sparse_grand_product.rs:905-1020 as the prover with
 * COZK_TOGGLE_SPARSE=1 drives them): a layer counts as stored sparse when its first round runs -- its bytes then, and the bytes
 * n x 32 x NC of the dense layer it stands for --, a to_dense before any round as a layer scattered at construct, a to_dense after
 * a round as a mid-sumcheck handover */
typedef struct cozk_sparse_stats {
    uint64_t layers_sparse, layers_scattered, sparse_rounds, handovers, bytes_sparse, bytes_dense_equivalent;
} cozk_sparse_stats;
int cozk_sparse_get_stats(const cozk_ctx* ctx, cozk_sparse_stats* out);
int cozk_sparse_reset_stats(cozk_ctx* ctx);

/* ---- Lasso's primary sumcheck of the instruction lookups (co-jolt/src/jolt/vm/instruction_lookups/worker.rs:180-720):
 *   sum_x eq(r, x) ( sum_i flag_i(x) g_i(E_1(x), .., E_alpha(x)) - lookup_output(x) ) = 0.
 * cozk_primary holds eq (public), the instruction flags (public 0/1 U8 columns), the E polynomials and lookup_outputs
 * (shared) and binds them LowToHigh once per round.  The collations g_i (combine_lookups_rep3_batched,
 * co-jolt/src/jolt/instruction/, one .rs each) are given as a table of forms over memory indices:
 *   COZK_G_CONCAT  (and.rs:89-101, utils/instruction_utils.rs:26-47): sum_j 2^(bits (n-1-j)) E_mems[j]        -- local
 *                  ADD SUB AND OR XOR SLL MUL MULU MULHU VIRTUAL_ADVICE VIRTUAL_MOVE; bits = 0: the plain sum of SRA / SRL
 *                  (sra.rs:122-132); the same memory listed twice: MOVSIGN (virtual_movsign.rs:126-139)
 *   COZK_G_PRODUCT (beq.rs:106-130 -> product_many, mpc-core rep3/arithmetic.rs:86-102): prod_j E_mems[j]
 *   COZK_G_LTU     (sltu.rs:139-170): mems = C LTU memories then C - 1 EQ memories: sum_i ltu_i prod_{j<i} eq_j
 *   COZK_G_NOT_PRODUCT (bne.rs:108-140), COZK_G_NOT_LTU (bgeu.rs:113-132), COZK_G_NOT_SLT (bge.rs:121-140): 1 - the form
 *   COZK_G_SLT     (slt.rs:184-302): mems = left_msb, right_msb, C - 1 LTU, C - 2 EQ, lt_abs, eq_abs (2C + 1):
 *                  l (1 - r) + (l r + (1 - l)(1 - r)) (lt_abs + sum_i ltu_i eq_abs prod_{j<i} eq_j)
 *   COZK_G_LTE     (virtual_assert_lte.rs:144-209): mems = C LTU then C EQ: sum_i ltu_i prod_{j<i} eq_j + prod_j eq_j
 *   COZK_G_NOT_FIRST (virtual_assert_halfword_alignment.rs:111-125): 1 - E_mems[0]                               -- local
 *   COZK_G_DIV0    (virtual_assert_valid_div0.rs:36-42, the plain formula): mems = C left_is_zero then C div_by_zero:
 *                  1 - prod left_is_zero + prod div_by_zero   (the Rep3 body at :159-225 computes 1 - (.. + ..): a sign
 *                  slip in the reference that its own plain verifier would reject; not reproduced)
 *   COZK_G_UNSIGNED_REM (virtual_assert_valid_unsigned_remainder.rs:154-249): mems = C LTU, C - 1 EQ, C right_is_zero:
 *                  LTU form + prod right_is_zero
 *   COZK_G_SIGNED_REM (virtual_assert_valid_signed_remainder.rs:40-67; its Rep3 body, :265-273, is todo!() in the reference, the
 *                  multiplication schedule here is ours): mems = left_msb, right_msb, C - 1 EQ, C - 1 LTU, eq_abs, lt_abs,
 *                  C left_is_zero, C right_is_zero (4C + 2)
 *   COZK_G_ZERO    (virtual_pow2.rs:70-78, virtual_right_shift_padding.rs:74-82): 0                                   -- local
 * The multiplicative forms multiply shared values: each level is ONE batched mul_vec / reshare_additive_many over all
 * active (index, instruction, point) items -- cozk_primary_level does the local half and names the device buffers of the
 * ring exchange, which the host runs (cozk_reshare / its own transport) before the next call.  The last multiplication of
 * every form stays additive (into_additive follows it in worker.rs:553): same totals, one ring round less.
 *
 * What cozk_primary_create admits (anything else is COZK_ERR_INVALID_ARG): the chunk count C follows from the form and
 * n_mems, a table's sumcheck degree is the largest g degree + 2 and at most 8, every level is one exchange per round:
 *   form                     n_mems    C      g degree   levels
 *   CONCAT                   1..20     -      1          0          bits * (n_mems - 1) < 200
 *   NOT_FIRST, ZERO          1..20     -      1          0          (only mems[0] is read / nothing is)
 *   PRODUCT, NOT_PRODUCT     C         1..6   C          max(C - 2, 0)
 *   LTU, NOT_LTU             2C - 1    1..6   C          max(C - 2, 0)
 *   LTE                      2C        1..6   C          max(C - 2, 0)
 *   DIV0                     2C        1..6   C          max(C - 2, 0)
 *   UNSIGNED_REM             3C - 1    1..6   C          max(C - 2, 0)
 *   SLT, NOT_SLT             2C + 1    2..4   C + 2      C - 1
 *   SIGNED_REM               4C + 2    2..4   C + 2      C - 1
 * At most 64 instructions, 32 of them multiplicative (neither CONCAT, NOT_FIRST nor ZERO). */
#define COZK_G_CONCAT 0
#define COZK_G_PRODUCT 1
#define COZK_G_LTU 2
#define COZK_G_NOT_PRODUCT 3
#define COZK_G_NOT_LTU 4
#define COZK_G_SLT 5
#define COZK_G_NOT_SLT 6
#define COZK_G_LTE 7
#define COZK_G_NOT_FIRST 8
#define COZK_G_DIV0 9
#define COZK_G_UNSIGNED_REM 10
#define COZK_G_SIGNED_REM 11
#define COZK_G_ZERO 12
#define COZK_PRIMARY_MAX_MEMS 20
typedef struct cozk_primary cozk_primary;
typedef struct cozk_primary_instr {
    int form;                         /* COZK_G_* */
    int n_mems;                       /* 1..COZK_PRIMARY_MAX_MEMS (the chunk count C follows from form and n_mems) */
    int mems[COZK_PRIMARY_MAX_MEMS];  /* indices into the E polynomials, in the order the form lists them */
    int bits;                         /* CONCAT: operand bits per chunk */
} cozk_primary_instr;
/* flags: U8 0/1 columns, or FR vectors (flags that are already bound: the remaining rounds after a worker sub-net split) */
int cozk_primary_create(cozk_ctx* ctx, int mode, int party_id, const cozk_primary_instr* instrs, size_t n_instr,
                        const cozk_vec* const* flags, const cozk_poly* const* E, size_t n_mem,
                        const cozk_poly* lookup_outputs, const cozk_vec* eq, cozk_primary** out);
int cozk_primary_free(cozk_primary* p);
int cozk_primary_degree(const cozk_primary* p); /* sumcheck_poly_degree (worker.rs:701-708): max g degree + 2 */
size_t cozk_primary_len(const cozk_primary* p);
/* what cozk_primary_level of `level` will report as n_elems in the current round; 0 when the level holds nothing, without items, for a
 * level outside 1 .. n_levels or a NULL handle.  Host only. */
size_t cozk_primary_level_elems(const cozk_primary* p, int level);
/* The public exchange plan.  Which (index, instruction) items are live in a round depends on the public flags alone: an instruction is
 * live at index j of round r iff one of the 2^(r + 1) cycles below j carries its flag (a bound flag is non-zero iff one of its pair
 * was, up to a negligible probability) -- an OR pyramid over the per-index live masks cozk_primary_round_begin forms for round 0.  So
 * the n_elems that cozk_primary_level / cozk_primary_group_level report can be computed before any share exists:
 * n_elems_out[COZK_PRIMARY_MAX_LEVELS r + level - 1] for every round r < log_n, zero where a level holds nothing, and *total_out, their
 * sum.  instrs, n_instr and flags (U8 columns of 2^log_n entries on ctx's device) are cozk_primary_create's; no E, lookup_outputs or eq
 * is read and no cozk_primary is made.  The columns are downloaded and the pyramid runs on the host (offline work: n_instr bytes per
 * cycle); item counts become level sizes through round_begin's own formula. */
#define COZK_PRIMARY_MAX_LEVELS 4
int cozk_primary_plan(cozk_ctx* ctx, const cozk_primary_instr* instrs, size_t n_instr, const cozk_vec* const* flags, int log_n,
                      uint64_t* n_elems_out /* log_n x COZK_PRIMARY_MAX_LEVELS */, uint64_t* total_out);
/* one round = primary_sumcheck_prover_message (worker.rs:454-598), in three steps:
 * round_begin: bind with the previous challenge r (NULL in the first round), the pass over the linear instructions, the
 *   item list of the multiplicative ones (*n_items; *n_levels mul_vec levels follow, 0 if there are no items);
 * level (1 .. n_levels): local products + zero-sharing masks PRF(key_self, counter + j) - PRF(key_prev, counter + j) of
 *   n_elems elements (every item's reshared values of this level x degree; 0: nothing to exchange at this level); Rep3: exchange *send -> next party, previous party's -> *recv, then go on;
 * round_finish: out_evals = degree x 4 u64, this party's additive evaluations at X = 0, 2, 3, .., degree. */
int cozk_primary_round_begin(cozk_ctx* ctx, cozk_primary* p, const uint64_t* r, size_t* n_items, int* n_levels);
int cozk_primary_level(cozk_ctx* ctx, cozk_primary* p, int level, const uint8_t* key_self, const uint8_t* key_prev,
                       uint64_t counter, const void** send, void** recv, size_t* n_elems);
int cozk_primary_round_finish(cozk_ctx* ctx, cozk_primary* p, uint64_t* out_evals);
/* after the last round: bind with the last challenge; E_evals = n_mem x (a[4], b[4]), flag_evals = n_instr x 4 (public),
 * out_eval = (a[4], b[4]), eq_eval[4] (may be NULL)  (worker.rs:427-452) */
int cozk_primary_final_evals(cozk_ctx* ctx, cozk_primary* p, const uint64_t r[4], uint64_t* E_evals,
                             uint64_t* flag_evals, uint64_t out_eval[8], uint64_t eq_eval[4]);
/* Level groups: one multiplication level, and the last local step of a round, of the primary sumcheck for the k = 2t + 1 SENDERS of a
 * Shamir prover as one unit of work.  Every slot of a collation program is a sum of products of TWO affine forms, so a party that runs
 * the PLAIN program on degree-t shares of the memories (and of the earlier slots) holds a point of a degree-2t sharing of the slot; where
 * Rep3 reshares over the ring, Shamir reduces the degree: sender m re-deals its value z with cozk_shamir_mul_deal's rule
 *     h[m -> q][pos] = z + sum_{c = 1..t} PRF(keys_m[c - 1], counter + pos) (q + 1)^c,   q = 0 .. 2t,
 * pos = the element's position in the level buffer, and receiver q stores sum_{m <= 2t} lambda_m h[m -> q][pos], lambda =
 * lagrange(1 .. 2t + 1), canonical, at pos of ITS level buffer.  Public constants enter every member's single component (PLAIN): the
 * constant sharing.  Receivers are the 2t + 1 senders only: a party above 2t runs no program and would have no use for a slot value.
 * A group has k = 2t + 1 members, 3 <= k <= COZK_PRIMARY_GROUP_MAX, k odd: PLAIN cozk_primary made from one instruction table, one set
 * of public flags, one eq and one length, pairwise distinct, each of a context on the DRIVER's device, all driven through the same
 * cozk_primary_round_begin calls (round_begin and final_evals stay per member).  keys = k x t x COZK_PRF_KEY_BYTES, member m's t keys at
 * keys + m t 32; create uploads them to a device table.  The group REFERS to its members: it does not own them, freeing it leaves them
 * valid, they must outlive it; create drains the stream of every member's context once.  The staging block [k][k][n_elems] of the level
 * in flight ((2t + 1)^2 x n_elems x 32 bytes) belongs to the group, lives in the driver's pool and grows on demand.
 *   level         level 1 .. n_levels of the current round for all members: TWO launches whatever k is (deal: item blocks x degree x k
 *                 workgroups, each reading ONE member's secrets; combine: element blocks x k, the receiver's step).  *n_elems = the
 *                 elements exchanged per (sender, receiver) pair; 0: nothing is launched and the caller does not advance its counter
 *                 (which instructions are active where is public, as in the Rep3 path).  Otherwise the next exchange's counter is
 *                 counter + n_elems.  When the call returns member q's level buffer holds what per-sender cozk_primary_level, one
 *                 cozk_shamir_mul_deal-rule dealing per sender and one cozk_shamir_combine_vec per receiver would have left there.
 *   round_finish  out = k x degree x 4 u64; row m is byte for byte cozk_primary_round_finish of member m.  One launch with the member on
 *                 a grid axis, one finishing launch over all members' rows, one fetch (no launch when there are no items).
 *   len           the members' current length.
 *   level_buffer  the device address and element count of member `member`'s level buffer (NULL / 0 when the level holds nothing).
 * Streams: round_begin and final_evals stay per member and run on the member's own stream, and cozk_primary_round_begin returns with
 * its last launches (item list, bases) still enqueued there.  So level (when it launches) and round_finish (when there are items) drain,
 * after their host checks and before their first launch, the stream of every distinct member context other than the driver's: nothing
 * a member's stream still writes is read by the group's kernels.  Every launch goes on the driver's stream and every call returns with
 * that stream drained, so a member call that follows sees what the group wrote.  The caller must not run a member's calls on another
 * thread while a group call is in progress.
 * Memory: the staging block of the largest level must fit the device beside the members ((2t + 1)^2 x n_elems x 32 bytes: 961 MB at 2^18
 * cycles, t = 2, uniform mix); a level call that cannot allocate it fails with the allocator's error before any launch and leaves the
 * members untouched.  The per-sender composition holds the same (2t + 1)^2 dealt vectors, so it is no way around that size; a level
 * call that deals and combines a slice of the positions at a time is not built.
 * Refused on the host before any launch,
 * with COZK_ERR_INVALID_ARG and the text left with the driver (*out is NULL), the members untouched: null arguments, k even or out of
 * range, a member that is not PLAIN, a duplicate member, a member on another device, members whose table, degree, n_mem or length
 * differ (create and every call), members whose item counts or level sizes differ (every call), a level outside 1 .. n_levels or a
 * level call without items.
 * The KING level (Damgard-Nielsen on a preprocessed double-random pair, as cozk_shamir_mul_king_pairs_inproc):
 *   create_king   a group WITHOUT PRF keys; member rules, refusals and stream rules are create's.  cozk_primary_group_level on such a
 *                 group is refused on the host.
 *   level_king    on either kind of group.  r_t[q] / r_2t[m], q, m < k: member q's degree-t half and member m's degree-2t half of the
 *                 pair, FR vectors on the driver's device (they may belong to other contexts there; they are read on the driver's
 *                 stream and ordering that read behind their writers is the caller's job).  TWO launches whatever k is:
 *                 k_primary_group_mask (level's grid; staging[m][pos] = z_m[pos] + r_2t[m][r_offset + pos], z never stored) and the
 *                 king's finish (k_shamir_king_finish, the launch of cozk_shamir_king_finish: zed[pos] = sum_m lambda_m
 *                 staging[m][pos], member q's level buffer[pos] = zed[pos] - r_t[q][r_offset + pos], canonical; 2k x 32 B read and
 *                 k x 32 B written per element).  Pair element r_offset + pos serves position pos ONCE: no element of a pair may be
 *                 used twice, so the next exchange's offset is r_offset + n_elems.  r_offset + n_elems <= len for all 2k halves is
 *                 checked on the host before any launch; with n_elems == 0 nothing is launched; the call returns with the driver's
 *                 stream drained.  No PRF runs: everything random was made offline.
 *   staging_bytes the staging block's current size: it grows on demand and after a king level of n_elems it is k x n_elems x 32
 *                 bytes, not k^2 x n_elems x 32 (192 MB instead of 961 MB for the largest level at 2^18 cycles, t = 2, uniform mix).
 * level_king adds to the refusals above: a null half, a half that is not an FR vector of the driver's device, halves too short for
 * r_offset + n_elems.  Every refusal leaves the members untouched.
 * Not built: groups over several GPUs, one public item list shared by the members.
 * Parity unpinned (the reference has no Shamir prover); restated in tests/shamir_primary_ref.py and tests/shamir_primary_king_ref.py. */
#define COZK_PRIMARY_GROUP_MAX 15 /* 2t + 1 with 2t <= COZK_SHAMIR_MAX_DEGREE */
typedef struct cozk_primary_group cozk_primary_group;
int cozk_primary_group_create(cozk_ctx* driver, cozk_primary* const* members, int k, const uint8_t* keys /* k x t x 32 */,
                              cozk_primary_group** out);
int cozk_primary_group_level(cozk_primary_group* g, int level, uint64_t counter, size_t* n_elems);
int cozk_primary_group_round_finish(cozk_primary_group* g, uint64_t* out /* k x degree x 4 */);
size_t cozk_primary_group_len(const cozk_primary_group* g);
int cozk_primary_group_level_buffer(const cozk_primary_group* g, int member, int level, const void** buf, size_t* n_elems);
int cozk_primary_group_free(cozk_primary_group* g);
int cozk_primary_group_create_king(cozk_ctx* driver, cozk_primary* const* members, int k, cozk_primary_group** out);
int cozk_primary_group_level_king(cozk_primary_group* g, int level, const cozk_vec* const* r_t, const cozk_vec* const* r_2t,
                                  size_t r_offset, size_t* n_elems);
size_t cozk_primary_group_staging_bytes(const cozk_primary_group* g);

/* ---- co-jolt's Spartan outer sumcheck over Az / Bz / Cz (co-jolt/src/poly/spartan_interleaved_poly.rs,
 * co-jolt/src/r1cs/spartan/worker.rs:63-120,277-300):  sum_x eq(tau, x) (Az(x) Bz(x) - Cz(x)) = 0.
 * The constraint system is an input (the concrete Jolt constraints live in jolt-core): linear combinations over the
 * witness columns (`flattened_polynomials`, one entry per step each), as jolt-core's r1cs builder holds them:
 *   uniform constraint i (Constraint {a, b, c}):           row i of a step:  Az = a.z, Bz = b.z, Cz = c.z
 *   cross-step constraint j (OffsetEqConstraint {cond, a, b}): Az = a.z - b.z, Bz = cond.z, Cz = 0, where an LC with
 *   offset != 0 reads the NEXT step (its constant term only at the last step; spartan_interleaved_poly.rs:666-684).
 * Az, Bz, Cz live as dense share arrays over rows = step * padded_num_constraints + constraint (a public column enters as
 * its trivial share), built on the device straight from the columns. */
typedef struct cozk_lc {
    int first_term; /* terms [first_term, first_term + n_terms) of the system's term arrays */
    int n_terms;
    int offset;
} cozk_lc;
typedef struct cozk_r1cs {
    const int* term_var;       /* column index, or -1 for the constant */
    const int64_t* term_coeff; /* small integer coefficients (F::from_i64) */
    size_t n_terms;
    const cozk_lc* uniform;    /* 3 per constraint: a, b, c */
    size_t n_uniform;
    const cozk_lc* cross;      /* 3 per constraint: a, b, cond */
    size_t n_cross;
    size_t padded_num_constraints; /* rows per step: a power of two >= n_uniform + n_cross */
} cozk_r1cs;
typedef struct cozk_outer cozk_outer;
/* compute_spartan_Az_Bz_Cz + GruenSplitEqPolynomial::new(tau); vars: REP3 polynomials are shared columns, PLAIN ones
 * public; tau = log2(steps * padded_num_constraints) challenges */
int cozk_outer_create(cozk_ctx* ctx, int mode, int party_id, const cozk_r1cs* sys, const cozk_poly* const* vars,
                      size_t n_vars, const uint64_t* tau, size_t n_tau, cozk_outer** out);
int cozk_outer_free(cozk_outer* st);
size_t cozk_outer_len(const cozk_outer* st);
int cozk_outer_download(cozk_ctx* ctx, const cozk_outer* st, uint64_t* az_a, uint64_t* az_b, uint64_t* bz_a,
                        uint64_t* bz_b, uint64_t* cz_a, uint64_t* cz_b);
/* first_sumcheck_round / subsequent_sumcheck_round (spartan_interleaved_poly.rs:189-612) without the network leg: bind with
 * the previous challenge r (NULL in the first round), then the cubic round polynomial of
 * process_eq_sumcheck_round_worker (subprotocols/sumcheck_spartan.rs:44-79) as 4 additive coefficient shares.
 * Every check comes before the bind: a refused call (COZK_ERR_INVALID_ARG) launches nothing and leaves the handle as it was, so
 * the call the message names can follow on the same handle.  Refused: a NULL ctx, st, claim or out_coeffs ("outer_round: bad
 * argument"); a fully bound handle (cozk_outer_len == 1), with or without r ("outer_round: fully bound"); r with one unbound
 * variable left (cozk_outer_len == 2), where the bind would leave nothing to sum -- that challenge belongs to
 * cozk_outer_final_evals ("outer_round: nothing left to sum after this bind"). */
int cozk_outer_round(cozk_ctx* ctx, cozk_outer* st, const uint64_t* r, const uint64_t claim[4], uint64_t out_coeffs[16]);
/* final_sumcheck_evals (:648-664) after binding with the last challenge: additive Az(r), Bz(r), Cz(r).  Refused before the bind,
 * the handle unchanged, unless exactly one unbound variable is left (cozk_outer_len == 2). */
int cozk_outer_final_evals(cozk_ctx* ctx, cozk_outer* st, const uint64_t r[4], uint64_t out[12]);
/* ---- Spartan inner / shift sumchecks (co-jolt/src/r1cs/spartan/worker.rs:100-275).
 * EqPlusOnePolynomial::evals(r, None).1 (jolt-core, used worker.rs:116): out[y] = eq_plus_one(r, y), big-endian, 2^nv entries;
 * eq_plus_one(x, y) = 1 iff y = x + 1 and x < 2^nv - 1 (no wrap-around).  The eq half of the pair is cozk_eq_evals. */
int cozk_eq_plus_one_evals(cozk_ctx* ctx, const uint64_t* r, int nv, cozk_vec** out);
/* bind_z / bind_shift_z (worker.rs:139-152): dot_product_with_public (dense_mlpoly.rs:228-234) of k polynomials of one length
 * with n_pub = 1 or 2 public vectors in ONE pass over the polynomials.  out[(p * n_pub + q) * 8 ..] = share (a[4], b[4]);
 * b = 0 for a PLAIN polynomial (the dot product of a public polynomial is a public value) */
int cozk_poly_batch_dot_public(cozk_ctx* ctx, const cozk_poly* const* polys, size_t k, const cozk_vec* const* pubs,
                               size_t n_pub, uint64_t* out);

/* ---- co-noir-spartan's public lookup round (co-noir-spartan/co-spartan/src/worker.rs:400-575,694-724,836-846;
 * co-noir-spartan/spartan/src/logup.rs:31-80; co-spartan/src/sumcheck.rs:434-500): plain Fr data, no shares. */
/* hash_tuple (worker.rs:836-846): out[j] = idx[j] + v_msg * eq[idx[j]] for the (pre-filtered) indices, the tail up to n_out
 * (a power of two) repeats entry 0.
 * PRECONDITION (not checked): every idx[j] < eq's length.  The kernel reads eq[idx[j]] as it stands, so a larger index is an
 * out-of-bounds device read (the reference panics there). */
int cozk_hash_tuple(cozk_ctx* ctx, const cozk_vec* idx_u32, const cozk_vec* eq, const uint64_t v_msg[4], size_t n_out,
                    cozk_vec** out);
/* eq_tilde_{rx,ry}(_chunk) of third_round (worker.rs:296-343,376-391): out[j] = src[idx[j]] (0xffffffff = usize::MAX and the
 * padding up to n_out: 0) */
int cozk_vec_gather(cozk_ctx* ctx, const cozk_vec* idx_u32, const cozk_vec* src, size_t n_out, cozk_vec** out);
/* LogLookupProof::prove's field work (logup.rs:45-70): phi = x + values, h = m / phi (m = NULL: 1 / phi) */
int cozk_logup_h(cozk_ctx* ctx, const cozk_vec* values, const cozk_vec* m, const uint64_t x[4], cozk_vec** out_phi,
                 cozk_vec** out_h);
/* boost_degree (spartan/src/utils.rs:11-27): scale by 2^-(new_num_vars - num_vars) and repeat up to 2^new_num_vars */
int cozk_vec_boost_degree(cozk_ctx* ctx, const cozk_vec* v, int new_num_vars, cozk_vec** out);
/* distributed_sumcheck_worker's prover (worker.rs:694-724) = ark-linear-sumcheck IPForMLSumcheck::{prover_init,
 * prove_round} over a ListOfProductsOfPolynomials: product q = coefs[q] * prod of counts[q] polynomials
 * (factor_idx lists them product after product; <= 48 polynomials, <= 32 products, <= 4 factors) */
typedef struct cozk_prodlist cozk_prodlist;
int cozk_prodlist_create(cozk_ctx* ctx, const cozk_vec* const* polys, size_t n_polys, const uint64_t* coefs,
                         const int* counts, const int* factor_idx, size_t n_terms, cozk_prodlist** out);
int cozk_prodlist_free(cozk_prodlist* pl);
int cozk_prodlist_degree(const cozk_prodlist* pl); /* max_multiplicands */
/* prove_round: fix_variables with the previous randomness r (NULL in the first round), then out_evals =
 * (degree + 1) x 4 u64: the evaluations at t = 0 .. degree.
 * Every check comes before the fix: a refused call (COZK_ERR_INVALID_ARG) launches nothing and leaves the list as it was.
 * Refused: a NULL ctx, pl or out_evals ("prodlist_round: bad argument"); a fully fixed list (one element per polynomial), with r
 * ("prodlist_round: fully fixed") or without ("prodlist_round: no variable left"); r with one variable left (two elements per
 * polynomial), where the fix would leave nothing to sum -- that randomness belongs to cozk_prodlist_final ("prodlist_round:
 * nothing left to sum after this fix"). */
int cozk_prodlist_round(cozk_ctx* ctx, cozk_prodlist* pl, const uint64_t* r, uint64_t* out_evals);
/* the last fix_variables + obtain_distrbuted_sumcheck_prover_state (sumcheck.rs:434-452): n_polys x 4 u64.  Refused before the
 * fix, the list unchanged, unless exactly one variable is left. */
int cozk_prodlist_final(cozk_ctx* ctx, cozk_prodlist* pl, const uint64_t r[4], uint64_t* out_vals);

/* SplitEqPolynomial::{new, bind} */
int cozk_spliteq_new(cozk_ctx* ctx, const uint64_t* w, int nv, cozk_spliteq** out);
int cozk_spliteq_free(cozk_spliteq* e);
int cozk_spliteq_lens(const cozk_spliteq* e, size_t* e1_len, size_t* e2_len);
int cozk_spliteq_bind(cozk_ctx* ctx, cozk_spliteq* e, const uint64_t r[4]);
/* current tables -> host (tests): E1_len x 4 u64 and E2_len x 4 u64; either pointer may be NULL */
int cozk_spliteq_download(cozk_ctx* ctx, const cozk_spliteq* e, uint64_t* e1, uint64_t* e2);

/* the layer's current coefficients as a borrowed dense polynomial (for evaluating a layer's MLE) */
int cozk_layer_as_poly(cozk_ctx* ctx, const cozk_layer* l, cozk_poly** out);

/* ---------------------------------------------------------------- network seam ------------- */
/* Host-supplied transports for the worker drivers (libcozk's C++ host layer, csrc/host/prover.hpp).
 * Star = MpcStarNetWorker::{send_response, receive_request} (mpc-net/src/mpc_star.rs:5-66); payloads
 * are ark-serialize uncompressed bytes.  Ring = Rep3Network reshare (send to next, receive from prev;
 * mpc-core/src/protocols/rep3/arithmetic.rs:144-164) on DEVICE buffers, e.g. an RCCL
 * ncclSend/ncclRecv pair.  Callbacks return 0 on success. */
typedef struct cozk_star_net {
    void* user;
    int (*send_response)(void* user, const void* bytes, size_t len);
    int (*receive_request)(void* user, void* buf, size_t cap, size_t* out_len);
} cozk_star_net;
typedef struct cozk_ring_net {
    void* user;
    int (*reshare)(void* user, const void* dev_send, void* dev_recv, size_t nbytes);
    int stream_ordered; /* 0: libcozk synchronises the context's stream before the call and the callback returns when
                           dev_recv is complete; 1: the callback only ENQUEUES the exchange on the context's stream
                           (cozk_ctx_stream) -- no host synchronisation on either side (cozk_ring_net_native) */
} cozk_ring_net;

/* Native ring: the same exchange carried by RCCL inside libcozk -- one ncclSend (to the next party) / ncclRecv (from the
 * previous one) pair per call on the context's stream, GPU to GPU over xGMI, asynchronous to the host.  One party per
 * GPU / process.  Set-up mirrors ncclCommInitRank: ONE participant draws an id (cozk_ring_unique_id), the host
 * distributes those 128 bytes through its own channel (the mpc-net connection it already has), every participant calls
 * cozk_ring_init(ctx, id, rank, nranks) -- rank = PartyID, nranks = 3 for Rep3; the call blocks until all have joined.
 * librccl is loaded on first use.  Replaces Rep3Network::{reshare, send_next, recv_prev} as used by
 * mpc-core/src/protocols/rep3/arithmetic.rs:144-164. */
#define COZK_RING_ID_BYTES 128
int cozk_ring_unique_id(uint8_t out[COZK_RING_ID_BYTES]);
int cozk_ring_init(cozk_ctx* ctx, const uint8_t id[COZK_RING_ID_BYTES], int rank, int nranks);
int cozk_ring_destroy(cozk_ctx* ctx);
int cozk_ring_info(cozk_ctx* ctx, int* rank, int* nranks, uint64_t* bytes_sent);
/* reshare_additive_many (arithmetic.rs:152-164): send `send` to the next party, receive `recv` from the previous one */
int cozk_reshare(cozk_ctx* ctx, const cozk_vec* send, cozk_vec* recv);
/* rep3::arithmetic::mul_vec, whole: out_a = x (x) y + PRF(key_self, counter + j) - PRF(key_prev, counter + j) (local
 * product, mpc-types/src/protocols/rep3/arithmetic/ops.rs:71-78, + zero-sharing mask), then the ring exchange:
 * out_b = the previous party's out_a.  x, y as SoA component vectors; both outputs are new vectors. */
int cozk_rep3_mul_vec(cozk_ctx* ctx, const cozk_vec* xa, const cozk_vec* xb, const cozk_vec* ya, const cozk_vec* yb,
                      const uint8_t* key_self, const uint8_t* key_prev, uint64_t counter, cozk_vec** out_a,
                      cozk_vec** out_b);
/* every rank to every rank on the context's communicator (any number of ranks): ONE ncclGroupStart / ncclGroupEnd on the
 * context's stream with ncclSend(send[r] -> rank r) for every non-NULL send[r] and ncclRecv(recv[r] <- rank r) for every
 * non-NULL recv[r], r = 0..nranks-1; the own rank goes through the same calls (a single-rank ring runs the real path).
 * Entries are FR vectors; that rank r receives exactly what rank s sends it (matching NULL patterns and lengths across
 * ranks) is the caller's contract.  The exchange of cozk_shamir_mul_vec; 32 B per element per xGMI link there. */
int cozk_ring_all_to_all(cozk_ctx* ctx, const cozk_vec* const* send, cozk_vec* const* recv);
/* a cozk_ring_net backed by the context's native ring, for the worker drivers and cozk_harness_prove_distributed */
int cozk_ring_net_native(cozk_ctx* ctx, cozk_ring_net* out);

/* ---------------------------------------------------------------- wire format -------------- */
/* ark-serialize *uncompressed* G1Affine, the encoding of every point the workers send and of the proof structs
 * PST13Commitment{nv, g_product} / Proof{proofs} (mpc-net/src/rep3/quic/worker.rs:187-219; co-jolt/src/poly/commitment/
 * pst13.rs:397-401): x || y as 32-byte LE canonical integers, SWFlags in the top bits of the last byte (bit 6 = infinity,
 * bit 7 = y > -y).  Host-only (no device needed).  decode validates like arkworks' Validate::Yes -- canonical
 * coordinates, consistent flags, on the curve -- and returns COZK_ERR_INVALID_ARG for bytes arkworks would reject. */
int cozk_wire_g1_encode(const uint64_t xy[8], int infinity, uint8_t out[64]);
int cozk_wire_g1_decode(const uint8_t in[64], uint64_t xy[8], int* infinity);

/* ---------------------------------------------------------------- worker drivers ----------- */
/* The C++ round loops (csrc/host/prover.hpp) run against host-supplied nets: the calls a Rust host makes
 * when it wants the whole loop rather than the per-round kernels. */
typedef struct cozk_worker_params {
    int mode;               /* COZK_MODE_PLAIN / COZK_MODE_REP3 */
    int party;              /* PartyID 0..2 */
    uint8_t key_self[COZK_PRF_KEY_BYTES]; /* zero-sharing PRF key shared with the next party */
    uint8_t key_prev[COZK_PRF_KEY_BYTES]; /* ... with the previous party */
    uint64_t mask_counter;                /* starting counter of the zero-sharing stream */
} cozk_worker_params;
/* construct + prove_grand_product_worker (co-jolt/src/subprotocols/grand_product.rs:111-130,239-255) on a
 * clone of `leaves`; ring may be NULL for the plain prover.  out_r = final point (r_cap x 4 u64). */
int cozk_worker_prove_grand_product(cozk_ctx* ctx, const cozk_worker_params* wp, const cozk_star_net* star,
                                    const cozk_ring_net* ring, cozk_layer* leaves, size_t batch_size,
                                    uint64_t* out_r, size_t r_cap, size_t* out_r_len);
/* prove_arbitrary_worker (co-jolt/src/subprotocols/sumcheck.rs:168-246), comb_func = product of the m
 * polynomials; binds them HighToLow in place; out_r = num_rounds x 4, out_final_evals = m x 4 (additive) */
int cozk_worker_prove_arbitrary(cozk_ctx* ctx, const cozk_worker_params* wp, const cozk_star_net* star,
                                cozk_poly* const* polys, size_t m, int combined_degree,
                                const uint64_t claim[4], int num_rounds, uint64_t* out_r,
                                uint64_t* out_final_evals);
/* rep3_first_sumcheck_worker / second (co-noir-spartan/co-spartan/src/worker.rs:593-639, sumcheck.rs:171-395) */
int cozk_worker_spartan_first_sumcheck(cozk_ctx* ctx, const cozk_worker_params* wp, const cozk_star_net* star,
                                       cozk_poly* za, cozk_poly* zb, cozk_poly* zc, cozk_poly* eq,
                                       uint64_t* out_point, uint64_t out_finals[16]);
int cozk_worker_spartan_second_sumcheck(cozk_ctx* ctx, const cozk_worker_params* wp, const cozk_star_net* star,
                                        cozk_poly* z, cozk_poly* a, cozk_poly* b, cozk_poly* c,
                                        const uint64_t coef[12], uint64_t* out_point, uint64_t out_finals[16]);

/* ---------------------------------------------------------------- in-process harness ------- */
/* Counterpart of the reference's runner (co-jolt/examples/rep3_jolt.rs:118-317, run_3_party_jolt.sh):
 * synthesises one trace's witness, runs every party on its own thread / ctx and the
 * coordinator on the caller's thread, and verifies the assembled proof. */
typedef struct cozk_harness cozk_harness;
typedef struct cozk_harness_config {
    int mode;          /* COZK_MODE_PLAIN: one party (plain prover); COZK_MODE_REP3: three parties */
    int log_n;         /* padded trace length N = 2^log_n ("cycles") */
    int n_fr;          /* committed polynomials with uniform Fr scalars (shared in REP3) */
    int n_u16;         /* public u16-valued polynomials */
    int n_u32;         /* public u32-valued polynomials */
    int n_flags;       /* public 0/1 flag polynomials */
    int n_small;       /* shared polynomials of length N/16 (own batch_commit + own opening) */
    int gp_batch;      /* circuits in the dense grand product */
    int gp_log_leaves; /* log2(interleaved leaves per circuit) */
    int precompute;    /* build the 16-window SRS table */
    int devices[3];    /* HIP device per party */
    uint64_t seed;
    int log_workers;   /* worker sub-nets per party: 2^log_workers workers, each holding one high-variable chunk
                          of every polynomial and gp_batch / 2^log_workers circuits (reference: split_poly,
                          dense_mlpoly.rs:275-301; co-jolt/README.md:44).  0 = the single-worker path. */
    int worker_devices[8]; /* HIP device per worker index (in-process form) */
    int leaf_fingerprints; /* 0: the grand-product leaves are seeded random shares (cloned per prove);
                              1: compute_leaves (K11): after the commitments the coordinator sends (gamma, tau) and every
                              circuit's leaves are fingerprints of committed columns -- read leaves gamma u16 + gamma^2 u32 +
                              gamma^3 flag + gamma^k shared - tau over the N cycles, then the write leaves (+ gamma^(k+1)), as
                              the bytecode instance lays them out (jolt/vm/bytecode/worker.rs:57-100).  Needs
                              gp_log_leaves == log_n + 1, n_fr >= 1 and log_workers == 0. */
} cozk_harness_config;
typedef struct cozk_harness_result {
    int verified; /* 1 accepted, 0 rejected, -1 verifier not run */
    double wall_ms;
    /* worker-side phase times, max over parties */
    double t_commit_ms, t_gp_construct_ms, t_gp_prove_ms, t_eval_ms, t_open_ms, t_worker_ms;
    uint64_t bytes_star_up, bytes_star_down, bytes_ring, star_messages;
    uint64_t proof_len;
    uint8_t proof_digest[32]; /* SHA-256 of the serialized proof */
    double t_hub_wait_ms;     /* cozk_harness_prove_distributed: time this participant's coordinator copy spent inside the hub's
                               * all_gather (waiting for the slowest participant of every star exchange); 0 in-process */
    uint64_t hub_exchanges;
} cozk_harness_result;
int cozk_harness_create(const cozk_harness_config* cfg, cozk_harness** out);
const char* cozk_harness_error(const cozk_harness* h);
int cozk_harness_destroy(cozk_harness* h);
int cozk_harness_prove(cozk_harness* h, int verify, cozk_harness_result* res);
int cozk_harness_proof_bytes(const cozk_harness* h, uint8_t* out, size_t cap);

/* Distributed form (BASELINE config 3, "one MI355X per party"): one party per process / GPU.  Every process
 * runs its own copy of the deterministic coordinator; a star gather becomes an all-gather of the parties'
 * messages through the host transport (torch.distributed / RCCL), the ring reshare goes through
 * cozk_ring_net on device pointers.  all_gather: participant i contributes `len` bytes; recv holds
 * n_participants slots of `cap` bytes, lens[i] the received lengths.  Returns 0 on success. */
typedef struct cozk_hub_net {
    void* user;
    int n_participants;
    int my_index;
    int (*all_gather)(void* user, const void* send, size_t len, void* recv, size_t cap, size_t* lens);
} cozk_hub_net;
int cozk_harness_create_party(const cozk_harness_config* cfg, int local_party, cozk_harness** out);
/* one (party, worker) participant of the worker sub-net form (cfg.log_workers > 0): the hub then has
 * nparties * 2^log_workers participants, index = worker * nparties + party; ring may be NULL for MODE_PLAIN */
int cozk_harness_create_participant(const cozk_harness_config* cfg, int local_party, int local_worker,
                                    cozk_harness** out);
int cozk_harness_prove_distributed(cozk_harness* h, const cozk_hub_net* hub, const cozk_ring_net* ring,
                                   int verify, cozk_harness_result* res);
/* Single-node hub: byte all-gather through one POSIX shared-memory segment (lock-free, double-buffered
 * mailboxes; ~1 us per exchange) for one-process-per-GPU runs on ONE node -- the per-round star messages
 * (mpc-net/src/mpc_star.rs:29-66) are a few hundred bytes and latency-bound.  Exactly one participant opens
 * with create = 1 (fails if `name` exists), the others attach with create = 0 afterwards (order the two
 * with the launcher's barrier); cozk_shm_hub_net fills a cozk_hub_net whose callbacks stay valid until
 * close.  Waits are bounded (default 120 s, set_timeout_ms) and any participant can abort all of them. */
typedef struct cozk_shm_hub cozk_shm_hub;
int cozk_shm_hub_open(const char* name, int create, int n_participants, int my_index, size_t slot_bytes,
                      cozk_shm_hub** out);
int cozk_shm_hub_net(cozk_shm_hub* hub, cozk_hub_net* out);
int cozk_shm_hub_unlink(cozk_shm_hub* hub);
int cozk_shm_hub_set_timeout_ms(cozk_shm_hub* hub, uint64_t ms);
void cozk_shm_hub_abort(cozk_shm_hub* hub);
void cozk_shm_hub_close(cozk_shm_hub* hub);
/* synchronous raw copy between any two pointers (device or host) on the context's stream: lets a host
 * transport stage ring payloads in buffers of its own (e.g. torch tensors) */
int cozk_copy(cozk_ctx* ctx, void* dst, const void* src, size_t nbytes);
cozk_ctx* cozk_harness_ctx(cozk_harness* h, int party);

/* ---------------------------------------------------------------- co-noir-spartan harness ---- */
/* BASELINE config 4 restated: a satisfied synthetic R1CS with 2^log_n constraints and
 * variables, 3 entries per row shared by A, B, C; worker side of SpartanProverWorker::prove
 * (co-noir-spartan/co-spartan/src/worker.rs:119-300): zero_round, PST commit of z, first (degree-3) and
 * second (degree-2) sumcheck, z(ry), distributed_open; the calling thread is coordinator + verifier.
 * MODE_REP3 runs three parties (devices[p]); MODE_PLAIN one. */
typedef struct cozk_spartan cozk_spartan;
typedef struct cozk_spartan_config {
    int mode;
    int log_n;
    int precompute; /* window table for the SRS (as cozk_harness_config) */
    int devices[3];
    uint64_t seed;
    int lookup_round; /* 1: also the PUBLIC part of the protocol with one public worker (party 0's GPU):
                       * third_round's tail (worker.rs:296-343: val_a, val_b, val_c, commitments of eq_tilde_rx / ry) and
                       * fourth_round (worker.rs:398-575: two logup lookups, distributed sumcheck, batch opening of 15
                       * polynomials under ck_index); its proof part is appended and verified (spartan/src/logup.rs:117-190) */
    int log_pub_workers; /* 0..3 (needs lookup_round): 2^k public workers, each on chunk j of the index as setup.rs's split_ipk
                          * deals it (rows / cols / val / freq chunks, the SRS slice of ck_index with its generator scaled by
                          * eq(t_high, j)); the coordinator sums val_a, val_b, val_c and the commitments (coordinator.rs:425-475),
                          * sums the sumcheck messages of the first qv - k rounds, proves the last k rounds itself on the
                          * gathered finals (distributed_sumcheck_coordinator, coordinator.rs:748-811), and finishes the batched
                          * opening's last k folds.  The proof bytes equal the one-worker proof. */
} cozk_spartan_config;
typedef struct cozk_spartan_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    double wall_ms;
    double t_zero_round_ms, t_commit_ms, t_sumcheck1_ms, t_matrix_build_ms, t_sumcheck2_ms, t_open_ms, t_worker_ms;
    uint64_t bytes_star_up, bytes_star_down, star_messages;
    uint64_t proof_len;
    uint8_t proof_digest[32]; /* SHA-256 of the serialized proof */
    double t_lookup_ms;       /* cfg.lookup_round: the public worker's third-round tail + fourth round */
    int pub_workers;          /* public workers that proved the lookup round (1 << log_pub_workers) */
    uint64_t pub_star_messages, pub_bytes_up, pub_bytes_down; /* their star (log_pub_workers > 0) */
} cozk_spartan_result;
int cozk_spartan_create(const cozk_spartan_config* cfg, cozk_spartan** out);
const char* cozk_spartan_error(const cozk_spartan* h);
int cozk_spartan_destroy(cozk_spartan* h);
int cozk_spartan_prove(cozk_spartan* h, int verify, cozk_spartan_result* res);
int cozk_spartan_proof_bytes(const cozk_spartan* h, uint8_t* out, size_t cap);

/* ---------------------------------------------------------------- co-noir-spartan by n Shamir parties ---- */
/* The harness above proved by n Shamir parties of degree t, semi-honest, all driven from the calling thread, which owns every party's
 * context and plays the coordinator (csrc/host/shamir_spartan.hpp; restated in tests/shamir_spartan_ref.py; the reference has no Shamir
 * prover).  The instance is cozk_spartan's for (seed, log_n).  Every step of the worker is linear in the witness share or multiplies at
 * most two secret factors, so each party runs the COZK_MODE_PLAIN calls on its degree-t share of z: THE PROOF IS THE PLAIN PROVER'S, BYTE
 * FOR BYTE (cozk_spartan with MODE_PLAIN, oracle/pyspartan.py), accepted by the same verifier.
 *   witness    z is dealt once with cozk_shamir_share_vec's rule at share_counter: coefficient c of element i = PRF(share key c,
 *              share_counter + i), share key c = the harness key (seed ^ 0x53484152, c), c = 0 .. t - 1 (harness keys: the 32 bytes
 *              of four SplitMix64 steps from seed' ^ (0xC0DEC0DE + idx * 0x9E3779B97F4A7C15), as every in-process harness derives them)
 *   zero_round per sender 0..2t, cozk_sparse_matvec3 on its share
 *   commit     parties 0..t commit to their share; the points are combined with lagrange(1..t + 1) (cozk_shamir_combine_points)
 *   masks      M = 4 log_n openings of degree 2t: ONE dealing (cozk_shamir_rand_inproc's rule) of M elements at rand_counter, pair 0
 *              only, zero_p[m] = r2t_p^0[m] - rt_p^0[m].  Party p's (3t + 1) x 32 rand key bytes: key j = the harness key
 *              (seed ^ 0x52414E44, 64 p + j).  As for the grand product A PAIR MUST NEVER BE USED TWICE: (seed, rand_counter ..
 *              rand_counter + M) must not serve another proof -- the caller's contract.
 *   sumcheck 1 sum_x eq(tau, x) (Az Bz - Cz)(x): sender p <= 2t sends g_p(0..3) + zero_p[4 round + e]; opened with lagrange(1..2t + 1).
 *              za, zb, zc(rx) are opened from parties 0..t with lagrange(1..t + 1), unmasked; eq(tau, rx) is public
 *   sumcheck 2 sum_y z(y) (alpha A + beta B + gamma C)(rx, y): the matrices are public, parties 0..t send g_p(0..2), opened with
 *              lagrange(1..t + 1), unmasked, as z's final value is; A, B, C(rx, ry) are public
 *   opening    z(ry) and PST13 open per party 0..t on its share; scalars and quotient commitments combined with lagrange(1..t + 1)
 * When the senders' contexts are on one device each sumcheck runs as ONE cozk_spartan_group on sender 0's context (stats: group_rounds
 * = 2 log_n, group_finals = 2); otherwise, or with COZK_SHAMIR_GP_GROUP=0 in the environment (read on every prove), every sender runs
 * cozk_spartan_first_round / cozk_spartan_second_round and cozk_poly_bind (single_rounds = (2t + 1) log_n + (t + 1) log_n,
 * single_finals = 2 (t + 1)).  Proof, msgs and finals are the same bytes either way.
 * Refused by create before any launch (the handle is returned with its error text): 1 <= t, 2t <= COZK_SHAMIR_MAX_DEGREE,
 * 2t + 1 <= n <= COZK_SHAMIR_MAX_PARTIES, 1 <= log_n <= 24.  Not built: the public lookup round, one party per process, groups over
 * several GPUs, a king variant (no secret-by-secret multiplication is reshared here). */
typedef struct cozk_shamir_spartan cozk_shamir_spartan;
typedef struct cozk_shamir_spartan_config {
    int log_n;
    int precompute; /* window table for the SRS (as cozk_harness_config) */
    int degree, num_parties;
    int devices[COZK_SHAMIR_MAX_PARTIES]; /* one per party */
    uint64_t seed;
    uint64_t share_counter, rand_counter;
} cozk_shamir_spartan_config;
typedef struct cozk_shamir_spartan_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    int grouped;  /* 1: the sumchecks ran as Spartan groups */
    uint64_t proof_len;
    uint8_t proof_digest[32]; /* SHA-256 of the serialized proof */
    uint64_t n_opened;        /* M */
    /* host clock, every party's stream drained at both ends; one thread drives the parties in turn: SUMS over parties */
    double wall_ms, t_zero_round_ms, t_commit_ms, t_masks_ms, t_sumcheck1_ms, t_matrix_build_ms, t_sumcheck2_ms, t_open_ms;
} cozk_shamir_spartan_result;
int cozk_shamir_spartan_create(const cozk_shamir_spartan_config* cfg, cozk_shamir_spartan** out);
const char* cozk_shamir_spartan_error(const cozk_shamir_spartan* h);
int cozk_shamir_spartan_destroy(cozk_shamir_spartan* h);
int cozk_shamir_spartan_prove(cozk_shamir_spartan* h, int verify, cozk_shamir_spartan_result* res);
int cozk_shamir_spartan_proof_bytes(const cozk_shamir_spartan* h, uint8_t* out, size_t cap);
/* the masked first-sumcheck messages [m][p <= 2t], m = 4 round + evaluation index (msgs_len = 4 log_n (2t + 1) elements x 4 u64) */
size_t cozk_shamir_spartan_msgs_len(const cozk_shamir_spartan* h);
int cozk_shamir_spartan_msgs(const cozk_shamir_spartan* h, uint64_t* out, size_t cap);
/* the t + 1 openers' shares [value][p <= t] of: za(rx), zb(rx), zc(rx); round by round the second sumcheck's g(0), g(1), g(2); z's
 * final value; z(ry) (finals_len = (3 log_n + 5)(t + 1) elements) */
size_t cozk_shamir_spartan_finals_len(const cozk_shamir_spartan* h);
int cozk_shamir_spartan_finals(const cozk_shamir_spartan* h, uint64_t* out, size_t cap);
int cozk_shamir_spartan_get_stats(const cozk_shamir_spartan* h, cozk_shamir_gp_stats* stats);

/* ---------------------------------------------------------------- instruction-lookups harness ---- */
/* SURVEY.md 8(f)1 restated synthetically: the toggled / sparse batched grand product of Lasso's read / write memory
 * checking (jolt/vm/instruction_lookups/worker.rs:763-859 + subprotocols/sparse_grand_product.rs): n_pairs memories, each
 * with one public 0/1 flag column over the 2^log_n cycles (density_pct % set) shared by its read and write circuit, and a
 * shared fingerprint vector per circuit.  Workers on the GPU(s), coordinator + plain verifier on the calling thread. */
typedef struct cozk_lookups cozk_lookups;
typedef struct cozk_lookups_config {
    int mode;        /* COZK_MODE_PLAIN / COZK_MODE_REP3 */
    int log_n;       /* cycles N = 2^log_n */
    int n_pairs;     /* memories: 2 * n_pairs circuits */
    int density_pct; /* share of the flags that are set, 0..100 */
    int devices[3];
    uint64_t seed;
    int log_workers; /* worker sub-nets of the primary sumcheck (jolt/vm/instruction_lookups/worker.rs:194-360, coordinator.rs:
                        97-150): 2^log_workers workers per party, each proving the first log_n - log_workers rounds on its
                        high-variable chunk of every polynomial; worker 0 finishes the rest on the gathered finals.  The
                        workers of a party are time-sliced on its context here (one GPU each in a real deployment) */
    int primary; /* 1: run Lasso's primary sumcheck first (n_pairs E polynomials, a five-instruction synthetic table of the
                    three collation forms, lookup_outputs = sum_i flag_i g_i(E)); the proof then starts with its part */
    int mix;     /* instruction mix of the synthetic trace: 0 = uniform over the 27 RV32I instructions (37 % of the cycles run a
                    multiplicative collation); 1 = trace-shaped, the proportions of a sha2-chain guest (ADD / XOR / AND / OR / SLL /
                    SRL dominant, ~6 % multiplicative; csrc/host/lookups_harness.hpp LOOKUPS_SHA2_MIX) */
} cozk_lookups_config;
typedef struct cozk_lookups_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    double wall_ms, t_primary_ms, t_construct_ms, t_prove_ms, t_worker_ms;
    uint64_t bytes_star_up, bytes_star_down, bytes_ring, star_messages;
    uint64_t proof_len;
    uint8_t proof_digest[32];
} cozk_lookups_result;
int cozk_lookups_create(const cozk_lookups_config* cfg, cozk_lookups** out);
const char* cozk_lookups_error(const cozk_lookups* h);
int cozk_lookups_destroy(cozk_lookups* h);
int cozk_lookups_prove(cozk_lookups* h, int verify, cozk_lookups_result* res);
int cozk_lookups_proof_bytes(const cozk_lookups* h, uint8_t* out, size_t cap);
/* the sparse pair layer counters (cozk_sparse_stats) of party `party`'s context, accumulated over the harness's proves, and their
 * reset for every party; all zero unless a prove ran with COZK_TOGGLE_SPARSE=1 */
int cozk_lookups_get_sparse_stats(const cozk_lookups* h, int party, cozk_sparse_stats* out);
int cozk_lookups_reset_sparse_stats(cozk_lookups* h);

/* ---------------------------------------------------------------- Spartan outer-sumcheck harness ---- */
/* SURVEY.md 8(f)2 restated synthetically: Az / Bz / Cz of a satisfied constraint system over 14 witness columns (shared and
 * public; 5 uniform + 2 cross-step constraints, 8 rows per step; csrc/host/outer_harness.hpp) and co-jolt's outer cubic
 * sumcheck with the Gruen split-eq (r1cs/spartan/worker.rs:63-100,277-300); coordinator + plain verifier on the caller. */
typedef struct cozk_outer_harness cozk_outer_harness;
typedef struct cozk_outer_config {
    int mode;
    int log_steps; /* steps (cycles) = 2^log_steps; rows = 8 (toy system) or 128 (Jolt constraint set) per step */
    int devices[3];
    uint64_t seed;
    int system; /* 0: the 7-constraint toy system; 1: the reference's own constraint SET (co-jolt/src/r1cs/constraints.rs:39-257,
                 * 70 uniform + 2 cross-step constraints over the 78 inputs of r1cs/inputs.rs) on a synthetic satisfying trace */
    int full;   /* 1: the whole Rep3UniformSpartanProver::prove (r1cs/spartan/worker.rs:63-273: outer + inner + shift sumchecks,
                 * two batch_evaluate + opening appends); 0: the outer sumcheck alone */
} cozk_outer_config;
typedef struct cozk_outer_result {
    int verified;
    double wall_ms, t_build_ms, t_prove_ms, t_worker_ms;
    double t_outer_ms, t_inner_ms, t_shift_ms, t_openings_ms; /* cfg.full: the parts of t_prove_ms */
    uint64_t bytes_star_up, bytes_star_down, star_messages;
    uint64_t proof_len;
    uint8_t proof_digest[32];
} cozk_outer_result;
int cozk_outer_harness_create(const cozk_outer_config* cfg, cozk_outer_harness** out);
const char* cozk_outer_harness_error(const cozk_outer_harness* h);
int cozk_outer_harness_destroy(cozk_outer_harness* h);
int cozk_outer_harness_prove(cozk_outer_harness* h, int verify, cozk_outer_result* res);
int cozk_outer_harness_proof_bytes(const cozk_outer_harness* h, uint8_t* out, size_t cap);

/* ---------------------------------------------------------------- co-jolt's Spartan worker by n Shamir parties ---- */
/* The whole Spartan worker of the outer harness (cfg.full = 1: outer + inner + shift sumchecks and the two claim exchanges) proved by n
 * Shamir parties of degree t, semi-honest, all driven from the calling thread, which owns every party's context and plays the
 * coordinator (csrc/host/shamir_jolt_spartan.hpp; the reference has no Shamir prover: parity unpinned; restated in tests/
 * (tests/shamir_jolt_spartan_ref.py)).  The instance is the outer harness's own for (seed, log_steps, system).  Every step of the worker
 * is linear in the witness share or multiplies exactly two secret factors, so each party runs the COZK_MODE_PLAIN calls on its shares:
 * THE PROOF IS THE PLAIN PROVER'S, BYTE FOR BYTE (cozk_outer_harness with MODE_PLAIN and full = 1, oracle/pyspartan_outer.py run_full),
 * accepted by the same verifier.
 *   witness    a public column stays public at every party.  Shared column v is dealt once with cozk_shamir_share_vec's rule at
 *              share_counter + v * num_steps; share key c = the harness key (seed ^ 0x53484152, c), c = 0 .. t - 1.
 *   masks      M = 4 (log_steps + log2(rows per step)) openings of degree 2t: ONE dealing (cozk_shamir_rand_inproc's rule) of M elements
 *              at rand_counter, pair 0 only, zero_p[m] = r2t_p^0[m] - rt_p^0[m].  Party p's (3t + 1) x 32 rand key bytes: key j = the
 *              harness key (seed ^ 0x52414E44, 64 p + j).  As for the grand product A PAIR MUST NEVER BE USED TWICE: (seed,
 *              rand_counter .. rand_counter + M) must not serve another proof -- the caller's contract.
 *   outer      senders 0..2t each hold a PLAIN cozk_outer over their columns (a constant or a public column is added to every party's
 *              Az, Bz, Cz: the constant sharing).  Per round sender p's four coefficients + zero_p[4 round + i] are opened with
 *              lagrange(1..2t + 1); the opened claim is every sender's hint of the next round.  In the first round every party's t(0) is 0.
 *              Az, Bz, Cz(r) are opened from parties 0..t with lagrange(1..t + 1), unmasked.
 *   inner      on the host: parties 0..t run the plain round arithmetic on bind_z / bind_shift_z from ONE cozk_poly_batch_dot_public
 *              each, with the opened claim as running claim; each of the three coefficients is opened with lagrange(1..t + 1).
 *   shift      z_ry from cozk_poly_linear_combination per opener; shift_claim is opened from parties 0..t and not appended to the
 *              transcript; the rounds (evaluations at 0 and 2, the opened running claim) are opened from parties 0..t, unmasked.
 *   claims     two exchanges: cozk_poly_batch_evaluate_at_chi per opener at rx_step and at the shift point, every column's value opened
 *              from parties 0..t (a public column's value opens to itself).
 * When the senders' contexts are on one device the outer sumcheck runs as ONE cozk_outer_group on sender 0's context and the shift
 * sumcheck as ONE cozk_shift_group over the openers with one eq_plus_one (stats: group_rounds = n_tau + log_steps with n_tau = log_steps
 * + log2(rows per step), group_finals = 2, or 1 when log_steps = 0: there is no shift round and no shift group then); otherwise, or with
 * COZK_SHAMIR_GP_GROUP=0 in the environment (read on every prove), every sender runs cozk_outer_round / cozk_prod_sumcheck_evals +
 * cozk_poly_bind (single_rounds = (2t + 1) n_tau + (t + 1) log_steps, single_finals = 2 (t + 1), or t + 1 when log_steps = 0).  Proof,
 * msgs and finals are the same bytes either way.
 * Refused by create before any launch (the handle is returned with its error text): 1 <= t, 2t <= COZK_SHAMIR_MAX_DEGREE,
 * 2t + 1 <= n <= COZK_SHAMIR_MAX_PARTIES, 0 <= log_steps <= 24, system 0 or 1.  The Lasso primary sumcheck has a Shamir prover of its
 * own (cozk_shamir_primary below: its multiplicative collations exceed degree 2t, so a degree reduction runs between their levels).
 * Not built: one party per process, groups over several GPUs. */
typedef struct cozk_shamir_jolt_spartan cozk_shamir_jolt_spartan;
typedef struct cozk_shamir_jolt_spartan_config {
    int log_steps;
    int system; /* 0: the toy system, 1: the Jolt constraint set (as cozk_outer_config) */
    int degree, num_parties;
    int devices[COZK_SHAMIR_MAX_PARTIES]; /* one per party */
    uint64_t seed;
    uint64_t share_counter, rand_counter;
} cozk_shamir_jolt_spartan_config;
typedef struct cozk_shamir_jolt_spartan_result {
    int verified; /* 1 ok, 0 rejected, -1 not run: verify_spartan and the opened evaluations against the dealer's columns */
    int grouped;  /* 1: the outer and shift sumchecks ran as groups */
    uint64_t proof_len;
    uint8_t proof_digest[32]; /* SHA-256 of the serialized proof */
    uint64_t n_opened;        /* M */
    /* host clock, every party's stream drained at both ends; one thread drives the parties in turn: SUMS over parties.  t_build: Az, Bz,
     * Cz of every sender */
    double wall_ms, t_build_ms, t_masks_ms, t_outer_ms, t_inner_ms, t_shift_ms, t_openings_ms;
} cozk_shamir_jolt_spartan_result;
int cozk_shamir_jolt_spartan_create(const cozk_shamir_jolt_spartan_config* cfg, cozk_shamir_jolt_spartan** out);
const char* cozk_shamir_jolt_spartan_error(const cozk_shamir_jolt_spartan* h);
int cozk_shamir_jolt_spartan_destroy(cozk_shamir_jolt_spartan* h);
int cozk_shamir_jolt_spartan_prove(cozk_shamir_jolt_spartan* h, int verify, cozk_shamir_jolt_spartan_result* res);
int cozk_shamir_jolt_spartan_proof_bytes(const cozk_shamir_jolt_spartan* h, uint8_t* out, size_t cap);
/* the masked outer messages [m][p <= 2t], m = 4 round + coefficient (msgs_len = 4 n_tau (2t + 1) elements x 4 u64) */
size_t cozk_shamir_jolt_spartan_msgs_len(const cozk_shamir_jolt_spartan* h);
int cozk_shamir_jolt_spartan_msgs(const cozk_shamir_jolt_spartan* h, uint64_t* out, size_t cap);
/* the t + 1 openers' shares [value][p <= t], in proof order: Az, Bz, Cz(r); 3 coefficients per inner round; shift_claim; 3 coefficients
 * per shift round; the nvars witness evaluations; the nvars shift-witness evaluations
 * (finals_len = (3 + 3 log2(4 V) + 1 + 3 log_steps + 2 nvars)(t + 1) elements; nvars = 14 / 78 columns, V = nvars rounded up to a
 * power of two) */
size_t cozk_shamir_jolt_spartan_finals_len(const cozk_shamir_jolt_spartan* h);
int cozk_shamir_jolt_spartan_finals(const cozk_shamir_jolt_spartan* h, uint64_t* out, size_t cap);
int cozk_shamir_jolt_spartan_get_stats(const cozk_shamir_jolt_spartan* h, cozk_shamir_gp_stats* stats);

/* ---------------------------------------------------------------- Lasso's primary sumcheck by n Shamir parties ---- */
/* The primary sumcheck of the instruction lookups (cozk_primary above; the lookups harness's primary phase) proved by n Shamir parties
 * of degree t, semi-honest, all driven from the calling thread, which owns every party's context and plays the coordinator
 * (csrc/host/shamir_primary.hpp; the reference has no Shamir prover: parity unpinned; restated in tests/shamir_primary_ref.py).  The
 * instance is the lookups harness's own for (seed, log_n, n_pairs = n_mem, mix): lookups_instr_table, the instruction of every cycle,
 * the E streams at seed + 9000 (m + 1), lookup_outputs in the clear.  Every slot of a collation program multiplies two affine forms of
 * degree-t values and the 2t + 1 senders reduce the degree between the levels (cozk_primary_group above), so each sender runs the
 * COZK_MODE_PLAIN calls on its shares: THE PROOF IS THE PLAIN PROVER'S, BYTE FOR BYTE (the first proof_len bytes of cozk_lookups with
 * MODE_PLAIN and primary = 1; oracle/pyprimary.prove under a "cozk-lookups" transcript whose first draw is r_eq), accepted by the same
 * verifier.
 *   witness    flags and eq are public.  Column v (E_v for v < n_mem, lookup_outputs = column n_mem) is dealt once with
 *              cozk_shamir_share_vec's rule at share_counter + v 2^log_n; share key c = the harness key (seed ^ 0x53484152, c),
 *              c = 0 .. t - 1.  Only parties 0..2t keep their shares: a party above 2t runs no program in this phase.
 *   rounds     senders 0..2t each hold a PLAIN cozk_primary.  Per round: cozk_primary_round_begin on every sender; every level
 *              1..n_levels through the exchange; round_finish; sender p's D evaluations + zero_p[D round + k] are opened with
 *              lagrange(1..2t + 1); then coordinate_primary_sumcheck's arithmetic (claim - e(0) inserted, compressed, appended, the
 *              challenge drawn).  The transcript has the label "cozk-lookups" and r_eq is drawn first.
 *   exchange   the e-th exchange with n_elems > 0, in the order they happen, uses the counter mul_counter + (the sum of the earlier
 *              exchanges' n_elems); sender p's t mul keys: key c = the harness key (seed ^ 0x4D554C54, 64 p + c).
 *   masks      M = D log_n openings of degree 2t (D = the table's sumcheck degree): ONE dealing (cozk_shamir_rand_inproc's rule) of M
 *              elements at rand_counter, pair 0 only, zero_p[m] = r2t_p^0[m] - rt_p^0[m]; party p's (3t + 1) rand keys: key j = the harness
 *              key (seed ^ 0x52414E44, 64 p + j).  A PAIR MUST NEVER BE USED TWICE: the grand product's contract.
 *   finals     after the last bind E_m(r) and lookup_outputs(r) are degree-t sharings, opened from parties 0..t with lagrange(1..t + 1),
 *              unmasked; flags(r) are public.  The proof's openings are E, flags, outputs, in that order.
 * When the senders' contexts are on one device the levels and the finishes run as ONE cozk_primary_group on sender 0's context; otherwise,
 * or with COZK_SHAMIR_GP_GROUP=0 in the environment (read on every prove), every sender runs cozk_primary_level, deals its level buffer
 * to the senders (cozk_shamir_scatter: the dealing launch and the peer copies of cozk_shamir_mul_inproc), every receiver runs
 * cozk_shamir_combine_vec and copies the result into its level buffer, and every sender runs cozk_primary_round_finish.  Proof, msgs
 * and finals are the same bytes either way.  Stats, with X = the exchanges made (those with n_elems > 0; result.n_exchanges) and
 * L = the sum over the rounds of n_levels (public: 0 in a round without items):
 *   grouped    group_rounds = X + log_n,  single_rounds = 0
 *   per sender group_rounds = 0,          single_rounds = (2t + 1) (L + log_n)
 *   group_finals = single_finals = 0 either way: the final evaluations are read per opener (cozk_primary_final_evals).
 * Refused by create before any launch (the handle is returned with its error text): 1 <= t, 2t <= COZK_SHAMIR_MAX_DEGREE,
 * 2t + 1 <= n <= COZK_SHAMIR_MAX_PARTIES, 1 <= log_n <= 24, 1 <= n_mem <= 128 (what lookups_instr_table admits), mix 0 or 1.
 * The KING construct of the exchange (cozk_shamir_primary_prep + cozk_shamir_primary_prove_king; tests/shamir_primary_king_ref.py):
 * the sizes of all exchanges follow from the public flags (cozk_primary_plan), so everything that needs fresh randomness is made
 * before the witness is touched, as for the grand product (cozk_shamir_gp_prep_inproc):
 *   prep        on a created handle, once.  (A) the M = D log_n opening masks at rand_counter, pair 0: the masks prove deals.  (B) ONE
 *               dealing (cozk_shamir_rand_inproc's rule) of total = the plan's sum elements at rand_counter + M, pair 0 only, of which
 *               the degree-t and the degree-2t halves are extracted for parties 0..2t only: receivers are the senders.
 *               (rand_keys, rand_counter .. rand_counter + M + total) must never be used again: the caller's contract; a second prep of
 *               a handle is refused.  Result: n_openings = M, pair_elems = total, n_exchanges = X, used, t_offline_ms (host clock
 *               around the plan and both dealings, every party's stream drained at both ends).
 *   prove_king  consumes the prep: it is marked used before the first launch, a second king prove and a king prove without a prep are
 *               refused with COZK_ERR_INVALID_ARG and a text, 0 <= king < n.  Exchange e uses the pair at the element offset = the
 *               sum of the earlier exchanges' n_elems: sender m sends z_m + r_2t,m to the king, who opens zed = slot + r and sends it
 *               to everyone; receiver q keeps zed - r_t,q.  Before a level launches anything its size is compared with the plan's and
 *               a difference (a bound flag that happens to be zero) fails the prove with a text naming the round and the level.
 *               Transcript, masks, openings, finals, verifier, tamper_final, every getter and the result are those of prove: THE PROOF
 *               IS THE PLAIN PROVER'S, BYTE FOR BYTE; n_exchanged = pair_elems.  Grouped: one cozk_primary_group_level_king per exchange
 *               on a keyless group (group_rounds = X + log_n).  Otherwise every sender runs cozk_primary_level and adds its r_2t slice
 *               (cozk_vec_binop), the king's context runs cozk_shamir_king_finish at the offset for the senders of its device, each
 *               result is copied into that sender's level buffer, and a sender on another device gets zed by peer copy and subtracts
 *               its r_t slice on its own stream (single_rounds as above).  The same bytes either way.
 * Not built: the other n - t - 1 pairs of the prep's dealing (B) (only pair 0 is extracted), one party per process, groups over several
 * GPUs, one item list shared by the senders, worker sub-nets (log_workers), the primary inside a chained Shamir flow. */
typedef struct cozk_shamir_primary cozk_shamir_primary;
typedef struct cozk_shamir_primary_config {
    int log_n;  /* cycles = 2^log_n */
    int n_mem;  /* E polynomials (the lookups harness's n_pairs) */
    int mix;    /* 0 uniform, 1 sha2-shaped (as cozk_lookups_config) */
    int degree, num_parties;
    int devices[COZK_SHAMIR_MAX_PARTIES]; /* one per party */
    uint64_t seed;
    uint64_t share_counter, mul_counter, rand_counter;
    int tamper_final; /* tests: k > 0 adds 1 to element k - 1 of `finals` (an opener's share) before it is opened; verify must reject */
} cozk_shamir_primary_config;
typedef struct cozk_shamir_primary_result {
    int verified; /* 1 ok, 0 rejected, -1 not run: verify_primary_sumcheck and the opened evaluations against the dealer's columns */
    int grouped;  /* 1: the levels and finishes ran as a group */
    int degree;   /* D */
    uint64_t proof_len;
    uint8_t proof_digest[32]; /* SHA-256 of the serialized proof */
    uint64_t n_opened;        /* M = D log_n */
    uint64_t n_exchanges;     /* X: exchanges with n_elems > 0 */
    uint64_t n_exchanged;     /* the sum of their n_elems: the next free mul counter is mul_counter + n_exchanged */
    /* host clock, every party's stream drained at both ends; one thread drives the parties in turn: SUMS over parties.  t_build: eq and
     * cozk_primary_create of every sender */
    double wall_ms, t_build_ms, t_masks_ms, t_rounds_ms, t_finals_ms;
} cozk_shamir_primary_result;
int cozk_shamir_primary_create(const cozk_shamir_primary_config* cfg, cozk_shamir_primary** out);
const char* cozk_shamir_primary_error(const cozk_shamir_primary* h);
int cozk_shamir_primary_destroy(cozk_shamir_primary* h);
int cozk_shamir_primary_prove(cozk_shamir_primary* h, int verify, cozk_shamir_primary_result* res);
int cozk_shamir_primary_proof_bytes(const cozk_shamir_primary* h, uint8_t* out, size_t cap);
/* the masked round messages [D round + k][p <= 2t] (msgs_len = D log_n (2t + 1) elements x 4 u64) */
size_t cozk_shamir_primary_msgs_len(const cozk_shamir_primary* h);
int cozk_shamir_primary_msgs(const cozk_shamir_primary* h, uint64_t* out, size_t cap);
/* the t + 1 openers' shares [value][p <= t]: E_0(r) .. E_{n_mem - 1}(r), lookup_outputs(r) (finals_len = (n_mem + 1)(t + 1) elements) */
size_t cozk_shamir_primary_finals_len(const cozk_shamir_primary* h);
int cozk_shamir_primary_finals(const cozk_shamir_primary* h, uint64_t* out, size_t cap);
int cozk_shamir_primary_get_stats(const cozk_shamir_primary* h, cozk_shamir_gp_stats* stats);
typedef struct cozk_shamir_primary_prep_result {
    uint64_t n_openings;  /* M */
    uint64_t pair_elems;  /* total: the elements of the exchanges' pair */
    uint64_t n_exchanges; /* X: the plan's exchanges with n_elems > 0 */
    int used;             /* 1 once a king prove has started with it */
    double t_offline_ms;
} cozk_shamir_primary_prep_result;
int cozk_shamir_primary_prep(cozk_shamir_primary* h, cozk_shamir_primary_prep_result* res);
/* all zero before a prep */
int cozk_shamir_primary_prep_get_result(const cozk_shamir_primary* h, cozk_shamir_primary_prep_result* res);
int cozk_shamir_primary_prove_king(cozk_shamir_primary* h, int king, int verify, cozk_shamir_primary_result* res);

/* ---- the dealer's Lasso lookup witness (co-jolt/src/jolt/vm/instruction_lookups/witness.rs:85-150): the coordinator's walk over
 * the trace that makes read_cts / final_cts / E of every memory, before stream_secret_shares (witness.rs:281-310) hands them to the
 * witness scatter (cozk_rep3_scatter).  For memory m with addr = dims[mem_dim[m]], flag = flags[m], subtable = subtables[mem_subtable[m]]:
 *   read_cts[m][j]  = #{ j' < j : flag[j'] = 1 and addr[j'] = addr[j] } if flag[j] = 1, else 0     (TIME order, deterministic)
 *   final_cts[m][a] = #{ j : flag[j] = 1 and addr[j] = a }
 *   E[m][j]         = subtable[addr[j]] if flag[j] = 1, else 0
 * dims: n_dims U32 vectors of n addresses, 1 <= n < 2^32 (any n).  subtables: n_subtables U32 vectors of M entries, 1 <= M <= 65536.
 * flags: n_mem U8 vectors of n entries (non-zero = the step uses the memory); a NULL entry = used at every step.  An unflagged step's
 * address is never used as an index.  A flagged address >= M: COZK_ERR_INVALID_ARG, cozk_last_error names the first such (memory,
 * step), no vector is returned (the kernels skip the address; nothing is read or written out of bounds).
 * Outputs: n_mem NEW vectors each, U32[n], U32[n], U32[M] -- compact columns as the MSM's small-scalar path and
 * cozk_fingerprint_leaves take them.  All memories go through one batched set of launches (tiles of COZK_LASSO_TILE steps x memories);
 * the transient tile histograms are 6 bytes per (tile, memory, address) and the memories are processed in batches that keep them
 * under 256 MiB.  The call returns after the device has finished. */
#define COZK_LASSO_TILE 32768
int cozk_lasso_witness(cozk_ctx* ctx, const cozk_vec* const* dims, size_t n_dims, const cozk_vec* const* subtables, size_t n_subtables,
                       const cozk_vec* const* flags, const int* mem_dim, const int* mem_subtable, size_t n_mem, cozk_vec** read_cts,
                       cozk_vec** E, cozk_vec** final_cts);
size_t cozk_lasso_tile(void); /* COZK_LASSO_TILE of the loaded library */

/* ---- the dealer's read-write memory witness (jolt-core's ReadWriteMemoryPolynomials::generate_witness, the coordinator's walk
 * before read_write_memory/witness.rs:34-93 shares its result): v_read / t_read / v_final / t_final of the register + RAM memory from
 * the trace's addresses and written values.  The n * n_slots operations are ordered by (step j, slot s) -- for Jolt n_slots = 4 in the
 * order rs1, rs2, rd, ram (read_write_memory/worker.rs:243-310): rs1 and rs2 only read, rd writes at every step, ram writes where
 * the store flag is set -- and all slots share ONE memory of MEM = v_init->n words.  From v = v_init, t = 0, per operation with
 * a = addr[s][j]:
 *   v_read[s][j] = v[a];   t_read[s][j] = t[a];
 *   w = (slot s writes at step j) ? v_write[s][j] : v[a];
 *   v[a] = w;   t[a] = j;   (v_written[s][j] = w where that vector exists)           and at the end   v_final = v, t_final = t
 * so t_read[s][j] <= j, the write fingerprint of every operation of step j carries j, and
 *   prod_a h(a, v_init[a], 0) * prod_(j,s) h(a, w, j) == prod_(j,s) h(a, v_read, t_read) * prod_a h(a, v_final[a], t_final[a]).
 * addr: n_slots vectors of n addresses, each U8 or U32.  v_write[s]: U32[n], or NULL = the slot only reads.  is_write[s]: U8[n],
 * non-zero = the step writes, or NULL = every step writes (if v_write[s] is given); it must be NULL where v_write[s] is NULL.
 * v_write / is_write may be NULL as a whole (= every entry NULL).  1 <= n, 1 <= n_slots <= COZK_RW_MEMORY_MAX_SLOTS,
 * n * n_slots < 2^32, 1 <= MEM < 2^32 (Jolt's RAM is 2^20 words and more; no 65536 limit here).
 * Outputs: v_read, t_read: n_slots NEW U32[n] each; v_written: n_slots entries, a NEW U32[n] for a slot with is_write flags, else
 * NULL (there it is v_write[s] or v_read[s]); v_final, t_final: one NEW U32[MEM] each -- compact columns as cozk_fingerprint_leaves
 * and the MSM's small-scalar path take them.  Bit-for-bit deterministic.
 * An address >= MEM: COZK_ERR_INVALID_ARG, cozk_last_error names the smallest (step, slot); nothing is read or written out of
 * bounds.  A wrong kind, a length other than n and is_write without v_write are refused with their own texts.  On any failure every
 * output pointer is NULL (the per-slot ones if n_slots <= COZK_RW_MEMORY_MAX_SLOTS) and the context works on.
 * The walk is a stable sort of the operations by address (16-bit radix passes over tiles of COZK_LASSO_TILE operations; one pass
 * for MEM <= 65536, else two) and a sweep over the sorted operations.  Transient device memory, with N = n * n_slots,
 * tiles = ceil(N / COZK_LASSO_TILE), D = max(min(MEM, 65536), MEM > 65536 ? ceil(MEM / 65536) : 0):
 *   4 N (8 N for two passes) + 2 N + 6 tiles D + 4 D + N / 512 bytes
 * = 72 MiB at n = 2^20 with 4 slots and MEM = 2^16, 88 MiB at MEM = 2^20.  The call returns after the device has finished. */
#define COZK_RW_MEMORY_MAX_SLOTS 8
int cozk_rw_memory_witness(cozk_ctx* ctx, const cozk_vec* const* addr, const cozk_vec* const* v_write, const cozk_vec* const* is_write,
                           size_t n_slots, const cozk_vec* v_init, cozk_vec** v_read, cozk_vec** t_read, cozk_vec** v_written,
                           cozk_vec** v_final, cozk_vec** t_final);

/* ---- Lasso counters over an identity table of any length, and the dealer's timestamp range-check witness made of them (jolt-core's
 * TimestampRangeCheckPolynomials::generate_witness, the coordinator's third walk before sharing: its four families
 * read_cts_read_timestamp / read_cts_global_minus_read / final_cts_read_timestamp / final_cts_global_minus_read are shared as public
 * vectors at co-jolt/src/jolt/vm/jolt/witness.rs:384-409 and timestamp_range_check.rs:31-58, and are the inputs of
 * TimestampValidityProof::prove).  jolt-core is not in the reference tree: the recurrence below is restated from upstream knowledge
 * (parity unpinned).  What pins it is the field names at witness.rs:384-409 and the multiset identity of the memory checking,
 *   prod_a h(a, a, 0) * prod_j h(key_j, key_j, read_cts_j + 1) == prod_j h(key_j, key_j, read_cts_j) * prod_a h(a, a, final_cts[a]).
 * cozk_time_counters: n_cols independent columns (1 <= n_cols <= COZK_TIME_COUNTERS_MAX_COLS) of n U32 keys each over an identity
 * table of M entries, 1 <= n < 2^32, 1 <= M < 2^32 (no 65536 limit: the steps are sorted by key, not counted in LDS).  Per column:
 *   read_cts[c][j]  = #{ j' < j : keys[c][j'] == keys[c][j] }          (TIME order, as in cozk_lasso_witness)
 *   final_cts[c][a] = #{ j : keys[c][j] == a }
 * Outputs: per column a NEW U32[n] and a NEW U32[M] -- compact columns as cozk_fingerprint_leaves and the MSM's small-scalar path
 * take them.  Bit-for-bit deterministic.  A key >= M: COZK_ERR_INVALID_ARG, cozk_last_error names the smallest (column, step);
 * every kernel uses such a key as 0, so nothing is read or written out of bounds.
 * cozk_timestamp_range_witness: t_read[s] is U32[n] for 1 <= n_slots <= COZK_RW_MEMORY_MAX_SLOTS slots, exactly as
 * cozk_rw_memory_witness returns it, and M >= n is the table's length (Jolt: the padded trace length).  The same launches over
 * 2 * n_slots columns whose keys are derived where they are used and never stored:
 *   key = t_read[s][j]       -> read_cts_read_timestamp[s],     final_cts_read_timestamp[s]
 *   key = j - t_read[s][j]   -> read_cts_global_minus_read[s],  final_cts_global_minus_read[s]
 * t_read[s][j] > j: COZK_ERR_INVALID_ARG, cozk_last_error names the smallest (step, slot).
 * Both calls: a wrong kind, columns of unequal length and M < n (second call) are refused with their own texts before any launch;
 * on any failure every output pointer is NULL (if the column / slot count is within its limit) and the context works on.
 * A stable sort of each column's steps by key (16-bit radix passes over tiles of COZK_LASSO_TILE steps; one pass for M <= 65536,
 * else two): with one pass the tile bases + in-tile ranks are read_cts and the digit counts final_cts; with two, a sweep over the
 * sorted steps takes each step's position minus its segment's start, and a segment's length.  Transient device memory for B
 * columns at a time, with tiles = ceil(n / COZK_LASSO_TILE), D = max(min(M, 65536), M > 65536 ? ceil(M / 65536) : 0):
 *   B (6 tiles D + 2 n) bytes, and B (4 D + 12 n) more for two passes
 * where B is the largest column count that keeps 6 tiles D B under 256 MiB (at least one column)
 * = 210 MiB at n = 2^20 with 4 slots (8 columns) and M = 2^20.  Both calls return after the device has finished. */
#define COZK_TIME_COUNTERS_MAX_COLS 16
int cozk_time_counters(cozk_ctx* ctx, const cozk_vec* const* keys, size_t n_cols, size_t M, cozk_vec** read_cts, cozk_vec** final_cts);
int cozk_timestamp_range_witness(cozk_ctx* ctx, const cozk_vec* const* t_read, size_t n_slots, size_t M, cozk_vec** read_cts_read_timestamp,
                                 cozk_vec** read_cts_global_minus_read, cozk_vec** final_cts_read_timestamp,
                                 cozk_vec** final_cts_global_minus_read);

/* ---- The timestamp range-check proof's device calls (TimestampValidityProof::prove, which party 0 alone runs over public data after
 * the output check, co-jolt/src/jolt/vm/read_write_memory/worker.rs:78-105).  Every polynomial of that proof is a public column of
 * 32-bit integers, so its openings and its leaves are made from the compact columns and no Fr copy of a column exists.  jolt-core is
 * not in the reference tree: the circuit order below is this project's (parity unpinned).  cozk_ts_proof_* below is the proof.
 *
 * cozk_compact_batch_evaluate_at_chi: out[c] (4 x u64, Montgomery) = sum_i chi[i] * cols[c][i] for 1 <= k <= COZK_COMPACT_MAX_COLS
 * columns of kind U8 / U16 / U32 / U64 (mixed freely), all of one length 1 <= n < 2^32, n <= chi->n, chi an FR vector.  chi is read
 * once per 8 columns (a workgroup row), not once per column or pair.  Bit for bit what cozk_poly_batch_evaluate_at_chi returns for PLAIN Fr polynomials of the same values.
 * cozk_compact_linear_combination: *out_vec = a NEW FR vector, out[i] = sum_c coeffs[c] * cols[c][i]; coeffs: k x 4 u64 (Montgomery);
 * the same kinds and limits.  Bit for bit cozk_poly_linear_combination (PLAIN) on the same values.
 * Both: a wrong kind, columns of unequal length, k out of range or a chi that is too short is refused with COZK_ERR_INVALID_ARG and
 * a text of its own before any launch, and the context works on.  The sums are exact integers reduced once (a Montgomery-form
 * operand times a plain integer is a Montgomery form); an accumulator holds 2^32 terms, which n < 2^32 keeps out of reach.
 *
 * cozk_timestamp_range_leaves: the leaves of the 6 n_slots + 1 grand-product circuits of the range check in one launch, from the
 * t_read columns and the four counter families of cozk_timestamp_range_witness with M == n (every column U32[n], 1 <= n < 2^32,
 * 1 <= n_slots <= COZK_RW_MEMORY_MAX_SLOTS).  With h(key, count) = count gamma^2 + key (gamma + 1) - tau, the tuple (key, key, count)
 * under a + v gamma + t gamma^2 - tau, circuit c is out[offset + c n + j] (FR, room for (6 n_slots + 1) n entries from offset;
 * cozk_layer_create adopts it):
 *   4 s + 0: h(t_read[s][j], rc_rt[s][j])          4 s + 1: circuit 4 s + 0 plus gamma^2
 *   4 s + 2: h(j - t_read[s][j], rc_gmr[s][j])     4 s + 3: circuit 4 s + 2 plus gamma^2
 *   4 n_slots: init, h(j, 0)
 *   4 n_slots + 1 + 2 s: init plus fc_rt[s][j] gamma^2        4 n_slots + 2 + 2 s: init plus fc_gmr[s][j] gamma^2
 * No iota column and no key column is stored.  gamma, tau: 4 x u64 (Montgomery).  Every leaf is bit for bit what the composition of
 * cozk_fingerprint_leaves calls gives.  t_read[s][j] > j: COZK_ERR_INVALID_ARG, cozk_last_error names the smallest (step, slot);
 * such an entry is used as 0 and nothing is read out of bounds.  Returns after the device has finished. */
#define COZK_COMPACT_MAX_COLS 24
int cozk_compact_batch_evaluate_at_chi(cozk_ctx* ctx, const cozk_vec* const* cols, size_t k, const cozk_vec* chi, uint64_t* out);
int cozk_compact_linear_combination(cozk_ctx* ctx, const cozk_vec* const* cols, const uint64_t* coeffs, size_t k, cozk_vec** out_vec);
int cozk_timestamp_range_leaves(cozk_ctx* ctx, const cozk_vec* const* t_read, const cozk_vec* const* rc_rt, const cozk_vec* const* rc_gmr,
                                const cozk_vec* const* fc_rt, const cozk_vec* const* fc_gmr, size_t n_slots, const uint64_t gamma[4],
                                const uint64_t tau[4], cozk_vec* out, size_t offset);

/* ---- The timestamp range-check proof itself, as an in-process harness (csrc/host/ts_range_proof.hpp; modelled on cozk_lookups and
 * cozk_outer_harness): party 0's public proof that every t_read[s][j] and every j - t_read[s][j] lies in [0, N), a Lasso memory check
 * over an identity table of N entries with ONE batched dense grand product and ONE batched opening.  PLAIN only.  jolt-core is not in
 * the reference tree: the circuit order, the transcript order and the proof bytes are this project's (parity unpinned); what pins them
 * is the plain verifier below and the Python restatement tests/ts_proof_ref.py.  The chained flow does not call this proof (its
 * t_read are seeded streams, which the witness call refuses).
 * create: a Jolt-shaped trace from `seed` (tests/rw_witness_ref.py jolt_instance(seed, N, 2^log_mem, n_regs = 32): rs1, rs2 read, rd
 * writes every step, ram writes where flagged), cozk_rw_memory_witness and cozk_timestamp_range_witness(M = N) on the device; the
 * first n_slots slots' t_read and their 4 n_slots counter columns stay compact U32 vectors, no Fr copy of a column is made; the SRS
 * as the other harnesses build it.
 * prove (worker on the device, coordinator and verifier on the calling thread, transcript "cozk-ts-range"):
 *   1. commit the 5 n_slots columns (cozk_batch_msm_vec, the U32 path): rc_rt[0..], rc_gmr[0..], fc_rt[0..], fc_gmr[0..], t_read[0..];
 *      the commitments go into the transcript      2. gamma, tau      3. the leaves (cozk_timestamp_range_leaves, or with
 *      leaves_fused = 0 the composition of cozk_fingerprint_leaves calls: the same bytes)
 *   4. the claimed outputs (the multiset hashes) into the transcript, then one dense batched grand product over the 6 n_slots + 1
 *      circuits; its point is r = (r_hi, r_lo), r_hi over the circuits padded to a power of two
 *   5. the 5 n_slots claims at r_lo (cozk_eq_evals + cozk_compact_batch_evaluate_at_chi), one claim exchange (rho), the joint
 *      polynomial by cozk_compact_linear_combination over the rho powers, appended as one opening
 *   6. reduce_and_prove over that one opening: one PST13 opening.
 * Proof bytes: commitments (count, then nv and point each), hashes, grand-product proof, claims, reduced opening proof.
 * The verifier replays the transcript and checks, each with a reason of its own in cozk_ts_proof_error:
 *   "multiset equality"  hash[init] * hash[write] == hash[read] * hash[final] for every slot and both kinds
 *   "grand product"      verify_grand_product, and the hashes are its outputs
 *   "leaf claim"         the final claim == the batched evaluation of the 6 n_slots + 1 leaf values rebuilt from the claims, the
 *                        init term being iota(r_lo) (gamma + 1) - tau, missing circuits padded with zero
 *   "opening"            the reduced opening against the rho-combined commitments
 * tamper (tests): 1 adds 1 to fc_rt[0][t_read[0][N / 2]] before the commit -- every other relation holds, only the multiset check
 * can reject; 2 makes the worker send claim 0 plus one -- the leaf check rejects. */
typedef struct cozk_ts_proof cozk_ts_proof;
typedef struct cozk_ts_proof_config {
    int mode;         /* COZK_MODE_PLAIN; anything else is refused */
    int device;
    int log_n;        /* trace length N = 2^log_n, 1..22 */
    int log_mem;      /* memory of 2^log_mem words, 5..24 (32 registers alias its low words) */
    int n_slots;      /* 1..4: the first n_slots of rs1, rs2, rd, ram (Jolt: 4) */
    uint64_t seed;
    int precompute;   /* the SRS window table (cozk_bases_upload) */
    int leaves_fused; /* 1: cozk_timestamp_range_leaves; 0: the composition of cozk_fingerprint_leaves (kept for the A/B) */
    int tamper;       /* 0, 1, 2: see above */
} cozk_ts_proof_config;
typedef struct cozk_ts_proof_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    double wall_ms, t_witness_ms, t_commit_ms, t_leaves_ms, t_gp_ms, t_open_ms;
    uint64_t proof_len;
    uint8_t proof_digest[32];
} cozk_ts_proof_result;
int cozk_ts_proof_create(const cozk_ts_proof_config* cfg, cozk_ts_proof** out);
const char* cozk_ts_proof_error(const cozk_ts_proof* h);
int cozk_ts_proof_destroy(cozk_ts_proof* h);
int cozk_ts_proof_prove(cozk_ts_proof* h, int verify, cozk_ts_proof_result* res);
int cozk_ts_proof_proof_bytes(const cozk_ts_proof* h, uint8_t* out, size_t cap);

/* ---- The read-write memory proof's leaves (the dealer's side of ReadWriteMemoryProof over the consistent witness of
 * cozk_rw_memory_witness).  With h(a, v, t) = a + v gamma + t gamma^2 - tau (the convention of the chained flow's phase 4):
 * cozk_rw_memory_leaves: the 2 n_slots read / write circuits in one launch from the compact columns, circuit-major:
 *   circuit 2 s     : out[offset + (2 s) n + j]     = h(addr[s][j], v_read[s][j], t_read[s][j])
 *   circuit 2 s + 1 : out[offset + (2 s + 1) n + j] = h(addr[s][j], w, j),   w = v_written[s][j], or v_read[s][j] where v_written[s]
 *                                                     is NULL (the slot only reads; v_written may be NULL as a whole)
 * addr[s]: U8 or U32, exactly as cozk_rw_memory_witness takes it (the kinds mixed freely over the slots); v_read[s], t_read[s],
 * v_written[s]: U32; every column of one length 1 <= n < 2^32 (any length), 1 <= n_slots <= COZK_RW_MEMORY_MAX_SLOTS.
 * cozk_rw_memory_init_final_leaves: out[offset + a] = h(a, v_init[a], 0), out[offset + MEM + a] = h(a, v_final[a], t_final[a]);
 * three U32 columns of one length 1 <= MEM < 2^32.
 * Both: out is an FR vector with room for 2 n_slots n (2 MEM) entries from offset, which cozk_layer_create adopts; gamma, tau:
 * 4 x u64 (Montgomery).  No iota column is stored: j and a exist only in registers.  Every leaf is bit for bit what the composition of
 * cozk_fingerprint_leaves calls gives.  A wrong kind, columns of unequal length or an out that is too short is refused with
 * COZK_ERR_INVALID_ARG and a text of its own before any launch, and the context works on.  The launch is asynchronous on the
 * context's stream, as cozk_fingerprint_leaves is.
 * A leaf is made as an exact 9-limb integer sum of 32 x 256-bit products reduced by a short Barrett quotient (a full Montgomery product
 * per term measured 2.5 times as long: DESIGN 4). */
int cozk_rw_memory_leaves(cozk_ctx* ctx, const cozk_vec* const* addr, const cozk_vec* const* v_read, const cozk_vec* const* t_read,
                          const cozk_vec* const* v_written, size_t n_slots, const uint64_t gamma[4], const uint64_t tau[4], cozk_vec* out,
                          size_t offset);
int cozk_rw_memory_init_final_leaves(cozk_ctx* ctx, const cozk_vec* v_init, const cozk_vec* v_final, const cozk_vec* t_final,
                                     const uint64_t gamma[4], const uint64_t tau[4], cozk_vec* out, size_t offset);

/* ---- The same circuits with the values as polynomials, plain or Rep3 shares (Rep3ReadWriteMemoryProver::compute_leaves,
 * co-jolt/src/jolt/vm/read_write_memory/worker.rs:196-344: the addresses and the timestamps are public compact columns, v_read, v_write,
 * v_init and v_final are shares, and every leaf is add_public(mul_public(v_share, gamma), t gamma^2 + a - tau, party_id)).  The layout
 * and h are those of cozk_rw_memory_leaves.
 * cozk_rw_memory_shared_leaves: ONE launch, a thread per (slot, step).  addr[s]: U8 or U32; t_read[s]: U32; one length 1 <= n < 2^32;
 * v_read[s], and v_written[s] where it is not NULL (v_written may be NULL as a whole), are polynomials of at least n entries, PLAIN or
 * REP3; 1 <= n_slots <= COZK_RW_MEMORY_MAX_SLOTS.  A slot that only reads makes one gamma v product per component for both leaves.
 * cozk_rw_memory_shared_init_final_leaves: ONE launch, a thread per address.  t_final: U32 of 1 <= MEM < 2^32 entries; v_init and
 * v_final: polynomials of at least MEM entries, PLAIN or REP3.
 * Both: a REP3 polynomial is accepted only with mode == COZK_MODE_REP3.  With COZK_MODE_REP3, out_a / out_b take the two components
 * of the party's leaf shares: gamma times the components of the value, and the public part a + t gamma^2 - tau through add_public
 * exactly as in cozk_fingerprint_leaves, party 0's a and party 1's b; party 2 computes no public part.  A PLAIN polynomial in a REP3
 * call is a public polynomial and joins the public part (only parties 0 and 1 read it).  With COZK_MODE_PLAIN out_a takes the leaf
 * and out_b is NULL.  out_a (and out_b, another vector) are FR vectors with room for 2 n_slots n (2 MEM) entries from offset, which
 * cozk_layer_create adopts; gamma, tau: 4 x u64 (Montgomery); asynchronous on the context's stream; every refusal comes before any
 * launch with a text of its own and COZK_ERR_INVALID_ARG, and the context works on.  Every leaf is bit for bit what the composition of
 * cozk_fingerprint_leaves calls gives in the same mode for the same party.
 * The public part is the exact 9-limb sum of cozk_rw_memory_leaves with two terms; each share component takes one Montgomery product
 * by gamma and one addition (csrc/rw_memory_leaves.hip). */
int cozk_rw_memory_shared_leaves(cozk_ctx* ctx, const cozk_vec* const* addr, const cozk_poly* const* v_read, const cozk_vec* const* t_read,
                                 const cozk_poly* const* v_written, size_t n_slots, const uint64_t gamma[4], const uint64_t tau[4], int mode,
                                 int party_id, cozk_vec* out_a, cozk_vec* out_b, size_t offset);
int cozk_rw_memory_shared_init_final_leaves(cozk_ctx* ctx, const cozk_poly* v_init, const cozk_poly* v_final, const cozk_vec* t_final,
                                            const uint64_t gamma[4], const uint64_t tau[4], int mode, int party_id, cozk_vec* out_a,
                                            cozk_vec* out_b, size_t offset);

/* ---- The bytecode memory check's device calls (Rep3BytecodeProver, co-jolt/src/jolt/vm/bytecode/worker.rs:43-142): a consistent
 * witness over the six public table columns (preprocessing.v_init_final: address, bitflags, rd, rs1, rs2, imm), and the leaves of its
 * four grand-product circuits from seven compact public columns plus the one shared field column v_imm.
 *
 * cozk_bytecode_witness: a is a U32 vector of 1 <= n < 2^32 entries, the table row each step reads; table[0..5] are the columns of
 * 1 <= B < 2^32 rows: address U32 or U64, bitflags U64, rd / rs1 / rs2 U8, imm I64.  Outputs, all NEW vectors:
 *   v_read[k][j] = table[k][a[j]], k = 0..4, in the table column's own kind (n entries)
 *   v_imm[j]     = F::from_i64(table[5][a[j]]) as an FR vector: the canonical Montgomery word; a negative value v is r - |v|
 *   t_read[j]    = #{ j' < j : a[j'] == a[j] }    U32[n]
 *   t_final[i]   = #{ j : a[j] == i }             U32[B]
 * The counters are the launches of cozk_time_counters (one column, M = B: its transient memory); the gather is one kernel over the six
 * columns.  a[j] >= B: COZK_ERR_INVALID_ARG, cozk_last_error names the smallest such step; nothing is read out of bounds.  A wrong
 * kind or table columns of unequal length are refused with texts of their own before any launch.  On any failure every output
 * pointer is NULL and the context works on.  Bit-for-bit deterministic; returns after the device has finished.
 *
 * With g^k the powers of gamma, the convention of the chained flow's phase 2 and of the reference:
 *   read = a g + v[0] g^2 + v[1] g^3 + v[2] g^4 + v[3] g^5 + v[4] g^6 + t g^7 + imm - tau,   write = read + g^7
 * cozk_bytecode_leaves: ONE launch makes circuit 0 (read) at out[offset + j] and circuit 1 (write) at out[offset + n + j].  a, v[0..4]
 * and t_read are U8 / U16 / U32 / U64 vectors, mixed freely, of one length 1 <= n < 2^32; imm is a polynomial of at least n entries,
 * PLAIN or REP3 (REP3 only with mode == COZK_MODE_REP3).  With COZK_MODE_REP3 the public part enters through add_public exactly as in
 * cozk_fingerprint_leaves: party 0's a, party 1's b, and party 2 carries the imm share alone; out_b is required for REP3 and NULL for
 * PLAIN.
 * cozk_bytecode_init_final_leaves: out[offset + i] = i g + table[0][i] g^2 + .. + table[4][i] g^6 + from_i64(table[5][i]) - tau and
 * out[offset + B + i] the same plus t_final[i] g^7, in ONE launch.  The row number i exists only in registers: no iota column is
 * stored.  table[0..4] and t_final: U8 / U16 / U32 / U64; table[5]: those or I64; one length 1 <= B < 2^32.  In REP3 the leaves are
 * the trivial shares cozk_fingerprint_leaves gives for a columns-only call.
 * Both: out_a (and out_b) are FR vectors with room for 2 n (2 B) entries from offset, which cozk_layer_create adopts; gamma, tau:
 * 4 x u64 (Montgomery); asynchronous on the context's stream; every refusal comes before any launch with a text of its own.  Every
 * leaf is bit for bit what the composition of cozk_fingerprint_leaves calls gives in the same mode for the same party.
 * A leaf's public part is the exact 11-limb integer sum of its 64 x 256-bit products (Montgomery-form coefficients, plain-integer
 * entries), below 2^68 r, reduced once by a 69-bit Barrett quotient (csrc/bytecode_leaves.hip has the bounds). */
int cozk_bytecode_witness(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* const* table, cozk_vec** v_read, cozk_vec** v_imm,
                          cozk_vec** t_read, cozk_vec** t_final);
int cozk_bytecode_leaves(cozk_ctx* ctx, const cozk_vec* a, const cozk_vec* const* v, const cozk_vec* t_read, const cozk_poly* imm,
                         const uint64_t gamma[4], const uint64_t tau[4], int mode, int party_id, cozk_vec* out_a, cozk_vec* out_b,
                         size_t offset);
int cozk_bytecode_init_final_leaves(cozk_ctx* ctx, const cozk_vec* const* table, const cozk_vec* t_final, const uint64_t gamma[4],
                                    const uint64_t tau[4], int mode, int party_id, cozk_vec* out_a, cozk_vec* out_b, size_t offset);

/* ---- The bytecode proof itself, as an in-process harness (csrc/host/bytecode_proof.hpp, on the pattern of cozk_rw_proof and built
 * from memcheck_steps.hpp): party 0's public proof of init * writes == reads * final over the consistent witness of
 * cozk_bytecode_witness.  PLAIN only.  The transcript label is "cozk-bytecode".  jolt-core is not in the reference tree: the transcript
 * order and the proof bytes are this project's (parity unpinned); what pins them is the plain verifier below and tests/bytecode_ref.py.
 * create: the instance of tests/bytecode_ref.py bytecode_instance(seed, N = 2^log_n, B = 2^log_b) restated on the host (row 0 the no-op
 * row; address 0x80000000 + 4 i as U64; a seeded 64-bit bitflags word, the top bit set in every third row; rd, rs1, rs2 below 32; a
 * seeded I64 imm, -2^63 and 2^63 - 1 in rows 1 and 2 where B > 2; the trace starts at row 1 % B, jumps with probability 1/8 to a seeded
 * row in [1, B), else steps on and wraps to 1; the last N / 8 steps are padding at row 0), then cozk_bytecode_witness on the device.
 * The SRS has max(log_n, log_b) variables.
 * prove: (1) PST13::batch_commit of a, v_address, v_bitflags, v_rd, v_rs1, v_rs2, t_read, v_imm (FR), t_final in that order (mixed
 * lengths and kinds; the table is public preprocessing and is not committed), the commitments into the transcript; (2) gamma, tau,
 * the leaves by the two calls above (leaves_fused = 0: the four cozk_fingerprint_leaves launches with an iota column: the same bytes);
 * (3) the two grand products, batch 2 and 2, giving r_rw and r_if; (4) at r_rw eight claims in the commit order -- the seven compact
 * columns by cozk_compact_batch_evaluate_at_chi, v_imm by the Fr evaluation on the same eq table -- ONE claim exchange, the joint
 * polynomial cozk_compact_linear_combination over rho^0..rho^6 plus rho^7 v_imm appended as ONE opening; at r_if t_final opened alone;
 * (5) ONE reduce_and_prove.  Proof bytes: the commitments, the MemCheckProof, the reduced opening.
 * The plain verifier replays the transcript; each check has its own reason (cozk_bytecode_proof_error after a rejected prove):
 * "multiset equality" (hash[init] * hash[write] == hash[read] * hash[final]), "grand product", "leaf claim" (read and write rebuilt
 * from the eight claims; init and final from iota(r_if), the six table MLEs at r_if evaluated on the host, and the t_final claim),
 * "opening".  tamper (tests): 1 adds 1 to v_rd[N / 2] before the commit (only the multiset check can reject); 2 sends claim 0 plus one
 * (the leaf check rejects); 3 adds 1 to t_final[a[N / 2]] (the multiset check rejects). */
typedef struct cozk_bytecode_proof cozk_bytecode_proof;
typedef struct cozk_bytecode_proof_config {
    int mode;         /* COZK_MODE_PLAIN; anything else is refused */
    int device;
    int log_n;        /* trace length N = 2^log_n, 1..22 */
    int log_b;        /* table of 2^log_b rows, 1..22; either of log_n and log_b may be the larger */
    uint64_t seed;
    int precompute;   /* the SRS window table (cozk_bases_upload) */
    int leaves_fused; /* 1: cozk_bytecode_leaves + cozk_bytecode_init_final_leaves; 0: the composition (kept for the A/B) */
    int tamper;       /* 0..3: see above */
} cozk_bytecode_proof_config;
typedef struct cozk_bytecode_proof_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    double wall_ms, t_witness_ms, t_commit_ms, t_leaves_ms, t_gp_ms, t_open_ms; /* t_open_ms: the two openings plus reduce_and_prove */
    uint64_t proof_len;
    uint8_t proof_digest[32];
} cozk_bytecode_proof_result;
int cozk_bytecode_proof_create(const cozk_bytecode_proof_config* cfg, cozk_bytecode_proof** out);
const char* cozk_bytecode_proof_error(const cozk_bytecode_proof* h);
int cozk_bytecode_proof_destroy(cozk_bytecode_proof* h);
int cozk_bytecode_proof_prove(cozk_bytecode_proof* h, int verify, cozk_bytecode_proof_result* res);
int cozk_bytecode_proof_proof_bytes(const cozk_bytecode_proof* h, uint8_t* out, size_t cap);

/* ---- The read-write memory proof itself, as an in-process harness (csrc/host/rw_memory_proof.hpp, on the pattern of cozk_ts_proof):
 * party 0's public proof of init * writes == reads * final over the consistent witness of cozk_rw_memory_witness, with the timestamp
 * range check chained behind it under the same transcript and the same opening accumulator, as Jolt's ReadWriteMemoryProof has it:
 * the t_read commitments are shared and there is ONE reduce_and_prove for everything.  PLAIN only.  jolt-core is not in the reference
 * tree: the circuit order, the transcript order and the proof bytes are this project's (parity unpinned); what pins them is the plain
 * verifier below and the Python restatement tests/rw_proof_ref.py.  The output check over the consistent v_final is not part of this
 * proof: cozk_memory_proof_* below runs it between these steps.  Not built: the public-opening exchange to the other parties, and the
 * chained flow's use of any of this.
 * create: the trace of cozk_ts_proof (tests/rw_witness_ref.py jolt_instance(seed, N, MEM, n_regs = 32)) restricted to the first n_slots
 * of rs1, rs2, rd, ram (with 1 or 2 nothing writes); the register address columns are U8, the RAM column U32; cozk_rw_memory_witness
 * over exactly those slots and, with with_ts, cozk_timestamp_range_witness(M = N).  Every column stays compact: no Fr copy of a column
 * is made.  The SRS has max(log_n, log_mem) variables.
 * prove (worker on the device, coordinator and verifier on the calling thread, transcript "cozk-rw-memory"):
 *   1. commit (PST13::batch_commit: mixed lengths and compact kinds), in this order: addr[0..ns), v_read[0..ns), v_written of the slots
 *      that write (slot order), t_read[0..ns), v_final, t_final, and with with_ts rc_rt, rc_gmr, fc_rt, fc_gmr, each [0..ns); all
 *      commitments go into the transcript.  v_init is public preprocessing and is not committed.
 *   2. gamma, tau; the leaves: 2 ns circuits of N entries, 2 of MEM entries (the two calls above, or with leaves_fused = 0 the
 *      composition of cozk_fingerprint_leaves calls with an iota column: the same bytes)
 *   3. both hash vectors into the transcript, then the dense grand products (batch 2 ns, then batch 2): points r_rw and r_if
 *   4. two openings from the compact columns (cozk_eq_evals, cozk_compact_batch_evaluate_at_chi, one claim exchange each,
 *      cozk_compact_linear_combination over the rho powers, appended as one joint polynomial): at r_rw the N-long columns of step 1,
 *      at r_if v_final and t_final
 *   5. with with_ts the timestamp range check of cozk_ts_proof from its step 2 on (a gamma and tau of its own, the 6 ns + 1 circuits,
 *      one batched grand product, the claims of the 4 ns counter columns and of t_read at its r_lo, a third joint opening); t_read is
 *      not committed again
 *   6. ONE reduce_and_prove over the two or three openings (their points differ in length when log_n != log_mem).
 * Proof bytes: commitments, read-write hashes, init-final hashes, the two grand-product proofs, the claims at r_rw and at r_if, with
 * with_ts the range check's hashes, grand-product proof and claims, then the reduced opening proof.
 * The verifier replays the transcript; each check has a reason of its own in cozk_rw_proof_error:
 *   "multiset equality"  hash[init] * prod_s hash[write_s] == prod_s hash[read_s] * hash[final]
 *   "grand product"      both grand products, and the hashes are their outputs
 *   "leaf claim"         the read / write leaves rebuilt from the claims (the write leaf's time is iota(r_rw)); the init / final leaves
 *                        with iota(r_if) and the MLE of the public v_init at r_if (on the host); missing circuits padded with zero
 *   "timestamp: ..."     the four checks of cozk_ts_proof, prefixed
 *   "opening"            the reduced opening
 * tamper (tests): 1 adds 1 to v_read[last slot][N / 2] before the commit -- a read that no write made: every other relation holds,
 * only the multiset check can reject; 2 sends claim 0 at r_rw plus one -- the leaf check rejects; 3 (with with_ts) is cozk_ts_proof's
 * tamper 1 on fc_rt[0] -- "timestamp: multiset equality". */
typedef struct cozk_rw_proof cozk_rw_proof;
typedef struct cozk_rw_proof_config {
    int mode;         /* COZK_MODE_PLAIN; anything else is refused */
    int device;
    int log_n;        /* trace length N = 2^log_n, 1..22 */
    int log_mem;      /* memory of 2^log_mem words, 5..24; either of log_n and log_mem may be the larger */
    int n_slots;      /* 1..4: the first n_slots of rs1, rs2, rd, ram; with 1 or 2 nothing writes */
    uint64_t seed;
    int precompute;   /* the SRS window table (cozk_bases_upload) */
    int with_ts;      /* 0 or 1: chain the timestamp range check */
    int leaves_fused; /* 1: cozk_rw_memory_leaves + cozk_rw_memory_init_final_leaves (and cozk_timestamp_range_leaves); 0: the
                       * composition of cozk_fingerprint_leaves (kept for the A/B); both give the same bytes */
    int tamper;       /* 0..3: see above */
} cozk_rw_proof_config;
typedef struct cozk_rw_proof_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    /* t_leaves_ms, t_gp_ms: the memory check's; t_ts_ms: the whole chained range check (its leaves, grand product and claims);
     * t_open_ms: the two compact openings at r_rw and r_if plus reduce_and_prove */
    double wall_ms, t_witness_ms, t_commit_ms, t_leaves_ms, t_gp_ms, t_ts_ms, t_open_ms;
    uint64_t proof_len;
    uint8_t proof_digest[32];
} cozk_rw_proof_result;
int cozk_rw_proof_create(const cozk_rw_proof_config* cfg, cozk_rw_proof** out);
const char* cozk_rw_proof_error(const cozk_rw_proof* h);
int cozk_rw_proof_destroy(cozk_rw_proof* h);
int cozk_rw_proof_prove(cozk_rw_proof* h, int verify, cozk_rw_proof_result* res);
int cozk_rw_proof_proof_bytes(const cozk_rw_proof* h, uint8_t* out, size_t cap);

/* ---- The same memory check proved by three Rep3 parties, as an in-process harness (csrc/host/rw_memory_proof_rep3.hpp;
 * Rep3ReadWriteMemoryProver, co-jolt/src/jolt/vm/read_write_memory/worker.rs:196-344): the addresses and the timestamps are public
 * compact columns, v_read, v_written and v_final are Rep3 shares, v_init is public preprocessing.  The instance, the column order, the
 * transcript ("cozk-rw-memory"), the proof bytes and the verifier are cozk_rw_proof's with with_ts = 0: the proof is byte for byte the
 * plain proof of the same seed, and the verifier (the same code) runs the multiset check and reports the same reasons.
 * create (all of it outside prove's clock): cozk_rw_proof's instance on party 0's context (devices[0]); every party gets the public
 * columns addr, t_read, t_final and v_init, the last as a PLAIN polynomial; each secret column -- v_read[s], the v_written of the slots
 * that write, v_final -- is widened to Fr (cozk_compact_linear_combination with coefficient 1) and shared under the harness keys, a
 * seed per column; every party holds an SRS of its own.
 * prove (three workers on threads of their own with a ring between them, coordinator and verifier on the calling thread):
 *   1. commit in the plain order addr, v_read, v_written, t_read, v_final, t_final: each party the a components of its shares and the
 *      public columns; the coordinator adds the share commitments and keeps party 0's public ones
 *   2. gamma, tau; the leaves in REP3: cozk_rw_memory_shared_leaves + cozk_rw_memory_shared_init_final_leaves (leaves_fused = 1), or
 *      the composition of ten (at 4 slots) cozk_fingerprint_leaves calls with an iota column (leaves_fused = 0): the same bytes
 *   3. both hash vectors, then the two dense grand products in REP3: points r_rw and r_if
 *   4. the openings at r_rw and at r_if, each ONE claim exchange and ONE joint polynomial: the claims of public columns from
 *      cozk_compact_batch_evaluate_at_chi, reported by party 0 (the convention of the chained flow's openings), those of shared columns
 *      additive from cozk_poly_batch_evaluate_at_chi; the joint polynomial is the compact combination of the public columns over their
 *      rho powers, as a PLAIN polynomial, plus the shared polynomials over theirs (cozk_poly_linear_combination)
 *   5. ONE reduce_and_prove.
 * tamper: 1 adds 1 to v_read[last slot][N / 2] before the sharing ("multiset equality"); 2: party 0 adds one to its share of claim 0 at
 * r_rw ("leaf claim").
 * Refused by create before any context exists: log_n outside 1..22, log_mem outside 5..24, n_slots outside 1..4, leaves_fused outside
 * 0..1, tamper outside 0..2.
 * The output check by the same parties behind these steps: cozk_memory_proof_rep3_* below.
 * Not built: the timestamp range check by Rep3 parties, one party per process. */
typedef struct cozk_rw_proof_rep3 cozk_rw_proof_rep3;
typedef struct cozk_rw_proof_rep3_config {
    int devices[3];   /* one device per party */
    int log_n;        /* 1..22 */
    int log_mem;      /* 5..24 */
    int n_slots;      /* 1..4, as cozk_rw_proof_config */
    uint64_t seed;    /* the instance seed: the same seed gives cozk_rw_proof's instance */
    int precompute;   /* as cozk_rw_proof_config */
    int leaves_fused; /* 1: the two shared calls; 0: the composition (kept for the A/B); both give the same bytes */
    int tamper;       /* 0..2: see above */
} cozk_rw_proof_rep3_config;
typedef struct cozk_rw_proof_rep3_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    /* t_witness_ms: the dealer's witness walks (create); t_share_ms: uploading, widening and sharing the columns (create), and the
     * phases of prove, each the maximum over the parties; t_open_ms: the two openings plus reduce_and_prove */
    double wall_ms, t_witness_ms, t_share_ms, t_commit_ms, t_leaves_ms, t_gp_ms, t_open_ms;
    uint64_t ring_bytes; /* sent over the ring by the three parties together */
    uint64_t proof_len;
    uint8_t proof_digest[32];
} cozk_rw_proof_rep3_result;
int cozk_rw_proof_rep3_create(const cozk_rw_proof_rep3_config* cfg, cozk_rw_proof_rep3** out);
const char* cozk_rw_proof_rep3_error(const cozk_rw_proof_rep3* h);
int cozk_rw_proof_rep3_destroy(cozk_rw_proof_rep3* h);
int cozk_rw_proof_rep3_prove(cozk_rw_proof_rep3* h, int verify, cozk_rw_proof_rep3_result* res);
int cozk_rw_proof_rep3_proof_bytes(const cozk_rw_proof_rep3* h, uint8_t* out, size_t cap);

/* ---- The output check of the read-write memory proof on the device (prove_outputs, co-jolt/src/jolt/vm/read_write_memory/worker.rs:
 * 110-175; csrc/output_check.inc):
 *     sum_x eq(r_eq, x) * io_range(x) * (v_final(x) - v_io(x)) = 0,   degree 3, binding HighToLow,
 * from the compact columns.  v_final: U32, MEM = 2^m entries, 1 <= m < 32; v_io: U32, io_len >= 1 entries, the public io words of the
 * window [io_start, io_start + io_len) ONLY; r_eq: m x 4 u64 (Montgomery).  With W' the power of two at or above io_len, the rounds
 * whose half length is at least W' need four windowed dot products each and host scalars (eq is never a table of MEM entries, the
 * range never a vector), only d = v_final - v_io is folded whole, and the last log2 W' rounds are the dense product sumcheck on
 * W'-entry vectors; W' = MEM: d is materialised once and every round is dense.
 * cozk_output_check_round: with r != NULL it first binds the previous variable with r; out = the round polynomial at X = 0, 2, 3,
 *   exactly what cozk_prod_sumcheck_evals({eq, io_range, v_final - v_io}, 3, 3, ..) writes for the dense Fr vectors in the same state.
 * cozk_output_check_final: the last bind; out = eq(r), io_range(r), (v_final - v_io)(r), what cozk_poly_get_coeff(.., 0, ..) of the
 *   three bound polynomials gives.  m = 1: round(NULL), then final(r).
 * cozk_output_check_len: the current length 2^(variables left).
 * Each call returns with the stream drained and the values on the host.  v_final and v_io are only read and must outlive the handle.
 * Device memory, all taken in create from the context's pool: W' < MEM: MEM / 2 Fr entries for the folds plus two W'-entry Fr vectors;
 * W' = MEM: three MEM-entry Fr vectors.  No Fr vector of MEM entries exists unless W' = MEM.
 * Refused with COZK_ERR_INVALID_ARG and a text of its own before any launch, *out NULL, the context working on: a null argument; a
 * v_final that is not U32 or whose length is not a power of two of at least 2 (and below 2^32); a v_io that is not U32; io_len == 0;
 * io_start + io_len > MEM; a vector on another device; a round with r == NULL after round 0 or with r != NULL in round 0; a round
 * when one variable is left; a final when more than one is left. */
typedef struct cozk_output_check cozk_output_check;
int cozk_output_check_create(cozk_ctx* ctx, const cozk_vec* v_final, const cozk_vec* v_io, size_t io_start, const uint64_t* r_eq,
                             cozk_output_check** out);
int cozk_output_check_round(cozk_output_check* oc, const uint64_t* r, uint64_t out[12]);
int cozk_output_check_final(cozk_output_check* oc, const uint64_t r[4], uint64_t out[12]);
size_t cozk_output_check_len(const cozk_output_check* oc);
int cozk_output_check_free(cozk_output_check* oc);
/* The same check on a v_final that is a polynomial: PLAIN (one Fr component) or a party's REP3 share; the mode is the polynomial's own.
 * v_final: exactly 2^m unbound entries, 1 <= m < 32; party: 0..2 for REP3, 0 for PLAIN; v_io, io_start and r_eq as above.  The handle
 * is the same type: cozk_output_check_round / _final / _len / _free serve it, with their refusals.  Everything the check sends is linear
 * in the share, and a party's message is the additive share (a + b) * 2^-1 of its two components, so the device works on ONE Fr vector
 *     T[x] = a[x] + b[x] (REP3), a[x] (PLAIN);   d[x] = T[x] - sub * v_io[x - io_start] inside the window, T[x] outside,
 * sub = 1 for PLAIN and for REP3 parties 0 and 1, 0 for REP3 party 2 (cozk_poly_linear_combination puts a public term into party 0's a
 * and party 1's b), and for REP3 the three round values and d's final value are multiplied by 2^-1.  Every value is canonical:
 * _round's out is byte for byte cozk_prod_sumcheck_evals({eq, io_range, cozk_poly_linear_combination({v_final, v_io}, {1, -1}, mode,
 * party)}, 3, 3, ..) in the same state, and _final's out = eq(r), io_range(r) and, for REP3, the additive share (a + b) * 2^-1 of
 * cozk_poly_get_coeff(d, 0, ..) -- the three parties' values sum to the PLAIN ones.  Device memory as above; v_final and v_io are only
 * read and must outlive the handle; a party with sub = 0 reads no v_io entry.
 * Refused with COZK_ERR_INVALID_ARG and a text of its own before any launch, *out NULL, the context working on: a null argument; a
 * length that is not a power of two of at least 2 (and below 2^32); a bound polynomial; party outside its range; a v_io that is not
 * U32; io_len == 0; io_start + io_len > MEM; a vector or polynomial on another device. */
int cozk_output_check_shared_create(cozk_ctx* ctx, const cozk_poly* v_final, const cozk_vec* v_io, size_t io_start, const uint64_t* r_eq,
                                    int party, cozk_output_check** out);

/* ---- The whole ReadWriteMemoryProof in the reference's order, as an in-process harness (csrc/host/memory_proof.hpp): the memory
 * check, the output check, the timestamp range check, under one transcript ("cozk-rw-memory") and one opening accumulator, with ONE
 * reduce_and_prove.  PLAIN only; the trace and the witness of cozk_rw_proof_create for the same fields.  Parity unpinned: pinned by the
 * verifier below and tests/memory_proof_ref.py.
 * prove: steps 1-4 are cozk_rw_proof_prove's, so everything up to and including the claims at r_if is byte for byte cozk_rw_proof's proof
 * at the same config.  Then the output check: the coordinator draws r_eq (log_mem challenges) and sends it, log_mem rounds in the
 * messages of prove_arbitrary_worker (windowed = 1: cozk_output_check_*; windowed = 0: the chained flow's composition on Fr copies of
 * MEM entries, the same bytes, kept for the A/B), then a third opening: v_final from the compact column at the sumcheck's point.  v_io is
 * v_final over the io window [io_start, io_start + io_len) words, so an honest run verifies.  Then cozk_rw_proof's steps 5 and 6.
 * Proof bytes: commitments, the memory-check part, the output sumcheck's compressed polynomials and the v_final claim, the range-check
 * part, the reduced opening.  prefix_len: the offset at which the output check's part begins.
 * The verifier: cozk_rw_proof's checks, and between "leaf claim" and "timestamp: ...":
 *   "output check: shape"        log_mem compressed cubics, one claim
 *   "output check: final claim"  s_last(r_last) == eq(r_eq, r) * io_range(r) * (claim - v_io(r)); io_range(r) and v_io(r) are evaluated
 *                                on the host over the window only, in O(io_len log_mem)
 * tamper: 1-3 are cozk_rw_proof's; 4 adds 1 to v_io[io_len / 2] -- the program's claimed output is wrong, and only the output check's
 * final claim can reject.
 * Refused: whatever cozk_rw_proof_create refuses, io_len < 1, io_start + io_len > MEM, windowed outside 0..1, tamper outside 0..4. */
typedef struct cozk_memory_proof cozk_memory_proof;
typedef struct cozk_memory_proof_config {
    int mode;         /* COZK_MODE_PLAIN; anything else is refused */
    int device;
    int log_n;        /* trace length N = 2^log_n, 1..22 */
    int log_mem;      /* memory of 2^log_mem words, 5..24 */
    int n_slots;      /* 1..4 */
    uint64_t seed;
    int precompute;
    int with_ts;      /* 0 or 1: chain the timestamp range check */
    int leaves_fused; /* as cozk_rw_proof_config */
    int tamper;       /* 0..4: see above */
    uint64_t io_start; /* first word of the io window */
    uint64_t io_len;   /* its length in words, >= 1 */
    int windowed;     /* 1: cozk_output_check_*; 0: the dense composition on Fr copies */
} cozk_memory_proof_config;
typedef struct cozk_memory_proof_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    /* as cozk_rw_proof_result; t_out_ms: the output check (its rounds and the v_final opening) */
    double wall_ms, t_witness_ms, t_commit_ms, t_leaves_ms, t_gp_ms, t_out_ms, t_ts_ms, t_open_ms;
    uint64_t proof_len;
    uint64_t prefix_len;     /* proof[0 .. prefix_len) is cozk_rw_proof's prefix: the commitments and the memory-check part */
    uint64_t out_peak_bytes; /* device memory the output sumcheck held at its peak beyond what it found (the context's allocator's
                              * count plus the growth of its scratch buffers), the v_final opening after it not included */
    uint8_t proof_digest[32];
} cozk_memory_proof_result;
int cozk_memory_proof_create(const cozk_memory_proof_config* cfg, cozk_memory_proof** out);
const char* cozk_memory_proof_error(const cozk_memory_proof* h);
int cozk_memory_proof_destroy(cozk_memory_proof* h);
int cozk_memory_proof_prove(cozk_memory_proof* h, int verify, cozk_memory_proof_result* res);
int cozk_memory_proof_proof_bytes(const cozk_memory_proof* h, uint8_t* out, size_t cap);

/* ---- The memory check and the output check of ReadWriteMemoryProof by three Rep3 parties, as an in-process harness
 * (csrc/host/memory_proof_rep3.hpp): cozk_rw_proof_rep3's sharing and steps with prove_outputs on each party's share of v_final behind
 * them, under one transcript and one opening accumulator.  The instance, v_io, the proof bytes and the verifier are cozk_memory_proof's
 * with with_ts = 0: the proof is byte for byte that harness's PLAIN proof of the same seed and window, for windowed 0 and 1 and
 * leaves_fused 0 and 1 alike, and proof[0 .. prefix_len) is cozk_rw_proof_rep3's proof prefix.
 * prove: cozk_rw_proof_rep3's steps 1-4 (the memory check with its two openings); the coordinator draws r_eq and sends it; log_mem rounds
 * in the messages of prove_arbitrary_worker, every party's round message an additive share (windowed = 1: cozk_output_check_shared_create
 * on the party's polynomial, then cozk_output_check_round / _final; windowed = 0: the dense composition in REP3 on each party's
 * polynomials -- an eq table and two public vectors of MEM entries and the two-component difference, all bound every round); one
 * opening of the shared v_final at the sumcheck's point, its claim additive; ONE reduce_and_prove.
 * tamper: 1 and 2 are cozk_rw_proof_rep3's; 4 adds 1 to v_io[io_len / 2] ("output check: final claim").
 * Refused: whatever cozk_rw_proof_rep3_create refuses, io_len < 1, io_start + io_len > MEM, windowed outside 0..1, tamper 3 and above 4.
 * Not built: the timestamp range check by Rep3 parties, one party per process. */
typedef struct cozk_memory_proof_rep3 cozk_memory_proof_rep3;
typedef struct cozk_memory_proof_rep3_config {
    int devices[3];    /* one device per party */
    int log_n;         /* 1..22 */
    int log_mem;       /* 5..24 */
    int n_slots;       /* 1..4 */
    uint64_t seed;     /* the instance seed: the same seed gives cozk_memory_proof's instance */
    int precompute;
    int leaves_fused;  /* as cozk_rw_proof_rep3_config */
    int tamper;        /* 0, 1, 2 or 4: see above */
    uint64_t io_start; /* first word of the io window */
    uint64_t io_len;   /* its length in words, >= 1 */
    int windowed;      /* 1: the shared device calls; 0: the dense composition in REP3 */
} cozk_memory_proof_rep3_config;
typedef struct cozk_memory_proof_rep3_result {
    int verified; /* 1 ok, 0 rejected, -1 not run */
    /* as cozk_rw_proof_rep3_result; t_out_ms: the output check (its rounds and the v_final opening), the maximum over the parties */
    double wall_ms, t_witness_ms, t_share_ms, t_commit_ms, t_leaves_ms, t_gp_ms, t_out_ms, t_open_ms;
    uint64_t ring_bytes; /* sent over the ring by the three parties together */
    uint64_t proof_len;
    uint64_t prefix_len;     /* proof[0 .. prefix_len) is cozk_rw_proof_rep3's prefix: the commitments and the memory-check part */
    uint64_t out_peak_bytes; /* as cozk_memory_proof_result, the maximum over the parties */
    uint8_t proof_digest[32];
} cozk_memory_proof_rep3_result;
int cozk_memory_proof_rep3_create(const cozk_memory_proof_rep3_config* cfg, cozk_memory_proof_rep3** out);
const char* cozk_memory_proof_rep3_error(const cozk_memory_proof_rep3* h);
int cozk_memory_proof_rep3_destroy(cozk_memory_proof_rep3* h);
int cozk_memory_proof_rep3_prove(cozk_memory_proof_rep3* h, int verify, cozk_memory_proof_rep3_result* res);
int cozk_memory_proof_rep3_proof_bytes(const cozk_memory_proof_rep3* h, uint8_t* out, size_t cap);

/* ---- ONE chained co-jolt worker flow (JoltRep3Prover::prove, co-jolt/src/jolt/vm/jolt/worker.rs:175-266, against its coordinator
 * jolt/vm/jolt/coordinator.rs:118-222): commit-all -> bytecode memory checking -> instruction lookups (primary sumcheck, toggled
 * read / write + dense init / final grand products) -> read-write memory checking + output check -> Spartan (outer + inner + shift) ->
 * ONE reduce_and_prove over all accumulated openings; one transcript, one opening accumulator, all leaves K11 fingerprints of
 * committed columns.  Synthetic Jolt-shaped witness (csrc/host/flow_harness.hpp); oracle/pyflow.py restates it.
 * By default the counters of all three memory-checking instances are seeded streams and the harness verifier skips the
 * multiset-equality check of their hashes.  lookups_witness = 1 makes the instruction lookups a consistent instance (cozk_lasso_witness
 * on the dealer's device, before sharing) and the verifier runs that check for them; the bytecode and the read-write memory keep
 * synthetic counters.  With lookups_witness = 0 the proof bytes are what they were before the field existed.
 * COZK_BYTECODE_FUSED=1 in the environment (read on every prove; unset or 0: four cozk_fingerprint_leaves launches) makes the leaves
 * of the bytecode phase with cozk_bytecode_leaves and cozk_bytecode_init_final_leaves, in PLAIN and REP3; the proof bytes are the same.
 * COZK_RW_FUSED=1 (read on every prove; unset or 0: ten cozk_fingerprint_leaves launches) makes the leaves of the read-write memory
 * phase with cozk_rw_memory_shared_leaves and cozk_rw_memory_shared_init_final_leaves over the flow's own columns (U8 and U32
 * addresses, U32 timestamps, shared or plain value polynomials, the shared v_init), in PLAIN and REP3; the proof bytes are the same.
 * A column of another kind than the calls take fails the prove with a text that names the switch. */
typedef struct cozk_flow cozk_flow;
typedef struct cozk_flow_config {
    int mode;
    int log_n;        /* trace length 2^log_n */
    int log_m;        /* subtable / memory size M of the instruction lookups (Jolt: 16) */
    int log_b;        /* bytecode size */
    int log_mem;      /* read-write memory size */
    int n_mem;        /* NUM_MEMORIES of the instruction lookups (Jolt RV32I: 54) */
    int n_subtables;  /* Subtables::COUNT */
    int devices[3];
    uint64_t seed;
    int precompute;   /* the SRS window table (cozk_bases_upload) */
    int small_witness; /* 0: read / final counters, E polynomials and memory values are uniform field elements -- what a Rep3 party
                        * commits to (its share of every value is uniform) and an upper bound for a plain prover; 1: they are as wide
                        * as a real trace makes them (counters < 2^log_n, subtable entries and memory words 32 bits), so a PLAIN
                        * prover's commitments fill 2 of the 16 windows; Rep3 shares stay uniform either way */
    int lookups_witness; /* 0: read_cts / E / final_cts of the instruction lookups are seeded streams and the verifier skips the
                          * multiset-equality check of their memory-checking hashes.  1: they are a consistent offline-memory-checking
                          * instance made on the device (cozk_lasso_witness over the committed query-chunk columns, the memory flags and
                          * the subtables; needs log_m == 16), shared as ordinary columns, and the verifier checks, per memory m,
                          * rw_hashes[2m] * final_hash(m) == rw_hashes[2m + 1] * init_hash(m % n_subtables)
                          * (lasso/memory_checking/worker.rs:40-127).  The bytecode and the read-write memory keep synthetic counters. */
    int lookups_tamper;  /* tests, with lookups_witness: k > 0 adds 1 to final_cts[0][k - 1] before sharing -- every sumcheck,
                          * opening and fingerprint relation still holds, only the multiset check can reject */
} cozk_flow_config;
typedef struct cozk_flow_result {
    int verified;
    double wall_ms, t_commit_ms, t_bytecode_ms, t_primary_ms, t_lookups_gp_ms, t_rw_ms, t_spartan_ms, t_open_ms, t_worker_ms;
    double t_spartan_build_ms;
    uint64_t bytes_star_up, bytes_star_down, bytes_ring, star_messages;
    uint64_t n_polys, n_openings;
    uint64_t proof_len;
    uint8_t proof_digest[32];
} cozk_flow_result;
int cozk_flow_create(const cozk_flow_config* cfg, cozk_flow** out);
const char* cozk_flow_error(const cozk_flow* h);
int cozk_flow_destroy(cozk_flow* h);
size_t cozk_flow_num_polys(const cozk_flow* h);
cozk_ctx* cozk_flow_ctx(cozk_flow* h, int party);
int cozk_flow_prove(cozk_flow* h, int verify, cozk_flow_result* res);
int cozk_flow_proof_bytes(const cozk_flow* h, uint8_t* out, size_t cap);

/* ---------------------------------------------------------------- profiling ---------------- */
/* HIP-event timing of the dominant kernel (MSM bucket accumulation, k_msm_accum0) on the ctx stream,
 * for bench.py's roofline object: launches, total ms, point additions issued, and the algorithmic
 * bytes of those launches (n x (64 B base + scalar bytes) per MSM). */
int cozk_prof_enable(cozk_ctx* ctx, int on);
int cozk_prof_read(cozk_ctx* ctx, uint64_t* launches, double* total_ms, uint64_t* point_adds,
                   uint64_t* alg_bytes);
/* the same for the HBM-bound kernels of the polynomial seam: slot 0 k_poly_eval_chi, 1 k_poly_lincomb,
 * 2 k_layer_bind_cubic, 3 k_msm_scatter_lds, 4 k_layer_output (cozk_prof_kernel_name; NULL past the last slot);
 * alg_bytes = the algorithmic bytes of SURVEY.md 8d for those launches (stated per kernel in DESIGN.md 4) */
const char* cozk_prof_kernel_name(int slot);
int cozk_prof_read_kernel(cozk_ctx* ctx, int slot, uint64_t* launches, double* total_ms, uint64_t* alg_bytes);
/* Fq Montgomery-multiply micro-benchmark: `iters` dependent products per lane on `lanes` lanes;
 * returns elapsed ms (HIP events) -- the measured integer-ALU peak. */
int cozk_bench_montmul(cozk_ctx* ctx, size_t lanes, int iters, int variant, double* out_ms);

#ifdef __cplusplus
}
#endif
#endif /* COZK_H */
