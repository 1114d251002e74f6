/*
 * ORACLE (test infrastructure, NOT product code) -- plain-C restatement of the co-zkvms hot path
 * (Pippenger MSM, Rep3 share arithmetic, dense/interleaved polynomial ops, GKR grand product,
 * opening reduction, PST13 open) and of the synthetic pipeline of co-zkvms_amd/csrc/harness.hip.
 * Two jobs: (1) second, independent oracle cross-checked against the exact big-int oracle
 * (oracle/pyref.py, oracle/pyharness.py); (2) the same-run CPU baseline (`cpu_baseline.kind = "port"`)
 * of bench.py, multi-threaded with OpenMP like the reference's rayon loops.
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.
 * Each function cites the reference file:line it follows (relative to the reference root).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "bn254.h"

/* ------------------------------------------------------------------ basics exported for tests */
void orc_fp_binop(int base_field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    const fp_params* P = base_field ? &FQ : &FR;
    for (size_t i = 0; i < n; i++) {
        fp x, y, r;
        memcpy(x.l, a + 4 * i, 32);
        memcpy(y.l, b + 4 * i, 32);
        if (op == 0) fp_add(P, &r, &x, &y);
        else if (op == 1) fp_sub(P, &r, &x, &y);
        else fp_mul(P, &r, &x, &y);
        memcpy(out + 4 * i, r.l, 32);
    }
}
/* the cores this process may really use: the CPU affinity mask capped by the cgroup's CPU quota and by OMP_NUM_THREADS (a container
 * on a 128-thread host with a 16-CPU share runs 16 threads' worth of work, and 128 OpenMP threads only fight over them) */
static int effective_cpus(void) {
    int n = 0;
#ifdef _OPENMP
    n = omp_get_num_procs();
#endif
    if (n < 1) n = 1;
    FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (f) {
        char q[64];
        long long period = 0;
        if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            long long quota = atoll(q);
            int c = (int)((quota + period - 1) / period);
            if (c >= 1 && c < n) n = c;
        }
        fclose(f);
    }
    const char* o = getenv("OMP_NUM_THREADS");
    if (o && atoi(o) >= 1 && atoi(o) < n) n = atoi(o);
    const char* e = getenv("ORC_THREADS");
    if (e && atoi(e) >= 1) n = atoi(e);
    return n;
}
/* test hook: the fast Fq product (bn254.h fq_mul_fast) -- tests/test_oracle.py compares it with fp_mul and the Python oracle */
void orc_fq_mul_fast(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
        fp x, y, r;
        memcpy(x.l, a + 4 * i, 32);
        memcpy(y.l, b + 4 * i, 32);
        fq_mul_fast(&r, &x, &y);
        memcpy(out + 4 * i, r.l, 32);
    }
}
int orc_num_threads(void) {
#ifdef _OPENMP
    static int set = 0;
    if (!set) {
        omp_set_num_threads(effective_cpus());
        set = 1;
    }
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* ------------------------------------------------------------------ Pippenger MSM
 * arkworks `VariableBaseMSM::msm_bigint` / jolt-core `msm` shape: signed c-bit digits,
 * c = 3 if n < 32 else floor(0.69 log2 n) + 2, 2^(c-1) Jacobian buckets per window filled by mixed
 * additions in input order, running-sum reduction, Horner combine with c doublings; windows run in
 * parallel (rayon there, OpenMP here).  Call sites: pst13.rs:286-294,319-323,461-469. */
static int msm_window_bits(size_t n) {
    if (n < 32) return 3;
    int lg = 0;
    while (((size_t)1 << (lg + 1)) <= n) lg++;
    return lg * 69 / 100 + 2;
}
/* scalars: canonical (non-Montgomery) 4-limb integers, only the low `nbits` bits may be set */
static void msm_core(const g1a* bases, const uint64_t* scalars, size_t n, int nbits, g1a* out) {
    if (n == 0) { fp_zero(&out->x); fp_zero(&out->y); out->inf = 1; return; }
    int c = msm_window_bits(n);
    if (c > nbits + 1) c = nbits + 1;
    int nwin = (nbits + c - 1) / c + 1;
    /* signed digits */
    int32_t* digits = (int32_t*)malloc(sizeof(int32_t) * n * (size_t)nwin);
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) {
        const uint64_t* s = scalars + 4 * i;
        int64_t carry = 0;
        for (int w = 0; w < nwin; w++) {
            int bit = w * c;
            uint64_t v = 0;
            if (bit < 256) {
                int limb = bit / 64, sh = bit % 64;
                v = s[limb] >> sh;
                if (sh + c > 64 && limb < 3) v |= s[limb + 1] << (64 - sh);
                v &= ((uint64_t)1 << c) - 1;
            }
            int64_t d = (int64_t)v + carry;
            if (d > ((int64_t)1 << (c - 1))) { d -= (int64_t)1 << c; carry = 1; } else carry = 0;
            digits[i * nwin + w] = (int32_t)d;
        }
    }
    g1x* wsum = (g1x*)malloc(sizeof(g1x) * nwin);
    size_t nb = (size_t)1 << (c - 1);
#pragma omp parallel for schedule(dynamic, 1)
    for (int w = 0; w < nwin; w++) {
        g1x* buckets = (g1x*)malloc(sizeof(g1x) * nb);
        for (size_t b = 0; b < nb; b++) g1x_identity(&buckets[b]);
        for (size_t i = 0; i < n; i++) {
            int32_t d = digits[i * nwin + w];
            if (d > 0) g1x_add_affine(&buckets[d - 1], &buckets[d - 1], &bases[i], 0);
            else if (d < 0) g1x_add_affine(&buckets[-d - 1], &buckets[-d - 1], &bases[i], 1);
        }
        g1x run, acc;
        g1x_identity(&run);
        g1x_identity(&acc);
        for (size_t b = nb; b-- > 0;) {
            g1x_add(&run, &run, &buckets[b]);
            g1x_add(&acc, &acc, &run);
        }
        wsum[w] = acc;
        free(buckets);
    }
    g1x total;
    g1x_identity(&total);
    for (int w = nwin - 1; w >= 0; w--) {
        for (int k = 0; k < c; k++) g1x_double(&total, &total);
        g1x_add(&total, &total, &wsum[w]);
    }
    g1x_to_affine(out, &total);
    free(wsum);
    free(digits);
}

static void load_bases(const uint64_t* xy, const uint8_t* inf, size_t n, g1a* out) {
    for (size_t i = 0; i < n; i++) {
        memcpy(out[i].x.l, xy + 8 * i, 32);
        memcpy(out[i].y.l, xy + 8 * i + 4, 32);
        out[i].inf = inf ? inf[i] : 0;
    }
}
/* scalars_mont: Fr Montgomery limbs (arkworks layout) */
void orc_msm(const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars_mont, size_t n, uint64_t* out_xy, int* out_inf) {
    (void)orc_num_threads();
    g1a* bases = (g1a*)malloc(sizeof(g1a) * (n ? n : 1));
    load_bases(xy, inf, n, bases);
    uint64_t* sc = (uint64_t*)malloc(32 * (n ? n : 1));
    for (size_t i = 0; i < n; i++) {
        fp m, c;
        memcpy(m.l, scalars_mont + 4 * i, 32);
        fp_from_mont(&FR, &c, &m);
        memcpy(sc + 4 * i, c.l, 32);
    }
    g1a r;
    msm_core(bases, sc, n, 254, &r);
    memcpy(out_xy, r.x.l, 32);
    memcpy(out_xy + 4, r.y.l, 32);
    *out_inf = r.inf;
    free(sc);
    free(bases);
}

/* ------------------------------------------------------------------ SplitMix64 streams (shared
 * with cozk_vec_fill_random and oracle/pyref.py synthetic_fr) */
static uint64_t sm_next(uint64_t* s) {
    *s += 0x9E3779B97F4A7C15ull;
    uint64_t z = *s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void stream_fr(uint64_t seed, uint64_t i, fp* out_mont) {
    uint64_t s = seed + i * 0xD1342543DE82EF95ull;
    fp v;
    for (;;) {
        v.l[0] = sm_next(&s); v.l[1] = sm_next(&s); v.l[2] = sm_next(&s);
        v.l[3] = sm_next(&s) & (((uint64_t)1 << 62) - 1);
        if (!fp_geq(v.l, FR.mod)) break;
    }
    fp_to_mont(&FR, out_mont, &v);
}
static uint64_t stream_small(uint64_t seed, uint64_t i, int bits) {
    uint64_t s = seed + i * 0xD1342543DE82EF95ull;
    uint64_t v = sm_next(&s);
    return bits < 64 ? v & (((uint64_t)1 << bits) - 1) : v;
}

/* ------------------------------------------------------------------ keyed PRF (restates co-zkvms_amd/csrc/prf.hip.hpp and
 * oracle/pyref.py prf_fr): element j of a stream = one ChaCha12 block, rejection-sampled below r */
static uint32_t prf_rotl(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }
#define ORC_QR(a, b, c, d) a += b; d ^= a; d = prf_rotl(d, 16); c += d; b ^= c; b = prf_rotl(b, 12); a += b; d ^= a; d = prf_rotl(d, 8); c += d; b ^= c; b = prf_rotl(b, 7);
static void prf_block(const uint8_t key[32], uint64_t counter, uint32_t attempt, uint32_t out[16]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
    for (int i = 0; i < 8; i++) s[4 + i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) | ((uint32_t)key[4 * i + 3] << 24);
    s[12] = (uint32_t)counter; s[13] = (uint32_t)(counter >> 32); s[14] = 0x4b5a4f43u; s[15] = attempt;
    uint32_t x[16];
    memcpy(x, s, sizeof x);
    for (int i = 0; i < 6; i++) {
        ORC_QR(x[0], x[4], x[8], x[12]) ORC_QR(x[1], x[5], x[9], x[13]) ORC_QR(x[2], x[6], x[10], x[14]) ORC_QR(x[3], x[7], x[11], x[15])
        ORC_QR(x[0], x[5], x[10], x[15]) ORC_QR(x[1], x[6], x[11], x[12]) ORC_QR(x[2], x[7], x[8], x[13]) ORC_QR(x[3], x[4], x[9], x[14])
    }
    for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}
static void prf_fr(const uint8_t key[32], uint64_t j, fp* out_mont) {
    for (uint32_t attempt = 0;; attempt++) {
        uint32_t w[16];
        prf_block(key, j, attempt, w);
        for (int half = 0; half < 2; half++) {
            fp v;
            for (int i = 0; i < 4; i++) v.l[i] = (uint64_t)w[8 * half + 2 * i] | ((uint64_t)w[8 * half + 2 * i + 1] << 32);
            v.l[3] &= ((uint64_t)1 << 62) - 1;
            if (!fp_geq(v.l, FR.mod)) { fp_to_mont(&FR, out_mont, &v); return; }
        }
    }
}
/* keys of the synthetic harness runs (csrc/host/prover.hpp harness_prf_key) */
static void harness_prf_key(uint64_t seed, uint64_t idx, uint8_t out[32]) {
    uint64_t s = seed ^ (0xC0DEC0DEull + idx * 0x9E3779B97F4A7C15ull);
    for (int i = 0; i < 4; i++) {
        uint64_t z = sm_next(&s);
        for (int b = 0; b < 8; b++) out[8 * i + b] = (uint8_t)(z >> (8 * b));
    }
}

/* out[i] = PRF(key, counter + i), Montgomery limbs (cross-check against pyref.prf_fr and cozk_vec_fill_prf) */
void orc_prf_fr(const uint8_t* key, uint64_t counter, size_t n, uint64_t* out) {
    for (size_t i = 0; i < n; i++) {
        fp v;
        prf_fr(key, counter + i, &v);
        memcpy(out + 4 * i, v.l, 32);
    }
}

/* ------------------------------------------------------------------ SHA-256 + transcript */
typedef struct { uint32_t h[8]; uint8_t buf[64]; uint64_t len; size_t fill; } sha256;
static uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static const uint32_t SHA_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
static void sha_init(sha256* s) {
    static const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    memcpy(s->h, iv, 32);
    s->len = 0;
    s->fill = 0;
}
static void sha_block(sha256* s, const uint8_t* p) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
        uint32_t s0 = rotr32(w[i - 15], 7) ^ rotr32(w[i - 15], 18) ^ (w[i - 15] >> 3);
        uint32_t s1 = rotr32(w[i - 2], 17) ^ rotr32(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = s->h[0], b = s->h[1], c = s->h[2], d = s->h[3], e = s->h[4], f = s->h[5], g = s->h[6], h = s->h[7];
    for (int i = 0; i < 64; i++) {
        uint32_t t1 = h + (rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25)) + ((e & f) ^ (~e & g)) + SHA_K[i] + w[i];
        uint32_t t2 = (rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    s->h[0] += a; s->h[1] += b; s->h[2] += c; s->h[3] += d; s->h[4] += e; s->h[5] += f; s->h[6] += g; s->h[7] += h;
}
static void sha_update(sha256* s, const uint8_t* p, size_t n) {
    s->len += n;
    while (n) {
        size_t k = 64 - s->fill < n ? 64 - s->fill : n;
        memcpy(s->buf + s->fill, p, k);
        s->fill += k; p += k; n -= k;
        if (s->fill == 64) { sha_block(s, s->buf); s->fill = 0; }
    }
}
static void sha_final(sha256* s, uint8_t out[32]) {
    uint64_t bits = s->len * 8;
    uint8_t pad = 0x80, z = 0, lb[8];
    sha_update(s, &pad, 1);
    while (s->fill != 56) sha_update(s, &z, 1);
    for (int i = 0; i < 8; i++) lb[i] = (uint8_t)(bits >> (56 - 8 * i));
    sha_update(s, lb, 8);
    for (int i = 0; i < 8; i++) { out[4 * i] = s->h[i] >> 24; out[4 * i + 1] = s->h[i] >> 16; out[4 * i + 2] = s->h[i] >> 8; out[4 * i + 3] = s->h[i]; }
}

typedef struct { uint8_t* p; size_t n, cap; } bytes;
static void by_put(bytes* b, const void* d, size_t n) {
    if (b->n + n > b->cap) { b->cap = (b->n + n) * 2 + 64; b->p = (uint8_t*)realloc(b->p, b->cap); }
    memcpy(b->p + b->n, d, n);
    b->n += n;
}
static void by_u64(bytes* b, uint64_t v) { by_put(b, &v, 8); } /* little-endian host */
static void by_fr(bytes* b, const fp* mont) { fp c; fp_from_mont(&FR, &c, mont); by_put(b, c.l, 32); }
static void by_g1(bytes* b, const g1a* p) {
    if (p->inf) { uint8_t z[64] = {0}; z[63] = 0x40; by_put(b, z, 64); return; }
    fp x, y;
    fp_from_mont(&FQ, &x, &p->x);
    fp_from_mont(&FQ, &y, &p->y);
    by_put(b, x.l, 32);
    by_put(b, y.l, 32);
    /* ark-ec SWFlags::from_y_coordinate, written also when uncompressed: bit 7 of the last byte iff y > -y */
    fp ny, zero;
    fp_zero(&zero);
    fp_sub(&FQ, &ny, &zero, &p->y);
    fp_from_mont(&FQ, &ny, &ny);
    int neg = 0;
    for (int i = 3; i >= 0; i--) if (y.l[i] != ny.l[i]) { neg = y.l[i] > ny.l[i]; break; }
    if (neg) b->p[b->n - 1] |= 0x80;
}

typedef struct { uint8_t state[32]; uint32_t n_rounds; } transcript;
static void tr_init(transcript* t, const char* label) {
    sha256 s; sha_init(&s); sha_update(&s, (const uint8_t*)label, strlen(label)); sha_final(&s, t->state); t->n_rounds = 0;
}
static void tr_absorb(transcript* t, const uint8_t* d, size_t n) {
    sha256 s; sha_init(&s);
    sha_update(&s, t->state, 32);
    uint8_t c[4] = {(uint8_t)t->n_rounds, (uint8_t)(t->n_rounds >> 8), (uint8_t)(t->n_rounds >> 16), (uint8_t)(t->n_rounds >> 24)};
    sha_update(&s, c, 4);
    sha_update(&s, d, n);
    sha_final(&s, t->state);
    t->n_rounds++;
}
static void tr_scalars(transcript* t, const fp* xs, size_t n) {
    bytes b = {0, 0, 0};
    for (size_t i = 0; i < n; i++) by_fr(&b, &xs[i]);
    tr_absorb(t, b.p, b.n);
    free(b.p);
}
static void tr_point(transcript* t, const g1a* p) {
    bytes b = {0, 0, 0};
    /* raw x || y, no serialization flags (jolt's append_point hashes the two coordinates; zeros for infinity) */
    if (p->inf) { uint8_t z[64] = {0}; by_put(&b, z, 64); }
    else { fp x, y; fp_from_mont(&FQ, &x, &p->x); fp_from_mont(&FQ, &y, &p->y); by_put(&b, x.l, 32); by_put(&b, y.l, 32); }
    tr_absorb(t, b.p, b.n);
    free(b.p);
}
static void tr_challenge(transcript* t, fp* out) {
    tr_absorb(t, (const uint8_t*)"challenge", 9);
    fp c = {{0, 0, 0, 0}};
    memcpy(c.l, t->state, 16);
    fp_to_mont(&FR, out, &c);
}

/* ------------------------------------------------------------------ shares */
typedef struct { fp a, b; } sh; /* plain mode uses only .a */
static fp TWO_INV_M; /* (r+1)/2, snarks-core/src/field.rs:5-7 */
static int g_mode;   /* 1 plain, 2 rep3 */
static void init_consts(void) {
    fp c = {{0xa1f0fac9f8000001ull, 0x9419f4243cdcb848ull, 0xdc2822db40c0ac2eull, 0x183227397098d014ull}};
    fp_to_mont(&FR, &TWO_INV_M, &c);
}
static inline void sh_sub_(sh* r, const sh* x, const sh* y) { fp_sub(&FR, &r->a, &x->a, &y->a); if (g_mode == 2) fp_sub(&FR, &r->b, &x->b, &y->b); }
static inline void sh_add_(sh* r, const sh* x, const sh* y) { fp_add(&FR, &r->a, &x->a, &y->a); if (g_mode == 2) fp_add(&FR, &r->b, &x->b, &y->b); }
static inline void sh_mulp(sh* r, const sh* x, const fp* c) { fp_mul(&FR, &r->a, &x->a, c); if (g_mode == 2) fp_mul(&FR, &r->b, &x->b, c); }
static inline void sh_lerp_(sh* r, const sh* lo, const sh* hi, const fp* c) { sh d; sh_sub_(&d, hi, lo); sh_mulp(&d, &d, c); sh_add_(r, lo, &d); }
/* Share x Share -> additive (mpc-types/.../rep3/arithmetic/ops.rs:71-78), literally 3 products */
static inline void sh_local_mul_(fp* r, const sh* x, const sh* y) {
    fp t;
    fp_mul(&FR, r, &x->a, &y->a);
    if (g_mode == 2) {
        fp_mul(&FR, &t, &x->a, &y->b); fp_add(&FR, r, r, &t);
        fp_mul(&FR, &t, &x->b, &y->a); fp_add(&FR, r, r, &t);
    }
}
/* into_additive (types.rs:76-81) */
static inline void sh_into_additive_(fp* r, const sh* x) {
    if (g_mode == 1) { *r = x->a; return; }
    fp t; fp_add(&FR, &t, &x->a, &x->b); fp_mul(&FR, r, &t, &TWO_INV_M);
}
static const sh SH_ZERO = {{{0, 0, 0, 0}}, {{0, 0, 0, 0}}};

/* EqPolynomial::evals (big-endian) */
static fp* eq_evals(const fp* r, int nv) {
    size_t n = (size_t)1 << nv;
    fp* ev = (fp*)malloc(sizeof(fp) * n);
    fp_one(&FR, &ev[0]);
    size_t cur = 1;
    for (int j = 0; j < nv; j++) {
        for (size_t i = cur; i-- > 0;) {
            fp hi; fp_mul(&FR, &hi, &ev[i], &r[j]);
            fp_sub(&FR, &ev[2 * i], &ev[i], &hi);
            ev[2 * i + 1] = hi;
        }
        cur *= 2;
    }
    return ev;
}

/* UniPoly::from_evals, n in {3,4} */
static void unipoly_from_evals(const fp* ev, int n, fp* cf) {
    fp inv2 = TWO_INV_M;
    if (n == 3) {
        fp t; fp_dbl(&FR, &t, &ev[1]); fp c2; fp_sub(&FR, &c2, &ev[2], &t); fp_add(&FR, &c2, &c2, &ev[0]); fp_mul(&FR, &c2, &c2, &inv2);
        cf[0] = ev[0]; cf[2] = c2; fp_sub(&FR, &cf[1], &ev[1], &ev[0]); fp_sub(&FR, &cf[1], &cf[1], &c2);
        return;
    }
    /* solve by Lagrange: explicit Vandermonde inverse on nodes 0..3
       c3 = (-e0 + 3e1 - 3e2 + e3)/6 ; c2 = (2e0 - 5e1 + 4e2 - e3)/2 ; c1 = (-11e0 + 18e1 - 9e2 + 2e3)/6 */
    fp six, inv6; fp_from_u64(&FR, &six, 6); fp_inv(&FR, &inv6, &six);
    fp k[12]; for (int i = 0; i < 12; i++) fp_from_u64(&FR, &k[i], (uint64_t)i);
    fp t, acc;
    /* c3 */
    fp_sub(&FR, &acc, &ev[3], &ev[0]); fp_mul(&FR, &t, &ev[1], &k[3]); fp_add(&FR, &acc, &acc, &t); fp_mul(&FR, &t, &ev[2], &k[3]); fp_sub(&FR, &acc, &acc, &t);
    fp_mul(&FR, &cf[3], &acc, &inv6);
    /* c2 */
    fp_mul(&FR, &acc, &ev[0], &k[2]); fp_mul(&FR, &t, &ev[1], &k[5]); fp_sub(&FR, &acc, &acc, &t); fp_mul(&FR, &t, &ev[2], &k[4]); fp_add(&FR, &acc, &acc, &t); fp_sub(&FR, &acc, &acc, &ev[3]);
    fp_mul(&FR, &cf[2], &acc, &inv2);
    /* c1 */
    fp_mul(&FR, &acc, &ev[1], &k[9]); fp_dbl(&FR, &acc, &acc); fp_mul(&FR, &t, &ev[0], &k[11]); fp_sub(&FR, &acc, &acc, &t); fp_mul(&FR, &t, &ev[2], &k[9]); fp_sub(&FR, &acc, &acc, &t); fp_dbl(&FR, &t, &ev[3]); fp_add(&FR, &acc, &acc, &t);
    fp_mul(&FR, &cf[1], &acc, &inv6);
    cf[0] = ev[0];
}
static void unipoly_eval(const fp* cf, int n, const fp* x, fp* out) {
    fp acc; fp_zero(&acc);
    for (int i = n - 1; i >= 0; i--) { fp_mul(&FR, &acc, &acc, x); fp_add(&FR, &acc, &acc, &cf[i]); }
    *out = acc;
}

/* ------------------------------------------------------------------ split-eq + interleaved layer */
typedef struct { fp *E1, *E2; size_t E1_len, E2_len; int nv; } spliteq;
static void spliteq_new(spliteq* e, const fp* w, int nv) {
    int m = nv / 2;
    e->nv = nv;
    e->E2 = eq_evals(w, m);
    e->E1 = eq_evals(w + m, nv - m);
    e->E2_len = (size_t)1 << m;
    e->E1_len = (size_t)1 << (nv - m);
}
static void spliteq_bind(spliteq* e, const fp* r) {
    if (e->E1_len == 1) {
        size_t n = e->E2_len / 2;
        for (size_t i = 0; i < n; i++) { fp d; fp_sub(&FR, &d, &e->E2[2 * i + 1], &e->E2[2 * i]); fp_mul(&FR, &d, &d, r); fp_add(&FR, &e->E2[i], &e->E2[2 * i], &d); }
        e->E2_len = n;
    } else {
        size_t n = e->E1_len / 2;
        for (size_t i = 0; i < n; i++) { fp d; fp_sub(&FR, &d, &e->E1[2 * i + 1], &e->E1[2 * i]); fp_mul(&FR, &d, &d, r); fp_add(&FR, &e->E1[i], &e->E1[2 * i], &d); }
        e->E1_len = n;
        if (n == 1) for (size_t i = 0; i < e->E2_len; i++) fp_mul(&FR, &e->E2[i], &e->E2[i], &e->E1[0]);
    }
}
static void spliteq_free(spliteq* e) { free(e->E1); free(e->E2); }

static inline void eq3_(const fp* e0, const fp* e1, fp out[3]) {
    fp m; fp_sub(&FR, &m, e1, e0);
    out[0] = *e0; fp_add(&FR, &out[1], e1, &m); fp_add(&FR, &out[2], &out[1], &m);
}
static inline sh lget(const sh* c, size_t i, size_t len) { return i < len ? c[i] : SH_ZERO; }
static inline void cubic_terms(const sh* c, size_t k, size_t len, const fp e[3], fp t[3]) {
    sh l0 = lget(c, 4 * k, len), r0 = lget(c, 4 * k + 1, len), l1 = lget(c, 4 * k + 2, len), r1 = lget(c, 4 * k + 3, len);
    sh ml, mr, l2, l3, r2, r3;
    sh_sub_(&ml, &l1, &l0); sh_sub_(&mr, &r1, &r0);
    sh_add_(&l2, &l1, &ml); sh_add_(&l3, &l2, &ml);
    sh_add_(&r2, &r1, &mr); sh_add_(&r3, &r2, &mr);
    sh_local_mul_(&t[0], &l0, &r0); fp_mul(&FR, &t[0], &t[0], &e[0]);
    sh_local_mul_(&t[1], &l2, &r2); fp_mul(&FR, &t[1], &t[1], &e[1]);
    sh_local_mul_(&t[2], &l3, &r3); fp_mul(&FR, &t[2], &t[2], &e[2]);
}
/* compute_cubic (dense_interleaved_poly.rs:210-365): s = [g(0), g(2), g(3)] partial sums */
static void layer_cubic(const sh* c, size_t len, const spliteq* eq, fp s[3]) {
    size_t nch = (len + 3) / 4;
    fp s0, s1, s2; fp_zero(&s0); fp_zero(&s1); fp_zero(&s2);
    if (eq->E1_len == 1) {
        size_t lim = eq->E2_len / 2; if (nch > lim) nch = lim;
#pragma omp parallel
        {
            fp a0, a1, a2; fp_zero(&a0); fp_zero(&a1); fp_zero(&a2);
#pragma omp for schedule(static) nowait
            for (size_t k = 0; k < nch; k++) {
                fp e[3], t[3]; eq3_(&eq->E2[2 * k], &eq->E2[2 * k + 1], e);
                cubic_terms(c, k, len, e, t);
                fp_add(&FR, &a0, &a0, &t[0]); fp_add(&FR, &a1, &a1, &t[1]); fp_add(&FR, &a2, &a2, &t[2]);
            }
#pragma omp critical
            { fp_add(&FR, &s0, &s0, &a0); fp_add(&FR, &s1, &s1, &a1); fp_add(&FR, &s2, &s2, &a2); }
        }
    } else {
        size_t h1 = eq->E1_len / 2;
        size_t npow = 1; while (npow < len) npow <<= 1;
        size_t chunk = npow / eq->E2_len; if (chunk < 1) chunk = 1;
#pragma omp parallel
        {
            fp a0, a1, a2; fp_zero(&a0); fp_zero(&a1); fp_zero(&a2);
#pragma omp for schedule(static) nowait
            for (size_t x2 = 0; x2 < eq->E2_len; x2++) {
                size_t base = x2 * chunk;
                if (base >= len) continue;
                size_t plen = len - base < chunk ? len - base : chunk;
                fp i0, i1, i2; fp_zero(&i0); fp_zero(&i1); fp_zero(&i2);
                size_t nc = (plen + 3) / 4; if (nc > h1) nc = h1;
                for (size_t j = 0; j < nc; j++) {
                    fp e[3], t[3]; eq3_(&eq->E1[2 * j], &eq->E1[2 * j + 1], e);
                    cubic_terms(c + base, j, plen, e, t);
                    fp_add(&FR, &i0, &i0, &t[0]); fp_add(&FR, &i1, &i1, &t[1]); fp_add(&FR, &i2, &i2, &t[2]);
                }
                fp_mul(&FR, &i0, &i0, &eq->E2[x2]); fp_mul(&FR, &i1, &i1, &eq->E2[x2]); fp_mul(&FR, &i2, &i2, &eq->E2[x2]);
                fp_add(&FR, &a0, &a0, &i0); fp_add(&FR, &a1, &a1, &i1); fp_add(&FR, &a2, &a2, &i2);
            }
#pragma omp critical
            { fp_add(&FR, &s0, &s0, &a0); fp_add(&FR, &s1, &s1, &a1); fp_add(&FR, &s2, &s2, &a2); }
        }
    }
    s[0] = s0; s[1] = s1; s[2] = s2;
}
/* bind (dense_interleaved_poly.rs:155-195): returns new length; out must hold 2*ceil(len/4) */
static size_t layer_bind(const sh* c, size_t len, const fp* r, sh* out) {
    size_t nch = (len + 3) / 4;
#pragma omp parallel for schedule(static)
    for (size_t k = 0; k < nch; k++) {
        sh u0 = lget(c, 4 * k, len), u1 = lget(c, 4 * k + 1, len), u2 = lget(c, 4 * k + 2, len), u3 = lget(c, 4 * k + 3, len);
        sh_lerp_(&out[2 * k], &u0, &u2, r);
        sh_lerp_(&out[2 * k + 1], &u1, &u3, r);
    }
    return 2 * nch;
}

/* ------------------------------------------------------------------ pipeline (twin of harness.hip) */
typedef struct {
    int mode, log_n, n_fr, n_u16, n_u32, n_flags, n_small, gp_batch, gp_log_leaves;
    uint64_t seed;
} orc_config;
typedef struct {
    double t_setup_s, t_commit_s, t_gp_construct_s, t_gp_prove_s, t_eval_s, t_open_s, t_total_s;
    uint8_t digest[32];
    uint64_t proof_len;
    int threads;
} orc_result;

static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

/* per-party share vector of the secret stream(seed) (harness.hip make_share_vectors) */
static sh* make_shares(uint64_t seed, size_t n, int party) {
    sh* out = (sh*)malloc(sizeof(sh) * n);
    uint8_t k0[32], k1[32];
    harness_prf_key(seed, 101, k0);
    harness_prf_key(seed, 102, k1);
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) {
        fp v; stream_fr(seed, i, &v);
        if (g_mode == 1) { out[i].a = v; fp_zero(&out[i].b); continue; }
        fp t0, t1, t2; prf_fr(k0, i, &t0); prf_fr(k1, i, &t1);
        fp_sub(&FR, &t2, &v, &t0); fp_sub(&FR, &t2, &t2, &t1);
        if (party == 0) { out[i].a = t0; out[i].b = t2; }
        else if (party == 1) { out[i].a = t1; out[i].b = t0; }
        else { out[i].a = t2; out[i].b = t1; }
    }
    return out;
}

typedef struct { int is_public; size_t len; sh** parts; /* per party */ uint64_t* small; int small_bits; } wpoly;

static void commit_poly(const g1a* bases, const wpoly* p, int party, g1a* out) {
    size_t n = p->len;
    uint64_t* sc = (uint64_t*)malloc(32 * n);
    int bits = 254;
    if (p->is_public) {
        for (size_t i = 0; i < n; i++) { sc[4 * i] = p->small[i]; sc[4 * i + 1] = sc[4 * i + 2] = sc[4 * i + 3] = 0; }
        bits = p->small_bits;
    } else {
#pragma omp parallel for schedule(static)
        for (size_t i = 0; i < n; i++) { fp c; fp_from_mont(&FR, &c, &p->parts[party][i].a); memcpy(sc + 4 * i, c.l, 32); }
    }
    msm_core(bases, sc, n, bits, out);
    free(sc);
}

int orc_pipeline(const orc_config* cfg, orc_result* res, uint8_t* proof_out, size_t proof_cap) {
    init_consts();
    g_mode = cfg->mode;
    int np = cfg->mode == 2 ? 3 : 1;
    int nv = cfg->log_n;
    size_t N = (size_t)1 << nv;
    uint64_t seed = cfg->seed;
    double T0 = now_s();
    res->threads = orc_num_threads();
    /* ---- SRS: powers_of_g[i][b] = g^{eq_le(t[i..], b)} (MultilinearPC::setup), levels concatenated */
    fp* t = (fp*)malloc(sizeof(fp) * nv);
    for (int i = 0; i < nv; i++) stream_fr(seed ^ 0x7A7A7A7Aull, (uint64_t)i, &t[i]);
    size_t total = ((size_t)1 << (nv + 1)) - 2;
    g1a* srs = (g1a*)malloc(sizeof(g1a) * total);
    size_t* loff = (size_t*)malloc(sizeof(size_t) * (nv + 1));
    g1a gen; fp_one(&FQ, &gen.x); fp_from_u64(&FQ, &gen.y, 2); gen.inf = 0;
    for (int i = 0; i < nv; i++) {
        loff[i] = ((size_t)1 << (nv + 1)) - ((size_t)1 << (nv - i + 1));
        int k = nv - i;
        fp* rev = (fp*)malloc(sizeof(fp) * k);
        for (int j = 0; j < k; j++) rev[j] = t[nv - 1 - j];
        fp* ev = eq_evals(rev, k);
        size_t n = (size_t)1 << k;
#pragma omp parallel for schedule(dynamic, 16)
        for (size_t b = 0; b < n; b++) {
            fp c; fp_from_mont(&FR, &c, &ev[b]);
            g1j pj; g1_scalar_mul(&pj, &gen, c.l);
            g1j_to_affine(&srs[loff[i] + b], &pj);
        }
        free(ev); free(rev);
    }
    /* ---- witness */
    int K = cfg->n_fr + cfg->n_u16 + cfg->n_u32 + cfg->n_flags;
    wpoly* polys = (wpoly*)calloc((size_t)K, sizeof(wpoly));
    int j = 0;
    for (int k = 0; k < cfg->n_fr; k++, j++) {
        polys[j].is_public = 0; polys[j].len = N; polys[j].parts = (sh**)malloc(sizeof(sh*) * np);
        for (int p = 0; p < np; p++) polys[j].parts[p] = make_shares(seed + 1000ull * (uint64_t)(j + 1), N, p);
    }
    int counts[3] = {cfg->n_u16, cfg->n_u32, cfg->n_flags}, bitsv[3] = {16, 32, 1};
    for (int g = 0; g < 3; g++)
        for (int k = 0; k < counts[g]; k++, j++) {
            polys[j].is_public = 1; polys[j].len = N; polys[j].small_bits = bitsv[g];
            polys[j].small = (uint64_t*)malloc(8 * N);
            sh* frv = (sh*)malloc(sizeof(sh) * N);
            for (size_t i = 0; i < N; i++) { polys[j].small[i] = stream_small(seed + 1000ull * (uint64_t)(j + 1), i, bitsv[g]); fp_from_u64(&FR, &frv[i].a, polys[j].small[i]); fp_zero(&frv[i].b); }
            polys[j].parts = (sh**)malloc(sizeof(sh*) * np);
            for (int p = 0; p < np; p++) polys[j].parts[p] = frv;
        }
    wpoly* small = (wpoly*)calloc((size_t)(cfg->n_small ? cfg->n_small : 1), sizeof(wpoly));
    for (int k = 0; k < cfg->n_small; k++) {
        small[k].is_public = 0; small[k].len = N >> 4; small[k].parts = (sh**)malloc(sizeof(sh*) * np);
        for (int p = 0; p < np; p++) small[k].parts[p] = make_shares(seed + 300000ull + 1000ull * (uint64_t)k, N >> 4, p);
    }
    size_t nleaves = (size_t)cfg->gp_batch << cfg->gp_log_leaves;
    sh** leaves = (sh**)malloc(sizeof(sh*) * np);
    for (int p = 0; p < np; p++) leaves[p] = make_shares(seed + 500000ull, nleaves, p);
    double T1 = now_s();
    res->t_setup_s = T1 - T0;

    transcript tr; tr_init(&tr, "cozk-harness");
    bytes proof = {0, 0, 0};
    /* ---- 1. commit (every party MSMs every polynomial; shared: sum of parties; public: P0's) */
    g1a* cm = (g1a*)malloc(sizeof(g1a) * (size_t)(K + cfg->n_small + 1));
    /* batch_msm on the CPU is rayon over the polynomials, each an independent MSM (jolt-core batch_msm):
     * one (polynomial, party) MSM per thread; the window-level loops inside msm_core then run serially (nested
     * parallelism is off), which is what keeps all host cores busy when there are more polynomials than windows */
    {
        int total = (K + cfg->n_small) * np;
        g1a* parts = (g1a*)malloc(sizeof(g1a) * (size_t)total);
#pragma omp parallel for schedule(dynamic, 1)
        for (int t = 0; t < total; t++) {
            int i = t / np, q = t % np;
            const wpoly* p = i < K ? &polys[i] : &small[i - K];
            commit_poly(srs, p, q, &parts[t]);
        }
        for (int i = 0; i < K + cfg->n_small; i++) {
            const wpoly* p = i < K ? &polys[i] : &small[i - K];
            g1j acc; g1j_identity(&acc);
            for (int q = 0; q < np; q++) g1j_add_affine(&acc, &acc, &parts[i * np + q]);
            if (p->is_public) cm[i] = parts[i * np]; else g1j_to_affine(&cm[i], &acc);
        }
        free(parts);
    }
    for (int i = 0; i < K + cfg->n_small; i++) tr_point(&tr, &cm[i]);
    by_u64(&proof, (uint64_t)K);
    for (int i = 0; i < K; i++) { by_u64(&proof, (uint64_t)nv); by_g1(&proof, &cm[i]); }
    by_u64(&proof, (uint64_t)cfg->n_small);
    for (int i = 0; i < cfg->n_small; i++) { by_u64(&proof, (uint64_t)(nv - 4)); by_g1(&proof, &cm[K + i]); }
    double T2 = now_s();
    res->t_commit_s = T2 - T1;

    /* ---- 2. grand product: construct (grand_product.rs:239-255) */
    int L = cfg->gp_log_leaves;
    sh*** layers = (sh***)malloc(sizeof(sh**) * L);
    size_t* llen = (size_t*)malloc(sizeof(size_t) * L);
    layers[0] = leaves; llen[0] = nleaves;
    uint64_t mask_ctr = 0;
    for (int l = 1; l < L; l++) {
        size_t n_out = (llen[l - 1] + 1) / 2;
        layers[l] = (sh**)malloc(sizeof(sh*) * np);
        fp** ca = (fp**)malloc(sizeof(fp*) * np);
        for (int p = 0; p < np; p++) {
            ca[p] = (fp*)malloc(sizeof(fp) * n_out);
            const sh* prev = layers[l - 1][p];
            size_t plen = llen[l - 1];
            uint8_t key_self[32], key_prev[32];
            harness_prf_key(seed, (uint64_t)p, key_self);
            harness_prf_key(seed, (uint64_t)((p + 2) % 3), key_prev);
#pragma omp parallel for schedule(static)
            for (size_t jj = 0; jj < n_out; jj++) {
                sh lft = lget(prev, 2 * jj, plen), rgt = lget(prev, 2 * jj + 1, plen);
                sh_local_mul_(&ca[p][jj], &lft, &rgt);
                if (np == 3) {
                    fp m1, m2; prf_fr(key_self, mask_ctr + jj, &m1); prf_fr(key_prev, mask_ctr + jj, &m2);
                    fp_add(&FR, &ca[p][jj], &ca[p][jj], &m1); fp_sub(&FR, &ca[p][jj], &ca[p][jj], &m2);
                }
            }
        }
        for (int p = 0; p < np; p++) {
            layers[l][p] = (sh*)malloc(sizeof(sh) * n_out);
            for (size_t jj = 0; jj < n_out; jj++) { layers[l][p][jj].a = ca[p][jj]; if (np == 3) layers[l][p][jj].b = ca[(p + 2) % 3][jj]; else fp_zero(&layers[l][p][jj].b); }
        }
        for (int p = 0; p < np; p++) free(ca[p]);
        free(ca);
        llen[l] = n_out;
        mask_ctr += n_out;
    }
    double T3 = now_s();
    res->t_gp_construct_s = T3 - T2;
    /* prove (grand_product.rs:56-130,143-217; sumcheck.rs:96-165) */
    size_t nout = llen[L - 1] / 2;
    fp* outputs = (fp*)malloc(sizeof(fp) * nout);
    for (size_t i = 0; i < nout; i++) {
        fp_zero(&outputs[i]);
        for (int p = 0; p < np; p++) { fp v; sh_local_mul_(&v, &layers[L - 1][p][2 * i], &layers[L - 1][p][2 * i + 1]); fp_add(&FR, &outputs[i], &outputs[i], &v); }
    }
    tr_scalars(&tr, outputs, nout);
    size_t npad = 1; int nvo = 0; while (npad < nout) { npad <<= 1; nvo++; }
    int rcap = nvo + L + 2;
    fp* r = (fp*)malloc(sizeof(fp) * rcap);
    int rlen = nvo;
    for (int i = 0; i < nvo; i++) tr_challenge(&tr, &r[i]);
    fp claim_pub; fp_zero(&claim_pub);
    { fp* ev = eq_evals(r, nvo); for (size_t i = 0; i < nout; i++) { fp tt; fp_mul(&FR, &tt, &ev[i], &outputs[i]); fp_add(&FR, &claim_pub, &claim_pub, &tt); } free(ev); }
    by_u64(&proof, nout); for (size_t i = 0; i < nout; i++) by_fr(&proof, &outputs[i]);
    by_u64(&proof, (uint64_t)L);
    fp claims[3]; for (int p = 0; p < np; p++) { if (p == 0) claims[p] = claim_pub; else fp_zero(&claims[p]); }
    for (int l = L - 1; l >= 0; l--) {
        size_t len = llen[l];
        sh* cur[3]; sh* alt[3];
        for (int p = 0; p < np; p++) { cur[p] = (sh*)malloc(sizeof(sh) * len); memcpy(cur[p], layers[l][p], sizeof(sh) * len); alt[p] = (sh*)malloc(sizeof(sh) * (len / 2 + 4)); }
        spliteq eqs[3]; for (int p = 0; p < np; p++) spliteq_new(&eqs[p], r, rlen);
        int rounds = rlen;
        fp* rs = (fp*)malloc(sizeof(fp) * (rounds + 1));
        by_u64(&proof, (uint64_t)rounds);
        fp prev[3]; for (int p = 0; p < np; p++) prev[p] = claims[p];
        for (int rd = 0; rd < rounds; rd++) {
            fp poly[4]; for (int k = 0; k < 4; k++) fp_zero(&poly[k]);
            for (int p = 0; p < np; p++) {
                fp s[3]; layer_cubic(cur[p], len, &eqs[p], s);
                fp ev[4]; ev[0] = s[0]; fp_sub(&FR, &ev[1], &prev[p], &s[0]); ev[2] = s[1]; ev[3] = s[2];
                fp cf[4]; unipoly_from_evals(ev, 4, cf);
                for (int k = 0; k < 4; k++) fp_add(&FR, &poly[k], &poly[k], &cf[k]);
            }
            fp comp[3] = {poly[0], poly[2], poly[3]};
            tr_scalars(&tr, comp, 3);
            fp rj; tr_challenge(&tr, &rj);
            rs[rd] = rj;
            fp nxt; unipoly_eval(poly, 4, &rj, &nxt);
            size_t nl = 0;
            for (int p = 0; p < np; p++) { nl = layer_bind(cur[p], len, &rj, alt[p]); sh* tmp = cur[p]; cur[p] = alt[p]; alt[p] = tmp; spliteq_bind(&eqs[p], &rj); }
            len = nl;
            for (int p = 0; p < np; p++) { if (p == 0) prev[p] = nxt; else fp_zero(&prev[p]); }
            by_u64(&proof, 3); for (int k = 0; k < 3; k++) by_fr(&proof, &comp[k]);
        }
        fp left, right; fp_zero(&left); fp_zero(&right);
        for (int p = 0; p < np; p++) { fp_add(&FR, &left, &left, &cur[p][0].a); fp_add(&FR, &right, &right, &cur[p][1].a); }
        tr_scalars(&tr, &left, 1); tr_scalars(&tr, &right, 1);
        for (int i = 0; i < rounds; i++) r[i] = rs[rounds - 1 - i];
        fp r_layer; tr_challenge(&tr, &r_layer);
        for (int p = 0; p < np; p++) { sh s; sh_lerp_(&s, &cur[p][0], &cur[p][1], &r_layer); sh_into_additive_(&claims[p], &s); }
        r[rounds] = r_layer; rlen = rounds + 1;
        by_fr(&proof, &left); by_fr(&proof, &right);
        for (int p = 0; p < np; p++) { free(cur[p]); free(alt[p]); spliteq_free(&eqs[p]); }
        free(rs);
    }
    double T4 = now_s();
    res->t_gp_prove_s = T4 - T3;

    /* ---- 3. openings: batch_evaluate + append (dense_mlpoly.rs:160-192; opening_proof.rs:77-128) */
    int half = (K + 1) / 2;
    int ngroups = 1 + (half < K ? 1 : 0) + (cfg->n_small > 0 ? 1 : 0);
    typedef struct { const wpoly* ps; int cnt; const fp* point; int plen; } group;
    group groups[3]; int gi = 0;
    groups[gi++] = (group){polys, half, r + (rlen - nv), nv};
    if (half < K) groups[gi++] = (group){polys + half, K - half, r, nv};
    if (cfg->n_small > 0) groups[gi++] = (group){small, cfg->n_small, r + (rlen - (nv - 4)), nv - 4};
    fp* r_gp = (fp*)malloc(sizeof(fp) * rlen); memcpy(r_gp, r, sizeof(fp) * rlen);
    for (int g = 0; g < ngroups; g++) { /* the points alias r, which stays intact from here on */
        size_t off = groups[g].point - r; groups[g].point = r_gp + off;
    }
    by_u64(&proof, (uint64_t)ngroups);
    /* per party, per group: RLC polynomial + eq table + claim share */
    sh* op_poly[3][3]; fp* op_eq[3][3]; sh op_claim[3][3]; size_t op_len[3];
    for (int g = 0; g < ngroups; g++) {
        int cnt = groups[g].cnt; size_t len = groups[g].ps[0].len;
        fp* eq = eq_evals(groups[g].point, groups[g].plen);
        fp* cl = (fp*)malloc(sizeof(fp) * cnt);
        for (int i = 0; i < cnt; i++) {
            fp_zero(&cl[i]);
            for (int p = 0; p < np; p++) {
                const wpoly* wp = &groups[g].ps[i];
                if (wp->is_public && p != 0) continue; /* additive::promote_to_trivial_share: P0 only */
                fp acc; fp_zero(&acc);
#pragma omp parallel
                {
                    fp a; fp_zero(&a);
#pragma omp for schedule(static) nowait
                    for (size_t x = 0; x < len; x++) {
                        fp v, tt;
                        if (wp->is_public) v = wp->parts[p][x].a; else sh_into_additive_(&v, &wp->parts[p][x]);
                        fp_mul(&FR, &tt, &v, &eq[x]); fp_add(&FR, &a, &a, &tt);
                    }
#pragma omp critical
                    fp_add(&FR, &acc, &acc, &a);
                }
                fp_add(&FR, &cl[i], &cl[i], &acc);
            }
        }
        by_u64(&proof, (uint64_t)cnt); for (int i = 0; i < cnt; i++) by_fr(&proof, &cl[i]);
        fp rho; tr_challenge(&tr, &rho);
        fp* pw = (fp*)malloc(sizeof(fp) * cnt); fp_one(&FR, &pw[0]);
        for (int i = 1; i < cnt; i++) fp_mul(&FR, &pw[i], &pw[i - 1], &rho);
        fp batched; fp_zero(&batched);
        for (int i = 0; i < cnt; i++) { fp tt; fp_mul(&FR, &tt, &pw[i], &cl[i]); fp_add(&FR, &batched, &batched, &tt); }
        op_len[g] = len;
        for (int p = 0; p < np; p++) {
            sh* acc = (sh*)calloc(len, sizeof(sh));
#pragma omp parallel for schedule(static)
            for (size_t x = 0; x < len; x++)
                for (int i = 0; i < cnt; i++) {
                    const wpoly* wp = &groups[g].ps[i];
                    if (wp->is_public) { /* add_public: P0 -> a, P1 -> b (plain: the value itself) */
                        fp tt; fp_mul(&FR, &tt, &wp->parts[p][x].a, &pw[i]);
                        if (p == 0) fp_add(&FR, &acc[x].a, &acc[x].a, &tt); else if (p == 1) fp_add(&FR, &acc[x].b, &acc[x].b, &tt);
                    } else { sh tt; sh_mulp(&tt, &wp->parts[p][x], &pw[i]); sh_add_(&acc[x], &acc[x], &tt); }
                }
            op_poly[p][g] = acc;
            op_eq[p][g] = (fp*)malloc(sizeof(fp) * len); memcpy(op_eq[p][g], eq, sizeof(fp) * len);
            fp_zero(&op_claim[p][g].a); fp_zero(&op_claim[p][g].b);
            if (g_mode == 1 || p == 0) op_claim[p][g].a = batched; else if (p == 1) op_claim[p][g].b = batched;
        }
        free(pw); free(cl); free(eq);
    }
    double T5 = now_s();
    res->t_eval_s = T5 - T4;

    /* ---- 4. reduce_and_prove (opening_proof.rs:181-437) */
    fp rho2; tr_challenge(&tr, &rho2);
    fp coeffs[3]; fp_one(&FR, &coeffs[0]); for (int g = 1; g < ngroups; g++) fp_mul(&FR, &coeffs[g], &coeffs[g - 1], &rho2);
    int max_nv = 0; for (int g = 0; g < ngroups; g++) if (groups[g].plen > max_nv) max_nv = groups[g].plen;
    /* keep the unbound RLC polynomials (share a) for the joint polynomial */
    fp* unbound_a[3][3];
    for (int p = 0; p < np; p++) for (int g = 0; g < ngroups; g++) { unbound_a[p][g] = (fp*)malloc(sizeof(fp) * op_len[g]); for (size_t x = 0; x < op_len[g]; x++) unbound_a[p][g][x] = op_poly[p][g][x].a; }
    fp es[3];
    for (int p = 0; p < np; p++) {
        fp_zero(&es[p]);
        for (int g = 0; g < ngroups; g++) {
            sh cl = op_claim[p][g];
            if (groups[g].plen != max_nv) { fp sc; fp_from_u64(&FR, &sc, (uint64_t)1 << (max_nv - groups[g].plen)); sh_mulp(&cl, &cl, &sc); }
            fp ad, tt; sh_into_additive_(&ad, &cl); fp_mul(&FR, &tt, &ad, &coeffs[g]); fp_add(&FR, &es[p], &es[p], &tt);
        }
    }
    size_t cur_len[3]; for (int g = 0; g < ngroups; g++) cur_len[g] = op_len[g];
    fp* r_red = (fp*)malloc(sizeof(fp) * (max_nv + 1));
    by_u64(&proof, (uint64_t)max_nv);
    for (int rd = 0; rd < max_nv; rd++) {
        int remaining = max_nv - rd;
        fp uni[3]; for (int k = 0; k < 3; k++) fp_zero(&uni[k]);
        for (int p = 0; p < np; p++) {
            fp c0, c2; fp_zero(&c0); fp_zero(&c2);
            for (int g = 0; g < ngroups; g++) {
                fp e0, e2;
                if (remaining <= groups[g].plen) {
                    size_t hh = cur_len[g] / 2; const sh* pl = op_poly[p][g]; const fp* eq = op_eq[p][g];
                    fp a0, a2; fp_zero(&a0); fp_zero(&a2);
#pragma omp parallel
                    {
                        fp l0, l2; fp_zero(&l0); fp_zero(&l2);
#pragma omp for schedule(static) nowait
                        for (size_t x = 0; x < hh; x++) {
                            sh m; fp ad, tt;
                            sh_mulp(&m, &pl[x], &eq[x]); sh_into_additive_(&ad, &m); fp_add(&FR, &l0, &l0, &ad);
                            sh pb; sh_add_(&pb, &pl[x + hh], &pl[x + hh]); sh_sub_(&pb, &pb, &pl[x]);
                            fp eb; fp_dbl(&FR, &eb, &eq[x + hh]); fp_sub(&FR, &eb, &eb, &eq[x]);
                            sh_mulp(&m, &pb, &eb); sh_into_additive_(&tt, &m); fp_add(&FR, &l2, &l2, &tt);
                        }
#pragma omp critical
                        { fp_add(&FR, &a0, &a0, &l0); fp_add(&FR, &a2, &a2, &l2); }
                    }
                    e0 = a0; e2 = a2;
                } else {
                    int rem = remaining - groups[g].plen - 1;
                    fp sc, ad; fp_from_u64(&FR, &sc, (uint64_t)1 << rem); sh_into_additive_(&ad, &op_claim[p][g]); fp_mul(&FR, &e0, &ad, &sc); e2 = e0;
                }
                fp tt; fp_mul(&FR, &tt, &e0, &coeffs[g]); fp_add(&FR, &c0, &c0, &tt);
                fp_mul(&FR, &tt, &e2, &coeffs[g]); fp_add(&FR, &c2, &c2, &tt);
            }
            fp ev[3]; ev[0] = c0; fp_sub(&FR, &ev[1], &es[p], &c0); ev[2] = c2;
            fp cf[3]; unipoly_from_evals(ev, 3, cf);
            for (int k = 0; k < 3; k++) fp_add(&FR, &uni[k], &uni[k], &cf[k]);
        }
        fp comp[2] = {uni[0], uni[2]};
        tr_scalars(&tr, comp, 2);
        fp rj; tr_challenge(&tr, &rj); r_red[rd] = rj;
        fp nc; unipoly_eval(uni, 3, &rj, &nc);
        for (int p = 0; p < np; p++) { if (p == 0) es[p] = nc; else fp_zero(&es[p]); }
        for (int g = 0; g < ngroups; g++) {
            if (remaining <= groups[g].plen) {
                size_t hh = cur_len[g] / 2;
                for (int p = 0; p < np; p++) {
                    sh* pl = op_poly[p][g]; fp* eq = op_eq[p][g];
#pragma omp parallel for schedule(static)
                    for (size_t x = 0; x < hh; x++) {
                        sh_lerp_(&pl[x], &pl[x], &pl[x + hh], &rj);
                        fp d; fp_sub(&FR, &d, &eq[x + hh], &eq[x]); fp_mul(&FR, &d, &d, &rj); fp_add(&FR, &eq[x], &eq[x], &d);
                    }
                }
                cur_len[g] = hh;
            }
        }
        by_u64(&proof, 2); by_fr(&proof, &comp[0]); by_fr(&proof, &comp[1]);
    }
    fp red_claims[3];
    for (int g = 0; g < ngroups; g++) { fp_zero(&red_claims[g]); for (int p = 0; p < np; p++) { fp ad; sh_into_additive_(&ad, &op_poly[p][g][0]); fp_add(&FR, &red_claims[g], &red_claims[g], &ad); } }
    tr_scalars(&tr, red_claims, (size_t)ngroups);
    by_u64(&proof, (uint64_t)ngroups); for (int g = 0; g < ngroups; g++) by_fr(&proof, &red_claims[g]);
    fp gamma; tr_challenge(&tr, &gamma);
    fp gpw[3]; fp_one(&FR, &gpw[0]); for (int g = 1; g < ngroups; g++) fp_mul(&FR, &gpw[g], &gpw[g - 1], &gamma);
    /* PST13 open (pst13.rs:428-474) per party on the joint share-a polynomial, proofs summed (:110-122) */
    g1j* pf = (g1j*)malloc(sizeof(g1j) * nv); for (int i = 0; i < nv; i++) g1j_identity(&pf[i]);
    for (int p = 0; p < np; p++) {
        fp* rr = (fp*)calloc(N, sizeof(fp));
        for (int g = 0; g < ngroups; g++)
#pragma omp parallel for schedule(static)
            for (size_t x = 0; x < op_len[g]; x++) { fp tt; fp_mul(&FR, &tt, &unbound_a[p][g][x], &gpw[g]); fp_add(&FR, &rr[x], &rr[x], &tt); }
        size_t cur = N;
        for (int i = 0; i < nv; i++) {
            size_t hh = cur / 2; const fp* pt = &r_red[max_nv - 1 - i]; /* point reversed (pst13.rs:134) */
            uint64_t* sc = (uint64_t*)malloc(32 * cur);
            fp* nr = (fp*)malloc(sizeof(fp) * hh);
#pragma omp parallel for schedule(static)
            for (size_t b = 0; b < hh; b++) {
                fp q; fp_sub(&FR, &q, &rr[2 * b + 1], &rr[2 * b]);
                fp d; fp_mul(&FR, &d, &q, pt); fp_add(&FR, &nr[b], &rr[2 * b], &d);
                fp c; fp_from_mont(&FR, &c, &q);
                memcpy(sc + 8 * b, c.l, 32); memcpy(sc + 8 * b + 4, c.l, 32); /* scalars q[x >> 1] (:459) */
            }
            g1a pi; msm_core(srs + loff[i], sc, cur, 254, &pi);
            g1j_add_affine(&pf[i], &pf[i], &pi);
            free(sc); free(rr); rr = nr; cur = hh;
        }
        free(rr);
    }
    by_u64(&proof, (uint64_t)nv);
    for (int i = 0; i < nv; i++) { g1a a; g1j_to_affine(&a, &pf[i]); by_g1(&proof, &a); }
    double T6 = now_s();
    res->t_open_s = T6 - T5;
    res->t_total_s = T6 - T1;
    sha256 s; sha_init(&s); sha_update(&s, proof.p, proof.n); sha_final(&s, res->digest);
    res->proof_len = proof.n;
    int rc = 0;
    if (proof_out) { if (proof_cap < proof.n) rc = -1; else memcpy(proof_out, proof.p, proof.n); }
    free(proof.p);
    /* (allocations of the witness are left to process exit in the bounded baseline run; the test
       sizes are tiny) */
    return rc;
}
