// The steps of a dense layer's sumcheck round, callable on the device and on the host, and the host tail made of them.
//
// A round of a layer of a few hundred elements moves almost no data: on the device its cost is barriers, a system-scope fence and
// the PCIe hops of the mailbox, on the host it is a few hundred 4 x 64 Montgomery products.  cozk_layer_prove_rounds (poly.hip)
// therefore hands the last rounds of a layer to layer_tail_rounds below.  The kernels and the host tail call the SAME step
// functions, so there is one copy of the bind, the eq pair, the chunk count, the three terms and the eq fold.
#pragma once
#include "../poly.hip.hpp"

// ------------------------------------------------------------------ the steps (device and host)
// Their shape is the one at which every kernel keeps the registers, scratch and occupancy it had with the steps written out in its
// body; the notes say where that decided something.
// bind 4 -> 2 with a zero-padded ragged tail (dense_interleaved_poly.rs:155-195): input chunk ci becomes the bound elements
// 2 ci and 2 ci + 1, stored (lo before hi is computed) and handed back.  All four loads come before the first store, so a
// sequential caller may bind in place (oa == ia): chunk ci writes below what chunk ci + 1 reads.
template <int NC>
static FF_HD void layer_bind_chunk(const fe* ia, const fe* ib, size_t len_in, size_t ci, const fe& r, fe* oa, fe* ob, Sh<NC>& lo, Sh<NC>& hi) {
    Sh<NC> u0 = sh_load_or_zero<NC>(ia, ib, 4 * ci, len_in), u1 = sh_load_or_zero<NC>(ia, ib, 4 * ci + 1, len_in);
    Sh<NC> u2 = sh_load_or_zero<NC>(ia, ib, 4 * ci + 2, len_in), u3 = sh_load_or_zero<NC>(ia, ib, 4 * ci + 3, len_in);
    lo = sh_lerp<NC>(u0, u2, r);
    sh_store<NC>(oa, ob, 2 * ci, lo);
    hi = sh_lerp<NC>(u1, u3, r);
    sh_store<NC>(oa, ob, 2 * ci + 1, hi);
}

// eq evaluations at 0, 2, 3 of the linear factor through (e0, e1)
static FF_HD void eq3(const fe& e0, const fe& e1, fe out[3]) {
    fe m = Fr::sub(e1, e0);
    out[0] = e0;
    out[1] = Fr::add(e1, m);
    out[2] = Fr::add(out[1], m);
}

// chunks of 4 elements that a round sums over: zip() stops at the shorter side of the layer and the eq table
static FF_HD size_t layer_chunk_count(size_t len, bool nested, size_t E1_half, size_t E2_len) {
    size_t nch = (len + 3) / 4;
    size_t limit = nested ? E1_half * E2_len : E2_len / 2;
    return nch > limit ? limit : nch;
}

// the eq pair of item c at 0, 2, 3 from split-eq tables, for the dense layers, the toggle layers and the sparse pair layers alike.
// Not nested: E1 fully bound, the pair comes from E2 (dense_interleaved_poly.rs:218-268).  Nested: Dao-Thaler split, item c
// belongs to x2 = c >> log_E1_half, x1 = c % E1_half (:269-356); `scale` = E2[x2] multiplies its terms -- handed back on its own,
// so that a caller multiplies it into the weights or into its products, whichever keeps fewer values live.
static FF_HD void split_eq_at(bool nested, const fe* E1, int log_E1_half, const fe* E2, size_t c, fe e[3], fe& scale) {
    if (nested) {
        size_t x2 = c >> log_E1_half, x1 = c & (((size_t)1 << log_E1_half) - 1);
        eq3(fe_load(E1 + 2 * x1), fe_load(E1 + 2 * x1 + 1), e);
        scale = fe_load(E2 + x2);
    } else {
        eq3(fe_load(E2 + 2 * c), fe_load(E2 + 2 * c + 1), e);
    }
}
// the dense layer kernels carry E1_half itself, a power of two
static FF_HD void layer_eq_at(bool nested, const fe* E1, size_t E1_half, const fe* E2, size_t c, fe e[3], fe& scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    split_eq_at(nested, E1, __ffsll((long long)E1_half) - 1, E2, c, e, scale);
#else
    split_eq_at(nested, E1, __builtin_ffsll((long long)E1_half) - 1, E2, c, e, scale);
#endif
}

// the three terms of one chunk (l0, r0, l1, r1): t_X = (L(X) x R(X)) e_X [scale] at X = 0, 2, 3.  The caller adds them to its sums
// (with the sums taken by reference here, k_layer_cubic<2, 1> and k_layer_bind_cubic<1, 1> allocate other registers).
template <int NC>
static FF_HD void layer_terms(const Sh<NC>& l0, const Sh<NC>& r0, const Sh<NC>& l1, const Sh<NC>& r1, const fe e[3], bool nested, const fe& scale, fe& t0,
                              fe& t2, fe& t3) {
    Sh<NC> ml = sh_sub<NC>(l1, l0), mr = sh_sub<NC>(r1, r0);
    Sh<NC> l2 = sh_add<NC>(l1, ml), r2 = sh_add<NC>(r1, mr);
    Sh<NC> l3 = sh_add<NC>(l2, ml), r3 = sh_add<NC>(r2, mr);
    t0 = Fr::mul(sh_local_mul<NC>(l0, r0), e[0]);
    t2 = Fr::mul(sh_local_mul<NC>(l2, r2), e[1]);
    t3 = Fr::mul(sh_local_mul<NC>(l3, r3), e[2]);
    if (nested) {
        t0 = Fr::mul(t0, scale);
        t2 = Fr::mul(t2, scale);
        t3 = Fr::mul(t3, scale);
    }
}

// SplitEqPolynomial::bind of one pair: lo + (hi - lo) r
static FF_HD fe fold_pair(const fe* in, size_t i, const fe& r) {
    fe lo = fe_load(in + 2 * i), hi = fe_load(in + 2 * i + 1);
    return Fr::add(lo, Fr::mul(Fr::sub(hi, lo), r));
}

// ------------------------------------------------------------------ the host tail
// One host area holds what the tail works on, in this order: the layer's component a (len elements), its component b (NC = 2),
// the live E1 table, the live E2 table.  The resident kernel and k_layer_tail_out write that layout, the host binds it in place.
struct LayerTailView {
    fe *la, *lb;  // lb: null for NC = 1
    size_t len;
    fe* E1;
    size_t E1_len;
    fe* E2;
    size_t E2_len;
};
static inline size_t layer_tail_entries(int nc, size_t len, size_t E1_len, size_t E2_len) { return (size_t)nc * len + E1_len + E2_len; }
static inline LayerTailView layer_tail_view(fe* area, int nc, size_t len, size_t E1_len, size_t E2_len) {
    fe* eq = area + (size_t)nc * len;
    return LayerTailView{area, nc == 2 ? area + len : nullptr, len, eq, E1_len, eq + E1_len, E2_len};
}

// lengths of layer and eq tables after one bind (what layer_advance and spliteq_advance do to theirs)
struct LayerTailShape {
    size_t len, E1_len, E2_len;
};
static inline LayerTailShape layer_tail_shape_bound(LayerTailShape s) {
    s.len = 2 * ((s.len + 3) / 4);
    if (s.E1_len == 1) s.E2_len /= 2;
    else s.E1_len /= 2;
    return s;
}

// the cubic sums g(0), g(2), g(3) of one round (k_layer_cubic's loop on one lane)
template <int NC>
static inline void layer_tail_sums(const LayerTailView& t, fe s[3]) {
    const bool nested = t.E1_len != 1;
    const size_t E1_half = t.E1_len / 2;
    const size_t nch = layer_chunk_count(t.len, nested, E1_half, t.E2_len);
    s[0] = s[1] = s[2] = Fr::zero();
    for (size_t c = 0; c < nch; c++) {
        fe e[3];
        fe scale = Fr::zero();
        layer_eq_at(nested, t.E1, E1_half, t.E2, c, e, scale);
        Sh<NC> l0 = sh_load_or_zero<NC>(t.la, t.lb, 4 * c, t.len), r0 = sh_load_or_zero<NC>(t.la, t.lb, 4 * c + 1, t.len);
        Sh<NC> l1 = sh_load_or_zero<NC>(t.la, t.lb, 4 * c + 2, t.len), r1 = sh_load_or_zero<NC>(t.la, t.lb, 4 * c + 3, t.len);
        fe t0, t2, t3;
        layer_terms<NC>(l0, r0, l1, r1, e, nested, scale, t0, t2, t3);
        s[0] = Fr::add(s[0], t0);
        s[1] = Fr::add(s[1], t2);
        s[2] = Fr::add(s[2], t3);
    }
}

// bind the layer 4 -> 2 and the eq tables (SplitEqPolynomial::bind: E1 folds until it is one value, which then scales E2; then E2
// folds), all in place
template <int NC>
static inline void layer_tail_bind(LayerTailView& t, const fe& r) {
    const size_t nch_in = (t.len + 3) / 4;
    for (size_t c = 0; c < nch_in; c++) {
        Sh<NC> lo, hi;
        layer_bind_chunk<NC>(t.la, t.lb, t.len, c, r, t.la, t.lb, lo, hi);
    }
    t.len = 2 * nch_in;
    if (t.E1_len == 1) {
        const size_t n = t.E2_len / 2;
        for (size_t i = 0; i < n; i++) fe_store(t.E2 + i, fold_pair(t.E2, i, r));
        t.E2_len = n;
    } else {
        const size_t n = t.E1_len / 2;
        for (size_t i = 0; i < n; i++) fe_store(t.E1 + i, fold_pair(t.E1, i, r));
        t.E1_len = n;
        if (n == 1) {
            const fe sc = fe_load(t.E1);
            for (size_t i = 0; i < t.E2_len; i++) fe_store(t.E2 + i, Fr::mul(fe_load(t.E2 + i), sc));
        }
    }
}

// final claims of the fully bound layer (len == 2): left.a, left.b, right.a, right.b
template <int NC>
static inline void layer_tail_final_claims(const LayerTailView& t, fe out[4]) {
    const fe z = Fr::zero();
    out[0] = fe_load(t.la);
    out[1] = NC == 2 ? fe_load(t.lb) : z;
    out[2] = fe_load(t.la + 1);
    out[3] = NC == 2 ? fe_load(t.lb + 1) : z;
}

// The remaining rounds of one layer's sumcheck on the host: the bind that a device round left pending (have_r), then per round
// the sums -> exchange(j, sums) -> bind with the challenge it returns; after the last round the layer is fully bound and `final`
// gets its claims.  Returns the number of binds done.
template <int NC, class Exchange>
static inline int layer_tail_rounds(LayerTailView& t, bool have_r, fe r, int nrounds, Exchange&& exchange, fe final[4]) {
    int binds = 0;
    for (int j = 0; j < nrounds; j++) {
        if (have_r) {
            layer_tail_bind<NC>(t, r);
            binds++;
        }
        fe s[3];
        layer_tail_sums<NC>(t, s);
        r = exchange(j, s);
        have_r = true;
    }
    if (have_r) {
        layer_tail_bind<NC>(t, r);
        binds++;
    }
    layer_tail_final_claims<NC>(t, final);
    return binds;
}
