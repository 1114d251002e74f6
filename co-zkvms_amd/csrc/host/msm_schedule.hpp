// The launch schedule of the batched MSM (msm.hip: msm_batch): how a batch is cut into tail blocks and launch sets, their launch
// order, each set's sort shape and the room it needs.  Host-only: no kernel, no HIP call, no device pointer.  msm_schedule() raises
// every refusal before it returns and msm.hip then executes what it returned, so a refused batch has enqueued and reserved nothing.
// tests/native/msm_schedule_check prints it without a GPU; tests/test_msm_schedule_host.py holds that to tests/test_msm_schedule_model.py.
#pragma once
#include "../common.hpp"  // COZK_SCALAR_*, COZK_REQUIRE, CozkError
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

static constexpr uint32_t NB = 1u << 15;  // buckets per group
static constexpr int TPB = 256;           // threads per block of the gather and fold kernels (sizes `blk`)
static constexpr int LTPB = 1024;         // launch bound of the LDS-histogram kernels; the launch width is MsmSetSchedule::ltpb
// launch width and workgroups-per-polynomial cap of a sort that runs alone, and of one that slips under a gather
static constexpr int MSM_WIDE_LTPB = 1024, MSM_NARROW_LTPB = 256;
static constexpr int MSM_WIDE_WGS = 64, MSM_NARROW_WGS = 64;
// polynomials per launch set, with the window table and with 16 window groups (measured: 64 small-scalar polynomials per set
// beat 16 by 1.7 ms per proof)
static constexpr size_t MSM_SET_POLYS_TABLE = 64, MSM_SET_POLYS_GROUPS = 4;
// the bucket-reduction tail (running sums, Horner, to-affine) is latency-bound, so it runs ONCE over the dense bucket sums of
// up to MSM_TAIL_GROUPS bucket groups (256 polynomials with the table, 16 without) instead of once per launch set
static constexpr size_t MSM_TAIL_GROUPS = 256;
// bounds of the references per launch set (msm_schedule) and of COZK_MSM_SET_REFS_LOG2
static constexpr int MSM_SET_REFS_LOG2_MIN = 28, MSM_SET_REFS_LOG2_MAX = 30, MSM_SET_REFS_PIN_MIN = 12, MSM_SET_REFS_PIN_MAX = 31;

// 16-bit windows per scalar kind (plain form: the top window of the small kinds takes the carry); the one copy of the table,
// msm.hip holds ScalarKind<K>::NWIN to it
static constexpr int MSM_KINDS = COZK_SCALAR_I64 + 1;
static constexpr int MSM_KIND_NWIN[MSM_KINDS] = {16, 1, 2, 3, 5, 5};
static constexpr const char* MSM_KIND_NAME[MSM_KINDS] = {"FR", "U8", "U16", "U32", "U64", "I64"};
static inline int kind_offset_slot(int kind) {  // index into cozk_bases::SliceSum::cS, -1 for kinds that are always plain
    return kind == COZK_SCALAR_U16 ? 0 : kind == COZK_SCALAR_U32 ? 1 : kind == COZK_SCALAR_U64 ? 2 : -1;
}

// ---- the two rules that size a set's sort (restated in tests/test_msm_schedule_model.py)
//
// Shape.  The 256-thread shape exists to slip a sort under the gather kernel of the set launched before it; wide
// workgroups wait for that gather's grid to drain and then run with the chip to themselves.  Measured in place on the
// bench's commit at 2^20 (profiles/msm_schedule_kernel_stats_{before,after}.txt), sort of a set of 18 field-element
// columns whose own gather lasts 22.5 ms: beside a gather the narrow sort spans 18.9 ms (0.84 of its own gather) and slows
// that gather by ~7 %; with nothing beside it the narrow sort takes 0.86 + 4.52 ms (0.24), the wide one 0.68 + 4.13 ms
// (0.214: the scatter is bound by its 4-byte writes to random lines, not by the shape).  With x = predecessor's
// references / own references (a gather lasts as long as its references), the narrow shape leaves
// (1 - x / 0.84) x 0.24 + 0.07 x of the own gather's length exposed, the wide one 0.214: they meet at x ~ 0.12.  The rule
// takes 1/8.  The sets of one batch are equal-sized apart from a small one, so nothing in the bench sits near the threshold.
static inline bool msm_sort_wide(uint64_t pred_refs, uint64_t own_refs) { return 8 * pred_refs < own_refs; }

// Workgroups per polynomial.  A sort workgroup pays for 2^15 LDS counters whatever the column holds (zeroing, the sweep, one
// global atomic per non-empty bucket).  A field-element column of 2^20 scalars gives each of its 64 workgroups 2^18 digits
// for them (measured on such columns: 64 beats 16 workgroups 2 x; they keep one workgroup per 4096 scalars).  The other
// kinds place 1 to 5 digits per scalar: sized by scalars a u16 column hands each workgroup 2^14 digits and issues nearly
// one global atomic per reference, so they are sized by digits.  Measured at 2^20 beside the gather (commit per step, median
// of three alternated runs, shape rule on): one workgroup per 4096 scalars 95.90 ms; per 2^15 digits 95.68; 2^16 94.98 and
// 95.25 (two sessions); 2^17 95.57; 2^18 96.08; 2^20 103.97 (too few workgroups for the slots the gather leaves free, and
// a flag column serialises on one LDS counter per workgroup).  2^16: histogram of 32 u16 columns 5.4 -> 3.6 ms.
static constexpr int MSM_WG_DIGITS_LOG2 = 16;
static inline uint32_t msm_sort_wgs(int kind, size_t max_n, int wg_digits_log2, uint32_t wgs_max) {
    uint64_t w = kind == COZK_SCALAR_FR || wg_digits_log2 == 0 ? ((uint64_t)max_n + 4095) / 4096
                                                               : (((uint64_t)max_n * MSM_KIND_NWIN[kind] + (1ull << wg_digits_log2) - 1) >> wg_digits_log2);
    if (w < 1) w = 1;
    return (uint32_t)(w > wgs_max ? wgs_max : w);
}

// ---- the switches.  None of them changes a result.
//   COZK_MSM_DIGIT_FORM = auto (default) | plain | offset
//   COZK_MSM_SHAPE_RULE=0      sort shape as before msm_sort_wide: wide for the first set of a batch and serial batches only
//   COZK_MSM_WG_DIGITS_LOG2=d  digits per sort workgroup of the narrow kinds (10..24); 0: one workgroup per 4096 scalars
//   COZK_MSM_SET_REFS_LOG2=c   (12..31) pins the references per launch set: A/B runs, tests that cut a small batch into many sets
//   COZK_MSM_SERIAL            no side stream: every sort runs in front of its own accumulation
//   COZK_MSM_LTPB / _WGS       override the launch width and the workgroups-per-polynomial cap of both sort shapes
//   COZK_TRACE_MSM             one line per launch set on stderr (msm_set_trace_line)
enum { MSM_FORM_AUTO = 0, MSM_FORM_PLAIN = 1, MSM_FORM_OFFSET = 2 };
static constexpr int MSM_BY_SHAPE = INT_MIN;  // ltpb / wgs: not overridden
struct MsmOptions {
    int digit_form = MSM_FORM_AUTO, wg_digits_log2 = MSM_WG_DIGITS_LOG2;
    int set_refs_log2 = 0;  // 0: a quarter of the tail block within [2^28, 2^30]
    int ltpb = MSM_BY_SHAPE, wgs = MSM_BY_SHAPE;
    bool shape_rule = true, serial = false, trace = false;
};
static inline int msm_digit_form_parse(const char* e) {
    if (!e || !*e || !strcmp(e, "auto")) return MSM_FORM_AUTO;
    if (!strcmp(e, "plain")) return MSM_FORM_PLAIN;
    if (!strcmp(e, "offset")) return MSM_FORM_OFFSET;
    throw CozkError(COZK_ERR_INVALID_ARG, "COZK_MSM_DIGIT_FORM must be auto, plain or offset");
}
static inline void msm_options_check(const MsmOptions& o) {
    COZK_REQUIRE(o.wg_digits_log2 == 0 || (o.wg_digits_log2 >= 10 && o.wg_digits_log2 <= 24), "COZK_MSM_WG_DIGITS_LOG2 must be 0 or 10..24");
}
// The digit form, the shape rule, the digits per workgroup and the set cap are read at every call, so that one process can
// compare them; the serial switch, the shape overrides and the trace once per process.  An override of 0 counts as not set.
static inline MsmOptions msm_options_env() {
    static const bool serial = getenv("COZK_MSM_SERIAL") != nullptr, trace = getenv("COZK_TRACE_MSM") != nullptr;
    static const int ltpb = getenv("COZK_MSM_LTPB") ? atoi(getenv("COZK_MSM_LTPB")) : 0, wgs = getenv("COZK_MSM_WGS") ? atoi(getenv("COZK_MSM_WGS")) : 0;
    MsmOptions o;
    o.digit_form = msm_digit_form_parse(getenv("COZK_MSM_DIGIT_FORM"));
    if (const char* e = getenv("COZK_MSM_SHAPE_RULE")) o.shape_rule = atoi(e) != 0;
    if (const char* e = getenv("COZK_MSM_WG_DIGITS_LOG2")) o.wg_digits_log2 = atoi(e);
    msm_options_check(o);
    if (const char* e = getenv("COZK_MSM_SET_REFS_LOG2")) o.set_refs_log2 = atoi(e);
    o.serial = serial;
    o.trace = trace;
    if (ltpb) o.ltpb = ltpb;
    if (wgs) o.wgs = wgs;
    return o;
}
// may column (kind, n) take the offset digit form?  Only on a window table, and an empty column has nothing to offset.
static inline bool msm_column_eligible(int nwin, const MsmOptions& o, int kind, size_t n) {
    return nwin == 16 && o.digit_form != MSM_FORM_PLAIN && kind_offset_slot(kind) >= 0 && n != 0;
}

// ---- the schedule
// One launch set = P MSMs (polynomial p runs over bases[offsets[p] .. offsets[p]+ns[p]); scalars[p] = device
// pointer of kinds[p]) in two phases that msm_batch pipelines on two streams:
//   msm_sort        digits -> histogram -> offsets -> sorted point references (LDS atomics, HBM writes)
//   msm_accumulate  gather + fold levels -> one XYZZ sum per bucket in `dense_out` (integer ALU)
// The phases stress different units, so the sort of set k+1 hides behind the accumulation of set k.
struct MsmKindRun {                // the columns of one kind in a set on a window table: one launch of each sort kernel
    int kind;
    uint32_t first;                // its first descriptor
    std::vector<uint32_t> cols;    // polynomial indices inside the set, in descriptor order (empty columns get none)
    size_t max_n;
    uint32_t wgs;                  // workgroups per polynomial (msm_sort_wgs)
    uint32_t form_grid;            // grid width of the form count (kinds with an offset form)
};
struct MsmSetSchedule {
    size_t first = 0;              // columns [first, first + P) of the caller's arrays
    uint32_t P = 0, G = 1, nb = 0, L0 = 8;
    uint32_t fold_levels = 1;      // fold levels queued before the heavy-bucket launch
    uint64_t M = 0, bound = 0, maxseg0 = 0;  // references if every digit is non-zero, the most of them one polynomial places, level-0 segments
    uint64_t part_entries = 0, exc_entries = 0, blk_entries = 0;  // what partA / partB, exc and blk must hold (refs: M)
    bool table = false;            // window table (G == 1): LDS sort by kind runs, length-ordered gather
    bool wide = false;             // sort shape (msm_sort_wide): nothing runs beside this set's sort that could hide it
    int ltpb = 0;                  // launch width of the LDS sort kernels
    uint32_t wgs_max = 0;
    std::vector<MsmKindRun> runs;  // launch order; empty without the table (there every non-empty column is a launch of its own)
    uint64_t elig = 0;             // bit p: polynomial p may take the offset form
    bool force_offset = false;     // COZK_MSM_DIGIT_FORM=offset
    uint32_t ws = 0;               // which of the two sort workspaces
    uint32_t index = 0;            // position in the tail block's launch order
};
struct MsmTailBlock {
    size_t first = 0, count = 0;   // columns of the caller's arrays
    uint32_t ngroups = 0;
    bool pipelined = false;        // sorts on the side stream, beside the accumulation of the set in front
    std::vector<MsmSetSchedule> sets;  // launch order
};
struct MsmBatchSchedule { std::vector<MsmTailBlock> blocks; };

static inline uint64_t msm_column_refs(const size_t* ns, const int* kinds, size_t p) { return (uint64_t)ns[p] * MSM_KIND_NWIN[kinds[p]]; }

// everything about one launch set that does not depend on its neighbours
static inline MsmSetSchedule msm_set_counts(int nwin, size_t n_bases, const size_t* offsets, const size_t* ns, const int* kinds, size_t first, size_t P) {
    MsmSetSchedule s;
    s.first = first;
    s.P = (uint32_t)P;
    s.table = nwin == 16;
    s.G = s.table ? 1u : 16u;
    s.nb = (uint32_t)P * s.G * NB;
    for (size_t p = first; p < first + P; p++) {
        COZK_REQUIRE(offsets[p] + ns[p] <= n_bases, "msm: base slice out of range");
        const uint64_t m = msm_column_refs(ns, kinds, p);
        s.M += m;
        if (m > s.bound) s.bound = m;
    }
    COZK_REQUIRE(s.M < (1ull << 32), "msm: batch too large (reference count exceeds 32 bits)");
    // segment length of level 0: aim at >= ~2^18 lanes, clamp to [8, 127] (measured: 256-long segments leave
    // too few waves per SIMD and run the gather kernel 14 % slower)
    uint32_t L0 = (uint32_t)(s.M >> 18);
    if (L0 < 8) L0 = 8;
    if (L0 > 127) L0 = 127;  // < SEGKEYS; measured with length-ordered segments: 127 beats 64 by 2 ms per proof (fewer partial sums)
    s.L0 = L0;
    s.maxseg0 = s.M / L0 + s.nb;
    // Fold levels, sized from the plan and not from the data: enough 8-long levels for the buckets of the polynomial
    // with the most references per bucket if its digits are uniform (n nwin / 2^15 with the table, n / 2^15 per window
    // group without; + 25 % and one segment for the Poisson spread: 2^20 field elements give 512 per bucket, 5 segments
    // of <= 127, one level; 2^22 give 2048, 17 segments, two levels; 2^24 three).  Buckets that are fuller than that
    // (flag columns, carry digits, skewed scalars) are left to k_msm_fold_heavy.
    uint64_t per = 0;
    for (size_t p = first; p < first + P; p++) {
        const uint64_t m = ((uint64_t)ns[p] * (s.table ? MSM_KIND_NWIN[kinds[p]] : 1) + NB - 1) / NB;
        if (m > per) per = m;
    }
    uint64_t segs = (per * 5 + 4 * L0 - 1) / (4 * L0) + 1;
    while ((segs = (segs + 7) / 8) > 1) s.fold_levels++;
    // segment counts obey x_{k+1} = x_k / 8 + nb <= max(x_0, 2 nb): both ping-pong buffers of partial sums are sized for that
    s.part_entries = std::max<uint64_t>(s.maxseg0, 2ull * s.nb);
    s.exc_entries = s.maxseg0 + 2;
    s.blk_entries = (s.part_entries + TPB - 1) / TPB + 2;
    return s;
}

// Sort shape and kind runs of a set on a window table.
// 256-thread workgroups (one wave per SIMD, 128 KiB of LDS each): narrow enough to slip into the CU slots that free
// up under the register-heavy gather kernel of the previous launch set, so the sort really runs beside it (wider
// workgroups wait for the gather's grid to drain: measured 127.8 -> 123.5 ms per proof at 2^20, same box).
// A set whose predecessor cannot hide its sort (msm_sort_wide: the first of a batch, a single set, serial batches,
// a set behind a much smaller one) takes the wide shape instead (measured at 2^20: 1024 x 64, 1024 x 32, 1024 x 16,
// 512 x 64 and 512 x 32 all within 0.2 ms of each other): COZK_MSM_LTPB / COZK_MSM_WGS override both shapes.
static inline void msm_set_sort_shape(MsmSetSchedule& s, const size_t* ns, const int* kinds, const MsmOptions& o) {
    s.ltpb = o.ltpb != MSM_BY_SHAPE ? o.ltpb : (s.wide ? MSM_WIDE_LTPB : MSM_NARROW_LTPB);
    s.wgs_max = (uint32_t)(o.wgs != MSM_BY_SHAPE ? o.wgs : (s.wide ? MSM_WIDE_WGS : MSM_NARROW_WGS));
    if (!s.table || s.M == 0) return;  // no LDS sort: nothing takes the shape
    COZK_REQUIRE(s.P <= MSM_SET_POLYS_TABLE, "msm: too many polynomials in one launch set");
    COZK_REQUIRE(s.ltpb >= 64 && s.ltpb <= LTPB && s.ltpb % 64 == 0, "COZK_MSM_LTPB out of range");
    COZK_REQUIRE(s.wgs_max >= 1 && s.wgs_max <= 1024, "COZK_MSM_WGS out of range (1..1024)");
    // one launch per scalar kind, grid = (workgroups per polynomial, polynomials)
    uint32_t nd = 0;
    size_t max_n = 0;
    for (int kind = 0; kind < MSM_KINDS; kind++) {
        MsmKindRun r{kind, nd, {}, 0, 0, 0};
        for (uint32_t p = 0; p < s.P; p++)
            if (kinds[s.first + p] == kind && ns[s.first + p]) {
                r.cols.push_back(p);
                r.max_n = std::max(r.max_n, ns[s.first + p]);
            }
        nd += (uint32_t)r.cols.size();
        max_n = std::max(max_n, r.max_n);
        if (!r.cols.empty()) s.runs.push_back(r);
    }
    for (auto& r : s.runs) {
        r.wgs = msm_sort_wgs(r.kind, r.max_n, o.wg_digits_log2, s.wgs_max);
        r.form_grid = (uint32_t)std::min<uint64_t>(((uint64_t)max_n + 4095) / 4096, 64);
    }
}

// k MSMs with per-polynomial base slices -> the schedule of the whole batch.  Tail blocks of at most MSM_TAIL_GROUPS bucket
// groups; inside a block, launch sets of at most 2^28 .. 2^30 point references (1 GiB of refs) and at most 64 (window table) /
// 4 (16 window groups) polynomials.  `eligible[p]` != 0: column p may take the offset form (msm_column_eligible).
static inline MsmBatchSchedule msm_schedule(int nwin, size_t n_bases, const size_t* offsets, const size_t* ns, const int* kinds, size_t k,
                                            const uint8_t* eligible, const MsmOptions& o) {
    MsmBatchSchedule out;
    if (k == 0) return out;
    COZK_REQUIRE((uint64_t)n_bases * (uint64_t)nwin < (1ull << 31), "msm: table too large for 31-bit refs");
    for (size_t p = 0; p < k; p++) COZK_REQUIRE(kinds[p] >= 0 && kinds[p] < MSM_KINDS, "unknown scalar kind");
    const size_t G = nwin == 16 ? 1 : 16;
    const size_t maxP = nwin == 16 ? MSM_SET_POLYS_TABLE : MSM_SET_POLYS_GROUPS;
    const size_t tail_cap = MSM_TAIL_GROUPS / G;
    for (size_t t0 = 0; t0 < k; t0 += tail_cap) {
        MsmTailBlock b;
        b.first = t0;
        b.count = std::min(k - t0, tail_cap);
        b.ngroups = (uint32_t)(b.count * G);
        // References per launch set: a quarter of the batch, so that the sort of set k + 1 still hides behind the accumulation of set
        // k, within [2^28, 2^30] (the two sort workspaces hold 4 bytes per reference).  Measured: at 2^22 coefficients 2^30 beats 2^28
        // by 7 % of the commit (4 instead of 16 polynomials per set paid the per-set scans and the host's wait for the fullest bucket
        // 4 x as often); at 2^20 one 2^30 set would hold all 64 field-element polynomials and lose the overlap (+4 %).
        uint64_t cap;
        if (o.set_refs_log2) cap = 1ull << std::min(std::max(o.set_refs_log2, MSM_SET_REFS_PIN_MIN), MSM_SET_REFS_PIN_MAX);
        else {
            uint64_t total = 0;
            for (size_t p = t0; p < t0 + b.count; p++) total += msm_column_refs(ns, kinds, p);
            cap = std::min<uint64_t>(std::max<uint64_t>(total / 4, 1ull << MSM_SET_REFS_LOG2_MIN), 1ull << MSM_SET_REFS_LOG2_MAX);
        }
        struct Cut { size_t first, P; uint64_t M; };
        std::vector<Cut> cuts;
        for (size_t s = t0; s < t0 + b.count;) {
            Cut c{s, 0, 0};
            while (s + c.P < t0 + b.count && c.P < maxP) {
                const uint64_t m = msm_column_refs(ns, kinds, s + c.P);
                if (c.P > 0 && c.M + m > cap) break;
                c.M += m;
                c.P++;
            }
            cuts.push_back(c);
            s += c.P;
        }
        // the first set's sort has nothing to hide behind: start with the cheapest one (fewest references)
        if (cuts.size() > 2) {
            auto best = std::min_element(cuts.begin(), cuts.end(), [](const Cut& a, const Cut& c) { return a.M < c.M; });
            std::rotate(cuts.begin(), best, best + 1);
        }
        b.pipelined = !o.serial && cuts.size() > 1;
        for (size_t i = 0; i < cuts.size(); i++) {
            MsmSetSchedule s = msm_set_counts(nwin, n_bases, offsets, ns, kinds, cuts[i].first, cuts[i].P);
            for (uint32_t p = 0; p < s.P; p++)
                if (eligible[s.first + p]) s.elig |= 1ull << p;
            s.force_offset = o.digit_form == MSM_FORM_OFFSET;
            // what the sort runs beside: the accumulation of the set launched before it (none for the first set of a tail
            // block, whose sort waits for everything queued so far, and in a serial batch)
            const uint64_t pred_refs = i > 0 && b.pipelined ? b.sets[i - 1].M : 0;
            s.wide = o.shape_rule ? msm_sort_wide(pred_refs, s.M) : (i == 0 && t0 == 0) || !b.pipelined;
            s.index = (uint32_t)i;
            s.ws = (uint32_t)(i & 1);
            msm_set_sort_shape(s, ns, kinds, o);
            b.sets.push_back(std::move(s));
        }
        out.blocks.push_back(std::move(b));
    }
    return out;
}

// COZK_TRACE_MSM=1: one line per launch set on stderr -- index, polynomials, references, shape, then kind:columns:workgroups
static inline std::string msm_set_trace_line(const MsmSetSchedule& s) {
    std::string line = "cozk msm set " + std::to_string(s.index) + ": polys " + std::to_string(s.P) + " refs " + std::to_string(s.M) + " shape " +
                       (s.wide ? "wide" : "narrow") + " " + std::to_string(s.ltpb) + "x" + std::to_string(s.wgs_max) + " kinds";
    for (const auto& r : s.runs) line += " " + std::string(MSM_KIND_NAME[r.kind]) + ":" + std::to_string(r.cols.size()) + ":" + std::to_string(r.wgs);
    return line;
}
