// GENERATED (see DESIGN.md, 'dual multiplier'): two independent Montgomery products whose column-accumulator
// chains are interleaved instruction by instruction.  Chain 1 carries through VCC, chain 2 through an SGPR pair.
// The accumulators are early-clobber for the reason given in ff_macc.inc.
#define DMACC1_VV(lo1, hi1, lo2, hi2, xa0, ya0, xb0, yb0) { uint64_t c2_; asm("v_mad_u64_u32 %0, vcc, %5, %6, %0\n\tv_mad_u64_u32 %2, %4, %7, %8, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4" : "+&v"(lo1), "+&v"(hi1), "+&v"(lo2), "+&v"(hi2), "=&s"(c2_) : "v"(xa0), "v"(ya0), "v"(xb0), "v"(yb0) : "vcc"); }
#define DMACC2_VV(lo1, hi1, lo2, hi2, xa0, xa1, ya0, ya1, xb0, xb1, yb0, yb1) { uint64_t c2_; asm("v_mad_u64_u32 %0, vcc, %5, %7, %0\n\tv_mad_u64_u32 %2, %4, %9, %11, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %6, %8, %0\n\tv_mad_u64_u32 %2, %4, %10, %12, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4" : "+&v"(lo1), "+&v"(hi1), "+&v"(lo2), "+&v"(hi2), "=&s"(c2_) : "v"(xa0), "v"(xa1), "v"(ya0), "v"(ya1), "v"(xb0), "v"(xb1), "v"(yb0), "v"(yb1) : "vcc"); }
#define DMACC3_VV(lo1, hi1, lo2, hi2, xa0, xa1, xa2, ya0, ya1, ya2, xb0, xb1, xb2, yb0, yb1, yb2) { uint64_t c2_; asm("v_mad_u64_u32 %0, vcc, %5, %8, %0\n\tv_mad_u64_u32 %2, %4, %11, %14, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %6, %9, %0\n\tv_mad_u64_u32 %2, %4, %12, %15, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %7, %10, %0\n\tv_mad_u64_u32 %2, %4, %13, %16, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4" : "+&v"(lo1), "+&v"(hi1), "+&v"(lo2), "+&v"(hi2), "=&s"(c2_) : "v"(xa0), "v"(xa1), "v"(xa2), "v"(ya0), "v"(ya1), "v"(ya2), "v"(xb0), "v"(xb1), "v"(xb2), "v"(yb0), "v"(yb1), "v"(yb2) : "vcc"); }
#define DMACC4_VV(lo1, hi1, lo2, hi2, xa0, xa1, xa2, xa3, ya0, ya1, ya2, ya3, xb0, xb1, xb2, xb3, yb0, yb1, yb2, yb3) { uint64_t c2_; asm("v_mad_u64_u32 %0, vcc, %5, %9, %0\n\tv_mad_u64_u32 %2, %4, %13, %17, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %6, %10, %0\n\tv_mad_u64_u32 %2, %4, %14, %18, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %7, %11, %0\n\tv_mad_u64_u32 %2, %4, %15, %19, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %8, %12, %0\n\tv_mad_u64_u32 %2, %4, %16, %20, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4" : "+&v"(lo1), "+&v"(hi1), "+&v"(lo2), "+&v"(hi2), "=&s"(c2_) : "v"(xa0), "v"(xa1), "v"(xa2), "v"(xa3), "v"(ya0), "v"(ya1), "v"(ya2), "v"(ya3), "v"(xb0), "v"(xb1), "v"(xb2), "v"(xb3), "v"(yb0), "v"(yb1), "v"(yb2), "v"(yb3) : "vcc"); }
#define DMACC1_VS(lo1, hi1, lo2, hi2, xa0, xb0, y0) { uint64_t c2_; asm("v_mad_u64_u32 %0, vcc, %5, %7, %0\n\tv_mad_u64_u32 %2, %4, %6, %7, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4" : "+&v"(lo1), "+&v"(hi1), "+&v"(lo2), "+&v"(hi2), "=&s"(c2_) : "v"(xa0), "v"(xb0), "s"(y0) : "vcc"); }
#define DMACC2_VS(lo1, hi1, lo2, hi2, xa0, xa1, xb0, xb1, y0, y1) { uint64_t c2_; asm("v_mad_u64_u32 %0, vcc, %5, %9, %0\n\tv_mad_u64_u32 %2, %4, %7, %9, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %6, %10, %0\n\tv_mad_u64_u32 %2, %4, %8, %10, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4" : "+&v"(lo1), "+&v"(hi1), "+&v"(lo2), "+&v"(hi2), "=&s"(c2_) : "v"(xa0), "v"(xa1), "v"(xb0), "v"(xb1), "s"(y0), "s"(y1) : "vcc"); }
#define DMACC3_VS(lo1, hi1, lo2, hi2, xa0, xa1, xa2, xb0, xb1, xb2, y0, y1, y2) { uint64_t c2_; asm("v_mad_u64_u32 %0, vcc, %5, %11, %0\n\tv_mad_u64_u32 %2, %4, %8, %11, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %6, %12, %0\n\tv_mad_u64_u32 %2, %4, %9, %12, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %7, %13, %0\n\tv_mad_u64_u32 %2, %4, %10, %13, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4" : "+&v"(lo1), "+&v"(hi1), "+&v"(lo2), "+&v"(hi2), "=&s"(c2_) : "v"(xa0), "v"(xa1), "v"(xa2), "v"(xb0), "v"(xb1), "v"(xb2), "s"(y0), "s"(y1), "s"(y2) : "vcc"); }
#define DMACC4_VS(lo1, hi1, lo2, hi2, xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3, y0, y1, y2, y3) { uint64_t c2_; asm("v_mad_u64_u32 %0, vcc, %5, %13, %0\n\tv_mad_u64_u32 %2, %4, %9, %13, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %6, %14, %0\n\tv_mad_u64_u32 %2, %4, %10, %14, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %7, %15, %0\n\tv_mad_u64_u32 %2, %4, %11, %15, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4\n\tv_mad_u64_u32 %0, vcc, %8, %16, %0\n\tv_mad_u64_u32 %2, %4, %12, %16, %2\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\tv_addc_co_u32_e64 %3, %4, 0, %3, %4" : "+&v"(lo1), "+&v"(hi1), "+&v"(lo2), "+&v"(hi2), "=&s"(c2_) : "v"(xa0), "v"(xa1), "v"(xa2), "v"(xa3), "v"(xb0), "v"(xb1), "v"(xb2), "v"(xb3), "s"(y0), "s"(y1), "s"(y2), "s"(y3) : "vcc"); }
#define FF_MUL2_BODY \
        DMACC1_VV(lo1, hi1, lo2, hi2, A[0], B[0], C[0], D[0]); \
        m1[0] = (uint32_t)lo1 * Pm::INV; m2[0] = (uint32_t)lo2 * Pm::INV; \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[0], m2[0], Pm::MOD[0]); \
        lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC2_VV(lo1, hi1, lo2, hi2, A[0], A[1], B[1], B[0], C[0], C[1], D[1], D[0]); \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[0], m2[0], Pm::MOD[1]); \
        m1[1] = (uint32_t)lo1 * Pm::INV; m2[1] = (uint32_t)lo2 * Pm::INV; \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[1], m2[1], Pm::MOD[0]); \
        lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC3_VV(lo1, hi1, lo2, hi2, A[0], A[1], A[2], B[2], B[1], B[0], C[0], C[1], C[2], D[2], D[1], D[0]); \
        DMACC2_VS(lo1, hi1, lo2, hi2, m1[0], m1[1], m2[0], m2[1], Pm::MOD[2], Pm::MOD[1]); \
        m1[2] = (uint32_t)lo1 * Pm::INV; m2[2] = (uint32_t)lo2 * Pm::INV; \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[2], m2[2], Pm::MOD[0]); \
        lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[0], A[1], A[2], A[3], B[3], B[2], B[1], B[0], C[0], C[1], C[2], C[3], D[3], D[2], D[1], D[0]); \
        DMACC3_VS(lo1, hi1, lo2, hi2, m1[0], m1[1], m1[2], m2[0], m2[1], m2[2], Pm::MOD[3], Pm::MOD[2], Pm::MOD[1]); \
        m1[3] = (uint32_t)lo1 * Pm::INV; m2[3] = (uint32_t)lo2 * Pm::INV; \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[3], m2[3], Pm::MOD[0]); \
        lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[0], A[1], A[2], A[3], B[4], B[3], B[2], B[1], C[0], C[1], C[2], C[3], D[4], D[3], D[2], D[1]); \
        DMACC1_VV(lo1, hi1, lo2, hi2, A[4], B[0], C[4], D[0]); \
        DMACC4_VS(lo1, hi1, lo2, hi2, m1[0], m1[1], m1[2], m1[3], m2[0], m2[1], m2[2], m2[3], Pm::MOD[4], Pm::MOD[3], Pm::MOD[2], Pm::MOD[1]); \
        m1[4] = (uint32_t)lo1 * Pm::INV; m2[4] = (uint32_t)lo2 * Pm::INV; \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[4], m2[4], Pm::MOD[0]); \
        lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[0], A[1], A[2], A[3], B[5], B[4], B[3], B[2], C[0], C[1], C[2], C[3], D[5], D[4], D[3], D[2]); \
        DMACC2_VV(lo1, hi1, lo2, hi2, A[4], A[5], B[1], B[0], C[4], C[5], D[1], D[0]); \
        DMACC4_VS(lo1, hi1, lo2, hi2, m1[0], m1[1], m1[2], m1[3], m2[0], m2[1], m2[2], m2[3], Pm::MOD[5], Pm::MOD[4], Pm::MOD[3], Pm::MOD[2]); \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[4], m2[4], Pm::MOD[1]); \
        m1[5] = (uint32_t)lo1 * Pm::INV; m2[5] = (uint32_t)lo2 * Pm::INV; \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[5], m2[5], Pm::MOD[0]); \
        lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[0], A[1], A[2], A[3], B[6], B[5], B[4], B[3], C[0], C[1], C[2], C[3], D[6], D[5], D[4], D[3]); \
        DMACC3_VV(lo1, hi1, lo2, hi2, A[4], A[5], A[6], B[2], B[1], B[0], C[4], C[5], C[6], D[2], D[1], D[0]); \
        DMACC4_VS(lo1, hi1, lo2, hi2, m1[0], m1[1], m1[2], m1[3], m2[0], m2[1], m2[2], m2[3], Pm::MOD[6], Pm::MOD[5], Pm::MOD[4], Pm::MOD[3]); \
        DMACC2_VS(lo1, hi1, lo2, hi2, m1[4], m1[5], m2[4], m2[5], Pm::MOD[2], Pm::MOD[1]); \
        m1[6] = (uint32_t)lo1 * Pm::INV; m2[6] = (uint32_t)lo2 * Pm::INV; \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[6], m2[6], Pm::MOD[0]); \
        lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[0], A[1], A[2], A[3], B[7], B[6], B[5], B[4], C[0], C[1], C[2], C[3], D[7], D[6], D[5], D[4]); \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[4], A[5], A[6], A[7], B[3], B[2], B[1], B[0], C[4], C[5], C[6], C[7], D[3], D[2], D[1], D[0]); \
        DMACC4_VS(lo1, hi1, lo2, hi2, m1[0], m1[1], m1[2], m1[3], m2[0], m2[1], m2[2], m2[3], Pm::MOD[7], Pm::MOD[6], Pm::MOD[5], Pm::MOD[4]); \
        DMACC3_VS(lo1, hi1, lo2, hi2, m1[4], m1[5], m1[6], m2[4], m2[5], m2[6], Pm::MOD[3], Pm::MOD[2], Pm::MOD[1]); \
        m1[7] = (uint32_t)lo1 * Pm::INV; m2[7] = (uint32_t)lo2 * Pm::INV; \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[7], m2[7], Pm::MOD[0]); \
        lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[1], A[2], A[3], A[4], B[7], B[6], B[5], B[4], C[1], C[2], C[3], C[4], D[7], D[6], D[5], D[4]); \
        DMACC3_VV(lo1, hi1, lo2, hi2, A[5], A[6], A[7], B[3], B[2], B[1], C[5], C[6], C[7], D[3], D[2], D[1]); \
        DMACC4_VS(lo1, hi1, lo2, hi2, m1[1], m1[2], m1[3], m1[4], m2[1], m2[2], m2[3], m2[4], Pm::MOD[7], Pm::MOD[6], Pm::MOD[5], Pm::MOD[4]); \
        DMACC3_VS(lo1, hi1, lo2, hi2, m1[5], m1[6], m1[7], m2[5], m2[6], m2[7], Pm::MOD[3], Pm::MOD[2], Pm::MOD[1]); \
        r1[0] = (uint32_t)lo1; r2[0] = (uint32_t)lo2; lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[2], A[3], A[4], A[5], B[7], B[6], B[5], B[4], C[2], C[3], C[4], C[5], D[7], D[6], D[5], D[4]); \
        DMACC2_VV(lo1, hi1, lo2, hi2, A[6], A[7], B[3], B[2], C[6], C[7], D[3], D[2]); \
        DMACC4_VS(lo1, hi1, lo2, hi2, m1[2], m1[3], m1[4], m1[5], m2[2], m2[3], m2[4], m2[5], Pm::MOD[7], Pm::MOD[6], Pm::MOD[5], Pm::MOD[4]); \
        DMACC2_VS(lo1, hi1, lo2, hi2, m1[6], m1[7], m2[6], m2[7], Pm::MOD[3], Pm::MOD[2]); \
        r1[1] = (uint32_t)lo1; r2[1] = (uint32_t)lo2; lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[3], A[4], A[5], A[6], B[7], B[6], B[5], B[4], C[3], C[4], C[5], C[6], D[7], D[6], D[5], D[4]); \
        DMACC1_VV(lo1, hi1, lo2, hi2, A[7], B[3], C[7], D[3]); \
        DMACC4_VS(lo1, hi1, lo2, hi2, m1[3], m1[4], m1[5], m1[6], m2[3], m2[4], m2[5], m2[6], Pm::MOD[7], Pm::MOD[6], Pm::MOD[5], Pm::MOD[4]); \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[7], m2[7], Pm::MOD[3]); \
        r1[2] = (uint32_t)lo1; r2[2] = (uint32_t)lo2; lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC4_VV(lo1, hi1, lo2, hi2, A[4], A[5], A[6], A[7], B[7], B[6], B[5], B[4], C[4], C[5], C[6], C[7], D[7], D[6], D[5], D[4]); \
        DMACC4_VS(lo1, hi1, lo2, hi2, m1[4], m1[5], m1[6], m1[7], m2[4], m2[5], m2[6], m2[7], Pm::MOD[7], Pm::MOD[6], Pm::MOD[5], Pm::MOD[4]); \
        r1[3] = (uint32_t)lo1; r2[3] = (uint32_t)lo2; lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC3_VV(lo1, hi1, lo2, hi2, A[5], A[6], A[7], B[7], B[6], B[5], C[5], C[6], C[7], D[7], D[6], D[5]); \
        DMACC3_VS(lo1, hi1, lo2, hi2, m1[5], m1[6], m1[7], m2[5], m2[6], m2[7], Pm::MOD[7], Pm::MOD[6], Pm::MOD[5]); \
        r1[4] = (uint32_t)lo1; r2[4] = (uint32_t)lo2; lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC2_VV(lo1, hi1, lo2, hi2, A[6], A[7], B[7], B[6], C[6], C[7], D[7], D[6]); \
        DMACC2_VS(lo1, hi1, lo2, hi2, m1[6], m1[7], m2[6], m2[7], Pm::MOD[7], Pm::MOD[6]); \
        r1[5] = (uint32_t)lo1; r2[5] = (uint32_t)lo2; lo1 = (lo1 >> 32) | ((uint64_t)hi1 << 32); hi1 = 0; lo2 = (lo2 >> 32) | ((uint64_t)hi2 << 32); hi2 = 0; \
        DMACC1_VV(lo1, hi1, lo2, hi2, A[7], B[7], C[7], D[7]); \
        DMACC1_VS(lo1, hi1, lo2, hi2, m1[7], m2[7], Pm::MOD[7]); \
        r1[6] = (uint32_t)lo1; r1[7] = (uint32_t)(lo1 >> 32); r2[6] = (uint32_t)lo2; r2[7] = (uint32_t)(lo2 >> 32);
