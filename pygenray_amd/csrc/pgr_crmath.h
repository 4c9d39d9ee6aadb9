// pgr_crmath.h -- correctly rounded pow(x, -+0.2), asin and sin for the ray-fan kernel.
//
// pygenray's integrator calls exactly three libm functions (through NumPy / SciPy):
//   error_norm ** -0.2 and (0.01 / d) ** 0.2   SCIPY/rk.py:156,162 ; SCIPY/common.py:131
//   arcsin(p c)                                REF/integration_processes.py:333 (ray_angle)
//   sin(radians(theta_b))                      REF/launch_rays.py:480 (reflection law)
// Everything else on the path is +, -, *, /, sqrt, fixed by IEEE 754.  libm results are faithful
// but not correctly rounded, so the reference is only reproducible to "whichever libm NumPy was
// linked against"; glibc 2.35's pow / asin / sin differ from the correctly rounded value in
// 0.09 / 0.21 / 0.14 % of calls -- and ONE differing ulp moves a 1000 km ray by millimetres
// (the adaptive controller is chaotic at the last bit).  The functions here
// return the CORRECTLY ROUNDED results: the platform-independent value every libm approximates
// and the one the CPU oracle computes in its ORC_MATH_CR mode (binary128 via libquadmath,
// oracle/ray_oracle.c), so the HIP path and the oracle agree bit for bit.
//
// Method: a double-precision approximation, then ONE correction computed in double-double
// arithmetic (error-free products by fma) to ~2^-100 relative, and a single final rounding
// (an fma or an add of the approximation and its correction).  asin, sin: correctly rounded
// unless the exact value lies within ~2^-98 relative of a rounding boundary (1e-13 per call).
// The two powers are evaluated Ziv-style (round 4): the fast evaluation prices the 5.6e-17 excess of
// the double 0.2 over 1/5 with an fp32 logarithm and is good to 2^-74; it is followed by a
// ROUNDING TEST -- the exact residual (approximation + correction) - result against half an ulp
// less 2^-71 -- and an argument that fails it (3e-6 of the calls) is evaluated again with the
// logarithm in double precision and a rounding-limited root, good to ~2^-100 (pgr_cr_pow_*_slow).
// tests/test_crmath.py checks the host build of this file against libquadmath on 1e7 random
// arguments per function, on every argument that fails the rounding test in 4e8 draws and on the
// hard cases of tests/golden/g14_pow_hard_cases.npz (exact value within 2^-80 of a midpoint,
// scripts/gen/gen_pow_hard_cases.py); tests/test_hip_parity.py the device build against the same.
//
// The text is plain C99 / C++: `PGR_CR_HOST` selects the host twin (tests only -- the product
// has no CPU path), otherwise it is device code.  Build with -ffp-contract=off.
#ifndef PGR_CRMATH_H
#define PGR_CRMATH_H

#ifdef PGR_CR_HOST
#include <math.h>
#define PGR_CR_FN static inline
#define PGR_CR_RARE(c) (__builtin_expect((c), 0))
#define PGR_CR_TABLE(type, name, n) static const type name[n]
static inline float pgr_cr_seed_log2f(float x) { return log2f(x); }
static inline float pgr_cr_seed_exp2f(float x) { return exp2f(x); }
static inline double pgr_cr_seed_asin(double x) { return asin(x); }
static inline double pgr_cr_fallback_sin(double x) { return sin(x); }
static inline double pgr_cr_fallback_pow(double x, double y) { return pow(x, y); }
#else
#define PGR_CR_FN __device__ __forceinline__
// (a rare per-lane condition as ONE wave-uniform branch to an out-of-line block: the common path falls through)
#define PGR_CR_RARE(c) (__builtin_expect(__builtin_amdgcn_ballot_w64(c) != 0ull, 0))
#define PGR_CR_TABLE(type, name, n) __device__ const type name[n]
__device__ __forceinline__ float pgr_cr_seed_log2f(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float pgr_cr_seed_exp2f(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ double pgr_cr_seed_asin(double x) { return asin(x); }
__device__ __forceinline__ double pgr_cr_fallback_sin(double x) { return sin(x); }
__device__ __forceinline__ double pgr_cr_fallback_pow(double x, double y) { return pow(x, y); }
#endif

// ---- selects of the event locator's replayed halvings (pgr_fan_kernel.h) that do not go through the condition register ----
// all ones where d has its sign bit set, zero elsewhere: one arithmetic shift of the sign word.  d = a - b of finite doubles
// is negative exactly when a < b, and a == b gives +0 -- except (-0) - (+0) = -0: the halvings' operands all lie in the
// step [t, t_new], which holds no zero where halvings are taken (t > 0 or t_new < 0) ...
PGR_CR_FN int pgr_sign_mask(double d)
{
    union { double d; unsigned long long u; } v;
    v.d = d;
    return (int)(v.u >> 32) >> 31;
}
// ... and a where the mask is all ones, b where it is zero (one v_bfi_b32 per half on the device)
PGR_CR_FN double pgr_mask_select(int m, double a, double b)
{
    union { double d; unsigned long long u; } va, vb;
    const unsigned long long mm = ((unsigned long long)(unsigned)m << 32) | (unsigned)m;
    va.d = a; vb.d = b;
    va.u = (va.u & mm) | (vb.u & ~mm);
    return va.d;
}

// ---- decisions of a step attempt's tail (pgr_fan_kernel.h) that do not go through the condition register ----
// all ones where a < b, zero elsewhere, for EVERY double a -- NaN, +-inf, zeros of both signs, subnormals -- given a finite
// constant b != 0 and a finite `above` > b.  fmin drops a NaN (NaN < b is false: `above` - b > 0 says so) and caps +inf; the
// difference of two doubles is zero only where they are equal (gradual underflow) and then +0 (b is not a zero, so the
// (-0) - (+0) of pgr_sign_mask cannot occur); everywhere else it has the sign of a - b, overflow to -inf included.
PGR_CR_FN int pgr_mask_lt_const(double a, double b, double above)
{
    return pgr_sign_mask(__builtin_fmin(a, above) - b);
}
// all ones where d >= 0, for d = t - t_bound of a committed step: t <= t_bound (the attempt clamps t_new), neither is NaN
// (a NaN step is never accepted), so d <= 0 and "d >= 0" is "d is a zero".  Equal operands give +0; the one -0,
// (-0) - (+0), would need t = -0, which a sum t + h with h > 0 never is and the clamp only copies from t_bound.
PGR_CR_FN int pgr_mask_reached(double d)
{
    return ~pgr_sign_mask(d);
}
// RK45's step factor, SCIPY/rk.py:148-165, from pw = SAFETY * err ** -0.2 (NaN where the power is not a number):
//   accepted:  min(MAX_FACTOR, pw), and min(1, that) behind a rejected attempt  ==  fmin(pw, limit), limit = 1 or MAX_FACTOR
//   rejected:  max(MIN_FACTOR, pw)                                              ==  fmax(pw, MIN_FACTOR)
// fmin / fmax return the other operand for a NaN: MAX_FACTOR (1 behind a rejection) and MIN_FACTOR, what the compare forms
// `pw < MAX_FACTOR ? pw : MAX_FACTOR` and `pw > MIN_FACTOR ? pw : MIN_FACTOR` give.  The limit depends on the attempt
// BEFORE this one only: it is formed ahead of the stages, off the chain error norm -> power -> factor -> h_abs.
PGR_CR_FN double pgr_factor_limit(int m_prev_rejected, double max_factor)
{
    return pgr_mask_select(m_prev_rejected, 1.0, max_factor);
}
PGR_CR_FN double pgr_step_factor(int m_accepted, double pw, double limit, double min_factor)
{
    return pgr_mask_select(m_accepted, __builtin_fmin(pw, limit), __builtin_fmax(pw, min_factor));
}
// a lane's wait bits -- PGR_WAIT_PARKED: its step fired an event and waits for the service, PGR_WAIT_INIT: it (re)starts --
// where the lane is still running, zero elsewhere: RUNNING (-1) is the only negative status, so the sign word of the status
// is the mask.  One integer in a vector register per lane instead of three lane masks in scalar pairs: the gate's "anybody
// parked" is one compare of this word with zero.
#define PGR_WAIT_PARKED 1
#define PGR_WAIT_INIT 2
PGR_CR_FN int pgr_lane_pending(int status, int wait)
{
    return wait & (status >> 31);
}

// ---- generated by scripts/gen/gen_crmath_tables.py (mpmath, 400 bits) ----
// sin(j/32), cos(j/32), j = 0..28, as double-double {hi, lo}
PGR_CR_TABLE(double, pgr_cr_sincos_tab, 29 * 4) = {
    0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p+0, 0x0.0p+0,
    0x1.ffeaaaeeee86fp-6, -0x1.cd406fb224ae2p-60, 0x1.ffc00155527d3p-1, -0x1.3b54492d89b5bp-55,
    0x1.ffaaaeeed4edbp-5, -0x1.2d16d32684b69p-59, 0x1.ff0015549f4d3p-1, 0x1.328387b99426fp-55,
    0x1.7f701032550e4p-4, 0x1.afc2d1800501ap-60, 0x1.fdc06bf7e6b9bp-1, 0x1.31902b535f8dbp-55,
    0x1.feaaeee86ee36p-4, -0x1.afcb2bcc6f03bp-59, 0x1.fc015527d5bd3p-1, 0x1.b68f35094efb8p-55,
    0x1.3eb312c5d66cbp-3, 0x1.47d666b66cb91p-57, 0x1.f9c340a7cc428p-1, 0x1.c5b6b063b7462p-55,
    0x1.7dc102fbaf2b5p-3, 0x1.5ab50e23c97c3p-59, 0x1.f706bdf9ece1cp-1, -0x1.698c80c36dcb4p-55,
    0x1.bc6f84edc6199p-3, 0x1.9c1a56a7b0cabp-57, 0x1.f3cc7c3b3d16ep-1, -0x1.21a3ad28a3494p-57,
    0x1.faaeed4f31577p-3, -0x1.15d88508e32b8p-57, 0x1.f01549f7deea1p-1, 0x1.d3c1e99e5cafdp-55,
    0x1.1c37d64c6b876p-2, 0x1.46076fe0dcff4p-56, 0x1.ebe214f76efa8p-1, -0x1.02f9f12ba543ep-55,
    0x1.3ad129769d3d8p-2, 0x1.03d550487839ap-63, 0x1.e733ea0193d40p-1, -0x1.6428b3546ce13p-55,
    0x1.591bc9fa2f597p-2, 0x1.7c74bac3fe0cbp-57, 0x1.e20bf49acd6c1p-1, -0x1.660aec7ef636bp-58,
    0x1.7710255764214p-2, -0x1.6ead7314bb6cep-57, 0x1.dc6b7eb995912p-1, 0x1.4b364776dcd35p-58,
    0x1.94a6be9f546c5p-2, -0x1.69ce13e683f58p-56, 0x1.d653f073e4040p-1, -0x1.76236434bec37p-55,
    0x1.b1d8305321617p-2, -0x1.ae242cb99f519p-56, 0x1.cfc6cfa52ad9fp-1, 0x1.8b5b5508f2a0dp-55,
    0x1.ce9d2e3d4a51fp-2, -0x1.2fc8a12dae298p-57, 0x1.c8c5bf8ce1a84p-1, 0x1.ab3d1a1590123p-56,
    0x1.eaee8744b05f0p-2, -0x1.789b43c9b027dp-58, 0x1.c1528065b7d50p-1, -0x1.892111312e828p-55,
    0x1.0362939c69955p-1, -0x1.2d8cd78397b01p-55, 0x1.b96eeef58840ep-1, 0x1.45a3cc78fade0p-58,
    0x1.110d0c4b69c3bp-1, 0x1.d918998809981p-55, 0x1.b11d04162a4c6p-1, 0x1.1dd561efbc0c2p-56,
    0x1.1e7343236574cp-1, 0x1.22a3fa4f41d5ap-56, 0x1.a85ed4373e02dp-1, 0x1.9be06385ec792p-57,
    0x1.2b91dea88421ep-1, -0x1.fa371db216ab0p-55, 0x1.9f368ed912f85p-1, -0x1.1d200c5791606p-55,
    0x1.386597456282bp-1, -0x1.10fada93b07a8p-56, 0x1.95a67e00cb1fdp-1, -0x1.0befda21f862dp-55,
    0x1.44eb381cf386bp-1, -0x1.3ed6c1e6a5505p-55, 0x1.8bb105a5dc900p-1, 0x1.863e03e9474c1p-55,
    0x1.511f9fd7b351cp-1, -0x1.5c0e861c48831p-55, 0x1.8158a31916d5dp-1, -0x1.de8b90b8228dep-57,
    0x1.5cffc16bf8f0dp-1, 0x1.96cb370eb578ap-55, 0x1.769fec655211fp-1, -0x1.827d5cf8c68c5p-57,
    0x1.6888a4e134b2fp-1, -0x1.6b7d37644d5e6p-55, 0x1.6b898fa9efb5dp-1, 0x1.15ac786ccf4b2p-56,
    0x1.73b7680dea578p-1, -0x1.2248306dc12a2p-56, 0x1.6018526f563dfp-1, 0x1.46ca5e0e432d0p-55,
    0x1.7e893f5037959p-1, 0x1.0eefbaa650c4cp-55, 0x1.544f10f592ca5p-1, -0x1.e7ae8e6c7a62fp-55,
    0x1.88fb7640b8da2p-1, -0x1.49987c11efaa3p-55, 0x1.4830bd7d4ceb3p-1, 0x1.df77ff20d5448p-55,
};
#define PGR_CR_PIO2_H 0x1.921fb54442d18p+0
#define PGR_CR_PIO2_L 0x1.1a62633145c07p-54
#define PGR_CR_PIO2_1 0x1.921fb54400000p+0
#define PGR_CR_PIO2_2 0x1.0b4611a626331p-34
#define PGR_CR_PIO2_3 0x1.1701b839a2520p-88
#define PGR_CR_2OPI 0x1.45f306dc9c883p-1
#define PGR_CR_S3_H -0x1.5555555555555p-3
#define PGR_CR_S3_L -0x1.5555555555555p-57
#define PGR_CR_S5_H 0x1.1111111111111p-7
#define PGR_CR_S5_L 0x1.1111111111111p-63
#define PGR_CR_S7_H -0x1.a01a01a01a01ap-13
#define PGR_CR_S7_L -0x1.a01a01a01a01ap-73
#define PGR_CR_C4_H 0x1.5555555555555p-5
#define PGR_CR_C4_L 0x1.5555555555555p-59
#define PGR_CR_C6_H -0x1.6c16c16c16c17p-10
#define PGR_CR_C6_L 0x1.f49f49f49f49fp-65
#define PGR_CR_S9 0x1.71de3a556c734p-19
#define PGR_CR_S11 -0x1.ae64567f544e4p-26
#define PGR_CR_C8 0x1.a01a01a01a01ap-16
#define PGR_CR_C10 -0x1.27e4fb7789f5cp-22
#define PGR_CR_C12 0x1.1eed8eff8d898p-29
// 0.2 (double) = (1/5)(1 + kappa), kappa = 5.5511151231257827021e-17
#define PGR_CR_POW_KLN2 -0x1.1be9bff2e94bfp-57   /* -(kappa/5) ln 2: x**-0.2 = x^(-1/5) (1 + this * log2 x) */
// ---- end of generated constants ----

// ------------------------------------------------------------------------------------
// x ** -0.2 for the step-size controller (SCIPY/rk.py:156,162), x = error_norm in [1e-7, 1e4]:
// the one correctly rounded function on the hot path (31 VALU instructions, 14 more than a
// 2-ulp Newton iteration).
//   y  = x^(-1/5) by Newton on y^-5 = x from an fp32 seed (ONE step: good to ~2^-41; round 3 -- two steps,
//        rounding-limited, until then; A/B lone steepest wave 5.005 -> 4.982 ms, same bits)
//   rho = 1 - x y^5 evaluated error-free (three products by fma), so x^(-1/5) = y (1 + rho/5 - 2 rho^2/25 + O(rho^3))
//   the exponent is the DOUBLE -0.2 = -(1/5)(1 + 5.55e-17): x**-0.2 = x^(-1/5) (1 + KLN2 log2 x)
//   result = fma(y, rho/5 + KLN2 log2 x, y): one rounding of a value good to ~2^-77
// ------------------------------------------------------------------------------------
// one Newton step on y^-5 = x:  y <- y + y (1 - x y^5) / 5
PGR_CR_FN double pgr_cr_newton5(double x, double y, const double fifth)
{
    const double y2 = y * y, y4 = y2 * y2, y5 = y4 * y;
    const double e = __builtin_fma(-x, y5, 1.0);
    return __builtin_fma(y * fifth, e, y);
}
// log2(x) to ~2^-50 absolute for the slow paths (x > 0, finite, normal): x = 2^E m, m in [1/sqrt2, sqrt2),
// ln m = 2 atanh(z), z = (m - 1)/(m + 1), |z| <= 0.1716: the odd series to z^19 (next term 2^-53)
PGR_CR_FN double pgr_cr_log2_slow(double x)
{
    union { double d; unsigned long long u; } v;
    v.d = x;
    int E = (int)((v.u >> 52) & 0x7ff) - 1023;
    v.u = (v.u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;          // m in [1, 2)
    double m = v.d;
    if (m > 0x1.6a09e667f3bcdp+0) { m *= 0.5; E += 1; }                    // m in [1/sqrt2, sqrt2)
    const double z = (m - 1.0) / (m + 1.0), w = z * z;
    double p = 1.0 / 19.0;
    p = __builtin_fma(p, w, 1.0 / 17.0); p = __builtin_fma(p, w, 1.0 / 15.0); p = __builtin_fma(p, w, 1.0 / 13.0);
    p = __builtin_fma(p, w, 1.0 / 11.0); p = __builtin_fma(p, w, 1.0 / 9.0); p = __builtin_fma(p, w, 1.0 / 7.0);
    p = __builtin_fma(p, w, 1.0 / 5.0); p = __builtin_fma(p, w, 1.0 / 3.0); p = __builtin_fma(p, w, 1.0);
    return __builtin_fma(2.0 * z * p, 0x1.71547652b82fep+0, (double)E);    // 2 atanh(z) / ln 2 + E
}
// The rounding test (Ziv): `r` is the rounding of a value known to |err| <= 2^-72 r, `res` its exact residual (value
// as evaluated - r, below half an ulp).  The rounding is certain unless |res| comes within 2^-71 2^e of half an ulp of r
// (2^e <= r < 2^(e+1): half an ulp is 2^(e-53), and 2^-72 r < 2^-71 2^e).
// (r = 2^e itself: the doubles BELOW it are half as far apart and this test would not see a value just short of that
// boundary.  Such results belong to x = 32^-e (1 + k ulp), |k| <= 3, where the power is linear in k to 2^-100 -- the
// residues are multiples of 0.2 or 0.4 ulp, never near 0.5 -- and tests/test_crmath.py::test_hard_neighbourhoods
// enumerates those arguments on both sides of every 32^n in range.)
#define PGR_CR_ZIV_K 0x1.ffff8p-55   /* (2^-53 - 2^-71) / 2: frexp's exponent is e + 1 */
PGR_CR_FN int pgr_cr_rounding_uncertain(double res, double r)
{
#ifdef PGR_CR_HOST
    int e;
    (void)frexp(r, &e);
    const double thr = ldexp(PGR_CR_ZIV_K, e);
#else
    const double thr = __builtin_ldexp(PGR_CR_ZIV_K, __builtin_amdgcn_frexp_exp(r));   // v_frexp_exp_i32_f64, v_ldexp_f64
#endif
    return __builtin_fabs(res) > thr;
}
// the second level: one more Newton step (y is then the rounding-limited root, rho ~ 2^-52 and its square is
// nothing), the same error-free residual, the logarithm in double precision: good to ~2^-100
PGR_CR_FN double pgr_cr_pow_m02_slow(double x, double y, const double fifth, const double kln2)
{
    y = pgr_cr_newton5(x, y, fifth);
    const double ah = y * y, al = __builtin_fma(y, y, -ah);
    const double bh = ah * ah, bl = __builtin_fma(ah, al + al, __builtin_fma(ah, ah, -bh));
    const double ch = bh * y, cl = __builtin_fma(bl, y, __builtin_fma(bh, y, -ch));
    const double dh = ch * x, dl = __builtin_fma(cl, x, __builtin_fma(ch, x, -dh));
    const double rho = (1.0 - dh) - dl;
    const double u = __builtin_fma(pgr_cr_log2_slow(x), kln2, rho * fifth);
    return __builtin_fma(y, u, y);
}
// (fifth = 0.2 and kln2 = PGR_CR_POW_KLN2 as arguments: a caller for whom every fp64 literal costs two scalar
// moves per use keeps them in registers)
PGR_CR_FN double pgr_cr_pow_m02_k(double x, const double fifth, const double kln2)
{
    const float lf = pgr_cr_seed_log2f((float)x);
    double y = (double)pgr_cr_seed_exp2f(-0.2f * lf);
    // ONE Newton step: the fp32 seed is good to ~2^-21, the step leaves ~3 * 2^-42, i.e. rho = 1 - x y^5 ~ 2^-39;
    // x^(-1/5) = y (1 + rho)^(1/5) = y (1 + rho/5 - 2 rho^2/25 + O(rho^3)): the second-order term (2^-81) is carried
    // below, the third-order one (2^-120) is not needed
    y = pgr_cr_newton5(x, y, fifth);
    const double ah = y * y, al = __builtin_fma(y, y, -ah);                                // y^2
    const double bh = ah * ah, bl = __builtin_fma(ah, al + al, __builtin_fma(ah, ah, -bh));  // y^4
    const double ch = bh * y, cl = __builtin_fma(bl, y, __builtin_fma(bh, y, -ch));          // y^5
    const double dh = ch * x, dl = __builtin_fma(cl, x, __builtin_fma(ch, x, -dh));          // x y^5
    const double rho = (1.0 - dh) - dl;
    const double r5 = rho * fifth;                                                          // rho/5 - 2 (rho/5)^2
    const double u = __builtin_fma((double)lf, kln2, __builtin_fma(-2.0 * r5, r5, r5));
    double r = __builtin_fma(y, u, y);
#ifndef PGR_POW_NO_ZIV
    // the fp32 logarithm leaves y (1 + u) good to 2^-74 only (|log2 x| < 128: an ulp of lf is <= 2^-17, times |kln2| =
    // 2^-56.85; the controller's min / max decide everything outside 6e-6 < x < 2e3 anyway): rounding test on the exact
    // residual y + y u - r = fma(y, u, -(r - y))  (r - y is exact: r and y differ by 2^-39 y)
    if (PGR_CR_RARE(pgr_cr_rounding_uncertain(__builtin_fma(y, u, -(r - y)), r)))
        r = pgr_cr_pow_m02_slow(x, y, fifth, kln2);
#endif
    return r;
}
PGR_CR_FN double pgr_cr_pow_m02(double x) { return pgr_cr_pow_m02_k(x, 0.2, PGR_CR_POW_KLN2); }

// x ** 0.2 for select_initial_step (SCIPY/common.py:131), x = 0.01 / max(d1, d2) > 0: through
// w = x^(-1/5) as above and x^(1/5) = x w^4 in double-double; `lg` = log2 x (fp32 in the fast evaluation)
PGR_CR_FN double pgr_cr_pow_p02_eval(double x, double w, double lg, double* approx, double* corr)
{
    const double ah = w * w, al = __builtin_fma(w, w, -ah);
    const double bh = ah * ah, bl = __builtin_fma(ah, al + al, __builtin_fma(ah, ah, -bh));
    const double ch = bh * w, cl = __builtin_fma(bl, w, __builtin_fma(bh, w, -ch));
    const double dh = ch * x, dl = __builtin_fma(cl, x, __builtin_fma(ch, x, -dh));
    const double rho = (1.0 - dh) - dl;                  // x^(-1/5) = w (1 + rho/5)
    const double rh = bh * x, rl = __builtin_fma(bl, x, __builtin_fma(bh, x, -rh));  // x w^4
    // x^(1/5) = x w^4 (1 + rho/5)^4 ; x**0.2 = x^(1/5) (1 - KLN2 log2 x)
    const double u = __builtin_fma(-lg, PGR_CR_POW_KLN2, rho * 0.8);
    *approx = rh;
    *corr = __builtin_fma(rh, u, rl);
    return rh + *corr;
}
PGR_CR_FN double pgr_cr_pow_p02(double x)
{
    // (the fp32 logarithm prices the exponent's excess to 2^-74 only while |log2 x| < 64; on this path
    // 1e-15 < max(d1, d2), so x < 1e13; anything else takes the plain library pow)
    if (!(x > 0x1.0p-60 && x < 0x1.0p+60)) return pgr_cr_fallback_pow(x, 0.2);
    const float lf = pgr_cr_seed_log2f((float)x);
    double w = (double)pgr_cr_seed_exp2f(-0.2f * lf);
    w = pgr_cr_newton5(x, pgr_cr_newton5(x, w, 0.2), 0.2);
    double approx, corr;
    double r = pgr_cr_pow_p02_eval(x, w, (double)lf, &approx, &corr);
#ifndef PGR_POW_NO_ZIV
    // (|lf| < 64 here: the fast evaluation is good to 2^-22 x 64 x 2^-57 = 2^-73; the same rounding test, then the
    // logarithm in double precision -- w is rounding limited already)
    if (PGR_CR_RARE(pgr_cr_rounding_uncertain((approx - r) + corr, r)))      // (approx - r is exact, the sum cancels to below half an ulp)
        r = pgr_cr_pow_p02_eval(x, w, pgr_cr_log2_slow(x), &approx, &corr);
#endif
    return r;
}

// ------------------------------------------------------------------------------------
// double-double helpers (a value is hi + lo, |lo| <= ulp(hi)/2)
// ------------------------------------------------------------------------------------
struct pgr_dd {
    double h, l;
};
PGR_CR_FN struct pgr_dd pgr_dd_fast_two_sum(double a, double b)  // |a| >= |b| (or a == 0)
{
    struct pgr_dd r;
    r.h = a + b;
    r.l = b - (r.h - a);
    return r;
}
PGR_CR_FN struct pgr_dd pgr_dd_two_sum(double a, double b)
{
    struct pgr_dd r;
    r.h = a + b;
    const double bb = r.h - a;
    r.l = (a - (r.h - bb)) + (b - bb);
    return r;
}
PGR_CR_FN struct pgr_dd pgr_dd_mul(struct pgr_dd a, struct pgr_dd b)
{
    const double p = a.h * b.h;
    double e = __builtin_fma(a.h, b.h, -p);
    e = __builtin_fma(a.h, b.l, e);
    e = __builtin_fma(a.l, b.h, e);
    return pgr_dd_fast_two_sum(p, e);
}
PGR_CR_FN struct pgr_dd pgr_dd_add(struct pgr_dd a, struct pgr_dd b)
{
    const struct pgr_dd s = pgr_dd_two_sum(a.h, b.h);
    return pgr_dd_fast_two_sum(s.h, s.l + (a.l + b.l));
}
PGR_CR_FN struct pgr_dd pgr_dd_make(double h, double l)
{
    struct pgr_dd r;
    r.h = h;
    r.l = l;
    return r;
}

// sin and cos of y = y.h + y.l, |y| <= 0.89, as double-double, ~2^-100 relative (sin) / absolute (cos):
// y = j/32 + d, |d| <= 1/64 + ulp; sin d and cos d by their Taylor series, the leading terms
// in double-double; the angle-sum formulas with the tabulated sin(j/32), cos(j/32)
PGR_CR_FN void pgr_dd_sincos_x(struct pgr_dd y, struct pgr_dd* s_out, struct pgr_dd* c_out, const int c_plain)
{
    const double jr = __builtin_rint(y.h * 32.0);
    const struct pgr_dd d = pgr_dd_fast_two_sum(y.h - jr * 0.03125, y.l);  // y.h - j/32 is exact
    const struct pgr_dd z = pgr_dd_mul(d, d);
    // sin d = d (1 + z (S3 + z (S5 + z (S7 + z (S9 + z S11)))))
    struct pgr_dd t = pgr_dd_two_sum(PGR_CR_S7_H, z.h * __builtin_fma(z.h, PGR_CR_S11, PGR_CR_S9));
    t.l += PGR_CR_S7_L;
    t = pgr_dd_add(pgr_dd_make(PGR_CR_S5_H, PGR_CR_S5_L), pgr_dd_mul(z, t));
    t = pgr_dd_add(pgr_dd_make(PGR_CR_S3_H, PGR_CR_S3_L), pgr_dd_mul(z, t));
    t = pgr_dd_mul(z, t);
    {
        const struct pgr_dd o = pgr_dd_fast_two_sum(1.0, t.h);
        t = pgr_dd_fast_two_sum(o.h, o.l + t.l);
    }
    const struct pgr_dd sd = pgr_dd_mul(d, t);
    // cos d = 1 + z (-1/2 + z (C4 + z (C6 + z (C8 + z (C10 + z C12)))))
    struct pgr_dd u = pgr_dd_two_sum(
        PGR_CR_C6_H, z.h * __builtin_fma(z.h, __builtin_fma(z.h, PGR_CR_C12, PGR_CR_C10), PGR_CR_C8));
    u.l += PGR_CR_C6_L;
    u = pgr_dd_add(pgr_dd_make(PGR_CR_C4_H, PGR_CR_C4_L), pgr_dd_mul(z, u));
    u = pgr_dd_mul(z, u);
    {
        const struct pgr_dd o = pgr_dd_fast_two_sum(-0.5, u.h);
        u = pgr_dd_fast_two_sum(o.h, o.l + u.l);
    }
    u = pgr_dd_mul(z, u);
    {
        const struct pgr_dd o = pgr_dd_fast_two_sum(1.0, u.h);
        u = pgr_dd_fast_two_sum(o.h, o.l + u.l);
    }
    const struct pgr_dd cd = u;
    if (jr == 0.0) {
        *s_out = sd;
        *c_out = cd;
        return;
    }
    const int j = (int)__builtin_fabs(jr);
    const double sg = jr < 0.0 ? -1.0 : 1.0;
    const double* q = pgr_cr_sincos_tab + 4 * (j > 28 ? 28 : j);
    const struct pgr_dd sj = pgr_dd_make(sg * q[0], sg * q[1]), cj = pgr_dd_make(q[2], q[3]);
    *s_out = pgr_dd_add(pgr_dd_mul(sj, cd), pgr_dd_mul(cj, sd));
    if (c_plain) {  // the cosine to double precision only (the divisor of arcsine's Newton step)
        *c_out = pgr_dd_make(cj.h * cd.h - sj.h * sd.h, 0.0);
        return;
    }
    const struct pgr_dd m = pgr_dd_mul(sj, sd);
    *c_out = pgr_dd_add(pgr_dd_mul(cj, cd), pgr_dd_make(-m.h, -m.l));
}
PGR_CR_FN void pgr_dd_sincos(struct pgr_dd y, struct pgr_dd* s_out, struct pgr_dd* c_out)
{
    pgr_dd_sincos_x(y, s_out, c_out, 0);
}

// sin(x), correctly rounded, |x| <= 6.5 (the reflection law's argument is radians(theta_b),
// |theta_b| <= 270 degrees); beyond that the plain library sine (not reached on this path)
PGR_CR_FN double pgr_cr_sin(double x)
{
    if (x == 0.0) return x;
    if (!(__builtin_fabs(x) <= 6.5)) return pgr_cr_fallback_sin(x);
    const double kd = __builtin_rint(x * PGR_CR_2OPI);
    // y = x - k pi/2: k PIO2_1 is exact (33-bit constant), the first subtraction too
    const double t = __builtin_fma(-kd, PGR_CR_PIO2_1, x);
    const double p = kd * PGR_CR_PIO2_2, pe = __builtin_fma(kd, PGR_CR_PIO2_2, -p);
    struct pgr_dd y = pgr_dd_two_sum(t, -p);
    y = pgr_dd_fast_two_sum(y.h, y.l - __builtin_fma(kd, PGR_CR_PIO2_3, pe));
    struct pgr_dd s, c;
    pgr_dd_sincos(y, &s, &c);
    const int n = ((int)kd) & 3;
    const double r = (n & 1) ? c.h : s.h;
    return (n & 2) ? -r : r;
}

// asin(v) as a double-double (hi = the correctly rounded asin, hi + lo = asin to ~2^-100): one Newton
// step on sin(a) = v from a double-precision seed, sin and cos of the seed in double-double; |v| > 0.75
// through asin(v) = pi/2 - asin(sqrt(1 - v^2))
PGR_CR_FN struct pgr_dd pgr_cr_asin_dd(double v)
{
    const double a = __builtin_fabs(v);
    if (!(a <= 1.0)) return pgr_dd_make(pgr_cr_seed_asin(v), 0.0);  // NaN, as the library (Q7)
    if (a == 0.0) return pgr_dd_make(v, 0.0);
    struct pgr_dd r, s, c;
    if (a <= 0.75) {
        const double a0 = pgr_cr_seed_asin(a);
        pgr_dd_sincos_x(pgr_dd_make(a0, 0.0), &s, &c, 1);
        r = pgr_dd_fast_two_sum(a0, ((a - s.h) - s.l) / c.h);
    } else {
        const double m = 1.0 - a;  // exact
        const struct pgr_dd n = pgr_dd_two_sum(1.0, a);
        const double ph = m * n.h, pl = __builtin_fma(m, n.l, __builtin_fma(m, n.h, -ph));  // 1 - v^2
        const double wh = __builtin_sqrt(ph);
        struct pgr_dd b = pgr_dd_make(0.0, 0.0);
        if (wh > 0.0) {
            const double wl = (__builtin_fma(-wh, wh, ph) + pl) / (wh + wh);  // sqrt(1 - v^2) = wh + wl
            const double b0 = pgr_cr_seed_asin(wh);
            pgr_dd_sincos_x(pgr_dd_make(b0, 0.0), &s, &c, 1);
            b = pgr_dd_fast_two_sum(b0, (((wh - s.h) - s.l) + wl) / c.h);
        }
        const struct pgr_dd q = pgr_dd_two_sum(PGR_CR_PIO2_H, -b.h);
        r = pgr_dd_fast_two_sum(q.h, q.l + (PGR_CR_PIO2_L - b.l));
    }
    return v < 0.0 ? pgr_dd_make(-r.h, -r.l) : r;
}
PGR_CR_FN double pgr_cr_asin(double v) { return pgr_cr_asin_dd(v).h; }

// sin(x) for an x that is a few ulps from -asin(v) -- the reflection law's sin(radians(-degrees(arcsin v)))
// at the surface or a flat sea floor (REF/launch_rays.py:459-480): with A = asin v as a double-double,
// x = -A + d with |d| ~ 2^-51 |A|, so sin x = -v cos d + sqrt(1 - v^2) sin d = -v + sqrt(1 - v^2) d
// + O(2^-102): one rounding of a value good to ~2^-98, correctly rounded like pgr_cr_sin(x) and two
// hundred instructions cheaper.  The caller passes x as it computed it; anything further from -A than
// 2^-40 |A| (not a reflection of this kind) takes the general sine.
PGR_CR_FN double pgr_cr_sin_near_minus_asin(double x, double v, struct pgr_dd A)
{
    const struct pgr_dd t = pgr_dd_two_sum(x, A.h);       // x + A, exactly
    const double d = t.h + (t.l + A.l);
    if (!(__builtin_fabs(d) <= 0x1.0p-40 * __builtin_fabs(A.h)) || !(__builtin_fabs(v) < 0.999)) return pgr_cr_sin(x);
    const double w = __builtin_sqrt(__builtin_fma(-v, v, 1.0)) * d;
    return -v + w;
}

#endif  // PGR_CRMATH_H
