// pgr_trig.h -- gcos2pi / gsin2pi, the library's cos(2 pi t) and sin(2 pi t), beside gexp (included by pgr_beams.h).
// Plain arithmetic behind __device__ __forceinline__ and nothing else of the translation unit, so that a host compiler can
// build it too (tests/test_coherent_host.py compiles it with both words defined away and compares bits with the restatement).
#ifndef PGR_TRIG_H
#define PGR_TRIG_H

// cos(2 pi t) and sin(2 pi t) for t in [-0.5, 0.5] (NaN for a NaN) from compares and + - x only, in a fixed order and without
// contraction, for the same reason as gexp: |t| folded about 1/4 (the cosine changes sign) and about 1/8 (sine and cosine
// change places) to b in [0, 1/8], every fold an exact subtraction; then, in z = b^2, the Taylor polynomials of degree 8 of
// sin(2 pi b) / b - 2 pi and cos(2 pi b) - 1 in Horner form (truncation < 1e-19), 2 pi taken in two parts so that the
// sine's leading term b * 2 pi is rounded once.  Absolute error at most 1.36e-16 measured.
__device__ __forceinline__ void gcossin2pi(double t, double& c, double& s)
{
    double a = t < 0.0 ? -t : t;
    const bool flip = a > 0.25;
    a = flip ? 0.5 - a : a;
    const bool swap = a > 0.125;
    const double b = swap ? 0.25 - a : a;
    const double z = b * b;
    double ps = 0x1.aaec32af93359p-4;                                        // (2 pi)^17 / 17!
    ps = ps * z + -0x1.6fadb9f155744p-1;
    ps = ps * z + 0x1.e8f434d018d63p+1;
    ps = ps * z + -0x1.e3074fde8871fp+3;
    ps = ps * z + 0x1.50783487ee782p+5;
    ps = ps * z + -0x1.32d2cce62bd86p+6;
    ps = ps * z + 0x1.466bc6775aae2p+6;
    ps = ps * z + -0x1.4abbce625be53p+5;                                     // -(2 pi)^3 / 3!
    double pc = 0x1.20c62c2f2d7f5p-2;                                        // (2 pi)^16 / 16!
    pc = pc * z + -0x1.b6e24f44b128fp+0;
    pc = pc * z + 0x1.f9d38a3763cc3p+2;
    pc = pc * z + -0x1.a6d1f2a204a8cp+4;
    pc = pc * z + 0x1.e1f506891babbp+5;
    pc = pc * z + -0x1.55d3c7e3cbffap+6;
    pc = pc * z + 0x1.03c1f081b5ac4p+6;
    pc = pc * z + -0x1.3bd3cc9be45dep+4;                                     // -(2 pi)^2 / 2!
    const double S = b * 0x1.921fb54442d18p+2 + b * (0x1.1a62633145c07p-52 + z * ps);   // 2 pi = hi + lo
    const double C = 1.0 + z * pc;
    const double cv = swap ? S : C, sv = swap ? C : S;
    c = flip ? -cv : cv;
    s = t < 0.0 ? -sv : sv;
}

__device__ __forceinline__ double gcos2pi(double t)
{
    double c, s;
    gcossin2pi(t, c, s);
    return c;
}

__device__ __forceinline__ double gsin2pi(double t)
{
    double c, s;
    gcossin2pi(t, c, s);
    return s;
}

#endif  // PGR_TRIG_H
