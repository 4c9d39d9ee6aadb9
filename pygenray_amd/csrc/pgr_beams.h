// pgr_beams.h -- incoherent geometric Gaussian-beam intensity of a fan on a range-depth grid: pgr_fan_beam_intensity,
// pgr_beam_intensity_device.  (Part of the ONE translation unit pgr_hip.hip, included there after pgr_tl.h and
// pgr_arrivals.h; not a stand-alone header.)
//
// The quantity (DESIGN.md section "Gaussian beams"), in TL's notation: tube k (rays k, k + 1) at save column s has
//   E_k = 0.5 (g_k + g_k+1) |p0_k+1 - p0_k| / r_s                       the depth-integrated intensity of TL's tube
//   sigma_k = max(D_k-1, D_k, D_k+1, w_min),  D_i = |d_i+1 - d_i|      (NaN widths, and those beyond the fan, ignored)
//   m_k = 0.5 (d_k + d_k+1),   A_k = E_k / (sigma_k SQRT_2PI)
// and receiver j gets the sum, in increasing k from 0.0 and for each tube over the centres m_k, -m_k, 2 b_s - m_k (the beam
// and its images in the surface and the bottom), of A_k gexp(-v / 2) over the terms with v = ((d_j - centre) / sigma_k)^2
// <= 16 (beams cut at 4 sigma).  A tube adds nothing when g is not finite at either end (a NaN sample, |p c| >= 1); unlike
// TL, d_k+1 == d_k is allowed.  The column r_s == 0 is NaN.
//
// pgr_tl.h's two-pass tube walk with a second tube shape (chunks of GB_TUBES tubes and a halo ray either side):
//   pgr_gb_bounds  tube_bounds: the depths the chunk's beams reach, [min(m - 4 sigma), max(m + 4 sigma)], widened so that it
//                  is never stricter than the per-term test;
//   pgr_gb_sum     tube_walk: enters the chunks whose interval or its mirror about 0 or about b_s meets the band (a mask
//                  of three tests, one per centre), forms the chunk's tubes (m, sigma, A) into LDS, and each lane adds its
//                  receiver's terms tube by tube, centre by centre.  One lane forms each receiver's sum in the
//                  definition's order, so the result equals the sequential sum bit for bit.
#ifndef PGR_BEAMS_H
#define PGR_BEAMS_H

// tubes per chunk: lane t holds ray c * GB_TUBES - 1 + t, so tube u of the chunk (rays u + 1, u + 2 of the wave) finds the
// neighbouring rays its sigma needs in lanes u and u + 3
#define GB_TUBES 61

#define GB_SQRT_2PI 0x1.40d931ff62706p+1   // the double nearest sqrt(2 pi)
// a beam's reach for the cheap tests: 4 sigma (1 + 2^-20).  fl((e / sigma)^2) <= 16 implies |e| <= 4 sigma (1 + 3 eps), so a
// test |e| <= sigma * GB_REACH never drops a term the definition keeps
#define GB_REACH 0x1.00001p+2

// exp(y) for y in [-8, 0] from + - x, rint and ldexp only, in a fixed order and without contraction (so a NumPy
// restatement repeats it bit for bit): y = k ln2 + r with fdlibm's two-part ln2, |r| <= ln2 / 2, then the degree-13
// Taylor polynomial of exp(r) in Horner form (truncation < 4e-18 relative) and the exact scaling by 2^k
__device__ __forceinline__ double gexp(double y)
{
    const double k = rint(y * 0x1.71547652b82fep+0);                       // log2(e)
    const double r = (y - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33;
    double p = 0x1.6124613a86d09p-33;                                        // 1 / 13!
    p = p * r + 0x1.1eed8eff8d898p-29;
    p = p * r + 0x1.ae64567f544e4p-26;
    p = p * r + 0x1.27e4fb7789f5cp-22;
    p = p * r + 0x1.71de3a556c734p-19;
    p = p * r + 0x1.a01a01a01a01ap-16;
    p = p * r + 0x1.a01a01a01a01ap-13;
    p = p * r + 0x1.6c16c16c16c17p-10;
    p = p * r + 0x1.1111111111111p-7;
    p = p * r + 0x1.5555555555555p-5;
    p = p * r + 0x1.5555555555555p-3;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return ldexp(p, (int)k);
}

#include "pgr_trig.h"   // gcos2pi, gsin2pi: cos / sin of 2 pi t by a fixed sequence, for the coherent sum (pgr_phase.h)

// the tube walk's arguments (chunks of GB_TUBES tubes; all S columns, no column list) and the beams' own
struct GbArgs : TlArgs {
    const double* bottom;     // [S] bottom depth at x_s, in the frame the fan was traced in
    double wmin;              // floor on the beam width sigma
};

// lane t holds ray c * GB_TUBES - 1 + t's depth d: tube t's centre and width (valid for t < GB_TUBES).  fmax ignores NaN
__device__ __forceinline__ void gb_shape(double wmin, double d, double& mid, double& sig)
{
    const double d1 = __shfl_down(d, 1), d2 = __shfl_down(d, 2), d3 = __shfl_down(d, 3);
    mid = 0.5 * (d1 + d2);
    sig = fmax(fmax(fmax(fabs(d1 - d), fabs(d2 - d1)), fabs(d3 - d2)), wmin);
}

// pass 1: the depths chunk c's beams reach in column s, [lo, hi] (tubes with a NaN centre ignored; none: [+inf, -inf]).
// Widened by 2^-40 of its magnitude, which covers the rounding of m -+ sigma GB_REACH and of the receiver's d - m.
// (column slot blockIdx.y is column s: the slot itself, or with COLS the caller's cols[slot], pgr_beam_arrivals.h)
template <bool COLS>
__device__ __forceinline__ void gb_bounds(const GbArgs& g)
{
    const int s = COLS ? tl_column(g, blockIdx.y) : (int)blockIdx.y;
    tube_bounds<GB_TUBES, -1, true>(g, [&](int t, int64_t m, double& lo, double& hi) {
        double d = NAN;                              // (rays outside 0 .. M-1 are NaN)
        if (m >= 0 && m < g.M) d = g.zsign * g.Z[tl_index(g, s, m)];
        double mid, sig;
        gb_shape(g.wmin, d, mid, sig);
        if (t < GB_TUBES && m + 2 < g.M && mid == mid) {
            const double w = sig * GB_REACH;
            lo = mid - w;
            hi = mid + w;
        }
    });
}

__global__ void __launch_bounds__(256) pgr_gb_bounds(GbArgs g) { gb_bounds<false>(g); }

// the LDS of one wave's walk: the current chunk's tubes (m NaN where the tube adds nothing)
struct GbTubes { double m[64], sig[64], A[64]; };

// The tubes of chunk c in column s into LDS: lane t loads ray c * GB_TUBES - 1 + t and forms tube t from lanes t .. t + 3
// by lane shuffles.
__device__ __forceinline__ void gb_chunk_tubes(const GbArgs& g, const Ctx<false, 0>& C, int s, double x, double r,
                                               int64_t c, int t, GbTubes& L)
{
    const int64_t k = c * GB_TUBES + t;
    const int64_t m = k - 1;
    const TlRay y = tl_ray<false>(g, C, s, x, m, m >= 0 && m < g.M);
    double mid, sig;
    gb_shape(g.wmin, y.d, mid, sig);
    const double g1 = __shfl_down(y.g, 1), g2 = __shfl_down(y.g, 2);
    const double q1 = __shfl_down(y.q0, 1), q2 = __shfl_down(y.q0, 2);
    double A = 0.0;
    if (t < GB_TUBES && k + 1 < g.M && g1 == g1 && g2 == g2) {
        const double E = fdiv_inf(0.5 * (g1 + g2) * fabs(q2 - q1), r);          // (g W can be infinite, as in tl_chunk_tubes)
        A = fdiv_inf(E, sig * GB_SQRT_2PI);
    } else {
        mid = NAN;                                   // every test of a NaN centre fails: the tube adds nothing
    }
    __syncthreads();                                 // (the previous chunk's tubes have been read)
    L.m[t] = mid;
    L.sig[t] = sig;
    L.A[t] = A;
    __syncthreads();
}

// one term: the beam of width sig and amplitude A centred at ctr, at depth d
__device__ __forceinline__ void gb_term(double& acc, double d, double ctr, double sig, double A)
{
    const double e = d - ctr;
    if (fabs(e) <= sig * GB_REACH) {                 // (a cheap test that never drops a term the next one keeps)
        const double u = fdiv(e, sig);
        const double v = u * u;
        if (v <= 16.0) acc = acc + A * gexp(-0.5 * v);
    }
}

// pass 2: one wave per (column, band of 64 receivers)
__global__ void __launch_bounds__(64) pgr_gb_sum(EnvDev env, GbArgs g)
{
    __shared__ GbTubes L;
    const TlBand b = tl_band<false>(g);
    if (b.r == 0.0) {                                // the source's own column
        b.put(g, NAN);
        return;
    }
    const double b2 = 2.0 * g.bottom[b.s];
    const double padb = 0x1p-40 * fabs(b2);          // the rounding of 2 b - m, beyond what pass 1's widening covers
    const Ctx<false, 0> C(env, nullptr);
    double acc = 0.0;
    tube_walk<3>(g, b.slot, b.d, b.t,
                 // the centres of the chunk that may reach the band: the beam, its images in the surface and the bottom
                 [&](double lo, double hi, double dlo, double dhi) {
                     return ((lo <= dhi) & (hi >= dlo))
                          | (((-hi <= dhi) & (-lo >= dlo)) << 1)
                          | (((b2 - hi - padb <= dhi) & (b2 - lo + padb >= dlo)) << 2);
                 },
                 [&](int64_t c, int w) {
                     gb_chunk_tubes(g, C, b.s, b.x, b.r, c, b.t, L);
                     for (int u = 0; u < GB_TUBES; u++) {
                         const double m = L.m[u], sig = L.sig[u], A = L.A[u];
                         if (w & 1) gb_term(acc, b.d, m, sig, A);
                         if (w & 2) gb_term(acc, b.d, -m, sig, A);
                         if (w & 4) gb_term(acc, b.d, b2 - m, sig, A);
                     }
                 });
    b.put(g, acc);
}

// the beams' own checks (tl_check has run)
static int gb_check(const double* bottom, double min_width, const char* who)
{
    if (!bottom) return fail(std::string(who) + ": null argument");
    if (!(min_width > 0.0) || !std::isfinite(min_width)) return fail(std::string(who) + ": min_width must be finite and > 0");
    return 0;
}

static int gb_intensity(const pgr_env* env, const TlArgs& a, const double* bottom, double min_width, double* out,
                        void* stream, const char* who)
{
    GbArgs g{a, bottom, min_width};
    g.out = out;
    return tube_run(env, g, GB_TUBES, pgr_gb_bounds, nullptr, 0, (hipStream_t)stream, who, pgr_gb_sum);
}

// the two entries and their weighted twins (`who`: the entry named in errors)
static int gb_fan_intensity(pgr_fan* f, const double* p0, const double* W, const double* bottom, const double* depths,
                            int64_t n_depths, double min_width, double* out, void* stream, const char* who)
{
    return tl_fan_entry(f, p0, W, depths, n_depths, out, who, [&](int32_t) { return gb_check(bottom, min_width, who); },
                        [&](const pgr_env* e, const TlArgs& a) {
                            return gb_intensity(e, a, bottom, min_width, out, stream, who);
                        });
}

static int gb_buffer_intensity(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                               const double* x, const double* p0, const double* W, const double* bottom,
                               const double* depths, int64_t n_depths, double min_width, double* out, void* stream,
                               const char* who)
{
    return tl_buffer_entry<false>(env, nullptr, z, p, n_rays, n_samples, x, p0, W, depths, n_depths, out, who,
                                  [&](int32_t) { return gb_check(bottom, min_width, who); },
                                  [&](const pgr_env* e, const TlArgs& a) {
                                      return gb_intensity(e, a, bottom, min_width, out, stream, who);
                                  });
}

extern "C" int pgr_fan_beam_intensity(pgr_fan* f, const double* p0, const double* bottom, const double* depths,
                                      int64_t n_depths, double min_width, double* out, void* stream)
{
    return gb_fan_intensity(f, p0, nullptr, bottom, depths, n_depths, min_width, out, stream, "pgr_fan_beam_intensity");
}

extern "C" int pgr_fan_beam_intensity_w(pgr_fan* f, const double* p0, const double* weights, const double* bottom,
                                        const double* depths, int64_t n_depths, double min_width, double* out, void* stream)
{
    return gb_fan_intensity(f, p0, weights, bottom, depths, n_depths, min_width, out, stream, "pgr_fan_beam_intensity_w");
}

extern "C" int pgr_beam_intensity_device(pgr_env* env, const double* z, const double* p, int64_t n_rays,
                                         int32_t n_samples, const double* x, const double* p0, const double* bottom,
                                         const double* depths, int64_t n_depths, double min_width, double* out,
                                         void* stream)
{
    return gb_buffer_intensity(env, z, p, n_rays, n_samples, x, p0, nullptr, bottom, depths, n_depths, min_width, out,
                               stream, "pgr_beam_intensity_device");
}

extern "C" int pgr_beam_intensity_device_w(pgr_env* env, const double* z, const double* p, int64_t n_rays,
                                           int32_t n_samples, const double* x, const double* p0, const double* weights,
                                           const double* bottom, const double* depths, int64_t n_depths, double min_width,
                                           double* out, void* stream)
{
    return gb_buffer_intensity(env, z, p, n_rays, n_samples, x, p0, weights, bottom, depths, n_depths, min_width, out,
                               stream, "pgr_beam_intensity_device_w");
}

#endif  // PGR_BEAMS_H
