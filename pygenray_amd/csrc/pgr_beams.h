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
// Two passes, no atomics, as TL's:
//   pgr_gb_bounds  one wave per (column s, chunk of GB_TUBES tubes): the depths the chunk's beams reach, [min(m - 4 sigma),
//                  max(m + 4 sigma)], widened so that it is never stricter than the per-term test;
//   pgr_gb_sum     one wave per (column, band of 64 receivers): walks the chunks in order, enters those whose interval or
//                  its mirror about 0 or about b_s meets the band, forms the chunk's tubes (m, sigma, A) into LDS, and
//                  each lane adds its receiver's terms tube by tube, centre by centre.  One lane forms each receiver's sum
//                  in the definition's order, so the result equals the sequential sum bit for bit.
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

struct GbArgs {
    TlArgs t;                 // the fan, its frame, p0, the receivers, the chunk bounds and out, as TL's (chunks of GB_TUBES
                              // tubes; all S columns, no column list)
    const double* bottom;     // [S] bottom depth at x_s, in the frame the fan was traced in
    double wmin;              // floor on the beam width sigma
};

// where surviving ray m's sample s lies in Z / P (m in 0 .. M-1; dropped rays skipped through the keep list)
__device__ __forceinline__ int64_t gb_index(const TlArgs& a, int s, int64_t m)
{
    return tl_index(a, s, a.keep ? (int64_t)a.keep[m] : m);
}

// lane t holds ray c * GB_TUBES - 1 + t's depth d: tube t's centre and width (valid for t < GB_TUBES).  fmax ignores NaN
__device__ __forceinline__ void gb_shape(double wmin, double d, double& mid, double& sig)
{
    const double d1 = __shfl_down(d, 1), d2 = __shfl_down(d, 2), d3 = __shfl_down(d, 3);
    mid = 0.5 * (d1 + d2);
    sig = fmax(fmax(fmax(fabs(d1 - d), fabs(d2 - d1)), fabs(d3 - d2)), wmin);
}

// pass 1: the depths chunk c's beams reach in column s, [lo, hi] (tubes with a NaN centre ignored; none: [+inf, -inf]).
// Widened by 2^-40 of its magnitude, which covers the rounding of m -+ sigma GB_REACH and of the receiver's d - m.
__global__ void __launch_bounds__(256) pgr_gb_bounds(GbArgs g)
{
    const TlArgs& a = g.t;
    const int s = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = threadIdx.x & 63;
    if (c >= a.nchunk) return;                      // (whole waves: c is uniform in the wave)
    const int64_t k = c * GB_TUBES + t;             // lane t: ray k - 1 and tube k
    const int64_t m = k - 1;
    double d = NAN;                                 // (rays outside 0 .. M-1 are NaN)
    if (m >= 0 && m < a.M) d = a.zsign * a.Z[gb_index(a, s, m)];
    double mid, sig;
    gb_shape(g.wmin, d, mid, sig);
    double lo = INFINITY, hi = -INFINITY;
    if (t < GB_TUBES && k + 1 < a.M && mid == mid) {
        const double w = sig * GB_REACH;
        lo = mid - w;
        hi = mid + w;
    }
    lo = tl_wave_min(lo);
    hi = tl_wave_max(hi);
    if (t == 0) {
        if (lo <= hi) {
            const double pad = 0x1p-40 * fmax(fabs(lo), fabs(hi));
            lo -= pad;
            hi += pad;
        }
        double* b = a.bounds + 2 * ((int64_t)s * a.nchunk + c);
        b[0] = lo;
        b[1] = hi;
    }
}

// the LDS of one wave's walk: the current chunk's tubes (m NaN where the tube adds nothing)
struct GbTubes { double m[64], sig[64], A[64]; };

// The tubes of chunk c in column s into LDS: lane t loads ray c * GB_TUBES - 1 + t (its depth, g and launch slowness) and
// forms tube t from lanes t .. t + 3 by lane shuffles.
__device__ __forceinline__ void gb_chunk_tubes(const GbArgs& g, const Ctx<false, 0>& C, int s, double x, double r,
                                               int64_t c, int t, GbTubes& L)
{
    const TlArgs& a = g.t;
    const int64_t k = c * GB_TUBES + t;
    const int64_t m = k - 1;
    double d = NAN, gr = NAN, q0 = NAN;
    if (m >= 0 && m < a.M) {
        const int64_t i = gb_index(a, s, m);
        d = a.zsign * a.Z[i];
        const double p = a.P[i];
        q0 = a.p0[m];
        if (d == d && p == p) {
            double cv, cp;
            C.lookup(x, d, cv, cp);
            const double pc = p * cv;
            if (fabs(pc) < 1.0) gr = fdiv(cv, fsqrt(1.0 - pc * pc));
        }
    }
    double mid, sig;
    gb_shape(g.wmin, d, mid, sig);
    const double g1 = __shfl_down(gr, 1), g2 = __shfl_down(gr, 2);
    const double q1 = __shfl_down(q0, 1), q2 = __shfl_down(q0, 2);
    double A = 0.0;
    if (t < GB_TUBES && k + 1 < a.M && g1 == g1 && g2 == g2) {
        const double E = fdiv(0.5 * (g1 + g2) * fabs(q2 - q1), r);
        A = fdiv(E, sig * GB_SQRT_2PI);
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
    const TlArgs& a = g.t;
    const int s = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.y * 64 + t;
    const bool rcv = j < a.R;
    const double d = rcv ? a.depths[j] : a.depths[a.R - 1];
    const double x = a.x[s];
    const double r = fabs(x - a.x[0]);
    if (r == 0.0) {                                  // the source's own column
        if (rcv) a.out[j * a.S + s] = NAN;
        return;
    }
    const double b2 = 2.0 * g.bottom[s];
    const double padb = 0x1p-40 * fabs(b2);          // the rounding of 2 b - m, beyond what pass 1's widening covers
    const Ctx<false, 0> C(env, nullptr);
    const double dlo = tl_wave_min(d), dhi = tl_wave_max(d);
    const double* bnd = a.bounds + 2 * (int64_t)s * a.nchunk;
    double acc = 0.0;
    for (int64_t c0 = 0; c0 < a.nchunk; c0 += 64) {
        int which = 0;                               // lane t: the centres of chunk c0 + t that may reach the band
        if (c0 + t < a.nchunk) {
            const double lo = bnd[2 * (c0 + t)], hi = bnd[2 * (c0 + t) + 1];
            which = ((lo <= dhi) & (hi >= dlo))
                  | (((-hi <= dhi) & (-lo >= dlo)) << 1)
                  | (((b2 - hi - padb <= dhi) & (b2 - lo + padb >= dlo)) << 2);
        }
        unsigned long long mask = ballot64(which != 0);
        while (mask) {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int w = __shfl(which, l);
            gb_chunk_tubes(g, C, s, x, r, c0 + l, t, L);
            for (int u = 0; u < GB_TUBES; u++) {
                const double m = L.m[u], sig = L.sig[u], A = L.A[u];
                if (w & 1) gb_term(acc, d, m, sig, A);
                if (w & 2) gb_term(acc, d, -m, sig, A);
                if (w & 4) gb_term(acc, d, b2 - m, sig, A);
            }
        }
    }
    if (rcv) a.out[j * a.S + s] = acc;
}

static int gb_run(const pgr_env* env, GbArgs g, hipStream_t st, const char* who)
{
    TlArgs& a = g.t;
    a.nchunk = (a.M - 1 + GB_TUBES - 1) / GB_TUBES;
    a.cols = nullptr;
    a.ncol = a.S;
    void* b = nullptr;
    if (hipMallocAsync(&b, (size_t)a.S * (size_t)a.nchunk * 16, st) != hipSuccess)
        return fail(std::string(who) + ": device allocation of the chunk bounds failed");
    a.bounds = (double*)b;
    hipLaunchKernelGGL(pgr_gb_bounds, dim3((unsigned)((a.nchunk + 3) / 4), (unsigned)a.S), dim3(256), 0, st, g);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_gb_sum, dim3((unsigned)a.S, (unsigned)((a.R + 63) / 64)), dim3(64), 0, st, env->d, g);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

static int gb_check(int64_t M, int32_t S, const double* p0, const double* bottom, const double* depths, int64_t R,
                    double min_width, const void* out, const char* who)
{
    int rc = tl_check(M, S, p0, depths, R, out, who);
    if (rc) return rc;
    if (!bottom) return fail(std::string(who) + ": null argument");
    if (!(min_width > 0.0) || !std::isfinite(min_width)) return fail(std::string(who) + ": min_width must be finite and > 0");
    return 0;
}

extern "C" int pgr_fan_beam_intensity(pgr_fan* f, const double* p0, const double* bottom, const double* depths,
                                      int64_t n_depths, double min_width, double* out, void* stream)
{
    const char* who = "pgr_fan_beam_intensity";
    if (!f) return fail(std::string(who) + ": null fan");
    if (!f->save) return fail(std::string(who) + ": the fan was launched without trajectories (S = 0)");
    std::lock_guard<std::mutex> lock(f->m);
    GbArgs g{};
    int rc = tl_fan_args(f, g.t, who,
                         [&] { return gb_check(f->M, f->S, p0, bottom, depths, n_depths, min_width, out, who); });
    if (rc) return rc;
    g.t.p0 = p0; g.t.depths = depths; g.t.R = n_depths; g.t.out = out;
    g.bottom = bottom;
    g.wmin = min_width;
    return gb_run(f->env, g, (hipStream_t)stream, who);
}

extern "C" int pgr_beam_intensity_device(pgr_env* env, const double* z, const double* p, int64_t n_rays,
                                         int32_t n_samples, const double* x, const double* p0, const double* bottom,
                                         const double* depths, int64_t n_depths, double min_width, double* out,
                                         void* stream)
{
    const char* who = "pgr_beam_intensity_device";
    if (!env) return fail(std::string(who) + ": null environment");
    if (!z || !p || !x) return fail(std::string(who) + ": null argument");
    int rc = gb_check(n_rays, n_samples, p0, bottom, depths, n_depths, min_width, out, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(env->device));
    GbArgs g{};
    TlArgs& a = g.t;
    a.Z = z; a.P = p; a.keep = nullptr;
    a.N = n_rays; a.M = n_rays; a.S = n_samples; a.blocked = 0;
    a.zsign = -1.0;
    a.x = x; a.p0 = p0; a.depths = depths; a.R = n_depths; a.out = out;
    g.bottom = bottom;
    g.wmin = min_width;
    return gb_run(env, g, (hipStream_t)stream, who);
}

#endif  // PGR_BEAMS_H
