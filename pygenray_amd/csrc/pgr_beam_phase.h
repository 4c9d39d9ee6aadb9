// pgr_beam_phase.h -- the coherent sum of a fan's geometric Gaussian beams, with the wavefront curvature across each tube:
// pgr_fan_beam_pressure_w, pgr_beam_pressure_device_w.
// (Part of the ONE translation unit pgr_hip.hip, included there after pgr_phase.h; not a stand-alone header.)
//
// The quantity, in the notation of pgr_beams.h and pgr_phase.h.  Tube k (rays k, k + 1) at save column s
// has pgr_beams.h's E_k, D_k = |d_k+1 - d_k|, sigma_k and m_k, bit for bit, and with p = zsign P the rays' slowness along
// increasing depth (dT/dd at a fixed range; the stored p with the depth's own sign, an exact operation)
//   T_m = 0.5 (T_k + T_k+1),   p_m = 0.5 (p_k + p_k+1)
//   hk  = curvature && D_k > 0 ? 0.5 * ((p_k+1 - p_k) / (d_k+1 - d_k)) : 0.0
//   A'_k = sqrt(E_k * D_k) / (sigma_k SQRT_2PI)
// A tube adds its terms when pgr_gb_sum's tube does and q[s][k] >= 0 (q: pgr_phase.h's phase index, NULL: all zero).  Receiver
// j takes the centres m_k, -m_k, 2 b_s - m_k in that order, each with pgr_gb_sum's own v and its v <= 16 test, and
//   e = d_j - m_k,   (-d_j) - m_k,   (2 b_s - d_j) - m_k        the receiver, mirrored with the image, in the beam's own space
//   dq = 0, 2, 0                                                  a pressure-release surface, a rigid bottom
//   a   = A'_k gexp(-0.5 v)
//   tau = T_m + (p_m e + hk (e e))
//   y = f tau;  y = y - rint(y);  t = y - 0.25 ((q + dq) & 3);  t = t - rint(t)
//   re += a gcos2pi(t),  im += a gsin2pi(t)
// summed from 0.0 in increasing k and per tube in centre order.
//   pgr_gbc_sum     pgr_gb_sum's walk after pgr_gb_bounds (sigma and the reach are the same): one wave per (column, band of 64
//                   receivers), chunks of GB_TUBES tubes, the 3-bit centre mask.  Each lane also loads its ray's T; the tubes'
//                   m, sigma, A', T_m, p_m, hk and q are staged in LDS.  One lane forms each receiver's two sums in the
//                   definition's order: no atomics, the result equals the sequential sum bit for bit.
#ifndef PGR_BEAM_PHASE_H
#define PGR_BEAM_PHASE_H

// the LDS of one wave's walk: the current chunk's tubes (m NaN where the tube adds nothing)
struct GbcTubes { double m[64], sig[64], A[64], Tm[64], pm[64], hk[64]; int32_t q[64]; };

// The tubes of chunk c in column s into LDS: gb_chunk_tubes with the rays' T and p.  `curv` (uniform in the launch): 0 leaves
// every hk 0.0, the plain geometric beam.  `q`: column s's row of the phase index or NULL.
__device__ __forceinline__ void gbc_chunk_tubes(const GbArgs& g, const Ctx<false, 0>& C, int s, double x, double r,
                                                int64_t c, int t, const int32_t* q, int curv, GbcTubes& L)
{
    const int64_t k = c * GB_TUBES + t;              // tube t of the chunk: surviving rays k, k + 1 (lanes t + 1, t + 2)
    const int64_t m = k - 1;
    const TlRay y = tl_ray<true>(g, C, s, x, m, m >= 0 && m < g.M);
    double mid, sig;
    gb_shape(g.wmin, y.d, mid, sig);
    const double pd = g.zsign * y.p;                 // dT/dd: the slowness along increasing depth
    const double d1 = __shfl_down(y.d, 1), d2 = __shfl_down(y.d, 2);
    const double g1 = __shfl_down(y.g, 1), g2 = __shfl_down(y.g, 2);
    const double q1 = __shfl_down(y.q0, 1), q2 = __shfl_down(y.q0, 2);
    const double T1 = __shfl_down(y.T, 1), T2 = __shfl_down(y.T, 2);
    const double p1 = __shfl_down(pd, 1), p2 = __shfl_down(pd, 2);
    double A = 0.0, hk = 0.0;
    int qk = 0;
    const bool tube = t < GB_TUBES && k + 1 < g.M;
    if (tube && q) qk = q[k];
    if (tube && g1 == g1 && g2 == g2 && qk >= 0) {
        const double E = fdiv_inf(0.5 * (g1 + g2) * fabs(q2 - q1), r);
        const double D = fabs(d2 - d1);
        A = fdiv_inf(fsqrt(E * D), sig * GB_SQRT_2PI);
        if (curv && D > 0.0) hk = 0.5 * fdiv(p2 - p1, d2 - d1);
    } else {
        mid = NAN;                                   // every test of a NaN centre fails: the tube adds nothing
    }
    __syncthreads();                                 // (the previous chunk's tubes have been read)
    L.m[t] = mid;
    L.sig[t] = sig;
    L.A[t] = A;
    L.Tm[t] = 0.5 * (T1 + T2);
    L.pm[t] = 0.5 * (p1 + p2);
    L.hk[t] = hk;
    L.q[t] = qk & 3;                                 // (whole cycles dropped here: q + 2 cannot overflow)
    __syncthreads();
}

// one term: the beam centred at ctr, seen from depth d (gb_term's tests), the receiver at e in the beam's own space and qk
// quarter cycles.  (Its two tests, a and tau have a twin, gbc_kept in pgr_beam_arrivals.h, which lists these terms as arrivals:
// an edit here is mirrored there, statement for statement.)
__device__ __forceinline__ void gbc_term(double& re, double& im, double f, double d, double ctr, double e, double sig, double A,
                                         double Tm, double pm, double hk, int qk)
{
    const double e0 = d - ctr;
    if (fabs(e0) <= sig * GB_REACH) {                // (a cheap test that never drops a term the next one keeps)
        const double u = fdiv(e0, sig);
        const double v = u * u;
        if (v <= 16.0) {
            const double a = A * gexp(-0.5 * v);
            const double tau = Tm + (pm * e + hk * (e * e));
            double y = f * tau;
            y = y - rint(y);
            double t = y - 0.25 * (double)(qk & 3);
            t = t - rint(t);
            double cv, sv;
            gcossin2pi(t, cv, sv);
            re = re + a * cv;
            im = im + a * sv;
        }
    }
}

// pass 2: one wave per (column, band of 64 receivers).  (The walk below -- the chunk test, the tubes in order, the centres the
// mask keeps -- has a twin, gbc_walk in pgr_beam_arrivals.h: an edit here is mirrored there; sharing it changed this kernel's
// machine code)
__global__ void __launch_bounds__(64) pgr_gbc_sum(EnvDev env, GbArgs g, CohOut o, int curv)
{
    __shared__ GbcTubes L;
    const TlBand b = tl_band<false>(g);
    double re = 0.0, im = 0.0;
    if (b.r == 0.0) {                                // the source's own column (uniform in the wave)
        re = NAN;
        im = NAN;
    } else {
        const double b2 = 2.0 * g.bottom[b.s];
        const double padb = 0x1p-40 * fabs(b2);      // the rounding of 2 b - m, beyond what pass 1's widening covers
        const Ctx<false, 0> C(env, nullptr);
        const int32_t* q = o.q ? o.q + (int64_t)b.s * g.M : nullptr;
        const double es = -b.d, eb = b2 - b.d;       // the receiver mirrored in the surface and in the bottom
        tube_walk<3>(g, b.slot, b.d, b.t,
                     // pgr_gb_sum's test: the centres of the chunk that may reach the band
                     [&](double lo, double hi, double dlo, double dhi) {
                         return ((lo <= dhi) & (hi >= dlo))
                              | (((-hi <= dhi) & (-lo >= dlo)) << 1)
                              | (((b2 - hi - padb <= dhi) & (b2 - lo + padb >= dlo)) << 2);
                     },
                     [&](int64_t c, int w) {
                         gbc_chunk_tubes(g, C, b.s, b.x, b.r, c, b.t, q, curv, L);
                         for (int u = 0; u < GB_TUBES; u++) {
                             const double m = L.m[u], sig = L.sig[u], A = L.A[u], Tm = L.Tm[u], pm = L.pm[u], hk = L.hk[u];
                             const int qk = L.q[u];
                             // (one body of the term for the three centres: its polynomials' constants are held once)
#pragma unroll 1
                             for (int ci = 0; ci < 3; ci++) {
                                 if (!((w >> ci) & 1)) continue;
                                 const double ctr = ci == 0 ? m : ci == 1 ? -m : b2 - m;
                                 const double e = (ci == 0 ? b.d : ci == 1 ? es : eb) - m;
                                 gbc_term(re, im, o.f, b.d, ctr, e, sig, A, Tm, pm, hk, ci == 1 ? qk + 2 : qk);
                             }
                         }
                     });
    }
    if (b.rcv) {
        o.re[b.j * g.S + b.s] = re;
        o.im[b.j * g.S + b.s] = im;
    }
}

static int gbc_run(const pgr_env* env, const TlArgs& a, const double* bottom, double min_width, const CohOut& o, int32_t curv,
                   void* stream, const char* who)
{
    GbArgs g{a, bottom, min_width};
    return tube_run(env, g, GB_TUBES, pgr_gb_bounds, nullptr, 0, (hipStream_t)stream, who, pgr_gbc_sum, o, (int)(curv != 0));
}

// the checks of both entries beyond tl_check: pgr_beams.h's and pgr_phase.h's
static int gbc_check(const double* bottom, double min_width, const double* re, const double* im, double f, const char* who)
{
    const int rc = gb_check(bottom, min_width, who);
    return rc ? rc : coh_check(re, im, f, who);
}

extern "C" int pgr_fan_beam_pressure_w(pgr_fan* f, const double* p0, const double* weights, const int32_t* q, double frequency,
                                       const double* bottom, const double* depths, int64_t n_depths, double min_width,
                                       int32_t curvature, double* re, double* im, void* stream)
{
    const char* who = "pgr_fan_beam_pressure_w";
    const CohOut o{q, frequency, re, im};
    return tl_fan_entry(f, p0, weights, depths, n_depths, re, who,
                        [&](int32_t) { return gbc_check(bottom, min_width, re, im, frequency, who); },
                        [&](const pgr_env* e, const TlArgs& a) {
                            return gbc_run(e, a, bottom, min_width, o, curvature, stream, who);
                        });
}

extern "C" int pgr_beam_pressure_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                          int32_t n_samples, const double* x, const double* p0, const double* weights,
                                          const int32_t* q, double frequency, const double* bottom, const double* depths,
                                          int64_t n_depths, double min_width, int32_t curvature, double* re, double* im,
                                          void* stream)
{
    const char* who = "pgr_beam_pressure_device_w";
    const CohOut o{q, frequency, re, im};
    return tl_buffer_entry<true>(env, T, z, p, n_rays, n_samples, x, p0, weights, depths, n_depths, re, who,
                                 [&](int32_t) { return gbc_check(bottom, min_width, re, im, frequency, who); },
                                 [&](const pgr_env* e, const TlArgs& a) {
                                     return gbc_run(e, a, bottom, min_width, o, curvature, stream, who);
                                 });
}

#endif  // PGR_BEAM_PHASE_H
