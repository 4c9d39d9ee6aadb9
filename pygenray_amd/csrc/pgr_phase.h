// pgr_phase.h -- the phase of a fan's ray tubes and their coherent sum: the caustic index of every tube at every save range
// (pgr_fan_caustic_index, pgr_caustic_index_device) and the complex pressure of the tubes at receiver depths
// (pgr_fan_pressure_w, pgr_pressure_device_w).
// (Part of the ONE translation unit pgr_hip.hip, included there last; not a stand-alone header.)
//
// The quantities.  Tube k is the surviving rays k, k + 1 in launch order, d = zsign Z their depths, and
// nb / ns [S][M] the per-sample bounce counts pgr_fan_boundary_loss writes (NULL: all zero).
//   valid(s): d_k(s), d_k+1(s) not NaN, d_k+1(s) != d_k(s), nb_k(s) == nb_k+1(s), ns_k(s) == ns_k+1(s)
//   u(s) = sign(d_k+1(s) - d_k(s)) (-1)^(nb_k(s) + ns_k(s))           the tube's width with the mirror flips undone
//   kappa[s][k] = the number of times u changed between consecutive valid samples up to s;  kappa[s][M - 1] = 0.
// A tube folded over a boundary (the counts differ) is skipped and carries its last sign, as a NaN sample does.
//   pgr_caustic_scan  one lane per tube (a wave reads 64 consecutive rays of a row and the next one by a second load), the
//                     loop over s sequential as in pgr_path_scan.  Integer output, one lane owns each tube: no atomics.
//
// The coherent sum: receiver j at column s gets, over exactly the tubes pgr_tl_sum adds there that also have q[s][k] >= 0
// (q: a phase index in quarter cycles, NULL: all zero), in increasing k from 0.0,
//   w = (D_j - d_k) / (d_k+1 - d_k),  T = T_k + w (T_k+1 - T_k)       the arrival's bits (pgr_arrivals.h)
//   a = sqrt(I_k)                                                     I_k: the (weighted) term of the TL sum, the same bits
//   y = f T;  y = y - rint(y);  t = y - 0.25 (q & 3);  t = t - rint(t)
//   re += a gcos2pi(t),  im += a gsin2pi(t)                           p = sum a exp(i (2 pi f T - (pi / 2) q))
//   pgr_coh_sum       pgr_tl_sum's walk (tl_walk with the rays' T in LDS) after pgr_tl_bounds: one wave per (column, band of 64
//                     receivers), each receiver's two sums formed by one lane in tube order.
#ifndef PGR_PHASE_H
#define PGR_PHASE_H

struct CausticArgs {
    TlArgs t;                 // the fan as pgr_tl.h reads it (Z, keep, N, M, S, blocked, zsign); the rest unused
    const int32_t* nb;        // [S][M] or NULL
    const int32_t* ns;        // [S][M] or NULL
    int32_t* kappa;           // [S][M]
};

__global__ void __launch_bounds__(64) pgr_caustic_scan(CausticArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= a.t.M) return;
    const bool tube = k + 1 < a.t.M;                 // (the last ray bounds no tube: its entries are 0)
    int sig = 0, n = 0;
#pragma unroll 4
    for (int s = 0; s < a.t.S; s++) {
        const int64_t o = (int64_t)s * a.t.M + k;
        if (tube) {
            const double d0 = a.t.zsign * a.t.Z[tl_index(a.t, s, k)], d1 = a.t.zsign * a.t.Z[tl_index(a.t, s, k + 1)];
            const int b0 = a.nb ? a.nb[o] : 0, b1 = a.nb ? a.nb[o + 1] : 0;
            const int s0 = a.ns ? a.ns[o] : 0, s1 = a.ns ? a.ns[o + 1] : 0;
            if (d0 == d0 && d1 == d1 && d1 != d0 && b0 == b1 && s0 == s1) {
                const int u = ((d1 > d0) != (((b0 + s0) & 1) != 0)) ? 1 : -1;
                if (sig != 0 && u != sig) n++;
                sig = u;
            }
        }
        a.kappa[o] = n;
    }
}

// the checks of both caustic entries, before any device work
static int caustic_check(int64_t M, int32_t S, const void* kappa, const char* who)
{
    if (!kappa) return fail(std::string(who) + ": null argument");
    if (M < 2) return fail(std::string(who) + ": need at least two rays (one ray tube)");
    if (M > INT32_MAX) return fail(std::string(who) + ": too many rays");
    if (S < 1) return fail(std::string(who) + ": n_samples must be >= 1");
    return 0;
}

static int caustic_run(TlArgs t, const int32_t* nb, const int32_t* ns, int32_t* kappa, void* stream, const char* who)
{
    const CausticArgs a{t, nb, ns, kappa};
    hipLaunchKernelGGL(pgr_caustic_scan, dim3((unsigned)((t.M + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

extern "C" int pgr_fan_caustic_index(pgr_fan* f, const int32_t* nb, const int32_t* ns, int32_t* kappa, void* stream)
{
    const char* who = "pgr_fan_caustic_index";
    return fan_entry(f, who, [&](int64_t M, int32_t S) { return caustic_check(M, S, kappa, who); },
                     [&](const pgr_env*, TlArgs t) { return caustic_run(t, nb, ns, kappa, stream, who); });
}

extern "C" int pgr_caustic_index_device(int device, const double* z, int64_t n_rays, int32_t n_samples, const int32_t* nb,
                                        const int32_t* ns, int32_t* kappa, void* stream)
{
    const char* who = "pgr_caustic_index_device";
    if (!z) return fail(std::string(who) + ": null argument");
    const int rc = caustic_check(n_rays, n_samples, kappa, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    TlArgs t{};
    t.Z = z; t.keep = nullptr;
    t.N = n_rays; t.M = n_rays; t.S = n_samples; t.blocked = 0;
    t.zsign = -1.0;
    return caustic_run(t, nb, ns, kappa, stream, who);
}

// ---- the coherent tube sum ----

struct CohOut {
    const int32_t* q;         // [S][M] phase index of tube k in quarter cycles, < 0: the tube adds nothing; NULL: all zero
    double f;                 // frequency, Hz
    double* re;               // [R][S]
    double* im;               // [R][S]
};

__global__ void __launch_bounds__(64) pgr_coh_sum(EnvDev env, TlArgs a, CohOut o)
{
#define COH_PHI 0
#include "pgr_coh_sum_body.h"
#undef COH_PHI
}

static int coh_check(const double* re, const double* im, double f, const char* who)
{
    if (!re || !im) return fail(std::string(who) + ": null argument");
    if (!std::isfinite(f) || f < 0.0) return fail(std::string(who) + ": frequency must be finite and >= 0");
    return 0;
}

static int coh_run(const pgr_env* env, const TlArgs& a, const CohOut& o, void* stream, const char* who)
{
    return tube_run(env, a, TL_TUBES, pgr_tl_bounds, nullptr, 0, (hipStream_t)stream, who, pgr_coh_sum, o);
}

extern "C" int pgr_fan_pressure_w(pgr_fan* f, const double* p0, const double* weights, const int32_t* q, double frequency,
                                  const double* depths, int64_t n_depths, double* re, double* im, void* stream)
{
    const char* who = "pgr_fan_pressure_w";
    const CohOut o{q, frequency, re, im};
    return tl_fan_entry(f, p0, weights, depths, n_depths, re, who, [&](int32_t) { return coh_check(re, im, frequency, who); },
                        [&](const pgr_env* e, const TlArgs& a) { return coh_run(e, a, o, stream, who); });
}

extern "C" int pgr_pressure_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                     int32_t n_samples, const double* x, const double* p0, const double* weights,
                                     const int32_t* q, double frequency, const double* depths, int64_t n_depths, double* re,
                                     double* im, void* stream)
{
    const char* who = "pgr_pressure_device_w";
    const CohOut o{q, frequency, re, im};
    return tl_buffer_entry<true>(env, T, z, p, n_rays, n_samples, x, p0, weights, depths, n_depths, re, who,
                                 [&](int32_t) { return coh_check(re, im, frequency, who); },
                                 [&](const pgr_env* e, const TlArgs& a) { return coh_run(e, a, o, stream, who); });
}

#endif  // PGR_PHASE_H
