// pgr_reflect.h -- the coherent sums with a real phase per arrival, the bottom's complex reflection coefficient:
// pgr_fan_pressure_phi, pgr_pressure_device_phi, pgr_signal_device_phi.  (pgr_spectrum_device_phi sits in pgr_spectrum.h, whose
// helpers it needs.)
// (Part of the ONE translation unit pgr_hip.hip, included there after pgr_signal.h; not a stand-alone header.)
//
// The quantity (include/pgr_reflection.h).  phi holds lags in cycles: per ray and save column, [S][M], for
// the tube sum -- what pgr_fan_boundary_loss accumulates from a table of lags in the bottom's slot -- and per arrival for the
// signal sum.  The arrival of tube k takes  d = Phi_k+1 - Phi_k;  d = w d;  phi_a = Phi_k + d  with its own w, and every sum's
// term is its sibling's with, behind the sibling's own  t = t - rint(t),
//   r = phi_a - rint(phi_a);  t = t - r;  t = t - rint(t).
// At r = 0 both operations leave t's bits alone: with phi all zero (or whole cycles) each kernel gives its sibling's bits.
//
// The kernels are their siblings' bodies, stated once each (pgr_coh_sum_body.h, pgr_sig_sum_body.h) and included here with the
// lag switched on: the same walk, staging, LDS and launch shape, no atomics, every output entry written.
//   pgr_coh_sum_phi   reads the tube's two lags from global memory at the visit, next to q: the wave visits tube u together, so
//                     both are one address for all lanes (broadcast loads that hit in L2 / TCP: neighbouring tubes share a line).
//                     Staging them in LDS beside T would add 512 B per wave and a store per ray for lags most visits never
//                     read -- a visit happens for the few tubes of a chunk that hold a receiver.
//   pgr_sig_sum_phi   lane l applies r where it stages arrival a0 + l, before cos / sin: nothing more is broadcast.
#ifndef PGR_REFLECT_H
#define PGR_REFLECT_H

// phi: [S][M], the rays' lag in cycles
__global__ void __launch_bounds__(64) pgr_coh_sum_phi(EnvDev env, TlArgs a, CohOut o, const double* phi)
{
#define COH_PHI 1
#include "pgr_coh_sum_body.h"
#undef COH_PHI
}

static int coh_phi_check(const double* phi, const double* re, const double* im, double f, const char* who)
{
    if (!phi) return fail(std::string(who) + ": null phi (pgr_fan_pressure_w / pgr_pressure_device_w are the entries without it)");
    return coh_check(re, im, f, who);
}

static int coh_phi_run(const pgr_env* env, const TlArgs& a, const CohOut& o, const double* phi, void* stream, const char* who)
{
    return tube_run(env, a, TL_TUBES, pgr_tl_bounds, nullptr, 0, (hipStream_t)stream, who, pgr_coh_sum_phi, o, phi);
}

extern "C" int pgr_fan_pressure_phi(pgr_fan* f, const double* p0, const double* weights, const int32_t* q, const double* phi,
                                    double frequency, const double* depths, int64_t n_depths, double* re, double* im,
                                    void* stream)
{
    const char* who = "pgr_fan_pressure_phi";
    const CohOut o{q, frequency, re, im};
    return tl_fan_entry(f, p0, weights, depths, n_depths, re, who,
                        [&](int32_t) { return coh_phi_check(phi, re, im, frequency, who); },
                        [&](const pgr_env* e, const TlArgs& a) { return coh_phi_run(e, a, o, phi, stream, who); });
}

extern "C" int pgr_pressure_device_phi(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                       int32_t n_samples, const double* x, const double* p0, const double* weights,
                                       const int32_t* q, const double* phi, double frequency, const double* depths,
                                       int64_t n_depths, double* re, double* im, void* stream)
{
    const char* who = "pgr_pressure_device_phi";
    const CohOut o{q, frequency, re, im};
    return tl_buffer_entry<true>(env, T, z, p, n_rays, n_samples, x, p0, weights, depths, n_depths, re, who,
                                 [&](int32_t) { return coh_phi_check(phi, re, im, frequency, who); },
                                 [&](const pgr_env* e, const TlArgs& a) { return coh_phi_run(e, a, o, phi, stream, who); });
}

// phi: [n_arrivals], every arrival's lag in cycles
__global__ void __launch_bounds__(64) pgr_sig_sum_phi(SigArgs s, const double* phi)
{
#define SIG_PHI 1
#include "pgr_sig_sum_body.h"
#undef SIG_PHI
}

extern "C" int pgr_signal_device_phi(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                                     const int32_t* q, const double* phi, const double* tstart, double frequency,
                                     double inv_sigma, double dt, int32_t n_times, double* re, double* im, void* stream)
{
    const char* who = "pgr_signal_device_phi";
    if (!phi) return fail(std::string(who) + ": null phi (pgr_signal_device is the entry without it)");
    return sig_run(who, device, offsets, n_groups, T, I, q, tstart, frequency, inv_sigma, dt, n_times, re, im, stream,
                   pgr_sig_sum_phi, phi);
}

#endif  // PGR_REFLECT_H
