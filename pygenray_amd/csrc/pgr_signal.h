// pgr_signal.h -- the received time series of a Gaussian pulse from a fan's ray-tube arrivals: pgr_signal_device.
// (Part of the ONE translation unit pgr_hip.hip, included there last; not a stand-alone header.)
//
// The quantity.  Arrivals come in groups, in pgr_fan_arrivals' order: arrival a of group g lies in
// [off[g], off[g + 1]), in increasing tube order, with its travel time T_a, its intensity I_a (the weighted term of the TL
// sum) and its phase index q_a in quarter cycles (int32; < 0: the arrival adds nothing; NULL: all zero).  With the centre
// frequency f, rs = 1 / sigma of the Gaussian envelope (0: the CW limit), the sample spacing dt and the group's start time,
//   t_n = tstart[g] + (double)n * dt                                     (not contracted in either build)
//   re = im = 0.0;  for a = off[g] ... off[g + 1] - 1 in order:
//       if q_a < 0: continue
//       x = (t_n - T_a) * rs;  v = x * x;  if !(v <= 64.0): continue     (cut at 8 sigma; a NaN T_a adds nothing)
//       amp = fsqrt(I_a);  y = f * T_a;  y = y - rint(y);  ph = y - 0.25 * (q_a & 3);  ph = ph - rint(ph)
//       (cv, sv) = gcossin2pi(ph);  E = gexp(-0.5 * v)
//       re = re + (amp * cv) * E;  im = im + (amp * sv) * E
//   u[g][n] = re + i im                                                  the complex baseband signal
// At rs = 0 every term has v = 0 and E = gexp(-0.0) = 1.0 exactly: u[g][n] is pgr_coh_sum's value, bit for bit in the
// reference build.
//
//   pgr_sig_sum   one wave per (group, tile of SIG_TILE samples).  Lane l owns the samples n0 + i * 64 + l, i = 0 ...
//                 SIG_ROWS - 1: consecutive lanes hold consecutive n, so the stores are coalesced and an arrival's constants
//                 serve SIG_ROWS samples.  The group's arrivals are staged 64 at a time: lane l loads arrival a0 + l and forms
//                 T, amp cv and amp sv once.  The staged arrivals that can reach the tile (one ballot) are then visited in
//                 increasing a, their three constants broadcast by v_readlane: each sample's sum is the definition's
//                 sequential sum.  No atomics, no LDS.
// The wave-level skip.  t_n is non-decreasing in n (every operation of it is monotone), so tA = t_n0 and tB = t_last bound
// the tile's times exactly.  For T_a < tA every sample has t_n - T_a >= tA - T_a > 0, and subtraction, the product with
// rs >= 0 and the square are monotone there: v_n >= vA = ((tA - T_a) rs)^2, formed by the per-sample test's own operations.
// So vA > 64 means no sample of the tile keeps the arrival; likewise vB on the other side.  An arrival with tA <= T_a <= tB is
// always visited.  Never stricter than the per-sample test (as GB_REACH, section 10, but with no slack needed), and at rs = 0
// (x = 0 for a finite T_a) nothing is skipped.
#ifndef PGR_SIGNAL_H
#define PGR_SIGNAL_H

#define SIG_ROWS 4                    // samples per lane
#define SIG_TILE (64 * SIG_ROWS)      // samples per wave

struct SigArgs {
    const int64_t* off;       // [G + 1]
    const double* T;          // [n_arrivals]
    const double* I;          // [n_arrivals]
    const int32_t* q;         // [n_arrivals] or NULL
    const double* tstart;     // [G]
    double f, rs, dt;
    int32_t nt;               // samples per group
    double* re;               // [G][nt]
    double* im;               // [G][nt]
};

// t_n, the same bits in both builds and wherever it is formed
__device__ __forceinline__ double sig_time(double t0, int32_t n, double dt)
{
#pragma clang fp contract(off)
    const double e = (double)n * dt;
    return t0 + e;
}

// lane u's value in every lane (u uniform in the wave)
__device__ __forceinline__ double sig_lane(double v, int u)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), u);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), u);
    return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(64) pgr_sig_sum(SigArgs s)
{
#define SIG_PHI 0
#include "pgr_sig_sum_body.h"
#undef SIG_PHI
}

// the checks of every sum over arrival lists at time samples (the entries here and pgr_array_response_device) -> 0 and
// `tiles`, the tiles of SIG_TILE samples, or the failure
static int sig_check(const char* who, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                     const double* tstart, double frequency, double inv_sigma, double dt, int32_t n_times, const double* re,
                     const double* im, int64_t* n_tiles)
{
    if (!offsets || !T || !I || !tstart || !re || !im) return fail(std::string(who) + ": null argument");
    if (n_groups < 1) return fail(std::string(who) + ": n_groups must be >= 1");
    if (n_groups > INT32_MAX) return fail(std::string(who) + ": too many groups");
    if (n_times < 1) return fail(std::string(who) + ": n_times must be >= 1");
    const int64_t tiles = ((int64_t)n_times + SIG_TILE - 1) / SIG_TILE;
    if (tiles > 65535) return fail(std::string(who) + ": n_times must be <= " + std::to_string(65535 * SIG_TILE));
    if (!std::isfinite(frequency) || frequency < 0.0) return fail(std::string(who) + ": frequency must be finite and >= 0");
    if (!std::isfinite(inv_sigma) || inv_sigma < 0.0) return fail(std::string(who) + ": inv_sigma must be finite and >= 0");
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(std::string(who) + ": dt must be finite and > 0");
    *n_tiles = tiles;
    return 0;
}

// both entries: the checks, then `sum` (pgr_sig_sum, or with phi pgr_sig_sum_phi) over (group, tile of samples)
template <typename... Extra>
static int sig_run(const char* who, int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                   const int32_t* q, const double* tstart, double frequency, double inv_sigma, double dt, int32_t n_times,
                   double* re, double* im, void* stream, void (*sum)(SigArgs, Extra...), Extra... extra)
{
    int64_t tiles = 0;
    if (sig_check(who, offsets, n_groups, T, I, tstart, frequency, inv_sigma, dt, n_times, re, im, &tiles)) return -1;
    HIPCHK(hipSetDevice(device));
    const SigArgs s{offsets, T, I, q, tstart, frequency, inv_sigma, dt, n_times, re, im};
    hipLaunchKernelGGL(sum, dim3((unsigned)n_groups, (unsigned)tiles), dim3(64), 0, (hipStream_t)stream, s, extra...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

extern "C" int pgr_signal_device(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                                 const int32_t* q, const double* tstart, double frequency, double inv_sigma, double dt,
                                 int32_t n_times, double* re, double* im, void* stream)
{
    return sig_run("pgr_signal_device", device, offsets, n_groups, T, I, q, tstart, frequency, inv_sigma, dt, n_times, re, im,
                   stream, pgr_sig_sum);
}

#endif  // PGR_SIGNAL_H
