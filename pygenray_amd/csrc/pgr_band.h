// pgr_band.h -- the power of a fan's arrivals summed over a band of frequencies: pgr_band_power_device.
// (Part of the ONE translation unit pgr_hip.hip.  It builds on pgr_spectrum.h -- SPEC_ROWS, SPEC_TILE, SPEC_K20, spec_check -- and
// includes it itself, so pgr_hip.hip may name it anywhere behind pgr_signal.h and pgr_reflect.h; not a stand-alone header.)
//
// The quantity.  Groups, arrivals, frequencies and absorption are pgr_spectrum_device's, the lag phi (NULL:
// none) pgr_spectrum_device_phi's, and there is no reduction time: tau = T_a.  With the band weights wf[F] (finite, >= 0), for
// every group g
//   for k = 0 ... F - 1:  (re_k, im_k) = pgr_spectrum_device's sums for (g, k) with tred = 0.0 (with phi: pgr_spectrum_device_phi's)
//                         P_k = re_k * re_k + im_k * im_k
//   s_l = 0.0 for the lanes l = 0 ... 63
//   for k = l, l + 64, l + 128, ... < F in increasing k:  s_l = s_l + wf[k] * P_k
//   for d = 32, 16, 8, 4, 2, 1:  s_l = s_l + s_(l xor d)             (every lane at once; all lanes end equal)
//   out[g] = s_0
// An empty group gives +0.0; a NaN T_a, I_a or lag makes out[g] NaN; q_a < 0 adds nothing.  H itself is never stored.
//
//   pgr_band_sum  one wave per group.  The wave walks the band in tiles of SPEC_TILE frequencies, lane l owning the frequencies
//                 k0 + i * 64 + l, i = 0 ... SPEC_ROWS - 1, of a tile as in pgr_spec_sum; per tile it runs spec_sum's walk over
//                 the group's arrivals -- 64 staged at a time, the live ones (one ballot) visited in increasing a, their constants
//                 broadcast by sig_lane, freq[k] * tau formed per term -- and at the tile's end folds wf * P into the lane's s_l
//                 in increasing k.  Behind the last tile six exchanges (__shfl_xor) and lane 0's one store.  No LDS, no atomics,
//                 no barrier; repeated calls are bit-equal.  Lanes past F load clamped indices and fold nothing.  A launch of
//                 few groups and a long band is latency-bound: one wave walks all F frequencies.
#ifndef PGR_BAND_H
#define PGR_BAND_H

#include "pgr_spectrum.h"

struct BandArgs {
    const int64_t* off;       // [G + 1]
    const double* T;          // [n_arrivals]
    const double* I;          // [n_arrivals]
    const int32_t* q;         // [n_arrivals] or NULL
    const double* phi;        // [n_arrivals] or NULL
    const double* L;          // [n_arrivals] or NULL
    const double* freq;       // [nf] (device copy)
    const double* alpha;      // [nf] (device copy) or NULL, with L
    const double* wf;         // [nf] (device copy)
    int32_t nf;               // frequencies in the band
    double* out;              // [G]
};

template <bool ABSORB, bool PHI>
__device__ __forceinline__ void band_sum(const BandArgs& s)
{
    const int64_t g = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t a_begin = s.off[g], a_end = s.off[g + 1];
    double sl = 0.0;
    for (int32_t k0 = 0; k0 < s.nf; k0 += SPEC_TILE) {          // (uniform in the wave)
        double fk[SPEC_ROWS], ak[SPEC_ROWS], wk[SPEC_ROWS], re[SPEC_ROWS], im[SPEC_ROWS];
#pragma unroll
        for (int i = 0; i < SPEC_ROWS; i++) {
            const int32_t k = min(k0 + i * 64 + lane, s.nf - 1);
            fk[i] = s.freq[k];
            ak[i] = ABSORB ? s.alpha[k] : 0.0;
            wk[i] = s.wf[k];
            re[i] = 0.0;
            im[i] = 0.0;
        }
        for (int64_t a0 = a_begin; a0 < a_end; a0 += 64) {
            const int64_t a = a0 + lane;
            double tau = 0.0, amp = 0.0, qc = 0.0, La = 0.0, rc = 0.0;
            bool live = false;
            if (a < a_end) {
                const int qa = s.q ? s.q[a] : 0;
                live = qa >= 0;
                tau = s.T[a];
                amp = fsqrt(s.I[a]);
                qc = 0.25 * (double)(qa & 3);
                if (ABSORB) La = s.L[a];
                if (PHI) {
                    const double pa = s.phi[a];
                    rc = pa - rint(pa);
                }
            }
            uint64_t todo = __ballot(live);
            while (todo) {                                      // uniform in the wave: increasing a
                const int u = __builtin_ctzll(todo);
                todo &= todo - 1;
                const double tu = sig_lane(tau, u), au = sig_lane(amp, u), qu = sig_lane(qc, u);
                const double Lu = ABSORB ? sig_lane(La, u) : 0.0;
                const double ru = PHI ? sig_lane(rc, u) : 0.0;
#pragma unroll
                for (int i = 0; i < SPEC_ROWS; i++) {
                    double y = fk[i] * tu;
                    y = y - rint(y);
                    double ph = y - qu;
                    ph = ph - rint(ph);
                    if (PHI) {
                        ph = ph - ru;
                        ph = ph - rint(ph);
                    }
                    double cv, sv;
                    gcossin2pi(ph, cv, sv);
                    if (ABSORB) {
                        const double yw = -((ak[i] * Lu) * SPEC_K20);
                        const double W = yw != yw ? NAN : (yw < -700.0 ? 0.0 : gexp(yw));
                        re[i] = re[i] + (au * cv) * W;
                        im[i] = im[i] + (au * sv) * W;
                    } else {
                        re[i] = re[i] + au * cv;
                        im[i] = im[i] + au * sv;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < SPEC_ROWS; i++) {                   // the lane's frequencies of this tile, in increasing k
            if (k0 + i * 64 + lane < s.nf) {
                const double rr = re[i] * re[i], ii = im[i] * im[i];
                const double P = rr + ii;
                sl = sl + wk[i] * P;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sl = sl + __shfl_xor(sl, d, 64);
    if (lane == 0) s.out[g] = sl;
}

__global__ void __launch_bounds__(64) pgr_band_sum(BandArgs s)
{
    if (s.phi) {                                                // (both uniform in the grid)
        if (s.alpha) band_sum<true, true>(s);
        else band_sum<false, true>(s);
    } else {
        if (s.alpha) band_sum<true, false>(s);
        else band_sum<false, false>(s);
    }
}

extern "C" int pgr_band_power_device(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                                     const int32_t* q, const double* phi, const double* L, const double* freq,
                                     const double* alpha, const double* wf, int32_t n_freq, double* out, void* stream)
{
    const std::string who = "pgr_band_power_device";
    int64_t tiles = 0;
    if (spec_check(who.c_str(), offsets, n_groups, T, I, L, freq, alpha, n_freq, wf && out, &tiles)) return -1;
    for (int32_t k = 0; k < n_freq; k++)
        if (!std::isfinite(wf[k]) || wf[k] < 0.0) return fail(who + ": wf must be finite and >= 0");
    HIPCHK(hipSetDevice(device));
    const hipStream_t st = (hipStream_t)stream;
    // freq, wf and alpha in one stream-ordered allocation, freed behind the launch (as spec_run's)
    const size_t nf = (size_t)n_freq;
    std::vector<double> tab(alpha ? 3 * nf : 2 * nf);
    memcpy(tab.data(), freq, nf * sizeof(double));
    memcpy(tab.data() + nf, wf, nf * sizeof(double));
    if (alpha) memcpy(tab.data() + 2 * nf, alpha, nf * sizeof(double));
    void* b = nullptr;
    if (hipMallocAsync(&b, tab.size() * sizeof(double), st) != hipSuccess)
        return fail(who + ": device allocation of the band failed");
    const double* d_tab = (const double*)b;
    const BandArgs s{offsets, T, I, q, phi, L, d_tab, alpha ? d_tab + 2 * nf : nullptr, d_tab + nf, n_freq, out};
    hipError_t e = hipMemcpyAsync(b, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_band_sum, dim3((unsigned)n_groups), dim3(64), 0, st, s);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(who + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

#endif  // PGR_BAND_H
