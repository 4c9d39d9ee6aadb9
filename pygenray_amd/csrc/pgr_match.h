// pgr_match.h -- matched-field processing, the Bartlett ambiguity surface from the elements' arrival lists: pgr_matched_field_device.
// (Part of the ONE translation unit pgr_hip.hip.  It builds on pgr_spectrum.h -- SPEC_ROWS, SPEC_TILE, SPEC_K20, spec_check -- and
// includes it itself, so pgr_hip.hip may name it anywhere behind pgr_signal.h and pgr_reflect.h; not a stand-alone header.)
//
// The quantity.  N elements and G cells; the arrival lists of the N * G groups stand element-major, group
// e = j * G + g, so off[N * G + 1].  Arrivals, frequencies and absorption are pgr_spectrum_device's, the lag phi (NULL: none)
// pgr_spectrum_device_phi's, and there is no reduction time: tau = T_a.  With the band weights wf[F] (finite, >= 0), the data
// dr[N * F], di[N * F] indexed [j][k] (finite) and the flag `normalize`, for every cell g
//   for k = 0 ... F - 1:
//       cr = ci = nn = 0.0
//       for j = 0 ... N - 1 in increasing j:
//           (re, im) = pgr_spectrum_device's sums for group (j * G + g, k) with tred = 0.0 (with phi: pgr_spectrum_device_phi's)
//           cr = cr + (re * dr[j][k] + im * di[j][k])          conj(H) d: real part
//           ci = ci + (re * di[j][k] - im * dr[j][k])                     imaginary part
//           nn = nn + (re * re + im * im)
//       A = cr * cr + ci * ci
//       B_k = A without normalize;  with it  nn == 0.0 ? 0.0 : A / nn      (IEEE division; a NaN nn gives NaN)
//   s_l = 0.0 for the lanes l = 0 ... 63
//   for k = l, l + 64, l + 128, ... < F in increasing k:  s_l = s_l + wf[k] * B_k
//   for d = 32, 16, 8, 4, 2, 1:  s_l = s_l + s_(l xor d)             (every lane at once; all lanes end equal)
//   out[g] = s_0
// A cell no element reaches gives +0.0; a NaN T_a, I_a or lag in one of a cell's lists makes that cell NaN and no other; q_a < 0
// adds nothing.  No replica H_j is ever stored.
//
//   pgr_mfp_sum  one wave per cell.  The wave walks the band in tiles of SPEC_TILE frequencies, lane l owning the frequencies
//                k0 + i * 64 + l, i = 0 ... SPEC_ROWS - 1, of a tile as in pgr_band_sum; per tile an outer loop over the elements
//                j runs spec_sum's walk over the arrivals of group (j, g) -- 64 staged at a time, the live ones (one ballot)
//                visited in increasing a, their constants broadcast by sig_lane, freq[k] * tau formed per term -- and folds the
//                walk's (re, im) with d[j][k] (loaded coalesced: consecutive lanes, consecutive k) into the lane's cr, ci and nn.
//                At the tile's end the lane folds wf * B into its s_l in increasing k; behind the last tile six exchanges
//                (__shfl_xor) and lane 0's one store.  No LDS, no atomics, no barrier; repeated calls are bit-equal.  Lanes past
//                F load clamped indices and fold nothing.  ABSORB, PHI and NORMALIZE are template choices, uniform in the grid.
//                The walk over the elements is serial in a wave: a cell costs the N spec_sum walks it replaces, without their
//                stores.
#ifndef PGR_MATCH_H
#define PGR_MATCH_H

#include "pgr_spectrum.h"

// (the band and the data travel as ONE table, so that the wave holds one base address for all of them:
//  tab = freq[nf] | wf[nf] | alpha[nf] (with L only) | then per element j its two rows dr[j][nf] | di[j][nf])
struct MatchArgs {
    const int64_t* off;       // [N * G + 1]
    const double* T;          // [n_arrivals]
    const double* I;          // [n_arrivals]
    const int32_t* q;         // [n_arrivals] or NULL
    const double* phi;        // [n_arrivals] or NULL
    const double* L;          // [n_arrivals] or NULL, with alpha in the table
    const double* tab;        // the table above (device copy)
    double* out;              // [G]
    int32_t nf;               // frequencies in the band
    int32_t ne;               // elements N
    int32_t nc;               // cells G (N * G <= INT32_MAX)
    int32_t normalize;        // 0 or 1
};

// A wave-uniform address kept in the lane's VGPRs instead of the wave's SGPRs.  spec_sum's walk with the loop over the elements
// around it leaves no SGPR to spare (pgr_band_sum stands at the limit already), and the VGPRs have room up to 128 at the same
// occupancy.  What is used once per element and tile, not per arrival, lives there: the cell's place in the offsets, the table,
// the output's address.
template <typename P>
__device__ __forceinline__ P* mfp_lane_address(P* p)
{
    uint64_t v = (uint64_t)p;
    asm volatile("" : "+v"(v));
    return (P*)v;
}

template <bool ABSORB, bool PHI, bool NORMALIZE>
__device__ __forceinline__ void mfp_sum(const MatchArgs& s)
{
    const int lane = threadIdx.x;
    const int64_t* og_off = mfp_lane_address(s.off + blockIdx.x);       // the offsets of group (0, g)
    const double* tab = mfp_lane_address(s.tab);
    double* og_out = mfp_lane_address(s.out + blockIdx.x);
    double sl = 0.0;
    for (int32_t k0 = 0; k0 < s.nf; k0 += SPEC_TILE) {          // (uniform in the wave)
        double fk[SPEC_ROWS], ak[SPEC_ROWS], cr[SPEC_ROWS], ci[SPEC_ROWS], nn[SPEC_ROWS];
#define MFP_K(i) min(k0 + (i) * 64 + lane, s.nf - 1)             /* the lane's i-th frequency of the tile, clamped */
#pragma unroll
        for (int i = 0; i < SPEC_ROWS; i++) {
            fk[i] = tab[MFP_K(i)];
            ak[i] = ABSORB ? tab[2 * (int64_t)s.nf + MFP_K(i)] : 0.0;
            cr[i] = 0.0;
            ci[i] = 0.0;
            nn[i] = 0.0;
        }
        const int64_t* oj = og_off;                             // group (j, g): nc further per element
        const double* dj = tab + (ABSORB ? 3 : 2) * (int64_t)s.nf;   // the data of element j: 2 nf further per element
        for (int32_t left = s.ne; left > 0; left--, oj += s.nc, dj += 2 * (int64_t)s.nf) {   // the elements, in increasing j
            // (the walk's place and end in VGPRs too, every lane holding its own a: a0 + lane)
            const int64_t a_end = oj[1];
            int64_t a = oj[0] + lane;
            double re[SPEC_ROWS], im[SPEC_ROWS];
#pragma unroll
            for (int i = 0; i < SPEC_ROWS; i++) {
                re[i] = 0.0;
                im[i] = 0.0;
            }
            for (; __any(a < a_end); a += 64) {                 // (uniform in the wave: lane 0's a is the block's a0)
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
                while (todo) {                                  // uniform in the wave: increasing a
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
            for (int i = 0; i < SPEC_ROWS; i++) {               // conj(H_j) d_j, and |H_j|^2
                const double xr = dj[MFP_K(i)], xi = dj[(int64_t)s.nf + MFP_K(i)];
                const double rr = re[i] * xr, ii = im[i] * xi;
                const double ri = re[i] * xi, ir = im[i] * xr;
                const double tr = rr + ii, ti = ri - ir;
                cr[i] = cr[i] + tr;
                ci[i] = ci[i] + ti;
                if (NORMALIZE) {
                    const double r2 = re[i] * re[i], i2 = im[i] * im[i];
                    const double p2 = r2 + i2;
                    nn[i] = nn[i] + p2;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < SPEC_ROWS; i++) {                   // the lane's frequencies of this tile, in increasing k
            if (k0 + i * 64 + lane < s.nf) {
                const double c2 = cr[i] * cr[i], s2 = ci[i] * ci[i];
                const double A = c2 + s2;
                double B = A;
                if (NORMALIZE) B = nn[i] == 0.0 ? 0.0 : A / nn[i];
                sl = sl + tab[(int64_t)s.nf + MFP_K(i)] * B;
            }
        }
    }
#undef MFP_K
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sl = sl + __shfl_xor(sl, d, 64);
    if (lane == 0) *og_out = sl;
}

template <bool ABSORB, bool PHI>
__device__ __forceinline__ void mfp_pick(const MatchArgs& s, bool normalize)
{
    if (normalize) mfp_sum<ABSORB, PHI, true>(s);
    else mfp_sum<ABSORB, PHI, false>(s);
}

__global__ void __launch_bounds__(64) pgr_mfp_sum(MatchArgs s)
{
    if (s.phi) {                                                // (all three uniform in the grid)
        if (s.L) mfp_pick<true, true>(s, s.normalize != 0);
        else mfp_pick<false, true>(s, s.normalize != 0);
    } else {
        if (s.L) mfp_pick<true, false>(s, s.normalize != 0);
        else mfp_pick<false, false>(s, s.normalize != 0);
    }
}

extern "C" int pgr_matched_field_device(int device, const int64_t* offsets, int32_t n_elements, int64_t n_cells, const double* T,
                                        const double* I, const int32_t* q, const double* phi, const double* L, const double* freq,
                                        const double* alpha, const double* wf, const double* d_re, const double* d_im,
                                        int32_t n_freq, int normalize, double* out, void* stream)
{
    const std::string who = "pgr_matched_field_device";
    if (n_elements < 1) return fail(who + ": n_elements must be >= 1");
    if (n_cells < 1) return fail(who + ": n_cells must be >= 1");
    if (n_cells > INT32_MAX / (int64_t)n_elements) return fail(who + ": too many groups (n_elements * n_cells)");
    if (normalize != 0 && normalize != 1) return fail(who + ": normalize must be 0 or 1");
    int64_t tiles = 0;
    if (spec_check(who.c_str(), offsets, (int64_t)n_elements * n_cells, T, I, L, freq, alpha, n_freq, wf && d_re && d_im && out,
                   &tiles))
        return -1;
    const size_t nf = (size_t)n_freq, nd = (size_t)n_elements * nf;
    for (size_t k = 0; k < nf; k++)
        if (!std::isfinite(wf[k]) || wf[k] < 0.0) return fail(who + ": wf must be finite and >= 0");
    for (size_t k = 0; k < nd; k++)
        if (!std::isfinite(d_re[k]) || !std::isfinite(d_im[k])) return fail(who + ": the data d_re, d_im must be finite");
    HIPCHK(hipSetDevice(device));
    const hipStream_t st = (hipStream_t)stream;
    // freq, wf, alpha and the data in one stream-ordered allocation, freed behind the launch (as pgr_band_power_device's)
    const size_t na = alpha ? nf : 0;
    std::vector<double> tab(2 * nf + na + 2 * nd);
    memcpy(tab.data(), freq, nf * sizeof(double));
    memcpy(tab.data() + nf, wf, nf * sizeof(double));
    if (alpha) memcpy(tab.data() + 2 * nf, alpha, nf * sizeof(double));
    for (size_t j = 0; j < (size_t)n_elements; j++) {               // per element its row of d_re, then its row of d_im
        memcpy(tab.data() + 2 * nf + na + 2 * j * nf, d_re + j * nf, nf * sizeof(double));
        memcpy(tab.data() + 2 * nf + na + (2 * j + 1) * nf, d_im + j * nf, nf * sizeof(double));
    }
    void* b = nullptr;
    if (hipMallocAsync(&b, tab.size() * sizeof(double), st) != hipSuccess)
        return fail(who + ": device allocation of the band and the data failed");
    const MatchArgs s{offsets, T, I, q, phi, L, (const double*)b, out, n_freq, n_elements, (int32_t)n_cells, normalize};
    hipError_t e = hipMemcpyAsync(b, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_mfp_sum, dim3((unsigned)n_cells), dim3(64), 0, st, s);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(who + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

#endif  // PGR_MATCH_H
