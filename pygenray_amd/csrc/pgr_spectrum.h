// pgr_spectrum.h -- the transfer function of a fan's ray-tube arrivals over a band of frequencies: pgr_spectrum_device.
// (Part of the ONE translation unit pgr_hip.hip, named there last and first included by pgr_band.h, which builds on it; not a
// stand-alone header.)
//
// The quantity.  Groups and arrivals are section 17's: arrival a of group g lies in
// [off[g], off[g + 1]), in increasing tube order, with its travel time T_a, its intensity I_a and its phase index q_a in
// quarter cycles (int32; < 0: the arrival adds nothing; NULL: all zero), and now its path length L_a in metres (NULL: none).
// With the frequencies freq[F] in Hz, the absorption alpha[F] in dB per metre (given exactly when L is) and a reduction time
// per group, for every group g and frequency index k
//   re = im = 0.0;  for a = off[g] ... off[g + 1] - 1 in order:
//       if q_a < 0: continue
//       tau = T_a - tred[g]
//       amp = fsqrt(I_a);  y = freq[k] * tau;  y = y - rint(y);  ph = y - 0.25 * (q_a & 3);  ph = ph - rint(ph)
//       (cv, sv) = gcossin2pi(ph)
//       without alpha:  re = re + amp * cv;          im = im + amp * sv
//       with alpha:     yw = -((alpha[k] * L_a) * K20);  W = yw != yw ? NaN : (yw < -700.0 ? 0.0 : gexp(yw))
//                       re = re + (amp * cv) * W;    im = im + (amp * sv) * W
//   H[g][k] = re + i im
// K20 = 0.5 * PATH_LN10_10 (exact: the double nearest ln 10 / 20), the amplitude twin of pgr_path_weight's weight.  Nothing
// is filtered but q_a < 0: a NaN T_a or I_a makes the group's entries NaN by IEEE rules, as in pgr_coh_sum.  With
// tred[g] == 0.0 tau is T_a exactly and, without alpha, the operations are pgr_coh_sum's own in its order: H[g][k] is
// pgr_fan_pressure_w's value at (j, column) for freq[k], bit for bit in the reference build.
//
//   pgr_spec_sum  one wave per (group, tile of SPEC_TILE frequencies), pgr_sig_sum's layout.  Lane l owns the frequencies
//                 k0 + i * 64 + l, i = 0 ... SPEC_ROWS - 1: consecutive lanes hold consecutive k, so every store is 512
//                 contiguous bytes and an arrival's constants serve SPEC_ROWS frequencies.  The group's arrivals are staged
//                 64 at a time: lane l loads arrival a0 + l (T, I, q, L: coalesced) and forms tau, amp and 0.25 (q & 3)
//                 once.  The staged arrivals with q >= 0 (one ballot) are visited in increasing a, their constants broadcast
//                 by v_readlane (sig_lane): each (g, k) sum is the definition's sequential sum.  No atomics, no LDS, no
//                 barrier; repeated calls are bit-equal.  The product freq[k] * tau is formed per term -- no phase recurrence
//                 across k, which would lose the bit identity with pgr_coh_sum.
#ifndef PGR_SPECTRUM_H
#define PGR_SPECTRUM_H

#define SPEC_ROWS 4                    // frequencies per lane
#define SPEC_TILE (64 * SPEC_ROWS)     // frequencies per wave
#define SPEC_K20 (0.5 * PATH_LN10_10)  // the double nearest ln(10) / 20

struct SpecArgs {
    const int64_t* off;       // [G + 1]
    const double* T;          // [n_arrivals]
    const double* I;          // [n_arrivals]
    const int32_t* q;         // [n_arrivals] or NULL
    const double* L;          // [n_arrivals] or NULL
    const double* tred;       // [G]
    const double* freq;       // [nf] (device copy)
    const double* alpha;      // [nf] (device copy) or NULL, with L
    int32_t nf;               // frequencies per group
    double* re;               // [G][nf]
    double* im;               // [G][nf]
};

// PHI (pgr_spec_sum_phi): every arrival is turned back by its lag phi[a] in cycles, whose r = phi - rint(phi)
// lane l forms where it stages the arrival and sig_lane broadcasts with the other constants; without it the instructions are
// pgr_spec_sum's as they ever were.
template <bool ABSORB, bool PHI>
__device__ __forceinline__ void spec_sum(const SpecArgs& s, const double* phi)
{
    const int64_t g = blockIdx.x;
    const int32_t k0 = (int32_t)blockIdx.y * SPEC_TILE;         // (k0 < nf: the grid has ceil(nf / SPEC_TILE) tiles)
    const int lane = threadIdx.x;
    const int64_t a_end = s.off[g + 1];
    const double t0 = s.tred[g];
    double fk[SPEC_ROWS], ak[SPEC_ROWS], re[SPEC_ROWS], im[SPEC_ROWS];
#pragma unroll
    for (int i = 0; i < SPEC_ROWS; i++) {
        const int32_t k = min(k0 + i * 64 + lane, s.nf - 1);
        fk[i] = s.freq[k];
        ak[i] = ABSORB ? s.alpha[k] : 0.0;
        re[i] = 0.0;
        im[i] = 0.0;
    }
    for (int64_t a0 = s.off[g]; a0 < a_end; a0 += 64) {
        const int64_t a = a0 + lane;
        double tau = 0.0, amp = 0.0, qc = 0.0, La = 0.0, rc = 0.0;
        bool live = false;
        if (a < a_end) {
            const int qa = s.q ? s.q[a] : 0;
            live = qa >= 0;
            tau = s.T[a] - t0;
            amp = fsqrt(s.I[a]);
            qc = 0.25 * (double)(qa & 3);
            if (ABSORB) La = s.L[a];
            if (PHI) {
                const double pa = phi[a];
                rc = pa - rint(pa);
            }
        }
        uint64_t todo = __ballot(live);
        while (todo) {                                          // uniform in the wave: increasing a
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
    for (int i = 0; i < SPEC_ROWS; i++) {
        const int32_t k = k0 + i * 64 + lane;
        if (k < s.nf) {
            s.re[g * s.nf + k] = re[i];
            s.im[g * s.nf + k] = im[i];
        }
    }
}

__global__ void __launch_bounds__(64) pgr_spec_sum(SpecArgs s)
{
    if (s.alpha) spec_sum<true, false>(s, nullptr);             // (uniform in the grid)
    else spec_sum<false, false>(s, nullptr);
}

// pgr_spectrum_device_phi's sum (include/pgr_reflection.h)
__global__ void __launch_bounds__(64) pgr_spec_sum_phi(SpecArgs s, const double* phi)
{
    if (s.alpha) spec_sum<true, true>(s, phi);                  // (uniform in the grid)
    else spec_sum<false, true>(s, phi);
}

// what every entry over a band refuses of the arrival lists and the band (`outputs`: whether its other required pointers are
// all there), before any device work -> 0 with the number of tiles in *tiles, or fail()'s -1
static int spec_check(const char* who, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                      const double* L, const double* freq, const double* alpha, int32_t n_freq, bool outputs, int64_t* tiles)
{
    if (!offsets || !T || !I || !freq || !outputs) return fail(std::string(who) + ": null argument");
    if ((L != nullptr) != (alpha != nullptr))
        return fail(std::string(who) + ": L (the arrivals' path lengths) and alpha go together: give both or neither");
    if (n_groups < 1) return fail(std::string(who) + ": n_groups must be >= 1");
    if (n_groups > INT32_MAX) return fail(std::string(who) + ": too many groups");
    if (n_freq < 1) return fail(std::string(who) + ": n_freq must be >= 1");
    *tiles = ((int64_t)n_freq + SPEC_TILE - 1) / SPEC_TILE;
    if (*tiles > 65535) return fail(std::string(who) + ": n_freq must be <= " + std::to_string(65535 * SPEC_TILE));
    for (int32_t k = 0; k < n_freq; k++) {
        if (!std::isfinite(freq[k]) || freq[k] < 0.0) return fail(std::string(who) + ": freq must be finite and >= 0");
        if (alpha && (!std::isfinite(alpha[k]) || alpha[k] < 0.0)) return fail(std::string(who) + ": alpha must be finite and >= 0");
    }
    return 0;
}

// both entries: the checks, the frequencies' device copy, then `sum` (pgr_spec_sum, or with phi pgr_spec_sum_phi) over (group,
// tile of frequencies)
template <typename... Extra>
static int spec_run(const char* who, int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                    const int32_t* q, const double* L, const double* tred, const double* freq, const double* alpha,
                    int32_t n_freq, double* re, double* im, void* stream, void (*sum)(SpecArgs, Extra...), Extra... extra)
{
    int64_t tiles = 0;
    if (spec_check(who, offsets, n_groups, T, I, L, freq, alpha, n_freq, tred && re && im, &tiles)) return -1;
    HIPCHK(hipSetDevice(device));
    const hipStream_t st = (hipStream_t)stream;
    // freq and alpha in one stream-ordered allocation, freed behind the launch (as pgr_path.h's profile)
    const size_t nf = (size_t)n_freq;
    std::vector<double> tab(alpha ? 2 * nf : nf);
    memcpy(tab.data(), freq, nf * sizeof(double));
    if (alpha) memcpy(tab.data() + nf, alpha, nf * sizeof(double));
    void* b = nullptr;
    if (hipMallocAsync(&b, tab.size() * sizeof(double), st) != hipSuccess)
        return fail(std::string(who) + ": device allocation of the frequencies failed");
    const double* d_freq = (const double*)b;
    const SpecArgs s{offsets, T, I, q, L, tred, d_freq, alpha ? d_freq + nf : nullptr, n_freq, re, im};
    hipError_t e = hipMemcpyAsync(b, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sum, dim3((unsigned)n_groups, (unsigned)tiles), dim3(64), 0, st, s, extra...);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

extern "C" int pgr_spectrum_device(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                                   const int32_t* q, const double* L, const double* tred, const double* freq,
                                   const double* alpha, int32_t n_freq, double* re, double* im, void* stream)
{
    return spec_run("pgr_spectrum_device", device, offsets, n_groups, T, I, q, L, tred, freq, alpha, n_freq, re, im, stream,
                    pgr_spec_sum);
}

extern "C" int pgr_spectrum_device_phi(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                                       const int32_t* q, const double* phi, const double* L, const double* tred,
                                       const double* freq, const double* alpha, int32_t n_freq, double* re, double* im,
                                       void* stream)
{
    const char* who = "pgr_spectrum_device_phi";
    if (!phi) return fail(std::string(who) + ": null phi (pgr_spectrum_device is the entry without it)");
    return spec_run(who, device, offsets, n_groups, T, I, q, L, tred, freq, alpha, n_freq, re, im, stream, pgr_spec_sum_phi, phi);
}

#endif  // PGR_SPECTRUM_H
