// pgr_array.h -- the time-angle response of a vertical line array, delay-and-sum over the elements' arrival lists:
// pgr_array_response_device.
// (Part of the ONE translation unit pgr_hip.hip, included there behind pgr_signal.h and pgr_reflect.h: it uses pgr_signal.h's
// sig_time, sig_lane, SIG_TILE and sig_check; not a stand-alone header.)
//
// The quantity.  The arrival lists are pgr_signal_device's: groups g = j * n_cols + c for element j of
// R and column slot c, arrival a of group g in [off[g], off[g + 1]) with T_a, I_a, q_a and, with phi, its lag in cycles.  With
// a delay per group and look, delay[g * B + b], a weight per group, weight[g], and a start time per column slot, tstart[c],
//   t_n = sig_time(tstart[c], n, dt)
//   re = im = 0.0
//   for j = 0 ... R - 1:  g = j * n_cols + c;  dl = delay[g * B + b];  w = weight[g]
//     for a = off[g] ... off[g + 1] - 1 in order:
//       if q_a < 0: continue                                              (q NULL: 0)
//       Ts = T_a - dl
//       x = (t_n - Ts) * rs;  v = x * x;  if !(v <= 64.0): continue       (a NaN T_a or delay adds nothing)
//       amp = fsqrt(I_a);  amp = amp * w
//       y = f * Ts;  y = y - rint(y);  ph = y - 0.25 * (q_a & 3);  ph = ph - rint(ph)
//       if phi:  r = phi_a - rint(phi_a);  ph = ph - r;  ph = ph - rint(ph)
//       (cv, sv) = gcossin2pi(ph);  E = gexp(-0.5 * v)
//       re = re + (amp * cv) * E;  im = im + (amp * sv) * E
//   y[c][b][n] = re + i im
// which is pgr_sig_sum's term with every travel time shifted by the element's steering delay, under one more loop: with R = 1,
// dl = 0.0 and w = 1.0 (Ts = T_a and amp * 1.0 = amp exactly) the bits are pgr_sig_sum's, with phi pgr_sig_sum_phi's.
//
//   pgr_bf_sum   one wave per (c * B + b, tile of SIG_TILE samples), lanes along time with SIG_ROWS samples each, as in
//                pgr_sig_sum.  The wave walks the elements in order and stages each group's arrivals 64 at a time: lane l loads
//                arrival a0 + l, forms Ts and the live test, and only for a live arrival amp cv and amp sv.  The live arrivals
//                are visited in increasing a, their three constants broadcast by sig_lane: each sample's sum is the definition's
//                sequential sum.  No atomics, no LDS; every output entry is written.  phi is a nullable pointer, uniform in the
//                wave: r = 0 leaves ph's bits alone, so one kernel serves both cases.
// The wave-level skip is pgr_sig_sum's with Ts in T_a's place: tA and tB bound the tile's times exactly and subtraction, the
// product with rs >= 0 and the square are monotone on either side, so vA > 64 (vB > 64) means no sample of the tile keeps the
// arrival.  Never stricter than the per-sample test; at rs = 0 nothing finite is skipped.
#ifndef PGR_ARRAY_H
#define PGR_ARRAY_H

struct BfArgs {
    const int64_t* off;       // [R * n_cols + 1]
    const double* T;          // [n_arrivals]
    const double* I;          // [n_arrivals]
    const int32_t* q;         // [n_arrivals] or NULL
    const double* phi;        // [n_arrivals] or NULL
    const double* delay;      // [R * n_cols][B]
    const double* weight;     // [R * n_cols]
    const double* tstart;     // [n_cols]
    double f, rs, dt;
    int32_t nt;               // samples per (column, look)
    int32_t R, n_cols, B;
    double* re;               // [n_cols][B][nt]
    double* im;               // [n_cols][B][nt]
};

__global__ void __launch_bounds__(64) pgr_bf_sum(BfArgs s)
{
    const int64_t cb = blockIdx.x;                              // c * B + b
    const int64_t c = cb / s.B, b = cb - c * s.B;
    const int32_t n0 = (int32_t)blockIdx.y * SIG_TILE;          // (n0 < nt: the grid has ceil(nt / SIG_TILE) tiles)
    const int lane = threadIdx.x;
    const double t0 = s.tstart[c];
    const int32_t last = min(n0 + SIG_TILE - 1, s.nt - 1);
    const double tA = sig_time(t0, n0, s.dt), tB = sig_time(t0, last, s.dt);
    double t[SIG_ROWS], re[SIG_ROWS], im[SIG_ROWS];
#pragma unroll
    for (int i = 0; i < SIG_ROWS; i++) {
        t[i] = sig_time(t0, min(n0 + i * 64 + lane, s.nt - 1), s.dt);
        re[i] = 0.0;
        im[i] = 0.0;
    }
    for (int32_t j = 0; j < s.R; j++) {                         // the elements in order
        const int64_t g = (int64_t)j * s.n_cols + c;
        const double dl = s.delay[g * s.B + b], w = s.weight[g];
        const int64_t a_end = s.off[g + 1];
        for (int64_t a0 = s.off[g]; a0 < a_end; a0 += 64) {
            const int64_t a = a0 + lane;
            double Ts = NAN, C = 0.0, Sn = 0.0;
            bool live = false;
            if (a < a_end) {
                const int qa = s.q ? s.q[a] : 0;
                Ts = s.T[a] - dl;
                const double xA = (tA - Ts) * s.rs, xB = (tB - Ts) * s.rs;
                const double vA = xA * xA, vB = xB * xB;
                // the shifted arrival before the tile, inside it, behind it; a NaN Ts fails all three
                live = qa >= 0 && ((xA > 0.0 && vA <= 64.0) || (xA <= 0.0 && xB >= 0.0) || (xB < 0.0 && vB <= 64.0));
                if (live) {
                    double amp = fsqrt(s.I[a]);
                    amp = amp * w;
                    double y = s.f * Ts;
                    y = y - rint(y);
                    double ph = y - 0.25 * (double)(qa & 3);
                    ph = ph - rint(ph);
                    if (s.phi) {
                        const double pa = s.phi[a];
                        const double r = pa - rint(pa);
                        ph = ph - r;
                        ph = ph - rint(ph);
                    }
                    double cv, sv;
                    gcossin2pi(ph, cv, sv);
                    C = amp * cv;
                    Sn = amp * sv;
                }
            }
            uint64_t todo = __ballot(live);
            while (todo) {                                      // uniform in the wave: increasing a
                const int u = __builtin_ctzll(todo);
                todo &= todo - 1;
                const double Tu = sig_lane(Ts, u), Cu = sig_lane(C, u), Su = sig_lane(Sn, u);
#pragma unroll
                for (int i = 0; i < SIG_ROWS; i++) {
                    const double x = (t[i] - Tu) * s.rs;
                    const double v = x * x;
                    if (v <= 64.0) {
                        const double E = gexp(-0.5 * v);
                        re[i] = re[i] + Cu * E;
                        im[i] = im[i] + Su * E;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < SIG_ROWS; i++) {
        const int32_t n = n0 + i * 64 + lane;
        if (n < s.nt) {
            s.re[cb * s.nt + n] = re[i];
            s.im[cb * s.nt + n] = im[i];
        }
    }
}

extern "C" int pgr_array_response_device(int device, const int64_t* offsets, int64_t n_elements, int64_t n_cols, const double* T,
                                         const double* I, const int32_t* q, const double* phi, const double* delay,
                                         const double* weight, const double* tstart, double frequency, double inv_sigma,
                                         double dt, int32_t n_times, int64_t n_looks, double* re, double* im, void* stream)
{
    const std::string who = "pgr_array_response_device";
    if (!delay || !weight) return fail(who + ": null argument");
    if (n_elements < 1) return fail(who + ": n_elements must be >= 1");
    if (n_cols < 1) return fail(who + ": n_cols must be >= 1");
    if (n_looks < 1) return fail(who + ": n_looks must be >= 1");
    if (n_cols > INT32_MAX || n_looks > INT32_MAX || n_cols * n_looks > INT32_MAX)
        return fail(who + ": n_cols * n_looks must be <= " + std::to_string(INT32_MAX));
    // (n_cols fits in 32 bits here: the product below cannot overflow for an n_elements that passes the check behind it)
    const int64_t n_groups = n_elements > INT32_MAX ? n_elements : n_elements * n_cols;
    int64_t tiles = 0;
    if (sig_check(who.c_str(), offsets, n_groups, T, I, tstart, frequency, inv_sigma, dt, n_times, re, im, &tiles)) return -1;
    HIPCHK(hipSetDevice(device));
    const BfArgs s{offsets, T, I, q, phi, delay, weight, tstart, frequency, inv_sigma, dt, n_times, (int32_t)n_elements,
                   (int32_t)n_cols, (int32_t)n_looks, re, im};
    hipLaunchKernelGGL(pgr_bf_sum, dim3((unsigned)(n_cols * n_looks), (unsigned)tiles), dim3(64), 0, (hipStream_t)stream, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

#endif  // PGR_ARRAY_H
