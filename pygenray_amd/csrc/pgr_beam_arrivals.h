// pgr_beam_arrivals.h -- the terms of the coherent Gaussian-beam sum listed as arrivals, per receiver and requested save
// column: pgr_fan_beam_arrival_counts_w, pgr_fan_beam_arrivals_w and their _device twins.
// (Part of the ONE translation unit pgr_hip.hip, included there after pgr_beam_phase.h; not a stand-alone header.)
//
// The quantity, in pgr_beam_phase.h's notation: every term pgr_gbc_sum adds at receiver j and save column
// s -- tube k, centre ci (0 the beam, 1 its surface image, 2 its bottom image), kept by gbc_kept -- is one arrival
//   tube = k,  image = ci,  time = tau,  amplitude = a,  q = (q_k + dq) & 3
// with gbc_kept's own a and tau: the same operations on the same tubes (gbc_chunk_tubes), so the same bits.
//
// Over a caller's list of columns cols[n_cols], after pgr_gba_bounds (pgr_gb_bounds over those columns), one wave per
// (requested column, band of 64 receivers) walks the chunks exactly as pgr_gbc_sum does (gbc_walk):
//   pgr_gba_count  lane j counts its receiver's kept terms: counts[j * n_cols + c];
//   pgr_gba_emit   the same walk; lane j writes its arrivals, in tube and centre order, from offsets[j * n_cols + c] (the
//                  exclusive scan of the counts, formed by the caller).
// No atomics: every receiver's arrivals are found and written by one lane in order, so the output is deterministic.  Lane j's
// stores go to its own run of consecutive entries, 28 bytes per arrival over five arrays -- scattered across the wave, as
// pgr_arr_emit's are: with gexp and the delay they make the emit pass about twice the count pass.  A list
// over few columns is a launch of few waves, each walking all of its column's chunks: latency-bound, not throughput-bound.
#ifndef PGR_BEAM_ARRIVALS_H
#define PGR_BEAM_ARRIVALS_H

struct GbaOut {
    const int32_t* q;         // [S][M] phase index of tube k in quarter cycles, < 0: the tube adds nothing; NULL: all zero
    int64_t* counts;          // count pass: [R][ncol]
    const int64_t* offsets;   // emit pass: [R][ncol], where receiver j's arrivals at slot c start
    int64_t n;                // emit pass: arrivals the outputs hold (writes at or past n are dropped)
    int32_t *tube, *image;
    double *time, *amp;
    int32_t* qa;
};

// gbc_term up to its phase: is the term of the beam centred at ctr kept at depth d, and if so its amplitude a and delay tau
// (the receiver at e in the beam's own space).  The same tests and operations, statement for statement; pgr_gbc_sum keeps its
// own copy so that its machine code stays what it was.
__device__ __forceinline__ bool gbc_kept(double d, double ctr, double e, double sig, double A, double Tm, double pm, double hk,
                                         double& a, double& tau)
{
    const double e0 = d - ctr;
    if (fabs(e0) <= sig * GB_REACH) {                // (a cheap test that never drops a term the next one keeps)
        const double u = fdiv(e0, sig);
        const double v = u * u;
        if (v <= 16.0) {
            a = A * gexp(-0.5 * v);
            tau = Tm + (pm * e + hk * (e * e));
            return true;
        }
    }
    return false;
}

// pgr_gbc_sum's walk over column b.s (b.r != 0) for the band b, statement for statement (the chunk test with padb and the 3-bit
// centre mask, gbc_chunk_tubes, the tubes in order and per tube the centres the mask keeps): term(c, u, ci, ctr, e, sig, A, Tm,
// pm, hk, qk) for tube u of chunk c and centre ci, the receiver at e in the beam's own space, qk the quarter cycles with the
// image's.  pgr_gbc_sum keeps its own copy for the same reason as gbc_term.
template <typename Term>
__device__ __forceinline__ void gbc_walk(const EnvDev& env, const GbArgs& g, const TlBand& b, const int32_t* qin, int curv,
                                         GbcTubes& L, Term term)
{
    const double b2 = 2.0 * g.bottom[b.s];
    const double padb = 0x1p-40 * fabs(b2);          // the rounding of 2 b - m, beyond what pass 1's widening covers
    const Ctx<false, 0> C(env, nullptr);
    const int32_t* q = qin ? qin + (int64_t)b.s * g.M : nullptr;
    const double es = -b.d, eb = b2 - b.d;           // the receiver mirrored in the surface and in the bottom
    tube_walk<3>(g, b.slot, b.d, b.t,
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
#pragma unroll 1
                         for (int ci = 0; ci < 3; ci++) {
                             if (!((w >> ci) & 1)) continue;
                             const double ctr = ci == 0 ? m : ci == 1 ? -m : b2 - m;
                             const double e = (ci == 0 ? b.d : ci == 1 ? es : eb) - m;
                             term(c, u, ci, ctr, e, sig, A, Tm, pm, hk, ci == 1 ? qk + 2 : qk);
                         }
                     }
                 });
}

// pass 1 over the caller's columns: pgr_gb_bounds with slot blockIdx.y mapped through the column list
__global__ void __launch_bounds__(256) pgr_gba_bounds(GbArgs g) { gb_bounds<true>(g); }

__global__ void __launch_bounds__(64) pgr_gba_count(EnvDev env, GbArgs g, GbaOut o)
{
    __shared__ GbcTubes L;
    const TlBand b = tl_band<true>(g);
    int64_t n = 0;
    if (b.r != 0.0) {                                // (the source's own column has no arrivals; uniform in the wave)
        // (the curvature changes an arrival's time alone: counted without it)
        gbc_walk(env, g, b, o.q, 0, L,
                 [&](int64_t, int, int, double ctr, double e, double sig, double A, double Tm, double pm, double hk, int) {
                     double a, tau;
                     if (gbc_kept(b.d, ctr, e, sig, A, Tm, pm, hk, a, tau)) n++;
                 });
    }
    if (b.rcv) o.counts[b.j * g.ncol + b.slot] = n;
}

__global__ void __launch_bounds__(64) pgr_gba_emit(EnvDev env, GbArgs g, GbaOut o, int curv)
{
    __shared__ GbcTubes L;
    const TlBand b = tl_band<true>(g);
    if (b.r == 0.0) return;
    int64_t i = b.rcv ? o.offsets[b.j * g.ncol + b.slot] : -1;
    gbc_walk(env, g, b, o.q, curv, L,
             [&](int64_t c, int u, int ci, double ctr, double e, double sig, double A, double Tm, double pm, double hk, int qk) {
                 double a, tau;
                 if (gbc_kept(b.d, ctr, e, sig, A, Tm, pm, hk, a, tau)) {
                     if (i >= 0 && i < o.n) {
                         o.tube[i] = (int32_t)(c * GB_TUBES + u);
                         o.image[i] = ci;
                         o.time[i] = tau;
                         o.amp[i] = a;
                         o.qa[i] = qk & 3;
                     }
                     if (i >= 0) i++;
                 }
             });
}

// the checks of the entries beyond tl_check: the beams' own, the column list's and, with `emit`, the emit pass's outputs
static int gba_check(const double* bottom, double min_width, const int32_t* cols, int32_t n_cols, int32_t S, bool emit,
                     const GbaOut& o, const char* who)
{
    int rc = gb_check(bottom, min_width, who);
    if (!rc) rc = arr_check(cols, n_cols, S, who);
    if (rc || !emit) return rc;
    if (!o.offsets || !o.tube || !o.image || !o.time || !o.amp || !o.qa) return fail(std::string(who) + ": null argument");
    if (o.n < 1) return fail(std::string(who) + ": n_arrivals must be at least 1 (skip the call when there are none)");
    return 0;
}

// count (o.counts set) or emit on `stream`, over the HOST column list cols[n_cols]
static int gba_run(const pgr_env* env, const TlArgs& a, const double* bottom, double min_width, const int32_t* cols,
                   int32_t n_cols, const GbaOut& o, int32_t curv, void* stream, const char* who)
{
    GbArgs g{a, bottom, min_width};
    if (o.counts) return tube_run(env, g, GB_TUBES, pgr_gba_bounds, cols, n_cols, (hipStream_t)stream, who, pgr_gba_count, o);
    return tube_run(env, g, GB_TUBES, pgr_gba_bounds, cols, n_cols, (hipStream_t)stream, who, pgr_gba_emit, o,
                    (int)(curv != 0));
}

// both passes on a fan handle and on caller buffers (`first`: the entry's first output, `emit`: the emit pass)
static int gba_fan(pgr_fan* f, const double* p0, const double* W, const double* bottom, const double* depths, int64_t n_depths,
                   double min_width, const int32_t* cols, int32_t n_cols, bool emit, const GbaOut& o, int32_t curv,
                   void* stream, const char* who)
{
    const void* first = emit ? (const void*)o.offsets : (const void*)o.counts;
    return tl_fan_entry(f, p0, W, depths, n_depths, first, who,
                        [&](int32_t S) { return gba_check(bottom, min_width, cols, n_cols, S, emit, o, who); },
                        [&](const pgr_env* e, const TlArgs& a) {
                            return gba_run(e, a, bottom, min_width, cols, n_cols, o, curv, stream, who);
                        });
}

static int gba_buffer(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                      const double* x, const double* p0, const double* W, const double* bottom, const double* depths,
                      int64_t n_depths, double min_width, const int32_t* cols, int32_t n_cols, bool emit, const GbaOut& o,
                      int32_t curv, void* stream, const char* who)
{
    const void* first = emit ? (const void*)o.offsets : (const void*)o.counts;
    return tl_buffer_entry<true>(env, T, z, p, n_rays, n_samples, x, p0, W, depths, n_depths, first, who,
                                 [&](int32_t S) { return gba_check(bottom, min_width, cols, n_cols, S, emit, o, who); },
                                 [&](const pgr_env* e, const TlArgs& a) {
                                     return gba_run(e, a, bottom, min_width, cols, n_cols, o, curv, stream, who);
                                 });
}

extern "C" int pgr_fan_beam_arrival_counts_w(pgr_fan* f, const double* p0, const double* weights, const int32_t* q,
                                             const double* bottom, const double* depths, int64_t n_depths, double min_width,
                                             const int32_t* cols, int32_t n_cols, int64_t* counts, void* stream)
{
    const GbaOut o{q, counts};
    return gba_fan(f, p0, weights, bottom, depths, n_depths, min_width, cols, n_cols, false, o, 0, stream,
                   "pgr_fan_beam_arrival_counts_w");
}

extern "C" int pgr_fan_beam_arrivals_w(pgr_fan* f, const double* p0, const double* weights, const int32_t* q,
                                       const double* bottom, const double* depths, int64_t n_depths, double min_width,
                                       const int32_t* cols, int32_t n_cols, int32_t curvature, const int64_t* offsets,
                                       int64_t n_arrivals, int32_t* tube, int32_t* image, double* time, double* amplitude,
                                       int32_t* qa, void* stream)
{
    const GbaOut o{q, nullptr, offsets, n_arrivals, tube, image, time, amplitude, qa};
    return gba_fan(f, p0, weights, bottom, depths, n_depths, min_width, cols, n_cols, true, o, curvature, stream,
                   "pgr_fan_beam_arrivals_w");
}

extern "C" int pgr_beam_arrival_counts_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                                int32_t n_samples, const double* x, const double* p0, const double* weights,
                                                const int32_t* q, const double* bottom, const double* depths, int64_t n_depths,
                                                double min_width, const int32_t* cols, int32_t n_cols, int64_t* counts,
                                                void* stream)
{
    const GbaOut o{q, counts};
    return gba_buffer(env, T, z, p, n_rays, n_samples, x, p0, weights, bottom, depths, n_depths, min_width, cols, n_cols, false,
                      o, 0, stream, "pgr_beam_arrival_counts_device_w");
}

extern "C" int pgr_beam_arrivals_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                          int32_t n_samples, const double* x, const double* p0, const double* weights,
                                          const int32_t* q, const double* bottom, const double* depths, int64_t n_depths,
                                          double min_width, const int32_t* cols, int32_t n_cols, int32_t curvature,
                                          const int64_t* offsets, int64_t n_arrivals, int32_t* tube, int32_t* image,
                                          double* time, double* amplitude, int32_t* qa, void* stream)
{
    const GbaOut o{q, nullptr, offsets, n_arrivals, tube, image, time, amplitude, qa};
    return gba_buffer(env, T, z, p, n_rays, n_samples, x, p0, weights, bottom, depths, n_depths, min_width, cols, n_cols, true, o,
                      curvature, stream, "pgr_beam_arrivals_device_w");
}

#endif  // PGR_BEAM_ARRIVALS_H
