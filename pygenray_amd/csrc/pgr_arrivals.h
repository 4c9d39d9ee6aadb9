// pgr_arrivals.h -- ray-tube arrivals of a fan at receiver depths: pgr_fan_arrival_counts, pgr_fan_arrivals and their
// _device twins.  (Part of the ONE translation unit pgr_hip.hip, included there after pgr_tl.h; not a stand-alone header.)
//
// The quantity (DESIGN.md section "Arrivals"): every tube k that pgr_tl_sum adds at receiver j and save column s is one
// arrival, with w = (D_j - d_k) / (d_k+1 - d_k) and T, p interpolated linearly by w between the tube's two rays; I is the
// tube's term of the TL sum, the same bits (tl_chunk_tubes forms the tubes of all three walks).
//
// Over a caller's list of columns cols[n_cols], after pgr_tl_bounds over those columns, one wave per (requested column,
// band of 64 receivers) walks the chunks exactly as pgr_tl_sum does (tl_walk):
//   pgr_arr_count  lane j counts its receiver's tubes: counts[j * n_cols + c];
//   pgr_arr_emit   the same walk; lane j writes its arrivals, in tube order, from offsets[j * n_cols + c] (the exclusive
//                  scan of the counts, formed by the caller).
// No atomics: every receiver's arrivals are found and written by one lane in tube order, so the output is deterministic.
#ifndef PGR_ARRIVALS_H
#define PGR_ARRIVALS_H

struct ArrOut {
    int64_t* counts;          // count pass: [R][ncol]
    const int64_t* offsets;   // emit pass: [R][ncol], where receiver j's arrivals at slot c start
    int64_t n;                // emit pass: arrivals the outputs hold (writes at or past n are dropped)
    int32_t* tube;
    double *w, *T, *p, *I;
};

__global__ void __launch_bounds__(64) pgr_arr_count(EnvDev env, TlArgs a, ArrOut o)
{
    __shared__ TlTubes L;
    const TlBand b = tl_band<true>(a);
    int64_t n = 0;
    if (b.r != 0.0) {                              // (the source's own column has no arrivals; uniform in the wave)
        const Ctx<false, 0> C(env, nullptr);
        tl_walk<false>(a, C, b, L, nullptr, [&](int64_t, int) { n++; });
    }
    if (b.rcv) o.counts[b.j * a.ncol + b.slot] = n;
}

__global__ void __launch_bounds__(64) pgr_arr_emit(EnvDev env, TlArgs a, ArrOut o)
{
    __shared__ TlTubes L;
    __shared__ TlRays Y;
    const TlBand b = tl_band<true>(a);
    if (b.r == 0.0) return;
    const Ctx<false, 0> C(env, nullptr);
    int64_t k = b.rcv ? o.offsets[b.j * a.ncol + b.slot] : -1;
    tl_walk<true>(a, C, b, L, &Y, [&](int64_t c, int u) {
        if (k >= 0 && k < o.n) {
            const double d0 = Y.d[u], d1 = Y.d[u + 1];
            const double w = fdiv(b.d - d0, d1 - d0);
            o.tube[k] = (int32_t)(c * TL_TUBES + u);
            o.w[k] = w;
            o.T[k] = Y.T[u] + w * (Y.T[u + 1] - Y.T[u]);
            o.p[k] = Y.p[u] + w * (Y.p[u + 1] - Y.p[u]);
            o.I[k] = L.I[u];
        }
        if (k >= 0) k++;
    });
}

// the column list's own checks (tl_check has run)
static int arr_check(const int32_t* cols, int32_t n_cols, int32_t S, const char* who)
{
    if (!cols) return fail(std::string(who) + ": null argument");
    if (n_cols < 1 || n_cols > 65535) return fail(std::string(who) + ": n_cols must be 1 .. 65535");
    for (int32_t c = 0; c < n_cols; c++)
        if (cols[c] < 0 || cols[c] >= S)
            return fail(std::string(who) + ": cols[" + std::to_string(c) + "] = " + std::to_string(cols[c]) +
                        " is not a column 0 .. n_samples - 1");
    return 0;
}

// the column list, then the emit pass's outputs
static int arr_check_emit(const int32_t* cols, int32_t n_cols, int32_t S, const int64_t* offsets, int64_t n,
                          const int32_t* tube, const double* w, const double* T, const double* p, const double* I,
                          const char* who)
{
    const int rc = arr_check(cols, n_cols, S, who);
    if (rc) return rc;
    if (!offsets || !tube || !w || !T || !p || !I) return fail(std::string(who) + ": null argument");
    if (n < 1) return fail(std::string(who) + ": n_arrivals must be at least 1 (skip the call when there are none)");
    return 0;
}

// count (o.counts set) or emit on `stream`, over the HOST column list cols[n_cols]
static int arr_run(const pgr_env* env, const TlArgs& a, const int32_t* cols, int32_t n_cols, const ArrOut& o, void* stream,
                   const char* who)
{
    return tube_run(env, a, TL_TUBES, pgr_tl_bounds, cols, n_cols, (hipStream_t)stream, who,
                    o.counts ? pgr_arr_count : pgr_arr_emit, o);
}

extern "C" int pgr_fan_arrival_counts(pgr_fan* f, const double* p0, const double* depths, int64_t n_depths,
                                      const int32_t* cols, int32_t n_cols, int64_t* counts, void* stream)
{
    const char* who = "pgr_fan_arrival_counts";
    return tl_fan_entry(f, p0, nullptr, depths, n_depths, counts, who, [&](int32_t S) { return arr_check(cols, n_cols, S, who); },
                        [&](const pgr_env* e, const TlArgs& a) { return arr_run(e, a, cols, n_cols, {counts}, stream, who); });
}

// the emit entries and their weighted twins (`who`: the entry named in errors)
static int arr_fan_emit(pgr_fan* f, const double* p0, const double* W, const double* depths, int64_t n_depths,
                        const int32_t* cols, int32_t n_cols, const int64_t* offsets, int64_t n_arrivals, int32_t* tube,
                        double* w, double* T, double* p, double* I, void* stream, const char* who)
{
    const ArrOut o{nullptr, offsets, n_arrivals, tube, w, T, p, I};
    return tl_fan_entry(f, p0, W, depths, n_depths, offsets, who,
                        [&](int32_t S) { return arr_check_emit(cols, n_cols, S, offsets, n_arrivals, tube, w, T, p, I, who); },
                        [&](const pgr_env* e, const TlArgs& a) { return arr_run(e, a, cols, n_cols, o, stream, who); });
}

static int arr_buffer_emit(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                           int32_t n_samples, const double* x, const double* p0, const double* W, const double* depths,
                           int64_t n_depths, const int32_t* cols, int32_t n_cols, const int64_t* offsets,
                           int64_t n_arrivals, int32_t* tube, double* w, double* T_out, double* p_out, double* I,
                           void* stream, const char* who)
{
    const ArrOut o{nullptr, offsets, n_arrivals, tube, w, T_out, p_out, I};
    return tl_buffer_entry<true>(env, T, z, p, n_rays, n_samples, x, p0, W, depths, n_depths, offsets, who,
                                 [&](int32_t S) {
                                     return arr_check_emit(cols, n_cols, S, offsets, n_arrivals, tube, w, T_out, p_out, I, who);
                                 },
                                 [&](const pgr_env* e, const TlArgs& a) { return arr_run(e, a, cols, n_cols, o, stream, who); });
}

extern "C" int pgr_fan_arrivals(pgr_fan* f, const double* p0, const double* depths, int64_t n_depths, const int32_t* cols,
                                int32_t n_cols, const int64_t* offsets, int64_t n_arrivals, int32_t* tube, double* w,
                                double* T, double* p, double* I, void* stream)
{
    return arr_fan_emit(f, p0, nullptr, depths, n_depths, cols, n_cols, offsets, n_arrivals, tube, w, T, p, I, stream,
                        "pgr_fan_arrivals");
}

extern "C" int pgr_fan_arrivals_w(pgr_fan* f, const double* p0, const double* weights, const double* depths,
                                  int64_t n_depths, const int32_t* cols, int32_t n_cols, const int64_t* offsets,
                                  int64_t n_arrivals, int32_t* tube, double* w, double* T, double* p, double* I, void* stream)
{
    return arr_fan_emit(f, p0, weights, depths, n_depths, cols, n_cols, offsets, n_arrivals, tube, w, T, p, I, stream,
                        "pgr_fan_arrivals_w");
}

extern "C" int pgr_arrival_counts_device(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                                         const double* x, const double* p0, const double* depths, int64_t n_depths,
                                         const int32_t* cols, int32_t n_cols, int64_t* counts, void* stream)
{
    const char* who = "pgr_arrival_counts_device";
    return tl_buffer_entry<false>(env, nullptr, z, p, n_rays, n_samples, x, p0, nullptr, depths, n_depths, counts, who,
                                  [&](int32_t S) { return arr_check(cols, n_cols, S, who); },
                                  [&](const pgr_env* e, const TlArgs& a) {
                                      return arr_run(e, a, cols, n_cols, {counts}, stream, who);
                                  });
}

extern "C" int pgr_arrivals_device(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                   int32_t n_samples, const double* x, const double* p0, const double* depths,
                                   int64_t n_depths, const int32_t* cols, int32_t n_cols, const int64_t* offsets,
                                   int64_t n_arrivals, int32_t* tube, double* w, double* T_out, double* p_out, double* I,
                                   void* stream)
{
    return arr_buffer_emit(env, T, z, p, n_rays, n_samples, x, p0, nullptr, depths, n_depths, cols, n_cols, offsets,
                           n_arrivals, tube, w, T_out, p_out, I, stream, "pgr_arrivals_device");
}

extern "C" int pgr_arrivals_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                     int32_t n_samples, const double* x, const double* p0, const double* weights,
                                     const double* depths, int64_t n_depths, const int32_t* cols, int32_t n_cols,
                                     const int64_t* offsets, int64_t n_arrivals, int32_t* tube, double* w, double* T_out,
                                     double* p_out, double* I, void* stream)
{
    return arr_buffer_emit(env, T, z, p, n_rays, n_samples, x, p0, weights, depths, n_depths, cols, n_cols, offsets,
                           n_arrivals, tube, w, T_out, p_out, I, stream, "pgr_arrivals_device_w");
}

#endif  // PGR_ARRIVALS_H
