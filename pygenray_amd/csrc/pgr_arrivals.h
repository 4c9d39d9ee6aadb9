// pgr_arrivals.h -- ray-tube arrivals of a fan at receiver depths: pgr_fan_arrival_counts, pgr_fan_arrivals and their
// _device twins.  (Part of the ONE translation unit pgr_hip.hip, included there after pgr_tl.h; not a stand-alone header.)
//
// The quantity (DESIGN.md section "Arrivals"): every tube k that pgr_tl_sum adds at receiver j and save column s is one
// arrival, with w = (D_j - d_k) / (d_k+1 - d_k) and T, p interpolated linearly by w between the tube's two rays; I is the
// tube's term of the TL sum, the same bits (tl_chunk_tubes forms the tubes of all three walks).
//
// Over a caller's list of columns cols[n_cols], after pgr_tl_bounds over those columns, one wave per (requested column,
// band of 64 receivers) walks the chunks exactly as pgr_tl_sum does:
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
    const int slot = blockIdx.x;
    const int s = a.cols[slot];
    const int t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.y * 64 + t;
    const bool rcv = j < a.R;
    const double d = rcv ? a.depths[j] : a.depths[a.R - 1];
    const double x = a.x[s];
    const double r = fabs(x - a.x[0]);
    int64_t n = 0;
    if (r != 0.0) {                                // (the source's own column has no arrivals; uniform in the wave)
        const Ctx<false, 0> C(env, nullptr);
        tl_walk<false>(a, C, slot, s, x, r, d, t, L, nullptr, [&](int64_t, int) { n++; });
    }
    if (rcv) o.counts[j * a.ncol + slot] = n;
}

__global__ void __launch_bounds__(64) pgr_arr_emit(EnvDev env, TlArgs a, ArrOut o)
{
    __shared__ TlTubes L;
    __shared__ TlRays Y;
    const int slot = blockIdx.x;
    const int s = a.cols[slot];
    const int t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.y * 64 + t;
    const bool rcv = j < a.R;
    const double d = rcv ? a.depths[j] : a.depths[a.R - 1];
    const double x = a.x[s];
    const double r = fabs(x - a.x[0]);
    if (r == 0.0) return;
    const Ctx<false, 0> C(env, nullptr);
    int64_t k = rcv ? o.offsets[j * a.ncol + slot] : -1;
    tl_walk<true>(a, C, slot, s, x, r, d, t, L, &Y, [&](int64_t c, int u) {
        if (k >= 0 && k < o.n) {
            const double d0 = Y.d[u], d1 = Y.d[u + 1];
            const double w = fdiv(d - d0, d1 - d0);
            o.tube[k] = (int32_t)(c * TL_TUBES + u);
            o.w[k] = w;
            o.T[k] = Y.T[u] + w * (Y.T[u + 1] - Y.T[u]);
            o.p[k] = Y.p[u] + w * (Y.p[u + 1] - Y.p[u]);
            o.I[k] = L.I[u];
        }
        if (k >= 0) k++;
    });
}

static int arr_check(int64_t M, int32_t S, const double* p0, const double* depths, int64_t R, const int32_t* cols,
                     int32_t n_cols, const void* out, const char* who)
{
    int rc = tl_check(M, S, p0, depths, R, out, who);
    if (rc) return rc;
    if (!cols) return fail(std::string(who) + ": null argument");
    if (n_cols < 1 || n_cols > 65535) return fail(std::string(who) + ": n_cols must be 1 .. 65535");
    for (int32_t c = 0; c < n_cols; c++)
        if (cols[c] < 0 || cols[c] >= S)
            return fail(std::string(who) + ": cols[" + std::to_string(c) + "] = " + std::to_string(cols[c]) +
                        " is not a column 0 .. n_samples - 1");
    return 0;
}

static int arr_check_out(const int64_t* offsets, int64_t n, const int32_t* tube, const double* w, const double* T,
                         const double* p, const double* I, const char* who)
{
    if (!offsets || !tube || !w || !T || !p || !I) return fail(std::string(who) + ": null argument");
    if (n < 1) return fail(std::string(who) + ": n_arrivals must be at least 1 (skip the call when there are none)");
    return 0;
}

// count (o.counts set) or emit on `stream`, over the HOST column list cols[n_cols]
static int arr_run(const pgr_env* env, TlArgs a, const int32_t* cols, int32_t n_cols, const ArrOut& o, hipStream_t st,
                   const char* who)
{
    a.ncol = n_cols;
    return tl_run(a, cols, st, who, [&](const TlArgs& b) {
        const dim3 grid((unsigned)b.ncol, (unsigned)((b.R + 63) / 64));
        if (o.counts) hipLaunchKernelGGL(pgr_arr_count, grid, dim3(64), 0, st, env->d, b, o);
        else hipLaunchKernelGGL(pgr_arr_emit, grid, dim3(64), 0, st, env->d, b, o);
    });
}

extern "C" int pgr_fan_arrival_counts(pgr_fan* f, const double* p0, const double* depths, int64_t n_depths,
                                      const int32_t* cols, int32_t n_cols, int64_t* counts, void* stream)
{
    const char* who = "pgr_fan_arrival_counts";
    if (!f) return fail(std::string(who) + ": null fan");
    if (!f->save) return fail(std::string(who) + ": the fan was launched without trajectories (S = 0)");
    std::lock_guard<std::mutex> lock(f->m);
    TlArgs a;
    int rc = tl_fan_args(f, a, who, [&] { return arr_check(f->M, f->S, p0, depths, n_depths, cols, n_cols, counts, who); });
    if (rc) return rc;
    a.p0 = p0; a.depths = depths; a.R = n_depths;
    ArrOut o{};
    o.counts = counts;
    return arr_run(f->env, a, cols, n_cols, o, (hipStream_t)stream, who);
}

extern "C" int pgr_fan_arrivals(pgr_fan* f, const double* p0, const double* depths, int64_t n_depths, const int32_t* cols,
                                int32_t n_cols, const int64_t* offsets, int64_t n_arrivals, int32_t* tube, double* w,
                                double* T, double* p, double* I, void* stream)
{
    const char* who = "pgr_fan_arrivals";
    if (!f) return fail(std::string(who) + ": null fan");
    if (!f->save) return fail(std::string(who) + ": the fan was launched without trajectories (S = 0)");
    int rc = arr_check_out(offsets, n_arrivals, tube, w, T, p, I, who);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(f->m);
    TlArgs a;
    rc = tl_fan_args(f, a, who, [&] { return arr_check(f->M, f->S, p0, depths, n_depths, cols, n_cols, offsets, who); });
    if (rc) return rc;
    a.p0 = p0; a.depths = depths; a.R = n_depths;
    ArrOut o{nullptr, offsets, n_arrivals, tube, w, T, p, I};
    return arr_run(f->env, a, cols, n_cols, o, (hipStream_t)stream, who);
}

static TlArgs arr_device_args(const double* T, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                              const double* x, const double* p0, const double* depths, int64_t n_depths)
{
    TlArgs a{};
    a.Z = z; a.P = p; a.T = T; a.keep = nullptr;
    a.N = n_rays; a.M = n_rays; a.S = n_samples; a.blocked = 0;
    a.zsign = -1.0;
    a.x = x; a.p0 = p0; a.depths = depths; a.R = n_depths;
    return a;
}

extern "C" int pgr_arrival_counts_device(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                                         const double* x, const double* p0, const double* depths, int64_t n_depths,
                                         const int32_t* cols, int32_t n_cols, int64_t* counts, void* stream)
{
    const char* who = "pgr_arrival_counts_device";
    if (!env) return fail(std::string(who) + ": null environment");
    if (!z || !p || !x) return fail(std::string(who) + ": null argument");
    int rc = arr_check(n_rays, n_samples, p0, depths, n_depths, cols, n_cols, counts, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(env->device));
    ArrOut o{};
    o.counts = counts;
    return arr_run(env, arr_device_args(nullptr, z, p, n_rays, n_samples, x, p0, depths, n_depths), cols, n_cols, o,
                   (hipStream_t)stream, who);
}

extern "C" int pgr_arrivals_device(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                   int32_t n_samples, const double* x, const double* p0, const double* depths,
                                   int64_t n_depths, const int32_t* cols, int32_t n_cols, const int64_t* offsets,
                                   int64_t n_arrivals, int32_t* tube, double* w, double* T_out, double* p_out, double* I,
                                   void* stream)
{
    const char* who = "pgr_arrivals_device";
    if (!env) return fail(std::string(who) + ": null environment");
    if (!T || !z || !p || !x) return fail(std::string(who) + ": null argument");
    int rc = arr_check(n_rays, n_samples, p0, depths, n_depths, cols, n_cols, offsets, who);
    if (rc) return rc;
    rc = arr_check_out(offsets, n_arrivals, tube, w, T_out, p_out, I, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(env->device));
    ArrOut o{nullptr, offsets, n_arrivals, tube, w, T_out, p_out, I};
    return arr_run(env, arr_device_args(T, z, p, n_rays, n_samples, x, p0, depths, n_depths), cols, n_cols, o,
                   (hipStream_t)stream, who);
}

#endif  // PGR_ARRIVALS_H
