// pgr_bounce.h -- boundary reflection loss of a fan's rays at every save range, from the bounce log the LOG instances of the fan
// kernel write (pgr_fan_launch_log): pgr_fan_boundary_loss, pgr_boundary_loss_device.  A per-ray product, as pgr_path.h.
// (Part of the ONE translation unit pgr_hip.hip, included there last; not a stand-alone header.)
//
// The quantity.  Ray m's log holds its events e = 0 ... E - 1 (E = the leading slots whose kind is not
// the fill -1, at most K), in the order they happened, so bx is non-decreasing along e: range bx_e, slowness bp_e the next
// segment starts with (stored sign: p = psign bp, psign = -1), kind bk_e (0 surface, 1 bottom).
//   c_e     = the table look-up of tl_ray at (bx_e, d_b), d_b = 0 at the surface and the frame's bottom depth at bx_e (the
//             fan kernel's own linear interpolation of depths / depth_ranges) at the bottom;
//   theta_e = degrees(asin(p c_e)), the arcsine correctly rounded (pgr_crmath.h), times 180 / pi;
//   phi_e   = |theta_e| at the surface, |theta_e - beta(bx_e)| at the bottom: the grazing angle, beta the bottom slope in
//             degrees from the table beta_x / beta_deg;
//   loss_e  = the loss table of the boundary at phi_e;  NaN when bx_e, bp_e, c_e or phi_e is NaN (|p c_e| > 1).
// Every table is n values on strictly ascending nodes with section 13's rule (path_alpha): n == 1 the constant, else held at
// the end values outside the nodes and v_j + w (v_j+1 - v_j), w the correctly rounded (q - x_j) / (x_j+1 - x_j), in between.
// The samples an event counts for are the reference's (_interpolate_ray, REF/launch_rays.py:745-784): with x_s the save ranges,
//   j_e = argmin_s |x_s - bx_e| (the first minimum; 0 for a bx_e that is not finite),
//   seg(s) = #{e < E : j_e <= s} for s < S - 1,  seg(S - 1) = E,
//   out[s][m] = sum of loss_e over e < seg(s), from 0.0 in increasing e;  nb / ns[s][m] = those events counted by kind.
//
// Two passes on the caller's stream, no atomics (the choice is argued in DESIGN.md section 14):
//   pgr_bounce_event  one lane per (slot e, ray): loss_e and j_e into a stream-ordered scratch [K][M].  The look-up, the
//                     arcsine and the table searches of different events are independent: full occupancy, no lane waits
//                     for another lane's event;
//   pgr_bounce_rows   one lane per ray walks the rows s = 0 ... S - 1 in step with the other 63 rays of its wave (every row
//                     store is 64 consecutive doubles), taking its next events in whenever their j_e has been reached.
// One lane forms each ray's sum in order, so repeated calls are bit-equal and equal the sequential sum.
#ifndef PGR_BOUNCE_H
#define PGR_BOUNCE_H

struct BounceArgs {
    const double* bx;         // [K][N]
    const double* bp;         // [K][N]
    const signed char* bk;    // [K][N]
    const int* keep;          // column of surviving ray m (NULL: m itself)
    int64_t N, M;
    int32_t K, S;
    int32_t nblk;             // blocks of 256 rays
    double psign;             // the ODE slowness is psign * bp
    const double* x;          // [S] save ranges, ascending, in the frame of the environment
    const double *g, *gl, *sg, *sl, *btx, *bt;
    int32_t ng, ns, nbeta;
    double* loss;             // scratch [K][M]
    int32_t* je;              // scratch [K][M]: j_e, -1 for a slot that holds no event
    double* out;              // [S][M]
    int32_t* nb;              // [S][M] or NULL
    int32_t* nsf;             // [S][M] or NULL
};

// section 13's interpolation rule on the nodes xs[n] (path_alpha's, for any table)
__device__ __forceinline__ double bounce_table(const double* xs, const double* vs, int n, double q)
{
    if (n == 1) return vs[0];
    int lo = 0, hi = n;                            // np.searchsorted(xs, q, side = "right")
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xs[mid] <= q) lo = mid + 1; else hi = mid;
    }
    const int j = min(max(lo - 1, 0), n - 2);
    const double x0 = xs[j], x1 = xs[j + 1], v0 = vs[j], v1 = vs[j + 1];
    if (q <= xs[0]) return vs[0];
    if (q >= xs[n - 1]) return vs[n - 1];
    const double w = fdiv(q - x0, x1 - x0);
    return v0 + w * (v1 - v0);
}

// np.argmin(|x - v|) on the ascending x[S]: the first minimum
__device__ __forceinline__ int bounce_nearest(const double* x, int S, double v)
{
    if (!(fabs(v) <= DBL_MAX)) return 0;           // (NaN: np.argmin's first NaN; +-inf: every distance is inf)
    int lo = 0, hi = S;                            // the nodes below v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] < v) lo = mid + 1; else hi = mid;
    }
    int j = lo == 0 ? 0 : (lo == S ? S - 1 : ((fabs(x[lo] - v) < fabs(x[lo - 1] - v)) ? lo : lo - 1));
    const double d = fabs(x[j] - v);
    while (j > 0 && fabs(x[j - 1] - v) == d) j--;  // (distances that round to the same double: the first one)
    return j;
}

__global__ void __launch_bounds__(256) pgr_bounce_event(EnvDev env, BounceArgs a)
{
    const int e = blockIdx.x / a.nblk;
    const int64_t m = (int64_t)(blockIdx.x % a.nblk) * 256 + threadIdx.x;
    if (m >= a.M) return;
    const int64_t i = (int64_t)e * a.N + (a.keep ? (int64_t)a.keep[m] : m), o = (int64_t)e * a.M + m;
    const int kind = a.bk[i];
    if (kind < 0) { a.je[o] = -1; a.loss[o] = 0.0; return; }
    const double x = a.bx[i], p = a.psign * a.bp[i];
    a.je[o] = bounce_nearest(a.x, a.S, x);
    double loss = NAN;
    if (x == x && p == p) {
        const Ctx<false, 0> C(env, nullptr);
        double c, cp;
        const double d = kind ? C.bathy(x) : 0.0;
        C.lookup(x, d, c, cp);
        const double theta = pgr_cr_asin(p * c) * (180.0 / M_PI);
        const double phi = kind ? fabs(theta - bounce_table(a.btx, a.bt, a.nbeta, x)) : fabs(theta);
        if (phi == phi) loss = kind ? bounce_table(a.g, a.gl, a.ng, phi) : bounce_table(a.sg, a.sl, a.ns, phi);
    }
    a.loss[o] = loss;
}

__global__ void __launch_bounds__(64) pgr_bounce_rows(BounceArgs a)
{
    const int64_t m = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.M) return;
    const int64_t col = a.keep ? (int64_t)a.keep[m] : m;
    double run = 0.0;
    int cb = 0, cs = 0, e = 0;
    int jn = a.K > 0 ? a.je[m] : -1;               // j of the next event, -1: none left
    for (int s = 0; s < a.S; s++) {
        while (jn >= 0 && (jn <= s || s == a.S - 1)) {
            run = run + a.loss[(int64_t)e * a.M + m];
            if (a.bk[(int64_t)e * a.N + col]) cb++; else cs++;
            e++;
            jn = e < a.K ? a.je[(int64_t)e * a.M + m] : -1;
        }
        const int64_t o = (int64_t)s * a.M + m;
        a.out[o] = run;
        if (a.nb) a.nb[o] = cb;
        if (a.nsf) a.nsf[o] = cs;
    }
}

struct BounceTables {
    const double *g, *bot, *s, *surf, *bx, *b;
    int32_t ng, ns, nb;
};

static int bounce_table_check(const double* xs, const double* vs, int32_t n, bool db, const char* what, const char* who)
{
    if (n < 1) return fail(std::string(who) + ": " + what + ": need at least one entry");
    if (!vs || (n > 1 && !xs)) return fail(std::string(who) + ": " + what + ": null table");
    for (int32_t k = 0; k < n; k++) {
        if (!std::isfinite(vs[k]) || (db && vs[k] < 0.0))
            return fail(std::string(who) + ": " + what + (db ? ": the values must be finite and >= 0 dB" : ": the values must be finite"));
        if (n > 1 && (!std::isfinite(xs[k]) || (k && !(xs[k] > xs[k - 1]))))
            return fail(std::string(who) + ": " + what + ": the nodes must be finite and strictly ascending");
    }
    return 0;
}

// the checks of both entries, before any device work
static int bounce_check(int64_t M, int32_t S, int32_t K, const BounceTables& t, const void* out, const char* who)
{
    if (!out) return fail(std::string(who) + ": null out_db");
    int rc = bounce_table_check(t.g, t.bot, t.ng, true, "bottom loss", who);
    if (!rc) rc = bounce_table_check(t.s, t.surf, t.ns, true, "surface loss", who);
    if (!rc) rc = bounce_table_check(t.bx, t.b, t.nb, false, "bottom slope", who);
    if (rc) return rc;
    if (K < 1) return fail(std::string(who) + ": the log needs at least one slot per ray");
    if (M < 1) return fail(std::string(who) + ": need at least one ray");
    if (M > INT32_MAX) return fail(std::string(who) + ": too many rays");
    if (S < 1) return fail(std::string(who) + ": n_samples must be >= 1");
    if (((M + 255) / 256) * (int64_t)K > INT32_MAX) return fail(std::string(who) + ": too many rays times log slots for one launch");
    return 0;
}

// both passes on `stream`; x_host: the save ranges to upload beside the tables (NULL: a.x is set)
static int bounce_run(const pgr_env* env, BounceArgs a, const BounceTables& t, const double* x_host, void* stream, const char* who)
{
    const hipStream_t st = (hipStream_t)stream;
    a.nblk = (int32_t)((a.M + 255) / 256);
    a.ng = t.ng; a.ns = t.ns; a.nbeta = t.nb;
    const size_t nx = x_host ? (size_t)a.S : 0;
    std::vector<double> tab(2 * ((size_t)t.ng + (size_t)t.ns + (size_t)t.nb) + nx, 0.0);
    size_t at = 0, off[7];
    const double* src[6] = {t.g, t.bot, t.s, t.surf, t.bx, t.b};
    const int32_t len[6] = {t.ng, t.ng, t.ns, t.ns, t.nb, t.nb};
    for (int q = 0; q < 6; q++) {
        off[q] = at;
        for (int32_t k = 0; k < len[q]; k++) tab[at + (size_t)k] = src[q] ? src[q][k] : 0.0;
        at += (size_t)len[q];
    }
    off[6] = at;
    for (size_t k = 0; k < nx; k++) tab[at + k] = x_host[k];
    const size_t km = (size_t)a.K * (size_t)a.M;
    const size_t tab_bytes = (tab.size() * 8 + 255) & ~(size_t)255, loss_bytes = (km * 8 + 255) & ~(size_t)255;
    void* b = nullptr;
    if (hipMallocAsync(&b, tab_bytes + loss_bytes + km * 4, st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(std::string(who) + ": device allocation of the tables and the per-event scratch failed");
    }
    const double* base = (const double*)b;
    a.g = base + off[0]; a.gl = base + off[1]; a.sg = base + off[2]; a.sl = base + off[3];
    a.btx = base + off[4]; a.bt = base + off[5];
    if (x_host) a.x = base + off[6];
    a.loss = (double*)((char*)b + tab_bytes);
    a.je = (int32_t*)((char*)b + tab_bytes + loss_bytes);
    hipError_t e = hipMemcpyAsync(b, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_bounce_event, dim3((unsigned)(a.nblk * a.K)), dim3(256), 0, st, env->d, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_bounce_rows, dim3((unsigned)((a.M + 63) / 64)), dim3(64), 0, st, a);
        e = hipGetLastError();
    }
    // (the upload reads `tab`, pageable host memory: staged by the runtime before hipMemcpyAsync returns)
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

extern "C" int pgr_fan_boundary_loss(pgr_fan* f, const double* g_deg, const double* bot_db, int32_t n_bot, const double* s_deg,
                                     const double* surf_db, int32_t n_surf_tab, const double* beta_x, const double* beta_deg,
                                     int32_t n_beta, double* out_db, int32_t* nb, int32_t* ns, void* stream)
{
    const char* who = "pgr_fan_boundary_loss";
    if (!f) return fail(std::string(who) + ": null fan");
    if (!f->log.K) return fail(std::string(who) + ": the fan was launched without a bounce log (pgr_fan_launch_log)");
    const BounceTables t{g_deg, bot_db, s_deg, surf_db, beta_x, beta_deg, n_bot, n_surf_tab, n_beta};
    return fan_entry(f, who, [&](int64_t M, int32_t S) { return bounce_check(M, S, f->log.K, t, out_db, who); },
                     [&](const pgr_env* e, TlArgs ta) {
                         BounceArgs a{};
                         a.bx = f->log.x; a.bp = f->log.p; a.bk = f->log.k; a.keep = ta.keep;
                         a.N = ta.N; a.M = ta.M; a.K = f->log.K; a.S = ta.S;
                         a.psign = ta.zsign;
                         a.x = ta.x;
                         a.out = out_db; a.nb = nb; a.nsf = ns;
                         return bounce_run(e, a, t, nullptr, stream, who);
                     });
}

extern "C" int pgr_boundary_loss_device(pgr_env* env, const double* bx, const double* bp, const int8_t* bk, int64_t n_rays,
                                        int32_t K, double x0, double x1, int32_t n_samples, const double* g_deg,
                                        const double* bot_db, int32_t n_bot, const double* s_deg, const double* surf_db,
                                        int32_t n_surf_tab, const double* beta_x, const double* beta_deg, int32_t n_beta,
                                        double* out_db, int32_t* nb, int32_t* ns, void* stream)
{
    const char* who = "pgr_boundary_loss_device";
    if (!env) return fail(std::string(who) + ": null environment");
    if (!bx || !bp || !bk) return fail(std::string(who) + ": null argument");
    const BounceTables t{g_deg, bot_db, s_deg, surf_db, beta_x, beta_deg, n_bot, n_surf_tab, n_beta};
    const int rc = bounce_check(n_rays, n_samples, K, t, out_db, who);
    if (rc) return rc;
    if (!std::isfinite(x0) || !std::isfinite(x1) || (n_samples > 1 && !(x0 < x1)))
        return fail(std::string(who) + ": need finite x0 < x1 (the frame the fan was traced in; a backwards fan is mirrored)");
    HIPCHK(hipSetDevice(env->device));
    std::vector<double> x((size_t)n_samples);
    for (int32_t k = 0; k < n_samples; k++) x[(size_t)k] = linspace_at(x0, x1, n_samples, k);
    BounceArgs a{};
    a.bx = bx; a.bp = bp; a.bk = (const signed char*)bk; a.keep = nullptr;
    a.N = n_rays; a.M = n_rays; a.K = K; a.S = n_samples;
    a.psign = -1.0;
    a.out = out_db; a.nb = nb; a.nsf = ns;
    return bounce_run(env, a, t, x.data(), stream, who);
}

#endif  // PGR_BOUNCE_H
