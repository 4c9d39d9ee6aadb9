// pgr_path.h -- the running path integral of a fan's rays at every save range (path length, volume absorption) and the
// weights the tube products take from it: pgr_fan_path_integral, pgr_path_integral_device, pgr_absorption_weights_device.
// A per-ray product, as pgr_front.h; it reads the fan where it lies.
// (Part of the ONE translation unit pgr_hip.hip, included there last; not a stand-alone header.)
//
// The quantity ("Path integrals and volume absorption"): for surviving ray m with depth d_s = zsign Z,
// travel time T_s and save range x_s, c_s the look-up of tl_ray and alpha_s = alpha(d_s) from the profile alpha[na] on the
// strictly ascending nodes ad[na] (na == 1: the constant; else held at the end values outside the nodes and, in cell
// j = searchsorted(ad, d, side = "right") - 1 clamped to 0 ... na - 2, alpha_j + w (alpha_j+1 - alpha_j) with
// w = (d - ad_j) / (ad_j+1 - ad_j)),
//   q_s = alpha_s c_s,   inc_s = (0.5 (q_s + q_s+1)) (T_s+1 - T_s),   A(0) = 0.0,   A(s + 1) = A(s) + inc_s,
// added sequentially in increasing s.  A NaN in T or d propagates by IEEE rules: A is NaN from that sample on (A(0) is 0.0
// whatever sample 0 holds).  alpha == 1: the path length, the trapezoid sum of ds = c dT.
//
// Two passes on the caller's stream, no atomics:
//   pgr_path_node  one lane per (sample, ray): q_s into out[s][m].  Every look-up is independent of every other, so the
//                  binary searches of the table look-up and of the profile run at full occupancy;
//   pgr_path_scan  one lane per ray (a wave reads 64 consecutive rays of a row): reads q and T along s and turns out[.][m]
//                  into the running sum in place, in the definition's order.
// One lane forms each ray's sums in order, so repeated calls are bit-equal and equal the sequential sum.  The profile is
// uploaded into a stream-ordered allocation freed behind the second pass.
// pgr_path_weight turns A into the weight W = 10^(-A / 10) = gexp(-(A K)), K the double nearest ln(10) / 10, which tl_ray
// multiplies g by (TlArgs::W): 0 below an argument of -700, NaN for a NaN.
#ifndef PGR_PATH_H
#define PGR_PATH_H

#define PATH_LN10_10 0x1.d791c5f888822p-3  // the double nearest ln(10) / 10

struct PathArgs {
    TlArgs t;                 // the fan as pgr_tl.h reads it (T, Z, keep, N, M, S, blocked, zsign, x); the rest unused
    const double* ad;         // [na] depth nodes of the profile, strictly ascending
    const double* al;         // [na] alpha at the nodes
    int32_t na;
    int32_t nblk;             // blocks of 256 rays
    double* out;              // [S][M]
};

// alpha at depth d (NaN for a NaN depth unless the profile is a constant)
__device__ __forceinline__ double path_alpha(const PathArgs& a, double d)
{
    if (a.na == 1) return a.al[0];
    int lo = 0, hi = a.na;                         // np.searchsorted(ad, d, side = "right")
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.ad[mid] <= d) lo = mid + 1; else hi = mid;
    }
    const int j = min(max(lo - 1, 0), a.na - 2);
    const double d0 = a.ad[j], d1 = a.ad[j + 1], v0 = a.al[j], v1 = a.al[j + 1];
    if (d <= a.ad[0]) return a.al[0];
    if (d >= a.ad[a.na - 1]) return a.al[a.na - 1];
    const double w = fdiv(d - d0, d1 - d0);
    return v0 + w * (v1 - v0);
}

__global__ void __launch_bounds__(256) pgr_path_node(EnvDev env, PathArgs a)
{
    const int s = blockIdx.x / a.nblk;
    const int64_t m = (int64_t)(blockIdx.x % a.nblk) * 256 + threadIdx.x;
    if (m >= a.t.M) return;
    const double d = a.t.zsign * a.t.Z[tl_index(a.t, s, m)];
    double c = NAN, cp;
    if (d == d) {
        const Ctx<false, 0> C(env, nullptr);
        C.lookup(a.t.x[s], d, c, cp);
    }
    a.out[(int64_t)s * a.t.M + m] = path_alpha(a, d) * c;
}

__global__ void __launch_bounds__(64) pgr_path_scan(PathArgs a)
{
    const int64_t m = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (m >= a.t.M) return;
    double* o = a.out + m;
    double q0 = a.t.S > 1 ? o[0] : 0.0, T0 = a.t.T[tl_index(a.t, 0, m)], run = 0.0;   // (S == 1: the node pass did not run)
    o[0] = 0.0;
#pragma unroll 8
    for (int s = 1; s < a.t.S; s++) {
        const double q1 = o[(int64_t)s * a.t.M], T1 = a.t.T[tl_index(a.t, s, m)];
        const double inc = (0.5 * (q0 + q1)) * (T1 - T0);
        run = run + inc;
        o[(int64_t)s * a.t.M] = run;
        q0 = q1;
        T0 = T1;
    }
}

__global__ void __launch_bounds__(256) pgr_path_weight(const double* A, int64_t n, double* W)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double y = -(A[i] * PATH_LN10_10);
    W[i] = y != y ? NAN : (y < -700.0 ? 0.0 : gexp(y));
}

// the checks of both entries, before any device work
static int path_check(int64_t M, int32_t S, const double* ad, const double* al, int32_t na, const void* out, const char* who)
{
    if (!al || !out) return fail(std::string(who) + ": null argument");
    if (na < 1) return fail(std::string(who) + ": n_a must be at least 1");
    if (na > 1 && !ad) return fail(std::string(who) + ": null a_depths (only a constant profile, n_a = 1, needs none)");
    for (int32_t k = 0; k < na; k++)
        if (!std::isfinite(al[k]) || al[k] < 0.0) return fail(std::string(who) + ": alpha must be finite and >= 0");
    for (int32_t k = 0; k < na; k++)
        if (na > 1 && (!std::isfinite(ad[k]) || (k && !(ad[k] > ad[k - 1]))))
            return fail(std::string(who) + ": a_depths must be finite and strictly ascending");
    if (M < 1) return fail(std::string(who) + ": need at least one ray");
    if (M > INT32_MAX) return fail(std::string(who) + ": too many rays");
    if (S < 1) return fail(std::string(who) + ": n_samples must be >= 1");
    if (((M + 255) / 256) * (int64_t)S > INT32_MAX) return fail(std::string(who) + ": too many rays times samples for one launch");
    return 0;
}

// both passes on `stream` for the HOST profile (checked)
static int path_run(const pgr_env* env, TlArgs t, const double* ad, const double* al, int32_t na, double* out, void* stream,
                    const char* who)
{
    const hipStream_t st = (hipStream_t)stream;
    PathArgs a{};
    a.t = t;
    a.na = na;
    a.nblk = (int32_t)((t.M + 255) / 256);
    a.out = out;
    std::vector<double> tab((size_t)2 * (size_t)na, 0.0);
    for (int32_t k = 0; k < na; k++) {
        if (ad) tab[(size_t)k] = ad[k];
        tab[(size_t)na + (size_t)k] = al[k];
    }
    void* b = nullptr;
    if (hipMallocAsync(&b, tab.size() * sizeof(double), st) != hipSuccess)
        return fail(std::string(who) + ": device allocation of the profile failed");
    a.ad = (const double*)b;
    a.al = a.ad + na;
    hipError_t e = hipMemcpyAsync(b, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && t.S > 1) {                // (S == 1: only A(0) = 0.0, which the scan writes)
        hipLaunchKernelGGL(pgr_path_node, dim3((unsigned)(a.nblk * t.S)), dim3(256), 0, st, env->d, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_path_scan, dim3((unsigned)((t.M + 63) / 64)), dim3(64), 0, st, a);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

extern "C" int pgr_fan_path_integral(pgr_fan* f, const double* a_depths, const double* alpha, int32_t n_a, double* out,
                                     void* stream)
{
    const char* who = "pgr_fan_path_integral";
    return fan_entry(f, who, [&](int64_t M, int32_t S) { return path_check(M, S, a_depths, alpha, n_a, out, who); },
                     [&](const pgr_env* e, TlArgs t) { return path_run(e, t, a_depths, alpha, n_a, out, stream, who); });
}

extern "C" int pgr_path_integral_device(pgr_env* env, const double* T, const double* z, int64_t n_rays, int32_t n_samples,
                                        const double* x, const double* a_depths, const double* alpha, int32_t n_a,
                                        double* out, void* stream)
{
    const char* who = "pgr_path_integral_device";
    if (!env) return fail(std::string(who) + ": null environment");
    if (!T || !z || !x) return fail(std::string(who) + ": null argument");
    const int rc = path_check(n_rays, n_samples, a_depths, alpha, n_a, out, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(env->device));
    TlArgs t{};
    t.Z = z; t.T = T; t.keep = nullptr;
    t.N = n_rays; t.M = n_rays; t.S = n_samples; t.blocked = 0;
    t.zsign = -1.0;
    t.x = x;
    return path_run(env, t, a_depths, alpha, n_a, out, stream, who);
}

extern "C" int pgr_absorption_weights_device(int device, const double* A, int64_t n, double* W, void* stream)
{
    const char* who = "pgr_absorption_weights_device";
    if (!A || !W) return fail(std::string(who) + ": null argument");
    if (n < 1 || (n + 255) / 256 > INT32_MAX) return fail(std::string(who) + ": n must be 1 .. 2^39");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(pgr_path_weight, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A, n, W);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

#endif  // PGR_PATH_H
