// pgr_tl.h -- ray-tube intensity (transmission loss) of a fan on a range-depth grid: pgr_fan_intensity, pgr_intensity_device.
// (Part of the ONE translation unit pgr_hip.hip, included there last; not a stand-alone header.)
//
// The quantity (DESIGN.md section "Transmission loss"): adjacent surviving rays k, k + 1 bound a tube; at save sample s
//   g = c / sqrt(1 - (p c)^2),   I_k(s) = 0.5 (g_k + g_k+1) |p0_k+1 - p0_k| / (r_s |z_k+1 - z_k|),   r_s = |x_s - x_0|,
// and receiver j gets the sum, in increasing k from 0.0, of I_k(s) over the tubes with lo <= d_j < hi (lo / hi: the min / max
// depth of the tube's two samples).  A tube with a NaN sample, |p c| >= 1 at either end or z_k+1 == z_k adds nothing; the
// column r_s == 0 is NaN.
//
// Two passes, no atomics:
//   pgr_tl_bounds  one wave per (column s, chunk of TL_TUBES consecutive tubes = TL_TUBES + 1 rays): the chunk's depth interval;
//   pgr_tl_sum     one wave per (column s, band of 64 receivers), a lane per receiver: walks the chunks of its column in
//                  order, skips those whose interval misses the band, and for each of the others the lanes form the chunk's
//                  tubes (lane t: ray t of the chunk, its neighbour by a lane shuffle) into LDS, then every lane adds, tube by
//                  tube in order, those that contain its receiver.  Each receiver's sum is formed by one lane in tube order,
//                  so the result does not depend on scheduling and equals the sequential sum bit for bit.
#ifndef PGR_TL_H
#define PGR_TL_H

#define TL_TUBES 63   // tubes per chunk: a chunk's 64 rays fill one wave, lane 63 only lends its ray to tube 62

struct TlArgs {
    const double* Z;          // depth samples, stored convention (depth = zsign * Z)
    const double* P;
    const double* T;          // travel times (arrivals only; NULL for TL)
    const int* keep;          // column of surviving ray m in Z / P (NULL: m itself)
    int64_t N;                // rays held in Z / P (the column stride)
    int64_t M;                // surviving rays (tubes: M - 1)
    int32_t S;
    int32_t blocked;          // Z / P are [ceil(S/4)][N][4] (PGR_SAMPLE_BLOCKED), else [S][N]
    double zsign;
    const double* x;          // save ranges [S], in the frame the fan was traced in
    const double* p0;         // [M]
    const double* depths;     // [R]
    int64_t R;
    int64_t nchunk;
    const int32_t* cols;      // the columns walked: slot c is column cols[c] (NULL: slot s is column s, all S of them)
    int32_t ncol;             // slots (S when cols is NULL)
    double* bounds;           // [ncol][nchunk][2]
    double* out;              // [R][S]
};

__device__ __forceinline__ int64_t tl_index(const TlArgs& a, int s, int64_t n)
{
    return a.blocked ? (((int64_t)(s >> 2) * a.N + n) << 2) + (s & 3) : (int64_t)s * a.N + n;
}

__device__ __forceinline__ int tl_column(const TlArgs& a, int c) { return a.cols ? a.cols[c] : c; }

__device__ __forceinline__ double tl_wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ double tl_wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// pass 1: [min, max] depth of the rays of chunk c in column slot y (NaN samples ignored; an all-NaN chunk gets the empty
// [+inf, -inf])
__global__ void __launch_bounds__(256) pgr_tl_bounds(TlArgs a)
{
    const int s = tl_column(a, blockIdx.y);
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = threadIdx.x & 63;
    if (c >= a.nchunk) return;                      // (whole waves: c is uniform in the wave)
    const int64_t m = c * TL_TUBES + t;
    double lo = INFINITY, hi = -INFINITY;
    if (m < a.M) {
        const int64_t n = a.keep ? (int64_t)a.keep[m] : m;
        const double d = a.zsign * a.Z[tl_index(a, s, n)];
        if (d == d) { lo = d; hi = d; }
    }
    lo = tl_wave_min(lo);
    hi = tl_wave_max(hi);
    if (t == 0) {
        double* b = a.bounds + 2 * ((int64_t)blockIdx.y * a.nchunk + c);
        b[0] = lo;
        b[1] = hi;
    }
}

// the LDS of one wave's walk: the current chunk's tubes, and with RAYS its rays' depth, travel time and stored-sign slowness
struct TlTubes { double lo[64], hi[64], I[64]; };
struct TlRays { double d[64], T[64], p[64]; };

// The tubes of chunk c in column s into LDS: lane t loads ray m = c * TL_TUBES + t (its depth, g and launch slowness),
// takes its neighbour's by a lane shuffle and forms tube t (an empty interval [0, 0) where the tube adds nothing).  TL and
// the arrival passes all form their tubes here, so they see the same tubes and the same bits of I.
template <bool RAYS>
__device__ __forceinline__ void tl_chunk_tubes(const TlArgs& a, const Ctx<false, 0>& C, int s, double x, double r,
                                               int64_t c, int t, TlTubes& L, TlRays* Y)
{
    const int64_t m = c * TL_TUBES + t;
    double dz = NAN, g = NAN, q0 = NAN, p = NAN, T = NAN;
    if (m < a.M) {
        const int64_t n = a.keep ? (int64_t)a.keep[m] : m;
        const int64_t i = tl_index(a, s, n);
        dz = a.zsign * a.Z[i];
        p = a.P[i];
        if (RAYS) T = a.T[i];
        q0 = a.p0[m];
        if (dz == dz && p == p) {
            double cv, cp;
            C.lookup(x, dz, cv, cp);
            const double pc = p * cv;
            if (fabs(pc) < 1.0) g = fdiv(cv, fsqrt(1.0 - pc * pc));
        }
    }
    const double dz1 = __shfl_down(dz, 1), g1 = __shfl_down(g, 1), q1 = __shfl_down(q0, 1);
    double lo = 0.0, hi = 0.0, I = 0.0;
    if (t < TL_TUBES && m + 1 < a.M && g == g && g1 == g1 && dz != dz1) {
        lo = fmin(dz, dz1);
        hi = fmax(dz, dz1);
        I = fdiv(0.5 * (g + g1) * fabs(q1 - q0), r * fabs(dz1 - dz));
    }
    __syncthreads();                               // (the previous chunk's tubes have been read)
    L.lo[t] = lo;
    L.hi[t] = hi;
    L.I[t] = I;
    if (RAYS) {
        Y->d[t] = dz;
        Y->T[t] = T;
        Y->p[t] = -a.zsign * p;                    // RayFan.ps's sign whatever the fan kernel stored
    }
    __syncthreads();
}

// The walk of one wave over column s for its band of receivers (lane t: receiver depth d): the chunks of the column in
// order, those whose interval misses the band skipped, and for every tube u of a chunk, in order, that holds d,
// visit(u).  The tubes of chunk c are then in L (and Y), tube u being rays c * TL_TUBES + u and + u + 1.
template <bool RAYS, typename Visit>
__device__ __forceinline__ void tl_walk(const TlArgs& a, const Ctx<false, 0>& C, int slot, int s, double x, double r,
                                        double d, int t, TlTubes& L, TlRays* Y, Visit visit)
{
    // the band's depth span (whatever the order of the depths)
    const double dlo = tl_wave_min(d), dhi = tl_wave_max(d);
    const double* bnd = a.bounds + 2 * (int64_t)slot * a.nchunk;
    for (int64_t c0 = 0; c0 < a.nchunk; c0 += 64) {
        bool hit = false;
        if (c0 + t < a.nchunk) {
            const double clo = bnd[2 * (c0 + t)], chi = bnd[2 * (c0 + t) + 1];
            hit = (clo <= dhi) & (chi > dlo);      // a tube [lo, hi) of the chunk may hold a receiver of the band
        }
        unsigned long long mask = ballot64(hit);
        while (mask) {
            const int64_t c = c0 + __builtin_ctzll(mask);
            mask &= mask - 1;
            tl_chunk_tubes<RAYS>(a, C, s, x, r, c, t, L, Y);
            for (int u = 0; u < TL_TUBES; u++)
                if ((L.lo[u] <= d) & (d < L.hi[u])) visit(c, u);
        }
    }
}

// pass 2: one wave per (column, band of 64 receivers)
__global__ void __launch_bounds__(64) pgr_tl_sum(EnvDev env, TlArgs a)
{
    __shared__ TlTubes L;
    const int s = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.y * 64 + t;
    const bool rcv = j < a.R;
    const double d = rcv ? a.depths[j] : a.depths[a.R - 1];
    const double x = a.x[s];
    const double r = fabs(x - a.x[0]);
    if (r == 0.0) {                                // the source's own column
        if (rcv) a.out[j * a.S + s] = NAN;
        return;
    }
    const Ctx<false, 0> C(env, nullptr);
    double acc = 0.0;
    tl_walk<false>(a, C, s, s, x, r, d, t, L, nullptr, [&](int64_t, int u) { acc = acc + L.I[u]; });
    if (rcv) a.out[j * a.S + s] = acc;
}

// pass 1 over a.ncol column slots (a.cols: HOST [ncol], uploaded here; NULL: all S columns), then `second` on `stream`; the
// chunk bounds (and the column list) live in a stream-ordered allocation freed behind the second pass
template <typename Second>
static int tl_run(TlArgs a, const int32_t* cols, hipStream_t st, const char* who, Second second)
{
    a.nchunk = (a.M - 1 + TL_TUBES - 1) / TL_TUBES;
    if (!cols) a.ncol = a.S;
    const size_t nb = (size_t)a.ncol * (size_t)a.nchunk * 16;
    void* b = nullptr;
    if (hipMallocAsync(&b, nb + (cols ? (size_t)a.ncol * sizeof(int32_t) : 0), st) != hipSuccess)
        return fail(std::string(who) + ": device allocation of the chunk bounds failed");
    a.bounds = (double*)b;
    a.cols = nullptr;
    hipError_t e = hipSuccess;
    if (cols) {
        a.cols = (const int32_t*)((char*)b + nb);
        e = hipMemcpyAsync((void*)a.cols, cols, (size_t)a.ncol * sizeof(int32_t), hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_tl_bounds, dim3((unsigned)((a.nchunk + 3) / 4), (unsigned)a.ncol), dim3(256), 0, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        second(a);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

static int tl_run(const pgr_env* env, TlArgs a, hipStream_t st, const char* who)
{
    return tl_run(a, nullptr, st, who, [&](const TlArgs& b) {
        hipLaunchKernelGGL(pgr_tl_sum, dim3((unsigned)b.S, (unsigned)((b.R + 63) / 64)), dim3(64), 0, st, env->d, b);
    });
}

static int tl_check(int64_t M, int32_t S, const double* p0, const double* depths, int64_t R, const void* out, const char* who)
{
    if (!p0 || !depths || !out) return fail(std::string(who) + ": null argument");
    if (M < 2) return fail(std::string(who) + ": need at least two rays (one ray tube)");
    if (M > INT32_MAX) return fail(std::string(who) + ": too many rays");
    if (S < 1 || S > 65535) return fail(std::string(who) + ": n_samples must be 1 .. 65535");
    if (R < 1 || R > (int64_t)65535 * 64) return fail(std::string(who) + ": n_depths must be 1 .. 4194240");
    return 0;
}

// a device-resident fan's TlArgs: waits for its kernel, runs the caller's argument `check` (the fan's M is known then),
// uploads the keep list and the save ranges on first use (held by the handle); the caller holds f->m
template <typename Check>
static int tl_fan_args(pgr_fan* f, TlArgs& a, const char* who, Check check)
{
    HIPCHK(hipSetDevice(f->env->device));
    int rc = fan_finish(f);
    if (rc) return rc;
    rc = check();
    if (rc) return rc;
    if (f->M != f->N && !f->d_keep) {
        // the columns of the surviving rays, uploaded once per fan (freed with it): dropped rays are skipped in place
        if (hipMalloc(&f->d_keep, (size_t)f->M * sizeof(int)) != hipSuccess) {
            f->d_keep = nullptr;
            return fail(std::string(who) + ": device allocation failed");
        }
        HIPCHK(hipMemcpy(f->d_keep, f->keep.data(), (size_t)f->M * sizeof(int), hipMemcpyHostToDevice));
    }
    if (!f->r_filled) {
        // the save ranges, np.linspace's bits (PGR_SAVE_LINSPACE: the fan kernel's for S > 1; at S = 1 the one column is NaN)
        std::vector<double> r((size_t)f->S);
        for (int32_t k = 0; k < f->S; k++) r[(size_t)k] = linspace_at(f->x0, f->x1, f->S, k);
        HIPCHK(hipMemcpy(f->d.r, r.data(), (size_t)f->S * sizeof(double), hipMemcpyHostToDevice));
        f->r_filled = true;
    }
    a = TlArgs{};
    a.Z = f->d.Z; a.P = f->d.P; a.T = f->d.T; a.keep = (f->M != f->N) ? f->d_keep : nullptr;
    a.N = f->N; a.M = f->M; a.S = f->S; a.blocked = f->blocked ? 1 : 0;
    a.zsign = (f->flags & PGR_STORED_SIGN) ? -1.0 : 1.0;
    a.x = f->d.r;
    return 0;
}

extern "C" int pgr_fan_intensity(pgr_fan* f, const double* p0, const double* depths, int64_t n_depths, double* out,
                                 void* stream)
{
    if (!f) return fail("pgr_fan_intensity: null fan");
    if (!f->save) return fail("pgr_fan_intensity: the fan was launched without trajectories (S = 0)");
    std::lock_guard<std::mutex> lock(f->m);
    TlArgs a;
    int rc = tl_fan_args(f, a, "pgr_fan_intensity",
                         [&] { return tl_check(f->M, f->S, p0, depths, n_depths, out, "pgr_fan_intensity"); });
    if (rc) return rc;
    a.p0 = p0; a.depths = depths; a.R = n_depths; a.out = out;
    return tl_run(f->env, a, (hipStream_t)stream, "pgr_fan_intensity");
}

extern "C" int pgr_intensity_device(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                                    const double* x, const double* p0, const double* depths, int64_t n_depths, double* out,
                                    void* stream)
{
    if (!env) return fail("pgr_intensity_device: null environment");
    if (!z || !p || !x) return fail("pgr_intensity_device: null argument");
    int rc = tl_check(n_rays, n_samples, p0, depths, n_depths, out, "pgr_intensity_device");
    if (rc) return rc;
    HIPCHK(hipSetDevice(env->device));
    TlArgs a{};
    a.Z = z; a.P = p; a.keep = nullptr;
    a.N = n_rays; a.M = n_rays; a.S = n_samples; a.blocked = 0;
    a.zsign = -1.0;
    a.x = x; a.p0 = p0; a.depths = depths; a.R = n_depths; a.out = out;
    return tl_run(env, a, (hipStream_t)stream, "pgr_intensity_device");
}

#endif  // PGR_TL_H
