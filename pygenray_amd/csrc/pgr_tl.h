// pgr_tl.h -- the ray-tube walk of a fan's trajectories, shared by every product on the tubes, and on it the ray-tube
// intensity (transmission loss) on a range-depth grid: pgr_fan_intensity, pgr_intensity_device.
// (Part of the ONE translation unit pgr_hip.hip, included there after the fan side; not a stand-alone header.)
//
// The quantity (DESIGN.md section "Transmission loss"): adjacent surviving rays k, k + 1 bound a tube; at save sample s
//   g = c / sqrt(1 - (p c)^2),   I_k(s) = 0.5 (g_k + g_k+1) |p0_k+1 - p0_k| / (r_s |z_k+1 - z_k|),   r_s = |x_s - x_0|,
// and receiver j gets the sum, in increasing k from 0.0, of I_k(s) over the tubes with lo <= d_j < hi (lo / hi: the min / max
// depth of the tube's two samples).  A tube with a NaN sample, |p c| >= 1 at either end or z_k+1 == z_k adds nothing; the
// column r_s == 0 is NaN.
//
// Two passes, no atomics, for every tube product (TL and the arrivals of pgr_arrivals.h on this file's tubes of 63, the
// Gaussian beams of pgr_beams.h on tubes of 61 with a halo ray either side):
//   pass 1  tube_bounds: one wave per (column slot, chunk of consecutive tubes): the depth interval the chunk's tubes can
//           reach (TL: its rays' depths), into a.bounds;
//   pass 2  tube_walk: one wave per (column slot, band of 64 receivers), a lane per receiver: walks the chunks of its column
//           in order and skips those whose interval fails the product's test against the band; for each of the others the
//           lanes form the chunk's tubes (lane t: ray t of the chunk, its neighbours by lane shuffles) into LDS, then every
//           lane goes through them in order for its own receiver.  Each receiver's result is formed by one lane in tube
//           order, so it does not depend on scheduling and equals the sequential sum bit for bit.
// tube_run launches both on the caller's stream; tl_fan_entry and tl_buffer_entry are the prologues of the C entries.
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
    const double* W;          // weights of g, [S][M] rows over the surviving rays (pgr_path.h); NULL: none
};

// where surviving ray m's sample s lies in Z / P (dropped rays skipped through the keep list)
__device__ __forceinline__ int64_t tl_index(const TlArgs& a, int s, int64_t m)
{
    const int64_t n = a.keep ? (int64_t)a.keep[m] : m;
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

// Pass 1 of a tube shape (TUBES tubes per chunk, lane t holding ray c * TUBES + t + RAY0): one wave per (column slot
// blockIdx.y, chunk c).  interval(t, m, lo, hi) sets the part of the chunk's interval lane t knows from its ray m; the
// wave's [min lo, max hi] (none: the empty [+inf, -inf]) is the chunk's, with PAD widened by 2^-40 of its magnitude.
template <int TUBES, int RAY0, bool PAD, typename Interval>
__device__ __forceinline__ void tube_bounds(const TlArgs& a, Interval interval)
{
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = threadIdx.x & 63;
    if (c >= a.nchunk) return;                      // (whole waves: c is uniform in the wave)
    double lo = INFINITY, hi = -INFINITY;
    interval(t, c * TUBES + t + RAY0, lo, hi);
    lo = tl_wave_min(lo);
    hi = tl_wave_max(hi);
    if (t == 0) {
        if (PAD && lo <= hi) {
            const double pad = 0x1p-40 * fmax(fabs(lo), fabs(hi));
            lo -= pad;
            hi += pad;
        }
        double* b = a.bounds + 2 * ((int64_t)blockIdx.y * a.nchunk + c);
        b[0] = lo;
        b[1] = hi;
    }
}

// TL's pass 1: [min, max] depth of the rays of chunk c in column slot y (NaN samples ignored)
__global__ void __launch_bounds__(256) pgr_tl_bounds(TlArgs a)
{
    const int s = tl_column(a, blockIdx.y);
    tube_bounds<TL_TUBES, 0, false>(a, [&](int, int64_t m, double& lo, double& hi) {
        if (m < a.M) {
            const double d = a.zsign * a.Z[tl_index(a, s, m)];
            if (d == d) { lo = d; hi = d; }
        }
    });
}

// The band of a pass-2 wave: column slot blockIdx.x (column s: a.cols[slot] with COLS, else the slot itself), lane t's
// receiver j (rcv: j < R; the lanes past the last receiver take its depth, so the band's span is the receivers'), its
// depth d, and the column's range x and distance r from the source (r == 0: the source's own column, uniform in the wave)
struct TlBand {
    int slot, s, t;
    int64_t j;
    bool rcv;
    double d, x, r;
    // an image's value at (j, s): a.out[R][S]
    __device__ __forceinline__ void put(const TlArgs& a, double v) const { if (rcv) a.out[j * a.S + s] = v; }
};

template <bool COLS>
__device__ __forceinline__ TlBand tl_band(const TlArgs& a)
{
    TlBand b;
    b.slot = blockIdx.x;
    b.s = COLS ? a.cols[b.slot] : b.slot;
    b.t = threadIdx.x;
    b.j = (int64_t)blockIdx.y * 64 + b.t;
    b.rcv = b.j < a.R;
    b.d = b.rcv ? a.depths[b.j] : a.depths[a.R - 1];
    b.x = a.x[b.s];
    b.r = fabs(b.x - a.x[0]);
    return b;
}

// The walk of a pass-2 wave over column slot `slot` for its band (lane t: receiver depth d): the chunks of the column in
// order, and for each whose interval [lo, hi] passes test(lo, hi, dlo, dhi) against the band's span -- a mask of BITS
// tests, evaluated by the lane c mod 64 -- chunk(c, mask), uniformly in the wave (BITS = 1: the mask is 1).
template <int BITS, typename Test, typename Chunk>
__device__ __forceinline__ void tube_walk(const TlArgs& a, int slot, double d, int t, Test test, Chunk chunk)
{
    // the band's depth span (whatever the order of the depths)
    const double dlo = tl_wave_min(d), dhi = tl_wave_max(d);
    const double* bnd = a.bounds + 2 * (int64_t)slot * a.nchunk;
    for (int64_t c0 = 0; c0 < a.nchunk; c0 += 64) {
        int hit = 0;
        if (c0 + t < a.nchunk) hit = test(bnd[2 * (c0 + t)], bnd[2 * (c0 + t) + 1], dlo, dhi);
        unsigned long long mask = ballot64(hit != 0);
        while (mask) {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            chunk(c0 + l, BITS == 1 ? 1 : __shfl(hit, l));
        }
    }
}

// Lane t's ray m of column s when `in`, else all NaN: its depth d, slowness p (stored sign), with RAYS its travel time T,
// its launch slowness q0 and g = c / sqrt(1 - (p c)^2) (NaN for a NaN sample or |p c| >= 1).  Every tube shape loads its
// rays here, so TL, the arrivals and the beams see the same bits of g.  With weights (a.W, uniform in the launch) g is
// g W[s][m]: a NaN weight makes the sample one that adds nothing, as a NaN g does.
struct TlRay { double d, p, T, q0, g; };

template <bool RAYS>
__device__ __forceinline__ TlRay tl_ray(const TlArgs& a, const Ctx<false, 0>& C, int s, double x, int64_t m, bool in)
{
    TlRay y{NAN, NAN, NAN, NAN, NAN};
    if (in) {
        const int64_t i = tl_index(a, s, m);
        y.d = a.zsign * a.Z[i];
        y.p = a.P[i];
        if (RAYS) y.T = a.T[i];
        y.q0 = a.p0[m];
        if (y.d == y.d && y.p == y.p) {
            double cv, cp;
            C.lookup(x, y.d, cv, cp);
            const double pc = y.p * cv;
            if (fabs(pc) < 1.0) y.g = fdiv(cv, fsqrt(1.0 - pc * pc));
            if (a.W && y.g == y.g) y.g = y.g * a.W[(int64_t)s * a.M + m];
        }
    }
    return y;
}

// the LDS of one wave's walk: the current chunk's tubes, and with RAYS its rays' depth, travel time and stored-sign slowness
struct TlTubes { double lo[64], hi[64], I[64]; };
struct TlRays { double d[64], T[64], p[64]; };

// The tubes of chunk c in column s into LDS: lane t loads ray m = c * TL_TUBES + t, takes its neighbour's by a lane shuffle
// and forms tube t (an empty interval [0, 0) where the tube adds nothing).
template <bool RAYS>
__device__ __forceinline__ void tl_chunk_tubes(const TlArgs& a, const Ctx<false, 0>& C, int s, double x, double r,
                                               int64_t c, int t, TlTubes& L, TlRays* Y)
{
    const int64_t m = c * TL_TUBES + t;
    const TlRay y = tl_ray<RAYS>(a, C, s, x, m, m < a.M);
    const double dz = y.d, g = y.g, q0 = y.q0;
    const double dz1 = __shfl_down(dz, 1), g1 = __shfl_down(g, 1), q1 = __shfl_down(q0, 1);
    double lo = 0.0, hi = 0.0, I = 0.0;
    if (t < TL_TUBES && m + 1 < a.M && g == g && g1 == g1 && dz != dz1) {
        lo = fmin(dz, dz1);
        hi = fmax(dz, dz1);
        I = fdiv_inf(0.5 * (g + g1) * fabs(q1 - q0), r * fabs(dz1 - dz));   // (g W can be infinite: a weight that overflowed)
    }
    __syncthreads();                               // (the previous chunk's tubes have been read)
    L.lo[t] = lo;
    L.hi[t] = hi;
    L.I[t] = I;
    if (RAYS) {
        Y->d[t] = dz;
        Y->T[t] = y.T;
        Y->p[t] = -a.zsign * y.p;                  // RayFan.ps's sign whatever the fan kernel stored
    }
    __syncthreads();
}

// TL's walk (TL and both arrival passes): for every tube u of a chunk, in order, that holds the lane's receiver, visit(c, u);
// the tubes of chunk c are then in L (and Y), tube u being rays c * TL_TUBES + u and + u + 1
template <bool RAYS, typename Visit>
__device__ __forceinline__ void tl_walk(const TlArgs& a, const Ctx<false, 0>& C, const TlBand& b, TlTubes& L, TlRays* Y,
                                        Visit visit)
{
    tube_walk<1>(a, b.slot, b.d, b.t,
                 // a tube [lo, hi) of the chunk may hold a receiver of the band
                 [](double lo, double hi, double dlo, double dhi) { return (lo <= dhi) & (hi > dlo); },
                 [&](int64_t c, int) {
                     tl_chunk_tubes<RAYS>(a, C, b.s, b.x, b.r, c, b.t, L, Y);
                     for (int u = 0; u < TL_TUBES; u++)
                         if ((L.lo[u] <= b.d) & (b.d < L.hi[u])) visit(c, u);
                 });
}

// TL's pass 2: one wave per (column, band of 64 receivers)
__global__ void __launch_bounds__(64) pgr_tl_sum(EnvDev env, TlArgs a)
{
    __shared__ TlTubes L;
    const TlBand b = tl_band<false>(a);
    if (b.r == 0.0) {                              // the source's own column
        b.put(a, NAN);
        return;
    }
    const Ctx<false, 0> C(env, nullptr);
    double acc = 0.0;
    tl_walk<false>(a, C, b, L, nullptr, [&](int64_t, int u) { acc = acc + L.I[u]; });
    b.put(a, acc);
}

// Pass 1 (`bounds`, chunks of `tubes` tubes) over the column slots -- the HOST list cols[ncol], uploaded here, or (cols
// NULL) all S columns -- then pass 2, sum(env, g, extra...) with one wave per (slot, band of 64 receivers), on `st`.  The
// chunk bounds (and the column list) live in a stream-ordered allocation freed behind pass 2.
template <typename Args, typename... Extra>
static int tube_run(const pgr_env* env, Args g, int tubes, void (*bounds)(Args), const int32_t* cols, int32_t ncol,
                    hipStream_t st, const char* who, void (*sum)(EnvDev, Args, Extra...), Extra... extra)
{
    TlArgs& a = g;
    a.nchunk = (a.M - 1 + tubes - 1) / tubes;
    a.ncol = cols ? ncol : a.S;
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
        hipLaunchKernelGGL(bounds, dim3((unsigned)((a.nchunk + 3) / 4), (unsigned)a.ncol), dim3(256), 0, st, g);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sum, dim3((unsigned)a.ncol, (unsigned)((a.R + 63) / 64)), dim3(64), 0, st, env->d, g, extra...);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

// the checks every tube entry makes; `out` is its first output
static int tl_check(int64_t M, int32_t S, const double* p0, const double* depths, int64_t R, const void* out, const char* who)
{
    if (!p0 || !depths || !out) return fail(std::string(who) + ": null argument");
    if (M < 2) return fail(std::string(who) + ": need at least two rays (one ray tube)");
    if (M > INT32_MAX) return fail(std::string(who) + ": too many rays");
    if (S < 1 || S > 65535) return fail(std::string(who) + ": n_samples must be 1 .. 65535");
    if (R < 1 || R > (int64_t)65535 * 64) return fail(std::string(who) + ": n_depths must be 1 .. 4194240");
    return 0;
}

// The prologue of every entry on a fan handle: a fan with trajectories; under its lock, once its kernel has finished (its M
// is known then), the entry's check(M, S); the keep list and the save ranges uploaded on first use (held by the handle);
// then run(env, a) with the fan's TlArgs (the receivers and p0 unset).
template <typename Check, typename Run>
static int fan_entry(pgr_fan* f, const char* who, Check check, Run run)
{
    if (!f) return fail(std::string(who) + ": null fan");
    if (!f->save) return fail(std::string(who) + ": the fan was launched without trajectories (S = 0)");
    std::lock_guard<std::mutex> lock(f->m);
    HIPCHK(hipSetDevice(f->env->device));
    int rc = fan_finish(f);
    if (!rc) rc = check(f->M, f->S);
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
    TlArgs a{};
    a.Z = f->d.Z; a.P = f->d.P; a.T = f->d.T; a.keep = (f->M != f->N) ? f->d_keep : nullptr;
    a.N = f->N; a.M = f->M; a.S = f->S; a.blocked = f->blocked ? 1 : 0;
    a.zsign = (f->flags & PGR_STORED_SIGN) ? -1.0 : 1.0;
    a.x = f->d.r;
    return run(f->env, a);
}

// The prologue of the tube entries on a fan handle: fan_entry with tl_check before the entry's own check(S), and the
// receivers, p0 and the weights W (NULL: none) set.
template <typename Check, typename Run>
static int tl_fan_entry(pgr_fan* f, const double* p0, const double* W, const double* depths, int64_t R, const void* out,
                        const char* who, Check check, Run run)
{
    return fan_entry(f, who,
                     [&](int64_t M, int32_t S) {
                         const int rc = tl_check(M, S, p0, depths, R, out, who);
                         return rc ? rc : check(S);
                     },
                     [&](const pgr_env* e, TlArgs a) {
                         a.p0 = p0; a.W = W; a.depths = depths; a.R = R;
                         return run(e, a);
                     });
}

// The prologue of the entries on caller buffers z / p [S][N] (stored sign, every ray surviving), x [S] and with RAYS the
// travel times T, the weights W [S][N] (NULL: none): an environment, the buffers, tl_check and the entry's own check(S); then
// run(env, a) on env's device.
template <bool RAYS, typename Check, typename Run>
static int tl_buffer_entry(const pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                           int32_t n_samples, const double* x, const double* p0, const double* W, const double* depths,
                           int64_t R, const void* out, const char* who, Check check, Run run)
{
    if (!env) return fail(std::string(who) + ": null environment");
    if ((RAYS && !T) || !z || !p || !x) return fail(std::string(who) + ": null argument");
    int rc = tl_check(n_rays, n_samples, p0, depths, R, out, who);
    if (!rc) rc = check(n_samples);
    if (rc) return rc;
    HIPCHK(hipSetDevice(env->device));
    TlArgs a{};
    a.Z = z; a.P = p; a.T = T; a.keep = nullptr;
    a.N = n_rays; a.M = n_rays; a.S = n_samples; a.blocked = 0;
    a.zsign = -1.0;
    a.x = x; a.p0 = p0; a.W = W; a.depths = depths; a.R = R;
    return run(env, a);
}

static int tl_no_check(int32_t) { return 0; }

static int tl_intensity(const pgr_env* env, TlArgs a, double* out, void* stream, const char* who)
{
    a.out = out;
    return tube_run(env, a, TL_TUBES, pgr_tl_bounds, nullptr, 0, (hipStream_t)stream, who, pgr_tl_sum);
}

// the two entries and their weighted twins (`who`: the entry named in errors)
static int tl_fan_intensity(pgr_fan* f, const double* p0, const double* W, const double* depths, int64_t n_depths, double* out,
                            void* stream, const char* who)
{
    return tl_fan_entry(f, p0, W, depths, n_depths, out, who, tl_no_check,
                        [&](const pgr_env* e, TlArgs a) { return tl_intensity(e, a, out, stream, who); });
}

static int tl_buffer_intensity(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                               const double* x, const double* p0, const double* W, const double* depths, int64_t n_depths,
                               double* out, void* stream, const char* who)
{
    return tl_buffer_entry<false>(env, nullptr, z, p, n_rays, n_samples, x, p0, W, depths, n_depths, out, who, tl_no_check,
                                  [&](const pgr_env* e, TlArgs a) { return tl_intensity(e, a, out, stream, who); });
}

extern "C" int pgr_fan_intensity(pgr_fan* f, const double* p0, const double* depths, int64_t n_depths, double* out,
                                 void* stream)
{
    return tl_fan_intensity(f, p0, nullptr, depths, n_depths, out, stream, "pgr_fan_intensity");
}

extern "C" int pgr_fan_intensity_w(pgr_fan* f, const double* p0, const double* weights, const double* depths,
                                   int64_t n_depths, double* out, void* stream)
{
    return tl_fan_intensity(f, p0, weights, depths, n_depths, out, stream, "pgr_fan_intensity_w");
}

extern "C" int pgr_intensity_device(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                                    const double* x, const double* p0, const double* depths, int64_t n_depths, double* out,
                                    void* stream)
{
    return tl_buffer_intensity(env, z, p, n_rays, n_samples, x, p0, nullptr, depths, n_depths, out, stream,
                               "pgr_intensity_device");
}

extern "C" int pgr_intensity_device_w(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                                      const double* x, const double* p0, const double* weights, const double* depths,
                                      int64_t n_depths, double* out, void* stream)
{
    return tl_buffer_intensity(env, z, p, n_rays, n_samples, x, p0, weights, depths, n_depths, out, stream,
                               "pgr_intensity_device_w");
}

#endif  // PGR_TL_H
