// pgr_sens.h -- travel-time sensitivity kernels of a fan on a range-depth grid: pgr_fan_travel_time_kernel,
// pgr_travel_time_kernel_device.  The first per-ray product (the tube products of pgr_tl.h work on pairs of rays).
// (Part of the ONE translation unit pgr_hip.hip, included there last; not a stand-alone header.)
//
// The quantity (DESIGN.md section "Travel-time sensitivity kernels"): K[m, a, b] = dT_m / dc_ab on the grid g[A] x h[B],
// phi_ab the bilinear basis of host_physics.bilinear_interp (clamped cell, unclamped weights).  Ray m's path to column
// `col` is the polyline through its samples 0 ... col.  Chord s -> s + 1 is cut at the interior grid lines it crosses
// strictly inside; on each piece (length l) Simpson's rule at 0, 1/2, 1 gives
//   Q_ab(s) += l/6 [f(0) + 4 f(1/2) + f(1)],  f = phi_ab / c^2,     Q_1(s) += l/6 [g(0) + 4 g(1/2) + g(1)],  g = 1 / c,
// c the look-up of pgr_tl.h (Ctx<false, 0>::lookup).  beta_s = (T(s+1) - T(s)) / Q_1(s) (0 when Q_1 == 0), and
//   K[m, a, b] = sum over s, in increasing s from 0.0, of  - beta_s Q_ab(s).
// A NaN in T or the depth at samples 0 ... col makes the row NaN.
//
// Pieces.  On each axis the chord's start cell is the cell it leaves its start point into (searchsorted side 'right' - 1
// going up, 'left' - 1 going down or standing still; clamped to the grid's cells), and the cut of line l sits at the
// parameter u_l = (G_l - q0) / (q1 - q0), monotone along the chord.  Every cut moves the cell by one.  The pieces in range
// cell i (its sub-chord [pa, pb], the cuts of the lines on either side, 0 and 1 at the ends) are cut again by the depth cuts
// with pa < v < pb; the piece k of the sub-chord lies in depth cell j_first + k (its direction), j_first = the cell after
// the depth cuts with v <= pa.  So a piece's cell is counted, not found from its midpoint: mathematically the same cell,
// and immune to the rounding of a midpoint that sits on a grid line.  A zero-length sub-chord (pa == pb) is skipped; a
// zero-length piece adds exactly 0.
//
// Three passes on the caller's stream, no atomics:
//   pgr_ttk_seg   one block per ray: beta_s for every chord (one lane walks its chord's pieces in order, so Q_1 is the
//                 sequential sum), and the row's finiteness flag;
//   pgr_ttk_span  one block per range node a: the first and last chord that reaches a cell of node a (a - 1 or a);
//   pgr_ttk_sum   one wave per (ray, range node a): the depth cells its chords reach, then, tile by tile of TTK_TILE depth
//                 nodes, zeros for the tiles they miss and, for the others, a walk of the chords in increasing s: lane t
//                 evaluates the piece of depth cell tile0 - 1 + t in range cell a - 1 and a, and node b = tile0 + t adds
//                 its two neighbouring cells' terms (lanes t and t + 1, by a shuffle) in chord order.  Each K entry is
//                 formed by one lane in the order of the definition, and every entry of the row is written once.
#ifndef PGR_SENS_H
#define PGR_SENS_H

#define TTK_TILE 63   // depth nodes per tile: the tile's 64 cells (tile0 - 1 ... tile0 + 62) are one per lane

struct TtkArgs {
    TlArgs t;             // the fan as pgr_tl.h reads it (Z, T, keep, N, M, S, blocked, zsign, x); the rest unused
    const double* g;      // kernel ranges [A], ascending, in the frame the fan was traced in
    const double* h;      // kernel depths [B], ascending
    int32_t A, B;
    int32_t col;          // the paths end at sample col
    double* beta;         // [M][col]
    int32_t* ok;          // [M]: row m has no NaN sample
    int32_t* span;        // [A][2]: first, last chord reaching range node a (none: col, -1)
    double* out;          // [M][A][B]
};

// #(G[0 .. n) <= q) (le) or #(G[0 .. n) < q): np.searchsorted side 'right' / 'left'
__device__ __forceinline__ int ttk_count(const double* G, int n, double q, bool le)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (le ? (G[mid] <= q) : (G[mid] < q)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One axis of a chord q0 -> q1 on the grid G[n]: direction, start cell, and the nc cuts in chord order (cut r is line
// first + dir * r, at parameter cut(r)); after r cuts the chord is in cell(r).
struct TtkAxis {
    double q0, dq;
    int dir, cell0, first, nc;
    __device__ __forceinline__ double cut(const double* G, int r) const { return fdiv(G[first + dir * r] - q0, dq); }
    __device__ __forceinline__ int cell(int r) const { return cell0 + dir * r; }
    // the r with cell(r) == i (-1 when the chord does not visit cell i)
    __device__ __forceinline__ int visit(int i) const
    {
        const int r = (i - cell0) * (dir ? dir : 1);
        return (r >= 0 && r <= nc) ? r : -1;
    }
    // #(cuts at a parameter <= p) (le) or < p
    __device__ __forceinline__ int count(const double* G, double p, bool le) const
    {
        int lo = 0, hi = nc;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const double v = cut(G, mid);
            if (le ? (v <= p) : (v < p)) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
};

__device__ __forceinline__ TtkAxis ttk_axis(const double* G, int n, double q0, double q1)
{
    TtkAxis x;
    x.q0 = q0;
    x.dq = q1 - q0;
    x.dir = (q1 > q0) ? 1 : ((q1 < q0) ? -1 : 0);
    int lo = 1, hi = 0;
    if (x.dir > 0) {
        const int c = ttk_count(G, n, q0, true);
        x.cell0 = c - 1;
        lo = max(c, 1);
        hi = min(ttk_count(G, n, q1, false) - 1, n - 2);
        x.first = lo;
    } else {
        const int c = ttk_count(G, n, q0, false);
        x.cell0 = c - 1;
        if (x.dir < 0) {
            lo = max(ttk_count(G, n, q1, true), 1);
            hi = min(c - 1, n - 2);
        }
        x.first = hi;
    }
    x.cell0 = min(max(x.cell0, 0), n - 2);
    x.nc = max(hi - lo + 1, 0);
    return x;
}

// does a chord whose range axis is X reach a cell of range node ia (ia - 1 or ia)?
__device__ __forceinline__ bool ttk_reaches(const TtkAxis& X, int ia)
{
    const int c1 = X.cell(X.nc);
    return min(X.cell0, c1) <= ia && max(X.cell0, c1) >= ia - 1;
}

// chord s -> s + 1 of ray m (finite samples): start, extent, length, travel-time step and both axes
struct TtkChord {
    double x0, d0, dx, dd, L, dT;
    TtkAxis X, D;
    __device__ __forceinline__ double px(double u) const { return x0 + u * dx; }
    __device__ __forceinline__ double pd(double u) const { return d0 + u * dd; }
};

__device__ __forceinline__ TtkChord ttk_chord(const TtkArgs& a, int64_t m, int s)
{
    TtkChord c;
    const int64_t i0 = tl_index(a.t, s, m), i1 = tl_index(a.t, s + 1, m);
    c.x0 = a.t.x[s];
    const double x1 = a.t.x[s + 1];
    c.d0 = a.t.zsign * a.t.Z[i0];
    const double d1 = a.t.zsign * a.t.Z[i1];
    c.dx = x1 - c.x0;
    c.dd = d1 - c.d0;
    c.L = fsqrt(c.dx * c.dx + c.dd * c.dd);
    c.dT = a.t.T[i1] - a.t.T[i0];
    c.X = ttk_axis(a.g, a.A, c.x0, x1);
    c.D = ttk_axis(a.h, a.B, c.d0, d1);
    return c;
}

// 1 / c at the chord's point u
__device__ __forceinline__ double ttk_ic(const Ctx<false, 0>& C, const TtkChord& ch, double u)
{
    double c, cp;
    C.lookup(ch.px(u), ch.pd(u), c, cp);
    return fdiv(1.0, c);
}

// The sub-chord of chord ch in range cell i (visit r): its parameter interval [pa, pb], the depth cuts before it (r0) and
// inside it (nin; pieces 0 ... nin).  False for a cell the chord does not visit or a zero-length sub-chord.
struct TtkSub { double pa, pb; int r0, nin; };

__device__ __forceinline__ bool ttk_sub(const TtkArgs& a, const TtkChord& ch, int r, TtkSub& u)
{
    if (r < 0) return false;
    u.pa = r == 0 ? 0.0 : ch.X.cut(a.g, r - 1);
    u.pb = r == ch.X.nc ? 1.0 : ch.X.cut(a.g, r);
    if (!(u.pa < u.pb)) return false;
    u.r0 = ch.D.count(a.h, u.pa, true);
    u.nin = ch.D.count(a.h, u.pb, false) - u.r0;
    return true;
}

// piece k of sub-chord u: [p, q]
__device__ __forceinline__ void ttk_piece(const TtkArgs& a, const TtkChord& ch, const TtkSub& u, int k, double& p, double& q)
{
    p = k == 0 ? u.pa : ch.D.cut(a.h, u.r0 + k - 1);
    q = k == u.nin ? u.pb : ch.D.cut(a.h, u.r0 + k);
}

__device__ __forceinline__ int ttk_wave_min(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int ttk_wave_max(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// Pass 1: one block per ray m.  Lane-strided over the chords s < col: beta_s, its chord's pieces walked in order (range
// sub-chords in chord order, depth pieces in order within each), c at a piece's end reused as the next piece's start (the
// same point: a point is a function of its parameter alone).  ok[m]: no NaN in T or depth at samples 0 ... col.
__global__ void __launch_bounds__(256) pgr_ttk_seg(EnvDev env, TtkArgs a)
{
    __shared__ int bad;
    const int64_t m = blockIdx.x;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int s = threadIdx.x; s <= a.col; s += blockDim.x) {
        const int64_t i = tl_index(a.t, s, m);
        const double T = a.t.T[i], d = a.t.Z[i];
        if (!(T == T && d == d)) bad = 1;       // (every writer stores the same value)
    }
    __syncthreads();
    const bool row = !bad;
    if (threadIdx.x == 0) a.ok[m] = row ? 1 : 0;
    if (!row) return;                          // (uniform in the block)
    const Ctx<false, 0> C(env, nullptr);
    for (int s = threadIdx.x; s < a.col; s += blockDim.x) {
        const TtkChord ch = ttk_chord(a, m, s);
        double Q1 = 0.0;
        double ic0 = ttk_ic(C, ch, 0.0);
        for (int r = 0; r <= ch.X.nc; r++) {
            TtkSub u;
            if (!ttk_sub(a, ch, r, u)) continue;
            for (int k = 0; k <= u.nin; k++) {
                double p, q;
                ttk_piece(a, ch, u, k, p, q);
                const double w6 = fdiv((q - p) * ch.L, 6.0);
                const double icm = ttk_ic(C, ch, 0.5 * (p + q)), ic1 = ttk_ic(C, ch, q);
                Q1 = Q1 + w6 * ((ic0 + 4.0 * icm) + ic1);
                ic0 = ic1;
            }
        }
        a.beta[m * a.col + s] = Q1 != 0.0 ? fdiv(ch.dT, Q1) : 0.0;
    }
}

// Pass 2 (ray independent): one block per range node ia, the first and last chord reaching one of its cells.
__global__ void __launch_bounds__(256) pgr_ttk_span(TtkArgs a)
{
    __shared__ int lo[256], hi[256];
    const int ia = blockIdx.x, t = threadIdx.x;
    int l = a.col, h = -1;
    for (int s = t; s < a.col; s += 256) {
        if (ttk_reaches(ttk_axis(a.g, a.A, a.t.x[s], a.t.x[s + 1]), ia)) {
            l = min(l, s);
            h = max(h, s);
        }
    }
    lo[t] = l;
    hi[t] = h;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            lo[t] = min(lo[t], lo[t + w]);
            hi[t] = max(hi[t], hi[t + w]);
        }
        __syncthreads();
    }
    if (t == 0) {
        a.span[2 * ia] = lo[0];
        a.span[2 * ia + 1] = hi[0];
    }
}

// Pass 3: one wave per (ray blockIdx.x, range node blockIdx.y); writes K[m, ia, 0 ... B) once, entry by entry.
__global__ void __launch_bounds__(64) pgr_ttk_sum(EnvDev env, TtkArgs a)
{
    const int64_t m = blockIdx.x;
    const int ia = blockIdx.y, t = threadIdx.x;
    double* o = a.out + ((int64_t)m * a.A + ia) * a.B;
    if (!a.ok[m]) {
        for (int b = t; b < a.B; b += 64) o[b] = NAN;
        return;
    }
    const int s_lo = a.span[2 * ia], s_hi = a.span[2 * ia + 1];
    // the depth cells reached by the chords that reach node ia: tiles outside [jlo, jhi] are zero
    int jlo = 0x7fffffff, jhi = -1;
    for (int s = s_lo + t; s <= s_hi; s += 64) {
        const TtkChord ch = ttk_chord(a, m, s);
        if (ttk_reaches(ch.X, ia)) {
            const int c1 = ch.D.cell(ch.D.nc);
            jlo = min(jlo, min(ch.D.cell0, c1));
            jhi = max(jhi, max(ch.D.cell0, c1));
        }
    }
    jlo = ttk_wave_min(jlo);
    jhi = ttk_wave_max(jhi);
    const Ctx<false, 0> C(env, nullptr);
    for (int tile0 = 0; tile0 < a.B; tile0 += TTK_TILE) {
        double acc = 0.0;
        if (jlo <= tile0 + TTK_TILE - 1 && jhi >= tile0 - 1) {
            const int j = tile0 - 1 + t;                       // the lane's depth cell
            const bool cell = j >= 0 && j <= a.B - 2;
            for (int s = s_lo; s <= s_hi; s++) {
                const TtkChord ch = ttk_chord(a, m, s);
                if (!ttk_reaches(ch.X, ia)) continue;
                const double beta = a.beta[m * a.col + s];
                double q = 0.0;
                for (int e = 0; e < 2; e++) {
                    const int i = ch.X.dir >= 0 ? ia - 1 + e : ia - e;   // the range cells of node ia in chord order
                    TtkSub u;
                    if (i < 0 || i > a.A - 2 || !ttk_sub(a, ch, ch.X.visit(i), u)) continue;
                    double vlo = 0.0, vhi = 0.0;                       // the lane's piece's terms at nodes j, j + 1
                    const int k = cell ? (j - ch.D.cell0) * (ch.D.dir ? ch.D.dir : 1) - u.r0 : -1;
                    if (k >= 0 && k <= u.nin) {
                        double p, pq;
                        ttk_piece(a, ch, u, k, p, pq);
                        const double w6 = fdiv((pq - p) * ch.L, 6.0);
                        const double g0 = a.g[i], g1 = a.g[i + 1], h0 = a.h[j], h1 = a.h[j + 1];
                        const double uu[3] = {p, 0.5 * (p + pq), pq};
                        double flo[3], fhi[3];
                        for (int n = 0; n < 3; n++) {
                            const double ic = ttk_ic(C, ch, uu[n]), sq = ic * ic;
                            const double wx = fdiv(ch.px(uu[n]) - g0, g1 - g0), wy = fdiv(ch.pd(uu[n]) - h0, h1 - h0);
                            const double rf = i == ia ? (1 - wx) : wx;
                            flo[n] = (rf * (1 - wy)) * sq;
                            fhi[n] = (rf * wy) * sq;
                        }
                        vlo = w6 * ((flo[0] + 4.0 * flo[1]) + flo[2]);
                        vhi = w6 * ((fhi[0] + 4.0 * fhi[1]) + fhi[2]);
                    }
                    // node tile0 + t: cell tile0 + t - 1 (this lane, its upper node) and cell tile0 + t (lane t + 1, its
                    // lower node), in chord order
                    const double vlo1 = __shfl_down(vlo, 1);
                    q = ch.D.dir >= 0 ? (q + vhi) + vlo1 : (q + vlo1) + vhi;
                }
                acc = acc - beta * q;
            }
        }
        const int b = tile0 + t;
        if (t < TTK_TILE && b < a.B) o[b] = acc;
    }
}

// the checks of both entries
static int ttk_check(int64_t M, int32_t S, const double* g, int32_t A, const double* h, int32_t B, int32_t col,
                     const void* out, const char* who)
{
    if (!g || !h || !out) return fail(std::string(who) + ": null argument");
    if (M < 1) return fail(std::string(who) + ": need at least one ray");
    if (M > (1 << 24)) return fail(std::string(who) + ": too many rays (at most 16777216)");
    if (S < 1) return fail(std::string(who) + ": n_samples must be >= 1");
    if (A < 2 || A > 65535) return fail(std::string(who) + ": n_ranges must be 2 .. 65535");
    if (B < 2 || B > (1 << 30)) return fail(std::string(who) + ": n_depths must be 2 .. 1073741824");
    if (col < 0 || col >= S) return fail(std::string(who) + ": column must be 0 .. n_samples - 1");
    return 0;
}

// the three passes on `st`; the scratch (beta, ok, span) is a stream-ordered allocation freed behind the last pass
static int ttk_run(const pgr_env* env, TtkArgs a, void* stream, const char* who)
{
    const hipStream_t st = (hipStream_t)stream;
    const size_t nbeta = (size_t)a.t.M * (size_t)a.col * sizeof(double), nok = (size_t)a.t.M * sizeof(int32_t);
    void* b = nullptr;
    if (hipMallocAsync(&b, nbeta + nok + (size_t)a.A * 2 * sizeof(int32_t) + 16, st) != hipSuccess)
        return fail(std::string(who) + ": device allocation of the scratch failed");
    a.beta = (double*)b;
    a.ok = (int32_t*)((char*)b + nbeta);
    a.span = a.ok + a.t.M;
    hipLaunchKernelGGL(pgr_ttk_seg, dim3((unsigned)a.t.M), dim3(256), 0, st, env->d, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_ttk_span, dim3((unsigned)a.A), dim3(256), 0, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_ttk_sum, dim3((unsigned)a.t.M, (unsigned)a.A), dim3(64), 0, st, env->d, a);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

static TtkArgs ttk_args(const TlArgs& t, const double* g, int32_t A, const double* h, int32_t B, int32_t col, double* out)
{
    TtkArgs a{};
    a.t = t;
    a.g = g; a.A = A;
    a.h = h; a.B = B;
    a.col = col;
    a.out = out;
    return a;
}

extern "C" int pgr_fan_travel_time_kernel(pgr_fan* f, const double* ranges, int32_t n_ranges, const double* depths,
                                          int32_t n_depths, int32_t column, double* out, void* stream)
{
    const char* who = "pgr_fan_travel_time_kernel";
    return fan_entry(f, who,
                     [&](int64_t M, int32_t S) {
                         return ttk_check(M, S, ranges, n_ranges, depths, n_depths, column, out, who);
                     },
                     [&](const pgr_env* e, TlArgs t) {
                         return ttk_run(e, ttk_args(t, ranges, n_ranges, depths, n_depths, column, out), stream, who);
                     });
}

extern "C" int pgr_travel_time_kernel_device(pgr_env* env, const double* T, const double* z, int64_t n_rays,
                                             int32_t n_samples, const double* x, const double* ranges, int32_t n_ranges,
                                             const double* depths, int32_t n_depths, int32_t column, double* out,
                                             void* stream)
{
    const char* who = "pgr_travel_time_kernel_device";
    if (!env) return fail(std::string(who) + ": null environment");
    if (!T || !z || !x) return fail(std::string(who) + ": null argument");
    int rc = ttk_check(n_rays, n_samples, ranges, n_ranges, depths, n_depths, column, out, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(env->device));
    TlArgs t{};
    t.Z = z; t.T = T; t.keep = nullptr;
    t.N = n_rays; t.M = n_rays; t.S = n_samples; t.blocked = 0;
    t.zsign = -1.0;
    t.x = x;
    return ttk_run(env, ttk_args(t, ranges, n_ranges, depths, n_depths, column, out), stream, who);
}

#endif  // PGR_SENS_H
