// pgr_front.h -- time fronts and turning-point counts of a fan at chosen save columns: pgr_fan_time_front,
// pgr_time_front_device.  A per-ray product, as pgr_sens.h; it reads the fan where it lies.
// (Part of the ONE translation unit pgr_hip.hip, included there last; not a stand-alone header.)
//
// The quantity ("Time fronts and ray identifiers"): for surviving ray m with slowness samples
// p_m(s), s = 0 ... S - 1, and cls(v) = +1 (v > 0), -1 (v < 0), 0 (v == +-0), a NaN being a class that differs from every
// class, itself included,
//   change_m(s) = cls(p_m(s + 1)) differs from cls(p_m(s)) ? 1 : 0,            s = 0 ... S - 2,
//   turns[c][m] = sum over s < cols[c] of change_m(s)                          (0 for column 0),
// which is np.sum(np.diff(np.sign(ps[:, :col + 1]), axis=1) != 0, axis=1) entry for entry.  The time front of slot c is that
// count with T, z, p of the surviving rays at column cols[c], copied as the fan holds them.
//
// The count is a prefix sum along s, an integer, so any order of summation gives the same answer.  The host sorts the
// requested columns and cuts the changes 0 ... max(cols) - 1 into segments at them, and every gap longer than FRONT_SEG
// into pieces of FRONT_SEG.  Three passes on the caller's stream, no atomics, one lane per ray (a wave reads 64 consecutive
// rays of a row):
//   pgr_front_count  one workgroup per (block of 256 rays, segment): the segment's changes of each ray, into part[g][m];
//                    reads samples lo ... hi of p, so every sample up to max(cols) once plus one seam sample per segment,
//                    and nothing past max(cols);
//   pgr_front_scan   one lane per ray: part[g][m] becomes the running sum over the segments 0 ... g;
//   pgr_front_put    one lane per (ray, slot): the running sum in front of the slot's column and the samples there, to
//                    the caller's slot.
// Without `turns` only the last pass runs.  The scratch (the column tables and part) is a stream-ordered allocation freed
// behind the last pass.
#ifndef PGR_FRONT_H
#define PGR_FRONT_H

#include <algorithm>

#define FRONT_SEG 32   // changes per segment at most: 32 pieces of a 1001-sample row, 50 000 waves for a 1e5-ray fan

struct FrontArgs {
    TlArgs t;                 // the fan as pgr_tl.h reads it (T, Z, P, keep, N, M, S, blocked); the rest unused
    const int32_t* bnd;       // [nseg + 1]: segment g holds the changes bnd[g] ... bnd[g + 1] - 1
    int32_t nseg;
    const int32_t* slot_col;  // [ncol]: the column of slot c
    const int32_t* slot_seg;  // [ncol]: the segments in front of it (bnd[slot_seg[c]] == slot_col[c])
    int32_t ncol;
    int32_t nblk;             // blocks of 256 rays
    int32_t* part;            // [nseg][M]
    double* T_out;            // [ncol][M] each, any may be NULL
    double* z_out;
    double* p_out;
    int32_t* turns;
};

// 0 / 1 / 2: zero, positive, negative; 3: NaN
__device__ __forceinline__ int front_cls(double v) { return v > 0.0 ? 1 : (v < 0.0 ? 2 : (v == 0.0 ? 0 : 3)); }

__global__ void __launch_bounds__(256) pgr_front_count(FrontArgs a)
{
    const int g = blockIdx.x / a.nblk;
    const int64_t m = (int64_t)(blockIdx.x % a.nblk) * 256 + threadIdx.x;
    if (m >= a.t.M) return;
    const int lo = a.bnd[g], hi = a.bnd[g + 1];
    int prev = front_cls(a.t.P[tl_index(a.t, lo, m)]);
    int n = 0;
#pragma unroll 8
    for (int s = lo + 1; s <= hi; s++) {
        const int c = front_cls(a.t.P[tl_index(a.t, s, m)]);
        n += (c != prev || c == 3) ? 1 : 0;
        prev = c;
    }
    a.part[(int64_t)g * a.t.M + m] = n;
}

__global__ void __launch_bounds__(256) pgr_front_scan(FrontArgs a)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.t.M) return;
    int run = 0;
#pragma unroll 8
    for (int g = 0; g < a.nseg; g++) {
        int32_t* q = a.part + (int64_t)g * a.t.M + m;
        run += *q;
        *q = run;
    }
}

__global__ void __launch_bounds__(256) pgr_front_put(FrontArgs a)
{
    const int c = blockIdx.x / a.nblk;
    const int64_t m = (int64_t)(blockIdx.x % a.nblk) * 256 + threadIdx.x;
    if (m >= a.t.M) return;
    const int64_t i = tl_index(a.t, a.slot_col[c], m), o = (int64_t)c * a.t.M + m;
    if (a.T_out) a.T_out[o] = a.t.T[i];
    if (a.z_out) a.z_out[o] = a.t.Z[i];
    if (a.p_out) a.p_out[o] = a.t.P[i];
    if (a.turns) {
        const int k = a.slot_seg[c];
        a.turns[o] = k ? a.part[(int64_t)(k - 1) * a.t.M + m] : 0;
    }
}

// the checks of both entries
static int front_check(int64_t M, int32_t S, const int32_t* cols, int32_t n_cols, const void* T_out, const void* z_out,
                       const void* p_out, const void* turns, const char* who)
{
    if (!cols) return fail(std::string(who) + ": null cols");
    if (!T_out && !z_out && !p_out && !turns) return fail(std::string(who) + ": every output is NULL");
    if (M < 1) return fail(std::string(who) + ": need at least one ray");
    if (M > INT32_MAX) return fail(std::string(who) + ": too many rays");
    if (S < 1) return fail(std::string(who) + ": n_samples must be >= 1");
    if (n_cols < 1 || n_cols > 65535) return fail(std::string(who) + ": n_cols must be 1 .. 65535");
    for (int32_t c = 0; c < n_cols; c++)
        if (cols[c] < 0 || cols[c] >= S) return fail(std::string(who) + ": a column is outside 0 .. n_samples - 1");
    return 0;
}

// the passes on `stream` for the HOST list cols[n_cols] (checked)
static int front_run(TlArgs t, const int32_t* cols, int32_t n_cols, double* T_out, double* z_out, double* p_out,
                     int32_t* turns, void* stream, const char* who)
{
    const hipStream_t st = (hipStream_t)stream;
    FrontArgs a{};
    a.t = t;
    a.ncol = n_cols;
    a.nblk = (int32_t)((t.M + 255) / 256);
    a.T_out = T_out; a.z_out = z_out; a.p_out = p_out; a.turns = turns;
    // the tables: segment bounds (cuts at the sorted requested columns, gaps in pieces of FRONT_SEG), then per slot its
    // column and the segments in front of it
    std::vector<int32_t> sorted(cols, cols + n_cols), tab;
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    if (turns) {
        tab.push_back(0);
        for (int32_t u : sorted)
            while (tab.back() < u) tab.push_back(std::min(tab.back() + FRONT_SEG, u));
        a.nseg = (int32_t)tab.size() - 1;
    }
    const size_t nbnd = tab.size();
    tab.insert(tab.end(), cols, cols + n_cols);
    for (int32_t c = 0; c < n_cols; c++)
        tab.push_back(turns ? (int32_t)(std::lower_bound(tab.begin(), tab.begin() + (ptrdiff_t)nbnd, cols[c]) - tab.begin()) : 0);
    if ((int64_t)a.nblk * std::max(a.nseg, a.ncol) > INT32_MAX)
        return fail(std::string(who) + ": too many rays times columns for one launch");
    const size_t ntab = (tab.size() * sizeof(int32_t) + 15) & ~(size_t)15;
    void* b = nullptr;
    if (hipMallocAsync(&b, ntab + (size_t)a.nseg * (size_t)t.M * sizeof(int32_t) + 16, st) != hipSuccess)
        return fail(std::string(who) + ": device allocation of the scratch failed");
    a.bnd = (const int32_t*)b;
    a.slot_col = a.bnd + nbnd;
    a.slot_seg = a.slot_col + n_cols;
    a.part = (int32_t*)((char*)b + ntab);
    hipError_t e = hipMemcpyAsync(b, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && a.nseg > 0) {
        hipLaunchKernelGGL(pgr_front_count, dim3((unsigned)(a.nblk * a.nseg)), dim3(256), 0, st, a);
        e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(pgr_front_scan, dim3((unsigned)a.nblk), dim3(256), 0, st, a);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pgr_front_put, dim3((unsigned)(a.nblk * a.ncol)), dim3(256), 0, st, a);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(b, st);
    if (e != hipSuccess) return fail(std::string(who) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

extern "C" int pgr_fan_time_front(pgr_fan* f, const int32_t* cols, int32_t n_cols, double* T_out, double* z_out,
                                  double* p_out, int32_t* turns, void* stream)
{
    const char* who = "pgr_fan_time_front";
    return fan_entry(f, who,
                     [&](int64_t M, int32_t S) { return front_check(M, S, cols, n_cols, T_out, z_out, p_out, turns, who); },
                     [&](const pgr_env*, TlArgs t) { return front_run(t, cols, n_cols, T_out, z_out, p_out, turns, stream, who); });
}

extern "C" int pgr_time_front_device(int device, const double* T, const double* z, const double* p, int64_t n_rays,
                                     int32_t n_samples, const int32_t* cols, int32_t n_cols, double* T_out, double* z_out,
                                     double* p_out, int32_t* turns, void* stream)
{
    const char* who = "pgr_time_front_device";
    int rc = front_check(n_rays, n_samples, cols, n_cols, T_out, z_out, p_out, turns, who);
    if (rc) return rc;
    if ((T_out && !T) || (z_out && !z) || ((p_out || turns) && !p))
        return fail(std::string(who) + ": an output is asked for whose input is NULL");
    HIPCHK(hipSetDevice(device));
    TlArgs t{};
    t.T = T; t.Z = z; t.P = p; t.keep = nullptr;
    t.N = n_rays; t.M = n_rays; t.S = n_samples; t.blocked = 0;
    return front_run(t, cols, n_cols, T_out, z_out, p_out, turns, stream, who);
}

#endif  // PGR_FRONT_H
