// pgr_host.h -- host side, common part: error string, PGR_TRACE marks, HIPCHK, the environment object (struct pgr_env) and its
// stream, grow-only and scoped buffers, the layout of a fan's device buffers (FanBufs), np.linspace's save ranges, and what
// the library says about its own build (pgr_build_info).
// (Part of the ONE translation unit pgr_hip.hip, included there in this order; not a stand-alone header.)
#ifndef PGR_HOST_H
#define PGR_HOST_H

// ====================================================================================
// host side
// ====================================================================================
static thread_local std::string g_err;

// PGR_TRACE=1 in the environment: wall-clock marks of the host-pointer paths on stderr (diagnostics)
static bool trace_on() { static const bool on = getenv("PGR_TRACE") != nullptr; return on; }
static double trace_now()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
#define PGR_MARK(t0, what) do { if (trace_on()) fprintf(stderr, "[pgr] %8.2f ms  %s\n", trace_now() - (t0), what); } while (0)

static int fail(const std::string& m)
{
    g_err = m;
    return -1;
}
#define HIPCHK(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(std::string(#call) + ": " + hipGetErrorString(e_));                \
    } while (0)

struct pgr_env {
    int device = 0;
    // tuning options of THIS environment (pgr_env_set_option; per-ray results never depend on them).
    // No process-wide state: two host threads driving two GPUs keep two environments.
    int waves_per_block = 0;          // 0 = automatic
    int depth_search = 0;             // 0: automatic, 1: binary search only, 2: bucket table but no index polynomial (tests)
    int park_lanes = 64, park_trips = 10;
    int place = 2;                    // 0 off, 1 issue priorities only, 2 cost-aware placement + priorities
    int api_blocked = 1;              // host-pointer entry / fan handles: HBM-table trajectory fans run the sample-blocked kernel (un-blocked on the way out)
    int d2h_register = 1;             // pipelined D2H copy: page-lock the destination sub-jobs (0: never -- every sub-job goes the "registration failed" way)
    int persistent = 1;               // fans of several rounds: persistent waves claiming packets from the cost-sorted list (0: whole workgroups, static)
    hipStream_t stream = nullptr;     // the host-pointer entry's own stream (env_stream: created on first use)
    EnvDev d{};
    const EnvDev* d_dev = nullptr;  // device copy of `d` (kernel argument by pointer)
    // grow-only staging workspace of the host-pointer entry and of the eigenray loop (kept while <= 16 GB so the many
    // small fans of an eigenray search do not pay 11 hipMalloc/hipFree per call)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    // device buffers of destroyed pgr_fan handles, kept for the next one (hipMalloc + hipFree of 2.4 GB per fan cost
    // more than the kernel's launch; hipFree also waits for the whole device): at most 4 buffers / 64 GB
    std::vector<std::pair<void*, size_t>> fan_pool;
    std::mutex fan_pool_mutex;
    // device-resident fans (pgr_fan_*) that still point at this environment, and whether pgr_env_destroy has been called
    // meanwhile (the last fan to go then releases the environment): both under fan_pool_mutex
    int live_fans = 0;
    bool doomed = false;
    void* stage = nullptr;   // page-locked host staging of the compacted per-ray fetch (grow-only)
    size_t stage_bytes = 0;
    void* ws2 = nullptr;   // second grow-only workspace: the squeezed trajectories (un-blocked, or compacted by PGR_COMPACT)
    size_t ws2_bytes = 0;
    std::mutex ws_mutex;
    // small buffers for the per-launch wave placement (cost[waves] + map[slots]): a slot is handed to a launch and
    // an event is recorded on that launch's stream behind its fan kernel; the slot is taken again only when the
    // event has completed -- however many launches are in flight on however many user streams, none reads a map
    // another launch is writing (the pool grows instead)
    struct PlaceSlot {
        void* buf = nullptr;
        size_t bytes = 0;
        hipEvent_t ev = nullptr;
        bool in_flight = false;   // claimed by a launch ...
        bool recorded = false;    // ... whose event has been recorded for THIS use (only then may hipEventQuery release it)
    };
    std::vector<PlaceSlot> place_slots;
    std::mutex place_mutex;
    int range_indep = 0;
    int lds_path = 0;
    std::vector<void*> allocs;
    int num_cus = 256;
    size_t max_lds = 64 * 1024;
    // the fan-kernel instance and launch shape of the LAST pgr_shoot_fan_device on this environment (pgr_debug_last_instance:
    // the test that walks every instance asserts that it launched the one it meant to)
    // (atomics: two host threads may launch on one environment; the record is a diagnostic, each field is whole)
    std::atomic<int> last_instance[8];
    std::atomic<int> last_instance_log{-1};   // LOG of that instance (pgr_debug_last_instance_log)
    pgr_env() { for (int q = 0; q < 8; q++) last_instance[q].store(q < 4 ? -1 : 0, std::memory_order_relaxed); }
};

extern "C" const char* pgr_last_error(void) { return g_err.c_str(); }

// the environment's own stream, created on first use (callers that hold ws_mutex create it before they take the lock)
static int env_stream(pgr_env* env)
{
    if (env->stream) return 0;
    std::lock_guard<std::mutex> lock(env->ws_mutex);
    if (!env->stream) HIPCHK(hipStreamCreateWithFlags(&env->stream, hipStreamNonBlocking));
    return 0;
}

// Grow-only buffer (device memory, page-locked host memory with `host`): kept when it holds `bytes` already, else freed and
// allocated anew.  A failed allocation leaves (nullptr, 0), clears the HIP error state and returns false.
static bool grow_buffer(void*& p, size_t& have, size_t bytes, bool host = false)
{
    if (bytes <= have) return true;
    if (p) (void)(host ? hipHostFree(p) : hipFree(p));
    have = 0;
    if ((host ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes)) == hipSuccess) { have = bytes; return true; }
    p = nullptr;
    (void)hipGetLastError();
    return false;
}

// scoped device buffer (the debug entries)
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8) == hipSuccess ? 0 : -1; }
};

// One block cut into consecutive 256-byte aligned pieces.  The same cuts run twice: with base == nullptr for the block's
// size (`total`; the pointers stay null), then on the block itself.
struct Carve {
    char* base = nullptr;
    size_t total = 0;
    template <class T> T* take(size_t count)
    {
        const size_t o = total;
        total += (count * sizeof(T) + 255) & ~(size_t)255;
        return base ? (T*)(base + o) : nullptr;
    }
};

// A fan's device buffers (the host-pointer entry's workspace, a pgr_fan handle's block), in their order in the block
struct FanBufs {
    double *y0, *r, *T, *Z, *P, *end;
    int32_t *nb, *ns, *st, *n1, *n2;
};

// y0 [N][3]; r [S] (one double without trajectories); T, Z, P [S][N] (sample-blocked: [ceil(S/4)][N][4]); end [N][3];
// n_bott, n_surf, status, n_steps, n_rej [N].  `bytes`: the block's size.
static FanBufs fan_carve(void* base, int64_t N, int32_t S, bool save, bool blocked, size_t* bytes = nullptr)
{
    const size_t n = (size_t)N, ns = !save ? 0 : n * (size_t)(blocked ? 4 * ((S + 3) / 4) : S);
    Carve c{(char*)base};
    FanBufs b;
    b.y0 = c.take<double>(3 * n); b.r = c.take<double>(save ? (size_t)S : 1);
    b.T = c.take<double>(ns); b.Z = c.take<double>(ns); b.P = c.take<double>(ns); b.end = c.take<double>(3 * n);
    b.nb = c.take<int32_t>(n); b.ns = c.take<int32_t>(n); b.st = c.take<int32_t>(n); b.n1 = c.take<int32_t>(n); b.n2 = c.take<int32_t>(n);
    if (bytes) *bytes = c.total;
    return b;
}

static size_t fan_bytes(int64_t N, int32_t S, bool save, bool blocked) { size_t b = 0; fan_carve(nullptr, N, S, save, blocked, &b); return b; }

// np.linspace(x0, x1, S)[j] to the bit: j * step + x0 (the last one x1), the product rounded before the sum whatever the
// host compiler's contraction setting
static double linspace_at(double x0, double x1, int32_t S, int32_t j)
{
    if (S > 1 && j == S - 1) return x1;
    volatile double m = (double)j * (S > 1 ? (x1 - x0) / (double)(S - 1) : 0.0);
    return m + x0;
}

// What the build did to this library: the second pass of the build (pygenray_amd/_isa_layout.py, run
// by pygenray_amd/_lib.py) re-encodes the device code and, when it has succeeded, overwrites this tag
// in the host object -- "plain hipcc" means the pass did not run or failed and the unmodified hipcc
// output is what is loaded.  The arithmetic switches come from the preprocessor.
extern "C" {
__attribute__((used)) char pgr_build_tag[96] = "PGR_BUILD_TAG:plain hipcc                                                                     ";
}
extern "C" const char* pgr_build_info(void)
{
    static std::string info;
    static std::once_flag once;
    std::call_once(once, [] {
        std::string t(pgr_build_tag + 14);
        while (!t.empty() && t.back() == ' ') t.pop_back();
        info = "layout: " + t + "; arithmetic: ";
#ifdef PGR_FMA
        info += "FMA contraction allowed (the PGR_ARITH=contracted opt-in: NOT the reference's bits, no bit-parity claim)";
#else
        info += "reference order, correctly rounded div/sqrt/pow/asin/sin";
#endif
    });
    return info.c_str();
}

extern "C" int pgr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { fail("hipGetDeviceCount failed"); return -1; }
    return n;
}

#endif  // PGR_HOST_H
