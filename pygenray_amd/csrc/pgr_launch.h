// pgr_launch.h -- launching a fan: per-launch wave scheduling (placement slots, pgr_wave_cost / pgr_wave_place), the ONE statement of
// which pgr_fan_kernel instances exist (fan_instance_exists: the instance table and every refusal follow from it), the ONE LDS
// layout (lds_layout), and pgr_shoot_fan_device in four steps -- argument checks, instance selection, launch shape, launch;
// whether the host entries run a fan sample-blocked (fan_blocked).
// (Part of the ONE translation unit pgr_hip.hip, included there in this order; not a stand-alone header.)
#ifndef PGR_LAUNCH_H
#define PGR_LAUNCH_H

// The shape of a launch: waves per workgroup and grid, and what schedule_waves adds where it is on and useful -- the
// slot -> wave map (null: the strided deal) and, for persistent waves, the packet queue (FanArgs has their meaning)
struct FanShape {
    int wpb = 0;
    int64_t blocks = 0;
    const int* map = nullptr;
    int* queue = nullptr;
    int n_queue = 0, n_tail = 0;
};

// Builds the slot -> wave map for this launch on `st` (see pgr_wave_place) and sets the grid that goes with it, or leaves map
// null.  The placement slot goes out through `slot_out` the moment it is claimed: PlaceGuard releases it on every return after that.
static int schedule_waves(pgr_env* env, const double* y0, int64_t N, int64_t waves, int W, hipStream_t st, bool persist_ok,
                          int& slot_out, FanShape& out)
{
    slot_out = -1;
    if (env->place == 0 || env->waves_per_block != 0 || W < 5 || waves > (1 << 27)) return 0;
    const int64_t cus = env->num_cus;
    int mode, B;
    if (waves <= (int64_t)W * cus && W <= 8 && waves > 4 * cus) {  // single round, 1-2 waves per SIMD
        mode = env->place;                                  // 1 or 2
        B = (mode == 1) ? (int)((waves + W - 1) / W) : (int)cus;
    } else if (waves > (int64_t)W * cus) {                  // several rounds
        mode = 3;
        B = (int)((waves + W - 1) / W);
        // persistent waves (default): one workgroup per CU, its waves claim the packets of the cost-sorted list one by
        // one (FanArgs::wave_queue); PGR_OPT_PERSISTENT 0 keeps the static deal of whole workgroups
        if (env->persistent && persist_ok) B = (int)cus;
    } else {
        return 0;
    }
    std::lock_guard<std::mutex> lock(env->place_mutex);  // host threads may share an env
    const bool persistent = (mode == 3) && env->persistent && persist_ok;
    size_t n_slots = persistent ? (size_t)waves : (size_t)B * W;
    // cost[waves] | the queue's counter (its own 256 bytes) | map[n_slots]
    size_t need = ((((size_t)waves * 4 + 255) & ~(size_t)255) + 256 + n_slots * 4 + 255) & ~(size_t)255;
    int pick = -1;
    for (size_t k = 0; k < env->place_slots.size() && pick < 0; k++) {
        pgr_env::PlaceSlot& ps = env->place_slots[k];
        // (a slot that is claimed but whose event has not been recorded yet -- another host thread between its
        // schedule_waves and its launch -- still carries the completed record of its previous use: not reclaimable)
        if (ps.in_flight && ps.recorded && hipEventQuery(ps.ev) == hipSuccess) ps.in_flight = false;
        if (!ps.in_flight) pick = (int)k;
    }
    if (pick < 0) {
        if (env->place_slots.size() >= 4096) return fail("pgr_shoot_fan: more than 4096 fans in flight on one environment");
        env->place_slots.emplace_back();
        pick = (int)env->place_slots.size() - 1;
        HIPCHK(hipEventCreateWithFlags(&env->place_slots[pick].ev, hipEventDisableTiming));
    }
    pgr_env::PlaceSlot& ps = env->place_slots[pick];
    // (the slot is not in flight: nobody reads its buffer)
    if (need > ps.bytes && !grow_buffer(ps.buf, ps.bytes, need > 65536 ? need : 65536)) return fail("pgr_shoot_fan: device allocation of the wave placement failed");
    ps.in_flight = true;   // (the event is recorded by the caller behind the fan kernel: PlaceGuard)
    ps.recorded = false;
    slot_out = pick;
    char* slot = (char*)ps.buf;
    float* cost = (float*)slot;
    int* counter = (int*)(slot + (((size_t)waves * 4 + 255) & ~(size_t)255));
    int* map = counter + 64;
    HIPCHK(hipMemsetAsync(map, 0xFF, n_slots * sizeof(int), st));
    if (persistent) {
        HIPCHK(hipMemsetAsync(counter, 0, sizeof(int), st));
        out.queue = counter;
        out.n_queue = (int)waves;
        // Fans of up to two rounds (eight-wave workgroups): the first packets of waves 4 .. 7 come from the list's cheap
        // end, so that every steep packet starts beside a cheap one (140 000 rays: 6.6 instead of 7.9 ms, 200 000: 8.8 instead
        // of 9.6); beyond two rounds the steep packets are a small share of a long launch and the plain list is 1 - 3 %
        // faster (300 000 rays 11.9 against 12.2 ms, 1e6 34.3 against 34.5).  PGR_OPT_PERSISTENT 2 / 3: never / always.
        const bool tail_first = env->persistent == 3 || (env->persistent == 1 && waves <= 16 * (int64_t)B);
        if (tail_first && W == 8 && waves >= 8 * (int64_t)B) out.n_tail = 4 * B;
    }
    hipLaunchKernelGGL(pgr_wave_cost, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, y0, N, (int)waves, cost);
    hipLaunchKernelGGL(pgr_wave_place, dim3(1), dim3(1024), 0, st, cost, (int)waves, B, W, mode, map);
    out.map = map;
    out.blocks = B;
    return 0;
}

// Kernel variant of an environment: where the table lives (LDS copy of the single profile / HBM) and how a depth cell is
// found (zm 1 / 4: zin[j] = j dz exactly, 5: cubic index estimate, 3: quadratic estimate + three nodes, 2: bin table -- zin
// in LDS for those three --, 0: closed form for other uniform grids or binary search); zx_bytes = LDS the depth search takes.
struct FanVariant { bool lds_tab; int zm; size_t zx_bytes; };
static FanVariant select_variant(const pgr_env* env)
{
    const EnvDev& D = env->d;
    const size_t tab_bytes = (size_t)D.nz * sizeof(double2);
    const size_t zb_bytes = D.z_bucket ? ((size_t)D.nz * sizeof(double) + (((size_t)D.zb_B * 2 + 15) & ~(size_t)15)) : 0;
    const size_t zq_bytes = (size_t)D.nz * sizeof(double);
    FanVariant v{env->lds_path != 0, D.z_simple ? ((D.dz == 1.0) ? 4 : 1) : 0, 0};
    // a depth search that keeps zin in the LDS: beside the table when the two fit, else with the tables in HBM
    auto take = [&](int zm, size_t bytes) {
        if (env->range_indep && tab_bytes + bytes <= env->max_lds) v = {true, zm, bytes};
        else if (bytes <= env->max_lds) v = {false, zm, bytes};
    };
    if (!D.z_simple && env->depth_search != 1) {
        if (D.z_cubic && env->depth_search == 0) take(5, zq_bytes);
        if (v.zm == 0 && D.z_quad && (env->depth_search == 0 || env->depth_search == 3)) take(3, zq_bytes);
        if (v.zm == 0 && D.z_bucket) take(2, zb_bytes);
    }
    return v;
}

// The dynamic LDS of a fan kernel, in the order it is laid out: the table (LDS-table variants), the depth search's arrays,
// {depth_ranges, depths} when 16 nb bytes are left for them (bathy_off -1: read from HBM), and -- PGR_SAMPLE_BLOCKED -- 6 KB of
// per-lane sample staging per wave.  fits: the staging found room (everything before it is optional or was budgeted by select_variant).
struct LdsLayout { int bathy_off = -1, blk_off = 0; size_t total = 0; bool fits = true; };
static LdsLayout lds_layout(const pgr_env* env, const FanVariant& v, int wpb, bool blocked)
{
    LdsLayout L;
    L.total = (v.lds_tab ? (size_t)env->d.nz * sizeof(double2) : 0) + v.zx_bytes;
    auto append = [&](size_t need, int& off) {
        const size_t at = (L.total + 15) & ~(size_t)15;
        if (at + need > env->max_lds) return false;
        off = (int)at; L.total = at + need;
        return true;
    };
    append((size_t)env->d.nb * 16, L.bathy_off);
    if (blocked) L.fits = append((size_t)wpb * 6144, L.blk_off);
    return L;
}

// Which pgr_fan_kernel<LDS_TAB, ZM, SAVE, PERSIST, LOG> instances the library holds -- THE statement of it: the instance
// table below instantiates exactly these, and every refusal of a launch that would need another one asks here.
// SAVE 3 (sample-blocked) goes with the tables in HBM; persistent waves are not built for SAVE 2; the bounce log is built
// where the API's trajectory fans run: rows with the LDS table (SAVE 1), sample-blocked with the tables in HBM (SAVE 3).
// 6 x (3 + 4) x 2 - 6 x 2 = 72 without a log, 6 x 2 x 2 = 24 with one.
constexpr bool fan_instance_exists(bool lds_tab, int zm, int save, bool persist, bool log)
{
    if (zm < 0 || zm > 5 || save < 0 || save > 3) return false;
    if (persist && save == 2) return false;
    if (log) return save == (lds_tab ? 1 : 3);
    return save != 3 || !lds_tab;
}

// SAVE of the instance a launch needs: 0 end state only, 1 trajectories on a linspace grid (default sample form), 2 any grid /
// PGR_EXACT_SAMPLES, 3 = 1 in the sample-blocked layout (the flags that must go with PGR_SAMPLE_BLOCKED: shoot_fan_device)
static int fan_save(bool save, uint32_t flags) { return !save ? 0 : (flags & PGR_SAMPLE_BLOCKED) ? 3 : ((flags & PGR_SAVE_LINSPACE) && !(flags & PGR_EXACT_SAMPLES)) ? 1 : 2; }

// The instance table: entry fan_instance_index(...) is the kernel's address, null where fan_instance_exists says no.
constexpr int kFanInstanceSlots = 2 * 2 * 6 * 4 * 2;
constexpr int fan_instance_index(bool lds_tab, int zm, int save, bool persist, bool log) { return ((((int)log * 2 + (int)lds_tab) * 6 + zm) * 4 + save) * 2 + (int)persist; }

template <int I> static const void* fan_instance_entry()
{
    constexpr bool LG = I / 96 != 0, LT = I / 48 % 2 != 0, PV = I % 2 != 0;
    constexpr int ZMV = I / 8 % 6, SV = I / 2 % 4;
    static_assert(fan_instance_index(LT, ZMV, SV, PV, LG) == I, "fan_instance_entry decodes fan_instance_index");
    if constexpr (fan_instance_exists(LT, ZMV, SV, PV, LG)) return (const void*)pgr_fan_kernel<LT, ZMV, SV, PV, LG>;
    else return nullptr;
}

template <int... I> static const void* fan_instance(int i, std::integer_sequence<int, I...>)
{
    static const void* const table[] = {fan_instance_entry<I>()...};
    return table[i];
}

// Would a trajectory fan of this environment run the sample-blocked kernel (PGR_SAMPLE_BLOCKED) if asked to?  The host-pointer
// entry and the fan handles ask before they size their device buffers: tables in HBM / L2 (the LDS-table kernels gain
// nothing from it, and have no such instance), and room in the LDS for the staging of eight waves.
static bool blocked_layout_fits(const pgr_env* env)
{
    const FanVariant v = select_variant(env);
    return env->api_blocked && fan_instance_exists(v.lds_tab, v.zm, 3, false, false) && lds_layout(env, v, 8, true).fits;
}

// Does a fan of these flags, launched by the host-pointer entry or a fan handle, run sample-blocked (un-blocked on the way
// out)?  Trajectories on a linspace grid in the default sample form, sample-major, and an environment it fits.
static bool fan_blocked(const pgr_env* env, bool save, uint32_t flags)
{
    return save && (flags & PGR_SAVE_LINSPACE) && (flags & PGR_SAMPLE_MAJOR) && !(flags & PGR_EXACT_SAMPLES) && blocked_layout_fits(env);
}

// The bounce log of a launch: three [K][N] arrays the LOG instances of the fan kernel write; K == 0: none.
struct FanLog {
    double* x = nullptr;
    double* p = nullptr;
    signed char* k = nullptr;
    int32_t K = 0;
};

// The claimed placement slot becomes reclaimable when everything queued on `st` so far has run: its event is recorded
// behind the fan kernel, or -- on an early error return -- behind the map-building kernels already queued
struct PlaceGuard {
    pgr_env* env; hipStream_t st; int& slot;
    void release() {
        if (slot < 0) return;
        bool recorded;
        {
            std::lock_guard<std::mutex> lock(env->place_mutex);
            pgr_env::PlaceSlot& ps = env->place_slots[slot];   // (by index: the vector may have grown meanwhile)
            recorded = hipEventRecord(ps.ev, st) == hipSuccess;
            if (recorded) ps.recorded = true;
        }
        if (!recorded) {
            // no event to wait on: drain the stream WITHOUT the lock (other host threads keep launching on this
            // environment meanwhile; the slot stays claimed, so nobody takes it), then hand the slot back
            (void)hipStreamSynchronize(st);
            std::lock_guard<std::mutex> lock(env->place_mutex);
            env->place_slots[slot].in_flight = false;
        }
        slot = -1;
    }
    ~PlaceGuard() { release(); }
};

// shoot_fan_device, argument checks: what can be refused from the arguments alone (a fan of no rays never gets here)
static int check_fan_args(const double* y0, double source_range, double receiver_range, const double* r_save, int32_t S,
                          double rtol, double atol, int64_t max_steps, const double* T, const double* z, const double* p,
                          const int32_t* n_bott, const int32_t* n_surf, const int32_t* status)
{
    if (!y0 || !n_bott || !n_surf || !status) return fail("pgr_shoot_fan: null argument");
    const bool save = (T != nullptr);
    if (save && (!z || !p || !r_save)) return fail("pgr_shoot_fan: T, z, p and r_save go together");
    if (save && S < 1) return fail("pgr_shoot_fan: num_range_save must be >= 1");
    if (!(rtol > 0) || !(atol >= 0)) return fail("pgr_shoot_fan: bad tolerances");
    if (max_steps <= 0 || max_steps > (1LL << 30)) return fail("pgr_shoot_fan: max_steps out of range");
    // REF/launch_rays.py:404: an empty `while x < receiver_range` leaves `sols` empty and the
    // reference fails with IndexError; backwards shots are mirrored by the caller first
    if (!(source_range < receiver_range)) return fail("pgr_shoot_fan: need source_range < receiver_range (mirror backwards shots)");
    return 0;
}

// shoot_fan_device, instance selection but for PERSIST (known once the waves are scheduled): SAVE goes out through `sv`;
// everything that can be refused from the flags alone is refused HERE, before the scheduling claims a placement slot and
// queues its memset and two kernels on the caller's stream
static int select_fan_save(const FanVariant& v, bool save, uint32_t flags, const FanLog& log, int& sv)
{
    if (flags & PGR_SAMPLE_BLOCKED) {
        if (!save || !(flags & PGR_SAMPLE_MAJOR)) return fail("pgr_shoot_fan: PGR_SAMPLE_BLOCKED goes with trajectories and PGR_SAMPLE_MAJOR");
        if (!fan_instance_exists(v.lds_tab, v.zm, 3, false, false)) return fail("pgr_shoot_fan: PGR_SAMPLE_BLOCKED is for environments whose tables stay in HBM (this one is on the LDS-table path)");
        if (!(flags & PGR_SAVE_LINSPACE) || (flags & PGR_EXACT_SAMPLES)) return fail("pgr_shoot_fan: PGR_SAMPLE_BLOCKED needs a linspace save grid (PGR_SAVE_LINSPACE) and the default sample form");
    }
    sv = fan_save(save, flags);
    if (log.K) {
        if (!log.x || !log.p || !log.k) return fail("pgr_shoot_fan: the bounce log needs its three arrays");
        if (!fan_instance_exists(v.lds_tab, v.zm, sv, false, true))
            return fail("pgr_shoot_fan: a bounce log goes with trajectories on a linspace grid in the default sample form: rows with the "
                        "LDS table, sample-blocked with the tables in HBM (not PGR_EXACT_SAMPLES, end states only, or PGR_OPT_API_BLOCKED off)");
    }
    return 0;
}

// shoot_fan_device, launch shape: workgroup size and grid, and the cost-aware scheduling of the waves (placement,
// priorities, homogeneous workgroups) where the fan is large enough for it
static int fan_launch_shape(pgr_env* env, bool lds_tab, const double* y0, int64_t N, hipStream_t st, bool persist_ok,
                            int& place_slot, FanShape& s)
{
    const int64_t waves = (N + 63) / 64, cus = env->num_cus;
    int W;   // waves per workgroup of the scheduled launch
    if (lds_tab) {
        // one workgroup per CU (the LDS table is per workgroup): the smallest workgroup that
        // covers the fan in a single round, capped at 8 waves
        const int64_t w = (waves + cus - 1) / cus;
        s.wpb = env->waves_per_block ? env->waves_per_block : w < 1 ? 1 : w > 8 ? 8 : (int)w;
        W = s.wpb;
    } else {
        // a fan too small for the scheduling keeps 4-wave workgroups
        const int cap = 8;
        s.wpb = env->waves_per_block ? env->waves_per_block : 4;
        if (s.wpb > cap) s.wpb = cap;
        W = (waves <= 4 * cus) ? 0 : waves <= cap * cus ? (int)((waves + cus - 1) / cus) : cap;
    }
    s.blocks = (waves + s.wpb - 1) / s.wpb;
    if (W == 0) return 0;
    if (schedule_waves(env, y0, N, waves, W, st, persist_ok, place_slot, s)) return -1;
    if (s.map) s.wpb = W;
    return 0;
}

static int shoot_fan_device(pgr_env* env, const double* y0, int64_t N, double source_range, double receiver_range,
                            const double* r_save, int32_t S, double rtol, double atol, uint32_t flags, int64_t max_steps,
                            double* T, double* z, double* p, double* end_state, int32_t* n_bott, int32_t* n_surf,
                            int32_t* status, int32_t* n_steps, int32_t* n_rej, void* stream, const FanLog& log)
{
    if (!env) return fail("pgr_shoot_fan: null env");
    if (N < 0) return fail("pgr_shoot_fan: negative ray count");
    if (N == 0) return 0;
    if (check_fan_args(y0, source_range, receiver_range, r_save, S, rtol, atol, max_steps, T, z, p, n_bott, n_surf, status)) return -1;
    const bool save = (T != nullptr);
    HIPCHK(hipSetDevice(env->device));

    FanArgsLog a{};   // (the instances without a log take its FanArgs part)
    a.log_x = log.x; a.log_p = log.p; a.log_k = log.k; a.log_K = log.K;
    a.y0 = y0; a.r_save = r_save; a.T = T; a.Z = z; a.P = p; a.end_state = end_state;
    a.n_bott = n_bott; a.n_surf = n_surf; a.status = status; a.n_steps = n_steps; a.n_rej = n_rej;
    a.N = N; a.S = save ? S : 1;
    if (flags & PGR_SAMPLE_MAJOR) { a.stride_ray = 1; a.stride_smp = N; }
    else { a.stride_ray = S; a.stride_smp = 1; }
    // solve_ivp's validate_tol (SCIPY/common.py:44-51): an rtol below 100 EPS is raised to it (SciPy warns)
    if (rtol < 100 * DBL_EPSILON) rtol = 100 * DBL_EPSILON;
    a.x0 = source_range; a.x1 = receiver_range; a.rtol = rtol; a.atol = atol;
    a.inv_dsave = (S > 1 && receiver_range != source_range) ? (double)(S - 1) / (receiver_range - source_range) : 0.0;
    // np.linspace: step = (stop - start) / (num - 1); y = arange(num) * step + start; y[-1] = stop
    a.save_step = (S > 1) ? (receiver_range - source_range) / (double)(S - 1) : 0.0;
    a.save_formula = (flags & PGR_SAVE_LINSPACE) ? 1 : 0;
    a.park_lanes = env->park_lanes; a.park_trips = env->park_trips;
    a.max_steps = max_steps; a.flags = flags;
    // instance selection: everything refusable is refused before a placement slot is claimed
    hipStream_t st = (hipStream_t)stream;
    const FanVariant v = select_variant(env);
    const bool logged = log.K != 0;
    int sv;
    if (select_fan_save(v, save, flags, log, sv)) return -1;
    const bool persist_ok = fan_instance_exists(v.lds_tab, v.zm, sv, true, logged);
    // launch shape: workgroups, wave schedule, LDS
    int place_slot = -1;
    PlaceGuard guard{env, st, place_slot};
    FanShape s;
    if (fan_launch_shape(env, v.lds_tab, y0, N, st, persist_ok, place_slot, s)) return -1;
    a.wave_map = s.map; a.wave_queue = s.queue; a.n_queue = s.n_queue; a.n_queue_tail = s.n_tail;
    const int threads = s.wpb * 64;
    const LdsLayout L = lds_layout(env, v, s.wpb, (flags & PGR_SAMPLE_BLOCKED) != 0);
    if (!L.fits) return fail("pgr_shoot_fan: no LDS left for PGR_SAMPLE_BLOCKED");
    a.bathy_lds_off = L.bathy_off; a.blk_lds_off = L.blk_off;
    // n_queue_tail = 4 x grid is only right for eight-wave workgroups on a grid of exactly `blocks` workgroups (the kernel reads
    // tail entry n - 1 - (4 blockIdx + wave - 4) and never queues the tail): a change of either would skip or double-integrate packets
    if (a.n_queue_tail && !(threads == 512 && s.blocks * 4 == (int64_t)a.n_queue_tail))
        return fail("pgr_shoot_fan: internal error: the packet queue's pre-assigned tail does not match the launch shape");
    const bool persist = a.wave_queue != nullptr;
    const void* kernel = fan_instance(fan_instance_index(v.lds_tab, v.zm, sv, persist, logged), std::make_integer_sequence<int, kFanInstanceSlots>{});
    if (!kernel) return fail("pgr_shoot_fan: internal error: no kernel instance for the selected variant");
    // launch: the record of the selected instance, then the kernel (FanArgsLog for the LOG instances, its FanArgs base for the others)
    const int li[8] = {(int)v.lds_tab, v.zm, sv, (int)persist, (int)s.blocks, threads, (int)L.total, a.n_queue_tail};
    for (int q = 0; q < 8; q++) env->last_instance[q].store(li[q], std::memory_order_relaxed);
    env->last_instance_log.store((int)logged, std::memory_order_relaxed);
    if (L.total > 64 * 1024) HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total));
    void* kernel_args[2] = {(void*)&env->d_dev, logged ? (void*)&a : (void*)static_cast<FanArgs*>(&a)};
    (void)hipLaunchKernel(kernel, dim3((unsigned)s.blocks), dim3(threads), kernel_args, L.total, st);
    const hipError_t launch_err = hipGetLastError();
    // (the placement map is this launch's until its fan kernel has run: `guard` records the slot's event on `st` here
    // and on every error return between the slot's pick and this point)
    guard.release();
    if (launch_err != hipSuccess) return fail(std::string("fan kernel launch: ") + hipGetErrorString(launch_err));
    return 0;
}

extern "C" int pgr_shoot_fan_device(pgr_env* env, const double* y0, int64_t N, double source_range,
                                    double receiver_range, const double* r_save, int32_t S,
                                    double rtol, double atol, uint32_t flags, int64_t max_steps,
                                    double* T, double* z, double* p, double* end_state,
                                    int32_t* n_bott, int32_t* n_surf, int32_t* status,
                                    int32_t* n_steps, int32_t* n_rej, void* stream)
{
    return shoot_fan_device(env, y0, N, source_range, receiver_range, r_save, S, rtol, atol, flags, max_steps, T, z, p, end_state,
                            n_bott, n_surf, status, n_steps, n_rej, stream, FanLog{});
}

// LOG of the instance the last launch on this environment selected (1: it writes a bounce log), -1 before any launch: the
// eight slots of pgr_debug_last_instance are all taken
extern "C" int pgr_debug_last_instance_log(const pgr_env* env)
{
    if (!env) return fail("pgr_debug_last_instance_log: null argument");
    return env->last_instance_log.load(std::memory_order_relaxed);
}

extern "C" int pgr_debug_last_instance(const pgr_env* env, int32_t out[8])
{
    if (!env || !out) return fail("pgr_debug_last_instance: null argument");
    for (int q = 0; q < 8; q++) out[q] = env->last_instance[q].load(std::memory_order_relaxed);
    return 0;
}

#endif  // PGR_LAUNCH_H
