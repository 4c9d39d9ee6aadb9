// pgr_sig_sum_body.h -- the body of the signal sum's kernel, stated once and included, inside the kernel's braces, by pgr_sig_sum
// (pgr_signal.h, SIG_PHI 0) and by pgr_sig_sum_phi (pgr_reflect.h, SIG_PHI 1: `phi`, every arrival's lag in cycles, applied
// where lane l stages arrival a0 + l).  Textual on purpose: with SIG_PHI 0 the compiler sees pgr_sig_sum's
// statements as they ever were, so its instructions do not change.  In scope: SigArgs s (and const double* phi).  No include guard.
    const int64_t g = blockIdx.x;
    const int32_t n0 = (int32_t)blockIdx.y * SIG_TILE;          // (n0 < nt: the grid has ceil(nt / SIG_TILE) tiles)
    const int lane = threadIdx.x;
    const int64_t a_end = s.off[g + 1];
    const double t0 = s.tstart[g];
    const int32_t last = min(n0 + SIG_TILE - 1, s.nt - 1);
    const double tA = sig_time(t0, n0, s.dt), tB = sig_time(t0, last, s.dt);
    double t[SIG_ROWS], re[SIG_ROWS], im[SIG_ROWS];
#pragma unroll
    for (int i = 0; i < SIG_ROWS; i++) {
        t[i] = sig_time(t0, min(n0 + i * 64 + lane, s.nt - 1), s.dt);
        re[i] = 0.0;
        im[i] = 0.0;
    }
    for (int64_t a0 = s.off[g]; a0 < a_end; a0 += 64) {
        const int64_t a = a0 + lane;
        double Ta = NAN, C = 0.0, Sn = 0.0;
        bool live = false;
        if (a < a_end) {
            const int qa = s.q ? s.q[a] : 0;
            Ta = s.T[a];
            const double xA = (tA - Ta) * s.rs, xB = (tB - Ta) * s.rs;
            const double vA = xA * xA, vB = xB * xB;
            // the arrival before the tile, inside it, behind it; a NaN T fails all three
            live = qa >= 0 && ((xA > 0.0 && vA <= 64.0) || (xA <= 0.0 && xB >= 0.0) || (xB < 0.0 && vB <= 64.0));
            if (live) {
                const double amp = fsqrt(s.I[a]);
                double y = s.f * Ta;
                y = y - rint(y);
                double ph = y - 0.25 * (double)(qa & 3);
                ph = ph - rint(ph);
#if SIG_PHI
                {
                    const double pa = phi[a];
                    const double r = pa - rint(pa);
                    ph = ph - r;
                    ph = ph - rint(ph);
                }
#endif
                double cv, sv;
                gcossin2pi(ph, cv, sv);
                C = amp * cv;
                Sn = amp * sv;
            }
        }
        uint64_t todo = __ballot(live);
        while (todo) {                                          // uniform in the wave: increasing a
            const int u = __builtin_ctzll(todo);
            todo &= todo - 1;
            const double Tu = sig_lane(Ta, u), Cu = sig_lane(C, u), Su = sig_lane(Sn, u);
#pragma unroll
            for (int i = 0; i < SIG_ROWS; i++) {
                const double x = (t[i] - Tu) * s.rs;
                const double v = x * x;
                if (v <= 64.0) {
                    const double E = gexp(-0.5 * v);
                    re[i] = re[i] + Cu * E;
                    im[i] = im[i] + Su * E;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < SIG_ROWS; i++) {
        const int32_t n = n0 + i * 64 + lane;
        if (n < s.nt) {
            s.re[g * s.nt + n] = re[i];
            s.im[g * s.nt + n] = im[i];
        }
    }
