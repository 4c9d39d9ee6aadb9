// pgr_coh_sum_body.h -- the body of the coherent tube sum's kernel, stated once and included, inside the kernel's braces, by
// pgr_coh_sum (pgr_phase.h, COH_PHI 0) and by pgr_coh_sum_phi (pgr_reflect.h, COH_PHI 1: `phi` [S][M], the rays' lag in cycles;
// DESIGN.md section 19).  Textual on purpose: with COH_PHI 0 the compiler sees pgr_coh_sum's statements as they ever were, so
// its instructions do not change.  In scope: EnvDev env, TlArgs a, CohOut o (and const double* phi).  No include guard.
    __shared__ TlTubes L;
    __shared__ TlRays Y;
    const TlBand b = tl_band<false>(a);
    double re = 0.0, im = 0.0;
    if (b.r == 0.0) {                              // the source's own column (uniform in the wave)
        re = NAN;
        im = NAN;
    } else {
        const Ctx<false, 0> C(env, nullptr);
        const int32_t* q = o.q ? o.q + (int64_t)b.s * a.M : nullptr;
#if COH_PHI
        const double* lag = phi + (int64_t)b.s * a.M;
#endif
        tl_walk<true>(a, C, b, L, &Y, [&](int64_t c, int u) {
            const int qk = q ? q[c * TL_TUBES + u] : 0;
            if (qk < 0) return;
            const double d0 = Y.d[u], d1 = Y.d[u + 1];
            const double w = fdiv(b.d - d0, d1 - d0);
            const double T = Y.T[u] + w * (Y.T[u + 1] - Y.T[u]);
            const double amp = fsqrt(L.I[u]);
            double y = o.f * T;
            y = y - rint(y);
            double t = y - 0.25 * (double)(qk & 3);
            t = t - rint(t);
#if COH_PHI
            {
                // (a visited tube has both its rays: k + 1 < M.  The wave visits tube u together: two broadcast loads)
                const double f0 = lag[c * TL_TUBES + u], f1 = lag[c * TL_TUBES + u + 1];
                double pa = f1 - f0;
                pa = w * pa;
                pa = f0 + pa;
                const double r = pa - rint(pa);
                t = t - r;
                t = t - rint(t);
            }
#endif
            double cv, sv;
            gcossin2pi(t, cv, sv);                 // (gcos2pi(t) and gsin2pi(t), their common part formed once)
            re = re + amp * cv;
            im = im + amp * sv;
        });
    }
    if (b.rcv) {
        o.re[b.j * a.S + b.s] = re;
        o.im[b.j * a.S + b.s] = im;
    }
