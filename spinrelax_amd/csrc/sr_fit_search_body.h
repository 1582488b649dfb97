// sr_fit_search_body.h -- the body of k_order_search and k_order_search_sums (sr_fit.hip), included once in each with
// SR_SEARCH_FROM_SUMS 0 / 1.  A textual include and not a shared function template: k_order_search<..> must stay the instruction
// stream it was (scripts/dev/isa_diff.py), and the same body reached through an inlined function came out with other registers.
// In scope: the template parameters NMAX, W, LDS, the kernel argument `a` (SearchArgs) and, with SR_SEARCH_FROM_SUMS, `src`
// (SumsSource): the residue is then staged from kernel 1's raw sums (Residue::stage_sums) and C(t) / dC(t) are written as well.
    const int res = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x;
    if (a.tail_signal && blockIdx.x == gridDim.x - 1 && tid == 0)
        __hip_atomic_store(a.tail_signal, a.tail_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    // The fits are the latency chain of a group: their waves issue before the waves of the bandwidth kernels that fill the
    // launch's tail (the group's histograms: 24.0 -> 23.1 ms for the merged launch of 20 batches with them beside it).
    __builtin_amdgcn_s_setprio(SR_FIT_SETPRIO);
    Residue<W, LDS> T;
    T.L = a.L;
    T.tid = tid;
#if SR_SEARCH_FROM_SUMS
    T.stage_sums(a.t + (int64_t)res * a.t_stride, src.sums + (int64_t)res * src.R * src.Lp, src.R, src.F, src.Lp,
                 const_cast<double *>(a.y) + (int64_t)res * a.L, const_cast<double *>(a.sigma) + (int64_t)res * a.L,
                 LDS ? nullptr : a.fws + (int64_t)res * a.L, a.geo);
#else
    const double *sg_res = a.sigma ? a.sigma + (int64_t)res * a.L : nullptr;
    T.stage(a.t + (int64_t)res * a.t_stride, a.y + (int64_t)res * a.L, sg_res, LDS ? nullptr : a.fws + (int64_t)res * a.L, a.geo);
#endif

    const int ns = a.L < 10 ? a.L : 10;                 // nSample = 10, fitting_Ct_functions.py:359
    const double avgBeg = np_mean_y(T, 0, ns);
    const double avgEnd = np_mean_y(T, a.L - ns, ns);

    if (tid == 0) {
        for (int j = 0; j < a.nOrders; ++j) {
            const int64_t o = (int64_t)j * a.nRes + res;
            for (int i = 0; i < a.Pmax; ++i) { a.popt[o * a.Pmax + i] = NAN; a.dP[o * a.Pmax + i] = NAN; }
            a.chisq[o] = INFINITY;
            a.status[o] = -100;
            a.nfev[o] = 0;
        }
    }
    // The search state lives in LDS, not on the stack: it crosses the (non-inlined) per-order solver calls by reference, and a
    // stack object costs every lane a scratch frame.  It is workgroup-uniform: every thread stores the same values and reads
    // them back behind its own stores (LDS operations of a wave complete in order), so no barrier is needed.
    static_assert(sizeof(SearchState) <= kStateDoubles * sizeof(double), "SearchState does not fit its LDS slot");
    SearchState &st = *reinterpret_cast<SearchState *>(fit_smem + Residue<W, LDS>::ST);
    st.first = true; st.done = false; st.best = -1; st.best_chi = INFINITY;
#pragma unroll
    for (int i = 0; i < kNmax; ++i) st.xbest[i] = 0.0;

    for (int j = 0; j < a.nOrders && !st.done; ++j) {
        switch (a.orders[j]) {
            case 2: search_order<2>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 3: search_order<3>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 4: search_order<4>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 5: search_order<5>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 6: if (NMAX >= 6) search_order<(NMAX >= 6 ? 6 : 2)>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 7: if (NMAX >= 7) search_order<(NMAX >= 7 ? 7 : 2)>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 8: if (NMAX >= 8) search_order<(NMAX >= 8 ? 8 : 2)>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 9: if (NMAX >= 9) search_order<(NMAX >= 9 ? 9 : 2)>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 10: if (NMAX >= 10) search_order<(NMAX >= 10 ? 10 : 2)>(T, a, j, res, avgBeg, avgEnd, st); break;
            case 11: if (NMAX >= 11) search_order<(NMAX >= 11 ? 11 : 2)>(T, a, j, res, avgBeg, avgEnd, st); break;
            default: break;
        }
    }

    // selected model with its components sorted by tau (sort_components, fitting_Ct_functions.py:203-209)
    if (tid == 0) {
        a.best[res] = st.best;
        double Cs[kNmax / 2], ts[kNmax / 2];
        int K = 0;
        double S2 = 0.0, chi = NAN;
        if (st.best >= 0) {
#pragma clang fp contract(off)
            const int nP = a.orders[st.best];
            K = nP / 2;
            double sum = 0.0;
            for (int k = 0; k < kNmax / 2; ++k) {
                // st.xbest is indexed with compile-time constants only (registers): unrolled selects
                double c = 0.0, tt = 0.0;
#pragma unroll
                for (int i = 0; i < kNmax; ++i) {
                    if (i == k) c = st.xbest[i];
                    if (i == K + k) tt = st.xbest[i];
                }
                if (k < K) { Cs[k] = c; ts[k] = tt; sum += c; }
            }
            double last = 0.0;
#pragma unroll
            for (int i = 0; i < kNmax; ++i)
                if (i == nP - 1) last = st.xbest[i];
            S2 = (nP & 1) ? last : 1.0 - sum;
            chi = st.best_chi;
            for (int i = 1; i < K; ++i) {               // stable insertion sort by tau
                const double tc = ts[i], cc = Cs[i];
                int q = i - 1;
                while (q >= 0 && ts[q] > tc) { ts[q + 1] = ts[q]; Cs[q + 1] = Cs[q]; --q; }
                ts[q + 1] = tc; Cs[q + 1] = cc;
            }
        }
        a.sel_S2[res] = S2;
        a.sel_chi[res] = chi;
        a.sel_K[res] = K;
        for (int k = 0; k < a.Kmax; ++k) {
            a.sel_C[(int64_t)res * a.Kmax + k] = k < K ? Cs[k] : 0.0;
            a.sel_tau[(int64_t)res * a.Kmax + k] = k < K ? ts[k] : 1.0;
        }
    }
