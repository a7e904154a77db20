// ba_debug_host.inc — host side of the instrumented builds (`make timing`: -DK7_TIMING; tools/dev/build_variant.sh: -DSCHUR_STAMPS,
// -DPREP_STAMPS): what ptam_ba_compute and ptam_ba_bench_jacobian print from the cycle stamps the kernels leave in BaDev::dbg, and
// ba_prepare_impl from those in PrepScalars.  tools/dev/schur_fit.py, schur_fit2.py and schur_wg_timeline.py parse this text.  In the
// product build every ba_dbg_* function up to ba_dbg_prep_stamps is empty; behind them, what prepare prints under PTAM_DEBUG_PREPARE
// and PTAM_DEBUG_SCHUR (tests/test_gpu_parity.py parses the latter).
// Included by bundle.hip behind ptam_ba.
struct BaHostTimes {
    double t0 = 0, first = 0, loop = 0;   // us: Compute() began, read its first trial's verdict, left its loop
};
#ifdef K7_TIMING
static double ba_dbg_now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#endif

static inline void ba_dbg_begin(ptam_ba* ba, BaHostTimes& ht) {
#ifdef K7_TIMING
    ht.t0 = ba_dbg_now_us();
    (void)hipMemsetAsync(ba->d.dbg + TL_BASE, 0, 8, ba->ctx->stream);
#endif
}
static inline void ba_dbg_first_read(BaHostTimes& ht) {
#ifdef K7_TIMING
    if (ht.first == 0) ht.first = ba_dbg_now_us();
#endif
}
// the loop is over (the read-back has not begun)
static inline int ba_dbg_loop_end(ptam_ba* ba, BaHostTimes& ht) {
#ifdef K7_TIMING
    ht.loop = ba_dbg_now_us();
    const BaDev& d = ba->d;
    long long h[16];
    HIP_TRY(hipMemcpy(h, d.dbg, sizeof h, hipMemcpyDeviceToHost));
    std::printf("LDLT step2 wg0: loop %lld tail %lld | last wg (role %lld): loop %lld tail %lld\n", h[1] - h[0], h[2] - h[1], h[7],
                h[5] - h[4], h[6] - h[5]);
    long long q[8];
    HIP_TRY(hipMemcpy(q, d.dbg + 32, sizeof q, hipMemcpyDeviceToHost));
    std::printf("LDLT step2 wg0 iteration 3 (cycles): micro factor %lld | my rows %lld | next panel columns %lld | publish %lld | barrier %lld | "
                "operand reads issued %lld | off-chain updates %lld\n", q[1] - q[0], q[2] - q[1], q[3] - q[2], q[4] - q[3], q[5] - q[4], q[6] - q[5], q[7] - q[6]);
#endif
    return PTAM_OK;
}
// the call is over
static inline int ba_dbg_dump(ptam_ba* ba, const BaHostTimes& ht) {
#if defined(K7_TIMING) || defined(SCHUR_STAMPS)
    const BaDev& d = ba->d;
#endif
#ifdef K7_TIMING
    std::printf("HOST Compute: first trial read at %.1f us, loop end %.1f us, total %.1f us (%zu trials)\n", ht.first - ht.t0, ht.loop - ht.t0,
                ba_dbg_now_us() - ht.t0, ba->trials.size());
    {
        long long c[4];
        HIP_TRY(hipMemcpy(c, d.dbg + 5000, sizeof c, hipMemcpyDeviceToHost));
        if (c[3] > c[1])
            std::printf("K7 INSIDE Compute() (its last launch, block 100): %lld shader cycles in %.2f us = %.2f GHz\n", c[2] - c[0], (c[3] - c[1]) * 0.01,
                        (double)(c[2] - c[0]) / ((c[3] - c[1]) * 10.0));
    }
    if (getenv("PTAM_TIMELINE")) {
        std::vector<long long> tl(2 + 2 * TL_MAX);
        HIP_TRY(hipMemcpy(tl.data(), d.dbg + TL_BASE, tl.size() * 8, hipMemcpyDeviceToHost));
        const long long n_tl = std::min<long long>(tl[0], TL_MAX);
        static const char* nm[] = {"?", "purge_pass1", "select_compact", "select_final", "K7", "reduce_vinv", "vinv", "schur_tile", "schur_reduce",
                                   "ldlt_step0", "backward", "point_update", "finalize", "project_e2", "pass1_trial", "purge", "reduce_partials", "publish"};
        for (long long i = 0; i < n_tl; i++)
            std::printf("TL %4lld %-16s start %9.2f us  (+%.2f)\n", i, nm[tl[2 + 2 * i] < 18 ? tl[2 + 2 * i] : 0], (tl[3 + 2 * i] - tl[3]) * 0.01,
                        i ? (tl[3 + 2 * i] - tl[1 + 2 * i]) * 0.01 : 0.0);
    }
#endif
#ifdef SCHUR_STAMPS
    {
        std::vector<long long> wt(1024);
        HIP_TRY(hipMemcpy(wt.data(), d.dbg + 3072, wt.size() * 8, hipMemcpyDeviceToHost));
        const int nw = std::min(512, d.n_schur_wg);
        const long long M40 = (1ll << 40) - 1, M56 = (1ll << 56) - 1;
        long long e0 = wt[0] & M40, x1 = 0;
        for (int i = 0; i < nw; i++) e0 = std::min(e0, wt[2 * i] & M40), x1 = std::max(x1, wt[2 * i + 1] & M56 & M40);
        std::printf("SCHUR workgroups %d: makespan %.2f us; per workgroup (entry, exit in us from the first entry, segments, hw id):\n", nw, (x1 - e0) * 0.01);
        for (int i = 0; i < nw; i++)
            std::printf("%s[%d %.1f %.1f %d %llx]", i % 8 ? " " : "\n  ", i, ((wt[2 * i] & M40) - e0) * 0.01, ((wt[2 * i + 1] & M40) - e0) * 0.01, (int)(wt[2 * i + 1] >> 56),
                        (unsigned long long)(wt[2 * i] >> 40));
        std::printf("\n");
        // the schedule: per workgroup its segments as pair:groups
        std::vector<int> wseg((size_t)d.n_schur_wg + 1);
        HIP_TRY(hipMemcpy(wseg.data(), d.s_wg_seg, wseg.size() * 4, hipMemcpyDeviceToHost));
        std::vector<SchurWG> segs((size_t)wseg.back());
        HIP_TRY(hipMemcpy(segs.data(), d.s_segs, segs.size() * sizeof(SchurWG), hipMemcpyDeviceToHost));
        std::vector<SchurEntry> ents((size_t)std::max(1, d.n_schur_entries));
        HIP_TRY(hipMemcpy(ents.data(), d.s_entries, (size_t)d.n_schur_entries * sizeof(SchurEntry), hipMemcpyDeviceToHost));
        std::printf("SCHUR schedule:");   // per segment  pair : groups : model cost of its entries (the split's units)
        for (int i = 0; i < nw; i++) {
            std::printf("%s{%d", i % 8 ? " " : "\n  ", i);
            for (int sg = wseg[i]; sg < wseg[i + 1]; sg++) {
                long long cost = 0;
                for (int e = segs[sg].e_begin; e < segs[sg].e_end; e++) cost += ents[(size_t)e].pad & 0xffff;
                std::printf(" %d:%d:%lld", segs[sg].pair, (segs[sg].e_end - segs[sg].e_begin + 3) / 4, cost);
            }
            std::printf("}");
        }
        std::printf("\n");
    }
    {
        std::vector<long long> st(1024);
        HIP_TRY(hipMemcpy(st.data(), d.dbg + 2048, st.size() * 8, hipMemcpyDeviceToHost));
        for (int sel = 0; sel < 2; sel++) {
            const long long* b = st.data() + sel * 512;
            long long t0 = b[0];
            for (int w = 0; w < 4; w++) if (b[w * 64] && b[w * 64] < t0) t0 = b[w * 64];
            std::printf("SCHUR stamps wg %d (groups %lld): per wave, per group: top, loads issued, data there, MFMAs issued (cycles from the first top)\n", sel ? 150 : 0, b[260]);
            for (int w = 0; w < 4; w++) {
                std::printf("  w%d:", w);
                for (int i = 0; i < 16 && b[(w * 16 + i) * 4]; i++)
                    std::printf(" [%lld %lld %lld %lld]", b[(w * 16 + i) * 4] - t0, b[(w * 16 + i) * 4 + 1] - t0, b[(w * 16 + i) * 4 + 2] - t0, b[(w * 16 + i) * 4 + 3] - t0);
                std::printf(" end %lld\n", b[256 + w] - t0);
            }
            std::printf("  kernel entry %lld, exit %lld, segments %lld; last segment's epilogue (wave 0): loop end %lld, barrier 1 %lld, 2 %lld, 3 %lld, laid out %lld, stores issued %lld\n",
                        b[264] - t0, b[265] - t0, b[266], b[268] - t0, b[269] - t0, b[270] - t0, b[271] - t0, b[272] - t0, b[273] - t0);
        }
    }
#endif
    return PTAM_OK;
}
// ptam_ba_bench_jacobian: the stamps of the last of `reps` back-to-back launches of K7
static inline int ba_dbg_k7_stamps(ptam_ba* ba, int reps) {
#ifdef K7_TIMING
    const BaDev& d = ba->d;
    long long h[16];
    HIP_TRY(hipMemcpy(h, d.dbg, sizeof h, hipMemcpyDeviceToHost));
    {
        long long c[4];
        HIP_TRY(hipMemcpy(c, d.dbg + 5000, sizeof c, hipMemcpyDeviceToHost));
        if (c[3] > c[1])
            std::printf("K7 BACK TO BACK (last of %d launches, block 100): %lld shader cycles in %.2f us = %.2f GHz\n", reps, c[2] - c[0], (c[3] - c[1]) * 0.01,
                        (double)(c[2] - c[0]) / ((c[3] - c[1]) * 10.0));
    }
    std::printf("K7 stamps (10 ns ticks since kernel-body start):");
    for (int i = 1; i < 10; i++) std::printf(" [%d] %lld", i, h[i] - h[0]);
    std::printf("\n");
    const int nb = std::min(ba->d.grid_acc, 2000);
    std::vector<long long> w(2 * nb);
    HIP_TRY(hipMemcpy(w.data(), d.dbg + 16, w.size() * 8, hipMemcpyDeviceToHost));
    long long t0 = w[0];
    for (int b = 0; b < nb; b++) t0 = std::min(t0, w[2 * b]);
    std::vector<long long> st(nb), en(nb), du(nb);
    for (int b = 0; b < nb; b++) st[b] = w[2 * b] - t0, en[b] = w[2 * b + 1] - t0, du[b] = en[b] - st[b];
    std::sort(st.begin(), st.end());
    std::sort(en.begin(), en.end());
    std::sort(du.begin(), du.end());
    std::printf("K7 block 7: body starts %lld ticks after the block's first instruction\n", h[0] - w[14]);
    std::printf("K7 wall (10 ns ticks, %d blocks): start p0/p50/p90/p100 %lld %lld %lld %lld | end %lld %lld %lld %lld | dur %lld %lld %lld %lld\n",
                nb, st[0], st[nb / 2], st[nb * 9 / 10], st[nb - 1], en[0], en[nb / 2], en[nb * 9 / 10], en[nb - 1], du[0], du[nb / 2],
                du[nb * 9 / 10], du[nb - 1]);
#endif
    return PTAM_OK;
}
// -DPREP_STAMPS: the phases of prep_split_kernel per XCD list
static inline void ba_dbg_prep_stamps(const PrepScalars& ps) {
#ifdef PREP_STAMPS
    for (int x = 0; x < 8; x++) {
        std::fprintf(stderr, "[ptam] split kernel, list %d (us from its start): lists built %.1f | in LDS %.1f | round 1 done %.1f | search done %.1f | cut written %.1f\n", x,
                     (ps.stamp[x][1] - ps.stamp[x][0]) * 0.01, (ps.stamp[x][2] - ps.stamp[x][0]) * 0.01, (ps.stamp[x][3] - ps.stamp[x][0]) * 0.01,
                     (ps.stamp[x][4] - ps.stamp[x][0]) * 0.01, (ps.stamp[x][5] - ps.stamp[x][0]) * 0.01);
        std::fprintf(stderr, "[ptam]    the search: %lld shader cycles in %.1f us = %.2f GHz\n", ps.stamp[x][7] - ps.stamp[x][6], (ps.stamp[x][4] - ps.stamp[x][2]) * 0.01,
                     (double)(ps.stamp[x][7] - ps.stamp[x][6]) / ((ps.stamp[x][4] - ps.stamp[x][2]) * 10.0));
    }
#endif
}
// PTAM_DEBUG_SCHUR=1
static void ba_dbg_schur_lists(const PrepScalars& ps) {
    if (!getenv("PTAM_DEBUG_SCHUR")) return;
    std::fprintf(stderr, "[ptam] schur: %d segments, %d workgroups; %lld entries in %d (XCD, pair) lists, budgets", ps.n_segs, ps.n_schur_wg,
                 ps.n_entries, ps.n_xp);
    for (int x = 0; x < 8; x++) std::fprintf(stderr, " %lld", ps.t_cut[x]);
    std::fprintf(stderr, "; workgroups per XCD");
    for (int x = 0; x < 8; x++) std::fprintf(stderr, " %d", ps.n_wgs[x]);
    std::fprintf(stderr, "\n");
}
// PTAM_DEBUG_PREPARE=1: host time of the phases of ba_prepare_impl, and the sizes it asked for
static bool ba_dbg_prepare_on() {
    static const bool on = getenv("PTAM_DEBUG_PREPARE") != nullptr;
    return on;
}
struct PrepLaps {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!ba_dbg_prepare_on()) return;
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[ptam] prepare: %-18s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    }
};
static void ba_dbg_prepare_sizes(const ptam_ba* ba, size_t clear_bytes, size_t staging_bytes) {
    if (!ba_dbg_prepare_on()) return;
    std::fprintf(stderr, "[ptam] prepare: block_bytes %zu clear_bytes %zu sblock_bytes %zu staging_bytes %zu\n", ba->block_bytes, clear_bytes,
                 ba->sblock ? ba->sblock_bytes : (size_t)0, staging_bytes);
}
