/* k_step.inc — the fused step kernel template; included by k_step_explicit.hip and k_step_auto.hip */
/* Two kernels from one text.  k_step is the kernel as it always was; k_step_waverow (same arguments) is the wave-per-row form, launched
 * where rows_index takes its strip branch (the host decides: picles_hip.hip, launch_step_rows).  The file includes itself once per
 * kernel, with the kernel's name and the WROW switch as macros, rather than instantiating a shared __forceinline__ body: handing the
 * kernel's arguments on to a body function changes the instruction stream of k_step (one instruction more with references, one fewer
 * by value, different scheduling around the pull), and k_step has to stay what the committed profiles and budgets describe. */
#ifndef K_STEP_NAME
#define K_STEP_NAME k_step
#define K_STEP_WROW false
#include "k_step.inc"
#undef K_STEP_NAME
#undef K_STEP_WROW
#define K_STEP_NAME k_step_waverow
#define K_STEP_WROW true
#include "k_step.inc"
#undef K_STEP_NAME
#undef K_STEP_WROW
#else
/* ------------------------------------------------------------------------------------------
 * k_step — one whole model step per launch, for consecutive run!-style steps (State zeroed
 * before each step, time-constant winds): the thread of node/particle k
 *   1. pull-scatters the PREVIOUS step's records -> State[k]          (k_scatter)
 *   2. remeshes particle k from that node value, in registers          (NodeToParticle!)
 *   3. advances it over the CURRENT step and writes its new record into the other record buffer
 * Neither the particle state nor State round-trip through HBM: per step only the records (48 B in, 48 B out),
 * winds (16 B), ln(qold) (8+8 B) and status (4 B) move.  The last step's scatter+remesh is done by a
 * stand-alone k_scatter when somebody looks (flush()) — that is also the only writer of State in a run
 * of fused steps.  Results are bit-identical to the k_advance + k_scatter sequence.
 * ---------------------------------------------------------------------------------------- */
/* STATIC = false: winds linear in time over the step window (u0,v0 -> u1,v1); the remesh of the previous step
 * needs the wind at ITS start-of-step clock = level 0 of the previous window, kept in (uP, vP) */
/* Occupancy.  The explicit pairs (DP5, Tsit5) are built for 128 VGPRs = FOUR waves per SIMD: with the tableau read through scalar
 * loads (physics.h, TABS) the step needs 137 registers, the cap costs 8 - 27 spilled ones (one scratch access inside
 * the RK loop of the BASELINE flavour, the rest around it), and the fourth wave covers the LDS and hazard waits three waves left open:
 * 2.40 -> 2.28 ms on the BASELINE box with the same instruction count (same-box A/B; at three waves the kernel used 165 of 168
 * registers and no scratch).  The auto-switching flavour (Rosenbrock23 peaks at ~220 live registers) is built for three waves and
 * spills ~140 B per lane: same-box A/B against the spill-free two-wave build gave 3.76 vs 3.81 ms (static winds, aligned), 5.64 vs
 * 5.69 ms (generic direction) and 0.99 vs 1.11 ms on the time-varying-wind flavour (config 5) in round 2's first measurements — the
 * third wave is worth more than the scratch costs; a two-phase split was slower still (profiles/r2_two_phase_auto_experiment.md).
 * The general-physics flavours run at two waves. */
/* WROW = true: the wave-per-row form (k_step_waverow).  The launch covers one range of whole 64-column strips, four rows at a
 * time (the strip branch of rows_index), so a wave's row, its column block and everything derived from them — tile, row bases of the
 * records and of every per-node array, the interior tests of the pull — are the same in all 64 lanes.  The compiler cannot know
 * (threadIdx.x >> 6 is divergent to it); the wave index goes through readfirstlane and all of that arithmetic lands on the scalar unit:
 * a lane adds its own 32-bit offset to a scalar base in the address mode of the load or store.  No fp64 operation differs. */
/* (K_STEP_NAME / K_STEP_WROW: this text is compiled twice, see the head of the file) */
template <bool FAST, bool TSIT, bool STATIC, bool METRIC, bool AUTO>
__global__ void __launch_bounds__(256, (FAST && !AUTO) ? 4 : (FAST ? 3 : 2)) K_STEP_NAME(KParams P, GridP G, Arrays A, double t_prev, double DT_prev,
                                                double t_start, double DT, int r0, int n0, int r1, int n1)
{
    constexpr bool WROW = K_STEP_WROW;
    static_assert(!WROW || (FAST && !METRIC), "k_step_waverow: specialised physics, Cartesian");
#ifdef PICLES_PHASE_CLOCK      /* debug build only: wave cycles per phase into the statistics slots' padding (scripts/phase_clock.py) */
    const unsigned long long pc0_ = __builtin_readcyclecounter();
    unsigned long long pc1_ = pc0_, pc2_ = pc0_, pc3_ = pc0_;
#endif
#ifdef PICLES_WAVE_LOG          /* debug build only: per-wave timeline into the (unused) MovieState planes (scripts/wave_timeline.py) */
    const unsigned long long wl0_ = __builtin_amdgcn_s_memrealtime();
    unsigned long long wl1_ = 0;
#endif
    dp_device_init(TSIT ? 1 : 0);
    order_sign_init();
    const long long ord_counts = order_counts(A);
    const int ord_entry = order_entry(A);
    const int mr_early = pull_reach_early(A);
    pm_device_init();
    long long t = 0;
    const unsigned int lblock = ordered_block(A, ord_counts, ord_entry);
    WaveRow wr = {0, 0, 0};                      /* WROW: the wave's row, first column and first particle, all scalars */
    const unsigned int lane = threadIdx.x & 63u;
    bool active;
    if constexpr (WROW) { active = rows_index_waverow(G, r0, n0, lblock, wr); t = wr.t0 + lane; }
    else active = rows_index(G, r0, n0, r1, n1, t, lblock);
    StepStats S = {{0u, 0u, 0u, 0}, 0u, 0u, 0u, 0u, 0u, 0u, 0};
    int rtile = -1, ccode = -1;
    if (active) {
        int i, jl;
        if constexpr (WROW) { i = wr.i0 + (int)lane; jl = wr.jl; }
        else { i = (int)(t % G.Nx); jl = (int)(t / G.Nx); }
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if constexpr (WROW) rmap_clear_ahead_waverow(A, wr, lane);
        else rmap_clear_ahead(A, t);
        /* the per-node arrays as the lane indexes them: by its particle index from the arrays' bases, or (WROW) by its lane number from
         * the bases moved to the wave's first particle */
        const Arrays Av = WROW ? arrays_at(A, wr.t0) : A;
        const long long tx = WROW ? (long long)lane : t;
        /* what the particle needs from memory besides its node value depends on nothing but its index.  The three-wave (default-solver)
         * kernels issue those loads here, ahead of the pull, so that their round trips overlap the pull's own (the prologue is a chain
         * of dependent memory round trips: a third of a wave's life, measured with the phase clock): -1 %; at four waves per SIMD the
         * registers they occupy across the pull cost more than the overlap gains (+4 %): the explicit pairs load at the point of use */
        constexpr bool PREFETCH = AUTO;
        /* the four-wave static flavours of the wave-per-row form ask for the same values here too, by loads that hold no register: u0,
         * v0 and ln q_old go straight into LDS (kernels.h, stage_fetch_waverow) and are read from there behind the pull; the flags
         * byte takes one register across it */
        constexpr bool STAGE = WROW && STATIC && !AUTO;
        unsigned char pf_pre = 0;
        if constexpr (STAGE) {
            stage_fetch_waverow(Av, lane);
            pf_pre = Av.pflags[tx];
        }
        Wind w_pre = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double qold_pre = 0.0, uP_pre = 0.0, vP_pre = 0.0;
        int asw_pre = 0;
        if constexpr (PREFETCH) {
            pf_pre = Av.pflags[tx];
            w_pre = load_wind(P, Av, tx);
            if constexpr (WROW) w_pre.xi = (unsigned int)t;
            qold_pre = Av.qold[tx];
            asw_pre = Av.asw[tx];
            /* the wind the remesh of the previous step decides with (level 0 of its window): a node without energy — every node of a
             * calm region — asks for it behind the pull otherwise, one more round trip in a wave that consists of round trips */
            if (!STATIC) { uP_pre = Av.uP[tx]; vP_pre = Av.vP[tx]; }
        }
        if constexpr (WROW) {
            int cls;
            const int Rl = pull_reach_local_waverow(G, A, wr, lane, pull_reach(G, A, jl, mr_early), cls);
            pull_waverow(G, A, wr, lane, Rl, cls, s0, s1, s2);
        }
        else pull_any(G, A, i, jl, pull_reach_local(G, A, i, jl, pull_reach(G, A, jl, mr_early)), s0, s1, s2);
#ifdef PICLES_PHASE_CLOCK
        __asm__ volatile("" : "+v"(s0), "+v"(s1), "+v"(s2));
        pc1_ = __builtin_readcyclecounter();
#endif
#ifdef PICLES_WAVE_LOG
        __asm__ volatile("" : "+v"(s0), "+v"(s1), "+v"(s2));
        wl1_ = __builtin_amdgcn_s_memrealtime();
#endif
        /* (s0, s1, s2) is State[k] of the PREVIOUS step.  It is not stored: nobody can read State while a fused step is pending —
         * every observer goes through flush(), whose k_scatter writes the State of the latest step — so the store would be dead
         * (24 B per particle and step of HBM writes, measured: 85 -> 61 B written per particle). */
        unsigned char pf = (PREFETCH || STAGE) ? pf_pre : Av.pflags[tx];
        /* What is needed again only behind the RK loop — the particle index, its node, its flags — waits in LDS instead of in
         * registers: at 128 VGPRs the compiler otherwise spills exactly these to scratch (8 dwords, 36 B per lane and step of extra
         * HBM traffic, measured 135 -> 172 B/particle); two LDS accesses per value cost the same and move nothing. */
        /* (WROW: the index and the node are formed again from the block number, which lives through the loop anyway, and the lane:
         * only the flags wait) */
        __shared__ int stash_[WROW ? 1 : 5][256];
        if (pf & PF_STEPPED) {
            /* (STAGE: load_wind's result under static winds, the two planes and ln q_old read from the wave's stage) */
            if constexpr (STAGE) stage_wait_waverow();
            Wind w = PREFETCH ? w_pre : (STAGE ? stage_wind_waverow(lane) : load_wind(P, Av, tx));
            if constexpr (WROW) w.xi = (unsigned int)t;
            Vec5 z = {0.0, 0.0, 0.0, 0.0, 0.0};
            double qold = PREFETCH ? qold_pre : (STAGE ? (*stage_of_wave())[STAGE_QOLD][lane] : Av.qold[tx]), dtn = -1.0;
            int br = remesh_regs_lazy(P, pf, s0, s1, s2, DT_prev, z, STATIC ? &Av.u0[tx] : (PREFETCH ? &uP_pre : &Av.uP[tx]),
                                      STATIC ? &Av.v0[tx] : (PREFETCH ? &vP_pre : &Av.vP[tx]));
            int on = (br <= 1);
            int asw = AUTO ? (PREFETCH ? asw_pre : Av.asw[tx]) : 0;
            if (br == 1) { qold = PI_LNQOLDINIT; asw = ASW_FRESH; S.reseeds = 1; }
            unsigned int rs = S.reseeds;
            S.reseeds = 0;
            const int tid_ = threadIdx.x;
            if constexpr (WROW) stash_[0][tid_] = (int)pf | ((int)rs << 8);
            else {
                stash_[0][tid_] = (int)(unsigned int)((unsigned long long)t & 0xffffffffull); stash_[1][tid_] = (int)((unsigned long long)t >> 32);
                stash_[2][tid_] = i; stash_[3][tid_] = jl; stash_[4][tid_] = (int)pf | ((int)rs << 8);
            }
            int status;
            if (METRIC) status = advance_core<FAST, STATIC, true, TSIT, AUTO>(P, w, z, on, qold, dtn, t_start, DT, S, Av.m11[tx], Av.m22[tx], Av.pc[tx], &asw);
            else status = advance_core<FAST, STATIC, false, TSIT, AUTO>(P, w, z, on, qold, dtn, t_start, DT, S, 0.0, 0.0, 0.0, &asw);
#ifdef PICLES_PHASE_CLOCK
            __asm__ volatile("" : "+v"(z.lne));
            pc2_ = __builtin_readcyclecounter();
#endif
            /* behind the RK loop: the arguments are read again from the kernarg segment (kernels.h, kargs_reload) */
            KStepArgsPtr K = kargs_reload();
            const KParams Pb = K->P;
            const GridP Gb = K->G;
            const Arrays Ab = K->A;
            __asm__ volatile("" ::: "memory");        /* the stash is read back, not forwarded in registers */
            const int tid2_ = threadIdx.x;
            WaveRow wrb = {0, 0, 0};
            long long tb;
            int ib = 0, jlb = 0, pr_;
            if constexpr (WROW) {
                wrb = waverow_of(Gb, K->r0, lblock);
                tb = wrb.t0 + (threadIdx.x & 63u);
                pr_ = stash_[0][tid2_];
            } else {
                tb = (long long)(((unsigned long long)(unsigned int)stash_[1][tid2_] << 32) | (unsigned int)stash_[0][tid2_]);
                ib = stash_[2][tid2_]; jlb = stash_[3][tid2_]; pr_ = stash_[4][tid2_];
            }
            const unsigned char pfb = (unsigned char)(pr_ & 0xff);
            const Arrays Abv = WROW ? arrays_at(Ab, wrb.t0) : Ab;
            const long long tbx = WROW ? (long long)(threadIdx.x & 63u) : tb;
            status = advance_guards(Pb, [&]() { Wind wg = load_wind(Pb, Abv, tbx); if constexpr (WROW) wg.xi = (unsigned int)tb; return wg; },
                                    z, dtn, K->t_start, K->DT, status, S);
            if (AUTO) Abv.asw[tbx] = asw;
            S.reseeds += (unsigned int)(pr_ >> 8);
            Abv.qold[tbx] = qold;
            Abv.status[tbx] = status;
            if constexpr (WROW) write_record_at(Gb, rec_row_out(Ab, Gb, wrb.jl + Gb.R) + wrb.i0, threadIdx.x & 63u, pfb, on, z, S, &ccode);
            else write_record(Gb, Ab, ib, jlb, pfb, on, z, S);
            rtile = WROW ? (int)(wrb.t0 >> 6) : (int)(tb >> 6);
        }
    }
    {
        KStepArgsPtr K = kargs_reload();
        const Arrays Ab = K->A;
        flush_stats<WROW>(Ab, S, rtile, ccode);
        if (Ab.ord && order_wanted(Ab)) order_file(Ab, lblock, __ballot(S.adv != 0 || S.reseeds != 0) != 0);
#ifdef PICLES_WAVE_LOG
        if ((threadIdx.x & 63) == 0) {
            unsigned int hw_, xcc_;
            __asm__ volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));
            __asm__ volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));
            unsigned long long *wl_ = (unsigned long long *)Ab.movie + 4ull * ((unsigned long long)lblock * 4ull + (threadIdx.x >> 6));
            wl_[0] = wl0_; wl_[1] = wl1_; wl_[2] = __builtin_amdgcn_s_memrealtime();
            wl_[3] = (unsigned long long)hw_ | ((unsigned long long)xcc_ << 32) | ((unsigned long long)blockIdx.x << 40);
        }
#endif
#ifdef PICLES_PHASE_CLOCK
        pc3_ = __builtin_readcyclecounter();
        if ((threadIdx.x & 63) == 0) {
            DevCounters *c = Ab.cnt + ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (NSLOTS - 1));
            if (pc1_ == pc0_) pc1_ = pc3_;
            if (pc2_ < pc1_) pc2_ = pc1_;
            atomicAdd(&c->pad_[0], pc1_ - pc0_); atomicAdd(&c->pad_[1], pc2_ - pc1_); atomicAdd(&c->pad_[2], pc3_ - pc2_); atomicAdd(&c->pad_[3], 1ull);
        }
#endif
    }
}
#endif /* K_STEP_NAME */
