// dev_expand_kernel.inc -- the body of the expansion kernels, included by k_expand and k_expand_until (dev_kernels.hpp) with
// DR, L, CS, LITE, BIG, W, KR, UW, SHP and BS in scope. (A shared __forceinline__ function instead gives the shipped k_expand instances
// other register allocations.)
    const Ctx &c = *cp;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    // the planned round's gate in ONE 8-byte read (Plan::gate): is it this launch's round, and how many slots has it? The plan
    // pointer is a kernel argument of its own (not read through *cp), so this is the first and only load a workgroup without
    // work waits for. A planner that stops (done, pool full, host needed) leaves the gate on the launch that has just run: the
    // rest of the burst fails this test -- no separate look at the status word.
    static_assert(offsetof(Plan, gate) == 0, "the gate is the plan's first word");
    // ---- ONE batch of independent loads before anything is waited for: the gate, the plan words of the round (through the plan
    // ARGUMENT, not through the pointer inside *cp), the context words the prologue needs and the register copy of the context.
    // (Round 3's prologue was a chain of a dozen dependent scalar loads -- gate, then *cp, then cp->progress, then cp->plan, then
    // plan->rounds, then stage_words, then img, ... -- eight of them first touches of a cache line after the launch boundary, on
    // the critical path of every round. The empty asm below pins the batch in front of the gate test.)
    const kptr pk = (kptr)(const __attribute__((address_space(1))) int *)plan_arg;
    const unsigned long long gate = ((const __attribute__((address_space(4))) unsigned long long *)(const __attribute__((address_space(1))) unsigned long long *)plan_arg)[0];
    auto pl = [&](size_t off) { return (uint32_t)pk[(int)(off / 4)]; };
    const uint32_t p_in_lo = pl(offsetof(Plan, in_base)), p_in_hi = pl(offsetof(Plan, in_base) + 4);
    const uint32_t p_out_lo = pl(offsetof(Plan, out_base)), p_out_hi = pl(offsetof(Plan, out_base) + 4);
    const uint32_t p_in_cap = pl(offsetof(Plan, in_cap)), p_out_cap = pl(offsetof(Plan, out_cap)), p_cand_cap = pl(offsetof(Plan, cand_cap));
    const uint32_t p_parity = pl(offsetof(Plan, parity)), p_rounds = pl(offsetof(Plan, rounds));
    const int c_stage_words = c.stage_words, c_NK = c.NK, c_stack_slots = c.stack_slots, c_sib_depth = c.sib_depth, c_world = c.world;
    const uint32_t *const c_img = c.img;
    uint32_t *const c_arena = c.arena, *const c_cand = c.cand, *const c_ctl = c.ctl;
    Progress *const c_progress = c.progress;
    const int lane = threadIdx.x & 63, wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t hot[2];
#pragma unroll
    for (int q = 0; q < 2; q++) hot[q] = q * 64 + lane < kCtxWords ? ((const uint32_t *)cp)[q * 64 + lane] : 0u;
    asm volatile("" ::"s"(p_in_lo), "s"(p_in_hi), "s"(p_out_lo), "s"(p_out_hi), "s"(p_in_cap), "s"(p_out_cap), "s"(p_cand_cap), "s"(p_parity), "s"(p_rounds),
                 "s"(c_stage_words), "s"(c_NK), "s"(c_stack_slots), "s"(c_sib_depth), "s"(c_world), "s"(c_img), "s"(c_arena), "s"(c_cand), "s"(c_ctl), "s"(c_progress));
    if ((unsigned)(gate >> 32) != launch_id) return;  // another launch's round (this workgroup is late, or the burst ran past a stop)
    const int n_slots = (int)(unsigned)gate;
    const int wpb = BIG ? STCSP_BIG_WAVES : 4;  // wavefronts per workgroup
    // workgroups without a node slot leave at once; the ticket below counts the working ones only
    if ((int)blockIdx.x * wpb >= n_slots) return;
    const unsigned n_working = (unsigned)min((n_slots + wpb - 1) / wpb, (int)gridDim.x);
    if (blockIdx.x == 0 && threadIdx.x == 0 && c_progress)  // (the streaming export's "the round before this one has ended")
        __hip_atomic_store(&c_progress->started, (unsigned long long)(p_rounds + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int img_words = (c_stage_words + 3) & ~3;  // L: the whole image; else a prefix of hot sections (or 0)
    const unsigned long long t_k0 = PHASE_NOW();
    (void)t_k0;
    if (img_words) {
        const uint4 *src = (const uint4 *)c_img;
        uint4 *dst = (uint4 *)smem;
        for (int k = threadIdx.x; k < img_words / 4; k += (BIG ? STCSP_BIG_WAVES * 64 : 256)) dst[k] = src[k];
        __syncthreads();
    }
    const int per_wave = wave_scratch_words(c_NK, c_stack_slots, LITE, c_sib_depth, UW > 1 ? expire_words(c.n_until_cons) : 1, BS);
    int *lds_vals = smem + img_words + wib * per_wave + (BS ? kBigScopeWords : 0);  // (BS: the big-scope table in front)
    int *lds_stk = lds_vals + kMaxLowVars * 64;
    int *ldom = LITE ? lds_vals : lds_stk + c_stack_slots * 64;  // NK-word AND-accumulator of this wavefront, then its counters
    const int sib_off = img_words + wib * per_wave + wave_sib_offset(c_NK, c_stack_slots, LITE, BS);  // word offset in the launch's LDS
    Img<L> P{c_img, (const uint32_t *)smem, c_stage_words};
    ExpandArgs a;
    a.in_base = c_arena + ((unsigned long long)p_in_hi << 32 | p_in_lo);
    a.in_cap = p_in_cap;
    a.out_base = c_arena + ((unsigned long long)p_out_hi << 32 | p_out_lo);
    a.out_cap = p_out_cap;
    a.cand_base = c_cand;
    a.cand_cap = p_cand_cap;
    a.parity = (int)p_parity;
    const int total_waves = gridDim.x * wpb;
    const unsigned long long t_k1 = PHASE_NOW();
    (void)t_k1;
    WaveEnv<DR> env;
    {
        // the state table's generation changes with every solve; the device copy of the context does not have to: the launch
        // brings it along and it goes straight into the register copy the node loops read
        constexpr int gw_ = (int)(offsetof(Ctx, tab_gen) / 4);
        static_assert(gw_ < 64, "tab_gen sits in the first register of the context copy");
        if (lane == gw_) hot[0] = tab_gen;
    }
#ifdef STCSP_STATIC_SLOTS
    for (int gw = blockIdx.x * wpb + wib; gw < n_slots; gw += total_waves) expand_node<DR, L, CS, LITE, W, KR, UW, SHP, BS>(hot, a, P, gw, lane, lds_vals, lds_stk, ldom, sib_off, env);
#else
    // Slots: the first one by position, every further one by ticket -- slots differ widely in cost (a chain of up to `chain`
    // expansions, each anything between a failed sweep and a leaf with a new state), and with a fixed stride the round waits for
    // the wavefront whose share happened to be the dearest. The ticket for the NEXT slot is requested before the current one is
    // expanded (its latency disappears behind the node load); kSlotCursors counters deal interleaved tickets.
    {
        const CtlLayout L_(c_world);
        const int ncur = min(kSlotCursors, (int)gridDim.x);  // (a grid smaller than the counters: every residue needs a workgroup)
        const int cur = (int)blockIdx.x % ncur;
        uint32_t *cursor = c_ctl + L_.slotcur0 + cur * CST;
        for (int gw = blockIdx.x * wpb + wib; gw < n_slots;) {
            unsigned ticket = 0;
            if (lane == 0) ticket = atomicAdd(cursor, 1u);
            if constexpr (DR > 4)
                [[clang::always_inline]] expand_node<DR, L, CS, LITE, W, KR, UW, SHP, BS>(hot, a, P, gw, lane, lds_vals, lds_stk, ldom, sib_off, env, n_slots <= total_waves);
            else
                expand_node<DR, L, CS, LITE, W, KR, UW, SHP, BS>(hot, a, P, gw, lane, lds_vals, lds_stk, ldom, sib_off, env, n_slots <= total_waves);
            gw = total_waves + (int)rflu(ticket) * ncur + cur;
        }
    }
#endif
    flush_env<DR>(c, env, blockIdx.x * wpb + wib, lane);
    __syncthreads();
#ifdef STCSP_PHASES
    if (threadIdx.x == 0) {
        add_stats(c, blockIdx.x, ST_CYC_STAGE, t_k1 - t_k0);
        add_stats(c, blockIdx.x, ST_BLOCKS, 1);
        add_stats(c, blockIdx.x, ST_CYC_BLOCK, PHASE_NOW() - t_k0);
    }
#endif
    if (wib == 0) {
        // No fence on either side of the ticket: what the finalizing wavefront reads of the other workgroups are cursors and
        // counters, all of them written by returning agent-scope atomics that completed before the workgroup's barrier
        // above; the node and edge records themselves are only read by LATER launches (a kernel boundary away). An
        // agent-scope fence here costs 2-3.5 us on the critical path of every round (MI355X_MICROARCH.md, fence table).
        unsigned t = 0;
        if (lane == 0) t = atomicAdd(&c.plan->done_blocks, 1u);
        if (rflu(t) == n_working - 1) {  // last working workgroup: every cursor of this round is final
            if (lane == 0) __hip_atomic_store(&c.plan->done_blocks, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifndef STCSP_STATIC_SLOTS
            // (every other wavefront of the launch has drawn its last ticket: the counters start the next round at zero)
            if (lane < kSlotCursors) __hip_atomic_store(&c.ctl[CtlLayout(c.world).slotcur0 + lane * CST], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
            const unsigned long long t_k2 = PHASE_NOW();
            (void)t_k2;
            const Verdict vd = finalize_round(c, c.plan, lane, launch_id + 1u, a.parity);
            mirror_plan(c, vd, lane);
#ifdef STCSP_PHASES
            if (lane == 0) {
                add_stats(c, 0, ST_CYC_FINAL, PHASE_NOW() - t_k2);
                add_stats(c, 0, ST_ROUNDS_FINAL, 1);
            }
#endif
        }
    }
