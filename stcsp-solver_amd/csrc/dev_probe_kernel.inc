// dev_probe_kernel.inc -- the body of k_probe and k_probe_big (dev_kernels.hpp), with DR, L, CS, LITE and BS in scope. (Included,
// like dev_expand_kernel.inc, so that the shipped k_probe instances stay exactly what they are.)
    const Ctx &c = *cp;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int lane = threadIdx.x & 63, wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int img_words = (c.stage_words + 3) & ~3;
    if (img_words) {
        const uint4 *src = (const uint4 *)c.img;
        uint4 *dst = (uint4 *)smem;
        for (int k = threadIdx.x; k < img_words / 4; k += 256) dst[k] = src[k];
        __syncthreads();
    }
    const int per_wave = wave_scratch_words(c.NK, c.stack_slots, LITE, c.sib_depth, 1, BS);
    int *lds_vals = smem + img_words + wib * per_wave + (BS ? kBigScopeWords : 0);
    int *lds_stk = lds_vals + kMaxLowVars * 64;
    int *ldom = LITE ? lds_vals : lds_stk + c.stack_slots * 64;
    Img<L> P{c.img, (const uint32_t *)smem, c.stage_words};
    WaveEnv<DR> env;
    for (int gw = blockIdx.x * 4 + wib; gw < n; gw += gridDim.x * 4) {
        uint32_t *blk = blocks + (size_t)gw * c.NK;
        Dom<DR> dom;
#pragma unroll
        for (int q = 0; q < DR; q++) {
            const int idx = q * 64 + lane;
            dom.r[q] = idx < c.NK ? blk[idx] : 0u;
        }
        NodeHdr hd;
        hd.h0 = hd.h1 = 0u;
        hd.set = rfl(set >= 0 ? set : gw);  // (set < 0: block i under constraint set i, and no work counters -- engine.hip fresh_init)
        hd.seed = 0u;
        hd.expire = rflu(expire);
        BranchOut bo;
        LeafOut<DR> lo;
        const int oc = process_node<DR, L, CS, LITE, 1, 1, false, BS>(c, P, lane, lds_vals, lds_stk, ldom, dom, hd, gw, env, bo, lo);
#pragma unroll
        for (int q = 0; q < DR; q++) {
            const int idx = q * 64 + lane;
            if (idx < c.NK) blk[idx] = dom.r[q];
        }
        if (lane == 0) outcome[gw] = oc;
    }
    if (set >= 0) flush_env<DR>(c, env, blockIdx.x * 4 + wib, lane);
