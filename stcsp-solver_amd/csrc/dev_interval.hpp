// dev_interval.hpp -- interval domains (STCSP_F_INTERVAL_DOMAINS): every variable is held as the reference holds it, one pair of
// bounds per look-ahead point (Variable::currLB/currUB, src/variable.h:19-20), whatever its width in [INT_MIN, INT_MAX].
//
// Block layout: chunk-major with two chunks, the layout of the W = 2 bitset blocks -- word (0, p, v) = p * N + v holds the lower
// bound of variable v at point p, word (1, p, v) = N*K + p * N + v the upper bound, both as int32. Everything that only MOVES
// blocks is shared with the bitset kernels; process_node_wide (dev_wide.hpp, W = kWIntervals) calls the revisions below and reads
// bounds where the bitset kernels decode bits.
//
// Propagation is the reference's bounds consistency (enforcePointConsistencyAt, src/solveralgorithm.cpp:476-523):
//  * a constraint in the defining form v == e (v not in e; cset.cpp tags it) moves v's bounds to the least and greatest value of e
//    over the tuples of the other variables that lies in [lb_v, ub_v] (the IMAGE pass) -- one enumeration whatever v's width, and
//    the only way an aux variable of `/` or `%` under next ([INT_MIN, INT_MAX]) gets narrowed; v itself is never enumerated: a
//    value of another variable is supported when e takes a value in [lb_v, ub_v] on some tuple with it;
//  * every other bound is scanned inward from the bound, one support search per candidate (exists support, lanes over tuples).
// No loop here runs longer with a wider domain: an enumeration takes at most the tuple budget (Ctx::budget_*, the W > 1 budget),
// a bound scan at most kIvScanLanes candidates when every other variable is fixed (one per lane, 64 per trip) and kIvScanSerial
// otherwise. A scan or an enumeration over its budget leaves the bound as it is and counts a skipped revision: sound (nothing is
// pruned without proof), and leaves are exact (every variable fixed: one tuple).
#pragma once
#include "dev_propagate.hpp"
namespace stcsp {
namespace dev {

constexpr int kWIntervals = 0;          // the W of k_expand / expand_node / process_node_wide that selects interval domains
constexpr unsigned kIvScanLanes = 1024;  // candidates per bound and revision when every other scope variable is fixed (16 trips)
constexpr unsigned kIvScanSerial = 64;   // ... and when some other one is open (one support search each)
constexpr unsigned kIvMaxTuples = 1u << 24;  // hard cap of one enumeration, whatever STCSP_BUDGET_* ask for

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

enum IvMode : int { IV_EXISTS = 0, IV_DEF = 1, IV_IMAGE = 2 };

// Enumerate the tuples of the scope positions in `em` (wave-uniform, at most kMaxLowVars positions), 64 per trip, each lane
// decoding its tuple index in mixed radix (the first position of `em` fastest): position j takes the values base_j + dir_j * d,
// d < n_j (lane j holds base, dir, n). Every other position reads `curval` (lane j). `total` = product of the n_j (<= the budget).
//   IV_EXISTS: the constraint holds (tuple bitmap or program);  IV_DEF: e (program at e_off) takes a value in [vlo, vhi];
//   IV_IMAGE:  mn / mx = least / greatest value of e in [vlo, vhi] over every tuple (mn > mx: none).
// Returns the least tuple index that qualifies (IV_EXISTS, IV_DEF), -1 if none. Every lane must be active.
template <int L>
__device__ int iv_enumerate(const Ctx &c, const Img<L> &G, const ConDesc &C, int lane, unsigned long long em, int base, int dir, uint32_t n,
                            int curval, int vlb, int mystride, unsigned total, int mode, int e_off, int e_len, int vlo, int vhi, int *lds_vals,
                            int *lds_stk, unsigned long long &n_evals, int &mn, int &mx) {
    const int s = C.scope_len;
    const bool use_bitmap = mode == IV_EXISTS && C.bitmap_off >= 0;
    const uint32_t varinfo = ((em >> lane) & 1ull) ? 1u + (uint32_t)__popcll(em & ((1ull << lane) - 1ull)) : 0u;
    int base_sum = 0;
    if (use_bitmap) base_sum = wave_sum((lane < s && !((em >> lane) & 1ull)) ? (curval - vlb) * mystride : 0);
    mn = INT_MAX;
    mx = INT_MIN;
    const unsigned trips = (total + 63u) >> 6;  // total <= kIvMaxTuples
    for (unsigned trip = 0; trip < trips; trip++) {
        const unsigned t = trip * 64u + (unsigned)lane;
        const bool active = t < total;
        unsigned u = active ? t : 0u;
        int lane_part = 0, slot = 0;
        for (unsigned long long m = em; m; m &= m - 1, slot++) {  // <= kMaxLowVars positions
            const int j = __ffsll((long long)m) - 1;
            const unsigned nj = rdlane(n, j);
            const unsigned q = u / nj, d = u - q * nj;
            u = q;
            const int val = (int)(rdlane((uint32_t)base, j) + (uint32_t)(int)rdlane((uint32_t)dir, j) * d);
            if (use_bitmap)
                lane_part += (val - (int)rdlane((uint32_t)vlb, j)) * (int)rdlane((uint32_t)mystride, j);
            else
                lds_vals[slot * 64 + lane] = val;
        }
        bool ok;
        int val = 0;
        if (use_bitmap) {
            const int bit = base_sum + lane_part;
            ok = active && ((((uint32_t)G.vc(c.o.tables + C.bitmap_off + (bit >> 5))) >> (bit & 31)) & 1u);
        } else if (mode == IV_EXISTS) {
            // (every lane runs the interpreter: it reads its program and the fixed values across lanes)
            const int res = eval_program<L>(c, G, C.code_off, C.code_len, C.uses_valid != 0, lane, varinfo, curval, lds_vals, lds_stk);
            ok = active && res != 0;
        } else {
            val = eval_program<L>(c, G, e_off, e_len, false, lane, varinfo, curval, lds_vals, lds_stk);
            ok = active && val >= vlo && val <= vhi;
        }
        n_evals += min(total - trip * 64u, 64u);
        if (mode == IV_IMAGE) {
            mn = min(mn, wave_min_int(ok ? val : INT_MAX));
            mx = max(mx, wave_max_int(ok ? val : INT_MIN));
            continue;
        }
        const unsigned long long hit = __ballot(ok);
        if (hit) return (int)(trip * 64u) + __ffsll((long long)hit) - 1;
    }
    return -1;
}

// One point constraint at one time point, bounds consistency for every scope variable. `defpos`: scope position of v when the
// constraint is v == e (program of e at e_off), else -1. Returns false on a wipe-out; `changedm`: scope positions whose bounds moved.
template <int L>
__device__ bool revise_bounds_iv(const Ctx &c, const Img<L> &G, const ConDesc &C, int defpos, int e_off, int e_len, int p, int lane, int *ldom,
                                 int *lds_vals, int *lds_stk, unsigned long long &changedm, unsigned long long &n_evals, unsigned &n_skipped) {
    const int s = C.scope_len, NK1 = c.N * c.K;
    const int var = lane < s ? G.v(c.o.scope + C.scope_off + lane) : 0;
    const int word = p * c.N + var;
    int lo = lane < s ? ldom[word] : 0, hi = lane < s ? ldom[NK1 + word] : 0;
    changedm = 0;
    if (__ballot(lane < s && lo > hi)) return false;
    const int lo_in = lo, hi_in = hi;
    const int vlb = lane < s ? G.v(c.o.var_lb + var) : 0;
    const bool use_bitmap = C.bitmap_off >= 0;
    const int mystride = (use_bitmap && lane < s) ? G.v(c.o.strides + C.stride_off + lane) : 0;
    const unsigned budget = (unsigned)min((unsigned long long)(unsigned)(use_bitmap ? c.budget_bitmap : c.budget_code) * 32ull * 64ull,
                                          (unsigned long long)kIvMaxTuples);  // tuples per enumeration
    const unsigned long long defm = defpos >= 0 ? 1ull << defpos : 0ull;
    // product of the domain sizes of the positions in m, saturated at budget + 1 (<= 64 iterations)
    auto product_of = [&](unsigned long long m) -> unsigned {
        unsigned long long P = 1;
        for (; m; m &= m - 1) {
            const int j = __ffsll((long long)m) - 1;
            P *= (unsigned long long)rdlane((uint32_t)hi - (uint32_t)lo, j) + 1ull;
            if (P > budget) return budget + 1u;
        }
        return (unsigned)P;
    };
    int mn = 0, mx = 0;
    const unsigned long long openm = __ballot(lane < s && lo < hi);
    if (!openm) {  // every variable fixed: the single tuple is checked (this is what makes leaves exact)
        return iv_enumerate<L>(c, G, C, lane, 0ull, 0, 0, 1u, lo, vlb, mystride, 1u, IV_EXISTS, 0, 0, 0, 0, lds_vals, lds_stk, n_evals, mn, mx) >= 0;
    }
    // ---- v == e: v's new bounds are the least and greatest value of e over the other variables' tuples inside [lb_v, ub_v]
    if (defpos >= 0) {
        const unsigned long long em = openm & ~defm;
        const unsigned P = product_of(em);
        if (__popcll(em) > kMaxLowVars || P > budget) {
            n_skipped++;
        } else {
            const int vlo = rfl((int)rdlane((uint32_t)lo, defpos)), vhi = rfl((int)rdlane((uint32_t)hi, defpos));
            iv_enumerate<L>(c, G, C, lane, em, lo, 1, (uint32_t)hi - (uint32_t)lo + 1u, lo, vlb, mystride, P, IV_IMAGE, e_off, e_len, vlo, vhi, lds_vals, lds_stk,
                            n_evals, mn, mx);
            mn = rfl(mn);
            mx = rfl(mx);
            if (mn > mx) return false;
            if (lane == defpos) {
                lo = mn;
                hi = mx;
            }
        }
    }
    // ---- the other bounds, scanned inward (<= 64 positions x 2 sides)
    const int mode = defpos >= 0 ? IV_DEF : IV_EXISTS;
    for (unsigned long long m = openm & ~defm; m; m &= m - 1) {
        const int j0 = __ffsll((long long)m) - 1;
        for (int side = 0; side < 2; side++) {
            const int jlo = rfl((int)rdlane((uint32_t)lo, j0)), jhi = rfl((int)rdlane((uint32_t)hi, j0));
            if (jlo == jhi) break;  // (side 1: the least value is supported already)
            const unsigned long long ncand = (unsigned long long)((uint32_t)jhi - (uint32_t)jlo) + 1ull;
            const int bound = side == 0 ? jlo : jhi, dir = side == 0 ? 1 : -1;
            const int vlo = defpos >= 0 ? rfl((int)rdlane((uint32_t)lo, defpos)) : 0, vhi = defpos >= 0 ? rfl((int)rdlane((uint32_t)hi, defpos)) : 0;
            const unsigned long long others = __ballot(lane < s && lo < hi) & ~defm & ~(1ull << j0);
            int found = -1;
            bool gave_up = false;
            if (!others) {
                // every other variable fixed: the candidates themselves go across the lanes, 64 per trip
                const unsigned nc = (unsigned)min(ncand, (unsigned long long)kIvScanLanes);
                found = iv_enumerate<L>(c, G, C, lane, 1ull << j0, bound, dir, nc, lo, vlb, mystride, nc, mode, e_off, e_len, vlo, vhi, lds_vals,
                                        lds_stk, n_evals, mn, mx);
                gave_up = found < 0 && ncand > nc;
            } else {
                const unsigned P = product_of(others);
                if (__popcll(others) > kMaxLowVars || P > budget) {
                    gave_up = true;
                } else {
                    const unsigned nc = (unsigned)min(ncand, (unsigned long long)kIvScanSerial);
                    for (unsigned k = 0; k < nc && found < 0; k++) {  // one support search per candidate
                        const int cand = (int)((uint32_t)bound + (uint32_t)dir * k);
                        const int cv = lane == j0 ? cand : lo;
                        if (iv_enumerate<L>(c, G, C, lane, others, lo, 1, (uint32_t)hi - (uint32_t)lo + 1u, cv, vlb, mystride, P, mode, e_off, e_len, vlo, vhi, lds_vals,
                                            lds_stk, n_evals, mn, mx) >= 0)
                            found = (int)k;
                    }
                    gave_up = found < 0 && ncand > nc;
                }
            }
            if (gave_up) {  // the side keeps its bound
                n_skipped++;
                continue;
            }
            if (found < 0) return false;  // no candidate of the whole domain is supported
            const int nb = (int)((uint32_t)bound + (uint32_t)dir * (uint32_t)found);
            if (lane == j0) {
                if (side == 0)
                    lo = nb;
                else
                    hi = nb;
            }
        }
    }
    const bool ch = lane < s && (lo != lo_in || hi != hi_in);
    changedm = __ballot(ch);
    if (ch) {
        ldom[word] = lo;
        ldom[NK1 + word] = hi;
    }
    STCSP_REJOIN();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return true;
}

// X == next Y at point p (enforceNextConsistency, src/solveralgorithm.cpp:544-593): both get the intersection of X[p] and Y[p+1].
__device__ __forceinline__ bool revise_next_iv(const Ctx &c, int wx, int wy, int lane, int *ldom, bool &chx, bool &chy) {
    const int NK1 = c.N * c.K;
    const int xl = ldom[wx], xh = ldom[NK1 + wx], yl = ldom[wy], yh = ldom[NK1 + wy];
    const int l = max(xl, yl), h = min(xh, yh);
    if (l > h) return false;
    chx = xl != l || xh != h;
    chy = yl != l || yh != h;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        ldom[wx] = l;
        ldom[NK1 + wx] = h;
        ldom[wy] = l;
        ldom[NK1 + wy] = h;
    }
    STCSP_REJOIN();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return true;
}

}  // namespace dev
}  // namespace stcsp
