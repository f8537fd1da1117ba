// automaton.hip -- the host side of the services on the exported automaton: post-processing, bisimulation quotient, stream monitor,
// generator, repair, alignment, inference, posterior marginals, observer, comparison, components, optimisation and fair CTL, with the kernels they launch. No kernel is shared with the search (engine.hip).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "automaton.hpp"
#include "dev_postproc.hpp"
#include "dev_quotient.hpp"
#include "dev_monitor.hpp"
#include "monitor_host.hpp"
#include "dev_generate.hpp"
#include "generate_host.hpp"
#include "dev_repair.hpp"
#include "dev_align.hpp"
#include "dev_infer.hpp"
#include "dev_posterior.hpp"
#include "dev_observer.hpp"
#include "dev_compare.hpp"
#include "dev_components.hpp"
#include "dev_optimise.hpp"
#include "dev_ctl.hpp"
#include "ctl_host.hpp"
#include "repair_host.hpp"
#include "align_host.hpp"
#include "infer_host.hpp"
#include "posterior_host.hpp"

namespace stcsp {
using namespace dev;

// widest adversarial variable the device post-processing passes take (cover sets of kPostMaxWidth / 32 words per state)
static constexpr long long kPostMaxWidth = 4096;
// the columns of a label row a 0/1 mask over the variables selects
static std::vector<int32_t> observed_columns(const uint8_t *mask, int N) {
    std::vector<int32_t> obs;
    for (int x = 0; x < N; x++)
        if (mask[x]) obs.push_back(x);
    return obs;
}

AutomatonServices::AutomatonServices() = default;
AutomatonServices::~AutomatonServices() {
    if (aln.h_ctl) (void)hipHostFree(aln.h_ctl);
}

int AutomatonServices::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *v.err = buf;
    return code;
}

void AutomatonServices::invalidate() {
    post.done = post.live_done = mon.built = gen.built = false;
    gen.drop_derived();
    mon.host.reset();
}

// Every entry point starts here: takes the view and checks what `who` needs. host_twin: what to use on a sharded solve's merged automaton.
int AutomatonServices::enter(const AutomatonView &view, const char *who, Need need, const char *host_twin) {
    v = view;
    if (v.sharded)
        return host_twin ? fail(STCSP_E_UNSUPPORTED, "%s: the device services are for unsharded engines (%s on the merged automaton)", who, host_twin)
                         : fail(STCSP_E_STATE, "%s: device post-processing is for unsharded engines (merge shards on the host)", who);
    if (!v.exp_on_device) return fail(STCSP_E_STATE, "%s needs the device export of a finished solve (export first)", who);
    if (need == NEED_EXPORT) return STCSP_OK;
    if (!post.done) return fail(STCSP_E_STATE, "%s needs the flags of postprocess() on the last solve", who);
    if (v.truncated) return fail(STCSP_E_STATE, "%s after a truncated solve: the open states of a partial automaton have no known language", who);
    if (need == NEED_MONITOR && !mon.built) return fail(STCSP_E_STATE, "%s needs monitor_build() after the last postprocess()", who);
    if (need == NEED_GENERATOR && !gen.built) return fail(STCSP_E_STATE, "%s needs generator_build() after the last postprocess()", who);
    return STCSP_OK;
}

// The live automaton: forward reachability from a valid root over alive edges (what write_dot walks), on first need after a postprocess()
int AutomatonServices::live_set() {
    if (post.live_done) return STCSP_OK;
    const uint32_t E = (uint32_t)v.exp_edges, S = v.n_states;
    HIPCHK(post.d_live.reserve(S));
    HIPCHK(post.d_lctl.reserve_exact(Q_WORDS));
    uint32_t ctl[Q_WORDS] = {0, 0, 0, 0};
    HIPCHK(hipMemsetAsync(post.d_lctl.p, 0, sizeof ctl, v.stream));
    HIPCHK(hipMemsetAsync(post.d_live.p, 0, S, v.stream));
    HIPCHK(hipMemcpyAsync(post.d_live.p, post.d_pvalid.p, 1, hipMemcpyDeviceToDevice, v.stream));
    for (int sweeps = 0; E; sweeps++) {
        HIPCHK(hipMemsetAsync(post.d_lctl.p + Q_CHANGED, 0, sizeof(uint32_t), v.stream));
        hipLaunchKernelGGL(k_q_reach, dim3((E + 255) / 256), dim3(256), 0, v.stream, E, v.d_osrc, v.d_odst, (const uint8_t *)post.d_palive.p,
                           (const uint8_t *)post.d_pvalid.p, post.d_live.p, post.d_lctl.p);
        HIPCHK(hipMemcpyAsync(ctl, post.d_lctl.p, sizeof ctl, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        if (!ctl[Q_CHANGED]) break;
        if (sweeps > (int)S + 8) return fail(STCSP_E_INTERNAL, "live set: reachability did not converge");
    }
    post.live.resize(S);
    HIPCHK(hipMemcpyAsync(post.live.data(), post.d_live.p, S, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    post.n_live = std::count(post.live.begin(), post.live.end(), 1);
    post.root_live = S > 0 && post.live[0];
    post.live_done = true;
    return STCSP_OK;
}

// The bytes the tables of one batch of streams may take: the environment's, else half of the free memory, 1 MiB at least
int AutomatonServices::table_budget(const char *env_name, size_t &budget) {
    budget = 0;
    if (const char *e = getenv(env_name)) budget = (size_t)std::max(0ll, atoll(e));
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        budget = std::max<size_t>(free_b / 2, (size_t)1 << 20);
    }
    return STCSP_OK;
}

// The next batch of a repair(), infer() or posterior(): the streams from b0 on whose tables, need(len) bytes each, fit the budget together, 65535 at most
template <typename NeedFn>
int AutomatonServices::plan_batch(const char *who, const int64_t *offsets, size_t n, size_t b0, size_t budget, NeedFn need, std::vector<BatchStream> &meta, Batch &b) {
    b = Batch{b0, b0};
    meta.clear();
    while (b.b1 < n && b.b1 - b0 < 65535) {
        const size_t len = (size_t)(offsets[b.b1 + 1] - offsets[b.b1]);
        if (need(len) > budget)
            return fail(STCSP_E_NOMEM, "%s: stream %zu of %zu steps needs %zu bytes of tables, the budget is %zu", who, b.b1, len, need(len), budget);
        if (b.b1 > b0 && b.bytes + need(len) > budget) break;
        meta.push_back(BatchStream{(unsigned long long)b.entries, (unsigned long long)b.steps, (uint32_t)len, (uint32_t)(b.b1 - b0)});
        b.bytes += need(len);
        b.entries += (len + 1) * (size_t)v.n_states;
        b.steps += len;
        b.longest = std::max(b.longest, len);
        b.b1++;
    }
    return STCSP_OK;
}

// What repair(), infer() and posterior() share once the request is checked and the result is sized: label ids and, on request,
// dictionaries on first need, the budget, and per batch of consecutive streams whose tables fit it the upload of the stream
// records and observed rows, then body(batch, nb, first_step, records, rows): the launches and copies of the service.
template <typename Result, typename NeedFn, typename Body>
int AutomatonServices::stream_batches(const char *who, const char *budget_env, int64_t n_streams, const int64_t *offsets, const int32_t *values,
                                      bool dictionaries, NeedFn need, Result *out, Body body) {
    const size_t n = (size_t)n_streams, n_obs = (size_t)gen.n_obs;
    if (!n || !post.root_live) return STCSP_OK;
    if (int rc = lab.built ? STCSP_OK : repair_labels()) return rc;
    if (int rc = !dictionaries || dict.built ? STCSP_OK : infer_dictionaries()) return rc;
    size_t budget = 0;
    if (int rc = table_budget(budget_env, budget)) return rc;
    HIPCHK(ev.ready(8));
    std::vector<BatchStream> meta;
    for (size_t b0 = 0; b0 < n;) {
        Batch b;
        if (int rc = plan_batch(who, offsets, n, b0, budget, need, meta, b)) return rc;
        const size_t nb = b.b1 - b0, cells = b.steps * n_obs, first_step = (size_t)offsets[b0];
        HIPCHK(bat.d_streams.reserve(nb));
        HIPCHK(bat.d_rows.reserve(cells));
        HIPCHK(hipMemcpyAsync(bat.d_streams.p, meta.data(), nb * sizeof(BatchStream), hipMemcpyHostToDevice, v.stream));
        if (cells) HIPCHK(hipMemcpyAsync(bat.d_rows.p, values + first_step * n_obs, cells * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
        if (int rc = body(b, nb, first_step, (const BatchStream *)bat.d_streams.p, (const int32_t *)bat.d_rows.p)) return rc;
        out->n_batches++;
        out->table_bytes = std::max<int64_t>(out->table_bytes, (int64_t)b.bytes);
        b0 = b.b1;
    }
    out->n_labels = lab.n_labels;
    return STCSP_OK;
}

// Every (table, count) of a batch with reserve_or_release(), or none: all released and the service's message
template <typename... Tables>
int AutomatonServices::reserve_tables(const char *who, size_t bytes, Tables &&...tables) {
    return reserve_or_release_all(true, tables...) ? (int)STCSP_OK : fail(STCSP_E_NOMEM, "%s: no room for %zu bytes of tables", who, bytes);
}

// What components(), optimise() and ctl() share: the timed batch of launches, ...
hipError_t AutomatonServices::LaunchBatch::begin() {
    hipError_t e = open ? hipSuccess : ev.ready(2);
    if (e == hipSuccess && !open) e = hipEventRecord(ev[0], stream);
    open = true;
    return e;
}
hipError_t AutomatonServices::LaunchBatch::flush() {
    float batch_ms = 0;
    hipError_t e = begin();
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_ctl, d_ctl, words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipEventElapsedTime(&batch_ms, ev[0], ev[1]);
    ms += batch_ms;
    open = false;
    return e;
}

// ... the fixpoint of sweeps: a batch clears the control word `changed`, launches step(i) for the next kBatch sweeps i (from 0) and ends
// with one look at the word; past the fixpoint a sweep changes nothing. Past `bound` sweeps: `diverged`, which may print them (%u).
template <typename Step>
int AutomatonServices::batched_fixpoint(LaunchBatch &run, int changed, uint32_t bound, const char *diverged, Step step) {
    for (uint32_t done = 0;;) {
        HIPCHK(run.begin());
        HIPCHK(hipMemsetAsync(run.d_ctl + changed, 0, sizeof(uint32_t), v.stream));
        for (int b = 0; b < kBatch; b++)
            if (int rc = step(done++)) return rc;
        HIPCHK(run.flush());
        if (!run.h_ctl[changed]) return STCSP_OK;
        if (done > bound) return fail(STCSP_E_INTERNAL, diverged, done);
    }
}

// ... the CSR group, first half: the out-degrees over the edges that are alive with both ends in `states`, their scan, and the total read
// back at the end of the batch (too_many: the caller's message for one past the export, %u of %u). A byte budget is checked here ...
int AutomatonServices::csr_count(LaunchBatch &run, const uint8_t *states, const char *too_many, uint32_t &count) {
    const uint32_t E = (uint32_t)v.exp_edges, S = v.n_states;
    HIPCHK(reserve_all(S, 1, csr.deg, csr.off, csr.cur));
    csr.states = states;
    HIPCHK(run.begin());
    HIPCHK(hipMemsetAsync(csr.deg.p, 0, (size_t)S * sizeof(uint32_t), v.stream));
    if (E)
        hipLaunchKernelGGL(k_s_count, dim3((E + 255) / 256), dim3(256), 0, v.stream, E, v.d_osrc, v.d_odst, (const uint8_t *)post.d_palive.p, states, csr.deg.p);
    hipLaunchKernelGGL(k_s_scan, dim3(1), dim3(256), 0, v.stream, S, (S + 255) / 256, (const uint32_t *)csr.deg.p, csr.off.p, csr.cur.p);
    HIPCHK(hipMemcpyAsync(&csr.n, csr.off.p + S, sizeof csr.n, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(run.flush());
    if ((count = csr.n) > E) return fail(STCSP_E_INTERNAL, too_many, count, E);
    return STCSP_OK;
}

// ... before the second half: room for the positions, and the launch that fills them
int AutomatonServices::csr_fill() {
    const uint32_t E = (uint32_t)v.exp_edges;
    HIPCHK(reserve_all(csr.n, 1, csr.src, csr.dst, csr.eid));
    if (csr.n)
        hipLaunchKernelGGL(k_s_fill, dim3((E + 255) / 256), dim3(256), 0, v.stream, E, v.d_osrc, v.d_odst, (const uint8_t *)post.d_palive.p, csr.states,
                           csr.cur.p, csr.n, csr.src.p, csr.dst.p, csr.eid.p);
    return STCSP_OK;
}

// ... and the label rows of the n export edges a walk wrote, from the pinned export (past_export: the caller's message, %u of %u)
int AutomatonServices::walked_rows(const uint32_t *eid, size_t n, const char *past_export, std::vector<int32_t> &rows) {
    const size_t E = v.exp_edges, N = (size_t)v.N;
    for (size_t t = 0; t < n; t++) {
        if (eid[t] >= E) return fail(STCSP_E_INTERNAL, past_export, eid[t], (uint32_t)E);
        rows.insert(rows.end(), v.h_oval + eid[t] * N, v.h_oval + (eid[t] + 1) * N);
    }
    return STCSP_OK;
}

// graphTraverse / adversarialTraverse / adversarialTraverse2 on the device (dev_postproc.hpp)
int AutomatonServices::postprocess(const AutomatonView &view, const stcsp_post_options *po, stcsp_post_result *out) {
    if (int rc = enter(view, "postprocess", NEED_EXPORT, nullptr)) return rc;
    const int N = v.N;
    const int a1 = po ? po->adversarial_var : -1, op = po ? po->adversarial2_op : -1, ava = po ? po->adversarial2_ava : -1;
    if (a1 >= N || op >= N || ava >= N || a1 < -1 || op < -1 || (op >= 0 && ava < 0))
        return fail(STCSP_E_INVALID, "postprocess: variable index out of range");
    auto t0 = std::chrono::steady_clock::now();
    invalidate();
    const size_t E = v.exp_edges;
    const uint32_t S = v.n_states;
    auto width = [&](int x) { return (long long)v.ub[x] - (long long)v.lb[x] + 1; };
    // cover sets of CW = ceil(width / 32) words (dev_postproc.hpp); without interval domains widths are at most 128 (create()
    // refuses wider), with them the adversarial variables may have at most kPostMaxWidth values
    for (int x : {a1, op, op >= 0 ? ava : -1})
        if (x >= 0 && width(x) > kPostMaxWidth)
            return fail(STCSP_E_UNSUPPORTED, "postprocess: variable %d has %lld values; the device adversarial passes take at most %lld (%lld cover words per state)",
                        x, width(x), kPostMaxWidth, kPostMaxWidth / 32);
    auto cover_w = [&](int x) { return (int)((width(x) + 31) / 32); };
    auto last_full = [&](int x) { return width(x) % 32 == 0 ? 0xffffffffu : ((1u << (width(x) % 32)) - 1u); };
    const int wa = op >= 0 ? (int)width(ava) : 0;
    const int cw1 = a1 >= 0 ? cover_w(a1) : 1, cw2 = op >= 0 ? cover_w(op) : 1;
    HIPCHK(reserve_all(S, 0, post.d_pvalid, post.d_pfinal, post.d_pnodeok));
    const size_t cover_words = (size_t)S * std::max(cw1, std::max(1, wa) * cw2);
    HIPCHK(post.d_pcover.reserve(cover_words));
    HIPCHK(post.d_palive.reserve(E, 1));
    HIPCHK(post.d_pctl.reserve_exact(4));
    const unsigned eb = (unsigned)((E + 255) / 256), sb = (S + 255) / 256;
    const long long *src = v.d_osrc, *dst = v.d_odst;
    const int32_t *val = v.d_oval;
    uint32_t *changed = post.d_pctl.p;
    // one round = the kernels `body` enqueues; returns the number of rounds until nothing changed
    auto fixpoint = [&](int &rounds, auto body) -> int {  // HIPCHK returns the error code from the enclosing lambda
        for (rounds = 0;; rounds++) {
            HIPCHK(hipMemsetAsync(changed, 0, sizeof(uint32_t), v.stream));
            const int rb = body();
            if (rb != STCSP_OK) return rb;
            uint32_t ch = 0;
            HIPCHK(hipMemcpyAsync(&ch, changed, sizeof ch, hipMemcpyDeviceToHost, v.stream));
            HIPCHK(hipStreamSynchronize(v.stream));
            if (!ch) return STCSP_OK;
            if (rounds > (int)S + 8) return fail(STCSP_E_INTERNAL, "post-processing fixpoint did not converge");
        }
    };
    int rounds[3] = {0, 0, 0};
    HIPCHK(hipMemsetAsync(post.d_palive.p, 1, E + 1, v.stream));
    // graphTraverse (src/graph.cpp:357-418); the loop bound numSignVar + numUntil is the reference's
    hipLaunchKernelGGL(k_trav_init, dim3(sb), dim3(256), 0, v.stream, S, (const uint32_t *)v.d_state_keys, v.KL, v.n_sig,
                       v.n_sig + v.n_until, (int)(v.n_until_cons == 0), post.d_pvalid.p, post.d_pfinal.p);
    if (E) {
        if (int rc = fixpoint(rounds[0], [&] {
            hipLaunchKernelGGL(k_trav_back, dim3(eb), dim3(256), 0, v.stream, (uint32_t)E, src, dst, (const uint8_t *)post.d_palive.p, post.d_pvalid.p, changed);
            return (int)STCSP_OK;
        })) return rc;
        hipLaunchKernelGGL(k_kill_into_invalid, dim3(eb), dim3(256), 0, v.stream, (uint32_t)E, src, dst, post.d_palive.p, (const uint8_t *)post.d_pvalid.p, 1);
    }
    int adver1 = -1, adver2 = -1;
    uint8_t root_valid = 0;
    if (a1 >= 0) {  // adversarialTraverse (src/graph.cpp:304-355)
        const uint32_t full = last_full(a1);
        if (int rc = fixpoint(rounds[1], [&] {
            HIPCHK(hipMemsetAsync(post.d_pcover.p, 0, (size_t)S * cw1 * sizeof(uint32_t), v.stream));
            if (E)
                hipLaunchKernelGGL(k_adv_cover, dim3(eb), dim3(256), 0, v.stream, (uint32_t)E, src, dst, val, N, a1, v.lb[a1], cw1,
                                   (const uint8_t *)post.d_palive.p, (const uint8_t *)post.d_pvalid.p, post.d_pcover.p);
            hipLaunchKernelGGL(k_adv_check, dim3(sb), dim3(256), 0, v.stream, S, (const uint32_t *)post.d_pcover.p, cw1, full, post.d_pvalid.p, changed);
            return (int)STCSP_OK;
        })) return rc;
        if (E) hipLaunchKernelGGL(k_kill_into_invalid, dim3(eb), dim3(256), 0, v.stream, (uint32_t)E, src, dst, post.d_palive.p, (const uint8_t *)post.d_pvalid.p, 0);
        HIPCHK(hipMemcpyAsync(&root_valid, post.d_pvalid.p, 1, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        adver1 = root_valid;
    }
    if (op >= 0) {  // adversarialTraverse2 (src/graph.cpp:247-302)
        const uint32_t full = last_full(op);
        if (int rc = fixpoint(rounds[2], [&] {
            HIPCHK(hipMemsetAsync(post.d_pcover.p, 0, (size_t)S * wa * cw2 * sizeof(uint32_t), v.stream));
            if (E)
                hipLaunchKernelGGL(k_adv2_cover, dim3(eb), dim3(256), 0, v.stream, (uint32_t)E, src, dst, val, N, op, ava, v.lb[op], v.lb[ava],
                                   wa, cw2, (const uint8_t *)post.d_palive.p, (const uint8_t *)post.d_pvalid.p, post.d_pcover.p);
            hipLaunchKernelGGL(k_adv2_check, dim3(sb), dim3(256), 0, v.stream, S, (const uint32_t *)post.d_pcover.p, wa, cw2, full, post.d_pvalid.p, post.d_pnodeok.p,
                               changed);
            if (E)
                hipLaunchKernelGGL(k_adv2_kill, dim3(eb), dim3(256), 0, v.stream, (uint32_t)E, src, dst, val, N, ava, v.lb[ava], wa, cw2, full, post.d_palive.p,
                                   (const uint8_t *)post.d_pvalid.p, (const uint8_t *)post.d_pnodeok.p, (const uint32_t *)post.d_pcover.p);
            return (int)STCSP_OK;
        })) return rc;
        HIPCHK(hipMemcpyAsync(&root_valid, post.d_pvalid.p, 1, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        adver2 = root_valid;
        // the reference drops the edges into invalid states only when the root survived (graph.cpp:288-301)
        if (root_valid && E)
            hipLaunchKernelGGL(k_kill_into_invalid, dim3(eb), dim3(256), 0, v.stream, (uint32_t)E, src, dst, post.d_palive.p, (const uint8_t *)post.d_pvalid.p, 0);
    }
    HIPCHK(hipGetLastError());
    post.p_valid.resize(S);
    post.p_final.resize(S);
    post.p_alive.resize(E + 1);
    HIPCHK(hipMemcpyAsync(post.p_valid.data(), post.d_pvalid.p, S, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipMemcpyAsync(post.p_final.data(), post.d_pfinal.p, S, hipMemcpyDeviceToHost, v.stream));
    if (E) HIPCHK(hipMemcpyAsync(post.p_alive.data(), post.d_palive.p, E, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    memset(out, 0, sizeof *out);
    out->n_states = S;
    out->n_edges = (int64_t)E;
    out->state_valid = post.p_valid.data();
    out->state_final = post.p_final.data();
    out->edge_alive = post.p_alive.data();
    out->adver1 = adver1;
    out->adver2 = adver2;
    for (int i = 0; i < 3; i++) out->rounds[i] = rounds[i];
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    post.done = true;
    return STCSP_OK;
}

// Bisimulation quotient of the live automaton on the device (dev_quotient.hpp): classes of the
// states that are valid and reachable from the root over alive edges, under the labels projected on `observable`.
int AutomatonServices::quotient(const AutomatonView &view, const stcsp_quotient_options *qo, stcsp_quotient_result *out) {
    if (int rc = enter(view, "quotient", NEED_FLAGS, "stcsp_automaton_bisimulation")) return rc;
    auto t0 = std::chrono::steady_clock::now();
    const int N = v.N;
    const uint32_t E = (uint32_t)v.exp_edges, S = v.n_states;
    const std::vector<int32_t> obs = observed_columns(qo && qo->observable ? qo->observable : v.default_observable, N);
    auto pow2 = [](size_t n) {
        size_t c = 1024;
        while (c < 2 * n) c <<= 1;
        return c;
    };
    const size_t cap_e = pow2(E), cap_s = pow2(S);
    if (cap_e > 0x80000000ull) return fail(STCSP_E_NOMEM, "edge list too large for the device quotient");
    if (int rc = live_set()) return rc;
    HIPCHK(reserve_all(S, 0, quo.d_qcls[0], quo.d_qcls[1], quo.d_qacc[0], quo.d_qacc[1], quo.d_qcnt));
    HIPCHK(reserve_all(E, 1, quo.d_qsrc, quo.d_qdst, quo.d_qlid));
    HIPCHK(quo.d_qtab_e.reserve_exact(cap_e));
    HIPCHK(quo.d_qtab_s.reserve_exact(cap_s));
    HIPCHK(quo.d_qobs.reserve_exact((size_t)N));
    HIPCHK(quo.d_qctl.reserve_exact(Q_WORDS));
    const unsigned eb = (E + 255) / 256, sb = (S + 255) / 256;
    const uint32_t mask_e = (uint32_t)(cap_e - 1), mask_s = (uint32_t)(cap_s - 1);
    uint32_t ctl[Q_WORDS] = {0, 0, 0, 0};
    auto check = [&]() -> int {
        HIPCHK(hipMemcpyAsync(ctl, quo.d_qctl.p, sizeof ctl, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        if (ctl[Q_ERROR] & Q_ERR_TABLE_FULL) return fail(STCSP_E_INTERNAL, "quotient: a device table overflowed");
        if (ctl[Q_ERROR]) return fail(STCSP_E_INTERNAL, "quotient: a state differs from its class representative (signature collision, flags %u)", ctl[Q_ERROR]);
        return STCSP_OK;
    };
    if (!obs.empty()) HIPCHK(hipMemcpyAsync(quo.d_qobs.p, obs.data(), obs.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    HIPCHK(hipMemsetAsync(quo.d_qctl.p, 0, sizeof ctl, v.stream));
    // label ids (the one sweep over the label rows) and the 12-byte edge records of the rounds
    if (E) {
        HIPCHK(hipMemsetAsync(quo.d_qtab_e.p, 0xff, cap_e * sizeof(uint32_t), v.stream));
        hipLaunchKernelGGL(k_q_labels, dim3(eb), dim3(256), 0, v.stream, E, (const long long *)v.d_osrc, (const long long *)v.d_odst,
                           (const int32_t *)v.d_oval, N, (const int32_t *)quo.d_qobs.p, (int)obs.size(), (const uint8_t *)post.d_palive.p,
                           (const uint8_t *)post.d_live.p, quo.d_qtab_e.p, mask_e, quo.d_qsrc.p, quo.d_qdst.p, quo.d_qlid.p, quo.d_qctl.p);
    }
    // every live state starts in class 0; a round splits the classes by (final, set of (label id, class of destination))
    HIPCHK(hipMemsetAsync(quo.d_qcls[0].p, 0, (size_t)S * sizeof(uint32_t), v.stream));
    int cur = 0, rounds = 0;
    bool dedup = true;  // until round 1 has shown that no state has two edges with one projected label
    auto edge_sweep = [&](bool dd) -> int {
        hipLaunchKernelGGL(k_q_state_init, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_pfinal.p, quo.d_qacc[0].p, quo.d_qacc[1].p, quo.d_qcnt.p);
        if (!E) return STCSP_OK;
        if (dd) HIPCHK(hipMemsetAsync(quo.d_qtab_e.p, 0xff, cap_e * sizeof(uint32_t), v.stream));
        hipLaunchKernelGGL(k_q_edges, dim3(eb), dim3(256), 0, v.stream, E, (const uint32_t *)quo.d_qsrc.p, (const uint32_t *)quo.d_qdst.p,
                           (const uint32_t *)quo.d_qlid.p, (const uint32_t *)quo.d_qcls[cur].p, (int)dd, quo.d_qtab_e.p, mask_e, quo.d_qacc[0].p, quo.d_qacc[1].p,
                           quo.d_qcnt.p, quo.d_qctl.p);
        return STCSP_OK;
    };
    for (uint32_t prev = 0;;) {
        rounds++;
        HIPCHK(hipMemsetAsync(quo.d_qctl.p, 0, 2 * sizeof(uint32_t), v.stream));  // Q_CLASSES, Q_DUPS
        if (int rc = edge_sweep(dedup)) return rc;
        HIPCHK(hipMemsetAsync(quo.d_qtab_s.p, 0xff, cap_s * sizeof(uint32_t), v.stream));
        hipLaunchKernelGGL(k_q_number, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_live.p, (const uint32_t *)quo.d_qcls[cur].p,
                           (const unsigned long long *)quo.d_qacc[0].p, (const unsigned long long *)quo.d_qacc[1].p, quo.d_qtab_s.p, mask_s,
                           quo.d_qcls[1 - cur].p, quo.d_qctl.p);
        if (int rc = check()) return rc;
        cur = 1 - cur;
        if (rounds == 1 && ctl[Q_DUPS] == 0) dedup = false;
        if (ctl[Q_CLASSES] == prev) break;
        prev = ctl[Q_CLASSES];
        if ((uint32_t)rounds > S + 1) return fail(STCSP_E_INTERNAL, "quotient: refinement did not converge");
    }
    // exact verification against the class representatives; leaves the distinct pairs per state in d_qcnt
    if (int rc = edge_sweep(true)) return rc;
    if (E)
        hipLaunchKernelGGL(k_q_verify_edges, dim3(eb), dim3(256), 0, v.stream, E, (const uint32_t *)quo.d_qsrc.p, (const uint32_t *)quo.d_qdst.p,
                           (const uint32_t *)quo.d_qlid.p, (const uint32_t *)quo.d_qcls[cur].p, (const uint32_t *)quo.d_qtab_e.p, mask_e, quo.d_qctl.p);
    hipLaunchKernelGGL(k_q_verify_states, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_live.p, (const uint8_t *)post.d_pfinal.p,
                       (const uint32_t *)quo.d_qcls[cur].p, (const uint32_t *)quo.d_qcnt.p, quo.d_qctl.p);
    HIPCHK(hipGetLastError());
    quo.q_raw.resize(S);
    quo.q_cnt.resize(S);
    HIPCHK(hipMemcpyAsync(quo.q_raw.data(), quo.d_qcls[cur].p, (size_t)S * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipMemcpyAsync(quo.q_cnt.data(), quo.d_qcnt.p, (size_t)S * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
    if (int rc = check()) return rc;
    // canonical class numbers: by least member (the first state, in index order, that shows the class)
    quo.q_class.assign(S, -1);
    std::vector<int32_t> number(S, -1);
    int64_t n_classes = 0, n_class_edges = 0;
    for (uint32_t s = 0; s < S; s++) {
        const uint32_t r = quo.q_raw[s];
        if (r == kQEmpty) continue;  // (not live)
        if (number[r] < 0) {
            number[r] = (int32_t)n_classes++;
            n_class_edges += quo.q_cnt[r];
        }
        quo.q_class[s] = number[r];
    }
    memset(out, 0, sizeof *out);
    out->n_states = post.n_live;
    out->n_classes = n_classes;
    out->n_class_edges = n_class_edges;
    out->state_class = quo.q_class.data();
    out->rounds = rounds;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Stream monitor, build (dev_monitor.hpp): label ids and the (state, label id) -> destinations
// multimap of the live automaton under one mask, from the flags the last postprocess() left in HBM.
int AutomatonServices::monitor_build(const AutomatonView &view, const stcsp_monitor_options *mo, stcsp_monitor_info *info) {
    if (int rc = enter(view, "monitor_build", NEED_FLAGS, "stcsp_automaton_check_streams")) return rc;
    auto t0 = std::chrono::steady_clock::now();
    mon.built = false;
    mon.host.reset();
    const int N = v.N;
    const uint32_t E = (uint32_t)v.exp_edges, S = v.n_states;
    const uint8_t *mask = mo && mo->observable ? mo->observable : v.default_observable;
    const std::vector<int32_t> obs = observed_columns(mask, N);
    mon.observable.assign(mask, mask + N);
    size_t cap = 1024;
    while (cap < 2 * (size_t)E) cap <<= 1;
    if (cap > 0x80000000ull) return fail(STCSP_E_NOMEM, "edge list too large for the device monitor");
    if (int rc = live_set()) return rc;
    HIPCHK(reserve_all(E, 1, mon.d_mdst, mon.d_mnext));
    HIPCHK(mon.d_mltab.reserve_exact(cap));
    HIPCHK(mon.d_mhead.reserve_exact(cap));
    HIPCHK(mon.d_mdst0.reserve_exact(cap));
    HIPCHK(mon.d_mkeys.reserve_exact(cap));
    HIPCHK(mon.d_mobs.reserve_exact((size_t)N));
    HIPCHK(mon.d_mctl.reserve_exact(M_WORDS));
    const unsigned eb = (E + 255) / 256;
    uint32_t ctl[M_WORDS] = {0};
    if (!obs.empty()) HIPCHK(hipMemcpyAsync(mon.d_mobs.p, obs.data(), obs.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    HIPCHK(hipMemsetAsync(mon.d_mctl.p, 0, sizeof ctl, v.stream));
    if (E) {
        HIPCHK(hipMemsetAsync(mon.d_mltab.p, 0xff, cap * sizeof(uint32_t), v.stream));
        HIPCHK(hipMemsetAsync(mon.d_mhead.p, 0xff, cap * sizeof(uint32_t), v.stream));
        HIPCHK(hipMemsetAsync(mon.d_mkeys.p, 0xff, cap * sizeof(unsigned long long), v.stream));
        hipLaunchKernelGGL(k_m_build, dim3(eb), dim3(256), 0, v.stream, E, (const long long *)v.d_osrc, (const long long *)v.d_odst,
                           (const int32_t *)v.d_oval, N, (const int32_t *)mon.d_mobs.p, (int)obs.size(), (const uint8_t *)post.d_palive.p,
                           (const uint8_t *)post.d_live.p, mon.d_mltab.p, mon.d_mkeys.p, mon.d_mhead.p, (uint32_t)(cap - 1), mon.d_mdst.p, mon.d_mnext.p, mon.d_mctl.p);
        hipLaunchKernelGGL(k_m_finish, dim3((unsigned)(cap / 256)), dim3(256), 0, v.stream, (uint32_t)cap, (const unsigned long long *)mon.d_mkeys.p,
                           (const uint32_t *)mon.d_mhead.p, mon.d_mnext.p, (const uint32_t *)mon.d_mdst.p, mon.d_mdst0.p, mon.d_mctl.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(ctl, mon.d_mctl.p, sizeof ctl, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    if (ctl[M_ERROR]) return fail(STCSP_E_INTERNAL, "monitor: a device table overflowed");
    mon.n_obs = (int)obs.size();
    mon.max_dst = (int)std::max(ctl[M_MAXDST], ctl[M_PAIRS] ? 1u : 0u);
    mon.mask = (uint32_t)(cap - 1);
    mon.built = true;
    memset(info, 0, sizeof *info);
    info->n_states = post.n_live;
    info->n_edges = ctl[M_EDGES];
    info->n_labels = ctl[M_LABELS];
    info->n_pairs = ctl[M_PAIRS];
    info->table_bytes = (int64_t)(E ? cap * (3 * sizeof(uint32_t) + sizeof(unsigned long long)) + 2 * (size_t)E * sizeof(uint32_t) : 0) + S;
    info->n_observable = mon.n_obs;
    info->max_destinations = mon.max_dst;
    info->set_capacity = kMonSetCap;
    info->root_live = post.root_live;
    info->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Stream monitor, check: every stream's accepted_len / n_end / end_final (contract: stcsp_engine.h). Exact always: the
// streams the state-set kernel marks as over its capacity are finished by the host twin (monitor_host.hpp).
int AutomatonServices::monitor_check(const AutomatonView &view, const stcsp_monitor_streams *ms, stcsp_monitor_result *out) {
    if (int rc = enter(view, "monitor_check", NEED_MONITOR, "stcsp_automaton_check_streams")) return rc;
    if (!monitor_offsets_ok(ms->n_streams, ms->offsets)) return fail(STCSP_E_INVALID, "monitor_check: malformed stream offsets");
    auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)ms->n_streams;
    const size_t steps = n ? (size_t)ms->offsets[n] : 0;
    if (steps && mon.n_obs && !ms->values) return fail(STCSP_E_INVALID, "monitor_check: no step values");
    if (n >= 0x7fffffffull || steps >= 0x7fffffffull) return fail(STCSP_E_NOMEM, "monitor_check: too many streams or steps for one call");
    mon.m_acc.assign(n, 0);
    mon.m_nend.assign(n, 0);
    mon.m_fin.assign(n, 0);
    memset(out, 0, sizeof *out);
    out->n_streams = ms->n_streams;
    out->accepted_len = mon.m_acc.data();
    out->n_end = mon.m_nend.data();
    out->end_final = mon.m_fin.data();
    if (n && post.root_live) {
        const bool sets = mon.max_dst > 1 || (ms->flags & STCSP_MON_FORCE_SETS);
        const uint32_t E = (uint32_t)v.exp_edges;
        HIPCHK(mon.d_moff.reserve(n, 1));
        HIPCHK(reserve_all(n, 0, mon.d_macc, mon.d_mnend, mon.d_mfin));
        HIPCHK(mon.d_mlid.reserve(steps));
        HIPCHK(mon.d_mrows.reserve(steps * mon.n_obs));
        HIPCHK(ev.ready(3));
        HIPCHK(hipMemcpyAsync(mon.d_moff.p, ms->offsets, (n + 1) * sizeof(long long), hipMemcpyHostToDevice, v.stream));
        if (steps * mon.n_obs) HIPCHK(hipMemcpyAsync(mon.d_mrows.p, ms->values, steps * mon.n_obs * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipMemsetAsync(mon.d_mctl.p + M_OVERFLOW, 0, sizeof(uint32_t), v.stream));
        HIPCHK(hipEventRecord(ev[0], v.stream));
        if (steps) {
            if (E)
                hipLaunchKernelGGL(k_m_steps, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)steps, (const int32_t *)mon.d_mrows.p,
                                   mon.n_obs, (const int32_t *)v.d_oval, v.N, (const int32_t *)mon.d_mobs.p, (const uint32_t *)mon.d_mltab.p, mon.mask,
                                   mon.d_mlid.p);
            else  // no edge, no label: every step is a rejection
                HIPCHK(hipMemsetAsync(mon.d_mlid.p, 0xff, steps * sizeof(uint32_t), v.stream));
        }
        HIPCHK(hipEventRecord(ev[1], v.stream));
        if (sets)
            hipLaunchKernelGGL(k_m_walk_sets, dim3((unsigned)n), dim3(64), 0, v.stream, (uint32_t)n, (const long long *)mon.d_moff.p,
                               (const uint32_t *)mon.d_mlid.p, (const unsigned long long *)mon.d_mkeys.p, (const uint32_t *)mon.d_mhead.p,
                               (const uint32_t *)mon.d_mnext.p, (const uint32_t *)mon.d_mdst.p, mon.mask, (const uint8_t *)post.d_pfinal.p, mon.d_macc.p, mon.d_mnend.p,
                               mon.d_mfin.p, mon.d_mctl.p);
        else
            hipLaunchKernelGGL(k_m_walk_det, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)n, (const long long *)mon.d_moff.p,
                               (const uint32_t *)mon.d_mlid.p, (const unsigned long long *)mon.d_mkeys.p, (const uint32_t *)mon.d_mdst0.p, mon.mask,
                               (const uint8_t *)post.d_pfinal.p, mon.d_macc.p, mon.d_mnend.p, mon.d_mfin.p);
        HIPCHK(hipEventRecord(ev[2], v.stream));
        HIPCHK(hipGetLastError());
        uint32_t over = 0;
        HIPCHK(hipMemcpyAsync(mon.m_acc.data(), mon.d_macc.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(mon.m_nend.data(), mon.d_mnend.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(mon.m_fin.data(), mon.d_mfin.p, n, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(&over, mon.d_mctl.p + M_OVERFLOW, sizeof over, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        float ms_l = 0, ms_w = 0;
        HIPCHK(hipEventElapsedTime(&ms_l, ev[0], ev[1]));
        HIPCHK(hipEventElapsedTime(&ms_w, ev[1], ev[2]));
        out->seconds_labels = ms_l * 1e-3;
        out->seconds_walk = ms_w * 1e-3;
        out->walk_kernel = sets ? 2 : 1;
        if (over) {
            if (!mon.host) {
                const MonitorView mv{v.N, v.n_states, (int64_t)v.exp_edges, (const int64_t *)v.h_osrc, (const int64_t *)v.h_odst, v.h_oval,
                                     post.p_valid.data(), post.p_final.data(), post.p_alive.data()};
                mon.host.reset(new HostMonitor());
                mon.host->build(mv, mon.observable.data());
            }
            for (size_t i = 0; i < n; i++)
                if (mon.m_acc[i] < 0) {
                    mon.host->check_one(ms->values + ms->offsets[i] * mon.n_obs, ms->offsets[i + 1] - ms->offsets[i], &mon.m_acc[i], &mon.m_nend[i], &mon.m_fin[i]);
                    out->n_host_fallback++;
                }
        }
    }
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Stream generator, build (dev_generate.hpp): the live edges by source in canonical order and the
// weights W_0 .. W_horizon of every state, from the flags the last postprocess() left in HBM.
int AutomatonServices::generator_build(const AutomatonView &view, const stcsp_generator_options *go, stcsp_generator_info *info) {
    if (int rc = enter(view, "generator_build", NEED_FLAGS, "stcsp_automaton_generate")) return rc;
    if (!go || go->horizon < 0) return fail(STCSP_E_INVALID, "generator_build: the horizon must not be negative");
    auto t0 = std::chrono::steady_clock::now();
    gen.built = false;
    gen.drop_derived();
    const int N = v.N, H = go->horizon;
    const uint32_t E = (uint32_t)v.exp_edges, S = v.n_states;
    if ((size_t)v.exp_edges > 0x7fffffffull) return fail(STCSP_E_NOMEM, "edge list too large for the device generator");
    const std::vector<int32_t> obs = observed_columns(go->observable ? go->observable : v.default_observable, N);
    const uint32_t n_tiles = (S + kGenScanTile - 1) / kGenScanTile;
    if (int rc = live_set()) return rc;
    HIPCHK(gen.d_gtile.reserve_exact(grown(S) / kGenScanTile + 2));
    HIPCHK(gen.d_goff.reserve(S, 1));
    HIPCHK(gen.d_gcur.reserve(S));
    HIPCHK(reserve_all(E, 0, gen.d_gseg, gen.d_geid, gen.d_gdst));
    const size_t table = ((size_t)H + 1) * S;
    if (!gen.d_gw.reserve_or_release(table)) return fail(STCSP_E_NOMEM, "generator_build: no room for the %d x %u table of weights", H + 1, S);
    HIPCHK(gen.d_gcount.reserve_exact((size_t)H + 1));
    HIPCHK(gen.d_gobs.reserve_exact((size_t)N));
    HIPCHK(gen.d_gctl.reserve_exact(G_WORDS));
    const unsigned eb = (E + 255) / 256, sb = (S + 255) / 256;
    uint32_t ctl[G_WORDS] = {0}, total = 0;
    if (!obs.empty()) HIPCHK(hipMemcpyAsync(gen.d_gobs.p, obs.data(), obs.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    HIPCHK(hipMemsetAsync(gen.d_gctl.p, 0, sizeof ctl, v.stream));
    // live edges by source: histogram, exclusive scan over the states, fill through a cursor, canonical order
    HIPCHK(hipMemsetAsync(gen.d_gcur.p, 0, (size_t)S * sizeof(uint32_t), v.stream));
    if (E)
        hipLaunchKernelGGL(k_g_degree, dim3(eb), dim3(256), 0, v.stream, E, (const long long *)v.d_osrc, (const long long *)v.d_odst,
                           (const uint8_t *)post.d_palive.p, (const uint8_t *)post.d_live.p, gen.d_gcur.p);
    hipLaunchKernelGGL(k_g_scan_tiles, dim3(n_tiles), dim3(256), 0, v.stream, S, (const uint32_t *)gen.d_gcur.p, gen.d_gtile.p);
    hipLaunchKernelGGL(k_g_scan_sums, dim3(1), dim3(256), 0, v.stream, n_tiles, gen.d_gtile.p);
    hipLaunchKernelGGL(k_g_scan_write, dim3(n_tiles), dim3(256), 0, v.stream, S, (const uint32_t *)gen.d_gcur.p, (const uint32_t *)gen.d_gtile.p, n_tiles,
                       gen.d_goff.p, gen.d_gcur.p);
    if (E) {
        hipLaunchKernelGGL(k_g_fill, dim3(eb), dim3(256), 0, v.stream, E, (const long long *)v.d_osrc, (const long long *)v.d_odst,
                           (const uint8_t *)post.d_palive.p, (const uint8_t *)post.d_live.p, gen.d_gcur.p, gen.d_gseg.p);
        hipLaunchKernelGGL(k_g_order, dim3((S + 3) / 4), dim3(256), 0, v.stream, S, (const uint32_t *)gen.d_goff.p, gen.d_gseg.p, (const long long *)v.d_odst,
                           (const int32_t *)v.d_oval, N, gen.d_geid.p, gen.d_gdst.p, gen.d_gctl.p);
    }
    // the weights, one launch per level
    hipLaunchKernelGGL(k_g_level0, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_live.p, (const uint8_t *)post.d_pfinal.p,
                       (go->flags & STCSP_GEN_END_FINAL) ? 1 : 0, gen.d_gw.p, gen.d_gcount.p);
    for (int t = 0; t < H; t++)
        hipLaunchKernelGGL(k_g_weights, dim3(sb), dim3(256), 0, v.stream, S, (const uint32_t *)gen.d_goff.p, (const uint32_t *)gen.d_gdst.p,
                           (const double *)(gen.d_gw.p + (size_t)t * S), gen.d_gw.p + (size_t)(t + 1) * S, gen.d_gcount.p + t + 1);
    HIPCHK(hipGetLastError());
    gen.count.assign((size_t)H + 1, 0.0);
    HIPCHK(hipMemcpyAsync(gen.count.data(), gen.d_gcount.p, ((size_t)H + 1) * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipMemcpyAsync(&total, gen.d_goff.p + S, sizeof total, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipMemcpyAsync(ctl, gen.d_gctl.p, sizeof ctl, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    for (double c : gen.count)
        if (!std::isfinite(c)) return fail(STCSP_E_UNSUPPORTED, "generator_build: the number of prefixes of length %d overflows a double", H);
    gen.n_obs = (int)obs.size();
    gen.horizon = H;
    gen.built = true;
    memset(info, 0, sizeof *info);
    info->n_states = post.n_live;
    info->n_edges = total;
    info->table_bytes = (int64_t)(table * sizeof(double) + 3 * (size_t)E * sizeof(uint32_t) + (2 * (size_t)S + 1) * sizeof(uint32_t) + S);
    info->count = gen.count.data();
    info->n_observable = gen.n_obs;
    info->horizon = H;
    info->max_out_degree = (int32_t)ctl[G_MAXDEG];
    info->root_live = post.root_live;
    info->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Stream generator, generate: n_streams prefixes of one length, sampled or unranked (contract: stcsp_engine.h).
int AutomatonServices::generate(const AutomatonView &view, const stcsp_generate_request *rq, stcsp_generate_result *out) {
    if (int rc = enter(view, "generate", NEED_GENERATOR, "stcsp_automaton_generate")) return rc;
    if (!generate_request_ok(gen.count, rq->n_streams, rq->len, rq->n_streams > 0 ? rq->ranks : nullptr))
        return fail(STCSP_E_INVALID, "generate: a length outside 0 .. horizon or without a prefix, or a rank that is not below count[len] < 2^53");
    auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)rq->n_streams, len = (size_t)rq->len;
    const size_t cells = n * len * (size_t)gen.n_obs;
    if (n >= 0x7fffffffull) return fail(STCSP_E_NOMEM, "generate: too many streams for one call");
    gen.g_values.assign(cells, 0);
    gen.g_fin.assign(n, 0);
    memset(out, 0, sizeof *out);
    out->n_streams = rq->n_streams;
    out->values = gen.g_values.data();
    out->end_final = gen.g_fin.data();
    out->len = rq->len;
    out->n_observable = gen.n_obs;
    if (n) {  // (count[len] > 0: the root is live)
        HIPCHK(gen.d_gfin.reserve(n));
        HIPCHK(gen.d_gout.reserve(cells));
        if (rq->ranks) HIPCHK(gen.d_granks.reserve(n));
        HIPCHK(ev.ready(2));
        if (rq->ranks) HIPCHK(hipMemcpyAsync(gen.d_granks.p, rq->ranks, n * sizeof(uint64_t), hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipMemsetAsync(gen.d_gctl.p + G_ERROR, 0, sizeof(uint32_t), v.stream));
        HIPCHK(hipEventRecord(ev[0], v.stream));
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        hipLaunchKernelGGL(rq->ranks ? k_g_generate<true> : k_g_generate<false>, grid, block, 0, v.stream, (uint32_t)n, (uint32_t)len,
                           rq->ranks ? 0ull : (unsigned long long)rq->seed, rq->ranks ? (const unsigned long long *)gen.d_granks.p : nullptr, v.n_states,
                           (const double *)gen.d_gw.p, (const uint32_t *)gen.d_goff.p, (const uint32_t *)gen.d_gdst.p, (const uint32_t *)gen.d_geid.p,
                           (const int32_t *)v.d_oval, v.N, (const int32_t *)gen.d_gobs.p, gen.n_obs, (const uint8_t *)post.d_pfinal.p, gen.d_gout.p, gen.d_gfin.p, gen.d_gctl.p);
        HIPCHK(hipEventRecord(ev[1], v.stream));
        HIPCHK(hipGetLastError());
        uint32_t bad = 0;
        if (cells) HIPCHK(hipMemcpyAsync(gen.g_values.data(), gen.d_gout.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(gen.g_fin.data(), gen.d_gfin.p, n, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(&bad, gen.d_gctl.p + G_ERROR, sizeof bad, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        float ms_k = 0;
        HIPCHK(hipEventElapsedTime(&ms_k, ev[0], ev[1]));
        out->seconds_kernel = ms_k * 1e-3;
        if (bad) return fail(STCSP_E_INTERNAL, "generate: a state without an edge of non-zero weight");
    }
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Stream repair, the label ids of the generator's CSR (dev_repair.hpp): built on the first repair() after a generator_build().
int AutomatonServices::repair_labels() {
    const uint32_t S = v.n_states;
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, gen.d_goff.p + S, sizeof total, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    uint32_t slots = 64;
    while (slots < 2 * (size_t)total && slots < 0x80000000u) slots <<= 1;
    HIPCHK(lab.d_rtab.reserve_exact(slots));
    HIPCHK(reserve_all(total, 0, lab.d_rlid, lab.d_rrep));
    HIPCHK(lab.d_rlong.reserve(S));
    HIPCHK(lab.d_rctl.reserve_exact(R_WORDS));
    lab.wave_segment = kRepWaveSegment;
    if (const char *e = getenv("STCSP_REPAIR_WAVE_SEGMENT")) lab.wave_segment = (uint32_t)std::max(1ll, std::min(atoll(e), 0x7fffffffll));
    uint32_t ctl[R_WORDS] = {0};
    HIPCHK(hipMemsetAsync(lab.d_rctl.p, 0, sizeof ctl, v.stream));
    HIPCHK(hipMemsetAsync(lab.d_rtab.p, 0xff, (size_t)slots * sizeof(uint32_t), v.stream));
    if (total) {
        const unsigned kb = (total + 255) / 256;
        hipLaunchKernelGGL(k_r_labels, dim3(kb), dim3(256), 0, v.stream, total, (const uint32_t *)gen.d_geid.p, (const int32_t *)v.d_oval, v.N,
                           (const int32_t *)gen.d_gobs.p, gen.n_obs, lab.d_rtab.p, slots - 1, lab.d_rlid.p, lab.d_rctl.p);
        hipLaunchKernelGGL(k_r_number, dim3((slots + 255) / 256), dim3(256), 0, v.stream, slots, lab.d_rtab.p, lab.d_rrep.p, lab.d_rctl.p);
        hipLaunchKernelGGL(k_r_remap, dim3(kb), dim3(256), 0, v.stream, total, (const uint32_t *)lab.d_rtab.p, lab.d_rlid.p);
    }
    hipLaunchKernelGGL(k_r_long, dim3((S + 255) / 256), dim3(256), 0, v.stream, S, (const uint32_t *)gen.d_goff.p, lab.wave_segment, lab.d_rlong.p, lab.d_rctl.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctl, lab.d_rctl.p, sizeof ctl, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    if (ctl[R_ERROR]) return fail(STCSP_E_INTERNAL, "repair: the label table overflowed");
    lab.total = total;
    lab.n_labels = ctl[R_LABELS];
    lab.n_long = ctl[R_LONG];
    lab.built = true;
    return STCSP_OK;
}

// Stream repair: the nearest solution prefix of every stream (contract: stcsp_engine.h).
int AutomatonServices::repair(const AutomatonView &view, const stcsp_repair_request *rq, stcsp_repair_result *out) {
    if (int rc = enter(view, "repair", NEED_GENERATOR, "stcsp_automaton_repair_streams")) return rc;
    if (!repair_request_ok(rq->n_streams, rq->offsets, rq->weights, gen.n_obs))
        return fail(STCSP_E_INVALID, "repair: malformed stream offsets, a negative weight, or (sum of the weights) x (longest stream) above 2^31 - 2");
    auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)rq->n_streams, n_obs = (size_t)gen.n_obs;
    const size_t steps = n ? (size_t)rq->offsets[n] : 0;
    if (steps && n_obs && !rq->values) return fail(STCSP_E_INVALID, "repair: no step values");
    rep.r_dist.assign(n, -1);
    rep.r_values.assign(steps * n_obs, 0);
    rep.r_fin.assign(n, 0);
    rep.r_nchg.assign(n, 0);
    memset(out, 0, sizeof *out);
    out->n_streams = rq->n_streams;
    out->distance = rep.r_dist.data();
    out->values = rep.r_values.data();
    out->end_final = rep.r_fin.data();
    out->n_changed = rep.r_nchg.data();
    out->n_observable = gen.n_obs;
    const uint32_t S = v.n_states;
    const uint32_t &nL = lab.n_labels;  // a reference: stream_batches() may build the labels, need() and body() read them after that
    const int end_final = (rq->flags & STCSP_REPAIR_END_FINAL) ? 1 : 0;
    const unsigned sb = (S + 255) / 256;
    auto need = [&](size_t len) { return ((len + 1) * (size_t)S + len * (size_t)nL) * sizeof(uint32_t); };
    std::vector<int32_t> w(n_obs, 1);
    if (rq->weights) w.assign(rq->weights, rq->weights + n_obs);
    auto body = [&](const Batch &b, size_t nb, size_t first_step, const BatchStream *streams, const int32_t *rows) -> int {
        const size_t b0 = b.b0, cells = b.steps * n_obs, words_c = b.steps * (size_t)nL, first = first_step * n_obs;
        const SweepCsr csr = sweep_csr();
        const LabelRows L = label_rows();
        if (int rc = reserve_tables("repair", b.bytes, rep.d_rG, b.entries, rep.d_rcost, words_c)) return rc;
        HIPCHK(reserve_all(nb, 0, rep.d_rdist, rep.d_rnchg, rep.d_rfin));
        HIPCHK(rep.d_rout.reserve(cells));
        if (!b0) {
            HIPCHK(rep.d_rweights.reserve_exact(n_obs));
            if (n_obs) HIPCHK(hipMemcpyAsync(rep.d_rweights.p, w.data(), n_obs * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
        }
        if (cells) HIPCHK(hipMemsetAsync(rep.d_rout.p, 0, cells * sizeof(int32_t), v.stream));
        HIPCHK(hipMemsetAsync(lab.d_rctl.p + R_ERROR, 0, sizeof(uint32_t), v.stream));
        HIPCHK(ev.mark(0, v.stream));
        if (words_c)
            hipLaunchKernelGGL(k_r_cost, dim3((nL + 255) / 256, (unsigned)std::min<size_t>(b.steps, 65535)), dim3(256), 0, v.stream, nL,
                               (uint32_t)b.steps, L.rep, L.values, L.N, L.obs, L.n_obs, (const int32_t *)rep.d_rweights.p, rows, rep.d_rcost.p);
        HIPCHK(ev.mark(1, v.stream));
        hipLaunchKernelGGL(k_r_level0, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, streams, (const uint8_t *)post.d_live.p,
                           (const uint8_t *)post.d_pfinal.p, end_final, rep.d_rG.p);
        for (uint32_t r = 1; r <= (uint32_t)b.longest; r++) {
            hipLaunchKernelGGL(k_r_relax, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, r, streams, csr.off, csr.lid, csr.dstp, nL,
                               (const uint32_t *)rep.d_rcost.p, lab.wave_segment, rep.d_rG.p);
            if (lab.n_long)
                hipLaunchKernelGGL(k_r_relax_long, dim3((lab.n_long + 3) / 4, (unsigned)nb), dim3(256), 0, v.stream, lab.n_long,
                                   (const uint32_t *)lab.d_rlong.p, S, r, streams, csr.off, csr.lid, csr.dstp, nL, (const uint32_t *)rep.d_rcost.p,
                                   rep.d_rG.p);
        }
        HIPCHK(ev.mark(2, v.stream));
        hipLaunchKernelGGL(k_r_walk, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)nb, streams, S, (const uint32_t *)rep.d_rG.p,
                           csr.off, csr.lid, csr.dstp, csr.eid, nL, (const uint32_t *)rep.d_rcost.p, L.values, L.N, L.obs, L.n_obs,
                           (const uint8_t *)post.d_pfinal.p, rows, rep.d_rout.p, rep.d_rdist.p, rep.d_rfin.p, rep.d_rnchg.p, lab.d_rctl.p);
        HIPCHK(ev.mark(3, v.stream));
        HIPCHK(hipGetLastError());
        uint32_t bad = 0;
        if (cells) HIPCHK(hipMemcpyAsync(rep.r_values.data() + first, rep.d_rout.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(rep.r_dist.data() + b0, rep.d_rdist.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(rep.r_nchg.data() + b0, rep.d_rnchg.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(rep.r_fin.data() + b0, rep.d_rfin.p, nb, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(&bad, lab.d_rctl.p + R_ERROR, sizeof bad, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        HIPCHK(ev.add_spans(0, {&out->seconds_cost, &out->seconds_relax, &out->seconds_walk}));
        if (bad) return fail(STCSP_E_INTERNAL, "repair: a state with a finite cost to go and no edge that attains it");
        return STCSP_OK;
    };
    if (int rc = stream_batches("repair", "STCSP_REPAIR_BYTES", rq->n_streams, rq->offsets, rq->values, false, need, out, body)) return rc;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Stream alignment: the weighted edit distance of every stream to the solution language and the aligned prefix
// (contract: stcsp_engine.h).
int AutomatonServices::align(const AutomatonView &view, const stcsp_align_request *rq, stcsp_align_result *out) {
    if (int rc = enter(view, "align", NEED_GENERATOR, "stcsp_automaton_align_streams")) return rc;
    if (!align_request_ok(rq->n_streams, rq->offsets, rq->weights, gen.n_obs, rq->skip_cost, rq->gap_cost, v.n_states))
        return fail(STCSP_E_INVALID, "align: malformed stream offsets, a negative weight, a cost below 1, or max(sum of the weights, skip) x (longest "
                                     "stream) + gap x (states) above 2^31 - 2");
    auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)rq->n_streams, n_obs = (size_t)gen.n_obs;
    const size_t steps = n ? (size_t)rq->offsets[n] : 0;
    if (steps && n_obs && !rq->values) return fail(STCSP_E_INVALID, "align: no step values");
    aln.a_dist.assign(n, -1);
    aln.a_fin.assign(n, 0);
    aln.a_nchg.assign(n, 0);
    aln.a_nskip.assign(n, 0);
    aln.a_nins.assign(n, 0);
    aln.a_ooff.assign(n + 1, 0);
    aln.a_poff.assign(n + 1, 0);
    aln.a_values.clear();
    aln.a_ops.clear();
    auto publish = [&] {  // (the two grow batch by batch)
        out->values = aln.a_values.data();
        out->ops = aln.a_ops.data();
    };
    memset(out, 0, sizeof *out);
    out->n_streams = rq->n_streams;
    out->distance = aln.a_dist.data();
    out->out_offsets = aln.a_ooff.data();
    out->op_offsets = aln.a_poff.data();
    out->end_final = aln.a_fin.data();
    out->n_changed = aln.a_nchg.data();
    out->n_skipped = aln.a_nskip.data();
    out->n_inserted = aln.a_nins.data();
    out->n_observable = gen.n_obs;
    publish();
    const uint32_t S = v.n_states;
    const uint32_t &nL = lab.n_labels;  // a reference: stream_batches() may build the labels, need() and body() read them after that
    const int end_final = (rq->flags & STCSP_ALIGN_END_FINAL) ? 1 : 0;
    const uint32_t skip = (uint32_t)rq->skip_cost, gap = (uint32_t)rq->gap_cost;
    const unsigned sb = (S + 255) / 256;
    uint32_t capacity = kAlnFusedStates;
    if (const char *e = getenv("STCSP_ALIGN_FUSED_STATES")) capacity = (uint32_t)std::max(0ll, std::min<long long>(atoll(e), kAlnFusedStates));
    const char *road = getenv("STCSP_ALIGN_FUSED");
    const bool fused = S <= capacity && !(road && strcmp(road, "0") == 0);  // (only "0" forces the general road)
    auto need = [&](size_t len) { return ((len + 1) * (size_t)S + len * (size_t)nL) * sizeof(uint32_t); };
    std::vector<int32_t> w(n_obs, 1);
    if (rq->weights) w.assign(rq->weights, rq->weights + n_obs);
    std::vector<long long> room;
    std::vector<int32_t> rows_h, nrows, nops;
    std::vector<uint8_t> ops_h;
    auto body = [&](const Batch &b, size_t nb, size_t first_step, const BatchStream *streams, const int32_t *rows) -> int {
        (void)first_step;
        const size_t b0 = b.b0, words_c = b.steps * (size_t)nL;
        const SweepCsr csr = sweep_csr();
        const LabelRows L = label_rows();
        if (int rc = reserve_tables("align", b.bytes, aln.d_aG, b.entries, aln.d_acost, words_c)) return rc;
        HIPCHK(reserve_all(nb, 0, aln.d_adist, aln.d_anrows, aln.d_anops, aln.d_anchg, aln.d_anskip, aln.d_anins, aln.d_afin));
        HIPCHK(aln.d_aroom.reserve(nb + 1));
        HIPCHK(aln.d_actl.reserve_exact(A_WORDS));
        if (!aln.h_ctl) HIPCHK(hipHostMalloc((void **)&aln.h_ctl, A_WORDS * sizeof(uint32_t), hipHostMallocDefault));
        if (!b0) {
            HIPCHK(aln.d_aweights.reserve_exact(n_obs));
            if (n_obs) HIPCHK(hipMemcpyAsync(aln.d_aweights.p, w.data(), n_obs * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
        }
        HIPCHK(hipMemsetAsync(aln.d_actl.p, 0, A_WORDS * sizeof(uint32_t), v.stream));
        HIPCHK(ev.mark(0, v.stream));
        if (words_c)
            hipLaunchKernelGGL(k_r_cost, dim3((nL + 255) / 256, (unsigned)std::min<size_t>(b.steps, 65535)), dim3(256), 0, v.stream, nL,
                               (uint32_t)b.steps, L.rep, L.values, L.N, L.obs, L.n_obs, (const int32_t *)aln.d_aweights.p, rows, aln.d_acost.p);
        HIPCHK(ev.mark(1, v.stream));
        const uint8_t *live = post.d_live.p, *fin = post.d_pfinal.p;
        const uint32_t *cost = aln.d_acost.p, *long_states = lab.d_rlong.p;
        if (fused) {
            const size_t lds = 2 * (size_t)S * sizeof(uint32_t);
            if (lds > (64u << 10)) HIPCHK(hipFuncSetAttribute((const void *)k_a_fused, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_a_fused, dim3((unsigned)nb), dim3(kAlnFusedThreads), lds, v.stream, S, streams, csr.off, csr.lid, csr.dstp, nL, cost,
                               lab.wave_segment, lab.n_long, long_states, live, fin, end_final, skip, gap, aln.d_aG.p, aln.d_actl.p);
            out->path_kernel = 1;
        } else {
            // the closure of level r: groups of sweeps until a group stores nothing (a sweep too many changes nothing)
            auto close_level = [&](uint32_t r) -> int {
                for (uint32_t sweeps = 0;; sweeps += kAlnSweepGroup) {
                    HIPCHK(hipMemsetAsync(aln.d_actl.p + A_CHANGED, 0, sizeof(uint32_t), v.stream));
                    for (uint32_t g = 0; g < kAlnSweepGroup; g++) {
                        hipLaunchKernelGGL(k_a_sweep, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, r, streams, csr.off, csr.dstp, lab.wave_segment,
                                           gap, aln.d_aG.p, aln.d_actl.p);
                        if (lab.n_long)
                            hipLaunchKernelGGL(k_a_sweep_long, dim3((lab.n_long + 3) / 4, (unsigned)nb), dim3(256), 0, v.stream, lab.n_long, long_states,
                                               S, r, streams, csr.off, csr.dstp, gap, aln.d_aG.p, aln.d_actl.p);
                    }
                    HIPCHK(hipMemcpyAsync(aln.h_ctl, aln.d_actl.p, A_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
                    HIPCHK(hipStreamSynchronize(v.stream));
                    if (!aln.h_ctl[A_CHANGED]) return STCSP_OK;
                    if (sweeps > S) return fail(STCSP_E_INTERNAL, "align: the closure of a level did not converge");
                }
            };
            hipLaunchKernelGGL(k_r_level0, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, streams, live, fin, end_final, aln.d_aG.p);
            if (end_final)
                if (int rc = close_level(0)) return rc;
            for (uint32_t r = 1; r <= (uint32_t)b.longest; r++) {
                hipLaunchKernelGGL(k_a_base, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, r, streams, csr.off, csr.lid, csr.dstp, nL, cost,
                                   lab.wave_segment, skip, aln.d_aG.p);
                if (lab.n_long)
                    hipLaunchKernelGGL(k_a_base_long, dim3((lab.n_long + 3) / 4, (unsigned)nb), dim3(256), 0, v.stream, lab.n_long, long_states, S, r,
                                       streams, csr.off, csr.lid, csr.dstp, nL, cost, skip, aln.d_aG.p);
                if (int rc = close_level(r)) return rc;
            }
            out->path_kernel = 2;
        }
        hipLaunchKernelGGL(k_a_distance, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)nb, streams, S,
                           (const uint32_t *)aln.d_aG.p, aln.d_adist.p);
        HIPCHK(ev.mark(2, v.stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(aln.a_dist.data() + b0, aln.d_adist.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        // room for len + distance / gap rows and ops per stream
        room.assign(nb + 1, 0);
        for (size_t i = 0; i < nb; i++) {
            const int32_t d = aln.a_dist[b0 + i];
            room[i + 1] = room[i] + (d < 0 ? 0 : (long long)(rq->offsets[b0 + i + 1] - rq->offsets[b0 + i]) + d / rq->gap_cost);
        }
        const size_t cap = (size_t)room[nb];
        HIPCHK(aln.d_aout.reserve(cap * n_obs));
        HIPCHK(aln.d_aops.reserve(cap));
        HIPCHK(hipMemcpyAsync(aln.d_aroom.p, room.data(), (nb + 1) * sizeof(long long), hipMemcpyHostToDevice, v.stream));
        HIPCHK(ev.mark(3, v.stream));
        hipLaunchKernelGGL(k_a_walk, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)nb, streams, S, (const uint32_t *)aln.d_aG.p,
                           csr.off, csr.lid, csr.dstp, csr.eid, nL, cost, L.values, L.N, L.obs, L.n_obs, fin, rows, skip, gap,
                           (const long long *)aln.d_aroom.p, (const int32_t *)aln.d_adist.p, aln.d_aout.p, aln.d_aops.p, aln.d_anrows.p, aln.d_anops.p,
                           aln.d_afin.p, aln.d_anchg.p, aln.d_anskip.p, aln.d_anins.p, aln.d_actl.p);
        HIPCHK(ev.mark(4, v.stream));
        HIPCHK(hipGetLastError());
        rows_h.resize(cap * n_obs);
        ops_h.resize(cap);
        nrows.resize(nb);
        nops.resize(nb);
        if (cap * n_obs) HIPCHK(hipMemcpyAsync(rows_h.data(), aln.d_aout.p, cap * n_obs * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        if (cap) HIPCHK(hipMemcpyAsync(ops_h.data(), aln.d_aops.p, cap, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(nrows.data(), aln.d_anrows.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(nops.data(), aln.d_anops.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(aln.a_nchg.data() + b0, aln.d_anchg.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(aln.a_nskip.data() + b0, aln.d_anskip.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(aln.a_nins.data() + b0, aln.d_anins.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(aln.a_fin.data() + b0, aln.d_afin.p, nb, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(aln.h_ctl, aln.d_actl.p, A_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        HIPCHK(ev.add_spans(0, {&out->seconds_cost, &out->seconds_levels}));
        HIPCHK(ev.add_spans(3, {&out->seconds_walk}));
        if (aln.h_ctl[A_ERROR])
            return fail(STCSP_E_INTERNAL, "align: a state with a finite cost to go and no rule that attains it (error word %u)", aln.h_ctl[A_ERROR]);
        for (size_t i = 0; i < nb; i++) {  // the streams' rows and ops, packed
            const size_t at = (size_t)room[i];
            aln.a_values.insert(aln.a_values.end(), rows_h.begin() + at * n_obs, rows_h.begin() + (at + (size_t)nrows[i]) * n_obs);
            aln.a_ops.insert(aln.a_ops.end(), ops_h.begin() + at, ops_h.begin() + at + (size_t)nops[i]);
            aln.a_ooff[b0 + i + 1] = aln.a_ooff[b0 + i] + nrows[i];
            aln.a_poff[b0 + i + 1] = aln.a_poff[b0 + i] + nops[i];
        }
        return STCSP_OK;
    };
    const int rc = stream_batches("align", "STCSP_ALIGN_BYTES", rq->n_streams, rq->offsets, rq->values, false, need, out, body);
    publish();
    if (rc) return rc;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Stream inference, the value dictionaries (dev_infer.hpp): built on the first infer() after a generator_build(), over
// the label representatives of repair_labels(). Sized by what the labels carry, not by the variables' bounds.
int AutomatonServices::infer_dictionaries() {
    const size_t nL = lab.n_labels, n_obs = (size_t)gen.n_obs, cells = nL * n_obs;
    std::vector<int32_t> rows(cells);
    if (cells) {
        HIPCHK(dict.d_ilabrows.reserve(cells));
        const LabelRows L = label_rows();
        hipLaunchKernelGGL(k_i_rows, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)nL, L.rep, L.values, L.N, L.obs, L.n_obs,
                           dict.d_ilabrows.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rows.data(), dict.d_ilabrows.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
    }
    dict.values.assign(n_obs, std::vector<int32_t>());
    dict.word_off.assign(n_obs, 0);
    dict.bin_off.assign(n_obs, 0);
    std::vector<uint32_t> vidx(cells);
    size_t words = 0;
    dict.n_values = 0;
    for (size_t x = 0; x < n_obs; x++) {
        std::vector<int32_t> &d = dict.values[x];
        d.resize(nL);
        for (size_t l = 0; l < nL; l++) d[l] = rows[l * n_obs + x];
        std::sort(d.begin(), d.end());
        d.erase(std::unique(d.begin(), d.end()), d.end());
        for (size_t l = 0; l < nL; l++) vidx[l * n_obs + x] = (uint32_t)(std::lower_bound(d.begin(), d.end(), rows[l * n_obs + x]) - d.begin());
        dict.word_off[x] = (uint32_t)words;
        words += (d.size() + 31) / 32;
        dict.bin_off[x] = (uint32_t)dict.n_values;
        dict.n_values += d.size();
    }
    if (words > 0x7fffffffull) return fail(STCSP_E_NOMEM, "infer: the support bitmaps of one step are too large");
    dict.words = (uint32_t)words;
    HIPCHK(dict.d_ividx.reserve(cells));
    HIPCHK(dict.d_iwoff.reserve_exact(n_obs));
    if (cells) HIPCHK(hipMemcpyAsync(dict.d_ividx.p, vidx.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
    if (n_obs) HIPCHK(hipMemcpyAsync(dict.d_iwoff.p, dict.word_off.data(), n_obs * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));  // (vidx is a local)
    dict.built = true;
    return STCSP_OK;
}

// Stream inference: supports, counts and draws of partially observed streams (contract: stcsp_engine.h).
int AutomatonServices::infer(const AutomatonView &view, const stcsp_infer_request *rq, stcsp_infer_result *out) {
    if (int rc = enter(view, "infer", NEED_GENERATOR, "stcsp_automaton_infer_streams")) return rc;
    if (!infer_request_ok(rq->n_streams, rq->offsets, rq->draws)) return fail(STCSP_E_INVALID, "infer: malformed stream offsets or a negative number of draws");
    auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)rq->n_streams, n_obs = (size_t)gen.n_obs, draws = (size_t)rq->draws;
    const size_t steps = n ? (size_t)rq->offsets[n] : 0;
    if (steps && n_obs && !rq->values) return fail(STCSP_E_INVALID, "infer: no step values");
    inf.i_count.assign(n, 0.0);
    inf.i_feas.assign(n, 0);
    inf.i_soff.assign(steps * n_obs + 1, 0);
    inf.i_sval.clear();
    inf.i_nstates.assign(steps + n, 0);
    inf.i_values.assign(steps * draws * n_obs, STCSP_INFER_MISSING);
    inf.i_fin.assign(n * draws, 0);
    memset(out, 0, sizeof *out);
    out->n_streams = rq->n_streams;
    out->n_observable = gen.n_obs;
    out->draws = rq->draws;
    auto publish = [&]() {  // (the vectors may have grown)
        out->count = inf.i_count.data();
        out->feasible = inf.i_feas.data();
        out->support_off = inf.i_soff.data();
        out->support_val = inf.i_sval.data();
        out->n_states = inf.i_nstates.data();
        out->values = inf.i_values.data();
        out->end_final = inf.i_fin.data();
    };
    publish();
    const uint32_t S = v.n_states;
    const uint32_t &nL = lab.n_labels, &W = dict.words;  // references: stream_batches() may build both, need() and body() read them after that
    const int end_final = (rq->flags & STCSP_INFER_END_FINAL) ? 1 : 0;
    const unsigned sb = (S + 255) / 256;
    auto need = [&](size_t len) { return (len + 1) * (size_t)S * (sizeof(double) + 1) + len * ((size_t)nL * 2 + (size_t)W * sizeof(uint32_t)); };
    auto body = [&](const Batch &b, size_t nb, size_t first_step, const BatchStream *streams, const int32_t *rows) -> int {
        const size_t b0 = b.b0, cells = b.steps * n_obs, marks = b.steps * (size_t)nL, words = b.steps * (size_t)W;
        const size_t n_q = nb * draws, out_cells = cells * draws, first = first_step * n_obs;
        const SweepCsr csr = sweep_csr();
        const LabelRows L = label_rows();
        if (n_q >= 0x7fffffffull) return fail(STCSP_E_NOMEM, "infer: too many draws for one batch");
        if (int rc = reserve_tables("infer", b.bytes, inf.d_iB, b.entries, inf.d_iF, b.entries, inf.d_imatch, marks, inf.d_ifeas, marks, inf.d_ibits, words)) return rc;
        HIPCHK(inf.d_icount.reserve(nb));
        HIPCHK(inf.d_instates.reserve(b.steps + nb));
        HIPCHK(inf.d_ictl.reserve_exact(I_WORDS));
        if (n_q) {
            HIPCHK(inf.d_ifin.reserve(n_q));
            if (rq->ranks) HIPCHK(inf.d_iranks.reserve(n_q));
            HIPCHK(inf.d_iout.reserve(out_cells));
        }
        HIPCHK(hipMemsetAsync(inf.d_iF.p, 0, b.entries, v.stream));
        if (marks) HIPCHK(hipMemsetAsync(inf.d_ifeas.p, 0, marks, v.stream));
        if (words) HIPCHK(hipMemsetAsync(inf.d_ibits.p, 0, words * sizeof(uint32_t), v.stream));
        HIPCHK(hipMemsetAsync(inf.d_instates.p, 0, (b.steps + nb) * sizeof(int32_t), v.stream));
        HIPCHK(hipMemsetAsync(inf.d_ictl.p, 0, I_WORDS * sizeof(uint32_t), v.stream));
        const unsigned step_rows = (unsigned)std::min<size_t>(std::max<size_t>(b.steps, 1), 65535);
        HIPCHK(ev.mark(0, v.stream));
        if (marks)
            hipLaunchKernelGGL(k_i_match, dim3((nL + 255) / 256, step_rows), dim3(256), 0, v.stream, nL, (uint32_t)b.steps, L.rep, L.values, L.N, L.obs,
                               L.n_obs, rows, inf.d_imatch.p);
        HIPCHK(ev.mark(1, v.stream));
        hipLaunchKernelGGL(k_i_level0, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, streams, (const uint8_t *)post.d_live.p, (const uint8_t *)post.d_pfinal.p,
                           end_final, inf.d_iB.p);
        for (uint32_t r = 1; r <= (uint32_t)b.longest; r++)
            hipLaunchKernelGGL(k_i_backward<false>, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, r, streams, csr.off, csr.lid, csr.dstp, nL,
                               (const uint8_t *)inf.d_imatch.p, inf.d_iB.p);
        hipLaunchKernelGGL(k_i_root, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)nb, streams, S, (const double *)inf.d_iB.p, inf.d_iF.p,
                           inf.d_icount.p);
        HIPCHK(ev.mark(2, v.stream));
        for (uint32_t t = 0; t < (uint32_t)b.longest; t++) {
            hipLaunchKernelGGL(k_i_forward, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, t, streams, csr.off, csr.lid, csr.dstp, nL,
                               (const uint8_t *)inf.d_imatch.p, (const double *)inf.d_iB.p, lab.wave_segment, inf.d_iF.p, inf.d_ifeas.p);
            if (lab.n_long)
                hipLaunchKernelGGL(k_i_forward_long, dim3((lab.n_long + 3) / 4, (unsigned)nb), dim3(256), 0, v.stream, lab.n_long,
                                   (const uint32_t *)lab.d_rlong.p, S, t, streams, csr.off, csr.lid, csr.dstp, nL, (const uint8_t *)inf.d_imatch.p,
                                   (const double *)inf.d_iB.p, inf.d_iF.p, inf.d_ifeas.p);
        }
        hipLaunchKernelGGL(k_i_count, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, streams, (const uint8_t *)inf.d_iF.p, inf.d_instates.p);
        HIPCHK(ev.mark(3, v.stream));
        if (marks && W)
            hipLaunchKernelGGL(k_i_support, dim3((nL + 255) / 256, step_rows), dim3(256), 0, v.stream, nL, (uint32_t)b.steps, (const uint8_t *)inf.d_ifeas.p,
                               (const uint32_t *)dict.d_ividx.p, (const uint32_t *)dict.d_iwoff.p, gen.n_obs, W, inf.d_ibits.p);
        HIPCHK(ev.mark(4, v.stream));
        HIPCHK(hipGetLastError());
        inf.i_bits.resize(words);
        HIPCHK(hipMemcpyAsync(inf.i_count.data() + b0, inf.d_icount.p, nb * sizeof(double), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(inf.i_nstates.data() + first_step + b0, inf.d_instates.p, (b.steps + nb) * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        if (words) HIPCHK(hipMemcpyAsync(inf.i_bits.data(), inf.d_ibits.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        HIPCHK(ev.add_spans(0, {&out->seconds_match, &out->seconds_backward, &out->seconds_forward, &out->seconds_support}));
        // the bitmaps -> sorted lists: bit order is value order
        for (size_t step = 0; step < b.steps; step++)
            for (size_t x = 0; x < n_obs; x++) {
                const uint32_t *w = inf.i_bits.data() + step * W + dict.word_off[x];
                const std::vector<int32_t> &d = dict.values[x];
                for (size_t k = 0; k < d.size(); k++)
                    if (w[k >> 5] >> (k & 31) & 1u) inf.i_sval.push_back(d[k]);
                inf.i_soff[(first_step + step) * n_obs + x + 1] = (int64_t)inf.i_sval.size();
            }
        for (size_t i = b0; i < b.b1; i++) inf.i_feas[i] = inf.i_count[i] > 0.0;
        publish();
        if (!n_q) return STCSP_OK;
        // the draws: the counts decide whether they can be asked for
        for (size_t i = b0; i < b.b1; i++) {
            const int bad = infer_draws_ok(inf.i_count[i], rq->draws, rq->ranks ? rq->ranks + i * draws : nullptr);
            if (bad == 1) return fail(STCSP_E_UNSUPPORTED, "infer: draws from stream %zu, whose count overflows a double", i);
            if (bad) return fail(STCSP_E_INVALID, "infer: stream %zu: a rank that is not below its count < 2^53", i);
        }
        if (rq->ranks) HIPCHK(hipMemcpyAsync(inf.d_iranks.p, rq->ranks + b0 * draws, n_q * sizeof(uint64_t), hipMemcpyHostToDevice, v.stream));
        if (out_cells) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)inf.d_iout.p, STCSP_INFER_MISSING, out_cells, v.stream));
        HIPCHK(hipMemsetAsync(inf.d_ifin.p, 0, n_q, v.stream));
        const dim3 grid((unsigned)((n_q + 255) / 256)), block(256);
        HIPCHK(ev.mark(5, v.stream));
        hipLaunchKernelGGL(rq->ranks ? k_i_walk<true> : k_i_walk<false>, grid, block, 0, v.stream, (uint32_t)n_q, (uint32_t)draws,
                           (unsigned long long)(b0 * draws), rq->ranks ? 0ull : (unsigned long long)rq->seed,
                           rq->ranks ? (const unsigned long long *)inf.d_iranks.p : nullptr, streams, S, (const double *)inf.d_iB.p, csr.off, csr.lid,
                           csr.dstp, csr.eid, nL, (const uint8_t *)inf.d_imatch.p, L.values, L.N, L.obs, L.n_obs, (const uint8_t *)post.d_pfinal.p,
                           inf.d_iout.p, inf.d_ifin.p, inf.d_ictl.p);
        HIPCHK(ev.mark(6, v.stream));
        HIPCHK(hipGetLastError());
        uint32_t bad = 0;
        if (out_cells) HIPCHK(hipMemcpyAsync(inf.i_values.data() + first * draws, inf.d_iout.p, out_cells * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(inf.i_fin.data() + b0 * draws, inf.d_ifin.p, n_q, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(&bad, inf.d_ictl.p + I_ERROR, sizeof bad, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        HIPCHK(ev.add_spans(5, {&out->seconds_walk}));
        if (bad) return fail(STCSP_E_INTERNAL, "infer: a state with weight to go and no matching edge of non-zero weight");
        return STCSP_OK;
    };
    if (int rc = stream_batches("infer", "STCSP_INFER_BYTES", rq->n_streams, rq->offsets, rq->values, true, need, out, body)) return rc;
    if (inf.i_sval.empty()) inf.i_sval.reserve(1);
    publish();
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Posterior marginals of partially observed streams under value weights (contract: stcsp_engine.h).
int AutomatonServices::posterior(const AutomatonView &view, const stcsp_posterior_request *rq, stcsp_posterior_result *out) {
    if (int rc = enter(view, "posterior", NEED_GENERATOR, "stcsp_automaton_posterior_streams")) return rc;
    if (!posterior_request_ok(rq->n_streams, rq->offsets, gen.n_obs, rq->weight_off, rq->weight_val, rq->weight_w))
        return fail(STCSP_E_INVALID, "posterior: malformed stream offsets, or weights that are not a CSR of strictly increasing values and weights >= 0");
    auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)rq->n_streams, n_obs = (size_t)gen.n_obs;
    const size_t steps = n ? (size_t)rq->offsets[n] : 0;
    if (steps && n_obs && !rq->values) return fail(STCSP_E_INVALID, "posterior: no step values");
    pos.y_mass.assign(n, 0.0);
    pos.y_exact.assign(n, 1);
    pos.y_feas.assign(n, 0);
    pos.y_fmass.assign(n, 0);
    pos.y_moff.assign(steps * n_obs + 1, 0);
    pos.y_mval.clear();
    pos.y_mmass.clear();
    memset(out, 0, sizeof *out);
    out->n_streams = rq->n_streams;
    out->n_observable = gen.n_obs;
    const uint32_t S = v.n_states;
    const uint32_t &nL = lab.n_labels;  // references: stream_batches() may build both, need() and body() read them after that
    const size_t &nB = dict.n_values;   // one bin per (variable, dictionary value)
    const int end_final = (rq->flags & STCSP_POSTERIOR_END_FINAL) ? 1 : 0;
    const unsigned sb = (S + 255) / 256;
    const std::vector<uint32_t> &bin_off = dict.bin_off;
    std::vector<double> wbin;
    auto need = [&](size_t len) {
        return (len + 1) * (size_t)S * sizeof(double) + 2 * (size_t)S * sizeof(uint64_t) + len * ((size_t)nL * (1 + sizeof(uint64_t)) + (size_t)nB * sizeof(uint64_t));
    };
    auto body = [&](const Batch &b, size_t nb, size_t first_step, const BatchStream *streams, const int32_t *rows) -> int {
        const size_t b0 = b.b0, marks = b.steps * (size_t)nL, bins = b.steps * (size_t)nB, rows_a = nb * 2 * (size_t)S;
        const SweepCsr csr = sweep_csr();
        const LabelRows L = label_rows();
        if (!b0) {  // the weight of every bin, and of every label
            if (nB > 0x7fffffffull) return fail(STCSP_E_NOMEM, "posterior: the bins of one step are too many");
            for (size_t x = 0; x < n_obs; x++)
                for (int32_t value : dict.values[x]) wbin.push_back(posterior_value_weight((int)x, value, rq->weight_off, rq->weight_val, rq->weight_w));
            HIPCHK(pos.d_yw.reserve(nL));
            HIPCHK(pos.d_ywbin.reserve(nB));
            HIPCHK(pos.d_yboff.reserve_exact(n_obs));
            if (nB) HIPCHK(hipMemcpyAsync(pos.d_ywbin.p, wbin.data(), nB * sizeof(double), hipMemcpyHostToDevice, v.stream));
            if (n_obs) HIPCHK(hipMemcpyAsync(pos.d_yboff.p, bin_off.data(), n_obs * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
            HIPCHK(ev.mark(5, v.stream));
            if (nL)
                hipLaunchKernelGGL(k_p_label_weight, dim3((nL + 255) / 256), dim3(256), 0, v.stream, nL, (const uint32_t *)dict.d_ividx.p,
                                   (const uint32_t *)pos.d_yboff.p, gen.n_obs, (const double *)pos.d_ywbin.p, pos.d_yw.p);
            HIPCHK(ev.mark(6, v.stream));
            HIPCHK(hipGetLastError());
        }
        if (int rc = reserve_tables("posterior", b.bytes, pos.d_yB, b.entries, pos.d_yA, rows_a, pos.d_ymatch, marks, pos.d_ylab, marks, pos.d_ybins, bins)) return rc;
        HIPCHK(reserve_all(nb, 0, pos.d_ymass, pos.d_yexact, pos.d_yfmass));
        HIPCHK(hipMemsetAsync(pos.d_yA.p, 0, rows_a * sizeof(uint64_t), v.stream));
        HIPCHK(hipMemsetAsync(pos.d_yfmass.p, 0, nb * sizeof(uint64_t), v.stream));
        if (marks) HIPCHK(hipMemsetAsync(pos.d_ylab.p, 0, marks * sizeof(uint64_t), v.stream));
        if (bins) HIPCHK(hipMemsetAsync(pos.d_ybins.p, 0, bins * sizeof(uint64_t), v.stream));
        const unsigned step_rows = (unsigned)std::min<size_t>(std::max<size_t>(b.steps, 1), 65535);
        HIPCHK(ev.mark(0, v.stream));
        if (marks)
            hipLaunchKernelGGL(k_i_match, dim3((nL + 255) / 256, step_rows), dim3(256), 0, v.stream, nL, (uint32_t)b.steps, L.rep, L.values, L.N, L.obs,
                               L.n_obs, rows, pos.d_ymatch.p);
        HIPCHK(ev.mark(1, v.stream));
        hipLaunchKernelGGL(k_i_level0, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, streams, (const uint8_t *)post.d_live.p, (const uint8_t *)post.d_pfinal.p,
                           end_final, pos.d_yB.p);
        for (uint32_t r = 1; r <= (uint32_t)b.longest; r++)
            hipLaunchKernelGGL((k_i_backward<true, const double *>), dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, r, streams, csr.off, csr.lid, csr.dstp, nL,
                               (const uint8_t *)pos.d_ymatch.p, (const double *)pos.d_yw.p, pos.d_yB.p);
        hipLaunchKernelGGL(k_p_root, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)nb, streams, S, (const double *)pos.d_yB.p, pos.d_yA.p,
                           pos.d_ymass.p, pos.d_yexact.p);
        HIPCHK(ev.mark(2, v.stream));
        for (uint32_t t = 0; t < (uint32_t)b.longest; t++) {
            if (lab.n_long)  // before k_p_forward, which clears A_t
                hipLaunchKernelGGL(k_p_forward_long, dim3((lab.n_long + 3) / 4, (unsigned)nb), dim3(256), 0, v.stream, lab.n_long,
                                   (const uint32_t *)lab.d_rlong.p, S, t, streams, csr.off, csr.lid, csr.dstp, nL, (const uint8_t *)pos.d_ymatch.p,
                                   (const double *)pos.d_yw.p, (const double *)pos.d_yB.p, pos.d_yA.p, pos.d_ylab.p);
            hipLaunchKernelGGL(k_p_forward, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, t, streams, csr.off, csr.lid, csr.dstp, nL,
                               (const uint8_t *)pos.d_ymatch.p, (const double *)pos.d_yw.p, (const double *)pos.d_yB.p, lab.wave_segment, pos.d_yA.p,
                               pos.d_ylab.p);
        }
        hipLaunchKernelGGL(k_p_final, dim3(sb, (unsigned)nb), dim3(256), 0, v.stream, S, streams, (const uint8_t *)post.d_pfinal.p,
                           (const unsigned long long *)pos.d_yA.p, pos.d_yfmass.p);
        HIPCHK(ev.mark(3, v.stream));
        if (marks && nB)
            hipLaunchKernelGGL(k_p_bins, dim3((nL + 255) / 256, step_rows), dim3(256), 0, v.stream, nL, (uint32_t)b.steps,
                               (const unsigned long long *)pos.d_ylab.p, (const uint32_t *)dict.d_ividx.p, (const uint32_t *)pos.d_yboff.p, gen.n_obs, (uint32_t)nB, pos.d_ybins.p);
        HIPCHK(ev.mark(4, v.stream));
        HIPCHK(hipGetLastError());
        pos.y_bins.resize(bins);
        HIPCHK(hipMemcpyAsync(pos.y_mass.data() + b0, pos.d_ymass.p, nb * sizeof(double), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(pos.y_exact.data() + b0, pos.d_yexact.p, nb, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(pos.y_fmass.data() + b0, pos.d_yfmass.p, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, v.stream));
        if (bins) HIPCHK(hipMemcpyAsync(pos.y_bins.data(), pos.d_ybins.p, bins * sizeof(uint64_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        // seconds_weights = match + label weights, the latter once
        HIPCHK(ev.add_spans(0, {&out->seconds_weights, &out->seconds_backward, &out->seconds_forward, &out->seconds_bins}));
        if (!b0) HIPCHK(ev.add_spans(5, {&out->seconds_weights}));
        // the bins -> sorted lists: dictionary order is value order
        for (size_t step = 0; step < b.steps; step++)
            for (size_t x = 0; x < n_obs; x++) {
                const unsigned long long *row = pos.y_bins.data() + step * nB + bin_off[x];
                const std::vector<int32_t> &d = dict.values[x];
                for (size_t k = 0; k < d.size(); k++)
                    if (row[k]) {
                        pos.y_mval.push_back(d[k]);
                        pos.y_mmass.push_back((uint64_t)row[k]);
                    }
                pos.y_moff[(first_step + step) * n_obs + x + 1] = (int64_t)pos.y_mval.size();
            }
        return STCSP_OK;
    };
    if (int rc = stream_batches("posterior", "STCSP_POSTERIOR_BYTES", rq->n_streams, rq->offsets, rq->values, true, need, out, body)) return rc;
    for (size_t i = 0; i < n; i++) pos.y_feas[i] = pos.y_mass[i] > 0.0;
    if (pos.y_mval.empty()) {
        pos.y_mval.reserve(1);
        pos.y_mmass.reserve(1);
    }
    out->mass = pos.y_mass.data();
    out->exact = pos.y_exact.data();
    out->feasible = pos.y_feas.data();
    out->final_mass = pos.y_fmass.data();
    out->marg_off = pos.y_moff.data();
    out->marg_val = pos.y_mval.data();
    out->marg_mass = pos.y_mmass.data();
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// A buffer that has to grow in the middle of a construction: the first `keep` elements move to the larger one.
template <typename T>
int AutomatonServices::grow_keeping(DevBuf<T> &buf, size_t keep, size_t count, const char *who) {
    if (buf.n >= count) return STCSP_OK;
    DevBuf<T> bigger;
    const size_t room = std::max(grown(count), 2 * buf.n);
    if (bigger.alloc(room) != hipSuccess) {
        (void)hipGetLastError();
        return fail(STCSP_E_NOMEM, "%s: no room for %zu bytes on the device", who, room * sizeof(T));
    }
    if (keep) HIPCHK(hipMemcpyAsync(bigger.p, buf.p, keep * sizeof(T), hipMemcpyDeviceToDevice, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    std::swap(buf.p, bigger.p);
    std::swap(buf.n, bigger.n);
    return STCSP_OK;
}

// Observer, the ordered out-edges (dev_observer.hpp): built on the first observer() after a generator_build(), over the label
// ids of repair_labels(). The host sorts the n_labels projected rows; their ranks are the labels of the construction.
int AutomatonServices::observer_order(double &seconds) {
    const uint32_t S = v.n_states, nL = lab.n_labels;
    const size_t n_obs = (size_t)gen.n_obs, cells = (size_t)nL * n_obs;
    std::vector<int32_t> rows(cells);
    if (cells) {
        HIPCHK(dict.d_ilabrows.reserve(cells));
        const LabelRows L = label_rows();
        hipLaunchKernelGGL(k_i_rows, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, v.stream, nL, L.rep, L.values, L.N, L.obs, L.n_obs,
                           dict.d_ilabrows.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rows.data(), dict.d_ilabrows.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
    }
    std::vector<uint32_t> order(nL), lrank(nL);
    for (uint32_t l = 0; l < nL; l++) order[l] = l;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return std::lexicographical_compare(rows.begin() + a * n_obs, rows.begin() + (a + 1) * n_obs, rows.begin() + b * n_obs, rows.begin() + (b + 1) * n_obs);
    });
    obsv.rows.resize(cells);
    for (uint32_t r = 0; r < nL; r++) {
        lrank[order[r]] = r;
        std::copy(rows.begin() + order[r] * n_obs, rows.begin() + (order[r] + 1) * n_obs, obsv.rows.begin() + r * n_obs);
    }
    HIPCHK(obsv.d_olrank.reserve(nL));
    HIPCHK(obsv.d_okey.reserve(lab.total));
    HIPCHK(obsv.d_octl.reserve_exact(O_WORDS));
    HIPCHK(ev.ready(2));
    uint32_t ctl[O_WORDS] = {0};
    HIPCHK(hipMemsetAsync(obsv.d_octl.p, 0, sizeof ctl, v.stream));
    if (nL) HIPCHK(hipMemcpyAsync(obsv.d_olrank.p, lrank.data(), nL * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
    HIPCHK(hipEventRecord(ev[0], v.stream));
    if (lab.total)
        hipLaunchKernelGGL(k_o_order, dim3((S + 3) / 4), dim3(256), 0, v.stream, S, (const uint32_t *)gen.d_goff.p, (const uint32_t *)lab.d_rlid.p,
                           (const uint32_t *)gen.d_gdst.p, (const uint32_t *)obsv.d_olrank.p, obsv.d_okey.p, obsv.d_octl.p);
    HIPCHK(hipEventRecord(ev[1], v.stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctl, obsv.d_octl.p, sizeof ctl, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));  // (lrank is a local)
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    seconds = ms * 1e-3;
    obsv.max_deg = ctl[O_MAXDEG];
    obsv.built = true;
    return STCSP_OK;
}

// Observer: the subset construction of the live automaton under the generator's mask (contract: stcsp_engine.h).
int AutomatonServices::observer(const AutomatonView &view, const stcsp_observer_options *oo, stcsp_observer_result *out) {
    if (int rc = enter(view, "observer", NEED_GENERATOR, "stcsp_automaton_observer")) return rc;
    cmp.valid = false;  // (the left operand of compare() is the observer of the last call that succeeded)
    if (oo && oo->max_states < 0) return fail(STCSP_E_INVALID, "observer: max_states must not be negative");
    auto t0 = std::chrono::steady_clock::now();
    const unsigned long long max_states = std::min<unsigned long long>(oo && oo->max_states ? (unsigned long long)oo->max_states : 1ull << 26, 0x7ffffffeull);
    const size_t n_obs = (size_t)gen.n_obs;
    obsv.o_moff.assign(1, 0);
    obsv.o_member.clear();
    obsv.o_final.clear();
    obsv.o_esrc.clear();
    obsv.o_edst.clear();
    obsv.o_evalues.clear();
    memset(out, 0, sizeof *out);
    out->n_observable = gen.n_obs;
    auto publish = [&]() {  // (empty vectors still give valid pointers)
        obsv.o_member.reserve(1);
        obsv.o_final.reserve(1);
        obsv.o_esrc.reserve(1);
        obsv.o_edst.reserve(1);
        obsv.o_evalues.reserve(1);
        out->member_off = obsv.o_moff.data();
        out->member = obsv.o_member.data();
        out->state_final = obsv.o_final.data();
        out->edge_src = obsv.o_esrc.data();
        out->edge_dst = obsv.o_edst.data();
        out->edge_values = obsv.o_evalues.data();
        out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    if (!post.root_live) {
        cmp.left.clear();
        cmp.left.n_obs = gen.n_obs;
        cmp.valid = true;
        cmp.left_on_device = false;
        publish();
        return STCSP_OK;
    }
    if (int rc = lab.built ? STCSP_OK : repair_labels()) return rc;
    if (int rc = obsv.built ? STCSP_OK : observer_order(out->seconds_build)) return rc;
    size_t budget = 0;
    if (int rc = table_budget("STCSP_OBSERVER_BYTES", budget)) return rc;
    const char *force = getenv("STCSP_OBSERVER_GLOBAL_SCRATCH");
    const uint32_t S = v.n_states, W = (S + 31) / 32, nL = lab.n_labels;
    const bool global_bits = W > kObsLdsWords || (force && atoi(force) != 0);
    auto pow2 = [](unsigned long long n) {
        unsigned long long c = 1024;
        while (c < n) c <<= 1;
        return c;
    };
    HIPCHK(ev.ready(6));
    // the root's set
    unsigned long long cap_s = 1024, pool_top = 1, scratch_peak = 0;
    uint32_t n_states = 1, e_total = 0;
    HIPCHK(obsv.d_ostab.reserve_exact(cap_s));
    HIPCHK(obsv.d_ossid.reserve_exact(cap_s));
    HIPCHK(obsv.d_orec.reserve(1));
    HIPCHK(obsv.d_opool.reserve(1));
    uint32_t ctl[O_WORDS] = {0};
    HIPCHK(hipMemsetAsync(obsv.d_octl.p, 0, sizeof ctl, v.stream));
    HIPCHK(hipMemsetAsync(obsv.d_ostab.p, 0xff, cap_s * sizeof(unsigned long long), v.stream));
    hipLaunchKernelGGL(k_o_init, dim3(1), dim3(64), 0, v.stream, (const uint8_t *)post.d_pfinal.p, obsv.d_orec.p, obsv.d_opool.p, obsv.d_ostab.p, obsv.d_ossid.p, (uint32_t)(cap_s - 1),
                       obsv.d_octl.p);
    auto read_ctl = [&]() -> int {
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ctl, obsv.d_octl.p, sizeof ctl, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        if (ctl[O_ERROR] & (O_ERR_TABLE_FULL | O_ERR_ITEMS_FULL)) return fail(STCSP_E_INTERNAL, "observer: a device table overflowed (flags %u)", ctl[O_ERROR]);
        if (ctl[O_ERROR]) return fail(STCSP_E_INTERNAL, "observer: two distinct sets of states share a hash (collision)");
        return STCSP_OK;
    };
    bool commit_pending = false;
    auto take_commit_time = [&]() -> int {
        float ms = 0;
        if (commit_pending) HIPCHK(hipEventElapsedTime(&ms, ev[4], ev[5]));
        out->seconds_commit += ms * 1e-3;
        commit_pending = false;
        return STCSP_OK;
    };
    auto succ = [&](int mode, uint32_t n_items, uint32_t c0, uint32_t grid, uint32_t e_base) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, v.stream, n_items, c0, (const unsigned long long *)obsv.d_oitems.p, obsv.d_orec.p, obsv.d_opool.p,
                               (const uint32_t *)gen.d_goff.p, (const unsigned long long *)obsv.d_okey.p, (const uint8_t *)post.d_pfinal.p, W, obsv.d_oscratch.p, obsv.d_ostab.p,
                               obsv.d_ossid.p, (uint32_t)(cap_s - 1), obsv.d_oslot.p, e_base, obsv.d_oesrc.p, obsv.d_oelab.p, obsv.d_oedst.p, obsv.d_octl.p);
        };
        if (global_bits)
            mode == O_INTERN ? go(k_o_succ<true, O_INTERN>) : mode == O_WRITE ? go(k_o_succ<true, O_WRITE>) : go(k_o_succ<true, O_VERIFY>);
        else
            mode == O_INTERN ? go(k_o_succ<false, O_INTERN>) : mode == O_WRITE ? go(k_o_succ<false, O_WRITE>) : go(k_o_succ<false, O_VERIFY>);
    };
    struct Level { uint32_t e0, e1, s0, s1; };  // the edges logged at a level, the states new there
    std::vector<Level> levels;
    unsigned long long level_members = 1;
    for (uint32_t f0 = 0, f1 = 1; f0 < f1;) {
        const uint32_t e_begin = e_total;
        const unsigned long long pool_begin = pool_top;
        const int level = (int)levels.size();
        for (uint32_t c0 = f0; c0 < f1;) {
            // the chunk: as many frontier sets as their possible items (a set has at most n_labels, a member at most max_deg) leave in the budget
            auto bound_of = [&](unsigned long long sets) {
                return std::max<unsigned long long>(1, std::min<unsigned long long>(sets * nL, level_members * obsv.max_deg));
            };
            auto bytes_of = [&](unsigned long long items) { return pow2(2 * items) * sizeof(unsigned long long) + items * (sizeof(unsigned long long) + sizeof(uint32_t)); };
            unsigned long long chunk = f1 - c0;
            while (chunk > 1 && (bytes_of(bound_of(chunk)) > budget || bound_of(chunk) > 0x3fffffffull)) chunk = (chunk + 1) / 2;
            const unsigned long long bound = bound_of(chunk);
            if (bytes_of(bound) > budget || bound > 0x3fffffffull)
                return fail(STCSP_E_NOMEM, "observer: the %llu possible work items of one set need %llu bytes, the budget (STCSP_OBSERVER_BYTES) is %zu; the construction got to level %d with %u states and %u edges",
                            bound, bytes_of(bound), budget, level, n_states, e_total);
            const uint32_t c1 = c0 + (uint32_t)chunk;
            const unsigned long long cap_i = pow2(2 * bound);
            scratch_peak = std::max(scratch_peak, bytes_of(bound));
            if (!obsv.d_oitab.reserve_or_release(cap_i) || !obsv.d_oitems.reserve_or_release(bound))
                return fail(STCSP_E_NOMEM, "observer: no room for %llu bytes of work items at level %d (%u states so far)", bytes_of(bound), level, n_states);
            HIPCHK(hipMemsetAsync(obsv.d_oitab.p, 0xff, cap_i * sizeof(unsigned long long), v.stream));
            HIPCHK(hipMemsetAsync(obsv.d_octl.p + O_ITEMS, 0, sizeof(uint32_t), v.stream));
            HIPCHK(hipEventRecord(ev[0], v.stream));
            hipLaunchKernelGGL(k_o_items, dim3((unsigned)std::min<unsigned long long>(chunk, 4096)), dim3(256), 0, v.stream, c0, c1, (const ObsRec *)obsv.d_orec.p,
                               (const uint32_t *)obsv.d_opool.p, (const uint32_t *)gen.d_goff.p, (const unsigned long long *)obsv.d_okey.p, obsv.d_oitab.p, (uint32_t)(cap_i - 1),
                               obsv.d_oitems.p, (uint32_t)bound, obsv.d_octl.p);
            HIPCHK(hipEventRecord(ev[1], v.stream));
            if (int rc = read_ctl()) return rc;
            if (int rc = take_commit_time()) return rc;
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
            out->seconds_items += ms * 1e-3;
            const uint32_t n_items = ctl[O_ITEMS];
            c0 = c1;
            if (!n_items) continue;
            if ((unsigned long long)e_total + n_items > 0x7fffffffull)
                return fail(STCSP_E_NOMEM, "observer: more than 2^31 - 1 edges (level %d, %u states so far)", level, n_states);
            // room for what the items may add: slots, records, edges
            if (cap_s < 2ull * ((unsigned long long)n_states + n_items)) {
                const unsigned long long old = cap_s;
                cap_s = pow2(2ull * ((unsigned long long)n_states + n_items));
                if (cap_s > 0x80000000ull || !obsv.d_ostab2.reserve_or_release(cap_s) || !obsv.d_ossid2.reserve_or_release(cap_s))
                    return fail(STCSP_E_NOMEM, "observer: no room for a table of %llu slots at level %d (%u states so far)", cap_s, level, n_states);
                HIPCHK(hipMemsetAsync(obsv.d_ostab2.p, 0xff, cap_s * sizeof(unsigned long long), v.stream));
                hipLaunchKernelGGL(k_o_rehash, dim3((unsigned)(old / 256)), dim3(256), 0, v.stream, (uint32_t)old, (const unsigned long long *)obsv.d_ostab.p,
                                   (const uint32_t *)obsv.d_ossid.p, obsv.d_ostab2.p, obsv.d_ossid2.p, (uint32_t)(cap_s - 1), obsv.d_octl.p);
                HIPCHK(hipStreamSynchronize(v.stream));
                std::swap(obsv.d_ostab.p, obsv.d_ostab2.p);
                std::swap(obsv.d_ostab.n, obsv.d_ostab2.n);
                std::swap(obsv.d_ossid.p, obsv.d_ossid2.p);
                std::swap(obsv.d_ossid.n, obsv.d_ossid2.n);
            }
            if (int rc = grow_keeping(obsv.d_orec, n_states, (size_t)n_states + n_items)) return rc;
            if (int rc = grow_keeping(obsv.d_oesrc, e_total, (size_t)e_total + n_items)) return rc;
            if (int rc = grow_keeping(obsv.d_oelab, e_total, (size_t)e_total + n_items)) return rc;
            if (int rc = grow_keeping(obsv.d_oedst, e_total, (size_t)e_total + n_items)) return rc;
            HIPCHK(obsv.d_oslot.reserve(n_items));
            uint32_t grid = std::min<uint32_t>(n_items, 2048);
            if (global_bits) {  // a slice of W words per workgroup
                grid = (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>(std::min<uint32_t>(n_items, 1024), budget / ((size_t)W * sizeof(uint32_t))));
                scratch_peak = std::max(scratch_peak, bytes_of(bound) + (unsigned long long)grid * W * sizeof(uint32_t));
                if (!obsv.d_oscratch.reserve_or_release((size_t)grid * W))
                    return fail(STCSP_E_NOMEM, "observer: no room for %zu bytes of bitsets at level %d (%u states so far)", (size_t)grid * W * sizeof(uint32_t), level, n_states);
            }
            HIPCHK(hipEventRecord(ev[2], v.stream));
            succ(O_INTERN, n_items, c1 - (uint32_t)chunk, grid, e_total);
            HIPCHK(hipEventRecord(ev[3], v.stream));
            if (int rc = read_ctl()) return rc;
            HIPCHK(hipEventElapsedTime(&ms, ev[2], ev[3]));
            out->seconds_intern += ms * 1e-3;
            const unsigned long long pool_now = (unsigned long long)ctl[O_POOL] | ((unsigned long long)ctl[O_POOL + 1] << 32);
            // both limits are checked here, before a list is written
            if (ctl[O_STATES] > max_states)
                return fail(STCSP_E_NOMEM, "observer: more than max_states = %llu states; the construction got to level %d with %u states and %u edges", max_states,
                            level, n_states, e_total);
            if (pool_now * sizeof(uint32_t) > budget)
                return fail(STCSP_E_NOMEM, "observer: the member lists need more than the budget of %zu bytes (STCSP_OBSERVER_BYTES); the construction got to level %d with %u states, %llu members and %u edges",
                            budget, level, n_states, pool_top, e_total);
            if (int rc = grow_keeping(obsv.d_opool, (size_t)pool_top, (size_t)pool_now)) return rc;
            HIPCHK(hipEventRecord(ev[4], v.stream));
            succ(O_WRITE, n_items, c1 - (uint32_t)chunk, grid, e_total);
            succ(O_VERIFY, n_items, c1 - (uint32_t)chunk, grid, e_total);
            HIPCHK(hipEventRecord(ev[5], v.stream));
            commit_pending = true;
            n_states = ctl[O_STATES];
            pool_top = pool_now;
            e_total += n_items;
        }
        levels.push_back(Level{e_begin, e_total, f1, n_states});
        level_members = pool_top - pool_begin;
        f0 = f1;
        f1 = n_states;
    }
    if (int rc = read_ctl()) return rc;  // (the last verify)
    if (int rc = take_commit_time()) return rc;
    // canonical numbers, level by level: a new state's key is the least (number of a parent, label rank) over the edges of the level
    std::vector<uint32_t> canon(n_states, 0), idx;
    std::vector<unsigned long long> keys;
    HIPCHK(obsv.d_ocanon.reserve(n_states));
    HIPCHK(obsv.d_okeys.reserve(n_states));
    HIPCHK(hipMemsetAsync(obsv.d_okeys.p, 0xff, (size_t)n_states * sizeof(unsigned long long), v.stream));
    HIPCHK(hipMemsetAsync(obsv.d_ocanon.p, 0, sizeof(uint32_t), v.stream));
    uint32_t next = 1;
    for (const Level &lv : levels) {
        const uint32_t n_new = lv.s1 - lv.s0;
        if (!n_new) continue;
        hipLaunchKernelGGL(k_o_keys, dim3((lv.e1 - lv.e0 + 255) / 256), dim3(256), 0, v.stream, lv.e0, lv.e1, (const uint32_t *)obsv.d_oesrc.p,
                           (const uint32_t *)obsv.d_oelab.p, (const uint32_t *)obsv.d_oedst.p, lv.s0, (const uint32_t *)obsv.d_ocanon.p, obsv.d_okeys.p);
        HIPCHK(hipGetLastError());
        keys.resize(n_new);
        HIPCHK(hipMemcpyAsync(keys.data(), obsv.d_okeys.p + lv.s0, (size_t)n_new * sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        idx.resize(n_new);
        for (uint32_t i = 0; i < n_new; i++) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
        for (uint32_t i = 0; i < n_new; i++) canon[lv.s0 + idx[i]] = next++;
        HIPCHK(hipMemcpyAsync(obsv.d_ocanon.p + lv.s0, canon.data() + lv.s0, (size_t)n_new * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
    }
    // the result: records, members in canonical order, edges sorted by (source number, label rank)
    std::vector<ObsRec> rec(n_states);
    std::vector<unsigned long long> where(n_states);
    HIPCHK(hipMemcpyAsync(rec.data(), obsv.d_orec.p, (size_t)n_states * sizeof(ObsRec), hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    obsv.o_moff.assign((size_t)n_states + 1, 0);
    obsv.o_final.assign(n_states, 0);
    int64_t max_set = 0;
    for (uint32_t s = 0; s < n_states; s++) {
        obsv.o_moff[canon[s] + 1] = rec[s].n;
        obsv.o_final[canon[s]] = (uint8_t)rec[s].fin;
        max_set = std::max<int64_t>(max_set, rec[s].n);
    }
    for (uint32_t c = 0; c < n_states; c++) obsv.o_moff[c + 1] += obsv.o_moff[c];
    for (uint32_t s = 0; s < n_states; s++) where[s] = (unsigned long long)obsv.o_moff[canon[s]];
    if ((unsigned long long)obsv.o_moff[n_states] != pool_top) return fail(STCSP_E_INTERNAL, "observer: the records name %lld members, the pool holds %llu", (long long)obsv.o_moff[n_states], pool_top);
    HIPCHK(obsv.d_owhere.reserve(n_states));
    HIPCHK(obsv.d_omember.reserve((size_t)pool_top));
    HIPCHK(hipMemcpyAsync(obsv.d_owhere.p, where.data(), (size_t)n_states * sizeof(unsigned long long), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(k_o_gather, dim3(std::min<uint32_t>(n_states, 4096)), dim3(256), 0, v.stream, n_states, (const ObsRec *)obsv.d_orec.p,
                       (const unsigned long long *)obsv.d_owhere.p, (const uint32_t *)obsv.d_opool.p, obsv.d_omember.p);
    if (e_total)
        hipLaunchKernelGGL(k_o_renumber, dim3((e_total + 255) / 256), dim3(256), 0, v.stream, e_total, obsv.d_oesrc.p, obsv.d_oedst.p, (const uint32_t *)obsv.d_ocanon.p);
    HIPCHK(hipGetLastError());
    obsv.o_member.resize((size_t)pool_top);
    std::vector<uint32_t> esrc(e_total), elab(e_total), edst(e_total);
    HIPCHK(hipMemcpyAsync(obsv.o_member.data(), obsv.d_omember.p, (size_t)pool_top * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
    if (e_total) {
        HIPCHK(hipMemcpyAsync(esrc.data(), obsv.d_oesrc.p, (size_t)e_total * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(elab.data(), obsv.d_oelab.p, (size_t)e_total * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(edst.data(), obsv.d_oedst.p, (size_t)e_total * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
    }
    HIPCHK(hipStreamSynchronize(v.stream));
    idx.resize(e_total);
    for (uint32_t e = 0; e < e_total; e++) idx[e] = e;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return esrc[a] != esrc[b] ? esrc[a] < esrc[b] : elab[a] < elab[b]; });
    obsv.o_esrc.resize(e_total);
    obsv.o_edst.resize(e_total);
    obsv.o_evalues.resize((size_t)e_total * n_obs);
    for (uint32_t i = 0; i < e_total; i++) {
        const uint32_t e = idx[i];
        obsv.o_esrc[i] = (int32_t)esrc[e];
        obsv.o_edst[i] = (int32_t)edst[e];
        std::copy(obsv.rows.begin() + elab[e] * n_obs, obsv.rows.begin() + (elab[e] + 1) * n_obs, obsv.o_evalues.begin() + i * n_obs);
    }
    cmp.left.set_graph(gen.n_obs, n_states, obsv.o_final.data(), e_total, [&](size_t i) { return obsv.o_esrc[i]; }, [&](size_t i) { return elab[idx[i]]; },
                       [&](size_t i) { return obsv.o_edst[i]; });
    cmp.left.rows = obsv.rows;
    cmp.left.n_rows = nL;
    cmp.valid = true;
    cmp.left_on_device = false;
    out->n_states = n_states;
    out->n_edges = e_total;
    out->n_labels = nL;
    out->max_set = max_set;
    out->levels = (int32_t)levels.size();
    out->table_bytes = (int64_t)(pool_top * sizeof(uint32_t) + (size_t)n_states * sizeof(ObsRec) + cap_s * (sizeof(unsigned long long) + sizeof(uint32_t)) +
                                 (size_t)e_total * 3 * sizeof(uint32_t) + scratch_peak + (size_t)lab.total * sizeof(unsigned long long));
    publish();
    return STCSP_OK;
}

// Comparison: the synchronous product of the last observer (left) and the request's automaton (right), its four inclusions and their
// witnesses (contract: stcsp_engine.h; dev_compare.hpp).
int AutomatonServices::compare(const AutomatonView &view, const stcsp_compare_request *rq, stcsp_compare_result *out) {
    if (int rc = enter(view, "compare", NEED_GENERATOR, "stcsp_compare_observers")) return rc;
    if (!cmp.valid) return fail(STCSP_E_STATE, "compare needs a successful observer() after the last generator_build()");
    if (!rq->right || rq->max_pairs < 0) return fail(STCSP_E_INVALID, "compare: no right operand, or a negative max_pairs");
    if (const char *fault = compare_operand_fault(*rq->right)) return fail(STCSP_E_INVALID, "compare: the right operand %s", fault);
    if (rq->right->n_observable != cmp.left.n_obs)
        return fail(STCSP_E_INVALID, "compare: the right operand has %d observable variables, the observer has %d", rq->right->n_observable, cmp.left.n_obs);
    auto t0 = std::chrono::steady_clock::now();
    const unsigned long long max_pairs = std::min<unsigned long long>(rq->max_pairs ? (unsigned long long)rq->max_pairs : 1ull << 26, 0x7ffffffeull);
    const size_t n_obs = (size_t)cmp.left.n_obs;
    cmp.c_witness.clear();
    cmp.c_witness.reserve(1);  // (an empty vector still gives a valid pointer)
    memset(out, 0, sizeof *out);
    out->n_observable = cmp.left.n_obs;
    out->witness_values = cmp.c_witness.data();
    for (int k = 0; k < 4; k++) out->witness_len[k] = out->witness_left[k] = out->witness_right[k] = -1;
    const CompareOperand &left = cmp.left;
    CompareOperand right;
    right.load(*rq->right);
    if (!left.n_states && !right.n_states) {  // two automata without states: no pair
        out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return STCSP_OK;
    }
    // common label ranks: the rows of both operands in one order
    std::vector<int32_t> rows;
    std::vector<uint32_t> map_l, map_r, lab_l(left.lab.size()), lab_r(right.lab.size());
    const uint32_t n_rows = merge_rows(n_obs, left.rows, left.n_rows, right.rows, right.n_rows, rows, map_l, map_r);
    for (size_t e = 0; e < lab_l.size(); e++) lab_l[e] = map_l[left.lab[e]];
    for (size_t e = 0; e < lab_r.size(); e++) lab_r[e] = map_r[right.lab[e]];
    size_t budget = 0;
    if (int rc = table_budget("STCSP_COMPARE_BYTES", budget)) return rc;
    const size_t operand_bytes = (left.off.size() + right.off.size() + 2 * (lab_l.size() + lab_r.size())) * sizeof(uint32_t) + left.fin.size() + right.fin.size();
    if (operand_bytes > budget)
        return fail(STCSP_E_NOMEM, "compare: the operands need %zu bytes, the budget (STCSP_COMPARE_BYTES) is %zu; the product got to level 0 with 0 pairs", operand_bytes, budget);
    auto upload = [&](auto &buf, const auto &vec) -> int {
        HIPCHK(buf.reserve(vec.size()));
        if (!vec.empty()) HIPCHK(hipMemcpyAsync(buf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, v.stream));
        return STCSP_OK;
    };
    if (!cmp.left_on_device) {
        if (int rc = upload(cmp.d_cloff, left.off)) return rc;
        if (int rc = upload(cmp.d_cldst, left.dst)) return rc;
        if (int rc = upload(cmp.d_clfin, left.fin)) return rc;
    }
    if (int rc = upload(cmp.d_cllab, lab_l)) return rc;
    if (int rc = upload(cmp.d_croff, right.off)) return rc;
    if (int rc = upload(cmp.d_crlab, lab_r)) return rc;
    if (int rc = upload(cmp.d_crdst, right.dst)) return rc;
    if (int rc = upload(cmp.d_crfin, right.fin)) return rc;
    HIPCHK(hipStreamSynchronize(v.stream));  // (the vectors of this call are locals)
    cmp.left_on_device = true;
    const CmpSide L{cmp.d_cloff.p, cmp.d_cllab.p, cmp.d_cldst.p, cmp.d_clfin.p, left.n_states}, R{cmp.d_croff.p, cmp.d_crlab.p, cmp.d_crdst.p, cmp.d_crfin.p, right.n_states};
    auto pow2 = [](unsigned long long n) {
        unsigned long long c = 64;
        while (c < n) c <<= 1;
        return c;
    };
    unsigned long long slots = 1024;
    if (const char *e = getenv("STCSP_COMPARE_SLOTS")) slots = pow2((unsigned long long)std::max(1ll, std::min(atoll(e), 1ll << 30)));
    unsigned long long cap_new = 1, n_pairs = 0, edges = 0, peak = 0;
    int levels = 0;
    auto bytes_of = [&](unsigned long long s, unsigned long long fresh, unsigned long long pairs) {
        return operand_bytes + s * 2 * sizeof(unsigned long long) + fresh * (sizeof(unsigned long long) + 2 * sizeof(uint32_t)) +
               pairs * (sizeof(unsigned long long) + 2 * sizeof(uint32_t));
    };
    auto over_budget = [&](unsigned long long need) {
        return fail(STCSP_E_NOMEM, "compare: level %d needs %llu bytes of table, records and scratch, the budget (STCSP_COMPARE_BYTES) is %zu; the product got to level %d with %llu pairs and %llu edges",
                    levels, need, budget, levels, n_pairs, edges);
    };
    if (bytes_of(slots, cap_new, 1) > budget) return over_budget(bytes_of(slots, cap_new, 1));
    if (!cmp.d_ctab.reserve_or_release(slots) || !cmp.d_cmin.reserve_or_release(slots)) return fail(STCSP_E_NOMEM, "compare: no room for a table of %llu slots", slots);
    HIPCHK(cmp.d_cnew.reserve(1));
    HIPCHK(cmp.d_cctl.reserve_exact(C_WORDS));
    HIPCHK(ev.ready(6));
    uint32_t ctl[C_WORDS] = {0};
    for (int k = 0; k < 4; k++) ctl[C_VERDICT + k] = kCmpNone;
    HIPCHK(hipMemcpyAsync(cmp.d_cctl.p, ctl, sizeof ctl, hipMemcpyHostToDevice, v.stream));
    HIPCHK(hipMemsetAsync(cmp.d_ctab.p, 0xff, slots * sizeof(unsigned long long), v.stream));
    HIPCHK(hipMemsetAsync(cmp.d_cmin.p, 0xff, slots * sizeof(unsigned long long), v.stream));
    // the root pair: an operand without states starts in its sink (index 0 == n_states)
    hipLaunchKernelGGL(k_c_init, dim3(1), dim3(64), 0, v.stream, 0ull, cmp.d_ctab.p, cmp.d_cmin.p, (uint32_t)(slots - 1), cmp.d_cnew.p, cmp.d_cctl.p);
    auto read_ctl = [&]() -> int {
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ctl, cmp.d_cctl.p, sizeof ctl, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        if (ctl[C_ERROR]) return fail(STCSP_E_INTERNAL, "compare: a device table overflowed (flags %u)", ctl[C_ERROR]);
        return STCSP_OK;
    };
    bool number_pending = false;
    auto take_number_time = [&]() -> int {
        float ms = 0;
        if (number_pending) HIPCHK(hipEventElapsedTime(&ms, ev[4], ev[5]));
        out->seconds_number += ms * 1e-3;
        number_pending = false;
        return STCSP_OK;
    };
    std::vector<unsigned long long> keys;
    std::vector<uint32_t> idx;
    std::vector<uint32_t> &rank = cmp.c_rank;  // (a member: its upload may still be queued when a level fails)
    for (unsigned long long n_new = 1; n_new;) {
        // the n_new pairs of this level: their numbers, their records, their verdicts
        if (n_pairs + n_new > max_pairs)
            return fail(STCSP_E_NOMEM, "compare: more than max_pairs = %llu pairs; the product got to level %d with %llu pairs and %llu edges", max_pairs, levels,
                        n_pairs, edges);
        if (bytes_of(slots, cap_new, n_pairs + n_new) > budget) return over_budget(bytes_of(slots, cap_new, n_pairs + n_new));
        if (int rc = grow_keeping(cmp.d_cpkey, (size_t)n_pairs, (size_t)(n_pairs + n_new), "compare")) return rc;
        if (int rc = grow_keeping(cmp.d_cparent, (size_t)n_pairs, (size_t)(n_pairs + n_new), "compare")) return rc;
        if (int rc = grow_keeping(cmp.d_cplabel, (size_t)n_pairs, (size_t)(n_pairs + n_new), "compare")) return rc;
        HIPCHK(cmp.d_ckeys.reserve((size_t)n_new));
        HIPCHK(cmp.d_crank.reserve((size_t)n_new));
        const unsigned nb = (unsigned)((n_new + 255) / 256);
        HIPCHK(hipMemsetAsync(cmp.d_cctl.p + C_DEG, 0, 2 * sizeof(uint32_t), v.stream));
        HIPCHK(hipEventRecord(ev[2], v.stream));
        hipLaunchKernelGGL(k_c_collect, dim3(nb), dim3(256), 0, v.stream, (uint32_t)n_new, (const uint32_t *)cmp.d_cnew.p, (const unsigned long long *)cmp.d_ctab.p,
                           (const unsigned long long *)cmp.d_cmin.p, L.off, R.off, cmp.d_ckeys.p, cmp.d_cctl.p);
        HIPCHK(hipEventRecord(ev[3], v.stream));
        keys.resize((size_t)n_new);
        HIPCHK(hipMemcpyAsync(keys.data(), cmp.d_ckeys.p, (size_t)n_new * sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream));
        if (int rc = read_ctl()) return rc;
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev[2], ev[3]));
        out->seconds_number += ms * 1e-3;
        idx.resize((size_t)n_new);
        rank.resize((size_t)n_new);
        for (uint32_t i = 0; i < n_new; i++) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
        for (uint32_t i = 0; i < n_new; i++) rank[idx[i]] = i;
        HIPCHK(hipMemcpyAsync(cmp.d_crank.p, rank.data(), (size_t)n_new * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipEventRecord(ev[4], v.stream));
        hipLaunchKernelGGL(k_c_number, dim3(nb), dim3(256), 0, v.stream, (uint32_t)n_new, (uint32_t)n_pairs, (const uint32_t *)cmp.d_cnew.p, (const uint32_t *)cmp.d_crank.p,
                           (const unsigned long long *)cmp.d_ctab.p, (const unsigned long long *)cmp.d_ckeys.p, L.fin, R.fin, L.n, R.n, cmp.d_cpkey.p, cmp.d_cparent.p, cmp.d_cplabel.p,
                           cmp.d_cctl.p);
        HIPCHK(hipEventRecord(ev[5], v.stream));
        number_pending = true;
        const uint32_t f0 = (uint32_t)n_pairs, f1 = (uint32_t)(n_pairs + n_new);
        n_pairs += n_new;
        levels++;
        peak = std::max(peak, bytes_of(slots, cap_new, n_pairs));
        // the next level: the out-degrees of the frontier's components bound its new pairs
        const unsigned long long bound = (unsigned long long)ctl[C_DEG] | ((unsigned long long)ctl[C_DEG + 1] << 32);
        if (!bound) break;
        if (n_pairs + bound > 0x3fffffffull)
            return fail(STCSP_E_NOMEM, "compare: a table for %llu pairs has more than 2^31 slots; the product got to level %d with %llu pairs and %llu edges",
                        n_pairs + bound, levels, n_pairs, edges);
        const unsigned long long want = std::max(slots, pow2(2 * (n_pairs + bound)));
        if (bytes_of(want, bound, n_pairs) > budget) return over_budget(bytes_of(want, bound, n_pairs));
        if (want > slots) {
            if (!cmp.d_ctab2.reserve_or_release(want) || !cmp.d_cmin.reserve_or_release(want))
                return fail(STCSP_E_NOMEM, "compare: no room for a table of %llu slots at level %d (%llu pairs so far)", want, levels, n_pairs);
            HIPCHK(hipMemsetAsync(cmp.d_ctab2.p, 0xff, want * sizeof(unsigned long long), v.stream));
            HIPCHK(hipMemsetAsync(cmp.d_cmin.p, 0xff, want * sizeof(unsigned long long), v.stream));
            hipLaunchKernelGGL(k_c_rehash, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, v.stream, (uint32_t)slots, (const unsigned long long *)cmp.d_ctab.p, cmp.d_ctab2.p,
                               (uint32_t)(want - 1), cmp.d_cctl.p);
            std::swap(cmp.d_ctab.p, cmp.d_ctab2.p);
            std::swap(cmp.d_ctab.n, cmp.d_ctab2.n);
            slots = want;
        }
        cap_new = std::min<unsigned long long>(bound, 0xffffffffull);
        if (!cmp.d_cnew.reserve_or_release((size_t)cap_new)) return fail(STCSP_E_NOMEM, "compare: no room for %llu new pairs at level %d (%llu pairs so far)", cap_new, levels, n_pairs);
        peak = std::max(peak, bytes_of(slots, cap_new, n_pairs));
        // lanes per pair by the mean out-degree of the frontier: 8 for the common few edges per pair, a wavefront for wide pairs
        const bool wide = bound > 16ull * (f1 - f0);
        const unsigned groups = wide ? 4 : 32;
        const unsigned grid = (unsigned)std::min<unsigned long long>(((unsigned long long)(f1 - f0) + groups - 1) / groups, 8192);
        HIPCHK(hipMemsetAsync(cmp.d_cctl.p + C_NEW, 0, sizeof(uint32_t), v.stream));
        HIPCHK(hipEventRecord(ev[0], v.stream));
        hipLaunchKernelGGL(wide ? k_c_expand<64> : k_c_expand<8>, dim3(grid), dim3(256), 0, v.stream, f0, f1, (const unsigned long long *)cmp.d_cpkey.p, L, R, cmp.d_ctab.p,
                           cmp.d_cmin.p, (uint32_t)(slots - 1), cmp.d_cnew.p, (uint32_t)cap_new, cmp.d_cctl.p);
        HIPCHK(hipEventRecord(ev[1], v.stream));
        if (int rc = read_ctl()) return rc;
        if (int rc = take_number_time()) return rc;
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        out->seconds_expand += ms * 1e-3;
        n_new = ctl[C_NEW];
        edges = (unsigned long long)ctl[C_EDGES] | ((unsigned long long)ctl[C_EDGES + 1] << 32);
    }
    if (int rc = read_ctl()) return rc;  // (the last number launch)
    if (int rc = take_number_time()) return rc;
    // the witnesses: the access sequence of each verdict's pair, from the (parent, label) records
    std::vector<uint32_t> parent((size_t)n_pairs), plabel((size_t)n_pairs);
    HIPCHK(hipMemcpyAsync(parent.data(), cmp.d_cparent.p, (size_t)n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipMemcpyAsync(plabel.data(), cmp.d_cplabel.p, (size_t)n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
    unsigned long long wkey[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; k++)
        if (ctl[C_VERDICT + k] != kCmpNone) {
            if (ctl[C_VERDICT + k] >= n_pairs) return fail(STCSP_E_INTERNAL, "compare: verdict %d names pair %u of %llu", k, ctl[C_VERDICT + k], n_pairs);
            HIPCHK(hipMemcpyAsync(&wkey[k], cmp.d_cpkey.p + ctl[C_VERDICT + k], sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream));
        }
    HIPCHK(hipStreamSynchronize(v.stream));
    std::vector<uint32_t> path;
    for (int k = 0; k < 4; k++) {
        out->witness_off[k + 1] = out->witness_off[k];
        if (ctl[C_VERDICT + k] == kCmpNone) continue;
        path.clear();
        for (uint32_t q = ctl[C_VERDICT + k]; q; q = parent[q]) {
            if (parent[q] >= q || plabel[q] >= n_rows)
                return fail(STCSP_E_INTERNAL, "compare: the record of pair %u does not lead to the root", q);
            path.push_back(plabel[q]);
        }
        for (size_t i = path.size(); i-- > 0;) cmp.c_witness.insert(cmp.c_witness.end(), rows.begin() + path[i] * n_obs, rows.begin() + (path[i] + 1) * n_obs);
        const uint32_t l = (uint32_t)(wkey[k] >> 32), r = (uint32_t)wkey[k];
        out->witness_len[k] = (int32_t)path.size();
        out->witness_left[k] = l == left.n_states ? -1 : (int32_t)l;
        out->witness_right[k] = r == right.n_states ? -1 : (int32_t)r;
        out->witness_off[k + 1] += (int64_t)path.size();
    }
    cmp.c_witness.reserve(1);
    out->witness_values = cmp.c_witness.data();
    out->n_pairs = (int64_t)n_pairs;
    out->n_pair_edges = (int64_t)edges;
    out->levels = levels;
    out->table_bytes = (int64_t)peak;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Strongly connected components of the live automaton, omega-liveness and lasso solutions (contract: stcsp_engine.h;
// dev_components.hpp). Every device buffer lives for the call, the shared CSR group too; no other service's state is touched.
int AutomatonServices::components(const AutomatonView &view, const stcsp_components_options *co, stcsp_components_result *out) {
    if (int rc = enter(view, "components", NEED_FLAGS, "stcsp_automaton_components")) return rc;
    auto t0 = std::chrono::steady_clock::now();
    const int N = v.N;
    const uint32_t S = v.n_states;
    const int64_t max_lassos = co ? co->max_lassos : 0;
    const int32_t flags = co ? co->flags : 0;
    if (max_lassos < -1) return fail(STCSP_E_INVALID, "components: max_lassos is 0 (none), -1 (all) or a positive count");
    if (v.exp_edges > 0x7fffffffull || S > 0x3fffffffu) return fail(STCSP_E_NOMEM, "automaton too large for the device component pass");
    if (int rc = live_set()) return rc;
    HIPCHK(reserve_all(S, 1, scc.d_scomp, scc.d_scolour, scc.d_sin, scc.d_sout, scc.d_sdepth));
    HIPCHK(scc.d_sinfo.reserve(4 * (size_t)S));
    HIPCHK(scc.d_somega.reserve(S));
    HIPCHK(scc.d_sctl.reserve_exact(S_WORDS));
    HIPCHK(scc.d_ssel.reserve_exact(64));
    const unsigned sb = (S + 255) / 256;
    const size_t sw = (size_t)S * sizeof(uint32_t);
    uint32_t ctl[S_WORDS] = {0, 0, 0, 0};
    LaunchBatch run{v.stream, ev, scc.d_sctl.p, ctl, S_WORDS};
    int32_t sweeps = 0, trim_rounds = 0, colour_rounds = 0;
    // the live edges as CSR by source
    uint32_t L = 0;
    HIPCHK(run.begin());
    HIPCHK(hipMemsetAsync(scc.d_sctl.p, 0, sizeof ctl, v.stream));
    if (int rc = csr_count(run, post.d_live.p, "components: %u live edges of %u", L)) return rc;
    if (int rc = csr_fill()) return rc;
    const unsigned lb = (L + 255) / 256;
    const uint32_t *csrc = csr.src.p, *cdst = csr.dst.p;
    auto fixpoint = [&](const char *diverged, auto &&step) -> int {  // step(i) launches sweep i
        return batched_fixpoint(run, S_CHANGED, S + 8, diverged, [&](uint32_t i) -> int { return sweeps++, step(i); });
    };
    // trim and colour until every live state has a component
    HIPCHK(hipMemsetAsync(scc.d_scomp.p, 0xff, sw, v.stream));
    while ((int64_t)ctl[S_ASSIGNED] < post.n_live) {
        if (!(flags & STCSP_SCC_NO_TRIM)) {
            const int rc = fixpoint("components: trimming did not converge", [&](uint32_t) -> int {
                HIPCHK(hipMemsetAsync(scc.d_sin.p, 0, sw, v.stream));
                HIPCHK(hipMemsetAsync(scc.d_sout.p, 0, sw, v.stream));
                if (L) hipLaunchKernelGGL(k_s_deg, dim3(lb), dim3(256), 0, v.stream, L, csrc, cdst, (const uint32_t *)scc.d_scomp.p, scc.d_sin.p, scc.d_sout.p);
                hipLaunchKernelGGL(k_s_trim, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_live.p, (const uint32_t *)scc.d_sin.p,
                                   (const uint32_t *)scc.d_sout.p, scc.d_scomp.p, scc.d_sctl.p);
                trim_rounds++;
                return STCSP_OK;
            });
            if (rc) return rc;
            if ((int64_t)ctl[S_ASSIGNED] >= post.n_live) break;
        }
        if ((uint32_t)colour_rounds++ > S + 8) return fail(STCSP_E_INTERNAL, "components: the colouring rounds did not converge");
        HIPCHK(run.begin());
        hipLaunchKernelGGL(k_s_colour_init, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_live.p, (const uint32_t *)scc.d_scomp.p, scc.d_scolour.p);
        int rc = fixpoint("components: colouring did not converge", [&](uint32_t) -> int {
            if (L) hipLaunchKernelGGL(k_s_colour_fwd, dim3(lb), dim3(256), 0, v.stream, L, csrc, cdst, scc.d_scolour.p, scc.d_sctl.p);
            return STCSP_OK;
        });
        if (rc) return rc;
        HIPCHK(run.begin());
        hipLaunchKernelGGL(k_s_roots, dim3(sb), dim3(256), 0, v.stream, S, (const uint32_t *)scc.d_scolour.p, scc.d_scomp.p, scc.d_sctl.p);
        rc = fixpoint("components: collecting did not converge", [&](uint32_t) -> int {
            if (L) hipLaunchKernelGGL(k_s_colour_back, dim3(lb), dim3(256), 0, v.stream, L, csrc, cdst, (const uint32_t *)scc.d_scolour.p, scc.d_scomp.p, scc.d_sctl.p);
            return STCSP_OK;
        });
        if (rc) return rc;
    }
    if ((int64_t)ctl[S_ASSIGNED] != post.n_live) return fail(STCSP_E_INTERNAL, "components: %u of %lld live states have a component", ctl[S_ASSIGNED], (long long)post.n_live);
    // depths, the facts of every component, omega
    HIPCHK(run.begin());
    HIPCHK(hipMemsetAsync(scc.d_sdepth.p, 0xff, sw, v.stream));
    if (post.root_live) HIPCHK(hipMemsetAsync(scc.d_sdepth.p, 0, sizeof(uint32_t), v.stream));
    if (int rc = fixpoint("components: the depths did not converge", [&](uint32_t level) -> int {
            if (L) hipLaunchKernelGGL(k_s_bfs, dim3(lb), dim3(256), 0, v.stream, L, level, csrc, cdst, scc.d_sdepth.p, scc.d_sctl.p);
            return STCSP_OK;
        }))
        return rc;
    HIPCHK(run.begin());
    HIPCHK(hipMemsetAsync(scc.d_sinfo.p, 0, 2 * sw, v.stream));
    HIPCHK(hipMemsetAsync(scc.d_sinfo.p + 2 * (size_t)S, 0xff, 2 * sw, v.stream));
    hipLaunchKernelGGL(k_s_state_info, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_live.p, (const uint8_t *)post.d_pfinal.p,
                       (const uint32_t *)scc.d_scomp.p, (const uint32_t *)scc.d_sdepth.p, scc.d_sinfo.p);
    if (L) hipLaunchKernelGGL(k_s_edge_info, dim3(lb), dim3(256), 0, v.stream, L, S, csrc, cdst, (const uint32_t *)scc.d_scomp.p, scc.d_sinfo.p);
    hipLaunchKernelGGL(k_s_omega_init, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_live.p, (const uint32_t *)scc.d_scomp.p,
                       (const uint32_t *)scc.d_sinfo.p, scc.d_somega.p);
    if (int rc = fixpoint("components: omega did not converge", [&](uint32_t) -> int {
            if (L) hipLaunchKernelGGL(k_s_omega_back, dim3(lb), dim3(256), 0, v.stream, L, csrc, cdst, scc.d_somega.p, scc.d_sctl.p);
            return STCSP_OK;
        }))
        return rc;
    std::vector<uint32_t> raw(S), info(4 * (size_t)S);
    scc.s_omega.assign(S, 0);
    HIPCHK(hipMemcpyAsync(raw.data(), scc.d_scomp.p, sw, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipMemcpyAsync(info.data(), scc.d_sinfo.p, 4 * sw, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(hipMemcpyAsync(scc.s_omega.data(), scc.d_somega.p, S, hipMemcpyDeviceToHost, v.stream));
    HIPCHK(run.flush());
    // component numbers by least member: a component's raw name is its least member, so the first state that shows it is that member
    scc.s_component.assign(S, -1);
    scc.s_size.clear();
    scc.s_depth.clear();
    scc.s_flags.clear();
    std::vector<int32_t> number(S, -1);
    std::vector<uint32_t> least;
    memset(out, 0, sizeof *out);
    for (uint32_t s = 0; s < S; s++) {
        if (!post.live[s]) continue;
        const uint32_t r = raw[s];
        if (r >= S || (number[r] < 0 && r != s)) return fail(STCSP_E_INTERNAL, "components: state %u is named after %u, not its component's least member", s, r);
        if (number[r] < 0) {
            number[r] = (int32_t)least.size();
            least.push_back(r);
            const uint32_t f = info[(size_t)S + r];
            int32_t cf = (f & S_INFO_CYCLIC ? STCSP_SCC_CYCLIC : 0) | (f & S_INFO_FINAL ? STCSP_SCC_FINAL : 0) | (f & S_INFO_LEAVES ? 0 : STCSP_SCC_BOTTOM);
            if ((f & S_INFO_CYCLIC) && (f & S_INFO_FINAL)) cf |= STCSP_SCC_ACCEPTING;
            scc.s_size.push_back((int32_t)info[r]);
            scc.s_depth.push_back((int32_t)info[2 * (size_t)S + r]);
            scc.s_flags.push_back(cf);
            out->n_cyclic += (cf & STCSP_SCC_CYCLIC) != 0;
            out->n_accepting += (cf & STCSP_SCC_ACCEPTING) != 0;
            out->n_bottom += (cf & STCSP_SCC_BOTTOM) != 0;
        }
        scc.s_component[s] = number[r];
        out->n_omega += scc.s_omega[s];
    }
    // lassos: the accepting components by (depth, number), 64 stems per pass, then every loop at once
    scc.s_lcomp.clear();
    scc.s_lstem.clear();
    scc.s_lvalues.clear();
    scc.s_loff.assign(1, 0);
    std::vector<int32_t> wanted;
    if (max_lassos != 0)
        for (int32_t c = 0; c < (int32_t)scc.s_flags.size(); c++)
            if ((scc.s_flags[c] & STCSP_SCC_ACCEPTING) && (!(flags & STCSP_SCC_LASSO_BOTTOM) || (scc.s_flags[c] & STCSP_SCC_BOTTOM))) wanted.push_back(c);
    std::stable_sort(wanted.begin(), wanted.end(), [&](int32_t a, int32_t b) { return scc.s_depth[a] < scc.s_depth[b]; });
    if (max_lassos > 0 && (int64_t)wanted.size() > max_lassos) wanted.resize((size_t)max_lassos);
    if (!wanted.empty()) {
        std::vector<uint32_t> depth(S), off((size_t)S + 1), heid(L), dist(S), anchors(wanted.size());
        auto hdst = [&](uint32_t k) { return (uint32_t)v.h_odst[heid[k]]; };  // (the destinations are in the pinned export already)
        std::vector<unsigned long long> mark(S);
        std::vector<std::vector<int32_t>> stems(wanted.size());
        HIPCHK(scc.d_smark.reserve(S));
        HIPCHK(scc.d_sdist.reserve(S));
        HIPCHK(hipMemcpyAsync(depth.data(), scc.d_sdepth.p, sw, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(off.data(), csr.off.p, sw + sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(heid.data(), csr.eid.p, (size_t)L * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
        bool twice = false;
        // the position of the live out-edge of u with the least full row among those whose destination `ok` admits; L when there is none
        auto least_edge = [&](uint32_t u, auto &&ok) {
            uint32_t best = L;
            for (uint32_t k = off[u]; k < off[u + 1]; k++) {
                if (!ok(hdst(k))) continue;
                if (best == L) {
                    best = k;
                    continue;
                }
                const int32_t *x = v.h_oval + (size_t)heid[k] * N, *y = v.h_oval + (size_t)heid[best] * N;
                if (std::equal(x, x + N, y)) twice = true;
                if (std::lexicographical_compare(x, x + N, y, y + N)) best = k;
            }
            return best;
        };
        for (size_t p0 = 0; p0 < wanted.size(); p0 += 64) {
            const int n_sel = (int)std::min<size_t>(64, wanted.size() - p0);
            uint32_t sel[64], deepest = 0;
            for (int j = 0; j < n_sel; j++) {
                sel[j] = least[(size_t)wanted[p0 + j]];
                deepest = std::max(deepest, info[3 * (size_t)S + sel[j]]);
            }
            if (deepest > S) return fail(STCSP_E_INTERNAL, "components: an accepting component without a final state");
            HIPCHK(run.begin());
            HIPCHK(hipMemcpyAsync(scc.d_ssel.p, sel, (size_t)n_sel * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
            hipLaunchKernelGGL(k_s_stem_init, dim3(sb), dim3(256), 0, v.stream, S, n_sel, (const uint32_t *)scc.d_ssel.p, (const uint8_t *)post.d_live.p,
                               (const uint8_t *)post.d_pfinal.p, (const uint32_t *)scc.d_scomp.p, (const uint32_t *)scc.d_sdepth.p, (const uint32_t *)scc.d_sinfo.p,
                               scc.d_smark.p);
            for (uint32_t level = deepest; level-- > 0; sweeps++)
                hipLaunchKernelGGL(k_s_stem_back, dim3(lb), dim3(256), 0, v.stream, L, level, csrc, cdst, (const uint32_t *)scc.d_sdepth.p, scc.d_smark.p);
            HIPCHK(hipMemcpyAsync(mark.data(), scc.d_smark.p, (size_t)S * sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream));
            HIPCHK(run.flush());
            for (int j = 0; j < n_sel; j++) {
                const uint32_t len = info[3 * (size_t)S + sel[j]];
                uint32_t u = 0;
                for (uint32_t t = 0; t < len; t++) {
                    const uint32_t k = least_edge(u, [&](uint32_t w) { return depth[w] == t + 1 && ((mark[w] >> j) & 1); });
                    if (twice) return fail(STCSP_E_INTERNAL, "components: two live out-edges of state %u carry the same full row", u);
                    if (k == L) return fail(STCSP_E_INTERNAL, "components: the stem of component %d stops at state %u", wanted[p0 + j], u);
                    stems[p0 + j].insert(stems[p0 + j].end(), v.h_oval + (size_t)heid[k] * N, v.h_oval + ((size_t)heid[k] + 1) * N);
                    u = hdst(k);
                }
                if (raw[u] != sel[j] || !((mark[u] >> j) & 1)) return fail(STCSP_E_INTERNAL, "components: the stem of component %d ends in state %u", wanted[p0 + j], u);
                anchors[p0 + j] = u;
            }
        }
        // the anchors' buffer: the colours are no longer needed (as many anchors as components at the most)
        HIPCHK(run.begin());
        HIPCHK(hipMemcpyAsync(scc.d_scolour.p, anchors.data(), anchors.size() * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipMemsetAsync(scc.d_sdist.p, 0xff, sw, v.stream));
        hipLaunchKernelGGL(k_s_loop_init, dim3(((unsigned)anchors.size() + 255) / 256), dim3(256), 0, v.stream, (uint32_t)anchors.size(), S,
                           (const uint32_t *)scc.d_scolour.p, scc.d_sdist.p);
        if (int rc = fixpoint("components: the loop distances did not converge", [&](uint32_t level) -> int {
                if (L) hipLaunchKernelGGL(k_s_loop_back, dim3(lb), dim3(256), 0, v.stream, L, level, csrc, cdst, (const uint32_t *)scc.d_scomp.p, scc.d_sdist.p, scc.d_sctl.p);
                return STCSP_OK;
            }))
            return rc;
        HIPCHK(hipMemcpyAsync(dist.data(), scc.d_sdist.p, sw, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(run.flush());
        for (size_t i = 0; i < wanted.size(); i++) {
            const uint32_t a = anchors[i], r = raw[a];
            uint32_t loop_len = kSNone;
            for (uint32_t k = off[a]; k < off[a + 1]; k++)
                if (raw[hdst(k)] == r && dist[hdst(k)] != kSNone) loop_len = std::min(loop_len, dist[hdst(k)] + 1);
            if (loop_len == kSNone) return fail(STCSP_E_INTERNAL, "components: no loop through state %u of component %d", a, wanted[i]);
            scc.s_lvalues.insert(scc.s_lvalues.end(), stems[i].begin(), stems[i].end());
            uint32_t u = a;
            for (uint32_t rem = loop_len; rem > 0; rem--) {
                const uint32_t k = least_edge(u, [&](uint32_t w) { return raw[w] == r && dist[w] == rem - 1; });
                if (twice) return fail(STCSP_E_INTERNAL, "components: two live out-edges of state %u carry the same full row", u);
                if (k == L) return fail(STCSP_E_INTERNAL, "components: the loop of component %d stops at state %u", wanted[i], u);
                scc.s_lvalues.insert(scc.s_lvalues.end(), v.h_oval + (size_t)heid[k] * N, v.h_oval + ((size_t)heid[k] + 1) * N);
                u = hdst(k);
            }
            if (u != a) return fail(STCSP_E_INTERNAL, "components: the loop of component %d ends in state %u, not in %u", wanted[i], u, a);
            scc.s_lcomp.push_back(wanted[i]);
            scc.s_lstem.push_back((int32_t)(stems[i].size() / (size_t)std::max(N, 1)));
            scc.s_loff.push_back(scc.s_loff.back() + (int64_t)(stems[i].size() / (size_t)std::max(N, 1)) + loop_len);
        }
    }
    for (auto *vec : {&scc.s_component, &scc.s_size, &scc.s_depth, &scc.s_flags, &scc.s_lcomp, &scc.s_lstem, &scc.s_lvalues}) vec->reserve(1);
    scc.s_omega.reserve(1);
    out->n_states = post.n_live;
    out->n_components = (int64_t)scc.s_size.size();
    out->state_component = scc.s_component.data();
    out->state_omega = scc.s_omega.data();
    out->comp_size = scc.s_size.data();
    out->comp_depth = scc.s_depth.data();
    out->comp_flags = scc.s_flags.data();
    out->n_lassos = (int64_t)scc.s_lcomp.size();
    out->lasso_component = scc.s_lcomp.data();
    out->lasso_off = scc.s_loff.data();
    out->lasso_stem_len = scc.s_lstem.data();
    out->lasso_values = scc.s_lvalues.data();
    out->n_vars = N;
    out->root_omega = post.root_live && scc.s_omega[0];
    out->rounds[0] = trim_rounds;
    out->rounds[1] = colour_rounds;
    out->rounds[2] = sweeps;
    out->seconds_kernels = run.ms * 1e-3;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Optimal solution streams: the least cost of a solution prefix per length with its lexicographically least witness, and the
// minimum cycle mean of every cyclic component (contract: stcsp_engine.h; dev_optimise.hpp). Every
// device buffer is this call's own or, the CSR group, built anew by it; with STCSP_OPT_MEAN the component pass above runs first and its result is replaced.
int AutomatonServices::optimise(const AutomatonView &view, const stcsp_optimise_request *rq, stcsp_optimise_result *out) {
    if (int rc = enter(view, "optimise", NEED_FLAGS, "stcsp_automaton_optimise")) return rc;
    auto t0 = std::chrono::steady_clock::now();
    const int N = v.N;
    const uint32_t S = v.n_states;
    const int32_t horizon = rq->horizon, n_len = rq->n_lengths, flags = rq->flags;
    if (!rq->weights) return fail(STCSP_E_INVALID, "optimise: weights is null");
    if (horizon < 0) return fail(STCSP_E_INVALID, "optimise: horizon %d is negative", horizon);
    if (n_len < 0 || (n_len > 0 && !rq->lengths)) return fail(STCSP_E_INVALID, "optimise: n_lengths = %d without that many lengths", n_len);
    for (int32_t i = 0; i < n_len; i++)
        if (rq->lengths[i] < 0 || rq->lengths[i] > horizon)
            return fail(STCSP_E_INVALID, "optimise: lengths[%d] = %d is outside 0 .. horizon = %d", i, rq->lengths[i], horizon);
    const __int128 kLimit = (__int128)1 << 62;
    __int128 cmax = 0;
    for (int x = 0; x < N; x++)
        cmax += (__int128)std::llabs((long long)rq->weights[x]) * std::max(std::llabs((long long)v.lb[x]), std::llabs((long long)v.ub[x]));
    if (cmax * std::max(horizon, 1) > kLimit)
        return fail(STCSP_E_INVALID, "optimise: the largest edge cost %.0f times the horizon %d exceeds 2^62", (double)cmax, horizon);
    if (v.exp_edges > 0x7fffffffull || S > 0x3fffffffu) return fail(STCSP_E_NOMEM, "automaton too large for the device optimisation pass");
    if (int rc = live_set()) return rc;
    const bool maximise = flags & STCSP_OPT_MAXIMISE, mean = flags & STCSP_OPT_MEAN, witnesses = n_len > 0;
    const int end_final = (flags & STCSP_OPT_END_FINAL) ? 1 : 0;
    // the components first: their call takes the view again
    uint32_t nmax = 0, n_comp = 0;
    std::vector<uint32_t> n_of, comp_of, least;
    if (mean) {
        const stcsp_components_options co = {0, 0, 0};
        stcsp_components_result cres;
        if (int rc = components(view, &co, &cres)) return rc;
        n_comp = (uint32_t)scc.s_size.size();
        n_of.assign(S, 0);
        comp_of.assign(S, kOptIdxNone);
        least.assign(n_comp, kOptIdxNone);
        for (uint32_t s = 0; s < S; s++) {
            const int32_t c = scc.s_component[s];
            if (c < 0) continue;
            comp_of[s] = (uint32_t)c;
            if (least[c] == kOptIdxNone) least[c] = s;
            if (scc.s_flags[c] & STCSP_SCC_CYCLIC) {
                n_of[s] = (uint32_t)scc.s_size[c];
                nmax = std::max(nmax, n_of[s]);
            }
        }
        if ((__int128)nmax * nmax * cmax > kLimit)
            return fail(STCSP_E_UNSUPPORTED, "optimise: the largest cyclic component has nmax = %u states and the largest edge cost is cmax = %.0f; nmax^2 * cmax exceeds 2^62, the range of the exact comparisons",
                        nmax, (double)cmax);
    }
    size_t budget = 0;
    if (int rc = table_budget("STCSP_OPTIMISE_BYTES", budget)) return rc;
    const size_t n_rows = witnesses ? (size_t)horizon + 1 : 2;
    const size_t row_bytes = n_rows * (size_t)S * sizeof(long long);
    if (row_bytes > budget)
        return fail(STCSP_E_NOMEM, "optimise: %zu value rows of %u states need %zu bytes, the budget (STCSP_OPTIMISE_BYTES) is %zu", n_rows, S, row_bytes, budget);
    opt.opt_best.assign((size_t)horizon + 1, kOptNone);
    opt.opt_state_best.clear();
    opt.opt_woff.assign((size_t)n_len + 1, 0);
    opt.opt_wvalues.clear();
    opt.opt_wstates.clear();
    opt.opt_component.clear();
    opt.opt_num.assign(n_comp, 0);
    opt.opt_den.assign(n_comp, 0);
    HIPCHK(opt.d_opt_ctl.reserve_exact(OPT_WORDS));
    HIPCHK(opt.d_opt_w.reserve_exact((size_t)std::max(N, 1)));
    HIPCHK(opt.d_opt_best.reserve((size_t)horizon + 1));
    const unsigned sb = (S + 255) / 256;
    uint32_t ctl[OPT_WORDS] = {0, 0, 0, 0};  // the error words
    LaunchBatch run{v.stream, ev, opt.d_opt_ctl.p, ctl, OPT_WORDS};
    int32_t launches_dp = 0, launches_karp = 0;
    std::vector<int32_t> w(rq->weights, rq->weights + N);
    for (int x = 0; x < N && maximise; x++) {
        if (w[x] == INT32_MIN) return fail(STCSP_E_INVALID, "optimise: weights[%d] = INT32_MIN cannot be negated to maximise", x);
        w[x] = -w[x];
    }
    // the live edges as CSR by source, built anew (the component pass above has left its own in the group)
    uint32_t L = 0;
    if (S) {
        HIPCHK(run.begin());
        HIPCHK(hipMemsetAsync(opt.d_opt_ctl.p, 0, sizeof ctl, v.stream));
        if (N) HIPCHK(hipMemcpyAsync(opt.d_opt_w.p, w.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
        if (int rc = csr_count(run, post.d_live.p, "optimise: %u live edges of %u", L)) return rc;
    }
    const size_t need = row_bytes + 3 * ((size_t)S + 1) * sizeof(uint32_t) + (size_t)L * (3 * sizeof(uint32_t) + sizeof(long long)) +
                        ((size_t)horizon + 1) * sizeof(long long) +
                        (mean ? (size_t)S * (3 * sizeof(uint32_t) + 4 * sizeof(long long)) + 2 * (size_t)n_comp * sizeof(uint32_t) : 0);
    if (need > budget)
        return fail(STCSP_E_NOMEM, "optimise: %zu value rows of %u states, %u live edges%s need %zu bytes, the budget (STCSP_OPTIMISE_BYTES) is %zu", n_rows, S, L,
                    mean ? " and the cycle-mean tables" : "", need, budget);
    if (!opt.d_opt_rows.reserve_or_release(n_rows * (size_t)S)) return fail(STCSP_E_NOMEM, "optimise: no room for %zu bytes of value rows", row_bytes);
    HIPCHK(opt.d_opt_cost.reserve(L, 1));
    const unsigned lb = (L + 255) / 256;
    if (S) {
        // finite horizon: V_0, then a relaxation and a clearing launch per level
        auto row = [&](int32_t k) { return opt.d_opt_rows.p + (size_t)(witnesses ? k : k % 2) * S; };
        auto next_row = [&](int32_t k) { return k + 1 <= horizon ? row(k + 1) : (long long *)nullptr; };
        HIPCHK(run.begin());
        if (int rc = csr_fill()) return rc;
        if (L) hipLaunchKernelGGL(k_opt_cost, dim3(lb), dim3(256), 0, v.stream, L, N, (const uint32_t *)csr.eid.p, v.d_oval, (const int32_t *)opt.d_opt_w.p, opt.d_opt_cost.p);
        hipLaunchKernelGGL(k_opt_init, dim3(sb), dim3(256), 0, v.stream, S, (const uint8_t *)post.d_live.p, (const uint8_t *)post.d_pfinal.p, end_final, row(0));
        hipLaunchKernelGGL(k_opt_clear, dim3(sb), dim3(256), 0, v.stream, S, next_row(0), (const long long *)row(0), opt.d_opt_best.p);
        launches_dp += 2;
        for (int32_t k = 1; k <= horizon; k++, launches_dp += 2) {
            if (L)
                hipLaunchKernelGGL(k_opt_relax_back, dim3(lb), dim3(256), 0, v.stream, L, (const uint32_t *)csr.src.p, (const uint32_t *)csr.dst.p, (const long long *)opt.d_opt_cost.p,
                                   (const long long *)row(k - 1), row(k));
            hipLaunchKernelGGL(k_opt_clear, dim3(sb), dim3(256), 0, v.stream, S, next_row(k), (const long long *)row(k), opt.d_opt_best.p + k);
        }
        HIPCHK(hipMemcpyAsync(opt.opt_best.data(), opt.d_opt_best.p, ((size_t)horizon + 1) * sizeof(long long), hipMemcpyDeviceToHost, v.stream));
        if (flags & STCSP_OPT_STATE_BEST) {
            opt.opt_state_best.resize(S);
            HIPCHK(hipMemcpyAsync(opt.opt_state_best.data(), row(horizon), (size_t)S * sizeof(long long), hipMemcpyDeviceToHost, v.stream));
        }
        HIPCHK(run.flush());
        // witnesses: one wavefront per requested length walks the rows; the host gathers the label rows from the pinned export
        for (int32_t i = 0; i < n_len; i++) opt.opt_woff[(size_t)i + 1] = opt.opt_woff[i] + (opt.opt_best[rq->lengths[i]] == kOptNone ? 0 : rq->lengths[i]);
        const size_t T = (size_t)opt.opt_woff[n_len];
        if (T) {
            std::vector<uint32_t> weid(T);
            opt.opt_wstates.resize(T);
            HIPCHK(opt.d_opt_len.reserve((size_t)n_len));
            HIPCHK(opt.d_opt_woff.reserve((size_t)n_len + 1));
            HIPCHK(reserve_all(T, 0, opt.d_opt_weid, opt.d_opt_wstate));
            HIPCHK(run.begin());
            HIPCHK(hipMemcpyAsync(opt.d_opt_len.p, rq->lengths, (size_t)n_len * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
            HIPCHK(hipMemcpyAsync(opt.d_opt_woff.p, opt.opt_woff.data(), ((size_t)n_len + 1) * sizeof(long long), hipMemcpyHostToDevice, v.stream));
            hipLaunchKernelGGL(k_opt_walk, dim3((unsigned)n_len), dim3(64), 0, v.stream, S, N, (int)n_len, (const int32_t *)opt.d_opt_len.p, (const long long *)opt.d_opt_woff.p,
                               (const long long *)opt.d_opt_rows.p, (const uint32_t *)csr.off.p, (const uint32_t *)csr.dst.p, (const uint32_t *)csr.eid.p, (const long long *)opt.d_opt_cost.p,
                               v.d_oval, opt.d_opt_weid.p, opt.d_opt_wstate.p, opt.d_opt_ctl.p);
            launches_dp++;
            HIPCHK(hipMemcpyAsync(weid.data(), opt.d_opt_weid.p, T * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
            HIPCHK(hipMemcpyAsync(opt.opt_wstates.data(), opt.d_opt_wstate.p, T * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
            HIPCHK(run.flush());
            if (ctl[OPT_DUPLICATE]) return fail(STCSP_E_INTERNAL, "optimise: two live out-edges of state %u carry the same full row", ctl[OPT_DUPLICATE] - 1);
            if (ctl[OPT_STUCK]) return fail(STCSP_E_INTERNAL, "optimise: the walk stops at state %u", ctl[OPT_STUCK] - 1);
            if (int rc = walked_rows(weid.data(), T, "optimise: the walk names edge %u of %u", opt.opt_wvalues)) return rc;
        }
    }
    // long run: Karp's minimum cycle mean of every cyclic component in two passes over two rows
    int64_t omega_num = 0, omega_den = 0;
    int32_t omega_comp = -1;
    if (mean) {
        opt.opt_component = scc.s_component;
        if (nmax) {
            std::vector<long long> num(S);
            std::vector<uint32_t> den(S), arg(n_comp);
            HIPCHK(reserve_all(S, 0, opt.d_opt_nof, opt.d_opt_comp, opt.d_opt_den));
            HIPCHK(reserve_all(n_comp, 0, opt.d_opt_least, opt.d_opt_arg));
            HIPCHK(reserve_all(S, 0, opt.d_opt_dn, opt.d_opt_num));
            HIPCHK(opt.d_opt_d.reserve(2 * (size_t)S));
            long long *d[2] = {opt.d_opt_d.p, opt.d_opt_d.p + S};
            HIPCHK(run.begin());
            HIPCHK(hipMemcpyAsync(opt.d_opt_nof.p, n_of.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
            HIPCHK(hipMemcpyAsync(opt.d_opt_comp.p, comp_of.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
            HIPCHK(hipMemcpyAsync(opt.d_opt_least.p, least.data(), (size_t)n_comp * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
            HIPCHK(hipMemsetAsync(opt.d_opt_den.p, 0, (size_t)S * sizeof(uint32_t), v.stream));
            HIPCHK(hipMemsetAsync(opt.d_opt_num.p, 0, (size_t)S * sizeof(long long), v.stream));
            HIPCHK(hipMemsetAsync(opt.d_opt_arg.p, 0xff, (size_t)n_comp * sizeof(uint32_t), v.stream));
            const uint32_t *nof = opt.d_opt_nof.p, *comp = opt.d_opt_comp.p;
            auto fwd = [&](uint32_t k) {
                if (L)
                    hipLaunchKernelGGL(k_opt_karp_fwd, dim3(lb), dim3(256), 0, v.stream, L, (const uint32_t *)csr.src.p, (const uint32_t *)csr.dst.p, comp, (const long long *)opt.d_opt_cost.p,
                                       (const long long *)d[(k - 1) % 2], d[k % 2]);
                launches_karp++;
            };
            // pass 1: D_n of every state, n the size of its component
            hipLaunchKernelGGL(k_opt_karp_init, dim3(sb), dim3(256), 0, v.stream, S, nof, comp, (const uint32_t *)opt.d_opt_least.p, d[0], d[1], opt.d_opt_dn.p);
            for (uint32_t k = 1; k <= nmax; k++, launches_karp++) {
                fwd(k);
                hipLaunchKernelGGL(k_opt_karp_keep, dim3(sb), dim3(256), 0, v.stream, S, k, nof, (const long long *)d[k % 2], d[(k - 1) % 2], opt.d_opt_dn.p);
            }
            // pass 2: D_k again, level by level, and per state the greatest (D_n - D_k) / (n - k)
            hipLaunchKernelGGL(k_opt_karp_init, dim3(sb), dim3(256), 0, v.stream, S, nof, comp, (const uint32_t *)opt.d_opt_least.p, d[0], d[1], (long long *)nullptr);
            for (uint32_t k = 0; k < nmax; k++, launches_karp++) {
                if (k) fwd(k);
                hipLaunchKernelGGL(k_opt_karp_ratio, dim3(sb), dim3(256), 0, v.stream, S, k, nof, (const long long *)d[k % 2], d[(k + 1) % 2],
                                   (const long long *)opt.d_opt_dn.p, opt.d_opt_num.p, opt.d_opt_den.p);
            }
            hipLaunchKernelGGL(k_opt_karp_min, dim3(sb), dim3(256), 0, v.stream, S, S, comp, (const long long *)opt.d_opt_num.p, (const uint32_t *)opt.d_opt_den.p,
                               opt.d_opt_arg.p, opt.d_opt_ctl.p);
            launches_karp += 3;
            HIPCHK(hipMemcpyAsync(num.data(), opt.d_opt_num.p, (size_t)S * sizeof(long long), hipMemcpyDeviceToHost, v.stream));
            HIPCHK(hipMemcpyAsync(den.data(), opt.d_opt_den.p, (size_t)S * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
            HIPCHK(hipMemcpyAsync(arg.data(), opt.d_opt_arg.p, (size_t)n_comp * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
            HIPCHK(run.flush());
            if (ctl[OPT_STUCK]) return fail(STCSP_E_INTERNAL, "optimise: the least mean of the component of state %u did not settle", ctl[OPT_STUCK] - 1);
            for (uint32_t c = 0; c < n_comp; c++) {
                if (!(scc.s_flags[c] & STCSP_SCC_CYCLIC)) continue;
                const uint32_t a = arg[c];
                if (a >= S || den[a] == 0 || comp_of[a] != c) return fail(STCSP_E_INTERNAL, "optimise: cyclic component %u has no cycle mean", c);
                long long p = num[a], q = (long long)den[a], x = std::llabs(p), y = q;
                while (y) {
                    const long long r = x % y;
                    x = y;
                    y = r;
                }
                opt.opt_num[c] = p / x;
                opt.opt_den[c] = q / x;
            }
        }
        for (uint32_t c = 0; c < n_comp; c++) {
            if (!(scc.s_flags[c] & STCSP_SCC_ACCEPTING)) continue;
            if (omega_comp < 0 || (__int128)opt.opt_num[c] * omega_den < (__int128)omega_num * opt.opt_den[c]) {
                omega_num = opt.opt_num[c];
                omega_den = opt.opt_den[c];
                omega_comp = (int32_t)c;
            }
        }
    }
    if (maximise) {
        for (int64_t &x : opt.opt_best)
            if (x != kOptNone) x = -x;
        for (int64_t &x : opt.opt_state_best)
            if (x != kOptNone) x = -x;
        for (int64_t &x : opt.opt_num) x = -x;
        omega_num = -omega_num;
    }
    opt.opt_wvalues.reserve(1);
    opt.opt_wstates.reserve(1);
    opt.opt_num.reserve(1);
    opt.opt_den.reserve(1);
    memset(out, 0, sizeof *out);
    out->n_states = post.n_live;
    out->best = opt.opt_best.data();
    out->state_best = (flags & STCSP_OPT_STATE_BEST) ? opt.opt_state_best.data() : nullptr;
    out->n_witnesses = n_len;
    out->witness_off = opt.opt_woff.data();
    out->witness_values = opt.opt_wvalues.data();
    out->witness_states = opt.opt_wstates.data();
    out->n_components = n_comp;
    out->state_component = mean ? opt.opt_component.data() : nullptr;
    out->comp_mean_num = opt.opt_num.data();
    out->comp_mean_den = opt.opt_den.data();
    out->omega_mean_num = omega_num;
    out->omega_mean_den = omega_den;
    out->omega_component = omega_comp;
    out->n_vars = N;
    out->horizon = horizon;
    out->largest_cyclic = (int32_t)nmax;
    out->rounds[0] = launches_dp;
    out->rounds[1] = launches_karp;
    out->seconds_kernels = run.ms * 1e-3;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

// Fair CTL over the infinite solutions (contract: stcsp_engine.h, stcsp_engine_ctl; dev_ctl.hpp). The
// lowering is CtlProgram's, shared with the host twin. The component pass above runs first and its result is replaced; every
// other device buffer is this call's own (the CSR group: built anew). A set of worlds is a slot of d_ctl_sets; the evaluation is a walk over the lowered
// tree that holds at most the slots CtlProgram measured.
int AutomatonServices::ctl(const AutomatonView &view, const stcsp_ctl_request *rq, stcsp_ctl_result *out) {
    if (int rc = enter(view, "ctl", NEED_FLAGS, "stcsp_automaton_ctl")) return rc;
    auto t0 = std::chrono::steady_clock::now();
    const int N = v.N;
    const uint32_t E = (uint32_t)v.exp_edges, S = v.n_states;
    CtlProgram prog;
    if (int rc = prog.build(rq->program, rq->n_words, N)) return fail(rc, "%s", prog.error.c_str());
    if (v.exp_edges > 0x7fffffffull || S > 0x3fffffffu) return fail(STCSP_E_NOMEM, "automaton too large for the device CTL pass");
    const stcsp_components_options co = {0, 0, 0};  // omega first: the call takes the view again
    stcsp_components_result cres;
    if (int rc = components(view, &co, &cres)) return rc;
    size_t budget = 0;
    if (int rc = table_budget("STCSP_CTL_BYTES", budget)) return rc;
    bool negated = false;
    const int32_t wit = (rq->flags & STCSP_CTL_WITNESS) ? prog.witness_node(&negated) : -1;
    // the slices of the maximal temporal-free subtrees, uploaded once: node -> (first word, length)
    std::vector<int32_t> words_h, slice_off(prog.nodes.size(), -1), slice_len(prog.nodes.size(), 0);
    {
        std::vector<int32_t> todo{prog.root};
        while (!todo.empty()) {
            const int32_t r = todo.back();
            todo.pop_back();
            const CtlNode &n = prog.nodes[(size_t)r];
            if (!n.temporal) {
                slice_off[(size_t)r] = (int32_t)words_h.size();
                prog.slice(r, words_h);
                slice_len[(size_t)r] = (int32_t)words_h.size() - slice_off[(size_t)r];
                continue;
            }
            if (n.a >= 0) todo.push_back(n.a);
            if (n.b >= 0) todo.push_back(n.b);
        }
    }
    HIPCHK(ctlq.d_ctl_ctl.reserve_exact(CTL_WORDS));
    HIPCHK(ctlq.d_ctl_prog.reserve(words_h.size(), 1));
    uint32_t cw[CTL_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    LaunchBatch run{v.stream, ev, ctlq.d_ctl_ctl.p, cw, CTL_WORDS, cres.seconds_kernels * 1e3};  // (the component pass's time counts)
    int32_t sweeps = 0, launches = 0, most_outer = 0;
    // the worlds as CSR by source, built anew over the component pass's: the omega bytes are the state filter
    uint32_t W = 0;
    if (S) {
        HIPCHK(run.begin());
        HIPCHK(hipMemsetAsync(ctlq.d_ctl_ctl.p, 0, sizeof cw, v.stream));
        if (int rc = csr_count(run, scc.d_somega.p, "ctl: %u worlds of %u edges", W)) return rc;
        launches += 2;
    }
    const size_t nw = ((size_t)W + 63) / 64;
    const int n_slots = prog.nodes[(size_t)prog.root].slots;
    const size_t need = 3 * ((size_t)S + 1) * sizeof(uint32_t) + (size_t)W * 3 * sizeof(uint32_t) + 2 * (size_t)S + 2 * (size_t)E +
                        ((size_t)n_slots + 1) * nw * sizeof(unsigned long long) + (wit >= 0 ? 2 * ((size_t)W + 16) * sizeof(uint32_t) : 0) +
                        words_h.size() * sizeof(int32_t);
    if (need > budget)
        return fail(STCSP_E_NOMEM, "ctl: %u worlds, %u states, %u edges and %d sets need %zu bytes, the budget (STCSP_CTL_BYTES) is %zu", W, S, E, n_slots, need, budget);
    ctlq.ctl_world.assign(E, 0);
    ctlq.ctl_sat.assign(E, 0);
    ctlq.ctl_witness.clear();
    int32_t witness_kind = STCSP_CTL_NONE, witness_len = 0;
    if (W) {
        HIPCHK(ctlq.d_ctl_sets.reserve(((size_t)n_slots + 1) * nw));
        HIPCHK(ctlq.d_ctl_some.reserve(2 * (size_t)S));
        HIPCHK(reserve_all(E, 1, ctlq.d_ctl_world, ctlq.d_ctl_sat));
        if (wit >= 0) HIPCHK(reserve_all((size_t)W + 16, 0, ctlq.d_ctl_dist, ctlq.d_ctl_weid));
        const unsigned wb = (W + 255) / 256, bb = (unsigned)((nw + 255) / 256);
        auto set = [&](int slot) { return ctlq.d_ctl_sets.p + (size_t)slot * nw; };
        const unsigned long long *fin = set(n_slots);
        std::vector<uint8_t> used((size_t)n_slots, 0);
        auto take = [&](int &slot) -> int {
            for (slot = 0; slot < n_slots; slot++)
                if (!used[(size_t)slot]) {
                    used[(size_t)slot] = 1;
                    return STCSP_OK;
                }
            return fail(STCSP_E_INTERNAL, "ctl: more than the %d set slots measured", n_slots);
        };
        HIPCHK(run.begin());
        if (int rc = csr_fill()) return rc;
        const uint32_t *csrc = csr.src.p, *cdst = csr.dst.p, *ceid = csr.eid.p;
        hipLaunchKernelGGL(k_ctl_fin, dim3(wb), dim3(256), 0, v.stream, W, cdst, (const uint8_t *)post.d_pfinal.p, set(n_slots));
        HIPCHK(hipMemsetAsync(ctlq.d_ctl_some.p, 0, 2 * (size_t)S, v.stream));
        if (!words_h.empty()) HIPCHK(hipMemcpyAsync(ctlq.d_ctl_prog.p, words_h.data(), words_h.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
        launches += 2;
        int parity = 0;  // which half of some[] the next sweep marks; the other half is the one its second launch clears
        // one sweep: EX of `from`, combined into `to` (k_ctl_pre); two launches
        auto sweep = [&](int from, const unsigned long long *f, int or_old, int to, uint32_t *dist, uint32_t level) {
            uint8_t *mark = ctlq.d_ctl_some.p + (size_t)parity * S, *other = ctlq.d_ctl_some.p + (size_t)(parity ^ 1) * S;
            hipLaunchKernelGGL(k_ctl_mark, dim3(wb), dim3(256), 0, v.stream, W, csrc, (const unsigned long long *)set(from), mark);
            hipLaunchKernelGGL(k_ctl_pre, dim3(wb), dim3(256), 0, v.stream, W, csrc, cdst, (const uint8_t *)mark, other, f, or_old, set(to), dist, level,
                               ctlq.d_ctl_ctl.p);
            parity ^= 1;
            sweeps++;
            launches += 2;
        };
        auto boolean = [&](int op, int a, int b, int to) {
            hipLaunchKernelGGL(k_ctl_bool, dim3(bb), dim3(256), 0, v.stream, W, op, (const unsigned long long *)set(a), (const unsigned long long *)set(b), set(to));
            launches++;
        };
        // z = the least fixpoint of z | (f & EX z): sweep i is level i + 1; *levels: the sweeps run
        auto until = [&](int f, int z, uint32_t *dist, uint32_t *levels) -> int {
            return batched_fixpoint(run, CTL_CHANGED, W + 8, "ctl: an EU fixpoint did not converge in %u rounds", [&](uint32_t i) -> int {
                sweep(z, set(f), 1, z, dist, i + 1);
                if (levels) *levels = i + 1;
                return STCSP_OK;
            });
        };
        // the witness walk, at the node it belongs to (the ! above it works in place afterwards)
        auto walk = [&](uint32_t max_len, const uint32_t *dist, const unsigned long long *set_a, const unsigned long long *set_b) -> int {
            std::vector<uint32_t> weid(max_len);
            HIPCHK(run.begin());
            hipLaunchKernelGGL(k_ctl_walk, dim3(1), dim3(64), 0, v.stream, W, N, max_len, (const uint32_t *)csr.off.p, cdst, ceid, dist, set_a, set_b, v.d_oval,
                               ctlq.d_ctl_weid.p, ctlq.d_ctl_ctl.p);
            launches++;
            HIPCHK(hipMemcpyAsync(weid.data(), ctlq.d_ctl_weid.p, (size_t)max_len * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
            HIPCHK(run.flush());
            if (cw[CTL_DUPLICATE]) return fail(STCSP_E_INTERNAL, "ctl: two worlds out of state %u carry the same full row", cw[CTL_DUPLICATE] - 1);
            if (cw[CTL_STUCK]) return fail(STCSP_E_INTERNAL, "ctl: the witness walk stops at state %u", cw[CTL_STUCK] - 1);
            const uint32_t len = cw[CTL_WITNESS_LEN];
            if (len > max_len) return fail(STCSP_E_INTERNAL, "ctl: a witness of %u worlds, %u at the most", len, max_len);
            if (int rc = walked_rows(weid.data(), len, "ctl: the witness names edge %u of %u", ctlq.ctl_witness)) return rc;
            witness_len = (int32_t)len;
            if (len) witness_kind = negated ? STCSP_CTL_IS_COUNTEREXAMPLE : STCSP_CTL_IS_WITNESS;
            return STCSP_OK;
        };
        // the set of node r into a slot it takes
        auto eval = [&](auto &&self, int32_t r, int &slot) -> int {
            const CtlNode &n = prog.nodes[(size_t)r];
            if (!n.temporal) {
                if (int rc = take(slot)) return rc;
                hipLaunchKernelGGL(k_ctl_pred, dim3(wb), dim3(256), 0, v.stream, W, N, ceid, v.d_oval, (const int32_t *)ctlq.d_ctl_prog.p + slice_off[(size_t)r],
                                   (int)slice_len[(size_t)r], set(slot));
                launches++;
                return STCSP_OK;
            }
            int a = -1, b = -1;
            if (int rc = self(self, n.a, a)) return rc;
            if (n.b >= 0)
                if (int rc = self(self, n.b, b)) return rc;
            slot = a;
            switch (n.kind) {
            case STCSP_CTL_NOT: boolean(CTL_B_NOT, a, a, a); return STCSP_OK;
            case STCSP_CTL_AND:
            case STCSP_CTL_OR:
                boolean(n.kind == STCSP_CTL_AND ? CTL_B_AND : CTL_B_OR, a, b, a);
                used[(size_t)b] = 0;
                return STCSP_OK;
            case STCSP_CTL_EX:
                if (r != wit) {
                    sweep(a, nullptr, 0, a, nullptr, 0);
                    return STCSP_OK;
                }
                if (int rc = take(slot)) return rc;
                boolean(CTL_B_COPY, a, a, slot);  // (the second launch compares with what the target holds)
                sweep(a, nullptr, 0, slot, nullptr, 0);
                used[(size_t)a] = 0;
                return walk(2, nullptr, set(slot), set(a));
            case STCSP_CTL_EU: {
                slot = b;
                uint32_t levels = 0;
                uint32_t *dist = r == wit ? ctlq.d_ctl_dist.p : nullptr;
                if (dist) {
                    hipLaunchKernelGGL(k_ctl_dist_init, dim3(wb), dim3(256), 0, v.stream, W, (const unsigned long long *)set(b), dist);
                    launches++;
                }
                if (int rc = until(a, b, dist, &levels)) return rc;
                used[(size_t)a] = 0;
                return dist ? walk(std::min<uint32_t>(levels + 1, W + 16), dist, nullptr, nullptr) : (int)STCSP_OK;
            }
            default: {  // EG, Emerson-Lei: z = f & EX E[f U (z & Fin)] from z = f down
                int z = -1, t = -1;
                if (int rc = take(z)) return rc;
                if (int rc = take(t)) return rc;
                boolean(CTL_B_COPY, a, a, z);
                for (int32_t round = 1;; round++) {
                    most_outer = std::max(most_outer, round);
                    hipLaunchKernelGGL(k_ctl_bool, dim3(bb), dim3(256), 0, v.stream, W, (int)CTL_B_AND, (const unsigned long long *)set(z), fin, set(t));
                    launches++;
                    if (int rc = until(a, t, nullptr, nullptr)) return rc;
                    HIPCHK(run.begin());
                    HIPCHK(hipMemsetAsync(ctlq.d_ctl_ctl.p + CTL_CHANGED, 0, sizeof(uint32_t), v.stream));
                    sweep(t, set(a), 0, z, nullptr, 0);
                    HIPCHK(run.flush());
                    if (!cw[CTL_CHANGED]) break;
                    if ((uint32_t)round > W + 8) return fail(STCSP_E_INTERNAL, "ctl: an EG fixpoint did not converge in %d rounds", round);
                }
                used[(size_t)a] = used[(size_t)t] = 0;
                slot = z;
                return STCSP_OK;
            }
            }
        };
        int top = -1;
        if (int rc = eval(eval, prog.root, top)) return rc;
        HIPCHK(run.begin());
        HIPCHK(hipMemsetAsync(ctlq.d_ctl_world.p, 0, E, v.stream));
        HIPCHK(hipMemsetAsync(ctlq.d_ctl_sat.p, 0, E, v.stream));
        HIPCHK(hipMemsetAsync(ctlq.d_ctl_ctl.p, 0, sizeof cw, v.stream));
        hipLaunchKernelGGL(k_ctl_scatter, dim3(wb), dim3(256), 0, v.stream, W, csrc, ceid, (const unsigned long long *)set(top), ctlq.d_ctl_world.p, ctlq.d_ctl_sat.p,
                           ctlq.d_ctl_ctl.p);
        launches++;
        HIPCHK(hipMemcpyAsync(ctlq.ctl_world.data(), ctlq.d_ctl_world.p, E, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(hipMemcpyAsync(ctlq.ctl_sat.data(), ctlq.d_ctl_sat.p, E, hipMemcpyDeviceToHost, v.stream));
        HIPCHK(run.flush());
    }
    ctlq.ctl_world.reserve(1);
    ctlq.ctl_sat.reserve(1);
    ctlq.ctl_witness.reserve(1);
    memset(out, 0, sizeof *out);
    out->n_worlds = W;
    out->n_initial = W ? cw[CTL_INITIAL] : 0;
    out->n_initial_sat = W ? cw[CTL_INITIAL_SAT] : 0;
    out->n_edges = E;
    out->edge_world = ctlq.ctl_world.data();
    out->edge_sat = ctlq.ctl_sat.data();
    out->witness_values = ctlq.ctl_witness.data();
    out->witness_kind = witness_kind;
    out->witness_len = witness_len;
    out->n_vars = N;
    out->rounds[0] = sweeps;
    out->rounds[1] = most_outer;
    out->rounds[2] = launches;
    out->seconds_kernels = run.ms * 1e-3;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return STCSP_OK;
}

}  // namespace stcsp
