// automaton.hpp -- what engine.hip sees of the services on the exported automaton (automaton.hip)
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "compare_host.hpp"
#include "hip_host.hpp"

namespace stcsp {

namespace dev { struct BatchStream; struct ObsRec; }
struct HostMonitor;

// what the engine hands a service call: the last export and the facts of model and solve the services read. Valid for the call only.
struct AutomatonView {
    hipStream_t stream;  // the engine's: a service is ordered after the export
    int N, KL;
    uint32_t n_states;
    size_t exp_edges;
    const long long *d_osrc, *d_odst;  // [exp_edges]
    const int32_t *d_oval;             // [exp_edges][N]
    const uint32_t *d_state_keys;      // [n_states][KL]
    const long long *h_osrc, *h_odst;  // the pinned host copies
    const int32_t *h_oval;
    const int *lb, *ub;  // [N] the variables' bounds
    int n_sig, n_until, n_until_cons;
    const uint8_t *default_observable;  // [N]
    bool sharded, truncated, exp_on_device;
    std::string *err;  // where a failing call leaves its message
};

struct AutomatonServices {
    AutomatonServices();  // (both out of line: HostMonitor is incomplete here)
    ~AutomatonServices();
    AutomatonServices(const AutomatonServices &) = delete;  // (it owns device memory, and lab / dict / obsv / cmp below refer into it)
    AutomatonServices &operator=(const AutomatonServices &) = delete;
    void invalidate();     // a new solve, a new export or new flags: everything derived from the old ones is dropped
    int postprocess(const AutomatonView &view, const stcsp_post_options *po, stcsp_post_result *out);
    int quotient(const AutomatonView &view, const stcsp_quotient_options *qo, stcsp_quotient_result *out);
    int monitor_build(const AutomatonView &view, const stcsp_monitor_options *mo, stcsp_monitor_info *info);
    int monitor_check(const AutomatonView &view, const stcsp_monitor_streams *ms, stcsp_monitor_result *out);
    int generator_build(const AutomatonView &view, const stcsp_generator_options *go, stcsp_generator_info *info);
    int generate(const AutomatonView &view, const stcsp_generate_request *rq, stcsp_generate_result *out);
    int repair(const AutomatonView &view, const stcsp_repair_request *rq, stcsp_repair_result *out);
    int align(const AutomatonView &view, const stcsp_align_request *rq, stcsp_align_result *out);
    int infer(const AutomatonView &view, const stcsp_infer_request *rq, stcsp_infer_result *out);
    int posterior(const AutomatonView &view, const stcsp_posterior_request *rq, stcsp_posterior_result *out);
    int observer(const AutomatonView &view, const stcsp_observer_options *oo, stcsp_observer_result *out);
    int compare(const AutomatonView &view, const stcsp_compare_request *rq, stcsp_compare_result *out);
    int components(const AutomatonView &view, const stcsp_components_options *co, stcsp_components_result *out);
    int optimise(const AutomatonView &view, const stcsp_optimise_request *rq, stcsp_optimise_result *out);
    int ctl(const AutomatonView &view, const stcsp_ctl_request *rq, stcsp_ctl_result *out);

private:
    enum Need { NEED_EXPORT, NEED_FLAGS, NEED_MONITOR, NEED_GENERATOR };
    struct Batch { size_t b0 = 0, b1 = 0, bytes = 0, entries = 0, steps = 0, longest = 0; };  // of plan_batch(): the streams [b0, b1)
    int fail(int code, const char *fmt, ...);
    int enter(const AutomatonView &view, const char *who, Need need, const char *host_twin);
    int live_set();
    int table_budget(const char *env_name, size_t &budget);
    template <typename NeedFn>
    int plan_batch(const char *who, const int64_t *offsets, size_t n, size_t b0, size_t budget, NeedFn need, std::vector<dev::BatchStream> &meta, Batch &b);
    template <typename Result, typename NeedFn, typename Body>
    int stream_batches(const char *who, const char *budget_env, int64_t n_streams, const int64_t *offsets, const int32_t *values, bool dictionaries,
                       NeedFn need, Result *out, Body body);
    // A timed batch of launches of a graph service (components, optimise, ctl): begin() before its launches (nothing while one is open);
    // flush() after them copies the service's control words to their host copy, waits, and adds the batch's time on the device to ms.
    struct LaunchBatch {
        hipStream_t stream;
        DevEvents &ev;  // [0], [1]
        uint32_t *d_ctl, *h_ctl;
        size_t words;
        double ms = 0;
        bool open = false;
        hipError_t begin(), flush();
    };
    static constexpr int kBatch = 4;  // the sweeps of a fixpoint between two looks at the changed word
    template <typename Step>
    int batched_fixpoint(LaunchBatch &run, int changed, uint32_t bound, const char *diverged, Step step);
    int csr_count(LaunchBatch &run, const uint8_t *states, const char *too_many, uint32_t &count), csr_fill();
    int walked_rows(const uint32_t *eid, size_t n, const char *past_export, std::vector<int32_t> &rows);
    template <typename... Tables>
    int reserve_tables(const char *who, size_t bytes, Tables &&...tables);
    // the two argument lists the stream kernels share, cast once: the generator's CSR with the label id of every position ...
    struct SweepCsr { const uint32_t *off, *lid, *dstp, *eid; };
    // ... and what gives the projected row of a label: values[rep[l] * N + obs[v]]
    struct LabelRows { const uint32_t *rep; const int32_t *values; int N; const int32_t *obs; int n_obs; };
    SweepCsr sweep_csr() const { return {gen.d_goff.p, gen.lab.d_rlid.p, gen.d_gdst.p, gen.d_geid.p}; }
    LabelRows label_rows() const { return {gen.lab.d_rrep.p, v.d_oval, v.N, gen.d_gobs.p, gen.n_obs}; }
    int repair_labels();
    int infer_dictionaries();
    int observer_order(double &seconds);
    template <typename T>
    int grow_keeping(DevBuf<T> &buf, size_t keep, size_t count, const char *who = "observer");

    AutomatonView v{};  // of the call that is running: its pointers are the engine's, not to be used after it
    DevEvents ev;     // (every call waits for its own work: one set serves them all)
    // What a group is derived from is where it stands: invalidate() drops the flags, the monitor and the generator; the generator
    // holds what is built on its CSR (labels, then dictionaries and the observer, then the comparison's left operand) and drops
    // all of it in drop_derived(), its one drop point. The groups without a flag live for one call; their vectors back the
    // result until the next call.
    struct Flags {  // post-processing (dev_postproc.hpp): the flags of the last postprocess(), valid while done; and the live set (the
        // valid states reachable from the root over alive edges), computed on first need after a postprocess(), valid while live_done
        bool done = false, live_done = false, root_live = false;
        int64_t n_live = 0;
        DevBuf<uint8_t> d_pvalid, d_pfinal, d_palive, d_pnodeok, d_live;
        DevBuf<uint32_t> d_pcover, d_pctl, d_lctl;
        std::vector<uint8_t> p_valid, p_final, p_alive, live;
    } post;
    struct Quotient {  // bisimulation quotient (dev_quotient.hpp)
        DevBuf<int32_t> d_qobs;
        DevBuf<uint32_t> d_qsrc, d_qdst, d_qlid, d_qcls[2], d_qcnt, d_qtab_e, d_qtab_s, d_qctl;
        DevBuf<unsigned long long> d_qacc[2];
        std::vector<int32_t> q_class;
        std::vector<uint32_t> q_raw, q_cnt;
    } quo;
    struct Monitor {  // stream monitor (dev_monitor.hpp): the look-up structures of the last monitor_build(), valid while built
        bool built = false;
        int n_obs = 0, max_dst = 0;
        uint32_t mask = 0;
        std::vector<uint8_t> observable, m_fin;
        std::unique_ptr<HostMonitor> host;  // built when the first stream falls back to the host twin
        DevBuf<uint8_t> d_mfin;
        DevBuf<int32_t> d_mobs, d_mrows, d_macc, d_mnend;
        DevBuf<uint32_t> d_mltab, d_mhead, d_mdst0, d_mdst, d_mnext, d_mctl, d_mlid;
        DevBuf<unsigned long long> d_mkeys;
        DevBuf<long long> d_moff;
        std::vector<int32_t> m_acc, m_nend;
    } mon;
    struct Labels {  // (dev_repair.hpp) label ids per position of the generator's CSR, built by the first service that asks
        bool built = false;
        uint32_t n_labels = 0, n_long = 0, total = 0, wave_segment = 0;
        DevBuf<uint32_t> d_rtab, d_rlid, d_rrep, d_rlong, d_rctl;
    };
    struct Dictionaries {  // (dev_infer.hpp) the value dictionaries of the labels, built by the first infer() or posterior()
        bool built = false;
        uint32_t words = 0;                        // bitmap words per step: the sum over the variables
        size_t n_values = 0;                       // ... and the dictionary entries (the posterior's bins)
        std::vector<std::vector<int32_t>> values;  // [n_obs] the sorted distinct values the labels carry
        std::vector<uint32_t> word_off, bin_off;   // [n_obs] first bitmap word of a variable, and first of its entries among all
        DevBuf<uint32_t> d_ividx, d_iwoff;
        DevBuf<int32_t> d_ilabrows;
    };
    struct Observer {  // (dev_observer.hpp) the out-edges ordered by (label rank, destination) and the label rows in rank order,
        // built by the first observer(); everything else lives for one call
        bool built = false;
        uint32_t max_deg = 0;
        std::vector<int32_t> rows;  // [n_labels][n_obs], sorted
        DevBuf<unsigned long long> d_okey, d_oitab, d_oitems, d_ostab, d_ostab2, d_okeys, d_owhere;
        DevBuf<uint32_t> d_olrank, d_octl, d_opool, d_ossid, d_ossid2, d_oslot, d_oesrc, d_oelab, d_oedst, d_ocanon, d_oscratch;
        DevBuf<dev::ObsRec> d_orec;
        DevBuf<int32_t> d_omember;
        std::vector<int64_t> o_moff;
        std::vector<int32_t> o_member, o_esrc, o_edst, o_evalues;
        std::vector<uint8_t> o_final;
    };
    struct Comparison {  // (dev_compare.hpp) the left operand is the observer of the last successful observer(), kept on the host
        // while valid and, from the first compare() on, as CSR in HBM while left_on_device; everything else lives for one call
        bool valid = false, left_on_device = false;
        CompareOperand left;
        DevBuf<uint32_t> d_cloff, d_cllab, d_cldst, d_croff, d_crlab, d_crdst, d_cnew, d_crank, d_cparent, d_cplabel, d_cctl;
        DevBuf<uint8_t> d_clfin, d_crfin;
        DevBuf<unsigned long long> d_ctab, d_ctab2, d_cmin, d_ckeys, d_cpkey;
        std::vector<int32_t> c_witness;
        std::vector<uint32_t> c_rank;
    };
    struct Generator {  // stream generator (dev_generate.hpp): the structures of the last generator_build(), valid while built
        bool built = false;
        int n_obs = 0, horizon = 0;
        std::vector<double> count;
        DevBuf<uint8_t> d_gfin;
        DevBuf<int32_t> d_gobs, d_gout;
        DevBuf<uint32_t> d_goff, d_gcur, d_gseg, d_geid, d_gdst, d_gtile, d_gctl;
        DevBuf<double> d_gw, d_gcount;
        DevBuf<unsigned long long> d_granks;
        std::vector<int32_t> g_values;
        std::vector<uint8_t> g_fin;
        Labels lab;         // on the CSR
        Dictionaries dict;  // on the labels
        Observer obs;       // on the labels
        Comparison cmp;     // on the observer
        void drop_derived() { lab.built = dict.built = obs.built = cmp.valid = false; }
    } gen;
    // short names for the four inside gen, in automaton.hip
    Labels &lab = gen.lab;
    Dictionaries &dict = gen.dict;
    Observer &obsv = gen.obs;
    Comparison &cmp = gen.cmp;
    struct Batches {  // the stream records and observed rows of the batch stream_batches() is at
        DevBuf<dev::BatchStream> d_streams;
        DevBuf<int32_t> d_rows;
    } bat;
    struct Repair {  // stream repair (dev_repair.hpp)
        DevBuf<uint32_t> d_rG, d_rcost;
        DevBuf<int32_t> d_rweights, d_rout, d_rdist, d_rnchg;
        DevBuf<uint8_t> d_rfin;
        std::vector<int32_t> r_dist, r_values, r_nchg;
        std::vector<uint8_t> r_fin;
    } rep;
    struct Align {  // stream alignment (dev_align.hpp): nothing is kept between calls; the vectors back the result
        DevBuf<uint32_t> d_aG, d_acost, d_actl;
        DevBuf<int32_t> d_aweights, d_aout, d_adist, d_anrows, d_anops, d_anchg, d_anskip, d_anins;
        DevBuf<uint8_t> d_aops, d_afin;
        DevBuf<long long> d_aroom;
        uint32_t *h_ctl = nullptr;  // pinned, A_WORDS: where the host reads the changed word of a group of sweeps
        std::vector<int32_t> a_dist, a_values, a_nchg, a_nskip, a_nins;
        std::vector<int64_t> a_ooff, a_poff;
        std::vector<uint8_t> a_ops, a_fin;
    } aln;
    struct Infer {  // stream inference (dev_infer.hpp)
        DevBuf<uint32_t> d_ibits, d_ictl;
        DevBuf<double> d_iB, d_icount;
        DevBuf<uint8_t> d_iF, d_imatch, d_ifeas, d_ifin;
        DevBuf<int32_t> d_iout, d_instates;
        DevBuf<unsigned long long> d_iranks;
        std::vector<double> i_count;
        std::vector<uint8_t> i_feas, i_fin;
        std::vector<int64_t> i_soff;
        std::vector<int32_t> i_sval, i_nstates, i_values;
        std::vector<uint32_t> i_bits;
    } inf;
    struct Posterior {  // posterior marginals (dev_posterior.hpp)
        DevBuf<double> d_yB, d_yw, d_ywbin, d_ymass;
        DevBuf<unsigned long long> d_yA, d_ylab, d_ybins, d_yfmass;
        DevBuf<uint8_t> d_ymatch, d_yexact;
        DevBuf<uint32_t> d_yboff;
        std::vector<double> y_mass;
        std::vector<uint8_t> y_exact, y_feas;
        std::vector<uint64_t> y_fmass, y_mmass;
        std::vector<unsigned long long> y_bins;
        std::vector<int64_t> y_moff;
        std::vector<int32_t> y_mval;
    } pos;
    // The live edges as 32-bit CSR by source (dev_csr.hpp), for the graph services. It lives for one call: csr_count() and
    // csr_fill() build it anew, under the state filter of the caller, and nothing reads it after the call returns. optimise(mean)
    // and ctl() run components() first, which builds and uses its CSR to the end; they then build their own into this same
    // group (ctl under scc.d_somega, which stays in scc). No call may rely on the CSR an earlier call left here.
    struct LiveCsr {
        DevBuf<uint32_t> deg, off, cur, src, dst, eid;  // [S + 1] out-degrees, offsets, fill cursors; [n] source, destination, export index
        const uint8_t *states = nullptr;                // the filter csr_count() ran under, for csr_fill()
        uint32_t n = 0;                                 // positions: off[S]
    } csr;
    struct Components {  // components (dev_components.hpp); d_sin / d_sout: the has_in / has_out marks of the trim rounds, arrays of their own
        DevBuf<uint32_t> d_scomp, d_scolour, d_sin, d_sout, d_sdepth, d_sdist, d_sinfo, d_ssel, d_sctl;
        DevBuf<uint8_t> d_somega;
        DevBuf<unsigned long long> d_smark;
        std::vector<int32_t> s_component, s_size, s_depth, s_flags, s_lcomp, s_lstem, s_lvalues;
        std::vector<uint8_t> s_omega;
        std::vector<int64_t> s_loff;
    } scc;
    struct Optimise {  // optimisation (dev_optimise.hpp)
        DevBuf<uint32_t> d_opt_weid, d_opt_wstate, d_opt_ctl;
        DevBuf<uint32_t> d_opt_nof, d_opt_comp, d_opt_least, d_opt_den, d_opt_arg;
        DevBuf<int32_t> d_opt_w, d_opt_len;
        DevBuf<long long> d_opt_cost, d_opt_rows, d_opt_best, d_opt_woff, d_opt_d, d_opt_dn, d_opt_num;
        std::vector<int64_t> opt_best, opt_state_best, opt_woff, opt_num, opt_den;
        std::vector<int32_t> opt_wvalues, opt_wstates, opt_component;
    } opt;
    struct Ctl {  // fair CTL (dev_ctl.hpp): nothing is kept between calls; the vectors back the result
        DevBuf<uint32_t> d_ctl_dist, d_ctl_weid, d_ctl_ctl;
        DevBuf<unsigned long long> d_ctl_sets;  // the set slots, then Fin
        DevBuf<uint8_t> d_ctl_some, d_ctl_world, d_ctl_sat;
        DevBuf<int32_t> d_ctl_prog;
        std::vector<uint8_t> ctl_world, ctl_sat;
        std::vector<int32_t> ctl_witness;
    } ctlq;
};

}  // namespace stcsp
