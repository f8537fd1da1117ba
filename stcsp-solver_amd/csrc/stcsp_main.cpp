// stcsp_main.cpp -- the `stcsp` command line, functionally as the reference's
// (src/stcsp.y:180-219 main, src/solver.cpp:195-359 solve): same flags, same stdout contract,
// same solutions.dot. The search itself runs on the MI355X engine behind the C-ABI.
//
//   stcsp [-s] [-m<sec>] [-t] [-a] [-z] [-k<K>] [-l<level>] [--binary=<file>] [--shards=<N>] [--intervals] [--quotient[=all]] [--observer[=all|NAME[,NAME...]] [--compare=<file>]] [--components[=bottom|all|<N>]] [--optimise=<spec>] [--ctl=<formula>] [--check=<file>]
//         [--sample=<N>:<L>[:<seed>] [--sample-final] [--sample-mask=all]] [--count=<L>]
//         [--repair=<file> [--repair-final]] [--align=<file> [--align-costs=<skip>:<gap>] [--align-final]] [--infer=<file> [--infer-final] [--infer-draws=<D>[:<seed>]]]
//         [--posterior=<file> [--posterior-final] [--posterior-weights=<name>=<value>:<weight>[,...]]] input.csp
//
// --observer (not in the reference) writes the observer of the automaton instead of the automaton itself, to solutions.dot and
// --binary=: the deterministic automaton whose states are the sets of states the system can be in after an observed prefix
// (include/stcsp_engine.h, stcsp_engine_observer). Observable are the variables whose name does not start with "_V";
// --observer=all makes every variable observable, --observer=NAME[,NAME...] the named ones only. The stdout line is unchanged;
// "observer: <live states> -> <states> states, <edges> edges" goes to stderr. The construction runs on the device for an unsharded
// solve and by the host twin otherwise (--shards=N, host adversarial passes). With --quotient the observer is then folded by the
// host bisimulation under the same mask (--quotient=all is not taken with it): the minimal deterministic automaton of the observable language, which
// --quotient alone cannot promise.
// --components[=bottom|all|<N>] (not in the reference) prints to stderr what the automaton says about INFINITE solutions
// (include/stcsp_engine.h, stcsp_engine_components): a line of counts that ends in "infinite solution: yes|no", one line per strongly
// connected component (number, size, depth, flags: C cyclic, F final, B bottom, A accepting) and, asked for with =all, =bottom (the
// bottom accepting components only) or =<N> (the first N), lasso solutions stem . loop^omega: a line "# name name ..." of the
// variables of the default mask, then per lasso the lines "stem:" and "loop:", the rows in the format --check= reads, separated by
// ';'. stdout and the written files are unchanged. On the device for an unsharded solve, by the host twin otherwise.
//
// --optimise=min|max:NAME=W[,NAME=W...][:HORIZON][:mean] (not in the reference) says which solution is best under the cost
// sum of W * NAME per step (include/stcsp_engine.h, stcsp_engine_optimise; the variables not named weigh 0; HORIZON 0 when left
// out). To stderr: a line "optimise: best[L] = <cost>" (or "none") for L = 0 .. HORIZON; when there is a prefix of HORIZON steps, a
// line "optimise: # name name ..." of the variables of the default mask and a line "optimise: witness:" with the lexicographically
// least best prefix, the rows in the format --check= reads, separated by ';'; with mean a line "optimise: component <c>: mean
// <num>/<den>" per cyclic component and "optimise: omega: mean <num>/<den> in component <c>" (or "optimise: omega: none"), the
// infimum of the long-run mean cost over the infinite solutions. stdout and the written files are unchanged. On the device for an
// unsharded solve, by the host twin otherwise.
//
// --ctl=<formula> (not in the reference) asks a temporal question about the INFINITE solutions in fair CTL (include/stcsp_engine.h,
// stcsp_engine_ctl; the grammar: include/stcsp_host.h, stcsp_ctl_parse), e.g. --ctl='AG EF m == 0'. To stderr: a line "ctl: <n> steps
// on infinite solutions, holds at <k> of <n> first steps: yes|no|vacuous" and, where the contract gives one, a line "ctl: # name
// name ..." of the variables of the default mask and a line "ctl: witness:" or "ctl: counterexample:" with the rows in the format
// --check= reads, separated by ';'. A formula that does not parse ends the run with status 1 and "--ctl: <position>: <message>"
// before anything is solved. stdout and the written files are unchanged. On the device for an unsharded solve, by the host twin
// otherwise.
//
// --compare=<file> (not in the reference; only together with --observer) compares what this model shows with what another one
// shows (include/stcsp_engine.h, stcsp_engine_compare). The file is a binary automaton written by --binary= of any run: it
// carries its variable names, the observable variables are matched by name (a name the file lacks is an error that says so),
// its observer under those variables is built by the host twin and its columns are put in this model's order. This model's
// observer is the left operand, the file's the right one. The comparison runs on the device for an unsharded solve and by the
// host twin otherwise. Five lines go to stderr, "compare: <pairs> pairs, <edges> edges, <levels> levels" and one per inclusion,
// "compare: <P|F>(<left|right>) in <P|F>(<right|left>): yes" or "...: no, <len> steps: v v ..; v v .." with the shortest stream
// that refutes it (P: the streams with a run, F: those whose run ends in a final state). stdout and the written automaton are
// unchanged.
// --binary=<file> (not in the reference) additionally writes the printed automaton in the compact
// binary form of include/stcsp_host.h.
// --shards=<N> (not in the reference, which is single-threaded) shards the open search frontier and the state table over N
// engines -- one per GPU of the node, round robin when there are fewer GPUs than shards -- driven by N host threads through
// stcsp_engine_solve_sharded() and the in-process transport (include/stcsp_sharded.h: records move between the GPUs with
// hipMemcpyPeerAsync); the shards' automata are merged and post-processed on the host.
// --intervals (not in the reference) holds every variable as an interval, like the reference does (STCSP_F_INTERVAL_DOMAINS):
// domains of any width in [INT_MIN, INT_MAX], where the default bitset domains take at most 128 values. Works with --shards=N.
// --quotient (not in the reference) writes the bisimulation quotient of the automaton instead of the automaton itself: the states
// that accept the same language over the observable variables are folded into one (include/stcsp_engine.h). Observable are the
// variables whose name does not start with "_V"; --quotient=all makes every variable observable (the automaton is then deterministic
// and the quotient is its minimal form). The stdout line is unchanged; "quotient: <live states> -> <classes>" goes to stderr. The
// partition is computed on the device, or by the host twin where the flags live on the host (--shards=N, host adversarial passes).
// When an -a / -z variable is wider than the device post-processing passes take, the host passes run instead.
//
// --check=<file> (not in the reference) checks observed streams against the automaton: which prefix of each stream is a prefix
// of a solution (include/stcsp_engine.h, stcsp_engine_monitor_check). The file is text: its first line "# name name ..." names
// the observable variables, one column each, and thereby sets the mask; then one step per line, and a blank line ends a stream
// (two blank lines in a row give an empty stream). stdout then holds one line per stream and nothing else,
//     index accepted_len len n_end end_final
// and the reference's statistics line (and "adver1: ..." of -a / -z) goes to stderr. The streams are checked on the device, or
// by the host twin where the flags live on the host (--shards=N, host adversarial passes); with -a / -z the flags are the ones
// those passes left. Combined with --quotient the streams are checked against the automaton before it is folded.
//
// --sample=<N>:<L>[:<seed>] (not in the reference) prints N sampled solution prefixes of L steps (include/stcsp_engine.h,
// stcsp_engine_generate; seed 0 when left out) in exactly the format --check= reads: the line "# name name ..." names the
// observable variables -- the default mask, or every variable with --sample-mask=all -- then one step per line, and a blank line
// ends each stream, so the output can be fed straight back into --check=. --count=<L> prints "t count[t]" for t = 0 .. L instead:
// the number of solution prefixes of every length. With --sample-final both take only the prefixes that end in a final state.
// As with --check, stdout then holds these lines only, and the work is done on the device, or by the host twin where the flags
// live on the host (--shards=N, host adversarial passes). --check, --sample and --count exclude each other.
//
// --repair=<file> (not in the reference) repairs observed streams: for each stream of the file, which has the format of --check=
// and sets the mask by its first line, the nearest prefix of a solution and its distance (include/stcsp_engine.h,
// stcsp_engine_repair; every weight 1). A token "?" is a value that was not observed. stdout holds the repaired streams in
// exactly the format --check= reads, each one preceded by the comment line
//     # index distance <d> len <len> n_changed <k> end_final <f>
// (--check= skips lines that start with '#' after the first, so the output can be fed straight back into it); a stream without
// a solution prefix of its length has distance -1 and prints that line and a blank line only. --repair-final asks for prefixes
// that end in a final state. The work is done on the device, or by the host twin where the flags live on the host (--shards=N,
// host adversarial passes). --repair excludes --check, --sample and --count.
//
// --align=<file> (not in the reference) aligns observed streams whose recorder may have lost or repeated steps: the weighted edit
// distance of each stream of the file (the format of --repair=, "?" = not observed) to the solution language, and the aligned solution
// prefix (include/stcsp_engine.h, stcsp_engine_align; every weight 1). --align-costs=<skip>:<gap> (default 1:1) prices a dropped
// observed step and an inserted solution step; --align-final asks for prefixes that end in a final state. For each stream stdout holds
//   # <index> distance <d> len <L> out_len <L2> n_changed <k> n_skipped <a> n_inserted <b> end_final <f> ops <MMDIM...>
// and the L2 emitted rows in the format --check= reads (M = matched, D = observed step dropped, I = solution step inserted). On the
// device after an unsharded solve, by the host twin otherwise. --align excludes --check, --repair, --infer, --posterior, --sample, --count.
//
// --infer=<file> (not in the reference) infers what the entries of partially observed streams that were not seen can be
// (include/stcsp_engine.h, stcsp_engine_infer). The file has the format of --repair=: "?" is a value that was not observed. For
// each stream stdout holds the comment line
//     # index count <c> len <len> feasible <f>
// where c is the number of solution prefixes consistent with the stream, then one comment line per step, "# {a,b,...} {...} ...":
// for every observable variable the sorted values it can take at that step. --infer-final counts only the prefixes that end in a
// final state. --infer-draws=<D>[:<seed>] prints, after the supports of a feasible stream, D sampled completions of it (seed 0 when
// left out), each followed by a blank line: every line that is no stream starts with '#', so the output can be fed straight into
// --check=. The work is done on the device for an unsharded solve, by the host twin otherwise (--shards=N, host adversarial
// passes). --infer excludes --check, --repair, --sample and --count.
//
// --posterior=<file> (not in the reference) says how many of the solution prefixes consistent with a partially observed stream
// give each value of an entry that was not seen (include/stcsp_engine.h, stcsp_engine_posterior). The file has the format of
// --repair=. For each stream stdout holds the comment line
//     # index mass <m> len <len> exact <e> final_mass <f>
// then one comment line per step, "# {a:m_a,b:m_b,...} {...} ...": for every observable variable the values it can take at that
// step, each with the mass of the consistent prefixes that give it. --posterior-final takes only the prefixes that end in a
// final state. --posterior-weights=x=1:3,y=0:0 weighs the value 1 of x by 3 and the value 0 of y by 0 (non-negative integers;
// a value that is not listed weighs 1; the variables must be among the file's). The work is done on the device for an unsharded
// solve, by the host twin otherwise. --posterior excludes --check, --repair, --infer, --sample and --count.
//
// Options must be glued to their value (-k3, not -k 3): like the reference, the first argument
// that does not start with '-' is the input file (stcsp.y:199-206).
#include <sys/times.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "stcsp_engine.h"
#include "stcsp_host.h"
#include "stcsp_sharded.h"

static double cpu_time() {  // cpuTime (util.cpp:149-155)
    struct tms b;
    times(&b);
    return (double)(b.tms_utime + b.tms_stime + b.tms_cutime + b.tms_cstime) / (double)sysconf(_SC_CLK_TCK);
}

struct Flags {
    bool print_solution = false, testing = false, adv1 = false, adv2 = false, intervals = false;
    bool quotient = false, quotient_all = false;
    bool observer = false;
    const char *observer_mask = "";  // "" (the default mask), "all" or NAME[,NAME...]
    const char *compare = nullptr;
    bool components = false;
    long long components_lassos = 0;  // 0 none, -1 all, n the first n
    bool components_bottom = false;
    const char *optimise = nullptr;  // the text after --optimise=
    const char *ctl = nullptr;       // the text after --ctl=
    int prefix_k = 2, time_limit = 0, shards = 1;
    const char *file = nullptr;
    const char *binary = nullptr;
    const char *check = nullptr;
    const char *repair = nullptr;
    bool repair_final = false;
    const char *align = nullptr;
    bool align_final = false;
    int align_skip = 1, align_gap = 1;
    const char *infer = nullptr;
    bool infer_final = false;
    int infer_draws = 0;
    long long infer_seed = 0;
    const char *posterior = nullptr;
    bool posterior_final = false;
    const char *posterior_weights = nullptr;  // the text after --posterior-weights=
    bool sample = false, sample_final = false, sample_all = false;
    long long sample_n = 0, sample_seed = 0;
    int sample_len = 0, count_len = -1;
    bool quiet() const { return check || repair || align || infer || posterior || sample || count_len >= 0; }  // stdout holds the answers only
    // the one streams file (the five options exclude each other) or NULL, and whether it may hold "?": all but --check's
    const char *streams_file(bool *missing_ok) const {
        *missing_ok = !check;
        return check ? check : repair ? repair : align ? align : infer ? infer : posterior;
    }
};

// --check=<file>, --repair=<file>, ...: the streams of the file, columns reordered to variable order
struct Streams {
    std::vector<uint8_t> mask;
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> values;
    size_t n() const { return offsets.size() - 1; }
    long long len(size_t i) const { return (long long)(offsets[i + 1] - offsets[i]); }
    size_t n_obs() const { return (size_t)std::count_if(mask.begin(), mask.end(), [](uint8_t m) { return m != 0; }); }
};

static int read_streams(const char *path, const stcsp_problem *p, Streams &out, bool missing_ok = false) {
    FILE *fp = fopen(path, "r");
    if (!fp) {
        fprintf(stderr, "cannot read %s\n", path);
        return 1;
    }
    out.mask.assign((size_t)p->n_vars, 0);
    std::vector<int> col_var, col_pos;  // variable of a column; position of a column in a row in variable order
    std::string line;
    bool header = false;
    int64_t steps = 0, lineno = 0;
    for (int c = 0; c != EOF;) {
        line.clear();
        while ((c = fgetc(fp)) != EOF && c != '\n') line.push_back((char)c);
        if (c == EOF && line.empty()) break;
        lineno++;
        std::vector<std::string> tok;
        for (size_t i = 0; i < line.size();) {
            while (i < line.size() && isspace((unsigned char)line[i])) i++;
            size_t j = i;
            while (j < line.size() && !isspace((unsigned char)line[j])) j++;
            if (j > i) tok.push_back(line.substr(i, j - i));
            i = j;
        }
        if (!header) {
            if (tok.empty() || tok[0] != "#") {
                fprintf(stderr, "%s: the first line must be \"# name name ...\"\n", path);
                fclose(fp);
                return 1;
            }
            for (size_t k = 1; k < tok.size(); k++) {
                int v = -1;
                for (int i = 0; i < p->n_vars; i++)
                    if (p->var_names && p->var_names[i] && tok[k] == p->var_names[i]) v = i;
                if (v < 0 || out.mask[(size_t)v]) {
                    fprintf(stderr, "%s: %s variable %s\n", path, v < 0 ? "unknown" : "repeated", tok[k].c_str());
                    fclose(fp);
                    return 1;
                }
                out.mask[(size_t)v] = 1;
                col_var.push_back(v);
            }
            for (int v : col_var) {
                int pos = 0;
                for (int i = 0; i < v; i++) pos += out.mask[(size_t)i];
                col_pos.push_back(pos);
            }
            header = true;
            continue;
        }
        if (!tok.empty() && tok[0][0] == '#') continue;  // a comment (--repair writes one per stream)
        if (tok.empty()) {  // a blank line ends the stream
            out.offsets.push_back(steps);
            continue;
        }
        if (tok.size() != col_var.size()) {
            fprintf(stderr, "%s:%lld: expected %zu values\n", path, (long long)lineno, col_var.size());
            fclose(fp);
            return 1;
        }
        const size_t base = out.values.size();
        out.values.resize(base + col_var.size());
        for (size_t k = 0; k < tok.size(); k++) {
            if (missing_ok && tok[k] == "?") {
                out.values[base + (size_t)col_pos[k]] = STCSP_REPAIR_MISSING;
                continue;
            }
            char *end = nullptr;
            const long long x = strtoll(tok[k].c_str(), &end, 10);
            if (end == tok[k].c_str() || *end || x < INT32_MIN || x > INT32_MAX) {
                fprintf(stderr, "%s:%lld: not an int32: %s\n", path, (long long)lineno, tok[k].c_str());
                fclose(fp);
                return 1;
            }
            out.values[base + (size_t)col_pos[k]] = (int32_t)x;
        }
        steps++;
    }
    fclose(fp);
    if (!header) {
        fprintf(stderr, "%s: the first line must be \"# name name ...\"\n", path);
        return 1;
    }
    if (steps > out.offsets.back()) out.offsets.push_back(steps);
    return 0;
}

// ---- what the printers share
// the default mask: the variables whose name does not start with "_V"
static bool in_default_mask(const stcsp_problem *p, int v) { return !(p->var_names && p->var_names[v] && strncmp(p->var_names[v], "_V", 2) == 0); }
static bool is_observable(const stcsp_problem *p, const uint8_t *mask, int v) { return mask ? mask[v] != 0 : in_default_mask(p, v); }

// the line "# name name ..." of the variables of `mask` (NULL: the default mask); returns their number
static size_t print_header(FILE *out, const stcsp_problem *p, const uint8_t *mask) {
    size_t n_obs = 0;
    fprintf(out, "#");
    for (int v = 0; v < p->n_vars; v++)
        if (is_observable(p, mask, v)) {
            fprintf(out, " %s", p->var_names[v]);
            n_obs++;
        }
    fprintf(out, "\n");
    return n_obs;
}

// one step of a stream in the format --check= reads
static void print_row(FILE *out, const int32_t *row, size_t n_obs) {
    for (size_t k = 0; k < n_obs; k++) fprintf(out, k ? " %d" : "%d", row[k]);
    fprintf(out, "\n");
}

// the steps b .. e of rows over all `n_vars` variables as one line " v v; v v": the variables of the default mask
static void print_steps(FILE *out, const stcsp_problem *p, const int32_t *values, int64_t n_vars, int64_t b, int64_t e) {
    for (int64_t t = b; t < e; t++) {
        if (t > b) fprintf(out, ";");
        for (int v = 0; v < p->n_vars; v++)
            if (in_default_mask(p, v)) fprintf(out, " %d", values[t * n_vars + v]);
    }
    fprintf(out, "\n");
}

// ---- the services. Each is one function: with `eng` (a finished postprocess()) it runs on the device, over the flags postprocess()
// has just left, and with eng NULL by the host twin on `a`'s current flags; one printer follows both. A service prints its own
// error, the engine's message on the device and a fixed sentence on the host, and returns non-zero.
static int engine_error(stcsp_engine *eng) {
    fprintf(stderr, "%s\n", stcsp_engine_last_error(eng));
    return 1;
}
static int host_error(const char *sentence) {
    fprintf(stderr, "%s\n", sentence);
    return 1;
}

// the stream services of the device run on the generator's structures under the streams' mask
static int build_generator(stcsp_engine *eng, const uint8_t *mask) {
    stcsp_generator_options go = {mask, 0, 0, {0, 0}};
    stcsp_generator_info gi;
    return stcsp_engine_generator_build(eng, &go, &gi);
}

// --check
static int check(const Flags &, const stcsp_problem *, const Streams &st, const stcsp_automaton *a, stcsp_engine *eng) {
    const stcsp_monitor_streams ms = {(int64_t)st.n(), st.offsets.data(), st.values.data(), 0, 0};
    stcsp_monitor_result r = {};
    std::vector<int32_t> acc, n_end;  // (the twin's output)
    std::vector<uint8_t> fin;
    if (eng) {
        stcsp_monitor_options mo = {st.mask.data(), {0, 0}};
        stcsp_monitor_info mi;
        if (stcsp_engine_monitor_build(eng, &mo, &mi) != STCSP_OK || stcsp_engine_monitor_check(eng, &ms, &r) != STCSP_OK) return engine_error(eng);
    } else {
        acc.resize(st.n() + 1), n_end.resize(st.n() + 1), fin.resize(st.n() + 1);
        if (stcsp_automaton_check_streams(a, st.mask.data(), ms.n_streams, ms.offsets, ms.values, acc.data(), n_end.data(), fin.data(), nullptr) != STCSP_OK)
            return host_error("the streams could not be checked");
        r.accepted_len = acc.data(), r.n_end = n_end.data(), r.end_final = fin.data();
    }
    for (size_t i = 0; i < st.n(); i++) printf("%zu %d %lld %d %d\n", i, r.accepted_len[i], st.len(i), r.n_end[i], (int)r.end_final[i]);
    fflush(stdout);
    return 0;
}

// --sample / --count
static void print_samples(const Flags &f, const stcsp_problem *p, const uint8_t *mask, const stcsp_generate_result &r) {
    const size_t n_obs = print_header(stdout, p, mask);
    for (long long i = 0; i < f.sample_n; i++) {
        for (int t = 0; t < f.sample_len; t++) print_row(stdout, r.values + ((size_t)i * (size_t)f.sample_len + (size_t)t) * n_obs, n_obs);
        printf("\n");
    }
    fflush(stdout);
}

static int generate(const Flags &f, const stcsp_problem *p, const stcsp_automaton *a, stcsp_engine *eng) {
    static const char *const failed = "the streams could not be generated: no solution prefix of that length, or their number overflows a double";
    const bool counting = f.count_len >= 0;
    const int32_t horizon = counting ? f.count_len : f.sample_len, flags = f.sample_final ? STCSP_GEN_END_FINAL : 0;
    std::vector<uint8_t> mask((size_t)p->n_vars, 1);
    for (int v = 0; v < p->n_vars; v++) mask[(size_t)v] = f.sample_all || in_default_mask(p, v);
    const double *count = nullptr;
    stcsp_generate_result r = {};
    std::vector<double> host_count;  // (the twin's output)
    std::vector<int32_t> values;
    std::vector<uint8_t> fin;
    if (eng) {
        stcsp_generator_options go = {mask.data(), horizon, flags, {0, 0}};
        stcsp_generator_info gi;
        if (stcsp_engine_generator_build(eng, &go, &gi) != STCSP_OK) return engine_error(eng);
        count = gi.count;
        stcsp_generate_request rq = {f.sample_n, nullptr, (uint64_t)f.sample_seed, f.sample_len, 0};
        if (!counting && stcsp_engine_generate(eng, &rq, &r) != STCSP_OK) return engine_error(eng);
    } else if (counting) {
        host_count.resize((size_t)horizon + 1);
        if (stcsp_automaton_count_streams(a, horizon, flags, host_count.data()) != STCSP_OK) return host_error(failed);
        count = host_count.data();
    } else {
        const size_t n_obs = (size_t)std::count(mask.begin(), mask.end(), 1);
        values.resize((size_t)f.sample_n * (size_t)f.sample_len * n_obs + 1), fin.resize((size_t)f.sample_n + 1);
        if (stcsp_automaton_generate(a, mask.data(), horizon, flags, f.sample_n, f.sample_len, (uint64_t)f.sample_seed, nullptr, nullptr, values.data(),
                                     fin.data()) != STCSP_OK)
            return host_error(failed);
        r.values = values.data(), r.end_final = fin.data();
    }
    if (counting) {
        for (int t = 0; t <= horizon; t++) printf("%d %.0f\n", t, count[t]);
        fflush(stdout);
    } else {
        print_samples(f, p, mask.data(), r);
    }
    return 0;
}

// --repair
static void print_repairs(const stcsp_problem *p, const Streams &st, const stcsp_repair_result &r) {
    const size_t n_obs = print_header(stdout, p, st.mask.data());
    for (size_t i = 0; i < st.n(); i++) {
        printf("# %zu distance %d len %lld n_changed %d end_final %d\n", i, r.distance[i], st.len(i), r.n_changed[i], (int)r.end_final[i]);
        for (int64_t t = st.offsets[i]; r.distance[i] >= 0 && t < st.offsets[i + 1]; t++) print_row(stdout, r.values + (size_t)t * n_obs, n_obs);
        printf("\n");
    }
    fflush(stdout);
}

static int repair(const Flags &f, const stcsp_problem *p, const Streams &st, const stcsp_automaton *a, stcsp_engine *eng) {
    const stcsp_repair_request rq = {(int64_t)st.n(), st.offsets.data(), st.values.data(), nullptr, f.repair_final ? STCSP_REPAIR_END_FINAL : 0, 0};
    stcsp_repair_result r = {};
    std::vector<int32_t> distance, n_changed, values;  // (the twin's output)
    std::vector<uint8_t> fin;
    if (eng) {
        if (build_generator(eng, st.mask.data()) != STCSP_OK || stcsp_engine_repair(eng, &rq, &r) != STCSP_OK) return engine_error(eng);
    } else {
        distance.resize(st.n() + 1), n_changed.resize(st.n() + 1), values.resize(st.values.size() + 1), fin.resize(st.n() + 1);
        if (stcsp_automaton_repair_streams(a, st.mask.data(), rq.flags, rq.weights, rq.n_streams, rq.offsets, rq.values, distance.data(), values.data(),
                                           fin.data(), n_changed.data()) != STCSP_OK)
            return host_error("the streams could not be repaired");
        r.distance = distance.data(), r.values = values.data(), r.end_final = fin.data(), r.n_changed = n_changed.data();
    }
    print_repairs(p, st, r);
    return 0;
}

// --align
static void print_alignments(const stcsp_problem *p, const Streams &st, const stcsp_align_result &r) {
    const size_t n_obs = print_header(stdout, p, st.mask.data());
    for (size_t i = 0; i < st.n(); i++) {
        printf("# %zu distance %d len %lld out_len %lld n_changed %d n_skipped %d n_inserted %d end_final %d ops ", i, r.distance[i], st.len(i),
               (long long)(r.out_offsets[i + 1] - r.out_offsets[i]), r.n_changed[i], r.n_skipped[i], r.n_inserted[i], (int)r.end_final[i]);
        for (int64_t k = r.op_offsets[i]; k < r.op_offsets[i + 1]; k++) putchar("MDI"[r.ops[k] < 3 ? r.ops[k] : 0]);
        printf("\n");
        for (int64_t t = r.out_offsets[i]; t < r.out_offsets[i + 1]; t++) print_row(stdout, r.values + (size_t)t * n_obs, n_obs);
        printf("\n");
    }
    fflush(stdout);
}

static int align(const Flags &f, const stcsp_problem *p, const Streams &st, const stcsp_automaton *a, stcsp_engine *eng) {
    const stcsp_align_request rq = {(int64_t)st.n(), st.offsets.data(), st.values.data(), nullptr, f.align_skip, f.align_gap,
                                    f.align_final ? STCSP_ALIGN_END_FINAL : 0, 0};
    stcsp_align_result r = {};
    std::vector<int32_t> distance, n_changed, n_skipped, n_inserted;  // (the twin's output; it allocates the rows and the ops)
    std::vector<int64_t> out_off, op_off;
    std::vector<uint8_t> fin;
    int32_t *values = nullptr;
    uint8_t *ops = nullptr;
    if (eng) {
        if (build_generator(eng, st.mask.data()) != STCSP_OK || stcsp_engine_align(eng, &rq, &r) != STCSP_OK) return engine_error(eng);
    } else {
        distance.resize(st.n() + 1), n_changed.resize(st.n() + 1), n_skipped.resize(st.n() + 1), n_inserted.resize(st.n() + 1);
        out_off.resize(st.n() + 1), op_off.resize(st.n() + 1), fin.resize(st.n() + 1);
        if (stcsp_automaton_align_streams(a, st.mask.data(), rq.flags, rq.weights, rq.skip_cost, rq.gap_cost, rq.n_streams, rq.offsets, rq.values,
                                          distance.data(), out_off.data(), &values, op_off.data(), &ops, fin.data(), n_changed.data(), n_skipped.data(),
                                          n_inserted.data()) != STCSP_OK)
            return host_error("the streams could not be aligned");
        r.distance = distance.data(), r.out_offsets = out_off.data(), r.values = values, r.op_offsets = op_off.data(), r.ops = ops;
        r.n_changed = n_changed.data(), r.n_skipped = n_skipped.data(), r.n_inserted = n_inserted.data(), r.end_final = fin.data();
    }
    print_alignments(p, st, r);
    stcsp_host_free(values);
    stcsp_host_free(ops);
    return 0;
}

// --infer
static void print_inferences(const stcsp_problem *p, const Streams &st, int draws, const stcsp_infer_result &r) {
    const size_t n_obs = print_header(stdout, p, st.mask.data());
    for (size_t i = 0; i < st.n(); i++) {
        printf("# %zu count %.0f len %lld feasible %d\n", i, r.count[i], st.len(i), r.count[i] > 0.0 ? 1 : 0);
        for (int64_t t = st.offsets[i]; t < st.offsets[i + 1]; t++) {
            printf("#");
            for (size_t k = 0; k < n_obs; k++) {
                const int64_t b = r.support_off[(size_t)t * n_obs + k], e = r.support_off[(size_t)t * n_obs + k + 1];
                printf(" {");
                for (int64_t j = b; j < e; j++) printf(j > b ? ",%d" : "%d", r.support_val[j]);
                printf("}");
            }
            printf("\n");
        }
        for (int j = 0; j < draws && r.count[i] > 0.0; j++) {
            const int32_t *rows = r.values + ((size_t)st.offsets[i] * (size_t)draws + (size_t)j * (size_t)st.len(i)) * n_obs;
            for (long long t = 0; t < st.len(i); t++) print_row(stdout, rows + (size_t)t * n_obs, n_obs);
            printf("\n");
        }
    }
    fflush(stdout);
}

static int infer(const Flags &f, const stcsp_problem *p, const Streams &st, const stcsp_automaton *a, stcsp_engine *eng) {
    const stcsp_infer_request rq = {(int64_t)st.n(), st.offsets.data(), st.values.data(), nullptr, (uint64_t)f.infer_seed,
                                    f.infer_final ? STCSP_INFER_END_FINAL : 0, f.infer_draws};
    stcsp_infer_result r = {};
    std::vector<double> count;  // (the twin's output; it allocates the support values)
    std::vector<int64_t> support_off;
    std::vector<int32_t> n_states, values;
    std::vector<uint8_t> fin;
    int32_t *support_val = nullptr;
    if (eng) {
        if (build_generator(eng, st.mask.data()) != STCSP_OK || stcsp_engine_infer(eng, &rq, &r) != STCSP_OK) return engine_error(eng);
    } else {
        const size_t steps = (size_t)st.offsets.back(), draws = (size_t)f.infer_draws;
        count.resize(st.n() + 1), support_off.resize(steps * st.n_obs() + 1), n_states.resize(steps + st.n() + 1);
        values.resize(steps * draws * st.n_obs() + 1), fin.resize(st.n() * draws + 1);
        if (stcsp_automaton_infer_streams(a, st.mask.data(), rq.flags, rq.n_streams, rq.offsets, rq.values, rq.draws, rq.ranks, rq.seed, count.data(),
                                          support_off.data(), &support_val, n_states.data(), values.data(), fin.data()) != STCSP_OK)
            return host_error("the streams could not be inferred: draws from a count that overflows a double");
        r.count = count.data(), r.support_off = support_off.data(), r.support_val = support_val, r.values = values.data();
    }
    print_inferences(p, st, f.infer_draws, r);
    stcsp_host_free(support_val);
    return 0;
}

// --posterior-weights=<name>=<value>:<weight>[,...]: the CSR of the contract over the observable variables of the streams' mask
struct ValueWeights {
    std::vector<int64_t> off;
    std::vector<int32_t> val, w;
};
static int parse_value_weights(const char *text, const stcsp_problem *p, const Streams &st, ValueWeights &out) {
    std::vector<int> column((size_t)p->n_vars, -1);
    int n_obs = 0;
    for (int v = 0; v < p->n_vars; v++)
        if (st.mask[(size_t)v]) column[(size_t)v] = n_obs++;
    std::vector<std::vector<std::pair<long long, long long>>> per((size_t)n_obs);
    for (const char *q = text; *q;) {
        const char *eq = strchr(q, '=');
        if (!eq) return 1;
        const std::string name(q, eq);
        int var = -1;
        for (int v = 0; v < p->n_vars; v++)
            if (p->var_names && p->var_names[v] && name == p->var_names[v]) var = v;
        if (var < 0 || column[(size_t)var] < 0) {
            fprintf(stderr, "--posterior-weights: %s is not a variable of the streams\n", name.c_str());
            return 1;
        }
        char *end = nullptr;
        const long long value = strtoll(eq + 1, &end, 10);
        if (end == eq + 1 || *end != ':' || value < INT_MIN || value > INT_MAX) return 1;
        const char *ws = end + 1;
        const long long weight = strtoll(ws, &end, 10);
        if (end == ws || (*end != 0 && *end != ',') || weight < 0 || weight > INT_MAX) return 1;
        per[(size_t)column[(size_t)var]].push_back({value, weight});
        q = *end ? end + 1 : end;
    }
    out.off.assign(1, 0);
    for (auto &list : per) {
        std::stable_sort(list.begin(), list.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
        for (const auto &vw : list) {
            out.val.push_back((int32_t)vw.first);
            out.w.push_back((int32_t)vw.second);
        }
        out.off.push_back((int64_t)out.val.size());
    }
    out.val.push_back(0);  // (never NULL)
    out.w.push_back(0);
    return 0;
}

// --posterior
static void print_posteriors(const stcsp_problem *p, const Streams &st, const stcsp_posterior_result &r) {
    const size_t n_obs = print_header(stdout, p, st.mask.data());
    for (size_t i = 0; i < st.n(); i++) {
        printf("# %zu mass %.0f len %lld exact %d final_mass %llu\n", i, r.mass[i], st.len(i), r.exact[i] ? 1 : 0, (unsigned long long)r.final_mass[i]);
        for (int64_t t = st.offsets[i]; t < st.offsets[i + 1]; t++) {
            printf("#");
            for (size_t k = 0; k < n_obs; k++) {
                const int64_t b = r.marg_off[(size_t)t * n_obs + k], e = r.marg_off[(size_t)t * n_obs + k + 1];
                printf(" {");
                for (int64_t j = b; j < e; j++) printf(j > b ? ",%d:%llu" : "%d:%llu", r.marg_val[j], (unsigned long long)r.marg_mass[j]);
                printf("}");
            }
            printf("\n");
        }
    }
    fflush(stdout);
}

static int posterior(const Flags &f, const stcsp_problem *p, const Streams &st, const stcsp_automaton *a, stcsp_engine *eng) {
    static const char *const failed = "the posterior marginals could not be computed: malformed weights";
    ValueWeights vw;
    const bool weighted = f.posterior_weights != nullptr;
    // weights the command line cannot read are the host's to refuse: this sentence on the device road too, not the engine's message
    if (weighted && parse_value_weights(f.posterior_weights, p, st, vw)) return host_error(failed);
    const stcsp_posterior_request rq = {(int64_t)st.n(), st.offsets.data(), st.values.data(), weighted ? vw.off.data() : nullptr,
                                        weighted ? vw.val.data() : nullptr, weighted ? vw.w.data() : nullptr,
                                        f.posterior_final ? STCSP_POSTERIOR_END_FINAL : 0, 0};
    stcsp_posterior_result r = {};
    std::vector<double> mass;  // (the twin's output; it allocates the marginals)
    std::vector<uint8_t> exact;
    std::vector<uint64_t> final_mass;
    std::vector<int64_t> marg_off;
    int32_t *marg_val = nullptr;
    uint64_t *marg_mass = nullptr;
    if (eng) {
        if (build_generator(eng, st.mask.data()) != STCSP_OK || stcsp_engine_posterior(eng, &rq, &r) != STCSP_OK) return engine_error(eng);
    } else {
        mass.resize(st.n() + 1), exact.resize(st.n() + 1), final_mass.resize(st.n() + 1), marg_off.resize((size_t)st.offsets.back() * st.n_obs() + 1);
        if (stcsp_automaton_posterior_streams(a, st.mask.data(), rq.flags, rq.n_streams, rq.offsets, rq.values, rq.weight_off, rq.weight_val, rq.weight_w,
                                              mass.data(), exact.data(), final_mass.data(), marg_off.data(), &marg_val, &marg_mass) != STCSP_OK)
            return host_error(failed);
        r.mass = mass.data(), r.exact = exact.data(), r.final_mass = final_mass.data(), r.marg_off = marg_off.data();
        r.marg_val = marg_val, r.marg_mass = marg_mass;
    }
    print_posteriors(p, st, r);
    stcsp_host_free(marg_val);
    stcsp_host_free(marg_mass);
    return 0;
}

// --quotient: replace *a by its quotient. The one service whose roads differ in more than where the work is done: with an engine
// the partition is the device pass's (stcsp_engine_quotient), without one the host twin's.
static int fold(const Flags &f, const stcsp_problem *p, stcsp_automaton **a, stcsp_engine *eng) {
    static const char *const failed = "the quotient could not be built";
    std::vector<uint8_t> all((size_t)p->n_vars, 1);
    const uint8_t *mask = f.quotient_all ? all.data() : nullptr;
    std::vector<int32_t> host_class;
    const int32_t *state_class = nullptr;
    int64_t n_live = 0, n_classes = 0;
    if (eng) {
        stcsp_quotient_options qo = {mask, {0, 0}};
        stcsp_quotient_result qr;
        if (stcsp_engine_quotient(eng, &qo, &qr) != STCSP_OK) return engine_error(eng);
        state_class = qr.state_class, n_live = qr.n_states, n_classes = qr.n_classes;
        stcsp_automaton_set_observable(*a, mask);
    } else {
        host_class.assign((size_t)stcsp_automaton_num_states(*a) + 1, -1);
        if (stcsp_automaton_bisimulation(*a, mask, host_class.data(), &n_classes) < 0) return host_error(failed);
        state_class = host_class.data();
        for (int32_t c : host_class) n_live += c >= 0;
    }
    stcsp_automaton *q = nullptr;
    if (stcsp_automaton_quotient(*a, state_class, n_classes, &q) != STCSP_OK) return host_error(failed);
    stcsp_automaton_free(*a);
    *a = q;
    fprintf(stderr, "quotient: %lld -> %lld\n", (long long)n_live, (long long)n_classes);
    return 0;
}

// --compare=FILE: the observer `mine` of this model under `mask` (left) against the observer of FILE's automaton under the same
// variables, matched by name (right); on the device (eng: its last observer() built `mine`) or by the host twin (eng NULL)
static int compare_with_file(const Flags &f, const stcsp_problem *p, const uint8_t *mask, const stcsp_observer_result *mine, stcsp_engine *eng) {
    stcsp_automaton *other = nullptr;
    if (stcsp_automaton_read_binary(f.compare, &other) != STCSP_OK) {
        fprintf(stderr, "--compare: cannot read the automaton of '%s'\n", f.compare);
        return 1;
    }
    const int n_other = stcsp_automaton_num_vars(other);
    std::vector<uint8_t> other_mask((size_t)n_other, 0);
    std::vector<int> index_there;  // per observable variable of this model, in its order: the variable's index in FILE
    for (int v = 0; v < p->n_vars; v++) {
        if (!is_observable(p, mask, v)) continue;
        int u = 0;
        while (u < n_other && strcmp(stcsp_automaton_var_name(other, u), p->var_names[v]) != 0) u++;
        if (u == n_other) {
            fprintf(stderr, "--compare: '%s' has no variable named '%s'\n", f.compare, p->var_names[v]);
            stcsp_automaton_free(other);
            return 1;
        }
        other_mask[(size_t)u] = 1;
        index_there.push_back(u);
    }
    stcsp_observer *theirs = nullptr;
    if (stcsp_automaton_observer(other, other_mask.data(), 0, &theirs) != STCSP_OK) {
        fprintf(stderr, "--compare: the observer of '%s' could not be built\n", f.compare);
        stcsp_automaton_free(other);
        return 1;
    }
    // FILE's rows have its own column order: into this model's, and the edges of every state into the order of the new rows
    stcsp_observer_result right = *stcsp_observer_get(theirs);
    const size_t w = index_there.size(), E = (size_t)right.n_edges;
    std::vector<size_t> column(w), order(E);
    for (size_t c = 0; c < w; c++) column[c] = (size_t)std::count(other_mask.begin(), other_mask.begin() + index_there[c], 1);
    std::vector<int32_t> rows(E * w), src(E), dst(E), values(E * w);
    for (size_t e = 0; e < E; e++) {
        order[e] = e;
        for (size_t c = 0; c < w; c++) rows[e * w + c] = right.edge_values[e * w + column[c]];
    }
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        if (right.edge_src[a] != right.edge_src[b]) return right.edge_src[a] < right.edge_src[b];
        return std::lexicographical_compare(rows.begin() + a * w, rows.begin() + (a + 1) * w, rows.begin() + b * w, rows.begin() + (b + 1) * w);
    });
    for (size_t i = 0; i < E; i++) {
        src[i] = right.edge_src[order[i]];
        dst[i] = right.edge_dst[order[i]];
        std::copy(rows.begin() + order[i] * w, rows.begin() + (order[i] + 1) * w, values.begin() + i * w);
    }
    src.reserve(1);
    dst.reserve(1);
    values.reserve(1);
    right.edge_src = src.data();
    right.edge_dst = dst.data();
    right.edge_values = values.data();
    stcsp_comparison *twin = nullptr;
    stcsp_compare_result dev;
    const stcsp_compare_result *res = &dev;
    int rc = 0;
    if (eng) {
        stcsp_compare_request rq = {&right, 0, {0, 0}};
        if (stcsp_engine_compare(eng, &rq, &dev) != STCSP_OK) {
            fprintf(stderr, "%s\n", stcsp_engine_last_error(eng));
            rc = 1;
        }
    } else if (stcsp_compare_observers(mine, &right, 0, &twin) != STCSP_OK) {
        fprintf(stderr, "--compare: the comparison failed\n");
        rc = 1;
    } else {
        res = stcsp_comparison_get(twin);
    }
    if (!rc) {
        static const char *const claim[4] = {"P(left) in P(right)", "P(right) in P(left)", "F(left) in F(right)", "F(right) in F(left)"};
        fprintf(stderr, "compare: %lld pairs, %lld edges, %d levels\n", (long long)res->n_pairs, (long long)res->n_pair_edges, res->levels);
        for (int k = 0; k < 4; k++) {
            if (res->witness_len[k] < 0) {
                fprintf(stderr, "compare: %s: yes\n", claim[k]);
                continue;
            }
            fprintf(stderr, "compare: %s: no, %d steps:", claim[k], res->witness_len[k]);
            for (int t = 0; t < res->witness_len[k]; t++) {
                if (t) fprintf(stderr, ";");
                for (size_t c = 0; c < w; c++) fprintf(stderr, " %d", res->witness_values[((size_t)res->witness_off[k] + (size_t)t) * w + c]);
            }
            fprintf(stderr, "\n");
        }
    }
    stcsp_comparison_free(twin);
    stcsp_observer_free(theirs);
    stcsp_automaton_free(other);
    return rc;
}

// --components[=bottom|all|N]: the strongly connected components of the live automaton, which states start an infinite solution,
// and lasso solutions; on the device (eng: a finished postprocess()) or by the host twin on `a`'s current flags (eng NULL). stderr.
static int report_components(const Flags &f, const stcsp_problem *p, const stcsp_automaton *a, stcsp_engine *eng) {
    stcsp_components_options co = {f.components_lassos, f.components_bottom ? STCSP_SCC_LASSO_BOTTOM : 0, 0};
    stcsp_components_result dev;
    stcsp_components *twin = nullptr;
    const stcsp_components_result *r = &dev;
    if (eng) {
        if (stcsp_engine_components(eng, &co, &dev) != STCSP_OK) return engine_error(eng);
    } else {
        if (stcsp_automaton_components(a, co.max_lassos, co.flags, &twin) != STCSP_OK) return host_error("the components could not be computed");
        r = stcsp_components_get(twin);
    }
    fprintf(stderr, "components: %lld states, %lld components, %lld cyclic, %lld accepting, %lld bottom, %lld omega-live, infinite solution: %s\n",
            (long long)r->n_states, (long long)r->n_components, (long long)r->n_cyclic, (long long)r->n_accepting, (long long)r->n_bottom,
            (long long)r->n_omega, r->root_omega ? "yes" : "no");
    for (int64_t c = 0; c < r->n_components; c++) {
        const int32_t cf = r->comp_flags[c];
        fprintf(stderr, "components: component %lld: size %d, depth %d, flags %s%s%s%s%s\n", (long long)c, r->comp_size[c], r->comp_depth[c],
                cf & STCSP_SCC_CYCLIC ? "C" : "", cf & STCSP_SCC_FINAL ? "F" : "", cf & STCSP_SCC_BOTTOM ? "B" : "", cf & STCSP_SCC_ACCEPTING ? "A" : "",
                cf ? "" : "-");
    }
    if (r->n_lassos) {
        fprintf(stderr, "components: ");
        print_header(stderr, p, nullptr);
    }
    for (int64_t i = 0; i < r->n_lassos; i++) {
        const int64_t b = r->lasso_off[i], m = b + r->lasso_stem_len[i], e = r->lasso_off[i + 1];
        fprintf(stderr, "components: lasso of component %d: %lld + %lld steps\n", r->lasso_component[i], (long long)(m - b), (long long)(e - m));
        for (int part = 0; part < 2; part++) {
            fprintf(stderr, part ? "components: loop:" : "components: stem:");
            print_steps(stderr, p, r->lasso_values, r->n_vars, part ? m : b, part ? e : m);
        }
    }
    stcsp_components_free(twin);
    return 0;
}

// --optimise=min|max:NAME=W[,NAME=W...][:HORIZON][:mean]: the weights per variable, STCSP_OPT_* and the horizon of the spec; says what is
// wrong with one it cannot read
static int parse_optimise(const char *text, const stcsp_problem *p, std::vector<int32_t> &w, int32_t &flags, int32_t &horizon) {
    w.assign((size_t)p->n_vars, 0);
    std::string spec = text;
    std::vector<std::string> parts;
    for (size_t at = 0;;) {
        const size_t colon = spec.find(':', at);
        parts.push_back(spec.substr(at, colon == std::string::npos ? colon : colon - at));
        if (colon == std::string::npos) break;
        at = colon + 1;
    }
    const char *usage = "--optimise takes min|max:NAME=W[,NAME=W...][:HORIZON][:mean]";
    if (parts.size() < 2 || (parts[0] != "min" && parts[0] != "max")) {
        fprintf(stderr, "%s\n", usage);
        return 1;
    }
    flags = parts[0] == "max" ? STCSP_OPT_MAXIMISE : 0;
    horizon = 0;
    for (size_t at = 0; at <= parts[1].size();) {
        const size_t comma = std::min(parts[1].find(',', at), parts[1].size());
        const std::string item = parts[1].substr(at, comma - at);
        const size_t eq = item.find('=');
        int var = -1;
        for (int v = 0; v < p->n_vars && eq != std::string::npos; v++)
            if (p->var_names && p->var_names[v] && item.substr(0, eq) == p->var_names[v]) var = v;
        char *end = nullptr;
        const long long value = eq == std::string::npos ? 0 : strtoll(item.c_str() + eq + 1, &end, 10);
        if (var < 0 || !end || *end || end == item.c_str() + eq + 1 || value < -2147483647ll || value > 2147483647ll) {
            fprintf(stderr, "--optimise: '%s' is not NAME=W with a variable of the model and an integer\n", item.c_str());
            return 1;
        }
        w[(size_t)var] = (int32_t)value;
        at = comma + 1;
    }
    for (size_t i = 2; i < parts.size(); i++) {
        char *end = nullptr;
        const long long h = strtoll(parts[i].c_str(), &end, 10);
        if (parts[i] == "mean" && i + 1 == parts.size())
            flags |= STCSP_OPT_MEAN;
        else if (i == 2 && !parts[i].empty() && !*end && h >= 0 && h <= 0x7fffffffll)
            horizon = (int32_t)h;
        else {
            fprintf(stderr, "%s\n", usage);
            return 1;
        }
    }
    return 0;
}

// --optimise: the best prefixes and the least long-run mean; on the device (eng: a finished postprocess()) or by the host twin on
// `a`'s current flags (eng NULL). stderr.
static int report_optimum(const Flags &f, const stcsp_problem *p, const stcsp_automaton *a, stcsp_engine *eng) {
    static const char *const failed = "the optimum could not be computed";
    std::vector<int32_t> w;
    int32_t flags = 0, horizon = 0;
    // a spec that cannot be read: after the parser's complaint the host roads add their sentence, the device road adds nothing
    if (parse_optimise(f.optimise, p, w, flags, horizon)) return eng ? 1 : host_error(failed);
    const stcsp_optimise_request rq = {w.data(), &horizon, horizon, 1, flags, 0};
    stcsp_optimise_result dev;
    stcsp_optimise *twin = nullptr;
    const stcsp_optimise_result *r = &dev;
    if (eng) {
        if (stcsp_engine_optimise(eng, &rq, &dev) != STCSP_OK) return engine_error(eng);
    } else {
        if (stcsp_automaton_optimise(a, &rq, &twin) != STCSP_OK) return host_error(failed);
        r = stcsp_optimise_get(twin);
    }
    for (int32_t L = 0; L <= horizon; L++) {
        if (r->best[L] == STCSP_OPT_NONE)
            fprintf(stderr, "optimise: best[%d] = none\n", L);
        else
            fprintf(stderr, "optimise: best[%d] = %lld\n", L, (long long)r->best[L]);
    }
    if (r->best[horizon] != STCSP_OPT_NONE) {
        fprintf(stderr, "optimise: ");
        print_header(stderr, p, nullptr);
        fprintf(stderr, "optimise: witness:");
        print_steps(stderr, p, r->witness_values, r->n_vars, r->witness_off[0], r->witness_off[1]);
    }
    if (flags & STCSP_OPT_MEAN) {
        for (int64_t c = 0; c < r->n_components; c++)
            if (r->comp_mean_den[c])
                fprintf(stderr, "optimise: component %lld: mean %lld/%lld\n", (long long)c, (long long)r->comp_mean_num[c], (long long)r->comp_mean_den[c]);
        if (r->omega_mean_den)
            fprintf(stderr, "optimise: omega: mean %lld/%lld in component %d\n", (long long)r->omega_mean_num, (long long)r->omega_mean_den, r->omega_component);
        else
            fprintf(stderr, "optimise: omega: none\n");
    }
    stcsp_optimise_free(twin);
    return 0;
}

// --ctl: a fair CTL query over the infinite solutions; on the device (eng: a finished postprocess()) or by the host twin on `a`'s
// current flags (eng NULL). program: what load() parsed. stderr.
static int report_ctl(const stcsp_problem *p, const std::vector<int32_t> &program, const stcsp_automaton *a, stcsp_engine *eng) {
    const stcsp_ctl_request rq = {program.data(), (int32_t)program.size(), STCSP_CTL_WITNESS};
    stcsp_ctl_result dev;
    stcsp_ctl *twin = nullptr;
    const stcsp_ctl_result *r = &dev;
    if (eng) {
        if (stcsp_engine_ctl(eng, &rq, &dev) != STCSP_OK) return engine_error(eng);
    } else {
        if (stcsp_automaton_ctl(a, &rq, &twin) != STCSP_OK) return host_error("the formula could not be evaluated");
        r = stcsp_ctl_get(twin);
    }
    fprintf(stderr, "ctl: %lld steps on infinite solutions, holds at %lld of %lld first steps: %s\n", (long long)r->n_worlds, (long long)r->n_initial_sat,
            (long long)r->n_initial, r->n_initial == 0 ? "vacuous" : r->n_initial_sat == r->n_initial ? "yes" : "no");
    if (r->witness_kind != STCSP_CTL_NONE) {
        fprintf(stderr, "ctl: ");
        print_header(stderr, p, nullptr);
        fprintf(stderr, r->witness_kind == STCSP_CTL_IS_WITNESS ? "ctl: witness:" : "ctl: counterexample:");
        print_steps(stderr, p, r->witness_values, r->n_vars, 0, r->witness_len);
    }
    stcsp_ctl_free(twin);
    return 0;
}

// --observer: replace *a by its observer, built on the device (eng: a finished postprocess()) or by the host twin (eng NULL);
// with --quotient, folded by the host bisimulation under the same mask
static int replace_by_observer(const Flags &f, const stcsp_problem *p, stcsp_automaton **a, stcsp_engine *eng) {
    std::vector<uint8_t> named((size_t)p->n_vars, strcmp(f.observer_mask, "all") == 0 ? 1 : 0);
    const uint8_t *mask = f.observer_mask[0] ? named.data() : nullptr;
    if (f.observer_mask[0] && strcmp(f.observer_mask, "all") != 0) {
        std::string list = f.observer_mask;
        for (size_t at = 0; at <= list.size();) {
            const size_t comma = std::min(list.find(',', at), list.size());
            const std::string name = list.substr(at, comma - at);
            int v = 0;
            while (v < p->n_vars && name != p->var_names[v]) v++;
            if (v == p->n_vars) {
                fprintf(stderr, "--observer: no variable named '%s'\n", name.c_str());
                return 1;
            }
            named[(size_t)v] = 1;
            at = comma + 1;
        }
    }
    const long long n_live = (long long)stcsp_automaton_num_live_states(*a);
    stcsp_observer *twin = nullptr;
    stcsp_observer_result dev;
    const stcsp_observer_result *res = &dev;
    if (eng) {
        stcsp_observer_options oo = {0, {0, 0}};
        if (build_generator(eng, mask) != STCSP_OK || stcsp_engine_observer(eng, &oo, &dev) != STCSP_OK) return engine_error(eng);
    } else {
        if (stcsp_automaton_observer(*a, mask, 0, &twin) != STCSP_OK) return 1;
        res = stcsp_observer_get(twin);
    }
    stcsp_automaton *q = nullptr;
    const int rc = stcsp_automaton_from_observer(*a, mask, res, &q);
    fprintf(stderr, "observer: %lld -> %lld states, %lld edges\n", n_live, (long long)res->n_states, (long long)res->n_edges);
    if (rc == STCSP_OK && f.compare && compare_with_file(f, p, mask, res, eng)) {
        stcsp_observer_free(twin);
        stcsp_automaton_free(q);
        return 1;
    }
    stcsp_observer_free(twin);
    if (rc != STCSP_OK) return 1;
    stcsp_automaton_free(*a);
    *a = q;
    if (f.quotient) {
        std::vector<int32_t> cls((size_t)stcsp_automaton_num_states(*a) + 1, -1);
        int64_t n_classes = 0, n_states = 0;
        if (stcsp_automaton_bisimulation(*a, mask, cls.data(), &n_classes) < 0) return 1;
        for (int32_t c : cls) n_states += c >= 0;
        if (stcsp_automaton_quotient(*a, cls.data(), n_classes, &q) != STCSP_OK) return 1;
        stcsp_automaton_free(*a);
        *a = q;
        fprintf(stderr, "quotient: %lld -> %lld\n", (long long)n_states, (long long)n_classes);
    }
    return 0;
}

// --observer: whatever failed has been named above, by the parser, the engine or --compare; on both roads this sentence follows it
static int observe(const Flags &f, const stcsp_problem *p, stcsp_automaton **a, stcsp_engine *eng) {
    return replace_by_observer(f, p, a, eng) ? host_error("the observer could not be built") : 0;
}

// Every service the flags ask for, in this order, on the device (eng: a finished postprocess() whose flags *a has adopted) or by
// the host twins on *a's current flags (eng NULL). The one list of services: a new one is entered here and nowhere else.
static int run_services(const Flags &f, const stcsp_problem *p, const Streams &streams, const std::vector<int32_t> &ctl_program, stcsp_automaton **a,
                        stcsp_engine *eng) {
    if (f.check && check(f, p, streams, *a, eng)) return 1;
    if ((f.sample || f.count_len >= 0) && generate(f, p, *a, eng)) return 1;
    if (f.repair && repair(f, p, streams, *a, eng)) return 1;
    if (f.align && align(f, p, streams, *a, eng)) return 1;
    if (f.infer && infer(f, p, streams, *a, eng)) return 1;
    if (f.posterior && posterior(f, p, streams, *a, eng)) return 1;
    if (f.components && report_components(f, p, *a, eng)) return 1;
    if (f.optimise && report_optimum(f, p, *a, eng)) return 1;
    if (f.ctl && report_ctl(p, ctl_program, *a, eng)) return 1;
    if (f.observer && observe(f, p, a, eng)) return 1;
    if (f.quotient && !f.observer && fold(f, p, a, eng)) return 1;  // (with --observer, observe() has folded the observer)
    return 0;
}

// ---- one run: load(), a solve that leaves (result, automaton, engine or NULL), run_services(), finish()
struct Run {
    stcsp_model *model = nullptr;
    const stcsp_problem *p = nullptr;
    Streams streams;       // of the one streams file, if any
    std::vector<int32_t> ctl_program;  // of --ctl
    FILE *info = stdout;   // the adver and statistics lines: stderr when stdout holds a service's answers only
    double init_time = 0;
    ~Run() { stcsp_model_free(model); }  // (on the early returns too; after the engines, which are destroyed before a return 0)
};

static int load(const Flags &f, Run &run) {
    const double t_init = cpu_time();
    if (stcsp_model_load_file(f.file, f.prefix_k, &run.model) != STCSP_OK) {
        // syntax errors go to stdout like yyerror (stcsp.y:221-224); the rest to error.txt in the
        // reference (myLog) -- stderr here
        const char *msg = stcsp_host_last_error();
        if (strncmp(msg, "Line ", 5) == 0)
            printf("%s\n", msg);
        else
            fprintf(stderr, "%s\n", msg);
        return 1;
    }
    run.p = stcsp_model_problem(run.model);
    bool missing_ok = false;
    const char *path = f.streams_file(&missing_ok);
    if (path && read_streams(path, run.p, run.streams, missing_ok)) return 1;
    if (f.ctl) {  // before anything is solved: a formula that does not parse ends the run
        int32_t *words = nullptr, n_words = 0, at = 0;
        char message[256] = "";
        if (stcsp_ctl_parse(f.ctl, run.p, &words, &n_words, &at, message, sizeof message) != STCSP_OK) {
            fprintf(stderr, "--ctl: %d: %s\n", at, message);
            return 1;
        }
        run.ctl_program.assign(words, words + n_words);
        stcsp_host_free(words);
    }
    run.info = f.quiet() ? stderr : stdout;
    run.init_time = cpu_time() - t_init;
    return 0;
}

// graphTraverse / adversarialTraverse / adversarialTraverse2 (solveralgorithm.cpp:974-983) by the host passes
static void host_passes(const Flags &f, stcsp_automaton *a, FILE *info) {
    stcsp_automaton_traverse(a);
    if (f.adv1) fprintf(info, "adver1: %d; ", stcsp_automaton_adversarial(a, 5));
    if (f.adv2) fprintf(info, "adver2: %d\n", stcsp_automaton_adversarial2(a, 5, 6));
}

// the tail of a run: the files, the statistics line of `res`'s counters, and the automaton's release
static void finish(const Flags &f, const Run &run, stcsp_automaton *a, const stcsp_result &res, double solve_time, double t_proc, bool print_line,
                   double *total) {
    if (f.print_solution || f.binary) stcsp_automaton_order_by_label(a);  // reproducible files whatever the GPU's scheduling
    stcsp_automaton_renumber(a);
    const double proc_time = cpu_time() - t_proc;
    if (f.print_solution) stcsp_automaton_write_dot(a, "solutions.dot");
    if (f.binary && stcsp_automaton_write_binary(a, f.binary) != STCSP_OK) fprintf(stderr, "cannot write %s\n", f.binary);
    if (print_line) {
        // init_time, var, con, dom, node, fail, solve_time, processTime (solveralgorithm.cpp:1001)
        fprintf(run.info, "%.2f\t%d\t%d\t%d\t%d\t%d\t%.2f\t%.5f\n", run.init_time, run.p->n_vars, run.p->n_constraints, (int)res.counters.dominance,
                (int)res.n_states, (int)res.counters.fails, solve_time, proc_time);
        fflush(run.info);
    }
    if (total) *total = solve_time + proc_time;
    stcsp_automaton_free(a);
}

static int run_once(const Flags &f, bool print_line, double *total) {
    Run run;
    if (load(f, run)) return 1;
    stcsp_options opt;
    memset(&opt, 0, sizeof opt);
    opt.world = 1;
    opt.flags = f.intervals ? STCSP_F_INTERVAL_DOMAINS : 0;
    opt.time_limit_s = f.time_limit;  // -m: the reference exit(0)s silently on SIGALRM (solver.cpp:190-193)
    stcsp_engine *eng = nullptr;
    if (stcsp_engine_create(run.p, &opt, &eng) != STCSP_OK) return engine_error(nullptr);
    const double t_solve = cpu_time();
    stcsp_result res;
    if (stcsp_engine_solve(eng, &res) != STCSP_OK) return engine_error(eng);
    if (res.truncated) exit(0);  // time limit: silent exit 0, like the reference
    const double solve_time = cpu_time() - t_solve, t_proc = cpu_time();
    stcsp_automaton *a = nullptr;
    stcsp_automaton_build(run.p, &res, &a);
    // the traversals run on the device over the automaton the export left in HBM; the host only adopts the flags
    stcsp_post_options po = {f.adv1 ? 5 : -1, f.adv2 ? 5 : -1, f.adv2 ? 6 : -1, 0};
    stcsp_post_result post;
    stcsp_engine *device = eng;  // where the services run
    const int rc = stcsp_engine_postprocess(eng, &po, &post);
    if (rc == STCSP_E_UNSUPPORTED) {  // an adversarial variable wider than the device passes take: the host passes and twins
        host_passes(f, a, run.info);
        device = nullptr;
    } else if (rc != STCSP_OK) {
        return engine_error(eng);
    } else {
        stcsp_automaton_import_flags(a, post.state_valid, post.state_final, post.edge_alive);
        if (f.adv1) fprintf(run.info, "adver1: %d; ", post.adver1);
        if (f.adv2) fprintf(run.info, "adver2: %d\n", post.adver2);
    }
    if (run_services(f, run.p, run.streams, run.ctl_program, &a, device)) return 1;
    finish(f, run, a, res, solve_time, t_proc, print_line, total);
    stcsp_engine_destroy(eng);
    return 0;
}

// --shards=N: the same run with the frontier and the state table sharded over N engines (see the header comment); the merged
// automaton lives on the host, so the host passes and the host twins work on it
static int run_sharded(const Flags &f, bool print_line, double *total) {
    Run run;
    if (load(f, run)) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return host_error("no HIP device available");
    const int world = f.shards;
    std::vector<stcsp_engine *> eng((size_t)world, nullptr);
    for (int r = 0; r < world; r++) {
        stcsp_options opt;
        memset(&opt, 0, sizeof opt);
        opt.device = r % ndev;
        opt.rank = r;
        opt.world = world;
        opt.flags = f.intervals ? STCSP_F_INTERVAL_DOMAINS : 0;
        opt.time_limit_s = f.time_limit;
        if (stcsp_engine_create(run.p, &opt, &eng[(size_t)r]) != STCSP_OK) return engine_error(nullptr);
    }
    stcsp_local_group *group = nullptr;
    if (stcsp_local_group_create(world, &group) != STCSP_OK) return 1;
    const double t_solve = cpu_time();
    std::vector<int> rcs((size_t)world, 0);
    {
        std::vector<std::thread> th;
        for (int r = 0; r < world; r++)
            th.emplace_back([&, r] { rcs[(size_t)r] = stcsp_engine_solve_sharded(eng[(size_t)r], stcsp_local_group_transport(group, r), nullptr, nullptr); });
        for (auto &t : th) t.join();
    }
    for (int r = 0; r < world; r++)
        if (rcs[(size_t)r] != STCSP_OK) {
            fprintf(stderr, "shard %d: %s\n", r, stcsp_engine_last_error(eng[(size_t)r]));
            return 1;
        }
    std::vector<stcsp_result> res((size_t)world);
    std::vector<const stcsp_result *> resp;
    for (int r = 0; r < world; r++) {
        if (stcsp_engine_export(eng[(size_t)r], &res[(size_t)r]) != STCSP_OK) {
            fprintf(stderr, "shard %d: %s\n", r, stcsp_engine_last_error(eng[(size_t)r]));
            return 1;
        }
        if (res[(size_t)r].truncated) exit(0);  // time limit: silent exit 0, like the reference
        resp.push_back(&res[(size_t)r]);
    }
    stcsp_merged *mg = nullptr;
    if (stcsp_merge_shards(resp.data(), world, &mg) != STCSP_OK) return host_error("merging the shards failed");
    const double solve_time = cpu_time() - t_solve, t_proc = cpu_time();
    stcsp_automaton *a = nullptr;
    stcsp_automaton_build(run.p, stcsp_merged_result(mg), &a);
    host_passes(f, a, run.info);
    if (run_services(f, run.p, run.streams, run.ctl_program, &a, nullptr)) return 1;
    finish(f, run, a, *stcsp_merged_result(mg), solve_time, t_proc, print_line, total);
    stcsp_merged_free(mg);
    stcsp_local_group_destroy(group);
    for (stcsp_engine *e : eng) stcsp_engine_destroy(e);
    return 0;
}

int main(int argc, char **argv) {
    Flags f;
    // Option letters of the reference (getopt string "b:e:cv:l:stk:m:az", src/solver.cpp:211). Short flags
    // may be grouped (-sa); an option value may be attached (-k3, the only form the reference's own
    // main() handles, src/stcsp.y:199-206) or be the next argument (-k 3).
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        if (a[0] != '-' || a[1] == 0) {
            if (!f.file) f.file = a;
            continue;
        }
        if (strncmp(a, "--binary=", 9) == 0) {
            f.binary = a + 9;
            continue;
        }
        if (strcmp(a, "--observer") == 0 || strncmp(a, "--observer=", 11) == 0) {
            f.observer = true;
            f.observer_mask = a[10] == '=' ? a + 11 : "";
            continue;
        }
        if (strcmp(a, "--components") == 0 || strncmp(a, "--components=", 13) == 0) {
            const char *arg = a[12] == '=' ? a + 13 : "";
            f.components = true;
            f.components_bottom = strcmp(arg, "bottom") == 0;
            f.components_lassos = !*arg ? 0 : (f.components_bottom || strcmp(arg, "all") == 0) ? -1 : atoll(arg);
            if (*arg && f.components_lassos == 0) f.components_lassos = -2;
            if (f.components_lassos < -1) {
                fprintf(stderr, "--components takes nothing, bottom, all or a positive count\n");
                return 1;
            }
            continue;
        }
        if (strncmp(a, "--optimise=", 11) == 0) {
            f.optimise = a + 11;
            continue;
        }
        if (strcmp(a, "--ctl") == 0 || strncmp(a, "--ctl=", 6) == 0) {
            if (a[5] != '=') {
                fprintf(stderr, "--ctl takes a formula, as in --ctl='AG EF m == 0'\n");
                return 1;
            }
            f.ctl = a + 6;
            continue;
        }
        if (strncmp(a, "--compare=", 10) == 0) {
            f.compare = a + 10;
            continue;
        }
        if (strcmp(a, "--quotient") == 0 || strcmp(a, "--quotient=all") == 0) {
            f.quotient = true;
            f.quotient_all = a[10] == '=';
            continue;
        }
        if (strncmp(a, "--check=", 8) == 0) {
            f.check = a + 8;
            continue;
        }
        if (strncmp(a, "--repair=", 9) == 0) {
            f.repair = a + 9;
            continue;
        }
        if (strcmp(a, "--repair-final") == 0) {
            f.repair_final = true;
            continue;
        }
        if (strncmp(a, "--align=", 8) == 0) {
            f.align = a + 8;
            continue;
        }
        if (strcmp(a, "--align-final") == 0) {
            f.align_final = true;
            continue;
        }
        if (strncmp(a, "--align-costs=", 14) == 0) {
            char tail = 0;
            if (sscanf(a + 14, "%d:%d%c", &f.align_skip, &f.align_gap, &tail) != 2 || f.align_skip < 1 || f.align_gap < 1) {
                fprintf(stderr, "--align-costs=SKIP:GAP takes two integers of at least 1\n");
                return 1;
            }
            continue;
        }
        if (strncmp(a, "--infer=", 8) == 0) {
            f.infer = a + 8;
            continue;
        }
        if (strcmp(a, "--infer-final") == 0) {
            f.infer_final = true;
            continue;
        }
        if (strncmp(a, "--infer-draws=", 14) == 0) {
            char *end = nullptr;
            const long d = strtol(a + 14, &end, 10);
            bool ok = end != a + 14 && (*end == 0 || *end == ':') && d >= 0 && d <= 1000000;
            if (ok && *end == ':') {
                const char *q = end + 1;
                f.infer_seed = strtoll(q, &end, 10);
                ok = end != q && *end == 0 && f.infer_seed >= 0;
            }
            if (!ok) {
                fprintf(stderr, "Invalid argument: %s\n", a);
                return 1;
            }
            f.infer_draws = (int)d;
            continue;
        }
        if (strncmp(a, "--posterior=", 12) == 0) {
            f.posterior = a + 12;
            continue;
        }
        if (strcmp(a, "--posterior-final") == 0) {
            f.posterior_final = true;
            continue;
        }
        if (strncmp(a, "--posterior-weights=", 20) == 0) {
            f.posterior_weights = a + 20;
            continue;
        }
        if (strncmp(a, "--sample=", 9) == 0) {
            char *end = nullptr;
            f.sample_n = strtoll(a + 9, &end, 10);
            bool ok = end != a + 9 && *end == ':' && f.sample_n >= 0 && f.sample_n <= 100000000;
            if (ok) {
                const char *q = end + 1;
                const long len = strtol(q, &end, 10);
                ok = end != q && (*end == 0 || *end == ':') && len >= 0 && len <= 1000000;
                f.sample_len = (int)len;
                if (ok && *end == ':') {
                    q = end + 1;
                    f.sample_seed = strtoll(q, &end, 10);
                    ok = end != q && *end == 0 && f.sample_seed >= 0;
                }
            }
            if (!ok) {
                fprintf(stderr, "Invalid argument: %s\n", a);
                return 1;
            }
            f.sample = true;
            continue;
        }
        if (strncmp(a, "--count=", 8) == 0) {
            char *end = nullptr;
            const long len = strtol(a + 8, &end, 10);
            if (end == a + 8 || *end || len < 0 || len > 1000000) {
                fprintf(stderr, "Invalid argument: %s\n", a);
                return 1;
            }
            f.count_len = (int)len;
            continue;
        }
        if (strcmp(a, "--sample-final") == 0) {
            f.sample_final = true;
            continue;
        }
        if (strcmp(a, "--sample-mask=all") == 0) {
            f.sample_all = true;
            continue;
        }
        if (strcmp(a, "--intervals") == 0) {
            f.intervals = true;
            continue;
        }
        if (strncmp(a, "--shards=", 9) == 0) {
            f.shards = atoi(a + 9);
            if (f.shards < 1 || f.shards > 64) {
                fprintf(stderr, "Invalid argument: %s\n", a);
                return 1;
            }
            continue;
        }
        for (const char *q = a + 1; *q; q++) {
            const char o = *q;
            if (strchr("bevlkm", o)) {  // takes a value: the rest of this argument, else the next one
                const char *val = q[1] ? q + 1 : (i + 1 < argc ? argv[++i] : nullptr);
                if (!val) {
                    fprintf(stderr, "Option -%c needs a value\n", o);
                    return 1;
                }
                if (o == 'k' || o == 'm') {
                    char *end = nullptr;
                    const long n = strtol(val, &end, 10);
                    if (end == val || *end || n < 0 || n > 1000000 || (o == 'k' && n <= 0)) {
                        fprintf(stderr, "Invalid argument: -%c %s\n", o, val);
                        return 1;
                    }
                    (o == 'k' ? f.prefix_k : f.time_limit) = (int)n;
                }
                break;  // b, e, v, l: parsed but unused in the reference too
            }
            switch (o) {
                case 's': f.print_solution = true; break;
                case 't': f.testing = true; break;
                case 'a': f.adv1 = true; break;
                case 'z': f.adv2 = true; break;
                default: fprintf(stderr, "Unknown argument: %c\n", o); return 1;
            }
        }
    }
    if ((f.check != nullptr) + (f.repair != nullptr) + (f.align != nullptr) + (f.infer != nullptr) + (f.posterior != nullptr) + f.sample + (f.count_len >= 0) > 1) {
        fprintf(stderr, "--check, --repair, --align, --infer, --posterior, --sample and --count exclude each other\n");
        return 1;
    }
    if (f.compare && !f.observer) {
        fprintf(stderr, "--compare needs --observer: the observers of the two models are compared\n");
        return 1;
    }
    if (!f.file) {
        printf("No constraints!\n");
        return 0;
    }
    auto run = [&](bool print_line, double *total) { return f.shards > 1 ? run_sharded(f, print_line, total) : run_once(f, print_line, total); };
    int rc = run(!f.testing, nullptr);
    if (rc) return rc;
    if (f.testing) {  // -t: re-solve until the 95% CI half-width < 2.5% of the mean (solver.cpp:295-349)
        std::vector<double> times;
        for (;;) {
            printf("%d ", (int)times.size());
            fflush(stdout);
            double t = 0;
            if ((rc = run(true, &t))) return rc;
            times.push_back(t);
            size_t n = times.size();
            if (n >= 10) {
                double mean = 0, var = 0;
                for (double x : times) mean += x;
                mean /= n;
                for (double x : times) var += (x - mean) * (x - mean);
                var /= (n - 1);
                if (2 * 1.96 * sqrt(var) / sqrt((double)n) < 0.05 * mean) {
                    printf("\nMean execution time is %f pm %f\n", mean, 1.96 * sqrt(var) / sqrt((double)n));
                    break;
                }
            }
        }
    }
    return 0;
}
