/*
 * stcsp_engine.h -- C-ABI of the MI355X stream-CSP propagation + search engine.
 *
 * This is the drop-in boundary for the reference's
 *     double solverSolve(Solver *solver, bool testing)
 * (reference: src/solveralgorithm.h:11, defined src/solveralgorithm.cpp:945-1005; the
 * narrowest cut is lines 966-971 = "levelUp; if (GAC) solverSolveRe(root) else numFails++").
 *
 * What crosses the boundary is exactly what solverSolve reads from / leaves in `Solver`
 * (src/solver.h:22-49), flattened to plain-old-data:
 *   in : varQueue (lb/ub, order = branching order = edge-label order), arrayQueue,
 *        constrQueue (the normalised constraint trees, in queue order), prefixK
 *   out: the automaton the search leaves in solver->graph (src/graph.h:47-72): the state
 *        table (signature, constraint-set id, fail flag), the labelled edges, and the
 *        counters numFails / numDominance / numNodes (src/solver.h:28-39).
 * Everything else in solverSolve (graphTraverse, adversarial passes, renumberVertex,
 * solutions.dot, the stats line; lines 972-1005) stays on the host side of this ABI
 * (see stcsp_host.h).
 *
 * Plain C types only. Every function returns 0 on success or a negative STCSP_E_* code;
 * the library never calls exit() (the reference exit(1)s on every error, e.g.
 * src/solver.cpp:33-36).
 */
#ifndef STCSP_ENGINE_H
#define STCSP_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- expression-tree tokens (mirror of the yacc tokens used in ConstraintNode::token,
 *      src/constraint.h:24-31; numbering is this ABI's own, not y.tab.h's) ---- */
enum stcsp_token {
    STCSP_T_CONST = 1, /* CONSTANT            num = value                       */
    STCSP_T_VAR,       /* IDENTIFIER          var = variable index              */
    STCSP_T_ARR,       /* ARR_IDENTIFIER      arr = array index, right = index  */
    STCSP_T_FIRST,     /* first e             right = e                         */
    STCSP_T_NEXT,      /* next  e             right = e                         */
    STCSP_T_FBY,       /* a fby b             (never present after normalise)   */
    STCSP_T_AT,        /* e @ k               left = e, right = CONST k         */
    STCSP_T_ABS,       /* abs e               right = e                         */
    STCSP_T_NOT,       /* not e               right = e                         */
    STCSP_T_IF,        /* if c then a else b  left = c, right = THEN(a, b)      */
    STCSP_T_THEN,
    STCSP_T_AND,
    STCSP_T_OR,
    STCSP_T_ADD,
    STCSP_T_SUB,
    STCSP_T_MUL,
    STCSP_T_DIV,
    STCSP_T_MOD,
    STCSP_T_LT_OP, /* lt gt le ge eq ne : expression-level comparisons */
    STCSP_T_GT_OP,
    STCSP_T_LE_OP,
    STCSP_T_GE_OP,
    STCSP_T_EQ_OP,
    STCSP_T_NE_OP,
    STCSP_T_LT_CON, /* <  >  <=  >=  ==  !=  ->  until : constraint roots */
    STCSP_T_GT_CON,
    STCSP_T_LE_CON,
    STCSP_T_GE_CON,
    STCSP_T_EQ_CON,
    STCSP_T_NE_CON,
    STCSP_T_IMPLY_CON,
    STCSP_T_UNTIL_CON
};

/* One node of a flattened constraint tree (ConstraintNode, src/constraint.h:24-31).
 * left/right index into stcsp_problem::nodes, -1 = NULL. */
typedef struct stcsp_node {
    int32_t token;
    int32_t num;
    int32_t var;   /* -1 unless token == STCSP_T_VAR */
    int32_t arr;   /* -1 unless token == STCSP_T_ARR */
    int32_t left;
    int32_t right;
} stcsp_node;

/* The built model, as solverSolve finds it (src/solver.h:22-49). */
typedef struct stcsp_problem {
    int32_t n_vars;               /* varQueue->size(), aux vars (_V%d) included, in queue order */
    int32_t prefix_k;             /* Solver::prefixK (-k, default 2)                           */
    const int32_t *var_lb;        /* [n_vars] Variable::lb  (src/variable.h:13)                */
    const int32_t *var_ub;        /* [n_vars] Variable::ub                                      */
    const char *const *var_names; /* [n_vars] may be NULL (only the dot writer needs names)    */
    int32_t n_arrays;             /* arrayQueue->size()                                         */
    const int32_t *array_off;     /* [n_arrays + 1] offsets into array_data                     */
    const int32_t *array_data;    /* Array::elements, concatenated (src/variable.h:54-59)       */
    int32_t n_nodes;
    const stcsp_node *nodes;         /* all constraint trees                                    */
    int32_t n_constraints;           /* constrQueue->size()                                     */
    const int32_t *constraint_root;  /* [n_constraints] root node of each, in constrQueue order */
} stcsp_problem;

typedef struct stcsp_options {
    int32_t device;           /* HIP device ordinal (ignored by the CPU oracle)                    */
    int32_t rank;             /* this shard (0 when not sharded)                                   */
    int32_t world;            /* number of shards; states are owned by hash(key) % world          */
    int32_t batch_nodes;      /* max open search nodes expanded per kernel launch (0 = default)    */
    int64_t max_search_nodes; /* stop after this many node expansions (0 = unlimited)              */
    double time_limit_s;      /* stop after this many seconds of search (0 = unlimited); result is
                                 then partial and stcsp_result::truncated is set                   */
    int32_t flags;            /* STCSP_F_*                                                         */
    int32_t reserved;
} stcsp_options;

#define STCSP_F_KEEP_RAW_EDGES 1 /* also keep edges into failed states in the result (debug)       */
#define STCSP_F_NO_EXPORT 2      /* solve() leaves the automaton on the device; call
                                    stcsp_engine_export() to copy it out (bench: HBM-resident)     */
#define STCSP_F_PROFILE 4        /* bracket every k_expand launch with HIP events (roofline)       */
#define STCSP_F_STEPPED 8        /* run the sharded pipeline (leaves emit successor candidates, the
                                    owner commits them: begin/expand_local/outbox/commit/finish) even
                                    with world == 1 -- measures/tests that pipeline on a single GPU   */
#define STCSP_F_INTERVAL_DOMAINS 16 /* hold every variable as an interval (lb, ub per time point) instead of
                                    a bitset: any width in [INT_MIN, INT_MAX]; 2*N*K <= 256 block words */

typedef struct stcsp_counters {
    int64_t search_nodes; /* node expansions = propagation-to-fixpoint + classification; the
                             reference's unit is one solverSolveRe call (solveralgorithm.cpp:733) */
    int64_t gac_calls;    /* generalisedArcConsistent calls (solveralgorithm.cpp:617)             */
    int64_t fails;        /* Solver::numFails  (solveralgorithm.cpp:862,923,936,970)              */
    int64_t dominance;    /* Solver::numDominance (solveralgorithm.cpp:871)                        */
    int64_t leaves;       /* leaf cases reached (solveralgorithm.cpp:739)                          */
    int64_t revisions;    /* arc (reference) / constraint-point (engine) revisions                 */
    int64_t evaluations;  /* constraint-tuple evaluations (validate calls, solveralgorithm.cpp:428)*/
    int64_t levels;       /* engine only: kernel launch rounds                                     */
    double seconds_search;/* wall time of the search phase (automaton resident on device / in RAM) */
    double seconds_export;/* wall time of copying the automaton out + ok-fixpoint                  */
    /* engine only, with STCSP_F_PROFILE: HIP-event time of the dominant kernel (k_expand), summed
       over its launches, on the stream it is launched on */
    double seconds_expand_kernel;
    int64_t expand_launches;
    int64_t wave_revisions; /* engine only: revisions done by a whole wavefront (bitmap / bytecode) */
    int64_t sweeps;         /* engine only: lane-per-item sweeps over the small constraints         */
    int64_t skipped_revisions; /* engine only: revisions skipped because the product to refute
                                  exceeded the per-revision budget (sound, see engine.hip)          */
    int64_t translation_stops; /* engine only: times the device stopped for the host to translate a
                                  constraint set (constraintTranslate, constraint.cpp:540-548)       */
} stcsp_counters;

/* The automaton as the search leaves it in solver->graph, before graphTraverse.
 * State 0 is the root (Signature({},0), solveralgorithm.cpp:951-954); its signature row is
 * all zeros and is not meaningful. Arrays are owned by the engine and stay valid until the
 * next solve()/export() on it or stcsp_engine_destroy(). */
typedef struct stcsp_result {
    int64_t n_states;           /* vertexTable->size(): failed states included                    */
    int32_t sig_len;            /* numSignVar + (#UNTIL constraints)                               */
    int32_t n_sig_vars;         /* Solver::numSignVar                                              */
    int32_t n_until;            /* Solver::numUntil (distinct right-hand vars of `until`)          */
    int32_t n_until_cons;       /* number of UNTIL constraints (one signature flag each)           */
    const int32_t *state_cid;   /* [n_states] Signature::constraintID                              */
    const int32_t *state_sig;   /* [n_states * sig_len] Signature::sigValues                       */
    const uint8_t *state_fail;  /* [n_states] Vertex::fail                                         */
    int64_t n_edges;            /* edges whose destination is not failed (== reference edges)      */
    const int64_t *edge_src;    /* [n_edges] state index                                           */
    const int64_t *edge_dst;    /* [n_edges]                                                       */
    const int32_t *edge_values; /* [n_edges * n_vars] Edge::values: time-0 value of EVERY variable */
    int32_t n_vars;
    int32_t n_constraint_sets;  /* seenConstraints->size()                                         */
    const uint8_t *var_is_signature; /* [n_vars] Variable::isSignature after classification        */
    int32_t root_final;         /* solveralgorithm.cpp:956-964: no UNTIL constraint in the model   */
    int32_t truncated;          /* 1 if a node/time limit stopped the search early                 */
    stcsp_counters counters;
} stcsp_result;

enum stcsp_error {
    STCSP_OK = 0,
    STCSP_E_INVALID = -1,      /* malformed problem descriptor                                     */
    STCSP_E_UNSUPPORTED = -2,  /* feature outside the bitset path (e.g. a domain wider than the
                                  engine's word budget: aux vars of / and % get [INT_MIN,INT_MAX],
                                  solveralgorithm.cpp:316-322)                                     */
    STCSP_E_DEVICE = -3,       /* HIP runtime error / no device                                    */
    STCSP_E_NOMEM = -4,        /* a device pool overflowed and could not grow                      */
    STCSP_E_INTERNAL = -5,     /* watchdog / invariant violation inside a kernel                   */
    STCSP_E_STATE = -6         /* call sequence error                                              */
};

typedef struct stcsp_engine stcsp_engine;

/* Build an engine for one model on one device: classifies the constraints
 * (solverConstraintQueuePush, src/constraint.cpp:254-318), compiles them for the device and
 * allocates the frontier / state-table / edge-log pools. */
int stcsp_engine_create(const stcsp_problem *problem, const stcsp_options *options, stcsp_engine **out);

/* Run the whole search (solveralgorithm.cpp:966-971 and everything it calls) and fill *result
 * with the raw automaton. Blocking. May be called repeatedly (the reference's -t loop,
 * src/solver.cpp:295-349, re-solves the same model). */
int stcsp_engine_solve(stcsp_engine *engine, stcsp_result *result);

/* Copy the device-resident automaton of the last solve() out (only needed with
 * STCSP_F_NO_EXPORT, or per shard in sharded mode). */
int stcsp_engine_export(stcsp_engine *engine, stcsp_result *result);

/* ---- post-search graph passes on the device -------------------
 * Run on the compacted automaton that the last solve()/export() left in HBM; the edge indices of
 * the returned flags are those of that stcsp_result. Replaces, in this order,
 *   graphTraverse         src/graph.cpp:357-418 (called at src/solveralgorithm.cpp:974)   always
 *   adversarialTraverse   src/graph.cpp:304-355 (-a, solveralgorithm.cpp:975-978); the reference
 *                         hard-codes variable index 5 (graph.cpp:329)
 *   adversarialTraverse2  src/graph.cpp:247-302 (-z, solveralgorithm.cpp:980-983); the reference
 *                         hard-codes opponent 5 / avatar 6 (graph.cpp:275)
 * Unsharded engines only (sharded runs post-process the merged automaton on the host). */
typedef struct stcsp_post_options {
    int32_t adversarial_var;  /* variable index for adversarialTraverse, -1 = pass not run          */
    int32_t adversarial2_op;  /* opponent variable for adversarialTraverse2, -1 = pass not run      */
    int32_t adversarial2_ava; /* avatar variable                                                    */
    int32_t reserved;
} stcsp_post_options;

typedef struct stcsp_post_result {
    int64_t n_states, n_edges;  /* sizes of the arrays below (== the exported stcsp_result)          */
    const uint8_t *state_valid; /* [n_states] Vertex::valid after the passes                         */
    const uint8_t *state_final; /* [n_states] Vertex::final                                          */
    const uint8_t *edge_alive;  /* [n_edges] 0 = the reference removed this edge from its EdgeMap    */
    int32_t adver1, adver2;     /* what the reference prints as "adver1: %d; " / "adver2: %d" (the
                                   root's valid flag after the pass), -1 when the pass was not run   */
    int32_t rounds[3];          /* sweeps until the fixpoint: traverse, adversarial, adversarial2    */
    double seconds;             /* wall time of the passes incl. copying the flags out               */
} stcsp_post_result;

int stcsp_engine_postprocess(stcsp_engine *engine, const stcsp_post_options *options, stcsp_post_result *out);

/* ---- bisimulation quotient of the live automaton on the device (no reference counterpart) ---------
 * The live automaton is what solutions.dot shows after stcsp_engine_postprocess(): the states with
 * state_valid set that the root reaches over edges with edge_alive set (a valid root included), and
 * those edges. The projected label of an edge is its `values` restricted to the observable variables.
 * The result is the coarsest partition of the live states in which two states share a class only if
 *   1. they have the same `final` flag, and
 *   2. their live out-edges give the same SET of pairs (projected label, class of the destination):
 * the largest bisimulation, which is unique. The root is an ordinary state; the quotient's root is its
 * class. With every variable observable the live automaton is deterministic and the quotient is its
 * minimal form. Under a projecting mask (the default hides the auxiliary `_V%d` variables of `next`,
 * which carry look-ahead) the projected automaton is nondeterministic: the quotient still accepts the
 * same language but is not guaranteed to be the smallest automaton that does.
 * Valid after stcsp_engine_postprocess() (STCSP_E_STATE before it and after a truncated solve, whose open
 * states have no known language), on unsharded engines (STCSP_E_UNSUPPORTED otherwise: run
 * stcsp_automaton_bisimulation() of stcsp_host.h on the merged automaton). The flags used are the ones
 * postprocess() last wrote, adversarial passes included. A state whose exact comparison with its class
 * representative fails (a collision of the 128-bit signatures the rounds work with) gives
 * STCSP_E_INTERNAL, never a wrong partition. */
typedef struct stcsp_quotient_options {
    const uint8_t *observable; /* [n_vars] nonzero = observable; NULL = every variable whose name does
                                  not start with "_V"                                                  */
    int32_t reserved[2];
} stcsp_quotient_options;

typedef struct stcsp_quotient_result {
    int64_t n_states;           /* live states                                                         */
    int64_t n_classes;
    int64_t n_class_edges;      /* distinct (source class, projected label, destination class)         */
    const int32_t *state_class; /* [stcsp_result::n_states] classes numbered by their least member's
                                   state index (so the root's class is 0); -1 outside the live
                                   automaton. Owned by the engine, valid until the next call on it      */
    int32_t rounds;             /* refinement sweeps, the confirming one included: <= n_states + 1     */
    double seconds;             /* wall time from the flags in HBM to state_class on the host          */
} stcsp_quotient_result;

int stcsp_engine_quotient(stcsp_engine *engine, const stcsp_quotient_options *options, stcsp_quotient_result *out);

/* ---- checking observed streams against the live automaton on the device (no reference counterpart) ----------
 * Live automaton, projected label and default mask as in stcsp_engine_quotient(). A stream is a sequence of `len`
 * steps, each one int32 per observable variable in variable order. With S_0 = {root} (empty without a live root) and
 * S_{t+1} = the live states reached from a state of S_t over a live edge whose projected label equals step t, the
 * answer for a stream is
 *   accepted_len  the largest L <= len with S_L not empty: len exactly when the stream is a prefix of a solution stream
 *                 under the mask (every live state is valid), else the index of the first violating step;
 *   n_end         |S_accepted_len|: 1 for every stream when every variable is observable (the automaton is then
 *                 deterministic), 0 only without a live root;
 *   end_final     1 if some state of S_accepted_len has `final` set.
 * All three are independent of the state numbering and of the GPU's scheduling. A step with a value no edge carries is
 * an ordinary rejection. Both calls are valid where stcsp_engine_quotient() is (STCSP_E_STATE before postprocess() and
 * after a truncated solve, STCSP_E_UNSUPPORTED on sharded engines: stcsp_automaton_check_streams() of stcsp_host.h
 * takes the merged automaton).
 *
 * monitor_build() builds the look-up structures for one mask in HBM: exact ids of the projected labels, and a hash
 * multimap (state, label id) -> destinations. They stay valid until the next solve(), export(), postprocess() or
 * monitor_build() on the engine. monitor_check() walks the streams: one lane per stream while no (state, label) pair
 * has two destinations, else one wavefront per stream with the state sets in LDS. A stream whose set outgrows
 * set_capacity is finished by the host twin, never answered approximately: the result is always exact, and
 * n_host_fallback says how many streams took that road. */
typedef struct stcsp_monitor_options {
    const uint8_t *observable; /* [n_vars] nonzero = observable; NULL = the default mask of stcsp_engine_quotient() */
    int32_t reserved[2];
} stcsp_monitor_options;

typedef struct stcsp_monitor_info {
    int64_t n_states;         /* live states                                                              */
    int64_t n_edges;          /* live edges (entered in the multimap)                                     */
    int64_t n_labels;         /* distinct projected labels                                                */
    int64_t n_pairs;          /* distinct (state, label id) pairs                                         */
    int64_t table_bytes;      /* HBM the look-up structures hold                                          */
    int32_t n_observable;     /* values per step                                                          */
    int32_t max_destinations; /* most distinct destinations of one pair: 1 = deterministic under this mask
                                 (0 without a live edge)                                                  */
    int32_t set_capacity;     /* states a stream's set may hold in the state-set kernel                   */
    int32_t root_live;
    double seconds;           /* wall time from the flags in HBM to the finished structures               */
} stcsp_monitor_info;

#define STCSP_MON_FORCE_SETS 1 /* (tests, measurements) run the state-set kernel under a deterministic mask too */

typedef struct stcsp_monitor_streams {
    int64_t n_streams;
    const int64_t *offsets; /* [n_streams + 1] in steps: offsets[0] == 0, not decreasing, every stream < 2^31 steps */
    const int32_t *values;  /* [offsets[n_streams] * n_observable]                                                  */
    int32_t flags;          /* STCSP_MON_*                                                                          */
    int32_t reserved;
} stcsp_monitor_streams;

typedef struct stcsp_monitor_result {
    int64_t n_streams;
    const int32_t *accepted_len; /* [n_streams] owned by the engine, valid until the next call on it   */
    const int32_t *n_end;        /* [n_streams]                                                        */
    const uint8_t *end_final;    /* [n_streams]                                                        */
    int64_t n_host_fallback;     /* streams finished by the host twin                                  */
    int32_t walk_kernel;         /* 0 none ran, 1 the deterministic walk, 2 the state-set walk         */
    int32_t reserved;
    double seconds;              /* wall time from the host input to the host output                   */
    double seconds_labels;       /* HIP-event time of the step -> label id kernel                      */
    double seconds_walk;         /* HIP-event time of the walk kernel                                  */
} stcsp_monitor_result;

int stcsp_engine_monitor_build(stcsp_engine *engine, const stcsp_monitor_options *options, stcsp_monitor_info *info);
int stcsp_engine_monitor_check(stcsp_engine *engine, const stcsp_monitor_streams *streams, stcsp_monitor_result *result);

/* ---- counting, enumerating and sampling solution prefixes on the device (no reference counterpart) -----------
 * The converse of the monitor. Live automaton and default mask as in stcsp_engine_quotient().
 *
 * Canonical order. The live out-edges of a state are ordered lexicographically by their full value row (edge_values,
 * all n_vars, variable order), ties broken by edge index. The order does not depend on state or edge numbers, so
 * nothing below does.
 *
 * Weights. W_0(s) = 1, or final[s] (0 or 1) with STCSP_GEN_END_FINAL. W_{t+1}(s) = the sum over the live out-edges of
 * s, in canonical order, of W_t(dst): IEEE doubles, added one after the other in that order, starting from 0.
 * count[t] = W_t(root) for t = 0 .. horizon, all 0 without a live root. While a value is below 2^53 it is the exact
 * number of live paths of that length (ending in a final state with STCSP_GEN_END_FINAL), whatever the order of the
 * sums; beyond that it is the double the fixed order gives. If a count[t] is not finite, generator_build() returns
 * STCSP_E_UNSUPPORTED.
 *
 * A stream of length L <= horizon. Start at s = root. For t = 0 .. L-1, with r = L - t and a target tau: go over the
 * live out-edges of s in canonical order with a running sum that starts at 0 and adds W_{r-1}(dst) per edge; take the
 * first edge after whose addition the sum exceeds tau (if rounding lets none exceed it, the last edge of non-zero
 * weight); emit that edge's row projected on the observable variables, in variable order; s = its destination.
 *   sample  (ranks == NULL): tau = u * W_r(s) with u = (double)(z >> 11) * 2^-53 and
 *               z = mix(mix(mix(seed + 0x9e3779b97f4a7c15) + i) + t)                    (i: index of the stream; mod 2^64)
 *               mix(x): x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31
 *           (the splitmix64 finaliser). Nothing is carried from step to step. Every path of length L is drawn with
 *           probability 1 / count[L] while count[L] < 2^53: uniform over PATHS; under a hiding mask two paths may
 *           project on the same stream.
 *   unrank  (ranks[i] given): tau = (double)ranks[i] at t = 0; after each step tau -= the running sum before the
 *           chosen edge. Needs count[L] < 2^53 and ranks[i] < count[L] (else STCSP_E_INVALID). The answer is the
 *           ranks[i]-th path of length L in lexicographic order of its sequence of full rows.
 * A length with count[L] == 0 gives STCSP_E_INVALID. end_final[i] = final[the state stream i ends in].
 *
 * Every floating-point step above is one addition, one subtraction, one multiplication or one comparison of doubles:
 * no fused multiply-add, no reassociation. The device, the host twin (stcsp_automaton_generate() of stcsp_host.h) and
 * any IEEE implementation of this text therefore agree bit for bit, beyond 2^53 too.
 *
 * generator_build() builds, in HBM, the live edges by source in canonical order and the (horizon + 1) x n_states table
 * of weights (STCSP_E_NOMEM if it cannot be allocated). They stay valid until the next solve(), export(),
 * postprocess() or generator_build() on the engine, and live apart from the monitor's structures. Both calls are valid
 * where stcsp_engine_monitor_build() is: STCSP_E_STATE before postprocess(), after a truncated solve and for
 * generate() without valid structures; STCSP_E_UNSUPPORTED on sharded and stepped engines. */
#define STCSP_GEN_END_FINAL 1 /* count and generate only the prefixes that end in a final state */

typedef struct stcsp_generator_options {
    const uint8_t *observable; /* [n_vars] nonzero = observable; NULL = the default mask of stcsp_engine_quotient() */
    int32_t horizon;           /* >= 0: the longest stream generate() may be asked for                              */
    int32_t flags;             /* STCSP_GEN_*                                                                       */
    int32_t reserved[2];
} stcsp_generator_options;

typedef struct stcsp_generator_info {
    int64_t n_states;       /* live states                                                       */
    int64_t n_edges;        /* live edges                                                        */
    int64_t table_bytes;    /* HBM the structures hold                                           */
    const double *count;    /* [horizon + 1] owned by the engine, valid until the next build     */
    int32_t n_observable;   /* values per step                                                   */
    int32_t horizon;
    int32_t max_out_degree; /* most live out-edges of one state                                  */
    int32_t root_live;
    double seconds;         /* wall time from the flags in HBM to the finished structures        */
} stcsp_generator_info;

typedef struct stcsp_generate_request {
    int64_t n_streams;
    const uint64_t *ranks; /* [n_streams] unrank these; NULL = sample */
    uint64_t seed;         /* sample only                             */
    int32_t len;           /* steps per stream, 0 .. horizon          */
    int32_t reserved;
} stcsp_generate_request;

typedef struct stcsp_generate_result {
    int64_t n_streams;
    const int32_t *values;    /* [n_streams * len * n_observable] owned by the engine, valid until the next call on it */
    const uint8_t *end_final; /* [n_streams]                                                                            */
    int32_t len;
    int32_t n_observable;
    double seconds;           /* wall time from the request to the host output */
    double seconds_kernel;    /* HIP-event time of the generate kernel         */
} stcsp_generate_result;

int stcsp_engine_generator_build(stcsp_engine *engine, const stcsp_generator_options *options, stcsp_generator_info *info);
int stcsp_engine_generate(stcsp_engine *engine, const stcsp_generate_request *request, stcsp_generate_result *result);

/* ---- repairing observed streams: the nearest solution prefix, on the device (no reference counterpart) ---------
 * The monitor says where a stream stops being a prefix of a solution; this says which prefix of a solution is the
 * closest one and how far away it is. Live automaton, projected label, default mask and the canonical order of a
 * state's live out-edges (full value row, ties by edge index) are exactly those of stcsp_engine_generate().
 *
 * Input. Streams in the monitor's format (n_streams, offsets in steps, values), weights[n_observable] (int32, each
 * >= 0; NULL = all 1) and flags. A value STCSP_REPAIR_MISSING in a row means "not observed".
 *
 * Step cost. For an edge e with projected row p_e and the observed row x_t:
 *   c_t(e) = the sum over the observable variables v of weights[v] * [x_t[v] != STCSP_REPAIR_MISSING and p_e[v] != x_t[v]].
 *
 * Cost to go, for a stream of len steps. G_0(s) = 0 for every live state (with STCSP_REPAIR_END_FINAL: 0 if final[s],
 * else infinity). G_{r+1}(s) = the minimum over the live out-edges e of s of c_{len-r-1}(e) + G_r(dst(e)); infinity for a
 * state without a live out-edge or when every term is infinite. Infinity is 0xffffffff, finite values are uint32. A
 * request with (the sum of the weights) * (the longest len) > 2^31 - 2 is STCSP_E_INVALID, so no finite value reaches
 * infinity.
 *
 * Answer per stream i.
 *   distance[i]   G_len(root) as int32; -1 if it is infinite or the root is not live. That is no error: the other
 *                 outputs of that stream are then 0.
 *   values        the repaired stream, len rows in the place of the input's. Start at s = root; at step t, with
 *                 r = len - t, take the FIRST live out-edge of s in canonical order with c_t(e) + G_{r-1}(dst) == G_r(s),
 *                 emit its projected row, s = dst. That is the path whose sequence of full rows is lexicographically
 *                 least among the paths of minimum cost: it depends on no state number, edge number or scheduling.
 *   end_final[i]  final[the last s].
 *   n_changed[i]  the (step, variable) positions that were observed (not MISSING) and whose emitted value differs.
 * Everything is integer arithmetic: the device, the host twin (stcsp_automaton_repair_streams() of stcsp_host.h) and any
 * implementation of this text agree exactly.
 *
 * Consequences. With every weight > 0, no MISSING entry and without END_FINAL, distance == 0 exactly when the monitor
 * reports accepted_len == len, and the repaired stream is then the input. Every repaired stream is accepted whole by
 * the monitor under the same mask. A stream of L rows of MISSING repairs to the generator's prefix of rank 0 and length L.
 *
 * repair() needs a valid stcsp_engine_generator_build() on the engine and uses its mask, live set and canonical order;
 * the generator's horizon does not limit len and its STCSP_GEN_END_FINAL is not inherited. Without one: STCSP_E_STATE;
 * STCSP_E_STATE and STCSP_E_UNSUPPORTED otherwise as for stcsp_engine_generate(). Malformed offsets, a negative weight
 * and the bound above: STCSP_E_INVALID. On the first repair after a generator_build() the exact ids of the projected
 * labels are built in HBM (n_labels of them); per step and label the cost is then computed once, and a level of the
 * table reads 4-byte ids, not rows. The request is cut, in its order, into consecutive batches of streams: for each
 * batch the tables [stream][len + 1][n_states] of uint32 and the costs [step][n_labels] of uint32 fit a byte budget,
 * by default half of the free device memory; the environment variable STCSP_REPAIR_BYTES sets it (tests use it to
 * force several batches). STCSP_E_NOMEM only when the table and costs of a SINGLE stream do not fit the budget.
 * STCSP_REPAIR_WAVE_SEGMENT (default 128) sets the out-degree above which a state is relaxed by a whole wavefront
 * instead of one lane (measurements). Results are owned by the engine until the next call on it. The call invalidates
 * neither the generator's nor the monitor's structures. */
#define STCSP_REPAIR_END_FINAL 1           /* the repaired stream must end in a final state */
#define STCSP_REPAIR_MISSING (-2147483647 - 1) /* INT32_MIN in a row: this variable was not observed at this step */
/* INT32_MIN as a label value. A variable whose domain reaches INT32_MIN (interval domains) can carry it on a live edge.
 *   - In an INPUT row of repair() and infer() INT32_MIN always means "not observed": it matches every value, costs
 *     nothing and counts as not observed in n_changed; an observed INT32_MIN cannot be expressed there. The monitor has
 *     no MISSING: in its rows INT32_MIN is the value, matched like any other.
 *   - OUTPUT rows (generate, repaired values, infer's supports and draws, the optimiser's witnesses, observer and compare
 *     labels) carry INT32_MIN wherever the chosen edge has it: there it is a value. The only output rows of MISSING are
 *     the draws of an infeasible stream, which have count == 0.
 * Device, host twin and yardsticks are pinned to this by tests/test_service_shapes_gpu.py. */

typedef struct stcsp_repair_request {
    int64_t n_streams;
    const int64_t *offsets; /* [n_streams + 1] in steps: offsets[0] == 0, not decreasing, every stream < 2^31 steps */
    const int32_t *values;  /* [offsets[n_streams] * n_observable]                                                  */
    const int32_t *weights; /* [n_observable], each >= 0; NULL = all 1                                              */
    int32_t flags;          /* STCSP_REPAIR_*                                                                       */
    int32_t reserved;
} stcsp_repair_request;

typedef struct stcsp_repair_result {
    int64_t n_streams;
    const int32_t *distance;  /* [n_streams] owned by the engine, valid until the next call on it               */
    const int32_t *values;    /* [offsets[n_streams] * n_observable] the repaired rows, at the input's offsets  */
    const uint8_t *end_final; /* [n_streams]                                                                    */
    const int32_t *n_changed; /* [n_streams]                                                                    */
    int64_t n_labels;         /* distinct projected labels of the live automaton                                */
    int64_t table_bytes;      /* HBM of the largest batch: tables and costs                                     */
    int32_t n_batches;
    int32_t n_observable;
    double seconds;           /* wall time from the host input to the host output                               */
    double seconds_relax;     /* HIP-event time of the level-0 and relax kernels, all batches                   */
    double seconds_walk;      /* HIP-event time of the walk kernel, all batches                                 */
    double seconds_cost;      /* HIP-event time of the cost kernel, all batches                                 */
} stcsp_repair_result;

int stcsp_engine_repair(stcsp_engine *engine, const stcsp_repair_request *request, stcsp_repair_result *result);

/* ---- aligning observed streams: repair with dropped and spurious steps, on the device (no reference counterpart) ----
 * The repair keeps step t of the stream at step t of the solution. A recorder that loses a sample or records one twice
 * shifts every later step; this is the weighted edit distance between a stream and the solution language, with the
 * aligned solution prefix. Live automaton, projected label, default mask, canonical order of a state's live out-edges,
 * STCSP_REPAIR_MISSING and the step cost c_t(e) are exactly those of stcsp_engine_repair().
 *
 * Input. Streams in the monitor's format; weights[n_observable] (int32, each >= 0; NULL = all 1); skip_cost (int32 >= 1),
 * the price of dropping one observed step as spurious; gap_cost (int32 >= 1), the price of one solution step the
 * recorder missed; flags.
 *
 * Cost to go, for a stream x_0 .. x_{m-1}: G[t][s], with t steps consumed in the live state s; uint32, infinity is
 * 0xffffffff, infinite terms stay out of every minimum.
 *   base(s)  = 0 for a live state (with STCSP_ALIGN_END_FINAL: 0 if final[s], else infinity).
 *   G[m][s]  = the least fixpoint of G = min(base(s), gap_cost + min over the live out-edges e of s of G[dst(e)]):
 *              base without END_FINAL, gap_cost times the edge distance from s to a final state with it.
 *   B[t][s]  = min(skip_cost + G[t+1][s], min over e of c_t(e) + G[t+1][dst(e)])                      for t < m,
 *   G[t][s]  = the least fixpoint of G = min(B[t][s], gap_cost + min over e of G[dst(e)]).
 * The fixpoint is unique because gap_cost >= 1, so every relaxation order reaches it. A request with
 *   max(the sum of the weights, skip_cost) * (the longest len) + gap_cost * n_states > 2^31 - 2
 * (n_states counts every state of the automaton, live or not) is STCSP_E_INVALID; under that bound no finite value, those
 * in the middle of a relaxation included, reaches infinity.
 *
 * Answer per stream i.
 *   distance[i]  G[0][root] as int32; -1 if it is infinite or the root is not live. That is no error: the stream's other
 *                outputs are then 0 or empty.
 *   The walk starts at (t, s) = (0, root) and takes the FIRST rule that applies:
 *     1. t == m and G[m][s] == base(s): stop.
 *     2. match (t < m): the first live out-edge in canonical order with c_t(e) + G[t+1][dst] == G[t][s]: its projected row
 *        is emitted, op M, go to (t + 1, dst).
 *     3. skip (t < m): skip_cost + G[t+1][s] == G[t][s]: op D, go to (t + 1, s).
 *     4. insert: the first live out-edge in canonical order with gap_cost + G[t][dst] == G[t][s]: its row is emitted,
 *        op I, go to (t, dst).
 *   An insert strictly lowers G within a level, so the walk ends.
 *   out_offsets [n_streams + 1], values: the emitted rows of stream i are the rows out_offsets[i] .. out_offsets[i + 1].
 *   op_offsets [n_streams + 1], ops: uint8, 0 = M, 1 = D, 2 = I, in the order of the walk.
 *   n_changed[i]   the (step, variable) positions of MATCHED steps that were observed and whose emitted value differs.
 *   n_skipped[i], n_inserted[i]   the D and the I ops.  end_final[i]   final[the last s].
 * Everything is integer arithmetic, and no output depends on a state number or on scheduling: the device, the host twin
 * (stcsp_automaton_align_streams() of stcsp_host.h) and any implementation of this text agree exactly.
 *
 * Consequences. #M + #D == len and #M + #I == the number of emitted rows. distance == the matched steps' costs +
 * skip_cost * n_skipped + gap_cost * n_inserted. Every emitted prefix is accepted whole by the monitor under the same
 * mask. With every weight > 0, no MISSING entry and without END_FINAL, distance == 0 exactly when the monitor accepts the
 * stream whole. With skip_cost = gap_cost = d + 1, d the stream's finite repair distance, distance, rows, n_changed and
 * end_final are the repair's and every op is M. With END_FINAL a stream of length 0 yields a shortest path from the root
 * to a final state. One step deleted from a solution prefix: distance <= gap_cost; one duplicated: distance <= skip_cost.
 *
 * align() needs a valid stcsp_engine_generator_build(); without one: STCSP_E_STATE; on a sharded engine
 * STCSP_E_UNSUPPORTED (the host twin takes the merged automaton). Malformed offsets, a negative weight, a cost below 1
 * and the bound: STCSP_E_INVALID. Label ids, costs per (step, label), the table [stream][len + 1][n_states] of uint32,
 * the batches and STCSP_E_NOMEM are the repair's; the byte budget is STCSP_ALIGN_BYTES. Two roads fill the table with the
 * same values (path_kernel): the fused kernel, one workgroup per stream with two rows in LDS and every level in one
 * launch, when n_states <= 20,352 (160 KiB of LDS less 1 KiB, 8 bytes per state); else one launch per level and per
 * closure sweep, the host reading a changed word through pinned memory once per group of sweeps. STCSP_ALIGN_FUSED=0
 * forces the second road; STCSP_ALIGN_FUSED_STATES lowers the capacity of the first (tests). STCSP_REPAIR_WAVE_SEGMENT
 * applies as in the repair. Results are owned by the engine until the next call on it. The call invalidates no other
 * structure and builds none that a later call relies on: its device buffers and one small pinned block are scratch that the
 * engine keeps for reuse until it is destroyed. */
#define STCSP_ALIGN_END_FINAL 1 /* the aligned prefix must end in a final state */

typedef struct stcsp_align_request {
    int64_t n_streams;
    const int64_t *offsets; /* [n_streams + 1] in steps, as for the repair         */
    const int32_t *values;  /* [offsets[n_streams] * n_observable]                 */
    const int32_t *weights; /* [n_observable], each >= 0; NULL = all 1             */
    int32_t skip_cost;      /* >= 1                                                */
    int32_t gap_cost;       /* >= 1                                                */
    int32_t flags;          /* STCSP_ALIGN_*                                       */
    int32_t reserved;
} stcsp_align_request;

typedef struct stcsp_align_result {
    int64_t n_streams;
    const int32_t *distance;    /* [n_streams] owned by the engine, valid until the next call on it */
    const int64_t *out_offsets; /* [n_streams + 1] in rows                                          */
    const int32_t *values;      /* [out_offsets[n_streams] * n_observable] the emitted rows         */
    const int64_t *op_offsets;  /* [n_streams + 1]                                                  */
    const uint8_t *ops;         /* [op_offsets[n_streams]] 0 = M, 1 = D, 2 = I                      */
    const int32_t *n_changed;   /* [n_streams]                                                      */
    const int32_t *n_skipped;   /* [n_streams]                                                      */
    const int32_t *n_inserted;  /* [n_streams]                                                      */
    const uint8_t *end_final;   /* [n_streams]                                                      */
    int64_t n_labels;           /* distinct projected labels of the live automaton                  */
    int64_t table_bytes;        /* HBM of the largest batch: tables and costs                       */
    int32_t n_batches;
    int32_t n_observable;
    int32_t path_kernel;        /* 0 = no batch ran, 1 = fused, 2 = general                         */
    int32_t reserved;
    double seconds;             /* wall time from the host input to the host output                 */
    double seconds_levels;      /* HIP-event time of the levels (either road), all batches          */
    double seconds_walk;        /* HIP-event time of the walk kernel, all batches                   */
    double seconds_cost;        /* HIP-event time of the cost kernel, all batches                   */
} stcsp_align_result;

int stcsp_engine_align(stcsp_engine *engine, const stcsp_align_request *request, stcsp_align_result *result);

/* ---- inferring the unobserved entries of a stream: supports, counts, draws, on the device (no reference counterpart) ----
 * The monitor says whether a stream is a prefix of a solution, the generator gives some solution, the repair the nearest
 * one. This says, for a PARTIALLY observed stream, what the entries that were not seen can be and how many solutions
 * are still consistent with what was seen: the forward-backward pass over (time x automaton). Live automaton,
 * projected label p_e, default mask and the canonical order of a state's live out-edges (full value row, ties by edge
 * index) are exactly those of stcsp_engine_generate() / stcsp_engine_repair().
 *
 * Input. Streams in the repair's format (n_streams, offsets in steps, values), a value STCSP_INFER_MISSING (the same
 * value as STCSP_REPAIR_MISSING) meaning "not observed"; flags; draws >= 0, the number of completions returned per
 * stream; ranks[n_streams * draws] to unrank, NULL to sample with `seed`.
 *
 * Match. Edge e matches the row x_t iff for every observable variable v: x_t[v] == MISSING or p_e[v] == x_t[v].
 *
 * Weight to go, for a stream of len steps. B_0(s) = 1 on the live states (with STCSP_INFER_END_FINAL: final[s]).
 * B_{r+1}(s) = the sum of B_r(dst(e)) over the live out-edges e of s that match step len-r-1, in canonical order:
 * IEEE doubles, added one after the other starting from 0, no fused multiply-add, no reassociation.
 * count[i] = B_len(root), 0 without a live root. Below 2^53 it is the exact number of live paths of len edges from the
 * root whose every edge matches its step (and that end in a final state with END_FINAL). A count may be +inf; all
 * terms are non-negative, so no NaN arises and "> 0" below is exact.
 *
 * Feasible edges. F_0 = {root} if count[i] > 0, else empty. Edge e is feasible at step t iff src(e) is in F_t, e matches
 * x_t and B_{len-t-1}(dst(e)) > 0; F_{t+1} = the destinations of the edges feasible at t. So an edge is feasible at t
 * exactly when some consistent path uses it there.
 *
 * Answer per stream i.
 *   count[i], feasible[i] = count[i] > 0.
 *   support       for every (step t, observable variable v) of the request, in the input's row order: the sorted, distinct
 *                 values p_e[v] over the edges feasible at t, as CSR: support_off[total_steps * n_observable + 1] (int64)
 *                 and support_val[] (int32). An infeasible stream has empty sets; an observed entry of a feasible stream
 *                 has the one-element set of its value.
 *   n_states      |F_t| for t = 0 .. len, at n_states[offsets[i] + i + t]: the number of automaton states the system can
 *                 be in. It does not depend on the state numbering.
 *   values        `draws` completions, draw j of stream i at index q = i * draws + j: len rows at row
 *                 offsets[i] * draws + j * len; end_final[q]. Start at s = root. For t = 0 .. len-1, with r = len - t and
 *                 a target tau: go over the live out-edges of s that match x_t, in canonical order, with a running sum
 *                 that starts at 0 and adds B_{r-1}(dst) per edge; take the first edge after whose addition the sum
 *                 exceeds tau (if rounding lets none exceed it, the last matching edge of non-zero weight); emit its
 *                 projected row; s = dst.
 *                   sample (ranks == NULL): tau = u * B_r(s), u and z = mix(mix(mix(seed + 0x9e3779b97f4a7c15) + q) + t)
 *                     exactly as in stcsp_engine_generate(). Every consistent path is drawn with probability
 *                     1 / count[i] while count[i] < 2^53.
 *                   unrank: tau = (double)ranks[q] at t = 0; after each step tau -= the running sum before the chosen
 *                     edge. Needs count[i] < 2^53 and ranks[q] < count[i], else STCSP_E_INVALID; the ranks of an
 *                     infeasible stream are ignored. The answer is the ranks[q]-th consistent path in lexicographic
 *                     order of its sequence of full rows.
 *                 The draws of an infeasible stream are rows of MISSING with end_final 0. draws > 0 with a feasible
 *                 stream whose count is not finite: STCSP_E_UNSUPPORTED (with draws == 0 everything else is answered).
 * Integers, sets, and doubles added in a fixed order: the device, the host twin (stcsp_automaton_infer_streams() of
 * stcsp_host.h) and any IEEE implementation of this text agree exactly, the doubles bit for bit.
 *
 * Consequences. count > 0 <=> the repair's distance is 0 under all-1 weights and the same END_FINAL. Without a MISSING
 * entry and with every variable observable, count is 0 or 1, and 1 <=> the monitor accepts the stream whole. L rows of
 * MISSING give the generator's count[L] under the same END_FINAL. Every draw agrees with the stream on every observed
 * entry and is accepted whole by the monitor. The draw of rank 0 is the repair's repaired stream at distance 0.
 * Replacing a MISSING entry by a value of its support keeps count > 0, any other value makes it 0, and the counts of the
 * streams so specialised sum to count[i], exactly below 2^53.
 *
 * infer() needs a valid stcsp_engine_generator_build() on the engine and uses its mask, live set and CSR; the generator's
 * horizon does not limit len and its STCSP_GEN_END_FINAL is not inherited. Without one, before postprocess() or after a
 * truncated solve: STCSP_E_STATE; on sharded and stepped engines STCSP_E_UNSUPPORTED; malformed offsets or draws < 0:
 * STCSP_E_INVALID. The exact label ids of stcsp_engine_repair() are built on the first infer or repair after a
 * generator_build() and serve both calls; the first infer adds, per observable variable, the sorted dictionary of the
 * values the labels carry. The request is cut, in its order, into consecutive batches of at most 65,535 streams whose
 * structures fit a byte budget: [stream][len + 1][n_states] doubles (B) and bytes (F), [step][n_labels] bytes twice
 * (match, feasible) and the support bitmaps; by default half of the free device memory, the environment variable
 * STCSP_INFER_BYTES sets it. STCSP_E_NOMEM only when a SINGLE stream does not fit. STCSP_REPAIR_WAVE_SEGMENT applies to
 * the forward sweep as it does to the repair's relaxation. Results are owned by the engine until the next call on it.
 * The call invalidates none of the generator's, monitor's or repair's structures; its own are invalidated wherever the
 * generator's are. */
#define STCSP_INFER_END_FINAL 1            /* count only the completions that end in a final state */
#define STCSP_INFER_MISSING (-2147483647 - 1) /* == STCSP_REPAIR_MISSING; INT32_MIN as a label value: see there */

typedef struct stcsp_infer_request {
    int64_t n_streams;
    const int64_t *offsets; /* [n_streams + 1] in steps: offsets[0] == 0, not decreasing, every stream < 2^31 steps */
    const int32_t *values;  /* [offsets[n_streams] * n_observable]                                                  */
    const uint64_t *ranks;  /* [n_streams * draws] unrank these; NULL = sample                                      */
    uint64_t seed;          /* sample only                                                                          */
    int32_t flags;          /* STCSP_INFER_*                                                                        */
    int32_t draws;          /* >= 0 completions per stream                                                          */
} stcsp_infer_request;

typedef struct stcsp_infer_result {
    int64_t n_streams;
    const double *count;        /* [n_streams] owned by the engine, valid until the next call on it             */
    const uint8_t *feasible;    /* [n_streams]                                                                  */
    const int64_t *support_off; /* [offsets[n_streams] * n_observable + 1]                                      */
    const int32_t *support_val; /* [support_off[last]]                                                          */
    const int32_t *n_states;    /* [offsets[n_streams] + n_streams]: |F_t| at offsets[i] + i + t                */
    const int32_t *values;      /* [offsets[n_streams] * draws * n_observable] the draws                        */
    const uint8_t *end_final;   /* [n_streams * draws]                                                          */
    int64_t n_labels;           /* distinct projected labels of the live automaton                              */
    int64_t table_bytes;        /* HBM of the largest batch: B, F, match, feasible, support bitmaps             */
    int32_t n_batches;          /* 0 without streams or without a live root: nothing runs on the device         */
    int32_t n_observable;
    int32_t draws;
    int32_t reserved;
    double seconds;             /* wall time from the host input to the host output                             */
    double seconds_match;       /* HIP-event times, all batches: the match kernel                               */
    double seconds_backward;    /* level 0, the backward levels and the counts                                  */
    double seconds_forward;     /* the forward levels and |F_t|                                                 */
    double seconds_support;     /* the support bitmaps                                                          */
    double seconds_walk;        /* the draws                                                                    */
} stcsp_infer_result;

int stcsp_engine_infer(stcsp_engine *engine, const stcsp_infer_request *request, stcsp_infer_result *result);

/* ---- posterior marginals of the unobserved entries of a stream, under value weights, on the device (no reference counterpart) ----
 * stcsp_engine_infer() says which values an entry that was not seen can take and how many solution prefixes fit the
 * stream. This says how many of them give each value: the per-edge products A * B of the forward-backward pass, with a
 * weight on every edge. Live automaton, projected label p_e, default mask, the canonical order of a state's live
 * out-edges, the match of an edge and a row, the label ids, the per-variable sorted value dictionaries and
 * vidx[label][v] are exactly those of stcsp_engine_infer().
 *
 * Input. Streams in the repair's / infer's format (n_streams, offsets in steps, values), STCSP_POSTERIOR_MISSING ==
 * STCSP_INFER_MISSING meaning "not observed"; flags; optional value weights as CSR over the observable variables, in
 * mask order: weight_off[n_observable + 1] (int64, weight_off[0] == 0, not decreasing), weight_val[] (int32, strictly
 * increasing inside a variable), weight_w[] (int32, each >= 0). A value that is not listed weighs 1. All three NULL:
 * every value weighs 1. Values out of order or listed twice, a negative weight, malformed offsets or one of the three
 * arrays missing where it is needed: STCSP_E_INVALID.
 *
 * Label weight. w(l) = the product over the observable variables v, in variable order, of the weight of p_l[v]: doubles,
 * starting from 1.0, one multiplication at a time. It may be +inf. The weight of an edge is that of its label.
 *
 * Weight to go, for a stream of len steps. B_0(s) = 1 on the live states (with STCSP_POSTERIOR_END_FINAL: final[s]).
 * B_{r+1}(s) = the sum over the live out-edges e of s, in canonical order, of w(e) * B_r(dst(e)), over the edges that
 * match step len-r-1 and have w(e) > 0 and B_r(dst(e)) > 0. A term that fails one of the three is skipped, not
 * multiplied: 0 * inf never arises, and no NaN. Each term is one multiplication, then one addition to the running sum
 * that starts at 0: IEEE doubles, no fused multiply-add, no reassociation. mass[i] = B_len(root), 0 without a live root.
 * With all weights 1, mass[i] is stcsp_engine_infer()'s count[i], bit for bit.
 *
 * Exactness. exact[i] = mass[i] < 2^53. Every partial result is a non-negative double and rounding is monotone, so a
 * computed root mass below 2^53 means every term under it was below 2^53, hence an exact integer; and on every state s
 * reachable at level t over matching edges of positive weight with weight to go, A_t(s) * B_{len-t}(s) <= mass. For an
 * exact stream every quantity below is therefore an integer below 2^53; the forward pass runs in uint64_t, the order of
 * its additions does not matter, and no floating-point atomic is used anywhere. A stream that is not exact still gets
 * its mass (the double the fixed order gives, possibly +inf), exact = 0, final_mass = 0 and empty marginals: no error,
 * and the other streams of the call are answered in full.
 *
 * Forward, exact streams only. A_0(root) = 1 if mass > 0, 0 elsewhere. Edge e is feasible at t iff A_t(src(e)) > 0, e
 * matches x_t, w(e) > 0 and B_{len-t-1}(dst(e)) > 0. A_{t+1}(d) = the sum over the edges feasible at t into d of
 * A_t(src) * w. With all weights positive this is stcsp_engine_infer()'s feasibility.
 *
 * Answer per stream i.
 *   mass[i], exact[i], feasible[i] = mass[i] > 0.
 *   final_mass[i]  the sum of A_len(s) over the final states s. With END_FINAL it equals mass[i].
 *   marginals      for every (step t, observable variable v) of the request, in the input's row order, as CSR:
 *                  marg_off[total_steps * n_observable + 1] (int64), marg_val[] (int32, sorted, distinct), marg_mass[]
 *                  (uint64): the values a with m(t, v, a) > 0, where m(t, v, a) = the sum over the edges e feasible at
 *                  t with p_e[v] == a of A_t(src) * w(e) * B_{len-t-1}(dst).
 * Integers, and doubles multiplied and added in a fixed order: the device, the host twin
 * (stcsp_automaton_posterior_streams() of stcsp_host.h) and any IEEE implementation of this text agree exactly.
 *
 * Consequences (tests/test_posterior.py checks each).
 *   (a) For every (t, v) of an exact feasible stream the marginal masses sum to mass.
 *   (b) With all weights positive the values of a marginal are exactly stcsp_engine_infer()'s support of that entry.
 *   (c) An observed entry of an exact feasible stream has the one-element marginal {value: mass}.
 *   (d) Replacing a MISSING entry by a value a gives a stream whose mass is m(t, v, a); a value outside the marginal
 *       gives 0.
 *   (e) A weight of 0 on a value gives what deleting every edge that carries it would give.
 *   (f) Multiplying every weight of one variable by c multiplies mass and every marginal by c^len, while exact.
 *   (g) L rows of MISSING with all weights 1 give the generator's count[L] under the same END_FINAL.
 *
 * posterior() needs a valid stcsp_engine_generator_build() and builds or reuses the repair's label ids and the infer's
 * dictionaries. STCSP_E_STATE, STCSP_E_UNSUPPORTED and STCSP_E_INVALID as for stcsp_engine_infer(). The label weights
 * are computed once per call in one launch over the labels. The request is cut, in its order, into consecutive batches
 * of at most 65,535 streams whose structures fit a byte budget: [stream][len + 1][n_states] doubles (B), two rolling
 * rows [stream][2][n_states] of uint64 (A: the marginals of step t need A_t only), [step][n_labels] bytes (match) and
 * uint64 (the per-label masses) and [step][bins] uint64, one bin per (variable, dictionary value); by default half of
 * the free device memory, the environment variable STCSP_POSTERIOR_BYTES sets it. STCSP_E_NOMEM only when a SINGLE
 * stream does not fit. STCSP_REPAIR_WAVE_SEGMENT applies to the forward sweep as in infer. Results are owned by the
 * engine until the next call on it. The call invalidates nothing of the generator, monitor, repair or infer; its own
 * structures fall wherever the generator's do. */
#define STCSP_POSTERIOR_END_FINAL 1             /* only the completions that end in a final state */
#define STCSP_POSTERIOR_MISSING (-2147483647 - 1) /* == STCSP_INFER_MISSING */

typedef struct stcsp_posterior_request {
    int64_t n_streams;
    const int64_t *offsets;    /* [n_streams + 1] in steps: offsets[0] == 0, not decreasing, every stream < 2^31 steps */
    const int32_t *values;     /* [offsets[n_streams] * n_observable]                                                  */
    const int64_t *weight_off; /* [n_observable + 1]; NULL with the two below = every value weighs 1                   */
    const int32_t *weight_val; /* [weight_off[n_observable]] strictly increasing inside a variable                     */
    const int32_t *weight_w;   /* [weight_off[n_observable]] each >= 0                                                 */
    int32_t flags;             /* STCSP_POSTERIOR_*                                                                    */
    int32_t reserved;
} stcsp_posterior_request;

typedef struct stcsp_posterior_result {
    int64_t n_streams;
    const double *mass;         /* [n_streams] owned by the engine, valid until the next call on it             */
    const uint8_t *exact;       /* [n_streams] mass < 2^53                                                      */
    const uint8_t *feasible;    /* [n_streams] mass > 0                                                         */
    const uint64_t *final_mass; /* [n_streams]                                                                  */
    const int64_t *marg_off;    /* [offsets[n_streams] * n_observable + 1]                                      */
    const int32_t *marg_val;    /* [marg_off[last]]                                                             */
    const uint64_t *marg_mass;  /* [marg_off[last]]                                                             */
    int64_t n_labels;           /* distinct projected labels of the live automaton                              */
    int64_t table_bytes;        /* HBM of the largest batch: B, A, match, per-label masses, bins                */
    int32_t n_batches;          /* 0 without streams or without a live root: nothing runs on the device         */
    int32_t n_observable;
    double seconds;             /* wall time from the host input to the host output                             */
    double seconds_weights;     /* HIP-event times, all batches: the label weights and the match kernel         */
    double seconds_backward;    /* level 0, the backward levels and the masses                                  */
    double seconds_forward;     /* the forward levels and final_mass                                            */
    double seconds_bins;        /* the bins                                                                     */
} stcsp_posterior_result;

int stcsp_engine_posterior(stcsp_engine *engine, const stcsp_posterior_request *request, stcsp_posterior_result *result);

/* ---- the observer of the live automaton: subset construction on the device (no reference counterpart) ----------------
 * Under a mask that hides a variable the live automaton is nondeterministic in its projected labels. The observer is the
 * deterministic automaton whose states are the sets of automaton states the system can be in after an observed prefix:
 * the state estimator of the partially observed system. Live automaton, projected label p_e, default mask and label ids
 * are those of the last stcsp_engine_generator_build() on the engine; its horizon and flags play no part.
 *
 * Definition. D_0 = {root}. delta(D, l) = { dst(e) : e a live edge, src(e) in D, p_e = l }, defined when it is not empty.
 * The observer's states are the sets reachable from D_0, its edges the triples (D, l, delta(D, l)). final(D) = some member
 * of D is final (the monitor's end_final). Without a live root the observer is empty: n_states == 0, and the call succeeds.
 *
 * Canonical numbering. Breadth-first from D_0 = number 0, the out-edges of a state taken in lexicographic order of their
 * projected rows (the convention of the canonical text and of stcsp_automaton_quotient()). Edges are returned sorted by
 * (source number, projected row). Nothing in the result depends on state numbers, edge numbers or scheduling, except that
 * the members of a set are named by their stcsp_result state index (ascending within a set).
 *
 * Consequences. Under a mask with every variable observable every set is a singleton and the observer is the live
 * automaton. A stream the monitor accepts for accepted_len steps with n_end states drives the observer for accepted_len
 * steps into the one state D with |D| == n_end and final(D) == end_final. Paths of the observer and distinct observable
 * streams correspond one to one. Folding the observer with the bisimulation quotient under the same mask gives the minimal
 * deterministic automaton of the observable language.
 *
 * Limits. options.max_states bounds the observer's states; 0 selects the default 2^26. The pool of member lists (4 bytes
 * per member of every set) and the scratch of one level are bounded by a byte budget, by default half of the free device
 * memory; the environment variable STCSP_OBSERVER_BYTES sets it. A frontier whose work items would not fit is cut into
 * chunks. Exceeding either limit gives STCSP_E_NOMEM with a message that names the limit and how far the construction
 * got; there is never a partial result, the engine stays usable, and the generator's, monitor's, repair's and inference's
 * structures stay valid. Sets of any size up to the number of live states are built on the device: a set lives as a
 * bitset over the states in LDS (up to 262,144 states) or in a slice of global scratch per workgroup;
 * STCSP_OBSERVER_GLOBAL_SCRATCH=1 forces the second road (tests).
 *
 * Needs a valid stcsp_engine_generator_build(): without one, before stcsp_engine_postprocess() and after a truncated solve
 * STCSP_E_STATE; on sharded and stepped engines STCSP_E_UNSUPPORTED (run stcsp_automaton_observer() of stcsp_host.h on the
 * merged automaton). Sets are interned by a 64-bit hash; every set that finds an existing entry is compared with its
 * member list exactly, and a difference (a collision of the hash) gives STCSP_E_INTERNAL, never a wrong automaton.
 * Results are owned by the engine until the next call on it. */
typedef struct stcsp_observer_options {
    int64_t max_states; /* 0 = the default (2^26) */
    int32_t reserved[2];
} stcsp_observer_options;

typedef struct stcsp_observer_result {
    int64_t n_states, n_edges;
    const int64_t *member_off;  /* [n_states + 1] into member[]                                                       */
    const int32_t *member;      /* [member_off[n_states]] stcsp_result state indices, ascending within a set          */
    const uint8_t *state_final; /* [n_states]                                                                         */
    const int32_t *edge_src;    /* [n_edges] observer numbers; edges sorted by (source, projected row)                */
    const int32_t *edge_dst;    /* [n_edges]                                                                          */
    const int32_t *edge_values; /* [n_edges * n_observable] the projected rows                                        */
    int64_t n_labels;           /* distinct projected labels of the live automaton                                    */
    int64_t max_set;            /* the largest set                                                                    */
    int64_t table_bytes;        /* HBM the construction held at its end: pool, records, tables, edge log, scratch     */
    int32_t n_observable;
    int32_t levels;             /* breadth-first levels, the root's included                                          */
    double seconds;             /* wall time from the generator's structures in HBM to the result on the host         */
    double seconds_build;       /* HIP-event time of the ordering kernel (first call after a generator_build())       */
    double seconds_items;       /* HIP-event time of the item kernels, all levels                                     */
    double seconds_intern;      /* HIP-event time of the intern launches, all levels                                  */
    double seconds_commit;      /* HIP-event time of the write and verify launches, all levels                        */
} stcsp_observer_result;

int stcsp_engine_observer(stcsp_engine *engine, const stcsp_observer_options *options, stcsp_observer_result *result);

/* ---- comparing two observable languages: inclusion and shortest witnesses on the device (no reference counterpart) ----
 * Do two models show the same streams, and if not, which is the shortest stream one admits and the other does not? The
 * call builds the synchronous product of two deterministic automata and reads four inclusions off it.
 *
 * Operands. The left operand L is the observer that the last successful stcsp_engine_observer() built on this engine,
 * under that call's mask. The engine keeps what it needs of it; stcsp_engine_compare() does not disturb it, so several
 * right operands can be compared against one observer. A new solve, new flags, a new stcsp_engine_generator_build() and
 * a failed stcsp_engine_observer() end its validity. The right operand R is a deterministic labelled automaton in the
 * layout of stcsp_observer_result, of which only n_states, n_edges, state_final, edge_src, edge_dst, edge_values and
 * n_observable are read: state 0 is the root, n_states == 0 is an automaton without states, and its rows are in the
 * column order of this engine's observable variables (the caller's job). STCSP_E_INVALID when n_observable differs from
 * the left's, an index is out of range, the edges are not sorted by (source, row), or two edges share (source, row).
 *
 * Languages. For a deterministic automaton X, P(X) is the set of row sequences that have a run from the root (it holds
 * the empty sequence iff X has a state), and F(X) the subset whose run ends in a final state.
 *
 * Product. Each operand is completed with a sink _|_ that is not final and that every missing (state, row) leads to. The
 * product's states are the pairs (l, r) != (_|_, _|_) reachable from (root of L or _|_, root of R or _|_); a pair has one
 * edge per row that at least one of its components has. Pairs are numbered breadth-first from the root pair, the
 * out-edges of a pair taken in lexicographic order of their rows (the observer's convention). So the least-numbered pair
 * that satisfies a predicate is reached by the shortest row sequence that reaches such a pair, and by the
 * lexicographically least among those. Nothing in the result depends on scheduling.
 *
 * Verdicts. Verdict k is the least-numbered pair that satisfies predicate k, or none:
 *   0  refutes P(L) in P(R):  l != _|_ and r == _|_
 *   1  refutes P(R) in P(L):  r != _|_ and l == _|_
 *   2  refutes F(L) in F(R):  l != _|_, final(l), and (r == _|_ or not final(r))
 *   3  refutes F(R) in F(L):  r != _|_, final(r), and (l == _|_ or not final(l))
 * witness_len[k] == -1 means the inclusion holds. Otherwise the witness is the pair's access sequence: witness_len[k]
 * rows of n_observable values at witness_values + witness_off[k] * n_observable (witness_off counts rows), and
 * witness_left[k] / witness_right[k] are the pair's components, -1 for _|_. The whole product is always explored.
 *
 * Limits. request.max_pairs bounds the pairs; 0 selects the default 2^26. The table, the records of the pairs and the
 * scratch of a level are bounded by a byte budget, by default half of the free device memory; the environment variable
 * STCSP_COMPARE_BYTES sets it. Exceeding either limit gives STCSP_E_NOMEM with a message that names the limit, the level
 * and the pairs so far; there is never a partial result, and the engine, the observer and the generator's, monitor's,
 * repair's and inference's structures stay valid. STCSP_COMPARE_SLOTS sets the initial slot count of the table (tests:
 * the table grows by rehashing between launches). STCSP_E_STATE without a valid observer; STCSP_E_UNSUPPORTED on sharded
 * and stepped engines (run stcsp_compare_observers() of stcsp_host.h on two observers). Results are owned by the engine
 * until the next call on it. */
typedef struct stcsp_compare_request {
    const stcsp_observer_result *right;
    int64_t max_pairs; /* 0 = the default (2^26) */
    int32_t reserved[2];
} stcsp_compare_request;

typedef struct stcsp_compare_result {
    int64_t n_pairs, n_pair_edges;
    int64_t witness_off[5];        /* in rows: witness k is rows [witness_off[k], witness_off[k + 1])                    */
    const int32_t *witness_values; /* [witness_off[4] * n_observable]                                                   */
    int32_t witness_len[4];        /* -1: the inclusion holds                                                           */
    int32_t witness_left[4];       /* the witness pair's state of L, -1 for the sink                                    */
    int32_t witness_right[4];      /* ... and of R                                                                      */
    int64_t table_bytes;           /* HBM the comparison held at its end: operands, table, records, scratch of a level  */
    int32_t n_observable;
    int32_t levels;                /* breadth-first levels, the root pair's included                                    */
    double seconds;                /* wall time from the request to the result on the host                              */
    double seconds_expand;         /* HIP-event time of the expansion launches, all levels                              */
    double seconds_number;         /* HIP-event time of the collect and number launches, all levels                     */
} stcsp_compare_result;

int stcsp_engine_compare(stcsp_engine *engine, const stcsp_compare_request *request, stcsp_compare_result *result);

/* ---- strongly connected components and lasso solutions on the device (no reference counterpart) ----------------------
 * Every other service speaks about finite prefixes; a solution of a stream CSP is an infinite stream. This call answers the
 * questions about it: is there an infinite solution, which long-run regimes (components) exist, which states are only
 * passed through, and what does one ultimately periodic solution stem . loop^omega look like.
 *
 * Live automaton, flags and validity are those of stcsp_engine_quotient(): the flags the last stcsp_engine_postprocess()
 * wrote, adversarial passes included; STCSP_E_STATE before it and after a truncated solve; STCSP_E_UNSUPPORTED on sharded
 * engines (run stcsp_automaton_components() of stcsp_host.h on the merged automaton). The call touches no other service's
 * state: the monitor's, generator's, repair's and inference's structures, the observer and the compare operand stay valid.
 *
 * Components. state_component[s] is the strongly connected component of the live state s over the live edges, -1 outside
 * the live automaton. Components are numbered by their least member's state index (the quotient's rule), so the numbers
 * follow this solve's state numbering while the partition does not. Per component: comp_size, comp_depth (the least number
 * of steps from the root to a member) and comp_flags:
 *   STCSP_SCC_CYCLIC     more than one state, or a live self-loop
 *   STCSP_SCC_FINAL      holds a final state
 *   STCSP_SCC_BOTTOM     no live edge leaves it
 *   STCSP_SCC_ACCEPTING  CYCLIC and FINAL
 * state_omega[s] == 1 when s reaches an accepting component: Buechi acceptance on `final`, the state starts an infinite run
 * that is final infinitely often. root_omega == 1 is "the model has an infinite solution".
 *
 * Lassos. options.max_lassos asks for them: 0 none, -1 all, n > 0 the first n. STCSP_SCC_LASSO_BOTTOM keeps only the
 * accepting components that are bottom. The candidates are the accepting components (the root reaches every live
 * component), taken in order of (comp_depth, component number); so which components of equal depth survive a truncating
 * max_lassos follows this solve's state numbering. For a component c,
 *   stem  is the shortest sequence of full label rows (all n_vars variables, in variable order) from the root to a final
 *         state of c, and among the shortest the lexicographically least (length 0 when the root is such a state); its
 *         end state is the anchor;
 *   loop  is the shortest sequence, of at least one row, from the anchor back to the anchor over edges inside c, and among
 *         the shortest the lexicographically least.
 * The live automaton is deterministic under full labels, so both are unique and depend on neither scheduling nor state
 * numbering; two live out-edges of one state with the same full row, met on a walk, give STCSP_E_INTERNAL. Lasso i belongs
 * to component lasso_component[i] and is the rows [lasso_off[i], lasso_off[i + 1]) of lasso_values: lasso_stem_len[i] rows
 * of stem, then the loop.
 *
 * STCSP_SCC_NO_TRIM (tests, measurements) lets the colouring rounds find every component, the trivial ones included; the
 * result is the same. A pass that has not converged after n_states + 8 rounds gives STCSP_E_INTERNAL. Results are owned by
 * the engine until the next call on it. */
#define STCSP_SCC_LASSO_BOTTOM 1 /* options.flags: lassos of bottom accepting components only                        */
#define STCSP_SCC_NO_TRIM 2      /* options.flags: no trimming, colouring alone                                        */
#define STCSP_SCC_CYCLIC 1       /* comp_flags                                                                         */
#define STCSP_SCC_FINAL 2
#define STCSP_SCC_BOTTOM 4
#define STCSP_SCC_ACCEPTING 8

typedef struct stcsp_components_options {
    int64_t max_lassos; /* 0 = none, -1 = all */
    int32_t flags;      /* STCSP_SCC_LASSO_BOTTOM | STCSP_SCC_NO_TRIM */
    int32_t reserved;
} stcsp_components_options;

typedef struct stcsp_components_result {
    int64_t n_states; /* live states */
    int64_t n_components, n_cyclic, n_accepting, n_bottom;
    int64_t n_omega;                /* live states with state_omega set                                                  */
    const int32_t *state_component; /* [stcsp_result::n_states], -1 outside the live automaton                           */
    const uint8_t *state_omega;     /* [stcsp_result::n_states]                                                          */
    const int32_t *comp_size;       /* [n_components]                                                                    */
    const int32_t *comp_depth;      /* [n_components]                                                                    */
    const int32_t *comp_flags;      /* [n_components] STCSP_SCC_CYCLIC | FINAL | BOTTOM | ACCEPTING                      */
    int64_t n_lassos;
    const int32_t *lasso_component; /* [n_lassos]                                                                        */
    const int64_t *lasso_off;       /* [n_lassos + 1] in rows                                                            */
    const int32_t *lasso_stem_len;  /* [n_lassos]                                                                        */
    const int32_t *lasso_values;    /* [lasso_off[n_lassos] * n_vars]                                                    */
    int32_t n_vars;
    int32_t root_omega;
    int32_t rounds[3];      /* trim rounds, colouring rounds, launches of sweep kernels in all (0 on the host twin)      */
    int32_t reserved;
    double seconds;         /* wall time from the flags in HBM to the result on the host                                 */
    double seconds_kernels; /* HIP-event time of the launches, all phases (0 on the host twin)                           */
} stcsp_components_result;

int stcsp_engine_components(stcsp_engine *engine, const stcsp_components_options *options, stcsp_components_result *result);

/* ---- optimal solution streams on the device: least cost per length, least mean (no reference counterpart) -----------
 * Which solution is BEST under an objective: a linear integer cost over the values on an edge,
 *   c(e) = sum over the variables v of weights[v] * edge_values[e][v]        (int64),
 * minimised exactly in two ways over the live automaton.
 *
 * Live automaton, flags and validity are those of stcsp_engine_quotient() and stcsp_engine_components(): the flags of the
 * last stcsp_engine_postprocess(); STCSP_E_STATE before it and after a truncated solve; STCSP_E_UNSUPPORTED on sharded
 * engines (run stcsp_automaton_optimise() of stcsp_host.h on the merged automaton). The call keeps its own buffers and
 * leaves the monitor, generator, repair, inference, observer and compare operand valid. With STCSP_OPT_MEAN it runs the
 * component pass of stcsp_engine_components() itself (no lassos): the result pointers of an earlier
 * stcsp_engine_components() call are then no longer valid. It invalidates nothing else. Results are owned by the engine
 * until the next call on it.
 *
 * Request. weights[n_vars]: one int32 per variable of the full label row (callers give the auxiliary variables 0; the
 * engine does not care). horizon >= 0. lengths[n_lengths]: the lengths for which a witness is wanted, each in 0 .. horizon.
 * STCSP_OPT_MAXIMISE is done on the host: the weights are negated, the kernels minimise, and every reported cost and
 * numerator is negated again. With cmax = sum of |weights[v]| * max(|lb[v]|, |ub[v]|): cmax * max(horizon, 1) > 2^62 is
 * STCSP_E_INVALID, as are horizon < 0, a length outside 0 .. horizon, n_lengths < 0 and a null weights.
 *
 * Finite horizon. best[L], L = 0 .. horizon: the least sum of c(e) over the paths of L live edges from the root; with
 * STCSP_OPT_END_FINAL over those that end in a final state. STCSP_OPT_NONE (INT64_MAX, also under MAXIMISE) where there
 * is no such path; best[0] is 0, or NONE under END_FINAL with a root that is not final. No live root: NONE everywhere, no
 * error. With STCSP_OPT_STATE_BEST, state_best[s] is the same quantity for L = horizon from every live state s, NONE
 * outside the live automaton (NULL without the flag).
 * Witness i belongs to lengths[i] and is the rows [witness_off[i], witness_off[i + 1]) of witness_values (full label rows,
 * n_vars values each); witness_states holds, row by row, the state the step enters (every walk starts at the root, state
 * 0). It is empty when best[lengths[i]] is NONE. The walk: with k steps left in state s (V_k = the least cost of k steps
 * from a state), take the live out-edge with the least full row among those with c(e) + V_{k-1}[dst] == V_k[s]. The live
 * automaton is deterministic under full rows, so the witness is the lexicographically least prefix that attains
 * best[L]; two equal rows among the candidates of one step give STCSP_E_INTERNAL.
 *
 * Long run (STCSP_OPT_MEAN). n_components and state_component exactly as stcsp_engine_components() numbers them.
 * comp_mean_num[c] / comp_mean_den[c]: the minimum cycle mean (Karp) of component c over the live edges with both ends in
 * c, a reduced fraction with den > 0; num == den == 0 for a component that is not STCSP_SCC_CYCLIC. omega_mean_num /
 * omega_mean_den and omega_component: the least mean over the STCSP_SCC_ACCEPTING components, ties to the least component
 * number; den == 0 and component -1 when the model has no infinite solution. This is the INFIMUM of the long-run mean
 * cost over the infinite solutions: a lasso attains it only if a least-mean cycle passes a final state, which is always
 * so in a model without `until` constraints (every state is final there). The rational comparisons cross-multiply in
 * int64: with nmax the size of the largest cyclic component, nmax^2 * cmax > 2^62 is STCSP_E_UNSUPPORTED with a message
 * that names both numbers. Without the flag n_components is 0 and the omega fields are 0, 0, -1.
 *
 * Memory: two rows of n_states int64 without witnesses, horizon + 1 with them, besides the live edges (20 B each) and,
 * with MEAN, 44 B per state. All of it is counted against a byte budget (the environment's STCSP_OPTIMISE_BYTES, else half
 * of the free device memory): beyond it STCSP_E_NOMEM with a message that names the limit and the need, never a partial
 * result. */
#define STCSP_OPT_MAXIMISE 1
#define STCSP_OPT_END_FINAL 2
#define STCSP_OPT_MEAN 4
#define STCSP_OPT_STATE_BEST 8
#define STCSP_OPT_NONE INT64_MAX

typedef struct stcsp_optimise_request {
    const int32_t *weights; /* [n_vars]                                 */
    const int32_t *lengths; /* [n_lengths], each in 0 .. horizon        */
    int32_t horizon;
    int32_t n_lengths;
    int32_t flags; /* STCSP_OPT_*                                       */
    int32_t reserved;
} stcsp_optimise_request;

typedef struct stcsp_optimise_result {
    int64_t n_states;              /* live states                                                                       */
    const int64_t *best;           /* [horizon + 1]                                                                     */
    const int64_t *state_best;     /* [stcsp_result::n_states] with STCSP_OPT_STATE_BEST, else NULL                     */
    int64_t n_witnesses;           /* == n_lengths                                                                      */
    const int64_t *witness_off;    /* [n_witnesses + 1] in rows                                                         */
    const int32_t *witness_values; /* [witness_off[n_witnesses] * n_vars]                                               */
    const int32_t *witness_states; /* [witness_off[n_witnesses]] the state every step enters                            */
    int64_t n_components;          /* with STCSP_OPT_MEAN, else 0                                                       */
    const int32_t *state_component; /* [stcsp_result::n_states] with STCSP_OPT_MEAN, else NULL                          */
    const int64_t *comp_mean_num;  /* [n_components]                                                                    */
    const int64_t *comp_mean_den;  /* [n_components]                                                                    */
    int64_t omega_mean_num, omega_mean_den;
    int32_t omega_component;
    int32_t n_vars;
    int32_t horizon;
    int32_t largest_cyclic; /* nmax: the size of the largest cyclic component (0 without STCSP_OPT_MEAN)                */
    int32_t rounds[2];      /* launches of the finite-horizon kernels, of the Karp kernels (0 on the host twin)         */
    double seconds;         /* wall time from the flags in HBM to the result on the host                                */
    double seconds_kernels; /* HIP-event time of the launches (0 on the host twin)                                      */
} stcsp_optimise_result;

int stcsp_engine_optimise(stcsp_engine *engine, const stcsp_optimise_request *request, stcsp_optimise_result *result);

/* ---- temporal queries over the infinite solutions on the device: fair CTL (no reference counterpart) ------------------
 * "Can GAMEOVER == 1 always be avoided", "is it inevitable", "can the system always get back to m == 0": properties of the
 * branching structure of the INFINITE solutions, the streams stcsp_engine_components() speaks about.
 *
 * ONLY SOLUTIONS ARE QUANTIFIED OVER. A prefix that cannot be continued to an infinite solution does not exist for this
 * call: it is neither a witness of an E nor a counterexample of an A.
 *
 * Worlds. A world is one step on an infinite solution: a live edge e (alive, both ends live) with state_omega[dst(e)] == 1.
 * Live, flags and validity are exactly those of stcsp_engine_components(). The successors of a world e are the worlds f
 * with src(f) == dst(e); every world has at least one. The initial worlds are the worlds that leave the root (state 0).
 * Solutions. A solution from w is an infinite sequence of worlds w0 = w, w(i+1) a successor of w(i), with
 * final[dst(w(i))] set for infinitely many i (the Buechi condition of stcsp_engine_components()). Every world starts at
 * least one. A model without an infinite solution has 0 worlds: every query on it is vacuous (n_initial == 0), not an error.
 *
 * Atoms hold on a world and are read from that edge's full value row: NAME op INT and NAME op NAME with op one of
 * == != < <= > >=, compared as int32 (INT_MIN is a value), and true and false. Formulas: the connectives ! & | -> and the
 * temporal operators EX f, EF f, EG f, E[f U g], AX f, AF f, AG f, A[f U g] with their standard CTL meaning, the path
 * quantifiers ranging over the solutions from the world.
 *
 * Request: a postfix program of int32 words. An atom is its token followed by its operands:
 *   STCSP_CTL_TRUE | STCSP_CTL_FALSE
 *   STCSP_CTL_CMP_CONST var op value      STCSP_CTL_CMP_VAR var op var2      (op: STCSP_CTL_OP_*)
 *   STCSP_CTL_NOT (1 operand)  STCSP_CTL_AND | OR | IMPLIES (2)  STCSP_CTL_EX | EF | EG | AX | AF | AG (1)
 *   STCSP_CTL_EU | STCSP_CTL_AU (2: f then g)
 * (stcsp_ctl_parse() of stcsp_host.h writes it from text). A malformed program is STCSP_E_INVALID: stack underflow, a
 * variable index or comparison outside its range, an unknown token, leftover operands, an empty program.
 *
 * Lowering, on the host, to the basis {atoms, !, &, |, EX, EU, EG}:  f -> g = !f | g,  EF f = E[true U f],
 * AX f = !EX !f,  AG f = !E[true U !f],  AF f = !EG !f,  A[f U g] = !E[!g U (!f & !g)] & !EG !g.  Double negations are
 * not removed. Limits, on the LOWERED program (STCSP_E_UNSUPPORTED beyond them, with a message): STCSP_CTL_MAX_NODES atoms
 * and operators in all (A[f U g] counts f once and g three times), a maximal temporal-free subformula whose postfix
 * evaluation needs a stack deeper than 64, and STCSP_CTL_MAX_SLOTS sets of worlds held at once (an operand pair holds the
 * first set while the second is computed; EG holds three).
 *
 * Evaluation (every world is fair: it starts a solution):  EX f: some successor is in f.  E[f U g]: the least fixpoint
 * Z = g | (f & EX Z).  EG f: Emerson-Lei, the greatest fixpoint Z = f & EX E[f U (Z & Fin)] with Fin(e) = final[dst(e)];
 * every outer round runs an inner EU to its own fixpoint. A fixpoint that has not converged after n_worlds + 8 rounds is
 * STCSP_E_INTERNAL.
 *
 * Verdict. n_worlds, n_initial, n_initial_sat and per exported edge two bytes: edge_world[e] (e is a world) and edge_sat[e]
 * (the formula holds there; 0 outside the worlds). "Holds for the model" is n_initial_sat == n_initial; "possible" is
 * n_initial_sat > 0.
 *
 * Witness (flags & STCSP_CTL_WITNESS). When the lowered top operator is EX or EU and some initial world satisfies it, a
 * witness; when the top is !EX or !EU and some initial world fails it, a counterexample (a witness of the operand). For EU
 * it is the shortest sequence of worlds from an initial world that stays in sat(f) and ends in sat(g); for EX, two worlds,
 * the second in sat(f). Among the shortest the lexicographically least by full rows, the choice of the initial world being
 * part of the minimisation (the walk of stcsp_engine_components()). witness_kind is STCSP_CTL_NONE, STCSP_CTL_IS_WITNESS or
 * STCSP_CTL_IS_COUNTEREXAMPLE; witness_values holds witness_len full rows. Two equal full rows among the candidates of a
 * step give STCSP_E_INTERNAL. No lasso is built for EG / AF: the result says STCSP_CTL_NONE.
 *
 * Errors. STCSP_E_STATE before stcsp_engine_postprocess() and after a truncated solve; STCSP_E_UNSUPPORTED on sharded
 * engines (run stcsp_automaton_ctl() of stcsp_host.h on the merged automaton) and over the limits; STCSP_E_INVALID as above;
 * STCSP_E_NOMEM over the byte budget (the environment's STCSP_CTL_BYTES, else half of the free device memory), checked once
 * the worlds are counted and before any set is computed, with a message that names the need and the limit. Memory: 12 B per
 * world, 14 B per state, 2 B per exported edge, one bit per world and held set, 8 B per world with a witness.
 *
 * The call runs the component pass of stcsp_engine_components() itself (no lassos): the result pointers of an earlier
 * stcsp_engine_components() call are then no longer valid. It invalidates nothing else. Results are owned by the engine
 * until the next call on it. */
#define STCSP_CTL_TRUE 1
#define STCSP_CTL_FALSE 2
#define STCSP_CTL_CMP_CONST 3
#define STCSP_CTL_CMP_VAR 4
#define STCSP_CTL_NOT 10
#define STCSP_CTL_AND 11
#define STCSP_CTL_OR 12
#define STCSP_CTL_IMPLIES 13
#define STCSP_CTL_EX 20
#define STCSP_CTL_EF 21
#define STCSP_CTL_EG 22
#define STCSP_CTL_EU 23
#define STCSP_CTL_AX 24
#define STCSP_CTL_AF 25
#define STCSP_CTL_AG 26
#define STCSP_CTL_AU 27
#define STCSP_CTL_OP_EQ 0
#define STCSP_CTL_OP_NE 1
#define STCSP_CTL_OP_LT 2
#define STCSP_CTL_OP_LE 3
#define STCSP_CTL_OP_GT 4
#define STCSP_CTL_OP_GE 5
#define STCSP_CTL_WITNESS 1 /* request.flags */
#define STCSP_CTL_NONE 0    /* witness_kind */
#define STCSP_CTL_IS_WITNESS 1
#define STCSP_CTL_IS_COUNTEREXAMPLE 2
#define STCSP_CTL_MAX_NODES 256
#define STCSP_CTL_MAX_SLOTS 16

typedef struct stcsp_ctl_request {
    const int32_t *program; /* [n_words] postfix                        */
    int32_t n_words;
    int32_t flags; /* STCSP_CTL_WITNESS                                 */
} stcsp_ctl_request;

typedef struct stcsp_ctl_result {
    int64_t n_worlds;
    int64_t n_initial, n_initial_sat;
    int64_t n_edges;               /* stcsp_result::n_edges: the length of the two byte arrays                         */
    const uint8_t *edge_world;     /* [n_edges]                                                                        */
    const uint8_t *edge_sat;       /* [n_edges]                                                                        */
    const int32_t *witness_values; /* [witness_len * n_vars]                                                           */
    int32_t witness_kind;          /* STCSP_CTL_NONE | IS_WITNESS | IS_COUNTEREXAMPLE                                  */
    int32_t witness_len;           /* in rows                                                                          */
    int32_t n_vars;
    int32_t rounds[3];      /* sweeps in all, the most outer rounds of any EG, launches (0 on the host twin)           */
    double seconds;         /* wall time from the flags in HBM to the result on the host                               */
    double seconds_kernels; /* HIP-event time of the launches, the component pass included (0 on the host twin)        */
} stcsp_ctl_result;

int stcsp_engine_ctl(stcsp_engine *engine, const stcsp_ctl_request *request, stcsp_ctl_result *result);

void stcsp_engine_destroy(stcsp_engine *engine);

/* Message of the last error on this engine (or of the last failed create when engine==NULL). */
const char *stcsp_engine_last_error(const stcsp_engine *engine);

/* ------------------------------------------------------------------------------------------
 * Sharded stepping interface (one engine per GPU, options.world > 1). There is no reference
 * counterpart (the reference is single-threaded); this is the seam the multi-GPU driver uses:
 *
 *   begin();                                   rank owning the root seeds it
 *   loop:
 *     expand_local()                           run this shard's open search nodes until only
 *                                              leaf successor candidates remain, bucketed by
 *                                              owner = hash(cid, signature) % world
 *     outbox(peer) -> device ptr, count        fixed-size candidate records for `peer`
 *     <driver moves records between shards: RCCL all-to-all-v over xGMI>
 *     commit(device ptr, count)                lookup-or-insert each candidate's state, log its
 *                                              edge, open the successor node if the state is new.
 *                                              Asynchronous: the records must stay valid until the
 *                                              next expand_local() / finish() returns
 *     stop when every shard has no open node and no candidate
 *   export() per shard; stcsp_merge_shards() on the gathering rank.
 *
 * State ids in sharded mode are global: gid = ((int64)owner << 40) | local_index.
 * ------------------------------------------------------------------------------------------ */
int stcsp_engine_begin(stcsp_engine *engine);
int stcsp_engine_expand_local(stcsp_engine *engine, int64_t *open_nodes_left);
int stcsp_engine_candidate_bytes(const stcsp_engine *engine); /* record stride */
int stcsp_engine_outbox(stcsp_engine *engine, int peer, void **device_ptr, int64_t *count);
int stcsp_engine_commit(stcsp_engine *engine, const void *device_records, int64_t count);
int stcsp_engine_finish(stcsp_engine *engine); /* closes the timed search phase */

/* Frontier redistribution ("load-imbalance-triggered redistribution of branch nodes",
 * the work unit being the branch case of solverSolveRe, src/solveralgorithm.cpp:911-939). Open search nodes are
 * self-contained records, so any shard can expand any of them:
 *
 *   set_expand_budget(max_rounds, min_open)  expand_local() returns early -- with open nodes left -- once it has
 *                                            run max_rounds launch rounds AND holds at least min_open open nodes
 *                                            (0, 0 = run the local frontier dry, the default). This is what lets
 *                                            the driver see an imbalance, and what makes the start "expand on the
 *                                            root's shard for a few rounds, then scatter".
 *   donate(want) -> device ptr, count        removes up to `want` open nodes from the OLDEST end of the local
 *                                            frontier (the shallowest nodes = the biggest subtrees) and returns them
 *                                            as fixed-size transfer records (node_bytes() each: src state gid,
 *                                            constraint-set TAG, until-expire bits, dirty seed, domain block);
 *                                            valid until the next donate / expand_local
 *   <driver moves the records: the same all-to-all-v as the candidates>
 *   adopt(device ptr, count)                 pushes received records onto the local frontier (the sender's
 *                                            constraint sets must have been imported first: sets_import)
 */
int stcsp_engine_set_expand_budget(stcsp_engine *engine, int64_t max_rounds, int64_t min_open);
int stcsp_engine_node_bytes(const stcsp_engine *engine); /* transfer record stride */
int stcsp_engine_donate(stcsp_engine *engine, int64_t want, void **device_ptr, int64_t *count);
int stcsp_engine_adopt(stcsp_engine *engine, const void *device_records, int64_t count);
/* counters of the last / current solve without exporting the automaton */
int stcsp_engine_counters(stcsp_engine *engine, stcsp_counters *out);
/* The expansion kernel the engine runs for its current program (tests, diagnostics): bit 0 a LITE kernel, bit 1 the
 * one-register LITE shape kernel, bit 2 the image staged in LDS. */
int stcsp_engine_expand_variant(const stcsp_engine *engine);
/* The three kernels the engine runs for its current program, by the template arguments they were instantiated with (tests,
 * diagnostics; read-only). Written by the statements that choose the kernels (select_kernels() in engine.hip). */
enum { /* family: the expansion kernel's row in the table at select_kernels() */
    STCSP_KF_VARIANT = 0,      /* k_expand<DR, L, CS, LITE> with its big-workgroup and one-register refinements */
    STCSP_KF_PREFIX = 1,       /* k_expand<DR, 2, false, false> */
    STCSP_KF_WIDE_DOMAINS = 2, /* k_expand<DR, false, false, false, false, W> */
    STCSP_KF_LONG_KEY = 3,     /* k_expand<4, false, CS, false, false, W, 2> */
    STCSP_KF_LARGE_BLOCK = 4,  /* k_expand<8, false, CS, false, false, W, KR> */
    STCSP_KF_UNTIL_HEAVY = 5,  /* k_expand_until<DR, CS, W, KR, ..> */
    STCSP_KF_BIG_SCOPE = 6     /* k_expand_big<DR, CS, W, KR> */
};
enum { STCSP_KP_PROBE = 0, STCSP_KP_PROBE_BIG = 1 };    /* probe_family: k_probe, k_probe_big */
enum { STCSP_KC_COMMIT = 0, STCSP_KC_COMMIT_UNTIL = 1 }; /* commit_family: k_commit, k_commit_until */
typedef struct stcsp_kernel_choice {
    int32_t family;             /* STCSP_KF_* */
    int32_t dom_regs;           /* DR: 1, 2, 4 or 8 block registers per lane */
    int32_t domain_form;        /* W: 1, 2 or 4 bitset words per domain; 0: interval domains */
    int32_t key_regs;           /* KR: 1, or 2 for a key of more than 64 words */
    int32_t image_in_lds;       /* the expansion kernel's own L (whole image, or the prefix family's staged prefix) ... */
    int32_t compact_sweeps;     /* ... CS ... */
    int32_t lite;               /* ... LITE ... */
    int32_t big_workgroup;      /* ... BIG ... */
    int32_t one_register_shape; /* ... and SHP */
    int32_t expand_threads;     /* its workgroup size */
    int32_t probe_family;       /* STCSP_KP_* */
    int32_t probe_image_in_lds, probe_compact_sweeps, probe_lite; /* k_probe's L, CS, LITE (k_probe_big: 0, CS, 0) */
    int32_t commit_family;      /* STCSP_KC_* */
    int32_t commit_key_regs;    /* the commit kernel's KR */
} stcsp_kernel_choice;
int stcsp_engine_kernel_choice(const stcsp_engine *engine, stcsp_kernel_choice *out);
/* Constraint-set registry exchange: every shard must know a set before it can open a state that
 * uses it. sets_blob returns this shard's registry serialised as int32 words (valid until the
 * next call); sets_import registers the sets of another shard's blob (idempotent). */
int stcsp_engine_sets_blob(stcsp_engine *engine, const int32_t **words, int64_t *n_words);
int stcsp_engine_sets_import(stcsp_engine *engine, const int32_t *words, int64_t n_words);

/* Kernel-granularity check (tests, diagnostics): propagate `count` caller-provided domain blocks
 * (N*K words each, point-major: word[p*N + v], bit i <=> value lb[v] + i) under constraint set `set`
 * with the production device code of one search node (the propagation of generalisedArcConsistent,
 * src/solveralgorithm.cpp:617-706, followed by the classification of solverSolveRe, :738). The blocks are
 * overwritten by their propagated form; outcome[i] = 0 wiped out, 1 branch node, 2 leaf whose
 * constraint-set translation is not known yet, 3 leaf. *skipped (may be NULL) receives the number of
 * revisions the device skipped for their enumeration budget (0 => every block is at its GAC fixpoint).
 * `expire` holds one flag per until constraint: engines with more than 32 until constraints return
 * STCSP_E_UNSUPPORTED. Unsharded engines, between solves. */
int stcsp_engine_propagate(stcsp_engine *engine, int32_t set, uint32_t expire, uint32_t *blocks, int64_t count,
                           int32_t *outcome, int64_t *skipped);

#define STCSP_GID_SHIFT 40

#ifdef __cplusplus
}
#endif
#endif /* STCSP_ENGINE_H */
