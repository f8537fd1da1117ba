/*
 * stcsp_host.h -- host-side plumbing around the engine seam (plain C++ behind a C-ABI so the
 * Python tests, bench.py and the `stcsp` CLI share one implementation).
 *
 *   front end  : .csp text -> built model (stcsp_problem)
 *                replaces src/stcsp.l + src/stcsp.y:56-174 (hand-written: no lex/yacc in the
 *                image) and src/solver.cpp:138-159 solverParse +
 *                src/solveralgorithm.cpp:16-332 solverAddConstr / constraintNormalise.
 *   post-proc  : raw automaton -> pruned, renumbered automaton -> solutions.dot
 *                replaces src/graph.cpp:357-442 (graphTraverse, renumberVertex),
 *                src/graph.cpp:167-355 (adversarialTraverse{,2}) and
 *                src/solveralgorithm.cpp:709-730 + src/graph.cpp:41-101,145-154 (dot writer).
 *
 * None of this is on the GPU hot path (SURVEY.md section 8 marks it plumbing / "next").
 */
#ifndef STCSP_HOST_H
#define STCSP_HOST_H

#include <stddef.h>
#include "stcsp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- front end ---------------- */
typedef struct stcsp_model stcsp_model;

/* Parse + normalise + flatten. prefix_k <= 0 selects the reference default 2
 * (src/solver.cpp:204). On error returns a negative code; stcsp_host_last_error() has the
 * message the reference would have logged / printed (e.g. "Line 3: syntax error"). */
int stcsp_model_load_file(const char *path, int prefix_k, stcsp_model **out);
int stcsp_model_load_text(const char *text, int prefix_k, stcsp_model **out);
const stcsp_problem *stcsp_model_problem(const stcsp_model *model);
void stcsp_model_free(stcsp_model *model);
const char *stcsp_host_last_error(void);

/* Pretty-print constraint `index` of the model the way constraintNodeLogPrint does
 * (src/constraint.cpp:91-154), for diagnostics. Returns a malloc'd string (stcsp_host_free). */
char *stcsp_model_constraint_string(const stcsp_model *model, int index);

/* ---------------- automaton post-processing ---------------- */
typedef struct stcsp_automaton stcsp_automaton;

/* Copies the raw result (so the engine may be destroyed afterwards). */
int stcsp_automaton_build(const stcsp_problem *problem, const stcsp_result *result, stcsp_automaton **out);
void stcsp_automaton_free(stcsp_automaton *a);

/* graphTraverse (src/graph.cpp:357-418): final flags from the until part of the signature,
 * valid = can reach a final state, edges into invalid states deleted. */
int stcsp_automaton_traverse(stcsp_automaton *a);
/* adversarialTraverse (src/graph.cpp:304-355); the reference hard-codes var_index = 5.
 * Returns root->valid (0/1) or a negative error. */
int stcsp_automaton_adversarial(stcsp_automaton *a, int var_index);
/* adversarialTraverse2 (src/graph.cpp:247-302); the reference hard-codes opponent=5, avatar=6. */
int stcsp_automaton_adversarial2(stcsp_automaton *a, int opponent_index, int avatar_index);
/* Take the flags computed on the device by stcsp_engine_postprocess() (stcsp_engine.h) instead of
 * running the three passes above on the host: valid / final per state, alive per edge, indexed like
 * the stcsp_result the automaton was built from. */
int stcsp_automaton_import_flags(stcsp_automaton *a, const uint8_t *state_valid, const uint8_t *state_final,
                                 const uint8_t *edge_alive);
/* Read the current flags back (any pointer may be NULL): [n_states], [n_states], [n_edges]. */
int stcsp_automaton_flags(const stcsp_automaton *a, uint8_t *state_valid, uint8_t *state_final, uint8_t *edge_alive);
/* Make the output order independent of the search's scheduling: out-edges of every state ordered by
 * content (destination buckets by smallest label, edges by label). Call before renumber / write_dot /
 * write_binary when the files must be reproducible byte for byte; O(E log E) label comparisons. */
int stcsp_automaton_order_by_label(stcsp_automaton *a);
/* renumberVertex (src/graph.cpp:420-442). */
int stcsp_automaton_renumber(stcsp_automaton *a);

/* solverOut (src/solveralgorithm.cpp:709-730). Same line formats; the body order follows this
 * implementation's own deterministic DFS (byte-identical order would need
 * __gnu_cxx::hash_map iteration order: SURVEY.md parity level L3, not a goal). */
int stcsp_automaton_write_dot(const stcsp_automaton *a, const char *path);

/* Compact binary form of the same printed automaton (layout: postproc.cpp, "STCSPAUT" v1):
 * ~(4 + n_vars) bytes per edge instead of ~4*n_vars of text -- the exchange format for consumers
 * that do not need Graphviz. read_binary gives an automaton on which write_dot / canonical /
 * num_* work (traverse / adversarial passes have already been applied to what it holds). */
int stcsp_automaton_write_binary(const stcsp_automaton *a, const char *path);
int stcsp_automaton_read_binary(const char *path, stcsp_automaton **out);

/* Canonical text of the automaton: BFS from the root over edges
 * sorted by label, states renumbered in discovery order, constraint-set ids renumbered by
 * first appearance. sha256 of this text is the parity object. malloc'd; stcsp_host_free. */
char *stcsp_automaton_canonical(const stcsp_automaton *a, size_t *len);

int64_t stcsp_automaton_num_states(const stcsp_automaton *a);      /* table size (incl. failed) */
int64_t stcsp_automaton_num_live_states(const stcsp_automaton *a); /* reachable + printed        */
int64_t stcsp_automaton_num_live_edges(const stcsp_automaton *a);
/* The variables of the automaton (a binary file carries their names): how many, and the name of one, owned by the
 * automaton; NULL for an index out of range. */
int stcsp_automaton_num_vars(const stcsp_automaton *a);
const char *stcsp_automaton_var_name(const stcsp_automaton *a, int index);

/* ---- bisimulation quotient (definition: stcsp_engine.h, stcsp_engine_quotient) ----
 * The exact CPU twin of the device pass, written as plain partition refinement with ordered containers: the
 * checker of the device pass in the tests, and the path for automata whose flags live on the host (sharded
 * runs, host adversarial passes). Uses the automaton's current flags (traverse / adversarial* / import_flags).
 * observable: [n_vars], nonzero = observable; NULL = every variable whose name does not start with "_V".
 * state_class_out: [num_states] classes numbered by their least member, -1 outside the live automaton.
 * Returns the number of refinement rounds (>= 1) or a negative error. The mask is remembered for
 * stcsp_automaton_quotient(). */
int stcsp_automaton_bisimulation(stcsp_automaton *a, const uint8_t *observable, int32_t *state_class_out, int64_t *n_classes);
/* Set the mask stcsp_automaton_quotient() projects with, when the partition comes from the device pass. */
int stcsp_automaton_set_observable(stcsp_automaton *a, const uint8_t *observable);
/* Build the quotient of `a` under a partition of its live states: one state per class, printed with the
 * constraint id and signature of the member that the canonical numbering (breadth-first from the root,
 * out-edges in label order) reaches first -- state indices depend on the search's scheduling, that
 * numbering does not; one edge per distinct (source class, projected label, destination class), carrying
 * the lexicographically least full label of the edges that project on it. The root is class 0; a
 * partition without a live root gives the EMPTY automaton. Under a projecting mask the result is
 * language-preserving, not necessarily minimal. write_dot, write_binary, canonical, renumber and
 * order_by_label work on the result; free it with stcsp_automaton_free(). */
int stcsp_automaton_quotient(const stcsp_automaton *a, const int32_t *state_class, int64_t n_classes, stcsp_automaton **out);

/* ---- checking observed streams (definition: stcsp_engine.h, stcsp_engine_monitor_check) ----
 * The same contract written plainly with ordered containers, on the automaton's current flags: the checker of the
 * device pass in the tests, the road of the streams whose state set outgrows the device kernel's capacity, and the
 * path for automata whose flags live on the host (sharded runs, host adversarial passes, read_binary).
 * observable: as in stcsp_automaton_bisimulation(). offsets: [n_streams + 1] in steps, offsets[0] == 0, not
 * decreasing; values: [offsets[n_streams] * (number of observable variables)]. accepted_len / n_end: [n_streams]
 * int32, end_final: [n_streams] uint8. max_set_size (may be NULL) receives the largest |S_t| met over all streams.
 * STCSP_E_INVALID on malformed offsets. */
int stcsp_automaton_check_streams(const stcsp_automaton *a, const uint8_t *observable, int64_t n_streams, const int64_t *offsets,
                                  const int32_t *values, int32_t *accepted_len, int32_t *n_end, uint8_t *end_final,
                                  int64_t *max_set_size);
/* Values per step under a mask: the number of observable variables (NULL = the default mask). */
int stcsp_automaton_num_observable(const stcsp_automaton *a, const uint8_t *observable);

/* ---- counting, enumerating and sampling solution prefixes (definition: stcsp_engine.h, stcsp_engine_generate) ----
 * The same contract written plainly, on the automaton's current flags: the checker of the device pass in the tests, and
 * the path for automata whose flags live on the host (sharded runs, host adversarial passes, read_binary). One call
 * builds the canonical order and the weights and generates. observable: as in stcsp_automaton_bisimulation(); flags:
 * STCSP_GEN_*; ranks: [n_streams] to unrank, NULL to sample with `seed`. count (may be NULL): [horizon + 1];
 * values: [n_streams * len * (number of observable variables)]; end_final: [n_streams]. count is filled whenever the
 * weights are finite, also when the request itself is then refused. STCSP_E_INVALID and STCSP_E_UNSUPPORTED as there. */
int stcsp_automaton_generate(const stcsp_automaton *a, const uint8_t *observable, int32_t horizon, int32_t flags, int64_t n_streams,
                             int32_t len, uint64_t seed, const uint64_t *ranks, double *count, int32_t *values, uint8_t *end_final);
/* count[t], t = 0 .. horizon, alone. */
int stcsp_automaton_count_streams(const stcsp_automaton *a, int32_t horizon, int32_t flags, double *count);

/* ---- repairing observed streams: the nearest solution prefix (definition: stcsp_engine.h, stcsp_engine_repair) ----
 * The same contract written plainly, on the automaton's current flags: the checker of the device pass in the tests, and
 * the path for automata whose flags live on the host (sharded runs, host adversarial passes, read_binary). observable:
 * as in stcsp_automaton_bisimulation(); flags: STCSP_REPAIR_*; weights: [number of observable variables] or NULL;
 * offsets / values: the streams, as for stcsp_automaton_check_streams() (STCSP_REPAIR_MISSING = not observed).
 * distance, end_final, n_changed: [n_streams]; out_values: the repaired rows at the input's offsets, 0 for a stream of
 * distance -1. STCSP_E_INVALID as there. */
int stcsp_automaton_repair_streams(const stcsp_automaton *a, const uint8_t *observable, int32_t flags, const int32_t *weights, int64_t n_streams,
                                   const int64_t *offsets, const int32_t *values, int32_t *distance, int32_t *out_values, uint8_t *end_final,
                                   int32_t *n_changed);

/* ---- aligning observed streams: dropped and spurious steps (definition: stcsp_engine.h, stcsp_engine_align) ----
 * The same contract written plainly, on the automaton's current flags: the checker of the device pass in the tests, and
 * the path for automata whose flags live on the host (sharded runs, host adversarial passes, read_binary). observable,
 * weights, offsets / values: as for stcsp_automaton_repair_streams(); flags: STCSP_ALIGN_*; skip_cost, gap_cost >= 1.
 * distance, end_final, n_changed, n_skipped, n_inserted: [n_streams]; out_offsets, op_offsets: [n_streams + 1], in rows
 * and in ops; *out_values and *ops receive the emitted rows and the ops, each in one block the caller releases with
 * stcsp_host_free(). The bound of the contract counts every state of the automaton. STCSP_E_INVALID as there. */
int stcsp_automaton_align_streams(const stcsp_automaton *a, const uint8_t *observable, int32_t flags, const int32_t *weights, int32_t skip_cost,
                                  int32_t gap_cost, int64_t n_streams, const int64_t *offsets, const int32_t *values, int32_t *distance,
                                  int64_t *out_offsets, int32_t **out_values, int64_t *op_offsets, uint8_t **ops, uint8_t *end_final,
                                  int32_t *n_changed, int32_t *n_skipped, int32_t *n_inserted);

/* ---- inferring the unobserved entries of a stream (definition: stcsp_engine.h, stcsp_engine_infer) ----
 * The same contract written plainly, on the automaton's current flags: the checker of the device pass in the tests, and
 * the path for automata whose flags live on the host (sharded runs, host adversarial passes, read_binary). observable:
 * as in stcsp_automaton_bisimulation(); flags: STCSP_INFER_*; offsets / values: the streams (STCSP_INFER_MISSING = not
 * observed); draws >= 0; ranks: [n_streams * draws] to unrank, NULL to sample with `seed`. count: [n_streams];
 * support_off: [offsets[n_streams] * (number of observable variables) + 1]; *support_val receives the support values in
 * one block the caller releases with stcsp_host_free(); n_states: [offsets[n_streams] + n_streams]; draw_values:
 * [offsets[n_streams] * draws * (number of observable variables)]; end_final: [n_streams * draws]. STCSP_E_INVALID and
 * STCSP_E_UNSUPPORTED as there; the outputs of the streams before the refused one are then filled. */
int stcsp_automaton_infer_streams(const stcsp_automaton *a, const uint8_t *observable, int32_t flags, int64_t n_streams, const int64_t *offsets,
                                  const int32_t *values, int32_t draws, const uint64_t *ranks, uint64_t seed, double *count, int64_t *support_off,
                                  int32_t **support_val, int32_t *n_states, int32_t *draw_values, uint8_t *end_final);

/* ---- posterior marginals of the unobserved entries of a stream (definition: stcsp_engine.h, stcsp_engine_posterior) ----
 * The same contract written plainly, on the automaton's current flags: the checker of the device pass in the tests, and
 * the path for automata whose flags live on the host (sharded runs, host adversarial passes, read_binary). observable:
 * as in stcsp_automaton_bisimulation(); flags: STCSP_POSTERIOR_*; offsets / values: the streams (STCSP_POSTERIOR_MISSING
 * = not observed); weight_off / weight_val / weight_w: the value weights as there, all NULL = every value weighs 1.
 * mass, exact, final_mass: [n_streams]; marg_off: [offsets[n_streams] * (number of observable variables) + 1];
 * *marg_val and *marg_mass receive the marginals in two blocks the caller releases with stcsp_host_free().
 * STCSP_E_INVALID as there. */
int stcsp_automaton_posterior_streams(const stcsp_automaton *a, const uint8_t *observable, int32_t flags, int64_t n_streams, const int64_t *offsets,
                                      const int32_t *values, const int64_t *weight_off, const int32_t *weight_val, const int32_t *weight_w,
                                      double *mass, uint8_t *exact, uint64_t *final_mass, int64_t *marg_off, int32_t **marg_val, uint64_t **marg_mass);

/* ---- the observer: subset construction under a mask (definition: stcsp_engine.h, stcsp_engine_observer) ----
 * The same contract written plainly with ordered containers, on the automaton's current flags: the checker of the device
 * pass in the tests, and the path for automata whose flags live on the host (sharded runs, host adversarial passes,
 * read_binary). observable: as in stcsp_automaton_bisimulation(); max_states: 0 = the default of the device pass,
 * STCSP_E_NOMEM beyond it. The result (stcsp_observer_get(): members named by this automaton's state indices; the time
 * fields other than `seconds` and table_bytes are 0) lives until stcsp_observer_free(). */
typedef struct stcsp_observer stcsp_observer;
int stcsp_automaton_observer(const stcsp_automaton *a, const uint8_t *observable, int64_t max_states, stcsp_observer **out);
const stcsp_observer_result *stcsp_observer_get(const stcsp_observer *o);
void stcsp_observer_free(stcsp_observer *o);
/* The observer as an automaton. `observer` is the result of stcsp_engine_observer() or of stcsp_automaton_observer() for
 * the automaton `a` (same states, same flags) under `observable`. One state per set, printed with the constraint id and
 * signature of its member of least canonical number (breadth-first from the root, out-edges in label order); final as
 * the set; an edge carries the lexicographically least full label among the live edges out of the source set that
 * project on its row, as stcsp_automaton_quotient() does. An observer without states gives the EMPTY automaton; a result
 * that does not fit `a` is STCSP_E_INVALID. write_dot, write_binary, canonical, renumber, order_by_label, bisimulation,
 * quotient, check_streams, count_streams, generate and observer work on the result, whose remembered mask is
 * `observable`; free it with stcsp_automaton_free(). */
int stcsp_automaton_from_observer(const stcsp_automaton *a, const uint8_t *observable, const stcsp_observer_result *observer,
                                  stcsp_automaton **out);

/* ---- comparing two observable languages (definition: stcsp_engine.h, stcsp_engine_compare) ----
 * The same contract written plainly with ordered containers over two observers (results of stcsp_engine_observer() or
 * stcsp_automaton_observer(), or any deterministic automata in that layout; `right` has its rows in the column order of
 * `left`): the checker of the device pass in the tests, and the road for sharded runs, host adversarial passes and
 * automata read from binary files. max_pairs: 0 = the default of the device pass, STCSP_E_NOMEM beyond it;
 * STCSP_E_INVALID for a malformed operand, either one. The result (stcsp_comparison_get(): the time fields other than
 * `seconds` and table_bytes are 0) lives until stcsp_comparison_free(). */
typedef struct stcsp_comparison stcsp_comparison;
int stcsp_compare_observers(const stcsp_observer_result *left, const stcsp_observer_result *right, int64_t max_pairs, stcsp_comparison **out);
const stcsp_compare_result *stcsp_comparison_get(const stcsp_comparison *c);
void stcsp_comparison_free(stcsp_comparison *c);

/* ---- strongly connected components and lasso solutions (definition: stcsp_engine.h, stcsp_engine_components) ----
 * The same contract written plainly, on the automaton's current flags: an iterative Tarjan, breadth-first searches and the
 * same greedy walks. The checker of the device pass in the tests, and the path for automata whose flags live on the host
 * (merged sharded runs, host adversarial passes, read_binary, import_flags). max_lassos and flags as in
 * stcsp_components_options (STCSP_SCC_NO_TRIM has no meaning here); STCSP_E_INTERNAL when a walk meets two live out-edges
 * of one state with the same full row. The result (stcsp_components_get(): rounds and seconds_kernels are 0) lives until
 * stcsp_components_free(). */
typedef struct stcsp_components stcsp_components;
int stcsp_automaton_components(const stcsp_automaton *a, int64_t max_lassos, int32_t flags, stcsp_components **out);
const stcsp_components_result *stcsp_components_get(const stcsp_components *c);
void stcsp_components_free(stcsp_components *c);

/* ---- optimal solution streams: least cost per length, least mean (definition: stcsp_engine.h, stcsp_engine_optimise) ----
 * The same contract written plainly, on the automaton's current flags: the same dynamic programme, the same greedy walk,
 * and a textbook Karp per component with the full table of (size + 1) * size int64 (STCSP_E_NOMEM when that cannot be
 * allocated). The checker of the device pass in the tests, and the path for automata whose flags live on the host (merged
 * sharded runs, host adversarial passes, read_binary, import_flags). The variables' bounds are the automaton's. Errors as
 * there, without a message. The result (stcsp_optimise_get(): rounds and seconds_kernels are 0) lives until
 * stcsp_optimise_free(). */
typedef struct stcsp_optimise stcsp_optimise;
int stcsp_automaton_optimise(const stcsp_automaton *a, const stcsp_optimise_request *request, stcsp_optimise **out);
const stcsp_optimise_result *stcsp_optimise_get(const stcsp_optimise *o);
void stcsp_optimise_free(stcsp_optimise *o);

/* ---- temporal queries over the infinite solutions: fair CTL (definition: stcsp_engine.h, stcsp_engine_ctl) ----
 * stcsp_ctl_parse() turns formula text into the postfix program of stcsp_ctl_request. Of `problem` it reads n_vars and
 * var_names only. Grammar, loosest first:  f -> g (right associative),  f | g,  f & g,  then the prefix operators
 * ! EX EF EG AX AF AG,  E[f U g],  A[f U g],  ( f ),  true,  false  and the atoms NAME op INT and NAME op NAME with op one
 * of == != < <= > >= (INT: a decimal int32, with a sign if negative). A word followed by a comparison is a variable, whatever
 * its spelling. *program receives the words in one block the caller releases with stcsp_host_free(), *n_words their count.
 * On an error (STCSP_E_INVALID: a syntax error, an unknown variable name, an integer outside int32) *error_pos receives the
 * 0-based offset into text and message (message_len bytes, may be NULL) what is wrong there.
 *
 * stcsp_automaton_ctl() is the same contract written plainly, on the automaton's current flags: the same lowering (shared
 * with the device pass, limits included), the same fixpoints over one byte per world, the same witness rule. The checker of
 * the device pass in the tests, and the path for automata whose flags live on the host (merged sharded runs, host
 * adversarial passes, read_binary, import_flags). Errors as there, without a message. The result (stcsp_ctl_get(): rounds
 * and seconds_kernels are 0) lives until stcsp_ctl_free(). */
int stcsp_ctl_parse(const char *text, const stcsp_problem *problem, int32_t **program, int32_t *n_words, int32_t *error_pos, char *message,
                    size_t message_len);
typedef struct stcsp_ctl stcsp_ctl;
int stcsp_automaton_ctl(const stcsp_automaton *a, const stcsp_ctl_request *request, stcsp_ctl **out);
const stcsp_ctl_result *stcsp_ctl_get(const stcsp_ctl *c);
void stcsp_ctl_free(stcsp_ctl *c);

/* Merge the per-shard results of a sharded run (global state ids, see stcsp_engine.h) into
 * one result with dense ids; runs the ok-fixpoint over the union. The merged result is owned
 * by the returned handle. */
typedef struct stcsp_merged stcsp_merged;
int stcsp_merge_shards(const stcsp_result *const *shards, int n_shards, stcsp_merged **out);
const stcsp_result *stcsp_merged_result(const stcsp_merged *m);
void stcsp_merged_free(stcsp_merged *m);

void stcsp_host_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* STCSP_HOST_H */
