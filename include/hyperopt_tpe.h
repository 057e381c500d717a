/*
 * hyperopt_tpe.h -- C ABI of the MI355X (gfx950) TPE suggestion engine.
 *
 * Plain C, plain pointers and sizes; no torch or HIP types cross this
 * boundary.  Every entry point cites the reference function it replaces
 * (mvanveen/hyperopt, paths relative to the repository root).  The reference
 * is pure Python, so its "FFI" is the pyll operator registry: `scope.define`
 * (hyperopt/pyll/base.py:132-138) registers each numeric op by name and
 * `build_posterior` (hyperopt/tpe.py:651-739) wires them per hyperparameter.
 * The ops below are those registry entries, plus one fused entry point
 * (`tpe_suggest`) that runs the whole per-label chain on the GPU.
 *
 * All calls are synchronous with respect to the host: on return, outputs are
 * in the caller's buffers.  A context is not thread-safe; use one per thread.
 * Return value: TPE_OK (0) or a negative TPE_ERR_*; the message is available
 * from tpe_last_error(ctx) (or tpe_last_error(NULL) for tpe_ctx_create).
 */
#ifndef HYPEROPT_TPE_H
#define HYPEROPT_TPE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPE_ABI_VERSION 5

/* error codes; the Python layer maps them to the reference's exception types */
#define TPE_OK 0
#define TPE_ERR_VALUE (-1)   /* ValueError (e.g. 'low >= high', tpe.py:86-87)      */
#define TPE_ERR_TYPE (-2)    /* TypeError (e.g. non-vector params, tpe.py:117-122)  */
#define TPE_ERR_ARG (-3)     /* bad pointer / size / state                          */
#define TPE_ERR_HIP (-4)     /* HIP runtime failure                                 */
#define TPE_ERR_SAMPLE (-5)  /* truncated sampler could not reach the interval     */

/* arithmetic of the dense (unquantized) lpdf paths; quantized and sampling
 * paths always run in fp64 */
#define TPE_F64 0
#define TPE_F32 1

/* posterior families (the `<sampler>` names of tpe.py:712) */
#define TPE_GMM1 0         /* truncated Gaussian mixture            tpe.py:68-172  */
#define TPE_LGMM1 1        /* log-space Gaussian mixture            tpe.py:222-307 */
#define TPE_CATEGORICAL 2  /* categorical over 0..upper-1           tpe.py:56-63   */

/* presence flags for the optional `low`, `high`, `q` arguments (None in Python) */
#define TPE_HAS_LOW 1
#define TPE_HAS_HIGH 2
#define TPE_HAS_Q 4
/* tpe_label_spec only: `stream` names the label's Philox stream (default: its
 * position in the spec array) -- a process holding a subset of the labels
 * (label-sharded ranks) draws the candidates the whole space would */
#define TPE_HAS_STREAM 8

typedef struct tpe_ctx tpe_ctx;

/* One hyperparameter's pair of posteriors (the below/`l` and above/`g`
 * mixtures that build_posterior makes per label, tpe.py:684-692).
 * Mixture components live in flat arrays passed to tpe_set_posterior:
 *   GMM1/LGMM1: weights[off+k], mus[off+k], sigmas[off+k], k < n (as returned
 *               by adaptive_parzen_normal, tpe.py:404-477);
 *   CATEGORICAL: weights[off+k] = p[k] (pseudocount posterior,
 *               tpe.py:581-617); n == upper; mus/sigmas unused.
 * low/high/q are the GMM1/LGMM1 keyword arguments; for LGMM1 low/high are in
 * log space exactly as in the reference call LGMM1(..., low, high, q). */
typedef struct {
    int32_t kind;       /* TPE_GMM1 / TPE_LGMM1 / TPE_CATEGORICAL */
    int32_t flags;      /* TPE_HAS_LOW | TPE_HAS_HIGH | TPE_HAS_Q */
    double low;
    double high;
    double q;
    int64_t below_off;
    int64_t above_off;
    int32_t n_below;
    int32_t n_above;
} tpe_label_desc;       /* 56 bytes */

/* Observation transforms of the adaptive-Parzen samplers (tpe.py:493-576),
 * applied by the caller before tpe_build_posterior (so the transform is the
 * caller's own float64 log, bit-for-bit the reference's np.log):
 *   IDENTITY   uniform, quniform, normal, qnormal, randint, categorical
 *   LOG        loguniform, lognormal:          log(obs)
 *   LOG_FLOOR  qloguniform, qlognormal:        log(max(obs, floor)) */
#define TPE_OBS_IDENTITY 0
#define TPE_OBS_LOG 1
#define TPE_OBS_LOG_FLOOR 2

/* One hyperparameter as build_posterior sees it (tpe.py:678-692): the
 * sampler arguments of its posterior and the prior of its adaptive-Parzen
 * estimator. */
typedef struct {
    int32_t kind;        /* TPE_GMM1 / TPE_LGMM1 / TPE_CATEGORICAL             */
    int32_t flags;       /* TPE_HAS_LOW | TPE_HAS_HIGH | TPE_HAS_Q             */
    double low;          /* sampler arguments, as in tpe_label_desc            */
    double high;
    double q;
    double prior_mu;     /* ap_*_sampler prior (tpe.py:493-576)                */
    double prior_sigma;
    int32_t upper;       /* categorical: number of categories                  */
    int32_t randint;     /* categorical: 1 randint (counts + prior_weight,
                            tpe.py:581-589), 0 pchoice (counts + upper *
                            prior_weight * p, tpe.py:598-617)                  */
    int64_t p_off;       /* pchoice: offset of its p vector in cat_p           */
    int32_t stream;      /* with TPE_HAS_STREAM: the label's Philox stream     */
    int32_t reserved;    /* 0                                                  */
} tpe_label_spec;        /* 72 bytes */

/* Winner of one label's candidate set (broadcast_best, tpe.py:769-778). */
typedef struct {
    double value;       /* samples[best] (categorical: the integer index as double) */
    double score;       /* lpdf_below[best] - lpdf_above[best]                      */
    double lpdf_below;
    double lpdf_above;
    int64_t index;      /* GLOBAL candidate index of the winner (-1: no candidates) */
    int32_t label;
    int32_t status;     /* 0 ok; TPE_STATUS_VALUE_ONLY: index and value only        */
} tpe_label_result;     /* 48 bytes */

/* status of a TPE_OPT_VALUE_ONLY round's cell that the screen alone decided:
 * index and value are the winner's, score / lpdf_below / lpdf_above are NaN
 * (not computed).  Such records carry no order key, so tpe_merge_results and
 * tpe_merge_results_device refuse them (TPE_ERR_ARG). */
#define TPE_STATUS_VALUE_ONLY 1

int tpe_abi_version(void);

/* Hash of the sources the library was built from (16 hex digits); the
 * loader compares it with the sources in the tree and refuses a stale build. */
const char *tpe_source_hash(void);

/* device: HIP ordinal; precision: TPE_F64 or TPE_F32 */
int tpe_ctx_create(int device, int precision, tpe_ctx **out);

/* One context over several GPUs of the node (devices[0] first; a device may
 * repeat, e.g. to test sharding on one GPU).  Every entry point keeps its
 * meaning: posterior uploads, device builds, history appends and options
 * go to every device; tpe_suggest / tpe_suggest_batch split each round over
 * the devices -- contiguous global candidate ranges when every device gets
 * at least 1024 candidates of each round, else whole rounds -- one host
 * thread and HIP stream per device, and merge the per-device winners with
 * the broadcast_best order.  The results are bit-identical to a one-device
 * context's (the reference's single synchronous algo call per
 * round, hyperopt/fmin.py:201-202, keeps the fan-out inside the call).  The
 * single-op entry points, tpe_score and tpe_get_mixture use devices[0]. */
int tpe_ctx_create_multi(const int *devices, int32_t n_devices, int precision, tpe_ctx **out);

/* Devices of a context (writes at most cap ordinals); returns their count. */
int32_t tpe_ctx_devices(const tpe_ctx *ctx, int32_t *devices, int32_t cap);

/* Label shards of a multi-device context (TPE_OPT_LABEL_SHARDS): the
 * position in tpe_ctx_devices' list of the device holding `label` of the
 * resident history, or -1 when the context's labels are not sharded (one
 * device, replicated posteriors, no such label). */
int32_t tpe_label_device(const tpe_ctx *ctx, int32_t label);

void tpe_ctx_destroy(tpe_ctx *ctx);
const char *tpe_last_error(const tpe_ctx *ctx);

/* ---- reference operators, 1:1 (host buffers in and out) ------------------ */

/* GMM1_lpdf(samples, weights, mus, sigmas, low, high, q)   tpe.py:110-172 */
int tpe_gmm1_lpdf(tpe_ctx *ctx, const double *samples, int64_t n,
                  const double *weights, const double *mus, const double *sigmas,
                  int32_t k, int32_t flags, double low, double high, double q,
                  double *out);

/* LGMM1_lpdf(samples, weights, mus, sigmas, low, high, q)  tpe.py:265-307 */
int tpe_lgmm1_lpdf(tpe_ctx *ctx, const double *samples, int64_t n,
                   const double *weights, const double *mus, const double *sigmas,
                   int32_t k, int32_t flags, double low, double high, double q,
                   double *out);

/* categorical_lpdf(sample, p, upper)                        tpe.py:56-63 */
int tpe_categorical_lpdf(tpe_ctx *ctx, const int64_t *samples, int64_t n,
                         const double *p, int32_t upper, double *out);

/* np.argmax(below_llik - above_llik) of broadcast_best      tpe.py:769-778
 * (first NaN wins, NaN above +inf, lowest index wins ties) */
int tpe_broadcast_best(tpe_ctx *ctx, const double *below, const double *above,
                       int64_t n, int64_t *best);

/* GMM1(weights, mus, sigmas, low, high, q, rng, size)      tpe.py:68-99
 * Same distribution as the reference (component ~ weights, Gaussian draw,
 * accept iff low <= draw < high, round(x/q)*q); the random stream is
 * Philox4x32-10 keyed by `seed`, counter = (offset + i, attempt, stream,
 * round), so draw i is the same whatever the batching or GPU count. */
int tpe_gmm1_sample(tpe_ctx *ctx, const double *weights, const double *mus,
                    const double *sigmas, int32_t k, int32_t flags, double low,
                    double high, double q, uint64_t seed, uint32_t stream,
                    uint32_t round, int64_t offset, int64_t n, double *out);

/* LGMM1(weights, mus, sigmas, low, high, q, rng, size)     tpe.py:222-256 */
int tpe_lgmm1_sample(tpe_ctx *ctx, const double *weights, const double *mus,
                     const double *sigmas, int32_t k, int32_t flags, double low,
                     double high, double q, uint64_t seed, uint32_t stream,
                     uint32_t round, int64_t offset, int64_t n, double *out);

/* categorical(p, upper, rng, size)            hyperopt/pyll/stochastic.py:109-147 */
int tpe_categorical_sample(tpe_ctx *ctx, const double *p, int32_t upper,
                           uint64_t seed, uint32_t stream, uint32_t round,
                           int64_t offset, int64_t n, int64_t *out);

/* ---- resident posterior + fused suggestion round ------------------------- */

/* Upload the per-label posteriors (replaces the graph that
 * build_posterior/tpe_transform rebuild on every call, tpe.py:651-739,
 * 794-820).  Arrays are copied; the device copy stays resident until the
 * next call or tpe_ctx_destroy.  A mixture's components may come in any
 * order; only a posterior whose above mixtures are ordered by mu (as
 * adaptive_parzen_normal and the device builds leave them) gets the
 * expansion index (TPE_OPT_EXPAND), any other takes the windowed screen. */
int tpe_set_posterior(tpe_ctx *ctx, const tpe_label_desc *labels, int32_t n_labels,
                      const double *weights, const double *mus, const double *sigmas,
                      int64_t n_components);

/* Build the resident posterior ON THE DEVICE from the trial history
 * (replaces ap_filter_trials tpe.py:624-648, linear_forgetting_weights
 * :385-398, adaptive_parzen_normal :404-477 and the categorical pseudocount
 * posteriors :581-617 for every label, then the same upload as
 * tpe_set_posterior).
 *   losses[t], t < n_trials: loss of trial t, trials in tid order (the
 *       order suggest() sorts docs in, tpe.py:858); +inf for no loss;
 *   per label l, observations obs_off[l] .. obs_off[l+1]-1 in tid order:
 *       obs_trial = position t of the observation's trial in `losses`,
 *       obs_val   = the (already transformed, TPE_OBS_*) value;
 *   gamma, prior_weight: the tpe.suggest arguments; lf: the linear
 *       forgetting of the Parzen weights (adaptive_parzen_normal's LF,
 *       tpe.py:406; 25 = DEFAULT_LF in the reference, which never passes
 *       another -- tpe.suggest's linear_forgetting is unused, :828).
 * The below set is the n_below = min(ceil(gamma sqrt(n_trials)), 25) lowest
 * (gamma_cap = DEFAULT_LF, tpe.py:626,636, whatever lf is)
 * losses; equal losses and equal observations are ordered by position
 * (a stable sort; the reference's np.argsort order for ties is numpy's
 * unstable quicksort -- tpe_build_posterior_resident_ordered takes the
 * reference's order where it matters).  n_below_out (may be NULL) receives
 * n_below. */
int tpe_build_posterior(tpe_ctx *ctx, const tpe_label_spec *specs, int32_t n_labels,
                        const double *cat_p, int64_t n_cat_p,
                        const double *losses, int64_t n_trials,
                        const int64_t *obs_off, const int32_t *obs_trial,
                        const double *obs_val, double gamma, double prior_weight,
                        int32_t lf, int32_t *n_below_out);

/* Device-resident history (the columnar trial history of SURVEY §8f rank 1,
 * kept on the GPU): tpe_history_reset fixes the labels; tpe_history_append
 * adds only NEW observations (per label n_new[l] of them, concatenated
 * label-major: trial position in tid order and transformed value, as for
 * tpe_build_posterior) -- each label's observations are kept in observation
 * order and value-sorted (a stable merge of the sorted new batch), so a
 * rebuild sorts nothing; tpe_build_posterior_resident then rebuilds the
 * posterior from the current losses.  losses[t] = NaN marks a trial that is
 * not in the history (its observations join neither set, like a NaN-loss doc
 * in tpe.py:849-853); n_valid = the number of non-NaN losses (len(l_vals)).
 * tpe_build_posterior is reset + append(all) + build_resident. */
int tpe_history_reset(tpe_ctx *ctx, const tpe_label_spec *specs, int32_t n_labels,
                      const double *cat_p, int64_t n_cat_p);
int tpe_history_append(tpe_ctx *ctx, const int64_t *n_new, const int32_t *obs_trial,
                       const double *obs_val);
int tpe_build_posterior_resident(tpe_ctx *ctx, const double *losses, int64_t n_trials,
                                 int64_t n_valid, double gamma, double prior_weight,
                                 int32_t lf, int32_t *n_below_out);

/* Diagnostic readback of the resident history (tests): label `label`'s pool
 * region as the appends left it.  *n receives its observation count, and the
 * first min(cap, *n) entries of each non-NULL array are written: trial and val
 * in observation order (what tpe_history_append was given), and for a
 * non-categorical label its value-sorted view -- key ascending, idx the
 * observation index of each key, equal keys in observation order (key and idx
 * are left untouched for a categorical label, which has none).  region_cap /
 * region_off: the capacity and the offset of the label's region in the pool
 * (a label never observed owns a region of capacity 0).  With every array
 * NULL only the three numbers are returned.  Waits for the context's stream
 * (the appends are queued) before it reads; changes nothing.  A label-sharded
 * multi-device context reads the owning device (as tpe_get_mixture does); a
 * replicated one reads replica `device` (0 .. devices - 1); a one-device
 * context ignores `device`.  TPE_ERR_ARG before tpe_history_reset. */
int tpe_history_get(tpe_ctx *ctx, int32_t label, int32_t device, int32_t *trial, double *val,
                    double *key, int32_t *idx, int64_t cap, int64_t *n, int64_t *region_cap,
                    int64_t *region_off);

/* tpe_build_posterior_resident with the reference's tie order (ap_filter_trials
 * tpe.py:637 `l_order = np.argsort(l_vals)` and adaptive_parzen_normal
 * tpe.py:433 `order = np.argsort(mus)`: numpy's unstable sort, whose order of
 * equal keys the device cannot reproduce, so the caller computes it with
 * numpy itself when it matters):
 *   below (NULL: the device split, ties by position): per trial position
 *       1 if the trial is in the below set -- exactly n_below trials, each
 *       with a loss;
 *   order_off[n_labels + 1], order (NULL: none supplied): label l's entries
 *       order[order_off[l] .. order_off[l+1]) are np.argsort of its above
 *       observations (in observation order) -- the above list's indices in
 *       value order; an empty range keeps the device's position order;
 *   ties (may be NULL; n_labels + 1 entries) receives what depends on a tie
 *       order the caller did not supply: ties[l] bit 1 (bit 0) when label l's
 *       above (below) mixture has equal mus while its linear-forgetting
 *       weights differ (the tie order decides which weight meets a run end's
 *       sigma, and the order of the normalising sum); ties[n_labels] = 1
 *       when equal losses straddle the n_below boundary of the split.
 * A caller that gets a non-zero flag computes the reference's order for it
 * and builds again (hyperopt_amd/posterior.py reference_orders). */
int tpe_build_posterior_resident_ordered(tpe_ctx *ctx, const double *losses, int64_t n_trials,
                                         int64_t n_valid, double gamma, double prior_weight,
                                         int32_t lf, const uint8_t *below, const int64_t *order_off,
                                         const int32_t *order, int32_t *n_below_out, int32_t *ties);

/* The ordered rebuild restricted to `labels` (n_only increasing label
 * indices): right after a build of the same resident history with the same
 * arguments (no append in between, or TPE_ERR_ARG), rebuild only those
 * labels with the supplied orders and keep the others' mixtures and records
 * -- the labels whose ties the previous build flagged, when equal losses did
 * not straddle the split (the below set is kept too).  Same outputs as
 * tpe_build_posterior_resident_ordered; the others' tie flags read 0. */
int tpe_rebuild_labels(tpe_ctx *ctx, const double *losses, int64_t n_trials, int64_t n_valid,
                       double gamma, double prior_weight, int32_t lf, const int64_t *order_off,
                       const int32_t *order, const int32_t *labels, int32_t n_only,
                       int32_t *n_below_out, int32_t *ties);

/* Read back one mixture of the resident posterior built by
 * tpe_build_posterior (side 0 below, 1 above): the (weights, mus, sigmas)
 * that adaptive_parzen_normal returns (categorical: p in weights).  *n
 * receives the component count; at most `cap` entries are written. */
int tpe_get_mixture(tpe_ctx *ctx, int32_t label, int32_t side, double *weights,
                    double *mus, double *sigmas, int32_t cap, int32_t *n);

/* Number of labels of the resident posterior (the row count tpe_suggest
 * writes per round). */
int32_t tpe_resident_labels(const tpe_ctx *ctx);

/* Device time (ms, HIP events) of the last tpe_build_posterior's kernels
 * (-1 for a rebuild whose report was deferred, TPE_OPT_DEFER_REPORT). */
int tpe_last_build_ms(const tpe_ctx *ctx, float *ms);

/* The last build's report, applied first if it was deferred
 * (TPE_OPT_DEFER_REPORT): n_below and the tie report tpe_rebuild_labels
 * returns (ties: n_labels + 1 entries, NULL to skip).  After a
 * tpe_rebuild_labels the flags of the labels outside its subset read 0 --
 * on a label-sharded multi-device context also those of a device that holds
 * none of the subset's labels, as on one device.  Replaces nothing in
 * the reference: the deferral is this library's (posterior.py
 * _build_reference_order reads it after the round). */
int tpe_build_report(tpe_ctx *ctx, int32_t *n_below, int32_t *ties);

/* One suggestion round over every resident label: sample n_candidates per
 * label from the below posterior (global candidate indices
 * cand_offset .. cand_offset+n_candidates-1), score them under both
 * posteriors and keep the best (the GMM1 -> *_lpdf x2 -> broadcast_best
 * chain of tpe.py:686-724, rec_eval'd per label at tpe.py:900).
 * out[label] receives the winner.  `round` separates independent rounds
 * (e.g. new_id) under one seed. */
int tpe_suggest(tpe_ctx *ctx, uint64_t seed, uint32_t round, int64_t n_candidates,
                int64_t cand_offset, tpe_label_result *out);

/* Batched independent rounds (several new_ids at once): round j uses
 * rounds[j]; out has n_rounds * n_labels entries, round-major. */
int tpe_suggest_batch(tpe_ctx *ctx, uint64_t seed, const uint32_t *rounds,
                      int32_t n_rounds, int64_t n_candidates, int64_t cand_offset,
                      tpe_label_result *out);

/* tpe_suggest_batch with the results left in DEVICE memory: d_out (on this
 * single-device context's GPU, n_rounds * n_labels entries) receives them
 * by a device-to-device copy, complete when the call returns -- the buffer a
 * process-per-GPU caller all-gathers over RCCL without a host round trip
 * (the reference's one algo call per round, fmin.py:201-202).
 * out (host, may be NULL) receives them too.  The call runs on the
 * context's own stream: the caller completes any work of its own streams on
 * d_out first. */
int tpe_suggest_batch_device(tpe_ctx *ctx, uint64_t seed, const uint32_t *rounds,
                             int32_t n_rounds, int64_t n_candidates, int64_t cand_offset,
                             tpe_label_result *d_out, tpe_label_result *out);

/* tpe_merge_results on device buffers of ctx's GPU (d_parts: n_parts blocks
 * of n results, e.g. an RCCL all-gather of the ranks' tpe_suggest_batch_device
 * outputs; d_out: n results), on the context's stream, complete on return.
 * d_parts must be complete when called (an H2D copy or collective on another
 * stream synchronised first: nothing orders it against this stream). */
int tpe_merge_results_device(tpe_ctx *ctx, const tpe_label_result *d_parts, int32_t n_parts,
                             int32_t n, tpe_label_result *d_out);

/* north_star's multi-GPU partition (the reference builds each
 * label's posterior once per suggest call, tpe.py:678-692, and the ranks here
 * split that work): a rank builds the posterior and expansion index of the
 * labels it owns (tpe_build_posterior_resident* over its label shard, each
 * spec carrying its TPE_HAS_STREAM space index), exports them as one device
 * blob, the ranks all-gather the blobs over RCCL, and each imports the
 * assembled posterior of every label to score its slice of the candidates
 * (cand_offset) -- the slices' winners merge with tpe_merge_results_device.
 *
 * tpe_export_posterior: the resident posterior, with its expansion index
 * (queued first when the context's screen would build one), into d_out on
 * this context's GPU.  *bytes receives the blob size; d_out NULL or cap
 * smaller than it is a size query (nothing written).  Complete on return.
 *
 * tpe_import_posterior: replace the resident posterior with the labels of
 * n_parts blobs in d_blobs (blob_bytes long; part p at part_off[p], a
 * multiple of 256, holding part_labels[p] labels).  label_ids lists, part
 * by part, the space index of each blob label: together a permutation of
 * 0..L-1, L = sum part_labels; imported label label_ids[i] is the resident
 * label of that index.  The records, sampling records and index come over
 * device to device (one copy kernel); rounds on the result are the rounds of
 * one context that built every label.  Complete on return.  The built
 * mixtures are not imported (tpe_get_mixture refuses until the next build). */
int tpe_export_posterior(tpe_ctx *ctx, void *d_out, int64_t cap, int64_t *bytes);
int tpe_import_posterior(tpe_ctx *ctx, const void *d_blobs, int64_t blob_bytes, const int64_t *part_off,
                         int32_t n_parts, const int32_t *part_labels, const int32_t *label_ids);

/* ---- multivariate (joint) TPE ---------------------------------------------
 * A joint group of D dense continuous labels modelled together: each side's
 * mixture has one product kernel per trial (component 0 is the prior),
 *   f_S(y) = (1/A_S) sum_k W_k prod_d phi(y_d; mu_kd, s_kd)  on the box
 *   prod_d [low_d, high_d),  A_S = sum_k W_k prod_d m_kd  (m_kd: the mass of
 *   N(mu_kd, s_kd) in [low_d, high_d), 1 without both bounds),
 * in each label's working space (y = log x for TPE_LGMM1 dimensions; low and
 * high are working-space bounds), lpdf_S(x) = log f_S(y) - sum_{d log} y_d.
 * Candidate g of a round picks a below component with the pick word of the
 * reserved Philox stream TPE_JOINT_STREAM (cumulative W_k prod_d m_kd / A) and
 * draws dimension d from that component's normal truncated to [low_d, high_d)
 * with the two words of the dimension's own stream.  The joint posterior is
 * separate from the resident per-label posterior.
 *
 * Multi-device contexts (tpe_ctx_create_multi), label-sharded or not, hold
 * every joint posterior on every device: tpe_joint_set_group,
 * tpe_joint_condition_group and
 * tpe_joint_clear_groups run on all of them (the fold is deterministic, so
 * the replicas are the same bits; an error on any device, TPE_ERR_SAMPLE
 * included, is the call's), and tpe_joint_build_groups builds every replica
 * from the univariate build.  tpe_joint_get_group, tpe_joint_draw_group and
 * tpe_joint_score_group answer from the primary device's replica.
 * tpe_joint_suggest_group and tpe_joint_suggest_batch split over the nd
 * devices like tpe_suggest: contiguous near-equal candidate ranges when
 * n_candidates >= 1024 nd (every (slot, round) cell runs on every device over
 * its range and the shards' winners merge in broadcast_best's order: larger
 * lpdf_below - lpdf_above, NaN greatest, lowest global index), else
 * contiguous near-equal ranges of whole rounds when n_rounds >= nd, else the
 * primary device alone -- the one-device results bit for bit either way;
 * tpe_last_timing then reports the slowest device. */
#define TPE_JOINT_STREAM 0x7FFFFFFF

typedef struct {
    int32_t kind;        /* TPE_GMM1 | TPE_LGMM1 (not read for a categorical dimension) */
    int32_t flags;       /* TPE_HAS_LOW | TPE_HAS_HIGH */
    double low, high;
    int32_t stream;      /* the label's Philox stream */
} tpe_joint_dim;         /* 32 bytes */

/* A context holds up to TPE_JOINT_MAX_GROUPS joint posteriors, one per slot,
 * each with the Philox stream of its component pick (tpe.suggest(group=True)
 * gives slot j TPE_JOINT_STREAM - j; a single group is slot 0 with
 * TPE_JOINT_STREAM).  A slot outside [0, TPE_JOINT_MAX_GROUPS), or one that is
 * not set where a call reads it: TPE_ERR_ARG. */
#define TPE_JOINT_MAX_GROUPS 64

/* tpe_joint_set_group: upload and fold both mixtures of one slot and leave the
 * other slots as they are -- weights w[k], means and sigmas row-major [k][d],
 * k = 0 the prior.  "This slot alone" is tpe_joint_clear_groups, then this
 * call: a refused posterior then leaves every slot unset.  q, upper and cat_p
 * may each be NULL (no dimension quantized / none categorical); an all-zero q
 * or upper is its NULL, the same instantiations and bits.
 *
 * Dense dimension (q[d] = 0, upper[d] = 0): as described above.
 *
 * Quantized dimension, q[d] > 0 its step.  W_k, mu_kd, s_kd, m_kd, A_S, the
 * component pick and the draw of y in the working space are those of the dense
 * dimension; the drawn value is x_d = rint(v / q_d) q_d with v = exp(y) for
 * TPE_LGMM1, and the factor of the dimension is the component's mass on the
 * value's interval,
 *   g_kd(x_d) = Phi((ub - mu_kd)/s_kd) - Phi((lb - mu_kd)/s_kd),
 *   ub = x_d + q_d/2, lb = x_d - q_d/2, clipped to [low, high] by the flags
 *   (TPE_GMM1), or clipped to [exp(low), exp(high)], lb = max(0, lb), then
 *   ub = log(max(ub, 1e-12)), lb = log(max(lb, 1e-12))  (TPE_LGMM1),
 * 0 for an empty interval (ub <= lb):
 *   f_S(x) = (1/A_S) sum_k W_k prod_d g_kd(x_d)     (g = phi for a dense d),
 *   lpdf_S(x) = log f_S(x) - sum_{d dense, TPE_LGMM1} y_d
 * (a quantized TPE_LGMM1 dimension has no Jacobian term: its factor is a
 * probability of the value).  A configuration no component reaches has lpdf
 * -inf.  Equal configurations get equal lpdf bits, so among them the lowest
 * index wins.
 *
 * Categorical dimension, upper[d] = C_d > 0 its categories 0 .. C_d - 1, with
 * prior p_d, the next C_d entries of cat_p (cat_p and prior_weight are read
 * only when a dimension is categorical).  With K_S = n_S the side's components
 * and a_Sd = C_d prior_weight / K_S the factor of category x in component k is
 *   r_0d[x] = p_d[x]                                        (the prior),
 *   r_td[x] = ([x == o_td] + a_Sd p_d[x]) / (1 + a_Sd)      (trial t observed o_td),
 *   g_kd(x_d) = r_kd[x_d],  m_kd = 1:
 * A_S, the pick thresholds and the pick stream are those of the group without
 * the dimension, and it has no Jacobian term.  The observed category of trial t
 * travels in mu*[k][d] (k >= 1), integer-valued; row 0 and sig*[.][d] of the
 * dimension are not read, nor are kind, flags, low and high of dims[d] -- its
 * stream is.  Values are doubles holding the category index.  A value that is
 * no integer in [0, C_d) has factor 0: lpdf -inf on both sides; NaN gives NaN.
 * The draw of dimension d takes word x of the Philox counter (g, 0, stream_d,
 * round) -- the categorical layout of the independent round -- and the first
 * category c with ceil(cdf_kd[c] 2^32) above it, cdf_kd the running sum of
 * r_kd in category order over its total, the last entry 1.
 *
 * Accepted groups: S = n_dims + (number of quantized dimensions) <= 128 -- a
 * candidate keeps one value per dense or categorical and two (ub, lb) per
 * quantized dimension in LDS.  A group with a quantized or categorical
 * dimension runs the quantized variant of the round; the draw, score, suggest
 * and batch calls serve every slot.
 * TPE_ERR_ARG: a NULL dims or mixture pointer; n_dims outside [1, 128] or
 * S > 128; n_below outside [1, 4096] or n_above < 1; a kind that is not
 * TPE_GMM1 or TPE_LGMM1, or flags other than the two bounds; q[d] negative,
 * NaN or infinite; upper[d] < 0; q[d] > 0 and upper[d] > 0; a categorical
 * dimension with cat_p NULL, a p entry that is not positive and finite, a p
 * whose sum is not within 1e-9 of 1, an observed category that is no integer
 * in [0, upper[d]), or prior_weight not positive and finite.
 * TPE_ERR_VALUE: low >= high; a negative or NaN weight; a sigma that
 * is not positive and finite.  TPE_ERR_SAMPLE when the box holds none of the
 * below mixture's mass: the slot counts as set, and the draw, suggest and
 * batch calls return it too. */
int tpe_joint_set_group(tpe_ctx *ctx, int32_t slot, uint32_t pick_stream, const tpe_joint_dim *dims,
                        const double *q /* [n_dims], 0 = dense; NULL */,
                        const int32_t *upper /* [n_dims], 0 = not categorical; NULL */,
                        const double *cat_p /* the categorical dimensions' priors, concatenated; NULL */,
                        double prior_weight, int32_t n_dims, int32_t n_below, const double *wb,
                        const double *mub, const double *sigb, int32_t n_above, const double *wa,
                        const double *mua, const double *siga);
/* Condition a set slot on the values of some of its dimensions ("suggest with
 * these hyperparameters held fixed"): dst_slot receives the group over the
 * free dimensions R of src_slot, in their source order, given the n_fixed
 * dimensions F = dims[] (distinct indices of the source) at values[] -- label
 * values as documents carry them: x, not log x; a category index as a double.
 * A mixture of product kernels conditions in closed form: each side's
 * conditional is again a mixture of product kernels over R whose components
 * keep their means and sigmas (the free columns are copied bit for bit), and
 * only the weights change,
 *   L_k  = log W_k + sum_{d in F} log g_kd(x_d),
 *   lse  = L_max + log(sum_k exp(L_k - L_max)),
 *   W'_k = max(exp(L_k - lse), 2^-1022),
 * g_kd the factor tpe_joint_set_group defines for the dimension: phi(y_d; mu_kd,
 * s_kd) in the working space (dense), the rounding-interval mass (quantized),
 * r_kd[x_d] (categorical, a_Sd with the source's K_S, which does not change).
 * The floor keeps log W'_k finite for the fold (it adds at most K 2^-1022 of
 * relative mass); a component with L_k = -inf (an empty quantized interval)
 * takes it.  The truncation needs nothing more: A_S is the fold's, over R, and
 * lpdf_S(x_R | x_F) differs from the source's lpdf_S(x_F, x_R) by a constant, so
 * the conditioned slot's scores order candidates as the source orders them at
 * x_F.  dst_slot keeps the source's pick stream, each free dimension's stream,
 * q, upper, cat_p, the prior weight and both component counts: it is the slot
 * tpe_joint_set_group(W', free columns) makes.  dst_slot == src_slot conditions
 * in place, with the same result.  The sums run over one fixed tree per side
 * (no atomics), so equal sources give equal bits on every device.
 * TPE_ERR_ARG: a slot out of range or src_slot not set; n_fixed outside
 * [1, n_dims - 1]; a repeated or out-of-range dimension; a NULL pointer.
 * TPE_ERR_VALUE: a NaN value; every component of a side has L_k = -inf (a value
 * no component reaches) -- the destination is left as it was.  TPE_ERR_SAMPLE
 * as tpe_joint_set_group.  A multi-device context conditions every device's
 * replica; an error on any device is the call's. */
int tpe_joint_condition_group(tpe_ctx *ctx, int32_t src_slot, int32_t dst_slot, int32_t n_fixed,
                              const int32_t *dims, const double *values);
/* Unset every slot (their buffers are kept for the next posterior). */
int tpe_joint_clear_groups(tpe_ctx *ctx);
/* Joint groups built on the device from the current build of the resident
 * history (tpe_build_posterior_resident and its kin) -- nothing is uploaded but
 * the arguments.  The joint mixture of a group is its labels' univariate
 * mixtures read back in trial order (row 0 the prior, row t + 1 the t-th
 * observation of the side in observation order, each with the sigma and the
 * weight its own sorted position gave it; W is the first non-categorical
 * label's; a categorical label's rows hold the observed categories, sigma 1):
 * one launch un-permutes them into the arrays tpe_joint_set_group takes,
 * then each slot is folded as that call folds it -- the same bits wherever the
 * univariate mixtures are the host's.  One stream synchronisation per call.
 * Group g is labels[group_off[g] .. group_off[g + 1]) -- indices of the
 * resident history's labels, whose tpe_label_spec supplies kind, bounds and
 * prior -- in slot slots[g] with pick stream pick_streams[g]; streams, q and
 * upper are parallel to labels (q, upper: NULL or 0 as in
 * tpe_joint_set_group; upper[i] must be the label's own), cat_p the
 * categorical labels' priors concatenated in that order.
 * flags[g] != 0: the group was not built and its slot is left unset (the other
 * groups are built) --
 *   TPE_JOINT_FLAG_TIE       a label's side holds two equal observations (or a
 *                            NaN) whose np.argsort order the build was not given
 *                            (tpe_build_posterior_resident_ordered /
 *                            tpe_rebuild_labels): which trial gets which sigma
 *                            would depend on the tie order,
 *   TPE_JOINT_FLAG_CATEGORY  an observed category is no integer in [0, upper),
 *   TPE_JOINT_FLAG_COUNT     the group's labels do not hold the same number of
 *                            observations on a side.
 * TPE_ERR_ARG: no build of the resident history is current (none, a failed one,
 * or the history appended to or reset since); a label index out of range or
 * listed twice; a slot out of range or used twice; a group without a
 * non-categorical label; upper[i] not the label's; more than 128 dimensions
 * (plus quantized dimensions), 4096 below components or TPE_JOINT_MAX_GROUPS
 * groups.  TPE_ERR_SAMPLE as tpe_joint_set_group.
 * Multi-device contexts: a replicated one (label shards off) runs the call
 * on every device, the flags are the primary's.  On a label-sharded one a
 * group's labels live on different devices: each device gathers the columns
 * (W, mu, sigma per label) of the labels it owns and synchronises, then
 * every device copies in the columns it does not own, device to device --
 * (16 D + 8) K bytes per group and further device, K both sides' components,
 * nothing through host memory -- interleaves them into the [K][D] arrays and
 * folds.  The flags are OR-ed over the devices, a flagged group is left
 * unset on every device, and the validation is the one above against the
 * owners' records. */
#define TPE_JOINT_FLAG_TIE 1
#define TPE_JOINT_FLAG_CATEGORY 2
#define TPE_JOINT_FLAG_COUNT 4
int tpe_joint_build_groups(tpe_ctx *ctx, int32_t n_groups, const int32_t *slots,
                           const uint32_t *pick_streams, const int64_t *group_off /* [n_groups + 1] */,
                           const int32_t *labels, const int32_t *streams, const double *q,
                           const int32_t *upper, const double *cat_p, double prior_weight,
                           int32_t *flags /* [n_groups] */);
/* tpe_joint_build_groups with the bandwidth rule of the groups' kernels;
 * tpe_joint_build_groups is this call with TPE_JOINT_BW_NEIGHBOUR.
 *   TPE_JOINT_BW_NEIGHBOUR  the rule above: each trial's sigma in dimension d
 *                           is the one the univariate build gave it (the gap
 *                           to its neighbours in the sorted values of label d),
 *   TPE_JOINT_BW_SCOTT      one sigma per (side, dimension) from the number of
 *                           trials and the dimension: with n trials on the
 *                           side, K = n + 1 components and D labels in the
 *                           group (categorical ones counted),
 *                             s_d = clip(f psig_d, psig_d / min(100, 1 + K), psig_d),
 *                             f = tpe_joint_bandwidth_factor(n, D) = 0.2 n^(-1/(D+4)),
 *                           psig_d the label's prior sigma (tpe_label_spec);
 *                           row 0 keeps psig_d; categorical rows as above.  W
 *                           = w / sum(w), w = (prior_weight, the linear-
 *                           forgetting weights of n trials, lf = 25) in trial
 *                           order, the sum in numpy's pairwise order; means
 *                           as above.  prior_weight must be positive and
 *                           finite whatever the labels (TPE_ERR_ARG).
 * The Scott rule reads neither the univariate weights and sigmas nor a sorted
 * position -- two equal observations get equal rows -- so it never raises
 * TPE_JOINT_FLAG_TIE; _CATEGORY and _COUNT are raised as above.  The factor is
 * computed on the host (0.2 * pow((double)n, -1.0 / (double)(D + 4)), 0.2 for
 * n <= 1) and handed to the kernel, so a host build that evaluates the same
 * expression gets the same bits.  Any other bandwidth: TPE_ERR_ARG.
 * Multi-device contexts as tpe_joint_build_groups; under label shards the
 * owner of a group's first non-categorical label forms its W column. */
#define TPE_JOINT_BW_NEIGHBOUR 0
#define TPE_JOINT_BW_SCOTT 1
int tpe_joint_build_groups_bw(tpe_ctx *ctx, int32_t n_groups, const int32_t *slots,
                              const uint32_t *pick_streams, const int64_t *group_off /* [n_groups + 1] */,
                              const int32_t *labels, const int32_t *streams, const double *q,
                              const int32_t *upper, const double *cat_p, double prior_weight,
                              int32_t bandwidth, int32_t *flags /* [n_groups] */);
double tpe_joint_bandwidth_factor(int32_t n, int32_t D);
/* A set slot's unfolded arrays, however it was set (tests, diagnostics): the
 * first min(cap, K) components of side 0 (below) or 1 (above) -- w[k], mu and
 * sigma [k][D] row-major; K and D through n_components and n_dims.  Output
 * pointers may be NULL. */
int tpe_joint_get_group(tpe_ctx *ctx, int32_t slot, int32_t side, double *w, double *mu, double *sigma,
                        int32_t cap, int32_t *n_components, int32_t *n_dims);
/* Candidates cand_offset .. cand_offset + n - 1 of (seed, round) of a set
 * slot: values[n D] row-major and the below component each was drawn from. */
int tpe_joint_draw_group(tpe_ctx *ctx, int32_t slot, uint64_t seed, uint32_t round, int64_t n,
                         int64_t cand_offset, double *values, int32_t *comp);
/* Joint lpdfs of supplied configurations values[n D]: ll below, lg above. */
int tpe_joint_score_group(tpe_ctx *ctx, int32_t slot, const double *values, int64_t n, double *ll,
                          double *lg);
/* One fused round: draw n_candidates, score both sides, broadcast_best's
 * winner (NaN greatest, lowest index on ties): its D values, index and lpdfs. */
int tpe_joint_suggest_group(tpe_ctx *ctx, int32_t slot, uint64_t seed, uint32_t round,
                            int64_t n_candidates, double *values, int64_t *index, double *ll, double *lg);
/* tpe_joint_suggest_group for every set slot (ascending) and every round
 * rounds[r], bit for bit, in packed launches: the lanes run over the flat
 * index of (round, candidate), so the launches, copies and the one stream
 * synchronisation of a call do not grow with n_rounds.  values[n_rounds][sum
 * of D over the set slots] (the slots' values concatenated per round); index,
 * ll, lg [n_rounds][number of set slots].  TPE_ERR_ARG when no slot is set,
 * TPE_ERR_SAMPLE as tpe_joint_suggest_group. */
int tpe_joint_suggest_batch(tpe_ctx *ctx, uint64_t seed, const uint32_t *rounds, int32_t n_rounds,
                            int64_t n_candidates, double *values, int64_t *index, double *ll, double *lg);
/* How the last tpe_joint_suggest_group / tpe_joint_suggest_batch call was
 * split: mode 0 the primary device alone (always so on a one-device context),
 * 1 candidate shards, 2 round shards; n_devices the devices that ran a shard.
 * Either pointer may be NULL. */
int tpe_joint_last_shards(const tpe_ctx *ctx, int32_t *mode, int32_t *n_devices);

/* ---- candidate pools ------------------------------------------------------
 * Rank a finite, caller-supplied set of whole configurations under the
 * current posterior (no reference counterpart: the reference only draws its
 * candidates, tpe.py:686-724; the acquisition is the one broadcast_best ranks
 * by, tpe.py:769-778, summed over a configuration's labels).
 *
 * tpe_pool_set uploads the pool once: values[n][n_cols] row-major, one column
 * per label of the posterior it will be ranked under, NaN where the label is
 * not active in the entry (a conditional branch not taken); values as documents
 * carry them (x, not log x; a category index as a double).  It stays on the
 * device, column-major, across tpe_set_posterior and every build, until the
 * next tpe_pool_set, tpe_pool_clear or tpe_ctx_destroy.  tpe_pool_size reports
 * it (0, 0: none).
 *
 * tpe_pool_rank, for every entry i:
 *   term of an active column c (value v): lb - la, lb and la the lpdfs
 *       tpe_score(ctx, c, v) defines under the resident posterior, one fp64
 *       subtraction;
 *   a listed joint group g (slot slots[g], set by tpe_joint_set_group or a
 *       device build) covers the columns group_cols[group_off[g] ..
 *       group_off[g + 1]): they get no term of their own, the group's lb, la
 *       are tpe_joint_score_group's ll, lg on those columns in that order, and
 *       the group is inactive for an entry with a NaN in any of them;
 *   score[i] = the fp64 sum, from 0.0 and left to right, of the uncovered
 *       active columns' terms in ascending column order, then the listed
 *       groups' in the order listed (no term: 0.0; a NaN term, e.g. -inf - -inf:
 *       NaN).  One thread adds an entry's terms and every term is computed from
 *       the entry's own value alone, so a score depends neither on n, on the
 *       entry's position nor on the other entries; equal inputs give equal bits.
 * The order is broadcast_best's: NaN greatest, then the larger score, then the
 * lowest index.  Entries listed in taken[n_taken] are left out (duplicates and
 * indices outside [0, n) are ignored); *n_top = min(top_k, entries not taken)
 * pairs (top_index, top_score) are written, best first.  score (NULL, or [n])
 * receives every entry's score, taken ones included; lpdf_below / lpdf_above
 * (both NULL, or both [n][n_cols + n_groups] row-major) the terms' lpdfs,
 * column n_cols + g the group g's, NaN in both for an inactive or covered
 * cell.
 * One stream synchronisation per call (the optional vectors are copied after
 * it); nothing is uploaded but the arguments.
 * TPE_ERR_ARG: no pool set; no posterior, or n_cols is not its label count; a
 * slot that is unset or listed twice; a column out of range or in two groups;
 * a group whose column count is not its slot's D; top_k < 1; n < 1 or
 * n_cols < 1 (tpe_pool_set); a NULL pointer where one is needed; a TPE_F32
 * context; a multi-device context (tpe_pool_set too).  TPE_ERR_VALUE: at
 * tpe_pool_set a value of +-inf; at tpe_pool_rank what the plain round flags
 * for a supplied candidate -- an active categorical value that is no integer
 * in [0, upper), a quantized LGMM1 value whose interval's upper end is
 * negative.  TPE_ERR_SAMPLE as tpe_joint_score_group.  On an error the
 * outputs are untouched. */
int tpe_pool_set(tpe_ctx *ctx, const double *values /* [n][n_cols] row-major, NaN = label not active */,
                 int64_t n, int32_t n_cols);
int tpe_pool_clear(tpe_ctx *ctx);
int tpe_pool_size(const tpe_ctx *ctx, int64_t *n, int32_t *n_cols);
int tpe_pool_rank(tpe_ctx *ctx, int32_t n_groups, const int32_t *slots, const int64_t *group_off /* [n_groups+1] */,
                  const int32_t *group_cols, const int64_t *taken, int64_t n_taken, int32_t top_k,
                  int64_t *top_index, double *top_score, int32_t *n_top,
                  double *score /* [n] or NULL */,
                  double *lpdf_below, double *lpdf_above /* [n][n_cols + n_groups] or NULL: diagnostics */);

/* tpe_pool_draw: TPE's own step on the resident pool -- draw m entries from
 * the good-trial density l, seeded and without replacement, and return the
 * drawn entry with the best l/g -- once per round, all on the device.  The
 * pool, the posterior, the groups, `taken`, the planes lb / la and score[i] are
 * tpe_pool_rank's.
 *   lsum[i] (the draw weight, log l of entry i): the fp64 sum, from 0.0 and
 *       left to right, over the same terms in the same order as score[i], each
 *       term the below lpdf in the label's working space: lb for every kind
 *       but a dense log label (loguniform, lognormal), whose term is
 *       lb + log v (one fp64 add; v the entry's value); a group's is
 *       ll + (the sum, from 0.0, of log v_d over its dense log columns in the
 *       order the group lists them).  No term: 0.0.  In the working space the
 *       prior of uniform and loguniform labels is flat (the document-space
 *       density's Jacobian 1/x would weight a log-spaced grid by 1/x); for the
 *       normal kinds the prior's own factor remains.
 *   noise of entry i (its pool index) in round r under seed s:
 *       (w0, w1, ., .) = philox4x32_10(counter (i, 0, TPE_POOL_STREAM, r),
 *       key (s & 0xffffffff, s >> 32)); t = (w0 << 20) | (w1 >> 12), 52 bits;
 *       u = (t + 0.5) 2^-52, exact and strictly inside (0, 1);
 *       G = -log(-log u), standard Gumbel; key_r[i] = lsum[i] + G.  A key
 *       depends on (s, r, i, lsum[i]) alone.
 *   round j = 0 .. n_rounds - 1, in order, r = rounds[j]: free_j is the entries
 *       not in `taken` and, with distinct != 0, not among best_index[0 .. j);
 *       an empty free_j ends the call with *n_best = j.  drawn_j is the
 *       d_j = min(m, |free_j|) entries of free_j first by key descending (NaN
 *       greatest), then index ascending -- the Gumbel top-m form of a draw
 *       without replacement with probabilities proportional to l (m = 1:
 *       P(i) = l_i / sum l); an entry with l = 0 is drawn only when fewer than
 *       d_j entries have a finite key.  best_index[j] is the entry of drawn_j
 *       first in tpe_pool_rank's order of score, best_score[j] its score.
 *   With m >= |free_0| and distinct != 0, best_index / best_score are
 *   tpe_pool_rank's top n_rounds bit for bit, whatever the seed.
 * Diagnostics, each NULL or given: drawn [n_rounds][min(m, n)] with n_drawn
 * [n_rounds] (both or neither): row j's first n_drawn[j] = d_j values are
 * drawn_j in that order, 0 for a round past *n_best; lsum [n]; keys
 * [n_rounds][n]: every entry's key of the round, entries that are not free
 * included; score [n] as tpe_pool_rank's.
 * One stream synchronisation per call, the planes computed once per call; the
 * optional vectors are copied after it.  Errors as tpe_pool_rank (TPE_ERR_ARG,
 * a multi-device or TPE_F32 context included; TPE_ERR_VALUE; TPE_ERR_SAMPLE),
 * and TPE_ERR_ARG for m < 1, n_rounds outside [1, 4096], a NULL rounds,
 * best_index, best_score or n_best, drawn without n_drawn or the reverse.  On
 * an error the outputs are untouched. */
#define TPE_POOL_STREAM 0x7FFFFFBF   /* the first stream below the pick streams TPE_JOINT_STREAM - j */
int tpe_pool_draw(tpe_ctx *ctx, int32_t n_groups, const int32_t *slots, const int64_t *group_off,
                  const int32_t *group_cols, const int64_t *taken, int64_t n_taken,
                  uint64_t seed, const uint32_t *rounds, int32_t n_rounds, int64_t m, int32_t distinct,
                  int64_t *best_index /* [n_rounds] */, double *best_score /* [n_rounds] */, int32_t *n_best,
                  int64_t *drawn /* [n_rounds][min(m, n)] or NULL */, int32_t *n_drawn /* [n_rounds] or NULL */,
                  double *lsum /* [n] or NULL */, double *keys /* [n_rounds][n] or NULL */,
                  double *score /* [n] or NULL */);

/* ---- several objectives ---------------------------------------------------
 * The Pareto-compliant total order of n objective vectors, all objectives
 * minimised (no reference counterpart: the reference splits the trials by one
 * loss, tpe.py:624-648; tpe.suggest(objectives=...) splits them by these keys
 * instead).  objectives[n][n_obj] row-major, row i the vector F[i] of trial i,
 * compared by IEEE comparisons: -0.0 equals 0.0, +-inf are ordinary values.
 *   i dominates j: F[i][m] <= F[j][m] for every m and F[i][m] < F[j][m] for
 *       one; equal rows do not dominate each other;
 *   dominated_by[i]: the number of rows that dominate i (0 exactly on the
 *       Pareto front; smaller for a than for b whenever a dominates b);
 *   dominates[i]: the number of rows i dominates;
 *   the order: ascending dominated_by, then descending dominates, then
 *       ascending i; keys[i] is row i's position in it, 0 .. n - 1 (distinct
 *       integers as doubles; n_obj = 1: the stable argsort rank of the column);
 *   a row with a NaN in any objective is compared with nobody and counted by
 *       nobody: keys[i] = NaN, dominated_by[i] = dominates[i] = -1, and the
 *       other rows' keys are their positions among the rows without a NaN.
 * All n^2 pairs are tested on the device, each row's two counters summed as
 * integers (the same bits on every run and device); one radix sort of (by,
 * n - do, i) packed into 3 x 21 bits gives the positions, hence n <= 2^20.
 * dominated_by and dominates may each be NULL.
 * One stream synchronisation per call.  Nothing is kept on the context but
 * reusable buffers (counted by tpe_device_bytes); no posterior, history or
 * pool is read or changed.  A multi-device context runs it on its primary
 * device.
 * TPE_ERR_ARG: a NULL objectives or keys; n < 1 or n > 2^20; n_obj outside
 * [1, 8].  On an error the outputs are untouched. */
int tpe_mo_keys(tpe_ctx *ctx, const double *objectives /* [n][n_obj] row-major */,
                int64_t n, int32_t n_obj, double *keys /* [n] */,
                int32_t *dominated_by /* [n] or NULL */, int32_t *dominates /* [n] or NULL */);

/* The same order under constraints (tpe.suggest(constraints=...)): feasible
 * rows first, in the order above among themselves, then the infeasible rows by
 * ascending violation.  constraints[n][n_con] row-major, c <= 0 satisfied,
 * c > 0 violated by that amount; IEEE comparisons throughout.
 *   a row with a NaN in any objective or constraint is dead: keys[i] = NaN,
 *       dominated_by[i] = dominates[i] = -1, violation[i] = NaN, and it counts
 *       for no other row;
 *   violation[i] = ((0.0 + max(G[i][0], 0)) + max(G[i][1], 0)) + ... in fp64,
 *       in this order (additions only: the bits a host loop gives; -inf and
 *       -0.0 contribute zero, +inf is an ordinary value);
 *   a row is feasible when violation[i] == 0;
 *   feasible rows: dominated_by and dominates as above, counted among the
 *       feasible rows only -- an infeasible row dominates nobody and is
 *       dominated by nobody;
 *   infeasible rows: dominated_by[i] = the live rows of strictly smaller
 *       violation (every feasible row is one: at least the number of feasible
 *       rows, more than any feasible row's), dominates[i] = 0;
 *   the order: ascending dominated_by, descending dominates, ascending i;
 *       keys[i] is the position, 0 .. (live rows) - 1.  Every row feasible:
 *       tpe_mo_keys' keys.  No row feasible: ascending violation, then i.
 * dominated_by, dominates and violation may each be NULL.  One upload, one
 * stream synchronisation, pinned read-back; its own reusable buffers (counted
 * by tpe_device_bytes) are allocated by the first such call, never by
 * tpe_mo_keys, whose results it does not change.  A multi-device context runs
 * it on its primary device.
 * TPE_ERR_ARG: a NULL objectives, constraints or keys; n < 1 or n > 2^20;
 * n_obj or n_con outside [1, 8].  On an error the outputs are untouched. */
int tpe_mo_keys_constrained(tpe_ctx *ctx, const double *objectives /* [n][n_obj] row-major */,
                            int64_t n, int32_t n_obj,
                            const double *constraints /* [n][n_con] row-major */, int32_t n_con,
                            double *keys /* [n] */, int32_t *dominated_by /* [n] or NULL */,
                            int32_t *dominates /* [n] or NULL */, double *violation /* [n] or NULL */);

/* Hyperparameter importance from the resident posterior (tpe.importance;
 * no reference counterpart -- Optuna's PED-ANOVA evaluator is the nearest).
 * For each of the n_sel selected labels, with l / g its below / above mixture,
 * alpha the share of its observations among the good trials and the cells
 * (x_j, w_j), j in [cell_off[s], cell_off[s + 1]):
 *     p(x) = alpha l(x) + (1 - alpha) g(x),   m(x) = alpha l(x) / p(x),
 *     v[s] = sum_j w_j p(x_j) (m(x_j) - alpha)^2
 * -- the variance, under the density of the label's observed values, of the
 * model's probability that a trial with that value is good.  The lpdfs at x_j
 * are tpe_score's, bit for bit; a cell of a quantized label with merge[s] > 1
 * takes the quantized lpdf with the step merge[s] q (the mass of merge[s]
 * consecutive support values around their mean x_j).  Per cell, from lb =
 * log l(x_j) and la = log g(x_j), in this order and without cancellation:
 *     d = lb - la
 *     d <= 0:  t = expm1(d),   dev =  alpha (1 - alpha) t / (1 + alpha t)
 *     d >  0:  t = expm1(-d),  dev = -alpha (1 - alpha) t / (1 + (1 - alpha) t)
 *     term = w_j (alpha exp(lb) + (1 - alpha) exp(la)) dev^2
 * a cell with lb = la = -inf contributes 0, a NaN lpdf makes v[s] NaN.  The
 * terms of 256 consecutive cells are added in a fixed order and a label's
 * partial sums in ascending order: v[s] is the same bits on every run, and
 * whichever other labels the call lists, in whatever order.  v[s] = 0 for a
 * label without cells.  lb / la (both or neither): the two lpdf planes, in the
 * layout of x.  The call runs on the resident posterior however it was set or
 * built and changes neither it nor the pool; one stream synchronisation; a
 * multi-device context runs it on its primary device (not a label-sharded
 * one).  TPE_F64 contexts.
 * TPE_ERR_ARG (tpe_last_error names the function): no posterior; a NULL
 * argument other than lb / la; a label out of range or listed twice; alpha
 * outside (0, 1); merge < 1, or merge != 1 on a label that is not quantized;
 * cell_off[0] != 0 or decreasing offsets.  TPE_ERR_VALUE: a categorical
 * label's point that is not an integer in [0, upper); a quantized LGMM1
 * label's cell whose upper end is negative.  On an error the outputs are
 * untouched. */
int tpe_importance(tpe_ctx *ctx, int32_t n_sel, const int32_t *labels,
                   const int64_t *cell_off /* [n_sel + 1] */, const double *x, const double *w,
                   const int32_t *merge /* [n_sel] */, const double *alpha /* [n_sel] */,
                   double *v /* [n_sel] */, double *lb, double *la /* [cell_off[n_sel]] or NULL */);

/* Score a caller-supplied candidate set for one resident label (the parity
 * entry point: identical candidates in, both lpdf vectors and the winner
 * out).  lpdf_below / lpdf_above may be NULL. */
int tpe_score(tpe_ctx *ctx, int32_t label, const double *cand, int64_t n,
              double *lpdf_below, double *lpdf_above, tpe_label_result *out);

/* Merge per-shard winners (e.g. gathered from every GPU over RCCL) with the
 * broadcast_best comparator: larger score, NaN greatest, then lowest global
 * index.  parts: n_parts blocks of n results each.  Host-only, no ctx. */
int tpe_merge_results(const tpe_label_result *parts, int32_t n_parts, int32_t n,
                      tpe_label_result *out);

/* Device time (ms, HIP events on the context stream) of the last fused round:
 * scoring kernels only, and the whole round including the reduction. */
int tpe_last_timing(const tpe_ctx *ctx, float *score_ms, float *round_ms);

/* Number of (candidate, component) lpdf evaluations the last round executed,
 * counted over both mixtures (categorical: 2 per candidate). */
int64_t tpe_last_evals(const tpe_ctx *ctx);

/* Per kernel family of the last round (index: 0 dense GMM1, 1 dense LGMM1,
 * 2 quantized GMM1, 3 quantized LGMM1, 4 categorical): device ms of that
 * family's launch and the evaluations it executed.  Arrays of 5.  Sampled
 * tile/packed rounds launch both dense families together: slot 0 then holds
 * the GMM1 + LGMM1 launch and its evaluations, slot 1 stays 0. */
int tpe_last_mode_stats(const tpe_ctx *ctx, float *ms, int64_t *evals);

/* Candidates the last round screened in fp32 (sampled tile-map rounds of
 * the dense GMM1/LGMM1 labels, TPE_F64 contexts) and how many of them it
 * re-scored in fp64 -- those whose rigorous fp32 error interval reaches the
 * largest lower bound of their round; the winner and its lpdfs are those
 * of the plain fp64 round (tpe_device.h screen_err).  screen_ms: device
 * time of the fp32 screening kernel alone (HIP events). */
int tpe_last_screen(const tpe_ctx *ctx, int64_t *screened, int64_t *rescored,
                    float *screen_ms);

/* (candidate, component) terms the last round's screen actually summed
 * (both mixtures).  The windowed screen (TPE_OPT_WINDOW) leaves out the
 * components whose terms stay below 2^-T (TPE_OPT_WIN_T) of the largest
 * coefficient over a whole tile; the plain screen sums them all (then this
 * is screened x (nb + na)).  Winners are unaffected. */
int tpe_last_screen_terms(const tpe_ctx *ctx, int64_t *terms);

/* (candidate, component) terms the last round's fp64 re-score evaluated:
 * every re-scored candidate over both mixtures of its label (the exact
 * GMM1_lpdf / LGMM1_lpdf of tpe.py:110-172,265-307 on that candidate).
 * With tpe_last_screen_terms this is the dense work the round executed. */
int tpe_last_rescore_terms(const tpe_ctx *ctx, int64_t *terms);

/* Candidates the last round actually drew for its quantized and categorical
 * labels (TPE_OPT_EARLY: the exact early exit stops a label's round once a
 * candidate holds the best score any draw can have; the rest are never
 * drawn).  The categorical evals in tpe_last_mode_stats count these. */
int tpe_last_drawn(const tpe_ctx *ctx, int64_t *quantized, int64_t *categorical);

/* Device memory the library holds right now, over every context of the
 * process (posteriors, resident histories, expansion indexes, round
 * buffers; the HIP runtime's own allocations not included), in bytes.
 * Buffers grow by 1/4 and are kept between calls, so after a run this is
 * its high-water mark. */
int64_t tpe_device_bytes(void);

/* Which screen the last round's dense tile-map labels went through: 0 none
 * (unscreened fp64, fp32 precision, or no dense tile round), 1 the plain
 * fp32 screen, 2 the windowed fp32 screen, 3 the expansion screen
 * (TPE_OPT_EXPAND); packed-map rounds report 3 when the expansion screen
 * ran, else 0. */
int32_t tpe_last_screen_mode(const tpe_ctx *ctx);

/* The hot-bin prefilter of the last round's expansion screen (TPE_OPT_HOT):
 * the candidates it listed for the expansion screen (-1: it did not run) --
 * the others were proven unable to win from their sub-bin's score interval
 * (tpe_device.h "hot-bin prefilter") -- and whether the round fell back to
 * screening every candidate (1: a round's best lower bound stayed below the
 * listing threshold).  Winners are unaffected either way. */
int tpe_last_hot(const tpe_ctx *ctx, int64_t *listed, int32_t *fallback);

/* Device milliseconds (HIP events; TPE_OPT_TIMING on) of the last build of
 * the expansion screen's index -- bin tables, lists and the prefilter's
 * sub-bin bounds -- which runs once per posterior, before its first large
 * sampled round or in tpe_prepare (0 if it has not run).  Waits for the
 * index if it is still running. */
int tpe_last_prepare(tpe_ctx *ctx, float *ms);

/* Diagnostic of the hot-bin prefilter (tests): for caller-supplied
 * candidates of one dense resident label, the interval [lower, upper] of
 * the fp64 score over each candidate's sub-bin (+inf / -inf outside the
 * bins): lower <= lpdf_below - lpdf_above <= upper of tpe_score; mass: the
 * sub-bin's sampling mass under the below mixture (0 outside). */
int tpe_hot_probe(tpe_ctx *ctx, int32_t label, const double *cand, int64_t n,
                  double *upper, double *lower, double *mass);

/* Diagnostic of the expansion index (tests): the layout of one dense
 * resident label's bins, so that candidates can be aimed at bin and sub-bin
 * edges.  In recentred draw space x' = x - centre (GMM1) or log x - centre
 * (LGMM1), bin b covers [xlo + b bw, xlo + (b + 1) bw) and is cut into 16
 * sub-bins of equal width; n_nc: the unclipped above components (each
 * bin's list slot); tcut: the window's cut T.  Builds the index of the tile
 * rounds if it is not there, and fails as tpe_hot_probe does when the
 * posterior has none.  Any output pointer may be NULL. */
int tpe_bx_layout(tpe_ctx *ctx, int32_t label, double *xlo, double *bw, int32_t *nbins,
                  int32_t *n_nc, double *tcut, double *centre);

/* Diagnostic of the screen (tests): for caller-supplied candidates of one
 * dense resident label, the fp32 score lpdf_below - lpdf_above the screen
 * computes and its rigorous error bound (x 1.25, as used by the round):
 * |score32 - score64| <= err_bound for every finite bound.  With
 * TPE_OPT_WINDOW on and n >= 2048 the candidates go through the windowed
 * screen (sorted into tiles of neighbours, windows of components); with
 * TPE_OPT_EXPAND on, n >= 2048 and an eligible posterior, through the
 * expansion screen (score and bound in fp64). */
int tpe_screen_probe(tpe_ctx *ctx, int32_t label, const double *cand, int64_t n,
                     double *score32, double *err_bound);

/* Engine options (defaults in brackets):
 *   TPE_OPT_SCREEN  fp32 screen + fp64 re-score of sampled tile rounds [1]
 *   TPE_OPT_SPLITK  split-K map for small sampled rounds                [1]
 *   TPE_OPT_DEDUP   quantized labels scored once per grid value         [1]
 *   TPE_OPT_CHUNKS  chunks of the packed map's above mixtures (0 auto)  [0]
 *   TPE_OPT_WINDOW  windowed screen of large tile rounds: candidates sorted
 *                   into tiles of neighbours, each summed over the window of
 *                   components that can matter to it                   [1]
 *   TPE_OPT_WIN_T   the windowed screen's cut T: components left out of a
 *                   tile stay below 2^-T of the largest term (8..62)    [16]
 *   TPE_OPT_EXPAND  expansion screen of large tile rounds (taken before the
 *                   windowed one when every dense label qualifies): the
 *                   above mixture's equal-sigma components as a per-bin
 *                   Taylor polynomial in fp64, bounds ~1e-12, no sort.
 *                   Mixtures need not be ordered, but only above mixtures
 *                   ordered by mu get this index; others qualify for the
 *                   windowed screen only                                [1]
 *   TPE_OPT_HOT     hot-bin prefilter of the expansion screen: every
 *                   candidate is drawn and bounded by its sub-bin's score
 *                   interval; only those that can still win are scored
 *                   (2: tests -- a listing threshold no candidate reaches,
 *                   so every round takes the fallback)                  [1]
 *   TPE_OPT_EARLY   exact early exit of sampled tile rounds of quantized
 *                   (bounded) and categorical labels: candidates in index
 *                   order, stopped once one holds the best score any draw
 *                   can have (its first index is the np.argmax winner)  [1]
 *   TPE_OPT_HOT_DIV the hot-bin prefilter's lists hold n / HOT_DIV
 *                   candidates per (round, label) (at least 4096); a round
 *                   whose list overflows screens every candidate instead
 *                   and divides HOT_DIV by 4 for the next rounds        [16]
 *   TPE_OPT_ZERO_WIN  the packed map's fp64 re-score sums only the above
 *                   components whose terms can be nonzero at the wave's
 *                   candidates (the others are exactly +0.0: the same
 *                   bits)                                                 [1]
 *   TPE_OPT_VALUE_ONLY  packed-map rounds (batched small rounds) report
 *                   only the winner's index and value for a (round, label)
 *                   whose screen selected one candidate clearing every
 *                   other's upper bound by 1e-9 (relative): no fp64 lpdfs
 *                   are computed for it (score, lpdf_below, lpdf_above NaN);
 *                   the same index and value as the exact round.  For
 *                   callers that read the value only (tpe.suggest); not for
 *                   shards whose winners are merged by score            [0]
 *   TPE_OPT_RESCORE_CAP  candidates the packed map's re-score buffers hold
 *                   (grown when a round lists more: that round runs again;
 *                   tests set it small to take that path)               [65536]
 *   TPE_OPT_MODE_MASK  bit m set: rounds launch the labels of family m
 *                   (tpe_last_mode_stats' index: 1 | 2 dense, 4 | 8
 *                   quantized, 16 categorical); the other labels' result
 *                   entries are unspecified and their families' statistics
 *                   stay those of the round that last ran them.  Lets a
 *                   caller run the dense labels while the host still
 *                   computes the quantized labels' tie orders, then those
 *                   after their rebuild (posterior.py)                 [31]
 *   TPE_OPT_AUX_FAMILIES  sampled rounds run the quantized and categorical
 *                   labels on the context's second stream, beside the dense
 *                   labels' draw (joined before the reduction; results
 *                   unchanged; single-device contexts).  Their early exit's
 *                   draw counts (tpe_last_drawn, the families' evals) are
 *                   those of a scan in index order either way              [0]
 *   TPE_OPT_BX_SPLIT  workgroups per 64-bin block of the expansion index's
 *                   Taylor tables, each summing one part of the bins' window
 *                   (k_bx_table / k_bx_table_fin; 1..8, 0: enough for ~8192
 *                   workgroups)                                            [0]
 *   TPE_OPT_BX_T    the expansion index's window cut T (components left
 *                   out stay below 2^-T of the largest term; 32..128; 0:
 *                   64)                                                   [0]
 *   TPE_OPT_PK_SLICED  a packed-map round re-scores up to this many listed
 *                   candidates one wave per (64 candidates, summation slice)
 *                   instead of one thread per candidate walking its chunk
 *                   (same bits; 0: never; at most 65536)                [8192]
 *   TPE_OPT_DEFER_REPORT  1: the next tpe_rebuild_labels of quantized /
 *                   categorical labels only (run on the second stream
 *                   beside the expansion index) returns without waiting
 *                   for its report: its ties output is zeros, the next
 *                   round applies the report after queuing the dense
 *                   labels' kernels, any other call on the context first;
 *                   tpe_build_report then returns the real tie report
 *                   (single-device contexts; consumed by that rebuild)  [0]
 *   TPE_OPT_LABEL_SHARDS  multi-device contexts: the resident history's
 *                   labels partitioned over the devices (each device
 *                   appends, builds, indexes and runs whole rounds of its
 *                   labels; winners scattered to their space positions)
 *                   from the next tpe_history_reset with at least one label
 *                   per device; 0: every device holds every label and the
 *                   rounds split by candidates / rounds                  [1]
 *   TPE_OPT_JOINT_CAP  flat candidates (rounds x candidates) of one packed
 *                   launch of tpe_joint_suggest_batch; the rounds run in
 *                   chunks within it (same rows; tests; 0: the default,
 *                   at most 2^30)                                      [2^20]
 *   TPE_OPT_WIN_GROUPS  label groups of a windowed round, each sorted on a
 *                   second stream while the previous one is screened
 *                   (0: one group; the chip is busy either way)          [0]
 *   TPE_OPT_TIMING  HIP-event timing of every round (tpe_last_timing,
 *                   tpe_last_mode_stats, tpe_last_screen's ms); off saves
 *                   ~20 event calls per round on latency-bound calls   [1]
 *   TPE_OPT_WHOLE_N, TPE_OPT_WHOLE_ROUNDS  the whole problem's candidates
 *                   per round / rounds when this context computes one shard
 *                   of it (one process per GPU); map choices that change a
 *                   summation order follow the whole problem, so the merged
 *                   shards equal one context's round bit for bit     [0: this call's]
 * None of them changes a winner; they exist for tests, experiments and
 * sharded runs (TPE_OPT_VALUE_ONLY drops the lpdfs a caller does not read). */
#define TPE_OPT_SCREEN 1
#define TPE_OPT_SPLITK 2
#define TPE_OPT_DEDUP 3
#define TPE_OPT_CHUNKS 4
#define TPE_OPT_WHOLE_N 5
#define TPE_OPT_WHOLE_ROUNDS 6
#define TPE_OPT_TIMING 7
#define TPE_OPT_WINDOW 8
#define TPE_OPT_WIN_T 9
#define TPE_OPT_WIN_GROUPS 10
#define TPE_OPT_EXPAND 11
#define TPE_OPT_HOT 12
#define TPE_OPT_EARLY 13
#define TPE_OPT_HOT_DIV 14
#define TPE_OPT_ZERO_WIN 15
#define TPE_OPT_VALUE_ONLY 16
#define TPE_OPT_RESCORE_CAP 17
#define TPE_OPT_MODE_MASK 18
#define TPE_OPT_AUX_FAMILIES 19
/* (20: TPE_OPT_HOT32, the fp32 draw kernel -- measured slower, removed in round 6) */
#define TPE_OPT_BX_SPLIT 21
#define TPE_OPT_BX_T 22
#define TPE_OPT_PK_SLICED 23
#define TPE_OPT_DEFER_REPORT 24
#define TPE_OPT_LABEL_SHARDS 25
#define TPE_OPT_JOINT_CAP 26
int tpe_set_option(tpe_ctx *ctx, int32_t option, int64_t value);

/* Build now what the resident posterior's first round(s) of n_candidates
 * per label (n_rounds of them: tpe_suggest_batch) would build lazily: the
 * expansion screen's index (bin tables, lists, sub-bin bounds; fp64
 * contexts with the screen and TPE_OPT_EXPAND on, n_candidates x n_rounds
 * >= 8192; otherwise nothing) and, for rounds of >= 8192 candidates, the
 * hot-bin prefilter's threshold.  Lets a caller overlap the
 * index with host work (tpe.suggest computes numpy's tie orders meanwhile).
 * A later rebuild of the posterior that leaves every dense label
 * bit-identical keeps the index (compared on the device against a snapshot).
 * No reference counterpart: the reference has no index. */
int tpe_prepare(tpe_ctx *ctx, int64_t n_candidates, int32_t n_rounds);

/* Arm tpe_prepare(n_candidates, n_rounds) for the next device build of the
 * resident history (tpe_build_posterior_resident[_ordered], not a
 * label-subset rebuild): that build queues the index itself, right after its
 * own sync and before it returns -- tpe_prepare's work without the caller's
 * round trip between the two calls.  Every such build consumes the arm,
 * whether or not it queued anything (and a failed build queues nothing);
 * n_candidates = 0 disarms.  A tpe_prepare after it is a no-op.  No
 * reference counterpart (tpe.suggest's fresh posterior every step). */
int tpe_arm_prepare(tpe_ctx *ctx, int64_t n_candidates, int32_t n_rounds);

#ifdef __cplusplus
}
#endif

#endif /* HYPEROPT_TPE_H */
