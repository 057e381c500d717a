// tpe_multi.hip -- multi-device contexts: one suggestion engine over several
// GPUs of one node behind the same C ABI (include/hyperopt_tpe.h).
//
// The reference plugs one synchronous `algo(new_ids, domain, trials, seed)`
// call per round into fmin (hyperopt/fmin.py:201-202), so the fan-out over
// GPUs lives inside the call: the primary context (first device) owns one
// peer context per further device, each with its own HIP stream, and
//   * posterior uploads / device builds / history appends / options are
//     forwarded to every device (the builds are deterministic, so every
//     device holds the bit-identical posterior);
//   * a suggestion round is split into contiguous shards -- the candidate
//     range [off, off + n) of every round when there are enough candidates,
//     else whole rounds (batched new_ids) -- one host thread per device runs
//     its shard on its stream, and the per-shard winners are merged with the
//     broadcast_best order (larger score, NaN greatest, lowest global index);
//   * decisions that change a summation order follow the whole problem
//     (tpe_ctx::hint_*), and the quantized labels' grid windows are
//     exchanged between the shards before their tables are built, so every
//     sharding returns the single-device winners bit for bit.
// Candidate indices are global (the Philox counter), so the shards draw
// exactly the single-device candidate set.
//
// Label shards (round 6; the resident-history path -- tpe_history_reset,
// append, the device builds, the index, the rounds -- with at least one
// label per device, TPE_OPT_LABEL_SHARDS on): labels are independent (one
// build_posterior_wrapper + broadcast_best per label, tpe.py:678-692,
// 769-778), so device d holds only its labels (longest processing time
// first: dense 1, quantized 1.5, categorical 0.5 -- parallel.label_shards'
// partition), keeps each label's Philox stream (TPE_HAS_STREAM = its space
// index), and uploads, appends, builds, indexes and runs whole rounds for
// those labels alone; the host scatters each device's winners (48 B per
// label) to their space positions.  The per-posterior work -- history
// append, build, tie orders, expansion index -- then divides over the
// devices with the candidates, where the candidate split repeats it on
// every device.  Spaces with fewer labels than devices, tpe_set_posterior
// and the one-shot tpe_build_posterior keep the candidate / round split.
//
// Joint posteriors (tpe_joint.hip) are replicated on every device of either
// kind of context: tpe_joint_set_group folds the same arrays everywhere, and
// tpe_joint_build_groups builds them from the univariate build -- on a
// label-sharded context in two for_all phases (the owners gather their
// labels' columns; every device copies in the others', device to device,
// interleaves and folds).  The joint rounds split like the univariate ones
// (joint_sharded); tpe_joint_last_shards tells how the last one ran.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <algorithm>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"

namespace {

constexpr int64_t kMinShard = 1024;   // candidates per shard (one tile of the tile map)

int ndev(const tpe_ctx* c) { return 1 + (int)c->peers.size(); }

tpe_ctx* dev(tpe_ctx* c, int d) { return d == 0 ? c : c->peers[d - 1]; }

// One persistent host thread per peer device, created with the first
// fanned-out call and bound to its device once (a call used to spawn and
// join a thread per device): for_all hands every worker the same job and
// waits for the count of pending devices to drop to zero.
struct Workers {
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    const std::function<int(tpe_ctx*, int)>* job = nullptr;
    uint64_t gen = 0;
    int pending = 0;
    bool stop = false;
    std::vector<int> rc;
    std::vector<std::thread> th;

    ~Workers() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_job.notify_all();
        for (auto& t : th) t.join();
    }
};

void worker_main(Workers* w, tpe_ctx* x, int d) {
    const bool bound = hipSetDevice(x->device) == hipSuccess;
    uint64_t seen = 0;
    for (;;) {
        std::unique_lock<std::mutex> lk(w->mu);
        w->cv_job.wait(lk, [&] { return w->stop || w->gen != seen; });
        if (w->stop) return;
        seen = w->gen;
        const auto* job = w->job;
        lk.unlock();
        int r;
        if (bound) {
            r = (*job)(x, d);
        } else {
            x->err = "hipSetDevice failed";
            r = TPE_ERR_HIP;
        }
        lk.lock();
        w->rc[d] = r;
        if (--w->pending == 0) w->cv_done.notify_all();
    }
}

Workers* workers_of(tpe_ctx* c) {
    if (!c->workers) {
        auto w = std::make_shared<Workers>();
        const int n = ndev(c);
        w->rc.assign(n, TPE_OK);
        for (int d = 1; d < n; ++d) w->th.emplace_back(worker_main, w.get(), dev(c, d), d);
        c->workers = std::static_pointer_cast<void>(w);
    }
    return static_cast<Workers*>(c->workers.get());
}

// Run fn(device context, d) on every device concurrently (the primary on
// the calling thread, the peers on their workers); the first failing
// device's code and message become the primary's.
int for_all(tpe_ctx* c, const std::function<int(tpe_ctx*, int)>& fn) {
    const int n = ndev(c);
    if (n == 1) return fn(c, 0);
    Workers* w = workers_of(c);
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->job = &fn;
        w->pending = n - 1;
        for (int d = 0; d < n; ++d) w->rc[d] = TPE_OK;
        ++w->gen;
    }
    w->cv_job.notify_all();
    const int rc0 = fn(c, 0);
    std::vector<int> rc;
    {
        std::unique_lock<std::mutex> lk(w->mu);
        w->cv_done.wait(lk, [&] { return w->pending == 0; });
        rc = w->rc;
    }
    rc[0] = rc0;
    for (int d = 0; d < n; ++d)
        if (rc[d] != TPE_OK) {
            if (d > 0) c->err = "device " + std::to_string(dev(c, d)->device) + ": " + dev(c, d)->err;
            return rc[d];
        }
    return TPE_OK;
}

// The window exchange of one sharded round: every shard posts its per-label
// min/max grid index and waits for the others; a shard that fails before
// posting aborts the exchange so nobody waits forever.
struct WindowExchange final : tpe_rt::QExchange {
    std::mutex mu;
    std::condition_variable cv;
    int expected, arrived = 0;
    bool aborted = false;
    std::vector<unsigned long long> mm;   // combined: min over [0, nq), max over [nq, 2 nq)
    std::vector<char> posted;             // per device: reached the exchange

    explicit WindowExchange(int n) : expected(n), posted(n, 0) {}

    int exchange(tpe_ctx* ctx, std::vector<unsigned long long>& local) override {
        std::unique_lock<std::mutex> lk(mu);
        if (ctx->shard_id >= 0 && ctx->shard_id < expected) posted[ctx->shard_id] = 1;
        const size_t nq = local.size() / 2;
        if (mm.empty()) {
            mm.assign(local.size(), 0ull);
            for (size_t i = 0; i < nq; ++i) mm[i] = ~0ull;
        }
        if (mm.size() != local.size()) {
            aborted = true;
            cv.notify_all();
            return ctx->fail(TPE_ERR_ARG, "multi-device round: shards disagree on the quantized labels");
        }
        for (size_t i = 0; i < nq; ++i) {
            mm[i] = local[i] < mm[i] ? local[i] : mm[i];
            mm[nq + i] = local[nq + i] > mm[nq + i] ? local[nq + i] : mm[nq + i];
        }
        if (++arrived == expected) cv.notify_all();
        cv.wait(lk, [&] { return arrived == expected || aborted || arrived + unposted == expected; });
        if (aborted) return ctx->fail(TPE_ERR_ARG, "multi-device round: another device failed");
        if (arrived != expected)
            return ctx->fail(TPE_ERR_ARG, "multi-device round: shards took different paths");
        local = mm;
        return TPE_OK;
    }

    void abort() {
        std::lock_guard<std::mutex> lk(mu);
        aborted = true;
        cv.notify_all();
    }

    // A shard that finished without posting (its round took a path without
    // quantized tables while another's did -- the shards' paths are meant to
    // be identical) must not leave the others waiting: fail them instead.
    void finished(int d) {
        std::lock_guard<std::mutex> lk(mu);
        if (!posted[d]) {
            ++unposted;
            cv.notify_all();
        }
    }
    int unposted = 0;
};

struct Shard {
    int64_t cand_lo = 0, n_cand = 0;   // candidate range of every round
    int32_t round_lo = 0, n_rounds = 0;
};

// Aggregate the last round's statistics of all devices into the primary
// (RoundStats::merge: work summed, times the slowest device's; the screen
// mode is the primary's own).
void aggregate_stats(tpe_ctx* c) {
    for (int d = 1; d < ndev(c); ++d) c->stats.merge(dev(c, d)->stats);
}

// One sharded round (tpe_suggest / tpe_suggest_batch): shards by candidate
// range when every device gets at least kMinShard candidates of each round,
// else by whole rounds, else the primary runs it alone.
int sharded_round(tpe_ctx* c, uint64_t seed, const uint32_t* rounds, int32_t n_rounds,
                  int64_t n, int64_t cand_offset, tpe_label_result* out) {
    const int nd = ndev(c);
    const int32_t L = c->resident.n_labels;
    const bool by_cand = n >= (int64_t)nd * kMinShard;
    const bool by_round = !by_cand && n_rounds >= nd && n > 0;
    if (nd == 1 || L <= 0 || (!by_cand && !by_round))
        return tpe1_suggest_batch(c, seed, rounds, n_rounds, n, cand_offset, out);
    std::vector<Shard> sh(nd);
    for (int d = 0; d < nd; ++d) {
        if (by_cand) {
            const int64_t q = n / nd, r = n % nd;
            sh[d].n_cand = q + (d < r ? 1 : 0);
            sh[d].cand_lo = d * q + std::min<int64_t>(d, r);
            sh[d].round_lo = 0;
            sh[d].n_rounds = n_rounds;
        } else {
            const int32_t q = n_rounds / nd, r = n_rounds % nd;
            sh[d].n_rounds = q + (d < r ? 1 : 0);
            sh[d].round_lo = d * q + std::min<int32_t>(d, r);
            sh[d].cand_lo = 0;
            sh[d].n_cand = n;
        }
    }
    // per-shard outputs: candidate shards into their own blocks (merged
    // below), round shards straight into their rows of `out`
    std::vector<tpe_label_result> parts(by_cand ? (size_t)nd * n_rounds * L : 0);
    WindowExchange wx(nd);
    int rc = for_all(c, [&](tpe_ctx* x, int d) {
        x->hint_n = n;
        x->hint_rounds = n_rounds;
        x->qx = &wx;
        x->shard_id = d;
        tpe_label_result* o = by_cand ? parts.data() + (size_t)d * n_rounds * L
                                      : out + (size_t)sh[d].round_lo * L;
        // candidate shards merge by score: a value-only cell has none
        const bool vo = x->opt.value_only;
        if (by_cand) x->opt.value_only = false;
        int r = tpe1_suggest_batch(x, seed, rounds + sh[d].round_lo, sh[d].n_rounds, sh[d].n_cand,
                                   cand_offset + sh[d].cand_lo, o);
        x->opt.value_only = vo;
        x->hint_n = 0;
        x->hint_rounds = 0;
        x->qx = nullptr;
        if (r) wx.abort();
        else wx.finished(d);
        return r;
    });
    if (rc) return rc;
    if (by_cand) {
        const int32_t rows = n_rounds * L;
        rc = tpe_merge_results(parts.data(), nd, rows, out);
        if (rc) return c->fail(rc, "merging the shards' winners failed");
    }
    aggregate_stats(c);
    return TPE_OK;
}

// -------------------------------------------------------- label shards ----
bool lsharded(const tpe_ctx* c) { return !c->lsh_ids.empty(); }

double label_cost(const tpe_label_spec& s) {
    if (s.kind == TPE_CATEGORICAL) return 0.5;
    return (s.flags & TPE_HAS_Q) ? 1.5 : 1.0;
}

// the partition: largest cost to the least-loaded device (ties: lower
// device, lower label), each device's labels in increasing order
void lsh_assign(tpe_ctx* c, const tpe_label_spec* specs, int32_t L) {
    const int nd = ndev(c);
    c->lsh_ids.assign(nd, {});
    std::vector<double> load(nd, 0.0);
    std::vector<int32_t> order(L);
    for (int32_t i = 0; i < L; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t a, int32_t b) { return label_cost(specs[a]) > label_cost(specs[b]); });
    for (int32_t i : order) {
        int d = 0;
        for (int k = 1; k < nd; ++k)
            if (load[k] < load[d]) d = k;
        c->lsh_ids[d].push_back(i);
        load[d] += label_cost(specs[i]);
    }
    c->lsh_dev.assign(L, 0);
    c->lsh_local.assign(L, 0);
    for (int d = 0; d < nd; ++d) {
        std::sort(c->lsh_ids[d].begin(), c->lsh_ids[d].end());
        for (size_t j = 0; j < c->lsh_ids[d].size(); ++j) {
            c->lsh_dev[c->lsh_ids[d][j]] = d;
            c->lsh_local[c->lsh_ids[d][j]] = (int32_t)j;
        }
    }
    c->lsh_L = L;
}

void lsh_clear(tpe_ctx* c) {
    c->lsh_ids.clear();
    c->lsh_dev.clear();
    c->lsh_local.clear();
    c->lsh_L = 0;
}

// a device's share of per-label orders (order_off[L + 1] / order over the
// global labels) in its local numbering
void lsh_orders(const std::vector<int32_t>& ids, const int64_t* order_off, const int32_t* order,
                std::vector<int64_t>& off, std::vector<int32_t>& ord) {
    off.assign(ids.size() + 1, 0);
    ord.clear();
    for (size_t j = 0; j < ids.size(); ++j) {
        const int64_t a = order_off[ids[j]], b = order_off[ids[j] + 1];
        ord.insert(ord.end(), order + a, order + b);
        off[j + 1] = (int64_t)ord.size();
    }
}

// a device's tie report (local labels + the split flag) into the global one
void lsh_ties_merge(const std::vector<int32_t>& ids, const std::vector<int32_t>& t, int32_t L, int32_t* ties) {
    for (size_t j = 0; j < ids.size(); ++j) ties[ids[j]] = t[j];
    ties[L] |= t[ids.size()];
}

// one round of every device's labels, scattered into out[round][label]
int lsh_round(tpe_ctx* c, uint64_t seed, const uint32_t* rounds, int32_t n_rounds, int64_t n, int64_t cand_offset,
              tpe_label_result* out) {
    const int nd = ndev(c);
    const int32_t L = c->lsh_L;
    std::vector<std::vector<tpe_label_result>> parts(nd);
    int rc = for_all(c, [&](tpe_ctx* x, int d) {
        const std::vector<int32_t>& ids = c->lsh_ids[d];
        parts[d].resize((size_t)n_rounds * ids.size());
        return tpe1_suggest_batch(x, seed, rounds, n_rounds, n, cand_offset, parts[d].data());
    });
    if (rc) return rc;
    for (int d = 0; d < nd; ++d) {
        const std::vector<int32_t>& ids = c->lsh_ids[d];
        const size_t Ld = ids.size();
        for (int32_t r = 0; r < n_rounds; ++r)
            for (size_t j = 0; j < Ld; ++j) {
                tpe_label_result v = parts[d][(size_t)r * Ld + j];
                v.label = ids[j];
                out[(size_t)r * L + ids[j]] = v;
            }
    }
    aggregate_stats(c);
    return TPE_OK;
}

// ---------------------------------------------------------- joint rounds ----
// One joint call -- rounds[0 .. n_rounds) of n candidates for `ns` slots of
// dimensions D[] -- split like sharded_round: candidate shards from kMinShard
// candidates per device, else whole rounds, else the primary alone.  The
// joint posterior is replicated (tpe_joint_set_group), so every device draws
// and scores its range [lo, lo + m) of the global candidate indices; the
// shards' winners merge with tpe_merge_results, the one broadcast_best order.
// run(x, shard, values, index, ll, lg) is the device's call on its rows.
using JointRun = std::function<int(tpe_ctx*, const Shard&, double*, int64_t*, double*, double*)>;

void joint_timing(tpe_ctx* c) {   // (the slowest device's, as aggregate_stats)
    float score_ms = 0.f, round_ms = 0.f;
    for (int d = 0; d < ndev(c); ++d) {
        score_ms = std::max(score_ms, dev(c, d)->stats.score_ms);
        round_ms = std::max(round_ms, dev(c, d)->stats.round_ms);
    }
    c->stats.score_ms = score_ms;
    c->stats.round_ms = round_ms;
}

int joint_sharded(tpe_ctx* c, int32_t n_rounds, int64_t n, int32_t ns, const int32_t* D, const JointRun& run,
                  double* values, int64_t* index, double* ll, double* lg) {
    const int nd = ndev(c);
    const bool by_cand = n >= (int64_t)nd * kMinShard;
    const bool by_round = !by_cand && n_rounds >= nd && n > 0;
    c->joint_shard_mode = by_cand ? 1 : (by_round ? 2 : 0);
    c->joint_shard_devs = by_cand || by_round ? nd : 1;
    Shard whole;
    whole.n_cand = n;
    whole.n_rounds = n_rounds;
    if (!by_cand && !by_round) return run(c, whole, values, index, ll, lg);
    size_t sumD = 0;
    for (int32_t s = 0; s < ns; ++s) sumD += (size_t)D[s];
    std::vector<Shard> sh(nd);
    for (int d = 0; d < nd; ++d) {
        if (by_cand) {
            const int64_t q = n / nd, r = n % nd;
            sh[d].n_cand = q + (d < r ? 1 : 0);
            sh[d].cand_lo = d * q + std::min<int64_t>(d, r);
            sh[d].round_lo = 0;
            sh[d].n_rounds = n_rounds;
        } else {
            const int32_t q = n_rounds / nd, r = n_rounds % nd;
            sh[d].n_rounds = q + (d < r ? 1 : 0);
            sh[d].round_lo = d * q + std::min<int32_t>(d, r);
            sh[d].cand_lo = 0;
            sh[d].n_cand = n;
        }
    }
    if (by_round) {   // each device writes its own rows: nothing to merge
        const int rc = for_all(c, [&](tpe_ctx* x, int d) {
            const size_t r0 = (size_t)sh[d].round_lo;
            return run(x, sh[d], values + r0 * sumD, index + r0 * ns, ll + r0 * ns, lg + r0 * ns);
        });
        if (rc) return rc;
        joint_timing(c);
        return TPE_OK;
    }
    const size_t cells = (size_t)n_rounds * ns, nv = (size_t)n_rounds * sumD;
    std::vector<double> pv(nd * nv), pl(nd * cells), pg(nd * cells);
    std::vector<int64_t> pi(nd * cells);
    int rc = for_all(c, [&](tpe_ctx* x, int d) {
        return run(x, sh[d], pv.data() + d * nv, pi.data() + d * cells, pl.data() + d * cells, pg.data() + d * cells);
    });
    if (rc) return rc;
    std::vector<tpe_label_result> parts(nd * cells), best(cells);
    for (size_t j = 0; j < nd * cells; ++j) {
        tpe_label_result& p = parts[j];
        p.value = 0.0;
        p.score = pl[j] - pg[j];   // (the round's own key: lpdf_below - lpdf_above)
        p.lpdf_below = pl[j];
        p.lpdf_above = pg[j];
        p.index = pi[j];
        p.label = 0;
        p.status = 0;
    }
    rc = tpe_merge_results(parts.data(), nd, (int32_t)cells, best.data());
    if (rc) return c->fail(rc, "merging the shards' joint winners failed");
    for (int32_t r = 0; r < n_rounds; ++r) {
        size_t doff = 0;
        for (int32_t s = 0; s < ns; ++s) {
            const size_t j = (size_t)r * ns + s;
            int d = 0;   // the shard whose range holds the winner
            while (d + 1 < nd && best[j].index >= sh[d + 1].cand_lo) ++d;
            ll[j] = best[j].lpdf_below;
            lg[j] = best[j].lpdf_above;
            index[j] = best[j].index;
            const double* v = pv.data() + d * nv + (size_t)r * sumD + doff;
            std::copy(v, v + D[s], values + (size_t)r * sumD + doff);
            doff += (size_t)D[s];
        }
    }
    joint_timing(c);
    return TPE_OK;
}

}  // namespace

extern "C" {

int tpe_ctx_create_multi(const int* devices, int32_t n_devices, int precision, tpe_ctx** out) {
    if (!out || !devices || n_devices <= 0) return TPE_ERR_ARG;
    *out = nullptr;
    tpe_ctx* c = nullptr;
    int rc = tpe_ctx_create(devices[0], precision, &c);
    if (rc) return rc;
    for (int32_t d = 1; d < n_devices; ++d) {
        tpe_ctx* p = nullptr;
        rc = tpe_ctx_create(devices[d], precision, &p);
        if (rc) {
            tpe_ctx_destroy(c);
            return rc;
        }
        c->peers.push_back(p);
    }
    *out = c;
    return TPE_OK;
}

int32_t tpe_ctx_devices(const tpe_ctx* ctx, int32_t* devices, int32_t cap) {
    if (!ctx) return 0;
    const int n = 1 + (int)ctx->peers.size();
    for (int d = 0; d < n && d < cap; ++d)
        if (devices) devices[d] = d == 0 ? ctx->device : ctx->peers[d - 1]->device;
    return n;
}

void tpe_ctx_destroy(tpe_ctx* ctx) {
    if (!ctx) return;
    ctx->workers.reset();   // (joins the peer workers before their contexts go)
    for (tpe_ctx* p : ctx->peers) tpe1_ctx_destroy(p);
    ctx->peers.clear();
    tpe1_ctx_destroy(ctx);
}

int tpe_set_posterior(tpe_ctx* ctx, const tpe_label_desc* labels, int32_t n_labels,
                      const double* weights, const double* mus, const double* sigmas,
                      int64_t n_components) {
    if (!ctx) return TPE_ERR_ARG;
    lsh_clear(ctx);   // (uploaded posteriors: replicated, candidate / round split)
    return for_all(ctx, [&](tpe_ctx* x, int) {
        return tpe1_set_posterior(x, labels, n_labels, weights, mus, sigmas, n_components);
    });
}

int tpe_set_option(tpe_ctx* ctx, int32_t option, int64_t value) {
    if (!ctx) return TPE_ERR_ARG;
    if (option == TPE_OPT_LABEL_SHARDS) {   // (the multi-device context's own: from the next history reset)
        ctx->lsh_enable = value != 0;
        return TPE_OK;
    }
    return for_all(ctx, [&](tpe_ctx* x, int) { return tpe1_set_option(x, option, value); });
}

int tpe_prepare(tpe_ctx* ctx, int64_t n_candidates, int32_t n_rounds) {
    if (!ctx) return TPE_ERR_ARG;
    return for_all(ctx, [&](tpe_ctx* x, int) { return tpe1_prepare(x, n_candidates, n_rounds); });
}

int tpe_arm_prepare(tpe_ctx* ctx, int64_t n_candidates, int32_t n_rounds) {
    if (!ctx) return TPE_ERR_ARG;
    return for_all(ctx, [&](tpe_ctx* x, int) { return tpe1_arm_prepare(x, n_candidates, n_rounds); });
}

int tpe_history_reset(tpe_ctx* ctx, const tpe_label_spec* specs, int32_t n_labels,
                      const double* cat_p, int64_t n_cat_p) {
    if (!ctx) return TPE_ERR_ARG;
    const int nd = ndev(ctx);
    if (nd == 1 || !ctx->lsh_enable || !specs || n_labels < nd) {
        lsh_clear(ctx);
        return for_all(ctx, [&](tpe_ctx* x, int) {
            return tpe1_history_reset(x, specs, n_labels, cat_p, n_cat_p);
        });
    }
    lsh_assign(ctx, specs, n_labels);
    const int rc = for_all(ctx, [&](tpe_ctx* x, int d) {
        std::vector<tpe_label_spec> sub;
        for (int32_t g : ctx->lsh_ids[d]) {
            tpe_label_spec sp = specs[g];
            if (!(sp.flags & TPE_HAS_STREAM)) {   // (its stream: its space position)
                sp.flags |= TPE_HAS_STREAM;
                sp.stream = g;
            }
            sub.push_back(sp);
        }
        return tpe1_history_reset(x, sub.data(), (int32_t)sub.size(), cat_p, n_cat_p);
    });
    if (rc) lsh_clear(ctx);
    return rc;
}

int tpe_history_append(tpe_ctx* ctx, const int64_t* n_new, const int32_t* obs_trial,
                       const double* obs_val) {
    if (!ctx) return TPE_ERR_ARG;
    if (!lsharded(ctx))
        return for_all(ctx, [&](tpe_ctx* x, int) {
            return tpe1_history_append(x, n_new, obs_trial, obs_val);
        });
    if (!n_new) return ctx->fail(TPE_ERR_ARG, "tpe_history_append: no counts");
    const int32_t L = ctx->lsh_L;
    std::vector<int64_t> off(L + 1, 0);   // (the new observations: label after label)
    for (int32_t l = 0; l < L; ++l) {
        if (n_new[l] < 0) return ctx->fail(TPE_ERR_ARG, "tpe_history_append: negative count");
        off[l + 1] = off[l] + n_new[l];
    }
    return for_all(ctx, [&](tpe_ctx* x, int d) {
        const std::vector<int32_t>& ids = ctx->lsh_ids[d];
        std::vector<int64_t> nn(ids.size());
        std::vector<int32_t> tr;
        std::vector<double> va;
        for (size_t j = 0; j < ids.size(); ++j) {
            const int64_t a = off[ids[j]], b = off[ids[j] + 1];
            nn[j] = b - a;
            if (b > a) {
                tr.insert(tr.end(), obs_trial + a, obs_trial + b);
                va.insert(va.end(), obs_val + a, obs_val + b);
            }
        }
        return tpe1_history_append(x, nn.data(), tr.data(), va.data());
    });
}

int tpe_build_posterior_resident(tpe_ctx* ctx, const double* losses, int64_t n_trials,
                                 int64_t n_valid, double gamma, double prior_weight, int32_t lf,
                                 int32_t* n_below_out) {
    if (!ctx) return TPE_ERR_ARG;
    return for_all(ctx, [&](tpe_ctx* x, int d) {
        return tpe1_build_posterior_resident(x, losses, n_trials, n_valid, gamma, prior_weight, lf,
                                             d == 0 ? n_below_out : nullptr);
    });
}

int tpe_build_posterior_resident_ordered(tpe_ctx* ctx, const double* losses, int64_t n_trials,
                                         int64_t n_valid, double gamma, double prior_weight, int32_t lf,
                                         const uint8_t* below, const int64_t* order_off, const int32_t* order,
                                         int32_t* n_below_out, int32_t* ties) {
    if (!ctx) return TPE_ERR_ARG;
    if (!lsharded(ctx))
        return for_all(ctx, [&](tpe_ctx* x, int d) {
            return tpe1_build_posterior_resident_ordered(x, losses, n_trials, n_valid, gamma, prior_weight, lf,
                                                         below, order_off, order, d == 0 ? n_below_out : nullptr,
                                                         d == 0 ? ties : nullptr);
        });
    const int nd = ndev(ctx);
    const int32_t L = ctx->lsh_L;
    std::vector<std::vector<int32_t>> td(nd);
    const int rc = for_all(ctx, [&](tpe_ctx* x, int d) {
        const std::vector<int32_t>& ids = ctx->lsh_ids[d];
        std::vector<int64_t> off;
        std::vector<int32_t> ord;
        const bool orders = order_off && order && order_off[L] > 0;
        if (orders) lsh_orders(ids, order_off, order, off, ord);
        td[d].assign(ids.size() + 1, 0);
        return tpe1_build_posterior_resident_ordered(x, losses, n_trials, n_valid, gamma, prior_weight, lf, below,
                                                     orders ? off.data() : nullptr, orders ? ord.data() : nullptr,
                                                     d == 0 ? n_below_out : nullptr, td[d].data());
    });
    if (rc) return rc;
    if (ties) {
        std::fill(ties, ties + L + 1, 0);
        for (int d = 0; d < nd; ++d) lsh_ties_merge(ctx->lsh_ids[d], td[d], L, ties);
    }
    return TPE_OK;
}

int tpe_rebuild_labels(tpe_ctx* ctx, const double* losses, int64_t n_trials, int64_t n_valid, double gamma,
                       double prior_weight, int32_t lf, const int64_t* order_off, const int32_t* order,
                       const int32_t* labels, int32_t n_only, int32_t* n_below_out, int32_t* ties) {
    if (!ctx) return TPE_ERR_ARG;
    if (!lsharded(ctx))
        return for_all(ctx, [&](tpe_ctx* x, int d) {
            return tpe1_rebuild_labels(x, losses, n_trials, n_valid, gamma, prior_weight, lf, order_off, order,
                                       labels, n_only, d == 0 ? n_below_out : nullptr, d == 0 ? ties : nullptr);
        });
    if (!labels || n_only <= 0 || !order_off) return ctx->fail(TPE_ERR_ARG, "tpe_rebuild_labels: no labels");
    const int nd = ndev(ctx);
    const int32_t L = ctx->lsh_L;
    std::vector<std::vector<int32_t>> td(nd);
    std::vector<int32_t> nbd(nd, -1);
    const int rc = for_all(ctx, [&](tpe_ctx* x, int d) {
        const std::vector<int32_t>& ids = ctx->lsh_ids[d];
        td[d].assign(ids.size() + 1, 0);
        std::vector<int32_t> mine;   // (its labels of the subset, local numbers: increasing)
        for (int32_t i = 0; i < n_only; ++i) {
            const int32_t g = labels[i];
            if (g < 0 || g >= L) return x->fail(TPE_ERR_ARG, "tpe_rebuild_labels: label out of range");
            if (ctx->lsh_dev[g] == d) mine.push_back(ctx->lsh_local[g]);
        }
        // (its labels keep their build; their tie flags read 0 from now on,
        // as the labels outside a one-device subset rebuild's do)
        if (mine.empty()) return tpe1_report_skipped(x);
        std::vector<int64_t> off;
        std::vector<int32_t> ord;
        lsh_orders(ids, order_off, order, off, ord);
        return tpe1_rebuild_labels(x, losses, n_trials, n_valid, gamma, prior_weight, lf, off.data(), ord.data(),
                                   mine.data(), (int32_t)mine.size(), &nbd[d], td[d].data());
    });
    if (rc) return rc;
    if (n_below_out) {
        *n_below_out = 0;
        for (int d = 0; d < nd; ++d)
            if (nbd[d] >= 0) {
                *n_below_out = nbd[d];
                break;
            }
    }
    if (ties) {
        std::fill(ties, ties + L + 1, 0);
        for (int d = 0; d < nd; ++d) lsh_ties_merge(ctx->lsh_ids[d], td[d], L, ties);
    }
    return TPE_OK;
}

int tpe_build_report(tpe_ctx* ctx, int32_t* n_below, int32_t* ties) {
    if (!ctx) return TPE_ERR_ARG;
    if (!lsharded(ctx)) return tpe1_build_report(ctx, n_below, ties);
    const int nd = ndev(ctx);
    const int32_t L = ctx->lsh_L;
    std::vector<std::vector<int32_t>> td(nd);
    int32_t nb0 = 0;
    const int rc = for_all(ctx, [&](tpe_ctx* x, int d) {
        td[d].assign(ctx->lsh_ids[d].size() + 1, 0);
        return tpe1_build_report(x, d == 0 ? &nb0 : nullptr, td[d].data());
    });
    if (rc) return rc;
    if (n_below) *n_below = nb0;
    if (ties) {
        std::fill(ties, ties + L + 1, 0);
        for (int d = 0; d < nd; ++d) lsh_ties_merge(ctx->lsh_ids[d], td[d], L, ties);
    }
    return TPE_OK;
}

int tpe_get_mixture(tpe_ctx* ctx, int32_t label, int32_t side, double* weights, double* mus, double* sigmas,
                    int32_t cap, int32_t* n) {
    if (!ctx) return TPE_ERR_ARG;
    if (!lsharded(ctx)) return tpe1_get_mixture(ctx, label, side, weights, mus, sigmas, cap, n);
    if (label < 0 || label >= ctx->lsh_L) return ctx->fail(TPE_ERR_ARG, "tpe_get_mixture: no such built mixture");
    tpe_ctx* x = dev(ctx, ctx->lsh_dev[label]);
    HIPCHK(ctx, hipSetDevice(x->device));
    const int rc = tpe1_get_mixture(x, ctx->lsh_local[label], side, weights, mus, sigmas, cap, n);
    if (rc) ctx->err = x->err;
    return rc;
}

int tpe_history_get(tpe_ctx* ctx, int32_t label, int32_t device, int32_t* trial, double* val, double* key,
                    int32_t* idx, int64_t cap, int64_t* n, int64_t* region_cap, int64_t* region_off) {
    if (!ctx) return TPE_ERR_ARG;
    if (ctx->peers.empty())   // (one device: `device` is not looked at)
        return tpe1_history_get(ctx, label, trial, val, key, idx, cap, n, region_cap, region_off);
    tpe_ctx* x;
    int32_t local = label;
    if (lsharded(ctx)) {   // (the owning device and its local label number, as tpe_get_mixture)
        if (label < 0 || label >= ctx->lsh_L) return ctx->fail(TPE_ERR_ARG, "tpe_history_get: label out of range");
        x = dev(ctx, ctx->lsh_dev[label]);
        local = ctx->lsh_local[label];
    } else {               // (replicated: every device holds every label)
        if (device < 0 || device >= ndev(ctx)) return ctx->fail(TPE_ERR_ARG, "tpe_history_get: no such device");
        x = dev(ctx, device);
    }
    const int rc = tpe1_history_get(x, local, trial, val, key, idx, cap, n, region_cap, region_off);
    if (rc && x != ctx) ctx->err = x->err;
    return rc;
}

int32_t tpe_label_device(const tpe_ctx* ctx, int32_t label) {
    if (!ctx || !lsharded(ctx) || label < 0 || label >= ctx->lsh_L) return -1;
    return ctx->lsh_dev[label];
}

int32_t tpe_resident_labels(const tpe_ctx* ctx) {
    if (!ctx) return 0;
    return lsharded(ctx) ? ctx->lsh_L : tpe1_resident_labels(ctx);
}

int tpe_last_build_ms(const tpe_ctx* ctx, float* ms) {
    if (!ctx || !ms) return TPE_ERR_ARG;
    if (!lsharded(ctx)) return tpe1_last_build_ms(ctx, ms);
    float m = 0.f;
    for (int d = 0; d < ndev(const_cast<tpe_ctx*>(ctx)); ++d) {
        float v = 0.f;
        const int rc = tpe1_last_build_ms(dev(const_cast<tpe_ctx*>(ctx), d), &v);
        if (rc) return rc;
        m = std::max(m, v);
    }
    *ms = m;
    return TPE_OK;
}

int tpe_score(tpe_ctx* ctx, int32_t label, const double* cand, int64_t n, double* lpdf_below, double* lpdf_above,
              tpe_label_result* out) {
    if (!ctx) return TPE_ERR_ARG;
    if (!lsharded(ctx)) return tpe1_score(ctx, label, cand, n, lpdf_below, lpdf_above, out);
    if (label < 0 || label >= ctx->lsh_L) return ctx->fail(TPE_ERR_ARG, "tpe_score: label out of range");
    tpe_ctx* x = dev(ctx, ctx->lsh_dev[label]);
    HIPCHK(ctx, hipSetDevice(x->device));
    const int rc = tpe1_score(x, ctx->lsh_local[label], cand, n, lpdf_below, lpdf_above, out);
    if (rc) ctx->err = x->err;
    if (!rc && out) out->label = label;
    return rc;
}

int tpe_build_posterior(tpe_ctx* ctx, const tpe_label_spec* specs, int32_t n_labels,
                        const double* cat_p, int64_t n_cat_p, const double* losses,
                        int64_t n_trials, const int64_t* obs_off, const int32_t* obs_trial,
                        const double* obs_val, double gamma, double prior_weight, int32_t lf,
                        int32_t* n_below_out) {
    if (!ctx) return TPE_ERR_ARG;
    lsh_clear(ctx);   // (the one-shot build: replicated, candidate / round split)
    return for_all(ctx, [&](tpe_ctx* x, int d) {
        return tpe1_build_posterior(x, specs, n_labels, cat_p, n_cat_p, losses, n_trials, obs_off,
                                    obs_trial, obs_val, gamma, prior_weight, lf,
                                    d == 0 ? n_below_out : nullptr);
    });
}

int tpe_suggest(tpe_ctx* ctx, uint64_t seed, uint32_t round, int64_t n_candidates,
                int64_t cand_offset, tpe_label_result* out) {
    if (!ctx || !out) return TPE_ERR_ARG;
    if (ctx->peers.empty()) return tpe1_suggest(ctx, seed, round, n_candidates, cand_offset, out);
    if (lsharded(ctx)) return lsh_round(ctx, seed, &round, 1, n_candidates, cand_offset, out);
    return sharded_round(ctx, seed, &round, 1, n_candidates, cand_offset, out);
}

int tpe_suggest_batch(tpe_ctx* ctx, uint64_t seed, const uint32_t* rounds, int32_t n_rounds,
                      int64_t n_candidates, int64_t cand_offset, tpe_label_result* out) {
    if (!ctx || !out || !rounds) return TPE_ERR_ARG;
    if (ctx->peers.empty())
        return tpe1_suggest_batch(ctx, seed, rounds, n_rounds, n_candidates, cand_offset, out);
    if (n_rounds <= 0) return ctx->fail(TPE_ERR_ARG, "bad candidate/round count");
    if (lsharded(ctx)) return lsh_round(ctx, seed, rounds, n_rounds, n_candidates, cand_offset, out);
    return sharded_round(ctx, seed, rounds, n_rounds, n_candidates, cand_offset, out);
}

// ---- joint (multivariate) posteriors: replicated on every device, also on a
// label-sharded context (a joint group is a posterior of its own) ----
int tpe_joint_set_group(tpe_ctx* ctx, int32_t slot, uint32_t pick_stream, const tpe_joint_dim* dims,
                        const double* q, const int32_t* upper, const double* cat_p, double prior_weight,
                        int32_t n_dims, int32_t n_below, const double* wb, const double* mub, const double* sigb,
                        int32_t n_above, const double* wa, const double* mua, const double* siga) {
    if (!ctx) return TPE_ERR_ARG;
    return for_all(ctx, [&](tpe_ctx* x, int) {
        return tpe1_joint_set_group(x, slot, pick_stream, dims, q, upper, cat_p, prior_weight, n_dims, n_below, wb,
                                    mub, sigb, n_above, wa, mua, siga);
    });
}

// (every replica holds the source's bits and the weights' tree is fixed: the same destination everywhere)
int tpe_joint_condition_group(tpe_ctx* ctx, int32_t src_slot, int32_t dst_slot, int32_t n_fixed, const int32_t* dims,
                              const double* values) {
    if (!ctx) return TPE_ERR_ARG;
    return for_all(ctx, [&](tpe_ctx* x, int) {
        return tpe1_joint_condition_group(x, src_slot, dst_slot, n_fixed, dims, values);
    });
}

int tpe_joint_clear_groups(tpe_ctx* ctx) {
    if (!ctx) return TPE_ERR_ARG;
    return for_all(ctx, [&](tpe_ctx* x, int) { return tpe1_joint_clear_groups(x); });
}

int tpe_joint_build_groups(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const uint32_t* pick_streams,
                           const int64_t* group_off, const int32_t* labels, const int32_t* streams, const double* q,
                           const int32_t* upper, const double* cat_p, double prior_weight, int32_t* flags) {
    return tpe_joint_build_groups_bw(ctx, n_groups, slots, pick_streams, group_off, labels, streams, q, upper, cat_p,
                                     prior_weight, TPE_JOINT_BW_NEIGHBOUR, flags);
}

int tpe_joint_build_groups_bw(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const uint32_t* pick_streams,
                              const int64_t* group_off, const int32_t* labels, const int32_t* streams,
                              const double* q, const int32_t* upper, const double* cat_p, double prior_weight,
                              int32_t bandwidth, int32_t* flags) {
    if (!ctx) return TPE_ERR_ARG;
    const int nd = ndev(ctx);
    if (nd == 1)
        return tpe1_joint_build_groups(ctx, n_groups, slots, pick_streams, group_off, labels, streams, q, upper, cat_p,
                                       prior_weight, bandwidth, flags);
    if (!lsharded(ctx)) {   // replicated: every device holds the whole univariate build
        std::vector<std::vector<int32_t>> fd(nd, std::vector<int32_t>(std::max(n_groups, 1), 0));
        const int rc = for_all(ctx, [&](tpe_ctx* x, int d) {
            return tpe1_joint_build_groups(x, n_groups, slots, pick_streams, group_off, labels, streams, q, upper,
                                           cat_p, prior_weight, bandwidth, d == 0 ? flags : fd[d].data());
        });
#ifndef NDEBUG
        if (flags && n_groups > 0 && (rc == TPE_OK || rc == TPE_ERR_SAMPLE))
            for (int d = 1; d < nd; ++d)
                for (int32_t g = 0; g < n_groups; ++g)
                    if (fd[d][g] != flags[g]) return ctx->fail(TPE_ERR_ARG, "joint build: devices disagree on flags");
#endif
        return rc;
    }
    int rc = for_all(ctx, [&](tpe_ctx* x, int) { return tpe1_joint_lsh_check(x); });
    if (rc) return rc;
    std::shared_ptr<void> plan;
    if ((rc = tpe1_joint_lsh_plan(ctx, n_groups, slots, pick_streams, group_off, labels, streams, q, upper, cat_p,
                                  prior_weight, bandwidth, flags, &plan)))
        return rc;
    // two phases with the host barrier of for_all between them: every
    // device's columns are complete (its stream synchronised) before another
    // device copies them
    if ((rc = for_all(ctx, [&](tpe_ctx* x, int d) { return tpe1_joint_lsh_gather(x, d, plan.get()); }))) return rc;
    tpe1_joint_lsh_flags(plan.get(), flags);
    return for_all(ctx, [&](tpe_ctx* x, int d) { return tpe1_joint_lsh_fold(x, d, plan.get()); });
}

// (the primary's replica answers these three)
int tpe_joint_get_group(tpe_ctx* ctx, int32_t slot, int32_t side, double* w, double* mu, double* sigma, int32_t cap,
                        int32_t* n_components, int32_t* n_dims) {
    return tpe1_joint_get_group(ctx, slot, side, w, mu, sigma, cap, n_components, n_dims);
}

int tpe_joint_draw_group(tpe_ctx* ctx, int32_t slot, uint64_t seed, uint32_t round, int64_t n, int64_t cand_offset,
                         double* values, int32_t* comp) {
    return tpe1_joint_draw_group(ctx, slot, seed, round, n, cand_offset, values, comp);
}

int tpe_joint_score_group(tpe_ctx* ctx, int32_t slot, const double* values, int64_t n, double* ll, double* lg) {
    return tpe1_joint_score_group(ctx, slot, values, n, ll, lg);
}

int tpe_joint_suggest_group(tpe_ctx* ctx, int32_t slot, uint64_t seed, uint32_t round, int64_t n_candidates,
                            double* values, int64_t* index, double* ll, double* lg) {
    if (!ctx) return TPE_ERR_ARG;
    ctx->joint_shard_mode = 0;
    ctx->joint_shard_devs = 1;
    int32_t D[TPE_JOINT_MAX_GROUPS];
    // (an unset slot, a bad argument: the primary's own refusal)
    if (ctx->peers.empty() || !values || !index || !ll || !lg || slot < 0 ||
        tpe1_joint_set_slots(ctx, slot, D) != 1)
        return tpe1_joint_suggest_group(ctx, slot, seed, round, n_candidates, 0, values, index, ll, lg);
    return joint_sharded(
        ctx, 1, n_candidates, 1, D,
        [&](tpe_ctx* x, const Shard& s, double* v, int64_t* i, double* l, double* g) {
            return tpe1_joint_suggest_group(x, slot, seed, round, s.n_cand, s.cand_lo, v, i, l, g);
        },
        values, index, ll, lg);
}

int tpe_joint_suggest_batch(tpe_ctx* ctx, uint64_t seed, const uint32_t* rounds, int32_t n_rounds,
                            int64_t n_candidates, double* values, int64_t* index, double* ll, double* lg) {
    if (!ctx) return TPE_ERR_ARG;
    ctx->joint_shard_mode = 0;
    ctx->joint_shard_devs = 1;
    int32_t D[TPE_JOINT_MAX_GROUPS];
    int32_t ns = 0;
    if (ctx->peers.empty() || !rounds || !values || !index || !ll || !lg || n_rounds < 1 ||
        (ns = tpe1_joint_set_slots(ctx, -1, D)) < 1)
        return tpe1_joint_suggest_batch(ctx, seed, rounds, n_rounds, n_candidates, 0, values, index, ll, lg);
    return joint_sharded(
        ctx, n_rounds, n_candidates, ns, D,
        [&](tpe_ctx* x, const Shard& s, double* v, int64_t* i, double* l, double* g) {
            return tpe1_joint_suggest_batch(x, seed, rounds + s.round_lo, s.n_rounds, s.n_cand, s.cand_lo, v, i, l, g);
        },
        values, index, ll, lg);
}

// the candidate pool lives on one device: a multi-device context refuses it
int tpe_pool_set(tpe_ctx* ctx, const double* values, int64_t n, int32_t n_cols) {
    if (!ctx) return TPE_ERR_ARG;
    if (!ctx->peers.empty()) return ctx->fail(TPE_ERR_ARG, "tpe_pool_set: not available on a multi-device context");
    return tpe1_pool_set(ctx, values, n, n_cols);
}

int tpe_pool_clear(tpe_ctx* ctx) { return tpe1_pool_clear(ctx); }

int tpe_pool_size(const tpe_ctx* ctx, int64_t* n, int32_t* n_cols) { return tpe1_pool_size(ctx, n, n_cols); }

int tpe_pool_rank(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const int64_t* group_off,
                  const int32_t* group_cols, const int64_t* taken, int64_t n_taken, int32_t top_k, int64_t* top_index,
                  double* top_score, int32_t* n_top, double* score, double* lpdf_below, double* lpdf_above) {
    if (!ctx) return TPE_ERR_ARG;
    if (!ctx->peers.empty()) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: not available on a multi-device context");
    return tpe1_pool_rank(ctx, n_groups, slots, group_off, group_cols, taken, n_taken, top_k, top_index, top_score,
                          n_top, score, lpdf_below, lpdf_above);
}

int tpe_pool_draw(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const int64_t* group_off,
                  const int32_t* group_cols, const int64_t* taken, int64_t n_taken, uint64_t seed,
                  const uint32_t* rounds, int32_t n_rounds, int64_t m, int32_t distinct, int64_t* best_index,
                  double* best_score, int32_t* n_best, int64_t* drawn, int32_t* n_drawn, double* lsum, double* keys,
                  double* score) {
    if (!ctx) return TPE_ERR_ARG;
    if (!ctx->peers.empty()) return ctx->fail(TPE_ERR_ARG, "tpe_pool_draw: not available on a multi-device context");
    return tpe1_pool_draw(ctx, n_groups, slots, group_off, group_cols, taken, n_taken, seed, rounds, n_rounds, m,
                          distinct, best_index, best_score, n_best, drawn, n_drawn, lsum, keys, score);
}

int tpe_joint_last_shards(const tpe_ctx* ctx, int32_t* mode, int32_t* n_devices) {
    if (!ctx) return TPE_ERR_ARG;
    if (mode) *mode = ctx->joint_shard_mode;
    if (n_devices) *n_devices = ctx->joint_shard_devs;
    return TPE_OK;
}

}  // extern "C"
