// smx_calls.cpp -- the one-shot calls of libsmx.so over host buffers: alignments (smx_align, smx_align_batch), specimine
// (smx_mine.hip), clusters (smx_pairs.hip), consensus (smx_cons.hip), crosstalk (smx_nearest.hip), identify (smx_hits.hip), bimera (smx_reach.hip) and the inner scan (smx_inner.hip).  Each keeps one grow-only device workspace; its calls are serialised.
#include "smx_host.h"
#include "smx_align_lane.h"   // align_collect
#include "smx_cons_plan.h"
#include "smx_nearest_plan.h"
#include "smx_hits_plan.h"
#include "smx_reach_plan.h"
#include "smx_mine_plan.h"
#include "smx_pairs_plan.h"
#include "smx_inner_plan.h"

int smx_align(const char *query, int qlen, const char *target, int tlen, int k, int mode, int *dist, int *starts,
              int *ends, int cap, int *nloc) {
    if (!query || !target || !dist || !nloc) return fail(SMX_ERR_ARG, "null argument");
    if (qlen < 1 || qlen > 64) return fail(SMX_ERR_UNSUPPORTED, "query length %d outside 1..64", qlen);
    if (mode != 0 && mode != 1) return fail(SMX_ERR_UNSUPPORTED, "mode %d (0 = HW, 1 = SHW)", mode);
    if (tlen < 1) return fail(SMX_ERR_UNSUPPORTED, "empty target");
    unsigned long long peq[32];
    std::string bad, q(query, qlen), rq(q.rbegin(), q.rend());
    if (!build_peq(q.data(), qlen, peq, &bad) || !build_peq(rq.data(), qlen, peq + 16, &bad))
        return fail(SMX_ERR_UNSUPPORTED, "%s", bad.c_str());
    SMX_TRY(require_device());   // every argument check is above: a bad call is refused without a device
    std::vector<unsigned char> codes(tlen);
    for (int i = 0; i < tlen; i++) codes[i] = (unsigned char)code_of((unsigned char)target[i]);
    DevMem<unsigned char> d;
    size_t o_codes = 256, o_flag = o_codes + ((tlen + 15) & ~15), o_starts = o_flag + ((tlen + 15) & ~15),
           o_dist = o_starts + (size_t)tlen * 4, total = o_dist + 16;
    HIP_TRY(d.alloc(total));
    hipError_t e = hipMemcpy(d, peq, 256, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_codes, codes.data(), tlen, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = (hipError_t)smx_launch_align(nullptr, (unsigned long long *)d.p, (unsigned long long *)d.p + 16, qlen, d + o_codes,
                                         tlen, k, mode, (int *)(d + o_dist), d + o_flag, (int *)(d + o_starts));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<unsigned char> flag(tlen);
    std::vector<int> st(tlen);
    if (e == hipSuccess) e = hipMemcpy(dist, d + o_dist, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(flag.data(), d + o_flag, tlen, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(st.data(), d + o_starts, (size_t)tlen * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SMX_ERR_DEVICE, "smx_align: %s", hipGetErrorString(e));
    *nloc = smx::align_collect(*dist, flag.data(), st.data(), tlen, starts, ends, cap);
    return SMX_OK;
}

// ---- batched alignments: grow-only device workspace shared by all calls (serialised)
static struct {
    std::mutex mutex;
    DevBuf qpeq, qlen, qidx, codes, toff, k, mode;    // what the call uploads
    DevBuf scores, dist, nloc, starts, ends;    // the raw score of every target column, and what comes back
} g_align;

int smx_align_batch(const char *queries, const uint32_t *qoff, uint32_t n_queries, const char *targets, const uint64_t *toff,
                    const uint32_t *qidx, const int32_t *k, const uint8_t *mode, uint32_t n, int32_t *dist, int32_t *nloc,
                    int32_t *starts, int32_t *ends, uint32_t cap) {
    if (!queries || !qoff || !targets || !toff || !qidx || !k || !mode || !dist || !nloc || (cap && (!starts || !ends)))
        return fail(SMX_ERR_ARG, "null argument");
    if (n == 0) return SMX_OK;
    std::vector<unsigned long long> qpeq((size_t)n_queries * 32);
    std::vector<int> qlen(n_queries);
    std::string bad;
    for (uint32_t q = 0; q < n_queries; q++) {
        const int m = (int)(qoff[q + 1] - qoff[q]);
        if (m < 1 || m > 64) return fail(SMX_ERR_UNSUPPORTED, "query %u: length %d outside 1..64", q, m);
        std::string s(queries + qoff[q], m), r(s.rbegin(), s.rend());
        if (!build_peq(s.data(), m, &qpeq[(size_t)q * 32], &bad) || !build_peq(r.data(), m, &qpeq[(size_t)q * 32 + 16], &bad))
            return fail(SMX_ERR_UNSUPPORTED, "query %u: %s", q, bad.c_str());
        qlen[q] = m;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (toff[i + 1] <= toff[i]) return fail(SMX_ERR_UNSUPPORTED, "alignment %u: empty target", i);
        if (qidx[i] >= n_queries || mode[i] > 1) return fail(SMX_ERR_ARG, "alignment %u: bad query index or mode", i);
        if (k[i] < 0 || k[i] > 250) return fail(SMX_ERR_ARG, "alignment %u: bad max distance", i);
    }
    SMX_TRY(require_device());   // every argument check is above: a bad call is refused without a device
    const uint64_t tbytes = toff[n];
    std::vector<unsigned char> codes(tbytes);
    for (uint64_t j = 0; j < tbytes; j++) codes[j] = (unsigned char)code_of((unsigned char)targets[j]);
    std::lock_guard<std::mutex> guard(g_align.mutex);
    auto &W = g_align;
    const size_t nbytes = (size_t)n * 4, loc_bytes = (size_t)n * cap * 4;
    HIP_TRY(W.qpeq.upload(qpeq));
    HIP_TRY(W.qlen.upload(qlen));
    HIP_TRY(W.qidx.upload(qidx, nbytes));
    HIP_TRY(W.codes.upload(codes));
    HIP_TRY(W.toff.upload(toff, ((size_t)n + 1) * 8));
    HIP_TRY(W.k.upload(k, nbytes));
    HIP_TRY(W.mode.upload(mode, n));
    HIP_TRY(W.scores.ensure((size_t)tbytes));
    for (DevBuf *b : {&W.dist, &W.nloc}) HIP_TRY(b->ensure(nbytes));
    for (DevBuf *b : {&W.starts, &W.ends}) HIP_TRY(b->ensure(loc_bytes));
    int e = smx_launch_align_batch(nullptr, W.qpeq.as<unsigned long long>(), W.qlen.as<int>(), W.qidx.as<unsigned>(),
                                   W.codes.as<unsigned char>(), W.toff.as<unsigned long long>(), W.k.as<int>(),
                                   W.mode.as<unsigned char>(), n, W.scores.as<unsigned char>(), W.dist.as<int>(),
                                   W.nloc.as<int>(), W.starts.as<int>(), W.ends.as<int>(), cap);
    if (e != 0) return fail(SMX_ERR_DEVICE, "alignment kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dist, W.dist.p, nbytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nloc, W.nloc.p, nbytes, hipMemcpyDeviceToHost));
    if (cap) {
        HIP_TRY(hipMemcpy(starts, W.starts.p, loc_bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ends, W.ends.p, loc_bytes, hipMemcpyDeviceToHost));
    }
    return SMX_OK;
}

// ---- specimine: batched long-read HW distances (smx_mine.hip); grow-only device workspace, calls serialised
namespace {
struct {
    std::mutex mutex;
    DevBuf queries, qoff, targets, tdoff, tlen, pairs, chunk_start;
    DevBuf scratch;     // per-lane state of the generic class, one slice per workgroup
    DevBuf jobs_out;    // the jobs, then the output
} g_mine;

// the padded copy of the targets (smx_chunk_plan.h), failing the call's way
int mine_targets(const char *targets, const uint64_t *toff, uint32_t n_targets, std::vector<uint64_t> *tdoff,
                 std::vector<int32_t> *tlen, std::vector<unsigned char> *tpad) {
    std::string why;
    const int rc = smx::mine_targets(targets, toff, n_targets, tdoff, tlen, tpad, &why);
    return rc == SMX_OK ? SMX_OK : fail(rc, "%s", why.c_str());
}

// One smx_mine_* call.  distances: job j's nq x nt distances at out[sum over earlier jobs of nq * nt] (int32); else
// the best identities at out[sum over earlier jobs of nt] (double).  Device and host memory hold the queries, the
// targets, sum(nq) (job, query) pairs and the output: only the distance output grows with sum(nq * nt).
int mine_call(bool distances, const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k,
              const char *targets, const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs, uint32_t n_jobs,
              void *out, float *kernel_ms) {
    if (!out && n_jobs) return fail(SMX_ERR_ARG, "null argument");
    if (!queries || !qoff || !k || !targets || !toff || (n_jobs && !jobs)) return fail(SMX_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> guard(g_mine.mutex);
    SMX_TRY(require_device());
    // the checks, the padded targets, the jobs, the (job, query) records by class and the grids: smx_mine_plan.h
    smx::MinePlan P;
    std::string why;
    const int rc = smx::mine_plan(queries, qoff, n_queries, k, targets, toff, n_targets, jobs, n_jobs, smx::CHUNK_SCRATCH_BYTES,
                                  &P, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    const uint64_t n_out = distances ? P.n_dist : P.n_best;
    if (n_out == 0) {
        if (kernel_ms) *kernel_ms = 0.0f;
        return SMX_OK;
    }
    const size_t out_bytes = n_out * (distances ? sizeof(int32_t) : sizeof(double));
    auto &W = g_mine;
    const size_t jobs_bytes = n_jobs * sizeof(smx::MineJobDev);
    HIP_TRY(W.queries.upload(queries, (size_t)qoff[n_queries]));
    HIP_TRY(W.qoff.upload(qoff, ((size_t)n_queries + 1) * 8));
    HIP_TRY(W.targets.upload(P.tpad));
    HIP_TRY(W.tdoff.upload(P.tdoff));
    HIP_TRY(W.tlen.upload(P.tlen));
    HIP_TRY(W.pairs.upload(P.pairs));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    if (P.n_pairs[0]) HIP_TRY(W.scratch.ensure((size_t)P.scratch_words * 8));
    HIP_TRY(W.jobs_out.upload(P.jobs.data(), jobs_bytes, out_bytes));
    void *d_out = W.jobs_out.as<char>() + jobs_bytes;
    if (!distances) HIP_TRY(hipMemset(d_out, 0, out_bytes));       // +0.0: "no pair counts"
    KernelTimer timer;
    if (kernel_ms) HIP_TRY(timer.start());
    const int e = smx::chunk_for_each_class(P.n_pairs, [&](int c, int wr, uint32_t n, size_t pat, size_t cat) {
        return smx_launch_mine(nullptr, wr, distances, W.queries.as<unsigned char>(), W.qoff.as<uint64_t>(),
                               W.targets.as<unsigned char>(), W.tdoff.as<uint64_t>(), W.tlen.as<int32_t>(),
                               W.pairs.as<smx::MinePair>() + pat, W.chunk_start.as<uint64_t>() + cat, n, W.jobs_out.p,
                               (int)P.grid[c], P.per_block[c], P.lds_max[c], d_out, W.scratch.as<unsigned long long>(),
                               P.words_max0);
    });
    if (e != 0) return fail(SMX_ERR_DEVICE, "mining kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (kernel_ms) HIP_TRY(timer.stop(kernel_ms));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}
}  // namespace

int smx_mine_distances(const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k, const char *targets,
                       const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs, uint32_t n_jobs, int32_t *dist,
                       float *kernel_ms) {
    return mine_call(true, queries, qoff, n_queries, k, targets, toff, n_targets, jobs, n_jobs, dist, kernel_ms);
}

int smx_mine_best_identity(const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k,
                           const char *targets, const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs,
                           uint32_t n_jobs, double *best, float *kernel_ms) {
    return mine_call(false, queries, qoff, n_queries, k, targets, toff, n_targets, jobs, n_jobs, best, kernel_ms);
}

// ---- clusters: all-pairs NW distances within each job's reads (smx_pairs.hip); the workspace is specimine's own
// shape (padded reads, row list, chunk prefix, scratch, jobs + output), kept apart so that the two never wait for each other
namespace {
struct {
    std::mutex mutex;
    DevBuf reads, doff, len, k, rows, chunk_start;
    DevBuf scratch;     // per-lane state of the generic class, one slice per workgroup
    DevBuf jobs_out;    // the jobs, then the output
} g_pairs;

// One smx_pairs_* call.  distances: job j's n (n - 1) / 2 distances (int32); else its n x ceil(n / 32) adjacency words,
// the upper triangle from the kernel, mirrored here.  Either way job j's output follows the earlier jobs'.
int pairs_call(bool distances, const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
               const smx_pairs_job *jobs, uint32_t n_jobs, uint32_t *out, float *kernel_ms) {
    if (!reads || !roff || !k || (n_jobs && (!jobs || !out))) return fail(SMX_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> guard(g_pairs.mutex);
    SMX_TRY(require_device());
    // the checks, the padded reads, the jobs, the rows by class and the grids: smx_pairs_plan.h
    smx::PairsPlan P;
    std::string why;
    const int rc = smx::pairs_plan(distances, reads, roff, n_reads, jobs, n_jobs, smx::CHUNK_SCRATCH_BYTES, &P, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    if (kernel_ms) *kernel_ms = 0.0f;
    if (P.n_out == 0) return SMX_OK;
    const size_t out_bytes = P.n_out * 4;
    if (P.rows.empty()) {                         // only jobs of one read: a zero word each
        memset(out, 0, out_bytes);
        return SMX_OK;
    }
    auto &W = g_pairs;
    const size_t jobs_bytes = (n_jobs * sizeof(smx::PairsJobDev) + 15) & ~(size_t)15;
    HIP_TRY(W.reads.upload(P.pad));
    HIP_TRY(W.doff.upload(P.doff));
    HIP_TRY(W.len.upload(P.len));
    HIP_TRY(W.k.upload(k, (size_t)n_reads * 4));
    HIP_TRY(W.rows.upload(P.rows));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    if (P.n_rows[0]) HIP_TRY(W.scratch.ensure((size_t)P.scratch_words * 8));
    HIP_TRY(W.jobs_out.upload(P.jobs.data(), n_jobs * sizeof(smx::PairsJobDev), jobs_bytes - n_jobs * sizeof(smx::PairsJobDev) + out_bytes));
    void *d_out = W.jobs_out.as<char>() + jobs_bytes;
    if (!distances) HIP_TRY(hipMemset(d_out, 0, out_bytes));
    KernelTimer timer;
    if (kernel_ms) HIP_TRY(timer.start());
    const int e = smx::chunk_for_each_class(P.n_rows, [&](int c, int wr, uint32_t n, size_t rat, size_t cat) {
        return smx_launch_pairs(nullptr, wr, distances, W.reads.as<unsigned char>(), W.doff.as<uint64_t>(),
                                W.len.as<int32_t>(), W.k.as<int32_t>(), W.rows.as<smx::PairsRow>() + rat,
                                W.chunk_start.as<uint64_t>() + cat, n, W.jobs_out.p, (int)P.grid[c], P.per_block[c],
                                P.lds_max[c], d_out, W.scratch.as<unsigned long long>(), P.words_max0);
    });
    if (e != 0) return fail(SMX_ERR_DEVICE, "pairs kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (kernel_ms) HIP_TRY(timer.stop(kernel_ms));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    if (!distances) smx::pairs_mirror(P, out);    // bit i of row j for every bit j > i of row i
    return SMX_OK;
}
}  // namespace

int smx_pairs_distances(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                        const smx_pairs_job *jobs, uint32_t n_jobs, int32_t *dist, float *kernel_ms) {
    return pairs_call(true, reads, roff, n_reads, k, jobs, n_jobs, reinterpret_cast<uint32_t *>(dist), kernel_ms);
}

int smx_pairs_neighbours(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                         const smx_pairs_job *jobs, uint32_t n_jobs, uint32_t *adj, float *kernel_ms) {
    return pairs_call(false, reads, roff, n_reads, k, jobs, n_jobs, adj, kernel_ms);
}

// ---- crosstalk: every read of a job against every ref of the job, reduced to the nearest own and the nearest other
// ref (smx_nearest.hip); a workspace of its own, like g_pairs
namespace {
struct {
    std::mutex mutex;
    DevBuf seqs, doff, len, k, group, refs, runs, chunk_start, jobs;
    DevBuf scratch;     // per-lane state of the generic class, one slice per workgroup
    DevBuf out;         // best_own then best_other, or the distances
} g_nearest;

// One smx_nearest* call.  distances: dist receives job after job its nq x nt distances; else own / other receive
// sum(nt) keys each.
int nearest_call(bool distances, const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k,
                 const uint32_t *group, const smx_nearest_job *jobs, uint32_t n_jobs, uint64_t *own, uint64_t *other,
                 int32_t *dist, float *kernel_ms) {
    if (!seqs || !off || !k || !group || (n_jobs && (!jobs || (distances ? !dist : !own || !other))))
        return fail(SMX_ERR_ARG, "null argument");
    // every check of the arguments comes before the device is touched
    smx::NearestPlan P;
    std::string why;
    const int rc = smx::nearest_plan(seqs, off, n_seqs, jobs, n_jobs, &P, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    std::lock_guard<std::mutex> guard(g_nearest.mutex);
    SMX_TRY(require_device());
    // G: the chunks a call should keep the device busy with, 32 per CU, or the test hook's figure
    uint64_t min_chunks = 0;
    if (const char *env = getenv("SMX_NEAREST_MIN_CHUNKS")) {
        min_chunks = strtoull(env, nullptr, 10);
    } else {
        int dev = 0, n_cu = 0;
        HIP_TRY(hipGetDevice(&dev));
        HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        min_chunks = smx::NEAREST_CHUNKS_PER_CU * (uint64_t)std::max(n_cu, 1);
    }
    smx::nearest_plan_runs(&P, min_chunks);
    if (kernel_ms) *kernel_ms = 0.0f;
    if ((distances ? P.n_dist : P.n_best) == 0) return SMX_OK;
    const size_t out_bytes = distances ? (size_t)P.n_dist * 4 : (size_t)P.n_best * 16;
    if (P.runs.empty()) {                         // reads, but no job has a ref: no key, no distance
        if (!distances) { memset(own, 0xff, (size_t)P.n_best * 8); memset(other, 0xff, (size_t)P.n_best * 8); }
        return SMX_OK;
    }
    std::vector<uint64_t> doff;
    std::vector<int32_t> len;
    std::vector<unsigned char> pad;
    SMX_TRY(mine_targets(seqs, off, n_seqs, &doff, &len, &pad));
    auto &W = g_nearest;
    HIP_TRY(W.seqs.upload(pad));
    HIP_TRY(W.doff.upload(doff));
    HIP_TRY(W.len.upload(len));
    HIP_TRY(W.k.upload(k, (size_t)n_seqs * 4));
    HIP_TRY(W.group.upload(group, (size_t)n_seqs * 4));
    HIP_TRY(W.refs.upload(P.refs));
    HIP_TRY(W.runs.upload(P.runs));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    HIP_TRY(W.jobs.upload(P.jobs));
    if (P.n_runs[0]) HIP_TRY(W.scratch.ensure((size_t)P.scratch_words * 8));
    HIP_TRY(W.out.ensure(out_bytes));
    // nearest: "no ref" until a lane says otherwise.  distances: every pair is written (nt > 0 and nq > 0 make runs)
    if (!distances) HIP_TRY(hipMemset(W.out.p, 0xff, out_bytes));
    unsigned long long *d_own = W.out.as<unsigned long long>(), *d_other = d_own + (distances ? 0 : P.n_best);
    KernelTimer timer;
    if (kernel_ms) HIP_TRY(timer.start());
    size_t ref_at[6] = {0, 0, 0, 0, 0, 0};             // every class's own ref list, one after the other
    for (int c = 1; c < 6; c++) ref_at[c] = ref_at[c - 1] + P.n_refs[c - 1];
    const int e = smx::chunk_for_each_class(P.n_runs, [&](int c, int wr, uint32_t n, size_t rat, size_t cat) {
        return smx_launch_nearest(nullptr, wr, distances, W.seqs.as<unsigned char>(), W.doff.as<uint64_t>(),
                                  W.len.as<int32_t>(), W.k.as<int32_t>(), W.group.as<uint32_t>(), W.refs.as<uint32_t>() + ref_at[c],
                                  W.runs.as<smx::NearestRun>() + rat, W.chunk_start.as<uint64_t>() + cat, n, W.jobs.p,
                                  (int)P.grid[c], P.per_block[c], P.lds_max[c], d_own, d_other, W.out.as<int32_t>(),
                                  W.scratch.as<unsigned long long>(), P.words_max0);
    });
    if (e != 0) return fail(SMX_ERR_DEVICE, "nearest kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (kernel_ms) HIP_TRY(timer.stop(kernel_ms));
    HIP_TRY(hipDeviceSynchronize());
    if (distances) {
        HIP_TRY(hipMemcpy(dist, W.out.p, out_bytes, hipMemcpyDeviceToHost));
    } else {
        HIP_TRY(hipMemcpy(own, d_own, (size_t)P.n_best * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(other, d_other, (size_t)P.n_best * 8, hipMemcpyDeviceToHost));
    }
    return SMX_OK;
}
}  // namespace

int smx_nearest(const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k, const uint32_t *group,
                const smx_nearest_job *jobs, uint32_t n_jobs, uint64_t *best_own, uint64_t *best_other, float *kernel_ms) {
    return nearest_call(false, seqs, off, n_seqs, k, group, jobs, n_jobs, best_own, best_other, nullptr, kernel_ms);
}

int smx_nearest_distances(const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k, const uint32_t *group,
                          const smx_nearest_job *jobs, uint32_t n_jobs, int32_t *dist, float *kernel_ms) {
    return nearest_call(true, seqs, off, n_seqs, k, group, jobs, n_jobs, nullptr, nullptr, dist, kernel_ms);
}

// ---- identify: every query of a job against every target of the job, the shorter of a pair as the pattern, reduced to
// the K best targets per query (smx_hits.hip); a workspace of its own, like g_nearest
namespace {
struct {
    std::mutex mutex;
    DevBuf seqs, doff, len, k, ord, recs, chunk_start, jobs;
    DevBuf scratch;     // per-lane state of the generic class, one slice per workgroup
    DevBuf out;         // the keys, or the distances
} g_hits;

// One smx_best_hits* call.  distances: dist receives job after job its nq x nt distances; else keys receives sum(nq) x K keys.
int hits_call(bool distances, const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k,
              const smx_hits_job *jobs, uint32_t n_jobs, uint32_t K, uint32_t min_cov_permille, uint64_t *keys, int32_t *dist,
              float *kernel_ms) {
    if (!seqs || !off || !k || (n_jobs && (!jobs || (distances ? !dist : !keys)))) return fail(SMX_ERR_ARG, "null argument");
    // every check of the arguments comes before the device is touched
    smx::HitsPlan P;
    std::string why;
    const int rc = smx::hits_plan(seqs, off, n_seqs, jobs, n_jobs, K, min_cov_permille, &P, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    std::lock_guard<std::mutex> guard(g_hits.mutex);
    SMX_TRY(require_device());
    if (kernel_ms) *kernel_ms = 0.0f;
    const uint64_t n_out = distances ? P.n_dist : P.n_rows * K;
    if (n_out == 0) return SMX_OK;
    const size_t out_bytes = (size_t)n_out * (distances ? 4 : 8);
    // "empty slot" / "no hit" until a lane says otherwise: all-ones is UINT64_MAX as a key and -1 as a distance
    if (P.recs.empty()) {
        memset(distances ? (void *)dist : (void *)keys, 0xff, out_bytes);
        return SMX_OK;
    }
    std::vector<uint64_t> doff;
    std::vector<int32_t> len;
    std::vector<unsigned char> pad;
    SMX_TRY(mine_targets(seqs, off, n_seqs, &doff, &len, &pad));
    auto &W = g_hits;
    HIP_TRY(W.seqs.upload(pad));
    HIP_TRY(W.doff.upload(doff));
    HIP_TRY(W.len.upload(len));
    HIP_TRY(W.k.upload(k, (size_t)n_seqs * 4));
    HIP_TRY(W.ord.upload(P.ord));
    HIP_TRY(W.recs.upload(P.recs));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    HIP_TRY(W.jobs.upload(P.jobs));
    if (P.n_recs[0]) HIP_TRY(W.scratch.ensure((size_t)P.scratch_words * 8));
    HIP_TRY(W.out.ensure(out_bytes));
    HIP_TRY(hipMemset(W.out.p, 0xff, out_bytes));
    KernelTimer timer;
    if (kernel_ms) HIP_TRY(timer.start());
    const int e = smx::chunk_for_each_class(P.n_recs, [&](int c, int wr, uint32_t n, size_t rat, size_t cat) {
        return smx_launch_hits(nullptr, wr, distances, W.seqs.as<unsigned char>(), W.doff.as<uint64_t>(),
                               W.len.as<int32_t>(), W.k.as<int32_t>(), W.ord.as<uint32_t>(), W.recs.as<smx::HitsRec>() + rat,
                               W.chunk_start.as<uint64_t>() + cat, n, W.jobs.p, (int)P.grid[c], P.per_block[c], P.lds_max[c],
                               (int)K, W.out.as<unsigned long long>(), W.out.as<int32_t>(), W.scratch.as<unsigned long long>(),
                               P.words_max0);
    });
    if (e != 0) return fail(SMX_ERR_DEVICE, "hits kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (kernel_ms) HIP_TRY(timer.stop(kernel_ms));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(distances ? (void *)dist : (void *)keys, W.out.p, out_bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}
}  // namespace

int smx_best_hits(const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k, const smx_hits_job *jobs,
                  uint32_t n_jobs, uint32_t K, uint32_t min_cov_permille, uint64_t *keys, float *kernel_ms) {
    return hits_call(false, seqs, off, n_seqs, k, jobs, n_jobs, K, min_cov_permille, keys, nullptr, kernel_ms);
}

int smx_best_hits_distances(const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k,
                            const smx_hits_job *jobs, uint32_t n_jobs, uint32_t K, uint32_t min_cov_permille, int32_t *dist,
                            float *kernel_ms) {
    return hits_call(true, seqs, off, n_seqs, k, jobs, n_jobs, K, min_cov_permille, nullptr, dist, kernel_ms);
}

// ---- bimera: every query of a job against every eligible target of the job by furthest-reaching diagonals, both
// sides, reduced to the two furthest-reaching targets per (query, side, e) (smx_reach.hip); a workspace of its own
namespace {
struct {
    std::mutex mutex;
    DevBuf seqs, doff, len, weight, need, recs, chunk_start, jobs;
    DevBuf out;         // the keys, or the matrix
} g_reach;

// One smx_prefix_reach* call.  matrix: reach receives job after job its nq x nt x 2 x (E + 1) values; else keys receives
// sum(nq) x 2 x (E + 1) x 2 keys.
int reach_call(bool matrix, const char *seqs, const uint64_t *off, uint32_t n_seqs, const uint32_t *weight,
               const uint32_t *need, const smx_reach_job *jobs, uint32_t n_jobs, uint32_t E, uint64_t *keys, uint32_t *reach,
               float *kernel_ms) {
    if (!seqs || !off || !weight || !need || (n_jobs && (!jobs || (matrix ? !reach : !keys)))) return fail(SMX_ERR_ARG, "null argument");
    // every check of the arguments comes before the device is touched
    smx::ReachPlan P;
    std::string why;
    int rc = smx::reach_plan(off, n_seqs, jobs, n_jobs, E, &P, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    std::lock_guard<std::mutex> guard(g_reach.mutex);
    SMX_TRY(require_device());
    if (kernel_ms) *kernel_ms = 0.0f;
    const uint64_t n_out = matrix ? P.n_values : P.n_keys;
    if (n_out == 0) return SMX_OK;
    const size_t out_bytes = (size_t)n_out * (matrix ? 4 : 8);
    // "empty slot" / "not eligible" until a lane says otherwise: all-ones is UINT64_MAX as a key and UINT32_MAX as a value
    if (P.recs.empty()) {
        memset(matrix ? (void *)reach : (void *)keys, 0xff, out_bytes);
        return SMX_OK;
    }
    std::vector<uint64_t> doff;
    std::vector<unsigned char> pad;
    rc = smx::reach_sequences(seqs, off, n_seqs, &doff, &pad, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    auto &W = g_reach;
    HIP_TRY(W.seqs.upload(pad));
    HIP_TRY(W.doff.upload(doff));
    HIP_TRY(W.len.upload(P.len));
    HIP_TRY(W.weight.upload(weight, (size_t)n_seqs * 4));
    HIP_TRY(W.need.upload(need, (size_t)n_seqs * 4));
    HIP_TRY(W.recs.upload(P.recs));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    HIP_TRY(W.jobs.upload(P.jobs));
    HIP_TRY(W.out.ensure(out_bytes));
    HIP_TRY(hipMemset(W.out.p, 0xff, out_bytes));
    KernelTimer timer;
    if (kernel_ms) HIP_TRY(timer.start());
    const int e = smx_launch_reach(nullptr, matrix, W.seqs.as<unsigned char>(), W.doff.as<uint64_t>(), W.len.as<int32_t>(),
                                   W.weight.as<uint32_t>(), W.need.as<uint32_t>(), W.recs.p, W.chunk_start.as<uint64_t>(),
                                   (uint32_t)P.recs.size(), W.jobs.p, (int)P.grid, P.per_block, (int)E, n_seqs,
                                   W.out.as<unsigned long long>(), W.out.as<uint32_t>());
    if (e != 0) return fail(SMX_ERR_DEVICE, "reach kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (kernel_ms) HIP_TRY(timer.stop(kernel_ms));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(matrix ? (void *)reach : (void *)keys, W.out.p, out_bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}
}  // namespace

int smx_prefix_reach(const char *seqs, const uint64_t *off, uint32_t n_seqs, const uint32_t *weight, const uint32_t *need,
                     const smx_reach_job *jobs, uint32_t n_jobs, uint32_t E, uint64_t *keys, float *kernel_ms) {
    return reach_call(false, seqs, off, n_seqs, weight, need, jobs, n_jobs, E, keys, nullptr, kernel_ms);
}

int smx_prefix_reach_matrix(const char *seqs, const uint64_t *off, uint32_t n_seqs, const uint32_t *weight,
                            const uint32_t *need, const smx_reach_job *jobs, uint32_t n_jobs, uint32_t E, uint32_t *reach,
                            float *kernel_ms) {
    return reach_call(true, seqs, off, n_seqs, weight, need, jobs, n_jobs, E, nullptr, reach, kernel_ms);
}

// ---- consensus: every member read of a job aligned to the job's draft with traceback, the rows reduced to votes
// (smx_cons.hip); a workspace of its own, like g_pairs, with the history of the workgroups in flight
namespace {
struct {
    std::mutex mutex;
    DevBuf reads, doff, len, k, jobs, align, chunk_start;
    DevBuf scratch;             // per-lane state of the generic class, one slice per workgroup
    DevBuf hist_pm, hist_s;     // the alignment history, one slice per workgroup
    DevBuf rows, dist, votes, aligned;
    DevBuf planes_off, sites, n_sites, n_qualified, planes, link;   // smx_cons_phase (smx_phase.hip)
    DevBuf masks, member_off, agree_off, agree, sub_aligned;        // smx_cons_resample (smx_resample.hip)
} g_cons;

struct ConsPhase {      // what smx_cons_phase adds to a votes call
    uint32_t min_permille, min_reads, max_sites;
    smx_cons_site *sites;
    uint32_t *n_sites, *n_qualified;
    uint64_t *planes;
    uint32_t *link;
};

struct ConsResample {   // what smx_cons_resample adds to a votes call
    const uint64_t *masks;
    uint32_t n_levels;
    uint64_t *agree;
    uint32_t *sub_aligned;
};

// One smx_cons_* call.  rows / dist (pileup) or votes / aligned (votes) receive the result, the others are null; with
// `phase` a votes call goes on to the variant kernels over the rows and votes it left on the device, with `resample` to
// the resampling kernel over the rows and distances.
int cons_call(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k, const smx_cons_job *jobs,
              uint32_t n_jobs, uint32_t *rows, int32_t *dist, uint32_t *votes, uint32_t *aligned, float *kernel_ms,
              const ConsPhase *phase = nullptr, const ConsResample *resample = nullptr) {
    const bool pileup = rows || dist;
    if (!reads || !roff || !k || (n_jobs && (!jobs || (pileup ? !rows || !dist : !votes || !aligned))))
        return fail(SMX_ERR_ARG, "null argument");
    if (phase && n_jobs && (!phase->sites || !phase->n_sites || !phase->n_qualified || !phase->planes || !phase->link))
        return fail(SMX_ERR_ARG, "null argument");
    if (resample && n_jobs && (!resample->agree || !resample->sub_aligned)) return fail(SMX_ERR_ARG, "null argument");
    // every check of the arguments comes before the device is touched
    uint64_t hist_budget = smx::CONS_HIST_BYTES;
    if (const char *env = getenv("SMX_CONS_HIST_BYTES")) hist_budget = strtoull(env, nullptr, 10);   // test hook: few workgroups in flight
    smx::ConsPlan P;
    std::string why;
    int rc = smx::cons_plan(reads, roff, n_reads, k, jobs, n_jobs, hist_budget, &P, &why);
    if (rc == SMX_OK && phase) rc = smx::cons_plan_phase(phase->min_permille, phase->max_sites, &P, &why);
    if (rc == SMX_OK && resample) rc = smx::cons_plan_resample(resample->masks != nullptr, resample->n_levels, &P, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return SMX_OK;
    std::lock_guard<std::mutex> guard(g_cons.mutex);
    SMX_TRY(require_device());
    std::vector<uint64_t> doff;
    std::vector<int32_t> len;
    std::vector<unsigned char> pad;
    SMX_TRY(mine_targets(reads, roff, n_reads, &doff, &len, &pad));
    auto &W = g_cons;
    HIP_TRY(W.reads.upload(pad));
    HIP_TRY(W.doff.upload(doff));
    HIP_TRY(W.len.upload(len));
    HIP_TRY(W.k.upload(k, (size_t)n_reads * 4));
    HIP_TRY(W.jobs.upload(P.jobs));
    HIP_TRY(W.align.upload(P.align));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    HIP_TRY(W.rows.ensure((size_t)P.rows_words * 4));
    HIP_TRY(W.dist.ensure((size_t)P.n_dist * 4));
    // runs of chunks per workgroup only where the history bounds the grid: a chunk is 128 alignments with traceback,
    // and a call has few of them by the standards of the device
    smx::ChunkGrid G[6];
    uint64_t grid_max = 0;
    for (int c = 0; c < 6; c++) {
        G[c] = smx::chunk_grid(P.chunks[c], 1, P.grid_cap);
        grid_max = std::max(grid_max, G[c].grid);
    }
    HIP_TRY(W.hist_pm.ensure((size_t)(grid_max * P.hist_slice * MINE_THREADS * sizeof(smx::cons_pm))));
    HIP_TRY(W.hist_s.ensure((size_t)(grid_max * P.hist_slice * MINE_THREADS * sizeof(int))));
    if (P.n_align[0]) HIP_TRY(W.scratch.ensure((size_t)smx::chunk_scratch_words(G[0].grid, P.words_max0) * 8));
    if (!pileup) {
        HIP_TRY(W.votes.ensure((size_t)P.votes_words * 4));
        HIP_TRY(W.aligned.ensure((size_t)n_jobs * 4));
    }
    if (phase) {
        HIP_TRY(W.planes_off.upload(P.planes_off));
        HIP_TRY(W.sites.ensure((size_t)P.site_slots * sizeof(smx_cons_site)));
        HIP_TRY(W.n_sites.ensure((size_t)n_jobs * 4));
        HIP_TRY(W.n_qualified.ensure((size_t)n_jobs * 4));
        HIP_TRY(W.planes.ensure((size_t)P.planes_off.back() * 8));
        HIP_TRY(W.link.ensure((size_t)P.link_words * 4));
    }
    if (resample) {
        HIP_TRY(W.masks.upload(resample->masks, (size_t)P.mask_words * 8));
        HIP_TRY(W.member_off.upload(P.member_off));
        HIP_TRY(W.agree_off.upload(P.agree_off));
        HIP_TRY(W.agree.ensure((size_t)P.agree_off.back() * 8));
        HIP_TRY(W.sub_aligned.ensure((size_t)P.sub_words * 4));
    }
    KernelTimer timer;
    if (kernel_ms) HIP_TRY(timer.start());
    int e = smx::chunk_for_each_class(P.n_align, [&](int c, int wr, uint32_t n, size_t jat, size_t cat) {
        return smx_launch_cons_align(nullptr, wr, W.reads.as<unsigned char>(), W.doff.as<uint64_t>(), W.len.as<int32_t>(),
                                     W.k.as<int32_t>(), W.align.as<smx::ConsJobDev>() + jat, W.chunk_start.as<uint64_t>() + cat,
                                     n, (int)G[c].grid, G[c].per_block, P.lds_max[c], W.rows.as<uint32_t>(),
                                     W.dist.as<int32_t>(), W.hist_pm.p, W.hist_s.as<int>(), P.hist_slice,
                                     W.scratch.as<unsigned long long>(), P.words_max0);
    });
    if (e == 0 && !pileup)
        e = smx_launch_cons_vote(nullptr, W.len.as<int32_t>(), W.jobs.p, n_jobs, P.max_words, W.rows.as<uint32_t>(),
                                 W.dist.as<int32_t>(), W.votes.as<uint32_t>(), W.aligned.as<uint32_t>());
    if (e == 0 && phase)
        e = smx_launch_cons_phase(nullptr, W.len.as<int32_t>(), W.jobs.p, n_jobs, W.rows.as<uint32_t>(), W.dist.as<int32_t>(),
                                  W.votes.as<uint32_t>(), W.aligned.as<uint32_t>(), phase->min_permille, phase->min_reads,
                                  phase->max_sites, P.max_plane_words, W.planes_off.as<uint64_t>(), W.sites.p,
                                  W.n_sites.as<uint32_t>(), W.n_qualified.as<uint32_t>(), W.planes.as<uint64_t>(),
                                  W.link.as<uint32_t>());
    if (e == 0 && resample)
        e = smx_launch_cons_resample(nullptr, W.reads.as<unsigned char>(), W.doff.as<uint64_t>(), W.len.as<int32_t>(), W.jobs.p,
                                     n_jobs, resample->n_levels, P.max_words, W.rows.as<uint32_t>(), W.dist.as<int32_t>(),
                                     W.masks.as<uint64_t>(), W.member_off.as<uint64_t>(), W.agree_off.as<uint64_t>(),
                                     P.member_off.back(), W.agree.as<uint64_t>(), W.sub_aligned.as<uint32_t>());
    if (e != 0) return fail(SMX_ERR_DEVICE, "consensus kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (kernel_ms) HIP_TRY(timer.stop(kernel_ms));
    HIP_TRY(hipDeviceSynchronize());
    if (pileup) {
        if (P.n_dist) HIP_TRY(hipMemcpy(dist, W.dist.p, (size_t)P.n_dist * 4, hipMemcpyDeviceToHost));
        if (P.rows_words) HIP_TRY(hipMemcpy(rows, W.rows.p, (size_t)P.rows_words * 4, hipMemcpyDeviceToHost));
        for (const smx::ConsJobDev &J : P.jobs) {     // a member above the limit has no row
            const size_t words = (size_t)P.len[J.draft] + 1;
            for (uint32_t i = 0; i < J.n; i++)
                if (dist[J.dist_off + i] < 0) memset(rows + J.rows_off + i * words, 0xff, words * 4);
        }
    } else {
        HIP_TRY(hipMemcpy(votes, W.votes.p, (size_t)P.votes_words * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(aligned, W.aligned.p, (size_t)n_jobs * 4, hipMemcpyDeviceToHost));
    }
    if (phase) {
        HIP_TRY(hipMemcpy(phase->sites, W.sites.p, (size_t)P.site_slots * sizeof(smx_cons_site), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(phase->n_sites, W.n_sites.p, (size_t)n_jobs * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(phase->n_qualified, W.n_qualified.p, (size_t)n_jobs * 4, hipMemcpyDeviceToHost));
        if (P.planes_off.back()) HIP_TRY(hipMemcpy(phase->planes, W.planes.p, (size_t)P.planes_off.back() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(phase->link, W.link.p, (size_t)P.link_words * 4, hipMemcpyDeviceToHost));
    }
    if (resample) {
        HIP_TRY(hipMemcpy(resample->agree, W.agree.p, (size_t)P.agree_off.back() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(resample->sub_aligned, W.sub_aligned.p, (size_t)P.sub_words * 4, hipMemcpyDeviceToHost));
    }
    return SMX_OK;
}
}  // namespace

int smx_cons_pileup(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k, const smx_cons_job *jobs,
                    uint32_t n_jobs, uint32_t *rows, int32_t *dist, float *kernel_ms) {
    if (n_jobs && (!rows || !dist)) return fail(SMX_ERR_ARG, "null argument");
    return cons_call(reads, roff, n_reads, k, jobs, n_jobs, rows, dist, nullptr, nullptr, kernel_ms);
}

int smx_cons_votes(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k, const smx_cons_job *jobs,
                   uint32_t n_jobs, uint32_t *votes, uint32_t *aligned, float *kernel_ms) {
    if (n_jobs && (!votes || !aligned)) return fail(SMX_ERR_ARG, "null argument");
    return cons_call(reads, roff, n_reads, k, jobs, n_jobs, nullptr, nullptr, votes, aligned, kernel_ms);
}

int smx_cons_phase(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k, const smx_cons_job *jobs,
                   uint32_t n_jobs, uint32_t min_permille, uint32_t min_reads, uint32_t max_sites, uint32_t *votes,
                   uint32_t *aligned, smx_cons_site *sites, uint32_t *n_sites, uint32_t *n_qualified, uint64_t *planes,
                   uint32_t *link, float *kernel_ms) {
    if (n_jobs && (!votes || !aligned)) return fail(SMX_ERR_ARG, "null argument");
    const ConsPhase phase{min_permille, min_reads, max_sites, sites, n_sites, n_qualified, planes, link};
    return cons_call(reads, roff, n_reads, k, jobs, n_jobs, nullptr, nullptr, votes, aligned, kernel_ms, &phase);
}

int smx_cons_resample(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k, const smx_cons_job *jobs,
                      uint32_t n_jobs, const uint64_t *masks, uint32_t n_levels, uint32_t *votes, uint32_t *aligned,
                      uint64_t *agree, uint32_t *sub_aligned, float *kernel_ms) {
    if (n_jobs && (!votes || !aligned)) return fail(SMX_ERR_ARG, "null argument");
    const ConsResample resample{masks, n_levels, agree, sub_aligned};
    return cons_call(reads, roff, n_reads, k, jobs, n_jobs, nullptr, nullptr, votes, aligned, kernel_ms, nullptr, &resample);
}

// ---- inner scan: every pattern against the whole read, hits on the internal columns (smx_inner.hip)
extern "C" int smx_batch_seq_view(const smx_batch *b, const char **seq, uint32_t *len);   // smx_io.cpp

namespace {
struct {
    std::mutex mutex;
    DevBuf bases, roff, ustart, unit_read, recs, out, tables;
} g_inner;

// The reads are seq[i][0 .. len[i]); with `flat` they also lie back to back from flat (seq[i] = flat + flat_off[i]).
int inner_call(const char *patterns, const uint32_t *poff, uint32_t Q, const int32_t *k, const char *const *seq,
               const uint32_t *len, const uint8_t *flat, uint32_t n_reads, int32_t margin, uint32_t H,
               uint64_t budget, uint8_t *nhit, int8_t *hit_dist, int32_t *hit_end, float *kernel_ms) {
    if (!patterns || !poff || !k) return fail(SMX_ERR_ARG, "null argument");
    if (n_reads && (!seq || !len || !nhit || !hit_dist || !hit_end)) return fail(SMX_ERR_ARG, "null argument");
    // the pattern checks, lead / PL / RW, the table blob and the launch groups: smx_inner_plan.h
    smx::InnerPlan P;
    std::string why;
    int rc = smx::inner_plan(patterns, poff, Q, k, margin, H, budget, smx::INNER_DEFAULT_BUDGET,
                             smx::InnerAlphabet{code_of, build_peq}, &P, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    std::lock_guard<std::mutex> guard(g_inner.mutex);
    SMX_TRY(require_device());
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_reads == 0) return SMX_OK;
    auto &W = g_inner;
    HIP_TRY(W.tables.upload(P.blob));
    KernelTimer timer;
    smx::InnerGroup g;
    std::vector<unsigned char> stage, out;
    // groups of whole reads: everything one launch group keeps on the device fits the budget (one read always goes)
    for (uint32_t r0 = 0; r0 < n_reads; r0 = g.r1) {
        rc = P.next_group(len, n_reads, r0, &g, &why);
        if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
        const uint32_t nr = g.nr();
        const unsigned char *src;
        if (flat) {
            src = (const unsigned char *)seq[r0];
        } else {
            stage.resize(g.nb);
            for (uint32_t i = 0; i < nr; i++)
                if (len[r0 + i]) memcpy(stage.data() + g.roff[i], seq[r0 + i], len[r0 + i]);
            src = stage.data();
        }
        HIP_TRY(W.bases.upload(src, g.nb, g.bases_bytes - g.nb));    // readable to the end of the last byte's 16-byte word
        HIP_TRY(W.roff.upload(g.roff));
        HIP_TRY(W.ustart.upload(g.ustart));
        HIP_TRY(W.unit_read.upload(g.unit_read));
        HIP_TRY(W.recs.ensure(g.rec_bytes));
        HIP_TRY(W.out.ensure(g.out_bytes()));
        smx::InnerArgs A{};
        A.lut = W.tables.as<unsigned char>();
        A.bases = W.bases.as<smx::mine_u4>();
        A.roff = W.roff.as<uint64_t>();
        A.ustart = W.ustart.as<uint32_t>();
        A.unit_read = W.unit_read.as<uint32_t>();
        A.n_units = (uint32_t)g.units;
        A.Q = (int)Q;
        A.H = (int)H;
        A.margin = margin;
        A.PL = P.PL;
        A.lead = P.lead;
        A.recs = W.recs.as<uint32_t>();
        int32_t *d_he = W.out.as<int32_t>();
        int8_t *d_hd = W.out.as<int8_t>() + g.he_bytes;
        uint8_t *d_nh = W.out.as<uint8_t>() + g.he_bytes + g.hd_bytes;
        if (kernel_ms) HIP_TRY(timer.start());
        int e = 0;
        for (const smx::InnerClass &C : P.cls) {
            if (C.idx.empty() || g.units == 0 || e != 0) continue;
            A.peq = W.tables.as<char>() + C.peq_at;
            A.pm = (const int *)(W.tables.as<char>() + C.tab_at);
            A.pk = A.pm + C.slots();
            A.jmap = A.pm + 2 * C.slots();
            e = smx_launch_inner_scan(nullptr, C.w64, C.G, C.npass, &A);
        }
        if (e == 0) e = smx_launch_inner_merge(nullptr, &A, nr, d_nh, d_hd, d_he);
        if (e != 0) return fail(SMX_ERR_DEVICE, "inner scan launch failed: %s", hipGetErrorString((hipError_t)e));
        if (kernel_ms) {
            float ms = 0.0f;
            HIP_TRY(timer.stop(&ms));
            *kernel_ms += ms;
        }
        HIP_TRY(hipDeviceSynchronize());
        out.resize(g.out_bytes());
        HIP_TRY(hipMemcpy(out.data(), W.out.p, out.size(), hipMemcpyDeviceToHost));
        memcpy(hit_end + (size_t)r0 * Q * H, out.data(), g.he_bytes);
        memcpy(hit_dist + (size_t)r0 * Q * H, out.data() + g.he_bytes, g.hd_bytes);
        memcpy(nhit + (size_t)r0 * Q, out.data() + g.he_bytes + g.hd_bytes, g.nh_bytes);
    }
    return SMX_OK;
}
}  // namespace

int smx_inner_scan(const char *patterns, const uint32_t *poff, uint32_t n_patterns, const int32_t *k, const uint8_t *bases,
                   const uint64_t *off, uint32_t n_reads, int32_t margin, uint32_t max_hits, uint64_t budget_bytes,
                   uint8_t *nhit, int8_t *hit_dist, int32_t *hit_end, float *kernel_ms) {
    if (n_reads && (!bases || !off)) return fail(SMX_ERR_ARG, "null argument");
    std::vector<const char *> seq(n_reads);
    std::vector<uint32_t> len(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > (uint64_t)INT32_MAX) return fail(SMX_ERR_ARG, "read %u: bad offsets", i);
        seq[i] = (const char *)bases + off[i];
        len[i] = (uint32_t)(off[i + 1] - off[i]);
    }
    return inner_call(patterns, poff, n_patterns, k, seq.data(), len.data(), bases, n_reads, margin, max_hits, budget_bytes,
                      nhit, hit_dist, hit_end, kernel_ms);
}

int smx_inner_scan_batch(const smx_batch *batch, const char *patterns, const uint32_t *poff, uint32_t n_patterns,
                         const int32_t *k, int32_t margin, uint32_t max_hits, uint64_t budget_bytes, uint8_t *nhit,
                         int8_t *hit_dist, int32_t *hit_end, float *kernel_ms) {
    if (!batch) return fail(SMX_ERR_ARG, "null argument");
    const uint32_t n_reads = smx_batch_size(batch);
    std::vector<const char *> seq(n_reads);
    std::vector<uint32_t> len(n_reads);
    SMX_TRY(smx_batch_seq_view(batch, seq.data(), len.data()));
    return inner_call(patterns, poff, n_patterns, k, seq.data(), len.data(), nullptr, n_reads, margin, max_hits, budget_bytes,
                      nhit, hit_dist, hit_end, kernel_ms);
}
