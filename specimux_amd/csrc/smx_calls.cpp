// smx_calls.cpp -- the one-shot calls of libsmx.so over host buffers: alignments (smx_align, smx_align_batch), specimine
// (smx_mine.hip), clusters (smx_pairs.hip), consensus (smx_cons.hip), crosstalk (smx_nearest.hip), identify (smx_hits.hip), bimera (smx_reach.hip), tree (smx_nj.hip), msa (smx_msa.hip) and the inner scan (smx_inner.hip).  Each keeps one grow-only device workspace; its calls are serialised.
// Every *_call below runs in one order: null checks, the plan (a bad call is refused here, without a
// device), the workspace's lock, require_device, *kernel_ms = 0, the early returns of a call without work, the uploads,
// the launches (timed_launches), the copy-out.  Consensus alone zeroes *kernel_ms and answers a call without jobs
// before it asks for the device (the tests pin it), so there a good call without a device fails with *kernel_ms
// zeroed.  What a call uploads beyond its sequences and what it copies out is spelled out in the call; the rest is
// the frame right below.
#include "smx_host.h"
#include "smx_align_lane.h"   // align_collect
#include "smx_cons_plan.h"
#include "smx_nearest_plan.h"
#include "smx_hits_plan.h"
#include "smx_reach_plan.h"
#include "smx_nj_plan.h"
#include "smx_msa_plan.h"
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

// ---- the frame of the chunked calls
namespace {
// a plan's refusal (smx_*_plan.h: a status and why) as the call's failure
int refused(int rc, const std::string &why) { return rc == SMX_OK ? SMX_OK : fail(rc, "%s", why.c_str()); }

// The padded sequences of a call on the device: the bytes, where each begins and how long it is.
struct DevSeqs {
    DevBuf bytes, doff, len;
    int upload(const std::vector<unsigned char> &pad, const std::vector<uint64_t> &off, const std::vector<int32_t> &lens) {
        HIP_TRY(bytes.upload(pad));
        HIP_TRY(doff.upload(off));
        HIP_TRY(len.upload(lens));
        return SMX_OK;
    }
    int upload(const char *seqs, const uint64_t *off, uint32_t n) {   // the caller's sequences, padded here (smx_chunk_plan.h)
        std::vector<uint64_t> d;
        std::vector<int32_t> l;
        std::vector<unsigned char> pad;
        std::string why;
        SMX_TRY(refused(smx::chunk_padded_sequences(seqs, off, n, &d, &l, &pad, &why), why));
        return upload(pad, d, l);
    }
};

// the generic class's per-lane state, one slice per workgroup: only a call with records of that class needs it
int ensure_scratch(DevBuf *scratch, const smx::ChunkLaunches &L) {
    if (L.n[0]) HIP_TRY(scratch->ensure((size_t)L.scratch_words * 8));
    return SMX_OK;
}

// The launches of a call, timed if the caller asks for it: enqueue() puts them on the null stream and returns the
// first nonzero launch status.  what: "mining kernel launch", for the message.  Returns once the device is idle.
// The events are the section's own: the inner scan, which has a section per launch group, creates a pair per group.
template <typename F> int timed_launches(float *kernel_ms, const char *what, F &&enqueue) {
    KernelTimer timer;
    if (kernel_ms) HIP_TRY(timer.start());
    if (const int e = enqueue()) return fail(SMX_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString((hipError_t)e));
    if (kernel_ms) HIP_TRY(timer.stop(kernel_ms));
    HIP_TRY(hipDeviceSynchronize());
    return SMX_OK;
}
}  // namespace

// ---- specimine: batched long-read HW distances (smx_mine.hip); grow-only device workspace, calls serialised
namespace {
struct {
    std::mutex mutex;
    DevBuf queries, qoff, pairs, chunk_start;
    DevSeqs targets;
    DevBuf scratch;     // per-lane state of the generic class, one slice per workgroup
    DevBuf jobs_out;    // the jobs, then the output
} g_mine;

// One smx_mine_* call.  distances: job j's nq x nt distances at out[sum over earlier jobs of nq * nt] (int32); else
// the best identities at out[sum over earlier jobs of nt] (double).  Device and host memory hold the queries, the
// targets, sum(nq) (job, query) pairs and the output: only the distance output grows with sum(nq * nt).
int mine_call(bool distances, const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k,
              const char *targets, const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs, uint32_t n_jobs,
              void *out, float *kernel_ms) {
    if (!out && n_jobs) return fail(SMX_ERR_ARG, "null argument");
    if (!queries || !qoff || !k || !targets || !toff || (n_jobs && !jobs)) return fail(SMX_ERR_ARG, "null argument");
    // the checks, the padded targets, the jobs, the (job, query) records by class and the grids: smx_mine_plan.h
    smx::MinePlan P;
    std::string why;
    SMX_TRY(refused(smx::mine_plan(queries, qoff, n_queries, k, targets, toff, n_targets, jobs, n_jobs, smx::CHUNK_SCRATCH_BYTES,
                                   &P, &why), why));
    std::lock_guard<std::mutex> guard(g_mine.mutex);
    SMX_TRY(require_device());
    if (kernel_ms) *kernel_ms = 0.0f;
    const uint64_t n_out = distances ? P.n_dist : P.n_best;
    if (n_out == 0) return SMX_OK;
    const size_t out_bytes = n_out * (distances ? sizeof(int32_t) : sizeof(double));
    auto &W = g_mine;
    const size_t jobs_bytes = n_jobs * sizeof(smx::MineJobDev);
    HIP_TRY(W.queries.upload(queries, (size_t)qoff[n_queries]));
    HIP_TRY(W.qoff.upload(qoff, ((size_t)n_queries + 1) * 8));
    SMX_TRY(W.targets.upload(P.tpad, P.tdoff, P.tlen));
    HIP_TRY(W.pairs.upload(P.pairs));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    SMX_TRY(ensure_scratch(&W.scratch, P));
    HIP_TRY(W.jobs_out.upload(P.jobs.data(), jobs_bytes, out_bytes));
    void *d_out = W.jobs_out.as<char>() + jobs_bytes;
    if (!distances) HIP_TRY(hipMemset(d_out, 0, out_bytes));       // +0.0: "no pair counts"
    SMX_TRY(timed_launches(kernel_ms, "mining kernel launch", [&] {
        return smx::chunk_for_each_class(P, [&](const smx::ChunkLaunch &L) {
            return smx_launch_mine(nullptr, L.wr, distances, W.queries.as<unsigned char>(), W.qoff.as<uint64_t>(),
                                   W.targets.bytes.as<unsigned char>(), W.targets.doff.as<uint64_t>(), W.targets.len.as<int32_t>(),
                                   W.pairs.as<smx::MinePair>() + L.rec_at, W.chunk_start.as<uint64_t>() + L.start_at, L.n,
                                   W.jobs_out.p, L.grid, L.per_block, L.lds, d_out, W.scratch.as<unsigned long long>(),
                                   P.words_max0);
        });
    }));
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
    DevSeqs reads;
    DevBuf k, rows, chunk_start;
    DevBuf scratch;     // per-lane state of the generic class, one slice per workgroup
    DevBuf jobs_out;    // the jobs, then the output
} g_pairs;

// One smx_pairs_* call.  distances: job j's n (n - 1) / 2 distances (int32); else its n x ceil(n / 32) adjacency words,
// the upper triangle from the kernel, mirrored here.  Either way job j's output follows the earlier jobs'.
int pairs_call(bool distances, const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
               const smx_pairs_job *jobs, uint32_t n_jobs, uint32_t *out, float *kernel_ms) {
    if (!reads || !roff || !k || (n_jobs && (!jobs || !out))) return fail(SMX_ERR_ARG, "null argument");
    // the checks, the padded reads, the jobs, the rows by class and the grids: smx_pairs_plan.h
    smx::PairsPlan P;
    std::string why;
    SMX_TRY(refused(smx::pairs_plan(distances, reads, roff, n_reads, jobs, n_jobs, smx::CHUNK_SCRATCH_BYTES, &P, &why), why));
    std::lock_guard<std::mutex> guard(g_pairs.mutex);
    SMX_TRY(require_device());
    if (kernel_ms) *kernel_ms = 0.0f;
    if (P.n_out == 0) return SMX_OK;
    const size_t out_bytes = P.n_out * 4;
    if (P.rows.empty()) {                         // only jobs of one read: a zero word each
        memset(out, 0, out_bytes);
        return SMX_OK;
    }
    auto &W = g_pairs;
    const size_t jobs_bytes = (n_jobs * sizeof(smx::PairsJobDev) + 15) & ~(size_t)15;
    SMX_TRY(W.reads.upload(P.pad, P.doff, P.len));
    HIP_TRY(W.k.upload(k, (size_t)n_reads * 4));
    HIP_TRY(W.rows.upload(P.rows));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    SMX_TRY(ensure_scratch(&W.scratch, P));
    HIP_TRY(W.jobs_out.upload(P.jobs.data(), n_jobs * sizeof(smx::PairsJobDev), jobs_bytes - n_jobs * sizeof(smx::PairsJobDev) + out_bytes));
    void *d_out = W.jobs_out.as<char>() + jobs_bytes;
    if (!distances) HIP_TRY(hipMemset(d_out, 0, out_bytes));
    SMX_TRY(timed_launches(kernel_ms, "pairs kernel launch", [&] {
        return smx::chunk_for_each_class(P, [&](const smx::ChunkLaunch &L) {
            return smx_launch_pairs(nullptr, L.wr, distances, W.reads.bytes.as<unsigned char>(), W.reads.doff.as<uint64_t>(),
                                    W.reads.len.as<int32_t>(), W.k.as<int32_t>(), W.rows.as<smx::PairsRow>() + L.rec_at,
                                    W.chunk_start.as<uint64_t>() + L.start_at, L.n, W.jobs_out.p, L.grid, L.per_block, L.lds,
                                    d_out, W.scratch.as<unsigned long long>(), P.words_max0);
        });
    }));
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
    DevSeqs seqs;
    DevBuf k, group, refs, runs, chunk_start, jobs;
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
    smx::NearestPlan P;
    std::string why;
    SMX_TRY(refused(smx::nearest_plan(seqs, off, n_seqs, jobs, n_jobs, &P, &why), why));
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
    auto &W = g_nearest;
    SMX_TRY(W.seqs.upload(seqs, off, n_seqs));
    HIP_TRY(W.k.upload(k, (size_t)n_seqs * 4));
    HIP_TRY(W.group.upload(group, (size_t)n_seqs * 4));
    HIP_TRY(W.refs.upload(P.refs));
    HIP_TRY(W.runs.upload(P.runs));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    HIP_TRY(W.jobs.upload(P.jobs));
    SMX_TRY(ensure_scratch(&W.scratch, P));
    HIP_TRY(W.out.ensure(out_bytes));
    // nearest: "no ref" until a lane says otherwise.  distances: every pair is written (nt > 0 and nq > 0 make runs)
    if (!distances) HIP_TRY(hipMemset(W.out.p, 0xff, out_bytes));
    unsigned long long *d_own = W.out.as<unsigned long long>(), *d_other = d_own + (distances ? 0 : P.n_best);
    size_t ref_at[6] = {0, 0, 0, 0, 0, 0};             // every class's own ref list, one after the other
    for (int c = 1; c < 6; c++) ref_at[c] = ref_at[c - 1] + P.n_refs[c - 1];
    SMX_TRY(timed_launches(kernel_ms, "nearest kernel launch", [&] {
        return smx::chunk_for_each_class(P, [&](const smx::ChunkLaunch &L) {
            return smx_launch_nearest(nullptr, L.wr, distances, W.seqs.bytes.as<unsigned char>(), W.seqs.doff.as<uint64_t>(),
                                      W.seqs.len.as<int32_t>(), W.k.as<int32_t>(), W.group.as<uint32_t>(),
                                      W.refs.as<uint32_t>() + ref_at[L.c], W.runs.as<smx::NearestRun>() + L.rec_at,
                                      W.chunk_start.as<uint64_t>() + L.start_at, L.n, W.jobs.p, L.grid, L.per_block, L.lds, d_own,
                                      d_other, W.out.as<int32_t>(), W.scratch.as<unsigned long long>(), P.words_max0);
        });
    }));
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
    DevSeqs seqs;
    DevBuf k, ord, recs, chunk_start, jobs;
    DevBuf scratch;     // per-lane state of the generic class, one slice per workgroup
    DevBuf out;         // the keys, or the distances
} g_hits;

// One smx_best_hits* call.  distances: dist receives job after job its nq x nt distances; else keys receives sum(nq) x K keys.
int hits_call(bool distances, const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k,
              const smx_hits_job *jobs, uint32_t n_jobs, uint32_t K, uint32_t min_cov_permille, uint64_t *keys, int32_t *dist,
              float *kernel_ms) {
    if (!seqs || !off || !k || (n_jobs && (!jobs || (distances ? !dist : !keys)))) return fail(SMX_ERR_ARG, "null argument");
    smx::HitsPlan P;
    std::string why;
    SMX_TRY(refused(smx::hits_plan(seqs, off, n_seqs, jobs, n_jobs, K, min_cov_permille, &P, &why), why));
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
    auto &W = g_hits;
    SMX_TRY(W.seqs.upload(seqs, off, n_seqs));
    HIP_TRY(W.k.upload(k, (size_t)n_seqs * 4));
    HIP_TRY(W.ord.upload(P.ord));
    HIP_TRY(W.recs.upload(P.recs));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    HIP_TRY(W.jobs.upload(P.jobs));
    SMX_TRY(ensure_scratch(&W.scratch, P));
    HIP_TRY(W.out.ensure(out_bytes));
    HIP_TRY(hipMemset(W.out.p, 0xff, out_bytes));
    SMX_TRY(timed_launches(kernel_ms, "hits kernel launch", [&] {
        return smx::chunk_for_each_class(P, [&](const smx::ChunkLaunch &L) {
            return smx_launch_hits(nullptr, L.wr, distances, W.seqs.bytes.as<unsigned char>(), W.seqs.doff.as<uint64_t>(),
                                   W.seqs.len.as<int32_t>(), W.k.as<int32_t>(), W.ord.as<uint32_t>(),
                                   W.recs.as<smx::HitsRec>() + L.rec_at, W.chunk_start.as<uint64_t>() + L.start_at, L.n, W.jobs.p,
                                   L.grid, L.per_block, L.lds, (int)K, W.out.as<unsigned long long>(), W.out.as<int32_t>(),
                                   W.scratch.as<unsigned long long>(), P.words_max0);
        });
    }));
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
    DevSeqs seqs;       // forwards, then reversed (reach_sequences); len per sequence
    DevBuf weight, need, recs, chunk_start, jobs;
    DevBuf out;         // the keys, or the matrix
} g_reach;

// One smx_prefix_reach* call.  matrix: reach receives job after job its nq x nt x 2 x (E + 1) values; else keys receives
// sum(nq) x 2 x (E + 1) x 2 keys.
int reach_call(bool matrix, const char *seqs, const uint64_t *off, uint32_t n_seqs, const uint32_t *weight,
               const uint32_t *need, const smx_reach_job *jobs, uint32_t n_jobs, uint32_t E, uint64_t *keys, uint32_t *reach,
               float *kernel_ms) {
    if (!seqs || !off || !weight || !need || (n_jobs && (!jobs || (matrix ? !reach : !keys)))) return fail(SMX_ERR_ARG, "null argument");
    smx::ReachPlan P;
    std::string why;
    SMX_TRY(refused(smx::reach_plan(off, n_seqs, jobs, n_jobs, E, &P, &why), why));
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
    SMX_TRY(refused(smx::reach_sequences(seqs, off, n_seqs, &doff, &pad, &why), why));
    auto &W = g_reach;
    SMX_TRY(W.seqs.upload(pad, doff, P.len));
    HIP_TRY(W.weight.upload(weight, (size_t)n_seqs * 4));
    HIP_TRY(W.need.upload(need, (size_t)n_seqs * 4));
    HIP_TRY(W.recs.upload(P.recs));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    HIP_TRY(W.jobs.upload(P.jobs));
    HIP_TRY(W.out.ensure(out_bytes));
    HIP_TRY(hipMemset(W.out.p, 0xff, out_bytes));
    SMX_TRY(timed_launches(kernel_ms, "reach kernel launch", [&] {
        return smx_launch_reach(nullptr, matrix, W.seqs.bytes.as<unsigned char>(), W.seqs.doff.as<uint64_t>(),
                                W.seqs.len.as<int32_t>(), W.weight.as<uint32_t>(), W.need.as<uint32_t>(), W.recs.p,
                                W.chunk_start.as<uint64_t>(), (uint32_t)P.recs.size(), W.jobs.p, (int)P.grid, P.per_block, (int)E,
                                n_seqs, W.out.as<unsigned long long>(), W.out.as<uint32_t>());
    }));
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

// ---- tree: the neighbour-joining merges of n tips from their packed distance triangle (smx_nj.hip); a workspace of its
// own.  Every buffer entry a launch reads was written by an earlier launch of the same call, so nothing an earlier,
// larger call left in the workspace is ever seen
namespace {
struct {
    std::mutex mutex;
    DevBuf tri, d, r, node, best_q, best_hi, merges;
} g_nj;

int nj_call(const int32_t *tri, uint32_t n, smx_nj_merge *merges, uint32_t *last, double *last_d, float *kernel_ms) {
    // the checks, the buffer sizes and the launch counts: smx_nj_plan.h
    smx::NjPlan P;
    std::string why;
    SMX_TRY(refused(smx::nj_plan(tri, n, merges, last, last_d, &P, &why), why));
    std::lock_guard<std::mutex> guard(g_nj.mutex);
    SMX_TRY(require_device());
    if (kernel_ms) *kernel_ms = 0.0f;
    if (P.iterations == 0) {                      // n <= 3: nothing to join
        smx::nj_small(tri, n, last, last_d);
        return SMX_OK;
    }
    auto &W = g_nj;
    HIP_TRY(W.tri.upload(tri, (size_t)P.tri_bytes));
    HIP_TRY(W.d.ensure((size_t)P.d_bytes));
    HIP_TRY(W.r.ensure((size_t)P.r_bytes));
    HIP_TRY(W.node.ensure((size_t)P.node_bytes));
    HIP_TRY(W.best_q.ensure((size_t)P.best_q_bytes));
    HIP_TRY(W.best_hi.ensure((size_t)P.best_hi_bytes));
    HIP_TRY(W.merges.ensure((size_t)P.merges_bytes));
    SMX_TRY(timed_launches(kernel_ms, "tree kernel launch", [&] {
        return smx_launch_nj(nullptr, W.tri.as<int32_t>(), n, W.d.as<double>(), W.r.as<double>(), W.node.as<uint32_t>(),
                             W.best_q.as<double>(), W.best_hi.as<uint32_t>(), W.merges.p);
    }));
    HIP_TRY(hipMemcpy(merges, W.merges.p, (size_t)P.merges_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(last, W.node.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    double d3[3][3];                              // the slots 0, 1, 2 of the matrix
    HIP_TRY(hipMemcpy2D(d3, sizeof d3[0], W.d.p, (size_t)n * sizeof(double), sizeof d3[0], 3, hipMemcpyDeviceToHost));
    last_d[0] = d3[0][1];
    last_d[1] = d3[0][2];
    last_d[2] = d3[1][2];
    return SMX_OK;
}
}  // namespace

int smx_nj(const int32_t *tri, uint32_t n, smx_nj_merge *merges, uint32_t last[3], double last_d[3], float *kernel_ms) {
    return nj_call(tri, n, merges, last, last_d, kernel_ms);
}

// ---- msa: the progressive alignment of n sequences along a guide tree (smx_msa.hip); a workspace of its own.  The host
// waits once per level of the tree, reads that level's lengths (one small copy) and sizes the next level's launches by
// them.  Every buffer entry a launch reads was written by an earlier launch of the same call
namespace {
struct {
    std::mutex mutex;
    DevBuf bytes, doff, prof_off, prof, maps, recs, tb, ops, row, lens, costs, parent, map_off, rows, phase;
    // what smx_msa_debug_times hands out: of the last call that asked for kernel_ms, the device time of every level and of
    // the tips and rows launches; with SMX_MSA_PHASE_TIMING, the wall-clock ticks of the merge kernel's three phases,
    // summed over the call's merges
    std::vector<float> level_ms;
    float tips_ms = 0.0f, rows_ms = 0.0f;
    uint64_t phase_ticks[3] = {0, 0, 0};
    int clock_khz = 0;
} g_msa;

// a buffer that keeps its first `used` bytes when it grows: the profiles and maps of the levels that have run
hipError_t grow_keeping(DevBuf *b, size_t need, size_t used) {
    if (need <= b->cap) return hipSuccess;
    DevBuf bigger;
    hipError_t e = bigger.ensure(need + need / 2);
    if (e == hipSuccess && used) e = hipMemcpy(bigger.p, b->p, used, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
        bigger.release();
        return e;
    }
    b->release();
    *b = bigger;
    return hipSuccess;
}

int msa_call(const char *seqs, const uint64_t *off, uint32_t n, const smx_msa_merge *merges, uint32_t X, uint32_t G,
             uint32_t cap_cols, uint8_t *rows, uint32_t *n_cols, uint32_t *lens, uint64_t *costs, float *kernel_ms) {
    // the checks, the levels and the sizes: smx_msa_plan.h
    smx::MsaPlan P;
    std::string why;
    SMX_TRY(refused(smx::msa_plan(seqs, off, n, merges, X, G, rows, n_cols, lens, costs, &P, &why), why));
    // clusters.budget_bytes(): SMX_CLUSTERS_BUDGET_BYTES, else SMX_MINE_BUDGET_BYTES, else the default; empty or 0 is unset
    uint64_t budget = 0;
    for (const char *name : {"SMX_CLUSTERS_BUDGET_BYTES", "SMX_MINE_BUDGET_BYTES"})
        if (const char *env = budget ? nullptr : getenv(name)) budget = strtoull(env, nullptr, 10);
    if (!budget) budget = smx::MSA_DEFAULT_BUDGET;
    const bool phases = getenv("SMX_MSA_PHASE_TIMING") != nullptr;   // diagnostic: smx_msa_debug_times
    std::lock_guard<std::mutex> guard(g_msa.mutex);
    SMX_TRY(require_device());
    if (kernel_ms) *kernel_ms = 0.0f;
    *n_cols = 0;
    if (n == 0) return SMX_OK;
    if (n == 1) {                                 // nothing to align: the sequence is the row
        *n_cols = (uint32_t)(off[1] - off[0]);
        if (*n_cols > cap_cols) return fail(SMX_ERR_OVERFLOW, "%u columns, room for %u", *n_cols, cap_cols);
        memcpy(rows, seqs + off[0], *n_cols);
        return SMX_OK;
    }
    auto &W = g_msa;
    smx::MsaState S;
    smx::msa_state_init(P, off, &S);
    std::vector<uint64_t> doff(n + 1);
    for (uint32_t i = 0; i <= n; i++) doff[i] = off[i] - off[0];
    HIP_TRY(W.bytes.upload(seqs + off[0], (size_t)P.seq_bytes));
    HIP_TRY(W.doff.upload(doff));
    HIP_TRY(W.prof_off.upload(S.prof_off.data(), (size_t)n * sizeof(uint64_t)));
    HIP_TRY(W.prof.ensure((size_t)S.prof_used * 4 * sizeof(smx::MsaCol)));   // a guess; grow_keeping has the last word
    HIP_TRY(W.lens.ensure((size_t)P.n_merges * sizeof(uint32_t)));
    HIP_TRY(W.costs.ensure((size_t)P.n_merges * sizeof(uint64_t)));
    float total = 0.0f, ms = 0.0f;
    float *part = kernel_ms ? &ms : nullptr;
    W.level_ms.clear();
    W.tips_ms = W.rows_ms = 0.0f;
    W.phase_ticks[0] = W.phase_ticks[1] = W.phase_ticks[2] = 0;
    std::vector<unsigned long long> h_phase;
    SMX_TRY(timed_launches(part, "msa tips launch", [&] {
        return smx_launch_msa_tips(nullptr, W.bytes.as<unsigned char>(), W.doff.as<uint64_t>(), n, W.prof_off.as<uint64_t>(), W.prof.p);
    }));
    total += ms;
    W.tips_ms = ms;
    std::vector<uint32_t> h_lens(P.n_merges);
    std::vector<smx::MsaLaunch> launches;
    std::vector<smx::MsaMergeDev> recs;
    for (uint32_t v = 1; v <= P.n_levels; v++) {
        smx::msa_level_launches(P, merges, S, v, budget, &launches);
        float level = 0.0f;
        for (const smx::MsaLaunch &L : launches) {
            const uint64_t prof_before = S.prof_used, map_before = S.map_used;
            smx::msa_launch_records(P, merges, L, &S, &recs);
            HIP_TRY(grow_keeping(&W.prof, (size_t)S.prof_used * sizeof(smx::MsaCol), (size_t)prof_before * sizeof(smx::MsaCol)));
            HIP_TRY(grow_keeping(&W.maps, (size_t)S.map_used * sizeof(uint16_t), (size_t)map_before * sizeof(uint16_t)));
            HIP_TRY(W.recs.upload(recs));
            HIP_TRY(W.tb.ensure((size_t)L.tb_words * sizeof(uint32_t)));
            HIP_TRY(W.ops.ensure((size_t)L.ops_bytes));
            HIP_TRY(W.row.ensure((size_t)L.row_entries * sizeof(uint64_t)));
            if (phases) HIP_TRY(W.phase.ensure((size_t)L.count * 4 * sizeof(unsigned long long)));
            SMX_TRY(timed_launches(part, "msa merge launch", [&] {
                return smx_launch_msa_merge(nullptr, W.recs.p, L.count, X, G, W.prof.p, W.maps.as<uint16_t>(), W.tb.as<uint32_t>(),
                                            W.ops.as<uint8_t>(), W.row.as<uint64_t>(), W.lens.as<uint32_t>(), W.costs.as<uint64_t>(),
                                            phases ? W.phase.as<unsigned long long>() : nullptr);
            }));
            total += ms;
            level += ms;
            if (phases) {
                h_phase.resize((size_t)L.count * 4);
                HIP_TRY(hipMemcpy(h_phase.data(), W.phase.p, h_phase.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
                for (uint32_t x = 0; x < L.count; x++)
                    for (int k = 0; k < 3; k++) W.phase_ticks[k] += h_phase[4 * x + k + 1] - h_phase[4 * x + k];
            }
        }
        if (kernel_ms) W.level_ms.push_back(level);
        // the level's lengths: the next level is sized by them (entries of later levels are not looked at)
        HIP_TRY(hipMemcpy(h_lens.data(), W.lens.p, (size_t)P.n_merges * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (const smx::MsaLaunch &L : launches) SMX_TRY(refused(smx::msa_launch_done(P, L, h_lens.data(), &S, &why), why));
    }
    const uint32_t root_cols = S.len[P.n_nodes - 1];
    *n_cols = root_cols;
    memcpy(lens, h_lens.data(), (size_t)P.n_merges * sizeof(uint32_t));
    HIP_TRY(hipMemcpy(costs, W.costs.p, (size_t)P.n_merges * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = total;
    if (root_cols > cap_cols) return fail(SMX_ERR_OVERFLOW, "%u columns, room for %u", root_cols, cap_cols);
    HIP_TRY(W.parent.upload(P.parent));
    HIP_TRY(W.map_off.upload(S.map_off));
    HIP_TRY(W.rows.ensure((size_t)n * root_cols));
    SMX_TRY(timed_launches(part, "msa rows launch", [&] {
        return smx_launch_msa_rows(nullptr, W.bytes.as<unsigned char>(), W.doff.as<uint64_t>(), n, W.parent.as<uint32_t>(),
                                   W.map_off.as<uint64_t>(), W.maps.as<uint16_t>(), root_cols, W.rows.as<uint8_t>());
    }));
    total += ms;
    W.rows_ms = ms;
    if (kernel_ms) *kernel_ms = total;
    HIP_TRY(hipMemcpy(rows, W.rows.p, (size_t)n * root_cols, hipMemcpyDeviceToHost));
    return SMX_OK;
}
}  // namespace

int smx_msa_debug_times(float *level_ms, uint32_t cap_levels, uint32_t *n_levels, float tips_rows_ms[2], double phase_us[3]) {
    if (!n_levels || !tips_rows_ms || !phase_us || (cap_levels && !level_ms)) return fail(SMX_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> guard(g_msa.mutex);
    auto &W = g_msa;
    if (!W.clock_khz) {
        SMX_TRY(require_device());
        if (hipDeviceGetAttribute(&W.clock_khz, hipDeviceAttributeWallClockRate, 0) != hipSuccess || W.clock_khz <= 0)
            W.clock_khz = 100000;                 // gfx9's constant 100 MHz
    }
    *n_levels = (uint32_t)W.level_ms.size();
    for (uint32_t v = 0; v < *n_levels && v < cap_levels; v++) level_ms[v] = W.level_ms[v];
    tips_rows_ms[0] = W.tips_ms;
    tips_rows_ms[1] = W.rows_ms;
    for (int k = 0; k < 3; k++) phase_us[k] = (double)W.phase_ticks[k] * 1000.0 / (double)W.clock_khz;
    return SMX_OK;
}

int smx_msa(const char *seqs, const uint64_t *off, uint32_t n, const smx_msa_merge *merges, uint32_t mismatch, uint32_t gap,
            uint32_t cap_cols, uint8_t *rows, uint32_t *n_cols, uint32_t *lens, uint64_t *costs, float *kernel_ms) {
    return msa_call(seqs, off, n, merges, mismatch, gap, cap_cols, rows, n_cols, lens, costs, kernel_ms);
}

// ---- consensus: every member read of a job aligned to the job's draft with traceback, the rows reduced to votes
// (smx_cons.hip); a workspace of its own, like g_pairs, with the history of the workgroups in flight
namespace {
struct {
    std::mutex mutex;
    DevSeqs reads;
    DevBuf k, jobs, align, chunk_start;
    DevBuf scratch;             // per-lane state of the generic class, one slice per workgroup
    DevBuf hist_pm, hist_s;     // the alignment history, one slice per workgroup
    DevBuf rows, dist, votes, aligned;
    DevBuf planes_off, sites, n_sites, n_qualified, planes, link;   // smx_cons_phase (smx_phase.hip)
    DevBuf masks, member_off, agree_off, agree, sub_aligned;        // smx_cons_resample (smx_resample.hip)
    DevBuf quals, qoff, per_member, tables;                         // smx_cons_profile (smx_profile.hip)
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

struct ConsProfile {    // what smx_cons_profile adds to a votes call
    const unsigned char *quals;
    uint32_t *per_member, *tables;
};

// One smx_cons_* call.  rows / dist (pileup) or votes / aligned (votes) receive the result, the others are null; with
// `phase` a votes call goes on to the variant kernels over the rows and votes it left on the device, with `resample` to
// the resampling kernel over the rows and distances, with `profile` to the error-profile kernel over the same.
int cons_call(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k, const smx_cons_job *jobs,
              uint32_t n_jobs, uint32_t *rows, int32_t *dist, uint32_t *votes, uint32_t *aligned, float *kernel_ms,
              const ConsPhase *phase = nullptr, const ConsResample *resample = nullptr, const ConsProfile *profile = nullptr) {
    const bool pileup = rows || dist;
    if (!reads || !roff || !k || (n_jobs && (!jobs || (pileup ? !rows || !dist : !votes || !aligned))))
        return fail(SMX_ERR_ARG, "null argument");
    if (phase && n_jobs && (!phase->sites || !phase->n_sites || !phase->n_qualified || !phase->planes || !phase->link))
        return fail(SMX_ERR_ARG, "null argument");
    if (resample && n_jobs && (!resample->agree || !resample->sub_aligned)) return fail(SMX_ERR_ARG, "null argument");
    uint64_t hist_budget = smx::CONS_HIST_BYTES;
    if (const char *env = getenv("SMX_CONS_HIST_BYTES")) hist_budget = strtoull(env, nullptr, 10);   // test hook: few workgroups in flight
    smx::ConsPlan P;
    std::string why;
    int rc = smx::cons_plan(reads, roff, n_reads, k, jobs, n_jobs, hist_budget, &P, &why);
    if (rc == SMX_OK && phase) rc = smx::cons_plan_phase(phase->min_permille, phase->max_sites, &P, &why);
    if (rc == SMX_OK && resample) rc = smx::cons_plan_resample(resample->masks != nullptr, resample->n_levels, &P, &why);
    if (rc == SMX_OK && profile)
        rc = smx::cons_plan_profile(profile->quals != nullptr, profile->per_member != nullptr, profile->tables != nullptr, &P, &why);
    SMX_TRY(refused(rc, why));
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return SMX_OK;     // a call without jobs is answered without a device (the tests pin it): the one step out of order
    std::lock_guard<std::mutex> guard(g_cons.mutex);
    SMX_TRY(require_device());
    auto &W = g_cons;
    SMX_TRY(W.reads.upload(reads, roff, n_reads));
    HIP_TRY(W.k.upload(k, (size_t)n_reads * 4));
    HIP_TRY(W.jobs.upload(P.jobs));
    HIP_TRY(W.align.upload(P.align));
    HIP_TRY(W.chunk_start.upload(P.chunk_start));
    HIP_TRY(W.rows.ensure((size_t)P.rows_words * 4));
    HIP_TRY(W.dist.ensure((size_t)P.n_dist * 4));
    const uint64_t grid_max = P.grid_max();   // a history slice per workgroup of the largest launch
    HIP_TRY(W.hist_pm.ensure((size_t)(grid_max * P.hist_slice * MINE_THREADS * sizeof(smx::cons_pm))));
    HIP_TRY(W.hist_s.ensure((size_t)(grid_max * P.hist_slice * MINE_THREADS * sizeof(int))));
    SMX_TRY(ensure_scratch(&W.scratch, P));
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
    if (profile) {      // the quality bytes beside the reads, in the caller's layout
        HIP_TRY(W.quals.upload(profile->quals, P.n_dist ? (size_t)roff[n_reads] : 0));   // without members: may be null, never read
        HIP_TRY(W.qoff.upload(roff, ((size_t)n_reads + 1) * 8));
        HIP_TRY(W.per_member.ensure((size_t)P.member_words * 4));
        HIP_TRY(W.tables.ensure((size_t)P.table_words * 4));
        HIP_TRY(hipMemset(W.tables.p, 0, (size_t)P.table_words * 4));   // the kernel adds into them
    }
    const int32_t *d_len = W.reads.len.as<int32_t>();
    SMX_TRY(timed_launches(kernel_ms, "consensus kernel launch", [&] {
        int e = smx::chunk_for_each_class(P, [&](const smx::ChunkLaunch &L) {
            return smx_launch_cons_align(nullptr, L.wr, W.reads.bytes.as<unsigned char>(), W.reads.doff.as<uint64_t>(), d_len,
                                         W.k.as<int32_t>(), W.align.as<smx::ConsJobDev>() + L.rec_at,
                                         W.chunk_start.as<uint64_t>() + L.start_at, L.n, L.grid, L.per_block, L.lds,
                                         W.rows.as<uint32_t>(), W.dist.as<int32_t>(), W.hist_pm.p, W.hist_s.as<int>(), P.hist_slice,
                                         W.scratch.as<unsigned long long>(), P.words_max0);
        });
        if (e == 0 && !pileup)
            e = smx_launch_cons_vote(nullptr, d_len, W.jobs.p, n_jobs, P.max_words, W.rows.as<uint32_t>(),
                                     W.dist.as<int32_t>(), W.votes.as<uint32_t>(), W.aligned.as<uint32_t>());
        if (e == 0 && phase)
            e = smx_launch_cons_phase(nullptr, d_len, W.jobs.p, n_jobs, W.rows.as<uint32_t>(), W.dist.as<int32_t>(),
                                      W.votes.as<uint32_t>(), W.aligned.as<uint32_t>(), phase->min_permille, phase->min_reads,
                                      phase->max_sites, P.max_plane_words, W.planes_off.as<uint64_t>(), W.sites.p,
                                      W.n_sites.as<uint32_t>(), W.n_qualified.as<uint32_t>(), W.planes.as<uint64_t>(),
                                      W.link.as<uint32_t>());
        if (e == 0 && resample)
            e = smx_launch_cons_resample(nullptr, W.reads.bytes.as<unsigned char>(), W.reads.doff.as<uint64_t>(), d_len, W.jobs.p,
                                         n_jobs, resample->n_levels, P.max_words, W.rows.as<uint32_t>(), W.dist.as<int32_t>(),
                                         W.masks.as<uint64_t>(), W.member_off.as<uint64_t>(), W.agree_off.as<uint64_t>(),
                                         P.member_off.back(), W.agree.as<uint64_t>(), W.sub_aligned.as<uint32_t>());
        if (e == 0 && profile)
            e = smx_launch_cons_profile(nullptr, W.reads.bytes.as<unsigned char>(), W.reads.doff.as<uint64_t>(), d_len, W.jobs.p,
                                        n_jobs, P.profile_max_members, W.rows.as<uint32_t>(), W.dist.as<int32_t>(),
                                        W.quals.as<unsigned char>(), W.qoff.as<uint64_t>(), W.per_member.as<uint32_t>(),
                                        W.tables.as<uint32_t>());
        return e;
    }));
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
    if (profile) {
        if (P.member_words) HIP_TRY(hipMemcpy(profile->per_member, W.per_member.p, (size_t)P.member_words * 4, hipMemcpyDeviceToHost));
        if (profile->tables) HIP_TRY(hipMemcpy(profile->tables, W.tables.p, (size_t)P.table_words * 4, hipMemcpyDeviceToHost));
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

int smx_cons_profile(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k, const smx_cons_job *jobs,
                     uint32_t n_jobs, const unsigned char *quals, uint32_t *votes, uint32_t *aligned, uint32_t *per_member,
                     uint32_t *tables, float *kernel_ms) {
    if (n_jobs && (!votes || !aligned)) return fail(SMX_ERR_ARG, "null argument");
    const ConsProfile profile{quals, per_member, tables};
    return cons_call(reads, roff, n_reads, k, jobs, n_jobs, nullptr, nullptr, votes, aligned, kernel_ms, nullptr, nullptr, &profile);
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
    SMX_TRY(refused(smx::inner_plan(patterns, poff, Q, k, margin, H, budget, smx::INNER_DEFAULT_BUDGET,
                                    smx::InnerAlphabet{code_of, build_peq}, &P, &why), why));
    std::lock_guard<std::mutex> guard(g_inner.mutex);
    SMX_TRY(require_device());
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_reads == 0) return SMX_OK;
    auto &W = g_inner;
    HIP_TRY(W.tables.upload(P.blob));
    smx::InnerGroup g;
    std::vector<unsigned char> stage, out;
    // groups of whole reads: everything one launch group keeps on the device fits the budget (one read always goes)
    for (uint32_t r0 = 0; r0 < n_reads; r0 = g.r1) {
        SMX_TRY(refused(P.next_group(len, n_reads, r0, &g, &why), why));
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
        float ms = 0.0f;
        SMX_TRY(timed_launches(kernel_ms ? &ms : nullptr, "inner scan launch", [&] {
            int e = 0;
            for (const smx::InnerClass &C : P.cls) {
                if (C.idx.empty() || g.units == 0 || e != 0) continue;
                A.peq = W.tables.as<char>() + C.peq_at;
                A.pm = (const int *)(W.tables.as<char>() + C.tab_at);
                A.pk = A.pm + C.slots();
                A.jmap = A.pm + 2 * C.slots();
                e = smx_launch_inner_scan(nullptr, C.w64, C.G, C.npass, &A);
            }
            return e ? e : smx_launch_inner_merge(nullptr, &A, nr, d_nh, d_hd, d_he);
        }));
        if (kernel_ms) *kernel_ms += ms;
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
